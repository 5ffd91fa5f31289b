"""Per-launch float64 reference and per-element error gate for the conv stack (test helper, no GPU).

The launches of an arena plan that keep a layer's output on chip (tail and chain GEMMs, the stem's PAIR form) have no reference here: they
are gated by equality, tensor by tensor, to a plan of stand-alone launches that passes THIS gate in the same test
(tests/test_gpu_fused_plan.py; VNECT_KEEP_FUSED=1 builds them on private buffers), which carries the bounds below over to them.

Every tensor a keep_activations handle can return is checked ON ITS OWN: its reference is computed in float64 from the
device's own input tensors (exact fp32 widenings of what the device holds), so no error of an earlier layer reaches it, and
every output element is held to a bound on what the launch's arithmetic may owe -- no allowance for a fraction of elements.

Notation, per output element: y = the exact (float64) result of the launch's epilogue on the device inputs, d = |gpu - y|,
A = the same sum on absolute values (sum |x||w| + |bias| + |shortcut|; BN columns |scale| (sum |x||w| + |bias|) + |shift|),
K = the true reduction length, u = 2^-24 (fp32 round to nearest even), ub = 2^-8 (bf16 round to nearest even).

fp32 accumulation term E (every order of summation, every tile shape, split-K):
  * rigorous:   E = gamma(n) u A / u,  gamma(n) = n u / (1 - n u),  n = K + 2 (K + 3 on the BN columns: bias, scale, shift).
    This holds for any order of the K products and the epilogue's additions (Higham, Accuracy and Stability of Numerical
    Algorithms, 3.1), and it is loose: K runs to 4608, measured errors stay below 8 u A.
  * calibrated: E = C_CAL u A, one constant for the whole suite, set from the worst d / (u A) measured on an MI355X (see C_CAL).
fp32 output:  d <= E.
bf16 output (every tensor of a bf16 handle but the final maps): the launch computes v with |v - y| <= E in fp32, applies ReLU
(1-Lipschitz) and rounds once to bf16: |RNE(v) - v| <= ub |v| <= ub (|y| + E), so d <= ub |y| + (1 + ub) E.
Split-product launches (VNECT_FP32_SPLIT, conv.hip "X3"; hostplan.h split3 / pack_split3): the activation x is cut by truncation
into bf16 pieces xh + xm + xl = x EXACTLY (8 + 8 + 8 significand bits), |xm| < 2^-7 |x|, |xl| < 2^-14 |x|, all of x's sign; the
weight w into RNE pieces, w = wh + wm + wl + r3 with |w - wh| <= ub |w|, |wm| <= 2^-8 (1 + 2^-8) |w|, |wl| <= 2^-16 (1 + 2^-8) |w|,
|r3| <= 2^-24 |w|.  The kernel sums the six products xh wh, xh wm, xm wh, xh wl, xl wh, xm wm (each exact in fp32) and drops
    |xm wl| + |xl wm| + |xl wl| + |x r3| <= (2 + 4 + 2^-6 + 1)(1 + 2^-8) u |x||w| <= SPLIT_DROP u |x||w|.
The six kept products have sum of magnitudes <= |x| (|wh| + |wm| + |wl|) <= SPLIT_KEEP |x||w|, and there are 6K of them:
    E_split = (rigorous: gamma(6K + 2); calibrated: C_CAL u) SPLIT_KEEP A + SPLIT_DROP u sum |x||w|.
Bone lengths (res5c_branch2a_feat columns 191..211, computed from the device's stored deltas): sqrt((x x + y y) + z z) in fp32 is
within 2.5 u of the exact value (three roundings of a sum of positive terms, halved by the square root, one more): n = 3, A = y,
in both tiers.
pool1 and input are exact: pool1 == the max over the device's own conv1 (SAME, -inf padding), input == the batch (bf16: its RNE).

Sharpness (bf16 tensors): over elements with y != 0, the fraction where gpu == RNE_bf16(float32(y)) must reach MATCH_FLOOR.  A
launch that truncates, or rounds twice, lands near 1/2 (tests/test_layer_bounds_cpu.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
UB = 2.0 ** -8
# Calibrated fp32 accumulation constant, one for every precision, launch form and tile shape: the worst d / (u A) measured on an
# MI355X over the 48 configurations of tests/test_gpu_layer_bounds.py is 7.21 (fp32, six scales, res2a_branch2b; split-product
# 6.05 at conv1; bf16 1.91 on its fp32 final maps), the CPU stand-in's torch fp32 7.4.  C_CAL leaves 3.9x headroom over the GPU.
# The six configurations of the paper wiring stay below it: 6.54 (fp32, one scale, res5a_branch1_new), split-product 6.05, bf16 1.54.
# The weight families of tests/weight_families.py (tests/test_gpu_weight_families.py) reach further: 15.0 on res5c_branch2b under signed_bn
# (fp32, three scales, whole-K 64 x 64 tiles; the CPU stand-in's torch fp32 12-17 on the same tensor over six seeds).  There a few BN columns of folded
# scale near 31.6 carry A, so the running sum sits at A's size while K = 1908 small terms are added to it, each rounding at that size; on
# He-uniform data the partial sums grow like a random walk and stay small.  Every other family stays below 12; C_CAL keeps 1.9x over it.
MEASURED_CAL = 7.21
C_CAL = 28.0
# bf16 match fraction: lowest measured on an MI355X 0.99968 (the paper wiring at the baseline scales, res3a_branch2b; the default
# wiring's lowest is 0.99975: res5a_branch2b_new, forced 64x64 tiles); the planted faults of tests/test_layer_bounds_cpu.py give 0.50
# (truncating store) to 0.990 (one border row misread).
MEASURED_MATCH = 0.99968
MATCH_FLOOR = 0.999
SPLIT_KEEP = 1.008
SPLIT_DROP = 7.03
BONE_N = 3


def _round_bf16(a):
    from tests.gpu_common import _round_bf16 as r
    return r(a)


def table(paper_res2c=False):
    """Tensor name -> (op, input tensor names, params) for every readable tensor of a keep_activations plan, in launch order
    (vnect_model.py:25-217 as restated in tests/torch_net.py).  paper_res2c=False: the default wiring, res2c_branch2b reads
    res2b_branch2a and res2c_branch2a does not exist; True: vnect_config::paper_res2c = 1, res2c_branch2a = conv1x1(res2b) sits right
    behind res2b and res2c_branch2b reads it.  op: 'input', 'conv' (inputs [x] or [x, shortcut]: a block output
    resNx is its branch2c conv + shortcut, ReLU), 'pool', 'feat' (transposed convs + BN + ReLU | deltas | bone lengths), 'head'."""
    T = {"input": ("input", [], {})}

    def conv(name, x, k, stride=1, relu=True, scope=None, resid=None):
        T[name] = ("conv", [x] + ([resid] if resid else []), dict(scope=scope or name, k=k, stride=stride, relu=relu))

    def proj(p, x, stride):
        conv(p + "_branch2a", x, 1, stride)
        conv(p + "_branch1", x, 1, stride, relu=False)
        conv(p + "_branch2b", p + "_branch2a", 3)
        conv(p, p + "_branch2b", 1, scope=p + "_branch2c", resid=p + "_branch1")

    def ident(p, x, a=None):
        if a is None:
            conv(p + "_branch2a", x, 1)
            a = p + "_branch2a"
        conv(p + "_branch2b", a, 3)
        conv(p, p + "_branch2b", 1, scope=p + "_branch2c", resid=x)

    conv("conv1", "input", 7, 2)
    T["pool1"] = ("pool", ["conv1"], {})
    proj("res2a", "pool1", 1)
    ident("res2b", "res2a")
    if paper_res2c:
        ident("res2c", "res2b")
    else:
        ident("res2c", "res2b", a="res2b_branch2a")  # vnect_model.py:56: res2c_branch2b reads res2b_branch2a
    proj("res3a", "res2c", 2)
    for p, x in (("res3b", "res3a"), ("res3c", "res3b"), ("res3d", "res3c")):
        ident(p, x)
    proj("res4a", "res3d", 2)
    for p, x in (("res4b", "res4a"), ("res4c", "res4b"), ("res4d", "res4c"), ("res4e", "res4d"), ("res4f", "res4e")):
        ident(p, x)
    conv("res5a_branch2a_new", "res4f", 1)
    conv("res5a_branch1_new", "res4f", 1, relu=False)
    conv("res5a_branch2b_new", "res5a_branch2a_new", 3)
    conv("res5a", "res5a_branch2b_new", 1, scope="res5a_branch2c_new", resid="res5a_branch1_new")
    conv("res5b_branch2a_new", "res5a", 1)
    conv("res5b_branch2b_new", "res5b_branch2a_new", 3)
    conv("res5b_branch2c_new", "res5b_branch2b_new", 1)
    # (the bone columns read the device's own stored deltas: the feat tensor is an input of its own reference)
    T["res5c_branch2a_feat"] = ("feat", ["res5b_branch2c_new", "res5c_branch2a_feat"], {})
    conv("res5c_branch2b", "res5c_branch2a_feat", 3)
    T["res5c_branch2c"] = ("head", ["res5c_branch2b"], {})
    return T


TABLE = table()
TABLE_PAPER = table(paper_res2c=True)


def launch_tensors(name, stem=False, pair=False, table=TABLE):
    """Tensors a launch of h.layers() writes (the names test_conv_stack_every_layer derives), under the wiring of `table` (TABLE or
    TABLE_PAPER).  Raises KeyError on a launch form this module does not know under that wiring, so that a new one -- or one that
    belongs to the other wiring -- cannot escape the gate.  stem: the fused stem stands for conv1 + pool1; pair: in
    its PAIR form, which runs res2a_branch2a + res2a_branch1 on the pooled tile and stores neither conv1 nor pool1.
    Fused launches "<3x3 scope>><1x1 scope>[><next branch2a>]" (rt_plan.cpp add_conv_tail) store the block output (the head: the final
    maps) and, chained, the next block's branch2a; the 3x3 layer's output stays in LDS."""
    if stem and name in ("conv1", "pool1"):  # the fused stem writes pool1 only; it is checked from `input`
        return ["res2a_branch2a", "res2a_branch1"] if pair else ["pool1"]
    if ">" in name:
        parts = name.split(">")
        b, c = parts[0], parts[1]
        if len(parts) > 3 or not b.endswith("_branch2b") or c != b[:-1] + "c" or (len(parts) == 3 and not parts[2].endswith("_branch2a")):
            raise KeyError("launch %r: not a tail or chain form this module knows" % name)
        out = [c if c == "res5c_branch2c" else c.split("_")[0]] + parts[2:]
        if len(parts) == 3 and (table.get(parts[2], (None, [None]))[1][0] != out[0]):
            raise KeyError("launch %r: the chained layer does not read the block output" % name)
    elif name in ("res5c_deconv", "res5c_deconv+bone_length", "res5c_bone_length"):
        out = ["res5c_branch2a_feat"]
    elif "[" in name:                           # "<scope>[:N]": head split of a paired launch
        out = [name.split("[")[0]]
    elif "+" in name:                         # "<scope_a>+<rest of scope_b>"
        a, b = name.split("+")
        out = [a, b if b.startswith("res") else a.split("_")[0] + "_" + b]
        if all(t in table for t in out) and table[out[0]][1][:1] != table[out[1]][1][:1]:
            raise KeyError("launch %r: its two layers do not read the same tensor" % name)
    elif name == "res5c_branch2c":
        out = [name]
    elif name.endswith("_branch2c") or name == "res5a_branch2c_new":
        out = [name.split("_")[0]]
    else:
        out = [name]
    for t in out:
        if t not in table or table[t][0] == "input":
            raise KeyError("launch %r: no per-element gate for tensor %r" % (name, t))
    return out


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _same(x, k, stride, value=0.0):
    def lohi(n):
        total = max((-(-n // stride) - 1) * stride + k - n, 0)
        return total // 2, total - total // 2
    (t, b), (l, r) = lohi(x.shape[2]), lohi(x.shape[3])
    return F.pad(x, (l, r, t, b), value=value)


def maxpool_same(x):
    """pool1 (vnect_model.py:29, 3x3 stride 2 SAME): NCHW tensor, -inf padding."""
    return F.max_pool2d(_same(x, 3, 2, float("-inf")), 3, 2)


def layer_weights(weights, prec):
    """The weights as the device multiplies them: bf16 handles round every conv / transposed-conv weight to nearest even
    (rt_plan.cpp upload_weights); biases and the BN parameters stay fp32."""
    if prec != "bf16":
        return weights
    return {k: (_round_bf16(v) if k.endswith("/weights") or k.endswith("/kernel") else v) for k, v in weights.items()}


def fold_bn(weights):
    """bias, scale, shift of the 128 BN columns exactly as plan::fold_bn computes them in fp32."""
    g, be, mu, va = (np.asarray(weights["bn5c_branch2a/" + n], np.float32) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
    scale = g * (np.float32(1.0) / np.sqrt(va + np.float32(0.001)))
    return -mu, scale.astype(np.float32), be


def _conv_ref(x, xa, w, b, k, stride):
    wt = torch.from_numpy(np.asarray(w)).to(torch.float64).permute(3, 2, 0, 1)
    bt = torch.from_numpy(np.asarray(b)).to(torch.float64).view(1, -1, 1, 1)
    if k > 1:
        x, xa = _same(x, k, stride), _same(xa, k, stride)
    return F.conv2d(x, wt, stride=stride) + bt, F.conv2d(xa, wt.abs(), stride=stride) + bt.abs()


def reference(name, acts, lw, table=TABLE):
    """float64 reference of one tensor of `table` from the device's input tensors `acts` (name -> NHWC float32) and the layer weights
    `lw` (layer_weights).  Returns dict(y, A, dot, K, epi, cal_n) -- arrays NHWC, K / epi / cal_n per channel (cal_n: a fixed
    coefficient that replaces C_CAL, NaN where C_CAL applies) -- or dict(exact=array) for pool1."""
    op, ins, p = table[name]
    if op == "pool":
        return dict(exact=_nhwc(maxpool_same(_t64(acts[ins[0]]))))
    if op == "conv" or op == "head":
        x = _t64(acts[ins[0]])
        if op == "head":
            w = lw["res5c_branch2c/kernel"]
            b = np.zeros(w.shape[3], np.float32)
            k, stride, relu, cin = 1, 1, False, w.shape[2]
        else:
            w, b = lw[p["scope"] + "/weights"], lw[p["scope"] + "/biases"]
            k, stride, relu, cin = p["k"], p["stride"], p["relu"], w.shape[2]
        y, A = _conv_ref(x, x.abs(), w, b, k, stride)
        dot = A - torch.from_numpy(np.abs(np.asarray(b))).to(torch.float64).view(1, -1, 1, 1)
        if len(ins) > 1:
            s = _t64(acts[ins[1]])
            y, A = y + s, A + s.abs()
        if relu:
            y = F.relu(y)
        C = y.shape[1]
        return dict(y=_nhwc(y), A=_nhwc(A), dot=_nhwc(dot), K=np.full(C, k * k * cin, np.float64), epi=np.full(C, 2.0),
                    cal_n=np.full(C, np.nan))
    if op == "feat":
        x = _t64(acts[ins[0]])
        xa = x.abs()
        parts_y, parts_A, parts_dot = [], [], []
        for scope in ("res5c_branch2a", "res5c_branch1a"):  # BN columns 0..127, then the deltas 128..190
            w = torch.from_numpy(np.asarray(lw[scope + "/kernel"])).to(torch.float64).permute(3, 2, 0, 1)
            d = F.conv_transpose2d(x, w, stride=2, padding=1)
            da = F.conv_transpose2d(xa, w.abs(), stride=2, padding=1)
            if scope == "res5c_branch2a":
                bias, scale, shift = (torch.from_numpy(np.asarray(v, np.float64)).view(1, -1, 1, 1) for v in fold_bn(lw))
                parts_y.append(F.relu((d + bias) * scale + shift))
                parts_A.append(scale.abs() * (da + bias.abs()) + shift.abs())
                parts_dot.append(scale.abs() * da)
            else:
                parts_y.append(d), parts_A.append(da), parts_dot.append(da)
        f = acts[ins[1]]  # the device's stored deltas (bf16 handles: bf16 values) -> bone lengths
        dx, dy, dz = (f[..., 128 + 21 * i:149 + 21 * i].astype(np.float64) for i in range(3))
        bone = np.sqrt(dx * dx + dy * dy + dz * dz)
        y = np.concatenate([_nhwc(torch.cat(parts_y, 1)), bone], -1)
        A = np.concatenate([_nhwc(torch.cat(parts_A, 1)), bone], -1)
        dot = np.concatenate([_nhwc(torch.cat(parts_dot, 1)), np.zeros_like(bone)], -1)
        K = np.concatenate([np.full(191, 4.0 * x.shape[1]), np.zeros(21)])
        epi = np.concatenate([np.full(128, 3.0), np.full(63, 2.0), np.full(21, BONE_N)])
        cal_n = np.concatenate([np.full(191, np.nan), np.full(21, float(BONE_N))])
        return dict(y=y, A=A, dot=dot, K=K, epi=epi, cal_n=cal_n)
    raise ValueError(name)


def _gamma_over_u(n):
    return n / (1.0 - n * U)


def bounds(r, bf16_out, split=False):
    """Per-element bounds of a reference r (reference()) for the two tiers: (rigorous, calibrated)."""
    y, A, K, epi, cal_n = r["y"], r["A"], r["K"], r["epi"], r["cal_n"]
    if split:
        n = 6.0 * K + epi
        A = A * np.where(K > 0, SPLIT_KEEP, 1.0)
        drop = SPLIT_DROP * U * r["dot"]
    else:
        n, drop = K + epi, 0.0
    out = []
    for coef in (_gamma_over_u(n), np.where(np.isnan(cal_n), C_CAL, cal_n)):
        E = coef * U * A + drop
        out.append(UB * np.abs(y) + (1.0 + UB) * E if bf16_out else E)
    return out


def _ratio(d, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / b)
    return float(q.max()) if q.size else 0.0


def _implied_c(d, r, bf16_out, split):
    """The smallest calibrated constant under which these elements pass: max (d - rounding - dropped) / (keep u A) over the
    elements whose accumulation term is calibrated (for calibrating C_CAL; 0 where the output rounding covers all of d)."""
    y, A, cal = r["y"], r["A"], np.isnan(r["cal_n"])
    drop = SPLIT_DROP * U * r["dot"] if split else 0.0
    keep = SPLIT_KEEP if split else 1.0
    if bf16_out:
        num = d - UB * np.abs(y) - (1.0 + UB) * drop
        den = (1.0 + UB) * keep * U * A
    else:
        num, den = d - drop, keep * U * A
    sel = np.broadcast_to(cal, y.shape) & (den > 0)
    return float(max(0.0, (num[sel] / den[sel]).max())) if sel.any() else 0.0


def check_tensor(name, gpu, r, bf16_out, split=False):
    """One tensor's row: worst d / bound per tier, the implied calibration constant, the bf16 match fraction, and ok."""
    if "exact" in r:
        eq = bool(np.array_equal(gpu, r["exact"]))
        return dict(tensor=name, rig=0.0 if eq else float("inf"), cal=0.0 if eq else float("inf"), c=None, match=None, ok=eq)
    y = r["y"]
    assert gpu.shape == y.shape, (name, gpu.shape, y.shape)
    d = np.abs(gpu.astype(np.float64) - y)
    rig_b, cal_b = bounds(r, bf16_out, split)
    rig, cal = _ratio(d, rig_b), _ratio(d, cal_b)
    match = None
    if bf16_out:
        nz = y != 0
        match = float(np.mean(gpu[nz] == _round_bf16(y[nz].astype(np.float32)))) if nz.any() else 1.0
    ok = rig <= 1.0 and cal <= 1.0 and (match is None or match >= MATCH_FLOOR)
    return dict(tensor=name, rig=rig, cal=cal, c=_implied_c(d, r, bf16_out, split), match=match, ok=ok)


def stem_pool_reference(acts, lw):
    """pool1 of a fused-stem launch (stem.hip: conv1 + ReLU -> max-pool, conv1 never stored): the 3x3 window maximum of the
    float64 conv1 from `input`.  RNE is monotone, so the max and the rounding commute, and the bound of a window maximum is the
    largest element bound in the window (|max a - max b| <= max |a - b|)."""
    r = reference("conv1", acts, lw)
    y = _nhwc(maxpool_same(_t64(r["y"])))
    return r, y


def check_all(acts, weights, prec, batch, stem=False, split_tensors=(), table=TABLE):
    """Gate every tensor of `table` present in `acts` (name -> NHWC float32 as read from the device).  prec: 'fp32', 'bf16' or
    'fp32_split'; batch: the (S,368,368,3) input the forward ran on; stem: the fused stem wrote pool1 (conv1 is not checked);
    split_tensors: tensors written by a split-product launch.  Returns the rows (check_tensor), input first."""
    bf = prec == "bf16"
    lw = layer_weights(weights, prec)
    rows = []
    want_in = _round_bf16(batch) if bf else np.asarray(batch, np.float32)
    eq = bool(np.array_equal(acts["input"], want_in))
    rows.append(dict(tensor="input", rig=0.0 if eq else float("inf"), cal=0.0 if eq else float("inf"), c=None, match=None, ok=eq))
    for name in table:
        if name == "input" or name not in acts or (stem and name == "conv1"):
            continue
        bf_out = bf and name != "res5c_branch2c"
        if stem and name == "pool1":
            r, y = stem_pool_reference(acts, lw)
            rig_b, cal_b = (_nhwc(maxpool_same(_t64(b))) for b in bounds(r, bf_out))
            gpu = acts["pool1"]
            d = np.abs(gpu.astype(np.float64) - y)
            rig, cal = _ratio(d, rig_b), _ratio(d, cal_b)
            match = None
            if bf_out:
                nz = y != 0
                match = float(np.mean(gpu[nz] == _round_bf16(y[nz].astype(np.float32))))
            rows.append(dict(tensor="pool1", rig=rig, cal=cal, c=None, match=match,
                             ok=rig <= 1.0 and cal <= 1.0 and (match is None or match >= MATCH_FLOOR)))
            continue
        r = reference(name, acts, lw, table)
        rows.append(check_tensor(name, acts[name], r, bf_out, split=name in split_tensors))
    return rows
