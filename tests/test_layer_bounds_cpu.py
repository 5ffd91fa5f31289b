"""The per-element gate of tests/layer_ref.py is not vacuous (CPU, no GPU needed).

A CPU stand-in for the device computes every tensor of a keep_activations plan from its inputs the way the HIP launches do:
torch float32 accumulation, bf16 round-to-nearest-even at the kernels' rounding points (every stored activation of a bf16 handle
but the fp32 final maps), the BN scale / shift of plan::fold_bn, the bone lengths from the stored deltas.  The clean stand-in must
pass the gate on every tensor in fp32 and in bf16; each planted fault must fail it on exactly the tensor it was planted in (the
stand-in recomputes everything behind a fault from the faulty tensor, as a device would, so only that tensor's own launch is
wrong).  One scale at 368 x 368, synthetic weights.

The fused launches of the product plan (rt_plan.cpp: tails, chains, the stem's PAIR form) are gated on the device by equality to the
stand-alone plan, tensor by tensor (tests/test_gpu_fused_plan.py).  Here the stand-in has a fused mode: the same arithmetic at the
kernels' rounding points (conv.hip tail_gemm / tail_wide: the 3x3 layer's relu(acc + bias) goes to LDS in the activations' type and is
never stored; chain_gemm / chain_narrow read the block output from LDS as it is stored, rounded; stem.hip: the pooled tile in the
activations' type, conv1 and pool1 never stored).  Clean, it must equal the plain stand-in on every tensor it stores; each planted
fused-launch fault must break that equality first -- in launch order -- on the tensor its launch writes.

Both wirings of res2c (vnect_config::paper_res2c; layer_ref.TABLE and TABLE_PAPER) go through all of this: the stand-in takes the wiring,
the clean one passes the table of that wiring, a stand-in that runs the OTHER wiring's res2c_branch2b fails on exactly that tensor, and the
paper plan's own chain launch (res2b_branch2b>res2b_branch2c>res2c_branch2a: an identity shortcut, rows of 64) has its planted faults.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers, layer_ref
from tests.layer_ref import TABLE, TABLE_PAPER

# fault -> (tensor, precision).  (a) truncating store, (b) bias lost on 4 channels of a 1x1 layer, (c) the first 64-element K chunk
# lost in the last tile (64 output pixels) of a 3x3 layer, (d) a block output rounded before the shortcut add and again after it,
# (e) a 3x3 layer's top output row read without its SAME padding row (image rows 0..2 instead of pad, 0, 1), (f) one low-magnitude
# channel of an fp32 layer 1e-3 off
FAULTS = {
    "truncate": ("res4b_branch2a", "bf16"),
    "bias": ("res3b_branch2a", "bf16"),
    "kchunk": ("res4b_branch2b", "bf16"),
    "double_round": ("res3c", "bf16"),
    "pad_row": ("res2b_branch2b", "bf16"),
    "channel": ("res5a_branch1_new", "fp32"),
}
# wiring fault -> (tensor, precision, the wiring the device was asked for).  (a) asked for the paper wiring, res2c_branch2b still reads
# res2b_branch2a (the switch ignored behind a correct res2c_branch2a), (b) asked for the default wiring, res2c_branch2b reads a
# res2c_branch2a that the plan should have pruned (the switch crossed)
WIRING_FAULTS = {
    "wiring_ignored": ("res2c_branch2b", "bf16", True),
    "wiring_crossed": ("res2c_branch2b", "fp32", False),
}

# Faults that no tensor notices under synthetic_weights() -- they need weights the default family never draws -- and that fail on exactly
# their own tensor under a family of tests/weight_families.py (tests/test_weight_families_cpu.py asserts both halves):
# fault -> (tensor, precision, family).  (a) the BN epilogue multiplies by |scale| (the default gamma is positive), (b) an output
# channel whose filter is all zeros is skipped together with its bias and comes out 0 (the default weights have no zero filter)
FAMILY_FAULTS = {
    "bn_abs": ("res5c_branch2a_feat", "fp32", "signed_bn"),
    "dead_skip": ("res3b_branch2a", "bf16", "dead"),
}


# The fused launches of the one-scale bf16 product plan (h.layers() names; VNECT_FORCE_CHAIN gives fp32 the wide chains too), and the
# stem in its PAIR form
FUSED_LAUNCHES = ["res2a_branch2b>res2a_branch2c>res2b_branch2a", "res2b_branch2b>res2b_branch2c", "res2c_branch2b>res2c_branch2c",
                  "res3a_branch2b>res3a_branch2c>res3b_branch2a", "res3b_branch2b>res3b_branch2c>res3c_branch2a",
                  "res3c_branch2b>res3c_branch2c>res3d_branch2a", "res3d_branch2b>res3d_branch2c", "res5c_branch2b>res5c_branch2c"]
HIDDEN = {"conv1", "pool1"} | {n.split(">")[0] for n in FUSED_LAUNCHES}
# ... and of the paper wiring's plan: res2b's tail chains res2c_branch2a (rt_plan.cpp, the paper_res2c block); the same tensors stay on chip
FUSED_LAUNCHES_PAPER = [FUSED_LAUNCHES[0], "res2b_branch2b>res2b_branch2c>res2c_branch2a"] + FUSED_LAUNCHES[2:]
assert HIDDEN == {"conv1", "pool1"} | {n.split(">")[0] for n in FUSED_LAUNCHES_PAPER}
# fused-launch fault -> (the first tensor, in launch order, that differs from the plain stand-in; precision).  (a) the tail GEMM's bias
# lost on 4 channels, (b) the 3x3 layer's tile put into LDS without its ReLU, (c) the shortcut rows of the last, partial tile (M = 2116 =
# 66 x 32 + 4) read one row further down, (d) the second half of the tail's K = 64 lost for the column block 32..63, (e) the PAIR form's
# pool windows at the right border reading on into the next row's first pixel instead of the -inf padding column (a zero there would
# hide behind conv1's ReLU), (f) a chain GEMM reading the block output before its 16-bit rounding
FUSED_FAULTS = {
    "tail_bias": ("res3b", "bf16"),
    "inner_relu": ("res3c", "fp32"),
    "resid_row": ("res3d", "bf16"),
    "half_k": ("res2c", "fp32"),
    "pair_pad": ("res2a_branch2a", "fp32"),
    "chain_unrounded": ("res3b_branch2a", "bf16"),
}
# the paper plan's chain launch: (f) on the layer it chains, (c) on its identity shortcut -- the narrow tail's tiles have 64 rows, M = 8464 =
# 132 x 64 + 16
FUSED_FAULTS_PAPER = {
    "chain_unrounded": ("res2c_branch2a", "bf16"),
    "resid_row": ("res2b", "bf16"),
}


def _trunc_bf16(t):
    return (t.view(torch.int32) & -65536).view(torch.float32)


def _rne_bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _low_channel(y):
    """the channel with the smallest nonzero maximum of |y| (NCHW)"""
    m = y.abs().amax(dim=(0, 2, 3))
    m = torch.where(m > 0, m, torch.full_like(m, float("inf")))
    return int(torch.argmin(m))


def device_forward(weights, batch, prec, fault=None, fused=False, paper=False):
    """Every tensor of TABLE (paper: of TABLE_PAPER; name -> NHWC float32 numpy) as a device with fp32 accumulation computes it; fault: a
    key of FAULTS, of WIRING_FAULTS or of FAMILY_FAULTS.  fused: as the launches of FUSED_LAUNCHES (FUSED_LAUNCHES_PAPER) and the PAIR stem compute them --
    the tensors of HIDDEN stay on chip and are not returned; fault: a key of FUSED_FAULTS (FUSED_FAULTS_PAPER)."""
    bf = prec == "bf16"
    lw = layer_ref.layer_weights(weights, prec)
    faults = ((FUSED_FAULTS_PAPER if paper else FUSED_FAULTS) if fused else
              {k: v for k, v in WIRING_FAULTS.items() if v[2] == paper} if fault in WIRING_FAULTS else
              FAMILY_FAULTS if fault in FAMILY_FAULTS else FAULTS)
    assert fault is None or fault in faults, (fault, fused, paper)
    target = faults[fault][0] if fault else None
    # the graph the device runs: the asked wiring's table, but for the two wiring faults
    graph = dict(TABLE_PAPER if paper or fault == "wiring_crossed" else TABLE)
    if fault == "wiring_ignored":
        graph[target] = (graph[target][0], ["res2b_branch2a"], graph[target][2])
    tile = 64 if target and target.startswith("res2") else 32   # rows of a tail launch's tile: narrow (92x92 stage) 64, wide 32
    T = {}
    RAW = {}   # a block output as the tail GEMM's epilogue holds it, before the store rounds it
    info = {}

    def f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32))

    def store(name, v, f32_out=False):
        RAW[name] = v
        if bf and not f32_out:
            v = _trunc_bf16(v) if (fault == "truncate" and name == target) else _rne_bf16(v)
        T[name] = v

    def same(x, k, stride, top=None):
        def lohi(n):
            total = max((-(-n // stride) - 1) * stride + k - n, 0)
            return total // 2, total - total // 2
        (t, b), (l, r) = lohi(x.shape[2]), lohi(x.shape[3])
        if top is not None:
            t, b = top, t + b - top
        return F.pad(x, (l, r, t, b))

    for name, (op, ins, p) in graph.items():
        if op == "input":
            x = f32(batch).permute(0, 3, 1, 2)
            T[name] = _rne_bf16(x) if bf else x
        elif op == "pool":
            x = T[ins[0]]
            if fault == "pair_pad":   # the right padding column holds the next row's first pixel (the last row's: the slack's zero)
                nxt = torch.cat([x[:, :, 1:, :1], torch.zeros_like(x[:, :, :1, :1])], 2)
                T[name] = F.max_pool2d(F.pad(torch.cat([x, nxt], 3), (0, 0, 0, 1), value=float("-inf")), 3, 2)
            else:
                T[name] = layer_ref.maxpool_same(x)
        elif op in ("conv", "head"):
            x = T[ins[0]]
            if op == "head":
                w, b, k, stride, relu = lw["res5c_branch2c/kernel"], np.zeros(84, np.float32), 1, 1, False
            else:
                w, b = lw[p["scope"] + "/weights"], np.array(lw[p["scope"] + "/biases"], np.float32)
                k, stride, relu = p["k"], p["stride"], p["relu"]
            if fault == "chain_unrounded" and name == target:
                x = RAW[ins[0]]
            if fault == "inner_relu" and name == graph[target][1][0]:
                relu = False
            if fault in ("bias", "tail_bias") and name == target:
                b = b.copy()
                b[:4] = 0
            wt = f32(w).permute(3, 2, 0, 1)
            if fault == "half_k" and name == target:
                wt = wt.clone()
                wt[32:64, wt.shape[1] // 2:] = 0
            acc = F.conv2d(same(x, k, stride) if k > 1 else x, wt, stride=stride)
            if fault == "kchunk" and name == target:   # the last tile's rows without K chunk 0 (tap (0,0), channels 0..63)
                wc = wt.clone()
                wc[:, :64, 0, 0] = 0
                tail = F.conv2d(same(x, k, stride), wc, stride=stride)
                S, C, H, W = acc.shape
                a2 = acc.permute(0, 2, 3, 1).reshape(-1, C).clone()
                a2[-64:] = tail.permute(0, 2, 3, 1).reshape(-1, C)[-64:]
                acc = a2.reshape(S, H, W, C).permute(0, 3, 1, 2)
            if fault == "pad_row" and name == target:  # output row 0 with no padding row above the image (both below it)
                acc = acc.clone()
                acc[:, :, 0] = F.conv2d(same(x, k, stride, top=0), wt, stride=stride)[:, :, 0]
            v = acc + f32(b).view(1, -1, 1, 1)
            if len(ins) > 1:
                if fault == "double_round" and name == target:
                    v = _rne_bf16(v)
                s = T[ins[1]]
                if fault == "resid_row" and name == target:   # rows of the last, partial tile: the shortcut of the row below
                    S, C, H, W = s.shape
                    s2 = s.permute(0, 2, 3, 1).reshape(-1, C).clone()
                    m0 = s2.shape[0] // tile * tile
                    assert m0 < s2.shape[0] - 1
                    s2[m0:-1] = s2[m0 + 1:].clone()
                    s2[-1] = 0
                    s = s2.reshape(S, H, W, C).permute(0, 3, 1, 2)
                v = v + s
            if relu:
                v = F.relu(v)
            if fault == "dead_skip" and name == target:   # the columns of all-zero filters: not computed, bias and all
                v = v.clone()
                v[:, (wt.reshape(wt.shape[0], -1) != 0).sum(1) == 0] = 0
            if fault == "channel" and name == target:
                ch = _low_channel(v)
                info.update(channel=ch, ch_max=float(v[:, ch].abs().max()), layer_max=float(v.abs().max()))
                v = v.clone()
                v[:, ch] *= 1.001
            store(name, v, f32_out=op == "head")
        elif op == "feat":
            x = T[ins[0]]
            d2 = F.conv_transpose2d(x, f32(lw["res5c_branch2a/kernel"]).permute(3, 2, 0, 1), stride=2, padding=1)
            d1 = F.conv_transpose2d(x, f32(lw["res5c_branch1a/kernel"]).permute(3, 2, 0, 1), stride=2, padding=1)
            bias, scale, shift = (f32(v).view(1, -1, 1, 1) for v in layer_ref.fold_bn(lw))
            if fault == "bn_abs":
                scale = scale.abs()
            bn = F.relu((d2 + bias) * scale + shift)
            deltas = _rne_bf16(d1) if bf else d1
            dx, dy, dz = deltas[:, 0:21], deltas[:, 21:42], deltas[:, 42:63]
            bone = torch.sqrt((dx * dx + dy * dy) + dz * dz)
            store(name, torch.cat([bn, d1, bone], 1))
    asked = TABLE_PAPER if paper else TABLE   # (wiring_crossed: the res2c_branch2a it ran is no tensor of the plan it was asked for)
    return {k: v.permute(0, 2, 3, 1).contiguous().numpy() for k, v in T.items() if k in asked and not (fused and k in HIDDEN)}, info


@pytest.fixture(scope="module")
def batch():
    frame = helpers.synth_frame(1234, smooth=True).astype(np.float32)
    return (frame / 255.0 - 0.4)[None]


def _failing(rows):
    return sorted(r["tensor"] for r in rows if not r["ok"])


def _report(tag, rows):
    worst = max(rows, key=lambda r: r["cal"])
    m = [r["match"] for r in rows if r["match"] is not None]
    print("%-24s worst calibrated %.3g (%s), worst rigorous %.3g, lowest bf16 match %s" % (
        tag, worst["cal"], worst["tensor"], max(r["rig"] for r in rows), ("%.5f" % min(m)) if m else "-"))


def _table(paper):
    return TABLE_PAPER if paper else TABLE


def _clean_stand_in(weights, batch, prec, paper):
    acts, _ = device_forward(weights, batch, prec, paper=paper)
    rows = layer_ref.check_all(acts, weights, prec, batch, table=_table(paper))
    _report(prec + (" paper" if paper else ""), rows)
    assert len(rows) == len(_table(paper)) == len(TABLE) + paper
    assert _failing(rows) == [], [r for r in rows if not r["ok"]][:3]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_clean_stand_in_passes_every_tensor(weights, batch, prec):
    _clean_stand_in(weights, batch, prec, False)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_clean_stand_in_passes_every_tensor_of_the_paper_table(weights, batch, prec):
    _clean_stand_in(weights, batch, prec, True)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_fails_the_gate_on_its_tensor(weights, batch, fault):
    target, prec = FAULTS[fault]
    acts, info = device_forward(weights, batch, prec, fault)
    rows = layer_ref.check_all(acts, weights, prec, batch)
    _report(fault, rows)
    assert _failing(rows) == [target]
    row = next(r for r in rows if r["tensor"] == target)
    if fault == "truncate":
        assert row["match"] < 0.75  # the sharpness gate alone catches a truncating store
    if fault == "channel":
        # invisible to the layer-maximum gate of test_conv_stack_every_layer, caught by the calibrated tier only
        assert 1e-3 * info["ch_max"] <= 1e-4 * info["layer_max"], info
        assert row["cal"] > 1.0 and row["rig"] <= 1.0, row


@pytest.mark.parametrize("fault", sorted(WIRING_FAULTS))
def test_planted_wiring_fault_fails_the_gate_on_res2c_branch2b(weights, batch, fault):
    """A device that runs the other wiring's res2c_branch2b fails the table of the wiring it was asked for on exactly that tensor: every
    tensor behind it is gated from the device's own inputs, and res2c_branch2a -- present or pruned -- is itself right."""
    target, prec, paper = WIRING_FAULTS[fault]
    acts, _ = device_forward(weights, batch, prec, fault, paper=paper)
    rows = layer_ref.check_all(acts, weights, prec, batch, table=_table(paper))
    _report(fault, rows)
    assert len(rows) == len(_table(paper))
    assert _failing(rows) == [target] == ["res2c_branch2b"]
    row = next(r for r in rows if r["tensor"] == target)
    assert row["rig"] > 1.0 and row["cal"] > 1.0, row   # (no bound is near: the two wirings differ by the tensor's own size)


@pytest.fixture(scope="module")
def plain_acts(weights, batch):
    return {(prec, paper): device_forward(weights, batch, prec, paper=paper)[0] for prec in ("fp32", "bf16") for paper in (False, True)}


def _first_difference(fused, plain, table=TABLE):
    """the first tensor, in launch order (the table's), that the fused stand-in stores and that differs from the plain one's"""
    return next((n for n in table if n in fused and not np.array_equal(fused[n], plain[n])), None)


def _clean_fused(weights, batch, plain_acts, prec, paper):
    acts, _ = device_forward(weights, batch, prec, fused=True, paper=paper)
    table = _table(paper)
    written = {"input"}
    for n in ["conv1", "pool1"] + (FUSED_LAUNCHES_PAPER if paper else FUSED_LAUNCHES):
        written.update(layer_ref.launch_tensors(n, stem=True, pair=True, table=table))
    assert set(table) - set(acts) == HIDDEN and written <= set(acts)
    assert ("res2c_branch2a" in written) == paper
    assert _first_difference(acts, plain_acts[prec, paper], table) is None


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_clean_fused_stand_in_equals_the_plain_one(weights, batch, plain_acts, prec):
    _clean_fused(weights, batch, plain_acts, prec, False)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_clean_fused_stand_in_of_the_paper_plan_equals_the_plain_one(weights, batch, plain_acts, prec):
    _clean_fused(weights, batch, plain_acts, prec, True)


@pytest.mark.parametrize("fault", sorted(FUSED_FAULTS))
def test_planted_fused_fault_breaks_equality_first_on_its_tensor(weights, batch, plain_acts, fault):
    target, prec = FUSED_FAULTS[fault]
    acts, _ = device_forward(weights, batch, prec, fault, fused=True)
    assert _first_difference(acts, plain_acts[prec, False]) == target


@pytest.mark.parametrize("fault", sorted(FUSED_FAULTS_PAPER))
def test_planted_fault_of_the_paper_chain_breaks_equality_first_on_its_tensor(weights, batch, plain_acts, fault):
    """res2b_branch2b>res2b_branch2c>res2c_branch2a: its block output read unrounded by the chain GEMM -> res2c_branch2a; its identity
    shortcut (the block input res2a) read one row down in the last, partial 64-row tile -> res2b."""
    target, prec = FUSED_FAULTS_PAPER[fault]
    acts, _ = device_forward(weights, batch, prec, fault, fused=True, paper=True)
    assert _first_difference(acts, plain_acts[prec, True], TABLE_PAPER) == target


def _table_is_the_float64_graph(weights, batch, paper):
    """The input table is the graph of tests/torch_net.py, in either wiring: each tensor's reference, fed torch_net's own float64
    activations (as float32), reproduces torch_net's activation of that name (a wrong input, scope, stride, padding, ReLU or BN fold
    would not)."""
    from tests import torch_net
    taps = {}
    torch_net.forward(weights, batch, paper_res2c=paper, taps=taps)
    acts = {k: v.numpy().astype(np.float32) for k, v in taps.items()}
    acts["input"] = batch
    table = _table(paper)
    assert ("res2c_branch2a" in table) == paper and table["res2c_branch2b"][1] == ["res2c_branch2a" if paper else "res2b_branch2a"]
    for name, (op, _, _) in table.items():
        if op == "input":
            continue
        r = layer_ref.reference(name, acts, weights, table)
        y = r["exact"] if "exact" in r else r["y"]
        want = taps[name].numpy()
        assert y.shape == want.shape, name
        assert float(np.abs(y - want).max()) <= 1e-5 * float(np.abs(want).max()), name


def test_every_launch_form_maps_to_a_checked_tensor():
    """launch_tensors: the launch names of rt_plan.cpp's plans map to the table tensors they write -- a fused tail to its block output (the
    head's to the final maps), a chain also to the next block's branch2a, the stem's PAIR form to res2a_branch2a and res2a_branch1; unknown
    names raise, so that the GPU tests' coverage assertions fail on a launch form they do not know."""
    lt = layer_ref.launch_tensors
    assert lt("res2a_branch2a+branch1") == ["res2a_branch2a", "res2a_branch1"]
    assert lt("res2b_branch2b+res2c_branch2b") == ["res2b_branch2b", "res2c_branch2b"]
    assert lt("res5a_branch2a_new[:256]") == ["res5a_branch2a_new"]
    assert lt("res5a_branch2a_new+branch1_new") == ["res5a_branch2a_new", "res5a_branch1_new"]
    assert lt("res3b_branch2c") == ["res3b"] and lt("res5a_branch2c_new") == ["res5a"]
    assert lt("res5c_deconv") == lt("res5c_bone_length") == ["res5c_branch2a_feat"]
    assert lt("res5c_branch2c") == ["res5c_branch2c"] and lt("res5b_branch2c_new") == ["res5b_branch2c_new"]
    assert lt("conv1", stem=True) == lt("pool1", stem=True) == ["pool1"]
    assert lt("conv1", stem=True, pair=True) == lt("pool1", stem=True, pair=True) == ["res2a_branch2a", "res2a_branch1"]
    assert lt("res2a_branch2b>res2a_branch2c") == ["res2a"] and lt("res3d_branch2b>res3d_branch2c") == ["res3d"]
    assert lt("res2a_branch2b>res2a_branch2c>res2b_branch2a") == ["res2a", "res2b_branch2a"]
    assert lt("res3a_branch2b>res3a_branch2c>res3b_branch2a") == ["res3a", "res3b_branch2a"]
    assert lt("res5c_branch2b>res5c_branch2c") == ["res5c_branch2c"]
    for bad in ("res2a_branch2b>res2b_branch2c", "res3a_branch2b>res3a_branch2c>res3c_branch2a", "res3a_branch2b>res3a_branch2c>res3b_branch2b",
                "res2b_branch2b>res2b_branch2c>res2c_branch2a", "res3a_branch2a>res3a_branch2c", "res3a_branch2b>res3a_branch2c>res3b_branch2a>res3b",
                "res2c_branch2a", "res6a"):
        with pytest.raises(KeyError):
            lt(bad)
    # the paper wiring (TABLE_PAPER): res2c_branch2a is a tensor, res2b's tail may chain it, and the two 3x3 layers of res2b / res2c no longer
    # read one tensor, so their dual-output launch is unknown there; everything else as above
    ltp = lambda name, **kw: lt(name, table=TABLE_PAPER, **kw)
    assert ltp("res2c_branch2a") == ["res2c_branch2a"]
    assert ltp("res2b_branch2b>res2b_branch2c>res2c_branch2a") == ["res2b", "res2c_branch2a"]
    assert ltp("res2a_branch2b>res2a_branch2c>res2b_branch2a") == ["res2a", "res2b_branch2a"]
    assert ltp("res2c_branch2b>res2c_branch2c") == ["res2c"] and ltp("res2c_branch2b") == ["res2c_branch2b"]
    assert ltp("res2a_branch2a+branch1") == ["res2a_branch2a", "res2a_branch1"]
    assert ltp("conv1", stem=True, pair=True) == ["res2a_branch2a", "res2a_branch1"]
    for bad in ("res2b_branch2b+res2c_branch2b", "res2a_branch2b>res2a_branch2c>res2c_branch2a", "res2c_branch2b>res2c_branch2c>res2c_branch2a",
                "res2b_branch2b>res2b_branch2c>res3a_branch2a", "res6a"):
        with pytest.raises(KeyError):
            ltp(bad)


def test_table_wiring_matches_the_float64_graph(weights, batch):
    _table_is_the_float64_graph(weights, batch, False)


def test_paper_table_wiring_matches_the_float64_graph(weights, batch):
    _table_is_the_float64_graph(weights, batch, True)
