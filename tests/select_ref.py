"""Selection weights: a known answer for every conv launch that needs no tolerance (test helper; numpy only, nothing imported from
the code under test).

Every output channel of every conv has exactly ONE non-zero weight, +1 or -1, at one tap (ky, kx) and one input channel ci, and the
batch holds small integers.  Then every tensor of the network is an integer-valued gather of its input tensor: each product and each
partial sum is exact in fp32 whatever the summation order, tile shape, K split, MFMA form or fusion, so a device tensor that differs
from `expected` has a wrong index, a wrong halo, a dropped or doubled term or a wrong weight layout -- never rounding.

The index rules are TensorFlow's documented SAME rule (out = ceil(n / s), total padding max((out - 1) s + k - n, 0), the smaller half
before), which is how src/vnect_model.py:27-217 builds these layers; for this network's fixed shapes they are the literals of PAD:
  conv1   7x7 stride 2, 368 -> 184: pad 2 before, 3 after;   tap (ky, kx) of out[y, x] reads in[2y + ky - 2, 2x + kx - 2]
  pool1   3x3 stride 2, 184 -> 92:  pad 0 before, 1 after;   out[y, x] = max over rows 2y .. 2y + 2, columns 2x .. 2x + 2
  3x3     stride 1:                 pad 1 before, 1 after;   in[y + ky - 1, x + kx - 1]
  1x1     stride 2 (VALID):                                  in[2y, 2x]
  transposed conv 4x4 stride 2, 23 -> 46:  out[2i - 1 + ky, 2j - 1 + kx] += in[i, j] w[ky, kx, co, ci]
          i.e. out[oy, ox] reads in[(oy + 1 - ky) / 2, (ox + 1 - kx) / 2] where that is an integer
  out of range contributes 0 (the pool: is ignored); a block output adds its shortcut tensor, then ReLU; BN columns: relu(2 d).
Bone lengths (res5c_branch2a_feat[..., 191:212] = sqrt(dx^2 + dy^2 + dz^2) of the deltas) are the one thing that is not a gather:
BONE marks them, bone_channels() says which channels of the tensors behind them inherit them in a chain from the batch alone.

16-bit handles (FP16.md): every stored tensor but the final maps, and every tensor a fused launch hands over on chip, is rounded to
nearest even in the handle's element type; `expected` rounds at exactly those points.  expected() composes: an input tensor that is
not in `acts` (a fused launch keeps it on chip) is computed by the same rule from ITS inputs and rounded.
"""
import numpy as np

SETS = 4          # weight sets: the widest fan-in ratio (256 -> 64, 1024 -> 256) needs four to select every input channel once
BONE = slice(191, 212)
WIDE = (-100, 100) # batch range that takes the chain past 2^8 (bf16 stores round there) and keeps it below 2^11 (fp16 stores stay exact)
BN_VARIANCE = np.float32(0.25) - np.float32(0.001)   # + 0.001 -> 0.25 exactly: the folded scale is 1 / sqrt(0.25) = 2.0

# (scope, k, Cin, Cout, relu) of every conv2d scope (weights (k, k, Cin, Cout) + biases)
CONVS = [("conv1", 7, 3, 64, True)]
for _p, _cin, _mid, _out, _ids in (("res2", 64, 64, 256, "bc"), ("res3", 256, 128, 512, "bcd"), ("res4", 512, 256, 1024, "bcdef")):
    CONVS += [(_p + "a_branch1", 1, _cin, _out, False), (_p + "a_branch2a", 1, _cin, _mid, True),
              (_p + "a_branch2b", 3, _mid, _mid, True), (_p + "a_branch2c", 1, _mid, _out, False)]
    for _i in _ids:
        CONVS += [(_p + _i + "_branch2a", 1, _out, _mid, True), (_p + _i + "_branch2b", 3, _mid, _mid, True),
                  (_p + _i + "_branch2c", 1, _mid, _out, False)]
CONVS += [("res5a_branch2a_new", 1, 1024, 512, True), ("res5a_branch2b_new", 3, 512, 512, True), ("res5a_branch2c_new", 1, 512, 1024, False),
          ("res5a_branch1_new", 1, 1024, 1024, False), ("res5b_branch2a_new", 1, 1024, 256, True), ("res5b_branch2b_new", 3, 256, 128, True),
          ("res5b_branch2c_new", 1, 128, 256, True), ("res5c_branch2b", 3, 212, 128, True)]
HEAD = ("res5c_branch2c", 1, 128, 84, False)                 # kernel (1, 1, Cin, Cout), no bias
DECONVS = [("res5c_branch2a", 256, 128), ("res5c_branch1a", 256, 63)]   # kernel (4, 4, Cout, Cin), no bias; BN + ReLU | deltas
# (k, stride) -> (pad before, pad after), per axis
PAD = {(7, 2): (2, 3), (3, 1): (1, 1), (1, 1): (0, 0), (1, 2): (0, 0)}
POOL_PAD = (0, 1)
# transposed conv: output parity (oy % 2) -> the two ky with 2i - 1 + ky of that parity
DECONV_TAPS = {0: (1, 3), 1: (0, 2)}


def _scope_seed(scope):
    return sum((i + 1) * ord(c) for i, c in enumerate(scope)) % 100003


def _channel_map(rs, set_index, cin, cout):
    """ci per output channel: a seeded permutation of the input channels, read at R co + (set_index mod R), R = ceil(Cin / Cout): the
    sets 0 .. R - 1 together select every input channel."""
    R = -(-cin // cout)
    return rs.permutation(cin)[(R * np.arange(cout) + set_index % R) % cin]


def selection(set_index, paper_res2c=False):
    """scope -> dict(sign, ky, kx, ci), int64 arrays per output channel; the transposed convs: arrays (4, Cout), one row per output
    parity class q = 2 (oy % 2) + (ox % 2).  Signs are -1 only on layers without ReLU.  In a projection block a channel never has
    both branch1 and branch2c at -1 (relu(-s - b) is dead); in the identity blocks of a stage a channel's branch2c sign alternates
    from block to block from a seeded phase, so that no channel adds (and doubles) in every block.  (paper_res2c changes the wiring,
    not the weights: res2c_branch2a has weights either way.)"""
    sel = {}
    phase = {}
    for scope, k, cin, cout, relu in CONVS + [HEAD]:
        rs = np.random.RandomState(_scope_seed(scope))      # per layer, the same in every set: the sets differ by set_index alone
        ci = _channel_map(rs, set_index, cin, cout)
        tap = (rs.permutation(cout) + set_index * 5) % (k * k)
        sign = np.ones(cout, np.int64)
        if not relu:
            coin = np.random.RandomState(_scope_seed(scope) + 7919 * (set_index + 1)).randint(0, 2, cout)
            block = scope.split("_")[0]
            stage = block[:4]
            if scope == HEAD[0]:
                sign = 1 - 2 * coin
            elif scope == "res5a_branch2c_new":               # (listed before its shortcut, which takes the other sign below)
                sign = 1 - 2 * coin
            elif "_branch1" in scope:                         # projection shortcut: its branch2c (below) takes the other sign
                sign = 1 - 2 * coin
                phase[block] = coin
            elif block in phase:                              # branch2c of a projection block
                sign = 2 * phase[block] - 1
                phase[stage] = coin
            else:                                             # branch2c of an identity block
                n = phase.setdefault(stage + "#", 0)
                phase[stage + "#"] = n + 1
                sign = 1 - 2 * ((phase[stage] + n) % 2)
        sel[scope] = dict(sign=sign.astype(np.int64), ky=(tap // k).astype(np.int64), kx=(tap % k).astype(np.int64), ci=ci.astype(np.int64))
    # res5a's projection pair is listed branch2c first: give branch1 the other sign
    sel["res5a_branch1_new"]["sign"] = -sel["res5a_branch2c_new"]["sign"]
    for scope, cin, cout in DECONVS:
        rs = np.random.RandomState(_scope_seed(scope))
        d = dict(sign=np.ones((4, cout), np.int64), ky=np.zeros((4, cout), np.int64), kx=np.zeros((4, cout), np.int64),
                 ci=np.zeros((4, cout), np.int64))
        for q in range(4):
            pick = (rs.permutation(cout) + set_index) % 4
            d["ky"][q] = np.asarray(DECONV_TAPS[q // 2])[pick // 2]
            d["kx"][q] = np.asarray(DECONV_TAPS[q % 2])[pick % 2]
            d["ci"][q] = _channel_map(rs, set_index + q, cin, cout)
            if scope == "res5c_branch1a":
                d["sign"][q] = 1 - 2 * np.random.RandomState(_scope_seed(scope) + 31 * q + 7919 * (set_index + 1)).randint(0, 2, cout)
        sel[scope] = d
    return sel


def weights_from(sel):
    """The weight dict (the schema of vnect_amd.weights) of a selection."""
    w = {}
    for scope, k, cin, cout, _ in CONVS:
        s = sel[scope]
        a = np.zeros((k, k, cin, cout), np.float32)
        a[s["ky"], s["kx"], s["ci"], np.arange(cout)] = s["sign"]
        w[scope + "/weights"] = a
        w[scope + "/biases"] = np.zeros(cout, np.float32)
    scope, k, cin, cout, _ = HEAD
    s = sel[scope]
    a = np.zeros((1, 1, cin, cout), np.float32)
    a[0, 0, s["ci"], np.arange(cout)] = s["sign"]
    w[scope + "/kernel"] = a
    for scope, cin, cout in DECONVS:
        s = sel[scope]
        a = np.zeros((4, 4, cout, cin), np.float32)
        for q in range(4):
            a[s["ky"][q], s["kx"][q], np.arange(cout), s["ci"][q]] = s["sign"][q]
        w[scope + "/kernel"] = a
    w["bn5c_branch2a/gamma"] = np.ones(128, np.float32)
    w["bn5c_branch2a/beta"] = np.zeros(128, np.float32)
    w["bn5c_branch2a/moving_mean"] = np.zeros(128, np.float32)
    w["bn5c_branch2a/moving_variance"] = np.full(128, BN_VARIANCE, np.float32)
    scale = w["bn5c_branch2a/gamma"] * (np.float32(1.0) / np.sqrt(w["bn5c_branch2a/moving_variance"] + np.float32(0.001)))
    assert scale.dtype == np.float32 and np.all(scale == np.float32(2.0)), scale
    return w


def weights(set_index, paper_res2c=False):
    return weights_from(selection(set_index, paper_res2c))


def batch(seed, S, lo=-4, hi=4):
    """(S, 368, 368, 3) float32 of integers in [lo, hi]."""
    return np.random.RandomState(1000 + seed).randint(lo, hi + 1, (S, 368, 368, 3)).astype(np.float32)


def round_elem(a, elem):
    """Round to nearest even in the element type of a handle: None / 'fp32' / 'fp32_split' store fp32 (the values here are exact in
    it), 'bf16', 'fp16'."""
    if elem in (None, "fp32", "fp32_split"):
        return a
    f = np.ascontiguousarray(a, np.float32)
    if elem == "fp16":
        with np.errstate(over="ignore"):
            return _exact(f.astype(np.float16).astype(np.float32))
    assert elem == "bf16", elem
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return _exact(u.astype(np.uint32).view(np.float32).reshape(f.shape))


def _exact(a):
    """int64 where every value is an integer below 2^53, float64 otherwise (the stem's tensors of a real frame: copies and maxima)."""
    a = np.asarray(a)
    if a.dtype == np.int64:
        return a
    a = a.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if np.all(np.isfinite(a)) and np.all(a == np.rint(a)) and np.all(np.abs(a) < 2.0 ** 53):
            return a.astype(np.int64)
    return a


def _relu(a):
    return np.maximum(a, 0)


def gather_conv(x, s, k, stride):
    """out[n, y, x, co] = sign[co] * in[n, stride y + ky[co] - before, stride x + kx[co] - before, ci[co]], 0 out of range."""
    before, after = PAD[(k, stride)]
    N, H, W, _ = x.shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    assert (Ho - 1) * stride + k - 1 - before <= H - 1 + after
    xp = np.zeros((N, H + before + after, W + before + after, x.shape[3]), x.dtype)
    xp[:, before:before + H, before:before + W] = x
    out = np.zeros((N, Ho, Wo, len(s["ci"])), x.dtype)
    for tap in np.unique(s["ky"] * k + s["kx"]):
        ky, kx = int(tap) // k, int(tap) % k
        co = np.nonzero((s["ky"] == ky) & (s["kx"] == kx))[0]
        out[..., co] = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride][..., s["ci"][co]] * s["sign"][co].astype(x.dtype)
    return out


def pool(x):
    before, after = POOL_PAD
    N, H, W, C = x.shape
    Ho, Wo = -(-H // 2), -(-W // 2)
    low = np.iinfo(np.int64).min if x.dtype == np.int64 else -np.inf
    xp = np.full((N, H + before + after, W + before + after, C), low, x.dtype)
    xp[:, before:before + H, before:before + W] = x
    out = xp[:, 0:2 * Ho:2, 0:2 * Wo:2]
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2])
    return out


def gather_deconv(x, s):
    """out[n, oy, ox, co], class q = 2 (oy % 2) + (ox % 2): sign[q, co] * in[n, (oy + 1 - ky[q, co]) / 2, (ox + 1 - kx[q, co]) / 2,
    ci[q, co]], 0 out of range -- the one term of out[2i - 1 + ky, 2j - 1 + kx] += in[i, j] w[ky, kx, co, ci] that is not zero."""
    N, H, W, _ = x.shape
    xp = np.zeros((N, H + 2, W + 2, x.shape[3]), x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = np.zeros((N, 2 * H, 2 * W, s["ci"].shape[1]), x.dtype)
    for q in range(4):
        py, px = q // 2, q % 2
        assert np.all((s["ky"][q] + 1 + py) % 2 == 0) and np.all((s["kx"][q] + 1 + px) % 2 == 0)
        for tap in np.unique(s["ky"][q] * 4 + s["kx"][q]):
            ky, kx = int(tap) // 4, int(tap) % 4
            co = np.nonzero((s["ky"][q] == ky) & (s["kx"][q] == kx))[0]
            dy, dx = (py + 1 - ky) // 2, (px + 1 - kx) // 2   # oy = 2a + py reads in[a + dy]
            v = xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W][..., s["ci"][q][co]] * s["sign"][q][co].astype(x.dtype)
            sub = out[:, py::2, px::2]
            sub[..., co] = v
    return out


def expected(name, acts, sel, table, elem=None, memo=None):
    """The tensor `name` of `table` (tests/layer_ref.py table(): the wiring only) as a handle of element type `elem` stores it,
    from its input tensors in `acts` (name -> NHWC array).  An input that `acts` lacks is composed: computed by this rule from its own
    inputs and rounded like a stored one (the on-chip layer of a fused launch); `memo` keeps those.  int64 (float64 where the inputs
    are not integers, and in the bone columns)."""
    memo = {} if memo is None else memo

    def get(t):
        if t in acts:
            return _exact(acts[t])
        if t not in memo:
            memo[t] = expected(t, acts, sel, table, elem, memo)
        return memo[t]

    op, ins, p = table[name]
    if op == "input":
        raise KeyError("the input has no rule: it is given")
    if op == "pool":
        out = pool(get(ins[0]))
    elif op == "conv":
        out = gather_conv(get(ins[0]), sel[p["scope"]], p["k"], p["stride"])
        if len(ins) > 1:
            sc = get(ins[1])
            if out.dtype != sc.dtype:
                out, sc = out.astype(np.float64), sc.astype(np.float64)
            out = out + sc
        if p["relu"]:
            out = _relu(out)
    elif op == "head":
        out = gather_conv(get(ins[0]), sel[HEAD[0]], 1, 1)
    elif op == "feat":
        x = get(ins[0])
        bn = _relu(2 * gather_deconv(x, sel["res5c_branch2a"]))
        dl = gather_deconv(x, sel["res5c_branch1a"])
        stored = _exact(acts[name][..., 128:191]) if name in acts else round_elem(dl, elem)
        d = stored.astype(np.float64)
        dx, dy, dz = d[..., 0:21], d[..., 21:42], d[..., 42:63]
        bone = np.sqrt(dx * dx + dy * dy + dz * dz)
        out = np.concatenate([bn.astype(np.float64), dl.astype(np.float64), bone], -1)
        if elem in ("bf16", "fp16"):
            out = np.asarray(round_elem(out, elem), np.float64)
        return out
    else:
        raise ValueError(name)
    return out if name == HEAD[0] else round_elem(out, elem)


def chain(batch_, sel, table, elem=None):
    """Every tensor of `table` from the batch alone."""
    acts = {"input": round_elem(_exact(batch_), elem)}
    memo = {}
    for name in table:
        if name != "input" and name not in memo:
            memo[name] = expected(name, acts, sel, table, elem, memo)
    memo["input"] = acts["input"]
    return memo


def bone_channels(name, sel):
    """bool per channel of `name`: derived from a bone-length column in a chain from the batch alone (None: no channel is)."""
    if name == "res5c_branch2a_feat":
        m = np.zeros(212, bool)
        m[BONE] = True
        return m
    b = sel["res5c_branch2b"]["ci"] >= BONE.start
    if name == "res5c_branch2b":
        return b
    if name == HEAD[0]:
        return b[sel[HEAD[0]]["ci"]]
    return None
