"""Selection weights (tests/select_ref.py) on the CPU: the integer rule against anchors written out by hand, the three restatements of
the network (oracle/vnect_net.c, tests/torch_net.py, tests/layer_ref.py) against the rule, the conditions that make the weight sets a
gate (coverage, density, distinctness, range), and planted faults on a numpy stand-in of a device, each caught on its own tensors only."""
import functools

import numpy as np
import pytest

from tests import layer_ref, select_ref as sr

TABLES = {False: layer_ref.table(False), True: layer_ref.table(True)}
COMBOS = [(s, p) for p in (False, True) for s in range(sr.SETS)]


@functools.lru_cache(maxsize=None)
def _chain(set_index, paper=False, elem=None):
    return sr.chain(sr.batch(set_index, 1), sr.selection(set_index, paper), TABLES[paper], elem)


def _val(shape, c_step=10 ** 6, sign=1):
    """in[0, y, x, c] = sign * (c * 1e6 + y * 1000 + x + 1): a tensor that names its own indices"""
    _, H, W, C = shape
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return (sign * (c * c_step + y * 1000 + x + 1))[None].astype(np.int64)


def _sel(rows):
    """[(sign, ky, kx, ci)] per output channel"""
    a = np.asarray(rows, np.int64).reshape(len(rows), 4)
    return dict(sign=a[:, 0], ky=a[:, 1], kx=a[:, 2], ci=a[:, 3])


# ---- a. anchors ------------------------------------------------------------------------------------------------------------------------

def test_anchor_conv1():
    """7x7 stride 2 on 368: pad 2 before, 3 after -- out[y, x] tap (ky, kx) reads in[2y + ky - 2, 2x + kx - 2]"""
    table = {"conv1": ("conv", ["input"], dict(scope="conv1", k=7, stride=2, relu=True))}
    sel = {"conv1": _sel([(1, 0, 0, 0), (1, 6, 6, 2), (1, 3, 2, 1), (1, 2, 2, 0)])}
    out = sr.expected("conv1", {"input": _val((1, 368, 368, 3))}, sel, table)
    assert out.shape == (1, 184, 184, 4) and out.dtype == np.int64
    o = out[0]
    assert o[0, 0, 0] == 0                # in[-2, -2]: the two pad rows before
    assert o[0, 1, 0] == 0                # in[-2, 0]
    assert o[1, 1, 0] == 1                # in[0, 0, 0]
    assert o[0, 0, 3] == 1                # tap (2, 2) of output 0 is input pixel 0
    assert o[183, 183, 1] == 0            # in[370, 370]: past the end
    assert o[181, 182, 1] == 0            # in[366, 368]: column 368 is the first pad column after
    assert o[181, 181, 1] == 2366367      # in[366, 366, 2]
    assert o[183, 183, 2] == 1367367      # tap (3, 2): in[367, 366, 1], the last input row
    assert o[10, 20, 2] == 1021041        # in[21, 40, 1]
    assert o[183, 0, 3] == 366001         # tap (2, 2): in[366, 0, 0]


def test_anchor_pool1():
    """3x3 stride 2 on 184: pad 0 before, 1 after -- the window of out[y, x] is rows 2y .. 2y + 2, columns 2x .. 2x + 2"""
    table = {"pool1": ("pool", ["conv1"], {})}
    up = sr.expected("pool1", {"conv1": _val((1, 184, 184, 2))}, {}, table)[0]       # rising: the maximum is the window's far corner
    assert up.shape == (92, 92, 2)
    assert up[0, 0, 0] == 2003            # in[2, 2]
    assert up[91, 91, 0] == 183184        # in[183, 183]: row 184 is padding
    assert up[91, 0, 1] == 1183003        # in[183, 2, 1]
    assert up[5, 7, 0] == 12017           # in[12, 16]
    down = sr.expected("pool1", {"conv1": _val((1, 184, 184, 2), sign=-1)}, {}, table)[0]   # falling: its near corner
    assert down[0, 0, 0] == -1            # in[0, 0]: no row before 0
    assert down[5, 7, 0] == -10015        # in[10, 14]
    assert down[91, 91, 0] == -182183     # in[182, 182]


def test_anchor_3x3():
    """3x3 stride 1: pad 1 / 1 -- in[y + ky - 1, x + kx - 1]"""
    table = {"t": ("conv", ["x"], dict(scope="t", k=3, stride=1, relu=False))}
    sel = {"t": _sel([(1, 0, 0, 0), (1, 2, 2, 1), (-1, 0, 2, 0), (1, 1, 1, 1)])}
    o = sr.expected("t", {"x": _val((1, 46, 46, 2))}, sel, table)[0]
    assert o.shape == (46, 46, 4)
    assert o[0, 0, 0] == 0                # in[-1, -1]
    assert o[0, 5, 0] == 0                # the top halo row reads 0
    assert o[1, 1, 0] == 1                # in[0, 0, 0]
    assert o[45, 45, 0] == 44045          # in[44, 44, 0]
    assert o[0, 0, 1] == 1001002          # in[1, 1, 1]
    assert o[45, 45, 1] == 0              # in[46, 46]
    assert o[45, 0, 1] == 0               # in[46, 1]
    assert o[7, 9, 2] == -6011            # -in[6, 10, 0]
    assert o[7, 45, 2] == 0               # in[6, 46]
    assert o[45, 45, 3] == 1045046        # the centre tap: in[45, 45, 1]


def test_anchor_1x1_stride_2():
    """1x1 stride 2 VALID: in[2y, 2x]"""
    table = {"t": ("conv", ["x"], dict(scope="t", k=1, stride=2, relu=True))}
    o = sr.expected("t", {"x": _val((1, 92, 92, 3))}, {"t": _sel([(1, 0, 0, 2), (1, 0, 0, 0)])}, table)[0]
    assert o.shape == (46, 46, 2)
    assert o[0, 0, 1] == 1                # in[0, 0, 0]
    assert o[0, 1, 1] == 3                # in[0, 2, 0]: the even pixels
    assert o[45, 45, 1] == 90091          # in[90, 90, 0]; row 91 is never read
    assert o[3, 4, 0] == 2006009          # in[6, 8, 2]


def test_anchor_transposed_conv():
    """4x4 stride 2, 23 -> 46: out[2i - 1 + ky, 2j - 1 + kx] += in[i, j] w[ky, kx, co, ci]"""
    s = dict(sign=np.asarray([[1], [1], [-1], [1]], np.int64), ci=np.asarray([[0], [1], [0], [1]], np.int64),
             ky=np.asarray([[1], [3], [0], [2]], np.int64), kx=np.asarray([[1], [2], [3], [0]], np.int64))   # classes (even, even), (even, odd), (odd, even), (odd, odd)
    o = sr.gather_deconv(_val((1, 23, 23, 2)), s)[0, :, :, 0]
    assert o.shape == (46, 46)
    assert o[0, 0] == 1                   # ky = 1: i = 0;  kx = 1: j = 0
    assert o[44, 44] == 22023             # i = j = 22
    assert o[0, 1] == 0                   # ky = 3: 2i + 2 = 0 has i = -1
    assert o[2, 1] == 1000001             # ky = 3: i = 0;  kx = 2: 2j + 1 = 1, j = 0; ci 1
    assert o[1, 0] == 0                   # kx = 3: 2j + 2 = 0 has j = -1
    assert o[1, 2] == -1001               # ky = 0: 2i - 1 = 1, i = 1;  kx = 3: j = 0; sign -1
    assert o[45, 45] == 0                 # kx = 0: 2j - 1 = 45 has j = 23
    assert o[45, 43] == 1022023           # ky = 2: 2i + 1 = 45, i = 22;  kx = 0: j = 22
    # through expected(): BN columns relu(2 d), deltas d, bone lengths from the deltas
    sel = sr.selection(0)
    x = np.zeros((1, 23, 23, 256), np.int64)
    x[0, 3, 4] = np.arange(256) + 1
    f = sr.expected("res5c_branch2a_feat", {"res5b_branch2c_new": x}, sel, TABLES[False])
    assert f.shape == (1, 46, 46, 212)
    a, d = sel["res5c_branch2a"], sel["res5c_branch1a"]
    for co in (0, 5, 127):
        for q in range(4):
            oy, ox = 2 * 3 - 1 + a["ky"][q, co], 2 * 4 - 1 + a["kx"][q, co]
            assert (oy % 2, ox % 2) == (q // 2, q % 2) and f[0, oy, ox, co] == 2 * (a["ci"][q, co] + 1)
    for co in (0, 62):
        for q in range(4):
            oy, ox = 2 * 3 - 1 + d["ky"][q, co], 2 * 4 - 1 + d["kx"][q, co]
            assert f[0, oy, ox, 128 + co] == d["sign"][q, co] * (d["ci"][q, co] + 1)
    dl = f[..., 128:191]
    assert np.array_equal(f[..., sr.BONE], np.sqrt(dl[..., 0:21] ** 2 + dl[..., 21:42] ** 2 + dl[..., 42:63] ** 2))


def test_block_output_adds_the_shortcut_then_relu():
    table = {"b": ("conv", ["x", "s"], dict(scope="b", k=1, stride=1, relu=True))}
    x = np.asarray([3, 5], np.int64).reshape(1, 1, 1, 2)
    s = np.asarray([-4, 1, 9], np.int64).reshape(1, 1, 1, 3)
    o = sr.expected("b", {"x": x, "s": s}, {"b": _sel([(1, 0, 0, 0), (-1, 0, 0, 1), (-1, 0, 0, 1)])}, table)
    assert o.ravel().tolist() == [0, 0, 4]     # relu(3 - 4), relu(-5 + 1), relu(-5 + 9)


def test_16_bit_rounding_of_the_rule():
    a = np.asarray([255, 256, 257, 258, 259, 1025, 2049, 2051, -259, 65519, 65520], np.int64)
    assert sr.round_elem(a, "bf16").tolist() == [255, 256, 256, 258, 260, 1024, 2048, 2048, -260, 65536, 65536]
    h = sr.round_elem(a, "fp16")
    assert h[:10].tolist() == [255, 256, 257, 258, 259, 1025, 2048, 2052, -259, 65504] and np.isinf(h[10])
    assert sr.round_elem(a, "fp32") is a and sr.round_elem(a, None) is a


# ---- the weights ---------------------------------------------------------------------------------------------------------------------------

def test_weights_have_the_schema_and_one_entry_per_output_channel():
    from vnect_amd.weights import check_schema, schema
    for s in range(sr.SETS):
        w = sr.weights(s)
        check_schema(w)
        assert set(w) == {n for n, _ in schema()}
        for name, a in w.items():
            leaf = name.split("/")[1]
            if leaf == "weights":
                assert np.array_equal((a != 0).sum((0, 1, 2)), np.ones(a.shape[3])) and set(np.unique(a)) <= {-1.0, 0.0, 1.0}
            elif leaf == "biases":
                assert not a.any()
        assert np.array_equal((w["res5c_branch2c/kernel"] != 0).sum((0, 1, 2)), np.ones(84))
        for scope in ("res5c_branch2a", "res5c_branch1a"):     # one tap per output-parity class
            k = w[scope + "/kernel"]
            for py in (0, 1):
                for px in (0, 1):
                    assert np.all((k[list(sr.DECONV_TAPS[py])][:, list(sr.DECONV_TAPS[px])] != 0).sum((0, 1, 3)) == 1)
        assert np.all(layer_ref.fold_bn(w)[1] == np.float32(2.0)) and not layer_ref.fold_bn(w)[0].any() and not layer_ref.fold_bn(w)[2].any()


def test_signs_are_negative_only_where_there_is_no_relu():
    relu = {scope: r for scope, _, _, _, r in sr.CONVS}
    from vnect_amd.weights import CONV_LAYERS
    assert sorted(sr.CONVS) == sorted((s, k, ci, co, a == "relu") for s, k, ci, co, a in CONV_LAYERS)   # the literal list is the schema's
    for s in range(sr.SETS):
        sel = sr.selection(s)
        for scope, r in relu.items():
            assert not r or np.all(sel[scope]["sign"] == 1), scope
            if not r:
                assert 0.2 < np.mean(sel[scope]["sign"] < 0) < 0.8, scope
        assert np.all(sel["res5c_branch2a"]["sign"] == 1)
        assert np.mean(sr.bone_channels("res5c_branch2b", sel)) <= 0.25      # at least 3/4 of its columns select a non-bone channel


# ---- d. conditions: from the rule alone --------------------------------------------------------------------------------------------------

def test_coverage_every_tap_and_every_input_channel_of_every_layer():
    taps, chans = {}, {}
    for s in range(sr.SETS):
        sel = sr.selection(s)
        for scope, d in sel.items():
            taps.setdefault(scope, set()).update(zip(d["ky"].ravel().tolist(), d["kx"].ravel().tolist()))
            chans.setdefault(scope, set()).update(d["ci"].ravel().tolist())
    for scope, k, cin, _, _ in sr.CONVS + [sr.HEAD]:
        assert len(taps[scope]) == k * k and chans[scope] == set(range(cin)), scope
    for scope, cin, _ in sr.DECONVS:
        assert len(taps[scope]) == 16 and chans[scope] == set(range(cin)), scope


@pytest.mark.parametrize("set_index,paper", COMBOS)
def test_density_distinctness_and_range(set_index, paper):
    """every gated tensor: >= 15 % non-zero, >= 25 % of the elements differ from their right and from their lower neighbour; magnitudes
    below 2^24 -- and below 2^11 in the simulated 16-bit chains, so that fp16 stores are exact and nothing nears its infinity"""
    sel = sr.selection(set_index, paper)
    for name, a in _chain(set_index, paper).items():
        if name == "input":
            continue
        a = np.asarray(a, np.float64)
        assert (a != 0).mean() >= 0.15, (name, (a != 0).mean())
        assert (a[:, :, 1:] != a[:, :, :-1]).mean() >= 0.25 and (a[:, 1:] != a[:, :-1]).mean() >= 0.25, name
        assert np.abs(a).max() < 2.0 ** 8, (name, np.abs(a).max())
        # below 2^8 even bf16's stores are exact: the simulated 16-bit chains ARE this chain (so its figures are theirs), the bone
        # columns and what is derived from them aside, and those stay finite and below 2^11
        b = sr.bone_channels(name, sel)
        keep = slice(None) if b is None else ~b
        for elem in ("bf16", "fp16"):
            c = np.asarray(_chain(set_index, paper, elem)[name], np.float64)
            assert np.array_equal(a[..., keep], c[..., keep]), (name, elem)
            assert np.all(np.isfinite(c)) and np.abs(c).max() < 2.0 ** 11, (name, elem)


def test_wide_batch_makes_bf16_stores_round_and_keeps_the_conditions():
    """the batch of the *_wide GPU configurations (set 0): its simulated bf16 chain differs from the fp32 chain (stores past 2^8 round, ties
    among them), stays below 2^11 -- far from 2^15 -- and keeps density and distinctness; its fp16 chain is still the fp32 chain"""
    sel, table = sr.selection(0), TABLES[False]
    x = sr.batch(0, 1, *sr.WIDE)
    assert x.min() == sr.WIDE[0] and x.max() == sr.WIDE[1]
    c32, cb, ch = (sr.chain(x, sel, table, e) for e in (None, "bf16", "fp16"))
    rounded = ties = 0
    for name in table:
        if name == "input":
            continue
        b = np.asarray(cb[name], np.float64)
        assert (b != 0).mean() >= 0.15 and (b[:, :, 1:] != b[:, :, :-1]).mean() >= 0.25 and (b[:, 1:] != b[:, :-1]).mean() >= 0.25, name
        assert np.abs(b).max() < 2.0 ** 11 and np.abs(np.asarray(c32[name], np.float64)).max() < 2.0 ** 11, name
        bone = sr.bone_channels(name, sel)
        keep = slice(None) if bone is None else ~bone
        assert np.array_equal(np.asarray(c32[name])[..., keep], np.asarray(ch[name])[..., keep]), name
        if table[name][0] == "conv" and len(table[name][1]) == 2:          # a block output: the sum, before its store rounds
            v = sr.expected(name, {t: cb[t] for t in table[name][1]}, sel, table, None)
            rounded += int((v != b).sum())
            ties += int(((v > 256) & (v < 512) & (v % 2 == 1)).sum() + ((v > 512) & (v % 4 == 2)).sum())
    assert rounded > 1000 and ties > 100, (rounded, ties)


# ---- b, c. the restatements against the rule ----------------------------------------------------------------------------------------------

def _per_tensor(tensors, sel, table, who, bn_scale=None):
    """every tensor of `tensors` == expected() of ITS OWN input tensors; bone columns within 3 u (bn_scale: a BN scale other than 2.0)"""
    n = 0
    for name in table:
        if name == "input":
            continue
        got = np.asarray(tensors[name])
        want = sr.expected(name, {t: tensors[t] for t in set(table[name][1])}, sel, table)
        assert got.shape == want.shape, (who, name)
        if name == "res5c_branch2a_feat":
            if bn_scale is not None:
                want[..., :128] = want[..., :128] / 2 * bn_scale
            assert np.array_equal(got[..., :191], want[..., :191]), (who, name)
            assert np.all(np.abs(got[..., sr.BONE] - want[..., sr.BONE]) <= layer_ref.BONE_N * layer_ref.U * want[..., sr.BONE]), (who, name)
        else:
            assert np.array_equal(got, want), (who, name, int((got != want).sum()))
        n += 1
    return n


@pytest.mark.parametrize("set_index,paper", COMBOS)
def test_oracle_torch_net_and_layer_ref_equal_the_rule(set_index, paper):
    import oracle
    import torch
    from tests import torch_net
    table, sel = TABLES[paper], sr.selection(set_index, paper)
    w, x = sr.weights_from(sel), sr.batch(set_index, 1)
    net = oracle.Oracle(w, keep=True, paper_res2c=paper)
    maps = net.forward(x)
    o = {name: (x if name == "input" else net.activation(name)) for name in table}
    assert np.array_equal(maps, o["res5c_branch2c"])
    assert _per_tensor(o, sel, table, "oracle") == len(table) - 1
    # torch_net folds nothing: in float64 its BN scale is 1 / sqrt(float64(variance) + 0.001) = 2 (1 - 2.6e-8), not the 2.0 that the
    # fp32 graph, the oracle, the device and layer_ref.fold_bn hold.  So in float64 its raw transposed conv is held to the rule and its
    # BN columns to relu(d * that scale), computed here in the same two operations; in float32 (0.249 + 0.001 rounds to 0.25) it is exact.
    s64 = 1.0 / np.sqrt(np.float64(sr.BN_VARIANCE) + 0.001)
    assert s64 != 2.0 and abs(s64 - 2.0) < 1e-7
    for dtype in (torch.float64, torch.float32):
        taps = {}
        tmaps = torch_net.forward(w, x, paper_res2c=paper, dtype=dtype, taps=taps)
        t = {name: (x if name == "input" else taps[name].numpy()) for name in table}
        assert np.array_equal(tmaps.numpy(), t["res5c_branch2c"])
        if dtype == torch.float64:
            d = sr.gather_deconv(sr._exact(t["res5b_branch2c_new"]), sel["res5c_branch2a"])
            assert np.array_equal(taps["res5c_branch2a"].numpy(), d)
            assert np.array_equal(t["res5c_branch2a_feat"][..., :128], np.maximum(d * s64, 0))
        assert _per_tensor(t, sel, table, "torch_net", bn_scale=s64 if dtype == torch.float64 else None) == len(table) - 1
    # layer_ref.reference on the oracle's tensors (float64; its bone columns come from the feat tensor it is given)
    r = {"input": x}
    for name in table:
        if name != "input":
            ref = layer_ref.reference(name, o, w, table)
            r[name] = ref["exact"] if "exact" in ref else ref["y"]
            want = sr.expected(name, {t_: o[t_] for t_ in set(table[name][1])}, sel, table)
            keep = slice(0, 191) if name == "res5c_branch2a_feat" else slice(None)
            assert np.array_equal(r[name][..., keep], want[..., keep]), ("layer_ref", name)
    # c. end to end: the final maps from the batch alone, apart from the bone-derived columns
    ch = _chain(set_index, paper)
    for name in table:
        b = sr.bone_channels(name, sel)
        keep = slice(None) if b is None else ~b
        assert np.array_equal(o[name][..., keep], np.asarray(ch[name])[..., keep]), name
        assert np.array_equal(t[name][..., keep], np.asarray(ch[name])[..., keep]), name
    assert 63 <= int((~sr.bone_channels("res5c_branch2c", sel)).sum()) < 84


# ---- e. planted faults on a numpy stand-in --------------------------------------------------------------------------------------------------

def _standin(name, acts, w, table, fault=None):
    """A device stand-in: tensor `name` from the WEIGHT arrays (their non-zero entries, found here -- not the selection), with one fault."""
    op, ins, p = table[name]
    x = np.asarray(acts[ins[0]], np.float64)
    N, H, W, _ = x.shape

    def conv(wt, k, stride):
        before, after = {7: (2, 3), 3: (1, 1), 1: (0, 0)}[k]
        off = 0
        if fault == "conv1_pad_3_2" and k == 7:
            before, after = 3, 2
        if fault == "odd_pixels" and stride == 2 and k == 1:
            off = 1
        if fault == "ky_kx_swapped" and k > 1:
            wt = wt.transpose(1, 0, 2, 3)
        if fault == "channels_swapped_in_a_group" and name == "res3b_branch2b":
            wt = wt.copy()
            wt[:, :, [35, 43]] = wt[:, :, [43, 35]]       # input channels 3 and 11 of the third 16-channel group
        Ho, Wo = -(-H // stride), -(-W // stride)
        xp = np.zeros((N, H + before + after + off, W + before + after + off, x.shape[3]))
        xp[:, before:before + H, before:before + W] = x
        if fault == "top_halo_wraps" and k == 3:
            xp[:, 0, before:before + W] = x[:, H - 1]
        out = np.zeros((N, Ho, Wo, wt.shape[3]))
        ky, kx, ci, co = np.nonzero(wt)
        for a, b in set(zip(ky.tolist(), kx.tolist())):
            m = (ky == a) & (kx == b)
            out[..., co[m]] += xp[:, a + off:a + off + stride * Ho:stride, b + off:b + off + stride * Wo:stride][..., ci[m]] * wt[a, b, ci[m], co[m]]
        return out

    def deconv(wt):                                     # (4, 4, Cout, Cin), scattered: out[2i - 1 + ky, 2j - 1 + kx] += in[i, j] w
        shift = 1
        if fault == "deconv_shifted":
            shift = 0
        if fault == "deconv_flipped":
            wt = wt[::-1, ::-1]
        if fault == "deconv_cout_cin_swapped":
            wt = wt.reshape(4, 4, wt.shape[3], wt.shape[2]).transpose(0, 1, 3, 2)
        big = np.zeros((N, 2 * H + 4, 2 * W + 4, wt.shape[2]))
        ky, kx, co, ci = np.nonzero(wt)
        for a, b in set(zip(ky.tolist(), kx.tolist())):
            m = (ky == a) & (kx == b)
            big[:, a:a + 2 * H:2, b:b + 2 * W:2][..., co[m]] += x[..., ci[m]] * wt[a, b, co[m], ci[m]]
        return big[:, shift:shift + 2 * H, shift:shift + 2 * W]

    if op == "pool":
        before = 1 if fault == "pool_pad_1_0" else 0
        xp = np.full((N, H + 2, W + 2, x.shape[3]), -np.inf)
        xp[:, before:before + H, before:before + W] = x
        out = np.max([xp[:, a:a + H:2, b:b + W:2] for a in range(3) for b in range(3)], 0)
    elif op == "conv":
        out = conv(np.asarray(w[p["scope"] + "/weights"], np.float64), p["k"], p["stride"])
        if len(ins) > 1:
            out = out + acts[ins[1]]
        if p["relu"]:
            out = np.maximum(out, 0)
    elif op == "head":
        out = conv(np.asarray(w["res5c_branch2c/kernel"], np.float64), 1, 1)
    else:
        bn = np.maximum(2.0 * deconv(np.asarray(w["res5c_branch2a/kernel"], np.float64)), 0)
        d = deconv(np.asarray(w["res5c_branch1a/kernel"], np.float64))
        out = np.concatenate([bn, d, np.sqrt(d[..., 0:21] ** 2 + d[..., 21:42] ** 2 + d[..., 42:63] ** 2)], -1)
    if fault == "last_four_pixels_dropped" and op in ("conv", "head") and out.shape[1] * out.shape[2] == 2116:
        out.reshape(out.shape[0], 2116, -1)[:, 2112:] = 0     # M = 2116 = 33 x 64 + 4: the partial last tile never stored
    return out


_K3 = [n for n, (op, _, p) in TABLES[False].items() if op == "conv" and p["k"] == 3]
_M2116 = ["res3a_branch2a", "res3a_branch1"] + [n for n in TABLES[False] if n.startswith("res3") and n not in ("res3a_branch2a", "res3a_branch1")] + \
    ["res5c_branch2b", "res5c_branch2c"]
FAULTS = {None: [],
          "conv1_pad_3_2": ["conv1"],
          "pool_pad_1_0": ["pool1"],
          "odd_pixels": ["res3a_branch2a", "res3a_branch1", "res4a_branch2a", "res4a_branch1"],
          "deconv_shifted": ["res5c_branch2a_feat"],
          "deconv_flipped": ["res5c_branch2a_feat"],
          "deconv_cout_cin_swapped": ["res5c_branch2a_feat"],
          "ky_kx_swapped": ["conv1"] + _K3,
          "top_halo_wraps": _K3,
          "last_four_pixels_dropped": _M2116,
          "channels_swapped_in_a_group": ["res3b_branch2b"]}


@pytest.mark.parametrize("fault", list(FAULTS), ids=[str(f) for f in FAULTS])
def test_planted_fault_fails_exactly_its_own_tensors(fault):
    """the gate as the GPU tests apply it -- each tensor against expected() of the true input tensors -- on a stand-in with one fault"""
    table, ch = TABLES[False], _chain(0)
    w = sr.weights(0)
    assert len(_K3) == 16 and len(_M2116) == 15
    failed = [name for name in table if name != "input" and not np.array_equal(_standin(name, ch, w, table, fault), ch[name])]
    assert failed == [n for n in table if n in FAULTS[fault]], (fault, failed)
