"""GPU (MI355X), through the C ABI: the PRODUCT plan's fused launches, tensor by tensor.

An arena handle -- what the benchmark and every caller run -- builds launches a keep_activations handle does not (rt_plan.cpp): the tail
GEMMs `a>b`, the chain GEMMs `a>b>c`, the stem from the frame with its PAIR form, the bone features inside the transposed conv.
VNECT_KEEP_FUSED=1 builds exactly those launches on private buffers (the seam), so every tensor they STORE can be read back.  The design
claims a fused launch sums what its stand-alone layers sum, in their order; so each stored tensor must be np.array_equal to the tensor of
that name on a handle without fused forms whose absorbed layers run whole-K 64 x 64 tiles -- and that handle passes the per-element
float64 gate of tests/layer_ref.py in the same test, which carries its bounds over to the fused plan.  S = 1, 2, 3 (67 / 133 / 199
workgroups of the wide tail; M = 2116 = 33 x 64 + 4 at one scale: a partial last tile) in every precision.
The paper wiring of res2c (paper_res2c=True, configurations paper_*; gated by layer_ref.TABLE_PAPER) builds launches the default one never
does -- in bf16 / fp16 the narrow chain res2b_branch2b>res2b_branch2c>res2c_branch2a, whose shortcut is the block input itself; in fp32 two
stand-alone 1x1 launches between three narrow tails -- and goes through the same body.
Tables: fused_plan.json in the tests' log directory (gpu_common.OUT)."""
import json
import os

import numpy as np
import pytest

from tests import layer_ref
from tests.gpu_common import BASELINE_SCALES, G, T0, _handle, _log, _native

pytestmark = pytest.mark.gpu

SCALES = {1: [1.0], 2: [1.0, 0.7], 3: BASELINE_SCALES}

# Launches that cannot sum in the order of ANY stand-alone tile shape, per precision: (which launches, why, tolerance of the tensor's
# maximum for their tensors and every tensor behind them -- test_tail_and_chain_gemms_are_bit_identical's figure for that precision).
#   fp32_split: a split-product handle multiplies by three-way bf16 splits wherever a layer runs 64 x 64 or 64 x 32 x 2 tiles (rt_plan.cpp
#   upload_layer_weights: a.x3), and those are its only whole-K shapes (hostplan.h tile_shape_ok: 32 x 32 has four K groups).  The second
#   GEMM of a fused launch -- conv.hip tail_gemm, stem.hip's PAIR GEMM -- reads fp32 weights in fragment order (plan::pack_tail) and
#   multiplies with v_mfma_f32_32x32x2_f32: other products, not another order.  The first such launch is the stem (res2a_branch2a,
#   res2a_branch1), so only `input` is in front of it.
NOT_EQUAL = {"fp32_split": (lambda name: name == "conv1" or ">" in name, "fp32-instruction tail GEMM against split products", 1e-5)}

CONFIGS = [("%s_S%d" % (prec, S), prec, S, {}, False) for prec in ("fp32", "bf16", "fp16", "fp32_split") for S in (1, 2, 3)]
CONFIGS += [("fp32_S%d_wide" % S, "fp32", S, {"VNECT_FORCE_WIDE_TAIL": "1"}, False) for S in (1, 2)]
CONFIGS += [("fp32_S3_chain", "fp32", 3, {"VNECT_FORCE_CHAIN": "1"}, False)]
CONFIGS += [("paper_%s_S%d" % (prec, S), prec, S, {}, True) for prec in ("bf16", "fp16") for S in (1, 2, 3)]
CONFIGS += [("paper_%s_S%d" % (prec, S), prec, S, {}, True) for prec in ("fp32", "fp32_split") for S in (1, 3)]
# the res2 stage of the paper wiring's arena plan, by launch name (rt_plan.cpp, the paper_res2c block): 16-bit handles chain every next
# branch2a; fp32 handles run res2b_branch2a and res2c_branch2a as launches of their own between three two-part tails
PAPER_CHAINS = ["res2a_branch2b>res2a_branch2c>res2b_branch2a", "res2b_branch2b>res2b_branch2c>res2c_branch2a", "res2c_branch2b>res2c_branch2c"]
PAPER_TAILS = ["res2a_branch2b>res2a_branch2c", "res2b_branch2a", "res2b_branch2b>res2b_branch2c", "res2c_branch2a", "res2c_branch2b>res2c_branch2c"]
RESULTS = {}


def _prec(name):
    n = _native()
    return {"fp32": n.FP32, "bf16": n.BF16, "fp16": n.FP16, "fp32_split": n.FP32_SPLIT}[name]


def _with_env(monkeypatch, env, *a, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return _handle(*a, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _plan(layers):
    return [(L["name"], L["tile_m"], L["tile_n"], L["split_k"], L["M"], L["N"], L["K"], L["workgroups"]) for L in layers]


def _stem_pair(names):
    """the stem of an arena plan runs in its PAIR form when the launch behind pool1 is res2a's 1x1 pair (rt_plan.cpp setup_stem)"""
    return names[:3] == ["conv1", "pool1", "res2a_branch2a+branch1"]


def _written(names, table=layer_ref.TABLE):
    """launch name -> tensors it stores, for the seam plan (launch order); the pair behind pool1 runs inside the PAIR stem"""
    pair = _stem_pair(names)
    out = []
    for n in names:
        if n in ("conv1", "pool1"):
            out.append((n, layer_ref.launch_tensors(n, stem=True, pair=pair, table=table)))
        else:
            out.append((n, layer_ref.launch_tensors(n, table=table)))
    return out


def _absorbed(names):
    """the stand-alone launches a fused launch of this plan stands for: the layers of every `a>b[>c]` name and the PAIR form's pair"""
    out = set()
    for n in names:
        if ">" in n:
            out.update(n.split(">"))
    if _stem_pair(names):
        out.add(names[2])
    return out


def _is_absorbed(name, absorbed):
    return name in absorbed or all(part in absorbed for part in name.split("+"))   # (res2b_branch2b+res2c_branch2b: both 3x3 layers)


def _paper_res2_stage(names, prec):
    """the paper plan's shape, by name: the launches between the stem's pair and res3a's"""
    i0, i1 = names.index("res2a_branch2a+branch1") + 1, names.index("res3a_branch2a+branch1")
    assert names[i0:i1] == (PAPER_CHAINS if prec in ("bf16", "fp16") else PAPER_TAILS), names[i0:i1]
    if prec in ("bf16", "fp16"):
        assert "res2b_branch2a" not in names and "res2c_branch2a" not in names


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_seam_plan_is_the_arena_plan(weights, monkeypatch, prec, S):
    """VNECT_KEEP_FUSED=1 on a keep_activations handle: the launches of a default arena handle, name for name and tile for tile; on an
    arena handle, and unset, it changes nothing."""
    _seam_is_arena(weights, monkeypatch, prec, S, False)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_seam_plan_is_the_arena_plan_with_paper_wiring(weights, monkeypatch, prec, S):
    """... and with paper_res2c=True: the seam handle of the paper_* configurations below runs what a paper arena handle runs."""
    _seam_is_arena(weights, monkeypatch, prec, S, True)


def _seam_is_arena(weights, monkeypatch, prec, S, paper):
    kw = dict(precision=_prec(prec), paper_res2c=paper)
    arena = _handle(SCALES[S], weights, **kw)
    keep = _handle(SCALES[S], weights, keep_activations=True, **kw)
    seam = _with_env(monkeypatch, {"VNECT_KEEP_FUSED": "1"}, SCALES[S], weights, keep_activations=True, **kw)
    arena2 = _with_env(monkeypatch, {"VNECT_KEEP_FUSED": "1"}, SCALES[S], weights, **kw)
    try:
        want = _plan(arena.layers())
        assert _plan(seam.layers()) == want
        assert _plan(arena2.layers()) == want
        if paper:
            _paper_res2_stage([x[0] for x in want], prec)
        # (one scale: the transposed conv runs 64 x 32 tiles with two K groups, which do not take the bone features)
        assert any(">" in n for n, *_ in want) and any(n == "res5c_deconv+bone_length" for n, *_ in want) == (S >= 2)
        assert not any(">" in L["name"] or "bone_length" in L["name"].split("+") for L in keep.layers())
        assert seam.timings()["conv_launches"] == arena.timings()["conv_launches"]
    finally:
        for h in (arena, keep, seam, arena2):
            h.close()


def test_default_plans_are_unchanged(weights):
    """The launches of handles built without the seam -- arena and keep_activations, every precision, S = 1, 2, 3 -- are the recorded ones
    (tests/golden/default_plans.json: name, tile, K split, M, N, K, workgroups of every launch, on the 256-CU MI355X)."""
    with open(os.path.join(G, "default_plans.json")) as f:
        golden = json.load(f)
    assert len(golden) == 24
    for key, want in sorted(golden.items()):
        prec, S, kind = key.rsplit("_", 2)
        h = _handle(SCALES[int(S[1:])], weights, precision=_prec(prec), keep_activations=kind == "keep")
        got = _plan(h.layers())
        h.close()
        assert got == [tuple(x) for x in want], key


@pytest.mark.parametrize("cid,prec,S,env,paper", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_stored_tensor_of_the_fused_plan_equals_the_plain_plans(weights, monkeypatch, cid, prec, S, env, paper):
    fused_equals_plain(weights, monkeypatch, cid, prec, S, env, paper, RESULTS, "fused_plan.json")


def fused_equals_plain(weights, monkeypatch, cid, prec, S, env, paper, results, logname=None):
    """The body of the test above, for any weights (tests/test_gpu_weight_families.py runs it on its families): every tensor the seam plan
    stores equals the plain plan's, and the plain plan passes the per-element float64 gate.  Returns the plain plan's rows."""
    import oracle
    from tests import helpers, layer_ref_f16
    n = _native()
    scales = SCALES[S]
    table = layer_ref.TABLE_PAPER if paper else layer_ref.TABLE
    fused = _with_env(monkeypatch, dict(env, VNECT_KEEP_FUSED="1"), scales, weights, precision=_prec(prec), keep_activations=True,
                      paper_res2c=paper)
    plain = None
    try:
        names = [L["name"] for L in fused.layers()]
        assert any(">" in x for x in names) and _stem_pair(names) and ("res5c_deconv+bone_length" in names) == (S >= 2), names
        absorbed = _absorbed(names)
        if paper:
            _paper_res2_stage(names, prec)
            assert ("res2c_branch2a" in absorbed) == (prec in ("bf16", "fp16"))
        pins = ";".join("%s=64,64,1,1" % x for x in sorted(absorbed))
        plain = _with_env(monkeypatch, {"VNECT_NO_TAIL": "1", "VNECT_NO_STEM": "1", "VNECT_PLAN": pins}, scales, weights,
                          precision=_prec(prec), keep_activations=True, paper_res2c=paper)
        pl = plain.layers()
        assert not any(">" in L["name"] for L in pl) and [L["name"] for L in pl][:2] == ["conv1", "pool1"]
        pinned = [L for L in pl if _is_absorbed(L["name"], absorbed)]
        # every absorbed layer is a launch of the plain plan (the two 3x3 layers that read res2b_branch2a: one dual-output launch) ...
        assert {p for L in pinned for p in ([L["name"]] if L["name"] in absorbed else L["name"].split("+"))} == absorbed
        # ... on whole-K 64 x 64 tiles
        assert all((L["tile_m"], L["tile_n"], L["split_k"]) == (64, 64, 1) for L in pinned), [x for x in _plan(pinned)]

        # what the fused plan stores, from its launch names; exactly that can be read back
        written = _written(names, table)
        stored = {"input"} | {t for _, ts in written for t in ts}
        for name in table:
            if name in stored:
                continue
            with pytest.raises(n.VnectError) as e:
                fused.activation(name)
            created = name in ("conv1", "pool1")   # tensors of the plan that the stem keeps on chip; a tail's 3x3 layer is no tensor at all
            assert e.value.code == (n.E_STATE if created else n.E_ARG), (name, e.value)
            assert name in str(e.value)
        order = [t for t in table if t in stored]   # the table is in launch order
        launch_of = {t: ln for ln, ts in reversed(written) for t in ts}

        def first_approx():
            if prec not in NOT_EQUAL:
                return None
            hit = [ts[0] for ln, ts in written if NOT_EQUAL[prec][0](ln)]
            return min(order.index(t) for t in hit) if hit else None

        approx_at = first_approx()

        def compare(tag, skip=()):
            worst = 0.0
            for i, t in enumerate(order):
                if t in skip:
                    continue
                a, b = fused.activation(t), plain.activation(t)
                assert a.shape == b.shape, (cid, tag, t)
                if approx_at is not None and i >= approx_at:
                    err = float(np.abs(a - b).max()) / float(np.abs(b).max())
                    worst = max(worst, err)
                    print("%-16s %-8s %-22s %.3g of its maximum from the plain plan's (%s)" % (cid, tag, t, err, NOT_EQUAL[prec][1]))
                    assert err <= NOT_EQUAL[prec][2], (cid, tag, t, launch_of.get(t), err)
                    continue
                if not np.array_equal(a, b):
                    d = np.abs(a - b)
                    rows = np.unique(np.nonzero(d.reshape(-1, d.shape[-1]))[0])
                    pytest.fail("%s %s: the first tensor that differs is %s (launch %s): %d of %d elements, max |d| %.3g of max %.3g, flat rows %d..%d"
                                % (cid, tag, t, launch_of.get(t), int((d != 0).sum()), d.size, float(d.max()), float(np.abs(b).max()),
                                   int(rows[0]), int(rows[-1])))
            return worst

        batch, _, _ = oracle.gen_input_batch(helpers.synth_frame(1234, smooth=True), scales)
        out_f, out_p = fused.forward(batch), plain.forward(batch)
        worst_fwd = compare("forward")
        assert np.array_equal(out_f, fused.activation("res5c_branch2c")) and np.array_equal(out_p, plain.activation("res5c_branch2c"))
        acts = {name: plain.activation(name) for name in table}
        # one frame whose squarify step is a copy (long side 368): the stem builds the pyramid from the frame, the batch tensor is not written
        frame = helpers.synth_frame(91 + S, 368, 300, smooth=True)
        jf, jp = fused.infer(frame, T0 + 5, T0 + 5.001), plain.infer(frame, T0 + 5, T0 + 5.001)
        worst_inf = compare("infer", skip=("input",))
        if approx_at is None:
            assert np.array_equal(jf[0], jp[0]) and np.array_equal(jf[1], jp[1]), cid
    finally:
        fused.close()
        if plain is not None:
            plain.close()

    # the plain plan inside its float64 bounds, per element
    if prec == "fp16":
        rows = layer_ref_f16.check_all(acts, weights, batch, table=table)
    else:
        split = set()
        if prec == "fp32_split":
            for L in pl:
                if L["M"] and L["tile_m"] == 64 and L["tile_n"] in (32, 64) and L["name"] != "conv1":
                    split.update(layer_ref.launch_tensors(L["name"], table=table))
        rows = layer_ref.check_all(acts, weights, prec, batch, split_tensors=split, table=table)
    results[cid] = dict(prec=prec, scales=scales, env=env, paper_res2c=paper, fused_launches=names, stored=order, pinned=sorted(absorbed),
                        equal=order if approx_at is None else order[:approx_at], worst_of_max=dict(forward=worst_fwd, infer=worst_inf),
                        plain_rows=rows)
    if logname:
        _log(logname, results)
    assert len(rows) == len(table)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad[:4]
    return rows
