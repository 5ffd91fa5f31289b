"""GPU (MI355X), through the C ABI: the fp16 precision (VNECT_FP16) -- the bf16 plan launch for launch with fp16 elements.

The plan equals the bf16 handle's; every readable tensor stays within the fp16 per-element bounds (tests/layer_ref_f16.py); the final maps
sit at most 1/4 of bf16's error from the fp32 handle's; planted joints with a real maximum land in the fp32 cell; pre-processing, the fused
stem and every execution mode are bit-identical where they should be; refusals and read-back behave.  Worst ratios: fp16_bounds.json and
fp16_accuracy.json in the tests' log directory (gpu_common.OUT)."""
import numpy as np
import pytest

from tests import layer_ref, layer_ref_f16
from tests.gpu_common import BASELINE_SCALES, T0, _handle, _log, _native, _read_table

pytestmark = pytest.mark.gpu

# fp16 final-map gate, of the fp32 handle's map maximum: profiles/fp16_rate.txt measures fp16 at <= 1/8 of bf16's 1.1-2.3e-2 over the
# nine weight sets of profiles/r06_bf16_gate_spread.txt; bf16's gate (3e-2) has 1.3x headroom over its spread, this one more.
EPS16 = 7.5e-3
SIX = [1.0, 0.95, 0.9, 0.8, 0.7, 0.6]
EIGHT = [1.0, 0.93, 0.86, 0.79, 0.72, 0.65, 0.58, 0.45]   # VNECT_MAX_SCALES images
TILES = ["64,64,1,1", "64,32,2,1", "32,32,4,1", "64,64,1,5", "64,32,2,2", "32,32,4,3"]


def _configs():
    c = [("base_square", BASELINE_SCALES, "square", {}, "synthetic"), ("base_300x368", BASELINE_SCALES, "300x368", {}, "synthetic")]
    for scales in ([1.0], [1.0, 0.7], [1, 0.85, 0.7, 0.5], SIX, EIGHT):
        c.append(("S%d" % len(scales), scales, "square", {}, "synthetic"))
    for force in TILES:
        c.append(("tile%s" % force.replace(",", "x"), [1.0, 0.7], "square", {"VNECT_FORCE_TILE": force, "VNECT_NO_STEM": "1"}, "synthetic"))
    c.append(("stem", BASELINE_SCALES, "square", {"VNECT_FORCE_STEM": "batch"}, "synthetic"))
    c.append(("seed7", BASELINE_SCALES, "square", {}, "seed7"))
    c.append(("planted", BASELINE_SCALES, "planted", {}, "planted"))
    c = [x + (False,) for x in c]
    # the paper wiring of res2c (paper_res2c=True; layer_ref.TABLE_PAPER)
    c.append(("paper_base", BASELINE_SCALES, "square", {}, "synthetic", True))
    c.append(("paper_S1", [1.0], "square", {}, "synthetic", True))
    return c


CONFIGS = _configs()
RESULTS = {}
PAPER = []   # the configurations with paper_res2c=True


def _weights(kind, default):
    from tests import planted
    from vnect_amd.weights import synthetic_weights
    return synthetic_weights(seed=7) if kind == "seed7" else (planted.weights() if kind == "planted" else default)


def _frame(kind):
    from tests import helpers, planted
    if kind == "square":
        return helpers.synth_frame(1234, smooth=True)
    if kind == "planted":
        return planted.frame(301)[0]
    return helpers.synth_frame(4242, 300, 368, smooth=True)


def _plan(layers):
    return [(L["name"], L["M"], L["N"], L["K"], L["tile_m"], L["tile_n"], L["split_k"], L["workgroups"]) for L in layers]


@pytest.mark.parametrize("scales,paper", [([1.0], False), ([1.0, 0.7], False), (BASELINE_SCALES, False), (SIX, False),
                                          ([1.0], True), (BASELINE_SCALES, True)], ids=["S1", "S2", "S3", "S6", "paper_S1", "paper_S3"])
def test_fp16_plan_is_the_bf16_plan(weights, scales, paper):
    n = _native()
    hb = _handle(scales, weights, precision=n.BF16, stream_batch=2 if len(scales) <= 4 else 1, paper_res2c=paper)
    hh = _handle(scales, weights, precision=n.FP16, stream_batch=2 if len(scales) <= 4 else 1, paper_res2c=paper)
    assert _plan(hh.layers()) == _plan(hb.layers())
    # (the paper wiring's own chain launch, in the scale plan and the batched one)
    assert any(L["name"] == "res2b_branch2b>res2b_branch2c>res2c_branch2a" for L in hh.layers()) == paper
    if len(scales) <= 4:
        assert _plan(hh.batch_layers()) == _plan(hb.batch_layers())
    hb.close(), hh.close()


@pytest.mark.parametrize("cid,scales,frame,env,wkind,paper", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fp16_every_tensor_within_its_element_bounds(weights, monkeypatch, cid, scales, frame, env, wkind, paper):
    import oracle
    n = _native()
    w = _weights(wkind, weights)
    table = layer_ref.TABLE_PAPER if paper else layer_ref.TABLE
    batch, _, _ = oracle.gen_input_batch(_frame(frame), scales)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = _handle(scales, w, precision=n.FP16, keep_activations=True, paper_res2c=paper)
    for k in env:
        monkeypatch.delenv(k)
    try:
        launches = h.layers()
        out = h.forward(batch)
        acts = _read_table(h, unwritten=("conv1",) if "VNECT_FORCE_STEM" in env else (), table=table)
    finally:
        h.close()
    assert np.array_equal(out, acts["res5c_branch2c"])
    stem = "VNECT_FORCE_STEM" in env
    rows = layer_ref_f16.check_all(acts, w, batch, stem=stem, table=table)
    checked = {r["tensor"] for r in rows}
    uncovered = [L["name"] for L in launches if not set(layer_ref.launch_tensors(L["name"], stem, table=table)) & checked]
    names = [L["name"] for L in launches]
    RESULTS[cid] = rows
    if paper:
        PAPER.append(cid)
    worst = {k: max((r[k], c, r["tensor"]) for c, rs in RESULTS.items() for r in rs) for k in ("rig", "cal")}
    low = min((r["match"], c, r["tensor"]) for c, rs in RESULTS.items() for r in rs if r["match"] is not None)
    _log("fp16_bounds.json", dict(match_floor=layer_ref_f16.MATCH_FLOOR_F16, worst=worst, lowest_match=low, paper_res2c=PAPER,
                                  configs=RESULTS))
    for r in rows:
        print("%-16s %-22s rigorous %.3g calibrated %.3g match %s" % (cid, r["tensor"], r["rig"], r["cal"],
                                                                       "-" if r["match"] is None else "%.5f" % r["match"]))
    assert not uncovered, uncovered
    if paper:
        assert "res2c_branch2a" in names and not any("res2b_branch2b+res2c_branch2b" in x for x in names), names
    assert len(rows) == len(table) - (1 if stem else 0)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad[:4]


def test_fp16_error_is_a_quarter_of_bf16s(weights):
    """Same frames, same weights: fp16's final-map error against the fp32 handle is at most 1/4 of bf16's on every frame (the rounding
    units say 1/8; a bf16 conversion left anywhere in the fp16 path would put the ratio near 1), and within EPS16 of the map maximum."""
    import oracle
    from tests import helpers
    from vnect_amd.weights import synthetic_weights
    n = _native()
    rows = []
    for wname, w in (("default", weights), ("seed3", synthetic_weights(seed=3))):
        hs = {p: _handle(BASELINE_SCALES, w, precision=p) for p in (n.FP32, n.BF16, n.FP16)}
        for k, f in enumerate([helpers.synth_frame(1234, smooth=True), helpers.synth_frame(77), helpers.synth_frame(9, 300, 420, smooth=True)]):
            batch, _, _ = oracle.gen_input_batch(f, BASELINE_SCALES)
            m32, mb, mh = (hs[p].forward(batch) for p in (n.FP32, n.BF16, n.FP16))
            top = float(np.abs(m32).max())
            eb, eh = float(np.abs(mb - m32).max()) / top, float(np.abs(mh - m32).max()) / top
            rows.append((wname, k, eb, eh, eh / eb))
            print("%-8s frame %d: bf16 %.3g fp16 %.3g of max (ratio %.3f)" % (wname, k, eb, eh, eh / eb))
        for h in hs.values():
            h.close()
    _log("fp16_accuracy.json", rows)
    assert all(eb <= 3e-2 for _, _, eb, _, _ in rows), rows   # (bf16 within its own gate: the ratio below means something)
    assert all(eh <= 0.25 * eb for _, _, eb, eh, _ in rows), rows
    assert all(eh <= EPS16 for _, _, _, eh, _ in rows), rows


def test_fp16_margin_conditioned_joints():
    """test_bf16_margin_conditioned_joints with fp16 and EPS16: planted peaks, 16 frames, every joint whose fp32 maximum clears the rest of
    its map by more than 2 EPS16 has its fp16 arg-max in the fp32 cell; at least 240 such pairs (bf16's count on these frames)."""
    import oracle
    from tests import planted
    from tests.test_planted import cell_margin
    n = _native()
    pw = planted.weights()
    hh = _handle(BASELINE_SCALES, pw, precision=n.FP16)
    hf = _handle(BASELINE_SCALES, pw)
    shapes = [(368, 368), (538, 368), (240, 320), (368, 300)]
    pairs, map_err, worst3 = 0, 0.0, 0.0
    for k in range(16):
        H, W = shapes[k % 4]
        frame, centres = planted.frame(300 + k, H, W)
        want = planted.expected(centres)
        scaler = 368.0 / max(H, W)
        t = T0 + 900 + k
        hh.reset_filters(), hf.reset_filters()
        j2h, j3h = hh.infer(frame, t, t + 0.001)
        mh = hh.activation("res5c_branch2c")
        j2f, _ = hf.infer(frame, t, t + 0.001)
        mf = hf.activation("res5c_branch2c")
        assert np.abs(j2h - want).max() <= 8.0 / scaler, k
        top = float(np.abs(mf).max())
        eps = EPS16 * top
        map_err = max(map_err, float(np.abs(mh - mf).max()) / top)
        assert float(np.abs(mh - mf).max()) <= eps, k
        avg_f, avg_h = oracle.merge_scales(mf, BASELINE_SCALES), oracle.merge_scales(mh, BASELINE_SCALES)
        raw_f, raw_h = oracle.extract_2d(avg_f[0]), oracle.extract_2d(avg_h[0])
        for j in range(21):
            up = oracle.resize(np.ascontiguousarray(avg_f[0][:, :, j]), 8.0)
            assert up[int(raw_h[j, 0]), int(raw_h[j, 1])] >= up.max() - 2 * eps, (k, j)
            if cell_margin(up, raw_f[j]) > 2 * eps:
                pairs += 1
                assert np.all(raw_h[j] // 8 == raw_f[j] // 8), (k, j)
        at_h = oracle.extract_3d(raw_h, avg_f[1], avg_f[2], avg_f[3])
        assert np.array_equal(oracle.extract_3d(raw_h, avg_h[1], avg_h[2], avg_h[3]), j3h), k
        amp = 1.0 + 2 * (7.0 / 16)
        bound3 = 2 * (eps * 100) * amp * amp
        d3 = float(np.abs(j3h.astype(np.float64) - at_h).max())
        worst3 = max(worst3, d3 / bound3)
        assert d3 <= bound3, (k, d3, bound3)
    print("fp16 margin gate: %d of %d (frame, joint) pairs clear 2 eps16 (all in the fp32 cell); fp16 map error %.3g of max; 3-D %.2f of its bound"
          % (pairs, 16 * 21, map_err, worst3))
    _log("fp16_margin_pairs.json", {"pairs": pairs, "map_err": map_err, "worst_3d_over_bound": worst3})
    assert pairs >= 240, pairs
    hh.close(), hf.close()


def test_fp16_preprocessing_and_fused_stem_are_exact(weights, monkeypatch):
    import oracle
    from tests import helpers
    n = _native()
    h = _handle(BASELINE_SCALES, weights, precision=n.FP16, keep_activations=True)
    big = helpers.synth_frame(21, 400, 500)
    for f in (helpers.synth_frame(5, smooth=True), helpers.synth_frame(6, 300, 420), big[17:317, 9:409]):
        got, s, off = h.preprocess(f)
        rb, rs, roff = oracle.gen_input_batch(np.ascontiguousarray(f), BASELINE_SCALES)
        assert s == rs and off == roff and np.array_equal(got, rb.astype(np.float16).astype(np.float32))
    frames = [helpers.synth_frame(31, smooth=True), helpers.synth_frame(32, 538, 368, smooth=True), helpers.synth_frame(33, 240, 320)]
    want = []
    for k, f in enumerate(frames):
        want.append(h.infer(f, T0 + k, T0 + k + 0.001) + (h.activation("pool1"), h.activation("res5c_branch2c")))
    h.close()
    for env in ({"VNECT_FORCE_STEM": "batch"}, {"VNECT_FORCE_STEM": "frame"}, {"VNECT_NO_STEM": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = _handle(BASELINE_SCALES, weights, precision=n.FP16, keep_activations=True)
        for k in env:
            monkeypatch.delenv(k)
        for k, f in enumerate(frames):
            j2, j3 = g.infer(f, T0 + k, T0 + k + 0.001)
            assert np.array_equal(g.activation("pool1"), want[k][2]) and np.array_equal(g.activation("res5c_branch2c"), want[k][3]), (env, k)
            assert np.array_equal(j2, want[k][0]) and np.array_equal(j3, want[k][1]), (env, k)
        g.close()


def test_fp16_execution_modes_are_bit_identical(weights):
    import oracle
    from tests import helpers
    n = _native()
    batch, _, _ = oracle.gen_input_batch(helpers.synth_frame(1234, smooth=True), BASELINE_SCALES)
    arena = _handle(BASELINE_SCALES, weights, precision=n.FP16)
    plain = _handle(BASELINE_SCALES, weights, precision=n.FP16, keep_activations=True)
    assert np.array_equal(arena.forward(batch), plain.forward(batch))
    plain.close()
    frames = [helpers.synth_frame(500 + k, *((368, 368), (300, 420))[k % 2], smooth=True) for k in range(10)]
    ts = [T0 + 2000 + k / 30 for k in range(10)]
    arena.reset_filters()
    eager = [arena.infer(f, t, t + 0.001) for f, t in zip(frames, ts)]
    arena.close()
    graph = _handle(BASELINE_SCALES, weights, precision=n.FP16, use_graph=True)
    got = [graph.infer(f, t, t + 0.001) for f, t in zip(frames, ts)]
    graph.close()
    lanes = _handle(BASELINE_SCALES, weights, precision=n.FP16, lanes=3, num_frame_slots=8)
    deep = []
    for k, (f, t) in enumerate(zip(frames, ts)):
        lanes.upload_frame(k % 8, f)
        if k >= 3:
            deep.append(lanes.collect())
        lanes.submit_resident(k % 8, t, t + 0.001)
    deep += [lanes.collect() for _ in range(3)]
    lanes.close()
    for k in range(10):
        for other in (got, deep):
            assert np.array_equal(eager[k][0], other[k][0]) and np.array_equal(eager[k][1], other[k][1]), k
    # two streams per launch: each stream's joints equal a handle of its own
    vids = [[helpers.synth_frame(9100 + k, smooth=True) for k in range(4)], [helpers.synth_frame(9200 + k, 368, 300, smooth=True) for k in range(4)]]
    own = []
    for s in range(2):
        h = _handle(BASELINE_SCALES, weights, precision=n.FP16)
        own.append([h.infer(vids[s][k], T0 + 7 * s + k / 30, T0 + 7 * s + k / 30 + 0.0005) for k in range(4)])
        h.close()
    hb = _handle(BASELINE_SCALES, weights, precision=n.FP16, stream_batch=2, num_frame_slots=8)
    for k in range(4):
        t = [T0 + 7 * s + k / 30 for s in range(2)]
        res = hb.infer_streams([vids[0][k], vids[1][k]], t, [x + 0.0005 for x in t])
        for s in range(2):
            assert np.array_equal(res[s][0], own[s][k][0]) and np.array_equal(res[s][1], own[s][k][1]), (s, k)
    hb.close()


def test_fp16_refusals_and_read_back(weights):
    import oracle
    from tests import helpers
    n = _native()
    with pytest.raises(n.VnectError) as e:
        n.Handle(BASELINE_SCALES, precision=4)
    assert e.value.code == n.E_ARG
    w = {k: np.array(v, copy=True) for k, v in weights.items()}
    w["res4c_branch2b/weights"].flat[123] = 1e5
    h = n.Handle(BASELINE_SCALES, precision=n.FP16)
    h.set_weights(w)
    with pytest.raises(n.VnectError) as e:
        h.finalize()
    assert e.value.code == n.E_ARG and "res4c_branch2b/weights" in str(e.value)
    h.close()
    _handle(BASELINE_SCALES, w, precision=n.BF16).close()   # bf16 accepts it, as it always did
    h = _handle(BASELINE_SCALES, weights, precision=n.FP16, keep_activations=True)
    batch, _, _ = oracle.gen_input_batch(helpers.synth_frame(1234, smooth=True), BASELINE_SCALES)
    maps = h.forward(batch)
    for name in ("input", "pool1", "res2a", "res4f", "res5c_branch2a_feat", "res5c_branch2b"):
        a = h.activation(name)
        assert np.array_equal(a, a.astype(np.float16).astype(np.float32)), name
    assert not np.array_equal(maps, maps.astype(np.float16).astype(np.float32))   # the final maps are fp32
    h.close()
