"""GPU (MI355X), through the C ABI: the ARENA plan of the paper wiring (vnect_config::paper_res2c = 1) and every way of running a frame on it.

The per-element gate (tests/test_gpu_layer_bounds.py, test_gpu_fp16.py: paper_*) and the equality gate (tests/test_gpu_fused_plan.py: paper_*)
hold the paper wiring's launches on private buffers.  What callers run shares an arena, and there the switch changes tensor lifetimes --
res2b_branch2a dies one block earlier, res2c_branch2a lives -- in the scale plan, in the batched plan of two streams and in every plan
built again behind a change of scales.  So, per precision at the baseline scales: the seam handle of the equality gate (VNECT_KEEP_FUSED=1:
the arena plan's launches, each tensor in a buffer of its own) is the reference, computed once, and an arena handle -- eager, graph replay,
three lanes, two streams per launch, after vnect_set_scales, after the facade reopened it at another number of scales -- must return its
final maps and joints BIT FOR BIT (all handles of a test share the precision, so this holds for fp32_split too).  The fp32 facade runs the
end-to-end gate against the oracle with the paper wiring; bf16 and fp16 final maps are held to the fp32 paper handle's with the map
tolerances of test_bf16_path_gated_against_fp32 / test_fp16_error_is_a_quarter_of_bf16s; and the same handle without the switch must be
far away (the two wirings differ by 0.40 of the final maps' maximum on the CPU: tests/torch_net.py, one scale).
Figures: paper_wiring.json in the tests' log directory (gpu_common.OUT)."""
import numpy as np
import pytest

from tests.gpu_common import BASELINE_SCALES, T0, _EndToEnd, _handle, _log, _native
from tests.test_gpu_fp16 import EPS16

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16", "fp16", "fp32_split"]
FOUR = [1.0, 0.9, 0.75, 0.6]
# two non-square frames among the first four; a long side of 368 makes the squarify step a copy, so the stem builds the pyramid from the frame
SHAPES = [(368, 368), (368, 300), (240, 320), (368, 368), (300, 368), (368, 368)]
CHAIN = "res2b_branch2b>res2b_branch2c>res2c_branch2a"
_REF = {}
FIGURES = {}


def _prec(name):
    n = _native()
    return {"fp32": n.FP32, "bf16": n.BF16, "fp16": n.FP16, "fp32_split": n.FP32_SPLIT}[name]


def _frames():
    from tests import helpers
    return [np.ascontiguousarray(helpers.synth_frame(6100 + k, H, W, smooth=True)) for k, (H, W) in enumerate(SHAPES)]


def _times(k):
    t = T0 + 3000 + k / 30 + 0.002 * (k % 3)
    return t, t + 0.001


def _plan(layers):
    return [(L["name"], L["tile_m"], L["tile_n"], L["split_k"], L["M"], L["N"], L["K"], L["workgroups"]) for L in layers]


def _paper(scales, weights, prec, **kw):
    return _handle(scales, weights, precision=_prec(prec), paper_res2c=True, **kw)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _carries_res2c_branch2a(names, prec):
    """res2c_branch2a in the form the precision's arena plan gives it: chained behind res2b's tail on 16-bit handles, a launch of its own else"""
    return (CHAIN in names and "res2c_branch2a" not in names) if prec in ("bf16", "fp16") else ("res2c_branch2a" in names and CHAIN not in names)


def _reference(prec, weights):
    """The seam handle's results at the baseline scales, once per precision: batches and final maps of `forward` for every frame, joints of
    `infer` over the six frames as one video, the maps behind each `infer`, the plan."""
    if prec in _REF:
        return _REF[prec]
    import oracle
    frames = _frames()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VNECT_KEEP_FUSED", "1")
        seam = _paper(BASELINE_SCALES, weights, prec, keep_activations=True)
    try:
        plan = _plan(seam.layers())
        names = [x[0] for x in plan]
        assert _carries_res2c_branch2a(names, prec) and not any("res2b_branch2b+res2c_branch2b" in x for x in names), names
        batches = [oracle.gen_input_batch(f, BASELINE_SCALES)[0] for f in frames]
        maps = [seam.forward(b) for b in batches]
        joints, infer_maps = [], []
        for k, f in enumerate(frames):
            joints.append(seam.infer(f, *_times(k)))
            infer_maps.append(seam.activation("res5c_branch2c"))
    finally:
        seam.close()
    _REF[prec] = dict(frames=frames, batches=batches, maps=maps, joints=joints, infer_maps=infer_maps, plan=plan)
    return _REF[prec]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("prec", PRECS)
def test_paper_arena_handle_equals_the_seam_handle(weights, prec, graph):
    """An arena handle, use_graph = 0 and 1: the seam's plan launch for launch, and over four frames the seam's final maps from `forward` and
    its joints (and the maps behind them) from `infer`."""
    ref = _reference(prec, weights)
    h = _paper(BASELINE_SCALES, weights, prec, use_graph=graph)
    try:
        assert _plan(h.layers()) == ref["plan"]
        for k in range(4):
            assert np.array_equal(h.forward(ref["batches"][k]), ref["maps"][k]), ("forward", k)
        for k in range(4):
            got = h.infer(ref["frames"][k], *_times(k))
            assert np.array_equal(h.activation("res5c_branch2c"), ref["infer_maps"][k]), ("infer maps", k, SHAPES[k])
            assert _same(got, ref["joints"][k]), ("infer", k, SHAPES[k])
    finally:
        h.close()


@pytest.mark.parametrize("prec", PRECS)
def test_paper_frames_three_deep_on_three_lanes(weights, prec):
    """lanes=3: three arenas, six frames submitted three deep; collected, they are the frame-by-frame results."""
    ref = _reference(prec, weights)
    h = _paper(BASELINE_SCALES, weights, prec, lanes=3, num_frame_slots=8)
    try:
        got = []
        for k, f in enumerate(ref["frames"]):
            h.upload_frame(k, f)
            if k >= 3:
                got.append(h.collect())
            h.submit_resident(k, *_times(k))
        got += [h.collect() for _ in range(3)]
    finally:
        h.close()
    for k in range(6):
        assert _same(got[k], ref["joints"][k]), k


@pytest.mark.parametrize("prec", PRECS)
def test_paper_two_streams_per_launch(weights, prec):
    """vnect_set_stream_batch(h, 2): the batched plan (2 S images) lists res2c_branch2a in the scale plan's form; `forward` of 2 S images
    equals two forwards; streams 0 and 1 submitted as three batches equal handles of their own (stream 0: the reference video's first
    three frames; stream 1: its last three on a fresh handle)."""
    ref = _reference(prec, weights)
    own = _paper(BASELINE_SCALES, weights, prec)
    h = _paper(BASELINE_SCALES, weights, prec, stream_batch=2, num_frame_slots=8)
    try:
        want1 = [own.infer(ref["frames"][k], *_times(k)) for k in (3, 4, 5)]
        single, batched = h.layers(), h.batch_layers()
        assert _plan(single) == ref["plan"]
        names = [L["name"] for L in batched]
        assert names == [L["name"] for L in single] and _carries_res2c_branch2a(names, prec), names
        for a, b in zip(single, batched):
            assert (b["tile_m"], b["tile_n"], b["split_k"], b["N"], b["K"], b["M"]) == (a["tile_m"], a["tile_n"], a["split_k"], a["N"], a["K"], 2 * a["M"]), a["name"]
        both = h.forward(np.concatenate([ref["batches"][1], ref["batches"][2]]))
        assert np.array_equal(both, np.concatenate([ref["maps"][1], ref["maps"][2]]))
        assert np.array_equal(h.forward(ref["batches"][1]), ref["maps"][1])
        for k in range(3):
            (ta, ta3), (tb, tb3) = _times(k), _times(k + 3)
            h.upload_frame(0, ref["frames"][k])
            h.upload_frame(1, ref["frames"][k + 3])
            h.submit_streams([0, 1], [0, 1], [ta, tb], [ta3, tb3])
            for s, want in ((0, ref["joints"][k]), (1, want1[k])):
                rs, j2, j3 = h.collect_stream()
                assert rs == s and _same((j2, j3), want), (s, k)
    finally:
        own.close(), h.close()


@pytest.mark.parametrize("prec", PRECS)
def test_paper_wiring_survives_a_change_of_scales(weights, prec):
    """vnect_set_scales keeps the number of scales (the conv stack's batch size): other scales and back on a live arena handle equal fresh
    handles.  Another NUMBER of scales goes through the facade's `scales` attribute, which opens a new handle from the estimator's
    configuration -- the switch must be in it: a four-scale paper estimator runs the six res2b / res2c layers as launches of their own
    (529 tiles: no tail fits); set to three scales, to [1.0, 0.7] and to three again, it equals fresh paper handles at those scales."""
    from vnect_amd import VNectEstimator
    ref = _reference(prec, weights)
    frames = ref["frames"]
    other, two = [1.0, 0.75, 0.5], [1.0, 0.7]

    def run(h, n=3):
        return [h.infer(frames[k], *_times(k)) for k in range(n)]

    live = _paper(BASELINE_SCALES, weights, prec)
    fresh = _paper(other, weights, prec)
    try:
        run(live, 2)
        live.set_scales(other)
        live.reset_filters()
        a, b = run(live), run(fresh)
        assert all(_same(a[k], b[k]) for k in range(3)), "set_scales to other scales"
        live.set_scales(BASELINE_SCALES)
        live.reset_filters()
        a = run(live)
        assert all(_same(a[k], ref["joints"][k]) for k in range(3)), "set_scales back"
        assert np.array_equal(live.forward(ref["batches"][3]), ref["maps"][3])
    finally:
        live.close(), fresh.close()

    est = VNectEstimator(scales=FOUR, weights=weights, precision=prec, paper_res2c=True, verbose=False)
    fresh = _paper(two, weights, prec)
    try:
        names = [L["name"] for L in est.handle.layers()]
        for x in ("res2b_branch2a", "res2b_branch2b", "res2b_branch2c", "res2c_branch2a", "res2c_branch2b", "res2c_branch2c"):
            assert x in names, (x, names)
        assert not any(x.startswith("res2") and ">" in x for x in names) and not any("res2b_branch2b+res2c_branch2b" in x for x in names), names
        est(frames[0], timestamp=_times(0))
        est.scales = BASELINE_SCALES
        assert _plan(est.handle.layers()) == ref["plan"]
        a = [est(frames[k], timestamp=_times(k)) for k in range(3)]
        assert all(_same(a[k], ref["joints"][k]) for k in range(3)), "four scales -> three"
        est.scales = two
        assert _carries_res2c_branch2a([L["name"] for L in est.handle.layers()], prec)
        a, b = [est(frames[k], timestamp=_times(k)) for k in range(3)], run(fresh)
        assert all(_same(a[k], b[k]) for k in range(3)), "three scales -> two"
        est.scales = BASELINE_SCALES
        a = [est(frames[k], timestamp=_times(k)) for k in range(3)]
        assert all(_same(a[k], ref["joints"][k]) for k in range(3)), "two scales -> three"
    finally:
        est.close(), fresh.close()


@pytest.fixture(scope="module")
def oracle_paper(weights):
    import oracle
    return oracle.Oracle(weights, paper_res2c=True)


def test_paper_end_to_end_vs_oracle(weights, oracle_paper):
    """VNectEstimator(paper_res2c=True), fp32, three frames against the oracle with the paper wiring: the every-frame, every-joint gate
    (gpu_common._EndToEnd: final maps within 1e-4 of the oracle's maximum, everything behind them bit for bit)."""
    from vnect_amd import VNectEstimator
    est = VNectEstimator(scales=BASELINE_SCALES, weights=weights, paper_res2c=True, verbose=False)
    e2e = _EndToEnd(BASELINE_SCALES, oracle_paper)
    try:
        for k, f in enumerate(_frames()[:3]):
            t2, t3 = _times(k)
            j2, j3 = est(f, timestamp=(t2, t3))
            e2e.check(f, t2, t3, j2, j3, est.handle.activation("res5c_branch2c"), (k, SHAPES[k]))
    finally:
        est.close()
    print("legal arg-max ties: %d, worst 3-D excess over tolerance: %.3g" % (e2e.ties, e2e.worst3))


def test_paper_bf16_and_fp16_maps_against_the_fp32_paper_handle(weights):
    """The final maps of the bf16 and fp16 paper plans against the fp32 paper plan's, of its maximum, on every frame: bf16 within 3e-2
    (test_bf16_path_gated_against_fp32), fp16 within a quarter of bf16's and within EPS16 (test_fp16_error_is_a_quarter_of_bf16s)."""
    m32, mb, mh = (_reference(p, weights)["maps"] for p in ("fp32", "bf16", "fp16"))
    rows = []
    for k in range(len(m32)):
        top = float(np.abs(m32[k]).max())
        eb, eh = float(np.abs(mb[k] - m32[k]).max()) / top, float(np.abs(mh[k] - m32[k]).max()) / top
        rows.append((k, eb, eh, eh / eb))
        print("frame %d: bf16 %.3g fp16 %.3g of max (ratio %.3f)" % rows[-1])
    FIGURES["maps_vs_fp32"] = rows
    _log("paper_wiring.json", FIGURES)
    assert all(eb <= 3e-2 for _, eb, _, _ in rows), rows
    assert all(eh <= 0.25 * eb for _, eb, eh, _ in rows), rows
    assert all(eh <= EPS16 for _, _, eh, _ in rows), rows


@pytest.mark.parametrize("prec", PRECS)
def test_paper_switch_is_honoured(weights, prec):
    """The same arena handle without the switch: its final maps differ from the paper handle's by more than 0.1 of their maximum."""
    ref = _reference(prec, weights)
    h = _handle(BASELINE_SCALES, weights, precision=_prec(prec), paper_res2c=False)
    try:
        names = [L["name"] for L in h.layers()]
        assert CHAIN not in names and "res2c_branch2a" not in names
        out = h.forward(ref["batches"][0])
    finally:
        h.close()
    diff = float(np.abs(out - ref["maps"][0]).max()) / float(np.abs(ref["maps"][0]).max())
    print("%s: default wiring %.3g of the paper maps' maximum away" % (prec, diff))
    FIGURES.setdefault("default_vs_paper", {})[prec] = diff
    _log("paper_wiring.json", FIGURES)
    assert diff > 0.1, diff
