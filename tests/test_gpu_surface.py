"""GPU (MI355X): the rest of the reference's call surface and the rows SURVEY 8(f) marks "next", through the C ABI.

joint_filter (estimator.py:83-95), weight files (caffe2pkl.py:83-88 / vnect_model.py:219-236), the person-box initialiser
(hog_box.py:25-58), the static gen_input_batch (estimator.py:70-81), timestamp errors (OneEuroFilter.py:19-23,65-66) and the
no-exception-crosses-the-boundary promise of include/vnect_abi.h.
"""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T0 = 1.7e9
BASELINE_SCALES = [1.0, 0.8, 0.6]


def _est(weights, **kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=weights, verbose=False, **kw)


# ------------------------------------------------------------------------------------------ joint_filter (row b / a14)
@pytest.mark.parametrize("promo", ["legacy", "nep50"])
def test_joint_filter_in_place_bit_exact(weights, promo):
    """VNectEstimator.joint_filter(joints, dim) alone: in place, returns its argument, float64 for the 2-D bank and numpy's
    float32 scalar promotion for the 3-D bank -- bit-exact against the oracle's OneEuro filters (themselves bit-exact against
    the imported reference class, tests/test_golden.py) over 40 calls with irregular time steps."""
    import oracle
    est = _est(weights, scales=[1.0], numpy_promotion=promo)
    cfg2 = dict(freq=30, mincutoff=1.7, beta=0.3, dcutoff=0.4)   # estimator.py:34-45
    cfg3 = dict(freq=30, mincutoff=0.8, beta=0.4, dcutoff=0.4)
    ref2 = [[oracle.OneEuro(**cfg2) for _ in range(2)] for _ in range(21)]
    post = oracle.OracleEstimator(scales=[1.0], nep50=(promo == "nep50"))
    rng = np.random.RandomState(7)
    t = T0
    for k in range(40):
        t += 1 / 30 + 0.002 * (k % 4)
        a2 = 184 + 60 * np.sin(0.2 * k + np.arange(42).reshape(21, 2)) + rng.uniform(-3, 3, (21, 2))
        want2 = np.array([[ref2[j][c](a2[j, c], t) for c in range(2)] for j in range(21)])
        got = est.joint_filter(a2, dim=2, timestamp=t)
        assert got is a2 and a2.dtype == np.float64                 # in place, as estimator.py:86-88 assigns
        assert np.array_equal(a2, want2), k
    # 3-D bank: float32 joints, in place; the first call of a OneEuro filter is the identity (OneEuroFilter.py:25-34,69-70).
    # The float32-fed chain itself is checked frame by frame in test_joint_filter_3d_chain_vs_reference_recording.
    j3 = rng.uniform(-500, 500, (21, 3)).astype(np.float32)
    keep = j3.copy()
    out = est.joint_filter(j3, dim=3, timestamp=T0)
    assert out is j3 and j3.dtype == np.float32 and np.array_equal(j3, keep)
    j3b = (keep + np.float32(1.5)).astype(np.float32)
    est.joint_filter(j3b, dim=3, timestamp=T0 + 0.04)
    assert np.all(np.abs(j3b - keep) <= 1.5) and not np.array_equal(j3b, keep + np.float32(1.5))   # smoothed towards the past
    # `dim` is normalised the way the reference's if / else reads it (estimator.py:85-93): anything but 2 is the 3-D bank, and a
    # (21, 2) array then fails where the reference's joints[i, 2] does -- with IndexError, before any state changes
    with pytest.raises(IndexError):
        est.joint_filter(np.zeros((21, 2)), dim=1, timestamp=T0 + 1)
    with pytest.raises(IndexError):
        est.joint_filter(np.zeros((21, 2)), dim=3, timestamp=T0 + 1)
    j3c = (keep + np.float32(3)).astype(np.float32)
    assert est.joint_filter(j3c, dim=5, timestamp=T0 + 0.08) is j3c      # the 3-D bank again
    assert not np.array_equal(j3c, keep + np.float32(3))
    est.close()


@pytest.mark.parametrize("promo", [0, 1])
def test_joint_filter_3d_chain_vs_reference_recording(weights, promo):
    """The 3-D bank through joint_filter over a float32 sequence, against the float32-fed OneEuro chain the oracle runs
    inside vo_est_postprocess (bit-exact against the imported reference, tests/golden/glue_*.npz): planted maps whose
    read-off is known make the oracle's raw 3-D joints available, so both sides filter the same float32 inputs."""
    from vnect_amd import _native
    from tests import helpers
    import oracle
    h = _native.Handle([1.0], numpy_promotion=promo)
    h.set_weights(weights)
    h.finalize()
    ref = oracle.OracleEstimator(scales=[1.0], nep50=bool(promo))
    t = T0
    for k in range(25):
        t += 1 / 30 + 0.004 * ((k * 3) % 4)
        maps = helpers.synth_maps(1200 + k, 1)
        # oracle: full post-processing (2-D filter, read-off at the filtered joints, 3-D filter)
        o2, o3 = ref.postprocess(maps, t, t + 0.0005)
        # GPU, piecewise through the public surface: raw joints from a throw-away handle state, then the two banks by hand
        avg = oracle.merge_scales(maps, [1.0])
        raw2 = oracle.extract_2d(avg[0])
        f2 = h.joint_filter(2, raw2, False, t)
        assert np.array_equal(f2, o2), k                               # un-mapping is the identity here (scaler 1, offsets 0)
        raw3 = oracle.extract_3d(f2, avg[1], avg[2], avg[3])           # float32, root-relative (utils.py:178-219)
        f3 = h.joint_filter(3, raw3, True, t + 0.0005).astype(np.float32)
        assert np.array_equal(f3, o3), k
    h.close()


def test_timestamp_errors_mirror_reference(weights):
    """t == previous -> ZeroDivisionError (OneEuroFilter.py:66); t < previous -> ValueError (negative freq drives alpha out of
    (0, 1], OneEuroFilter.py:19-23).  Either way the call is rejected BEFORE any state changes: the next valid frame equals
    what an estimator that never saw the bad call returns."""
    from tests import helpers
    a, b = _est(weights, scales=[1.0]), _est(weights, scales=[1.0])
    f = [helpers.synth_frame(60 + k, smooth=True) for k in range(3)]
    a(f[0], timestamp=10.0), b(f[0], timestamp=10.0)
    with pytest.raises(ZeroDivisionError):
        a(f[1], timestamp=10.0)
    with pytest.raises(ValueError):
        a(f[1], timestamp=9.5)
    with pytest.raises(ValueError):
        a.joint_filter(np.zeros((21, 2)), dim=2, timestamp=9.0)
    with pytest.raises(TypeError):   # in place or not at all: a list cannot be filtered in place (nor indexed [i, 0] by the reference)
        a.joint_filter([[0.0, 0.0]] * 21, dim=2, timestamp=11.0)
    with pytest.raises(ValueError):
        a.postprocess(helpers.synth_maps(1, 1), timestamp=(9.0, 11.0))
    x2, x3 = a(f[1], timestamp=10.04)
    y2, y3 = b(f[1], timestamp=10.04)
    assert np.array_equal(x2, y2) and np.array_equal(x3, y3)
    # timestamp 0.0 is "no timestamp" (truthiness test, OneEuroFilter.py:65): accepted after any time
    a(f[2], timestamp=0.0)
    a.close(), b.close()


# ------------------------------------------------------------------------------------------ weight files (row f2)
def test_weight_files_pickle_and_npz(weights, oracle_net, tmp_path):
    """VNectEstimator(weights=path) with the reference's params.pkl layout (caffe2pkl.py:83-88: one pickled dict) and with
    an .npz of the same keys: maps bit-identical to the dict-fed handle and within the fp32 tolerance of the oracle; files
    with a missing or mis-shaped array are refused like the reference's load_weights (vnect_model.py:219-236 KeyErrors)."""
    import oracle
    from tests import helpers
    pkl, npz = tmp_path / "params.pkl", tmp_path / "params.npz"
    with open(pkl, "wb") as f:
        pickle.dump({k: np.asarray(v) for k, v in weights.items()}, f)
    np.savez(npz, **weights)
    batch, _, _ = oracle.gen_input_batch(helpers.synth_frame(808, smooth=True), [1.0])
    ref = oracle_net.forward(batch)
    base = _est(weights, scales=[1.0])
    want = base.forward(batch)
    assert np.abs(want - ref).max() <= 1e-4 * np.abs(ref).max()
    for path in (pkl, npz):
        est = _est(str(path), scales=[1.0])
        assert np.array_equal(est.forward(batch), want), path.name
        j2, j3 = est(helpers.synth_frame(809, 300, 400, smooth=True), timestamp=5.0)
        b2, b3 = base(helpers.synth_frame(809, 300, 400, smooth=True), timestamp=5.0)
        base.reset()
        assert np.array_equal(j2, b2) and np.array_equal(j3, b3)
        est.close()
    base.close()
    bad = dict(weights)
    del bad["res4c_branch2b/weights"]
    np.savez(tmp_path / "missing.npz", **bad)
    with pytest.raises(ValueError, match="res4c_branch2b/weights"):
        _est(str(tmp_path / "missing.npz"), scales=[1.0])
    bad = dict(weights)
    bad["res5c_branch1a/kernel"] = np.zeros((4, 4, 256, 63), np.float32)   # Cin/Cout swapped
    with open(tmp_path / "shape.pkl", "wb") as f:
        pickle.dump(bad, f)
    with pytest.raises(ValueError, match="res5c_branch1a/kernel"):
        _est(str(tmp_path / "shape.pkl"), scales=[1.0])
    # the C ABI itself refuses an incomplete set too (a host that bypasses weights.py)
    from vnect_amd import _native
    h = _native.Handle([1.0])
    h.set_weights({k: v for k, v in weights.items() if k != "conv1/biases"})
    with pytest.raises(_native.VnectError, match="conv1/biases"):
        h.finalize()
    h.close()


# ------------------------------------------------------------------------------------------ person box (row f3)
def test_init_box_on_the_gpu_vs_oracle(weights, oracle_net):
    """runner.init_box with a real estimator: the probe over the whole frame (the reference's no-detection rectangle,
    hog_box.py:28-29) must give the box the oracle-driven equivalent gives, and must not leave filter state behind: the first
    tracked frame is bit-identical to a fresh estimator's."""
    import oracle
    from vnect_amd import runner
    scales = BASELINE_SCALES
    est, fresh = _est(weights, scales=scales), _est(weights, scales=scales)
    frame = next(runner.synthetic_stream(5, 1, 420, 560))

    class OracleEst:  # the oracle behind the estimator call surface init_box uses
        def __init__(self):
            self.o = oracle.OracleEstimator(scales=scales, net=oracle_net)

        def __call__(self, img, timestamp=None):
            return self.o(np.ascontiguousarray(img), timestamp, timestamp)

        def reset(self):
            self.o.reset()

    box = runner.init_box(est, frame, timestamp=3.0)
    ref_est = OracleEst()
    ref_box = runner.init_box(ref_est, frame, timestamp=3.0)
    # the box is arithmetic on the arg-max joints: equal unless a heat-map tie moved an extreme joint (then the GPU's
    # joints must still satisfy the tie rule; checked by recomputing the box from them)
    j2, _ = fresh(frame, timestamp=3.0)
    fresh.reset()
    assert box == runner.bbox_update(j2, 560, 420)
    r2, _ = ref_est(frame, timestamp=3.0)
    ref_est.reset()
    if np.array_equal(j2, r2):
        assert box == ref_box
    else:
        batch, _, _ = oracle.gen_input_batch(frame, scales)
        avg = oracle.merge_scales(oracle_net.forward(batch), scales)[0]
        sc = 368.0 / 560
        for j in np.nonzero(np.any(j2 != r2, axis=1))[0]:
            up = oracle.resize(np.ascontiguousarray(avg[:, :, j]), 8.0)
            y, x = int(round(j2[j, 0] * sc + (184 - int(round(420 * sc)) // 2))), int(round(j2[j, 1] * sc))
            assert up[min(max(y, 0), 367), min(max(x, 0), 367)] >= up.max() - 1e-4 * np.abs(avg).max(), j
    assert 0 <= box[0] and 0 <= box[1] and box[0] + box[2] <= 560 and box[1] + box[3] <= 420 and box[2] >= 1 and box[3] >= 1
    # filter-reset property: the frame after the probe is an unfiltered first frame
    x, y, w, h = box
    crop = frame[y:y + h, x:x + w]
    a2, a3 = est(crop, timestamp=4.0)
    b2, b3 = fresh(crop, timestamp=4.0)
    assert np.array_equal(a2, b2) and np.array_equal(a3, b3)
    est.close(), fresh.close()


# ------------------------------------------------------------------------------------------ joints -> angles, rendering (f4)
def test_angles_and_rendering_from_gpu_joints(weights, oracle_net, tmp_path):
    """SURVEY 8(f) rank 4 on the GPU: 24 frames of a synthetic video through VNectEstimator -> Joints2Angles (filtered, scripted
    clock; src/joints2angles.py:23-109) against the oracle chain -> Joints2Angles, and draw_limbs_2d / draw_limbs_3d
    (src/utils.py:222-244) of the GPU's joints written to files on the GPU box.

    The consumer is a pure function of joints_3d plus its own eight OneEuro filters, so the gate is the estimator's: (1) the oracle's
    post-processing of the GPU's OWN maps reproduces the GPU joints bit for bit, hence the eight angles bit for bit, every frame,
    through both filter chains; (2) against the full oracle chain (oracle maps) the angles agree to 1e-3 rad on every frame up to the
    first heat-map tie among the joints the formulas read (shoulders, elbows, wrists: 2..7; the root row every joint has subtracted
    cancels in their differences) -- beyond a tie the filter states legitimately differ."""
    import oracle
    from vnect_amd import VNectEstimator, render
    from vnect_amd.angles import Joints2Angles
    from tests import helpers
    scales = BASELINE_SCALES
    est = _est(weights, scales=scales)
    post = oracle.OracleEstimator(scales=scales)                      # GPU maps -> oracle joints (lockstep filters)
    full = oracle.OracleEstimator(scales=scales, net=oracle_net)      # the oracle's whole __call__
    ang_gpu, ang_post, ang_full = Joints2Angles(filter=True), Joints2Angles(filter=True), Joints2Angles(filter=True)
    arm = [2, 3, 4, 5, 6, 7]        # every vector of the formulas is a difference of two of these: the root row cancels
    clean, compared, worst = True, 0, 0.0
    H, W = 368, 368   # square: a letter-boxed frame's heat-maps have exactly flat regions (the zero padding), where last-bit noise picks the arg-max
    for k in range(24):
        frame = helpers.synth_frame(6100 + k // 3, H, W, smooth=True)   # a new picture every third frame: the filters see motion and rest
        t = T0 + 700 + k / 30 + 0.001 * (k % 5)                         # irregular clock
        j2, j3 = est(frame, timestamp=(t, t + 0.0007))
        maps = est.handle.activation("res5c_branch2c")
        batch, scaler, (ox, oy) = oracle.gen_input_batch(frame, scales)
        p2, p3 = post.postprocess(maps, t, t + 0.0007, scaler, ox, oy)
        assert np.array_equal(j2, p2) and np.array_equal(j3, p3), k
        a_gpu, a_post = ang_gpu(j3, timestamp=t + 0.002), ang_post(p3, timestamp=t + 0.002)
        assert np.array_equal(np.array(a_gpu), np.array(a_post)), k                                    # (1)
        assert len(a_gpu) == 8 and np.all(np.isfinite(a_gpu)), k
        ref_maps = oracle_net.forward(batch)
        r2, r3 = full.postprocess(ref_maps, t, t + 0.0007, scaler, ox, oy)
        a_full = ang_full(r3, timestamp=t + 0.002)
        raw_g = oracle.extract_2d(oracle.merge_scales(maps, scales)[0])
        raw_r = oracle.extract_2d(oracle.merge_scales(ref_maps, scales)[0])
        clean = clean and bool(np.array_equal(raw_g[arm], raw_r[arm]))
        if clean:                                                                                     # (2)
            d = float(np.abs(np.array(a_gpu) - np.array(a_full)).max())
            worst, compared = max(worst, d), compared + 1
            assert d <= 1e-3, (k, d)
    assert compared >= 1
    print("angles: %d/24 frames compared with the full oracle chain (before the first tie on an arm joint), worst |d| %.3g rad" % (compared, worst))
    # rendering of the GPU's joints to files on this box
    img = render.draw_limbs_2d(frame, j2, VNectEstimator.joint_parents, [0, 0, W - 1, H - 1])
    assert img.shape == frame.shape and img.dtype == np.uint8 and np.any(img != frame)
    r, c = (j2[2] + j2[1]) / 2                                         # middle of limb 2 -> 1
    if 3 <= r < H - 3 and 3 <= c < W - 3:
        assert tuple(img[int(round(r)), int(round(c))]) in (render.LIMB_BGR, render.RECT_BGR)
    v3 = render.draw_limbs_3d(j3, VNectEstimator.joint_parents)
    assert v3.shape == (400, 400, 3) and np.any(v3 != 255)
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out_dir, exist_ok=True)
    for name, pic in (("f4_limbs_2d.png", img), ("f4_limbs_3d.png", v3)):
        for d in (str(tmp_path), out_dir):
            render.save(os.path.join(d, name), pic)
        from PIL import Image
        back = np.asarray(Image.open(os.path.join(str(tmp_path), name)))[:, :, ::-1]
        assert np.array_equal(back, pic), name
    est.close()


# ------------------------------------------------------------------------------------------ static gen_input_batch (a10)
def test_static_gen_input_batch_needs_no_weights(weights):
    """VNectEstimator.gen_input_batch is a @staticmethod in the reference (estimator.py:70-81): it runs on a pre-processing-only
    handle (no weights, no launch plan) and is bit-exact against the oracle; such a handle refuses everything else."""
    import oracle
    from tests import helpers
    from vnect_amd import VNectEstimator, _native
    frame = helpers.synth_frame(31, 300, 500, smooth=True)
    for scales in ([1, 0.85, 0.7], [1.0, 0.6]):
        b, s, off = VNectEstimator.gen_input_batch(frame, 368, scales)
        rb, rs, roff = oracle.gen_input_batch(frame, scales)
        assert np.array_equal(b, rb) and s == rs and off == roff
    flipped = frame[::-1, ::-1]   # negative strides: the reference takes any ndarray
    b, _, _ = VNectEstimator.gen_input_batch(flipped, 368, [1.0])
    rb, _, _ = oracle.gen_input_batch(np.ascontiguousarray(flipped), [1.0])
    assert np.array_equal(b, rb)
    h = _native.Handle([1.0], preprocess_only=True)
    with pytest.raises(_native.VnectError):
        h.finalize()
    with pytest.raises(_native.VnectError):
        h.infer(frame, 1.0, 1.0)
    with pytest.raises(_native.VnectError):
        h.forward(np.zeros((1, 368, 368, 3), np.float32))
    h.close()


# ------------------------------------------------------------------------------------------ boundary robustness
def test_no_exception_crosses_the_abi(weights):
    """include/vnect_abi.h promises codes, never C++ exceptions.  A weight whose shape multiplies out to more elements than
    any allocation can hold makes std::vector throw inside vnect_set_weight: the call must return VNECT_E_INTERNAL (or
    VNECT_E_ARG), leave a message, and leave the handle usable."""
    from vnect_amd import _native
    L = _native.lib()
    h = _native.Handle([1.0])
    shp = (C.c_int64 * 2)(1 << 40, 1 << 20)      # 2^60 floats
    one = np.zeros(4, np.float32)
    rc = L.vnect_set_weight(h._h, b"conv1/biases", one.ctypes.data_as(C.POINTER(C.c_float)), shp, 2)
    assert rc in (_native.E_INTERNAL, _native.E_ARG)
    assert L.vnect_last_error(h._h)
    h.set_weights(weights)   # still usable
    h.finalize()
    out = h.forward(np.zeros((1, 368, 368, 3), np.float32))
    assert np.all(np.isfinite(out))
    h.close()


# ------------------------------------------------------------------------------------------ several streams on one handle
@pytest.mark.parametrize("two_launches,how", [(False, "sync"), (True, "sync"), (False, "lanes3"), (True, "lanes3"), (False, "batch2")],
                         ids=["False", "True", "lanes3", "lanes3-two_launches", "batch2"])
def test_reassigned_scales_equal_a_fresh_estimator(weights, monkeypatch, two_launches, how):
    """`estimator.scales = [...]` (a plain attribute in the reference, estimator.py:32) re-plans pyramid and merge on a live
    handle: the frames after it are bit-identical to a new estimator made with those scales.  The merge geometry is a by-value
    kernel argument, so the two-launch form of the post-processing (VNECT_NO_POST_MERGE=1), whose arg-max launch sits inside the
    captured graph, has to capture again -- both forms are run.
    lanes3 / batch2: the same on a handle with more than one plan -- three lanes with three frames in flight (in both forms of the
    post-processing: every lane captures again), and the two-stream batch through submit_streams -- on frames whose long side is
    368, which take the stem's from-the-frame form where every plan's rectangles fit its LDS scratch.  They fit at the old scales
    and do not at the new ones (tests/test_hostplan.py: fits([1.0, 0.15]) == 0), so a plan whose stem_frame_ok the reassignment
    left behind would go on reading rectangles that do not fit.  The fresh handle is a plain one, run frame by frame."""
    from tests import helpers
    if two_launches:
        monkeypatch.setenv("VNECT_NO_POST_MERGE", "1")
    if how != "sync":
        return _reassigned_scales_on_plans(weights, how)
    frames = [np.ascontiguousarray(helpers.synth_frame(300 + k, 300, 420, smooth=True)) for k in range(4)]
    live = _est(weights, scales=[1.0, 0.85, 0.7])
    for k in range(2):
        live(frames[k], timestamp=T0 + k / 30)
    live.scales = BASELINE_SCALES
    live.handle.reset_filters()
    fresh = _est(weights, scales=BASELINE_SCALES)
    for k, f in enumerate(frames):
        a2, a3 = live(f, timestamp=T0 + 10 + k / 30)
        b2, b3 = fresh(f, timestamp=T0 + 10 + k / 30)
        assert np.array_equal(a2, b2) and np.array_equal(a3, b3), k
    live.close(), fresh.close()


def _reassigned_scales_on_plans(weights, how):
    from vnect_amd import _native
    from tests import helpers
    old, new = [1.0, 0.7], [1.0, 0.15]
    shapes = [(368, 200), (240, 368)] if how == "batch2" else [(368, 200)]
    frames = [np.ascontiguousarray(helpers.synth_frame(340 + k, *shapes[k % len(shapes)], smooth=True)) for k in range(4)]

    def make(scales, **kw):
        h = _native.Handle(scales, num_frame_slots=4, **kw)
        h.set_weights(weights)
        h.finalize()
        for k, f in enumerate(frames):
            h.upload_frame(k, f)
        return h

    def run(h, t0, batched, depth):
        """-> [(stream, j2, j3)] of the four frames: as two batches of streams (0, 1), or stream 0's, `depth` in flight"""
        got = []
        if how == "batch2":
            for k in range(2):
                t = [t0 + k / 30, t0 + 5 + k / 30]
                if batched:
                    h.submit_streams([0, 1], [2 * k, 2 * k + 1], t, t)
                else:
                    for s in (0, 1):
                        h.submit_stream(s, 2 * k + s, t[s], t[s])
                got += [h.collect_stream() for _ in range(2)]
            return got
        for k0 in range(0, 4, depth):
            ks = range(k0, min(k0 + depth, 4))
            for k in ks:
                h.submit_resident(k, t0 + k / 30, t0 + k / 30)
            got += [h.collect_stream() for _ in ks]
        return got

    live = make(old, **({"stream_batch": 2} if how == "batch2" else {"lanes": 3}))
    run(live, T0, True, 3)
    live.set_scales(new)
    live.reset_filters()
    a = run(live, T0 + 10, True, 3)
    fresh = make(new)
    b = run(fresh, T0 + 10, False, 1)
    for k in range(4):
        assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][2], b[k][2]), k
    live.close(), fresh.close()


def test_streams_on_one_handle_equal_handles_of_their_own(weights):
    """vnect_submit_stream: three independent videos (different frames, crop sizes, timestamps, irregular interleaving) served by
    ONE handle with three lanes -- one weight copy, a filter bank per stream -- must return, for every frame of every stream,
    exactly what a handle of its own returns for that video frame by frame (the reference's model: one VNectEstimator per video,
    run_estimator_ps.py:120-129).  Frames of different streams are in flight together; only frames of one stream chain."""
    from vnect_amd import _native
    from tests import helpers
    scales = [1.0, 0.8, 0.6]

    def make(**kw):
        h = _native.Handle(scales, num_frame_slots=8, **kw)
        h.set_weights(weights)
        h.finalize()
        return h
    shapes = [(368, 368), (240, 320), (368, 200)]
    nfr = 5
    vids = [[helpers.synth_frame(7000 + 100 * s + k, *shapes[s], smooth=True) for k in range(nfr)] for s in range(3)]
    times = [[T0 + 10 * s + 0.04 * k + 0.003 * ((k * (s + 2)) % 3) for k in range(nfr)] for s in range(3)]
    want = []
    for s in range(3):                      # the reference's way: an estimator per video, one frame at a time
        h = make()
        want.append([h.infer(vids[s][k], times[s][k], times[s][k] + 0.001) for k in range(nfr)])
        h.close()
    shared = make(lanes=3)
    order = [0, 1, 2, 2, 0, 1, 1, 1, 0, 2, 0, 2, 1, 0, 2]   # 5 frames of each stream, irregularly interleaved
    nxt, inflight, got = [0, 0, 0], [], [[], [], []]
    for i, s in enumerate(order):
        if len(inflight) == 3:
            rs, j2, j3 = shared.collect_stream()
            assert rs == inflight.pop(0)
            got[rs].append((j2, j3))
        k = nxt[s]
        nxt[s] += 1
        slot = i % 8
        shared.upload_frame(slot, vids[s][k])
        shared.submit_stream(s, slot, times[s][k], times[s][k] + 0.001)
        inflight.append(s)
    while inflight:
        rs, j2, j3 = shared.collect_stream()
        assert rs == inflight.pop(0)
        got[rs].append((j2, j3))
    for s in range(3):
        assert len(got[s]) == nfr
        for k in range(nfr):
            assert np.array_equal(got[s][k][0], want[s][k][0]) and np.array_equal(got[s][k][1], want[s][k][1]), (s, k)
    # a stream's filters restart on their own; a bad stream index and a repeated timestamp are refused before any state changes
    shared.reset_filters_stream(1)
    shared.upload_frame(0, vids[1][0])
    shared.submit_stream(1, 0, times[1][0], times[1][0] + 0.001)     # t earlier than stream 1's last frame: fine after the reset
    rs, j2, j3 = shared.collect_stream()
    assert rs == 1 and np.array_equal(j2, want[1][0][0]) and np.array_equal(j3, want[1][0][1])
    with pytest.raises(_native.VnectError):
        shared.submit_stream(4, 0, 1.0, 1.0)
    with pytest.raises(_native.VnectError) as e:
        shared.submit_stream(0, 0, times[0][-1], times[0][-1] + 0.001)
    assert e.value.code == _native.E_TIMESTAMP
    shared.close()


def test_warm_start_leaves_a_fresh_handle(weights):
    """vnect_finalize primes the launch plan on a grey frame (warm start).  Afterwards the handle must be indistinguishable from an
    unprimed one (VNECT_PRIME_FRAMES=0): frames uploaded BEFORE finalize are intact, the first real frame is the filters' identity
    frame, and a sequence gives the same joints bit for bit."""
    import os
    from vnect_amd import _native
    from tests import helpers
    frames = [helpers.synth_frame(9100 + k, 300, 368, smooth=True) for k in range(3)]

    def run(prime):
        old = os.environ.pop("VNECT_PRIME_FRAMES", None)
        if not prime:
            os.environ["VNECT_PRIME_FRAMES"] = "0"
        try:
            h = _native.Handle([1.0, 0.8], num_frame_slots=2, lanes=2)
            h.upload_frame(0, frames[0])            # before finalize: must survive the priming
            h.set_weights(weights)
            h.finalize()
        finally:
            os.environ.pop("VNECT_PRIME_FRAMES", None)
            if old is not None:
                os.environ["VNECT_PRIME_FRAMES"] = old
        out = [h.infer_resident(0, T0, T0 + 0.001)]
        for k in (1, 2):
            out.append(h.infer(frames[k], T0 + k / 30, T0 + k / 30 + 0.001))
        h.close()
        return out
    a, b = run(True), run(False)
    for (a2, a3), (b2, b3) in zip(a, b):
        assert np.array_equal(a2, b2) and np.array_equal(a3, b3)


WARM_START_INJECT = r"""
import os, sys, json
import numpy as np
sys.path.insert(0, %r)
from vnect_amd import _native
from vnect_amd.weights import synthetic_weights
from tests import helpers
assert "test_hooks=1" in _native.build_info()["text"], _native.build_info()["text"]
weights, T0, out = synthetic_weights(), 1.7e9, {}
frame = helpers.synth_frame(9200, smooth=True)
os.environ["VNECT_PRIME_INJECT"] = "hip"
h = _native.Handle([1.0], num_frame_slots=2)
h.set_weights(weights)
try:
    h.finalize()
    out["hip"] = "no error"
except _native.VnectError as e:
    out["hip"] = [e.code, str(e)]
h.close()
os.environ["VNECT_PRIME_INJECT"] = "state"
h = _native.Handle([1.0], num_frame_slots=2)
h.set_weights(weights)
h.finalize()                                   # succeeds; the note says what was skipped and why
out["state_note"] = _native.lib().vnect_last_error(h._h).decode()
a = [h.infer(frame, T0 + k / 30, T0 + k / 30 + 0.001) for k in range(2)]
h.close()
del os.environ["VNECT_PRIME_INJECT"]
os.environ["VNECT_PRIME_FRAMES"] = "0"
os.environ["VNECT_PRIME_MS"] = "0"
h = _native.Handle([1.0], num_frame_slots=2)
h.set_weights(weights)
h.finalize()
b = [h.infer(frame, T0 + k / 30, T0 + k / 30 + 0.001) for k in range(2)]
h.close()
out["equal"] = all(np.array_equal(a2, b2) and np.array_equal(a3, b3) for (a2, a3), (b2, b3) in zip(a, b))
print(json.dumps(out))
"""


def test_warm_start_failure_injection(weights, monkeypatch):
    """What a failure INSIDE the warm start means for vnect_finalize (advisor, round 4): a launch / device error on the plan the handle
    will run for every frame (VNECT_PRIME_INJECT=hip) fails vnect_finalize with VNECT_E_HIP and its reason; a benign refusal of the
    grey frame (=state) is skipped with a note in vnect_last_error, the handle is finalized and returns exactly what an unprimed
    handle returns.  Either way nothing is left in flight and the filter banks are fresh.
    Round 6 (advisor): the injection hook is compiled only into the TEST build of the host runtime (`make testhooks` ->
    libvnect_hip_testhooks.so: the product's kernel objects, rt_*.cpp with -DVNECT_TEST_HOOKS=1), loaded here in a child process through
    VNECT_LIB; the shipped library has no such hook and ignores the variable."""
    import json
    import subprocess
    import sys
    from vnect_amd import _native
    from tests import helpers
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(_native.TESTHOOKS_LIB), "run __graft_entry__.build() (make -C vnect_amd/csrc testhooks)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("VNECT_PRIME")}
    env["VNECT_LIB"] = _native.TESTHOOKS_LIB
    r = subprocess.run([sys.executable, "-c", WARM_START_INJECT % root], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    code, msg = out["hip"]
    assert code == _native.E_HIP and "warm start failed" in msg and "injected warm-start failure (hip)" in msg
    assert "warm start skipped" in out["state_note"] and "injected warm-start failure (state)" in out["state_note"]
    assert out["equal"] is True
    # the product library: no hook -- with the variable set, vnect_finalize succeeds and leaves no note
    assert _native.build_info()["test_hooks"] == "0"
    monkeypatch.setenv("VNECT_PRIME_INJECT", "hip")
    h = _native.Handle([1.0], num_frame_slots=2)
    h.set_weights(weights)
    h.finalize()
    assert _native.lib().vnect_last_error(h._h).decode() == ""
    frame = helpers.synth_frame(9200, smooth=True)
    j2, j3 = h.infer(frame, T0, T0 + 0.001)
    assert np.all(np.isfinite(j2)) and np.all(np.isfinite(j3))
    h.close()


def test_pinned_frame_buffer_equals_pageable_frames(weights):
    """vnect_frame_buffer (ABI v5): frames captured into the handle's pinned buffers -- whole, or as the strided crops the tracking loop
    cuts (run_estimator_ps.py:88) -- give bit for bit what the same pixels give from pageable numpy memory (the CPU-staged path), on one
    filter chain each.  Also: a pageable frame LARGER than anything staged so far grows the internal staging buffer without moving the
    caller's buffers."""
    from vnect_amd import VNectEstimator
    from tests import helpers
    big = helpers.synth_frame(9300, 480, 640, smooth=True)
    a = VNectEstimator(scales=[1.0, 0.8], weights=weights, verbose=False)
    b = VNectEstimator(scales=[1.0, 0.8], weights=weights, verbose=False)
    buf = [a.frame_buffer(480, 640, i) for i in range(2)]
    addr = [x.ctypes.data for x in buf]
    assert buf[0].shape == (480, 640, 3) and buf[0].dtype == np.uint8 and addr[0] != addr[1]
    crops = [(0, 0, 640, 480), (100, 40, 368, 368), (3, 7, 301, 255), (272, 112, 368, 368)]
    for k, (x, y, w, h) in enumerate(crops):
        frame = helpers.synth_frame(9301 + k, 480, 640, smooth=True)
        buf[k % 2][...] = frame                                           # "capture"
        t = (T0 + k / 30, T0 + k / 30 + 0.001)
        p2, p3 = a(buf[k % 2][y:y + h, x:x + w, :], timestamp=t)          # a view INTO the pinned buffer: no CPU copy
        q2, q3 = b(frame[y:y + h, x:x + w, :], timestamp=t)               # pageable: staged by the CPU
        assert np.array_equal(p2, q2) and np.array_equal(p3, q3), (k, x, y, w, h)
    t = (T0 + 1, T0 + 1.001)
    p2, p3 = a(np.ascontiguousarray(big), timestamp=t)                      # pageable on the handle that owns capture buffers
    q2, q3 = b(big, timestamp=t)
    assert np.array_equal(p2, q2) and np.array_equal(p3, q3)
    assert [a.frame_buffer(480, 640, i).ctypes.data for i in range(2)] == addr   # the caller's buffers did not move
    with pytest.raises(Exception):
        a.handle.frame_buffer(2, 10, 10)
    a.close(), b.close()


def test_pinned_crops_at_every_byte_alignment_reach_the_device_intact(weights):
    """The copy kernel behind vnect_infer for crops of a pinned capture buffer (post.hip: frame_copy_rows_kernel; advisor, round 5): a
    crop starts at byte 3 * x0 of a frame row and is 3 * w bytes wide (run_estimator_ps.py:88), so three in four are not dword-aligned.
    Every combination of source phase (3 x0 mod 4), row-length phase (3 w mod 4: the packed destination rows then start at every phase
    too), widths from a few pixels to several waves' worth, in both capture buffers -- checked on EVERY BYTE: a handle with per-layer
    read-back returns the network's input batch, which at scale 1.0 is gen_input_batch of the crop (bit-exact against the oracle)."""
    import oracle
    from vnect_amd import _native
    from tests import helpers
    h = _native.Handle([1.0], keep_activations=True, num_frame_slots=2)
    h.set_weights(weights)
    h.finalize()
    buf = [h.frame_buffer(i, 300, 500) for i in range(2)]
    rng = np.random.RandomState(11)
    for i in range(2):
        buf[i][...] = rng.randint(0, 256, size=buf[i].shape, dtype=np.uint8)
    crops = [(x0, 3 + (x0 % 5), w, hh) for x0 in range(8) for (w, hh) in ((368, 21), (367, 22), (366, 23), (365, 24))]
    crops += [(1, 0, 1, 1), (2, 1, 2, 3), (3, 2, 5, 2), (5, 0, 63, 4), (6, 1, 85, 5), (7, 2, 253, 3), (9, 0, 337, 300), (0, 0, 500, 300), (131, 5, 369, 295)]
    seen = set()
    for k, (x, y, w, hh) in enumerate(crops):
        src = buf[k % 2]
        view = src[y:y + hh, x:x + w, :]
        seen.add(((view.ctypes.data & 3), (3 * w) & 3))
        t = T0 + k / 30
        h.infer(view, t, t + 0.001)
        got = h.activation("input")
        ref = oracle.gen_input_batch(np.ascontiguousarray(view), [1.0])[0]
        assert got.shape == ref.shape and np.array_equal(got, ref), (k, x, y, w, hh, int((got != ref).sum()))
    assert len(seen) == 16, sorted(seen)   # all source phases x all row-length phases
    h.close()


def test_timings_carry_the_shader_clock_and_accept_the_v5_struct(weights):
    """ABI v6: vnect_timings ends with shader_cycles / shader_ticks -- workgroup 0 of every conv launch of the profiling twin stamps the
    shader-cycle counter (s_memtime) beside the 100 MHz clock at its start and its end; 100 * cycles / ticks is the clock the chip held while
    the launches ran (bench.py reports it per rank).  A caller compiled against ABI v5 passes the 56-byte struct and gets the v5 fields,
    nothing written behind them."""
    from vnect_amd import _native
    from tests import helpers
    h = _native.Handle(BASELINE_SCALES, num_frame_slots=2)
    h.set_weights(weights)
    h.finalize()
    h.upload_frame(0, helpers.synth_frame(9400))
    for k in range(5):
        h.infer_resident(0, T0 + k / 30, T0 + k / 30 + 0.001)
    h.set_profiling(True)
    h.reset_timings()
    n = 12
    for k in range(n):
        h.infer_resident(0, T0 + 1 + k / 30, T0 + 1 + k / 30 + 0.001)
    t = h.timings()
    h.set_profiling(False)
    assert t["frames"] == n and t["conv_launches"] == 40
    assert 1500 < t["shader_clock_mhz"] < 2500, t          # MI355X: 2.4 GHz peak engine clock
    # workgroup 0 lives from a launch's start to (about) its end: its spans add up to most of the conv launches' own durations
    span_ms = t["shader_ticks"] * 1e-5
    assert 0.5 * t["conv_ms"] < span_ms <= 1.02 * t["conv_ms"], (span_ms, t["conv_ms"])

    class TimingsV5(C.Structure):
        _fields_ = _native.Timings._fields_[:-2] + [("guard", C.c_double * 2)]
    v5 = TimingsV5()
    v5.struct_size = 56
    v5.guard[0], v5.guard[1] = -1.0, -2.0
    L = _native.lib()
    rc = L.vnect_get_timings(h._h, C.cast(C.byref(v5), C.POINTER(_native.Timings)))
    assert rc == 0 and v5.struct_size == 56 and v5.frames == n and abs(v5.conv_slot_ms - t["conv_slot_ms"]) < 1e-9
    assert (v5.guard[0], v5.guard[1]) == (-1.0, -2.0)       # nothing written past the caller's struct
    bad = _native.Timings()
    bad.struct_size = 64
    assert L.vnect_get_timings(h._h, C.byref(bad)) == _native.E_ARG
    h.close()


def test_a_c_program_runs_frames_through_the_abi(weights, tmp_path):
    """The product path with NO Python in the process: tests/c/infer_frame.c (plain C99: vnect_create, 109 x vnect_set_weight,
    vnect_finalize, vnect_infer per frame) linked against libvnect_hip.so, fed the weights and three frames through a flat file, prints
    the joints as hex floats -- bit for bit what the ctypes path returns for the same frames and timestamps, fp32 and bf16."""
    import shutil
    import struct
    import subprocess
    from vnect_amd import _native
    from tests import helpers
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_native.LIB_PATH)
    exe = tmp_path / "infer_frame"
    r = subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "infer_frame.c"),
                        "-o", str(exe), "-L", libdir, "-lvnect_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    frames = [helpers.synth_frame(9500 + k, smooth=True) for k in range(3)]
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(weights)))
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, np.float32)
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<i", a.ndim) + struct.pack("<%dq" % a.ndim, *a.shape) + a.tobytes())
        f.write(struct.pack("<iii", len(frames), 368, 368))
        for fr in frames:
            f.write(np.ascontiguousarray(fr).tobytes())
    for prec_name, prec in (("fp32", _native.FP32), ("bf16", _native.BF16)):
        r = subprocess.run([str(exe), str(blob)] + (["bf16"] if prec_name == "bf16" else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
        lines = [ln.split() for ln in r.stdout.strip().splitlines() if ln.startswith("frame ")]
        assert len(lines) == 3
        h = _native.Handle(BASELINE_SCALES, precision=prec)
        h.set_weights(weights)
        h.finalize()
        for k, ln in enumerate(lines):
            vals = [float.fromhex(x) for x in ln[2:]]
            c2 = np.array(vals[:42]).reshape(21, 2)
            c3 = np.array(vals[42:], np.float32).reshape(21, 3)
            t = 1.7e9 + k / 30.0
            p2, p3 = h.infer(frames[k], t, t + 0.001)
            assert np.array_equal(c2, p2) and np.array_equal(c3, p3), (prec_name, k)
        h.close()


# ------------------------------------------------------------------------------------------ the bench line's contract
def test_bench_line_contract():
    """`python bench.py --full` (N = 1): ONE JSON line on stdout with the contract's keys -- metric / value / unit /
    n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload -- plus the
    `roofline` and `cpu_baseline` objects, the bf16 and split-product legs, and the evidence of what ran (ranks, backend)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "12", "--warmup", "3", "--cpu-seconds", "1.5"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("frames/sec") and d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["steps"] == 12 and d["warmup"] == 3
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"] and 300 < d["value"] < 5000
    assert "configs[1]" in d["config"]["workload"] and d["config"]["h2d_in_timed_region"] is False
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 157.3 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert 0.2 < rf["frac"] < 1.0 and 30 <= rf["launches_per_frame"] <= 45 and "traffic" in rf
    # `frac` again from the committed rocprofv3 summary alone: the file exists, and its numbers reproduce the fraction it states
    rc = rf["recomputed_from"]
    assert os.path.exists(os.path.join(root, rc["file"])) and rc["file"] == "profiles/" + rf["rocprofv3_source"]
    assert abs(rc["achieved_tflops"] - rc["flops_per_frame"] / (rc["conv_ms_per_frame"] * 1e-3) / 1e12) < 0.01
    assert abs(rc["frac_of_fp32_instruction_peak"] - rc["achieved_tflops"] / 157.3) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "frames/s" and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]
    # the parsed key is the FASTER of the two honest CPU implementations; the C port stays beside it
    port, fw = d["cpu_baseline_port"], d["cpu_baseline_framework"]
    assert port["kind"] == "port" and "cannot run" in port["stands_in_for"] and cb["value"] == max(port["value"], fw.get("value", 0))
    # every leg finds ITS committed profile (the split leg's files are profiles/rNN_split_*)
    for leg, pre in ((d, ""), (d["bf16"], "_bf16"), (d["fp32_split"], "_split")):
        r = leg["roofline"]
        assert r["traffic_source"] and re.match(r"r\d\d%s_traffic\.json$" % pre, r["traffic_source"]), (pre, r["traffic_source"])
        assert r["rocprofv3_source"] and re.match(r"r\d\d%s_conv_roofline\.json$" % pre, r["rocprofv3_source"]), (pre, r["rocprofv3_source"])
    assert d["bf16"]["dtype"] == "bf16" and d["bf16"]["value"] > d["value"] and d["bf16"]["roofline"]["bound"] == "hbm"
    # every leg says what the same stream does three frames deep, and the call-surface rates sit beside `value` (never above it by much)
    assert d["bf16"]["pipelined_frames_per_s_per_gpu"] > 0 and d["fp32_split"]["pipelined_frames_per_s_per_gpu"] > 0 and d["pipelined_frames_per_s_per_gpu"] > 0
    assert 0 < d["pcie_inclusive_frames_per_s_per_gpu"] < 1.02 * d["value"] and 0 < d["pcie_inclusive_from_pinned_capture_buffer_frames_per_s_per_gpu"] < 1.02 * d["value"]
    assert d["fp32_split"]["value"] > 0 and d["fp32_split"]["roofline"]["bound"] == "mfma"
    # round 6: the call-surface legs are interleaved (>= 200 frames per variant whatever --steps says), medians; a short run carries its
    # per-frame latencies and the median-based rate; the line says how the library was built and what the (one) rank did
    cs = d["call_surface"]
    assert cs["frames_per_variant"] >= 200 and set(cs["frames_per_s"]) == {"resident", "pageable", "pinned"}
    assert cs["frames_per_s"]["pinned"] <= 1.01 * cs["frames_per_s"]["resident"] and cs["frames_per_s"]["pageable"] <= 1.01 * cs["frames_per_s"]["resident"]
    assert 0 < cs["extra_us_per_frame"]["pinned"] < 60 and 0 < cs["extra_us_per_frame"]["pageable"] < 80, cs
    assert abs(d["pcie_inclusive_frames_per_s_per_gpu"] - cs["frames_per_s"]["pageable"]) < 0.02
    for leg in (d, d["bf16"], d["fp32_split"]):
        lm = leg["latency_ms"]
        assert len(lm["frames_ms"]) == 12 and abs(lm["value_from_median"] - 1e3 / lm["p50"]) < 0.5
    assert "probes_off=1" in d["build"] and "test_hooks=0" in d["build"] and d["n1_same_job"] is None
    pr = d["per_rank"]
    assert len(pr) == 1 and pr[0]["rank"] == 0 and 800 < pr[0]["shader_clock_mhz"] < 2600 and pr[0]["host_binding"]["bound"] is False
    # `value` is K / (the frames' own time + the closing barrier + synchronize the contract puts inside the region)
    assert abs(d["steps"] / (pr[0]["own_elapsed_s"] + pr[0]["closing_barrier_us"] * 1e-6) - d["value"]) <= 2e-3 * d["value"]
    assert d["rccl_ranks"] == 1 and d["ranks"][0]["device"] == 0 and d["launched_by"] == "single process"
