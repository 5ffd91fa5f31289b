"""GPU: re-detection inside the device tracking loop through the C ABI and Python (vnect_track_redetect, vnect_result_redetect,
runner.track_on_device(redetect=)) -- HOG.md, "Re-detection".

The device loop with lost=(c, n, "reset") and redetect=True must yield, frame by frame and bit for bit, what the host loop
runner.track(lost=(c, n, "detect")) yields on the same frames; a stream that is never lost must yield what the loop without the setting
yields; every refusal leaves everything as it was."""
import ctypes as C

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import hog_ref as R
from tests.test_gpu_hog import Pool

pytestmark = pytest.mark.gpu

HP, WP = R.PLANTED_SIZE
ALWAYS, NEVER = (1e9, 21), (-1e9, 1)     # every frame lost / no frame lost, whatever the weights are


@pytest.fixture(scope="module")
def frames():
    pic, _ = R.planted_frame()
    return [pic, np.ascontiguousarray(np.roll(pic, 8, axis=1)), R.background(HP, WP), pic.copy()]


@pytest.fixture(scope="module")
def est():
    from vnect_amd import VNectEstimator
    from vnect_amd.weights import synthetic_weights
    e = VNectEstimator(scales=[1.0], weights=synthetic_weights(), verbose=False, hog_detector=R.planted_detector(), lanes=3)
    yield e
    e.close()


@pytest.fixture()
def pool():
    p = Pool(dr.load_probe())
    yield p
    p.close()


def _device(pool, frames):
    out = []
    for f in frames:
        f = np.ascontiguousarray(f)
        d = dr.FakeCuda(pool.put(f), f.shape, f.strides)
        d.ptr = d.__cuda_array_interface__["data"][0]
        out.append(d)
    return out


def _stamps(base, n=4):
    return [base + k * 0.0625 for k in range(n)]


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), (what, k, "joints")
        assert list(x[2]) == list(y[2]), (what, k, x[2], y[2])
        assert np.array_equal(x[3], y[3]) and x[4] == y[4], (what, k, "confidence / lost")


@pytest.fixture(scope="module")
def host_a(est, frames):
    """Sequence A on the host: every frame lost, the next box is hog_box of the frame"""
    from vnect_amd import runner
    est.reset()
    want = list(runner.track(est, frames, timestamps=_stamps(100.0), confidence=True, lost=ALWAYS + ("detect",)))
    est.reset()
    boxes = [runner.hog_box(est, f) for f in frames]
    assert boxes[0] != [0, 0, WP, HP] and boxes[2] == [0, 0, WP, HP]           # a cal_rect box that is not the whole frame; nobody on the blank frame
    assert [w[2] for w in want[1:]] == boxes[:3]                               # ... and each is the next frame's crop
    assert want[3][2] == [0, 0, WP, HP]                                        # the frame after the blank one is cropped with the whole frame
    return want


@pytest.mark.parametrize("ahead", [0, 1, 2])
def test_sequence_a_equals_the_host_loop_with_detect(est, frames, pool, host_a, ahead):
    from vnect_amd import runner
    est.reset()
    got = list(runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(100.0), ahead=ahead, source="device", confidence=True,
                                      lost=ALWAYS + ("reset",), redetect=True))
    _same(got, host_a, ("ahead", ahead))
    assert [g[5] for g in got] == [1, 1, 2, 1]


def test_sequence_a_under_hold_takes_the_detection_too(est, frames, pool, host_a):
    from vnect_amd import runner
    est.reset()
    got = list(runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(100.0), source="device", confidence=True,
                                      lost=ALWAYS + ("hold",), redetect=True))
    _same(got, host_a, "hold")
    assert [g[5] for g in got] == [1, 1, 2, 1]


def test_sequence_a_with_draw_and_preview(est, frames, pool, host_a):
    """the detector reads the clean frame: the results are unchanged by draw= (the overlay launch comes behind the chain) and by preview="""
    from vnect_amd import runner
    flat = [np.ascontiguousarray(f).reshape(-1) for f in frames]
    est.reset()
    dev = _device(pool, frames)
    got = list(runner.track_on_device(est, dev, timestamps=_stamps(100.0), ahead=1, source="device", confidence=True, lost=ALWAYS + ("reset",),
                                      redetect=True, draw=True))
    _same(got, host_a, "draw")
    assert all(not np.array_equal(pool.get(d.ptr), f) for d, f in zip(dev, flat))          # every frame was annotated ...
    from vnect_amd import _native
    style = _native.overlay_style(parents=est.joint_parents)
    for d, clean, g in zip(dev, _device(pool, frames), got):                               # ... with the overlay of its own joints and rect_used
        est.handle.draw_device(_native.device_frame(clean, "bgr"), g[0], g[2], None, style, _native.STREAM_SYNCED)
        assert np.array_equal(pool.get(d.ptr), pool.get(clean.ptr))
    est.reset()
    plain = _device(pool, frames)
    list(runner.track_on_device(est, plain, timestamps=_stamps(100.0), ahead=1, source="device", lost=ALWAYS + ("reset",), redetect=True))
    assert all(np.array_equal(pool.get(p.ptr), f) for p, f in zip(plain, flat))            # and without draw= none is written
    est.reset()
    got = list(runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(100.0), source="device", confidence=True, lost=ALWAYS + ("reset",),
                                      redetect=True, preview=True))
    _same([g[:5] for g in got], host_a, "preview")
    assert [g[-1] for g in got] == [1, 1, 2, 1] and all(g[5] is not None and g[5].ndim == 3 for g in got)


def test_sequence_a_turned_frames(est, frames, pool, host_a):
    """orientation 3: the frames stored so that np.rot90(stored, 3) is the picture -- the same pictures, the same results"""
    from vnect_amd import runner
    est.reset()
    turned = [np.ascontiguousarray(np.rot90(f, -3)) for f in frames]
    got = list(runner.track_on_device(est, _device(pool, turned), timestamps=_stamps(100.0), source="device", confidence=True, lost=ALWAYS + ("reset",),
                                      redetect=True, orientation=3))
    _same(got, host_a, "orientation 3")


def test_sequence_a_bf16(frames, pool):
    from vnect_amd import VNectEstimator, runner
    from vnect_amd.weights import synthetic_weights
    e = VNectEstimator(scales=[1.0], weights=synthetic_weights(), verbose=False, hog_detector=R.planted_detector(), lanes=3, precision="bf16")
    try:
        want = list(runner.track(e, frames, timestamps=_stamps(100.0), confidence=True, lost=ALWAYS + ("detect",)))
        e.reset()
        got = list(runner.track_on_device(e, _device(pool, frames), timestamps=_stamps(100.0), ahead=2, source="device", confidence=True,
                                          lost=ALWAYS + ("reset",), redetect=True))
        _same(got, want, "bf16")
        assert [g[5] for g in got] == [1, 1, 2, 1] and want[1][2] != [0, 0, WP, HP]
    finally:
        e.close()


def test_sequence_a_nv12_and_a_pitched_four_byte_rgb_layout(est, frames, pool):
    """NV12 in one allocation and in two with odd pitches (the picture is the project's conversion of it: tests/nv12_ref.py), and the BGR
    pictures stored as 4-byte RGB with padded rows: the device loop on each equals the host loop on the pictures"""
    from tests import nv12_ref as nr
    from vnect_amd import pixfmt, runner
    nv = [pixfmt.bgr_to_nv12(f) for f in frames]
    pics = [nr.restate(n) for n in nv]
    est.reset()
    want = list(runner.track(est, pics, timestamps=_stamps(100.0), confidence=True, lost=ALWAYS + ("detect",)))
    assert want[1][2] != [0, 0, WP, HP] and want[3][2] == [0, 0, WP, HP]
    for two in (False, True):
        dev = []
        for img in nv:
            if not two:
                dev.append(dr.FakeCuda(pool.put(img), img.shape, (WP, 1)))
                continue
            ys, uvs = WP + 3, WP + 5
            yb, ub = np.zeros((HP, ys), np.uint8), np.zeros((HP // 2, uvs), np.uint8)
            yb[:, :WP], ub[:, :WP] = img[:HP], img[HP:]
            dev.append((dr.FakeCuda(pool.put(yb.reshape(-1)[:(HP - 1) * ys + WP]), (HP, WP), (ys, 1)),
                        dr.FakeCuda(pool.put(ub.reshape(-1)[:(HP // 2 - 1) * uvs + WP]), (HP // 2, WP), (uvs, 1))))
        est.reset()
        got = list(runner.track_on_device(est, dev, timestamps=_stamps(100.0), ahead=1, source="device", pixel_format="nv12", confidence=True,
                                          lost=ALWAYS + ("reset",), redetect=True))
        _same(got, want, ("nv12", two))
        assert [g[5] for g in got] == [1, 1, 2, 1]
    est.reset()
    want = list(runner.track(est, frames, timestamps=_stamps(100.0), confidence=True, lost=ALWAYS + ("detect",)))
    dev = []
    for f in frames:
        buf = np.zeros((HP, WP * 4 + 12), np.uint8)
        buf[:, :WP * 4].reshape(HP, WP, 4)[:, :, :3] = f[:, :, ::-1]
        dev.append(dr.FakeCuda(pool.put(buf), (HP, WP, 3), (WP * 4 + 12, 4, 1)))
    est.reset()
    got = list(runner.track_on_device(est, dev, timestamps=_stamps(100.0), source="device", pixel_format="rgb", confidence=True,
                                      lost=ALWAYS + ("reset",), redetect=True))
    _same(got, want, "rgb4")


def test_sequence_b_never_lost_is_the_loop_without_the_setting(est, frames, pool):
    from vnect_amd import runner
    est.reset()
    want = list(runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(200.0), source="device", confidence=True, lost=NEVER + ("reset",)))
    est.reset()
    h, stats, got = est.handle, [], []
    for g in runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(200.0), source="device", confidence=True, lost=NEVER + ("reset",),
                                    redetect=True, ahead=0):
        got.append(g)
        stats.append(h.result_redetect())
    _same(got, want, "never lost")
    assert all(g[5] == 0 for g in got) and all(s == (0, [0, 0, 0, 0], 0) for s in stats)


def test_thresholded_rule_hold_and_reset(est, frames, pool):
    """test_gpu_hog.py's thresholded case: thr sits just above frame 0's third-highest confidence, so that frame is lost whatever follows"""
    from vnect_amd import runner
    est.reset()
    plain = list(runner.track(est, frames, timestamps=_stamps(300.0), confidence=True))
    thr = float(np.nextafter(np.sort(plain[0][3])[-3], np.inf))
    est.reset()
    want = list(runner.track(est, frames, timestamps=_stamps(300.0), confidence=True, lost=(thr, 3, "detect")))
    assert want[0][4] == 1
    for action in ("reset", "hold"):
        est.reset()
        got = list(runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(300.0), source="device", confidence=True,
                                          lost=(thr, 3, action), redetect=True))
        # a lost frame's next box is the detection under either action; a frame that is not lost takes the box update under either: one sequence
        _same(got, want, action)
        assert [g[5] != 0 for g in got] == [bool(w[4]) for w in want]


def test_overflow_gives_the_whole_frame_and_the_loop_goes_on(est, frames, pool):
    from vnect_amd import runner
    est.reset()
    h, stats, got = est.handle, [], []
    for g in runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(400.0), source="device", confidence=True, lost=ALWAYS + ("reset",),
                                    redetect=dict(max_hits=1), ahead=0):
        got.append(g)
        stats.append(h.result_redetect())
    assert len(got) == 4 and stats[0][0] == 3 and stats[0][1] == [0, 0, 0, 0] and stats[0][2] > 1
    assert got[1][2] == [0, 0, WP, HP]                      # the next box of an overflowing frame is the whole frame
    assert [s[0] for s in stats] == [3, 3, stats[2][0], 3] and stats[2][0] in (2, 3) and stats[3][2] == stats[0][2]
    assert all(g[2] == [0, 0, WP, HP] for g in got)         # (nobody, or overflow again, on the blank frame: the whole frame either way)


def test_refusals_leave_nothing_written(est, frames, pool):
    from vnect_amd import VNectEstimator, _native, runner
    from vnect_amd.weights import synthetic_weights
    h = est.handle
    dev = _device(pool, frames)
    with pytest.raises(ValueError):                          # source="pinned"
        next(runner.track_on_device(est, frames, lost=ALWAYS + ("reset",), redetect=True))
    with pytest.raises(ValueError):                          # no rule: no frame is ever lost
        next(runner.track_on_device(est, dev, source="device", redetect=True))
    with pytest.raises(ValueError):                          # "detect" stays the host loop's word
        next(runner.track_on_device(est, dev, source="device", lost=ALWAYS + ("detect",), redetect=True))
    with pytest.raises(ValueError):                          # max_hits 4097
        next(runner.track_on_device(est, dev, source="device", lost=ALWAYS + ("reset",), redetect=dict(max_hits=4097)))
    est.reset()                                              # a refused setting leaves no loss rule behind: a plain loop on the stream loses nothing
    plain = list(runner.track_on_device(est, dev, timestamps=_stamps(600.0), source="device", confidence=True))
    assert all(p[4] == 0 for p in plain)
    L = _native.lib()
    sp = _native.hog_spec(max_hits=4097)
    assert L.vnect_track_redetect(h._h, 0, C.byref(sp), 1) == _native.E_ARG
    assert L.vnect_track_redetect(h._h, 99, None, 1) == _native.E_ARG
    bad = _native.hog_spec()
    bad.scale0 = 1.0
    assert L.vnect_track_redetect(h._h, 0, C.byref(bad), 1) == _native.E_ARG
    # the setting changed with a frame in flight; the other submit forms on a re-detecting stream
    est.reset()
    h.track_begin(0, HP, WP, None)
    h.track_policy(0, ALWAYS[0], ALWAYS[1], "reset")
    h.track_redetect(0, None, True)
    h.frame_buffer(0, 1, HP * WP)
    assert L.vnect_submit_tracked_pinned(h._h, 0, 0, 3 * WP, 1.0, 1.0) == _native.E_ARG
    assert L.vnect_submit_tracked(h._h, 0, 0, 1.0, 1.0) == _native.E_ARG
    f = _native.device_frame(dev[0], "bgr")
    h.submit_tracked_device(0, f, 500.0, 500.0, None)
    assert L.vnect_track_redetect(h._h, 0, None, 0) == _native.E_STATE
    assert L.vnect_track_redetect(h._h, 0, None, 1) == _native.E_STATE
    _, _, _, used = h.collect_tracked()
    assert list(used) == [0, 0, WP, HP] and h.result_redetect()[0] == 1
    h.track_redetect(0, None, False)
    h.track_policy(0, 0.0, 1, "off")
    est.reset()
    # no detector: VNECT_E_STATE, and the stream stays as it was
    e2 = VNectEstimator(scales=[1.0], weights=synthetic_weights(), verbose=False)
    try:
        assert L.vnect_track_redetect(e2.handle._h, 0, None, 1) == _native.E_STATE
        assert len(list(runner.track_on_device(e2, _device(pool, frames[:1]), timestamps=[1.0], source="device"))) == 1
    finally:
        e2.close()


def test_a_synchronous_detection_between_tracked_frames_shares_the_handle(est, frames, pool, host_a):
    from vnect_amd import runner
    est.reset()
    want = R.detect(frames[1], R.planted_detector(), R.spec(), keep=False)["rects"]
    got = []
    for g in runner.track_on_device(est, _device(pool, frames), timestamps=_stamps(100.0), ahead=1, source="device", confidence=True,
                                    lost=ALWAYS + ("reset",), redetect=True):
        got.append(g)
        rects, _ = est.detect_people(frames[1])            # on the handle's own workspace, on the upload stream
        assert [tuple(int(v) for v in r) for r in rects] == [tuple(r) for r in want]
    _same(got, host_a, "detect_people in between")
