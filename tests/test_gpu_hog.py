"""GPU: the person detector through the C ABI (vnect_hog_set_detector, vnect_hog_levels, vnect_hog_detect_device, vnect_hog_detect) and
the Python layer above it (est.detect_people, runner.hog_box, runner.track(lost=(.., "detect"))) -- HOG.md.

What the device returns must be exactly the numpy statement's grouped rects and weights (tests/hog_ref.py), from host frames and from
frames in device memory in every layout; the frame is never written; every refusal comes before any launch, with nothing written.  The
device memory comes from the device-frame probe's allocator and is described to the library by a bare __cuda_array_interface__
(tests/devframe_ref.py: FakeCuda), so nothing here needs torch -- except the child process, which is about torch."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import hog_ref as R
from tests import preview_ref as P

pytestmark = pytest.mark.gpu

DET = R.seeded_detector(1, rho=0.05, scale=0.04)


class Pool:
    """device buffers of one test: put() uploads a byte buffer, get() reads it back; freed at the test's end"""

    def __init__(self, probe):
        self.probe, self.ptrs = probe, {}

    def put(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        p = C.c_void_p()
        assert self.probe.ip_alloc(len(buf), C.byref(p)) == 0 and p.value
        assert self.probe.ip_h2d(p.value, buf.ctypes.data, len(buf)) == 0
        self.ptrs[p.value] = len(buf)
        return p.value

    def get(self, p):
        out = np.zeros(self.ptrs[p], np.uint8)
        assert self.probe.ip_d2h(out.ctypes.data, p, len(out)) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.probe.ip_free(p)
        self.ptrs = {}


@pytest.fixture()
def pool():
    p = Pool(dr.load_probe())
    yield p
    p.close()


def _source(pool, lay, buf):
    p = pool.put(buf)
    fmt = ("bgr", "rgb", "nv12")[lay["format"]]
    if lay["format"] == 2:
        arr = (dr.FakeCuda(p + lay["data_off"], (lay["H"], lay["W"]), (lay["sy"], 1)), dr.FakeCuda(p + lay["uv_off"], (lay["H"] // 2, lay["W"]), (lay["uv_stride"], 1)))
    else:
        arr = dr.FakeCuda(p + lay["data_off"], (lay["H"], lay["W"], 3), (lay["sy"], lay["sx"], lay["sc"]))
    return p, arr, fmt


def _rects(ref):
    return [tuple(r) for r in ref["rects"]], np.array(ref["weights"], np.float64)


def _same(got, ref, what):
    rects, ws = got
    want_r, want_w = _rects(ref)
    assert [tuple(int(v) for v in r) for r in rects] == want_r, (what, rects, want_r)
    assert rects.dtype == np.int32 and ws.dtype == np.float64 and np.array_equal(ws, want_w), what


@pytest.fixture(scope="module")
def planted():
    pic, cells = R.planted_frame()
    det = R.planted_detector()
    ref = R.detect(pic, det, R.spec(), keep=False)
    assert len(ref["rects"]) == len(cells)
    return pic, cells, det, ref


def test_abi_on_a_preprocess_only_handle_host_and_device_frames(pool):
    """needs no weights and no plan: levels, host frames (packed and row-strided), device frames in every layout under codes going round,
    final_threshold below 1 (the hits ungrouped), the full count above the capacity, the frame unchanged"""
    from vnect_amd import _native
    h = _native.Handle([1.0], preprocess_only=True)
    try:
        h.hog_set_detector(DET)
        H, W = 200, 100
        pic = R.textured(H, W, seed=H)
        for kw in (dict(), dict(final_threshold=0.5), dict(scale0=1.2, win_stride=(16, 8)), dict(hit_threshold=-0.1, nlevels=3)):
            s = R.spec(**kw)
            ref = R.detect(pic, DET, s, keep=False)
            assert ref["hits"]
            sp = _native.hog_spec(**kw)
            _same(h.hog_detect(pic, sp), ref, ("host", kw))
            wide = np.zeros((H, W + 7, 3), np.uint8)
            wide[:, :W] = pic
            _same(h.hog_detect(wide[:, :W], sp), ref, ("host strided", kw))
            f = _native.DeviceFrame()
            f.struct_size, f.H, f.W = C.sizeof(_native.DeviceFrame), H, W
            hw, sc = h.hog_levels(f, sp)
            assert [tuple(int(v) for v in x) for x in hw] == [(a, b) for a, b, _ in ref["levels"]] and np.array_equal(sc, [x[2] for x in ref["levels"]])
        ungrouped = R.detect(pic, DET, R.spec(final_threshold=0.5), keep=False)
        assert len(ungrouped["rects"]) == len(ungrouped["hits"]) > 3
        rects, ws, cnt = np.full((2, 4), -7, np.int32), np.full(2, -7.0), C.c_int32(-7)
        sp = _native.hog_spec(final_threshold=0.5)
        rc = _native.lib().vnect_hog_detect(h._h, pic.ctypes.data_as(R.u8p), H, W, 3 * W, C.byref(sp), rects.ctypes.data_as(R.i32p), ws.ctypes.data_as(R.f64p), 1, C.byref(cnt))
        assert rc == 0 and cnt.value == len(ungrouped["hits"])           # count_out is the full count, also above the capacity ...
        assert tuple(rects[0]) == ungrouped["rects"][0] and (rects[1] == -7).all() and ws[1] == -7.0      # ... and nothing lies behind it
        for k, lay in enumerate(P.layouts(136, 72)):
            o = (k * 3) % 8
            h.set_orientation(o)
            if lay["format"] == 2:
                buf = P.fresh(lay)
            else:
                buf = R.lay_from_picture(R.textured(136, 72, seed=k), lay, 0)
            p, arr, fmt = _source(pool, lay, buf)
            ref = R.detect(P.picture(buf, lay, o), DET, R.spec(final_threshold=0.5), keep=False)
            _same(h.hog_detect_device(_native.device_frame(arr, fmt), _native.hog_spec(final_threshold=0.5), stream=0), ref, (lay["name"], o))
            assert np.array_equal(pool.get(p), buf), (lay["name"], "the frame was written")
        h.set_orientation(0)
        # smaller than the window: no level, no detection, no error
        small = np.zeros((127, 64, 3), np.uint8)
        rects, ws = h.hog_detect(small)
        assert rects.shape == (0, 4) and ws.shape == (0,)
    finally:
        h.close()


def test_every_refusal_with_nothing_written(pool):
    from vnect_amd import _native
    h = _native.Handle([1.0], preprocess_only=True)
    L = _native.lib()
    try:
        pic = R.textured(136, 72)
        lay = R.packed(136, 72)
        p, arr, fmt = _source(pool, lay, R.lay_from_picture(pic, lay, 0))
        frame = _native.device_frame(arr, fmt)

        def call(spec=None, fr=frame, host=False, capacity=4):
            rects, ws, cnt = np.full((4, 4), -7, np.int32), np.full(4, -7.0), C.c_int32(-7)
            sp = None if spec is None else C.byref(spec)
            if host:
                rc = L.vnect_hog_detect(h._h, pic.ctypes.data_as(R.u8p), 136, 72, 216, sp, rects.ctypes.data_as(R.i32p), ws.ctypes.data_as(R.f64p), capacity, C.byref(cnt))
            else:
                rc = L.vnect_hog_detect_device(h._h, C.byref(fr), None, sp, rects.ctypes.data_as(R.i32p), ws.ctypes.data_as(R.f64p), capacity, C.byref(cnt))
            untouched = (rects == -7).all() and (ws == -7.0).all() and cnt.value == -7
            return rc, untouched

        # no detector set: VNECT_E_STATE
        for host in (False, True):
            assert call(host=host) == (_native.E_STATE, True)
        # the detector itself
        for bad in (np.zeros(3779, np.float32), np.zeros(3782, np.float32), np.zeros(0, np.float32)):
            with pytest.raises(ValueError):
                h.hog_set_detector(bad)
        for v in (np.nan, np.inf, -np.inf):
            bad = DET.copy()
            bad[5] = v
            with pytest.raises(ValueError):
                h.hog_set_detector(bad)
        assert call() == (_native.E_STATE, True)                       # a refused detector sets nothing
        h.hog_set_detector(DET[:3780])                                 # 3780: rho 0
        h.hog_set_detector(DET)
        assert call()[0] == 0

        def spec(**kw):
            s = _native.hog_spec()
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        bads = [spec(win_stride_x=4), spec(win_stride_y=12), spec(win_stride_x=-8), spec(scale0=1.0), spec(scale0=0.5), spec(scale0=float("nan")),
                spec(scale0=float("inf")), spec(hit_threshold=float("nan")), spec(hit_threshold=float("inf")), spec(final_threshold=float("nan")),
                spec(final_threshold=float("-inf")), spec(nlevels=65), spec(nlevels=-1), spec(max_hits=-1), spec(struct_size=40)]
        for s in bads:
            for host in (False, True):
                assert call(s, host=host) == (_native.E_ARG, True), [getattr(s, k) for k, _ in s._fields_]
            n = C.c_int32(-7)
            assert L.vnect_hog_levels(h._h, C.byref(frame), C.byref(s), C.byref(n), None, None, 0) == _native.E_ARG and n.value == -7
        # a frame with a rect; a picture side above 4096 (vnect_hog_levels: arithmetic only, the pointers are not looked at)
        assert call(fr=_native.device_frame(arr, fmt, rect=(0, 0, 64, 128))) == (_native.E_ARG, True)
        big = _native.DeviceFrame()
        big.struct_size, big.H, big.W = C.sizeof(_native.DeviceFrame), 4097, 64
        n = C.c_int32(-7)
        assert L.vnect_hog_levels(h._h, C.byref(big), None, C.byref(n), None, None, 0) == _native.E_ARG and n.value == -7
        big.H, big.W = 128, 4098
        assert L.vnect_hog_levels(h._h, C.byref(big), None, C.byref(n), None, None, 0) == _native.E_ARG
        assert call(capacity=-1) == (_native.E_ARG, True)
        # more hits than max_hits: the call fails with a message that says what to do; nothing is returned
        hot = DET.copy()
        hot[3780] = 1000.0
        h.hog_set_detector(hot)
        rc, untouched = call(spec(max_hits=2))
        assert rc == _native.E_STATE and untouched and "raise hit_threshold" in L.vnect_last_error(h._h).decode()
        rc, untouched = call(spec(max_hits=2), host=True)
        assert rc == _native.E_STATE and untouched
        assert np.array_equal(pool.get(p), R.lay_from_picture(pic, lay, 0))
    finally:
        h.close()
    # a pyramid-sharded handle
    hs = _native.Handle([1.0, 0.8], pyramid=(0, 2))
    try:
        with pytest.raises(ValueError):
            hs.hog_set_detector(DET)
    finally:
        hs.close()


@pytest.fixture(scope="module")
def est():
    from vnect_amd import VNectEstimator
    from vnect_amd.weights import synthetic_weights
    e = VNectEstimator(scales=[1.0], weights=synthetic_weights(), verbose=False, hog_detector=R.planted_detector())
    yield e
    e.close()


def test_planted_frame_detect_people_and_hog_box(est, planted, pool):
    """the planted 640 x 360 frame gives the CPU statement's rects -- one per painted figure, each containing it, nothing else -- from the
    host frame and from device memory; runner.hog_box takes the larger through cal_rect; nobody there: the whole frame"""
    from vnect_amd import runner
    pic, cells, det, ref = planted
    _same(est.detect_people(pic), ref, "host")
    for cell in cells:
        x0, y0, x1, y1 = R.painted_extent(cell)
        assert sum(r[0] <= x0 and r[1] <= y0 and r[0] + r[2] > x1 and r[1] + r[3] > y1 for r in ref["rects"]) == 1
    lay = R.packed(*R.PLANTED_SIZE)
    p, arr, fmt = _source(pool, lay, pic)
    _same(est.detect_people(arr, stream=0), ref, "device")
    rects = np.array(ref["rects"])
    biggest = rects[int(np.argmax(rects[:, 2] * rects[:, 3]))]
    assert runner.hog_box(est, pic) == runner.cal_rect(biggest, 360, 640) == runner.hog_box(est, arr, stream=0)
    assert runner.hog_box(est, R.background(360, 640)) == [0, 0, 640, 360]
    turned = np.ascontiguousarray(np.rot90(pic, -3))                     # stored so that np.rot90(stored, 3) is the picture
    assert runner.hog_box(est, turned, orientation=3) == runner.cal_rect(biggest, 360, 640)
    est.set_hog_detector(det)                                           # the explicit setter, and detector= on the call
    _same(est.detect_people(pic, detector=det, final_threshold=2.0), ref, "detector=")
    with pytest.raises(ValueError):
        est.detect_people(pic, nlevels=0)
    with pytest.raises(TypeError):
        est.detect_people(pic, padding=(8, 8))


def test_track_with_lost_detect_equals_the_loop_that_calls_hog_box(est, planted):
    """runner.track(lost=(c, n, "detect")) on a short synthetic stream yields on every frame exactly what the same loop yields when the
    test calls hog_box on the host after each lost frame; the device loops refuse "detect" """
    from vnect_amd import runner
    pic = planted[0]
    frames = [np.ascontiguousarray(np.roll(pic, 8 * k, axis=1)) for k in range(5)]
    est.reset()
    plain = list(runner.track(est, frames, timestamps=[100 + k * 0.0625 for k in range(5)], confidence=True))
    thr = float(np.nextafter(np.sort(plain[0][3])[-3], np.inf))         # just above the first frame's third-highest confidence: that frame is
                                                                        # lost whatever follows (it is the same frame in every run below)
    rule = (thr, 3, "detect")
    est.reset()
    got = list(runner.track(est, frames, timestamps=[200 + k * 0.0625 for k in range(5)], confidence=True, lost=rule))
    est.reset()
    want, rect = [], None
    for k, frame in enumerate(frames):
        H, W = frame.shape[:2]
        x, y, w, h = rect if rect is not None and rect[2] >= 1 and rect[3] >= 1 else [0, 0, W, H]
        j2, j3, conf = est(frame[y:y + h, x:x + w, :], timestamp=300 + k * 0.0625, return_confidence=True)
        j2[:, 0] += y
        j2[:, 1] += x
        rect = runner.bbox_update(j2, W, H)
        gone = runner.is_lost(conf, thr, 3)
        if gone:
            rect = runner.hog_box(est, frame)
        want.append((j2, j3, [x, y, w, h], conf, int(gone)))
    assert len(got) == len(want) == 5 and any(w[4] for w in want)
    for a, b in zip(got, want):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and list(a[2]) == list(b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    lost_at = [k for k, w in enumerate(want) if w[4] and k + 1 < len(want)]
    assert any(want[k + 1][2] == runner.hog_box(est, frames[k]) for k in lost_at)
    for loop in (runner.track_on_device, ):
        with pytest.raises(ValueError):
            next(loop(est, frames, lost=rule))
    with pytest.raises(ValueError):
        next(runner.track_many_on_device(est, [frames], lost=rule))
    est.reset()


def test_a_detection_leaves_the_estimator_as_it_was(planted):
    from vnect_amd import VNectEstimator
    from vnect_amd.weights import synthetic_weights
    pic, _, det, ref = planted
    out = []
    for detect in (False, True):
        e = VNectEstimator(scales=[1.0, 0.8], weights=synthetic_weights(), verbose=False)
        try:
            a = e(pic, timestamp=5.0)
            if detect:
                _same(e.detect_people(pic, detector=det), ref, "between frames")
            b = e(pic[20:300, 40:500], timestamp=5.0625)
            out.append(a + b)
        finally:
            e.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_torch_tensors_in_every_layout():
    """a child process that imports torch first: est.detect_people on packed, permuted, 4-byte, sliced, RGB and NV12 tensors equals the
    numpy statement over their host copies, and no tensor's storage changes"""
    r = subprocess.run([sys.executable, "-m", "tests.hog_torch_child"], cwd=R.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "hog child ok"
