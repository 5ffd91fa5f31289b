"""GPU: the overlay through the C ABI (vnect_draw_device, vnect_submit_tracked_device_draw) and the Python layers above it (OVERLAY.md).

What the device leaves in the caller's frame must be exactly what render.draw_limbs_2d_exact (NV12: tests/overlay_ref.py) draws into the
frame's host copy, and a tracked loop that draws must yield exactly what the same loop yields without drawing.  The device memory comes
from the device-frame probe's allocator (vnect_amd/csrc/ingest_probe.hip) and is described to the library by a bare
__cuda_array_interface__ (tests/devframe_ref.py: FakeCuda), so nothing here needs torch -- except the child process, which is about torch."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import overlay_ref as R

pytestmark = pytest.mark.gpu

T0 = 1.7e9
H, W = 96, 128
_CACHE = {}


def _planted():
    if "w" not in _CACHE:
        from tests import planted as pl
        _CACHE["w"] = pl.weights(noise=1.0)
    return _CACHE["w"]


def _est(**kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=_planted(), verbose=False, **kw)


def _times(n, base=0.0):
    return [(T0 + base + 0.033 * k + 0.002 * (k % 3), T0 + base + 0.033 * k + 0.0005) for k in range(n)]


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


def _target(pool, lay, buf):
    """the layout's frame in a device buffer holding `buf` -> (the buffer's address, the array the library is given, its pixel format)"""
    p = pool.put(buf)
    fmt = ("bgr", "rgb", "nv12")[lay["format"]]
    if lay["format"] == 2:
        arr = (dr.FakeCuda(p + lay["data_off"], (lay["H"], lay["W"]), (lay["sy"], 1)), dr.FakeCuda(p + lay["uv_off"], (lay["H"] // 2, lay["W"]), (lay["uv_stride"], 1)))
    else:
        arr = dr.FakeCuda(p + lay["data_off"], (lay["H"], lay["W"], 3), (lay["sy"], lay["sx"], lay["sc"]))
    return p, arr, fmt


def test_draw_device_in_every_layout_on_a_preprocess_only_handle(pool):
    """vnect_draw_device needs no weights and no plan: every layout of tests/overlay_ref.py, the skeleton with a threshold and the
    band-over-limb case, equal to the rule in the target's whole buffer (padding, fourth bytes, the bytes around an odd base)."""
    from vnect_amd import _native
    h = _native.Handle([1.0], preprocess_only=True)
    try:
        for lay in R.layouts(37, 53):
            for case in [c for c in R.cases(37, 53) if c["name"] in ("skeleton", "band_over_limb", "half_outside", "nonfinite")]:
                want = R.fresh(lay)
                assert R.draw(want, lay, case) > 0
                p, arr, fmt = _target(pool, lay, R.fresh(lay))
                style = _native.overlay_style(case["thr"], None, case["parents"])
                h.draw_device(_native.device_frame(arr, fmt), case["joints"], case["rect"], case["conf"], style, _native.STREAM_SYNCED)
                assert np.array_equal(pool.get(p), want), (lay["name"], case["name"])
        # the reference's style (NULL) draws the reference's parents in the reference's colours
        lay = R.layouts(37, 53)[0]
        case = [c for c in R.cases(37, 53) if c["name"] == "skeleton"][0]
        want = R.fresh(lay)
        R.draw(want, lay, dict(case, name="skeleton_no_threshold", conf=None, thr=None))
        p, arr, fmt = _target(pool, lay, R.fresh(lay))
        h.draw_device(_native.device_frame(arr, fmt), case["joints"], case["rect"], None, None, _native.STREAM_SYNCED)
        assert np.array_equal(pool.get(p), want)
    finally:
        h.close()


def test_est_draw_equals_the_numpy_renderer(pool):
    from vnect_amd import render
    est = _est()
    try:
        case = [c for c in R.cases(H, W) if c["name"] == "skeleton"][0]
        for lay in [lay for lay in R.layouts(H, W) if lay["format"] != 2]:
            fmt = "rgb" if lay["format"] == 1 else "bgr"
            want = R.fresh(lay)
            render.draw_limbs_2d_exact(R.view(want, lay), case["joints"], est.joint_parents, case["rect"], fmt, case["conf"], 0.4, ((9, 8, 7), None), inplace=True)
            p, arr, _ = _target(pool, lay, R.fresh(lay))
            assert est.draw(arr, case["joints"], rect=case["rect"], confidence=case["conf"], pixel_format=fmt, min_confidence=0.4, colors=((9, 8, 7), None)) is arr
            assert np.array_equal(pool.get(p), want) and (want != R.fresh(lay)).any(), lay["name"]
    finally:
        est.close()


def test_refusals_leave_the_target_untouched(pool):
    from vnect_amd import _native
    L = _native.lib()
    lay = R.layouts(H, W)[0]
    case = [c for c in R.cases(H, W) if c["name"] == "skeleton"][0]
    before = R.fresh(lay)
    p, arr, fmt = _target(pool, lay, before)
    host = before.copy()
    j2 = np.ascontiguousarray(case["joints"], np.float64)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = _native.Handle([1.0], preprocess_only=True)

    def raw(frame, rect=(3, 2, 40, 30), style=None):
        r = np.asarray(rect, np.int32)
        rc = L.vnect_draw_device(h._h, C.byref(frame), C.c_void_p(_native.STREAM_SYNCED), j2.ctypes.data_as(f64p), None, r.ctypes.data_as(i32p),
                                 None if style is None else C.byref(style))
        return rc, L.vnect_last_error(h._h).decode()

    def style(**over):
        s = _native.overlay_style(parents=R.PARENTS)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    try:
        good = lambda: _native.device_frame(arr, fmt)  # noqa: E731
        bad_parent = style()
        bad_parent.parents[5] = 21
        bad_colour = style()
        bad_colour.rect_bgr[1] = 256
        rng = np.zeros(2, np.int64)
        assert pool.probe.ip_range(p, rng.ctypes.data_as(dr.i64p)) == 0 and rng[0] <= p and rng[1] >= len(before)
        room = int(rng[0] + rng[1] - p)                                   # bytes from the frame's first to the allocation's end, as the runtime reports them
        short = dr.FakeCuda(p, (room // lay["sy"] + 2, W, 3), (lay["sy"], 3, 1))   # rows past the allocation's end
        cases = [
            ("a host pointer", _native.device_frame(dr.FakeCuda(host.ctypes.data, (H, W, 3), (lay["sy"], 3, 1))), {}, "vnect_infer / vnect_upload_frame"),
            ("has_rect", _native.device_frame(arr, fmt, (0, 0, 10, 10)), {}, "takes no rect"),
            ("a parent of 21", good(), dict(style=bad_parent), "parent"),
            ("an empty rect", good(), dict(rect=(3, 2, 0, 30)), "at least one pixel"),
            ("a rect of negative height", good(), dict(rect=(3, 2, 5, -1)), "at least one pixel"),
            ("a colour of 256", good(), dict(style=bad_colour), "0 .. 255"),
            ("a wrong style size", good(), dict(style=style(struct_size=8)), "struct_size"),
            ("a last byte outside the allocation", _native.device_frame(short), {}, "past the end of the allocation"),
        ]
        for what, frame, kw, text in cases:
            rc, msg = raw(frame, **kw)
            assert rc == _native.E_ARG and text in msg and msg.startswith("vnect_draw_device: "), (what, rc, msg)
            assert np.array_equal(pool.get(p), before), what
        assert L.vnect_draw_device(h._h, C.byref(good()), C.c_void_p(_native.STREAM_SYNCED), None, None, None, None) == _native.E_ARG
        with pytest.raises(ValueError, match="vnect_draw_device: .*takes no rect"):     # the Python layer: a ValueError, like every refused argument
            h.draw_device(_native.device_frame(arr, fmt, (0, 0, 10, 10)), j2)
        assert np.array_equal(pool.get(p), before)
        # and the handle goes on
        want = before.copy()
        R.draw(want, lay, dict(case, name="skeleton_after_refusals", conf=None, thr=None, rect=(3, 2, 40, 30)))
        assert raw(good())[0] == 0 and np.array_equal(pool.get(p), want)
    finally:
        h.close()


def _frames(fmt, n=4):
    """n frames of a 96 x 128 synthetic stream: (host arrays as the resident loop takes them, layouts of their device copies)"""
    from vnect_amd import pixfmt, runner
    bgr = list(runner.synthetic_stream(0, n, H, W))
    if fmt == "nv12":
        lay = dict(name="nv12_frame", format=2, H=H, W=W, data_off=0, uv_off=H * W, sy=W, sx=1, sc=0, uv_stride=W, size=H * W * 3 // 2)
        return [pixfmt.bgr_to_nv12(f).reshape(-1) for f in bgr], [lay] * n
    names = ["packed3_padded", "planar", "packed4", "packed3_odd_base"]
    lays = [[lay for lay in R.layouts(H, W) if lay["name"] == names[k % 4]][0] for k in range(n)]
    bufs = []
    for f, lay in zip(bgr, lays):
        b = R.fresh(lay, 5)
        R.view(b, lay)[...] = f
        bufs.append(b)
    return bufs, lays


def _device_copies(pool, bufs, lays):
    out = [_target(pool, lay, b) for b, lay in zip(bufs, lays)]
    arrs = [a for _, a, _ in out]
    if lays[0]["format"] == 2:           # the (H * 3 // 2, W) form the runner takes
        arrs = [dr.FakeCuda(p, (H * 3 // 2, W), (W, 1)) for p, _, _ in out]
    return [p for p, _, _ in out], arrs


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_tracked_loop_with_draw(pool, fmt):
    """track_on_device(source="device", draw=True) over 4 frames, submitted ahead on two lanes: what it yields is what draw=False yields on
    copies of the frames, bit for bit, and every frame afterwards is the rule applied to the original frame with that frame's own yielded
    joints and rect_used."""
    from vnect_amd import runner
    bufs, lays = _frames(fmt)
    times, rect = _times(4), [9, 5, 90, 70]
    e = _est(lanes=2)
    try:
        _, plain = _device_copies(pool, bufs, lays)
        want = list(runner.track_on_device(e, plain, rect=rect, timestamps=times, ahead=1, source="device", pixel_format=fmt, confidence=True))
        e.reset()
        ptrs, drawn = _device_copies(pool, bufs, lays)
        got = list(runner.track_on_device(e, drawn, rect=rect, timestamps=times, ahead=1, source="device", pixel_format=fmt, confidence=True, draw=True))
        assert len(got) == len(want) == 4
        for k, (g, w) in enumerate(zip(got, want)):
            assert list(g[2]) == list(w[2]) and g[4] == w[4], (fmt, k, g[2], w[2])
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[3], w[3]), (fmt, k)
            exp = bufs[k].copy()
            n = R.draw(exp, lays[k], dict(name=None, joints=g[0], parents=R.PARENTS, rect=list(g[2])))
            assert n > 0 and np.array_equal(pool.get(ptrs[k]), exp), (fmt, k, int((pool.get(ptrs[k]) != exp).sum()))
        assert e.handle.track_box(0) is not None
    finally:
        e.close()


def test_tracked_draw_with_hold_and_a_threshold(pool):
    """lost=(.., "hold") and a style with min_confidence: the limbs with an end below the threshold are absent, the results are those of
    the loop without drawing, and the held box is the rect drawn."""
    from vnect_amd import _native, runner
    bufs, lays = _frames("bgr")
    times, rect = _times(4, 3), [9, 5, 90, 70]
    e = _est(lanes=2)
    try:
        _, plain = _device_copies(pool, bufs, lays)
        lost = (0.5, 21, "hold")
        want = list(runner.track_on_device(e, plain, rect=rect, timestamps=times, ahead=1, source="device", confidence=True, lost=lost))
        thr = float(np.median(np.concatenate([w[3] for w in want])))      # some joints of the run lie below it, some above
        e.reset()
        ptrs, drawn = _device_copies(pool, bufs, lays)
        style = _native.overlay_style(thr, ((5, 250, 5), (250, 5, 5)), e.joint_parents)
        got = list(runner.track_on_device(e, drawn, rect=rect, timestamps=times, ahead=1, source="device", confidence=True, lost=lost, draw=style))
        absent = 0
        for k, (g, w) in enumerate(zip(got, want)):
            assert list(g[2]) == list(w[2]) and g[4] == w[4] and all(np.array_equal(g[i], w[i]) for i in (0, 1, 3)), k
            exp, every = bufs[k].copy(), bufs[k].copy()
            case = dict(name=None, joints=g[0], parents=R.PARENTS, rect=list(g[2]), conf=g[3], thr=thr)
            R.draw(exp, lays[k], case, (5, 250, 5), (250, 5, 5))
            R.draw(every, lays[k], dict(case, conf=None, thr=None), (5, 250, 5), (250, 5, 5))
            assert np.array_equal(pool.get(ptrs[k]), exp), k
            absent += int((exp != every).sum())
        assert absent > 0                                                   # the threshold took limbs away
    finally:
        e.close()


def test_refused_crop_is_not_drawn_and_break_leaves_nothing_in_flight(pool):
    """A stream stopped by a refused crop (the initial rect, as in tests/test_gpu_track.py) leaves its frames undrawn; the refusals of
    vnect_submit_tracked_device are this call's too; and a loop the caller leaves early has nothing in flight afterwards."""
    from vnect_amd import _native, runner
    Hb, Wb = 480, 1000
    lay = dict(name="big", format=0, H=Hb, W=Wb, data_off=0, uv_off=0, sy=3 * Wb, sx=3, sc=1, uv_stride=0, size=Hb * Wb * 3)
    before = R.fresh(lay, 9)
    e = _est(lanes=2)
    try:
        h = e.handle
        tg = [_target(pool, lay, before) for _ in range(2)]
        h.track_begin(0, Hb, Wb, [0, 10, 1000, 1])
        style = _native.overlay_style(parents=e.joint_parents)
        with pytest.raises(ValueError, match="vnect_submit_tracked_device_draw: .*takes no rect"):
            h.submit_tracked_device_draw(0, _native.device_frame(tg[0][1], "bgr", (0, 0, 5, 5)), *_times(1)[0], style=style)
        bad = _native.overlay_style(parents=[0] * 20 + [33])
        with pytest.raises(ValueError, match="vnect_submit_tracked_device_draw: .*parent"):
            h.submit_tracked_device_draw(0, _native.device_frame(tg[0][1]), *_times(1)[0], style=bad)
        times = _times(2)
        for k in range(2):
            h.submit_tracked_device_draw(0, _native.device_frame(tg[k][1]), *times[k], _native.STREAM_SYNCED, style)
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_ARG
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_STATE
        for p, _, _ in tg:
            assert np.array_equal(pool.get(p), before)
        # an early break: the frames still in flight are collected and dropped, and the estimator serves a frame at once
        bufs, lays = _frames("bgr")
        _, drawn = _device_copies(pool, bufs, lays)
        for k, _ in enumerate(runner.track_on_device(e, drawn, timestamps=_times(4, 5), ahead=1, source="device", draw=True)):
            if k == 1:
                break
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_STATE and "nothing in flight" in str(err.value)
        j2, _ = e(R.view(bufs[0], lays[0]).copy(), timestamp=_times(5, 6)[4])
        assert j2.shape == (21, 2) and np.all(np.isfinite(j2))
    finally:
        e.close()


def test_torch_tensors_in_every_layout():
    """a child process that imports torch first: est.draw on packed, permuted, 4-byte, sliced, transposed, RGB and NV12 tensors equals
    render.draw_limbs_2d_exact on their host copies, storage and all"""
    r = subprocess.run([sys.executable, "-m", "tests.overlay_torch_child"], cwd=R.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "overlay child ok"
