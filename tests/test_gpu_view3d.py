"""GPU: the 3-D view through the C ABI (vnect_view3d_device, vnect_track_view3d, vnect_result_view3d) and the Python layers above it
(VIEW3D.md).

What the device writes must be exactly render.view3d_exact of the same joints -- to a numpy array, to device memory, into a column block
of a wider canvas beside a preview -- and every refusal is VNECT_E_ARG with nothing written.  A tracked loop that asks for views must yield
exactly what the same loop yields without them, bit for bit, and each view must be render.view3d_exact of the joints_3d yielded with it.
The device memory comes from the device-frame probe's allocator and is described to the library by a bare __cuda_array_interface__
(tests/devframe_ref.py: FakeCuda), so nothing here needs torch -- except the child process, which is about torch.  Frames, device copies
and the estimator of the tracked loops come from the helpers of tests/test_gpu_overlay.py."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import overlay_ref as R
from tests import test_gpu_overlay as ov
from tests import view3d_ref as V

pytestmark = pytest.mark.gpu

pool = ov.pool


def _exact(case, rows, cols):
    from vnect_amd import render
    return render.view3d_exact(case["joints"], (rows, cols), case.get("view"), case.get("extent", 500.0), case.get("line_width", 3.0),
                               case.get("background"), case.get("colors"), case.get("parents"), case.get("conf"), case.get("thr"),
                               "rgb" if case.get("fmt") else "bgr", case.get("order", 0))


def _spec(case, rows, cols):
    from vnect_amd import _native
    return _native.view3d_spec((rows, cols), case.get("view"), case.get("extent", 500.0), case.get("line_width", 3.0), case.get("background"),
                               case.get("colors"), case.get("parents"), case.get("thr"), "rgb" if case.get("fmt") else "bgr", case.get("order", 0))


def test_view3d_device_on_a_preprocess_only_handle(pool):
    """vnect_view3d_device needs no weights and no plan: every case of the CPU tests at 33 x 65, to pageable host memory (pitched) and to a
    pitched device buffer at an odd address whose every other byte keeps its canary; a NULL spec is the reference's 400 x 400 view"""
    from vnect_amd import _native
    h = _native.Handle([1.0], preprocess_only=True)
    try:
        rows, cols = 33, 65
        for k, case in enumerate(V.cases(rows, cols)):
            want = _exact(case, rows, cols)
            spec = _spec(case, rows, cols)
            host = np.full((rows, 3 * cols + 5), V.CANARY, np.uint8)
            h.view3d_device(case["joints"], spec, host.ctypes.data, 3 * cols + 5, case.get("conf"))
            assert np.array_equal(host[:, :3 * cols].reshape(rows, cols, 3), want) and (host[:, 3 * cols:] == V.CANARY).all(), (k, "host")
            buf, pitch = V.out_buffer(rows, cols, k % 4, 7)
            q = pool.put(np.concatenate([buf, np.full(64, V.CANARY, np.uint8)]))
            h.view3d_device(case["joints"], spec, q + k % 4, pitch, case.get("conf"))
            got = pool.get(q)
            assert np.array_equal(got[:len(buf)], V.whole(want, k % 4, pitch)) and (got[len(buf):] == V.CANARY).all(), (k, "device")
        j = V.skeleton(3)
        pic = np.zeros((400, 400, 3), np.uint8)
        h.view3d_device(j, None, pic.ctypes.data, 1200)
        assert np.array_equal(pic, V.view(j)) and (pic != 255).any()
    finally:
        h.close()


def test_est_view3d_numpy_device_and_a_canvas_beside_the_preview(pool):
    from tests import planted as pl
    from tests import preview_ref as P
    from vnect_amd import VNectEstimator, render
    est = VNectEstimator(weights=pl.weights(noise=1.0), verbose=False)
    try:
        j = V.skeleton(21)
        conf = np.linspace(1.0, 0.0, 21)
        assert list(est.joint_parents) == V.PARENTS
        got = est.view3d(j)
        assert got.shape == (400, 400, 3) and np.array_equal(got, render.view3d_exact(j)) and np.array_equal(got, V.view(j))
        R20 = render.view_matrix(20, -60)
        got = est.view3d(j, (120, 200), R20, confidence=conf, min_confidence=0.3, order=1, out_format="rgb", line_width=5.0)
        assert np.array_equal(got, render.view3d_exact(j, (120, 200), R20, confidence=conf, min_confidence=0.3, order=1, out_format="rgb", line_width=5.0))
        assert np.array_equal(got, V.view(j, 120, 200, view=R20, conf=conf, thr=0.3, order=1, fmt=1, line_width=5.0))
        # into a numpy array: the right-hand block of a wider host canvas
        canvas = np.full((64, 100 + 64, 3), V.CANARY, np.uint8)
        assert est.view3d(j, 64, out=canvas[:, 100:]) is not None
        assert np.array_equal(canvas[:, 100:], render.view3d_exact(j, 64)) and (canvas[:, :100] == V.CANARY).all()
        with pytest.raises(ValueError, match="out must be"):
            est.view3d(j, 64, out=canvas[:, 99:])
        # one device canvas: est.preview fills the left block, est.view3d the right one; neither touches the other's block or the margin
        H, W = 70, 50
        lay = P.layouts(H, W)[0]
        case = P.skeleton(H, W)
        src = P.fresh(lay)
        p = pool.put(src)
        frame = dr.FakeCuda(p + lay["data_off"], (H, W, 3), (lay["sy"], lay["sx"], lay["sc"]))
        pv = render.preview_exact(P.picture(src, lay, 0), case["joints"], case["parents"], case["rect"], factor=1.0)
        assert pv.shape == (H, W, 3)
        cw = W + H + 3                                                        # preview | view (H x H) | a margin of 3 pixels
        margin = 16
        q = pool.put(np.full(margin + H * cw * 3 + margin, V.CANARY, np.uint8))
        left = dr.FakeCuda(q + margin, (H, W, 3), (3 * cw, 3, 1))
        right = dr.FakeCuda(q + margin + 3 * W, (H, H, 3), (3 * cw, 3, 1))
        assert est.preview(frame, case["joints"], rect=case["rect"], factor=1.0, out=left) is left
        after_preview = pool.get(q)[margin:margin + H * cw * 3].reshape(H, cw, 3).copy()
        assert np.array_equal(after_preview[:, :W], pv) and (after_preview[:, W:] == V.CANARY).all()
        assert est.view3d(j, H, out=right) is right
        whole = pool.get(q)
        both = whole[margin:margin + H * cw * 3].reshape(H, cw, 3)
        assert np.array_equal(both[:, :W], pv) and np.array_equal(both[:, W:W + H], render.view3d_exact(j, H))
        assert (both[:, W + H:] == V.CANARY).all() and (whole[:margin] == V.CANARY).all() and (whole[-margin:] == V.CANARY).all()
        assert np.array_equal(pool.get(p), src)
    finally:
        est.close()


def test_refusals_write_nothing(pool):
    from vnect_amd import _native
    L = _native.lib()
    rows, cols = 33, 65
    j = np.ascontiguousarray(V.skeleton(5), np.float32)
    canary = np.full(rows * cols * 3 + 64, V.CANARY, np.uint8)
    q = pool.put(canary)
    other = pool.put(np.zeros(4096, np.uint8))
    rng = np.zeros(2, np.int64)
    assert pool.probe.ip_range(other, rng.ctypes.data_as(dr.i64p)) == 0 and rng[0] <= other and rng[1] >= 4096
    near_end = int(rng[0] + rng[1]) - 100
    host = np.full(rows * cols * 3, V.CANARY, np.uint8)
    h = _native.Handle([1.0], preprocess_only=True)

    def raw(spec=None, out=None, pitch=3 * cols, joints=j):
        spec = _native.view3d_spec((rows, cols)) if spec is None else spec
        rc = L.vnect_view3d_device(h._h, None if joints is None else joints.ctypes.data_as(V.f32p), None, C.byref(spec), C.c_void_p(q if out is None else out), pitch)
        return rc, L.vnect_last_error(h._h).decode()

    def spec(**over):
        s = _native.view3d_spec((rows, cols))
        for k, v in over.items():
            if k == "view_nan":
                s.has_view = 1
                for i in range(9):
                    s.view[i] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, v)[i]
            elif k == "parent":
                s.has_parents = 1
                s.parents[3] = v
            elif k == "colour":
                s.has_colors = 1
                s.colors_bgr[20][2] = v
            elif k == "bg":
                s.has_background = 1
                s.background_bgr[1] = v
            else:
                setattr(s, k, v)
        return s

    try:
        cases = [
            ("a wrong struct_size", dict(spec=spec(struct_size=16)), "struct_size"),
            ("rows of 2049", dict(spec=spec(rows=2049)), "1 .. 2048"),
            ("cols of -1", dict(spec=spec(cols=-1)), "1 .. 2048"),
            ("a pitch below 3 cols", dict(pitch=3 * cols - 1), "out_pitch"),
            ("a negative extent", dict(spec=spec(extent=-500.0)), "extent"),
            ("an infinite extent", dict(spec=spec(extent=float("inf"))), "extent"),
            ("a NaN extent", dict(spec=spec(extent=float("nan"))), "extent"),
            ("a NaN view entry", dict(spec=spec(view_nan=float("nan"))), "view"),
            ("an infinite view entry", dict(spec=spec(view_nan=float("-inf"))), "view"),
            ("a line_width of 64.5", dict(spec=spec(line_width=64.5)), "line_width"),
            ("a negative line_width", dict(spec=spec(line_width=-1.0)), "line_width"),
            ("a NaN line_width", dict(spec=spec(line_width=float("nan"))), "line_width"),
            ("a colour of 256", dict(spec=spec(colour=256)), "0 .. 255"),
            ("a background of -1", dict(spec=spec(bg=-1)), "0 .. 255"),
            ("a parent of 21", dict(spec=spec(parent=21)), "parent"),
            ("a parent of -1", dict(spec=spec(parent=-1)), "parent"),
            ("an order of 2", dict(spec=spec(order=2)), "order"),
            ("an NV12 output", dict(spec=spec(out_format=_native.PIX_NV12)), "out_format"),
            ("an output past its allocation's end", dict(out=near_end), "past the end of the allocation"),
            ("a null output", dict(out=0), "no output"),
            ("no joints", dict(joints=None), "no joints"),
        ]
        for what, kw, text in cases:
            rc, msg = raw(**kw)
            assert rc == _native.E_ARG and text in msg and msg.startswith("vnect_view3d_device: "), (what, rc, msg)
            assert np.array_equal(pool.get(q), canary) and (pool.get(other) == 0).all(), what
        rc, msg = raw(spec=spec(rows=2049), out=host.ctypes.data)          # a host output is not written either
        assert rc == _native.E_ARG and (host == V.CANARY).all()
        with pytest.raises(ValueError, match="vnect_view3d_device: .*order"):      # the Python layer: a ValueError, like every refused argument
            h.view3d_device(j, spec(order=5), q, 3 * cols)
        with pytest.raises(ValueError, match="vnect_track_view3d: .*stream"):
            h.track_view3d(99, spec())
        with pytest.raises(ValueError, match="vnect_track_view3d: .*order"):
            h.track_view3d(0, spec(order=5))
        assert h.result_view3d() is None
        # and the handle goes on
        assert raw()[0] == 0
        got = pool.get(q)
        assert np.array_equal(got[:rows * cols * 3].reshape(rows, cols, 3), V.view(j, rows, cols)) and (got[rows * cols * 3:] == V.CANARY).all()
    finally:
        h.close()


def _host_frames(bufs, lays):
    return [np.ascontiguousarray(R.view(b, lay)) for b, lay in zip(bufs, lays)]


@pytest.mark.parametrize("source", ["pinned", "resident", "device"])
def test_tracked_loop_with_view3d(pool, source):
    """track_on_device(..., view3d=True) over 4 frames, submitted ahead on two lanes: what it yields is what view3d=False yields, bit for
    bit, and every view is render.view3d_exact of the joints_3d yielded with it"""
    from vnect_amd import render, runner
    bufs, lays = ov._frames("bgr")
    kw = dict(rect=[9, 5, 90, 70], timestamps=ov._times(4), ahead=2, source=source, confidence=True)
    e = ov._est(lanes=2)
    try:
        def frames():
            return ov._device_copies(pool, bufs, lays)[1] if source == "device" else _host_frames(bufs, lays)
        want = list(runner.track_on_device(e, frames(), **kw))
        e.reset()
        got = list(runner.track_on_device(e, frames(), view3d=True, **kw))
        assert len(got) == len(want) == 4
        seen = set()
        for k, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w) + 1 and list(g[2]) == list(w[2]) and g[4] == w[4], (source, k)
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[3], w[3]), (source, k)
            exp = render.view3d_exact(g[1])
            assert g[5].shape == (400, 400, 3) and np.array_equal(g[5], exp), (source, k, int((g[5] != exp).sum()))
            assert (exp != 255).any(), (source, k, "nothing drawn")
            seen.add(g[5].tobytes())
        assert len(seen) > 1                                   # the frames' views differ: each is its own frame's
        assert e.handle.result_view3d() is not None
        # the setting is off again: a plain loop delivers no view
        e.reset()
        again = list(runner.track_on_device(e, frames(), **kw))
        assert len(again[0]) == len(want[0]) and e.handle.result_view3d() is None
    finally:
        e.close()


def test_two_videos_each_get_their_own_view():
    """track_many_on_device: two videos on two streams of one handle, their frames overlapping on its lanes"""
    from vnect_amd import render, runner
    bufs, lays = ov._frames("bgr")
    a = _host_frames(bufs, lays)
    videos = [a, a[::-1]]
    kw = dict(rects=[[9, 5, 90, 70], [20, 10, 80, 60]], timestamps=[ov._times(4), ov._times(4, 9)], ahead=1, source="pinned")
    e = ov._est(lanes=2)
    try:
        want = list(runner.track_many_on_device(e, videos, **kw))
        e.reset()
        got = list(runner.track_many_on_device(e, videos, view3d=True, **kw))
        assert len(got) == len(want) == 8
        for k, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0] and list(g[3]) == list(w[3]) and np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]), k
            assert np.array_equal(g[4], render.view3d_exact(g[2])), k
    finally:
        e.close()


def test_tracked_view3d_beside_draw_preview_and_hold(pool):
    """draw=True, preview= and lost=(.., "hold") alongside, and a spec of its own (a threshold, order 1, RGB, 33 x 65, a tilted view)"""
    from vnect_amd import _native, render, runner
    bufs, lays = ov._frames("bgr")
    kw = dict(rect=[9, 5, 90, 70], timestamps=ov._times(4), ahead=2, source="device", confidence=True, lost=(0.5, 21, "hold"))
    R20 = render.view_matrix(20, -60)
    e = ov._est(lanes=2)
    try:
        _, plain = ov._device_copies(pool, bufs, lays)
        want = list(runner.track_on_device(e, plain, draw=True, preview=0.5, **kw))
        e.reset()
        _, frames = ov._device_copies(pool, bufs, lays)
        spec = _native.view3d_spec((33, 65), R20, min_confidence=0.2, order=1, out_format="rgb", parents=e.joint_parents)
        got = list(runner.track_on_device(e, frames, draw=True, preview=0.5, view3d=spec, **kw))
        assert len(got) == len(want) == 4
        for k, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w) + 1 and list(g[2]) == list(w[2]) and g[4] == w[4], k
            assert all(np.array_equal(g[i], w[i]) for i in (0, 1, 3, 5)), k
            exp = render.view3d_exact(g[1], (33, 65), R20, confidence=g[3], min_confidence=0.2, order=1, out_format="rgb")
            assert np.array_equal(g[6], exp), (k, int((g[6] != exp).sum()))
    finally:
        e.close()


def test_refused_crop_break_and_state(pool):
    from vnect_amd import _native, render, runner
    bufs, lays = ov._frames("bgr")
    e = ov._est(lanes=2)
    try:
        h = e.handle
        # an early break: the frames still in flight are collected and dropped, and the estimator serves a frame at once
        for k, res in enumerate(runner.track_on_device(e, _host_frames(bufs, lays), timestamps=ov._times(4), ahead=1, view3d=True)):
            assert np.array_equal(res[3], render.view3d_exact(res[1]))
            if k == 1:
                break
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_STATE and "nothing in flight" in str(err.value)
        j2, _ = e(_host_frames(bufs, lays)[0], timestamp=ov._times(5, 1)[4])
        assert j2.shape == (21, 2) and np.all(np.isfinite(j2))
        # changing the setting with a frame in flight: VNECT_E_STATE, and nothing changes
        e.reset()
        h.track_begin(0, ov.H, ov.W, None)
        small = _native.view3d_spec(48, parents=e.joint_parents)
        h.track_view3d(0, small)
        _, frames = ov._device_copies(pool, bufs, lays)
        t = ov._times(3, 2)
        h.submit_tracked_device(0, _native.device_frame(frames[0]), *t[0], _native.STREAM_SYNCED)
        for new in (_native.view3d_spec(800), None):
            with pytest.raises(_native.VnectError) as err:
                h.track_view3d(0, new)
            assert err.value.code == _native.E_STATE and "in flight" in str(err.value)
        _, j2, j3, used = h.collect_tracked()
        assert np.array_equal(h.result_view3d(), render.view3d_exact(j3, 48))
        h.track_view3d(0, None)
        h.submit_tracked_device(0, _native.device_frame(frames[1]), *t[1], _native.STREAM_SYNCED)
        h.collect_tracked()
        assert h.result_view3d() is None                                       # off: the next frame has none
        # a stream stopped by a refused crop (the initial rect, as in tests/test_gpu_track.py): its frame has no view
        e.reset()
        Hb, Wb = 480, 1000
        lay = dict(name="big", format=0, H=Hb, W=Wb, data_off=0, uv_off=0, sy=3 * Wb, sx=3, sc=1, uv_stride=0, size=Hb * Wb * 3)
        p, arr, _ = ov._target(pool, lay, R.fresh(lay, 9))
        h.track_begin(0, Hb, Wb, [0, 10, 1000, 1])
        h.track_view3d(0, small)
        h.submit_tracked_device(0, _native.device_frame(arr), *ov._times(1, 6)[0], _native.STREAM_SYNCED)
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_ARG and h.result_view3d() is None
        h.track_view3d(0, None)
    finally:
        e.close()


def test_torch_tensors():
    """a child process that imports torch first: est.view3d into a CUDA tensor and into the right-hand block of a canvas tensor whose left
    block est.preview filled equals render.view3d_exact, and nothing else of the canvas changes"""
    r = subprocess.run([sys.executable, "-m", "tests.view3d_torch_child"], cwd=R.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "view3d child ok"
