"""GPU: previews delivered by the tracked device loop (vnect_submit_tracked_device_preview, vnect_result_preview,
runner.track_on_device(..., preview=); PREVIEW.md).

A loop that asks for previews must yield exactly what the same loop yields without them -- joints, rects, confidences, lost flags, bit for
bit -- and each preview must be render.preview_exact of that frame's oriented picture with the frame's own yielded joints and rect_used.
The frames are never written, unless draw= is given too: then the preview is that of the clean frame and the frame is what draw=True
alone leaves.  Frames, device copies and the estimator come from the helpers of tests/test_gpu_overlay.py."""
import numpy as np
import pytest

from tests import overlay_ref as R
from tests import preview_ref as P
from tests import test_gpu_overlay as ov

pytestmark = pytest.mark.gpu

pool = ov.pool


def _exact(buf, lay, o, j2, used, f, **kw):
    from vnect_amd import render
    return render.preview_exact(P.picture(buf, lay, o), j2, R.PARENTS, list(used), factor=f, **kw)


@pytest.mark.parametrize("hold", [False, True], ids=["plain", "hold"])
@pytest.mark.parametrize("code", [0, 3])
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_tracked_loop_with_preview(pool, fmt, code, hold):
    from vnect_amd import render, runner
    bufs, lays = ov._frames(fmt)
    times = ov._times(4)
    rect = [9, 5, 90, 70] if code == 0 else [5, 9, 70, 90]                 # in the picture's coordinates
    factor = None if fmt == "bgr" else 0.37
    kw = dict(rect=rect, timestamps=times, ahead=1, source="device", pixel_format=fmt, confidence=True, orientation=code)
    if hold:
        kw["lost"] = (0.5, 21, "hold")
    e = ov._est(lanes=2)
    try:
        _, plain = ov._device_copies(pool, bufs, lays)
        want = list(runner.track_on_device(e, plain, **kw))
        e.reset()
        ptrs, frames = ov._device_copies(pool, bufs, lays)
        got = list(runner.track_on_device(e, frames, preview=True if factor is None else factor, **kw))
        assert len(got) == len(want) == 4
        for k, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w) + 1 and list(g[2]) == list(w[2]) and g[4] == w[4], (fmt, code, k, g[2], w[2])
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(g[3], w[3]), (fmt, code, k)
            exp = _exact(bufs[k], lays[k], code, g[0], g[2], factor)
            assert g[5].shape == exp.shape and np.array_equal(g[5], exp), (fmt, code, k, int((g[5] != exp).sum()))
            assert (exp != render.preview_exact(P.picture(bufs[k], lays[k], code), None, R.PARENTS, None, factor=factor)).any(), (fmt, code, k, "not annotated")
            assert np.array_equal(pool.get(ptrs[k]), bufs[k]), (fmt, code, k, "the frame was written")
    finally:
        e.close()


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_draw_and_preview_together(pool, fmt):
    """draw=True, preview=True: the preview launch runs in front of the overlay launch -- it shows the clean frame annotated by the rule in
    the BGR domain -- and the frame is left as draw=True alone leaves it"""
    from vnect_amd import runner
    bufs, lays = ov._frames(fmt)
    kw = dict(rect=[9, 5, 90, 70], timestamps=ov._times(4), ahead=1, source="device", pixel_format=fmt)
    e = ov._est(lanes=2)
    try:
        _, plain = ov._device_copies(pool, bufs, lays)
        want = list(runner.track_on_device(e, plain, **kw))
        e.reset()
        ptrs, frames = ov._device_copies(pool, bufs, lays)
        got = list(runner.track_on_device(e, frames, draw=True, preview=0.5, **kw))
        for k, (g, w) in enumerate(zip(got, want)):
            assert list(g[2]) == list(w[2]) and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), (fmt, k)
            assert np.array_equal(g[3], _exact(bufs[k], lays[k], 0, g[0], g[2], 0.5)), (fmt, k, "the preview is not the clean frame's")
            drawn = bufs[k].copy()
            assert R.draw(drawn, lays[k], dict(name=None, joints=g[0], parents=R.PARENTS, rect=list(g[2]))) > 0
            assert np.array_equal(pool.get(ptrs[k]), drawn), (fmt, k, "the frame is not what draw=True leaves")
    finally:
        e.close()


def test_refused_crop_break_resize_and_refusals(pool):
    from vnect_amd import _native, runner
    Hb, Wb = 480, 1000
    lay = dict(name="big", format=0, H=Hb, W=Wb, data_off=0, uv_off=0, sy=3 * Wb, sx=3, sc=1, uv_stride=0, size=Hb * Wb * 3)
    before = R.fresh(lay, 9)
    e = ov._est(lanes=2)
    try:
        h = e.handle
        assert h.result_preview() is None                                     # nothing delivered yet
        # an early break: the frames still in flight are collected and dropped, and the estimator serves a frame at once
        bufs, lays = ov._frames("bgr")
        _, frames = ov._device_copies(pool, bufs, lays)
        for k, res in enumerate(runner.track_on_device(e, frames, timestamps=ov._times(4), ahead=1, source="device", preview=0.25)):
            assert res[3].shape == (24, 32, 3)
            if k == 1:
                break
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_STATE and "nothing in flight" in str(err.value)
        j2, _ = e(R.view(bufs[0], lays[0]).copy(), timestamp=ov._times(5, 1)[4])
        assert j2.shape == (21, 2) and np.all(np.isfinite(j2))
        # a larger preview while a frame is in flight: refused (the ring's buffers are re-sized only while nothing is in flight), nothing changes
        e.reset()
        h.track_begin(0, ov.H, ov.W, None)
        style = _native.overlay_style(parents=e.joint_parents)
        t = ov._times(3, 2)
        h.submit_tracked_device_preview(0, _native.device_frame(frames[0]), *t[0], _native.STREAM_SYNCED, style, _native.preview_spec(0.25))
        with pytest.raises(_native.VnectError) as err:
            h.submit_tracked_device_preview(0, _native.device_frame(frames[1]), *t[1], _native.STREAM_SYNCED, style, _native.preview_spec(2.0))
        assert err.value.code == _native.E_STATE and "in flight" in str(err.value)
        _, j2, _, used = h.collect_tracked()
        assert np.array_equal(h.result_preview(), _exact(bufs[0], lays[0], 0, j2, used, 0.25))
        # the refusals of the style, the spec and the frame are this call's, before anything changes
        for kw, text in ((dict(style=_native.overlay_style(parents=[0] * 20 + [33])), "parent"), (dict(spec=_native.preview_spec(-1.0)), "factor"),
                         (dict(spec=_native.preview_spec(100.0)), "4096"), (dict(frame=_native.device_frame(frames[1], "bgr", (0, 0, 5, 5))), "takes no rect")):
            with pytest.raises(ValueError, match="vnect_submit_tracked_device_preview: .*" + text):
                h.submit_tracked_device_preview(0, kw.get("frame", _native.device_frame(frames[1])), *t[1], _native.STREAM_SYNCED, kw.get("style", style),
                                                kw.get("spec", _native.preview_spec(0.25)))
        with pytest.raises(ValueError, match="source='device'"):
            next(runner.track_on_device(e, [R.view(bufs[0], lays[0])], preview=True))
        # a change of frame size between two loops re-sizes the ring: larger frames, the default factor
        e.reset()
        big = [np.ascontiguousarray(f) for f in runner.synthetic_stream(0, 2, 120, 160)]
        blay = P.plain_layout(120, 160)
        _, bframes = ov._device_copies(pool, [f.reshape(-1) for f in big], [blay] * 2)
        got = list(runner.track_on_device(e, bframes, timestamps=ov._times(2, 4), ahead=1, source="device", preview=True))
        assert len(got) == 2
        for k, g in enumerate(got):
            assert g[3].shape == (768, 1024, 3) and np.array_equal(g[3], _exact(big[k].reshape(-1), blay, 0, g[0], g[2], None)), k
        # a stream stopped by a refused crop (the initial rect, as in tests/test_gpu_track.py): its frame has no preview
        e.reset()
        p, arr, _ = ov._target(pool, lay, before)
        h.track_begin(0, Hb, Wb, [0, 10, 1000, 1])
        h.submit_tracked_device_preview(0, _native.device_frame(arr), *ov._times(1, 6)[0], _native.STREAM_SYNCED, style, _native.preview_spec(0.25))
        with pytest.raises(_native.VnectError) as err:
            h.collect_tracked()
        assert err.value.code == _native.E_ARG and h.result_preview() is None and np.array_equal(pool.get(p), before)
    finally:
        e.close()
