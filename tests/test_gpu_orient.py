"""GPU: orientation through the C ABI (vnect_set_orientation) and the Python layers above it (ORIENTATION.md).

THE CONTRACT: every result of an entry point given a stored frame under orientation o is bit-identical to the same entry point given
np.ascontiguousarray(oriented picture) under orientation 0 -- slot bytes, input batches, joints, confidences, rects, filter state.  The
oriented picture is tests/orient_ref.py's two lines of numpy.  Device memory comes from the device-frame probe's allocator and is described
by a bare __cuda_array_interface__ (tests/devframe_ref.py), so nothing here needs torch."""
import ctypes as C

import numpy as np
import pytest

from . import devframe_ref as dr
from . import nv12_ref
from . import orient_ref as orf

pytestmark = pytest.mark.gpu

T0 = 1.7e9
SIZES = [(96, 128), (130, 70)]
_CACHE = {}


def _weights(planted=False):
    if planted not in _CACHE:
        if planted:
            from tests import planted as pl
            _CACHE[planted] = pl.weights(noise=1.0)
        else:
            from vnect_amd.weights import synthetic_weights
            _CACHE[planted] = synthetic_weights()
    return _CACHE[planted]


def _est(planted=False, **kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=_weights(planted), verbose=False, **kw)


def _times(n, base=0.0):
    return [(T0 + base + 0.033 * k + 0.002 * (k % 3), T0 + base + 0.033 * k + 0.0005) for k in range(n)]


class Pool:
    """device allocations of one test, freed at its end"""

    def __init__(self, probe):
        self.probe, self.ptrs = probe, {}

    def put(self, buf):
        buf = np.ascontiguousarray(buf).reshape(-1)
        p = C.c_void_p()
        assert self.probe.ip_alloc(len(buf), C.byref(p)) == 0 and p.value
        self.ptrs[p.value] = len(buf)
        assert self.probe.ip_h2d(p.value, buf.ctypes.data, len(buf)) == 0
        return p.value

    def get(self, p):
        out = np.zeros(self.ptrs[p], np.uint8)
        assert self.probe.ip_d2h(out.ctypes.data, p, len(out)) == 0
        return out

    def frame(self, form, order, bgr, off=1, pad=5, seed=0):
        """the BGR picture `bgr` stored in `form` / `order` in device memory -> the (H, W, 3) device array"""
        lay = dr.Layout(form, bgr.shape[0], bgr.shape[1], off, pad)
        p = self.put(lay.place(dr.as_bgr(bgr, order), seed))
        return dr.FakeCuda(p + lay.off, (lay.H, lay.W, 3), (lay.sy, lay.sx, lay.sc))

    def nv12(self, img, two=False):
        H, W = img.shape[0] * 2 // 3, img.shape[1]
        if not two:
            return dr.FakeCuda(self.put(img), img.shape, (W, 1))
        ys, uvs = W + 3, W + 5
        yb, ub = np.zeros((H, ys), np.uint8), np.zeros((H // 2, uvs), np.uint8)
        yb[:, :W], ub[:, :W] = img[:H], img[H:]
        return (dr.FakeCuda(self.put(yb.reshape(-1)[:(H - 1) * ys + W]), (H, W), (ys, 1)),
                dr.FakeCuda(self.put(ub.reshape(-1)[:(H // 2 - 1) * uvs + W]), (H // 2, W), (uvs, 1)))

    def close(self):
        for p in self.ptrs:
            self.probe.ip_free(p)
        self.ptrs = {}


@pytest.fixture(scope="module")
def probe():
    return dr.load_probe()


@pytest.fixture()
def pool(probe):
    p = Pool(probe)
    yield p
    p.close()


@pytest.fixture(scope="module")
def est():
    e = _est()
    yield e
    e.close()


def _pic(bgr, o):
    return np.ascontiguousarray(orf.oriented(bgr, o))


def _crop(pic, rect):
    if rect is None:
        return pic
    x, y, w, h = rect
    return np.ascontiguousarray(pic[y:y + h, x:x + w])


def _rects(o, H, W):
    """None, an odd-origin crop, and one that runs past the far edges (clipped as numpy clips it), in ORIENTED coordinates"""
    Ho, Wo = orf.oriented_size(o, H, W)
    return [None, (5, 3, Wo - 11, Ho - 9), (Wo - 30, Ho - 20, 500, 500)]


@pytest.mark.parametrize("o", orf.CODES)
def test_upload_then_read_frame_is_the_oriented_crop(est, pool, o):
    """every source of a frame: what vnect_read_frame returns is the oriented picture (its crop), byte for byte"""
    from vnect_amd import _native
    h = est.handle
    try:
        for (H, W) in SIZES:
            bgr = dr.pixels(H, W, 7 * o + H)
            nv = nv12_ref.content(H, W, 2 * (o + H))
            nbgr = nv12_ref.restate(nv)
            h.set_orientation(o)
            pic, npic = _pic(bgr, o), _pic(nbgr, o)
            h.upload_frame(0, bgr)                                   # pageable BGR
            assert np.array_equal(h.read_frame(0), pic), ("pageable bgr", o, H, W)
            h.upload_frame(1, np.ascontiguousarray(np.pad(bgr, ((0, 0), (0, 3), (0, 0))))[:, :W])   # ... row-strided
            assert np.array_equal(h.read_frame(1), pic), ("strided bgr", o, H, W)
            buf = h.frame_buffer(0, H, W)                            # BGR in a pinned buffer
            buf[...] = bgr
            h.upload_frame(0, buf)
            assert np.array_equal(h.read_frame(0), pic), ("pinned bgr", o, H, W)
            nbuf = h.frame_buffer_nv12(1, H, W)
            nbuf[...] = nv
            for rect in _rects(o, H, W):
                h.upload_frame_nv12(0, nv, rect)                     # pageable NV12
                assert np.array_equal(h.read_frame(0), _crop(npic, rect)), ("pageable nv12", o, H, W, rect)
                h.upload_frame_nv12(1, nbuf, rect)                   # pinned NV12
                assert np.array_equal(h.read_frame(1), _crop(npic, rect)), ("pinned nv12", o, H, W, rect)
                for name, form, order in (("bgr", dr.PACKED3, 0), ("rgb", dr.PACKED3, 1), ("bgra", dr.PACKED4, 0), ("planar", dr.PLANAR, 1),
                                          ("strided", dr.GENERIC, 0)):
                    arr = pool.frame(form, order, bgr, seed=o)
                    h.upload_frame_device(2, _native.device_frame(arr, "rgb" if order else "bgr", rect), _native.STREAM_SYNCED)
                    assert np.array_equal(h.read_frame(2), _crop(pic, rect)), ("device " + name, o, H, W, rect)
                for two in (False, True):
                    h.upload_frame_device(3, _native.device_frame(pool.nv12(nv, two), "nv12", rect), _native.STREAM_SYNCED)
                    assert np.array_equal(h.read_frame(3), _crop(npic, rect)), ("device nv12", two, o, H, W, rect)
            pool.close()
    finally:
        h.set_orientation(0)


@pytest.mark.parametrize("o", [1, 3, 6, 7])
def test_preprocess_batches_are_equal(est, pool, o):
    from vnect_amd import _native
    h = est.handle
    H, W = SIZES[0]
    bgr, nv = dr.pixels(H, W, 40 + o), nv12_ref.content(H, W, 2 * o)
    pic, npic = _pic(bgr, o), _pic(nv12_ref.restate(nv), o)
    rect = _rects(o, H, W)[1]
    base0, want, nwant = h.preprocess(bgr), h.preprocess(pic), h.preprocess(_crop(npic, rect))
    dwant = h.preprocess(_crop(pic, rect))
    try:
        h.set_orientation(o)
        for got, exp, tag in ((h.preprocess(bgr), want, "bgr"), (h.preprocess_nv12(nv, rect), nwant, "nv12"),
                              (h.preprocess_device(_native.device_frame(pool.frame(dr.PACKED3, 0, bgr), "bgr", rect), _native.STREAM_SYNCED), dwant, "device"),
                              (h.preprocess_device(_native.device_frame(pool.nv12(nv, True), "nv12", rect), _native.STREAM_SYNCED), nwant, "device nv12")):
            assert np.array_equal(got[0], exp[0]) and got[1] == exp[1] and got[2] == exp[2], (tag, o)
    finally:
        h.set_orientation(0)
    # the static gen_input_batch: a handle of its own, and a given handle left as it was found
    from vnect_amd import VNectEstimator
    got = VNectEstimator.gen_input_batch(bgr, 368, est.scales, _handle=h, orientation=o)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert np.array_equal(h.preprocess(bgr)[0], base0[0])          # the handle is at orientation 0 again


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_call_with_orientation_equals_call_on_the_oriented_frame(pool, precision):
    """est(x, orientation=o[, rect]) == est(np.ascontiguousarray(oriented)[crop]) over three frames: joints, confidences -- and with them
    the filter state, which the second and third frame's joints carry"""
    H, W = SIZES[1]
    a, b = _est(precision=precision), _est(precision=precision)
    try:
        for k, o in enumerate((3, 6, 1, 7)):
            a.reset(), b.reset()
            times = _times(3, 10.0 * k)
            rect = _rects(o, H, W)[1]
            for t in range(3):
                bgr, nv = dr.pixels(H, W, 90 + 3 * k + t), nv12_ref.content(H, W, 2 * (k + t) + 1)
                pic, npic = _pic(bgr, o), _pic(nv12_ref.restate(nv), o)
                if t == 0:      # host BGR
                    got, want = a(bgr, timestamp=times[t], orientation=o, return_confidence=True), b(pic, timestamp=times[t], return_confidence=True)
                elif t == 1:    # host NV12 with a rect
                    got = a(nv, timestamp=times[t], pixel_format="nv12", rect=rect, orientation=o, return_confidence=True)
                    want = b(_crop(npic, rect), timestamp=times[t], return_confidence=True)
                else:           # a device frame with a rect
                    got = a(pool.frame(dr.PACKED4, 1, bgr), timestamp=times[t], pixel_format="rgb", rect=rect, orientation=o, return_confidence=True)
                    want = b(_crop(pic, rect), timestamp=times[t], return_confidence=True)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), (precision, o, t)
        # orientation=0 is a call without the kwarg; the estimator's own orientation is the default
        a.reset(), b.reset()
        bgr = dr.pixels(H, W, 5)
        for g, w in zip(a(bgr, timestamp=_times(1, 99.0)[0], orientation=0), b(bgr, timestamp=_times(1, 99.0)[0])):
            assert np.array_equal(g, w)
        a.reset(), b.reset()
        a.orientation = 3
        assert a.orientation == 3
        for g, w in zip(a(bgr, timestamp=_times(1, 199.0)[0]), b(_pic(bgr, 3), timestamp=_times(1, 199.0)[0])):
            assert np.array_equal(g, w)
    finally:
        a.close(), b.close()


def test_orientation_changes_between_submits_with_frames_in_flight():
    """frames already in flight keep their orientation: two submits under different codes, then both collected"""
    H, W = SIZES[0]
    a, b = _est(lanes=2), _est()
    try:
        f0, f1 = dr.pixels(H, W, 11), dr.pixels(H, W, 12)
        times = _times(2, 7.0)
        a.submit(f0, timestamp=times[0], orientation=3)
        a.submit(f1, timestamp=times[1], orientation=1)
        got = [a.collect(), a.collect()]
        want = [b(_pic(f0, 3), timestamp=times[0]), b(_pic(f1, 1), timestamp=times[1])]
        for g, w in zip(got, want):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
    finally:
        a.close(), b.close()


def test_refusals_leave_the_state_untouched(est, pool):
    from vnect_amd import _native
    h = est.handle
    H, W = SIZES[0]
    bgr, nv = dr.pixels(H, W, 3), nv12_ref.content(H, W, 4)
    try:
        h.set_orientation(1)
        for bad in (8, -1):
            with pytest.raises(_native.VnectError) as e:
                h.set_orientation(bad)
            assert e.value.code == _native.E_ARG and "0 .. 7" in str(e.value)
        h.upload_frame(0, bgr)
        assert np.array_equal(h.read_frame(0), _pic(bgr, 1))          # still code 1
        # a rect that lies inside the stored frame but outside the oriented picture (128 x 96: Wo = 96)
        before = h.read_frame(0)
        with pytest.raises(_native.VnectError) as e:
            h.upload_frame_nv12(0, nv, (100, 0, 10, 10))
        assert e.value.code == _native.E_ARG and "origin" in str(e.value)
        with pytest.raises(_native.VnectError):
            h.upload_frame_device(0, _native.device_frame(pool.frame(dr.PACKED3, 0, bgr), "bgr", (100, 0, 10, 10)), _native.STREAM_SYNCED)
        assert np.array_equal(h.read_frame(0), before)
        # an NV12 draw target under an orientation
        dev = pool.nv12(nv)
        ptr = dev.__cuda_array_interface__["data"][0]
        with pytest.raises(_native.VnectError) as e:
            h.draw_device(_native.device_frame(dev, "nv12"), np.full((21, 2), 20.0), rect=(1, 1, 20, 20), stream=_native.STREAM_SYNCED)
        assert e.value.code == _native.E_ARG and "NV12" in str(e.value) and "orientation" in str(e.value)
        assert np.array_equal(pool.get(ptr), nv.reshape(-1))
        # a tracked stream: a stored frame whose oriented size is not the track's
        Ho, Wo = orf.oriented_size(1, H, W)
        h.track_begin(0, Ho, Wo)
        wrong = pool.frame(dr.PACKED3, 0, dr.pixels(Ho, Wo, 1))          # stored (Ho, Wo): its picture is (Wo, Ho)
        with pytest.raises(_native.VnectError) as e:
            h.submit_tracked_device(0, _native.device_frame(wrong, "bgr"), T0 + 900, T0 + 900, _native.STREAM_SYNCED)
        assert e.value.code == _native.E_ARG and "size" in str(e.value)
        h.submit_tracked_device(0, _native.device_frame(pool.frame(dr.PACKED3, 0, bgr), "bgr"), T0 + 901, T0 + 901, _native.STREAM_SYNCED)
        s, j2, j3, used = h.collect_tracked()
        assert used == [0, 0, Wo, Ho]
    finally:
        h.set_orientation(0)
        est.reset()
    # a pyramid-sharded handle takes no orientation (before finalize, without weights)
    sh = _native.Handle([1.0, 0.8], pyramid=(0, 2))
    try:
        with pytest.raises(_native.VnectError) as e:
            sh.set_orientation(3)
        assert e.value.code == _native.E_ARG and "sharded" in str(e.value)
    finally:
        sh.close()
    # it works on a preprocess_only handle
    po = _native.Handle([1.0], preprocess_only=True)
    try:
        po.set_orientation(7)
        got = po.preprocess(bgr)
        po.set_orientation(0)
        want = po.preprocess(_pic(bgr, 7))
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    finally:
        po.close()


# ---- tracked ---------------------------------------------------------------------------------------------------------------------------------
TH, TW, TN = 240, 320, 12


def _video(n=TN, H=TH, W=TW, seed=0):
    """the planted-weights video of tests/test_gpu_track.py, smaller: three blobs that move while their spread changes"""
    from tests import planted
    out = []
    for k in range(n):
        cy, cx = H * (0.40 + 0.2 * np.sin(k / 4.0)), W * (0.30 + 0.40 * k / max(n - 1, 1))
        r = 14 + 22 * (0.5 + 0.5 * np.sin(k / 2.0))
        blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
        out.append(planted.scene(H, W, blobs, sigma=5.0, seed=seed + k, texture=0.15))
    return out


@pytest.fixture(scope="module")
def pest():
    e = _est(planted=True, lanes=3)
    yield e
    e.close()


def _run(gen):
    return [tuple(np.array(v) if isinstance(v, np.ndarray) else (list(v) if isinstance(v, (list, tuple)) else v) for v in r) for r in gen]


def _same(got, want, tag):
    assert len(got) == len(want) and len(got) > 0, (tag, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (tag, k)
        for a, b in zip(g, w):
            assert np.array_equal(a, b), (tag, k, a, b)


def _stored(pictures, o):
    """stored frames whose oriented pictures are `pictures`: the inverse turn of each"""
    inv = {0: 0, 1: 3, 2: 2, 3: 1, 4: 4, 5: 5, 6: 6, 7: 7}[o]
    out = [np.ascontiguousarray(orf.oriented(p, inv)) for p in pictures]
    assert all(np.array_equal(orf.oriented(s, o), p) for s, p in zip(out[:2], pictures[:2]))
    return out


@pytest.mark.parametrize("source", ["pinned", "resident", "device"])
def test_tracked_orientation_3_equals_the_hosts_transpose(pest, pool, source):
    from vnect_amd import runner
    frames, times = _video(), _times(TN, 20.0)
    pest.reset()
    want = _run(runner.track(pest, frames, transpose=True, timestamps=times))
    assert len({tuple(r[2]) for r in want}) >= 6                  # the crop moves
    pest.reset()
    src = [pool.frame(dr.PACKED3, 0, f, off=0, pad=0) for f in frames] if source == "device" else frames
    got = _run(runner.track_on_device(pest, src, orientation=3, timestamps=times, ahead=1, source=source))
    _same(got, want, ("o=3", source))
    assert pest.handle.orientation == pest.orientation == 0           # the loop left the estimator's own orientation in force


@pytest.mark.parametrize("o,ahead,lost", [(1, 0, None), (6, 2, (1e9, 21, "hold")), (7, 1, (1e9, 21, "reset")), (5, 2, None)])
def test_tracked_codes_depths_and_the_loss_rule(pest, o, ahead, lost):
    """pinned BGR under codes 1, 6, 7 (and 5), one frame at a time and two ahead, with the loss rule holding / resetting the box on every
    frame (no confidence reaches 1e9, so every frame is lost): equal to runner.track on the host-oriented frames"""
    from vnect_amd import runner
    frames, times = _video(seed=50 + o), _times(TN, 40.0 + o)
    pics = [_pic(f, o) for f in frames]
    Ho, Wo = pics[0].shape[:2]
    rect = [Wo // 8, Ho // 8, Wo // 2, Ho // 2]
    pest.reset()
    want = _run(runner.track(pest, pics, rect=rect, timestamps=times, confidence=True, lost=lost))
    pest.reset()
    host = _run(runner.track(pest, frames, rect=rect, timestamps=times, confidence=True, lost=lost, orientation=o))
    _same(host, want, ("track", o))
    pest.reset()
    got = _run(runner.track_on_device(pest, frames, rect=rect, orientation=o, timestamps=times, ahead=ahead, confidence=True, lost=lost))
    _same(got, want, ("track_on_device", o, ahead, lost))
    if lost is not None:
        assert all(r[4] == 1 for r in want)


@pytest.mark.parametrize("source", ["pinned", "resident", "device"])
def test_tracked_nv12_equals_tracking_the_converted_oriented_frames(pest, pool, source):
    from vnect_amd import pixfmt, runner
    o = 3
    nvs = [pixfmt.bgr_to_nv12(f) for f in _video(seed=200)]
    times = _times(TN, 60.0)
    pics = [_pic(nv12_ref.restate(nv), o) for nv in nvs]
    pest.reset()
    want = _run(runner.track(pest, pics, timestamps=times))
    pest.reset()
    host = _run(runner.track(pest, nvs, timestamps=times, pixel_format="nv12", orientation=o))
    _same(host, want, "track nv12")
    pest.reset()
    src = [pool.nv12(nv, two=bool(k & 1)) for k, nv in enumerate(nvs)] if source == "device" else nvs
    got = _run(runner.track_on_device(pest, src, orientation=o, timestamps=times, ahead=1, source=source, pixel_format="nv12"))
    _same(got, want, ("nv12", source))


def test_two_videos_with_different_orientations_share_a_handle(pest):
    from vnect_amd import runner
    va, vb = _video(seed=300), _video(seed=400, H=TW, W=TH)
    ta, tb = _times(TN, 80.0), _times(TN, 85.0)
    pest.reset()
    wa = _run(runner.track(pest, [_pic(f, 3) for f in va], timestamps=ta))
    pest.reset()
    wb = _run(runner.track(pest, [_pic(f, 6) for f in vb], timestamps=tb))
    pest.reset()
    got = _run(runner.track_many_on_device(pest, [va, vb], orientation=[3, 6], timestamps=[ta, tb], ahead=2, source="resident"))
    _same([g[1:] for g in got if g[0] == 0], wa, "video 0")
    _same([g[1:] for g in got if g[0] == 1], wb, "video 1")
    pest.reset()
    got = _run(runner.track_many_on_device(pest, [va, vb], orientation=[3, 6], timestamps=[ta, tb], ahead=1, source="pinned"))
    _same([g[1:] for g in got if g[0] == 0], wa, "video 0 pinned")
    _same([g[1:] for g in got if g[0] == 1], wb, "video 1 pinned")


@pytest.mark.parametrize("o,fmt", [(3, "bgr"), (5, "rgb"), (6, "bgr")])
def test_tracked_draw_annotates_the_stored_frame(pest, pool, o, fmt):
    """draw=True yields what draw=False yields, and the stored frame afterwards is render.draw_limbs_2d_exact applied to its oriented host
    copy -- a view of the stored copy, so the drawing lands turned back"""
    from vnect_amd import render, runner
    n = 4
    frames, times = _video(n, seed=500 + o), _times(n, 100.0 + o)
    order = 1 if fmt == "rgb" else 0
    pest.reset()
    plain = [pool.frame(dr.PACKED3, order, f, off=0, pad=0) for f in frames]
    want = _run(runner.track_on_device(pest, plain, orientation=o, timestamps=times, ahead=1, source="device", pixel_format=fmt))
    pest.reset()
    drawn = [pool.frame(dr.PACKED3, order, f, off=0, pad=0) for f in frames]
    got = _run(runner.track_on_device(pest, drawn, orientation=o, timestamps=times, ahead=1, source="device", pixel_format=fmt, draw=True))
    _same(got, want, ("draw", o))
    for k, arr in enumerate(drawn):
        exp = np.ascontiguousarray(dr.as_bgr(frames[k], order))                    # the stored bytes
        render.draw_limbs_2d_exact(orf.oriented(exp, o), got[k][0], pest.joint_parents, got[k][2], fmt, inplace=True)
        assert (exp != dr.as_bgr(frames[k], order)).any()
        assert np.array_equal(pool.get(arr.__cuda_array_interface__["data"][0]).reshape(exp.shape), exp), (o, k)
    # est.draw on its own
    arr = pool.frame(dr.PACKED3, 0, frames[0], off=0, pad=0)
    exp = np.array(frames[0])
    render.draw_limbs_2d_exact(orf.oriented(exp, o), got[0][0], pest.joint_parents, got[0][2], "bgr", inplace=True)
    pest.draw(arr, got[0][0], rect=got[0][2], orientation=o)
    assert np.array_equal(pool.get(arr.__cuda_array_interface__["data"][0]).reshape(exp.shape), exp)


def test_an_estimators_own_orientation_is_every_loops_default(pool):
    """VNectEstimator(orientation=3): runner.track, track_on_device and a plain call all run under code 3 without being told, an explicit
    code wins in both loops, and gen_input_batch leaves a given handle with the code it found"""
    from vnect_amd import VNectEstimator, runner
    frames, times = _video(6, seed=700), _times(6, 120.0)
    pics = [_pic(f, 3) for f in frames]
    ref, e = _est(planted=True), _est(planted=True, orientation=3)
    try:
        want = _run(runner.track(ref, pics, timestamps=times))
        want0 = _run(runner.track(ref.reset() or ref, frames, timestamps=times))
        for tag, gen in (("track", lambda: runner.track(e, frames, timestamps=times)),
                         ("track_on_device", lambda: runner.track_on_device(e, frames, timestamps=times, ahead=1)),
                         ("device", lambda: runner.track_on_device(e, [pool.frame(dr.PACKED3, 0, f, off=0, pad=0) for f in frames], timestamps=times,
                                                                  source="device"))):
            e.reset()
            _same(_run(gen()), want, tag)
            # (the device loops put the estimator's code back; after track the handle holds the last call's code 0 until the next call sets it)
            assert e.orientation == 3 and e.handle.orientation == (0 if tag == "track" else 3), tag
        for tag, gen in (("track 0", lambda: runner.track(e, frames, timestamps=times, orientation=0)),
                         ("track_on_device 0", lambda: runner.track_on_device(e, frames, timestamps=times, orientation=0))):
            e.reset()
            _same(_run(gen()), want0, tag)
            assert e.orientation == 3 and e.handle.orientation == (0 if tag == "track 0" else 3), tag
        e.reset(), ref.reset()
        for g, w in zip(e(frames[0], timestamp=times[0]), ref(pics[0], timestamp=times[0])):
            assert np.array_equal(g, w)
        h = e.handle                                                  # (holds code 3)
        under3, under0 = ref.handle.preprocess(pics[0]), ref.handle.preprocess(frames[0])
        for o, exp in ((None, under3), (0, under0), (3, under3), (6, ref.handle.preprocess(_pic(frames[0], 6)))):
            got = VNectEstimator.gen_input_batch(frames[0], 368, e.scales, _handle=h, orientation=o)
            assert np.array_equal(got[0], exp[0]) and got[1:] == exp[1:], o
            assert h.orientation == 3, o
        for g, w in zip(e(frames[1], timestamp=times[1]), ref(pics[1], timestamp=times[1])):   # the estimator still runs under its own code
            assert np.array_equal(g, w)
    finally:
        ref.close(), e.close()
