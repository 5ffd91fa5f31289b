"""GPU: NV12 frames through the C ABI (vnect_upload_frame_nv12, vnect_infer_nv12, vnect_preprocess_nv12,
vnect_submit_tracked_pinned_nv12, vnect_read_frame) and the Python layers above it.

The conversion happens on the device, inside the frame's copy; everything behind the resident slot is unchanged.  So every result must be
BIT-identical to the BGR entry point given the converted frame -- converted here by the tests' own restatement (tests/nv12_ref.py) -- on a
second estimator with the same weights and timestamps."""
import ctypes as C

import numpy as np
import pytest

from tests import nv12_ref as nr

pytestmark = pytest.mark.gpu

T0 = 1.7e9
RECT = (13, 7, 101, 95)
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


@pytest.fixture(scope="module")
def est():
    e = _est()
    yield e
    e.close()


@pytest.mark.parametrize("H,W", [(368, 368), (120, 160), (1080, 1920)])
def test_upload_then_read_frame_is_the_converted_frame(est, H, W):
    h = est.handle
    for seed, pinned in ((0, False), (1, True)):
        img = nr.content(H, W, seed)
        src = img
        if pinned:
            src = h.frame_buffer_nv12(0, H, W)
            src[...] = img
        h.upload_frame_nv12(1, src)
        got = h.read_frame(1)
        assert got.shape == (H, W, 3) and np.array_equal(got, nr.restate(img)), (H, W, seed, int(np.sum(got != nr.restate(img))))
    # a row-strided view: the UV plane starts at row H of the view
    wide = np.random.default_rng(5).integers(0, 256, (H * 3 // 2, W + 14), dtype=np.uint8)
    view = wide[:, 6:6 + W]
    h.upload_frame_nv12(2, view)
    assert np.array_equal(h.read_frame(2), nr.restate(np.ascontiguousarray(view)))
    # ... and the slot serves the BGR entry points unchanged: the same joints as the converted frame uploaded as BGR
    est.reset()
    a = h.infer_resident(2, *_times(1)[0])
    est.reset()
    h.upload_frame(3, nr.restate(np.ascontiguousarray(view)))
    b = h.infer_resident(3, *_times(1)[0])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    est.reset()


@pytest.mark.parametrize("rect", [None, RECT, (1, 3, 159, 117)])
def test_preprocess_equals_preprocess_of_the_converted_crop(est, rect):
    from vnect_amd import _native
    img = nr.content(120, 160, 7)
    bgr = nr.restate(img)
    crop = bgr if rect is None else bgr[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
    pre = _native.Handle(est.scales, preprocess_only=True)
    try:
        for h in (est.handle, pre):
            want = h.preprocess(np.ascontiguousarray(crop))
            got = h.preprocess_nv12(img, rect)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), rect
            assert got[1] == want[1] and got[2] == want[2], (rect, got[1:], want[1:])
        # the single slot of a preprocess_only handle grows on demand, as for BGR
        big = nr.content(720, 1280, 8)
        got, want = pre.preprocess_nv12(big), pre.preprocess(nr.restate(big))
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and got[1:] == want[1:]
    finally:
        pre.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("use_graph", [False, "auto"])
def test_infer_equals_infer_of_the_converted_crop(precision, use_graph):
    """est(nv12, pixel_format="nv12", rect=r) == est(restated[crop]) on a second estimator, bit for bit, over three frames so that the
    filters advance; a pinned source (read in place) and a pageable one (staged); r None and (13, 7, 101, 95)."""
    H, W = 120, 160
    frames = [nr.content(H, W, 20 + k) for k in range(3)]
    a, b = _est(precision=precision, use_graph=use_graph), _est(precision=precision, use_graph=use_graph)
    try:
        run = 0
        for pinned in (True, False):
            for rect in (None, RECT):
                a.reset(), b.reset()
                for k, (img, t) in enumerate(zip(frames, _times(3, 10.0 * run))):
                    src = img
                    if pinned:
                        src = a.frame_buffer(H, W, index=k % 2, pixel_format="nv12")
                        src[...] = img
                    got = a(src, timestamp=t, pixel_format="nv12", rect=rect)
                    bgr = nr.restate(img)
                    crop = bgr if rect is None else bgr[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
                    want = b(np.ascontiguousarray(crop), timestamp=t)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (precision, use_graph, pinned, rect, k)
                run += 1
        # the pipelined form: a whole frame, an odd rect and one past the far edges, through the upload + submit_resident
        a.reset(), b.reset()
        rects = (None, RECT, (61, 33, 500, 500))
        for k, (img, t) in enumerate(zip(frames, _times(3, 100.0))):
            a.submit(img, timestamp=t, pixel_format="nv12", rect=rects[k])
            bgr = nr.restate(img)
            b.submit(bgr if k == 0 else np.ascontiguousarray(bgr[rects[k][1]:rects[k][1] + rects[k][3], rects[k][0]:rects[k][0] + rects[k][2]]), timestamp=t)
            for _ in range(1 if k == 1 else 2 if k == 2 else 0):     # (one lane holds two frames in flight)
                got, want = a.collect(), b.collect()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("submit", k)
    finally:
        a.close(), b.close()


# ---- tracking ------------------------------------------------------------------------------------------------------------------------------
def _planted_video(n=6, H=120, W=160, seed=0):
    """n NV12 frames of a planted-weights video (tests/planted.py: joint j sits on the blob of colour j % 3, the blobs move and spread),
    and the restated BGR frames the reference loop sees."""
    key = ("video", n, H, W, seed)
    if key not in _CACHE:
        from tests import planted
        from vnect_amd import pixfmt
        nv = []
        for k in range(n):
            cy, cx = H * (0.45 + 0.1 * np.sin(k / 2.0)), W * (0.40 + 0.04 * k)
            r = 9 + 6 * (0.5 + 0.5 * np.sin(k / 1.5))
            blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
            nv.append(pixfmt.bgr_to_nv12(planted.scene(H, W, blobs, sigma=3.0, seed=seed + k, texture=0.15)))
        _CACHE[key] = (nv, [nr.restate(f) for f in nv])
    return _CACHE[key]


def _host_track(frames_bgr, times, rect, **kw):
    key = ("host", id(frames_bgr), tuple(times), tuple(rect), tuple(sorted(kw.items())))
    if key not in _CACHE:
        from vnect_amd import runner
        e = _est(planted=True, **kw)
        try:
            _CACHE[key] = [(j2, j3, list(u)) for j2, j3, u in runner.track(e, frames_bgr, rect=list(rect), timestamps=times)]
        finally:
            e.close()
    return _CACHE[key]


def _same(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, ((g2, g3, gr), (w2, w3, wr)) in enumerate(zip(got, want)):
        assert list(gr) == list(wr), (tag, k, gr, wr)
        assert np.array_equal(g2, w2) and np.array_equal(g3, w3), (tag, k, float(np.abs(g2 - w2).max()), float(np.abs(g3 - w3).max()))


@pytest.mark.parametrize("lanes", [1, 3])
def test_tracking_on_the_device_from_nv12_equals_the_host_loop_on_the_converted_frames(lanes):
    from vnect_amd import runner
    nv, bgr = _planted_video()
    times = _times(6)
    want = _host_track(bgr, times, RECT)
    assert len({tuple(u) for _, _, u in want}) > 2          # the box does move: the crops differ from frame to frame
    e = _est(planted=True, lanes=lanes)
    try:
        for source in ("pinned", "resident"):
            for ahead in (0, 1):
                e.reset()
                got = [(j2, j3, list(u)) for j2, j3, u in runner.track_on_device(e, nv, rect=list(RECT), timestamps=times, ahead=ahead, source=source,
                                                                                  pixel_format="nv12")]
                _same(got, want, (lanes, source, ahead))
        # the host loop in NV12 (rect= instead of a slice) gives the same
        e.reset()
        got = [(j2, j3, list(u)) for j2, j3, u in runner.track(e, nv, rect=list(RECT), timestamps=times, pixel_format="nv12")]
        _same(got, want, (lanes, "host loop"))
    finally:
        e.close()


def test_nv12_tracked_bgr_tracked_and_untracked_streams_interleave_on_one_handle():
    nv, bgr = _planted_video()
    nv2, bgr2 = _planted_video(seed=40)
    H, W, n = 120, 160, 6
    ta, tb, tc_ = _times(n), _times(n, 50.0), _times(n, 90.0)
    want_a = _host_track(bgr, ta, RECT)
    want_b = _host_track(bgr2, tb, (20, 10, 120, 100))
    plain = [nr.restate(nr.content(H, W, 61 + 2 * k)) for k in range(n)]
    ref = _est(planted=True)
    try:
        want_c = [ref(f, timestamp=t) for f, t in zip(plain, tc_)]
    finally:
        ref.close()
    e = _est(planted=True, lanes=3)
    try:
        h = e.handle
        buf_a, buf_b = h.frame_buffer_nv12(0, H, W), h.frame_buffer(1, H, W)
        h.track_begin(0, H, W, RECT)
        h.track_begin(1, H, W, (20, 10, 120, 100))
        got = {0: [], 1: [], 2: []}
        for k in range(n):
            buf_a[...] = nv[k]
            buf_b[...] = bgr2[k]
            h.upload_frame(2, plain[k])
            h.submit_tracked_pinned_nv12(0, 0, W, H * W, W, *ta[k])
            h.submit_tracked_pinned(1, 1, 3 * W, *tb[k])
            h.submit_stream(2, 2, *tc_[k])
            for _ in range(3):
                s, j2, j3, used = h.collect_tracked()
                got[s].append((j2, j3, used))
        _same(got[0], want_a, "nv12 tracked")
        _same(got[1], want_b, "bgr tracked")
        for k in range(n):
            assert got[2][k][2] == [-1] * 4
            assert np.array_equal(got[2][k][0], want_c[k][0]) and np.array_equal(got[2][k][1], want_c[k][1]), ("untracked", k)
    finally:
        e.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def _raw_infer(h, y, ys, uv, uvs, H, W, rect, t):
    from vnect_amd import _native
    L = _native.lib()
    u8p, i32p, f64p, f32p = (C.POINTER(c) for c in (C.c_uint8, C.c_int32, C.c_double, C.c_float))
    j2, j3 = np.zeros((21, 2), np.float64), np.zeros((21, 3), np.float32)
    r = None if rect is None else np.asarray(rect, np.int32)
    rc = L.vnect_infer_nv12(h._h, C.cast(C.c_void_p(y), u8p), ys, C.cast(C.c_void_p(uv), u8p), uvs, H, W, None if r is None else r.ctypes.data_as(i32p),
                            t[0], t[1], j2.ctypes.data_as(f64p), j3.ctypes.data_as(f32p))
    return rc, L.vnect_last_error(h._h).decode(), j2, j3


def test_every_refusal_by_code_and_message_and_the_handle_goes_on():
    """Each refusal: VNECT_E_ARG and its message; nothing is committed -- the valid frame served right after it, with the next timestamp
    of the sequence, gives what a fresh handle fed only the valid frames gives."""
    from tests.gpu_common import _handle
    from vnect_amd import _native
    H, W = 120, 160
    cap = H * W * 3
    mk = lambda: _handle([1.0, 0.8, 0.6], _weights(), max_frame_bytes=cap)  # noqa: E731
    a, b = mk(), mk()
    try:
        img = nr.content(H, W, 31)
        pin = a.frame_buffer_nv12(0, H, W)
        pin[...] = img
        base = pin.ctypes.data
        page = np.ascontiguousarray(img)
        pb = page.ctypes.data
        bigger = nr.content(H, W + 2, 33)
        cases = [
            ("odd W", (pb, W, pb + H * W, W, H, W - 1, None), "even W and H"),
            ("odd H", (pb, W, pb + H * W, W, H - 1, W, None), "even W and H"),
            ("y stride below W", (pb, W - 2, pb + H * W, W, H, W, None), "at least W"),
            ("uv stride below W", (pb, W, pb + H * W, W - 2, H, W, None), "at least W"),
            ("UV overlaps Y", (pb, W, pb + (H - 1) * W, W, H, W, None), "overlaps the Y plane"),
            ("UV overlaps Y (pinned)", (base, W, base + W, W, H, W, None), "overlaps the Y plane"),
            ("past the pinned buffer", (base, W, base + (1 << 20) - W, W, H, W, None), "run past the pinned buffer"),
            ("rect origin right of the frame", (pb, W, pb + H * W, W, H, W, (W, 0, 4, 4)), "origin must lie inside"),
            ("rect origin below the frame", (pb, W, pb + H * W, W, H, W, (0, H, 4, 4)), "origin must lie inside"),
            ("rect origin negative", (pb, W, pb + H * W, W, H, W, (-1, 0, 4, 4)), "origin must lie inside"),
            ("more BGR bytes than max_frame_bytes", (bigger.ctypes.data, W + 2, bigger.ctypes.data + H * (W + 2), W + 2, H, W + 2, None), "max_frame_bytes"),
        ]
        times = _times(len(cases) + 1)
        for k, (what, args, text) in enumerate(cases):
            rc, msg, _, _ = _raw_infer(a, *args, times[k])
            assert rc == _native.E_ARG and text in msg and msg.startswith("vnect_infer_nv12: "), (what, rc, msg)
            got = a.infer_nv12(pin if k % 2 else page, *times[k], rect=RECT if k % 3 == 0 else None)
            want = b.infer_nv12(page, *times[k], rect=RECT if k % 3 == 0 else None)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
        # the same checks in front of the upload, the pre-processing and the tracked submit, by their own names
        with pytest.raises(_native.VnectError, match="vnect_upload_frame_nv12: .*even W and H") as ei:
            a.upload_frame_nv12(1, np.zeros((6, 5), np.uint8))
        assert ei.value.code == _native.E_ARG
        with pytest.raises(_native.VnectError, match="vnect_upload_frame_nv12_rect: .*origin must lie inside"):
            a.upload_frame_nv12(1, page, rect=(0, H, 2, 2))
        with pytest.raises(_native.VnectError, match="vnect_preprocess_nv12: .*origin must lie inside"):
            a.preprocess_nv12(page, rect=(W, 0, 2, 2))
        a.track_begin(0, H, W, RECT)
        for args, text in (((0, 0, W - 2, H * W, W), "at least W"), ((0, 0, W, H * W - 1, W), "overlaps the Y plane"),
                           ((0, 0, W, (1 << 20) - W, W), "run past the pinned buffer"), ((0, 1, W, H * W, W), "no such pinned buffer")):
            with pytest.raises(_native.VnectError, match="vnect_submit_tracked_pinned_nv12: .*" + text) as ei:
                a.submit_tracked_pinned_nv12(*args, *times[-1])
            assert ei.value.code == _native.E_ARG
        a.track_begin(0, H - 1, W, None)
        with pytest.raises(_native.VnectError, match="even W and H"):
            a.submit_tracked_pinned_nv12(0, 0, W, H * W, W, *times[-1])
        got, want = a.infer_nv12(page, *times[-1]), b.infer_nv12(page, *times[-1])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        a.close(), b.close()
