"""GPU: the device-frame copy kernels of post.hip alone (ingest_copy_kernel, its tracked twin and the generic pair, and the NV12 copies on
planes in two device allocations), byte for byte against the plain gather of tests/devframe_ref.py.

The product's own post.o and track.o, linked behind a test shim (`make ingestprobe`: vnect_amd/csrc/ingest_probe.hip; the product never
loads it), are driven case by case.  Every frame lies in a device allocation of exactly its own size, and the kernels get that
allocation's true address range as their load bounds; every destination is filled with a canary first, and every byte outside the packed
crop rows must still be the canary afterwards.  tests/test_device_frames_cpu.py asserts, without a GPU, that the case lists cover what
they claim.  No case is skipped: one the shim refuses fails."""
import ctypes as C

import numpy as np
import pytest

from tests import devframe_ref as dr

pytestmark = pytest.mark.gpu

u8p, i32p, f64p = dr.u8p, dr.i32p, C.POINTER(C.c_double)
EL_F32 = 0
FORM_ORDER = [(f, o) for f in dr.FORMS for o in dr.ORDERS]
FORM_ORDER_IDS = ["%s-%s" % (dr.FORM_NAMES[f], "rgb" if o else "bgr") for f, o in FORM_ORDER]


@pytest.fixture(scope="module")
def probe():
    return dr.load_probe()


def _p(a, t=u8p):
    return a.ctypes.data_as(t)


def _check(probe, lay, src, order, rects, modes, phase=0, flush_end=0, seed=0):
    """the rects of one frame at one layout, by the kernels `modes` name (bit 0 tracked, bit 1 generic): every destination region whole"""
    buf = lay.place(src, seed)
    n = len(rects)
    r = np.ascontiguousarray(rects, np.int32)
    m = np.ascontiguousarray(modes, np.int32)
    dst_cap = (max(3 * w * h for _, _, w, h in rects) + phase + 63) // 64 * 64 + 64   # at least 64 bytes longer than the crop
    out = np.zeros((n, dst_cap + 2 * probe.guard), np.uint8)
    err = np.zeros(n, np.int32)
    rc = probe.ip_copy(_p(buf), len(buf), flush_end, lay.off, lay.H, lay.W, lay.sy, lay.sx, lay.sc, order, n, _p(r, i32p), _p(m, i32p), phase, dst_cap,
                       _p(out), _p(err, i32p))
    assert rc == 0, (rc, lay.key(), err[np.nonzero(err)[0][:8]])   # a case the shim refuses is a failure, not a skip
    bgr = dr.as_bgr(src, order)
    for i, rect in enumerate(rects):
        want = dr.expected_region(bgr, rect, dst_cap, probe.fill, probe.guard, phase)
        if not np.array_equal(out[i], want):
            bad = np.nonzero(out[i] != want)[0]
            first = int(bad[0]) - probe.guard - phase
            raise AssertionError(("mode", int(modes[i]), lay.key(), "order", order, rect, "phase", phase, "flush_end", flush_end, "differing bytes", len(bad),
                                  "first at crop byte", first, "row", first // (3 * rect[2]), "got", out[i][bad[:6]], "want", want[bad[:6]]))


def _modes(form):
    """the form's own kernel with the rect as arguments and from a TrackState, and the generic kernel on the same strides"""
    return [0, 1] if form == dr.GENERIC else [0, 1, 2, 3]


@pytest.mark.parametrize("form,order", FORM_ORDER, ids=FORM_ORDER_IDS)
def test_small_frames(probe, form, order):
    """H 1, 2, 3, 5 x the widths around every span x source offset 0..3 x row pitch tight, +1, +5, whole frames: the gathered frame, and
    the canary everywhere else.  The destination's phase moves with the case."""
    for k, lay in enumerate(dr.small_layouts(form)):
        modes = _modes(form)
        _check(probe, lay, dr.pixels(lay.H, lay.W, k), order, [(0, 0, lay.W, lay.H)] * len(modes), modes, phase=k % 4, seed=k)


@pytest.mark.parametrize("form,order", FORM_ORDER, ids=FORM_ORDER_IDS)
def test_crops(probe, form, order):
    """every crop origin residue mod 4 in x with widths 1..12 of the 40 x 6 frame (base at byte 1, pitch + 5), by every kernel"""
    lay = dr.crop_frame(form)
    rects = dr.crop_rects()
    for phase, mode in enumerate(_modes(form)):
        _check(probe, lay, dr.pixels(lay.H, lay.W, 7), order, rects, [mode] * len(rects), phase=phase)


@pytest.mark.parametrize("form,order", FORM_ORDER, ids=FORM_ORDER_IDS)
def test_allocation_edges(probe, form, order):
    """A frame whose first byte is its allocation's first, and frames whose last byte is its last with that end on every dword phase: the
    kernels get the allocation's true range and must read the frame correctly from inside it."""
    for k, (lay, flush_end) in enumerate(dr.edge_layouts(form)):
        modes = _modes(form)
        _check(probe, lay, dr.pixels(lay.H, lay.W, 100 + k), order, [(0, 0, lay.W, lay.H)] * len(modes), modes, phase=k % 4, flush_end=flush_end, seed=k)


@pytest.mark.parametrize("form", dr.FORMS, ids=dr.FORM_NAMES)
def test_more_rows_than_one_grid(probe, form):
    """1- and 2-pixel-wide frames of 65 531 .. 65 540 rows: across the 16-bit grid.y, where launch_ingest_copy splits the launch (the tracked
    kernel too while the frame fits its one launch)."""
    for W in dr.SEAM_WIDTHS:
        for H in dr.SEAM_HEIGHTS:
            lay = dr.Layout(form, H, W, off=H % 4, pad=W % 2)
            modes = [0, 1] if H <= dr.TRACK_MAX_ROWS else [0]
            _check(probe, lay, dr.pixels(H, W, H + W), (H + form) % 2, [(0, 0, W, H)] * len(modes), modes, phase=(H + W) % 4)


@pytest.mark.parametrize("seed", [0, 1])
def test_nv12_planes_in_two_allocations(probe, seed):
    """The small-crop list of tests/nv12_ref.py on a 32 x 12 NV12 frame whose planes lie in two exactly sized device allocations with odd
    pitches, each with its own load bounds (the Y plane flush against its allocation's end): pixfmt.nv12_to_bgr of the same bytes."""
    from tests import nv12_ref as nr
    from vnect_amd import pixfmt
    H, W, y_off, ys, uv_off, uvs = 12, 32, 2, 32 + 13, 3, 32 + 7
    img = nr.content(H, W, seed)
    rng = np.random.default_rng(50 + seed)
    ybuf = rng.integers(0, 256, y_off + (H - 1) * ys + W, dtype=np.uint8)
    uvbuf = rng.integers(0, 256, uv_off + (H // 2 - 1) * uvs + W, dtype=np.uint8)
    for r in range(H):
        ybuf[y_off + r * ys:y_off + r * ys + W] = img[r]
    for r in range(H // 2):
        uvbuf[uv_off + r * uvs:uv_off + r * uvs + W] = img[H + r]
    assert len(ybuf) % 4 and ys % 2 and uvs % 2
    bgr = pixfmt.nv12_to_bgr(img)
    assert np.array_equal(bgr, nr.restate(img))
    rects = nr.crop_rects()
    n = 2 * len(rects)
    r = np.ascontiguousarray(rects + rects, np.int32)
    m = np.ascontiguousarray([0] * len(rects) + [1] * len(rects), np.int32)
    dst_cap = (max(3 * w * h for _, _, w, h in rects) + 63) // 64 * 64 + 64
    out = np.zeros((n, dst_cap + 2 * probe.guard), np.uint8)
    err = np.zeros(n, np.int32)
    rc = probe.ip_copy_nv12(_p(ybuf), len(ybuf), y_off, ys, _p(uvbuf), len(uvbuf), uv_off, uvs, H, W, n, _p(r, i32p), _p(m, i32p), dst_cap, _p(out), _p(err, i32p))
    assert rc == 0, (rc, err[np.nonzero(err)[0][:8]])
    for i in range(n):
        want = dr.expected_region(bgr, tuple(r[i]), dst_cap, probe.fill, probe.guard)
        assert np.array_equal(out[i], want), ("tracked" if m[i] else "host rect", tuple(r[i]), np.nonzero(out[i] != want)[0][:6] - probe.guard)


_PYR = {}


def _pyramid_reference():
    """(source pixels, rect, fp32 reference (S, 368, 368, 4)): computed once, shared, left unchanged"""
    if not _PYR:
        from tests import nv12_ref as nr
        from tests import track_cases as tc
        H, W, rect = dr.PYRAMID_CASE
        bgr = nr.smooth_bgr(H, W, 3)
        x, y, w, h = rect
        ref = tc.pyramid_reference(bgr[y:y + h, x:x + w], tc.BASELINE_SCALES)
        ref.setflags(write=False)
        bgr.setflags(write=False)
        _PYR["case"] = (bgr, rect, ref)
    return _PYR["case"]


@pytest.mark.parametrize("form,order", [(dr.PLANAR, dr.RGB), (dr.PACKED4, dr.BGR)], ids=["planar-rgb", "packed4-bgr"])
def test_tracked_pyramid_from_a_device_frame(probe, form, order):
    """launch_ingest_copy_track, then launch_pyramid_track (packed = 1) on what it left: oracle.gen_input_batch of the crop, bit for bit."""
    from tests import track_cases as tc
    bgr, rect, ref = _pyramid_reference()
    H, W, _ = dr.PYRAMID_CASE
    lay = dr.Layout(form, H, W, 0, 0)
    buf = lay.place(dr.as_bgr(bgr, order))              # (the source's pixels are the picture in the source's channel order)
    S = len(tc.BASELINE_SCALES)
    out = np.zeros((S, 368, 368, 4), np.float32)
    sc = np.asarray(tc.BASELINE_SCALES, np.float64)
    r = np.asarray(rect, np.int32)
    rc = probe.ip_pyramid(_p(buf), len(buf), H, W, lay.sy, lay.sx, lay.sc, order, _p(r, i32p), _p(sc, f64p), S, EL_F32, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), int(np.sum(out != ref))
