"""GPU: the NV12 copy kernels of post.hip alone (nv12_copy_kernel, nv12_copy_track_kernel), bit for bit against the tests' restatement.

The product's own post.o and track.o, linked behind a test shim (`make nv12probe`: vnect_amd/csrc/nv12_probe.cpp; the product never loads
it), are driven case by case: whole frames at every width / height / stride / plane alignment of tests/nv12_ref.py, every crop of a small
frame and the seam crops of a wide one -- by the host-rect kernel and by the TrackState kernel -- and the tracked pyramid behind the copy.
Every destination is filled with a canary first, and every byte outside the packed crop rows must still be the canary afterwards.
tests/test_nv12_cpu.py asserts, without a GPU, that the case lists cover what they claim.  No case is skipped: one the shim refuses fails."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import nv12_ref as nr

pytestmark = pytest.mark.gpu

u8p, i32p, f64p = nr.u8p, nr.i32p, C.POINTER(C.c_double)
EL_F32, EL_BF16, EL_F16 = 0, 1, 2


@pytest.fixture(scope="module")
def probe():
    from vnect_amd import _native
    path = os.environ.get("VNECT_NV12PROBE_LIB") or _native.NV12PROBE_LIB
    assert os.path.exists(path), "libvnect_nv12probe.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    L = C.CDLL(path)
    L.np_copy.argtypes = [u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, i32p, i32p, C.c_int64, u8p, i32p]
    L.np_pyramid.argtypes = [u8p, C.c_int, C.c_int, i32p, f64p, C.c_int, C.c_int, C.c_void_p]
    lay = (C.c_int32 * 5)()
    L.np_layout(lay)
    L.fill, L.guard = lay[0], lay[1]
    assert tuple(lay[2:5]) == nr.kernel_spans()      # the probe and the CPU shim were built from one nv12.h
    return L


def _p(a, t=u8p):
    return a.ctypes.data_as(t)


def _run(probe, lay, img, rects, tracked, seed=0):
    """both kernels' destinations for the rects of one image at one layout: (n, guard + dst_cap + guard) bytes, and dst_cap"""
    buf = lay.place(img, seed)
    n = len(rects)
    r = np.ascontiguousarray(rects, np.int32)
    t = np.ascontiguousarray(tracked, np.int32)
    dst_cap = (max(3 * w * h for _, _, w, h in rects) + 63) // 64 * 64 + 64
    out = np.zeros((n, dst_cap + 2 * probe.guard), np.uint8)
    err = np.zeros(n, np.int32)
    rc = probe.np_copy(_p(buf), len(buf), lay.y_off, lay.ys, lay.uv_off, lay.uvs, lay.H, lay.W, n, _p(r, i32p), _p(t, i32p), dst_cap, _p(out), _p(err, i32p))
    assert rc == 0, (rc, lay.key(), err[np.nonzero(err)[0][:8]])   # a case the shim refuses is a failure, not a skip
    return out, dst_cap


def _check(probe, lay, img, rects, tracked, seed=0):
    out, dst_cap = _run(probe, lay, img, rects, tracked, seed)
    bgr = nr.restate(img)
    for i, rect in enumerate(rects):
        want = nr.expected_region(bgr, rect, dst_cap, probe.fill, probe.guard)
        if not np.array_equal(out[i], want):
            bad = np.nonzero(out[i] != want)[0]
            first = int(bad[0]) - probe.guard
            raise AssertionError(("tracked" if tracked[i] else "host rect", lay.key(), rect, "differing bytes", len(bad), "first at crop byte", first,
                                  "row", first // (3 * rect[2]), "got", out[i][bad[:6]], "want", want[bad[:6]]))


@pytest.mark.parametrize("H", nr.FRAME_HEIGHTS)
def test_whole_frames(probe, H):
    """Every width x stride x Y base offset x UV placement at this height, the whole frame by both kernels, random and smooth content in
    turn: the converted frame, and the canary everywhere else (the 3 bytes before, the bytes after, up to and past the next 16-byte
    boundary)."""
    for k, lay in enumerate(nr.frame_layouts(H)):
        seed = nr.frame_seed(k, H)
        _check(probe, lay, nr.content(lay.H, lay.W, seed), [(0, 0, lay.W, lay.H)] * 2, [0, 1], seed)


@pytest.mark.parametrize("seed", [0, 1])
def test_every_small_crop(probe, seed):
    """x 0..7, y 0..3, w 1..9, h 1..5 of the 32 x 12 frame (odd Y stride, Y base at byte 1, UV plane apart): 1 440 crops, each by both
    kernels.  Chroma is indexed by absolute frame coordinates, so odd origins take the second half of a chroma pair / row."""
    rects = nr.crop_rects()
    _check(probe, nr.CROP_FRAME, nr.content(12, 32, seed), rects + rects, [0] * len(rects) + [1] * len(rects), seed)


@pytest.mark.parametrize("seed", [0, 1])
def test_wide_crops_across_the_seams(probe, seed):
    lay = nr.WIDE_FRAME
    _check(probe, lay, nr.content(lay.H, lay.W, seed), nr.WIDE_RECTS * 2, [0] * 3 + [1] * 3, seed)


def test_more_strips_than_one_grid(probe):
    """131 080 rows: more 2-row strips than grid.y holds, so launch_nv12_copy splits the launch (host-rect kernel; a tracked frame has at
    most 65 532 rows)."""
    lay = nr.TALL_FRAME
    _check(probe, lay, nr.content(lay.H, lay.W, 0), nr.TALL_RECTS, [0] * len(nr.TALL_RECTS))


_PYR = {}


def _pyramid_case(i):
    """(nv12, rect, fp32 reference (S, 368, 368, 4)) of pyramid case i: computed once, shared, left unchanged"""
    if i not in _PYR:
        from tests import track_cases as tc
        H, W, rect = nr.PYRAMID_CASES[i]
        img = nr.content(H, W, 1)                     # a smooth picture: neighbouring pixels differ, nothing saturates
        x, y, w, h = rect
        ref = tc.pyramid_reference(nr.restate(img)[y:y + h, x:x + w], tc.BASELINE_SCALES)
        ref.setflags(write=False)
        _PYR[i] = (img, rect, ref)
    return _PYR[i]


@pytest.mark.parametrize("case,el", [(0, EL_F32), (0, EL_BF16), (0, EL_F16), (1, EL_F32)])
def test_tracked_pyramid_from_an_nv12_crop(probe, case, el):
    """launch_nv12_copy_track, then launch_pyramid_track (packed = 1) on what it left: oracle.gen_input_batch of the restated crop, in
    fp32 bit for bit and in bf16 / fp16 as its round-to-nearest-even -- from a 640 x 480 frame, and once from a 4096 x 2160 one."""
    from tests import track_cases as tc
    img, rect, ref = _pyramid_case(case)
    H, W, _ = nr.PYRAMID_CASES[case]
    S = len(tc.BASELINE_SCALES)
    out = np.zeros((S, 368, 368, 4), np.float32 if el == EL_F32 else np.uint16)
    sc = np.asarray(tc.BASELINE_SCALES, np.float64)
    r = np.asarray(rect, np.int32)
    rc = probe.np_pyramid(_p(np.ascontiguousarray(img)), H, W, _p(r, i32p), _p(sc, f64p), S, el, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    if el == EL_F32:
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), int(np.sum(out != ref))
    else:
        want = tc.to_16(ref, el == EL_F16)
        assert np.array_equal(out, want), int(np.sum(out != want))
