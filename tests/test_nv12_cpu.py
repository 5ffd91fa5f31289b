"""CPU: NV12 -> BGR.  g++'s build of vnect_amd/csrc/nv12.h -- the one source the copy kernels of post.hip convert with -- and
vnect_amd/pixfmt.py against the tests' own restatement of the specification (tests/nv12_ref.py), over all 2^24 (Y, U, V) triples; the
case lists of tests/test_gpu_nv12_kernels.py against what they claim to cover; the ABI's new entry points; and the sanitizer build, a
stand-alone program that is never loaded into python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import nv12_ref as nr

u8p = nr.u8p


def _p(a):
    return a.ctypes.data_as(u8p)


def _plane(Y):
    """every (U, V) with luma Y: the restatement, (256, 256, 3)"""
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return nr.restate_yuv(np.full_like(U, Y), U, V), U, V


def test_known_answers():
    L = nr.cpu_lib()
    yuv = np.array([k for k, _ in nr.KNOWN], np.uint8)
    want = np.array([v for _, v in nr.KNOWN], np.uint8)
    got = np.zeros_like(want)
    L.nv12_pixels(_p(yuv), len(yuv), _p(got))
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(nr.restate_yuv(yuv[:, 0], yuv[:, 1], yuv[:, 2]), want)


def test_every_triple_pixel_and_quad_equal_the_restatement_and_the_float_form():
    """All 2^24 triples: nv12_pixel and nv12_quad (every triple in each of the helper's four pixel positions) equal the restatement bit for
    bit, and the restatement lies within 1 of the rounded float form with OpenCV's coefficients 1.164, 2.018, 0.391, 0.813, 1.596."""
    L = nr.cpu_lib()
    one, four = np.zeros((256, 256, 3), np.uint8), np.zeros((4, 256, 256, 3), np.uint8)
    worst = 0
    for Y in range(256):
        want, U, V = _plane(Y)
        L.nv12_plane_pixel(Y, _p(one))
        assert np.array_equal(one, want), (Y, np.argwhere(one != want)[:4])
        assert L.nv12_plane_quad(Y, _p(four)) == 0, Y     # the quad's other three pixels are their own triples' conversions
        for p in range(4):
            assert np.array_equal(four[p], want), (Y, p, np.argwhere(four[p] != want)[:4])
        worst = max(worst, int(np.abs(want.astype(np.int64) - nr.float_form(np.full_like(U, Y), U, V)).max()))
    assert worst <= 1, worst


def test_pixfmt_equals_the_restatement_on_whole_images():
    from vnect_amd import pixfmt
    for H, W, seed in [(2, 2, 0), (2, 2, 1), (4, 6, 2), (4, 6, 3), (120, 160, 4), (120, 160, 5), (368, 368, 6)]:
        img = nr.content(H, W, seed)
        got = pixfmt.nv12_to_bgr(img)
        assert got.shape == (H, W, 3) and got.dtype == np.uint8
        assert np.array_equal(got, nr.restate(img)), (H, W, seed)
    with pytest.raises(ValueError):
        pixfmt.nv12_to_bgr(np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError):
        pixfmt.bgr_to_nv12(np.zeros((3, 4, 3), np.uint8))


def test_cpp_image_walk_equals_the_restatement_on_strided_crops():
    """nv12_convert (nv12_quad group by group, on the host) over every crop of the 32 x 12 case frame at its odd strides."""
    L = nr.cpu_lib()
    lay = nr.CROP_FRAME
    img = nr.content(lay.H, lay.W, 0)
    buf, want = lay.place(img), nr.restate(img)
    for x, y, w, h in nr.crop_rects()[::7]:
        out = np.zeros((h, w, 3), np.uint8)
        rc = L.nv12_convert(_p(buf[lay.y_off:]), lay.ys, _p(buf[lay.uv_off:]), lay.uvs, lay.H, lay.W, x, y, w, h, _p(out))
        assert rc == 0 and np.array_equal(out, want[y:y + h, x:x + w]), (x, y, w, h)


def test_generator_round_trip_stays_within_its_bound():
    """nv12_to_bgr(bgr_to_nv12(img)) for a smooth image: a sanity check on the generator only.  Bound: the 8-bit rounding of Y, U and V
    (half a code each) times the inverse's gains 1.164, 2.018 and 1.596 is under 2.4; chroma averaged over 2 x 2 and replicated adds the
    image's own step across a 2 x 2 block, under 2 codes per pixel for this 368-pixel interpolation of an 8 x 8 grid of colours 20..235,
    again times the chroma gains: measured here 5, bound 8."""
    from vnect_amd import pixfmt
    img = nr.smooth_bgr(368, 368, 11)
    back = pixfmt.nv12_to_bgr(pixfmt.bgr_to_nv12(img))
    err = int(np.abs(back.astype(np.int64) - img.astype(np.int64)).max())
    print("round-trip max abs error:", err)
    assert err <= 8, err


def test_gpu_case_lists_cover_what_they_claim():
    lane, wave, wg = nr.kernel_spans()
    assert lane == 4 and wave % lane == 0 and wg % wave == 0 and wg > wave
    # crops: every residue of x mod 4, y mod 2, w mod 4, h mod 2 -- in every combination
    rects = nr.crop_rects()
    assert len(rects) == 1440 and len(set(rects)) == 1440
    assert {(x % 4, y % 2, w % 4, h % 2) for x, y, w, h in rects} == {(a, b, c, d) for a in range(4) for b in range(2) for c in range(4) for d in range(2)}
    lay = nr.CROP_FRAME
    assert (lay.H, lay.W) == (12, 32) and all(x + w <= lay.W and y + h <= lay.H for x, y, w, h in rects)
    assert lay.ys % 2 == 1 and lay.y_off % 4 != 0 and not lay.behind
    assert (nr.WIDE_FRAME.H, nr.WIDE_FRAME.W) == (6, 2052) and nr.WIDE_RECTS == [(1, 1, 2049, 4), (3, 0, 1025, 5), (1021, 1, 9, 3)]
    assert any(x % 4 + w > wg for x, _, w, _ in nr.WIDE_RECTS) and any(wave < x % 4 + w <= wg + wave for x, _, w, _ in nr.WIDE_RECTS)
    assert nr.TALL_FRAME.H // 2 > 65535          # more 2-row strips than one grid holds
    # whole frames
    widths = nr.frame_widths()
    assert set(range(2, 20, 2)) | {254, 256, 258, 1022, 1024, 1026, 2050} <= set(widths) and all(w % 2 == 0 for w in widths)
    for span in (wave, wg):                      # both sides of what one wave and one workgroup cover
        assert span - 2 in widths and span in widths and span + 2 in widths
    assert max(widths) > wg + wave
    seen = set()
    for H in nr.FRAME_HEIGHTS:
        lays = nr.frame_layouts(H)
        assert len({la.key() for la in lays}) == len(lays)
        for la in lays:
            assert la.ys >= la.W and la.uvs >= la.W
            y_end, uv_end = la.y_off + (la.H - 1) * la.ys + la.W, la.uv_off + (la.H // 2 - 1) * la.uvs + la.W
            assert la.uv_off >= y_end and uv_end <= la.cap            # planes disjoint, inside the buffer
            seen.add((la.W, la.ys - la.W, la.y_off % 4, la.behind))
    assert nr.FRAME_HEIGHTS == [2, 4, 6]
    for W in widths:
        for pad in (0, 2, 13):
            for off in range(4):                 # Y base at byte offsets 0 .. 3, UV directly behind and apart
                assert (W, pad, off, True) in seen and (W, pad, off, False) in seen
    for H in nr.FRAME_HEIGHTS:                   # random and smooth content both reach both UV placements
        assert {(la.behind, nr.frame_seed(k, H) % 2) for k, la in enumerate(nr.frame_layouts(H))} == {(a, b) for a in (True, False) for b in (0, 1)}
    strides = {la.ys for H in nr.FRAME_HEIGHTS for la in nr.frame_layouts(H)}
    assert any(s % 4 == 0 for s in strides) and any(s % 4 == 2 for s in strides) and any(s % 2 == 1 for s in strides)
    uv = {(la.uvs % 4, la.uv_off % 4) for la in nr.frame_layouts(4) if not la.behind}
    assert {a for a, _ in uv} == {0, 1, 2, 3}
    assert len({b for _, b in uv}) == 4
    # content: both kinds, and random bytes do saturate
    a = nr.content(64, 64, 0)
    bgr = nr.restate(a)
    frac = float(np.mean(np.any((bgr == 0) | (bgr == 255), axis=2)))
    assert frac > 0.7, frac
    b = nr.restate(nr.content(64, 64, 1))
    assert float(np.mean(np.any((b == 0) | (b == 255), axis=2))) < 0.01


def test_abi_declares_the_nv12_entry_points():
    from vnect_amd import _native
    hdr = open(os.path.join(nr.ROOT, "include", "vnect_abi.h")).read()
    names = ["vnect_upload_frame_nv12", "vnect_upload_frame_nv12_rect", "vnect_infer_nv12", "vnect_preprocess_nv12", "vnect_submit_tracked_pinned_nv12", "vnect_read_frame"]
    L = _native.lib()
    for n in names:
        assert "int " + n + "(" in hdr and n in _native.SYMBOLS and getattr(L, n)
    assert _native.ABI_VERSION == 7 and C.sizeof(_native.Config) == 128     # additive: the version and the config stay
    pos = hdr.index("int vnect_upload_frame_nv12")
    doc = hdr[hdr.rindex("/*", 0, pos):pos]
    assert "run_estimator_ps.py:79" in doc and "camera_capture.read()" in doc and "OpenCV's, not the reference's" in doc
    # null handles come back as codes
    assert L.vnect_infer_nv12(None, None, 0, None, 0, 2, 2, None, 0.0, 0.0, None, None) == _native.E_ARG
    assert L.vnect_read_frame(None, 0, None, 0, None) == _native.E_ARG
    # the Python layer's own argument checks
    with pytest.raises(ValueError):
        _native._as_nv12(np.zeros((4, 4), np.uint8))
    y, ys, uv, uvs, H, W = _native._as_nv12(np.zeros((12, 20), np.uint8)[:, 2:10])
    assert (ys, uvs, H, W) == (20, 20, 8, 8)
    assert C.addressof(uv.contents) - C.addressof(y.contents) == 8 * 20


def test_runner_refuses_transpose_with_nv12():
    from vnect_amd import runner
    with pytest.raises(ValueError, match="transpose"):
        next(runner.track(None, [np.zeros((6, 4), np.uint8)], transpose=True, pixel_format="nv12"))
    with pytest.raises(ValueError, match="transpose"):
        next(runner.track_on_device(None, [np.zeros((6, 4), np.uint8)], transpose=True, pixel_format="nv12"))
    with pytest.raises(ValueError, match="pixel_format"):
        next(runner.track(None, [np.zeros((6, 4), np.uint8)], pixel_format="yuy2"))


def test_sanitizer_sweep_is_a_standalone_program():
    """-fsanitize=address,undefined build of nv12.h behind its own main: the all-triples sweep (pixel and quad against a 64-bit, shift-free
    statement of the formula) and every crop of strided images in exactly sized heap blocks.  Built (sanitizer runtimes linked statically)
    and run here, on the CPU, in the environment as it is; nothing of it is loaded into python."""
    subprocess.check_call(["make", "-C", nr.CSRC, "nv12_sweep_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(nr.LIBDIR, "nv12_sweep_asan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "16777216 triples" in r.stdout and " 0 mismatches" in r.stdout and "runtime error" not in r.stderr, (r.stdout, r.stderr[-2000:])
