"""CPU: the overlay (OVERLAY.md).  g++'s build of vnect_amd/csrc/overlay.h -- the set-up, the tests and the stores the kernel of
overlay.hip runs, walked tile by tile on the host -- held to tests/overlay_ref.py (an independent numpy statement of the rule) and to
render.draw_limbs_2d_exact on the WHOLE buffer of every layout, padding and fourth bytes included; the rule's known answers; the ABI's new
symbols and structure; the sanitizer build, a stand-alone program that is never loaded into python; and the Python layer's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import overlay_ref as R

LAYOUT_NAMES = [lay["name"] for lay in R.layouts(*R.SIZES[0])]
NEW = ["vnect_draw_device", "vnect_submit_tracked_device_draw"]


def _walk(buf, lay, case, **kw):
    args, keep = R.walk_args(buf, lay, case, **kw)
    return R.cpu_lib().overlay_walk(*args)


@pytest.mark.parametrize("size", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
@pytest.mark.parametrize("layout", range(len(LAYOUT_NAMES)), ids=LAYOUT_NAMES)
def test_host_walk_equals_the_rule_and_the_numpy_renderer(size, layout):
    from vnect_amd import render
    lay = R.layouts(*size)[layout]
    names = set()
    for case in R.cases(*size):
        want, got = R.fresh(lay), R.fresh(lay)
        drawn = R.draw(want, lay, case)
        assert (drawn == 0) == case["empty"], (case["name"], drawn)      # on the reference: no case passes by drawing nothing
        assert case["empty"] or (want != R.fresh(lay)).any(), case["name"]
        assert _walk(got, lay, case) == 0
        assert np.array_equal(got, want), (lay["name"], case["name"], int((got != want).sum()))
        if lay["format"] != 2:
            host = R.fresh(lay)
            out = render.draw_limbs_2d_exact(R.view(host, lay), case["joints"], case["parents"], case["rect"],
                                             pixel_format="rgb" if lay["format"] == 1 else "bgr", confidence=case["conf"],
                                             min_confidence=case["thr"], inplace=True)
            assert np.array_equal(host, want), (lay["name"], case["name"])
            assert out.shape == (lay["H"], lay["W"], 3)
        names.add(case["name"])
    assert {"horizontal", "vertical", "diagonals", "half_to_even", "L2_exact", "L2_one_ulp_below", "short_and_root", "nonfinite", "two_pow_21",
            "half_outside", "wholly_outside", "rect_flush", "rect_hanging", "rect_1x1", "rect_4x4", "band_over_limb", "nv12_odd_edges",
            "confidence", "skeleton"} <= names


def test_known_answers_of_the_rule():
    L = R.cpu_lib()
    lay = dict(name="known", format=0, H=24, W=64, data_off=0, uv_off=0, sy=192, sx=3, sc=1, uv_stride=0, size=24 * 192)
    case = R._case("known_175", [(10, 10, 10, 50)])
    limb, band = R.masks(lay, case)
    ys, xs = np.nonzero(limb)
    assert int(limb.sum()) == 175 and (ys.min(), ys.max(), xs.min(), xs.max()) == (7, 13, 10, 50) and not band.any()
    buf = np.zeros(lay["size"], np.uint8)
    assert _walk(buf, lay, case) == 0
    px = buf.reshape(24, 64, 3)
    assert int((px == np.array(R.LIMB_BGR, np.uint8)).all(axis=2).sum()) == 175 and np.array_equal(px.any(axis=2), limb)
    # the half-axis: 4 a^2 <= L2 exactly, one ulp below, and where sqrt alone would be a step off
    out = np.zeros(4)

    def setup(r1, c1, r2, c2):
        L.overlay_limb_setup(r1, c1, r2, c2, out.ctypes.data_as(R.f64p))
        return None if out[0] else (out[1], out[2], out[3])

    assert setup(10, 10, 10, 18) == (16.0, 10.0, 14.0) and setup(10, 10, 10, float(np.nextafter(18.0, 0.0)))[0] == 9.0
    assert setup(0, 0, 0, 2) == (1.0, 0.0, 1.0) and setup(0, 0, 0, float(np.nextafter(2.0, 0.0))) is None and setup(5, 5, 5, 5) is None
    # half to even: 10.5 -> 10, 11.5 -> 12, 15.5 -> 16, -0.5 -> -0
    assert setup(10, 10, 11, 21)[1:] == (10.0, 16.0) and setup(11, 3, 12, 9)[1:] == (12.0, 6.0) and setup(-3, 0, 2, 8)[1:] == (-0.0, 4.0)
    for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 21, -2.0 ** 20 - 1.0):
        assert setup(bad, 0, 5, 5) is None and setup(0, 5, 5, bad) is None
    assert setup(2.0 ** 20, 5, 5, 5) is not None
    rs = np.random.RandomState(3)
    for _ in range(2000):
        v = rs.uniform(-300, 300, 4) * rs.choice([1.0, 0.5, 0.01])
        if rs.rand() < 0.3:
            v = np.round(v * 2) / 2
        ref = R.limb_setup(*v)
        assert setup(*v) == (None if ref is None else (float(ref[3] * ref[3]), float(ref[4]), float(ref[5]))), v
    # BT.601 limited range in 8-bit integers
    yuv = np.zeros(3, np.uint8)
    for bgr in [R.LIMB_BGR, R.RECT_BGR, (0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (17, 200, 93)]:
        L.overlay_yuv(np.asarray(bgr, np.int32).ctypes.data_as(R.i32p), yuv.ctypes.data_as(R.u8p))
        assert tuple(int(v) for v in yuv) == R.yuv_of(bgr), bgr
    assert R.yuv_of((255, 255, 255)) == (235, 128, 128) and R.yuv_of((0, 0, 0)) == (16, 128, 128)


def test_colours_parents_and_refusals_of_the_walk():
    from vnect_amd import render
    H, W = 38, 54
    for lay in R.layouts(H, W):
        case = dict(R.cases(H, W)[-1], name="skeleton_coloured_%s" % lay["name"])
        want, got = R.fresh(lay), R.fresh(lay)
        assert R.draw(want, lay, case, (1, 2, 3), (250, 128, 7)) > 0
        assert _walk(got, lay, case, limb_bgr=(1, 2, 3), rect_bgr=(250, 128, 7)) == 0 and np.array_equal(got, want), lay["name"]
        if lay["format"] != 2:
            host = R.fresh(lay)
            render.draw_limbs_2d_exact(R.view(host, lay), case["joints"], case["parents"], case["rect"], "rgb" if lay["format"] == 1 else "bgr",
                                       case["conf"], case["thr"], ((1, 2, 3), (250, 128, 7)), inplace=True)
            assert np.array_equal(host, want), lay["name"]
    lay = R.layouts(H, W)[0]
    ok = R.cases(H, W)[0]
    before = R.fresh(lay)
    for bad in [dict(ok, parents=[21] + list(range(1, 21))), dict(ok, parents=[-1] + list(range(1, 21))), dict(ok, rect=(3, 3, 0, 5)), dict(ok, rect=(3, 3, 5, -1))]:
        buf = R.fresh(lay)
        assert _walk(buf, lay, bad) == -1 and np.array_equal(buf, before)
    buf = R.fresh(lay)
    assert _walk(buf, lay, ok, limb_bgr=(256, 0, 0)) == -1 and _walk(buf[:-1], lay, ok) == -1 and np.array_equal(buf, before)   # a frame one byte too long for its buffer
    # the renderer returns a copy unless told otherwise, and refuses what the device refuses
    img = np.full((H, W, 3), 90, np.uint8)
    out = render.draw_limbs_2d_exact(img, ok["joints"], ok["parents"], (2, 2, 20, 20))
    assert (img == 90).all() and (out != 90).any()
    with pytest.raises(ValueError):
        render.draw_limbs_2d_exact(img, ok["joints"], ok["parents"], (2, 2, 0, 20))
    with pytest.raises(ValueError):
        render.draw_limbs_2d_exact(img, ok["joints"], [21] * 21, None)
    with pytest.raises(ValueError):
        render.draw_limbs_2d_exact(img, ok["joints"], ok["parents"], None, pixel_format="nv12")


def test_symbols_structure_and_null_handles(tmp_path):
    from vnect_amd import _native
    hdr = open(os.path.join(R.ROOT, "include", "vnect_abi.h")).read()
    L = _native.lib()
    for n in NEW:
        assert "int " + n + "(" in hdr and n in _native.SYMBOLS and getattr(L, n)
    assert "vnect_*" in open(os.path.join(R.CSRC, "vnect.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        assert set(NEW) <= {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert _native.ABI_VERSION == 7 and L.vnect_abi_version() == 7 and C.sizeof(_native.Config) == 128   # additive: both stay
    assert "#define VNECT_ABI_VERSION 7" in hdr
    pos = hdr.index("typedef struct vnect_overlay_style")
    doc = hdr[hdr.rindex("/*", 0, pos):pos]
    assert "run_estimator_ps.py:92-94" in doc and "src/utils.py:222-243" in doc and "WRITTEN UNTIL THE FRAME HAS BEEN COLLECTED" in doc
    fields = [k for k, _ in _native.OverlayStyle._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vnect_abi.h"\nint main(void) {\n  printf("%zu", sizeof(vnect_overlay_style));\n'
                   + "".join('  printf(" %%zu", offsetof(vnect_overlay_style, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(R.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_native.OverlayStyle)] + [getattr(_native.OverlayStyle, f).offset for f in fields], got
    # the colours and parents of the header, the kernel's header, the Python layer and the reference statement are the same
    oh = open(os.path.join(R.CSRC, "overlay.h")).read()
    assert "OVERLAY_LIMB_BGR[3] = {49, 22, 122}" in oh and "OVERLAY_RECT_BGR[3] = {60, 66, 207}" in oh
    assert "{%s}" % ", ".join(str(p) for p in R.PARENTS) in oh
    from vnect_amd.estimator import VNectEstimator
    assert VNectEstimator.joint_parents == R.PARENTS and (_native.LIMB_BGR, _native.RECT_BGR) == (R.LIMB_BGR, R.RECT_BGR)
    # null handles come back as codes
    assert L.vnect_draw_device(None, None, None, None, None, None, None) == _native.E_ARG
    assert L.vnect_submit_tracked_device_draw(None, 0, None, None, 0.0, 0.0, None) == _native.E_ARG
    # the tile the kernel reports is the one the GPU tests derive their seams from
    t = np.zeros(3, np.int32)
    R.cpu_lib().overlay_tile(t.ctypes.data_as(R.i32p))
    assert t[0] == 64 and t[1] >= 4 and t[2] == 256 and (t[0] * t[1]) % t[2] == 0


def test_sanitizer_sweep_is_a_standalone_program():
    """-fsanitize=address,undefined build of the same walk behind its own main, every target in an exactly sized heap block (a store
    outside the frame is the sanitizer's finding).  Built (sanitizer runtimes linked statically) and run here, on the CPU, in the
    environment as it is; nothing of it is loaded into python."""
    subprocess.check_call(["make", "-C", R.CSRC, "overlay_sweep_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(R.LIBDIR, "overlay_sweep_asan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"overlay sweep: (\d+) walks, (\d+) bytes drawn, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) >= 500 and int(m.group(2)) > 100000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]


def test_python_layer_style_and_refusals():
    from vnect_amd import _native, runner
    from vnect_amd.estimator import VNectEstimator
    s = _native.overlay_style()
    assert s.struct_size == C.sizeof(_native.OverlayStyle) and tuple(s.limb_bgr) == R.LIMB_BGR and tuple(s.rect_bgr) == R.RECT_BGR
    assert s.min_confidence != s.min_confidence and s.has_parents == 0
    s = _native.overlay_style(0.25, ((1, 2, 3), None), R.PARENTS)
    assert s.min_confidence == 0.25 and tuple(s.limb_bgr) == (1, 2, 3) and tuple(s.rect_bgr) == R.RECT_BGR
    assert s.has_parents == 1 and list(s.parents) == R.PARENTS
    with pytest.raises(ValueError):
        _native.overlay_style(parents=[0] * 20)
    est = VNectEstimator.__new__(VNectEstimator)
    est._h, est.verbose, est._submitted = None, False, 0
    with pytest.raises(ValueError, match="device memory"):
        est.draw(np.zeros((4, 4, 3), np.uint8), np.zeros((21, 2)))
    for source in ("pinned", "resident"):
        with pytest.raises(ValueError, match="draw"):
            next(runner.track_on_device(None, [np.zeros((6, 4, 3), np.uint8)], source=source, draw=True))
    with pytest.raises(ValueError, match="draw"):
        next(runner.track_many_on_device(None, [[np.zeros((6, 4, 3), np.uint8)]], draw=_native.overlay_style()))
