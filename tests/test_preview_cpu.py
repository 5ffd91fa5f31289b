"""CPU: the preview's rule (PREVIEW.md).  Three independent statements agree byte for byte on the whole output buffer of every case: the
composition of existing pins (tests/preview_ref.py: oracle.resize of render.draw_limbs_2d_exact of the oriented / converted picture),
render.preview_exact (numpy) and g++'s walk of the kernel's tiles over vnect_amd/csrc/preview.h (libvnect_preview.so).  Known answers
derived by hand, the walk's refusals, the sanitizer sweep as a stand-alone program, and non-vacuity as a condition."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import orient_ref
from tests import overlay_ref as R
from tests import preview_ref as P
from vnect_amd import _native, render


def _exact_backend(src, lay, o, case, f, fmt, out, out_off, pitch):
    """render.preview_exact over the picture, laid into the output buffer as the device lays it"""
    got = render.preview_exact(P.picture(src, lay, o), case["joints"], case["parents"], case.get("rect"), factor=f,
                               out_format="rgb" if fmt else "bgr", confidence=case.get("conf"), min_confidence=case.get("thr"))
    dh, dw = got.shape[:2]
    np.lib.stride_tricks.as_strided(out[out_off:], (dh, 3 * dw), (pitch, 1))[:] = got.reshape(dh, 3 * dw)
    return src


@pytest.mark.parametrize("size", P.SIZES, ids=["%dx%d" % s for s in P.SIZES])
@pytest.mark.parametrize("layout", range(len(P.LAYOUT_NAMES)), ids=P.LAYOUT_NAMES)
def test_composition_numpy_and_host_walk_agree(size, layout):
    shares = P.run_jobs(size, layout, P.cpu_backend)
    P.run_jobs(size, layout, _exact_backend)
    assert shares                                                   # every group has its skeleton jobs, and none of them is vacuous
    for key, share in shares:
        assert 0.05 <= share <= 0.95, (key, share)


def test_footprints_defaults_thin_outputs_and_tile_straddles():
    P.run_special(P.cpu_backend)
    P.run_special(_exact_backend)


@pytest.mark.parametrize("form", ["packed3_padded", "planar", "transposed", "nv12_pitched_odd_base", "nv12_two_planes"])
def test_every_orientation_of_every_source_form(form):
    """all eight codes; on a non-square picture codes 1 .. 7 differ from code 0"""
    size = P.SIZES[0]
    lay = [l for l in P.layouts(*size) if l["name"] == form][0]
    src = P.fresh(lay)
    outs = []
    for o in range(8):
        Hp, Wp = orient_ref.oriented_size(o, lay["H"], lay["W"])
        case = P.skeleton(Hp, Wp)
        for f in (0.5, 1.7):
            exp = P.expected(src, lay, o, case, f)
            out, pitch = P.out_buffer(exp.shape[0], exp.shape[1], o % 4, 3)
            P.cpu_backend(src, lay, o, case, f, 0, out, o % 4, pitch)
            assert np.array_equal(out, P.whole(exp, o % 4, pitch)), (form, o, f)
            if f == 0.5:
                outs.append(exp)
    for o in range(1, 8):
        assert outs[o].shape != outs[0].shape or not np.array_equal(outs[o], outs[0]), o


def test_resize_u8_exact_equals_the_oracle():
    rng = np.random.default_rng(5)
    n = 0
    for H in range(1, 41):
        for W in (1, 2, 3, 5, 8, 13, 21, 34, 40, H):
            img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            for f in (0.5, 0.37, 1.0 / 3.0, 1.0, 1.7, 0.09, 2.0, 3.3, 14.6):
                if P.shape_of(H, W, f) is None:
                    with pytest.raises(ValueError):
                        render.resize_u8_exact(img, f)
                    continue
                got, want = render.resize_u8_exact(img, f), oracle.resize(img, f)
                assert got.shape == want.shape and np.array_equal(got, want), (H, W, f)
                n += 1
    assert n > 2000
    g = rng.integers(0, 256, (9, 7), dtype=np.uint8)                # a 2-D array too
    assert np.array_equal(render.resize_u8_exact(g, 1.7), oracle.resize(g, 1.7))


def test_known_answers():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (12, 18, 3), dtype=np.uint8)
    a = img.astype(np.int64)
    half = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2      # the 2 x 2 area mean cv2 takes at exactly half size
    assert np.array_equal(render.resize_u8_exact(img, 0.5), half.astype(np.uint8))
    assert np.array_equal(render.preview_exact(img, None, R.PARENTS, None, factor=0.5), half.astype(np.uint8))
    # a uniform frame of value v, a rect (x, y, w, h) = (7, 6, 20, 12): the band is columns 5 .. 28, rows 4 .. 19 without columns 9 .. 24, rows 8 .. 15
    v, col = 90, np.array(R.RECT_BGR)
    frame = np.full((24, 34, 3), v, np.uint8)
    out = render.preview_exact(frame, None, R.PARENTS, (7, 6, 20, 12), factor=0.5)
    assert out.shape == (12, 17, 3)
    assert (out[2, 3] == col).all()          # taps rows 4, 5 x columns 6, 7: all four in the band
    assert (out[0, 0] == v).all()            # taps rows 0, 1 x columns 0, 1: none
    assert (out[5, 5] == v).all()            # taps rows 10, 11 x columns 10, 11: inside the exclusion
    assert (out[5, 2] == (2 * col + 2 * v + 2) >> 2).all()      # taps rows 10, 11 x columns 4, 5: column 5 is in the band, column 4 is not
    assert (out[1, 8] == v).all() and (out[2, 8] == col).all()  # rows 2, 3: above the band; rows 4, 5: in it
    lay = P.plain_layout(24, 34)
    case = dict(R._case("k", rect=(7, 6, 20, 12)), joints=None)
    buf, pitch = P.out_buffer(12, 17, 0, 0)
    P.cpu_backend(frame.reshape(-1).copy(), lay, 0, case, 0.5, 0, buf, 0, pitch)
    assert np.array_equal(buf.reshape(12, 17, 3), out)


def test_sizes_and_the_walks_refusals():
    L = P.cpu_lib()
    hw = np.zeros(2, np.int32)
    for o, H, W, f in ((0, 50, 70, 0.0), (3, 50, 70, 0.0), (0, 1080, 1920, 0.0), (1, 131, 150, 0.37), (0, 5, 5, 0.5), (0, 3, 7, 1.5)):
        assert L.preview_size(o, H, W, f, hw.ctypes.data_as(P.i32p)) == 0
        Hp, Wp = orient_ref.oriented_size(o, H, W)
        assert tuple(hw) == P.shape_of(Hp, Wp, f), (o, H, W, f)
    assert tuple(hw) == (4, 10)              # 4.5 -> 4 and 10.5 -> 10: half to even
    for f in (-0.5, float("nan"), float("inf"), 0.009, 100.0):       # 70 x 50 at 0.009 is (1, 0); at 100 a side exceeds 4096
        assert L.preview_size(0, 50, 70, f, hw.ctypes.data_as(P.i32p)) != 0, f
    lay, case = P.plain_layout(50, 70), P.skeleton(50, 70)
    src = P.fresh(lay)

    def refused(lay=lay, case=case, f=0.5, fmt=0, pad=0, o=0, short=0, has_rect=0, out=None, **kw):
        buf, pitch = P.out_buffer(25, 35, 0, 0)
        buf = buf[:len(buf) - short] if out is None else out
        before = buf.copy()
        args, keep = P.walk_args(src, lay, o, case, f, fmt, buf, 0, pitch + pad, has_rect, **kw)
        rc = L.preview_walk(*args)
        assert rc == 0 or np.array_equal(buf, before)                # a refusal writes nothing
        return rc != 0

    assert not refused()
    for f in (-1.0, float("nan"), float("inf"), 0.009, 100.0):
        assert refused(f=f), f
    assert refused(has_rect=1)                                       # a source with a rect
    assert refused(pad=-1)                                           # a pitch below 3 dw
    assert refused(short=1)                                          # the last row's last byte outside the output
    assert refused(fmt=2) and refused(o=8)
    assert refused(lay=dict(lay, sy=0)) and refused(lay=dict(lay, H=51)) and refused(lay=dict(lay, format=2, H=51))
    assert refused(case=dict(case, parents=[21] * 21)) and refused(case=dict(case, rect=(1, 1, 0, 5)))
    assert refused(limb_bgr=(0, 256, 0)) and refused(rect_bgr=(-1, 0, 0))
    assert refused(out=src[100:])                                    # an output that overlaps the source


def test_sanitizer_sweep_is_a_standalone_program():
    """preview_capi.cpp with its own main under -fsanitize=address,undefined (runtimes linked statically; never loaded into python): sources
    and outputs in exactly sized heap blocks, every walk held to a per-pixel statement of the rule"""
    subprocess.check_call(["make", "-C", R.CSRC, "preview_sweep_asan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(R.LIBDIR, "preview_sweep_asan")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"preview sweep: (\d+) walks, (\d+) refused sizes, (\d+) annotated source pixels, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) > 400 and int(m.group(3)) > 10000, r.stdout[-500:]


def test_abi_structure_and_python_layer(tmp_path):
    spec = _native.preview_spec(0.5, "rgb")
    assert (spec.struct_size, spec.factor, spec.out_format, spec.draw_frame) == (C.sizeof(_native.PreviewSpec), 0.5, _native.PIX_RGB, 0)
    assert _native.preview_spec().factor == 0.0
    with pytest.raises(ValueError):
        _native.preview_spec(out_format="nv12")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vnect_abi.h"\nint main(void){printf("%zu %zu %zu %zu %d\\n", sizeof(vnect_preview_spec), '
                   'offsetof(vnect_preview_spec, factor), offsetof(vnect_preview_spec, out_format), offsetof(vnect_preview_spec, draw_frame), VNECT_PREVIEW_MAX);return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(R.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _native.PreviewSpec
    assert got == [C.sizeof(S), S.factor.offset, S.out_format.offset, S.draw_frame.offset, _native.PREVIEW_MAX] and render.PREVIEW_MAX == got[4]
    assert {"vnect_preview_size", "vnect_preview_device"} <= set(_native.SYMBOLS)
    with pytest.raises(ValueError):
        render.preview_exact(np.zeros((50, 70, 3), np.uint8), None, R.PARENTS, None, factor=0.009)
    with pytest.raises(ValueError):
        render.preview_exact(np.zeros((50, 70, 3), np.uint8), None, R.PARENTS, None, out_format="nv12")
