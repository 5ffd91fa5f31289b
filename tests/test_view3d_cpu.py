"""CPU: the 3-D view's rule (VIEW3D.md).  Three statements agree byte for byte on the whole output buffer of every case, padding included:
tests/view3d_ref.py (numpy, written from VIEW3D.md), render.view3d_exact (numpy, the package's) and g++'s walk of the kernel's tiles over
vnect_amd/csrc/view3d.h (libvnect_view3d.so).  Known answers derived by hand, the walk's refusals, the colour table against matplotlib's,
and the sanitizer sweep as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import view3d_ref as V
from vnect_amd import _native, render


def _exact(case, rows, cols):
    return render.view3d_exact(case["joints"], (rows, cols), case.get("view"), case.get("extent", 500.0), case.get("line_width", 3.0),
                               case.get("background"), case.get("colors"), case.get("parents"), case.get("conf"), case.get("thr"),
                               "rgb" if case.get("fmt") else "bgr", case.get("order", 0))


@pytest.mark.parametrize("size", V.SIZES, ids=["%dx%d" % s for s in V.SIZES])
def test_numpy_statements_and_host_walk_agree(size):
    rows, cols = size
    drawn = 0
    for n, case in enumerate(V.cases(rows, cols)):
        exp = V.expected(case, rows, cols)
        assert np.array_equal(_exact(case, rows, cols), exp), (size, n)
        bg = np.array(case.get("background", (255, 255, 255)))[::-1 if case.get("fmt") else 1]
        drawn += int((exp != bg).any(axis=2).sum())
        for pad in V.PADS if (n % 4 == 0 or rows < 100) else V.PADS[n % 3:n % 3 + 1]:
            out, pitch = V.out_buffer(rows, cols, n % 4, pad)
            V.cpu_backend(case, rows, cols, out, n % 4, pitch)
            assert np.array_equal(out, V.whole(exp, n % 4, pitch)), (size, n, pad)
    if rows * cols > 1000:
        assert drawn > 50 * len(V.cases(rows, cols))     # not vacuous: limbs are drawn


def test_orders_and_formats_differ_and_the_disc_is_a_disc():
    cs = V.cases(400, 400)
    pics = {(c.get("fmt", 0), c.get("order", 0)): V.expected(c, 400, 400) for c in cs[4:8]}      # the tilted view
    assert not np.array_equal(pics[(0, 0)], pics[(0, 1)])
    assert np.array_equal(pics[(0, 0)][:, :, ::-1], pics[(1, 0)])
    # the view along x: limb 3 projects onto one point -> exactly the pixels within w / 2 = 1.5 of it carry its colour somewhere
    c = [c for c in cs[8:12] if c.get("fmt", 0) == 0 and c.get("order", 0) == 1][0]
    only = dict(c, parents=[i if i != 3 else 2 for i in range(21)])
    pic = V.expected(only, 400, 400)
    k = 399.0 / 1000.0
    pc, pr = 199.5 + (-100.0) * k, 199.5 + 150.0 * k
    yy, xx = np.mgrid[0:400, 0:400]
    disc = (xx - pc) ** 2 + (yy - pr) ** 2 <= 2.25
    assert disc.sum() > 4 and np.array_equal((pic != 255).any(axis=2), disc)


def test_the_hand_answer():
    """65 x 65, extent 32 (k = 1, centre 32), width 3, one limb (-22, -22, 0) -> (18, -22, 0): the segment from (row 10, col 10) to (row 10,
    col 50), and the pixels within 1.5 of it -- rows 9 .. 11 of columns 10 .. 50, and the round caps add rows 9 .. 11 of columns 9 and 51
    (their corners lie sqrt(2) <= 1.5 from an end; column 8 and rows 8 and 12 lie 2 away): 3 x 43 = 129 pixels of colour 0"""
    par = list(range(21))
    par[0] = 1
    j = np.zeros((21, 3), np.float32)
    j[0], j[1] = (-22, -22, 0), (18, -22, 0)
    exp = np.full((65, 65, 3), 255, np.uint8)
    exp[9:12, 9:52] = V.CYCLE_RGB[0][::-1]
    assert int((exp != 255).any(axis=2).sum()) == 129
    case = dict(joints=j, parents=par, extent=32.0)
    assert np.array_equal(V.expected(case, 65, 65), exp)
    assert np.array_equal(_exact(case, 65, 65), exp)
    out, pitch = V.out_buffer(65, 65, 0, 0)
    V.cpu_backend(case, 65, 65, out, 0, pitch)
    assert np.array_equal(out.reshape(65, 65, 3), exp)


def test_the_order_answer():
    """two crossing limbs: limb 0 (joint 0 -> 1) horizontal at depth -50, limb 2 (joint 2 -> 3) vertical at depth +50.  Order 0: the higher
    index (2) owns the crossing; order 1: the nearer one (0, the smaller depth) does"""
    par = list(range(21))
    par[0], par[2] = 1, 3
    j = np.zeros((21, 3), np.float32)
    j[0], j[1], j[2], j[3] = (-20, 0, -50), (20, 0, -50), (0, -20, 50), (0, 20, 50)
    for backend in ("ref", "exact", "walk"):
        for order, top in ((0, 2), (1, 0)):
            case = dict(joints=j, parents=par, extent=32.0, order=order)
            if backend == "walk":
                out, pitch = V.out_buffer(65, 65, 0, 0)
                V.cpu_backend(case, 65, 65, out, 0, pitch)
                pic = out.reshape(65, 65, 3)
            else:
                pic = V.expected(case, 65, 65) if backend == "ref" else _exact(case, 65, 65)
            assert tuple(pic[32, 32]) == V.CYCLE_RGB[top][::-1], (backend, order)
            assert tuple(pic[32, 20]) == V.CYCLE_RGB[0][::-1] and tuple(pic[20, 32]) == V.CYCLE_RGB[2][::-1]
    # equal keys: the higher index
    j[:4, 2] = 0
    assert tuple(V.expected(dict(joints=j, parents=par, extent=32.0, order=1), 65, 65)[32, 32]) == V.CYCLE_RGB[2][::-1]
    assert tuple(_exact(dict(joints=j, parents=par, extent=32.0, order=1), 65, 65)[32, 32]) == V.CYCLE_RGB[2][::-1]


def test_the_colour_table_is_matplotlibs_cycle():
    t = np.zeros((21, 3), np.int32)
    V.cpu_lib().view3d_default_colors(t.ctypes.data_as(V.i32p))
    assert [tuple(int(v) for v in r[::-1]) for r in t] == [V.CYCLE_RGB[i % 10] for i in range(21)]
    assert [tuple(c) for c in render.VIEW3D_CYCLE_RGB] == V.CYCLE_RGB
    matplotlib = pytest.importorskip("matplotlib")
    from matplotlib.colors import to_rgb
    cyc = [tuple(int(round(255 * v)) for v in to_rgb(c)) for c in matplotlib.rcParamsDefault["axes.prop_cycle"].by_key()["color"]]
    assert cyc == V.CYCLE_RGB


def test_view_matrix():
    assert np.array_equal(render.view_matrix(-90, -90), np.eye(3))
    assert np.array_equal(render.view_matrix(20, -60), V.views()["tilted"])
    for e, a in ((20, -60), (35.5, 10), (-90, -90), (0, 0)):
        R = render.view_matrix(e, a)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)


def test_the_walks_refusals():
    j = V.skeleton(1)
    good = dict(joints=j)

    def rc(case, rows=33, cols=65, pad=0, short=0, off=0):
        out, pitch = V.out_buffer(rows if 0 < rows <= 2048 else 1, cols if 0 < cols <= 2048 else 1, off, 0)
        pitch += pad
        out = out[:out.size - short] if short else out
        before = out.copy()
        args, keep = V.walk_args(case, rows, cols, out, off, pitch)
        r = V.cpu_lib().view3d_walk(*args)
        if r:
            assert np.array_equal(out, before)       # a refusal writes nothing
        return r

    assert rc(good) == 0
    assert rc(good, rows=-1) == -1 and rc(good, cols=2049) == -1 and rc(good, rows=2049) == -1
    assert rc(good, pad=-1) == -1                       # out_pitch < 3 * cols
    assert rc(good, short=1) == -1                      # the last row would end outside the buffer
    for bad in (dict(extent=-1.0), dict(extent=float("inf")), dict(extent=float("nan")), dict(line_width=-2.0), dict(line_width=64.5),
                dict(line_width=float("nan")), dict(fmt=2), dict(order=2), dict(order=-1), dict(background=(0, 256, 0)),
                dict(colors=[(0, 0, -1)] * 21), dict(parents=[21] + [0] * 20), dict(parents=[-1] + [0] * 20),
                dict(view=np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1.0])), dict(view=np.array([1, 0, 0, 0, 1, 0, 0, 0, np.inf]))):
        assert rc(dict(good, **bad)) == -1, bad
    assert rc(dict(good, line_width=64.0)) == 0
    # zero fields are the defaults: 400 x 400, extent 500, width 3
    out, pitch = V.out_buffer(400, 400, 0, 0)
    args, keep = V.walk_args(dict(good, extent=0.0, line_width=0.0), 0, 0, out, 0, pitch)
    assert V.cpu_lib().view3d_walk(*args) == 0
    assert np.array_equal(out.reshape(400, 400, 3), V.expected(good, 400, 400))


def test_sanitizer_sweep_is_a_standalone_program():
    """view3d_capi.cpp with its own main under -fsanitize=address,undefined (runtimes linked statically; never loaded into python): outputs
    in exactly sized heap blocks at every size and pitch, every walk held to a per-pixel statement of the rule"""
    subprocess.check_call(["make", "-C", V.CSRC, "view3d_sweep_asan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(V.LIBDIR, "view3d_sweep_asan")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"view3d sweep: (\d+) walks, (\d+) limb pixels, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) >= 180 and int(m.group(2)) > 10000, r.stdout[-500:]


def test_abi_structure_and_python_layer():
    s = _native.view3d_spec((33, 65), render.view_matrix(20, -60), extent=250.0, line_width=5.0, background=(1, 2, 3), min_confidence=0.5,
                            out_format="rgb", order=1)
    assert (s.struct_size, s.rows, s.cols, s.extent, s.line_width) == (C.sizeof(_native.View3dSpec), 33, 65, 250.0, 5.0)
    assert (s.has_view, s.has_background, s.has_colors, s.has_parents, s.out_format, s.order) == (1, 1, 0, 0, _native.PIX_RGB, 1)
    assert list(s.view) == list(render.view_matrix(20, -60).reshape(-1)) and s.min_confidence == 0.5
    d = _native.view3d_spec()
    assert (d.rows, d.cols, d.has_view) == (400, 400, 0) and d.min_confidence != d.min_confidence
    for bad in (dict(size=0), dict(extent=0), dict(line_width=0), dict(out_format="nv12"), dict(view=np.eye(2)), dict(parents=[0] * 20),
                dict(colors=[(0, 0, 0)] * 20)):
        with pytest.raises(ValueError):
            _native.view3d_spec(**bad)
    for name in ("vnect_view3d_device", "vnect_track_view3d", "vnect_result_view3d"):
        assert name in _native.SYMBOLS
    header = open(os.path.join(V.ROOT, "include", "vnect_abi.h")).read()
    assert "#define VNECT_ABI_VERSION 7" in header and "#define VNECT_VIEW3D_MAX %d" % _native.VIEW3D_MAX in header
    assert V.tile()[4] == _native.VIEW3D_MAX
    with pytest.raises(ValueError):
        render.view3d_exact(np.zeros((21, 3)), size=0)
    with pytest.raises(ValueError):
        render.view3d_exact(np.zeros((20, 3)))
