"""The 3-D view's rule (VIEW3D.md) stated in numpy, independently of vnect_amd/render.py and of vnect_amd/csrc/view3d.h: every limb's
coverage mask by the three-case test, then the limbs painted from the one that lies under all others to the one on top.  Also the cases
the CPU and GPU tests share, the buffers they compare whole (padding and canaries included), and the two test libraries' prototypes."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
LIBDIR = os.path.join(ROOT, "vnect_amd", "lib")
u8p, i32p, f32p, f64p = (C.POINTER(t) for t in (C.c_uint8, C.c_int32, C.c_float, C.c_double))
_WALK_ARGS = [f32p, f64p, C.c_int, C.c_int, C.c_double, f64p, C.c_double, i32p, i32p, i32p, C.c_double, C.c_int, C.c_int, u8p, C.c_int64,
              C.c_int64, C.c_int64]
_libs = {}
CANARY = 0xA5
PARENTS = [16, 15, 1, 2, 3, 1, 5, 6, 14, 8, 9, 14, 11, 12, 14, 14, 1, 4, 7, 10, 13]   # src/estimator.py joint_parents
# matplotlib's colour cycle, RGB (checked against rcParams['axes.prop_cycle'] where matplotlib is installed)
CYCLE_RGB = [(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127),
             (188, 189, 34), (23, 190, 207)]
SIZES = [(1, 1), (1, 7), (33, 65), (65, 33), (400, 400)]
PADS = [0, 1, 5]


def cpu_lib():
    """g++'s build of vnect_amd/csrc/view3d.h behind view3d_capi.cpp (no GPU code)"""
    if "cpu" not in _libs:
        subprocess.check_call(["make", "-C", CSRC, "view3d"], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_view3d.so"))
        L.view3d_walk.restype, L.view3d_walk.argtypes = C.c_int, _WALK_ARGS
        L.view3d_tile.restype, L.view3d_tile.argtypes = None, [i32p]
        L.view3d_default_colors.restype, L.view3d_default_colors.argtypes = None, [i32p]
        _libs["cpu"] = L
    return _libs["cpu"]


def probe_lib():
    """the product's view3d.o behind view3d_probe.hip (built by _native.build(); needs a GPU to run)"""
    if "probe" not in _libs:
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_view3dprobe.so"))
        L.vp_layout.restype, L.vp_layout.argtypes = None, [i32p]
        L.vp_view3d.restype, L.vp_view3d.argtypes = C.c_int, _WALK_ARGS + [C.c_int, C.c_int, u8p]
        _libs["probe"] = L
    return _libs["probe"]


def tile():
    """(width, height, lanes, pixels per lane, largest side) of the kernel's tile, from the CPU shim -- not restated here"""
    t = np.zeros(5, np.int32)
    cpu_lib().view3d_tile(t.ctypes.data_as(i32p))
    return tuple(int(v) for v in t)


def view(joints_3d, rows=400, cols=400, extent=500.0, view=None, line_width=3.0, background=None, colors=None, parents=None, conf=None,
         thr=None, fmt=0, order=0):
    """The (rows, cols, 3) picture by the rule of VIEW3D.md.  colors / background: BGR; fmt 1: the output is RGB."""
    R = np.eye(3) if view is None else np.asarray(view, np.float64).reshape(3, 3)
    par = PARENTS if parents is None else list(parents)
    table = [CYCLE_RGB[i % 10][::-1] for i in range(21)] if colors is None else [tuple(int(v) for v in c) for c in colors]
    bgc = (255, 255, 255) if background is None else tuple(int(v) for v in background)
    s = min(rows, cols)
    k = np.float64(s - 1) / (np.float64(2.0) * np.float64(extent))
    cx, cy = np.float64(cols - 1) * np.float64(0.5), np.float64(rows - 1) * np.float64(0.5)
    half = np.float64(line_width) * np.float64(0.5)
    r2 = half * half
    J = np.asarray(joints_3d, np.float32)
    scr = []
    with np.errstate(all="ignore"):
        for n in range(21):
            x, y, z = (np.float64(J[n, c]) for c in range(3))
            u = (R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z
            v = (R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z
            d = (R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z
            scr.append((cx + u * k, cy + v * k, d))
    lim = np.float64(1048576.0)
    drawn = []                                 # (limb, key)
    for i in range(21):
        p = par[i]
        if p == i:
            continue
        ends = (scr[i], scr[p])
        if any(not np.isfinite(e[q]) or abs(e[q]) > lim for e in ends for q in (0, 1)):
            continue
        if order == 1 and not (np.isfinite(ends[0][2]) and np.isfinite(ends[1][2])):
            continue
        if thr is not None and conf is not None and (conf[i] < thr or conf[p] < thr):
            continue
        drawn.append((i, ends[0][2] + ends[1][2]))
    # from the limb under all others to the one on top: order 0 by index; order 1 by falling key, equal keys by index
    drawn.sort(key=(lambda t: t[0]) if order == 0 else (lambda t: (-t[1], t[0])))
    pic = np.empty((rows, cols, 3), np.uint8)
    pic[:, :] = bgc[::-1] if fmt else bgc
    ys = np.arange(rows, dtype=np.float64)[:, None]
    xs = np.arange(cols, dtype=np.float64)[None, :]
    for i, _ in drawn:
        (ac, ar, _), (bc, br, _) = scr[i], scr[par[i]]
        ex, ey = bc - ac, br - ar
        L2 = ex * ex + ey * ey
        wx, wy = xs - ac, ys - ar
        t = wx * ex + wy * ey
        near_a = t <= 0.0
        near_b = ~near_a & (t >= L2)
        mid = ~near_a & ~near_b
        qx, qy = xs - bc, ys - br
        c = wx * ey - wy * ex
        cover = (near_a & (wx * wx + wy * wy <= r2)) | (near_b & (qx * qx + qy * qy <= r2)) | (mid & (c * c <= r2 * L2))
        pic[cover] = table[i][::-1] if fmt else table[i]
    return pic


# ---- shared cases ----------------------------------------------------------------------------------------------------------------------
def skeleton(seed, extent=500.0):
    """21 joints spread over the cube the view shows, a few of them outside it"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.15, 1.15, (21, 3)) * extent).astype(np.float32)


def views():
    """the identity; view_init(20, -60) as render.view_matrix builds it (restated: no import of render here); a view along the x axis, which
    projects every limb that runs along x onto one point"""
    e, a = np.deg2rad(20.0), np.deg2rad(-60.0)
    ce, se, ca, sa = np.cos(e), np.sin(e), np.cos(a), np.sin(a)
    tilted = np.array([[-sa, ca, 0.0], [se * ca, se * sa, -ce], [-ce * ca, -ce * sa, -se]])
    return {"identity": None, "tilted": tilted, "along_x": np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])}


def cases(rows, cols):
    """the cases of one size: dicts of view()'s keyword arguments plus `joints`"""
    out = []
    vs = views()
    for n, (name, v) in enumerate(vs.items()):
        j = skeleton(100 + n + rows)
        if name == "along_x":                      # limb 3 (joint 3 -> joint 2) along x: its ends project onto one point, a disc
            j[2] = np.float32([50.0, -100.0, 150.0])
            j[3] = j[2] + np.float32([120.0, 0.0, 0.0])
        for fmt in (0, 1):
            for order in (0, 1):
                out.append(dict(joints=j, view=v, fmt=fmt, order=order))
    j = skeleton(7 + cols)
    j[4, 0], j[9, 1], j[12, 0] = np.nan, np.inf, np.float32(3e9)       # skipped: NaN, infinite, beyond 2^20 on the screen
    out.append(dict(joints=j, order=1))
    conf = np.linspace(0.0, 1.0, 21)[::-1].copy()
    out.append(dict(joints=skeleton(8), conf=conf, thr=0.3))
    par = [(i + 1) % 21 for i in range(21)]
    par[5] = 5
    cols_bgr = [((i * 37) % 256, (i * 91 + 5) % 256, (255 - i * 11) % 256) for i in range(21)]
    out.append(dict(joints=skeleton(9), parents=par, colors=cols_bgr, background=(10, 20, 30), line_width=6.5, extent=420.0, fmt=1))
    return out


def out_buffer(rows, cols, off, pad):
    """a canary-filled buffer that holds a rows x cols picture `off` bytes in, rows 3 cols + pad apart, and not a byte more"""
    pitch = 3 * cols + pad
    return np.full(off + (rows - 1) * pitch + 3 * cols, CANARY, np.uint8), pitch


def whole(pic, off, pitch):
    """the buffer out_buffer gives as it must look after `pic` was rendered into it"""
    rows, cols = pic.shape[:2]
    buf = np.full(off + (rows - 1) * pitch + 3 * cols, CANARY, np.uint8)
    np.lib.stride_tricks.as_strided(buf[off:], (rows, 3 * cols), (pitch, 1))[:] = pic.reshape(rows, 3 * cols)
    return buf


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def walk_args(case, rows, cols, out, off, pitch):
    """the arguments view3d_walk and vp_view3d share, and the arrays they point into (keep them alive for the call)"""
    j = np.ascontiguousarray(case["joints"], np.float32)
    conf = None if case.get("conf") is None else np.ascontiguousarray(case["conf"], np.float64)
    v = None if case.get("view") is None else np.ascontiguousarray(case["view"], np.float64).reshape(9)
    bg = None if case.get("background") is None else np.asarray(case["background"], np.int32)
    col = None if case.get("colors") is None else np.ascontiguousarray(case["colors"], np.int32)
    par = None if case.get("parents") is None else np.asarray(case["parents"], np.int32)
    thr = case.get("thr")
    keep = (j, conf, v, bg, col, par, out)
    args = [_ptr(j, f32p), _ptr(conf, f64p), rows, cols, float(case.get("extent", 500.0)), _ptr(v, f64p), float(case.get("line_width", 3.0)),
            _ptr(bg, i32p), _ptr(col, i32p), _ptr(par, i32p), float("nan") if thr is None else float(thr), int(case.get("fmt", 0)),
            int(case.get("order", 0)), _ptr(out, u8p), out.size, off, pitch]
    return args, keep


def expected(case, rows, cols):
    kw = {k: v for k, v in case.items() if k != "joints"}
    return view(case["joints"], rows, cols, **kw)


def cpu_backend(case, rows, cols, out, off, pitch):
    args, keep = walk_args(case, rows, cols, out, off, pitch)
    assert cpu_lib().view3d_walk(*args) == 0
