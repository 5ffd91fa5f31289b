"""An independent numpy statement of the overlay's drawing rule (OVERLAY.md), written from the rule's text and not from
vnect_amd/csrc/overlay.h: what libvnect_overlay.so (the host walk of the kernel's code), render.draw_limbs_2d_exact and the device are
held to, byte for byte.  Also the layouts, frame sizes and cases the CPU and GPU tests share.  No tiles and no culling here: every limb
is tested against every pixel of the frame.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
LIBDIR = os.path.join(ROOT, "vnect_amd", "lib")
u8p, i32p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
_WALK_ARGS = [u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, f64p, f64p,
              C.c_double, i32p, i32p, i32p, i32p]
_libs = {}
LIMB_BGR = (49, 22, 122)
RECT_BGR = (60, 66, 207)
PARENTS = [16, 15, 1, 2, 3, 1, 5, 6, 14, 8, 9, 14, 11, 12, 14, 14, 1, 4, 7, 10, 13]   # src/estimator.py joint_parents
SIZES = [(37, 53), (64, 48), (120, 200)]


def cpu_lib():
    """g++'s build of vnect_amd/csrc/overlay.h behind overlay_capi.cpp (no GPU code)"""
    if "cpu" not in _libs:
        path = os.path.join(LIBDIR, "libvnect_overlay.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", CSRC, "overlay"], stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.overlay_walk.restype, L.overlay_walk.argtypes = C.c_int, _WALK_ARGS
        L.overlay_tile.restype, L.overlay_tile.argtypes = None, [i32p]
        L.overlay_yuv.restype, L.overlay_yuv.argtypes = None, [i32p, u8p]
        L.overlay_limb_setup.restype, L.overlay_limb_setup.argtypes = None, [C.c_double] * 4 + [f64p]
        _libs["cpu"] = L
    return _libs["cpu"]


def probe_lib():
    """the product's overlay.o behind overlay_probe.hip (built by _native.build(); needs a GPU to run)"""
    if "probe" not in _libs:
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_overlayprobe.so"))
        L.op_layout.restype, L.op_layout.argtypes = None, [i32p]
        L.op_draw.restype, L.op_draw.argtypes = C.c_int, _WALK_ARGS + [C.c_int, C.c_int, u8p]
        _libs["probe"] = L
    return _libs["probe"]


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def walk_args(buf, lay, case, limb_bgr=LIMB_BGR, rect_bgr=RECT_BGR):
    """the arguments overlay_walk and op_draw share, and the arrays they point into (keep them alive for the call)"""
    keep = [np.ascontiguousarray(case["joints"], np.float64),
            None if case.get("conf") is None else np.ascontiguousarray(case["conf"], np.float64),
            np.asarray(case["parents"], np.int32),
            None if case.get("rect") is None else np.asarray(case["rect"], np.int32),
            np.asarray(limb_bgr, np.int32), np.asarray(rect_bgr, np.int32)]
    thr = case.get("thr")
    args = [_ptr(buf, u8p), len(buf), lay["data_off"], lay["uv_off"], lay["format"], lay["H"], lay["W"], lay["sy"], lay["sx"], lay["sc"],
            lay["uv_stride"], _ptr(keep[0], f64p), _ptr(keep[1], f64p), float("nan") if thr is None else float(thr), _ptr(keep[2], i32p),
            _ptr(keep[3], i32p), _ptr(keep[4], i32p), _ptr(keep[5], i32p)]
    return args, keep


def half_axis(L2):
    """the largest integer a >= 0 with 4 a a <= L2"""
    a = int(math.sqrt(L2) / 2)
    while a > 0 and 4.0 * a * a > L2:
        a -= 1
    while 4.0 * (a + 1) * (a + 1) <= L2:
        a += 1
    return a


def limb_setup(r1, c1, r2, c2):
    """None for a skipped limb, else (dr, dc, L2, a, cr, cc)"""
    vals = [float(r1), float(c1), float(r2), float(c2)]
    if any(math.isnan(v) or math.isinf(v) or abs(v) > 2.0 ** 20 for v in vals):
        return None
    dr, dc = vals[0] - vals[2], vals[1] - vals[3]
    L2 = dr * dr + dc * dc
    a = half_axis(L2)
    if a == 0:
        return None
    return dr, dc, L2, a, round((vals[0] + vals[2]) / 2), round((vals[1] + vals[3]) / 2)   # Python's round: half to even


def limb_mask(H, W, joints, parents, conf=None, thr=None):
    m = np.zeros((H, W), bool)
    y = np.arange(H, dtype=np.float64).reshape(H, 1) * np.ones((1, W))
    x = np.ones((H, 1)) * np.arange(W, dtype=np.float64).reshape(1, W)
    for i in range(21):
        p = parents[i]
        if thr is not None and conf is not None and (conf[i] < thr or conf[p] < thr):
            continue
        su = limb_setup(joints[i][0], joints[i][1], joints[p][0], joints[p][1])
        if su is None:
            continue
        dr, dc, L2, a, cr, cc = su
        u, v = y - float(cr), x - float(cc)
        s = u * dr + v * dc
        t = u * dc - v * dr
        aa = float(a * a)
        m |= (s * s) * 9.0 + (t * t) * aa <= (aa * 9.0) * L2
    return m


def band_mask(H, W, rect):
    m = np.zeros((H, W), bool)
    if rect is None:
        return m
    x0, y0, w, h = (int(v) for v in rect)
    for y in range(max(0, y0 - 2), min(H - 1, y0 + h + 1) + 1):
        for x in range(max(0, x0 - 2), min(W - 1, x0 + w + 1) + 1):
            m[y, x] = not (x0 + 2 <= x <= x0 + w - 3 and y0 + 2 <= y <= y0 + h - 3)
    return m


def yuv_of(bgr):
    B, G, R = (int(v) for v in bgr)
    return (((66 * R + 129 * G + 25 * B + 128) >> 8) + 16, ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128,
            ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128)


_MASKS = {}


def masks(lay, case):
    """(limb mask, band mask) of a case in an (H, W) frame: computed once, shared by every layout and test (read-only)"""
    key = (lay["H"], lay["W"], case["name"]) if case.get("name") else None
    if key is None or key not in _MASKS:
        m = (limb_mask(lay["H"], lay["W"], case["joints"], case["parents"], case.get("conf"), case.get("thr")),
             band_mask(lay["H"], lay["W"], case.get("rect")))
        for a in m:
            a.setflags(write=False)
        if key is None:
            return m
        _MASKS[key] = m
    return _MASKS[key]


def draw(buf, lay, case, limb_bgr=LIMB_BGR, rect_bgr=RECT_BGR):
    """Draws `case` into the flat uint8 buffer `buf` (in place) as layout `lay` addresses it; returns the number of pixels drawn."""
    H, W = lay["H"], lay["W"]
    limb, band = masks(lay, case)
    limb = limb & ~band
    if lay["format"] == 2:
        cols = {1: yuv_of(limb_bgr), 2: yuv_of(rect_bgr)}
        state = np.where(band, 2, np.where(limb, 1, 0))
        for st in (1, 2):
            ys, xs = np.nonzero(state == st)
            buf[lay["data_off"] + ys * lay["sy"] + xs] = cols[st][0]
        quads = state.reshape(H // 2, 2, W // 2, 2)
        for st in (1, 2):                            # the rect's chroma last: it wins the block
            bys, bxs = np.nonzero((quads == st).any(axis=(1, 3)))
            o = lay["uv_off"] + bys * lay["uv_stride"] + 2 * bxs
            buf[o], buf[o + 1] = cols[st][1], cols[st][2]
    else:
        order = (2, 1, 0) if lay["format"] == 1 else (0, 1, 2)
        for mask, col in ((limb, limb_bgr), (band, rect_bgr)):
            ys, xs = np.nonzero(mask)
            for c in range(3):
                buf[lay["data_off"] + ys * lay["sy"] + xs * lay["sx"] + c * lay["sc"]] = col[order[c]]
    return int(limb.sum() + band.sum())


def layouts(H, W):
    """The layouts of an (H, W) frame (NV12: H and W rounded up to even): dicts with format (0 BGR, 1 RGB, 2 NV12), the byte offsets of the
    frame (and its UV plane) in a buffer of `size` bytes whose last pixel byte is the buffer's last, and the strides."""
    out = []

    def add(name, fmt, off, sy, sx, sc):
        out.append(dict(name=name, format=fmt, H=H, W=W, data_off=off, uv_off=0, sy=sy, sx=sx, sc=sc, uv_stride=0,
                        size=off + (H - 1) * sy + (W - 1) * sx + 2 * sc + 1))

    add("packed3_padded", 0, 0, 3 * W + 7, 3, 1)
    add("packed4", 0, 0, 4 * W, 4, 1)
    add("planar", 0, 0, W + 3, 1, (W + 3) * H + 5)
    add("transposed", 0, 0, 3, 3 * H, 1)            # a (W, H, 3) packed array seen as its transpose
    add("rgb_packed3", 1, 0, 3 * W, 3, 1)
    add("packed3_odd_base", 0, 1, 3 * W + 2, 3, 1)
    add("rgb_packed4_odd_base", 1, 3, 4 * W + 1, 4, 1)
    He, We = (H + 1) & ~1, (W + 1) & ~1
    sy, uvs = We + 6, We + 10
    uv_off = 1 + He * sy + 2                         # (an odd offset, like the Y plane's)
    out.append(dict(name="nv12_pitched_odd_base", format=2, H=He, W=We, data_off=1, uv_off=uv_off, sy=sy, sx=1, sc=0, uv_stride=uvs,
                    size=uv_off + (He // 2 - 1) * uvs + We))
    return out


def fresh(lay, seed=0):
    """the buffer of a layout before a draw: bytes 64 .. 127 (no drawn colour component or canary lies there)"""
    return (np.random.RandomState(seed).randint(64, 128, lay["size"])).astype(np.uint8)


def view(buf, lay):
    """the (H, W, 3) view of a BGR / RGB layout's pixels in `buf`"""
    return np.lib.stride_tricks.as_strided(buf[lay["data_off"]:], shape=(lay["H"], lay["W"], 3), strides=(lay["sy"], lay["sx"], lay["sc"]))


def _case(name, limbs=(), rect=None, conf=None, thr=None, empty=False, joints=None, parents=None):
    """limb k = (r1, c1, r2, c2) sits in joints 2k, 2k + 1 (2k's parent is 2k + 1); every other joint is its own parent"""
    if joints is None:
        joints = np.zeros((21, 2))
        parents = list(range(21))
        for k, (r1, c1, r2, c2) in enumerate(limbs):
            joints[2 * k], joints[2 * k + 1], parents[2 * k] = (r1, c1), (r2, c2), 2 * k + 1
    return dict(name=name, joints=np.asarray(joints, np.float64), parents=list(parents), rect=rect, conf=conf, thr=thr, empty=empty)


def cases(H, W):
    """The cases of an (H, W) frame.  `empty`: the rule draws nothing (every limb skipped or outside, no rect in sight)."""
    nan, inf = float("nan"), float("inf")
    below = float(np.nextafter(18.0, 0.0))
    cs = [
        _case("horizontal", [(10, 5, 10, W - 6)]),
        _case("vertical", [(4, 20, H - 5, 20)]),
        _case("diagonals", [(5, 5, H - 6, W - 12), (H - 6, 5, 5, W - 12)]),
        _case("half_to_even", [(10.0, 10.0, 11.0, 21.0), (21.0, 6.0, 24.0, 25.0), (14.25, 30.75, 28.75, 38.25)]),
        _case("L2_exact", [(10, 10, 10, 18)]),
        _case("L2_one_ulp_below", [(10, 10, 10, below)]),
        _case("short_and_root", [(10, 10, 10.5, 11.8), (20, 20, 20, 20)], empty=True),
        _case("nonfinite", [(nan, 5, 10, 10), (8, inf, 20, 20), (9, 9, -inf, 12), (15, 6, 15, 30)]),
        _case("two_pow_21", [(2.0 ** 21, 5, 10, 10), (5, -2.0 ** 21, 10, 10)], empty=True),
        _case("two_pow_20", [(2.0 ** 20, 5, 5, 5)]),
        _case("half_outside", [(-8, 12, 9, 16), (H - 9, 10, H + 9, 22), (12, -9, 20, 9), (6, W - 8, 16, W + 7)]),
        _case("wholly_outside", [(-30, 5, -12, 25), (H + 12, 5, H + 30, 25), (5, -30, 25, -12), (5, W + 12, 25, W + 30)], empty=True),
        _case("rect_flush", rect=(0, 0, W, H)),
        _case("rect_hanging", [(12, 12, 30, 30)], rect=(-5, -7, 20, 22)),
        _case("rect_hanging_far", rect=(W - 10, H - 12, 30, 31)),
        _case("rect_1x1", rect=(10, 10, 1, 1)),
        _case("rect_2x3", rect=(20, 10, 2, 3)),
        _case("rect_4x4", rect=(10, 20, 4, 4)),
        _case("rect_3x1_edge", rect=(W - 2, 0, 3, 1)),
        _case("rect_outside", rect=(W + 10, H + 10, 5, 5), empty=True),
        _case("band_over_limb", [(3, 3, H - 4, W - 4), (16, 2, 16, W - 3)], rect=(8, 9, 24, 15)),
        _case("nv12_odd_edges", [(11, 11, 11, 31), (13, 13, 31, 13), (5, 21, 27, 33)], rect=(7, 9, 13, 11)),
        _case("confidence", [(6, 6, 6, 30), (14, 6, 14, 30), (22, 6, 22, 30)],
              conf=np.array([0.9, 0.9, 0.9, 0.2, 0.49999, 0.9] + [0.9] * 15), thr=0.5),
    ]
    # the reference's skeleton with its own parents, a person standing in the frame, and the crop rectangle around it
    rs = np.random.RandomState(7)
    body = np.stack([rs.uniform(3, H - 4, 21), rs.uniform(3, W - 4, 21)], 1)
    cs.append(_case("skeleton", joints=body, parents=PARENTS, rect=(3, 2, W - 8, H - 6), conf=rs.uniform(0, 1, 21), thr=0.3))
    return cs
