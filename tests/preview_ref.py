"""What the preview (PREVIEW.md) is held to, and the cases the CPU and GPU tests share.

The expected bytes are a COMPOSITION OF EXISTING PINS, none of them written for the preview: the oriented picture by tests/orient_ref.py's
rule (np.rot90 / mirror) over the layout's pixels -- an NV12 source converted by tests/nv12_ref.py's restatement --, annotated by
render.draw_limbs_2d_exact (pinned to tests/overlay_ref.py by tests/test_overlay_cpu.py), scaled by oracle.resize (the C restatement of
cv2's resize the pyramid is held to).  render.preview_exact (numpy only), libvnect_preview.so (g++'s walk of the kernel's tiles over
vnect_amd/csrc/preview.h) and the device must each reproduce them on the WHOLE output buffer: pitch padding, the bytes in front of the
first row and behind the last one keep their canary.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle
from tests import nv12_ref, orient_ref
from tests import overlay_ref as R
from vnect_amd import render

LIBDIR, CSRC = R.LIBDIR, R.CSRC
u8p, i32p, f64p = R.u8p, R.i32p, R.f64p
_WALK_ARGS = [u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int,
              f64p, f64p, C.c_double, i32p, i32p, i32p, i32p, C.c_double, C.c_int, u8p, C.c_int64, C.c_int64, C.c_int64]
_libs = {}
CANARY = 0xA5
SIZES = [(70, 50), (96, 64), (150, 131)]            # 70 x 50 and 96 x 64 are even: they serve NV12 as they are
FACTORS = [0.5, 0.37, 1.0 / 3.0, 1.0, 1.7, None]    # None: the reference's 1024 / the longer side


def cpu_lib():
    """g++'s build of vnect_amd/csrc/preview.h behind preview_capi.cpp (no GPU code)"""
    if "cpu" not in _libs:
        subprocess.check_call(["make", "-C", CSRC, "preview"], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_preview.so"))
        L.preview_walk.restype, L.preview_walk.argtypes = C.c_int, _WALK_ARGS
        L.preview_tile.restype, L.preview_tile.argtypes = None, [i32p]
        L.preview_size.restype, L.preview_size.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, i32p]
        _libs["cpu"] = L
    return _libs["cpu"]


def probe_lib():
    """the product's preview.o behind preview_probe.hip (built by _native.build(); needs a GPU to run)"""
    if "probe" not in _libs:
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_previewprobe.so"))
        L.pp_layout.restype, L.pp_layout.argtypes = None, [i32p]
        L.pp_preview.restype, L.pp_preview.argtypes = C.c_int, _WALK_ARGS + [C.c_int, C.c_int, C.c_int, u8p]
        _libs["probe"] = L
    return _libs["probe"]


def tile():
    """(width, height, lanes, pixels per lane) of the kernel's output tile, from the CPU shim -- not restated here"""
    t = np.zeros(4, np.int32)
    cpu_lib().preview_tile(t.ctypes.data_as(i32p))
    return tuple(int(v) for v in t)


def layouts(H, W):
    """tests/overlay_ref.py's layouts (each frame's last byte is its buffer's last), a packed frame at every base alignment 0 .. 3, and NV12
    with the UV plane apart (`uv_separate`: the device tests give it an allocation of its own)"""
    out = [dict(lay, uv_separate=0) for lay in R.layouts(H, W)]
    for off in (0, 2, 3):   # (1 is packed3_odd_base)
        out.append(dict(name="packed3_base%d" % off, format=0, H=H, W=W, data_off=off, uv_off=0, sy=3 * W + 1, sx=3, sc=1, uv_stride=0,
                        size=off + (H - 1) * (3 * W + 1) + 3 * W, uv_separate=0))
    He, We = (H + 1) & ~1, (W + 1) & ~1
    uv_off = He * We + 5
    out.append(dict(name="nv12_two_planes", format=2, H=He, W=We, data_off=0, uv_off=uv_off, sy=We, sx=1, sc=0, uv_stride=We + 2,
                    size=uv_off + (He // 2 - 1) * (We + 2) + We, uv_separate=1))
    return out


LAYOUT_NAMES = [lay["name"] for lay in layouts(*SIZES[0])]


def fresh(lay, seed=0):
    """a layout's source bytes: uniformly random (an NV12 frame then saturates channels in both directions)"""
    return np.random.RandomState(seed + 11).randint(0, 256, lay["size"]).astype(np.uint8)


def picture(buf, lay, o):
    """the oriented BGR picture P of the frame `lay` describes in `buf` (a fresh contiguous array)"""
    H, W = lay["H"], lay["W"]
    if lay["format"] == 2:
        ys = np.lib.stride_tricks.as_strided(buf[lay["data_off"]:], (H, W), (lay["sy"], 1))
        uv = np.lib.stride_tricks.as_strided(buf[lay["uv_off"]:], (H // 2, W // 2, 2), (lay["uv_stride"], 2, 1))
        up = np.repeat(np.repeat(uv, 2, axis=0), 2, axis=1)
        bgr = nv12_ref.restate_yuv(ys, up[..., 0], up[..., 1])
    else:
        bgr = R.view(buf, lay)
        if lay["format"] == 1:
            bgr = bgr[:, :, ::-1]
    return np.ascontiguousarray(orient_ref.oriented(np.asarray(bgr, np.uint8), o))


def skeleton(Hp, Wp, seed=3):
    """21 joints uniform in the central 80 % of the picture, the reference's parents, a rect at a 5 % margin"""
    rs = np.random.RandomState(seed)
    j = np.stack([rs.uniform(0.1 * Hp, 0.9 * Hp, 21), rs.uniform(0.1 * Wp, 0.9 * Wp, 21)], 1)
    x, y = int(0.05 * Wp), int(0.05 * Hp)
    return R._case("skeleton80", joints=j, parents=R.PARENTS, rect=(x, y, Wp - 2 * x, Hp - 2 * y))


def cases(Hp, Wp):
    """tests/overlay_ref.py's cases of an (Hp, Wp) picture (limbs over every edge, non-finite and far joints, a band flush with the border
    and hanging over it, a threshold ...), then: nothing to draw at all (no joints, no rect), a rect without joints, joints without a
    rect, every joint NaN, every joint outside, and the skeleton of the non-vacuity condition"""
    cs = list(R.cases(Hp, Wp))
    body = skeleton(Hp, Wp)
    cs.append(dict(R._case("plain"), joints=None, rect=None))
    cs.append(dict(R._case("rect_no_joints", rect=(4, 5, Wp - 9, Hp - 11)), joints=None))
    cs.append(R._case("joints_no_rect", joints=body["joints"], parents=R.PARENTS))
    cs.append(R._case("all_nan", joints=np.full((21, 2), np.nan), parents=R.PARENTS, rect=(0, 0, Wp, Hp)))
    cs.append(R._case("all_outside", joints=body["joints"] + [3.0 * Hp, 0.0], parents=R.PARENTS))
    cs.append(body)
    return cs


def shape_of(Hp, Wp, f):
    """(dh, dw) by the oracle's cv_round, or None for what the rule refuses"""
    f = 1024.0 / max(Hp, Wp) if not f else f
    if not (0.0 < f < 1e300):
        return None
    dh, dw = oracle.cvround(Hp * f), oracle.cvround(Wp * f)
    return (dh, dw) if 1 <= dh <= 4096 and 1 <= dw <= 4096 else None


_EXPECTED = {}


def annotated(P, case):
    if case["joints"] is None and case.get("rect") is None:
        return P
    j = np.full((21, 2), np.nan) if case["joints"] is None else case["joints"]
    return render.draw_limbs_2d_exact(P, j, case["parents"], case.get("rect"), confidence=case.get("conf"), min_confidence=case.get("thr"))


def expected(buf, lay, o, case, f, fmt=0, key=None):
    """THE COMPOSITION: oracle.resize(render.draw_limbs_2d_exact(picture, ...), f) -> (dh, dw, 3) in the output's channel order.  Computed
    once per `key` and shared (read-only)."""
    if key is not None and key in _EXPECTED:
        return _EXPECTED[key]
    P = picture(buf, lay, o)
    ff = 1024.0 / max(P.shape[:2]) if not f else f
    out = oracle.resize(annotated(P, case), ff)
    assert out.shape[:2] == shape_of(P.shape[0], P.shape[1], f)
    if fmt:
        out = np.ascontiguousarray(out[:, :, ::-1])
    out.setflags(write=False)
    if key is not None:
        _EXPECTED[key] = out
    return out


def out_buffer(dh, dw, out_off, pad):
    """a canary-filled output buffer whose last row's last byte is its last: (buffer, pitch)"""
    pitch = 3 * dw + pad
    return np.full(out_off + (dh - 1) * pitch + 3 * dw, CANARY, np.uint8), pitch


def whole(exp, out_off, pitch):
    """the whole output buffer as it must be afterwards"""
    dh, dw = exp.shape[:2]
    want, _ = out_buffer(dh, dw, out_off, pitch - 3 * dw)
    rows = np.lib.stride_tricks.as_strided(want[out_off:], (dh, 3 * dw), (pitch, 1))
    rows[:] = exp.reshape(dh, 3 * dw)
    return want


def walk_args(buf, lay, o, case, f, fmt, out, out_off, pitch, has_rect=0, limb_bgr=None, rect_bgr=None):
    """the arguments preview_walk and pp_preview share, and the arrays they point into (keep them alive for the call)"""
    keep = [None if case["joints"] is None else np.ascontiguousarray(case["joints"], np.float64),
            None if case.get("conf") is None else np.ascontiguousarray(case["conf"], np.float64),
            np.asarray(case["parents"], np.int32),
            None if case.get("rect") is None else np.asarray(case["rect"], np.int32),
            None if limb_bgr is None else np.asarray(limb_bgr, np.int32), None if rect_bgr is None else np.asarray(rect_bgr, np.int32)]
    p = R._ptr
    thr = case.get("thr")
    args = [p(buf, u8p), len(buf), lay["data_off"], lay["uv_off"], lay["format"], lay["H"], lay["W"], lay["sy"], lay["sx"], lay["sc"],
            lay["uv_stride"], has_rect, o, p(keep[0], f64p), p(keep[1], f64p), float("nan") if thr is None else float(thr), p(keep[2], i32p),
            p(keep[3], i32p), p(keep[4], i32p), p(keep[5], i32p), 0.0 if f is None else float(f), fmt, p(out, u8p), len(out), out_off, pitch]
    return args, keep


def jobs(size, li):
    """The (layout, code, case, factor, out format, output offset, pitch padding) of one size and layout: every case once, codes, factors,
    output alignments and paddings going round so that over the sizes and layouts every pairing occurs."""
    lay = layouts(*size)[li]
    out = []
    k = li + size[0]
    for o in ((k % 8), ((k * 3 + 1) % 8)):
        Hp, Wp = orient_ref.oriented_size(o, lay["H"], lay["W"])
        for ci, case in enumerate(cases(Hp, Wp)):
            if (ci + o) % 2 and case["name"] != "skeleton80":
                continue                                         # (each case under one of the two codes; the skeleton under both)
            f = FACTORS[(ci + k) % len(FACTORS)]
            out.append((lay, o, case, f, (ci + k) % 2, (ci + li) % 4, (0, 1, 7)[(ci + k) % 3]))
    return out


def run_jobs(size, li, backend):
    """backend(src, lay, o, case, f, fmt, out, out_off, pitch) -> the source bytes afterwards.  Every job's whole output buffer must equal
    the composition and its source must be unchanged.  Returns the share of annotated output pixels per skeleton job."""
    shares = []
    for lay, o, case, f, fmt, out_off, pad in jobs(size, li):
        src = fresh(lay)
        key = (size, lay["name"], o, case["name"], f, fmt)
        exp = expected(src, lay, o, case, f, fmt, key)
        out, pitch = out_buffer(exp.shape[0], exp.shape[1], out_off, pad)
        after = backend(src.copy(), lay, o, case, f, fmt, out, out_off, pitch)
        assert np.array_equal(after, src), (key, "the source was written")
        want = whole(exp, out_off, pitch)
        if not np.array_equal(out, want):
            bad = np.nonzero(out != want)[0]
            raise AssertionError((key, "differing bytes", len(bad), "of", len(want), "first at", int(bad[0]), "got", out[bad[:6]], "want", want[bad[:6]]))
        if case["name"] == "skeleton80" and exp.shape[0] * exp.shape[1] > 1:
            plain = expected(src, lay, o, dict(case, joints=None, rect=None), f, fmt)
            shares.append((key, float((exp != plain).any(axis=2).mean())))
    return shares


def cpu_backend(src, lay, o, case, f, fmt, out, out_off, pitch):
    args, keep = walk_args(src, lay, o, case, f, fmt, out, out_off, pitch)
    rc = cpu_lib().preview_walk(*args)
    assert rc == 0, (rc, lay["name"], case["name"], f)
    return src


def make_gpu_backend(probe, guard, fill, tracked=0, status=0):
    def backend(src, lay, o, case, f, fmt, out, out_off, pitch):
        guards = np.zeros(2 * guard, np.uint8)
        args, keep = walk_args(src, lay, o, case, f, fmt, out, out_off, pitch)
        rc = probe.pp_preview(*args, lay.get("uv_separate", 0), tracked, status, guards.ctypes.data_as(u8p))
        assert rc == 0, (rc, lay["name"], case["name"], f)          # a case the shim refuses is a failure, not a skip
        assert (guards == fill).all(), (lay["name"], case["name"], "a guard byte was written", np.nonzero(guards != fill)[0][:8])
        return src
    return backend


def plain_layout(H, W, fmt=0):
    """a packed BGR (fmt 0) or single-buffer NV12 (fmt 2) frame"""
    if fmt == 2:
        return dict(name="nv12", format=2, H=H, W=W, data_off=0, uv_off=H * W, sy=W, sx=1, sc=0, uv_stride=W, size=H * W * 3 // 2, uv_separate=0)
    return dict(name="packed3", format=0, H=H, W=W, data_off=0, uv_off=0, sy=3 * W, sx=3, sc=1, uv_stride=0, size=3 * H * W, uv_separate=0)


def special_jobs():
    """(layout, code, case, factor) beyond the round-robin: footprints that exceed any LDS budget, the default factor's 1024 x 731, a
    one-pixel-wide and a one-pixel-high output, a factor that keeps one axis only (not a copy), and output sizes that straddle the kernel's
    tile in both axes by -1, 0, +1."""
    tw, th = tile()[:2]
    out = []
    for H, W in ((64, 1024), (1024, 64)):
        for f in (1.0 / 16, 1.0 / 3):
            out.append((plain_layout(H, W), 0, skeleton(H, W), f))
            out.append((plain_layout(H, W, 2), 5, skeleton(W, H), f))
    out.append((plain_layout(50, 70), 0, skeleton(50, 70), None))             # 70 x 50 -> 1024 x 731
    assert shape_of(50, 70, None) == (731, 1024)
    out.append((plain_layout(70, 50), 3, skeleton(50, 70), 0.025))            # dh == 1
    out.append((plain_layout(70, 50), 0, skeleton(70, 50), 0.025))            # dw == 1
    assert shape_of(50, 70, 0.025) == (1, 2) and shape_of(70, 50, 0.025) == (2, 1)
    out.append((plain_layout(50, 70), 0, skeleton(50, 70), 1.008))            # 70 -> 71 columns, 50 rows stay: one axis kept is no copy
    assert shape_of(50, 70, 1.008) == (50, 71)
    for d in (-1, 0, 1):
        H, W = 2 * (th + d), 2 * (tw + d)
        out.append((plain_layout(H, W), 0, skeleton(H, W), 0.5))
        out.append((plain_layout(H, W, 2), 6, skeleton(H, W), 0.5))
        out.append((plain_layout(2 * th + d, 2 * tw - d), 0, skeleton(2 * th + d, 2 * tw - d), 1.0))
    return out


def run_special(backend):
    for n, (lay, o, case, f) in enumerate(special_jobs()):
        src = fresh(lay, n)
        exp = expected(src, lay, o, case, f, 0, ("special", n))
        out, pitch = out_buffer(exp.shape[0], exp.shape[1], n % 4, (0, 5)[n % 2])
        after = backend(src.copy(), lay, o, case, f, 0, out, n % 4, pitch)
        assert np.array_equal(after, src), (n, "the source was written")
        want = whole(exp, n % 4, pitch)
        assert np.array_equal(out, want), (n, lay["name"], (lay["H"], lay["W"]), o, f, "differing bytes", int((out != want).sum()))
