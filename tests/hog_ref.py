"""The person detector's rule (HOG.md) stated independently in numpy -- written from the document, not from vnect_amd/csrc/hog.h -- and
the plumbing the HOG tests share: g++'s walk of the kernels' tiling (libvnect_hog.so, `make hog`), the device probe over the product's
hog.o (libvnect_hogprobe.so), frames in every layout, and the planted figure (in the manner of tests/planted.py).

Every float32 operation below is one numpy float32 operation, and every sum runs in the order HOG.md fixes, so the numpy statement, the
walk and the GPU agree bit for bit.  The one host-computed ingredient a libm can round differently is the Gaussian table
g(k) = float32(exp(-(k - 7.5)^2 / 32)): `tables()` computes it in float64 itself, holds the library's table to within 1 ulp of float32,
then uses the library's table as data.  G_DIFFER records how many of the 16 entries differed (HOG.md: 0 when this was written)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import preview_ref as P
from vnect_amd import render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
LIBDIR = os.path.join(ROOT, "vnect_amd", "lib")
u8p, i32p, i64p, f32p, f64p = (C.POINTER(t) for t in (C.c_uint8, C.c_int32, C.c_int64, C.c_float, C.c_double))
_libs = {}
F = np.float32
WIN_W, WIN_H, DESC = 64, 128, 3780
DEFAULTS = dict(hit_threshold=0.0, win_stride=(8, 8), scale0=1.05, final_threshold=2.0, nlevels=64, max_hits=65536)
_SPEC_C = [C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
_FRAME_C = [u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64]
G_DIFFER = None


def spec(**kw):
    s = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in s:
            raise TypeError(k)
        s[k] = v
    return s


def spec_args(s):
    return [float(s["hit_threshold"]), int(s["win_stride"][0]), int(s["win_stride"][1]), float(s["scale0"]), float(s["final_threshold"]),
            int(s["nlevels"]), int(s["max_hits"])]


def cpu_lib():
    """g++'s build of vnect_amd/csrc/hog.h behind hog_capi.cpp (no GPU code)"""
    if "cpu" not in _libs:
        subprocess.check_call(["make", "-C", CSRC, "hog"], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_hog.so"))
        L.hog_tile.restype, L.hog_tile.argtypes = None, [i32p]
        L.hog_tables_c.restype, L.hog_tables_c.argtypes = None, [f32p, f32p, f32p]
        L.hog_levels_c.restype, L.hog_levels_c.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int] + _SPEC_C + [i32p, i32p, f64p, i32p, i64p]
        L.hog_walk.restype = C.c_int
        L.hog_walk.argtypes = _FRAME_C + [C.c_int, C.c_int] + _SPEC_C + [f32p, C.c_int, u8p, f32p, u8p, f32p, f32p, i32p, f32p, i32p, i32p, f64p, C.c_int, i32p]
        L.hog_rects_c.restype, L.hog_rects_c.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, i32p, C.c_int, i32p]
        L.hog_group_c.restype, L.hog_group_c.argtypes = C.c_int, [i32p, f64p, C.c_int, C.c_int, i32p]
        _libs["cpu"] = L
    return _libs["cpu"]


def probe_lib():
    """the product's hog.o behind hog_probe.hip (built by _native.build(); needs a GPU to run)"""
    if "probe" not in _libs:
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_hogprobe.so"))
        L.hp_layout.restype, L.hp_layout.argtypes = None, [i32p]
        L.hp_detect.restype = C.c_int
        L.hp_detect.argtypes = _FRAME_C + [C.c_int, C.c_int] + _SPEC_C + [f32p, C.c_int, f32p, u8p, f32p, f32p, i32p, f32p, i64p]
        L.hp_time.restype, L.hp_time.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, f32p, i64p]
        _libs["probe"] = L
    return _libs["probe"]


def tile():
    """(lanes per workgroup, the vote tile's width, its height, blocks / windows per workgroup), from the CPU shim -- not restated here"""
    t = np.zeros(4, np.int32)
    cpu_lib().hog_tile(t.ctypes.data_as(i32p))
    return tuple(int(v) for v in t)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def tables():
    """(lut[256], g[16], wt[4, 16, 16]) -- lut and wt restated here and held bit for bit to the library's; g: see the module's docstring"""
    global G_DIFFER
    if "tables" in _libs:
        return _libs["tables"]
    lut_l, g_l, wt_l = np.zeros(256, F), np.zeros(16, F), np.zeros(1024, F)
    cpu_lib().hog_tables_c(lut_l.ctypes.data_as(f32p), g_l.ctypes.data_as(f32p), wt_l.ctypes.data_as(f32p))
    lut = np.sqrt(np.arange(256, dtype=np.float64)).astype(F)
    assert np.array_equal(lut, lut_l)
    k = np.arange(16, dtype=np.float64)
    g = np.exp(-(k - 7.5) ** 2 / 32.0).astype(F)
    G_DIFFER = int(np.count_nonzero(g != g_l))
    assert np.all(np.abs(g.astype(np.float64) - g_l.astype(np.float64)) <= np.spacing(np.minimum(g, g_l)).astype(np.float64)), (g, g_l)
    g = g_l                                                            # from here on: the library's table as data
    c = (np.arange(16, dtype=F) + F(0.5)) / F(8) - F(0.5)            # a pixel's position in cell units
    f0 = np.floor(c)
    fr = c - f0
    cw = np.zeros((2, 16), F)                                         # [cell][pixel]: the bilinear weight, kept where the cell is 0 or 1
    for cell in (0, 1):
        cw[cell] = np.where(f0 == cell, F(1) - fr, F(0)) + np.where(f0 + 1 == cell, fr, F(0))
    wt = np.zeros((4, 16, 16), F)
    gw = g[:, None] * g[None, :]                                      # g(i) * g(j)
    for cx in (0, 1):
        for cy in (0, 1):
            wt[cx * 2 + cy] = (cw[cx][None, :] * cw[cy][:, None]) * gw
    assert np.array_equal(wt.reshape(-1), wt_l)
    _libs["tables"] = (lut, g, wt)
    return _libs["tables"]


def levels(Hp, Wp, s):
    """[(rows, columns, scale)]: s_0 = 1, s_{n+1} = s_n * scale0 in double; a level exists while both rounded sides hold a window"""
    out, sc = [], 1.0
    for _ in range(int(s["nlevels"])):
        w, h = int(np.rint(Wp / sc)), int(np.rint(Hp / sc))
        if w < WIN_W or h < WIN_H:
            break
        out.append((h, w, sc))
        sc = sc * float(s["scale0"])
    return out


def level_image(pic, h, w):
    """cv2.resize(P, (w, h), INTER_LINEAR) in the pinned 8-bit fixed point, per-axis scale 1.0 / (dst / src); equal sizes: a copy"""
    Hp, Wp = pic.shape[:2]
    if (h, w) == (Hp, Wp):
        return pic.copy()
    x0, x1, a0, a1, edge = render._resize_axis(w, Wp, 1.0 / (float(w) / float(Wp)), True)
    y0, y1, b0, b1, _ = render._resize_axis(h, Hp, 1.0 / (float(h) / float(Hp)), False)
    src = pic.astype(np.int64)
    a0, a1, edge = a0[None, :, None], a1[None, :, None], edge[None, :, None]

    def row(y):
        top = src[y]
        return np.where(edge, top[:, x0] * 2048, top[:, x0] * a0 + top[:, np.minimum(x0 + 1, Wp - 1)] * a1)

    r0, r1 = row(y0), row(y1)
    return ((((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


K = [F(0.9997878412794807), F(-0.3258083974640975), F(0.1555786518463281), F(-0.04432655554792128)]


def votes(img):
    """(v0, v1, h0) of every pixel of a level image: gamma-corrected gradient of the dominant channel, fastAtan2's polynomial, 9 unsigned
    bins with linear interpolation between neighbouring bins"""
    lut = tables()[0]
    g = lut[img]                                                       # (h, w, 3) float32
    pad = np.pad(g, ((1, 1), (1, 1), (0, 0)), mode="reflect")          # reflect-101
    dxs, dys = pad[1:-1, 2:] - pad[1:-1, :-2], pad[2:, 1:-1] - pad[:-2, 1:-1]
    dx, dy = dxs[..., 2].copy(), dys[..., 2].copy()
    m2 = dx * dx + dy * dy
    for c in (1, 0):
        n2 = dxs[..., c] * dxs[..., c] + dys[..., c] * dys[..., c]
        take = n2 > m2
        dx, dy, m2 = np.where(take, dxs[..., c], dx), np.where(take, dys[..., c], dy), np.where(take, n2, m2)
    mag = np.sqrt(m2)
    ax, ay = np.abs(dx), np.abs(dy)
    c = np.minimum(ax, ay) / (np.maximum(ax, ay) + F(np.finfo(np.float64).eps))
    c2 = c * c
    a = c * (K[0] + c2 * (K[1] + c2 * (K[2] + c2 * K[3])))
    a = np.where(ay > ax, F(np.pi / 2) - a, a)
    a = np.where(dx < 0, F(np.pi) - a, a)
    a = np.where(dy < 0, F(2 * np.pi) - a, a)
    pos = a * F(9.0 / np.pi) - F(0.5)
    fl = np.floor(pos)
    fr = pos - fl
    h0 = fl.astype(np.int64)
    h0 = np.where(h0 < 0, h0 + 9, h0)
    h0 = np.where(h0 >= 9, h0 - 9, h0)
    assert mag.dtype == F and fr.dtype == F
    return mag * (F(1) - fr), mag * fr, h0.astype(np.uint8)


def blocks(v0, v1, h0):
    """(nby, nbx, 36) float32: the 16 x 16 blocks every 8 pixels -- column sums inside a row, then the rows, then L2-Hys"""
    wt = tables()[2]
    h, w = v0.shape
    nby, nbx = h // 8 - 1, w // 8 - 1
    h1 = np.where(h0 == 8, 0, h0 + 1)
    hist = np.zeros((nby, nbx, 36), F)
    for b in range(9):
        vb = np.ascontiguousarray(np.where(h0 == b, v0, np.where(h1 == b, v1, F(0))).astype(F))
        win = np.lib.stride_tricks.as_strided(vb, (nby, nbx, 16, 16), (8 * w * 4, 8 * 4, w * 4, 4))
        for c in range(4):
            term = win * wt[c]                                         # (nby, nbx, i, j)
            rows = np.zeros((nby, nbx, 16), F)
            for j in range(16):
                rows = rows + term[..., j]
            s = np.zeros((nby, nbx), F)
            for i in range(16):
                s = s + rows[..., i]
            hist[..., c * 9 + b] = s

    def sumsq(v):
        s = np.zeros(v.shape[:2], F)
        for k in range(36):
            s = s + v[..., k] * v[..., k]
        return s

    sc1 = F(1) / (np.sqrt(sumsq(hist)) + F(3.6))
    u = np.minimum(hist * sc1[..., None], F(0.2))
    sc2 = F(1) / (np.sqrt(sumsq(u)) + F(1e-3))
    out = u * sc2[..., None]
    assert out.dtype == F
    return out


def scores(desc, det, stride):
    """(nwy, nwx) float32: s = rho + the sum over block columns of the sums over their blocks of the blocks' 36-term dot products"""
    nby, nbx = desc.shape[:2]
    sx, sy = stride[0] // 8, stride[1] // 8
    nwx, nwy = (nbx - 7) // sx + 1, (nby - 15) // sy + 1
    S = np.zeros((nwy, nwx), F)
    d = det[:DESC].reshape(7, 15, 36)
    for bx in range(7):
        Ccol = np.zeros((nwy, nwx), F)
        for by in range(15):
            sub = desc[by:by + (nwy - 1) * sy + 1:sy, bx:bx + (nwx - 1) * sx + 1:sx]
            T = np.zeros((nwy, nwx), F)
            for k in range(36):
                T = T + d[bx, by, k] * sub[..., k]
            Ccol = Ccol + T
        S = S + Ccol
    return det[DESC] + S


def similar(a, b):
    d = 0.2 * (min(a[2], b[2]) + min(a[3], b[3])) * 0.5
    return abs(a[0] - b[0]) <= d and abs(a[1] - b[1]) <= d and abs(a[0] + a[2] - b[0] - b[2]) <= d and abs(a[1] + a[3] - b[1] - b[3]) <= d


def group(rects, weights, threshold):
    """groupRectangles(rects, threshold, eps=0.2) with the weights' maxima: (rects, weights) as lists"""
    rects, weights = [tuple(int(v) for v in r) for r in rects], [float(w) for w in weights]
    if threshold < 1 or not rects:
        return rects, weights
    n, label, classes = len(rects), [-1] * len(rects), []
    for i in range(n):                                                 # connected components, named in the order of their lowest member
        if label[i] >= 0:
            continue
        label[i], todo, members = len(classes), [i], []
        while todo:
            a = todo.pop()
            members.append(a)
            for b in range(n):
                if label[b] < 0 and similar(rects[a], rects[b]):
                    label[b] = label[i]
                    todo.append(b)
        classes.append(sorted(members))
    mean, cnt, wmax = [], [], []
    for m in classes:
        s = F(1) / F(len(m))
        mean.append(tuple(int(np.rint(np.float64(F(sum(rects[i][k] for i in m)) * s))) for k in range(4)))
        cnt.append(len(m))
        wmax.append(max(weights[i] for i in m))
    out, wout = [], []
    for i, r1 in enumerate(mean):
        if cnt[i] <= threshold:
            continue
        for j, r2 in enumerate(mean):
            if j == i or cnt[j] <= threshold:
                continue
            dx, dy = int(np.rint(r2[2] * 0.2)), int(np.rint(r2[3] * 0.2))
            if (r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx and r1[1] + r1[3] <= r2[1] + r2[3] + dy
                    and (cnt[j] > max(3, cnt[i]) or cnt[i] < 3)):
                break
        else:
            out.append(r1)
            wout.append(wmax[i])
    return out, wout


def detector_of(det):
    det = np.asarray(det, F).reshape(-1)
    return np.concatenate([det, np.zeros(1, F)]) if det.size == DESC else det


def detect(pic, det, s, keep=True):
    """The whole rule over the oriented picture `pic`: a dict of every stage -- levels [(h, w, scale)], images, votes (v0, v1, h0), blocks,
    scores (per level), hits [(level, y, x)], hit_s, rects / weights (grouped); "overflow" when more than max_hits windows hit"""
    det = detector_of(det)
    lv = levels(pic.shape[0], pic.shape[1], s)
    out = dict(levels=lv, images=[], votes=[], blocks=[], scores=[], hits=[], hit_s=[], overflow=False)
    for n, (h, w, sc) in enumerate(lv):
        img = level_image(pic, h, w)
        v = votes(img)
        d = blocks(*v)
        sco = scores(d, det, s["win_stride"])
        if keep:
            out["images"].append(img), out["votes"].append(v), out["blocks"].append(d)
        out["scores"].append(sco)
        ys, xs = np.nonzero(sco.astype(np.float64) >= float(s["hit_threshold"]))       # row-major: the order (y, x)
        for y, x in zip(ys, xs):
            out["hits"].append((n, int(y) * s["win_stride"][1], int(x) * s["win_stride"][0]))
            out["hit_s"].append(sco[y, x])
    if len(out["hits"]) > s["max_hits"]:
        out["overflow"] = True
        return out
    raw = [(int(np.rint(x * lv[n][2])), int(np.rint(y * lv[n][2])), int(np.rint(64 * lv[n][2])), int(np.rint(128 * lv[n][2]))) for n, y, x in out["hits"]]
    out["raw_rects"] = raw
    out["rects"], out["weights"] = group(raw, [float(v) for v in out["hit_s"]], int(s["final_threshold"]))
    return out


# ---- the walk and the probe --------------------------------------------------------------------------------------------------------------
def frame_args(buf, lay):
    return [buf.ctypes.data_as(u8p), buf.size, lay["data_off"], lay["uv_off"], lay["format"], lay["H"], lay["W"], lay["sy"], lay["sx"], lay["sc"], lay["uv_stride"]]


def sizes_of(lay, o, s):
    """(levels, hw (n, 2), scales, geom (n, 4): nbx nby nwx nwy, totals: pixels blocks windows) from the library's level table"""
    n, hw, sc, geom, tot = C.c_int32(0), np.zeros((64, 2), np.int32), np.zeros(64), np.zeros((64, 4), np.int32), np.zeros(3, np.int64)
    rc = cpu_lib().hog_levels_c(o, lay["H"], lay["W"], *spec_args(s), C.byref(n), hw.ctypes.data_as(i32p), sc.ctypes.data_as(f64p),
                                geom.ctypes.data_as(i32p), tot.ctypes.data_as(i64p))
    assert rc == 0, rc
    return n.value, hw[:n.value], sc[:n.value], geom[:n.value], tot


def _outputs(tot, s):
    npix, nblk, nwin = (int(v) for v in tot)
    return dict(votes=np.zeros(2 * npix + 1, F), bins=np.zeros(npix + 1, np.uint8), blocks=np.zeros(36 * nblk + 1, F), scores=np.zeros(nwin + 1, F),
                hits=np.zeros(3 * s["max_hits"], np.int32), hit_s=np.zeros(s["max_hits"], F))


def walk(buf, lay, o, det, s, capacity=256):
    """g++'s walk -> (rc, dict: level_img, votes, bins, blocks, scores, hits (n, 3), hit_s, rects (n, 4), weights, count)"""
    det = np.ascontiguousarray(det, F)
    _, _, _, _, tot = sizes_of(lay, o, s)
    out = _outputs(tot, s)
    img = np.zeros(3 * int(tot[0]) + 1, np.uint8)
    nh, cnt = C.c_int32(-1), C.c_int32(-1)
    rects, ws = np.zeros((max(capacity, 1), 4), np.int32), np.zeros(max(capacity, 1))
    rc = cpu_lib().hog_walk(*frame_args(buf, lay), 0, o, *spec_args(s), det.ctypes.data_as(f32p), det.size, img.ctypes.data_as(u8p),
                            out["votes"].ctypes.data_as(f32p), out["bins"].ctypes.data_as(u8p), out["blocks"].ctypes.data_as(f32p),
                            out["scores"].ctypes.data_as(f32p), out["hits"].ctypes.data_as(i32p), out["hit_s"].ctypes.data_as(f32p), C.byref(nh),
                            rects.ctypes.data_as(i32p), ws.ctypes.data_as(f64p), capacity, C.byref(cnt))
    out["level_img"] = img[:-1]
    for k in ("votes", "bins", "blocks", "scores"):
        out[k] = out[k][:-1]
    n = max(nh.value, 0)
    out["hits"], out["hit_s"], out["count"] = out["hits"][:3 * n].reshape(n, 3), out["hit_s"][:n], cnt.value
    m = max(min(cnt.value, capacity), 0)
    out["rects"], out["weights"] = rects[:m], ws[:m]
    return rc, out


def probe(buf, lay, o, det, s):
    """the device probe -> (rc, dict: votes, bins, blocks, scores, hits, hit_s, count, launches, guard_damage); `buf` gets the device's bytes back"""
    det = np.ascontiguousarray(det, F)
    _, _, _, _, tot = sizes_of(lay, o, s)
    out = _outputs(tot, s)
    info = np.zeros(4, np.int64)
    rc = probe_lib().hp_detect(*frame_args(buf, lay), o, lay.get("uv_separate", 0), *spec_args(s), det.ctypes.data_as(f32p), det.size,
                               out["votes"].ctypes.data_as(f32p), out["bins"].ctypes.data_as(u8p), out["blocks"].ctypes.data_as(f32p),
                               out["scores"].ctypes.data_as(f32p), out["hits"].ctypes.data_as(i32p), out["hit_s"].ctypes.data_as(f32p),
                               info.ctypes.data_as(i64p))
    for k in ("votes", "bins", "blocks", "scores"):
        out[k] = out[k][:-1]
    n = int(info[3])
    out["hits"], out["hit_s"] = out["hits"][:3 * n].reshape(n, 3), out["hit_s"][:n]
    out["count"], out["launches"], out["guard_damage"] = int(info[0]), int(info[1]), int(info[2])
    return rc, out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def flat_ref(ref):
    """the numpy statement's stages laid out as the workspace lays them: level after level"""
    if not ref["levels"]:
        z = np.zeros(0, F)
        return dict(level_img=np.zeros(0, np.uint8), votes=z, bins=np.zeros(0, np.uint8), blocks=z, scores=z)
    return dict(level_img=np.concatenate([i.reshape(-1) for i in ref["images"]]),
                votes=np.concatenate([np.stack([v[0], v[1]], axis=-1).reshape(-1) for v in ref["votes"]]),
                bins=np.concatenate([v[2].reshape(-1) for v in ref["votes"]]),
                blocks=np.concatenate([b.reshape(-1) for b in ref["blocks"]]),
                scores=np.concatenate([x.reshape(-1) for x in ref["scores"]]))


def assert_stages_equal(got, ref, what, stages=("level_img", "votes", "bins", "blocks", "scores")):
    flat = flat_ref(ref)
    for k in stages:
        a, b = got[k], flat[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        same = np.array_equal(bits(a), bits(b)) if a.dtype == F else np.array_equal(a, b)
        assert same, (what, k, int(np.count_nonzero(a != b)), "values differ")
    assert [tuple(int(v) for v in r) for r in got["hits"]] == ref["hits"], (what, "hits")
    assert np.array_equal(bits(got["hit_s"]), bits(np.asarray(ref["hit_s"], F))), (what, "hit scores")


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def textured(H, W, seed=0):
    """a (H, W, 3) uint8 picture with structure at several scales (smooth blobs, an edge, noise): every stage has something to round"""
    rng = np.random.RandomState(seed + 3)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3))
    for c in range(3):
        img[..., c] = 120 + 70 * np.sin(xx / (5.0 + 2 * c) + c) * np.cos(yy / (7.0 + c)) + 25 * rng.randn(H, W)
    img[:, W // 3:W // 3 + 2] += 60
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def lay_from_picture(pic, lay, o):
    """the bytes of layout `lay` (tests/preview_ref.py's terms, BGR / RGB forms) whose oriented picture under code `o` is `pic`"""
    from tests import orient_ref
    buf = np.zeros(lay["size"], np.uint8)
    stored = orient_ref.stored_from_oriented(pic, o) if hasattr(orient_ref, "stored_from_oriented") else _unorient(pic, o)
    view = np.lib.stride_tricks.as_strided(buf[lay["data_off"]:], (lay["H"], lay["W"], 3), (lay["sy"], lay["sx"], lay["sc"]))
    view[...] = stored[:, :, ::-1] if lay["format"] == 1 else stored
    return buf


def _unorient(pic, o):
    """the stored frame whose picture under code o (np.rot90(frame, o & 3), mirrored when o & 4) is `pic`"""
    g = pic[:, ::-1] if o & 4 else pic
    return np.ascontiguousarray(np.rot90(g, -(o & 3)))


def packed(H, W):
    return P.plain_layout(H, W, 0)


def seeded_detector(seed=0, rho=0.0, scale=1.0):
    rng = np.random.RandomState(seed + 17)
    det = (rng.randn(DESC + 1) * scale).astype(F)
    det[DESC] = F(rho)
    return det


# ---- the planted figure (in the manner of tests/planted.py) -------------------------------------------------------------------------------
def figure(h=128, w=64):
    """a painted 'person' on mid grey: a dark head disc, a bright torso and two dark legs, with its own strong vertical and curved edges"""
    img = np.full((h, w, 3), 128, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    sy, sx = h / 128.0, w / 64.0
    head = (yy - 24 * sy) ** 2 / (10 * sy) ** 2 + (xx - 32 * sx) ** 2 / (9 * sx) ** 2 <= 1
    torso = (yy >= 36 * sy) & (yy < 80 * sy) & (np.abs(xx - 32 * sx) <= 13 * sx)
    legl = (yy >= 80 * sy) & (yy < 116 * sy) & (xx >= 20 * sx) & (xx < 29 * sx)
    legr = (yy >= 80 * sy) & (yy < 116 * sy) & (xx >= 35 * sx) & (xx < 44 * sx)
    img[head] = (40, 60, 90)
    img[torso] = (230, 200, 60)
    img[legl | legr] = (30, 30, 70)
    return img


def background(H, W, seed=0):
    """flat grey with mild texture: weak gradients everywhere, nothing figure-like"""
    rng = np.random.RandomState(seed + 29)
    return np.clip(128 + np.rint(6 * rng.randn(H, W, 3)), 0, 255).astype(np.uint8)


def planted_detector(rho_share=0.6):
    """det = the L2-normalised descriptor of the figure centred in a 64 x 128 window; rho = -rho_share * (its score on itself): a window
    scores above 0 only when its descriptor's projection on the figure's exceeds that share"""
    d = blocks(*votes(figure()))                                     # (15, 7, 36)
    v = np.transpose(d, (1, 0, 2)).reshape(-1).astype(np.float64)      # (bx, by, k): the descriptor's layout
    v = v / np.sqrt((v * v).sum())
    det = np.zeros(DESC + 1, F)
    det[:DESC] = v.astype(F)
    self_score = float((det[:DESC].astype(np.float64) * np.transpose(d, (1, 0, 2)).reshape(-1)).sum())
    det[DESC] = F(-rho_share * self_score)
    return det


PLANTED_SIZE = (360, 640)
PLANTED_FIGURES = [(40, 60, 1.0), (150, 330, 1.5)]                  # (y, x, size factor) of each figure's 64 x 128 cell
PLANTED_DECOY = (180, 60, 1.25, 73)                                 # the top 73 of a 160-row figure: head and half a torso -- a borderline case:
                                                                    # a window or two reach 0 there, too few to survive grouping


def planted_frame(H=PLANTED_SIZE[0], W=PLANTED_SIZE[1]):
    """(picture, [(x, y, w, h) of each painted figure's cell])"""
    pic = background(H, W)
    cells = []
    for y, x, f in PLANTED_FIGURES:
        h, w = int(round(128 * f)), int(round(64 * f))
        pic[y:y + h, x:x + w] = figure(h, w)
        cells.append((x, y, w, h))
    y, x, f, rows = PLANTED_DECOY
    pic[y:y + rows, x:x + int(round(64 * f))] = figure(int(round(128 * f)), int(round(64 * f)))[:rows]
    return pic, cells


def painted_extent(cell):
    """(x0, y0, x1, y1), inclusive: the part of a figure's cell that is painted -- head top to leg ends, torso edge to torso edge"""
    cx, cy, cw, ch = cell
    return cx + int(np.ceil(cw * 19 / 64.0)), cy + int(np.ceil(ch * 14 / 128.0)), cx + int(cw * 45 / 64.0), cy + int(np.ceil(ch * 116 / 128.0)) - 1
