"""Orientation: the tests' own numpy statement of the rule, and the case lists of the kernel tests (tests/test_gpu_orient_kernels.py runs
them on the GPU; tests/test_orient_cpu.py asserts, without one, that they cover what they claim and walks the same cases through g++'s
build of vnect_amd/csrc/orient.h).

The statement is two lines: the oriented picture of a stored frame f under code o is np.rot90(f, o & 3), mirrored ([:, ::-1]) when
o & 4.  Nothing here shares code with orient.h, and nothing imports vnect_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import devframe_ref as dr
from . import nv12_ref

ROOT, CSRC, LIBDIR = dr.ROOT, dr.CSRC, dr.LIBDIR
u8p, i32p, i64p = dr.u8p, dr.i32p, dr.i64p
CODES = list(range(1, 8))
NV12 = 4                                     # the source form behind devframe_ref's four
FORM_NAMES = dr.FORM_NAMES + ["nv12"]


def oriented(f, o):
    """THE RULE: the oriented picture of the stored frame `f` (a view)"""
    g = np.rot90(f, o & 3)
    if o & 4:
        g = g[:, ::-1]
    return g


def oriented_size(o, H, W):
    return (W, H) if o & 1 else (H, W)


def index_map(o, H, W):
    """(Ho, Wo, 2) int array: the stored (row, column) of every oriented pixel, by THE RULE applied to an array of indices"""
    rc = np.stack(np.meshgrid(np.arange(H), np.arange(W), indexing="ij"), axis=-1)
    return np.ascontiguousarray(oriented(rc, o))


def src_rect(o, H, W, rect):
    """brute force: the stored rectangle (x, y, w, h) an oriented crop reads, from the index map"""
    x, y, w, h = rect
    m = index_map(o, H, W)[y:y + h, x:x + w].reshape(-1, 2)
    r0, c0, r1, c1 = m[:, 0].min(), m[:, 1].min(), m[:, 0].max(), m[:, 1].max()
    assert (r1 - r0 + 1) * (c1 - c0 + 1) == w * h          # a rectangle again
    return (int(c0), int(r0), int(c1 - c0 + 1), int(r1 - r0 + 1))


# ---- g++'s build of vnect_amd/csrc/orient.h ----------------------------------------------------------------------------------------------
_CPU = None


def cpu_lib():
    """libvnect_orient.so (orient.h behind orient_capi.cpp), built on demand with plain g++."""
    global _CPU
    if _CPU is None:
        subprocess.check_call(["make", "-C", CSRC, "orient"], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_orient.so"))
        L.orient_kernel_spans.argtypes = [i32p]
        L.orient_size_c.argtypes = [C.c_int] * 3 + [i32p]
        L.orient_map_c.argtypes = [C.c_int] * 5 + [i32p]
        L.orient_src_rect_c.argtypes = [C.c_int] * 7 + [i32p]
        L.orient_walk.argtypes = [u8p, C.c_int64, C.c_int64, u8p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64] + \
            [C.c_int] * 7 + [u8p, u8p, i64p, i64p]
        L.orient_walk.restype = C.c_int64
        _CPU = L
    return _CPU


def kernel_spans():
    """(tile edge, threads, LDS row pitch in dwords, LDS dwords) of the built kernels, from the shim -- not restated here."""
    out = (C.c_int32 * 4)()
    cpu_lib().orient_kernel_spans(out)
    return tuple(out)


def tile():
    return kernel_spans()[0]


def load_probe():
    """libvnect_orientprobe.so (the product's orient.o behind vnect_amd/csrc/orient_probe.hip), with its argument types"""
    path = os.environ.get("VNECT_ORIENTPROBE_LIB") or os.path.join(LIBDIR, "libvnect_orientprobe.so")
    assert os.path.exists(path), "libvnect_orientprobe.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    L = C.CDLL(path)
    L.op_copy.argtypes = [u8p, C.c_int64, C.c_int64, u8p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                          C.c_int, C.c_int, C.c_int, C.c_int, i32p, i32p, C.c_int, C.c_int64, u8p, i32p]
    lay = (C.c_int32 * 3)()
    L.op_layout(lay)
    L.fill, L.guard = lay[0], lay[1]
    assert lay[2] == tile()                        # the probe and the CPU shim were built from one orient.h
    return L


# ---- sources -----------------------------------------------------------------------------------------------------------------------------
class Source:
    """A stored (H, W) frame in one of the five forms, in exactly sized buffers (the frame's last byte is the buffer's last; `off` bytes
    of slack in front), and the BGR picture it holds.  NV12: `two` = the UV plane in a buffer of its own."""

    def __init__(self, form, order, H, W, off=0, pad=0, two=False, seed=0):
        self.form, self.order, self.H, self.W, self.off, self.two = form, order, H, W, off, two
        if form == NV12:
            assert H % 2 == 0 and W % 2 == 0
            img = nv12_ref.content(H, W, 2 * seed)                   # (even seeds: random bytes, both clamps at work)
            self.sy, self.sx, self.sc = W + pad, 1, W + (pad and pad + 2)
            span0, span1 = (H - 1) * self.sy + W, (H // 2 - 1) * self.sc + W
            rng = np.random.default_rng(3000 + seed)
            self.buf0 = rng.integers(0, 256, off + span0 + (0 if two else off + span1), dtype=np.uint8)
            self.buf1 = rng.integers(0, 256, off + span1, dtype=np.uint8) if two else None
            self.off0, self.off1 = off, off if two else off + span0 + off
            uvb = self.buf1 if two else self.buf0
            for r in range(H):
                self.buf0[off + r * self.sy:off + r * self.sy + W] = img[r]
            for r in range(H // 2):
                uvb[self.off1 + r * self.sc:self.off1 + r * self.sc + W] = img[H + r]
            self.bgr = nv12_ref.restate(img)
        else:
            lay = dr.Layout(form, H, W, off, pad)
            px = dr.pixels(H, W, 100 + seed)
            self.sy, self.sx, self.sc = lay.sy, lay.sx, lay.sc
            self.buf0, self.buf1, self.off0, self.off1 = lay.place(px, seed), None, off, 0
            self.bgr = np.ascontiguousarray(dr.as_bgr(px, order))

    def picture(self, o):
        """the oriented BGR picture, contiguous"""
        return np.ascontiguousarray(oriented(self.bgr, o))

    def key(self):
        return (FORM_NAMES[self.form], self.order, self.H, self.W, self.off, self.two)


def walk(src, o, rect, phase=0):
    """the host walk of one case -> (crop bytes (h, w, 3), hits, seen[4], stray, shared_whole)"""
    L = cpu_lib()
    x, y, w, h = rect
    n = 3 * w * h
    blk = np.full(phase + n, 0xC7, np.uint8)
    hits = np.zeros(n, np.uint8)
    seen, shared = (C.c_int64 * 4)(), C.c_int64(-1)
    b1 = src.buf1
    stray = L.orient_walk(src.buf0.ctypes.data_as(u8p), src.buf0.size, src.off0, None if b1 is None else b1.ctypes.data_as(u8p),
                          0 if b1 is None else b1.size, src.off1, src.form, src.order, src.sy, src.sx, src.sc, o, src.H, src.W, x, y, w, h,
                          blk[phase:].ctypes.data_as(u8p), hits.ctypes.data_as(u8p), seen, C.byref(shared))
    return blk[phase:].reshape(h, w, 3), hits, tuple(seen), int(stray), int(shared.value), blk[:phase]


def expected_region(pic, rect, dst_cap, fill, guard, phase=0):
    """What a case's destination must hold after its launch: guard | phase canary bytes | the packed crop rows | canary up to dst_cap | guard."""
    return dr.expected_region(pic, rect, dst_cap, fill, guard, phase)


# ---- the GPU case lists ------------------------------------------------------------------------------------------------------------------
def seam_sizes():
    """1, T - 1, T, T + 1, 2 T + 1: every one of them in each axis, in five (H, W) pairs"""
    T = tile()
    return [(1, T - 1), (T - 1, T), (T, T + 1), (T + 1, 2 * T + 1), (2 * T + 1, 1)]


def seam_sizes_nv12():
    """the even neighbours"""
    T = tile()
    return [(2, T - 2), (T - 2, T), (T, T + 2), (T + 2, 2 * T + 2), (2 * T + 2, 2)]


def seam_rects(Ho, Wo):
    """of an (Ho, Wo) picture: the whole, crops at odd origins whose far edge falls before, on and after every tile seam counted from the
    crop's origin, and 1 x 1, 1 x w and h x 1 crops"""
    T = tile()
    out = [(0, 0, Wo, Ho)]
    for x, y in ((1, 1), (3, 1)):
        for w in (T - 1, T, T + 1, 2 * T - 1, 2 * T):
            if x + w <= Wo and y + 1 <= Ho:
                out.append((x, y, w, min(3, Ho - y)))
        for h in (T - 1, T, T + 1, 2 * T - 1, 2 * T):
            if y + h <= Ho and x + 1 <= Wo:
                out.append((x, y, min(3, Wo - x), h))
    out += [(0, 0, 1, 1), (Wo - 1, Ho - 1, 1, 1), (Wo // 2, Ho // 2, 1, 1), (0, Ho // 2, Wo, 1), (Wo // 2, 0, 1, Ho)]
    return sorted(set(out))


def gpu_cases():
    """(source arguments, code, phase, flush_end) of every kernel case group: codes 1 .. 7 x the four BGR / RGB forms x both orders and NV12
    in one and in two allocations, over the seam sizes; source slack, destination phase and the end the frame is flush with go round"""
    out, k = [], 0
    for o in CODES:
        for form in range(4):
            for order in (0, 1):
                for (H, W) in seam_sizes():
                    out.append((dict(form=form, order=order, H=H, W=W, off=k % 4, pad=(0, 1, 5)[k % 3], seed=k), o, (k // 2) % 4, (k // 3) % 2))
                    k += 1
        for two in (False, True):
            for (H, W) in seam_sizes_nv12():
                out.append((dict(form=NV12, order=0, H=H, W=W, off=k % 4, pad=(0, 2, 6)[k % 3], two=two, seed=k), o, (k // 2) % 4, (k // 3) % 2))
                k += 1
    return out
