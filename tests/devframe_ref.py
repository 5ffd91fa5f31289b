"""Frames in device memory: the tests' own numpy statement of what a slot must hold, and the case lists of the kernel tests
(tests/test_gpu_device_ingest_kernels.py runs them on the GPU; tests/test_device_frames_cpu.py asserts, without one, that they cover what
they claim and walks the same cases through g++'s build of vnect_amd/csrc/ingest.h).

The statement is a plain gather: channel c of pixel (y, x) is the byte at data + y * stride_y + x * stride_x + c * stride_c, the slot holds
those bytes as packed BGR rows, and an RGB source has channels 0 and 2 exchanged.  Nothing here imports vnect_amd."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
LIBDIR = os.path.join(ROOT, "vnect_amd", "lib")
u8p, i32p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)

PACKED3, PACKED4, PLANAR, GENERIC = 0, 1, 2, 3
FORMS = [PACKED3, PACKED4, PLANAR, GENERIC]
FORM_NAMES = ["packed3", "packed4", "planar", "generic"]
BGR, RGB = 0, 1
ORDERS = [BGR, RGB]

# ---- g++'s build of vnect_amd/csrc/ingest.h --------------------------------------------------------------------------------------------
_CPU = None


def cpu_lib():
    """libvnect_ingest.so (ingest.h behind ingest_capi.cpp), built on demand with plain g++."""
    global _CPU
    if _CPU is None:
        subprocess.check_call(["make", "-C", CSRC, "ingest"], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_ingest.so"))
        L.ingest_kernel_spans.argtypes = [i32p]
        L.ingest_classify.argtypes = [C.c_int64, C.c_int64]
        L.ingest_frame_span.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64]
        L.ingest_frame_span.restype = C.c_int64
        L.ingest_walk.argtypes = [u8p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int, u8p, u8p, i64p]
        L.ingest_walk.restype = C.c_int64
        L.ingest_store_walk.argtypes = [C.c_int, C.c_int, u8p, u8p]
        L.ingest_store_walk.restype = C.c_int64
        L.ingest_store_byte.argtypes = [C.c_int64]
        L.ingest_store_byte.restype = C.c_uint8
        _CPU = L
    return _CPU


def kernel_spans():
    """(pixels per lane, per wave, per workgroup of the coalesced kernels, per workgroup of the generic one) of the built kernels, from the
    shim (vnect_amd/csrc/ingest.h) -- not restated here."""
    out = (C.c_int32 * 4)()
    cpu_lib().ingest_kernel_spans(out)
    return tuple(out)


def load_probe():
    """libvnect_ingestprobe.so (the product's post.o and track.o behind vnect_amd/csrc/ingest_probe.hip), with its argument types: the kernel
    cases, and a device allocator, copies and streams for the surface tests"""
    f64p = C.POINTER(C.c_double)
    path = os.environ.get("VNECT_INGESTPROBE_LIB") or os.path.join(LIBDIR, "libvnect_ingestprobe.so")
    assert os.path.exists(path), "libvnect_ingestprobe.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    L = C.CDLL(path)
    L.ip_copy.argtypes = [u8p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, i32p, i32p, C.c_int,
                          C.c_int64, u8p, i32p]
    L.ip_copy_nv12.argtypes = [u8p, C.c_int64, C.c_int64, C.c_int64, u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, i32p, i32p,
                               C.c_int64, u8p, i32p]
    L.ip_pyramid.argtypes = [u8p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, i32p, f64p, C.c_int, C.c_int, C.c_void_p]
    L.ip_alloc.argtypes = [C.c_int64, C.POINTER(C.c_void_p)]
    L.ip_free.argtypes = [C.c_void_p]
    L.ip_range.argtypes = [C.c_void_p, i64p]
    L.ip_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.ip_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.ip_fill.argtypes = [C.c_void_p, C.c_int, C.c_int64]
    L.ip_stream_create.argtypes = [C.POINTER(C.c_void_p)]
    L.ip_stream_sync.argtypes = [C.c_void_p]
    L.ip_stream_destroy.argtypes = [C.c_void_p]
    L.ip_delayed_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double]
    lay = (C.c_int32 * 6)()
    L.ip_layout(lay)
    L.fill, L.guard = lay[0], lay[1]
    assert tuple(lay[2:6]) == kernel_spans()      # the probe and the CPU shim were built from one ingest.h
    return L


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
class Layout:
    """Where an (H, W) frame of 3 channels lies in a byte buffer: pixel (0, 0) channel 0 at byte `off`, the strides of its form with
    `pad` extra bytes per row.  The buffer ends with the frame's last byte (cap = off + span): a packed-4 frame's last pixel has no fourth
    byte, a planar frame's planes lie 3 bytes apart."""

    def __init__(self, form, H, W, off=0, pad=0):
        self.form, self.H, self.W, self.off, self.pad = form, H, W, off, pad
        if form == PACKED3:
            self.sx, self.sc, self.sy = 3, 1, 3 * W + pad
        elif form == PACKED4:
            self.sx, self.sc, self.sy = 4, 1, 4 * W + pad
        elif form == PLANAR:
            self.sx, self.sy = 1, W + pad
            self.sc = self.sy * H + 3
        else:                                      # channels two bytes apart, pixels five: no form's strides
            self.sx, self.sc, self.sy = 5, 2, 5 * W + pad
        self.span = (H - 1) * self.sy + (W - 1) * self.sx + 2 * self.sc + 1
        self.cap = off + self.span

    def view(self, buf):
        """the plain gather: the (H, W, 3) view of the frame's bytes in `buf`, channels in the source's order"""
        return np.lib.stride_tricks.as_strided(buf[self.off:], shape=(self.H, self.W, 3), strides=(self.sy, self.sx, self.sc))

    def place(self, pixels, seed=0):
        """`pixels` (H, W, 3), channels in the source's order, at this layout in a buffer of `cap` bytes; everything between and around
        the pixels is noise, not zeros (a kernel that takes a wrong stride reads wrong pixels, not a lucky blank)."""
        buf = np.random.default_rng(2000 + seed).integers(0, 256, self.cap, dtype=np.uint8)
        self.view(buf)[...] = pixels
        return buf

    def key(self):
        return (FORM_NAMES[self.form], self.H, self.W, self.off, self.pad)


def pixels(H, W, seed):
    """(H, W, 3) uniformly random bytes"""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def as_bgr(src_pixels, order):
    """what the slot must hold for pixels given in the source's channel order"""
    return src_pixels[..., ::-1] if order == RGB else src_pixels


def expected_region(bgr, rect, dst_cap, fill, guard, phase=0):
    """What a case's destination must hold after its launch: guard | phase canary bytes | the packed crop rows | canary up to dst_cap | guard."""
    x, y, w, h = rect
    out = np.full(guard + dst_cap + guard, fill, np.uint8)
    out[guard + phase:guard + phase + 3 * w * h] = np.ascontiguousarray(bgr[y:y + h, x:x + w]).reshape(-1)
    return out


# ---- the GPU case lists ----------------------------------------------------------------------------------------------------------------------
SMALL_HEIGHTS = [1, 2, 3, 5]
SMALL_OFFSETS = [0, 1, 2, 3]
SMALL_PADS = [0, 1, 5]


def small_widths(form):
    """1 .. 5 and 21, and one below, at and above what a wave and a workgroup of the form's kernel cover"""
    _, wave, wg, gwg = kernel_spans()
    ws = {1, 2, 3, 4, 5, 21}
    for s in ((gwg,) if form == GENERIC else (wave, wg)):
        ws |= {s - 1, s, s + 1}
    return sorted(ws)


def small_layouts(form):
    return [Layout(form, H, W, off, pad) for H in SMALL_HEIGHTS for W in small_widths(form) for off in SMALL_OFFSETS for pad in SMALL_PADS]


def crop_frame(form):
    return Layout(form, 6, 40, off=1, pad=5)


def crop_rects():
    """every x 0..7 and w 1..12 (both row ends on every dword phase of every form), two origins and heights in y: 384"""
    return [(x, y, w, h) for x in range(8) for w in range(1, 13) for y in (0, 1) for h in (1, 3)]


EDGE_HEIGHTS = [1, 3]


def edge_widths(form):
    _, wave, _, gwg = kernel_spans()
    return [1, 2, 3, 5, 7, 21, (gwg if form == GENERIC else wave) + 1]


def edge_layouts(form):
    """(layout, flush_end): frames whose first byte is their allocation's first (offset 0) and frames whose last byte is its last (every
    offset, so the end falls on every dword phase)"""
    out = []
    for H in EDGE_HEIGHTS:
        for W in edge_widths(form):
            out.append((Layout(form, H, W, 0, 1), 0))
            for off in range(4):
                out.append((Layout(form, H, W, off, 1), 1))
    return out


SEAM_HEIGHTS = list(range(65531, 65541))     # around the 16-bit grid.y: the launch splits into chunks of 65 535 rows
SEAM_WIDTHS = [1, 2]
TRACK_MAX_ROWS = 65535                        # the tracked kernels' grid covers the whole frame in one launch

PYRAMID_CASE = (480, 640, (101, 53, 333, 271))   # (H, W, rect), as tests/nv12_ref.py's first


# ---- a stand-in for a device array -----------------------------------------------------------------------------------------------------------
class FakeCuda:
    """An object with __cuda_array_interface__ and nothing else: what the Python layer must be content with (no torch)."""

    def __init__(self, ptr, shape, strides=None, typestr="|u1"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3,
                                         "strides": None if strides is None else tuple(strides)}
