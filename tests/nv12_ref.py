"""The tests' own statement of NV12 -> BGR, and the case lists of the NV12 kernel tests (tests/test_gpu_nv12_kernels.py runs them on the
GPU; tests/test_nv12_cpu.py asserts, without one, that they cover what they claim).

`restate` is written from the specification -- BT.601 limited range in OpenCV's 20-bit fixed point, chroma replicated:

    y = max(0, Y - 16) * 1220542,  u = U - 128,  v = V - 128
    B = clamp((y + 524288 + 2116026 u) >> 20),  G = clamp((y + 524288 - 852492 v - 409993 u) >> 20),  R = clamp((y + 524288 + 1673527 v) >> 20)

with `>>` as a floor -- and imports nothing from vnect_amd: vnect_amd/pixfmt.py and vnect_amd/csrc/nv12.h are both held to it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
LIBDIR = os.path.join(ROOT, "vnect_amd", "lib")
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((126, 128, 128), (128, 128, 128)), ((81, 90, 240), (0, 0, 254)),
         ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255)),
         ((255, 0, 0), (20, 255, 74)), ((0, 255, 255), (255, 0, 203))]


def restate_yuv(Y, U, V):
    """(Y, U, V) integer arrays of one shape -> (..., 3) uint8 BGR.  int64 throughout, floor division for the shift."""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    y = np.maximum(Y - 16, 0) * 1220542 + 524288
    u, v = U - 128, V - 128
    chans = [y + 2116026 * u, y - 852492 * v - 409993 * u, y + 1673527 * v]
    return np.stack([np.clip(np.floor_divide(c, 1 << 20), 0, 255) for c in chans], axis=-1).astype(np.uint8)


def restate(nv12):
    """(H * 3 // 2, W) uint8 NV12 -> (H, W, 3) uint8 BGR."""
    a = np.asarray(nv12)
    assert a.dtype == np.uint8 and a.ndim == 2 and a.shape[0] % 3 == 0 and a.shape[1] % 2 == 0
    H, W = a.shape[0] * 2 // 3, a.shape[1]
    rows, cols = np.arange(H)[:, None] >> 1, (np.arange(W)[None, :] >> 1) * 2
    return restate_yuv(a[:H], a[H:][rows, cols], a[H:][rows, cols + 1])


def float_form(Y, U, V, c=(1.164, 2.018, 0.391, 0.813, 1.596)):
    """The rounded float form with OpenCV's documented coefficients (the sanity check that the fixed-point constants are the right ones)."""
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    y = c[0] * np.maximum(Y - 16, 0)
    chans = [y + c[1] * (U - 128), y - c[3] * (V - 128) - c[2] * (U - 128), y + c[4] * (V - 128)]
    return np.stack([np.clip(np.rint(ch), 0, 255) for ch in chans], axis=-1).astype(np.int64)


# ---- g++'s build of vnect_amd/csrc/nv12.h -------------------------------------------------------------------------------------------------
_CPU = None


def cpu_lib():
    """libvnect_nv12.so (nv12.h behind nv12_capi.cpp), built on demand with plain g++."""
    global _CPU
    if _CPU is None:
        subprocess.check_call(["make", "-C", CSRC, "nv12"], stdout=subprocess.DEVNULL)
        L = C.CDLL(os.path.join(LIBDIR, "libvnect_nv12.so"))
        L.nv12_kernel_spans.argtypes = [i32p]
        L.nv12_pixels.argtypes = [u8p, C.c_int64, u8p]
        L.nv12_plane_pixel.argtypes = [C.c_int, u8p]
        L.nv12_plane_quad.argtypes = [C.c_int, u8p]
        L.nv12_plane_quad.restype = C.c_int64
        L.nv12_convert.argtypes = [u8p, C.c_int64, u8p, C.c_int64] + [C.c_int] * 6 + [u8p]
        _CPU = L
    return _CPU


def kernel_spans():
    """(pixels per lane, per wave, per workgroup) of the built kernels, from the shim (vnect_amd/csrc/nv12.h) -- not restated here."""
    out = (C.c_int32 * 3)()
    cpu_lib().nv12_kernel_spans(out)
    return tuple(out)


# ---- content ---------------------------------------------------------------------------------------------------------------------------------
def smooth_bgr(H, W, seed):
    """A random smooth BGR image: an 8 x 8 grid of random colours, bilinearly upsampled (in gamut, nothing clipped)."""
    g = np.random.default_rng(seed).uniform(20, 235, (9, 9, 3))
    ys, xs = np.linspace(0, 8, H, endpoint=False), np.linspace(0, 8, W, endpoint=False)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    img = (g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx) * (1 - fy) + (g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx) * fy
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def content(H, W, seed):
    """An (H * 3 // 2, W) NV12 image: even seeds uniformly random bytes (about 85 % of such triples saturate a channel: both clamps and
    max(0, Y - 16) are exercised), odd seeds bgr_to_nv12 of a random smooth image (in gamut)."""
    if seed % 2 == 0:
        return np.random.default_rng(seed).integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
    from vnect_amd import pixfmt
    return pixfmt.bgr_to_nv12(smooth_bgr(H, W, seed))


class Layout:
    """Where an (H, W) NV12 image lies in a byte buffer: Y plane at y_off, rows ys apart; UV plane at uv_off, rows uvs apart."""

    def __init__(self, H, W, y_off, ys, uv_off=None, uvs=None):
        self.H, self.W, self.y_off, self.ys = H, W, y_off, ys
        self.uv_off = y_off + H * ys if uv_off is None else uv_off      # None: directly behind the Y rows, same stride
        self.uvs = ys if uvs is None else uvs
        self.behind = uv_off is None
        self.cap = max(self.y_off + (H - 1) * self.ys + W, self.uv_off + (H // 2 - 1) * self.uvs + W)

    def place(self, nv12, seed=0):
        """The image's bytes at this layout in a buffer of `cap` bytes; everything between and around the rows is noise, not zeros (a
        kernel that takes a wrong stride or plane reads wrong pixels, not a lucky blank)."""
        buf = np.random.default_rng(1000 + seed).integers(0, 256, self.cap, dtype=np.uint8)
        for r in range(self.H):
            buf[self.y_off + r * self.ys:self.y_off + r * self.ys + self.W] = nv12[r]
        for r in range(self.H // 2):
            buf[self.uv_off + r * self.uvs:self.uv_off + r * self.uvs + self.W] = nv12[self.H + r]
        return buf

    def key(self):
        return (self.H, self.W, self.y_off, self.ys, self.uv_off, self.uvs)


# ---- the GPU case lists ------------------------------------------------------------------------------------------------------------------
FRAME_HEIGHTS = [2, 4, 6]
FRAME_STRIDE_PADS = [0, 2, 13]
FRAME_Y_OFFSETS = [0, 1, 2, 3]


def frame_widths():
    """The whole-frame widths: the small ones, the ones around 256 / 1024 / 2048, and whatever the built kernel's wave and workgroup
    cover, two pixels either side."""
    _, wave, wg = kernel_spans()
    ws = set(range(2, 20, 2)) | {254, 256, 258, 1022, 1024, 1026, 2050}
    for s in (wave, wg):
        ws |= {s - 2, s, s + 2}
    return sorted(ws)


def frame_layouts(H):
    """Every whole-frame layout of height H: width x stride pad x Y base offset x (UV directly behind | UV apart with its own stride)."""
    out = []
    for W in frame_widths():
        for pad in FRAME_STRIDE_PADS:
            for off in FRAME_Y_OFFSETS:
                ys = W + pad
                out.append(Layout(H, W, off, ys))
                y_end = off + (H - 1) * ys + W
                out.append(Layout(H, W, off, ys, uv_off=y_end + 5 + 2 * off, uvs=W + 6 - pad % 4))
    return out


def frame_seed(k, H):
    """Content seed of layout k of frame_layouts(H).  Layouts come in pairs (UV behind, UV apart) that share a seed, and the seed's
    parity -- random bytes or a smooth picture -- alternates from pair to pair: both kinds of content reach both placements."""
    return k // 2 + H


CROP_FRAME = Layout(12, 32, 1, 32 + 13, uv_off=1 + 11 * 45 + 32 + 6, uvs=32 + 6)   # odd Y stride, Y base at byte 1, UV plane apart


def crop_rects():
    """Every crop x 0..7, y 0..3, w 1..9, h 1..5 of the 32 x 12 frame: 1 440."""
    return [(x, y, w, h) for x in range(8) for y in range(4) for w in range(1, 10) for h in range(1, 6)]


WIDE_FRAME = Layout(6, 2052, 3, 2052 + 2)
WIDE_RECTS = [(1, 1, 2049, 4), (3, 0, 1025, 5), (1021, 1, 9, 3)]
TALL_FRAME = Layout(131080, 2, 0, 2)           # more chroma rows than one grid's 65 535: launch_nv12_copy splits
TALL_RECTS = [(0, 0, 2, 131080), (1, 131069, 1, 11)]

PYRAMID_CASES = [(480, 640, (101, 53, 333, 271)), (2160, 4096, (1001, 501, 2001, 1501))]   # (H, W, rect); the second in fp32 only


def expected_region(bgr, rect, dst_cap, fill, guard):
    """What a case's destination must hold after its launch: guard | the packed crop rows | canary up to dst_cap | guard."""
    x, y, w, h = rect
    out = np.full(guard + dst_cap + guard, fill, np.uint8)
    out[guard:guard + 3 * w * h] = np.ascontiguousarray(bgr[y:y + h, x:x + w]).reshape(-1)
    return out
