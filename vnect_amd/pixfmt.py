"""NV12 <-> BGR in numpy, for users and fixtures.

An NV12 frame of H x W pixels (both even) is a uint8 array of ``H * 3 // 2`` rows of W bytes: H rows of Y, then H / 2 rows of
interleaved U, V, one (U, V) pair per 2 x 2 pixels.

* ``nv12_to_bgr`` is what the device computes inside the frame's copy (vnect_amd/csrc/nv12.h): the integer arithmetic of OpenCV's
  ``cv2.cvtColor(nv12, cv2.COLOR_YUV2BGR_NV12)`` -- BT.601 limited range in 20-bit fixed point, chroma replicated, not interpolated.
* ``bgr_to_nv12`` is the BT.601 limited-range forward transform with 2 x 2 chroma averaging: a generator of plausible inputs.
  Nothing is held to it.
"""
import numpy as np

# OpenCV's fixed-point BT.601 coefficients (20 fractional bits)
_SHIFT = 20
_CY, _CUB, _CUG, _CVG, _CVR = 1220542, 2116026, -409993, -852492, 1673527


def _split(nv12):
    a = np.asarray(nv12)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] % 3 or a.shape[1] % 2 or a.shape[0] < 3:
        raise ValueError("an NV12 frame must be a uint8 (H * 3 // 2, W) array with even H and W")
    H = a.shape[0] * 2 // 3
    if H % 2:
        raise ValueError("an NV12 frame needs an even H")
    return a[:H], a[H:], H, a.shape[1]


def nv12_to_bgr(nv12):
    """(H * 3 // 2, W) uint8 NV12 -> (H, W, 3) uint8 BGR."""
    yp, uvp, H, W = _split(nv12)
    y = np.maximum(yp.astype(np.int32) - 16, 0) * _CY + (1 << (_SHIFT - 1))
    u = np.repeat(np.repeat(uvp[:, 0::2].astype(np.int32) - 128, 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uvp[:, 1::2].astype(np.int32) - 128, 2, axis=0), 2, axis=1)
    out = np.empty((H, W, 3), np.uint8)
    out[..., 0] = np.clip((y + _CUB * u) >> _SHIFT, 0, 255)
    out[..., 1] = np.clip((y + _CVG * v + _CUG * u) >> _SHIFT, 0, 255)
    out[..., 2] = np.clip((y + _CVR * v) >> _SHIFT, 0, 255)
    return out


def bgr_to_nv12(bgr):
    """(H, W, 3) uint8 BGR, H and W even -> (H * 3 // 2, W) uint8 NV12 (BT.601 limited range, chroma averaged over 2 x 2)."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] % 2 or a.shape[1] % 2 or a.size == 0:
        raise ValueError("bgr must be a uint8 (H, W, 3) array with even H and W")
    H, W = a.shape[:2]
    b, g, r = (a[..., k].astype(np.float64) for k in range(3))
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    cb = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    cr = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    out = np.empty((H * 3 // 2, W), np.uint8)
    out[:H] = np.clip(np.rint(y), 16, 235)
    mean = lambda c: c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))  # noqa: E731
    out[H:, 0::2] = np.clip(np.rint(mean(cb)), 16, 240)
    out[H:, 1::2] = np.clip(np.rint(mean(cr)), 16, 240)
    return out
