// nv12.h -- NV12 -> BGR, ONE source for host and device (as crop.h and axis.h are for the crop and the resize tables).
// The arithmetic is OpenCV's cv2.cvtColor(nv12, cv2.COLOR_YUV2BGR_NV12): BT.601 limited range in 20-bit fixed point (imgproc's
// color_yuv: ITUR_BT_601_CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, rounding term 1 << 19), chroma
// replicated over its 2 x 2 pixels.  The reference takes its frames from camera_capture.read() (run_estimator_ps.py:79,109), which
// hands out BGR that OpenCV itself converted from what the decoder delivered: colour conversion is OpenCV's, not the reference's own
// code, so OpenCV's integers are what a user of the reference gets.  Every intermediate fits int32 (largest magnitude over all 2^24
// triples: 560 969 128).  `>>` on a negative sum is an arithmetic shift (floor) with every compiler this is built with.
// HIP-free when compiled by g++ (nv12_capi.cpp: tests/test_nv12_cpu.py holds it to a numpy restatement over all triples).
#pragma once
#include <stdint.h>

#include "axis.h"  // VNECT_HD

namespace vnect {

// What the kernels of post.hip cover (nv12_strip): a lane converts the 4 pixels of one aligned group of absolute frame columns
// 4 G .. 4 G + 3 in both rows of a chroma row, a wave 64 consecutive groups, a workgroup four waves.  The first group of a crop is
// (x >> 2), so the seams between waves and workgroups lie at these distances from column (x & ~3).
constexpr int NV12_LANE_PX = 4;
constexpr int NV12_WAVE_PX = 64 * NV12_LANE_PX;
constexpr int NV12_WG_PX = 4 * NV12_WAVE_PX;

// The clamped channel goes through an empty asm on the device, so that the compiler sees an opaque value and not a shift-and-saturate
// it can pair up: hipcc for gfx950 fuses two of them and the `| << 8` behind them into one v_ashr_pk_u8_i32 and then uses the
// register as if its upper 16 bits were zero, while the instruction leaves there what the destination register held before (seen on
// an MI355X: bytes 2 and 3 of a group's first dword came out OR-ed with the upper half of the green channel's unshifted sum).  The
// arithmetic is unchanged; tests/test_gpu_nv12_kernels.py is what notices if a compiler finds another way to the same instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#define VNECT_NV12_OPAQUE(v) asm volatile("" : "+v"(v))
#else
#define VNECT_NV12_OPAQUE(v) (void)0
#endif
VNECT_HD int nv12_clamp8(int v)
{
    int c = v < 0 ? 0 : (v > 255 ? 255 : v);
    VNECT_NV12_OPAQUE(c);
    return c;
}

// one pixel: (Y, U, V) -> bgr[0..2]
VNECT_HD void nv12_pixel(int Y, int U, int V, int* bgr)
{
    const int y = (Y > 16 ? Y - 16 : 0) * 1220542 + 524288, u = U - 128, v = V - 128;
    bgr[0] = nv12_clamp8((y + 2116026 * u) >> 20);
    bgr[1] = nv12_clamp8((y - 852492 * v - 409993 * u) >> 20);
    bgr[2] = nv12_clamp8((y + 1673527 * v) >> 20);
}

// Four horizontally adjacent pixels that start at an even column, from one dword of the Y row (bytes Y0 Y1 Y2 Y3, little endian) and
// the dword of the UV row under it (U0 V0 U1 V1): pixels 0, 1 take (U0, V0), pixels 2, 3 (U1, V1).  out: the 12 packed bytes
// B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3 as three little-endian dwords.
VNECT_HD void nv12_quad(uint32_t y4, uint32_t uv4, uint32_t* out)
{
    uint32_t b[12];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int p = 0; p < 4; p++) {
        const int sh = (p >> 1) * 16;
        int c[3];
        nv12_pixel((int)((y4 >> (8 * p)) & 255u), (int)((uv4 >> sh) & 255u), (int)((uv4 >> (sh + 8)) & 255u), c);
        b[3 * p] = (uint32_t)c[0], b[3 * p + 1] = (uint32_t)c[1], b[3 * p + 2] = (uint32_t)c[2];
    }
    out[0] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
    out[1] = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
    out[2] = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
}

}  // namespace vnect
