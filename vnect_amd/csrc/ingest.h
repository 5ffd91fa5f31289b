// ingest.h -- a uint8 frame that already lies in DEVICE memory -> packed BGR rows of a resident frame slot: the per-lane window arithmetic,
// ONE source for host and device (as nv12.h and crop.h are).  The kernels of post.hip (ingest_copy_kernel and its tracked twin) and the
// host walk of ingest_capi.cpp (tests/test_device_frames_cpu.py, and the sanitizer sweep) call the same functions: which source dwords a
// lane loads, how a dword that an allocation's edge cuts is read, the byte permute, and which destination bytes the lane owns.
// There is nothing of the reference here: it reads its frame on the host (src/estimator.py:97-99) and crops it with a numpy slice
// (run_estimator_ps.py:88).  HIP-free when compiled by g++.
//
// A source is three byte strides (stride_y, stride_x, stride_c) and a channel order.  A lane owns one GROUP: the four pixels 4 G .. 4 G + 3
// of a crop row (G counted from the crop's first column), 12 destination bytes.  What it loads depends on the form:
//   packed-3  (stride_x 3, stride_c 1): 12 bytes at row + 12 G -- three dwords of one stream;
//   packed-4  (stride_x 4, stride_c 1): 16 bytes at row + 16 G -- four dwords of one stream, every fourth byte dropped;
//   planar    (stride_x 1):             4 bytes at row + c stride_c + 4 G -- one dword of each of three streams.
// A stream's bytes start at any alignment `sh` of the dword grid, the same for every lane of the row: the lane loads the ND ALIGNED dwords
// that hold its first bytes (a wave: 64 ND consecutive dwords) and takes the one behind them from lane + 1 through a shuffle (the last
// lane of a wave or of the row loads it itself), and a funnel shift by `sh` bytes gives the payload.  Any other strides: the generic
// kernel, one pixel per lane with byte loads -- slow, simple, and what the three forms above must equal.
#pragma once
#include <stdint.h>
#include <string.h>

#include "axis.h"  // VNECT_HD

namespace vnect {

enum { INGEST_PACKED3 = 0, INGEST_PACKED4 = 1, INGEST_PLANAR = 2, INGEST_GENERIC = 3 };
enum { INGEST_BGR = 0, INGEST_RGB = 1 };  // the source's channel order (RGB: channels 0 and 2 change places on the way)

constexpr int INGEST_LANE_PX = 4;
constexpr int INGEST_WAVE_PX = 64 * INGEST_LANE_PX;
constexpr int INGEST_WG_PX = 4 * INGEST_WAVE_PX;
constexpr int INGEST_GENERIC_WG_PX = 256;  // the generic kernel: one pixel per lane, 256 lanes

VNECT_HD int ingest_form(long long stride_x, long long stride_c)
{
    if (stride_x == 3 && stride_c == 1) return INGEST_PACKED3;
    if (stride_x == 4 && stride_c == 1) return INGEST_PACKED4;
    if (stride_x == 1 && stride_c >= 1) return INGEST_PLANAR;
    return INGEST_GENERIC;
}
VNECT_HD int ingest_streams(int form) { return form == INGEST_PLANAR ? 3 : 1; }
// aligned dwords of one stream that hold a group's first bytes
VNECT_HD int ingest_dwords(int form) { return form == INGEST_PACKED3 ? 3 : (form == INGEST_PACKED4 ? 4 : 1); }
// bytes of one stream that a crop row of w pixels needs, from the stream's first (packed-4: the last pixel's fourth byte is not needed,
// and may lie outside the allocation)
VNECT_HD long long ingest_row_need(int form, int w) { return form == INGEST_PACKED3 ? 3LL * w : (form == INGEST_PACKED4 ? 4LL * w - 1 : (long long)w); }
// bytes from pixel (0, 0) channel 0 to the end of the last byte of an (H, W) frame: what must lie inside the allocation
VNECT_HD long long ingest_span(int H, int W, long long sy, long long sx, long long sc) { return (long long)(H - 1) * sy + (long long)(W - 1) * sx + 2 * sc + 1; }

// the four bytes at byte `sh` (0 .. 4) of the dword pair (hi, lo)
VNECT_HD uint32_t ingest_funnel(uint32_t hi, uint32_t lo, int sh) { return (uint32_t)((((unsigned long long)hi << 32) | lo) >> (8 * sh)); }

// The LOAD BOUNDS.  [need_lo, need_end): the row's bytes of this stream; [lo, end): the allocation the frame lies in (hipMemGetAddressRange),
// at any alignment.  The aligned dword at `a` is
//   not loaded at all where none of its bytes is needed (behind the row's end);
//   loaded whole where it lies inside the allocation (it may start up to 3 bytes in front of the row or end up to 3 behind it);
//   assembled from byte loads of the needed bytes otherwise -- a row that ends flush with its allocation, on an end that is no multiple of 4.
// No load touches a byte outside [lo, end).  `seen` (host walks; nullptr in the kernels): [0] lowest, [1] highest byte address loaded.
VNECT_HD uint32_t ingest_load(uintptr_t a, uintptr_t need_lo, uintptr_t need_end, uintptr_t lo, uintptr_t end, uintptr_t* seen = nullptr)
{
    if (a >= need_end || a + 4 <= need_lo) return 0u;
    if (a >= lo && a + 4 <= end) {
        if (seen) seen[0] = a < seen[0] ? a : seen[0], seen[1] = a + 3 > seen[1] ? a + 3 : seen[1];
#if defined(__HIP_DEVICE_COMPILE__)
        return *(const uint32_t*)a;
#else
        uint32_t v;
        memcpy(&v, (const void*)a, 4);
        return v;
#endif
    }
    uint32_t v = 0;
    for (int j = 0; j < 4; j++) {
        const uintptr_t b = a + (unsigned)j;
        if (b < need_lo || b >= need_end || b < lo || b >= end) continue;
        if (seen) seen[0] = b < seen[0] ? b : seen[0], seen[1] = b > seen[1] ? b : seen[1];
        v |= (uint32_t)(*(const uint8_t*)b) << (8 * j);
    }
    return v;
}

// The PERMUTE: a group's payload -> its 12 packed bytes B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3 as three little-endian dwords.
// v: packed-3 three dwords, packed-4 four, planar v[c] = the four bytes of source channel c.
VNECT_HD void ingest_pack(int form, int order, const uint32_t* v, uint32_t* P)
{
    uint32_t b[12];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 12; i++) {
        const int p = i / 3, c = i - 3 * p, sc = order == INGEST_RGB ? 2 - c : c;
        const int idx = form == INGEST_PLANAR ? 4 * sc + p : (form == INGEST_PACKED4 ? 4 * p + sc : 3 * p + sc);
        b[i] = (v[idx >> 2] >> (8 * (idx & 3))) & 255u;
    }
    P[0] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
    P[1] = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
    P[2] = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
}

// The DESTINATION.  A group's 12 bytes land at byte t0 of a packed row of `row` = 3 w bytes that starts at any alignment: t0 = 12 G where
// groups are counted from the crop's first column (the device-frame copies), 12 G - 3 x where they are counted in frame columns (the NV12
// copies: the row's first group starts 0, 3, 6 or 9 bytes in front of the row).  e = the alignment of the group's first byte (the same for
// every group of a row).  The lane's WINDOW is the four aligned dwords from 4 bytes * floor: dword k holds bytes of the lane's dwords
// k - 1 and k (ingest_window_dword; k = 0: the previous lane's last dword, `prev`).
// Bit j of the mask: the lane writes byte j of its window.  The rules are those of copy_row_any_align:
//   bytes in front of the group's own (j < e) are the previous lane's, written here when the lane holds them (`head`: e == 0, or not lane 0
//   of its wave); the window's last dword, the lane's last e bytes, is written only when no lane behind this one in the wave writes it as
//   ITS dword 0 (`tail`: the wave's last lane or the row's last group); nothing outside [0, row) is written.  A dword whose four bits are set is one
//   whole store; the first and last dword of a row and the dword two waves share come out as byte stores.
VNECT_HD unsigned ingest_dst_mask(long long t0, int e, long long row, bool head, bool tail)
{
    // Window byte j is byte j - e of the group (negative: the previous group's), row byte t0 + j - e.  Each rule bounds j from one side,
    // so the lane's bytes are ONE run [lo, hi): from the previous group's bytes (head) or its own first, up to its dword 2's end or (tail)
    // its own last byte, cut to the row
    long long lo = head ? 0 : e, hi = tail ? 12 + e : 12;
    if (e - t0 > lo) lo = e - t0;                   // row byte 0
    if (row - t0 + e < hi) hi = row - t0 + e;       // row byte `row`
    if (hi <= lo) return 0u;                        // (0 <= lo and hi <= 15 from here)
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}
// the common lane, known without the mask: every byte of window dwords 0 .. 2 and nothing behind them (the mask is 0xfff there)
VNECT_HD bool ingest_dst_inner(long long t0, int e, long long row, bool head, bool tail) { return head && !tail && t0 - e >= 0 && t0 - e + 12 <= row; }
VNECT_HD uint32_t ingest_window_dword(const uint32_t* P, uint32_t prev, int e, int k)
{
    const uint32_t lo = k == 0 ? prev : P[k - 1], hi = k < 3 ? P[k] : 0u;
    return ingest_funnel(hi, lo, 4 - e);
}

}  // namespace vnect
