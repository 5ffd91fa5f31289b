// orient.h -- a frame that is stored rotated and / or mirrored -> the packed BGR crop of its ORIENTED picture: the map, the tile
// decomposition, the loads and the destination dwords, ONE source for host and device (as ingest.h, nv12.h and crop.h are).  The kernels
// of orient.hip and the host walk of orient_capi.cpp (tests/test_orient_cpu.py, and the sanitizer sweep) call the same functions.
// The reference turns a sideways camera's frame on the host with np.rot90(frame, 3) before it crops (run_estimator_ps.py:57-62, 81-85);
// here the turn happens inside the crop's copy, so only the crop is moved.  HIP-free when compiled by g++.
//
// An orientation is a code o in 0 .. 7: the oriented picture of a stored (H, W) frame f is
//     g = np.rot90(f, o & 3);  if o & 4: g = g[:, ::-1]
// (o = 3: the reference's `T`; o = 7: its commented np.transpose variant).  Everything a caller gives or gets -- rects, boxes, joints --
// is in oriented coordinates; H, W and the strides describe memory.
//
// A workgroup owns one ORIENT_T x ORIENT_T tile of the OUTPUT crop.  The stored pixels of that tile form a rectangle again (orient_src_rect).
// Its rows are loaded along the stored x axis as ALIGNED dwords (ingest_load's bounds rule) and parked in LDS as they come, one LDS row
// of ORIENT_PITCH dwords per stored row; behind one barrier every lane assembles one aligned DESTINATION dword of an output row from the
// bytes of the (at most two) pixels it covers.  Source forms: ingest.h's four and NV12 (two streams per row: Y, and the UV row under it).
#pragma once
#include <stdint.h>

#include "ingest.h"
#include "nv12.h"

namespace vnect {

enum { ORIENT_NV12 = 4 };            // the source form behind ingest.h's INGEST_PACKED3 .. INGEST_GENERIC
constexpr int ORIENT_T = 32;         // tile edge in pixels (64 was measured too: a 400 x 600 crop is then 70 workgroups, too few to hide their latency)
constexpr int ORIENT_THREADS = 256;  // four waves: wave v takes the tile's rows v, v + 4, ...
// An LDS row: the aligned dwords of a stored tile row.  packed-3: <= 25, packed-4: <= 33; planar: three streams of <= 9, NV12: Y <= 9
// and UV <= 10, each stream at its own ORIENT_SLOT.  The pitch is odd, so the 32 rows of a column lie in 32 different banks.
constexpr int ORIENT_SLOT = 11;
constexpr int ORIENT_PITCH = 35;
constexpr int ORIENT_ROW_DWORDS = (4 * ORIENT_T + 3 + 3) / 4;  // the longest row (packed-4 at the worst alignment): at most one per lane
static_assert(ORIENT_ROW_DWORDS <= 64 && ORIENT_ROW_DWORDS <= ORIENT_PITCH && 3 * ORIENT_SLOT <= ORIENT_PITCH && (ORIENT_T + 3 + 3) / 4 + 1 <= ORIENT_SLOT, "orient.h: LDS row layout");
constexpr int ORIENT_LDS_DWORDS = ORIENT_T * ORIENT_PITCH;

struct OrientSrc {
    const uint8_t* p0;      // pixel (0, 0), channel 0 (NV12: the Y plane's first byte), any alignment
    const uint8_t* p1;      // NV12: the interleaved U, V plane's first byte
    long long sy, sx, sc;   // byte strides, positive (NV12: sy = the Y pitch, sx = 1, sc = the UV pitch)
    const uint8_t* lo0;     // [lo0, end0): the allocation p0's bytes lie in -- no byte outside it is loaded
    const uint8_t* end0;
    const uint8_t* lo1;     // NV12: the same for the UV plane (one allocation: equal to lo0, end0)
    const uint8_t* end1;
    int form;               // INGEST_PACKED3 / PACKED4 / PLANAR / GENERIC, ORIENT_NV12
    int order;              // INGEST_BGR / INGEST_RGB
};

VNECT_HD bool orient_ok(int o) { return o >= 0 && o <= 7; }
// the oriented picture's size
VNECT_HD void orient_size(int o, int H, int W, int* Ho, int* Wo) { *Ho = (o & 1) ? W : H, *Wo = (o & 1) ? H : W; }
// oriented pixel (i, j) -> the stored pixel (r, c) of the (H, W) frame
VNECT_HD void orient_map(int o, int H, int W, int i, int j, int* r, int* c)
{
    if (o & 4) j = ((o & 1) ? H : W) - 1 - j;
    switch (o & 3) {
    case 0: *r = i, *c = j; break;
    case 1: *r = j, *c = W - 1 - i; break;
    case 2: *r = H - 1 - i, *c = W - 1 - j; break;
    default: *r = H - 1 - j, *c = i; break;
    }
}
// the other way: stored pixel (r, c) -> where it lies in the oriented picture
VNECT_HD void orient_unmap(int o, int H, int W, int r, int c, int* i, int* j)
{
    switch (o & 3) {
    case 0: *i = r, *j = c; break;
    case 1: *i = W - 1 - c, *j = r; break;
    case 2: *i = H - 1 - r, *j = W - 1 - c; break;
    default: *i = c, *j = H - 1 - r; break;
    }
    if (o & 4) *j = ((o & 1) ? H : W) - 1 - *j;
}
// the stored rectangle s = (x, y, w, h) that the oriented crop (x, y, w, h) reads (w, h >= 1, inside the oriented picture)
VNECT_HD void orient_src_rect(int o, int H, int W, int x, int y, int w, int h, int* s)
{
    int r0, c0, r1, c1;
    orient_map(o, H, W, y, x, &r0, &c0);
    orient_map(o, H, W, y + h - 1, x + w - 1, &r1, &c1);
    s[0] = c0 < c1 ? c0 : c1, s[1] = r0 < r1 ? r0 : r1;
    s[2] = (o & 1) ? h : w, s[3] = (o & 1) ? w : h;
}

// Tile (ti, tj) of the crop (x, y, w, h): rows i0 .. i0 + th - 1 and columns j0 .. j0 + tw - 1 of the CROP, and the stored rectangle
// (C0, R0, sw, sh) they come from.  false: the tile lies outside the crop.
struct OrientTile {
    int i0, j0, th, tw;
    int C0, R0, sw, sh;
};
VNECT_HD bool orient_tile(int o, int H, int W, int x, int y, int w, int h, int ti, int tj, OrientTile* t)
{
    const long long i0 = (long long)ti * ORIENT_T, j0 = (long long)tj * ORIENT_T;
    if (i0 >= h || j0 >= w) return false;
    t->i0 = (int)i0, t->j0 = (int)j0;
    t->th = h - t->i0 < ORIENT_T ? h - t->i0 : ORIENT_T, t->tw = w - t->j0 < ORIENT_T ? w - t->j0 : ORIENT_T;
    int s[4];
    orient_src_rect(o, H, W, x + t->j0, y + t->i0, t->tw, t->th, s);
    t->C0 = s[0], t->R0 = s[1], t->sw = s[2], t->sh = s[3];
    return true;
}

VNECT_HD int orient_streams(int form) { return form == INGEST_PLANAR ? 3 : (form == ORIENT_NV12 ? 2 : 1); }
// stream k of stored row R from column C0, sw pixels: its first byte, the bytes needed from there, the allocation
VNECT_HD void orient_stream(const OrientSrc& s, int form, int k, int R, int C0, int sw, uintptr_t* A, long long* need, uintptr_t* lo, uintptr_t* end)
{
    *lo = (uintptr_t)s.lo0, *end = (uintptr_t)s.end0;
    const uintptr_t row = (uintptr_t)s.p0 + (unsigned long long)R * (unsigned long long)s.sy;
    if (form == INGEST_PACKED3) *A = row + 3ull * (unsigned)C0, *need = 3LL * sw;
    else if (form == INGEST_PACKED4) *A = row + 4ull * (unsigned)C0, *need = 4LL * sw - 1;
    else if (form == INGEST_PLANAR) *A = row + (unsigned)C0 + (unsigned long long)k * (unsigned long long)s.sc, *need = sw;
    else if (k == 0) *A = row + (unsigned)C0, *need = sw;  // NV12: Y
    else {                                                 // NV12: the chroma pairs of columns C0 .. C0 + sw - 1
        const int u0 = C0 & ~1, u1 = ((C0 + sw - 1) & ~1) + 2;
        *A = (uintptr_t)s.p1 + (unsigned long long)(R >> 1) * (unsigned long long)s.sc + (unsigned)u0, *need = u1 - u0;
        *lo = (uintptr_t)s.lo1, *end = (uintptr_t)s.end1;
    }
}

// The LOADS of one lane for stored row R of a tile: aligned dwords lane, lane + 64, ... of every stream -> the LDS row.  The generic form
// (any strides) has no streams: lane = pixel, three byte loads, one dword B | G << 8 | R << 16 (source order) per pixel.
// `seen` (host walks, four words; nullptr in the kernels): [0] lowest, [1] highest byte address loaded.
VNECT_HD void orient_load_row(const OrientSrc& s, int form, int R, int C0, int sw, uint32_t* ldsrow, int lane, uintptr_t* seen = nullptr)
{
    if (form == INGEST_GENERIC) {
        for (int c = lane; c < sw; c += 64) {
            const uintptr_t p = (uintptr_t)s.p0 + (unsigned long long)R * (unsigned long long)s.sy + (unsigned long long)(C0 + c) * (unsigned long long)s.sx;
            uint32_t v = 0;
            for (int k = 0; k < 3; k++) {
                const uintptr_t a = p + (unsigned long long)k * (unsigned long long)s.sc;
                if (seen) seen[0] = a < seen[0] ? a : seen[0], seen[1] = a > seen[1] ? a : seen[1];
                v |= (uint32_t)(*(const uint8_t*)a) << (8 * k);
            }
            ldsrow[c] = v;
        }
        return;
    }
    const int ns = orient_streams(form);
    for (int k = 0; k < ns; k++) {
        uintptr_t A, lo, end;
        long long need;
        orient_stream(s, form, k, R, C0, sw, &A, &need, &lo, &end);
        const uintptr_t al = A & ~(uintptr_t)3;
        const int ndw = (int)((A + (unsigned long long)need - al + 3) >> 2);
        uintptr_t* sn = seen && form == ORIENT_NV12 ? seen + 2 * k : seen;  // (NV12: the UV plane's loads are reported apart, [2], [3])
        for (int l = lane; l < ndw; l += 64) ldsrow[k * ORIENT_SLOT + l] = ingest_load(al + 4ull * (unsigned)l, A, A + (unsigned long long)need, lo, end, sn);
    }
}

// The COMMON TILE: every aligned dword its loads touch lies inside the allocation(s), so none of them needs ingest_load's tests (a tile at
// the very start or end of an allocation, and the generic form, take orient_load_row).  Rows lie at ascending addresses (strides are
// positive), so the tile's first and last row bound every stream.
VNECT_HD bool orient_tile_inside(const OrientSrc& s, int form, const OrientTile& t)
{
    if (form == INGEST_GENERIC) return false;
    const int ns = orient_streams(form);
    for (int k = 0; k < ns; k++) {
        uintptr_t A0, A1, lo, end;
        long long need;
        orient_stream(s, form, k, t.R0, t.C0, t.sw, &A0, &need, &lo, &end);
        orient_stream(s, form, k, t.R0 + t.sh - 1, t.C0, t.sw, &A1, &need, &lo, &end);
        if ((A0 & ~(uintptr_t)3) < lo || ((A1 + (unsigned long long)need + 3) & ~(uintptr_t)3) > end) return false;
    }
    return true;
}
// In such a tile, dword `l` of stream k of tile row rr: *a = the address to load, *at = the LDS dword it goes to, or -1 -- the lane has
// no dword there (rr or l past the end) and loads the row's (the tile's) first instead, which is always valid, and drops it.  Every
// lane's load is then unconditional, and the loads of all of a wave's rows can be in flight together.
VNECT_HD void orient_inside_dword(const OrientSrc& s, int form, const OrientTile& t, int k, int rr, int l, uintptr_t* a, int* at)
{
    const bool row = rr < t.sh;
    uintptr_t A, lo, end;
    long long need;
    orient_stream(s, form, k, t.R0 + (row ? rr : 0), t.C0, t.sw, &A, &need, &lo, &end);
    const uintptr_t al = A & ~(uintptr_t)3;
    const bool mine = row && l < (int)((A + (unsigned long long)need - al + 3) >> 2);
    *a = al + (mine ? 4ull * (unsigned)l : 0ull);
    *at = mine ? rr * ORIENT_PITCH + k * ORIENT_SLOT + l : -1;
}
VNECT_HD uint32_t orient_load_inside(uintptr_t a, int at, int form, int k, uintptr_t* seen = nullptr)
{
    uintptr_t* sn = seen && form == ORIENT_NV12 ? seen + 2 * k : seen;
    (void)at;
    if (sn) sn[0] = a < sn[0] ? a : sn[0], sn[1] = a + 3 > sn[1] ? a + 3 : sn[1];
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint32_t*)a;
#else
    uint32_t v;
    memcpy(&v, (const void*)a, 4);
    return v;
#endif
}

VNECT_HD int orient_lds_byte(const uint32_t* ldsrow, int off) { return (int)((ldsrow[off >> 2] >> (8 * (off & 3))) & 255u); }
// stored pixel (R, C) of a tile whose LDS row for R is `ldsrow` (loaded from column C0) -> its B, G, R
VNECT_HD void orient_pixel(const OrientSrc& s, int form, const uint32_t* ldsrow, int R, int C, int C0, int* bgr)
{
    const uintptr_t row = (uintptr_t)s.p0 + (unsigned long long)R * (unsigned long long)s.sy;
    if (form == ORIENT_NV12) {
        const int ay = (int)((row + (unsigned)C0) & 3), u0 = C0 & ~1;
        const int au = (int)(((uintptr_t)s.p1 + (unsigned long long)(R >> 1) * (unsigned long long)s.sc + (unsigned)u0) & 3);
        const int ou = 4 * ORIENT_SLOT + au + ((C & ~1) - u0);
        nv12_pixel(orient_lds_byte(ldsrow, ay + (C - C0)), orient_lds_byte(ldsrow, ou), orient_lds_byte(ldsrow, ou + 1), bgr);
        return;
    }
    int c[3];
    if (form == INGEST_GENERIC) {
        for (int k = 0; k < 3; k++) c[k] = orient_lds_byte(ldsrow, 4 * (C - C0) + k);
    } else if (form == INGEST_PLANAR) {
        for (int k = 0; k < 3; k++)
            c[k] = orient_lds_byte(ldsrow, 4 * ORIENT_SLOT * k + (int)((row + (unsigned)C0 + (unsigned long long)k * (unsigned long long)s.sc) & 3) + (C - C0));
    } else {
        const int px = form == INGEST_PACKED3 ? 3 : 4;
        const int a = (int)((row + (unsigned long long)px * (unsigned)C0) & 3) + px * (C - C0);
        for (int k = 0; k < 3; k++) c[k] = orient_lds_byte(ldsrow, a + k);
    }
    bgr[0] = s.order == INGEST_RGB ? c[2] : c[0], bgr[1] = c[1], bgr[2] = s.order == INGEST_RGB ? c[0] : c[2];
}

// The DESTINATION dword of lane `l` for row `ii` of tile t: the crop's rows are packed, 3 w bytes apart, from `dst` (any alignment), so the
// tile row's 3 tw bytes start at any phase of the dword grid.  Lane l owns the l-th aligned dword that holds bytes of the tile row.
// Returns the mask of the bytes it writes (bit j: byte j of the dword at *addr gets byte j of *val): 15 -- the dword lies wholly inside
// the tile row -- is one whole store; a dword at either end of the tile row is shared with the neighbouring tile or crop row, or sticks out
// of the 3 w h bytes, and the lane stores only its own bytes, one by one.  0: nothing (no such dword).
VNECT_HD unsigned orient_out_dword(const OrientSrc& s, int form, int o, int H, int W, int x, int y, int w, const OrientTile& t, int ii, int l,
                                   const uint32_t* lds, uintptr_t dst, uintptr_t* addr, uint32_t* val)
{
    const int i = t.i0 + ii, row = 3 * t.tw;
    const uintptr_t d = dst + ((unsigned long long)i * (unsigned)w + (unsigned)t.j0) * 3ull;
    const uintptr_t d0 = d & ~(uintptr_t)3;
    const int ad = (int)(d - d0);
    if (l >= ((ad + row + 3) >> 2)) return 0u;
    const int q0 = 4 * l - ad;                  // tile-row byte index of the dword's byte 0
    const int pa = (q0 > 0 ? q0 : 0) / 3;       // the first pixel with a byte in the dword; the last is pa or pa + 1
    int px[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 2; k++) {
        if (pa + k >= t.tw || 3 * (pa + k) >= q0 + 4) continue;
        int R, C;
        orient_map(o, H, W, y + i, x + t.j0 + pa + k, &R, &C);
        orient_pixel(s, form, lds + (R - t.R0) * ORIENT_PITCH, R, C, t.C0, px + 3 * k);
    }
    unsigned m = 0;
    uint32_t v = 0;
    for (int j = 0; j < 4; j++) {
        const int q = q0 + j;
        if (q < 0 || q >= row) continue;
        m |= 1u << j, v |= (uint32_t)px[q - 3 * pa] << (8 * j);
    }
    *addr = d0 + 4ull * (unsigned)l, *val = v;
    return m;
}

}  // namespace vnect
