// ingest_capi.cpp -- C shim over ingest.h for tests/test_device_frames_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.
// Built with plain g++ (`make -C vnect_amd/csrc ingest`).  ingest_walk goes through a crop the way the kernels of post.hip do -- row by
// row, wave by wave, 64 lanes at a time, the shuffles as array look-ups -- with the SAME functions for the loads, the permute and the
// destination masks, so the window arithmetic is held to a plain gather without a GPU, and the lowest and highest byte it loads are
// reported.  ingest_store_walk drives the store rule alone, from the row starts the NV12 copies have.  With -DINGEST_SWEEP_MAIN
// (`make ... ingest_sweep_asan`, -fsanitize=address,undefined) the same file is a stand-alone program whose sources sit in exactly sized
// heap blocks: a load outside the allocation is the sanitizer's finding.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ingest.h"

using namespace vnect;

namespace {

struct Walk {
    uintptr_t lo, end;      // the allocation
    uintptr_t seen[2];      // lowest / highest byte loaded
    uint8_t* dst;           // the crop's first destination byte
    long long dst_bytes;    // 3 w h
    uint8_t* hits;          // per destination byte: times written (may be null)
    long long stray;        // stores outside [dst, dst + dst_bytes)
};

void put(Walk& W, uintptr_t addr, uint8_t v)
{
    const long long off = (long long)(addr - (uintptr_t)W.dst);
    if (addr < (uintptr_t)W.dst || off >= W.dst_bytes) {
        W.stray++;
        return;
    }
    W.dst[off] = v;
    if (W.hits && W.hits[off] < 255) W.hits[off]++;
}

// The stores of one wave, as ingest_store_row (post.hip) runs them: lane `lane` holds the 12 bytes P[lane] of group Gw + lane, which land at
// byte 12 G - lead of the packed row of `row` bytes at `drow`.  lead 0: groups counted from the crop's first column (ingest_row); 3, 6 or 9:
// the row's first group starts that many bytes in front of the row (nv12_strip: groups counted in frame columns, lead = 3 (x & 3)).
void store_wave(Walk& W, uint8_t* drow, long long row, int lead, int Gw, int G1, const uint32_t (*P)[3])
{
    for (int lane = 0; lane < 64; lane++) {
        const int G = Gw + lane;
        if (G > G1) break;
        const uint32_t prev = P[lane > 0 ? lane - 1 : 0][2];  // __shfl_up(.., 1)
        const long long t0 = 12LL * G - lead;
        const uintptr_t E = (uintptr_t)((long long)(uintptr_t)drow + t0);
        const int e = (int)(E & 3);
        const bool head = e == 0 || lane > 0, tail = e != 0 && (lane == 63 || G == G1);
        const unsigned m = ingest_dst_inner(t0, e, row, head, tail) ? 0xfffu : ingest_dst_mask(t0, e, row, head, tail);
        for (int k = 0; k < 4; k++) {
            const uint32_t q = ingest_window_dword(P[lane], prev, e, k);
            for (int b = 0; b < 4; b++)
                if (m & (1u << (4 * k + b))) put(W, E - (unsigned)e + 4u * k + b, (uint8_t)(q >> (8 * b)));
        }
    }
}

// one row of the crop, as ingest_row + ingest_store_row (post.hip) run it
void walk_row(Walk& W, int form, int order, uintptr_t origin, long long sy, long long sc, int w, int y)
{
    const int NS = ingest_streams(form), ND = ingest_dwords(form), G1 = (w - 1) >> 2;
    const uintptr_t row0 = origin + (unsigned long long)y * (unsigned long long)sy;
    uint8_t* drow = W.dst + (unsigned long long)y * (3ull * (unsigned)w);
    for (int Gw = 0; Gw <= G1; Gw += 64) {
        uint32_t d[64][3][5], P[64][3];
        int sh[3] = {0, 0, 0};
        memset(d, 0, sizeof d);
        for (int lane = 0; lane < 64; lane++) {
            const int G = Gw + lane;
            const bool act = G <= G1, self_hi = act && (lane == 63 || G == G1);
            for (int c = 0; c < NS; c++) {
                const uintptr_t a0 = row0 + (unsigned long long)c * (unsigned long long)sc, need_end = a0 + (unsigned long long)ingest_row_need(form, w);
                const uintptr_t a = a0 + 4ull * ND * (unsigned)G, al = a & ~(uintptr_t)3;
                sh[c] = (int)(a & 3);
                if (!act) continue;
                for (int i = 0; i < ND; i++) d[lane][c][i] = ingest_load(al + 4u * i, a0, need_end, W.lo, W.end, W.seen);
                if (self_hi && sh[c]) d[lane][c][ND] = ingest_load(al + 4u * ND, a0, need_end, W.lo, W.end, W.seen);
            }
        }
        for (int lane = 0; lane < 64; lane++) {
            const int G = Gw + lane;
            const bool self_hi = G <= G1 && (lane == 63 || G == G1);
            uint32_t v[12];
            for (int c = 0; c < NS; c++) {
                if (sh[c] && !self_hi) d[lane][c][ND] = d[lane < 63 ? lane + 1 : lane][c][0];  // __shfl_down(.., 1)
                for (int i = 0; i < ND; i++) v[c * ND + i] = sh[c] ? ingest_funnel(d[lane][c][i + 1], d[lane][c][i], sh[c]) : d[lane][c][i];
            }
            ingest_pack(form, order, v, P[lane]);
        }
        store_wave(W, drow, 3LL * w, 0, Gw, G1, P);
    }
}

void walk_row_generic(Walk& W, int order, uintptr_t origin, long long sy, long long sx, long long sc, int w, int y)
{
    for (int px = 0; px < w; px++) {
        const uintptr_t p = origin + (unsigned long long)y * (unsigned long long)sy + (unsigned long long)px * (unsigned long long)sx;
        uint8_t c[3];
        for (int k = 0; k < 3; k++) {
            const uintptr_t a = p + (unsigned long long)k * (unsigned long long)sc;
            W.seen[0] = a < W.seen[0] ? a : W.seen[0], W.seen[1] = a > W.seen[1] ? a : W.seen[1];
            c[k] = *(const uint8_t*)a;
        }
        const uintptr_t q = (uintptr_t)W.dst + ((unsigned long long)y * (unsigned)w + (unsigned)px) * 3ull;
        put(W, q, order == INGEST_RGB ? c[2] : c[0]), put(W, q + 1, c[1]), put(W, q + 2, order == INGEST_RGB ? c[0] : c[2]);
    }
}

}  // namespace

extern "C" {

// [0] pixels per lane, [1] per wave, [2] per workgroup of the coalesced kernels, [3] per workgroup of the generic one (ingest.h)
void ingest_kernel_spans(int32_t* out) { out[0] = INGEST_LANE_PX, out[1] = INGEST_WAVE_PX, out[2] = INGEST_WG_PX, out[3] = INGEST_GENERIC_WG_PX; }

int ingest_classify(int64_t stride_x, int64_t stride_c) { return ingest_form(stride_x, stride_c); }

int64_t ingest_frame_span(int H, int W, int64_t sy, int64_t sx, int64_t sc) { return ingest_span(H, W, sy, sx, sc); }

// The crop (x, y, w, h) of the (H, W) frame whose pixel (0, 0) lies data_off bytes into the allocation [base, base + size) -> dst, rows
// packed 3 w bytes apart (dst at any alignment).  hits (3 w h bytes, or null): how often each destination byte was written.  seen: the
// lowest and highest offset from `base` of any byte loaded.  Returns the number of stores that fell outside the 3 w h bytes (0 when the
// masks are right), or -1 for arguments the runtime would refuse.
int64_t ingest_walk(const uint8_t* base, int64_t size, int64_t data_off, int H, int W, int64_t sy, int64_t sx, int64_t sc, int order, int force_generic,
                    int x, int y, int w, int h, uint8_t* dst, uint8_t* hits, int64_t* seen)
{
    if (!base || !dst || H < 1 || W < 1 || sy < 1 || sx < 1 || sc < 1 || data_off < 0 || x < 0 || y < 0 || w < 1 || h < 1 || (int64_t)x + w > W || (int64_t)y + h > H)
        return -1;
    if (data_off + ingest_span(H, W, sy, sx, sc) > size) return -1;
    Walk Wk = {(uintptr_t)base, (uintptr_t)base + (uint64_t)size, {~(uintptr_t)0, 0}, dst, 3LL * w * h, hits, 0};
    const uintptr_t origin = (uintptr_t)base + (uint64_t)data_off + (uint64_t)y * (uint64_t)sy + (uint64_t)x * (uint64_t)sx;
    const int form = force_generic ? INGEST_GENERIC : ingest_form(sx, sc);
    for (int r = 0; r < h; r++) {
        if (form == INGEST_GENERIC) walk_row_generic(Wk, order, origin, sy, sx, sc, w, r);
        else walk_row(Wk, form, order, origin, sy, sc, w, r);
    }
    if (seen) seen[0] = (int64_t)(Wk.seen[0] - (uintptr_t)base), seen[1] = (int64_t)(Wk.seen[1] - (uintptr_t)base);
    return Wk.stray;
}

// The store rule alone, as the NV12 copies drive it: one packed row of w pixels at `dst` (any alignment) whose first group starts `lead`
// (0, 3, 6 or 9) bytes in front of the row.  Every byte a group holds is synthetic, ingest_store_byte of its row byte index (bytes in front
// of the row and behind it have indices outside [0, 3 w): none of them may be stored).  hits (3 w bytes, or null) as in ingest_walk.
// Returns the number of stores outside the row's 3 w bytes, or -1 for arguments nv12_strip cannot produce.
uint8_t ingest_store_byte(int64_t t) { return (uint8_t)(((t + 12) * 37) % 251); }

int64_t ingest_store_walk(int w, int lead, uint8_t* dst, uint8_t* hits)
{
    if (!dst || w < 1 || lead < 0 || lead > 9 || lead % 3) return -1;
    Walk Wk = {0, 0, {~(uintptr_t)0, 0}, dst, 3LL * w, hits, 0};
    const int G1 = (lead / 3 + w - 1) >> 2;
    for (int Gw = 0; Gw <= G1; Gw += 64) {
        uint32_t P[64][3];
        for (int lane = 0; lane < 64; lane++)
            for (int k = 0; k < 3; k++) {
                P[lane][k] = 0;
                for (int b = 0; b < 4; b++) P[lane][k] |= (uint32_t)ingest_store_byte(12LL * (Gw + lane) - lead + 4 * k + b) << (8 * b);
            }
        store_wave(Wk, dst, 3LL * w, lead, Gw, G1, P);
    }
    return Wk.stray;
}

}  // extern "C"

#ifdef INGEST_SWEEP_MAIN
// Every form x order x source offset 0..3 x destination phase 0..3 x width, three rows: the frame flush against both ends of an exactly
// sized heap block (offset 0: flush at the start too), the destination in an exactly sized block of its own.
int main()
{
    long long walks = 0, bad = 0;
    std::vector<int> widths;
    for (int w = 1; w <= 2 * INGEST_WAVE_PX + 1; w++)
        if (w <= 41 || (w % INGEST_WAVE_PX) <= 2 || (w % INGEST_WAVE_PX) >= INGEST_WAVE_PX - 2) widths.push_back(w);
    const int h = 3;
    for (int form = 0; form < 4; form++)
        for (int order = 0; order < 2; order++)
            for (int w : widths)
                for (int off = 0; off < 4; off++)
                    for (int pad = 0; pad < 6; pad += 5) {
                        long long sx, sc, sy;
                        if (form == INGEST_PACKED3) sx = 3, sc = 1, sy = 3LL * w + pad;
                        else if (form == INGEST_PACKED4) sx = 4, sc = 1, sy = 4LL * w + pad;
                        else if (form == INGEST_PLANAR) sx = 1, sy = w + pad, sc = sy * h + 3;
                        else sx = 5, sc = 2, sy = 5LL * w + pad;
                        const long long span = ingest_span(h, w, sy, sx, sc);
                        uint8_t* src = (uint8_t*)malloc((size_t)(off + span));
                        for (long long i = 0; i < off + span; i++) src[i] = (uint8_t)((i * 2654435761u) >> 13);
                        for (int ph = 0; ph < 4; ph++) {
                            const long long n = 3LL * w * h;
                            uint8_t* blk = (uint8_t*)malloc((size_t)(ph + n));
                            std::vector<uint8_t> hits((size_t)n, 0);
                            int64_t seen[2];
                            const int64_t stray = ingest_walk(src, off + span, off, h, w, sy, sx, sc, order, 0, 0, 0, w, h, blk + ph, hits.data(), seen);
                            bad += stray != 0;
                            if (seen[0] < 0 || seen[1] >= off + span) bad++;
                            for (int r = 0; r < h; r++)
                                for (int p = 0; p < w; p++)
                                    for (int c = 0; c < 3; c++) {
                                        const long long i = ((long long)r * w + p) * 3 + c;
                                        const int scn = order == INGEST_RGB ? 2 - c : c;
                                        bad += blk[ph + i] != src[off + r * sy + p * sx + scn * sc];
                                        bad += hits[(size_t)i] != 1;
                                    }
                            free(blk);
                            walks++;
                        }
                        free(src);
                    }
    // the store rule alone at NV12's row starts: lead 0, 3, 6, 9 x destination phase 0..3 x the same widths
    for (int w : widths)
        for (int lead = 0; lead < 12; lead += 3)
            for (int ph = 0; ph < 4; ph++) {
                const long long n = 3LL * w;
                uint8_t* blk = (uint8_t*)malloc((size_t)(ph + n));
                std::vector<uint8_t> hits((size_t)n, 0);
                bad += ingest_store_walk(w, lead, blk + ph, hits.data()) != 0;
                for (long long i = 0; i < n; i++) bad += blk[ph + i] != ingest_store_byte(i), bad += hits[(size_t)i] != 1;
                free(blk);
                walks++;
            }
    printf("ingest sweep: %lld walks, %lld mismatches\n", walks, bad);
    return bad ? 1 : 0;
}
#endif
