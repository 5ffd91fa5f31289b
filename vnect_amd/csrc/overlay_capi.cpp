// overlay_capi.cpp -- C shim over overlay.h for tests/test_overlay_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.
// Built with plain g++ (`make -C vnect_amd/csrc overlay`).  overlay_walk goes through a frame the way the kernel of overlay.hip does --
// tile by tile, the limbs and the band culled against the tile, an empty tile left at once, then lane by lane, cell by cell -- with the
// SAME functions for the set-up, the tests and the stores, so the rule as the device runs it is held to an independent numpy statement of
// it without a GPU.  The stores go straight into the caller's buffer: with -DOVERLAY_SWEEP_MAIN (`make ... overlay_sweep_asan`,
// -fsanitize=address,undefined) the same file is a stand-alone program whose targets sit in exactly sized heap blocks, and a store outside
// the frame is the sanitizer's finding.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "overlay.h"

using namespace vnect;

namespace {

// the frame's bytes from pixel (0, 0) channel 0 to its last (ingest.h: ingest_span), and an NV12 plane's
long long span_of(int H, int W, long long sy, long long sx, long long sc) { return (long long)(H - 1) * sy + (long long)(W - 1) * sx + 2 * sc + 1; }
long long plane_span(int rows, int W, long long pitch) { return (long long)(rows - 1) * pitch + W; }

void walk(const OverlayTarget& t, const OverlayInput& in)
{
    const int px = t.nv12 ? 2 : 1, ncy = overlay_cells_y(t), ncx = overlay_cells_x(t);
    OverlayLimb L[OVERLAY_NJ];
    for (int i = 0; i < OVERLAY_NJ; i++) L[i] = overlay_limb_of(in.j2d, in.conf, in.has_conf != 0, in.min_conf, in.parents, i);
    const OverlayBand band = overlay_band(in.has_rect != 0, in.rect[0], in.rect[1], in.rect[2], in.rect[3]);
    for (int cy0 = 0; cy0 < ncy; cy0 += OVERLAY_TILE_H)
        for (int cx0 = 0; cx0 < ncx; cx0 += OVERLAY_TILE_W) {
            const int cy1 = (cy0 + OVERLAY_TILE_H < ncy ? cy0 + OVERLAY_TILE_H : ncy) - 1, cx1 = (cx0 + OVERLAY_TILE_W < ncx ? cx0 + OVERLAY_TILE_W : ncx) - 1;
            const long long y0 = (long long)cy0 * px, y1 = (long long)cy1 * px + (px - 1), x0 = (long long)cx0 * px, x1 = (long long)cx1 * px + (px - 1);
            int live[OVERLAY_NJ], n = 0;
            for (int i = 0; i < OVERLAY_NJ; i++)
                if (overlay_limb_near(L[i], y0, y1, x0, x1)) live[n++] = i;
            if (n == 0 && !overlay_band_near(band, y0, y1, x0, x1)) continue;
            for (int tid = 0; tid < OVERLAY_THREADS; tid++) {
                const int cx = cx0 + tid % OVERLAY_TILE_W, cy = cy0 + tid / OVERLAY_TILE_W;
                if (cx > cx1 || cy > cy1) continue;
                overlay_lane(t, L, live, n, band, cx, cy, cy1);
            }
        }
}

}  // namespace

extern "C" {

// [0] the tile's width and [1] height in cells (a cell: one pixel, or NV12's 2 x 2 block), [2] lanes per workgroup
void overlay_tile(int32_t* out) { out[0] = OVERLAY_TILE_W, out[1] = OVERLAY_TILE_H, out[2] = OVERLAY_THREADS; }

void overlay_yuv(const int32_t* bgr, uint8_t* yuv3)
{
    const int c[3] = {bgr[0], bgr[1], bgr[2]};
    overlay_bgr_to_yuv(c, yuv3);
}

// a limb's set-up: out = (skip, a^2, centre row, centre column)
void overlay_limb_setup(double r1, double c1, double r2, double c2, double* out4)
{
    const OverlayLimb l = overlay_limb(r1, c1, r2, c2, false);
    out4[0] = l.skip, out4[1] = l.aa, out4[2] = l.cr, out4[3] = l.cc;
}

// Draws into the frame whose pixel (0, 0) channel 0 (NV12: Y plane) lies data_off bytes into the buffer [base, base + size), the UV plane
// uv_off bytes in.  format 0 BGR, 1 RGB, 2 NV12.  conf / parents / rect4 may be null (no threshold -- min_conf is ignored then --, the
// reference's parents, no rectangle).  Returns 0, or -1 for arguments the runtime would refuse (then nothing is written).
int overlay_walk(uint8_t* base, int64_t size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
                 int64_t uv_stride, const double* j2d, const double* conf, double min_conf, const int32_t* parents, const int32_t* rect4,
                 const int32_t* limb_bgr, const int32_t* rect_bgr)
{
    if (!base || !j2d || !limb_bgr || !rect_bgr || H < 1 || W < 1 || data_off < 0 || format < 0 || format > 2) return -1;
    OverlayTarget t;
    OverlayInput in;
    memset(&t, 0, sizeof t);
    memset(&in, 0, sizeof in);
    t.H = H, t.W = W, t.data = base + data_off;
    if (format == 2) {
        if (((H | W) & 1) || sy < W || uv_stride < W || uv_off < 0) return -1;
        if (data_off + plane_span(H, W, sy) > size || uv_off + plane_span(H / 2, W, uv_stride) > size) return -1;
        t.nv12 = 1, t.sy = sy, t.sx = 1, t.uv = base + uv_off, t.uv_stride = uv_stride;
    } else {
        if (sy < 1 || sx < 1 || sc < 1 || data_off + span_of(H, W, sy, sx, sc) > size) return -1;
        t.sy = sy, t.sx = sx, t.sc = sc;
    }
    int lc[3], rc[3];
    for (int k = 0; k < 3; k++) {
        lc[k] = limb_bgr[k], rc[k] = rect_bgr[k];
        if (lc[k] < 0 || lc[k] > 255 || rc[k] < 0 || rc[k] > 255) return -1;
    }
    overlay_colours(&t, format == 1, lc, rc);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        in.parents[i] = parents ? parents[i] : OVERLAY_PARENTS[i];
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return -1;
    }
    memcpy(in.j2d, j2d, sizeof in.j2d);
    if (conf) memcpy(in.conf, conf, sizeof in.conf), in.min_conf = min_conf, in.has_conf = min_conf == min_conf;
    if (rect4) {
        if (rect4[2] < 1 || rect4[3] < 1) return -1;
        for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
        in.has_rect = 1;
    }
    walk(t, in);
    return 0;
}

}  // extern "C"

#ifdef OVERLAY_SWEEP_MAIN
// Layouts x odd sizes x limbs and rects hanging over every edge, each target in an exactly sized heap block (its first pixel byte at the
// block's first, its last at the block's last): a store outside the frame is the sanitizer's finding.  Every walk is also held to a plain
// per-pixel statement of the rule (no tiles, no cull), and the bytes that are no pixel's -- row padding, fourth bytes -- to their canary.
namespace {

struct Layout { int format; long long sx, sc; int pad; const char* name; };

long long check(const uint8_t* blk, const std::vector<uint8_t>& before, const OverlayTarget& t, const OverlayInput& in, long long size)
{
    OverlayLimb L[OVERLAY_NJ];
    for (int i = 0; i < OVERLAY_NJ; i++) L[i] = overlay_limb_of(in.j2d, in.conf, in.has_conf != 0, in.min_conf, in.parents, i);
    const OverlayBand band = overlay_band(in.has_rect != 0, in.rect[0], in.rect[1], in.rect[2], in.rect[3]);
    std::vector<uint8_t> want(before);
    auto state = [&](int y, int x) {
        if (overlay_in_band(band, y, x)) return (int)OVERLAY_BAND;
        for (int i = 0; i < OVERLAY_NJ; i++)
            if (!L[i].skip && overlay_inside(L[i], y, x)) return (int)OVERLAY_LIMB;
        return (int)OVERLAY_NONE;
    };
    const long long uv0 = t.nv12 ? t.uv - t.data : 0;
    for (int y = 0; y < t.H; y++)
        for (int x = 0; x < t.W; x++) {
            const int s = state(y, x);
            if (s == OVERLAY_NONE) continue;
            if (!t.nv12) {
                for (int c = 0; c < 3; c++) want[(size_t)(y * t.sy + x * t.sx + c * t.sc)] = t.col[s - 1][c];
            } else {
                want[(size_t)(y * t.sy + x)] = t.col[s - 1][0];
            }
        }
    if (t.nv12)
        for (int by = 0; by < t.H / 2; by++)
            for (int bx = 0; bx < t.W / 2; bx++) {
                int c = OVERLAY_NONE;
                for (int q = 0; q < 4; q++) c = overlay_chroma(c, state(2 * by + q / 2, 2 * bx + q % 2));
                if (c == OVERLAY_NONE) continue;
                want[(size_t)(uv0 + by * t.uv_stride + 2 * bx)] = t.col[c - 1][1], want[(size_t)(uv0 + by * t.uv_stride + 2 * bx + 1)] = t.col[c - 1][2];
            }
    long long bad = 0;
    for (long long i = 0; i < size; i++) bad += blk[i] != want[(size_t)i];
    return bad;
}

}  // namespace

int main()
{
    const Layout layouts[] = {{0, 3, 1, 0, "packed-3"}, {0, 3, 1, 5, "packed-3 padded"}, {1, 4, 1, 0, "packed-4 rgb"}, {0, 1, 0, 3, "planar"},
                              {0, 5, 2, 1, "generic"},  {2, 1, 0, 0, "nv12"},            {2, 1, 0, 6, "nv12 pitched"}};
    const int sizes[][2] = {{37, 53}, {1, 1}, {3, 129}, {65, 7}, {34, 66}, {64, 128}};
    long long walks = 0, bad = 0, drawn = 0;
    for (const Layout& lay : layouts)
        for (const auto& hw : sizes) {
            int H = hw[0], W = hw[1];
            if (lay.format == 2) H = (H + 1) & ~1, W = (W + 1) & ~1;
            // limbs (joint 0 -> 16, 16 -> 1, 1 -> 15 ...: the reference's parents) across the frame and over every edge and corner
            for (int cse = 0; cse < 12; cse++) {
                OverlayTarget t;
                OverlayInput in;
                memset(&t, 0, sizeof t), memset(&in, 0, sizeof in);
                t.H = H, t.W = W;
                long long size, uv_off = 0;
                if (lay.format == 2) {
                    t.nv12 = 1, t.sy = W + lay.pad, t.sx = 1, t.uv_stride = W + lay.pad;
                    const long long ys = plane_span(H, W, t.sy);
                    size = ys + plane_span(H / 2, W, t.uv_stride);  // the UV plane directly behind the Y plane's last byte
                    uv_off = ys;
                } else {
                    t.sx = lay.sx, t.sy = (lay.sc ? lay.sx * W : W) + lay.pad, t.sc = lay.sc ? lay.sc : t.sy * H + 3;
                    size = span_of(H, W, t.sy, t.sx, t.sc);
                }
                uint8_t* blk = (uint8_t*)malloc((size_t)size);
                for (long long i = 0; i < size; i++) blk[i] = (uint8_t)(0x40 + (i * 2654435761u >> 13) % 64);
                std::vector<uint8_t> before(blk, blk + size);
                t.data = blk;
                if (t.nv12) t.uv = blk + uv_off;
                overlay_colours(&t, lay.format == 1, OVERLAY_LIMB_BGR, OVERLAY_RECT_BGR);
                for (int i = 0; i < OVERLAY_NJ; i++) in.parents[i] = OVERLAY_PARENTS[i];
                for (int i = 0; i < OVERLAY_NJ; i++) {  // a fan of joints around a centre that moves over the frame's edges with the case
                    const double ang_r[4] = {-1.0, 1.0, 0.5, -0.25}, ang_c[4] = {1.0, 0.5, -1.0, -1.0};
                    const double cr = (cse % 3 - 0.5) * H * 0.75, cc = ((cse / 3) % 4 - 1) * W * 0.5;
                    in.j2d[2 * i] = cr + ang_r[i & 3] * (3.5 + 2.25 * i), in.j2d[2 * i + 1] = cc + ang_c[(i + 1) & 3] * (2.5 + 1.75 * i);
                }
                in.has_rect = 1;
                in.rect[0] = (cse % 4 - 1) * (W / 2) - 1, in.rect[1] = (cse / 4 - 1) * (H / 2) - 1, in.rect[2] = 1 + (cse * 7) % (W + 6), in.rect[3] = 1 + (cse * 5) % (H + 6);
                walk(t, in);
                const long long b = check(blk, before, t, in, size);
                bad += b;
                for (long long i = 0; i < size; i++) drawn += blk[i] != before[(size_t)i];
                if (b) printf("overlay sweep: %s %dx%d case %d: %lld bytes differ\n", lay.name, H, W, cse, b);
                free(blk);
                walks++;
            }
        }
    printf("overlay sweep: %lld walks, %lld bytes drawn, %lld mismatches\n", walks, drawn, bad);
    return (bad || !drawn) ? 1 : 0;
}
#endif
