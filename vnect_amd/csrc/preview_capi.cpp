// preview_capi.cpp -- C shim over preview.h for tests/test_preview_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.
// Built with plain g++ (`make -C vnect_amd/csrc preview`).  preview_walk goes through an output the way the kernel of preview.hip does --
// tile by tile, the limbs and the band culled against the tile's footprint in the picture, then lane by lane, four pixels and one
// preview_store each -- with the SAME functions for the taps, the blend and the stores, so the rule as the device runs it is held to
// independent statements of it without a GPU.  Loads and stores go straight to the caller's buffers: with -DPREVIEW_SWEEP_MAIN
// (`make ... preview_sweep_asan`, -fsanitize=address,undefined) the same file is a stand-alone program whose sources and outputs sit in
// exactly sized heap blocks, and a load outside the frame or a store outside the output's rows is the sanitizer's finding.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "preview.h"

using namespace vnect;

namespace {

void walk(const PreviewArgs& a, const OverlayInput& in)
{
    OverlayLimb L[OVERLAY_NJ];
    for (int i = 0; i < OVERLAY_NJ; i++) L[i] = preview_limb_of(a, in.j2d, in.conf, in.has_conf != 0, in.min_conf, in.parents, i);
    for (int dy0 = 0; dy0 < a.g.dh; dy0 += PREVIEW_TILE_H)
        for (int dx0 = 0; dx0 < a.g.dw; dx0 += PREVIEW_TILE_W) {
            const int dy1 = (dy0 + PREVIEW_TILE_H < a.g.dh ? dy0 + PREVIEW_TILE_H : a.g.dh) - 1, dx1 = (dx0 + PREVIEW_TILE_W < a.g.dw ? dx0 + PREVIEW_TILE_W : a.g.dw) - 1;
            long long y0, y1, x0, x1;
            preview_footprint(a.g, dy0, dy1, dx0, dx1, &y0, &y1, &x0, &x1);
            OverlayBand band = overlay_band(in.has_rect != 0, in.rect[0], in.rect[1], in.rect[2], in.rect[3]);
            if (!overlay_band_near(band, y0, y1, x0, x1)) band.on = 0;
            int live[OVERLAY_NJ], n = 0;
            for (int i = 0; i < OVERLAY_NJ; i++)
                if (overlay_limb_near(L[i], y0, y1, x0, x1)) live[n++] = i;
            for (int tid = 0; tid < PREVIEW_THREADS; tid++) {
                const int dy = dy0 + tid / PREVIEW_LANES_X, dx = dx0 + (tid % PREVIEW_LANES_X) * PREVIEW_LANE_PX;
                if (dy > dy1 || dx > dx1) continue;
                preview_lane(a, L, live, n, band, dy, dx);
            }
        }
}

// the frame's description -> a.src, a.H, a.W, a.o; false: a frame the runtime would refuse
bool source_of(PreviewArgs* a, const uint8_t* base, int64_t size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx,
               int64_t sc, int64_t uv_stride, int orient)
{
    if (!base || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24) || data_off < 0 || format < 0 || format > 2 || !orient_ok(orient)) return false;
    if (format == 2) {
        if (((H | W) & 1) || sy < W || uv_stride < W || uv_off < 0) return false;
        if (data_off + (int64_t)(H - 1) * sy + W > size || uv_off + (int64_t)(H / 2 - 1) * uv_stride + W > size) return false;
    } else if (sy < 1 || sx < 1 || sc < 1 || data_off + ingest_span(H, W, sy, sx, sc) > size)
        return false;
    a->src = preview_source(format == 2, format == 1, base + data_off, base + uv_off, sy, sx, sc, uv_stride);
    a->H = H, a->W = W, a->o = orient;
    return true;
}

}  // namespace

extern "C" {

// [0] the tile's width and [1] height in output pixels, [2] lanes per workgroup, [3] pixels per lane
void preview_tile(int32_t* out) { out[0] = PREVIEW_TILE_W, out[1] = PREVIEW_TILE_H, out[2] = PREVIEW_THREADS, out[3] = PREVIEW_LANE_PX; }

// the output's (rows, columns) of a stored (H, W) frame under `orient` at `factor`; 0, or preview.h's refusal code
int preview_size(int orient, int H, int W, double factor, int32_t* out_hw)
{
    if (!orient_ok(orient) || H < 1 || W < 1) return -1;
    PreviewGeom g;
    const int rc = preview_geom(orient, H, W, factor, &g);
    if (rc == PREVIEW_OK) out_hw[0] = g.dh, out_hw[1] = g.dw;
    return rc;
}

// The preview of the frame whose pixel (0, 0) channel 0 (NV12: Y plane) lies data_off bytes into [src, src + src_size), the UV plane
// uv_off bytes in; format 0 BGR, 1 RGB, 2 NV12; src_has_rect: the descriptor carries a rect.  j2d / conf / parents / rect4 / limb_bgr /
// rect_bgr may be null.  The output's pixel (0, 0) lies out_off bytes into [out, out + out_size), rows out_pitch apart, out_format 0 BGR,
// 1 RGB.  Returns 0, or -1 for arguments the runtime would refuse (then nothing is read or written).
int preview_walk(const uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
                 int64_t uv_stride, int src_has_rect, int orient, const double* j2d, const double* conf, double min_conf, const int32_t* parents,
                 const int32_t* rect4, const int32_t* limb_bgr, const int32_t* rect_bgr, double factor, int out_format, uint8_t* out, int64_t out_size,
                 int64_t out_off, int64_t out_pitch)
{
    PreviewArgs a;
    OverlayInput in;
    memset(&a, 0, sizeof a);
    memset(&in, 0, sizeof in);
    if (src_has_rect || !source_of(&a, src, src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, orient)) return -1;
    if (preview_geom(orient, H, W, factor, &a.g) != PREVIEW_OK) return -1;
    if (!out || out_off < 0 || (out_format != 0 && out_format != 1) || out_pitch < 3LL * a.g.dw) return -1;
    if (out_off + (int64_t)(a.g.dh - 1) * out_pitch + 3LL * a.g.dw > out_size) return -1;
    if ((uintptr_t)out < (uintptr_t)src + (uintptr_t)src_size && (uintptr_t)src < (uintptr_t)out + (uintptr_t)out_size) return -1;  // the output overlaps the source
    int lc[3], rc[3];
    for (int k = 0; k < 3; k++) {
        lc[k] = limb_bgr ? limb_bgr[k] : OVERLAY_LIMB_BGR[k], rc[k] = rect_bgr ? rect_bgr[k] : OVERLAY_RECT_BGR[k];
        if (lc[k] < 0 || lc[k] > 255 || rc[k] < 0 || rc[k] > 255) return -1;
    }
    preview_colours(&a, lc, rc);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        in.parents[i] = parents ? parents[i] : OVERLAY_PARENTS[i];
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return -1;
    }
    if (j2d) memcpy(in.j2d, j2d, sizeof in.j2d), a.has_joints = 1;
    if (conf) memcpy(in.conf, conf, sizeof in.conf), in.min_conf = min_conf, in.has_conf = min_conf == min_conf;
    if (rect4) {
        if (rect4[2] < 1 || rect4[3] < 1) return -1;
        for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
        in.has_rect = 1;
    }
    a.out = out + out_off, a.pitch = out_pitch, a.out_rgb = out_format;
    walk(a, in);
    return 0;
}

// The people form (preview.h: PreviewPeople; PEOPLE.md), walked as preview_people_kernel goes: per tile every person's band and limbs
// culled against the footprint, then the lanes.  preview_walk's arguments, but P persons (1 .. 4): j2d holds P x 42 doubles, conf P x 21
// (or null), rects P x 4 (every person has a rect, as a tracked frame has), drawn P flags (or null: everybody; 0: the person is left
// out, as one whose crop was refused).
int preview_walk_people(const uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
                        int64_t uv_stride, int orient, int P, const double* j2d, const double* conf, double min_conf, const int32_t* parents,
                        const int32_t* rects, const int32_t* drawn, const int32_t* limb_bgr, const int32_t* rect_bgr, double factor, int out_format,
                        uint8_t* out, int64_t out_size, int64_t out_off, int64_t out_pitch)
{
    PreviewArgs a;
    memset(&a, 0, sizeof a);
    if (P < 1 || P > PREVIEW_MAX_PEOPLE || !j2d || !rects) return -1;
    if (!source_of(&a, src, src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, orient)) return -1;
    if (preview_geom(orient, H, W, factor, &a.g) != PREVIEW_OK) return -1;
    if (!out || out_off < 0 || (out_format != 0 && out_format != 1) || out_pitch < 3LL * a.g.dw) return -1;
    if (out_off + (int64_t)(a.g.dh - 1) * out_pitch + 3LL * a.g.dw > out_size) return -1;
    if ((uintptr_t)out < (uintptr_t)src + (uintptr_t)src_size && (uintptr_t)src < (uintptr_t)out + (uintptr_t)out_size) return -1;
    int lc[3], rc[3], par[OVERLAY_NJ];
    for (int k = 0; k < 3; k++) {
        lc[k] = limb_bgr ? limb_bgr[k] : OVERLAY_LIMB_BGR[k], rc[k] = rect_bgr ? rect_bgr[k] : OVERLAY_RECT_BGR[k];
        if (lc[k] < 0 || lc[k] > 255 || rc[k] < 0 || rc[k] > 255) return -1;
    }
    preview_colours(&a, lc, rc);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        par[i] = parents ? parents[i] : OVERLAY_PARENTS[i];
        if (par[i] < 0 || par[i] >= OVERLAY_NJ) return -1;
    }
    for (int p = 0; p < P; p++)
        if (rects[4 * p + 2] < 1 || rects[4 * p + 3] < 1) return -1;
    const bool has_conf = conf && min_conf == min_conf;
    a.has_joints = 1, a.out = out + out_off, a.pitch = out_pitch, a.out_rgb = out_format;
    OverlayLimb L[PREVIEW_MAX_PEOPLE * OVERLAY_NJ];
    for (int p = 0; p < P; p++)
        for (int i = 0; i < OVERLAY_NJ; i++)
            L[p * OVERLAY_NJ + i] = preview_limb_of(a, j2d + p * OVERLAY_NJ * 2, conf ? conf + p * OVERLAY_NJ : nullptr, has_conf, min_conf, par, i);
    for (int dy0 = 0; dy0 < a.g.dh; dy0 += PREVIEW_TILE_H)
        for (int dx0 = 0; dx0 < a.g.dw; dx0 += PREVIEW_TILE_W) {
            const int dy1 = (dy0 + PREVIEW_TILE_H < a.g.dh ? dy0 + PREVIEW_TILE_H : a.g.dh) - 1, dx1 = (dx0 + PREVIEW_TILE_W < a.g.dw ? dx0 + PREVIEW_TILE_W : a.g.dw) - 1;
            long long y0, y1, x0, x1;
            preview_footprint(a.g, dy0, dy1, dx0, dx1, &y0, &y1, &x0, &x1);
            OverlayBand band[PREVIEW_MAX_PEOPLE];
            int live[PREVIEW_MAX_PEOPLE * OVERLAY_NJ], nlive[PREVIEW_MAX_PEOPLE];
            for (int p = 0; p < P; p++) {
                const bool on = !drawn || drawn[p];
                band[p] = overlay_band(on, on ? rects[4 * p] : 0, on ? rects[4 * p + 1] : 0, on ? rects[4 * p + 2] : 0, on ? rects[4 * p + 3] : 0);
                if (!overlay_band_near(band[p], y0, y1, x0, x1)) band[p].on = 0;
                nlive[p] = 0;
                for (int i = 0; i < OVERLAY_NJ && on; i++)
                    if (overlay_limb_near(L[p * OVERLAY_NJ + i], y0, y1, x0, x1)) live[p * OVERLAY_NJ + nlive[p]++] = i;
            }
            const PreviewPeople scene{P, L, live, nlive, band};
            for (int tid = 0; tid < PREVIEW_THREADS; tid++) {
                const int dy = dy0 + tid / PREVIEW_LANES_X, dx = dx0 + (tid % PREVIEW_LANES_X) * PREVIEW_LANE_PX;
                if (dy > dy1 || dx > dx1) continue;
                preview_lane_of(a, scene, dy, dx);
            }
        }
    return 0;
}

}  // extern "C"

#ifdef PREVIEW_SWEEP_MAIN
// Layouts x orientations x factors x overlay cases: every source in an exactly sized heap block (its first pixel byte at the block's
// first, its last at the block's last) and every output in a block of exactly (dh - 1) pitch + 3 dw bytes -- a load outside the frame or a
// store behind the last row is the sanitizer's finding.  Every walk is also held to a plain per-pixel statement of the rule (no tiles, no
// cull, no dword stores), and the pitch padding to its canary.
namespace {

struct Layout { int format; long long sx, sc; int pad; const char* name; };

}  // namespace

int main()
{
    const Layout layouts[] = {{0, 3, 1, 0, "packed-3"}, {0, 3, 1, 5, "packed-3 padded"}, {1, 4, 1, 0, "packed-4 rgb"}, {0, 1, 0, 3, "planar"},
                              {0, 5, 2, 1, "generic"},  {2, 1, 0, 0, "nv12"},            {2, 1, 0, 6, "nv12 pitched"}};
    const int sizes[][2] = {{37, 53}, {1, 1}, {3, 129}, {66, 8}, {34, 70}};
    const double factors[] = {0.5, 0.37, 1.0 / 3.0, 1.0, 1.7, 0.0, 0.06, 3.9};
    long long walks = 0, bad = 0, refused = 0, annotated = 0;
    for (const Layout& lay : layouts)
        for (const auto& hw : sizes)
            for (int cse = 0; cse < 16; cse++) {
                int H = hw[0], W = hw[1];
                if (lay.format == 2) H = (H + 1) & ~1, W = (W + 1) & ~1;
                const int o = cse & 7;
                const double f = factors[(cse * 3 + (int)(&hw - &sizes[0])) % 8];
                long long sy, sx = 1, sc = 0, uvs = 0, size, uv_off = 0;
                if (lay.format == 2) {
                    sy = uvs = W + lay.pad;
                    const long long ys = (long long)(H - 1) * sy + W;
                    size = ys + (long long)(H / 2 - 1) * uvs + W, uv_off = ys;
                } else {
                    sx = lay.sx, sy = (lay.sc ? lay.sx * W : W) + lay.pad, sc = lay.sc ? lay.sc : sy * H + 3;
                    size = ingest_span(H, W, sy, sx, sc);
                }
                uint8_t* blk = (uint8_t*)malloc((size_t)size);
                for (long long i = 0; i < size; i++) blk[i] = (uint8_t)((i * 2654435761u >> 11) % 251);
                PreviewGeom g;
                if (preview_geom(o, H, W, f, &g) != PREVIEW_OK) {
                    refused++;
                    free(blk);
                    continue;
                }
                const long long pitch = 3LL * g.dw + (cse % 3) * 5, osize = (long long)(g.dh - 1) * pitch + 3LL * g.dw;
                uint8_t* out = (uint8_t*)malloc((size_t)osize);
                memset(out, 0xA5, (size_t)osize);
                double j2d[OVERLAY_NJ * 2];
                for (int i = 0; i < OVERLAY_NJ; i++) {  // a fan of joints around a centre that moves over the picture's edges with the case
                    const double ang_r[4] = {-1.0, 1.0, 0.5, -0.25}, ang_c[4] = {1.0, 0.5, -1.0, -1.0};
                    const double cr = (cse % 3 - 0.5) * g.Hp * 0.75, cc = ((cse / 3) % 4 - 1) * g.Wp * 0.5;
                    j2d[2 * i] = cr + ang_r[i & 3] * (3.5 + 2.25 * i), j2d[2 * i + 1] = cc + ang_c[(i + 1) & 3] * (2.5 + 1.75 * i);
                }
                const int32_t rect[4] = {(cse % 4 - 1) * (g.Wp / 2) - 1, (cse / 4 - 1) * (g.Hp / 2) - 1, 1 + (cse * 7) % (g.Wp + 6), 1 + (cse * 5) % (g.Hp + 6)};
                const bool plain = cse == 15;
                const int rc = preview_walk(blk, size, 0, uv_off, lay.format, H, W, sy, sx, sc, uvs, 0, o, plain ? nullptr : j2d, nullptr, 0.0, nullptr,
                                            plain ? nullptr : rect, nullptr, nullptr, f, cse & 1, out, osize, 0, pitch);
                if (rc) {
                    printf("preview sweep: %s %dx%d case %d: refused\n", lay.name, H, W, cse);
                    bad++;
                }
                // the plain statement: A per pixel, then the project's resize per output pixel
                PreviewArgs a;
                memset(&a, 0, sizeof a);
                a.src = preview_source(lay.format == 2, lay.format == 1, blk, blk + uv_off, sy, sx, sc, uvs), a.H = H, a.W = W, a.o = o, a.g = g;
                preview_colours(&a, nullptr, nullptr);
                std::vector<int> A((size_t)g.Hp * g.Wp * 3), P(A.size());
                OverlayLimb L[OVERLAY_NJ];
                for (int i = 0; i < OVERLAY_NJ; i++) L[i] = overlay_limb_of(j2d, nullptr, false, 0.0, OVERLAY_PARENTS, i);
                const OverlayBand band = overlay_band(!plain, rect[0], rect[1], rect[2], rect[3]);
                for (int i = 0; i < g.Hp; i++)
                    for (int j = 0; j < g.Wp; j++) {
                        int* p = &A[((size_t)i * g.Wp + j) * 3];
                        preview_src_pixel(a.src, o, H, W, i, j, p);
                        memcpy(&P[((size_t)i * g.Wp + j) * 3], p, 3 * sizeof(int));
                        int s = OVERLAY_NONE;
                        if (!plain)
                            for (int k = 0; k < OVERLAY_NJ; k++)
                                if (!L[k].skip && overlay_inside(L[k], i, j)) s = OVERLAY_LIMB;
                        if (overlay_in_band(band, i, j)) s = OVERLAY_BAND;
                        if (s) p[0] = a.col[s - 1][0], p[1] = a.col[s - 1][1], p[2] = a.col[s - 1][2], annotated++;
                    }
                long long b = 0;
                for (int dy = 0; dy < g.dh; dy++) {
                    for (int q = 0; q < 3 * g.dw; q++) {
                        const int dx = q / 3, c = (cse & 1) ? 2 - q % 3 : q % 3;
                        int want;
                        if (g.copy) want = A[((size_t)dy * g.Wp + dx) * 3 + c];
                        else {
                            const AxE x = axis_x_at(dx, g.Wp, g.scale), y = axis_y_at(dy, g.Hp, g.scale);
                            auto px = [&](int r, int cc) { return A[((size_t)r * g.Wp + cc) * 3 + c]; };
                            const int a0 = crop_sat((1.f - x.f) * 2048.f), a1 = crop_sat(x.f * 2048.f), b0 = crop_sat((1.f - y.f) * 2048.f), b1 = crop_sat(y.f * 2048.f);
                            const int r0 = x.edge ? px(y.s0, x.s0) * 2048 : px(y.s0, x.s0) * a0 + px(y.s0, x.s0 + 1) * a1;
                            const int r1 = x.edge ? px(y.s1, x.s0) * 2048 : px(y.s1, x.s0) * a0 + px(y.s1, x.s0 + 1) * a1;
                            want = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                        }
                        b += out[(size_t)dy * pitch + q] != want;
                    }
                    if (dy + 1 < g.dh)
                        for (long long q = 3LL * g.dw; q < pitch; q++) b += out[(size_t)dy * pitch + q] != 0xA5;
                }
                if (b) printf("preview sweep: %s %dx%d code %d factor %g case %d: %lld bytes differ\n", lay.name, H, W, o, f, cse, b);
                bad += b;
                free(out), free(blk);
                walks++;
            }
    printf("preview sweep: %lld walks, %lld refused sizes, %lld annotated source pixels, %lld mismatches\n", walks, refused, annotated, bad);
    return (bad || !walks || !annotated) ? 1 : 0;
}
#endif
