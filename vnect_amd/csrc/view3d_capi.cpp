// view3d_capi.cpp -- C shim over view3d.h for tests/test_view3d_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.
// Built with plain g++ (`make -C vnect_amd/csrc view3d`).  view3d_walk goes through a picture the way the kernel of view3d.hip does --
// tile by tile, the limbs set up, culled against the tile and listed from the lowest rank to the highest, then lane by lane, four pixels
// and one preview_store each -- with the SAME functions for the projection, the inside test, the ranking and the stores, so the rule as
// the device runs it is held to independent statements of it without a GPU.  Stores go straight to the caller's buffer: with
// -DVIEW3D_SWEEP_MAIN (`make ... view3d_sweep_asan`, -fsanitize=address,undefined) the same file is a stand-alone program whose outputs
// sit in exactly sized heap blocks, and a store outside the picture's rows is the sanitizer's finding.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "view3d.h"

using namespace vnect;

namespace {

void walk(const View3dArgs& a, const float* j3d, const double* conf)
{
    View3dLimb L[VIEW3D_NJ];
    int rank[VIEW3D_NJ], byrank[VIEW3D_NJ];
    for (int i = 0; i < VIEW3D_NJ; i++) L[i] = view3d_limb_of(a, j3d, conf, i), byrank[i] = -1;
    for (int i = 0; i < VIEW3D_NJ; i++) {  // wave 0's counting compares
        rank[i] = 0;
        for (int j = 0; j < VIEW3D_NJ; j++) rank[i] += (!L[j].skip && !L[i].skip && j != i && view3d_over(a.order, L[i].key, i, L[j].key, j)) ? 1 : 0;
        if (!L[i].skip) byrank[rank[i]] = i;
    }
    for (int dy0 = 0; dy0 < a.rows; dy0 += VIEW3D_TILE_H)
        for (int dx0 = 0; dx0 < a.cols; dx0 += VIEW3D_TILE_W) {
            const int dy1 = (dy0 + VIEW3D_TILE_H < a.rows ? dy0 + VIEW3D_TILE_H : a.rows) - 1, dx1 = (dx0 + VIEW3D_TILE_W < a.cols ? dx0 + VIEW3D_TILE_W : a.cols) - 1;
            int live[VIEW3D_NJ], n = 0;
            for (int r = 0; r < VIEW3D_NJ; r++)  // (lane r holds rank r's limb; the ballot keeps the lanes' order)
                if (byrank[r] >= 0 && view3d_limb_near(L[byrank[r]], a.grow, dy0, dy1, dx0, dx1)) live[n++] = byrank[r];
            for (int tid = 0; tid < VIEW3D_THREADS; tid++) {
                const int dy = dy0 + tid / VIEW3D_LANES_X, dx = dx0 + (tid % VIEW3D_LANES_X) * VIEW3D_LANE_PX;
                if (dy > dy1 || dx > dx1) continue;
                view3d_lane(a, L, live, n, dy, dx);
            }
        }
}

}  // namespace

extern "C" {

// [0] the tile's width and [1] height in pixels, [2] lanes per workgroup, [3] pixels per lane, [4] the largest side
void view3d_tile(int32_t* out) { out[0] = VIEW3D_TILE_W, out[1] = VIEW3D_TILE_H, out[2] = VIEW3D_THREADS, out[3] = VIEW3D_LANE_PX, out[4] = VIEW3D_MAX; }

// the default colour table as BGR, 21 x 3
void view3d_default_colors(int32_t* out)
{
    for (int i = 0; i < VIEW3D_NJ; i++)
        for (int c = 0; c < 3; c++) out[3 * i + c] = VIEW3D_CYCLE_BGR[i % 10][c];
}

// The view of j3d (21 x 3 float32) into the picture whose pixel (0, 0) lies out_off bytes into [out, out + out_size), rows out_pitch
// apart.  A zero rows / cols / extent / line_width and a null view9 / background_bgr / colors_bgr (21 x 3) / parents mean the default; conf
// may be null (then a threshold applies to nothing); min_conf NaN: no threshold.  Returns 0, or -1 for arguments the runtime would refuse
// (then nothing is written).
int view3d_walk(const float* j3d, const double* conf, int rows, int cols, double extent, const double* view9, double line_width, const int32_t* background_bgr,
                const int32_t* colors_bgr, const int32_t* parents, double min_conf, int out_format, int order, uint8_t* out, int64_t out_size, int64_t out_off,
                int64_t out_pitch)
{
    View3dArgs a;
    const View3dSpecIn s = {rows, cols, extent, view9, line_width, background_bgr, (const int (*)[3])colors_bgr, parents, min_conf, out_format, order};
    if (!j3d || view3d_setup(s, OVERLAY_PARENTS, &a)) return -1;
    if (!out || out_off < 0 || out_pitch < 3LL * a.cols) return -1;
    if (out_off + (int64_t)(a.rows - 1) * out_pitch + 3LL * a.cols > out_size) return -1;
    if (!conf) a.has_conf = 0;
    a.out = out + out_off, a.pitch = out_pitch;
    if (!view3d_args_ok(a)) return -1;
    walk(a, j3d, conf);
    return 0;
}

}  // extern "C"

#ifdef VIEW3D_SWEEP_MAIN
// Sizes x pitches x formats x orders x views: every output in a block of exactly (rows - 1) pitch + 3 cols bytes -- a store behind the
// last row is the sanitizer's finding.  Every walk is also held to a plain per-pixel statement of the rule (no tiles, no cull, no ranking,
// no dword stores), and the pitch padding to its canary.
int main()
{
    const int sizes[][2] = {{1, 1}, {1, 7}, {33, 65}, {65, 33}, {400, 400}, {17, 129}};
    const int pads[] = {0, 1, 5};
    const double views[3][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.8, -0.6, 0, 0.36, 0.48, -0.8, 0.48, 0.64, 0.6}, {1, 0, 0, 0, 0, 1, 0, -1, 0}};
    long long walks = 0, bad = 0, drawn = 0;
    for (const auto& hw : sizes)
        for (int pad : pads)
            for (int cse = 0; cse < 12; cse++) {
                const int rows = hw[0], cols = hw[1], fmt = cse & 1, order = (cse >> 1) & 1, vi = cse % 3;
                const double extent = cse % 4 == 3 ? 40.0 : 500.0, w = cse % 5 == 4 ? 7.5 : 3.0;
                float j3d[VIEW3D_NJ * 3];
                for (int i = 0; i < VIEW3D_NJ; i++) {
                    j3d[3 * i] = (float)(((i * 37 + cse * 11) % 97 - 48) * extent / 45.0);
                    j3d[3 * i + 1] = (float)(((i * 53 + cse * 7) % 89 - 44) * extent / 45.0);
                    j3d[3 * i + 2] = (float)(((i * 29 + cse * 5) % 83 - 41) * extent / 45.0);
                }
                if (cse == 5) j3d[3 * 4] = NAN, j3d[3 * 9 + 1] = INFINITY, j3d[3 * 12] = 3e9f;
                double conf[VIEW3D_NJ];
                for (int i = 0; i < VIEW3D_NJ; i++) conf[i] = (i * 7 % 10) / 10.0;
                const double min_conf = cse == 7 ? 0.25 : NAN;
                const long long pitch = 3LL * cols + pad, osize = (long long)(rows - 1) * pitch + 3LL * cols;
                uint8_t* out = (uint8_t*)malloc((size_t)osize);
                memset(out, 0xA5, (size_t)osize);
                const int rc = view3d_walk(j3d, conf, rows, cols, extent, views[vi], w, nullptr, nullptr, nullptr, min_conf, fmt, order, out, osize, 0, pitch);
                if (rc) {
                    printf("view3d sweep: %dx%d case %d: refused\n", rows, cols, cse);
                    bad++;
                }
                View3dArgs a;
                const View3dSpecIn s = {rows, cols, extent, views[vi], w, nullptr, nullptr, nullptr, min_conf, fmt, order};
                if (view3d_setup(s, OVERLAY_PARENTS, &a)) bad++;
                View3dLimb L[VIEW3D_NJ];
                for (int i = 0; i < VIEW3D_NJ; i++) L[i] = view3d_limb_of(a, j3d, conf, i);
                long long b = 0;
                for (int y = 0; y < rows; y++) {
                    for (int x = 0; x < cols; x++) {
                        int sel = -1;
                        for (int i = 0; i < VIEW3D_NJ; i++)
                            if (!L[i].skip && view3d_inside(L[i], a.r2, y, x) && (sel < 0 || view3d_over(order, L[i].key, i, L[sel].key, sel))) sel = i;
                        drawn += sel >= 0;
                        for (int c = 0; c < 3; c++) {
                            const int want = sel < 0 ? 255 : VIEW3D_CYCLE_BGR[sel % 10][fmt ? 2 - c : c];
                            b += out[(size_t)y * pitch + 3 * x + c] != want;
                        }
                    }
                    if (y + 1 < rows)
                        for (long long q = 3LL * cols; q < pitch; q++) b += out[(size_t)y * pitch + q] != 0xA5;
                }
                if (b) printf("view3d sweep: %dx%d pad %d case %d: %lld bytes differ\n", rows, cols, pad, cse, b);
                bad += b;
                free(out);
                walks++;
            }
    printf("view3d sweep: %lld walks, %lld limb pixels, %lld mismatches\n", walks, drawn, bad);
    return (bad || !walks || !drawn) ? 1 : 0;
}
#endif
