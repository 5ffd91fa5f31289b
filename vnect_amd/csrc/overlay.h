// overlay.h -- the skeleton and the crop rectangle drawn into a uint8 frame (the reference: utils.draw_limbs_2d, src/utils.py:222-243, called
// by the frame loop at run_estimator_ps.py:92-94): the drawing RULE, ONE source for host and device (as nv12.h, ingest.h and crop.h are).
// The kernel of overlay.hip and the host walk of overlay_capi.cpp (tests/test_overlay_cpu.py, and the sanitizer sweep) call the same
// functions: a limb's set-up, the inside test, the band test, the chroma decision of an NV12 block, the colour
// conversion, and the tests and stores of one lane.  The rule (OVERLAY.md) is this project's own: cv2 rounds the limb's angle to whole degrees and
// fills a polygon, which cannot be pinned without cv2; this uses float64 multiplies, adds and compares only -- no trigonometry, no
// division, and (built with contraction off) no fused multiply-add -- so numpy, g++ and the GPU agree bit for bit.  HIP-free under g++.
#pragma once
#include <math.h>
#include <stdint.h>

#include "axis.h"  // VNECT_HD

namespace vnect {

constexpr int OVERLAY_NJ = 21;
// The kernel's tile, in CELLS: a cell is one pixel (BGR / RGB) or one 2 x 2 block (NV12: a lane owns a chroma sample and its four Y bytes).
// 256 lanes own a 64 x 32 tile, eight cells each (rows ty, ty + 4, .. ty + 28 of column tx).
constexpr int OVERLAY_TILE_W = 64, OVERLAY_TILE_H = 32, OVERLAY_THREADS = 256;
constexpr int OVERLAY_LANE_STEP = OVERLAY_THREADS / OVERLAY_TILE_W;     // rows between a lane's cells: 4
constexpr int OVERLAY_LANE_ROWS = OVERLAY_TILE_H / OVERLAY_LANE_STEP;   // cells of a lane: 8
constexpr double OVERLAY_COORD_MAX = 1048576.0;  // 2^20: a joint further out (or non-finite) skips its limbs
constexpr int OVERLAY_LIMB_BGR[3] = {49, 22, 122};  // src/utils.py:236
constexpr int OVERLAY_RECT_BGR[3] = {60, 66, 207};  // src/utils.py:241
// VNectEstimator.joint_parents (src/estimator.py): limb i joins joint i to joint OVERLAY_PARENTS[i]; the root (14) is its own parent
constexpr int OVERLAY_PARENTS[OVERLAY_NJ] = {16, 15, 1, 2, 3, 1, 5, 6, 14, 8, 9, 14, 11, 12, 14, 14, 1, 4, 7, 10, 13};
enum { OVERLAY_NONE = 0, OVERLAY_LIMB = 1, OVERLAY_BAND = 2 };  // a pixel's state; the greater wins (the reference draws the rectangle last)

// One limb, set up once: joint (r1, c1) to its parent (r2, c2).  src/utils.py:229-235 in this rule's terms.
struct OverlayLimb {
    double dr, dc, L2;  // the limb's vector and its squared length
    double aa;          // a^2, a = the half-axis along the limb: the largest integer >= 0 with 4 a^2 <= L2 (int(length / 2), :233)
    double rhs;         // (aa * 9) * L2, the inside test's right-hand side
    double cr, cc;      // the centre, rounded half-to-even (Python's round, :232)
    double m;           // max(a, 3): no pixel further than this from the centre in either axis is inside
    int skip;
};

VNECT_HD bool overlay_coord_ok(double v) { return v >= -OVERLAY_COORD_MAX && v <= OVERLAY_COORD_MAX; }  // (false for NaN and both infinities)

// low: a confidence threshold is set and one end's confidence lies below it
VNECT_HD OverlayLimb overlay_limb(double r1, double c1, double r2, double c2, bool low)
{
    OverlayLimb l;
    l.dr = l.dc = l.L2 = l.aa = l.rhs = l.cr = l.cc = l.m = 0.0;
    l.skip = 1;
    if (low || !overlay_coord_ok(r1) || !overlay_coord_ok(c1) || !overlay_coord_ok(r2) || !overlay_coord_ok(c2)) return l;
    l.dr = r1 - r2, l.dc = c1 - c2;
    l.L2 = l.dr * l.dr + l.dc * l.dc;
    // a from sqrt, then held to its definition by two comparisons: however sqrt rounds, it is at most one off (4 a^2 is exact: a < 2^21)
    double a = floor(sqrt(l.L2) * 0.5);
    if (4.0 * a * a > l.L2) a -= 1.0;
    if (4.0 * (a + 1.0) * (a + 1.0) <= l.L2) a += 1.0;
    if (!(a >= 1.0)) return l;  // the root joint (its own parent) and limbs under 2 px: nothing drawn (cv2 draws a sliver)
    l.aa = a * a;
    l.rhs = (l.aa * 9.0) * l.L2;
    l.cr = rint((r1 + r2) * 0.5), l.cc = rint((c1 + c2) * 0.5);
    l.m = a > 3.0 ? a : 3.0;
    l.skip = 0;
    return l;
}

// The ellipse of :232-235, half-axes (a, 3) along the limb: every operand float64, in exactly this order
VNECT_HD bool overlay_inside(const OverlayLimb& l, int y, int x)
{
    const double u = (double)y - l.cr, v = (double)x - l.cc;
    const double s = u * l.dr + v * l.dc, t = u * l.dc - v * l.dr;
    return (s * s) * 9.0 + (t * t) * l.aa <= l.rhs;
}
// Can any pixel of rows [y0, y1], columns [x0, x1] be inside?  Two conservative culls, each a pixel wider than it has to be (so that their
// own rounding cannot matter; neither takes part in the rule): the bounding box of radius m, and the limb's own frame -- a pixel inside has
// |t| <= 3 |limb| and |s| <= a |limb|, and s and t of a pixel differ from the box centre's by at most R |limb|, R the centre's distance
// to the box's corners (bounded here by the sum of the half extents).
VNECT_HD bool overlay_limb_near(const OverlayLimb& l, long long y0, long long y1, long long x0, long long x1)
{
    const double m = l.m + 1.0;
    if (l.skip || !((double)y1 >= l.cr - m && (double)y0 <= l.cr + m && (double)x1 >= l.cc - m && (double)x0 <= l.cc + m)) return false;
    const double u = ((double)y0 + (double)y1) * 0.5 - l.cr, v = ((double)x0 + (double)x1) * 0.5 - l.cc;
    const double R = ((double)(y1 - y0) + (double)(x1 - x0)) * 0.5 + 1.0, len = sqrt(l.L2);
    return fabs(u * l.dc - v * l.dr) <= (3.0 + R) * len && fabs(u * l.dr + v * l.dc) <= (sqrt(l.aa) + R) * len;
}

// The rectangle's outline, thickness 4 (:241): 2 px outside (x0, y0) .. (x0 + w - 1, y0 + h - 1) and 2 px inside
struct OverlayBand {
    long long x0, y0, x1, y1;  // the outer box, inclusive
    long long ix0, iy0, ix1, iy1;  // the inner exclusion, inclusive (empty where ix1 < ix0 or iy1 < iy0)
    int on;
};
VNECT_HD OverlayBand overlay_band(bool on, long long x, long long y, long long w, long long h)
{
    OverlayBand b;
    b.on = on ? 1 : 0;
    b.x0 = x - 2, b.x1 = x + w + 1, b.y0 = y - 2, b.y1 = y + h + 1;
    b.ix0 = x + 2, b.ix1 = x + w - 3, b.iy0 = y + 2, b.iy1 = y + h - 3;
    return b;
}
VNECT_HD bool overlay_in_band(const OverlayBand& b, long long y, long long x)
{
    return b.on && x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1 && !(x >= b.ix0 && x <= b.ix1 && y >= b.iy0 && y <= b.iy1);
}
// can any pixel of rows [y0, y1], columns [x0, x1] be in the band?  Yes unless the box lies outside the outer box or inside the exclusion
VNECT_HD bool overlay_band_near(const OverlayBand& b, long long y0, long long y1, long long x0, long long x1)
{
    if (!b.on || x1 < b.x0 || x0 > b.x1 || y1 < b.y0 || y0 > b.y1) return false;
    return !(x0 >= b.ix0 && x1 <= b.ix1 && y0 >= b.iy0 && y1 <= b.iy1);
}

// The chroma sample of a 2 x 2 block: the rect's if any of its four pixels is in the band, else the limb's if any is inside a limb
// (a state is OVERLAY_NONE < OVERLAY_LIMB < OVERLAY_BAND: the block's sample is the greatest of its four pixels' states, folded in one by one)
VNECT_HD int overlay_chroma(int so_far, int s) { return so_far > s ? so_far : s; }

// BT.601 limited range, 8-bit integer arithmetic (>> of a negative value: arithmetic, as numpy's and every compiler's here)
VNECT_HD void overlay_bgr_to_yuv(const int* bgr, uint8_t* yuv)
{
    const int B = bgr[0], G = bgr[1], R = bgr[2];
    yuv[0] = (uint8_t)(((66 * R + 129 * G + 25 * B + 128) >> 8) + 16);
    yuv[1] = (uint8_t)(((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128);
    yuv[2] = (uint8_t)(((112 * R - 94 * G - 18 * B + 128) >> 8) + 128);
}

// The target as the stores address it, and the two colours in the TARGET's terms: col[state - 1][c] is what channel c gets -- BGR as
// given, RGB with channels 0 and 2 exchanged, NV12 (Y, U, V).
struct OverlayTarget {
    uint8_t* data;   // pixel (0, 0) channel 0; NV12: the Y plane
    long long sy, sx, sc;  // byte strides (NV12: sy = the Y pitch, sx = 1)
    uint8_t* uv;     // NV12: the interleaved U, V plane, rows uv_stride apart
    long long uv_stride;
    int H, W;
    int nv12;
    uint8_t col[2][3];
};
VNECT_HD void overlay_colours(OverlayTarget* t, int format_rgb, const int* limb_bgr, const int* rect_bgr)
{
    const int* c[2] = {limb_bgr, rect_bgr};
    for (int k = 0; k < 2; k++) {
        if (t->nv12) overlay_bgr_to_yuv(c[k], t->col[k]);
        else
            for (int ch = 0; ch < 3; ch++) t->col[k][ch] = (uint8_t)c[k][format_rgb ? 2 - ch : ch];
    }
}
VNECT_HD int overlay_cells_x(const OverlayTarget& t) { return t.nv12 ? t.W / 2 : t.W; }
VNECT_HD int overlay_cells_y(const OverlayTarget& t) { return t.nv12 ? t.H / 2 : t.H; }

// The cells of ONE lane: column cx, rows cy_first, cy_first + OVERLAY_LANE_STEP, ... up to cy_last (at most OVERLAY_LANE_ROWS of them), all
// inside the frame.  Every surviving limb is loaded ONCE and all of the lane's pixels are tested against it (bit p of `hit`: pixel p is
// inside a limb) -- without the per-pixel cull, which cannot change an answer (no pixel further than m from the centre passes the test).
// Then the band decides per pixel, and the stores follow: plain byte stores, and none where the state is OVERLAY_NONE -- so no byte outside
// the frame's pixels (row padding, a fourth byte, memory behind the last pixel) is ever written.  PX: pixels per cell and axis.
template <int PX>
VNECT_HD void overlay_lane_px(const OverlayTarget& t, const OverlayLimb* L, const int* live, int nlive, const OverlayBand& b, int cx, int cy_first, int cy_last)
{
    static_assert(OVERLAY_LANE_ROWS * PX * PX <= 32, "one bit of `hit` per pixel of the lane");
    unsigned hit = 0;
    for (int k = 0; k < nlive; k++) {
        const OverlayLimb l = L[live[k]];
        if ((double)(cx * PX) - l.cc > l.m || l.cc - (double)(cx * PX + PX - 1) > l.m) continue;  // none of the lane's columns is near
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int p = 0; p < OVERLAY_LANE_ROWS * PX * PX; p++) {
            const int y = (cy_first + (p / (PX * PX)) * OVERLAY_LANE_STEP) * PX + ((p / PX) % PX), x = cx * PX + (p % PX);
            hit |= (overlay_inside(l, y, x) ? 1u : 0u) << p;
        }
    }
    for (int j = 0; j < OVERLAY_LANE_ROWS; j++) {
        const int cy = cy_first + j * OVERLAY_LANE_STEP;
        if (cy > cy_last) break;
        int c = OVERLAY_NONE;
        for (int q = 0; q < PX * PX; q++) {
            const int y = cy * PX + q / PX, x = cx * PX + q % PX;
            const int s = overlay_in_band(b, y, x) ? OVERLAY_BAND : (((hit >> (j * PX * PX + q)) & 1u) ? OVERLAY_LIMB : OVERLAY_NONE);
            c = overlay_chroma(c, s);
            if (s == OVERLAY_NONE) continue;
            uint8_t* p = t.data + (long long)y * t.sy + (long long)x * t.sx;
            p[0] = t.col[s - 1][0];
            if (PX == 1) p[t.sc] = t.col[s - 1][1], p[2 * t.sc] = t.col[s - 1][2];
        }
        if (PX == 2 && c != OVERLAY_NONE) {
            uint8_t* q = t.uv + (long long)cy * t.uv_stride + 2LL * cx;
            q[0] = t.col[c - 1][1], q[1] = t.col[c - 1][2];
        }
    }
}
VNECT_HD void overlay_lane(const OverlayTarget& t, const OverlayLimb* L, const int* live, int nlive, const OverlayBand& b, int cx, int cy_first, int cy_last)
{
    if (t.nv12) overlay_lane_px<2>(t, L, live, nlive, b, cx, cy_first, cy_last);
    else overlay_lane_px<1>(t, L, live, nlive, b, cx, cy_first, cy_last);
}

// What a draw reads: the joints ([row, col] in the frame's coordinates), the confidences and the threshold, the parents, the rect.
struct OverlayInput {
    double j2d[OVERLAY_NJ * 2];
    double conf[OVERLAY_NJ];
    double min_conf;
    int parents[OVERLAY_NJ];
    int has_conf;  // a threshold is set (conf and min_conf count)
    int rect[4];   // (x, y, w, h)
    int has_rect;
};
VNECT_HD OverlayLimb overlay_limb_of(const double* j2d, const double* conf, bool has_conf, double min_conf, const int* parents, int i)
{
    const int p = parents[i];
    const bool low = has_conf && (conf[i] < min_conf || conf[p] < min_conf);
    return overlay_limb(j2d[2 * i], j2d[2 * i + 1], j2d[2 * p], j2d[2 * p + 1], low);
}

}  // namespace vnect
