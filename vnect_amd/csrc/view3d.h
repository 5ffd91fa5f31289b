// view3d.h -- the reference's SECOND window: the 3-D skeleton plot that its frame loop feeds joints_3d through q_joints
// (run_estimator_ps.py:90, 124-126; src/utils.py:272-304: set_xlim/ylim/zlim(-500, 500), view_init(-90, -90), one line of width 3 per
// limb, in the colour cycle's order; :317-330 the process that shows it).  The drawing RULE, ONE source for host and device (as overlay.h and
// preview.h are): the kernel of view3d.hip and the host walk of view3d_capi.cpp (tests/test_view3d_cpu.py, and the sanitizer sweep) call
// the same functions -- a joint's projection, a limb's set-up and cull, the inside test, the ranking, the tests and stores of one lane.
// The rule (VIEW3D.md) is this project's own: matplotlib's anti-aliased Agg lines cannot be pinned; this uses float64 multiplies, adds,
// subtracts and compares only, each in the order written -- no trigonometry, no division on the device, and (built with contraction off)
// no fused multiply-add -- so numpy, g++ and the GPU agree bit for bit.  HIP-free under g++.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "axis.h"     // VNECT_HD
#include "preview.h"  // preview_store: a lane's bytes as aligned dwords where they are whole, single bytes elsewhere

namespace vnect {

constexpr int VIEW3D_NJ = 21;
constexpr int VIEW3D_MAX = 2048;  // VNECT_VIEW3D_MAX: rows and columns at most
// The kernel's tile: 256 lanes own 64 x 16 pixels of the output, four adjacent pixels (12 bytes) each
constexpr int VIEW3D_TILE_W = 64, VIEW3D_TILE_H = 16, VIEW3D_THREADS = 256, VIEW3D_LANE_PX = 4;
constexpr int VIEW3D_LANES_X = VIEW3D_TILE_W / VIEW3D_LANE_PX;
constexpr double VIEW3D_COORD_MAX = 1048576.0;  // 2^20: a joint projected further out (or non-finite) skips its limbs
// matplotlib's colour cycle (rcParams['axes.prop_cycle'], "tab10") as BGR: limb i takes entry i % 10 (src/utils.py:289, 298 set no colour)
constexpr int VIEW3D_CYCLE_BGR[10][3] = {{180, 119, 31}, {14, 127, 255}, {44, 160, 44},   {40, 39, 214}, {189, 103, 148},
                                         {75, 86, 140},  {194, 119, 227}, {127, 127, 127}, {34, 189, 188}, {207, 190, 23}};

// What a launch is given by value: the output, the host constants of the rule, the view, the parents and the colours in the OUTPUT's
// channel order (BGR as given, RGB with channels 0 and 2 exchanged).
struct View3dArgs {
    uint8_t* out;     // pixel (0, 0) channel 0
    long long pitch;  // bytes between rows, >= 3 * cols
    int rows, cols;
    double R[9];      // the view, row-major: (u, v, d) = R (x, y, z)
    double k, cx, cy; // pixels per mm; the centre's column and row
    double r2;        // (w / 2)^2
    double grow;      // w / 2 + 1: the cull's margin (no part of the rule)
    double min_conf;
    int has_conf;     // a threshold is set AND confidences are given
    int order;        // 0: the higher index lies on top; 1: the nearer limb does
    int parents[VIEW3D_NJ];
    uint8_t col[VIEW3D_NJ + 1][3];  // [VIEW3D_NJ]: the background
};

// s = min(rows, cols); k = double(s - 1) / (2.0 * extent); cx = double(cols - 1) * 0.5; cy = double(rows - 1) * 0.5; r2 = (w * 0.5) * (w * 0.5).
// HOST ONLY (the one division of the rule): the device gets the results.
inline void view3d_constants(View3dArgs* a, double extent, double w)
{
    const int s = a->rows < a->cols ? a->rows : a->cols;
    a->k = (double)(s - 1) / (2.0 * extent);
    a->cx = (double)(a->cols - 1) * 0.5, a->cy = (double)(a->rows - 1) * 0.5;
    a->r2 = (w * 0.5) * (w * 0.5);
    a->grow = w * 0.5 + 1.0;
}

// limb i's colour and the background in the output's order
inline void view3d_colours(View3dArgs* a, int out_rgb, const int (*colors_bgr)[3], const int* background_bgr)
{
    for (int i = 0; i < VIEW3D_NJ; i++)
        for (int c = 0; c < 3; c++) a->col[i][c] = (uint8_t)(colors_bgr ? colors_bgr[i][out_rgb ? 2 - c : c] : VIEW3D_CYCLE_BGR[i % 10][out_rgb ? 2 - c : c]);
    for (int c = 0; c < 3; c++) a->col[VIEW3D_NJ][c] = (uint8_t)(background_bgr ? background_bgr[out_rgb ? 2 - c : c] : 255);
}

// A view's specification as plain fields (vnect_view3d_spec without the ABI's framing): a zero field or a null pointer is its default.
struct View3dSpecIn {
    int rows, cols;               // 0: 400
    double extent;                // 0: 500.0 (set_xlim/ylim/zlim(-500, 500), src/utils.py:277-279)
    const double* view;           // nullptr: the identity (view_init(-90, -90), src/utils.py:280)
    double line_width;            // 0: 3.0 (linewidth=3, src/utils.py:289)
    const int* background_bgr;    // nullptr: white
    const int (*colors_bgr)[3];   // nullptr: the colour cycle
    const int* parents;           // nullptr: `default_parents`
    double min_conf;              // NaN: no threshold
    int out_format;               // 0 BGR, 1 RGB
    int order;
};
// HOST ONLY.  Validates the specification and fills everything of *a but out, pitch and has_conf's second half (has_conf says here that a
// threshold is set; a caller without confidences clears it).  Returns nullptr, or what is wrong.
inline const char* view3d_setup(const View3dSpecIn& s, const int* default_parents, View3dArgs* a)
{
    memset(a, 0, sizeof *a);
    a->rows = s.rows ? s.rows : 400, a->cols = s.cols ? s.cols : 400;
    if (a->rows < 1 || a->rows > VIEW3D_MAX || a->cols < 1 || a->cols > VIEW3D_MAX) return "rows and cols must lie in 1 .. 2048";
    const double extent = s.extent == 0.0 ? 500.0 : s.extent, w = s.line_width == 0.0 ? 3.0 : s.line_width;
    if (!(extent > 0.0) || !(extent - extent == 0.0)) return "extent must be finite and positive";
    if (!(w > 0.0) || !(w <= 64.0)) return "line_width must lie in (0, 64]";
    for (int i = 0; i < 9; i++) {
        a->R[i] = s.view ? s.view[i] : (i % 4 == 0 ? 1.0 : 0.0);
        if (!(a->R[i] - a->R[i] == 0.0)) return "a view entry is not finite";
    }
    if (s.out_format != 0 && s.out_format != 1) return "out_format must be VNECT_PIX_BGR or VNECT_PIX_RGB";
    if (s.order != 0 && s.order != 1) return "order must be 0 or 1";
    for (int c = 0; c < 3; c++)
        if (s.background_bgr && (s.background_bgr[c] < 0 || s.background_bgr[c] > 255)) return "a colour component must lie in 0 .. 255";
    for (int i = 0; i < VIEW3D_NJ; i++) {
        for (int c = 0; c < 3; c++)
            if (s.colors_bgr && (s.colors_bgr[i][c] < 0 || s.colors_bgr[i][c] > 255)) return "a colour component must lie in 0 .. 255";
        a->parents[i] = s.parents ? s.parents[i] : default_parents[i];
        if (a->parents[i] < 0 || a->parents[i] >= VIEW3D_NJ) return "a parent must be a joint, 0 .. 20";
    }
    view3d_constants(a, extent, w);
    view3d_colours(a, s.out_format, s.colors_bgr, s.background_bgr);
    a->order = s.order;
    if (s.min_conf == s.min_conf) a->min_conf = s.min_conf, a->has_conf = 1;
    return nullptr;
}

VNECT_HD bool view3d_coord_ok(double v) { return v >= -VIEW3D_COORD_MAX && v <= VIEW3D_COORD_MAX; }  // (false for NaN and both infinities)
VNECT_HD bool view3d_finite(double v) { return v - v == 0.0; }                                         // (false for NaN and both infinities)

// One joint: (pc, pr) on the screen and its depth d (larger: farther from the camera)
VNECT_HD void view3d_project(const View3dArgs& a, const float* j, double* pc, double* pr, double* d)
{
    const double x = (double)j[0], y = (double)j[1], z = (double)j[2];
    const double u = (a.R[0] * x + a.R[1] * y) + a.R[2] * z;
    const double v = (a.R[3] * x + a.R[4] * y) + a.R[5] * z;
    *d = (a.R[6] * x + a.R[7] * y) + a.R[8] * z;
    *pc = a.cx + u * a.k, *pr = a.cy + v * a.k;
}

// One limb, set up once: A = joint i, B = its parent
struct View3dLimb {
    double ax, ay, bx, by;  // (column, row) of both ends
    double ex, ey, L2;      // B - A and its squared length
    double rL2;             // r2 * L2, the band test's right-hand side
    double key;             // dA + dB (order 1: the smaller lies on top)
    int skip;
};

VNECT_HD View3dLimb view3d_limb_of(const View3dArgs& a, const float* j3d, const double* conf, int i)
{
    View3dLimb l;
    l.ax = l.ay = l.bx = l.by = l.ex = l.ey = l.L2 = l.rL2 = l.key = 0.0;
    l.skip = 1;
    const int p = a.parents[i];
    if (p == i) return l;
    if (a.has_conf && (conf[i] < a.min_conf || conf[p] < a.min_conf)) return l;
    double da, db;
    view3d_project(a, j3d + 3 * i, &l.ax, &l.ay, &da);
    view3d_project(a, j3d + 3 * p, &l.bx, &l.by, &db);
    if (!view3d_coord_ok(l.ax) || !view3d_coord_ok(l.ay) || !view3d_coord_ok(l.bx) || !view3d_coord_ok(l.by)) return l;
    if (a.order == 1 && (!view3d_finite(da) || !view3d_finite(db))) return l;
    l.ex = l.bx - l.ax, l.ey = l.by - l.ay;
    l.L2 = l.ex * l.ex + l.ey * l.ey;
    l.rL2 = a.r2 * l.L2;
    l.key = a.order == 1 ? da + db : 0.0;
    l.skip = 0;
    return l;
}

// Is pixel (row y, column x) inside the limb: within w / 2 of the segment A B (round caps; a limb of length 0 is a disc)
VNECT_HD bool view3d_inside(const View3dLimb& l, double r2, int y, int x)
{
    const double wx = (double)x - l.ax, wy = (double)y - l.ay;
    const double t = wx * l.ex + wy * l.ey;
    if (t <= 0.0) return wx * wx + wy * wy <= r2;
    if (t >= l.L2) {
        const double qx = (double)x - l.bx, qy = (double)y - l.by;
        return qx * qx + qy * qy <= r2;
    }
    const double c = wx * l.ey - wy * l.ex;
    return c * c <= l.rL2;
}

// Can any pixel of rows [y0, y1], columns [x0, x1] be inside?  The bounding box of the two ends grown by w / 2 + 1: a pixel inside lies
// within w / 2 of the segment, so within w / 2 of the box; the extra pixel keeps the cull's own rounding out of the answer.
VNECT_HD bool view3d_limb_near(const View3dLimb& l, double grow, int y0, int y1, int x0, int x1)
{
    if (l.skip) return false;
    const double lox = (l.ax < l.bx ? l.ax : l.bx) - grow, hix = (l.ax < l.bx ? l.bx : l.ax) + grow;
    const double loy = (l.ay < l.by ? l.ay : l.by) - grow, hiy = (l.ay < l.by ? l.by : l.ay) + grow;
    return (double)x1 >= lox && (double)x0 <= hix && (double)y1 >= loy && (double)y0 <= hiy;
}

// Does limb i lie over limb j where both cover a pixel?  order 0: the higher index (the reference adds line 0 first and line 20 last);
// order 1: the smaller key, ties to the higher index.  A total order: a limb's rank is the number of limbs it lies over.
VNECT_HD bool view3d_over(int order, double key_i, int i, double key_j, int j)
{
    if (order == 1 && key_i != key_j) return key_i < key_j;
    return i > j;
}

// The pixels of ONE lane: row dy, columns dx .. dx + VIEW3D_LANE_PX - 1 (those below cols).  `live`: the tile's surviving limbs from the
// lowest rank to the highest, so the last one that covers a pixel is the one on top.  Every pixel is written, exactly once.
VNECT_HD void view3d_lane(const View3dArgs& a, const View3dLimb* L, const int* live, int nlive, int dy, int dx)
{
    const int npx = a.cols - dx < VIEW3D_LANE_PX ? a.cols - dx : VIEW3D_LANE_PX;
    int sel[VIEW3D_LANE_PX];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int p = 0; p < VIEW3D_LANE_PX; p++) sel[p] = VIEW3D_NJ;  // (the background's entry of the colour table)
    for (int q = 0; q < nlive; q++) {
        const int i = live[q];
        const View3dLimb l = L[i];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int p = 0; p < VIEW3D_LANE_PX; p++)
            if (view3d_inside(l, a.r2, dy, dx + p)) sel[p] = i;
    }
    uint32_t w[3] = {0u, 0u, 0u};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int p = 0; p < VIEW3D_LANE_PX; p++) {
        if (p >= npx) break;
        const uint32_t c0 = a.col[sel[p]][0], c1 = a.col[sel[p]][1], c2 = a.col[sel[p]][2];
        // pixel p's bytes are 3 p, 3 p + 1, 3 p + 2 of the stream
        w[(3 * p) >> 2] |= c0 << (8 * ((3 * p) & 3));
        w[(3 * p + 1) >> 2] |= c1 << (8 * ((3 * p + 1) & 3));
        w[(3 * p + 2) >> 2] |= c2 << (8 * ((3 * p + 2) & 3));
    }
    preview_store((uintptr_t)a.out + (unsigned long long)dy * (unsigned long long)a.pitch + 3ull * (unsigned)dx, w, 3 * npx);
}

// what a launcher (and the host walk) refuses: anything the kernel could not run safely
VNECT_HD bool view3d_args_ok(const View3dArgs& a)
{
    if (!a.out || a.rows < 1 || a.cols < 1 || a.rows > VIEW3D_MAX || a.cols > VIEW3D_MAX || a.pitch < 3LL * a.cols) return false;
    if (a.order != 0 && a.order != 1) return false;
    for (int i = 0; i < VIEW3D_NJ; i++)
        if (a.parents[i] < 0 || a.parents[i] >= VIEW3D_NJ) return false;
    return true;
}

}  // namespace vnect
