// preview.h -- the annotated frame scaled for display (the reference: run_estimator_ps.py:94-96 -- utils.draw_limbs_2d into frame.copy(),
// then utils.img_scale(frame_draw, 1024 / max(W_img, H_img)), i.e. cv2.resize(.., fx = fy = f, INTER_LINEAR), then cv2.imshow): the
// RULE, ONE source for host and device (as overlay.h, orient.h, nv12.h and crop.h are).  The kernel of preview.hip and the host walk of
// preview_capi.cpp (tests/test_preview_cpu.py, and the sanitizer sweep) call the same functions: the output size, a tile's footprint, a
// source pixel of the oriented picture P, a tap of the annotated picture A (band over limbs over P, overlay.h unchanged, in the BGR
// domain), the 11-bit fixed-point blend of cv2's 8-bit INTER_LINEAR (axis.h's taps, hostplan.h::sample_u8's line) and the stores of one
// lane.  The frame is only ever READ.  PREVIEW.md has the rule in words.  HIP-free when compiled by g++.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "axis.h"
#include "crop.h"  // crop_sat: hostplan.h's sat_short for host and device
#include "nv12.h"
#include "orient.h"
#include "overlay.h"

namespace vnect {

constexpr int PREVIEW_MAX = 4096;  // an output side at most (include/vnect_abi.h: VNECT_PREVIEW_MAX)
// The kernel's tile, in OUTPUT pixels: 256 lanes own 64 x 16, each lane four horizontally adjacent pixels (12 output bytes) of one row.
constexpr int PREVIEW_TILE_W = 64, PREVIEW_TILE_H = 16, PREVIEW_THREADS = 256, PREVIEW_LANE_PX = 4;
constexpr int PREVIEW_LANES_X = PREVIEW_TILE_W / PREVIEW_LANE_PX;
static_assert(PREVIEW_LANES_X * PREVIEW_TILE_H == PREVIEW_THREADS, "preview.h: one lane per four pixels of the tile");

enum { PREVIEW_OK = 0, PREVIEW_E_FACTOR = 1, PREVIEW_E_EMPTY = 2, PREVIEW_E_LARGE = 3 };
inline const char* preview_refusal(int code)
{
    return code == PREVIEW_E_FACTOR ? "the factor must be finite and not negative (0: 1024 / the picture's longer side)"
                                    : code == PREVIEW_E_EMPTY ? "an output side rounds to 0"
                                                              : code == PREVIEW_E_LARGE ? "an output side exceeds 4096 (VNECT_PREVIEW_MAX)" : nullptr;
}

struct PreviewGeom {
    int Hp, Wp;    // the oriented picture
    int dh, dw;    // the output: (cv_round(Hp f), cv_round(Wp f)), half to even
    int copy;      // both sizes kept: the output is A itself
    double scale;  // 1 / f, the source step (cv2 keeps the user's fx when dsize is (0, 0))
};
// The output of an (H, W) frame stored under orientation o at factor f (0: the reference's 1024.0 / max(Wp, Hp)).  HOST only
// (nearbyint in the default rounding mode); the kernel gets the result.
inline int preview_geom(int o, int H, int W, double f, PreviewGeom* g)
{
    orient_size(o, H, W, &g->Hp, &g->Wp);
    if (!(f >= 0.0) || !(f <= 1.7e308)) return PREVIEW_E_FACTOR;  // (NaN fails the first, +inf the second)
    if (f == 0.0) f = 1024.0 / (double)(g->Wp > g->Hp ? g->Wp : g->Hp);
    const double dhf = g->Hp * f, dwf = g->Wp * f;
    if (!(dhf < 1e6) || !(dwf < 1e6)) return PREVIEW_E_LARGE;  // before the casts: a hostile factor must not overflow an int
    g->dh = (int)nearbyint(dhf), g->dw = (int)nearbyint(dwf);
    if (g->dh < 1 || g->dw < 1) return PREVIEW_E_EMPTY;
    if (g->dh > PREVIEW_MAX || g->dw > PREVIEW_MAX) return PREVIEW_E_LARGE;
    g->copy = g->dh == g->Hp && g->dw == g->Wp;
    g->scale = 1.0 / f;
    return PREVIEW_OK;
}

// What a launch reads and writes.  `src` is the stored frame as orient.h describes it (its bounds are not used: every pixel a tap reads
// lies inside the validated frame, and pixels are read byte by byte).
struct PreviewArgs {
    OrientSrc src;
    int o, H, W;       // the orientation code and the frame as it is STORED
    PreviewGeom g;
    uint8_t* out;      // output pixel (0, 0), any alignment; rows `pitch` bytes apart, 3 dw bytes each
    long long pitch;
    int out_rgb;       // the output's channel order: 0 BGR, 1 RGB
    int has_joints;    // 0: no limb is drawn
    int col[2][3];     // the limb's and the rect's colour, BGR
};

// a validated frame (vnect_device_frame's terms) as `src`; the bounds stay empty
inline OrientSrc preview_source(bool nv12, bool rgb, const uint8_t* data, const uint8_t* uv, long long sy, long long sx, long long sc, long long uv_stride)
{
    OrientSrc s;
    memset(&s, 0, sizeof s);
    s.p0 = data, s.sy = sy, s.order = rgb ? INGEST_RGB : INGEST_BGR;
    if (nv12) s.p1 = uv, s.sx = 1, s.sc = uv_stride, s.form = ORIENT_NV12;
    else s.sx = sx, s.sc = sc, s.form = ingest_form(sx, sc);
    return s;
}
// the two colours of a launch, BGR (nullptr: the reference's)
inline void preview_colours(PreviewArgs* a, const int* limb_bgr, const int* rect_bgr)
{
    for (int k = 0; k < 3; k++) a->col[0][k] = limb_bgr ? limb_bgr[k] : OVERLAY_LIMB_BGR[k], a->col[1][k] = rect_bgr ? rect_bgr[k] : OVERLAY_RECT_BGR[k];
}

// Pixel (i, j) of the oriented picture P, as ingest delivers it: orient_map, then RGB -> BGR, or nv12.h's conversion of the stored pixel
// with the chroma of the 2 x 2 block it lies in
VNECT_HD void preview_src_pixel(const OrientSrc& s, int o, int H, int W, int i, int j, int* bgr)
{
    int r, c;
    orient_map(o, H, W, i, j, &r, &c);
    if (s.form == ORIENT_NV12) {
        const uint8_t* y = s.p0 + (long long)r * s.sy + c;
        const uint8_t* uv = s.p1 + (long long)(r >> 1) * s.sc + (c & ~1);
        nv12_pixel((int)y[0], (int)uv[0], (int)uv[1], bgr);
        return;
    }
    const uint8_t* p = s.p0 + (long long)r * s.sy + (long long)c * s.sx;
    const int c0 = p[0], c1 = p[s.sc], c2 = p[2 * s.sc];
    bgr[0] = s.order == INGEST_RGB ? c2 : c0, bgr[1] = c1, bgr[2] = s.order == INGEST_RGB ? c0 : c2;
}

// Pixel (i, j) of the annotated picture A: overlay.h's rule -- in the band: the rect's colour; else inside a surviving limb: the limb's;
// else P's pixel, which is fetched only then
VNECT_HD void preview_tap(const PreviewArgs& a, const OverlayLimb* L, const int* live, int nlive, const OverlayBand& b, int i, int j, int* bgr)
{
    int s = overlay_in_band(b, i, j) ? OVERLAY_BAND : OVERLAY_NONE;
    for (int k = 0; k < nlive && s == OVERLAY_NONE; k++)
        if (overlay_inside(L[live[k]], i, j)) s = OVERLAY_LIMB;
    if (s == OVERLAY_NONE) preview_src_pixel(a.src, a.o, a.H, a.W, i, j, bgr);
    else bgr[0] = a.col[s - 1][0], bgr[1] = a.col[s - 1][1], bgr[2] = a.col[s - 1][2];
}

// The annotation of ONE person as a tap's source: what preview_kernel and vnect_preview_device draw
struct PreviewOne {
    const OverlayLimb* L;
    const int* live;
    int nlive;
    const OverlayBand* b;
    VNECT_HD void tap(const PreviewArgs& a, int i, int j, int* bgr) const { preview_tap(a, L, live, nlive, *b, i, j, bgr); }
};

// The annotation of P persons of one frame (people mode; PEOPLE.md; no reference counterpart: run_estimator_ps.py:92-96 draws the one
// person it follows): pixel (i, j) of A is band p over limbs p over ... for p = P-1 down to 0, over P's pixel -- exactly P applications of
// overlay.h's rule in person order 0 .. P-1, each drawing over the one before.  Person p's limbs are L[p * OVERLAY_NJ ..], the survivors'
// indices live[p * OVERLAY_NJ ..] (nlive[p] of them), its band b[p]; a person that is not drawn has nlive 0 and its band off.
constexpr int PREVIEW_MAX_PEOPLE = 4;
struct PreviewPeople {
    int P;
    const OverlayLimb* L;
    const int* live;
    const int* nlive;
    const OverlayBand* b;
    VNECT_HD void tap(const PreviewArgs& a, int i, int j, int* bgr) const
    {
        int s = OVERLAY_NONE;
        for (int p = P - 1; p >= 0 && s == OVERLAY_NONE; p--) {
            if (overlay_in_band(b[p], i, j)) s = OVERLAY_BAND;
            for (int k = 0; k < nlive[p] && s == OVERLAY_NONE; k++)
                if (overlay_inside(L[p * OVERLAY_NJ + live[p * OVERLAY_NJ + k]], i, j)) s = OVERLAY_LIMB;
        }
        if (s == OVERLAY_NONE) preview_src_pixel(a.src, a.o, a.H, a.W, i, j, bgr);
        else bgr[0] = a.col[s - 1][0], bgr[1] = a.col[s - 1][1], bgr[2] = a.col[s - 1][2];
    }
};

// Output pixel (dy, dx): cv2's 8-bit INTER_LINEAR as the project pins it (oracle.resize; hostplan.h: build_u8_tab + sample_u8)
template <class Scene>
VNECT_HD void preview_pixel_of(const PreviewArgs& a, const Scene& sc, int dy, int dx, int* bgr)
{
    if (a.g.copy) {
        sc.tap(a, dy, dx, bgr);
        return;
    }
    const AxE x = axis_x_at(dx, a.g.Wp, a.g.scale), y = axis_y_at(dy, a.g.Hp, a.g.scale);
    const int b0 = crop_sat((1.f - y.f) * 2048.f), b1 = crop_sat(y.f * 2048.f);
    int t0[3], t1[3], r0[3], r1[3];
    sc.tap(a, y.s0, x.s0, t0);
    sc.tap(a, y.s1, x.s0, t1);
    if (!x.edge) {
        const int a0 = crop_sat((1.f - x.f) * 2048.f), a1 = crop_sat(x.f * 2048.f);
        int u0[3], u1[3];
        sc.tap(a, y.s0, x.s0 + 1, u0);
        sc.tap(a, y.s1, x.s0 + 1, u1);
        for (int c = 0; c < 3; c++) r0[c] = t0[c] * a0 + u0[c] * a1, r1[c] = t1[c] * a0 + u1[c] * a1;
    } else {
        for (int c = 0; c < 3; c++) r0[c] = t0[c] * 2048, r1[c] = t1[c] * 2048;  // a column at or past xmax: the single tap
    }
    for (int c = 0; c < 3; c++) bgr[c] = (((b0 * (r0[c] >> 4)) >> 16) + ((b1 * (r1[c] >> 4)) >> 16) + 2) >> 2;
}
VNECT_HD void preview_pixel(const PreviewArgs& a, const OverlayLimb* L, const int* live, int nlive, const OverlayBand& b, int dy, int dx, int* bgr)
{
    preview_pixel_of(a, PreviewOne{L, live, nlive, &b}, dy, dx, bgr);
}

// The rectangle of A that the taps of output rows dy0 .. dy1 and columns dx0 .. dx1 lie in (taps are monotonic in the output index)
VNECT_HD void preview_footprint(const PreviewGeom& g, int dy0, int dy1, int dx0, int dx1, long long* y0, long long* y1, long long* x0, long long* x1)
{
    if (g.copy) {
        *y0 = dy0, *y1 = dy1, *x0 = dx0, *x1 = dx1;
        return;
    }
    *y0 = axis_y_at(dy0, g.Hp, g.scale).s0, *y1 = axis_y_at(dy1, g.Hp, g.scale).s1;
    *x0 = axis_x_at(dx0, g.Wp, g.scale).s0, *x1 = axis_x_at(dx1, g.Wp, g.scale).s1;
}

// The STORES of one lane: n (1 .. 12) bytes, the little-endian stream w[0] w[1] w[2], to address `at` (any alignment).  They go out as
// the aligned dwords the bytes lie in: a dword wholly inside the n bytes is one store; one that the lane shares with its neighbour, with
// the next tile or with the row's end goes out as its own bytes, one by one -- so nothing outside [at, at + n) is written (orient.h's
// orient_out_dword and ingest.h's ingest_dst_mask draw the same line).
VNECT_HD void preview_store(uintptr_t at, const uint32_t* w, int n)
{
    const uintptr_t al = at & ~(uintptr_t)3;
    const int ad = (int)(at - al);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; k++) {
        const uint32_t lo = k > 0 ? w[k - 1] : 0u, hi = k < 3 ? w[k] : 0u;
        const uint32_t v = ad ? (lo >> (8 * (4 - ad))) | (hi << (8 * ad)) : hi;
        const int q = 4 * k - ad;  // stream index of the dword's byte 0
        if (q >= n) break;
        if (q >= 0 && q + 4 <= n) {
#if defined(__HIP_DEVICE_COMPILE__)
            *(uint32_t*)(al + 4u * k) = v;
#else
            memcpy((void*)(al + 4u * k), &v, 4);
#endif
            continue;
        }
        for (int j = 0; j < 4; j++)
            if (q + j >= 0 && q + j < n) *(uint8_t*)(al + 4u * k + j) = (uint8_t)(v >> (8 * j));
    }
}

// One lane: output row dy, columns dx .. dx + PREVIEW_LANE_PX - 1 (those below dw)
template <class Scene>
VNECT_HD void preview_lane_of(const PreviewArgs& a, const Scene& sc, int dy, int dx)
{
    uint32_t w[3] = {0u, 0u, 0u};
    const int npx = a.g.dw - dx < PREVIEW_LANE_PX ? a.g.dw - dx : PREVIEW_LANE_PX;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int p = 0; p < PREVIEW_LANE_PX; p++) {
        if (p >= npx) break;
        int c[3];
        preview_pixel_of(a, sc, dy, dx + p, c);
        const uint32_t c0 = (uint32_t)(a.out_rgb ? c[2] : c[0]), c1 = (uint32_t)c[1], c2 = (uint32_t)(a.out_rgb ? c[0] : c[2]);
        // pixel p's bytes are 3 p, 3 p + 1, 3 p + 2 of the stream
        w[(3 * p) >> 2] |= c0 << (8 * ((3 * p) & 3));
        w[(3 * p + 1) >> 2] |= c1 << (8 * ((3 * p + 1) & 3));
        w[(3 * p + 2) >> 2] |= c2 << (8 * ((3 * p + 2) & 3));
    }
    preview_store((uintptr_t)a.out + (unsigned long long)dy * (unsigned long long)a.pitch + 3ull * (unsigned)dx, w, 3 * npx);
}
VNECT_HD void preview_lane(const PreviewArgs& a, const OverlayLimb* L, const int* live, int nlive, const OverlayBand& b, int dy, int dx)
{
    preview_lane_of(a, PreviewOne{L, live, nlive, &b}, dy, dx);
}

// The limbs and the band of a launch as every workgroup sets them up
VNECT_HD OverlayLimb preview_limb_of(const PreviewArgs& a, const double* j2d, const double* conf, bool has_conf, double min_conf, const int* parents, int i)
{
    if (!a.has_joints) return overlay_limb(0.0, 0.0, 0.0, 0.0, true);
    return overlay_limb_of(j2d, conf, has_conf, min_conf, parents, i);
}

}  // namespace vnect
