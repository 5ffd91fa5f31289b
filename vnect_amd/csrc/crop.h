// crop.h -- the tracking loop's per-frame crop arithmetic, ONE source for host and device (as axis.h is for the merge tables):
//   * squarify geometry of an (H, W) crop: utils.img_scale_squarify + img_padding's FrameParams (hostplan.h: squarify / build_u8_tab,
//     OpenCV's 11-bit fixed point), as a head (sizes, scaler, offsets, refusals) and one entry d of the seven 368-long table arrays --
//     the device builds a FrameParams with one thread per entry (track.hip), the host loops over the entries (crop_squarify below);
//   * the box rule of run_estimator_ps.py:96-107 (runner.bbox_update) and the degenerate-box fallback of the loop (runner.track).
// The arithmetic is IEEE double / float multiply, divide, round and convert: track.hip is built with contraction off, so the device
// gets the host's bits.  HIP-free when compiled by g++ (hostplan_capi.cpp: tests/test_track_cpu.py holds it to hostplan.h's squarify).
#pragma once
#include <math.h>
#include <string.h>

#include "axis.h"
#include "tables.h"

namespace vnect {

// why squarify refuses a crop (0: it does not); crop_refusal() gives hostplan.h's message for each
enum { SQ_OK = 0, SQ_RANGE = 1, SQ_SCALED = 2, SQ_LONG = 3 };
inline const char* crop_refusal(int code)
{
    return code == SQ_RANGE ? "frame size out of range"
                            : code == SQ_SCALED ? "squarify: scaled size exceeds 368" : code == SQ_LONG ? "squarify: scaled long side != 368" : nullptr;
}

struct SqHead {
    double scaler, scale;  // 368 / long side; its inverse, the source step of the resize
    int dh, dw, copy, offx, offy;
};
// hostplan.h: squarify's checks and build_u8_tab's destination size, in the same order.  Returns SQ_OK or the refusal.
VNECT_HD int crop_head(int H, int W, SqHead* g)
{
    if (H < 1 || W < 1 || H > 8192 || W > 8192) return SQ_RANGE;
    g->scaler = (double)BOX / (H > W ? H : W);
    const double f = g->scaler;
    if (!(f > 0.0)) return SQ_SCALED;
    const double dwf = W * f, dhf = H * f;
    if (!(dwf < 1e6) || !(dhf < 1e6)) return SQ_SCALED;
    g->dw = (int)nearbyint(dwf), g->dh = (int)nearbyint(dhf);  // cv_round: half to even
    if (g->dw < 1 || g->dh < 1 || g->dw > BOX || g->dh > BOX) return SQ_SCALED;
    g->copy = g->dw == W && g->dh == H;
    g->scale = 1.0 / f;
    if ((g->dh > g->dw ? g->dh : g->dw) != BOX) return SQ_LONG;
    g->offx = g->dh > g->dw ? BOX / 2 - g->dw / 2 : 0;
    g->offy = g->dh > g->dw ? 0 : BOX / 2 - g->dh / 2;
    return SQ_OK;
}
VNECT_HD short crop_sat(float v)  // hostplan.h: sat_short
{
    const int r = (int)nearbyintf(v);
    return (short)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
}
// Entry d (0 .. BOX-1) of the seven table arrays, zero past the destination size.  Returns 1 if column d is an inner one (a two-tap
// column below xmax): the columns at or past the far border are a suffix (axis_x_at's source offset is monotonic in d), so xmax is
// the number of inner columns.
VNECT_HD int crop_entry(const SqHead& g, int W, int H, int d, ResizeTab* t)
{
    int inner = 0;
    short sx = 0, a0 = 0, a1 = 0, sy0 = 0, sy1 = 0, b0 = 0, b1 = 0;
    if (d < g.dw) {
        const AxE e = axis_x_at(d, W, g.scale);
        sx = (short)e.s0, a0 = crop_sat((1.f - e.f) * 2048.f), a1 = crop_sat(e.f * 2048.f);
        inner = !e.edge;
    }
    if (d < g.dh) {
        const AxE e = axis_y_at(d, H, g.scale);
        sy0 = (short)e.s0, sy1 = (short)e.s1, b0 = crop_sat((1.f - e.f) * 2048.f), b1 = crop_sat(e.f * 2048.f);
    }
    t->sx[d] = sx, t->a0[d] = a0, t->a1[d] = a1, t->sy0[d] = sy0, t->sy1[d] = sy1, t->b0[d] = b0, t->b1[d] = b1;
    return inner;
}
// the fields of FrameParams besides the tables (a refused crop gets zero sizes: the pyramid reads nothing of it)
VNECT_HD void crop_fill_head(const SqHead& g, int status, int H, int W, int xmax, FrameParams* c)
{
    const bool ok = status == SQ_OK;
    c->scaler = ok ? g.scaler : 0.0;
    c->offx = ok ? g.offx : 0, c->offy = ok ? g.offy : 0;
    c->H = ok ? H : 0, c->W = ok ? W : 0;
    c->sq.dh = ok ? g.dh : 0, c->sq.dw = ok ? g.dw : 0, c->sq.copy = ok ? g.copy : 0, c->sq.xmax = ok ? xmax : 0;
}

// The whole FrameParams on the host, entry by entry as the device builds it.  Returns SQ_OK or the refusal (then *c holds zero tables).
inline int crop_squarify(int H, int W, FrameParams* c)
{
    memset(c, 0, sizeof *c);
    SqHead g;
    memset(&g, 0, sizeof g);
    const int status = crop_head(H, W, &g);
    int xmax = 0;
    if (status == SQ_OK)
        for (int d = 0; d < BOX; d++) xmax += crop_entry(g, W, H, d, &c->sq);
    crop_fill_head(g, status, H, W, xmax, c);
    return status;
}

// ---- the tracking loop (runner.track; run_estimator_ps.py:80-109) ----------------------------------------------------------------
// One axis of runner.bbox_update: lo / span of the joints along it, `grow` 0.8 (x) or 0.2 (y), the frame's extent `limit`.
//   margin = grow * (span + 1); origin = max(int(lo - margin / 2), 0); extent = int(min(span + margin, limit - origin))
// (Python's min keeps its first argument unless the second is smaller; int() truncates toward zero, as the casts here do.)
VNECT_HD void box_axis(double lo, double span, double grow, int limit, int* origin, int* extent)
{
    const double margin = grow * (span + 1);
    const long long o = (long long)(lo - margin / 2);
    const long long org = o > 0 ? o : 0;
    const long long room = (long long)limit - org;
    const double ext = span + margin;
    *origin = (int)org;
    *extent = (int)((double)room < ext ? room : (long long)ext);
}
// runner.bbox_update over 21 joints (j2 [row, col] in frame coordinates).  rect = (x, y, w, h).
VNECT_HD void box_update(const double* j2, int W, int H, int* rect)
{
    double lo[2] = {j2[0], j2[1]}, hi[2] = {j2[0], j2[1]};
    for (int j = 1; j < NJ; j++)
        for (int k = 0; k < 2; k++) {
            const double v = j2[2 * j + k];
            lo[k] = v < lo[k] ? v : lo[k];
            hi[k] = v > hi[k] ? v : hi[k];
        }
    int x, w, y, h;
    box_axis(lo[1], hi[1] - lo[1], 0.8, W, &x, &w);
    box_axis(lo[0], hi[0] - lo[0], 0.2, H, &y, &h);
    rect[0] = x, rect[1] = y, rect[2] = w, rect[3] = h;
}
// the loop's fallback to the whole frame for a box narrower or lower than one pixel (runner.track: `if w < 1 or h < 1`)
VNECT_HD void box_fallback(int W, int H, int* rect)
{
    if (rect[2] < 1 || rect[3] < 1) rect[0] = 0, rect[1] = 0, rect[2] = W, rect[3] = H;
}

}  // namespace vnect
