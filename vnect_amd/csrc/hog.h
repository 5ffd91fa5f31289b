// hog.h -- the person detector in front of the frame loop (the reference: src/hog_box.py:24-46 -- cv2.HOGDescriptor() with the default
// people detector, detectMultiScale(img), the biggest rectangle inflated by cal_rect): the RULE, ONE source for host and device (as
// preview.h, overlay.h, orient.h and nv12.h are).  The kernels of hog.hip and the host walk of hog_capi.cpp call the same functions: the
// level table, a pixel of a level image, a pixel's two votes, a block's row partials and its L2-Hys scales, a window's score, and -- host
// only -- the ordered hits, their rectangles and groupRectangles.  Nothing here is pinned against cv2 (nobody here has it): the rule is
// stated from OpenCV's published algorithm, HOG.md lists every point.  HIP-free when compiled by g++.
//
// PRECISION AND ORDER.  Everything below the level table is float32 unless it says otherwise; every operation is one IEEE add, subtract,
// multiply, divide, sqrt, floor or compare (hog.hip is built with -ffp-contract=off, g++ likewise; hipcc's float divide and sqrt are the
// correctly rounded ones, its default).  Sums run in the order written:
//   gradient   m2 = dx*dx + dy*dy (two products, one add); channels 2, 1, 0, a later one replaces only when strictly larger
//   angle      c = mn / (mx + float32(DBL_EPSILON)), c2 = c*c, a = c * (K0 + c2 * (K1 + c2 * (K2 + c2 * K3))) -- Horner, innermost first,
//              K* the float32 of the stated doubles; then a = float32(pi/2) - a when ay > ax, a = float32(pi) - a when dx < 0,
//              a = float32(2 pi) - a when dy < 0; pos = a * float32(9/pi) - 0.5f
//   histogram  hist[c*9 + b] = sum over rows i = 0 .. 15 ascending of R(c, b, i), R(c, b, i) = sum over columns j = 0 .. 15 ascending of
//              wt[c][i][j] * vote_b(i, j), each sum starting at +0 (vote_b: v0 if h0 == b, v1 if h1 == b, else no term -- every term
//              is >= 0, so an absent term and an added +0 are the same bits)
//   L2-Hys     s1 = sum over k = 0 .. 35 ascending of hist[k]*hist[k]; u = min(hist[k] * (1.f / (sqrtf(s1) + 3.6f)), 0.2f);
//              s2 = the same sum over u; out[k] = u * (1.f / (sqrtf(s2) + 1e-3f))
//   score      T(bx, by) = sum over k = 0 .. 35 ascending of det[(bx*15 + by)*36 + k] * desc(bx, by)[k]; C(bx) = sum over by = 0 .. 14
//              ascending of T(bx, by); S = sum over bx = 0 .. 6 ascending of C(bx); s = det[3780] + S
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "preview.h"  // preview_src_pixel: the oriented BGR picture P, pixel by pixel, from every layout (PREVIEW.md); axis.h, crop.h

#include <algorithm>
#include <vector>

namespace vnect {

// cv2's HOGDescriptor() defaults (hog_box.py:25)
constexpr int HOG_WIN_W = 64, HOG_WIN_H = 128, HOG_BLOCK = 16, HOG_CELL = 8, HOG_NBINS = 9, HOG_BLOCK_LEN = 36;
constexpr int HOG_WIN_BX = 7, HOG_WIN_BY = 15, HOG_DESC = HOG_WIN_BX * HOG_WIN_BY * HOG_BLOCK_LEN;  // 3780
constexpr int HOG_MAX_LEVELS = 64, HOG_MAX_SIDE = 4096, HOG_DEFAULT_MAX_HITS = 65536;
static_assert(HOG_DESC == 3780, "hog.h: the descriptor of cv2.HOGDescriptor_getDefaultPeopleDetector()");
// the kernels' tiles: votes -- 256 lanes own 64 x 4 pixels of a level, one each; blocks and windows -- one wave each, four per workgroup
constexpr int HOG_THREADS = 256, HOG_VTILE_W = 64, HOG_VTILE_H = 4, HOG_PER_WG = 4;

constexpr float HOG_K0 = (float)0.9997878412794807, HOG_K1 = (float)-0.3258083974640975, HOG_K2 = (float)0.1555786518463281,
                HOG_K3 = (float)-0.04432655554792128;
constexpr float HOG_PI = (float)3.14159265358979323846, HOG_HALF_PI = (float)(3.14159265358979323846 / 2.0), HOG_TWO_PI = (float)(3.14159265358979323846 * 2.0);
constexpr float HOG_BINS_PER_RAD = (float)(9.0 / 3.14159265358979323846), HOG_ATAN_EPS = (float)DBL_EPSILON;
constexpr float HOG_L2_EPS = 3.6f, HOG_CLIP = 0.2f, HOG_L2_EPS2 = 1e-3f;
constexpr double HOG_GROUP_EPS = 0.2;

enum { HOG_OK = 0, HOG_E_STRIDE = 1, HOG_E_SCALE = 2, HOG_E_THRESH = 3, HOG_E_LEVELS = 4, HOG_E_SIDE = 5, HOG_E_HITS = 6 };
inline const char* hog_refusal(int code)
{
    switch (code) {
    case HOG_E_STRIDE: return "win_stride_x and win_stride_y must be positive multiples of 8";
    case HOG_E_SCALE: return "scale0 must be finite and greater than 1";
    case HOG_E_THRESH: return "hit_threshold and final_threshold must be finite";
    case HOG_E_LEVELS: return "nlevels must lie in 1 .. 64";
    case HOG_E_SIDE: return "a picture side exceeds 4096";
    case HOG_E_HITS: return "max_hits must be positive";
    }
    return nullptr;
}

// detectMultiScale's parameters, defaults filled in (hog_box.py:28 passes none)
struct HogSpec {
    double hit_threshold, scale0, final_threshold;
    int stride_x, stride_y, nlevels, max_hits;
};
// a zero field means its default (include/vnect_abi.h: vnect_hog_spec); the refusals of a spec
inline int hog_spec(double hit_threshold, int sx, int sy, double scale0, double final_threshold, int nlevels, int max_hits, HogSpec* s)
{
    s->hit_threshold = hit_threshold;
    s->stride_x = sx ? sx : 8, s->stride_y = sy ? sy : 8;
    s->scale0 = scale0 == 0.0 ? 1.05 : scale0;
    s->final_threshold = final_threshold == 0.0 ? 2.0 : final_threshold;
    s->nlevels = nlevels ? nlevels : 64, s->max_hits = max_hits ? max_hits : HOG_DEFAULT_MAX_HITS;
    if (s->stride_x < 8 || s->stride_y < 8 || s->stride_x % 8 || s->stride_y % 8) return HOG_E_STRIDE;
    if (!(s->scale0 > 1.0) || !(s->scale0 <= 1e6)) return HOG_E_SCALE;
    if (!(fabs(s->hit_threshold) <= 1.7e308) || !(fabs(s->final_threshold) <= 1.7e308)) return HOG_E_THRESH;  // (NaN fails both)
    if (s->nlevels < 1 || s->nlevels > HOG_MAX_LEVELS) return HOG_E_LEVELS;
    if (s->max_hits < 1) return HOG_E_HITS;
    return HOG_OK;
}

// One level of the pyramid, and where its pixels, blocks and windows lie in the workspace and in each launch's grid
struct HogLevel {
    int h, w;            // the level image: (cv_round(Hp / s), cv_round(Wp / s))
    int copy;            // both sizes kept: the level is P itself
    int nbx, nby;        // blocks, one every 8 pixels: w / 8 - 1, h / 8 - 1
    int nwx, nwy;        // windows: (w - 64) / stride_x + 1, (h - 128) / stride_y + 1
    int vtx;             // vote tiles per tile row
    double s;            // the level's scale s_n
    double sx, sy;       // the resize's source steps: 1.0 / ((double)w / Wp), 1.0 / ((double)h / Hp) -- cv2's form when dsize is given
    long long pix0, blk0, win0;  // the level's first pixel / block / window in the workspace
    int vt0, bt0, wt0;   // the level's first workgroup in the vote / block / window launch
    int pad;
};
struct HogPlan {
    int n, Hp, Wp, stride_x, stride_y;
    int vtiles, btiles, wtiles;   // workgroups of the three launches
    long long npix, nblk, nwin;
    HogLevel lv[HOG_MAX_LEVELS];
};
// The level table of an (H, W) frame stored under orientation o.  HOST only (nearbyint in the default rounding mode).  A picture smaller
// than the window has no level; the loop stops at the first level that fails.
inline int hog_plan(int o, int H, int W, const HogSpec& sp, HogPlan* p)
{
    memset(p, 0, sizeof *p);
    orient_size(o, H, W, &p->Hp, &p->Wp);
    p->stride_x = sp.stride_x, p->stride_y = sp.stride_y;
    if (p->Hp > HOG_MAX_SIDE || p->Wp > HOG_MAX_SIDE) return HOG_E_SIDE;
    double s = 1.0;
    for (int n = 0; n < sp.nlevels; n++, s *= sp.scale0) {
        const int w = (int)nearbyint(p->Wp / s), h = (int)nearbyint(p->Hp / s);  // cv_round: half to even
        if (w < HOG_WIN_W || h < HOG_WIN_H) break;
        HogLevel& L = p->lv[p->n++];
        L.h = h, L.w = w, L.copy = h == p->Hp && w == p->Wp, L.s = s;
        L.sx = 1.0 / ((double)w / (double)p->Wp), L.sy = 1.0 / ((double)h / (double)p->Hp);
        L.nbx = w / HOG_CELL - 1, L.nby = h / HOG_CELL - 1;
        L.nwx = (w - HOG_WIN_W) / sp.stride_x + 1, L.nwy = (h - HOG_WIN_H) / sp.stride_y + 1;
        L.vtx = (w + HOG_VTILE_W - 1) / HOG_VTILE_W;
        L.pix0 = p->npix, L.blk0 = p->nblk, L.win0 = p->nwin;
        L.vt0 = p->vtiles, L.bt0 = p->btiles, L.wt0 = p->wtiles;
        p->npix += (long long)h * w, p->nblk += (long long)L.nbx * L.nby, p->nwin += (long long)L.nwx * L.nwy;
        p->vtiles += L.vtx * ((h + HOG_VTILE_H - 1) / HOG_VTILE_H);
        p->btiles += (L.nbx * L.nby + HOG_PER_WG - 1) / HOG_PER_WG;
        p->wtiles += (L.nwx * L.nwy + HOG_PER_WG - 1) / HOG_PER_WG;
    }
    return HOG_OK;
}

// The host-built tables: lut[v] = float32(sqrt(double(v))) (gamma correction); g[k] = float32(exp(-(k - 7.5)^2 / 32)), the Gaussian of
// sigma 4 over a 16-pixel block; wt[c][i * 16 + j]: the weight pixel (row i, column j) of a block gives cell c = cx * 2 + cy --
// (wx * wy) * (g[i] * g[j]) in float32, wx / wy the bilinear cell weights of cx / cy at (j + 0.5) / 8 - 0.5 and (i + 0.5) / 8 - 0.5
struct HogTables {
    float lut[256];
    float g[HOG_BLOCK];
    float wt[4][HOG_BLOCK * HOG_BLOCK];
};
inline float hog_cell_weight(int k, int cell)  // the bilinear weight pixel index k (row or column) gives cell 0 / 1 of its axis
{
    const float c = ((float)k + 0.5f) / 8.f - 0.5f, f0 = floorf(c), fr = c - f0;
    const int i0 = (int)f0;
    return (i0 == cell ? 1.f - fr : 0.f) + (i0 + 1 == cell ? fr : 0.f);
}
inline void hog_tables(HogTables* t)
{
    for (int v = 0; v < 256; v++) t->lut[v] = (float)sqrt((double)v);
    for (int k = 0; k < HOG_BLOCK; k++) t->g[k] = (float)exp(-((double)k - 7.5) * ((double)k - 7.5) / 32.0);
    for (int cx = 0; cx < 2; cx++)
        for (int cy = 0; cy < 2; cy++)
            for (int i = 0; i < HOG_BLOCK; i++)
                for (int j = 0; j < HOG_BLOCK; j++) {
                    const float cw = hog_cell_weight(j, cx) * hog_cell_weight(i, cy), gw = t->g[i] * t->g[j];
                    t->wt[cx * 2 + cy][i * HOG_BLOCK + j] = cw * gw;
                }
}

// the frame a detection reads: preview.h's source, orientation and stored size
struct HogSrc {
    OrientSrc src;
    int o, H, W;
};

// Pixel (y, x) of level L: cv2.resize(P, (w, h), INTER_LINEAR) in the pinned 8-bit fixed point (preview.h: preview_pixel's line)
VNECT_HD void hog_level_pixel(const HogSrc& a, int Hp, int Wp, const HogLevel& L, int y, int x, int* bgr)
{
    if (L.copy) {
        preview_src_pixel(a.src, a.o, a.H, a.W, y, x, bgr);
        return;
    }
    const AxE ex = axis_x_at(x, Wp, L.sx), ey = axis_y_at(y, Hp, L.sy);
    const int b0 = crop_sat((1.f - ey.f) * 2048.f), b1 = crop_sat(ey.f * 2048.f);
    int t0[3], t1[3], r0[3], r1[3];
    preview_src_pixel(a.src, a.o, a.H, a.W, ey.s0, ex.s0, t0);
    preview_src_pixel(a.src, a.o, a.H, a.W, ey.s1, ex.s0, t1);
    if (!ex.edge) {
        const int a0 = crop_sat((1.f - ex.f) * 2048.f), a1 = crop_sat(ex.f * 2048.f);
        int u0[3], u1[3];
        preview_src_pixel(a.src, a.o, a.H, a.W, ey.s0, ex.s0 + 1, u0);
        preview_src_pixel(a.src, a.o, a.H, a.W, ey.s1, ex.s0 + 1, u1);
        for (int c = 0; c < 3; c++) r0[c] = t0[c] * a0 + u0[c] * a1, r1[c] = t1[c] * a0 + u1[c] * a1;
    } else {
        for (int c = 0; c < 3; c++) r0[c] = t0[c] * 2048, r1[c] = t1[c] * 2048;
    }
    for (int c = 0; c < 3; c++) bgr[c] = (((b0 * (r0[c] >> 4)) >> 16) + ((b1 * (r1[c] >> 4)) >> 16) + 2) >> 2;
}

// The two votes of a pixel from its four neighbours (left, right, up, down; BGR): v0 into bin *h0, v1 into bin *h0 + 1 (0 at 9)
VNECT_HD void hog_vote(const float* lut, const int* pl, const int* pr, const int* pu, const int* pd, float* v0, float* v1, int* h0)
{
    float dx = lut[pr[2]] - lut[pl[2]], dy = lut[pd[2]] - lut[pu[2]];
    float m2 = dx * dx + dy * dy;
    for (int c = 1; c >= 0; c--) {
        const float ex = lut[pr[c]] - lut[pl[c]], ey = lut[pd[c]] - lut[pu[c]];
        const float n2 = ex * ex + ey * ey;
        if (n2 > m2) dx = ex, dy = ey, m2 = n2;
    }
    const float mag = sqrtf(m2);
    const float ax = fabsf(dx), ay = fabsf(dy);
    const float mn = ax < ay ? ax : ay, mx = ax < ay ? ay : ax;
    const float c = mn / (mx + HOG_ATAN_EPS), c2 = c * c;
    float a = c * (HOG_K0 + c2 * (HOG_K1 + c2 * (HOG_K2 + c2 * HOG_K3)));
    if (ay > ax) a = HOG_HALF_PI - a;
    if (dx < 0.f) a = HOG_PI - a;
    if (dy < 0.f) a = HOG_TWO_PI - a;
    const float pos = a * HOG_BINS_PER_RAD - 0.5f, fl = floorf(pos), fr = pos - fl;
    int h = (int)fl;
    if (h < 0) h += HOG_NBINS;
    if (h >= HOG_NBINS) h -= HOG_NBINS;
    *h0 = h, *v0 = mag * (1.f - fr), *v1 = mag * fr;
}

// One lane of the vote launch: pixel (y, x) of level L, borders reflect-101
VNECT_HD void hog_vote_at(const HogSrc& a, int Hp, int Wp, const HogLevel& L, const float* lut, int y, int x, float* v0, float* v1, int* h0)
{
    const int xl = x > 0 ? x - 1 : 1, xr = x + 1 < L.w ? x + 1 : L.w - 2, yu = y > 0 ? y - 1 : 1, yd = y + 1 < L.h ? y + 1 : L.h - 2;
    int pl[3], pr[3], pu[3], pd[3];
    hog_level_pixel(a, Hp, Wp, L, y, xl, pl);
    hog_level_pixel(a, Hp, Wp, L, y, xr, pr);
    hog_level_pixel(a, Hp, Wp, L, yu, x, pu);
    hog_level_pixel(a, Hp, Wp, L, yd, x, pd);
    hog_vote(lut, pl, pr, pu, pd, v0, v1, h0);
}

// One lane of the block launch: R(c, b, i) for the nine bins b, from row i of the block's votes (16 pixels) and row i of cell c's weights
VNECT_HD void hog_row_partial(const float* wt_row, const float* v0, const float* v1, const uint8_t* h0, float* acc9)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int b = 0; b < HOG_NBINS; b++) acc9[b] = 0.f;
    for (int j = 0; j < HOG_BLOCK; j++) {
        const int h = h0[j], h1 = h + 1 == HOG_NBINS ? 0 : h + 1;
        const float t0 = wt_row[j] * v0[j], t1 = wt_row[j] * v1[j];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int b = 0; b < HOG_NBINS; b++) acc9[b] += h == b ? t0 : (h1 == b ? t1 : 0.f);
    }
}
// hist[k], k = c * 9 + b, from the row partials R[(k * 16) + i]
VNECT_HD float hog_hist_sum(const float* Rk)
{
    float s = 0.f;
    for (int i = 0; i < HOG_BLOCK; i++) s += Rk[i];
    return s;
}
// L2-Hys: element k of the normalised block from the 36 sums
VNECT_HD float hog_l2hys(const float* hist, int k)
{
    float s1 = 0.f;
    for (int q = 0; q < HOG_BLOCK_LEN; q++) s1 += hist[q] * hist[q];
    const float sc1 = 1.f / (sqrtf(s1) + HOG_L2_EPS);
    float s2 = 0.f;
    for (int q = 0; q < HOG_BLOCK_LEN; q++) {
        const float u = fminf(hist[q] * sc1, HOG_CLIP);
        s2 += u * u;
    }
    const float sc2 = 1.f / (sqrtf(s2) + HOG_L2_EPS2);
    return fminf(hist[k] * sc1, HOG_CLIP) * sc2;
}
// T(bx, by): a block's share of a window's score
VNECT_HD float hog_block_dot(const float* det36, const float* desc36)
{
    float s = 0.f;
    for (int k = 0; k < HOG_BLOCK_LEN; k++) s += det36[k] * desc36[k];
    return s;
}
// the score from the 105 shares T[bx * 15 + by]
VNECT_HD float hog_score(const float* T, float rho)
{
    float S = 0.f;
    for (int bx = 0; bx < HOG_WIN_BX; bx++) {
        float C = 0.f;
        for (int by = 0; by < HOG_WIN_BY; by++) C += T[bx * HOG_WIN_BY + by];
        S += C;
    }
    return rho + S;
}

// a window that cleared hit_threshold, as the window launch appends it (in any order) and the host orders it
struct HogHit {
    int level, y, x;
    float s;
};

// ---- host only: hits -> rectangles -> groupRectangles ------------------------------------------------------------------------------------
struct HogRect {
    int x, y, w, h;
};
inline int hog_round(double v) { return (int)nearbyint(v); }  // cv_round: half to even

// the hits in the order (level, y, x), their rectangles in picture coordinates and their weights
inline void hog_hit_rects(const HogPlan& p, std::vector<HogHit>& hits, std::vector<HogRect>* rects, std::vector<double>* weights)
{
    std::sort(hits.begin(), hits.end(), [](const HogHit& a, const HogHit& b) { return a.level != b.level ? a.level < b.level : (a.y != b.y ? a.y < b.y : a.x < b.x); });
    rects->clear(), weights->clear();
    for (const HogHit& t : hits) {
        const double s = p.lv[t.level].s;
        rects->push_back(HogRect{hog_round(t.x * s), hog_round(t.y * s), hog_round(HOG_WIN_W * s), hog_round(HOG_WIN_H * s)});
        weights->push_back((double)t.s);
    }
}
VNECT_HD bool hog_similar(const HogRect& a, const HogRect& b)
{
    const double d = HOG_GROUP_EPS * ((a.w < b.w ? a.w : b.w) + (a.h < b.h ? a.h : b.h)) * 0.5;
    return abs(a.x - b.x) <= d && abs(a.y - b.y) <= d && abs(a.x + a.w - b.x - b.w) <= d && abs(a.y + a.h - b.y - b.h) <= d;
}
// groupRectangles(rects, weights, threshold, eps = 0.2): classes are the connected components of hog_similar ordered by their lowest
// member; a class becomes its mean rect and its largest weight; classes of at most `threshold` members, and small classes inside
// large ones, are dropped.  threshold < 1: the hits as they are.
inline void hog_group(std::vector<HogRect>& rects, std::vector<double>& weights, int threshold)
{
    if (threshold < 1 || rects.empty()) return;
    const int n = (int)rects.size();
    std::vector<int> root(n);
    for (int i = 0; i < n; i++) root[i] = i;
    auto find = [&](int i) {
        while (root[i] != i) i = root[i] = root[root[i]];
        return i;
    };
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (hog_similar(rects[i], rects[j])) {
                const int a = find(i), b = find(j);
                if (a != b) root[a > b ? a : b] = a > b ? b : a;  // the lower index stays the root: a class is named by its lowest member
            }
    std::vector<int> cls(n, -1), count;
    std::vector<long long> sum;  // [class][4]
    std::vector<double> wmax;
    for (int i = 0; i < n; i++) {
        const int r = find(i);
        if (cls[r] < 0) cls[r] = (int)count.size(), count.push_back(0), sum.insert(sum.end(), 4, 0LL), wmax.push_back(weights[i]);
        const int c = cls[r];
        count[c]++, sum[4 * c] += rects[i].x, sum[4 * c + 1] += rects[i].y, sum[4 * c + 2] += rects[i].w, sum[4 * c + 3] += rects[i].h;
        if (weights[i] > wmax[c]) wmax[c] = weights[i];
    }
    const int nc = (int)count.size();
    std::vector<HogRect> mean(nc);
    for (int c = 0; c < nc; c++) {
        const float s = 1.f / (float)count[c];
        mean[c] = HogRect{hog_round((double)((float)sum[4 * c] * s)), hog_round((double)((float)sum[4 * c + 1] * s)), hog_round((double)((float)sum[4 * c + 2] * s)),
                          hog_round((double)((float)sum[4 * c + 3] * s))};
    }
    std::vector<HogRect> out;
    std::vector<double> wout;
    for (int i = 0; i < nc; i++) {
        const HogRect r1 = mean[i];
        const int n1 = count[i];
        if (n1 <= threshold) continue;
        int j = 0;
        for (; j < nc; j++) {
            const int n2 = count[j];
            if (j == i || n2 <= threshold) continue;
            const HogRect r2 = mean[j];
            const int dx = hog_round(r2.w * HOG_GROUP_EPS), dy = hog_round(r2.h * HOG_GROUP_EPS);
            if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.w <= r2.x + r2.w + dx && r1.y + r1.h <= r2.y + r2.h + dy && (n2 > (3 > n1 ? 3 : n1) || n1 < 3)) break;
        }
        if (j == nc) out.push_back(r1), wout.push_back(wmax[i]);
    }
    rects.swap(out), weights.swap(wout);
}
// the detector as a call holds it: 3781 floats, rho last (3780 given: rho 0); false: a length or an entry it refuses
inline bool hog_detector(const float* w, int n, std::vector<float>* det)
{
    if (!w || (n != HOG_DESC && n != HOG_DESC + 1)) return false;
    for (int i = 0; i < n; i++)
        if (!(fabsf(w[i]) <= FLT_MAX)) return false;
    det->assign(w, w + n);
    if (n == HOG_DESC) det->push_back(0.f);
    return true;
}

// ---- re-detection inside the device tracking loop (vnect_track_redetect): hits -> the stream's next crop, host and device -------------------
// THE RULE.  While re-detection is set on a tracked stream, the next box of a frame that the stream's loss rule (CONFIDENCE.md) declares
// lost is runner.hog_box of that frame -- under "hold" as under "reset"; with the rule off no frame is ever lost.  hog_box here: the hits
// become rectangles as hog_hit_rects makes them, are grouped as hog_group groups them, the class of the largest w * h wins -- the first of
// equals in hog_group's class order, which is the order of the classes' lowest (level, y, x) members --, and goes through cal_rect; when no
// class survives the box is [0, 0, W, H].  The box then takes the crop_head / crop_entry / crop_fill_head path of any box.  One stated
// difference from the host loop: more hits than max_hits make the host loop raise; the device loop takes the whole frame and reports
// HOG_RD_OVERFLOW.
// hog_pick_* below are the phases of hog_pick_kernel (hog.hip), written once for the kernel's lanes and for g++'s walk of them
// (hog_capi.cpp): `tid` of `nthr` lanes, a barrier between two phases.  A hit is one 32-bit key, level << 24 | y << 12 | x (sides are at
// most 4096, levels at most 64): keys are unique per hit and order as (level, y, x), so sorting the keys makes the slot order the order
// hog_hit_rects gives and nothing depends on the order in which lanes appended the hits.  Classes are the components of hog_similar, named
// by their lowest slot: a lock-free union (compare-and-swap of a root's parent, the higher root under the lower) whose final partition and
// names do not depend on scheduling, path halving while it runs and pointer jumping to flatten it; sums in integer atomics.
constexpr int HOG_TRACK_MAX_HITS = 4096;  // the hit budget of a tracked stream: keys, rects and labels of one detection fit one workgroup's LDS
constexpr int HOG_PICK_THREADS = 1024;
enum { HOG_RD_NOT_RUN = 0, HOG_RD_FOUND = 1, HOG_RD_NOBODY = 2, HOG_RD_OVERFLOW = 3 };
struct RedetectOut {  // per result-ring slot (device-mapped pinned host memory): vnect_result_redetect
    int status;       // HOG_RD_*
    int rect[4];      // the chosen detection before cal_rect; written only with HOG_RD_FOUND
    int hits;         // the full hit count; written whenever the detection ran
};

VNECT_HD int hog_rint(double v) { return (int)rint(v); }  // cv_round on both sides: half to even in the default rounding mode
VNECT_HD unsigned hog_key(int level, int y, int x) { return (unsigned)level << 24 | (unsigned)y << 12 | (unsigned)x; }
// cal_rect (hog_box.py:48-58; runner.cal_rect), term by term
VNECT_HD void hog_cal_rect(const int* r, int H, int W, int* out)
{
    const int ow = (int)(0.4 / 2 * (double)W), oh = (int)(0.2 / 2 * (double)H);
    const int x0 = r[0] - ow > 0 ? r[0] - ow : 0, y0 = r[1] - oh > 0 ? r[1] - oh : 0;
    const int x1 = r[0] + r[2] + ow < W ? r[0] + r[2] + ow : W, y1 = r[1] + r[3] + oh < H ? r[1] + r[3] + oh : H;
    out[0] = x0, out[1] = y0, out[2] = x1 - x0, out[3] = y1 - y0;
}
// a class's mean field as hog_group rounds it
VNECT_HD int hog_class_mean(int sum, int n) { return hog_rint((double)((float)sum * (1.f / (float)n))); }
// hog_group's second drop rule: class (r1, n1) lies inside the surviving class (r2, n2)
VNECT_HD bool hog_class_inside(const HogRect& r1, int n1, const HogRect& r2, int n2)
{
    const int dx = hog_rint(r2.w * HOG_GROUP_EPS), dy = hog_rint(r2.h * HOG_GROUP_EPS);
    return r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.w <= r2.x + r2.w + dx && r1.y + r1.h <= r2.y + r2.h + dy && (n2 > (3 > n1 ? 3 : n1) || n1 < 3);
}

#if defined(__HIP_DEVICE_COMPILE__)
VNECT_HD int hog_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
VNECT_HD int hog_ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
VNECT_HD void hog_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
VNECT_HD void hog_st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
VNECT_HD int hog_cas(int* p, int cmp, int v) { return atomicCAS(p, cmp, v); }
VNECT_HD void hog_add(int* p, int v) { atomicAdd(p, v); }
VNECT_HD void hog_max64(unsigned long long* p, unsigned long long v) { atomicMax(p, v); }
#else  // g++'s walk runs the lanes one after the other
VNECT_HD int hog_ld(const int* p) { return *p; }
VNECT_HD int hog_ld_agent(const int* p) { return *p; }
VNECT_HD void hog_st(int* p, int v) { *p = v; }
VNECT_HD void hog_st_agent(int* p, int v) { *p = v; }
VNECT_HD int hog_cas(int* p, int cmp, int v)
{
    const int o = *p;
    if (o == cmp) *p = v;
    return o;
}
VNECT_HD void hog_add(int* p, int v) { *p += v; }
VNECT_HD void hog_max64(unsigned long long* p, unsigned long long v)
{
    if (v > *p) *p = v;
}
#endif

// What one pick works on.  a, b, c: three arrays of HOG_TRACK_MAX_HITS words in the workgroup's LDS, which change their meaning as the
// phases go: keys / rect origins / parents, then -- per class, at its root's slot -- (w | h << 16) / (x | y << 16) / member count.
// cls: 5 * HOG_TRACK_MAX_HITS ints of device memory (count, sum x, sum y, sum w, sum h per root), all zero between two picks.
struct HogPick {
    unsigned* a;
    unsigned* b;
    int* c;
    int* cls;
    const HogLevel* lv;
    unsigned long long* best;  // (area << 12 | 4095 - root) of the winning class, 0: none
    int n, np2, threshold;
};
VNECT_HD HogRect hog_pick_rect(const HogPick& m, int i)  // slot i's rectangle (phases 2 .. 5)
{
    const double s = m.lv[m.a[i] >> 24].s;
    return HogRect{(int)(m.b[i] & 0xffffu), (int)(m.b[i] >> 16), hog_rint(HOG_WIN_W * s), hog_rint(HOG_WIN_H * s)};
}
VNECT_HD int hog_pick_find(int* parent, int i)  // the root of i; halves the path (every write is an ancestor of the slot it replaces)
{
    int p = hog_ld(parent + i);
    while (p != i) {
        const int g = hog_ld(parent + p);
        if (g != p) hog_st(parent + i, g);
        i = p, p = g;
    }
    return i;
}
// phase 0: the keys of the first n hits (n <= HOG_TRACK_MAX_HITS), padded to a power of two with keys behind every hit's
VNECT_HD void hog_pick_load(const HogPick& m, const HogHit* hits, int tid, int nthr)
{
    for (int i = tid; i < m.np2; i += nthr) m.a[i] = i < m.n ? hog_key(hits[i].level, hits[i].y, hits[i].x) : 0xffffffffu;
    if (tid == 0) *m.best = 0ull;
}
// phase 1, once per (k, j) of a bitonic sort over np2 keys: k = 2, 4 .. np2; j = k / 2, k / 4 .. 1
VNECT_HD void hog_pick_sort_step(const HogPick& m, int k, int j, int tid, int nthr)
{
    for (int i = tid; i < m.np2; i += nthr) {
        const int l = i ^ j;
        if (l > i) {
            const unsigned x = m.a[i], y = m.a[l];
            if (((i & k) == 0) == (x > y)) m.a[i] = y, m.a[l] = x;
        }
    }
}
// phase 2: the rect origins (cv_round(x * s), cv_round(y * s)) and every slot its own class
VNECT_HD void hog_pick_init(const HogPick& m, int tid, int nthr)
{
    for (int i = tid; i < m.n; i += nthr) {
        const unsigned key = m.a[i];
        const double s = m.lv[key >> 24].s;
        m.b[i] = (unsigned)hog_rint((int)(key & 0xfffu) * s) | (unsigned)hog_rint((int)(key >> 12 & 0xfffu) * s) << 16;
        m.c[i] = i;
    }
}
// phase 3: every similar pair (i < j) joins its two classes (threshold < 1: hog_group leaves the hits as they are)
VNECT_HD void hog_pick_union(const HogPick& m, int tid, int nthr)
{
    if (m.threshold < 1) return;
    for (int i = tid; i < m.n; i += nthr) {
        const HogRect ri = hog_pick_rect(m, i);
        for (int j = i + 1; j < m.n; j++) {
            if (!hog_similar(ri, hog_pick_rect(m, j))) continue;
            int x = hog_pick_find(m.c, i), y = hog_pick_find(m.c, j);
            while (x != y) {  // the higher root goes under the lower; a lost race moves on to that root's new parent
                const int hi = x > y ? x : y, lo = x > y ? y : x;
                const int old = hog_cas(m.c + hi, hi, lo);
                if (old == hi) break;
                x = hog_pick_find(m.c, old), y = lo;
            }
        }
    }
}
// phase 4: pointer jumping -- every slot's parent becomes its root
VNECT_HD void hog_pick_flatten(const HogPick& m, int tid, int nthr)
{
    for (int i = tid; i < m.n; i += nthr) {
        int r = hog_ld(m.c + i);
        for (int p = hog_ld(m.c + r); p != r; p = hog_ld(m.c + r)) r = p;
        hog_st(m.c + i, r);
    }
}
// phase 5: the class sums, integers
VNECT_HD void hog_pick_sums(const HogPick& m, int tid, int nthr)
{
    for (int i = tid; i < m.n; i += nthr) {
        const HogRect r = hog_pick_rect(m, i);
        int* q = m.cls + m.c[i];
        hog_add(q, 1), hog_add(q + HOG_TRACK_MAX_HITS, r.x), hog_add(q + 2 * HOG_TRACK_MAX_HITS, r.y), hog_add(q + 3 * HOG_TRACK_MAX_HITS, r.w),
            hog_add(q + 4 * HOG_TRACK_MAX_HITS, r.h);
    }
}
// phase 6: every root's mean rect and count into its own slot of the three arrays (0 members: not a root); the sums go back to zero
VNECT_HD void hog_pick_means(const HogPick& m, int tid, int nthr)
{
    for (int r = tid; r < m.n; r += nthr) {
        int* q = m.cls + r;
        const int cnt = m.c[r] == r ? hog_ld_agent(q) : 0;
        if (cnt) {
            int f[4];
            for (int k = 0; k < 4; k++) f[k] = hog_class_mean(hog_ld_agent(q + (k + 1) * HOG_TRACK_MAX_HITS), cnt);
            m.b[r] = (unsigned)f[0] | (unsigned)f[1] << 16, m.a[r] = (unsigned)f[2] | (unsigned)f[3] << 16;
            for (int k = 0; k < 5; k++) hog_st_agent(q + k * HOG_TRACK_MAX_HITS, 0);
        }
        m.c[r] = cnt;
    }
}
VNECT_HD HogRect hog_pick_mean(const HogPick& m, int r) { return HogRect{(int)(m.b[r] & 0xffffu), (int)(m.b[r] >> 16), (int)(m.a[r] & 0xffffu), (int)(m.a[r] >> 16)}; }
// phase 7: hog_group's two drop rules; of the classes that stay, the largest w * h, ties to the lowest root
VNECT_HD void hog_pick_best(const HogPick& m, int tid, int nthr)
{
    for (int i = tid; i < m.n; i += nthr) {
        const int n1 = m.c[i];
        if (n1 == 0 || (m.threshold >= 1 && n1 <= m.threshold)) continue;
        const HogRect r1 = hog_pick_mean(m, i);
        int j = m.n;
        if (m.threshold >= 1)
            for (j = 0; j < m.n; j++) {
                const int n2 = m.c[j];
                if (j == i || n2 <= m.threshold) continue;
                if (hog_class_inside(r1, n1, hog_pick_mean(m, j), n2)) break;
            }
        if (j == m.n) hog_max64(m.best, (unsigned long long)((long long)r1.w * r1.h) << 12 | (unsigned long long)(HOG_TRACK_MAX_HITS - 1 - i));
    }
}
// phase 8 (one lane): the verdict -- `count` is the window launch's counter; next4: the stream's next box
VNECT_HD void hog_pick_result(const HogPick& m, unsigned count, int max_hits, int H, int W, RedetectOut* out, int* next4)
{
    next4[0] = 0, next4[1] = 0, next4[2] = W, next4[3] = H;
    out->hits = (int)count;
    if (count > (unsigned)max_hits) {
        out->status = HOG_RD_OVERFLOW;
    } else if (*m.best == 0ull) {
        out->status = HOG_RD_NOBODY;
    } else {
        const HogRect r = hog_pick_mean(m, HOG_TRACK_MAX_HITS - 1 - (int)(*m.best & 0xfffull));
        const int d[4] = {r.x, r.y, r.w, r.h};
        hog_cal_rect(d, H, W, next4);
        out->rect[0] = r.x, out->rect[1] = r.y, out->rect[2] = r.w, out->rect[3] = r.h;
        out->status = HOG_RD_FOUND;
    }
}

}  // namespace vnect
