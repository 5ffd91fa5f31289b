// hog_capi.cpp -- C shim over hog.h for tests/test_hog_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.  Built with plain
// g++ (`make -C vnect_amd/csrc hog`).  hog_walk goes through a detection the way the kernels of hog.hip do -- level by level through the
// level table, workgroup by workgroup, wave by wave, lane by lane, with the SAME functions for a level pixel, a vote, a row partial, the
// normalisation and a score -- so the rule as the device runs it is held to an independent statement of it (tests/hog_ref.py) without a
// GPU.  Loads and stores go straight to the caller's buffers: with -DHOG_SWEEP_MAIN (`make ... hog_sweep_asan`,
// -fsanitize=address,undefined) the same file is a stand-alone program whose frames and workspaces sit in exactly sized heap blocks.
// hog_pick_walk goes through the pick of a re-detection (hog.h: THE RULE) phase by phase, lane by lane, as hog_pick_kernel does;
// -DREDETECT_SWEEP_MAIN (`make ... redetect_sweep_asan`) is the stand-alone program over it, hit lists in exactly sized heap blocks.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hog.h"

using namespace vnect;

namespace {

constexpr int R_STRIDE = HOG_BLOCK + 1;  // hog.hip: HOG_R_STRIDE

void walk_votes(const HogSrc& a, const HogPlan& p, const HogTables& tab, uint8_t* level_img, float* votes, uint8_t* bins)
{
    for (int n = 0; n < p.n; n++) {
        const HogLevel& L = p.lv[n];
        const int tiles = L.vtx * ((L.h + HOG_VTILE_H - 1) / HOG_VTILE_H);
        for (int tile = 0; tile < tiles; tile++)
            for (int tid = 0; tid < HOG_THREADS; tid++) {
                const int ty = tile / L.vtx, tx = tile - ty * L.vtx;
                const int y = ty * HOG_VTILE_H + tid / HOG_VTILE_W, x = tx * HOG_VTILE_W + tid % HOG_VTILE_W;
                if (y >= L.h || x >= L.w) continue;
                float v0, v1;
                int h0;
                hog_vote_at(a, p.Hp, p.Wp, L, tab.lut, y, x, &v0, &v1, &h0);
                const long long at = L.pix0 + (long long)y * L.w + x;
                votes[2 * at] = v0, votes[2 * at + 1] = v1, bins[at] = (uint8_t)h0;
                if (level_img) {  // (the kernel never stores the level images; the walk shows them to the tests)
                    int c[3];
                    hog_level_pixel(a, p.Hp, p.Wp, L, y, x, c);
                    for (int k = 0; k < 3; k++) level_img[3 * at + k] = (uint8_t)c[k];
                }
            }
    }
}

void walk_blocks(const HogPlan& p, const HogTables& tab, const float* votes, const uint8_t* bins, float* blocks)
{
    for (int n = 0; n < p.n; n++) {
        const HogLevel& L = p.lv[n];
        const int nb = L.nbx * L.nby;
        for (int b = 0; b < nb; b++) {  // one wave
            const int by = b / L.nbx, bx = b - by * L.nbx;
            float sv0[HOG_BLOCK * HOG_BLOCK], sv1[HOG_BLOCK * HOG_BLOCK], R[HOG_BLOCK_LEN * R_STRIDE], hist[HOG_BLOCK_LEN];
            uint8_t sh[HOG_BLOCK * HOG_BLOCK];
            for (int lane = 0; lane < 64; lane++) {
                const int i = lane >> 2, j0 = (lane & 3) * 4;
                const long long at = L.pix0 + (long long)(by * HOG_CELL + i) * L.w + bx * HOG_CELL + j0;
                for (int q = 0; q < 4; q++) sv0[i * HOG_BLOCK + j0 + q] = votes[2 * (at + q)], sv1[i * HOG_BLOCK + j0 + q] = votes[2 * (at + q) + 1], sh[i * HOG_BLOCK + j0 + q] = bins[at + q];
            }
            for (int lane = 0; lane < 64; lane++) {
                const int c = lane >> 4, i = lane & 15;
                float acc[HOG_NBINS];
                hog_row_partial(&tab.wt[c][i * HOG_BLOCK], &sv0[i * HOG_BLOCK], &sv1[i * HOG_BLOCK], &sh[i * HOG_BLOCK], acc);
                for (int q = 0; q < HOG_NBINS; q++) R[(c * HOG_NBINS + q) * R_STRIDE + i] = acc[q];
            }
            for (int lane = 0; lane < HOG_BLOCK_LEN; lane++) hist[lane] = hog_hist_sum(&R[lane * R_STRIDE]);
            for (int lane = 0; lane < HOG_BLOCK_LEN; lane++) blocks[(L.blk0 + b) * HOG_BLOCK_LEN + lane] = hog_l2hys(hist, lane);
        }
    }
}

// returns the number of windows that cleared the threshold; the first max_hits of them are appended to `hits`
long long walk_windows(const HogPlan& p, const float* det, const float* blocks, double hit_threshold, int max_hits, float* scores, std::vector<HogHit>* hits)
{
    long long count = 0;
    for (int n = 0; n < p.n; n++) {
        const HogLevel& L = p.lv[n];
        for (int wi = 0; wi < L.nwx * L.nwy; wi++) {  // one wave
            const int wy = wi / L.nwx, wx = wi - wy * L.nwx, x = wx * p.stride_x, y = wy * p.stride_y;
            float T[HOG_WIN_BX * HOG_WIN_BY];
            for (int lane = 0; lane < 64; lane++)
                for (int t = lane; t < HOG_WIN_BX * HOG_WIN_BY; t += 64) {
                    const int bx = t / HOG_WIN_BY, by = t - bx * HOG_WIN_BY;
                    const long long blk = L.blk0 + (long long)(y / HOG_CELL + by) * L.nbx + (x / HOG_CELL + bx);
                    T[t] = hog_block_dot(det + t * HOG_BLOCK_LEN, blocks + blk * HOG_BLOCK_LEN);
                }
            const float s = hog_score(T, det[HOG_DESC]);
            if (scores) scores[L.win0 + wi] = s;
            if ((double)s >= hit_threshold) {
                if (count < max_hits) hits->push_back(HogHit{n, y, x, s});
                count++;
            }
        }
    }
    return count;
}

// the frame's description -> a->src, a->H, a->W, a->o; false: a frame the runtime would refuse
bool source_of(HogSrc* a, const uint8_t* base, int64_t size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
               int64_t uv_stride, int orient)
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

// [0] lanes per workgroup, [1] the vote tile's width and [2] height in level pixels, [3] blocks / windows per workgroup
void hog_tile(int32_t* out) { out[0] = HOG_THREADS, out[1] = HOG_VTILE_W, out[2] = HOG_VTILE_H, out[3] = HOG_PER_WG; }

// the host-built tables: lut[256], g[16], wt[4 * 256]
void hog_tables_c(float* lut, float* g, float* wt)
{
    HogTables t;
    hog_tables(&t);
    memcpy(lut, t.lut, sizeof t.lut), memcpy(g, t.g, sizeof t.g), memcpy(wt, t.wt, sizeof t.wt);
}

// The level table of a stored (H, W) frame under `orient` (zero spec fields: the defaults): n_out levels, hw_out[2 n] (rows, columns),
// scales_out[n], geom_out[4 n] (nbx, nby, nwx, nwy), totals[3] (pixels, blocks, windows) -- each may be null.  0, or hog.h's refusal code.
int hog_levels_c(int orient, int H, int W, double hit_threshold, int sx, int sy, double scale0, double final_threshold, int nlevels, int max_hits,
                 int32_t* n_out, int32_t* hw_out, double* scales_out, int32_t* geom_out, int64_t* totals)
{
    if (!orient_ok(orient) || H < 1 || W < 1) return -1;
    HogSpec sp;
    int rc = hog_spec(hit_threshold, sx, sy, scale0, final_threshold, nlevels, max_hits, &sp);
    if (rc) return rc;
    static thread_local HogPlan p;
    if ((rc = hog_plan(orient, H, W, sp, &p))) return rc;
    if (n_out) *n_out = p.n;
    for (int n = 0; n < p.n; n++) {
        const HogLevel& L = p.lv[n];
        if (hw_out) hw_out[2 * n] = L.h, hw_out[2 * n + 1] = L.w;
        if (scales_out) scales_out[n] = L.s;
        if (geom_out) geom_out[4 * n] = L.nbx, geom_out[4 * n + 1] = L.nby, geom_out[4 * n + 2] = L.nwx, geom_out[4 * n + 3] = L.nwy;
    }
    if (totals) totals[0] = p.npix, totals[1] = p.nblk, totals[2] = p.nwin;
    return 0;
}

// The detection of the frame whose pixel (0, 0) channel 0 (NV12: Y plane) lies data_off bytes into [src, src + src_size), the UV plane
// uv_off bytes in; format 0 BGR, 1 RGB, 2 NV12.  det[ndet]: the detector.  The stages' outputs, each may be null: level_img [3 npix],
// votes [2 npix], bins [npix], blocks [36 nblk], scores [nwin]; hits3 [3 max_hits] (level, y, x) and hit_s [max_hits] in the order
// (level, y, x), nhits_out; the grouped rects4 [4 capacity] and weights [capacity], count_out (the full count, also above capacity).
// Returns 0; -1 for arguments the runtime would refuse; -2 when more than max_hits windows clear hit_threshold (then no hit, no rect
// and no count is written).
int hog_walk(const uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
             int64_t uv_stride, int src_has_rect, int orient, double hit_threshold, int stride_x, int stride_y, double scale0, double final_threshold,
             int nlevels, int max_hits, const float* det, int ndet, uint8_t* level_img, float* votes, uint8_t* bins, float* blocks, float* scores,
             int32_t* hits3, float* hit_s, int32_t* nhits_out, int32_t* rects4, double* weights, int capacity, int32_t* count_out)
{
    HogSrc a;
    memset(&a, 0, sizeof a);
    std::vector<float> d;
    if (src_has_rect || !hog_detector(det, ndet, &d) || capacity < 0) return -1;
    if (!source_of(&a, src, src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, orient)) return -1;
    HogSpec sp;
    if (hog_spec(hit_threshold, stride_x, stride_y, scale0, final_threshold, nlevels, max_hits, &sp)) return -1;
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(orient, H, W, sp, &p)) return -1;
    std::vector<HogHit> hits;
    if (p.n) {
        HogTables tab;
        hog_tables(&tab);
        std::vector<float> v, b;
        std::vector<uint8_t> q;
        if (!votes) v.resize(2 * (size_t)p.npix), votes = v.data();
        if (!bins) q.resize((size_t)p.npix), bins = q.data();
        if (!blocks) b.resize(HOG_BLOCK_LEN * (size_t)p.nblk), blocks = b.data();
        walk_votes(a, p, tab, level_img, votes, bins);
        walk_blocks(p, tab, votes, bins, blocks);
        if (walk_windows(p, d.data(), blocks, sp.hit_threshold, sp.max_hits, scores, &hits) > sp.max_hits) return -2;
    }
    std::vector<HogRect> rects;
    std::vector<double> ws;
    hog_hit_rects(p, hits, &rects, &ws);
    for (size_t i = 0; i < hits.size(); i++) {
        if (hits3) hits3[3 * i] = hits[i].level, hits3[3 * i + 1] = hits[i].y, hits3[3 * i + 2] = hits[i].x;
        if (hit_s) hit_s[i] = hits[i].s;
    }
    if (nhits_out) *nhits_out = (int32_t)hits.size();
    hog_group(rects, ws, (int)sp.final_threshold);
    for (size_t i = 0; i < rects.size() && (int)i < capacity; i++) {
        if (rects4) rects4[4 * i] = rects[i].x, rects4[4 * i + 1] = rects[i].y, rects4[4 * i + 2] = rects[i].w, rects4[4 * i + 3] = rects[i].h;
        if (weights) weights[i] = ws[i];
    }
    if (count_out) *count_out = (int32_t)rects.size();
    return 0;
}

// hits (level, y, x) of an (H, W) frame's level table -> their rectangles, in the order given (which must be the order (level, y, x))
int hog_rects_c(int orient, int H, int W, double scale0, int nlevels, const int32_t* hits3, int n, int32_t* rects4)
{
    HogSpec sp;
    if (!orient_ok(orient) || H < 1 || W < 1 || hog_spec(0.0, 0, 0, scale0, 0.0, nlevels, 0, &sp)) return -1;
    std::vector<HogPlan> pv(1);
    if (hog_plan(orient, H, W, sp, &pv[0])) return -1;
    std::vector<HogHit> hits;
    for (int i = 0; i < n; i++) {
        if (hits3[3 * i] < 0 || hits3[3 * i] >= pv[0].n) return -1;
        hits.push_back(HogHit{hits3[3 * i], hits3[3 * i + 1], hits3[3 * i + 2], 0.f});
    }
    std::vector<HogRect> rects;
    std::vector<double> ws;
    hog_hit_rects(pv[0], hits, &rects, &ws);
    for (int i = 0; i < n; i++) rects4[4 * i] = rects[i].x, rects4[4 * i + 1] = rects[i].y, rects4[4 * i + 2] = rects[i].w, rects4[4 * i + 3] = rects[i].h;
    return 0;
}

// groupRectangles in place: rects4 [4 n], weights [n] -> the first *n_out of them
int hog_group_c(int32_t* rects4, double* weights, int n, int threshold, int32_t* n_out)
{
    if (n < 0 || !n_out) return -1;
    std::vector<HogRect> r;
    std::vector<double> w(weights, weights + n);
    for (int i = 0; i < n; i++) r.push_back(HogRect{rects4[4 * i], rects4[4 * i + 1], rects4[4 * i + 2], rects4[4 * i + 3]});
    hog_group(r, w, threshold);
    for (size_t i = 0; i < r.size(); i++) rects4[4 * i] = r[i].x, rects4[4 * i + 1] = r[i].y, rects4[4 * i + 2] = r[i].w, rects4[4 * i + 3] = r[i].h, weights[i] = w[i];
    *n_out = (int32_t)r.size();
    return 0;
}

// The pick of a re-detection as hog_pick_kernel (hog.hip) runs it: `nthr` lanes one after the other through every phase, a barrier
// between two phases.  The frame is stored (H, W) under `orient`; hits3 [3 n] are the hits as the window launch left them (ANY order),
// n = min(count, max_hits) of them; count: the launch's counter.  out6: status, the chosen rect, the hit count; next4: the stream's next
// box.  Returns 0; -1 for arguments the runtime refuses; -3 when the class sums were not left at zero.
int hog_pick_walk(int orient, int H, int W, double scale0, int nlevels, const int32_t* hits3, int n, int64_t count, int max_hits, int threshold, int nthr,
                  int32_t* out6, int32_t* next4)
{
    HogSpec sp;
    if (!orient_ok(orient) || H < 1 || W < 1 || hog_spec(0.0, 0, 0, scale0, 0.0, nlevels, max_hits, &sp)) return -1;
    if (max_hits < 1 || max_hits > HOG_TRACK_MAX_HITS || nthr < 1 || count < 0 || n < 0 || n != (count < max_hits ? count : max_hits)) return -1;
    std::vector<HogPlan> pv(1);
    if (hog_plan(orient, H, W, sp, &pv[0])) return -1;
    const HogPlan& p = pv[0];
    std::vector<HogHit> hits;
    for (int i = 0; i < n; i++) {
        if (hits3[3 * i] < 0 || hits3[3 * i] >= p.n || hits3[3 * i + 1] < 0 || hits3[3 * i + 1] >= HOG_MAX_SIDE || hits3[3 * i + 2] < 0 || hits3[3 * i + 2] >= HOG_MAX_SIDE) return -1;
        hits.push_back(HogHit{hits3[3 * i], hits3[3 * i + 1], hits3[3 * i + 2], 0.f});
    }
    std::vector<unsigned> a(HOG_TRACK_MAX_HITS), b(HOG_TRACK_MAX_HITS);
    std::vector<int> c(HOG_TRACK_MAX_HITS), cls(5 * HOG_TRACK_MAX_HITS, 0);
    unsigned long long best = ~0ull;
    HogPick m{a.data(), b.data(), c.data(), cls.data(), p.lv, &best, 0, 1, threshold};
    m.n = count > max_hits ? 0 : n;
    while (m.np2 < m.n) m.np2 <<= 1;
#define PICK_PHASE(call) \
    for (int tid = 0; tid < nthr; tid++) call
    PICK_PHASE(hog_pick_load(m, hits.data(), tid, nthr));
    for (int k = 2; k <= m.np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) PICK_PHASE(hog_pick_sort_step(m, k, j, tid, nthr));
    PICK_PHASE(hog_pick_init(m, tid, nthr));
    PICK_PHASE(hog_pick_union(m, tid, nthr));
    PICK_PHASE(hog_pick_flatten(m, tid, nthr));
    PICK_PHASE(hog_pick_sums(m, tid, nthr));
    PICK_PHASE(hog_pick_means(m, tid, nthr));
    PICK_PHASE(hog_pick_best(m, tid, nthr));
#undef PICK_PHASE
    RedetectOut out{};
    int next[4];
    hog_pick_result(m, (unsigned)count, max_hits, p.Hp, p.Wp, &out, next);
    out6[0] = out.status, out6[5] = out.hits;
    for (int k = 0; k < 4; k++) out6[1 + k] = out.rect[k], next4[k] = next[k];
    for (int v : cls)
        if (v) return -3;
    return 0;
}

// The same verdict from the host's own pieces: hog_hit_rects, hog_group, the largest w * h (the first of equals), cal_rect
int hog_pick_ref(int orient, int H, int W, double scale0, int nlevels, const int32_t* hits3, int n, int64_t count, int max_hits, int threshold, int32_t* out6,
                 int32_t* next4)
{
    HogSpec sp;
    if (!orient_ok(orient) || H < 1 || W < 1 || hog_spec(0.0, 0, 0, scale0, 0.0, nlevels, max_hits, &sp) || n < 0 || count < 0) return -1;
    std::vector<HogPlan> pv(1);
    if (hog_plan(orient, H, W, sp, &pv[0])) return -1;
    const HogPlan& p = pv[0];
    for (int k = 0; k < 6; k++) out6[k] = 0;
    next4[0] = 0, next4[1] = 0, next4[2] = p.Wp, next4[3] = p.Hp;
    out6[5] = (int32_t)count;
    if (count > max_hits) {
        out6[0] = HOG_RD_OVERFLOW;
        return 0;
    }
    std::vector<HogHit> hits;
    for (int i = 0; i < n; i++) {
        if (hits3[3 * i] < 0 || hits3[3 * i] >= p.n) return -1;
        hits.push_back(HogHit{hits3[3 * i], hits3[3 * i + 1], hits3[3 * i + 2], 0.f});
    }
    std::vector<HogRect> rects;
    std::vector<double> ws;
    hog_hit_rects(p, hits, &rects, &ws);
    hog_group(rects, ws, threshold);
    if (rects.empty()) {
        out6[0] = HOG_RD_NOBODY;
        return 0;
    }
    size_t at = 0;
    for (size_t i = 1; i < rects.size(); i++)
        if ((long long)rects[i].w * rects[i].h > (long long)rects[at].w * rects[at].h) at = i;
    const int r[4] = {rects[at].x, rects[at].y, rects[at].w, rects[at].h};
    int nx[4];
    hog_cal_rect(r, p.Hp, p.Wp, nx);
    out6[0] = HOG_RD_FOUND;
    for (int k = 0; k < 4; k++) out6[1 + k] = r[k], next4[k] = nx[k];
    return 0;
}

}  // extern "C"

#ifdef REDETECT_SWEEP_MAIN
// Hit lists in exactly sized heap blocks -- seeded clusters of windows over a level table, shuffled, at sizes round the lane counts and at
// the budget's edges -- through hog_pick_walk at several lane counts, each held to hog_pick_ref.  A load outside a list or a store outside
// the pick's arrays is the sanitizer's finding.
int main()
{
    const int sizes[] = {0, 1, 2, 3, 63, 64, 65, 200, 1023, 1024, 1025, 4096, 4097};
    const int lanes[] = {1, 64, 1000, HOG_PICK_THREADS};
    const int frames[][3] = {{360, 640, 0}, {1080, 1920, 0}, {640, 360, 3}, {200, 264, 5}};
    long long picks = 0, bad = 0, found = 0, nobody = 0, over = 0;
    unsigned rng = 12345u;
    auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
    std::vector<uint8_t> seen((size_t)1 << 30 >> 3, 0);  // one bit per key
    std::vector<unsigned> used;
    for (const auto& fr : frames)
        for (int total : sizes)
            for (int thr = 0; thr < 3; thr++) {
                HogSpec sp;
                hog_spec(0.0, 0, 0, 0.0, 0.0, 0, 0, &sp);
                std::vector<HogPlan> pv(1);
                hog_plan(fr[2], fr[0], fr[1], sp, &pv[0]);
                const HogPlan& p = pv[0];
                const int max_hits = total == 4097 ? HOG_TRACK_MAX_HITS : (total > 64 ? HOG_TRACK_MAX_HITS : 64 + (int)(next() % 2) * 4032);
                const int n = total < max_hits ? total : max_hits;
                if (n > p.nwin / 4) continue;  // (a small frame has too few windows for a long list of distinct hits)
                int32_t* h3 = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)n + !n);
                // clusters: a centre window and neighbours a stride or two away, on the same or the next level; keys must be unique
                for (unsigned k : used) seen[k >> 3] = 0;
                used.clear();
                int filled = 0;
                while (filled < n) {
                    const int lv0 = (int)(next() % (unsigned)p.n);
                    const HogLevel& L = p.lv[lv0];
                    const int cx = (int)(next() % (unsigned)L.nwx), cy = (int)(next() % (unsigned)L.nwy), members = 1 + (int)(next() % 9);
                    for (int q = 0; q < members && filled < n; q++) {
                        int lv = lv0 + (int)(next() % 2);
                        if (lv >= p.n) lv = lv0;
                        const HogLevel& M = p.lv[lv];
                        int wx = cx + (int)(next() % 3) - 1, wy = cy + (int)(next() % 3) - 1;
                        wx = wx < 0 ? 0 : (wx >= M.nwx ? M.nwx - 1 : wx), wy = wy < 0 ? 0 : (wy >= M.nwy ? M.nwy - 1 : wy);
                        const unsigned key = hog_key(lv, wy * 8, wx * 8);
                        if (seen[key >> 3] >> (key & 7) & 1) continue;
                        seen[key >> 3] |= (uint8_t)(1 << (key & 7)), used.push_back(key);
                        h3[3 * filled] = lv, h3[3 * filled + 1] = wy * 8, h3[3 * filled + 2] = wx * 8, filled++;
                    }
                }
                int32_t want6[6], want4[4];
                if (hog_pick_ref(fr[2], fr[0], fr[1], 0.0, 0, h3, n, total, max_hits, thr, want6, want4)) bad++;
                for (int nthr : lanes)
                    for (int shuffle = 0; shuffle < 2; shuffle++) {
                        for (int i = n - 1; i > 0 && shuffle; i--) {
                            const int j = (int)(next() % (unsigned)(i + 1));
                            for (int k = 0; k < 3; k++) std::swap(h3[3 * i + k], h3[3 * j + k]);
                        }
                        int32_t got6[6], got4[4];
                        const int rc = hog_pick_walk(fr[2], fr[0], fr[1], 0.0, 0, h3, n, total, max_hits, thr, nthr, got6, got4);
                        if (rc || memcmp(got6, want6, sizeof got6) || memcmp(got4, want4, sizeof got4)) {
                            printf("redetect sweep: %dx%d code %d, %d hits, threshold %d, %d lanes: rc %d, status %d / %d\n", fr[0], fr[1], fr[2], total, thr, nthr, rc, got6[0], want6[0]);
                            bad++;
                        }
                        picks++;
                    }
                found += want6[0] == HOG_RD_FOUND, nobody += want6[0] == HOG_RD_NOBODY, over += want6[0] == HOG_RD_OVERFLOW;
                free(h3);
            }
    printf("redetect sweep: %lld picks, %lld lists found / %lld nobody / %lld overflow, %lld mismatches\n", picks, found, nobody, over, bad);
    return (bad || !picks || !found || !nobody || !over) ? 1 : 0;
}
#endif

#ifdef HOG_SWEEP_MAIN
// Layouts x orientations x sizes: every frame in an exactly sized heap block (its first pixel byte at the block's first, its last at the
// block's last) and every workspace in a block of exactly the size the level table gives -- a load outside the frame or a store outside a
// workspace is the sanitizer's finding.  Every walk is also held to a plain statement of the rule (no tiles, no lanes: the level images,
// then per block a dense loop over its pixels in the stated order).
namespace {

struct Layout { int format; long long sx, sc; int pad; const char* name; };

}  // namespace

int main()
{
    const Layout layouts[] = {{0, 3, 1, 0, "packed-3"}, {0, 3, 1, 5, "packed-3 padded"}, {1, 4, 1, 0, "packed-4 rgb"}, {0, 1, 0, 3, "planar"},
                              {0, 5, 2, 1, "generic"},  {2, 1, 0, 0, "nv12"},            {2, 1, 0, 6, "nv12 pitched"}};
    const int sizes[][2] = {{128, 64}, {129, 65}, {135, 71}, {136, 72}, {150, 90}, {127, 64}, {128, 63}};
    HogTables tab;
    hog_tables(&tab);
    std::vector<float> det(HOG_DESC + 1);
    for (int i = 0; i < HOG_DESC; i++) det[i] = (float)((i * 2654435761u >> 9) % 2001) / 1000.f - 1.f;
    det[HOG_DESC] = 0.25f;
    long long walks = 0, bad = 0, empty = 0, hits_seen = 0;
    for (const Layout& lay : layouts)
        for (const auto& hw : sizes)
            for (int o = 0; o < 8; o++) {
                // (H, W) is the ORIENTED picture; the frame is stored with the sides swapped under an odd code
                int Hp = hw[0], Wp = hw[1];
                if (lay.format == 2) Hp = (Hp + 1) & ~1, Wp = (Wp + 1) & ~1;
                const int H = (o & 1) ? Wp : Hp, W = (o & 1) ? Hp : Wp;
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
                HogSpec sp;
                hog_spec(0.0, (o & 2) ? 16 : 8, 8, (o & 4) ? 1.2 : 1.05, 0.0, 0, 0, &sp);
                std::vector<HogPlan> pv(1);
                HogPlan& p = pv[0];
                hog_plan(o, H, W, sp, &p);
                uint8_t* img = (uint8_t*)malloc((size_t)(3 * p.npix) + !p.npix);
                float* votes = (float*)malloc(sizeof(float) * (size_t)(2 * p.npix) + !p.npix);
                uint8_t* bins = (uint8_t*)malloc((size_t)p.npix + !p.npix);
                float* blocks = (float*)malloc(sizeof(float) * (size_t)(HOG_BLOCK_LEN * p.nblk) + !p.nblk);
                float* scores = (float*)malloc(sizeof(float) * (size_t)p.nwin + !p.nwin);
                int32_t rects[4 * 64], count = -1, nh = -1;
                double ws[64];
                std::vector<int32_t> h3(3 * (size_t)sp.max_hits);
                std::vector<float> hs((size_t)sp.max_hits);
                const int rc = hog_walk(blk, size, 0, uv_off, lay.format, H, W, sy, sx, sc, uvs, 0, o, 0.0, sp.stride_x, sp.stride_y, sp.scale0, 0.0, 0, 0, det.data(),
                                        HOG_DESC + 1, img, votes, bins, blocks, scores, h3.data(), hs.data(), &nh, rects, ws, 64, &count);
                if (rc) printf("hog sweep: %s %dx%d code %d: refused (%d)\n", lay.name, H, W, o, rc), bad++;
                if (!p.n) empty++;
                hits_seen += nh > 0 ? nh : 0;
                // the plain statement
                HogSrc a;
                memset(&a, 0, sizeof a);
                a.src = preview_source(lay.format == 2, lay.format == 1, blk, blk + uv_off, sy, sx, sc, uvs), a.H = H, a.W = W, a.o = o;
                long long b = 0;
                for (int n = 0; n < p.n && !rc; n++) {
                    const HogLevel& L = p.lv[n];
                    auto px = [&](int y, int x, int c) { return (int)img[3 * (L.pix0 + (long long)y * L.w + x) + c]; };
                    for (int y = 0; y < L.h; y++)
                        for (int x = 0; x < L.w; x++) {
                            int c[3];
                            hog_level_pixel(a, p.Hp, p.Wp, L, y, x, c);
                            for (int k = 0; k < 3; k++) b += c[k] != px(y, x, k);
                            const int xl = x ? x - 1 : 1, xr = x + 1 < L.w ? x + 1 : L.w - 2, yu = y ? y - 1 : 1, yd = y + 1 < L.h ? y + 1 : L.h - 2;
                            const int pl[3] = {px(y, xl, 0), px(y, xl, 1), px(y, xl, 2)}, pr[3] = {px(y, xr, 0), px(y, xr, 1), px(y, xr, 2)};
                            const int pu[3] = {px(yu, x, 0), px(yu, x, 1), px(yu, x, 2)}, pd[3] = {px(yd, x, 0), px(yd, x, 1), px(yd, x, 2)};
                            float v0, v1;
                            int h0;
                            hog_vote(tab.lut, pl, pr, pu, pd, &v0, &v1, &h0);
                            const long long at = L.pix0 + (long long)y * L.w + x;
                            b += memcmp(&v0, &votes[2 * at], 4) != 0 || memcmp(&v1, &votes[2 * at + 1], 4) != 0 || bins[at] != h0;
                        }
                    for (int by = 0; by < L.nby; by++)
                        for (int bx = 0; bx < L.nbx; bx++) {
                            float hist[HOG_BLOCK_LEN];
                            for (int k = 0; k < HOG_BLOCK_LEN; k++) {
                                float s = 0.f;
                                for (int i = 0; i < HOG_BLOCK; i++) {
                                    float r = 0.f;
                                    for (int j = 0; j < HOG_BLOCK; j++) {
                                        const long long at = L.pix0 + (long long)(by * 8 + i) * L.w + bx * 8 + j;
                                        const int h0 = bins[at], h1 = h0 == 8 ? 0 : h0 + 1, bin = k % 9;
                                        if (h0 == bin) r += tab.wt[k / 9][i * 16 + j] * votes[2 * at];
                                        else if (h1 == bin) r += tab.wt[k / 9][i * 16 + j] * votes[2 * at + 1];
                                    }
                                    s += r;
                                }
                                hist[k] = s;
                            }
                            for (int k = 0; k < HOG_BLOCK_LEN; k++) {
                                const float want = hog_l2hys(hist, k);
                                b += memcmp(&want, &blocks[(L.blk0 + (long long)by * L.nbx + bx) * HOG_BLOCK_LEN + k], 4) != 0;
                            }
                        }
                }
                if (b) printf("hog sweep: %s %dx%d code %d: %lld values differ\n", lay.name, H, W, o, b);
                bad += b;
                free(img), free(votes), free(bins), free(blocks), free(scores), free(blk);
                walks++;
            }
    printf("hog sweep: %lld walks, %lld without a level, %lld hits, %lld mismatches\n", walks, empty, hits_seen, bad);
    return (bad || !walks || !empty || empty == walks) ? 1 : 0;
}
#endif
