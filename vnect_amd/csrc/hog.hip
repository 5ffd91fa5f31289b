// hog.hip -- the reference's first step (src/hog_box.py:24-33: cv2.HOGDescriptor().detectMultiScale(img) with the default people
// detector) on a frame that lies in DEVICE memory, by the rule of hog.h (HOG.md).  Three launches, each covering ALL levels of the
// pyramid: a workgroup finds its level in the level table by its index.
//   hog_vote_kernel    a workgroup owns 64 x 4 pixels of a level; a lane computes its pixel's four neighbours of the level image (cv2's
//                      8-bit INTER_LINEAR of the picture, read where the frame lies, in any layout and orientation -- the level images are
//                      never stored) and from them the pixel's two votes and its bin
//   hog_block_kernel   a wave owns one 16 x 16 block: its votes go to LDS, lane (cell, row) sums its row's nine bins in column order, 36
//                      lanes sum the rows in row order and normalise (L2-Hys); every block is computed once for all windows over it
//   hog_window_kernel  a wave owns one window: lanes take the 105 blocks' shares of the score, one lane sums them in the fixed order and
//                      appends a hit behind an integer counter -- never past max_hits
// No float atomics anywhere: every sum has the one order hog.h writes down.  Built with -ffp-contract=off.
// Each kernel's body is a device function of the WORKGROUP INDEX.  The three kernels above call it with blockIdx.x.  Their gated forms
// (re-detection inside the tracked loop, vnect_track_redetect; hog.h: THE RULE) return at once unless the stream's gate word is 1 and
// otherwise walk the same workgroup indices in a grid-stride loop over a capped grid; hog_pick_kernel behind them turns the hits into the
// stream's next crop.
#include "kernels.h"
#include "hog.h"
#include "trackbox.h"

namespace vnect {

// the level whose workgroups include `wg`: first workgroup indices ascend with the level (uniform: scalar loads)
#define HOG_FIND_LEVEL(field)                                 \
    int n = 0;                                                \
    for (int k = 1; k < nlev; k++)                            \
        if (lv[k].field <= wg) n = k;                         \
    const HogLevel L = lv[n];

__device__ __forceinline__ void hog_vote_body(int wg, const HogSrc& a, int Hp, int Wp, int nlev, const HogLevel* __restrict__ lv,
                                              const HogTables* __restrict__ tab, float2* __restrict__ votes, uint8_t* __restrict__ bins)
{
    HOG_FIND_LEVEL(vt0)
    const int tile = wg - L.vt0, ty = tile / L.vtx, tx = tile - ty * L.vtx;
    const int y = ty * HOG_VTILE_H + (int)threadIdx.x / HOG_VTILE_W, x = tx * HOG_VTILE_W + (int)threadIdx.x % HOG_VTILE_W;
    if (y >= L.h || x >= L.w) return;
    float v0, v1;
    int h0;
    hog_vote_at(a, Hp, Wp, L, tab->lut, y, x, &v0, &v1, &h0);
    const long long at = L.pix0 + (long long)y * L.w + x;
    votes[at] = make_float2(v0, v1);
    bins[at] = (uint8_t)h0;
}
__global__ __launch_bounds__(HOG_THREADS) void hog_vote_kernel(const HogSrc a, int Hp, int Wp, int nlev, const HogLevel* __restrict__ lv,
                                                               const HogTables* __restrict__ tab, float2* __restrict__ votes, uint8_t* __restrict__ bins)
{
    hog_vote_body((int)blockIdx.x, a, Hp, Wp, nlev, lv, tab, votes, bins);
}
// (every lane of a workgroup reads the same word: the exit and the loop's trip count are uniform)
__global__ __launch_bounds__(HOG_THREADS) void hog_vote_gated_kernel(const int* __restrict__ gate, int total, const HogSrc a, int Hp, int Wp, int nlev,
                                                                     const HogLevel* __restrict__ lv, const HogTables* __restrict__ tab, float2* __restrict__ votes,
                                                                     uint8_t* __restrict__ bins)
{
    if (*gate == 0) return;
    for (int wg = (int)blockIdx.x; wg < total; wg += (int)gridDim.x) hog_vote_body(wg, a, Hp, Wp, nlev, lv, tab, votes, bins);
}

constexpr int HOG_R_STRIDE = HOG_BLOCK + 1;  // a row-partial line in LDS, padded off the 16-float bank pattern

// (the barriers are uniform per workgroup: `wg`, and with it the level, is the same in every lane, and no lane leaves before the last)
__device__ __forceinline__ void hog_block_body(int wg, int nlev, const HogLevel* __restrict__ lv, const HogTables* __restrict__ tab,
                                               const float2* __restrict__ votes, const uint8_t* __restrict__ bins, float* __restrict__ blocks)
{
    __shared__ float sv0[HOG_PER_WG][HOG_BLOCK * HOG_BLOCK], sv1[HOG_PER_WG][HOG_BLOCK * HOG_BLOCK];
    __shared__ uint8_t sh[HOG_PER_WG][HOG_BLOCK * HOG_BLOCK];
    __shared__ float R[HOG_PER_WG][HOG_BLOCK_LEN * HOG_R_STRIDE];
    __shared__ float hist[HOG_PER_WG][HOG_BLOCK_LEN];
    HOG_FIND_LEVEL(bt0)
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int b = (wg - L.bt0) * HOG_PER_WG + w;
    const bool valid = b < L.nbx * L.nby;  // (wave-uniform; no lane leaves before the last barrier)
    const int by = valid ? b / L.nbx : 0, bx = valid ? b - by * L.nbx : 0;
    if (valid) {
        const int i = lane >> 2, j0 = (lane & 3) * 4;
        const long long at = L.pix0 + (long long)(by * HOG_CELL + i) * L.w + bx * HOG_CELL + j0;
        for (int q = 0; q < 4; q++) {
            const float2 v = votes[at + q];
            sv0[w][i * HOG_BLOCK + j0 + q] = v.x, sv1[w][i * HOG_BLOCK + j0 + q] = v.y, sh[w][i * HOG_BLOCK + j0 + q] = bins[at + q];
        }
    }
    __syncthreads();
    if (valid) {
        const int c = lane >> 4, i = lane & 15;
        float acc[HOG_NBINS];
        hog_row_partial(&tab->wt[c][i * HOG_BLOCK], &sv0[w][i * HOG_BLOCK], &sv1[w][i * HOG_BLOCK], &sh[w][i * HOG_BLOCK], acc);
#pragma unroll
        for (int q = 0; q < HOG_NBINS; q++) R[w][(c * HOG_NBINS + q) * HOG_R_STRIDE + i] = acc[q];
    }
    __syncthreads();
    if (valid && lane < HOG_BLOCK_LEN) hist[w][lane] = hog_hist_sum(&R[w][lane * HOG_R_STRIDE]);
    __syncthreads();
    if (valid && lane < HOG_BLOCK_LEN) blocks[(L.blk0 + b) * HOG_BLOCK_LEN + lane] = hog_l2hys(hist[w], lane);
}
__global__ __launch_bounds__(HOG_THREADS) void hog_block_kernel(int nlev, const HogLevel* __restrict__ lv, const HogTables* __restrict__ tab,
                                                                const float2* __restrict__ votes, const uint8_t* __restrict__ bins, float* __restrict__ blocks)
{
    hog_block_body((int)blockIdx.x, nlev, lv, tab, votes, bins, blocks);
}
__global__ __launch_bounds__(HOG_THREADS) void hog_block_gated_kernel(const int* __restrict__ gate, int total, int nlev, const HogLevel* __restrict__ lv,
                                                                      const HogTables* __restrict__ tab, const float2* __restrict__ votes,
                                                                      const uint8_t* __restrict__ bins, float* __restrict__ blocks)
{
    if (*gate == 0) return;
    for (int wg = (int)blockIdx.x; wg < total; wg += (int)gridDim.x) {
        hog_block_body(wg, nlev, lv, tab, votes, bins, blocks);
        __syncthreads();  // (a wave uses its own quarter of the LDS only; the barrier keeps the rounds apart all the same)
    }
}

constexpr int HOG_WIN_BLOCKS = HOG_WIN_BX * HOG_WIN_BY;  // 105

__device__ __forceinline__ void hog_window_body(int wg, int nlev, const HogLevel* __restrict__ lv, int stride_x, int stride_y, const float* __restrict__ det,
                                                const float* __restrict__ blocks, double hit_threshold, int max_hits, HogHit* __restrict__ hits,
                                                unsigned* __restrict__ count, float* __restrict__ scores)
{
    __shared__ float T[HOG_PER_WG][HOG_WIN_BLOCKS];
    HOG_FIND_LEVEL(wt0)
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int wi = (wg - L.wt0) * HOG_PER_WG + w;
    const bool valid = wi < L.nwx * L.nwy;
    const int wy = valid ? wi / L.nwx : 0, wx = valid ? wi - wy * L.nwx : 0;
    const int x = wx * stride_x, y = wy * stride_y;
    if (valid)
        for (int t = lane; t < HOG_WIN_BLOCKS; t += 64) {
            const int bx = t / HOG_WIN_BY, by = t - bx * HOG_WIN_BY;
            const long long blk = L.blk0 + (long long)(y / HOG_CELL + by) * L.nbx + (x / HOG_CELL + bx);
            T[w][t] = hog_block_dot(det + t * HOG_BLOCK_LEN, blocks + blk * HOG_BLOCK_LEN);
        }
    __syncthreads();
    if (valid && lane == 0) {
        const float s = hog_score(T[w], det[HOG_DESC]);
        if (scores) scores[L.win0 + wi] = s;
        if ((double)s >= hit_threshold) {
            const unsigned at = atomicAdd(count, 1u);  // the counter ends as the full number of hits; only the first max_hits are stored
            if (at < (unsigned)max_hits) hits[at] = HogHit{n, y, x, s};
        }
    }
}
__global__ __launch_bounds__(HOG_THREADS) void hog_window_kernel(int nlev, const HogLevel* __restrict__ lv, int stride_x, int stride_y, const float* __restrict__ det,
                                                                 const float* __restrict__ blocks, double hit_threshold, int max_hits, HogHit* __restrict__ hits,
                                                                 unsigned* __restrict__ count, float* __restrict__ scores)
{
    hog_window_body((int)blockIdx.x, nlev, lv, stride_x, stride_y, det, blocks, hit_threshold, max_hits, hits, count, scores);
}
__global__ __launch_bounds__(HOG_THREADS) void hog_window_gated_kernel(const int* __restrict__ gate, int total, int nlev, const HogLevel* __restrict__ lv, int stride_x,
                                                                       int stride_y, const float* __restrict__ det, const float* __restrict__ blocks,
                                                                       double hit_threshold, int max_hits, HogHit* __restrict__ hits, unsigned* __restrict__ count,
                                                                       float* __restrict__ scores)
{
    if (*gate == 0) return;
    for (int wg = (int)blockIdx.x; wg < total; wg += (int)gridDim.x) {
        hog_window_body(wg, nlev, lv, stride_x, stride_y, det, blocks, hit_threshold, max_hits, hits, count, scores);
        __syncthreads();
    }
}

// The hits of a lost frame -> the stream's next crop (hog.h: THE RULE and the phases hog_pick_*; g++ walks the same phases in hog_capi.cpp).
// One workgroup.  Gate 0: the frame's status word and nothing else.
__global__ __launch_bounds__(HOG_PICK_THREADS) void hog_pick_kernel(const int* __restrict__ gate, const HogLevel* __restrict__ lv, const HogHit* __restrict__ hits,
                                                                    const unsigned* __restrict__ count, int max_hits, int threshold, int* cls, TrackState* ts,
                                                                    unsigned xseq, RedetectOut* out)
{
    __shared__ unsigned a[HOG_TRACK_MAX_HITS], b[HOG_TRACK_MAX_HITS];
    __shared__ int c[HOG_TRACK_MAX_HITS];
    __shared__ unsigned long long best;
    __shared__ int next[4];
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    if (*gate == 0) {  // (uniform)
        if (tid == 0) out->status = HOG_RD_NOT_RUN;
        return;
    }
    const unsigned found = *count;
    const int H = ts->H, W = ts->W;
    HogPick m{a, b, c, cls, lv, &best, 0, 1, threshold};
    m.n = found > (unsigned)max_hits ? 0 : (int)found;  // (overflow: the whole frame, nothing to group)
    while (m.np2 < m.n) m.np2 <<= 1;
    hog_pick_load(m, hits, tid, nthr);
    __syncthreads();
    for (int k = 2; k <= m.np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            hog_pick_sort_step(m, k, j, tid, nthr);
            __syncthreads();
        }
    hog_pick_init(m, tid, nthr);
    __syncthreads();
    hog_pick_union(m, tid, nthr);
    __syncthreads();
    hog_pick_flatten(m, tid, nthr);
    __syncthreads();
    hog_pick_sums(m, tid, nthr);
    __syncthreads();
    hog_pick_means(m, tid, nthr);
    __syncthreads();
    hog_pick_best(m, tid, nthr);
    __syncthreads();
    if (tid == 0) hog_pick_result(m, found, max_hits, H, W, out, next);
    __syncthreads();
    track_box_commit(ts, next, xseq);
}

// gate == nullptr: the plain kernels; else their gated forms on grids of at most `cap` workgroups (cap 0: the plain kernels' grids)
static hipError_t launch_hog_any(const HogSrc& a, const HogPlan& p, const HogDev& d, double hit_threshold, int max_hits, int stages, const int* gate, int cap,
                                 hipStream_t st)
{
    if (!a.src.p0 || a.H < 1 || a.W < 1 || !orient_ok(a.o) || (a.src.form == ORIENT_NV12 && (!a.src.p1 || ((a.H | a.W) & 1)))) return hipErrorInvalidValue;
    int Hp, Wp;
    orient_size(a.o, a.H, a.W, &Hp, &Wp);
    if (Hp != p.Hp || Wp != p.Wp || Hp > HOG_MAX_SIDE || Wp > HOG_MAX_SIDE || p.n < 1 || p.n > HOG_MAX_LEVELS) return hipErrorInvalidValue;
    if (p.stride_x < 8 || p.stride_y < 8 || p.stride_x % 8 || p.stride_y % 8 || max_hits < 1 || !(hit_threshold == hit_threshold)) return hipErrorInvalidValue;
    if (!d.lv || !d.tab || !d.det || !d.votes || !d.bins || !d.blocks || !d.hits || !d.count) return hipErrorInvalidValue;
    for (int n = 0; n < p.n; n++) {  // the table the workspace was sized from: every level inside the picture and at least one window
        const HogLevel& L = p.lv[n];
        if (L.w < HOG_WIN_W || L.h < HOG_WIN_H || L.w > Wp || L.h > Hp || L.nbx != L.w / HOG_CELL - 1 || L.nby != L.h / HOG_CELL - 1) return hipErrorInvalidValue;
        if (L.nwx != (L.w - HOG_WIN_W) / p.stride_x + 1 || L.nwy != (L.h - HOG_WIN_H) / p.stride_y + 1 || L.copy != (L.w == Wp && L.h == Hp)) return hipErrorInvalidValue;
    }
    if (!gate) {  // (the gated launches leave the counter to their caller: at gate 0 they touch nothing)
        const hipError_t e = hipMemsetAsync(d.count, 0, sizeof(unsigned), st);
        if (e != hipSuccess) return e;
    }
    if (gate) {
        auto grid = [cap](int total) { return dim3((unsigned)(cap > 0 && cap < total ? cap : total)); };
        if (stages & 1)
            hipLaunchKernelGGL(hog_vote_gated_kernel, grid(p.vtiles), dim3(HOG_THREADS), 0, st, gate, p.vtiles, a, Hp, Wp, p.n, d.lv, d.tab, d.votes, d.bins);
        if (stages & 2)
            hipLaunchKernelGGL(hog_block_gated_kernel, grid(p.btiles), dim3(HOG_THREADS), 0, st, gate, p.btiles, p.n, d.lv, d.tab, (const float2*)d.votes,
                               (const uint8_t*)d.bins, d.blocks);
        if (stages & 4)
            hipLaunchKernelGGL(hog_window_gated_kernel, grid(p.wtiles), dim3(HOG_THREADS), 0, st, gate, p.wtiles, p.n, d.lv, p.stride_x, p.stride_y, d.det,
                               (const float*)d.blocks, hit_threshold, max_hits, d.hits, d.count, d.scores);
        return hipGetLastError();
    }
    if (stages & 1) hipLaunchKernelGGL(hog_vote_kernel, dim3((unsigned)p.vtiles), dim3(HOG_THREADS), 0, st, a, Hp, Wp, p.n, d.lv, d.tab, d.votes, d.bins);
    if (stages & 2) hipLaunchKernelGGL(hog_block_kernel, dim3((unsigned)p.btiles), dim3(HOG_THREADS), 0, st, p.n, d.lv, d.tab, (const float2*)d.votes, (const uint8_t*)d.bins, d.blocks);
    if (stages & 4)
        hipLaunchKernelGGL(hog_window_kernel, dim3((unsigned)p.wtiles), dim3(HOG_THREADS), 0, st, p.n, d.lv, p.stride_x, p.stride_y, d.det, (const float*)d.blocks,
                           hit_threshold, max_hits, d.hits, d.count, d.scores);
    return hipGetLastError();
}

hipError_t launch_hog(const HogSrc& a, const HogPlan& p, const HogDev& d, double hit_threshold, int max_hits, int stages, hipStream_t st)
{
    return launch_hog_any(a, p, d, hit_threshold, max_hits, stages, nullptr, 0, st);
}

hipError_t launch_hog_gated(const HogSrc& a, const HogPlan& p, const HogDev& d, double hit_threshold, int max_hits, int stages, const int* gate, int cap,
                            hipStream_t st)
{
    if (!gate || cap < 0) return hipErrorInvalidValue;
    return launch_hog_any(a, p, d, hit_threshold, max_hits, stages, gate, cap, st);
}

hipError_t launch_hog_pick(const HogDev& d, int nlev, int max_hits, int threshold, const int* gate, int* cls, TrackState* ts, unsigned xseq, RedetectOut* out,
                           hipStream_t st)
{
    if (!gate || !cls || !ts || !out || !d.hits || !d.count || !d.lv || nlev < 0 || nlev > HOG_MAX_LEVELS || max_hits < 1 || max_hits > HOG_TRACK_MAX_HITS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hog_pick_kernel, dim3(1), dim3(HOG_PICK_THREADS), 0, st, gate, d.lv, (const HogHit*)d.hits, (const unsigned*)d.count, max_hits, threshold, cls,
                       ts, xseq, out);
    return hipGetLastError();
}

}  // namespace vnect
