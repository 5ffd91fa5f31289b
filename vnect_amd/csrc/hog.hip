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
#include "kernels.h"
#include "hog.h"

namespace vnect {

// the level whose workgroups include `wg`: first workgroup indices ascend with the level (uniform: scalar loads)
#define HOG_FIND_LEVEL(field)                                 \
    int n = 0;                                                \
    for (int k = 1; k < nlev; k++)                            \
        if (lv[k].field <= (int)blockIdx.x) n = k;            \
    const HogLevel L = lv[n];

__global__ __launch_bounds__(HOG_THREADS) void hog_vote_kernel(const HogSrc a, int Hp, int Wp, int nlev, const HogLevel* __restrict__ lv,
                                                               const HogTables* __restrict__ tab, float2* __restrict__ votes, uint8_t* __restrict__ bins)
{
    HOG_FIND_LEVEL(vt0)
    const int tile = (int)blockIdx.x - L.vt0, ty = tile / L.vtx, tx = tile - ty * L.vtx;
    const int y = ty * HOG_VTILE_H + (int)threadIdx.x / HOG_VTILE_W, x = tx * HOG_VTILE_W + (int)threadIdx.x % HOG_VTILE_W;
    if (y >= L.h || x >= L.w) return;
    float v0, v1;
    int h0;
    hog_vote_at(a, Hp, Wp, L, tab->lut, y, x, &v0, &v1, &h0);
    const long long at = L.pix0 + (long long)y * L.w + x;
    votes[at] = make_float2(v0, v1);
    bins[at] = (uint8_t)h0;
}

constexpr int HOG_R_STRIDE = HOG_BLOCK + 1;  // a row-partial line in LDS, padded off the 16-float bank pattern

__global__ __launch_bounds__(HOG_THREADS) void hog_block_kernel(int nlev, const HogLevel* __restrict__ lv, const HogTables* __restrict__ tab,
                                                                const float2* __restrict__ votes, const uint8_t* __restrict__ bins, float* __restrict__ blocks)
{
    __shared__ float sv0[HOG_PER_WG][HOG_BLOCK * HOG_BLOCK], sv1[HOG_PER_WG][HOG_BLOCK * HOG_BLOCK];
    __shared__ uint8_t sh[HOG_PER_WG][HOG_BLOCK * HOG_BLOCK];
    __shared__ float R[HOG_PER_WG][HOG_BLOCK_LEN * HOG_R_STRIDE];
    __shared__ float hist[HOG_PER_WG][HOG_BLOCK_LEN];
    HOG_FIND_LEVEL(bt0)
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int b = ((int)blockIdx.x - L.bt0) * HOG_PER_WG + w;
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

constexpr int HOG_WIN_BLOCKS = HOG_WIN_BX * HOG_WIN_BY;  // 105

__global__ __launch_bounds__(HOG_THREADS) void hog_window_kernel(int nlev, const HogLevel* __restrict__ lv, int stride_x, int stride_y, const float* __restrict__ det,
                                                                 const float* __restrict__ blocks, double hit_threshold, int max_hits, HogHit* __restrict__ hits,
                                                                 unsigned* __restrict__ count, float* __restrict__ scores)
{
    __shared__ float T[HOG_PER_WG][HOG_WIN_BLOCKS];
    HOG_FIND_LEVEL(wt0)
    const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int wi = ((int)blockIdx.x - L.wt0) * HOG_PER_WG + w;
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

hipError_t launch_hog(const HogSrc& a, const HogPlan& p, const HogDev& d, double hit_threshold, int max_hits, int stages, hipStream_t st)
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
    hipError_t e = hipMemsetAsync(d.count, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return e;
    if (stages & 1) hipLaunchKernelGGL(hog_vote_kernel, dim3((unsigned)p.vtiles), dim3(HOG_THREADS), 0, st, a, Hp, Wp, p.n, d.lv, d.tab, d.votes, d.bins);
    if (stages & 2) hipLaunchKernelGGL(hog_block_kernel, dim3((unsigned)p.btiles), dim3(HOG_THREADS), 0, st, p.n, d.lv, d.tab, (const float2*)d.votes, (const uint8_t*)d.bins, d.blocks);
    if (stages & 4)
        hipLaunchKernelGGL(hog_window_kernel, dim3((unsigned)p.wtiles), dim3(HOG_THREADS), 0, st, p.n, d.lv, p.stride_x, p.stride_y, d.det, (const float*)d.blocks,
                           hit_threshold, max_hits, d.hits, d.count, d.scores);
    return hipGetLastError();
}

}  // namespace vnect
