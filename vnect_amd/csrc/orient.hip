// orient.hip -- the oriented copies: a frame that is stored rotated / mirrored (a sideways camera, a decoder's surface with a rotation tag)
// -> the packed BGR crop of its oriented picture, at the destination's origin.  orient.h holds the rule and every address; here are the
// barrier and the stores.  A workgroup owns one ORIENT_T x ORIENT_T tile of the OUTPUT crop: its four waves load the tile's stored rows along the
// stored x axis as aligned dwords into LDS (wave v: rows v, v + 4, ...), and behind one barrier write the output rows, every lane one
// aligned destination dword (whole inside a tile row, byte stores at its two ends).  Orientation 0 never comes here: the copies of
// post.hip keep it.  Loads stay inside the source's allocation(s); no byte outside the crop's 3 w h is stored.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "orient.h"

namespace vnect {

template <int FORM>
__device__ __forceinline__ void orient_tile_body(const OrientSrc& s, int o, int H, int W, int x, int y, int w, int h, uint8_t* __restrict__ dst)
{
    __shared__ uint32_t lds[ORIENT_LDS_DWORDS];
    OrientTile t;
    if (!orient_tile(o, H, W, x, y, w, h, (int)blockIdx.y, (int)blockIdx.x, &t)) return;  // (uniform over the workgroup)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (orient_tile_inside(s, FORM, t)) {  // (uniform over the workgroup) the common tile: all of a wave's rows' loads in flight, then their LDS writes
        constexpr int NS = FORM == INGEST_PLANAR ? 3 : (FORM == ORIENT_NV12 ? 2 : 1), NL = 1;  // (a row has at most ORIENT_ROW_DWORDS <= 64 dwords)
        uint32_t v[ORIENT_T / 4][NS][NL];
#pragma unroll
        for (int i = 0; i < ORIENT_T / 4; i++)
#pragma unroll
            for (int k = 0; k < NS; k++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    uintptr_t a;
                    int at;
                    orient_inside_dword(s, FORM, t, k, wave + 4 * i, lane + 64 * j, &a, &at);
                    v[i][k][j] = orient_load_inside(a, at, FORM, k);
                }
#pragma unroll
        for (int i = 0; i < ORIENT_T / 4; i++)
#pragma unroll
            for (int k = 0; k < NS; k++)
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    uintptr_t a;
                    int at;
                    orient_inside_dword(s, FORM, t, k, wave + 4 * i, lane + 64 * j, &a, &at);
                    if (at >= 0) lds[at] = v[i][k][j];
                }
    } else {
        for (int rr = wave; rr < t.sh; rr += 4) orient_load_row(s, FORM, t.R0 + rr, t.C0, t.sw, lds + rr * ORIENT_PITCH, lane);
    }
    __syncthreads();
    for (int ii = wave; ii < t.th; ii += 4) {
        uintptr_t a;
        uint32_t v;
        const unsigned m = orient_out_dword(s, FORM, o, H, W, x, y, w, t, ii, lane, lds, (uintptr_t)dst, &a, &v);
        if (m == 15u) {
            *(uint32_t*)a = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (m & (1u << j)) ((uint8_t*)a)[j] = (uint8_t)(v >> (8 * j));
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(ORIENT_THREADS) void orient_copy_kernel(const OrientSrc s, int o, int H, int W, int x, int y, int w, int h, uint8_t* __restrict__ dst)
{
    orient_tile_body<FORM>(s, o, H, W, x, y, w, h, dst);
}
// the tracked form (ingest_copy_track_kernel's contract): the rect -- in oriented coordinates -- is the stream's state on the device, the grid
// covers the whole oriented frame, tiles outside the crop leave at once
template <int FORM>
__global__ __launch_bounds__(ORIENT_THREADS) void orient_copy_track_kernel(const TrackState* __restrict__ ts, const OrientSrc s, int o, int H, int W,
                                                                           uint8_t* __restrict__ dst)
{
    orient_tile_body<FORM>(s, o, H, W, ts->x, ts->y, ts->w, ts->h, dst);
}

// what the kernels rely on: the whole stored frame inside the allocation(s), strides positive, NV12 even
static bool orient_src_ok(const OrientSrc& s, int o, int H, int W)
{
    if (o < 1 || o > 7 || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return false;
    if (!s.p0 || !s.lo0 || !s.end0 || s.sy < 1 || s.sx < 1 || s.sc < 1 || (s.order != INGEST_BGR && s.order != INGEST_RGB)) return false;
    if (s.form == ORIENT_NV12) {
        if (!s.p1 || !s.lo1 || !s.end1 || ((H | W) & 1) || s.sy < W || s.sc < W || s.sx != 1) return false;
        return s.p0 >= s.lo0 && (long long)(s.end0 - s.p0) >= (long long)(H - 1) * s.sy + W && s.p1 >= s.lo1 &&
               (long long)(s.end1 - s.p1) >= (long long)(H / 2 - 1) * s.sc + W;
    }
    if (s.form < INGEST_PACKED3 || s.form > INGEST_GENERIC) return false;
    if (s.form != INGEST_GENERIC && s.form != ingest_form(s.sx, s.sc)) return false;
    return s.p0 >= s.lo0 && (long long)(s.end0 - s.p0) >= ingest_span(H, W, s.sy, s.sx, s.sc);
}
template <class F>
static void orient_dispatch(int form, F&& f)
{
    switch (form) {
    case INGEST_PACKED3: f(std::integral_constant<int, INGEST_PACKED3>{}); break;
    case INGEST_PACKED4: f(std::integral_constant<int, INGEST_PACKED4>{}); break;
    case INGEST_PLANAR: f(std::integral_constant<int, INGEST_PLANAR>{}); break;
    case INGEST_GENERIC: f(std::integral_constant<int, INGEST_GENERIC>{}); break;
    default: f(std::integral_constant<int, ORIENT_NV12>{}); break;
    }
}
hipError_t launch_orient_copy(const OrientSrc& s, int o, int H, int W, int x, int y, int w, int h, uint8_t* dst, hipStream_t st)
{
    int Ho, Wo;
    orient_size(o, H, W, &Ho, &Wo);
    if (!orient_src_ok(s, o, H, W) || !dst || x < 0 || y < 0 || w < 1 || h < 1 || (long long)x + w > Wo || (long long)y + h > Ho) return hipErrorInvalidValue;
    const dim3 g((unsigned)((w + ORIENT_T - 1) / ORIENT_T), (unsigned)((h + ORIENT_T - 1) / ORIENT_T));
    if (g.y > 65535u) return hipErrorInvalidValue;
    orient_dispatch(s.form, [&](auto fm) {
        hipLaunchKernelGGL((orient_copy_kernel<decltype(fm)::value>), g, dim3(ORIENT_THREADS), 0, st, s, o, H, W, x, y, w, h, dst);
    });
    return hipGetLastError();
}
hipError_t launch_orient_copy_track(const TrackState* ts, const OrientSrc& s, int o, int H, int W, uint8_t* dst, hipStream_t st)
{
    int Ho, Wo;
    orient_size(o, H, W, &Ho, &Wo);
    if (!orient_src_ok(s, o, H, W) || !ts || !dst) return hipErrorInvalidValue;
    const dim3 g((unsigned)((Wo + ORIENT_T - 1) / ORIENT_T), (unsigned)((Ho + ORIENT_T - 1) / ORIENT_T));
    if (g.y > 65535u) return hipErrorInvalidValue;
    orient_dispatch(s.form, [&](auto fm) {
        hipLaunchKernelGGL((orient_copy_track_kernel<decltype(fm)::value>), g, dim3(ORIENT_THREADS), 0, st, ts, s, o, H, W, dst);
    });
    return hipGetLastError();
}

}  // namespace vnect
