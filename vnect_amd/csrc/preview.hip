// preview.hip -- the reference's display step (run_estimator_ps.py:94-96: draw_limbs_2d into frame.copy(), img_scale to 1024 on the
// longer side, imshow) on a frame that lies in DEVICE memory: one launch reads the frame where it lies, in any layout and under any
// orientation, applies the overlay per source tap and writes the scaled packed picture -- by the rule of preview.h (PREVIEW.md).  The
// frame itself is never written.  A workgroup owns a 64 x 16 tile of the OUTPUT; wave 0 sets the 21 limbs up and culls them (and one
// lane the band) against the rectangle of the picture the tile's taps lie in, as overlay.hip culls against its tile; then every lane
// computes four adjacent output pixels -- each tap decides band / limb / picture against the survivors and fetches the picture's bytes
// only when it needs them -- and stores its 12 bytes as aligned dwords (shared dwords as bytes: preview_store).  The taps are read straight
// from memory, not staged in LDS: a footprint of any size (f = 1/16: 1024 x 256 source pixels per tile) then costs nothing but its taps.
// Built with -ffp-contract=off: the inside test and the tap arithmetic round like numpy's and g++'s.
#include "kernels.h"
#include "crop.h"
#include "preview.h"

namespace vnect {

// jo / to / co: the tracked form -- joints in frame coordinates, rect_used and status, confidences, from the frame's result-ring slot
// (device-mapped pinned host memory) as the box stage in front of this launch left them; nullptr: everything is in `in`.
__global__ __launch_bounds__(PREVIEW_THREADS) void preview_kernel(const PreviewArgs a, const OverlayInput in, const JointsOut* jo, const TrackOut* to,
                                                                  const ConfOut* co, int tiles_x)
{
    __shared__ double sj[OVERLAY_NJ * 2];
    __shared__ double scf[OVERLAY_NJ];
    __shared__ OverlayLimb L[OVERLAY_NJ];
    __shared__ int live[OVERLAY_NJ];
    __shared__ int nlive;
    __shared__ OverlayBand band;
    const int tid = threadIdx.x;
    if (to && to->status != SQ_OK) return;  // the frame's crop was refused: it has no joints and no preview (uniform: every lane reads the same word)
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int dy0 = tile_y * PREVIEW_TILE_H, dx0 = tile_x * PREVIEW_TILE_W;
    const int dy1 = min(dy0 + PREVIEW_TILE_H, a.g.dh) - 1, dx1 = min(dx0 + PREVIEW_TILE_W, a.g.dw) - 1;  // the tile's last output pixels
    long long y0, y1, x0, x1;
    preview_footprint(a.g, dy0, dy1, dx0, dx1, &y0, &y1, &x0, &x1);
    if (tid < OVERLAY_NJ * 2) sj[tid] = jo ? jo->j2d[tid] : in.j2d[tid];
    if (tid >= 64 && tid < 64 + OVERLAY_NJ && in.has_conf) scf[tid - 64] = co ? co->conf[tid - 64] : in.conf[tid - 64];
    if (tid == 128) {
        OverlayBand b = to ? overlay_band(true, to->rect[0], to->rect[1], to->rect[2], to->rect[3])
                           : overlay_band(in.has_rect != 0, in.rect[0], in.rect[1], in.rect[2], in.rect[3]);
        if (!overlay_band_near(b, y0, y1, x0, x1)) b.on = 0;  // no tap of this tile can lie in it
        band = b;
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: one lane per limb; the survivors' indices compacted by a ballot
        bool near = false;
        if (tid < OVERLAY_NJ) {
            const OverlayLimb l = preview_limb_of(a, sj, scf, in.has_conf != 0, in.min_conf, in.parents, tid);
            L[tid] = l;
            near = overlay_limb_near(l, y0, y1, x0, x1);
        }
        const unsigned long long m = __ballot(near);
        if (near) live[__popcll(m & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) nlive = __popcll(m);
    }
    __syncthreads();
    const int dy = dy0 + tid / PREVIEW_LANES_X, dx = dx0 + (tid % PREVIEW_LANES_X) * PREVIEW_LANE_PX;
    if (dy > dy1 || dx > dx1) return;
    preview_lane(a, L, live, nlive, band, dy, dx);
}

hipError_t launch_preview(const PreviewArgs& a, const OverlayInput& in, const JointsOut* jo, const TrackOut* to, const ConfOut* co, hipStream_t st)
{
    if (!a.src.p0 || a.H < 1 || a.W < 1 || !orient_ok(a.o) || (a.src.form == ORIENT_NV12 && (!a.src.p1 || ((a.H | a.W) & 1)))) return hipErrorInvalidValue;
    int Hp, Wp;
    orient_size(a.o, a.H, a.W, &Hp, &Wp);
    if (Hp != a.g.Hp || Wp != a.g.Wp || a.g.dh < 1 || a.g.dw < 1 || a.g.dh > PREVIEW_MAX || a.g.dw > PREVIEW_MAX || !(a.g.scale > 0.0)) return hipErrorInvalidValue;
    if (a.g.copy != (a.g.dh == Hp && a.g.dw == Wp)) return hipErrorInvalidValue;
    if (!a.out || a.pitch < 3LL * a.g.dw) return hipErrorInvalidValue;
    if (!jo != !to || (co && !jo)) return hipErrorInvalidValue;
    for (int i = 0; i < OVERLAY_NJ; i++)
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return hipErrorInvalidValue;
    const int tx = (a.g.dw + PREVIEW_TILE_W - 1) / PREVIEW_TILE_W, ty = (a.g.dh + PREVIEW_TILE_H - 1) / PREVIEW_TILE_H;
    hipLaunchKernelGGL(preview_kernel, dim3((unsigned)(tx * ty)), dim3(PREVIEW_THREADS), 0, st, a, in, jo, to, co, tx);
    return hipGetLastError();
}

// The people form (preview.h: PreviewPeople): the same tile, lanes, blend and stores; wave p sets person p up -- its joints and confidences
// from that person's ring slot, its band, its limbs culled against the tile's footprint -- so four waves serve up to four persons at once.
static_assert(PREVIEW_THREADS / 64 >= PREVIEW_MAX_PEOPLE, "preview.hip: one wave per person");
__global__ __launch_bounds__(PREVIEW_THREADS) void preview_people_kernel(const PreviewArgs a, const OverlayInput in, const PreviewPeopleIn pin, int tiles_x)
{
    __shared__ double sj[PREVIEW_MAX_PEOPLE][OVERLAY_NJ * 2];
    __shared__ double scf[PREVIEW_MAX_PEOPLE][OVERLAY_NJ];
    __shared__ OverlayLimb L[PREVIEW_MAX_PEOPLE * OVERLAY_NJ];
    __shared__ int live[PREVIEW_MAX_PEOPLE * OVERLAY_NJ];
    __shared__ int nlive[PREVIEW_MAX_PEOPLE];
    __shared__ OverlayBand band[PREVIEW_MAX_PEOPLE];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int dy0 = tile_y * PREVIEW_TILE_H, dx0 = tile_x * PREVIEW_TILE_W;
    const int dy1 = min(dy0 + PREVIEW_TILE_H, a.g.dh) - 1, dx1 = min(dx0 + PREVIEW_TILE_W, a.g.dw) - 1;
    long long y0, y1, x0, x1;
    preview_footprint(a.g, dy0, dy1, dx0, dx1, &y0, &y1, &x0, &x1);
    const bool mine = w < pin.P;                                  // (uniform over the wave)
    const bool drawn = mine && pin.to[w]->status == SQ_OK;        // a refused crop has no joints: the person is left out
    if (drawn) {
        if (l < OVERLAY_NJ * 2) sj[w][l] = pin.jo[w]->j2d[l];
        else if (l < OVERLAY_NJ * 3 && in.has_conf) scf[w][l - OVERLAY_NJ * 2] = pin.co[w]->conf[l - OVERLAY_NJ * 2];
    }
    if (mine && l == 63) {
        OverlayBand b = overlay_band(drawn, drawn ? pin.to[w]->rect[0] : 0, drawn ? pin.to[w]->rect[1] : 0, drawn ? pin.to[w]->rect[2] : 0,
                                     drawn ? pin.to[w]->rect[3] : 0);
        if (!overlay_band_near(b, y0, y1, x0, x1)) b.on = 0;
        band[w] = b;
    }
    __syncthreads();
    if (mine) {
        bool near = false;
        if (drawn && l < OVERLAY_NJ) {
            const OverlayLimb lm = preview_limb_of(a, sj[w], scf[w], in.has_conf != 0, in.min_conf, in.parents, l);
            L[w * OVERLAY_NJ + l] = lm;
            near = overlay_limb_near(lm, y0, y1, x0, x1);
        }
        const unsigned long long m = __ballot(near);
        if (near) live[w * OVERLAY_NJ + __popcll(m & ((1ull << l) - 1ull))] = l;
        if (l == 0) nlive[w] = __popcll(m);
    }
    __syncthreads();
    const int dy = dy0 + tid / PREVIEW_LANES_X, dx = dx0 + (tid % PREVIEW_LANES_X) * PREVIEW_LANE_PX;
    if (dy > dy1 || dx > dx1) return;
    preview_lane_of(a, PreviewPeople{pin.P, L, live, nlive, band}, dy, dx);
}

hipError_t launch_preview_people(const PreviewArgs& a, const OverlayInput& in, const PreviewPeopleIn& pin, hipStream_t st)
{
    if (!a.src.p0 || a.H < 1 || a.W < 1 || !orient_ok(a.o) || (a.src.form == ORIENT_NV12 && (!a.src.p1 || ((a.H | a.W) & 1)))) return hipErrorInvalidValue;
    int Hp, Wp;
    orient_size(a.o, a.H, a.W, &Hp, &Wp);
    if (Hp != a.g.Hp || Wp != a.g.Wp || a.g.dh < 1 || a.g.dw < 1 || a.g.dh > PREVIEW_MAX || a.g.dw > PREVIEW_MAX || !(a.g.scale > 0.0)) return hipErrorInvalidValue;
    if (a.g.copy != (a.g.dh == Hp && a.g.dw == Wp)) return hipErrorInvalidValue;
    if (!a.out || a.pitch < 3LL * a.g.dw || !a.has_joints) return hipErrorInvalidValue;
    if (pin.P < 1 || pin.P > PREVIEW_MAX_PEOPLE) return hipErrorInvalidValue;
    for (int p = 0; p < pin.P; p++)
        if (!pin.jo[p] || !pin.to[p] || (in.has_conf && !pin.co[p])) return hipErrorInvalidValue;
    for (int i = 0; i < OVERLAY_NJ; i++)
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return hipErrorInvalidValue;
    const int tx = (a.g.dw + PREVIEW_TILE_W - 1) / PREVIEW_TILE_W, ty = (a.g.dh + PREVIEW_TILE_H - 1) / PREVIEW_TILE_H;
    hipLaunchKernelGGL(preview_people_kernel, dim3((unsigned)(tx * ty)), dim3(PREVIEW_THREADS), 0, st, a, in, pin, tx);
    return hipGetLastError();
}

}  // namespace vnect
