// overlay.hip -- the reference's second step of its frame loop (run_estimator_ps.py:92-94: utils.draw_limbs_2d, src/utils.py:222-243) on a
// frame that lies in DEVICE memory: the skeleton's limbs and the crop rectangle drawn into the caller's buffer, by the rule of overlay.h
// (OVERLAY.md).  One launch per frame; the grid depends on the frame's size only, because the tracked form (vnect_submit_tracked_device_draw)
// does not know the joints on the host: every workgroup owns a tile, sets the 20 limbs and the band up, culls them against its tile and
// leaves at once when nothing survives -- which is what all but a few tiles of a frame do.  Built with -ffp-contract=off: the inside test
// rounds like numpy's and g++'s (tests/test_gpu_overlay_kernels.py holds the device to the numpy rule byte for byte).
// A file of its own rather than a part of track.hip: the kernel shares nothing with the box stage but the three result structures it reads.
#include "kernels.h"
#include "crop.h"
#include "overlay.h"

namespace vnect {

// jo / to / co: the tracked form -- the frame's joints in frame coordinates, rect_used and status, and confidences, as the box stage in
// front of this launch left them in the frame's result-ring slot (device-mapped pinned host memory); nullptr: everything is in `in`.
__global__ __launch_bounds__(OVERLAY_THREADS) void overlay_kernel(const OverlayTarget t, const OverlayInput in, const JointsOut* jo,
                                                                  const TrackOut* to, const ConfOut* co, int tiles_x)
{
    __shared__ double sj[OVERLAY_NJ * 2];
    __shared__ double scf[OVERLAY_NJ];
    __shared__ OverlayLimb L[OVERLAY_NJ];
    __shared__ int live[OVERLAY_NJ];
    __shared__ int nlive, band_live;
    __shared__ OverlayBand band;
    const int tid = threadIdx.x;
    if (to && to->status != SQ_OK) return;  // the frame's crop was refused: it has no joints, and is not drawn (uniform: every lane reads the same word)
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int px = t.nv12 ? 2 : 1;  // pixels per cell and axis
    const int cy0 = tile_y * OVERLAY_TILE_H, cx0 = tile_x * OVERLAY_TILE_W;
    const int ncy = overlay_cells_y(t), ncx = overlay_cells_x(t);
    const int cy1 = min(cy0 + OVERLAY_TILE_H, ncy) - 1, cx1 = min(cx0 + OVERLAY_TILE_W, ncx) - 1;  // the tile's last cells
    const long long y0 = (long long)cy0 * px, y1 = (long long)cy1 * px + (px - 1), x0 = (long long)cx0 * px, x1 = (long long)cx1 * px + (px - 1);
    if (tid < OVERLAY_NJ * 2) sj[tid] = jo ? jo->j2d[tid] : in.j2d[tid];
    if (tid >= 64 && tid < 64 + OVERLAY_NJ && in.has_conf) scf[tid - 64] = co ? co->conf[tid - 64] : in.conf[tid - 64];
    if (tid == 128) {
        const bool on = to ? true : in.has_rect != 0;
        const OverlayBand b = to ? overlay_band(on, to->rect[0], to->rect[1], to->rect[2], to->rect[3])
                                 : overlay_band(on, in.rect[0], in.rect[1], in.rect[2], in.rect[3]);
        band = b;
        band_live = overlay_band_near(b, y0, y1, x0, x1) ? 1 : 0;
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: one lane per limb; the survivors' indices compacted by a ballot
        bool near = false;
        if (tid < OVERLAY_NJ) {
            const OverlayLimb l = overlay_limb_of(sj, scf, in.has_conf != 0, in.min_conf, in.parents, tid);
            L[tid] = l;
            near = overlay_limb_near(l, y0, y1, x0, x1);
        }
        const unsigned long long m = __ballot(near);
        if (near) live[__popcll(m & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) nlive = __popcll(m);
    }
    __syncthreads();
    const int n = nlive;
    if (n == 0 && !band_live) return;
    const int cx = cx0 + tid % OVERLAY_TILE_W, cy = cy0 + tid / OVERLAY_TILE_W;
    if (cx > cx1 || cy > cy1) return;
    overlay_lane(t, L, live, n, band, cx, cy, cy1);
}

hipError_t launch_overlay(const OverlayTarget& t, const OverlayInput& in, const JointsOut* jo, const TrackOut* to, const ConfOut* co, hipStream_t st)
{
    if (!t.data || t.H < 1 || t.W < 1 || (t.nv12 && (!t.uv || ((t.H | t.W) & 1)))) return hipErrorInvalidValue;
    if (!jo != !to || (co && !jo)) return hipErrorInvalidValue;
    for (int i = 0; i < OVERLAY_NJ; i++)
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return hipErrorInvalidValue;
    const long long tx = (overlay_cells_x(t) + OVERLAY_TILE_W - 1) / OVERLAY_TILE_W, ty = (overlay_cells_y(t) + OVERLAY_TILE_H - 1) / OVERLAY_TILE_H;
    if (tx * ty > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)(tx * ty)), dim3(OVERLAY_THREADS), 0, st, t, in, jo, to, co, (int)tx);
    return hipGetLastError();
}

}  // namespace vnect
