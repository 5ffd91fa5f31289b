// view3d.hip -- the reference's second window (run_estimator_ps.py:90, 124-126; src/utils.py:272-304, 317-330: the 3-D skeleton plot fed
// joints_3d through q_joints) rendered into DEVICE memory by the rule of view3d.h (VIEW3D.md).  One launch per picture; the grid depends
// on the picture's size only, because the tracked form (vnect_track_view3d) does not know the joints on the host.  A workgroup owns a
// 64 x 16 tile.  Wave 0 sets up one limb per lane (it projects both of the limb's joints), culls it against the tile and ranks it among
// all limbs by counting compares (view3d_over); the lane whose number is a rank then looks up that rank's limb, and a ballot compacts
// the survivors -- so `live` lists them from the lowest rank to the highest.  Then every lane tests its four adjacent pixels against the
// survivors, the last hit winning, and stores its 12 bytes as aligned dwords where they are whole and as bytes elsewhere
// (preview_store).  Every pixel of the output is written exactly once and no other byte is.
// Built with -ffp-contract=off: the projection and the inside test round like numpy's and g++'s.
#include "kernels.h"
#include "view3d.h"

namespace vnect {

// j3d / conf: 63 floats and (a.has_conf) 21 doubles in device memory; or, jo set, the tracked form -- the frame's joints_3d and status,
// and (co) its confidences, as the joints stage in front of this launch left them in the frame's result-ring slot (device-mapped pinned
// host memory): a frame whose status is not 0 (its crop was refused: it has no joints) writes nothing.
__global__ __launch_bounds__(VIEW3D_THREADS) void view3d_kernel(const View3dArgs a, const float* j3d, const double* conf, const JointsOut* jo,
                                                               const ConfOut* co, int tiles_x)
{
    __shared__ float sj[VIEW3D_NJ * 3];
    __shared__ double scf[VIEW3D_NJ];
    __shared__ View3dLimb L[VIEW3D_NJ];
    __shared__ int live[VIEW3D_NJ];
    __shared__ int nlive;
    const int tid = threadIdx.x;
    if (jo && jo->status != 0) return;  // (uniform: every lane reads the same word)
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int dy0 = tile_y * VIEW3D_TILE_H, dx0 = tile_x * VIEW3D_TILE_W;
    const int dy1 = min(dy0 + VIEW3D_TILE_H, a.rows) - 1, dx1 = min(dx0 + VIEW3D_TILE_W, a.cols) - 1;  // the tile's last pixels
    if (tid < VIEW3D_NJ * 3) sj[tid] = jo ? jo->j3d[tid] : j3d[tid];
    if (tid >= 64 && tid < 64 + VIEW3D_NJ) scf[tid - 64] = !a.has_conf ? 0.0 : (co ? co->conf[tid - 64] : conf[tid - 64]);
    __syncthreads();
    if (tid < 64) {  // wave 0
        View3dLimb l;
        l.key = 0.0, l.skip = 1;
        bool near = false;
        if (tid < VIEW3D_NJ) {
            l = view3d_limb_of(a, sj, scf, tid);
            L[tid] = l;
            near = view3d_limb_near(l, a.grow, dy0, dy1, dx0, dx1);
        }
        // this lane's limb lies over `rank` of the others; the limb whose rank is this lane's number is `mine`
        int rank = 0;
        for (int j = 0; j < VIEW3D_NJ; j++) {
            const double kj = __shfl(l.key, j);
            const int sk = __shfl(l.skip, j);
            rank += (!sk && !l.skip && j != tid && view3d_over(a.order, l.key, tid, kj, j)) ? 1 : 0;
        }
        int mine = -1;
        for (int j = 0; j < VIEW3D_NJ; j++) {
            const int rj = __shfl(rank, j), sk = __shfl(l.skip, j);
            if (!sk && rj == tid) mine = j;
        }
        const int nr = __shfl(near ? 1 : 0, mine < 0 ? 0 : mine);
        const bool keep = mine >= 0 && nr != 0;
        const unsigned long long m = __ballot(keep);
        if (keep) live[__popcll(m & ((1ull << tid) - 1ull))] = mine;
        if (tid == 0) nlive = __popcll(m);
    }
    __syncthreads();
    const int dy = dy0 + tid / VIEW3D_LANES_X, dx = dx0 + (tid % VIEW3D_LANES_X) * VIEW3D_LANE_PX;
    if (dy > dy1 || dx > dx1) return;
    view3d_lane(a, L, live, nlive, dy, dx);
}

hipError_t launch_view3d(const View3dArgs& a, const float* j3d, const double* conf, const JointsOut* jo, const ConfOut* co, hipStream_t st)
{
    if (!view3d_args_ok(a)) return hipErrorInvalidValue;
    if (!jo == !j3d || (co && !jo) || (conf && !j3d)) return hipErrorInvalidValue;
    if (a.has_conf && !(jo ? (const void*)co : (const void*)conf)) return hipErrorInvalidValue;
    const int tx = (a.cols + VIEW3D_TILE_W - 1) / VIEW3D_TILE_W, ty = (a.rows + VIEW3D_TILE_H - 1) / VIEW3D_TILE_H;
    hipLaunchKernelGGL(view3d_kernel, dim3((unsigned)(tx * ty)), dim3(VIEW3D_THREADS), 0, st, a, j3d, conf, jo, co, tx);
    return hipGetLastError();
}

}  // namespace vnect
