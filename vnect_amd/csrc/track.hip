// track.hip -- the tracking loop of run_estimator_ps.py:80-109 (runner.track) on the device: per tracked frame, the pyramid reads the
// crop the stream's state names, and a box kernel behind the joints stage shifts the 2-D joints into frame coordinates (:92-93), grows
// their bounding box into the next crop (:96-107) and builds that crop's squarify geometry (utils.img_scale_squarify), so the host never
// waits for a frame's joints to submit the next frame.  Built with -ffp-contract=off: crop.h's double / float arithmetic rounds like
// the host's (tests/test_track_cpu.py holds its host build to hostplan.h and runner.bbox_update; tests/test_gpu_track.py holds the
// device to runner.track, frame by frame, bit for bit).
#include "kernels.h"
#include "pyramid.h"
#include "crop.h"
#include "trackbox.h"

namespace vnect {

typedef float f32x4t __attribute__((ext_vector_type(4)));

// pyramid_kernel (post.hip) for a tracked frame: the same pixels, the crop taken from the stream's state -- at (x, y) of the whole frame
// in a resident slot, or (packed) the crop's own rows, 3 w bytes apart, as frame_copy_track_kernel left them
template <typename T>
__global__ void pyramid_track_kernel(const TrackState* __restrict__ ts, const FrameDyn dyn, int packed, const ScaleTabs* __restrict__ tabs,
                                     T* __restrict__ batch4)
{
    typedef T tx4 __attribute__((ext_vector_type(4)));
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, s = blockIdx.z;
    if (x >= BOX) return;
    FrameDyn d = dyn;
    if (packed) d.row_stride = 3LL * ts->w;
    else d.frame = dyn.frame + (long long)ts->y * dyn.row_stride + 3LL * ts->x;
    int v[3];
    pyramid_pixel(&ts->fp, d, tabs, s, y, x, v);
    f32x4t o = {tabs->lut[v[0]], tabs->lut[v[1]], tabs->lut[v[2]], 0.f};
    store_wt((tx4*)(batch4 + (((long long)s * BOX + y) * BOX + x) * 4), __builtin_convertvector(o, tx4));
}

hipError_t launch_pyramid_track(const TrackState* ts, FrameDyn dyn, int packed, const ScaleTabs* tabs, void* batch4, int S, int el, hipStream_t st)
{
    dim3 g((BOX + 127) / 128, BOX, S);
    with_el(el, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pyramid_track_kernel<T>, g, dim3(128), 0, st, ts, dyn, packed, tabs, (T*)batch4);
    });
    return hipGetLastError();
}

// pyramid_track_kernel for TWO tracked streams whose states lie side by side (people mode: persons 2 u and 2 u + 1 of one video), into the
// batched plan's (2 S)-image input tensor: image i is scale i % S of person i / S, cropped with ts[i / S] out of that person's frame
// argument.  Per pixel it is pyramid_track_kernel's code, so each half holds the bytes a launch of that kernel for its person writes.
template <typename T>
__global__ void pyramid_track_pair_kernel(const TrackState* __restrict__ ts2, const FrameDyn dyn0, const FrameDyn dyn1, int packed,
                                          const ScaleTabs* __restrict__ tabs, int S, T* __restrict__ batch4)
{
    typedef T tx4 __attribute__((ext_vector_type(4)));
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, i = blockIdx.z;
    if (x >= BOX) return;
    const int k = i >= S ? 1 : 0, s = i - k * S;  // (uniform over the workgroup)
    const TrackState* ts = ts2 + k;
    FrameDyn d = k ? dyn1 : dyn0;
    if (packed) d.row_stride = 3LL * ts->w;
    else d.frame = d.frame + (long long)ts->y * d.row_stride + 3LL * ts->x;
    int v[3];
    pyramid_pixel(&ts->fp, d, tabs, s, y, x, v);
    f32x4t o = {tabs->lut[v[0]], tabs->lut[v[1]], tabs->lut[v[2]], 0.f};
    store_wt((tx4*)(batch4 + (((long long)i * BOX + y) * BOX + x) * 4), __builtin_convertvector(o, tx4));
}

hipError_t launch_pyramid_track_pair(const TrackState* ts2, FrameDyn dyn0, FrameDyn dyn1, int packed, const ScaleTabs* tabs, void* batch4, int S, int el,
                                     hipStream_t st)
{
    if (S < 1 || 2 * S > VNECT_MAX_IMAGES) return hipErrorInvalidValue;
    dim3 g((BOX + 127) / 128, BOX, 2 * S);
    with_el(el, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pyramid_track_pair_kernel<T>, g, dim3(128), 0, st, ts2, dyn0, dyn1, packed, tabs, S, (T*)batch4);
    });
    return hipGetLastError();
}

// The box stage as its own launch, behind post_kernel (or joints_kernel): the joints come back from the result ring slot.  One workgroup, one
// thread per table entry.  A frame whose own crop was refused (its joints stage skipped, post_kernel's xfail test) keeps the stream
// stopped: the next frame is refused too, until vnect_track_begin.
constexpr int BOX_THREADS = 384;
// The loss rule (trackbox.h) takes the frame's confidences from DEVICE memory (conf_dev: the joints stage in front of this launch left
// them there as well as in the ring slot), requested up front with the state and the policy.
__global__ __launch_bounds__(BOX_THREADS) void track_box_kernel(TrackState* __restrict__ ts, JointsOut* out, TrackOut* tout, unsigned xseq,
                                                                const double* __restrict__ conf_dev, const TrackPolicy* __restrict__ polp,
                                                                ConfOut* cf, int* gate)
{
    __shared__ double j2[NJ * 2];
    __shared__ double cl[NJ];
    const int t = threadIdx.x;
    const TrackNow c = track_now(ts);
    const TrackPolicy pol = track_policy_now(polp);
    if (conf_dev && t < NJ) cl[t] = conf_dev[t];
    __syncthreads();  // (every thread has read the state before thread 0 overwrites it)
    if (c.status != SQ_OK) {
        track_refused(ts, c, tout, xseq, gate);
        return;
    }
    if (t < NJ * 2) {  // run_estimator_ps.py:92-93: joints_2d[:, 0] += y; joints_2d[:, 1] += x  (float64)
        const double v = out->j2d[t] + (double)((t & 1) ? c.x : c.y);
        out->j2d[t] = v;
        j2[t] = v;
    }
    __syncthreads();
    track_box_stage(ts, c, j2, tout, xseq, conf_dev ? cl : nullptr, pol, cf, gate);
}

hipError_t launch_track_box(TrackState* ts, JointsOut* out, TrackOut* tout, unsigned xseq, hipStream_t st, const double* conf_dev,
                            const TrackPolicy* pol, ConfOut* conf, int* gate)
{
    if (!conf_dev != !pol || (conf && !conf_dev)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_box_kernel, dim3(1), dim3(BOX_THREADS), 0, st, ts, out, tout, xseq, conf_dev, pol, conf, gate);
    return hipGetLastError();
}

}  // namespace vnect
