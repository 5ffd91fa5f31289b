// runtime.h -- internal header of the host runtime of libvnect_hip.so (not part of the ABI: include/vnect_abi.h is).
// The runtime is eight translation units along its seams:
//   rt_plan.cpp    weights -> packed device layouts, the launch plan (layers, tiles, fused forms), the activation arena, the resize tables,
//                  the further plans built from lane 0's (lanes, batched plans)
//   rt_exec.cpp    running frames: launch sequences, hipGraph, lanes, streams, the enqueue stages and the three submits built from them
//                  (frame, batch, pair) with people mode on top, collect, device tracking's begin, warm start, roctx ranges
//   rt_ingest.cpp  frames into slots: one resolver per source (host BGR, host NV12, device memory, a pinned buffer by index) that validates
//                  the caller's frame into a FrameSrc, the pinned staging buffers, and ingest(), the one way from a FrameSrc into a slot
//   rt_draw.cpp    frames out: the overlay drawn into a caller's device frame (overlay.h), on its own or as the tail of a tracked frame;
//                  the preview (preview.h)
//   rt_hog.cpp     the person detector (hog.h): the synchronous detection calls and re-detection inside the tracked loop
//   rt_view.cpp    the 3-D view (view3d.h): one picture of given joints, and a tracked stream's setting
//   rt_comm.cpp    the pyramid exchange: RCCL (dlopen'ed) and peer writes, vnect_comm_*
//   rt_abi.cpp     the extern "C" entry points of include/vnect_abi.h (argument checks, device selection, the no-exception guard)
#pragma once
#include <dlfcn.h>
#include <link.h>
#include <unistd.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <stddef.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vnect_abi.h"
#include "crop.h"
#include "hostplan.h"
#include "ingest.h"
#include "kernels.h"
#include "orient.h"
#include "overlay.h"
#include "preview.h"
#include "view3d.h"
#include "hog.h"

namespace vnect {
namespace rt {

struct HostArray {
    std::vector<float> d;
    std::vector<int64_t> shape;
};

struct Tensor {
    std::string name;
    int S = 0, H = 0, W = 0, C = 0, Cs = 0;  // C valid channels, Cs elements per pixel
    int esz = 4;                             // bytes per element: 4 (fp32) or 2 (bf16)
    float* d = nullptr;                      // device buffer (bf16 data when esz == 2)
    size_t elems() const { return (size_t)S * H * W * Cs; }
    size_t bytes() const { return elems() * esz; }
};

enum OpKind { OP_CONV, OP_POOL, OP_BONE };

struct Layer {
    OpKind op = OP_CONV;
    std::string name;
    int in = -1, resid = -1, out = -1, out2 = -1;
    int out3 = -1;  // the chain GEMM's output tensor (the next block's branch2a), or -1
    int out_col0 = 0;  // first channel of `out` this launch writes (a paired launch whose head columns run as a launch of their own)
    ConvArgs a{};
    ReduceArgs r{};
    int BM = 64, BN = 64, KG = 1;  // tile shape; KG = in-workgroup K groups (conv.hip)
    int dy[MAX_TAPS] = {}, dx[MAX_TAPS] = {};  // filter taps [phase*ntaps + tap] (host side; the kernel gets them packed)
    float *w = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr;
    float* frag_w = nullptr;  // a 1x1 pair on 64 input channels: the same weights in MFMA fragment order, for the stem's PAIR form
    int Nreal = 0, Kreal = 0;
    double flops = 0;
    float last_ms = 0;
};

constexpr int RING = 8;  // result ring entries: up to three lanes of two-frame batches (vnect_submit_streams) in flight
constexpr int MAX_LANES = 3;

// What one lane runs: the launch plan (layers over this plan's activation buffers), its stream and graph, and the per-launch scratch.
// Lane 0's plan is the handle itself (vnect_handle derives from Plan).  More lanes (cfg.lanes == 2, 3): a frame submitted while others are
// in flight runs on another plan over the same layers and weights -- its own stream, activation arena, split-K workspace, arg-max scratch,
// geometry block and graph.  A batched plan (vnect_set_stream_batch) is the same with M doubled, on its lane's stream.  Everything shared --
// config, tables, merge geometry, resident frames, the result ring, the filter banks (their users are chained by events) -- is read
// through `owner`, where errors go too.
struct Plan {
    vnect_handle* owner = nullptr;
    hipStream_t st = nullptr;
    bool owns_stream = false;  // (a batched plan runs on its lane's)
    int S = 0;      // scales of the pyramid (merge, tables)
    int Snet = 0;   // images this plan pushes through the conv stack: S, 1 when pyramid-sharded, 2 S for a batched plan
    bool bf16 = false;  // VNECT_BF16: bf16 activations + weights, fp32 accumulate; final maps and post-processing stay fp32/f64
                        // (VNECT_FP16 too: this flag means "16-bit elements" -- the plan, layouts and fused forms key on it alone)
    bool f16 = false;   // VNECT_FP16: the 16-bit elements are fp16 (IEEE binary16) instead of bf16; everything else is the bf16 handle's
    int el() const { return bf16 ? (f16 ? EL_F16 : EL_BF16) : EL_F32; }  // the element format the kernel launchers take
    std::vector<Tensor> tensors;
    std::vector<Layer> layers;
    std::map<std::string, int> tensor_by_name;
    int t_input4 = -1, t_out = -1;
    // The stem as one launch (stem.hip): conv1 + pool1 [+ gen_input_batch].  0: off (the stand-alone layers), 1: from the batch
    // tensor (behind pyramid_kernel; also what vnect_forward uses), 2: from the frame (no pyramid launch, no batch tensor).
    int stem_mode = 0;
    bool stem_pair = false;  // the stem launch also runs res2a_branch2a + res2a_branch1 (stem.hip, PAIR): layer l_pool1 + 1 is skipped
    bool stem_frame_ok = false;  // every tile's rectangle of frame bytes fits the kernel's LDS scratch at the current scales
    bool two_frames = false;     // a batched plan: images 0 .. S-1 come from one stream's frame, S .. 2 S-1 from another's (d_fp2; StemArgs::per_stream)
    int l_conv1 = -1, l_pool1 = -1;  // the two layers a stem launch stands for
    StemArgs stem{};
    bool keep_activations = false;  // one private buffer per layer output (vnect_read_activation needs it); false = arena.  Lane 0's is the
                                    // config's; every other plan's is false (a batched plan has an arena on a keep_activations handle too)
    bool keep_fused = false;        // keep_activations with VNECT_KEEP_FUSED=1: private buffers, but the fused launches of an arena plan
    bool private_only() const { return keep_activations && !keep_fused; }  // the plan must store every layer's output: no fused forms
    float* ws = nullptr;            // the split-K slabs of the largest K-split launch
    std::vector<void*> dev_allocs;
    FrameParams* d_fp = nullptr;   // crop geometry on the device; re-uploaded only when it differs from fp_dev
    FrameParams* h_fp[RING] = {};  // pinned staging for those uploads
    FrameParams fp_dev{};          // what d_fp holds
    bool fp_dev_valid = false;
    int fp_ring = 0;
    FrameParams* d_fp2 = nullptr;  // two_frames: the second stream's geometry
    FrameParams fp_dev2{};
    bool fp_dev2_valid = false;
    ArgPartial* d_part = nullptr;
    unsigned* d_ticket = nullptr;  // post_kernel's arrival counter (zero between launches)
    bool post_merged = true;       // merge + arg-max + joints as ONE launch (post_kernel); false: two launches (VNECT_NO_POST_MERGE=1)
    long long lane_seq = -1;       // sequence number of the last frame submitted on this lane
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    bool prof_graph = false;      // build_graph also captures the profiling graph (lane 0: profiled frames always run there)
    hipGraph_t pgraph = nullptr;  // profiling twin: same launches, every conv kernel stamps its start/end
    hipGraphExec_t pgexec = nullptr;
    unsigned long long* d_prof = nullptr;       // [layer][2] device stamps (100 MHz)
    unsigned long long* h_prof = nullptr;       // pinned read-back
    unsigned long long* d_prof_end = nullptr;   // [128 layers][PROF_WGS] per-workgroup end stamps of the profiling twin
    unsigned long long* h_prof_end = nullptr;   // pinned read-back
    double conv_flops = 0;
    int conv_launches = 0;
};

// a stream's filter timestamps as the host holds them (check_time / commit_time; the device has them in d_fb[stream])
struct TimeState { bool have2 = false, have3 = false; double last2 = 0, last3 = 0; };

// What a frame puts into its entry of the result ring: assigned whole when the frame is committed (rt_exec.cpp: commit_result)
struct FrameInfo {
    int stream = 0;
    unsigned long long unit = 0;  // the in-flight limit counts UNITS (a frame, or a batch of two streams' frames): this entry's
    bool batch = false;           // the entry is a frame of a batch (the handle's own profiling figures skip it)
    Plan* prof = nullptr;         // a profiled batch's plan, on the ring entry of its last frame (collect reads its layer times)
    bool tracked = false;
    int pv_h = 0, pv_w = 0;        // a tracked frame that carries a preview (vnect_submit_tracked_device_preview): its size; 0: none
    int v3_h = 0, v3_w = 0;        // a tracked frame that carries a 3-D view (vnect_track_view3d): its size; 0: none
    bool redetect = false;         // a tracked frame of a re-detecting stream (vnect_track_redetect): its ring slot's RedetectOut is its verdict
    TimeState before{};  // a tracked frame's stream timestamps before it was committed (a refused crop rolls them back)
};

// One entry of the result ring: what the slot owns for the handle's life, and the frame in flight there
struct InFlight {
    JointsOut* out = nullptr;      // pinned, device-mapped: joints_kernel writes a frame's results straight into its ring slot
    JointsOut* out_dev = nullptr;  // the same slot as the device addresses it
    hipEvent_t done = nullptr;
    FrameInfo f;
};

// A picture per result-ring slot (a tracked frame's preview, its 3-D view): a device buffer the kernel writes and a pinned host buffer its
// copy lands in, all `cap` bytes, re-sized only while nothing is in flight (ring_pictures_size); and the picture of the frame
// vnect_collect_tracked delivered last
struct RingPictures {
    uint8_t* dev[RING] = {};
    uint8_t* host[RING] = {};
    size_t cap = 0;
    int last_ring = -1, last_h = 0, last_w = 0;
    void deliver(int ring, int h, int w) { last_ring = ring, last_h = h, last_w = w; }  // (-1, 0, 0): the frame delivered last has none
    void result(const uint8_t** data, int32_t hw[2], int64_t* pitch) const  // vnect_result_preview, vnect_result_view3d
    {
        hw[0] = last_h, hw[1] = last_w;
        *data = last_ring >= 0 ? host[last_ring] : nullptr;
        *pitch = 3LL * last_w;
    }
};

// A video stream (vnect_submit_stream; stream 0 is what every other entry point uses): d_fb[stream] and d_track[stream] on the device, and here
// the host's copy of the last timestamps, the sequence number of the stream's last frame and the lane it ran on.  Tracking (vnect_track_begin;
// track.hip): the frame size, the number the next tracked frame gets (FrameDyn::xseq against TrackState::fail), and whether a refused
// crop has stopped the stream.
struct Stream {
    TimeState t;
    long long seq = -1;
    Plan* lane = nullptr;
    bool track_on = false, track_stopped = false;
    int track_H = 0, track_W = 0;  // the ORIENTED frame's size
    int orient = 0;                // the orientation in force at vnect_track_begin: every tracked submit of the stream uses it
    unsigned track_seq = 0;
    uint8_t* track_buf = nullptr;  // the stream's crop copied out of a pinned buffer (one suffices: the next frame's copy
    size_t track_cap = 0;          // waits for this frame's box kernel, which runs after everything that reads the crop)
    bool v3_on = false;            // vnect_track_view3d: every tracked submit of the stream also renders its frame's 3-D view
    View3dArgs v3{};               // ... with these arguments (but `out` and `pitch`, which are the ring slot's)
    TrackPolicy policy{0.0, 1, TRACK_LOST_OFF};  // the host's copy of d_policy[stream] (vnect_track_policy; survives vnect_track_begin)
    // re-detection inside the loop (vnect_track_redetect; rt_hog.cpp; hog.h: THE RULE): the setting, its spec, and -- built when the setting
    // and the stream's frame size and orientation are both known, in vnect_track_redetect or vnect_track_begin -- the level table and a
    // workspace of the stream's OWN (the synchronous vnect_hog_detect* calls keep using the handle's on the upload stream)
    bool rd_on = false;
    HogSpec rd_spec{};
    int rd_cap = HOG_GATED_CAP;    // workgroups of a gated launch at most (VNECT_REDETECT_CAP, read when the setting is made; 0: full grids)
    std::vector<HogPlan> rd_plan;  // one entry once built, for (rd_o, rd_H, rd_W)
    int rd_o = -1, rd_H = 0, rd_W = 0;  // the orientation and the STORED size the plan was built for
    uint8_t* rd_buf[7] = {};       // level table, votes, bins, blocks, hits, {counter, gate}, class sums
    size_t rd_bytes[7] = {};
    unsigned* rd_count() const { return (unsigned*)rd_buf[5]; }
    int* rd_gate() const { return (int*)rd_buf[5] + 16; }
};

}  // namespace rt
}  // namespace vnect

using namespace vnect;
using namespace vnect::rt;

// The object behind the C ABI, and lane 0's plan.
struct vnect_handle : Plan {
    vnect_config cfg{};
    std::string err;
    bool finalized = false;
    int orient = 0;         // vnect_set_orientation: how the frames submitted from now on are stored (orient.h; 0: as they are shown)
    bool pre_only = false;  // vnect_config::preprocess_only: the input batch buffer and the resize tables, nothing else
    bool x3 = false;    // VNECT_FP32_SPLIT: fp32 tensors; the 64x64-tile layers multiply on the bf16 pipe by three-way splits (conv.hip, X3)
    std::map<std::string, HostArray> weights;
    ScaleTabs stabs_host{};      // the host's copy of d_stabs (plan::stem_frame_fits reads it)
    float* in3 = nullptr;  // (S,368,368,3) staging for vnect_forward / preprocess read-back
    char* param_cur = nullptr;     // bump allocator over large blocks for packed weights / biases (param_alloc)
    size_t param_left = 0;
    std::vector<Plan*> lanes;   // [0] is this handle, then cfg.lanes - 1 more.  Frames on different lanes overlap everywhere except in the
                                // joints kernel (the filters are a chain)
    int stream_batch = 1;
    std::vector<Plan*> bplans;  // two video streams per launch: the batched plan once per lane, bplans[i] on lanes[i]'s stream
    // people mode (vnect_set_people; PEOPLE.md): persons 0 .. people-1 of ONE video are streams 0 .. people-1, submitted together
    int people = 0;             // 0: off
    bool people_pair = false;   // finalize builds pplans when people >= 2 and 2 S images fit a batch
    std::vector<Plan*> pplans;  // the (2 S)-image plan of a PAIR of persons once per lane, pplans[i] on lanes[i]'s stream (a batched plan
                                // under another name: a handle with bplans refuses tracking, a people handle is made for it)
    int last_people_units = 0, last_people_paired = 0;  // vnect_result_people: of the people frame submitted last
    // pre/post
    uint8_t* frames = nullptr;  // num_frame_slots * max_frame_bytes
    // A host frame's way to a slot: pinned (page-locked) buffers.  [0], [1] are the caller's capture buffers (vnect_frame_buffer; they
    // only move when the caller asks for a larger one): a frame that lies inside one of them is copied to the device straight from there.
    // Any other pointer is first copied into [2] by the CPU (grown on demand; its users are synchronous, so one suffices).
    uint8_t* stage[3] = {};
    uint8_t* stage_dev[3] = {};  // the same buffers as the device addresses them (hipHostMallocMapped)
    size_t stage_cap[3] = {};
    size_t pre_frame_cap = 0;   // preprocess_only: bytes of the one, growable frame slot
    uint8_t* preview_stage = nullptr;  // vnect_preview_device with a host `out`: the kernel's packed output, copied out from here (grown on demand)
    size_t preview_stage_cap = 0;
    RingPictures previews;  // tracked previews (vnect_submit_tracked_device_preview): sized at the first such submit
    // the 3-D view (rt_view.cpp; view3d.h).  vnect_view3d_device: the confidences and joints on the device (21 doubles, then 63 floats) and, for
    // a host `out`, the kernel's packed output (grown on demand).  Tracked views (vnect_track_view3d): sized when the setting is made
    double* view_in = nullptr;
    uint8_t* view_stage = nullptr;
    size_t view_stage_cap = 0;
    RingPictures views;
    // the person detector (rt_hog.cpp; hog.h): the detector as given (3781 floats, rho last) and on the device, the host-built tables and the
    // level table on the device, the workspace of the three launches and a host frame's device copy -- each grown on demand, never shrunk
    std::vector<float> hog_det;
    float* hog_det_dev = nullptr;
    HogTables* hog_tab = nullptr;
    HogLevel* hog_lv = nullptr;
    uint8_t* hog_buf[6] = {};   // votes, bins, blocks, hits, the counter, a host frame's copy
    size_t hog_cap[6] = {};
    hipStream_t upload_st = nullptr;  // ingest_sync's copy kernel (made on first use): not a lane's compute stream
    hipEvent_t producer_ev = nullptr; // a device frame's producer stream -> the stream that ingests it (wait_for_producer; made on first use)
    struct SlotInfo { int H = 0, W = 0; long long stride = 0; long long last_use = -1; };  // last_use: sequence number of the last frame that reads this slot
    std::vector<SlotInfo> slots;
    ScaleTabs* d_stabs = nullptr;
    MergeGeo mgeo{};  // the merge's resize geometry: passed to the post kernels by value, they compute table entries themselves
    FilterBank* d_fb = nullptr;    // [VNECT_MAX_STREAMS]
    double* h_filt = nullptr;      // pinned, device-mapped: vnect_joint_filter's values in ([0, 64)) and out ([64, 128))
    double* h_filt_dev = nullptr;
    InFlight ring[RING];
    unsigned long long seq_submit = 0, seq_collect = 0;
    unsigned long long unit_submit = 0;  // units submitted so far (FrameInfo::unit)
    Stream streams[VNECT_MAX_STREAMS];
    TrackState* d_track = nullptr;  // [VNECT_MAX_STREAMS]: per stream the next crop and its geometry on the device
    TrackOut* h_tout = nullptr;     // pinned, device-mapped, [RING]: rect_used + status of every tracked frame in flight
    TrackOut* h_tout_dev = nullptr;
    // per-joint confidence (CONFIDENCE.md): every frame's joints stage writes its ring slot's ConfOut beside its JointsOut
    ConfOut* h_conf = nullptr;      // pinned, device-mapped, [RING]
    ConfOut* h_conf_dev = nullptr;
    double* d_conf = nullptr;       // [VNECT_MAX_STREAMS][NJ], device: a tracked frame's confidences for a box kernel launched behind its
                                    // joints stage (VNECT_TRACK_BOX_LAUNCH=1, VNECT_NO_POST_MERGE=1); a stream's frames run one behind the other
    TrackPolicy* d_policy = nullptr;  // [VNECT_MAX_STREAMS]: the streams' loss rules as the box stage reads them
    RedetectOut* h_redet = nullptr;   // pinned, device-mapped, [RING]: a re-detecting stream's frames' verdicts (made by the first vnect_track_redetect)
    RedetectOut* h_redet_dev = nullptr;
    RedetectOut last_redet{};         // vnect_result_redetect: the frame most recently delivered, from its own ring slot
    double last_conf[NJ] = {};      // vnect_result_confidence: the frame most recently delivered, copied out of its own ring slot then
    int last_lost = 0;
    bool have_conf = false;
#if defined(VNECT_TEST_HOOKS) && VNECT_TEST_HOOKS
    // test build only (make testhooks; tests/test_gpu_track_maps.py): vnect_test_maps_override's maps on the device, RING + 1 buffers taken in
    // turn (a frame in flight keeps reading the one it was enqueued with), and the stream the uploads run on
    float* test_maps[RING + 1] = {};
    int test_maps_cur = -1;  // -1: no override
    hipStream_t test_st = nullptr;
#endif
    // cached squarify table
    int sq_H = -1, sq_W = -1;
    FrameParams sq_cache{};
    // profiling
    bool profiling = false;
    hipEvent_t ev[4] = {};
    vnect_timings tim{};
    // comm
    void* comm = nullptr;
    bool sharded = false;
    float* gather = nullptr;  // (S,46,46,84): all ranks' maps
    // exchange by peer writes (vnect_config::exchange == VNECT_XCHG_P2P; kernels.h: XchgArgs)
    char* xblock = nullptr;            // this rank's exchange block (fine-grained device memory, IPC-exported)
    char* xpeer[VNECT_MAX_SCALES] = {};  // every rank's block as this device addresses it; [rank] == xblock
    bool xopened[VNECT_MAX_SCALES] = {};  // xpeer[r] came from hipIpcOpenMemHandle (close it on destroy)
    bool p2p_ready = false;
    unsigned* xtickets = nullptr;
    int* h_xstatus = nullptr;          // pinned, device-mapped, one word per result-ring slot: a peer's flag did not arrive within the bound
    int* h_xstatus_dev = nullptr;
    unsigned* d_xfail = nullptr;       // device word: sequence number of the last frame whose exchange failed (post_kernel skips its joints stage)
};

namespace vnect {
namespace rt {

// message of the last vnect_create failure on THIS thread (handles are created from several threads / processes); rt_abi.cpp
extern thread_local std::string g_create_error;

// the message goes to the plan's handle (vnect_last_error), whichever lane reports it
inline int fail(Plan* p, int code, const std::string& msg) noexcept
{
    try {
        if (p) p->owner->err = msg;
        else g_create_error = msg;
    } catch (...) {  // out of memory while recording the message: the code still goes back
    }
    return code;
}

// No C++ exception crosses the ABI: every extern "C" body runs inside this guard (std::vector / std::string / std::map / new
// can throw std::bad_alloc or std::length_error on a hostile size).
template <typename F>
int guarded(vnect_handle* const* hp, F&& body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(hp ? *hp : nullptr, VNECT_E_INTERNAL, "host allocation failed");
    } catch (const std::exception& e) {
        return fail(hp ? *hp : nullptr, VNECT_E_INTERNAL, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(hp ? *hp : nullptr, VNECT_E_INTERNAL, "internal error");
    }
}

#define HIPCK(h, expr)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(h, VNECT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

template <typename T>
int dev_alloc(Plan* p, T** out, size_t count)
{
    void* q = nullptr;
    HIPCK(p, hipMalloc(&q, std::max<size_t>(count * sizeof(T), 16)));
    p->dev_allocs.push_back(q);
    *out = (T*)q;
    return VNECT_OK;
}

// a buffer of dev_alloc's back: freed, off the plan's list, the pointer null.  The caller has synchronised whatever may still use it.
template <typename T>
int dev_free(Plan* p, T** buf)
{
    if (!*buf) return VNECT_OK;
    HIPCK(p, hipFree(*buf));
    p->dev_allocs.erase(std::find(p->dev_allocs.begin(), p->dev_allocs.end(), (void*)*buf));
    *buf = nullptr;
    return VNECT_OK;
}

// the grow-on-demand buffer: room for `need` elements, never shrunk; *cap moves only when the new buffer is there
template <typename T>
int dev_grow(Plan* p, T** buf, size_t* cap, size_t need)
{
    if (need <= *cap) return VNECT_OK;
    int rc = dev_free(p, buf);
    if (rc) return rc;
    *cap = 0;
    if ((rc = dev_alloc(p, buf, need))) return rc;
    *cap = need;
    return VNECT_OK;
}

// Parameters (packed weights, biases, BN vectors) are carved out of a few large blocks instead of ~150 separate
// allocations: contiguous, 256-byte aligned, and mapped with large page fragments, so a layer's first touch of its
// weights does not start with a page-table walk per 4 KiB.
template <typename T>
int param_alloc(vnect_handle* h, T** p, size_t count)
{
    const size_t need = (std::max<size_t>(count * sizeof(T), 16) + 255) & ~(size_t)255;
    if (h->param_left < need) {
        const size_t block = std::max<size_t>(need, (size_t)32 << 20);
        char* q = nullptr;
        int rc = dev_alloc(h, &q, block);
        if (rc) return rc;
        h->param_cur = q, h->param_left = block;
    }
    *p = (T*)h->param_cur;
    h->param_cur += need, h->param_left -= need;
    return VNECT_OK;
}

template <typename T>
int upload(vnect_handle* h, T** dst, const std::vector<T>& v)
{
    int rc = param_alloc(h, dst, v.size());
    if (rc) return rc;
    HIPCK(h, hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return VNECT_OK;
}

// ---- rt_plan.cpp ---------------------------------------------------------------------------------------------------------------
int build_scale_tables(vnect_handle* h);
int build_up_table(vnect_handle* h);
int squarify_params(vnect_handle* h, int H, int W, FrameParams* fp);
int add_tensor(vnect_handle* h, const std::string& name, int S, int H, int W, int C, int Cs, bool force_f32 = false);
int finalize_impl(vnect_handle* h);
int build_plans(vnect_handle* h);   // lanes 1 .. cfg.lanes - 1, the batched plans and people mode's pair plans
void destroy_plan(Plan* p);         // every plan's teardown, lane 0's (the handle's) included
void destroy_plans(vnect_handle* h);  // all but lane 0
bool plan_writes(const Plan* p, int tensor);  // does a launch of the plan (or the pre-processing) write this tensor?
int live_rows_of(const std::vector<Layer>& layers, int li, int t_out);  // the live-rows rule for launch li: the readers' stride, or 0

// ---- rt_exec.cpp ---------------------------------------------------------------------------------------------------------------
int run_network(Plan* p, bool timed, bool stem_done = false);
int sync_geometry(Plan* p, const FrameParams& fp, int which = 0);  // which 1: a batch's second stream (d_fp2)
int run_pre(Plan* p, const FrameDyn& dyn, bool timed = false, bool want_batch = false);
int run_argmax(Plan* p);
// conf: the frame's ConfOut (device address of its ring slot's); conf_dev: nullptr, or where a box kernel behind this reads the confidences
int run_joints(Plan* p, const FrameDyn& dyn, JointsOut* out, ConfOut* conf, int stream = 0, const FrameParams* fp = nullptr, double* conf_dev = nullptr);  // fp: d_fp
int run_post(Plan* p, const FrameDyn& dyn, JointsOut* out, ConfOut* conf, int stream = 0, const FrameParams* fp = nullptr, double* conf_dev = nullptr);
void deliver_confidence(vnect_handle* h, int ring, bool tracked);  // a frame has been delivered from ring slot `ring`: vnect_result_confidence's values
int check_time(vnect_handle* h, const Stream& s, double t2d, double t3d);
void commit_time(Stream& s, double t2d, double t3d);
int reset_filters_impl(vnect_handle* h, int stream = -1);  // -1: every stream
void roctx_load();
int build_graph(Plan* p);
// A validated frame as the copy kernels address it: what a resolver of rt_ingest.cpp makes of the caller's arguments, what ingest() puts
// into a slot and what a tracked submit (enqueue_frame) cuts the stream's crop out of
enum FrameWhere {
    SRC_SLOT,        // a resident slot (vnect_submit_tracked; nothing to copy)
    SRC_PINNED_BGR,  // BGR rows in pinned host memory: a caller's buffer (vnect_frame_buffer) or the internal stage
    SRC_NV12,        // NV12 planes, in pinned host memory or in the caller's device memory (they differ in the bounds of `nv` and in `producer`)
    SRC_DEVICE       // BGR / RGB at any strides in the caller's device memory
};
struct PinnedBgr {
    const uint8_t* data;  // the frame's first byte as the device addresses it
    long long stride;     // its row stride
    const uint8_t* end;   // end of the pinned buffer it lies in
};
struct FrameSrc {
    FrameWhere where = SRC_SLOT;
    int H = 0, W = 0;         // the frame as it is STORED
    int orient = 0;           // orient.h's code: the picture is np.rot90(frame, orient & 3), mirrored when orient & 4
    int r[4] = {0, 0, 0, 0};  // the crop (x, y, w, h) in ORIENTED coordinates, clipped to the oriented frame (a tracked frame: all of it)
    PinnedBgr bgr{};          // the kernel argument block of its kind: SRC_PINNED_BGR,
    Nv12Src nv{};             // SRC_NV12,
    IngestSrc ing{};          // SRC_DEVICE
    void* producer = VNECT_STREAM_SYNCED;  // a device frame's producer stream as the caller gave it; every host source is synced
    bool people_unit = false;  // a single unit of a people frame (enqueue_people has checked the in-flight limit for all of the frame's units)
    // a tracked device frame that is also drawn into (vnect_submit_tracked_device_draw): one overlay launch behind its box stage
    bool draw = false;
    OverlayTarget draw_target{};
    OverlayInput draw_in{};  // the style: parents, threshold (joints, rect and confidences are read from the ring slot)
    // a tracked device frame that carries a preview (vnect_submit_tracked_device_preview): one preview launch behind its box stage (and in
    // front of its overlay launch, so that it reads the clean frame) into the ring slot's device buffer, and that buffer's copy to the host
    bool preview = false;
    PreviewArgs pv{};        // everything but `out` and `pitch`, which are the ring slot's
    OverlayInput pv_in{};    // the style
};
// a frame in a resident slot as the kernels address it
inline FrameDyn slot_dyn(const vnect_handle* h, int slot, double t2d, double t3d)
{
    FrameDyn dyn{};
    dyn.t2d = t2d, dyn.t3d = t3d;
    dyn.row_stride = h->slots[slot].stride;
    dyn.frame = h->frames + (size_t)slot * h->cfg.max_frame_bytes;
    return dyn;
}
// the ring's pictures: room for `need` bytes per slot (only with nothing in flight: the callers see to that); slot `ring`'s picture of `bytes`
// bytes to its pinned buffer, on `st`; teardown of the pinned buffers (the device buffers are on the handle's list)
int ring_pictures_size(vnect_handle* h, RingPictures& p, size_t need);
int ring_pictures_copy(vnect_handle* h, const RingPictures& p, int ring, size_t bytes, hipStream_t st);
void ring_pictures_free_host(RingPictures& p);
// tk: a tracked frame (vnect_submit_tracked*) -- in `slot` (SRC_SLOT) or where tk says (slot is -1 then)
int enqueue_frame(vnect_handle* h, int slot, double t2d, double t3d, int* ring_out, int stream = 0, const FrameSrc* tk = nullptr);
int collect_impl(vnect_handle* h, double* j2, float* j3, int32_t* stream_out = nullptr, int32_t* rect_out = nullptr);
int track_begin_impl(vnect_handle* h, int stream, int H, int W, const int32_t* rect4);
// people mode: vnect_track_begin for streams 0 .. n-1 (rects: 4 n values or nullptr), all or nothing
int people_begin_impl(vnect_handle* h, int n, int H, int W, const int32_t* rects);
// the next frame of persons 0 .. n-1 -- in `slot`, or (slot -1) where src says -- as ceil(n / 2) lane units; atomic.  src.draw: the P overlay
// launches behind every unit's joints, in person order
int enqueue_people(vnect_handle* h, int n, int slot, double t2d, double t3d, const FrameSrc& src);
int prime(vnect_handle* h);
int enqueue_batch(vnect_handle* h, const int32_t* streams, const int32_t* slots, const double* t2d, const double* t3d);
int forward_batch(vnect_handle* h, const float* batch, float* out);

// ---- rt_ingest.cpp -------------------------------------------------------------------------------------------------------------
// The resolvers: each validates everything and refuses with the entry point's name (`who`) in front; the host ones then copy a pageable
// frame into the internal stage.  Nothing else changes.
// (H, W and the strides describe memory; `orient` is the code the frame is stored under, rects are in oriented coordinates)
int resolve_host_bgr(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, int orient, FrameSrc* out);
int resolve_host_nv12(vnect_handle* h, const char* who, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W,
                      const int32_t* rect4, int orient, FrameSrc* out);  // rect4: nullptr, or the crop (x, y, w, h)
int resolve_pinned_bgr(vnect_handle* h, const char* who, int index, int H, int W, int64_t row_stride, int orient, FrameSrc* out);
int resolve_pinned_nv12(vnect_handle* h, const char* who, int index, int H, int W, int64_t y_stride, int64_t uv_offset, int64_t uv_stride, int orient, FrameSrc* out);
int check_device_frame(vnect_handle* h, const vnect_device_frame* f, void* producer_stream, const char* who, bool allow_rect, int orient, FrameSrc* out);
OrientSrc orient_src_of(const FrameSrc& f);  // the frame as the oriented copies (orient.hip) address it
int ingest(vnect_handle* h, int slot, const FrameSrc& src, hipStream_t st = nullptr);  // asynchronous on st (nullptr: the handle's stream)
int ingest_sync(vnect_handle* h, int slot, const FrameSrc& src);                       // on upload_st, done on return
int upload_frame_impl(vnect_handle* h, int slot, const uint8_t* bgr, int H, int W, int64_t row_stride);
int ensure_stage(vnect_handle* h, int i, size_t bytes);
int wait_for_producer(vnect_handle* h, void* producer_stream, hipStream_t consumer);

// ---- rt_draw.cpp ---------------------------------------------------------------------------------------------------------------
// validates a draw's target (check_device_frame; a rect is refused) and style, and describes them; src_out (may be null): the frame as a source
int check_draw(vnect_handle* h, const char* who, const vnect_device_frame* f, void* stream, const vnect_overlay_style* style, int orient, OverlayTarget* t,
               OverlayInput* in, FrameSrc* src_out);
int draw_device_impl(vnect_handle* h, const vnect_device_frame* target, void* stream, const double* j2d, const double* conf, const int32_t* rect4,
                     const vnect_overlay_style* style);

// the preview (vnect_preview_size / vnect_preview_device; preview.h)
int preview_size_impl(vnect_handle* h, const vnect_device_frame* f, const vnect_preview_spec* spec, int32_t* out_hw);
int preview_device_impl(vnect_handle* h, const vnect_device_frame* f, void* stream, const double* j2d, const double* conf, const int32_t* rect4,
                        const vnect_overlay_style* style, const vnect_preview_spec* spec, void* out, int64_t out_pitch);

// a tracked submit's preview: validates frame (as check_draw does when `style_too`), style and spec, sizes the ring's preview buffers, fills s->pv
int check_tracked_preview(vnect_handle* h, const char* who, const vnect_device_frame* f, void* stream, const vnect_overlay_style* style,
                          const vnect_preview_spec* spec, int orient, FrameSrc* s);

// ---- rt_view.cpp ---------------------------------------------------------------------------------------------------------------
// the 3-D view (vnect_view3d_device, vnect_track_view3d; view3d.h; VIEW3D.md)
int view3d_device_impl(vnect_handle* h, const float* j3d, const double* conf, const vnect_view3d_spec* spec, void* out, int64_t out_pitch);
int track_view3d_impl(vnect_handle* h, int stream, const vnect_view3d_spec* spec);
// where `out` lies: 1 device memory of the handle's device ([*lo, *end): its allocation), 0 host memory (pinned or pageable), -1 neither (rt_draw.cpp)
int out_kind(vnect_handle* h, const void* p, const uint8_t** lo, const uint8_t** end);

// ---- rt_hog.cpp ----------------------------------------------------------------------------------------------------------------
// the person detector (vnect_hog_*; hog.h; HOG.md)
int hog_set_detector_impl(vnect_handle* h, const float* w, int n);
int hog_levels_impl(vnect_handle* h, const vnect_device_frame* f, const vnect_hog_spec* spec, int32_t* n_out, int32_t* hw_out, double* scales_out, int capacity);
int hog_detect_device_impl(vnect_handle* h, const vnect_device_frame* f, void* stream, const vnect_hog_spec* spec, int32_t* rects4, double* weights, int capacity,
                           int32_t* count_out);
int hog_detect_host_impl(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, const vnect_hog_spec* spec, int32_t* rects4, double* weights,
                         int capacity, int32_t* count_out);
// re-detection inside the tracked loop (vnect_track_redetect; hog.h: THE RULE)
int track_redetect_impl(vnect_handle* h, int stream, const vnect_hog_spec* spec, int enable);
// the stream's level table and workspace for (H, W) oriented frames under `orient`; never with a tracked frame of the stream in flight
int redetect_prepare(vnect_handle* h, int stream, int H, int W, int orient);
// behind tracked frame `xseq`'s box stage on `st`: the counter reset, the three gated launches and the pick kernel; the verdict goes to ring slot `ring`
int redetect_enqueue(vnect_handle* h, int stream, const FrameSrc& src, unsigned xseq, int ring, hipStream_t st);

// ---- rt_comm.cpp ---------------------------------------------------------------------------------------------------------------
int exchange_maps(vnect_handle* h, unsigned long long seq, int ring);
bool comm_ready(const vnect_handle* h);
void comm_destroy(vnect_handle* h);  // the handle's RCCL communicator, if it has one

}  // namespace rt
}  // namespace vnect
