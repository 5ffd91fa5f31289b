// rt_exec.cpp -- running frames on a plan: launch sequences, the hipGraph and its profiling twin, lane choice, video streams, the enqueue
// stages and the submits built from them (a frame, a batch of two streams, a pair of persons; people mode on top), collect, the warm
// start.  One call of VNectEstimator.__call__ (the reference's src/estimator.py:97-142) is enqueue_frame +
// collect_impl.  (How a frame gets into a slot, or a tracked frame's description to enqueue_frame: rt_ingest.cpp.)
#include "runtime.h"

namespace vnect {
namespace rt {

// ---- launch sequences -------------------------------------------------------------------------------
// the stem's or a conv layer's arguments for layer li of plan p: stamping into the layer's profiling slots (timed), or not at all
template <typename Args>
static Args stamped(const Plan* p, const Args& args, int li, bool timed)
{
    Args a = args;
    a.prof = timed ? p->d_prof + PROF_SLOTS * li : nullptr;
    a.prof_end = timed ? p->d_prof_end + (size_t)PROF_WGS * li : nullptr;
    return a;
}

// the maps the merge reads: the plan's own, or on a pyramid-sharded handle all ranks'
static const float* maps_of(const Plan* p) { return p->owner->sharded ? p->owner->gather : p->tensors[p->t_out].d; }

// the stem from the batch tensor, which a pyramid launch (or vnect_forward) has written
static int stem_from_batch(Plan* p, bool timed)
{
    StemArgs a = stamped(p, p->stem, p->l_conv1, timed);
    a.from_frame = 0;
    HIPCK(p, launch_stem(a, p->st));
    return VNECT_OK;
}

// `stem_done`: the caller has launched the stem from the frame already (enqueue_frame: it takes the frame's arguments by value)
int run_network(Plan* h, bool timed, bool stem_done)
{
    int rc;
    for (Layer& L : h->layers) {
        const int li = (int)(&L - h->layers.data());
        if (h->stem_mode && (li == h->l_conv1 || li == h->l_pool1)) {
            // (stem_mode 1, or vnect_forward on a stem_mode 2 handle)
            if (li == h->l_conv1 && !stem_done && (rc = stem_from_batch(h, timed))) return rc;
            continue;
        }
        if (h->stem_mode && h->stem_pair && li == h->l_pool1 + 1) continue;  // ran inside the stem launch
        if (L.op == OP_CONV) {
            HIPCK(h, launch_conv(stamped(h, L.a, li, timed), L.BM, L.BN, L.KG, h->st));
            if (L.a.ksplit > 1) HIPCK(h, launch_reduce(L.r, h->st));
        } else if (L.op == OP_POOL) {
            const Tensor &i = h->tensors[L.in], &o = h->tensors[L.out];
            HIPCK(h, launch_maxpool(i.d, o.d, i.S, i.H, i.W, i.Cs, o.H, o.W, h->el(), h->st));
        } else {
            const Tensor& t = h->tensors[L.out];
            HIPCK(h, launch_bone(t.d, (long long)t.S * t.H * t.W, t.Cs, h->el(), h->st));
        }
    }
    return VNECT_OK;
}

// Crop geometry -> d_fp, only if it differs from what the device holds (a stream of equally sized crops never uploads).
// In-stream, so frames still in flight keep the geometry they were launched with.
int sync_geometry(Plan* h, const FrameParams& fp, int which)
{
    FrameParams& held = which ? h->fp_dev2 : h->fp_dev;
    bool& valid = which ? h->fp_dev2_valid : h->fp_dev_valid;
    if (valid && memcmp(&held, &fp, sizeof fp) == 0) return VNECT_OK;
    const int r = h->fp_ring = (h->fp_ring + 1) % RING;  // a staging slot of its own: earlier copies may still be queued
    *h->h_fp[r] = fp;
    HIPCK(h, hipMemcpyAsync(which ? h->d_fp2 : h->d_fp, h->h_fp[r], sizeof(FrameParams), hipMemcpyHostToDevice, h->st));
    held = fp, valid = true;
    return VNECT_OK;
}

int run_pre(Plan* h, const FrameDyn& dyn, bool timed, bool want_batch)
{
    const vnect_handle* o = h->owner;
    const int scale0 = o->sharded ? o->cfg.pyramid_rank : 0;
    const bool stem = h->stem_mode == 2 && !want_batch;
    // gen_input_batch + conv1 + pool1 in ONE launch, the batch tensor never written: for frames whose squarify step is a copy (long
    // side == 368) at scales whose rectangles fit the kernel's scratch.  Any other frame: pyramid_kernel, then the stem from the
    // batch tensor -- both in front of the graph, which starts at res2a either way.  Same results bit for bit.
    if (stem && h->stem_frame_ok && h->fp_dev_valid && h->fp_dev.sq.copy) {
        StemArgs a = stamped(h, h->stem, h->l_conv1, timed);
        a.from_frame = 1, a.dyn = dyn;
        HIPCK(h, launch_stem(a, h->st));
        return VNECT_OK;
    }
    HIPCK(h, launch_pyramid(h->d_fp, dyn, o->d_stabs, h->tensors[h->t_input4].d, h->Snet, scale0, h->el(), h->st));
    return stem ? stem_from_batch(h, timed) : VNECT_OK;
}

// multi-scale merge + arg-max (graph-capturable: no per-frame arguments)
int run_argmax(Plan* h)
{
    HIPCK(h, launch_argmax(maps_of(h), h->owner->mgeo, h->d_part, h->st));
    return VNECT_OK;
}

// filters + read-off; results go straight to `out` (a device-mapped pinned host slot)
int run_joints(Plan* h, const FrameDyn& dyn, JointsOut* out, ConfOut* conf, int stream, const FrameParams* fp, double* conf_dev)
{
    const vnect_handle* o = h->owner;
    HIPCK(h, launch_joints(h->d_part, maps_of(h), o->mgeo, o->d_fb + stream, fp ? fp : h->d_fp, dyn, o->cfg.numpy_promotion, out, h->st, conf, conf_dev));
    return VNECT_OK;
}

// both in one launch (post.hip: post_kernel): takes the frame's arguments by value, so it runs behind the graph, not inside it
int run_post(Plan* h, const FrameDyn& dyn, JointsOut* out, ConfOut* conf, int stream, const FrameParams* fp, double* conf_dev)
{
    const vnect_handle* o = h->owner;
    HIPCK(h, launch_post(maps_of(h), o->mgeo, h->d_part, h->d_ticket, o->d_fb + stream, fp ? fp : h->d_fp, dyn, o->cfg.numpy_promotion, out, h->st, conf,
                         conf_dev));
    return VNECT_OK;
}

// vnect_result_confidence's values are taken when a frame is DELIVERED, from that frame's own ring slot: with frames in flight they belong
// to the collected frame, not to the newest one (whose joints stage may be writing another slot meanwhile)
void deliver_confidence(vnect_handle* h, int ring, bool tracked)
{
    const ConfOut& c = h->h_conf[ring];
    memcpy(h->last_conf, c.conf, sizeof h->last_conf);
    h->last_lost = tracked ? c.lost : 0;
    h->have_conf = true;
}

// a tracked frame outside the slots: the crop's rows (packed) into the stream's buffer, on `st` (which has waited for the frame's producer)
static int copy_tracked_crop(vnect_handle* h, int stream, const FrameSrc& src, hipStream_t st)
{
    TrackState* ts = h->d_track + stream;
    const Stream& sm = h->streams[stream];
    if (src.orient && src.where != SRC_SLOT) {  // stored rotated / mirrored: the crop (oriented coordinates) through the oriented copy
        HIPCK(h, launch_orient_copy_track(ts, orient_src_of(src), src.orient, src.H, src.W, sm.track_buf, st));
        return VNECT_OK;
    }
    switch (src.where) {
    case SRC_SLOT: break;
    case SRC_PINNED_BGR: HIPCK(h, launch_frame_copy_track(ts, src.bgr.data, sm.track_buf, sm.track_H, sm.track_W, src.bgr.stride, src.bgr.end, st)); break;
    case SRC_NV12: HIPCK(h, launch_nv12_copy_track(ts, src.nv, sm.track_buf, sm.track_H, sm.track_W, st)); break;
    case SRC_DEVICE: HIPCK(h, launch_ingest_copy_track(ts, src.ing, sm.track_buf, sm.track_H, sm.track_W, st)); break;
    }
    return VNECT_OK;
}

// gen_input_batch of a tracked frame on lane L: the crop the stream's state names (its rows first copied out of the frame when that
// lies outside the slots), the pyramid from it, and on a stem_mode 2 lane the stem from the batch tensor (the host does not know whether
// the crop's squarify step is a copy, which the stem's frame form needs; the results are the same bit for bit)
static int run_pre_tracked(vnect_handle* h, Plan* L, int stream, const FrameDyn& dyn, const FrameSrc& src, bool timed)
{
    TrackState* ts = h->d_track + stream;
    // a frame outside the slots: this lane's stream waits for its producer, then copies the crop's rows (packed) into the stream's buffer
    int rc = wait_for_producer(h, src.producer, L->st);
    if (rc) return rc;
    if ((rc = copy_tracked_crop(h, stream, src, L->st))) return rc;
    HIPCK(h, launch_pyramid_track(ts, dyn, src.where != SRC_SLOT, h->d_stabs, L->tensors[L->t_input4].d, L->Snet, L->el(), L->st));
    return L->stem_mode == 2 ? stem_from_batch(L, timed) : VNECT_OK;
}

// OneEuroFilter.py:65-66: `if self.__lasttime and timestamp: self.__freq = 1.0 / (timestamp - self.__lasttime)`.
//   t == last  -> ZeroDivisionError (VNECT_E_TIMESTAMP);
//   t <  last  -> freq < 0, so alpha = 1 / (1 + tau * freq) leaves (0, 1] and LowPassFilter.__setAlpha raises ValueError
//                 (OneEuroFilter.py:19-23) -> VNECT_E_TIMEORDER.
// Nothing is committed here: the reference would leave half-updated filters behind its exception, this path rejects the call
// before any state changes, and the host-side copy of the last timestamps moves only after the frame has been enqueued.
int check_time(vnect_handle* h, const Stream& s, double t2d, double t3d)
{
    if (s.t.have2 && s.t.last2 != 0.0 && t2d != 0.0) {
        if (t2d == s.t.last2) return fail(h, VNECT_E_TIMESTAMP, "t2d equals the previous 2-D filter timestamp");
        if (t2d < s.t.last2) return fail(h, VNECT_E_TIMEORDER, "t2d is earlier than the previous 2-D filter timestamp");
    }
    if (s.t.have3 && s.t.last3 != 0.0 && t3d != 0.0) {
        if (t3d == s.t.last3) return fail(h, VNECT_E_TIMESTAMP, "t3d equals the previous 3-D filter timestamp");
        if (t3d < s.t.last3) return fail(h, VNECT_E_TIMEORDER, "t3d is earlier than the previous 3-D filter timestamp");
    }
    return VNECT_OK;
}
// `self.__lasttime = timestamp` runs on every call, also with timestamp 0.0 / None
void commit_time(Stream& s, double t2d, double t3d) { s.t = {true, true, t2d, t3d}; }

int reset_filters_impl(vnect_handle* h, int stream)  // -1: every stream
{
    std::vector<FilterBank> fb(1);
    memset(fb.data(), 0, sizeof(FilterBank));
    for (int j = 0; j < NJ; j++) {
        for (int k = 0; k < 2; k++) {  // filter_config_2d, estimator.py:34-39
            Filt& f = fb[0].f2[j][k];
            f.freq = 30, f.mincutoff = 1.7, f.beta = 0.3, f.dcutoff = 0.4;
        }
        for (int k = 0; k < 3; k++) {  // filter_config_3d, estimator.py:40-45
            Filt& f = fb[0].f3[j][k];
            f.freq = 30, f.mincutoff = 0.8, f.beta = 0.4, f.dcutoff = 0.4;
        }
    }
    for (int s = 0; s < VNECT_MAX_STREAMS; s++) {
        if (stream >= 0 && s != stream) continue;
        HIPCK(h, hipMemcpyAsync(h->d_fb + s, fb.data(), sizeof(FilterBank), hipMemcpyHostToDevice, h->st));
        h->streams[s].t.have2 = h->streams[s].t.have3 = false;
    }
    HIPCK(h, hipStreamSynchronize(h->st));
    return VNECT_OK;
}

// ---- roctx ranges (SURVEY 5 aux: tracing).  Opt-in with VNECT_ROCTX=1; libroctx64 is dlopen'ed, so nothing links it. -----
// The ranges bracket the ENQUEUE of each stage of a frame on the host thread (pre-processing, conv stack + merge/arg-max,
// filters + read-off); rocprofv3 --marker-trace shows them above the kernel rows of the same stream.
static struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
} g_roctx;
void roctx_load()
{
    if (g_roctx.tried) return;
    g_roctx.tried = true;
    const char* e = getenv("VNECT_ROCTX");
    if (!e || !atoi(e)) return;
    void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);  // what rocprofv3 --marker-trace listens to
    if (!lib) lib = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return;
    g_roctx.push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
    g_roctx.pop = (int (*)())dlsym(lib, "roctxRangePop");
    if (!g_roctx.push || !g_roctx.pop) g_roctx.push = nullptr, g_roctx.pop = nullptr;
}
struct RoctxRange {
    explicit RoctxRange(const char* name) { if (g_roctx.push) g_roctx.push(name); }
    ~RoctxRange() { if (g_roctx.pop) g_roctx.pop(); }
};

// The part of a frame without per-frame arguments (what the hipGraph holds): conv stack, merge + arg-max.  The pyramid kernel
// before it and the joints kernel after it take the frame's arguments by value and are launched around the graph.  A
// pyramid-sharded handle's graph ends with the conv stack: the exchange (whose flag value / parity change every frame) and the
// merge + arg-max launch behind it are eager (two captured parts around the exchange -- the
// second part is the single arg-max launch, which gains nothing from a graph of its own).
static int run_frame_kernels(Plan* h, bool timed)
{
    const size_t pbytes = h->layers.size() * PROF_SLOTS * sizeof(unsigned long long);
    int rc = run_network(h, timed, h->stem_mode == 2);  // stem_mode 2: run_pre has launched the stem in front of this
    if (rc) return rc;
    if (!h->owner->sharded && !h->post_merged && (rc = run_argmax(h))) return rc;
    if (timed) {
        HIPCK(h, hipMemcpyAsync(h->h_prof, h->d_prof, pbytes, hipMemcpyDeviceToHost, h->st));
        HIPCK(h, hipMemcpyAsync(h->h_prof_end, h->d_prof_end, h->layers.size() * PROF_WGS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
    }
    return VNECT_OK;
}

int build_graph(Plan* h)
{
    if (h->gexec) hipGraphExecDestroy(h->gexec), h->gexec = nullptr;
    if (h->graph) hipGraphDestroy(h->graph), h->graph = nullptr;
    if (h->pgexec) hipGraphExecDestroy(h->pgexec), h->pgexec = nullptr;
    if (h->pgraph) hipGraphDestroy(h->pgraph), h->pgraph = nullptr;
    if (!h->owner->cfg.use_graph) return VNECT_OK;
    HIPCK(h, hipStreamBeginCapture(h->st, hipStreamCaptureModeThreadLocal));
    int rc = run_frame_kernels(h, false);
    hipError_t e = hipStreamEndCapture(h->st, &h->graph);
    if (rc) return rc;
    HIPCK(h, e);
    HIPCK(h, hipGraphInstantiate(&h->gexec, h->graph, nullptr, nullptr, 0));
    if (!h->prof_graph) return VNECT_OK;
    // profiling twin: identical launches, but every conv kernel stamps {min start, max end} (s_memrealtime)
    HIPCK(h, hipStreamBeginCapture(h->st, hipStreamCaptureModeThreadLocal));
    rc = run_frame_kernels(h, true);
    e = hipStreamEndCapture(h->st, &h->pgraph);
    if (rc) return rc;
    HIPCK(h, e);
    HIPCK(h, hipGraphInstantiate(&h->pgexec, h->pgraph, nullptr, nullptr, 0));
    return VNECT_OK;
}

// Frames (or batches of two streams' frames) in flight, and how many may be: one lane queues two on its stream, more lanes one each
static unsigned long long units_in_flight(const vnect_handle* h)
{
    return h->seq_submit == h->seq_collect ? 0 : h->unit_submit - h->ring[h->seq_collect % RING].f.unit;
}
static unsigned long long max_in_flight(const vnect_handle* h) { return std::max<size_t>(h->lanes.size(), 2); }

// the lane a frame (or batch) submitted now runs on: the first whose last frame has been collected (lane 0 when nothing is in flight)
static Plan* pick_lane(vnect_handle* h, bool timed)
{
    if (!timed)
        for (Plan* l : h->lanes)
            if (l->lane_seq < (long long)h->seq_collect) return l;
    return h;
}

// use_graph 2 (auto): a frame submitted while nothing is in flight -- the synchronous pattern -- is launched eagerly (median
// 6.6 us shorter than pyramid + graph replay + joints, A/B in one call, both precisions; the host has nothing else to do
// meanwhile), a frame submitted behind others replays the graph (the host must stay ahead of two or three lanes)
static bool replays(const vnect_handle* h, const Plan* p) { return p->gexec && (h->cfg.use_graph == 1 || h->seq_submit != h->seq_collect); }

// ---- the ring's pictures (RingPictures: tracked previews, tracked 3-D views) ---------------------------------------------------------------
int ring_pictures_size(vnect_handle* h, RingPictures& p, size_t need)
{
    if (need <= p.cap) return VNECT_OK;
    int rc;
    for (int i = 0; i < RING; i++) {
        if (p.host[i]) HIPCK(h, hipHostFree(p.host[i]));
        p.host[i] = nullptr;
        if ((rc = dev_free(h, &p.dev[i]))) return rc;
    }
    p.cap = 0, p.deliver(-1, 0, 0);
    for (int i = 0; i < RING; i++) {
        HIPCK(h, hipHostMalloc((void**)&p.host[i], need, hipHostMallocDefault));
        if ((rc = dev_alloc(h, &p.dev[i], need))) return rc;
    }
    p.cap = need;
    return VNECT_OK;
}

int ring_pictures_copy(vnect_handle* h, const RingPictures& p, int ring, size_t bytes, hipStream_t st)
{
    HIPCK(h, hipMemcpyAsync(p.host[ring], p.dev[ring], bytes, hipMemcpyDeviceToHost, st));
    return VNECT_OK;
}

void ring_pictures_free_host(RingPictures& p)
{
    for (uint8_t* q : p.host)
        if (q) hipHostFree(q);
}

// ---- the stages of a submit: what enqueue_frame, enqueue_batch and enqueue_pair (and enqueue_people's drawing) are built from ------------------
// The stream's previous frame ran on another lane and may still be in flight: `lane`'s stream waits for it.  (A batched plan and a pair plan
// run on their lane's stream.)  WHERE a submit waits is its own decision: the filters are a chain within a video stream, so a frame's
// post-processing waits; a tracked frame's crop is the previous frame's box stage's output, so everything of it waits.
static int wait_prev(vnect_handle* h, const Stream& sm, Plan* lane)
{
    if (sm.seq >= (long long)h->seq_collect && sm.lane && sm.lane != lane) HIPCK(h, hipStreamWaitEvent(lane->st, h->ring[sm.seq % RING].done, 0));
    return VNECT_OK;
}

// the conv stack (+ merge + arg-max) of plan p: its graph, its profiling twin where it has one, or the launches themselves
static int launch_stack(const vnect_handle* h, Plan* p, bool timed)
{
    if (replays(h, p) && !timed) HIPCK(p, hipGraphLaunch(p->gexec, p->st));
    else if (p->pgexec && timed) HIPCK(p, hipGraphLaunch(p->pgexec, p->st));
    else return run_frame_kernels(p, timed);
    return VNECT_OK;
}

// lane's plan among `plans` (bplans, pplans: plans[i] runs on lanes[i]'s stream)
static Plan* sibling(const std::vector<Plan*>& plans, const vnect_handle* h, const Plan* lane)
{
    return plans[std::find(h->lanes.begin(), h->lanes.end(), lane) - h->lanes.begin()];
}

static bool slot_ok(const vnect_handle* h, int slot) { return slot >= 0 && slot < (int)h->slots.size() && h->slots[slot].H != 0; }

// a tracked frame of `stream` as the kernels address it: the whole frame in `slot`, or the stream's crop buffer
static FrameDyn tracked_dyn(const vnect_handle* h, int stream, bool from_slot, int slot, double t2d, double t3d)
{
    const Stream& sm = h->streams[stream];
    FrameDyn dyn{};
    if (from_slot) dyn = slot_dyn(h, slot, t2d, t3d);
    else dyn.t2d = t2d, dyn.t3d = t3d, dyn.frame = sm.track_buf;  // (the crop's rows, packed: pyramid_track_kernel takes their stride from the state)
    dyn.xfail = &h->d_track[stream].fail, dyn.xseq = sm.track_seq;  // a refused crop skips the joints stage
    return dyn;
}

// a preview's arguments with ring slot `ring`'s device buffer as the output, and that picture's way on to the slot's pinned buffer
static PreviewArgs preview_into(const vnect_handle* h, const PreviewArgs& pv, int ring)
{
    PreviewArgs a = pv;
    a.out = h->previews.dev[ring], a.pitch = 3LL * a.g.dw;
    return a;
}
static int preview_copy(vnect_handle* h, const PreviewArgs& a, int ring, hipStream_t st)
{
    return ring_pictures_copy(h, h->previews, ring, 3 * (size_t)a.g.dw * a.g.dh, st);
}

// run_estimator_ps.py:90 (q_joints.put(joints_3d): the 3-D plot's input): the 3-D view (vnect_track_view3d) of the frame in ring slot `ring` --
// joints_3d, status and confidences read from the slot -- into the slot's device buffer and on to its pinned host buffer
static int view3d_tail(vnect_handle* h, const Stream& sm, int ring, hipStream_t st)
{
    View3dArgs a = sm.v3;
    a.out = h->views.dev[ring], a.pitch = 3LL * a.cols;
    HIPCK(h, launch_view3d(a, nullptr, nullptr, h->ring[ring].out_dev, a.has_conf ? h->h_conf_dev + ring : nullptr, st));
    return ring_pictures_copy(h, h->views, ring, 3 * (size_t)a.cols * a.rows, st);
}

// Every launch of a frame has been accepted: only now its description `f` goes into its ring entry, whole, and the stream, the lane and the slot
// move on to it.  (unit_submit advances once per UNIT: the caller's.)  Returns the frame's ring slot.
static int commit_result(vnect_handle* h, Plan* lane, int slot, double t2d, double t3d, FrameInfo f)
{
    Stream& sm = h->streams[f.stream];
    const int ring = (int)(h->seq_submit % RING);
    f.unit = h->unit_submit;
    if (f.tracked) f.before = sm.t, sm.track_seq++;  // (a refused crop rolls the timestamps back)
    h->ring[ring].f = f;
    commit_time(sm, t2d, t3d);
    sm.seq = lane->lane_seq = (long long)h->seq_submit, sm.lane = lane;
    if (slot >= 0) h->slots[slot].last_use = (long long)h->seq_submit;
    h->seq_submit++;
    return ring;
}

// enqueue one frame from a resident slot; results land in its ring entry's slot.  `tk`: a tracked frame (vnect_submit_tracked*) -- its crop and
// geometry are the stream's state on the device, the frame is the whole one (in `slot`, or outside the slots where tk says: then slot is -1)
int enqueue_frame(vnect_handle* h, int slot, double t2d, double t3d, int* ring_out, int stream, const FrameSrc* tk)
{
    const bool from_slot = !tk || tk->where == SRC_SLOT;
    if (stream < 0 || stream >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
    if (stream != 0 && h->sharded) return fail(h, VNECT_E_ARG, "a pyramid-sharded handle serves one stream");
    if (from_slot && !slot_ok(h, slot)) return fail(h, VNECT_E_ARG, "frame slot empty or out of range");
    const Stream& sm = h->streams[stream];
    if (tk && from_slot && (h->slots[slot].H != sm.track_H || h->slots[slot].W != sm.track_W))
        return fail(h, VNECT_E_ARG, "the slot's frame is not of the size vnect_track_begin gave for this stream");
    if (!(tk && tk->people_unit) && units_in_flight(h) >= max_in_flight(h))  // (a people frame's units were counted together: enqueue_people)
        return fail(h, VNECT_E_STATE, "too many frames in flight: collect one first");
    if (h->sharded && !comm_ready(h))  // refuse before any filter / timestamp state changes
        return fail(h, VNECT_E_STATE, "pyramid-sharded handle: call vnect_comm_init / vnect_comm_p2p_init before inference");
    FrameParams fp;
    int rc = tk ? VNECT_OK : squarify_params(h, h->slots[slot].H, h->slots[slot].W, &fp);
    if (rc) return rc;
    rc = check_time(h, sm, t2d, t3d);
    if (rc) return rc;
    const int ring = (int)(h->seq_submit % RING);
    const InFlight& e = h->ring[ring];
    FrameDyn dyn = tk ? tracked_dyn(h, stream, from_slot, slot, t2d, t3d) : slot_dyn(h, slot, t2d, t3d);
    const bool timed = h->profiling;
    // Lane: the first whose last frame has been collected (lane 0 when nothing is in flight).  Frames on different lanes
    // overlap -- the idle CUs between one frame's launches are the other frames' -- and only the post-processing launch of a frame
    // (post_kernel: merge + arg-max + joints; with VNECT_NO_POST_MERGE=1 only the joints kernel) waits for the SAME video's previous
    // frame.  Measured (round 3, A/B in one call): 1 388-1 390 frames/s three deep with the merged launch, 1 388-1 389 with the two
    // launches -- ordering the 17-us merged launch instead of the 11-us joints kernel costs nothing measurable.
    Plan* L = pick_lane(h, timed);
    if (!tk && (rc = sync_geometry(L, fp))) return rc;
    // a tracked frame's crop is its previous frame's box kernel's output: everything of it waits
    if (tk && (rc = wait_prev(h, sm, L))) return rc;
    if (timed) HIPCK(h, hipEventRecord(h->ev[0], L->st));
    {
        RoctxRange r("vnect:gen_input_batch");
        if ((rc = tk ? run_pre_tracked(h, L, stream, dyn, *tk, timed) : run_pre(L, dyn, timed))) return rc;
    }
    RoctxRange r_net("vnect:conv_stack+merge+argmax");
    if ((rc = launch_stack(h, L, timed))) return rc;
#if defined(VNECT_TEST_HOOKS) && VNECT_TEST_HOOKS
    // test build only (vnect_test_maps_override): the conv stack's output replaced by the caller's maps, on the frame's own lane stream --
    // everything behind it (post-processing, box stage, ring slot, collect) is the product's path on chosen maps
    if (h->test_maps_cur >= 0 && !h->sharded)
        HIPCK(h, hipMemcpyAsync(L->tensors[L->t_out].d, h->test_maps[h->test_maps_cur], (size_t)h->S * HM * HM * MAPC * sizeof(float),
                                hipMemcpyDeviceToDevice, L->st));
#endif
    if (h->sharded) {  // (one lane.)  The one exchange of the pyramid path, then the merge + arg-max over everybody's maps
        if (g_roctx.pop) g_roctx.pop(), g_roctx.push("vnect:exchange+merge+argmax");
        if ((rc = exchange_maps(h, h->seq_submit, ring))) return rc;
        dyn.xfail = h->d_xfail, dyn.xseq = (unsigned)(h->seq_submit + 1);  // post_kernel skips the joints stage of a frame whose exchange failed
        if (!L->post_merged && (rc = run_argmax(L))) return rc;
    }
    if (g_roctx.pop) g_roctx.pop(), g_roctx.push(L->post_merged ? "vnect:merge+argmax+filters+readoff" : "vnect:filters+readoff");  // r_net's pop now closes this range
    // the filters are a chain WITHIN a video stream: this frame's post-processing waits for the stream's previous frame if that one
    // ran on another lane and may still be in flight (frames of other streams are no concern of it)
    if (!tk && (rc = wait_prev(h, sm, L))) return rc;
    // writes the ring slot in pinned host memory
    // A tracked frame also turns its joints into frame coordinates and grows the next crop and its geometry (trackbox.h): as the tail of
    // post_kernel (the default: measured faster, TRACKING.md), or -- the two-launch post-processing, VNECT_TRACK_BOX_LAUNCH=1 (A/B, read per
    // frame) -- as a launch of its own behind it, which reads the joints back from the result ring slot
    const bool box_tail = tk && L->post_merged && !getenv("VNECT_TRACK_BOX_LAUNCH");
    // vnect_track_redetect: the box stage also tells the detection chain behind it whether the frame is lost (the stream's gate word)
    const bool redetect = tk && sm.rd_on;
    int* const gate = redetect ? sm.rd_gate() : nullptr;
    if (box_tail) {
        HIPCK(h, launch_post_track(maps_of(L), h->mgeo, L->d_part, L->d_ticket, h->d_fb + stream, h->d_track + stream, dyn, h->cfg.numpy_promotion,
                                   e.out_dev, h->h_tout_dev + ring, L->st, h->h_conf_dev + ring, h->d_policy + stream, gate));
    } else {
        // (a box kernel of its own takes the confidences from device memory, not from the ring slot: the joints stage leaves them in both)
        const FrameParams* tfp = tk ? &h->d_track[stream].fp : nullptr;
        double* cdev = tk ? h->d_conf + (size_t)stream * NJ : nullptr;
        if ((rc = L->post_merged ? run_post(L, dyn, e.out_dev, h->h_conf_dev + ring, stream, tfp, cdev)
                                 : run_joints(L, dyn, e.out_dev, h->h_conf_dev + ring, stream, tfp, cdev)))
            return rc;
        if (tk)
            HIPCK(h, launch_track_box(h->d_track + stream, e.out_dev, h->h_tout_dev + ring, dyn.xseq, L->st, cdev, h->d_policy + stream, h->h_conf_dev + ring, gate));
    }
    // hog_box.py:26-31 in the place of the loop's whole-frame fallback (hog.h: THE RULE): the detection of THIS frame, gated by its box
    // stage's verdict, and the pick that turns the hits into the stream's next crop -- on the frame's stream, in front of the event the
    // stream's next frame waits for, and in front of the overlay launch, so that the detector reads the clean frame
    if (redetect && (rc = redetect_enqueue(h, stream, *tk, dyn.xseq, ring, L->st))) return rc;
    // run_estimator_ps.py:94-96: the frame's preview -- annotated with its own joints and rect_used, read from its ring slot, and scaled --
    // into the slot's device buffer and on to its pinned host buffer; in front of the overlay launch, so that it reads the clean frame
    if (tk && tk->preview) {
        const PreviewArgs a = preview_into(h, tk->pv, ring);
        HIPCK(h, launch_preview(a, tk->pv_in, e.out_dev, h->h_tout_dev + ring, tk->pv_in.has_conf ? h->h_conf_dev + ring : nullptr, L->st));
        if ((rc = preview_copy(h, a, ring, L->st))) return rc;
    }
    // run_estimator_ps.py:92-94: the frame itself annotated with its own joints and the rect it was cropped with, read from its ring slot
    if (tk && tk->draw)
        HIPCK(h, launch_overlay(tk->draw_target, tk->draw_in, e.out_dev, h->h_tout_dev + ring, tk->draw_in.has_conf ? h->h_conf_dev + ring : nullptr, L->st));
    const bool v3 = tk && sm.v3_on;
    if (v3 && (rc = view3d_tail(h, sm, ring, L->st))) return rc;
    if (timed) HIPCK(h, hipEventRecord(h->ev[3], L->st));
    HIPCK(h, hipEventRecord(e.done, L->st));
    FrameInfo f{};
    f.stream = stream, f.tracked = tk != nullptr, f.redetect = redetect;
    if (tk && tk->preview) f.pv_h = tk->pv.g.dh, f.pv_w = tk->pv.g.dw;
    if (v3) f.v3_h = sm.v3.rows, f.v3_w = sm.v3.cols;
    *ring_out = commit_result(h, L, slot, t2d, t3d, f);
    h->unit_submit++;
    return VNECT_OK;
}

// A layer's span on the profiling stamps of plan p (100 MHz ticks): its first workgroup's start, and for a conv launch its latest workgroup
// end (slots past the grid stay 0); any other layer has no end stamps, t1 is 0
struct LayerSpan { unsigned long long t0, t1; };
static LayerSpan layer_span(const Plan* p, size_t i)
{
    LayerSpan s{p->h_prof[PROF_SLOTS * i], 0};
    const unsigned long long* e = p->h_prof_end + (size_t)PROF_WGS * i;
    if (p->layers[i].op == OP_CONV)
        for (int k = 0; k < PROF_WGS; k++) s.t1 = std::max(s.t1, e[k]);
    return s;
}

// a profiled batch's per-layer times (vnect_get_batch_layer_info): first workgroup start to last workgroup end of every conv launch
static void read_layer_ms(Plan* b)
{
    for (size_t i = 0; i < b->layers.size(); i++) {
        Layer& L = b->layers[i];
        const LayerSpan s = layer_span(b, i);
        L.last_ms = (L.op == OP_CONV && s.t1 > s.t0) ? (float)((double)(s.t1 - s.t0) * 1e-5) : 0.f;
    }
}

int collect_impl(vnect_handle* h, double* j2, float* j3, int32_t* stream_out, int32_t* rect_out)
{
    if (h->seq_collect == h->seq_submit) return fail(h, VNECT_E_STATE, "nothing in flight");
    const int ring = (int)(h->seq_collect % RING);
    // the caller is about to consume the joints: poll (a frame is ~1 ms) before falling back to a blocking wait, whose
    // wake-up alone costs tens of microseconds of idle GPU per frame
    hipError_t q = hipErrorNotReady;
    FrameInfo& e = h->ring[ring].f;
    const hipEvent_t done = h->ring[ring].done;
    for (int spin = 0; spin < 200000 && (q = hipEventQuery(done)) == hipErrorNotReady; spin++) {}
    if (q == hipErrorNotReady) q = hipEventSynchronize(done);
    HIPCK(h, q);
    h->seq_collect++;
    if (h->h_xstatus && h->h_xstatus[ring]) {  // one word per ring slot: the error lands on the frame it belongs to
        h->h_xstatus[ring] = 0;
        // The frame's joints stage was skipped on the device (post_kernel: the filter banks did not advance on stale maps), but the
        // ranks are out of step now and the host's timestamps have moved: VNECT_E_COMM means tear the job down and reconnect.
        return fail(h, VNECT_E_COMM, "pyramid exchange: a peer's maps did not arrive within the bound (ranks out of step?); "
                                     "destroy the handles of every rank and reconnect");
    }
    h->previews.deliver(-1, 0, 0);   // (a frame whose crop was refused has no preview)
    h->views.deliver(-1, 0, 0);      // (nor a 3-D view)
    h->last_redet = RedetectOut{};   // (nor a detection)
    if (stream_out) *stream_out = e.stream;
    if (rect_out)
        for (int k = 0; k < 4; k++) rect_out[k] = e.tracked ? h->h_tout[ring].rect[k] : -1;
    if (e.tracked && h->h_tout[ring].status != SQ_OK) {  // the frame's crop was refused: its joints stage was skipped
        Stream& sm = h->streams[e.stream];
        if (sm.track_stopped)
            return fail(h, VNECT_E_STATE, "tracking of this stream stopped at a refused crop: call vnect_track_begin");
        sm.track_stopped = true;
        // vnect_infer's refusal commits no timestamp, and the device's filters did not see this frame (nor the stream's later ones, which
        // are refused too): the host's last timestamps go back to what they were before it
        sm.t = e.before;
        return fail(h, VNECT_E_ARG, crop_refusal(h->h_tout[ring].status));
    }
    if (j2) memcpy(j2, h->ring[ring].out->j2d, sizeof(double) * NJ * 2);
    if (j3) memcpy(j3, h->ring[ring].out->j3d, sizeof(float) * NJ * 3);
    deliver_confidence(h, ring, e.tracked);
    if (e.tracked && e.redetect) {  // the frame's verdict, from its own ring slot like the confidences; what the kernel did not write reads as zero
        const RedetectOut& r = h->h_redet[ring];
        h->last_redet.status = r.status;
        if (r.status != HOG_RD_NOT_RUN) h->last_redet.hits = r.hits;
        if (r.status == HOG_RD_FOUND) memcpy(h->last_redet.rect, r.rect, sizeof r.rect);
    }
    if (e.tracked && e.pv_h) h->previews.deliver(ring, e.pv_h, e.pv_w);
    if (e.tracked && e.v3_h) h->views.deliver(ring, e.v3_h, e.v3_w);
    if (e.prof) read_layer_ms(e.prof), e.prof = nullptr;
    if (h->profiling && !e.batch) {
        float frame_ms = 0;
        hipEventElapsedTime(&frame_ms, h->ev[0], h->ev[3]);
        unsigned long long first = ~0ull, last = 0;
        double conv_ms = 0;
        for (size_t i = 0; i < h->layers.size(); i++) {
            Layer& L = h->layers[i];
            unsigned long long* p = h->h_prof + PROF_SLOTS * i;
            const LayerSpan s = layer_span(h, i);
            const unsigned long long t0 = s.t0, t1 = s.t1;
            if (L.op == OP_CONV)
                for (int k = 1; k <= 8; k++) p[k] = t1;  // vnect_get_layer_stamps keeps its layout
            L.last_ms = 0;
            if (L.op != OP_CONV || t1 <= t0) continue;
            L.last_ms = (float)((double)(t1 - t0) * 1e-5);  // 100 MHz ticks -> ms
            conv_ms += L.last_ms;
            // workgroup 0's span in both clocks ([24], [25] shader cycles; [0], [26] 100 MHz): the clock held during this launch
            if (p[25] > p[24] && p[26] > p[0] && p[26] - p[0] < 100000000ull) h->tim.shader_cycles += (double)(p[25] - p[24]), h->tim.shader_ticks += (double)(p[26] - p[0]);
            first = std::min(first, t0), last = std::max(last, t1);
        }
        // slot of a conv kernel on the stream: its start to the next conv kernel's start when that one follows directly,
        // else its own duration + the median boundary of the direct pairs (pool / reduce / bone / arg-max follow it)
        std::vector<double> gaps;
        std::vector<size_t> convs;
        for (size_t i = 0; i < h->layers.size(); i++)
            if (h->layers[i].op == OP_CONV && h->layers[i].last_ms > 0) convs.push_back(i);
        auto t_start = [&](size_t i) { return h->h_prof[PROF_SLOTS * i]; };
        auto t_end = [&](size_t i) {
            unsigned long long e = 0;
            for (int k = 1; k <= 8; k++) e = std::max(e, h->h_prof[PROF_SLOTS * i + k]);
            return e;
        };
        auto direct = [&](size_t a, size_t b) {  // no kernel in between (the stem stands for conv1 AND pool1)
            return (b == a + 1 || (h->stem_mode && (int)a == h->l_conv1 && b == a + (h->stem_pair ? 3 : 2))) && h->layers[a].a.ksplit == 1;
        };
        for (size_t c = 0; c + 1 < convs.size(); c++)
            if (direct(convs[c], convs[c + 1]) && t_start(convs[c + 1]) > t_end(convs[c]))
                gaps.push_back((double)(t_start(convs[c + 1]) - t_end(convs[c])) * 1e-5);
        std::sort(gaps.begin(), gaps.end());
        const double med_gap = gaps.empty() ? 0.0 : gaps[gaps.size() / 2];
        double slot_ms = 0;
        for (size_t c = 0; c < convs.size(); c++) {
            const size_t i = convs[c];
            if (c + 1 < convs.size() && direct(i, convs[c + 1]) && t_start(convs[c + 1]) > t_start(i))
                slot_ms += (double)(t_start(convs[c + 1]) - t_start(i)) * 1e-5;
            else
                slot_ms += h->layers[i].last_ms + med_gap;
        }
        h->tim.conv_slot_ms += slot_ms;
        h->tim.frames++;
        h->tim.total_ms += frame_ms;                                     // HIP events around the whole frame
        h->tim.net_ms += last > first ? (double)(last - first) * 1e-5 : 0;  // first conv start .. last conv end
        h->tim.conv_ms += conv_ms;                                       // sum of conv kernel durations
    }
    return VNECT_OK;
}

// Warm start: a tracking loop wants its FIRST frames at steady-state speed, but the first ~25 frames behind vnect_finalize run 1.5-3 %
// slower (shader clocks ramp up from idle, instruction and translation caches are cold -- measured).  So finalize runs
// the launch plan a few times on a grey 368 x 368 frame in an empty slot (every lane once more, three in flight), then restores the state a fresh
// handle has: empty slot, new filters, no timestamps.  VNECT_PRIME_FRAMES overrides the count (0 = off).
// Round 6: the count is a MINIMUM -- the grey frames go on until VNECT_PRIME_MS (default 40) milliseconds have passed, at most 400 frames:
// 24 bf16 frames are 8 ms, and the driver-length bench (5 warm-up + 20 timed frames directly behind vnect_finalize) showed every frame
// of such a window 0.5-2 % slower than the one before it (profiles/r06_short_run_tail.txt): the clock ramp takes tens of milliseconds.
int prime(vnect_handle* h)
{
    const int n_env = getenv("VNECT_PRIME_FRAMES") ? atoi(getenv("VNECT_PRIME_FRAMES")) : 24;  // (read per call: a test flips it inside one process)
    const double min_ms = getenv("VNECT_PRIME_MS") ? atof(getenv("VNECT_PRIME_MS")) : 40.0;
    if (n_env <= 0 || h->sharded || (size_t)BOX * BOX * 3 > (size_t)h->cfg.max_frame_bytes) return VNECT_OK;
    int ps = -1;  // an EMPTY frame slot (a caller may have uploaded frames before vnect_finalize: those are not touched)
    for (size_t i = 0; i < h->slots.size() && ps < 0; i++)
        if (h->slots[i].H == 0) ps = (int)i;
    if (ps < 0) return VNECT_OK;
    HIPCK(h, hipMemsetAsync(h->frames + (size_t)ps * h->cfg.max_frame_bytes, 128, (size_t)BOX * BOX * 3, h->st));
    HIPCK(h, hipStreamSynchronize(h->st));
    h->slots[ps].H = BOX, h->slots[ps].W = BOX, h->slots[ps].stride = (long long)BOX * 3;
    int rc = VNECT_OK, ring = 0;
    double t = 1.0;
    // failure injection for the test of this path (tests/test_gpu_surface.py): VNECT_PRIME_INJECT=hip makes the second grey frame fail
    // like a launch error, =state like a benign refusal.  Compiled ONLY into the test build (`make testhooks`, -DVNECT_TEST_HOOKS=1 ->
    // libvnect_hip_testhooks.so; advisor, round 5): the shipped library has no hook on its initialisation path and ignores the variable.
#if defined(VNECT_TEST_HOOKS) && VNECT_TEST_HOOKS
    const char* inject = getenv("VNECT_PRIME_INJECT");
#else
    const char* inject = nullptr;
#endif
    timespec ts0;
    clock_gettime(CLOCK_MONOTONIC, &ts0);
    auto elapsed_ms = [&] {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)(ts.tv_sec - ts0.tv_sec) * 1e3 + (double)(ts.tv_nsec - ts0.tv_nsec) * 1e-6;
    };
    for (int i = 0; (i < n_env || (i < 400 && elapsed_ms() < min_ms)) && !rc; i++, t += 1.0) {
        if (inject && i == 1) {
            rc = fail(h, !strcmp(inject, "hip") ? VNECT_E_HIP : VNECT_E_STATE, std::string("injected warm-start failure (") + inject + ")");
            break;
        }
        rc = enqueue_frame(h, ps, t, t, &ring);
        if (!rc) rc = collect_impl(h, nullptr, nullptr);
    }
    for (int rep = 0; rep < 2 && !rc && h->lanes.size() > 1; rep++) {  // the other lanes: as many frames in flight as there are lanes
        const int depth = (int)h->lanes.size();
        for (int i = 0; i < depth && !rc; i++, t += 1.0) rc = enqueue_frame(h, ps, t, t, &ring);
        for (int i = 0; i < depth && !rc; i++) rc = collect_impl(h, nullptr, nullptr);
    }
    // the batched plan of two streams (vnect_set_stream_batch): synchronous batches, then as many in flight as there are lanes
    for (int i = 0; i < 8 && !rc && !h->bplans.empty(); i++) {
        const int32_t st2[2] = {0, 1}, sl[2] = {ps, ps};
        const int depth = i < 6 ? 1 : (int)h->bplans.size();
        for (int d = 0; d < depth && !rc; d++, t += 1.0) {
            const double tt[2] = {t, t};
            rc = enqueue_batch(h, st2, sl, tt, tt);
        }
        for (int d = 0; d < 2 * depth && !rc; d++) rc = collect_impl(h, nullptr, nullptr);
    }
    // (People mode's pair plans -- pplans -- are NOT warmed here: a paired unit needs tracking streams and their crop buffers, which begin on
    // a finalized handle.  Their graphs are built and their arenas allocated; the first paired frames of a handle pay the cold caches,
    // PEOPLE.md says so.)
    // A fresh handle's state comes back UNCONDITIONALLY: whatever is still in flight is drained and dropped, the slot is emptied, the
    // filter banks are rebuilt.  What the failure means for vnect_finalize depends on its kind (advisor, round 4):
    //  * VNECT_E_HIP / VNECT_E_INTERNAL / VNECT_E_COMM -- a launch was refused or the device faulted on the launch plan this handle
    //    will run for every real frame: that is a broken plan or a broken device, and vnect_finalize returns the code with the reason;
    //  * anything else (a refused argument or state of the grey frame itself) -- the warm start is an optimisation: skipped, noted in
    //    vnect_last_error, vnect_finalize succeeds.
    const std::string why = rc ? h->err : std::string();
    if (rc) {
        for (Plan* l : h->lanes) (void)hipStreamSynchronize(l->st);
        (void)hipGetLastError();
        h->seq_collect = h->seq_submit;
    }
    h->slots[ps] = vnect_handle::SlotInfo();
    const int rf = reset_filters_impl(h);  // (sets h->err itself when it fails)
    for (Stream& sm : h->streams) sm = Stream{};  // (no crop buffer to lose yet: tracking begins on a finalized handle, and this runs inside vnect_finalize)
    h->have_conf = false;  // (the grey frames' confidences are nobody's result: vnect_result_confidence starts at the caller's first delivery)
    for (Plan* l : h->lanes) l->fp_dev_valid = false;  // (the next frame uploads its own geometry)
    for (Plan* b : h->bplans) b->fp_dev_valid = b->fp_dev2_valid = false;
    const bool serious = rc == VNECT_E_HIP || rc == VNECT_E_INTERNAL || rc == VNECT_E_COMM;
    if (rf) {  // the filter banks could not be rebuilt: the handle must not be used; keep both reasons
        if (rc) h->err += "; behind a failed warm start: " + why;
        return rf;
    }
    if (serious) {
        h->err = "warm start failed -- the launch plan or the device is broken: " + why;
        return rc;
    }
    if (rc) h->err = "warm start skipped (not an error of vnect_finalize): " + why;
    return VNECT_OK;
}

// ---- two video streams per launch (vnect_submit_streams) ----------------------------------------------------------------------------
// Frames of two DIFFERENT streams from resident slots as ONE batch on the batched plan: one pyramid launch for both frames, the conv
// stack once for 2 S images, then each stream's merge + arg-max + joints on its own S images (post_kernel with the maps of its half,
// its filter bank, its geometry).  One batch takes one lane and counts once against the in-flight limit; its two results come back
// through collect_impl in array order.  Every check comes before any state changes: a refused batch leaves every filter bank, every
// timestamp and every slot as it was.
int enqueue_batch(vnect_handle* h, const int32_t* streams, const int32_t* slots, const double* t2d, const double* t3d)
{
    if (h->bplans.empty()) return fail(h, VNECT_E_STATE, "vnect_submit_streams of two frames needs vnect_set_stream_batch(h, 2) before vnect_finalize");
    FrameParams fp[2];
    FrameDyn dyn[2] = {};
    for (int k = 0; k < 2; k++) {
        if (streams[k] < 0 || streams[k] >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
        if (!slot_ok(h, slots[k])) return fail(h, VNECT_E_ARG, "frame slot empty or out of range");
    }
    if (streams[0] == streams[1]) return fail(h, VNECT_E_ARG, "a batch takes frames of two DIFFERENT streams (a stream's frames are a chain)");
    if (units_in_flight(h) >= max_in_flight(h)) return fail(h, VNECT_E_STATE, "too many frames in flight: collect one first");
    int rc;
    for (int k = 0; k < 2; k++) {
        const auto& si = h->slots[slots[k]];
        if ((rc = squarify_params(h, si.H, si.W, &fp[k]))) return rc;
        if ((rc = check_time(h, h->streams[streams[k]], t2d[k], t3d[k]))) return rc;
        dyn[k] = slot_dyn(h, slots[k], t2d[k], t3d[k]);
    }
    const bool timed = h->profiling;
    Plan* L = pick_lane(h, timed);
    Plan* b = sibling(h->bplans, h, L);
    if ((rc = sync_geometry(b, fp[0], 0)) || (rc = sync_geometry(b, fp[1], 1))) return rc;
    // gen_input_batch of both frames inside the stem launch (as run_pre does for one frame), or the batch tensor first
    if (b->stem_mode == 2 && b->stem_frame_ok && fp[0].sq.copy && fp[1].sq.copy) {
        StemArgs a = stamped(b, b->stem, b->l_conv1, timed);
        a.from_frame = 1;
        a.dyn = dyn[0], a.frame2 = dyn[1].frame, a.stride2 = dyn[1].row_stride;
        HIPCK(h, launch_stem(a, b->st));
    } else {
        HIPCK(h, launch_pyramid_streams(b->d_fp, b->d_fp2, dyn[0], dyn[1], h->d_stabs, b->tensors[b->t_input4].d, b->S, b->el(), b->st));
        if (b->stem_mode == 2 && (rc = stem_from_batch(b, timed))) return rc;
    }
    if ((rc = launch_stack(h, b, timed))) return rc;
    const size_t half = (size_t)b->S * HM * HM * MAPC;
    const float* maps = b->tensors[b->t_out].d;
    for (int k = 0; k < 2; k++) {
        const int ring = (int)((h->seq_submit + k) % RING);
        // the filters are a chain within a stream: each member's post-processing waits for its own stream's previous frame
        if ((rc = wait_prev(h, h->streams[streams[k]], L))) return rc;
        HIPCK(h, launch_post(maps + k * half, h->mgeo, b->d_part, b->d_ticket, h->d_fb + streams[k], k ? b->d_fp2 : b->d_fp, dyn[k], h->cfg.numpy_promotion,
                             h->ring[ring].out_dev, b->st, h->h_conf_dev + ring));
        HIPCK(h, hipEventRecord(h->ring[ring].done, b->st));
    }
    for (int k = 0; k < 2; k++) {
        FrameInfo f{};
        f.stream = streams[k], f.batch = true, f.prof = (timed && k == 1) ? b : nullptr;
        commit_result(h, L, slots[k], t2d[k], t3d[k], f);
    }
    h->unit_submit++;
    return VNECT_OK;
}

// vnect_forward of 2 S images on the batched plan (parity / debug aid): the first lane's batched plan on the handle's stream
int forward_batch(vnect_handle* h, const float* batch, float* out)
{
    Plan* b = h->bplans[0];
    const long long npix = (long long)b->Snet * BOX * BOX;
    HIPCK(h, hipMemcpyAsync(h->in3, batch, npix * 3 * sizeof(float), hipMemcpyHostToDevice, h->st));
    HIPCK(h, launch_pad3to4(h->in3, b->tensors[b->t_input4].d, npix, b->el(), h->st));
    int rc = run_network(b, false);
    if (rc) return rc;
    const Tensor& t = b->tensors[b->t_out];
    HIPCK(h, hipMemcpyAsync(out, t.d, t.bytes(), hipMemcpyDeviceToHost, h->st));
    HIPCK(h, hipStreamSynchronize(h->st));
    return VNECT_OK;
}

// ---- tracking on the device (vnect_track_begin) --------------------------------------------------------------------------------------
// The stream's first crop and its geometry, built here with crop.h (what the box kernel runs on the device for every later frame).
// what vnect_track_begin refuses, before anything changes; r: the stream's first rect behind the loop's fallback
static int track_begin_check(vnect_handle* h, int stream, int H, int W, const int32_t* rect4, int r[4])
{
    if (stream < 0 || stream >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
    if (h->sharded) return fail(h, VNECT_E_ARG, "vnect_track_begin: tracking on a pyramid-sharded handle is not supported");
    if (!h->bplans.empty()) return fail(h, VNECT_E_ARG, "vnect_track_begin: tracking on a handle with the two-stream batch is not supported");
    if (H < 1 || W < 1 || H > 65532 || (size_t)H * W * 3 > (size_t)h->cfg.max_frame_bytes)
        return fail(h, VNECT_E_ARG, "vnect_track_begin: frame size out of range (1 .. 65532 rows, at most max_frame_bytes)");
    if (h->streams[stream].seq >= (long long)h->seq_collect) return fail(h, VNECT_E_STATE, "vnect_track_begin: frames of this stream in flight");
    r[0] = 0, r[1] = 0, r[2] = W, r[3] = H;
    if (rect4) {
        for (int k = 0; k < 4; k++) r[k] = rect4[k];
        box_fallback(W, H, r);  // runner.track applies its fallback to the initial rect as well
        if (r[0] < 0 || r[1] < 0 || r[0] >= W || r[1] >= H)
            return fail(h, VNECT_E_ARG, "vnect_track_begin: the rect's origin must lie inside the frame");
    }
    return VNECT_OK;
}

int track_begin_impl(vnect_handle* h, int stream, int H, int W, const int32_t* rect4)
{
    int r[4];
    int rc0 = track_begin_check(h, stream, H, W, rect4, r);
    if (rc0) return rc0;
    Stream& sm = h->streams[stream];
    // a rect past the frame's far edges crops what numpy slicing crops (frame[y:y + h, x:x + w]) and is reported as given
    std::vector<TrackState> ts(1);
    memset(&ts[0], 0, sizeof(TrackState));
    TrackState& t = ts[0];
    t.x = r[0], t.y = r[1], t.w = std::min(r[2], W - r[0]), t.h = std::min(r[3], H - r[1]), t.uw = r[2], t.uh = r[3], t.H = H, t.W = W;
    t.status = crop_squarify(t.h, t.w, &t.fp);
    t.fail = t.status != SQ_OK ? 1u : 0u;  // (the first tracked frame is number 1)
    const size_t need = (size_t)H * W * 3 + 16;
    if (sm.track_cap < need) {  // the crop buffer of pinned frames (the largest crop is the frame)
        for (Plan* l : h->lanes) HIPCK(h, hipStreamSynchronize(l->st));
        int rc = dev_grow(h, &sm.track_buf, &sm.track_cap, need);
        if (rc) return rc;
    }
    // vnect_track_redetect is set on the stream: its level table and workspace for this size and orientation, now that they are known --
    // the last step that can refuse, so a refused vnect_track_begin leaves the stream's track and its detection plan as they were
    if (sm.rd_on) {
        int rc = redetect_prepare(h, stream, H, W, h->orient);
        if (rc) return rc;
    }
    HIPCK(h, hipMemcpyAsync(h->d_track + stream, &t, sizeof(TrackState), hipMemcpyHostToDevice, h->st));
    HIPCK(h, hipStreamSynchronize(h->st));
    sm.track_on = true, sm.track_stopped = false, sm.track_H = H, sm.track_W = W, sm.track_seq = 1, sm.orient = h->orient;
    return VNECT_OK;
}

// ---- people mode (vnect_set_people; PEOPLE.md): P persons of ONE video, person p on stream p, one submit per frame -------------------------
// No reference counterpart: hog_box.py:26-31 keeps the biggest rectangle and run_estimator_ps.py:80-109 follows that one person.  Each person's
// loop is that loop, on the device as for any tracked stream; what is new is that the persons of a frame go out together, two of them through
// ONE conv stack where the handle has the pair plan, and that the frame is drawn into only after every person's pyramid has read it.
int people_begin_impl(vnect_handle* h, int n, int H, int W, const int32_t* rects)
{
    int r[4], rc;
    for (int p = 0; p < n; p++)  // all or nothing: every stream's refusals first
        if ((rc = track_begin_check(h, p, H, W, rects ? rects + 4 * p : nullptr, r))) return rc;
    for (int p = 0; p < n; p++)
        if ((rc = track_begin_impl(h, p, H, W, rects ? rects + 4 * p : nullptr))) return rc;  // (only a HIP error can still stop it)
    return VNECT_OK;
}

// A paired unit: persons s0 and s0 + 1 of one frame on one lane's pair plan -- both crops' pyramids in one launch, the conv stack once for
// 2 S images, then each person's post-processing + box stage on its own half of the maps, with its own filter bank, state, rule and ring
// slot.  The caller (enqueue_people) has checked everything that can refuse.
// The pair plan is post_merged like every batched plan, and the box stage is always the tail of post_kernel (launch_post_track): the A/B
// switches of a single tracked frame -- VNECT_TRACK_BOX_LAUNCH, VNECT_NO_POST_MERGE -- and the test build's vnect_test_maps_override do NOT
// apply to paired units (single units of a people frame go through enqueue_frame and honour them).
static int enqueue_pair(vnect_handle* h, int s0, int slot, double t2d, double t3d, const FrameSrc& src)
{
    const bool from_slot = src.where == SRC_SLOT;
    const bool timed = h->profiling;
    Plan* L = pick_lane(h, timed);
    Plan* b = sibling(h->pplans, h, L);
    FrameDyn dyn[2];
    int rc;
    for (int k = 0; k < 2; k++) {
        // a person's crop is its previous frame's box stage's output: everything of the unit waits for both persons' previous frames
        if ((rc = wait_prev(h, h->streams[s0 + k], L))) return rc;
        dyn[k] = tracked_dyn(h, s0 + k, from_slot, slot, t2d, t3d);
    }
    if ((rc = wait_for_producer(h, src.producer, L->st))) return rc;
    for (int k = 0; k < 2; k++)
        if ((rc = copy_tracked_crop(h, s0 + k, src, L->st))) return rc;
    HIPCK(h, launch_pyramid_track_pair(h->d_track + s0, dyn[0], dyn[1], !from_slot, h->d_stabs, b->tensors[b->t_input4].d, b->S, b->el(), b->st));
    // (the stem from the batch tensor: the host does not know whether a crop's squarify step is a copy)
    if (b->stem_mode == 2 && (rc = stem_from_batch(b, timed))) return rc;
    if ((rc = launch_stack(h, b, timed))) return rc;
    const size_t half = (size_t)b->S * HM * HM * MAPC;
    const float* maps = b->tensors[b->t_out].d;
    for (int k = 0; k < 2; k++) {
        const int s = s0 + k, ring = (int)((h->seq_submit + k) % RING);
        HIPCK(h, launch_post_track(maps + k * half, h->mgeo, b->d_part, b->d_ticket, h->d_fb + s, h->d_track + s, dyn[k], h->cfg.numpy_promotion,
                                   h->ring[ring].out_dev, h->h_tout_dev + ring, b->st, h->h_conf_dev + ring, h->d_policy + s, nullptr));
        if (h->streams[s].v3_on && (rc = view3d_tail(h, h->streams[s], ring, b->st))) return rc;
        HIPCK(h, hipEventRecord(h->ring[ring].done, b->st));
    }
    for (int k = 0; k < 2; k++) {
        const Stream& sm = h->streams[s0 + k];
        FrameInfo f{};
        f.stream = s0 + k, f.batch = true, f.prof = (timed && k == 1) ? b : nullptr, f.tracked = true;
        if (sm.v3_on) f.v3_h = sm.v3.rows, f.v3_w = sm.v3.cols;
        commit_result(h, L, slot, t2d, t3d, f);
    }
    h->unit_submit++;
    return VNECT_OK;
}

int enqueue_people(vnect_handle* h, int n, int slot, double t2d, double t3d, const FrameSrc& src)
{
    const bool from_slot = src.where == SRC_SLOT;
    int rc;
    if (from_slot && !slot_ok(h, slot)) return fail(h, VNECT_E_ARG, "frame slot empty or out of range");
    // atomic: every refusal of every person before anything changes
    for (int p = 0; p < n; p++) {
        const Stream& sm = h->streams[p];
        if (!sm.track_on) return fail(h, VNECT_E_STATE, "person " + std::to_string(p) + " is not tracking: call vnect_people_begin first");
        if (sm.track_stopped)
            return fail(h, VNECT_E_STATE, "tracking of person " + std::to_string(p) + " stopped at a refused crop: call vnect_people_begin");
        const int fH = from_slot ? h->slots[slot].H : (src.orient & 1) ? src.W : src.H, fW = from_slot ? h->slots[slot].W : (src.orient & 1) ? src.H : src.W;
        if (fH != sm.track_H || fW != sm.track_W || (!from_slot && sm.orient != src.orient))
            return fail(h, VNECT_E_ARG, "the frame is not of the size (and orientation) vnect_people_begin gave for person " + std::to_string(p));
        if ((rc = check_time(h, sm, t2d, t3d))) return rc;
    }
    const bool pair = !h->pplans.empty();
    const int units = pair ? (n + 1) / 2 : n;
    // (one people frame is always accepted when nothing is in flight: four persons run singly are four units, on any handle)
    if (units_in_flight(h) && units_in_flight(h) + (unsigned long long)units > max_in_flight(h))
        return fail(h, VNECT_E_STATE, "too many frames in flight for this people frame's units: collect first");
    if (h->seq_submit - h->seq_collect + (unsigned long long)n > (unsigned long long)RING)
        return fail(h, VNECT_E_STATE, "too many results in flight for this people frame: collect first");
    const unsigned long long seq0 = h->seq_submit;
    FrameSrc one = src;  // a single unit is the tracked frame as it is today, but for drawing: that waits for every person's pyramid
    one.draw = one.preview = false, one.people_unit = true;
    int paired = 0;
    for (int p = 0; p < n;) {
        if (pair && p + 1 < n) {
            if ((rc = enqueue_pair(h, p, slot, t2d, t3d, src))) return rc;
            p += 2, paired++;
        } else {
            int ring;
            if ((rc = enqueue_frame(h, slot, t2d, t3d, &ring, p, &one))) return rc;
            p += 1;
        }
    }
    h->last_people_units = pair ? units : n, h->last_people_paired = paired;
    if (!src.draw && !src.preview) return VNECT_OK;
    // run_estimator_ps.py:92-94 once per person, in person order, behind EVERY unit's joints: nothing writes the frame before every
    // person's pyramid (or crop copy) has read it.  The last person's `done` is recorded again behind the drawing, so the frame is the
    // caller's again when that person has been collected.
    Plan* last = h->streams[n - 1].lane;
    for (int p = 0; p + 1 < n; p++)
        if (h->streams[p].lane != last) HIPCK(h, hipStreamWaitEvent(last->st, h->ring[(seq0 + p) % RING].done, 0));
    // run_estimator_ps.py:94-96 for everybody at once: the ONE picture of the frame (preview.h: PreviewPeople), first, so that it reads the
    // clean frame; it belongs to the LAST person's delivery (vnect_result_preview)
    if (src.preview) {
        const int ring = (int)((seq0 + n - 1) % RING);
        const PreviewArgs a = preview_into(h, src.pv, ring);
        PreviewPeopleIn pin{};
        pin.P = n;
        for (int p = 0; p < n; p++) {
            const int rp = (int)((seq0 + p) % RING);
            pin.jo[p] = h->ring[rp].out_dev, pin.to[p] = h->h_tout_dev + rp, pin.co[p] = src.pv_in.has_conf ? h->h_conf_dev + rp : nullptr;
        }
        HIPCK(h, launch_preview_people(a, src.pv_in, pin, last->st));
        if ((rc = preview_copy(h, a, ring, last->st))) return rc;
        h->ring[ring].f.pv_h = a.g.dh, h->ring[ring].f.pv_w = a.g.dw;  // (after the fact: the last person's unit was committed without it)
    }
    for (int p = 0; src.draw && p < n; p++) {
        const int ring = (int)((seq0 + p) % RING);
        HIPCK(h, launch_overlay(src.draw_target, src.draw_in, h->ring[ring].out_dev, h->h_tout_dev + ring, src.draw_in.has_conf ? h->h_conf_dev + ring : nullptr,
                                last->st));
    }
    HIPCK(h, hipEventRecord(h->ring[(seq0 + n - 1) % RING].done, last->st));
    return VNECT_OK;
}

}  // namespace rt
}  // namespace vnect
