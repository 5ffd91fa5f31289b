// rt_abi.cpp -- the extern "C" entry points of include/vnect_abi.h (which cites the reference lines each one replaces): argument and
// state checks, device selection, and the guard that lets no C++ exception cross the boundary.  The work is in rt_plan / rt_exec / rt_ingest / rt_comm.
#include "runtime.h"

namespace vnect {
namespace rt {
thread_local std::string g_create_error = "";
}  // namespace rt
}  // namespace vnect

// gen_input_batch of the frame in slot 0 (vnect_preprocess, vnect_preprocess_nv12)
static int preprocess_slot0(vnect_handle* h, float* batch_out, double* scaler, int32_t* offset_x, int32_t* offset_y)
{
    FrameParams fp;
    int rc;
    if ((rc = squarify_params(h, h->slots[0].H, h->slots[0].W, &fp))) return rc;
    if ((rc = sync_geometry(h, fp))) return rc;
    if ((rc = run_pre(h, slot_dyn(h, 0, 0.0, 0.0), false, true))) return rc;
    if (batch_out) {
        const long long npix = (long long)h->Snet * BOX * BOX;
        HIPCK(h, launch_strip4to3(h->tensors[h->t_input4].d, h->in3, npix, h->el(), h->st));
        HIPCK(h, hipMemcpyAsync(batch_out, h->in3, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, h->st));
    }
    HIPCK(h, hipStreamSynchronize(h->st));
    if (scaler) *scaler = fp.scaler;
    if (offset_x) *offset_x = fp.offx;
    if (offset_y) *offset_y = fp.offy;
    return VNECT_OK;
}

// ---- The four operations a frame source takes part in: upload, infer, preprocess, tracked submit.  `resolve(FrameSrc*)` is the source's
// resolver (rt_ingest.cpp) over the entry point's arguments.  The order everywhere: state, then the source's validation, then what changes
// state.
// finalized (or, where that serves, preprocess_only), nothing in flight; selects the device
static int idle(vnect_handle* h, const char* who, bool pre_only_serves)
{
    if (!h->finalized && !(pre_only_serves && h->pre_only)) return fail(h, VNECT_E_STATE, std::string(who) + " before vnect_finalize");
    if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
    HIPCK(h, hipSetDevice(h->cfg.device));
    return VNECT_OK;
}

static int tracked_ok(vnect_handle* h, int stream)
{
    if (!h->finalized) return fail(h, VNECT_E_STATE, "inference before vnect_finalize");
    if (stream < 0 || stream >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
    if (!h->streams[stream].track_on) return fail(h, VNECT_E_STATE, "stream is not tracking: call vnect_track_begin first");
    if (h->streams[stream].track_stopped) return fail(h, VNECT_E_STATE, "tracking of this stream stopped at a refused crop: call vnect_track_begin");
    return VNECT_OK;
}

// the size of the frames a tracked stream is given, as they are STORED: vnect_track_begin's (H, W) is the oriented picture's
static int stored_H(const Stream& sm) { return (sm.orient & 1) ? sm.track_W : sm.track_H; }
static int stored_W(const Stream& sm) { return (sm.orient & 1) ? sm.track_H : sm.track_W; }

// the frame into `slot`; done with the caller's buffer on return
template <class R>
static int upload_from(vnect_handle* h, int slot, const char* who, R&& resolve)
{
    if (slot < 0 || slot >= (int)h->slots.size()) return fail(h, VNECT_E_ARG, std::string(who) + ": bad frame slot");
    HIPCK(h, hipSetDevice(h->cfg.device));
    FrameSrc src;
    int rc = resolve(&src);
    return rc ? rc : ingest_sync(h, slot, src);
}

// the frame through slot 0, synchronously.  Nothing is in flight, so the frame will run on the first lane's stream (enqueue_frame), the
// stream ingest() copies on; the result is back when this returns, so the copy has long read the caller's buffer
template <class R>
static int infer_from(vnect_handle* h, const char* who, double t2d, double t3d, double* j2, float* j3, R&& resolve)
{
    int rc = idle(h, who, false);
    if (rc) return rc;
    FrameSrc src;
    if ((rc = resolve(&src))) return rc;
    if ((rc = ingest(h, 0, src))) return rc;
    return vnect_infer_resident(h, 0, t2d, t3d, j2, j3);
}

template <class R>
static int preprocess_from(vnect_handle* h, const char* who, float* batch_out, double* scaler, int32_t* offset_x, int32_t* offset_y, R&& resolve)
{
    int rc = idle(h, who, true);
    if (rc) return rc;
    FrameSrc src;
    if ((rc = resolve(&src))) return rc;
    if ((rc = ingest_sync(h, 0, src))) return rc;
    return preprocess_slot0(h, batch_out, scaler, offset_x, offset_y);
}

// the stream's next tracked frame: the whole frame in `slot`, or (slot -1) where the resolver says
// whole_on_device: the submit form leaves the whole frame in device memory in a layout HogSrc describes -- what a stream that re-detects
// (vnect_track_redetect) needs of every frame
template <class R>
static int submit_tracked_from(vnect_handle* h, int stream, int slot, double t2d, double t3d, R&& resolve, bool whole_on_device = false)
{
    int rc = tracked_ok(h, stream);
    if (rc) return rc;
    if (h->streams[stream].rd_on && !whole_on_device)
        return fail(h, VNECT_E_ARG, "vnect_track_redetect is set on this stream: its frames come through vnect_submit_tracked_device, _device_draw or "
                                    "_device_preview (the detector reads the whole frame in device memory)");
    HIPCK(h, hipSetDevice(h->cfg.device));
    FrameSrc src;
    if ((rc = resolve(&src))) return rc;
    int ring;
    return enqueue_frame(h, slot, t2d, t3d, &ring, stream, &src);
}

// =====================================================================================================
extern "C" {

int vnect_abi_version(void) { return VNECT_ABI_VERSION; }

#ifndef VNECT_BUILD_FLAGS
#define VNECT_BUILD_FLAGS "?"
#endif
#ifndef VNECT_BUILD_VARIANT
#define VNECT_BUILD_VARIANT ""
#endif
#ifndef VNECT_TEST_HOOKS
#define VNECT_TEST_HOOKS 0
#endif
const char* vnect_build_info(void)
{
    static const std::string info = [] {
        std::string s = "abi=" + std::to_string(VNECT_ABI_VERSION) + "; compiler=" + __VERSION__ + "; flags=" VNECT_BUILD_FLAGS + "; variant=" VNECT_BUILD_VARIANT +
                        "; test_hooks=" + std::to_string((int)VNECT_TEST_HOOKS) + "; conv: " + conv_build_probes() + "; post: " + post_build_probes() +
                        "; probes_off=" + ((conv_probes_off() && post_probes_off()) ? "1" : "0");
        return s;
    }();
    return info.c_str();
}

const char* vnect_last_error(vnect_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int vnect_create(const vnect_config* cfg, vnect_handle** out)
{
    if (out) *out = nullptr;  // the guard below reports on *out once the handle exists
    return guarded(out, [&]() -> int {
        if (!cfg || !out || cfg->struct_size != (int32_t)sizeof(vnect_config))
            return fail(nullptr, VNECT_E_ARG, "vnect_create: bad config (struct_size mismatch)");
        if (cfg->num_scales < 1 || cfg->num_scales > VNECT_MAX_SCALES)
            return fail(nullptr, VNECT_E_ARG, "vnect_create: num_scales out of range");
        if (cfg->precision != VNECT_FP32 && cfg->precision != VNECT_BF16 && cfg->precision != VNECT_FP32_SPLIT && cfg->precision != VNECT_FP16)
            return fail(nullptr, VNECT_E_ARG, "vnect_create: precision must be VNECT_FP32, VNECT_BF16, VNECT_FP32_SPLIT or VNECT_FP16");
        if (cfg->lanes < 0 || cfg->lanes > MAX_LANES)
            return fail(nullptr, VNECT_E_ARG, "vnect_create: lanes must be 0 .. 3");
        if (cfg->exchange != VNECT_XCHG_RCCL && cfg->exchange != VNECT_XCHG_P2P)
            return fail(nullptr, VNECT_E_ARG, "vnect_create: exchange must be VNECT_XCHG_RCCL or VNECT_XCHG_P2P");
        if (cfg->preprocess_only && cfg->pyramid_nranks > 0)
            return fail(nullptr, VNECT_E_ARG, "vnect_create: preprocess_only and pyramid sharding exclude each other");
        roctx_load();
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || cfg->device < 0 || cfg->device >= ndev)
            return fail(nullptr, VNECT_E_NODEVICE, "vnect_create: no HIP device " + std::to_string(cfg->device));
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || !strstr(prop.gcnArchName, "gfx950"))
            return fail(nullptr, VNECT_E_NODEVICE, "vnect_create: device is not gfx950 (MI355X); kernels are built for gfx950 only");
        const bool sharded = cfg->pyramid_nranks > 1 || (cfg->pyramid_nranks == 1 && cfg->num_scales == 1);
        if (sharded && (cfg->pyramid_nranks != cfg->num_scales || cfg->pyramid_rank < 0 || cfg->pyramid_rank >= cfg->pyramid_nranks))
            return fail(nullptr, VNECT_E_ARG, "vnect_create: pyramid sharding needs pyramid_nranks == num_scales and 0 <= pyramid_rank < nranks");
        vnect_handle* h = new vnect_handle();
        h->owner = h, h->lanes = {h}, h->owns_stream = true, h->prof_graph = true;  // lane 0
        h->cfg = *cfg;
        h->S = cfg->num_scales;
        h->Snet = sharded ? 1 : cfg->num_scales;
        h->bf16 = cfg->precision == VNECT_BF16 || cfg->precision == VNECT_FP16;  // 16-bit elements: the bf16 plan
        h->f16 = cfg->precision == VNECT_FP16;
        h->x3 = cfg->precision == VNECT_FP32_SPLIT;
        h->sharded = sharded;
        h->keep_activations = cfg->keep_activations != 0;
        const bool pre = cfg->preprocess_only != 0;
        h->pre_only = pre;
        if (h->cfg.max_frame_bytes <= 0) h->cfg.max_frame_bytes = 4096 * 4096 * 3;
        if (h->cfg.max_frame_bytes < INT32_MAX - 16) h->cfg.max_frame_bytes = (h->cfg.max_frame_bytes + 15) & ~15;  // slots start 16-byte aligned (the stem reads frame rows as aligned dwords)
        if (h->cfg.num_frame_slots <= 0) h->cfg.num_frame_slots = 4;
        // gen_input_batch alone (the static method creates and destroys such a handle per call): ONE frame slot that grows with the
        // frames it is given (upload_frame_impl), no gather buffer, no filter bank, no profiling buffers -- the resize tables and the
        // (S,368,368) batch + its read-back staging are all it owns (~20 MB at S = 3)
        if (pre) h->cfg.num_frame_slots = 1;
        *out = h;  // returned even on failure below so the caller can read the message, then destroy
        HIPCK(h, hipSetDevice(cfg->device));
        HIPCK(h, hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
        HIPCK(h, conv_setup());
        HIPCK(h, stem_setup());
        h->slots.resize(h->cfg.num_frame_slots);
        int rc;
        if (!pre && (rc = dev_alloc(h, &h->frames, (size_t)h->cfg.num_frame_slots * h->cfg.max_frame_bytes + 16))) return rc;  // + slack: a dword read may run 3 bytes past a frame's last pixel
        if ((rc = dev_alloc(h, &h->d_fp, 1))) return rc;
        if ((rc = dev_alloc(h, &h->d_stabs, 1))) return rc;
        if ((rc = dev_alloc(h, &h->d_part, (size_t)NJ * ARG_SLABS_MAX))) return rc;
        if ((rc = dev_alloc(h, &h->d_ticket, 4))) return rc;
        HIPCK(h, hipMemset(h->d_ticket, 0, 4 * sizeof(unsigned)));
        h->post_merged = getenv("VNECT_NO_POST_MERGE") == nullptr;
        if (!pre && (rc = dev_alloc(h, &h->d_fb, VNECT_MAX_STREAMS))) return rc;
        if (!pre && (rc = dev_alloc(h, &h->d_track, VNECT_MAX_STREAMS))) return rc;
        if (!pre) {
            HIPCK(h, hipHostMalloc((void**)&h->h_tout, RING * sizeof(TrackOut), hipHostMallocMapped | hipHostMallocCoherent));
            memset(h->h_tout, 0, RING * sizeof(TrackOut));
            HIPCK(h, hipHostGetDevicePointer((void**)&h->h_tout_dev, h->h_tout, 0));
            HIPCK(h, hipHostMalloc((void**)&h->h_conf, RING * sizeof(ConfOut), hipHostMallocMapped | hipHostMallocCoherent));
            memset(h->h_conf, 0, RING * sizeof(ConfOut));
            HIPCK(h, hipHostGetDevicePointer((void**)&h->h_conf_dev, h->h_conf, 0));
            if ((rc = dev_alloc(h, &h->d_conf, (size_t)VNECT_MAX_STREAMS * NJ))) return rc;
            if ((rc = dev_alloc(h, &h->d_policy, VNECT_MAX_STREAMS))) return rc;
            std::vector<TrackPolicy> off(VNECT_MAX_STREAMS, TrackPolicy{0.0, 1, TRACK_LOST_OFF});
            HIPCK(h, hipMemcpy(h->d_policy, off.data(), off.size() * sizeof(TrackPolicy), hipMemcpyHostToDevice));
        }
        if ((rc = dev_alloc(h, &h->in3, (size_t)(pre ? h->Snet : VNECT_MAX_SCALES) * BOX * BOX * 3))) return rc;
        if (!pre && (rc = dev_alloc(h, &h->gather, (size_t)VNECT_MAX_SCALES * HM * HM * MAPC))) return rc;
        for (int i = 0; i < RING; i++) {
            HIPCK(h, hipHostMalloc((void**)&h->h_fp[i], sizeof(FrameParams), hipHostMallocDefault));
            HIPCK(h, hipHostMalloc((void**)&h->ring[i].out, sizeof(JointsOut), hipHostMallocMapped | hipHostMallocCoherent));
            HIPCK(h, hipHostGetDevicePointer((void**)&h->ring[i].out_dev, h->ring[i].out, 0));
            HIPCK(h, hipEventCreateWithFlags(&h->ring[i].done, hipEventDisableTiming));
        }
        if (sharded && cfg->exchange == VNECT_XCHG_P2P) {
            // fine-grained device memory: peers' stores and the system-scope loads of this device bypass its L2, so a slot is
            // never served from a line cached two frames ago.  The protocol DEPENDS on it (exchange_kernel polls flags and reads slots
            // that a peer writes over xGMI): no silent fall-back to coarse-grained memory, whose stale flags / slots would
            // time out or -- worse -- merge old maps.
            void* q = nullptr;
            hipError_t e = hipExtMallocWithFlags(&q, XCHG_BYTES, hipDeviceMallocFinegrained);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, VNECT_E_COMM, std::string("exchange = VNECT_XCHG_P2P needs fine-grained device memory "
                                                         "(hipExtMallocWithFlags(hipDeviceMallocFinegrained): ") +
                                                 hipGetErrorString(e) + "); use VNECT_XCHG_RCCL");
            }
            h->dev_allocs.push_back(q);
            h->xblock = (char*)q;
            HIPCK(h, hipMemset(h->xblock, 0, XCHG_BYTES));
            if ((rc = dev_alloc(h, &h->xtickets, 8))) return rc;
            HIPCK(h, hipMemset(h->xtickets, 0, 8 * sizeof(unsigned)));
            HIPCK(h, hipHostMalloc((void**)&h->h_xstatus, RING * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
            for (int i = 0; i < RING; i++) h->h_xstatus[i] = 0;
            if ((rc = dev_alloc(h, &h->d_xfail, 4))) return rc;
            HIPCK(h, hipMemset(h->d_xfail, 0, 4 * sizeof(unsigned)));
            HIPCK(h, hipHostGetDevicePointer((void**)&h->h_xstatus_dev, h->h_xstatus, 0));
            h->xpeer[cfg->pyramid_rank] = h->xblock;
        }
        HIPCK(h, hipHostMalloc((void**)&h->h_filt, 128 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCK(h, hipHostGetDevicePointer((void**)&h->h_filt_dev, h->h_filt, 0));
        for (auto& e : h->ev) HIPCK(h, hipEventCreate(&e));
        if (!pre) {
            if ((rc = dev_alloc(h, &h->d_prof, PROF_SLOTS * 128))) return rc;
            if ((rc = dev_alloc(h, &h->d_prof_end, (size_t)PROF_WGS * 128))) return rc;
            HIPCK(h, hipMemset(h->d_prof_end, 0, (size_t)PROF_WGS * 128 * sizeof(unsigned long long)));
            HIPCK(h, hipHostMalloc((void**)&h->h_prof_end, (size_t)PROF_WGS * 128 * sizeof(unsigned long long), hipHostMallocDefault));
            HIPCK(h, hipHostMalloc((void**)&h->h_prof, PROF_SLOTS * 128 * sizeof(unsigned long long), hipHostMallocDefault));
            for (int i = 0; i < PROF_SLOTS * 128; i++) h->h_prof[i] = 0;
        }
        if ((rc = build_scale_tables(h))) return rc;
        if ((rc = build_up_table(h))) return rc;
        if (!pre && (rc = reset_filters_impl(h))) return rc;
        h->tim.struct_size = sizeof(vnect_timings);
        if (pre) {
            // gen_input_batch alone (the reference's static method needs no session either, estimator.py:70-81): the input
            // batch buffer and the tables made above; no weights, no launch plan, vnect_finalize is refused
            h->t_input4 = add_tensor(h, "input", h->Snet, BOX, BOX, 3, 4);
            Tensor& t = h->tensors[h->t_input4];
            char* p = nullptr;
            if ((rc = dev_alloc(h, &p, t.bytes() + 256))) return rc;
            t.d = (float*)p;
        }
        return VNECT_OK;
    });
}

void vnect_destroy(vnect_handle* h)
{
    if (!h) return;
    hipSetDevice(h->cfg.device);
    if (h->st) hipStreamSynchronize(h->st);
    destroy_plans(h);  // (batched plans first: they run on the lanes' streams)
    comm_destroy(h);
    for (InFlight& e : h->ring) {
        if (e.out) hipHostFree(e.out);
        if (e.done) hipEventDestroy(e.done);
    }
    for (auto& e : h->ev)
        if (e) hipEventDestroy(e);
    for (int r = 0; r < VNECT_MAX_SCALES; r++)
        if (h->xopened[r] && h->xpeer[r]) hipIpcCloseMemHandle(h->xpeer[r]);
    if (h->h_xstatus) hipHostFree(h->h_xstatus);
    if (h->h_tout) hipHostFree(h->h_tout);
    ring_pictures_free_host(h->previews);
    ring_pictures_free_host(h->views);
    if (h->h_conf) hipHostFree(h->h_conf);
    if (h->h_redet) hipHostFree(h->h_redet);
    for (int i = 0; i < 3; i++)
        if (h->stage[i]) hipHostFree(h->stage[i]);
    if (h->h_filt) hipHostFree(h->h_filt);
    if (h->upload_st) hipStreamDestroy(h->upload_st);
    if (h->producer_ev) hipEventDestroy(h->producer_ev);
#if VNECT_TEST_HOOKS
    if (h->test_st) hipStreamDestroy(h->test_st);
#endif
    destroy_plan(h);  // lane 0: its graphs, buffers (every device allocation of the handle is on its list) and stream
    delete h;
}

int vnect_set_weight(vnect_handle* h, const char* name, const float* data, const int64_t* shape, int ndim)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!name || !data || !shape || ndim < 1 || ndim > 4) return fail(h, VNECT_E_ARG, "vnect_set_weight: bad argument");
        if (h->finalized) return fail(h, VNECT_E_STATE, "vnect_set_weight after vnect_finalize");
        HostArray a;
        size_t n = 1;
        for (int i = 0; i < ndim; i++) {
            if (shape[i] < 1) return fail(h, VNECT_E_ARG, "vnect_set_weight: bad shape");
            a.shape.push_back(shape[i]);
            n *= (size_t)shape[i];
        }
        a.d.assign(data, data + n);
        h->weights[name] = std::move(a);
        return VNECT_OK;
    });
}

int vnect_finalize(vnect_handle* h)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (h->finalized) return fail(h, VNECT_E_STATE, "already finalized");
        if (h->pre_only) return fail(h, VNECT_E_STATE, "vnect_finalize on a preprocess_only handle");
        if (h->f16) {  // an fp16 handle holds its conv weights as fp16: one that rounds to infinity would poison every frame
            for (const auto& kv : h->weights) {
                const std::string& n = kv.first;
                const bool conv_w = n.size() > 8 && (n.compare(n.size() - 8, 8, "/weights") == 0 || n.compare(n.size() - 7, 7, "/kernel") == 0);
                const long long i = conv_w ? plan::first_f16_overflow(kv.second.d.data(), kv.second.d.size()) : -1;
                if (i >= 0)
                    return fail(h, VNECT_E_ARG, "vnect_finalize: weight " + n + " element " + std::to_string(i) + " = " +
                                                    std::to_string(kv.second.d[i]) + " is outside the fp16 range (|w| < 65520) of a VNECT_FP16 handle");
            }
        }
        HIPCK(h, hipSetDevice(h->cfg.device));
        int rc = finalize_impl(h);
        if (rc) {
            if (h->err.empty()) h->err = "finalize failed";
            return rc;
        }
        rc = build_graph(h);
        if (rc) return rc;
        rc = build_plans(h);
        if (rc) return rc;
        HIPCK(h, hipStreamSynchronize(h->st));
        h->finalized = true;
        h->weights.clear();
        return prime(h);
    });
}

int vnect_set_scales(vnect_handle* h, const double* scales, int n)
{
    return guarded(&h, [&]() -> int {
        if (!h || !scales) return VNECT_E_ARG;
        if (n != h->S) return fail(h, VNECT_E_ARG, "vnect_set_scales: the number of scales is fixed at create time");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        HIPCK(h, hipSetDevice(h->cfg.device));
        for (Plan* l : h->lanes) HIPCK(h, hipStreamSynchronize(l->st));
        double old[VNECT_MAX_SCALES];
        memcpy(old, h->cfg.scales, sizeof old);
        for (int i = 0; i < n; i++) h->cfg.scales[i] = scales[i];
        int rc = build_scale_tables(h);
        if (rc) {
            memcpy(h->cfg.scales, old, sizeof old);
            build_scale_tables(h);
        }
        // the two-launch form of the post-processing (VNECT_NO_POST_MERGE=1) has its arg-max launch -- and with it the merge geometry,
        // a by-value kernel argument -- inside the captured graph: capture again (the default form launches post_kernel eagerly)
        if (h->finalized && !h->sharded && !h->post_merged && h->gexec) {
            int rg = VNECT_OK;
            for (size_t i = 0; i < h->lanes.size() && !rg; i++) rg = build_graph(h->lanes[i]);
            if (rg) return rg;
        }
        return rc;
    });
}

int vnect_forward(vnect_handle* h, const float* batch, int num_images, float* out)
{
    return guarded(&h, [&]() -> int {
        if (!h || !batch || !out) return VNECT_E_ARG;
        if (!h->finalized) return fail(h, VNECT_E_STATE, "vnect_forward before vnect_finalize");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        const bool doubled = !h->bplans.empty() && num_images == 2 * h->Snet;
        if (num_images != h->Snet && !doubled)
            return fail(h, VNECT_E_ARG, "vnect_forward: num_images must equal num_scales (1 on a pyramid-sharded handle; "
                                        "or 2 x num_scales after vnect_set_stream_batch(h, 2))");
        HIPCK(h, hipSetDevice(h->cfg.device));
        if (doubled) return forward_batch(h, batch, out);
        const long long npix = (long long)h->Snet * BOX * BOX;
        HIPCK(h, hipMemcpyAsync(h->in3, batch, npix * 3 * sizeof(float), hipMemcpyHostToDevice, h->st));
        HIPCK(h, launch_pad3to4(h->in3, h->tensors[h->t_input4].d, npix, h->el(), h->st));
        int rc = run_network(h, false);
        if (rc) return rc;
        const Tensor& t = h->tensors[h->t_out];
        HIPCK(h, hipMemcpyAsync(out, t.d, t.bytes(), hipMemcpyDeviceToHost, h->st));
        HIPCK(h, hipStreamSynchronize(h->st));
        return VNECT_OK;
    });
}

int vnect_preprocess(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, float* batch_out,
                     double* scaler, int32_t* offset_x, int32_t* offset_y)
{
    return guarded(&h, [&]() -> int {
        if (!h || !bgr) return VNECT_E_ARG;
        int rc = idle(h, "vnect_preprocess", true);
        if (rc) return rc;
        if ((rc = upload_frame_impl(h, 0, bgr, H, W, row_stride))) return rc;  // (the pageable, synchronous copy: rt_ingest.cpp)
        return preprocess_slot0(h, batch_out, scaler, offset_x, offset_y);
    });
}

int vnect_postprocess(vnect_handle* h, const float* maps, double t2d, double t3d, double scaler, int32_t offset_x,
                      int32_t offset_y, double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h || !maps || !j2 || !j3) return VNECT_E_ARG;
        if (!h->finalized) return fail(h, VNECT_E_STATE, "vnect_postprocess before vnect_finalize");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        if (!(scaler > 0)) return fail(h, VNECT_E_ARG, "scaler must be positive");
        HIPCK(h, hipSetDevice(h->cfg.device));
        int rc = check_time(h, h->streams[0], t2d, t3d);
        if (rc) return rc;
        float* dst = h->sharded ? h->gather : h->tensors[h->t_out].d;
        HIPCK(h, hipMemcpyAsync(dst, maps, (size_t)h->S * HM * HM * MAPC * sizeof(float), hipMemcpyHostToDevice, h->st));
        FrameParams fp;
        memset(&fp, 0, sizeof fp);
        fp.scaler = scaler, fp.offx = offset_x, fp.offy = offset_y;
        FrameDyn dyn{};
        dyn.t2d = t2d, dyn.t3d = t3d;
        if ((rc = sync_geometry(h, fp))) return rc;
        if (h->post_merged) {
            if ((rc = run_post(h, dyn, h->ring[0].out_dev, h->h_conf_dev))) return rc;
        } else {
            if ((rc = run_argmax(h))) return rc;
            if ((rc = run_joints(h, dyn, h->ring[0].out_dev, h->h_conf_dev))) return rc;
        }
        commit_time(h->streams[0], t2d, t3d);
        HIPCK(h, hipStreamSynchronize(h->st));
        memcpy(j2, h->ring[0].out->j2d, sizeof(double) * NJ * 2);
        memcpy(j3, h->ring[0].out->j3d, sizeof(float) * NJ * 3);
        deliver_confidence(h, 0, false);
        return VNECT_OK;
    });
}

int vnect_frame_buffer(vnect_handle* h, int index, int64_t min_bytes, uint8_t** ptr_out)
{
    return guarded(&h, [&]() -> int {
        if (!h || !ptr_out || index < 0 || index > 1 || min_bytes < 1) return h ? fail(h, VNECT_E_ARG, "vnect_frame_buffer: bad argument") : VNECT_E_ARG;
        if (h->pre_only) return fail(h, VNECT_E_STATE, "vnect_frame_buffer on a preprocess_only handle");
        if (min_bytes > (int64_t)h->cfg.max_frame_bytes) return fail(h, VNECT_E_ARG, "vnect_frame_buffer: larger than max_frame_bytes");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        HIPCK(h, hipSetDevice(h->cfg.device));
        int rc = ensure_stage(h, index, (size_t)min_bytes);
        if (rc) return rc;
        *ptr_out = h->stage[index];
        return VNECT_OK;
    });
}

int vnect_upload_frame(vnect_handle* h, int slot, const uint8_t* bgr, int H, int W, int64_t row_stride)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return upload_frame_impl(h, slot, bgr, H, W, row_stride);
    });
}

int vnect_submit_resident(vnect_handle* h, int slot, double t2d, double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!h->finalized) return fail(h, VNECT_E_STATE, "inference before vnect_finalize");
        HIPCK(h, hipSetDevice(h->cfg.device));
        int ring;
        return enqueue_frame(h, slot, t2d, t3d, &ring);
    });
}

int vnect_submit_stream(vnect_handle* h, int stream, int slot, double t2d, double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!h->finalized) return fail(h, VNECT_E_STATE, "inference before vnect_finalize");
        HIPCK(h, hipSetDevice(h->cfg.device));
        int ring;
        return enqueue_frame(h, slot, t2d, t3d, &ring, stream);
    });
}

int vnect_collect_stream(vnect_handle* h, int32_t* stream_out, double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return collect_impl(h, j2, j3, stream_out);
    });
}

int vnect_reset_filters_stream(vnect_handle* h, int stream)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (stream < 0 || stream >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        if (h->pre_only) return fail(h, VNECT_E_STATE, "vnect_reset_filters_stream on a preprocess_only handle (it has no filter bank)");
        HIPCK(h, hipSetDevice(h->cfg.device));
        return reset_filters_impl(h, stream);
    });
}

int vnect_collect(vnect_handle* h, double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return collect_impl(h, j2, j3);
    });
}

int vnect_infer_resident(vnect_handle* h, int slot, double t2d, double t3d, double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h || !j2 || !j3) return VNECT_E_ARG;
        if (!h->finalized) return fail(h, VNECT_E_STATE, "inference before vnect_finalize");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        int rc = vnect_submit_resident(h, slot, t2d, t3d);
        if (rc) return rc;
        return collect_impl(h, j2, j3);
    });
}

int vnect_infer(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, double t2d, double t3d,
                double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h || !bgr || !j2 || !j3) return VNECT_E_ARG;
        return infer_from(h, "vnect_infer", t2d, t3d, j2, j3, [&](FrameSrc* s) { return resolve_host_bgr(h, bgr, H, W, row_stride, h->orient, s); });
    });
}

int vnect_joint_filter(vnect_handle* h, int dim, const double* joints_in, int values_are_f32, double t, double* joints_out)
{
    return guarded(&h, [&]() -> int {
        if (!h || !joints_in || !joints_out || (dim != 2 && dim != 3)) return h ? fail(h, VNECT_E_ARG, "vnect_joint_filter: bad argument") : VNECT_E_ARG;
        if (h->pre_only) return fail(h, VNECT_E_STATE, "vnect_joint_filter on a preprocess_only handle (it has no filter bank)");
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        HIPCK(h, hipSetDevice(h->cfg.device));
        // the timestamp rules of check_time, for the one bank this call advances
        TimeState& ts = h->streams[0].t;  // (stream 0: the bank vnect_infer advances)
        const bool have = dim == 2 ? ts.have2 : ts.have3;
        const double last = dim == 2 ? ts.last2 : ts.last3;
        if (have && last != 0.0 && t != 0.0) {
            if (t == last) return fail(h, VNECT_E_TIMESTAMP, "timestamp equals the previous one of this filter bank");
            if (t < last) return fail(h, VNECT_E_TIMEORDER, "timestamp is earlier than the previous one of this filter bank");
        }
        const int n = NJ * dim;
        memcpy(h->h_filt, joints_in, sizeof(double) * n);
        HIPCK(h, launch_filter(h->d_fb, dim, values_are_f32 != 0, h->cfg.numpy_promotion, t, h->h_filt_dev, h->h_filt_dev + 64, h->st));
        HIPCK(h, hipStreamSynchronize(h->st));
        if (dim == 2) ts.have2 = true, ts.last2 = t;
        else ts.have3 = true, ts.last3 = t;
        memcpy(joints_out, h->h_filt + 64, sizeof(double) * n);
        return VNECT_OK;
    });
}

int vnect_reset_filters(vnect_handle* h)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, "frames in flight");
        if (h->pre_only) return fail(h, VNECT_E_STATE, "vnect_reset_filters on a preprocess_only handle (it has no filter bank)");
        HIPCK(h, hipSetDevice(h->cfg.device));
        return reset_filters_impl(h);
    });
}

int vnect_read_activation(vnect_handle* h, const char* name, float* out, int64_t capacity, int32_t* shape4)
{
    return guarded(&h, [&]() -> int {
        if (!h || !name || !shape4) return VNECT_E_ARG;
        if (!h->finalized) return fail(h, VNECT_E_STATE, "not finalized");
        auto it = h->tensor_by_name.find(name);
        if (it == h->tensor_by_name.end()) return fail(h, VNECT_E_ARG, std::string("no activation named ") + name);
        const Tensor& t = h->tensors[it->second];
        shape4[0] = t.S, shape4[1] = t.H, shape4[2] = t.W, shape4[3] = t.C;
        if (!out) return VNECT_OK;
        if (!h->keep_activations && it->second != h->t_out)
            return fail(h, VNECT_E_STATE, "vnect_read_activation: inner layers share an arena; create the handle with keep_activations = 1");
        if (!plan_writes(h, it->second))
            return fail(h, VNECT_E_STATE, std::string("vnect_read_activation: no launch of this plan writes ") + name + " (a fused launch keeps it on chip)");
        const size_t npix = (size_t)t.S * t.H * t.W;
        if ((int64_t)(npix * t.C) > capacity) return fail(h, VNECT_E_ARG, "vnect_read_activation: capacity too small");
        HIPCK(h, hipSetDevice(h->cfg.device));
        HIPCK(h, hipStreamSynchronize(h->st));
        if (t.esz == 4) {
            HIPCK(h, hipMemcpy2D(out, (size_t)t.C * sizeof(float), t.d, (size_t)t.Cs * sizeof(float), (size_t)t.C * sizeof(float),
                                 npix, hipMemcpyDeviceToHost));
        } else {  // 16-bit activations: fetch raw, widen on the host
            std::vector<uint16_t> raw(npix * t.C);
            HIPCK(h, hipMemcpy2D(raw.data(), (size_t)t.C * 2, t.d, (size_t)t.Cs * 2, (size_t)t.C * 2, npix, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < raw.size(); i++) out[i] = h->f16 ? plan::from_f16(raw[i]) : plan::from_bf16(raw[i]);
        }
        return VNECT_OK;
    });
}

int vnect_get_layer_stamps(vnect_handle* h, int idx, uint64_t* out24)
{
    return guarded(&h, [&]() -> int {
        if (!h || !out24 || idx < 0 || idx >= (int)h->layers.size()) return h ? fail(h, VNECT_E_ARG, "bad layer index") : VNECT_E_ARG;
        for (int k = 0; k < 24; k++) out24[k] = h->h_prof[PROF_SLOTS * idx + k];
        return VNECT_OK;
    });
}

int vnect_set_profiling(vnect_handle* h, int on)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        h->profiling = on != 0;
        return VNECT_OK;
    });
}

int vnect_get_timings(vnect_handle* h, vnect_timings* out)
{
    return guarded(&h, [&]() -> int {
        // ABI v5 callers pass the struct without the shader-clock fields: they get exactly what they got before
        constexpr int32_t V5_SIZE = (int32_t)offsetof(vnect_timings, shader_cycles);
        if (!h || !out || (out->struct_size != (int32_t)sizeof(vnect_timings) && out->struct_size != V5_SIZE)) return VNECT_E_ARG;
        const int32_t sz = out->struct_size;
        vnect_timings t = h->tim;
        t.struct_size = sz;
        t.conv_launches = h->conv_launches;
        t.conv_flops = h->conv_flops;
        memcpy(out, &t, (size_t)sz);
        return VNECT_OK;
    });
}

int vnect_reset_timings(vnect_handle* h)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        memset(&h->tim, 0, sizeof h->tim);
        h->tim.struct_size = sizeof(vnect_timings);
        return VNECT_OK;
    });
}

static int layer_info(const std::vector<Layer>& layers, int idx, vnect_layer_info* out)
{
    if (!out || idx < 0 || idx >= (int)layers.size()) return VNECT_E_ARG;
    const Layer& L = layers[idx];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", L.name.c_str());
    if (L.op == OP_CONV) {
        out->M = L.a.M * L.a.nphase, out->N = L.Nreal, out->K = L.Kreal;
        out->tile_m = L.BM, out->tile_n = L.BN, out->split_k = L.a.ksplit;
        out->workgroups = ((L.a.M + L.BM - 1) / L.BM) * (L.a.Npad / L.BN) * L.a.nphase * L.a.ksplit;
        out->flops = L.flops;
    }
    out->last_ms = L.last_ms;
    return VNECT_OK;
}

int vnect_get_layer_info(vnect_handle* h, int idx, vnect_layer_info* out)
{
    return guarded(&h, [&]() -> int { return h ? layer_info(h->layers, idx, out) : VNECT_E_ARG; });
}

int vnect_get_batch_layer_info(vnect_handle* h, int idx, vnect_layer_info* out)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (h->bplans.empty()) return fail(h, VNECT_E_STATE, "vnect_get_batch_layer_info: no batched plan (vnect_set_stream_batch(h, 2), then vnect_finalize)");
        return layer_info(h->bplans[0]->layers, idx, out);
    });
}

// rows a launch computes: M (x phases) for every launch but a live-rows one
static int rows_computed(const std::vector<Layer>& layers, int idx, int32_t* rows)
{
    if (!rows || idx < 0 || idx >= (int)layers.size()) return VNECT_E_ARG;
    const Layer& L = layers[idx];
    *rows = L.op != OP_CONV ? 0 : L.a.live_s ? plan::live_rows(L.a.S, L.a.Ho, L.a.Wo, L.a.live_s) : L.a.M * L.a.nphase;
    return VNECT_OK;
}

int vnect_get_layer_rows(vnect_handle* h, int idx, int batch, int32_t* rows_computed_out, int32_t* live_rule_stride)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (batch && h->bplans.empty()) return fail(h, VNECT_E_STATE, "vnect_get_layer_rows: no batched plan (vnect_set_stream_batch(h, 2), then vnect_finalize)");
        const std::vector<Layer>& layers = batch ? h->bplans[0]->layers : h->layers;
        const int rc = rows_computed(layers, idx, rows_computed_out);
        if (rc == VNECT_OK && live_rule_stride) *live_rule_stride = live_rows_of(layers, idx, h->t_out);
        return rc;
    });
}

int vnect_set_stream_batch(vnect_handle* h, int n)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (h->finalized || h->pre_only) return fail(h, VNECT_E_STATE, "vnect_set_stream_batch after vnect_finalize or on a preprocess_only handle");
        if (h->sharded) return fail(h, VNECT_E_ARG, "vnect_set_stream_batch: a pyramid-sharded handle serves one stream");
        if (n < 1 || n > 2) return fail(h, VNECT_E_ARG, "vnect_set_stream_batch: n must be 1 or 2");
        if (2 * h->Snet > VNECT_MAX_SCALES && n == 2) return fail(h, VNECT_E_ARG, "vnect_set_stream_batch: 2 x num_scales exceeds VNECT_MAX_SCALES");
        if (h->people && n == 2) return fail(h, VNECT_E_ARG, "vnect_set_stream_batch: not together with vnect_set_people");
        h->stream_batch = n;
        return VNECT_OK;
    });
}

int vnect_submit_streams(vnect_handle* h, int n, const int32_t* streams, const int32_t* slots, const double* t2d, const double* t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!streams || !slots || !t2d || !t3d) return fail(h, VNECT_E_ARG, "vnect_submit_streams: bad argument");
        if (!h->finalized) return fail(h, VNECT_E_STATE, "inference before vnect_finalize");
        if (n != 1 && n != 2) return fail(h, VNECT_E_ARG, "vnect_submit_streams: n must be 1 or 2");
        HIPCK(h, hipSetDevice(h->cfg.device));
        if (n == 1) {
            int ring;
            return enqueue_frame(h, slots[0], t2d[0], t3d[0], &ring, streams[0]);
        }
        return enqueue_batch(h, streams, slots, t2d, t3d);
    });
}

// ---- tracking on the device (ABI v7, additive) ---------------------------------------------------------------------------------------
int vnect_track_begin(vnect_handle* h, int stream, int H, int W, const int32_t* rect4)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (h->sharded) return fail(h, VNECT_E_ARG, "vnect_track_begin: tracking on a pyramid-sharded handle is not supported");
        if (h->stream_batch == 2 || !h->bplans.empty())
            return fail(h, VNECT_E_ARG, "vnect_track_begin: tracking on a handle with the two-stream batch is not supported");
        if (!h->finalized) return fail(h, VNECT_E_STATE, "vnect_track_begin before vnect_finalize");
        HIPCK(h, hipSetDevice(h->cfg.device));
        return track_begin_impl(h, stream, H, W, rect4);
    });
}

int vnect_submit_tracked(vnect_handle* h, int stream, int slot, double t2d, double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return submit_tracked_from(h, stream, slot, t2d, t3d, [](FrameSrc*) { return VNECT_OK; });  // (a FrameSrc is born SRC_SLOT)
    });
}

int vnect_submit_tracked_pinned(vnect_handle* h, int stream, int buffer_index, int64_t row_stride, double t2d, double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return submit_tracked_from(h, stream, -1, t2d, t3d, [&](FrameSrc* s) {
            const Stream& sm = h->streams[stream];  // (the buffer holds the frame as it is stored: the track's size turned back)
            return resolve_pinned_bgr(h, "vnect_submit_tracked_pinned", buffer_index, stored_H(sm), stored_W(sm), row_stride, sm.orient, s);
        });
    });
}

int vnect_collect_tracked(vnect_handle* h, int32_t* stream_out, double* j2, float* j3, int32_t* rect4)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return collect_impl(h, j2, j3, stream_out, rect4);
    });
}

int vnect_track_box(vnect_handle* h, int stream, int32_t* rect4)
{
    return guarded(&h, [&]() -> int {
        if (!h || !rect4) return VNECT_E_ARG;
        if (stream < 0 || stream >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
        const Stream& sm = h->streams[stream];
        if (!sm.track_on) return fail(h, VNECT_E_STATE, "stream is not tracking: call vnect_track_begin first");
        HIPCK(h, hipSetDevice(h->cfg.device));
        if (sm.seq >= (long long)h->seq_collect) HIPCK(h, hipEventSynchronize(h->ring[sm.seq % RING].done));
        std::vector<TrackState> ts(1);
        HIPCK(h, hipMemcpy(&ts[0], h->d_track + stream, sizeof(TrackState), hipMemcpyDeviceToHost));
        rect4[0] = ts[0].x, rect4[1] = ts[0].y, rect4[2] = ts[0].uw, rect4[3] = ts[0].uh;
        return VNECT_OK;
    });
}

// ---- per-joint confidence and the loss rule of a tracked stream (ABI v7, additive; CONFIDENCE.md) ---------------------------------------
int vnect_result_confidence(vnect_handle* h, double* confidence21, int32_t* lost_out)
{
    return guarded(&h, [&]() -> int {
        if (!h || !confidence21) return h ? fail(h, VNECT_E_ARG, "vnect_result_confidence: bad argument") : VNECT_E_ARG;
        if (!h->have_conf) return fail(h, VNECT_E_STATE, "vnect_result_confidence: no frame has been delivered on this handle yet");
        memcpy(confidence21, h->last_conf, sizeof h->last_conf);
        if (lost_out) *lost_out = h->last_lost;
        return VNECT_OK;
    });
}

int vnect_track_policy(vnect_handle* h, int stream, double min_confidence, int min_joints, int action)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (h->sharded) return fail(h, VNECT_E_ARG, "vnect_track_policy: tracking on a pyramid-sharded handle is not supported");
        if (h->stream_batch == 2 || !h->bplans.empty())
            return fail(h, VNECT_E_ARG, "vnect_track_policy: tracking on a handle with the two-stream batch is not supported");
        if (stream < 0 || stream >= VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "stream out of range");
        if (min_joints < 1 || min_joints > NJ) return fail(h, VNECT_E_ARG, "vnect_track_policy: min_joints must be 1 .. 21");
        if (action < TRACK_LOST_OFF || action > TRACK_LOST_RESET) return fail(h, VNECT_E_ARG, "vnect_track_policy: action must be 0 (off), 1 (hold) or 2 (reset)");
        if (min_confidence != min_confidence) return fail(h, VNECT_E_ARG, "vnect_track_policy: min_confidence is NaN");
        if (!h->finalized) return fail(h, VNECT_E_STATE, "vnect_track_policy before vnect_finalize");
        Stream& sm = h->streams[stream];
        // the box stage of a tracked frame in flight reads the rule whenever it runs: no change under it
        if (sm.seq >= (long long)h->seq_collect && h->ring[sm.seq % RING].f.tracked)
            return fail(h, VNECT_E_STATE, "vnect_track_policy: the stream has a tracked frame in flight: collect it first");
        HIPCK(h, hipSetDevice(h->cfg.device));
        // (an untracked frame of the stream may still be in flight, and so may other streams' frames: none of them reads this rule)
        const TrackPolicy p{min_confidence, min_joints, action};
        HIPCK(h, hipMemcpy(h->d_policy + stream, &p, sizeof p, hipMemcpyHostToDevice));
        sm.policy = p;
        return VNECT_OK;
    });
}

// ---- people mode (ABI v7, additive; PEOPLE.md): several persons of one video, person p on stream p, one submit per frame -----------------
int vnect_set_people(vnect_handle* h, int n, int pair)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (n < 1 || n > VNECT_MAX_STREAMS) return fail(h, VNECT_E_ARG, "vnect_set_people: n must be 1 .. VNECT_MAX_STREAMS");
        if (pair != 0 && pair != 1) return fail(h, VNECT_E_ARG, "vnect_set_people: pair must be 0 or 1");
        if (h->finalized || h->pre_only) return fail(h, VNECT_E_STATE, "vnect_set_people after vnect_finalize or on a preprocess_only handle");
        if (h->sharded) return fail(h, VNECT_E_ARG, "vnect_set_people: a pyramid-sharded handle serves one stream");
        if (h->stream_batch == 2) return fail(h, VNECT_E_ARG, "vnect_set_people: not together with vnect_set_stream_batch(h, 2)");
        h->people = n, h->people_pair = pair != 0;
        return VNECT_OK;
    });
}

// n within what vnect_set_people gave, on a finalized people handle
static int people_ok(vnect_handle* h, const char* who, int n)
{
    if (!h->people) return fail(h, VNECT_E_STATE, std::string(who) + ": not a people handle (vnect_set_people before vnect_finalize)");
    if (n < 1 || n > h->people) return fail(h, VNECT_E_ARG, std::string(who) + ": n must be 1 .. the n vnect_set_people was given");
    if (!h->finalized) return fail(h, VNECT_E_STATE, std::string(who) + " before vnect_finalize");
    return VNECT_OK;
}

int vnect_people_begin(vnect_handle* h, int n, int H, int W, const int32_t* rects)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        int rc = people_ok(h, "vnect_people_begin", n);
        if (rc) return rc;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return people_begin_impl(h, n, H, W, rects);
    });
}

int vnect_submit_people(vnect_handle* h, int n, int slot, double t2d, double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        int rc = people_ok(h, "vnect_submit_people", n);
        if (rc) return rc;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return enqueue_people(h, n, slot, t2d, t3d, FrameSrc());  // (a FrameSrc is born SRC_SLOT)
    });
}

int vnect_submit_people_device(vnect_handle* h, int n, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d,
                               const vnect_overlay_style* style, const vnect_preview_spec* preview_spec)
{
    return guarded(&h, [&]() -> int {
        static const char* who = "vnect_submit_people_device";
        if (!h) return VNECT_E_ARG;
        int rc = people_ok(h, who, n);
        if (rc) return rc;
        for (int p = 0; p < n; p++)
            if ((rc = tracked_ok(h, p))) return rc;
        HIPCK(h, hipSetDevice(h->cfg.device));
        const int orient = h->streams[0].orient;  // (enqueue_people refuses persons that began under another one)
        FrameSrc s;
        if (preview_spec) {  // the frame's one picture; the frame itself is drawn into only where a style is given too
            vnect_preview_spec sp;
            const bool sized = preview_spec->struct_size == (int32_t)sizeof(vnect_preview_spec);
            if (sized) sp = *preview_spec, sp.draw_frame = style ? 1 : 0;
            if ((rc = check_tracked_preview(h, who, frame, producer_stream, style, sized ? &sp : preview_spec, orient, &s))) return rc;
        } else if (style) {
            OverlayTarget t;
            OverlayInput in;
            if ((rc = check_draw(h, who, frame, producer_stream, style, orient, &t, &in, &s))) return rc;
            s.draw = true, s.draw_target = t, s.draw_in = in;
        } else if ((rc = check_device_frame(h, frame, producer_stream, who, false, orient, &s))) {
            return rc;
        }
        return enqueue_people(h, n, -1, t2d, t3d, s);
    });
}

int vnect_result_people(vnect_handle* h, int32_t* units_out, int32_t* paired_out)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!units_out || !paired_out) return fail(h, VNECT_E_ARG, "vnect_result_people: bad argument");
        *units_out = h->last_people_units, *paired_out = h->last_people_paired;
        return VNECT_OK;
    });
}

// ---- NV12 frames (additive): the conversion to BGR happens on the device, inside the frame's copy (post.hip: nv12_copy_kernel) ----------
int vnect_upload_frame_nv12(vnect_handle* h, int slot, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return upload_from(h, slot, "vnect_upload_frame_nv12",
                           [&](FrameSrc* s) { return resolve_host_nv12(h, "vnect_upload_frame_nv12", y, y_stride, uv, uv_stride, H, W, nullptr, h->orient, s); });
    });
}

int vnect_upload_frame_nv12_rect(vnect_handle* h, int slot, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W,
                                 const int32_t* rect4)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return upload_from(h, slot, "vnect_upload_frame_nv12_rect",
                           [&](FrameSrc* s) { return resolve_host_nv12(h, "vnect_upload_frame_nv12_rect", y, y_stride, uv, uv_stride, H, W, rect4, h->orient, s); });
    });
}

int vnect_infer_nv12(vnect_handle* h, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W, const int32_t* rect4,
                     double t2d, double t3d, double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h || !y || !uv || !j2 || !j3) return VNECT_E_ARG;
        return infer_from(h, "vnect_infer_nv12", t2d, t3d, j2, j3,
                          [&](FrameSrc* s) { return resolve_host_nv12(h, "vnect_infer_nv12", y, y_stride, uv, uv_stride, H, W, rect4, h->orient, s); });
    });
}

int vnect_preprocess_nv12(vnect_handle* h, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W, const int32_t* rect4,
                          float* batch_out, double* scaler, int32_t* offset_x, int32_t* offset_y)
{
    return guarded(&h, [&]() -> int {
        if (!h || !y || !uv) return VNECT_E_ARG;
        return preprocess_from(h, "vnect_preprocess_nv12", batch_out, scaler, offset_x, offset_y,
                               [&](FrameSrc* s) { return resolve_host_nv12(h, "vnect_preprocess_nv12", y, y_stride, uv, uv_stride, H, W, rect4, h->orient, s); });
    });
}

int vnect_submit_tracked_pinned_nv12(vnect_handle* h, int stream, int buffer_index, int64_t y_stride, int64_t uv_offset, int64_t uv_stride, double t2d,
                                     double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return submit_tracked_from(h, stream, -1, t2d, t3d, [&](FrameSrc* s) {
            const Stream& sm = h->streams[stream];
            return resolve_pinned_nv12(h, "vnect_submit_tracked_pinned_nv12", buffer_index, stored_H(sm), stored_W(sm), y_stride, uv_offset, uv_stride,
                                       sm.orient, s);
        });
    });
}

// ---- frames in the caller's device memory (additive): a kernel writes them into the slot (post.hip: ingest_copy_kernel; ingest.h) ---------
int vnect_upload_frame_device(vnect_handle* h, int slot, const vnect_device_frame* frame, void* producer_stream)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return upload_from(h, slot, "vnect_upload_frame_device",
                           [&](FrameSrc* s) { return check_device_frame(h, frame, producer_stream, "vnect_upload_frame_device", true, h->orient, s); });
    });
}

int vnect_infer_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d, double* j2, float* j3)
{
    return guarded(&h, [&]() -> int {
        if (!h || !j2 || !j3) return VNECT_E_ARG;
        return infer_from(h, "vnect_infer_device", t2d, t3d, j2, j3,
                          [&](FrameSrc* s) { return check_device_frame(h, frame, producer_stream, "vnect_infer_device", true, h->orient, s); });
    });
}

int vnect_preprocess_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, float* batch_out, double* scaler,
                            int32_t* offset_x, int32_t* offset_y)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return preprocess_from(h, "vnect_preprocess_device", batch_out, scaler, offset_x, offset_y,
                               [&](FrameSrc* s) { return check_device_frame(h, frame, producer_stream, "vnect_preprocess_device", true, h->orient, s); });
    });
}

int vnect_submit_tracked_device(vnect_handle* h, int stream, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return submit_tracked_from(h, stream, -1, t2d, t3d, [&](FrameSrc* s) {
            const Stream& sm = h->streams[stream];
            int rc = check_device_frame(h, frame, producer_stream, "vnect_submit_tracked_device", false, sm.orient, s);
            if (rc) return rc;
            if (s->H != stored_H(sm) || s->W != stored_W(sm))
                return fail(h, VNECT_E_ARG, "vnect_submit_tracked_device: the frame is not of the size vnect_track_begin gave for this stream");
            return (int)VNECT_OK;
        }, true);
    });
}

int vnect_submit_tracked_device_draw(vnect_handle* h, int stream, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d,
                                     const vnect_overlay_style* style)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return submit_tracked_from(h, stream, -1, t2d, t3d, [&](FrameSrc* s) {
            static const char* who = "vnect_submit_tracked_device_draw";
            OverlayTarget t;
            OverlayInput in;
            const Stream& sm = h->streams[stream];
            int rc = check_draw(h, who, frame, producer_stream, style, sm.orient, &t, &in, s);
            if (rc) return rc;
            if (s->H != stored_H(sm) || s->W != stored_W(sm))
                return fail(h, VNECT_E_ARG, std::string(who) + ": the frame is not of the size vnect_track_begin gave for this stream");
            s->draw = true, s->draw_target = t, s->draw_in = in;
            return (int)VNECT_OK;
        }, true);
    });
}

// run_estimator_ps.py:94-96 inside the tracked loop: the frame's preview computed behind its box stage, delivered with the frame
int vnect_submit_tracked_device_preview(vnect_handle* h, int stream, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d,
                                        const vnect_overlay_style* style, const vnect_preview_spec* spec)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return submit_tracked_from(h, stream, -1, t2d, t3d, [&](FrameSrc* s) {
            static const char* who = "vnect_submit_tracked_device_preview";
            const Stream& sm = h->streams[stream];
            int rc = check_tracked_preview(h, who, frame, producer_stream, style, spec, sm.orient, s);
            if (rc) return rc;
            if (s->H != stored_H(sm) || s->W != stored_W(sm))
                return fail(h, VNECT_E_ARG, std::string(who) + ": the frame is not of the size vnect_track_begin gave for this stream");
            return (int)VNECT_OK;
        }, true);
    });
}

int vnect_result_preview(vnect_handle* h, const uint8_t** data, int32_t hw[2], int64_t* pitch)
{
    return guarded(&h, [&]() -> int {
        if (!h || !data || !hw || !pitch) return h ? fail(h, VNECT_E_ARG, "vnect_result_preview: bad argument") : VNECT_E_ARG;
        h->previews.result(data, hw, pitch);
        return VNECT_OK;
    });
}

int vnect_draw_device(vnect_handle* h, const vnect_device_frame* target, void* stream, const double* joints_2d, const double* confidence21,
                      const int32_t* rect4, const vnect_overlay_style* style)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return draw_device_impl(h, target, stream, joints_2d, confidence21, rect4, style);
    });
}

// ---- the 3-D view (additive; VIEW3D.md; run_estimator_ps.py:90, 124-126; src/utils.py:272-304, 317-330): one launch of view3d.hip ------
int vnect_view3d_device(vnect_handle* h, const float* joints_3d, const double* confidence21, const vnect_view3d_spec* spec, void* out, int64_t out_pitch)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return view3d_device_impl(h, joints_3d, confidence21, spec, out, out_pitch);
    });
}

// run_estimator_ps.py:90 inside the tracked loop: every tracked submit of the stream also renders its frame's view
int vnect_track_view3d(vnect_handle* h, int stream, const vnect_view3d_spec* spec)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return track_view3d_impl(h, stream, spec);
    });
}

// src/utils.py:317-330: the picture the plot process shows, of the frame delivered last
int vnect_result_view3d(vnect_handle* h, const uint8_t** data, int32_t hw[2], int64_t* pitch)
{
    return guarded(&h, [&]() -> int {
        if (!h || !data || !hw || !pitch) return h ? fail(h, VNECT_E_ARG, "vnect_result_view3d: bad argument") : VNECT_E_ARG;
        h->views.result(data, hw, pitch);
        return VNECT_OK;
    });
}

// ---- the preview (additive; PREVIEW.md; run_estimator_ps.py:94-96): the annotated frame scaled for display, one launch of preview.hip --
int vnect_preview_size(vnect_handle* h, const vnect_device_frame* frame, const vnect_preview_spec* spec, int32_t out_hw[2])
{
    return guarded(&h, [&]() -> int {
        if (!h || !out_hw) return VNECT_E_ARG;
        return preview_size_impl(h, frame, spec, out_hw);
    });
}

int vnect_preview_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, const double* joints_2d, const double* confidence21,
                         const int32_t* rect4, const vnect_overlay_style* style, const vnect_preview_spec* spec, void* out, int64_t out_pitch)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return preview_device_impl(h, frame, producer_stream, joints_2d, confidence21, rect4, style, spec, out, out_pitch);
    });
}

// ---- orientation (additive; ORIENTATION.md): frames that are stored rotated / mirrored, turned inside the crop's copy (orient.hip) ------
// ---- the person detector (additive; HOG.md; src/hog_box.py:24-33): HOG + linear SVM over a pyramid, three launches of hog.hip ----------
int vnect_hog_set_detector(vnect_handle* h, const float* w, int n)  // hog_box.py:26
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return hog_set_detector_impl(h, w, n);
    });
}

int vnect_hog_levels(vnect_handle* h, const vnect_device_frame* frame, const vnect_hog_spec* spec, int32_t* n_out, int32_t* hw_out, double* scales_out,
                     int capacity)  // hog_box.py:28
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        return hog_levels_impl(h, frame, spec, n_out, hw_out, scales_out, capacity);
    });
}

int vnect_hog_detect_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, const vnect_hog_spec* spec, int32_t* rects4,
                            double* weights, int capacity, int32_t* count_out)  // hog_box.py:28
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return hog_detect_device_impl(h, frame, producer_stream, spec, rects4, weights, capacity, count_out);
    });
}

int vnect_hog_detect(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, const vnect_hog_spec* spec, int32_t* rects4, double* weights,
                     int capacity, int32_t* count_out)  // hog_box.py:28
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return hog_detect_host_impl(h, bgr, H, W, row_stride, spec, rects4, weights, capacity, count_out);
    });
}

// ---- re-detection inside the device tracking loop (additive; HOG.md; src/hog_box.py:26-31 behind run_estimator_ps.py:96-107) -------------
int vnect_track_redetect(vnect_handle* h, int stream, const vnect_hog_spec* spec, int enable)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        HIPCK(h, hipSetDevice(h->cfg.device));
        return track_redetect_impl(h, stream, spec, enable);
    });
}

int vnect_result_redetect(vnect_handle* h, int32_t* status, int32_t rect4[4], int32_t* hits)
{
    return guarded(&h, [&]() -> int {
        if (!h || !status) return h ? fail(h, VNECT_E_ARG, "vnect_result_redetect: bad argument") : VNECT_E_ARG;
        *status = h->last_redet.status;
        if (rect4)
            for (int k = 0; k < 4; k++) rect4[k] = h->last_redet.rect[k];
        if (hits) *hits = h->last_redet.hits;
        return VNECT_OK;
    });
}

int vnect_set_orientation(vnect_handle* h, int orientation)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!orient_ok(orientation)) return fail(h, VNECT_E_ARG, "vnect_set_orientation: the orientation is a code 0 .. 7 (np.rot90 by code & 3, mirrored when code & 4)");
        if (h->sharded) return fail(h, VNECT_E_ARG, "vnect_set_orientation: orientation on a pyramid-sharded handle is not supported");
        h->orient = orientation;  // (a frame in flight has been copied, or carries its own code: nothing of it reads this)
        return VNECT_OK;
    });
}

int vnect_read_frame(vnect_handle* h, int slot, uint8_t* out, int64_t capacity, int32_t* hw2)
{
    return guarded(&h, [&]() -> int {
        if (!h || !hw2) return VNECT_E_ARG;
        if (slot < 0 || slot >= (int)h->slots.size() || h->slots[slot].H == 0) return fail(h, VNECT_E_ARG, "vnect_read_frame: frame slot empty or out of range");
        const vnect_handle::SlotInfo& si = h->slots[slot];
        hw2[0] = si.H, hw2[1] = si.W;
        if (!out) return VNECT_OK;
        if ((int64_t)si.H * si.W * 3 > capacity) return fail(h, VNECT_E_ARG, "vnect_read_frame: capacity too small");
        HIPCK(h, hipSetDevice(h->cfg.device));
        HIPCK(h, hipStreamSynchronize(h->st));  // (a staged frame's copy runs on the handle's stream)
        HIPCK(h, hipMemcpy2D(out, (size_t)si.W * 3, h->frames + (size_t)slot * h->cfg.max_frame_bytes, (size_t)si.stride, (size_t)si.W * 3, si.H, hipMemcpyDeviceToHost));
        return VNECT_OK;
    });
}

#if VNECT_TEST_HOOKS
// ---- test build only (`make testhooks`): NOT in the shipped library, NOT declared in include/vnect_abi.h --------------------------------
// While set, every enqueued frame's conv-stack output is overwritten with these (S, 46, 46, 84) maps before its post-processing launch
// (rt_exec.cpp: enqueue_frame), so a test chooses the joints -- and through them the next crop -- of a tracked frame, while lane choice,
// cross-lane waits, xfail / xseq, ring slots, collect, error propagation and the timestamps' rollback stay the product's.  The maps
// are copied to the device here: the caller's buffer is free on return, and a frame in flight keeps the maps it was enqueued with.
// maps == nullptr ends the override.
int vnect_test_maps_override(vnect_handle* h, const float* maps)
{
    return guarded(&h, [&]() -> int {
        if (!h) return VNECT_E_ARG;
        if (!h->finalized || h->sharded) return fail(h, VNECT_E_STATE, "vnect_test_maps_override: needs a finalized, unsharded handle");
        if (!maps) {
            h->test_maps_cur = -1;
            return VNECT_OK;
        }
        HIPCK(h, hipSetDevice(h->cfg.device));
        const size_t n = (size_t)h->S * HM * HM * MAPC;
        if (!h->test_st) HIPCK(h, hipStreamCreateWithFlags(&h->test_st, hipStreamNonBlocking));
        const int k = (h->test_maps_cur + 1) % (RING + 1);
        int rc;
        if (!h->test_maps[k] && (rc = dev_alloc(h, &h->test_maps[k], n))) return rc;
        HIPCK(h, hipMemcpyAsync(h->test_maps[k], maps, n * sizeof(float), hipMemcpyHostToDevice, h->test_st));
        HIPCK(h, hipStreamSynchronize(h->test_st));
        h->test_maps_cur = k;
        return VNECT_OK;
    });
}
// the stream's TrackState as the device holds it once the stream's last frame has finished: sizeof(TrackState) bytes (returned in *size)
int vnect_test_track_state(vnect_handle* h, int stream, uint8_t* out, int32_t cap, int32_t* size)
{
    return guarded(&h, [&]() -> int {
        if (!h || !out || !size) return VNECT_E_ARG;
        if (stream < 0 || stream >= VNECT_MAX_STREAMS || !h->streams[stream].track_on) return fail(h, VNECT_E_STATE, "vnect_test_track_state: stream is not tracking");
        *size = (int32_t)sizeof(TrackState);
        if (cap < *size) return fail(h, VNECT_E_ARG, "vnect_test_track_state: buffer too small");
        HIPCK(h, hipSetDevice(h->cfg.device));
        const Stream& sm = h->streams[stream];
        if (sm.seq >= (long long)h->seq_collect) HIPCK(h, hipEventSynchronize(h->ring[sm.seq % RING].done));
        HIPCK(h, hipMemcpy(out, h->d_track + stream, sizeof(TrackState), hipMemcpyDeviceToHost));
        return VNECT_OK;
    });
}
#endif

}  // extern "C"
