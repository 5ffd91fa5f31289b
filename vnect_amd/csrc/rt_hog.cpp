// rt_hog.cpp -- the person detector behind the C ABI (vnect_hog_set_detector / vnect_hog_levels / vnect_hog_detect_device /
// vnect_hog_detect; src/hog_box.py:24-33).  The frame is validated by the device-frame resolver of rt_ingest.cpp and read where it lies,
// as the preview reads it; the spec becomes hog.h's level table, from which the handle's workspace is sized; three launches of hog.hip
// cover all levels; the hits come back, are put in the order (level, y, x) and grouped on the host (hog.h: hog_group).  A refusal
// changes nothing and launches nothing.  vnect_track_redetect: the same detection inside the device tracking loop, on a workspace of the
// stream's own -- gated launches and a pick kernel behind every tracked frame's box stage, nothing coming back to the host but a verdict.
#include "runtime.h"

namespace vnect {
namespace rt {

static int refuse(vnect_handle* h, const char* who, const char* what) { return fail(h, VNECT_E_ARG, std::string(who) + ": " + what); }

// the spec (nullptr: all defaults) with its defaults filled in
static int spec_in(vnect_handle* h, const char* who, const vnect_hog_spec* s, HogSpec* out)
{
    vnect_hog_spec z;
    memset(&z, 0, sizeof z);
    if (s) {
        if (s->struct_size != (int32_t)sizeof(vnect_hog_spec)) return refuse(h, who, "vnect_hog_spec::struct_size is not sizeof(vnect_hog_spec)");
        z = *s;
    }
    if (z.win_stride_x < 0 || z.win_stride_y < 0 || z.nlevels < 0 || z.max_hits < 0) return refuse(h, who, "a negative field in vnect_hog_spec");
    const int rc = hog_spec(z.hit_threshold, z.win_stride_x, z.win_stride_y, z.scale0, z.final_threshold, z.nlevels, z.max_hits, out);
    return rc == HOG_OK ? VNECT_OK : refuse(h, who, hog_refusal(rc));
}

static int common_in(vnect_handle* h, const char* who, bool need_detector)
{
    if (h->sharded) return refuse(h, who, "the detector on a pyramid-sharded handle is not supported");
    if (need_detector && h->hog_det.empty()) return fail(h, VNECT_E_STATE, std::string(who) + ": no detector set: call vnect_hog_set_detector first");
    return VNECT_OK;
}

int hog_set_detector_impl(vnect_handle* h, const float* w, int n)
{
    static const char* who = "vnect_hog_set_detector";
    int rc0 = common_in(h, who, false);
    if (rc0) return rc0;
    std::vector<float> d;
    if (!hog_detector(w, n, &d)) return refuse(h, who, "the detector is 3781 finite floats, rho last (or 3780: rho 0)");
    for (const Stream& sm : h->streams)  // (a re-detecting stream's frame in flight reads the detector whenever its chain runs)
        if (sm.rd_on && sm.seq >= (long long)h->seq_collect && h->ring[sm.seq % RING].f.tracked)
            return fail(h, VNECT_E_STATE, std::string(who) + ": a re-detecting stream has a tracked frame in flight: collect it first");
    if (!h->hog_det_dev) {
        int rc = dev_alloc(h, &h->hog_det_dev, d.size());
        if (rc) return rc;
    }
    if (h->upload_st) HIPCK(h, hipStreamSynchronize(h->upload_st));
    HIPCK(h, hipMemcpy(h->hog_det_dev, d.data(), d.size() * sizeof(float), hipMemcpyHostToDevice));
    h->hog_det.swap(d);
    return VNECT_OK;
}

int hog_levels_impl(vnect_handle* h, const vnect_device_frame* f, const vnect_hog_spec* spec, int32_t* n_out, int32_t* hw_out, double* scales_out, int capacity)
{
    static const char* who = "vnect_hog_levels";
    int rc = common_in(h, who, false);
    if (rc) return rc;
    if (!f) return refuse(h, who, "no frame descriptor");
    if (f->struct_size != (int32_t)sizeof(vnect_device_frame)) return refuse(h, who, "vnect_device_frame::struct_size is not sizeof(vnect_device_frame)");
    if (f->H < 1 || f->W < 1 || f->H > (1 << 24) || f->W > (1 << 24)) return refuse(h, who, "bad frame geometry");
    if (!n_out || capacity < 0) return refuse(h, who, "bad argument");
    HogSpec sp;
    if ((rc = spec_in(h, who, spec, &sp))) return rc;
    std::vector<HogPlan> pv(1);
    if ((rc = hog_plan(h->orient, f->H, f->W, sp, &pv[0]))) return refuse(h, who, hog_refusal(rc));
    *n_out = pv[0].n;
    for (int n = 0; n < pv[0].n && n < capacity; n++) {
        if (hw_out) hw_out[2 * n] = pv[0].lv[n].h, hw_out[2 * n + 1] = pv[0].lv[n].w;
        if (scales_out) scales_out[n] = pv[0].lv[n].s;
    }
    return VNECT_OK;
}

// workspace buffer i with room for `need` bytes
static int grow(vnect_handle* h, int i, size_t need)
{
    if (need <= h->hog_cap[i]) return VNECT_OK;
    if (h->upload_st) HIPCK(h, hipStreamSynchronize(h->upload_st));
    return dev_grow(h, &h->hog_buf[i], &h->hog_cap[i], need);
}

// the host-built tables on the device (and the handle's level table), once
static int tables_ready(vnect_handle* h)
{
    if (h->hog_tab) return VNECT_OK;
    HogTables t;
    hog_tables(&t);
    int rc;
    if ((rc = dev_alloc(h, &h->hog_tab, 1))) return rc;
    HIPCK(h, hipMemcpy(h->hog_tab, &t, sizeof t, hipMemcpyHostToDevice));
    return dev_alloc(h, &h->hog_lv, HOG_MAX_LEVELS);
}

// the detection of a validated source on upload_st; `stream`: what the launches wait for
static int detect(vnect_handle* h, const char* who, const HogSrc& a, const HogSpec& sp, void* stream, int32_t* rects4, double* weights, int capacity, int32_t* count_out)
{
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    int rc = hog_plan(a.o, a.H, a.W, sp, &p);
    if (rc) return refuse(h, who, hog_refusal(rc));
    if (!p.n) {  // a picture smaller than the window: no level, no detection, no launch
        *count_out = 0;
        return VNECT_OK;
    }
    if ((rc = tables_ready(h))) return rc;
    if ((rc = grow(h, 0, sizeof(float2) * (size_t)p.npix)) || (rc = grow(h, 1, (size_t)p.npix)) || (rc = grow(h, 2, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk)) ||
        (rc = grow(h, 3, sizeof(HogHit) * (size_t)sp.max_hits)) || (rc = grow(h, 4, 256)))
        return rc;
    if (!h->upload_st) HIPCK(h, hipStreamCreateWithFlags(&h->upload_st, hipStreamNonBlocking));
    if ((rc = wait_for_producer(h, stream, h->upload_st))) return rc;
    HIPCK(h, hipMemcpyAsync(h->hog_lv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice, h->upload_st));
    const HogDev d{h->hog_lv, h->hog_tab, h->hog_det_dev, (float2*)h->hog_buf[0], h->hog_buf[1], (float*)h->hog_buf[2], (HogHit*)h->hog_buf[3],
                   (unsigned*)h->hog_buf[4], nullptr};
    HIPCK(h, launch_hog(a, p, d, sp.hit_threshold, sp.max_hits, 7, h->upload_st));
    unsigned count = 0;
    HIPCK(h, hipMemcpyAsync(&count, d.count, sizeof count, hipMemcpyDeviceToHost, h->upload_st));
    HIPCK(h, hipStreamSynchronize(h->upload_st));
    if (count > (unsigned)sp.max_hits)
        return fail(h, VNECT_E_STATE, std::string(who) + ": " + std::to_string(count) + " windows reached hit_threshold, more than max_hits (" + std::to_string(sp.max_hits) +
                                          "): raise hit_threshold (or max_hits)");
    std::vector<HogHit> hits(count);
    if (count) HIPCK(h, hipMemcpy(hits.data(), d.hits, sizeof(HogHit) * count, hipMemcpyDeviceToHost));
    std::vector<HogRect> rects;
    std::vector<double> ws;
    hog_hit_rects(p, hits, &rects, &ws);
    hog_group(rects, ws, (int)sp.final_threshold);
    for (size_t i = 0; i < rects.size() && (int)i < capacity; i++) {
        if (rects4) rects4[4 * i] = rects[i].x, rects4[4 * i + 1] = rects[i].y, rects4[4 * i + 2] = rects[i].w, rects4[4 * i + 3] = rects[i].h;
        if (weights) weights[i] = ws[i];
    }
    *count_out = (int32_t)rects.size();
    return VNECT_OK;
}

int hog_detect_device_impl(vnect_handle* h, const vnect_device_frame* f, void* stream, const vnect_hog_spec* spec, int32_t* rects4, double* weights, int capacity,
                           int32_t* count_out)
{
    static const char* who = "vnect_hog_detect_device";
    int rc = common_in(h, who, true);
    if (rc) return rc;
    if (!count_out || capacity < 0 || (capacity > 0 && (!rects4 || !weights))) return refuse(h, who, "bad output arguments");
    if (f && f->struct_size == (int32_t)sizeof(vnect_device_frame) && f->has_rect) return refuse(h, who, "the frame takes no rect: the whole picture is searched");
    HogSpec sp;
    if ((rc = spec_in(h, who, spec, &sp))) return rc;
    FrameSrc d;
    if ((rc = check_device_frame(h, f, stream, who, false, h->orient, &d))) return rc;
    int Hp, Wp;
    orient_size(h->orient, d.H, d.W, &Hp, &Wp);
    if (Hp > HOG_MAX_SIDE || Wp > HOG_MAX_SIDE) return refuse(h, who, hog_refusal(HOG_E_SIDE));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = orient_src_of(d), a.o = h->orient, a.H = d.H, a.W = d.W;
    return detect(h, who, a, sp, stream, rects4, weights, capacity, count_out);
}

int hog_detect_host_impl(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, const vnect_hog_spec* spec, int32_t* rects4, double* weights,
                         int capacity, int32_t* count_out)
{
    static const char* who = "vnect_hog_detect";
    int rc = common_in(h, who, true);
    if (rc) return rc;
    if (!count_out || capacity < 0 || (capacity > 0 && (!rects4 || !weights))) return refuse(h, who, "bad output arguments");
    if (!bgr || H < 1 || W < 1 || row_stride < (int64_t)W * 3) return refuse(h, who, "bad frame geometry");
    HogSpec sp;
    if ((rc = spec_in(h, who, spec, &sp))) return rc;
    int Hp, Wp;
    orient_size(h->orient, H, W, &Hp, &Wp);
    if (Hp > HOG_MAX_SIDE || Wp > HOG_MAX_SIDE) return refuse(h, who, hog_refusal(HOG_E_SIDE));
    if (Hp < HOG_WIN_H || Wp < HOG_WIN_W) {  // no level: nothing to copy either
        *count_out = 0;
        return VNECT_OK;
    }
    // the frame's rows to the device, packed: the pageable, synchronous copy vnect_upload_frame makes
    const size_t row = (size_t)W * 3;
    if ((rc = grow(h, 5, row * (size_t)H))) return rc;
    HIPCK(h, hipMemcpy2D(h->hog_buf[5], row, bgr, (size_t)row_stride, row, (size_t)H, hipMemcpyHostToDevice));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(false, false, h->hog_buf[5], nullptr, (long long)row, 3, 1, 0);
    a.o = h->orient, a.H = H, a.W = W;
    return detect(h, who, a, sp, VNECT_STREAM_SYNCED, rects4, weights, capacity, count_out);
}

// ---- re-detection inside the device tracking loop (vnect_track_redetect; hog.h: THE RULE) ------------------------------------------------
// buffer i of the stream's own workspace with room for `need` bytes (nothing of the stream is in flight; hipFree waits for the device)
static int rd_grow(vnect_handle* h, Stream& sm, int i, size_t need)
{
    if (need <= sm.rd_bytes[i]) return VNECT_OK;
    int rc = dev_grow(h, &sm.rd_buf[i], &sm.rd_bytes[i], need);
    if (rc) return rc;
    HIPCK(h, hipMemset(sm.rd_buf[i], 0, need));  // (the gate, the counter and the class sums start at zero)
    return VNECT_OK;
}

int redetect_prepare(vnect_handle* h, int stream, int H, int W, int orient)
{
    static const char* who = "vnect_track_redetect";
    Stream& sm = h->streams[stream];
    const int sH = (orient & 1) ? W : H, sW = (orient & 1) ? H : W;  // the frames as they are stored
    std::vector<HogPlan> pv(1);
    int rc = hog_plan(orient, sH, sW, sm.rd_spec, &pv[0]);
    if (rc) return refuse(h, who, hog_refusal(rc));
    const HogPlan& p = pv[0];
    if ((rc = tables_ready(h))) return rc;
    if ((rc = rd_grow(h, sm, 0, sizeof(HogLevel) * HOG_MAX_LEVELS)) || (rc = rd_grow(h, sm, 1, sizeof(float2) * (size_t)p.npix)) || (rc = rd_grow(h, sm, 2, (size_t)p.npix)) ||
        (rc = rd_grow(h, sm, 3, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk)) || (rc = rd_grow(h, sm, 4, sizeof(HogHit) * (size_t)sm.rd_spec.max_hits)) ||
        (rc = rd_grow(h, sm, 5, 256)) || (rc = rd_grow(h, sm, 6, sizeof(int) * 5 * HOG_TRACK_MAX_HITS)))
        return rc;
    if (p.n) HIPCK(h, hipMemcpy(sm.rd_buf[0], p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice));
    sm.rd_plan.swap(pv), sm.rd_o = orient, sm.rd_H = sH, sm.rd_W = sW;
    return VNECT_OK;
}

int track_redetect_impl(vnect_handle* h, int stream, const vnect_hog_spec* spec, int enable)
{
    static const char* who = "vnect_track_redetect";
    if (stream < 0 || stream >= VNECT_MAX_STREAMS) return refuse(h, who, "stream out of range");
    if (h->sharded) return refuse(h, who, "tracking on a pyramid-sharded handle is not supported");
    if (h->stream_batch == 2 || !h->bplans.empty()) return refuse(h, who, "tracking on a handle with the two-stream batch is not supported");
    // the pick takes the LARGEST detection, which would hand a lost person the other person (PEOPLE.md: a pick that excludes the others' boxes
    // is not built)
    if (h->people && enable) return refuse(h, who, "re-detection on a people handle (vnect_set_people) is not supported");
    if (!h->finalized) return fail(h, VNECT_E_STATE, std::string(who) + " before vnect_finalize");
    Stream& sm = h->streams[stream];
    HogSpec sp{};
    int rc;
    if (enable) {
        if ((rc = common_in(h, who, true))) return rc;
        if ((rc = spec_in(h, who, spec, &sp))) return rc;
        if (!spec || !spec->max_hits) sp.max_hits = HOG_TRACK_MAX_HITS;  // (the tracked default: what one workgroup's LDS groups)
        if (sp.max_hits > HOG_TRACK_MAX_HITS) return refuse(h, who, "max_hits of a tracked stream is at most 4096");
    }
    // the chain of a tracked frame in flight reads the setting's workspace whenever it runs: no change under it
    if (sm.seq >= (long long)h->seq_collect && h->ring[sm.seq % RING].f.tracked)
        return fail(h, VNECT_E_STATE, std::string(who) + ": the stream has a tracked frame in flight: collect it first");
    if (!enable) {
        sm.rd_on = false;
        return VNECT_OK;
    }
    if (!h->h_redet) {
        HIPCK(h, hipHostMalloc((void**)&h->h_redet, RING * sizeof(RedetectOut), hipHostMallocMapped | hipHostMallocCoherent));
        memset(h->h_redet, 0, RING * sizeof(RedetectOut));
        HIPCK(h, hipHostGetDevicePointer((void**)&h->h_redet_dev, h->h_redet, 0));
    }
    const HogSpec before = sm.rd_spec;
    sm.rd_spec = sp;
    if (sm.track_on && (rc = redetect_prepare(h, stream, sm.track_H, sm.track_W, sm.orient))) {
        sm.rd_spec = before;
        return rc;
    }
    const char* cap = getenv("VNECT_REDETECT_CAP");  // (tuning: tools/redetect_rate.py measures both grid shapes)
    sm.rd_cap = cap ? std::max(0, atoi(cap)) : HOG_GATED_CAP;
    sm.rd_on = true;
    return VNECT_OK;
}

int redetect_enqueue(vnect_handle* h, int stream, const FrameSrc& src, unsigned xseq, int ring, hipStream_t st)
{
    static const char* who = "re-detection";
    const Stream& sm = h->streams[stream];
    if (src.where != SRC_DEVICE && src.where != SRC_NV12) return refuse(h, who, "the frame is not whole in device memory");
    if (sm.rd_plan.empty() || src.orient != sm.rd_o || src.H != sm.rd_H || src.W != sm.rd_W)
        return fail(h, VNECT_E_INTERNAL, "re-detection: the stream's level table was not built for this frame");
    const HogPlan& p = sm.rd_plan[0];
    const HogDev d{(HogLevel*)sm.rd_buf[0], h->hog_tab, h->hog_det_dev, (float2*)sm.rd_buf[1], sm.rd_buf[2], (float*)sm.rd_buf[3], (HogHit*)sm.rd_buf[4], sm.rd_count(),
                   nullptr};
    HIPCK(h, hipMemsetAsync(d.count, 0, sizeof(unsigned), st));
    if (p.n) {  // (a picture smaller than the window has no level: nobody found)
        HogSrc a;
        memset(&a, 0, sizeof a);
        a.src = orient_src_of(src), a.o = src.orient, a.H = src.H, a.W = src.W;
        HIPCK(h, launch_hog_gated(a, p, d, sm.rd_spec.hit_threshold, sm.rd_spec.max_hits, 7, sm.rd_gate(), sm.rd_cap, st));
    }
    HIPCK(h, launch_hog_pick(d, p.n, sm.rd_spec.max_hits, (int)sm.rd_spec.final_threshold, sm.rd_gate(), (int*)sm.rd_buf[6], h->d_track + stream, xseq,
                             h->h_redet_dev + ring, st));
    return VNECT_OK;
}

}  // namespace rt
}  // namespace vnect
