// rt_view.cpp -- the 3-D view (VIEW3D.md): the reference's second window (run_estimator_ps.py:90, 124-126; src/utils.py:272-304, 317-330)
// rendered on the device by the kernel of view3d.hip.  vnect_view3d_device: one picture of caller-supplied joints into the caller's device or
// host memory, done on return.  vnect_track_view3d: a tracked stream's setting -- every tracked submit of the stream then carries its
// frame's view (enqueue_frame launches it behind the joints stage, its inputs read from the ring slot).  The specification is validated
// by view3d.h's view3d_setup, the one place that knows the defaults; a refusal changes nothing and launches nothing.
#include "runtime.h"

namespace vnect {
namespace rt {

static int refuse(vnect_handle* h, const char* who, const char* what) { return fail(h, VNECT_E_ARG, std::string(who) + ": " + what); }

// the specification (nullptr: all defaults) -> the kernel's arguments but `out` and `pitch`; has_conf: a threshold is set
static int spec_in(vnect_handle* h, const char* who, const vnect_view3d_spec* s, View3dArgs* a)
{
    View3dSpecIn in;
    memset(&in, 0, sizeof in);
    in.min_conf = NAN;
    if (s) {
        if (s->struct_size != (int32_t)sizeof(vnect_view3d_spec)) return refuse(h, who, "vnect_view3d_spec::struct_size is not sizeof(vnect_view3d_spec)");
        in.rows = s->rows, in.cols = s->cols, in.extent = s->extent, in.line_width = s->line_width;
        in.view = s->has_view ? s->view : nullptr;
        in.background_bgr = s->has_background ? s->background_bgr : nullptr;
        in.colors_bgr = s->has_colors ? s->colors_bgr : nullptr;
        in.parents = s->has_parents ? s->parents : nullptr;
        in.min_conf = s->min_confidence, in.out_format = s->out_format, in.order = s->order;
    }
    const char* bad = view3d_setup(in, OVERLAY_PARENTS, a);
    return bad ? refuse(h, who, bad) : VNECT_OK;
}

// vnect_view3d_device: on the upload stream (not a lane's); done on return
int view3d_device_impl(vnect_handle* h, const float* j3d, const double* conf, const vnect_view3d_spec* spec, void* out, int64_t out_pitch)
{
    static const char* who = "vnect_view3d_device";
    if (!j3d) return refuse(h, who, "no joints");
    if (!out) return refuse(h, who, "no output pointer");
    View3dArgs a;
    int rc = spec_in(h, who, spec, &a);
    if (rc) return rc;
    if (!conf) a.has_conf = 0;  // (a threshold without confidences applies to nothing)
    const size_t row = 3 * (size_t)a.cols;
    if (out_pitch < (int64_t)row || out_pitch > ((int64_t)1 << 32)) return refuse(h, who, "out_pitch must be at least 3 * cols");
    const size_t span = (size_t)(a.rows - 1) * (size_t)out_pitch + row;
    const uint8_t *lo = nullptr, *end = nullptr;
    const int kind = out_kind(h, out, &lo, &end);
    if (kind < 0) return refuse(h, who, "`out` is neither device memory of the handle's device nor host memory");
    if (kind == 1 && (size_t)(end - (const uint8_t*)out) < span) return refuse(h, who, "the output's last byte lies past the end of the allocation `out` points into");
    if (!h->upload_st) HIPCK(h, hipStreamCreateWithFlags(&h->upload_st, hipStreamNonBlocking));
    if (!h->view_in && (rc = dev_alloc(h, &h->view_in, VIEW3D_NJ * 3))) return rc;  // 21 doubles of confidences, then 63 floats of joints
    if (kind == 1) a.out = (uint8_t*)out, a.pitch = out_pitch;
    else {
        const size_t need = row * (size_t)a.rows;
        if (need > h->view_stage_cap) {
            HIPCK(h, hipStreamSynchronize(h->upload_st));
            if ((rc = dev_grow(h, &h->view_stage, &h->view_stage_cap, need))) return rc;
        }
        a.out = h->view_stage, a.pitch = (long long)row;
    }
    double* dconf = h->view_in;
    float* dj = (float*)(h->view_in + VIEW3D_NJ);
    HIPCK(h, hipMemcpyAsync(dj, j3d, sizeof(float) * VIEW3D_NJ * 3, hipMemcpyDefault, h->upload_st));
    if (a.has_conf) HIPCK(h, hipMemcpyAsync(dconf, conf, sizeof(double) * VIEW3D_NJ, hipMemcpyDefault, h->upload_st));
    HIPCK(h, launch_view3d(a, dj, a.has_conf ? dconf : nullptr, nullptr, nullptr, h->upload_st));
    if (kind == 0) HIPCK(h, hipMemcpy2DAsync(out, (size_t)out_pitch, h->view_stage, row, row, (size_t)a.rows, hipMemcpyDeviceToHost, h->upload_st));
    HIPCK(h, hipStreamSynchronize(h->upload_st));
    return VNECT_OK;
}

// vnect_track_view3d: the stream's setting; the ring's buffers are sized here, while nothing is in flight
int track_view3d_impl(vnect_handle* h, int stream, const vnect_view3d_spec* spec)
{
    const bool on = spec != nullptr;  // (nullptr turns the setting off; a zeroed spec with its struct_size is all defaults)
    static const char* who = "vnect_track_view3d";
    if (stream < 0 || stream >= VNECT_MAX_STREAMS) return refuse(h, who, "stream out of range");
    View3dArgs a;
    int rc;
    if (on && (rc = spec_in(h, who, spec, &a))) return rc;
    if (h->seq_submit != h->seq_collect) return fail(h, VNECT_E_STATE, std::string(who) + ": frames are in flight on the handle: collect them first");
    Stream& sm = h->streams[stream];
    if (!on) {
        sm.v3_on = false;
        return VNECT_OK;
    }
    if ((rc = ring_pictures_size(h, h->views, 3 * (size_t)a.cols * a.rows))) return rc;
    sm.v3 = a, sm.v3_on = true;
    return VNECT_OK;
}

}  // namespace rt
}  // namespace vnect
