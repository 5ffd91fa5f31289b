// rt_draw.cpp -- frames OUT: the overlay drawn into the caller's device frame (vnect_draw_device; the draw a tracked frame carries,
// vnect_submit_tracked_device_draw).  The target is validated by the device-frame resolver of rt_ingest.cpp (check_device_frame) and
// described as the kernel of overlay.hip addresses it (overlay.h: OverlayTarget); the style becomes the kernel's OverlayInput.  A refusal
// changes nothing and launches nothing.  Also the preview (vnect_preview_size / vnect_preview_device; preview.h): the same frame as a
// SOURCE that is read where it lies, annotated per tap and scaled into the caller's device or host memory.
#include "runtime.h"

namespace vnect {
namespace rt {

static int refuse(vnect_handle* h, const char* who, const char* what) { return fail(h, VNECT_E_ARG, std::string(who) + ": " + what); }

// the style (nullptr: the reference's) -> the colours of `t` in the target's own terms and the parents / threshold of `in`
static int style_in(vnect_handle* h, const char* who, const vnect_overlay_style* s, int format, OverlayTarget* t, OverlayInput* in)
{
    int limb[3], rect[3];
    for (int k = 0; k < 3; k++) limb[k] = OVERLAY_LIMB_BGR[k], rect[k] = OVERLAY_RECT_BGR[k];
    for (int i = 0; i < OVERLAY_NJ; i++) in->parents[i] = OVERLAY_PARENTS[i];
    in->min_conf = 0.0, in->has_conf = 0;
    if (s) {
        if (s->struct_size != (int32_t)sizeof(vnect_overlay_style)) return refuse(h, who, "vnect_overlay_style::struct_size is not sizeof(vnect_overlay_style)");
        for (int k = 0; k < 3; k++) {
            limb[k] = s->limb_bgr[k], rect[k] = s->rect_bgr[k];
            if (limb[k] < 0 || limb[k] > 255 || rect[k] < 0 || rect[k] > 255) return refuse(h, who, "a colour component must lie in 0 .. 255");
        }
        if (s->has_parents)
            for (int i = 0; i < OVERLAY_NJ; i++) {
                if (s->parents[i] < 0 || s->parents[i] >= OVERLAY_NJ) return refuse(h, who, "a parent must be a joint, 0 .. 20");
                in->parents[i] = s->parents[i];
            }
        if (!(s->min_confidence != s->min_confidence)) in->min_conf = s->min_confidence, in->has_conf = 1;  // (NaN: no threshold)
    }
    overlay_colours(t, format == VNECT_PIX_RGB, limb, rect);
    return VNECT_OK;
}

// Validates the target and the style and describes both; changes nothing
int check_draw(vnect_handle* h, const char* who, const vnect_device_frame* f, void* stream, const vnect_overlay_style* style, int orient, OverlayTarget* t,
               OverlayInput* in, FrameSrc* src_out)
{
    if (f && f->struct_size == (int32_t)sizeof(vnect_device_frame) && f->has_rect)
        return refuse(h, who, "the target takes no rect: the whole frame is drawn into");
    FrameSrc d;
    int rc = check_device_frame(h, f, stream, who, false, orient, &d);
    if (rc) return rc;
    if (orient && d.where == SRC_NV12)
        return refuse(h, who, "an NV12 target cannot be drawn into under an orientation other than 0 (oriented chroma addressing is not supported)");
    memset(t, 0, sizeof *t);
    memset(in, 0, sizeof *in);
    t->H = d.H, t->W = d.W;
    if (d.where == SRC_NV12) {
        t->nv12 = 1, t->data = const_cast<uint8_t*>(d.nv.y), t->sy = d.nv.y_stride, t->sx = 1, t->sc = 0;
        t->uv = const_cast<uint8_t*>(d.nv.uv), t->uv_stride = d.nv.uv_stride;
    } else {
        t->data = const_cast<uint8_t*>(d.ing.data), t->sy = d.ing.stride_y, t->sx = d.ing.stride_x, t->sc = d.ing.stride_c;
        if (orient) {
            // joints and rect are in oriented coordinates: the overlay gets the oriented VIEW of the stored frame -- oriented pixel (i, j)
            // is stored pixel orient_map(i, j), which is linear in (i, j): the origin's address, and the steps along i and j as strides
            // (signed; overlay.h addresses with signed long long throughout)
            int r0, c0, ri, ci, rj, cj;
            orient_size(orient, d.H, d.W, &t->H, &t->W);
            orient_map(orient, d.H, d.W, 0, 0, &r0, &c0);
            orient_map(orient, d.H, d.W, t->H > 1 ? 1 : 0, 0, &ri, &ci);
            orient_map(orient, d.H, d.W, 0, t->W > 1 ? 1 : 0, &rj, &cj);
            const long long sy = d.ing.stride_y, sx = d.ing.stride_x;
            t->data += r0 * sy + c0 * sx, t->sy = (ri - r0) * sy + (ci - c0) * sx, t->sx = (rj - r0) * sy + (cj - c0) * sx;
        }
    }
    if ((rc = style_in(h, who, style, f->format, t, in))) return rc;
    if (src_out) *src_out = d;
    return VNECT_OK;
}

// vnect_draw_device: on a stream of its own (the one ingest_sync uses: not a lane's compute stream), behind the producer; done on return
int draw_device_impl(vnect_handle* h, const vnect_device_frame* target, void* stream, const double* j2d, const double* conf, const int32_t* rect4,
                     const vnect_overlay_style* style)
{
    static const char* who = "vnect_draw_device";
    if (!j2d) return refuse(h, who, "no joints");
    OverlayTarget t;
    OverlayInput in;
    int rc = check_draw(h, who, target, stream, style, h->orient, &t, &in, nullptr);
    if (rc) return rc;
    if (rect4) {
        if (rect4[2] < 1 || rect4[3] < 1) return refuse(h, who, "the rect must be at least one pixel wide and high");
        for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
        in.has_rect = 1;
    }
    memcpy(in.j2d, j2d, sizeof in.j2d);
    if (conf) memcpy(in.conf, conf, sizeof in.conf);
    else in.has_conf = 0;  // (a threshold without confidences applies to nothing)
    if (!h->upload_st) HIPCK(h, hipStreamCreateWithFlags(&h->upload_st, hipStreamNonBlocking));
    if ((rc = wait_for_producer(h, stream, h->upload_st))) return rc;
    HIPCK(h, launch_overlay(t, in, nullptr, nullptr, nullptr, h->upload_st));
    HIPCK(h, hipStreamSynchronize(h->upload_st));
    return VNECT_OK;
}

// ---- the preview (preview.h; PREVIEW.md): the frame is a SOURCE here -- read where it lies, never written ---------------------------------
static int spec_in(vnect_handle* h, const char* who, const vnect_preview_spec* spec, int orient, int H, int W, PreviewGeom* g)
{
    if (!spec) return refuse(h, who, "no vnect_preview_spec");
    if (spec->struct_size != (int32_t)sizeof(vnect_preview_spec)) return refuse(h, who, "vnect_preview_spec::struct_size is not sizeof(vnect_preview_spec)");
    if (spec->out_format != VNECT_PIX_BGR && spec->out_format != VNECT_PIX_RGB) return refuse(h, who, "out_format must be VNECT_PIX_BGR or VNECT_PIX_RGB");
    const int rc = preview_geom(orient, H, W, spec->factor, g);
    if (rc != PREVIEW_OK) return refuse(h, who, preview_refusal(rc));
    return VNECT_OK;
}

int preview_size_impl(vnect_handle* h, const vnect_device_frame* f, const vnect_preview_spec* spec, int32_t* out_hw)
{
    static const char* who = "vnect_preview_size";
    if (!f) return refuse(h, who, "no frame descriptor");
    if (f->struct_size != (int32_t)sizeof(vnect_device_frame)) return refuse(h, who, "vnect_device_frame::struct_size is not sizeof(vnect_device_frame)");
    if (f->H < 1 || f->W < 1 || f->H > (1 << 24) || f->W > (1 << 24)) return refuse(h, who, "bad frame geometry");
    PreviewGeom g;
    const int rc = spec_in(h, who, spec, h->orient, f->H, f->W, &g);
    if (rc) return rc;
    out_hw[0] = g.dh, out_hw[1] = g.dw;
    return VNECT_OK;
}

// A tracked frame's preview (vnect_submit_tracked_device_preview).  With spec->draw_frame the frame is also drawn into (check_draw: an NV12
// frame under an orientation is refused then, as vnect_submit_tracked_device_draw refuses it).  The ring's buffers are sized here, before
// anything of the frame is enqueued: at the first such submit, and again for a larger preview only while nothing is in flight.
int check_tracked_preview(vnect_handle* h, const char* who, const vnect_device_frame* f, void* stream, const vnect_overlay_style* style,
                          const vnect_preview_spec* spec, int orient, FrameSrc* s)
{
    if (f && f->struct_size == (int32_t)sizeof(vnect_device_frame) && f->has_rect) return refuse(h, who, "a tracked frame takes no rect: the crop is the stream's box on the device");
    OverlayTarget t;
    OverlayInput in;
    memset(&t, 0, sizeof t);
    memset(&in, 0, sizeof in);
    int rc;
    const bool draw = spec && spec->struct_size == (int32_t)sizeof(vnect_preview_spec) && spec->draw_frame;
    if (draw) {
        if ((rc = check_draw(h, who, f, stream, style, orient, &t, &in, s))) return rc;
        s->draw = true, s->draw_target = t, s->draw_in = in;
    } else if ((rc = check_device_frame(h, f, stream, who, false, orient, s)))
        return rc;
    PreviewArgs a;
    memset(&a, 0, sizeof a);
    memset(&t, 0, sizeof t);
    memset(&in, 0, sizeof in);
    if ((rc = style_in(h, who, style, VNECT_PIX_BGR, &t, &in))) return rc;
    for (int k = 0; k < 3; k++) a.col[0][k] = t.col[0][k], a.col[1][k] = t.col[1][k];
    if ((rc = spec_in(h, who, spec, orient, s->H, s->W, &a.g))) return rc;
    const size_t need = 3 * (size_t)a.g.dw * a.g.dh;
    if (need > h->previews.cap && h->seq_submit != h->seq_collect)
        return fail(h, VNECT_E_STATE, std::string(who) + ": a larger preview needs larger buffers, which are re-sized only while nothing is in flight: collect first");
    if ((rc = ring_pictures_size(h, h->previews, need))) return rc;
    a.src = orient_src_of(*s), a.o = orient, a.H = s->H, a.W = s->W, a.out_rgb = spec->out_format == VNECT_PIX_RGB, a.has_joints = 1;
    s->preview = true, s->pv = a, s->pv_in = in;
    return VNECT_OK;
}

// where `out` lies: 1 device memory of the handle's device ([*lo, *end): its allocation), 0 host memory (pinned or pageable), -1 neither
int out_kind(vnect_handle* h, const void* p, const uint8_t** lo, const uint8_t** end)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // a pointer the runtime does not know: pageable host memory
        return 0;
    }
    if (at.isManaged) return -1;
    if (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeUnregistered) return 0;
    if (at.type != hipMemoryTypeDevice || at.device != h->cfg.device) return -1;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base || !size) {
        (void)hipGetLastError();
        return -1;
    }
    *lo = (const uint8_t*)base, *end = (const uint8_t*)base + size;
    return ((const uint8_t*)p >= *lo && (const uint8_t*)p < *end) ? 1 : -1;
}

static bool ranges_meet(const uint8_t* a, size_t na, const uint8_t* b, size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }

// vnect_preview_device: on the upload stream (not a lane's), behind the producer; done on return
int preview_device_impl(vnect_handle* h, const vnect_device_frame* f, void* stream, const double* j2d, const double* conf, const int32_t* rect4,
                        const vnect_overlay_style* style, const vnect_preview_spec* spec, void* out, int64_t out_pitch)
{
    static const char* who = "vnect_preview_device";
    if (f && f->struct_size == (int32_t)sizeof(vnect_device_frame) && f->has_rect) return refuse(h, who, "the frame takes no rect: the whole picture is scaled");
    FrameSrc d;
    int rc = check_device_frame(h, f, stream, who, false, h->orient, &d);
    if (rc) return rc;
    PreviewArgs a;
    OverlayInput in;
    OverlayTarget t;
    memset(&a, 0, sizeof a);
    memset(&in, 0, sizeof in);
    memset(&t, 0, sizeof t);
    if ((rc = style_in(h, who, style, VNECT_PIX_BGR, &t, &in))) return rc;
    for (int k = 0; k < 3; k++) a.col[0][k] = t.col[0][k], a.col[1][k] = t.col[1][k];
    if ((rc = spec_in(h, who, spec, h->orient, d.H, d.W, &a.g))) return rc;
    if (spec->draw_frame) return refuse(h, who, "draw_frame is not supported here: call vnect_draw_device to draw into the frame");
    if (rect4) {
        if (rect4[2] < 1 || rect4[3] < 1) return refuse(h, who, "the rect must be at least one pixel wide and high");
        for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
        in.has_rect = 1;
    }
    if (j2d) memcpy(in.j2d, j2d, sizeof in.j2d), a.has_joints = 1;
    if (conf) memcpy(in.conf, conf, sizeof in.conf);
    else in.has_conf = 0;  // (a threshold without confidences applies to nothing)
    if (!out) return refuse(h, who, "no output pointer");
    const size_t row = 3 * (size_t)a.g.dw;
    if (out_pitch < (int64_t)row || out_pitch > ((int64_t)1 << 32)) return refuse(h, who, "out_pitch must be at least 3 * the output's columns");
    const size_t span = (size_t)(a.g.dh - 1) * (size_t)out_pitch + row;
    const uint8_t *lo = nullptr, *end = nullptr;
    const int kind = out_kind(h, out, &lo, &end);
    if (kind < 0) return refuse(h, who, "`out` is neither device memory of the handle's device nor host memory");
    if (kind == 1) {
        if ((size_t)(end - (const uint8_t*)out) < span) return refuse(h, who, "the output's last byte lies past the end of the allocation `out` points into");
        bool meet;
        if (d.where == SRC_NV12)
            meet = ranges_meet((const uint8_t*)out, span, d.nv.y, (size_t)(d.H - 1) * d.nv.y_stride + d.W) ||
                   ranges_meet((const uint8_t*)out, span, d.nv.uv, (size_t)(d.H / 2 - 1) * d.nv.uv_stride + d.W);
        else meet = ranges_meet((const uint8_t*)out, span, d.ing.data, (size_t)ingest_span(d.H, d.W, d.ing.stride_y, d.ing.stride_x, d.ing.stride_c));
        if (meet) return refuse(h, who, "the output overlaps the frame");
    }
    a.src = orient_src_of(d), a.o = h->orient, a.H = d.H, a.W = d.W, a.out_rgb = spec->out_format == VNECT_PIX_RGB;
    if (kind == 1) a.out = (uint8_t*)out, a.pitch = out_pitch;
    else {
        const size_t need = row * (size_t)a.g.dh;
        if (need > h->preview_stage_cap) {
            if (h->upload_st) HIPCK(h, hipStreamSynchronize(h->upload_st));
            if ((rc = dev_grow(h, &h->preview_stage, &h->preview_stage_cap, need))) return rc;
        }
        a.out = h->preview_stage, a.pitch = (long long)row;
    }
    if (!h->upload_st) HIPCK(h, hipStreamCreateWithFlags(&h->upload_st, hipStreamNonBlocking));
    if ((rc = wait_for_producer(h, stream, h->upload_st))) return rc;
    HIPCK(h, launch_preview(a, in, nullptr, nullptr, nullptr, h->upload_st));
    if (kind == 0) HIPCK(h, hipMemcpy2DAsync(out, (size_t)out_pitch, h->preview_stage, row, row, (size_t)a.g.dh, hipMemcpyDeviceToHost, h->upload_st));
    HIPCK(h, hipStreamSynchronize(h->upload_st));
    return VNECT_OK;
}

}  // namespace rt
}  // namespace vnect
