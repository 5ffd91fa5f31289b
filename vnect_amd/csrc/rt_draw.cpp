// rt_draw.cpp -- frames OUT: the overlay drawn into the caller's device frame (vnect_draw_device; the draw a tracked frame carries,
// vnect_submit_tracked_device_draw).  The target is validated by the device-frame resolver of rt_ingest.cpp (check_device_frame) and
// described as the kernel of overlay.hip addresses it (overlay.h: OverlayTarget); the style becomes the kernel's OverlayInput.  A refusal
// changes nothing and launches nothing.
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

}  // namespace rt
}  // namespace vnect
