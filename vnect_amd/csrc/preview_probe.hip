// preview_probe.hip -- C shim over the preview's launcher for tests/test_gpu_preview_kernels.py.  TEST INFRASTRUCTURE: it is NOT part of
// libvnect_hip.so, and the product never loads it.  `make previewprobe` links this file with the SAME preview.o the shipped library links
// (nothing of the kernel is recompiled).  The shim copies the caller's source bytes into a device buffer, allocates the output with a
// guard zone in front of and behind the caller's bytes, launches, and reads everything back -- the source too, so that a test can see it
// unchanged.  Every case is validated on the host BEFORE anything is launched: a frame whose last pixel byte would lie outside the
// caller's bytes, or an output whose last row would, gets an error code, and then nothing at all is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "crop.h"
#include "kernels.h"
#include "preview.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { PP_OK = 0, PP_E_ARG = 1 };
constexpr uint8_t GUARD_FILL = 0xC7;
constexpr int GUARD = 256;  // canary bytes in front of and behind the output's bytes

constexpr int MAX_SIDE = 1 << 20;  // the largest frame side the shim takes

}  // namespace

extern "C" {

// [0] the guard's canary byte, [1] the guard's size, [2] the tile's width and [3] height in output pixels, [4] lanes per workgroup,
// [5] pixels per lane
void pp_layout(int32_t* out)
{
    out[0] = GUARD_FILL, out[1] = GUARD, out[2] = PREVIEW_TILE_W, out[3] = PREVIEW_TILE_H, out[4] = PREVIEW_THREADS, out[5] = PREVIEW_LANE_PX;
}

// The arguments of preview_capi.cpp's preview_walk, then: uv_separate 1 -- the UV plane (from uv_off to the end of `src`) gets a device
// allocation of its own; tracked 0 -- the inputs travel as the kernel's arguments (vnect_preview_device's form), 1 -- joints, rect,
// `status` and confidences are read from JointsOut / TrackOut / ConfOut structures in device memory (j2d and rect4 must be given);
// guards (2 * GUARD bytes out): the canaries in front of and behind the output's bytes as they are afterwards.  `src` gets the device
// buffer's bytes back, `out` (its initial bytes in) the output's.
int pp_preview(uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
               int64_t uv_stride, int src_has_rect, int orient, const double* j2d, const double* conf, double min_conf, const int32_t* parents,
               const int32_t* rect4, const int32_t* limb_bgr, const int32_t* rect_bgr, double factor, int out_format, uint8_t* out, int64_t out_size,
               int64_t out_off, int64_t out_pitch, int uv_separate, int tracked, int status, uint8_t* guards)
{
    if (!src || !out || !guards || src_has_rect || !orient_ok(orient)) return PP_E_ARG;
    if (!frame_fits(src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, MAX_SIDE)) return PP_E_ARG;
    if (uv_separate && (format != 2 || uv_off < data_off + (int64_t)(H - 1) * sy + W)) return PP_E_ARG;
    if (tracked && (!j2d || !rect4)) return PP_E_ARG;
    PreviewArgs a;
    OverlayInput in;
    memset(&a, 0, sizeof a);
    memset(&in, 0, sizeof in);
    if (preview_geom(orient, H, W, factor, &a.g) != PREVIEW_OK) return PP_E_ARG;
    if (out_off < 0 || out_size < 1 || (out_format != 0 && out_format != 1) || out_pitch < 3LL * a.g.dw || out_pitch > (1 << 24)) return PP_E_ARG;
    if (out_off + (int64_t)(a.g.dh - 1) * out_pitch + 3LL * a.g.dw > out_size) return PP_E_ARG;
    int lc[3], rc[3];
    for (int k = 0; k < 3; k++) {
        lc[k] = limb_bgr ? limb_bgr[k] : OVERLAY_LIMB_BGR[k], rc[k] = rect_bgr ? rect_bgr[k] : OVERLAY_RECT_BGR[k];
        if (lc[k] < 0 || lc[k] > 255 || rc[k] < 0 || rc[k] > 255) return PP_E_ARG;
    }
    preview_colours(&a, lc, rc);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        in.parents[i] = parents ? parents[i] : OVERLAY_PARENTS[i];
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return PP_E_ARG;
    }
    if (conf) in.min_conf = min_conf, in.has_conf = min_conf == min_conf;
    if (rect4 && (rect4[2] < 1 || rect4[3] < 1)) return PP_E_ARG;

    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t *ds = nullptr, *duv = nullptr;
    Guarded dout;
    const int64_t main_size = uv_separate ? uv_off : src_size;  // the bytes of the first allocation
    PROBE_HIP(D.alloc((void**)&ds, (size_t)main_size));
    PROBE_HIP(hipMemcpyAsync(ds, src, (size_t)main_size, hipMemcpyHostToDevice, D.st));
    if (uv_separate) {
        PROBE_HIP(D.alloc((void**)&duv, (size_t)(src_size - uv_off)));
        PROBE_HIP(hipMemcpyAsync(duv, src + uv_off, (size_t)(src_size - uv_off), hipMemcpyHostToDevice, D.st));
    }
    PROBE_HIP(guarded(D, &dout, (size_t)out_size, GUARD, GUARD_FILL, out));
    a.src = preview_source(format == 2, format == 1, ds + data_off, uv_separate ? duv : ds + uv_off, sy, sx, sc, uv_stride);
    a.H = H, a.W = W, a.o = orient;
    a.out = dout.data() + out_off, a.pitch = out_pitch, a.out_rgb = out_format;
    JointsOut* jo = nullptr;
    TrackOut* to = nullptr;
    ConfOut* co = nullptr;
    JointsOut hjo;
    TrackOut hto;
    ConfOut hco;
    if (tracked) {
        memset(&hjo, 0, sizeof hjo), memset(&hto, 0, sizeof hto), memset(&hco, 0, sizeof hco);
        memcpy(hjo.j2d, j2d, sizeof hjo.j2d);
        for (int k = 0; k < 4; k++) hto.rect[k] = rect4[k];
        hto.status = status;
        if (conf) memcpy(hco.conf, conf, sizeof hco.conf);
        PROBE_HIP(D.alloc((void**)&jo, sizeof hjo));
        PROBE_HIP(D.alloc((void**)&to, sizeof hto));
        PROBE_HIP(hipMemcpyAsync(jo, &hjo, sizeof hjo, hipMemcpyHostToDevice, D.st));
        PROBE_HIP(hipMemcpyAsync(to, &hto, sizeof hto, hipMemcpyHostToDevice, D.st));
        if (in.has_conf) {
            PROBE_HIP(D.alloc((void**)&co, sizeof hco));
            PROBE_HIP(hipMemcpyAsync(co, &hco, sizeof hco, hipMemcpyHostToDevice, D.st));
        }
        a.has_joints = 1;
    } else {
        if (j2d) memcpy(in.j2d, j2d, sizeof in.j2d), a.has_joints = 1;
        if (conf) memcpy(in.conf, conf, sizeof in.conf);
        if (rect4) {
            for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
            in.has_rect = 1;
        }
    }
    PROBE_HIP(launch_preview(a, in, jo, to, co, D.st));
    PROBE_HIP(read_guarded(D, dout, out, guards));
    PROBE_HIP(hipMemcpyAsync(src, ds, (size_t)main_size, hipMemcpyDeviceToHost, D.st));
    if (uv_separate) PROBE_HIP(hipMemcpyAsync(src + uv_off, duv, (size_t)(src_size - uv_off), hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return PP_OK;
}

// The people form (launch_preview_people; tests/test_gpu_people_kernels.py): preview_capi.cpp's preview_walk_people's arguments, with
// `status` (P ints, SQ_OK = 0: drawn) in the place of its `drawn`, then guards as in pp_preview.  Every person's joints, rect, status and
// confidences lie in JointsOut / TrackOut / ConfOut structures in device memory, as the runtime's ring slots do.
int pp_preview_people(uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc,
                      int64_t uv_stride, int orient, int P, const double* j2d, const double* conf, double min_conf, const int32_t* parents,
                      const int32_t* rects, const int32_t* status, const int32_t* limb_bgr, const int32_t* rect_bgr, double factor, int out_format,
                      uint8_t* out, int64_t out_size, int64_t out_off, int64_t out_pitch, uint8_t* guards)
{
    if (!src || !out || !guards || !j2d || !rects || !status || P < 1 || P > PREVIEW_MAX_PEOPLE) return PP_E_ARG;
    if (!orient_ok(orient) || !frame_fits(src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, MAX_SIDE)) return PP_E_ARG;
    PreviewArgs a;
    OverlayInput in;
    memset(&a, 0, sizeof a);
    memset(&in, 0, sizeof in);
    if (preview_geom(orient, H, W, factor, &a.g) != PREVIEW_OK) return PP_E_ARG;
    if (out_off < 0 || out_size < 1 || (out_format != 0 && out_format != 1) || out_pitch < 3LL * a.g.dw || out_pitch > (1 << 24)) return PP_E_ARG;
    if (out_off + (int64_t)(a.g.dh - 1) * out_pitch + 3LL * a.g.dw > out_size) return PP_E_ARG;
    int lc[3], rc[3];
    for (int k = 0; k < 3; k++) {
        lc[k] = limb_bgr ? limb_bgr[k] : OVERLAY_LIMB_BGR[k], rc[k] = rect_bgr ? rect_bgr[k] : OVERLAY_RECT_BGR[k];
        if (lc[k] < 0 || lc[k] > 255 || rc[k] < 0 || rc[k] > 255) return PP_E_ARG;
    }
    preview_colours(&a, lc, rc);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        in.parents[i] = parents ? parents[i] : OVERLAY_PARENTS[i];
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return PP_E_ARG;
    }
    if (conf) in.min_conf = min_conf, in.has_conf = min_conf == min_conf;
    for (int p = 0; p < P; p++)
        if (rects[4 * p + 2] < 1 || rects[4 * p + 3] < 1) return PP_E_ARG;
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t* ds = nullptr;
    Guarded dout;
    PROBE_HIP(D.alloc((void**)&ds, (size_t)src_size));
    PROBE_HIP(hipMemcpyAsync(ds, src, (size_t)src_size, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(guarded(D, &dout, (size_t)out_size, GUARD, GUARD_FILL, out));
    a.src = preview_source(format == 2, format == 1, ds + data_off, ds + uv_off, sy, sx, sc, uv_stride);
    a.H = H, a.W = W, a.o = orient, a.has_joints = 1;
    a.out = dout.data() + out_off, a.pitch = out_pitch, a.out_rgb = out_format;
    std::vector<JointsOut> hjo(P);
    std::vector<TrackOut> hto(P);
    std::vector<ConfOut> hco(P);
    PreviewPeopleIn pin;
    memset(&pin, 0, sizeof pin);
    pin.P = P;
    JointsOut* djo = nullptr;
    TrackOut* dto = nullptr;
    ConfOut* dco = nullptr;
    PROBE_HIP(D.alloc((void**)&djo, P * sizeof(JointsOut)));
    PROBE_HIP(D.alloc((void**)&dto, P * sizeof(TrackOut)));
    PROBE_HIP(D.alloc((void**)&dco, P * sizeof(ConfOut)));
    for (int p = 0; p < P; p++) {
        memset(&hjo[p], 0, sizeof(JointsOut)), memset(&hto[p], 0, sizeof(TrackOut)), memset(&hco[p], 0, sizeof(ConfOut));
        memcpy(hjo[p].j2d, j2d + p * OVERLAY_NJ * 2, sizeof hjo[p].j2d);
        for (int k = 0; k < 4; k++) hto[p].rect[k] = rects[4 * p + k];
        hto[p].status = status[p];
        if (conf) memcpy(hco[p].conf, conf + p * OVERLAY_NJ, sizeof hco[p].conf);
        pin.jo[p] = djo + p, pin.to[p] = dto + p, pin.co[p] = in.has_conf ? dco + p : nullptr;
    }
    PROBE_HIP(hipMemcpyAsync(djo, hjo.data(), P * sizeof(JointsOut), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dto, hto.data(), P * sizeof(TrackOut), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dco, hco.data(), P * sizeof(ConfOut), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(launch_preview_people(a, in, pin, D.st));
    PROBE_HIP(read_guarded(D, dout, out, guards));
    PROBE_HIP(hipMemcpyAsync(src, ds, (size_t)src_size, hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return PP_OK;
}

// The kernel's own duration (tools/preview_rate.py): n launches over an (H, W) frame the shim makes itself -- format 0: packed BGR,
// 2: NV12 in one buffer -- under `orient` at `factor`, with a fan of limbs around the picture's centre and a rect a twentieth in from its
// border, device events around each launch, ms_out[n].  out_hw: the output's size.
int pp_time(int format, int H, int W, int orient, double factor, int n, float* ms_out, int32_t* out_hw)
{
    if ((format != 0 && format != 2) || !ms_out || !out_hw || n < 1 || H < 2 || W < 2 || H > 8192 || W > 8192 || ((H | W) & 1) || !orient_ok(orient)) return PP_E_ARG;
    PreviewArgs a;
    OverlayInput in;
    memset(&a, 0, sizeof a);
    memset(&in, 0, sizeof in);
    if (preview_geom(orient, H, W, factor, &a.g) != PREVIEW_OK) return PP_E_ARG;
    out_hw[0] = a.g.dh, out_hw[1] = a.g.dw;
    const size_t bytes = format == 2 ? (size_t)H * W * 3 / 2 : (size_t)H * W * 3;
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t *ds = nullptr, *dout = nullptr;
    PROBE_HIP(D.alloc((void**)&ds, bytes));
    PROBE_HIP(hipMemsetAsync(ds, 0x5A, bytes, D.st));
    PROBE_HIP(D.alloc((void**)&dout, (size_t)a.g.dh * a.g.dw * 3));
    a.src = preview_source(format == 2, false, ds, ds + (size_t)H * W, format == 2 ? W : 3LL * W, 3, 1, W);
    a.H = H, a.W = W, a.o = orient, a.out = dout, a.pitch = 3LL * a.g.dw, a.has_joints = 1;
    preview_colours(&a, nullptr, nullptr);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        in.parents[i] = OVERLAY_PARENTS[i];
        in.j2d[2 * i] = a.g.Hp * (0.5 + 0.35 * ((i * 7) % 11 - 5) / 5.0), in.j2d[2 * i + 1] = a.g.Wp * (0.5 + 0.12 * ((i * 5) % 9 - 4) / 4.0);
    }
    in.has_rect = 1, in.rect[0] = a.g.Wp / 20, in.rect[1] = a.g.Hp / 20, in.rect[2] = a.g.Wp - a.g.Wp / 10, in.rect[3] = a.g.Hp - a.g.Hp / 10;
    return timed_launches(D.st, n, ms_out, [&](int) { return launch_preview(a, in, nullptr, nullptr, nullptr, D.st); });
}

}  // extern "C"
