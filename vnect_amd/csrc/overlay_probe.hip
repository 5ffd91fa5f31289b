// overlay_probe.hip -- C shim over the overlay's launcher for tests/test_gpu_overlay_kernels.py.  TEST INFRASTRUCTURE: it is NOT part of
// libvnect_hip.so, and the product never loads it.  `make overlayprobe` links this file with the SAME overlay.o the shipped library links
// (nothing of the kernel is recompiled).  The shim allocates a device buffer with a guard zone in front of and behind the caller's bytes,
// fills it, draws into it and reads everything back.  Every case is validated on the host BEFORE anything is launched: a frame whose last
// pixel byte would lie outside the caller's bytes gets an error code, and then nothing at all is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "crop.h"
#include "kernels.h"
#include "overlay.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { OP_OK = 0, OP_E_ARG = 1 };
constexpr uint8_t GUARD_FILL = 0xC7;
constexpr int GUARD = 256;  // canary bytes in front of and behind the caller's bytes

}  // namespace

extern "C" {

// [0] the guard's canary byte, [1] the guard's size, [2] the tile's width and [3] height in cells (a cell: one pixel, or NV12's 2 x 2
// block), [4] lanes per workgroup
void op_layout(int32_t* out) { out[0] = GUARD_FILL, out[1] = GUARD, out[2] = OVERLAY_TILE_W, out[3] = OVERLAY_TILE_H, out[4] = OVERLAY_THREADS; }

// Draws into the frame whose pixel (0, 0) channel 0 (NV12: the Y plane) lies data_off bytes into `buf` (cap bytes: the frame's initial
// bytes in, the drawn frame out), the UV plane uv_off bytes in.  format 0 BGR, 1 RGB, 2 NV12.  conf / parents / rect4 may be null.
// tracked 0: the inputs travel as the kernel's arguments (vnect_draw_device's form); 1: joints, rect, `status` and confidences are read
// from JointsOut / TrackOut / ConfOut structures in device memory (the tracked form; rect4 must be given).  guards (2 * GUARD bytes out):
// the canaries in front of and behind the caller's bytes as they are afterwards.
int op_draw(uint8_t* buf, int64_t cap, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uv_stride,
            const double* j2d, const double* conf, double min_conf, const int32_t* parents, const int32_t* rect4, const int32_t* limb_bgr,
            const int32_t* rect_bgr, int tracked, int status, uint8_t* guards)
{
    if (!buf || !j2d || !limb_bgr || !rect_bgr || !guards || !frame_fits(cap, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, 1 << 20)) return OP_E_ARG;
    if (tracked && !rect4) return OP_E_ARG;
    OverlayTarget t;
    OverlayInput in;
    memset(&t, 0, sizeof t);
    memset(&in, 0, sizeof in);
    t.H = H, t.W = W;
    if (format == 2) t.nv12 = 1, t.sy = sy, t.sx = 1, t.uv_stride = uv_stride;
    else t.sy = sy, t.sx = sx, t.sc = sc;
    int lc[3], rc[3];
    for (int k = 0; k < 3; k++) {
        lc[k] = limb_bgr[k], rc[k] = rect_bgr[k];
        if (lc[k] < 0 || lc[k] > 255 || rc[k] < 0 || rc[k] > 255) return OP_E_ARG;
    }
    overlay_colours(&t, format == 1, lc, rc);
    for (int i = 0; i < OVERLAY_NJ; i++) {
        in.parents[i] = parents ? parents[i] : OVERLAY_PARENTS[i];
        if (in.parents[i] < 0 || in.parents[i] >= OVERLAY_NJ) return OP_E_ARG;
    }
    if (conf) in.min_conf = min_conf, in.has_conf = min_conf == min_conf;
    if (rect4 && (rect4[2] < 1 || rect4[3] < 1)) return OP_E_ARG;

    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    Guarded d;
    PROBE_HIP(guarded(D, &d, (size_t)cap, GUARD, GUARD_FILL, buf));
    t.data = d.data() + data_off;
    if (t.nv12) t.uv = d.data() + uv_off;
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
    } else {
        memcpy(in.j2d, j2d, sizeof in.j2d);
        if (conf) memcpy(in.conf, conf, sizeof in.conf);
        if (rect4) {
            for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
            in.has_rect = 1;
        }
    }
    PROBE_HIP(launch_overlay(t, in, jo, to, co, D.st));
    PROBE_HIP(read_guarded(D, d, buf, guards));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return OP_OK;
}

// The kernel's own duration (tools/overlay_rate.py): n launches into a frame that already lies in device memory (data_dev; NV12: uv_dev),
// device events around each, ms_out[n].  tracked 1: the inputs are read from structures in device memory; 2: in device-mapped pinned host memory, where the tracked
// submit's launch reads them (the result ring's slots).  The caller vouches for the frame's memory (it made it with the device-frame probe's allocator).
int op_time_draw(void* data_dev, void* uv_dev, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uv_stride, const double* j2d,
                 const int32_t* rect4, int tracked, int n, float* ms_out)
{
    if (!data_dev || !j2d || !rect4 || !ms_out || n < 1 || H < 1 || W < 1 || format < 0 || format > 2 || (format == 2 && (!uv_dev || ((H | W) & 1)))) return OP_E_ARG;
    if (rect4[2] < 1 || rect4[3] < 1) return OP_E_ARG;
    OverlayTarget t;
    OverlayInput in;
    memset(&t, 0, sizeof t);
    memset(&in, 0, sizeof in);
    t.H = H, t.W = W, t.data = (uint8_t*)data_dev, t.sy = sy, t.sx = format == 2 ? 1 : sx, t.sc = format == 2 ? 0 : sc;
    if (format == 2) t.nv12 = 1, t.uv = (uint8_t*)uv_dev, t.uv_stride = uv_stride;
    overlay_colours(&t, format == 1, OVERLAY_LIMB_BGR, OVERLAY_RECT_BGR);
    for (int i = 0; i < OVERLAY_NJ; i++) in.parents[i] = OVERLAY_PARENTS[i];
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    JointsOut* jo = nullptr;
    TrackOut* to = nullptr;
    if (tracked) {
        JointsOut hjo;
        TrackOut hto;
        memset(&hjo, 0, sizeof hjo), memset(&hto, 0, sizeof hto);
        memcpy(hjo.j2d, j2d, sizeof hjo.j2d);
        for (int k = 0; k < 4; k++) hto.rect[k] = rect4[k];
        if (tracked == 2) {  // in device-mapped pinned host memory, where the result ring's slots lie
            char* hp = nullptr;
            PROBE_HIP(D.pinned((void**)&hp, 4096));
            memcpy(hp, &hjo, sizeof hjo), memcpy(hp + 2048, &hto, sizeof hto);
            char* dp = nullptr;
            PROBE_HIP(hipHostGetDevicePointer((void**)&dp, hp, 0));
            jo = (JointsOut*)dp, to = (TrackOut*)(dp + 2048);
        } else {
            PROBE_HIP(D.alloc((void**)&jo, sizeof hjo));
            PROBE_HIP(D.alloc((void**)&to, sizeof hto));
            PROBE_HIP(hipMemcpy(jo, &hjo, sizeof hjo, hipMemcpyHostToDevice));
            PROBE_HIP(hipMemcpy(to, &hto, sizeof hto, hipMemcpyHostToDevice));
        }
    } else {
        memcpy(in.j2d, j2d, sizeof in.j2d);
        for (int k = 0; k < 4; k++) in.rect[k] = rect4[k];
        in.has_rect = 1;
    }
    return timed_launches(D.st, n, ms_out, [&](int) { return launch_overlay(t, in, jo, to, nullptr, D.st); });
}

}  // extern "C"
