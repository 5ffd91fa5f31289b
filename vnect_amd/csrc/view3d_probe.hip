// view3d_probe.hip -- C shim over the 3-D view's launcher for tests/test_gpu_view3d_kernels.py.  TEST INFRASTRUCTURE: it is NOT part of
// libvnect_hip.so, and the product never loads it.  `make view3dprobe` links this file with the SAME view3d.o the shipped library links
// (nothing of the kernel is recompiled).  The shim allocates the output with a guard zone in front of and behind the caller's bytes,
// launches in either of the launcher's forms, and reads everything back.  Every case is validated on the host BEFORE anything is
// launched: an output whose last row would lie outside the caller's bytes gets an error code, and then nothing at all is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kernels.h"
#include "probe_util.h"
#include "view3d.h"

using namespace vnect;

namespace {

enum { VP_OK = 0, VP_E_ARG = 1 };
constexpr uint8_t GUARD_FILL = 0xC7;
constexpr int GUARD = 256;  // canary bytes in front of and behind the output's bytes (a multiple of 4: out_off alone sets the alignment)

// the inputs of a launch in either form: form 0 -- joints and confidences in device memory; form 1 -- a JointsOut and a ConfOut in pinned,
// device-mapped host memory, as a result-ring slot holds them
int place_inputs(Dev& D, int form, int status, const float* j3d, const double* conf, bool has_conf, const float** dj, const double** dc, const JointsOut** jo,
                 const ConfOut** co)
{
    *dj = nullptr, *dc = nullptr, *jo = nullptr, *co = nullptr;
    if (form == 1) {
        JointsOut* hjo = nullptr;
        ConfOut* hco = nullptr;
        PROBE_HIP(D.pinned((void**)&hjo, sizeof *hjo));
        memset(hjo, 0, sizeof *hjo);
        memcpy(hjo->j3d, j3d, sizeof hjo->j3d);
        hjo->status = status;
        void* d = nullptr;
        PROBE_HIP(hipHostGetDevicePointer(&d, hjo, 0));
        *jo = (const JointsOut*)d;
        if (has_conf) {
            PROBE_HIP(D.pinned((void**)&hco, sizeof *hco));
            memset(hco, 0, sizeof *hco);
            memcpy(hco->conf, conf, sizeof hco->conf);
            PROBE_HIP(hipHostGetDevicePointer(&d, hco, 0));
            *co = (const ConfOut*)d;
        }
        return VP_OK;
    }
    float* pj = nullptr;
    PROBE_HIP(D.alloc((void**)&pj, sizeof(float) * VIEW3D_NJ * 3));
    PROBE_HIP(hipMemcpyAsync(pj, j3d, sizeof(float) * VIEW3D_NJ * 3, hipMemcpyHostToDevice, D.st));
    *dj = pj;
    if (has_conf) {
        double* pc = nullptr;
        PROBE_HIP(D.alloc((void**)&pc, sizeof(double) * VIEW3D_NJ));
        PROBE_HIP(hipMemcpyAsync(pc, conf, sizeof(double) * VIEW3D_NJ, hipMemcpyHostToDevice, D.st));
        *dc = pc;
    }
    return VP_OK;
}

}  // namespace

extern "C" {

// [0] the guard's canary byte, [1] the guard's size, [2] the tile's width and [3] height in pixels, [4] lanes per workgroup, [5] pixels per lane
void vp_layout(int32_t* out)
{
    out[0] = GUARD_FILL, out[1] = GUARD, out[2] = VIEW3D_TILE_W, out[3] = VIEW3D_TILE_H, out[4] = VIEW3D_THREADS, out[5] = VIEW3D_LANE_PX;
}

// The arguments of view3d_capi.cpp's view3d_walk, then: form 0 / 1 (place_inputs), `status` of the ring slot (form 1; not 0: the launch must
// write nothing); guards (2 * GUARD bytes out): the canaries in front of and behind the output's bytes as they are afterwards.  `out` (its
// initial bytes in) gets the device buffer's bytes back.
int vp_view3d(const float* j3d, const double* conf, int rows, int cols, double extent, const double* view9, double line_width, const int32_t* background_bgr,
              const int32_t* colors_bgr, const int32_t* parents, double min_conf, int out_format, int order, uint8_t* out, int64_t out_size, int64_t out_off,
              int64_t out_pitch, int form, int status, uint8_t* guards)
{
    View3dArgs a;
    const View3dSpecIn s = {rows, cols, extent, view9, line_width, background_bgr, (const int (*)[3])colors_bgr, parents, min_conf, out_format, order};
    if (!j3d || !out || !guards || (form != 0 && form != 1) || view3d_setup(s, OVERLAY_PARENTS, &a)) return VP_E_ARG;
    if (out_off < 0 || out_size < 1 || out_pitch < 3LL * a.cols || out_pitch > (1 << 24)) return VP_E_ARG;
    if (out_off + (int64_t)(a.rows - 1) * out_pitch + 3LL * a.cols > out_size) return VP_E_ARG;
    if (!conf) a.has_conf = 0;
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    Guarded dout;
    PROBE_HIP(guarded(D, &dout, (size_t)out_size, GUARD, GUARD_FILL, out));
    a.out = dout.data() + out_off, a.pitch = out_pitch;
    const float* dj;
    const double* dc;
    const JointsOut* jo;
    const ConfOut* co;
    const int rc = place_inputs(D, form, status, j3d, conf, a.has_conf != 0, &dj, &dc, &jo, &co);
    if (rc) return rc;
    PROBE_HIP(launch_view3d(a, dj, dc, jo, co, D.st));
    PROBE_HIP(read_guarded(D, dout, out, guards));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return VP_OK;
}

// The kernel's own duration (tools/view3d_rate.py): n launches of a rows x cols picture of j3d at the defaults under `order`, inputs in
// device memory (form 0) or in pinned host memory (form 1), device events around each launch, ms_out[n].
int vp_time(const float* j3d, int rows, int cols, int order, int form, int n, float* ms_out)
{
    View3dArgs a;
    const View3dSpecIn s = {rows, cols, 0.0, nullptr, 0.0, nullptr, nullptr, nullptr, NAN, 0, order};
    if (!j3d || !ms_out || n < 1 || (form != 0 && form != 1) || view3d_setup(s, OVERLAY_PARENTS, &a)) return VP_E_ARG;
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t* dout = nullptr;
    PROBE_HIP(D.alloc((void**)&dout, (size_t)3 * a.rows * a.cols));
    a.out = dout, a.pitch = 3LL * a.cols, a.has_conf = 0;
    const float* dj;
    const double* dc;
    const JointsOut* jo;
    const ConfOut* co;
    const int rc = place_inputs(D, form, 0, j3d, nullptr, false, &dj, &dc, &jo, &co);
    if (rc) return rc;
    return timed_launches(D.st, n, ms_out, [&](int) { return launch_view3d(a, dj, dc, jo, co, D.st); });
}

}  // extern "C"
