// nv12_probe.cpp -- C shim over the NV12 copies' launchers for tests/test_gpu_nv12_kernels.py.  TEST INFRASTRUCTURE: it is NOT part of
// libvnect_hip.so, and the product never loads it.  `make nv12probe` links this file with the SAME post.o and track.o the shipped library
// links (nothing of the kernels is recompiled): batches of crops of one NV12 image in device-mapped pinned memory, one launch per crop on
// one stream, one copy back per batch.  Every case is validated on the host BEFORE anything is launched: a case that could make a kernel
// read outside the pinned buffer or write outside its destination gets an error code, and then nothing at all is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "crop.h"
#include "hostplan.h"
#include "kernels.h"
#include "nv12.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { NP_OK = 0, NP_E_FRAME = 1, NP_E_RECT = 2, NP_E_ROOM = 3, NP_E_GEOM = 4 };
constexpr uint8_t DST_FILL = 0xC7;  // the canary a destination holds before its launch
constexpr int DST_GUARD = 64;       // canary bytes in front of and behind every destination (which starts 64-byte aligned)

// an (H, W) NV12 image inside `cap` bytes: Y plane at y_off, rows ys apart; UV plane at uv_off, rows uvs apart; planes disjoint
int check_image(int64_t cap, int64_t y_off, int64_t ys, int64_t uv_off, int64_t uvs, int H, int W)
{
    if (H < 2 || W < 2 || ((H | W) & 1) || H > (1 << 20) || W > 65534 || ys < W || uvs < W || ys > (1 << 20) || uvs > (1 << 20) || y_off < 0 || uv_off < 0) return NP_E_FRAME;
    const int64_t y_end = y_off + (int64_t)(H - 1) * ys + W, uv_end = uv_off + (int64_t)(H / 2 - 1) * uvs + W;
    if (y_end > cap || uv_end > cap) return NP_E_FRAME;
    if (y_off < uv_end && uv_off < y_end) return NP_E_FRAME;
    return NP_OK;
}
int check_rect(const int32_t* r, int H, int W) { return rect_inside(r, H, W) ? NP_OK : NP_E_RECT; }
TrackState state_of(const int32_t* r, int H, int W)
{
    TrackState t;
    memset(&t, 0, sizeof t);
    t.x = r[0], t.y = r[1], t.w = t.uw = r[2], t.h = t.uh = r[3], t.H = H, t.W = W;
    return t;
}

}  // namespace

extern "C" {

// [0] the canary byte, [1] the guard, [2] pixels per lane, [3] per wave, [4] per workgroup of the kernels (nv12.h)
void np_layout(int32_t* out) { out[0] = DST_FILL, out[1] = DST_GUARD, out[2] = NV12_LANE_PX, out[3] = NV12_WAVE_PX, out[4] = NV12_WG_PX; }

// n crops (rects: n x (x, y, w, h)) of ONE NV12 image: `buf` holds cap bytes that are copied into a pinned buffer of cap rounded up to 4
// (the kernels' [lo, end)).  tracked[i] = 0: launch_nv12_copy with the rect as arguments; 1: launch_nv12_copy_track with the rect in a
// TrackState on the device (frames of at most 131 070 rows).  Every case has a destination of dst_cap bytes (a multiple of 64) between two guards, all pre-filled with
// the canary: dst_out gets n x (DST_GUARD + dst_cap + DST_GUARD) bytes.  Returns 0, the number of refused cases (nothing is launched
// then; err says why), or < -1000 for a HIP error.
int np_copy(const uint8_t* buf, int64_t cap, int64_t y_off, int64_t ys, int64_t uv_off, int64_t uvs, int H, int W, int n, const int32_t* rects,
            const int32_t* tracked, int64_t dst_cap, uint8_t* dst_out, int32_t* err)
{
    if (n < 1) return 0;
    const int fe = cap < 1 ? NP_E_FRAME : check_image(cap, y_off, ys, uv_off, uvs, H, W);
    int bad = 0;
    for (int i = 0; i < n; i++) {
        err[i] = fe ? fe : check_rect(rects + 4 * i, H, W);
        if (!err[i] && tracked[i] && H > 131070) err[i] = NP_E_FRAME;
        if (!err[i] && (dst_cap < 64 || dst_cap % 64 != 0 || 3LL * rects[4 * i + 2] * rects[4 * i + 3] > dst_cap)) err[i] = NP_E_ROOM;
        bad += err[i] != NP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    const size_t pcap = ((size_t)cap + 3) & ~(size_t)3;
    uint8_t *pin = nullptr, *pin_dev = nullptr;
    TrackState* ds = nullptr;
    Guarded dst;
    PROBE_HIP(D.pinned((void**)&pin, pcap));
    PROBE_HIP(hipHostGetDevicePointer((void**)&pin_dev, pin, 0));
    memset(pin, 0, pcap);
    memcpy(pin, buf, (size_t)cap);
    std::vector<TrackState> hs(n);
    for (int i = 0; i < n; i++) hs[i] = state_of(rects + 4 * i, H, W);
    PROBE_HIP(D.alloc((void**)&ds, (size_t)n * sizeof(TrackState)));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(guarded(D, &dst, (size_t)dst_cap, DST_GUARD, DST_FILL, nullptr, n));
    const Nv12Src s = {pin_dev + y_off, (long long)ys, pin_dev + uv_off, (long long)uvs, pin_dev, pin_dev + pcap};
    for (int i = 0; i < n; i++) {
        const int32_t* r = rects + 4 * i;
        if (tracked[i]) PROBE_HIP(launch_nv12_copy_track(&ds[i], s, dst.data(i), H, W, D.st));
        else PROBE_HIP(launch_nv12_copy(s, r[0], r[1], r[2], r[3], dst.data(i), D.st));
    }
    PROBE_HIP(read_regions(D, dst, dst_out));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// The tracked frame's way from a pinned NV12 image to the input batch: launch_nv12_copy_track of the rect (in a TrackState whose geometry
// is crop.h's for the crop's size), then launch_pyramid_track with packed = 1 on what it left.  The image is contiguous: Y rows W bytes
// apart at offset 0, the UV plane directly behind.  el: EL_F32 / EL_BF16 / EL_F16; out: (S, 368, 368, 4) elements.
int np_pyramid(const uint8_t* nv12, int H, int W, const int32_t* rect, const double* scales, int S, int el, void* out)
{
    if (S < 1 || S > 8 || el < EL_F32 || el > EL_F16) return NP_E_GEOM;
    const int64_t cap = (int64_t)H * W * 3 / 2;
    if (check_image(cap, 0, W, (int64_t)H * W, W, H, W) || check_rect(rect, H, W)) return NP_E_RECT;
    std::vector<ScaleTabs> tabs(1);
    memset(&tabs[0], 0, sizeof(ScaleTabs));
    tabs[0].S = S;
    plan::fill_lut(tabs[0].lut);
    for (int i = 0; i < S; i++)
        if (plan::build_scale_tab(scales[i], &tabs[0], i)) return NP_E_GEOM;
    std::vector<TrackState> hs(1, state_of(rect, H, W));
    hs[0].status = crop_squarify(hs[0].h, hs[0].w, &hs[0].fp);
    if (hs[0].status != SQ_OK) return NP_E_GEOM;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    const size_t pcap = ((size_t)cap + 3) & ~(size_t)3, per = (size_t)S * BOX * BOX * 4 * (el == EL_F32 ? 4 : 2);
    uint8_t *pin = nullptr, *pin_dev = nullptr, *crop = nullptr, *dout = nullptr;
    TrackState* ds = nullptr;
    ScaleTabs* dt = nullptr;
    PROBE_HIP(D.pinned((void**)&pin, pcap));
    PROBE_HIP(hipHostGetDevicePointer((void**)&pin_dev, pin, 0));
    memset(pin, 0, pcap);
    memcpy(pin, nv12, (size_t)cap);
    PROBE_HIP(D.alloc((void**)&crop, (size_t)3 * rect[2] * rect[3] + 16));
    PROBE_HIP(D.alloc((void**)&ds, sizeof(TrackState)));
    PROBE_HIP(D.alloc((void**)&dt, sizeof(ScaleTabs)));
    PROBE_HIP(D.alloc((void**)&dout, per));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dt, &tabs[0], sizeof(ScaleTabs), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemsetAsync(crop, DST_FILL, (size_t)3 * rect[2] * rect[3] + 16, D.st));
    PROBE_HIP(hipMemsetAsync(dout, 0xFF, per, D.st));
    const Nv12Src s = {pin_dev, (long long)W, pin_dev + (size_t)H * W, (long long)W, pin_dev, pin_dev + pcap};
    PROBE_HIP(launch_nv12_copy_track(ds, s, crop, H, W, D.st));
    FrameDyn dyn = {};
    dyn.frame = crop;
    PROBE_HIP(launch_pyramid_track(ds, dyn, 1, dt, dout, S, el, D.st));
    PROBE_HIP(hipMemcpyAsync(out, dout, per, hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

}  // extern "C"
