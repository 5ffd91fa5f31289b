// ingest_probe.hip -- C shim over the device-frame copies' launchers for tests/test_gpu_device_ingest_kernels.py, and a small device
// allocator for tests/test_gpu_device_frames.py (so that neither needs torch).  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so,
// and the product never loads it.  `make ingestprobe` links this file with the SAME post.o and track.o the shipped library links (nothing
// of the kernels is recompiled).  Every case is validated on the host BEFORE anything is launched: a case that could make a kernel read
// outside the frame's allocation or write outside its destination gets an error code, and then nothing at all is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "crop.h"
#include "hostplan.h"
#include "ingest.h"
#include "kernels.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { IP_OK = 0, IP_E_FRAME = 1, IP_E_RECT = 2, IP_E_ROOM = 3, IP_E_GEOM = 4 };
constexpr uint8_t DST_FILL = 0xC7;  // the canary a destination holds before its launch
constexpr int DST_GUARD = 64;       // canary bytes in front of and behind every destination (which starts 64-byte aligned, plus its phase)

int check_frame(int64_t cap, int64_t data_off, int H, int W, int64_t sy, int64_t sx, int64_t sc)
{
    return packed_fits(cap, data_off, H, W, sy, sx, sc, 1 << 20) ? IP_OK : IP_E_FRAME;
}
int check_rect(const int32_t* r, int H, int W) { return rect_inside(r, H, W) ? IP_OK : IP_E_RECT; }
TrackState state_of(const int32_t* r, int H, int W)
{
    TrackState t;
    memset(&t, 0, sizeof t);
    t.x = r[0], t.y = r[1], t.w = t.uw = r[2], t.h = t.uh = r[3], t.H = H, t.W = W;
    return t;
}

// a bounded wait on the 100 MHz clock: at most `ticks` ticks, and at most 2^24 passes whatever the clock does
__global__ void ip_spin_kernel(long long ticks, unsigned* sink)
{
    const long long t0 = wall_clock64();
    unsigned n = 0;
    while (wall_clock64() - t0 < ticks && n < (1u << 24)) n++;
    if (sink) *sink = n;
}

}  // namespace

extern "C" {

// [0] the canary byte, [1] the guard, [2] pixels per lane, [3] per wave, [4] per workgroup of the coalesced kernels, [5] per workgroup of
// the generic one (ingest.h)
void ip_layout(int32_t* out)
{
    out[0] = DST_FILL, out[1] = DST_GUARD, out[2] = INGEST_LANE_PX, out[3] = INGEST_WAVE_PX, out[4] = INGEST_WG_PX, out[5] = INGEST_GENERIC_WG_PX;
}

// n crops (rects: n x (x, y, w, h)) of ONE frame.  `buf` holds cap bytes that go into a device allocation of exactly cap bytes (`place`);
// pixel (0, 0) channel 0 lies data_off bytes into them.  mode[i]: bit 0 = the tracked kernel (the rect in a TrackState on the device; frames
// of at most 65 535 rows), bit 1 = the generic kernel whatever the strides.  Every case has a destination of dst_cap bytes (a multiple of
// 64) between two guards, all pre-filled with the canary, its first byte `phase` (0 .. 3) bytes behind a 64-byte boundary:
// dst_out gets n x (DST_GUARD + dst_cap + DST_GUARD) bytes.  Returns 0, the number of refused cases (nothing is launched then; err says
// why), or < -1000 for a HIP error.
int ip_copy(const uint8_t* buf, int64_t cap, int flush_end, int64_t data_off, int H, int W, int64_t sy, int64_t sx, int64_t sc, int order, int n,
            const int32_t* rects, const int32_t* mode, int phase, int64_t dst_cap, uint8_t* dst_out, int32_t* err)
{
    if (n < 1) return 0;
    const int fe = (order != INGEST_BGR && order != INGEST_RGB) || phase < 0 || phase > 3 ? IP_E_FRAME : check_frame(cap, data_off, H, W, sy, sx, sc);
    int bad = 0;
    for (int i = 0; i < n; i++) {
        err[i] = fe ? fe : check_rect(rects + 4 * i, H, W);
        if (!err[i] && (mode[i] & 1) && H > 65535) err[i] = IP_E_FRAME;
        if (!err[i] && (dst_cap < 64 || dst_cap % 64 != 0 || 3LL * rects[4 * i + 2] * rects[4 * i + 3] + phase > dst_cap)) err[i] = IP_E_ROOM;
        bad += err[i] != IP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *frame = nullptr, *lo = nullptr, *end = nullptr;
    TrackState* ds = nullptr;
    Guarded dst;
    int rc = place(D, buf, cap, flush_end, &frame, &lo, &end);
    if (rc) return rc;
    std::vector<TrackState> hs(n);
    for (int i = 0; i < n; i++) hs[i] = state_of(rects + 4 * i, H, W);
    PROBE_HIP(D.alloc((void**)&ds, (size_t)n * sizeof(TrackState)));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(guarded(D, &dst, (size_t)dst_cap, DST_GUARD, DST_FILL, nullptr, n));
    const IngestSrc s = {frame + data_off, (long long)sy, (long long)sx, (long long)sc, lo, end, order};
    for (int i = 0; i < n; i++) {
        uint8_t* d = dst.data(i) + phase;
        const int32_t* r = rects + 4 * i;
        if (mode[i] & 1) PROBE_HIP(launch_ingest_copy_track(&ds[i], s, d, H, W, D.st, (mode[i] >> 1) & 1));
        else PROBE_HIP(launch_ingest_copy(s, H, W, r[0], r[1], r[2], r[3], d, D.st, (mode[i] >> 1) & 1));
    }
    PROBE_HIP(read_regions(D, dst, dst_out));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// n crops of ONE NV12 frame whose planes lie in TWO device allocations of their own, each exactly its buffer's size: the Y plane y_off
// bytes into the first (rows ys apart), the UV plane uv_off bytes into the second (rows uvs apart), each plane with its own load bounds.
// mode[i] bit 0: launch_nv12_copy_track (frames of at most 131 070 rows).  Destinations as in ip_copy (phase 0).
int ip_copy_nv12(const uint8_t* ybuf, int64_t ycap, int64_t y_off, int64_t ys, const uint8_t* uvbuf, int64_t uvcap, int64_t uv_off, int64_t uvs, int H,
                 int W, int n, const int32_t* rects, const int32_t* mode, int64_t dst_cap, uint8_t* dst_out, int32_t* err)
{
    if (n < 1) return 0;
    int fe = IP_OK;
    if (ycap < 1 || uvcap < 1 || H < 2 || W < 2 || ((H | W) & 1) || H > 131070 || W > 65534 || ys < W || uvs < W || ys > (1 << 20) || uvs > (1 << 20) || y_off < 0 || uv_off < 0)
        fe = IP_E_FRAME;
    else if (y_off + (int64_t)(H - 1) * ys + W > ycap || uv_off + (int64_t)(H / 2 - 1) * uvs + W > uvcap)
        fe = IP_E_FRAME;
    int bad = 0;
    for (int i = 0; i < n; i++) {
        err[i] = fe ? fe : check_rect(rects + 4 * i, H, W);
        if (!err[i] && (dst_cap < 64 || dst_cap % 64 != 0 || 3LL * rects[4 * i + 2] * rects[4 * i + 3] > dst_cap)) err[i] = IP_E_ROOM;
        bad += err[i] != IP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *yf = nullptr, *ylo = nullptr, *yend = nullptr, *uf = nullptr, *ulo = nullptr, *uend = nullptr;
    TrackState* ds = nullptr;
    Guarded dst;
    int rc = place(D, ybuf, ycap, 1, &yf, &ylo, &yend);
    if (rc) return rc;
    if ((rc = place(D, uvbuf, uvcap, 0, &uf, &ulo, &uend))) return rc;
    std::vector<TrackState> hs(n);
    for (int i = 0; i < n; i++) hs[i] = state_of(rects + 4 * i, H, W);
    PROBE_HIP(D.alloc((void**)&ds, (size_t)n * sizeof(TrackState)));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(guarded(D, &dst, (size_t)dst_cap, DST_GUARD, DST_FILL, nullptr, n));
    Nv12Src s = {yf + y_off, (long long)ys, uf + uv_off, (long long)uvs, ylo, yend};
    s.uv_lo = ulo, s.uv_end = uend, s.any_bounds = 1;
    for (int i = 0; i < n; i++) {
        const int32_t* r = rects + 4 * i;
        if (mode[i] & 1) PROBE_HIP(launch_nv12_copy_track(&ds[i], s, dst.data(i), H, W, D.st));
        else PROBE_HIP(launch_nv12_copy(s, r[0], r[1], r[2], r[3], dst.data(i), D.st));
    }
    PROBE_HIP(read_regions(D, dst, dst_out));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// The tracked frame's way from a device frame to the input batch: launch_ingest_copy_track of the rect (in a TrackState whose geometry is
// crop.h's for the crop's size), then launch_pyramid_track with packed = 1 on what it left.  el: EL_F32 / EL_BF16 / EL_F16; out:
// (S, 368, 368, 4) elements.
int ip_pyramid(const uint8_t* buf, int64_t cap, int H, int W, int64_t sy, int64_t sx, int64_t sc, int order, const int32_t* rect, const double* scales,
               int S, int el, void* out)
{
    if (S < 1 || S > 8 || el < EL_F32 || el > EL_F16 || H > 65535) return IP_E_GEOM;
    if (check_frame(cap, 0, H, W, sy, sx, sc) || check_rect(rect, H, W)) return IP_E_RECT;
    std::vector<ScaleTabs> tabs(1);
    memset(&tabs[0], 0, sizeof(ScaleTabs));
    tabs[0].S = S;
    plan::fill_lut(tabs[0].lut);
    for (int i = 0; i < S; i++)
        if (plan::build_scale_tab(scales[i], &tabs[0], i)) return IP_E_GEOM;
    std::vector<TrackState> hs(1, state_of(rect, H, W));
    hs[0].status = crop_squarify(hs[0].h, hs[0].w, &hs[0].fp);
    if (hs[0].status != SQ_OK) return IP_E_GEOM;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    const size_t per = (size_t)S * BOX * BOX * 4 * (el == EL_F32 ? 4 : 2);
    uint8_t *frame = nullptr, *lo = nullptr, *end = nullptr, *crop = nullptr, *dout = nullptr;
    TrackState* ds = nullptr;
    ScaleTabs* dt = nullptr;
    int rc = place(D, buf, cap, 0, &frame, &lo, &end);
    if (rc) return rc;
    PROBE_HIP(D.alloc((void**)&crop, (size_t)3 * rect[2] * rect[3] + 16));
    PROBE_HIP(D.alloc((void**)&ds, sizeof(TrackState)));
    PROBE_HIP(D.alloc((void**)&dt, sizeof(ScaleTabs)));
    PROBE_HIP(D.alloc((void**)&dout, per));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dt, &tabs[0], sizeof(ScaleTabs), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemsetAsync(crop, DST_FILL, (size_t)3 * rect[2] * rect[3] + 16, D.st));
    PROBE_HIP(hipMemsetAsync(dout, 0xFF, per, D.st));
    const IngestSrc s = {frame, (long long)sy, (long long)sx, (long long)sc, lo, end, order};
    PROBE_HIP(launch_ingest_copy_track(ds, s, crop, H, W, D.st));
    FrameDyn dyn = {};
    dyn.frame = crop;
    PROBE_HIP(launch_pyramid_track(ds, dyn, 1, dt, dout, S, el, D.st));
    PROBE_HIP(hipMemcpyAsync(out, dout, per, hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// The copy kernel's own duration (tools/device_frame_rate.py): the crop `rect` of a frame already in device memory (frame_dev, inside the
// allocation hipMemGetAddressRange reports for it) into a scratch slot, `reps` launches each between two device events; ms_out[reps].
// format 2: NV12 (frame_dev = the Y plane, rows sy apart; uv_dev, rows uvs apart); otherwise order = format, strides (sy, sx, sc).
int ip_time_copy(const void* frame_dev, const void* uv_dev, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uvs, const int32_t* rect,
                 int force_generic, int reps, float* ms_out)
{
    if (!frame_dev || reps < 1 || reps > 10000 || check_rect(rect, H, W)) return IP_E_RECT;
    hipDeviceptr_t base = nullptr, ubase = nullptr;
    size_t size = 0, usize = 0;
    PROBE_HIP(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)frame_dev));
    const uint8_t *lo = (const uint8_t*)base, *end = lo + size, *f = (const uint8_t*)frame_dev;
    if (format == 2) {
        if (!uv_dev || H < 2 || W < 2 || ((H | W) & 1) || sy < W || uvs < W) return IP_E_FRAME;
        PROBE_HIP(hipMemGetAddressRange(&ubase, &usize, (hipDeviceptr_t)uv_dev));
        if ((int64_t)(end - f) < (int64_t)(H - 1) * sy + W || (int64_t)((const uint8_t*)ubase + usize - (const uint8_t*)uv_dev) < (int64_t)(H / 2 - 1) * uvs + W) return IP_E_FRAME;
    } else if (sy < 1 || sx < 1 || sc < 1 || (int64_t)(end - f) < ingest_span(H, W, sy, sx, sc)) {
        return IP_E_FRAME;
    }
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t* dst = nullptr;
    PROBE_HIP(D.alloc((void**)&dst, (size_t)3 * rect[2] * rect[3] + 64));
    const IngestSrc s = {f, (long long)sy, (long long)sx, (long long)sc, lo, end, format == 1 ? INGEST_RGB : INGEST_BGR};
    Nv12Src n = {f, (long long)sy, (const uint8_t*)uv_dev, (long long)uvs, lo, end};
    n.uv_lo = (const uint8_t*)ubase, n.uv_end = (const uint8_t*)ubase + usize, n.any_bounds = 1;
    return timed_launches(D.st, reps, ms_out, [&](int) {
        return format == 2 ? launch_nv12_copy(n, rect[0], rect[1], rect[2], rect[3], dst, D.st)
                           : launch_ingest_copy(s, H, W, rect[0], rect[1], rect[2], rect[3], dst, D.st, force_generic);
    });
}

// ---- device memory and streams for tests/test_gpu_device_frames.py -----------------------------------------------------------------------
int ip_alloc(int64_t bytes, void** p)
{
    if (bytes < 1 || !p) return IP_E_ROOM;
    PROBE_HIP(hipMalloc(p, (size_t)bytes));
    return 0;
}
int ip_free(void* p)
{
    PROBE_HIP(hipFree(p));
    return 0;
}
// the allocation `p` lies in: out[0] its base, out[1] its size (hipMemGetAddressRange)
int ip_range(const void* p, int64_t* out)
{
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    PROBE_HIP(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p));
    out[0] = (int64_t)(uintptr_t)base, out[1] = (int64_t)size;
    return 0;
}
int ip_h2d(void* dst, const void* src, int64_t n)
{
    PROBE_HIP(hipMemcpy(dst, src, (size_t)n, hipMemcpyHostToDevice));
    return 0;
}
int ip_d2h(void* dst, const void* src, int64_t n)
{
    PROBE_HIP(hipMemcpy(dst, src, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
int ip_fill(void* dst, int value, int64_t n)
{
    PROBE_HIP(hipMemset(dst, value, (size_t)n));
    return 0;
}
int ip_stream_create(void** st)
{
    PROBE_HIP(hipStreamCreateWithFlags((hipStream_t*)st, hipStreamNonBlocking));
    return 0;
}
int ip_stream_sync(void* st)
{
    PROBE_HIP(hipStreamSynchronize((hipStream_t)st));
    return 0;
}
int ip_stream_destroy(void* st)
{
    PROBE_HIP(hipStreamDestroy((hipStream_t)st));
    return 0;
}
// On `st`, without waiting: a kernel that spins `ms` milliseconds (at most 50) on the 100 MHz clock, then the copy of n bytes from
// src_dev to dst_dev (both device memory).  What reads dst_dev before that copy has run sees what dst_dev held before.
int ip_delayed_copy(void* st, void* dst_dev, const void* src_dev, int64_t n, double ms)
{
    if (!(ms >= 0) || ms > 50 || n < 1) return IP_E_GEOM;
    hipLaunchKernelGGL(ip_spin_kernel, dim3(1), dim3(1), 0, (hipStream_t)st, (long long)(ms * 1e5), (unsigned*)nullptr);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipMemcpyAsync(dst_dev, src_dev, (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)st));
    return 0;
}

}  // extern "C"
