// orient_probe.hip -- C shim over the oriented copies' launchers for tests/test_gpu_orient_kernels.py.  TEST INFRASTRUCTURE: it is NOT part
// of libvnect_hip.so, and the product never loads it.  `make orientprobe` links this file with the SAME orient.o the shipped library links
// (nothing of the kernels is recompiled; post.o and track.o come along for the unoriented baseline of op_time_copy).  Every case is
// validated on the host BEFORE anything is launched: a case that could make a kernel read outside the frame's allocation or write outside
// its destination gets an error code, and then nothing at all is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kernels.h"
#include "orient.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { OP_OK = 0, OP_E_FRAME = 1, OP_E_RECT = 2, OP_E_ROOM = 3 };
constexpr uint8_t DST_FILL = 0xC7;  // the canary a destination holds before its launch
constexpr int DST_GUARD = 64;       // canary bytes in front of and behind every destination (which starts 64-byte aligned, plus its phase)

}  // namespace

extern "C" {

// [0] the canary byte, [1] the guard, [2] the tile edge (orient.h)
void op_layout(int32_t* out) { out[0] = DST_FILL, out[1] = DST_GUARD, out[2] = ORIENT_T; }

// n oriented crops (rects: n x (x, y, w, h), oriented coordinates) of ONE stored (H, W) frame under code o.  `buf0` holds cap0 bytes that go
// into a device allocation of exactly cap0 bytes (`place`); pixel (0, 0) channel 0 (NV12, form 4: the Y plane) lies off0 bytes into them.
// NV12: the UV plane off1 bytes into buf1's allocation (buf1 null: into buf0's).  tracked[i]: the rect in a TrackState on the device.
// Every case has a destination of dst_cap bytes (a multiple of 64) between two guards, all pre-filled with the canary, its first byte
// `phase` (0 .. 3) bytes behind a 64-byte boundary: dst_out gets n x (DST_GUARD + dst_cap + DST_GUARD) bytes.  Returns 0, the number of
// refused cases (nothing is launched then; err says why), or < -1000 for a HIP error.
int op_copy(const uint8_t* buf0, int64_t cap0, int64_t off0, const uint8_t* buf1, int64_t cap1, int64_t off1, int flush_end, int form, int order,
            int64_t sy, int64_t sx, int64_t sc, int o, int H, int W, int n, const int32_t* rects, const int32_t* tracked, int phase, int64_t dst_cap,
            uint8_t* dst_out, int32_t* err)
{
    if (n < 1) return 0;
    int fe = OP_OK, Ho = 0, Wo = 0;
    if (!buf0 || cap0 < 1 || off0 < 0 || o < 1 || o > 7 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20) || sy < 1 || sx < 1 || sc < 1 || sy > (1 << 24) ||
        sx > (1 << 20) || sc > (1 << 28) || phase < 0 || phase > 3 || (order != INGEST_BGR && order != INGEST_RGB) || form < 0 || form > ORIENT_NV12)
        fe = OP_E_FRAME;
    else if (form == ORIENT_NV12) {
        const int64_t c1 = buf1 ? cap1 : cap0;
        if (((H | W) & 1) || sx != 1 || sy < W || sc < W || off1 < 0 || off0 + (int64_t)(H - 1) * sy + W > cap0 || off1 + (int64_t)(H / 2 - 1) * sc + W > c1 || (buf1 && cap1 < 1))
            fe = OP_E_FRAME;
    } else if ((form != INGEST_GENERIC && form != ingest_form(sx, sc)) || off0 + ingest_span(H, W, sy, sx, sc) > cap0)
        fe = OP_E_FRAME;
    if (!fe) orient_size(o, H, W, &Ho, &Wo);
    int bad = 0;
    for (int i = 0; i < n; i++) {
        const int32_t* r = rects + 4 * i;
        err[i] = fe;
        if (!err[i] && !rect_inside(r, Ho, Wo)) err[i] = OP_E_RECT;
        if (!err[i] && (dst_cap < 64 || dst_cap % 64 != 0 || 3LL * r[2] * r[3] + phase > dst_cap)) err[i] = OP_E_ROOM;
        bad += err[i] != OP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *f0 = nullptr, *lo0 = nullptr, *end0 = nullptr, *f1 = nullptr, *lo1 = nullptr, *end1 = nullptr;
    TrackState* ds = nullptr;
    Guarded dst;
    int rc = place(D, buf0, cap0, flush_end, &f0, &lo0, &end0);
    if (rc) return rc;
    if (form == ORIENT_NV12 && buf1) {
        if ((rc = place(D, buf1, cap1, flush_end, &f1, &lo1, &end1))) return rc;
    } else {
        f1 = f0, lo1 = lo0, end1 = end0;
    }
    std::vector<TrackState> hs(n);
    for (int i = 0; i < n; i++) {
        const int32_t* r = rects + 4 * i;
        memset(&hs[i], 0, sizeof(TrackState));
        hs[i].x = r[0], hs[i].y = r[1], hs[i].w = hs[i].uw = r[2], hs[i].h = hs[i].uh = r[3], hs[i].H = Ho, hs[i].W = Wo;
    }
    PROBE_HIP(D.alloc((void**)&ds, (size_t)n * sizeof(TrackState)));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(guarded(D, &dst, (size_t)dst_cap, DST_GUARD, DST_FILL, nullptr, n));
    const OrientSrc s = {f0 + off0, form == ORIENT_NV12 ? f1 + off1 : nullptr, (long long)sy, (long long)sx, (long long)sc, lo0, end0, lo1, end1, form, order};
    for (int i = 0; i < n; i++) {
        uint8_t* d = dst.data(i) + phase;
        const int32_t* r = rects + 4 * i;
        if (tracked[i]) PROBE_HIP(launch_orient_copy_track(&ds[i], s, o, H, W, d, D.st));
        else PROBE_HIP(launch_orient_copy(s, o, H, W, r[0], r[1], r[2], r[3], d, D.st));
    }
    PROBE_HIP(read_regions(D, dst, dst_out));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// The oriented copy's own duration (tools/orient_rate.py): the oriented crop `rect` of a packed BGR (nv12 = 0) or contiguous NV12 (nv12 = 1:
// Y rows, the UV rows directly behind, all W apart) frame of (H, W) pixels filled with `seed` noise -- in a device allocation, or
// (pinned) in mapped pinned host memory, which the kernel then reads over PCIe -- into a scratch slot: `reps` launches each between two
// device events, ms_out[reps].  o = 0: the UNORIENTED copy of `rect` (stored coordinates) by the copies of post.hip the product launches for
// code 0 -- launch_ingest_copy, launch_nv12_copy, and for the pinned frame launch_frame_copy of the crop's rows -- as the baseline.
int op_time_copy(int nv12, int pinned, int o, int H, int W, const int32_t* rect, int reps, float* ms_out)
{
    int Ho, Wo;
    if (o < 0 || o > 7 || H < 2 || W < 2 || H > 8192 || W > 8192 || ((H | W) & 1) || reps < 1 || reps > 10000) return OP_E_FRAME;
    orient_size(o, H, W, &Ho, &Wo);
    if (!rect_inside(rect, Ho, Wo)) return OP_E_RECT;
    const size_t bytes = nv12 ? (size_t)H * W * 3 / 2 : (size_t)H * W * 3;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *f = nullptr, *hostp = nullptr, *dst = nullptr;
    std::vector<uint8_t> noise(bytes);
    for (size_t i = 0; i < bytes; i++) noise[i] = (uint8_t)((i * 2654435761u) >> 13);
    if (pinned) {
        PROBE_HIP(D.pinned((void**)&hostp, bytes));
        memcpy(hostp, noise.data(), bytes);
        PROBE_HIP(hipHostGetDevicePointer((void**)&f, hostp, 0));
    } else {
        PROBE_HIP(D.alloc((void**)&f, bytes));
        PROBE_HIP(hipMemcpy(f, noise.data(), bytes, hipMemcpyHostToDevice));
    }
    PROBE_HIP(D.alloc((void**)&dst, (size_t)3 * rect[2] * rect[3] + 64));
    const OrientSrc s = {f, nv12 ? f + (size_t)H * W : nullptr, nv12 ? (long long)W : 3LL * W, nv12 ? 1LL : 3LL, nv12 ? (long long)W : 1LL, f, f + bytes, f, f + bytes,
                         nv12 ? (int)ORIENT_NV12 : (int)INGEST_PACKED3, INGEST_BGR};
    return timed_launches(D.st, reps, ms_out, [&](int) {
        if (o) return launch_orient_copy(s, o, H, W, rect[0], rect[1], rect[2], rect[3], dst, D.st);
        if (nv12) {
            const Nv12Src n = {f, (long long)W, f + (size_t)H * W, (long long)W, f, f + bytes};
            return launch_nv12_copy(n, rect[0], rect[1], rect[2], rect[3], dst, D.st);
        }
        if (pinned) return launch_frame_copy(f + (size_t)rect[1] * 3 * W + 3 * (size_t)rect[0], dst, rect[3], 3 * rect[2], 3LL * W, f + bytes, D.st);
        const IngestSrc g = {f, 3LL * W, 3LL, 1LL, f, f + bytes, INGEST_BGR};
        return launch_ingest_copy(g, H, W, rect[0], rect[1], rect[2], rect[3], dst, D.st);
    });
}

}  // extern "C"
