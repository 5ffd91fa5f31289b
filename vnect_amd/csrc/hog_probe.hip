// hog_probe.hip -- C shim over the detector's launcher for tests/test_gpu_hog_kernels.py.  TEST INFRASTRUCTURE: it is NOT part of
// libvnect_hip.so, and the product never loads it.  `make hogprobe` links this file with the SAME hog.o the shipped library links (nothing
// of the kernels is recompiled).  The shim copies the caller's source bytes into a device buffer, allocates every workspace buffer the
// launches write -- votes, bins, blocks, scores, hits, the counter -- with a guard zone in front of and behind it, launches, and reads
// everything back: the source too, so that a test can see it unchanged, and the guards, which it compares itself.  Every case is validated
// on the host BEFORE anything is launched; a picture without a level launches nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "kernels.h"
#include "hog.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { HP_OK = 0, HP_E_ARG = 1, HP_E_HITS = 2 };
constexpr uint8_t GUARD_FILL = 0xC7;
constexpr int GUARD = 256;  // canary bytes in front of and behind every workspace buffer

}  // namespace

extern "C" {

// [0] the guard's canary byte, [1] the guard's size, [2] lanes per workgroup, [3] the vote tile's width and [4] height in level pixels,
// [5] blocks / windows per workgroup
void hp_layout(int32_t* out) { out[0] = GUARD_FILL, out[1] = GUARD, out[2] = HOG_THREADS, out[3] = HOG_VTILE_W, out[4] = HOG_VTILE_H, out[5] = HOG_PER_WG; }

// The frame and the spec of hog_capi.cpp's hog_walk; uv_separate 1: the UV plane (from uv_off to the end of `src`) gets a device allocation
// of its own.  Outputs (each may be null): votes [2 npix], bins [npix], blocks [36 nblk], scores [nwin]; hits3 [3 max_hits] and hit_s
// [max_hits] in the order (level, y, x); info[4]: [0] the counter (the full number of hits), [1] launches issued (0 or 3), [2] guard bytes
// damaged, [3] the hits stored.  `src` gets the device buffer's bytes back.  Returns HP_OK; HP_E_ARG before anything is launched; HP_E_HITS
// when the counter exceeds max_hits (info is still filled, no hit is returned).
int hp_detect(uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uv_stride,
              int orient, int uv_separate, double hit_threshold, int stride_x, int stride_y, double scale0, double final_threshold, int nlevels, int max_hits,
              const float* det, int ndet, float* votes, uint8_t* bins, float* blocks, float* scores, int32_t* hits3, float* hit_s, int64_t* info)
{
    if (!src || !info || !orient_ok(orient) || !frame_fits(src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, HOG_MAX_SIDE)) return HP_E_ARG;
    if (uv_separate && (format != 2 || uv_off < data_off + (int64_t)(H - 1) * sy + W)) return HP_E_ARG;
    std::vector<float> d;
    if (!hog_detector(det, ndet, &d)) return HP_E_ARG;
    HogSpec sp;
    if (hog_spec(hit_threshold, stride_x, stride_y, scale0, final_threshold, nlevels, max_hits, &sp)) return HP_E_ARG;
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(orient, H, W, sp, &p)) return HP_E_ARG;
    info[0] = info[1] = info[2] = info[3] = 0;
    if (!p.n) return HP_OK;  // a picture smaller than the window: no level, no launch

    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t *ds = nullptr, *duv = nullptr;
    const int64_t main_size = uv_separate ? uv_off : src_size;
    PROBE_HIP(D.alloc((void**)&ds, (size_t)main_size));
    PROBE_HIP(hipMemcpyAsync(ds, src, (size_t)main_size, hipMemcpyHostToDevice, D.st));
    if (uv_separate) {
        PROBE_HIP(D.alloc((void**)&duv, (size_t)(src_size - uv_off)));
        PROBE_HIP(hipMemcpyAsync(duv, src + uv_off, (size_t)(src_size - uv_off), hipMemcpyHostToDevice, D.st));
    }
    HogTables tab;
    hog_tables(&tab);
    HogLevel* dlv = nullptr;
    HogTables* dtab = nullptr;
    float* ddet = nullptr;
    PROBE_HIP(D.alloc((void**)&dlv, sizeof(HogLevel) * p.n));
    PROBE_HIP(D.alloc((void**)&dtab, sizeof tab));
    PROBE_HIP(D.alloc((void**)&ddet, sizeof(float) * d.size()));
    PROBE_HIP(hipMemcpyAsync(dlv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dtab, &tab, sizeof tab, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(ddet, d.data(), sizeof(float) * d.size(), hipMemcpyHostToDevice, D.st));
    Guarded gv, gb, gk, gs, gh, gc;
    PROBE_HIP(guarded(D, &gv, sizeof(float2) * (size_t)p.npix, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gb, (size_t)p.npix, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gk, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gs, sizeof(float) * (size_t)p.nwin, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gh, sizeof(HogHit) * (size_t)sp.max_hits, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gc, 256, GUARD, GUARD_FILL));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(format == 2, format == 1, ds + data_off, uv_separate ? duv : ds + uv_off, sy, sx, sc, uv_stride);
    a.H = H, a.W = W, a.o = orient;
    HogDev dv{dlv, dtab, ddet, (float2*)gv.data(), gb.data(), (float*)gk.data(), (HogHit*)gh.data(), (unsigned*)gc.data(), (float*)gs.data()};
    PROBE_HIP(launch_hog(a, p, dv, sp.hit_threshold, sp.max_hits, 7, D.st));
    info[1] = 3;
    unsigned count = 0;
    PROBE_HIP(hipMemcpyAsync(&count, gc.data(), sizeof count, hipMemcpyDeviceToHost, D.st));
    if (votes) PROBE_HIP(hipMemcpyAsync(votes, gv.data(), gv.bytes, hipMemcpyDeviceToHost, D.st));
    if (bins) PROBE_HIP(hipMemcpyAsync(bins, gb.data(), gb.bytes, hipMemcpyDeviceToHost, D.st));
    if (blocks) PROBE_HIP(hipMemcpyAsync(blocks, gk.data(), gk.bytes, hipMemcpyDeviceToHost, D.st));
    if (scores) PROBE_HIP(hipMemcpyAsync(scores, gs.data(), gs.bytes, hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipMemcpyAsync(src, ds, (size_t)main_size, hipMemcpyDeviceToHost, D.st));
    if (uv_separate) PROBE_HIP(hipMemcpyAsync(src + uv_off, duv, (size_t)(src_size - uv_off), hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    info[0] = count;
    long long bad = 0;
    for (const Guarded* g : {&gv, &gb, &gk, &gs, &gh, &gc}) PROBE_HIP(guard_damage(D, *g, nullptr, &bad));
    {  // the counter's own buffer: only its first four bytes may have changed
        uint8_t z[256];
        PROBE_HIP(hipMemcpy(z, gc.data(), sizeof z, hipMemcpyDeviceToHost));
        for (int i = 4; i < 256; i++) bad += z[i] != GUARD_FILL;
    }
    info[2] = bad;
    if (count > (unsigned)sp.max_hits) {  // the hit list is full: everything behind its last entry must still be the canary, nothing is returned
        return HP_E_HITS;
    }
    std::vector<HogHit> hits(count);
    if (count) PROBE_HIP(hipMemcpy(hits.data(), gh.data(), sizeof(HogHit) * count, hipMemcpyDeviceToHost));
    std::sort(hits.begin(), hits.end(), [](const HogHit& x, const HogHit& y) { return x.level != y.level ? x.level < y.level : (x.y != y.y ? x.y < y.y : x.x < y.x); });
    for (unsigned i = 0; i < count; i++) {
        if (hits3) hits3[3 * i] = hits[i].level, hits3[3 * i + 1] = hits[i].y, hits3[3 * i + 2] = hits[i].x;
        if (hit_s) hit_s[i] = hits[i].s;
    }
    info[3] = count;
    return HP_OK;
}

// The launches' own durations (tools/hog_rate.py): n detections over an (H, W) frame the shim makes itself -- format 0: packed BGR, 2: NV12
// in one buffer -- at scale0 (0: 1.05) with a seeded detector and a threshold nothing clears, device events around each stage,
// ms_out[3 n] (votes, blocks, windows).  out[3]: levels, level pixels, windows.
int hp_time(int format, int H, int W, double scale0, int n, float* ms_out, int64_t* out)
{
    if ((format != 0 && format != 2) || !ms_out || !out || n < 1 || H < 2 || W < 2 || H > HOG_MAX_SIDE || W > HOG_MAX_SIDE || ((H | W) & 1)) return HP_E_ARG;
    HogSpec sp;
    if (hog_spec(0.0, 0, 0, scale0, 0.0, 0, 0, &sp)) return HP_E_ARG;
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(0, H, W, sp, &p) || !p.n) return HP_E_ARG;
    out[0] = p.n, out[1] = p.npix, out[2] = p.nwin;
    const size_t bytes = format == 2 ? (size_t)H * W * 3 / 2 : (size_t)H * W * 3;
    std::vector<uint8_t> host(bytes);
    for (size_t i = 0; i < bytes; i++) host[i] = (uint8_t)((i * 2654435761u >> 11) % 251);
    std::vector<float> d(HOG_DESC + 1);
    for (int i = 0; i < HOG_DESC; i++) d[i] = (float)((i * 2654435761u >> 9) % 2001) / 1000.f - 1.f;
    HogTables tab;
    hog_tables(&tab);
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t* ds = nullptr;
    HogDev dv{};
    PROBE_HIP(D.alloc((void**)&ds, bytes));
    PROBE_HIP(D.alloc((void**)&dv.lv, sizeof(HogLevel) * p.n));
    PROBE_HIP(D.alloc((void**)&dv.tab, sizeof tab));
    PROBE_HIP(D.alloc((void**)&dv.det, sizeof(float) * d.size()));
    PROBE_HIP(D.alloc((void**)&dv.votes, sizeof(float2) * (size_t)p.npix));
    PROBE_HIP(D.alloc((void**)&dv.bins, (size_t)p.npix));
    PROBE_HIP(D.alloc((void**)&dv.blocks, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk));
    PROBE_HIP(D.alloc((void**)&dv.hits, sizeof(HogHit) * (size_t)sp.max_hits));
    PROBE_HIP(D.alloc((void**)&dv.count, 256));
    PROBE_HIP(hipMemcpy(ds, host.data(), bytes, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy((void*)dv.lv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy((void*)dv.tab, &tab, sizeof tab, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy((void*)dv.det, d.data(), sizeof(float) * d.size(), hipMemcpyHostToDevice));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(format == 2, false, ds, ds + (size_t)H * W, format == 2 ? W : 3LL * W, 3, 1, W);
    a.H = H, a.W = W, a.o = 0;
    return timed_launches(D.st, n, ms_out, [&](int s) { return launch_hog(a, p, dv, 3.0e38, sp.max_hits, 1 << s, D.st); }, 3);
}

}  // extern "C"
