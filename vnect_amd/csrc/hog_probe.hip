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

using namespace vnect;

namespace {

enum { HP_OK = 0, HP_E_ARG = 1, HP_E_HITS = 2 };
constexpr uint8_t GUARD_FILL = 0xC7;
constexpr int GUARD = 256;  // canary bytes in front of and behind every workspace buffer

#define HP_HIP(x)                                     \
    do {                                              \
        const hipError_t e_ = (x);                    \
        if (e_ != hipSuccess) return -(int)e_ - 1000; \
    } while (0)

struct Dev {  // device allocations of one call, freed however it ends
    std::vector<void*> dev;
    hipStream_t st = nullptr;
    ~Dev()
    {
        if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
        for (void* p : dev) (void)hipFree(p);
    }
    hipError_t alloc(void** p, size_t n)
    {
        const hipError_t e = hipMalloc(p, n ? n : 1);
        if (e == hipSuccess) dev.push_back(*p);
        return e;
    }
};

// a workspace buffer of `bytes` between two guards, all canary
struct Guarded {
    uint8_t* base = nullptr;
    size_t bytes = 0;
    uint8_t* data() const { return base + GUARD; }
};
int guarded(Dev& D, Guarded* g, size_t bytes)
{
    g->bytes = bytes;
    HP_HIP(D.alloc((void**)&g->base, bytes + 2 * GUARD));
    HP_HIP(hipMemsetAsync(g->base, GUARD_FILL, bytes + 2 * GUARD, D.st));
    return 0;
}
// how many guard bytes of g are no longer the canary
int guard_damage(Dev& D, const Guarded& g, long long* bad)
{
    uint8_t z[2 * GUARD];
    HP_HIP(hipMemcpyAsync(z, g.base, GUARD, hipMemcpyDeviceToHost, D.st));
    HP_HIP(hipMemcpyAsync(z + GUARD, g.base + GUARD + g.bytes, GUARD, hipMemcpyDeviceToHost, D.st));
    HP_HIP(hipStreamSynchronize(D.st));
    for (uint8_t v : z) *bad += v != GUARD_FILL;
    return 0;
}

bool frame_ok(int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uv_stride, int orient)
{
    if (src_size < 1 || H < 1 || W < 1 || H > HOG_MAX_SIDE || W > HOG_MAX_SIDE || data_off < 0 || format < 0 || format > 2 || !orient_ok(orient)) return false;
    if (format == 2) {
        if (((H | W) & 1) || sy < W || uv_stride < W || uv_off < 0 || sy > (1 << 24) || uv_stride > (1 << 24)) return false;
        return data_off + (int64_t)(H - 1) * sy + W <= src_size && uv_off + (int64_t)(H / 2 - 1) * uv_stride + W <= src_size;
    }
    if (sy < 1 || sx < 1 || sc < 1 || sy > (1 << 24) || sx > (1 << 20) || sc > (1 << 28)) return false;
    return data_off + ingest_span(H, W, sy, sx, sc) <= src_size;
}

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
    if (!src || !info || !frame_ok(src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, orient)) return HP_E_ARG;
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
    HP_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t *ds = nullptr, *duv = nullptr;
    const int64_t main_size = uv_separate ? uv_off : src_size;
    HP_HIP(D.alloc((void**)&ds, (size_t)main_size));
    HP_HIP(hipMemcpyAsync(ds, src, (size_t)main_size, hipMemcpyHostToDevice, D.st));
    if (uv_separate) {
        HP_HIP(D.alloc((void**)&duv, (size_t)(src_size - uv_off)));
        HP_HIP(hipMemcpyAsync(duv, src + uv_off, (size_t)(src_size - uv_off), hipMemcpyHostToDevice, D.st));
    }
    HogTables tab;
    hog_tables(&tab);
    HogLevel* dlv = nullptr;
    HogTables* dtab = nullptr;
    float* ddet = nullptr;
    HP_HIP(D.alloc((void**)&dlv, sizeof(HogLevel) * p.n));
    HP_HIP(D.alloc((void**)&dtab, sizeof tab));
    HP_HIP(D.alloc((void**)&ddet, sizeof(float) * d.size()));
    HP_HIP(hipMemcpyAsync(dlv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice, D.st));
    HP_HIP(hipMemcpyAsync(dtab, &tab, sizeof tab, hipMemcpyHostToDevice, D.st));
    HP_HIP(hipMemcpyAsync(ddet, d.data(), sizeof(float) * d.size(), hipMemcpyHostToDevice, D.st));
    Guarded gv, gb, gk, gs, gh, gc;
    int rc;
    if ((rc = guarded(D, &gv, sizeof(float2) * (size_t)p.npix)) || (rc = guarded(D, &gb, (size_t)p.npix)) ||
        (rc = guarded(D, &gk, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk)) || (rc = guarded(D, &gs, sizeof(float) * (size_t)p.nwin)) ||
        (rc = guarded(D, &gh, sizeof(HogHit) * (size_t)sp.max_hits)) || (rc = guarded(D, &gc, 256)))
        return rc;
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(format == 2, format == 1, ds + data_off, uv_separate ? duv : ds + uv_off, sy, sx, sc, uv_stride);
    a.H = H, a.W = W, a.o = orient;
    HogDev dv{dlv, dtab, ddet, (float2*)gv.data(), gb.data(), (float*)gk.data(), (HogHit*)gh.data(), (unsigned*)gc.data(), (float*)gs.data()};
    HP_HIP(launch_hog(a, p, dv, sp.hit_threshold, sp.max_hits, 7, D.st));
    info[1] = 3;
    unsigned count = 0;
    HP_HIP(hipMemcpyAsync(&count, gc.data(), sizeof count, hipMemcpyDeviceToHost, D.st));
    if (votes) HP_HIP(hipMemcpyAsync(votes, gv.data(), gv.bytes, hipMemcpyDeviceToHost, D.st));
    if (bins) HP_HIP(hipMemcpyAsync(bins, gb.data(), gb.bytes, hipMemcpyDeviceToHost, D.st));
    if (blocks) HP_HIP(hipMemcpyAsync(blocks, gk.data(), gk.bytes, hipMemcpyDeviceToHost, D.st));
    if (scores) HP_HIP(hipMemcpyAsync(scores, gs.data(), gs.bytes, hipMemcpyDeviceToHost, D.st));
    HP_HIP(hipMemcpyAsync(src, ds, (size_t)main_size, hipMemcpyDeviceToHost, D.st));
    if (uv_separate) HP_HIP(hipMemcpyAsync(src + uv_off, duv, (size_t)(src_size - uv_off), hipMemcpyDeviceToHost, D.st));
    HP_HIP(hipStreamSynchronize(D.st));
    info[0] = count;
    long long bad = 0;
    for (const Guarded* g : {&gv, &gb, &gk, &gs, &gh, &gc})
        if ((rc = guard_damage(D, *g, &bad))) return rc;
    {  // the counter's own buffer: only its first four bytes may have changed
        uint8_t z[256];
        HP_HIP(hipMemcpy(z, gc.data(), sizeof z, hipMemcpyDeviceToHost));
        for (int i = 4; i < 256; i++) bad += z[i] != GUARD_FILL;
    }
    info[2] = bad;
    if (count > (unsigned)sp.max_hits) {  // the hit list is full: everything behind its last entry must still be the canary, nothing is returned
        return HP_E_HITS;
    }
    std::vector<HogHit> hits(count);
    if (count) HP_HIP(hipMemcpy(hits.data(), gh.data(), sizeof(HogHit) * count, hipMemcpyDeviceToHost));
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
    HP_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t* ds = nullptr;
    HogDev dv{};
    HP_HIP(D.alloc((void**)&ds, bytes));
    HP_HIP(D.alloc((void**)&dv.lv, sizeof(HogLevel) * p.n));
    HP_HIP(D.alloc((void**)&dv.tab, sizeof tab));
    HP_HIP(D.alloc((void**)&dv.det, sizeof(float) * d.size()));
    HP_HIP(D.alloc((void**)&dv.votes, sizeof(float2) * (size_t)p.npix));
    HP_HIP(D.alloc((void**)&dv.bins, (size_t)p.npix));
    HP_HIP(D.alloc((void**)&dv.blocks, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk));
    HP_HIP(D.alloc((void**)&dv.hits, sizeof(HogHit) * (size_t)sp.max_hits));
    HP_HIP(D.alloc((void**)&dv.count, 256));
    HP_HIP(hipMemcpy(ds, host.data(), bytes, hipMemcpyHostToDevice));
    HP_HIP(hipMemcpy((void*)dv.lv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice));
    HP_HIP(hipMemcpy((void*)dv.tab, &tab, sizeof tab, hipMemcpyHostToDevice));
    HP_HIP(hipMemcpy((void*)dv.det, d.data(), sizeof(float) * d.size(), hipMemcpyHostToDevice));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(format == 2, false, ds, ds + (size_t)H * W, format == 2 ? W : 3LL * W, 3, 1, W);
    a.H = H, a.W = W, a.o = 0;
    hipEvent_t ev[4];
    for (hipEvent_t& e : ev) HP_HIP(hipEventCreate(&e));
    int rc = HP_OK;
    for (int i = -2; i < n && rc == HP_OK; i++) {  // (two warm-up rounds)
        hipError_t e = hipEventRecord(ev[0], D.st);
        for (int s = 0; s < 3 && e == hipSuccess; s++) {
            e = launch_hog(a, p, dv, 3.0e38, sp.max_hits, 1 << s, D.st);
            if (e == hipSuccess) e = hipEventRecord(ev[s + 1], D.st);
        }
        if (e == hipSuccess) e = hipEventSynchronize(ev[3]);
        for (int s = 0; s < 3 && e == hipSuccess; s++) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, ev[s], ev[s + 1]);
            if (i >= 0) ms_out[3 * i + s] = ms;
        }
        if (e != hipSuccess) rc = -(int)e - 1000;
    }
    for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
