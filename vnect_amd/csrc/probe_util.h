// probe_util.h -- what every kernel probe (*_probe.cpp / *_probe.hip) needs around its launches.  TEST INFRASTRUCTURE: nothing that
// libvnect_hip.so links may include it.  Free functions and two small structs: the HIP error mapping, the allocations of one call, a
// buffer between guard zones, a buffer flush against an end of its allocation, the checks that a frame and a rect fit, and the timed loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ingest.h"  // ingest_span

namespace vnect {

// a HIP error ends the entry point with -(error) - 1000
#define PROBE_HIP(x)                                  \
    do {                                              \
        const hipError_t e_ = (x);                    \
        if (e_ != hipSuccess) return -(int)e_ - 1000; \
    } while (0)

struct Dev {  // the stream and the device / pinned allocations of one call, freed however it ends
    std::vector<void*> dev, host;
    hipStream_t st = nullptr;
    ~Dev()
    {
        if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
        for (void* p : dev) (void)hipFree(p);
        for (void* p : host) (void)hipHostFree(p);
    }
    hipError_t alloc(void** p, size_t n)
    {
        const hipError_t e = hipMalloc(p, n ? n : 1);
        if (e == hipSuccess) dev.push_back(*p);
        return e;
    }
    hipError_t pinned(void** p, size_t n)  // device-mapped: hipHostGetDevicePointer gives the address a kernel reads it at
    {
        const hipError_t e = hipHostMalloc(p, n ? n : 4, hipHostMallocMapped);
        if (e == hipSuccess) host.push_back(*p);
        return e;
    }
};

// n regions in one allocation, each `bytes` of payload between two guards of `guard` bytes
struct Guarded {
    uint8_t* base = nullptr;
    size_t bytes = 0, guard = 0, n = 1;
    uint8_t fill = 0;
    size_t region() const { return bytes + 2 * guard; }
    uint8_t* data(size_t i = 0) const { return base + i * region() + guard; }
};
// allocates g and fills all of it with the canary `fill`; `init` (may be null): `bytes` that then go behind region 0's front guard
inline hipError_t guarded(Dev& D, Guarded* g, size_t bytes, int guard, uint8_t fill, const void* init = nullptr, size_t n = 1)
{
    g->bytes = bytes, g->guard = (size_t)guard, g->n = n, g->fill = fill;
    hipError_t e = D.alloc((void**)&g->base, n * g->region());
    if (e == hipSuccess) e = hipMemsetAsync(g->base, fill, n * g->region(), D.st);
    if (e == hipSuccess && init) e = hipMemcpyAsync(g->data(), init, bytes, hipMemcpyHostToDevice, D.st);
    return e;
}
// region 0 back, on the stream and without waiting: the payload into `out` (may be null), the guards in front of and behind it into
// guards[2 * guard]
inline hipError_t read_guarded(Dev& D, const Guarded& g, void* out, uint8_t* guards)
{
    hipError_t e = out && g.bytes ? hipMemcpyAsync(out, g.data(), g.bytes, hipMemcpyDeviceToHost, D.st) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(guards, g.base, g.guard, hipMemcpyDeviceToHost, D.st);
    if (e == hipSuccess) e = hipMemcpyAsync(guards + g.guard, g.data() + g.bytes, g.guard, hipMemcpyDeviceToHost, D.st);
    return e;
}
// the same, waited for: *bad grows by the guard bytes of region 0 that are no longer the canary
inline hipError_t guard_damage(Dev& D, const Guarded& g, void* out, long long* bad)
{
    std::vector<uint8_t> z(2 * g.guard);
    hipError_t e = read_guarded(D, g, out, z.data());
    if (e == hipSuccess) e = hipStreamSynchronize(D.st);
    for (uint8_t v : z) *bad += e == hipSuccess && v != g.fill;
    return e;
}
// all n regions, guards and payloads as they lie, into out[n * region()], on the stream and without waiting
inline hipError_t read_regions(Dev& D, const Guarded& g, uint8_t* out)
{
    return hipMemcpyAsync(out, g.base, g.n * g.region(), hipMemcpyDeviceToHost, D.st);
}

// `buf` (cap bytes) into an allocation of its own of exactly cap bytes (rounded up only as hipMalloc rounds): flush against the start of
// the allocation's address range, or (flush_end) against its end.  lo / end: the range as hipMemGetAddressRange reports it.
inline int place(Dev& D, const uint8_t* buf, int64_t cap, int flush_end, uint8_t** frame, uint8_t** lo, uint8_t** end)
{
    uint8_t* a = nullptr;
    PROBE_HIP(D.alloc((void**)&a, (size_t)cap));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    PROBE_HIP(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)a));
    if ((uint8_t*)base > a || size < (size_t)cap + (size_t)(a - (uint8_t*)base)) return -999;
    *lo = (uint8_t*)base, *end = (uint8_t*)base + size;
    *frame = flush_end ? *end - cap : *lo;
    PROBE_HIP(hipMemsetAsync(base, 0x5A, size, D.st));
    PROBE_HIP(hipMemcpyAsync(*frame, buf, (size_t)cap, hipMemcpyHostToDevice, D.st));
    return 0;
}

// a packed (H, W, 3) frame of sides up to max_side, strides (sy, sx, sc), pixel (0, 0) channel 0 data_off bytes into `size` bytes
inline bool packed_fits(int64_t size, int64_t data_off, int H, int W, int64_t sy, int64_t sx, int64_t sc, int max_side)
{
    if (size < 1 || H < 1 || W < 1 || H > max_side || W > max_side || data_off < 0) return false;
    if (sy < 1 || sx < 1 || sc < 1 || sy > (1 << 24) || sx > (1 << 20) || sc > (1 << 28)) return false;
    return data_off + ingest_span(H, W, sy, sx, sc) <= size;
}
// format 0 / 1: that packed frame; 2: an NV12 frame, Y rows sy apart from data_off, UV rows uv_stride apart from uv_off
inline bool frame_fits(int64_t size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uv_stride,
                       int max_side)
{
    if (format != 2) return (format == 0 || format == 1) && packed_fits(size, data_off, H, W, sy, sx, sc, max_side);
    if (size < 1 || H < 1 || W < 1 || H > max_side || W > max_side || data_off < 0) return false;
    if (((H | W) & 1) || sy < W || uv_stride < W || uv_off < 0 || sy > (1 << 24) || uv_stride > (1 << 24)) return false;
    return data_off + (int64_t)(H - 1) * sy + W <= size && uv_off + (int64_t)(H / 2 - 1) * uv_stride + W <= size;
}
// the rect r = (x, y, w, h) is not empty and lies inside an (H, W) frame
inline bool rect_inside(const int32_t* r, int H, int W)
{
    return r[0] >= 0 && r[1] >= 0 && r[2] >= 1 && r[3] >= 1 && (int64_t)r[0] + r[2] <= W && (int64_t)r[1] + r[3] <= H;
}

// What tools/*_rate.py measure with: three warm-up rounds, then n rounds of `stages` launches -- launch(s) returns a hipError_t -- with a
// device event in front of the first and behind each, a synchronise per round; ms_out[stages * i + s] is stage s of round i.  The first
// HIP error ends the loop.
template <class Launch>
int timed_launches(hipStream_t st, int n, float* ms_out, Launch launch, int stages = 1)
{
    std::vector<hipEvent_t> ev(stages + 1, nullptr);
    hipError_t e = hipSuccess;
    for (int s = 0; s <= stages && e == hipSuccess; s++) e = hipEventCreate(&ev[s]);
    for (int i = -3; i < n && e == hipSuccess; i++) {
        e = hipEventRecord(ev[0], st);
        for (int s = 0; s < stages && e == hipSuccess; s++) {
            e = launch(s);
            if (e == hipSuccess) e = hipEventRecord(ev[s + 1], st);
        }
        if (e == hipSuccess) e = hipEventSynchronize(ev[stages]);
        for (int s = 0; s < stages && e == hipSuccess; s++) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, ev[s], ev[s + 1]);
            if (e == hipSuccess && i >= 0) ms_out[stages * i + s] = ms;
        }
    }
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    PROBE_HIP(e);
    return 0;
}

}  // namespace vnect
