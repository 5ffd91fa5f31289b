// redetect_probe.hip -- C shim over the launchers of a re-detection (launch_hog_gated, launch_hog_pick) for
// tests/test_gpu_redetect_kernels.py and tools/redetect_rate.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so, and the product
// never loads it.  `make redetectprobe` links this file with the SAME hog.o the shipped library links.  Every buffer a launch may write --
// votes, bins, blocks, hits, the counter, the class sums, the stream's state, the verdict -- lies between two guard zones, is filled with
// the canary (or a known value) first, and is read back whole, as are the guards.  Every case is validated on the host BEFORE a launch.
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

enum { RP_OK = 0, RP_E_ARG = 1 };
constexpr uint8_t GUARD_FILL = 0xC7;
constexpr int GUARD = 256;

// the buffer read back; *guard_bad grows by the guard bytes that are no longer the canary, *changed by the data bytes that differ from `was`
hipError_t read_back(Dev& D, const Guarded& g, const uint8_t* was, std::vector<uint8_t>* out, long long* guard_bad, long long* changed)
{
    std::vector<uint8_t> z(g.bytes);
    const hipError_t e = guard_damage(D, g, z.data(), guard_bad);
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < g.bytes; i++) *changed += z[i] != (was ? was[i] : GUARD_FILL);
    if (out) out->swap(z);
    return hipSuccess;
}

// the workspace of one (H, W) detection on the device, every buffer guarded
struct Work {
    HogLevel* lv = nullptr;
    HogTables* tab = nullptr;
    float* det = nullptr;
    Guarded votes, bins, blocks, hits, cnt;
    int* gate = nullptr;
    HogDev dev() const { return HogDev{lv, tab, det, (float2*)votes.data(), bins.data(), (float*)blocks.data(), (HogHit*)hits.data(), (unsigned*)cnt.data(), nullptr}; }
};
int make_work(Dev& D, const HogPlan& p, const std::vector<float>& d, int max_hits, Work* w)
{
    HogTables tab;
    hog_tables(&tab);
    PROBE_HIP(D.alloc((void**)&w->lv, sizeof(HogLevel) * HOG_MAX_LEVELS));
    PROBE_HIP(D.alloc((void**)&w->tab, sizeof tab));
    PROBE_HIP(D.alloc((void**)&w->det, sizeof(float) * d.size()));
    PROBE_HIP(D.alloc((void**)&w->gate, 64));
    PROBE_HIP(hipMemcpyAsync(w->lv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(w->tab, &tab, sizeof tab, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(w->det, d.data(), sizeof(float) * d.size(), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));  // (tab and p.lv are the caller's: copied before they go)
    PROBE_HIP(guarded(D, &w->votes, sizeof(float2) * (size_t)p.npix, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &w->bins, (size_t)p.npix, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &w->blocks, sizeof(float) * HOG_BLOCK_LEN * (size_t)p.nblk, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &w->hits, sizeof(HogHit) * (size_t)max_hits, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &w->cnt, 4, GUARD, GUARD_FILL));
    return 0;
}
std::vector<float> seeded_detector()
{
    std::vector<float> d(HOG_DESC + 1);
    for (int i = 0; i < HOG_DESC; i++) d[i] = (float)((i * 2654435761u >> 9) % 2001) / 1000.f - 1.f;
    return d;
}

}  // namespace

extern "C" {

// [0] the canary byte, [1] the guard's size, [2] sizeof(TrackState), [3] the pick kernel's lanes, [4] the tracked hit budget, [5] the product's cap
void rp_layout(int32_t* out)
{
    out[0] = GUARD_FILL, out[1] = GUARD, out[2] = (int32_t)sizeof(TrackState), out[3] = HOG_PICK_THREADS, out[4] = HOG_TRACK_MAX_HITS, out[5] = HOG_GATED_CAP;
}

// The three gated launches over the frame and the spec of hog_probe.hip's hp_detect, with the gate word `gate` and grids capped at `cap`
// workgroups (0: full grids).  The counter starts at `count0`.  Outputs (each may be null): votes [2 npix], bins [npix], blocks [36 nblk],
// hits3 [3 max_hits] and hit_s [max_hits] in the order (level, y, x).  info[4]: [0] the counter afterwards, [1] guard bytes damaged,
// [2] bytes of votes, bins, blocks and hits that are no longer the canary, [3] hits stored.  The source is compared with what was sent:
// a changed byte counts as guard damage.
int rp_gated(const uint8_t* src, int64_t src_size, int64_t data_off, int64_t uv_off, int format, int H, int W, int64_t sy, int64_t sx, int64_t sc, int64_t uv_stride,
             int orient, double hit_threshold, int stride_x, int stride_y, double scale0, double final_threshold, int nlevels, int max_hits, const float* det, int ndet,
             int gate, int cap, int count0, float* votes, uint8_t* bins, float* blocks, int32_t* hits3, float* hit_s, int64_t* info)
{
    if (!src || !info || cap < 0 || count0 < 0 || !orient_ok(orient)) return RP_E_ARG;
    if (!frame_fits(src_size, data_off, uv_off, format, H, W, sy, sx, sc, uv_stride, HOG_MAX_SIDE)) return RP_E_ARG;
    std::vector<float> d;
    HogSpec sp;
    if (!hog_detector(det, ndet, &d) || hog_spec(hit_threshold, stride_x, stride_y, scale0, final_threshold, nlevels, max_hits, &sp)) return RP_E_ARG;
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(orient, H, W, sp, &p) || !p.n) return RP_E_ARG;
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t* ds = nullptr;
    PROBE_HIP(D.alloc((void**)&ds, (size_t)src_size));
    PROBE_HIP(hipMemcpyAsync(ds, src, (size_t)src_size, hipMemcpyHostToDevice, D.st));
    Work w;
    int rc = make_work(D, p, d, sp.max_hits, &w);
    if (rc) return rc;
    const unsigned c0 = (unsigned)count0;
    PROBE_HIP(hipMemcpyAsync(w.cnt.data(), &c0, 4, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(w.gate, &gate, 4, hipMemcpyHostToDevice, D.st));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(format == 2, format == 1, ds + data_off, ds + uv_off, sy, sx, sc, uv_stride);
    a.H = H, a.W = W, a.o = orient;
    PROBE_HIP(launch_hog_gated(a, p, w.dev(), sp.hit_threshold, sp.max_hits, 7, w.gate, cap, D.st));
    long long bad = 0, changed = 0, cchanged = 0;
    std::vector<uint8_t> v, b, k, hb, c, back((size_t)src_size);
    PROBE_HIP(read_back(D, w.votes, nullptr, &v, &bad, &changed));
    PROBE_HIP(read_back(D, w.bins, nullptr, &b, &bad, &changed));
    PROBE_HIP(read_back(D, w.blocks, nullptr, &k, &bad, &changed));
    PROBE_HIP(read_back(D, w.hits, nullptr, &hb, &bad, &changed));
    PROBE_HIP(read_back(D, w.cnt, nullptr, &c, &bad, &cchanged));
    PROBE_HIP(hipMemcpy(back.data(), ds, (size_t)src_size, hipMemcpyDeviceToHost));
    bad += memcmp(back.data(), src, (size_t)src_size) != 0;
    unsigned count;
    memcpy(&count, c.data(), 4);
    info[0] = count, info[1] = bad, info[2] = changed, info[3] = 0;
    if (votes) memcpy(votes, v.data(), v.size());
    if (bins) memcpy(bins, b.data(), b.size());
    if (blocks) memcpy(blocks, k.data(), k.size());
    if (gate && count >= c0 && count - c0 <= (unsigned)sp.max_hits && c0 == 0) {
        std::vector<HogHit> hits(count);
        if (count) memcpy(hits.data(), hb.data(), sizeof(HogHit) * count);
        std::sort(hits.begin(), hits.end(), [](const HogHit& x, const HogHit& y) { return x.level != y.level ? x.level < y.level : (x.y != y.y ? x.y < y.y : x.x < y.x); });
        for (unsigned i = 0; i < count; i++) {
            if (hits3) hits3[3 * i] = hits[i].level, hits3[3 * i + 1] = hits[i].y, hits3[3 * i + 2] = hits[i].x;
            if (hit_s) hit_s[i] = hits[i].s;
        }
        info[3] = count;
    }
    return RP_OK;
}

// The pick kernel on a hit list.  The frame is stored (H, W) under `orient` (its level table gives the hits their scales); hits3 [3 n]:
// the hits in the order given, n = min(count, max_hits), in a device buffer of exactly n hits; `count`: the counter.  The stream's state
// starts as vnect_track_begin leaves it for a (tsH, tsW) frame cropped with rect0 -- tsH, tsW need not be the picture's size (a frame
// squarify refuses as a whole: the refusal path).  state_out [sizeof(TrackState)]: the state afterwards; state_want: the state the host
// expects when the next box is want_next4 (crop.h: crop_squarify) for tracked frame xseq; out6: status, rect, hits as the kernel left them
// in a verdict filled with the canary.  info[4]: [0] guard bytes damaged (the hits and the counter must be unchanged: they count here
// too), [1] class-sum words not zero afterwards, [2] state bytes changed, [3] verdict bytes changed.
int rp_pick(int orient, int H, int W, double scale0, int nlevels, const int32_t* hits3, int n, int64_t count, int max_hits, int threshold, int gate, int tsH, int tsW,
            const int32_t* rect0, unsigned xseq, const int32_t* want_next4, uint8_t* state_out, uint8_t* state_want, int32_t* out6, int64_t* info)
{
    HogSpec sp;
    if (!orient_ok(orient) || H < 1 || W < 1 || hog_spec(0.0, 0, 0, scale0, 0.0, nlevels, max_hits, &sp) || !info || !rect0 || !state_out || !out6) return RP_E_ARG;
    if (max_hits < 1 || max_hits > HOG_TRACK_MAX_HITS || count < 0 || n < 0 || n != (count < max_hits ? count : max_hits) || tsH < 1 || tsW < 1) return RP_E_ARG;
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(orient, H, W, sp, &p)) return RP_E_ARG;
    std::vector<HogHit> hits;
    for (int i = 0; i < n; i++) {
        if (hits3[3 * i] < 0 || hits3[3 * i] >= p.n || hits3[3 * i + 1] < 0 || hits3[3 * i + 1] >= HOG_MAX_SIDE || hits3[3 * i + 2] < 0 || hits3[3 * i + 2] >= HOG_MAX_SIDE) return RP_E_ARG;
        hits.push_back(HogHit{hits3[3 * i], hits3[3 * i + 1], hits3[3 * i + 2], 0.f});
    }
    std::vector<TrackState> tv(2);
    TrackState& t = tv[0];
    memset(&t, 0, sizeof t);
    t.x = rect0[0], t.y = rect0[1], t.w = rect0[2], t.h = rect0[3], t.uw = rect0[2], t.uh = rect0[3], t.H = tsH, t.W = tsW;
    t.status = crop_squarify(t.h, t.w, &t.fp);
    t.fail = t.status != SQ_OK ? 1u : 0u;
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    HogLevel* lv = nullptr;
    int* dgate = nullptr;
    PROBE_HIP(D.alloc((void**)&lv, sizeof(HogLevel) * HOG_MAX_LEVELS));
    PROBE_HIP(D.alloc((void**)&dgate, 64));
    if (p.n) PROBE_HIP(hipMemcpyAsync(lv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dgate, &gate, 4, hipMemcpyHostToDevice, D.st));
    Guarded gh, gc, gs, gt, go;
    PROBE_HIP(guarded(D, &gh, sizeof(HogHit) * (size_t)n, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gc, 4, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gs, sizeof(int) * 5 * HOG_TRACK_MAX_HITS, GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &gt, sizeof(TrackState), GUARD, GUARD_FILL));
    PROBE_HIP(guarded(D, &go, sizeof(RedetectOut), GUARD, GUARD_FILL));
    const unsigned cnt = (unsigned)count;
    if (n) PROBE_HIP(hipMemcpyAsync(gh.data(), hits.data(), sizeof(HogHit) * n, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(gc.data(), &cnt, 4, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemsetAsync(gs.data(), 0, gs.bytes, D.st));
    PROBE_HIP(hipMemcpyAsync(gt.data(), &t, sizeof t, hipMemcpyHostToDevice, D.st));
    const HogDev dv{lv, nullptr, nullptr, nullptr, nullptr, nullptr, (HogHit*)gh.data(), (unsigned*)gc.data(), nullptr};
    PROBE_HIP(launch_hog_pick(dv, p.n, max_hits, threshold, dgate, (int*)gs.data(), (TrackState*)gt.data(), xseq, (RedetectOut*)go.data(), D.st));
    long long bad = 0, hchg = 0, cchg = 0, schg = 0, tchg = 0, ochg = 0;
    std::vector<uint8_t> zeros(gs.bytes, 0), st, ov;
    PROBE_HIP(read_back(D, gh, (const uint8_t*)hits.data(), nullptr, &bad, &hchg));
    PROBE_HIP(read_back(D, gc, (const uint8_t*)&cnt, nullptr, &bad, &cchg));
    PROBE_HIP(read_back(D, gs, zeros.data(), nullptr, &bad, &schg));
    PROBE_HIP(read_back(D, gt, (const uint8_t*)&t, &st, &bad, &tchg));
    PROBE_HIP(read_back(D, go, nullptr, &ov, &bad, &ochg));
    memcpy(state_out, st.data(), sizeof t);
    memcpy(out6, ov.data(), sizeof(RedetectOut));
    if (state_want && want_next4) {
        TrackState& q = tv[1];
        q = t;
        q.x = want_next4[0], q.y = want_next4[1], q.w = q.uw = want_next4[2], q.h = q.uh = want_next4[3];
        q.status = crop_squarify(q.h, q.w, &q.fp);
        q.fail = q.status != SQ_OK ? xseq + 1 : 0u;
        memcpy(state_want, &q, sizeof q);
    }
    info[0] = bad + hchg + cchg, info[1] = schg, info[2] = tchg, info[3] = ochg;
    return RP_OK;
}

// The launches' own durations (tools/redetect_rate.py): n rounds over an (H, W) packed BGR frame the shim makes itself, defaults, a seeded
// detector and a threshold nothing clears; device events round each stage: ms_out[3 n] (votes, blocks, windows).  gate -1: the ungated
// launches; 0 / 1: the gated ones on grids capped at `cap` (0: full grids).
int rp_time(int H, int W, int gate, int cap, int n, float* ms_out)
{
    if (!ms_out || n < 1 || H < 2 || W < 2 || H > HOG_MAX_SIDE || W > HOG_MAX_SIDE || gate < -1 || gate > 1 || cap < 0) return RP_E_ARG;
    HogSpec sp;
    hog_spec(0.0, 0, 0, 0.0, 0.0, 0, HOG_TRACK_MAX_HITS, &sp);
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(0, H, W, sp, &p) || !p.n) return RP_E_ARG;
    const size_t bytes = (size_t)H * W * 3;
    std::vector<uint8_t> host(bytes);
    for (size_t i = 0; i < bytes; i++) host[i] = (uint8_t)((i * 2654435761u >> 11) % 251);
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    uint8_t* ds = nullptr;
    PROBE_HIP(D.alloc((void**)&ds, bytes));
    PROBE_HIP(hipMemcpy(ds, host.data(), bytes, hipMemcpyHostToDevice));
    Work w;
    int rc = make_work(D, p, seeded_detector(), sp.max_hits, &w);
    if (rc) return rc;
    const int g = gate > 0;
    PROBE_HIP(hipMemcpy(w.gate, &g, 4, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemset(w.cnt.data(), 0, 4));
    HogSrc a;
    memset(&a, 0, sizeof a);
    a.src = preview_source(false, false, ds, ds, 3LL * W, 3, 1, W);
    a.H = H, a.W = W, a.o = 0;
    return timed_launches(D.st, n, ms_out, [&](int s) {
        return gate < 0 ? launch_hog(a, p, w.dev(), 3.0e38, sp.max_hits, 1 << s, D.st) : launch_hog_gated(a, p, w.dev(), 3.0e38, sp.max_hits, 1 << s, w.gate, cap, D.st);
    }, 3);
}

// the pick kernel's duration on `nhits` hits of a 1920 x 1080 frame (clusters of up to nine neighbouring windows), n rounds: ms_out[n]
int rp_time_pick(int nhits, int n, float* ms_out)
{
    if (!ms_out || n < 1 || nhits < 0 || nhits > HOG_TRACK_MAX_HITS) return RP_E_ARG;
    HogSpec sp;
    hog_spec(0.0, 0, 0, 0.0, 0.0, 0, HOG_TRACK_MAX_HITS, &sp);
    std::vector<HogPlan> pv(1);
    HogPlan& p = pv[0];
    if (hog_plan(0, 1080, 1920, sp, &p) || !p.n) return RP_E_ARG;
    std::vector<HogHit> hits;
    unsigned rng = 777u;
    auto next = [&]() { return rng = rng * 1664525u + 1013904223u, rng >> 8; };
    std::vector<unsigned> keys;
    while ((int)hits.size() < nhits) {
        const int lv = (int)(next() % 20u);
        const HogLevel& L = p.lv[lv];
        const int cx = (int)(next() % (unsigned)(L.nwx - 2)), cy = (int)(next() % (unsigned)(L.nwy - 2));
        for (int q = 0; q < 9 && (int)hits.size() < nhits; q++) {
            const unsigned key = hog_key(lv, (cy + q / 3) * 8, (cx + q % 3) * 8);
            if (std::find(keys.begin(), keys.end(), key) != keys.end()) continue;
            keys.push_back(key);
            hits.push_back(HogHit{lv, (cy + q / 3) * 8, (cx + q % 3) * 8, 0.f});
        }
    }
    std::vector<TrackState> tv(1);
    memset(&tv[0], 0, sizeof(TrackState));
    tv[0].w = tv[0].uw = tv[0].W = 1920, tv[0].h = tv[0].uh = tv[0].H = 1080;
    tv[0].status = crop_squarify(1080, 1920, &tv[0].fp);
    Dev D;
    PROBE_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    HogLevel* lv = nullptr;
    HogHit* dh = nullptr;
    unsigned* dc = nullptr;
    int *gate = nullptr, *cls = nullptr;
    TrackState* ts = nullptr;
    RedetectOut* out = nullptr;
    PROBE_HIP(D.alloc((void**)&lv, sizeof(HogLevel) * HOG_MAX_LEVELS));
    PROBE_HIP(D.alloc((void**)&dh, sizeof(HogHit) * (size_t)nhits));
    PROBE_HIP(D.alloc((void**)&dc, 64));
    PROBE_HIP(D.alloc((void**)&gate, 64));
    PROBE_HIP(D.alloc((void**)&cls, sizeof(int) * 5 * HOG_TRACK_MAX_HITS));
    PROBE_HIP(D.alloc((void**)&ts, sizeof(TrackState)));
    PROBE_HIP(D.alloc((void**)&out, sizeof(RedetectOut)));
    const unsigned cnt = (unsigned)nhits;
    const int one = 1;
    PROBE_HIP(hipMemcpy(lv, p.lv, sizeof(HogLevel) * p.n, hipMemcpyHostToDevice));
    if (nhits) PROBE_HIP(hipMemcpy(dh, hits.data(), sizeof(HogHit) * nhits, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(dc, &cnt, 4, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(gate, &one, 4, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemset(cls, 0, sizeof(int) * 5 * HOG_TRACK_MAX_HITS));
    PROBE_HIP(hipMemcpy(ts, &tv[0], sizeof(TrackState), hipMemcpyHostToDevice));
    const HogDev dv{lv, nullptr, nullptr, nullptr, nullptr, nullptr, dh, dc, nullptr};
    return timed_launches(D.st, n, ms_out, [&](int) { return launch_hog_pick(dv, p.n, HOG_TRACK_MAX_HITS, 2, gate, cls, ts, 1u, out, D.st); });
}

}  // extern "C"
