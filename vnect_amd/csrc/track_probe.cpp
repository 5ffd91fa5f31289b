// track_probe.cpp -- C shim over the tracking kernels' launchers for tests/test_gpu_track_kernels.py.  TEST INFRASTRUCTURE: it is NOT part
// of libvnect_hip.so, and the product never loads it.  `make trackprobe` links this file with the SAME track.o and post.o the shipped
// library links (nothing of the kernels is recompiled), so the device compile of crop.h / trackbox.h / pyramid.h that the product runs
// is what the tests hold to the host's references, case by case: batches of cases in arrays, one launch per case on one stream, one
// copy back per batch.
// Every case is validated on the host BEFORE anything is launched (check_frame, check_frame_state, tp_box's own loop): a case that could make a kernel read or write outside
// its buffers gets an error code and no launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "crop.h"
#include "hostplan.h"
#include "kernels.h"
#include "probe_util.h"

using namespace vnect;

namespace {

enum { TP_OK = 0, TP_E_CROP = 1, TP_E_SIZE = 2, TP_E_STATE = 3, TP_E_JOINTS = 4, TP_E_ROOM = 5 };
constexpr uint8_t GARBAGE = 0xA5;   // what ts->fp holds before a box launch: an entry no thread writes keeps it
constexpr uint8_t DST_FILL = 0xCD;  // what a crop copy's destination holds before the launch
constexpr int DST_GUARD = 64;       // bytes in front of (and at least as many behind) a crop copy's destination

struct BoxCase {  // one case of tp_box on the device
    TrackState ts;
    JointsOut jo;
    TrackOut to;
};

// A state that a frame-reading kernel (crop copy, tracked pyramid) may be launched with, over an (H, W) frame `stride` bytes a row:
// the frame's size is the allocation's, the crop lies inside it, and the geometry is hostplan.h's for the crop's size -- or, for a
// refused crop, all zero (the pyramid reads nothing of it).
int check_frame_state(const TrackState& s, int H, int W)
{
    if (s.H != H || s.W != W) return TP_E_SIZE;
    if (s.x < 0 || s.y < 0 || s.w < 1 || s.h < 1 || (long long)s.x + s.w > W || (long long)s.y + s.h > H) return TP_E_CROP;
    std::vector<FrameParams> want(1);
    memset(&want[0], 0, sizeof(FrameParams));
    const char* why = plan::squarify(s.h, s.w, &want[0]);
    if (why) memset(&want[0], 0, sizeof(FrameParams));
    if ((s.status != SQ_OK) != (why != nullptr)) return TP_E_STATE;
    if (memcmp(&s.fp, &want[0], sizeof(FrameParams)) != 0) return TP_E_STATE;
    return TP_OK;
}
int check_frame(int H, int W, long long stride, long long cap)
{
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || stride < 3LL * W || stride > (1LL << 20)) return TP_E_SIZE;
    if ((long long)(H - 1) * stride + 3LL * W > cap) return TP_E_SIZE;
    return TP_OK;
}

}  // namespace

extern "C" {

// [0] sizeof(TrackState), [1] offset of its fp, [2] sizeof(FrameParams), [3] sizeof(TrackOut), [4] the garbage byte, [5] the
// destination fill byte, [6] the destination guard
void tp_layout(int32_t* out)
{
    out[0] = (int)sizeof(TrackState), out[1] = (int)offsetof(TrackState, fp), out[2] = (int)sizeof(FrameParams), out[3] = (int)sizeof(TrackOut);
    out[4] = GARBAGE, out[5] = DST_FILL, out[6] = DST_GUARD;
}

// The box stage (launch_track_box) over n cases: states (n x sizeof(TrackState) bytes), joints (n x 21 x 2 doubles in CROP coordinates),
// xseq (n).  ts->fp of every case is filled with the garbage byte before its launch.  Out: the states after the launch, tout
// (n x 6 ints: rect, status, pad) and the joints as the kernel left them.  err (n): TP_OK or why the case was not launched; returns 0,
// the number of refused cases (nothing at all is launched then), or < -1000 for a HIP error.
int tp_box(int n, const uint8_t* states, const double* joints, const uint32_t* xseq, uint8_t* states_out, int32_t* tout, double* joints_out,
           int32_t* err)
{
    if (n < 1) return 0;
    int bad = 0;
    for (int i = 0; i < n; i++) {
        TrackState s;
        memcpy(&s, states + (size_t)i * sizeof(TrackState), sizeof s);
        err[i] = TP_OK;
        if (s.status < SQ_OK || s.status > SQ_LONG) err[i] = TP_E_STATE;
        for (int k = 0; k < NJ * 2; k++) {
            const double v = joints[(size_t)i * NJ * 2 + k];
            if (!(fabs(v) < 1e9)) err[i] = TP_E_JOINTS;   // (NaN and infinities too: the C casts of box_axis need a finite value in range)
        }
        bad += err[i] != TP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    const int CH = 4096;
    std::vector<BoxCase> hb(n < CH ? n : CH);
    BoxCase* db = nullptr;
    PROBE_HIP(D.alloc((void**)&db, hb.size() * sizeof(BoxCase)));
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int m = n - c0 < CH ? n - c0 : CH;
        memset(hb.data(), 0, (size_t)m * sizeof(BoxCase));
        for (int i = 0; i < m; i++) {
            memcpy(&hb[i].ts, states + (size_t)(c0 + i) * sizeof(TrackState), sizeof(TrackState));
            memset(&hb[i].ts.fp, GARBAGE, sizeof(FrameParams));
            memcpy(hb[i].jo.j2d, joints + (size_t)(c0 + i) * NJ * 2, sizeof hb[i].jo.j2d);
            memset(&hb[i].to, GARBAGE, sizeof(TrackOut));
        }
        PROBE_HIP(hipMemcpyAsync(db, hb.data(), (size_t)m * sizeof(BoxCase), hipMemcpyHostToDevice, D.st));
        for (int i = 0; i < m; i++) PROBE_HIP(launch_track_box(&db[i].ts, &db[i].jo, &db[i].to, xseq[c0 + i], D.st));
        PROBE_HIP(hipMemcpyAsync(hb.data(), db, (size_t)m * sizeof(BoxCase), hipMemcpyDeviceToHost, D.st));
        PROBE_HIP(hipStreamSynchronize(D.st));
        for (int i = 0; i < m; i++) {
            memcpy(states_out + (size_t)(c0 + i) * sizeof(TrackState), &hb[i].ts, sizeof(TrackState));
            memcpy(tout + (size_t)(c0 + i) * 6, &hb[i].to, sizeof(TrackOut));
            memcpy(joints_out + (size_t)(c0 + i) * NJ * 2, hb[i].jo.j2d, sizeof hb[i].jo.j2d);
        }
    }
    return 0;
}

// The box stage with a loss rule (launch_track_box's policy form; CONFIDENCE.md; tests/test_gpu_conf_track_kernels.py) over n cases: tp_box's arrays plus conf (n x 21 doubles,
// any value: NaN and infinities are confidences like any other) and the rule of every case -- min_conf (n), min_joints (n, 1 .. 21),
// action (n, 0 .. 2).  The confidences and the rule lie in device memory, as the runtime's do.  ConfOut and ts->fp of every case hold the
// garbage byte before its launch.  Out: tp_box's three arrays and verdict (n x 2 ints: lost, confident).
int tp_box_policy(int n, const uint8_t* states, const double* joints, const uint32_t* xseq, const double* conf, const double* min_conf,
                  const int32_t* min_joints, const int32_t* action, uint8_t* states_out, int32_t* tout, double* joints_out, int32_t* verdict,
                  int32_t* err)
{
    struct PolicyCase {
        double conf[NJ];
        TrackPolicy pol;
        ConfOut co;
    };
    if (n < 1) return 0;
    int bad = 0;
    for (int i = 0; i < n; i++) {
        TrackState s;
        memcpy(&s, states + (size_t)i * sizeof(TrackState), sizeof s);
        err[i] = TP_OK;
        if (s.status < SQ_OK || s.status > SQ_LONG) err[i] = TP_E_STATE;
        if (min_joints[i] < 1 || min_joints[i] > NJ || action[i] < TRACK_LOST_OFF || action[i] > TRACK_LOST_RESET || min_conf[i] != min_conf[i]) err[i] = TP_E_STATE;
        for (int k = 0; k < NJ * 2; k++) {
            const double v = joints[(size_t)i * NJ * 2 + k];
            if (!(fabs(v) < 1e9)) err[i] = TP_E_JOINTS;
        }
        bad += err[i] != TP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    const int CH = 4096;
    const int m_max = n < CH ? n : CH;
    std::vector<BoxCase> hb(m_max);
    std::vector<PolicyCase> hp(m_max);
    BoxCase* db = nullptr;
    PolicyCase* dp = nullptr;
    PROBE_HIP(D.alloc((void**)&db, hb.size() * sizeof(BoxCase)));
    PROBE_HIP(D.alloc((void**)&dp, hp.size() * sizeof(PolicyCase)));
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int m = n - c0 < CH ? n - c0 : CH;
        memset(hb.data(), 0, (size_t)m * sizeof(BoxCase));
        for (int i = 0; i < m; i++) {
            memcpy(&hb[i].ts, states + (size_t)(c0 + i) * sizeof(TrackState), sizeof(TrackState));
            memset(&hb[i].ts.fp, GARBAGE, sizeof(FrameParams));
            memcpy(hb[i].jo.j2d, joints + (size_t)(c0 + i) * NJ * 2, sizeof hb[i].jo.j2d);
            memset(&hb[i].to, GARBAGE, sizeof(TrackOut));
            memcpy(hp[i].conf, conf + (size_t)(c0 + i) * NJ, sizeof hp[i].conf);
            hp[i].pol = TrackPolicy{min_conf[c0 + i], min_joints[c0 + i], action[c0 + i]};
            memset(&hp[i].co, GARBAGE, sizeof(ConfOut));
        }
        PROBE_HIP(hipMemcpyAsync(db, hb.data(), (size_t)m * sizeof(BoxCase), hipMemcpyHostToDevice, D.st));
        PROBE_HIP(hipMemcpyAsync(dp, hp.data(), (size_t)m * sizeof(PolicyCase), hipMemcpyHostToDevice, D.st));
        for (int i = 0; i < m; i++)
            PROBE_HIP(launch_track_box(&db[i].ts, &db[i].jo, &db[i].to, xseq[c0 + i], D.st, dp[i].conf, &dp[i].pol, &dp[i].co));
        PROBE_HIP(hipMemcpyAsync(hb.data(), db, (size_t)m * sizeof(BoxCase), hipMemcpyDeviceToHost, D.st));
        PROBE_HIP(hipMemcpyAsync(hp.data(), dp, (size_t)m * sizeof(PolicyCase), hipMemcpyDeviceToHost, D.st));
        PROBE_HIP(hipStreamSynchronize(D.st));
        for (int i = 0; i < m; i++) {
            memcpy(states_out + (size_t)(c0 + i) * sizeof(TrackState), &hb[i].ts, sizeof(TrackState));
            memcpy(tout + (size_t)(c0 + i) * 6, &hb[i].to, sizeof(TrackOut));
            memcpy(joints_out + (size_t)(c0 + i) * NJ * 2, hb[i].jo.j2d, sizeof hb[i].jo.j2d);
            verdict[(size_t)(c0 + i) * 2] = hp[i].co.lost, verdict[(size_t)(c0 + i) * 2 + 1] = hp[i].co.confident;
        }
    }
    return 0;
}

// The crop copy (launch_frame_copy_track) of n states' crops out of ONE pinned (H, W, 3) frame whose rows are `stride` bytes apart
// (frame: (H - 1) * stride + 3 W bytes).  The pinned buffer's capacity is that size rounded up to 4, and its end is the kernel's
// src_end.  Every case has its own destination of dst_cap bytes, pre-filled, with a pre-filled guard on both sides: dst_out gets
// n x (DST_GUARD + dst_cap + DST_GUARD) bytes.
int tp_copy(const uint8_t* frame, int H, int W, int64_t stride, int n, const uint8_t* states, int64_t dst_cap, uint8_t* dst_out, int32_t* err)
{
    if (n < 1) return 0;
    const long long used = H > 0 ? (long long)(H - 1) * stride + 3LL * W : 0;
    const long long cap = (used + 3) & ~3LL;
    const int fe = check_frame(H, W, stride, cap);
    int bad = 0;
    std::vector<TrackState> hs(n);
    for (int i = 0; i < n; i++) {
        memcpy(&hs[i], states + (size_t)i * sizeof(TrackState), sizeof(TrackState));
        err[i] = fe ? fe : check_frame_state(hs[i], H, W);
        if (!err[i] && (dst_cap < 0 || dst_cap % 64 != 0 || 3LL * hs[i].w * hs[i].h > dst_cap)) err[i] = TP_E_ROOM;
        bad += err[i] != TP_OK;
    }
    if (bad) return bad;
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *pin = nullptr, *pin_dev = nullptr;
    TrackState* ds = nullptr;
    Guarded dst;
    PROBE_HIP(D.pinned((void**)&pin, (size_t)cap));
    PROBE_HIP(hipHostGetDevicePointer((void**)&pin_dev, pin, 0));
    memset(pin, 0, (size_t)cap);
    memcpy(pin, frame, (size_t)used);
    PROBE_HIP(D.alloc((void**)&ds, (size_t)n * sizeof(TrackState)));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(guarded(D, &dst, (size_t)dst_cap, DST_GUARD, DST_FILL, nullptr, n));
    for (int i = 0; i < n; i++) PROBE_HIP(launch_frame_copy_track(&ds[i], pin_dev, dst.data(i), H, W, stride, pin_dev + cap, D.st));
    PROBE_HIP(read_regions(D, dst, dst_out));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// The tracked pyramid (launch_pyramid_track) of n states over ONE (H, W, 3) frame: packed[i] = 0 reads the crop at (x, y) of the whole
// frame in device memory, rows `stride` bytes apart; packed[i] = 1 reads the crop's own rows, 3 w bytes apart, from a buffer of exactly
// 3 w h bytes that the host packed.  ScaleTabs from hostplan.h (build_scale_tab, fill_lut).  el: EL_F32 / EL_BF16 / EL_F16.
// out: n x (S, 368, 368, 4) elements.
int tp_pyramid(const uint8_t* frame, int H, int W, int64_t stride, int n, const uint8_t* states, const int32_t* packed, const double* scales, int S,
               int el, void* out, int32_t* err)
{
    if (n < 1) return 0;
    if (S < 1 || S > 8 || el < EL_F32 || el > EL_F16) return -1;
    std::vector<ScaleTabs> tabs(1);
    memset(&tabs[0], 0, sizeof(ScaleTabs));
    tabs[0].S = S;
    plan::fill_lut(tabs[0].lut);
    for (int i = 0; i < S; i++)
        if (plan::build_scale_tab(scales[i], &tabs[0], i)) return -1;
    const long long used = H > 0 ? (long long)(H - 1) * stride + 3LL * W : 0;
    const int fe = check_frame(H, W, stride, used);
    int bad = 0;
    std::vector<TrackState> hs(n);
    std::vector<size_t> off(n + 1, 0);  // of every packed crop in the packed buffer (16-byte aligned, as hipMalloc'd buffers are)
    for (int i = 0; i < n; i++) {
        memcpy(&hs[i], states + (size_t)i * sizeof(TrackState), sizeof(TrackState));
        err[i] = fe ? fe : check_frame_state(hs[i], H, W);
        bad += err[i] != TP_OK;
        // (room for rows 3 uw bytes apart, not only 3 w: a kernel that took the stride from the REPORTED extent of an initial rect past the
        // frame's edge must read wrong pixels, not memory outside the buffer; what lies between the rows' ends is noise, not zeros)
        const size_t wide = (size_t)(hs[i].uw > hs[i].w ? hs[i].uw : hs[i].w);
        if (!err[i] && (hs[i].uw < hs[i].w || hs[i].uh < hs[i].h || hs[i].uw > 65535 || hs[i].uh > 65535)) err[i] = TP_E_STATE, bad++;
        off[i + 1] = off[i] + (err[i] || !packed[i] ? 0 : ((3 * wide * hs[i].h + 255) & ~(size_t)255));
    }
    if (bad) return bad;
    std::vector<uint8_t> pk(off[n] ? off[n] : 1, 0);
    for (size_t k = 0; k < pk.size(); k++) pk[k] = (uint8_t)(k * 2654435761u >> 24);
    for (int i = 0; i < n; i++)
        if (packed[i])
            for (int r = 0; r < hs[i].h; r++)
                memcpy(&pk[off[i] + (size_t)r * 3 * hs[i].w], frame + (size_t)(hs[i].y + r) * stride + (size_t)3 * hs[i].x, (size_t)3 * hs[i].w);
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *dframe = nullptr, *dpk = nullptr, *dout = nullptr;
    TrackState* ds = nullptr;
    ScaleTabs* dt = nullptr;
    const size_t per = (size_t)S * BOX * BOX * 4 * (el == EL_F32 ? 4 : 2);
    PROBE_HIP(D.alloc((void**)&dframe, (size_t)used));
    PROBE_HIP(D.alloc((void**)&dpk, pk.size()));
    PROBE_HIP(D.alloc((void**)&ds, (size_t)n * sizeof(TrackState)));
    PROBE_HIP(D.alloc((void**)&dt, sizeof(ScaleTabs)));
    PROBE_HIP(D.alloc((void**)&dout, (size_t)n * per));
    PROBE_HIP(hipMemcpyAsync(dframe, frame, (size_t)used, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dpk, pk.data(), pk.size(), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dt, &tabs[0], sizeof(ScaleTabs), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemsetAsync(dout, 0xFF, (size_t)n * per, D.st));
    for (int i = 0; i < n; i++) {
        FrameDyn dyn = {};
        dyn.frame = packed[i] ? dpk + off[i] : dframe;
        dyn.row_stride = stride;
        PROBE_HIP(launch_pyramid_track(&ds[i], dyn, packed[i] ? 1 : 0, dt, dout + (size_t)i * per, S, el, D.st));
    }
    PROBE_HIP(hipMemcpyAsync(out, dout, (size_t)n * per, hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

// The pair pyramid (launch_pyramid_track_pair; tests/test_gpu_people_kernels.py) of n PAIRS of states over ONE (H, W, 3) frame: states holds
// 2 n of them, pair i is states 2 i and 2 i + 1, side by side in device memory as the runtime's streams are.  packed[i] = 0: both persons
// read their crop at (x, y) of the whole frame; 1: each from a buffer of its own packed rows.  2 S <= 8.  out: n x (2 S, 368, 368, 4)
// elements, every byte pre-filled with `fill` (a pixel the kernel does not write, or writes at another image's offset, keeps or misplaces
// it).  err (2 n): per state.
int tp_pyramid_pair(const uint8_t* frame, int H, int W, int64_t stride, int n, const uint8_t* states, const int32_t* packed, const double* scales, int S,
                    int el, int fill, void* out, int32_t* err)
{
    if (n < 1) return 0;
    if (S < 1 || 2 * S > 8 || el < EL_F32 || el > EL_F16) return -1;
    std::vector<ScaleTabs> tabs(1);
    memset(&tabs[0], 0, sizeof(ScaleTabs));
    tabs[0].S = S;
    plan::fill_lut(tabs[0].lut);
    for (int i = 0; i < S; i++)
        if (plan::build_scale_tab(scales[i], &tabs[0], i)) return -1;
    const long long used = H > 0 ? (long long)(H - 1) * stride + 3LL * W : 0;
    const int fe = check_frame(H, W, stride, used);
    int bad = 0;
    std::vector<TrackState> hs(2 * n);
    std::vector<size_t> off(2 * n + 1, 0);
    for (int i = 0; i < 2 * n; i++) {
        memcpy(&hs[i], states + (size_t)i * sizeof(TrackState), sizeof(TrackState));
        err[i] = fe ? fe : check_frame_state(hs[i], H, W);
        if (!err[i] && (hs[i].uw != hs[i].w || hs[i].uh != hs[i].h)) err[i] = TP_E_STATE;
        bad += err[i] != TP_OK;
        off[i + 1] = off[i] + (err[i] || !packed[i / 2] ? 0 : ((3 * (size_t)hs[i].w * hs[i].h + 255) & ~(size_t)255));
    }
    if (bad) return bad;
    std::vector<uint8_t> pk(off[2 * n] ? off[2 * n] : 1, 0);
    for (size_t k = 0; k < pk.size(); k++) pk[k] = (uint8_t)(k * 2654435761u >> 24);
    for (int i = 0; i < 2 * n; i++)
        if (packed[i / 2])
            for (int r = 0; r < hs[i].h; r++)
                memcpy(&pk[off[i] + (size_t)r * 3 * hs[i].w], frame + (size_t)(hs[i].y + r) * stride + (size_t)3 * hs[i].x, (size_t)3 * hs[i].w);
    Dev D;
    PROBE_HIP(hipStreamCreate(&D.st));
    uint8_t *dframe = nullptr, *dpk = nullptr, *dout = nullptr;
    TrackState* ds = nullptr;
    ScaleTabs* dt = nullptr;
    const size_t per = (size_t)2 * S * BOX * BOX * 4 * (el == EL_F32 ? 4 : 2);
    PROBE_HIP(D.alloc((void**)&dframe, (size_t)used));
    PROBE_HIP(D.alloc((void**)&dpk, pk.size()));
    PROBE_HIP(D.alloc((void**)&ds, (size_t)2 * n * sizeof(TrackState)));
    PROBE_HIP(D.alloc((void**)&dt, sizeof(ScaleTabs)));
    PROBE_HIP(D.alloc((void**)&dout, (size_t)n * per));
    PROBE_HIP(hipMemcpyAsync(dframe, frame, (size_t)used, hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dpk, pk.data(), pk.size(), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(ds, hs.data(), (size_t)2 * n * sizeof(TrackState), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemcpyAsync(dt, &tabs[0], sizeof(ScaleTabs), hipMemcpyHostToDevice, D.st));
    PROBE_HIP(hipMemsetAsync(dout, fill & 0xFF, (size_t)n * per, D.st));
    for (int i = 0; i < n; i++) {
        FrameDyn dyn[2] = {};
        for (int k = 0; k < 2; k++) dyn[k].frame = packed[i] ? dpk + off[2 * i + k] : dframe, dyn[k].row_stride = stride;
        PROBE_HIP(launch_pyramid_track_pair(&ds[2 * i], dyn[0], dyn[1], packed[i] ? 1 : 0, dt, dout + (size_t)i * per, S, el, D.st));
    }
    PROBE_HIP(hipMemcpyAsync(out, dout, (size_t)n * per, hipMemcpyDeviceToHost, D.st));
    PROBE_HIP(hipStreamSynchronize(D.st));
    return 0;
}

}  // extern "C"
