// trackbox.h -- the box stage of a tracked frame (run_estimator_ps.py:96-107 and the loop's fallback, then the next crop's squarify
// geometry), as a device function of ONE workgroup of at least BOX threads: the body of track_box_kernel (track.hip, its own launch) and
// of post_kernel's tracked form (post.hip, the tail of the joints stage).  Arithmetic in crop.h.
#pragma once
#include "crop.h"
#include "kernels.h"

namespace vnect {

struct TrackNow {  // what a frame's box stage reads of the stream's state before it overwrites it
    int x, y, w, h, uw, uh, H, W, status;
};
__device__ __forceinline__ TrackNow track_now(const TrackState* ts)
{
    return TrackNow{ts->x, ts->y, ts->w, ts->h, ts->uw, ts->uh, ts->H, ts->W, ts->status};
}
// the frame's crop was refused (its joints stage skipped): report it, and keep the stream stopped -- the next frame is skipped too
// (gate: the stream's re-detection word or nullptr -- a refused frame never asks for a detection)
__device__ __forceinline__ void track_refused(TrackState* ts, const TrackNow& c, TrackOut* tout, unsigned xseq, int* gate = nullptr)
{
    if (threadIdx.x == 0) {
        tout->rect[0] = c.x, tout->rect[1] = c.y, tout->rect[2] = c.uw, tout->rect[3] = c.uh, tout->status = c.status;
        ts->fail = xseq + 1;
        if (gate) *gate = 0;
    }
}
// The second half of a box stage: `rect` (x, y, w, h; the same in every thread, e.g. read from LDS behind a barrier) becomes the stream's
// next crop -- its squarify geometry (crop_head / crop_entry / crop_fill_head) or its refusal.  Every thread of a workgroup of at least
// BOX threads calls this.  track_box_stage ends with it, and so does the pick kernel of a re-detection (hog.hip).
__device__ __forceinline__ void track_box_commit(TrackState* ts, const int* rect, unsigned xseq)
{
    const int t = threadIdx.x;
    const int cw = rect[2], ch = rect[3];
    SqHead g = {};
    const int status = crop_head(ch, cw, &g);
    if (status != SQ_OK) g = SqHead{};  // zero tables: the pyramid reads nothing of a refused crop
    const int inner = t < BOX ? crop_entry(g, cw, ch, t, &ts->fp.sq) : 0;
    const int xmax = __syncthreads_count(inner);
    if (t == 0) {
        crop_fill_head(g, status, ch, cw, xmax, &ts->fp);
        ts->x = rect[0], ts->y = rect[1], ts->w = cw, ts->h = ch, ts->uw = cw, ts->uh = ch;
        ts->status = status;
        ts->fail = status != SQ_OK ? xseq + 1 : 0u;
    }
}
// the stream's loss rule as a frame's box stage reads it, with the state, before anything else (pol == nullptr: off)
__device__ __forceinline__ TrackPolicy track_policy_now(const TrackPolicy* pol)
{
    return pol ? *pol : TrackPolicy{0.0, 1, TRACK_LOST_OFF};
}
// j2: the frame's 21 x 2 joints in FRAME coordinates, in LDS (every thread's write of them behind a barrier).  Every thread calls this.
// The loss rule (CONFIDENCE.md): conf -- the frame's NJ confidences, in LDS like j2, or nullptr (no rule) --, pol the stream's policy;
// cf (or nullptr) gets the verdict.  confident = #{j : conf[j] >= min_confidence} (a NaN or -inf confidence never counts),
// lost = action != OFF && confident < min_joints.  HOLD: the state stays as it is, every byte -- the next frame is cropped with this
// frame's crop (x, y, w, h, uw, uh and the geometry; fail is 0, since this frame ran).  RESET: the box rule's result is replaced by an
// empty rect, which box_fallback turns into the whole frame; everything behind it (crop_head / crop_entry, a refusal) is the usual path.
// gate (or nullptr): the re-detection word of a stream on which vnect_track_redetect is set (hog.h: THE RULE) -- 1 when this frame is
// lost, else 0; the gated detection launches and the pick kernel behind this stage read it.
__device__ __forceinline__ void track_box_stage(TrackState* ts, const TrackNow& c, const double* j2, TrackOut* tout, unsigned xseq,
                                                const double* conf = nullptr, const TrackPolicy pol = TrackPolicy{0.0, 1, TRACK_LOST_OFF},
                                                ConfOut* cf = nullptr, int* gate = nullptr)
{
    __shared__ int rect[4];
    __shared__ int lost_action;
    const int t = threadIdx.x;
    // (threads 0 .. NJ - 1 are in thread 0's wave: its ballot holds all 21 verdicts)
    const unsigned long long sure = conf ? __ballot(t < NJ && conf[t] >= pol.min_confidence) : 0ull;
    if (t == 0) {
        const int confident = __popcll(sure);
        const int lost = conf && pol.action != TRACK_LOST_OFF && confident < pol.min_joints;
        if (cf) cf->lost = lost, cf->confident = confident;
        lost_action = lost ? pol.action : TRACK_LOST_OFF;
        if (gate) *gate = lost;
        int r[4];
        box_update(j2, c.W, c.H, r);
        if (lost && pol.action == TRACK_LOST_RESET) r[0] = 0, r[1] = 0, r[2] = 0, r[3] = 0;
        box_fallback(c.W, c.H, r);
        rect[0] = r[0], rect[1] = r[1], rect[2] = r[2], rect[3] = r[3];
        tout->rect[0] = c.x, tout->rect[1] = c.y, tout->rect[2] = c.uw, tout->rect[3] = c.uh, tout->status = SQ_OK;
    }
    __syncthreads();
    if (lost_action == TRACK_LOST_HOLD) return;  // (uniform)
    track_box_commit(ts, rect, xseq);
}

}  // namespace vnect
