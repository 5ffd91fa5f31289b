"""GPU, product library: the loss rule end to end on a planted video in which the person leaves and returns (CONFIDENCE.md).

tests/planted.py's weights without heat-map noise turn a frame's brightest blob of colour j % 3 into joint j's peak; the video shows three
blobs, then empty frames (nobody there: black but for one dim white glow, so that every heat-map keeps ONE maximum and no frame's joints
hang on a tie between equal cells), then the blobs again.  The empty frames come an hour apart, as from a camera that idles while nobody
is there: the filters then follow every jump at once, all 21 joints sit on the glow, and the rule-free loop falls back to the whole
frame -- it finds the person again by itself, which the threshold's definition needs.  runner.track with confidence=True and no rule
gives the confidences; the threshold is the midpoint between the highest confidence on the empty frames and the lowest on the blob frames
(the test FAILS if they do not separate).  Then runner.track_on_device(..., lost=...) must equal runner.track(..., lost=...) bit for bit -- joints,
rect_used, confidences, lost flag -- in fp32 and bf16, from pinned, resident and device frames, for hold and reset."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 1.7e9
H, W = 480, 640
N, GAP = 20, (8, 14)
GLOW = 45.0
MIN_JOINTS = 11
_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        from tests import planted
        _CACHE["w"] = planted.weights(noise=0.0)
    return _CACHE["w"]


def _video():
    """N frames: three blobs drifting to the right; frames GAP[0] .. GAP[1] - 1 are empty but for a dim white glow where the person stood."""
    if "video" not in _CACHE:
        from tests import planted
        out = []
        for k in range(N):
            cy, cx, r = H * 0.5, W * (0.40 + 0.1 * k / (N - 1)), 50.0
            blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
            blank = GAP[0] <= k < GAP[1]
            glow = [(0.5 * H, 0.44 * W, c, GLOW) for c in range(3)]
            out.append(planted.scene(H, W, glow if blank else blobs, sigma=9.0, seed=k, texture=0.0 if blank else 0.15))
        _CACHE["video"] = out
    return _CACHE["video"]


def _times():
    """33 ms a frame while the person is there; an hour between the empty frames, and before the frame that shows the person again"""
    out, t = [], T0
    for k in range(N):
        t += 3600.0 if GAP[0] <= k <= GAP[1] else 0.033
        out.append((t, t + 0.0005))
    return out


def _est(precision, **kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=_weights(), verbose=False, precision=precision, **kw)


def _threshold(precision):
    """The rule-free run and the threshold taken from it: (threshold, that run's tuples)."""
    key = ("thr", precision)
    if key not in _CACHE:
        from vnect_amd import runner
        est = _est(precision)
        try:
            free = list(runner.track(est, _video(), timestamps=_times(), confidence=True))
        finally:
            est.close()
        assert all(len(f) == 5 and f[4] == 0 for f in free)
        blank = [f[3] for k, f in enumerate(free) if GAP[0] <= k < GAP[1]]
        blob = [f[3] for k, f in enumerate(free) if not GAP[0] <= k < GAP[1]]
        hi, lo = max(float(c.max()) for c in blank), min(float(c.min()) for c in blob)
        print(precision, "highest confidence on empty frames", hi, "lowest on blob frames", lo)
        assert hi < lo, ("the confidences of empty and blob frames do not separate", precision, hi, lo)
        _CACHE[key] = ((hi + lo) / 2, free)
    return _CACHE[key]


def _pool_frames(pool):
    from tests import devframe_ref as dr
    out = []
    for f in _video():
        buf = np.ascontiguousarray(f).reshape(-1)
        p = pool.alloc(len(buf))
        assert pool.probe.ip_h2d(p, buf.ctypes.data, len(buf)) == 0
        out.append(dr.FakeCuda(p, (H, W, 3), (3 * W, 3, 1)))
    return out


class _Pool:
    def __init__(self):
        import ctypes as C

        from tests import devframe_ref as dr
        self.C, self.probe, self.ptrs = C, dr.load_probe(), []

    def alloc(self, nbytes):
        p = self.C.c_void_p()
        assert self.probe.ip_alloc(int(nbytes), self.C.byref(p)) == 0 and p.value
        self.ptrs.append(p.value)
        return p.value

    def close(self):
        for p in self.ptrs:
            self.probe.ip_free(p)
        self.ptrs = []


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("action", ["hold", "reset"])
def test_device_loop_with_the_rule_equals_runner_track(action, precision):
    from vnect_amd import runner
    thr, free = _threshold(precision)
    rule = (thr, MIN_JOINTS, action)
    est = _est(precision, lanes=3)
    pool = _Pool()
    try:
        want = list(runner.track(est, _video(), timestamps=_times(), confidence=True, lost=rule))
        lost = [f[4] for f in want]
        print(precision, action, "lost", lost, "rects", [list(f[2]) for f in want][GAP[0] - 1:GAP[1] + 2])
        assert sum(lost) >= 2 and len(lost) - sum(lost) >= 2, lost
        assert any(a and not b for a, b in zip(lost, lost[1:])), ("no recovery", lost)
        assert lost == [int(GAP[0] <= k < GAP[1]) for k in range(N)], lost
        # the rule acts: behind a lost frame the crop is this frame's again (hold) or the whole frame (reset), not the rule-free loop's
        for k in range(GAP[0], GAP[1]):
            assert list(want[k + 1][2]) == (list(want[k][2]) if action == "hold" else [0, 0, W, H]), (k, want[k + 1][2])
        if action == "hold":   # (the rule-free loop falls back to the whole frame on the glow, as reset does: only hold parts from it)
            assert any(list(a[2]) != list(b[2]) for a, b in zip(want, free))
        # the confidences do not depend on the rule's bookkeeping: frame 0 .. GAP[0] are the rule-free run's
        for k in range(GAP[0] + 1):
            assert np.array_equal(want[k][3], free[k][3]) and np.array_equal(want[k][0], free[k][0])
        for source in ("pinned", "resident", "device"):
            est.reset()
            frames = _pool_frames(pool) if source == "device" else _video()
            got = list(runner.track_on_device(est, frames, timestamps=_times(), ahead=2, source=source, confidence=True, lost=rule))
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                tag = (precision, action, source, k)
                assert len(g) == 5 and list(g[2]) == list(w[2]) and g[4] == w[4], (tag, g[2], w[2], g[4], w[4])
                assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), tag
                assert g[3].dtype == np.float64 and g[3].tobytes() == w[3].tobytes(), tag
            # the loop leaves the stream's rule off again, and today's tuples come back by default
            est.reset()
            plain = list(runner.track_on_device(est, _video()[:3], timestamps=_times()[:3], source="pinned"))
            assert all(len(p) == 3 for p in plain)
            assert est.handle.result_confidence()[1] == 0
    finally:
        pool.close()
        est.close()
