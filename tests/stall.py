"""A stalled producer stream: the helper of tests/test_gpu_stream_order.py, its control, and the frames both are run on.

The runtime orders one stream behind another with event waits (wait_for_producer, wait_prev).  A missing wait shows only while the
producer is still busy: `stalled_frame` leaves a device buffer that holds picture `old` and, on the producer's stream, a bounded spin
(ip_delayed_copy of vnect_amd/csrc/ingest_probe.hip: at most 50 ms on the 100 MHz clock) followed by the copy that fills it with picture
`new`.  A consumer that waits reads `new`; one that does not reads `old` -- valid pixels, so nothing can fault.

THE CONTROL makes that a measurement instead of a hope: the same call with VNECT_STREAM_SYNCED while the producer still spins tells the
library a falsehood, it waits for nothing, and the result must be that of `old`.  `choose_stream` runs the control for the two kinds of
consumer stream (the upload stream: vnect_upload_frame_device + vnect_read_frame; a lane's stream: vnect_submit_tracked_device +
vnect_collect_tracked) on each of four candidate producer streams and names the first on which both see `old`: where producer and
consumer share a hardware queue they merely serialise, the control reads `new`, and a test on that stream would prove nothing.  Which
streams share a queue differs from handle to handle -- every handle's lanes are streams of its own -- so a test on another handle (the
people handle, a two-lane handle) runs the lane control on THAT handle first (`control_people`, `first_old`) over the same candidates.

Everything a GPU test relies on that can be said without a GPU -- `old` and `new` differ where it matters, the box of the moving video
moves -- is asserted by tests/test_stream_order_cpu.py on the frames below.  Nothing here is a fixture; nothing at import needs a GPU."""
import ctypes as C

import numpy as np

from tests import devframe_ref as dr
from tests import hog_ref
from tests import overlay_ref

STALL_MS, STALL_CAP_MS = 20.0, 50.0      # the first stall tried; the probe's cap, tried once if 20 ms shows nothing on any stream
CANDIDATES = 4                           # producer streams tried, no more
H, W = 120, 160                          # the pose frames
S3 = (1.0, 0.8, 0.6)
RECT0 = [3, 2, 152, 115]                 # the first crop of the tracked cases: it holds the blobs of `old` and of `new`
HOG_H, HOG_W = 176, 120                  # the detector's frames: the smallest here whose detection's box is not the whole frame
HOG_CELL = (40, 24)                      # (x, y) of the painted figure's 64 x 128 cell in `new`
ALWAYS = (1e9, 21)                       # the loss rule under which every frame is lost, whatever the weights
T0 = 1.7e9
CONTROL_SLOT = 3
_CACHE = {}


def times(n, base=0.0):
    return [(T0 + base + 0.033 * k + 0.002 * (k % 3), T0 + base + 0.033 * k + 0.0005) for k in range(n)]


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def blobs_at(cy, cx, r=13.0):
    """three blobs, one per colour, around (cy, cx): joint j of the planted weights sits on the blob of colour j % 3"""
    return [(cy - r, cx, 0, 255.0), (cy + 1.1 * r, cx - 0.9 * r, 1, 255.0), (cy + 0.4 * r, cx + 1.2 * r, 2, 255.0)]


def centres(blobs):
    """tests/planted.py's known answer of a scene: joints_2d [row, col], joint j on the blob of colour j % 3"""
    at = {k: (r, c) for r, c, k, _ in blobs}
    return np.array([at[j % 3] for j in range(21)], np.float64)


OLD_BLOBS, NEW_BLOBS = blobs_at(38.0, 44.0), blobs_at(80.0, 113.0)


def _scene(blobs, seed, size=(H, W)):
    from tests import planted
    return planted.scene(size[0], size[1], blobs, sigma=4.0, seed=seed, texture=0.15)


def pose_pair():
    """(old, new): two 120 x 160 planted scenes whose blobs -- whose joints -- lie 80 pixels apart, over different textures"""
    if "pose" not in _CACHE:
        _CACHE["pose"] = (_scene(OLD_BLOBS, 11), _scene(NEW_BLOBS, 12))
    return _CACHE["pose"]


def moving_blobs(k):
    """frame k of the moving video: the person walks 8 pixels a frame to the right -- inside the margin the box update leaves -- and breathes"""
    return blobs_at(58.0, 30.0 + 8.0 * k, 12.0 + (k % 2))


def moving_video(n):
    """n frames whose crop box moves from frame to frame (tests/test_stream_order_cpu.py: by at least 5 pixels): a crop taken with the
    box of the frame before last is another crop"""
    if ("moving", n) not in _CACHE:
        _CACHE["moving", n] = [_scene(moving_blobs(k), 20 + k) for k in range(n)]
    return _CACHE["moving", n]


def hog_pair():
    """(old, new) for the detector: the textured background alone -- nobody -- and the same with tests/hog_ref.py's painted figure"""
    if "hog" not in _CACHE:
        old = hog_ref.background(HOG_H, HOG_W)
        new = old.copy()
        x, y = HOG_CELL
        new[y:y + 128, x:x + 64] = hog_ref.figure()
        _CACHE["hog"] = (old, new)
    return _CACHE["hog"]


def people_video():
    """tests/test_gpu_people.py's 96 x 128 video of four drifting persons, and the first rects (person 1's holds person 0)"""
    from tests import test_gpu_people as tp
    return tp._video(tp.SMALL), tp._rects(tp.SMALL, 4)


def skeleton():
    """(joints_2d, rect) drawn by the draw and preview cases: a skeleton spread over the 120 x 160 frame"""
    case = [c for c in overlay_ref.cases(H, W) if c["name"] == "skeleton"][0]
    return np.asarray(case["joints"], np.float64), [int(v) for v in case["rect"]]


def packed_layout(h=H, w=W):
    """tests/overlay_ref.py's layout of a contiguous packed BGR frame"""
    return dict(name=None, format=0, H=h, W=w, data_off=0, uv_off=0, sy=3 * w, sx=3, sc=1, uv_stride=0, size=h * w * 3)


def drawn(frame, joints_2d, rect):
    """the flat bytes of the packed BGR `frame` with the reference's overlay (tests/overlay_ref.py: the rule in numpy)"""
    buf = np.ascontiguousarray(frame).reshape(-1).copy()
    n = overlay_ref.draw(buf, packed_layout(*frame.shape[:2]), dict(name=None, joints=np.asarray(joints_2d), parents=overlay_ref.PARENTS, rect=list(rect)))
    assert n > 0
    return buf


def stored(picture, o):
    """the array stored under orientation code o when the picture is `picture`"""
    g = picture[:, ::-1] if o & 4 else picture
    return np.ascontiguousarray(np.rot90(g, -(o & 3)))


FORMS = ["packed-bgr", "nv12", "nv12-two", "orient-3"]      # the source forms: each puts the wait in front of another copy kernel


class Source:
    """One picture pair in one source form: the bytes of `old` and `new` as that form stores them (flat arrays; a (y, uv) pair for NV12
    in two allocations, with odd pitches), how a device address becomes the array the library is given, and what the library must see."""

    def __init__(self, form, old, new):
        from vnect_amd import pixfmt
        assert form in FORMS and old.shape == new.shape
        self.form, (self.H, self.W), self.pictures = form, old.shape[:2], [old, new]
        self.pixel_format = "nv12" if form.startswith("nv12") else "bgr"
        self.orientation = 3 if form == "orient-3" else 0
        if form == "packed-bgr":
            self.host = [old, new]                                   # what the host entry point is given for the same picture
            self.bytes = [np.ascontiguousarray(f).reshape(-1) for f in self.host]
        elif form == "orient-3":
            self.host = [stored(f, 3) for f in (old, new)]
            self.bytes = [f.reshape(-1) for f in self.host]
        else:
            self.host = [pixfmt.bgr_to_nv12(f) for f in (old, new)]
            if form == "nv12":
                self.bytes = [f.reshape(-1) for f in self.host]
            else:
                self.ys, self.uvs = self.W + 3, self.W + 5
                self.bytes = [self._planes(f) for f in self.host]

    def _planes(self, img):
        Hh, Ww = self.H, self.W
        yb, ub = np.zeros((Hh, self.ys), np.uint8), np.zeros((Hh // 2, self.uvs), np.uint8)
        yb[:, :Ww], ub[:, :Ww] = img[:Hh], img[Hh:]
        return (yb.reshape(-1)[:(Hh - 1) * self.ys + Ww].copy(), ub.reshape(-1)[:(Hh // 2 - 1) * self.uvs + Ww].copy())

    def array(self, ptr):
        """the device array at `ptr` (stalled_frame's return) as the Python layer takes it"""
        if self.form == "nv12-two":
            return (dr.FakeCuda(ptr[0], (self.H, self.W), (self.ys, 1)), dr.FakeCuda(ptr[1], (self.H // 2, self.W), (self.uvs, 1)))
        if self.form == "nv12":
            return dr.FakeCuda(ptr, (self.H * 3 // 2, self.W), (self.W, 1))
        return dr.FakeCuda(ptr, self.host[0].shape)

    def frame(self, ptr):
        from vnect_amd import _native
        return _native.device_frame(self.array(ptr), self.pixel_format)

    def seen(self, which):
        """the BGR picture the library must see of old (0) or new (1): an NV12 frame's by the conversion rule (tests/nv12_ref.py)"""
        from tests import nv12_ref
        if self.pixel_format == "nv12":
            return nv12_ref.restate(self.host[which])
        return self.pictures[which]


# ---- device memory and the stall -----------------------------------------------------------------------------------------------------------
class Pool:
    """device allocations of one test (the probe's allocator), freed at its end"""

    def __init__(self, probe):
        self.probe, self.ptrs = probe, {}

    def put(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        p = C.c_void_p()
        assert self.probe.ip_alloc(len(buf), C.byref(p)) == 0 and p.value
        assert self.probe.ip_h2d(p.value, buf.ctypes.data, len(buf)) == 0
        self.ptrs[p.value] = len(buf)
        return p.value

    def get(self, p):
        out = np.zeros(self.ptrs[p], np.uint8)
        assert self.probe.ip_d2h(out.ctypes.data, p, len(out)) == 0
        return out

    def fill(self, p, value):
        """a blocking fill of the whole allocation"""
        assert self.probe.ip_fill(p, value, self.ptrs[p]) == 0

    def close(self):
        for p in self.ptrs:
            self.probe.ip_free(p)
        self.ptrs = {}


def stalled_frame(probe, pool, st, old, new, ms):
    """A device buffer that holds `old` (copied synchronously) and is filled with `new` by a copy on stream `st` (a stream handle, or
    None for HIP's default stream) behind a spin of `ms` milliseconds -> its address.  `old` / `new`: flat uint8 arrays of one size; a
    (y, uv) pair of them for NV12 in two allocations: two buffers, the second's copy on the same stream with no spin of its own.
    Everything is staged before the spin starts, so the stall is the caller's to use."""
    two = isinstance(new, tuple)
    olds, news = (old, new) if two else ((old,), (new,))
    assert len(olds) == len(news) and all(o.size == n.size and not np.array_equal(o, n) for o, n in zip(olds, news))
    frames = [pool.put(o) for o in olds]
    staged = [pool.put(n) for n in news]
    for k, (f, s, n) in enumerate(zip(frames, staged, news)):
        assert probe.ip_delayed_copy(st, f, s, n.size, float(ms) if k == 0 else 0.0) == 0
    return tuple(frames) if two else frames[0]


def same_result(got, want):
    """a collected (stream, joints_2d, joints_3d, rect_used) against a runner.track tuple: bit for bit"""
    return list(got[3]) == list(want[2]) and np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])


def track_ref(est, frames, rect, stamps, **kw):
    """runner.track on the host frames, from fresh filters: [(joints_2d, joints_3d, rect_used, confidence, lost)]"""
    from vnect_amd import runner
    est.reset()
    out = [(a, b, list(c), d, e) for a, b, c, d, e in runner.track(est, frames, rect=list(rect), timestamps=stamps, confidence=True, **kw)]
    est.reset()
    return out


# ---- the control ---------------------------------------------------------------------------------------------------------------------------
def _which(is_old, is_new):
    return "old" if is_old and not is_new else "new" if is_new and not is_old else "neither"


def control_upload(probe, pool, est, st, ms):
    """vnect_upload_frame_device told VNECT_STREAM_SYNCED while `st` still spins -> which picture the slot holds: "old", "new", "neither" """
    from vnect_amd import _native
    src = Source("packed-bgr", *pose_pair())
    p = stalled_frame(probe, pool, st, src.bytes[0], src.bytes[1], ms)
    est.handle.upload_frame_device(CONTROL_SLOT, src.frame(p), _native.STREAM_SYNCED)
    got = est.handle.read_frame(CONTROL_SLOT)
    assert probe.ip_stream_sync(st) == 0
    return _which(np.array_equal(got, src.seen(0)), np.array_equal(got, src.seen(1)))


def control_lane(probe, pool, est, st, ms, refs):
    """vnect_submit_tracked_device told VNECT_STREAM_SYNCED while `st` still spins -> whose result vnect_collect_tracked delivers; refs:
    (track_ref of old, track_ref of new), one frame each from RECT0 at times(1)"""
    from vnect_amd import _native
    src = Source("packed-bgr", *pose_pair())
    est.reset()
    est.handle.track_begin(0, H, W, RECT0)
    p = stalled_frame(probe, pool, st, src.bytes[0], src.bytes[1], ms)
    est.handle.submit_tracked_device(0, src.frame(p), *times(1)[0], producer=_native.STREAM_SYNCED)
    got = est.handle.collect_tracked()
    assert probe.ip_stream_sync(st) == 0
    est.reset()
    return _which(same_result(got, refs[0][0]), same_result(got, refs[1][0]))


def control_people(probe, pool, pest, st, ms, refs):
    """vnect_submit_people_device (two persons, one paired unit) told VNECT_STREAM_SYNCED while `st` still spins, on the people handle --
    whose lanes are other streams than the plain handle's; refs: ([person] track_ref of old, [person] track_ref of new), one frame each"""
    from vnect_amd import _native
    video, rects = people_video()
    src = Source("packed-bgr", video[4], video[0])
    pest.reset()
    pest.handle.people_begin(2, src.H, src.W, rects[:2])
    p = stalled_frame(probe, pool, st, src.bytes[0], src.bytes[1], ms)
    pest.handle.submit_people_device(2, src.frame(p), *times(1)[0], producer=_native.STREAM_SYNCED)
    got = [pest.handle.collect_tracked() for _ in range(2)]
    assert probe.ip_stream_sync(st) == 0
    pest.reset()
    return _which(all(same_result(got[q], refs[0][q][0]) for q in range(2)), all(same_result(got[q], refs[1][q][0]) for q in range(2)))


def first_old(probe, streams, control, prefer=None):
    """`control(pool, st)` once on each candidate stream -> (the first stream on which it reads "old" -- `prefer` if it does there -- or
    None, the outcomes in the candidates' order)"""
    outcomes = []
    for st in streams:
        pool = Pool(probe)
        try:
            outcomes.append(control(pool, st))
        finally:
            pool.close()
    good = [st for st, o in zip(streams, outcomes) if o == "old"]
    return (prefer if prefer in good else good[0] if good else None), outcomes


def choose_stream(probe, est, streams):
    """Both controls once on each candidate stream, at 20 ms; if no stream shows `old` in both, once more at the probe's cap.  Returns
    (index of the first stream on which both controls read `old`, or None; the stall used; the report for stream_order.json)."""
    old, new = pose_pair()
    refs = (track_ref(est, [old], RECT0, times(1)), track_ref(est, [new], RECT0, times(1)))
    assert not same_result((0,) + refs[0][0][:3], refs[1][0]), "the control's two pictures give one result"
    report = {"rounds": []}
    chosen, used = None, STALL_MS
    for ms in (STALL_MS, STALL_CAP_MS):
        used, outcomes = ms, []
        for i, st in enumerate(streams):
            pool = Pool(probe)
            try:
                outcomes.append({"stream": i, "upload": control_upload(probe, pool, est, st, ms), "lane": control_lane(probe, pool, est, st, ms, refs)})
            finally:
                pool.close()
        report["rounds"].append({"stall_ms": ms, "controls": outcomes})
        good = [o["stream"] for o in outcomes if o["upload"] == "old" and o["lane"] == "old"]
        if good:
            chosen = good[0]
            break
    report["stall_ms"], report["chosen"] = used, chosen
    return chosen, used, report
