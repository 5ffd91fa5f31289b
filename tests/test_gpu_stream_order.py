"""GPU: every cross-stream ordering edge of the runtime against a STALLED producer stream (tests/stall.py).

The kernels are held bit for bit elsewhere; this module holds what runs between them: the event waits that order the library's streams
behind the caller's producer stream (wait_for_producer: rt_ingest.cpp, rt_draw.cpp, rt_hog.cpp, rt_exec.cpp) and behind each other
(wait_prev, the people frame's drawing: rt_exec.cpp).  On an idle GPU a missing wait changes nothing: the stale read and the fresh read
give the same bytes.  So every test here makes ONE call whose frame is still being produced -- the device buffer holds picture `old`, and
the producer's stream fills it with picture `new` behind a spin of 20 to 50 ms -- without synchronising anything, and the result must be
the host reference's on `new`, bit for bit.  The hand-overs inside the runtime are held the same way: the stalled producer keeps frame k
in flight for a known time, and what depends on frame k is submitted with VNECT_STREAM_SYNCED at once.

That a consumer which does NOT wait reads `old` on this machine is not assumed: the `stall` fixture runs tests/stall.py's control (the
same calls told VNECT_STREAM_SYNCED while the producer spins) on four candidate producer streams, takes the first on which the upload
stream and a lane's stream both read `old`, FAILS if there is none (the streams serialised: every test below would be vacuous), and writes
what it saw to stream_order.json in the tests' log directory.  The people handle and the two-lane handle have lanes of their own, which
may share a hardware queue with another candidate: their tests run the lane control on their own handle first (`people_stall`).

MATRIX is the list the producer-edge test is parametrised from; tests/test_stream_order_cpu.py holds it against include/vnect_abi.h, so an
entry point that takes a producer stream and has no row here fails without a GPU.

The one edge this cannot reach is the untracked filter chain across lanes (wait_prev in enqueue_frame's untracked branch): untracked
asynchronous frames come only from resident slots, which have no producer to stall, and pick_lane never queues a frame behind an
uncollected one while another lane is free.  tests/test_gpu_end_to_end.py's lane tests remain its only gate."""
import ctypes as C

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import overlay_ref as R
from tests import stall as S

pytestmark = pytest.mark.gpu

# (entry point of include/vnect_abi.h, case): one stalled call each.  The source forms put the wait in front of another copy kernel.
MATRIX = [
    ("vnect_upload_frame_device", "upload-packed-bgr"),
    ("vnect_upload_frame_device", "upload-nv12"),
    ("vnect_upload_frame_device", "upload-nv12-two"),
    ("vnect_upload_frame_device", "upload-orient-3"),
    ("vnect_preprocess_device", "preprocess"),
    ("vnect_infer_device", "infer"),
    ("vnect_draw_device", "draw"),
    ("vnect_preview_device", "preview"),
    ("vnect_hog_detect_device", "hog"),
    ("vnect_submit_tracked_device", "tracked-packed-bgr"),
    ("vnect_submit_tracked_device", "tracked-nv12"),
    ("vnect_submit_tracked_device", "tracked-nv12-two"),
    ("vnect_submit_tracked_device", "tracked-orient-3"),
    ("vnect_submit_tracked_device", "tracked-null-stream"),
    ("vnect_submit_tracked_device_draw", "tracked-draw"),
    ("vnect_submit_tracked_device_preview", "tracked-preview"),
    ("vnect_submit_tracked_device", "redetect"),
    ("vnect_submit_tracked_device_draw", "redetect-draw"),
    ("vnect_submit_tracked_device_preview", "redetect-preview"),
    ("vnect_submit_people_device", "people-2"),
    ("vnect_submit_people_device", "people-3"),
]
CASES = {}          # case -> the function that runs it (every one is a row of MATRIX: tests/test_stream_order_cpu.py)


def case(*names):
    def reg(fn):
        for n in names:
            CASES[n] = fn
        return fn
    return reg


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
def _planted():
    from tests import planted
    if "w" not in S._CACHE:
        S._CACHE["w"] = planted.weights(noise=1.0)
    return S._CACHE["w"]


def _est(**kw):
    from tests import hog_ref
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=_planted(), verbose=False, precision="bf16", scales=list(S.S3), hog_detector=hog_ref.planted_detector(), **kw)


@pytest.fixture(scope="module")
def probe():
    return dr.load_probe()


@pytest.fixture(scope="module")
def est():
    e = _est(lanes=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pest():
    """the people handle: up to 3 persons, pairs through one conv stack, three lanes"""
    e = _est(lanes=3, people=3, pair_people=True)
    yield e
    e.close()


class Stall:
    def __init__(self, st, ms, streams, report):
        self.st, self.ms, self.streams, self.report = st, ms, streams, report


@pytest.fixture(scope="module")
def stall(probe, est):
    """Four non-blocking producer streams; both controls once on each; the first on which both read `old` (tests/stall.py)."""
    from tests.gpu_common import _log
    streams = []
    for _ in range(S.CANDIDATES):
        st = C.c_void_p()
        assert probe.ip_stream_create(C.byref(st)) == 0 and st.value
        streams.append(st.value)
    try:
        chosen, ms, report = S.choose_stream(probe, est, streams)
        _log("stream_order.json", report)
        if chosen is None:
            pytest.fail("the producer and consumer streams serialised on this machine: with VNECT_STREAM_SYNCED under a %g ms stall no "
                        "candidate stream let both the upload stream and a lane's stream read the old frame (%r) -- the ordering tests "
                        "would prove nothing here" % (ms, report["rounds"][-1]["controls"]))
        yield Stall(streams[chosen], ms, streams, report)
    finally:
        for st in streams:
            probe.ip_stream_sync(st)
            probe.ip_stream_destroy(st)


@pytest.fixture(scope="module")
def people_stall(probe, est, pest, stall):
    """The people handle's lanes are other streams than the plain handle's: the lane control once more on it (a paired people frame told
    VNECT_STREAM_SYNCED), on the same four candidates; the stream chosen above if it reads `old` there too, else the first that does."""
    from tests.gpu_common import _log
    video, rects = S.people_video()
    refs = tuple([S.track_ref(est, [video[k]], rects[q], S.times(1)) for q in range(2)] for k in (4, 0))
    st, outcomes = S.first_old(probe, stall.streams, lambda pool, s: S.control_people(probe, pool, pest, s, stall.ms, refs), prefer=stall.st)
    stall.report["people_lane"] = {"controls": outcomes, "chosen": None if st is None else stall.streams.index(st)}
    _log("stream_order.json", stall.report)
    if st is None:
        pytest.fail("the producer streams and the people handle's lane serialised on this machine: with VNECT_STREAM_SYNCED under a %g ms "
                    "stall a paired people frame read the new frame on every candidate stream (%r)" % (stall.ms, outcomes))
    return Stall(st, stall.ms, stall.streams, stall.report)


@pytest.fixture()
def pool(probe):
    p = S.Pool(probe)
    yield p
    p.close()


class Ctx:
    def __init__(self, request, probe, pool, est, stall):
        self.request, self.probe, self.pool, self.est, self.h, self.st, self.ms = request, probe, pool, est, est.handle, stall.st, stall.ms
        self.streams = stall.streams

    def people(self):
        """the people handle; from here on the stalled producer is the stream the people handle's own control chose"""
        self.st = self.request.getfixturevalue("people_stall").st
        return self.request.getfixturevalue("pest")

    def stalled(self, src, st="chosen"):
        """the source's buffer: it holds `old`, the producer fills it with `new` behind the stall -> (address, the library's frame)"""
        p = S.stalled_frame(self.probe, self.pool, self.st if st == "chosen" else st, src.bytes[0], src.bytes[1], self.ms)
        return p, src.frame(p)

    def sync(self, st="chosen"):
        assert self.probe.ip_stream_sync(self.st if st == "chosen" else st) == 0


@pytest.fixture()
def ctx(request, probe, pool, est, stall):
    c = Ctx(request, probe, pool, est, stall)
    yield c
    for st in c.streams:
        c.sync(st)
    est._orient(None)
    est.reset()


def _differ(a, b):
    """two runner.track tuples (or lists of them) differ in joints or rect"""
    if isinstance(a, list):
        return any(_differ(x, y) for x, y in zip(a, b))
    return list(a[2]) != list(b[2]) or not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1])


def _same(got, want, tag):
    """a collected (stream, joints_2d, joints_3d, rect_used) is the runner.track tuple, bit for bit"""
    assert list(got[3]) == list(want[2]), (tag, got[3], want[2])
    assert np.array_equal(got[1], want[0]), (tag, "joints_2d", float(np.abs(got[1] - want[0]).max()))
    assert np.array_equal(got[2], want[1]), (tag, "joints_3d", float(np.abs(got[2] - want[1]).max()))


# ---- the producer edge at every entry point --------------------------------------------------------------------------------------------------
@case("upload-packed-bgr", "upload-nv12", "upload-nv12-two", "upload-orient-3")
def _upload(c, name):
    """rt_ingest.cpp's wait via ingest_sync: the slot holds `new`"""
    src = S.Source(name[len("upload-"):], *S.pose_pair())
    assert not np.array_equal(src.seen(0), src.seen(1))
    c.est._orient(src.orientation)
    _, frame = c.stalled(src)
    c.h.upload_frame_device(1, frame, c.st)
    got = c.h.read_frame(1)
    assert got.shape == src.seen(1).shape and np.array_equal(got, src.seen(1)), (name, "old" if np.array_equal(got, src.seen(0)) else "neither")


@case("preprocess")
def _preprocess(c, name):
    src = S.Source("packed-bgr", *S.pose_pair())
    want, stale = c.h.preprocess(src.host[1]), c.h.preprocess(src.host[0])
    assert not np.array_equal(want[0], stale[0])
    _, frame = c.stalled(src)
    got = c.h.preprocess_device(frame, c.st)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and got[1:] == want[1:], name


@case("infer")
def _infer(c, name):
    src = S.Source("packed-bgr", *S.pose_pair())
    t = S.times(1)[0]
    c.est.reset()
    stale = c.est(src.host[0], timestamp=t)
    c.est.reset()
    want = c.est(src.host[1], timestamp=t)
    c.est.reset()
    assert not np.array_equal(want[0], stale[0]) and not np.array_equal(want[1], stale[1])
    p, _ = c.stalled(src)
    got = c.est(src.array(p), timestamp=t, stream=c.st)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name


@case("draw")
def _draw(c, name):
    """rt_draw.cpp's first wait: the overlay lands on `new` (one that did not wait is wiped out by the producer's copy)"""
    from vnect_amd import _native
    src = S.Source("packed-bgr", *S.pose_pair())
    j2, rect = S.skeleton()
    want = S.drawn(src.host[1], j2, rect)
    assert not np.array_equal(want, S.drawn(src.host[0], j2, rect)) and not np.array_equal(want, src.bytes[1])
    p, frame = c.stalled(src)
    c.h.draw_device(frame, j2, rect, None, _native.overlay_style(parents=c.est.joint_parents), c.st)
    got = c.pool.get(p)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def _preview_exact(picture, j2, rect, factor=0.5):
    from vnect_amd import render
    return render.preview_exact(picture, j2, R.PARENTS, None if rect is None else list(rect), factor=factor)


@case("preview")
def _preview(c, name):
    from vnect_amd import _native
    src = S.Source("packed-bgr", *S.pose_pair())
    j2, rect = S.skeleton()
    want = _preview_exact(src.host[1], j2, rect)
    assert not np.array_equal(want, _preview_exact(src.host[0], j2, rect))
    spec = _native.preview_spec(0.5)
    p, frame = c.stalled(src)
    assert c.h.preview_size(frame, spec) == want.shape[:2]
    got = np.zeros(want.shape, np.uint8)
    c.h.preview_device(frame, spec, got.ctypes.data, 3 * got.shape[1], j2, rect, None, _native.overlay_style(parents=c.est.joint_parents), c.st)
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    c.sync()
    assert np.array_equal(c.pool.get(p), src.bytes[1])               # (a preview writes no frame)


def _hog_source():
    return S.Source("packed-bgr", *S.hog_pair())


@case("hog")
def _hog(c, name):
    src = _hog_source()
    want, stale = c.h.hog_detect(src.host[1]), c.h.hog_detect(src.host[0])
    assert len(stale[0]) == 0 and len(want[0]) >= 1
    _, frame = c.stalled(src)
    got = c.h.hog_detect_device(frame, None, c.st)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, got, want)


def _begin(c, src, rect, stream=0, h=None):
    """vnect_track_begin for the source's picture under the source's orientation"""
    (c.est if h is None else h)._orient(src.orientation)
    (c.h if h is None else h.handle).track_begin(stream, src.H, src.W, rect)


@case("tracked-packed-bgr", "tracked-nv12", "tracked-nv12-two", "tracked-orient-3", "tracked-null-stream")
def _tracked(c, name):
    """rt_exec.cpp's run_pre_tracked: the stalled first frame and the (synchronised) frame after it are runner.track's on `new`, `new`.
    tracked-null-stream: producer_stream NULL is HIP's default stream -- the delayed copy is enqueued there (ip_delayed_copy with st NULL).
    The library's streams and the probe's are all non-blocking, so the default stream orders none of them by itself and the event the
    library records on it is what holds the frame back: the case is as meaningful as on any other stream.  (The fixture's controls are not
    run on the default stream; a library built without run_pre_tracked's wait fails this case like the other tracked ones.)"""
    from vnect_amd import _native
    null = name == "tracked-null-stream"
    src = S.Source("packed-bgr" if null else name[len("tracked-"):], *S.pose_pair())
    stamps = S.times(2)
    kw = dict(pixel_format=src.pixel_format, orientation=src.orientation)
    want = S.track_ref(c.est, [src.host[1], src.host[1]], S.RECT0, stamps, **kw)
    stale = S.track_ref(c.est, [src.host[0]], S.RECT0, stamps, **kw)
    assert _differ(want[0], stale[0])
    again = c.pool.put(src.bytes[1]) if not isinstance(src.bytes[1], tuple) else tuple(c.pool.put(b) for b in src.bytes[1])
    _begin(c, src, S.RECT0)
    st = None if null else c.st
    p, frame = c.stalled(src, st)
    c.h.submit_tracked_device(0, frame, *stamps[0], producer=0 if null else c.st)
    got = c.h.collect_tracked()
    c.h.submit_tracked_device(0, src.frame(again), *stamps[1], producer=_native.STREAM_SYNCED)
    got2 = c.h.collect_tracked()
    c.sync(st)
    _same(got, want[0], name)
    _same(got2, want[1], (name, "the next frame"))


@case("tracked-draw", "tracked-preview")
def _tracked_annotated(c, name):
    """the same with the overlay / the preview behind the frame's chain: the results, and the frame or the preview afterwards"""
    from vnect_amd import _native
    src = S.Source("packed-bgr", *S.pose_pair())
    stamps = S.times(1)
    want, stale = S.track_ref(c.est, [src.host[1]], S.RECT0, stamps), S.track_ref(c.est, [src.host[0]], S.RECT0, stamps)
    assert _differ(want[0], stale[0])
    style = _native.overlay_style(parents=c.est.joint_parents)
    _begin(c, src, S.RECT0)
    p, frame = c.stalled(src)
    if name == "tracked-draw":
        c.h.submit_tracked_device_draw(0, frame, *stamps[0], producer=c.st, style=style)
    else:
        c.h.submit_tracked_device_preview(0, frame, *stamps[0], producer=c.st, style=style, spec=_native.preview_spec(0.5))
    got = c.h.collect_tracked()
    pv = c.h.result_preview()
    _same(got, want[0], name)
    after = c.pool.get(p)
    if name == "tracked-draw":
        exp = S.drawn(src.host[1], got[1], got[3])
        assert pv is None and np.array_equal(after, exp), (name, int((after != exp).sum()))
    else:
        exp = _preview_exact(src.host[1], got[1], got[3])
        assert pv is not None and pv.shape == exp.shape and np.array_equal(pv, exp), name
        assert np.array_equal(after, src.bytes[1]), (name, "the frame was written")


class _Redetect:
    """vnect_track_redetect and the every-frame-is-lost rule on stream 0 of the detector's frames; off again at the end"""

    def __init__(self, c, src):
        self.c = c
        _begin(c, src, None)
        c.h.track_redetect(0, None, True)
        c.h.track_policy(0, S.ALWAYS[0], S.ALWAYS[1], "reset")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.h.track_redetect(0, None, False)
        self.c.h.track_policy(0, 0.0, 1, "off")


def _redetect_refs(c, src):
    """the host loop with lost=(.., "detect") on [new, new] and on [old, new]; new's detection (the largest, as hog_box picks it)"""
    from vnect_amd import runner
    stamps = S.times(2)
    want = S.track_ref(c.est, [src.host[1], src.host[1]], [0, 0, src.W, src.H], stamps, lost=S.ALWAYS + ("detect",))
    stale = S.track_ref(c.est, [src.host[0], src.host[1]], [0, 0, src.W, src.H], stamps, lost=S.ALWAYS + ("detect",))
    rects, _ = c.h.hog_detect(src.host[1])
    assert len(rects) >= 1 and len(c.h.hog_detect(src.host[0])[0]) == 0
    best = [int(v) for v in rects[int(np.argmax(rects[:, 2].astype(np.int64) * rects[:, 3]))]]
    box = runner.cal_rect(best, src.H, src.W)
    assert want[1][2] == box and stale[1][2] == [0, 0, src.W, src.H] and box != stale[1][2]      # the next box tells `new` from `old`
    return stamps, want, best, box


@case("redetect", "redetect-draw", "redetect-preview")
def _redetect(c, name):
    """vnect_track_redetect set and the frame lost: redetect_enqueue reads the whole frame behind the same wait.  Status, rect and hits
    are those of `new` (the hits: of the same frame submitted synchronised); the next box is hog_box of `new`, which the next frame is
    cropped with.  -draw and -preview (with draw_frame) also hold rt_exec.cpp's order behind the joints: the detector and the preview
    read the CLEAN frame -- the hits, the rect and the preview are those of clean `new` -- and the frame afterwards is `new` with the
    overlay."""
    from vnect_amd import _native
    src = _hog_source()
    stamps, want, best, box = _redetect_refs(c, src)
    style = _native.overlay_style(parents=c.est.joint_parents)
    again = c.pool.put(src.bytes[1])
    plain = c.pool.put(src.bytes[1])

    def submit(frame, producer):
        if name == "redetect":
            c.h.submit_tracked_device(0, frame, *stamps[0], producer=producer)
        elif name == "redetect-draw":
            c.h.submit_tracked_device_draw(0, frame, *stamps[0], producer=producer, style=style)
        else:
            c.h.submit_tracked_device_preview(0, frame, *stamps[0], producer=producer, style=style, spec=_native.preview_spec(0.5, "bgr", True))

    with _Redetect(c, src):             # the hits' reference: the same submit of a copy of `new`, nothing stalled (and whatever the form
        submit(src.frame(plain), _native.STREAM_SYNCED)              # allocates on first use exists before the stall begins)
        c.h.collect_tracked()
        status0, rect0, hits0 = c.h.result_redetect()
        assert (status0, rect0) == (1, best) and hits0 >= 3
    c.est.reset()
    with _Redetect(c, src):
        p, frame = c.stalled(src)
        submit(frame, c.st)
        got = c.h.collect_tracked()
        red, lost, pv = c.h.result_redetect(), c.h.result_confidence()[1], c.h.result_preview()
        nxt = c.h.track_box(0)
        c.h.submit_tracked_device(0, src.frame(again), *stamps[1], producer=_native.STREAM_SYNCED)
        got2 = c.h.collect_tracked()
    _same(got, want[0], name)
    assert lost == 1 and red == (1, best, hits0), (name, red, (1, best, hits0))
    assert nxt == box, (name, nxt, box)
    _same(got2, want[1], (name, "the next frame"))
    after = c.pool.get(p)
    if name == "redetect":
        assert pv is None and np.array_equal(after, src.bytes[1])
    else:
        exp = S.drawn(src.host[1], got[1], got[3])
        assert np.array_equal(after, exp), (name, "the frame afterwards", int((after != exp).sum()))
    if name == "redetect-preview":
        exp = _preview_exact(src.host[1], got[1], got[3])
        assert pv is not None and np.array_equal(pv, exp), (name, "the preview is not the clean frame's")


def _people_refs(c, frames, rects, stamps):
    """[person][frame]: runner.track for that person alone over the clean frames (on the plain estimator: the same precision and scales)"""
    return [S.track_ref(c.est, frames, rects[p], stamps) for p in range(len(rects))]


def _people_source(k_old, k_new):
    video, rects = S.people_video()
    return S.Source("packed-bgr", video[k_old], video[k_new]), rects


@case("people-2", "people-3")
def _people(c, name):
    """rt_exec.cpp's enqueue_pair (the pair's wait) and, for the third person, run_pre_tracked on a second lane: P = 2 is one paired
    unit, P = 3 a pair and a single unit; every person's tuple is runner.track's on `new`"""
    P = int(name[-1])
    src, rects = _people_source(4, 0)
    stamps = S.times(1)
    want, stale = _people_refs(c, [src.host[1]], rects[:P], stamps), _people_refs(c, [src.host[0]], rects[:P], stamps)
    assert all(_differ(want[p][0], stale[p][0]) for p in range(P))
    pe = c.people()
    pe.reset()
    pe.handle.people_begin(P, src.H, src.W, rects[:P])
    _, frame = c.stalled(src)
    pe.handle.submit_people_device(P, frame, *stamps[0], producer=c.st)
    got = [pe.handle.collect_tracked() for _ in range(P)]
    assert pe.handle.result_people() == (P - P // 2, P // 2)
    for p in range(P):
        assert got[p][0] == p
        _same(got[p], want[p][0], (name, p))


@pytest.mark.parametrize("entry,name", MATRIX, ids=[m[1] for m in MATRIX])
def test_the_consumer_waits_for_the_stalled_producer(ctx, entry, name):
    """one stalled call per row of MATRIX, on the stream the control chose, nothing synchronised: the result is the reference's on `new`"""
    CASES[name](ctx, name)


def test_every_case_is_a_row_and_every_row_a_case():
    assert sorted(CASES) == sorted(m[1] for m in MATRIX) and len(set(m[1] for m in MATRIX)) == len(MATRIX)


# ---- the contract's other sentences ----------------------------------------------------------------------------------------------------------
def test_one_producer_event_recorded_twice(ctx, probe):
    """The handle has ONE producer event.  Frame k of stream 0 comes from the stalled producer P1; straight after it frame k of stream 1
    comes from a second producer stream P2 that does not stall, and records the event again (lanes = 2: the two frames run on two lanes).
    Both results are their references: the first wait keeps the first record.  (Only correctness: stream 1 need not wait for the stall.)
    This handle's lanes are streams of its own, so P1 is chosen by the lane control on THIS handle, among the same four candidates."""
    e = _est(lanes=2)
    try:
        src = S.Source("packed-bgr", *S.pose_pair())
        other = S.moving_video(2)[1]
        stamps = S.times(1)
        rect1 = [20, 10, 120, 100]
        want0, stale0 = S.track_ref(e, [src.host[1]], S.RECT0, stamps), S.track_ref(e, [src.host[0]], S.RECT0, stamps)
        want1 = S.track_ref(e, [other], rect1, stamps)
        assert _differ(want0[0], stale0[0])
        p1, outcomes = S.first_old(probe, ctx.streams, lambda pool, st: S.control_lane(probe, pool, e, st, ctx.ms, (stale0, want0)), prefer=ctx.st)
        assert p1 is not None, ("this handle's lane serialised with every candidate producer stream", outcomes)
        p2 = [st for st in ctx.streams if st != p1][0]
        e.handle.track_begin(0, S.H, S.W, S.RECT0)
        e.handle.track_begin(1, S.H, S.W, rect1)
        blank = np.zeros_like(other)
        staged, f1 = ctx.pool.put(other), ctx.pool.put(blank)
        _, frame = ctx.stalled(src, p1)
        e.handle.submit_tracked_device(0, frame, *stamps[0], producer=p1)
        assert probe.ip_delayed_copy(p2, f1, staged, other.size, 0.0) == 0
        e.handle.submit_tracked_device(1, S.Source("packed-bgr", blank, other).frame(f1), *stamps[0], producer=p2)
        got = [e.handle.collect_tracked(), e.handle.collect_tracked()]
        assert [g[0] for g in got] == [0, 1]
        _same(got[0], want0[0], "stream 0, the stalled producer")
        _same(got[1], want1[0], "stream 1, the second producer")
    finally:
        for st in ctx.streams:
            ctx.sync(st)
        e.close()


@pytest.mark.parametrize("entry", ["upload", "infer", "preprocess"])
def test_done_with_the_callers_buffer_on_return(ctx, entry):
    """vnect_upload_frame_device, vnect_infer_device and vnect_preprocess_device are done with the caller's buffer when they return: it is
    overwritten with a blocking fill, and the slot the frame went into (slot 0 for the last two), run by vnect_submit_resident, still
    gives the result of `new`"""
    src = S.Source("packed-bgr", *S.pose_pair())
    stamps = S.times(2)
    ctx.est.reset()
    want = [ctx.est(src.host[1], timestamp=t) for t in stamps]
    ctx.est.reset()
    p, frame = ctx.stalled(src)
    slot, k = 0, 0
    if entry == "upload":
        slot = 2
        ctx.h.upload_frame_device(slot, frame, ctx.st)
    elif entry == "infer":
        got = ctx.h.infer_device(frame, *stamps[0], ctx.st)
        assert np.array_equal(got[0], want[0][0]) and np.array_equal(got[1], want[0][1])
        k = 1
    else:
        ctx.h.preprocess_device(frame, ctx.st)
    ctx.pool.fill(p, 0x5A)
    ctx.h.submit_resident(slot, *stamps[k])
    got = ctx.h.collect()
    assert np.array_equal(got[0], want[k][0]) and np.array_equal(got[1], want[k][1]), entry
    assert np.array_equal(ctx.h.read_frame(slot), src.host[1])


# ---- the hand-overs inside the runtime, under the same stall --------------------------------------------------------------------------------
def test_a_tracked_frame_waits_for_the_box_of_the_frame_before_it(ctx):
    """wait_prev of a tracked frame (enqueue_frame).  Three lanes; frame k of the moving video is stalled on lane 0; frame k + 1 is
    submitted with VNECT_STREAM_SYNCED at once and gets lane 1, because lane 0's frame is uncollected.  Its crop is frame k's box stage's
    output: taken before that stage has run it would be frame k's own crop (the box frame k - 1 left), which gives other joints -- asserted
    on the references first.  Every delivered tuple is runner.track's."""
    from vnect_amd import _native
    video = S.moving_video(3)
    stamps = S.times(3)
    rect = [2, 20, 90, 80]
    want = S.track_ref(ctx.est, video, rect, stamps)
    assert want[1][2] != want[2][2]                                  # the box moved between the two frames ...
    x, y, w, h = want[1][2]                                          # ... and frame k + 1 under frame k's crop gives other joints
    t = stamps[2]
    a = ctx.est(np.ascontiguousarray(video[2][y:y + h, x:x + w]), timestamp=t)
    ctx.est.reset()
    x2, y2, w2, h2 = want[2][2]
    b = ctx.est(np.ascontiguousarray(video[2][y2:y2 + h2, x2:x2 + w2]), timestamp=t)
    ctx.est.reset()
    assert not np.array_equal(a[0] + [y, x], b[0] + [y2, x2]) and not np.array_equal(a[1], b[1])
    src = S.Source("packed-bgr", video[0], video[1])
    first, nxt = ctx.pool.put(video[0]), ctx.pool.put(video[2])
    frame_of = S.Source("packed-bgr", video[0], video[2]).frame
    ctx.h.track_begin(0, S.H, S.W, rect)
    ctx.h.submit_tracked_device(0, frame_of(first), *stamps[0], producer=_native.STREAM_SYNCED)
    got = [ctx.h.collect_tracked()]
    _, frame = ctx.stalled(src)
    ctx.h.submit_tracked_device(0, frame, *stamps[1], producer=ctx.st)
    ctx.h.submit_tracked_device(0, frame_of(nxt), *stamps[2], producer=_native.STREAM_SYNCED)
    got += [ctx.h.collect_tracked(), ctx.h.collect_tracked()]
    for k in range(3):
        _same(got[k], want[k], ("frame", k))


def test_a_paired_people_unit_waits_for_both_persons_previous_frames(ctx):
    """wait_prev in enqueue_pair: people frame k (one paired unit, lane 0) is stalled; frame k + 1 comes with VNECT_STREAM_SYNCED at once
    and runs on lane 1.  Each person's crop is that person's previous box stage's output, and both boxes move from frame to frame."""
    from vnect_amd import _native
    video, rects = S.people_video()
    stamps = S.times(3)
    want = _people_refs(ctx, video[:3], rects[:2], stamps)
    assert all(want[p][1][2] != want[p][2][2] for p in range(2))
    src = S.Source("packed-bgr", video[0], video[1])
    first, nxt = ctx.pool.put(video[0]), ctx.pool.put(video[2])
    pe = ctx.people()
    pe.reset()
    pe.handle.people_begin(2, src.H, src.W, rects[:2])
    pe.handle.submit_people_device(2, src.frame(first), *stamps[0], producer=_native.STREAM_SYNCED)
    got = [[pe.handle.collect_tracked() for _ in range(2)]]
    _, frame = ctx.stalled(src)
    pe.handle.submit_people_device(2, frame, *stamps[1], producer=ctx.st)
    pe.handle.submit_people_device(2, src.frame(nxt), *stamps[2], producer=_native.STREAM_SYNCED)
    got += [[pe.handle.collect_tracked() for _ in range(2)] for _ in range(2)]
    for k in range(3):
        for p in range(2):
            assert got[k][p][0] == p
            _same(got[k][p], want[p][k], ("frame", k, "person", p))


def test_people_drawing_waits_for_every_person_under_a_stall(ctx):
    """The scene of tests/test_gpu_people.py's test_drawing_waits_for_every_persons_crop (person 0's limbs lie inside person 1's crop),
    P = 3 on three lanes, the frame's producer stalled: every unit waits for the producer, the drawing waits for every unit.  The results
    are the clean frame's references, the frame afterwards is `new` with P host draws in person order."""
    from vnect_amd import _native
    P = 3
    src, rects = _people_source(4, 3)                                # (not the frame of the people cases: the ring slots' old joints are other joints)
    stamps = S.times(1)
    want = _people_refs(ctx, [src.host[1]], rects[:P], stamps)
    assert all(_differ(want[q][0], w[0]) for q, w in enumerate(_people_refs(ctx, [S.people_video()[0][0]], rects[:P], stamps)))
    pe = ctx.people()
    pe.reset()
    pe.handle.people_begin(P, src.H, src.W, rects[:P])
    p, frame = ctx.stalled(src)
    pe.handle.submit_people_device(P, frame, *stamps[0], producer=ctx.st, style=_native.overlay_style(parents=pe.joint_parents))
    got = [pe.handle.collect_tracked() for _ in range(P)]
    for q in range(P):
        _same(got[q], want[q][0], ("person", q))
    exp = src.bytes[1].copy()
    lay = S.packed_layout(src.H, src.W)
    assert sum(R.draw(exp, lay, dict(name=None, joints=g[1], parents=R.PARENTS, rect=list(g[3]))) for g in got) > 0
    after = ctx.pool.get(p)
    assert np.array_equal(after, exp), int((after != exp).sum())
    x, y, w, h = got[1][3]                                           # the scene's premise: person 0's limbs inside person 1's crop
    j = got[0][1]
    assert np.all((j[:, 0] >= y) & (j[:, 0] < y + h) & (j[:, 1] >= x) & (j[:, 1] < x + w))


def test_collect_delivers_the_stalled_frames_own_values(ctx):
    """vnect_collect_tracked of the stalled frame returns that frame's values, not what its ring slot held before: the ring (8 entries) is
    filled first with 8 earlier frames of the moving video, whose joints all differ from the stalled frame's"""
    from vnect_amd import _native
    n = 8
    video = S.moving_video(n + 1)
    stamps = S.times(n + 1)
    rect = [2, 20, 90, 80]
    want = S.track_ref(ctx.est, video, rect, stamps)
    assert all(_differ(want[k], want[n]) for k in range(n))
    src = S.Source("packed-bgr", video[n - 1], video[n])
    ctx.h.track_begin(0, S.H, S.W, rect)
    got = []
    for k in range(n):
        ctx.h.submit_tracked_device(0, src.frame(ctx.pool.put(video[k])), *stamps[k], producer=_native.STREAM_SYNCED)
        got.append(ctx.h.collect_tracked())
    _, frame = ctx.stalled(src)
    ctx.h.submit_tracked_device(0, frame, *stamps[n], producer=ctx.st)
    got.append(ctx.h.collect_tracked())
    for k in range(n + 1):
        _same(got[k], want[k], ("frame", k))
