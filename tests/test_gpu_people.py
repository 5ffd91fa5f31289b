"""GPU: people mode (vnect_set_people / vnect_people_begin / vnect_submit_people*, runner.track_people_on_device; PEOPLE.md).

P persons of one video on one handle, person p on stream p, one submit per frame, two persons' crops through one conv stack where the
handle has the pair plan.  Every person's joints_2d, joints_3d, rect_used, confidences and lost flag must be BIT-identical to runner.track
for that person alone, on an estimator of its own, over the same clean frames from the same first rect -- paired or not, in every
precision, graph mode, lane count, depth and source.  The references are computed once per (precision, scales, video) and shared.
Device frames come from the device-frame probe's allocator behind a bare __cuda_array_interface__ (tests/devframe_ref.py: FakeCuda), as in
tests/test_gpu_overlay.py; real torch tensors, written on a side stream, go through the loop in a child process that imports torch first
(tests/people_torch_child.py)."""
import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import overlay_ref as R

pytestmark = pytest.mark.gpu

T0 = 1.7e9
N = 6
SMALL, WIDE = (96, 128), (270, 480)
S3, S1, S5 = (1.0, 0.8, 0.6), (1.0,), (1.0, 0.9, 0.8, 0.7, 0.6)
BRIGHT = (0, 1, 3)                                                   # the frames in which the persons are bright; dim in the others
CENTRES = [(0.32, 0.26), (0.64, 0.70), (0.36, 0.74), (0.70, 0.30)]   # (row, column) of person p, as fractions of the frame
_CACHE = {}


def _planted():
    if "w" not in _CACHE:
        from tests import planted
        _CACHE["w"] = planted.weights(noise=1.0)
    return _CACHE["w"]


def _video(size, n=N):
    """n planted-weights frames with four persons: person p is three blobs (one per colour) around CENTRES[p], drifting and breathing,
    so every person's box changes from frame to frame."""
    if size not in _CACHE:
        from tests import planted
        H, W = size
        m = min(H, W)
        out = []
        for k in range(n):
            blobs = []
            for p, (fy, fx) in enumerate(CENTRES):
                cy, cx = H * fy + 0.03 * m * np.sin(k / 2.0 + p), W * fx + 0.04 * m * np.cos(k / 3.0 + 2 * p)
                r = m * (0.07 + 0.02 * np.sin(k / 1.5 + p))
                amp = (255.0 - 12.0 * p) * (1.0 if k in BRIGHT else 0.45)   # (everybody dims together: a crop holding several persons dims too)
                blobs += [(cy - 0.8 * r, cx, 0, amp), (cy + 0.9 * r, cx - 1.2 * r, 1, amp), (cy + 0.3 * r, cx + 1.5 * r, 2, amp)]
            out.append(planted.scene(H, W, blobs, sigma=max(2.0, 0.035 * m), seed=40 + k, texture=0.15))
        _CACHE[size] = out
    return _CACHE[size]


def _rects(size, P):
    """first rects around the persons, overlapping their neighbours'; person 1's is wide enough to hold person 0"""
    H, W = size
    out = []
    for p, (fy, fx) in enumerate(CENTRES[:P]):
        x0, y0 = max(int(W * (fx - 0.24)), 0), max(int(H * (fy - 0.27)), 0)
        out.append([x0, y0, min(int(W * 0.5), W - x0), min(int(H * 0.55), H - y0)])
    if P >= 2:
        out[1] = [2, 1, W - 5, H - 3]
    return out


def _times(n=N, base=0.0):
    return [(T0 + base + 0.033 * k + 0.002 * (k % 3), T0 + base + 0.033 * k + 0.0005) for k in range(n)]


def _est(**kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=_planted(), verbose=False, **kw)


def _reference(precision, scales, size, P, lost=None, pixel_format="bgr", orientation=0):
    """runner.track per person, each on an estimator of its own: [person][frame] = (j2, j3, rect, conf, lost).  Kept and never changed."""
    from vnect_amd import pixfmt, runner
    out = []
    for p in range(P):
        key = ("ref", precision, scales, size, p, lost, pixel_format, orientation)
        if key not in _CACHE:
            frames = _video(size)
            if orientation:                      # the stored frames of a video whose PICTURE is _video's: turned back
                frames = [_stored(f, orientation) for f in frames]
            if pixel_format == "nv12":
                frames = [pixfmt.bgr_to_nv12(f) for f in frames]
            est = _est(precision=precision, scales=list(scales))
            try:
                _CACHE[key] = [(a, b, list(c), d, e) for a, b, c, d, e in
                               runner.track(est, frames, rect=list(_rects(size, 4)[p]), timestamps=_times(),
                                            confidence=True, lost=lost, pixel_format=pixel_format, orientation=orientation)]
            finally:
                est.close()
        out.append(_CACHE[key])
    return out


def _stored(picture, o):
    """the array that is stored under orientation code o when the picture is `picture` (the inverse of runner.orient_view)"""
    g = picture[:, ::-1] if o & 4 else picture
    return np.ascontiguousarray(np.rot90(g, -(o & 3)))


def _same(got, want, tag):
    """got: [frame] = (people list,); want: [person][frame]"""
    assert len(got) == len(want[0]), (tag, len(got))
    for k, res in enumerate(got):
        people = res[0]
        assert len(people) == len(want), (tag, k, len(people))
        for p, g in enumerate(people):
            w = want[p][k]
            assert list(g[2]) == w[2], (tag, k, p, g[2], w[2])
            assert np.array_equal(g[0], w[0]), (tag, k, p, np.abs(g[0] - w[0]).max())
            assert np.array_equal(g[1], w[1]), (tag, k, p, np.abs(g[1] - w[1]).max())
            assert np.array_equal(g[3], w[3]) and g[4] == w[4], (tag, k, p)


def _run(P, size=SMALL, precision="fp32", scales=S3, pair=True, ahead=0, source="resident", frames=None, expect_pairs=None, **kw):
    from vnect_amd import runner
    run_kw = {k: kw.pop(k) for k in ("lost", "pixel_format", "orientation", "draw") if k in kw}
    est = _est(precision=precision, scales=list(scales), people=P, pair_people=pair, **kw)
    try:
        rects = _rects(size, P)
        got = list(runner.track_people_on_device(est, _video(size) if frames is None else frames, rects, timestamps=_times(), ahead=ahead,
                                                 source=source, confidence=True, **run_kw))
        units, paired = est.handle.result_people()
        if expect_pairs is None:
            expect_pairs = P // 2 if pair and 2 * len(scales) <= 8 else 0
        assert paired == expect_pairs and units == P - expect_pairs, (P, pair, units, paired)
        return got
    finally:
        est.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_every_person_equals_its_own_loop(P, precision):
    """P = 1 .. 4 in every precision: pairs (0, 1) and (2, 3), an odd last person single; vnect_result_people says so."""
    _same(_run(P, precision=precision), _reference(precision, S3, SMALL, P), (P, precision))


def test_box_launch_switch_inside_a_people_frame(monkeypatch):
    """VNECT_TRACK_BOX_LAUNCH=1 with P = 3: the frame is a paired unit, which ignores the switch (PEOPLE.md, Limits), and a single unit,
    which honours it -- 2 units, 1 pair (_run asserts it), and every person's results are still the references' bit for bit."""
    want = _reference("bf16", S3, SMALL, 3)
    monkeypatch.setenv("VNECT_TRACK_BOX_LAUNCH", "1")
    _same(_run(3, precision="bf16"), want, (3, "bf16", "box launch"))


@pytest.mark.parametrize("P,precision,scales", [(4, "fp32", S1), (3, "bf16", S1), (3, "bf16", S5), (2, "fp32", S5)])
def test_one_scale_pairs_and_five_scales_run_singly(P, precision, scales):
    """[1.0]: a pair is two images.  Five scales: 2 S > 8, there is no pair plan, the people run singly, and that is not an error."""
    _same(_run(P, precision=precision, scales=scales), _reference(precision, scales, SMALL, P), (P, precision, scales))


@pytest.mark.parametrize("P,use_graph,lanes,ahead,size", [(2, False, 1, 0, WIDE), (2, True, 1, 1, SMALL), (3, "auto", 1, 1, SMALL), (2, "auto", 3, 1, WIDE),
                                                           (4, True, 3, 1, SMALL), (3, False, 3, 0, SMALL), (4, "auto", 3, 0, WIDE)])
def test_graph_modes_lanes_and_depths(P, use_graph, lanes, ahead, size):
    """use_graph 0 / 1 / 2, lanes 1 and 3, ahead 0 and 1 (clipped where a frame's units leave no room for a second frame)"""
    got = _run(P, size=size, precision="bf16", ahead=ahead, use_graph=use_graph, lanes=lanes)
    _same(got, _reference("bf16", S3, size, P), (P, use_graph, lanes, ahead, size))


@pytest.mark.parametrize("P,precision,lanes", [(2, "fp32", 1), (3, "bf16", 3), (4, "fp16", 1)])
def test_unpaired_gives_the_same_bits_and_no_pairs(P, precision, lanes):
    """pair=False: no unit is paired (vnect_result_people), and the results are the paired run's, which are the references'"""
    got = _run(P, precision=precision, pair=False, lanes=lanes, ahead=1)
    _same(got, _reference(precision, S3, SMALL, P), (P, precision, "unpaired"))


class _Pool:
    """device copies of host buffers (the device-frame probe's allocator), freed at the test's end"""

    def __init__(self):
        from tests import test_gpu_overlay as ov
        self.pool = ov.Pool(dr.load_probe())

    def packed(self, frame):
        H, W = frame.shape[:2]
        p = self.pool.put(frame)
        return p, dr.FakeCuda(p, (H, W, 3), (3 * W, 3, 1))

    def nv12(self, frame):
        from vnect_amd import pixfmt
        H, W = frame.shape[:2]
        p = self.pool.put(pixfmt.bgr_to_nv12(frame))
        return p, dr.FakeCuda(p, (H * 3 // 2, W), (W, 1))


@pytest.fixture()
def pool():
    p = _Pool()
    yield p
    p.pool.close()


@pytest.mark.parametrize("P,precision,size,lanes,ahead", [(3, "bf16", WIDE, 3, 1), (4, "fp32", SMALL, 1, 0), (2, "fp16", SMALL, 2, 1)])
def test_frames_in_device_memory(pool, P, precision, size, lanes, ahead):
    dev = [pool.packed(f)[1] for f in _video(size)]
    got = _run(P, size=size, precision=precision, source="device", frames=dev, lanes=lanes, ahead=ahead)
    _same(got, _reference(precision, S3, size, P), (P, precision, "device"))


@pytest.mark.parametrize("source", ["device", "resident"])
def test_nv12_frames(pool, source):
    from vnect_amd import pixfmt
    frames = [pool.nv12(f)[1] for f in _video(SMALL)] if source == "device" else [pixfmt.bgr_to_nv12(f) for f in _video(SMALL)]
    got = _run(3, precision="bf16", source=source, frames=frames, pixel_format="nv12", lanes=2, ahead=1)
    _same(got, _reference("bf16", S3, SMALL, 3, pixel_format="nv12"), ("nv12", source))


@pytest.mark.parametrize("source", ["device", "resident"])
def test_frames_stored_under_orientation_3(pool, source):
    """the video's picture is _video's; its frames are stored quarter-turned (ORIENTATION.md): the crops are turned on the device"""
    stored = [_stored(f, 3) for f in _video(SMALL)]
    frames = [pool.packed(f)[1] for f in stored] if source == "device" else stored
    got = _run(2, precision="fp32", source=source, frames=frames, orientation=3)
    _same(got, _reference("fp32", S3, SMALL, 2, orientation=3), ("orientation 3", source))


@pytest.mark.parametrize("P,lanes,ahead", [(2, 1, 1), (4, 3, 0), (3, 2, 1)])
def test_drawing_waits_for_every_persons_crop(pool, P, lanes, ahead):
    """Person 1's first rect is nearly the whole frame: person 0's limbs and band lie inside person 1's crop.  With draw=True every
    person's results are still the references' (those of clean frames), and every frame afterwards is P host draws in person order."""
    ptrs, dev = zip(*[pool.packed(f) for f in _video(SMALL)])
    got = _run(P, precision="bf16", source="device", frames=list(dev), lanes=lanes, ahead=ahead, draw=True)
    _same(got, _reference("bf16", S3, SMALL, P), ("draw", P, lanes, ahead))
    H, W = SMALL
    lay = dict(name=None, format=0, H=H, W=W, data_off=0, uv_off=0, sy=3 * W, sx=3, sc=1, uv_stride=0, size=H * W * 3)
    for k, res in enumerate(got):
        exp = _video(SMALL)[k].reshape(-1).copy()
        drawn = sum(R.draw(exp, lay, dict(name=None, joints=g[0], parents=R.PARENTS, rect=list(g[2]))) for g in res[0])
        assert drawn > 0 and np.array_equal(pool.pool.get(ptrs[k]), exp), (k, int((pool.pool.get(ptrs[k]) != exp).sum()))
    # the scene's premise: person 0's first limbs lie inside person 1's first crop
    x, y, w, h = got[0][0][1][2]
    j = got[0][0][0][0]
    assert np.all((j[:, 0] >= y) & (j[:, 0] < y + h) & (j[:, 1] >= x) & (j[:, 1] < x + w))


@pytest.mark.parametrize("P,lanes,ahead", [(3, 1, 0), (4, 3, 1)])
def test_every_delivery_carries_its_persons_3d_view(P, lanes, ahead):
    """view3d=True: each person's tuple ends with render.view3d_exact of the joints_3d yielded with it, for a paired and a single unit, and
    the other results are those without views"""
    from vnect_amd import render, runner
    est = _est(precision="bf16", scales=list(S3), people=P, pair_people=True, lanes=lanes)
    try:
        got = list(runner.track_people_on_device(est, _video(SMALL), _rects(SMALL, P), timestamps=_times(), ahead=ahead, source="resident",
                                                 confidence=True, view3d=True))
    finally:
        est.close()
    _same(got, _reference("bf16", S3, SMALL, P), ("view3d", P))
    for k, res in enumerate(got):
        for p, g in enumerate(res[0]):
            assert len(g) == 6 and np.array_equal(g[5], render.view3d_exact(g[1])), (k, p)


@pytest.mark.parametrize("action", ["hold", "reset"])
def test_loss_rule_per_person(action):
    """The threshold is the median of the reference loops' own confidences over the run; it must call frames lost AND kept for every
    person, or the scene is no test of the rule.  hold and reset each equal runner.track(..., lost=...) per person."""
    P = 3
    plain = _reference("bf16", S3, SMALL, P)
    thr = float(np.median(np.concatenate([f[3] for person in plain for f in person])))
    need = 11
    rule = (thr, need, action)
    want = _reference("bf16", S3, SMALL, P, lost=rule)
    for p, person in enumerate(want):
        flags = [f[4] for f in person]
        assert 0 < sum(flags) < len(flags), (p, flags, thr)
    _same(_run(P, precision="bf16", lost=rule, lanes=2, ahead=1), want, ("lost", action))


def _submit_collect(h, P, frame, t, slot=0):
    h.upload_frame(slot, frame)
    h.submit_people(P, slot, *t)
    return [h.collect_tracked() for _ in range(P)]


def test_refused_submits_change_nothing():
    """Every refusal of vnect_submit_people comes before anything changes: after each of them the next valid frame gives exactly what
    an unrefused run gives."""
    from vnect_amd import _native
    P = 3
    want = _reference("fp32", S3, SMALL, P)
    frames, times = _video(SMALL), _times()
    H, W = SMALL
    est = _est(scales=list(S3), people=P, pair_people=True, lanes=1)
    h = est.handle

    def refused(code, fn):
        with pytest.raises(_native.VnectError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    def check(k, got):
        for p, (s, j2, j3, r) in enumerate(got):
            assert s == p and r == want[p][k][2] and np.array_equal(j2, want[p][k][0]) and np.array_equal(j3, want[p][k][1]), (k, p)

    try:
        h.upload_frame(0, frames[0])
        refused(_native.E_STATE, lambda: h.submit_people(P, 0, *times[0]))            # nobody tracks yet
        h.people_begin(P, H, W, _rects(SMALL, P))
        check(0, _submit_collect(h, P, frames[0], times[0]))
        h.upload_frame(1, frames[1])
        refused(_native.E_TIMESTAMP, lambda: h.submit_people(P, 1, *times[0]))        # an equal timestamp
        refused(_native.E_ARG, lambda: h.submit_people(P + 1, 1, *times[1]))          # more persons than vnect_set_people's n
        refused(_native.E_ARG, lambda: h.submit_people(0, 1, *times[1]))
        h.upload_frame(2, np.zeros((H + 2, W, 3), np.uint8))
        refused(_native.E_ARG, lambda: h.submit_people(P, 2, *times[1]))              # a frame of another size
        refused(_native.E_ARG, lambda: h.submit_people(P, 3, *times[1]))              # an empty slot
        check(1, _submit_collect(h, P, frames[1], times[1], 1))
        # too many in flight: a frame of 3 persons is 2 units, a lanes=1 handle holds 2
        h.upload_frame(0, frames[2])
        h.submit_people(P, 0, *times[2])
        h.upload_frame(1, frames[3])
        refused(_native.E_STATE, lambda: h.submit_people(P, 1, *times[3]))
        check(2, [h.collect_tracked() for _ in range(P)])
        check(3, _submit_collect(h, P, frames[3], times[3], 1))
        # people_begin is all or nothing: person 2's rect starts outside the frame, and persons 0 and 1 keep their boxes
        boxes = [h.track_box(p) for p in range(P)]
        refused(_native.E_ARG, lambda: h.people_begin(P, H, W, [[0, 0, 10, 10], [1, 1, 10, 10], [W, 0, 5, 5]]))
        assert [h.track_box(p) for p in range(P)] == boxes
        check(4, _submit_collect(h, P, frames[4], times[4]))
        # re-detection is refused on a people handle; the per-stream calls work
        refused(_native.E_ARG, lambda: h.track_redetect(0, None, True))
        h.track_policy(1, 0.0, 1, "off")
        check(5, _submit_collect(h, P, frames[5], times[5]))
    finally:
        est.close()


def test_a_stopped_person_refuses_the_whole_frame():
    """One stream stopped at a refused crop (its first rect, 1 row of 1000 columns, which squarify refuses): its delivery fails, the other
    person's frame is delivered, and the next submit is refused as a whole with VNECT_E_STATE, leaving the other person as it was."""
    from vnect_amd import _native, runner
    from tests import planted
    H, W = 60, 1000
    frames = [planted.scene(H, W, [(30, 200 + 5 * k, 0, 255.0), (20, 240, 1, 255.0), (40, 260, 2, 255.0)], sigma=4.0, seed=k) for k in range(3)]
    times = _times(3, 50.0)
    ok_rect = [100, 0, 400, 60]
    ref = _est()
    want = list(runner.track(ref, frames, rect=ok_rect, timestamps=times))
    ref.close()
    est = _est(people=2, pair_people=True)
    h = est.handle
    try:
        h.people_begin(2, H, W, [ok_rect, [0, 10, 1000, 1]])
        h.upload_frame(0, frames[0])
        h.submit_people(2, 0, *times[0])
        s, j2, j3, r = h.collect_tracked()
        assert s == 0 and r == list(want[0][2]) and np.array_equal(j2, want[0][0]) and np.array_equal(j3, want[0][1])
        with pytest.raises(_native.VnectError) as e:
            h.collect_tracked()
        assert e.value.code == _native.E_ARG
        h.upload_frame(1, frames[1])
        with pytest.raises(_native.VnectError) as e:
            h.submit_people(2, 1, *times[1])
        assert e.value.code == _native.E_STATE
        # person 0 alone goes on from where it was: the refused submit touched nothing of it
        h.submit_people(1, 1, *times[1])
        s, j2, j3, r = h.collect_tracked()
        assert s == 0 and r == list(want[1][2]) and np.array_equal(j2, want[1][0]) and np.array_equal(j3, want[1][1])
    finally:
        est.close()


def test_set_people_refusals_and_handles_without_people_mode():
    from vnect_amd import _native
    h = _native.Handle([1.0, 0.7], stream_batch=2)
    for fn in (lambda: h.set_people(2), lambda: h.track_begin(0, 96, 128)):   # not together; and the batch handle still refuses tracking
        with pytest.raises(_native.VnectError) as e:
            fn()
        assert e.value.code == _native.E_ARG
    h.close()
    h = _native.Handle([1.0], people=2)
    with pytest.raises(_native.VnectError) as e:
        h.set_stream_batch(2)
    assert e.value.code == _native.E_ARG
    for n in (0, 5):
        with pytest.raises(_native.VnectError) as e:
            h.set_people(n)
        assert e.value.code == _native.E_ARG
    h.close()
    h = _native.Handle([1.0], pyramid=(0, 1))
    with pytest.raises(_native.VnectError) as e:
        h.set_people(2)
    assert e.value.code == _native.E_ARG
    h.close()
    est = _est()
    try:
        with pytest.raises(_native.VnectError) as e:
            est.handle.set_people(2)                       # after finalize
        assert e.value.code == _native.E_STATE
        with pytest.raises(_native.VnectError) as e:
            est.handle.people_begin(1, 96, 128)            # not a people handle
        assert e.value.code == _native.E_STATE
    finally:
        est.close()


@pytest.mark.parametrize("P,draw,lanes,ahead,factor", [(2, False, 1, 0, 0.5), (4, True, 3, 0, 1.7), (3, True, 2, 1, None), (1, False, 1, 1, 0.37)])
def test_one_preview_picture_per_frame(pool, P, draw, lanes, ahead, factor):
    """preview=: every frame yields ONE picture, the numpy composition -- render.draw_limbs_2d_exact P times in person order on the clean
    frame, then render.resize_u8_exact -- with and without draw; the results are the references'; without draw the frame is not written,
    with it the frame is the P host draws."""
    from vnect_amd import render, runner
    ptrs, dev = zip(*[pool.packed(f) for f in _video(SMALL)])
    est = _est(precision="bf16", scales=list(S3), people=P, pair_people=True, lanes=lanes)
    try:
        got = list(runner.track_people_on_device(est, list(dev), _rects(SMALL, P), timestamps=_times(), ahead=ahead, source="device", confidence=True,
                                                 draw=draw, preview=True if factor is None else factor))
    finally:
        est.close()
    _same(got, _reference("bf16", S3, SMALL, P), ("preview", P, draw))
    f = 1024.0 / max(SMALL) if factor is None else factor
    for k, res in enumerate(got):
        assert len(res) == 2
        drawn = _video(SMALL)[k]
        for g in res[0]:
            drawn = render.draw_limbs_2d_exact(drawn, g[0], R.PARENTS, list(g[2]))
        assert np.array_equal(res[1], render.resize_u8_exact(drawn, f)), (k, P, draw)
        after = pool.pool.get(ptrs[k]).reshape(drawn.shape)
        assert np.array_equal(after, drawn if draw else _video(SMALL)[k]), (k, "the frame afterwards")


def test_the_picture_comes_with_the_last_person_only(pool):
    from vnect_amd import _native
    P = 3
    _, dev = pool.packed(_video(SMALL)[0])
    est = _est(precision="bf16", scales=list(S3), people=P, pair_people=True)
    h = est.handle
    try:
        h.people_begin(P, SMALL[0], SMALL[1], _rects(SMALL, P))
        frame = _native.device_frame(dev, "bgr")
        h.submit_people_device(P, frame, *_times()[0], _native.STREAM_SYNCED, None, _native.preview_spec(0.5))
        seen = []
        for p in range(P):
            h.collect_tracked()
            seen.append(h.result_preview())
        assert seen[0] is None and seen[1] is None and seen[2] is not None and seen[2].shape == (48, 64, 3)
        h.submit_people_device(P, frame, *_times()[1], _native.STREAM_SYNCED)        # a frame without a picture has none
        for p in range(P):
            h.collect_tracked()
            assert h.result_preview() is None
    finally:
        est.close()


def test_torch_tensors_written_on_a_side_stream():
    """the torch child (tests/people_torch_child.py): CUDA tensors written on a side stream go through track_people_on_device with draw and
    preview"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "tests.people_torch_child"], cwd=dr.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "people child ok"
