"""GPU: the tracking loop with the crop box on the device (vnect_track_begin / vnect_submit_tracked*, runner.track_on_device).

The reference's tracking script (run_estimator_ps.py:80-109) -- restated on the host as runner.track -- crops each frame with the box it grew
from the previous frame's joints.  On the device every frame's joints_2d (frame coordinates), joints_3d and rect_used must be BIT-identical
to runner.track driving a VNectEstimator of the same configuration, in every precision, graph mode, lane count, submission depth and
frame source."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 1.7e9
H, W = 480, 640
_CACHE = {}


def _planted(noise=1.0):
    if noise not in _CACHE:
        from tests import planted
        _CACHE[noise] = planted.weights(noise=noise)
    return _CACHE[noise]


def _video(n=48, H=H, W=W, seed=0, texture=0.15, white=False):
    """A planted-weights video: one blob per colour (joint j sits on the blob of colour j % 3) moving across the frame while the blobs'
    spread grows and shrinks, so the joints' box -- and with it the crop -- changes size and place every frame.  white: the three blobs
    on ONE spot (every joint on the same pixel: a degenerate box, the loop's fallback to the whole frame)."""
    from tests import planted
    out = []
    for k in range(n):
        cy = H * (0.35 + 0.25 * np.sin(k / 7.0))
        cx = W * (0.30 + 0.40 * k / max(n - 1, 1))
        r = 25 + 45 * (0.5 + 0.5 * np.sin(k / 3.0))
        if white:
            blobs = [(cy, cx, c, 230.0) for c in range(3)]
        else:
            blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
        out.append(planted.scene(H, W, blobs, sigma=9.0, seed=seed + k, texture=texture))
    return out


def _times(n, s=0):
    return [(T0 + 5 * s + 0.033 * k + 0.002 * (k % 3), T0 + 5 * s + 0.033 * k + 0.0005) for k in range(n)]


def _est(weights, **kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=weights, verbose=False, **kw)


def _host(weights, frames, times, rect=None, transpose=False, **kw):
    from vnect_amd import runner
    est = _est(weights, **kw)
    try:
        return [(j2, j3, list(u)) for j2, j3, u in runner.track(est, frames, rect=rect, transpose=transpose, timestamps=times)]
    finally:
        est.close()


def _device(weights, frames, times, rect=None, transpose=False, ahead=1, source="pinned", **kw):
    from vnect_amd import runner
    est = _est(weights, **kw)
    try:
        return [(j2, j3, list(u)) for j2, j3, u in runner.track_on_device(est, frames, rect=rect, transpose=transpose, timestamps=times,
                                                                           ahead=ahead, source=source)]
    finally:
        est.close()


def _assert_same(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, ((g2, g3, gr), (w2, w3, wr)) in enumerate(zip(got, want)):
        assert gr == wr, (tag, k, gr, wr)
        assert np.array_equal(g2, w2), (tag, k, np.abs(g2 - w2).max())
        assert np.array_equal(g3, w3), (tag, k, np.abs(g3 - w3).max())


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("source", ["pinned", "resident"])
def test_tracked_video_equals_runner_track(precision, source):
    """48 frames of a moving, growing and shrinking person at 640 x 480: the box changes every frame; every frame's joints and rect equal
    runner.track's."""
    w = _planted()
    frames, times = _video(), _times(48)
    want = _host(w, frames, times, precision=precision)
    rects = [tuple(r) for _, _, r in want]
    assert sum(a != b for a, b in zip(rects, rects[1:])) >= 40, rects   # the crop moves (and resizes) nearly every frame
    assert len({(r[2], r[3]) for r in rects}) >= 20, rects
    got = _device(w, frames, times, source=source, precision=precision)
    _assert_same(got, want, (precision, source))


@pytest.mark.parametrize("use_graph,lanes,ahead", [(False, 1, 0), (True, 1, 1), ("auto", 1, 2), (False, 3, 2), (True, 3, 1),
                                                   ("auto", 3, 2), ("auto", 3, 0), (True, 3, 2)])
@pytest.mark.parametrize("source", ["pinned", "resident"])
def test_graph_modes_lanes_and_depths(use_graph, lanes, ahead, source):
    w = _planted()
    frames, times = _video(32, seed=300), _times(32, 1)
    want = _host(w, frames, times, rect=[40, 30, 500, 400], use_graph=use_graph, lanes=lanes)
    got = _device(w, frames, times, rect=[40, 30, 500, 400], ahead=ahead, source=source, use_graph=use_graph, lanes=lanes)
    _assert_same(got, want, (use_graph, lanes, ahead, source))


def test_transposed_video():
    """The reference's `T` option: every frame rotated (np.rot90(frame, 3)) on the host, the box in the rotated frame's coordinates."""
    w = _planted()
    frames, times = _video(24, seed=500), _times(24, 2)
    want = _host(w, frames, times, transpose=True, precision="bf16")
    got = _device(w, frames, times, transpose=True, ahead=1, precision="bf16")
    _assert_same(got, want, "transpose")


def test_degenerate_box_falls_back_to_the_whole_frame():
    """Every joint on one pixel (three blobs on one spot, no texture, no noise in the heat-maps): the joints' box is zero pixels wide, and
    the loop crops the whole frame next (runner.track's fallback) -- on the device too.  The initial rect, degenerate as well, takes
    the same fallback."""
    w = _planted(noise=0.0)
    frames, times = _video(16, seed=700, texture=0.0, white=True), _times(16, 3)
    want = _host(w, frames, times, rect=[10, 10, 0, 50])
    assert sum(r == [0, 0, W, H] for _, _, r in want[1:]) >= 1, [r for _, _, r in want]
    got = _device(w, frames, times, rect=[10, 10, 0, 50], ahead=1)
    _assert_same(got, want, "fallback")


def test_two_tracked_streams_and_an_untracked_one_interleaved():
    """Streams 0 and 1 tracked (resident and pinned frames), stream 2 plain vnect_submit_stream frames, interleaved three deep on a
    lanes=3 handle: each equals its own loop (runner.track / the estimator frame by frame) on a handle of its own."""
    from vnect_amd import _native
    w = _planted()
    n = 20
    va, vb = _video(n, seed=900), _video(n, seed=950)[::-1]
    vc = [f[100:468, 50:418] for f in _video(n, seed=990)]
    ta, tb, tc = _times(n, 4), _times(n, 5), _times(n, 6)
    want_a = _host(w, va, ta, rect=[0, 0, 400, 300])
    want_b = _host(w, vb, tb)
    own = _est(w)
    want_c = [own(f, timestamp=t) for f, t in zip(vc, tc)]
    own.close()
    est = _est(w, lanes=3)
    h = est.handle
    h.track_begin(0, H, W, [0, 0, 400, 300])
    h.track_begin(1, H, W)
    buf = [h.frame_buffer(b, H, W) for b in range(2)]
    got = {0: [], 1: [], 2: []}
    inflight, count = [], 0

    def collect():
        s, j2, j3, r = h.collect_tracked()
        got[s].append((j2, j3, r))
        inflight.pop(0)

    for k in range(n):
        for s in range(3):
            while len(inflight) >= 3 or (s == 1 and (1, k - 2) in inflight):   # (a pinned buffer is rewritten after its frame's collect)
                collect()
            slot = count % 4
            if s == 0:
                h.upload_frame(slot, va[k])
                h.submit_tracked(0, slot, *ta[k])
            elif s == 1:
                buf[k % 2][...] = vb[k]
                h.submit_tracked_pinned(1, k % 2, W * 3, *tb[k])
            else:
                h.upload_frame(slot, vc[k])
                h.submit_stream(2, slot, *tc[k])
            inflight.append((s, k))
            count += 1
    while inflight:
        collect()
    est.close()
    _assert_same(got[0], want_a, "stream 0")
    _assert_same(got[1], want_b, "stream 1")
    assert all(r == [-1, -1, -1, -1] for _, _, r in got[2])
    for k, ((g2, g3, _), (w2, w3)) in enumerate(zip(got[2], want_c)):
        assert np.array_equal(g2, w2) and np.array_equal(g3, w3), ("stream 2", k)


def test_refused_crop_stops_the_stream_until_track_begin():
    """A crop squarify refuses fails its frame with VNECT_E_ARG and the host path's message; the frame behind it, already in flight, and
    every later submit fail with VNECT_E_STATE until vnect_track_begin.  The refused crop here is the initial rect, whose geometry
    vnect_track_begin builds on the host.  The box stage's own refusal branch (a refused NEXT crop, trackbox.h: status, zero tables,
    `fail` for the next frame) is reached from a valid frame by joints within about 1.5 rows of a crop more than 736 pixels wide, or about
    0.67 columns of one more than 736 tall, or an extent clamped to 1 pixel at the frame's edge; no planted scene steers the joints there
    reliably, so it is covered with chosen maps (tests/test_gpu_track_maps.py::test_box_stage_refuses_a_crop) and chosen joints
    (tests/test_gpu_track_kernels.py).  This test holds the propagation from a refused INITIAL rect."""
    from vnect_amd import _native, runner
    w = _planted()
    frames, times = _video(6, H=480, W=1000, seed=1100), _times(6, 7)
    est = _est(w)
    with pytest.raises(_native.VnectError) as host_err:
        list(runner.track(est, frames, rect=[0, 10, 1000, 1], timestamps=times))
    est.close()
    est = _est(w, lanes=2)
    h = est.handle
    h.track_begin(0, 480, 1000, [0, 10, 1000, 1])
    assert h.track_box(0) == [0, 10, 1000, 1]
    h.upload_frame(0, frames[0])
    h.upload_frame(1, frames[1])
    h.submit_tracked(0, 0, *times[0])
    h.submit_tracked(0, 1, *times[1])
    with pytest.raises(_native.VnectError) as e:
        h.collect_tracked()
    assert e.value.code == _native.E_ARG and str(host_err.value) == str(e.value), (str(host_err.value), str(e.value))
    with pytest.raises(_native.VnectError) as e:
        h.collect_tracked()
    assert e.value.code == _native.E_STATE
    with pytest.raises(_native.VnectError) as e:
        h.submit_tracked(0, 0, *times[2])
    assert e.value.code == _native.E_STATE
    # a new start: the stream tracks again, and the filters were left untouched by the two refused frames
    h.track_begin(0, 480, 1000, [100, 50, 600, 400])
    got = []
    for k in range(2, 6):
        h.upload_frame(k % 4, frames[k])
        h.submit_tracked(0, k % 4, *times[k])
        got.append(h.collect_tracked()[1:])
    est.close()
    want = _host(w, frames[2:], times[2:], rect=[100, 50, 600, 400])
    _assert_same(got, want, "after restart")


def test_sharded_and_batched_handles_refuse_tracking():
    from vnect_amd import _native
    h = _native.Handle([1.0], pyramid=(0, 1))
    with pytest.raises(_native.VnectError) as e:
        h.track_begin(0, H, W)
    assert e.value.code == _native.E_ARG
    h.close()
    h = _native.Handle([1.0, 0.7], stream_batch=2)
    with pytest.raises(_native.VnectError) as e:
        h.track_begin(0, H, W)
    assert e.value.code == _native.E_ARG
    h.close()


def test_track_state_errors():
    from vnect_amd import _native
    est = _est(_planted())
    h = est.handle
    with pytest.raises(_native.VnectError) as e:
        h.submit_tracked(0, 0, 0.0, 0.0)   # the stream is not tracking
    assert e.value.code == _native.E_STATE
    with pytest.raises(_native.VnectError) as e:
        h.track_begin(0, H, W, [700, 0, 100, 100])   # the origin outside the frame (numpy would crop nothing)
    assert e.value.code == _native.E_ARG
    with pytest.raises(_native.VnectError) as e:
        h.track_box(1)
    assert e.value.code == _native.E_STATE
    h.track_begin(1, H, W, [0, 0, 0, 0])
    assert h.track_box(1) == [0, 0, W, H]
    est.close()


@pytest.mark.parametrize("source", ["pinned", "resident"])
def test_box_stage_as_its_own_launch(source, monkeypatch):
    """The box stage as a launch of its own behind post_kernel (VNECT_TRACK_BOX_LAUNCH=1, the A/B form of tools/track_rate.py) gives the
    same bits as the default form, the tail of post_kernel's joints stage."""
    monkeypatch.setenv("VNECT_TRACK_BOX_LAUNCH", "1")
    w = _planted()
    frames, times = _video(24, seed=1300), _times(24, 8)
    want = _host(w, frames, times, precision="bf16", lanes=3)
    got = _device(w, frames, times, ahead=2, source=source, precision="bf16", lanes=3)
    _assert_same(got, want, ("box launch", source))


def test_rect_past_the_frame_is_cropped_like_numpy():
    """An initial rect past the frame's far edges: runner.track crops what numpy slicing gives and reports the rect as given."""
    w = _planted()
    frames, times = _video(8, seed=1400), _times(8, 9)
    want = _host(w, frames, times, rect=[300, 200, 500, 400])
    assert want[0][2] == [300, 200, 500, 400]
    got = _device(w, frames, times, rect=[300, 200, 500, 400], ahead=1)
    _assert_same(got, want, "past the edges")


def test_python_loop_leaves_nothing_in_flight():
    """runner.track_on_device ending early -- a refused crop with the next frame already submitted (ahead=1), or the caller's `break` --
    collects what is still in flight: the estimator serves frames at once, and tracking restarts on the same stream.  The refused frames'
    timestamps do not count (vnect_infer's refusal commits none): the restart may use earlier ones."""
    from vnect_amd import _native, runner
    w = _planted()
    frames, times = _video(10, H=480, W=1000, seed=1500), _times(10, 10)
    est = _est(w)
    with pytest.raises(_native.VnectError) as e:
        list(runner.track_on_device(est, frames[5:], rect=[0, 10, 1000, 1], timestamps=times[5:], ahead=1))
    assert e.value.code == _native.E_ARG
    got = list(runner.track_on_device(est, frames[:4], rect=[100, 50, 600, 400], timestamps=times[:4], ahead=1))
    want = _host(w, frames[:4], times[:4], rect=[100, 50, 600, 400])
    _assert_same([(a, b, list(c)) for a, b, c in got], want, "restart")
    for k, _ in enumerate(runner.track_on_device(est, frames[4:], timestamps=times[4:], ahead=1)):
        if k == 1:
            break
    j2, j3 = est(frames[9], timestamp=times[9])
    assert j2.shape == (21, 2) and np.all(np.isfinite(j2))
    est.close()


def test_refused_second_video_leaves_no_rule_or_view_on_the_first():
    """runner.track_many_on_device whose second video's rect starts outside the frame: vnect_track_begin refuses it after the first
    video's stream has been given a loss rule under which every frame is lost, and a 3-D view.  The loop raises and switches both off
    again (vnect_track_begin itself resets neither): a plain loop on stream 0 afterwards is runner.track, bit for bit, with no frame
    lost and no view rendered."""
    from vnect_amd import _native, runner
    w = _planted()
    frames, times = _video(6, seed=1600), _times(6, 11)
    est = _est(w)
    with pytest.raises(_native.VnectError) as e:
        list(runner.track_many_on_device(est, [frames, frames], rects=[None, [700, 0, 100, 100]], timestamps=[times, times],
                                         lost=(1e30, 1, "hold"), view3d=True))
    assert e.value.code == _native.E_ARG
    got = list(runner.track_on_device(est, frames, timestamps=times, confidence=True))
    view = est.handle.result_view3d()
    est.close()
    assert [lost for _, _, _, _, lost in got] == [0] * 6
    assert view is None
    _assert_same([(j2, j3, list(u)) for j2, j3, u, _, _ in got], _host(w, frames, times), "after a refused setup")
