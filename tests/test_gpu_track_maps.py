"""GPU: the tracked post-processing on CHOSEN maps -- the box stage's own refusal branch, and random walks of the crop over whole frames.

tests/test_gpu_track.py steers the crop through planted videos, which never send the joints outside the crop, never refuse a NEXT crop
and never crop more than a 1000 x 480 frame.  Here the conv stack's output is replaced by given maps (vnect_test_maps_override: a hook of
the TEST build of the runtime only, libvnect_hip_testhooks.so, loaded in a child process as test_warm_start_failure_injection does), so
the test chooses where the 21 heat-map maxima lie; everything else -- the crop copy and the pyramid over real frame memory, lane choice,
cross-lane waits, xfail / xseq, the ring, collect, error propagation, the timestamps' rollback -- is the product's path.  The reference
is a CPU loop (tests/track_cases.py: cpu_loop): oracle post-processing of the same maps with the crop's geometry from
oracle.gen_input_batch, the shift, runner.bbox_update, the fallback.  Everything is compared bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import track_cases as tc

pytestmark = pytest.mark.gpu

ROOT = tc.ROOT
E_ARG, E_STATE = -1, -2


def _child(tmp_path, ops, cells, seeds):
    """Runs the operations in a child process on the test build of the runtime -> (record per operation, arrays)."""
    from vnect_amd import _native
    assert os.path.exists(_native.TESTHOOKS_LIB), "run __graft_entry__.build() (make -C vnect_amd/csrc testhooks)"
    assert _native.build_info()["test_hooks"] == "0"          # the product's library has no such hook
    spec, out = str(tmp_path / "spec.npz"), str(tmp_path / "out.npz")
    np.savez(spec, ops=json.dumps(ops), cells=np.asarray(cells, np.int64), seeds=np.asarray(seeds, np.int64))
    env = {k: v for k, v in os.environ.items() if k != "VNECT_TRACK_BOX_LAUNCH"}
    env["VNECT_LIB"] = _native.TESTHOOKS_LIB
    r = subprocess.run([sys.executable, "-m", "tests.track_maps_child", spec, out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    return json.loads(str(got["record"])), got


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the box stage refuses a crop ----------------------------------------------------------------------------------------------------------
RESTART_RECT = [100, 50, 600, 400]


def _refusal_ops(source, box_launch, base):
    """One pass of the refusal scenario (the handle exists): indices of the operations the checks read."""
    R = tc.REFUSAL
    t = lambda k: list(_t(base, k))   # noqa: E731
    # the restart's timestamps lie BEFORE the refused frames' (after frame 0's): they are accepted only if those were rolled back
    tr = lambda k: list(_tr(base, k))   # noqa: E731
    ops = [["env", "VNECT_TRACK_BOX_LAUNCH", "1" if box_launch else None], ["host_refusal", R["next"][3], R["next"][2]],
           ["frame", R["H"], R["W"], 77, source], ["reset"], ["begin", R["rect"]],     # (the frame after vnect_infer: that call uses slot 0)
           ["submit", 0] + t(0), ["collect"], ["box"], ["state"],                       # 5 .. 8: frame 0
           ["submit", 0] + t(1), ["submit", 0] + t(2), ["collect"], ["collect"],       # 9 .. 12: frame 1 refused, frame 2 behind it
           ["submit", 0] + t(3), ["box"],                                             # 13, 14: later submits
           ["begin", RESTART_RECT]]                                                   # 15
    for k in range(4):
        ops += [["submit", 1 + k] + tr(k), ["collect"]]                               # 16 ..: after the restart
    ops += [["state"]]
    return ops


def _refusal_cells():
    cells, seeds = tc.walk_cells(99, 4)
    return [tc.REFUSAL["cells"]] + [c.tolist() for c in cells], [-1] + [int(s) for s in seeds]


def _t(base, k):
    return (tc.T0 + base + 0.033 * k, tc.T0 + base + 0.033 * k + 0.0005)


def _tr(base, k):
    return (tc.T0 + base + 0.004 * (k + 1), tc.T0 + base + 0.004 * (k + 1) + 0.0005)


def _refusal_reference(base):
    import oracle
    R = tc.REFUSAL
    cells, seeds = _refusal_cells()
    S = len(R["scales"])
    est = oracle.OracleEstimator(scales=R["scales"], net=None)
    first = tc.cpu_loop(R["H"], R["W"], R["rect"], [tc.hot_maps(S, cells[0])] * 2, [_t(base, 0), _t(base, 1)], R["scales"], est=est)
    assert first[0][3] == R["next"] and first[1][0] is None          # frame 0 grows the refused crop; frame 1 is refused, the filters idle
    maps = [tc.hot_maps(S, [tuple(c) for c in cells[1 + k]], np.random.default_rng(seeds[1 + k])) for k in range(4)]
    times = [_tr(base, k) for k in range(4)]
    return first[0], tc.cpu_loop(R["H"], R["W"], RESTART_RECT, maps, times, R["scales"], est=est)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("use_graph", [False, True])
def test_box_stage_refuses_a_crop(tmp_path, lanes, use_graph):
    """Joints un-mapped from the padding bands grow the next crop [1079, 46, 1, 1565] in a 1920 x 1080 (H x W) frame, which squarify
    refuses: trackbox.h's `status != SQ_OK` branch (zero tables, ts->fail = xseq + 1), track_refused on the next frame and the host's
    rollback behind it, on the GPU.  Both box forms (the tail of post_kernel, and VNECT_TRACK_BOX_LAUNCH=1) and both frame sources run on
    each handle; lanes and use_graph are the parameters."""
    R = tc.REFUSAL
    forms = [(source, box_launch) for box_launch in (0, 1) for source in ("pinned", "resident")]
    ops = [["handle", {"scales": R["scales"], "precision": "fp32", "lanes": lanes, "use_graph": use_graph}]]
    base = []
    for f, (source, box_launch) in enumerate(forms):   # (every pass 10 s of video time behind the one before it)
        base.append(len(ops))
        ops += _refusal_ops(source, box_launch, 10.0 * f)
    cells, seeds = _refusal_cells()
    rec, arr = _child(tmp_path, ops, cells, seeds)
    message = "squarify: scaled size exceeds 368"
    assert tc.squarify_bytes(R["next"][3], R["next"][2])[1] == message
    for (source, box_launch), b in zip(forms, base):
        tag = (lanes, use_graph, source, box_launch)
        frame0, after = _refusal_reference(10.0 * forms.index((source, box_launch)))
        host = rec[b + 1]["err"]
        assert host[0] == E_ARG and message in host[1], (tag, host)
        assert rec[b + 4] == {"ok": None} and rec[b + 5] == {"ok": None}, (tag, rec[b + 4], rec[b + 5])
        # frame 0 collects normally: joints and rect_used equal the CPU loop's; the next crop is the refused one
        assert rec[b + 6]["ok"]["rect"] == frame0[2], (tag, rec[b + 6])
        assert _same(arr["j2_%d" % (b + 6)], frame0[0]) and _same(arr["j3_%d" % (b + 6)], frame0[1]), tag
        assert rec[b + 7] == {"ok": R["next"]}, (tag, rec[b + 7])
        # the state behind it: SQ_SCALED, zero tables, fail == the next frame's number (frame 0 is number 1, so fail = 1 + 1)
        state = arr["state_%d" % (b + 8)]
        assert _same(state, tc.state_after(R["H"], R["W"], R["next"], 1)), (tag, state[:40].view(np.int32))
        assert state[:40].view(np.int32)[8] == tc.SQ_SCALED and not state[40:].any() and state[:40].view(np.int32)[9] == 2, tag
        # frame 1 fails with VNECT_E_ARG and the host path's message; the frame behind it and later submits with VNECT_E_STATE
        assert rec[b + 9] == {"ok": None} and rec[b + 10] == {"ok": None}, (tag, rec[b + 9], rec[b + 10])
        assert rec[b + 11]["err"] == host, (tag, rec[b + 11], host)
        assert rec[b + 12]["err"][0] == E_STATE, (tag, rec[b + 12])
        assert rec[b + 13]["err"][0] == E_STATE, (tag, rec[b + 13])
        assert rec[b + 14] == {"ok": R["next"]}, (tag, rec[b + 14])
        # after vnect_track_begin the stream tracks again: frame 0 advanced the filters, the refused frames did not, and their
        # timestamps were rolled back (the restart's are earlier than theirs)
        assert rec[b + 15] == {"ok": None}, (tag, rec[b + 15])
        for k, want in enumerate(after):
            i = b + 16 + 2 * k
            assert rec[i] == {"ok": None}, (tag, k, rec[i])
            assert rec[i + 1]["ok"]["rect"] == want[2], (tag, k, rec[i + 1], want[2])
            assert _same(arr["j2_%d" % (i + 1)], want[0]) and _same(arr["j3_%d" % (i + 1)], want[1]), (tag, k)
        # (the state behind the restart's frame k: that frame's number is k + 1 again)
        assert _same(arr["state_%d" % (b + 24)], tc.state_after(R["H"], R["W"], after[3][3], 4)), tag


# ---- random walks ------------------------------------------------------------------------------------------------------------------------
_WALK_REF = {}


def _walk_ref(H, W):
    if (H, W) not in _WALK_REF:
        _WALK_REF[(H, W)] = tc.walk_reference(H, W, tc.WALKS[(H, W)])
    return _WALK_REF[(H, W)]


@pytest.mark.parametrize("ahead", [0, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_random_walks_equal_the_cpu_loop(tmp_path, precision, ahead):
    """64-frame walks on 640 x 480, 1920 x 1080, 1080 x 1920 and 4096 x 2160 frames with random hot cells, padding bands included (joints
    outside the crop, outside the frame and negative; degenerate boxes; crops up to the whole 4K frame, which the pyramid reads without a
    fault): every frame's joints and rect_used, and every eighth frame's TrackState bytes, equal the CPU loop's."""
    n = tc.WALK_FRAMES
    ops = [["handle", {"scales": tc.BASELINE_SCALES, "precision": precision, "lanes": 3, "use_graph": "auto"}]]
    cells, seeds, plan = [], [], []
    for v, ((H, W), seed) in enumerate(tc.WALKS.items()):
        c, s = tc.walk_cells(seed, n)
        first = len(cells)
        cells += c.tolist()
        seeds += [int(x) for x in s]
        ops += [["frame", H, W, 500 + v, "pinned" if (v + ahead // 2) % 2 == 0 else "resident"], ["reset"], ["begin", None]]
        times = tc.walk_times(n)
        inflight, collects, states = 0, [], []
        for k in range(n):
            ops.append(["submit", first + k, times[k][0], times[k][1]])
            inflight += 1
            if k % 8 == 7:
                states.append((k, len(ops)))
                ops.append(["state"])
            while inflight > ahead or (k == n - 1 and inflight):
                collects.append(len(ops))
                ops.append(["collect"])
                inflight -= 1
        plan.append(((H, W), collects, states))
    rec, arr = _child(tmp_path, ops, cells, seeds)
    for (H, W), collects, states in plan:
        want = _walk_ref(H, W)
        assert len(want) == n == len(collects) and want[-1][0] is not None
        for k, i in enumerate(collects):
            tag = (precision, ahead, (H, W), k)
            assert "ok" in rec[i], (tag, rec[i])
            assert rec[i]["ok"]["rect"] == want[k][2], (tag, rec[i], want[k][2])
            assert _same(arr["j2_%d" % i], want[k][0]) and _same(arr["j3_%d" % i], want[k][1]), tag
        for k, i in states:
            assert _same(arr["state_%d" % i], tc.state_after(H, W, want[k][3], k + 1)), (precision, ahead, (H, W), k)
