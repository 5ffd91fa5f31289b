"""GPU: the loss rule of a tracked stream on CHOSEN maps (the test build of the runtime in a child process, as
tests/test_gpu_track_maps.py does): 32-frame walks whose per-joint peak levels make the confident count straddle min_joints
(tests/conf_cases.py; tests/test_confidence_cpu.py asserts the walks' conditions from the CPU loop alone).  Every frame's joints,
rect_used, confidences and lost flag, and every eighth frame's TrackState bytes, equal the CPU loop's, bit for bit -- for hold and reset,
both box forms, graph replay off and on, one and three lanes, one and three frames in flight, pinned and resident frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import conf_cases as cc
from tests import track_cases as tc

pytestmark = pytest.mark.gpu

ROOT = tc.ROOT
E_ARG, E_STATE = -1, -2


def _child(tmp_path, ops, spec):
    from vnect_amd import _native
    assert os.path.exists(_native.TESTHOOKS_LIB), "run __graft_entry__.build() (make -C vnect_amd/csrc testhooks)"
    assert _native.build_info()["test_hooks"] == "0"          # the product's library has no such hook
    spec_path, out = str(tmp_path / "spec.npz"), str(tmp_path / "out.npz")
    cells, levels, seeds = spec
    np.savez(spec_path, ops=json.dumps(ops), cells=np.asarray(cells, np.int64), levels=np.asarray(levels, np.float64), seeds=np.asarray(seeds, np.int64))
    env = {k: v for k, v in os.environ.items() if k != "VNECT_TRACK_BOX_LAUNCH"}
    env["VNECT_LIB"] = _native.TESTHOOKS_LIB
    r = subprocess.run([sys.executable, "-m", "tests.conf_maps_child", spec_path, out], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    return json.loads(str(got["record"])), got


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _walk_ops(H, W, policy, source, box_launch, ahead, base, seed):
    """One walk behind an existing handle: (ops, indices of the collects, [(frame, index of the state read)])."""
    n = cc.WALK_FRAMES
    ops = [["env", "VNECT_TRACK_BOX_LAUNCH", "1" if box_launch else None], ["frame", H, W, seed, source], ["reset"],
           ["policy", policy[0], policy[1], policy[2]], ["begin", None]]     # the rule first: it survives vnect_track_begin
    times = tc.walk_times(n, base)
    inflight, collects, states = 0, [], []
    for k in range(n):
        ops.append(["submit", k, times[k][0], times[k][1]])
        inflight += 1
        if k % 8 == 7:
            states.append((k, len(ops)))
            ops.append(["state"])
        while inflight > ahead or (k == n - 1 and inflight):
            collects.append(len(ops))
            ops.append(["collect"])
            inflight -= 1
    return ops, collects, states


def _check_walk(rec, arr, b, collects, states, frames, tag):
    for k, i in enumerate(collects):
        f = frames[k]
        assert "ok" in rec[b + i], (tag, k, rec[b + i])
        got = rec[b + i]["ok"]
        assert got["rect"] == f["used"] and got["lost"] == f["lost"], (tag, k, got, f["used"], f["lost"], f["confident"])
        assert cc.same_conf(arr["conf_%d" % (b + i)], f["conf"]), (tag, k)
        assert _same(arr["j2_%d" % (b + i)], f["j2"]) and _same(arr["j3_%d" % (b + i)], f["j3"]), (tag, k)
    for k, i in states:
        assert _same(arr["state_%d" % (b + i)], frames[k]["state"]), (tag, "state", k, arr["state_%d" % (b + i)][:40].view(np.int32),
                                                                     frames[k]["state"][:40].view(np.int32))


@pytest.mark.parametrize("lanes,use_graph,ahead", [(1, False, 0), (3, True, 2), (3, False, 2), (1, True, 0)])
@pytest.mark.parametrize("action", [cc.HOLD, cc.RESET], ids=["hold", "reset"])
def test_walks_with_a_policy_equal_the_cpu_loop(tmp_path, action, lanes, use_graph, ahead):
    """Each child: one handle, and on it both frame sizes x both box forms (the tail of post_kernel, VNECT_TRACK_BOX_LAUNCH=1) x the
    threshold on the EXACT joint's confidence and one float64 above it -- sources alternate between pinned and resident."""
    ops = [["handle", {"scales": tc.BASELINE_SCALES, "lanes": lanes, "use_graph": use_graph}]]
    plan = []
    for v, (H, W) in enumerate(cc.WALK_SIZES):
        for box_launch in (0, 1):
            for above in (False, True):
                policy, frames = cc.walk_reference(H, W, action, above)
                source = "pinned" if (v + box_launch + above) % 2 == 0 else "resident"
                plan.append(((H, W), box_launch, above, source, policy, frames))
    for (H, W) in cc.WALK_SIZES:       # (a child's spec holds one size's maps: the sizes run in two children)
        spec = cc.walk_spec(cc.WALK_SIZES[(H, W)])
        ops_hw, checks = list(ops), []
        for p, ((h_, w_), box_launch, above, source, policy, frames) in enumerate(plan):
            if (h_, w_) != (H, W):
                continue
            w_ops, collects, states = _walk_ops(H, W, policy, source, box_launch, ahead, 10.0 * p, 600 + p)
            checks.append((len(ops_hw), collects, states, frames, (action, lanes, use_graph, ahead, (H, W), box_launch, above, source)))
            ops_hw += w_ops
        rec, arr = _child(tmp_path, ops_hw, spec)
        for b, collects, states, frames, tag in checks:
            assert rec[b + 3] == {"ok": None} and rec[b + 4] == {"ok": None}, (tag, rec[b + 3], rec[b + 4])
            _check_walk(rec, arr, b, collects, states, frames, tag)


def test_policy_off_is_todays_walk_and_in_flight_is_refused(tmp_path):
    """A policy set to action 0 (after a hold policy had been set): the walk equals tests/track_cases.py's cpu_loop without any rule, lost
    is reported 0.  vnect_track_policy with a tracked frame in flight returns VNECT_E_STATE and changes nothing; bad arguments return
    VNECT_E_ARG."""
    H, W = 64, 96
    spec = cc.walk_spec(cc.WALK_SIZES[(H, W)])
    n = 12
    maps = [cc.walk_maps(spec, tc.BASELINE_SCALES, k) for k in range(n)]
    times = tc.walk_times(n)
    want = tc.cpu_loop(H, W, None, maps, times, tc.BASELINE_SCALES)
    ops = [["handle", {"scales": tc.BASELINE_SCALES, "lanes": 3, "use_graph": "auto"}], ["frame", H, W, 5, "pinned"], ["reset"],
           ["policy", 0.5, 22, 1], ["policy", 0.5, 0, 1], ["policy", 0.5, 8, 3], ["policy", float("nan"), 8, 1],    # 3 .. 6: refused
           ["policy", 1e9, 21, 1], ["policy", 1e9, 21, 0], ["begin", None]]                                     # 7, 8: hold, then off
    first = len(ops)
    for k in range(n):
        ops += [["submit", k, times[k][0], times[k][1]]]
        if k == 4:
            ops += [["policy", 1e9, 21, 2]]          # a tracked frame is in flight
        ops += [["collect"]]
    rec, arr = _child(tmp_path, ops, spec)
    for i in (3, 4, 5, 6):
        assert rec[i]["err"][0] == E_ARG, (i, rec[i])
    assert rec[7] == {"ok": None} and rec[8] == {"ok": None} and rec[9] == {"ok": None}
    i = first
    for k in range(n):
        assert rec[i] == {"ok": None}, (k, rec[i])
        i += 1
        if k == 4:
            assert rec[i]["err"][0] == E_STATE, rec[i]
            i += 1
        got = rec[i]["ok"]
        assert got["rect"] == want[k][2] and got["lost"] == 0, (k, got, want[k][2])
        assert _same(arr["j2_%d" % i], want[k][0]) and _same(arr["j3_%d" % i], want[k][1]), k
        assert cc.same_conf(arr["conf_%d" % i], cc.conf_reference(maps[k], tc.BASELINE_SCALES)), k
        i += 1


def test_reset_in_a_frame_squarify_refuses_whole(tmp_path):
    """1 x 1000 (H x W): the whole frame is a crop squarify refuses.  The stream starts on an accepted rect; the first lost frame resets
    to the whole frame, the box stage's refusal path runs, and the next frame fails with the host path's message -- the stream stops."""
    H, W = 1, 1000
    spec = cc.walk_spec(cc.WALK_SIZES[(64, 96)])
    message = tc.squarify_bytes(H, W)[1]
    assert message == "squarify: scaled size exceeds 368"
    t = tc.walk_times(4)
    ops = [["handle", {"scales": tc.BASELINE_SCALES, "lanes": 1, "use_graph": False}], ["frame", H, W, 9, "resident"], ["reset"],
           ["policy", 1e9, 1, 2], ["begin", [100, 0, 300, 1]],
           ["submit", 0, t[0][0], t[0][1]], ["collect"], ["state"], ["submit", 1, t[1][0], t[1][1]], ["collect"], ["submit", 2, t[2][0], t[2][1]]]
    rec, arr = _child(tmp_path, ops, spec)
    assert rec[3] == {"ok": None} and rec[4] == {"ok": None} and rec[5] == {"ok": None}
    assert rec[6]["ok"]["rect"] == [100, 0, 300, 1] and rec[6]["ok"]["lost"] == 1, rec[6]
    assert _same(arr["state_7"], tc.state_after(H, W, [0, 0, 0, 0], 1)) and arr["state_7"][:40].view(np.int32)[8] == tc.SQ_SCALED
    assert rec[8] == {"ok": None}
    assert rec[9]["err"][0] == E_ARG and message in rec[9]["err"][1], rec[9]
    assert rec[10]["err"][0] == E_STATE, rec[10]
