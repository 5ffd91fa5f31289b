"""CPU: the device tracking loops of vnect_amd/runner.py, call by call, on a scripted handle (tests/runner_trace.py).

tests/golden/runner_traces.json holds what the loops did before they were built from one in-flight window: every Handle call with its
arguments, what was yielded, what was raised.  The loops must still make the same calls in the same order up to and including the last
delivery (collect_tracked or a result_*), the same calls in any order behind it (the teardown's off-calls, with nothing in flight), and
yield and raise the same.  The three scenarios at the end are the deliberate differences and state their expectation by hand."""
import collections
import json
import os

import pytest

from tests import runner_trace as rt
from vnect_amd import _native, runner

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_traces.json")
SCENARIOS = rt.golden_scenarios()
_TRACES = {}


def _golden():
    if not _TRACES:
        with open(GOLDEN) as fh:
            _TRACES.update(json.load(fh))
    return _TRACES


def _bag(calls):
    return collections.Counter(json.dumps(c, sort_keys=True) for c in calls)


def test_golden_file_holds_every_scenario():
    assert sorted(_golden()) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_loop_makes_the_recorded_calls(name):
    want, got = _golden()[name], SCENARIOS[name](runner)
    assert got["raised"] == want["raised"]
    assert got["yielded"] == want["yielded"]
    (got_head, got_tail), (want_head, want_tail) = rt.split(got["calls"]), rt.split(want["calls"])
    assert got_head == want_head
    assert _bag(got_tail) == _bag(want_tail)


def test_scenarios_reach_what_they_are_named_for():
    """the recorded traces themselves: the branches the scenarios are there for were taken"""
    g = _golden()
    names = lambda key: [c[0] for c in g[key]["calls"]]
    # the buffer-reuse wait: frame 2 waits for frame 0's collect before it is copied; frames that are the buffers' views do not
    assert names("many/pinned_reuse_wait")[:6].count("collect_tracked") == 1 and names("many/pinned_no_copy")[:6].count("collect_tracked") == 0
    assert [c[1][-1]["buffer_sum"] for c in g["many/pinned_reuse_wait"]["calls"] if c[0] == "submit_tracked_pinned"] == [
        (k + 1) * rt.FH * rt.FW * 3 for k in range(4)]
    # the default style of a preview without draw= (draw_frame 0) against draw=True (draw_frame 1); people mode passes no style
    spec = lambda key, name: [c[1] for c in g[key]["calls"] if c[0] == name][0]
    plain, drawn = spec("many/device_preview", "submit_tracked_device_preview"), spec("many/device_preview_half_draw", "submit_tracked_device_preview")
    assert plain[5]["struct"] == drawn[5]["struct"] == "OverlayStyle" and plain[6]["bytes"] != drawn[6]["bytes"]
    assert spec("people/device_preview_only", "submit_people_device")[5] is None
    assert spec("people/device_draw_preview", "submit_people_device")[5]["struct"] == "OverlayStyle"
    # the windows: three frames ahead for one person on four lanes, one for three paired persons on two
    assert names("people/device_P1_unpaired")[:5] == ["people_begin"] + ["submit_people_device"] * 3 + ["collect_tracked"]
    lone = names("people/lanes2_P3_paired_window1")
    assert lone.index("collect_tracked") < [k for k, n in enumerate(lone) if n == "submit_people_device"][1]
    # early endings: results first, then the error; a refused collect drops the frame's other persons
    assert g["many/end_second_submit_refused"]["raised"][0] == "VnectError" and len(g["many/end_second_submit_refused"]["yielded"]) == 1
    assert g["many/end_submit_timestamp"]["raised"] == ["ZeroDivisionError", "float division by zero"]
    assert g["many/end_size_changes"]["raised"] == ["ValueError", "frames of one video must have one size"]
    assert g["many/end_closed_after_first"]["raised"] is None and len(g["many/end_closed_after_first"]["yielded"]) == 1
    refused = g["people/end_collect_refused_second_person"]
    assert refused["raised"][0] == "VnectError" and names("people/end_collect_refused_second_person").count("collect_tracked") == 6
    for key in g:
        if key.startswith("refuse/"):
            assert g[key]["raised"][0] == "ValueError" and not g[key]["calls"] and not g[key]["yielded"], key


# ---- the deliberate differences: expectations written by hand ----------------------------------------------------------------------------
def _offs(calls):
    """the switch-off calls of a trace: (name, stream)"""
    off = {"track_policy": lambda a: a[3] == "off", "track_view3d": lambda a: a[1] is None, "track_redetect": lambda a: a[2] is False}
    return sorted((n, a[0]) for n, a in calls if n in off and off[n](a))


@pytest.mark.parametrize("refused", ["track_begin", "track_redetect", "track_policy", "track_view3d"])
def test_refused_setup_of_the_second_video_leaves_nothing_switched_on(refused):
    """lost=, view3d= and redetect= on two videos under orientation 3, the second video's setup refused: the library's error comes out,
    and behind it stream 5 (the first video's) has its rule, view and re-detection switched off exactly once each, stream 6 only what it
    had been given, and the handle is back under the estimator's own orientation."""
    got = rt.run(runner, "track_many_on_device", ([rt.dev(3), rt.dev(3)],),
                 dict(timestamps=[rt.times(3), rt.times(3, 1)], source="device", streams=[5, 6], lost=rt.LOST, view3d=True, redetect=True,
                      orientation=3, rects=[None, [70, 0, 10, 10]]),
                 handle={"fail": {refused: (2, _native.E_ARG)}}, est={"orientation": 1})
    assert got["raised"] == ["VnectError", "libvnect_hip: scripted refusal of %s (code -1)" % refused] and not got["yielded"]
    calls = got["calls"]
    names = [n for n, _ in calls]
    assert not any(n.startswith("submit") or n == "collect_tracked" for n in names)
    order = ["track_begin", "track_redetect", "track_policy", "track_view3d"]             # (the order the setup switches things on in)
    second = [(n, 6) for n in ("track_redetect", "track_policy", "track_view3d") if order.index(n) < order.index(refused)]
    assert _offs(calls) == sorted([("track_policy", 5), ("track_redetect", 5), ("track_view3d", 5)] + second)
    assert [a for n, a in calls if n == "set_orientation"] == [[3], [1]]


def test_people_refused_view_off_still_switches_the_rule_off():
    got = rt.run(runner, "track_people_on_device", (rt.dev(2), [None, None]),
                 dict(timestamps=rt.times(2), lost=rt.LOST, view3d=True), handle={"people": 2, "fail": {"track_view3d": (3, _native.E_ARG)}})
    assert got["raised"] is None and len(got["yielded"]) == 2
    assert _offs(got["calls"]) == [("track_policy", 0), ("track_policy", 1), ("track_view3d", 0), ("track_view3d", 1)]
