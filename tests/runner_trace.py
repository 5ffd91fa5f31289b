"""The device tracking loops of vnect_amd/runner.py driven by a scripted handle: every call they make on it, what they yield and what
they raise, as plain data (tests/test_runner_trace_cpu.py compares that with tests/golden/runner_traces.json, which
tests/golden/make_runner_traces.py recorded).

The loops touch the library only through ``estimator.handle`` and a few estimator members, so neither the library nor a GPU is needed:
``FakeHandle`` records each method call as (name, normalised arguments) and hands back one delivery per tracked submit (P per people
submit); ``FakeEstimator`` borrows VNectEstimator's own ``_orient``, ``_stamps``, ``_raise_like_reference`` and ``joint_parents``.
Arrays are recorded as dtype and shape, ctypes structures as their type's name and all their bytes in hex, everything else as it is.
Timestamps are always given, so a trace is deterministic."""
import collections
import ctypes as C
import json

import numpy as np

from tests.devframe_ref import FakeCuda
from vnect_amd import _native
from vnect_amd.estimator import VNectEstimator

FH, FW = 48, 64                                   # the frames' size
ADDR = 0x7F0000100000                             # where the fake device frames lie
PRODUCER = 7                                      # the stream "current" while a trace runs (_native.default_stream)
BUFFER_BYTES = 1 << 16                            # a pinned buffer of the fake handle


def norm(v):
    """an argument or a result as JSON-able data"""
    if isinstance(v, np.ndarray):
        return {"array": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, (C.Structure, C.Array)):
        return {"struct": type(v).__name__, "bytes": bytes(v).hex()}
    if isinstance(v, (tuple, list)):
        return [norm(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


class FakeHandle:
    """The part of _native.Handle the loops call.  ``fail``: {method: (n, code)} -- the method's n-th call raises VnectError(code)."""
    PLAIN = ("track_begin", "track_redetect", "track_policy", "track_view3d", "people_begin", "upload_frame", "upload_frame_nv12")
    SUBMITS = ("submit_tracked", "submit_tracked_pinned", "submit_tracked_pinned_nv12", "submit_tracked_device", "submit_tracked_device_draw",
               "submit_tracked_device_preview")
    PEOPLE_SUBMITS = ("submit_people", "submit_people_device")

    def __init__(self, people=0, pair=False, fail=None):
        self.calls = []
        self.orientation = 0
        self.people, self.pair_people = people, pair
        self.num_frame_slots = 0
        self.in_flight = collections.deque()      # the stream of every delivery still owed
        self.delivered = 0
        self._fail = dict(fail or {})
        self._seen = collections.Counter()
        self._buffers = [np.zeros(BUFFER_BYTES, np.uint8) for _ in range(2)]

    def _record(self, name, args, extra=None):
        self.calls.append([name, norm(args) + ([extra] if extra is not None else [])])
        self._seen[name] += 1
        if self._fail.get(name, (0, 0))[0] == self._seen[name]:
            raise _native.VnectError(self._fail[name][1], "scripted refusal of %s" % name)

    def __getattr__(self, name):
        if name in self.PLAIN:
            return lambda *a: self._record(name, a)
        if name in self.SUBMITS:
            def submit(stream, *a):
                extra = None
                if "pinned" in name:              # what the buffer holds when the frame is submitted: was the frame copied into it?
                    extra = {"buffer_sum": int(self._buffers[a[0]].sum(dtype=np.int64))}
                self._record(name, (stream,) + a, extra)
                self.in_flight.append(int(stream))
            return submit
        if name in self.PEOPLE_SUBMITS:
            def submit_people(n, *a):
                self._record(name, (n,) + a)
                self.in_flight.extend(range(int(n)))
            return submit_people
        raise AttributeError("the loops are not expected to call Handle.%s" % name)

    def set_orientation(self, orientation):
        self._record("set_orientation", (orientation,))
        self.orientation = int(orientation)

    def frame_buffer(self, index, H, W):
        self._record("frame_buffer", (index, H, W))
        return self._buffers[index][:H * W * 3].reshape(H, W, 3)

    def collect_tracked(self):
        assert self.in_flight, "collect_tracked with nothing in flight"
        s = self.in_flight.popleft()              # (a refused collect consumes its frame, as the library's does)
        self._record("collect_tracked", ())
        self.delivered += 1
        n = self.delivered
        return s, np.full((21, 2), float(n)), np.full((21, 3), float(n), np.float32), [n, s, FW, FH]

    def result_confidence(self):
        self._record("result_confidence", ())
        return np.full(21, 0.5), self.delivered % 2

    def result_preview(self):
        self._record("result_preview", ())
        return np.zeros((6, 8, 3), np.uint8)

    def result_view3d(self):
        self._record("result_view3d", ())
        return np.zeros((4, 5, 3), np.uint8)

    def result_redetect(self):
        self._record("result_redetect", ())
        return self.delivered % 4, [0, 0, 0, 0], 0


class FakeEstimator:
    """What the loops read of a VNectEstimator, over a FakeHandle."""
    joint_parents = VNectEstimator.joint_parents
    _check_orientation = staticmethod(VNectEstimator._check_orientation)
    _stamps = staticmethod(VNectEstimator._stamps)
    _raise_like_reference = staticmethod(VNectEstimator._raise_like_reference)
    _orient = VNectEstimator._orient

    def __init__(self, handle, lanes=1, orientation=0, scales=(1.0,)):
        self._h = self.handle = handle
        self._cfg = {"lanes": lanes}
        self._orientation = orientation
        self.scales = list(scales)
        handle.orientation = orientation          # (as VNectEstimator._open leaves it)

    @property
    def orientation(self):
        return self._orientation


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def host(n, nv12=False, H=FH, W=FW, first=0):
    shape = (H * 3 // 2, W) if nv12 else (H, W, 3)
    return [np.full(shape, first + k + 1, np.uint8) for k in range(n)]


def dev(n, nv12=False, H=FH, W=FW):
    shape = (H * 3 // 2, W) if nv12 else (H, W, 3)
    return [FakeCuda(ADDR + 0x10000 * k, shape) for k in range(n)]


def times(n, s=0):
    return [(100.0 * s + k + 1.0, 100.0 * s + k + 1.5) for k in range(n)]


# ---- one run ----------------------------------------------------------------------------------------------------------------------------------
def run(runner, name, args, kw, handle=None, est=None, take=None):
    """getattr(runner, name)(estimator, *args(handle), **kw) driven to its end (or closed after `take` results): the record of it"""
    handle = {} if handle is None else handle
    h = handle if isinstance(handle, FakeHandle) else FakeHandle(**handle)
    e = FakeEstimator(h, **(est or {}))
    args = args(h) if callable(args) else args
    del h.calls[:]                                # (what preparing the arguments called does not count)
    yielded, raised = [], None
    saved = _native.default_stream
    _native.default_stream = lambda: PRODUCER
    try:
        gen = getattr(runner, name)(e, *args, **kw)
        for res in gen:
            yielded.append(norm(res))
            if take is not None and len(yielded) == take:
                gen.close()
                break
    except Exception as err:                      # noqa: BLE001 (whatever the loop raises is the record)
        raised = [type(err).__name__, str(err)]
    finally:
        _native.default_stream = saved
    assert not h.in_flight, "the loop left %d deliveries in flight" % len(h.in_flight)
    return json.loads(json.dumps({"calls": h.calls, "yielded": yielded, "raised": raised}))


def _many(videos, **kw):
    kw.setdefault("timestamps", [times(len(v), s) for s, v in enumerate(videos)])
    handle, est, take = kw.pop("handle", None), kw.pop("est", None), kw.pop("take", None)
    return lambda runner: run(runner, "track_many_on_device", (videos,), kw, handle, est, take)


def _one(frames, **kw):
    kw.setdefault("timestamps", times(len(frames)))
    handle, est, take = kw.pop("handle", None), kw.pop("est", None), kw.pop("take", None)
    return lambda runner: run(runner, "track_on_device", (frames,), kw, handle, est, take)


def _people(frames, P, pair=False, rects=None, **kw):
    kw.setdefault("timestamps", times(len(frames)))
    handle = dict(kw.pop("handle", None) or {}, people=kw.pop("people", P), pair=pair)
    est, take = kw.pop("est", None), kw.pop("take", None)
    rects = [[2 * p, p, 30, 40] for p in range(P)] if rects is None else rects
    return lambda runner: run(runner, "track_people_on_device", (frames, rects), kw, handle, est, take)


def _buffer_views(h):
    """one video of 4 frames that already are the handle's two pinned buffers' views: nothing to copy"""
    buf = [h.frame_buffer(b, FH, FW) for b in range(2)]
    for b in range(2):
        buf[b][...] = 40 + b
    return ([[buf[k % 2] for k in range(4)]],)


LOST = (0.25, 5, "reset")
E_ARG, E_TIMESTAMP = _native.E_ARG, _native.E_TIMESTAMP


def golden_scenarios():
    """name -> f(runner module) -> record: the scenarios whose record is the parent commit's (tests/golden/runner_traces.json)"""
    s = {}
    # -- the many-video loop ----------------------------------------------------------------------------------------------------------------
    s["many/pinned_bgr_two_videos"] = _many([host(3), host(3, first=10)], ahead=1, est={"lanes": 2}, rects=[[1, 2, 30, 40], None])
    s["many/pinned_nv12_ahead0"] = _many([host(3, nv12=True)], ahead=0, pixel_format="nv12")
    s["many/pinned_reuse_wait"] = _many([host(4)], ahead=2, est={"lanes": 3})
    s["many/pinned_no_copy"] = lambda runner: run(runner, "track_many_on_device", _buffer_views, dict(timestamps=[times(4)], ahead=2),
                                                  est={"lanes": 3})
    s["many/pinned_transpose"] = _many([host(3)], transpose=True)
    s["many/resident_bgr_orientations"] = _many([host(3), host(3, first=10)], source="resident", orientation=[0, 3], est={"lanes": 2})
    s["many/resident_nv12_orientations"] = _many([host(3, nv12=True), host(3, nv12=True, first=10)], source="resident", pixel_format="nv12",
                                                 orientation=[0, 3], est={"lanes": 2})
    s["many/device_plain"] = _many([dev(3), dev(3)], source="device", est={"lanes": 2}, streams=[2, 1])
    s["many/device_draw"] = _many([dev(3)], source="device", draw=True)
    s["many/device_draw_style"] = _many([dev(3)], source="device", draw=_native.overlay_style(min_confidence=0.5))
    s["many/device_preview"] = _many([dev(3)], source="device", preview=True)
    s["many/device_preview_half_draw"] = _many([dev(3)], source="device", preview=0.5, draw=True)
    s["many/device_preview_spec_rgb"] = _many([dev(3)], source="device", preview=_native.preview_spec(0.25, "rgb"))
    s["many/device_view3d"] = _many([dev(3)], source="device", view3d=True)
    s["many/pinned_view3d_spec"] = _many([host(3)], view3d=_native.view3d_spec(size=(30, 20)))
    s["many/device_lost_redetect_confidence"] = _many([dev(3), dev(3)], source="device", lost=LOST, redetect=True, confidence=True,
                                                      est={"lanes": 2})
    s["many/device_redetect_dict"] = _many([dev(3)], source="device", lost=(0.5, 3, "hold"), redetect={"hit_threshold": 0.5})
    s["many/device_rgb"] = _many([dev(3)], source="device", pixel_format="rgb")
    s["many/device_nv12_own_orientation"] = _many([dev(3, nv12=True)], source="device", pixel_format="nv12", est={"orientation": 5})
    s["many/unequal_lengths"] = _many([host(2), host(4, first=10)], ahead=1, est={"lanes": 2})
    s["many/one_empty_video"] = _many([host(3), []], ahead=1, est={"lanes": 2}, lost=LOST, view3d=True)
    s["many/all_empty"] = _many([[]])
    s["one/device_everything"] = _one(dev(3), source="device", rect=[1, 2, 30, 40], stream=1, draw=True, preview=True, view3d=True, lost=LOST,
                                      redetect=True, confidence=True, orientation=6)
    # -- the many-video loop ending early ------------------------------------------------------------------------------------------------------
    s["many/end_second_submit_refused"] = _many([host(4)], ahead=1, est={"lanes": 2}, handle={"fail": {"submit_tracked_pinned": (2, E_ARG)}})
    s["many/end_third_device_submit_refused"] = _many([dev(4)], source="device", ahead=2, est={"lanes": 3}, lost=LOST, view3d=True,
                                                      handle={"fail": {"submit_tracked_device": (3, E_ARG)}})
    s["many/end_upload_refused"] = _many([host(3)], source="resident", orientation=2, handle={"fail": {"upload_frame": (2, E_ARG)}})
    s["many/end_submit_timestamp"] = _many([host(3)], ahead=1, est={"lanes": 2}, handle={"fail": {"submit_tracked_pinned": (2, E_TIMESTAMP)}})
    s["many/end_collect_refused"] = _many([host(4), host(4, first=10)], ahead=2, est={"lanes": 3}, lost=LOST,
                                          handle={"fail": {"collect_tracked": (2, E_ARG)}})
    s["many/end_closed_after_first"] = _many([dev(4)], source="device", ahead=2, est={"lanes": 3}, view3d=True, take=1)
    s["many/end_size_changes"] = _many([host(2) + host(2, H=FH + 2)], ahead=2, est={"lanes": 3}, lost=LOST)
    # -- the people loop -------------------------------------------------------------------------------------------------------------------------
    for P in (1, 2, 3):
        for pair in (False, True):
            s["people/device_P%d_%s" % (P, "paired" if pair else "unpaired")] = _people(dev(4), P, pair, ahead=2, est={"lanes": 4})
    s["people/lanes2_P3_paired_window1"] = _people(dev(3), 3, True, ahead=2, est={"lanes": 2})
    s["people/device_draw_preview"] = _people(dev(3), 2, True, draw=True, preview=0.5, est={"lanes": 4})
    s["people/device_preview_only"] = _people(dev(3), 2, preview=True)
    s["people/resident_nv12"] = _people(host(3, nv12=True), 2, True, source="resident", pixel_format="nv12", orientation=1, est={"lanes": 4})
    s["people/resident_bgr"] = _people(host(3), 2, source="resident", est={"lanes": 4})
    s["people/rects_with_none"] = _people(dev(2), 3, rects=[[1, 2, 30, 40], None, [5, 6, 7, 8]], people=4)
    s["people/confidence_lost_view3d"] = _people(dev(3), 2, True, confidence=True, lost=(0.5, 3, "hold"), view3d=True, est={"lanes": 4})
    s["people/no_frames"] = _people([], 2, lost=LOST, view3d=True)
    s["people/end_collect_refused_second_person"] = _people(dev(3), 3, ahead=1, est={"lanes": 8}, lost=LOST, view3d=True,
                                                            handle={"fail": {"collect_tracked": (2, E_ARG)}})
    s["people/end_submit_refused"] = _people(dev(4), 2, True, ahead=2, est={"lanes": 4}, handle={"fail": {"submit_people_device": (3, E_TIMESTAMP)}})
    s["people/end_closed_after_first"] = _people(dev(4), 2, True, ahead=2, est={"lanes": 4}, lost=LOST, take=1)
    s["people/end_size_changes"] = _people(dev(2) + dev(1, H=FH + 2), 2, True, ahead=2, est={"lanes": 4}, view3d=True)
    # -- every refusal of the options, each wrong in one way -----------------------------------------------------------------------------------
    s["refuse/many_draw_not_device"] = _many([host(2)], draw=True)
    s["refuse/many_preview_not_device"] = _many([host(2)], source="resident", preview=True)
    s["refuse/many_redetect_not_device"] = _many([host(2)], lost=LOST, redetect=True)
    s["refuse/many_redetect_without_rule"] = _many([dev(2)], source="device", redetect=True)
    s["refuse/many_unknown_source"] = _many([host(2)], source="mapped")
    s["refuse/many_lost_action"] = _many([host(2)], lost=(0.5, 3, "detect"))
    s["refuse/many_transpose_device"] = _many([dev(2)], source="device", transpose=True)
    s["refuse/many_orientation"] = _many([host(2)], orientation=8)
    s["refuse/people_draw_not_device"] = _people(host(2), 2, source="resident", draw=True)
    s["refuse/people_preview_not_device"] = _people(host(2), 2, source="resident", preview=True)
    s["refuse/people_pinned"] = _people(host(2), 2, source="pinned")
    s["refuse/people_too_many_rects"] = _people(dev(2), 3, people=2)
    s["refuse/people_no_rects"] = _people(dev(2), 0, people=2)
    return s


def split(calls):
    """(the calls up to and including the last delivery -- collect_tracked or a result_* --, the calls behind it)"""
    last = max([k for k, c in enumerate(calls) if c[0] == "collect_tracked" or c[0].startswith("result_")], default=-1)
    return calls[:last + 1], calls[last + 1:]
