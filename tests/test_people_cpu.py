"""CPU: people mode's entry points (vnect_set_people, vnect_people_begin, vnect_submit_people, vnect_submit_people_device,
vnect_result_people; PEOPLE.md) are exported, declared with the reference lines they stand beside, bound in _native with the header's
signatures, and refuse a NULL handle; runner.people_boxes orders hand-made detection lists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from vnect_amd import _native, runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vnect_set_people", "vnect_people_begin", "vnect_submit_people", "vnect_submit_people_device", "vnect_result_people")
CTYPE = {"vnect_handle*": C.c_void_p, "int": C.c_int, "double": C.c_double, "void*": C.c_void_p, "const int32_t*": C.POINTER(C.c_int32),
         "int32_t*": C.POINTER(C.c_int32), "const vnect_device_frame*": C.POINTER(_native.DeviceFrame),
         "const vnect_overlay_style*": C.POINTER(_native.OverlayStyle), "const vnect_preview_spec*": C.POINTER(_native.PreviewSpec)}


def _header():
    return open(os.path.join(ROOT, "include", "vnect_abi.h")).read()


def test_symbols_are_exported_and_declared_with_reference_lines():
    hdr = _header()
    assert re.search(r"#define VNECT_ABI_VERSION 7\b", hdr)            # additive: the version stays
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in NEW:
        assert fn in exported, fn
        pos = hdr.index("int " + fn + "(")
        comment = hdr[hdr.rindex("/*", 0, pos):pos]
        assert re.search(r"run_estimator_ps\.py:80-109", comment), fn   # what each person's loop replaces
        assert fn in _native.SYMBOLS
    comment = hdr[hdr.rindex("/*", 0, hdr.index("int vnect_set_people(")):hdr.index("int vnect_set_people(")]
    assert "no" in comment and "counterpart" in comment and "hog_box.py:26-31" in comment
    assert "Pinned sources are not supported" in hdr


def test_native_signatures_match_the_header():
    hdr = _header()
    for fn in NEW:
        proto = re.search(r"int " + fn + r"\(([^;]*)\);", hdr).group(1)
        params = [" ".join(p.split()) for p in proto.split(",")]
        types = [re.sub(r"\s*\w+$", "", p).replace(" *", "*") for p in params]     # drop the parameter's name
        res, args = _native.SYMBOLS[fn]
        assert res is C.c_int and len(args) == len(types), (fn, types)
        for t, a in zip(types, args):
            assert CTYPE[t] is a or CTYPE[t] == a, (fn, t, a)


def test_null_handle_and_out_of_range_n_are_refused():
    L = _native.lib()
    r = (C.c_int32 * 16)()
    u = C.c_int32()
    for n in (2, 0, 5, -1):
        assert L.vnect_set_people(None, n, 1) == _native.E_ARG
        assert L.vnect_people_begin(None, n, 96, 128, r) == _native.E_ARG
        assert L.vnect_submit_people(None, n, 0, 1.0, 1.0) == _native.E_ARG
        assert L.vnect_submit_people_device(None, n, None, None, 1.0, 1.0, None, None) == _native.E_ARG
    assert L.vnect_result_people(None, C.byref(u), C.byref(u)) == _native.E_ARG


class _Detections:
    """an estimator that 'finds' a hand-made list"""
    orientation = 0

    def __init__(self, rects):
        self.rects = np.asarray(rects, np.int32).reshape(-1, 4)

    def detect_people(self, frame, **kw):
        self.kw = kw
        return self.rects, np.ones(len(self.rects))


def test_people_boxes_orders_pads_and_grows():
    H, W = 200, 300
    frame = np.zeros((H, W, 3), np.uint8)
    big, mid, small = [10, 20, 60, 120], [150, 40, 50, 100], [200, 10, 30, 60]
    # ordering: area descending, whatever the detector's order
    for order in ([small, big, mid], [mid, small, big], [big, mid, small]):
        got = runner.people_boxes(_Detections(order), frame, 3)
        assert got == [runner.cal_rect(r, H, W) for r in (big, mid, small)], (order, got)
    # ties: equal areas by (y, x) -- the upper one first, then the left one
    a, b, c = [100, 50, 40, 80], [20, 50, 80, 40], [60, 30, 32, 100]      # all 3200 pixels
    got = runner.people_boxes(_Detections([a, b, c]), frame, 3)
    assert got == [runner.cal_rect(r, H, W) for r in (c, b, a)], got
    # more detections than people: the largest; fewer: padded with the whole frame; none: everybody gets the whole frame
    assert runner.people_boxes(_Detections([small, big, mid]), frame, 2) == [runner.cal_rect(big, H, W), runner.cal_rect(mid, H, W)]
    assert runner.people_boxes(_Detections([mid]), frame, 3) == [runner.cal_rect(mid, H, W), [0, 0, W, H], [0, 0, W, H]]
    assert runner.people_boxes(_Detections([]), frame, 4) == [[0, 0, W, H]] * 4
    # deterministic, and the spec goes to the detector
    est = _Detections([a, b, c])
    assert runner.people_boxes(est, frame, 2, hit_threshold=0.5) == runner.people_boxes(est, frame, 2, hit_threshold=0.5)
    assert est.kw["hit_threshold"] == 0.5
    # a quarter-turned video: the boxes are in the picture's coordinates (W x H becomes H x W)
    assert runner.people_boxes(_Detections([]), frame, 1, orientation=1) == [[0, 0, H, W]]


def test_python_layer_refuses_what_people_mode_does_not_do():
    class _H:
        people = 2
    class _E:
        handle = _H()
    frames = [np.zeros((6, 4, 3), np.uint8)]
    with pytest.raises(ValueError, match="pinned"):
        next(runner.track_people_on_device(_E(), frames, [None, None], source="pinned"))
    with pytest.raises(ValueError, match="preview"):
        next(runner.track_people_on_device(_E(), frames, [None, None], source="resident", preview=True))
    with pytest.raises(ValueError, match="source='device'"):
        next(runner.track_people_on_device(_E(), frames, [None, None], source="resident", draw=True))
    with pytest.raises(ValueError, match="people"):
        next(runner.track_people_on_device(_E(), frames, [None] * 3))
