"""No GPU: the matrix of tests/test_gpu_stream_order.py held against include/vnect_abi.h, and the premises its GPU tests rely on.

Every function of the ABI that takes a producer stream -- a `void* producer_stream` parameter, or a `void*` parameter its comment calls a
producer_stream (vnect_draw_device's `stream`) -- must be an entry point of MATRIX, the list the stalled-producer test is parametrised
from: one added later without an ordering test fails here.  And what a stalled test proves rests on `old` and `new` giving different
references, and on the moving video's box moving: both are asserted here on the host references alone (tests/stall.py's frames)."""
import os
import re

import numpy as np

from tests import stall as S
from tests import test_gpu_stream_order as G

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vnect_abi.h")


def producer_entry_points(text):
    """the functions of the header `text` that take a producer stream"""
    comments = re.findall(r"/\*.*?\*/", text, flags=re.S)
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(vnect_\w+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S)}
    out = {name for name, args in decls.items() if re.search(r"\bvoid\s*\*\s*producer_stream\b", args)}
    for c in comments:                           # "vnect_x: ... `stream` is a producer_stream": the parameter `stream` of vnect_x
        for m in re.finditer(r"`(\w+)` is a producer_stream", c):
            named = re.findall(r"\b(vnect_\w+):", c[:m.start()])
            assert named, "a parameter is called a producer_stream in a comment that names no function"
            assert named[-1] in decls and re.search(r"\bvoid\s*\*\s*%s\b" % m.group(1), decls[named[-1]]), (named[-1], m.group(1))
            out.add(named[-1])
    return out, decls


def test_every_producer_entry_point_is_a_row_of_the_matrix():
    with open(HEADER) as fh:
        text = fh.read()
    want, decls = producer_entry_points(text)
    assert "vnect_draw_device" in want and "vnect_upload_frame_device" in want and len(want) >= 10, sorted(want)
    rows = {entry for entry, _ in G.MATRIX}
    assert want - rows == set(), "no stalled-producer test for %s: add a row to MATRIX of tests/test_gpu_stream_order.py" % sorted(want - rows)
    assert rows - want == set(), "MATRIX names %s, which take no producer stream" % sorted(rows - want)
    # every void* of a device-frame entry point other than the handle, the frame's memory and an output is one of the two kinds above
    for name, args in decls.items():
        if "vnect_device_frame" in args and re.search(r"\bvoid\s*\*\s*(\w*stream\w*)", args):
            assert name in want, name


def test_the_parser_sees_an_entry_point_added_later():
    text = "/* vnect_new: `st` is a producer_stream */\nint vnect_new(vnect_handle* h, void* st);\nint vnect_other(vnect_handle* h, void* producer_stream,\n int k);\nint vnect_none(void* out);"
    assert producer_entry_points(text)[0] == {"vnect_new", "vnect_other"}


def test_every_row_has_its_case_and_every_case_its_row():
    """deleting a row of MATRIX leaves a case without one (or an entry point without a test): both fail here"""
    names = [name for _, name in G.MATRIX]
    assert len(set(names)) == len(names)
    assert sorted(G.CASES) == sorted(names)
    for form in S.FORMS:                         # the source forms, on the upload and on the tracked submit
        assert ("vnect_upload_frame_device", "upload-" + form) in G.MATRIX and ("vnect_submit_tracked_device", "tracked-" + form) in G.MATRIX
    with open(HEADER) as fh:
        for entry in producer_entry_points(fh.read())[0]:
            assert any(e == entry for e, _ in G.MATRIX), entry


# ---- the premises ----------------------------------------------------------------------------------------------------------------------------
def _box(blobs):
    from vnect_amd import runner
    return runner.bbox_update(S.centres(blobs), S.W, S.H)


def test_old_and_new_differ_where_it_matters_pose():
    """the joints: the planted answer (joint j on the blob of colour j % 3) of `old` and `new` lies 80 pixels apart, far more than the
    'cell or two' (8 to 16 pixels) the answer is known to through a crop; both sets of blobs lie inside the first crop; and every source
    form shows the library two different pictures"""
    old, new = S.pose_pair()
    d = np.abs(S.centres(S.OLD_BLOBS) - S.centres(S.NEW_BLOBS)).max(axis=1)
    assert d.min() > 40.0
    x, y, w, h = S.RECT0
    for blobs in (S.OLD_BLOBS, S.NEW_BLOBS):
        for r, c, k, amp in blobs:
            assert y + 8 <= r < y + h - 8 and x + 8 <= c < x + w - 8
            assert (old if blobs is S.OLD_BLOBS else new)[int(round(r)), int(round(c)), k] >= 250        # the blob is there
    assert old[int(S.NEW_BLOBS[0][0]), int(S.NEW_BLOBS[0][1]), 0] < 60 and new[int(S.OLD_BLOBS[0][0]), int(S.OLD_BLOBS[0][1]), 0] < 60
    for form in S.FORMS:
        src = S.Source(form, old, new)
        a, b = src.seen(0), src.seen(1)
        assert a.shape == b.shape == (S.H, S.W, 3) and (a != b).mean() > 0.5, form
        bo, bn = (src.bytes[0], src.bytes[1]) if isinstance(src.bytes[0], tuple) else ((src.bytes[0],), (src.bytes[1],))
        assert all(p.size == q.size and not np.array_equal(p, q) for p, q in zip(bo, bn)), form
        if form == "orient-3":
            from vnect_amd import runner
            assert np.array_equal(runner.orient_view(src.host[1], 3), new)


def test_old_and_new_differ_where_it_matters_overlay_and_preview():
    from vnect_amd import render
    old, new = S.pose_pair()
    j2, rect = S.skeleton()
    a, b = S.drawn(old, j2, rect), S.drawn(new, j2, rect)
    assert not np.array_equal(a, b)
    assert not np.array_equal(b, new.reshape(-1))                    # an overlay wiped out by the producer's copy is not the reference
    assert (a != old.reshape(-1)).sum() > 100 and (b != new.reshape(-1)).sum() > 100      # something is drawn ...
    assert ((a == old.reshape(-1)) & (old != new).reshape(-1)).sum() > 1000                # ... and most of the frame is left alone
    pa, pb = (render.preview_exact(f, j2, S.overlay_ref.PARENTS, rect, factor=0.5) for f in (old, new))
    assert pa.shape == pb.shape == (S.H // 2, S.W // 2, 3) and (pa != pb).mean() > 0.5


def test_old_and_new_differ_where_it_matters_detector():
    """`old` holds nobody, `new` one figure whose detection's box (cal_rect) is not the whole frame -- the box `old` hands on"""
    from tests import hog_ref
    from vnect_amd import runner
    old, new = S.hog_pair()
    det, spec = hog_ref.planted_detector(), hog_ref.spec()
    a, b = hog_ref.detect(old, det, spec, keep=False), hog_ref.detect(new, det, spec, keep=False)
    assert len(a["hits"]) == 0 and a["rects"] == []
    assert len(b["hits"]) >= 3 and len(b["rects"]) == 1
    box = runner.cal_rect(b["rects"][0], S.HOG_H, S.HOG_W)
    assert box != [0, 0, S.HOG_W, S.HOG_H]
    x, y, w, h = b["rects"][0]
    assert abs(x - S.HOG_CELL[0]) <= 8 and abs(y - S.HOG_CELL[1]) <= 8 and w >= 64 and h >= 128


def test_the_moving_videos_box_moves():
    """the box grown from frame k's known joints has its middle at least 5 pixels from frame k - 1's, and holds frame k + 1's blobs: a crop taken
    with the stale box is another crop of a person who is still in it"""
    n = 9
    boxes = [_box(S.moving_blobs(k)) for k in range(n)]
    for k in range(1, n):
        mid = [b[0] + b[2] / 2.0 for b in (boxes[k - 1], boxes[k])]
        assert abs(mid[1] - mid[0]) >= 5 and boxes[k] != boxes[k - 1], (k, boxes[k - 1], boxes[k])
        x, y, w, h = boxes[k - 1]
        for r, c, _, _ in S.moving_blobs(k):
            assert y <= r < y + h and x <= c < x + w and 0 <= r < S.H and 0 <= c < S.W, (k, r, c, boxes[k - 1])
    video = S.moving_video(n)
    assert all((video[k] != video[k - 1]).mean() > 0.5 for k in range(1, n))
    x, y, w, h = 2, 20, 90, 80                                       # the first rect of the GPU tests holds frame 0's blobs
    assert all(y + 8 <= r < y + h - 8 and x + 8 <= c < x + w - 8 for r, c, _, _ in S.moving_blobs(0))


def test_the_people_videos_frames_differ():
    video, rects = S.people_video()
    assert len(video) >= 5 and len(rects) == 4 and video[0].shape == (96, 128, 3)
    for a, b in ((4, 0), (0, 1), (1, 2)):                            # the (old, new) pairs of the people cases
        assert (video[a] != video[b]).mean() > 0.5
    x, y, w, h = rects[1]                                            # person 1's first rect holds person 0's: the drawing scene
    x0, y0, w0, h0 = rects[0]
    assert x <= x0 + w0 // 2 < x + w and y <= y0 + h0 // 2 < y + h
