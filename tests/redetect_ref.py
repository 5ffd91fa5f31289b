"""Re-detection inside the device tracking loop (HOG.md, "Re-detection"; vnect_amd/csrc/hog.h: THE RULE), stated in numpy over
tests/hog_ref.py: the hits of a lost frame -> the stream's next box.  `pick` is the statement; `walk` is g++'s walk of the pick kernel's
phases (hog_capi.cpp: hog_pick_walk), `host` the same verdict from the host's own hog_hit_rects + hog_group + cal_rect (hog_pick_ref)."""
import ctypes as C

import numpy as np

from tests import hog_ref as R

NOT_RUN, FOUND, NOBODY, OVERFLOW = 0, 1, 2, 3
MAX_HITS = 4096


def cal_rect(rect, H, W):
    """HOGBox.cal_rect (src/hog_box.py:48-58), as runner.cal_rect states it"""
    x, y, w, h = (int(v) for v in rect)
    ow, oh = int(0.4 / 2 * W), int(0.2 / 2 * H)
    x0, y0 = max(x - ow, 0), max(y - oh, 0)
    return [x0, y0, min(x + w + ow, W) - x0, min(y + h + oh, H) - y0]


def pick(hits, count, Hp, Wp, s, threshold=None):
    """(status, chosen rect, hit count, next box) of the (Hp, Wp) oriented picture whose detection left `hits` [(level, y, x)] in any order,
    `count` of them in all; s: tests/hog_ref.py's spec (max_hits is the stream's budget)"""
    threshold = int(s["final_threshold"]) if threshold is None else threshold
    whole = [0, 0, Wp, Hp]
    if count > s["max_hits"]:
        return OVERFLOW, [0, 0, 0, 0], count, whole
    lv = R.levels(Hp, Wp, s)
    hits = sorted(tuple(int(v) for v in h) for h in hits)                      # the order (level, y, x)
    raw = [(int(np.rint(x * lv[n][2])), int(np.rint(y * lv[n][2])), int(np.rint(64 * lv[n][2])), int(np.rint(128 * lv[n][2]))) for n, y, x in hits]
    rects, _ = R.group(raw, [0.0] * len(raw), threshold)
    if not rects:
        return NOBODY, [0, 0, 0, 0], count, whole
    area = np.array([r[2] * r[3] for r in rects], np.int64)
    best = rects[int(np.argmax(area))]                                          # the first of equals, in hog_group's class order
    return FOUND, [int(v) for v in best], count, cal_rect(best, Hp, Wp)


def _lib():
    L = R.cpu_lib()
    if not hasattr(L, "_redetect"):
        L.hog_pick_walk.restype = C.c_int
        L.hog_pick_walk.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, R.i32p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, R.i32p, R.i32p]
        L.hog_pick_ref.restype = C.c_int
        L.hog_pick_ref.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, R.i32p, C.c_int, C.c_int64, C.c_int, C.c_int, R.i32p, R.i32p]
        L._redetect = True
    return L


def _call(fn, hits, count, H, W, s, orient, threshold, extra):
    threshold = int(s["final_threshold"]) if threshold is None else threshold
    n = min(count, s["max_hits"])
    h3 = np.ascontiguousarray(np.asarray(hits, np.int32).reshape(-1, 3)[:n])
    out6, next4 = np.full(6, -7, np.int32), np.full(4, -7, np.int32)
    rc = fn(orient, H, W, float(s["scale0"]), int(s["nlevels"]), h3.ctypes.data_as(R.i32p), n, count, int(s["max_hits"]), threshold, *extra,
            out6.ctypes.data_as(R.i32p), next4.ctypes.data_as(R.i32p))
    return rc, (int(out6[0]), [int(v) for v in out6[1:5]], int(out6[5]), [int(v) for v in next4])


def walk(hits, count, H, W, s, orient=0, threshold=None, lanes=1024):
    """g++'s walk of hog_pick_kernel's phases with `lanes` lanes; (H, W): the frame as stored under `orient`"""
    return _call(_lib().hog_pick_walk, hits, count, H, W, s, orient, threshold, (lanes,))


def host(hits, count, H, W, s, orient=0, threshold=None):
    """hog_hit_rects + hog_group + the largest area + cal_rect, on the host"""
    return _call(_lib().hog_pick_ref, hits, count, H, W, s, orient, threshold, ())
