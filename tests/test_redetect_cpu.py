"""CPU: re-detection inside the device tracking loop (HOG.md, "Re-detection") -- hits -> the stream's next box.  Three statements must
agree bit for bit: the numpy statement (tests/redetect_ref.py), g++'s walk of the pick kernel's phases (hog_capi.cpp: hog_pick_walk) and
the host's own hog_hit_rects + hog_group + cal_rect (hog_pick_ref) -- on hand-made hit lists, each under several orders and lane counts,
on seeded random lists, and on the planted frame's detection."""
import os
import subprocess

import numpy as np
import pytest

from tests import hog_ref as R
from tests import redetect_ref as D

H, W = 720, 1280                         # the frame the hand-made lists live on; level 0 is the picture, 64 x 128 windows
S = R.spec(max_hits=D.MAX_HITS)


def _all(hits, count=None, Hp=H, Wp=W, s=S, threshold=None, orders=3, seed=0):
    """the three statements on the list as given, reversed and shuffled, at several lane counts: one verdict"""
    hits = [tuple(int(v) for v in h) for h in hits]
    count = len(hits) if count is None else count
    want = D.pick(hits, count, Hp, Wp, s, threshold)
    rc, got = D.host(hits, count, Hp, Wp, s, 0, threshold)
    assert rc == 0 and got == want, ("host", got, want)
    rng = np.random.RandomState(seed)
    lists = [hits, hits[::-1]] + [[hits[i] for i in rng.permutation(len(hits))] for _ in range(orders)]
    for k, hs in enumerate(lists):
        for lanes in ((1, 64, 1024) if k < 2 else (1000,)):
            rc, got = D.walk(hs, count, Hp, Wp, s, 0, threshold, lanes)
            assert rc == 0 and got == want, ("walk", k, lanes, got, want)
    return want


def _cluster(y, x, n, level=0):
    """n distinct hits one window stride apart round (y, x): all similar to each other at level 0 (eps * 96 = 19.2 px)"""
    assert n <= 9
    return [(level, y + 8 * (k // 3), x + 8 * (k % 3)) for k in range(n)]


def test_no_hits_and_one_hit():
    assert _all([]) == (D.NOBODY, [0, 0, 0, 0], 0, [0, 0, W, H])
    assert _all([(0, 40, 80)])[0] == D.NOBODY                      # a class of one is dropped at threshold 2
    st, rect, n, nxt = _all([(0, 40, 80)], threshold=0)          # below 1: the hits as they are
    assert (st, rect, n) == (D.FOUND, [80, 40, 64, 128], 1) and nxt == D.cal_rect(rect, H, W)


def test_threshold_members_dropped_one_more_kept():
    assert _all(_cluster(200, 400, 2))[0] == D.NOBODY
    st, rect, n, nxt = _all(_cluster(200, 400, 3))
    assert st == D.FOUND and n == 3 and rect[2:] == [64, 128] and nxt != [0, 0, W, H]


def test_chain_joins_what_is_not_similar_itself():
    a, b, c = (0, 200, 400), (0, 200, 416), (0, 200, 432)       # 16 px apart: neighbours similar, the ends (32 px) not
    rects = [(x, y, 64, 128) for _, y, x in (a, b, c)]
    assert R.similar(rects[0], rects[1]) and R.similar(rects[1], rects[2]) and not R.similar(rects[0], rects[2])
    st, rect, n, _ = _all([a, b, c])
    assert st == D.FOUND and rect == [416, 200, 64, 128]


def test_long_chain_converges():
    chain = [(0, 96, 16 * k) for k in range(200)]                 # 200 hits at level 0, each similar to its neighbours only
    st, rect, n, nxt = _all(chain, Hp=360, Wp=3400, orders=2)
    mean_x = int(np.rint(np.float64(np.float32(sum(16 * k for k in range(200))) * (np.float32(1) / np.float32(200)))))
    assert st == D.FOUND and n == 200 and rect == [mean_x, 96, 64, 128]


def test_equal_areas_the_lower_key_wins_under_every_order():
    lo, hi = _cluster(100, 100, 4), _cluster(400, 900, 4)
    want = _all(lo)[1]
    for seed in range(4):
        st, rect, _, _ = _all(hi + lo, seed=seed)
        assert st == D.FOUND and rect == want                     # the class whose lowest member has the smaller (level, y, x)


def test_small_class_inside_a_large_one_is_dropped():
    lv = R.levels(H, W, S)
    big_level = 12                                                # scale 1.05 ** 12 = 1.80: a 115 x 230 window
    s12 = lv[big_level][2]
    big = [(big_level, 96 + 8 * (k // 3), 160 + 8 * (k % 3)) for k in range(9)]
    y0, x0 = int(130 * s12), int(190 * s12)
    small = _cluster(y0 // 8 * 8, x0 // 8 * 8, 3)
    st, rect, n, _ = _all(big + small)
    assert st == D.FOUND and n == 12 and rect[2] == int(np.rint(64 * s12))
    alone = _all(small)
    assert alone[0] == D.FOUND and alone[1][2] == 64              # on its own the small class survives: it was dropped for lying inside


def test_mean_on_a_half_rounds_to_even():
    for x3 in (410, 418):                                         # x sums 1618 and 1626: means 404.5 and 406.5, both to the even 404 / 406
        m = [(0, 200, 400), (0, 200, 408), (0, 208, 400), (0, 208, x3)]
        xs = sum(h[2] for h in m)
        assert xs % 4 == 2
        st, rect, _, _ = _all(m)
        assert st == D.FOUND and rect[0] == xs // 4 + (xs // 4) % 2 and rect[0] % 2 == 0


@pytest.mark.parametrize("y,x", [(0, 0), (0, W - 64 - 16), (H - 128 - 16, 0), (H - 128 - 16, W - 64 - 16)])
def test_cal_rect_clamped_at_each_edge(y, x):
    st, rect, _, nxt = _all(_cluster(y, x, 4))
    assert st == D.FOUND and nxt == D.cal_rect(rect, H, W)
    assert (nxt[0] == 0) != (nxt[0] + nxt[2] == W) and (nxt[1] == 0) != (nxt[1] + nxt[3] == H)


def _many(n, seed=3):
    rng = np.random.RandomState(seed)
    lv = R.levels(1080, 1920, S)
    seen, out = set(), []
    while len(out) < n:
        k = int(rng.randint(0, 20))
        h, w = lv[k][0], lv[k][1]
        cy, cx = int(rng.randint(0, (h - 128) // 8 + 1)), int(rng.randint(0, (w - 64) // 8 + 1))
        for _ in range(int(rng.randint(1, 8))):
            y = min(max(cy + int(rng.randint(-1, 2)), 0), (h - 128) // 8) * 8
            x = min(max(cx + int(rng.randint(-1, 2)), 0), (w - 64) // 8) * 8
            if (k, y, x) not in seen and len(out) < n:
                seen.add((k, y, x))
                out.append((k, y, x))
    return out


def test_the_budget_exactly_and_one_more():
    hits = _many(4097)
    full = _all(hits[:4096], Hp=1080, Wp=1920, orders=1)
    assert full[0] in (D.FOUND, D.NOBODY) and full[2] == 4096
    want = (D.OVERFLOW, [0, 0, 0, 0], 4097, [0, 0, 1920, 1080])
    assert D.pick(hits, 4097, 1080, 1920, S) == want
    assert D.host(hits[:4096], 4097, 1080, 1920, S) == (0, want)
    for lanes in (1, 1024):
        assert D.walk(hits[:4096], 4097, 1080, 1920, S, lanes=lanes) == (0, want)


@pytest.mark.parametrize("n", [5, 63, 64, 65, 300, 1023, 1025])
def test_seeded_lists_every_order_one_verdict(n):
    for thr in (0, 1, 2):
        _all(_many(n, seed=n), Hp=1080, Wp=1920, threshold=thr, orders=2, seed=n)


def test_planted_frame_gives_a_box_and_a_blank_frame_the_whole_frame():
    pic, cells = R.planted_frame()
    s = R.spec(max_hits=D.MAX_HITS)
    ref = R.detect(pic, R.planted_detector(), s, keep=False)
    assert len(ref["rects"]) == 2 and len(ref["hits"]) > 60
    st, rect, n, nxt = _all(ref["hits"], Hp=360, Wp=640, s=s, orders=2)
    rects = np.array(ref["rects"])
    assert st == D.FOUND and n == len(ref["hits"]) and tuple(rect) == tuple(rects[int(np.argmax(rects[:, 2] * rects[:, 3]))])
    assert nxt != [0, 0, 640, 360] and nxt == D.cal_rect(rect, 360, 640)
    blank = R.detect(R.background(360, 640), R.planted_detector(), s, keep=False)
    assert _all(blank["hits"], Hp=360, Wp=640, s=s)[3] == [0, 0, 640, 360]


def test_refusals():
    hits = _cluster(100, 100, 3)
    for mh in (4097, -1):
        assert D.walk(hits, 3, H, W, dict(S, max_hits=mh))[0] == -1
    assert D.walk(hits, 3, H, W, S, lanes=0)[0] == -1
    assert D.walk(hits, 3, H, W, S, orient=9)[0] == -1
    assert D.walk([(70, 0, 0), (70, 0, 8), (70, 0, 16)], 3, H, W, S)[0] == -1      # a level the table does not have
    assert D.walk(hits, 3, 0, W, S)[0] == -1
    assert D.walk(hits, 3, H, 5000, S)[0] == -1                   # a picture side above 4096


def test_sanitizer_sweep_standalone():
    """`make redetect_sweep_asan`: a program with its own main over the pick's phases, every hit list in an exactly sized heap block"""
    r = subprocess.run(["make", "-C", R.CSRC, "redetect_sweep_asan"], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("the compiler has no static sanitizer runtime here")
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([os.path.join(R.LIBDIR, "redetect_sweep_asan")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout, out.stdout[-500:]
