"""CPU: the person detector's rule (HOG.md).  The independent numpy statement (tests/hog_ref.py) and g++'s walk of the kernels' tiling over
vnect_amd/csrc/hog.h (libvnect_hog.so, `make hog`) agree bit for bit on level sizes, level images, votes, block descriptors (float32
bits), scores, ordered hits and grouped rects and weights; known answers derived by hand; a planted figure; every refusal; the sanitizer
sweep as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import hog_ref as R
from tests import preview_ref as P
from vnect_amd import runner

F = np.float32


def _case(pic, lay, o, det, s, what):
    buf = R.lay_from_picture(pic, lay, o) if lay["format"] != 2 else None
    ref = R.detect(pic, det, s)
    rc, got = R.walk(buf, lay, o, det, s)
    assert rc == 0, (what, rc)
    n, hw, sc, _, _ = R.sizes_of(lay, o, s)
    assert [(int(h), int(w)) for h, w in hw] == [(h, w) for h, w, _ in ref["levels"]], what
    assert np.array_equal(sc, np.array([x[2] for x in ref["levels"]])), what
    R.assert_stages_equal(got, ref, what)
    assert got["count"] == len(ref["rects"]), (what, got["count"], ref["rects"])
    assert [tuple(int(v) for v in r) for r in got["rects"]] == ref["rects"][:len(got["rects"])], what
    assert np.array_equal(got["weights"], np.array(ref["weights"][:len(got["rects"])], np.float64)), what
    return ref, got


SHAPES = [(128, 64), (129, 65), (135, 71), (136, 72), (200, 100)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % (w, h) for h, w in SHAPES])
def test_numpy_statement_and_host_walk_agree(shape):
    H, W = shape
    pic = R.textured(H, W, seed=H)
    det = R.seeded_detector(1, rho=0.05, scale=0.04)
    ref, _ = _case(pic, R.packed(H, W), 0, det, R.spec(), shape)
    assert len(ref["levels"]) == (10 if shape == (200, 100) else (1 if H < 135 else 2))
    assert 0 < len(ref["hits"]) < sum(s.size for s in ref["scores"]) or H < 136        # the threshold separates something


def test_variants_strides_scale_levels_layouts_and_codes():
    pic = R.textured(136, 72, seed=5)
    det = R.seeded_detector(2, rho=0.0, scale=0.05)
    for s in (R.spec(win_stride=(16, 8)), R.spec(scale0=1.2), R.spec(nlevels=1), R.spec(final_threshold=0.5), R.spec(hit_threshold=-0.3)):
        _case(pic, R.packed(136, 72), 0, det, s, s)
    for o in (3, 5):                                                   # the stored frame is the picture turned back
        Hs, Ws = (72, 136) if o & 1 else (136, 72)
        _case(pic, R.packed(Hs, Ws), o, det, R.spec(), ("code", o))
    for lay in P.layouts(136, 72):
        if lay["format"] == 2:
            buf = P.fresh(lay)
            pic2 = P.picture(buf, lay, 0)
            ref = R.detect(pic2, det, R.spec())
            rc, got = R.walk(buf, lay, 0, det, R.spec())
            assert rc == 0
            R.assert_stages_equal(got, ref, lay["name"])
        else:
            _case(pic, lay, 0, det, R.spec(), lay["name"])


def test_known_answers():
    lut, g, wt = R.tables()
    print("exp table: %d of 16 entries differ from numpy's (each within 1 ulp)" % R.G_DIFFER)
    assert 0 <= R.G_DIFFER <= 16                                       # recorded in HOG.md: 0; tables() has held each to 1 ulp
    # 1920 x 1080 at the defaults: 44 levels
    assert len(R.levels(1080, 1920, R.spec())) == 44
    n, hw, _, _, _ = R.sizes_of(R.packed(1080, 1920), 0, R.spec())
    assert n == 44 and tuple(hw[0]) == (1080, 1920) and hw[-1][0] >= 128 and hw[-1][1] >= 64
    assert R.sizes_of(R.packed(127, 64), 0, R.spec())[0] == 0 and R.sizes_of(R.packed(128, 63), 0, R.spec())[0] == 0
    # a constant image: every descriptor 0, every score rho
    det = R.seeded_detector(3, rho=0.375)
    pic = np.full((136, 72, 3), 77, np.uint8)
    rc, got = R.walk(R.lay_from_picture(pic, R.packed(136, 72), 0), R.packed(136, 72), 0, det, R.spec())
    assert rc == 0 and not got["votes"].any() and not got["blocks"].any()
    assert got["scores"].size and np.all(got["scores"] == F(0.375))
    # a single vertical step edge: dy = 0, dx > 0 on the two columns beside the step -> angle 0 -> pos = -0.5: bins 8 and 0, half each
    pic = np.zeros((128, 64, 3), np.uint8)
    pic[:, 32:] = 100
    v0, v1, h0 = R.votes(pic)
    on = np.zeros((128, 64), bool)
    on[:, 31:33] = True
    assert np.all(h0[on] == 8) and np.all(v0[on] == F(5.0)) and np.all(v1[on] == F(5.0))      # mag = sqrt(100) - sqrt(0) = 10
    assert not v0[~on].any() and not v1[~on].any()
    rc, got = R.walk(R.lay_from_picture(pic, R.packed(128, 64), 0), R.packed(128, 64), 0, det, R.spec())
    assert rc == 0 and np.array_equal(R.bits(got["votes"].reshape(128, 64, 2)[..., 0]), R.bits(v0))
    # ... and the block that holds the edge at its columns 7 and 8 (block bx = 3: columns 24 .. 39): by hand, every row of cell c gives
    # bins 8 and 0 the same sum, 5 * (wt[c][i][7] + wt[c][i][8]) in that order; all other bins stay 0
    d = R.blocks(v0, v1, h0)[4, 3]
    hist = np.zeros(36, F)
    for c in range(4):
        s = F(0)
        for i in range(16):
            s = s + ((F(0) + wt[c, i, 7] * F(5)) + wt[c, i, 8] * F(5))
        hist[c * 9 + 8] = hist[c * 9 + 0] = s
    s1 = F(0)
    for k in range(36):
        s1 = s1 + hist[k] * hist[k]
    u = np.minimum(hist * (F(1) / (np.sqrt(s1) + F(3.6))), F(0.2))
    s2 = F(0)
    for k in range(36):
        s2 = s2 + u[k] * u[k]
    want = u * (F(1) / (np.sqrt(s2) + F(1e-3)))
    assert np.array_equal(R.bits(d), R.bits(want)) and np.count_nonzero(want) == 8
    blk = got["blocks"].reshape(15, 7, 36)[4, 3]
    assert np.array_equal(R.bits(blk), R.bits(want))


def _group_c(rects, weights, thr):
    r = np.array(rects, np.int32).reshape(-1, 4).copy()
    w = np.array(weights, np.float64).copy()
    n = C.c_int32(-1)
    assert R.cpu_lib().hog_group_c(r.ctypes.data_as(R.i32p), w.ctypes.data_as(R.f64p), len(w), thr, C.byref(n)) == 0
    return [tuple(int(v) for v in x) for x in r[:n.value]], [float(v) for v in w[:n.value]]


def test_grouping_on_hand_made_lists():
    three = [(100, 50, 64, 128), (102, 51, 64, 128), (101, 52, 66, 130)]
    for fn in (_group_c, R.group):
        # three near-identical rects give their mean (303 / 3, 153 / 3, 194 / 3 -> 65 (64.67), 386 / 3 -> 129 (128.67)) and the largest weight
        assert fn(three, [0.5, 0.9, 0.7], 2) == ([(101, 51, 65, 129)], [0.9])
        # two are dropped at threshold 2
        assert fn(three[:2], [0.5, 0.9], 2) == ([], [])
        assert fn(three[:2] + [(400, 50, 64, 128)] * 3, [0.1, 0.2, 0.3, 0.4, 0.5], 2) == ([(400, 50, 64, 128)], [0.5])
        # a small class inside a large one is dropped: three rects well inside a class of five around them
        big = [(200, 100, 128, 256)] * 5
        small = [(230, 160, 64, 128)] * 3
        assert fn(big + small, [1.0] * 8, 2) == ([(200, 100, 128, 256)], [1.0])
        assert fn(small + big, [1.0] * 3 + [2.0] * 5, 2) == ([(200, 100, 128, 256)], [2.0])
        # ... but not a class as large as its container (n2 > max(3, n1) fails and n1 >= 3)
        assert len(fn(big + [(230, 160, 64, 128)] * 5, [1.0] * 10, 2)[0]) == 2
        # final_threshold = 0 passes hits through
        assert fn(three, [0.5, 0.9, 0.7], 0) == (three, [0.5, 0.9, 0.7])
        # a chain is one class: similarity is not transitive, the components are
        chain = [(100 + 15 * k, 50, 64, 128) for k in range(4)]
        assert not R.similar(chain[0], chain[2]) and fn(chain, [1.0] * 4, 2) == ([(122, 50, 64, 128)], [1.0])
    rng = np.random.RandomState(4)
    for _ in range(30):                                                # seeded lists: the two statements agree
        n = rng.randint(1, 40)
        base = rng.randint(0, 300, (6, 2))
        rects = [tuple(int(v) for v in (*(base[rng.randint(6)] + rng.randint(-12, 13, 2)), 64 + rng.randint(-5, 6), 128 + rng.randint(-9, 10))) for _ in range(n)]
        ws = [float(v) for v in rng.randn(n)]
        for thr in (1, 2, 3):
            assert _group_c(rects, ws, thr) == R.group(rects, ws, thr)


def test_cal_rect_and_the_whole_frame_fallback():
    def reference(rect, H, W):                                         # src/hog_box.py:48-58, as written there
        x, y, w, h = rect
        offset_w = int(0.4 / 2 * W)
        offset_h = int(0.2 / 2 * H)
        return [np.max([x - offset_w, 0]), np.max([y - offset_h, 0]), np.min([x + w + offset_w, W]) - np.max([x - offset_w, 0]),
                np.min([y + h + offset_h, H]) - np.max([y - offset_h, 0])]
    for H, W in ((360, 640), (1080, 1920), (129, 65), (7, 3)):
        for rect in ((0, 0, 64, 128), (W - 70, H - 130, 64, 128), (W // 2, H // 3, 90, 181), (5, 9, W, H)):
            assert runner.cal_rect(rect, H, W) == [int(v) for v in reference(rect, H, W)], (H, W, rect)
    assert runner.cal_rect((300, 100, 64, 128), 360, 640) == [172, 64, 320, 200]

    class Nobody:
        orientation = 0

        def detect_people(self, frame, **kw):
            return np.zeros((0, 4), np.int32), np.zeros(0)

    class Two(Nobody):
        def detect_people(self, frame, **kw):                          # equal areas: the first, as np.argmax picks
            return np.array([[10, 20, 64, 128], [300, 40, 128, 64], [200, 30, 32, 64]], np.int32), np.array([0.1, 0.9, 0.5])

    frame = np.zeros((360, 640, 3), np.uint8)
    assert runner.hog_box(Nobody(), frame) == [0, 0, 640, 360]
    assert runner.hog_box(Two(), frame) == runner.cal_rect((10, 20, 64, 128), 360, 640)
    with pytest.raises(ValueError):
        runner.lost_rule((0.5, 3, "detect"))
    assert runner.lost_rule((0.5, 3, "detect"), detect=True) == (0.5, 3, "detect")
    with pytest.raises(ValueError):
        next(runner.track_on_device(None, [frame], lost=(0.5, 3, "detect")))


def test_planted_figure():
    """A detector built from the painted figure's own descriptor.  Conditions, on the numpy statement: every window ON a figure (the level
    and position whose rectangle matches the figure's cell best) clears 0, every window that does not meet a figure's cell at all stays
    below 0, by the margins recorded here; the share of windows that hit lies strictly between 0 and one half; at least one class
    survives grouping and at least one is dropped for size.  Then the grouped rects: each contains its figure's core and there is nothing
    else -- and the walk gives the same rects."""
    pic, cells = R.planted_frame()
    det = R.planted_detector()
    s = R.spec()
    ref = R.detect(pic, det, s, keep=False)
    nwin = sum(x.size for x in ref["scores"])
    share = len(ref["hits"]) / nwin
    assert 0 < share < 0.5, share
    on_min, off_max = np.inf, -np.inf
    for n, (h, w, sc) in enumerate(ref["levels"]):
        sco = ref["scores"][n]
        ys, xs = np.mgrid[0:sco.shape[0], 0:sco.shape[1]]
        x0, y0, ww, hh = xs * 8 * sc, ys * 8 * sc, 64 * sc, 128 * sc
        dy_, dx_, df_, _ = R.PLANTED_DECOY                             # windows over the decoy's cell are neither figure nor background
        meets = (x0 < dx_ + 64 * df_) & (x0 + ww > dx_) & (y0 < dy_ + 128 * df_) & (y0 + hh > dy_)
        for (cx, cy, cw, ch) in cells:
            meets |= (x0 < cx + cw) & (x0 + ww > cx) & (y0 < cy + ch) & (y0 + hh > cy)
            fit = (np.abs(x0 - cx) <= 4 * sc) & (np.abs(y0 - cy) <= 4 * sc) & (abs(ww - cw) <= 0.05 * cw)
            if fit.any():
                on_min = min(on_min, float(sco[fit].max()))
        if (~meets).any():
            off_max = max(off_max, float(sco[~meets].max()))
    # the bound: 0.15 either side of 0 -- 3 % of |rho| (rho = -0.6 * the figure's score on itself, 8.35: -5.01) and four orders of magnitude
    # above the float32 rounding of a 3780-term sum of this size, so no summation order could move a window across 0; recorded:
    # the best-fitting window of each figure scores >= 1.4443, every background window <= -0.8215, 0.433 % of the windows hit
    print("planted: figure windows >= %.4f, background windows <= %.4f, hit share %.5f" % (on_min, off_max, share))
    assert on_min > 0.15 and off_max < -0.15, (on_min, off_max)
    raw_classes = R.group(ref["raw_rects"], ref["hit_s"], 0)
    assert len(ref["rects"]) >= 1
    sizes = []                                                         # class sizes, from the ungrouped hits
    left = list(ref["raw_rects"])
    while left:
        comp, todo = [], [left.pop(0)]
        while todo:
            a = todo.pop()
            comp.append(a)
            near = [b for b in left if R.similar(a, b)]
            for b in near:
                left.remove(b)
            todo += near
        sizes.append(len(comp))
    assert any(n <= 2 for n in sizes) and any(n > 2 for n in sizes), sizes               # one dropped for size, one survives
    assert len(ref["rects"]) == len(cells), ref["rects"]
    for cell in cells:                                                 # everything painted of each figure lies in exactly one rect
        x0, y0, x1, y1 = R.painted_extent(cell)
        inside = [r for r in ref["rects"] if r[0] <= x0 and r[1] <= y0 and r[0] + r[2] > x1 and r[1] + r[3] > y1]
        assert len(inside) == 1, (ref["rects"], cells)
    lay = R.packed(*R.PLANTED_SIZE)
    rc, got = R.walk(R.lay_from_picture(pic, lay, 0), lay, 0, det, s)
    assert rc == 0 and [tuple(int(v) for v in r) for r in got["rects"]] == ref["rects"]
    assert np.array_equal(got["weights"], np.array(ref["weights"]))
    assert np.array_equal(R.bits(got["scores"]), R.bits(np.concatenate([x.reshape(-1) for x in ref["scores"]])))
    assert raw_classes[0] == [tuple(r) for r in ref["raw_rects"]]


def test_refusals_and_the_hit_limit():
    lay = R.packed(136, 72)
    pic = R.textured(136, 72)
    buf = R.lay_from_picture(pic, lay, 0)
    det = R.seeded_detector(0)
    ok = R.spec()
    assert R.walk(buf, lay, 0, det, ok)[0] == 0
    for bad in (dict(win_stride=(4, 8)), dict(win_stride=(8, 12)), dict(win_stride=(-8, 8)), dict(scale0=1.0), dict(scale0=0.9), dict(scale0=float("nan")),
                dict(scale0=float("inf")), dict(hit_threshold=float("nan")), dict(hit_threshold=float("inf")), dict(final_threshold=float("nan")),
                dict(nlevels=65), dict(nlevels=-1), dict(max_hits=-1)):
        s = R.spec(**bad)
        n = C.c_int32(0)
        assert R.cpu_lib().hog_levels_c(0, 136, 72, *R.spec_args(s), C.byref(n), None, None, None, None) != 0, bad
        small = dict(s, max_hits=max(s["max_hits"], 1))
        out = R._outputs(np.array([20000, 200, 10]), small)
        rc = R.cpu_lib().hog_walk(*R.frame_args(buf, lay), 0, 0, *R.spec_args(s), det.ctypes.data_as(R.f32p), det.size, None,
                                  out["votes"].ctypes.data_as(R.f32p), None, None, None, None, None, None, None, None, 0, None)
        assert rc == -1 and not out["votes"].any(), bad
    big = R.packed(4098, 64)
    n = C.c_int32(0)
    assert R.cpu_lib().hog_levels_c(0, 4098, 64, *R.spec_args(ok), C.byref(n), None, None, None, None) != 0          # a picture side above 4096
    for nd in (3779, 3782, 0):                                         # the detector's length
        assert R.walk(buf, lay, 0, np.zeros(nd, F), ok)[0] == -1
    nan = det.copy()
    nan[100] = np.nan
    assert R.walk(buf, lay, 0, nan, ok)[0] == -1
    nan[100] = np.inf
    assert R.walk(buf, lay, 0, nan, ok)[0] == -1
    rc, got = R.walk(buf, lay, 0, det[:3780], ok)                      # 3780: rho 0
    assert rc == 0
    z = det.copy()
    z[3780] = 0
    assert np.array_equal(R.bits(got["scores"]), R.bits(R.walk(buf, lay, 0, z, ok)[1]["scores"]))
    # smaller than the window: zero levels, zero detections, no error
    for H, W in ((127, 64), (128, 63)):
        l2 = R.packed(H, W)
        rc, got = R.walk(np.zeros(l2["size"], np.uint8), l2, 0, det, ok)
        assert rc == 0 and got["count"] == 0 and got["hits"].shape == (0, 3)
    # more hits than max_hits: the call fails, nothing is returned
    l3 = R.packed(200, 100)
    b3 = R.lay_from_picture(R.textured(200, 100), l3, 0)
    hot = det.copy()
    hot[3780] = 1000.0
    nwin = int(R.sizes_of(l3, 0, ok)[4][2])
    rc, got = R.walk(b3, l3, 0, hot, R.spec(max_hits=nwin - 1))
    assert rc == -2 and got["count"] == -1 and not got["hits"].size and not got["rects"].size
    rc, got = R.walk(b3, l3, 0, hot, R.spec(max_hits=nwin))
    assert rc == 0 and len(got["hits"]) == nwin
    # the full count above the capacity
    rc, got = R.walk(b3, l3, 0, hot, R.spec(max_hits=nwin, final_threshold=0.5), capacity=3)
    assert rc == 0 and got["count"] == nwin and len(got["rects"]) == 3


def test_sanitizer_sweep_standalone():
    """`make hog_sweep_asan`: a program with its own main over hog.h, every frame and every workspace in an exactly sized heap block"""
    subprocess.check_call(["make", "-C", R.CSRC, "hog_sweep_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(R.LIBDIR, "hog_sweep_asan")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert " 0 mismatches" in out.stdout, out.stdout[-500:]
