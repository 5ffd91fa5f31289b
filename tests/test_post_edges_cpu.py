"""CPU: the reference pinned at the edges tests/test_gpu_post_edges.py runs the device through (tests/post_edges.py) -- heat-map maxima
in the clamped border rows and columns of the x8 upsample, exact ties across the arg-max kernel's slab seams and waves, read-offs at
filtered coordinates < 4 and >= 364, and merges at scales so close to 1 that cv2's resize is a plain copy -- and the host restatements
of the device arithmetic (hostplan.h behind hp_merge / hp_merge_geo / hp_extract_2d) held to it.  The planted faults show that the
cases would notice each way the kernels could get these places wrong."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import post_edges, track_cases
from tests.test_oracle_post import np_resize

BOX, HM, NJ = 368, 46, 21
SWEEP = [[float(s)] for s in np.linspace(0.3, 1.0, 71)] + [[0.9999], [0.9893], [0.9892], [1 / 3]]


f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _p(a, t):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def hp():
    L = track_cases.hostplan()
    L.hp_merge.argtypes = [f32p, f64p, C.c_int, f64p]
    L.hp_merge_geo.argtypes = [f32p, f64p, C.c_int, f64p]
    L.hp_extract_2d.argtypes = [f64p, C.c_int, f64p]
    return L


@pytest.fixture(scope="module")
def cases():
    maps, want = post_edges.argmax_cases()
    maps.setflags(write=False), want.setflags(write=False)
    return maps, want


def _np_merge(maps, scales, near1_shift=False):
    """estimator.py:105-129 in numpy: every scale's maps resized by 1 / s, centre-cropped to 46 x 46, averaged in float64.
    near1_shift: the planted fault -- a scale whose resize is a plain copy read one cell up and to the left (clamped at 0)."""
    acc = np.zeros((4, HM, HM, NJ))
    for i, s in enumerate(scales):
        for q in range(4):
            src = np.ascontiguousarray(maps[i, :, :, NJ * q:NJ * q + NJ])
            r = np_resize(src, 1.0 / s)
            if near1_shift and s < 1 and r.shape[0] == HM:
                k = np.maximum(np.arange(HM) - 1, 0)
                r = src[k][:, k]
            mid = r.shape[0] // 2
            acc[q] += r[mid - 23:mid + 23, mid - 23:mid + 23]
    return acc / len(scales)


def _hp_merged(hp, fn, maps, scales):
    got = np.empty((HM, HM, 84), np.float64)
    s64 = np.array(scales, np.float64)
    assert getattr(hp, fn)(_p(np.ascontiguousarray(maps), f32p), _p(s64, f64p), len(scales), _p(got, f64p)) == 0, (fn, scales)
    return np.stack([got[:, :, NJ * q:NJ * q + NJ] for q in range(4)])


# ------------------------------------------------------------------------------------------ arg-max
def test_argmax_answers(hp, cases):
    """oracle.extract_2d on the 21 cases == the table derived by hand == np.argmax of a brute-force numpy upsample == hp_extract_2d
    (hostplan.h's build_up_tab applied as the arg-max kernel applies it)."""
    maps, want = cases
    heat = np.ascontiguousarray(oracle.merge_scales(maps, [1.0])[0])
    assert np.array_equal(heat, maps[0, :, :, :NJ].astype(np.float64))   # S = 1: the merged map is the input
    got = oracle.extract_2d(heat)
    assert np.array_equal(got, want), np.nonzero(np.any(got != want, axis=1))[0]
    for j in range(NJ):
        up = np_resize(np.ascontiguousarray(heat[:, :, j]), 8.0)
        assert up.shape == (BOX, BOX)
        assert tuple(want[j]) == np.unravel_index(np.argmax(up), up.shape), j
    j2 = np.empty((NJ, 2), np.float64)
    assert hp.hp_extract_2d(_p(heat, f64p), NJ, _p(j2, f64p)) == 0
    assert np.array_equal(j2, want)


# ------------------------------------------------------------------------------------------ planted faults
def _up_faulty(ch, no_far_edge=False):
    """the x8 upsample (368, 368) float64; no_far_edge: columns >= 364 blended like any other instead of taking the single tap --
    fraction kept, second tap the next element in memory (the next row's column 0; the last row's wraps to 45)"""
    up = np_resize(np.ascontiguousarray(ch), 8.0)
    if no_far_edge:
        nxt = np.concatenate([ch[1:, 0], ch[-1:, -1]])          # element 46 of each source row
        x = np.arange(364, BOX)
        f = ((x + 0.5) / 8.0 - 0.5 - 45.0)[None, :]
        rows = ch[:, 45:46] * (1.0 - f) + nxt[:, None] * f      # (46, 4): the horizontal pass of the source rows
        y = np.arange(BOX)
        fy = (y + 0.5) / 8.0 - 0.5
        sy = np.floor(fy).astype(int)
        b1 = fy - sy
        up[:, 364:] = rows[np.clip(sy, 0, 45)] * (1 - b1)[:, None] + rows[np.clip(sy + 1, 0, 45)] * b1[:, None]
    return up


def _first(up, rows=slice(None), cols=slice(None)):
    """(value, row, col) of the first maximum, in row-major order, of a sub-rectangle -- in the whole plane's coordinates"""
    sub = up[rows, cols]
    r, c = np.unravel_index(np.argmax(sub), sub.shape)
    return float(sub[r, c]), int(r) + (rows.start or 0), int(c) + (cols.start or 0)


def _argmax_fault(ch, fault):
    if fault == "last_maximum":
        up = _up_faulty(ch)
        k = up.size - 1 - int(np.argmax(up.ravel()[::-1]))
        return divmod(k, BOX)
    if fault in ("later_slab_wins", "later_wave_wins"):
        up = _up_faulty(ch)
        if fault == "later_slab_wins":      # slab k: segments 6k .. 6k+5 = rows 48k-4 .. 48k+43
            parts = [_first(up, rows=slice(max(48 * k - 4, 0), min(48 * k + 44, BOX))) for k in range(8)]
        else:                               # wave w: the threads of columns 64w .. 64w+63
            parts = [_first(up, cols=slice(64 * w, min(64 * w + 64, BOX))) for w in range(6)]
        best = parts[0]
        for p in parts[1:]:
            if p[0] >= best[0]:
                best = p
        return best[1], best[2]
    if fault == "no_far_edge_tap":
        _, r, c = _first(_up_faulty(ch, no_far_edge=True))
        return r, c
    if fault == "rows_above_the_map":       # segment 0's phases 0..3 are rows -4..-1: cell 0 once more, with lower flat indices
        up = _up_faulty(ch)
        _, r, c = _first(np.concatenate([up[:4], up]))
        return r - 4, c
    raise KeyError(fault)


@pytest.mark.parametrize("fault", ["last_maximum", "later_slab_wins", "later_wave_wins", "no_far_edge_tap", "rows_above_the_map"])
def test_planted_argmax_faults_are_caught(cases, fault):
    """numpy variants of upsample + arg-max with one defect each: every one returns another cell than the table on at least one case
    (and the clean variant returns the table on all of them: test_argmax_answers)."""
    maps, want = cases
    got = np.array([_argmax_fault(maps[0, :, :, j].astype(np.float64), fault) for j in range(NJ)], np.float64)
    wrong = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(wrong) >= 1, fault
    print(fault, "caught by cases", list(wrong))


def test_planted_near_one_shift_is_caught():
    """the merge with a copy scale read one cell off (what build_merge_tab / build_merge_geo did while they kept scale = s next to
    copy = 1): differs from the oracle on every near-1 set of scale_sets(), and on none of the others"""
    for k, scales in enumerate(post_edges.scale_sets()):
        maps = post_edges.edge_maps(600 + k, len(scales), scales)
        want = oracle.merge_scales(maps, scales)
        assert np.array_equal(_np_merge(maps, scales), want), scales
        near1 = any(s < 1 and oracle.cvround(HM / s) == HM for s in scales)
        assert np.array_equal(_np_merge(maps, scales, near1_shift=True), want) == (not near1), scales
    assert sum(any(s < 1 and oracle.cvround(HM / s) == HM for s in sc) for sc in post_edges.scale_sets()) >= 5


# ------------------------------------------------------------------------------------------ the merge
@pytest.mark.parametrize("part", ["sweep_lo", "sweep_hi", "sets"])
def test_merge_sweep(hp, part):
    """oracle.merge_scales == the numpy restatement == hp_merge (tables) == hp_merge_geo (per-entry functions, as the kernels evaluate
    it), every cell, over single scales 0.3 .. 1.0, the scales either side of the copy threshold 46 / 46.5, and scale_sets()."""
    sets = {"sweep_lo": SWEEP[:36], "sweep_hi": SWEEP[36:], "sets": post_edges.scale_sets()}[part]
    for k, scales in enumerate(sets):
        maps = post_edges.edge_maps(800 + k, len(scales))
        want = oracle.merge_scales(maps, scales)
        assert np.array_equal(_np_merge(maps, scales), want), scales
        for fn in ("hp_merge", "hp_merge_geo"):
            got = _hp_merged(hp, fn, maps, scales)
            assert np.array_equal(got, want), (fn, scales, int(np.sum(got != want)))


def test_copy_threshold():
    """cv_round(46 / s) == 46 exactly for 46 / 46.5 < s <= 1 (half to even: 46.5 -> 46): the sweep's 0.9893 is a copy, 0.9892 is not"""
    assert oracle.cvround(HM / 0.9893) == HM and oracle.cvround(HM / 0.9892) == HM + 1
    assert oracle.cvround(HM / 0.9999) == HM and oracle.cvround(HM / 0.99) == HM and oracle.cvround(HM / 0.989) == HM + 1


# ------------------------------------------------------------------------------------------ the read-off
def test_read_off_known_answers():
    """utils.hm_pt_interp_bilinear at the borders: at coordinates >= 364 x1 == x0 == 45 and the two weights cancel to an exact 0; below 4
    int() truncates toward zero and the formula extrapolates with a negative weight"""
    m = np.arange(HM * HM, dtype=np.float64).reshape(HM, HM)
    for pt in ((364, 364), (367, 367), (367, 0), (100, 367)):
        assert oracle.hm_pt_interp(m, 8.0, pt) == 0.0, pt
    assert oracle.hm_pt_interp(m, 8.0, (0, 0)) == -20.5625
    assert oracle.hm_pt_interp(m, 8.0, (3, 3)) == -2.9375
    assert oracle.hm_pt_interp(m, 8.0, (4, 4)) == 2.9375
    assert oracle.hm_pt_interp(m, 8.0, (363, 363)) == 2112.0625


def test_border_sequence_conditions():
    """What the GPU test relies on, from the reference alone: with scaler 1 and no offsets postprocess returns the filtered coordinates,
    and over border_sequence(40) they enter [364, 367], (0, 4) and (360, 364) -- both regimes of the read-off's taps and the far one's
    approach."""
    ref = oracle.OracleEstimator(scales=[1.0])
    seen = []
    for maps, (t2d, t3d) in zip(post_edges.border_sequence(40), post_edges.sequence_times(40)):
        j2, j3 = ref.postprocess(maps, t2d, t3d)
        assert np.all(np.isfinite(j2)) and np.all(np.isfinite(j3))
        seen.append(j2)
    seen = np.array(seen)
    assert np.all((seen >= 0) & (seen <= 367))
    assert np.any(seen >= 364) and np.any((seen > 0) & (seen < 4)) and np.any((seen > 360) & (seen < 364))
    assert np.all(seen[:, post_edges.PINNED] == 364.0)
    frac = seen[(seen != np.floor(seen))]
    assert frac.size > 1000       # the sweep is fractional: the filters are engaged
    # and it crosses both regime changes: some joint is on either side of 3|4 and of 363|364 on consecutive frames
    lo, hi = seen[:-1], seen[1:]
    assert np.any(((lo < 4) & (hi >= 4)) | ((lo >= 4) & (hi < 4)))
    assert np.any(((lo < 364) & (hi >= 364)) | ((lo >= 364) & (hi < 364)))


def test_edge_maps_reach_the_borders():
    """edge_maps forces 8 joints into cells {0, 1, 44, 45}, and with the set's scales its merged maps have border maxima: at least 5
    joints' raw arg-max in rows or columns < 8 or >= 360 for every set of scale_sets() and each of the three seeds the GPU test uses"""
    for k, scales in enumerate(post_edges.scale_sets()):
        for f in range(3):
            maps = post_edges.edge_maps(7000 + 10 * k + f, len(scales), scales)
            raw = oracle.extract_2d(oracle.merge_scales(maps, scales)[0])
            assert post_edges.border_joints(raw) >= 5, (scales, f, post_edges.border_joints(raw))
