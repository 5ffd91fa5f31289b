"""GPU (MI355X), through Handle.postprocess: post.hip -- merged_cell, argmax_body / heat_argmax_kernel, joints_kernel, post_kernel with
joints_stage_wide -- at map borders, slab and wave seams, and near-1 scales (tests/post_edges.py; tests/test_post_edges_cpu.py pins the
reference on the same cases).  Every comparison is bit for bit: the stage is exact arithmetic (gpu_common.py).  No test runs the conv
stack."""
import numpy as np
import pytest

import oracle
from tests import post_edges
from tests.gpu_common import BASELINE_SCALES, T0, _handle, _log

pytestmark = pytest.mark.gpu

_LOG = {}


def _record(key, value):
    _LOG[key] = value
    _log("post_edges.json", _LOG)


def _pairs(a):
    return [[int(r), int(c)] for r, c in np.asarray(a)]


@pytest.mark.parametrize("two_launches", [False, True])
def test_argmax_edges(weights, monkeypatch, two_launches):
    """The 21 known-answer cases on the first frame after reset_filters() of a [1.0] handle (the filters return their input: the joints are
    the raw arg-max), as one launch (post_kernel) and as two (heat_argmax_kernel + joints_kernel).  A joint at a coordinate >= 364 reads off
    an exact 0 (x1 == x0 == 45: the two weights cancel), so its 3-D row is minus the root's read-off."""
    if two_launches:
        monkeypatch.setenv("VNECT_NO_POST_MERGE", "1")
    maps, want = post_edges.argmax_cases()
    h = _handle([1.0], weights)
    ref = oracle.OracleEstimator(scales=[1.0])
    h.postprocess(post_edges.border_sequence(1)[0], T0 - 1, T0 - 1)   # some state for reset_filters() to clear
    h.reset_filters()
    j2, j3 = h.postprocess(maps, T0, T0)
    h.close()
    _record("argmax_%s" % ("two_launches" if two_launches else "merged"), {"expected": _pairs(want), "returned": _pairs(j2)})
    r2, r3 = ref.postprocess(maps, T0, T0)
    assert j2.dtype == np.float64 and j3.dtype == np.float32
    assert np.array_equal(j2, want), np.nonzero(np.any(j2 != want, axis=1))[0]
    assert np.array_equal(j2, r2) and np.array_equal(j3, r3)
    root = np.array([np.float32(oracle.hm_pt_interp(maps[0, :, :, 21 * (k + 1) + 14], 8.0, want[14]) * 100) for k in range(3)], np.float32)
    assert np.all(root != 0)
    far = np.nonzero(np.any(want >= 364, axis=1))[0]
    assert len(far) == 5     # (364,364), (0,364), (364,0), (364,163), (163,364)
    for j in far:
        assert np.array_equal(j3[j], -root), j


def _tiled(m1, S):
    """one scale's maps as S scales' with amplitudes that differ per scale"""
    return np.concatenate([m1 * np.float32(1.0 + 0.13 * i) for i in range(S)]).astype(np.float32)


@pytest.mark.parametrize("promo", [0, 1])
@pytest.mark.parametrize("scales", [[1.0], BASELINE_SCALES], ids=["one", "baseline"])
def test_border_sequence(weights, scales, promo):
    """40 frames whose peaks jump between opposite borders, irregular frame times, a t2d of 0.0 in the middle, un-mapped with the
    scaler and offsets of a 538 x 368 frame: the filtered coordinates sweep [0, 364] fractionally, the read-offs run in both border regimes
    (< 4: extrapolation with a negative weight; >= 364: the exact 0) -- equal to the oracle on every frame, in both numpy promotions."""
    h = _handle(scales, weights, numpy_promotion=promo)
    ref = oracle.OracleEstimator(scales=scales, nep50=bool(promo))
    scaler, ox, oy = 368 / 538, 58, 0
    seen = []
    for k, (m1, (t2d, t3d)) in enumerate(zip(post_edges.border_sequence(40), post_edges.sequence_times(40, T0))):
        maps = _tiled(m1, len(scales))
        a2, a3 = h.postprocess(maps, t2d, t3d, scaler, ox, oy)
        r2, r3 = ref.postprocess(maps, t2d, t3d, scaler, ox, oy)
        assert np.array_equal(a2, r2), k
        assert np.array_equal(a3, r3), k
        seen.append(r2 * scaler + np.array([oy, ox]))      # back to (about) the filtered coordinates
    h.close()
    seen = np.array(seen)
    assert np.any(seen >= 363.999) and np.any((seen > 0.001) & (seen < 3.999)) and np.any((seen > 360.001) & (seen < 363.999))


def _run_set(h, scales, seed, frames=3, need_border=True):
    """`frames` frames of edge_maps on handle h against a fresh oracle estimator; returns the border joints of each frame's raw arg-max"""
    ref = oracle.OracleEstimator(scales=scales)
    border = []
    for f in range(frames):
        maps = post_edges.edge_maps(seed + f, len(scales), scales)
        t = T0 + f / 30 + 0.002 * f * f
        a2, a3 = h.postprocess(maps, t, t + 0.0006, 368 / 538, 58, 0)
        r2, r3 = ref.postprocess(maps, t, t + 0.0006, 368 / 538, 58, 0)
        assert np.array_equal(a2, r2), (scales, f, np.nonzero(np.any(a2 != r2, axis=1))[0])
        assert np.array_equal(a3, r3), (scales, f)
        border.append(post_edges.border_joints(oracle.extract_2d(oracle.merge_scales(maps, scales)[0])))
    assert min(border) >= 5 or not need_border, (scales, border)     # not vacuously interior (tests/test_post_edges_cpu.py holds the same from the reference alone)
    return border


SETS = post_edges.scale_sets()


@pytest.mark.parametrize("k", range(len(SETS)), ids=["-".join("%g" % s for s in sc) for sc in SETS])
def test_scale_sets(weights, k):
    """Every set of scale_sets() -- near-1 scales whose resize is a plain copy (alone, first, last, behind a real resize), equal scales,
    5 to 8 scales through post_kernel<VNECT_MAX_S> -- on three frames of border-heavy maps: equal to the oracle."""
    scales = SETS[k]
    h = _handle(scales, weights)
    border = _run_set(h, scales, 7000 + 10 * k)
    h.close()
    _record("scale_set_%d" % k, {"scales": scales, "border_joints": border})


@pytest.mark.parametrize("k", [0, len(SETS) - 1], ids=["0.99", "eight"])
def test_scale_sets_two_launches(weights, monkeypatch, k):
    """[0.99] and the 8-scale set through heat_argmax_kernel + joints_kernel<VNECT_MAX_S>"""
    monkeypatch.setenv("VNECT_NO_POST_MERGE", "1")
    scales = SETS[k]
    h = _handle(scales, weights)
    border = _run_set(h, scales, 7000 + 10 * k)
    h.close()
    _record("scale_set_%d_two_launches" % k, {"scales": scales, "border_joints": border})


def test_near_one_scales_by_reassignment(weights):
    """[1.0, 0.9999] given to a live handle made with other scales (set_scales re-plans the merge geometry): as a fresh oracle"""
    scales = SETS[1]
    assert scales == [1.0, 0.9999]
    h = _handle(BASELINE_SCALES[:2], weights)
    _run_set(h, BASELINE_SCALES[:2], 7500, frames=1, need_border=False)
    h.set_scales(scales)
    h.reset_filters()
    border = _run_set(h, scales, 7000 + 10 * 1)
    h.close()
    _record("scale_set_1_reassigned", {"scales": scales, "border_joints": border})
