"""GPU (MI355X), product library: the per-joint confidence (CONFIDENCE.md) on every path that runs the joints stage.

Through Handle.postprocess the device's confidences must equal tests/conf_cases.py's conf_reference -- the maximum of the oracle's x8
upsample of the oracle's merged heat-map -- bit for bit, at S = 1, 3, 4 and 8, in the merged launch and in the two-launch form; through
the estimator they must equal conf_reference of the device's own maps, with frames in flight each collect its own frame's, and each
stream of a two-stream batch its single run's.  No tolerance anywhere: the stage is exact arithmetic."""
import ctypes as C

import numpy as np
import pytest

from tests import conf_cases as cc
from tests.gpu_common import BASELINE_SCALES, T0, _handle

pytestmark = pytest.mark.gpu

_SETS = None


def _sets():
    """the chosen map sets with their reference confidences, computed once"""
    global _SETS
    if _SETS is None:
        _SETS = [(name, maps, scales, cc.conf_reference(maps, scales)) for name, maps, scales in cc.chosen_map_sets()]
    return _SETS


@pytest.mark.parametrize("two_launches", [False, True], ids=["merged", "two_launches"])
def test_postprocess_confidences_equal_the_reference(weights, monkeypatch, two_launches):
    """Every chosen map set (S = 1, 3, 4, 8: post_kernel<3> and <VNECT_MAX_S>; reference, baseline and near-1 scales) through
    est.postprocess(..., return_confidence=True): the confidences equal the reference, and the joints equal the same call without the
    keyword on reset filters."""
    from vnect_amd import VNectEstimator
    if two_launches:
        monkeypatch.setenv("VNECT_NO_POST_MERGE", "1")
    seen, ests = set(), {}
    for name, maps, scales, want in _sets():
        key = tuple(scales)
        if key not in ests:
            ests[key] = VNectEstimator(scales=scales, weights=weights, verbose=False)
        est = ests[key]
        est.reset()
        p2, p3 = est.postprocess(maps, timestamp=(T0, T0 + 0.0005))
        est.reset()
        res = est.postprocess(maps, timestamp=(T0, T0 + 0.0005), return_confidence=True)
        assert len(res) == 3
        j2, j3, conf = res
        print(name, "max |conf - reference|", float(np.abs(conf - want).max()))
        assert conf.dtype == np.float64 and conf.shape == (21,)
        assert cc.same_conf(conf, want), (name, two_launches, np.nonzero(conf != want)[0], conf, want)
        assert np.array_equal(j2, p2) and np.array_equal(j3, p3), name
        again = est.handle.result_confidence()
        assert again[1] == 0 and np.array_equal(again[0], conf) and again[0] is not conf
        seen.add(len(scales))
    for est in ests.values():
        est.close()
    assert seen >= {1, 3, 4, 8}


@pytest.mark.parametrize("two_launches", [False, True], ids=["merged", "two_launches"])
def test_all_nan_heat_map_gives_minus_infinity(weights, monkeypatch, two_launches):
    """An all-NaN heat-map of one joint: -inf (NaN cells never win the arg-max), every other joint as the reference."""
    if two_launches:
        monkeypatch.setenv("VNECT_NO_POST_MERGE", "1")
    _, maps, scales, want = [s for s in _sets() if s[0] == "edge_baseline"][0]
    maps = maps.copy()
    maps[:, :, :, 6] = np.nan
    h = _handle(scales, weights)
    h.postprocess(maps, T0, T0)
    conf, lost = h.result_confidence()
    h.close()
    assert conf[6] == -np.inf and lost == 0
    others = np.arange(21) != 6
    assert cc.same_conf(conf[others], want[others])


def test_no_confidence_before_a_result(weights):
    from vnect_amd import _native
    h = _handle([1.0], weights)
    with pytest.raises(_native.VnectError) as e:
        h.result_confidence()
    assert e.value.code == _native.E_STATE
    # a failed call leaves the previous values standing
    maps = _sets()[0][1]
    h.postprocess(maps, T0, T0)
    first = h.result_confidence()[0]
    with pytest.raises(_native.VnectError):
        h.postprocess(maps, T0, T0)          # the same timestamp again: VNECT_E_TIMESTAMP
    assert np.array_equal(h.result_confidence()[0], first)
    assert _native.lib().vnect_result_confidence(h._h, first.ctypes.data_as(C.POINTER(C.c_double)), None) == 0   # lost_out may be NULL
    h.close()


_PLANTED = {}


def _planted_frames(n):
    from tests import planted
    if "w" not in _PLANTED:
        _PLANTED["w"] = planted.weights()
    return _PLANTED["w"], [planted.frame(40 + k)[0] for k in range(n)]


def _own_maps(est, frame):
    batch, _, _ = est.gen_input_batch(frame, 368, est.scales, _handle=est.handle)
    return est.forward(batch)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_estimator_confidences_equal_the_reference_of_its_own_maps(precision):
    """est(frame, return_confidence=True) on a planted frame: the confidences equal conf_reference of the device's own maps (the planted
    peaks stand far above the noise: the joints with the strongest gain are the most confident)."""
    from vnect_amd import VNectEstimator
    w, frames = _planted_frames(1)
    est = VNectEstimator(scales=BASELINE_SCALES, weights=w, verbose=False, precision=precision)
    j2, j3, conf = est(frames[0], timestamp=(T0, T0 + 0.0005), return_confidence=True)
    want = cc.conf_reference(_own_maps(est, frames[0]), BASELINE_SCALES)
    plain = est(frames[0], timestamp=(T0 + 1, T0 + 1.0005))
    est.close()
    assert len(plain) == 2
    assert cc.same_conf(conf, want), (precision, conf, want)
    assert np.all(np.isfinite(conf)) and conf.max() > conf.min()


def test_three_frames_in_flight_each_collects_its_own(weights):
    """lanes=3, three different frames in flight: each collect(return_confidence=True) returns its own frame's confidences, not the
    newest frame's."""
    from vnect_amd import VNectEstimator
    w, frames = _planted_frames(3)
    frames = [frames[0], frames[1][::-1].copy(), (frames[2] // 3).astype(np.uint8)]
    est = VNectEstimator(scales=BASELINE_SCALES, weights=w, verbose=False, lanes=3)
    want = [cc.conf_reference(_own_maps(est, f), BASELINE_SCALES) for f in frames]
    assert not cc.same_conf(want[0], want[1]) and not cc.same_conf(want[1], want[2]) and not cc.same_conf(want[0], want[2])
    for rounds in range(2):
        for k, f in enumerate(frames):
            est.submit(f, timestamp=(T0 + rounds + 0.03 * k, T0 + rounds + 0.03 * k + 0.0005))
        for k in range(3):
            res = est.collect(return_confidence=True)
            assert len(res) == 3 and cc.same_conf(res[2], want[k]), (rounds, k)
    est.submit(frames[0], timestamp=(T0 + 5, T0 + 5.0005))
    assert len(est.collect()) == 2
    est.close()


def test_two_stream_batch_each_stream_equals_its_single_run():
    """vnect_submit_streams: one delivery per result, each stream's confidences those of its frame run alone."""
    from vnect_amd import VNectEstimator
    w, frames = _planted_frames(2)
    single = VNectEstimator(scales=BASELINE_SCALES, weights=w, verbose=False)
    want = [single(f, timestamp=(T0, T0 + 0.0005), return_confidence=True)[2] for f in frames[:1]]
    single.reset()
    want.append(single(frames[1], timestamp=(T0, T0 + 0.0005), return_confidence=True)[2])
    single.close()
    h = _handle(BASELINE_SCALES, w, stream_batch=2)
    for slot, f in enumerate(frames):
        h.upload_frame(slot, f)
    h.submit_streams([0, 1], [0, 1], [T0, T0], [T0 + 0.0005, T0 + 0.0005])
    for k in range(2):
        s, _, _ = h.collect_stream()
        conf, lost = h.result_confidence()
        assert s == k and lost == 0 and cc.same_conf(conf, want[k]), (k, conf, want[k])
    h.close()
