"""CPU: the per-joint confidence's definition, the loss rule's loop and the ABI around them (CONFIDENCE.md) -- and the conditions the GPU
tests' case sets must meet, asserted here from the references alone so that no GPU test can pass vacuously."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import conf_cases as cc
from tests import track_cases as tc
from vnect_amd import _native, runner

ROOT = tc.ROOT


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
def test_reference_equals_a_numpy_restatement_of_the_upsample():
    """conf_reference (the oracle's resize) against cv2's rule restated in numpy, on every chosen map set: equal bit for bit."""
    sets = cc.chosen_map_sets()
    names = {n for n, _, _ in sets}
    assert {"argmax_cases", "all_negative", "constant", "peak_0_0_S1", "peak_45_45_S3", "random_baseline", "edge_near1", "edge_eight"} <= names
    assert {len(sc) for _, _, sc in sets} >= {1, 3, 4, 8}
    for name, maps, scales in sets:
        a, b = cc.conf_reference(maps, scales), cc.conf_numpy(maps, scales)
        assert a.dtype == np.float64 and a.shape == (21,) and np.all(np.isfinite(a)), name
        assert cc.same_conf(a, b), (name, np.nonzero(a != b)[0])


def test_known_confidences():
    """A constant map upsamples to the constant (the weights (1 - f, f) sum to 1 exactly); an all-negative map has a negative confidence;
    an isolated peak of level L does NOT upsample to L: no output pixel sits on a cell's centre (the nearest are 1/16 of a cell off in each
    axis, weight (15/16)^2) -- so a threshold has to be taken from the reference, never from the level."""
    sets = {n: (m, sc) for n, m, sc in cc.chosen_map_sets()}
    m, sc = sets["constant"]
    assert np.all(cc.conf_reference(m, sc) == np.float64(np.float32(0.3)))
    m, sc = sets["all_negative"]
    assert np.all(cc.conf_reference(m, sc) < 0)
    one = np.zeros((1, 46, 46, 84), np.float32)
    one[0, 20, 20, :21] = 0.5
    assert np.all(cc.conf_reference(one, [1.0]) == 0.5 * (15 / 16) ** 2)
    m, sc = sets["argmax_cases"]
    conf = cc.conf_reference(m, sc)
    assert conf[0] == 1.0 and conf[14] == -0.25 * (15 / 16) ** 2 - 1.0 * (1 - (15 / 16) ** 2)    # a plateau reaches its level; the negative peak


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------------
class _FakeEstimator:
    """What runner.track needs of an estimator, over scripted maps: the oracle's post-processing with the crop's geometry."""

    def __init__(self, maps, confs, scales):
        import oracle
        self.maps, self.confs, self.scales, self.k = maps, confs, scales, 0
        self.est = oracle.OracleEstimator(scales=scales, net=None)

    def __call__(self, crop, timestamp=None, return_confidence=False):
        geo = tc.crop_geometry(crop.shape[0], crop.shape[1], self.scales)
        j2, j3 = self.est.postprocess(self.maps[self.k], timestamp[0], timestamp[1], geo[0], geo[1], geo[2])
        self.k += 1
        return (j2, j3, self.confs[self.k - 1].copy()) if return_confidence else (j2, j3)


WALKS = [(H, W, action, above) for (H, W) in cc.WALK_SIZES for action in (cc.HOLD, cc.RESET) for above in (False, True)]


@pytest.mark.parametrize("H,W,action,above", WALKS)
def test_walk_conditions_and_runner_track(H, W, action, above):
    """Every walk the GPU tests run: at least 8 lost and 8 kept frames, a lost streak of 3 or more, a recovery, a frame with confident ==
    min_joints and one with min_joints - 1, and the EXACT frame -- a confidence equal to the threshold (kept), or, with the threshold one
    float64 above it, just below (lost).  No crop is refused.  runner.track(..., lost=...) over a scripted estimator equals the loop."""
    policy, frames = cc.walk_reference(H, W, action, above)
    c = cc.walk_conditions(policy, frames)
    assert c["frames"] == cc.WALK_FRAMES and frames[-1]["j2"] is not None, c
    assert c["lost"] >= 8 and c["kept"] >= 8 and c["streak"] >= 3 and c["recoveries"] >= 1, c
    assert c["at_min"] >= 1 and c["below_min"] >= 1, c
    f = frames[cc.EXACT_FRAME]
    if above:
        assert np.nextafter(f["conf"][cc.EXACT_JOINT], np.inf) == policy[0] and f["confident"] == policy[1] - 1 and f["lost"] == 1, c
    else:
        assert f["conf"][cc.EXACT_JOINT] == policy[0] and f["confident"] == policy[1] and f["lost"] == 0 and c["exact"] >= 1, c
    # the rule moves the crop: a held frame's successor is cropped like it, a reset one's with the whole frame
    for a, b in zip(frames, frames[1:]):
        if a["lost"]:
            assert b["used"] == (a["used"] if action == cc.HOLD else [0, 0, W, H])
        if b["lost"] and action == cc.HOLD:                     # a held frame leaves the state's bytes as they were
            assert b["state"].tobytes() == a["state"].tobytes()
        elif b["lost"]:
            assert b["state"].tobytes() == tc.frame_state(H, W, [0, 0, W, H]).tobytes()
    assert any(a["lost"] and a["next"] != b["used"] for a, b in zip(frames, frames[1:]))    # (and without the rule it would have moved elsewhere)
    spec = cc.walk_spec(cc.WALK_SIZES[(H, W)])
    maps = [cc.walk_maps(spec, tc.BASELINE_SCALES, k) for k in range(cc.WALK_FRAMES)]
    fake = _FakeEstimator(maps, [f["conf"] for f in frames], tc.BASELINE_SCALES)
    video = [np.zeros((H, W, 3), np.uint8)] * cc.WALK_FRAMES
    got = list(runner.track(fake, video, timestamps=tc.walk_times(cc.WALK_FRAMES), confidence=True,
                            lost=(policy[0], policy[1], "hold" if action == cc.HOLD else "reset")))
    assert len(got) == len(frames)
    for k, ((j2, j3, used, conf, lost), f) in enumerate(zip(got, frames)):
        assert list(used) == f["used"] and lost == f["lost"], (k, used, f["used"], lost, f["lost"])
        assert np.array_equal(j2, f["j2"]) and np.array_equal(j3, f["j3"]) and np.array_equal(conf, f["conf"]), k


def test_runner_defaults_are_todays_tuples():
    """Without the new keywords runner.track yields today's three values and never asks the estimator for confidences; lost= is checked."""
    policy, frames = cc.walk_reference(64, 96, cc.HOLD, False)
    spec = cc.walk_spec(cc.WALK_SIZES[(64, 96)])
    maps = [cc.walk_maps(spec, tc.BASELINE_SCALES, k) for k in range(4)]
    fake = _FakeEstimator(maps, [None] * 4, tc.BASELINE_SCALES)
    want = tc.cpu_loop(64, 96, None, maps, tc.walk_times(4), tc.BASELINE_SCALES)
    got = list(runner.track(fake, [np.zeros((64, 96, 3), np.uint8)] * 4, timestamps=tc.walk_times(4)))
    assert all(len(g) == 3 for g in got)
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and list(g[2]) == w[2]
    for bad in ((0.5, 0, "hold"), (0.5, 22, "hold"), (0.5, 3, "off"), (float("nan"), 3, "reset")):
        with pytest.raises(ValueError):
            runner.lost_rule(bad)
    assert runner.is_lost([0.5] * 10 + [np.nan, -np.inf] + [0.1] * 9, 0.5, 10) is False
    assert runner.is_lost([0.5] * 10 + [np.nan, -np.inf] + [0.1] * 9, 0.5, 11) is True


def test_init_box_returns_the_whole_frame_when_nobody_is_there():
    class Probe:
        def __init__(self, conf):
            self.conf, self.resets = conf, 0

        def __call__(self, frame, timestamp=None, return_confidence=False):
            j2 = np.array([[10.0 + j, 20.0 + 2 * j] for j in range(21)])
            return (j2, None, np.asarray(self.conf, np.float64)) if return_confidence else (j2, None)

        def reset(self):
            self.resets += 1

    frame = np.zeros((200, 300, 3), np.uint8)
    boxed = runner.init_box(Probe([0.9] * 21), frame)
    assert boxed != [0, 0, 300, 200]
    assert runner.init_box(Probe([0.9] * 21), frame, min_confidence=0.5, min_joints=8) == boxed
    p = Probe([0.9] * 7 + [0.1] * 14)
    assert runner.init_box(p, frame, min_confidence=0.5, min_joints=8) == [0, 0, 300, 200] and p.resets == 1
    assert runner.init_box(p, frame, min_confidence=0.5, min_joints=7) == boxed


# ---- the box stage's policy cases ------------------------------------------------------------------------------------------------------------------
def test_policy_cases_cover_what_the_gpu_test_claims():
    cases = cc.policy_cases()
    ref = cc.policy_reference(cases)
    n = len(cases["hdr"])
    live = cases["hdr"][:, 8] == tc.SQ_OK
    ver, act = ref["verdict"], cases["action"]
    assert n >= 5000 and (~live).sum() >= 100
    for a in (cc.OFF, cc.HOLD, cc.RESET):
        m = live & (act == a)
        assert m.sum() >= 1500, (a, m.sum())
        assert (ver[m, 0] == 1).sum() >= (0 if a == cc.OFF else 400) and (ver[m, 0] == 0).sum() >= 400, a
    assert np.all(ver[live & (act == cc.OFF), 0] == 0)
    assert (live & (ver[:, 1] == cases["min_joints"])).sum() >= 300 and (live & (ver[:, 1] == cases["min_joints"] - 1)).sum() >= 300
    with np.errstate(invalid="ignore"):
        assert (np.any(cases["conf"] == cases["thr"][:, None], axis=1) & live).sum() >= 300
        assert (np.any(np.nextafter(cases["conf"], np.inf) == cases["thr"][:, None], axis=1) & live).sum() >= 300
    assert np.isnan(cases["conf"]).any() and np.isposinf(cases["conf"]).any() and np.isneginf(cases["conf"]).any()
    # a held state that arrived behind an initial rect past the frame's edge keeps uw, uh (rewriting it from rect_used would not)
    held = live & (act == cc.HOLD) & (ver[:, 0] == 1)
    assert (held & ((cases["hdr"][:, 4] != cases["hdr"][:, 2]) | (cases["hdr"][:, 5] != cases["hdr"][:, 3]))).sum() >= 10
    assert np.array_equal(ref["hdr"][held], cases["hdr"][held])
    # a reset whose whole frame squarify refuses runs the refusal path
    reset = live & (act == cc.RESET) & (ver[:, 0] == 1)
    assert np.all(ref["hdr"][reset, :4] == np.stack([0 * cases["hdr"][reset, 0], 0 * cases["hdr"][reset, 0], cases["hdr"][reset, 7], cases["hdr"][reset, 6]], 1))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_names_version_and_sizes():
    hdr = open(os.path.join(ROOT, "include", "vnect_abi.h")).read()
    vmap = open(os.path.join(ROOT, "vnect_amd", "csrc", "vnect.map")).read()
    assert re.search(r"global:\s*vnect_\*;", vmap)
    for name in ("vnect_result_confidence", "vnect_track_policy"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _native.SYMBOLS
        pos = hdr.index("int " + name)
        assert "utils.py:169-172" in hdr[max(0, pos - 3500):pos] and "no counterpart" in hdr[max(0, pos - 3500):pos]
    assert "#define VNECT_ABI_VERSION 7" in hdr and _native.ABI_VERSION == 7 and C.sizeof(_native.Config) == 128
    L = _native.lib()
    assert L.vnect_abi_version() == 7
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
        assert {"vnect_result_confidence", "vnect_track_policy"} <= exported


def test_argument_validation_without_a_device():
    """Null handles and null outputs come back as VNECT_E_ARG from both entry points: no abort, no device needed."""
    L = _native.lib()
    conf, lost = (C.c_double * 21)(), C.c_int32(7)
    assert L.vnect_result_confidence(None, conf, C.byref(lost)) == _native.E_ARG
    assert L.vnect_result_confidence(None, None, None) == _native.E_ARG
    assert L.vnect_track_policy(None, 0, 0.5, 8, 1) == _native.E_ARG
    assert lost.value == 7
    assert _native.LOST_ACTIONS == {"off": 0, "hold": 1, "reset": 2}


def test_layouts_that_must_not_change():
    """JointsOut, TrackState and TrackOut stay as they are; ConfOut and TrackPolicy stand beside them."""
    k = open(os.path.join(ROOT, "vnect_amd", "csrc", "kernels.h")).read()
    assert re.search(r"struct JointsOut \{\s*double j2d\[NJ \* 2\];\s*float j3d\[NJ \* 3\];\s*int status;\s*\};", k)
    assert re.search(r"struct TrackOut \{[^}]*int rect\[4\];[^}]*int status;[^}]*int pad_;\s*\};", k)
    assert re.search(r"struct ConfOut \{\s*double conf\[NJ\];\s*int lost;\s*int confident;\s*\};", k)
    assert re.search(r"struct TrackPolicy \{\s*double min_confidence;\s*int min_joints;\s*int action;", k)
