"""The weight families of tests/weight_families.py under the CPU stand-ins (no GPU needed).

(a) Admission.  Every family passes every tensor of the per-element float64 gate on the clean stand-ins -- tests/test_layer_bounds_cpu.py's
for fp32 and bf16, tests/test_fp16_bounds_cpu.py's for fp16; signed_bn and dead in the paper wiring of res2c as well -- and with room under
the unchanged gates: implied c <= 0.6 C_CAL, bf16 match >= 0.9994, fp16 match >= 0.996.  These are conditions on the reference arithmetic;
a family that missed one was narrowed or re-seeded (weight_families.SEEDS), the gates stay.  So a figure beyond a gate on the device
(tests/test_gpu_weight_families.py) is a finding about the kernels.  The families of the fused-plan equality are admitted at its three
scales too: an image scaled below 1 is padded with a constant, every channel of the early layers holds ONE value over the thousands of
padded pixels, and a single such value next to a rounding midpoint moves a tensor's match fraction by half a percent (signed_bn at seed 72:
0.9921 in fp16 on res2a_branch2b here, 0.9927 on the MI355X, against 0.9980 at one scale).
(b) The families are what they claim: signed_bn folds to scales that are negative, exactly 0 and above 20; dead has channels that are
exactly 0 and channels that ReLU kills, in many layers; f16_range fills fp16's range at both ends without overflowing; f16_overflow puts
results beyond 65 520 into exactly one early tensor, with next to none of them in the band the overflow rule of FP16.md leaves open.
(c) The families see what the default weights cannot: each fault of test_layer_bounds_cpu.FAMILY_FAULTS passes every tensor under
synthetic_weights() and fails on exactly its own tensor under its family (the two fp16 candidates: see tests/test_fp16_bounds_cpu.py).
One scale at 368 x 368, the smooth frame 1234."""
import os

import numpy as np
import pytest

from tests import helpers, layer_ref, layer_ref_f16, weight_families
from tests import test_fp16_bounds_cpu as f16_stand_in
from tests import test_layer_bounds_cpu as stand_in
from tests.layer_ref import C_CAL, TABLE, TABLE_PAPER
from tests.weight_families import FAMILIES, FUSED_FAMILIES, SEEDS

C_ADMIT = 0.6 * C_CAL
MATCH_ADMIT = {"bf16": 0.9994, "fp16": 0.996}
PAPER_TOO = ("signed_bn", "dead")
F16_MAX = 65504.0
TINY = 2.0 ** -14      # fp16's smallest normal
CASES = [(f, prec, paper) for f in FAMILIES for paper in ((False, True) if f in PAPER_TOO else (False,)) for prec in ("fp32", "bf16", "fp16")]


@pytest.fixture(scope="module")
def batch():
    frame = helpers.synth_frame(1234, smooth=True).astype(np.float32)
    return (frame / 255.0 - 0.4)[None]


_W = {}


def _weights(name):
    if name not in _W:
        _W[name] = weight_families.family(name, SEEDS.get(name, weight_families.OVERFLOW_SEED))
    return _W[name]


def _run(w, batch, prec, paper=False, fault=None):
    """(activations of the stand-in, rows of the gate)"""
    table = TABLE_PAPER if paper else TABLE
    if prec == "fp16":
        acts = f16_stand_in.device_forward(w, batch, fault, table=table)
        return acts, layer_ref_f16.check_all(acts, w, batch, table=table)
    acts, _ = stand_in.device_forward(w, batch, prec, fault, paper=paper)
    return acts, layer_ref.check_all(acts, w, prec, batch, table=table)


_CLEAN = {}


@pytest.fixture(scope="module")
def clean(batch):
    """the clean stand-in of a family, computed once per (family, precision, wiring) and left unchanged"""
    def get(name, prec, paper=False):
        key = (name, prec, paper)
        if key not in _CLEAN:
            _CLEAN[key] = _run(_weights(name), batch, prec, paper)
        return _CLEAN[key]
    return get


@pytest.fixture(scope="module")
def batch3():
    import oracle
    from tests.gpu_common import BASELINE_SCALES
    return oracle.gen_input_batch(helpers.synth_frame(1234, smooth=True), BASELINE_SCALES)[0]


def _failing(rows):
    return sorted(r["tensor"] for r in rows if not r["ok"])


def _stored(acts):
    """the stored activations of a 16-bit handle: every tensor but the fp32 final maps"""
    return {k: v for k, v in acts.items() if k != "res5c_branch2c"}


@pytest.mark.parametrize("name,prec,paper", CASES, ids=["%s-%s%s" % (f, p, "-paper" if q else "") for f, p, q in CASES])
def test_family_is_admitted(clean, name, prec, paper):
    acts, rows = clean(name, prec, paper)
    _admit("%s %s%s" % (name, prec, " paper" if paper else ""), acts, rows, prec, len(TABLE) + paper)


def _admit(tag, acts, rows, prec, n):
    cs = [(r["c"], r["tensor"]) for r in rows if r.get("c") is not None]
    ms = [(r["match"], r["tensor"]) for r in rows if r["match"] is not None]
    c, m = (max(cs) if cs else (None, "-")), (min(ms) if ms else (None, "-"))
    top = max(float(np.abs(v).max()) for v in acts.values())
    print("%-28s worst implied c %s (%s)  lowest match %s (%s)  worst rigorous %.3g calibrated %.3g  largest |activation| %.4g" % (
        tag, "-" if c[0] is None else "%.2f" % c[0], c[1], "-" if m[0] is None else "%.5f" % m[0], m[1],
        max(r["rig"] for r in rows), max(r["cal"] for r in rows), top))
    assert len(rows) == n
    assert _failing(rows) == [], [r for r in rows if not r["ok"]][:3]
    if cs:
        assert c[0] <= C_ADMIT, c
    if ms:
        assert m[0] >= MATCH_ADMIT[prec], m


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", FUSED_FAMILIES)
def test_family_is_admitted_at_three_scales(batch3, name, prec):
    acts, rows = _run(_weights(name), batch3, prec)
    _admit("%s %s three scales" % (name, prec), acts, rows, prec, len(TABLE))


def test_signed_bn_folds_to_negative_zero_and_large_scales():
    w = _weights("signed_bn")
    _, scale, _ = layer_ref.fold_bn(w)
    g, va = w["bn5c_branch2a/gamma"], w["bn5c_branch2a/moving_variance"]
    print("signed_bn: folded scale %.4g .. %.4g; %d negative, %d exactly 0, %d above 20; %d channels of variance 0" % (
        scale.min(), scale.max(), (scale < 0).sum(), (scale == 0).sum(), (scale > 20).sum(), (va == 0).sum()))
    assert (g == 0).sum() == 4 and (va == 0).sum() == 4
    assert (scale < 0).sum() >= 32 and (scale == 0).sum() == 4 and (scale > 20).sum() >= 1 and (scale < -20).sum() >= 1
    # variance 0 reaches the largest factor the fold can give, 1 / sqrt(0.001), in either sign
    big = np.float32(1.0) / np.sqrt(np.float32(0.001))
    assert np.any(scale == big) and np.any(scale == -big)
    # ... and the default weights have none of it
    from vnect_amd.weights import synthetic_weights
    s0 = layer_ref.fold_bn(synthetic_weights())[1]
    assert s0.min() > 0.3 and s0.max() < 2.2


def test_dead_has_exact_zero_channels_and_relu_killed_channels(clean):
    """Per ReLU layer without a shortcut: channels whose float64 reference is exactly 0 because every term of their sum is (A == 0: zero
    filter, zero bias), and channels that ReLU kills everywhere (zero filter, bias -1: the float64 pre-activation is -1 at every pixel)."""
    w = _weights("dead")
    acts, _ = clean("dead", "fp32")
    dead = weight_families.dead_channels(w)
    exact, killed, constant = [], [], []
    for name, (op, ins, p) in TABLE.items():
        if op != "conv" or len(ins) > 1 or not p["relu"] or p["scope"] not in dead:
            continue
        r = layer_ref.reference(name, acts, w)
        b = w[p["scope"] + "/biases"]
        for ch in dead[p["scope"]]:
            y, A = r["y"][..., ch], r["A"][..., ch]
            assert np.all(y == max(float(b[ch]), 0.0)), (name, ch)
            if b[ch] == 0:
                assert np.all(A == 0)
                exact.append(name)
            elif b[ch] < 0:
                assert np.all(A == -float(b[ch]))
                killed.append(name)
            else:
                constant.append(name)
    print("dead: exactly-0 channels in %d layers (%d channels), ReLU-killed channels in %d layers (%d), constant channels in %d layers (%d)" % (
        len(set(exact)), len(exact), len(set(killed)), len(killed), len(set(constant)), len(constant)))
    assert len(set(exact)) >= 3 and len(set(killed)) >= 3 and len(set(constant)) >= 3
    from vnect_amd.weights import synthetic_weights
    assert weight_families.dead_channels(synthetic_weights()) == {}


def test_f16_range_fills_fp16s_range_at_both_ends(clean):
    a32, _ = clean("f16_range", "fp32")
    a16, _ = clean("f16_range", "fp16")
    top = max(float(np.abs(v).max()) for v in _stored(a32).values())
    top16 = max(float(np.abs(v).max()) for v in _stored(a16).values())
    sub = sum(int(((np.abs(v) < TINY) & (v != 0)).sum()) for v in _stored(a16).values())
    print("f16_range: largest stored |activation| fp32 %.5g, fp16 %.5g (fp16 holds up to 65 504); %d stored nonzero fp16 elements below 2^-14" % (
        top, top16, sub))
    assert 2.0 ** 14 <= top < F16_MAX
    assert all(np.all(np.isfinite(v)) for v in a16.values()) and top16 < F16_MAX
    assert sub >= 100


def test_f16_overflow_overflows_exactly_one_early_tensor(batch):
    """The family behind the overflow rule of FP16.md (a result beyond 65 520 is stored as +-inf): of the tensors computed from finite
    inputs exactly one, res2a_branch2a, holds such results; the band around 65 520 that the rule leaves open holds under 1 % of that tensor's
    elements with |y| > 2^15."""
    w = _weights("f16_overflow")
    with np.errstate(over="ignore", invalid="ignore"):
        acts = f16_stand_in.device_forward(w, batch)
    order = [n for n in TABLE if n != "input"]
    first = next(n for n in order if not np.all(np.isfinite(acts[n])))
    assert first == weight_families.OVERFLOW_TENSOR == "res2a_branch2a"
    finite_in = [n for n in order if all(np.all(np.isfinite(acts[i])) for i in TABLE[n][1] if i != n)]
    assert [n for n in finite_in if not np.all(np.isfinite(acts[n]))] == [first], finite_in
    r = layer_ref.reference(first, acts, layer_ref_f16.layer_weights(w))
    row = layer_ref_f16.check_overflow(first, acts[first], r)
    print("f16_overflow: %s holds %d results beyond 65 520 + bound, %d above 2^15, %d in the open band (%.3f %%); the stand-in stores %d inf; "
          "below the band: rigorous %.3g calibrated %.3g" % (first, row["over"], row["large"], row["band"], 100.0 * row["band"] / row["large"],
                                                            row["stored_inf"], row["rig"], row["cal"]))
    assert row["over"] >= 100 and row["band"] < 0.01 * row["large"]
    assert row["ok"], row


FAULT_CASES = [(f, prec, fam, t) for f, (t, prec, fam) in sorted(stand_in.FAMILY_FAULTS.items())]


@pytest.mark.parametrize("fault,prec,fam,target", FAULT_CASES, ids=[c[0] for c in FAULT_CASES])
def test_family_fault_hides_under_the_default_weights_and_fails_under_its_family(weights, batch, fault, prec, fam, target):
    _, rows = _run(weights, batch, prec, fault=fault)
    assert len(rows) == len(TABLE)
    print("%-10s passes under the default weights: every one of %d tensors (its own, %s: rigorous %.3g calibrated %.3g)" % (
        fault, len(rows), target, *[next(r[k] for r in rows if r["tensor"] == target) for k in ("rig", "cal")]))
    assert _failing(rows) == [], [r for r in rows if not r["ok"]][:3]
    _, rows = _run(_weights(fam), batch, prec, fault=fault)
    row = next(r for r in rows if r["tensor"] == target)
    print("%-10s fails on exactly its own tensor under its family %s: %s (rigorous %.3g calibrated %.3g)" % (
        fault, fam, _failing(rows), row["rig"], row["cal"]))
    assert _failing(rows) == [target]


def test_at_least_two_family_faults_are_planted():
    assert len(FAULT_CASES) >= 2


def test_the_tools_import_the_one_family_definition():
    """tools/bf16_gate_spread.py and tools/fp16_rate.py take their weight sets from weight_families.family, under the names they printed
    before; the three families they had are unchanged (the first weight of each, at the tools' seeds)."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    for f in ("bf16_gate_spread.py", "fp16_rate.py"):
        src = open(os.path.join(tools, f)).read()
        assert "from tests.weight_families import family as variant" in src and "def variant" not in src, f
        for kind in ("default", "channel_scales", "heavy_tails", "big_biases"):
            assert '("%s", ' % kind in src, (f, kind)
    from vnect_amd.weights import synthetic_weights
    for seed in (11, 12):
        w0, w = synthetic_weights(seed), weight_families.family("channel_scales", seed)
        s = (2.0 ** np.random.RandomState(seed).uniform(-2, 2, size=64)).astype(np.float32)
        s /= np.sqrt(np.mean(s ** 2))
        assert np.array_equal(w["conv1/weights"], w0["conv1/weights"] * s)
    assert np.array_equal(weight_families.family("big_biases", 31)["conv1/biases"], synthetic_weights(31)["conv1/biases"] * 8.0)
    assert all(np.array_equal(v, synthetic_weights(3)[k]) for k, v in weight_families.family("default", 3).items())
