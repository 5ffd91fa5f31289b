"""GPU (MI355X), through the C ABI: the conv stack on weight families shaped like trained networks (tests/weight_families.py).

Every gate that the conv kernels pass on synthetic_weights() -- the per-element float64 bound (tests/layer_ref.py, tests/layer_ref_f16.py),
the fused plan's equality to the plain one (tests/test_gpu_fused_plan.py), the oracle parity of the final maps -- on weights the default
family never draws: folded BN scales that are negative, 0 and near 31.6, zero filters, channel magnitudes spread over 2^12, biases that carry
the output, activations at both ends of fp16's range.  The CPU stand-ins admit every family with room under the unchanged gates
(tests/test_weight_families_cpu.py), so a figure beyond a gate here is a finding about the kernels.
One scale wherever the shapes are free: M = 8464 = 132 x 64 + 16 at the 92 x 92 stage and 2116 = 33 x 64 + 4 at 46 x 46, partial last tiles.
Every figure, and the bf16 / fp16 final-map errors against the fp32 handle (recorded, not asserted: their gates were calibrated on one
family): weight_families.json in the tests' log directory (gpu_common.OUT)."""
import numpy as np
import pytest

from tests import layer_ref, layer_ref_f16, weight_families
from tests.gpu_common import _handle, _log, _native, _read_table
from tests.test_gpu_fused_plan import _with_env, fused_equals_plain
from tests.test_gpu_layer_bounds import SIX, TILES
from tests.weight_families import FAMILIES, FUSED_FAMILIES, SEEDS

pytestmark = pytest.mark.gpu

ONE = [1.0]
PRECS = ("fp32", "bf16", "fp32_split", "fp16")
PAPER_TOO = ("signed_bn", "dead")
ELEMENT_CASES = [(f, prec, paper) for f in FAMILIES for paper in ((False, True) if f in PAPER_TOO else (False,)) for prec in PRECS]
FUSED_CASES = [(f, prec, S) for f in FUSED_FAMILIES for prec in ("fp32", "bf16", "fp16") for S in (1, 3)]
BN = "res5c_branch2a_feat"

LOG = dict(C_CAL=layer_ref.C_CAL, MATCH_FLOOR=layer_ref.MATCH_FLOOR, MATCH_FLOOR_F16=layer_ref_f16.MATCH_FLOOR_F16, seeds=SEEDS,
           rows=[], worst={}, bn_forms={}, fused={}, oracle_parity={}, dead={}, map_error_of_fp32_max={}, overflow={})
_W, _BATCH, _MAPS = {}, {}, {}


def _weights(name):
    if name not in _W:
        _W[name] = weight_families.family(name, SEEDS.get(name, weight_families.OVERFLOW_SEED))
    return _W[name]


def _batch(scales):
    """the batch of the smooth frame 1234 at these scales, computed once"""
    import oracle
    from tests import helpers
    key = tuple(scales)
    if key not in _BATCH:
        _BATCH[key] = oracle.gen_input_batch(helpers.synth_frame(1234, smooth=True), scales)[0]
    return _BATCH[key]


def _prec(name):
    n = _native()
    return {"fp32": n.FP32, "bf16": n.BF16, "fp16": n.FP16, "fp32_split": n.FP32_SPLIT}[name]


def _keep_run(monkeypatch, w, prec, scales, env=None, paper=False):
    """(launches, final maps, every tensor of the table) of a keep_activations handle on the batch of these scales"""
    table = layer_ref.TABLE_PAPER if paper else layer_ref.TABLE
    h = _with_env(monkeypatch, env or {}, scales, w, precision=_prec(prec), keep_activations=True, paper_res2c=paper)
    try:
        launches = h.layers()
        out = h.forward(_batch(scales))
        acts = _read_table(h, table=table)
    finally:
        h.close()
    assert np.array_equal(out, acts["res5c_branch2c"])
    return launches, out, acts


def _split_tensors(prec, launches, table):
    """tensors written by a split-product launch (rt_plan.cpp upload_layer_weights: 64x64 and 64x32x2 tiles, not conv1's gathered form)"""
    split = set()
    if prec == "fp32_split":
        for L in launches:
            if L["M"] and L["tile_m"] == 64 and L["tile_n"] in (32, 64) and L["name"] != "conv1":
                split.update(layer_ref.launch_tensors(L["name"], table=table))
    return split


def _gate(acts, w, prec, batch, launches, table):
    if prec == "fp16":
        return layer_ref_f16.check_all(acts, w, batch, table=table)
    return layer_ref.check_all(acts, w, prec, batch, split_tensors=_split_tensors(prec, launches, table), table=table)


def _worst(rows):
    c = [(r["c"], r["tensor"]) for r in rows if r.get("c") is not None]
    m = [(r["match"], r["tensor"]) for r in rows if r["match"] is not None]
    return dict(rigorous=max((r["rig"], r["tensor"]) for r in rows), calibrated=max((r["cal"], r["tensor"]) for r in rows),
                implied_c=max(c) if c else None, lowest_match=min(m) if m else None)


def _flush():
    _log("weight_families.json", LOG)


def _print(tag, rows):
    for r in rows:
        print("%-28s %-22s rigorous %.3g calibrated %.3g implied c %s match %s" % (
            tag, r["tensor"], r["rig"], r["cal"], "-" if r.get("c") is None else "%.2f" % r["c"],
            "-" if r["match"] is None else "%.5f" % r["match"]))


@pytest.mark.parametrize("fam,prec,paper", ELEMENT_CASES, ids=["%s-%s%s" % (f, p, "-paper" if q else "") for f, p, q in ELEMENT_CASES])
def test_every_tensor_within_its_element_bounds(monkeypatch, fam, prec, paper):
    w = _weights(fam)
    table = layer_ref.TABLE_PAPER if paper else layer_ref.TABLE
    launches, out, acts = _keep_run(monkeypatch, w, prec, ONE, paper=paper)
    names = [L["name"] for L in launches]
    rows = _gate(acts, w, prec, _batch(ONE), launches, table)
    checked = {r["tensor"] for r in rows}
    uncovered = [n for n in names if not set(layer_ref.launch_tensors(n, table=table)) & checked]
    tag = "%s %s%s" % (fam, prec, " paper" if paper else "")
    for r in rows:
        LOG["rows"].append(dict(family=fam, precision=prec, paper_res2c=paper, **r))
    LOG["worst"][tag] = _worst(rows)
    if not paper:
        _MAPS[fam, prec] = out
    _flush()
    _print(tag, rows)
    assert not uncovered, uncovered
    if paper:
        assert "res2c_branch2a" in names and not any("res2b_branch2b+res2c_branch2b" in x for x in names), names
    assert len(rows) == len(table)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad[:4]
    if fam == "dead":
        _dead_channels_are_exact(tag, acts, w, prec, table)


def _dead_channels_are_exact(tag, acts, w, prec, table):
    """Every element whose float64 reference is exactly 0 because every term of its sum is (A == 0: zero filter and zero bias, or all of
    its inputs 0) is exactly 0 on the device; a channel with a zero filter and a negative bias, which ReLU kills at every pixel, is all
    zeros; one with a zero filter and a positive bias holds the bias everywhere (0.5: exact in every format)."""
    lw = layer_ref_f16.layer_weights(w) if prec == "fp16" else layer_ref.layer_weights(w, "bf16" if prec == "bf16" else "fp32")
    dead = weight_families.dead_channels(w)
    n_exact = n_killed = n_const = 0
    layers = set()
    for name, (op, ins, p) in table.items():
        if op != "conv":
            continue
        r = layer_ref.reference(name, acts, lw, table)
        zero = r["A"] == 0
        assert np.all(r["y"][zero] == 0)
        assert np.all(acts[name][zero] == 0), (tag, name, int((acts[name][zero] != 0).sum()))
        n_exact += int(zero.sum())
        if len(ins) > 1 or not p["relu"]:
            continue
        b = w[p["scope"] + "/biases"]
        for ch in dead.get(p["scope"], ()):
            want = max(float(b[ch]), 0.0)
            assert np.all(r["y"][..., ch] == want)
            assert np.all(acts[name][..., ch] == want), (tag, name, int(ch), float(b[ch]))
            n_killed += b[ch] < 0
            n_const += b[ch] > 0
            layers.add(name)
    LOG["dead"][tag] = dict(exact_zero_elements=n_exact, relu_killed_channels=int(n_killed), constant_channels=int(n_const), layers=len(layers))
    _flush()
    assert n_exact > 0 and n_killed >= 3 and n_const >= 3 and len(layers) >= 3


def _bn_tensor(monkeypatch, tag, prec, scales, env, want_names, keep_fused=False):
    """The BN tensor of signed_bn on one launch form, against its float64 reference from the device's own res5b_branch2c_new."""
    w = _weights("signed_bn")
    h = _with_env(monkeypatch, dict(env, VNECT_KEEP_FUSED="1") if keep_fused else env, scales, w, precision=_prec(prec), keep_activations=True)
    try:
        launches = h.layers()
        h.forward(_batch(scales))
        acts = {n: h.activation(n) for n in ("res5b_branch2c_new", BN)}
    finally:
        h.close()
    names = [L["name"] for L in launches]
    lw = layer_ref_f16.layer_weights(w) if prec == "fp16" else layer_ref.layer_weights(w, prec)
    r = layer_ref.reference(BN, acts, lw)
    row = layer_ref_f16.check_tensor(BN, acts[BN], r, True) if prec == "fp16" else layer_ref.check_tensor(BN, acts[BN], r, prec == "bf16")
    deconv = next(L for L in launches if L["name"].startswith("res5c_deconv"))
    LOG["bn_forms"][tag] = dict(launch=deconv["name"], tile=[deconv["tile_m"], deconv["tile_n"], deconv["split_k"]],
                                workgroups=deconv["workgroups"], row=row)
    _flush()
    _print(tag, [row])
    for n in want_names:
        assert n in names, (n, names)
    # a column of negative scale is no column of zeros, and one of scale 0 holds relu(beta), rounded once, at every pixel
    scale, beta = layer_ref.fold_bn(w)[1], w["bn5c_branch2a/beta"]
    rnd = {"fp32": np.float32, "bf16": layer_ref._round_bf16, "fp16": layer_ref_f16.round_f16}[prec]
    assert any(np.any(acts[BN][..., c] > 0) for c in np.nonzero(scale < 0)[0])
    zeros = np.nonzero(scale == 0)[0]
    assert len(zeros) == 4
    for c in zeros:
        assert np.all(r["y"][..., c] == max(float(beta[c]), 0.0))
        assert np.all(acts[BN][..., c] == rnd(np.float32(max(float(beta[c]), 0.0)))), (tag, int(c))
    assert row["ok"], row
    return names


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("force", TILES, ids=[t.replace(",", "x") for t in TILES])
def test_bn_epilogue_on_every_forced_tile(monkeypatch, force, prec):
    names = _bn_tensor(monkeypatch, "tile%s %s" % (force.replace(",", "x"), prec), prec, [1.0, 0.7],
                       {"VNECT_FORCE_TILE": force, "VNECT_NO_STEM": "1"}, ["res5c_deconv", "res5c_bone_length"])
    assert "res5c_deconv+bone_length" not in names
    # the forced shape reached the transposed conv: tile rows, tile columns, K split
    bm, bn, _, ks = (int(x) for x in force.split(","))
    assert LOG["bn_forms"]["tile%s %s" % (force.replace(",", "x"), prec)]["tile"] == [bm, bn, ks]


def test_bn_epilogue_at_six_scales(monkeypatch):
    """... where the bone features are a launch of their own in the arena plan too (more than five scales)"""
    _bn_tensor(monkeypatch, "S6 fp32", "fp32", SIX, {}, ["res5c_deconv", "res5c_bone_length"])
    arena = _handle(SIX, _weights("signed_bn"))
    try:
        names = [L["name"] for L in arena.layers()]
    finally:
        arena.close()
    assert "res5c_bone_length" in names and "res5c_deconv+bone_length" not in names, names


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_bn_epilogue_with_the_bone_features_in_the_launch(monkeypatch, prec):
    """The arena plan's form, on private buffers (VNECT_KEEP_FUSED=1): the transposed conv computes the bone features itself.  Two scales:
    at one, the layer runs 64 x 32 tiles with two K groups, which do not take them."""
    names = _bn_tensor(monkeypatch, "fused S2 %s" % prec, prec, [1.0, 0.7], {}, ["res5c_deconv+bone_length"], keep_fused=True)
    assert "res5c_bone_length" not in names
    arena = _handle([1.0, 0.7], _weights("signed_bn"), precision=_prec(prec))
    try:
        assert "res5c_deconv+bone_length" in [L["name"] for L in arena.layers()]
    finally:
        arena.close()


@pytest.mark.parametrize("fam,prec,S", FUSED_CASES, ids=["%s-%s-S%d" % c for c in FUSED_CASES])
def test_fused_launches_equal_the_plain_plan(monkeypatch, fam, prec, S):
    """tests/test_gpu_fused_plan.py's rule on a family's weights: every tensor the product plan stores is bit-identical to the stand-alone
    plan's, which passes the float64 gate in the same test."""
    cid = "%s_%s_S%d" % (fam, prec, S)
    rows = fused_equals_plain(_weights(fam), monkeypatch, cid, prec, S, {}, False, LOG["fused"])
    LOG["worst"]["%s %s fused S%d plain plan" % (fam, prec, S)] = _worst(rows)
    _flush()


@pytest.mark.parametrize("fam", FAMILIES)
def test_final_maps_match_the_oracle(fam):
    """fp32: the final maps within 1e-4 of the map maximum of the CPU oracle on the family's weights (test_conv_stack_every_layer's gate)"""
    import oracle
    w = _weights(fam)
    ref = oracle.Oracle(w).forward(_batch(ONE))
    out = _final_maps(fam, "fp32")
    err = float(np.abs(out - ref).max() / np.abs(ref).max())
    LOG["oracle_parity"][fam] = err
    _flush()
    print("%-15s final maps %.3g of the oracle's map maximum" % (fam, err))
    assert np.all(np.isfinite(ref)) and err <= 1e-4


def _final_maps(fam, prec):
    if (fam, prec) not in _MAPS:
        h = _handle(ONE, _weights(fam), precision=_prec(prec))
        try:
            _MAPS[fam, prec] = h.forward(_batch(ONE))
        finally:
            h.close()
    return _MAPS[fam, prec]


def test_record_the_16_bit_final_map_errors():
    """bf16 and fp16 final maps against the fp32 handle's, of its map maximum, per family: recorded, not asserted (the 3e-2 and EPS16 gates
    were calibrated on one family); finite in every family."""
    for fam in FAMILIES:
        f = _final_maps(fam, "fp32")
        top = float(np.abs(f).max())
        errs = {p: float(np.abs(_final_maps(fam, p) - f).max()) / top for p in ("bf16", "fp16")}
        LOG["map_error_of_fp32_max"][fam] = errs
        print("%-15s final-map error of the fp32 map maximum: bf16 %.3g fp16 %.3g" % (fam, errs["bf16"], errs["fp16"]))
        assert all(np.isfinite(e) for e in errs.values()), (fam, errs)
    _flush()


def test_fp16_overflow_stores_infinity(monkeypatch):
    """FP16.md: the store rounds to nearest even, so a result beyond 65 520 is stored as +-inf.  f16_overflow puts such results into
    res2a_branch2a and into no tensor in front of it (tests/test_weight_families_cpu.py).  Tensors behind it are not gated."""
    w = _weights("f16_overflow")
    first = weight_families.OVERFLOW_TENSOR
    h = _handle(ONE, w, precision=_native().FP16, keep_activations=True)
    try:
        h.forward(_batch(ONE))
        order = list(layer_ref.TABLE)
        acts = {n: h.activation(n) for n in order[:order.index(first) + 1]}
    finally:
        h.close()
    before = {k: v for k, v in acts.items() if k != first}
    assert all(np.all(np.isfinite(v)) for v in before.values())
    rows = layer_ref_f16.check_all(before, w, _batch(ONE))
    assert len(rows) == len(before) and not [r for r in rows if not r["ok"]], rows
    r = layer_ref.reference(first, acts, layer_ref_f16.layer_weights(w))
    row = layer_ref_f16.check_overflow(first, acts[first], r)
    LOG["overflow"] = row
    _flush()
    print(row)
    assert row["over"] >= 100 and row["band"] < 0.01 * row["large"], row
    assert row["ok"], row
