"""GPU (MI355X), through the C ABI: every readable tensor of keep_activations handles against its per-launch float64 reference,
per element (tests/layer_ref.py: the device's own inputs, the rigorous and the calibrated fp32 accumulation bound, bf16's half ulp
on top, the bf16 match fraction).  Configurations: fp32 / bf16 / split-product at the baseline scales on a square and a non-square
frame; 1, 2, 4, 5, 6, 7 and 8 scales (other tile shapes, split-K + splitk_reduce_kernel, the stand-alone bone kernel; eight is
VNECT_MAX_SCALES: the edge of every per-image array, the arena, the split-K workspace); every forced tile
shape in every precision; the fused stem; two more weight sets; the paper wiring of res2c (paper_res2c=True, gated by
layer_ref.TABLE_PAPER: its six stand-alone res2b / res2c launches) at the baseline scales, at one scale and under the fused stem.
Every launch of every plan must map to a checked tensor of its wiring's table.
Per-configuration tables: layer_bounds.json in the tests' log directory (gpu_common.OUT)."""
import numpy as np
import pytest

from tests import layer_ref
from tests.gpu_common import BASELINE_SCALES, _handle, _log, _native, _read_table

pytestmark = pytest.mark.gpu

SIX = [1.0, 0.95, 0.9, 0.8, 0.7, 0.6]
FIVE = [1.0, 0.9, 0.8, 0.7, 0.6]
SEVEN = [1.0, 0.92, 0.84, 0.76, 0.68, 0.6, 0.5]
EIGHT = [1.0, 0.93, 0.86, 0.79, 0.72, 0.65, 0.58, 0.45]   # (0.45: below the smallest scale the stem's from-the-frame form fits)
TILES = ["64,64,1,1", "64,32,2,1", "32,32,4,1", "64,64,1,5", "64,32,2,2", "32,32,4,3"]  # test_every_tile_shape_on_every_layer


def _configs():
    c = []
    for prec in ("fp32", "bf16", "fp32_split"):
        for fr in ("square", "300x368"):
            c.append(("base_%s_%s" % (prec, fr), BASELINE_SCALES, prec, fr, {}, "synthetic", False))
    for prec in ("fp32", "bf16"):
        for scales in ([1.0], [1.0, 0.7], [1, 0.85, 0.7, 0.5], SIX, FIVE, SEVEN, EIGHT):
            c.append(("S%d_%s" % (len(scales), prec), scales, prec, "square", {}, "synthetic", False))
    for force in TILES:
        for prec in ("fp32", "bf16", "fp32_split"):
            c.append(("tile%s_%s" % (force.replace(",", "x"), prec), [1.0, 0.7], prec, "square",
                      {"VNECT_FORCE_TILE": force, "VNECT_NO_STEM": "1"}, "synthetic", False))
    for prec in ("fp32", "bf16"):
        c.append(("stem_%s" % prec, BASELINE_SCALES, prec, "square", {"VNECT_FORCE_STEM": "batch"}, "synthetic", False))
    c.append(("seed7_bf16", BASELINE_SCALES, "bf16", "square", {}, "seed7", False))
    c.append(("planted_bf16", BASELINE_SCALES, "bf16", "planted", {}, "planted", False))
    # the paper wiring (one scale: M = 8464 = 132 x 64 + 16 at the 92x92 stage and 2116 = 33 x 64 + 4 at 46x46, partial last tiles)
    for prec in ("fp32", "bf16", "fp32_split"):
        c.append(("paper_base_%s" % prec, BASELINE_SCALES, prec, "square", {}, "synthetic", True))
    for prec in ("fp32", "bf16"):
        c.append(("paper_S1_%s" % prec, [1.0], prec, "square", {}, "synthetic", True))
    c.append(("paper_stem_bf16", BASELINE_SCALES, "bf16", "square", {"VNECT_FORCE_STEM": "batch"}, "synthetic", True))
    return c


CONFIGS = _configs()
RESULTS = {}


def _weights(kind, default):
    from tests import planted
    from vnect_amd.weights import synthetic_weights
    if kind == "seed7":
        return synthetic_weights(seed=7)
    if kind == "planted":
        return planted.weights()
    return default


def _frame(kind):
    from tests import helpers, planted
    if kind == "square":
        return helpers.synth_frame(1234, smooth=True)
    if kind == "planted":
        return planted.frame(301)[0]
    return helpers.synth_frame(4242, 300, 368, smooth=True)


def _summary(paper=None):
    """worst figures per precision over the configurations run so far; paper=True / False: over those of one wiring"""
    out = {}
    for prec in ("fp32", "bf16", "fp32_split"):
        rows = [(cid, r) for cid, res in RESULTS.items() if res["prec"] == prec and paper in (None, res["paper_res2c"]) for r in res["rows"]]
        if not rows:
            continue
        m = [(r["match"], cid, r["tensor"]) for cid, r in rows if r["match"] is not None]
        c = [(r["c"], cid, r["tensor"]) for cid, r in rows if r["c"] is not None]
        out[prec] = dict(rigorous=max((r["rig"], cid, r["tensor"]) for cid, r in rows),
                         calibrated=max((r["cal"], cid, r["tensor"]) for cid, r in rows),
                         implied_c=max(c) if c else None, lowest_match=min(m) if m else None)
    return out


@pytest.mark.parametrize("cid,scales,prec,frame,env,wkind,paper", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_tensor_within_its_element_bounds(weights, monkeypatch, cid, scales, prec, frame, env, wkind, paper):
    import oracle
    n = _native()
    w = _weights(wkind, weights)
    table = layer_ref.TABLE_PAPER if paper else layer_ref.TABLE
    batch, _, _ = oracle.gen_input_batch(_frame(frame), scales)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = _handle(scales, w, precision={"fp32": n.FP32, "bf16": n.BF16, "fp32_split": n.FP32_SPLIT}[prec], keep_activations=True,
                paper_res2c=paper)
    for k in env:
        monkeypatch.delenv(k)
    try:
        launches = h.layers()
        out = h.forward(batch)
        # every tensor of the table is readable: a missing one raises (conv1 under the fused stem: refused, no launch writes it)
        acts = _read_table(h, unwritten=("conv1",) if "VNECT_FORCE_STEM" in env else (), table=table)
    finally:
        h.close()
    assert np.array_equal(out, acts["res5c_branch2c"])
    stem = "VNECT_FORCE_STEM" in env
    # split-product launches (rt_plan.cpp upload_layer_weights: 64x64 and 64x32x2 tiles, not conv1's gathered form)
    split = set()
    if prec == "fp32_split":
        for L in launches:
            if L["M"] and L["tile_m"] == 64 and L["tile_n"] in (32, 64) and L["name"] != "conv1":
                split.update(layer_ref.launch_tensors(L["name"], stem, table=table))
    rows = layer_ref.check_all(acts, w, prec, batch, stem=stem, split_tensors=split, table=table)
    checked = {r["tensor"] for r in rows}
    uncovered = [L["name"] for L in launches if not set(layer_ref.launch_tensors(L["name"], stem, table=table)) & checked]
    names = [L["name"] for L in launches]
    RESULTS[cid] = dict(prec=prec, scales=scales, env=env, weights=wkind, paper_res2c=paper, launches=names, rows=rows)
    _log("layer_bounds.json", dict(C_CAL=layer_ref.C_CAL, MATCH_FLOOR=layer_ref.MATCH_FLOOR, summary=_summary(),
                                   summary_default_wiring=_summary(False), summary_paper_wiring=_summary(True), configs=RESULTS))
    for r in rows:
        print("%-22s %-22s rigorous %.3g calibrated %.3g implied c %s match %s" % (
            cid, r["tensor"], r["rig"], r["cal"], "-" if r["c"] is None else "%.2f" % r["c"],
            "-" if r["match"] is None else "%.5f" % r["match"]))
    assert not uncovered, uncovered
    # the wiring shows in the plan: res2c_branch2a a launch of its own, and no launch that feeds both 3x3 layers from one tensor
    if paper:
        assert "res2c_branch2a" in names and not any("res2b_branch2b+res2c_branch2b" in x for x in names), names
    assert len(rows) == len(table) - (1 if stem else 0)
    bad = [r for r in rows if not r["ok"]]
    assert not bad, bad[:4]
