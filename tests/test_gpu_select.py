"""GPU (MI355X), through the C ABI: every conv launch against an exact known answer -- selection weights (tests/select_ref.py).

Every output channel of every conv holds one weight, +1 or -1, at one tap and one input channel, and the batch holds small integers, so
every tensor is an integer gather of its input tensor and every product and partial sum is exact in fp32 in any order, tile shape, K split
or fused form.  Each tensor a plan stores must be np.array_equal to the int64 index rule applied to the DEVICE'S OWN input tensors (a
tensor a fused launch keeps on chip: composed by the same rule); a mismatch is a wrong index, halo, term or weight layout, never rounding.
The one exception is the bone-length columns res5c_branch2a_feat[..., 191:212], square roots of the device's stored deltas, which stay
under tests/layer_ref.py's bone bound; everything behind them copies the stored values and is exact again.  No other tolerance.
  a. per-layer plans (keep_activations): four precisions x four weight sets at one image; three and six images, the paper wiring of
     res2c, every forced tile shape, one bf16 plan on a wider batch whose stores round; in fp32 the final maps also equal the chain from the batch alone.
  b. the product plan's fused launches (VNECT_KEEP_FUSED=1), every stored tensor against the composed rule, split-product handles
     included (their fp32-instruction tail GEMMs are exact on integers); an arena handle returns the same final maps.
  c. the stem from the frame: what it stores is copies, maxima and a sign of the input, exact for any float input.
One row per run: select.json in the tests' log directory (gpu_common.OUT)."""
import functools

import numpy as np
import pytest

from tests import layer_ref, layer_ref_f16, select_ref as sr
from tests.gpu_common import BASELINE_SCALES, T0, _handle, _log, _native, _read_table
from tests.test_gpu_fused_plan import _stem_pair, _with_env, _written
from tests.test_gpu_layer_bounds import SIX, TILES

pytestmark = pytest.mark.gpu

SCALES = {1: [1.0], 3: BASELINE_SCALES, 6: SIX}
PRECS = ["fp32", "bf16", "fp16", "fp32_split"]
TABLES = {False: layer_ref.TABLE, True: layer_ref.TABLE_PAPER}
FEAT = "res5c_branch2a_feat"
ROWS = {}


def _layer_configs():
    c = [("%s_set%d" % (prec, s), prec, 1, s, False, {}) for prec in PRECS for s in range(sr.SETS)]
    c += [("%s_S3" % prec, prec, 3, i, False, {}) for i, prec in enumerate(PRECS)]
    c += [("%s_S6" % prec, prec, 6, 1 + i, False, {}) for i, prec in enumerate(("fp32", "bf16"))]
    c += [("paper_%s" % prec, prec, 1, 2 + i, True, {}) for i, prec in enumerate(("fp32", "bf16"))]
    c += [("bf16_wide", "bf16", 1, 0, False, {})]
    c += [("tile%s_%s" % (t.replace(",", "x"), prec), prec, 1, (i + j) % sr.SETS, False, {"VNECT_FORCE_TILE": t, "VNECT_NO_STEM": "1"})
          for i, t in enumerate(TILES) for j, prec in enumerate(("fp32", "bf16"))]
    return c


LAYER_CONFIGS = _layer_configs()
FUSED_CONFIGS = [("fused_%s_S%d" % (prec, S), prec, S, (i + S) % sr.SETS, False) for i, prec in enumerate(PRECS) for S in (1, 3)]
FUSED_CONFIGS += [("fused_paper_%s" % prec, prec, 1, i, True) for i, prec in enumerate(("bf16", "fp16"))]
FUSED_CONFIGS += [("fused_bf16_wide", "bf16", 1, 0, False)]


def _batch(cid, set_index, S):
    """*_wide: integers in +-WIDE[1], which take the chain past 2^8, where bf16 stores round (ties included): the rule's rounding points --
    every stored tensor, every on-chip hand-over -- are then part of the known answer (tests/test_select_cpu.py simulates that chain)"""
    return sr.batch(set_index, S, *sr.WIDE) if cid.endswith("_wide") else sr.batch(set_index, S)


def _prec(name):
    n = _native()
    return {"fp32": n.FP32, "bf16": n.BF16, "fp16": n.FP16, "fp32_split": n.FP32_SPLIT}[name]


@functools.lru_cache(maxsize=4)
def _set(set_index, paper):
    sel = sr.selection(set_index, paper)
    return sel, sr.weights_from(sel)


def _where(got, want):
    """where two tensors differ, for the failure message: count, channels, and the first few (image, row, column, channel)"""
    bad = np.argwhere(np.asarray(got, np.float64) != np.asarray(want, np.float64))
    return "%d of %d elements; channels %s; rows %d..%d, columns %d..%d; first %s" % (
        len(bad), np.asarray(want).size, np.unique(bad[:, 3])[:12].tolist(), bad[:, 1].min(), bad[:, 1].max(), bad[:, 2].min(), bad[:, 2].max(),
        [(tuple(int(v) for v in i), float(got[tuple(i)]), float(np.asarray(want)[tuple(i)])) for i in bad[:4]])


def _bone_bounds(feat, prec):
    """layer_ref's bound on the bone columns: y = sqrt(dx^2 + dy^2 + dz^2) in float64 from the device's stored deltas, n = BONE_N"""
    d = feat[..., 128:191].astype(np.float64)
    y = np.sqrt(d[..., 0:21] ** 2 + d[..., 21:42] ** 2 + d[..., 42:63] ** 2)
    r = dict(y=y, A=y, dot=np.zeros_like(y), K=np.zeros(21), epi=np.full(21, float(layer_ref.BONE_N)), cal_n=np.full(21, float(layer_ref.BONE_N)))
    return y, (layer_ref_f16.bounds(r, True) if prec == "fp16" else layer_ref.bounds(r, prec == "bf16"))


def _gate(cid, acts, sel, table, prec, batch):
    """every tensor of `acts` but the input against the rule on the device's own tensors.  Returns (tensors, elements, bone elements)."""
    assert np.array_equal(acts["input"], sr.round_elem(batch, prec)), (cid, "input")
    memo, done, n_exact, n_bone = {}, [], 0, 0
    for name in table:
        if name == "input" or name not in acts:
            continue
        got = acts[name]
        want = sr.expected(name, acts, sel, table, prec, memo)
        assert got.shape == want.shape, (cid, name, got.shape, want.shape)
        if name == FEAT:
            y, (rig, cal) = _bone_bounds(got, prec)
            dev = np.abs(got[..., sr.BONE].astype(np.float64) - y)
            assert np.all(dev <= rig) and np.all(dev <= cal), (cid, name, "bone columns", float((dev / cal).max()))
            got, want = got[..., :sr.BONE.start], want[..., :sr.BONE.start]
            n_bone += y.size
        if not np.array_equal(got, want):
            pytest.fail("%s: %s differs from the rule on its own inputs %s: %s" % (cid, name, table[name][1], _where(got, want)))
        n_exact += got.size
        done.append(name)
    return done, n_exact, n_bone


def _covered(cid, launches, done, stem, pair, table):
    """every launch of the plan stores at least one compared tensor (an unknown launch form raises in launch_tensors)"""
    for ln in launches:
        ts = layer_ref.launch_tensors(ln, stem=stem and ln in ("conv1", "pool1"), pair=pair, table=table)
        assert set(ts) & set(done), (cid, ln, ts)


def _record(cid, **row):
    ROWS[cid] = row
    _log("select.json", ROWS)


def _end_to_end(cid, maps, batch, sel, table, S):
    """fp32: the final maps from the batch alone, apart from the columns that descend from a bone length"""
    keep = ~sr.bone_channels("res5c_branch2c", sel)
    for i in range(S):
        want = sr.chain(batch[i:i + 1], sel, table)["res5c_branch2c"]
        if not np.array_equal(maps[i:i + 1][..., keep], want[..., keep]):
            pytest.fail("%s: final maps of image %d differ from the chain: %s" % (cid, i, _where(maps[i:i + 1][..., keep], want[..., keep])))
    return int(keep.sum())


@pytest.mark.parametrize("cid,prec,S,set_index,paper,env", LAYER_CONFIGS, ids=[c[0] for c in LAYER_CONFIGS])
def test_every_tensor_of_a_per_layer_plan_equals_the_rule(monkeypatch, cid, prec, S, set_index, paper, env):
    sel, w = _set(set_index, paper)
    table = TABLES[paper]
    batch = _batch(cid, set_index, S)
    h = _with_env(monkeypatch, env, SCALES[S], w, precision=_prec(prec), keep_activations=True, paper_res2c=paper)
    try:
        launches = [L["name"] for L in h.layers()]
        out = h.forward(batch)
        acts = _read_table(h, table=table)
    finally:
        h.close()
    assert np.array_equal(out, acts["res5c_branch2c"])
    done, n_exact, n_bone = _gate(cid, acts, sel, table, prec, batch)
    assert len(done) == len(table) - 1
    _covered(cid, launches, done, False, False, table)
    cols = _end_to_end(cid, out, batch, sel, table, S) if prec == "fp32" else None
    _record(cid, kind="per-layer", prec=prec, images=S, weight_set=set_index, paper_res2c=paper, env=env, launches=launches, tensors=done,
            elements=n_exact, bone_elements=n_bone, end_to_end_columns=cols)


@pytest.mark.parametrize("cid,prec,S,set_index,paper", FUSED_CONFIGS, ids=[c[0] for c in FUSED_CONFIGS])
def test_every_stored_tensor_of_the_fused_plan_equals_the_composed_rule(monkeypatch, cid, prec, S, set_index, paper):
    sel, w = _set(set_index, paper)
    table = TABLES[paper]
    batch = _batch(cid, set_index, S)
    kw = dict(precision=_prec(prec), paper_res2c=paper)
    fused = _with_env(monkeypatch, {"VNECT_KEEP_FUSED": "1"}, SCALES[S], w, keep_activations=True, **kw)
    arena = None
    try:
        launches = [L["name"] for L in fused.layers()]
        assert any(">" in x for x in launches) and _stem_pair(launches), launches
        written = _written(launches, table)
        stored = {"input"} | {t for _, ts in written for t in ts}
        out = fused.forward(batch)
        acts = {t: fused.activation(t) for t in table if t in stored}
        arena = _handle(SCALES[S], w, **kw)
        assert [L["name"] for L in arena.layers()] == launches
        out_arena = arena.forward(batch)
    finally:
        fused.close()
        if arena is not None:
            arena.close()
    assert np.array_equal(out, acts["res5c_branch2c"])
    assert np.array_equal(out_arena, out), (cid, "arena", _where(out_arena, out))
    done, n_exact, n_bone = _gate(cid, acts, sel, table, prec, batch)
    assert set(done) == stored - {"input"}
    _covered(cid, launches, done, True, True, table)
    cols = _end_to_end(cid, out, batch, sel, table, S) if prec == "fp32" else None
    _record(cid, kind="fused", prec=prec, images=S, weight_set=set_index, paper_res2c=paper, env={"VNECT_KEEP_FUSED": "1"}, launches=launches,
            tensors=done, on_chip=[t for t in table if t not in stored], elements=n_exact, bone_elements=n_bone, end_to_end_columns=cols)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_stem_from_the_frame_stores_copies_and_maxima(monkeypatch, prec, S):
    """infer() of a frame whose long side is 368 (its squarify step is a copy) on the fused handle: the tensors the stem launch stores
    against the rule on oracle.gen_input_batch(frame) (bf16: rounded to nearest even first)"""
    import oracle
    from tests import helpers
    cid = "frame_%s_S%d" % (prec, S)
    sel, w = _set(S, False)
    table = TABLES[False]
    frame = helpers.synth_frame(77 + S, 368, 300)
    h = _with_env(monkeypatch, {"VNECT_KEEP_FUSED": "1"}, SCALES[S], w, precision=_prec(prec), keep_activations=True)
    try:
        launches = [L["name"] for L in h.layers()]
        names = layer_ref.launch_tensors("conv1", stem=True, pair=_stem_pair(launches))
        h.infer(frame, T0 + 5, T0 + 5.001)
        got = {t: h.activation(t) for t in names}
    finally:
        h.close()
    batch, _, _ = oracle.gen_input_batch(frame, SCALES[S])
    acts = {"input": sr.round_elem(batch, prec)}
    memo, n = {}, 0
    for t in names:
        want = sr.expected(t, acts, sel, table, prec, memo)
        assert want.dtype == np.float64 and (want != 0).mean() > 0.15
        if not np.array_equal(got[t], want):
            pytest.fail("%s: %s differs from the rule on the frame's input: %s" % (cid, t, _where(got[t], want)))
        n += want.size
    _record(cid, kind="stem from the frame", prec=prec, images=S, weight_set=S, paper_res2c=False, env={"VNECT_KEEP_FUSED": "1"},
            launches=launches[:3], tensors=names, elements=n, bone_elements=0, end_to_end_columns=None)
