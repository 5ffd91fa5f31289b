"""The per-element gate of tests/layer_ref.py for fp16 handles (VNECT_FP16; test helper, no GPU).

Same references (layer_ref.reference: float64 from the device's own input tensors), same fp32 accumulation term E in both tiers
(rigorous gamma(n), calibrated C_CAL = 28), with fp16's output rounding in place of bf16's: a launch computes v with |v - y| <= E in
fp32, applies ReLU and rounds once to fp16 (round to nearest even, unit roundoff uh = 2^-11; below 2^-14 the spacing is 2^-24, so the
absolute error of a subnormal result is at most half of it, 2^-25):
    d <= uh |y| + (1 + uh) E + 2^-25.
Sharpness: over elements with y != 0, the fraction where gpu == RNE_fp16(float32(y)) must reach MATCH_FLOOR_F16.  bf16's floor (0.999)
does not carry over: fp16's half ulp is 8x closer to the fp32 accumulation error, so a correct launch sits on the other side of a rounding
midpoint 8x as often -- the CPU stand-in of tests/test_fp16_bounds_cpu.py measures 0.9962 at the lowest -- while a truncating or bf16-rounding
store lands near 1/2.
Overflow (FP16.md): the store rounds to nearest even, so a result of magnitude 65 520 or more is stored as +-inf.  check_overflow gates a
tensor that holds such results: with b the larger of the two tiers' bounds, elements with |y| > 65 520 + b must be +-inf of y's sign,
elements with |y| < 65 520 - b finite and within both bounds; the band between, where a correct launch may land on either side, is left out.
"""
import numpy as np

from tests import layer_ref
from tests.layer_ref import TABLE, _nhwc, _ratio, _t64, maxpool_same

UH = 2.0 ** -11
SUB = 2.0 ** -25
MATCH_FLOOR_F16 = 0.995
F16_INF = 65520.0   # the midpoint between fp16's largest finite value, 65 504, and 2^16: it and everything beyond rounds to infinity


def round_f16(a):
    """float32 -> nearest-even fp16 -> float32."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def layer_weights(weights):
    """The weights as an fp16 handle multiplies them: every conv / transposed-conv weight rounded to fp16 (rt_plan.cpp upload_weights);
    biases and the BN parameters stay fp32."""
    return {k: (round_f16(v) if k.endswith("/weights") or k.endswith("/kernel") else v) for k, v in weights.items()}


def bounds(r, f16_out):
    """(rigorous, calibrated) per-element bounds of a reference r."""
    rig, cal = layer_ref.bounds(r, False)
    if not f16_out:
        return [rig, cal]
    y = np.abs(r["y"])
    return [UH * y + (1.0 + UH) * E + SUB for E in (rig, cal)]


def check_tensor(name, gpu, r, f16_out):
    if "exact" in r:
        eq = bool(np.array_equal(gpu, r["exact"]))
        return dict(tensor=name, rig=0.0 if eq else float("inf"), cal=0.0 if eq else float("inf"), match=None, ok=eq)
    y = r["y"]
    assert gpu.shape == y.shape, (name, gpu.shape, y.shape)
    d = np.abs(gpu.astype(np.float64) - y)
    rig_b, cal_b = bounds(r, f16_out)
    rig, cal = _ratio(d, rig_b), _ratio(d, cal_b)
    match = None
    if f16_out:
        nz = y != 0
        match = float(np.mean(gpu[nz] == round_f16(y[nz].astype(np.float32)))) if nz.any() else 1.0
    ok = rig <= 1.0 and cal <= 1.0 and (match is None or match >= MATCH_FLOOR_F16)
    return dict(tensor=name, rig=rig, cal=cal, match=match, ok=ok)


def check_overflow(name, gpu, r):
    """The overflow rule on one tensor of an fp16 handle (reference r): counts of the elements beyond, inside and below the band around
    65 520, of those above 2^15, and whether the rule holds (ok)."""
    y = r["y"]
    assert gpu.shape == y.shape, (name, gpu.shape, y.shape)
    rig_b, cal_b = bounds(r, True)
    b = np.maximum(rig_b, cal_b)
    over, under = np.abs(y) > F16_INF + b, np.abs(y) < F16_INF - b
    with np.errstate(invalid="ignore"):
        d = np.abs(gpu.astype(np.float64) - y)
    inf_ok = bool(np.array_equal(gpu[over], np.where(y[over] > 0, np.inf, -np.inf).astype(np.float32)))
    finite_ok = bool(np.all(np.isfinite(gpu[under])))
    rig, cal = (_ratio(d[under], x[under]) for x in (rig_b, cal_b)) if finite_ok else (float("inf"), float("inf"))
    return dict(tensor=name, over=int(over.sum()), band=int((~over & ~under).sum()), large=int((np.abs(y) > 2.0 ** 15).sum()),
                stored_inf=int(np.isinf(gpu).sum()), inf_ok=inf_ok, finite_ok=finite_ok, rig=rig, cal=cal,
                ok=inf_ok and finite_ok and rig <= 1.0 and cal <= 1.0)


def check_all(acts, weights, batch, stem=False, table=TABLE):
    """Gate every tensor of `table` (layer_ref.TABLE or TABLE_PAPER) present in `acts` (name -> NHWC float32 read from an fp16 handle); the input must be the batch's fp16
    rounding, the final maps (res5c_branch2c) are fp32.  Returns the rows, input first."""
    lw = layer_weights(weights)
    rows = []
    eq = bool(np.array_equal(acts["input"], round_f16(batch)))
    rows.append(dict(tensor="input", rig=0.0 if eq else float("inf"), cal=0.0 if eq else float("inf"), match=None, ok=eq))
    for name in table:
        if name == "input" or name not in acts or (stem and name == "conv1"):
            continue
        f16_out = name != "res5c_branch2c"
        if stem and name == "pool1":
            r, y = layer_ref.stem_pool_reference(acts, lw)
            rig_b, cal_b = (_nhwc(maxpool_same(_t64(b))) for b in bounds(r, True))
            gpu = acts["pool1"]
            d = np.abs(gpu.astype(np.float64) - y)
            nz = y != 0
            match = float(np.mean(gpu[nz] == round_f16(y[nz].astype(np.float32))))
            rig, cal = _ratio(d, rig_b), _ratio(d, cal_b)
            rows.append(dict(tensor="pool1", rig=rig, cal=cal, match=match,
                             ok=rig <= 1.0 and cal <= 1.0 and match >= MATCH_FLOOR_F16))
            continue
        rows.append(check_tensor(name, acts[name], layer_ref.reference(name, acts, lw, table), f16_out))
    return rows
