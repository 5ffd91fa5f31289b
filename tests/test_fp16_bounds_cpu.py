"""The fp16 per-element gate of tests/layer_ref_f16.py is not vacuous (CPU, no GPU needed): the counterpart of
tests/test_layer_bounds_cpu.py.  A CPU stand-in computes every tensor of a keep_activations plan the way the HIP launches of an fp16
handle do -- torch float32 accumulation, fp16 round-to-nearest-even at the kernels' rounding points (every stored activation but the fp32
final maps), the BN fold, the bone lengths from the stored deltas -- and must pass the gate on every tensor; each planted fault must fail
it on exactly the tensor it was planted in.  One scale at 368 x 368, synthetic weights."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers, layer_ref, layer_ref_f16
from tests.layer_ref import TABLE

# fault -> tensor: (a) a round-toward-zero store (what v_cvt_pkrtz_f16_f32 would do), (b) bf16 rounding in place of fp16 on one tensor,
# (c) a block output rounded before its shortcut add and again after it, (d) the bias lost on 4 channels
FAULTS = {"rtz": "res4b_branch2a", "bf16": "res3c_branch2b", "double_round": "res3c", "bias": "res3b_branch2a"}
# Two fp16 candidates for the family faults of tests/test_weight_families_cpu.py are NOT planted.  A store that flushes subnormal results
# (below 2^-14) to 0 is caught under the default weights already: planted in res2a_branch1 it fails that tensor at a calibrated ratio of
# 119, in res3c (58 subnormal results) at 19.8.  A layer that reads the subnormal elements of its input as 0 is caught under no family:
# on res2a_branch2b, res2a and res2b_branch2a under f16_range the products it loses, below 2^-14 |w|, stay inside every element's bound.


def _rne(t):
    return t.to(torch.float16).to(torch.float32)


def _rtz(t):
    r = _rne(t)
    return torch.where(r.abs() > t.abs(), torch.nextafter(r.to(torch.float16), torch.zeros_like(r, dtype=torch.float16)).to(torch.float32), r)


def device_forward(weights, batch, fault=None, table=TABLE):
    """Every tensor of `table` (layer_ref.TABLE or TABLE_PAPER) as an fp16 handle computes it; fault: a key of FAULTS."""
    lw = layer_ref_f16.layer_weights(weights)
    target = FAULTS.get(fault)
    T = {}

    def f32(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32))

    def store(name, v, f32_out=False):
        if not f32_out:
            if name == target and fault == "rtz":
                v = _rtz(v)
            elif name == target and fault == "bf16":
                v = v.to(torch.bfloat16).to(torch.float32)
            else:
                v = _rne(v)
        T[name] = v

    for name, (op, ins, p) in table.items():
        if op == "input":
            T[name] = _rne(f32(batch).permute(0, 3, 1, 2))
        elif op == "pool":
            T[name] = layer_ref.maxpool_same(T[ins[0]])
        elif op in ("conv", "head"):
            x = T[ins[0]]
            if op == "head":
                w, b, k, stride, relu = lw["res5c_branch2c/kernel"], np.zeros(84, np.float32), 1, 1, False
            else:
                w, b = lw[p["scope"] + "/weights"], np.array(lw[p["scope"] + "/biases"], np.float32)
                k, stride, relu = p["k"], p["stride"], p["relu"]
            if fault == "bias" and name == target:
                b = b.copy()
                b[:4] = 0
            xin = layer_ref._same(x, k, stride) if k > 1 else x
            v = F.conv2d(xin, f32(w).permute(3, 2, 0, 1), stride=stride) + f32(b).view(1, -1, 1, 1)
            if len(ins) > 1:
                if fault == "double_round" and name == target:
                    v = _rne(v)
                v = v + T[ins[1]]
            if relu:
                v = F.relu(v)
            store(name, v, f32_out=op == "head")
        elif op == "feat":
            x = T[ins[0]]
            d2 = F.conv_transpose2d(x, f32(lw["res5c_branch2a/kernel"]).permute(3, 2, 0, 1), stride=2, padding=1)
            d1 = F.conv_transpose2d(x, f32(lw["res5c_branch1a/kernel"]).permute(3, 2, 0, 1), stride=2, padding=1)
            bias, scale, shift = (f32(v).view(1, -1, 1, 1) for v in layer_ref.fold_bn(lw))
            bn = F.relu((d2 + bias) * scale + shift)
            deltas = _rne(d1)
            dx, dy, dz = deltas[:, 0:21], deltas[:, 21:42], deltas[:, 42:63]
            bone = torch.sqrt((dx * dx + dy * dy) + dz * dz)
            store(name, torch.cat([bn, d1, bone], 1))
    return {k: v.permute(0, 2, 3, 1).contiguous().numpy() for k, v in T.items()}


@pytest.fixture(scope="module")
def batch():
    frame = helpers.synth_frame(1234, smooth=True).astype(np.float32)
    return (frame / 255.0 - 0.4)[None]


def _failing(rows):
    return sorted(r["tensor"] for r in rows if not r["ok"])


def test_clean_fp16_stand_in_passes_every_tensor(weights, batch):
    rows = layer_ref_f16.check_all(device_forward(weights, batch), weights, batch)
    worst = max(rows, key=lambda r: r["cal"])
    print("fp16 stand-in: worst calibrated %.3g (%s), lowest match %.5f" % (worst["cal"], worst["tensor"],
                                                                          min(r["match"] for r in rows if r["match"] is not None)))
    assert len(rows) == len(TABLE)
    assert _failing(rows) == [], [r for r in rows if not r["ok"]][:3]


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fp16_fault_fails_the_gate_on_its_tensor(weights, batch, fault):
    rows = layer_ref_f16.check_all(device_forward(weights, batch, fault), weights, batch)
    assert _failing(rows) == [FAULTS[fault]], [r for r in rows if not r["ok"]][:3]
    row = next(r for r in rows if r["tensor"] == FAULTS[fault])
    print(fault, row)
    if fault in ("rtz", "bf16"):
        assert row["match"] < 0.75
