"""The fp16 precision (VNECT_FP16) against bf16 and fp32 in ONE process: what it costs and what it buys.
  (1) stream-frames/s, fp32 / bf16 / fp16 handles (scales [1.0, 0.8, 0.6], three lanes), interleaved rounds, median of 5:
      (a) synchronous frames, (c) three frames deep on three lanes;
  (2) per-layer kernel time of a profiled frame, fp16 against bf16 (profiling twin stamps, mean of 20 frames, vnect_get_layer_info);
  (3) final-map error against the fp32 handle, bf16 and fp16, over the nine weight sets of profiles/r06_bf16_gate_spread.txt
      (tests/weight_families.py: family) on a smooth and a noise frame -- what tests/test_gpu_fp16.py's EPS16 is set from;
  (4) the largest |activation| of every weight family (fp32 handle, every readable tensor): where fp16's range (65 504) would show first.
    python3 tools/fp16_rate.py > profiles/fp16_rate.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from stream_batch_rate import deep_single, layer_table, sync_single  # noqa: E402
from tests import helpers, layer_ref  # noqa: E402
from tests.weight_families import family as variant  # noqa: E402
from vnect_amd import _native  # noqa: E402
from vnect_amd.weights import MASTER_SEED, synthetic_weights  # noqa: E402

SCALES = [1.0, 0.8, 0.6]
ROUNDS = 5
PRECS = (("fp32", _native.FP32), ("bf16", _native.BF16), ("fp16", _native.FP16))
SETS = [("default", MASTER_SEED), ("default", 1), ("default", 2), ("default", 3), ("channel_scales", 11), ("channel_scales", 12),
        ("heavy_tails", 21), ("heavy_tails", 22), ("big_biases", 31)]


def _handle(prec, w, **kw):
    h = _native.Handle(SCALES, precision=prec, **kw)
    h.set_weights(w)
    h.finalize()
    return h


def rates(W):
    hs = {}
    for name, p in PRECS:
        hs[name] = _handle(p, W, lanes=3, num_frame_slots=8)
        for k in range(8):
            hs[name].upload_frame(k, helpers.synth_frame(1234 + k))
        sync_single(hs[name], 50)
    res = {(n, c): [] for n, _ in PRECS for c in "ac"}
    for _ in range(ROUNDS):
        for name, _ in PRECS:
            res[(name, "a")].append(sync_single(hs[name], 300))
            res[(name, "c")].append(deep_single(hs[name], 300))
    med = {k: float(np.median(v)) for k, v in res.items()}
    print("(1) stream-frames/s, scales %s, one process, median of %d interleaved rounds (min - max)" % (SCALES, ROUNDS))
    for c, what in (("a", "synchronous"), ("c", "three deep on three lanes")):
        for name, _ in PRECS:
            print("  %-28s %-5s %8.1f   (%.1f - %.1f)" % (what, name, med[(name, c)], min(res[(name, c)]), max(res[(name, c)])))
        print("  %-28s fp16 / bf16 = %.3f, fp16 / fp32 = %.3f" % (what, med[("fp16", c)] / med[("bf16", c)], med[("fp16", c)] / med[("fp32", c)]))
    tb, th = layer_table(hs["bf16"], False), layer_table(hs["fp16"], False)
    print("\n(2) per-layer kernel time of a profiled frame (mean of 20), fp16 against bf16")
    print("  %-44s %7s %5s %9s %9s %7s" % ("layer", "tile", "WGs", "bf16 us", "fp16 us", "ratio"))
    t1 = t2 = 0.0
    for a, b in zip(tb, th):
        assert a["name"] == b["name"]
        if a["us"] <= 0 and b["us"] <= 0:
            continue
        t1, t2 = t1 + a["us"], t2 + b["us"]
        print("  %-44s %7s %5d %9.1f %9.1f %7.3f" % (a["name"][:44], "%dx%d" % (a["tile_m"], a["tile_n"]), a["workgroups"], a["us"], b["us"],
                                                   b["us"] / a["us"] if a["us"] > 0 else float("nan")))
    print("  %-44s %7s %5s %9.1f %9.1f %7.3f" % ("sum of the conv launches", "", "", t1, t2, t2 / t1))
    for h in hs.values():
        h.close()


def errors():
    import oracle
    frames = [helpers.synth_frame(1234, smooth=True), helpers.synth_frame(77, smooth=False)]
    batches = [oracle.gen_input_batch(f, SCALES)[0] for f in frames]
    print("\n(3) final-map error against the fp32 handle, of the fp32 map maximum (weight sets of profiles/r06_bf16_gate_spread.txt)")
    worst = {"bf16": 0.0, "fp16": 0.0}
    ratios = []
    for kind, seed in SETS:
        w = variant(kind, seed)
        hs = {name: _handle(p, w) for name, p in PRECS}
        row = []
        for b in batches:
            f = hs["fp32"].forward(b)
            m = float(np.abs(f).max())
            eb, eh = (float(np.abs(hs[n].forward(b) - f).max()) / m for n in ("bf16", "fp16"))
            worst["bf16"], worst["fp16"] = max(worst["bf16"], eb), max(worst["fp16"], eh)
            ratios.append(eh / eb)
            row += [eb, eh]
        for h in hs.values():
            h.close()
        print("  %-15s seed %-9d  smooth: bf16 %.2e fp16 %.2e   noise: bf16 %.2e fp16 %.2e" % (kind, seed, *row), flush=True)
    print("  largest over %d sets x 2 frames: bf16 %.2e, fp16 %.2e; fp16 / bf16 per frame %.3f - %.3f" % (
        len(SETS), worst["bf16"], worst["fp16"], min(ratios), max(ratios)))
    print("  tests/test_gpu_fp16.py gates fp16 at EPS16 = 7.5e-3: %.1fx over the largest fp16 error here (bf16: 3e-2, %.1fx over its own)"
          % (7.5e-3 / worst["fp16"], 3e-2 / worst["bf16"]))


def ranges():
    import oracle
    b = oracle.gen_input_batch(helpers.synth_frame(1234, smooth=True), SCALES)[0]
    print("\n(4) largest |activation| per weight family (fp32 handle, every readable tensor, smooth frame); fp16 holds up to 65 504")
    for kind, seed in (("default", MASTER_SEED), ("channel_scales", 12), ("heavy_tails", 22), ("big_biases", 31)):
        h = _handle(_native.FP32, variant(kind, seed), keep_activations=True)
        h.forward(b)
        top = max(((float(np.abs(h.activation(n)).max()), n) for n in layer_ref.TABLE if n != "input"))
        h.close()
        print("  %-15s seed %-9d  %8.2f  (%s)" % (kind, seed, top[0], top[1]))


def main():
    print(_native.build_info()["text"])
    rates(synthetic_weights())
    errors()
    ranges()


if __name__ == "__main__":
    main()
