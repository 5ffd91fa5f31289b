"""How far does the bf16 path's map error move with the WEIGHTS?  The gate of tests/test_gpu_bf16.py (final maps <= 3e-2 of the map maximum) was
calibrated on ONE set of seeded synthetic weights (measured 1.7-2.3e-2); nobody here holds trained ones.  This probe runs the same comparison -- the
bf16 handle's final maps against the fp32 handle's (itself 3e-6 from the CPU oracle) -- over other seeds and over weight sets bent towards what a
trained network looks like: per-output-channel scales spread log-uniformly over x[1/4, 4] (folded-BN-like), heavier-tailed weights, larger biases.
Prints max |bf16 - fp32| / max |fp32| per weight set and frame; INTEGRATION.md quotes the range.  GPU box, ~1 minute."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import helpers
from tests.weight_families import family as variant  # the one definition of the weight families
from vnect_amd import _native
from vnect_amd.weights import MASTER_SEED

SCALES = [1.0, 0.8, 0.6]


def maps(handle, batch):
    return handle.forward(batch)


def main():
    import oracle  # noqa: E402  (pre-processing only: the batch both handles are fed)
    frames = [helpers.synth_frame(1234, smooth=True), helpers.synth_frame(77, smooth=False)]
    batches = [oracle.gen_input_batch(f, SCALES)[0] for f in frames]
    rows = []
    for kind, seed in [("default", MASTER_SEED), ("default", 1), ("default", 2), ("default", 3), ("channel_scales", 11), ("channel_scales", 12),
                       ("heavy_tails", 21), ("heavy_tails", 22), ("big_biases", 31)]:
        w = variant(kind, seed)
        hs = {}
        for prec in (_native.FP32, _native.BF16):
            h = _native.Handle(SCALES, precision=prec)
            h.set_weights(w); h.finalize()
            hs[prec] = h
        errs = []
        for b in batches:
            f, g = hs[_native.FP32].forward(b), hs[_native.BF16].forward(b)
            m = float(np.abs(f).max())
            errs.append(float(np.abs(g - f).max() / m) if np.isfinite(m) and m > 0 else float("nan"))
            hm = float(np.abs(g[..., :21] - f[..., :21]).max() / max(float(np.abs(f[..., :21]).max()), 1e-30))
            errs.append(hm)
        for h in hs.values():
            h.close()
        rows.append((kind, seed, errs))
        print("%-15s seed %-9d  all maps: smooth %.2e  noise %.2e   heat-maps only: smooth %.2e  noise %.2e" % (kind, seed, errs[0], errs[2], errs[1], errs[3]), flush=True)
    allmax = max(max(e[0], e[2]) for _, _, e in rows)
    print("largest final-map error over %d weight sets x 2 frames: %.2e of the map maximum (the gate is 3e-2)" % (len(rows), allmax))


if __name__ == "__main__":
    main()
