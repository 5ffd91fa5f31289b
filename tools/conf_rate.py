"""What the per-joint confidence and the loss rule cost the tracked loops (CONFIDENCE.md), in ONE process: tools/track_rate.py's
  configurations -- one video at ahead 1 on a lanes=1 handle, three videos on a lanes=3 handle, frames in the pinned buffers, planted
  weights, fp32 and bf16, 640 x 480 -- with the rule off and on (hold, with a threshold every frame passes, so the box sequence is the
  same), interleaved rounds, each variant run twice per round (A/A), frames/s.  Run from a tree without the rule (the parent commit),
  it measures the `off` variants alone: the two outputs side by side are the comparison against the parent.
    python3 tools/conf_rate.py >> profiles/confidence_rate.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import track_rate as tr  # noqa: E402

from tests import planted  # noqa: E402
from vnect_amd import VNectEstimator, _native, runner  # noqa: E402

ROUNDS, N1, N3 = 3, 200, 100
HAS_RULE = hasattr(runner, "lost_rule")
RULE = (0.0, 1, "hold")


def one(est, bufs, n, clock, lost):
    est.reset()
    kw = {"lost": lost} if lost else {}
    ts = clock.take(n)
    t0 = tr.time.perf_counter()
    for _ in runner.track_on_device(est, (bufs[k % 2] for k in range(n)), timestamps=ts, ahead=1, **kw):
        pass
    return n / (tr.time.perf_counter() - t0)


def three(est, bufs, n, clock, lost):
    est.reset()
    kw = {"lost": lost} if lost else {}
    tss = [clock.take(n) for _ in range(3)]
    vids = [(bufs[(3 * k + i) % 2] for k in range(n)) for i in range(3)]
    t0 = tr.time.perf_counter()
    for _ in runner.track_many_on_device(est, vids, timestamps=tss, ahead=2, **kw):
        pass
    return 3 * n / (tr.time.perf_counter() - t0)


def main():
    w = planted.weights()
    print(_native.build_info()["text"])
    print("loss rule in this tree:", HAS_RULE)
    clock = tr.Clock()
    H, W = 480, 640
    for prec in tr.PRECS:
        e1 = VNectEstimator(weights=w, precision=prec, verbose=False)
        e3 = VNectEstimator(weights=w, precision=prec, verbose=False, lanes=3)
        imgs = tr.scenes(H, W)
        b1, b3 = tr.pinned(e1, H, W, imgs), tr.pinned(e3, H, W, imgs)
        variants = [("one video ahead=1, rule off", lambda: one(e1, b1, N1, clock, None)),
                    ("three videos, rule off", lambda: three(e3, b3, N3, clock, None))]
        if HAS_RULE:
            variants += [("one video ahead=1, rule on", lambda: one(e1, b1, N1, clock, RULE)),
                         ("three videos, rule on", lambda: three(e3, b3, N3, clock, RULE))]
        for _, fn in variants:
            fn()
        res = {name: ([], []) for name, _ in variants}
        for _ in range(ROUNDS):
            for rep in range(2):
                for name, fn in variants:
                    res[name][rep].append(fn())
        print("\n%s, %d x %d, frames/s, median of %d interleaved rounds: first run | second run of the same variant (A/A)" % (prec, W, H, ROUNDS))
        for name, _ in variants:
            a, b = res[name]
            print("  %-30s %8.1f (%.1f - %.1f) | %8.1f (%.1f - %.1f)" % (name, np.median(a), min(a), max(a), np.median(b), min(b), max(b)))
        e1.close()
        e3.close()


if __name__ == "__main__":
    main()
