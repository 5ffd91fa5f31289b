"""Two video streams per launch (vnect_set_stream_batch / vnect_submit_streams): what the batched plan buys, in stream-frames/s.
The successor of tools/two_frames_per_launch.py, on the real form: the batched plan keeps every fused form at 2 S images and each stream's
joints are its own (tests/test_gpu_stream_batch.py).  One handle per precision (scales [1.0, 0.8, 0.6], three lanes, stream_batch = 2),
one process, interleaved rounds, median of 5:
  (a) single stream, synchronous frames
  (b) two streams batched, synchronous batches            (x2: stream-frames)
  (c) single stream, three frames deep on three lanes
  (d) two streams batched, three batches deep             (x2)
then the per-layer table of the batched plan beside 2 x the S-image plan (profiling twin stamps, mean of 20 frames / batches).
    python3 tools/stream_batch_rate.py > profiles/stream_batch_rate.txt"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import helpers  # noqa: E402
from vnect_amd import _native  # noqa: E402
from vnect_amd.weights import synthetic_weights  # noqa: E402

SCALES = [1.0, 0.8, 0.6]
ROUNDS = 5
clk = [1.7e9]


def tick():
    clk[0] += 1 / 30
    return clk[0]


def sync_single(h, n):
    t0 = time.perf_counter()
    for i in range(n):
        t = tick()
        h.infer_resident(i % 8, t, t + 1e-3)
    return n / (time.perf_counter() - t0)


def submit_batch(h, i):
    t = tick()
    h.submit_streams([0, 1], [(2 * i) % 8, (2 * i + 1) % 8], [t, t], [t + 1e-3, t + 1e-3])


def sync_batched(h, n):
    t0 = time.perf_counter()
    for i in range(n):
        submit_batch(h, i)
        h.collect_stream()
        h.collect_stream()
    return 2 * n / (time.perf_counter() - t0)


def deep_single(h, n, depth=3):
    t0 = time.perf_counter()
    for i in range(n):
        if i >= depth:
            h.collect()
        t = tick()
        h.submit_resident(i % 8, t, t + 1e-3)
    for _ in range(depth):
        h.collect()
    return n / (time.perf_counter() - t0)


def deep_batched(h, n, depth=3):
    t0 = time.perf_counter()
    for i in range(n):
        if i >= depth:
            h.collect_stream()
            h.collect_stream()
        submit_batch(h, i)
    for _ in range(2 * depth):
        h.collect_stream()
    return 2 * n / (time.perf_counter() - t0)


def layer_table(h, batched, n=20):
    h.set_profiling(True)
    acc = None
    for i in range(n):
        if batched:
            submit_batch(h, i)
            h.collect_stream()
            h.collect_stream()
            ls = h.batch_layers()
        else:
            t = tick()
            h.infer_resident(i % 8, t, t + 1e-3)
            ls = h.layers()
        if acc is None:
            acc = ls
        else:
            for a, l in zip(acc, ls):
                a["last_ms"] += l["last_ms"]
    h.set_profiling(False)
    for a in acc:
        a["us"] = a["last_ms"] / n * 1e3
    return acc


def run(prec_name, W):
    prec = {"fp32": _native.FP32, "bf16": _native.BF16}[prec_name]
    h = _native.Handle(SCALES, precision=prec, lanes=3, num_frame_slots=8, stream_batch=2)
    h.set_weights(W)
    h.finalize()
    for k in range(8):
        h.upload_frame(k, helpers.synth_frame(1234 + k))
    sync_single(h, 50), sync_batched(h, 25)
    res = {"a": [], "b": [], "c": [], "d": []}
    for _ in range(ROUNDS):
        res["a"].append(sync_single(h, 300))
        res["b"].append(sync_batched(h, 150))
        res["c"].append(deep_single(h, 300))
        res["d"].append(deep_batched(h, 150))
    med = {k: float(np.median(v)) for k, v in res.items()}
    print("%s, scales %s, stream-frames/s (median of %d interleaved rounds; min - max):" % (prec_name, SCALES, ROUNDS))
    for k, what in (("a", "single stream, synchronous"), ("b", "two streams batched, synchronous"),
                    ("c", "single stream, three deep on three lanes"), ("d", "two streams batched, three batches deep")):
        print("  (%s) %-44s %8.1f   (%.1f - %.1f)" % (k, what, med[k], min(res[k]), max(res[k])))
    print("  batched synchronous vs single synchronous: %.3fx;  batched three deep vs three lanes: %.3fx"
          % (med["b"] / med["a"], med["d"] / med["c"]))
    single, batched = layer_table(h, False), layer_table(h, True)
    print("\n  %-44s %7s %5s %5s %9s %9s %7s" % ("layer (same in both plans)", "tile", "WGs", "2xWGs", "2 x S us", "batch us", "ratio"))
    tot1 = tot2 = 0.0
    for a, b in zip(single, batched):
        if a["us"] <= 0 and b["us"] <= 0:
            continue
        tot1 += 2 * a["us"]
        tot2 += b["us"]
        name = "conv1 = stem from the frame" if a["name"] == "conv1" else a["name"]
        print("  %-44s %7s %5d %5d %9.1f %9.1f %7.2f" % (name[:44], "%dx%d" % (a["tile_m"], a["tile_n"]), a["workgroups"], b["workgroups"],
                                                     2 * a["us"], b["us"], b["us"] / (2 * a["us"]) if a["us"] > 0 else float("nan")))
    print("  %-44s %7s %5s %5s %9.1f %9.1f %7.2f" % ("sum of the conv launches", "", "", "", tot1, tot2, tot2 / tot1 if tot1 else float("nan")))
    print()
    h.close()


def main():
    W = synthetic_weights()
    print(_native.build_info()["text"])
    for prec_name in (sys.argv[1:] or ["bf16", "fp32"]):
        run(prec_name, W)


if __name__ == "__main__":
    main()
