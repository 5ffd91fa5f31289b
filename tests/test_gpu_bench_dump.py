"""GPU (MI355X): `bench.py --dump-outputs DIR` writes what the headline's LAST timed step returned, the same from run to run, and
`--steps` sets the number of timed steps the line reports; a run without `--full` is the headline of a `--full` run and nothing else."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1.0, 0.8, 0.6]
STEPS, WARMUP = 5, 3


def _run(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_PORT",
                                                             "VNECT_BENCH_BACKEND", "VNECT_BENCH_DEVICE", "VNECT_BENCH_WORKER")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[0])


def _bench(out_dir):
    return _run(["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--cpu-seconds", "0", "--no-aux", "--dump-outputs", str(out_dir)])


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path, weights):
    lines = [_bench(tmp_path / d) for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == STEPS and d["warmup"] == WARMUP
        assert d["ms_per_step"] > 0 and len(d["latency_ms"]["frames_ms"]) == STEPS
    j2a, j3a = np.load(tmp_path / "a" / "joints_2d.npy"), np.load(tmp_path / "a" / "joints_3d.npy")
    j2b, j3b = np.load(tmp_path / "b" / "joints_2d.npy"), np.load(tmp_path / "b" / "joints_3d.npy")
    assert j2a.shape == (21, 2) and j2a.dtype == np.float64 and j3a.shape == (21, 3) and j3a.dtype == np.float32
    assert np.array_equal(j2a, j2b) and np.array_equal(j3a, j3b), "two runs with the same arguments differ"

    # the same frames, weights and timestamps through a handle of its own: the dump is the joints of frame WARMUP + STEPS
    from tests import helpers
    from vnect_amd import _native
    from vnect_amd.parallel import stream_seed
    h = _native.Handle(SCALES, device=0, num_frame_slots=8, precision=_native.FP32, use_graph="auto", lanes=3)
    h.set_weights(weights)
    h.finalize()
    for k in range(8):
        h.upload_frame(k, helpers.synth_frame(stream_seed(0, k)))
    clock = 1.7e9
    for n in (WARMUP, STEPS):
        for i in range(n):
            clock += 1 / 30
            j2, j3 = h.infer_resident(i % 8, clock, clock + 1e-3)
    h.close()
    assert np.array_equal(j2, j2a) and np.array_equal(j3, j3a)


def test_plain_run_is_the_headline_of_a_full_run(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W`: set-up, warm-up, the K timed steps, the dump and the line -- none of the legs `--full`
    adds, the same joints as a `--full` run of the same arguments, and at most 30 s of the whole run outside its W + K steps."""
    common = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)]
    t0 = time.perf_counter()
    plain = _run(common + ["--dump-outputs", str(tmp_path / "plain")])
    wall = time.perf_counter() - t0
    full = _run(common + ["--full", "--cpu-seconds", "0", "--dump-outputs", str(tmp_path / "full")])
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config"):
        assert plain[k] == full[k], k
    assert abs(plain["value"] - 1e3 / plain["ms_per_step"]) <= 1e-2 * plain["value"] and len(plain["latency_ms"]["frames_ms"]) == STEPS
    legs = ("roofline", "cpu_baseline", "bf16", "fp32_split", "call_surface", "pipelined_frames_per_s_per_gpu", "n1_same_job")
    assert not [k for k in legs if k in plain] and all(k in full for k in legs)
    assert "conv_stack_ms" not in plain["per_rank"][0] and full["per_rank"][0]["conv_stack_ms"] > 0
    for name in ("joints_2d.npy", "joints_3d.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)), name
    outside = wall - (WARMUP + STEPS) * plain["ms_per_step"] * 1e-3
    assert outside < 30, "a plain run spent %.1f s outside its steps" % outside
