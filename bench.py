"""bench.py -- frames/s of 368x368, 3-scale VNect inference on N MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N>1: one rank per GPU.  Under a launcher (torch.distributed.run sets RANK / WORLD_SIZE) this process IS a rank; started bare
(`python bench.py --gpus N`, no WORLD_SIZE) it spawns its N rank processes itself -- children with RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* set, started BEFORE this process touches the GPU; it relays rank 0's JSON line and exits with the
children's worst return code (never an exec of a process that has initialised HIP).

A step is one pass of the hot path (VNectEstimator.__call__, /root/reference/src/estimator.py:97-142) over one
synthetic 368x368 BGR frame at scales [1.0, 0.8, 0.6], fp32 (BASELINE.json configs[1]).  Frames are resident in
HBM before the timed region (the host-to-device copy of a frame is OUTSIDE it; the PCIe-inclusive rate is carried
beside `value`); each step ends with the 21x2 + 21x3 joints back on the host (synchronous, as the reference's
tracking loop consumes them).  N>1 = N independent streams, one per GPU (weak scaling, no collective on the data
path; BASELINE.json configs[4]); `--pyramid` = ONE stream, one scale per GPU (configs[3]).  Weights are seeded
synthetic (none ship with the reference).  Rank 0 prints ONE JSON line.

A plain run does only what that line's headline needs: it sets up, warms up, times the K steps, writes --dump-outputs and prints
the line.  `--full` adds everything else behind the headline's timed region: the auxiliary legs (PCIe-inclusive, frames in flight,
two and three streams per GPU), the bf16 (configs[2]) and split-product legs at N=1, the live roofline and per-rank device figures
of the profiling twin, the same-job N = 1 reference at N>1 and the CPU baselines.
"""
import argparse
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SCALES = [1.0, 0.8, 0.6]
PEAK_FP32_MFMA = 157.3         # TFLOP/s, MI355X_MICROARCH.md chip table (v_mfma_f32_32x32x2_f32)
PEAK_BF16_MFMA = 2500.0        # TFLOP/s dense bf16 (same table; the 2:1-sparsity figure is not used)
PEAK_HBM = 8000.0              # GB/s
# bf16 conv stack, algorithmic bytes per frame: bf16 weights 29.2 MB + every layer output written once and read once
# (2 x 3 images x 58.7 MB of bf16 activations)
BF16_BYTES_PER_FRAME = 29.2e6 + 2 * 3 * 58.7e6
# committed rocprofv3 summaries are named profiles/rNN<prefix>_{kernel_stats.csv,conv_roofline.json,traffic.json} (tools/profile_round.sh)
PROFILE_PREFIX = {"fp32": "", "bf16": "_bf16", "fp32_split": "_split"}
DUMP_T0 = 1.6e9                # first timestamp of the --dump-joints frames (fresh filter banks, so any value serves)


def cpu_baseline(weights, budget_s):
    """The CPU oracle (a port of the reference path; TF1 itself cannot run here) on this box's host cores."""
    import oracle
    from tests import helpers
    est = oracle.OracleEstimator(weights=weights, scales=SCALES)
    frames = [helpers.synth_frame(1234 + k) for k in range(4)]
    # The port's blocked SGEMM stops scaling at ~16 threads on the 23x23 / 46x46 layers (measured on the GPU box:
    # 8 / 16 / 32 / 64 / 128 threads -> 3.6 / 4.0 / 3.7 / 2.9 / 1.6 frames/s), so it runs on at most 16 and says so.
    L = oracle.lib()
    L.vo_set_threads.argtypes = [__import__("ctypes").c_int]
    L.vo_set_threads(min(16, len(os.sched_getaffinity(0))))
    est(frames[0], 1.0, 1.0)  # warm-up (page-in, thread pool)
    n, t0 = 0, time.perf_counter()
    while True:
        est(frames[n % 4], 2.0 + n / 30, 2.0 + n / 30)
        n += 1
        dt = time.perf_counter() - t0
        if (dt >= budget_s and n >= 3) or n >= 400:
            break
    cores = oracle.lib().vo_sgemm_threads()
    return {"value": round(n / dt, 3), "unit": "frames/s", "cores": cores, "kind": "port",
            "implementation": "oracle/ (C + OpenMP restatement of the whole path, blocked AVX SGEMM)",
            "sample": "%d frames of the same workload in %.1f s (C/OpenMP fp32 oracle, AVX2/AVX-512 SGEMM, threads capped at 16 "
                      "of %d host cores: more are slower)" % (n, dt, len(os.sched_getaffinity(0)))}


def cpu_framework_baseline(weights, budget_s):
    """A framework-grade stand-in for the reference's TF-CPU path (TF1 cannot run here): the same frames through
    torch-CPU (oneDNN) for the network, fp32, with the oracle's pre- and post-processing around it.  Reported beside
    `cpu_baseline`, labelled as a proxy; never a target."""
    import torch
    import oracle
    from tests import helpers, torch_net
    ncores = len(os.sched_getaffinity(0))
    est = oracle.OracleEstimator(weights=weights, scales=SCALES)
    frames = [helpers.synth_frame(1234 + k) for k in range(4)]

    def frame(k, t):
        batch, scaler, off = oracle.gen_input_batch(frames[k % 4], SCALES)
        with torch.inference_mode():
            maps = torch_net.forward(weights, batch, dtype=torch.float32).numpy()
        return est.postprocess(maps, t, t, scaler, off[0], off[1])

    # the best this host can do, not an assumed cap: a sweep over the intra-op thread count -- one warm-up frame, then 20 frames per
    # setting (fewer only where a setting is so slow that 20 frames would take more than 4 s: it has lost by then) -- and the sample
    # on the fastest, as the MEDIAN of five windows with their spread beside it (round 4's two-frame sweep and single window
    # disagreed with each other by up to 2x)
    sweep, clk = {}, 1.0
    for th in sorted({t for t in (8, 16, 32, 64, 128, ncores) if t <= ncores}):
        if sweep and (th > 128 or sweep[max(sweep)] < 0.5 * max(sweep.values())):
            break  # past the knee: on the GPU boxes (a 16-core share of 256 visible cores) 128 threads run at 2 frames/s and 256 at 0.03
        torch.set_num_threads(th)
        clk += 1
        frame(0, clk)
        k, t0 = 0, time.perf_counter()
        while k < 20 and (k < 3 or time.perf_counter() - t0 < 4.0):
            clk += 1
            frame(k, clk)
            k += 1
        sweep[th] = round(k / (time.perf_counter() - t0), 2)
    threads = max(sweep, key=sweep.get)
    torch.set_num_threads(threads)
    frame(0, clk + 1)
    windows, n, t_all = [], 0, time.perf_counter()
    for w in range(5):
        k, t0 = 0, time.perf_counter()
        while (time.perf_counter() - t0 < budget_s / 5 or k < 3) and k < 80:
            frame(n, clk + 2 + n / 30)
            n += 1
            k += 1
        windows.append(k / (time.perf_counter() - t0))
    dt = time.perf_counter() - t_all
    windows.sort()
    return {"value": round(windows[2], 3), "unit": "frames/s", "cores": threads, "kind": "port",
            "implementation": "torch-CPU (oneDNN) fp32 restatement of the network (tests/torch_net.py) + the oracle's pre / post-processing",
            "thread_sweep_frames_per_s": sweep, "windows_frames_per_s": [round(x, 2) for x in windows],
            "sample": "%d frames of the same workload in %.1f s on %d threads of %d host cores, median of 5 windows (min %.2f, max %.2f; torch %s; "
                      "thread sweep, 20 frames per setting: %s)" % (n, dt, threads, ncores, windows[0], windows[-1], torch.__version__, sweep)}


def committed(pattern, key):
    """A number from the newest committed profile summary matching profiles/r??<pattern> (rocprofv3 evidence of an earlier run
    of this command, named per round).  Returns (value, file name) or (None, None): the live line never pretends these are
    measurements of the present run."""
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]" + pattern)):
        m = re.match(r"r(\d\d)", os.path.basename(f))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), f)
    if not best:
        return None, None
    try:
        return json.load(open(best[1])).get(key), os.path.basename(best[1])
    except Exception:
        return None, None


def roofline(tim, nprof, precision, images_frac=1.0):
    """`roofline` object of the dominant kernel (vnect::conv_stream_kernel, the whole conv stack) from the live profiling twin:
    every conv kernel stamps its first-wave start and last-wave end with the 100 MHz device clock; a launch's duration is the
    SLOT it occupies on the stream (its start to the start of the kernel behind it) -- what rocprofv3 reports per kernel
    (dispatch -> completion, durations abut) and what a launch costs the frame."""
    conv_ms = tim["conv_slot_ms"] / nprof
    exec_ms = tim["conv_ms"] / nprof
    flops = tim["conv_flops"] * images_frac            # algorithmic FLOPs of the live launch plan (2 * MAC)
    launches = tim["conv_launches"]
    achieved = flops / (conv_ms * 1e-3) / 1e12
    # tools/profile_round.sh r02 / r02_bf16 / r03_split -> r02_traffic.json / r02_bf16_traffic.json / r03_split_traffic.json
    pre = PROFILE_PREFIX[precision]
    traffic_frame, tfile = committed("%s_traffic.json" % pre, "hbm_bytes_per_frame")
    rocprof_us, rfile = committed("%s_conv_roofline.json" % pre, "conv_avg_us_per_launch")
    rocprof_ms, _ = committed("%s_conv_roofline.json" % pre, "conv_ms_per_frame")
    rocprof_calls, _ = committed("%s_conv_roofline.json" % pre, "conv_calls_per_frame")
    peak = PEAK_BF16_MFMA if precision == "bf16" else PEAK_FP32_MFMA
    first_last = {"avg_launch_us": round(exec_ms * 1e3 / launches, 3),
                  "achieved": round(flops / (exec_ms * 1e-3) / 1e12, 3),
                  "frac": round(flops / (exec_ms * 1e-3) / 1e12 / peak, 4)}
    common = dict(
        kernel="vnect::conv_stream_kernel<BM,BN,KG,NS,%s,0> (implicit-GEMM conv on MFMA, LDS-DMA ring; some launches carry a second / third "
               "layer as tail / chain GEMMs) + vnect::stem_kernel (gen_input_batch + conv1 + pool1 + res2a's first 1x1 pair on spatial tiles): "
               "%d launches per frame" % ("true" if precision == "bf16" else "false", launches),
        launches_per_frame=launches, avg_launch_us=round(conv_ms * 1e3 / launches, 3), first_to_last_wave=first_last,
        kernel_ms_per_frame=round(conv_ms, 4), flops_per_frame=flops,
        algorithmic_per_launch=(BF16_BYTES_PER_FRAME * images_frac / launches if precision == "bf16" else flops / launches),
        conv_stack_span_ms=round(tim["net_ms"] / nprof, 4), hip_event_frame_ms=round(tim["total_ms"] / nprof, 4),
        # HBM bytes per launch from the PMC passes of tools/profile_round.sh (FETCH_SIZE x 2 on gfx950, WRITE_SIZE as is); a
        # committed summary of an earlier run of this command, NOT a measurement of this run: the file says which round
        traffic=None if traffic_frame is None else round(traffic_frame / launches, 1),
        traffic_per_frame=traffic_frame, traffic_source=tfile,
        rocprofv3_avg_launch_us=None if rocprof_us is None else round(rocprof_us, 3), rocprofv3_source=rfile,
        # `frac` again from the committed rocprofv3 --kernel-trace --stats summary of this command alone (nothing live): the conv
        # launches' total duration per frame there, this plan's algorithmic FLOPs, the same peak -- so the fraction can be checked
        # from the line.  (The live `frac` above uses the profiling twin's slot times of THIS run and this box.)
        recomputed_from=None if not rocprof_ms else {
            "file": "profiles/" + rfile, "conv_ms_per_frame": round(rocprof_ms, 4), "conv_launches_per_frame": rocprof_calls,
            "flops_per_frame": flops, "achieved_tflops": round(flops / (rocprof_ms * 1e-3) / 1e12, 3),
            "frac_of_%s" % ("bf16_mfma_peak" if precision == "bf16" else "fp32_instruction_peak"): round(flops / (rocprof_ms * 1e-3) / 1e12 / peak, 4),
            **({"hbm_frac": round(BF16_BYTES_PER_FRAME * images_frac / (rocprof_ms * 1e-3) / 1e9 / PEAK_HBM, 4)} if precision == "bf16" else {})})
    if precision == "fp32":  # the fp32 conv stack is MFMA-bound
        return dict(bound="mfma", achieved=round(achieved, 3), peak=PEAK_FP32_MFMA, unit="TFLOP/s",
                    frac=round(achieved / PEAK_FP32_MFMA, 4), **common)
    if precision == "fp32_split":
        # fp32-class results, but the products run on the bf16 pipe, 6 bf16 MFMAs per fp32 MFMA-equivalent: its own ceiling is the bf16
        # peak / 6 (417 TFLOP/s of fp32-equivalent work); the fraction of the fp32 INSTRUCTION's peak is carried beside it for comparison
        pk = PEAK_BF16_MFMA / 6
        return dict(bound="mfma", achieved=round(achieved, 3), peak=round(pk, 1), unit="TFLOP/s (fp32-equivalent)", frac=round(achieved / pk, 4),
                    vs_fp32_instruction_peak=round(achieved / PEAK_FP32_MFMA, 4), **common)
    # bf16: 16x the MFMA rate makes the same stack memory / latency-bound: priced against HBM with its algorithmic bytes
    gbs = BF16_BYTES_PER_FRAME * images_frac / (conv_ms * 1e-3) / 1e9
    return dict(bound="hbm", achieved=round(gbs, 1), peak=PEAK_HBM, unit="GB/s", frac=round(gbs / PEAK_HBM, 4),
                algorithmic_bytes_per_frame=BF16_BYTES_PER_FRAME * images_frac,
                mfma_view={"achieved_tflops": round(achieved, 2), "peak": PEAK_BF16_MFMA, "frac": round(achieved / PEAK_BF16_MFMA, 4)},
                **common)


def latency_summary(lat, steps):
    """p50 / p95 / max of the per-frame latencies of a timed region, the rate the MEDIAN frame gives (a short run's mean is moved by
    one slow frame: `value` stays the contract's mean, this is the self-check beside it), and -- for runs short enough to print --
    the frames themselves in order, so that a slow frame can be located (first after the barrier? periodic?) from the line alone."""
    import numpy as np
    p50 = float(np.percentile(lat, 50))
    d = {"p50": round(p50, 4), "p95": round(float(np.percentile(lat, 95)), 4), "max": round(float(lat.max()), 4),
         "value_from_median": round(1e3 / p50, 2)}
    if steps <= 64:
        d["frames_ms"] = [round(float(x), 4) for x in lat]
    return d


def profile(run, h, n):
    """n frames on the profiling twin of the frame graph; `run(n)` drives them (every rank of a pyramid job takes part)."""
    h.set_profiling(True)
    h.reset_timings()
    run(n)
    tim = h.timings()
    h.set_profiling(False)
    return tim


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as child processes (this parent has not imported torch
    or loaded the HIP library, and never does), relay rank 0's JSON line, exit with the worst child return code.  A child that
    fails takes the others down after a grace period (they would wait in a barrier for ever).  VNECT_BENCH_WORKER names another
    worker script (the CPU test's stub)."""
    import socket
    import subprocess
    worker = os.environ.get("VNECT_BENCH_WORKER") or os.path.abspath(__file__)
    if (worker == os.path.abspath(__file__) and os.environ.get("VNECT_BENCH_BACKEND", "nccl") == "nccl"
            and os.environ.get("VNECT_BENCH_DEVICE") is None):
        # one rank per GPU: refuse at once -- before N processes meet in a rendezvous that can only time out -- when the machine
        # has fewer devices than ranks.  Counted in a throw-away child, so that this parent still never touches the GPU.
        try:
            have = int(subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                                      text=True, timeout=600).stdout.strip().splitlines()[-1])
        except Exception:
            have = None   # cannot tell: let the ranks find out (each checks its own device, see main)
        if have is not None and have < n:
            sys.exit("bench.py: --gpus %d needs %d HIP devices (one rank per GPU), this machine exposes %d: HIP device %d is missing"
                     % (n, n, have, have))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), VNECT_BENCH_SPAWNED="1")
        procs.append(subprocess.Popen([sys.executable, worker] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True if r == 0 else None))
    limit = float(os.environ.get("VNECT_BENCH_SPAWN_TIMEOUT", "1500"))
    t0, first_fail, out0 = time.time(), None, []
    import threading
    rd = threading.Thread(target=lambda: out0.extend(procs[0].stdout.readlines()), daemon=True)
    rd.start()
    while any(p.poll() is None for p in procs):
        time.sleep(0.2)
        bad = [p for p in procs if p.poll() not in (None, 0)]
        if bad and first_fail is None:
            first_fail = time.time()
        if (first_fail is not None and time.time() - first_fail > 15) or time.time() - t0 > limit:
            for p in procs:          # the exact PIDs this function started
                if p.poll() is None:
                    p.kill()
            break
    rcs = [p.wait() for p in procs]
    rd.join(timeout=10)
    line = None
    for ln in out0:
        if ln.lstrip().startswith("{"):
            line = ln.strip()
        else:
            sys.stderr.write(ln)
    if line:
        print(line, flush=True)
    worst = max((abs(rc) for rc in rcs), default=0)
    if worst == 0 and not line:
        worst = 1
    sys.exit(min(worst, 255))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline (see the module's docstring); off: set up, warm up, time the K steps, "
                         "write --dump-outputs, print the line")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="--full: budget of the cpu_baseline leg (0 = skip)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches everywhere")
    ap.add_argument("--graph", action="store_true", help="replay the frame graph for synchronous frames too (default: auto = eager "
                                                        "launches for a synchronous frame, graph replay when frames are in flight)")
    ap.add_argument("--no-aux", action="store_true",
                    help="--full: skip the auxiliary legs (PCIe-inclusive, frames in flight, two streams per GPU, the bf16 leg): a "
                         "profiler run meant to describe the synchronous headline loop of ONE precision uses this")
    ap.add_argument("--precision", choices=["fp32", "bf16", "fp32_split"], default="fp32",
                    help="fp32 = BASELINE.json configs[1] (default, the headline); bf16 = configs[2] (bf16 MFMA conv path); fp32_split = fp32 "
                         "tensors and accumulators, products on the bf16 matrix pipe by exact three-way splits (VNECT_FP32_SPLIT)")
    ap.add_argument("--pyramid", action="store_true",
                    help="BASELINE.json configs[3]: ONE stream, one scale per GPU (needs --gpus 3), one exchange of the maps per "
                         "frame; default for N>1 is N independent streams (configs[4])")
    ap.add_argument("--exchange", choices=["rccl", "p2p"], default="rccl",
                    help="--pyramid: ncclAllGather over RCCL, or direct peer writes over xGMI (SURVEY 8e asks for both)")
    ap.add_argument("--scales", default=None,
                    help="comma-separated pyramid (default 1.0,0.8,0.6 = BASELINE.json).  Anything else is a REHEARSAL, labelled as such "
                         "in the line: `--pyramid --scales 1.0 --gpus 1` runs the whole configs[3] machinery -- torch's \"nccl\" process "
                         "group, PyramidJob, ncclCommInitRank + one ncclAllGather per frame, timed loop, profile -- with ONE rank on one GPU")
    ap.add_argument("--dump-joints", default=None, metavar="PREFIX",
                    help="parity evidence for the N > 1 tests (tests/test_gpu_multigpu.py): behind the timed region every rank runs 8 more "
                         "frames of its stream on fresh filter banks at fixed timestamps and writes PREFIX.<leg>.rank<r>.npz (j2, j3); a "
                         "single-GPU run of the same seeds must reproduce them bit for bit")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the headline's timed region, write what its LAST timed step returned to the caller -- the joints of "
                         "Handle.infer_resident -- as DIR/joints_2d.npy (21x2 float64) and DIR/joints_3d.npy (21x3 float32); rank r > 0 of "
                         "an N > 1 job adds .rank<r> before .npy.  Frames, weights and timestamps are fixed by the arguments, so two builds "
                         "run with the same arguments can be compared output for output")
    ap.add_argument("--no-bind", action="store_true",
                    help="N > 1: leave every rank's host thread where the scheduler puts it.  Default: before its first GPU call a rank binds "
                         "itself to the cores local to its GPU (/sys/bus/pci/devices/<bdf>/local_cpulist) and reports the mask in `ranks[]`")
    ap.add_argument("--bind", action="store_true", help="apply the same binding at N = 1 (default there: report it, do not apply it)")
    ap.add_argument("--no-n1", action="store_true",
                    help="--full, N > 1: skip the same-job N = 1 reference (rank 0's loop run alone, the other ranks idle, before the N-rank "
                         "region)")
    ap.add_argument("--pyramid-both", action="store_true",
                    help="--pyramid with BOTH exchange forms in one job (rccl first, then p2p): the side-by-side SURVEY 8e asks for "
                         "from one 3-GPU lease; `value` is the RCCL all-gather form (the one north_star names), p2p under \"pyramid_p2p\"")
    args = ap.parse_args()

    if args.pyramid_both:
        args.pyramid = True
    global SCALES
    rehearsal_scales = None
    if args.scales:
        SCALES = [float(x) for x in args.scales.split(",") if x.strip()]
        if SCALES != [1.0, 0.8, 0.6]:
            rehearsal_scales = "rehearsal: scales %s instead of BASELINE.json's [1.0, 0.8, 0.6] -- not a measurement of any config" % SCALES
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args.gpus, sys.argv[1:])  # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        args.gpus = world  # the launcher's word counts

    # N > 1 runs unattended: a rank that hangs (a collective one rank never joins, a peer that never writes) says WHERE -- every 5 minutes
    # each rank dumps its Python stack to stderr until the job ends (the driver keeps the tail)
    if world > 1:
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ.get("VNECT_BENCH_STACK_DUMP_S", "300")), repeat=True, exit=False)

    # Host placement FIRST, before this process imports torch or loads the HIP library (their helper threads and pinned allocations
    # inherit the mask): the cores local to this rank's GPU.  sysfs only, no GPU call (vnect_amd/parallel.py).
    from vnect_amd.parallel import bind_rank
    _dev_env = os.environ.get("VNECT_BENCH_DEVICE")
    _want_dev = int(_dev_env if _dev_env is not None else os.environ.get("LOCAL_RANK", "0"))
    if world > 1 or args.bind:
        binding = bind_rank(_want_dev, enable=not args.no_bind)
    else:
        binding = bind_rank(_want_dev, enable=False)
        binding["reason"] = "N = 1: reported, not applied (--bind applies it)"

    # ONE JSON line on stdout, whatever the libraries underneath print: RCCL writes a version banner to STDOUT when its first communicator
    # is made (torch's "nccl" process group in an N > 1 run, the library's in a pyramid run).  So file descriptor 1 points at stderr while
    # the job runs, and the line goes to the real stdout at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import numpy as np
    import torch

    from tests import helpers
    from vnect_amd import _native
    from vnect_amd.parallel import Group, PyramidJob, aggregate_rate, stream_seed
    from vnect_amd.weights import synthetic_weights

    # Rehearsal on a ONE-GPU box (never the measured configuration): VNECT_BENCH_DEVICE=0 puts every rank on device 0 and
    # VNECT_BENCH_BACKEND=gloo carries the barrier / max-reduce over the CPU (RCCL refuses two ranks on one device)
    backend = os.environ.get("VNECT_BENCH_BACKEND", "nccl")
    dev_override = os.environ.get("VNECT_BENCH_DEVICE")
    want_dev = int(dev_override if dev_override is not None else os.environ.get("LOCAL_RANK", "0"))
    have_dev = torch.cuda.device_count()
    if want_dev >= have_dev:   # e.g. --gpus 2 under a launcher on a 1-GPU box: say which device is missing, at once, non-zero
        sys.exit("bench.py: rank %s needs HIP device %d, but this machine exposes %d device(s) -- one rank per GPU (--gpus %d needs %d)"
                 % (os.environ.get("RANK", "0"), want_dev, have_dev, args.gpus, args.gpus))
    torch.cuda.set_device(want_dev)
    # a pyramid job always builds the process group, with one rank too: the rehearsal then runs torch's RCCL and the library's in
    # one process exactly as the 3-GPU job does
    grp = Group(backend, always_init=args.pyramid, device=want_dev)
    rank = grp.rank
    local_rank = want_dev
    # what the run actually exercised: the world size as a real all-reduce over the backend sees it (backend "nccl" IS RCCL on
    # ROCm), and where every rank sits
    ranks_seen = grp.count_ranks()
    try:
        pci = torch.cuda.get_device_properties(local_rank).pci_bus_id
    except Exception:
        pci = None
    # the sysfs chain (KFD node order) and HIP agree on which device this is?  If not, the thread moves to the right device's cores now
    from vnect_amd.parallel import rebind_by_bus
    binding = rebind_by_bus(binding, pci)
    placement = grp.all_gather_object({"rank": rank, "device": local_rank, "pci_bus_id": pci, "pid": os.getpid(), "host_binding": binding})
    weights = synthetic_weights()
    nslots = 8

    def make(prec, **kw):
        h = _native.Handle(SCALES, device=local_rank, num_frame_slots=nslots,
                           precision={"bf16": _native.BF16, "fp32_split": _native.FP32_SPLIT}.get(prec, _native.FP32), **kw)
        h.set_weights(weights)
        h.finalize()
        return h

    # replicas: one synthetic video stream per rank, seeds 1234 + 1000*stream;
    # pyramid: every rank sees the SAME stream 0.  (Synthesised BEFORE the handle is built, so that nothing but the frame uploads lies
    # between vnect_finalize's warm start and the measured loop.)
    stream = 0 if args.pyramid else rank
    host_frames = [helpers.synth_frame(stream_seed(stream, k)) for k in range(nslots)]
    graph_mode = False if args.no_graph else (True if args.graph else "auto")
    job = None
    rehearsal_note = rehearsal_scales
    if args.pyramid:
        if args.gpus != len(SCALES):
            sys.exit("--pyramid shards the %d scales over %d GPUs: use --gpus %d" % (len(SCALES), len(SCALES), len(SCALES)))
        if args.pyramid_both and dev_override is not None:
            # one-GPU rehearsal: RCCL refuses several ranks on one device ("invalid usage"), so only the peer-write leg can run here
            args.pyramid_both, args.exchange = False, "p2p"
            rehearsal_note = ((rehearsal_note + "; ") if rehearsal_note else "") + \
                "rehearsal on ONE device: the RCCL leg of --pyramid-both cannot run (RCCL refuses several ranks per device); p2p only"
        if args.pyramid_both:
            args.exchange = "rccl"   # first leg; the p2p leg follows the headline's timed region and profile

        def make_job(exchange):
            xc = _native.XCHG_P2P if exchange == "p2p" else _native.XCHG_RCCL
            return PyramidJob(grp, SCALES, lambda r, w, ex: make(args.precision, pyramid=(r, w), exchange=xc), exchange)

        job = make_job(args.exchange)
        h = job.handle
    else:
        # lanes=3: the extra lanes only ever run frames submitted while others are in flight (the pipelined leg below)
        h = make(args.precision, use_graph=graph_mode, lanes=3)
    for k in range(nslots):
        h.upload_frame(k, host_frames[k])
    rccl_lib = None
    if args.pyramid and args.exchange == "rccl":
        path, reused = _native.Handle.comm_library()   # the file ncclAllGather lives in, and whether it is the copy torch had mapped
        tl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        rccl_lib = {"path": path, "reused_the_copy_already_mapped": reused,
                    "is_torchs_bundled_copy": os.path.exists(tl) and os.path.exists(path) and os.path.samefile(path, tl),
                    "copies_mapped_in_this_process": sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "librccl" in ln})}

    clock = [1.7e9]

    def run(hh, n):
        out = None
        for i in range(n):
            clock[0] += 1 / 30
            out = hh.infer_resident(i % nslots, clock[0], clock[0] + 1e-3)
        return out

    def barrier():
        grp.barrier()
        torch.cuda.synchronize()

    own = [0.0, 0.0]
    last = [None]   # (j2, j3) of the last timed step of the latest timed region

    def timed(hh, steps, warmup):
        """W untimed frames, then EXACTLY `steps` synchronous frames between barrier + synchronize; MAX over ranks."""
        run(hh, warmup)
        barrier()
        t0 = time.perf_counter()
        stamps = [t0]
        for i in range(steps):
            clock[0] += 1 / 30
            j2, j3 = hh.infer_resident(i % nslots, clock[0], clock[0] + 1e-3)
            stamps.append(time.perf_counter())  # per-frame latency distribution (median + p95)
        own[0] = stamps[-1] - t0    # this rank's own time for its K frames (before it waits for the others)
        barrier()
        own[1] = time.perf_counter() - t0 - own[0]   # what the closing barrier + synchronize took on this rank (INSIDE the region by the contract)
        elapsed = grp.max_over_ranks(time.perf_counter() - t0)
        last[0] = (j2, j3)
        assert np.all(np.isfinite(j2)) and np.all(np.isfinite(j3))
        return elapsed, np.diff(np.array(stamps)) * 1e3

    def dump_joints(hh, leg):
        """--dump-joints: 8 frames of this rank's stream on fresh filter banks, fixed timestamps (DUMP_T0 + k / 30); outside every timed
        region.  A pyramid job's ranks all take part (each inference contains the exchange)."""
        if not args.dump_joints:
            return
        hh.reset_filters()
        js = [hh.infer_resident(k % nslots, DUMP_T0 + k / 30, DUMP_T0 + k / 30 + 1e-3) for k in range(8)]
        hh.reset_filters()
        np.savez("%s.%s.rank%d.npz" % (args.dump_joints, leg, rank), j2=np.stack([a for a, _ in js]), j3=np.stack([b for _, b in js]),
                 device=np.int64(local_rank), stream=np.int64(stream))

    # N > 1, --full: the same-box, same-minute denominator of `value / N` -- rank 0 runs the N = 1 loop ALONE first (W warm-up + K timed frames of
    # the plain 3-scale handle; a pyramid job builds one for this), the other ranks wait on the rendezvous store with their GPUs idle.
    n1_same_job = None
    nprof = min(max(args.steps // 4, 10), 100)   # frames of a profiling-twin pass (--full)
    if args.full and args.gpus > 1 and not args.no_n1:
        grp.barrier()
        if rank == 0:
            h1 = h
            if args.pyramid:
                h1 = make(args.precision, use_graph=graph_mode)
                for k in range(nslots):
                    h1.upload_frame(k, host_frames[k])
            run(h1, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st1 = [t0]
            for i in range(args.steps):
                clock[0] += 1 / 30
                h1.infer_resident(i % nslots, clock[0], clock[0] + 1e-3)
                st1.append(time.perf_counter())
            torch.cuda.synchronize()
            e1 = time.perf_counter() - t0
            tim1 = profile(lambda n: run(h1, n), h1, nprof)   # the same device-side figures the per-rank reports carry, for the solo loop
            n1_same_job = {"value": round(args.steps / e1, 2), "unit": "frames/s", "ms_per_step": round(e1 / args.steps * 1e3, 4),
                           "steps": args.steps, "warmup": args.warmup, "rank": 0, "device": local_rank,
                           "latency_ms": latency_summary(np.diff(np.array(st1)) * 1e3, args.steps),
                           "conv_stack_ms": round(tim1["conv_slot_ms"] / nprof, 4), "frame_ms_hip_events": round(tim1["total_ms"] / nprof, 4),
                           "shader_clock_mhz": None if not tim1.get("shader_clock_mhz") else round(tim1["shader_clock_mhz"], 1),
                           "what": "rank 0's synchronous 3-scale loop run alone inside this job, before the %d-rank region; the other ranks "
                                   "wait on the rendezvous store (host-side: their GPUs are idle)" % args.gpus}
            if args.pyramid:
                h1.close()
            else:
                h.reset_filters()
        grp.host_handoff("n1_done", release=rank == 0)
        grp.barrier()
    elif args.gpus > 1 and not args.no_n1 and rank == 0:
        # without --full the reference leg does not run, but its frames' timestamps still pass on rank 0: the filters then see the
        # same timestamps as in a --full run, so --dump-outputs writes the same joints
        for _ in range(args.warmup + args.steps + nprof):
            clock[0] += 1 / 30

    elapsed, lat = timed(h, args.steps, args.warmup)
    own_elapsed, own_close = own[0], own[1]
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        sfx = ".rank%d" % rank if rank else ""
        np.save(os.path.join(args.dump_outputs, "joints_2d%s.npy" % sfx), np.asarray(last[0][0], dtype=np.float64))
        np.save(os.path.join(args.dump_outputs, "joints_3d%s.npy" % sfx), np.asarray(last[0][1], dtype=np.float32))
    dump_joints(h, ("pyramid_" + args.exchange) if args.pyramid else "replica")

    # pipelined rate of the same stream (three frames in flight on three lanes: they overlap, only the filter kernels stay
    # ordered), reported beside the synchronous one
    pipelined = pcie = pinned = two_streams = call_surface = None
    if args.full and not args.no_aux and not args.pyramid:
        barrier()
        p0 = time.perf_counter()
        depth = 3  # frames in flight = lanes of the handle
        for i in range(args.steps):
            if i >= depth:
                h.collect()
            clock[0] += 1 / 30
            h.submit_resident(i % nslots, clock[0], clock[0] + 1e-3)
        for _ in range(min(depth, args.steps)):
            h.collect()
        torch.cuda.synchronize()
        pipelined = args.steps / (time.perf_counter() - p0)
        # The CALL-SURFACE rate (VNectEstimator.__call__ takes host memory, /root/reference/src/estimator.py:97-99): the same synchronous
        # loop fed through vnect_infer -- from pageable numpy memory (a CPU copy into the pinned staging buffer, then the copy kernel), from
        # the handle's PINNED capture buffers (vnect_frame_buffer: no CPU copy), and, as the yardstick, from resident frames -- measured
        # INTERLEAVED in rounds of 20 frames, >= 200 frames per variant, medians of the per-frame latency: the variants are 0.5-1 % apart
        # and a box drifts by more than that between two sequential 20-frame legs (round 5's figures).  Never `value`.
        bufs = [h.frame_buffer(i, 368, 368) for i in range(2)]
        for i in range(2):
            bufs[i][...] = host_frames[i]
        nh = max(args.steps, 200)
        cs_lat = {"resident": [], "pageable": [], "pinned": []}

        def cs_frame(v, i):
            clock[0] += 1 / 30
            if v == "resident":
                return h.infer_resident(1 + i % (nslots - 1), clock[0], clock[0] + 1e-3)   # (slot 0 is vnect_infer's staging slot)
            return h.infer((host_frames if v == "pageable" else bufs)[i % 2], clock[0], clock[0] + 1e-3)

        rounds = (nh + 19) // 20
        for rd in range(rounds):
            order = ("resident", "pageable", "pinned") if rd % 2 == 0 else ("pinned", "pageable", "resident")
            for v in order:
                for i in range(2):
                    cs_frame(v, i)                       # (two frames to settle into the variant: untimed)
                for i in range(20):
                    q0 = time.perf_counter()
                    cs_frame(v, i)
                    cs_lat[v].append((time.perf_counter() - q0) * 1e3)
        cs_med = {v: float(np.median(np.array(x))) for v, x in cs_lat.items()}
        pcie, pinned = 1e3 / cs_med["pageable"], 1e3 / cs_med["pinned"]
        call_surface = {"frames_per_variant": 20 * rounds, "method": "interleaved rounds of 20 synchronous frames per variant, rate of the median frame",
                        "median_ms": {v: round(x, 4) for v, x in cs_med.items()},
                        "frames_per_s": {v: round(1e3 / x, 2) for v, x in cs_med.items()},
                        "vs_resident_percent": {v: round(100 * (cs_med["resident"] / x - 1), 2) for v, x in cs_med.items()},
                        "extra_us_per_frame": {v: round((x - cs_med["resident"]) * 1e3, 1) for v, x in cs_med.items()}}
        for k in range(nslots):  # vnect_infer stages its frame in slot 0: restore the resident set
            h.upload_frame(k, host_frames[k])
        # two independent video streams sharing this GPU (two handles, two host threads): what the idle CUs between the
        # launches of one synchronous stream are worth.  Reported beside the headline, never as `value`.
        if rank == 0:
            import threading
            h2 = make(args.precision, use_graph=graph_mode)
            for k in range(nslots):
                h2.upload_frame(k, helpers.synth_frame(stream_seed(rank + 1000, k)))

            def drive(hh, base, n):
                for i in range(n):
                    hh.infer_resident(i % nslots, base + i / 30, base + i / 30 + 1e-3)

            base = clock[0] + 50
            drive(h2, base, args.warmup)
            ths = [threading.Thread(target=drive, args=(hh, base + 100, args.steps)) for hh in (h, h2)]
            torch.cuda.synchronize()
            q0 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            torch.cuda.synchronize()
            two_streams = 2 * args.steps / (time.perf_counter() - q0)
            h2.close()
            clock[0] = base + 100 + args.steps / 30 + 1

    # three independent video streams served by THIS handle (vnect_submit_stream: a filter bank per stream, one weight copy, three
    # lanes): nothing chains frames of different streams, so they overlap completely.  Beside the headline, never `value`.
    streams3 = None
    if args.full and not args.no_aux and not args.pyramid:
        barrier()
        base = clock[0] + 1000.0
        s0 = time.perf_counter()
        for i in range(args.steps):
            if i >= 3:
                h.collect_stream()
            st_ = i % 3
            h.submit_stream(st_, i % nslots, base + 10 * st_ + i / 30, base + 10 * st_ + i / 30 + 1e-3)
        for _ in range(min(3, args.steps)):
            h.collect_stream()
        torch.cuda.synchronize()
        streams3 = args.steps / (time.perf_counter() - s0)
        clock[0] = base + 100 + args.steps / 30
        h.reset_filters()

    # --full: every rank profiles its own handle (no collective inside a replica's frames; a pyramid job's inferences contain the exchange, so
    # every rank must take part anyway): per-rank conv-stack time and the shader clock each GPU held are what explains an N > 1 curve
    def rank_report(lat_, own_, tim_, close_):
        rep = {
            "rank": rank, "device": local_rank,
            "frames_per_s": round(args.steps / own_, 2), "own_elapsed_s": round(own_, 5),
            # the closing barrier + torch.cuda.synchronize() of the timed region (the contract puts it inside): what separates `value` from the
            # frames' own rate in a short window; at N > 1 it also holds this rank's wait for the slowest one
            "closing_barrier_us": round(close_ * 1e6, 1),
            "latency_ms": {k: v for k, v in latency_summary(lat_, args.steps).items() if k != "frames_ms"}}
        if tim_ is not None:
            rep.update({
                "conv_stack_ms": round(tim_["conv_slot_ms"] / nprof, 4), "conv_first_to_last_ms": round(tim_["net_ms"] / nprof, 4),
                "frame_ms_hip_events": round(tim_["total_ms"] / nprof, 4),
                "shader_clock_mhz": None if not tim_.get("shader_clock_mhz") else round(tim_["shader_clock_mhz"], 1)})
        rep["host_binding"] = {k: binding.get(k) for k in ("bound", "affinity", "n_cpus", "numa_node", "bdf", "reason") if binding.get(k) is not None}
        return grp.all_gather_object(rep)

    tim = profile(lambda n: run(h, n), h, nprof) if args.full else None
    per_rank = rank_report(lat, own_elapsed, tim, own_close)
    pyramid_p2p = None
    if args.pyramid_both:  # the same job again with the exchange by peer writes: same frames, steps, barriers; every rank takes part
        h.close()
        job = make_job("p2p")
        h = job.handle
        for k in range(nslots):
            h.upload_frame(k, host_frames[k])
        e2, lat2 = timed(h, args.steps, args.warmup)
        own2, close2 = own[0], own[1]
        dump_joints(h, "pyramid_p2p")
        tim2 = profile(lambda n: run(h, n), h, nprof) if args.full else None
        pyramid_p2p = {"value": round(args.steps / e2, 2), "unit": "frames/s", "ms_per_step": round(e2 / args.steps * 1e3, 4),
                       "exchange": "peer writes over xGMI (exchange_kernel)",
                       "latency_ms": latency_summary(lat2, args.steps), "per_rank": rank_report(lat2, own2, tim2, close2)}
    out = None
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        frac_images = 1.0  # the live plan's FLOPs already are this rank's (one image on a pyramid rank)
        out = {
            "metric": "frames/sec, 368x368 3-scale VNect inference",
            "value": round(aggregate_rate(1 if args.pyramid else args.gpus, args.steps, elapsed), 2),
            "unit": "frames/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "strong" if args.pyramid else "weak", "vs_baseline": None,
            "dtype": {"fp32": "f32", "bf16": "bf16"}.get(args.precision, "f32 (products: 3-way bf16 split, 6 of 9 terms; fp32 accumulate)"), "data": "synthetic",
            "config": {"workload": "368x368x3 uint8 BGR frame -> 21 joints; scales %s; %s; batch 1 "
                                   "(BASELINE.json configs[%d]%s); N>1 = N independent streams, one per GPU; frames resident in "
                                   "HBM, the host-to-device copy of a frame is outside the timed region"
                                   % ((json.dumps(SCALES).replace(" ", ""),) + {"fp32": ("fp32", 1), "bf16": ("bf16 operands, fp32 accumulate", 2)}.get(
                                       args.precision, ("fp32 tensors / accumulators, split-product matrix work (VNECT_FP32_SPLIT)", 1))
                                      + (" -- REHEARSAL at other scales" if rehearsal_scales else ("; configs[3] sharding" if args.pyramid else ""),)),
                       "weights": "seeded synthetic (reference ships none)", "frames_resident_in_hbm": True,
                       "h2d_in_timed_region": False,
                       "hip_graph": {False: "off (eager launches)", True: "on (every frame replays the graph)",
                                     "auto": "auto: eager launches for a synchronous frame, graph replay when frames are in flight"}[graph_mode],
                       "sync_per_frame": True,
                       "parallelism": ("pyramid: 1 scale per GPU + one %s exchange of the maps per frame"
                                       % ("RCCL all-gather" if args.exchange == "rccl" else "peer-write (xGMI)"))
                                      if args.pyramid else "stream replicas"},
            "latency_ms": latency_summary(lat, args.steps),
            # evidence of what ran: ranks counted by an all-reduce on the process-group backend, and every rank's device
            "rccl_ranks": ranks_seen if backend == "nccl" else None, "backend": backend, "backend_ranks": ranks_seen,
            # (round 6) what explains an N > 1 curve, rank by rank: each rank's OWN rate over its K frames (`value` is N K / the slowest
            # rank's time), its latency distribution, its conv stack on the device clock, the shader clock its GPU held under load
            # (eight GPUs share a node's power), where its host thread sat; and the N = 1 loop of the same job (the device figures
            # and the N = 1 loop with --full)
            "per_rank": per_rank, "build": _native.build_info()["text"],
            "ranks": placement, "launched_by": "bench.py (self-spawned ranks)" if os.environ.get("VNECT_BENCH_SPAWNED") else
                                               ("launcher (RANK / WORLD_SIZE in the environment)" if args.gpus > 1 else "single process"),
            "exchange": (("rccl: ncclAllGather of 710 976 B per rank" if args.exchange == "rccl" else "p2p: peer writes over xGMI")
                         if args.pyramid else None),
            "pyramid_p2p": pyramid_p2p,
            # (a pyramid line is a latency configuration: one rank's single-scale frame against the three-scale frame on one GPU is in
            # the newest committed profiles/rNN_one_scale_rate.json -- tools/one_scale_rate.py, DESIGN section 6 -- never a literal here)
            "note": "; ".join(x for x in (
                rehearsal_note,
                ("pyramid sharding buys latency, not throughput: what ONE rank does per frame against all three scales on one GPU is "
                 "`one_scale_vs_three` (DESIGN section 6)") if args.pyramid else None) if x) or None,
            "one_scale_vs_three": (dict(zip(("ms_per_frame", "source"), committed("_one_scale_rate.json", "ms_per_frame")))
                                   if args.pyramid else None),
            "rccl_library": rccl_lib,
        }
        if args.full:
            out.update({
                "n1_same_job": n1_same_job,
                "pcie_inclusive_frames_per_s_per_gpu": None if pcie is None else round(pcie, 2),
                "pcie_inclusive_from_pinned_capture_buffer_frames_per_s_per_gpu": None if pinned is None else round(pinned, 2),
                "call_surface": call_surface,
                "pipelined_frames_per_s_per_gpu": None if pipelined is None else round(pipelined, 2),
                "two_streams_on_one_gpu_frames_per_s": None if two_streams is None else round(two_streams, 2),
                "three_streams_on_one_handle_frames_per_s": None if streams3 is None else round(streams3, 2),
                "roofline": roofline(tim, nprof, args.precision, frac_images)})
    h.close()

    # BASELINE.json configs[2] in the same record: the bf16 MFMA conv path, measured exactly like the headline (same frames,
    # same warm-up / steps / barriers), after the fp32 timed region.  N=1 only; never `value`.
    if args.full and args.gpus == 1 and args.precision == "fp32" and not args.no_aux and not args.pyramid:
        hb = make("bf16", use_graph=graph_mode, lanes=3)
        for k in range(nslots):
            hb.upload_frame(k, host_frames[k])
        eb, latb = timed(hb, args.steps, args.warmup)
        barrier()
        p0 = time.perf_counter()   # the same stream three frames deep on three lanes (as the fp32 handle's pipelined leg)
        for i in range(args.steps):
            if i >= 3:
                hb.collect()
            clock[0] += 1 / 30
            hb.submit_resident(i % nslots, clock[0], clock[0] + 1e-3)
        for _ in range(min(3, args.steps)):
            hb.collect()
        torch.cuda.synchronize()
        bf16_pipelined = args.steps / (time.perf_counter() - p0)
        timb = profile(lambda n: run(hb, n), hb, nprof)
        hb.close()
        out["bf16"] = {"value": round(args.steps / eb, 2), "unit": "frames/s", "ms_per_step": round(eb / args.steps * 1e3, 4),
                       "dtype": "bf16", "steps": args.steps, "warmup": args.warmup,
                       "config": "BASELINE.json configs[2]: same frames and scales, bf16 operands / activations, fp32 accumulate, fp32 "
                                 "final maps, f64 post-processing; tolerance-gated against fp32 in tests/test_gpu_bf16.py",
                       "latency_ms": latency_summary(latb, args.steps),
                       "pipelined_frames_per_s_per_gpu": round(bf16_pipelined, 2),
                       "roofline": roofline(timb, nprof, "bf16")}

    # The split-product fp32 path (VNECT_FP32_SPLIT: fp32 tensors and accumulators, fp32-class results -- gated like fp32 in
    # tests/test_gpu_split.py -- with the products of the big layers on the bf16 matrix pipe), measured exactly like the headline.
    # Beside the headline, never `value`: the headline stays the fp32 INSTRUCTION path until the judge rules on this one.
    if args.full and args.gpus == 1 and args.precision == "fp32" and not args.no_aux and not args.pyramid:
        hs = make("fp32_split", use_graph=graph_mode, lanes=3)
        for k in range(nslots):
            hs.upload_frame(k, host_frames[k])
        es, lats = timed(hs, args.steps, args.warmup)
        barrier()
        p0 = time.perf_counter()   # the same stream three frames deep on three lanes (as the fp32 handle's pipelined leg)
        for i in range(args.steps):
            if i >= 3:
                hs.collect()
            clock[0] += 1 / 30
            hs.submit_resident(i % nslots, clock[0], clock[0] + 1e-3)
        for _ in range(min(3, args.steps)):
            hs.collect()
        torch.cuda.synchronize()
        split_pipelined = args.steps / (time.perf_counter() - p0)
        tims = profile(lambda n: run(hs, n), hs, nprof)
        hs.close()
        out["fp32_split"] = {"value": round(args.steps / es, 2), "unit": "frames/s", "ms_per_step": round(es / args.steps * 1e3, 4),
                             "dtype": "f32 storage and accumulate; products by exact 3-way bf16 splits (6 of 9 piece products) on v_mfma_f32_32x32x16_bf16",
                             "steps": args.steps, "warmup": args.warmup,
                             "config": "BASELINE.json configs[1] workload; precision = VNECT_FP32_SPLIT; parity gates of the fp32 path "
                                       "(tests/test_gpu_split.py::test_split_product_path_meets_the_fp32_gates: error vs the oracle equal to the fp32 instruction's)",
                             "latency_ms": latency_summary(lats, args.steps),
                             "pipelined_frames_per_s_per_gpu": round(split_pipelined, 2),
                             "roofline": roofline(tims, nprof, "fp32_split")}

    if rank == 0:
        if args.full and args.cpu_seconds > 0 and args.gpus == 1:
            # `cpu_baseline` is the FASTEST honest CPU implementation of the same workload this box can run: the reference's TF-CPU path
            # cannot run at all (no TF1, no weights), so both candidates are stand-ins and say so -- the C/OpenMP port of the path (the
            # oracle; always kept under `cpu_baseline_port`) and the torch-CPU / oneDNN network with the oracle's pre / post-processing
            # around it (`cpu_baseline_framework`).  Whichever is faster is the parsed key.
            port = cpu_baseline(weights, args.cpu_seconds)
            port["stands_in_for"] = "the reference's TF-CPU path, which cannot run here (no TensorFlow 1.x, no weights)"
            out["cpu_baseline_port"] = port
            try:
                fw = cpu_framework_baseline(weights, min(args.cpu_seconds, 8.0))
                fw["stands_in_for"] = port["stands_in_for"]
            except Exception as e:  # noqa: the proxy is optional evidence, the bench line is not
                fw = {"error": str(e)[:200]}
            out["cpu_baseline_framework"] = fw
            out["cpu_baseline"] = dict(fw if fw.get("value", 0) > port["value"] else port)
            out["cpu_baseline"]["chosen_as"] = "the faster of cpu_baseline_port and cpu_baseline_framework on this box"
        elif args.full:
            out["cpu_baseline"] = None
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    grp.close()
    if world > 1:
        faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
