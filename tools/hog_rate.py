"""The person detector's cost (HOG.md), on one MI355X.  Frames of 640 x 360, 1920 x 1080 and 3840 x 2160 (seeded bytes), packed BGR and
NV12, at the defaults (scale0 = 1.05) and at scale0 = 1.2; a seeded detector vector.
  (a) the three launches alone: device events around each stage (the kernel probe, which makes a frame of the size itself; a threshold
      nothing clears), median of 60 (min), the variants interleaved in rounds of 10;
  (b) vnect_hog_detect_device, wall clock of the synchronous call on a frame in device memory (level table upload, three launches, counter
      read-back, wait; rho is set so low that no window of these seeded frames hits: grouping costs nothing here);
  (c) the tracked fp32 device loop, one frame at a time (submit + collect), the 400 x 600 crop of a 1920 x 1080 frame: never calling the
      detector, twice (the A / A' pair gives the run's own spread), against one detection of the whole frame every 30th frame;
  (d) the claim to check -- a loop that never calls the detector runs at the parent commit's rate: with --parent-lib PATH (the parent
      commit's libvnect_hip.so) the loop of (c) runs in CHILD processes, this build and the parent's taking turns (new, parent, new,
      parent), each a process of its own with one library; the spread between the two identical windows of each is the margin.
Within (a), (b) and (c) the variants take turns in rounds until each has its timed calls (one warm-up round each first).  The device
memory comes from the probes' allocator: no torch, one HIP runtime.
    python3 tools/hog_rate.py [--parent-lib PATH] > profiles/hog_rate.txt"""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ROUND, TIMED = 10, 60
LOOP_ROUND, LOOP_TIMED = 30, 300


def rounds(variants, per_round, timed):
    spent = {k: 0.0 for k in variants}
    for rnd in range(1 + timed // per_round):
        for name, f in variants.items():
            t0 = time.perf_counter()
            f(rnd)
            if rnd:
                spent[name] += time.perf_counter() - t0
    return {k: v / timed for k, v in spent.items()}


def loop_child():
    """the tracked fp32 loop that never calls the detector, two identical windows; prints `loop <frames/s A> <frames/s A'>` (a child of (d):
    the library is the one VNECT_LIB names, which may be the parent commit's -- it has no vnect_hog_* symbols)"""
    from vnect_amd import _native
    if os.environ.get("HOG_RATE_PARENT"):
        for k in [k for k in _native.SYMBOLS if k.startswith("vnect_hog_")]:
            del _native.SYMBOLS[k]
    r = tracked_loop(detect_every=None, legs=("A", "A'"))
    print("loop %.2f %.2f" % (1.0 / r["A"], 1.0 / r["A'"]))


def tracked_loop(detect_every, legs):
    from tests import devframe_ref as dr
    from tests import hog_ref as R
    from tests import planted
    from tools.device_frame_rate import RECT, H, W, Device, scene
    from vnect_amd import VNectEstimator, _native
    dev = Device()
    clock = [1.7e9]
    est = VNectEstimator(weights=planted.weights(noise=1.0), verbose=False, precision="fp32")
    try:
        h = est.handle
        if detect_every:
            est.set_hog_detector(R.seeded_detector(1, rho=-1.6, scale=0.04))
        _, bgr = scene()
        f = _native.device_frame(dr.FakeCuda(dev.put(bgr), (H, W, 3)), "bgr")
        est.reset()
        h.track_begin(0, H, W, RECT)
        count = [0]

        def leg(every):
            def go(rnd):
                ts = [(clock[0] + 0.001 * k, clock[0] + 0.001 * k + 0.0002) for k in range(LOOP_ROUND)]
                clock[0] += 1.0
                for a, b in ts:
                    h.submit_tracked_device(0, f, a, b, 0)
                    h.collect_tracked()
                    count[0] += 1
                    if every and count[0] % every == 0:
                        h.hog_detect_device(f, None, _native.STREAM_SYNCED)
            return go
        return rounds({k: leg(detect_every if k == "detect" else None) for k in legs}, LOOP_ROUND, LOOP_TIMED)
    finally:
        est.close()
        dev.close()


def main():
    if "--loop-child" in sys.argv:
        return loop_child()
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    print(__doc__.split("\n    python3")[0])
    from tests import devframe_ref as dr
    from tests import hog_ref as R
    from tools.device_frame_rate import Device
    from vnect_amd import _native
    P = R.probe_lib()
    sizes = ((360, 640), (1080, 1920), (2160, 3840))
    samples, info = {}, {}

    def kernel(fmt, Hs, Ws, scale0, key):
        def go(rnd):
            ms, out = np.zeros(3 * ROUND, np.float32), np.zeros(3, np.int64)
            rc = P.hp_time(fmt, Hs, Ws, scale0, ROUND, ms.ctypes.data_as(R.f32p), out.ctypes.data_as(R.i64p))
            assert rc == 0, rc
            info[key] = tuple(int(v) for v in out)
            if rnd:
                samples.setdefault(key, []).append(ms.reshape(ROUND, 3))
        return go
    va = {}
    for Hs, Ws in sizes:
        for fmt, name in ((0, "packed BGR"), (2, "NV12")):
            for sc in (1.05, 1.2):
                key = "%4d x %4d %-10s scale0 %.2f" % (Ws, Hs, name, sc)
                va[key] = kernel(fmt, Hs, Ws, sc, key)
    rounds(va, ROUND, TIMED)
    print("(a) the three launches alone, device events around each, median of %d in us (min of their sum); levels, level pixels per frame pixel, windows:" % TIMED)
    for key, chunks in samples.items():
        ms = np.concatenate(chunks)
        med = 1e3 * np.median(ms, axis=0)
        lv, npix, nwin = info[key]
        Ws, Hs = int(key[0:4]), int(key[7:11])
        print("  %-40s votes %8.1f  blocks %8.1f  windows %8.1f  sum %8.1f (%8.1f)   %2d levels, %5.2f x, %7d windows"
              % (key, med[0], med[1], med[2], med.sum(), 1e3 * ms.sum(axis=1).min(), lv, npix / float(Hs * Ws), nwin))

    dev = Device()
    h = _native.Handle([1.0], preprocess_only=True)
    try:
        h.hog_set_detector(R.seeded_detector(1, rho=-1.6, scale=0.04))
        variants, found = {}, {}
        for Hs, Ws in sizes:
            rs = np.random.RandomState(Hs)
            bgr = rs.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
            nv = rs.randint(0, 256, (Hs * 3 // 2, Ws)).astype(np.uint8)
            for fmt, arr in (("bgr", dr.FakeCuda(dev.put(bgr), (Hs, Ws, 3))), ("nv12", dr.FakeCuda(dev.put(nv), (Hs * 3 // 2, Ws)))):
                frame = _native.device_frame(arr, fmt)
                for sc in (1.05, 1.2):
                    spec = _native.hog_spec(scale0=sc)
                    key = "%4d x %4d %-4s scale0 %.2f" % (Ws, Hs, fmt, sc)

                    def call(rnd, frame=frame, spec=spec, key=key):
                        for _ in range(ROUND):
                            found[key] = len(h.hog_detect_device(frame, spec, _native.STREAM_SYNCED)[0])
                    variants[key] = call
        print("(b) vnect_hog_detect_device, wall clock of the synchronous call, %d timed calls each in rounds of %d (detections returned):" % (TIMED, ROUND))
        for name, sec in rounds(variants, ROUND, TIMED).items():
            print("  %-34s %10.1f us   (%d)" % (name, 1e6 * sec, found[name]))
    finally:
        h.close()
        dev.close()

    r = tracked_loop(30, ("A", "A'", "detect"))
    spread = abs(r["A"] - r["A'"]) / r["A"]
    print("(c) the tracked device loop, fp32, one frame at a time, %d timed frames each in rounds of %d:" % (LOOP_TIMED, LOOP_ROUND))
    print("  never detecting (A / A')            %8.1f / %8.1f frames/s   spread %.2f %%" % (1.0 / r["A"], 1.0 / r["A'"], 100 * spread))
    print("  a detection every 30th frame        %8.1f frames/s   %+6.2f %%   %+7.1f us per frame, %.0f us per detection"
          % (1.0 / r["detect"], 100 * (r["A"] / r["detect"] - 1.0), 1e6 * (r["detect"] - r["A"]), 30e6 * (r["detect"] - r["A"])))

    print("(d) the loop that never calls the detector, this build against the parent commit's library, child processes taking turns:")
    if not parent:
        print("  --parent-lib not given: not measured")
        return
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    new_lib = os.path.join(here, "vnect_amd", "lib", "libvnect_hip.so")
    res = {"new": [], "parent": []}
    for turn in range(2):
        for name, lib in (("new", new_lib), ("parent", parent)):
            env = dict(os.environ, VNECT_LIB=lib)
            if name == "parent":
                env["HOG_RATE_PARENT"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child"], cwd=here, env=env, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr[-2000:]
            a, b = (float(v) for v in out.stdout.strip().splitlines()[-1].split()[1:])
            res[name].append((a, b))
            print("  %-6s process %d   %8.1f / %8.1f frames/s (A / A')" % (name, turn, a, b))
    mean = {k: float(np.mean(v)) for k, v in res.items()}
    spread = max(abs(a - b) / a for v in res.values() for a, b in v)
    between = max(abs(x[0] - y[0]) / x[0] for v in res.values() for x in v for y in v)
    print("  new %.1f, parent %.1f frames/s: %+.2f %%; largest A / A' spread inside a process %.2f %%, between two processes of one library %.2f %%"
          % (mean["new"], mean["parent"], 100 * (mean["new"] / mean["parent"] - 1.0), 100 * spread, 100 * between))


if __name__ == "__main__":
    main()
