"""Re-detection inside the device tracking loop (HOG.md, "Re-detection inside the device loop"): what it costs, on one MI355X.  Methods as in
tools/hog_rate.py: device events around each launch (the kernel probe, `make redetectprobe`), variants interleaved in rounds, one warm-up
round, two identical windows per variant for the spread.
  (1) the three gated launches alone at GATE 0 -- what a frame that is not lost pays -- as full grids with the early exit (cap 0) and as
      capped grids (cap 1024, 8192, 16384), twice each (A / A'), at 640 x 360 and 1920 x 1080;
  (2) the same launches at gate 1 (cap 1024, 4096, 8192, 16384 and full grids) against the ungated launches;
  (3) the pick kernel at 64, 1024 and 4096 hits of a 1920 x 1080 frame (clusters of up to nine neighbouring windows);
  (4) the tracked fp32 device loop, one frame at a time, the 400 x 600 crop of a 1920 x 1080 frame: (a) without the setting, twice;
      (b) with it and never lost; (c0) the rule alone calling every 30th frame lost ("reset", no re-detection); (c) with the setting and
      every 30th frame lost (vnect_track_policy is switched between two frames for that: both (c0) and (c) pay those calls);
  (5) the claim to check -- a loop that never sets re-detection runs at the parent commit's rate: with --parent-lib PATH the loop of
      (4a) runs in CHILD processes, this build and the parent's taking turns, each with one library; the gap may not exceed twice the
      spread between the two identical windows of the same run.
    python3 tools/redetect_rate.py [--parent-lib PATH] > profiles/redetect_rate.txt"""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tools.hog_rate import LOOP_ROUND, LOOP_TIMED, ROUND, TIMED, rounds  # noqa: E402

NEW = ("vnect_track_redetect", "vnect_result_redetect")
ALWAYS, NEVER = (1e9, 21, "reset"), (-1e9, 1, "reset")


def loop_child():
    from vnect_amd import _native
    if os.environ.get("REDETECT_RATE_PARENT"):
        for k in NEW:
            del _native.SYMBOLS[k]
    r = tracked_loop({"A": None, "A'": None})
    print("loop %.2f %.2f" % (1.0 / r["A"], 1.0 / r["A'"]))


def tracked_loop(legs):
    """legs: name -> None (no setting) or (redetect?, lost every n-th frame or 0)"""
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
        if any(v for v in legs.values()):
            est.set_hog_detector(R.seeded_detector(1, rho=-1.6, scale=0.04))
        _, bgr = scene()
        f = _native.device_frame(dr.FakeCuda(dev.put(bgr), (H, W, 3)), "bgr")
        est.reset()
        h.track_begin(0, H, W, RECT)
        count = [0]

        def leg(cfg):
            def go(rnd):
                redetect, every = cfg if cfg else (False, 0)
                if cfg:
                    h.track_policy(0, *NEVER)
                    if redetect:
                        h.track_redetect(0, None, True)
                ts = [(clock[0] + 0.001 * k, clock[0] + 0.001 * k + 0.0002) for k in range(LOOP_ROUND)]
                clock[0] += 1.0
                t0 = time.perf_counter()               # (the leg's settings are made outside the timed window)
                for a, b in ts:
                    count[0] += 1
                    lose = every and count[0] % every == 0
                    if lose:
                        h.track_policy(0, *ALWAYS)
                    h.submit_tracked_device(0, f, a, b, 0)
                    h.collect_tracked()
                    if lose:
                        h.track_policy(0, *NEVER)
                spent = time.perf_counter() - t0
                if cfg:
                    if redetect:
                        h.track_redetect(0, None, False)
                    h.track_policy(0, 0.0, 1, "off")
                return spent
            return go
        fns = {k: leg(v) for k, v in legs.items()}
        spent = {k: 0.0 for k in fns}
        for rnd in range(1 + LOOP_TIMED // LOOP_ROUND):   # (tools/hog_rate.py's rounds, timing the frames alone)
            for name, fn in fns.items():
                t = fn(rnd)
                if rnd:
                    spent[name] += t
        return {k: v / LOOP_TIMED for k, v in spent.items()}
    finally:
        est.close()
        dev.close()


def main():
    if "--loop-child" in sys.argv:
        return loop_child()
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    print(__doc__.split("\n    python3")[0])
    from tests import hog_ref as R
    from vnect_amd import _native
    P = C.CDLL(_native.REDETECTPROBE_LIB)
    P.rp_time.restype, P.rp_time.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, R.f32p]
    P.rp_time_pick.restype, P.rp_time_pick.argtypes = C.c_int, [C.c_int, C.c_int, R.f32p]
    samples = {}

    def kernel(Hs, Ws, gate, cap, key):
        def go(rnd):
            ms = np.zeros(3 * ROUND, np.float32)
            rc = P.rp_time(Hs, Ws, gate, cap, ROUND, ms.ctypes.data_as(R.f32p))
            assert rc == 0, rc
            if rnd:
                samples.setdefault(key, []).append(ms.reshape(ROUND, 3))
        return go

    def pick(n, key):
        def go(rnd):
            ms = np.zeros(ROUND, np.float32)
            rc = P.rp_time_pick(n, ROUND, ms.ctypes.data_as(R.f32p))
            assert rc == 0, rc
            if rnd:
                samples.setdefault(key, []).append(ms.reshape(ROUND, 1))
        return go
    va = {}
    for Hs, Ws in ((360, 640), (1080, 1920)):
        for cap in (0, 1024, 8192, 16384):
            for leg in ("A", "A'"):
                key = "(1) %4d x %4d gate 0  %-9s %s" % (Ws, Hs, "full grid" if cap == 0 else "cap %d" % cap, leg)
                va[key] = kernel(Hs, Ws, 0, cap, key)
        va["(2) %4d x %4d ungated" % (Ws, Hs)] = kernel(Hs, Ws, -1, 0, "(2) %4d x %4d ungated" % (Ws, Hs))
        for cap in (1024, 4096, 8192, 16384, 0):
            key = "(2) %4d x %4d gate 1  %s" % (Ws, Hs, "full grid" if cap == 0 else "cap %d" % cap)
            va[key] = kernel(Hs, Ws, 1, cap, key)
    for n in (64, 1024, 4096):
        va["(3) pick kernel, %4d hits" % n] = pick(n, "(3) pick kernel, %4d hits" % n)
    rounds(va, ROUND, TIMED)
    print("(1) - (3) device events around each launch, median of %d in us (votes / blocks / windows, their sum; the minimum of the sum):" % TIMED)
    for key in sorted(samples):
        ms = np.concatenate(samples[key])
        med = 1e3 * np.median(ms, axis=0)
        if ms.shape[1] == 1:
            print("  %-44s %9.1f   (%9.1f)" % (key, med[0], 1e3 * ms.min()))
        else:
            print("  %-44s %8.1f / %8.1f / %8.1f   sum %8.1f   (%8.1f)" % (key, med[0], med[1], med[2], med.sum(), 1e3 * ms.sum(axis=1).min()))

    r = tracked_loop({"A": None, "A'": None, "b": (True, 0), "c0": (False, 30), "c": (True, 30)})
    spread = abs(r["A"] - r["A'"]) / r["A"]
    print("(4) the tracked device loop, fp32, one frame at a time, %d timed frames each in rounds of %d:" % (LOOP_TIMED, LOOP_ROUND))
    print("  (a) without the setting (A / A')                 %8.1f / %8.1f frames/s   spread %.2f %%" % (1.0 / r["A"], 1.0 / r["A'"], 100 * spread))
    print("  (b) with it, never lost                          %8.1f frames/s   %+6.2f %%   %+6.1f us per frame" % (1.0 / r["b"], 100 * (r["A"] / r["b"] - 1.0), 1e6 * (r["b"] - r["A"])))
    print("  (c0) the rule alone, every 30th frame lost       %8.1f frames/s   %+6.2f %%" % (1.0 / r["c0"], 100 * (r["A"] / r["c0"] - 1.0)))
    print("  (c) with the setting, every 30th frame lost      %8.1f frames/s   %+6.2f %%   %+6.1f us per frame over (c0), %.0f us per detection"
          % (1.0 / r["c"], 100 * (r["A"] / r["c"] - 1.0), 1e6 * (r["c"] - r["c0"]), 30e6 * (r["c"] - r["c0"])))

    print("(5) the loop that never sets re-detection, this build against the parent commit's library, child processes taking turns:")
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
                env["REDETECT_RATE_PARENT"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child"], cwd=here, env=env, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr[-2000:]
            a, b = (float(v) for v in out.stdout.strip().splitlines()[-1].split()[1:])
            res[name].append((a, b))
            print("  %-6s process %d   %8.1f / %8.1f frames/s (A / A')" % (name, turn, a, b))
    mean = {k: float(np.mean(v)) for k, v in res.items()}
    spread = max(abs(a - b) / a for v in res.values() for a, b in v)
    gap = abs(mean["new"] / mean["parent"] - 1.0)
    between = max(abs(x[0] - y[0]) / x[0] for v in res.values() for x in v for y in v)
    print("  new %.1f, parent %.1f frames/s: %+.2f %%; largest A / A' spread inside a process %.2f %%, between two processes of one library %.2f %%: "
          "the gap is %s twice the spread inside a process"
          % (mean["new"], mean["parent"], 100 * (mean["new"] / mean["parent"] - 1.0), 100 * spread, 100 * between, "within" if gap <= 2 * spread else "ABOVE"))


if __name__ == "__main__":
    main()
