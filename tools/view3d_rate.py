"""The 3-D view's cost (VIEW3D.md), on one MI355X.  Seeded joints spread over the cube the view shows; the reference's view, width 3.
  (a) the kernel alone at 400 x 400 and 1024 x 1024 under both orders: device events around each launch (the kernel probe), median of
      200 (min), inputs in device memory and in pinned host memory (the form a tracked frame launches), the variants interleaved in
      rounds of 20;
  (b) vnect_view3d_device, wall clock of the synchronous call (validation, the joints' upload, launch, copy, wait): into device memory
      and into pinned host memory (vnect_frame_buffer);
  (c) what a caller had before: render.draw_limbs_3d (PIL, on the host) plus the upload of its picture to the device;
  (d) the tracked device loop, one frame at a time (submit + collect), fp32 and bf16, the 400 x 600 crop of a 1920 x 1080 frame: no view
      twice (the A / A' pair gives the run's own spread) against the 400 x 400 view, fetched with vnect_result_view3d and copied;
  (e) the claim to check -- a loop that never sets a view runs at the parent commit's rate: with --parent-lib PATH (the parent commit's
      libvnect_hip.so) the fp32 loop of (d) without a view runs in CHILD processes, this build and the parent's taking turns (new, parent,
      new, parent), each a process of its own with one library; the spread between the two identical windows of each is the margin.
Within (a), (b) + (c) and (d) the variants take turns in rounds until each has its timed calls (one warm-up round each first).  The
device memory comes from the probes' allocator: no torch, one HIP runtime.
    python3 tools/view3d_rate.py [--parent-lib PATH] > profiles/view3d_rate.txt"""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ROUND, TIMED = 20, 200
LOOP_ROUND, LOOP_TIMED = 30, 600
NEW_SYMBOLS = ("vnect_view3d_device", "vnect_track_view3d", "vnect_result_view3d")


def rounds(variants, per_round, timed):
    spent = {k: 0.0 for k in variants}
    for rnd in range(1 + timed // per_round):
        for name, f in variants.items():
            t0 = time.perf_counter()
            f(rnd)
            if rnd:
                spent[name] += time.perf_counter() - t0
    return {k: v / timed for k, v in spent.items()}


def tracked_loop(prec, legs):
    """legs: name -> with a view?  -> name -> seconds per frame"""
    from tests import devframe_ref as dr
    from tests import planted
    from tools.device_frame_rate import RECT, H, W, Device, scene
    from vnect_amd import VNectEstimator, _native
    dev = Device()
    clock = [1.7e9]
    est = VNectEstimator(weights=planted.weights(noise=1.0), verbose=False, precision=prec)
    try:
        h = est.handle
        _, bgr = scene()
        f = _native.device_frame(dr.FakeCuda(dev.put(bgr), (H, W, 3)), "bgr")
        est.reset()
        h.track_begin(0, H, W, RECT)
        state = [False]

        def leg(view):
            def go(rnd):
                if view != state[0]:                       # (nothing is in flight between two rounds)
                    h.track_view3d(0, _native.view3d_spec(parents=est.joint_parents) if view else None)
                    state[0] = view
                ts = [(clock[0] + 0.001 * k, clock[0] + 0.001 * k + 0.0002) for k in range(LOOP_ROUND)]
                clock[0] += 1.0
                for a, b in ts:
                    h.submit_tracked_device(0, f, a, b, 0)
                    h.collect_tracked()
                    if view:
                        assert h.result_view3d() is not None
            return go
        return rounds({k: leg(v) for k, v in legs.items()}, LOOP_ROUND, LOOP_TIMED)
    finally:
        est.close()
        dev.close()


def loop_child():
    """the tracked fp32 loop that never sets a view, two identical windows; prints `loop <frames/s A> <frames/s A'>` (a child of (e): the
    library is the one VNECT_LIB names, which may be the parent commit's -- it has no view symbols)"""
    from vnect_amd import _native
    if os.environ.get("VIEW3D_RATE_PARENT"):
        for k in NEW_SYMBOLS:
            del _native.SYMBOLS[k]
    r = tracked_loop("fp32", {"A": False, "A'": False})
    print("loop %.2f %.2f" % (1.0 / r["A"], 1.0 / r["A'"]))


def main():
    if "--loop-child" in sys.argv:
        return loop_child()
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    print(__doc__.split("\n    python3")[0])
    from tests import view3d_ref as V
    from tools.device_frame_rate import Device
    from vnect_amd import _native, render
    P = V.probe_lib()
    P.vp_time.restype, P.vp_time.argtypes = C.c_int, [V.f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, V.f32p]
    j = np.ascontiguousarray(V.skeleton(2) / 1.3, np.float32)        # every joint inside the cube
    samples = {}

    def kernel(side, order, form, key):
        def go(rnd):
            ms = np.zeros(ROUND, np.float32)
            rc = P.vp_time(j.ctypes.data_as(V.f32p), side, side, order, form, ROUND, ms.ctypes.data_as(V.f32p))
            assert rc == 0, rc
            if rnd:
                samples.setdefault(key, []).extend(float(v) for v in ms)
        return go
    va = {}
    for side in (400, 1024):
        for order in (0, 1):
            for form, where in ((0, "device memory"), (1, "pinned host memory")):
                key = "%4d x %4d order %d, inputs in %s" % (side, side, order, where)
                va[key] = kernel(side, order, form, key)
    rounds(va, ROUND, TIMED)
    print("(a) the view kernel alone, device events around each launch, median of %d (min), and ns per pixel:" % TIMED)
    for key, ms in samples.items():
        side = int(key[0:4])
        print("  %-52s %7.1f us  (%7.1f)   %6.3f ns/px" % (key, 1e3 * np.median(ms), 1e3 * min(ms), 1e6 * np.median(ms) / (side * side)))

    dev = Device()
    from tests import planted
    from vnect_amd import VNectEstimator
    est = VNectEstimator(weights=planted.weights(noise=1.0), verbose=False)    # (a handle with pinned frame buffers)
    h = est.handle
    try:
        variants = {}
        pinned = h.frame_buffer(0, 1024, 1024)
        for side in (400, 1024):
            out = dev.put(np.zeros(side * side * 3, np.uint8))
            for order in (0, 1):
                spec = _native.view3d_spec(side, order=order)
                for where, ptr in (("device", out), ("pinned host", pinned.ctypes.data)):
                    def call(rnd, spec=spec, ptr=ptr, side=side):
                        for _ in range(ROUND):
                            h.view3d_device(j, spec, ptr, 3 * side)
                    variants["(b) %4d x %4d order %d -> %s" % (side, side, order, where)] = call
            try:
                render.draw_limbs_3d(j, V.PARENTS, side)

                def before(rnd, side=side, out=out):
                    for _ in range(ROUND):
                        pic = np.ascontiguousarray(render.draw_limbs_3d(j, V.PARENTS, side))
                        assert dev.L.ip_h2d(out, pic.ctypes.data, pic.size) == 0
                variants["(c) %4d x %4d render.draw_limbs_3d on the host, and its upload" % (side, side)] = before
            except ImportError:
                print("(c) %d x %d: not measured: PIL is not installed here" % (side, side))
        print("(b) vnect_view3d_device, wall clock of the synchronous call, and (c) what a caller had before, %d timed calls each in rounds of %d:" % (TIMED, ROUND))
        for name, sec in rounds(variants, ROUND, TIMED).items():
            print("  %-68s %9.1f us" % (name, 1e6 * sec))
    finally:
        est.close()
        dev.close()

    for prec in ("fp32", "bf16"):
        r = tracked_loop(prec, {"A": False, "A'": False, "view": True})
        spread = abs(r["A"] - r["A'"]) / r["A"]
        rel = r["A"] / r["view"] - 1.0
        print("(d) the tracked device loop, %s, one frame at a time, %d timed frames each in rounds of %d:" % (prec, LOOP_TIMED, LOOP_ROUND))
        print("  no view (A / A')                    %8.1f / %8.1f frames/s   spread %.2f %%" % (1.0 / r["A"], 1.0 / r["A'"], 100 * spread))
        print("  the 400 x 400 view with every frame %8.1f frames/s   %+6.2f %%   %+7.1f us per frame; %s"
              % (1.0 / r["view"], 100 * rel, 1e6 * (r["view"] - r["A"]), "slower than the spread" if rel < -spread else "within the spread"))

    print("(e) the fp32 loop that never sets a view, this build against the parent commit's library, child processes taking turns:")
    if not parent:
        print("  --parent-lib not given: not measured")
        return
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    new_lib = os.path.join(here, "vnect_amd", "lib", "libvnect_hip.so")
    res = {"new": [], "parent": []}
    for turn in range(2):
        for name, lib in (("new", new_lib), ("parent", os.path.abspath(parent))):
            env = dict(os.environ, VNECT_LIB=lib)
            if name == "parent":
                env["VIEW3D_RATE_PARENT"] = "1"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child"], cwd=here, env=env, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stderr[-2000:]
            a, b = (float(v) for v in out.stdout.strip().splitlines()[-1].split()[1:])
            res[name].append((a, b))
            print("  %-6s process %d   %8.1f / %8.1f frames/s (A / A')" % (name, turn, a, b))
    mean = {k: float(np.mean(v)) for k, v in res.items()}
    spread = max(abs(a - b) / a for v in res.values() for a, b in v)
    between = max(abs(x[0] - y[0]) / x[0] for v in res.values() for x in v for y in v)
    diff = mean["new"] / mean["parent"] - 1.0
    print("  new %.1f, parent %.1f frames/s: %+.2f %%; largest A / A' spread inside a process %.2f %%, between two processes of one library %.2f %%: %s"
          % (mean["new"], mean["parent"], 100 * diff, 100 * spread, 100 * between,
             "inside the spread" if abs(diff) <= max(spread, between) else "OUTSIDE the spread"))


if __name__ == "__main__":
    main()
