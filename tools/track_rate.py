"""The tracking loop with the crop box on the device (runner.track_on_device, vnect_track_begin) against the host's loop, in ONE process.
  Planted weights (tests/planted.py), default scales [1, 0.85, 0.7]; frames captured into the handle's two PINNED buffers (two scenes,
  one per buffer, whose person differs in place and size: the box changes size every frame); fp32 and bf16; 640 x 480 and 1920 x 1080.
  Interleaved rounds, median of 5 (min - max), frames/s:
  (1) one video: runner.track (the host loop over vnect_infer) against runner.track_on_device at ahead 0 and 1 (lanes=1 handle);
  (2) three videos on a lanes=3 handle: the best host loop -- every video's next frame submitted as soon as its previous one is
      collected (vnect_upload_frame of the crop + vnect_submit_stream, vnect_collect_stream, the box on the host), three in flight --
      against runner.track_many_on_device (ahead 2);
  and, interleaved with both, the box stage as a launch of its own behind post_kernel (VNECT_TRACK_BOX_LAUNCH=1) against the default,
  the tail of post_kernel's joints stage.
    python3 tools/track_rate.py > profiles/track_rate.txt
    python3 tools/track_rate.py --profile            # a short device-tracking run for rocprofv3 --kernel-trace --stats
    python3 tools/track_rate.py --stats STATS.csv    # rocprofv3's kernel_stats.csv -> the per-kernel lines of the tracking kernels"""
import csv
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import planted  # noqa: E402
from vnect_amd import VNectEstimator, _native, runner  # noqa: E402

ROUNDS = 5
N1 = 240   # frames per trial, one video
N3 = 120   # frames per video and trial, three videos
SIZES = ((480, 640), (1080, 1920))
PRECS = ("fp32", "bf16")


def scenes(H, W):
    """Two frames: the person (three blobs, planted weights: joint j on the blob of colour j % 3) small on the left / large on the right."""
    out = []
    for cy, cx, r in ((0.45 * H, 0.35 * W, 0.06 * H), (0.50 * H, 0.60 * W, 0.16 * H)):
        blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
        out.append(planted.scene(H, W, blobs, sigma=max(6.0, H / 80.0), seed=5))
    return out


class Clock:
    def __init__(self):
        self.t = 1.7e9

    def take(self, n):
        ts = [(self.t + 0.001 * k, self.t + 0.001 * k + 0.0002) for k in range(n)]
        self.t += 0.001 * n + 1.0
        return ts


def pinned(est, H, W, imgs):
    bufs = [est.frame_buffer(H, W, b) for b in range(2)]
    for b in range(2):
        bufs[b][...] = imgs[b]
    return bufs


def host_one(est, bufs, n, clock):
    est.reset()   # every trial tracks the same box sequence from fresh filters
    ts = clock.take(n)
    t0 = time.perf_counter()
    for _ in runner.track(est, (bufs[k % 2] for k in range(n)), timestamps=ts):
        pass
    return n / (time.perf_counter() - t0)


def device_one(est, bufs, n, clock, ahead):
    est.reset()   # every trial tracks the same box sequence from fresh filters
    ts = clock.take(n)
    t0 = time.perf_counter()
    for _ in runner.track_on_device(est, (bufs[k % 2] for k in range(n)), timestamps=ts, ahead=ahead):
        pass
    return n / (time.perf_counter() - t0)


def device_three(est, bufs, n, clock):
    est.reset()   # every trial tracks the same box sequence from fresh filters
    tss = [clock.take(n) for _ in range(3)]
    vids = [(bufs[(3 * k + i) % 2] for k in range(n)) for i in range(3)]   # (the buffer track_many_on_device puts frame 3 k + i in)
    t0 = time.perf_counter()
    for _ in runner.track_many_on_device(est, vids, timestamps=tss, ahead=2):
        pass
    return 3 * n / (time.perf_counter() - t0)


def host_three(est, bufs, n, clock):
    """Three videos, one frame of each in flight: a video's next crop waits for its previous frame's joints (runner.track's box)."""
    est.reset()
    h = est.handle
    tss = [clock.take(n) for _ in range(3)]
    H, W = bufs[0].shape[:2]
    rect = [[0, 0, W, H] for _ in range(3)]
    nxt = [0, 0, 0]
    origin = {}
    count = 0

    def submit(i):
        nonlocal count
        k = nxt[i]
        x, y, w, hh = rect[i]
        if w < 1 or hh < 1:
            x, y, w, hh = rect[i] = [0, 0, W, H]
        h.upload_frame(count % 4, bufs[(3 * k + i) % 2][y:y + hh, x:x + w])
        h.submit_stream(i, count % 4, *tss[i][k])
        origin[i] = (x, y)
        nxt[i] += 1
        count += 1

    t0 = time.perf_counter()
    for i in range(3):
        submit(i)
    done = 0
    while done < 3 * n:
        s, j2, _ = h.collect_stream()
        done += 1
        j2[:, 0] += origin[s][1]
        j2[:, 1] += origin[s][0]
        rect[s] = runner.bbox_update(j2, W, H)
        if nxt[s] < n:
            submit(s)
    return 3 * n / (time.perf_counter() - t0)


def box_launch(fn):
    """fn with the box stage as its own launch (the A/B form; the library reads the switch per frame)"""
    def run():
        os.environ["VNECT_TRACK_BOX_LAUNCH"] = "1"
        try:
            return fn()
        finally:
            del os.environ["VNECT_TRACK_BOX_LAUNCH"]
    return run


def rates():
    w = planted.weights()
    print(_native.build_info()["text"])
    clock = Clock()
    for prec in PRECS:
        e1 = VNectEstimator(weights=w, precision=prec, verbose=False)
        e3 = VNectEstimator(weights=w, precision=prec, verbose=False, lanes=3)
        for H, W in SIZES:
            imgs = scenes(H, W)
            b1, b3 = pinned(e1, H, W, imgs), pinned(e3, H, W, imgs)
            rect_sizes = {tuple(r[2:]) for _, _, r in runner.track(e1, (b1[k % 2] for k in range(8)), timestamps=clock.take(8))}
            variants = (("runner.track (host box)", lambda: host_one(e1, b1, N1, clock)),
                        ("track_on_device ahead=0", lambda: device_one(e1, b1, N1, clock, 0)),
                        ("track_on_device ahead=1", lambda: device_one(e1, b1, N1, clock, 1)),
                        ("3 videos, host loop, lanes=3", lambda: host_three(e3, b3, N3, clock)),
                        ("3 videos, device, lanes=3", lambda: device_three(e3, b3, N3, clock)),
                        ("ahead=1, box as own launch", box_launch(lambda: device_one(e1, b1, N1, clock, 1))),
                        ("3 videos, box as own launch", box_launch(lambda: device_three(e3, b3, N3, clock))))
            for _, fn in variants:   # warm-up
                fn()
            res = {name: [] for name, _ in variants}
            for _ in range(ROUNDS):
                for name, fn in variants:
                    res[name].append(fn())
            med = {k: float(np.median(v)) for k, v in res.items()}
            print("\n%s, %d x %d frames from pinned buffers (crop sizes of the first frames: %s), frames/s, median of %d interleaved rounds"
                  % (prec, W, H, sorted(rect_sizes), ROUNDS))
            for name, _ in variants:
                print("  %-32s %8.1f   (%.1f - %.1f)" % (name, med[name], min(res[name]), max(res[name])))
            base1, base3 = med["runner.track (host box)"], med["3 videos, host loop, lanes=3"]
            print("  device / host: ahead=0 %.3f, ahead=1 %.3f, three videos %.3f"
                  % (med["track_on_device ahead=0"] / base1, med["track_on_device ahead=1"] / base1, med["3 videos, device, lanes=3"] / base3))
            print("  box stage as the tail of post_kernel / as its own launch: one video %.3f, three videos %.3f"
                  % (med["track_on_device ahead=1"] / med["ahead=1, box as own launch"],
                     med["3 videos, device, lanes=3"] / med["3 videos, box as own launch"]))
        e1.close()
        e3.close()


def profile():
    """A short device-tracking run (both precisions, both sizes, one video at ahead 1) for rocprofv3's per-kernel statistics."""
    w = planted.weights()
    clock = Clock()
    for prec in PRECS:
        e1 = VNectEstimator(weights=w, precision=prec, verbose=False)
        for H, W in SIZES:
            b1 = pinned(e1, H, W, scenes(H, W))
            device_one(e1, b1, 100, clock, 1)
        e1.close()


def stats(path):
    rows = list(csv.DictReader(open(path)))
    print("\nrocprofv3 --kernel-trace --stats of `track_rate.py --profile` (400 tracked frames: fp32 and bf16, 640 x 480 and 1920 x 1080, "
          "ahead 1), per-kernel average")
    keys = ("track_box_kernel", "pyramid_track_kernel", "frame_copy_track_kernel", "pyramid_kernel", "post_kernel")
    for r in rows:
        name = r.get("Name", "")
        if any(k in name for k in keys):
            print("  %-60s calls %6s  avg %8.2f us  min %8.2f us  max %8.2f us" % (name.split("(")[0][:60], r["Calls"],
                  float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


if __name__ == "__main__":
    if "--profile" in sys.argv:
        profile()
    elif "--stats" in sys.argv:
        stats(sys.argv[sys.argv.index("--stats") + 1])
    else:
        rates()
