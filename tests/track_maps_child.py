"""Child process of tests/test_gpu_track_maps.py: `python -m tests.track_maps_child SPEC.npz OUT.npz` with VNECT_LIB naming the TEST build
of the runtime (libvnect_hip_testhooks.so: the product's kernel objects under rt_*.cpp with -DVNECT_TEST_HOOKS=1).  It runs a list of
operations -- handles, tracked submits with the conv stack's output overridden by given maps (vnect_test_maps_override), collects, reads
of the stream's TrackState (vnect_test_track_state) -- and records what every one of them returned.  It judges nothing: the parent
compares the record with the CPU loop."""
import ctypes as C
import json
import os
import sys

import numpy as np


def main(spec_path, out_path):
    from tests import track_cases
    from vnect_amd import _native
    from vnect_amd.weights import synthetic_weights
    spec = np.load(spec_path)
    ops = json.loads(str(spec["ops"]))
    assert "test_hooks=1" in _native.build_info()["text"], _native.build_info()["text"]
    L = _native.lib()
    u8p = C.POINTER(C.c_uint8)
    L.vnect_test_maps_override.restype, L.vnect_test_maps_override.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float)]
    L.vnect_test_track_state.restype = C.c_int
    L.vnect_test_track_state.argtypes = [C.c_void_p, C.c_int, u8p, C.c_int32, C.POINTER(C.c_int32)]
    weights = synthetic_weights()
    precisions = {"fp32": _native.FP32, "bf16": _native.BF16, "fp16": _native.FP16}
    h, frame, src, bufs, count, scales_n = None, None, None, None, 0, 0
    record, arrays = [], {}

    def guarded(fn):
        try:
            return {"ok": fn()}
        except _native.VnectError as e:
            return {"err": [e.code, str(e)]}

    for i, op in enumerate(ops):
        kind = op[0]
        res = {}
        if kind == "handle":        # ["handle", {scales, precision, lanes, use_graph}]
            if h is not None:
                h.close()
            cfg = op[1]
            h = _native.Handle(cfg["scales"], precision=precisions[cfg["precision"]], lanes=cfg["lanes"], use_graph=cfg["use_graph"])
            h.set_weights(weights)
            h.finalize()
            scales_n, count = len(cfg["scales"]), 0
        elif kind == "env":         # ["env", name, value or null]
            if op[2] is None:
                os.environ.pop(op[1], None)
            else:
                os.environ[op[1]] = op[2]
        elif kind == "frame":       # ["frame", H, W, seed, "pinned" | "resident"]: the video's one frame (its pixels do not matter to the result)
            _, H, W, seed, src = op
            frame = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
            if src == "pinned":
                bufs = [h.frame_buffer(b, H, W) for b in range(2)]
                for b in bufs:
                    b[...] = frame
            else:
                for slot in range(4):
                    h.upload_frame(slot, frame)
        elif kind == "host_refusal":  # ["host_refusal", h, w]: what vnect_infer says to a frame of this size (the host path's message)
            res = guarded(lambda: h.infer(np.zeros((op[1], op[2], 3), np.uint8), 1.0, 1.0) and None)
        elif kind == "reset":
            h.reset_filters_stream(0)
        elif kind == "begin":       # ["begin", rect or null]
            res = guarded(lambda: h.track_begin(0, frame.shape[0], frame.shape[1], op[1]))
        elif kind == "submit":      # ["submit", index into the spec's cells / seeds, t2d, t3d]
            seed = int(spec["seeds"][op[1]])     # the frame's maps: tests/track_cases.py hot_maps, as the parent's CPU loop builds them
            maps = track_cases.hot_maps(scales_n, [tuple(c) for c in spec["cells"][op[1]]], np.random.default_rng(seed) if seed >= 0 else None)
            rc = L.vnect_test_maps_override(h._h, maps.ctypes.data_as(C.POINTER(C.c_float)))
            assert rc == 0, L.vnect_last_error(h._h)
            if src == "pinned":
                res = guarded(lambda: h.submit_tracked_pinned(0, count % 2, frame.shape[1] * 3, op[2], op[3]))
            else:
                res = guarded(lambda: h.submit_tracked(0, count % 4, op[2], op[3]))
            count += 1
        elif kind == "collect":
            def collect():
                s, j2, j3, rect = h.collect_tracked()
                arrays["j2_%d" % i], arrays["j3_%d" % i] = j2, j3
                return {"stream": s, "rect": rect}
            res = guarded(collect)
        elif kind == "box":
            res = guarded(lambda: h.track_box(0))
        elif kind == "state":       # the stream's TrackState once its last submitted frame has finished
            buf, size = np.zeros(8192, np.uint8), C.c_int32(0)
            rc = L.vnect_test_track_state(h._h, 0, buf.ctypes.data_as(u8p), len(buf), C.byref(size))
            assert rc == 0, L.vnect_last_error(h._h)
            arrays["state_%d" % i] = buf[:size.value].copy()
        else:
            raise ValueError(kind)
        record.append(res)
    if h is not None:
        h.close()
    np.savez(out_path, record=json.dumps(record), **arrays)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
