"""Child process of tests/test_gpu_conf_track_maps.py: `python -m tests.conf_maps_child SPEC.npz OUT.npz` with VNECT_LIB naming the TEST
build of the runtime (tests/track_maps_child.py's pattern, with the loss rule): it runs a list of operations -- handles, vnect_track_policy,
tracked submits with the conv stack's output overridden by given maps (tests/conf_cases.py: conf_maps), collects with the frame's
confidences and lost flag, reads of the stream's TrackState -- and records what every one of them returned.  It judges nothing."""
import ctypes as C
import json
import os
import sys

import numpy as np


def main(spec_path, out_path):
    from tests import conf_cases
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
    h, frame, src, count, scales_n = None, None, None, 0, 0
    record, arrays = [], {}

    def guarded(fn):
        try:
            return {"ok": fn()}
        except _native.VnectError as e:
            return {"err": [e.code, str(e)]}

    for i, op in enumerate(ops):
        kind = op[0]
        res = {}
        if kind == "handle":        # ["handle", {scales, lanes, use_graph}]
            if h is not None:
                h.close()
            cfg = op[1]
            h = _native.Handle(cfg["scales"], lanes=cfg["lanes"], use_graph=cfg["use_graph"])
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
                for b in range(2):
                    h.frame_buffer(b, H, W)[...] = frame
            else:
                for slot in range(4):
                    h.upload_frame(slot, frame)
        elif kind == "reset":
            h.reset_filters_stream(0)
        elif kind == "begin":       # ["begin", rect or null]
            res = guarded(lambda: h.track_begin(0, frame.shape[0], frame.shape[1], op[1]))
        elif kind == "policy":      # ["policy", min_confidence, min_joints, action]
            res = guarded(lambda: h.track_policy(0, op[1], op[2], op[3]))
        elif kind == "submit":      # ["submit", index into the spec's cells / levels / seeds, t2d, t3d]
            k = op[1]
            maps = conf_cases.conf_maps(scales_n, [tuple(c) for c in spec["cells"][k]], spec["levels"][k], np.random.default_rng(int(spec["seeds"][k])))
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
                conf, lost = h.result_confidence()
                arrays["j2_%d" % i], arrays["j3_%d" % i], arrays["conf_%d" % i] = j2, j3, conf
                return {"stream": s, "rect": rect, "lost": lost}
            res = guarded(collect)
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
