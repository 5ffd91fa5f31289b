"""GPU: every refusal of the host-BGR entry points (vnect_infer, vnect_upload_frame, vnect_preprocess, vnect_submit_tracked_pinned) by code
and message, and the handle goes on.

A refusal changes nothing: the valid frame served right after it, with the next timestamp of the sequence, gives BIT for bit what a second
handle fed only the valid frames gives (the shape of tests/test_gpu_nv12.py's refusal test, for the one source it does not cover)."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

T0 = 1.7e9
H, W = 120, 160
RECT = (13, 7, 101, 95)
SLOTS = 4
PINNED_CAP = 1 << 20  # a pinned buffer grows in 1-MiB steps: what vnect_frame_buffer(0, H * W * 3) holds


def _times(n):
    return [(T0 + 0.033 * k + 0.002 * (k % 3), T0 + 0.033 * k + 0.0005) for k in range(n)]


def _raw(h, name, *args):
    """The C entry point itself (the Python layer derives H, W and the stride from the array): (return code, message)."""
    from vnect_amd import _native
    L = _native.lib()
    rc = getattr(L, name)(h._h, *args)
    return rc, L.vnect_last_error(h._h).decode()


def test_every_host_bgr_refusal_by_code_and_message_and_the_handle_goes_on():
    from tests.gpu_common import _handle
    from vnect_amd import _native
    from tests import planted
    n = _native
    u8p, f64p, f32p = (C.POINTER(c) for c in (C.c_uint8, C.c_double, C.c_float))
    weights = planted.weights(noise=1.0)  # (joints that follow the scene's blobs: the tracked frames' boxes stay inside the frame)
    mk = lambda: _handle([1.0, 0.8, 0.6], weights, max_frame_bytes=H * W * 3, num_frame_slots=SLOTS)  # noqa: E731
    a, b = mk(), mk()
    try:
        frames = []
        for k in range(3):
            cy, cx, r = H * (0.45 + 0.05 * k), W * (0.40 + 0.04 * k), 10.0 + 2 * k
            blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
            frames.append(np.ascontiguousarray(planted.scene(H, W, blobs, sigma=3.0, seed=40 + k, texture=0.15)))
        wide = np.ascontiguousarray(helpers.synth_frame(50, H, W + 2, smooth=True))  # 120 x 162: more than max_frame_bytes
        img = np.ascontiguousarray(frames[0])
        p, wp = img.ctypes.data_as(u8p), wide.ctypes.data_as(u8p)
        j2, j3 = np.zeros((21, 2), np.float64), np.zeros((21, 3), np.float32)
        out = (j2.ctypes.data_as(f64p), j3.ctypes.data_as(f32p))
        t = (T0 - 1.0, T0 - 1.0)  # (a refused call's timestamps must leave no trace either)

        # (what, entry point, arguments behind the handle, code, fragment of the message)
        geometry = [("H = 0", (0, W, 3 * W)), ("W = 0", (H, 0, 3 * W)), ("row_stride = 3 W - 1", (H, W, 3 * W - 1))]
        cases = []
        for what, (hh, ww, rs) in geometry:
            cases.append(("vnect_infer, " + what, "vnect_infer", (p, hh, ww, rs, *t, *out), n.E_ARG, "bad frame geometry"))
            cases.append(("vnect_upload_frame, " + what, "vnect_upload_frame", (1, p, hh, ww, rs), n.E_ARG, "bad frame geometry"))
            cases.append(("vnect_preprocess, " + what, "vnect_preprocess", (p, hh, ww, rs, None, None, None, None), n.E_ARG, "bad frame geometry"))
        big = (H, W + 2, 3 * (W + 2))
        cases += [
            ("vnect_infer, 120 x 162", "vnect_infer", (wp, *big, *t, *out), n.E_ARG, "larger than max_frame_bytes"),
            ("vnect_upload_frame, 120 x 162", "vnect_upload_frame", (1, wp, *big), n.E_ARG, "larger than max_frame_bytes"),
            ("vnect_preprocess, 120 x 162", "vnect_preprocess", (wp, *big, None, None, None, None), n.E_ARG, "larger than max_frame_bytes"),
            ("vnect_upload_frame, slot -1", "vnect_upload_frame", (-1, p, H, W, 3 * W), n.E_ARG, "bad frame slot"),
            ("vnect_upload_frame, slot num_frame_slots", "vnect_upload_frame", (SLOTS, p, H, W, 3 * W), n.E_ARG, "bad frame slot"),
        ]
        over = (PINNED_CAP - 3 * W) // (H - 1) + 1  # the last row's last byte lies past the buffer's capacity at this stride
        assert (H - 1) * over + 3 * W > PINNED_CAP >= (H - 1) * (over - 1) + 3 * W
        tracked = [
            ("buffer index 2", (0, 2, 3 * W, *t), n.E_ARG, "no such pinned buffer"),
            ("a buffer never requested", (0, 1, 3 * W, *t), n.E_ARG, "no such pinned buffer"),
            ("row_stride = 3 W - 1", (0, 0, 3 * W - 1, *t), n.E_ARG, "does not fit the pinned buffer"),
            ("the last row past the capacity", (0, 0, over, *t), n.E_ARG, "does not fit the pinned buffer"),
            ("a stream that is not tracking", (1, 0, 3 * W, *t), n.E_STATE, "not tracking"),
            ("stream VNECT_MAX_STREAMS", (n.MAX_STREAMS, 0, 3 * W, *t), n.E_ARG, "stream out of range"),
        ]
        times = _times(len(cases) + 2 + len(tracked))
        k = 0
        # untracked: the valid frame goes through vnect_infer, or through vnect_upload_frame + vnect_infer_resident, in turn
        for what, fn, args, code, text in cases:
            rc, msg = _raw(a, fn, *args)
            assert rc == code and text in msg, (what, rc, msg)
            f = frames[k % 3]
            if k % 2:
                a.upload_frame(k % SLOTS, f)
                got = a.infer_resident(k % SLOTS, *times[k])
            else:
                got = a.infer(f, *times[k])
            want = b.infer(f, *times[k])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
            k += 1
        # vnect_infer with one frame in flight: refused, the frame in flight comes back untouched, and so does the one behind it
        a.upload_frame(2, frames[1])
        a.submit_resident(2, *times[k])
        rc, msg = _raw(a, "vnect_infer", p, H, W, 3 * W, *t, *out)
        assert rc == n.E_STATE and "frames in flight" in msg, (rc, msg)
        got, want = a.collect(), b.infer(frames[1], *times[k])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        k += 1
        got, want = a.infer(frames[2], *times[k]), b.infer(frames[2], *times[k])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        k += 1
        # tracked: the valid frame is the stream's next one, from pinned buffer 0 (buffer 1 is never requested)
        pin = {}
        for h in (a, b):
            pin[h] = h.frame_buffer(0, H, W)
            h.track_begin(0, H, W, RECT)
        for what, args, code, text in tracked:
            rc, msg = _raw(a, "vnect_submit_tracked_pinned", *args)
            assert rc == code and text in msg, (what, rc, msg)
            res = []
            for h in (a, b):
                pin[h][...] = frames[k % 3]
                h.submit_tracked_pinned(0, 0, 3 * W, *times[k])
                res.append(h.collect_tracked())
            got, want = res
            assert got[0] == want[0] == 0 and got[3] == want[3] and got[3][2] > 0, (what, got[3], want[3])
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
            k += 1
    finally:
        a.close(), b.close()
