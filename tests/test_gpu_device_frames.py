"""GPU: frames in device memory through the C ABI (vnect_upload_frame_device, vnect_infer_device, vnect_preprocess_device,
vnect_submit_tracked_device) and the Python layers above it.

A kernel writes the caller's device frame into the resident slot as packed BGR; everything behind the slot is unchanged.  So every result
must be BIT-identical to the host entry point given the same BGR pixels, on a second estimator with the same weights and timestamps.  The
device memory comes from the kernel probe's allocator (vnect_amd/csrc/ingest_probe.hip) and is described to the library by a bare
__cuda_array_interface__ (tests/devframe_ref.py: FakeCuda), so nothing here needs torch -- except the two child processes at the end, which
are about torch."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import nv12_ref as nr

pytestmark = pytest.mark.gpu

T0 = 1.7e9
RECT = (13, 7, 101, 80)
_CACHE = {}


def _weights(planted=False):
    if planted not in _CACHE:
        if planted:
            from tests import planted as pl
            _CACHE[planted] = pl.weights(noise=1.0)
        else:
            from vnect_amd.weights import synthetic_weights
            _CACHE[planted] = synthetic_weights()
    return _CACHE[planted]


def _est(planted=False, **kw):
    from vnect_amd import VNectEstimator
    return VNectEstimator(weights=_weights(planted), verbose=False, **kw)


def _times(n, base=0.0):
    return [(T0 + base + 0.033 * k + 0.002 * (k % 3), T0 + base + 0.033 * k + 0.0005) for k in range(n)]


class Pool:
    """device allocations of one test, freed at its end"""

    def __init__(self, probe):
        self.probe, self.ptrs = probe, []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.probe.ip_alloc(int(nbytes), C.byref(p)) == 0 and p.value
        self.ptrs.append(p.value)
        return p.value

    def put(self, buf):
        """the bytes of `buf` in an allocation of exactly their size -> its address"""
        buf = np.ascontiguousarray(buf).reshape(-1)
        p = self.alloc(len(buf))
        assert self.probe.ip_h2d(p, buf.ctypes.data, len(buf)) == 0
        return p

    def frame(self, lay, src, seed=0):
        """the pixels `src` (in the source's channel order) at layout `lay` in device memory -> the (H, W, 3) device array"""
        p = self.put(lay.place(src, seed))
        return dr.FakeCuda(p + lay.off, (lay.H, lay.W, 3), (lay.sy, lay.sx, lay.sc))

    def nv12(self, img, two=False):
        """an (H * 3 // 2, W) NV12 image in device memory: one array, or a (y, uv) pair in two allocations with odd pitches"""
        H, W = img.shape[0] * 2 // 3, img.shape[1]
        if not two:
            return dr.FakeCuda(self.put(img), img.shape, (W, 1))
        ys, uvs = W + 3, W + 5
        yb, ub = np.zeros((H, ys), np.uint8), np.zeros((H // 2, uvs), np.uint8)
        yb[:, :W], ub[:, :W] = img[:H], img[H:]
        return (dr.FakeCuda(self.put(yb.reshape(-1)[:(H - 1) * ys + W]), (H, W), (ys, 1)), dr.FakeCuda(self.put(ub.reshape(-1)[:(H // 2 - 1) * uvs + W]), (H // 2, W), (uvs, 1)))

    def close(self):
        for p in self.ptrs:
            self.probe.ip_free(p)
        self.ptrs = []


@pytest.fixture(scope="module")
def probe():
    return dr.load_probe()


@pytest.fixture()
def pool(probe):
    p = Pool(probe)
    yield p
    p.close()


@pytest.fixture(scope="module")
def est():
    e = _est()
    yield e
    e.close()


def _crop(bgr, rect):
    return bgr if rect is None else np.ascontiguousarray(bgr[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]])


@pytest.mark.parametrize("rect", [None, (5, 3, 30, 29), (21, 17, 500, 500)], ids=["whole", "rect", "rect-past-the-edges"])
def test_upload_then_read_frame_is_the_gathered_frame(est, pool, rect):
    """a 37 x 53 frame in every form and order (and as NV12, 38 x 54): the slot holds the reference's bytes, and serves the host entry points"""
    h = est.handle
    H, W = 37, 53
    for form in dr.FORMS:
        for order in dr.ORDERS:
            src = dr.pixels(H, W, 10 * form + order)
            lay = dr.Layout(form, H, W, off=form + 1, pad=order * 5)
            h.upload_frame(1, pool.frame(lay, src), pixel_format="rgb" if order else "bgr", rect=rect)
            want = _crop(dr.as_bgr(src, order), rect)
            got = h.read_frame(1)
            assert got.shape == want.shape and np.array_equal(got, want), (lay.key(), order, rect)
    img = nr.content(38, 54, 3)
    for two in (False, True):
        h.upload_frame(2, pool.nv12(img, two), pixel_format="nv12", rect=rect)
        assert np.array_equal(h.read_frame(2), _crop(nr.restate(img), rect)), ("nv12", two, rect)
    # the slot serves the resident entry points unchanged: the same joints as the same pixels uploaded from the host
    est.reset()
    a = h.infer_resident(2, *_times(1)[0])
    est.reset()
    h.upload_frame(3, _crop(nr.restate(img), rect))
    b = h.infer_resident(3, *_times(1)[0])
    est.reset()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_infer_equals_infer_of_the_host_frame(pool, precision):
    """est(device frame) == est(the same BGR pixels on the host) on a second estimator, bit for bit, over 4 frames so that the filters have
    state: packed BGR, planar RGB, NV12 (one array and two planes), with and without a rect."""
    H, W = 120, 160
    a, b = _est(precision=precision), _est(precision=precision)
    try:
        run = 0
        for kind in ("packed-bgr", "planar-rgb", "nv12", "nv12-two"):
            for rect in (None, RECT):
                a.reset(), b.reset()
                for k, t in enumerate(_times(4, 10.0 * run)):
                    if kind.startswith("nv12"):
                        img = nr.content(H, W, 40 + k)
                        dev, fmt, bgr = pool.nv12(img, kind == "nv12-two"), "nv12", nr.restate(img)
                    else:
                        form, order = (dr.PACKED3, dr.BGR) if kind == "packed-bgr" else (dr.PLANAR, dr.RGB)
                        src = nr.smooth_bgr(H, W, 60 + k) if k % 2 else dr.pixels(H, W, 60 + k)
                        dev, fmt, bgr = pool.frame(dr.Layout(form, H, W, off=k % 4, pad=k), src, k), "rgb" if order else "bgr", dr.as_bgr(src, order)
                    got = a(dev, timestamp=t, pixel_format=fmt, rect=rect)
                    want = b(_crop(bgr, rect), timestamp=t)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (precision, kind, rect, k)
                run += 1
                pool.close()
        # the pipelined form: upload into a slot (done with the buffer on return), then submit_resident
        a.reset(), b.reset()
        for k, t in enumerate(_times(3, 500.0)):
            src = dr.pixels(H, W, 90 + k)
            a.submit(pool.frame(dr.Layout(dr.PACKED4, H, W, off=2, pad=3), src), timestamp=t, rect=RECT if k else None)
            b.submit(_crop(src, RECT if k else None), timestamp=t)
            pool.close()                                         # (the frame's memory is gone before the frame has run)
            if k:
                got, want = a.collect(), b.collect()
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("submit", k)
        got, want = a.collect(), b.collect()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("rect", [None, RECT])
def test_preprocess_equals_preprocess_of_the_host_frame(est, pool, rect):
    from vnect_amd import _native
    H, W = 120, 160
    src = dr.pixels(H, W, 7)
    pre = _native.Handle(est.scales, preprocess_only=True)
    try:
        for h in (est.handle, pre):
            for form, order in ((dr.PACKED3, dr.BGR), (dr.PLANAR, dr.RGB), (dr.GENERIC, dr.BGR)):
                want = h.preprocess(_crop(dr.as_bgr(src, order), rect))
                got = h.preprocess_device(_native.device_frame(pool.frame(dr.Layout(form, H, W, 1, 2), src), "rgb" if order else "bgr", rect))
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (form, rect)
                assert got[1] == want[1] and got[2] == want[2], (form, rect, got[1:], want[1:])
        # the single slot of a preprocess_only handle grows on demand, as for host frames
        big = dr.pixels(720, 1280, 8)
        got = pre.preprocess_device(_native.device_frame(pool.frame(dr.Layout(dr.PACKED3, 720, 1280), big)))
        want = pre.preprocess(big)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and got[1:] == want[1:]
    finally:
        pre.close()


def _same(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, ((g2, g3, gr), (w2, w3, wr)) in enumerate(zip(got, want)):
        assert list(gr) == list(wr), (tag, k, gr, wr)
        assert np.array_equal(g2, w2) and np.array_equal(g3, w3), (tag, k)


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_tracking_from_device_frames_equals_tracking_from_resident_slots(pool, fmt):
    """track_on_device(source="device") over 6 frames of a 96 x 128 synthetic stream, submitted ahead on two lanes, yields exactly what
    source="resident" yields on the same pixels."""
    from vnect_amd import pixfmt, runner
    frames = list(runner.synthetic_stream(0, 6, 96, 128))
    times = _times(6)
    rect = [9, 5, 90, 70]
    e = _est(planted=True, lanes=2)
    try:
        if fmt == "nv12":
            host = [pixfmt.bgr_to_nv12(f) for f in frames]
            dev = [pool.nv12(f, two=k % 2 == 1) for k, f in enumerate(host)]
        else:
            host = frames
            dev = [pool.frame(dr.Layout([dr.PACKED3, dr.PLANAR, dr.PACKED4][k % 3], 96, 128, off=k % 4, pad=k), f, k) for k, f in enumerate(frames)]
        want = [(j2, j3, list(u)) for j2, j3, u in runner.track_on_device(e, host, rect=rect, timestamps=times, ahead=1, source="resident", pixel_format=fmt)]
        e.reset()
        got = [(j2, j3, list(u)) for j2, j3, u in runner.track_on_device(e, dev, rect=rect, timestamps=times, ahead=1, source="device", pixel_format=fmt)]
        assert len(want) == 6
        _same(got, want, fmt)
    finally:
        e.close()


def _raw_infer(h, frame, t, stream=None):
    from vnect_amd import _native
    L = _native.lib()
    j2, j3 = np.zeros((21, 2), np.float64), np.zeros((21, 3), np.float32)
    rc = L.vnect_infer_device(h._h, C.byref(frame), _native._stream_arg(stream), t[0], t[1], j2.ctypes.data_as(C.POINTER(C.c_double)),
                              j3.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, L.vnect_last_error(h._h).decode()


def test_every_refusal_by_code_and_message_and_the_handle_goes_on(pool):
    """Each refusal: VNECT_E_ARG and its message; nothing is committed -- the valid frame served right after it, with the next timestamp
    of the sequence, gives what a fresh handle fed only the valid frames gives."""
    from tests.gpu_common import _handle
    from vnect_amd import _native
    H, W = 120, 160
    cap = H * W * 3
    mk = lambda: _handle([1.0, 0.8, 0.6], _weights(), max_frame_bytes=cap)  # noqa: E731
    a, b = mk(), mk()
    try:
        src = dr.pixels(H, W, 31)
        good = pool.frame(dr.Layout(dr.PACKED3, H, W), src)
        ptr = good.__cuda_array_interface__["data"][0]
        host = np.ascontiguousarray(src)
        rng = np.zeros(2, np.int64)
        assert pool.probe.ip_range(ptr, rng.ctypes.data_as(dr.i64p)) == 0 and rng[0] <= ptr and rng[1] >= cap
        size = int(rng[0] + rng[1] - ptr)                       # bytes from the frame's first to the allocation's end, as the runtime reports them
        nv = pool.nv12(nr.content(H, W, 2))
        nvp = nv.__cuda_array_interface__["data"][0]
        wide = pool.frame(dr.Layout(dr.PACKED3, H, W + 2), dr.pixels(H, W + 2, 5))

        def df(x, fmt="bgr", rect=None, **over):
            f = _native.device_frame(x, fmt, rect)
            for k, v in over.items():
                setattr(f, k, v)
            return f

        cases = [
            ("a host pointer", df(dr.FakeCuda(host.ctypes.data, (H, W, 3))), "vnect_infer / vnect_upload_frame"),
            ("a span past the allocation's end", df(dr.FakeCuda(ptr, (size // (3 * W) + 1, W, 3)), rect=(0, 0, W, H)), "past the end of the allocation"),
            ("a span past the allocation's end, by the pitch", df(dr.FakeCuda(ptr, (H, W, 3), (3 * W + 1, 3, 1))), "past the end of the allocation"),
            ("odd NV12 size", df(dr.FakeCuda(nvp, (H * 3 // 2, W), (W, 1)), "nv12", W=W - 1), "even W and H"),
            ("a rect origin right of the frame", df(good, rect=(W, 0, 4, 4)), "origin must lie inside"),
            ("a rect origin below the frame", df(good, rect=(0, H, 4, 4)), "origin must lie inside"),
            ("an empty rect", df(good, rect=(0, 0, 0, 4)), "at least one pixel"),
            ("a crop above max_frame_bytes", df(wide), "max_frame_bytes"),
            ("struct_size wrong", df(good, struct_size=C.sizeof(_native.DeviceFrame) - 8), "struct_size"),
            ("a zero stride", df(good, stride_x=0), "strides must be positive"),
            ("an unknown format", df(good, format=7), "format must be"),
        ]
        times = _times(len(cases) + 2)
        for k, (what, frame, text) in enumerate(cases):
            rc, msg = _raw_infer(a, frame, times[k])
            assert rc == _native.E_ARG and text in msg and msg.startswith("vnect_infer_device: "), (what, rc, msg)
            rect = RECT if k % 3 == 0 else None
            got = a.infer_device(df(good, rect=rect), *times[k])
            want = b.infer(_crop(src, rect), *times[k])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
        # the Python layer turns the refusal into a ValueError; the upload and the pre-processing refuse by their own names
        with pytest.raises(ValueError, match="vnect_upload_frame_device: .*vnect_infer / vnect_upload_frame") as ei:
            a.upload_frame(1, dr.FakeCuda(host.ctypes.data, (H, W, 3)))
        assert isinstance(ei.value, _native.VnectError) and ei.value.code == _native.E_ARG
        with pytest.raises(ValueError, match="vnect_preprocess_device: .*origin must lie inside"):
            a.preprocess_device(df(good, rect=(W, 0, 2, 2)))
        with pytest.raises(_native.VnectError, match="bad frame slot"):
            a.upload_frame(99, good)
        # a tracked frame of the wrong size, and one with a rect
        a.track_begin(0, H, W, RECT)
        b.track_begin(0, H, W, RECT)
        for frame, text in ((df(wide), "not of the size vnect_track_begin gave"), (df(good, rect=RECT), "takes no rect"),
                            (df(dr.FakeCuda(host.ctypes.data, (H, W, 3))), "vnect_infer / vnect_upload_frame")):
            with pytest.raises(ValueError, match="vnect_submit_tracked_device: .*" + text) as ei:
                a.submit_tracked_device(0, frame, *times[-2])
            assert ei.value.code == _native.E_ARG
        a.submit_tracked_device(0, df(good), *times[-2])
        b.upload_frame(0, host)
        b.submit_tracked(0, 0, *times[-2])
        got, want = a.collect_tracked(), b.collect_tracked()
        assert got[0] == want[0] and got[3] == want[3] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    finally:
        a.close(), b.close()


def test_the_ingest_waits_for_the_producers_stream(probe, pool):
    """On a non-default stream: a kernel that spins a few milliseconds, then the copy that fills the frame.  vnect_infer_device with that
    stream, without synchronising, gives the host call's result (a copy that did not wait would read the zeros the frame held before);
    then the same with VNECT_STREAM_SYNCED after a stream synchronise."""
    from vnect_amd import _native
    H, W = 120, 160
    a, b = _est(), _est()
    st = C.c_void_p()
    assert probe.ip_stream_create(C.byref(st)) == 0
    try:
        n = H * W * 3
        for k, (t, synced) in enumerate(zip(_times(2), (False, True))):
            src = dr.pixels(H, W, 70 + k)
            staged, frame = pool.put(src), pool.alloc(n)
            assert probe.ip_fill(frame, 0, n) == 0
            assert probe.ip_delayed_copy(st, frame, staged, n, 4.0) == 0
            if synced:
                assert probe.ip_stream_sync(st) == 0
            got = a(dr.FakeCuda(frame, (H, W, 3)), timestamp=t, stream=_native.STREAM_SYNCED if synced else st.value)
            want = b(src, timestamp=t)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("synced" if synced else "event", k)
            assert probe.ip_stream_sync(st) == 0
    finally:
        probe.ip_stream_destroy(st)
        a.close(), b.close()


def _child(mode):
    root = dr.ROOT
    r = subprocess.run([sys.executable, "-m", "tests.devframe_torch_child", mode], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout.strip().splitlines()[-1]


def test_torch_tensors_with_torch_imported_first():
    """a child process that imports torch first: est(tensor) for a packed tensor, a permuted CHW one, bgra[..., :3] and a slice equals
    est(tensor.cpu().numpy()), and exactly one libamdhip64 is mapped"""
    last = _child("torch_first")
    print(last)
    assert last.startswith("one runtime:"), last


def test_torch_imported_after_the_handle_is_refused_or_works():
    """a child process that opens a handle first and imports torch afterwards: with two HIP runtimes mapped, est(tensor) is a ValueError
    with the import-order sentence (nothing is launched); with one, it works.  The child asserts whichever applies and says which."""
    last = _child("vnect_first")
    print(last)
    assert last.startswith("one runtime:") or (last.startswith("two runtimes: ") and "refused with the import-order sentence" in last), last
