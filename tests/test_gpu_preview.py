"""GPU: the preview through the C ABI (vnect_preview_size, vnect_preview_device) and the Python layer above it (PREVIEW.md).

What the device writes must be exactly render.preview_exact of the frame's oriented picture, to host memory and to a device `out`, whole
output buffer and all; the frame is never written; every refusal is VNECT_E_ARG with nothing written.  The device memory comes from the
device-frame probe's allocator (vnect_amd/csrc/ingest_probe.hip) and is described to the library by a bare __cuda_array_interface__
(tests/devframe_ref.py: FakeCuda), so nothing here needs torch -- except the child process, which is about torch."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import devframe_ref as dr
from tests import orient_ref
from tests import overlay_ref as R
from tests import preview_ref as P

pytestmark = pytest.mark.gpu

H, W = 70, 50


class Pool:
    """device buffers of one test: put() uploads a byte buffer, get() reads it back; freed at the test's end"""

    def __init__(self, probe):
        self.probe, self.ptrs = probe, {}

    def put(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        p = C.c_void_p()
        assert self.probe.ip_alloc(len(buf), C.byref(p)) == 0 and p.value
        assert self.probe.ip_h2d(p.value, buf.ctypes.data, len(buf)) == 0
        self.ptrs[p.value] = len(buf)
        return p.value

    def get(self, p):
        out = np.zeros(self.ptrs[p], np.uint8)
        assert self.probe.ip_d2h(out.ctypes.data, p, len(out)) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.probe.ip_free(p)
        self.ptrs = {}


@pytest.fixture()
def pool():
    p = Pool(dr.load_probe())
    yield p
    p.close()


def _source(pool, lay, buf):
    """the layout's frame in a device buffer holding `buf` -> (the buffer's address, the array the library is given, its pixel format)"""
    p = pool.put(buf)
    fmt = ("bgr", "rgb", "nv12")[lay["format"]]
    if lay["format"] == 2:
        arr = (dr.FakeCuda(p + lay["data_off"], (lay["H"], lay["W"]), (lay["sy"], 1)), dr.FakeCuda(p + lay["uv_off"], (lay["H"] // 2, lay["W"]), (lay["uv_stride"], 1)))
    else:
        arr = dr.FakeCuda(p + lay["data_off"], (lay["H"], lay["W"], 3), (lay["sy"], lay["sx"], lay["sc"]))
    return p, arr, fmt


def _exact(src, lay, o, case, f, out_format="bgr", **kw):
    from vnect_amd import render
    return render.preview_exact(P.picture(src, lay, o), case["joints"], case["parents"], case.get("rect"), factor=f, out_format=out_format, **kw)


def test_preview_device_in_every_layout_on_a_preprocess_only_handle(pool):
    """vnect_preview_device needs no weights and no plan: every layout, codes and factors going round, to pageable host memory and to a
    pitched device buffer whose every other byte keeps its canary; vnect_preview_size gives the shape; the source is unchanged."""
    from vnect_amd import _native
    h = _native.Handle([1.0], preprocess_only=True)
    try:
        for k, lay in enumerate(P.layouts(H, W)):
            o, f, ofmt = (k * 3) % 8, P.FACTORS[k % len(P.FACTORS)], ("bgr", "rgb")[k % 2]
            h.set_orientation(o)
            Hp, Wp = orient_ref.oriented_size(o, lay["H"], lay["W"])
            case = [c for c in P.cases(Hp, Wp) if c["name"] == ("skeleton", "skeleton80", "plain")[k % 3]][0]
            src = P.fresh(lay)
            want = _exact(src, lay, o, case, f, ofmt, confidence=case.get("conf"), min_confidence=case.get("thr"))
            p, arr, fmt = _source(pool, lay, src)
            frame, spec = _native.device_frame(arr, fmt), _native.preview_spec(f, ofmt)
            style = _native.overlay_style(case.get("thr"), None, case["parents"])
            dh, dw = h.preview_size(frame, spec)
            assert (dh, dw, 3) == want.shape, (lay["name"], o, f)
            host = np.full((dh, 3 * dw + 5), P.CANARY, np.uint8)                       # pageable host memory, pitched
            h.preview_device(frame, spec, host.ctypes.data, 3 * dw + 5, case["joints"], case.get("rect"), case.get("conf"), style, _native.STREAM_SYNCED)
            assert np.array_equal(host[:, :3 * dw].reshape(dh, dw, 3), want) and (host[:, 3 * dw:] == P.CANARY).all(), (lay["name"], o, f, "host")
            buf, pitch = P.out_buffer(dh, dw, k % 4, 7)
            q = pool.put(np.concatenate([buf, np.full(64, P.CANARY, np.uint8)]))
            h.preview_device(frame, spec, q + k % 4, pitch, case["joints"], case.get("rect"), case.get("conf"), style, _native.STREAM_SYNCED)
            assert np.array_equal(pool.get(q)[:len(buf)], P.whole(want, k % 4, pitch)) and (pool.get(q)[len(buf):] == P.CANARY).all(), (lay["name"], o, f, "device")
            assert np.array_equal(pool.get(p), src), (lay["name"], "the source was written")
    finally:
        h.close()


def test_est_preview_and_preview_size(pool):
    from tests import planted as pl
    from vnect_amd import VNectEstimator
    est = VNectEstimator(weights=pl.weights(noise=1.0), verbose=False)
    try:
        for k, name in enumerate(("packed3_padded", "planar", "rgb_packed4_odd_base", "nv12_pitched_odd_base")):
            lay = [l for l in P.layouts(H, W) if l["name"] == name][0]
            o = (0, 3, 5, 6)[k]
            Hp, Wp = orient_ref.oriented_size(o, lay["H"], lay["W"])
            case = P.skeleton(Hp, Wp)
            assert case["parents"] == list(est.joint_parents)
            src = P.fresh(lay)
            p, arr, fmt = _source(pool, lay, src)
            conf = np.linspace(0.0, 1.0, 21)
            want = _exact(src, lay, o, case, None, confidence=conf, min_confidence=0.4, colors=((9, 8, 7), None))
            got = est.preview(arr, case["joints"], rect=case["rect"], confidence=conf, min_confidence=0.4, colors=((9, 8, 7), None), pixel_format=fmt, orientation=o)
            assert got.shape == want.shape == est.preview_size(lay["H"], lay["W"], orientation=o) + (3,) and np.array_equal(got, want), name
            assert max(got.shape[:2]) == 1024
            plain = est.preview(arr, pixel_format=fmt, factor=0.5, out_format="rgb", orientation=o)
            assert np.array_equal(plain, _exact(src, lay, o, dict(case, joints=None, rect=None), 0.5, "rgb")), name
            dh, dw = est.preview_size(lay["H"], lay["W"], 0.37, orientation=o)
            q = pool.put(np.full(dh * dw * 3, P.CANARY, np.uint8))
            out = dr.FakeCuda(q, (dh, dw, 3), (3 * dw, 3, 1))
            assert est.preview(arr, case["joints"], rect=case["rect"], pixel_format=fmt, factor=0.37, out=out, orientation=o) is out
            assert np.array_equal(pool.get(q).reshape(dh, dw, 3), _exact(src, lay, o, case, 0.37)), name
            with pytest.raises(ValueError, match="out must be"):
                est.preview(arr, pixel_format=fmt, factor=0.5, out=out, orientation=o)
            assert np.array_equal(pool.get(p), src), (name, "the source was written")
        with pytest.raises(ValueError, match="device memory"):
            est.preview(np.zeros((H, W, 3), np.uint8))
    finally:
        est.close()


def test_refusals_write_nothing(pool):
    from vnect_amd import _native
    L = _native.lib()
    lay = P.layouts(H, W)[0]
    case = P.skeleton(H, W)
    src = P.fresh(lay)
    p, arr, fmt = _source(pool, lay, src)
    dh, dw = P.shape_of(H, W, 0.5)
    canary = np.full(dh * dw * 3 + 64, P.CANARY, np.uint8)
    q = pool.put(canary)
    host_src = src.copy()
    j2 = np.ascontiguousarray(case["joints"], np.float64)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = _native.Handle([1.0], preprocess_only=True)

    def raw(frame=None, spec=None, out=None, pitch=3 * dw, rect=(3, 2, 40, 30), style=None):
        frame = _native.device_frame(arr, fmt) if frame is None else frame
        spec = _native.preview_spec(0.5) if spec is None else spec
        r = np.asarray(rect, np.int32)
        rc = L.vnect_preview_device(h._h, C.byref(frame), C.c_void_p(_native.STREAM_SYNCED), j2.ctypes.data_as(f64p), None, r.ctypes.data_as(i32p),
                                    None if style is None else C.byref(style), C.byref(spec), C.c_void_p(q if out is None else out), pitch)
        return rc, L.vnect_last_error(h._h).decode()

    def spec(f=0.5, **over):
        s = _native.preview_spec(f)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    try:
        bad_parent = _native.overlay_style(parents=R.PARENTS)
        bad_parent.parents[5] = 21
        bad_colour = _native.overlay_style(parents=R.PARENTS)
        bad_colour.rect_bgr[1] = 256
        other = pool.put(np.zeros(4096, np.uint8))
        rng = np.zeros(2, np.int64)
        assert pool.probe.ip_range(other, rng.ctypes.data_as(dr.i64p)) == 0 and rng[0] <= other and rng[1] >= 4096
        near_end = int(rng[0] + rng[1]) - 100                               # 100 bytes in front of the allocation's end, as the runtime reports it
        cases = [
            ("a negative factor", dict(spec=spec(-0.5)), "factor"),
            ("a NaN factor", dict(spec=spec(float("nan"))), "factor"),
            ("an infinite factor", dict(spec=spec(float("inf"))), "factor"),
            ("a side that rounds to 0", dict(spec=spec(0.009)), "rounds to 0"),
            ("a side above 4096", dict(spec=spec(100.0)), "4096"),
            ("a wrong spec size", dict(spec=spec(struct_size=8)), "struct_size"),
            ("draw_frame", dict(spec=spec(draw_frame=1)), "vnect_draw_device"),
            ("an NV12 output", dict(spec=spec(out_format=_native.PIX_NV12)), "out_format"),
            ("a host frame", dict(frame=_native.device_frame(dr.FakeCuda(host_src.ctypes.data, (H, W, 3), (lay["sy"], 3, 1)))), "vnect_infer / vnect_upload_frame"),
            ("has_rect", dict(frame=_native.device_frame(arr, fmt, (0, 0, 10, 10))), "takes no rect"),
            ("a parent of 21", dict(style=bad_parent), "parent"),
            ("a colour of 256", dict(style=bad_colour), "0 .. 255"),
            ("an empty rect", dict(rect=(3, 2, 0, 30)), "at least one pixel"),
            ("a pitch below 3 dw", dict(pitch=3 * dw - 1), "out_pitch"),
            ("an output that overlaps the frame", dict(out=p + 40), "overlaps"),
            ("an output past its allocation's end", dict(out=near_end), "past the end of the allocation"),
            ("a null output", dict(out=0), "no output"),
        ]
        for what, kw, text in cases:
            rc, msg = raw(**kw)
            assert rc == _native.E_ARG and text in msg and msg.startswith("vnect_preview_device: "), (what, rc, msg)
            assert np.array_equal(pool.get(q), canary) and np.array_equal(pool.get(p), src) and (pool.get(other) == 0).all(), what
        hw = (C.c_int32 * 2)()
        for s in (spec(-1.0), spec(0.009), spec(100.0), spec(struct_size=4)):
            assert L.vnect_preview_size(h._h, C.byref(_native.device_frame(arr, fmt)), C.byref(s), hw) == _native.E_ARG
        with pytest.raises(ValueError, match="vnect_preview_device: .*takes no rect"):     # the Python layer: a ValueError, like every refused argument
            h.preview_device(_native.device_frame(arr, fmt, (0, 0, 10, 10)), _native.preview_spec(0.5), q, 3 * dw)
        # and the handle goes on
        assert raw()[0] == 0
        want = _exact(src, lay, 0, dict(case, rect=(3, 2, 40, 30)), 0.5)
        assert np.array_equal(pool.get(q)[:want.size].reshape(want.shape), want) and (pool.get(q)[want.size:] == P.CANARY).all()
        assert np.array_equal(pool.get(p), src)
    finally:
        h.close()


def test_torch_tensors_in_every_layout():
    """a child process that imports torch first: est.preview on packed, permuted, 4-byte, sliced, transposed, RGB and NV12 tensors, to host
    and into a torch `out`, equals render.preview_exact of their host copies, and no tensor's storage changes"""
    r = subprocess.run([sys.executable, "-m", "tests.preview_torch_child"], cwd=R.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "preview child ok"
