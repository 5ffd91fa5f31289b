"""CPU: frames in device memory.  The ABI's new symbols and the descriptor's layout; g++'s build of vnect_amd/csrc/ingest.h -- the lane
windows the copy kernels of post.hip load, permute and store with -- walked wave by wave against the plain numpy gather of
tests/devframe_ref.py, with the lowest and highest byte any lane loads held inside the frame's own buffer; the sanitizer build, a
stand-alone program that is never loaded into python; the Python layer's marshalling of __cuda_array_interface__; and the case lists of
tests/test_gpu_device_ingest_kernels.py against what they claim to cover."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import devframe_ref as dr

u8p, i64p = dr.u8p, dr.i64p


def _p(a, t=u8p):
    return a.ctypes.data_as(t)


NEW = ["vnect_upload_frame_device", "vnect_infer_device", "vnect_preprocess_device", "vnect_submit_tracked_device"]


def test_symbols_and_descriptor_layout(tmp_path):
    from vnect_amd import _native
    hdr = open(os.path.join(dr.ROOT, "include", "vnect_abi.h")).read()
    L = _native.lib()
    for n in NEW:
        assert "int " + n + "(" in hdr and n in _native.SYMBOLS and getattr(L, n)
    assert "vnect_*" in open(os.path.join(dr.CSRC, "vnect.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:
        assert set(NEW) <= {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert _native.ABI_VERSION == 7 and L.vnect_abi_version() == 7 and C.sizeof(_native.Config) == 128   # additive: both stay
    pos = hdr.index("#define VNECT_PIX_BGR")
    doc = hdr[hdr.rindex("/*", 0, pos):pos]
    assert "src/estimator.py:97-99" in doc and "run_estimator_ps.py:88" in doc and "import torch first" in doc
    assert (_native.PIX_BGR, _native.PIX_RGB, _native.PIX_NV12) == tuple(int(re.search(r"#define VNECT_PIX_%s (\d+)" % k, hdr).group(1)) for k in ("BGR", "RGB", "NV12"))
    assert _native.STREAM_SYNCED == 2 ** 64 - 1 and "#define VNECT_STREAM_SYNCED ((void*)-1)" in hdr
    # sizeof and every field offset as the C compiler lays the header's structure out
    fields = [k for k, _ in _native.DeviceFrame._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vnect_abi.h"\nint main(void) {\n  printf("%zu", sizeof(vnect_device_frame));\n'
                   + "".join('  printf(" %%zu", offsetof(vnect_device_frame, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(dr.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_native.DeviceFrame)] + [getattr(_native.DeviceFrame, f).offset for f in fields], got
    # null handles come back as codes
    assert L.vnect_infer_device(None, None, None, 0.0, 0.0, None, None) == _native.E_ARG
    assert L.vnect_upload_frame_device(None, 0, None, None) == _native.E_ARG
    assert L.vnect_submit_tracked_device(None, 0, None, None, 0.0, 0.0) == _native.E_ARG


def _walk(lay, buf, order, rect, phase=0, generic=0):
    """the host walk of one crop: (the packed crop, times each of its bytes was written, the sentinel bytes around it, (lowest, highest)
    buffer offset loaded)"""
    L = dr.cpu_lib()
    x, y, w, h = rect
    n = 3 * w * h
    dst = np.full(phase + n + 64, 0xC7, np.uint8)
    hits = np.zeros(n, np.uint8)
    seen = np.zeros(2, np.int64)
    stray = L.ingest_walk(_p(buf), len(buf), lay.off, lay.H, lay.W, lay.sy, lay.sx, lay.sc, order, generic, x, y, w, h, _p(dst[phase:]), _p(hits), _p(seen, i64p))
    assert stray == 0, (lay.key(), rect, stray)
    return dst[phase:phase + n].reshape(h, w, 3), hits, np.concatenate([dst[:phase], dst[phase + n:]]), (int(seen[0]), int(seen[1]))


def _aligned(nbytes, align):
    """a uint8 array of nbytes whose first byte lies `align` bytes behind a 16-byte boundary"""
    raw = np.zeros(nbytes + 32, np.uint8)
    s = (-raw.ctypes.data) % 16 + align
    return raw[s:s + nbytes]


@pytest.mark.parametrize("form", dr.FORMS, ids=dr.FORM_NAMES)
@pytest.mark.parametrize("order", dr.ORDERS, ids=["bgr", "rgb"])
def test_host_walk_equals_the_gather(form, order):
    """Every source alignment 0..3 x destination phase 0..3 for widths 1 .. two waves' span + 1 (every combination for the widths up to
    24 and around the seams, one combination that moves with the width elsewhere), three rows, the frame flush against BOTH ends of its
    buffer: the walk's bytes are the gather's, every destination byte is written exactly once, the bytes around the crop keep their
    sentinel, and no load leaves the buffer."""
    L = dr.cpu_lib()
    _, wave, wg, gwg = dr.kernel_spans()
    assert L.ingest_classify(*{dr.PACKED3: (3, 1), dr.PACKED4: (4, 1), dr.PLANAR: (1, 777), dr.GENERIC: (5, 2)}[form]) == form
    H = 3
    for W in range(1, 2 * wave + 2):
        near_seam = min(W % wave, wave - W % wave) <= 2
        combos = [(a, p) for a in range(4) for p in range(4)] if W <= 24 or near_seam else [(W % 4, (W // 4) % 4)]
        for align, phase in combos:
            lay = dr.Layout(form, H, W, 0, pad=(W + align) % 3)
            buf = _aligned(lay.cap, align)
            src = dr.pixels(H, W, W * 16 + align * 4 + phase)
            buf[...] = lay.place(src)
            assert buf.ctypes.data % 4 == align and L.ingest_frame_span(H, W, lay.sy, lay.sx, lay.sc) == lay.span == len(buf)
            got, hits, around, seen = _walk(lay, buf, order, (0, 0, W, H), phase)
            want = dr.as_bgr(src, order)
            assert np.array_equal(got, want), (lay.key(), align, phase, np.argwhere(got != want)[:4])
            assert np.all(hits == 1), (lay.key(), align, phase, np.nonzero(hits != 1)[0][:8])
            assert np.all(around == 0xC7), (lay.key(), align, phase)
            assert 0 <= seen[0] and seen[1] < len(buf), (lay.key(), align, seen)      # flush at the start and at the end: nothing outside


@pytest.mark.parametrize("form", dr.FORMS, ids=dr.FORM_NAMES)
def test_host_walk_of_crops_and_the_generic_statement(form):
    """Every crop of the case frame (the GPU test's list), by the form's own walk and by the generic one: both equal the gather."""
    lay = dr.crop_frame(form)
    src = dr.pixels(lay.H, lay.W, 5)
    buf = lay.place(src)
    for order in dr.ORDERS:
        want = dr.as_bgr(src, order)
        for k, (x, y, w, h) in enumerate(dr.crop_rects()):
            for generic in (0, 1):
                got, hits, around, seen = _walk(lay, buf, order, (x, y, w, h), k % 4, generic)
                assert np.array_equal(got, want[y:y + h, x:x + w]) and np.all(hits == 1) and np.all(around == 0xC7), (lay.key(), order, (x, y, w, h), generic)
                assert 0 <= seen[0] and seen[1] < len(buf)


def test_a_wrong_mask_or_permute_would_be_noticed():
    """The walk is not vacuous: a source with one byte changed changes exactly that destination byte."""
    lay = dr.Layout(dr.PLANAR, 2, 9, 3, 2)
    src = dr.pixels(2, 9, 1)
    a, _, _, _ = _walk(lay, lay.place(src), dr.RGB, (0, 0, 9, 2))
    src[1, 7, 0] ^= 0x55
    b, _, _, _ = _walk(lay, lay.place(src), dr.RGB, (0, 0, 9, 2))
    assert np.argwhere(a != b).tolist() == [[1, 7, 2]]


def test_store_rule_at_the_row_starts_of_the_nv12_copies():
    """The store rule driven alone, as nv12_strip drives it: the row's first group starts 0, 3, 6 or 9 bytes in front of the row (NV12 counts
    its groups in frame columns: 3 (x & 3)), every destination phase 0..3, widths 1 .. two waves' span + 1.  The groups' bytes are synthetic,
    a function of the byte's row index: every byte of the row is written exactly once with its value, and nothing outside the row."""
    L = dr.cpu_lib()
    _, wave, _, _ = dr.kernel_spans()
    value = np.array([L.ingest_store_byte(t) for t in range(3 * (2 * wave + 1))], np.uint8)
    assert len(set(value[:12].tolist())) == 12 and value[0] == (12 * 37) % 251     # (neighbouring bytes differ: a shifted store shows)
    for w in range(1, 2 * wave + 2):
        n = 3 * w
        for lead in (0, 3, 6, 9):
            for phase in range(4):
                dst = _aligned(phase + n + 64, 0)
                dst[...] = 0xC7
                hits = np.zeros(n, np.uint8)
                assert L.ingest_store_walk(w, lead, _p(dst[phase:]), _p(hits)) == 0, (w, lead, phase)
                assert np.array_equal(dst[phase:phase + n], value[:n]), (w, lead, phase, np.nonzero(dst[phase:phase + n] != value[:n])[0][:8])
                assert np.all(hits == 1), (w, lead, phase, np.nonzero(hits != 1)[0][:8])
                assert np.all(dst[:phase] == 0xC7) and np.all(dst[phase + n:] == 0xC7), (w, lead, phase)
    assert L.ingest_store_walk(4, 2, _p(dst), None) == -1 and L.ingest_store_walk(4, 12, _p(dst), None) == -1


def test_sanitizer_sweep_is_a_standalone_program():
    """-fsanitize=address,undefined build of the same walk behind its own main, the sources in exactly sized heap blocks (a load outside
    the allocation is the sanitizer's finding).  Built (sanitizer runtimes linked statically) and run here, on the CPU, in the environment
    as it is; nothing of it is loaded into python."""
    subprocess.check_call(["make", "-C", dr.CSRC, "ingest_sweep_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(dr.LIBDIR, "ingest_sweep_asan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    m = re.search(r"ingest sweep: (\d+) walks, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) > 10000 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-2000:])


def test_python_marshalling_of_device_arrays():
    from vnect_amd import _native
    from vnect_amd.estimator import VNectEstimator
    base = 0x7F0000001000
    # packed
    f = _native.device_frame(dr.FakeCuda(base, (37, 53, 3)))
    assert (f.struct_size, f.format, f.H, f.W, f.data) == (C.sizeof(_native.DeviceFrame), _native.PIX_BGR, 37, 53, base)
    assert (f.stride_y, f.stride_x, f.stride_c, f.has_rect) == (159, 3, 1, 0) and _native.device_form(f.stride_x, f.stride_c) == 0
    # bgra[..., :3]
    f = _native.device_frame(dr.FakeCuda(base, (37, 53, 3), (53 * 4, 4, 1)), "rgb")
    assert (f.format, f.stride_y, f.stride_x, f.stride_c) == (_native.PIX_RGB, 212, 4, 1) and _native.device_form(4, 1) == 1
    # chw.permute(1, 2, 0)
    f = _native.device_frame(dr.FakeCuda(base, (37, 53, 3), (53, 1, 37 * 53)))
    assert (f.stride_y, f.stride_x, f.stride_c) == (53, 1, 1961) and _native.device_form(1, 1961) == 2
    # a sliced crop t[5:25, 7:40]: the data pointer is offset, the strides are the whole frame's
    f = _native.device_frame(dr.FakeCuda(base + 5 * 159 + 7 * 3, (20, 33, 3), (159, 3, 1)), rect=(1, 2, 3, 4))
    assert (f.H, f.W, f.data, f.stride_y) == (20, 33, base + 816, 159) and (f.has_rect, list(f.rect)) == (1, [1, 2, 3, 4])
    assert _native.device_form(6, 2) == 3 and _native.FORM_NAMES[3] == "generic"
    for sx, sc in [(3, 1), (4, 1), (1, 1), (1, 99), (5, 2), (3, 2), (4, 2), (2, 1)]:
        assert _native.device_form(sx, sc) == dr.cpu_lib().ingest_classify(sx, sc), (sx, sc)      # the Python statement is ingest.h's
    # NV12: one array, and a (y, uv) pair
    f = _native.device_frame(dr.FakeCuda(base, (12, 20), (24, 1)), "nv12")
    assert (f.format, f.H, f.W, f.stride_y, f.uv, f.uv_stride) == (_native.PIX_NV12, 8, 20, 24, base + 8 * 24, 24)
    f = _native.device_frame((dr.FakeCuda(base, (8, 20), (21, 1)), dr.FakeCuda(base + 4096, (4, 20), (23, 1))), "nv12")
    assert (f.H, f.W, f.data, f.stride_y, f.uv, f.uv_stride) == (8, 20, base, 21, base + 4096, 23)
    assert _native.is_device_array(dr.FakeCuda(base, (2, 2, 3))) and not _native.is_device_array(np.zeros((2, 2, 3), np.uint8))
    # refusals of the Python layer itself
    for bad in [dr.FakeCuda(base, (37, 53, 3), typestr="<f4"), dr.FakeCuda(base, (37, 53, 4)), dr.FakeCuda(base, (37, 53)),
                dr.FakeCuda(base, (37, 53, 3), (159, -3, 1)), dr.FakeCuda(base, (37, 53, 3), (0, 3, 1)), dr.FakeCuda(0, (37, 53, 3))]:
        with pytest.raises(ValueError):
            _native.device_frame(bad)
    with pytest.raises(ValueError):
        _native.device_frame(dr.FakeCuda(base, (10, 20)), "nv12")
    with pytest.raises(ValueError):
        _native.device_frame(dr.FakeCuda(base, (9, 21)), "nv12")
    with pytest.raises(ValueError):
        _native.device_frame(dr.FakeCuda(base, (2, 2, 3)), "yuy2")
    # 'rgb' is for device frames: a numpy array stays a ValueError, before the handle is touched
    est = VNectEstimator.__new__(VNectEstimator)
    est._h, est.verbose, est._submitted = None, False, 0
    with pytest.raises(ValueError, match="rgb"):
        est(np.zeros((4, 4, 3), np.uint8), timestamp=1.0, pixel_format="rgb")
    with pytest.raises(ValueError, match="rgb"):
        est.submit(np.zeros((4, 4, 3), np.uint8), timestamp=1.0, pixel_format="rgb")
    # the producer stream: the default stream unless torch is imported (it is never imported by the package)
    import sys
    if "torch" not in sys.modules:
        assert _native.default_stream() == 0
    assert _native._stream_arg(_native.STREAM_SYNCED).value == 2 ** 64 - 1 and _native.IMPORT_ORDER_HINT.startswith("import torch before vnect_amd")


def test_runner_refuses_transpose_with_device_frames():
    from vnect_amd import runner
    with pytest.raises(ValueError, match="transpose"):
        next(runner.track_on_device(None, [dr.FakeCuda(4096, (6, 4, 3))], transpose=True, source="device"))
    with pytest.raises(ValueError, match="transpose"):
        next(runner.track_many_on_device(None, [[dr.FakeCuda(4096, (6, 4, 3))]], transpose=True, source="device", pixel_format="rgb"))
    with pytest.raises(ValueError, match="source"):
        next(runner.track_on_device(None, [np.zeros((6, 4, 3), np.uint8)], source="vram"))


def test_gpu_case_lists_cover_what_they_claim():
    lane, wave, wg, gwg = dr.kernel_spans()
    assert lane == 4 and wave == 64 * lane and wg % wave == 0 and wg > wave and gwg >= 64
    rects = dr.crop_rects()
    assert len(rects) == len(set(rects)) == 384
    for form in dr.FORMS:
        spans = (gwg,) if form == dr.GENERIC else (wave, wg)
        lays = dr.small_layouts(form)
        assert len({la.key() for la in lays}) == len(lays)
        ws = set(dr.small_widths(form))
        assert {1, 2, 3, 4, 5, 21} <= ws and all({s - 1, s, s + 1} <= ws for s in spans)
        assert {la.H for la in lays} == {1, 2, 3, 5}
        # every width at every source alignment and row pitch; every destination row phase among the rows of the frames of each width class
        assert {(la.W, la.off, la.pad) for la in lays} == {(w, o, p) for w in ws for o in range(4) for p in (0, 1, 5)}
        assert all(la.cap == la.off + la.span for la in lays)
        for w in ws:                                      # rows start at byte 3 w y of the packed destination
            if w % 4 in (1, 3):
                assert {(3 * w * y) % 4 for y in range(5)} == {0, 1, 2, 3}
        assert {(3 * w * y) % 4 for w in ws for y in range(5)} == {0, 1, 2, 3}
        # crops: every origin residue, and both row ends on every dword phase of the source and of the destination
        cf = dr.crop_frame(form)
        assert all(x + w <= cf.W and y + h <= cf.H for x, y, w, h in rects) and cf.off % 4 and cf.pad % 4
        assert {x % 4 for x, _, _, _ in rects} == {0, 1, 2, 3}
        assert {((cf.off + x * cf.sx) % 4, (cf.off + (x + w) * cf.sx) % 4) for x, _, w, _ in rects} >= {(a, b) for a in range(4) for b in range(4)} or cf.sx == 4
        assert {(3 * w) % 4 for _, _, w, _ in rects} == {0, 1, 2, 3}
        # allocation edges: flush at the start, and the last byte on every dword phase of the end
        edges = dr.edge_layouts(form)
        assert any(not fe and la.off == 0 for la, fe in edges)
        assert {la.cap % 4 for la, fe in edges if fe} == {0, 1, 2, 3}
        assert any(la.W > spans[0] for la, _ in edges)
    assert min(dr.SEAM_HEIGHTS) < 65535 < max(dr.SEAM_HEIGHTS) and dr.SEAM_HEIGHTS == list(range(65531, 65541)) and dr.SEAM_WIDTHS == [1, 2]
    assert max(3 * w * h for w in dr.SEAM_WIDTHS for h in dr.SEAM_HEIGHTS) < 400 * 1024
