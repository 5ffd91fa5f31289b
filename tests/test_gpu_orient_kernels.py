"""The oriented copies of orient.hip on the GPU, case by case (ORIENTATION.md).

The product's own orient.o, linked behind a test shim (`make orientprobe`: vnect_amd/csrc/orient_probe.hip; the product never loads it),
runs tests/orient_ref.py's case lists: codes 1 .. 7 x packed-3, packed-4, planar and generic strides x BGR and RGB, and NV12 in one and in
two allocations, over frames of 1, T - 1, T, T + 1 and 2 T + 1 pixels per axis -- whole frames, crops at odd origins whose edges fall on,
before and after a tile seam, 1 x 1, 1 x w and h x 1 crops -- in the argument form and in the TrackState form.  Every source lies in a
device allocation of exactly its size, flush with its start or its end; every destination is canary-filled between guard zones, at
phases 0 .. 3.  The bytes must equal numpy's oriented crop, everything else must still hold the canary, and a case the shim refuses is a
failure.  tests/test_orient_cpu.py walks the same cases through the kernels' tile code on the host first."""
import ctypes as C

import numpy as np
import pytest

from . import orient_ref as orf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return orf.load_probe()


def _run(probe, src, o, rects, tracked, phase, flush_end):
    n = len(rects)
    cap = max(3 * w * h for _, _, w, h in rects) + phase
    dst_cap = (cap + 63) // 64 * 64
    region = dst_cap + 2 * probe.guard
    out = np.zeros(n * region, np.uint8)
    err = np.zeros(n, np.int32)
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(tracked, np.int32))
    b1 = src.buf1
    rc = probe.op_copy(src.buf0.ctypes.data_as(orf.u8p), src.buf0.size, src.off0, None if b1 is None else b1.ctypes.data_as(orf.u8p),
                       0 if b1 is None else b1.size, src.off1, flush_end, src.form, src.order, src.sy, src.sx, src.sc, o, src.H, src.W, n,
                       r.ctypes.data_as(orf.i32p), t.ctypes.data_as(orf.i32p), phase, dst_cap, out.ctypes.data_as(orf.u8p), err.ctypes.data_as(orf.i32p))
    assert rc == 0, (src.key(), o, rc, err.tolist())       # a refused case is a failure
    return out.reshape(n, region), dst_cap


@pytest.mark.parametrize("code", orf.CODES)
def test_oriented_copies_case_by_case(probe, code):
    groups = [g for g in orf.gpu_cases() if g[1] == code]
    assert groups
    checked = 0
    for kw, o, phase, flush_end in groups:
        src = orf.Source(**kw)
        pic = src.picture(o)
        rects = orf.seam_rects(*pic.shape[:2])
        for tracked in (0, 1):
            got, dst_cap = _run(probe, src, o, rects, [tracked] * len(rects), phase, flush_end)
            for i, rect in enumerate(rects):
                want = orf.expected_region(pic, rect, dst_cap, probe.fill, probe.guard, phase)
                if not np.array_equal(got[i], want):
                    bad = np.flatnonzero(got[i] != want)
                    raise AssertionError("%r code %d rect %r tracked %d phase %d: %d bytes differ, first at region byte %d (crop starts at %d)"
                                         % (src.key(), o, rect, tracked, phase, bad.size, bad[0], probe.guard + phase))
                checked += 1
    assert checked > 500


def test_refused_cases_launch_nothing(probe):
    """the shim's own validation: a rect outside the oriented picture, a frame past its buffer, no room -- each is reported, none is launched"""
    src = orf.Source(0, 0, 6, 10)
    out, err = np.zeros(4096, np.uint8), np.zeros(1, np.int32)

    def call(o, rect, cap0=None, dst_cap=1024):
        r = np.asarray(rect, np.int32)
        return probe.op_copy(src.buf0.ctypes.data_as(orf.u8p), src.buf0.size if cap0 is None else cap0, 0, None, 0, 0, 0, 0, 0, src.sy, src.sx, src.sc,
                             o, 6, 10, 1, r.ctypes.data_as(orf.i32p), np.zeros(1, np.int32).ctypes.data_as(orf.i32p), 0, dst_cap,
                             out.ctypes.data_as(orf.u8p), err.ctypes.data_as(orf.i32p)), int(err[0])
    assert call(1, (0, 0, 7, 1)) == (1, 2)          # the picture of code 1 is (10, 6): 7 columns do not exist
    assert call(2, (0, 0, 10, 7)) == (1, 2)
    assert call(0, (0, 0, 1, 1)) == (1, 1) and call(8, (0, 0, 1, 1)) == (1, 1)
    assert call(1, (0, 0, 6, 10), cap0=src.buf0.size - 1) == (1, 1)
    assert call(1, (0, 0, 6, 10), dst_cap=128) == (1, 3)
    assert call(1, (0, 0, 6, 10)) == (0, 0)
