"""GPU: the kernel of view3d.hip alone, byte for byte against the numpy statement of the rule (tests/view3d_ref.py; VIEW3D.md).

The product's own view3d.o, linked behind a test shim (`make view3dprobe`: vnect_amd/csrc/view3d_probe.hip; the product never loads it), is
driven case by case.  The output lies in a device buffer with a guard zone in front of and behind it; afterwards the WHOLE output buffer
-- rows, pitch padding, the bytes in front of the first row -- must equal the reference's and both guards must still hold their canary.
The cases are those of tests/test_view3d_cpu.py at the sizes where the kernel can go wrong: one pixel, one short row, one pixel more than a
tile in each axis, one pixel less than two tiles in each axis (the tile is the one the probe reports).  Both forms of the launcher run:
inputs in device memory, and inputs in a result-ring slot's structures in pinned host memory.  No case is skipped: one the shim refuses
fails."""
import numpy as np
import pytest

from tests import view3d_ref as V

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def _expected(size, n):
    """the reference of case n at `size`, computed once"""
    if (size, n) not in _EXPECTED:
        _EXPECTED[(size, n)] = V.expected(V.cases(*size)[n], *size)
    return _EXPECTED[(size, n)]


@pytest.fixture(scope="module")
def probe():
    L = V.probe_lib()
    lay = np.zeros(6, np.int32)
    L.vp_layout(lay.ctypes.data_as(V.i32p))
    L.fill, L.guard = int(lay[0]), int(lay[1])
    assert tuple(int(v) for v in lay[2:6]) == V.tile()[:4]          # the probe and the CPU shim were built from one view3d.h
    return L


def _run(probe, case, rows, cols, out, off, pitch, form=0, status=0):
    args, keep = V.walk_args(case, rows, cols, out, off, pitch)
    guards = np.zeros(2 * probe.guard, np.uint8)
    rc = probe.vp_view3d(*args, form, status, guards.ctypes.data_as(V.u8p))
    assert rc == 0, rc
    assert (guards == probe.fill).all(), "a guard zone was written"


def _sizes():
    tw, th = V.tile()[:2]
    return [(1, 1), (1, 7), (th + 1, tw + 1), (2 * th - 1, 2 * tw - 1)]


@pytest.mark.parametrize("which", range(4), ids=["1x1", "1x7", "tile+1", "two_tiles-1"])
def test_every_case_equals_the_numpy_statement(probe, which):
    size = _sizes()[which]
    rows, cols = size
    drawn = 0
    for n, case in enumerate(V.cases(rows, cols)):
        exp = _expected(size, n)
        drawn += int((exp != exp[0, 0]).any(axis=2).sum())
        for pad in V.PADS:
            out, pitch = V.out_buffer(rows, cols, n % 4, pad)
            _run(probe, case, rows, cols, out, n % 4, pitch, form=(n + pad) % 2)
            assert np.array_equal(out, V.whole(exp, n % 4, pitch)), (size, n, pad)
    if which >= 2:
        assert drawn > 20 * len(V.cases(rows, cols))


def test_every_alignment_and_pitch_in_both_forms(probe):
    """`out` at byte offsets 0 .. 3 from a 4-byte boundary with all three pitches: heads, tails and odd pitches take byte stores"""
    size = _sizes()[3]
    rows, cols = size
    for n in (1, 13):                       # the identity under order 1; the threshold case
        case = V.cases(rows, cols)[n]
        exp = _expected(size, n)
        for off in range(4):
            for pad in V.PADS:
                for form in (0, 1):
                    out, pitch = V.out_buffer(rows, cols, off, pad)
                    _run(probe, case, rows, cols, out, off, pitch, form=form)
                    assert np.array_equal(out, V.whole(exp, off, pitch)), (n, off, pad, form)


def test_the_default_size_from_a_ring_slot(probe):
    """400 x 400, the reference's view, its inputs read from pinned host memory"""
    size = (400, 400)
    case = V.cases(*size)[0]
    out, pitch = V.out_buffer(400, 400, 0, 0)
    _run(probe, case, 400, 400, out, 0, pitch, form=1)
    assert np.array_equal(out, V.whole(_expected(size, 0), 0, pitch))


def test_a_refused_status_writes_nothing(probe):
    rows, cols = _sizes()[2]
    case = V.cases(rows, cols)[0]
    for status in (1, 2):
        out, pitch = V.out_buffer(rows, cols, 1, 5)
        _run(probe, case, rows, cols, out, 1, pitch, form=1, status=status)
        assert (out == V.CANARY).all(), status
