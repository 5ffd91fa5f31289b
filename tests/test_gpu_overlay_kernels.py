"""GPU: the overlay kernel of overlay.hip alone, byte for byte against tests/overlay_ref.py (the independent numpy statement of the rule,
OVERLAY.md).

The product's own overlay.o, linked behind a test shim (`make overlayprobe`: vnect_amd/csrc/overlay_probe.hip; the product never loads it),
is driven case by case.  Every frame lies in a device buffer with a guard zone in front of and behind it; afterwards the WHOLE buffer --
pixels, row padding, fourth bytes -- must equal the reference's, and both guards must still hold their canary.  The cases and layouts are
those of tests/test_overlay_cpu.py; the tile seams are derived from the tile the probe reports.  No case is skipped: one the shim refuses
fails."""
import numpy as np
import pytest

from tests import overlay_ref as R

pytestmark = pytest.mark.gpu

LAYOUT_NAMES = [lay["name"] for lay in R.layouts(*R.SIZES[0])]


@pytest.fixture(scope="module")
def probe():
    L = R.probe_lib()
    lay = np.zeros(5, np.int32)
    L.op_layout(lay.ctypes.data_as(R.i32p))
    L.fill, L.guard, L.tile_w, L.tile_h = (int(v) for v in lay[:4])
    t = np.zeros(3, np.int32)
    R.cpu_lib().overlay_tile(t.ctypes.data_as(R.i32p))
    assert tuple(lay[2:5]) == tuple(t)          # the probe and the CPU shim were built from one overlay.h
    return L


def _draw(probe, lay, case, tracked=0, status=0, **kw):
    """the case drawn on the device into a fresh buffer of the layout -> the buffer afterwards; the guards are checked here"""
    buf = R.fresh(lay)
    guards = np.zeros(2 * probe.guard, np.uint8)
    args, keep = R.walk_args(buf, lay, case, **kw)
    rc = probe.op_draw(*args, tracked, status, guards.ctypes.data_as(R.u8p))
    assert rc == 0, (rc, lay["name"], case["name"])          # a case the shim refuses is a failure, not a skip
    assert (guards == probe.fill).all(), (lay["name"], case["name"], "a guard byte was written", np.nonzero(guards != probe.fill)[0][:8])
    return buf


def _check(probe, lay, case, tracked=0, **kw):
    want = R.fresh(lay)
    drawn = R.draw(want, lay, case, **kw)
    assert (drawn == 0) == case["empty"], (case["name"], drawn)
    got = _draw(probe, lay, case, tracked, **kw)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError((lay["name"], case["name"], "tracked", tracked, "differing bytes", len(bad), "first at", int(bad[0]), "got", got[bad[:6]],
                              "want", want[bad[:6]]))


@pytest.mark.parametrize("size", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
@pytest.mark.parametrize("layout", range(len(LAYOUT_NAMES)), ids=LAYOUT_NAMES)
def test_every_case_in_every_layout_equals_the_rule(probe, size, layout):
    lay = R.layouts(*size)[layout]
    for case in R.cases(*size):
        _check(probe, lay, case)


def test_the_tracked_form_reads_joints_rect_and_confidences_on_the_device(probe):
    """the same kernel with its inputs in JointsOut / TrackOut / ConfOut structures in device memory, as the tracked submit launches it; a
    frame whose status is not OK is not drawn"""
    H, W = R.SIZES[1]
    for lay in R.layouts(H, W):
        for case in R.cases(H, W):
            if case["rect"] is not None:
                _check(probe, lay, case, tracked=1)
        refused = [c for c in R.cases(H, W) if c["name"] == "skeleton"][0]
        for status in (1, 2, 3):
            assert np.array_equal(_draw(probe, lay, refused, tracked=1, status=status), R.fresh(lay)), (lay["name"], status)


def test_tile_seams(probe):
    """A limb and a band corner across the kernel's tile boundaries in both axes, in pixels and in NV12's 2 x 2 cells: frames of 2 x 2
    tiles and a bit, shapes centred on the seams and ending exactly on either side of them."""
    for nv12 in (False, True):
        px = 2 if nv12 else 1
        tw, th = probe.tile_w * px, probe.tile_h * px            # the tile in pixels
        H, W = 2 * th + 6, 2 * tw + 10
        lays = [lay for lay in R.layouts(H, W) if (lay["format"] == 2) == nv12 and lay["name"] in ("packed3_padded", "planar", "nv12_pitched_odd_base")]
        assert lays and all((lay["H"], lay["W"]) == (H, W) for lay in lays)
        cs = [
            R._case("seam_cross_%d" % nv12, [(th - 9, tw - 21, th + 10, tw + 19), (th + 7, tw - 13, th - 8, tw + 11)]),
            R._case("seam_along_%d" % nv12, [(th, 5, th, W - 6), (4, tw, H - 5, tw), (th - 1, 9, th - 1, W - 12), (7, tw - 1, H - 9, tw - 1)]),
            R._case("seam_ends_%d" % nv12, [(th - 4, 10, th - 4, tw - 1), (th + 3, tw, th + 3, 2 * tw - 1), (10, tw + 3, th - 1, tw + 3), (th, tw - 4, 2 * th - 1, tw - 4)]),
            R._case("seam_band_corner_%d" % nv12, rect=(tw - 1, th - 1, tw // 2, th // 2)),
            R._case("seam_band_inside_%d" % nv12, [(th - 5, tw - 30, th + 5, tw + 30)], rect=(tw + 2, th + 2, tw - 4, th - 4)),
            R._case("seam_band_around_%d" % nv12, rect=(2, 2, 2 * tw, 2 * th)),
        ]
        for lay in lays:
            for case in cs:
                _check(probe, lay, case)
                if case["rect"] is not None:
                    _check(probe, lay, case, tracked=1)


def test_colours_and_the_shims_refusals(probe):
    H, W = R.SIZES[0]
    for lay in R.layouts(H, W):
        case = dict(R.cases(H, W)[-1], name="skeleton_gpu_coloured_%s" % lay["name"])
        _check(probe, lay, case, limb_bgr=(1, 2, 3), rect_bgr=(250, 128, 7))
    lay = R.layouts(H, W)[0]
    ok = R.cases(H, W)[0]
    guards = np.zeros(2 * probe.guard, np.uint8)
    for bad, short in [(dict(ok, parents=[21] + list(range(1, 21))), 0), (dict(ok, rect=(3, 3, 0, 5)), 0), (ok, 1)]:
        buf = R.fresh(lay)
        args, keep = R.walk_args(buf[:len(buf) - short], lay, bad)
        assert probe.op_draw(*args, 0, 0, guards.ctypes.data_as(R.u8p)) == 1 and np.array_equal(buf, R.fresh(lay))
