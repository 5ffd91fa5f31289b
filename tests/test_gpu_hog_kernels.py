"""GPU: the three kernels of hog.hip alone, bit for bit against the numpy statement of the rule (tests/hog_ref.py; HOG.md).

The product's own hog.o, linked behind a test shim (`make hogprobe`: vnect_amd/csrc/hog_probe.hip; the product never loads it), is driven
case by case.  The frame lies in a device buffer of its own (NV12 in two planes: in two); every workspace buffer the launches write --
votes, bins, blocks, scores, hits, the counter -- lies between guard zones, which must still hold their canary afterwards; the frame is
read back and must be unchanged.  Each stage's output equals the CPU statement's: votes and block descriptors as float32 bits, every
window's score, the hits in the order (level, y, x).  The shapes are the smallest at which each thing can go wrong.  No case is skipped:
one the shim refuses fails."""
import numpy as np
import pytest

from tests import hog_ref as R
from tests import preview_ref as P

pytestmark = pytest.mark.gpu

STAGES = ("votes", "bins", "blocks", "scores")


@pytest.fixture(scope="module")
def probe():
    L = R.probe_lib()
    lay = np.zeros(6, np.int32)
    L.hp_layout(lay.ctypes.data_as(R.i32p))
    assert tuple(int(v) for v in lay[2:6]) == R.tile()              # the probe and the CPU shim were built from one hog.h
    return L


DET = R.seeded_detector(1, rho=0.05, scale=0.04)


def _run(pic, lay, o, s, det=DET, buf=None, what=None):
    buf = R.lay_from_picture(pic, lay, o) if buf is None else buf
    before = buf.copy()
    ref = R.detect(pic, det, s)
    rc, got = R.probe(buf, lay, o, det, s)
    assert rc == 0, (what, rc)
    assert got["guard_damage"] == 0, (what, "a guard byte was written")
    assert np.array_equal(buf, before), (what, "the frame was written")
    assert got["launches"] == (3 if ref["levels"] else 0), what
    R.assert_stages_equal(got, ref, what, STAGES)
    assert got["count"] == len(ref["hits"]), what
    return ref, got


@pytest.mark.parametrize("shape", [(128, 64), (129, 65), (135, 71), (136, 72), (200, 100)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_each_stage_equals_the_cpu_statement(probe, shape):
    """64 x 128: one window, one level, reflect borders on all four sides; 65 x 129 and 71 x 135: trailing partial cells; 72 x 136: 2 x 2
    windows sharing blocks; 100 x 200: ten levels at the defaults"""
    H, W = shape
    ref, got = _run(R.textured(H, W, seed=H), R.packed(H, W), 0, R.spec(), what=shape)
    assert len(ref["levels"]) == {128: 1, 129: 1, 135: 2, 136: 2, 200: 10}[H]
    if shape == (136, 72):
        assert ref["scores"][0].shape == (2, 2)


def test_a_picture_smaller_than_the_window_launches_nothing(probe):
    for H, W in ((128, 63), (127, 64)):
        ref, got = _run(R.textured(H, W), R.packed(H, W), 0, R.spec(), what=(H, W))
        assert not ref["levels"] and got["launches"] == 0 and got["count"] == 0


def test_tile_seams(probe):
    """one width and one height that straddle each kernel's tile seam, from the tile sizes the probe reports: the vote tile is tw x th
    pixels -- a level of tw + 1 columns and th * k + 1 rows has a one-pixel tile column and a one-row tile row; blocks and windows go four
    to a workgroup -- a level whose block count and window count are 1 more than a multiple of four ends in a workgroup with one wave at work"""
    _, tw, th, per = R.tile()
    W, H = tw + 1, 128 + th + 1                                       # 65 x 133: 2 tile columns, the last one pixel wide; the last tile row one row high
    assert W % tw == 1 and H % th == 1
    ref, _ = _run(R.textured(H, W, seed=9), R.packed(H, W), 0, R.spec(nlevels=1), what="vote seam")
    # blocks: nbx * nby = (W / 8 - 1) * (H / 8 - 1); windows: ((W - 64) / 8 + 1) * ((H - 128) / 8 + 1) -- the first size at which both
    # counts are 1 more than a multiple of `per`
    found = None
    for w in range(64, 64 + 8 * 12, 8):
        for h in range(128, 128 + 8 * 12, 8):
            nb, nw = (w // 8 - 1) * (h // 8 - 1), ((w - 64) // 8 + 1) * ((h - 128) // 8 + 1)
            if nb % per == 1 and nw % per == 1 and nw > per and found is None:
                found = (h, w)
    assert found is not None
    H, W = found
    _run(R.textured(H, W, seed=10), R.packed(H, W), 0, R.spec(nlevels=1), what=("block and window seam", found))


@pytest.mark.parametrize("kw", [dict(win_stride=(16, 8)), dict(scale0=1.2), dict(nlevels=1)], ids=["stride16x8", "scale1.2", "nlevels1"])
def test_spec_variants(probe, kw):
    ref, _ = _run(R.textured(152, 88, seed=3), R.packed(152, 88), 0, R.spec(**kw), what=kw)
    if "win_stride" in kw:
        assert ref["scores"][0].shape == (4, 2)
    if "nlevels" in kw:
        assert len(ref["levels"]) == 1


@pytest.mark.parametrize("name", ["packed3_base0", "rgb_packed4_odd_base", "planar", "nv12_pitched_odd_base", "nv12_two_planes"])
def test_source_layouts(probe, name):
    """packed BGR, 4-byte RGB, planar and NV12 (one buffer; two planes in two allocations) sources at 72 x 136"""
    lay = [l for l in P.layouts(136, 72) if l["name"] == name][0]
    if lay["format"] == 2:
        buf = P.fresh(lay)
        _run(P.picture(buf, lay, 0), lay, 0, R.spec(), buf=buf, what=name)
    else:
        _run(R.textured(136, 72, seed=6), lay, 0, R.spec(), what=name)


@pytest.mark.parametrize("o", [0, 3, 5])
def test_orientation_codes(probe, o):
    pic = R.textured(136, 72, seed=7)
    Hs, Ws = (72, 136) if o & 1 else (136, 72)
    _run(pic, R.packed(Hs, Ws), o, R.spec(), what=("code", o))


def test_more_hits_than_max_hits_is_refused_with_the_guards_intact(probe):
    """a detector with a large positive rho on 100 x 200: every window hits; max_hits below the window count -> the call is refused, the
    counter holds the full count, nothing lies behind the hit list's last entry"""
    lay = R.packed(200, 100)
    pic = R.textured(200, 100)
    hot = DET.copy()
    hot[3780] = 1000.0
    nwin = int(R.sizes_of(lay, 0, R.spec())[4][2])
    buf = R.lay_from_picture(pic, lay, 0)
    rc, got = R.probe(buf, lay, 0, hot, R.spec(max_hits=nwin - 1))
    assert rc == 2 and got["count"] == nwin and got["guard_damage"] == 0 and not got["hits"].size
    rc, got = R.probe(buf, lay, 0, hot, R.spec(max_hits=7))
    assert rc == 2 and got["count"] == nwin and got["guard_damage"] == 0
    rc, got = R.probe(buf, lay, 0, hot, R.spec(max_hits=nwin))
    assert rc == 0 and len(got["hits"]) == nwin and got["guard_damage"] == 0
