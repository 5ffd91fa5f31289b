"""Orientation without a GPU (ORIENTATION.md): the rule of vnect_amd/csrc/orient.h held to numpy, the kernels' own tile walk (orient_capi.cpp:
the same functions the kernels of orient.hip call) held to numpy byte for byte with its loads and stores bounded, the same sweep under the
sanitizers as a stand-alone program, the GPU case lists' claims, and the runner's argument rules."""
import os
import subprocess

import numpy as np
import pytest

from . import devframe_ref as dr
from . import orient_ref as orf

pytestmark = pytest.mark.filterwarnings("ignore")


def _all_rects(Ho, Wo):
    return [(x, y, w, h) for y in range(Ho) for x in range(Wo) for h in range(1, Ho - y + 1) for w in range(1, Wo - x + 1)]


def _check_walk(src, o, rect, phase=0):
    x, y, w, h = rect
    got, hits, seen, stray, shared, front = orf.walk(src, o, rect, phase)
    key = (src.key(), o, rect, phase)
    assert stray == 0 and shared == 0, key
    assert np.array_equal(got, src.picture(o)[y:y + h, x:x + w]), key
    assert (hits == 1).all(), key
    assert (front == 0xC7).all(), key
    assert 0 <= seen[0] and seen[1] < src.buf0.size, key
    if src.form == orf.NV12:
        assert 0 <= seen[2] and seen[3] < (src.buf1 if src.two else src.buf0).size, key


def test_the_rule_names_the_reference_options():
    """o = 3 is the reference's T (np.rot90(frame, 3)), o = 7 its commented np.transpose variant, 6 upside down, 4 a mirror, 0 nothing"""
    f = dr.pixels(5, 7, 1)
    assert np.array_equal(orf.oriented(f, 3), np.rot90(f, 3))
    assert np.array_equal(orf.oriented(f, 7), np.transpose(f, (1, 0, 2)))
    assert np.array_equal(orf.oriented(f, 6), f[::-1])
    assert np.array_equal(orf.oriented(f, 4), f[:, ::-1])
    assert np.array_equal(orf.oriented(f, 0), f)
    from vnect_amd import runner
    for o in range(8):
        assert np.array_equal(runner.orient_view(f, o), orf.oriented(f, o))


def test_map_size_and_src_rect_against_numpy():
    """orient.h's closed forms against the rule applied to an index array: every code, every size up to 6, every pixel and every rect"""
    L = orf.cpu_lib()
    out2, out4 = (orf.C.c_int32 * 2)(), (orf.C.c_int32 * 4)()
    for o in range(8):
        for H in range(1, 7):
            for W in range(1, 7):
                m = orf.index_map(o, H, W)
                L.orient_size_c(o, H, W, out2)
                assert tuple(out2) == m.shape[:2] == orf.oriented_size(o, H, W)
                for i in range(m.shape[0]):
                    for j in range(m.shape[1]):
                        L.orient_map_c(o, H, W, i, j, out2)
                        assert tuple(out2) == tuple(m[i, j]), (o, H, W, i, j)
                if H <= 4 and W <= 5:
                    for rect in _all_rects(*m.shape[:2]):
                        L.orient_src_rect_c(o, H, W, *rect, out4)
                        assert tuple(out4) == orf.src_rect(o, H, W, rect), (o, H, W, rect)


def test_walk_every_rect_of_small_frames():
    """codes 1 .. 7 x every (H, W) in 1 .. 6 x every rect, packed BGR, the destination phase going round (the stand-alone sweep below goes
    to 9, through every form)"""
    k = 0
    for o in orf.CODES:
        for H in range(1, 7):
            for W in range(1, 7):
                src = orf.Source(dr.PACKED3, k & 1, H, W, off=k % 4, pad=(0, 1, 5)[k % 3], seed=k)
                for rect in _all_rects(*orf.oriented_size(o, H, W)):
                    _check_walk(src, o, rect, k % 4)
                    k += 1


def test_walk_the_gpu_cases():
    """every case the GPU test runs, walked through the kernels' own tile code on the host: every form and order, the tile seams, odd origins,
    1-pixel crops, every destination phase"""
    n = 0
    for kw, o, phase, _ in orf.gpu_cases():
        src = orf.Source(**kw)
        for rect in orf.seam_rects(*orf.oriented_size(o, kw["H"], kw["W"])):
            _check_walk(src, o, rect, phase)
            n += 1
    assert n > 3000


def test_walk_whole_frames_at_every_phase():
    T = orf.tile()
    for form in range(5):
        H, W = (T + 2, 2 * T + 2) if form == orf.NV12 else (T + 1, 2 * T + 1)
        src = orf.Source(form, 1 if form < 4 else 0, H, W, off=3, pad=5 if form < 4 else 6, two=True, seed=form)
        for o in (1, 3, 6, 7):
            Ho, Wo = orf.oriented_size(o, H, W)
            for phase in range(4):
                _check_walk(src, o, (0, 0, Wo, Ho), phase)
                _check_walk(src, o, (1, 1, Wo - 2, Ho - 2), phase)


def test_walk_refuses_what_the_launcher_refuses():
    src = orf.Source(dr.PACKED3, 0, 4, 6)
    for o, rect in ((0, (0, 0, 1, 1)), (8, (0, 0, 1, 1)), (1, (0, 0, 5, 1)), (1, (0, 0, 4, 7)), (2, (-1, 0, 1, 1)), (2, (0, 0, 0, 1))):
        assert orf.walk(src, o, rect)[3] == -1, (o, rect)


def test_sweep_under_the_sanitizers():
    """the same walk as a stand-alone program with its own main, built with -fsanitize=address,undefined, its sources in exactly sized heap
    blocks: every code x every (H, W) in 1 .. 9 x every rect x every form, the tile seams, every order, against a reference of its own"""
    subprocess.check_call(["make", "-C", dr.CSRC, "orient_sweep_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(dr.LIBDIR, "orient_sweep_asan")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "0 mismatches" in p.stdout and "ERROR" not in p.stderr, p.stdout + p.stderr[-2000:]


def test_gpu_case_lists_cover_what_they_claim():
    T = orf.tile()
    want = {1, T - 1, T, T + 1, 2 * T + 1}
    assert {H for H, _ in orf.seam_sizes()} == want and {W for _, W in orf.seam_sizes()} == want
    even = {2, T - 2, T, T + 2, 2 * T + 2}
    assert {H for H, _ in orf.seam_sizes_nv12()} == even and {W for _, W in orf.seam_sizes_nv12()} == even
    cases = orf.gpu_cases()
    seen = {(kw["form"], kw["order"], kw.get("two", False), o) for kw, o, _, _ in cases}
    for o in orf.CODES:
        for form in range(4):
            for order in (0, 1):
                assert (form, order, False, o) in seen
        assert (orf.NV12, 0, False, o) in seen and (orf.NV12, 0, True, o) in seen
    assert {p for _, _, p, _ in cases} == {0, 1, 2, 3} and {e for _, _, _, e in cases} == {0, 1}
    assert {kw["off"] for kw, _, _, _ in cases} == {0, 1, 2, 3}
    # the rects of the largest picture: a far edge before, on and after a seam, in both axes, from an odd origin; and the 1-pixel crops
    Ho, Wo = 2 * T + 1, 2 * T + 1
    rects = orf.seam_rects(Ho, Wo)
    for x, second in ((1, {2 * T - 1, 2 * T}), (3, set())):     # (from x = 3 the picture ends before the second seam)
        assert {w for (xx, y, w, h) in rects if xx == x and y == 1 and h == 3} >= {T - 1, T, T + 1} | second
    assert {h for (xx, y, w, h) in rects if xx == 1 and y == 1 and w == 3} >= {T - 1, T, T + 1, 2 * T - 1, 2 * T}
    assert (0, 0, Wo, Ho) in rects and (0, 0, 1, 1) in rects and (Wo - 1, Ho - 1, 1, 1) in rects
    assert any(w == Wo and h == 1 for _, _, w, h in rects) and any(w == 1 and h == Ho for _, _, w, h in rects)
    for (H, W) in orf.seam_sizes() + orf.seam_sizes_nv12():
        for o in (1, 2):
            Ho, Wo = orf.oriented_size(o, H, W)
            for (x, y, w, h) in orf.seam_rects(Ho, Wo):
                assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= Wo and y + h <= Ho


class _NoEstimator:
    handle = None
    _cfg = {}
    joint_parents = list(range(21))


def test_runner_argument_rules():
    """transpose keeps its refusals (now pointing at orientation=3), and does not go together with an orientation"""
    from vnect_amd import runner
    frames = [np.zeros((8, 6, 3), np.uint8)]
    with pytest.raises(ValueError, match="transpose"):
        list(runner.track(_NoEstimator(), frames, transpose=True, pixel_format="nv12"))
    with pytest.raises(ValueError, match="transpose"):
        list(runner.track_on_device(_NoEstimator(), frames, transpose=True, source="device"))
    with pytest.raises(ValueError, match="orientation=3"):
        list(runner.track_on_device(_NoEstimator(), frames, transpose=True, pixel_format="nv12"))
    for fn in (runner.track, runner.track_on_device):
        with pytest.raises(ValueError, match="transpose"):
            list(fn(_NoEstimator(), frames, transpose=True, orientation=3))
        for bad in (8, -1, 1.0, True, "3"):
            with pytest.raises((ValueError, TypeError)):
                list(fn(_NoEstimator(), frames, orientation=bad))
    with pytest.raises(ValueError):
        list(runner.track_many_on_device(_NoEstimator(), [frames, frames], orientation=[1]))


def test_runner_track_turns_host_frames_like_transpose():
    """runner.track(orientation=3) on host BGR is runner.track(transpose=True): the same crops reach the estimator"""
    from vnect_amd import runner

    class Rec:
        def __init__(self):
            self.crops = []

        def __call__(self, img, timestamp=None):
            self.crops.append(np.array(img))
            j2 = np.zeros((21, 2))
            j2[:, 0], j2[:, 1] = np.linspace(2, img.shape[0] - 2, 21), np.linspace(1, img.shape[1] - 1, 21)
            return j2, np.zeros((21, 3), np.float32)

    frames = [dr.pixels(40, 56, s) for s in range(4)]
    a, b = Rec(), Rec()
    ra = list(runner.track(a, frames, transpose=True, timestamps=[1, 2, 3, 4]))
    rb = list(runner.track(b, frames, orientation=3, timestamps=[1, 2, 3, 4]))
    assert len(a.crops) == len(b.crops) == 4
    for x, y in zip(a.crops, b.crops):
        assert np.array_equal(x, y)
    for (j2a, _, ua), (j2b, _, ub) in zip(ra, rb):
        assert np.array_equal(j2a, j2b) and list(ua) == list(ub)
    c = Rec()
    list(runner.track(c, frames, orientation=7, timestamps=[1, 2, 3, 4]))
    assert np.array_equal(c.crops[0], np.transpose(frames[0], (1, 0, 2)))


def test_runner_track_defaults_to_the_estimators_own_orientation():
    """orientation=None is the estimator's own code: runner.track turns the host frame itself and then calls the estimator under code 0;
    an explicit code wins; an estimator without the attribute is code 0 and is never handed the kwarg"""
    from vnect_amd import runner

    class Rec:
        orientation = 3

        def __init__(self):
            self.calls = []

        def __call__(self, img, timestamp=None, orientation=None):
            self.calls.append((np.array(img), orientation))
            j2 = np.zeros((21, 2))
            j2[:, 0], j2[:, 1] = np.linspace(2, img.shape[0] - 2, 21), np.linspace(1, img.shape[1] - 1, 21)
            return j2, np.zeros((21, 3), np.float32)

    f = dr.pixels(40, 56, 9)
    a = Rec()
    list(runner.track(a, [f], timestamps=[1]))
    assert np.array_equal(a.calls[0][0], np.rot90(f, 3)) and a.calls[0][1] == 0
    b = Rec()
    list(runner.track(b, [f], timestamps=[1], orientation=0))
    assert np.array_equal(b.calls[0][0], f) and b.calls[0][1] == 0
    c = Rec()
    c.orientation = 0
    list(runner.track(c, [f], timestamps=[1], orientation=6))
    assert np.array_equal(c.calls[0][0], f[::-1]) and c.calls[0][1] is None
    with pytest.raises(ValueError, match="transpose"):
        list(runner.track(a, [f], timestamps=[1], transpose=True))
