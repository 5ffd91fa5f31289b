"""GPU: the pair pyramid of people mode (track.hip: pyramid_track_pair_kernel) behind the tracking probe (`make trackprobe`: the
product's track.o), held byte for byte to two pyramid_track_kernel launches and to oracle.gen_input_batch (PEOPLE.md).

Image i of the (2 S)-image batch is scale i % S of person i / S.  The batch tensor is pre-filled with a garbage byte, so a pixel the kernel
does not write, or a person written at another image's offset, shows.

The people form of the preview kernel (preview.hip: preview_people_kernel) runs behind the preview probe (`make previewprobe`: the
product's preview.o) over the cases of tests/test_people_preview_cpu.py and is held to the numpy composition and to the CPU walk."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import track_cases as tc

pytestmark = pytest.mark.gpu

u8p, f64p, i32p = tc.u8p, tc.f64p, tc.i32p
EL_F32, EL_BF16, EL_F16 = 0, 1, 2
H, W, STRIDE = 480, 800, 3 * 800 + 5
FILL = 0xA5
# (x, y, w, h): 1 x 16 and 17 x 9 (rows x columns), 368 x 368 (squarify is a copy), 400 x 600, and one squarify refuses (1 row of 790 columns)
TINY, SMALL, COPY, BIG, REFUSED = (3, 5, 16, 1), (40, 7, 9, 17), (101, 33, 368, 368), (11, 21, 600, 400), (5, 10, 790, 1)
PAIRS = [(COPY, BIG), (BIG, COPY), (TINY, SMALL), (SMALL, (500, 300, 17, 9)), (BIG, BIG), (REFUSED, BIG), (COPY, REFUSED), (REFUSED, REFUSED)]
ONE, FOUR = [1.0], [1.0, 0.9, 0.8, 0.7]


@pytest.fixture(scope="module")
def probe():
    from vnect_amd import _native
    path = os.environ.get("VNECT_TRACKPROBE_LIB") or _native.TRACKPROBE_LIB
    assert os.path.exists(path), "libvnect_trackprobe.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    L = C.CDLL(path)
    L.tp_pyramid.argtypes = [u8p, C.c_int, C.c_int, C.c_int64, C.c_int, u8p, i32p, f64p, C.c_int, C.c_int, C.c_void_p, i32p]
    L.tp_pyramid_pair.argtypes = [u8p, C.c_int, C.c_int, C.c_int64, C.c_int, u8p, i32p, f64p, C.c_int, C.c_int, C.c_int, C.c_void_p, i32p]
    return L


def _p(a, t):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def scene():
    buf, frame = tc.make_frame(H, W, STRIDE, 11)
    assert tc.squarify_bytes(REFUSED[3], REFUSED[2])[1] is not None and tc.squarify_bytes(BIG[3], BIG[2])[1] is None
    return buf, frame, {}


def _reference(scene, crop, scales):
    """oracle.gen_input_batch of the crop, computed once per (crop, scales)"""
    _, frame, cache = scene
    key = (crop, tuple(scales))
    if key not in cache:
        x, y, w, h = crop
        cache[key] = tc.pyramid_reference(frame[y:y + h, x:x + w], scales)
    return cache[key]


@pytest.mark.parametrize("scales,el", [(tc.BASELINE_SCALES, EL_F32), (tc.BASELINE_SCALES, EL_BF16), (tc.BASELINE_SCALES, EL_F16), (ONE, EL_F32),
                                       (ONE, EL_F16), (FOUR, EL_F32), (FOUR, EL_BF16)])
def test_pair_pyramid_equals_two_single_launches_and_the_oracle(probe, scene, scales, el):
    """overlapping and disjoint crops, one person's crop refused while the other's is valid, from the whole frame and from packed rows"""
    buf, frame, _ = scene
    S = len(scales)
    sc = np.asarray(scales, np.float64)
    again = [PAIRS[0], PAIRS[2], PAIRS[3], PAIRS[5], PAIRS[6]]
    pairs = PAIRS + again                                   # every pair from the frame, then five of them from packed rows
    packed = np.asarray([0] * len(PAIRS) + [1] * len(again), np.int32)
    n = len(pairs)
    states = np.ascontiguousarray(np.stack([tc.frame_state(H, W, c) for pair in pairs for c in pair]))
    dt = np.float32 if el == EL_F32 else np.uint16
    got = np.zeros((n, 2, S, 368, 368, 4), dt)
    err = np.zeros(2 * n, np.int32)
    rc = probe.tp_pyramid_pair(_p(buf, u8p), H, W, STRIDE, n, _p(states, u8p), _p(packed, i32p), _p(sc, f64p), S, el, FILL, got.ctypes.data, _p(err, i32p))
    assert rc == 0, (rc, err)
    single = np.zeros((2 * n, S, 368, 368, 4), dt)
    err1 = np.zeros(2 * n, np.int32)
    each = np.repeat(packed, 2).astype(np.int32)
    rc = probe.tp_pyramid(_p(buf, u8p), H, W, STRIDE, 2 * n, _p(states, u8p), _p(each, i32p), _p(sc, f64p), S, el, single.ctypes.data, _p(err1, i32p))
    assert rc == 0, (rc, err1)
    for i, pair in enumerate(pairs):
        for k, crop in enumerate(pair):
            tag = (pair, "person", k, "packed", int(packed[i]), "el", el, "scales", S)
            assert np.array_equal(got[i, k].view(np.uint8), single[2 * i + k].view(np.uint8)), tag + ("two single launches",)
            want = _reference(scene, crop, scales)
            want = want if el == EL_F32 else tc.to_16(want, el == EL_F16)
            if not np.array_equal(got[i, k].view(np.uint8), want.view(np.uint8)):
                where = np.argwhere(got[i, k] != want)
                raise AssertionError(tag + ("oracle: differing", len(where), "first (s, y, x, c)", where[:4].tolist()))


def test_pair_probe_refuses_bad_cases(probe, scene):
    """a crop outside the frame gets an error code and no launch; more than 8 images are refused"""
    buf, _, _ = scene
    states = np.ascontiguousarray(np.stack([tc.frame_state(H, W, BIG), tc.frame_state(H, W, (750, 2, 100, 10))]))
    err = np.zeros(2, np.int32)
    packed = np.zeros(1, np.int32)
    sc = np.asarray(tc.BASELINE_SCALES, np.float64)
    assert probe.tp_pyramid_pair(_p(buf, u8p), H, W, STRIDE, 1, _p(states, u8p), _p(packed, i32p), _p(sc, f64p), 3, EL_F32, FILL, None, _p(err, i32p)) == 1
    assert err[0] == 0 and err[1] != 0
    five = np.asarray([1.0, 0.9, 0.8, 0.7, 0.6], np.float64)
    assert probe.tp_pyramid_pair(_p(buf, u8p), H, W, STRIDE, 1, _p(states, u8p), _p(packed, i32p), _p(five, f64p), 5, EL_F32, FILL, None, _p(err, i32p)) == -1


# ---- the people preview kernel (preview.hip: preview_people_kernel) behind the preview probe ---------------------------------------------
def test_people_preview_kernel_equals_the_composition_and_the_cpu_walk():
    """the cases of tests/test_people_preview_cpu.py on the device: every job's whole output buffer equals the numpy composition (which
    the CPU walk equals), the guards around it keep their canary and the source is unchanged"""
    from tests import people_preview_ref as PP
    probe = PP.probe_lib()
    lay6 = (C.c_int32 * 6)()
    probe.pp_layout(lay6)
    fill, guard = lay6[0], lay6[1]

    def backend(src, lay, job, joints, rects, conf, out, pitch):
        guards = np.zeros(2 * guard, np.uint8)
        walked = out.copy()
        args, keep = PP.walk_args(src, lay, job, joints, rects, conf, out, pitch, flags=[0] * job[3])
        rc = probe.pp_preview_people(*(args + [guards.ctypes.data_as(u8p)]))
        assert rc == 0, (rc, lay["name"], job[1:])
        assert np.all(guards == fill), (lay["name"], job[1:])
        args, keep = PP.walk_args(src, lay, job, joints, rects, conf, walked, pitch)
        assert PP.cpu_lib().preview_walk_people(*args) == 0 and np.array_equal(out, walked), (lay["name"], job[1:], "CPU walk")

    assert PP.run(backend) == 36


def test_people_preview_kernel_leaves_a_refused_person_out():
    """status != SQ_OK for person 1: the kernel's picture is the CPU walk's with that person not drawn"""
    from tests import people_preview_ref as PP
    from tests import preview_ref as V
    probe = PP.probe_lib()
    lay6 = (C.c_int32 * 6)()
    probe.pp_layout(lay6)
    job = [j for j in PP.jobs() if j[3] == 4 and j[0]["format"] == 2][0]
    lay = job[0]
    src = V.fresh(lay, job[8])
    exp, joints, rects, conf = PP.expected(src, lay, job)
    cpu, pitch = V.out_buffer(exp.shape[0], exp.shape[1], job[6], job[7])
    gpu = cpu.copy()
    args, keep = PP.walk_args(src, lay, job, joints, rects, conf, cpu, pitch, flags=[1, 0, 1, 1])
    assert PP.cpu_lib().preview_walk_people(*args) == 0
    guards = np.zeros(2 * lay6[1], np.uint8)
    args, keep = PP.walk_args(src, lay, job, joints, rects, conf, gpu, pitch, flags=[0, 3, 0, 0])
    assert probe.pp_preview_people(*(args + [guards.ctypes.data_as(u8p)])) == 0
    assert np.array_equal(gpu, cpu) and np.all(guards == lay6[0])
    assert not np.array_equal(gpu, V.whole(exp, job[6], pitch))       # (person 1 was visible in the full picture)
