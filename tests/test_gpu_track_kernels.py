"""GPU: the device tracking kernels, one by one, against references that do not come from the code under test.

tests/test_track_cpu.py holds g++'s build of crop.h to the host path; tests/test_gpu_track.py holds the device end to end, through
planted videos (about a hundred crop sizes).  Here the product's own kernel objects (track.o, post.o -- linked behind a test shim,
`make trackprobe`: vnect_amd/csrc/track_probe.cpp) are driven case by case: the box stage (track_box_kernel: the joints' shift, the box
rule, the fallback, the next crop's whole FrameParams, the refusals), the crop copy out of a pinned frame (frame_copy_track_kernel) and
the tracked pyramid (pyramid_track_kernel).  Everything is exact arithmetic: every comparison is bit for bit.  The case sets and their
references are in tests/track_cases.py; tests/test_track_cases_cpu.py asserts, without a GPU, that they cover what they claim.
No case is skipped or filtered: a case the shim refuses to launch fails the test."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import track_cases as tc

pytestmark = pytest.mark.gpu

u8p, f64p, i32p, u32p = tc.u8p, tc.f64p, tc.i32p, tc.u32p
EL_F32, EL_BF16, EL_F16 = 0, 1, 2


@pytest.fixture(scope="module")
def probe():
    from vnect_amd import _native
    path = os.environ.get("VNECT_TRACKPROBE_LIB") or _native.TRACKPROBE_LIB
    assert os.path.exists(path), "libvnect_trackprobe.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    L = C.CDLL(path)
    L.tp_box.argtypes = [C.c_int, u8p, f64p, u32p, u8p, i32p, f64p, i32p]
    L.tp_copy.argtypes = [u8p, C.c_int, C.c_int, C.c_int64, C.c_int, u8p, C.c_int64, u8p, i32p]
    L.tp_pyramid.argtypes = [u8p, C.c_int, C.c_int, C.c_int64, C.c_int, u8p, i32p, f64p, C.c_int, C.c_int, C.c_void_p, i32p]
    lay = (C.c_int32 * 7)()
    L.tp_layout(lay)
    assert list(lay)[:3] == [tc.STATE_BYTES, 4 * tc.HDR_INTS, tc.FP_BYTES] and lay[3] == 24 and lay[4] == tc.GARBAGE, list(lay)
    L.dst_fill, L.dst_guard = lay[5], lay[6]
    return L


def _p(a, t):
    return a.ctypes.data_as(t)


def _run_box(probe, cases):
    n = len(cases["hdr"])
    states = tc.pack_states(cases["hdr"])
    joints = np.ascontiguousarray(cases["joints"], np.float64)
    xseq = np.ascontiguousarray(cases["xseq"], np.uint32)
    s_out, t_out = np.zeros((n, tc.STATE_BYTES), np.uint8), np.zeros((n, 6), np.int32)
    j_out, err = np.zeros((n, 21, 2), np.float64), np.zeros(n, np.int32)
    rc = probe.tp_box(n, _p(states, u8p), _p(joints, f64p), _p(xseq, u32p), _p(s_out, u8p), _p(t_out, i32p), _p(j_out, f64p), _p(err, i32p))
    assert rc == 0, (rc, np.nonzero(err)[0][:8], err[np.nonzero(err)[0][:8]])   # a case the shim refuses is a failure, not a skip
    return s_out, t_out, j_out


def _first_bad(mask):
    return int(np.nonzero(mask)[0][0])


def _assert_box(probe, cases, ref, what):
    s_out, t_out, j_out = _run_box(probe, cases)
    hp = tc.hostplan()
    nh = 4 * tc.HDR_INTS
    # the joints: numpy float64 j + (y, x), or untouched for a state that arrives refused
    bad = np.any(j_out.view(np.uint64) != ref["joints"].view(np.uint64), axis=(1, 2))
    assert not bad.any(), (what, "joints", _first_bad(bad), cases["hdr"][_first_bad(bad)])
    # rect_used (x, y, uw, uh) and the frame's own status
    bad = np.any(t_out[:, :5] != ref["tout"], axis=1)
    assert not bad.any(), (what, "tout", _first_bad(bad), t_out[_first_bad(bad)], ref["tout"][_first_bad(bad)])
    # the next crop, uw / uh, the frame's size, status and fail == xseq + 1 exactly when the crop is refused
    got_hdr = np.ascontiguousarray(s_out[:, :nh]).view(np.int32)
    bad = np.any(got_hdr != ref["hdr"], axis=1)
    assert not bad.any(), (what, "state", _first_bad(bad), cases["hdr"][_first_bad(bad)], got_hdr[_first_bad(bad)], ref["hdr"][_first_bad(bad)])
    # the FrameParams, byte for byte: hostplan.h's squarify of the new (h, w); zeros for a refused crop; the shim's garbage where the box
    # stage must not write (an entry no thread wrote would keep it)
    bad = np.any(s_out[:, nh:] != ref["states"][:, nh:], axis=1)
    if bad.any():
        i = _first_bad(bad)
        where = np.nonzero(s_out[i, nh:] != ref["states"][i, nh:])[0]
        raise AssertionError((what, "FrameParams", i, "next crop (x, y, w, h)", list(ref["hdr"][i, :4]), "differing bytes", len(where), where[:12],
                              s_out[i, nh:][where[:12]], ref["states"][i, nh:][where[:12]]))
    # the refusal's text through crop_refusal, for every status the device wrote
    for code in np.unique(got_hdr[:, 8]):
        text = hp.hp_crop_refusal(int(code))
        want = {v: k for k, v in tc.CODE_OF.items()}[int(code)]
        assert (text.decode() if text else None) == want, (code, text, want)
    return got_hdr


def test_box_stage_equals_the_references(probe):
    """More than 20 000 joint sets in frames up to 8192 x 8192 plus the targeted lists (tests/track_cases.py: box_cases; their conditions in
    tests/test_track_cases_cpu.py): joints, rect_used, the next crop, its FrameParams bytes, status, fail -- and track_refused for the
    states that arrive refused."""
    cases = tc.box_cases()
    ref = tc.box_reference(cases)
    got = _assert_box(probe, cases, ref, "box")
    refused = got[:, 8] != 0
    live = ref["info"]["status"] >= 0
    assert np.array_equal(got[live & refused, 9].view(np.uint32), cases["xseq"][live & refused] + np.uint32(1))
    assert np.all(got[live & ~refused, 9] == 0) and (live & refused).sum() >= 200


def test_geometry_sweep_on_the_device(probe):
    """The device twin of test_shared_geometry_equals_host_squarify_*: every (h, w) of tests/test_track_cpu.py's dense and random size sets
    through the box stage (joints for which runner.bbox_update gives exactly [0, 0, w, h]); the device's FrameParams equal hostplan.h's
    byte for byte, refusals included."""
    sizes = tc.dense_sizes() + tc.random_sizes()
    refused = 0
    for c0 in range(0, len(sizes), 16384):
        cases = tc.sweep_cases(sizes[c0:c0 + 16384])
        ref = tc.box_reference(cases)
        want = np.asarray([[0, 0, w, h] for h, w in sizes[c0:c0 + 16384]], np.int32)
        assert np.array_equal(ref["hdr"][:, :4], want)
        got = _assert_box(probe, cases, ref, ("sweep", c0))
        refused += int((got[:, 8] != 0).sum())
    assert refused > 100


def test_box_probe_refuses_bad_cases(probe):
    """The shim validates before it launches: non-finite or huge joints and an unknown status get an error code and nothing runs."""
    cases = tc.sweep_cases([(10, 10)] * 4)
    cases["joints"][1, 3, 0] = np.nan
    cases["joints"][2, 0, 1] = 2e9
    cases["hdr"][3, 8] = 7
    n = 4
    states = tc.pack_states(cases["hdr"])
    s_out, t_out = np.full((n, tc.STATE_BYTES), 0x11, np.uint8), np.zeros((n, 6), np.int32)
    j_out, err = np.zeros((n, 21, 2), np.float64), np.zeros(n, np.int32)
    rc = probe.tp_box(n, _p(states, u8p), _p(cases["joints"], f64p), _p(cases["xseq"], u32p), _p(s_out, u8p), _p(t_out, i32p), _p(j_out, f64p),
                      _p(err, i32p))
    assert rc == 3 and err[0] == 0 and all(err[1:] != 0) and np.all(s_out == 0x11), (rc, err)


# ---- crop copy ------------------------------------------------------------------------------------------------------------------------
def _states_for(H, W, crops):
    return np.ascontiguousarray(np.stack([tc.frame_state(H, W, c) for c in crops]))


def test_crop_copy_equals_numpy_slicing(probe):
    """frame_copy_track_kernel out of a pinned frame, at every x mod 4 / w mod 4 / destination row phase, 1, 2 and more than 6 workgroups
    per row, up to an 8192-wide frame, crops ending in the frame's last row and last byte (the src_end guard): the crop's 3 w h bytes equal
    frame[y:y+h, x:x+w].tobytes(), and every other byte of the pre-filled destination and its guards is untouched."""
    for f in tc.copy_cases():
        H, W, stride = f["H"], f["W"], f["stride"]
        buf, frame = tc.make_frame(H, W, stride, f["seed"])
        crops = f["crops"]
        n = len(crops)
        states = _states_for(H, W, crops)
        cap = (max(3 * w * h for _, _, w, h in crops) + 63) // 64 * 64 + 64
        region = cap + 2 * probe.dst_guard
        out, err = np.zeros((n, region), np.uint8), np.zeros(n, np.int32)
        rc = probe.tp_copy(_p(buf, u8p), H, W, stride, n, _p(states, u8p), cap, _p(out, u8p), _p(err, i32p))
        assert rc == 0, (rc, (H, W), [(crops[i], int(err[i])) for i in np.nonzero(err)[0][:8]])
        for i, (x, y, w, h) in enumerate(crops):
            want = np.full(region, probe.dst_fill, np.uint8)
            want[probe.dst_guard:probe.dst_guard + 3 * w * h] = np.frombuffer(frame[y:y + h, x:x + w].tobytes(), np.uint8)
            bad = np.nonzero(out[i] != want)[0]
            assert len(bad) == 0, ((H, W, stride), crops[i], "bytes (offset from the destination's start)", bad[:8] - probe.dst_guard,
                                   out[i][bad[:8]], want[bad[:8]], "crop bytes", 3 * w * h)


def test_frame_probes_refuse_bad_cases(probe):
    """A crop outside the frame, a frame size that is not the allocation's and a geometry that is not the crop's get an error code, not a
    launch."""
    H, W = 20, 50
    buf, _ = tc.make_frame(H, W, 150, 5)
    good = tc.frame_state(H, W, (3, 2, 30, 10))
    bad = [tc.frame_state(H, W, (30, 2, 30, 10)), tc.frame_state(H, W, (3, 15, 30, 10)), tc.frame_state(H + 1, W, (3, 2, 30, 10)),
           tc.frame_state(H, W, (-1, 2, 30, 10)), tc.frame_state(H, W, (3, 2, 0, 10))]
    other = good.copy()
    other[4 * tc.HDR_INTS:] = tc.squarify_bytes(10, 31)[0]      # the tables of another crop size
    stale = good.copy()
    stale[8:12] = np.array([29], np.int32).view(np.uint8)        # w no longer the geometry's
    states = np.ascontiguousarray(np.stack([good] + bad + [other, stale]))
    n = len(states)
    out, err = np.full((n, 1024 + 128), 0x22, np.uint8), np.zeros(n, np.int32)
    rc = probe.tp_copy(_p(buf, u8p), H, W, 150, n, _p(states, u8p), 1024, _p(out, u8p), _p(err, i32p))
    assert rc == n - 1 and err[0] == 0 and np.all(err[1:] != 0) and np.all(out == 0x22), (rc, err)
    scales = np.asarray(tc.BASELINE_SCALES)
    packed = np.zeros(n, np.int32)
    rc = probe.tp_pyramid(_p(buf, u8p), H, W, 150, n, _p(states, u8p), _p(packed, i32p), _p(scales, f64p), 3, EL_F32, None, _p(err, i32p))
    assert rc == n - 1 and err[0] == 0 and np.all(err[1:] != 0), (rc, err)


# ---- tracked pyramid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_index", range(4))
def test_tracked_pyramid_equals_gen_input_batch(probe, frame_index):
    """pyramid_track_kernel over crops at odd origins of 640 x 480, 1920 x 1080, 1080 x 1920 and 4096 x 2160 frames, from the whole frame
    in device memory (packed = 0, the origin from the state) and from the crop's own packed rows (packed = 1): bit-equal to
    oracle.gen_input_batch of frame[y:y+h, x:x+w] in fp32 with [1.0, 0.8, 0.6] and a 6-scale set, and to its round-to-nearest-even
    conversion in bf16 and fp16.  The geometry in the state is hostplan.h's squarify, not crop.h's."""
    f = tc.pyramid_cases()[frame_index]
    H, W = f["H"], f["W"]
    buf, frame = tc.make_frame(H, W, 3 * W, f["seed"])
    crops = f["crops"]
    both = [c for c in crops for _ in (0, 1)]
    packed = np.asarray([0, 1] * len(crops), np.int32)
    states = _states_for(H, W, both)
    # the first frame behind an initial rect that runs past the frame's far edges: the crop is clipped, the reported extent (uw, uh) is not
    # -- no kernel may take the crop's size from it
    edge = [(W - 301, H - 201, 301, 201), (W - 57, 3, 57, H - 3)]
    states = np.concatenate([states, np.stack([tc.frame_state(H, W, c, past=(57, 31)) for c in edge for _ in (0, 1)])])
    crops, both, packed = crops + edge, both + [c for c in edge for _ in (0, 1)], np.concatenate([packed, np.asarray([0, 1, 0, 1], np.int32)])
    n = len(both)
    for scales, els in ((tc.BASELINE_SCALES, (EL_F32, EL_BF16, EL_F16)), (tc.SIX_SCALES, (EL_F32,))):
        S = len(scales)
        sc = np.asarray(scales, np.float64)
        want32 = [tc.pyramid_reference(frame[y:y + h, x:x + w], scales) for x, y, w, h in crops]
        for el in els:
            out = np.zeros((n, S, 368, 368, 4), np.float32 if el == EL_F32 else np.uint16)
            err = np.zeros(n, np.int32)
            rc = probe.tp_pyramid(_p(buf, u8p), H, W, 3 * W, n, _p(states, u8p), _p(packed, i32p), _p(sc, f64p), S, el, out.ctypes.data, _p(err, i32p))
            assert rc == 0, (rc, [(both[i], int(err[i])) for i in np.nonzero(err)[0][:8]])
            for i in range(n):
                want = want32[i // 2]
                if el == EL_F32:
                    same = np.array_equal(out[i].view(np.uint32), want.view(np.uint32))
                else:
                    same = np.array_equal(out[i], tc.to_16(want, el == EL_F16))
                if not same:
                    w16 = want if el == EL_F32 else tc.to_16(want, el == EL_F16)
                    where = np.argwhere(out[i] != w16)
                    raise AssertionError(((W, H), "crop", both[i], "packed", int(packed[i]), "el", el, "scales", S, "differing", len(where),
                                          "first (s, y, x, c)", where[:4].tolist()))
