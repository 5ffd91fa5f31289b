"""GPU: the kernels of a re-detection -- the product's hog.o behind a probe (`make redetectprobe`; csrc/redetect_probe.hip).  Every buffer
lies between guard zones, which are compared after each call.  Gate 0: the gated launches and the pick kernel leave votes, blocks, hits,
the counter and the stream's state untouched, byte for byte.  Gate 1: the gated launches equal the ungated kernels with the grid capped at
1 and at 3 workgroups (the stride loop wraps), and the pick kernel equals the CPU statement (tests/redetect_ref.py) in the next state's
bytes, status, chosen rect and hit count -- on the CPU file's hand-made lists and on its random ones."""
import ctypes as C

import numpy as np
import pytest

from tests import hog_ref as R
from tests import redetect_ref as D
from tests import test_redetect_cpu as T

pytestmark = pytest.mark.gpu

DET = R.seeded_detector(1, rho=0.05, scale=0.04)
CANARY32 = int(np.frombuffer(bytes([0xC7] * 4), np.int32)[0])


@pytest.fixture(scope="module")
def probe():
    import os
    L = C.CDLL(os.path.join(R.LIBDIR, "libvnect_redetectprobe.so"))
    L.rp_layout.restype, L.rp_layout.argtypes = None, [R.i32p]
    L.rp_gated.restype = C.c_int
    L.rp_gated.argtypes = R._FRAME_C + [C.c_int] + R._SPEC_C + [R.f32p, C.c_int, C.c_int, C.c_int, C.c_int, R.f32p, R.u8p, R.f32p, R.i32p, R.f32p, R.i64p]
    L.rp_pick.restype = C.c_int
    L.rp_pick.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, R.i32p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, R.i32p,
                          C.c_uint, R.i32p, R.u8p, R.u8p, R.i32p, R.i64p]
    lay = np.zeros(6, np.int32)
    L.rp_layout(lay.ctypes.data_as(R.i32p))
    assert lay[0] == 0xC7 and lay[3] == 1024 and lay[4] == D.MAX_HITS
    L.state_size = int(lay[2])
    return L


def _gated(probe, pic, s, gate, cap, count0=0):
    lay = R.packed(*pic.shape[:2])
    buf = R.lay_from_picture(pic, lay, 0)
    _, _, _, _, tot = R.sizes_of(lay, 0, s)
    out = R._outputs(tot, s)
    info = np.zeros(4, np.int64)
    det = np.ascontiguousarray(DET, R.F)
    rc = probe.rp_gated(*R.frame_args(buf, lay), 0, *R.spec_args(s), det.ctypes.data_as(R.f32p), det.size, gate, cap, count0,
                        out["votes"].ctypes.data_as(R.f32p), out["bins"].ctypes.data_as(R.u8p), out["blocks"].ctypes.data_as(R.f32p),
                        out["hits"].ctypes.data_as(R.i32p), out["hit_s"].ctypes.data_as(R.f32p), info.ctypes.data_as(R.i64p))
    assert rc == 0, rc
    n = int(info[3])
    out["hits"], out["hit_s"] = out["hits"][:3 * n].reshape(n, 3), out["hit_s"][:n]
    for k in ("votes", "bins", "blocks"):
        out[k] = out[k][:-1]
    return out, dict(count=int(info[0]), guard=int(info[1]), changed=int(info[2]))


@pytest.fixture(scope="module")
def ungated():
    """the ungated kernels' stages (hog_probe.hip), once per shape"""
    out = {}
    for shape in ((128, 64), (264, 200)):
        pic = R.textured(*shape, seed=shape[0])
        s = R.spec(hit_threshold=-0.05, max_hits=D.MAX_HITS)
        lay = R.packed(*shape)
        rc, ref = R.probe(R.lay_from_picture(pic, lay, 0), lay, 0, DET, s)
        assert rc == 0 and ref["guard_damage"] == 0 and ref["launches"] == 3
        out[shape] = (pic, s, ref)
    assert len(out[(128, 64)][2]["scores"]) == 1 and out[(264, 200)][2]["count"] > 0
    return out


@pytest.mark.parametrize("shape", [(128, 64), (264, 200)])
def test_gate_0_the_launches_touch_nothing(probe, ungated, shape):
    pic, s, _ = ungated[shape]
    for cap in (0, 3, 1024):
        _, info = _gated(probe, pic, s, 0, cap, count0=5)
        assert info == dict(count=5, guard=0, changed=0), (cap, info)


@pytest.mark.parametrize("shape", [(128, 64), (264, 200)])
@pytest.mark.parametrize("cap", [1, 3, 1024, 0])
def test_gate_1_equals_the_ungated_kernels(probe, ungated, shape, cap):
    """one level and one window; several levels and tile seams -- with the grid forced down to 1 and 3 workgroups, so that the stride loop
    wraps many times and every round reuses the workgroup's LDS"""
    pic, s, ref = ungated[shape]
    got, info = _gated(probe, pic, s, 1, cap)
    assert info["guard"] == 0 and info["count"] == ref["count"]
    for k in ("votes", "blocks"):
        assert np.array_equal(R.bits(got[k]), R.bits(ref[k])), (k, cap)
    assert np.array_equal(got["bins"], ref["bins"])
    assert np.array_equal(got["hits"], ref["hits"]) and np.array_equal(R.bits(got["hit_s"]), R.bits(ref["hit_s"]))


def _pick(probe, hits, count, Hp, Wp, s=T.S, threshold=2, gate=1, ts=None, rect0=None, xseq=7, want_next=None):
    n = min(count, s["max_hits"])
    h3 = np.ascontiguousarray(np.asarray(hits, np.int32).reshape(-1, 3)[:n])
    tsH, tsW = ts if ts is not None else (Hp, Wp)
    rect0 = np.array(rect0 if rect0 is not None else [3, 5, min(tsW, 300) - 3, min(tsH, 400) - 5], np.int32)
    size = probe.state_size
    state, want = np.zeros(size, np.uint8), np.zeros(size, np.uint8)
    out6, info = np.zeros(6, np.int32), np.zeros(4, np.int64)
    nx = None if want_next is None else np.array(want_next, np.int32)
    rc = probe.rp_pick(0, Hp, Wp, float(s["scale0"]), int(s["nlevels"]), h3.ctypes.data_as(R.i32p), n, count, int(s["max_hits"]), threshold, gate, tsH, tsW,
                       rect0.ctypes.data_as(R.i32p), xseq, None if nx is None else nx.ctypes.data_as(R.i32p), state.ctypes.data_as(R.u8p),
                       want.ctypes.data_as(R.u8p), out6.ctypes.data_as(R.i32p), info.ctypes.data_as(R.i64p))
    assert rc == 0, rc
    return state, want, [int(v) for v in out6], dict(guard=int(info[0]), cls=int(info[1]), state=int(info[2]), verdict=int(info[3]))


def _pick_equals_cpu(probe, hits, count, Hp, Wp, s=T.S, threshold=2):
    rc, (st, rect, nh, nxt) = D.walk(hits, count, Hp, Wp, s, 0, threshold)
    assert rc == 0
    assert (st, rect, nh, nxt) == D.pick(hits, count, Hp, Wp, s, threshold)
    state, want, out6, info = _pick(probe, hits, count, Hp, Wp, s, threshold, want_next=nxt)
    assert info["guard"] == 0 and info["cls"] == 0, info
    assert out6[0] == st and out6[5] == nh, (out6, st, nh)
    assert out6[1:5] == (rect if st == D.FOUND else [CANARY32] * 4)           # the rect is written only when somebody was found
    assert np.array_equal(state, want), "the next TrackState differs from the CPU statement's"
    return st, nxt


def test_pick_gate_0_writes_the_status_word_and_nothing_else(probe):
    state, _, out6, info = _pick(probe, T._cluster(200, 400, 4), 4, T.H, T.W, gate=0)
    assert info == dict(guard=0, cls=0, state=0, verdict=4)
    assert out6 == [D.NOT_RUN] + [CANARY32] * 5


def test_pick_on_the_hand_made_lists(probe):
    H, W = T.H, T.W
    found = 0
    lists = [[], [(0, 40, 80)], T._cluster(200, 400, 2), T._cluster(200, 400, 3), [(0, 200, 400), (0, 200, 416), (0, 200, 432)],
             T._cluster(400, 900, 4) + T._cluster(100, 100, 4), T._cluster(100, 100, 4) + T._cluster(400, 900, 4),
             [(0, 200, 400), (0, 200, 408), (0, 208, 400), (0, 208, 410)], T._cluster(0, 0, 4), T._cluster(H - 144, W - 80, 4)]
    for hits in lists:
        for order in (hits, hits[::-1]):
            found += _pick_equals_cpu(probe, order, len(order), H, W)[0] == D.FOUND
    assert found >= 14
    assert _pick_equals_cpu(probe, [(0, 40, 80)], 1, H, W, threshold=0)[0] == D.FOUND
    chain = [(0, 96, 16 * k) for k in range(200)]
    rng = np.random.RandomState(5)
    for order in (chain, chain[::-1], [chain[i] for i in rng.permutation(200)]):
        assert _pick_equals_cpu(probe, order, 200, 360, 3400)[0] == D.FOUND


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097])
def test_pick_on_random_lists(probe, n):
    hits = T._many(n, seed=n)
    rng = np.random.RandomState(n)
    shuffled = [hits[i] for i in rng.permutation(len(hits))]
    a = _pick_equals_cpu(probe, shuffled, n, 1080, 1920)
    if n == 4097:
        assert a == (D.OVERFLOW, [0, 0, 1920, 1080])
    elif n <= 1025:
        assert _pick_equals_cpu(probe, hits, n, 1080, 1920, threshold=1) is not None


def test_a_next_crop_that_squarify_refuses_takes_the_refusal_path(probe):
    """nobody found on a stream whose frame is 100 000 wide: the whole frame is the next box, squarify refuses it (SQ_RANGE), and the
    state says so the way a box stage says it -- zero geometry, the status, the fail word naming the NEXT tracked frame"""
    state, want, out6, info = _pick(probe, [], 0, T.H, T.W, ts=(128, 100000), rect0=[0, 0, 300, 128], xseq=7, want_next=[0, 0, 100000, 128])
    assert info["guard"] == 0 and out6[0] == D.NOBODY and np.array_equal(state, want)
    head = state[:40].view(np.int32)
    assert list(head[:8]) == [0, 0, 100000, 128, 100000, 128, 128, 100000] and head[8] == 1 and head[9] == 8
