"""CPU: the live-rows plan rule and row enumeration (vnect_amd/csrc/hostplan.h: live_rows_stride, live_enumeration, live_wg_tile), through
the C shim the other host-planning tests use (hostplan_capi.cpp, built with plain g++).

A tail launch whose output tensor is read only by 1x1 convs of one stride s > 1 computes the pixels (s y, s x) alone.  The launch table
below is written down here from the network (the bottleneck blocks of the reference's vnect_model.py, as rt_plan.cpp fuses them on an
arena plan), independently of the runtime: one row per launch, in the nine-integer form rt_plan.cpp hands to the rule.

Which launches are tails depends on the plan, not on the rule: the 64-wide tails of the 92 x 92 stage exist up to three scales, the wide
tails of the 46 x 46 stage from two scales on in fp32 (every scale count in the 16-bit formats and with VNECT_FORCE_WIDE_TAIL) -- so the
table takes `wide` as a parameter, and at one fp32 scale res3d_branch2c is a stand-alone launch and only res2c's tail qualifies."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
SO = os.environ.get("VNECT_HOSTPLAN_SO") or os.path.join(ROOT, "vnect_amd", "lib", "libvnect_hostplan.so")

RES2C, RES3D = "res2c_branch2b>res2c_branch2c", "res3d_branch2b>res3d_branch2c"


@pytest.fixture(scope="module")
def hp():
    if "VNECT_HOSTPLAN_SO" not in os.environ:
        subprocess.check_call(["make", "-C", CSRC, "hostplan"], stdout=subprocess.DEVNULL)
    L = C.CDLL(SO)
    L.hp_live_rows_stride.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int]
    L.hp_live_enumeration.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    L.hp_live_enumeration.restype = None
    return L


class _Table:
    """launches as (name, in, resid, out, out2, out3, ntaps, stride, tap00, tail) over tensor names"""

    def __init__(self):
        self.t, self.rows = {}, []

    def ten(self, name):
        return -1 if name is None else self.t.setdefault(name, len(self.t))

    def add(self, name, src, out, k=1, stride=1, resid=None, out2=None, out3=None, tail=False, conv=True, taps=None):
        ntaps = 0 if not conv else (taps if taps is not None else k * k)
        self.rows.append((name, self.ten(src), self.ten(resid), self.ten(out), self.ten(out2), self.ten(out3), ntaps, stride,
                          int(conv and k == 1 and taps is None), int(tail)))

    def array(self):
        return np.ascontiguousarray([r[1:] for r in self.rows], np.int32)


def launch_table(paper, tails=True, wide=True, chain=False):
    """The arena plan's launches.  tails: the fused 3x3 > 1x1 launches exist at all (False: a keep_activations handle, every layer a launch
    of its own); wide: those of the 46 x 46 stage and the head too; chain: the 16-bit formats' chain GEMMs (the next block's branch2a as
    the launch's third output)."""
    T = _Table()

    def b_then_c(p, a, s, fused, nxt=None):
        if fused:
            T.add("%s_branch2b>%s_branch2c" % (p, p), a, p, k=3, resid=s, tail=True, out3=nxt)
        else:
            T.add(p + "_branch2b", a, p + "_branch2b", k=3)
            T.add(p + "_branch2c", p + "_branch2b", p, resid=s)
        return p

    def proj(p, x, stride, fused, nxt=None, sfx=""):
        T.add("%s_branch2a%s+branch1%s" % (p, sfx, sfx), x, p + "_branch2a", stride=stride, out2=p + "_branch1")
        return b_then_c(p, p + "_branch2a", p + "_branch1", fused, nxt)

    def ident(p, x, fused, have_a=False, nxt=None):
        if not have_a:
            T.add(p + "_branch2a", x, p + "_branch2a")
        return b_then_c(p, p + "_branch2a", x, fused, nxt)

    T.add("conv1", "input", "conv1", k=7, stride=2, taps=7)
    T.add("pool1", "conv1", "pool1", conv=False)
    r = proj("res2a", "pool1", 1, tails, nxt="res2b_branch2a" if chain and tails else None)
    if paper:
        r = ident("res2b", r, tails, have_a=chain and tails, nxt="res2c_branch2a" if chain and tails else None)
        r = ident("res2c", r, tails, have_a=chain and tails)
    else:
        x = r
        if not (chain and tails):
            T.add("res2b_branch2a", x, "res2b_branch2a")
        if tails:
            T.add("res2b_branch2b>res2b_branch2c", "res2b_branch2a", "res2b", k=3, resid=x, tail=True)
            T.add(RES2C, "res2b_branch2a", "res2c", k=3, resid="res2b", tail=True)
        else:
            T.add("res2b_branch2b+res2c_branch2b", "res2b_branch2a", "res2b_branch2b", k=3, out2="res2c_branch2b")
            T.add("res2b_branch2c", "res2b_branch2b", "res2b", resid=x)
            T.add("res2c_branch2c", "res2c_branch2b", "res2c", resid="res2b")
        r = "res2c"
    w = tails and wide
    r = proj("res3a", r, 2, w, nxt="res3b_branch2a" if chain and w else None)
    for p, nxt in (("res3b", "res3c"), ("res3c", "res3d"), ("res3d", None)):
        r = ident(p, r, w, have_a=chain and w, nxt=nxt + "_branch2a" if chain and w and nxt else None)
    r = proj("res4a", r, 2, False)
    for p in ("res4b", "res4c", "res4d", "res4e", "res4f"):
        r = ident(p, r, False)
    T.add("res5a_branch2a_new+branch1_new", r, "res5a_branch2a_new", out2="res5a_branch1_new")
    T.add("res5a_branch2b_new", "res5a_branch2a_new", "res5a_branch2b_new", k=3)
    T.add("res5a_branch2c_new", "res5a_branch2b_new", "res5a", resid="res5a_branch1_new")
    T.add("res5b_branch2a_new", "res5a", "res5b_branch2a_new")
    T.add("res5b_branch2b_new", "res5b_branch2a_new", "res5b_branch2b_new", k=3)
    T.add("res5b_branch2c_new", "res5b_branch2b_new", "res5b_branch2c_new")
    T.add("res5c_deconv", "res5b_branch2c_new", "feat", taps=16)
    if w:
        T.add("res5c_branch2b>res5c_branch2c", "feat", "maps", k=3, tail=True)
    else:
        T.add("res5c_branch2b", "feat", "res5c_branch2b", k=3)
        T.add("res5c_branch2c", "res5c_branch2b", "maps")
    return T


def _qualifying(hp, T):
    a = T.array()
    p = a.ctypes.data_as(C.POINTER(C.c_int32))
    return {T.rows[i][0]: hp.hp_live_rows_stride(p, len(T.rows), i, T.ten("maps")) for i in range(len(T.rows))}


@pytest.mark.parametrize("paper", [False, True], ids=["default", "paper"])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_exactly_the_two_tails_in_front_of_a_stride_2_block_qualify(hp, S, paper):
    # (the rule sees launches, not shapes: S enters through which tails the plan has)
    for wide in ({True} if S >= 2 else {False, True}):
        q = _qualifying(hp, launch_table(paper, wide=wide))
        want = {RES2C: 2, RES3D: 2} if wide else {RES2C: 2}
        assert {n: s for n, s in q.items() if s} == want, (S, paper, wide)
    # the 16-bit plans: the chained launches ahead feed every row to a third GEMM; res2c's and res3d's own launches have no chain
    q = _qualifying(hp, launch_table(paper, chain=True))
    assert {n: s for n, s in q.items() if s} == {RES2C: 2, RES3D: 2}


@pytest.mark.parametrize("paper", [False, True], ids=["default", "paper"])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_none_qualifies_with_keep_activations(hp, S, paper):
    """every layer a launch of its own: no tail launch, so nothing to qualify -- the tensors of such a handle are read back whole"""
    q = _qualifying(hp, launch_table(paper, tails=False))
    assert not any(q.values()) and len(q) >= 48   # (one launch per layer: 48 or 49 of them)


def test_the_rule_refuses_every_other_reader(hp):
    def q_of(edit):
        T = launch_table(False)
        edit(T)
        return _qualifying(hp, T)

    def set_row(T, name, **kw):
        i = [r[0] for r in T.rows].index(name)
        cols = ["name", "in", "resid", "out", "out2", "out3", "ntaps", "stride", "tap00", "tail"]
        r = list(T.rows[i])
        for k, v in kw.items():
            r[cols.index(k)] = v
        T.rows[i] = tuple(r)

    assert q_of(lambda T: None)[RES2C] == 2
    assert q_of(lambda T: set_row(T, "res3a_branch2a+branch1", stride=1))[RES2C] == 0             # a stride-1 reader
    assert q_of(lambda T: set_row(T, "res3a_branch2a+branch1", ntaps=9, tap00=0))[RES2C] == 0      # a 3x3 reader
    assert q_of(lambda T: T.add("x", "res2c", "x", stride=4))[RES2C] == 0                          # two strides
    assert q_of(lambda T: T.add("x", "res2c", "x", stride=2))[RES2C] == 2                          # one more reader of the same stride
    assert q_of(lambda T: T.add("x", "pool1", "x", resid="res2c"))[RES2C] == 0                     # a shortcut of another launch
    assert q_of(lambda T: T.add("x", "res2c", "x", conv=False))[RES2C] == 0                        # a pooling reader
    assert q_of(lambda T: set_row(T, RES2C, out3=T.ten("y")))[RES2C] == 0                          # a chain GEMM behind it
    assert q_of(lambda T: set_row(T, "res3a_branch2a+branch1", **{"in": T.ten("pool1")}))[RES2C] == 0  # no reader at all
    q = q_of(lambda T: None)
    assert q["res5c_branch2b>res5c_branch2c"] == 0 and q["res2b_branch2b>res2b_branch2c"] == 0      # the final maps; res2c's shortcut


def _enum(hp, S, Ho, Wo, s):
    pix = np.empty(S * Ho * Wo, np.int32)
    hp.hp_live_enumeration(S, Ho, Wo, s, pix.ctypes.data_as(C.POINTER(C.c_int32)))
    return pix


@pytest.mark.parametrize("S,Ho,Wo,s", [(1, 92, 92, 2), (2, 92, 92, 2), (3, 92, 92, 2), (6, 92, 92, 2), (3, 46, 46, 2), (2, 7, 5, 2), (1, 10, 9, 3)])
def test_the_live_first_enumeration_is_a_permutation_of_the_rows(hp, S, Ho, Wo, s):
    pix = _enum(hp, S, Ho, Wo, s)
    M = S * Ho * Wo
    assert np.array_equal(np.sort(pix), np.arange(M))
    Hl, Wl = -(-Ho // s), -(-Wo // s)
    L = hp.hp_live_rows(S, Ho, Wo, s)
    assert L == S * Hl * Wl
    # live row j = (image, oy', ox') in raster order of the live grid, at pixel (s oy', s ox'): what a 1x1 stride-s conv reads
    j = np.arange(L)
    im, oy, ox = j // (Hl * Wl), j // Wl % Hl, j % Wl
    assert np.array_equal(pix[:L], (im * Ho + s * oy) * Wo + s * ox)
    rest = pix[L:]
    assert np.all(np.diff(rest) > 0) and np.all(((rest % Wo) % s != 0) | ((rest // Wo % Ho) % s != 0))


@pytest.mark.parametrize("S", [1, 2, 3, 6])
def test_live_tiles_lead_every_xcd_range(hp, S):
    """conv.hip deals items to the XCDs in contiguous eighths, workgroup id on XCD id & 7: the ceil(live / 64) live tiles are the first
    workgroups of every XCD (so the lowest ids of the grid: dispatched first, at most one per CU), 12 or 13 per XCD at three scales"""
    M, L = S * 92 * 92, hp.hp_live_rows(S, 92, 92, 2)
    grid, tiles = -(-M // 64), -(-L // 64)
    got = np.array([hp.hp_live_wg_tile(tiles, grid, i) for i in range(grid)])
    assert np.array_equal(np.sort(got[got >= 0]), np.arange(tiles))   # every live tile once
    nxt = 0
    for x in range(8):
        mine = got[x::8]
        cnt = int((mine >= 0).sum())
        assert cnt in (tiles // 8, tiles // 8 + 1) and np.all(mine[cnt:] < 0)   # in front, nothing behind
        assert np.array_equal(mine[:cnt], np.arange(nxt, nxt + cnt))            # a contiguous range, in order
        nxt += cnt
    assert np.all(np.nonzero(got >= 0)[0] < 8 * -(-tiles // 8)) and tiles <= 256
    if S == 3:
        assert (L, grid, tiles) == (6348, 397, 100) and {int((got[x::8] >= 0).sum()) for x in range(8)} == {12, 13}
    if S == 1:
        assert (L, L % 64) == (2116, 4)   # 33 tiles and a partial one
    assert hp.hp_live_wg_tile(tiles, grid, grid) == -1 and hp.hp_live_wg_tile(tiles, grid, -1) == -1
