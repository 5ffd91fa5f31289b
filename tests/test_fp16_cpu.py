"""CPU: the fp16 precision (VNECT_FP16) -- its declarations, the host's fp16 conversions (hostplan.h to_f16 / from_f16, what
the weights of an fp16 handle are uploaded as and what vnect_read_activation widens with) against numpy's float16, and the 16-bit
weight layouts, which an fp16 handle shares with a bf16 one element for element."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
SO = os.path.join(ROOT, "vnect_amd", "lib", "libvnect_hostplan.so")
f32p, u16p = C.POINTER(C.c_float), C.POINTER(C.c_uint16)


@pytest.fixture(scope="module")
def hp():
    subprocess.check_call(["make", "-C", CSRC, "hostplan"], stdout=subprocess.DEVNULL)
    L = C.CDLL(SO)
    L.hp_to_f16.argtypes, L.hp_to_f16.restype = [C.c_float], C.c_uint16
    L.hp_from_f16.argtypes, L.hp_from_f16.restype = [C.c_uint16], C.c_float
    L.hp_to_16.argtypes = [f32p, C.c_int64, C.c_int, u16p]
    L.hp_from_f16_array.argtypes = [u16p, C.c_int64, f32p]
    L.hp_first_f16_overflow.argtypes, L.hp_first_f16_overflow.restype = [f32p, C.c_int64], C.c_longlong
    L.hp_pack_conv.argtypes = [f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32p]
    L.hp_pack_tail.argtypes = [f32p, C.c_int, C.c_int, C.c_int, f32p]
    return L


def _to16(hp, x, f16=True):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.shape, np.uint16)
    hp.hp_to_16(x.ctypes.data_as(f32p), x.size, int(f16), out.ctypes.data_as(u16p))
    return out


def _from16(hp, b):
    b = np.ascontiguousarray(b, np.uint16)
    out = np.empty(b.shape, np.float32)
    hp.hp_from_f16_array(b.ctypes.data_as(u16p), b.size, out.ctypes.data_as(f32p))
    return out


def test_declarations_agree():
    from vnect_amd import _native
    from vnect_amd.estimator import PRECISIONS
    h = open(os.path.join(ROOT, "include", "vnect_abi.h")).read()
    # (an added value of an existing field: no entry point, struct or symbol changes, so the ABI version stays the header's)
    assert int(re.search(r"#define VNECT_ABI_VERSION (\d+)", h).group(1)) == _native.ABI_VERSION
    assert int(re.search(r"VNECT_FP16 = (\d+)", h).group(1)) == 3 == _native.FP16
    assert PRECISIONS == {"fp32": 0, "bf16": 1, "fp32_split": 2, "fp16": 3}


def test_every_fp16_value_round_trips(hp):
    bits = np.arange(1 << 16, dtype=np.uint16)
    want = bits.view(np.float16).astype(np.float32)
    got = _from16(hp, bits)
    finite = np.isfinite(want)
    assert np.array_equal(got[finite], want[finite]) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.signbit(got), np.signbit(want))
    # and back: every finite fp16 value (subnormals, +-0 included) converts to itself
    assert np.array_equal(_to16(hp, want[finite]), bits[finite])
    assert hp.hp_from_f16(0x3C00) == 1.0 and hp.hp_to_f16(1.0) == 0x3C00


def test_midpoints_and_their_neighbours(hp):
    """Every midpoint between neighbouring finite fp16 values (a tie: round to even) and the float32 values on either side of it."""
    pos = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = ((pos[:-1] + pos[1:]) / 2).astype(np.float32)     # exact in float32 (12 significant bits at most)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    x = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    x = np.concatenate([x, -x])
    assert np.array_equal(_to16(hp, x), x.astype(np.float16).view(np.uint16))


def test_subnormal_range_and_edges(hp):
    sub = np.linspace(0, 2.0 ** -14, 200001, dtype=np.float64).astype(np.float32)
    x = np.concatenate([sub, -sub, np.float32([2.0 ** -25, 2.0 ** -25 * 3, 2.0 ** -26, 1e-8, 1.3e-8, 1e-45])])
    assert np.array_equal(_to16(hp, x), x.astype(np.float16).view(np.uint16))
    assert hp.hp_to_f16(1.3e-8) == 0                      # the smallest nonzero synthetic weight: zero in fp16
    assert hp.hp_from_f16(hp.hp_to_f16(np.float32(65519.99))) == 65504.0
    assert hp.hp_to_f16(65520.0) == 0x7C00 and hp.hp_to_f16(-65520.0) == 0xFC00
    assert hp.hp_to_f16(float("inf")) == 0x7C00 and hp.hp_to_f16(0.0) == 0 and hp.hp_to_f16(-0.0) == 0x8000
    assert np.isnan(hp.hp_from_f16(hp.hp_to_f16(float("nan"))))


def test_ten_million_random_floats(hp):
    rng = np.random.RandomState(16)
    x = np.concatenate([rng.standard_normal(4_000_000).astype(np.float32) * np.float32(2.0) ** rng.randint(-30, 20, 4_000_000).astype(np.float32),
                        rng.randint(0, 1 << 32, 6_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    got, want = _to16(hp, x), x.astype(np.float16).view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all((got[nan] & 0x7C00) == 0x7C00) and np.all(got[nan] & 0x3FF)


def test_overflow_scan(hp):
    w = np.zeros(1000, np.float32)
    assert hp.hp_first_f16_overflow(w.ctypes.data_as(f32p), w.size) == -1
    w[417], w[900] = 65519.99, -1e5
    assert hp.hp_first_f16_overflow(w.ctypes.data_as(f32p), w.size) == 900
    w[3] = np.inf  # (not a finite weight: the check is about values fp16 cannot hold)
    assert hp.hp_first_f16_overflow(w.ctypes.data_as(f32p), w.size) == 900


def test_16_bit_layouts_are_shared(hp):
    """hp_pack_conv / hp_pack_tail with the 16-bit layout, then the upload conversion: the fp16 and the bf16 handle hold the same element
    at every position (each rounded in its own format), and the fp16 one is numpy's float16 of the packed value."""
    from tests.gpu_common import _round_bf16
    rng = np.random.RandomState(3)
    for k, cin, cout, cp, conv1 in ((3, 64, 64, 64, 0), (1, 256, 128, 256, 0), (7, 3, 64, 4, 1)):
        W = (rng.standard_normal((k, k, cin, cout)) * 0.1).astype(np.float32)
        K = 4 * 64 if conv1 else k * k * cp
        wp = np.zeros((cout, K), np.float32)
        hp.hp_pack_conv(W.ctypes.data_as(f32p), k, cin, cout, cp, conv1, 1, cout, K, 0, wp.ctypes.data_as(f32p))
        h16, b16 = _to16(hp, wp, True), _to16(hp, wp, False)
        assert np.array_equal(h16, wp.astype(np.float16).view(np.uint16))
        assert np.array_equal((b16.astype(np.uint32) << 16).view(np.float32), _round_bf16(wp))
        assert np.array_equal(h16 != 0, b16 != 0) and np.count_nonzero(h16) == np.count_nonzero(W.astype(np.float16))
    for mid, cout in ((64, 256), (128, 512)):
        Wc = (rng.standard_normal((mid, cout)) * 0.1).astype(np.float32)
        w2 = np.zeros(((cout + 31) // 32 * 32, mid), np.float32)
        hp.hp_pack_tail(Wc.ctypes.data_as(f32p), mid, cout, 1, w2.ctypes.data_as(f32p))
        assert np.array_equal(_from16(hp, _to16(hp, w2)), w2.astype(np.float16).astype(np.float32))
        assert sorted(w2.ravel().tolist()) == sorted(Wc.ravel().tolist() + [0.0] * (w2.size - Wc.size))

