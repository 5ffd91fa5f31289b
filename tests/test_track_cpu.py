"""CPU: the device-side tracking loop's arithmetic (vnect_amd/csrc/crop.h) against the host's.

crop.h is ONE source for the host and the device (track.hip builds the next frame's crop geometry and box with it); here its host build,
behind the C shim hostplan_capi.cpp, is held to what the host path computes for an untracked frame: hostplan.h's squarify (the
FrameParams bytes, the refusals and their messages) and runner.bbox_update / runner.track's fallback.  The GPU half
(tests/test_gpu_track.py) holds the device's results to runner.track frame by frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import track_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
SO = os.environ.get("VNECT_HOSTPLAN_SO") or os.path.join(ROOT, "vnect_amd", "lib", "libvnect_hostplan.so")
u8p, f64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def hp():
    if "VNECT_HOSTPLAN_SO" not in os.environ:
        subprocess.check_call(["make", "-C", CSRC, "hostplan"], stdout=subprocess.DEVNULL)
    L = C.CDLL(SO)
    L.hp_squarify_bytes.argtypes = [C.c_int, C.c_int, u8p, C.c_char_p, C.c_int]
    L.hp_crop_squarify_bytes.argtypes = [C.c_int, C.c_int, u8p, C.c_char_p, C.c_int]
    L.hp_box_update.argtypes = [f64p, C.c_int, C.c_int, C.c_int, C.c_int, i32p]
    return L


def _both(hp, H, W):
    n = hp.hp_frame_params_size()
    a, b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    ea, eb = C.create_string_buffer(128), C.create_string_buffer(128)
    ra = hp.hp_squarify_bytes(H, W, a.ctypes.data_as(u8p), ea, 128)
    rb = hp.hp_crop_squarify_bytes(H, W, b.ctypes.data_as(u8p), eb, 128)
    return (ra, a, ea.value.decode()), (rb, b, eb.value.decode())


def _check(hp, H, W):
    (ra, a, ea), (rb, b, eb) = _both(hp, H, W)
    if ra == 0:
        assert rb == 0 and np.array_equal(a, b), (H, W, np.nonzero(a != b)[0][:8])
        return False
    assert rb != 0 and eb == ea, (H, W, ea, eb)   # a refusal with the host's message
    return True


def test_shared_geometry_equals_host_squarify_up_to_1024(hp):
    """Every crop size up to 1024 x 1024 on a dense subsample: all sizes up to 96 on both sides, every size paired with the
    sizes around 368 and with a stride-7 grid, the bytes of the whole FrameParams equal."""
    pairs = track_cases.dense_sizes()   # (shared with the device twin, tests/test_gpu_track_kernels.py)
    refused = sum(_check(hp, h, w) for h, w in pairs)
    assert refused > 0   # (h, w) = (1, 737): 368 / 737 scales the short side to 0 pixels


def test_shared_geometry_equals_host_squarify_random_sizes(hp):
    """Random sizes up to 8192 (and past it: "frame size out of range"), skinny ones included so that refusals occur."""
    sizes = track_cases.random_sizes()
    refused = sum(_check(hp, h, w) for h, w in sizes)
    assert refused > 100


def test_refusal_messages_are_the_host_paths():
    from vnect_amd import runner   # noqa: F401  (the package imports without a GPU)
    src = open(os.path.join(CSRC, "hostplan.h")).read()
    for msg in ("frame size out of range", "squarify: scaled size exceeds 368", "squarify: scaled long side != 368"):
        assert '"%s"' % msg in src and '"%s"' % msg in open(os.path.join(CSRC, "crop.h")).read(), msg


def _box_cases(n, seed=11):
    """n joint sets (21, 2) [row, col] with the frame sizes they are ruled in: spread, clustered, negative, outside the frame, and sets
    whose span is zero on one or both axes."""
    rng = np.random.default_rng(seed)
    H = rng.integers(1, 2000, n)
    W = rng.integers(1, 2000, n)
    kind = rng.integers(0, 5, n)
    centre = rng.uniform(-0.3, 1.3, (n, 1, 2)) * np.stack([H, W], 1)[:, None, :]
    spread = np.where(kind[:, None, None] == 0, 0.5, np.where(kind[:, None, None] == 1, 40.0, 400.0))
    j = centre + rng.normal(0, 1, (n, 21, 2)) * spread
    j = np.where(kind[:, None, None] == 3, np.round(j), j)          # integer coordinates, as an arg-max gives them
    j[kind == 4, :, 0] = j[kind == 4, :1, 0]                          # zero span in rows
    j[(kind == 4) & (np.arange(n) % 2 == 0)] = j[(kind == 4) & (np.arange(n) % 2 == 0), :1, :]  # one pixel: zero span on both
    return np.ascontiguousarray(j, np.float64), H, W


def test_box_rule_equals_runner_bbox_update(hp):
    """crop.h's box_update on 10^5 random joint sets against runner.bbox_update, and with the loop's fallback against runner.track's."""
    from vnect_amd import runner
    n = 100_000
    j, H, W = _box_cases(n)
    got = np.empty((n, 4), np.int32)
    fb = np.empty((n, 4), np.int32)
    for i in range(n):   # (one call per frame size)
        hp.hp_box_update(j[i].ctypes.data_as(f64p), 1, int(W[i]), int(H[i]), 0, got[i:].ctypes.data_as(i32p))
        hp.hp_box_update(j[i].ctypes.data_as(f64p), 1, int(W[i]), int(H[i]), 1, fb[i:].ctypes.data_as(i32p))
    degenerate = 0
    for i in range(n):
        want = runner.bbox_update(j[i], int(W[i]), int(H[i]))
        assert list(got[i]) == want, (i, j[i], W[i], H[i], list(got[i]), want)
        if want[2] < 1 or want[3] < 1:
            want = [0, 0, int(W[i]), int(H[i])]
            degenerate += 1
        assert list(fb[i]) == want, i
    assert degenerate > 1000


def test_new_symbols_are_declared_exported_and_bound():
    from vnect_amd import _native
    hdr = open(os.path.join(ROOT, "include", "vnect_abi.h")).read()
    new = ("vnect_track_begin", "vnect_submit_tracked", "vnect_submit_tracked_pinned", "vnect_collect_tracked", "vnect_track_box")
    declared = set(re.findall(r"\b(vnect_[a-z0-9_]+)\s*\(", hdr))
    vmap = open(os.path.join(CSRC, "vnect.map")).read()
    for name in new:
        assert name in declared and name in _native.SYMBOLS, name
        assert re.search(r"^\s*vnect_\*;", vmap, re.M) or name in vmap, name
    assert "#define VNECT_ABI_VERSION 7" in hdr and _native.ABI_VERSION == 7
    assert C.sizeof(_native.Config) == 128
