"""CPU: the ABI v7 entry points of two streams per launch (vnect_set_stream_batch, vnect_submit_streams, vnect_get_batch_layer_info) are
declared with the reference lines they mirror and refuse a NULL handle; the host planning of the stem's two-frame form (hostplan.h:
stem_frame_fits with per_stream, through hostplan_capi.cpp) decides per batch of 2 S images."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vnect_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vnect_set_stream_batch", "vnect_submit_streams", "vnect_get_batch_layer_info")


def test_new_declarations_cite_reference_lines():
    hdr = open(os.path.join(ROOT, "include", "vnect_abi.h")).read()
    assert re.search(r"#define VNECT_ABI_VERSION 7\b", hdr)
    for fn in NEW:
        pos = hdr.index("int " + fn + "(")
        comment = hdr[hdr.rindex("/*", 0, pos):pos]
        assert re.search(r"(src/\w+|run_estimator_ps)\.py:\d+", comment), fn
        assert fn in _native.SYMBOLS


def test_null_handle_is_refused():
    L = _native.lib()
    assert L.vnect_set_stream_batch(None, 2) == _native.E_ARG
    s = (C.c_int32 * 2)(0, 1)
    t = (C.c_double * 2)(1.0, 2.0)
    assert L.vnect_submit_streams(None, 2, s, s, t, t) == _native.E_ARG
    assert L.vnect_get_batch_layer_info(None, 0, C.byref(_native.LayerInfo())) == _native.E_ARG


def _hp():
    csrc = os.path.join(ROOT, "vnect_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "hostplan"], stdout=subprocess.DEVNULL)
    hp = C.CDLL(os.path.join(ROOT, "vnect_amd", "lib", "libvnect_hostplan.so"))
    f64p = C.POINTER(C.c_double)
    hp.hp_stem_frame_fits.argtypes = [f64p, C.c_int, C.c_int, C.c_int]
    hp.hp_stem_frame_fits_streams.argtypes = [f64p, C.c_int, C.c_int]
    return hp, f64p


def test_two_frame_stem_fits_at_two_s_images():
    """Image i of a batch is scale i % S of frame i / S, and the tiles are those of 2 S images (stem_groups(2 S)): the frame form of a
    batch must agree with the one-frame check of the scale list written out twice, and can differ from one frame at the same scales."""
    hp, f64p = _hp()

    def one(scales, bf16=0):
        s = np.array(scales + [1.0] * (8 - len(scales)), np.float64)
        return hp.hp_stem_frame_fits(s.ctypes.data_as(f64p), len(scales), 0, bf16)

    def two(scales, bf16=0):
        s = np.array(scales + [1.0] * (8 - len(scales)), np.float64)
        return hp.hp_stem_frame_fits_streams(s.ctypes.data_as(f64p), len(scales), bf16)

    for scales in ([1.0], [1.0, 0.7], [1.0, 0.8, 0.6], [1.0, 0.85, 0.7], [1.0, 0.5], [1.0, 0.3], [1.0, 0.8, 0.3], [1.0, 0.9, 0.8, 0.7]):
        for bf16 in (0, 1):
            assert two(scales, bf16) == one(scales + scales, bf16), (scales, bf16)
    assert two([1.0, 0.8, 0.6]) == 1 and two([1.0, 0.8, 0.6], 1) == 1 and two([1.0]) == 1
    assert one([1.0, 0.3]) == 1 and two([1.0, 0.3]) == 0   # two images: 2- and 3-row tiles; four: 4- and 5-row tiles, more frame rows
    assert two([1.0, 0.8, 0.6, 0.5, 0.4]) == -1             # 2 S > 8: no batched plan
