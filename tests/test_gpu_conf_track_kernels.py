"""GPU: the box stage with a loss rule (trackbox.h behind launch_track_box's policy form), case by case through the tracking kernels'
probe (`make trackprobe`: tp_box_policy over the product's own track.o and post.o), against tests/conf_cases.py's policy_reference --
tests/track_cases.py's box reference with the rule applied.  Before every launch the ConfOut and the next state's geometry hold
garbage, so a field nobody wrote shows.  Every comparison is bit for bit; a case the shim refuses fails the test."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import conf_cases as cc
from tests import track_cases as tc

pytestmark = pytest.mark.gpu

u8p, f64p, i32p, u32p = tc.u8p, tc.f64p, tc.i32p, tc.u32p


def _p(a, t):
    return a.ctypes.data_as(t)


def test_box_stage_with_a_policy_equals_the_cpu_rule():
    from vnect_amd import _native
    path = os.environ.get("VNECT_TRACKPROBE_LIB") or _native.TRACKPROBE_LIB
    assert os.path.exists(path), "libvnect_trackprobe.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
    L = C.CDLL(path)
    L.tp_box_policy.argtypes = [C.c_int, u8p, f64p, u32p, f64p, f64p, i32p, i32p, u8p, i32p, f64p, i32p, i32p]
    cases = cc.policy_cases()
    ref = cc.policy_reference(cases)
    n = len(cases["hdr"])
    assert n >= 5000
    states = tc.pack_states(cases["hdr"])
    joints = np.ascontiguousarray(cases["joints"], np.float64)
    xseq = np.ascontiguousarray(cases["xseq"], np.uint32)
    s_out, t_out = np.zeros((n, tc.STATE_BYTES), np.uint8), np.zeros((n, 6), np.int32)
    j_out, ver, err = np.zeros((n, 21, 2), np.float64), np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    rc = L.tp_box_policy(n, _p(states, u8p), _p(joints, f64p), _p(xseq, u32p), _p(cases["conf"], f64p), _p(cases["thr"], f64p),
                         _p(cases["min_joints"], i32p), _p(cases["action"], i32p), _p(s_out, u8p), _p(t_out, i32p), _p(j_out, f64p),
                         _p(ver, i32p), _p(err, i32p))
    assert rc == 0, (rc, np.nonzero(err)[0][:8])
    first = lambda m: int(np.nonzero(m)[0][0])   # noqa: E731
    what = lambda i: (i, cases["tag"][i], "action", int(cases["action"][i]), "min_joints", int(cases["min_joints"][i]))   # noqa: E731
    # lost / confident (the probe's garbage for a state that arrives refused: the box stage does not run)
    bad = np.any(ver != ref["verdict"], axis=1)
    assert not bad.any(), ("verdict", what(first(bad)), ver[first(bad)], ref["verdict"][first(bad)])
    bad = np.any(j_out.view(np.uint64) != ref["joints"].view(np.uint64), axis=(1, 2))
    assert not bad.any(), ("joints", what(first(bad)))
    bad = np.any(t_out[:, :5] != ref["tout"], axis=1)
    assert not bad.any(), ("tout", what(first(bad)), t_out[first(bad)], ref["tout"][first(bad)])
    nh = 4 * tc.HDR_INTS
    got_hdr = np.ascontiguousarray(s_out[:, :nh]).view(np.int32)
    bad = np.any(got_hdr != ref["hdr"], axis=1)
    assert not bad.any(), ("state", what(first(bad)), cases["hdr"][first(bad)], got_hdr[first(bad)], ref["hdr"][first(bad)])
    # the geometry: the next crop's, the whole frame's behind a reset, untouched garbage behind a hold
    bad = np.any(s_out[:, nh:] != ref["states"][:, nh:], axis=1)
    assert not bad.any(), ("FrameParams", what(first(bad)), int((s_out[first(bad), nh:] != ref["states"][first(bad), nh:]).sum()))
