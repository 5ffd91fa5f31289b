"""The people form of the preview (vnect_amd/csrc/preview.h: PreviewPeople; PEOPLE.md), shared by tests/test_people_preview_cpu.py (the
host walk, g++) and tests/test_gpu_people_kernels.py (the kernel behind the probe): the jobs, the numpy composition --
render.draw_limbs_2d_exact applied P times in person order, then render.resize_u8_exact -- and the argument lists of
preview_walk_people / pp_preview_people."""
import ctypes as C

import numpy as np

from tests import overlay_ref as R
from tests import preview_ref as V
from vnect_amd import render

u8p, f64p, i32p = V.u8p, V.f64p, V.i32p
SIZES = [(7, 5), (33, 64), (270, 480)]
CODES = [0, 3, 5]
FACTORS = [0.5, 1.7, 0.37, None, 1.0]          # shrinking, enlarging, the reference's 1024 / the longer side (enlarging here), a copy
_WALK = [u8p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, f64p, f64p,
         C.c_double, i32p, i32p, i32p, i32p, i32p, C.c_double, C.c_int, u8p, C.c_int64, C.c_int64, C.c_int64]
_EXPECTED = {}


def cpu_lib():
    L = V.cpu_lib()
    L.preview_walk_people.restype, L.preview_walk_people.argtypes = C.c_int, _WALK
    return L


def probe_lib():
    L = V.probe_lib()
    L.pp_preview_people.restype, L.pp_preview_people.argtypes = C.c_int, _WALK + [u8p]
    return L


def people(Hp, Wp, P, seed):
    """P skeletons and boxes that overlap each other and the picture's edges; confidences around 0.5"""
    rs = np.random.RandomState(seed)
    joints = np.stack([rs.uniform(-0.15 * Hp, 1.15 * Hp, (P, 21)), rs.uniform(-0.15 * Wp, 1.15 * Wp, (P, 21))], 2)
    rects = []
    for p in range(P):
        x, y = int(rs.uniform(-0.2, 0.6) * Wp), int(rs.uniform(-0.2, 0.6) * Hp)
        rects.append([x, y, max(1, int(rs.uniform(0.3, 0.9) * Wp)), max(1, int(rs.uniform(0.3, 0.9) * Hp))])
    conf = rs.uniform(0.0, 1.0, (P, 21))
    return joints, np.asarray(rects, np.int32), conf


def jobs():
    """(layout, code, factor, P, threshold or None, out format, output offset, pitch padding, seed): every size, format and P, the
    codes, factors, thresholds and output alignments going round"""
    out, n = [], 0
    for size in SIZES:
        lays = V.layouts(*size)
        for fmt in (0, 1, 2):
            lay = [lay for lay in lays if lay["format"] == fmt and not lay.get("uv_separate")][0]
            for P in (1, 2, 3, 4):
                out.append((lay, CODES[n % 3], FACTORS[(n + n // 3) % 5], P, 0.5 if n % 2 else None, (n // 2) % 2, n % 4, (n % 3) * 5, n))
                n += 1
    return out


def expected(src, lay, job):
    """THE COMPOSITION, once per job"""
    _, o, f, P, thr, fmt, _, _, seed = job
    if seed not in _EXPECTED:
        pic = V.picture(src, lay, o)
        Hp, Wp = pic.shape[:2]
        joints, rects, conf = people(Hp, Wp, P, seed)
        for p in range(P):
            pic = render.draw_limbs_2d_exact(pic, joints[p], R.PARENTS, [int(v) for v in rects[p]], confidence=None if thr is None else conf[p],
                                             min_confidence=thr)
        ff = 1024.0 / max(Hp, Wp) if f is None else f
        out = render.resize_u8_exact(pic, ff)
        assert out.shape[:2] == V.shape_of(Hp, Wp, f)
        out = np.ascontiguousarray(out[:, :, ::-1]) if fmt else out
        out.setflags(write=False)
        _EXPECTED[seed] = (out, joints, rects, conf)
    return _EXPECTED[seed]


def walk_args(src, lay, job, joints, rects, conf, out, pitch, flags=None):
    """the arguments preview_walk_people and pp_preview_people share (flags: the walk's `drawn` / the probe's `status`), and what they point
    into"""
    _, o, f, P, thr, fmt, out_off, _, _ = job
    keep = [np.ascontiguousarray(joints, np.float64), None if thr is None else np.ascontiguousarray(conf, np.float64), np.asarray(R.PARENTS, np.int32),
            np.ascontiguousarray(rects, np.int32), None if flags is None else np.asarray(flags, np.int32)]
    p = R._ptr
    args = [p(src, u8p), len(src), lay["data_off"], lay["uv_off"], lay["format"], lay["H"], lay["W"], lay["sy"], lay["sx"], lay["sc"], lay["uv_stride"], o, P,
            p(keep[0], f64p), p(keep[1], f64p), float("nan") if thr is None else float(thr), p(keep[2], i32p), p(keep[3], i32p), p(keep[4], i32p), None, None,
            0.0 if f is None else float(f), fmt, p(out, u8p), len(out), out_off, pitch]
    return args, keep


def run(backend):
    """backend(src, lay, job, joints, rects, conf, out, pitch): every job's whole output buffer equals the composition (padding and the
    bytes in front of the picture keep their canary) and its source is unchanged.  Returns the number of jobs."""
    done = 0
    for job in jobs():
        lay = job[0]
        src = V.fresh(lay, job[8])
        before = src.copy()
        exp, joints, rects, conf = expected(src, lay, job)
        out, pitch = V.out_buffer(exp.shape[0], exp.shape[1], job[6], job[7])
        backend(src, lay, job, joints, rects, conf, out, pitch)
        want = V.whole(exp, job[6], pitch)
        bad = np.nonzero(out != want)[0]
        assert len(bad) == 0, (lay["name"], "code", job[1], "factor", job[2], "P", job[3], "thr", job[4], "differing bytes", len(bad), bad[:6])
        assert np.array_equal(src, before)
        done += 1
    return done
