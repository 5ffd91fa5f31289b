"""CPU: the people form of the preview rule (vnect_amd/csrc/preview.h: PreviewPeople, through preview_capi.cpp's preview_walk_people,
g++) against numpy -- render.draw_limbs_2d_exact applied P times in person order, then render.resize_u8_exact -- byte for byte: P = 1 .. 4;
frames of 7 x 5, 33 x 64 and 270 x 480; factors that shrink and that enlarge; boxes and skeletons that overlap each other and the frame's
edge; BGR, RGB and NV12; orientations 0, 3 and 5; confidences that drop limbs.  With P = 1 it is render.preview_exact and the one-person
walk's bytes."""
import numpy as np

from tests import overlay_ref as R
from tests import people_preview_ref as PP
from tests import preview_ref as V
from vnect_amd import render


def _backend(src, lay, job, joints, rects, conf, out, pitch):
    args, keep = PP.walk_args(src, lay, job, joints, rects, conf, out, pitch)
    assert PP.cpu_lib().preview_walk_people(*args) == 0, (lay["name"], job[1:])


def test_people_walk_equals_the_numpy_composition():
    jobs = PP.jobs()
    assert {j[3] for j in jobs} == {1, 2, 3, 4} and {j[1] for j in jobs} == {0, 3, 5} and {j[0]["format"] for j in jobs} == {0, 1, 2}
    assert any(j[4] is not None for j in jobs) and any(j[2] == 1.7 for j in jobs) and any(j[2] == 0.5 for j in jobs)
    assert PP.run(_backend) == len(jobs) == 36


def test_one_person_is_preview_exact_and_the_one_person_walk():
    for job in [j for j in PP.jobs() if j[3] == 1]:
        lay, o, f, _, thr, fmt, out_off, pad, seed = job
        src = V.fresh(lay, seed)
        exp, joints, rects, conf = PP.expected(src, lay, job)
        pic = V.picture(src, lay, o)
        want = render.preview_exact(pic, joints[0], R.PARENTS, [int(v) for v in rects[0]], factor=f, out_format="rgb" if fmt else "bgr",
                                    confidence=None if thr is None else conf[0], min_confidence=thr)
        assert np.array_equal(exp, want), (lay["name"], job[1:])
        out, pitch = V.out_buffer(exp.shape[0], exp.shape[1], out_off, pad)
        one = out.copy()
        _backend(src, lay, job, joints, rects, conf, out, pitch)
        case = dict(joints=joints[0], parents=R.PARENTS, rect=[int(v) for v in rects[0]], conf=None if thr is None else conf[0], thr=thr)
        args, keep = V.walk_args(src, lay, o, case, f, fmt, one, out_off, pitch)
        assert V.cpu_lib().preview_walk(*args) == 0
        assert np.array_equal(out, one), (lay["name"], job[1:])


def test_a_person_left_out_is_not_drawn_and_bad_arguments_are_refused():
    job = [j for j in PP.jobs() if j[3] == 3 and j[0]["format"] == 0][1]
    lay = job[0]
    src = V.fresh(lay, job[8])
    exp, joints, rects, conf = PP.expected(src, lay, job)
    # person 1 left out (a refused crop): the picture is that of persons 0 and 2
    two = (lay, job[1], job[2], 2, job[4], job[5], job[6], job[7], 10_000 + job[8])
    PP._EXPECTED.pop(two[8], None)
    pic = V.picture(src, lay, job[1])
    for p in (0, 2):
        pic = render.draw_limbs_2d_exact(pic, joints[p], R.PARENTS, [int(v) for v in rects[p]], confidence=None if job[4] is None else conf[p],
                                         min_confidence=job[4])
    f = 1024.0 / max(pic.shape[:2]) if job[2] is None else job[2]
    want = render.resize_u8_exact(pic, f)
    want = want[:, :, ::-1] if job[5] else want
    out, pitch = V.out_buffer(want.shape[0], want.shape[1], job[6], job[7])
    args, keep = PP.walk_args(src, lay, job, joints, rects, conf, out, pitch, flags=[1, 0, 1])
    assert PP.cpu_lib().preview_walk_people(*args) == 0
    assert np.array_equal(out, V.whole(np.ascontiguousarray(want), job[6], pitch))
    before = out.copy()
    for P in (0, 5):
        bad = list(args)
        bad[12] = P
        assert PP.cpu_lib().preview_walk_people(*bad) == -1
    flat = rects.copy()
    flat[1, 2] = 0
    args, keep = PP.walk_args(src, lay, job, joints, flat, conf, out, pitch)
    assert PP.cpu_lib().preview_walk_people(*args) == -1 and np.array_equal(out, before)
