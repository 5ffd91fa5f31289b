"""CPU: the case sets of the device tracking tests (tests/track_cases.py) meet the conditions they were written for -- asserted from the
references alone (runner.bbox_update, hostplan.h's squarify), so what tests/test_gpu_track_kernels.py and tests/test_gpu_track_maps.py
claim to cover does not depend on a GPU run -- and `make trackprobe` links the product's own kernel objects."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import track_cases as tc


@pytest.fixture(scope="module")
def box():
    cases = tc.box_cases()
    return cases, tc.box_reference(cases)


def test_layout_constants_are_the_headers():
    """The TrackState image the tests pack (10 ints + FrameParams) against tables.h as the host build sees it, and kernels.h's text."""
    assert tc.hostplan().hp_frame_params_size() == tc.FP_BYTES == 5192
    src = open(os.path.join(tc.CSRC, "kernels.h")).read()
    body = re.search(r"struct TrackState \{(.*?)\n\};", src, re.S).group(1)
    fields = re.findall(r"^\s*(?:int|unsigned|FrameParams) ([A-Za-z, ]+);", body, re.M)
    assert [f.replace(" ", "") for f in fields] == ["x,y,w,h", "uw,uh", "H,W", "status", "fail", "fp"], fields


def test_box_cases_meet_their_conditions(box):
    """The issue's conditions on the box cases.  Refused "scaled long side != 368" (SQ_LONG): NO crop size up to 8192 x 8192 takes it --
    the long side L scales to cv_round(L * (368.0 / L)), searched here for every L in 1 .. 8192 and 368 for all of them -- so no box case
    can produce it; the status code itself is still covered by the states that ARRIVE refused."""
    cases, ref = box
    c = tc.box_conditions(cases, ref)
    print(c)
    assert c["cases"] >= 20000 and len(cases["joints"]) == len(cases["xseq"]) == c["cases"]
    assert c["fallback"] >= 1000 and c["fallback_w0_only"] >= 1 and c["fallback_h0_only"] >= 1 and c["fallback_both"] >= 1, c
    assert c["refused_scaled"] >= 200, c
    assert tc.long_side_refusals(8192) == [] and c["refused_long"] == 0, c
    assert min(c["copy"], c["tall"], c["wide"], c["above_736"]) >= 100, c
    assert c["half"] >= 50 and c["half_refused"] >= 8 and c["half_accepted"] >= 8, c
    assert c["initial"] >= 100, c
    assert c["arrives_refused"] >= 100, c
    assert min(c["route_wide"], c["route_tall"], c["route_clamp"]) >= 1, c
    j = cases["joints"]
    assert np.all(np.isfinite(j)) and np.abs(j).max() < 1e9 and np.abs(ref["joints"]).max() < 1e9
    assert cases["hdr"][:, 6].max() > 8000 and cases["hdr"][:, 7].max() > 8000   # frames up to 8192 x 8192


def test_half_cases_separate_the_two_roundings(box):
    """736 x 1 scales to 0.5 and 736 x 3 to 1.5: half-to-even gives 0 (refused) and 2, half-away would give 1 and 2 -- the cases on a half
    include sizes where the two roundings differ."""
    cases, ref = box
    new, st = ref["hdr"], ref["info"]["status"]
    sizes = {(int(h), int(w)): int(s) for (w, h), s in zip(new[:, 2:4], st) if s >= 0}
    for long_side, short, want in ((736, 1, tc.SQ_SCALED), (736, 3, tc.SQ_OK), (736, 5, tc.SQ_OK), (1472, 2, tc.SQ_SCALED), (1472, 6, tc.SQ_OK)):
        assert sizes[(long_side, short)] == want and sizes[(short, long_side)] == want, (long_side, short)
    fp, _ = tc.squarify_bytes(736, 5)
    assert tc.fp_head(fp)[6] == 2          # 2.5 rounds to 2 (half-away: 3)


def test_sweep_cases_give_the_whole_frame():
    """Every (h, w) of the geometry sweep as a box case: runner.bbox_update and the fallback give exactly [0, 0, w, h]."""
    from vnect_amd import runner
    sizes = tc.dense_sizes() + tc.random_sizes()
    assert len(sizes) > 80000
    cases = tc.sweep_cases(sizes)
    for i in range(0, len(sizes), 7):
        h, w = sizes[i]
        r = runner.bbox_update(cases["joints"][i], w, h)
        if r[2] < 1 or r[3] < 1:
            r = [0, 0, w, h]
        assert r == [0, 0, w, h], (sizes[i], r)
    ref = tc.box_reference({k: v[-8:] for k, v in cases.items()})   # the sizes out of range: (0, 5) ... (8192, 8192)
    assert list(ref["info"]["status"]) == [tc.SQ_OK, tc.SQ_OK] + [tc.SQ_RANGE] * 5 + [tc.SQ_OK]


def test_copy_cases_meet_their_conditions():
    phases, groups, last_byte, last_row, widest = set(), set(), 0, 0, 0
    for f in tc.copy_cases():
        used = (f["H"] - 1) * f["stride"] + 3 * f["W"]
        for x, y, w, h in f["crops"]:
            assert 0 <= x and 0 <= y and w >= 1 and h >= 3 and x + w <= f["W"] and y + h <= f["H"], (f["W"], x, y, w, h)
            phases.add((x % 4, w % 4, 3 * w % 4, f["stride"] % 4))
            groups.add(tc.copy_workgroups(w))
            last_row += y + h == f["H"]
            last_byte += (y + h - 1) * f["stride"] + 3 * (x + w) == used
        widest = max(widest, f["W"])
    for align in (0, 2, 3):                  # (row strides 0, 2 and 3 mod 4: the source phase of a row stays or moves)
        assert {(x, w) for x, w, _, a in phases if a == align} == {(x, w) for x in range(4) for w in range(4)}, align
    assert {p[2] for p in phases} == {0, 1, 2, 3}
    assert 1 in groups and 2 in groups and max(groups) > 6 and widest == 8192, groups
    assert last_row >= 8 and last_byte >= 8


def test_pyramid_cases_meet_their_conditions():
    frames = {(f["W"], f["H"]) for f in tc.pyramid_cases()}
    assert frames == {(640, 480), (1920, 1080), (1080, 1920), (4096, 2160)}
    kinds = {"wide": 0, "tall": 0, "copy": 0, "thin": 0, "refused": 0, "odd": 0, "last_byte": 0, "above_736": 0}
    for f in tc.pyramid_cases():
        for x, y, w, h in f["crops"]:
            assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= f["W"] and y + h <= f["H"]
            fp, msg = tc.squarify_bytes(h, w)
            kinds["odd"] += x % 2 == 1 and y % 2 == 1
            kinds["last_byte"] += x + w == f["W"] and y + h == f["H"]
            if msg is not None:
                kinds["refused"] += 1
                continue
            _, offx, offy, _, _, dh, dw, _, copy = tc.fp_head(fp)
            kinds["wide"] += dw > dh and offy > 0
            kinds["tall"] += dh > dw and offx > 0
            kinds["copy"] += copy == 1 and max(h, w) == 368
            kinds["thin"] += min(w, h) <= 3
            kinds["above_736"] += max(w, h) > 736
    assert all(v >= (3 if k == "refused" else 4) for k, v in kinds.items()), kinds
    thin = {min(w, h) for f in tc.pyramid_cases() for _, _, w, h in f["crops"] if tc.squarify_bytes(h, w)[1] is None}
    assert {1, 2, 3} <= thin


def _make(*args):
    return subprocess.check_output(["make", "-C", tc.CSRC] + list(args), text=True)


def _db_rule(db, target):
    """(prerequisites, recipe lines as written) of `target` in the database `make -p` prints"""
    block = re.search(r"^%s:(.*)\n((?:.+\n)*)" % re.escape(target), db, re.M)
    return block.group(1).split(), [ln for ln in block.group(2).splitlines() if ln.startswith("\t")]


def test_trackprobe_links_the_products_objects():
    """`make trackprobe` links the object files the shipped library links: its prerequisites, as make resolves them, are the product's
    track.o and post.o, and no .hip is compiled for it (the only compile of its own is the shim, track_probe.cpp)."""
    db = _make("-pn", "trackprobe")
    prereq, recipe = _db_rule(db, "../lib/libvnect_trackprobe.so")
    shipped, _ = _db_rule(_make("-pn"), "../lib/libvnect_hip.so")
    assert "../lib/obj/track.o" in shipped and "../lib/obj/post.o" in shipped
    assert prereq == ["../lib/obj/track.o", "../lib/obj/post.o", "../lib/obj/track_probe.o"], prereq
    assert len(recipe) == 1 and "$(filter %.o,$^)" in recipe[0] and ".hip" not in recipe[0] and " -c " not in recipe[0], recipe
    # one compile rule each for track.o and post.o, the product's: one rule line in the Makefile, and in a build from nothing one
    # command that writes the object, the same command the product's own build runs
    mk = open(os.path.join(tc.CSRC, "Makefile")).read()
    assert len(re.findall(r"^\$\(OBJ\)/(?:track|post)\.o:", mk, re.M)) == 2
    product, probe = _make("-n", "-B").splitlines(), _make("-n", "-B", "trackprobe").splitlines()
    for k in ("track", "post"):
        writes = [ln for ln in probe if "-o ../lib/obj/%s.o" % k in ln]
        assert len(writes) == 1 and "-c %s.hip" % k in writes[0] and product.count(writes[0]) == 1, writes
    # ... and the product does not know it: not in the exported-symbol map, not loaded by the binding
    assert "tp_" not in open(os.path.join(tc.CSRC, "vnect.map")).read()
    native = open(os.path.join(tc.ROOT, "vnect_amd", "_native.py")).read()
    assert "CDLL(LIB_PATH)" in native and "CDLL(TRACKPROBE" not in native


PROBE_LINKS = {   # probe: its shim, and the product's objects it links, in link order
    "track": ("track_probe.cpp", ["track", "post"]),
    "nv12": ("nv12_probe.cpp", ["track", "post"]),
    "ingest": ("ingest_probe.hip", ["track", "post"]),
    "overlay": ("overlay_probe.hip", ["overlay"]),
    "orient": ("orient_probe.hip", ["orient", "track", "post"]),
    "preview": ("preview_probe.hip", ["preview"]),
    "hog": ("hog_probe.hip", ["hog"]),
    "redetect": ("redetect_probe.hip", ["hog"]),
    "view3d": ("view3d_probe.hip", ["view3d"]),
}


@pytest.mark.parametrize("name", sorted(PROBE_LINKS))
def test_probe_compiles_only_its_shim(name):
    """What make would run if only a probe's shim had changed: the shim's compile and the link of the product's objects with it,
    nothing else -- no probe recompiles a kernel."""
    shim, kernels = PROBE_LINKS[name]
    objs = ["../lib/obj/%s.o" % k for k in kernels]
    out = _make("-n", "-W", shim, *[a for o in objs for a in ("-o", o)], name + "probe")
    cmds = [ln for ln in out.splitlines() if "hipcc" in ln]
    assert len(cmds) == 2 and "-c %s " % shim in cmds[0] and out.count(".hip") + out.count(".cpp") == 1, out
    assert " ".join(objs + ["../lib/obj/%s_probe.o" % name]) in cmds[1] and "libvnect_%sprobe.so" % name in cmds[1], cmds[1]
    assert "-Wl,--no-undefined" in cmds[1] and " -c " not in cmds[1]
    # every object the probe links besides its shim is one the shipped library links
    prereq, _ = _db_rule(_make("-pn", name + "probe"), "../lib/libvnect_%sprobe.so" % name)
    shipped, _ = _db_rule(_make("-pn"), "../lib/libvnect_hip.so")
    assert prereq == objs + ["../lib/obj/%s_probe.o" % name] and set(objs) <= set(shipped), prereq


def test_refusal_scenario_reaches_a_refused_crop():
    """tests/test_gpu_track_maps.py's refusal scenario, on the CPU loop alone: the chosen maps grow [1079, 46, 1, 1565] out of the crop
    [702, 100, 300, 1500] of a 1920 x 1080 (H x W) frame -- a one-pixel extent that the clamp to the frame's edge left -- and hostplan.h's
    squarify refuses it."""
    R = tc.REFUSAL
    m = tc.hot_maps(3, R["cells"])
    out = tc.cpu_loop(R["H"], R["W"], R["rect"], [m, m], [(tc.T0, tc.T0 + 0.001), (tc.T0 + 0.03, tc.T0 + 0.031)], R["scales"])
    assert out[0][2] == R["rect"] and out[0][3] == R["next"] == [1079, 46, 1, 1565]
    assert out[1][0] is None and tc.squarify_bytes(1565, 1)[1] == "squarify: scaled size exceeds 368"
    j2 = out[0][0]
    assert (j2[:, 1] > R["rect"][0] + R["rect"][2]).all() and j2[:, 1].max() > R["W"]    # joints outside the crop, and outside the frame


def test_random_walks_meet_their_conditions():
    """The CPU loop alone, with the fixed seeds: at least 40 distinct crop sizes per frame size, at least 3 fallbacks overall, crops over
    736 on each axis (in every frame that is larger than that), joints outside the crop, outside the frame and negative, no refused crop
    (the refusal has its own scenario)."""
    fallbacks, negative = 0, 0
    for (H, W), seed in tc.WALKS.items():
        out = tc.walk_reference(H, W, seed)
        assert len(out) == tc.WALK_FRAMES and all(o[0] is not None for o in out), (H, W)
        assert len({(o[2][2], o[2][3]) for o in out}) >= 40, (H, W)
        fallbacks += sum(1 for o in out if o[3][2] < 1 or o[3][3] < 1)
        negative += sum(1 for o in out if o[0].min() < 0)
        outside_crop = sum(1 for o in out if (o[0][:, 1] < o[2][0]).any() or (o[0][:, 1] >= o[2][0] + o[2][2]).any())
        outside_frame = sum(1 for o in out if (o[0][:, 0] >= H).any() or (o[0][:, 1] >= W).any())
        assert outside_crop >= 5 and outside_frame >= 1, (H, W, outside_crop, outside_frame)
        if W > 736:
            assert any(o[2][2] > 736 for o in out), (H, W)
        if H > 736:
            assert any(o[2][3] > 736 for o in out), (H, W)
        assert any(o[2] == [0, 0, W, H] for o in out[1:]) or (H, W) == (480, 640)   # the whole frame again, behind a fallback
    assert fallbacks >= 3 and negative >= 4, (fallbacks, negative)
