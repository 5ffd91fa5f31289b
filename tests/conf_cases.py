"""Case sets and CPU references for the per-joint confidence and the loss rule of a tracked stream (CONFIDENCE.md): what
tests/test_gpu_confidence.py, tests/test_gpu_conf_track_kernels.py and tests/test_gpu_conf_track_maps.py hold the device to, and the
conditions those sets must meet (tests/test_confidence_cpu.py asserts them WITHOUT a GPU, from the references alone).

Nothing in here comes from the code under test: the confidence is the maximum of the oracle's x8 upsample of the oracle's merged heat-map
(held to a plain-numpy restatement of cv2's bilinear rule), the rule is three lines of numpy, the loop is runner.track's with the rule
behind runner.bbox_update, and the box stage's reference is tests/track_cases.py's with the rule applied."""
import numpy as np

from tests import track_cases as tc

NJ, HM = 21, 46
OFF, HOLD, RESET = 0, 1, 2
ACTIONS = {"off": OFF, "hold": HOLD, "reset": RESET}


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
def conf_reference(maps, scales):
    """(21,) float64: per joint the maximum over the 368 x 368 bilinear x8 upsample of its merged heat-map -- the value of the element
    np.argmax picks in utils.py:169-172."""
    import oracle
    avg = oracle.merge_scales(maps, scales)[0]
    return np.array([oracle.resize(np.ascontiguousarray(avg[:, :, j]), 8.0).max() for j in range(NJ)], np.float64)


def upsample8_numpy(hm):
    """cv2.resize(hm float64 (46, 46), (0, 0), fx=8, fy=8, INTER_LINEAR) in plain numpy, from cv2's rule: the source coordinate of
    destination index d is (float32)((d + 0.5) / 8 - 0.5), split into floor and fraction; along x an index below 0 or at the last cell is
    clamped and its fraction zeroed, and from the first clamped-high column on the single tap is taken; along y the fraction stays and
    the two ROWS are clipped.  Weights are float32 (1 - f, f), the arithmetic float64: horizontal pass first, then vertical."""
    hm = np.asarray(hm, np.float64)
    d = np.arange(8 * HM)
    f = ((d + 0.5) * (1.0 / 8.0) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    fr = (f - s.astype(np.float32)).astype(np.float32)
    sx, fx = s.copy(), fr.copy()
    fx[sx < 0], sx[sx < 0] = 0, 0
    single = sx + 1 >= HM                      # (monotone in d: every column from the first such one on)
    fx[sx >= HM - 1], sx[sx >= HM - 1] = 0, HM - 1
    a0, a1 = (np.float32(1) - fx).astype(np.float64), fx.astype(np.float64)
    with np.errstate(invalid="ignore"):
        two = hm[:, sx] * a0 + hm[:, np.minimum(sx + 1, HM - 1)] * a1
        rows = np.where(single, hm[:, sx], two)
        b0, b1 = (np.float32(1) - fr).astype(np.float64), fr.astype(np.float64)
        return rows[np.clip(s, 0, HM - 1)] * b0[:, None] + rows[np.clip(s + 1, 0, HM - 1)] * b1[:, None]


def conf_numpy(maps, scales):
    """conf_reference with the upsample restated in numpy (the merge stays the oracle's: tests/test_oracle_post.py pins it)."""
    import oracle
    avg = oracle.merge_scales(maps, scales)[0]
    return np.array([upsample8_numpy(avg[:, :, j]).max() for j in range(NJ)], np.float64)


def same_conf(a, b):
    """Bit for bit -- up to the sign of a zero: a maximum over an array that holds +0.0 and -0.0 (tests/post_edges.py has such a map) is
    either, in numpy as anywhere, and they compare equal.  Every other float64 that compares equal has equal bits; NaN never passes."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(a == b))


def chosen_map_sets():
    """[(name, maps (S, 46, 46, 84) float32, scales)]: the map sets the definition is pinned on -- tests/post_edges.py's (known-answer
    arg-max cases, border sequence, edge maps at reference, baseline and near-1 scales, S = 1, 3, 4, 8), random float32 maps, an
    all-negative map, a constant map, peaks at cells (0, 0) and (45, 45)."""
    from tests import post_edges as pe
    out = [("argmax_cases", pe.argmax_cases()[0], [1.0])]
    out += [("border_%d" % k, m, [1.0]) for k, m in enumerate(pe.border_sequence(2))]
    for name, scales in (("reference", [1.0, 0.85, 0.7]), ("baseline", tc.BASELINE_SCALES), ("near1", [1.0, 0.9999]), ("near1_alone", [0.99]),
                         ("four", [1.0, 0.9, 0.8, 0.7]), ("eight", pe.scale_sets()[-1])):
        out.append(("edge_" + name, pe.edge_maps(8100 + len(scales), len(scales), scales), scales))
    rng = np.random.default_rng(31)
    for name, scales in (("one", [1.0]), ("baseline", tc.BASELINE_SCALES), ("eight", pe.scale_sets()[-1])):
        out.append(("random_" + name, rng.normal(0, 1, (len(scales), HM, HM, 84)).astype(np.float32), scales))
    neg = -rng.uniform(0.5, 2.0, (3, HM, HM, 84)).astype(np.float32)
    out.append(("all_negative", neg, tc.BASELINE_SCALES))
    out.append(("constant", np.full((3, HM, HM, 84), np.float32(0.3)), tc.BASELINE_SCALES))
    for name, cell in (("peak_0_0", (0, 0)), ("peak_45_45", (45, 45))):
        for scales in ([1.0], tc.BASELINE_SCALES):
            out.append(("%s_S%d" % (name, len(scales)), tc.hot_maps(len(scales), [cell] * NJ, np.random.default_rng(5), level=0.9), scales))
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def verdict(conf, min_confidence, min_joints, action):
    """(lost, confident): confident = #{j : conf[j] >= min_confidence}; lost = action != off and confident < min_joints."""
    with np.errstate(invalid="ignore"):
        confident = int(np.count_nonzero(np.asarray(conf, np.float64) >= min_confidence))
    return int(action != OFF and confident < min_joints), confident


# ---- the loop with the rule (tc.cpu_loop's pattern) ------------------------------------------------------------------------------------------
def cpu_loop(H, W, rect, maps_list, times, scales, policy=None, confs=None):
    """runner.track's loop on given maps with the loss rule behind runner.bbox_update: policy = (min_confidence, min_joints, action 0..2)
    or None.  Per frame a dict: j2, j3, used, next (the box rule's rect, before the rule and the fallback), conf, lost, confident, state
    (the TrackState bytes behind the frame).  Stops with j2 = None at a crop the squarify step refuses."""
    import oracle
    from vnect_amd import runner
    est = oracle.OracleEstimator(scales=scales, net=None)
    rect = [0, 0, W, H] if rect is None else [int(v) for v in rect]
    thr, mj, action = policy if policy is not None else (0.0, 1, OFF)
    out = []
    x, y, w, h = rect
    if w < 1 or h < 1:
        x, y, w, h = 0, 0, W, H
    state = tc.frame_state(H, W, [x, y, min(w, W - x), min(h, H - y)], past=(w - min(w, W - x), h - min(h, H - y)))
    for k, (maps, (t2d, t3d)) in enumerate(zip(maps_list, times)):
        x, y, w, h = rect
        if w < 1 or h < 1:
            x, y, w, h = rect = [0, 0, W, H]
        ch, cw = min(h, H - y), min(w, W - x)
        geo = tc.crop_geometry(ch, cw, scales) if tc.squarify_bytes(ch, cw)[1] is None else None
        if geo is None:
            out.append({"j2": None, "used": [x, y, w, h]})
            break
        j2, j3 = est.postprocess(maps, t2d, t3d, geo[0], geo[1], geo[2])
        j2[:, 0] += y
        j2[:, 1] += x
        conf = confs[k] if confs is not None else conf_reference(maps, scales)
        lost, confident = verdict(conf, thr, mj, action)
        nxt = list(runner.bbox_update(j2, W, H))
        used = [x, y, w, h]
        if lost and action == HOLD:
            rect = list(used)                                  # the state stays as it is, every byte
        elif lost:
            rect = [0, 0, W, H]
            state = tc.state_after(H, W, [0, 0, 0, 0], k + 1)
        else:
            rect = list(nxt)
            state = tc.state_after(H, W, nxt, k + 1)
        out.append({"j2": j2, "j3": j3, "used": used, "next": nxt, "conf": conf, "lost": lost, "confident": confident, "state": state.copy()})
    return out


# ---- walks on chosen maps whose confident count straddles min_joints -----------------------------------------------------------------------
WALK_FRAMES = 32
WALK_MIN_JOINTS = 11
EXACT_FRAME, EXACT_JOINT = 11, 4      # the threshold IS this joint's reference confidence on this frame
WALK_SIZES = {(1080, 1920): 21, (64, 96): 22}      # (H, W) -> seed
# per frame how many joints stand out ("present"): everybody, nobody, or around min_joints
_PLAN = [21] * 6 + [0] * 4 + [21, 11, 10, 11, 21, 21, 12] + [0] * 5 + [21, 0, 21, 0, 21, 21, 10, 21, 21, 21]


def conf_maps(S, cells, levels, rng):
    """tc.hot_maps with one level per joint: noise up to 0.05 under the peaks, random location maps."""
    m = tc.hot_maps(S, cells, rng, level=0.0)
    for j, (r, c) in enumerate(cells):
        m[:, r, c, j] = np.float32(levels[j])
    return m


def walk_spec(seed, n=WALK_FRAMES):
    """(cells (n, 21, 2), levels (n, 21), noise seeds (n,)): clusters of hot cells mostly inside the maps' middle, peak levels far above the
    noise for the joints that stand out (1.5 .. 2.0; the EXACT joint on the EXACT frame 0.5, the weakest of that frame's eleven) and
    at the noise's own level for the others."""
    assert len(_PLAN) == n and _PLAN[EXACT_FRAME] == WALK_MIN_JOINTS
    rng = np.random.default_rng(seed)
    cells = np.empty((n, NJ, 2), np.int64)
    levels = np.empty((n, NJ), np.float64)
    for k in range(n):
        centre = rng.uniform(12, 33, 2)
        spread = rng.uniform(0.8, 6, 2)
        cells[k] = np.clip(np.rint(centre + rng.normal(0, 1, (NJ, 2)) * spread), 0, 45)
        out = rng.permutation(NJ)[:_PLAN[k]]
        if k == EXACT_FRAME and EXACT_JOINT not in out:
            out[0] = EXACT_JOINT
        levels[k] = rng.uniform(0.0, 0.05, NJ)
        levels[k, out] = rng.uniform(1.5, 2.0, len(out))
        if k == EXACT_FRAME:
            levels[k, EXACT_JOINT] = 0.5
    return cells, levels, np.arange(n, dtype=np.int64) + 1000 * seed


def walk_maps(spec, scales, k):
    cells, levels, seeds = spec
    return conf_maps(len(scales), [tuple(c) for c in cells[k]], levels[k], np.random.default_rng(int(seeds[k])))


_WALKS = {}


def walk_reference(H, W, action, above, scales=tc.BASELINE_SCALES):
    """The CPU loop over the (H, W) walk under (threshold, WALK_MIN_JOINTS, action); threshold: the EXACT joint's confidence on the EXACT
    frame -- or, `above`, the next float64 above it.  Returns (policy, frames)."""
    key = (H, W, action, bool(above))
    if key not in _WALKS:
        spec = walk_spec(WALK_SIZES[(H, W)])
        ckey = (H, W, "conf")
        if ckey not in _WALKS:
            maps = [walk_maps(spec, scales, k) for k in range(WALK_FRAMES)]
            _WALKS[ckey] = (maps, [conf_reference(m, scales) for m in maps])
        maps, confs = _WALKS[ckey]
        thr = float(confs[EXACT_FRAME][EXACT_JOINT])
        if above:
            thr = float(np.nextafter(thr, np.inf))
        policy = (thr, WALK_MIN_JOINTS, action)
        _WALKS[key] = (policy, cpu_loop(H, W, None, maps, tc.walk_times(WALK_FRAMES), scales, policy, confs))
    return _WALKS[key]


def walk_conditions(policy, frames):
    """The counts the conditions are stated in, from the reference alone."""
    thr, mj, _ = policy
    lost = [f["lost"] for f in frames]
    streak = best = 0
    for v in lost:
        streak = streak + 1 if v else 0
        best = max(best, streak)
    return {"frames": len(frames), "lost": sum(lost), "kept": len(lost) - sum(lost), "streak": best,
            "recoveries": sum(1 for a, b in zip(lost, lost[1:]) if a and not b),
            "at_min": sum(1 for f in frames if f["confident"] == mj), "below_min": sum(1 for f in frames if f["confident"] == mj - 1),
            "exact": sum(1 for f in frames if np.any(f["conf"] == thr)),
            "just_below": sum(1 for f in frames if np.any(np.nextafter(f["conf"], np.inf) == thr))}


# ---- the box stage with a policy, case by case (tests/test_gpu_conf_track_kernels.py) --------------------------------------------------------
GARBAGE_I32 = int(np.array([tc.GARBAGE] * 4, np.uint8).view(np.int32)[0])


def policy_cases():
    """tc.box_cases()'s states and joints -- every targeted case and one random case in five -- with random confidences (NaN, +-inf and
    values exactly on the threshold among them), thresholds, min_joints and all three actions."""
    base = tc.box_cases()
    keep = np.nonzero((base["tag"] != "random") | (np.arange(len(base["tag"])) % 5 == 0))[0]
    n = len(keep)
    rng = np.random.default_rng(77)
    conf = rng.uniform(0, 1, (n, NJ))
    thr = rng.uniform(0.15, 0.85, n)
    odd = rng.integers(0, 8, n)
    for i in np.nonzero(odd == 0)[0]:
        conf[i, rng.integers(0, NJ, 3)] = (np.nan, np.inf, -np.inf)
    for i in np.nonzero(odd == 1)[0]:
        thr[i] = conf[i, rng.integers(0, NJ)]                       # a confidence exactly on the threshold counts
    for i in np.nonzero(odd == 2)[0]:
        thr[i] = np.nextafter(conf[i, rng.integers(0, NJ)], np.inf)  # ... and one an ulp below it does not
    thr[odd == 3] = -np.inf
    min_joints = rng.integers(1, NJ + 1, n).astype(np.int32)
    near = np.nonzero(odd >= 5)[0]                                   # min_joints at and right above the count: the rule's own edge
    with np.errstate(invalid="ignore"):
        count = (conf >= thr[:, None]).sum(1)
    min_joints[near] = np.clip(count[near] + (near % 2), 1, NJ)
    action = (np.arange(n) % 3).astype(np.int32)
    return {"hdr": base["hdr"][keep], "joints": base["joints"][keep], "xseq": base["xseq"][keep], "tag": base["tag"][keep],
            "conf": np.ascontiguousarray(conf), "thr": np.ascontiguousarray(thr), "min_joints": min_joints, "action": action}


def policy_reference(cases):
    """tc.box_reference with the rule: a held state keeps its header (and, in the probe, the garbage its geometry was filled with); a
    reset one is the whole frame's.  verdict (n, 2): lost, confident -- the probe's garbage for a state that arrives refused."""
    ref = tc.box_reference(cases)
    n = len(cases["hdr"])
    nh = 4 * tc.HDR_INTS
    ver = np.empty((n, 2), np.int32)
    for i in range(n):
        x, y, w, h, uw, uh, H, W, status, _ = (int(v) for v in cases["hdr"][i])
        if status != tc.SQ_OK:
            ver[i] = GARBAGE_I32
            continue
        lost, confident = verdict(cases["conf"][i], cases["thr"][i], int(cases["min_joints"][i]), int(cases["action"][i]))
        ver[i] = [lost, confident]
        if not lost:
            continue
        if cases["action"][i] == HOLD:
            ref["hdr"][i] = cases["hdr"][i]
            ref["states"][i, :nh] = np.ascontiguousarray(cases["hdr"][i], np.int32).view(np.uint8)
            ref["states"][i, nh:] = tc.GARBAGE
        else:
            fp, msg = tc.squarify_bytes(H, W)      # (tc.state_after's rule, with fail wrapped to 32 bits as the device's xseq + 1 is)
            code = tc.CODE_OF[msg]
            fail = np.uint32((int(cases["xseq"][i]) + 1) & 0xFFFFFFFF).astype(np.int32) if code else 0
            ref["hdr"][i] = [0, 0, W, H, W, H, H, W, code, fail]
            ref["states"][i, :nh] = np.ascontiguousarray(ref["hdr"][i], np.int32).view(np.uint8)
            ref["states"][i, nh:] = fp
    ref["verdict"] = ver
    return ref
