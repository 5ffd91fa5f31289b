"""Case sets for the post-processing at the places where post.hip can go wrong: map borders, the seams of the arg-max slabs and
waves, and scales so close to 1 that the merge's resize is a plain copy.  Pure numpy; tests/test_post_edges_cpu.py pins the
reference on them without a GPU, tests/test_gpu_post_edges.py runs the device through them.

Nothing in here comes from the code under test.  The arg-max answers are derived by hand from cv2's x8 bilinear upsample
(src = (d + 0.5) / 8 - 0.5: cell k's centre lies between rows 8k + 3 and 8k + 4, which tie; rows 0..3 repeat cell 0 and rows 364..367
cell 45) and np.argmax's first-maximum rule; the CPU test holds them to the oracle and to a brute-force numpy upsample."""
import numpy as np

from vnect_amd.weights import uniform01

NJ, HM = 21, 46
SEAM_CELLS = (5, 11, 17, 23, 29, 35, 41)   # cell k's tied rows 8k+3 | 8k+4 are the last row of one arg-max slab and the first of the next (48m+43 | 48m+44)


def _loc_maps(m, seed):
    """channels 21..83 of every scale of m: helpers.synth_maps' ramps plus hash noise, so that a border read-off sees non-trivial cells"""
    S = m.shape[0]
    m[:, :, :, NJ:] = (uniform01(seed, S * HM * HM * 63).reshape(S, HM, HM, 63).astype(np.float64) - 0.5) * 0.1
    yy, xx = np.mgrid[0:HM, 0:HM].astype(np.float64)
    for j in range(NJ):
        m[:, :, :, 21 + j] += (xx - 23) / 23.0 * (1 + 0.1 * j)
        m[:, :, :, 42 + j] += (yy - 23) / 23.0 * (1 - 0.02 * j)
        m[:, :, :, 63 + j] += np.sin(0.1 * (xx + yy) + j)


def argmax_cases():
    """((1,46,46,84) float32 maps, (21,2) expected raw arg-max [row, col]): one case per heat-map channel, every value exact in
    float32, so with S = 1 the merged map IS the input.  The root joint (14) has an interior peak."""
    m = np.zeros((1, HM, HM, 84), np.float64)
    _loc_maps(m, 4242)
    h = m[0, :, :, :NJ]
    third = float(np.float32(1.0 / 3.0))
    want = []

    def case(j, rc):
        assert j == len(want)
        want.append(rc)

    h[4:8, 6:10, 0] = 1.0                      # a plateau over the slab seam (rows 43|44) and the wave boundary (columns 63|64)
    case(0, (36, 52))
    for j, (cy, cx) in enumerate([(0, 0), (45, 45), (0, 45), (45, 0), (0, 20), (45, 20), (20, 0), (20, 45)], start=1):
        h[cy, cx, j] = 1.0                     # corners and border cells: the clamped rows / columns are plateaus, the far ones the single tap
        case(j, (0 if cy == 0 else 8 * cy + 3 if cy < 45 else 364, 0 if cx == 0 else 8 * cx + 3 if cx < 45 else 364))
    h[5, 10, 9], h[4, 10, 9], h[6, 10, 9] = 1.0, 0.5, 0.5   # rows 43 and 44 tie exactly, in two slabs
    case(9, (43, 83))
    h[40, 3, 10] = h[2, 40, 10] = float(np.float32(0.7))    # equal maxima in far-apart slabs: the earlier one
    case(10, (19, 323))
    h[10:14, 14:18, 11] = third
    case(11, (84, 116))
    h[11:13, 7:9, 12] = third                  # (columns 60..67: over the wave boundary 63|64)
    case(12, (92, 60))
    yy, xx = np.mgrid[0:HM, 0:HM]
    h[:, :, 13] = np.where((yy + xx) % 2 == 0, -0.0, 0.0)   # -0.0 at (0, 0); no positive value: everything compares equal
    case(13, (0, 0))
    h[:, :, 14] = -1.0
    h[30, 30, 14] = -0.25                      # every value negative (the running maximum must not start at 0)
    case(14, (243, 243))
    for j, (cy, cx) in enumerate(zip(SEAM_CELLS[1:], (7, 15, 23, 31, 39, 44)), start=15):
        h[cy, cx, j], h[cy - 1, cx, j], h[cy + 1, cx, j] = 1.0, 0.5, 0.5
        case(j, (8 * cy + 3, 8 * cx + 3))
    assert len(want) == NJ
    return m.astype(np.float32), np.array(want, np.float64)


def _bump(cy, cx, sigma=1.5):
    yy, xx = np.mgrid[0:HM, 0:HM].astype(np.float64)
    return np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma ** 2))


PINNED = 20   # border_sequence: this joint stays at the far corner (45, 45) on every frame


def border_sequence(n):
    """n map sets (1,46,46,84) float32 whose heat-map peaks jump between opposite borders: joint j's peak alternates every 3 + j % 4
    frames between a near-border cell (0 or 1 in each axis) and a far-border one (44 or 45); joint PINNED stays at the far corner.  Run
    through the OneEuro filters with irregular frame times, the filtered coordinates sweep [0, 364] fractionally and cross 3|4 and
    363|364, where the read-off's x0 / x1 change regime (tests/test_post_edges_cpu.py asserts that from the reference alone)."""
    out = []
    for k in range(n):
        m = np.zeros((1, HM, HM, 84), np.float64)
        m[0, :, :, :NJ] = (uniform01(9100 + k, HM * HM * NJ).reshape(HM, HM, NJ).astype(np.float64) - 0.5) * 0.1
        _loc_maps(m, 9200 + k)
        for j in range(NJ):
            far = j == PINNED or ((k + 2 * j) // (3 + j % 4)) % 2 == 1   # (+ 2j: some joints start at the far border)
            near_c, far_c = (j % 2, (j // 2) % 2), (45 - (j // 4) % 2, 45 - j % 2)
            cy, cx = (45, 45) if j == PINNED else (far_c if far else near_c)
            m[0, :, :, j] += _bump(cy, cx)
        out.append(m.astype(np.float32))
    return out


def sequence_times(n, t0=1.7e9):
    """the (t2d, t3d) of border_sequence's frames: irregular steps, and a t2d of 0.0 ("no timestamp", OneEuroFilter.py:65) in the middle"""
    out, t = [], t0
    for k in range(n):
        t += 1 / 30 + 0.004 * ((k * 7) % 5)
        out.append((0.0 if k == n // 2 else t, t + 0.0004))
    return out


def scale_sets():
    return [[0.99], [1.0, 0.9999], [0.995, 0.7], [0.9893], [0.7, 1.0, 0.9999], [0.8, 0.8, 0.8], [1.0, 0.95, 0.9, 0.8, 0.7],
            [0.55, 0.65, 0.75, 0.85, 0.99], [0.3, 0.35, 0.45, 0.5, 0.6, 0.66, 0.9], [1.0, 0.95, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4]]


FORCED = (0, 45, 0, 45, 1, 44, 45, 0)   # edge_maps: joint j < 8 has this cell in axis j % 2


def edge_maps(seed, S, scales=None):
    """helpers.synth_maps with the bump centres drawn over cells 0..45 inclusive, at least 8 of the 21 joints forced into cells
    {0, 1, 44, 45} in one axis, and amplitudes that differ per scale.

    scales=None: the same cell in every scale's map, as synth_maps has it.  With a scale list, scale i's bump sits where a pyramid
    puts it -- the image shrunk by s_i about the map's centre, 22.5 + (c - 22.5) * s_i, and as much narrower -- so that the MERGED map has
    its peak at the border cell whatever the scales are (the merge's centre crop drops the border cells of every scale below 1)."""
    m = np.zeros((S, HM, HM, 84), np.float64)
    m[:, :, :, :NJ] = (uniform01(seed, S * HM * HM * NJ).reshape(S, HM, HM, NJ).astype(np.float64) - 0.5) * 0.1
    _loc_maps(m, seed + 104729)
    centers = uniform01(seed + 7919, 42).reshape(NJ, 2).astype(np.float64) * 45.0
    for j in range(8):
        centers[j, j % 2] = FORCED[(j + seed) % 8]
    for j in range(NJ):
        for i in range(S):
            s = 1.0 if scales is None else float(scales[i])
            cy, cx = 22.5 + (centers[j] - 22.5) * s
            m[i, :, :, j] += (1.0 + 0.13 * i) * _bump(cy, cx, 1.5 * max(s, 0.5))
    return m.astype(np.float32)


def border_joints(raw):
    """how many joints of a raw arg-max (21,2) lie in rows or columns < 8 or >= 360"""
    raw = np.asarray(raw)
    return int(np.sum(np.any((raw < 8) | (raw >= 360), axis=1)))
