"""Case sets and CPU references for the device tracking kernels (tests/test_gpu_track_kernels.py, tests/test_gpu_track_maps.py), and the
conditions those sets must meet (tests/test_track_cases_cpu.py asserts them WITHOUT a GPU, from the references alone).

Nothing in here comes from the code under test: the references are numpy float64 (the joints' shift), runner.bbox_update and
runner.track's fallback (the box), hostplan.h's squarify behind hp_squarify_bytes (the geometry and the refusals), numpy slicing (the
crop copy) and oracle.gen_input_batch (the pyramid)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnect_amd", "csrc")
HP_SO = os.environ.get("VNECT_HOSTPLAN_SO") or os.path.join(ROOT, "vnect_amd", "lib", "libvnect_hostplan.so")
u8p, f64p, i32p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

# kernels.h: TrackState = 10 ints (x, y, w, h, uw, uh, H, W, status, fail) + FrameParams; tables.h: FrameParams = scaler (f64), offx, offy,
# H, W, then ResizeTab (dh, dw, xmax, copy, seven int16[368]).  The probe's tp_layout() and hp_frame_params_size() are held to these.
HDR_INTS, FP_BYTES = 10, 8 + 4 * 4 + 4 * 4 + 7 * 368 * 2
STATE_BYTES = 4 * HDR_INTS + FP_BYTES
SQ_OK, SQ_RANGE, SQ_SCALED, SQ_LONG = 0, 1, 2, 3
# hostplan.h's refusal texts (tests/test_track_cpu.py::test_refusal_messages_are_the_host_paths holds crop.h to them)
CODE_OF = {None: SQ_OK, "frame size out of range": SQ_RANGE, "squarify: scaled size exceeds 368": SQ_SCALED,
           "squarify: scaled long side != 368": SQ_LONG}
GARBAGE = 0xA5
BASELINE_SCALES = [1.0, 0.8, 0.6]
SIX_SCALES = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5]

_HP = None
_SQ = {}


def hostplan():
    """libvnect_hostplan.so (g++ build of hostplan.h behind hostplan_capi.cpp), built on demand."""
    global _HP
    if _HP is None:
        if "VNECT_HOSTPLAN_SO" not in os.environ:
            subprocess.check_call(["make", "-C", CSRC, "hostplan"], stdout=subprocess.DEVNULL)
        L = C.CDLL(HP_SO)
        L.hp_squarify_bytes.argtypes = [C.c_int, C.c_int, u8p, C.c_char_p, C.c_int]
        L.hp_crop_refusal.argtypes = [C.c_int]
        L.hp_crop_refusal.restype = C.c_char_p
        L.hp_to_16.argtypes = [C.POINTER(C.c_float), C.c_int64, C.c_int, C.POINTER(C.c_uint16)]
        assert L.hp_frame_params_size() == FP_BYTES
        _HP = L
    return _HP


def squarify_bytes(h, w):
    """hostplan.h: squarify(h, w) -> (the FrameParams bytes, None), or (zeros, the refusal's message)."""
    key = (int(h), int(w))
    if key not in _SQ:
        out, err = np.zeros(FP_BYTES, np.uint8), C.create_string_buffer(128)
        rc = hostplan().hp_squarify_bytes(key[0], key[1], out.ctypes.data_as(u8p), err, 128)
        if rc:
            out[:] = 0
        _SQ[key] = (out, err.value.decode() if rc else None)
    return _SQ[key]


def fp_head(fp):
    """(scaler, offx, offy, H, W, dh, dw, xmax, copy) of FrameParams bytes."""
    i = np.ascontiguousarray(fp[8:40]).view(np.int32)
    return (float(np.ascontiguousarray(fp[:8]).view(np.float64)[0]),) + tuple(int(v) for v in i)


def pack_states(hdr, fps=None):
    """(n, 10) int32 headers [+ (n, FP_BYTES) geometry] -> (n, STATE_BYTES) uint8 TrackState images."""
    hdr = np.ascontiguousarray(hdr, np.int32).reshape(-1, HDR_INTS)
    out = np.zeros((len(hdr), STATE_BYTES), np.uint8)
    out[:, :4 * HDR_INTS] = hdr.view(np.uint8).reshape(len(hdr), -1)
    if fps is not None:
        out[:, 4 * HDR_INTS:] = fps
    return out


def frame_state(H, W, rect, past=(0, 0)):
    """The TrackState a tracked frame of an (H, W) video is cropped with: rect (x, y, w, h) and hostplan.h's geometry of (h, w) -- zero
    tables and the refusal's status if squarify refuses it.  past: how far the REPORTED extent (uw, uh) runs past the crop's, as behind
    an initial rect that runs past the frame's far edges."""
    x, y, w, h = (int(v) for v in rect)
    fp, msg = squarify_bytes(h, w)
    return pack_states([[x, y, w, h, w + past[0], h + past[1], H, W, CODE_OF[msg], 0]], fp[None])[0]


# ---- crop sizes of the geometry sweep: tests/test_track_cpu.py's sets (the host build of crop.h goes through the same ones) -----------
def dense_sizes():
    """Every (h, w) up to 96 x 96, every size up to 1024 paired with the sizes around 368 and a few others, and a stride-7 grid."""
    small = range(1, 97)
    pairs = {(h, w) for h in small for w in small}
    ring = list(range(360, 377)) + [1, 2, 3, 735, 736, 737, 738, 1024]
    pairs |= {(h, w) for h in range(1, 1025) for w in ring} | {(w, h) for h in range(1, 1025) for w in ring}
    pairs |= {(h, w) for h in range(1, 1025, 7) for w in range(3, 1025, 7)}
    return sorted(pairs)


def random_sizes():
    """Random sizes up to 8192 (and past it: "frame size out of range"), skinny ones included so that refusals occur."""
    rng = np.random.default_rng(7)
    sizes = [(int(h), int(w)) for h, w in rng.integers(1, 8193, (3000, 2))]
    sizes += [(int(h), int(w)) for h, w in zip(rng.integers(1, 12, 1500), rng.integers(700, 8193, 1500))]
    sizes += [(int(w), int(h)) for h, w in zip(rng.integers(1, 12, 1500), rng.integers(700, 8193, 1500))]
    sizes += [(0, 5), (5, 0), (8193, 10), (10, 8193), (-1, 4), (8192, 8192)]
    return sizes


def sweep_cases(sizes):
    """One box-stage case per (h, w): an (h, w) frame and two joints far outside it on both sides, so that runner.bbox_update (with the
    fallback, for sizes below 1) gives exactly [0, 0, w, h] -- the box stage then builds the geometry of (h, w)."""
    n = len(sizes)
    hw = np.asarray(sizes, np.int64)
    hdr = np.zeros((n, HDR_INTS), np.int32)
    hdr[:, 2], hdr[:, 3], hdr[:, 4], hdr[:, 5] = 1, 1, 1, 1
    hdr[:, 6], hdr[:, 7] = hw[:, 0], hw[:, 1]
    j = np.zeros((n, 21, 2), np.float64)
    j[:, :, 0] = np.where(np.arange(21) % 2 == 0, -10.0, 10.0 + np.maximum(hw[:, :1], 0))
    j[:, :, 1] = np.where(np.arange(21) % 2 == 0, -10.0, 10.0 + np.maximum(hw[:, 1:], 0))
    return {"hdr": hdr, "joints": j, "xseq": np.arange(1, n + 1, dtype=np.uint32)}


# ---- box-stage cases ------------------------------------------------------------------------------------------------------------------
def _random_joint_sets(n, seed, top=8192):
    """tests/test_track_cpu.py's _box_cases with frames up to `top`: spread, clustered, negative, outside the frame, and sets whose span is
    zero on one or both axes (kind 4: rows / both; kind 5: columns)."""
    rng = np.random.default_rng(seed)
    H = rng.integers(1, top + 1, n)
    W = rng.integers(1, top + 1, n)
    kind = rng.integers(0, 6, n)
    centre = rng.uniform(-0.3, 1.3, (n, 1, 2)) * np.stack([H, W], 1)[:, None, :]
    spread = np.where(kind[:, None, None] == 0, 0.5, np.where(kind[:, None, None] == 1, 40.0, 400.0))
    j = centre + rng.normal(0, 1, (n, 21, 2)) * spread
    j = np.where(kind[:, None, None] == 3, np.round(j), j)
    j[kind == 4, :, 0] = j[kind == 4, :1, 0]
    both = (kind == 4) & (np.arange(n) % 2 == 0)
    j[both] = j[both, :1, :]
    j[kind == 5, :, 1] = j[kind == 5, :1, 1]
    return np.ascontiguousarray(j, np.float64), H, W


def _joints_for_rect(rng, rect):
    """21 joints [row, col] in frame coordinates whose runner.bbox_update is `rect` (x, y, w, h; w, h >= 1) in a frame the rect fits in: the
    joints' span is chosen so that the grown extent lands half a pixel inside [w, w + 1), the origin half a pixel inside [x, x + 1)."""
    x, y, w, h = rect
    out = np.empty((21, 2), np.float64)
    for axis, grow, o, e in ((1, 0.8, x, w), (0, 0.2, y, h)):
        span = (e + 0.5 - grow) / (1.0 + grow)
        lo = o + 0.5 + grow * (span + 1) / 2
        out[:, axis] = lo + span * rng.uniform(0, 1, 21)
        out[0, axis], out[1, axis] = lo, lo + span
    return out


def box_cases():
    """The box stage's cases: {"hdr": (n, 10) int32 TrackState headers, "joints": (n, 21, 2) f64 in CROP coordinates, "xseq": (n,) u32,
    "tag": (n,) what each was generated for}."""
    rng = np.random.default_rng(2024)
    hdr, joints, tags = [], [], []

    def add(tag, H, W, jf, crop=None, uw=None, uh=None, status=SQ_OK):
        """jf: joints in FRAME coordinates; crop: the frame's own crop (x, y, w, h), random inside the frame by default."""
        if crop is None:
            x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
            crop = (x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1)))
        x, y, w, h = crop
        hdr.append([x, y, w, h, w if uw is None else uw, h if uh is None else uh, H, W, status, 0])
        joints.append(jf - np.array([y, x], np.float64))
        tags.append(tag)

    def frame_for(rect):
        """A frame up to 8192 x 8192 that holds rect with room to spare (so the box rule's clamp does not cut it)."""
        x, y, w, h = rect
        return int(min(8192, y + h + rng.integers(0, 400))), int(min(8192, x + w + rng.integers(0, 400)))

    def target(tag, rect, **kw):
        H, W = frame_for(rect)
        add(tag, H, W, _joints_for_rect(rng, rect), **kw)

    # random joint sets in frames up to 8192 x 8192, one in twenty as the first frame behind an initial rect past the frame's far edges
    j, H, W = _random_joint_sets(20000, 11)
    for i in range(len(j)):
        add("random", int(H[i]), int(W[i]), j[i])
        if i % 20 == 0:
            hdr[-1][4 + i // 20 % 2] += int(rng.integers(1, 500))
            tags[-1] = "initial"
    # states that ARRIVE refused (the frame's own crop was refused: track_refused)
    for i in range(300):
        add("arrives_refused", int(H[i]), int(W[i]), j[i], status=(SQ_RANGE, SQ_SCALED, SQ_LONG)[i % 3])
    # the fallback: zero extent in columns, in rows, in both
    for i in range(150):
        Hf, Wf = int(rng.integers(1, 8193)), int(rng.integers(1, 8193))
        jf = rng.uniform(0, 1, (21, 2)) * [Hf, Wf]
        if i % 3 != 1:
            jf[:, 1] = jf[0, 1]
        if i % 3 != 0:
            jf[:, 0] = jf[0, 0]
        add("fallback", Hf, Wf, jf)
    # TRACKING.md's three ways to a refused next crop
    for i in range(120):   # 1: joints within a row or so of each other, more than 736 columns wide
        target("route_wide", (int(rng.integers(0, 300)), int(rng.integers(0, 2000)), int(rng.integers(737, 7800)), 1))
    for i in range(120):   # 2: within a column, more than 736 rows tall
        target("route_tall", (int(rng.integers(0, 2000)), int(rng.integers(0, 300)), 1, int(rng.integers(737, 7800))))
    for i in range(120):   # 3: an extent that the clamp to the frame's edge cuts to one pixel
        long_side = int(rng.integers(737, 4000))
        o = int(rng.integers(0, 500))
        jf = _joints_for_rect(rng, (o, o, long_side, long_side))
        if i % 2 == 0:     # the box starts in the frame's last column
            Wf, Hf = int(rng.integers(100, 8193)), o + long_side + 5
            jf[:, 1] = jf[:, 1] - jf[:, 1].min() + (Wf - 1) + 0.5 + 0.4 * (jf[:, 1].max() - jf[:, 1].min() + 1)
        else:              # ... in its last row
            Hf, Wf = int(rng.integers(100, 8193)), o + long_side + 5
            jf[:, 0] = jf[:, 0] - jf[:, 0].min() + (Hf - 1) + 0.5 + 0.1 * (jf[:, 0].max() - jf[:, 0].min() + 1)
        add("route_clamp", Hf, Wf, jf)
    # copy crops (long side exactly 368), tall and wide ones, sides above 736
    for i in range(150):
        s = int(rng.integers(1, 369))
        target("copy", (int(rng.integers(0, 900)), int(rng.integers(0, 900))) + ((368, s) if i % 2 else (s, 368)))
    for i in range(150):
        h = int(rng.integers(4, 3000))
        target("tall", (int(rng.integers(0, 900)), int(rng.integers(0, 900)), int(rng.integers(max(1, h // 300 + 1), h)), h))
    for i in range(150):
        w = int(rng.integers(4, 3000))
        target("wide", (int(rng.integers(0, 900)), int(rng.integers(0, 900)), w, int(rng.integers(max(1, w // 300 + 1), w))))
    for i in range(150):
        a = int(rng.integers(737, 6000))
        b = int(rng.integers(a // 4, a + 1))
        target("above_736", (int(rng.integers(0, 900)), int(rng.integers(0, 900))) + ((a, b) if i % 2 else (b, a)))
    # a scaled short side exactly on a half: long side 368 m, short side m (k + 1/2) -- 736 x 1 scales to 0.5 (to even: 0, refused),
    # 736 x 3 to 1.5 (2, accepted): where round-half-even and round-half-away part ways
    for m in (2, 4, 6, 8):
        for k in range(13):
            long_side, short = 368 * m, m * (2 * k + 1) // 2
            target("half", (int(rng.integers(0, 50)), int(rng.integers(0, 50)), short, long_side))
            target("half", (int(rng.integers(0, 50)), int(rng.integers(0, 50)), long_side, short))
    n = len(hdr)
    return {"hdr": np.asarray(hdr, np.int32), "joints": np.ascontiguousarray(np.stack(joints)), "tag": np.asarray(tags),
            "xseq": (np.arange(n, dtype=np.uint64) * 2654435761 % (2 ** 32 - 1)).astype(np.uint32)}


def box_reference(cases):
    """What the box stage must leave for every case: the states (fp of an untouched state: the probe's garbage), tout (rect_used + status)
    and the joints, plus what the conditions count (info)."""
    from vnect_amd import runner
    hdr, joints, xseq = cases["hdr"], cases["joints"], cases["xseq"]
    n = len(hdr)
    states = np.empty((n, STATE_BYTES), np.uint8)
    new_hdr = np.empty((n, HDR_INTS), np.int32)
    tout = np.empty((n, 5), np.int32)
    jout = np.empty_like(joints)
    info = {"fallback": np.zeros(n, bool), "raw": np.zeros((n, 4), np.int64), "status": np.zeros(n, np.int32), "msg": [None] * n}
    for i in range(n):
        x, y, w, h, uw, uh, H, W, status, _ = (int(v) for v in hdr[i])
        if status != SQ_OK:   # track_refused: joints untouched, the refusal reported, the stream kept stopped
            jout[i] = joints[i]
            tout[i] = [x, y, uw, uh, status]
            new_hdr[i] = hdr[i]
            new_hdr[i, 9] = np.uint32(int(xseq[i]) + 1).astype(np.int32)
            states[i, 4 * HDR_INTS:] = GARBAGE
            info["status"][i] = -1
            continue
        jf = joints[i].copy()
        jf[:, 0] += y
        jf[:, 1] += x
        rect = runner.bbox_update(jf, W, H)
        info["raw"][i] = rect
        if rect[2] < 1 or rect[3] < 1:
            rect = [0, 0, W, H]
            info["fallback"][i] = True
        fp, msg = squarify_bytes(rect[3], rect[2])
        code = CODE_OF[msg]
        jout[i] = jf
        tout[i] = [x, y, uw, uh, SQ_OK]
        fail = np.uint32((int(xseq[i]) + 1) & 0xFFFFFFFF).astype(np.int32) if code else 0
        new_hdr[i] = [rect[0], rect[1], rect[2], rect[3], rect[2], rect[3], H, W, code, fail]
        states[i, 4 * HDR_INTS:] = fp
        info["status"][i], info["msg"][i] = code, msg
    states[:, :4 * HDR_INTS] = new_hdr.view(np.uint8).reshape(n, -1)
    return {"states": states, "hdr": new_hdr, "tout": tout, "joints": jout, "info": info}


def box_conditions(cases, ref):
    """The counts the issue's conditions are stated in, from the reference alone."""
    hdr, new, info = cases["hdr"], ref["hdr"], ref["info"]
    live = info["status"] >= 0
    raw = info["raw"]
    heads = [fp_head(ref["states"][i, 4 * HDR_INTS:]) if live[i] and info["status"][i] == SQ_OK else None for i in range(len(hdr))]
    count = lambda f: int(sum(1 for hd in heads if hd is not None and f(hd)))   # noqa: E731  (scaler, offx, offy, H, W, dh, dw, xmax, copy)
    w, h = new[:, 2].astype(np.int64), new[:, 3].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        short_scaled = np.minimum(w, h) * (368.0 / np.maximum(w, h))
    half = live & (np.minimum(w, h) >= 1) & (short_scaled % 1.0 == 0.5)
    tag = cases["tag"]
    return {
        "cases": len(hdr),
        "fallback": int(info["fallback"].sum()),
        "fallback_w0_only": int((info["fallback"] & (raw[:, 2] == 0) & (raw[:, 3] >= 1)).sum()),
        "fallback_h0_only": int((info["fallback"] & (raw[:, 3] == 0) & (raw[:, 2] >= 1)).sum()),
        "fallback_both": int((info["fallback"] & (raw[:, 2] == 0) & (raw[:, 3] == 0)).sum()),
        "refused_scaled": int((info["status"] == SQ_SCALED).sum()),
        "refused_long": int((info["status"] == SQ_LONG).sum()),
        "refused_range": int((info["status"] == SQ_RANGE).sum()),
        "copy": count(lambda hd: hd[8] == 1),
        "tall": count(lambda hd: hd[5] > hd[6] and hd[1] > 0),
        "wide": count(lambda hd: hd[6] > hd[5] and hd[2] > 0),
        "above_736": int((live & (info["status"] == SQ_OK) & (np.maximum(w, h) > 736)).sum()),
        "half": int(half.sum()),
        "half_refused": int((half & (info["status"] == SQ_SCALED)).sum()),
        "half_accepted": int((half & (info["status"] == SQ_OK)).sum()),
        "initial": int((live & ((hdr[:, 4] != hdr[:, 2]) | (hdr[:, 5] != hdr[:, 3]))).sum()),
        "arrives_refused": int((~live).sum()),
        # TRACKING.md's three routes, told apart by what the reference computed: a refused crop one row high and uncut, one column wide
        # and uncut, and one whose one-pixel extent is what the frame's edge left of a larger one
        "route_wide": int(((info["status"] == SQ_SCALED) & (tag == "route_wide") & (h == 1) & (w > 736)).sum()),
        "route_tall": int(((info["status"] == SQ_SCALED) & (tag == "route_tall") & (w == 1) & (h > 736)).sum()),
        "route_clamp": int(((info["status"] == SQ_SCALED) & (tag == "route_clamp") & (np.minimum(w, h) == 1)
                            & ((new[:, 0] == hdr[:, 7] - 1) | (new[:, 1] == hdr[:, 6] - 1))).sum()),
    }


def long_side_refusals(top=8192):
    """Crop sizes up to `top` whose scaled LONG side is not 368 (hostplan.h's third refusal): cv_round(L * (368.0 / L)) for every long
    side L -- the short side does not enter.  Returns the list of such L."""
    L = np.arange(1, top + 1, dtype=np.float64)
    return [int(v) for v in L[np.rint(L * (368.0 / L)) != 368]]


# ---- crop copy --------------------------------------------------------------------------------------------------------------------------
def copy_workgroups(w):
    """Workgroups per row of frame_copy_track_kernel's grid that a w-pixel crop keeps busy: 252 destination dwords each."""
    return ((3 + 3 * w + 3) // 4 + 251) // 252


def copy_cases():
    """[{H, W, stride, seed, crops: [(x, y, w, h)]}]: every x mod 4 with every w mod 4 (hence every 3 w mod 4, the destination's row
    phase) at four or more rows, widths of 1, 2 and more than 6 workgroups per row up to an 8192-wide frame, 1 to 3 pixel wide crops,
    crops that end in the frame's last row and last byte, row strides that are and are not multiples of 4."""
    out = []
    for H, W, stride in ((12, 8192, 3 * 8192), (9, 701, 3 * 701), (7, 333, 1024), (6, 4099, 3 * 4099 + 1)):
        crops = []
        for xm in range(4):
            for wm in range(4):
                for base in (1, 40, 400, 2100):
                    w = base + (wm - base) % 4
                    x = 8 + xm + 4 * wm
                    if w < 1 or x + w > W:
                        continue
                    crops.append((x, (xm + wm) % 3, w, 4 + (xm ^ wm)))
                w = 5 + wm if W < 2000 else W - 64 - 4 * xm + wm - 4
                crops.append((W - w - (W - w - xm) % 4, H - 5, w, 5))            # ends in the last row
        crops += [(W - 1, H - 3, 1, 3), (W - 2, 0, 2, H), (W - 3, H - 4, 3, 4), (W - 37, H - 4, 37, 4), (0, 0, W, H), (1, 1, W - 1, H - 1)]
        crops = [c for c in crops if c[0] >= 0 and c[1] >= 0 and c[0] + c[2] <= W and c[1] + c[3] <= H]
        out.append({"H": H, "W": W, "stride": stride, "seed": 100 + H, "crops": crops})
    return out


def make_frame(H, W, stride, seed):
    """(H, W, 3) uint8 noise as a view of a buffer whose rows are `stride` bytes apart (the padding bytes are noise too)."""
    buf = np.random.default_rng(seed).integers(0, 256, (H - 1) * stride + 3 * W, dtype=np.uint8)
    return buf, np.lib.stride_tricks.as_strided(buf, (H, W, 3), (stride, 3, 1))


# ---- tracked pyramid --------------------------------------------------------------------------------------------------------------------
def pyramid_cases():
    """[{H, W, seed, crops}]: crops at odd origins in frames of 640 x 480, 1920 x 1080, 1080 x 1920 and 4096 x 2160 -- wide, tall, copy
    (long side 368), 1 to 3 pixels wide or high, the whole frame, a crop that ends in the frame's last byte, and refused crops (zero
    tables: the pyramid reads nothing and writes the black canvas)."""
    return [
        {"H": 480, "W": 640, "seed": 1, "crops": [
            (101, 33, 500, 300), (77, 5, 200, 470), (51, 21, 368, 250), (13, 7, 300, 368), (201, 101, 368, 368), (333, 3, 1, 300),
            (7, 9, 2, 450), (9, 11, 300, 1), (5, 3, 3, 470), (0, 0, 640, 480), (637, 111, 3, 369), (271, 111, 369, 369)]},
        {"H": 1080, "W": 1920, "seed": 2, "crops": [
            (301, 101, 1500, 700), (1001, 3, 400, 1075), (1501, 701, 368, 368), (3, 5, 368, 100), (0, 0, 1920, 1080), (1917, 301, 3, 736),
            (11, 13, 1, 500), (1919, 1, 1, 736), (46, 1079, 1565, 1), (1183, 343, 737, 737), (5, 1077, 700, 3)]},
        {"H": 1920, "W": 1080, "seed": 3, "crops": [
            (301, 101, 700, 1700), (702, 100, 300, 1500), (0, 0, 1080, 1920), (5, 7, 150, 368), (1077, 1183, 3, 737), (9, 1, 1000, 1900),
            (77, 1919, 600, 1), (1079, 3, 1, 368), (711, 1551, 369, 369)]},
        {"H": 2160, "W": 4096, "seed": 4, "crops": [
            (0, 0, 4096, 2160), (1001, 501, 3000, 1500), (3001, 1, 1000, 2159), (3727, 1791, 368, 368), (3728, 1792, 368, 368),
            (4093, 1423, 3, 737), (1, 2157, 2208, 3), (2047, 1079, 2049, 1081)]},
    ]


def pyramid_reference(crop_pixels, scales):
    """oracle.gen_input_batch of the crop as the batch tensor the kernel writes: (S, 368, 368, 4) float32, channel 3 zero.  A crop that
    squarify refuses: the black canvas, (float32)0 / 255 - 0.4 in every colour."""
    import oracle
    h, w = crop_pixels.shape[:2]
    out = np.zeros((len(scales), 368, 368, 4), np.float32)
    if squarify_bytes(h, w)[1] is None:
        out[..., :3] = oracle.gen_input_batch(np.ascontiguousarray(crop_pixels), scales)[0]
    else:
        out[..., :3] = np.float32(0.0) / np.float32(255.0) - np.float32(0.4)
    return out


def to_16(a, f16):
    """float32 -> bf16 / fp16 bits, round to nearest even (hostplan.h: to_16, what the runtime converts weights with)."""
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty(a.shape, np.uint16)
    hostplan().hp_to_16(a.ctypes.data_as(C.POINTER(C.c_float)), a.size, int(f16), out.ctypes.data_as(C.POINTER(C.c_uint16)))
    return out


# ---- the tracked post-processing on chosen maps (tests/test_gpu_track_maps.py) -----------------------------------------------------------
_GEO = {}


def crop_geometry(h, w, scales):
    """(scaler, offx, offy) of an (h, w) crop as oracle.gen_input_batch gives them, or None if it refuses the crop."""
    import oracle
    key = (int(h), int(w))
    if key not in _GEO:
        try:
            _, scaler, (ox, oy) = oracle.gen_input_batch(np.zeros((key[0], key[1], 3), np.uint8), scales[:1])
            _GEO[key] = (scaler, ox, oy)
        except ValueError:
            _GEO[key] = None
    return _GEO[key]


def hot_maps(S, cells, rng=None, level=1.0):
    """(S, 46, 46, 84) maps: heat-map channel j (0 .. 20) `level` at cell cells[j] = (row, col) in every scale; with rng, small noise
    below it everywhere and random location maps (channels 21 .. 83)."""
    m = np.zeros((S, 46, 46, 84), np.float32)
    if rng is not None:
        m[..., :21] = rng.uniform(0, 0.05, (S, 46, 46, 21))
        m[..., 21:] = rng.uniform(-1, 1, (S, 46, 46, 63))
    for j, (r, c) in enumerate(cells):
        m[:, r, c, j] = level
    return m


REFUSAL = {"H": 1920, "W": 1080, "rect": [702, 100, 300, 1500], "scales": BASELINE_SCALES,
           "cells": [(2 + 40 * (j % 2), 30 + (j % 3 == 0)) for j in range(21)], "next": [1079, 46, 1, 1565]}


def cpu_loop(H, W, rect, maps_list, times, scales, est=None):
    """runner.track's loop on given maps: oracle post-processing with the crop's geometry from oracle.gen_input_batch, the shift,
    runner.bbox_update, the fallback.  Yields (joints_2d, joints_3d, rect_used, next rect) per frame; stops with (None, None, rect_used,
    None) at a crop the squarify step refuses (the filters do not see that frame).  est: an oracle.OracleEstimator to go on with."""
    import oracle
    from vnect_amd import runner
    est = est if est is not None else oracle.OracleEstimator(scales=scales, net=None)
    rect = [0, 0, W, H] if rect is None else [int(v) for v in rect]
    out = []
    for maps, (t2d, t3d) in zip(maps_list, times):
        x, y, w, h = rect
        if w < 1 or h < 1:
            x, y, w, h = rect = [0, 0, W, H]
        ch, cw = min(h, H - y), min(w, W - x)
        # (the host path's refusal is hostplan.h's squarify; the oracle's resize does not refuse a side that scales to zero pixels)
        geo = crop_geometry(ch, cw, scales) if squarify_bytes(ch, cw)[1] is None else None
        if geo is None:
            out.append((None, None, [x, y, w, h], None))
            break
        j2, j3 = est.postprocess(maps, t2d, t3d, geo[0], geo[1], geo[2])
        j2[:, 0] += y
        j2[:, 1] += x
        rect = runner.bbox_update(j2, W, H)
        out.append((j2, j3, [x, y, w, h], list(rect)))
    return out


# 64-frame random walks: per frame the 21 heat-map maxima are a random cluster of cells of the 46 x 46 maps, padding bands included, so the
# joints un-map to points outside the crop, outside the frame and below zero; one frame in twelve or so has all maxima on ONE cell (a
# degenerate box: the fallback to the whole frame).  (H, W) -> seed, chosen so that the CPU loop alone meets the conditions
# tests/test_track_cases_cpu.py asserts and meets no refused crop (the refusal has its own test).
WALKS = {(480, 640): 1, (1080, 1920): 2, (1920, 1080): 3, (2160, 4096): 4}
WALK_FRAMES = 64
T0 = 1.7e9


def walk_cells(seed, n=WALK_FRAMES):
    """(n, 21, 2) cells (row, col) and (n,) noise seeds of a walk's maps."""
    rng = np.random.default_rng(seed)
    cells = np.empty((n, 21, 2), np.int64)
    for k in range(n):
        centre = rng.uniform(0, 45, 2)
        spread = rng.uniform(0.3, 14, 2)
        c = np.clip(np.rint(centre + rng.normal(0, 1, (21, 2)) * spread), 0, 45)
        if rng.uniform() < 0.08:
            c[:] = c[0]
        cells[k] = c
    return cells, np.arange(n, dtype=np.int64) + 1000 * seed


def walk_times(n=WALK_FRAMES, base=0.0):
    return [(T0 + base + 0.033 * k + 0.002 * (k % 3), T0 + base + 0.033 * k + 0.0005) for k in range(n)]


def walk_reference(H, W, seed, scales=BASELINE_SCALES, n=WALK_FRAMES):
    cells, seeds = walk_cells(seed, n)
    maps = (hot_maps(len(scales), [tuple(c) for c in cells[k]], np.random.default_rng(int(seeds[k]))) for k in range(n))
    return cpu_loop(H, W, None, maps, walk_times(n), scales)


def state_after(H, W, nxt, xseq):
    """The TrackState bytes behind a frame whose box rule gave `nxt` (before the fallback); xseq: that frame's number (the first is 1)."""
    x, y, w, h = nxt
    if w < 1 or h < 1:
        x, y, w, h = 0, 0, W, H
    fp, msg = squarify_bytes(h, w)
    return pack_states([[x, y, w, h, w, h, H, W, CODE_OF[msg], xseq + 1 if msg else 0]], fp[None])[0]
