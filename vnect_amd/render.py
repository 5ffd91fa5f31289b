"""Headless rendering of the results to image files (SURVEY 8 f-row 4; the reference: src/utils.py:222-330).

``draw_limbs_2d`` has the reference's signature and conventions (joints are [row, col]; limbs join joint i to
``limb_parents[i]``; the crop rectangle is outlined; colours are the reference's BGR triples) but draws with PIL, not
cv2: a limb is a 6-pixel-wide line instead of a filled 3-pixel half-axis ellipse, so pictures look alike without being
pixel-identical (there is no GUI here: results go to files).  ``draw_limbs_3d`` projects the skeleton orthographically
the way the reference's matplotlib view (elev -90, azim -90: x right, y down) shows it.
"""
import numpy as np

LIMB_BGR = (49, 22, 122)   # src/utils.py:238
RECT_BGR = (60, 66, 207)   # src/utils.py:243


def _canvas(img):
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(img[:, :, ::-1]))  # BGR -> RGB


def _back(pil):
    return np.ascontiguousarray(np.asarray(pil)[:, :, ::-1])


def draw_limbs_2d(img, joints_2d, limb_parents, rect):
    """Return a copy of the uint8 BGR frame with the skeleton and the crop rectangle drawn (src/utils.py:222-244)."""
    from PIL import ImageDraw
    pil = _canvas(img)
    d = ImageDraw.Draw(pil)
    for i, parent in enumerate(limb_parents):
        r1, c1 = joints_2d[i]
        r2, c2 = joints_2d[parent]
        d.line([(float(c1), float(r1)), (float(c2), float(r2))], fill=LIMB_BGR[::-1], width=6)
    x, y, w, h = rect
    d.rectangle([x, y, x + w, y + h], outline=RECT_BGR[::-1], width=4)
    return _back(pil)


def _limb_half_axis(L2):
    """The largest integer a >= 0 with 4 a^2 <= L2: int(length / 2) of src/utils.py:233, independent of how sqrt rounds."""
    a = np.floor(np.sqrt(L2) * 0.5)
    if 4.0 * a * a > L2:
        a -= 1.0
    if 4.0 * (a + 1.0) * (a + 1.0) <= L2:
        a += 1.0
    return a


def draw_limbs_2d_exact(img, joints_2d, limb_parents, rect, pixel_format="bgr", confidence=None, min_confidence=None, colors=None,
                        inplace=False):
    """``draw_limbs_2d`` by the exact rule the device draws with (OVERLAY.md; vnect_amd/csrc/overlay.h): pixel-identical to
    ``VNectEstimator.draw`` and to the frames ``track_on_device(..., draw=True)`` leaves.  A limb is the ellipse of half-axes
    (a, 3) along it (src/utils.py:232-235) tested per pixel in float64 -- no angle, hence no rounding of it to whole degrees as in
    cv2.ellipse2Poly: alike, not identical, to the reference's picture -- and the rectangle is a band of thickness 4 (:241), drawn over
    the limbs.  ``img``: a uint8 (H, W, 3) host array, any strides; ``pixel_format`` "bgr" or "rgb"; ``rect`` (x, y, w, h) or None;
    ``min_confidence`` with ``confidence`` (21,): limbs with an end below it are left out; ``colors``: (limb_bgr, rect_bgr), either None
    for the reference's.  Returns an annotated copy, or with ``inplace=True`` draws into ``img`` itself and returns it."""
    if pixel_format not in ("bgr", "rgb"):
        raise ValueError("pixel_format must be 'bgr' or 'rgb'")
    out = img if inplace else np.array(img, copy=True)
    if out.dtype != np.uint8 or out.ndim != 3 or out.shape[2] != 3:
        raise ValueError("frame must be a uint8 (H, W, 3) array")
    H, W = out.shape[:2]
    limb, box = (None, None) if colors is None else colors
    limb = tuple(int(v) for v in (LIMB_BGR if limb is None else limb))
    box = tuple(int(v) for v in (RECT_BGR if box is None else box))
    if pixel_format == "rgb":
        limb, box = limb[::-1], box[::-1]
    j = np.asarray(joints_2d, np.float64)
    thr = None if (min_confidence is None or confidence is None or np.isnan(min_confidence)) else float(min_confidence)
    with np.errstate(all="ignore"):
        for i, parent in enumerate(limb_parents):
            parent = int(parent)
            if not 0 <= parent < len(j):
                raise ValueError("a parent must be a joint")
            r1, c1, r2, c2 = (float(v) for v in (j[i, 0], j[i, 1], j[parent, 0], j[parent, 1]))
            if not all(abs(v) <= 2.0 ** 20 for v in (r1, c1, r2, c2)):   # (NaN and +-inf fail the comparison)
                continue
            if thr is not None and (confidence[i] < thr or confidence[parent] < thr):
                continue
            dr, dc = np.float64(r1 - r2), np.float64(c1 - c2)
            L2 = dr * dr + dc * dc
            a = _limb_half_axis(L2)
            if a < 1.0:
                continue
            cr, cc = float(np.rint((r1 + r2) * 0.5)), float(np.rint((c1 + c2) * 0.5))
            m = max(a, 3.0)                                               # no pixel further than this from the centre can be inside
            ya, yb = int(max(0.0, cr - m)), int(min(H - 1.0, cr + m))
            xa, xb = int(max(0.0, cc - m)), int(min(W - 1.0, cc + m))
            if yb < ya or xb < xa:
                continue
            u = (np.arange(ya, yb + 1, dtype=np.float64) - cr)[:, None]
            v = (np.arange(xa, xb + 1, dtype=np.float64) - cc)[None, :]
            s_, t_ = u * dr + v * dc, u * dc - v * dr
            aa = a * a
            inside = (s_ * s_) * 9.0 + (t_ * t_) * aa <= (aa * 9.0) * L2
            out[ya:yb + 1, xa:xb + 1][inside] = limb
    if rect is not None:
        x0, y0, w, h = (int(v) for v in rect)
        if w < 1 or h < 1:
            raise ValueError("the rect must be at least one pixel wide and high")
        ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
        outer = (xs >= x0 - 2) & (xs <= x0 + w + 1) & (ys >= y0 - 2) & (ys <= y0 + h + 1)
        inner = (xs >= x0 + 2) & (xs <= x0 + w - 3) & (ys >= y0 + 2) & (ys <= y0 + h - 3)
        out[outer & ~inner] = box
    return out


PREVIEW_MAX = 4096   # an output side at most (include/vnect_abi.h: VNECT_PREVIEW_MAX)


def _preview_geom(H, W, factor=None):
    """(rows, columns, the factor used) of an (H, W) picture scaled by ``factor`` as cv2.resize(.., (0, 0), fx=f, fy=f) sizes it: cv_round(H f),
    cv_round(W f), half to even.  ``factor`` None or 0: the reference's 1024.0 / max(W, H) (run_estimator_ps.py:95).  Raises ValueError
    for what the device refuses: a negative or non-finite factor, a side that rounds to 0 or exceeds PREVIEW_MAX."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("the picture must be at least one pixel wide and high")
    f = 0.0 if factor is None else float(factor)
    if not (0.0 <= f <= 1.7e308):
        raise ValueError("the factor must be finite and not negative")
    if f == 0.0:
        f = 1024.0 / float(max(W, H))
    dhf, dwf = H * f, W * f
    if not (dhf < 1e6 and dwf < 1e6):
        raise ValueError("an output side exceeds %d" % PREVIEW_MAX)
    dh, dw = int(np.rint(dhf)), int(np.rint(dwf))
    if dh < 1 or dw < 1:
        raise ValueError("an output side rounds to 0")
    if dh > PREVIEW_MAX or dw > PREVIEW_MAX:
        raise ValueError("an output side exceeds %d" % PREVIEW_MAX)
    return dh, dw, f


def _resize_axis(dsize, ssize, scale, x_axis):
    """cv2's per-axis INTER_LINEAR table (vnect_amd/csrc/axis.h): taps s0, s1, the 11-bit coefficients and the x axis's edge flag."""
    fx = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(fx)
    fr = (fx - fl).astype(np.float32)
    s = fl.astype(np.int64)
    if x_axis:
        fr = np.where(s < 0, np.float32(0), fr)
        s = np.maximum(s, 0)
        edge = s + 1 >= ssize
        fr = np.where(s >= ssize - 1, np.float32(0), fr).astype(np.float32)
        s0 = np.minimum(s, ssize - 1)
        s1 = np.minimum(s0 + 1, ssize - 1)
    else:
        edge = np.zeros(dsize, bool)
        s0, s1 = np.clip(s, 0, ssize - 1), np.clip(s + 1, 0, ssize - 1)
    c0 = np.clip(np.rint((np.float32(1) - fr) * np.float32(2048)), -32768, 32767).astype(np.int64)
    c1 = np.clip(np.rint(fr * np.float32(2048)), -32768, 32767).astype(np.int64)
    return s0, s1, c0, c1, edge


def resize_u8_exact(img, f):
    """cv2.resize(img, (0, 0), fx=f, fy=f, interpolation=cv2.INTER_LINEAR) of a uint8 (H, W) or (H, W, C) array in the 8-bit path's own
    11-bit fixed point (PREVIEW.md; vnect_amd/csrc/preview.h), in numpy: the arithmetic the pyramid and the preview kernel use on the
    device.  Equal sizes in both axes are a copy."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("resize_u8_exact takes a uint8 (H, W) or (H, W, C) array")
    H, W = img.shape[:2]
    dh, dw, f = _preview_geom(H, W, f)
    if dh == H and dw == W:
        return np.array(img, copy=True)
    scale = 1.0 / f
    x0, x1, a0, a1, edge = _resize_axis(dw, W, scale, True)
    y0, y1, b0, b1, _ = _resize_axis(dh, H, scale, False)
    src = img.astype(np.int64).reshape(H, W, -1)
    a0, a1, edge = a0[None, :, None], a1[None, :, None], edge[None, :, None]

    def row(y):
        top = src[y]
        return np.where(edge, top[:, x0] * 2048, top[:, x0] * a0 + top[:, x1] * a1)

    r0, r1 = row(y0), row(y1)
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8).reshape((dh, dw) + img.shape[2:])


def preview_exact(img, joints_2d, parents, rect, factor=None, out_format="bgr", confidence=None, min_confidence=None, colors=None):
    """The reference's display picture (run_estimator_ps.py:94-96: ``draw_limbs_2d`` into a copy, then ``img_scale`` to 1024 on the
    longer side) by the exact rule the device computes it with (PREVIEW.md): pixel-identical to ``VNectEstimator.preview``.  ``img``: the
    uint8 (H, W, 3) BGR picture as it is looked at (an oriented frame: turned first); ``joints_2d`` None: no limbs; ``rect`` None: no
    rectangle; ``factor`` None: 1024 / the longer side; ``out_format`` "bgr" or "rgb".  The other arguments are
    ``draw_limbs_2d_exact``'s.  Returns a fresh (dh, dw, 3) array; ``img`` is not changed."""
    if out_format not in ("bgr", "rgb"):
        raise ValueError("out_format must be 'bgr' or 'rgb'")
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("frame must be a uint8 (H, W, 3) array")
    _preview_geom(img.shape[0], img.shape[1], factor)
    if joints_2d is None and rect is None:
        a = img
    else:
        j = np.full((21, 2), np.nan) if joints_2d is None else joints_2d
        a = draw_limbs_2d_exact(img, j, parents, rect, confidence=confidence, min_confidence=min_confidence, colors=colors)
    out = resize_u8_exact(a, factor)
    return np.ascontiguousarray(out[:, :, ::-1]) if out_format == "rgb" else out


def draw_limbs_3d(joints_3d, joint_parents, size=400, extent=500.0):
    """Orthographic front view of the 21x3 joints in mm (the reference's plot limits are +-500): uint8 BGR (size, size, 3)."""
    from PIL import Image, ImageDraw
    pil = Image.new("RGB", (size, size), (255, 255, 255))
    d = ImageDraw.Draw(pil)
    j = np.asarray(joints_3d, np.float64)
    px = (j[:, 0] + extent) / (2 * extent) * (size - 1)
    py = (j[:, 1] + extent) / (2 * extent) * (size - 1)
    for i, parent in enumerate(joint_parents):
        d.line([(px[i], py[i]), (px[parent], py[parent])], fill=(30, 30, 30), width=2)
    for i in range(len(j)):
        d.ellipse([px[i] - 3, py[i] - 3, px[i] + 3, py[i] + 3], fill=LIMB_BGR[::-1])
    return _back(pil)


def save(path, img_bgr):
    """cv2.imwrite replacement (PNG / JPEG by extension)."""
    _canvas(img_bgr).save(path)


# matplotlib's colour cycle (rcParams['axes.prop_cycle']: "tab10") as RGB; limb i of the 3-D view takes entry i % 10
VIEW3D_CYCLE_RGB = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
                    (127, 127, 127), (188, 189, 34), (23, 190, 207))
JOINT_PARENTS = (16, 15, 1, 2, 3, 1, 5, 6, 14, 8, 9, 14, 11, 12, 14, 14, 1, 4, 7, 10, 13)   # src/estimator.py joint_parents


def _trig_deg(deg):
    """(cos, sin) of an angle in degrees, exact at the multiples of 90."""
    q = float(deg) % 360.0
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    if q in exact:
        return exact[q]
    return float(np.cos(np.deg2rad(deg))), float(np.sin(np.deg2rad(deg)))


def view_matrix(elev, azim):
    """The 3 x 3 view of ``view3d`` / ``view3d_exact`` for mplot3d's ``view_init(elev, azim)`` (degrees, no roll, |elev| <= 90): row 0
    is the screen's right, row 1 its DOWN, row 2 the direction away from the camera -- mplot3d's view axes u, -v, -w for the eye at
    (cos e cos a, cos e sin a, sin e).  ``view_matrix(-90, -90)`` is the identity, the reference's view (src/utils.py:280)."""
    ce, se = _trig_deg(elev)
    ca, sa = _trig_deg(azim)
    return np.array([[-sa, ca, 0.0], [se * ca, se * sa, -ce], [-ce * ca, -ce * sa, -se]], dtype=np.float64) + 0.0


def view3d_exact(joints_3d, size=400, view=None, extent=500.0, line_width=3.0, background=None, colors=None, parents=None, confidence=None,
                 min_confidence=None, out_format="bgr", order=0, out=None):
    """The 3-D skeleton view by the exact rule the device renders with (VIEW3D.md; vnect_amd/csrc/view3d.h): pixel-identical to
    ``VNectEstimator.view3d`` and to the views ``track_on_device(..., view3d=True)`` yields.  The reference's picture is matplotlib's
    (src/utils.py:272-304); this is its shapes by this project's rule -- orthographic, round caps, no anti-aliasing, no axes.
    ``joints_3d``: (21, 3) [x, y, z] in mm; the other arguments are ``_native.view3d_spec``'s.  Returns a fresh (rows, cols, 3) uint8 array, or
    fills ``out`` (a uint8 (rows, cols, 3) host array with unit channel stride and 3-byte pixel stride) and returns it."""
    if out_format not in ("bgr", "rgb"):
        raise ValueError("out_format must be 'bgr' or 'rgb'")
    rows, cols = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    extent, w = float(extent), float(line_width)
    if not (1 <= rows <= 2048 and 1 <= cols <= 2048):
        raise ValueError("rows and cols must lie in 1 .. 2048")
    if not (np.isfinite(extent) and extent > 0.0) or not (0.0 < w <= 64.0) or order not in (0, 1):
        raise ValueError("extent must be finite and positive, line_width in (0, 64], order 0 or 1")
    R = np.eye(3) if view is None else np.asarray(view, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError("view must be a finite 3 x 3 matrix")
    par = [int(p) for p in (JOINT_PARENTS if parents is None else parents)]
    if len(par) != 21 or min(par) < 0 or max(par) > 20:
        raise ValueError("parents must name one joint, 0 .. 20, for each of the 21 joints")
    col = np.array([c[::-1] for c in VIEW3D_CYCLE_RGB] * 3)[:21] if colors is None else np.asarray(colors)
    bg = np.array((255, 255, 255) if background is None else background)
    if col.shape != (21, 3) or col.min() < 0 or col.max() > 255 or bg.shape != (3,) or bg.min() < 0 or bg.max() > 255:
        raise ValueError("21 BGR colours and a BGR background, components 0 .. 255")
    if out_format == "rgb":
        col, bg = col[:, ::-1], bg[::-1]
    j = np.asarray(joints_3d, dtype=np.float32).astype(np.float64)
    if j.shape != (21, 3):
        raise ValueError("joints_3d must be (21, 3)")
    k = np.float64(min(rows, cols) - 1) / (2.0 * extent)
    cx, cy = np.float64(cols - 1) * 0.5, np.float64(rows - 1) * 0.5
    r2 = (w * 0.5) * (w * 0.5)
    with np.errstate(all="ignore"):
        x, y, z = j[:, 0], j[:, 1], j[:, 2]
        u = (R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z
        v = (R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z
        d = (R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z
        pc, pr = cx + u * k, cy + v * k
    ok = np.isfinite(pc) & np.isfinite(pr) & (np.abs(pc) <= 2.0 ** 20) & (np.abs(pr) <= 2.0 ** 20)
    low = np.zeros(21, bool)
    if min_confidence is not None and confidence is not None and not np.isnan(min_confidence):
        low = np.asarray(confidence, dtype=np.float64) < float(min_confidence)
    best = np.full((rows, cols), -1, np.int64)        # the limb on top so far
    bkey = np.zeros((rows, cols), np.float64)
    Y, X = np.mgrid[0:rows, 0:cols].astype(np.float64)
    for i in range(21):
        p = par[i]
        if p == i or not (ok[i] and ok[p]) or low[i] or low[p] or (order == 1 and not (np.isfinite(d[i]) and np.isfinite(d[p]))):
            continue
        ex, ey = pc[p] - pc[i], pr[p] - pr[i]
        L2 = ex * ex + ey * ey
        wx, wy = X - pc[i], Y - pr[i]
        t = wx * ex + wy * ey
        qx, qy = X - pc[p], Y - pr[p]
        c = wx * ey - wy * ex
        inside = np.where(t <= 0.0, wx * wx + wy * wy <= r2, np.where(t >= L2, qx * qx + qy * qy <= r2, c * c <= r2 * L2))
        key = d[i] + d[p] if order == 1 else 0.0
        # limb i lies over what is there: order 0 -- always (a higher index); order 1 -- a smaller key, or an equal one (a higher index)
        over = inside & ((best < 0) | (key <= bkey))
        best[over], bkey[over] = i, key
    pic = np.where((best >= 0)[:, :, None], col[np.maximum(best, 0)], bg[None, None, :]).astype(np.uint8)
    if out is None:
        return pic
    if out.dtype != np.uint8 or out.shape != (rows, cols, 3) or out.strides[2] != 1 or out.strides[1] != 3:
        raise ValueError("out must be a uint8 (%d, %d, 3) array with unit channel stride and 3-byte pixel stride" % (rows, cols))
    out[...] = pic
    return out
