"""Headless counterparts of the reference's runner scripts (SURVEY 8 f-row 1, BASELINE.json configs[0]).

* ``run_pic``   -- the flow of ``run_pic.py:18-30`` without cv2 / HOG / GUI: decode the picture, take the
  full-frame rectangle (the reference's no-detection fallback, ``src/hog_box.py:28-29``), estimate, shift the
  2-D joints back by the crop origin.
* ``track``     -- the frame loop of ``run_estimator_ps.py:80-109``: crop -> estimator -> bounding-box update from
  the joints, for any iterable of frames (synthetic streams on the GPU box; there is no camera / ffmpeg).
* ``init_box``  -- the person-box initialiser: the reference's HOG detector (``src/hog_box.py``) replaced by one pass of
  the network over the whole frame and the loop's own box arithmetic.
* ``hog_box``   -- the reference's initialiser itself (``src/hog_box.py:26-31``): the HOG people detector on the device (HOG.md), the
  largest detection through ``cal_rect``; ``track(lost=(c, n, "detect"))`` calls it for the frame behind a lost one.
The capture, drawing and 3-D plotting of the reference stay out of scope.
"""
from collections import deque
from operator import itemgetter

import numpy as np

from . import _native


def load_bgr(path):
    """cv2.imread replacement: uint8 BGR (H, W, 3) via PIL (cv2 is not available on either box)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def full_frame_rect(img):
    """HOGBox's fallback rectangle when no person is detected (src/hog_box.py:28-29): (x, y, w, h)."""
    h, w = img.shape[:2]
    return [0, 0, w, h]


def run_pic(estimator, img, rect=None, timestamp=None):
    """run_pic.py:18-30: returns (joints_2d in full-image [row, col], joints_3d, rect)."""
    x, y, w, h = rect if rect is not None else full_frame_rect(img)
    img_cropped = img[y: y + h, x: x + w, :]
    joints_2d, joints_3d = estimator(img_cropped, timestamp=timestamp)
    joints_2d[:, 0] += y
    joints_2d[:, 1] += x
    return joints_2d, joints_3d, [x, y, w, h]


def bbox_update(joints_2d, W_img, H_img):
    """The tracking loop's next crop rectangle (x, y, w, h) from the 2-D joints in frame coordinates -- the rule of
    run_estimator_ps.py:96-107: the joints' bounding box grown by 80 % of (its width + 1) and 20 % of (its height + 1), half of the
    margin before the box, the whole margin added to its extent, clamped to the frame; integer truncation as there."""
    lo = joints_2d.min(axis=0)                 # [row, col] = [y, x]
    span = joints_2d.max(axis=0) - lo
    rect = {}
    for axis, grow, limit in ((1, 0.8, W_img), (0, 0.2, H_img)):
        margin = grow * (span[axis] + 1)
        origin = max(int(lo[axis] - margin / 2), 0)
        rect[axis] = (origin, int(min(span[axis] + margin, limit - origin)))
    (x, w), (y, h) = rect[1], rect[0]
    return [x, y, w, h]


def lost_rule(lost, detect=False):
    """``lost=(min_confidence, min_joints, "hold" | "reset")`` of the tracking loops as (threshold, count, action) -- or None.  The rule
    (CONFIDENCE.md): a frame is lost when fewer than ``min_joints`` of its 21 confidences are >= ``min_confidence``.  ``detect``: the
    host loop's third action, "detect" (HOG.md), is allowed too."""
    if lost is None:
        return None
    min_confidence, min_joints, action = lost
    min_confidence, min_joints = float(min_confidence), int(min_joints)
    if action == "detect" and not detect:
        raise ValueError("lost=(min_confidence, min_joints, 'detect') runs the person detector on the host's side of the loop: "
                         "use runner.track (the device loops take 'hold' or 'reset')")
    if action not in ("hold", "reset") + (("detect",) if detect else ()):
        raise ValueError("lost=(min_confidence, min_joints, action): action must be 'hold' or 'reset'")
    if not 1 <= min_joints <= 21:
        raise ValueError("lost=(min_confidence, min_joints, action): min_joints must be 1 .. 21")
    if min_confidence != min_confidence:
        raise ValueError("lost=(min_confidence, min_joints, action): min_confidence is NaN")
    return min_confidence, min_joints, action


def is_lost(confidence, min_confidence, min_joints):
    """The loss rule on the host: fewer than min_joints confidences reach min_confidence (NaN and -inf never do)."""
    return int(np.count_nonzero(np.asarray(confidence) >= min_confidence)) < min_joints


def init_box(estimator, frame, timestamp=None, min_confidence=None, min_joints=1):
    """Person-box initialiser without cv2's HOG detector (SURVEY 8 f-row 3; the reference: src/hog_box.py:25-58).

    The reference asks a HOG people detector for a rectangle and falls back to the whole frame when it finds nobody
    (hog_box.py:28-29).  Here the network itself proposes the box: one pass over the whole frame (that fallback
    rectangle), then the tracking loop's own box arithmetic on the joints it found (run_estimator_ps.py:96-107).  The
    pass is a probe: the estimator's filters are reset afterwards, so the first tracked frame is still an unfiltered one
    as in the reference.  Returns (x, y, w, h).  ``min_confidence`` (additive; CONFIDENCE.md): when the probe pass is "lost" -- fewer
    than ``min_joints`` confidences reach it: nobody is there to box -- the whole frame.
    """
    H_img, W_img = frame.shape[:2]
    if min_confidence is None:
        joints_2d, _ = estimator(frame, timestamp=timestamp)
        estimator.reset()
    else:
        joints_2d, _, conf = estimator(frame, timestamp=timestamp, return_confidence=True)
        estimator.reset()
        if is_lost(conf, *lost_rule((min_confidence, min_joints, "reset"))[:2]):
            return [0, 0, W_img, H_img]
    x, y, w, h = bbox_update(joints_2d, W_img, H_img)
    if w < 1 or h < 1:
        return [0, 0, W_img, H_img]
    return [x, y, w, h]


def cal_rect(rect, H, W):
    """HOGBox.cal_rect (src/hog_box.py:48-58), term by term: the detection (x, y, w, h) grown by 40 % of the frame's width and 20 % of
    its height -- half of each on either side, ``int()`` truncation as there -- and clamped to the (H, W) frame."""
    x, y, w, h = (int(v) for v in rect)
    offset_w = int(0.4 / 2 * W)                      # hog_box.py:53
    offset_h = int(0.2 / 2 * H)                      # hog_box.py:54
    x0, y0 = max(x - offset_w, 0), max(y - offset_h, 0)
    return [x0, y0, min(x + w + offset_w, W) - x0, min(y + h + offset_h, H) - y0]


def hog_box(estimator, frame, pixel_format="bgr", orientation=None, stream=None, **spec):
    """``HOGBox.__call__`` without its window (src/hog_box.py:26-31): the person detector over the frame
    (``estimator.detect_people``; HOG.md), the detection of the largest area -- the first of equals, as ``np.argmax`` picks it --
    through ``cal_rect``; the whole frame when nobody is found.  Returns [x, y, w, h] in the oriented picture's coordinates."""
    rects, _ = estimator.detect_people(frame, pixel_format=pixel_format, orientation=orientation, stream=stream, **spec)
    if _native.is_device_array(frame):
        f = _native.device_frame(frame, pixel_format)
        H, W = int(f.H), int(f.W)
    else:
        H, W = frame.shape[:2]
    if (estimator.orientation if orientation is None else orientation) & 1:
        H, W = W, H
    if not len(rects):
        return [0, 0, W, H]
    return cal_rect(rects[int(np.argmax(rects[:, 2].astype(np.int64) * rects[:, 3]))], H, W)


def orient_view(frame, orientation):
    """The oriented picture of a stored frame as a numpy view (ORIENTATION.md): np.rot90 by ``orientation & 3``, mirrored when
    ``orientation & 4``.  3 is the reference's ``T`` (run_estimator_ps.py:57-62, 81-85), 7 its commented np.transpose variant."""
    g = np.rot90(frame, orientation & 3)
    return g[:, ::-1] if orientation & 4 else g


def _orientations(estimator, orientation, n, transpose):
    """one code 0 .. 7 per video, from one code or a sequence of n -- None: the estimator's own (``VNectEstimator(orientation=)``; an
    estimator without one: 0); not together with transpose"""
    if orientation is None:
        orientation = getattr(estimator, "orientation", 0)
    codes = [orientation] * n if isinstance(orientation, (int, np.integer)) and not isinstance(orientation, bool) else list(orientation)
    if len(codes) != n or any(isinstance(o, bool) or not isinstance(o, (int, np.integer)) or not 0 <= int(o) <= 7 for o in codes):
        raise ValueError("orientation must be a code 0 .. 7 (or one per video): np.rot90 by code & 3, mirrored when code & 4")
    if transpose and any(codes):
        raise ValueError("transpose=True is orientation=3: pass one of the two, not transpose together with a non-zero orientation")
    return [int(o) for o in codes]


def _nv12_checks(pixel_format, transpose, source=None):
    if source == "device":  # frames in device memory (DEVICE_FRAMES.md): 'rgb' exists there, rotating does not
        if pixel_format not in ("bgr", "rgb", "nv12"):
            raise ValueError("pixel_format must be 'bgr', 'rgb' or 'nv12'")
        if transpose:
            raise ValueError("transpose=True is not supported with source='device': use orientation=3, which turns the crop on the device")
        return pixel_format == "nv12"
    if pixel_format not in ("bgr", "nv12"):
        raise ValueError("pixel_format must be 'bgr' or 'nv12'")
    if pixel_format == "nv12" and transpose:
        raise ValueError("transpose=True is not supported with pixel_format='nv12': use orientation=3, which turns the crop on the device")
    return pixel_format == "nv12"


def track(estimator, frames, rect=None, transpose=False, timestamps=None, pixel_format="bgr", confidence=False, lost=None, orientation=None):
    """run_estimator_ps.py:80-109 without capture / drawing.  Yields (joints_2d, joints_3d, rect_used).

    Additive (CONFIDENCE.md): ``lost=(min_confidence, min_joints, "hold" | "reset")`` -- behind the box update, a frame with fewer than
    min_joints confidences >= min_confidence keeps its own crop for the next frame (hold) or hands it the whole frame (reset);
    "detect" (HOG.md; this loop only): the next frame's box is ``hog_box`` of the lost frame -- the reference's detector in the place of
    the whole frame; the estimator needs a detector (``set_hog_detector``);
    ``confidence=True`` yields (joints_2d, joints_3d, rect_used, confidence (21,) float64, lost flag).

    frames: iterable of uint8 BGR arrays of one size; rect: initial (x, y, w, h), default the full frame;
    transpose: the reference's `T` option (np.rot90(frame, 3)); timestamps: optional iterable for reproducible
    filtering (default wall clock, like the reference); pixel_format="nv12": the frames are (H * 3 // 2, W) NV12 arrays, converted
    and cropped on the device (no transpose).
    orientation (additive; ORIENTATION.md): the code 0 .. 7 the frames are stored under -- the picture is ``orient_view(frame, code)``;
    3 is ``transpose=True``; None (the default): the estimator's own ``orientation``.  A BGR frame is turned as a numpy view, like
    ``transpose``, and the estimator is called under code 0; an NV12 frame is turned on the device.  Rects and joints are in the
    picture's coordinates.
    """
    ts = iter(timestamps) if timestamps is not None else None
    nv12 = _nv12_checks(pixel_format, transpose)
    orientation = _orientations(estimator, orientation, 1, transpose)[0]
    own = getattr(estimator, "orientation", 0)
    call_code = orientation if nv12 else 0     # what the estimator itself still has to turn
    rule = lost_rule(lost, detect=True)
    want_conf = confidence or rule is not None
    for frame in frames:
        if transpose:
            frame = np.rot90(frame, 3)
        elif orientation and not nv12:
            frame = orient_view(frame, orientation)
        H_img, W_img = frame.shape[:2]
        if nv12:                                   # (H * 3 // 2, W): Y rows, then the U, V rows
            H_img = H_img * 2 // 3
            if orientation & 1:                    # (the picture of a quarter-turned frame)
                H_img, W_img = W_img, H_img
        if rect is None:
            rect = [0, 0, W_img, H_img]
        x, y, w, h = rect
        if w < 1 or h < 1:  # a degenerate box (all joints on one pixel): fall back to the whole frame
            x, y, w, h = rect = [0, 0, W_img, H_img]
        t = next(ts) if ts is not None else None
        kw = {"return_confidence": True} if want_conf else {}
        if call_code != own:                       # (said only where it differs from the estimator's own: any callable serves otherwise)
            kw["orientation"] = call_code
        if nv12:                                   # the device converts and crops: the rect goes along instead of a slice
            res = estimator(frame, timestamp=t, pixel_format="nv12", rect=[x, y, w, h], **kw)
        else:
            res = estimator(frame[y:y + h, x:x + w, :], timestamp=t, **kw)
        joints_2d, joints_3d = res[:2]
        joints_2d[:, 0] += y
        joints_2d[:, 1] += x
        used = [x, y, w, h]
        rect = bbox_update(joints_2d, W_img, H_img)
        gone = rule is not None and is_lost(res[2], rule[0], rule[1])
        if gone:                                   # the loss rule: this frame's crop again, the whole frame, or where the detector finds someone
            if rule[2] == "detect":
                rect = hog_box(estimator, frame, pixel_format, call_code)
            else:
                rect = list(used) if rule[2] == "hold" else [0, 0, W_img, H_img]
        if confidence:
            yield joints_2d, joints_3d, used, res[2], int(gone)
        else:
            yield joints_2d, joints_3d, used


# ---- the device loops: track_many_on_device and track_people_on_device are one scheme -- a submission is one library submit that delivers
# k results (a video's frame: 1; a people frame: one per person) -- built from the pieces below ----------------------------------------
def _given(option):
    return option is not False and option is not None


def _loop_options(estimator, device, draw, preview, view3d, lost, redetect=False, preview_style=False):
    """``draw=``, ``preview=``, ``view3d=``, ``lost=`` and ``redetect=`` of a device loop as (overlay style, preview spec, view spec, loss
    rule, re-detect spec), each None where not asked for.  ``device``: the frames are in device memory."""
    style = spec = vspec = rspec = None
    if _given(draw):
        if not device:
            raise ValueError("draw= annotates frames in device memory: it needs source='device'")
        style = draw if isinstance(draw, _native.OverlayStyle) else _native.overlay_style(parents=estimator.joint_parents)
    if _given(preview):
        if not device:
            raise ValueError("preview= scales frames in device memory: it needs source='device'")
        if isinstance(preview, _native.PreviewSpec):
            spec = _native.preview_spec(preview.factor, "rgb" if preview.out_format == _native.PIX_RGB else "bgr", style is not None)
        else:
            spec = _native.preview_spec(None if preview is True else float(preview), "bgr", style is not None)
        # The one asymmetry between the loops: a multi-video preview without draw= is submitted with a default style, made only now that
        # draw_frame has been decided without it; a people preview without draw= passes no style
        if style is None and preview_style:
            style = _native.overlay_style(parents=estimator.joint_parents)
    if _given(view3d):
        vspec = view3d if isinstance(view3d, _native.View3dSpec) else _native.view3d_spec(parents=estimator.joint_parents)
    rule = lost_rule(lost)
    if _given(redetect):
        if not device:
            raise ValueError("redetect= runs the detector over frames in device memory: it needs source='device'")
        if rule is None:
            raise ValueError("redetect= needs a lost=(min_confidence, min_joints, 'hold' | 'reset') rule: without one no frame is ever lost")
        kw = dict(redetect) if isinstance(redetect, dict) else {}
        kw.setdefault("max_hits", _native.HOG_TRACK_MAX_HITS)
        rspec = _native.hog_spec(**kw)
    return style, spec, vspec, rule, rspec


def _stored_size(f, device, nv12):
    """(H, W) of the picture a frame holds, as it is stored: a DeviceFrame's own, else from the array's shape"""
    if device:
        return (f.H, f.W)
    return (f.shape[0] * 2 // 3, f.shape[1]) if nv12 else f.shape[:2]


def _device_frame(f, pixel_format):
    """a device array's descriptor (which keeps the array alive); its producer is the stream current now"""
    d = _native.device_frame(f, pixel_format)
    d._producer = _native.default_stream()
    return d


def _upload(estimator, slot, frame, code, nv12):
    """a host frame into resident slot `slot` under orientation `code` (the slot holds the oriented frame from its upload on)"""
    estimator._orient(code)
    if nv12:
        estimator.handle.upload_frame_nv12(slot, frame)
    else:
        estimator.handle.upload_frame(slot, frame)


def _extras(h, confidence, spec, vspec, rspec):
    """what one delivery appends to its tuple, read from the result slot of the frame just delivered -- (confidence, lost flag), the
    preview (the pinned buffer of its ring slot, copied before the next submit), the view, the re-detection status"""
    if not (confidence or spec is not None or vspec is not None):
        return tuple                           # (nothing to append: tuple() is ())

    def extras():
        res = ()
        if confidence:
            res += h.result_confidence()
        if spec is not None:
            res += (h.result_preview(),)
        if vspec is not None:
            res += (h.result_view3d(),)
        if rspec is not None and confidence:
            res += (h.result_redetect()[0],)
        return res
    return extras


class _InFlight:
    """A device loop: the submissions it has in flight, oldest first, and what it switched on for them.

    ``k``: deliveries per submission; ``window``: submissions in flight at most; ``deliver(stream, joints_2d, joints_3d, rect_used)``:
    one delivery's tuple; ``result(tuples)``: what the loop yields for a submission's k tuples.  ``run`` is the loop; a caller describes
    its set-up and its submissions as a generator and yields from ``run`` of it."""

    def __init__(self, estimator, k, window, deliver, result):
        self.estimator, self.h = estimator, estimator.handle
        self.k, self.each, self.window, self.deliver, self.result = k, range(k), window, deliver, result
        self.queue = deque()                   # submission numbers
        self.held = {}                         # submission number -> the device frame it reads, until its last delivery has been collected
        self.count = 0                         # the next submission's number
        self.on = []                           # (the call that switches a thing off again, its arguments)

    def switch_on(self, stream, rspec, rule, vspec):
        """re-detection, loss rule and view of one stream, as far as asked for (re-detection first: what it refuses leaves no rule behind)"""
        h = self.h
        if rspec is not None:
            h.track_redetect(stream, rspec, True)
            self.on.append((h.track_redetect, (stream, None, False)))
        if rule is not None:
            h.track_policy(stream, *rule)
            self.on.append((h.track_policy, (stream, 0.0, 1, "off")))
        if vspec is not None:
            h.track_view3d(stream, vspec)
            self.on.append((h.track_view3d, (stream, None)))

    def collect(self):
        n = self.queue.popleft()
        got, deliver, collect_tracked = [], self.deliver, self.h.collect_tracked
        try:
            for _ in self.each:
                got.append(deliver(*collect_tracked()))
        except _native.VnectError as e:
            for _ in range(self.k - 1 - len(got)):     # the submission's other deliveries: collected and dropped
                try:
                    self.h.collect_tracked()
                except _native.VnectError:
                    pass
            self.estimator._raise_like_reference(e)
        finally:
            self.held.pop(n, None)
        return self.result(got)

    def run(self, submissions):
        """The loop.  ``submissions`` yields (call, args, hold, after), its set-up done by the time it yields the first: ``call(*args)``
        makes one library submit (and what belongs to it); ``hold``: the device frame it reads, or None; ``after``: the number of a
        submission that must have been collected before ``call`` runs, or None.  A refused submit raises as in ``track``: behind every
        earlier frame's results.  An accepted one is followed by results until the window has room again.  Whatever ends the loop -- a
        refused crop or timestamp, the caller's ``break``, any exception, in the set-up too -- what is still in flight is collected and
        dropped, the estimator's own orientation is back in force and exactly what ``switch_on`` switched on is off again, each call on
        its own: the estimator is usable at once afterwards (``track`` leaves nothing in flight either)."""
        queue, window, held, collect = self.queue, self.window, self.held, self.collect
        try:
            for call, args, hold, after in submissions:
                try:
                    if after is not None:
                        while any(n == after for n in queue):
                            yield collect()
                    call(*args)
                except _native.VnectError as e:
                    while queue:
                        yield collect()
                    self.estimator._raise_like_reference(e)
                if hold is not None:
                    held[self.count] = hold
                queue.append(self.count)
                self.count += 1                # (the submission has been made: `submissions` reads the count for its next one)
                while len(queue) >= window:
                    yield collect()
            while queue:
                yield collect()
        finally:
            while queue:
                queue.popleft()
                for _ in self.each:
                    try:
                        self.h.collect_tracked()
                    except _native.VnectError:
                        pass
            held.clear()
            self.estimator._orient(None)
            for off, args in self.on:          # (nothing is in flight any more)
                try:
                    off(*args)
                except _native.VnectError:
                    pass


def track_on_device(estimator, frames, rect=None, transpose=False, timestamps=None, ahead=1, source="pinned", stream=0, pixel_format="bgr",
                    confidence=False, lost=None, draw=False, orientation=None, preview=False, view3d=False, redetect=False):
    """``track`` with the crop box kept on the GPU (vnect_track_begin / vnect_submit_tracked*): yields what ``track`` yields, bit for bit.

    Each frame goes to the device whole; the device crops it with the box it grew from the previous frame's joints, so the host submits
    frame t+1 without waiting for frame t.  ``ahead``: frames submitted before the oldest is collected (0: one at a time; at most
    ``max(lanes, 2) - 1``).  ``source``: "pinned" -- the frame is written into the handle's pinned buffers and only the crop's rows cross
    PCIe -- "resident" (vnect_upload_frame of the whole frame) -- or "device": the frames are arrays in device memory (anything with
    ``__cuda_array_interface__``; ``pixel_format`` may then be "rgb" as well), read where they lie when the frame runs and held until it
    is collected (no ``transpose``).  ``stream``: which of the handle's video streams (its filter bank).
    ``rect`` must start inside the frame (``track`` would slice from outside it); one that runs past the far edges is cropped as
    ``track`` crops it.  However the loop ends -- a refused crop, the caller's ``break``, an exception -- nothing stays in flight.
    ``confidence`` / ``lost``: as in ``track``; the rule runs on the device (vnect_track_policy).
    ``draw`` (``source="device"`` only; OVERLAY.md): True, or an ``_native.overlay_style(...)`` -- every frame is annotated IN PLACE with its
    own joints and the rect it was cropped with (run_estimator_ps.py:92-94) by the time it is yielded; the results are those of
    ``draw=False``, bit for bit.
    ``orientation`` (ORIENTATION.md): the code 0 .. 7 the frames are stored under, from every source (None: the estimator's own); the crop
    is turned on the device.
    ``preview`` (``source="device"`` only; PREVIEW.md): True (the reference's 1024 on the longer side), a factor, or an
    ``_native.preview_spec(...)`` -- every yielded tuple gets the frame's display picture appended (run_estimator_ps.py:94-96: the frame
    annotated with its own joints and ``rect_used``, scaled; a fresh (dh, dw, 3) array, or None for a frame without one), computed on
    the device; the frame is not written unless ``draw`` is given too, and then the preview is that of the clean frame.
    ``view3d`` (every ``source``; VIEW3D.md): True (the reference's plot: 400 x 400, view_init(-90, -90)) or an
    ``_native.view3d_spec(...)`` -- every yielded tuple gets the frame's 3-D skeleton view appended last (run_estimator_ps.py:90,
    124-126; src/utils.py:272-304: a fresh (rows, cols, 3) array, the picture ``render.view3d_exact`` gives for the ``joints_3d`` yielded
    with it), rendered on the device behind the frame's joints stage; the other results are those of ``view3d=False``, bit for bit.
    ``redetect`` (``source="device"`` and a ``lost=`` rule of "hold" or "reset" only; HOG.md): True (the detector's defaults), or a dict of
    ``detect_people``'s spec -- the next box of a lost frame is ``hog_box`` of that frame, found on the device with no host wait: with
    "reset" the loop yields what ``track(lost=(c, n, "detect"))`` yields, bit for bit.  A frame with more than ``max_hits`` (at most 4096)
    hits hands on the whole frame where ``track`` would raise.  With ``confidence=True`` every tuple gets the frame's re-detection
    status appended last (0 none ran, 1 found, 2 nobody found, 3 overflow).  The estimator needs a detector (``set_hog_detector``)."""
    for res in track_many_on_device(estimator, [frames], None if rect is None else [rect], transpose,
                                    None if timestamps is None else [timestamps], ahead, source, [stream], pixel_format, confidence, lost, draw,
                                    orientation, preview, view3d, redetect):
        yield res[1:]


def track_many_on_device(estimator, videos, rects=None, transpose=False, timestamps=None, ahead=1, source="pinned", streams=None,
                         pixel_format="bgr", confidence=False, lost=None, draw=False, orientation=None, preview=False, view3d=False, redetect=False):
    """Several tracked videos on one handle, video i on stream ``streams[i]`` (default i): their frames are submitted in turn and
    overlap on the handle's lanes.  Yields (i, joints_2d, joints_3d, rect_used) in submission order; every video's sequence is what
    ``track`` yields for it alone on a handle of its own.  ``rects`` / ``timestamps``: one per video (or None).
    ``pixel_format="nv12"``: every frame is an (H * 3 // 2, W) NV12 array; the device converts the crop's rows as it reads them out of
    the pinned buffer (or, ``source="resident"``, the whole frame on upload).
    ``lost=(min_confidence, min_joints, "hold" | "reset")``: every video's stream gets this loss rule for the loop (and is off again
    afterwards); ``confidence=True`` appends
    (confidence, lost flag) to every tuple.
    ``draw``, ``preview``, ``view3d``, ``redetect``: as in ``track_on_device`` (the view, then the re-detection status, are the last
    elements of every tuple).
    ``orientation``: one code for all videos or one per video (ORIENTATION.md; None: the estimator's own): every stream keeps the code its track began with, so
    videos with different orientations share the handle; the estimator's own orientation is back in force afterwards."""
    device = source == "device"
    style, spec, vspec, rule, rspec = _loop_options(estimator, device, draw, preview, view3d, lost, redetect, preview_style=True)
    nv12 = _nv12_checks(pixel_format, transpose, source)
    codes = _orientations(estimator, orientation, len(videos), transpose)
    if source not in ("pinned", "resident", "device"):
        raise ValueError("source must be 'pinned', 'resident' or 'device'")
    h = estimator.handle
    n = len(videos)
    streams = list(range(n)) if streams is None else [int(s) for s in streams]
    its = [iter(v) for v in videos]
    tss = [iter(t) if t is not None else None for t in (timestamps if timestamps is not None else [None] * n)]
    rects = rects if rects is not None else [None] * n
    limit = max(int(estimator._cfg.get("lanes", 1)), 2)
    nslots = int(getattr(h, "num_frame_slots", 0) or 4)
    video_of = {s: i for i, s in enumerate(streams)}
    extras = _extras(h, confidence, spec, vspec, rspec)
    loop = _InFlight(estimator, 1, max(0, min(int(ahead), limit - 1)) + 1,
                     lambda s, j2, j3, used: (video_of[s], j2, j3, used) + extras(), itemgetter(0))

    def prep(f):
        if device:
            return _device_frame(f, pixel_format)
        f = np.rot90(f, 3) if transpose else f
        return np.ascontiguousarray(f, dtype=np.uint8)

    if spec is not None:                       # the device submit of this loop, and what it takes behind the producer stream
        submit_device, tail = h.submit_tracked_device_preview, (style, spec)
    elif style is not None:
        submit_device, tail = h.submit_tracked_device_draw, (style,)
    else:
        submit_device, tail = h.submit_tracked_device, ()

    submit_pinned = h.submit_tracked_pinned_nv12 if nv12 else h.submit_tracked_pinned

    def copy_submit_pinned(view, frame, *args):
        view[...] = frame
        submit_pinned(*args)

    def submit_resident(s, frame, t2d, t3d, code):
        slot = loop.count % nslots
        _upload(estimator, slot, frame, code, nv12)
        h.submit_tracked(s, slot, t2d, t3d)

    def submissions():
        pending, sizes = [None] * n, [None] * n
        for i in range(n):                     # the first frame of every video: its size starts the stream's track
            f = next(its[i], None)
            if f is not None:
                pending[i] = prep(f)
                H, W = sizes[i] = _stored_size(pending[i], device, nv12)
                estimator._orient(codes[i])    # the stream keeps the code in force now; H, W: the picture's
                h.track_begin(streams[i], W if codes[i] & 1 else H, H if codes[i] & 1 else W, rects[i])
                loop.switch_on(streams[i], rspec, rule, vspec)     # (nothing is in flight yet)
        flat = []
        if source == "pinned":                 # the two pinned buffers, sized for the largest frame (nothing is in flight yet)
            nbytes = max([p.size for p in pending if p is not None] + [3])
            flat = [h.frame_buffer(b, 1, (nbytes + 2) // 3).reshape(-1) for b in range(2)]
        live = [p is not None for p in pending]
        while any(live):
            for i in range(n):
                if not live[i]:
                    continue
                frame = pending[i]
                t2d, t3d = estimator._stamps(next(tss[i]) if tss[i] is not None else None)
                if device:
                    yield submit_device, (streams[i], frame, t2d, t3d, frame._producer) + tail, frame, None
                elif source == "pinned":
                    H, W = sizes[i]
                    b = loop.count % 2
                    args = (streams[i], b, W, H * W, W, t2d, t3d) if nv12 else (streams[i], b, W * 3, t2d, t3d)
                    view = flat[b][:frame.size].reshape(frame.shape)
                    if frame.ctypes.data == view.ctypes.data:      # captured into this buffer already (the view itself): not copied
                        yield submit_pinned, args, None, None
                    else:                      # the buffer's last frame, two submissions back, must have been copied: collected
                        yield copy_submit_pinned, (view, frame) + args, None, loop.count - 2
                else:
                    yield submit_resident, (streams[i], frame, t2d, t3d, codes[i]), None, None
                f = next(its[i], None)
                if f is None:
                    live[i] = False
                else:
                    pending[i] = prep(f)
                    if _stored_size(pending[i], device, nv12) != sizes[i]:
                        raise ValueError("frames of one video must have one size")

    yield from loop.run(submissions())


def people_boxes(estimator, frame, people, pixel_format="bgr", orientation=None, stream=None, **spec):
    """The first boxes of ``people`` persons in one frame (PEOPLE.md; the reference keeps one: src/hog_box.py:26-31).  The detections of
    ``estimator.detect_people`` ordered by area, largest first, equal areas by (y, x); the first ``people`` of them through ``cal_rect``;
    missing ones are the whole frame.  Host-only and deterministic.  Returns ``people`` rects [x, y, w, h] in the oriented picture's
    coordinates."""
    rects, _ = estimator.detect_people(frame, pixel_format=pixel_format, orientation=orientation, stream=stream, **spec)
    if _native.is_device_array(frame):
        f = _native.device_frame(frame, pixel_format)
        H, W = int(f.H), int(f.W)
    else:
        H, W = frame.shape[:2]
        if pixel_format == "nv12":
            H = H * 2 // 3
    if (estimator.orientation if orientation is None else orientation) & 1:
        H, W = W, H
    found = sorted(([int(v) for v in r] for r in rects), key=lambda r: (-r[2] * r[3], r[1], r[0]))
    boxes = [cal_rect(r, H, W) for r in found[:int(people)]]
    return boxes + [[0, 0, W, H] for _ in range(int(people) - len(boxes))]


def track_people_on_device(estimator, frames, rects, timestamps=None, ahead=1, source="device", pixel_format="bgr", confidence=False,
                           lost=None, draw=False, orientation=None, preview=False, view3d=False):
    """P persons of ONE video tracked on a people estimator (``VNectEstimator(people=P)``; PEOPLE.md): person p is stream p and starts at
    ``rects[p]`` (``people_boxes`` chooses them; None: the whole frame).  Every frame is submitted ONCE for everybody
    (vnect_submit_people*); two persons' crops share a conv stack where the estimator pairs.  Yields one tuple per frame: a list of P
    ``(joints_2d, joints_3d, rect_used[, confidence, lost][, view])`` -- each person's sequence is what ``track`` yields for that person
    alone on an estimator of its own, bit for bit.  ``source``: "device" (arrays in device memory, read where they lie and held until the
    frame has been collected) or "resident" (host arrays, uploaded whole); pinned sources are not supported.
    ``timestamps``, ``pixel_format``, ``confidence``, ``lost``, ``orientation``, ``view3d``: as in ``track_on_device``, for every person.
    ``draw`` (``source="device"`` only): every person's skeleton and rect are drawn into the frame, in person order, only after every
    person's crop has been read from the clean frame: the results are those of ``draw=False``.
    ``preview`` (``source="device"`` only; True, a factor or an ``_native.preview_spec(...)``): every yielded tuple gets the frame's ONE
    display picture appended -- the clean frame annotated with every person in person order (``render.draw_limbs_2d_exact`` P times), then
    scaled (``render.resize_u8_exact``) -- computed on the device; the frame is written only if ``draw`` is given too.
    ``ahead``: frames submitted before the oldest is collected, clipped to what the unit limit (``max(lanes, 2)`` units in flight, a frame
    is ceil(P / 2) units paired, P unpaired) and the result ring (8) allow.  However the loop ends, nothing stays in flight."""
    h = estimator.handle
    P = len(rects)
    if not 1 <= P <= int(getattr(h, "people", 0)):
        raise ValueError("rects must hold 1 .. people rects: make the estimator with VNectEstimator(people=P)")
    if source not in ("device", "resident"):
        raise ValueError("source must be 'device' or 'resident' (pinned sources are not supported in people mode)")
    device = source == "device"
    style, spec, vspec, rule, _ = _loop_options(estimator, device, draw, preview, view3d, lost)
    nv12 = _nv12_checks(pixel_format, False, source)
    code = _orientations(estimator, orientation, 1, False)[0]
    lanes = max(int(estimator._cfg.get("lanes", 1)), 1)
    paired = bool(getattr(h, "pair_people", False)) and P >= 2 and 2 * len(estimator.scales) <= 8
    units = (P + 1) // 2 if paired else P
    ts = iter(timestamps) if timestamps is not None else None
    nslots = int(getattr(h, "num_frame_slots", 0) or 4)
    extras = _extras(h, confidence, None, vspec, None)
    def result(people):                        # (the frame's one picture came with its last person)
        return (people, h.result_preview()) if spec is not None else (people,)

    loop = _InFlight(estimator, P, max(0, min(int(ahead), max(lanes, 2) // units - 1, 8 // P - 1)) + 1,
                     lambda s, j2, j3, used: (j2, j3, used) + extras(), result)

    def submit_resident(frame, t2d, t3d):
        slot = loop.count % nslots
        _upload(estimator, slot, frame, code, nv12)
        h.submit_people(P, slot, t2d, t3d)

    def submissions():
        size = None
        for f in frames:
            frame = _device_frame(f, pixel_format) if device else np.ascontiguousarray(f, dtype=np.uint8)
            H, W = _stored_size(frame, device, nv12)
            if size is None:
                estimator._orient(code)        # every person keeps the code in force now; pH, pW: the picture's
                pH, pW = (W, H) if code & 1 else (H, W)
                h.people_begin(P, pH, pW, [[0, 0, pW, pH] if r is None else r for r in rects])
                for p in range(P):
                    loop.switch_on(p, None, rule, vspec)
                size = (H, W)
            elif (H, W) != size:
                raise ValueError("frames of one video must have one size")
            t2d, t3d = estimator._stamps(next(ts) if ts is not None else None)
            if device:
                yield h.submit_people_device, (P, frame, t2d, t3d, frame._producer, style, spec), frame, None
            else:
                yield submit_resident, (frame, t2d, t3d), None, None

    yield from loop.run(submissions())


def synthetic_stream(stream, n_frames, height=368, width=368, smooth=True):
    """Deterministic synthetic video: frame k of stream s has seed 1234 + 1000*s + k."""
    from .parallel import stream_seed
    from .weights import uniform01
    for k in range(n_frames):
        seed = stream_seed(stream, k)
        if not smooth:
            yield (uniform01(seed, height * width * 3) * 256).astype(np.uint8).reshape(height, width, 3)
            continue
        g = uniform01(seed, 9 * 9 * 3).reshape(9, 9, 3).astype(np.float64)
        ys, xs = np.linspace(0, 8, height, endpoint=False), np.linspace(0, 8, width, endpoint=False)
        y0, x0 = ys.astype(int), xs.astype(int)
        fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
        a = g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx
        b = g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx
        yield np.clip((a * (1 - fy) + b * fy) * 256, 0, 255).astype(np.uint8)


def main(argv=None):
    """python -m vnect_amd.runner [picture.jpg]: the run_pic.py flow on the MI355X, printing the 21 joints."""
    import os
    import sys
    argv = sys.argv[1:] if argv is None else argv
    from .estimator import VNectEstimator
    path = argv[0] if argv else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "tests", "golden", "test_pic.jpg")
    img = load_bgr(path)
    est = VNectEstimator()
    j2, j3, rect = run_pic(est, img)
    print("rect", rect)
    for i in range(21):
        print(i, j2[i], j3[i])
    est.close()


if __name__ == "__main__":
    main()
