"""VNectEstimator: the reference's call surface (src/estimator.py:16-142) over libvnect_hip.so.

    from vnect_amd import VNectEstimator
    est = VNectEstimator()                       # reference defaults (scales [1, 0.85, 0.7])
    joints_2d, joints_3d = est(frame_bgr_uint8)  # (21,2) float64 [row, col], (21,3) float32 mm

Everything from gen_input_batch to the un-mapping runs on the MI355X in hand-written HIP kernels;
this file only marshals arguments.  Additive keyword arguments (not in the reference): ``scales``,
``weights``, ``seed``, ``device``, ``precision``, ``paper_res2c``, ``use_graph``, and
``timestamp=`` on ``__call__`` for reproducible filtering (default: wall clock, like the reference).
"""
import time

import numpy as np

from . import _native
from .weights import MASTER_SEED, check_schema, load_weights, synthetic_weights

# VNectEstimator(precision=...) -> vnect_config::precision
PRECISIONS = {"fp32": _native.FP32, "bf16": _native.BF16, "fp32_split": _native.FP32_SPLIT, "fp16": _native.FP16}


class VNectEstimator:
    # class attributes of src/estimator.py:18-25
    box_size = 368
    hm_factor = 8
    joints_sum = 21
    joint_parents = [16, 15, 1, 2, 3, 1, 5, 6, 14, 8, 9, 14, 11, 12, 14, 14, 1, 4, 7, 10, 13]

    def __init__(self, scales=None, weights=None, seed=MASTER_SEED, device=0, precision="fp32", paper_res2c=False,
                 use_graph="auto", numpy_promotion="legacy", verbose=True, lanes=1, orientation=0, hog_detector=None,
                 people=0, pair_people=False):
        if verbose:
            print('Initializing VNect Estimator...')
        # src/estimator.py:32; "for faster loops, use less scales e.g. [1], [1, 0.7]"
        self._scales = [float(s) for s in (scales if scales is not None else [1, 0.85, 0.7])]
        if isinstance(weights, str):
            weights = load_weights(weights)
        elif weights is None:
            # no trained weights ship with the reference (models/*/README.md): seeded synthetic ones
            weights = synthetic_weights(seed)
        else:
            check_schema(weights)
        self._cfg = dict(device=device, precision=PRECISIONS[precision],
                         paper_res2c=paper_res2c, use_graph=use_graph,
                         numpy_promotion={"legacy": 0, "nep50": 1}[numpy_promotion], lanes=lanes)
        # people mode (additive; PEOPLE.md): ``people=P`` (1 .. 4) -- runner.track_people_on_device follows P persons of one video,
        # person p on stream p; ``pair_people``: two persons' crops share one conv stack where the scale list allows (2 S <= 8)
        self.people = int(people)
        if self.people:
            self._cfg.update(people=self.people, pair=bool(pair_people))
        self._submitted = 0
        self._weights = weights
        self._orientation = self._check_orientation(orientation)
        self._hog_detector = None if hog_detector is None else np.array(hog_detector, dtype=np.float32).reshape(-1)
        self._h = None
        self._open()
        self.verbose = verbose
        if verbose:
            print('VNect Estimator initialized.')

    def _open(self):
        if self._h is not None:
            self._h.close()
        self._h = _native.Handle(self._scales, **self._cfg)
        self._h.set_weights(self._weights)
        self._h.finalize()
        self._orient(None)
        if self._hog_detector is not None:
            self._h.hog_set_detector(self._hog_detector)

    # -- orientation (additive; ORIENTATION.md): frames that are STORED rotated / mirrored ------------------------------
    @staticmethod
    def _check_orientation(o):
        if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or not 0 <= int(o) <= 7:
            raise ValueError("orientation must be a code 0 .. 7: the picture is np.rot90(frame, code & 3), mirrored when code & 4")
        return int(o)

    @property
    def orientation(self):
        """How the frames this estimator is given are stored: code 0 .. 7, the picture is ``np.rot90(frame, code & 3)``, mirrored
        (``[:, ::-1]``) when ``code & 4``.  3 is the reference's ``T`` option (run_estimator_ps.py:57-62, 81-85).  Rects, boxes and
        joints are in the picture's coordinates; the turn happens on the device, inside the crop's copy."""
        return self._orientation

    @orientation.setter
    def orientation(self, value):
        self._orientation = self._check_orientation(value)
        self._orient(None)

    def _orient(self, orientation):
        """the handle's orientation for the call at hand: `orientation`, or (None) the estimator's; set only when it differs"""
        o = self._orientation if orientation is None else self._check_orientation(orientation)
        if o != self._h.orientation:      # (the handle remembers what it was last given, whoever gave it)
            self._h.set_orientation(o)

    # `self.scales` is a plain attribute in the reference; assigning it re-plans the pyramid
    @property
    def scales(self):
        return list(self._scales)

    @scales.setter
    def scales(self, value):
        value = [float(s) for s in value]
        if len(value) == len(self._scales):
            self._h.set_scales(value)
            self._scales = value
        else:  # batch size of the conv stack changes: rebuild the handle (filters restart, as a new estimator would)
            self._scales = value
            self._open()

    @property
    def handle(self):
        return self._h

    @staticmethod
    def gen_input_batch(img_input, box_size, scales, _handle=None, orientation=None):
        """src/estimator.py:70-81 on the device.  Returns (batch (S,368,368,3) f32, scaler, [offset_x, offset_y])."""
        if box_size != 368:
            raise ValueError("box_size is fixed at 368 by the network")
        h = _handle
        own = h is None or h.num_scales != len(scales)
        if own:
            # a pre-processing-only handle: resize tables + the batch buffer, no weights, no launch plan
            h = _native.Handle(list(scales), preprocess_only=True)
        else:
            h.set_scales(scales)
        # orientation (additive; ORIENTATION.md): the batch of the oriented picture.  None: the code the handle holds (a handle of its
        # own: 0); a given handle is left with the code it was found with
        found = h.orientation
        o = found if orientation is None else VNectEstimator._check_orientation(orientation)
        try:
            if o != found:
                h.set_orientation(o)
            return h.preprocess(img_input)
        finally:
            if own:
                h.close()
            elif o != found:
                h.set_orientation(found)

    def joint_filter(self, joints, dim=2, timestamp=None):
        """src/estimator.py:83-95: the estimator's 2-D (``dim=2``) or 3-D OneEuro bank applied to ``joints`` IN PLACE; returns
        ``joints``.  The filter state lives on the device (the same banks ``__call__`` advances), so this runs one tiny
        kernel.  A float32 array is filtered the way the reference filters its float32 ``joints_3d`` (numpy scalar promotion,
        ``numpy_promotion=``), any other dtype in float64 like ``joints_2d``.  ``timestamp=`` is additive (default: one
        ``time.time()`` per call, like the reference)."""
        t = time.time() if timestamp is None else float(timestamp)
        if not isinstance(joints, np.ndarray):  # the reference indexes joints[i, 0]: anything but an array fails there too
            raise TypeError("joints must be a numpy array (it is filtered in place)")
        a = joints
        dim = 2 if dim == 2 else 3  # the reference's `else` branch takes every other value as 3 (dim=1, dim=5, ... included)
        if a.ndim != 2 or a.shape[0] < self.joints_sum or a.shape[1] < dim:  # where the reference's joints[i, 2] raises
            raise IndexError("joints must hold at least (%d, %d) values" % (self.joints_sum, dim))
        try:
            out = self._h.joint_filter(dim, a[:self.joints_sum, :dim], a.dtype == np.float32, t)
        except _native.VnectError as e:
            self._raise_like_reference(e)
        a[:self.joints_sum, :dim] = out  # in place; numpy casts to the array's dtype as `joints[i, 0] = ...` does
        return joints

    @staticmethod
    def _raise_like_reference(e):
        if e.code == _native.E_TIMESTAMP:
            raise ZeroDivisionError("float division by zero") from e  # src/OneEuroFilter.py:66
        if e.code == _native.E_TIMEORDER:  # negative freq -> alpha outside (0, 1]: LowPassFilter.__setAlpha, OneEuroFilter.py:19-23
            raise ValueError("alpha should be in (0.0, 1.0]: timestamp earlier than the previous one") from e
        raise e

    def postprocess(self, maps, timestamp=None, scaler=1.0, offset_x=0, offset_y=0, return_confidence=False):
        """``return_confidence=True`` (additive; CONFIDENCE.md): a third value, the (21,) float64 per-joint confidences."""
        t2d, t3d = self._stamps(timestamp)
        try:
            res = self._h.postprocess(maps, t2d, t3d, scaler, offset_x, offset_y)
        except _native.VnectError as e:
            self._raise_like_reference(e)
        return res + (self._h.result_confidence()[0],) if return_confidence else res

    def forward(self, batch):
        """sess.run equivalent (src/estimator.py:100-104): (S,368,368,3) -> (S,46,46,84)."""
        return self._h.forward(batch)

    @staticmethod
    def _stamps(timestamp):
        if timestamp is None:  # src/estimator.py:84 reads time.time() once per joint_filter call
            return time.time(), time.time()
        if isinstance(timestamp, (tuple, list)):
            return float(timestamp[0]), float(timestamp[1])
        return float(timestamp), float(timestamp)

    @staticmethod
    def _format(pixel_format, rect, device=False):
        if device:  # a frame in device memory: 'rgb' exists here only (a host caller flips with a slice), and any format takes a rect
            if pixel_format not in ("bgr", "rgb", "nv12"):
                raise ValueError("pixel_format must be 'bgr', 'rgb' or 'nv12'")
            return pixel_format == "nv12"
        if pixel_format == "rgb":
            raise ValueError("pixel_format='rgb' is for frames in device memory (a host caller passes frame[..., ::-1])")
        if pixel_format not in ("bgr", "nv12"):
            raise ValueError("pixel_format must be 'bgr' or 'nv12'")
        if rect is not None and pixel_format != "nv12":
            raise ValueError("rect= is for pixel_format='nv12' (a BGR caller slices the frame)")
        return pixel_format == "nv12"

    def __call__(self, img_input, timestamp=None, pixel_format="bgr", rect=None, stream=None, return_confidence=False, orientation=None):
        """``pixel_format="nv12"`` (additive): ``img_input`` is a 2-D uint8 array of ``H * 3 // 2`` rows -- H rows of Y, the interleaved
        U, V plane from row H on; row-strided views are fine -- converted to BGR on the device (NV12.md).  ``rect=(x, y, w, h)``: only
        that crop, as ``frame[y:y + h, x:x + w]`` of the converted frame; the joints are in crop coordinates.

        A frame already in DEVICE memory (additive; DEVICE_FRAMES.md): any object with ``__cuda_array_interface__`` -- a uint8 (H, W, 3)
        torch tensor on the GPU with any positive strides (packed, ``chw.permute(1, 2, 0)``, ``bgra[..., :3]``, any slice), read where it
        lies; ``pixel_format="rgb"`` for RGB order, ``"nv12"`` for an (H * 3 // 2, W) array or a ``(y, uv)`` pair.  ``stream=``: the
        integer handle of the stream that wrote it (default: torch's current stream if torch is imported, else the default stream).

        ``return_confidence=True`` (additive; CONFIDENCE.md): a third value, a fresh (21,) float64 array -- per joint the height of its
        heat-map's peak, the value of the element ``np.argmax`` picks in ``src/utils.py:169-172``.

        ``orientation=`` (additive; ORIENTATION.md): the code this frame is stored under (default: the estimator's ``orientation``);
        ``rect`` and the joints are in the oriented picture's coordinates."""
        t0 = time.time()
        t2d, t3d = self._stamps(timestamp)
        device = _native.is_device_array(img_input)
        nv12 = self._format(pixel_format, rect, device)
        self._orient(orientation)
        try:
            if device:
                joints_2d, joints_3d = self._h.infer_device(_native.device_frame(img_input, pixel_format, rect), t2d, t3d, stream)
            else:
                joints_2d, joints_3d = self._h.infer_nv12(img_input, t2d, t3d, rect) if nv12 else self._h.infer(img_input, t2d, t3d)
        except _native.VnectError as e:
            self._raise_like_reference(e)
        if self.verbose:
            print('FPS: {:>2.2f}'.format(1 / max(time.time() - t0, 1e-9)))
        if return_confidence:
            return joints_2d, joints_3d, self._h.result_confidence()[0]
        return joints_2d, joints_3d

    # -- pipelined use (additive; the reference's loop is strictly one frame at a time) --------------------------------
    def submit(self, img_input, timestamp=None, pixel_format="bgr", rect=None, stream=None, orientation=None):
        """Queue a frame and return at once; at most ``max(lanes, 2)`` may be in flight.  With ``lanes=2`` / ``3`` the frames
        overlap on the GPU (+29 % frames/s for one video stream at three lanes -- `pipelined_frames_per_s_per_gpu` against `value` in
        profiles/r06_bench_line.json -- at the price of their latency); ``collect()`` returns
        results in order and they are bit-identical to calling the estimator frame by frame."""
        t2d, t3d = self._stamps(timestamp)
        slot = self._submitted % 4
        device = _native.is_device_array(img_input)
        nv12 = self._format(pixel_format, rect, device)
        self._orient(orientation)    # (frames already in flight keep theirs: their slots hold the oriented frame)
        try:
            if device:  # (the upload is done with the caller's buffer when it returns)
                self._h.upload_frame_device(slot, _native.device_frame(img_input, pixel_format, rect), stream)
            elif nv12:
                self._h.upload_frame_nv12(slot, img_input, rect)
            else:
                self._h.upload_frame(slot, img_input)
            self._h.submit_resident(slot, t2d, t3d)
        except _native.VnectError as e:
            self._raise_like_reference(e)
        self._submitted += 1

    def collect(self, return_confidence=False):
        """(joints_2d, joints_3d) of the oldest frame in flight; ``return_confidence=True``: and that frame's (21,) confidences."""
        res = self._h.collect()
        return res + (self._h.result_confidence()[0],) if return_confidence else res

    def draw(self, frame, joints_2d, rect=None, confidence=None, pixel_format="bgr", min_confidence=None, colors=None, stream=None,
             orientation=None):
        """Additive (OVERLAY.md): the reference's ``utils.draw_limbs_2d`` (src/utils.py:222-243; run_estimator_ps.py:92-94) on a frame in
        DEVICE memory -- anything with ``__cuda_array_interface__``, in every layout the estimator reads (``pixel_format`` "bgr", "rgb" or
        "nv12") -- drawn IN PLACE by one kernel launch, and returned.  ``joints_2d``: (21, 2) [row, col] in the frame's coordinates;
        ``rect``: (x, y, w, h) or None; ``min_confidence`` with ``confidence`` (21,): limbs with an end below it are left out;
        ``colors``: (limb_bgr, rect_bgr), either None for the reference's.  The pixels are those of ``render.draw_limbs_2d_exact``."""
        if not _native.is_device_array(frame):
            raise ValueError("draw() takes a frame in device memory; render.draw_limbs_2d_exact draws into host arrays")
        self._format(pixel_format, None, True)
        self._orient(orientation)    # joints and rect are in the oriented picture's coordinates (an NV12 target: orientation 0 only)
        style = _native.overlay_style(min_confidence, colors, self.joint_parents)
        self._h.draw_device(_native.device_frame(frame, pixel_format), joints_2d, rect, confidence, style, stream)
        return frame

    def preview(self, frame, joints_2d=None, rect=None, confidence=None, min_confidence=None, colors=None, pixel_format="bgr", factor=None,
                out=None, out_format="bgr", stream=None, orientation=None):
        """Additive (PREVIEW.md): the picture the reference shows (run_estimator_ps.py:94-96: ``draw_limbs_2d`` into ``frame.copy()``, then
        ``img_scale`` to 1024 on the longer side) of a frame in DEVICE memory -- anything ``draw`` takes -- computed by one kernel launch
        that reads the frame where it lies and NEVER writes it.  ``joints_2d`` / ``rect`` None: no limbs / no rectangle; ``factor`` None:
        1024 / the oriented picture's longer side; ``out_format`` "bgr" or "rgb".  Returns a fresh (dh, dw, 3) uint8 numpy array -- or, with
        ``out`` (a device array with ``__cuda_array_interface__``: (dh, dw, 3) uint8, unit channel stride, 3-byte pixel stride), fills it
        and returns it.  The pixels are those of ``render.preview_exact``."""
        if not _native.is_device_array(frame):
            raise ValueError("preview() takes a frame in device memory; render.preview_exact computes the same picture from host arrays")
        self._format(pixel_format, None, True)
        self._orient(orientation)    # joints and rect are in the oriented picture's coordinates
        style = _native.overlay_style(min_confidence, colors, self.joint_parents)
        spec = _native.preview_spec(factor, out_format)
        f = _native.device_frame(frame, pixel_format)
        dh, dw = self._h.preview_size(f, spec)
        if out is None:
            res = np.empty((dh, dw, 3), np.uint8)
            self._h.preview_device(f, spec, res.ctypes.data, 3 * dw, joints_2d, rect, confidence, style, stream)
            return res
        ptr, shape, strides = _native._cai(out, 3, "out")
        if shape != (dh, dw, 3) or strides[2] != 1 or strides[1] != 3 or strides[0] < 3 * dw:
            raise ValueError("out must be a uint8 (%d, %d, 3) device array with unit channel stride and 3-byte pixel stride" % (dh, dw))
        self._h.preview_device(f, spec, ptr, strides[0], joints_2d, rect, confidence, style, stream)
        return out

    def preview_size(self, H, W, factor=None, orientation=None):
        """Additive (PREVIEW.md): (rows, columns) of ``preview``'s result for a stored (H, W) frame (an NV12 frame: its picture's H, W)."""
        self._orient(orientation)
        f = _native.DeviceFrame()
        f.struct_size, f.H, f.W = _native.C.sizeof(_native.DeviceFrame), int(H), int(W)
        return self._h.preview_size(f, _native.preview_spec(factor))

    def view3d(self, joints_3d, size=400, view=None, out=None, confidence=None, **spec):
        """Additive (VIEW3D.md): the reference's second window -- the 3-D skeleton plot its loop feeds ``joints_3d`` through ``q_joints``
        (run_estimator_ps.py:90, 124-126; src/utils.py:272-304) -- rendered by one kernel launch.  ``joints_3d``: (21, 3) as the estimator
        returns it; ``size``: rows = cols, or (rows, cols); ``view``: None for the reference's ``view_init(-90, -90)``, or
        ``render.view_matrix(elev, azim)``; ``confidence`` (21,) with ``min_confidence=``: limbs with an end below it are left out;
        ``spec``: ``_native.view3d_spec``'s other arguments (``extent``, ``line_width``, ``background``, ``colors``, ``parents``,
        ``min_confidence``, ``out_format``, ``order``).  Returns a fresh (rows, cols, 3) uint8 numpy array -- or, with ``out`` (a numpy array
        or a device array with ``__cuda_array_interface__``: (rows, cols, 3) uint8, unit channel stride, 3-byte pixel stride, any row pitch:
        a column block of a wider canvas counts), fills it and returns it.  The pixels are those of ``render.view3d_exact``."""
        spec.setdefault("parents", self.joint_parents)
        sp = _native.view3d_spec(size, view, **spec)
        rows, cols = sp.rows, sp.cols
        if out is None:
            res = np.empty((rows, cols, 3), np.uint8)
            self._h.view3d_device(joints_3d, sp, res.ctypes.data, 3 * cols, confidence)
            return res
        if _native.is_device_array(out):
            ptr, shape, strides = _native._cai(out, 3, "out")
        else:
            if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags.writeable:
                raise ValueError("out must be a writeable uint8 numpy array or a device array")
            ptr, shape, strides = out.ctypes.data, out.shape, out.strides
        if tuple(shape) != (rows, cols, 3) or strides[2] != 1 or strides[1] != 3 or (rows > 1 and strides[0] < 3 * cols):
            raise ValueError("out must be a uint8 (%d, %d, 3) array with unit channel stride and 3-byte pixel stride" % (rows, cols))
        self._h.view3d_device(joints_3d, sp, ptr, strides[0] if rows > 1 else 3 * cols, confidence)
        return out

    # -- the person detector (additive; HOG.md): the reference's HOGBox (src/hog_box.py:24-33) on the device -------------
    def set_hog_detector(self, detector):
        """The linear SVM of ``detect_people``: 3781 floats, rho last -- the array ``cv2.HOGDescriptor_getDefaultPeopleDetector()``
        returns, flattened -- or 3780 with rho 0.  Kept across a re-plan of the scales."""
        det = np.array(detector, dtype=np.float32).reshape(-1)
        self._h.hog_set_detector(det)
        self._hog_detector = det

    def detect_people(self, frame, detector=None, pixel_format="bgr", stream=None, orientation=None, **spec):
        """Additive (HOG.md): ``cv2.HOGDescriptor().detectMultiScale(frame)`` (src/hog_box.py:28) computed on the device by the rule of
        vnect_amd/csrc/hog.h -> (rects (n, 4) int32 [x, y, w, h] in the oriented picture's coordinates, weights (n,) float64).
        ``frame``: a host uint8 (H, W, 3) BGR array, or a frame in device memory as the estimator itself takes it (``pixel_format``
        "bgr", "rgb" or "nv12"; ``stream`` its producer).  ``detector``: set (and kept) before the call.  ``spec``: detectMultiScale's
        ``hit_threshold``, ``win_stride`` (x, y), ``scale0``, ``final_threshold``, ``nlevels``, and ``max_hits``."""
        if detector is not None:
            self.set_hog_detector(detector)
        sp = _native.hog_spec(**spec)
        device = _native.is_device_array(frame)
        self._format(pixel_format, None, device)
        if not device and pixel_format != "bgr":
            raise ValueError("detect_people takes a host frame as BGR; an NV12 frame is read in device memory")
        self._orient(orientation)
        if device:
            return self._h.hog_detect_device(_native.device_frame(frame, pixel_format), sp, stream)
        return self._h.hog_detect(frame, sp)

    def frame_buffer(self, height, width, index=0, pixel_format="bgr"):
        """Additive: a (height, width, 3) uint8 array in PINNED host memory (two exist, ``index`` 0 / 1).  Capture into it
        (``cap.read(buf)``, ``buf[...] = frame``) and pass it -- or a crop of it, as the tracking loop does -- to the estimator: the
        frame then crosses PCIe without the CPU copy a pageable array needs first.  ``pixel_format="nv12"``: the same buffer as a
        (height * 3 // 2, width) NV12 array (Y rows, then the U, V rows)."""
        if self._format(pixel_format, None):
            return self._h.frame_buffer_nv12(index, height, width)
        return self._h.frame_buffer(index, height, width)

    def reset(self):
        self._h.reset_filters()

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None

