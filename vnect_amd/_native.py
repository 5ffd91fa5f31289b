"""ctypes binding of libvnect_hip.so (include/vnect_abi.h).  No torch, no TensorFlow.

The library is the product path; there is no CPU fallback: if it is missing or no MI355X is
visible, loading / creating a handle raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VNECT_LIB") or os.path.join(_HERE, "lib", "libvnect_hip.so")  # VNECT_LIB: A/B tuning builds
_lib = None

MAX_SCALES = 8
OK, E_ARG, E_STATE, E_HIP, E_NODEVICE, E_TIMESTAMP, E_COMM, E_TIMEORDER, E_INTERNAL = 0, -1, -2, -3, -4, -5, -6, -7, -8
ABI_VERSION = 7
MAX_STREAMS = 4
XCHG_RCCL, XCHG_P2P = 0, 1
FP32, BF16, FP32_SPLIT, FP16 = 0, 1, 2, 3  # vnect_config::precision


class VnectError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libvnect_hip: %s (code %d)" % (msg, code))
        self.code = code


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("num_scales", C.c_int32),
                ("scales", C.c_double * MAX_SCALES), ("precision", C.c_int32), ("paper_res2c", C.c_int32),
                ("use_graph", C.c_int32), ("numpy_promotion", C.c_int32), ("max_frame_bytes", C.c_int32),
                ("num_frame_slots", C.c_int32), ("pyramid_nranks", C.c_int32), ("pyramid_rank", C.c_int32),
                ("keep_activations", C.c_int32), ("lanes", C.c_int32), ("preprocess_only", C.c_int32),
                ("exchange", C.c_int32)]


class Timings(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("frames", C.c_int32), ("total_ms", C.c_double), ("net_ms", C.c_double),
                ("conv_ms", C.c_double), ("conv_launches", C.c_int32), ("conv_flops", C.c_double), ("conv_slot_ms", C.c_double),
                ("shader_cycles", C.c_double), ("shader_ticks", C.c_double)]   # ABI v6: clock [MHz] = 100 * cycles / ticks


class LayerInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("tile_m", C.c_int32), ("tile_n", C.c_int32), ("split_k", C.c_int32), ("workgroups", C.c_int32),
                ("flops", C.c_double), ("last_ms", C.c_double)]


LOST_ACTIONS = {"off": 0, "hold": 1, "reset": 2}   # vnect_track_policy's action
PIX_BGR, PIX_RGB, PIX_NV12 = 0, 1, 2          # vnect_device_frame::format
STREAM_SYNCED = C.c_void_p(-1).value          # VNECT_STREAM_SYNCED: the caller has synchronised, wait for nothing


class DeviceFrame(C.Structure):
    """vnect_device_frame: a uint8 frame in device memory (include/vnect_abi.h; DEVICE_FRAMES.md)."""
    _fields_ = [("struct_size", C.c_int32), ("format", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("data", C.c_void_p),
                ("stride_y", C.c_int64), ("stride_x", C.c_int64), ("stride_c", C.c_int64), ("uv", C.c_void_p),
                ("uv_stride", C.c_int64), ("has_rect", C.c_int32), ("rect", C.c_int32 * 4)]


LIMB_BGR, RECT_BGR = (49, 22, 122), (60, 66, 207)   # the reference's colours (src/utils.py:236, 241)


class OverlayStyle(C.Structure):
    """vnect_overlay_style: colours, confidence threshold and parents of a draw (include/vnect_abi.h; OVERLAY.md)."""
    _fields_ = [("struct_size", C.c_int32), ("limb_bgr", C.c_int32 * 3), ("rect_bgr", C.c_int32 * 3), ("min_confidence", C.c_double),
                ("parents", C.c_int32 * 21), ("has_parents", C.c_int32)]


def _set_parents(s, parents):
    """parents (None: the reference's joint_parents stay) into the parents / has_parents fields of an OverlayStyle or a View3dSpec"""
    if parents is not None:
        parents = [int(v) for v in parents]
        if len(parents) != 21:
            raise ValueError("parents must name one joint for each of the 21 joints")
        s.has_parents = 1
        for k, v in enumerate(parents):
            s.parents[k] = v


def _out_pix(out_format):
    """the PIX_* code of a preview's or a view's out_format"""
    if out_format not in ("bgr", "rgb"):
        raise ValueError("out_format must be 'bgr' or 'rgb'")
    return PIX_RGB if out_format == "rgb" else PIX_BGR


def overlay_style(min_confidence=None, colors=None, parents=None):
    """The OverlayStyle of a draw.  min_confidence None: no threshold; colors: None, or (limb_bgr, rect_bgr) -- either may be None for the
    reference's; parents: None for the reference's joint_parents, or 21 joint indices."""
    s = OverlayStyle()
    s.struct_size = C.sizeof(OverlayStyle)
    limb, rect = (None, None) if colors is None else colors
    for k in range(3):
        s.limb_bgr[k] = int((LIMB_BGR if limb is None else limb)[k])
        s.rect_bgr[k] = int((RECT_BGR if rect is None else rect)[k])
    s.min_confidence = float("nan") if min_confidence is None else float(min_confidence)
    _set_parents(s, parents)
    return s


PREVIEW_MAX = 4096   # VNECT_PREVIEW_MAX: an output side of a preview at most


class PreviewSpec(C.Structure):
    """vnect_preview_spec: factor, output channel order and draw_frame of a preview (include/vnect_abi.h; PREVIEW.md)."""
    _fields_ = [("struct_size", C.c_int32), ("factor", C.c_double), ("out_format", C.c_int32), ("draw_frame", C.c_int32)]


def preview_spec(factor=None, out_format="bgr", draw_frame=False):
    """The PreviewSpec of a preview.  factor None (or 0): the reference's 1024 / the picture's longer side; out_format "bgr" or "rgb"."""
    out_format = _out_pix(out_format)
    s = PreviewSpec()
    s.struct_size = C.sizeof(PreviewSpec)
    s.factor = 0.0 if factor is None else float(factor)
    s.out_format = out_format
    s.draw_frame = int(bool(draw_frame))
    return s


VIEW3D_MAX = 2048   # VNECT_VIEW3D_MAX: rows and columns of a 3-D view at most


class View3dSpec(C.Structure):
    """vnect_view3d_spec: size, scale, view, line width, colours, parents, threshold, channel order and stacking order of a 3-D view; a zero
    field or a cleared has_* flag means its default (include/vnect_abi.h; VIEW3D.md)."""
    _fields_ = [("struct_size", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("extent", C.c_double), ("view", C.c_double * 9),
                ("has_view", C.c_int32), ("has_background", C.c_int32), ("line_width", C.c_double), ("background_bgr", C.c_int32 * 3),
                ("has_colors", C.c_int32), ("colors_bgr", (C.c_int32 * 3) * 21), ("parents", C.c_int32 * 21), ("has_parents", C.c_int32),
                ("min_confidence", C.c_double), ("out_format", C.c_int32), ("order", C.c_int32)]


def view3d_spec(size=400, view=None, extent=500.0, line_width=3.0, background=None, colors=None, parents=None, min_confidence=None,
                out_format="bgr", order=0):
    """The View3dSpec of a 3-D view.  size: rows = cols, or (rows, cols); view: None (the reference's view_init(-90, -90): the identity) or a
    3 x 3 matrix (render.view_matrix); background: None (white) or BGR; colors: None (matplotlib's cycle) or 21 BGR triples; parents: None
    for the reference's joint_parents; min_confidence None: no threshold; out_format "bgr" or "rgb"; order 0 (a higher limb index lies on
    top) or 1 (the nearer limb does)."""
    out_format = _out_pix(out_format)
    s = View3dSpec()
    s.struct_size = C.sizeof(View3dSpec)
    rows, cols = (size, size) if np.isscalar(size) else size
    s.rows, s.cols, s.extent, s.line_width = int(rows), int(cols), float(extent), float(line_width)
    # a zero means "the default" in the C structure: what the caller wrote as 0 where 0 is not the default must be refused, not replaced
    if s.rows == 0 or s.cols == 0 or s.extent == 0.0 or s.line_width == 0.0:
        raise ValueError("size, extent and line_width must not be 0")
    if view is not None:
        v = np.asarray(view, dtype=np.float64)
        if v.shape != (3, 3):
            raise ValueError("view must be a 3 x 3 matrix")
        s.has_view = 1
        for k, x in enumerate(v.reshape(-1)):
            s.view[k] = float(x)
    if background is not None:
        s.has_background = 1
        for k in range(3):
            s.background_bgr[k] = int(background[k])
    if colors is not None:
        c = np.asarray(colors)
        if c.shape != (21, 3):
            raise ValueError("colors must be 21 BGR triples")
        s.has_colors = 1
        for i in range(21):
            for k in range(3):
                s.colors_bgr[i][k] = int(c[i, k])
    _set_parents(s, parents)
    s.min_confidence = float("nan") if min_confidence is None else float(min_confidence)
    s.out_format = out_format
    s.order = int(order)
    return s


HOG_DETECTOR_SIZE, HOG_MAX_SIDE = 3781, 4096   # VNECT_HOG_DETECTOR_SIZE, VNECT_HOG_MAX_SIDE
HOG_TRACK_MAX_HITS = 4096                      # the hit budget of a re-detecting stream (vnect_track_redetect)
REDETECT_STATUS = {0: "not run", 1: "found", 2: "nobody", 3: "overflow"}   # vnect_result_redetect's status


class HogSpec(C.Structure):
    """vnect_hog_spec: detectMultiScale's parameters; a zero field means its default (include/vnect_abi.h; HOG.md)."""
    _fields_ = [("struct_size", C.c_int32), ("hit_threshold", C.c_double), ("win_stride_x", C.c_int32), ("win_stride_y", C.c_int32),
                ("scale0", C.c_double), ("final_threshold", C.c_double), ("nlevels", C.c_int32), ("max_hits", C.c_int32)]


def hog_spec(hit_threshold=0.0, win_stride=(8, 8), scale0=1.05, final_threshold=2.0, nlevels=64, max_hits=65536):
    """The HogSpec of a detection, cv2.HOGDescriptor.detectMultiScale's names and defaults (win_stride is (x, y))."""
    s = HogSpec()
    s.struct_size = C.sizeof(HogSpec)
    s.hit_threshold, s.scale0, s.final_threshold = float(hit_threshold), float(scale0), float(final_threshold)
    s.win_stride_x, s.win_stride_y = int(win_stride[0]), int(win_stride[1])
    s.nlevels, s.max_hits = int(nlevels), int(max_hits)
    # a zero means "the default" in the C structure: what the caller wrote as 0 where 0 is not the default must be refused, not replaced
    if s.win_stride_x == 0 or s.win_stride_y == 0 or s.scale0 == 0.0 or s.nlevels == 0 or s.max_hits == 0:
        raise ValueError("win_stride, scale0, nlevels and max_hits must not be 0")
    if s.final_threshold == 0.0:
        s.final_threshold = 0.5   # (below 1: the hits ungrouped, as 0 means in cv2)
    return s


class DeviceFrameError(VnectError, ValueError):
    """VNECT_E_ARG of a device-frame entry point: the frame as given cannot be read (a ValueError, like every refused argument)."""


# every symbol include/vnect_abi.h declares: name -> (restype, argtypes)
_f32p, _f64p, _u8p, _i32p = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int32))
_H = C.c_void_p
SYMBOLS = {
    "vnect_abi_version": (C.c_int, []),
    "vnect_build_info": (C.c_char_p, []),
    "vnect_create": (C.c_int, [C.POINTER(Config), C.POINTER(_H)]),
    "vnect_destroy": (None, [_H]),
    "vnect_last_error": (C.c_char_p, [_H]),
    "vnect_set_weight": (C.c_int, [_H, C.c_char_p, _f32p, C.POINTER(C.c_int64), C.c_int]),
    "vnect_finalize": (C.c_int, [_H]),
    "vnect_set_scales": (C.c_int, [_H, _f64p, C.c_int]),
    "vnect_forward": (C.c_int, [_H, _f32p, C.c_int, _f32p]),
    "vnect_preprocess": (C.c_int, [_H, _u8p, C.c_int, C.c_int, C.c_int64, _f32p, _f64p, _i32p, _i32p]),
    "vnect_postprocess": (C.c_int, [_H, _f32p, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, _f64p, _f32p]),
    "vnect_infer": (C.c_int, [_H, _u8p, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_double, _f64p, _f32p]),
    "vnect_frame_buffer": (C.c_int, [_H, C.c_int, C.c_int64, C.POINTER(_u8p)]),
    "vnect_upload_frame": (C.c_int, [_H, C.c_int, _u8p, C.c_int, C.c_int, C.c_int64]),
    "vnect_infer_resident": (C.c_int, [_H, C.c_int, C.c_double, C.c_double, _f64p, _f32p]),
    "vnect_submit_resident": (C.c_int, [_H, C.c_int, C.c_double, C.c_double]),
    "vnect_collect": (C.c_int, [_H, _f64p, _f32p]),
    "vnect_submit_stream": (C.c_int, [_H, C.c_int, C.c_int, C.c_double, C.c_double]),
    "vnect_collect_stream": (C.c_int, [_H, _i32p, _f64p, _f32p]),
    "vnect_reset_filters_stream": (C.c_int, [_H, C.c_int]),
    "vnect_set_stream_batch": (C.c_int, [_H, C.c_int]),
    "vnect_submit_streams": (C.c_int, [_H, C.c_int, _i32p, _i32p, _f64p, _f64p]),
    "vnect_get_batch_layer_info": (C.c_int, [_H, C.c_int, C.POINTER(LayerInfo)]),
    "vnect_joint_filter": (C.c_int, [_H, C.c_int, _f64p, C.c_int, C.c_double, _f64p]),
    "vnect_reset_filters": (C.c_int, [_H]),
    "vnect_read_activation": (C.c_int, [_H, C.c_char_p, _f32p, C.c_int64, _i32p]),
    "vnect_set_profiling": (C.c_int, [_H, C.c_int]),
    "vnect_get_timings": (C.c_int, [_H, C.POINTER(Timings)]),
    "vnect_reset_timings": (C.c_int, [_H]),
    "vnect_get_layer_info": (C.c_int, [_H, C.c_int, C.POINTER(LayerInfo)]),
    "vnect_get_layer_rows": (C.c_int, [_H, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vnect_get_layer_stamps": (C.c_int, [_H, C.c_int, C.POINTER(C.c_uint64)]),
    "vnect_comm_unique_id": (C.c_int, [C.c_void_p]),
    "vnect_comm_init": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p]),
    "vnect_comm_library": (C.c_int, [C.c_char_p, C.c_int, _i32p]),
    "vnect_comm_p2p_export": (C.c_int, [_H, C.c_void_p]),
    "vnect_comm_p2p_init": (C.c_int, [_H, C.c_int, C.c_int, C.c_void_p]),
    "vnect_track_begin": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _i32p]),
    "vnect_submit_tracked": (C.c_int, [_H, C.c_int, C.c_int, C.c_double, C.c_double]),
    "vnect_submit_tracked_pinned": (C.c_int, [_H, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_double]),
    "vnect_collect_tracked": (C.c_int, [_H, _i32p, _f64p, _f32p, _i32p]),
    "vnect_track_box": (C.c_int, [_H, C.c_int, _i32p]),
    "vnect_result_confidence": (C.c_int, [_H, _f64p, _i32p]),
    "vnect_track_policy": (C.c_int, [_H, C.c_int, C.c_double, C.c_int, C.c_int]),
    "vnect_upload_frame_nv12": (C.c_int, [_H, C.c_int, _u8p, C.c_int64, _u8p, C.c_int64, C.c_int, C.c_int]),
    "vnect_upload_frame_nv12_rect": (C.c_int, [_H, C.c_int, _u8p, C.c_int64, _u8p, C.c_int64, C.c_int, C.c_int, _i32p]),
    "vnect_infer_nv12": (C.c_int, [_H, _u8p, C.c_int64, _u8p, C.c_int64, C.c_int, C.c_int, _i32p, C.c_double, C.c_double, _f64p, _f32p]),
    "vnect_preprocess_nv12": (C.c_int, [_H, _u8p, C.c_int64, _u8p, C.c_int64, C.c_int, C.c_int, _i32p, _f32p, _f64p, _i32p, _i32p]),
    "vnect_submit_tracked_pinned_nv12": (C.c_int, [_H, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double]),
    "vnect_read_frame": (C.c_int, [_H, C.c_int, _u8p, C.c_int64, _i32p]),
    "vnect_upload_frame_device": (C.c_int, [_H, C.c_int, C.POINTER(DeviceFrame), C.c_void_p]),
    "vnect_infer_device": (C.c_int, [_H, C.POINTER(DeviceFrame), C.c_void_p, C.c_double, C.c_double, _f64p, _f32p]),
    "vnect_preprocess_device": (C.c_int, [_H, C.POINTER(DeviceFrame), C.c_void_p, _f32p, _f64p, _i32p, _i32p]),
    "vnect_submit_tracked_device": (C.c_int, [_H, C.c_int, C.POINTER(DeviceFrame), C.c_void_p, C.c_double, C.c_double]),
    "vnect_draw_device": (C.c_int, [_H, C.POINTER(DeviceFrame), C.c_void_p, _f64p, _f64p, _i32p, C.POINTER(OverlayStyle)]),
    "vnect_submit_tracked_device_draw": (C.c_int, [_H, C.c_int, C.POINTER(DeviceFrame), C.c_void_p, C.c_double, C.c_double,
                                                   C.POINTER(OverlayStyle)]),
    "vnect_set_orientation": (C.c_int, [_H, C.c_int]),
    "vnect_preview_size": (C.c_int, [_H, C.POINTER(DeviceFrame), C.POINTER(PreviewSpec), _i32p]),
    "vnect_preview_device": (C.c_int, [_H, C.POINTER(DeviceFrame), C.c_void_p, _f64p, _f64p, _i32p, C.POINTER(OverlayStyle),
                                       C.POINTER(PreviewSpec), C.c_void_p, C.c_int64]),
    "vnect_submit_tracked_device_preview": (C.c_int, [_H, C.c_int, C.POINTER(DeviceFrame), C.c_void_p, C.c_double, C.c_double,
                                                      C.POINTER(OverlayStyle), C.POINTER(PreviewSpec)]),
    "vnect_result_preview": (C.c_int, [_H, C.POINTER(_u8p), _i32p, C.POINTER(C.c_int64)]),
    "vnect_view3d_device": (C.c_int, [_H, _f32p, _f64p, C.POINTER(View3dSpec), C.c_void_p, C.c_int64]),
    "vnect_track_view3d": (C.c_int, [_H, C.c_int, C.POINTER(View3dSpec)]),
    "vnect_result_view3d": (C.c_int, [_H, C.POINTER(_u8p), _i32p, C.POINTER(C.c_int64)]),
    "vnect_hog_set_detector": (C.c_int, [_H, _f32p, C.c_int]),
    "vnect_hog_levels": (C.c_int, [_H, C.POINTER(DeviceFrame), C.POINTER(HogSpec), _i32p, _i32p, _f64p, C.c_int]),
    "vnect_hog_detect_device": (C.c_int, [_H, C.POINTER(DeviceFrame), C.c_void_p, C.POINTER(HogSpec), _i32p, _f64p, C.c_int, _i32p]),
    "vnect_hog_detect": (C.c_int, [_H, _u8p, C.c_int, C.c_int, C.c_int64, C.POINTER(HogSpec), _i32p, _f64p, C.c_int, _i32p]),
    "vnect_track_redetect": (C.c_int, [_H, C.c_int, C.POINTER(HogSpec), C.c_int]),
    "vnect_result_redetect": (C.c_int, [_H, _i32p, _i32p, _i32p]),
    "vnect_set_people": (C.c_int, [_H, C.c_int, C.c_int]),
    "vnect_people_begin": (C.c_int, [_H, C.c_int, C.c_int, C.c_int, _i32p]),
    "vnect_submit_people": (C.c_int, [_H, C.c_int, C.c_int, C.c_double, C.c_double]),
    "vnect_submit_people_device": (C.c_int, [_H, C.c_int, C.POINTER(DeviceFrame), C.c_void_p, C.c_double, C.c_double,
                                             C.POINTER(OverlayStyle), C.POINTER(PreviewSpec)]),
    "vnect_result_people": (C.c_int, [_H, _i32p, _i32p]),
}


TESTHOOKS_LIB = os.path.join(_HERE, "lib", "libvnect_hip_testhooks.so")   # the host runtime with -DVNECT_TEST_HOOKS=1 (tests only)


TRACKPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_trackprobe.so")     # track.o + post.o behind csrc/track_probe.cpp (tests only)


NV12PROBE_LIB = os.path.join(_HERE, "lib", "libvnect_nv12probe.so")       # post.o + track.o behind csrc/nv12_probe.cpp (tests only)
NV12_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_nv12.so")             # g++'s build of csrc/nv12.h (tests only; no GPU code)
INGESTPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_ingestprobe.so")   # post.o + track.o behind csrc/ingest_probe.hip (tests only)
INGEST_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_ingest.so")         # g++'s build of csrc/ingest.h (tests only; no GPU code)
OVERLAYPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_overlayprobe.so") # overlay.o behind csrc/overlay_probe.hip (tests only)
OVERLAY_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_overlay.so")       # g++'s build of csrc/overlay.h (tests only; no GPU code)
ORIENTPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_orientprobe.so")   # orient.o behind csrc/orient_probe.hip (tests only)
ORIENT_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_orient.so")         # g++'s build of csrc/orient.h (tests only; no GPU code)
PREVIEWPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_previewprobe.so") # preview.o behind csrc/preview_probe.hip (tests only)
PREVIEW_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_preview.so")       # g++'s build of csrc/preview.h (tests only; no GPU code)
HOGPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_hogprobe.so")         # hog.o behind csrc/hog_probe.hip (tests only)
REDETECTPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_redetectprobe.so")  # hog.o behind csrc/redetect_probe.hip (tests only)
HOG_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_hog.so")               # g++'s build of csrc/hog.h (tests only; no GPU code)
VIEW3DPROBE_LIB = os.path.join(_HERE, "lib", "libvnect_view3dprobe.so")   # view3d.o behind csrc/view3d_probe.hip (tests only)
VIEW3D_CPU_LIB = os.path.join(_HERE, "lib", "libvnect_view3d.so")         # g++'s build of csrc/view3d.h (tests only; no GPU code)


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the library (works without a GPU), and of its test twins: the same kernel objects under a
    host runtime compiled with the test hooks (`make testhooks`; tests/test_gpu_surface.py, tests/test_gpu_track_maps.py), and the
    kernels' objects behind probe shims (`make trackprobe` ...; tests/test_gpu_*_kernels.py).  The product loads none of them."""
    src = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", src] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    # the test-hooks twin, the nine kernel probes and g++'s builds of the kernels' headers: the tables of csrc/Makefile behind `make tests`
    subprocess.check_call(["make", "-C", src, "tests"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def build_info():
    """vnect_build_info() as a dict: {"abi": "6", "compiler": ..., "flags": ..., "variant": "", "test_hooks": "0", "probes_off": "1",
    "conv": "X3_DBG=0 ...", "post": "..."}."""
    text = lib().vnect_build_info().decode()
    out = {"text": text}
    for part in text.split("; "):
        if ": " in part and "=" not in part.split(": ", 1)[0]:
            k, v = part.split(": ", 1)
        else:
            k, v = part.split("=", 1)
        out[k.strip()] = v.strip()
    return out


def lib():
    """Load the library; raises if it has not been built (there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libvnect_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(needs hipcc); the VNect path has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the ABI and the header drift apart
            fn.restype, fn.argtypes = res, args
        if L.vnect_abi_version() != ABI_VERSION:
            raise ImportError("libvnect_hip.so ABI version mismatch")
        _lib = L
    return _lib


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _joints_out():
    """fresh (joints_2d (21, 2) float64, joints_3d (21, 3) float32) for the library to fill"""
    return np.empty((21, 2), np.float64), np.empty((21, 3), np.float32)


def _fixed(a, dtype, shape, name, optional=False):
    """a per-joint argument as a contiguous `dtype` array, which must have `shape`; an optional one may be None and stays None"""
    if a is None and optional:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != shape:
        raise ValueError("%s must be %s" % (name, str(shape)))
    return a


def _rect4(rect):
    """rect (x, y, w, h) or None -> the const int32_t* argument (ctypes keeps the array alive for the call)"""
    return None if rect is None else _ptr(np.asarray([int(v) for v in rect], np.int32), _i32p)


class Handle:
    """Thin RAII wrapper over vnect_handle; every method maps 1:1 to a C entry point."""

    def __init__(self, scales, device=0, precision=FP32, paper_res2c=False, use_graph="auto", numpy_promotion=0,
                 max_frame_bytes=0, num_frame_slots=0, pyramid=None, keep_activations=False, lanes=1,
                 preprocess_only=False, exchange=XCHG_RCCL, stream_batch=1, people=0, pair=False):
        L = lib()
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.device = device
        cfg.num_scales = len(scales)
        for i, s in enumerate(scales):
            cfg.scales[i] = float(s)
        # use_graph: False = eager launches, True = always replay the frame graph, "auto" = eager for a synchronous frame,
        # graph replay when frames are in flight (the default)
        cfg.precision, cfg.paper_res2c, cfg.use_graph = precision, int(paper_res2c), (2 if use_graph == "auto" else int(bool(use_graph)))
        cfg.numpy_promotion, cfg.max_frame_bytes, cfg.num_frame_slots = numpy_promotion, max_frame_bytes, num_frame_slots
        cfg.lanes = int(lanes)  # 2: submit_resident/collect overlap two frames on two lanes
        cfg.keep_activations = int(keep_activations)  # True: activation(name) can return inner layers (tests)
        cfg.preprocess_only = int(preprocess_only)    # gen_input_batch only: no weights, no launch plan
        cfg.exchange = int(exchange)                  # pyramid sharding: XCHG_RCCL (ncclAllGather) or XCHG_P2P (peer writes)
        if pyramid is not None:  # (rank, nranks): this handle runs one scale of the pyramid (vnect_comm_init)
            cfg.pyramid_rank, cfg.pyramid_nranks = int(pyramid[0]), int(pyramid[1])
        h = _H()
        rc = L.vnect_create(C.byref(cfg), C.byref(h))
        self._h = h if h.value else None
        self.num_scales = len(scales)
        self.orientation = 0  # the code the handle holds (set_orientation keeps it: the C ABI has no getter)
        self.net_images = 1 if pyramid is not None else len(scales)
        if rc:
            msg = L.vnect_last_error(self._h).decode()
            self.close()
            raise VnectError(rc, msg)
        self.stream_batch = int(stream_batch)  # 2: finalize also builds the batched plan of two streams (submit_streams)
        if self.stream_batch != 1:
            self.set_stream_batch(self.stream_batch)
        self.people = 0          # P > 0: people mode -- persons 0 .. P-1 of one video on streams 0 .. P-1 (set_people; PEOPLE.md)
        if people:
            self.set_people(people, pair)

    def set_people(self, n, pair=False):
        """vnect_set_people: people mode for n persons (before finalize); pair: two persons' crops share one conv stack where 2 S <= 8."""
        self._ck(lib().vnect_set_people(self._h, int(n), int(bool(pair))))
        self.people, self.pair_people = int(n), bool(pair)

    def people_begin(self, n, H, W, rects=None):
        """vnect_people_begin: persons 0 .. n-1 track (H, W) frames from now on, person p from rects[p] (x, y, w, h); None: the whole frame."""
        r = None
        if rects is not None:
            r = np.asarray([[int(v) for v in rect] for rect in rects], np.int32)
            if r.shape != (int(n), 4):
                raise ValueError("rects must hold n rects (x, y, w, h)")
        self._ck(lib().vnect_people_begin(self._h, int(n), int(H), int(W), None if r is None else _ptr(r, _i32p)))

    def submit_people(self, n, slot, t2d, t3d):
        """vnect_submit_people: the next frame for persons 0 .. n-1, the whole frame in resident slot `slot`; n collect_tracked() deliveries."""
        self._ck(lib().vnect_submit_people(self._h, int(n), int(slot), t2d, t3d))

    def submit_people_device(self, n, frame, t2d, t3d, producer=None, style=None, spec=None):
        """vnect_submit_people_device: the same from device memory (`frame`: a DeviceFrame without a rect, kept alive and untouched until the
        last person has been collected); style: every person is drawn into the frame, in person order, once every crop has been read."""
        self._ck_device(lib().vnect_submit_people_device(self._h, int(n), C.byref(frame), _stream_arg(producer), t2d, t3d,
                                                         None if style is None else C.byref(style), None if spec is None else C.byref(spec)))

    def result_people(self):
        """vnect_result_people: (lane units, paired units) of the people frame submitted last."""
        u, p = C.c_int32(0), C.c_int32(0)
        self._ck(lib().vnect_result_people(self._h, C.byref(u), C.byref(p)))
        return int(u.value), int(p.value)

    def set_stream_batch(self, n):
        """vnect_set_stream_batch: 2 = two video streams' frames per launch (before finalize)."""
        self._ck(lib().vnect_set_stream_batch(self._h, int(n)))
        self.stream_batch = int(n)

    def close(self):
        if getattr(self, "_h", None):
            lib().vnect_destroy(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc):
        if rc:
            raise VnectError(rc, lib().vnect_last_error(self._h).decode())

    def set_weights(self, weights):
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shp = (C.c_int64 * a.ndim)(*a.shape)
            self._ck(lib().vnect_set_weight(self._h, name.encode(), _ptr(a, _f32p), shp, a.ndim))

    def finalize(self):
        self._ck(lib().vnect_finalize(self._h))

    def set_scales(self, scales):
        sc = np.asarray(scales, np.float64)
        self._ck(lib().vnect_set_scales(self._h, _ptr(sc, _f64p), len(sc)))

    def forward(self, batch):
        """(S,368,368,3) -> (S,46,46,84); on a stream_batch=2 handle also (2S,368,368,3), run on the batched plan."""
        batch = np.ascontiguousarray(batch, dtype=np.float32)
        n = batch.shape[0] if batch.ndim == 4 else -1
        if batch.shape[1:] != (368, 368, 3) or (n != self.net_images and not (self.stream_batch == 2 and n == 2 * self.net_images)):
            raise ValueError("batch must be (%d,368,368,3)" % self.net_images)
        out = np.empty((n, 46, 46, 84), np.float32)
        self._ck(lib().vnect_forward(self._h, _ptr(batch, _f32p), n, _ptr(out, _f32p)))
        return out

    def _preprocessed(self, ck, fn, *args, want_batch=True):
        """fn(handle, *args, batch_out, scaler, offset_x, offset_y), checked by ck -> (batch or None, scaler, [offset_x, offset_y])"""
        batch = np.empty((self.net_images, 368, 368, 3), np.float32) if want_batch else None
        scaler, ox, oy = C.c_double(), C.c_int32(), C.c_int32()
        ck(fn(self._h, *args, _ptr(batch, _f32p) if want_batch else None, C.byref(scaler), C.byref(ox), C.byref(oy)))
        return batch, scaler.value, [ox.value, oy.value]

    def preprocess(self, img, want_batch=True):
        img = _as_frame(img)
        H, W = img.shape[:2]
        return self._preprocessed(self._ck, lib().vnect_preprocess, _ptr(img, _u8p), H, W, img.strides[0], want_batch=want_batch)

    def postprocess(self, maps, t2d, t3d, scaler=1.0, offset_x=0, offset_y=0):
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        if maps.shape != (self.num_scales, 46, 46, 84):
            raise ValueError("maps must be (%d,46,46,84)" % self.num_scales)
        j2, j3 = _joints_out()
        self._ck(lib().vnect_postprocess(self._h, _ptr(maps, _f32p), t2d, t3d, scaler, offset_x, offset_y,
                                         _ptr(j2, _f64p), _ptr(j3, _f32p)))
        return j2, j3

    def infer(self, img, t2d, t3d):
        img = _as_frame(img)
        H, W = img.shape[:2]
        j2, j3 = _joints_out()
        self._ck(lib().vnect_infer(self._h, _ptr(img, _u8p), H, W, img.strides[0], t2d, t3d, _ptr(j2, _f64p),
                                   _ptr(j3, _f32p)))
        return j2, j3

    def frame_buffer(self, index, H, W):
        """(H, W, 3) uint8 array over the handle's pinned staging buffer `index` (0 / 1): frames captured into it -- or crops of them --
        go to the device without a CPU copy when passed to infer().  Valid until a larger request for the same index or close()."""
        p = _u8p()
        self._ck(lib().vnect_frame_buffer(self._h, index, H * W * 3, C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(H, W, 3))

    def upload_frame(self, slot, img, pixel_format="bgr", rect=None, stream=None):
        if is_device_array(img):  # a frame in device memory (DEVICE_FRAMES.md): the other three arguments are for it alone
            return self.upload_frame_device(slot, device_frame(img, pixel_format, rect), stream)
        if pixel_format != "bgr" or rect is not None or stream is not None:
            raise ValueError("pixel_format=, rect= and stream= are for frames in device memory")
        img = _as_frame(img)
        H, W = img.shape[:2]
        self._ck(lib().vnect_upload_frame(self._h, slot, _ptr(img, _u8p), H, W, img.strides[0]))

    # The per-frame calls sit between two frames of a synchronous stream (the GPU idles meanwhile): they hand the library
    # one pair of result buffers whose ctypes pointers are made once, and return fresh copies as the reference does.
    def _results(self):
        if getattr(self, "_res", None) is None:
            j2, j3 = _joints_out()
            self._res = (j2, j3, _ptr(j2, _f64p), _ptr(j3, _f32p), lib().vnect_infer_resident, lib().vnect_collect)
        return self._res

    def infer_resident(self, slot, t2d, t3d):
        j2, j3, p2, p3, fn, _ = self._results()
        rc = fn(self._h, slot, t2d, t3d, p2, p3)
        if rc:
            self._ck(rc)
        return j2.copy(), j3.copy()

    def submit_resident(self, slot, t2d, t3d):
        self._ck(lib().vnect_submit_resident(self._h, slot, t2d, t3d))

    def collect(self):
        j2, j3, p2, p3, _, fn = self._results()
        rc = fn(self._h, p2, p3)
        if rc:
            self._ck(rc)
        return j2.copy(), j3.copy()

    def submit_stream(self, stream, slot, t2d, t3d):
        """One frame of video stream `stream` (its own filter bank and timestamps on this handle): frames of different streams
        overlap on the handle's lanes with no dependency between them."""
        self._ck(lib().vnect_submit_stream(self._h, stream, slot, t2d, t3d))

    def collect_stream(self):
        """(stream, joints_2d, joints_3d) of the oldest frame in flight."""
        j2, j3, p2, p3, _, _ = self._results()
        s = C.c_int32(-1)
        rc = lib().vnect_collect_stream(self._h, C.byref(s), p2, p3)
        if rc:
            self._ck(rc)
        return s.value, j2.copy(), j3.copy()

    def submit_streams(self, streams, slots, t2d, t3d):
        """Frames of DISTINCT streams from resident slots as one batch (two: the batched plan; one: submit_stream).  Their results come
        back through collect_stream, one per frame, in this order.  Refused as a whole, with no state changed, if any check fails."""
        n = len(streams)
        if not (len(slots) == len(t2d) == len(t3d) == n):
            raise ValueError("streams, slots, t2d and t3d must have the same length")
        st, sl = np.asarray(streams, np.int32), np.asarray(slots, np.int32)
        a2, a3 = np.asarray(t2d, np.float64), np.asarray(t3d, np.float64)
        self._ck(lib().vnect_submit_streams(self._h, n, _ptr(st, _i32p), _ptr(sl, _i32p), _ptr(a2, _f64p), _ptr(a3, _f64p)))

    def infer_streams(self, frames, t2d, t3d, streams=(0, 1), slots=(0, 1)):
        """Synchronous convenience: uploads frames[k] into slots[k], submits them as one batch of `streams` and collects
        -> [(joints_2d, joints_3d) per frame]."""
        for slot, img in zip(slots, frames):
            self.upload_frame(slot, img)
        self.submit_streams(list(streams)[:len(frames)], list(slots)[:len(frames)], t2d, t3d)
        return [self.collect_stream()[1:] for _ in frames]

    # -- tracking on the device (vnect_track_begin ...): runner.track's crop box kept on the GPU -------------------------------------
    def track_begin(self, stream, H, W, rect=None):
        """Stream `stream` tracks (H, W) frames from now on, starting at rect (x, y, w, h); None: the whole frame."""
        self._ck(lib().vnect_track_begin(self._h, stream, int(H), int(W), _rect4(rect)))

    def submit_tracked(self, stream, slot, t2d, t3d):
        """The stream's next frame, the whole frame in resident slot `slot`; the device crops it with the stream's box."""
        self._ck(lib().vnect_submit_tracked(self._h, stream, slot, t2d, t3d))

    def submit_tracked_pinned(self, stream, index, row_stride, t2d, t3d):
        """The stream's next frame, the whole frame in pinned buffer `index` (frame_buffer): only the crop's rows cross PCIe."""
        self._ck(lib().vnect_submit_tracked_pinned(self._h, stream, index, int(row_stride), t2d, t3d))

    def collect_tracked(self):
        """(stream, joints_2d in frame coordinates, joints_3d, rect_used) of the oldest frame in flight (rect_used [-1] * 4: untracked)."""
        j2, j3, p2, p3, _, _ = self._results()
        s, r = C.c_int32(-1), (C.c_int32 * 4)()
        rc = lib().vnect_collect_tracked(self._h, C.byref(s), p2, p3, r)
        if rc:
            self._ck(rc)
        return s.value, j2.copy(), j3.copy(), list(r)

    def track_box(self, stream):
        """The rect (x, y, w, h) the stream's next tracked frame will be cropped with."""
        r = (C.c_int32 * 4)()
        self._ck(lib().vnect_track_box(self._h, stream, r))
        return list(r)

    # -- per-joint confidence and the loss rule (include/vnect_abi.h; CONFIDENCE.md) ---------------------------------------------------
    def result_confidence(self):
        """((21,) float64 confidences, lost flag) of the frame most recently delivered on this handle (a fresh array)."""
        conf, lost = np.empty(21, np.float64), C.c_int32(0)
        self._ck(lib().vnect_result_confidence(self._h, _ptr(conf, _f64p), C.byref(lost)))
        return conf, int(lost.value)

    def set_orientation(self, orientation):
        """vnect_set_orientation: how the frames submitted from now on are stored -- code 0 .. 7, the picture is np.rot90(frame, code & 3),
        mirrored when code & 4 (ORIENTATION.md)"""
        self._ck(lib().vnect_set_orientation(self._h, int(orientation)))
        self.orientation = int(orientation)

    def track_policy(self, stream, min_confidence, min_joints, action):
        """The stream's loss rule: action 0 / "off", 1 / "hold", 2 / "reset" (LOST_ACTIONS)."""
        self._ck(lib().vnect_track_policy(self._h, int(stream), float(min_confidence), int(min_joints), int(LOST_ACTIONS.get(action, action))))

    # -- NV12 frames: converted to BGR on the device, inside the frame's copy (include/vnect_abi.h; NV12.md) --------------------------
    def frame_buffer_nv12(self, index, H, W):
        """(H * 3 // 2, W) uint8 array over pinned staging buffer `index`: the contiguous NV12 layout -- H rows of Y, then H / 2 rows of
        interleaved U, V directly behind, all W bytes apart.  Pass it (or a row-strided view) to the *_nv12 methods: read in place."""
        if H % 2 or W % 2:
            raise ValueError("an NV12 frame needs even H and W")
        p = _u8p()
        self._ck(lib().vnect_frame_buffer(self._h, index, H * W * 3 // 2, C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(H * 3 // 2, W))

    def upload_frame_nv12(self, slot, nv12, rect=None):
        """The converted frame -- or, with rect (x, y, w, h), its crop, cut on the device -- into resident slot `slot`."""
        y, ys, uv, uvs, H, W = _as_nv12(nv12)
        if rect is None:
            self._ck(lib().vnect_upload_frame_nv12(self._h, slot, y, ys, uv, uvs, H, W))
        else:
            self._ck(lib().vnect_upload_frame_nv12_rect(self._h, slot, y, ys, uv, uvs, H, W, _rect4(rect)))

    def infer_nv12(self, nv12, t2d, t3d, rect=None):
        y, ys, uv, uvs, H, W = _as_nv12(nv12)
        j2, j3 = _joints_out()
        self._ck(lib().vnect_infer_nv12(self._h, y, ys, uv, uvs, H, W, _rect4(rect), t2d, t3d, _ptr(j2, _f64p), _ptr(j3, _f32p)))
        return j2, j3

    def preprocess_nv12(self, nv12, rect=None, want_batch=True):
        y, ys, uv, uvs, H, W = _as_nv12(nv12)
        return self._preprocessed(self._ck, lib().vnect_preprocess_nv12, y, ys, uv, uvs, H, W, _rect4(rect), want_batch=want_batch)

    def submit_tracked_pinned_nv12(self, stream, index, y_stride, uv_offset, uv_stride, t2d, t3d):
        """The stream's next frame, the whole NV12 frame in pinned buffer `index` (Y plane at its start, UV plane `uv_offset` bytes in)."""
        self._ck(lib().vnect_submit_tracked_pinned_nv12(self._h, stream, index, int(y_stride), int(uv_offset), int(uv_stride), t2d, t3d))

    # -- frames in device memory: written into the slot by a kernel (include/vnect_abi.h; DEVICE_FRAMES.md) --------------------------
    def _ck_device(self, rc):
        if rc == E_ARG:
            raise DeviceFrameError(rc, lib().vnect_last_error(self._h).decode() + _runtime_hint())
        self._ck(rc)

    def upload_frame_device(self, slot, frame, stream=None):
        """`frame`: a DeviceFrame (device_frame()).  Done with the caller's buffer on return."""
        self._ck_device(lib().vnect_upload_frame_device(self._h, slot, C.byref(frame), _stream_arg(stream)))

    def infer_device(self, frame, t2d, t3d, stream=None):
        j2, j3 = _joints_out()
        self._ck_device(lib().vnect_infer_device(self._h, C.byref(frame), _stream_arg(stream), t2d, t3d, _ptr(j2, _f64p), _ptr(j3, _f32p)))
        return j2, j3

    def preprocess_device(self, frame, stream=None, want_batch=True):
        return self._preprocessed(self._ck_device, lib().vnect_preprocess_device, C.byref(frame), _stream_arg(stream), want_batch=want_batch)

    def submit_tracked_device(self, stream, frame, t2d, t3d, producer=None):
        """The stream's next frame, the whole frame in device memory (`frame`: a DeviceFrame without a rect).  The buffer is read when the
        frame runs: keep it alive and untouched until the frame has been collected."""
        self._ck_device(lib().vnect_submit_tracked_device(self._h, stream, C.byref(frame), _stream_arg(producer), t2d, t3d))

    # -- the overlay: skeleton and crop rectangle drawn into a frame in device memory (include/vnect_abi.h; OVERLAY.md) -------------------
    def draw_device(self, frame, joints_2d, rect=None, confidence=None, style=None, stream=None):
        """vnect_draw_device: draws into `frame` (a DeviceFrame without a rect); done on return."""
        j2 = _fixed(joints_2d, np.float64, (21, 2), "joints_2d")
        cf = _fixed(confidence, np.float64, (21,), "confidence", optional=True)
        self._ck_device(lib().vnect_draw_device(self._h, C.byref(frame), _stream_arg(stream), _ptr(j2, _f64p), _ptr(cf, _f64p), _rect4(rect),
                                                None if style is None else C.byref(style)))

    def submit_tracked_device_draw(self, stream, frame, t2d, t3d, producer=None, style=None):
        """submit_tracked_device, and the frame is annotated in place with its own joints and crop rect by the time it is collected: the
        buffer is WRITTEN until then."""
        self._ck_device(lib().vnect_submit_tracked_device_draw(self._h, stream, C.byref(frame), _stream_arg(producer), t2d, t3d,
                                                               None if style is None else C.byref(style)))

    # -- the preview: the annotated frame scaled for display, computed on the device (include/vnect_abi.h; PREVIEW.md) ------------------
    def preview_size(self, frame, spec):
        """vnect_preview_size: (rows, columns) of the preview of `frame` (a DeviceFrame; only its H and W count) under the orientation in force."""
        hw = (C.c_int32 * 2)()
        self._ck_device(lib().vnect_preview_size(self._h, C.byref(frame), C.byref(spec), hw))
        return int(hw[0]), int(hw[1])

    def preview_device(self, frame, spec, out, out_pitch, joints_2d=None, rect=None, confidence=None, style=None, stream=None):
        """vnect_preview_device: the preview of `frame` (a DeviceFrame without a rect) into the memory at address `out` (device or host),
        rows out_pitch bytes apart; done on return.  The frame is not written."""
        j2 = _fixed(joints_2d, np.float64, (21, 2), "joints_2d", optional=True)
        cf = _fixed(confidence, np.float64, (21,), "confidence", optional=True)
        self._ck_device(lib().vnect_preview_device(self._h, C.byref(frame), _stream_arg(stream), _ptr(j2, _f64p), _ptr(cf, _f64p), _rect4(rect),
                                                   None if style is None else C.byref(style), C.byref(spec), C.c_void_p(int(out)), int(out_pitch)))

    def submit_tracked_device_preview(self, stream, frame, t2d, t3d, producer=None, style=None, spec=None):
        """submit_tracked_device, and the frame's preview (annotated with its own joints and crop rect, scaled) is computed on the device
        and delivered with it: result_preview() after collect_tracked().  spec.draw_frame: the frame is annotated in place too."""
        spec = preview_spec() if spec is None else spec
        self._ck_device(lib().vnect_submit_tracked_device_preview(self._h, stream, C.byref(frame), _stream_arg(producer), t2d, t3d,
                                                                  None if style is None else C.byref(style), C.byref(spec)))

    def _result_picture(self, fn):
        """fn(handle, data, rows and columns, pitch): the (rows, columns, 3) picture of the frame delivered last as a fresh array, or None"""
        data, hw, pitch = _u8p(), (C.c_int32 * 2)(), C.c_int64()
        self._ck(fn(self._h, C.byref(data), hw, C.byref(pitch)))
        if hw[0] < 1 or hw[1] < 1:
            return None
        return np.ctypeslib.as_array(data, shape=(hw[0], hw[1] * 3)).reshape(hw[0], hw[1], 3).copy()

    def result_preview(self):
        """vnect_result_preview: the (dh, dw, 3) preview of the frame collect_tracked delivered last (a fresh array), or None if it has none."""
        return self._result_picture(lib().vnect_result_preview)

    # -- the 3-D view: the skeleton plot of joints_3d, rendered on the device (include/vnect_abi.h; VIEW3D.md) ---------------------------
    def view3d_device(self, joints_3d, spec, out, out_pitch, confidence=None):
        """vnect_view3d_device: the view of joints_3d (21, 3) into the memory at address `out` (device or host), rows out_pitch bytes apart;
        done on return."""
        j3 = _fixed(joints_3d, np.float32, (21, 3), "joints_3d")
        cf = _fixed(confidence, np.float64, (21,), "confidence", optional=True)
        self._ck_device(lib().vnect_view3d_device(self._h, _ptr(j3, _f32p), _ptr(cf, _f64p),
                                                  None if spec is None else C.byref(spec), C.c_void_p(int(out)), int(out_pitch)))

    def track_view3d(self, stream, spec):
        """vnect_track_view3d: while set (spec a View3dSpec), every tracked submit of `stream` also renders its frame's 3-D view:
        result_view3d() after collect_tracked().  spec None: off."""
        self._ck_device(lib().vnect_track_view3d(self._h, stream, None if spec is None else C.byref(spec)))

    def result_view3d(self):
        """vnect_result_view3d: the (rows, cols, 3) view of the frame collect_tracked delivered last (a fresh array), or None if it has none."""
        return self._result_picture(lib().vnect_result_view3d)

    # -- the person detector: HOG + linear SVM over a pyramid, on the device (include/vnect_abi.h; HOG.md) ------------------------------
    def track_redetect(self, stream, spec=None, enable=True):
        """vnect_track_redetect: while enabled, a tracked frame of `stream` that its loss rule declares lost hands the next frame the
        largest detection of itself through cal_rect (the whole frame when nobody is found), computed on the device (HOG.md).  spec: a
        HogSpec (max_hits at most 4096) or None for the defaults."""
        self._ck_device(lib().vnect_track_redetect(self._h, stream, None if spec is None else C.byref(spec), 1 if enable else 0))

    def result_redetect(self):
        """vnect_result_redetect: (status, [x, y, w, h], hits) of the frame collect_tracked delivered last -- status 0 no detection ran,
        1 found, 2 nobody found, 3 more hits than max_hits; the rect is the chosen detection before cal_rect (zeros unless found)."""
        st, hits, rect = C.c_int32(0), C.c_int32(0), np.zeros(4, np.int32)
        self._ck(lib().vnect_result_redetect(self._h, C.byref(st), _ptr(rect, _i32p), C.byref(hits)))
        return int(st.value), [int(v) for v in rect], int(hits.value)

    def hog_set_detector(self, w):
        """vnect_hog_set_detector: 3781 floats, rho last (cv2.HOGDescriptor_getDefaultPeopleDetector()'s layout), or 3780 with rho 0."""
        a = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))
        rc = lib().vnect_hog_set_detector(self._h, _ptr(a, _f32p), int(a.size))
        if rc == E_ARG:
            raise DeviceFrameError(rc, lib().vnect_last_error(self._h).decode())
        self._ck(rc)

    def hog_levels(self, frame, spec=None):
        """vnect_hog_levels: ((n, 2) int32 level sizes (rows, columns), (n,) float64 scales) of `frame` (a DeviceFrame; only H and W count)."""
        n, hw, sc = C.c_int32(0), np.zeros((64, 2), np.int32), np.zeros(64, np.float64)
        self._ck_device(lib().vnect_hog_levels(self._h, C.byref(frame), None if spec is None else C.byref(spec), C.byref(n), _ptr(hw, _i32p),
                                               _ptr(sc, _f64p), 64))
        return hw[:n.value].copy(), sc[:n.value].copy()

    def _hog_out(self, call, capacity):
        """call(rects pointer, weights pointer, capacity, count) -> ((n, 4) int32 rects [x, y, w, h], (n,) float64 weights), all of them"""
        while True:
            rects, ws, cnt = np.zeros((max(capacity, 1), 4), np.int32), np.zeros(max(capacity, 1), np.float64), C.c_int32(0)
            self._ck_device(call(_ptr(rects, _i32p), _ptr(ws, _f64p), capacity, C.byref(cnt)))
            if cnt.value <= capacity:
                return rects[:cnt.value].copy(), ws[:cnt.value].copy()
            capacity = cnt.value

    def hog_detect_device(self, frame, spec=None, stream=None, capacity=256):
        """vnect_hog_detect_device: the grouped detections of `frame` (a DeviceFrame without a rect); done on return."""
        sp, st = None if spec is None else C.byref(spec), _stream_arg(stream)
        return self._hog_out(lambda r, w, cap, cnt: lib().vnect_hog_detect_device(self._h, C.byref(frame), st, sp, r, w, cap, cnt), capacity)

    def hog_detect(self, img, spec=None, capacity=256):
        """vnect_hog_detect: the grouped detections of a host BGR frame."""
        img = _as_frame(img)
        H, W = img.shape[:2]
        sp = None if spec is None else C.byref(spec)
        return self._hog_out(lambda r, w, cap, cnt: lib().vnect_hog_detect(self._h, _ptr(img, _u8p), H, W, img.strides[0], sp, r, w, cap, cnt), capacity)

    def read_frame(self, slot):
        """The (H, W, 3) BGR frame resident slot `slot` holds (a debugging read)."""
        hw = (C.c_int32 * 2)()
        self._ck(lib().vnect_read_frame(self._h, slot, None, 0, hw))
        out = np.empty((hw[0], hw[1], 3), np.uint8)
        self._ck(lib().vnect_read_frame(self._h, slot, _ptr(out, _u8p), out.size, hw))
        return out

    def batch_layers(self):
        """The batched plan's layers (vnect_get_batch_layer_info), in the layout of layers()."""
        return self._layer_list(lib().vnect_get_batch_layer_info)

    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * 128)()
        rc = lib().vnect_comm_unique_id(buf)
        if rc:
            raise VnectError(rc, lib().vnect_last_error(None).decode())
        return bytes(buf)

    @staticmethod
    def comm_library():
        """(path of the RCCL the library resolved, True if it reused a copy the process had mapped already -- torch's)."""
        buf, reused = C.create_string_buffer(1024), C.c_int32(-1)
        rc = lib().vnect_comm_library(buf, len(buf), C.byref(reused))
        if rc:
            raise VnectError(rc, lib().vnect_last_error(None).decode())
        return buf.value.decode(), bool(reused.value)

    def comm_init(self, rank, nranks, unique_id):
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        self._ck(lib().vnect_comm_init(self._h, rank, nranks, buf))

    def joint_filter(self, dim, values, values_are_f32, t):
        """The handle's 2-D / 3-D OneEuro bank over (21, dim) values at timestamp t -> filtered float64 array."""
        vin = np.ascontiguousarray(values, dtype=np.float64)
        if vin.shape != (21, dim):
            raise ValueError("joints must be (21, %d)" % dim)
        out = np.empty((21, dim), np.float64)
        self._ck(lib().vnect_joint_filter(self._h, dim, _ptr(vin, _f64p), int(values_are_f32), float(t), _ptr(out, _f64p)))
        return out

    def p2p_export(self):
        """128-byte description of this rank's exchange block (exchange=XCHG_P2P); give every rank everybody's."""
        buf = (C.c_char * 128)()
        self._ck(lib().vnect_comm_p2p_export(self._h, buf))
        return bytes(buf)

    def p2p_init(self, rank, nranks, blobs):
        raw = b"".join(blobs)
        if len(raw) != 128 * nranks:
            raise ValueError("p2p_init needs one 128-byte blob per rank")
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)
        self._ck(lib().vnect_comm_p2p_init(self._h, rank, nranks, buf))

    def reset_filters_stream(self, stream):
        self._ck(lib().vnect_reset_filters_stream(self._h, stream))

    def reset_filters(self):
        self._ck(lib().vnect_reset_filters(self._h))

    def activation(self, name):
        shp = (C.c_int32 * 4)()
        self._ck(lib().vnect_read_activation(self._h, name.encode(), None, 0, shp))
        out = np.empty(tuple(shp), np.float32)
        self._ck(lib().vnect_read_activation(self._h, name.encode(), _ptr(out, _f32p), out.size, shp))
        return out

    def set_profiling(self, on):
        self._ck(lib().vnect_set_profiling(self._h, int(on)))

    def timings(self):
        t = Timings()
        t.struct_size = C.sizeof(Timings)
        self._ck(lib().vnect_get_timings(self._h, C.byref(t)))
        d = {k: getattr(t, k) for k, _ in Timings._fields_ if k != "struct_size"}
        # the shader clock the chip held while the conv launches of the profiled frames ran (s_memtime / s_memrealtime of workgroup 0)
        d["shader_clock_mhz"] = 100.0 * d["shader_cycles"] / d["shader_ticks"] if d["shader_ticks"] > 0 else None
        return d

    def reset_timings(self):
        self._ck(lib().vnect_reset_timings(self._h))

    def layer_stamps(self, idx):
        """Raw device-clock stamps (100 MHz) of layer idx in the last profiled frame; see vnect_get_layer_stamps."""
        buf = (C.c_uint64 * 24)()
        self._ck(lib().vnect_get_layer_stamps(self._h, idx, buf))
        return list(buf)

    def layers(self):
        return self._layer_list(lib().vnect_get_layer_info)

    def layer_rows(self, batch=False):
        """Per launch of the plan (batch: of the batched plan): (rows_computed, live_rule_stride) -- vnect_get_layer_rows."""
        out, i = [], 0
        while True:
            rows, rule = C.c_int32(), C.c_int32()
            rc = lib().vnect_get_layer_rows(self._h, i, int(batch), C.byref(rows), C.byref(rule))
            if rc == E_STATE:
                self._ck(rc)
            if rc:
                return out
            out.append((rows.value, rule.value))
            i += 1

    def _layer_list(self, fn):
        out, i = [], 0
        while True:
            li = LayerInfo()
            rc = fn(self._h, i, C.byref(li))
            if rc == E_STATE:
                self._ck(rc)
            if rc:
                return out
            out.append({k: (getattr(li, k).decode() if k == "name" else getattr(li, k)) for k, _ in LayerInfo._fields_})
            i += 1


def _as_frame(img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("frame must be a uint8 (H, W, 3) BGR array")
    # A positive row stride may stay arbitrary (crops of a larger frame are passed by stride, no copy); anything else the
    # reference accepts -- flipped views (negative strides), broadcast rows (stride 0), channel-swapped views -- is copied
    if img.strides[2] != 1 or img.strides[1] != 3 or img.strides[0] < img.shape[1] * 3:
        img = np.ascontiguousarray(img)
    return img


def _as_nv12(nv12):
    """(y pointer, y stride, uv pointer, uv stride, H, W) of a 2-D uint8 array of H * 3 // 2 rows: H rows of Y, then H / 2 rows of
    interleaved U, V.  A view with a positive row stride is passed by stride (no copy); anything else is copied."""
    a = np.asarray(nv12)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 3 or a.shape[0] % 3 or a.shape[1] < 2:
        raise ValueError("an NV12 frame must be a uint8 (H * 3 // 2, W) array")
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    H, W = a.shape[0] * 2 // 3, a.shape[1]
    base = a.ctypes.data
    a_keep = a  # (the pointers below are into it)
    y = C.cast(C.c_void_p(base), _u8p)
    uv = C.cast(C.c_void_p(base + H * a.strides[0]), _u8p)
    y._keep = uv._keep = a_keep
    return y, a.strides[0], uv, a.strides[0], H, W


# ---- frames in device memory ----------------------------------------------------------------------------------------------------------
def is_device_array(x):
    """True for an object that exposes device memory through __cuda_array_interface__ (a torch / cupy array on the GPU) -- or a
    (y, uv) pair of such objects (NV12 in separate planes)."""
    if isinstance(x, (tuple, list)):
        return len(x) == 2 and all(hasattr(p, "__cuda_array_interface__") for p in x)
    return hasattr(x, "__cuda_array_interface__")


def _cai(x, ndim, what):
    """(pointer, shape, strides in bytes) of a uint8 device array of `ndim` dimensions."""
    try:
        d = x.__cuda_array_interface__
    except AttributeError:
        raise ValueError("%s must expose device memory through __cuda_array_interface__" % what) from None
    if d.get("typestr") != "|u1":
        raise ValueError("%s must be uint8 (typestr '|u1'), not %r" % (what, d.get("typestr")))
    shape = tuple(int(v) for v in d["shape"])
    if len(shape) != ndim or any(v < 1 for v in shape):
        raise ValueError("%s must have %d non-empty dimensions, not shape %r" % (what, ndim, shape))
    strides = d.get("strides")
    if strides is None:  # C-contiguous
        strides, n = [], 1
        for v in reversed(shape):
            strides.insert(0, n)
            n *= v
    strides = tuple(int(v) for v in strides)
    if any(v < 1 for v in strides):
        raise ValueError("%s has a zero or negative stride %r: pass a flipped frame as it is stored, with orientation= (ORIENTATION.md); broadcast on the device first (.contiguous())" % (what, strides))
    ptr = d["data"][0]
    if not ptr:
        raise ValueError("%s has a null data pointer" % what)
    return int(ptr), shape, strides


FORM_NAMES = ("packed-3", "packed-4", "planar", "generic")


def device_form(stride_x, stride_c):
    """The kernel form the strides select (ingest.h: ingest_form) -- 0 packed-3, 1 packed-4, 2 planar, 3 generic."""
    if stride_x == 3 and stride_c == 1:
        return 0
    if stride_x == 4 and stride_c == 1:
        return 1
    if stride_x == 1 and stride_c >= 1:
        return 2
    return 3


def device_frame(x, pixel_format="bgr", rect=None):
    """The vnect_device_frame of `x`: for "bgr" / "rgb" an (H, W, 3) uint8 device array with any positive strides (a packed tensor,
    chw.permute(1, 2, 0), bgra[..., :3], any slice); for "nv12" an (H * 3 // 2, W) device array (Y rows, then the U, V rows) or a
    (y, uv) pair of (H, W) and (H // 2, W) arrays.  The structure keeps `x` alive."""
    if pixel_format not in ("bgr", "rgb", "nv12"):
        raise ValueError("pixel_format must be 'bgr', 'rgb' or 'nv12'")
    f = DeviceFrame()
    f.struct_size = C.sizeof(DeviceFrame)
    if pixel_format == "nv12":
        f.format = PIX_NV12
        if isinstance(x, (tuple, list)):
            if len(x) != 2:
                raise ValueError("separate NV12 planes are a (y, uv) pair")
            yp, ysh, yst = _cai(x[0], 2, "the Y plane")
            up, ush, ust = _cai(x[1], 2, "the UV plane")
            if ysh[0] % 2 or ysh[1] % 2 or ush != (ysh[0] // 2, ysh[1]):
                raise ValueError("NV12 planes must be (H, W) and (H // 2, W) with even H and W, not %r and %r" % (ysh, ush))
            if yst[1] != 1 or ust[1] != 1:
                raise ValueError("NV12 planes must have unit column stride")
            f.H, f.W, f.data, f.stride_y, f.uv, f.uv_stride = ysh[0], ysh[1], yp, yst[0], up, ust[0]
        else:
            p, sh, st = _cai(x, 2, "an NV12 frame")
            if sh[0] < 3 or sh[0] % 3 or sh[1] < 2 or sh[1] % 2 or st[1] != 1:
                raise ValueError("an NV12 frame must be a uint8 (H * 3 // 2, W) array with even H and W and unit column stride")
            H = sh[0] * 2 // 3
            f.H, f.W, f.data, f.stride_y, f.uv, f.uv_stride = H, sh[1], p, st[0], p + H * st[0], st[0]
    else:
        f.format = PIX_RGB if pixel_format == "rgb" else PIX_BGR
        p, sh, st = _cai(x, 3, "a device frame")
        if sh[2] != 3:
            raise ValueError("a device frame must be a uint8 (H, W, 3) array, not shape %r" % (sh,))
        f.H, f.W, f.data, f.stride_y, f.stride_x, f.stride_c = sh[0], sh[1], p, st[0], st[1], st[2]
    if rect is not None:
        f.has_rect = 1
        for k, v in enumerate(rect):
            f.rect[k] = int(v)
    f._keep = x
    return f


def default_stream():
    """The producer stream when the caller names none: torch's current stream if torch is already imported (never imported here), else
    HIP's default stream (0)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None:
        try:
            return int(torch.cuda.current_stream().cuda_stream)
        except Exception:
            return 0
    return 0


def _stream_arg(stream):
    if stream is None:
        stream = default_stream()
    return C.c_void_p(int(stream))


def hip_runtimes_mapped():
    """The distinct libamdhip64 files this process has mapped (more than one: two HIP runtimes, whose pointers mean nothing to each other)."""
    out = set()
    try:
        with open("/proc/self/maps") as fh:
            for ln in fh:
                path = ln.split(None, 5)[-1].strip() if ln.count(" ") >= 5 else ""
                if "libamdhip64" in os.path.basename(path):
                    out.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(out)


IMPORT_ORDER_HINT = "import torch before vnect_amd, so that the process holds one HIP runtime"


def _runtime_hint():
    libs = hip_runtimes_mapped()
    if len(libs) > 1:
        return " -- this process has %d HIP runtimes mapped (%s): %s" % (len(libs), ", ".join(libs), IMPORT_ORDER_HINT)
    return ""
