/*
 * vnect_abi.h -- C ABI of libvnect_hip.so, the MI355X (gfx950) VNect inference path.
 *
 * Drop-in boundary.  In the reference (XinArkh/VNect, paths relative to /root/reference) the
 * per-frame path is src/estimator.py:97-142 (VNectEstimator.__call__); its only native boundary
 * is tf.Session.run at src/estimator.py:100-104.  This library replaces that call AND the Python
 * pre/post-processing around it, so the host keeps one call per frame.  Every entry point cites
 * the reference code it replaces.  Plain C types only; caller owns every host pointer (valid only
 * for the duration of the call); the library owns all device memory, streams, graphs and the
 * OneEuro filter state (one handle == one video stream == one GPU).
 *
 * Conventions: every int-returning function returns VNECT_OK (0) or a negative VNECT_E_* code;
 * no C++ exception crosses the boundary; vnect_last_error() gives the message.  Calls on one
 * handle must be serialised by the caller; different handles are independent.
 */
#ifndef VNECT_ABI_H
#define VNECT_ABI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VNECT_ABI_VERSION 7
#define VNECT_MAX_SCALES 8
#define VNECT_MAX_STREAMS 4 /* independent video streams one handle can serve (vnect_submit_stream) */
#define VNECT_BOX 368      /* src/estimator.py:19 box_size   */
#define VNECT_HM 46        /* box_size / hm_factor (:21)     */
#define VNECT_JOINTS 21    /* src/estimator.py:23 joints_sum */

enum {
    VNECT_OK = 0,
    VNECT_E_ARG = -1,       /* bad argument / shape / name                          */
    VNECT_E_STATE = -2,     /* call order (e.g. infer before finalize)              */
    VNECT_E_HIP = -3,       /* HIP runtime error (message has hipGetErrorString)    */
    VNECT_E_NODEVICE = -4,  /* no usable gfx950 device                              */
    VNECT_E_TIMESTAMP = -5, /* timestamp equals the previous one: the reference raises
                               ZeroDivisionError at src/OneEuroFilter.py:66          */
    VNECT_E_COMM = -6,      /* RCCL / peer-access error                             */
    VNECT_E_TIMEORDER = -7, /* timestamp earlier than the previous one: the reference's negative freq drives
                               alpha out of (0, 1] and LowPassFilter.__setAlpha raises ValueError
                               (src/OneEuroFilter.py:19-23, 58-66)                   */
    VNECT_E_INTERNAL = -8   /* host allocation failure or an internal C++ exception, caught at the boundary */
};

enum { VNECT_FP32 = 0,        /* fp32 tensors, v_mfma_f32_32x32x2_f32 (BASELINE.json configs[1])                                      */
       VNECT_BF16 = 1,        /* bf16 tensors and weights, fp32 accumulate (configs[2])                                               */
       VNECT_FP32_SPLIT = 2,  /* fp32 tensors, fp32 accumulate; the PRODUCTS of the 64x64-tile layers run on the bf16 matrix pipe as
                                 exact three-way splits (x = xh + xm + xl, 6 of the 9 piece products; conv.hip, X3): fp32-class
                                 results -- gated like VNECT_FP32 -- at 2.7x the matrix rate of the fp32 instruction                  */
       VNECT_FP16 = 3         /* fp16 (IEEE binary16, round to nearest even) tensors and weights, fp32 accumulate, bias, BN and split-K
                                 slabs; final maps and post-processing fp32/f64 -- VNECT_BF16's plan launch for launch on
                                 v_mfma_f32_32x32x16_f16 (the same cycles), with 11 significant bits against 8.  vnect_finalize refuses a conv
                                 weight that rounds to infinity in fp16 (|w| >= 65520) with VNECT_E_ARG and the tensor's name                */ };

typedef struct vnect_handle vnect_handle;

typedef struct vnect_config {
    int32_t struct_size;              /* = sizeof(vnect_config)                                   */
    int32_t device;                   /* HIP device ordinal                                       */
    int32_t num_scales;               /* len(self.scales), src/estimator.py:32                    */
    double scales[VNECT_MAX_SCALES];  /* each in (0, 1]                                           */
    int32_t precision;                /* VNECT_FP32 | VNECT_BF16 | VNECT_FP32_SPLIT | VNECT_FP16  */
    int32_t paper_res2c;              /* 0 = reference wiring src/vnect_model.py:56 (default)     */
    int32_t use_graph;                /* 0 = eager launches; 1 = replay the frame as one hipGraph;
                                         2 = auto: eager for a frame submitted while none is in flight
                                         (synchronous use), graph replay behind frames in flight    */
    int32_t numpy_promotion;          /* float32-fed 3-D filters: 0 = numpy 1.x rules (the only
                                         numpy TF1 runs with), 1 = NEP 50 (numpy >= 2)            */
    int32_t max_frame_bytes;          /* capacity of one resident frame slot; 0 -> 4096*4096*3     */
    int32_t num_frame_slots;          /* resident frame slots (>=1); 0 -> 4                        */
    int32_t pyramid_nranks;           /* 0/1 = off; else must equal num_scales: this handle runs the
                                         pre-processing and conv stack of ONE scale (see vnect_comm_init) */
    int32_t pyramid_rank;             /* which scale (0 .. pyramid_nranks-1)                       */
    int32_t keep_activations;         /* 0 (default) = layer outputs share an activation arena sized for the peak
                                         live set, so weights + activations stay in the Infinity Cache between
                                         frames; 1 = one private buffer per layer output, which is what
                                         vnect_read_activation needs to return an inner layer (tests, debugging) */
    int32_t lanes;                    /* 0/1 (default): frames run one after the other.  2 or 3: a frame submitted while others
                                         are in flight (vnect_submit_resident before vnect_collect; up to `lanes` frames)
                                         runs on a lane of its own -- own stream, activation arena and graph, same weights --
                                         and overlaps with them; only the joints kernels stay in order (the OneEuro filters
                                         are a chain).  Results are bit-identical to sequential execution; each extra lane
                                         costs one more activation arena (~0.1 GB)                                          */
    int32_t preprocess_only;          /* 1: the handle serves vnect_preprocess (and vnect_set_scales) only -- the static
                                         gen_input_batch of src/estimator.py:70-81 needs no session either: no weights, no
                                         launch plan, ~20 MB of device memory; vnect_finalize and inference are refused      */
    int32_t exchange;                 /* pyramid sharding: how a rank's maps reach the others (VNECT_XCHG_*)                 */
} vnect_config;

enum { VNECT_XCHG_RCCL = 0,   /* ncclAllGather on the handle's stream (default)                                             */
       VNECT_XCHG_P2P = 1 };  /* peer writes over xGMI: a copy kernel stores the rank's 710 976 B straight into every peer's
                                 gather slot (hipDeviceEnablePeerAccess + IPC-mapped buffers), one flag per rank          */

/* Replaces VNectEstimator.__init__ (src/estimator.py:27-68): session + graph + 42 + 63 filters. */
int vnect_create(const vnect_config* cfg, vnect_handle** out);
void vnect_destroy(vnect_handle* h);
/* Message of the last failure on h (h == NULL: last vnect_create failure). Never NULL. */
const char* vnect_last_error(vnect_handle* h);
int vnect_abi_version(void);

/* ABI v6.  How THIS binary was built, as one line of `key=value` text (static storage, never NULL): `abi`, `compiler`, `flags`, `variant`
 * (the Makefile's VARIANT, empty for the product), `test_hooks` (1 only in the test build that can inject warm-start failures), every
 * compile-time probe switch of the kernel sources with its value (X3_DBG, WT_DBG, CH_DBG, F32_NOSTORE, BF16_NOSTORE, VNECT_AB, NS_6432,
 * NS_32128, POST_DBG, ARG_SLABS, ARG_ROWSPLIT -- most of them give wrong results on purpose) and `probes_off` = 1 iff all of them are
 * at their product values.  A deployment check (and tests/test_abi_cpu.py) reads `probes_off=1 test_hooks=0`.  Replaces nothing in the
 * reference: its counterpart is knowing which TensorFlow build `import tensorflow` loaded (src/estimator.py:9).                        */
const char* vnect_build_info(void);

/* Replaces VNect.load_weights / assign_weights_from_dict (src/vnect_model.py:219-236).
 * name is a key of the reference's pickle schema (src/caffe2pkl.py:51-80), e.g.
 * "conv1/weights" (kh,kw,Cin,Cout), "conv1/biases", "res5c_branch1a/kernel" (kh,kw,Cout,Cin),
 * "bn5c_branch2a/gamma".  Data is copied.  All 109 arrays must be set before vnect_finalize. */
int vnect_set_weight(vnect_handle* h, const char* name, const float* data, const int64_t* shape, int ndim);
/* Packs weights into kernel layouts, uploads them, plans buffers, builds the launch sequence, and warms the handle up on a few grey
 * frames (so that the first real frame runs at steady-state speed; the filters and frame slots are those of a fresh handle
 * afterwards).  A launch or device error DURING the warm start is returned (VNECT_E_HIP / VNECT_E_INTERNAL: the plan this handle
 * would run for every frame is broken); a refused grey frame only skips the warm start and leaves a note in vnect_last_error.
 * (The reference's counterpart is saver.restore, src/estimator.py:55-60.) */
int vnect_finalize(vnect_handle* h);

/* `self.scales = [...]` (src/estimator.py:32 is a plain attribute callers may overwrite). */
int vnect_set_scales(vnect_handle* h, const double* scales, int num_scales);

/* Replaces sess.run([heatmap,x,y,z], {input: batch}) (src/estimator.py:100-104):
 * batch (S,368,368,3) f32 NHWC -> out (S,46,46,84) f32, channels [hm | x | y | z] x 21
 * (the tf.split at src/vnect_model.py:216-217 is a view of this tensor). S = num_scales. */
int vnect_forward(vnect_handle* h, const float* batch_nhwc, int num_images, float* out_maps);

/* Replaces VNectEstimator.gen_input_batch (src/estimator.py:70-81) on the device.
 * bgr: (H,W,3) uint8, row_stride bytes per row.  batch_out may be NULL (batch stays on device). */
int vnect_preprocess(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, float* batch_out,
                     double* scaler, int32_t* offset_x, int32_t* offset_y);

/* Replaces src/estimator.py:105-139 (multi-scale merge, extract_2d_joints, joint_filter,
 * extract_3d_joints, joint_filter, un-mapping) for maps supplied by the caller.
 * t2d / t3d stand for the two time.time() reads at src/estimator.py:84. */
int vnect_postprocess(vnect_handle* h, const float* maps, double t2d, double t3d, double scaler, int32_t offset_x,
                      int32_t offset_y, double* joints_2d /*21x2 [row,col]*/, float* joints_3d /*21x3*/);

/* Replaces VNectEstimator.__call__ (src/estimator.py:97-142) end to end. */
int vnect_infer(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, double t2d, double t3d,
                double* joints_2d, float* joints_3d);

/* Where a capture pipeline should put its frames so that vnect_infer's host-to-device copy needs no CPU copy first: the handle's
 * two PINNED staging buffers (index 0 / 1, at least min_bytes each, <= max_frame_bytes; the pointer stays valid until a larger
 * request for the same index or vnect_destroy).  The reference's loop gets its frame from cv2.VideoCapture.read into pageable numpy
 * memory (run_estimator_ps.py:75-82) and hands it to __call__ (src/estimator.py:97-99); vnect_infer accepts ANY host pointer -- a
 * pageable one is copied into these buffers by the CPU (one memcpy), a pointer INSIDE one of them (the whole frame or a strided crop
 * of it) is DMA-ed from where it lies.  Either way the device copy is asynchronous on the frame's stream. */
int vnect_frame_buffer(vnect_handle* h, int index, int64_t min_bytes, uint8_t** ptr_out);

/* Frames resident in HBM (throughput measurement; a capture pipeline that DMA-writes frames).
 * upload copies a frame into slot; infer_resident runs __call__ on it without a host->device copy. */
int vnect_upload_frame(vnect_handle* h, int slot, const uint8_t* bgr, int H, int W, int64_t row_stride);
int vnect_infer_resident(vnect_handle* h, int slot, double t2d, double t3d, double* joints_2d, float* joints_3d);
/* Pipelining of the same call: submit enqueues a frame, collect waits for the oldest un-collected one (FIFO).
 * At most max(lanes, 2) frames may be in flight (one lane: the second frame queues behind the first on its stream). */
int vnect_submit_resident(vnect_handle* h, int slot, double t2d, double t3d);
int vnect_collect(vnect_handle* h, double* joints_2d, float* joints_3d);
/* Several independent video streams on ONE handle (one weight copy, `lanes` activation arenas): the reference runs one
 * VNectEstimator -- one set of 42 + 63 OneEuro filters, src/estimator.py:46-52 -- per video, each in a process of its own
 * (run_estimator_ps.py:120-129); here stream s (0 .. VNECT_MAX_STREAMS-1) is a filter bank + its timestamps on the device, and
 * vnect_submit_stream(h, s, ...) is that stream's __call__.  Frames of DIFFERENT streams have no dependency at all, so with
 * lanes = 2 / 3 they overlap completely (frames of one stream still chain through their filters, exactly as vnect_submit_resident
 * -- which is stream 0 -- does).  Results come back in submission order; vnect_collect_stream also says whose they are.  Each
 * stream's results are bit-identical to a handle of its own fed the same frames. */
int vnect_submit_stream(vnect_handle* h, int stream, int slot, double t2d, double t3d);
int vnect_collect_stream(vnect_handle* h, int32_t* stream_out, double* joints_2d, float* joints_3d);
/* New filters for ONE stream (vnect_reset_filters resets all of them). */
int vnect_reset_filters_stream(vnect_handle* h, int stream);
/* ABI v7.  Two videos' frames through ONE conv stack per launch.  The reference runs one estimator per video (run_estimator_ps.py:120-129)
 * over a batch whose images are independent (src/estimator.py:75-80, the batch that sess.run takes at :100-104); here two streams' frames
 * form one batch of 2 S images: image i is scale i % S of the i / S-th frame.  Called before vnect_finalize: n = 1 is the default (no
 * batched plan); n = 2 makes finalize build a second launch plan for 2 S images -- the S-image plan's layers, tiles, K splits and fused
 * forms with M doubled, the same packed weights -- and gives every lane an activation arena for it.  VNECT_E_STATE after finalize or on a
 * preprocess_only handle; VNECT_E_ARG on a pyramid-sharded handle, for n outside 1 .. 2, when 2 S > VNECT_MAX_SCALES, or (n = 2) on a
 * people handle (vnect_set_people).
 * Pays with two or more videos per GPU, where a frame is bound by launch count (bf16); a stream's latency becomes its batch's.         */
int vnect_set_stream_batch(vnect_handle* h, int n);
/* n frames of DISTINCT streams from resident slots as one batch (src/estimator.py:97-142 once per stream, as the reference's per-video
 * processes call it, run_estimator_ps.py:120-129).  n == 2 runs the batched plan; n == 1 is vnect_submit_stream.  Results come back through
 * vnect_collect_stream, one per frame, in array order.  A batch takes one lane and counts once against the in-flight limit.  Atomic: slots,
 * distinct streams, the in-flight limit and both streams' timestamps (VNECT_E_TIMESTAMP / VNECT_E_TIMEORDER as vnect_infer reports them)
 * are all checked before anything changes, so a refused batch leaves every filter bank and timestamp as it was.  Each stream's joints
 * are bit-identical to a handle of its own fed the same frames.  (vnect_forward on such a handle also takes num_images == 2 S and
 * runs the batched plan: a parity aid.) */
int vnect_submit_streams(vnect_handle* h, int n, const int32_t* streams, const int32_t* slots, const double* t2d, const double* t3d);

/* ABI v7, additive.  The tracking loop on the device.  The reference's tracking script (run_estimator_ps.py:80-109) crops every frame with
 * the current box (:88), runs the estimator (src/estimator.py:97-142), shifts the 2-D joints back into frame coordinates (:92-93) and grows
 * their bounding box into the next crop (:96-107), all on the host: frame t+1's crop waits for frame t's joints.  Here the box lives on the
 * device: a small kernel behind the joints stage writes the stream's next rect and its crop geometry, so frames of a tracked stream can be
 * submitted ahead and the host never waits for joints to feed the next frame.  Results are bit-identical to that loop over vnect_infer.
 *
 * vnect_track_begin: stream `stream` tracks (H, W) frames from now on, starting at rect4 = (x, y, w, h) -- NULL: the whole frame.  A rect
 * narrower or lower than one pixel stands for the whole frame (:85-86's fallback); any other rect must start inside the frame (VNECT_E_ARG
 * otherwise), and one that runs past its far edges crops what the loop's numpy slicing crops (:88) and is reported as given.
 * The stream's filters are not reset.  VNECT_E_STATE while frames of the stream are in flight; VNECT_E_ARG on a pyramid-sharded handle
 * or one with vnect_set_stream_batch(h, 2).
 * vnect_submit_tracked: the next frame, the WHOLE (H, W) frame in a resident slot (vnect_upload_frame); the device crops it.
 * vnect_submit_tracked_pinned: the same from pinned buffer buffer_index (vnect_frame_buffer; rows row_stride bytes apart): only the crop's
 * rows cross PCIe.  The buffer is read when the frame runs: rewrite it only after that frame has been collected.
 * vnect_collect_tracked: the oldest frame in flight, as vnect_collect_stream, with joints_2d in FRAME coordinates and the rect the frame was
 * cropped with; an untracked frame gives its usual joints and rect4 = (-1, -1, -1, -1).  vnect_collect / vnect_collect_stream return a
 * tracked frame's joints in frame coordinates too.  A crop squarify refuses (src/utils.py:82-120 raises for it) fails its frame with
 * VNECT_E_ARG and vnect_infer's message; the frame's filters do not advance and its timestamps do not count (as a refusal of vnect_infer
 * commits none), later frames of the stream already in flight fail with VNECT_E_STATE, and so does every submit on the stream until the
 * next vnect_track_begin.
 * vnect_track_box: the rect of the stream's next tracked frame (waits for the stream's frames in flight). */
int vnect_track_begin(vnect_handle* h, int stream, int H, int W, const int32_t* rect4);
int vnect_submit_tracked(vnect_handle* h, int stream, int slot, double t2d, double t3d);
int vnect_submit_tracked_pinned(vnect_handle* h, int stream, int buffer_index, int64_t row_stride, double t2d, double t3d);
int vnect_collect_tracked(vnect_handle* h, int32_t* stream_out, double* joints_2d, float* joints_3d, int32_t* rect4);
int vnect_track_box(vnect_handle* h, int stream, int32_t* rect4);

/* ABI v7, additive.  Per-joint confidence, and what a tracked stream does when it has lost its person (CONFIDENCE.md).  The reference has
 * no counterpart: it returns 21 joints for every frame, whether or not anybody is in it, and its loop grows the next crop from them
 * unconditionally (run_estimator_ps.py:96-107).
 *
 * vnect_result_confidence: confidence21[j] (float64, j = 0 .. 20) of the frame most recently DELIVERED by a successful call on this handle
 * -- vnect_infer*, vnect_postprocess, vnect_collect, vnect_collect_stream, vnect_collect_tracked; one result of a two-stream batch is one
 * delivery.  The value is the maximum of the 368 x 368 bilinear x8 upsample of joint j's merged heat-map, i.e. the element that np.argmax
 * picks in src/utils.py:169-172; for finite maps bit for bit that float64.  It comes from the frame's raw maps: the OneEuro filters do not
 * touch it.  Non-finite maps follow the arg-max's documented deviation: NaN cells never win, and an all-NaN heat-map gives -inf, which is
 * below every threshold.  The values are taken from the delivered frame's own result slot, so with frames in flight they belong to the
 * collected frame, not the newest one.  VNECT_E_STATE before any delivery; a failed call leaves the previous values standing.
 * lost_out (may be NULL): 1 if the loss rule below called the frame lost; 0 for untracked frames and for action 0.
 *
 * vnect_track_policy: the loss rule of tracked stream `stream`, applied on the device by the box stage of every tracked frame:
 *   confident = #{ j : confidence[j] >= min_confidence },  lost = confident < min_joints.
 * action 0 (off, the default): the loop as it is, lost reported 0.  action 1 (hold): a lost frame leaves the stream's box as it is -- the
 * next frame is cropped with this frame's crop.  action 2 (reset): the next crop is the whole frame (if squarify refuses the whole frame,
 * the stream stops as at any refused crop).  A lost frame's joints are still delivered and the filters advance as on any frame.
 * The rule belongs to the stream and survives vnect_track_begin, until it is set again.  VNECT_E_ARG for min_joints outside 1 .. 21, an
 * action outside 0 .. 2, a NaN threshold, and on the handles vnect_track_begin refuses; VNECT_E_STATE while the stream has a tracked frame
 * in flight. */
int vnect_result_confidence(vnect_handle* h, double* confidence21, int32_t* lost_out);
int vnect_track_policy(vnect_handle* h, int stream, double min_confidence, int min_joints, int action);

/* ABI v7, additive.  NV12 frames.  The reference's loop takes its frame from camera_capture.read() (run_estimator_ps.py:79,109), and
 * cv2.VideoCapture hands out BGR: whatever the camera or decoder delivered -- on this hardware NV12, a full-resolution Y plane and one
 * half-resolution plane of interleaved U, V -- OpenCV has converted by then.  That colour conversion is OpenCV's, not the reference's own
 * code; these entry points do it on the device, inside the copy that brings the frame into its resident slot (1.5 bytes per pixel cross
 * PCIe instead of 3), with the integer arithmetic of cv2.cvtColor(nv12, cv2.COLOR_YUV2BGR_NV12): BT.601 limited range, 20-bit fixed point,
 * chroma replicated (vnect_amd/csrc/nv12.h; NV12.md).  Everything behind the slot sees the BGR frame it always saw, so every result is
 * bit-identical to the BGR entry point given the converted frame.
 * y / uv: the two planes, rows y_stride / uv_stride bytes apart (each >= W), at any byte address; H and W are even.  rect4 = (x, y, w, h)
 * or NULL: only that crop of the frame is converted (chroma by absolute frame coordinates; odd origins and sizes are fine) and the call is
 * the BGR call on the converted frame's crop, as the tracking loop slices it (run_estimator_ps.py:88) -- joints in crop coordinates.  A
 * rect past the frame's far edges crops what that slicing crops.  Planes INSIDE one of the vnect_frame_buffer buffers are read where they
 * lie; anything else is first copied into an internal pinned stage by the CPU.
 * VNECT_E_ARG, before anything changes (no timestamp, no slot geometry): odd W or H; a stride below W; a UV plane that overlaps the Y plane
 * or planes that run past the pinned buffer they start in; a rect whose origin lies outside the frame or that is empty; more BGR bytes
 * (3 per pixel of the frame, or of the crop) than max_frame_bytes.
 * vnect_upload_frame_nv12: afterwards the slot holds the H x W BGR frame exactly as if vnect_upload_frame had been given the converted
 * frame (src/estimator.py:97-99 takes it from there): every resident-slot submit and vnect_submit_tracked work on it unchanged.
 * vnect_upload_frame_nv12_rect: the same with a crop, which lands at the slot's origin: the slot holds the converted frame's
 * [y:y + h, x:x + w] (run_estimator_ps.py:88).  Both return when the slot is filled and, like vnect_upload_frame, wait only for the slot's
 * last reader, not for frames computing from other slots.
 * vnect_infer_nv12: vnect_infer (src/estimator.py:97-142) of the converted frame's crop.
 * vnect_preprocess_nv12: vnect_preprocess (src/estimator.py:70-81) of it; also on a preprocess_only handle.
 * vnect_submit_tracked_pinned_nv12: vnect_submit_tracked_pinned with the NV12 frame in pinned buffer buffer_index -- Y plane at its start,
 * UV plane uv_offset bytes in; only the crop's rows of both planes cross PCIe.  Same refusals, status and rollback as the BGR form.
 * vnect_read_frame: the BGR bytes of a resident slot, packed (H, W, 3), and its size in hw2 = (H, W); out may be NULL (size only).  A
 * debugging read like vnect_read_activation (what the reference would see as the img_input of src/estimator.py:97). */
int vnect_upload_frame_nv12(vnect_handle* h, int slot, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W);
int vnect_upload_frame_nv12_rect(vnect_handle* h, int slot, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W,
                                 const int32_t* rect4);
int vnect_infer_nv12(vnect_handle* h, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W,
                     const int32_t* rect4, double t2d, double t3d, double* joints_2d, float* joints_3d);
int vnect_preprocess_nv12(vnect_handle* h, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W,
                          const int32_t* rect4, float* batch_out, double* scaler, int32_t* offset_x, int32_t* offset_y);
int vnect_submit_tracked_pinned_nv12(vnect_handle* h, int stream, int buffer_index, int64_t y_stride, int64_t uv_offset, int64_t uv_stride,
                                     double t2d, double t3d);
int vnect_read_frame(vnect_handle* h, int slot, uint8_t* out, int64_t capacity, int32_t* hw2);

/* ABI v7, additive.  Frames that already lie in DEVICE memory: a decoder's surface in VRAM, a torch tensor, another model's output.  The
 * reference reads its frame on the host (src/estimator.py:97-99 takes img_input from there) and its loop crops it with a numpy slice
 * (run_estimator_ps.py:88); these entry points take the same pixels from the caller's device allocation, and a kernel writes them -- or
 * the crop `rect` -- into a resident slot as the packed BGR rows every other entry point leaves there (vnect_amd/csrc/ingest.h;
 * DEVICE_FRAMES.md).  Everything behind the slot sees the frame it always saw, so every result is bit-identical to the host entry point
 * given the same BGR pixels.
 * format VNECT_PIX_BGR / VNECT_PIX_RGB: `data` is pixel (0, 0) channel 0 and channel c of pixel (y, x) lies at
 * data + y stride_y + x stride_x + c stride_c, all three strides positive: packed 3-byte pixels (., 3, 1), 4-byte pixels (., 4, 1: BGRA,
 * RGBA, BGRX -- the fourth byte is never read), planar CHW (., 1, plane stride) are read with coalesced dword loads, any other strides one
 * pixel per lane.  VNECT_PIX_NV12: `data` is the Y plane (rows stride_y apart), `uv` the interleaved U, V plane (rows uv_stride apart), in
 * one allocation or two; converted as vnect_infer_nv12 converts.  rect = (x, y, w, h) with has_rect: the crop, as numpy slicing crops it
 * (a rect past the far edges is cut there); joints in crop coordinates.
 * producer_stream: the hipStream_t on which the frame's last writes were enqueued; NULL is HIP's default stream; VNECT_STREAM_SYNCED: the
 * caller has synchronised, wait for nothing.  Otherwise the library records an event on that stream and the stream it ingests on waits
 * for it: the host never blocks on the producer.
 * VNECT_E_ARG, before any launch and before anything changes (no timestamp, no slot geometry, no filter): struct_size wrong; `data` (or
 * `uv`) not device memory of the handle's device as THIS process's HIP runtime knows it -- host memory, managed memory, another device's
 * memory: use vnect_infer / vnect_upload_frame for host memory; a frame whose last byte lies outside the allocation `data` points into
 * (hipMemGetAddressRange); a stride below 1; NV12 with odd W or H, a pitch below W or overlapping planes; a rect whose origin lies
 * outside the frame or that is empty; more BGR bytes (3 per pixel of the frame, or of the crop) than max_frame_bytes.
 * ONE HIP RUNTIME PER PROCESS: a pointer means something only to the runtime that allocated it.  A process that loads this library first
 * and imports torch afterwards can end up with two copies of libamdhip64 (torch ships its own), and torch's pointers are then refused here
 * with VNECT_E_ARG; import torch first, and there is one.
 * vnect_upload_frame_device: afterwards the slot is indistinguishable from one vnect_upload_frame filled with the same BGR pixels.  It
 * returns when the slot is filled (the caller's buffer is free again) and waits only for the slot's last reader.
 * vnect_infer_device: vnect_infer (src/estimator.py:97-142) of those pixels.  vnect_preprocess_device: vnect_preprocess
 * (src/estimator.py:70-81); also on a preprocess_only handle.  Both are done with the caller's buffer when they return.
 * vnect_submit_tracked_device: vnect_submit_tracked_pinned with the whole frame in device memory (a rect is refused: the crop is the
 * stream's box on the device, run_estimator_ps.py:88 and :99-107).  The buffer is read when the frame RUNS: keep it untouched until that
 * frame has been collected.  Same refusals (a frame of another size than vnect_track_begin's, a sharded or batched handle), status and
 * rollback as the pinned form. */
#define VNECT_PIX_BGR 0
#define VNECT_PIX_RGB 1
#define VNECT_PIX_NV12 2
#define VNECT_STREAM_SYNCED ((void*)-1)
typedef struct vnect_device_frame {
    int32_t struct_size;
    int32_t format;      /* VNECT_PIX_BGR | VNECT_PIX_RGB | VNECT_PIX_NV12 */
    int32_t H, W;        /* of the whole frame */
    const void* data;    /* pixel (0,0) channel 0; NV12: the Y plane */
    int64_t stride_y, stride_x, stride_c; /* bytes; NV12: stride_y = Y pitch, the other two ignored */
    const void* uv;      /* NV12 only */
    int64_t uv_stride;
    int32_t has_rect;
    int32_t rect[4];     /* (x, y, w, h) */
} vnect_device_frame;
int vnect_upload_frame_device(vnect_handle* h, int slot, const vnect_device_frame* frame, void* producer_stream);
int vnect_infer_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d, double* joints_2d,
                       float* joints_3d);
int vnect_preprocess_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, float* batch_out, double* scaler,
                            int32_t* offset_x, int32_t* offset_y);
int vnect_submit_tracked_device(vnect_handle* h, int stream, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d);

/* ABI v7, additive.  The skeleton and the crop rectangle drawn into a frame in DEVICE memory (OVERLAY.md).  The reference's frame loop
 * draws into the frame it has just estimated (run_estimator_ps.py:92-94: utils.draw_limbs_2d, src/utils.py:222-243 -- an ellipse of
 * half-axes (length / 2, 3) per limb, then the crop rectangle, thickness 4) with cv2 on the host; these entry points draw the same shapes
 * with one kernel launch into a vnect_device_frame, by an exact rule of this project's own (vnect_amd/csrc/overlay.h: float64 multiplies,
 * adds and compares only, so the host, numpy and the device agree bit for bit; cv2 itself rounds the angle to whole degrees and cannot be
 * pinned here).  Every layout vnect_device_frame describes is written where it lies: packed 3-byte, packed 4-byte (the fourth byte is
 * never written), planar, any positive strides, BGR or RGB order; NV12 gets Y per pixel and a 2 x 2 block's chroma sample if any of its
 * four pixels is drawn (the rect's colour wins), the colours converted once by BT.601 limited range in 8-bit integer arithmetic.  A pixel
 * that no shape covers is not written, nor is any byte that is no pixel of the frame.
 * The style, a vnect_overlay_style -- NULL: the reference's colours and parents, no threshold: limb_bgr / rect_bgr, 0 .. 255 each; min_confidence: a
 * limb is left out when the confidence of either of its joints lies below it (NaN: no threshold); parents[i] (with has_parents; 0 .. 20):
 * the joint limb i joins joint i to -- a joint that is its own parent has no limb.
 * vnect_draw_device: joints_2d (21 x 2 float64 [row, col] in the target's coordinates; non-finite or beyond 2^20: its limbs are left out),
 * confidence21 (or NULL: no threshold applies), rect4 = (x, y, w, h) or NULL (no rectangle) into `target`.  `stream` is a producer_stream:
 * the draw is ordered behind what has been enqueued there (NULL: HIP's default stream; VNECT_STREAM_SYNCED: wait for nothing).  Returns
 * when the draw is done.  Works on a preprocess_only handle and before vnect_finalize too.  VNECT_E_ARG, before anything is written: what
 * vnect_upload_frame_device refuses of a frame (a host pointer, a last byte outside the allocation, ...); target->has_rect; a parent
 * outside 0 .. 20; a rect with w < 1 or h < 1; a colour outside 0 .. 255; a wrong struct_size.
 * vnect_submit_tracked_device_draw: vnect_submit_tracked_device, plus one overlay launch on the frame's stream behind its box stage and in
 * front of its completion: `frame` itself is drawn into, as cv2 draws into the reference's `frame` -- with the frame's own joints in frame
 * coordinates, the rect it was cropped with and (with a threshold) its confidences, all read on the device; a frame whose crop was refused
 * is not drawn.  THE BUFFER IS WRITTEN UNTIL THE FRAME HAS BEEN COLLECTED: keep it alive and read it only after vnect_collect_tracked has
 * delivered the frame, which is annotated then.  Joints, rects, confidences and filter states are bit-identical to
 * vnect_submit_tracked_device; its refusals and rollback are that call's, plus the style's (checked before anything changes). */
typedef struct vnect_overlay_style {
    int32_t struct_size;     /* = sizeof(vnect_overlay_style) */
    int32_t limb_bgr[3];     /* (49, 22, 122): src/utils.py:236 */
    int32_t rect_bgr[3];     /* (60, 66, 207): src/utils.py:241 */
    double min_confidence;
    int32_t parents[VNECT_JOINTS];
    int32_t has_parents;     /* 0: the reference's (src/estimator.py joint_parents) */
} vnect_overlay_style;
int vnect_draw_device(vnect_handle* h, const vnect_device_frame* target, void* stream, const double* joints_2d, const double* confidence21,
                      const int32_t* rect4, const vnect_overlay_style* style);
int vnect_submit_tracked_device_draw(vnect_handle* h, int stream, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d,
                                     const vnect_overlay_style* style);

/* ABI v7, additive.  The preview: the annotated frame scaled for display, computed on the device (PREVIEW.md).  The reference's frame loop
 * draws into a copy of the frame and scales that copy to 1024 pixels on its longer side before it shows it (run_estimator_ps.py:94-96:
 * frame_draw = utils.draw_limbs_2d(frame.copy(), ..); frame_draw = utils.img_scale(frame_draw, 1024 / max(W_img, H_img)); cv2.imshow).
 * One kernel launch reads the frame where it lies -- every layout vnect_device_frame describes, under the orientation in force --, applies
 * the overlay's rule (vnect_amd/csrc/overlay.h, in the BGR domain) to every source tap and writes cv2.resize(.., fx = fy = factor,
 * INTER_LINEAR) of the annotated picture in cv2's own 11-bit fixed point (vnect_amd/csrc/preview.h).  THE FRAME IS NEVER WRITTEN.
 * vnect_preview_spec: factor -- 0: the reference's 1024.0 / max(W, H) of the oriented picture; out_format -- VNECT_PIX_BGR or VNECT_PIX_RGB,
 * packed 3 bytes per pixel; draw_frame -- vnect_submit_tracked_device_preview only: the frame itself is annotated too.
 * vnect_preview_size (run_estimator_ps.py:94-96: the size cv2.resize gives the displayed picture): out_hw = (rows, columns) =
 * (cv_round(Hp factor), cv_round(Wp factor)), half to even, of the frame's oriented picture (Hp, Wp) under the orientation in force.
 * Arithmetic only: the frame's pointers are not looked at; works before vnect_finalize and on a preprocess_only handle.
 * vnect_preview_device (run_estimator_ps.py:94-96): the preview of `frame` into `out`, rows out_pitch >= 3 * columns bytes apart; no byte
 * outside the 3 * columns bytes of each row is written.  joints_2d (21 x 2 float64 [row, col], oriented coordinates), confidence21, rect4
 * and style are vnect_draw_device's, each may be NULL (no joints and no rect: the plain scaled picture).  `out` is device memory of the
 * handle's device (the kernel writes it; its last byte must lie inside its allocation) or host memory, pinned or pageable (the library
 * stages and copies).  The launch is ordered behind producer_stream as in vnect_draw_device and runs on the handle's upload stream; the
 * preview is complete on return.  Needs no weights.  VNECT_E_ARG, before anything is launched or written: a factor that is negative, NaN
 * or infinite; an output side that rounds to 0 or exceeds VNECT_PREVIEW_MAX; everything vnect_draw_device refuses of a frame (but an NV12
 * frame under an orientation is accepted: it is only read) or a style; frame->has_rect; draw_frame; an out_format other than the two; an
 * output that overlaps the frame; out_pitch < 3 * columns; an `out` that is neither such device memory nor host memory.
 * vnect_submit_tracked_device_preview (run_estimator_ps.py:94-96 inside the tracked loop): vnect_submit_tracked_device, plus one preview
 * launch on the frame's lane stream behind its box stage -- joints in frame coordinates, rect_used, status and (with a threshold)
 * confidences are read from the frame's result-ring slot on the device -- plus the preview's copy to the host, both in front of the
 * frame's completion.  The preview lands in a pinned host buffer the handle owns, one per result-ring slot; the buffers are sized at the
 * first such submit and re-sized (for a larger preview) only while nothing is in flight: VNECT_E_STATE otherwise.  With spec->draw_frame
 * the overlay launch of vnect_submit_tracked_device_draw follows the preview launch on the same stream: the preview reads the clean frame
 * and the frame is then annotated in place as that call leaves it; this order is part of the contract.  A frame whose crop was refused
 * has no preview.  Joints, rects, confidences, filter states, refusals and rollback are those of vnect_submit_tracked_device, bit for
 * bit, plus the style's and the spec's (checked before anything changes).
 * vnect_result_preview (run_estimator_ps.py:94-96): the preview of the frame most recently delivered by vnect_collect_tracked -- *data,
 * hw = (rows, columns), *pitch = 3 * columns -- valid until the next submit on the handle; hw = (0, 0) and *data = NULL if that frame
 * has none. */
#define VNECT_PREVIEW_MAX 4096
typedef struct vnect_preview_spec {
    int32_t struct_size;  /* = sizeof(vnect_preview_spec) */
    double factor;        /* 0: 1024.0 / max(Wp, Hp) */
    int32_t out_format;   /* VNECT_PIX_BGR | VNECT_PIX_RGB */
    int32_t draw_frame;   /* 0 */
} vnect_preview_spec;
int vnect_preview_size(vnect_handle* h, const vnect_device_frame* frame, const vnect_preview_spec* spec, int32_t out_hw[2]);
int vnect_preview_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, const double* joints_2d, const double* confidence21,
                         const int32_t* rect4, const vnect_overlay_style* style, const vnect_preview_spec* spec, void* out, int64_t out_pitch);
int vnect_submit_tracked_device_preview(vnect_handle* h, int stream, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d,
                                        const vnect_overlay_style* style, const vnect_preview_spec* spec);
int vnect_result_preview(vnect_handle* h, const uint8_t** data, int32_t hw[2], int64_t* pitch);

/* ABI v7, additive.  The person detector in front of the loop (HOG.md).  The reference finds its first crop box with OpenCV's HOG people
 * detector (src/hog_box.py:24-33: cv2.HOGDescriptor(), setSVMDetector(cv2.HOGDescriptor_getDefaultPeopleDetector()),
 * detectMultiScale(img)), takes the biggest rectangle and inflates it (src/hog_box.py:37-58).  Here the detection runs on the device, by
 * the rule of vnect_amd/csrc/hog.h: a pyramid of the oriented picture in cv2's 8-bit INTER_LINEAR, gamma-corrected gradients, 9-bin votes,
 * 16 x 16 block histograms with L2-Hys, a 64 x 128 window's 3780-element descriptor against the detector vector, groupRectangles on the
 * host.  NOTHING is pinned against cv2 (HOG.md lists what a holder of cv2 should compare first); the detector vector is an INPUT, in the
 * layout cv2.HOGDescriptor_getDefaultPeopleDetector() returns.
 * vnect_hog_set_detector (src/hog_box.py:26): n = 3781 floats, rho last, or 3780 with rho 0.  VNECT_E_ARG: any other n, a NaN or an
 * infinite entry.  The handle keeps a copy.
 * VNECT_E_STATE (nothing changes): a stream on which vnect_track_redetect is set has a tracked frame in flight -- its detection reads the
 * detector whenever it runs.
 * vnect_hog_spec: detectMultiScale's parameters (src/hog_box.py:28 passes none: the defaults); a zero field means its default --
 * hit_threshold 0, win_stride 8 x 8, scale0 1.05, final_threshold 2.0, nlevels 64, max_hits 65536.  spec NULL: all defaults.
 * vnect_hog_levels (src/hog_box.py:28): the pyramid of the frame's oriented picture under the orientation in force -- *n_out levels,
 * hw_out[2 n] = (rows, columns), scales_out[n], the first `capacity` of them (each array may be NULL).  Arithmetic only: the frame's
 * pointers are not looked at.
 * vnect_hog_detect_device (src/hog_box.py:28): the grouped detections of `frame` -- rects4[4 i] = (x, y, w, h) in oriented picture
 * coordinates, weights[i] the largest score of the group -- the first `capacity` of them; *count_out is the full count, also above
 * capacity.  Three launches on the handle's upload stream cover all levels; they are ordered behind producer_stream as in
 * vnect_preview_device, the frame is only read, and the call is done on return.  The workspace belongs to the handle and grows on demand.
 * vnect_hog_detect (src/hog_box.py:28): the same for a host BGR frame, rows row_stride >= 3 * W bytes apart, under the orientation in
 * force; the frame is copied to the device first.
 * All of these work before vnect_finalize and on a preprocess_only handle.  VNECT_E_STATE: no detector set.  VNECT_E_ARG, before anything
 * is launched: frame->has_rect; strides that are not positive multiples of 8; scale0 <= 1; NaN or infinite thresholds; nlevels outside
 * 1 .. 64; a negative max_hits or capacity; a picture side above VNECT_HOG_MAX_SIDE; a pyramid-sharded handle; everything
 * vnect_preview_device refuses of a frame.  A picture smaller than the window in either axis is no error: no level, no detection, no
 * launch.  More than max_hits windows at or above hit_threshold fail the call (VNECT_E_STATE, "raise hit_threshold"): nothing is returned
 * and nothing is written out of bounds. */
#define VNECT_HOG_MAX_SIDE 4096
#define VNECT_HOG_DETECTOR_SIZE 3781
typedef struct vnect_hog_spec {
    int32_t struct_size;     /* = sizeof(vnect_hog_spec) */
    double hit_threshold;    /* 0 */
    int32_t win_stride_x;    /* 0: 8 */
    int32_t win_stride_y;    /* 0: 8 */
    double scale0;           /* 0: 1.05 */
    double final_threshold;  /* 0: 2.0 */
    int32_t nlevels;         /* 0: 64 */
    int32_t max_hits;        /* 0: 65536 */
} vnect_hog_spec;
int vnect_hog_set_detector(vnect_handle* h, const float* w, int n);
int vnect_hog_levels(vnect_handle* h, const vnect_device_frame* frame, const vnect_hog_spec* spec, int32_t* n_out, int32_t* hw_out, double* scales_out,
                     int capacity);
int vnect_hog_detect_device(vnect_handle* h, const vnect_device_frame* frame, void* producer_stream, const vnect_hog_spec* spec, int32_t* rects4,
                            double* weights, int capacity, int32_t* count_out);
int vnect_hog_detect(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, const vnect_hog_spec* spec, int32_t* rects4, double* weights,
                     int capacity, int32_t* count_out);

/* ABI v7, additive.  Re-detection inside the device tracking loop (HOG.md, "Re-detection").  The reference finds a person with HOGBox once
 * (src/hog_box.py:26-31) and its loop falls back to the whole frame ever after (run_estimator_ps.py:96-107); runner.track's
 * lost=(c, n, "detect") puts the detector in the place of that fallback on the host's side of the loop.  This is the same inside the
 * device loop: a setting of a tracked stream, like vnect_track_view3d -- NOT a fourth action of vnect_track_policy.
 * vnect_track_redetect (src/hog_box.py:26-31, 48-58): while enable != 0, the next box of a tracked frame that the stream's loss rule
 * (vnect_track_policy: hold or reset) declares lost is that frame's largest grouped detection through cal_rect, or the whole frame when
 * nobody is found -- computed on the device behind the frame's box stage, by the rule of vnect_amd/csrc/hog.h, with no host wait.  `spec`
 * (NULL: defaults) as in vnect_hog_detect_device, but max_hits defaults to 4096 and may not exceed it.  A frame with more than max_hits
 * hits cannot fail the call as the host loop does: its next box is the whole frame and its status says overflow.  While set, the stream's
 * frames come through vnect_submit_tracked_device, _device_draw or _device_preview; vnect_submit_tracked, _pinned and _pinned_nv12 return
 * VNECT_E_ARG.  VNECT_E_STATE: no detector set; before vnect_finalize; a tracked frame of the stream in flight.  VNECT_E_ARG: what
 * vnect_hog_detect_device refuses of a spec; max_hits above 4096; a picture side above VNECT_HOG_MAX_SIDE (here, or in the
 * vnect_track_begin that brings it); a handle on which vnect_track_begin is refused.  enable == 0 switches the setting off (spec ignored).
 * vnect_result_redetect (src/hog_box.py:28-31): the verdict on the frame vnect_collect_tracked delivered last, from its own result slot --
 * *status 0: no detection ran (not lost, not set, or a refused crop), 1: found, 2: nobody found, 3: more than max_hits hits; rect4 (may be
 * NULL): the chosen detection before cal_rect, zeros unless found; *hits (may be NULL): the full number of hits, 0 when none ran. */
int vnect_track_redetect(vnect_handle* h, int stream, const vnect_hog_spec* spec, int enable);
int vnect_result_redetect(vnect_handle* h, int32_t* status, int32_t rect4[4], int32_t* hits);

/* ABI v7, additive.  People mode: several persons of ONE video on one handle, one submit per frame (PEOPLE.md).  The reference has no
 * counterpart: src/hog_box.py:26-31 keeps the biggest rectangle, and run_estimator_ps.py:80-109 follows that one person.  Here person p
 * (0 .. n-1, n <= VNECT_MAX_STREAMS) is video stream p: each person's loop is that loop -- its own filter bank, box, loss rule
 * (vnect_track_policy) and 3-D view (vnect_track_view3d) -- and every person's results are bit for bit those of a tracked stream on a
 * handle of its own fed the same clean frames from the same first rect.
 * Called before vnect_finalize, with n in 1 .. VNECT_MAX_STREAMS and pair 0 or 1.  pair = 1 with n >= 2 and 2 S <= VNECT_MAX_SCALES makes
 * finalize build the (2 S)-image launch plan per lane (as vnect_set_stream_batch(h, 2) does), and two persons' crops then go through ONE conv
 * stack; with 2 S > VNECT_MAX_SCALES the people run singly, which is not an error.  VNECT_E_STATE after finalize or on a preprocess_only
 * handle; VNECT_E_ARG for n or pair out of range, on a pyramid-sharded handle, and together with vnect_set_stream_batch(h, 2).
 * On a people handle vnect_track_redetect is refused (VNECT_E_ARG: its pick takes the largest detection, which could be another person);
 * vnect_track_begin / vnect_submit_tracked* stay legal and run one person on the S-image plan. */
int vnect_set_people(vnect_handle* h, int n, int pair);
/* vnect_track_begin for streams 0 .. n-1 (the start of each person's loop, run_estimator_ps.py:80-109), all or nothing: rects holds 4 n values,
 * (x, y, w, h) per person, or is NULL for the whole frame for everyone.  The rect rules, the fallback and the refusals are
 * vnect_track_begin's; VNECT_E_STATE while any of those streams has a frame in flight; VNECT_E_ARG for n outside 1 .. vnect_set_people's n. */
int vnect_people_begin(vnect_handle* h, int n, int H, int W, const int32_t* rects);
/* The next frame for persons 0 .. n-1 (one pass of run_estimator_ps.py:80-109 per person): the WHOLE frame in a resident slot, or in device
 * memory (every format, layout and orientation vnect_submit_tracked_device accepts).  Pinned sources are not supported in people mode.
 * A frame of n persons is ceil(n / 2) lane units on a handle with the pair plan -- persons (0, 1) and (2, 3) share a conv stack, an odd last
 * person runs singly -- and n units without it.  Atomic, like vnect_submit_streams: that every stream tracks the submitted (H, W), that none
 * is stopped, both timestamps for every stream (VNECT_E_TIMESTAMP / VNECT_E_TIMEORDER), that the units in flight stay within the limit
 * (max(lanes, 2); a frame submitted while nothing is in flight is always accepted) and that the results in flight plus n stay within the
 * result ring (8) are all checked before anything changes.
 * style (may be NULL): as in vnect_submit_tracked_device_draw, for every person, in person order, and only after every person's crop has
 * been read from the clean frame; the frame is written until the LAST person has been collected.
 * preview_spec (may be NULL): the frame's ONE picture, as in vnect_submit_tracked_device_preview but with every person in it -- a tap of the
 * annotated picture is band p over limbs p over ..., for p = n-1 down to 0, over the source pixel: n applications of the overlay's rule in
 * person order -- computed from the clean frame before anything is drawn; a person whose crop was refused is left out.  The frame itself
 * is drawn into only where `style` is given (draw_frame of the spec is not read); with style NULL the picture uses the reference's style.
 * vnect_result_preview is valid after the LAST person's delivery of the frame.
 * Results come back through vnect_collect_tracked, n deliveries in person order; vnect_result_confidence and vnect_result_view3d belong to
 * each delivery. */
int vnect_submit_people(vnect_handle* h, int n, int slot, double t2d, double t3d);
int vnect_submit_people_device(vnect_handle* h, int n, const vnect_device_frame* frame, void* producer_stream, double t2d, double t3d,
                               const vnect_overlay_style* style, const vnect_preview_spec* preview_spec);
/* Of the people frame submitted last (each one pass of run_estimator_ps.py:80-109 per person): how many lane units it took, and how many
 * of those were paired conv stacks. */
int vnect_result_people(vnect_handle* h, int32_t* units_out, int32_t* paired_out);

/* ABI v7, additive.  The 3-D view (VIEW3D.md).  The reference's frame loop shows a second picture per frame: it puts joints_3d into
 * q_joints (run_estimator_ps.py:90, 124-126) and a second process plots the skeleton with matplotlib (src/utils.py:272-304: axes limits
 * -500 .. 500, view_init(-90, -90), one line of width 3 per limb; :317-330).  Here one launch of view3d.hip renders that picture into
 * device memory, by the rule of vnect_amd/csrc/view3d.h -- this project's own (orthographic, round caps, no anti-aliasing, no axes):
 * matplotlib's Agg lines cannot be pinned.
 * vnect_view3d_spec: src/utils.py:277-280 and 289 as a structure.  A zero field or a cleared has_* flag means its default -- rows x cols 400 x 400 (each at most
 * VNECT_VIEW3D_MAX), extent 500.0 (the axes' set_xlim/ylim/zlim(-500, 500)), view the identity (view_init(-90, -90): +x right, +y down, +z
 * away from the camera; row-major 3 x 3, (u, v, d) = view (x, y, z)), line_width 3.0 (linewidth=3), background white, colors the ten-entry
 * colour cycle by limb index, parents the reference's (src/estimator.py joint_parents); min_confidence as in vnect_overlay_style, NaN for
 * none (it needs confidences); out_format VNECT_PIX_BGR or VNECT_PIX_RGB, packed 3 bytes per pixel; order 0 -- a limb of a higher index
 * lies over one of a lower (src/utils.py:289, 298 add line 0 first) -- or 1 -- the nearer limb lies on top.  spec NULL: all defaults.
 * vnect_view3d_device (src/utils.py:283-304): the view of joints_3d (21 x 3 float32, host memory: what vnect_infer returns) into `out`,
 * rows out_pitch >= 3 * cols bytes apart; every pixel is written and no byte outside the 3 * cols bytes of each row is.  `out` is device
 * memory of the handle's device (its last byte must lie inside its allocation) or host memory (the library stages and copies), as in
 * vnect_preview_device; the call is done on return.  Needs no weights: it works before vnect_finalize, on a preprocess_only handle and
 * on batched and sharded handles.  VNECT_E_ARG, before anything is launched or written: a wrong struct_size; rows or cols outside
 * 1 .. VNECT_VIEW3D_MAX; out_pitch < 3 * cols; a non-finite or non-positive extent; a non-finite view entry; a line_width outside
 * (0, 64]; a colour outside 0 .. 255; a parent outside 0 .. 20; an order or out_format outside its two values; an `out` that is neither
 * such device memory nor host memory.
 * vnect_track_view3d (run_estimator_ps.py:90 inside the tracked loop): a setting of tracked stream `stream`, like vnect_track_policy.
 * While set, EVERY tracked submit on that stream -- vnect_submit_tracked, _pinned, _pinned_nv12, _device, _device_draw, _device_preview --
 * also renders the frame's view: one launch on the frame's lane stream behind its joints stage and in front of its completion, joints_3d,
 * status and (with a threshold) confidences read from the frame's result-ring slot on the device, then the view's copy into a pinned host
 * buffer the handle owns, one per result-ring slot.  spec NULL turns the setting off.  VNECT_E_STATE while frames are in flight on the
 * handle; VNECT_E_ARG for a bad stream or spec.  A frame whose crop was refused has no view.  Joints, rects, confidences and filter
 * states of every frame are bit-identical to the same loop without the setting.
 * vnect_result_view3d (src/utils.py:317-330: what the plot process shows): the view of the frame most recently delivered by
 * vnect_collect_tracked -- *data, hw = (rows, cols), *pitch = 3 * cols -- valid until the next submit on the handle; hw = (0, 0) and
 * *data = NULL if that frame has none. */
#define VNECT_VIEW3D_MAX 2048
typedef struct vnect_view3d_spec {
    int32_t struct_size;        /* = sizeof(vnect_view3d_spec) */
    int32_t rows, cols;         /* 0: 400 */
    double extent;              /* 0: 500.0 */
    double view[9];
    int32_t has_view;           /* 0: the identity */
    int32_t has_background;     /* 0: (255, 255, 255) */
    double line_width;          /* 0: 3.0 */
    int32_t background_bgr[3];
    int32_t has_colors;         /* 0: the colour cycle */
    int32_t colors_bgr[VNECT_JOINTS][3];
    int32_t parents[VNECT_JOINTS];
    int32_t has_parents;        /* 0: the reference's */
    double min_confidence;
    int32_t out_format;         /* VNECT_PIX_BGR | VNECT_PIX_RGB */
    int32_t order;              /* 0 | 1 */
} vnect_view3d_spec;
int vnect_view3d_device(vnect_handle* h, const float* joints_3d, const double* confidence21, const vnect_view3d_spec* spec, void* out, int64_t out_pitch);
int vnect_track_view3d(vnect_handle* h, int stream, const vnect_view3d_spec* spec);
int vnect_result_view3d(vnect_handle* h, const uint8_t** data, int32_t hw[2], int64_t* pitch);

/* Orientation (ABI v7, additive; ORIENTATION.md).  The reference's loop has a `T` option for a camera that is mounted sideways: it turns
 * every frame with np.rot90(frame, 3) before the crop (run_estimator_ps.py:57-62, 81-85; commented out beside it, an np.transpose
 * variant).  Here the turn happens on the device, inside the copy that brings the crop into the slot, so only the crop moves.
 * An orientation is a code o in 0 .. 7: the oriented picture of a stored (H, W) frame f is
 *     g = np.rot90(f, o & 3);  if o & 4: g = g[:, ::-1]
 * (0: as stored, the default; 3: the reference's T; 7: its np.transpose variant; 6: upside down; 4: a mirror).  Its size is (H, W) for an
 * even o & 3 and (W, H) for an odd one.
 * vnect_set_orientation sets the code for every frame SUBMITTED FROM NOW ON, through every entry point that takes a frame: vnect_infer,
 * vnect_upload_frame, vnect_preprocess, their _nv12 / _nv12_rect / _device kin, and -- through the stream, below -- the tracked submits.
 * Frames already in flight keep theirs.  The entry points keep taking the frame as it is STORED (H, W and the strides describe memory);
 * everything else the caller gives or gets is in ORIENTED coordinates: rects, the tracked box, vnect_track_begin's (H, W), rect_used,
 * joints_2d, and what vnect_draw_device draws.  Every result is bit-identical to the same entry point given the contiguous oriented copy
 * of the frame (NV12: of the converted BGR frame; the chroma of an oriented pixel is that of the stored pixel it comes from).
 * A resident slot holds the oriented frame from its upload on.  A tracked stream remembers the code in force at its vnect_track_begin and
 * its submits use that one, so two videos with different orientations can share a handle; a stored frame whose oriented size is not the
 * track's is refused as a wrong size is.  Works on a preprocess_only handle and before vnect_finalize.  VNECT_E_ARG: a code outside
 * 0 .. 7; a pyramid-sharded handle.  Under a code other than 0, an NV12 draw target is refused with VNECT_E_ARG. */
int vnect_set_orientation(vnect_handle* h, int orientation);

/* Replaces VNectEstimator.joint_filter(joints, dim) (src/estimator.py:83-95) on its own: the handle's 2-D (dim 2: 21x2)
 * or 3-D (dim 3: 21x3) OneEuro bank applied to caller-supplied joints at timestamp t (the reference reads time.time() once
 * per call, :84).  Values travel as float64; values_are_f32 = 1 says they are numpy float32 scalars -- what the reference
 * feeds the 3-D bank (:91-93) -- so numpy's scalar promotion rules (vnect_config::numpy_promotion) decide the arithmetic.
 * Same timestamp errors as vnect_infer.  The filter state lives on the device; this runs one tiny kernel. */
int vnect_joint_filter(vnect_handle* h, int dim, const double* joints_in, int values_are_f32, double t, double* joints_out);

/* New filters, as constructing a fresh VNectEstimator would (src/estimator.py:46-52). */
int vnect_reset_filters(vnect_handle* h);

/* Layer output of the last vnect_forward / vnect_infer, by reference scope name ("conv1", "pool1",
 * "res2a_branch2a", block outputs "res2a".."res5a", "res5c_branch2a_feat", "res5c_branch2c", ...).
 * Writes N,H,W,C to shape4 and up to capacity floats (dense NHWC, padding channels stripped).
 * A tensor of the plan that none of its launches writes -- "conv1" where the fused stem runs, "pool1" too where the stem also runs
 * res2a_branch2a + res2a_branch1 -- is refused with VNECT_E_STATE and a message naming it (its buffer holds nothing); a name the plan
 * never created (the inner layer of a fused tail launch among them) is VNECT_E_ARG as before.
 * Parity/debug aid; not on the hot path. */
int vnect_read_activation(vnect_handle* h, const char* name, float* out, int64_t capacity, int32_t* shape4);

typedef struct vnect_timings {
    int32_t struct_size;
    int32_t frames;            /* profiled frames since the last vnect_reset_timings                              */
    double total_ms;           /* HIP events around the whole frame (pre + conv stack + post), summed over frames  */
    double net_ms;             /* first conv kernel start .. last conv kernel end (device clock), summed           */
    double conv_ms;            /* sum of the conv kernels' own durations (device clock, like rocprofv3), summed    */
    int32_t conv_launches;     /* conv kernel launches per frame                                                   */
    double conv_flops;         /* algorithmic conv FLOPs per frame (2*MAC, live graph)                             */
    double conv_slot_ms;       /* sum over the conv kernels of the slot each one occupies on the stream: its start to the
                                  start of the kernel behind it (own duration + median boundary where another kind of
                                  kernel follows).  rocprofv3's per-kernel durations abut the same way (dispatch ->
                                  completion), so this is the figure its --stats average agrees with.  Summed.          */
    /* ABI v6 (a caller compiled against v5 passes the shorter struct_size and gets the fields above): the shader clock the chip HELD
     * while the conv launches of the profiled frames ran -- workgroup 0 of every conv launch stamps the shader-cycle counter
     * (s_memtime) and the 100 MHz clock (s_memrealtime) at its start and its end; clock [MHz] = 100 * shader_cycles / shader_ticks.
     * What an N > 1 run needs to tell a clock-limited rank (eight GPUs sharing a node's power) from a host-limited one.              */
    double shader_cycles;      /* sum over conv launches and profiled frames of workgroup 0's span in shader cycles                */
    double shader_ticks;       /* the same spans in 100 MHz ticks                                                                  */
} vnect_timings;
/* Profiling replays a twin of the frame graph in which every conv kernel stamps its start and end with the
 * 100 MHz device clock (s_memrealtime); off by default, no cost when off. */
int vnect_set_profiling(vnect_handle* h, int on);
int vnect_get_timings(vnect_handle* h, vnect_timings* out);
int vnect_reset_timings(vnect_handle* h);

/* Per-layer launch plan: fills name (<=63 chars + NUL) and the numbers for layer idx; returns
 * VNECT_E_ARG when idx is past the last layer. */
typedef struct vnect_layer_info {
    char name[64];
    int32_t M, N, K;           /* implicit-GEMM view                                              */
    int32_t tile_m, tile_n, split_k, workgroups;
    double flops;              /* algorithmic                                                     */
    double last_ms;            /* kernel duration in the last profiled frame, device clock (0 if none) */
} vnect_layer_info;
int vnect_get_layer_info(vnect_handle* h, int idx, vnect_layer_info* out);
/* ABI v7.  The same for the batched plan of vnect_set_stream_batch(h, 2) (VNECT_E_STATE without one); last_ms is from the last batch
 * submitted while profiling.  Its counterpart in the reference is the batch dimension of the one graph (src/estimator.py:100-104). */
int vnect_get_batch_layer_info(vnect_handle* h, int idx, vnect_layer_info* out);
/* Additive (the version and vnect_layer_info stay): the rows layer idx of the plan (batch != 0: of the batched plan) COMPUTES.  That is
 * vnect_layer_info::M for every launch but a live-rows one -- a tail launch whose output only stride-s 1x1 convs read computes the pixels
 * (s y, s x) alone and keeps M, tile and workgroups of the full grid; vnect_layer_info::flops and vnect_timings::conv_flops count the
 * computed rows.  live_rule_stride (may be NULL): the stride s by the plan rule for this launch, 0 where it does not apply -- the rule's
 * answer, whether or not the launch's kernel form takes the mode. */
int vnect_get_layer_rows(vnect_handle* h, int idx, int batch, int32_t* rows_computed, int32_t* live_rule_stride);
/* Raw 100 MHz device-clock stamps of layer idx in the last profiled frame (tuning aid): [0] earliest workgroup start,
 * [1..8] latest workgroup ends, [9..13] workgroup 0: start, operands requested, first chunk in LDS, K loop done,
 * stores done; [15] start of the last-dispatched workgroups; [16..18] shader-clock cycles producer wave 0 of workgroup
 * 0 spent waiting for landings / at the barrier / issuing; [19] cycles consumer wave 0 waited at the barrier.  (24 values:
 * the shader-clock stamps of ABI v6 are reported through vnect_timings, not here.) */
int vnect_get_layer_stamps(vnect_handle* h, int idx, uint64_t* out24);

/* Pyramid sharding over RCCL (one scale per rank; BASELINE.json configs[3]).  A handle created with
 * pyramid_nranks == num_scales runs gen_input_batch and the conv stack for scale `pyramid_rank` only (the S
 * images of the batch are independent through the net, src/estimator.py:75-80,100-104); its (46,46,84) maps are
 * all-gathered (ncclAllGather, 710 976 B per rank) and every rank finishes the post-processing, so every rank
 * returns the same joints.  All ranks must be fed the same frame and timestamps.  unique_id is an ncclUniqueId
 * (128 bytes) made by rank 0 with vnect_comm_unique_id and distributed by the host (torch.distributed / files).
 * vnect_comm_init must be called once, after vnect_create and before the first inference.  vnect_forward on such a
 * handle takes ONE image (its scale). */
int vnect_comm_unique_id(void* id128);
int vnect_comm_init(vnect_handle* h, int rank, int nranks, const void* id128);
/* Which RCCL the library resolved, and how: the file ncclAllGather lives in (dladdr) goes to path_out (NUL-terminated, truncated to
 * capacity); *reused_out = 1 when a copy the process had mapped already was reused -- the caller's torch.distributed "nccl" backend
 * loads torch's bundled librccl.so; the reference has no counterpart (its one process owns one TF session,
 * run_estimator_ps.py:35-36, 120-129) -- and 0 when the library opened librccl.so.1 itself.  VNECT_RCCL_LIB overrides the choice.
 * Loads RCCL if it is not loaded yet (VNECT_E_COMM if there is none). */
int vnect_comm_library(char* path_out, int capacity, int32_t* reused_out);
/* The same exchange by plain peer writes over xGMI instead of RCCL (vnect_config::exchange = VNECT_XCHG_P2P; SURVEY 8e asks for
 * both, measured side by side: 711 KB per rank is ~4.6 us of wire time, a collective's launch + sync latency is tens of us).
 * Every rank exports a 128-byte blob describing its exchange block (IPC memory handle + the address inside the exporting
 * process), the host distributes the blobs (torch.distributed all_gather_object / files), and vnect_comm_p2p_init(rank, nranks,
 * blobs[nranks * 128]) maps the peers' blocks (hipIpcOpenMemHandle across processes; hipDeviceEnablePeerAccess when the peer
 * handle lives in this process).  Per frame one kernel stores the rank's maps into every peer's block, publishes a per-rank flag
 * and gathers the peers' slots; a peer that does not show up within ~2 s makes the frame fail with VNECT_E_COMM, never hang. */
int vnect_comm_p2p_export(vnect_handle* h, void* blob128);
int vnect_comm_p2p_init(vnect_handle* h, int rank, int nranks, const void* blobs);

#ifdef __cplusplus
}
#endif
#endif
