// kernels.h -- argument blocks and launchers shared by the HIP kernels and the host runtime.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tables.h"

namespace vnect {

// element format of the activations and the packed weights: what the small launchers' `el` argument takes (the conv and stem launches
// say it as bf16 = "16-bit elements" plus f16 = "they are fp16")
enum { EL_F32 = 0, EL_BF16 = 1, EL_F16 = 2 };

// The one place where a launcher's run-time `el` becomes a C++ element type: f is called with an ElType<T> tag (host code only; any
// value other than EL_F32 / EL_F16 means bf16, as the launchers always took it).
template <typename T>
struct ElType {
    using type = T;
};
template <typename F>
inline auto with_el(int el, F&& f)
{
    return el == EL_F16 ? f(ElType<_Float16>{}) : el != EL_F32 ? f(ElType<__bf16>{}) : f(ElType<float>{});
}

constexpr int MAX_TAPS = 16;
constexpr int ARG_SLABS_MAX = 32;  // upper bound of the arg-max workgroups per joint (post.hip: ARG_SLABS): what the partials' buffer is sized for
constexpr int PROF_WGS = 512;   // end-stamp slots per launch (two workgroups per CU; a power of two: larger grids wrap around)
constexpr int PROF_SLOTS = 28;  // u64 per layer in the profiling buffer: [0] min start, [1..8] max end per id&7, [9..23] tuning stamps
                                // (vnect_get_layer_stamps), [24..26] workgroup 0: shader-clock counter (s_memtime) at its start and at its
                                // end, 100 MHz stamp at its end -- the clock the chip held during the launch (round 6)

// Implicit-GEMM convolution: out[m][n] = sum_k A[m][k] * Wp[n][k],
//   m = (s*Ho + oy)*Wo + ox, k = (tap, ci), A[m][k] = in[s][oy*stride + dy[tap]][ox*stride + dx[tap]][ci]
struct ConvArgs {
    const float* in;
    const float* w;       // packed [phase][Npad][K], K contiguous
    const float* bias;    // [Npad] (zeros when the layer has none)
    const float* scale;   // [Npad] or nullptr: v = (acc + bias) * scale + shift
    const float* shift;
    const float* resid;   // nullptr or same pixel indexing as out
    float* out;
    float* out2;          // second output tensor for columns >= split_n (two layers sharing one input), or nullptr
    float* ws;            // split-K workspace [ksplit][slab_pix][Npad]
    long long slab_pix;   // pixels per slab: out pixels + 64 of slack (the last tile's rows past M land there)
    unsigned long long* prof;  // nullptr, or {min start, ...} of this launch in 100 MHz s_memrealtime ticks
    unsigned long long* prof_end;  // profiling twin: [PROF_WGS] end stamp of every workgroup (plain stores: an atomic max
                                   // over 500 workgroups put ~1.4 us behind every launch); the host takes the maximum
    int S, H, W, Cs;      // input grid, floats per input pixel
    int Ho, Wo, M;        // logical output grid, M = S*Ho*Wo
    int K, ntaps, cpt;    // K = ntaps*cpt*32
    int stride;
    int Npad, Nvalid;
    int ldc, ldr;         // floats per out / resid pixel
    int ldc2, split_n;    // out2 pixel stride; first column of out2 (multiple of the tile width)
    int OH, OW, os;       // out pixel = (s, oy*os + py, ox*os + px) in an (OH, OW) grid
    int nphase;           // 1, or 4 for the transposed conv (py = phase>>1, px = phase&1)
    int ksplit;
    int relu_cols;        // ReLU on columns < relu_cols
    int pixmode;          // conv1: a chunk row is 8 consecutive NHWC4 pixels of one input row (bf16: of two rows)
    int bf16;             // operands and activations are bf16 (accumulators, bias, slabs stay fp32)
    int out_f32;          // bf16 path: this layer writes fp32 (the final maps feed the f64 post-processing)
    int f16;              // with bf16: the 16-bit elements are fp16 (VNECT_FP16), not bf16 -- the same plan, layouts and fused forms
    int tiles_m, tiles_n; // filled by the launcher
    int items;            // work items = tiles_m * tiles_n * nphase * ksplit (launcher; streaming kernel)
    unsigned mg_ks, mg_cpt;  // same for d = ksplit, cpt
    unsigned mg_wo, mg_ho, mg_tn, mg_tm;  // ceil(2^32 / d) for d = Wo, Ho, tiles_n, tiles_m (launcher): x / d == umulhi(x, mg) for x*d < 2^32
    long long w_phase_stride;
    // streaming kernel (buffer-addressed LDS-DMA): the byte offset of a tap from the lane's input pixel is
    // (dy*W + dx)*Cs*esz + tap_bias with tap_bias = -min over taps (so it is >= 0; the descriptor's base is in - tap_bias)
    int tap_bias;
    // filter taps (dy, dx) as 4-bit fields (value + 8, entry [phase*ntaps + tap] at bits 4*entry): the producers decode them
    // with scalar shifts -- no table in the argument block, no dependent scalar load per tap
    unsigned long long dy_pack, dx_pack;
    int tapgrid;  // 1: single tap (0,0); 3: the 3x3 grid with pad 1 (validity masks in closed form); 0: walk the table
    // Tail GEMM (conv_stream_kernel<..., FUSE = 1>; ONE tile per workgroup that holds ALL of the layer's channels: 64x64 tiles for
    // N = 64, 32x128 tiles for N = 128): the layer's own output never reaches HBM -- relu(acc + bias) stays in LDS as a tile and feeds
    // a 1x1 conv `tail_w` (K = the layer's N; in MFMA fragment order, hostplan.h: pack_tail) whose bias / shortcut / ReLU / output are
    // the fields `tail_bias`, resid, relu_cols, out, ldc, Nvalid above describe.  (res2*_branch2b -> res2*_branch2c, res3*_branch2b ->
    // res3*_branch2c, res5c_branch2b -> res5c_branch2c: vnect_model.py:38-41,50-53,56-59,62-103,211-217.)
    const float* tail_w;
    const float* tail_bias;
    int x3;       // 1: split-product form (VNECT_FP32_SPLIT): `w` holds [Npad][K / 32][3 planes][32] bf16 (hostplan.h: pack_split3), the kernel
                  // splits the fp32 activations three ways in registers and multiplies piece by piece on the bf16 matrix pipe
    int bone;     // 1: FUSE = 2 launch of the transposed conv: the bone-length columns 191 .. 211 (+ zero padding) are written here too
    int tail_n;   // 0: no tail; else the 1x1 conv's output channels (64-wide tile: 256 = 2 row halves x 8 column blocks over the 8 waves; 128-wide: up to 512, tail wave tw takes blocks tw, tw + 8)
    // Chain GEMM behind the wide tail (conv.hip: chain_gemm): the tail's output tile -- a bottleneck block's output, 32 pixels x 512
    // channels -- stays in LDS as well and feeds the NEXT block's branch2a (1x1, 512 -> 128, ReLU): `chain_w` (fragment order),
    // `chain_bias`, output `chain_out` ([M][chain_ld]).  res3*_branch2c -> res3(*+1)_branch2a, vnect_model.py:72-103.
    const float* chain_w;
    const float* chain_bias;
    float* chain_out;
    int chain_n;  // 0: none; else 128
    int chain_ld;
    // Live rows (rt_plan.cpp: the plan rule is plan::live_rows_stride): every reader of this tail launch's output is a 1x1 conv of stride
    // live_s > 1, so only the pixels (s oy', s ox') are computed, read as shortcut and stored; M, Ho, Wo above stay the full grid's (the
    // recorded plan and the launch's grid), the launcher derives the live grid.  0: off.
    int live_s;
};

struct ReduceArgs {  // split-K second pass: out = epilogue(sum_ks ws[ks])
    const float* ws;
    long long slab_pix;  // pixels per slab (ConvArgs::slab_pix)
    const float* bias;
    const float* scale;
    const float* shift;
    const float* resid;
    float* out;
    long long npix;
    int Npad, Nvalid, ldc, ldr, ksplit, relu_cols;
    int bf16, out_f32, f16;  // (as in ConvArgs)
};

// Write-through (`sc1`) vector stores for the small kernels between the conv launches: like the conv epilogue's, their output
// leaves the L2 while the kernel runs instead of in the write-back at the kernel boundary the next launch waits behind.
#if defined(__HIP_DEVICE_COMPILE__)
template <typename V>
__device__ __forceinline__ void store_wt(V* p, V v)
{
    static_assert(sizeof(V) == 16 || sizeof(V) == 8, "one dwordx4 / dwordx2 store");
    // (the s_nop: gfx9 requires wait states between a VMEM store of more than 64 bits and a VALU write of its data registers;
    // the compiler inserts them for its own stores but cannot see inside an asm block -- a thread that went on computing
    // right behind such a store stored the next iteration's loop counter instead of its data: found in round 2)
    if constexpr (sizeof(V) == 16) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 2" ::"v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
#else
template <typename V>
__device__ __forceinline__ void store_wt(V* p, V v) { *p = v; }
#endif

hipError_t launch_conv(const ConvArgs& a, int BM, int BN, int KG, hipStream_t st);  // KG: in-workgroup K groups (1, 2, 4)
hipError_t launch_reduce(const ReduceArgs& a, hipStream_t st);
hipError_t conv_setup();  // one-time function attributes (dynamic LDS size)
bool conv_deconv96_available();  // after conv_setup: the 64x96x2 three-accumulator instantiations fit the register file
int conv_cu_count();             // after conv_setup: compute units of the device (what a "round over the chip" is counted in)
// compile-time probe switches of the kernel translation units, as text and as "all at their product values" (vnect_build_info)
const char* conv_build_probes();
bool conv_probes_off();
const char* post_build_probes();
bool post_probes_off();

hipError_t launch_pad3to4(const float* in3, void* out4, long long npix, int el, hipStream_t st);  // el: EL_F32 / EL_BF16 / EL_F16
hipError_t launch_strip4to3(const void* in4, float* out3, long long npix, int el, hipStream_t st);
hipError_t launch_maxpool(const void* in, void* out, int S, int H, int W, int C, int Ho, int Wo, int el, hipStream_t st);
hipError_t launch_bone(void* feat, long long npix, int ld, int el, hipStream_t st);

// ---- pre-processing (the table structs live in tables.h) -------------------------------
struct FrameDyn {     // what does change every frame: passed to the two kernels that need it BY VALUE (kernel arguments),
                      // so a frame costs no host-to-device copy
    double t2d, t3d;
    const uint8_t* frame;  // device pointer
    long long row_stride;
    // pyramid-sharded handle, exchange by peer writes: device word that exchange_kernel sets to the frame's sequence number when a
    // peer's maps did not arrive (nullptr otherwise); post_kernel then skips the joints stage of frame `xseq`
    const unsigned* xfail;
    unsigned xseq;
};

hipError_t launch_pyramid(const FrameParams* fp, FrameDyn dyn, const ScaleTabs* tabs, void* batch4, int S, int scale_base, int el, hipStream_t st);
// two streams' frames into one (2 S)-image batch: images 0 .. S-1 from (fp0, dyn0), S .. 2 S-1 from (fp1, dyn1) (vnect_submit_streams)
constexpr int VNECT_MAX_IMAGES = 8;  // images of one batch at most (= VNECT_MAX_SCALES: the batched plan needs 2 S <= it)
hipError_t launch_pyramid_streams(const FrameParams* fp0, const FrameParams* fp1, FrameDyn dyn0, FrameDyn dyn1, const ScaleTabs* tabs,
                                  void* batch4, int S, int el, hipStream_t st);

// vnect_infer: H rows of `row` bytes from device-mapped pinned host memory (`stride` bytes apart) into a resident frame slot, as a kernel
hipError_t launch_frame_copy(const uint8_t* src_dev, uint8_t* dst, int H, int row, long long stride, const uint8_t* src_end, hipStream_t st);

// The same from an NV12 frame in device-mapped pinned memory, converted to BGR inside the read (post.hip: nv12_copy_kernel; nv12.h).
struct Nv12Src {
    const uint8_t* y;       // the Y plane's first byte (any alignment), rows y_stride bytes apart
    long long y_stride;
    const uint8_t* uv;      // the interleaved U, V plane's first byte, rows uv_stride bytes apart
    long long uv_stride;
    const uint8_t* lo;      // the pinned buffer both planes lie in, [lo, end): multiples of 4; no dword is loaded outside it
    const uint8_t* end;
    // planes in DEVICE memory (vnect_infer_device), possibly in two allocations: [lo, end) bounds the Y plane's loads, [uv_lo, uv_end) the UV
    // plane's (nullptr: [lo, end) holds both, as above).  `any_bounds`: the bounds are a caller's allocation and need not be multiples of 4 --
    // a dword an end cuts is then assembled from byte loads of the bytes inside
    const uint8_t* uv_lo = nullptr;
    const uint8_t* uv_end = nullptr;
    int any_bounds = 0;
};
// the crop (x, y, w, h) of the frame -> `dst`, rows packed 3 w bytes apart (whole frame: 0, 0, W, H); chroma by absolute coordinates
hipError_t launch_nv12_copy(const Nv12Src& s, int x, int y, int w, int h, uint8_t* dst, hipStream_t st);

// The same from a uint8 frame that already lies in DEVICE memory, in a caller's allocation (post.hip: ingest_copy_kernel; ingest.h).
struct IngestSrc {
    const uint8_t* data;    // pixel (0, 0), channel 0 (any alignment)
    long long stride_y, stride_x, stride_c;  // bytes, all positive: packed-3 (., 3, 1), packed-4 (., 4, 1), planar (., 1, plane), or anything else
    const uint8_t* lo;      // the allocation the frame lies in, [lo, end) at any alignment: no byte outside it is loaded
    const uint8_t* end;
    int order;              // INGEST_BGR / INGEST_RGB: the source's channel order
};
// the crop (x, y, w, h) of the (H, W) frame -> `dst`, rows packed 3 w bytes apart, BGR.  force_generic: the one-pixel-per-lane kernel
// whatever the strides (tests: what the coalesced forms must equal)
hipError_t launch_ingest_copy(const IngestSrc& s, int H, int W, int x, int y, int w, int h, uint8_t* dst, hipStream_t st, int force_generic = 0);

// ---- the stem as one launch (stem.hip): [gen_input_batch ->] conv1 + ReLU -> 3x3 / stride-2 max-pool on spatial tiles -------------
struct StemArgs {
    const void* batch;     // (S,368,368,4) NHWC4 batch (fp32 / bf16), or nullptr with from_frame
    const FrameParams* fp; // from_frame: the three arguments of pyramid_kernel
    FrameDyn dyn;
    const ScaleTabs* tabs;
    const float* w;        // conv1's packed weights as the stand-alone layer has them: fp32 [64][7 rows][8 px][4 ch], bf16 [64][4 row pairs][2][8][4]
    const float* bias;     // [64]
    void* out;             // pool1 (S,92,92,64), fp32 / bf16
    // PAIR form (round 3): res2a_branch2a (1x1, 64 -> 64, ReLU) + res2a_branch1 (1x1, 64 -> 256), vnect_model.py:32-35, on the pooled
    // tile while it is in LDS -- pool1 is then never written: weights of both layers side by side in MFMA fragment order
    // (hostplan.h: pack_tail over the concatenated [64][320]), biases [320], the two output tensors (S,92,92,64) / (S,92,92,256)
    const float* pair_w;   // nullptr: no pair
    const float* pair_bias;
    void* pair_out_a;
    void* pair_out_b;
    unsigned long long* prof;      // profiling twin: start stamp (workgroup 0) ...
    unsigned long long* prof_end;  // ... and every workgroup's end stamp, like ConvArgs
    int S, groups;         // images; row groups per image (grid = S * groups * 4 tiles)
    int scale_base;        // from_frame: image 0 of the batch is scale `scale_base` (a pyramid-sharded rank)
    // from_frame with TWO frames (a batch of two video streams, vnect_submit_streams): images 0 .. per_stream-1 come from (fp, dyn) at
    // scales 0 .. per_stream-1, images per_stream .. S-1 from (fp2, frame2, stride2) at the same scales.  per_stream = 0: one frame.
    int per_stream;
    const FrameParams* fp2;
    const uint8_t* frame2;
    long long stride2;
    int bf16, f16, from_frame;  // (bf16, f16 as in ConvArgs)
    int dbg;               // tuning only (VNECT_STEM_DBG): 1 = no conv blocks, 2 = no pooling, 4 = no patch (timing breakdowns; wrong results)
    unsigned char row0[STEM_MAXGROUPS + 1];  // first pooled row of every group; row0[groups] = 92
};
hipError_t launch_stem(const StemArgs& a, hipStream_t st);
hipError_t stem_setup();  // one-time function attributes (dynamic LDS size)

// ---- post-processing ------------------------------------------------------------------
struct ArgPartial {
    double v;
    int idx;
    int pad_;
};
struct Filt {  // OneEuroFilter + its two LowPassFilters
    double freq, mincutoff, beta, dcutoff;
    double lasttime;
    double x_y, x_s, dx_y, dx_s;
    int has_last, x_init, dx_init, pad_;
};
struct FilterBank {
    Filt f2[NJ][2];
    Filt f3[NJ][3];
};
struct JointsOut {
    double j2d[NJ * 2];
    float j3d[NJ * 3];
    int status;
};
// Per-joint confidence (CONFIDENCE.md), per result-ring slot beside JointsOut (device-mapped pinned host memory): conf[j] is the value of
// the element np.argmax picks in utils.py:169-172 -- the maximum of the x8 upsample of joint j's merged heat-map, the `bv` that wins
// the arg-max (NaN cells never win; an all-NaN map gives -inf).  It comes from the frame's raw maps: the filters do not touch it.
// lost / confident: the box stage's verdict on a tracked frame under the stream's TrackPolicy (0 / 0 on an untracked frame).
struct ConfOut {
    double conf[NJ];
    int lost;
    int confident;
};
// The loss rule of a tracked stream, device memory (vnect_track_policy): confident = #{j : conf[j] >= min_confidence},
// lost = action != 0 && confident < min_joints.
enum { TRACK_LOST_OFF = 0, TRACK_LOST_HOLD = 1, TRACK_LOST_RESET = 2 };
struct TrackPolicy {
    double min_confidence;
    int min_joints;
    int action;  // TRACK_LOST_OFF: today's loop; HOLD: the next frame is cropped with this frame's crop; RESET: with the whole frame
};

// merge + arg-max + joints in ONE launch: the last of the 168 arg-max workgroups (agent-scope ticket, zero between launches) runs the
// joints stage.  conf: the frame's ConfOut (like `out`, pinned host memory) or nullptr; conf_dev: nullptr, or NJ doubles of device memory
// that get the confidences too (what a box stage launched behind this reads)
hipError_t launch_post(const float* maps, MergeGeo geo, ArgPartial* part, unsigned* ticket,
                       FilterBank* fb, const FrameParams* fp, FrameDyn dyn, int nep50, JointsOut* out, hipStream_t st,
                       ConfOut* conf = nullptr, double* conf_dev = nullptr);
// multi-scale merge of the heat-maps (in LDS, the rows each workgroup needs) + arg-max of the virtual x8 upsample
hipError_t launch_argmax(const float* maps, MergeGeo geo, ArgPartial* part, hipStream_t st);
// out may be (device-mapped) pinned HOST memory: the kernel's 21x2 + 21x3 results then need no device-to-host copy
hipError_t launch_joints(const ArgPartial* part, const float* maps, MergeGeo geo, FilterBank* fb,
                         const FrameParams* fp, FrameDyn dyn, int nep50, JointsOut* out, hipStream_t st,
                         ConfOut* conf = nullptr, double* conf_dev = nullptr);  // (conf, conf_dev: as launch_post)

// ---- pyramid sharding: the exchange by peer writes (SURVEY 8e "plain peer writes ... into the gather buffer") -----------
// Every rank owns one exchange block [2 parities][nranks slots][XCHG_MAPS floats] + flags[2][8] (u32, one 128-B line per
// parity), reachable by every peer (IPC-mapped across processes, hipDeviceEnablePeerAccess inside one).  One launch per frame:
// workgroup (peer p, chunk c) stores chunk c of this rank's maps into slot `rank` of p's block (16-B system-scope
// write-through stores over xGMI), the last chunk-workgroup per peer publishes flags_p[parity][rank] = seq behind a
// system-scope release; then the same workgroup waits (bounded) for flags_local[parity][p] == seq and copies p's slot from the
// local block into the handle's plain gather buffer, which the post-processing kernels read.  Two parities: a rank can run at
// most one frame ahead of a peer (it needs the peer's maps of frame k to finish frame k).
constexpr int XCHG_MAPS = HM * HM * MAPC;   // 177 744 floats = 710 976 B per rank and frame
constexpr int XCHG_CHUNKS = 8;              // workgroups per peer
constexpr size_t XCHG_FLAG_OFF = (size_t)2 * 8 * XCHG_MAPS * sizeof(float);  // byte offset of the flags in an exchange block
constexpr size_t XCHG_BYTES = XCHG_FLAG_OFF + 2 * 128;
struct XchgArgs {
    const float* src;        // this rank's (46,46,84) maps
    char* block[8];          // every rank's exchange block as THIS device addresses it (block[rank] is the local one)
    float* gather;           // local (nranks, 46,46,84): what the merge / arg-max / joints kernels read
    unsigned* tickets;       // local, [8]: chunk-workgroups of a peer that have finished their stores
    int* status;             // device-mapped pinned host word (one per result-ring slot): set to 1 if a peer's flag did not arrive within the bound
    unsigned* dfail;         // device word: set to `seq` in that case (what post_kernel tests, FrameDyn::xfail)
    int rank, nranks, parity;
    unsigned seq;            // frame sequence number (> 0), the flag value
    unsigned spin_limit;     // polls before giving up (each ~1 us)
};
hipError_t launch_exchange(const XchgArgs& a, hipStream_t st);

// ---- the tracking loop on the device (track.hip; vnect_track_begin / vnect_submit_tracked) ------------------------------------
// run_estimator_ps.py:80-109 (runner.track) keeps the crop box on the host: frame t+1's crop comes from frame t's joints.  Here it stays
// on the device: a box kernel behind the joints stage turns a frame's joints into the next crop and its squarify geometry (crop.h).
struct TrackState {   // per video stream, device memory: the crop of the stream's NEXT tracked frame
    int x, y, w, h;   // the crop (after the fallback to the whole frame, clipped to the frame)
    int uw, uh;       // the rect's extent as reported (rect_used): an initial rect past the frame's far edges is cropped the way numpy
                      // slicing crops it (runner.track), but reported as given
    int H, W;         // the frame's size
    int status;       // SQ_OK, or why squarify refuses the crop (crop.h); sticky until vnect_track_begin
    unsigned fail;    // FrameDyn::xfail word: the number of the tracked frame whose joints stage is to be skipped
    FrameParams fp;   // the crop's squarify geometry
};
struct TrackOut {     // per result-ring slot, device-mapped pinned host memory
    int rect[4];      // the rect the frame was cropped with
    int status;       // SQ_OK, or the refusal of that crop (the frame's joints stage was skipped)
    int pad_;
};
// the pyramid of a tracked frame: the crop origin (and, `packed`, the row stride of a crop copied out of a pinned buffer) from the
// stream's state instead of FrameDyn::frame; geometry ts->fp
hipError_t launch_pyramid_track(const TrackState* ts, FrameDyn dyn, int packed, const ScaleTabs* tabs, void* batch4, int S, int el, hipStream_t st);
// the same for two streams whose states are ts2[0] and ts2[1], into one (2 S, 368, 368, 4) batch: images 0 .. S-1 from (ts2[0], dyn0),
// S .. 2 S-1 from (ts2[1], dyn1); 2 S <= VNECT_MAX_IMAGES (people mode: vnect_submit_people)
hipError_t launch_pyramid_track_pair(const TrackState* ts2, FrameDyn dyn0, FrameDyn dyn1, int packed, const ScaleTabs* tabs, void* batch4, int S, int el,
                                     hipStream_t st);
// the crop's rows (rect from the stream's state) out of a pinned frame of H rows into `dst`, packed; grid sized for the whole frame
hipError_t launch_frame_copy_track(const TrackState* ts, const uint8_t* src_dev, uint8_t* dst, int H, int W, long long stride, const uint8_t* src_end,
                                   hipStream_t st);
// the same out of a pinned NV12 frame of (H, W) pixels, converted to BGR on the way
hipError_t launch_nv12_copy_track(const TrackState* ts, const Nv12Src& s, uint8_t* dst, int H, int W, hipStream_t st);
// the same out of an (H, W) frame in device memory (H <= 65535)
hipError_t launch_ingest_copy_track(const TrackState* ts, const IngestSrc& s, uint8_t* dst, int H, int W, hipStream_t st, int force_generic = 0);
// The oriented copies (orient.hip; orient.h; ORIENTATION.md): the crop (x, y, w, h) -- in ORIENTED coordinates -- of an (H, W) frame that is
// stored rotated / mirrored by code o (1 .. 7; 0 stays with the copies above) -> `dst`, rows packed 3 w bytes apart, BGR.  One source
// block for every form: pinned or device BGR / RGB at any strides, NV12 in one or two allocations.
struct OrientSrc;
hipError_t launch_orient_copy(const OrientSrc& s, int o, int H, int W, int x, int y, int w, int h, uint8_t* dst, hipStream_t st);
// the same with the rect from the stream's state; grid sized for the whole oriented frame
hipError_t launch_orient_copy_track(const TrackState* ts, const OrientSrc& s, int o, int H, int W, uint8_t* dst, hipStream_t st);
// behind the joints stage of tracked frame `xseq`: joints to frame coordinates (in `out`), rect_used + status to `tout`, the next crop and
// its geometry to `ts`.  conf_dev: the frame's NJ confidences in device memory (launch_post / launch_joints left them there), pol: the
// stream's loss rule (device memory), conf: the frame's ConfOut, which gets lost / confident -- all three or none (no rule: today's loop)
// gate (here and in launch_post_track): nullptr, or the re-detection word of the stream (vnect_track_redetect): 1 when the rule calls the
// frame lost, else 0
hipError_t launch_track_box(TrackState* ts, JointsOut* out, TrackOut* tout, unsigned xseq, hipStream_t st, const double* conf_dev = nullptr,
                            const TrackPolicy* pol = nullptr, ConfOut* conf = nullptr, int* gate = nullptr);
// post_kernel with the same box stage as its tail (the last arriver's joints stage hands its frame-coordinate joints -- and the
// confidences -- over in LDS).  conf: the frame's ConfOut or nullptr; pol: the stream's loss rule or nullptr (off)
hipError_t launch_post_track(const float* maps, MergeGeo geo, ArgPartial* part, unsigned* ticket, FilterBank* fb, TrackState* ts, FrameDyn dyn,
                             int nep50, JointsOut* out, TrackOut* tout, hipStream_t st, ConfOut* conf = nullptr, const TrackPolicy* pol = nullptr,
                             int* gate = nullptr);

// ---- the overlay (overlay.hip; vnect_draw_device / vnect_submit_tracked_device_draw; OVERLAY.md) -----------------------------------
// utils.draw_limbs_2d (src/utils.py:222-243; run_estimator_ps.py:92-94) into a frame in device memory, by the rule of overlay.h.  One
// launch; the grid is fixed by the frame's size.  jo / to (both or neither) and co: the tracked form -- joints in frame coordinates,
// rect_used + status and (with a threshold in `in`) confidences are read from a frame's result-ring slot, which the box stage in front of
// this launch filled; a frame whose status is not SQ_OK is not drawn.  Otherwise they come from `in`.  The parents always come from `in`.
struct OverlayTarget;
struct OverlayInput;
hipError_t launch_overlay(const OverlayTarget& t, const OverlayInput& in, const JointsOut* jo, const TrackOut* to, const ConfOut* co, hipStream_t st);

// ---- the preview (preview.hip; vnect_preview_device; PREVIEW.md) ---------------------------------------------------------------------
// run_estimator_ps.py:94-96: the annotated frame scaled for display, by the rule of preview.h.  One launch; the grid is fixed by the
// output's size.  The frame is read, never written; the scaled packed picture goes to a.out.  jo / to / co: as in launch_overlay; a frame
// whose status is not SQ_OK writes nothing.
struct PreviewArgs;
hipError_t launch_preview(const PreviewArgs& a, const OverlayInput& in, const JointsOut* jo, const TrackOut* to, const ConfOut* co, hipStream_t st);
// The people form (people mode; PEOPLE.md): the ONE picture of a frame with P persons (1 .. 4) -- band p over limbs p over ... for
// p = P-1 down to 0 -- each person's joints, rect_used, status and confidences read from its own result-ring slot; `in` carries the style
// only (parents, threshold).  A person whose status is not SQ_OK is left out; the picture is always written.  With P = 1 and status
// SQ_OK it writes launch_preview's bytes.
struct PreviewPeopleIn {
    int P;
    const JointsOut* jo[4];
    const TrackOut* to[4];
    const ConfOut* co[4];  // (all nullptr without a threshold)
};
hipError_t launch_preview_people(const PreviewArgs& a, const OverlayInput& in, const PreviewPeopleIn& pin, hipStream_t st);

// ---- the 3-D view (view3d.hip; vnect_view3d_device, vnect_track_view3d; VIEW3D.md) ----------------------------------------------------
// run_estimator_ps.py:90, 124-126 and src/utils.py:272-304: the skeleton plot of joints_3d, by the rule of view3d.h.  One launch; the grid
// is fixed by the picture's size; every pixel of a.out is written once.  Two forms: j3d (63 floats) and conf (21 doubles, or nullptr
// without a threshold) in device memory; or jo (and co) -- a result-ring slot's JointsOut::j3d and ::status and its ConfOut, read on the
// device: a frame whose status is not 0 writes nothing.  Exactly one of j3d and jo is given.
struct View3dArgs;
hipError_t launch_view3d(const View3dArgs& a, const float* j3d, const double* conf, const JointsOut* jo, const ConfOut* co, hipStream_t st);

// ---- the person detector (hog.hip; vnect_hog_detect_device; HOG.md) --------------------------------------------------------------------
// hog_box.py:24-33: HOG + linear SVM over a pyramid of the oriented picture, by the rule of hog.h.  Three launches cover all levels through
// the level table `lv` (device memory, p.n entries): votes (the level images are computed inside it), block histograms + L2-Hys, window
// scores.  Everything the launches write is workspace the caller owns: votes / bins [p.npix], blocks [p.nblk * 36], hits [max_hits] and
// one counter, which ends as the number of windows that cleared hit_threshold -- only the first max_hits of them are stored.  scores
// (may be null): every window's score [p.nwin].  `stages`: bit 0 votes, bit 1 blocks, bit 2 windows (the product passes 7).
struct HogSrc;
struct HogPlan;
struct HogLevel;
struct HogTables;
struct HogHit;
struct HogDev {
    const HogLevel* lv;
    const HogTables* tab;
    const float* det;  // 3781 floats, rho last
    float2* votes;
    uint8_t* bins;
    float* blocks;
    HogHit* hits;
    unsigned* count;
    float* scores;
};
hipError_t launch_hog(const HogSrc& a, const HogPlan& p, const HogDev& d, double hit_threshold, int max_hits, int stages, hipStream_t st);
// Re-detection inside the tracked loop (vnect_track_redetect; hog.h: THE RULE).  launch_hog_gated: the same three launches WITHOUT the
// counter reset (the caller zeroes d.count in front of them), each returning at once unless *gate (device memory; a tracked frame's box stage wrote it) is 1.  cap > 0: each launch runs at
// most `cap` workgroups, which walk the launch's workgroup indices in a grid-stride loop -- a frame that is not lost then dispatches
// 3 * cap empty workgroups, not the pyramid's; cap 0: the ungated kernels' grids, every workgroup leaving at once.  Gate 1: the outputs of
// launch_hog, whatever the cap.
constexpr int HOG_GATED_CAP = 8192;  // measured (profiles/redetect_rate.txt): gate 0 costs what 1024 costs, gate 1 what the ungated launches cost
hipError_t launch_hog_gated(const HogSrc& a, const HogPlan& p, const HogDev& d, double hit_threshold, int max_hits, int stages, const int* gate, int cap,
                            hipStream_t st);
// launch_hog_pick: one workgroup behind them.  Gate 0: out->status = HOG_RD_NOT_RUN and nothing else.  Gate 1: the hits (d.hits, d.count;
// nlev levels in d.lv) become the stream's next crop by hog.h's rule -- grouped with `threshold` (the spec's (int)final_threshold), the
// largest class through cal_rect, or the whole frame when nobody is found or more than max_hits (<= HOG_TRACK_MAX_HITS) windows hit -- and
// *ts gets that crop the way a box stage commits it (trackbox.h: track_box_commit, for tracked frame `xseq`); `out` gets the verdict.
// cls: 5 * HOG_TRACK_MAX_HITS ints of device memory, zero before the first pick (every pick leaves them zero).
struct RedetectOut;
hipError_t launch_hog_pick(const HogDev& d, int nlev, int max_hits, int threshold, const int* gate, int* cls, TrackState* ts, unsigned xseq, RedetectOut* out,
                           hipStream_t st);

// VNectEstimator.joint_filter alone: bank `dim` of fb over NJ * dim values (float64 carriers; f32vals: they are float32 scalars)
hipError_t launch_filter(FilterBank* fb, int dim, bool f32vals, int nep50, double t, const double* in, double* out, hipStream_t st);

}  // namespace vnect
