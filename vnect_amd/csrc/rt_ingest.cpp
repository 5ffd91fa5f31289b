// rt_ingest.cpp -- frames into slots: validation, staging, ingest.  Every source of a frame -- host BGR, host NV12, a frame in the
// caller's device memory, a pinned buffer named by its index -- has one RESOLVER here, which validates everything the caller gave and
// describes the frame as the copy kernels address it (runtime.h: FrameSrc).  ingest() puts a described frame into a resident slot;
// enqueue_frame (rt_exec.cpp) takes a tracked frame's description and copies only the stream's crop.  A refusal changes nothing.
#include "runtime.h"

namespace vnect {
namespace rt {

// every refusal names its entry point (`who`; nullptr: the host-BGR entry points, whose messages carry none).  Built only when refusing.
static int refuse(vnect_handle* h, const char* who, const char* what)
{
    return fail(h, VNECT_E_ARG, who ? std::string(who) + ": " + what : std::string(what));
}

// ---- the rules the sources share ----------------------------------------------------------------------------------------------------------
// An NV12 frame's planes: even H and W, rows at least W bytes apart; the bytes from each plane's first to its last
static int nv12_planes(vnect_handle* h, const char* who, int H, int W, int64_t y_stride, int64_t uv_stride, size_t* y_span, size_t* uv_span)
{
    if (H < 2 || W < 2 || ((H | W) & 1)) return refuse(h, who, "an NV12 frame needs even W and H (>= 2)");
    if (y_stride < (int64_t)W || uv_stride < (int64_t)W) return refuse(h, who, "y_stride and uv_stride must be at least W");
    *y_span = (size_t)(H - 1) * (size_t)y_stride + (size_t)W, *uv_span = (size_t)(H / 2 - 1) * (size_t)uv_stride + (size_t)W;
    return VNECT_OK;
}
static int nv12_apart(vnect_handle* h, const char* who, const uint8_t* y, size_t y_span, const uint8_t* uv, size_t uv_span)
{
    return y < uv + uv_span && uv < y + y_span ? refuse(h, who, "the UV plane overlaps the Y plane") : VNECT_OK;
}

// r = the crop of an (H, W) frame: the whole frame, or rect4 = (x, y, w, h) clipped at the far edges as numpy slicing clips it; what lands
// in the slot is BGR, 3 bytes per pixel
static int clip_rect(vnect_handle* h, const char* who, const int32_t* rect4, int H, int W, int* r)
{
    r[0] = r[1] = 0, r[2] = W, r[3] = H;
    if (rect4) {
        for (int k = 0; k < 4; k++) r[k] = rect4[k];
        if (r[0] < 0 || r[1] < 0 || r[0] >= W || r[1] >= H) return refuse(h, who, "the rect's origin must lie inside the frame");
        if (r[2] < 1 || r[3] < 1) return refuse(h, who, "the rect must be at least one pixel wide and high");
        r[2] = std::min(r[2], W - r[0]), r[3] = std::min(r[3], H - r[1]);
    }
    if ((size_t)r[2] * r[3] * 3 > (size_t)h->cfg.max_frame_bytes)
        return refuse(h, who, "frame larger than max_frame_bytes (the slot holds BGR: 3 bytes per pixel)");
    return VNECT_OK;
}

// Host memory [p, p + span) as a view of one of the caller's pinned buffers (vnect_frame_buffer): the buffer's index; -1: p lies in
// neither (pageable memory as far as the handle knows); -2: it starts inside one and runs past its end
static int pinned_view(const vnect_handle* h, const uint8_t* p, size_t span)
{
    for (int i = 0; i < 2; i++) {
        const uint8_t* lo = h->stage[i];
        if (lo && p >= lo && p < lo + h->stage_cap[i]) return span <= (size_t)(lo + h->stage_cap[i] - p) ? i : -2;
    }
    return -1;
}
static const uint8_t* pinned_dev(const vnect_handle* h, int i, const uint8_t* p) { return h->stage_dev[i] + (p - h->stage[i]); }
static const uint8_t* pinned_end(const vnect_handle* h, int i) { return h->stage_dev[i] + h->stage_cap[i]; }

// pinned staging buffer i with room for `bytes` (grows in 1-MiB steps; a grown buffer moves, so nothing may be in flight)
int ensure_stage(vnect_handle* h, int i, size_t bytes)
{
    if (h->stage_cap[i] >= bytes) return VNECT_OK;
    HIPCK(h, hipStreamSynchronize(h->st));
    if (h->stage[i]) HIPCK(h, hipHostFree(h->stage[i]));
    h->stage[i] = nullptr, h->stage_cap[i] = 0;
    const size_t cap = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    HIPCK(h, hipHostMalloc((void**)&h->stage[i], cap, hipHostMallocMapped));
    HIPCK(h, hipHostGetDevicePointer((void**)&h->stage_dev[i], h->stage[i], 0));
    h->stage_cap[i] = cap;
    return VNECT_OK;
}

// ---- host BGR (vnect_infer, vnect_submit_tracked_pinned) ------------------------------------------------------------------------------------
// A frame that lies inside one of the caller's pinned buffers (a frame captured there, or a crop of it) is read where it lies; any other
// pointer is first copied by the CPU into the internal stage, rows packed -- behind the last refusal.
int resolve_host_bgr(vnect_handle* h, const uint8_t* bgr, int H, int W, int64_t row_stride, int orient, FrameSrc* out)
{
    if (H < 1 || W < 1 || row_stride < (int64_t)W * 3) return refuse(h, nullptr, "bad frame geometry");
    FrameSrc f;
    int Ho, Wo;
    orient_size(orient, H, W, &Ho, &Wo);
    int rc = clip_rect(h, nullptr, nullptr, Ho, Wo, f.r);
    if (rc) return rc;
    const size_t row = (size_t)W * 3;
    int i = pinned_view(h, bgr, (size_t)(H - 1) * (size_t)row_stride + row);
    f.where = SRC_PINNED_BGR, f.H = H, f.W = W, f.orient = orient;
    if (i >= 0) {
        f.bgr = {pinned_dev(h, i, bgr), (long long)row_stride, pinned_end(h, i)};
    } else {
        i = 2;
        if ((rc = ensure_stage(h, i, (size_t)H * row))) return rc;
        if ((size_t)row_stride == row) memcpy(h->stage[i], bgr, (size_t)H * row);
        else
            for (int y = 0; y < H; y++) memcpy(h->stage[i] + (size_t)y * row, bgr + (size_t)y * (size_t)row_stride, row);
        f.bgr = {h->stage_dev[i], (long long)row, pinned_end(h, i)};
    }
    *out = f;
    return VNECT_OK;
}

// the whole (H, W) frame at the start of pinned buffer `index`, rows row_stride apart
int resolve_pinned_bgr(vnect_handle* h, const char* who, int index, int H, int W, int64_t row_stride, int orient, FrameSrc* out)
{
    if (index < 0 || index > 1 || !h->stage[index]) return refuse(h, who, "no such pinned buffer (vnect_frame_buffer)");
    if (row_stride < (int64_t)W * 3 || pinned_view(h, h->stage[index], (size_t)(H - 1) * (size_t)row_stride + (size_t)W * 3) != index)
        return refuse(h, who, "the frame does not fit the pinned buffer at this row stride");
    FrameSrc f;
    f.where = SRC_PINNED_BGR, f.H = H, f.W = W, f.orient = orient;
    orient_size(orient, H, W, &f.r[3], &f.r[2]);
    f.bgr = {h->stage_dev[index], (long long)row_stride, pinned_end(h, index)};
    *out = f;
    return VNECT_OK;
}

// ---- host NV12 (vnect_infer_nv12 and its kin) -----------------------------------------------------------------------------------------------
// Planes inside ONE of the caller's pinned buffers (a decoder's surface captured there) are read where they lie; the conversion to BGR is
// the copy kernel's (post.hip: nv12_copy_kernel).  With a rect only the crop is converted, and lands at the slot's origin.
static int nv12_pinned(vnect_handle* h, const char* who, const uint8_t* y, int64_t y_stride, size_t y_span, const uint8_t* uv, int64_t uv_stride,
                       size_t uv_span, FrameSrc* f)
{
    const int i = pinned_view(h, y, y_span), iu = pinned_view(h, uv, uv_span);
    if (i == -1 && iu == -1) return VNECT_OK;  // (f->nv.y stays null: pageable)
    if (i < 0 || iu != i) return refuse(h, who, "the planes run past the pinned buffer they start in");
    f->nv = {pinned_dev(h, i, y), (long long)y_stride, pinned_dev(h, i, uv), (long long)uv_stride, h->stage_dev[i], pinned_end(h, i)};
    return VNECT_OK;
}

int resolve_host_nv12(vnect_handle* h, const char* who, const uint8_t* y, int64_t y_stride, const uint8_t* uv, int64_t uv_stride, int H, int W,
                      const int32_t* rect4, int orient, FrameSrc* out)
{
    if (!y || !uv) return refuse(h, who, "null plane pointer");
    size_t y_span, uv_span;
    FrameSrc f;
    int rc;
    if ((rc = nv12_planes(h, who, H, W, y_stride, uv_stride, &y_span, &uv_span))) return rc;
    if ((rc = nv12_apart(h, who, y, y_span, uv, uv_span))) return rc;
    int Ho, Wo;
    orient_size(orient, H, W, &Ho, &Wo);
    if ((rc = clip_rect(h, who, rect4, Ho, Wo, f.r))) return rc;
    if ((rc = nv12_pinned(h, who, y, y_stride, y_span, uv, uv_stride, uv_span, &f))) return rc;
    f.where = SRC_NV12, f.H = H, f.W = W, f.orient = orient;
    if (!f.nv.y) {
        // pageable planes: the CPU copies what the crop needs into the internal stage -- its Y rows from the even row at or above its
        // first, and the chroma rows under them, as a frame of its own (rows W apart, the UV plane directly behind; 1.5 bytes per
        // pixel); the rect moves up by the rows left out
        // (an oriented frame: the stored rows of the crop's stored rectangle, orient_src_rect; the staged frame is then `rows` high, and the
        // crop, which stays in oriented coordinates, moves by the rows left out as they lie in the oriented picture)
        int sr[4] = {f.r[0], f.r[1], f.r[2], f.r[3]};
        if (orient) orient_src_rect(orient, H, W, f.r[0], f.r[1], f.r[2], f.r[3], sr);
        const int i = 2, y0 = sr[1] & ~1, rows = (sr[1] + sr[3] - y0 + 1) & ~1;   // (y0 + rows <= H: H is even)
        const size_t plane = (size_t)rows * W;
        if ((rc = ensure_stage(h, i, plane + plane / 2))) return rc;
        for (int q = 0; q < rows; q++) memcpy(h->stage[i] + (size_t)q * W, y + (size_t)(y0 + q) * (size_t)y_stride, (size_t)W);
        for (int q = 0; q < rows / 2; q++) memcpy(h->stage[i] + plane + (size_t)q * W, uv + (size_t)(y0 / 2 + q) * (size_t)uv_stride, (size_t)W);
        f.nv = {h->stage_dev[i], (long long)W, h->stage_dev[i] + plane, (long long)W, h->stage_dev[i], pinned_end(h, i)};
        if (!orient) f.r[1] -= y0;
        else {
            // the staged frame is the stored rows y0 .. y0 + rows - 1: the crop's first pixel keeps its stored column and lies y0 rows
            // higher, and the crop starts where that stored pixel lies in the STAGED frame's oriented picture
            int r0, c0;
            orient_map(orient, H, W, f.r[1], f.r[0], &r0, &c0);
            orient_unmap(orient, rows, W, r0 - y0, c0, &f.r[1], &f.r[0]);
            f.H = rows;
        }
    }
    *out = f;
    return VNECT_OK;
}

// the whole (H, W) NV12 frame in pinned buffer `index`: the Y plane at its start, the UV plane uv_offset bytes in
int resolve_pinned_nv12(vnect_handle* h, const char* who, int index, int H, int W, int64_t y_stride, int64_t uv_offset, int64_t uv_stride, int orient, FrameSrc* out)
{
    if (index < 0 || index > 1 || !h->stage[index]) return refuse(h, who, "no such pinned buffer (vnect_frame_buffer)");
    size_t y_span, uv_span;
    FrameSrc f;
    int rc;
    if ((rc = nv12_planes(h, who, H, W, y_stride, uv_stride, &y_span, &uv_span))) return rc;
    const uint8_t *y = h->stage[index], *uv = y + std::max<int64_t>(uv_offset, 0);  // (an offset in front of the buffer's start counts as 0: it overlaps)
    if ((rc = nv12_apart(h, who, y, y_span, uv, uv_span))) return rc;
    if ((rc = nv12_pinned(h, who, y, y_stride, y_span, uv, uv_stride, uv_span, &f))) return rc;
    f.where = SRC_NV12, f.H = H, f.W = W, f.orient = orient;
    orient_size(orient, H, W, &f.r[3], &f.r[2]);
    *out = f;
    return VNECT_OK;
}

// ---- frames in the caller's DEVICE memory (vnect_infer_device and its kin) ---------------------------------------------------------------
// `p` must be device memory of the handle's device as this process's HIP runtime knows it; [*lo, *end) = the allocation it lies in
static int device_range(vnect_handle* h, const void* p, const char* who, const char* what, const uint8_t** lo, const uint8_t** end)
{
    static const char* advice =
        ": device-frame entry points take hipMalloc'ed memory of the handle's device only -- pass host memory to vnect_infer / vnect_upload_frame "
        "(vnect_infer_nv12 / vnect_upload_frame_nv12 for NV12); a pointer of another HIP runtime in this process means nothing to this one "
        "(torch ships its own libamdhip64: import torch BEFORE vnect_amd, so that the process holds one runtime)";
    auto no = [&](const std::string& why) { return refuse(h, who, (why + advice).c_str()); };
    const std::string w = what;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (an unknown pointer is the caller's mistake, not a sticky error of the handle)
        return no(w + " is not memory this process's HIP runtime allocated");
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged) return no(w + " is host or managed memory, not device memory");
    if (at.device != h->cfg.device) return no(w + " lies on another device than the handle's");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base || !size) {
        (void)hipGetLastError();
        return no("hipMemGetAddressRange does not know the allocation " + w + " points into");
    }
    *lo = (const uint8_t*)base, *end = (const uint8_t*)base + size;
    if ((const uint8_t*)p < *lo || (const uint8_t*)p >= *end) return no(w + " lies outside the allocation the runtime reports for it");
    return VNECT_OK;
}

// Validates everything -- the descriptor, the rect, the slot's room, the pointers (device memory of the handle's device, the frame's span
// inside its allocation) -- and changes nothing.  allow_rect false: a tracked frame (no rect, and no slot whose room matters)
int check_device_frame(vnect_handle* h, const vnect_device_frame* f, void* producer_stream, const char* who, bool allow_rect, int orient, FrameSrc* out)
{
    if (!f) return refuse(h, who, "no frame descriptor");
    if (f->struct_size != (int32_t)sizeof(vnect_device_frame)) return refuse(h, who, "vnect_device_frame::struct_size is not sizeof(vnect_device_frame)");
    if (f->format != VNECT_PIX_BGR && f->format != VNECT_PIX_RGB && f->format != VNECT_PIX_NV12)
        return refuse(h, who, "format must be VNECT_PIX_BGR, VNECT_PIX_RGB or VNECT_PIX_NV12");
    const bool nv12 = f->format == VNECT_PIX_NV12;
    const int H = f->H, W = f->W;
    const uint8_t *data = (const uint8_t*)f->data, *uv = (const uint8_t*)f->uv;
    if (!data || (nv12 && !uv)) return refuse(h, who, "null frame pointer");
    if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return refuse(h, who, "bad frame geometry");
    size_t span = 0, uv_span = 0;
    int rc;
    if (nv12) {
        if ((rc = nv12_planes(h, who, H, W, f->stride_y, f->uv_stride, &span, &uv_span))) return rc;
        if (f->stride_y > ((int64_t)1 << 32) || f->uv_stride > ((int64_t)1 << 32)) return refuse(h, who, "stride out of range");
        if ((rc = nv12_apart(h, who, data, span, uv, uv_span))) return rc;
    } else {
        if (f->stride_y < 1 || f->stride_x < 1 || f->stride_c < 1) return refuse(h, who, "strides must be positive (a flipped or rotated frame: pass it as it is stored and say how with vnect_set_orientation; broadcast on the device first)");
        if (f->stride_y > ((int64_t)1 << 32) || f->stride_x > ((int64_t)1 << 32) || f->stride_c > ((int64_t)1 << 36)) return refuse(h, who, "stride out of range");
        span = (size_t)ingest_span(H, W, f->stride_y, f->stride_x, f->stride_c);
    }
    FrameSrc d;
    if (f->has_rect && !allow_rect) return refuse(h, who, "a tracked frame takes no rect: the crop is the stream's box on the device");
    int Ho, Wo;
    orient_size(orient, H, W, &Ho, &Wo);
    if (allow_rect && (rc = clip_rect(h, who, f->has_rect ? f->rect : nullptr, Ho, Wo, d.r))) return rc;
    const uint8_t *lo = nullptr, *end = nullptr, *uv_lo = nullptr, *uv_end = nullptr;
    if ((rc = device_range(h, data, who, "data", &lo, &end))) return rc;
    if ((size_t)(end - data) < span)
        return refuse(h, who, "the frame's last byte lies past the end of the allocation `data` points into (at these strides)");
    if (nv12) {
        if ((rc = device_range(h, uv, who, "uv", &uv_lo, &uv_end))) return rc;
        if ((size_t)(uv_end - uv) < uv_span) return refuse(h, who, "the UV plane's last byte lies past the end of the allocation `uv` points into");
    }
    d.where = nv12 ? SRC_NV12 : SRC_DEVICE, d.H = H, d.W = W, d.orient = orient, d.producer = producer_stream;
    if (!allow_rect) d.r[2] = Wo, d.r[3] = Ho;
    if (nv12) {
        d.nv = {data, (long long)f->stride_y, uv, (long long)f->uv_stride, lo, end};
        d.nv.uv_lo = uv_lo, d.nv.uv_end = uv_end, d.nv.any_bounds = 1;
    } else {
        d.ing = {data, (long long)f->stride_y, (long long)f->stride_x, (long long)f->stride_c, lo, end, f->format == VNECT_PIX_RGB ? INGEST_RGB : INGEST_BGR};
    }
    *out = d;
    return VNECT_OK;
}

// the source block of the oriented copies: pinned BGR is packed-3 in mapped memory, NV12 keeps its one or two allocations
OrientSrc orient_src_of(const FrameSrc& f)
{
    OrientSrc s{};
    s.order = INGEST_BGR;
    if (f.where == SRC_PINNED_BGR) {
        // (a pinned buffer starts on a multiple of 4 in front of the frame: the aligned dword that holds the frame's first byte lies in it)
        s.p0 = f.bgr.data, s.sy = f.bgr.stride, s.sx = 3, s.sc = 1, s.form = INGEST_PACKED3;
        s.lo0 = (const uint8_t*)((uintptr_t)f.bgr.data & ~(uintptr_t)3), s.end0 = f.bgr.end;
    } else if (f.where == SRC_NV12) {
        s.p0 = f.nv.y, s.p1 = f.nv.uv, s.sy = f.nv.y_stride, s.sx = 1, s.sc = f.nv.uv_stride, s.form = ORIENT_NV12;
        s.lo0 = f.nv.lo, s.end0 = f.nv.end, s.lo1 = f.nv.uv_lo ? f.nv.uv_lo : f.nv.lo, s.end1 = f.nv.uv_lo ? f.nv.uv_end : f.nv.end;
    } else {
        s.p0 = f.ing.data, s.sy = f.ing.stride_y, s.sx = f.ing.stride_x, s.sc = f.ing.stride_c, s.order = f.ing.order;
        s.form = ingest_form(s.sx, s.sc), s.lo0 = f.ing.lo, s.end0 = f.ing.end;
    }
    return s;
}

// ---- into the slot ------------------------------------------------------------------------------------------------------------------------
// `slot` is about to be overwritten with a frame of `bytes` BGR bytes
static int claim_slot(vnect_handle* h, int slot, size_t bytes)
{
    if (h->pre_only && bytes > h->pre_frame_cap) {  // the one slot of a pre-processing-only handle grows with its frames
        HIPCK(h, hipStreamSynchronize(h->st));
        int rc = dev_grow(h, &h->frames, &h->pre_frame_cap, bytes);
        if (rc) return rc;
    }
    // a frame still being read by an in-flight inference must not be overwritten: wait for that inference only (frames in
    // other slots keep running, so a pipelined caller uploads frame k+1 while frames k and k-1 compute)
    const long long q = h->slots[slot].last_use;
    if (q >= (long long)h->seq_collect) HIPCK(h, hipEventSynchronize(h->ring[q % RING].done));
    return VNECT_OK;
}

// `consumer` waits for what has been enqueued on the producer's stream so far; the host does not
int wait_for_producer(vnect_handle* h, void* producer_stream, hipStream_t consumer)
{
    if (producer_stream == VNECT_STREAM_SYNCED) return VNECT_OK;
    if (!h->producer_ev) HIPCK(h, hipEventCreateWithFlags(&h->producer_ev, hipEventDisableTiming));
    HIPCK(h, hipEventRecord(h->producer_ev, (hipStream_t)producer_stream));  // (NULL: HIP's default stream)
    HIPCK(h, hipStreamWaitEvent(consumer, h->producer_ev, 0));
    return VNECT_OK;
}

// The frame's crop into `slot`, packed BGR at the slot's origin: one launch on `st` (nullptr: the handle's stream, where a caller runs the
// frame next), behind the slot's last reader and the frame's producer.  Asynchronous: nothing synchronises between the copy and the
// frame's first kernel.
int ingest(vnect_handle* h, int slot, const FrameSrc& f, hipStream_t st)
{
    if (slot < 0 || slot >= (int)h->slots.size()) return fail(h, VNECT_E_ARG, "bad frame slot");
    int rc = claim_slot(h, slot, (size_t)f.r[2] * f.r[3] * 3);
    if (rc) return rc;
    if (!st) st = h->st;
    if ((rc = wait_for_producer(h, f.producer, st))) return rc;
    uint8_t* dst = h->frames + (size_t)slot * h->cfg.max_frame_bytes;
    if (f.orient) {  // a frame stored rotated / mirrored: one oriented copy for every source (orient.hip)
        if (f.where == SRC_SLOT) return fail(h, VNECT_E_INTERNAL, "ingest: a resident slot is no source");
        HIPCK(h, launch_orient_copy(orient_src_of(f), f.orient, f.H, f.W, f.r[0], f.r[1], f.r[2], f.r[3], dst, st));
    } else {
        switch (f.where) {
        case SRC_PINNED_BGR: HIPCK(h, launch_frame_copy(f.bgr.data, dst, f.H, 3 * f.W, f.bgr.stride, f.bgr.end, st)); break;
        case SRC_NV12: HIPCK(h, launch_nv12_copy(f.nv, f.r[0], f.r[1], f.r[2], f.r[3], dst, st)); break;
        case SRC_DEVICE: HIPCK(h, launch_ingest_copy(f.ing, f.H, f.W, f.r[0], f.r[1], f.r[2], f.r[3], dst, st)); break;
        case SRC_SLOT: return fail(h, VNECT_E_INTERNAL, "ingest: a resident slot is no source");
        }
    }
    h->slots[slot].H = f.r[3], h->slots[slot].W = f.r[2], h->slots[slot].stride = 3LL * f.r[2];
    return VNECT_OK;
}

// The same, and done with the caller's buffer (and the internal stage) on return.  On a stream of its own, not on lane 0's: like
// vnect_upload_frame's blocking copy it waits only for the slot's last reader and the producer, so a pipelined caller uploads frame k + 1
// while frame k computes.
int ingest_sync(vnect_handle* h, int slot, const FrameSrc& f)
{
    if (!h->upload_st) HIPCK(h, hipStreamCreateWithFlags(&h->upload_st, hipStreamNonBlocking));
    int rc = ingest(h, slot, f, h->upload_st);
    if (rc) return rc;
    HIPCK(h, hipStreamSynchronize(h->upload_st));
    return VNECT_OK;
}

// vnect_upload_frame, vnect_preprocess and the growing slot of a preprocess_only handle: a pageable, synchronous copy, no pinned staging
int upload_frame_impl(vnect_handle* h, int slot, const uint8_t* bgr, int H, int W, int64_t row_stride)
{
    if (!bgr || slot < 0 || slot >= (int)h->slots.size()) return fail(h, VNECT_E_ARG, "bad frame slot");
    if (H < 1 || W < 1 || row_stride < (int64_t)W * 3) return fail(h, VNECT_E_ARG, "bad frame geometry");
    if ((size_t)H * W * 3 > (size_t)h->cfg.max_frame_bytes) return fail(h, VNECT_E_ARG, "frame larger than max_frame_bytes");
    if (h->orient) {  // stored rotated / mirrored: through the stage and the oriented copy, done on return like the copy below
        FrameSrc f;
        int rc = resolve_host_bgr(h, bgr, H, W, row_stride, h->orient, &f);
        return rc ? rc : ingest_sync(h, slot, f);
    }
    int rc = claim_slot(h, slot, (size_t)H * W * 3);
    if (rc) return rc;
    uint8_t* dst = h->frames + (size_t)slot * h->cfg.max_frame_bytes;
    HIPCK(h, hipMemcpy2D(dst, (size_t)W * 3, bgr, (size_t)row_stride, (size_t)W * 3, H, hipMemcpyHostToDevice));
    h->slots[slot].H = H, h->slots[slot].W = W, h->slots[slot].stride = (long long)W * 3;
    return VNECT_OK;
}

}  // namespace rt
}  // namespace vnect
