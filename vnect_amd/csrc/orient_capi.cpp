// orient_capi.cpp -- C shim over orient.h for tests/test_orient_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.
// Built with plain g++ (`make -C vnect_amd/csrc orient`).  orient_walk goes through an oriented crop the way the kernels of orient.hip do --
// tile by tile, the four waves' rows, 64 lanes at a time, LDS as an array -- with the SAME functions for the tiles, the loads and the
// destination dwords, so the rule is held to numpy without a GPU; the lowest and highest byte loaded, every store outside the crop's
// bytes and every whole-dword store into a dword that two tiles write are reported.  With -DORIENT_SWEEP_MAIN (`make ... orient_sweep_asan`,
// -fsanitize=address,undefined) the same file is a stand-alone program whose sources sit in exactly sized heap blocks: a load outside
// the allocation is the sanitizer's finding.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "orient.h"

using namespace vnect;

namespace {

struct DwordUse {
    int tile = -1;       // the first tile that wrote a byte of the dword
    bool multi = false;  // another tile wrote one too
    bool whole = false;  // somebody stored it whole
};

}  // namespace

extern "C" {

// [0] tile edge, [1] threads, [2] LDS row pitch in dwords, [3] LDS dwords per workgroup
void orient_kernel_spans(int32_t* out) { out[0] = ORIENT_T, out[1] = ORIENT_THREADS, out[2] = ORIENT_PITCH, out[3] = ORIENT_LDS_DWORDS; }

void orient_size_c(int o, int H, int W, int32_t* hw) { int a, b; orient_size(o, H, W, &a, &b); hw[0] = a, hw[1] = b; }
void orient_map_c(int o, int H, int W, int i, int j, int32_t* rc) { int r, c; orient_map(o, H, W, i, j, &r, &c); rc[0] = r, rc[1] = c; }
void orient_src_rect_c(int o, int H, int W, int x, int y, int w, int h, int32_t* s) { int t[4]; orient_src_rect(o, H, W, x, y, w, h, t); for (int k = 0; k < 4; k++) s[k] = t[k]; }

// The oriented crop (x, y, w, h) of the stored (H, W) frame under code o -> dst, rows packed 3 w bytes apart (dst at any alignment).
// The frame's pixel (0, 0) lies off0 bytes into the allocation [base0, base0 + size0); NV12 (form 4): the UV plane off1 bytes into
// [base1, base1 + size1) (base1 null: the same allocation).  hits (3 w h bytes, or null): how often each destination byte was written.
// seen[0..3]: lowest / highest offset from base0 of a byte loaded for the first plane, then the same from base1 for the UV plane
// (-1 where nothing was loaded).  shared_whole: whole-dword stores into a dword that more than one tile writes.  Returns the number
// of stores outside the 3 w h bytes, or -1 for arguments the launcher would refuse.
int64_t orient_walk(const uint8_t* base0, int64_t size0, int64_t off0, const uint8_t* base1, int64_t size1, int64_t off1, int form, int order,
                    int64_t sy, int64_t sx, int64_t sc, int o, int H, int W, int x, int y, int w, int h, uint8_t* dst, uint8_t* hits, int64_t* seen,
                    int64_t* shared_whole)
{
    int Ho, Wo;
    if (!base0 || !dst || o < 1 || o > 7 || H < 1 || W < 1 || sy < 1 || sx < 1 || sc < 1 || off0 < 0 || form < 0 || form > ORIENT_NV12) return -1;
    orient_size(o, H, W, &Ho, &Wo);
    if (x < 0 || y < 0 || w < 1 || h < 1 || (int64_t)x + w > Wo || (int64_t)y + h > Ho) return -1;
    if (!base1) base1 = base0, size1 = size0;
    if (form == ORIENT_NV12) {
        if (((H | W) & 1) || sx != 1 || sy < W || sc < W || off1 < 0) return -1;
        if (off0 + (int64_t)(H - 1) * sy + W > size0 || off1 + (int64_t)(H / 2 - 1) * sc + W > size1) return -1;
    } else {
        if (form != INGEST_GENERIC && form != ingest_form(sx, sc)) return -1;
        if (off0 + ingest_span(H, W, sy, sx, sc) > size0) return -1;
    }
    const OrientSrc s = {base0 + off0, form == ORIENT_NV12 ? base1 + off1 : nullptr, sy, sx, sc, base0, base0 + size0, base1, base1 + size1, form, order};
    uintptr_t sn[4] = {~(uintptr_t)0, 0, ~(uintptr_t)0, 0};
    const long long n = 3LL * w * h;
    const uintptr_t g0 = (uintptr_t)dst & ~(uintptr_t)3;  // the destination's dword grid
    std::vector<DwordUse> use((size_t)(((uintptr_t)dst + n + 3 - g0) >> 2) + 2);
    static thread_local std::vector<uint32_t> lds((size_t)ORIENT_LDS_DWORDS);  // (every tile fills the rows it uses before it loads)
    long long stray = 0;
    const int ty = (h + ORIENT_T - 1) / ORIENT_T, tx = (w + ORIENT_T - 1) / ORIENT_T;
    for (int ti = 0; ti < ty; ti++)
        for (int tj = 0; tj < tx; tj++) {
            OrientTile t;
            if (!orient_tile(o, H, W, x, y, w, h, ti, tj, &t)) continue;
            std::fill(lds.begin(), lds.begin() + (size_t)t.sh * ORIENT_PITCH, 0xdeadbeefu);  // (a byte the loads did not bring must not reach the output unnoticed)
            if (orient_tile_inside(s, form, t)) {  // the common tile, as orient_tile_body loads it
                const int NS = orient_streams(form), NL = 1;
                for (int wave = 0; wave < 4; wave++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int i = 0; i < ORIENT_T / 4 && wave + 4 * (i - 1) < t.sh; i++)  // (past the tile's rows every load is the same dropped one: one is walked)
                            for (int k = 0; k < NS; k++)
                                for (int j = 0; j < NL; j++) {
                                    uintptr_t a;
                                    int at;
                                    orient_inside_dword(s, form, t, k, wave + 4 * i, lane + 64 * j, &a, &at);
                                    const uint32_t v = orient_load_inside(a, at, form, k, sn);
                                    if (at >= 0) lds[(size_t)at] = v;
                                }
            } else {
                for (int wave = 0; wave < 4; wave++)
                    for (int rr = wave; rr < t.sh; rr += 4)
                        for (int lane = 0; lane < 64; lane++) orient_load_row(s, form, t.R0 + rr, t.C0, t.sw, lds.data() + rr * ORIENT_PITCH, lane, sn);
            }
            // -- the barrier --
            for (int wave = 0; wave < 4; wave++)
                for (int ii = wave; ii < t.th; ii += 4)
                    for (int lane = 0; lane < 64; lane++) {
                        uintptr_t a;
                        uint32_t v;
                        const unsigned m = orient_out_dword(s, form, o, H, W, x, y, w, t, ii, lane, lds.data(), (uintptr_t)dst, &a, &v);
                        if (!m) continue;
                        bool inside = true;
                        for (int j = 0; j < 4; j++) {
                            if (!(m & (1u << j))) continue;
                            const uintptr_t b = a + (unsigned)j;
                            if (b < (uintptr_t)dst || b >= (uintptr_t)dst + (uint64_t)n) {
                                stray++, inside = false;
                                continue;
                            }
                            dst[b - (uintptr_t)dst] = (uint8_t)(v >> (8 * j));
                            if (hits && hits[b - (uintptr_t)dst] < 255) hits[b - (uintptr_t)dst]++;
                        }
                        if (!inside) continue;
                        DwordUse& u = use[(size_t)((a - g0) >> 2)];
                        const int id = ti * tx + tj;
                        if (u.tile < 0) u.tile = id;
                        else if (u.tile != id) u.multi = true;
                        if (m == 15u) u.whole = true;
                    }
        }
    if (seen) {
        seen[0] = sn[1] >= sn[0] ? (int64_t)(sn[0] - (uintptr_t)base0) : -1, seen[1] = sn[1] >= sn[0] ? (int64_t)(sn[1] - (uintptr_t)base0) : -1;
        seen[2] = sn[3] >= sn[2] ? (int64_t)(sn[2] - (uintptr_t)base1) : -1, seen[3] = sn[3] >= sn[2] ? (int64_t)(sn[3] - (uintptr_t)base1) : -1;
    }
    if (shared_whole) {
        *shared_whole = 0;
        for (const DwordUse& u : use) *shared_whole += u.multi && u.whole;
    }
    return stray;
}

}  // extern "C"

#ifdef ORIENT_SWEEP_MAIN
namespace {

// the reference of this program: k quarter turns one after the other, then the mirror, on an array of stored pixel numbers
std::vector<int> oriented_index(int o, int H, int W, int* Ho, int* Wo)
{
    std::vector<int> g((size_t)H * W);
    for (int i = 0; i < H * W; i++) g[(size_t)i] = i;
    int h = H, w = W;
    for (int k = 0; k < (o & 3); k++) {  // np.rot90: out[i][j] = in[j][w - 1 - i], out is (w, h)
        std::vector<int> n((size_t)h * w);
        for (int i = 0; i < w; i++)
            for (int j = 0; j < h; j++) n[(size_t)i * h + j] = g[(size_t)j * w + (w - 1 - i)];
        g.swap(n);
        const int t = h;
        h = w, w = t;
    }
    if (o & 4)
        for (int i = 0; i < h; i++)
            for (int j = 0; j < w / 2; j++) {
                const int t = g[(size_t)i * w + j];
                g[(size_t)i * w + j] = g[(size_t)i * w + w - 1 - j], g[(size_t)i * w + w - 1 - j] = t;
            }
    *Ho = h, *Wo = w;
    return g;
}

long long g_walks = 0, g_bad = 0;

// one case: the frame flush with both ends of exactly sized heap blocks (`off` bytes of slack in front), the destination at phase `ph`
// of a block of its own
void one(int form, int order, int o, int H, int W, int x, int y, int w, int h, int off, int ph, int two_blocks)
{
    long long sy, sx, sc, span0, span1 = 0;
    if (form == INGEST_PACKED3) sx = 3, sc = 1, sy = 3LL * W + (off ? 5 : 0);
    else if (form == INGEST_PACKED4) sx = 4, sc = 1, sy = 4LL * W + (off ? 5 : 0);
    else if (form == INGEST_PLANAR) sx = 1, sy = W + (off ? 5 : 0), sc = sy * H + 3;
    else if (form == INGEST_GENERIC) sx = 5, sc = 2, sy = 5LL * W + (off ? 5 : 0);
    else sx = 1, sy = W + (off ? 6 : 0), sc = W + (off ? 2 : 0);
    if (form == ORIENT_NV12) span0 = (long long)(H - 1) * sy + W, span1 = (long long)(H / 2 - 1) * sc + W;
    else span0 = ingest_span(H, W, sy, sx, sc);
    // NV12 in one block: Y, then `off` bytes, then UV
    const long long size0 = off + span0 + (form == ORIENT_NV12 && !two_blocks ? off + span1 : 0);
    uint8_t* b0 = (uint8_t*)malloc((size_t)size0);
    uint8_t* b1 = form == ORIENT_NV12 && two_blocks ? (uint8_t*)malloc((size_t)(off + span1)) : nullptr;
    for (long long i = 0; i < size0; i++) b0[i] = (uint8_t)((i * 2654435761u) >> 13);
    if (b1)
        for (long long i = 0; i < off + span1; i++) b1[i] = (uint8_t)((i * 40503u) >> 5);
    const long long off1 = b1 ? off : off + span0 + off;
    const long long n = 3LL * w * h;
    uint8_t* blk = (uint8_t*)malloc((size_t)(ph + n));
    std::vector<uint8_t> hits((size_t)n, 0);
    int64_t seen[4], shared = 0;
    const int64_t stray = orient_walk(b0, size0, off, b1, b1 ? off + span1 : 0, off1, form, order, sy, sx, sc, o, H, W, x, y, w, h, blk + ph, hits.data(), seen, &shared);
    g_bad += stray != 0, g_bad += shared != 0;
    if (seen[0] < 0 || seen[1] >= size0) g_bad++;
    if (form == ORIENT_NV12 && (seen[2] < 0 || seen[3] >= (b1 ? off + span1 : size0))) g_bad++;
    // (the reference of one (o, H, W) serves every rect of it)
    static std::vector<int> g;
    static int go = -1, gH = -1, gW = -1, Ho = 0, Wo = 0;
    if (o != go || H != gH || W != gW) g = oriented_index(o, H, W, &Ho, &Wo), go = o, gH = H, gW = W;
    const uint8_t* uvp = b1 ? b1 + off1 : b0 + off1;
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            const int idx = g[(size_t)(y + i) * Wo + (x + j)], r = idx / W, c = idx % W;
            int want[3];
            if (form == ORIENT_NV12) {
                nv12_pixel(b0[off + r * sy + c], uvp[(r >> 1) * sc + (c & ~1)], uvp[(r >> 1) * sc + (c & ~1) + 1], want);
            } else {
                for (int k = 0; k < 3; k++) want[k] = b0[off + r * sy + c * sx + (order == INGEST_RGB ? 2 - k : k) * sc];
            }
            for (int k = 0; k < 3; k++) {
                const long long q = ((long long)i * w + j) * 3 + k;
                g_bad += blk[ph + q] != (uint8_t)want[k], g_bad += hits[(size_t)q] != 1;
            }
        }
    free(blk), free(b0), free(b1);
    g_walks++;
}

}  // namespace

int main()
{
    long long ctr = 0;
    // every code x every (H, W) in 1 .. 9 x every rect x every form (NV12: the even sizes); order, source slack and destination phase in turn
    for (int form = 0; form <= ORIENT_NV12; form++)
        for (int o = 1; o < 8; o++)
            for (int H = 1; H <= 9; H++)
                for (int W = 1; W <= 9; W++) {
                    if (form == ORIENT_NV12 && ((H | W) & 1)) continue;
                    int Ho, Wo;
                    orient_size(o, H, W, &Ho, &Wo);
                    for (int y = 0; y < Ho; y++)
                        for (int x = 0; x < Wo; x++)
                            for (int h = 1; y + h <= Ho; h++)
                                for (int w = 1; x + w <= Wo; w++, ctr++) one(form, (int)(ctr & 1), o, H, W, x, y, w, h, (int)((ctr >> 1) & 3), (int)((ctr >> 3) & 3), (int)((ctr >> 5) & 1));
                }
    // the tile seams: T - 1, T, T + 1, 2 T + 1 in each axis (NV12: the even neighbours); whole frames at every destination phase, crops at
    // odd origins, 1-pixel crops at the corners and on a seam
    const int T = ORIENT_T;
    const int sizes[6][2] = {{T - 1, T}, {T, T + 1}, {T + 1, 2 * T + 1}, {2 * T + 1, T - 1}, {3, 2 * T + 1}, {2 * T + 1, 3}};
    for (int form = 0; form <= ORIENT_NV12; form++)
        for (int o = 1; o < 8; o++)
            for (int k = 0; k < 6; k++) {
                int H = sizes[k][0], W = sizes[k][1], Ho, Wo;
                if (form == ORIENT_NV12) H += H & 1, W += W & 1;
                orient_size(o, H, W, &Ho, &Wo);
                for (int ph = 0; ph < 4; ph++, ctr++) one(form, (int)(ctr & 1), o, H, W, 0, 0, Wo, Ho, ph, ph, ph & 1);
                if (Ho > 2 && Wo > 2) one(form, (int)(ctr & 1), o, H, W, 1, 1, Wo - 2, Ho - 2, 1, (int)((ctr >> 1) & 3), 1);
                one(form, 0, o, H, W, 0, 0, 1, 1, 0, 1, 0), one(form, 1, o, H, W, Wo - 1, Ho - 1, 1, 1, 3, 2, 1);
                if (Ho > T && Wo > T) one(form, 0, o, H, W, T - 1, T - 1, 1, 1, 2, 3, 0), one(form, 1, o, H, W, T, T, 1, 1, 1, 0, 1);
                one(form, 0, o, H, W, Wo / 2, 0, 1, Ho, 2, 1, 0), one(form, 1, o, H, W, 0, Ho / 2, Wo, 1, 1, 3, 1);
            }
    printf("orient sweep: %lld walks, %lld mismatches\n", g_walks, g_bad);
    return g_bad ? 1 : 0;
}
#endif
