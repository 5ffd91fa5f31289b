// nv12_capi.cpp -- C shim over nv12.h for tests/test_nv12_cpu.py.  TEST INFRASTRUCTURE: it is NOT part of libvnect_hip.so.
// Built with plain g++ (`make -C vnect_amd/csrc nv12`): the one source the kernels of post.hip convert with, on the host, so the
// arithmetic is held to the tests' numpy restatement over all 2^24 (Y, U, V) triples without a GPU.  With -DNV12_SWEEP_MAIN
// (`make ... nv12_sweep_asan`, -fsanitize=address,undefined) the same file is a stand-alone program that runs the all-triples sweep
// and strided images against a second, table-free statement of the formula.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nv12.h"

using namespace vnect;

// A whole image on the host: rect (x, y, w, h) of an NV12 frame -> packed BGR rows, dst_stride bytes
// apart, through nv12_quad, one group of four frame columns at a time.  The caller guarantees the rect lies inside the frame.
static void nv12_image(const uint8_t* yp, long long ys, const uint8_t* uvp, long long uvs, int x, int y, int w, int h, uint8_t* dst,
                       long long dst_stride)
{
    for (int r = y; r < y + h; r++) {
        const uint8_t* yr = yp + (long long)r * ys;
        const uint8_t* ur = uvp + (long long)(r >> 1) * uvs;
        for (int g = x >> 2; g <= (x + w - 1) >> 2; g++) {
            uint32_t y4 = 0, uv4 = 0, o[3];
            for (int j = 0; j < 4; j++) {  // (bytes of the group past the crop's last column may lie outside the image: not read)
                const int c = 4 * g + j;
                if (c < x + w) y4 |= (uint32_t)yr[c] << (8 * j), uv4 |= (uint32_t)ur[(c & ~1) + 0] << (16 * (j >> 1)) | (uint32_t)ur[(c & ~1) + 1] << (16 * (j >> 1) + 8);
            }
            nv12_quad(y4, uv4, o);
            for (int j = 0; j < 4; j++) {
                const int c = 4 * g + j;
                if (c < x || c >= x + w) continue;
                for (int k = 0; k < 3; k++) dst[(long long)(r - y) * dst_stride + 3LL * (c - x) + k] = (uint8_t)(o[(3 * j + k) >> 2] >> (8 * ((3 * j + k) & 3)));
            }
        }
    }
}

extern "C" {

// [0] pixels per lane, [1] per wave, [2] per workgroup of the kernels (nv12.h)
void nv12_kernel_spans(int32_t* out) { out[0] = NV12_LANE_PX, out[1] = NV12_WAVE_PX, out[2] = NV12_WG_PX; }

// n (Y, U, V) triples -> n (B, G, R) triples through nv12_pixel
void nv12_pixels(const uint8_t* yuv, int64_t n, uint8_t* bgr)
{
    for (int64_t i = 0; i < n; i++) {
        int c[3];
        nv12_pixel(yuv[3 * i], yuv[3 * i + 1], yuv[3 * i + 2], c);
        bgr[3 * i] = (uint8_t)c[0], bgr[3 * i + 1] = (uint8_t)c[1], bgr[3 * i + 2] = (uint8_t)c[2];
    }
}

// Every triple with luma Y0 through nv12_pixel: out[(U * 256 + V) * 3 + k]
void nv12_plane_pixel(int Y0, uint8_t* out)
{
    for (int U = 0; U < 256; U++)
        for (int V = 0; V < 256; V++) {
            int c[3];
            nv12_pixel(Y0, U, V, c);
            for (int k = 0; k < 3; k++) out[((size_t)U * 256 + V) * 3 + k] = (uint8_t)c[k];
        }
}

// The same through nv12_quad, every triple in each of the helper's four pixel positions: the quad's four lumas are Y0 in position p and
// three different ones elsewhere, its two chroma pairs (U, V) on p's side and another pair on the other.  out[p][(U * 256 + V) * 3 + k];
// returns the number of bytes at the OTHER three positions that differ from nv12_pixel of what was put there (0 when the helper is right).
int64_t nv12_plane_quad(int Y0, uint8_t* out)
{
    int64_t bad = 0;
    for (int p = 0; p < 4; p++)
        for (int U = 0; U < 256; U++)
            for (int V = 0; V < 256; V++) {
                int Y[4], Uc[2], Vc[2];
                for (int j = 0; j < 4; j++) Y[j] = (Y0 * 7 + 31 * j + U + 3 * V + 11) & 255;
                Y[p] = Y0;
                Uc[p >> 1] = U, Vc[p >> 1] = V, Uc[1 - (p >> 1)] = (V + 77) & 255, Vc[1 - (p >> 1)] = (U + 191) & 255;
                const uint32_t y4 = (uint32_t)Y[0] | (uint32_t)Y[1] << 8 | (uint32_t)Y[2] << 16 | (uint32_t)Y[3] << 24;
                const uint32_t uv4 = (uint32_t)Uc[0] | (uint32_t)Vc[0] << 8 | (uint32_t)Uc[1] << 16 | (uint32_t)Vc[1] << 24;
                uint32_t o[3];
                nv12_quad(y4, uv4, o);
                uint8_t b[12];
                memcpy(b, o, 12);
                for (int j = 0; j < 4; j++) {
                    int c[3];
                    nv12_pixel(Y[j], Uc[j >> 1], Vc[j >> 1], c);
                    for (int k = 0; k < 3; k++) {
                        if (j == p) out[(((size_t)p * 256 + U) * 256 + V) * 3 + k] = b[3 * j + k];
                        else bad += b[3 * j + k] != (uint8_t)c[k];
                    }
                }
            }
    return bad;
}

// rect (x, y, w, h) of an (H, W) NV12 frame -> packed BGR (h, w, 3) through nv12_image.  Returns 0, or -1 for a rect outside the frame.
int nv12_convert(const uint8_t* yp, int64_t ys, const uint8_t* uvp, int64_t uvs, int H, int W, int x, int y, int w, int h, uint8_t* dst)
{
    if (H < 2 || W < 2 || (H & 1) || (W & 1) || ys < W || uvs < W || x < 0 || y < 0 || w < 1 || h < 1 || (int64_t)x + w > W || (int64_t)y + h > H) return -1;
    nv12_image(yp, ys, uvp, uvs, x, y, w, h, dst, 3LL * w);
    return 0;
}

}  // extern "C"

#ifdef NV12_SWEEP_MAIN
// The formula once more, written out with 64-bit integers and a floor division instead of shifts: what the sweep compares against.
static int ref_channel(long long v)
{
    long long q = v / 1048576;
    if (v % 1048576 < 0) q--;
    return q < 0 ? 0 : (q > 255 ? 255 : (int)q);
}
int main()
{
    long long bad = 0;
    std::vector<uint8_t> a(256 * 256 * 3), q(4 * 256 * 256 * 3);
    for (int Y = 0; Y < 256; Y++) {
        nv12_plane_pixel(Y, a.data());
        bad += nv12_plane_quad(Y, q.data());
        const long long y = (long long)(Y > 16 ? Y - 16 : 0) * 1220542 + 524288;
        for (int U = 0; U < 256; U++)
            for (int V = 0; V < 256; V++) {
                const long long u = U - 128, v = V - 128;
                const int want[3] = {ref_channel(y + 2116026 * u), ref_channel(y - 852492 * v - 409993 * u), ref_channel(y + 1673527 * v)};
                for (int k = 0; k < 3; k++) {
                    const size_t i = ((size_t)U * 256 + V) * 3 + k;
                    bad += a[i] != want[k];
                    for (int p = 0; p < 4; p++) bad += q[(size_t)p * 256 * 256 * 3 + i] != want[k];
                }
            }
    }
    // strided images in exactly sized heap blocks (the sanitizer sees any byte read or written outside them): odd strides, planes apart,
    // every crop origin and size residue
    long long crops = 0;
    const int H = 6, W = 12;
    for (int ys = W; ys <= W + 5; ys += 5)
        for (int uvs = W; uvs <= W + 3; uvs += 3) {
            std::vector<uint8_t> yp((size_t)(H - 1) * ys + W), up((size_t)(H / 2 - 1) * uvs + W);
            for (size_t i = 0; i < yp.size(); i++) yp[i] = (uint8_t)(i * 2654435761u >> 23);
            for (size_t i = 0; i < up.size(); i++) up[i] = (uint8_t)(i * 40503u >> 5);
            for (int x = 0; x < 5; x++)
                for (int y0 = 0; y0 < 3; y0++)
                    for (int w = 1; x + w <= W; w++)
                        for (int h = 1; y0 + h <= H; h++) {
                            std::vector<uint8_t> d((size_t)3 * w * h);
                            if (nv12_convert(yp.data(), ys, up.data(), uvs, H, W, x, y0, w, h, d.data())) bad++;
                            for (int r = 0; r < h; r++)
                                for (int c = 0; c < w; c++) {
                                    int px[3];
                                    const uint8_t* uv = &up[(size_t)((y0 + r) >> 1) * uvs + ((x + c) & ~1)];
                                    nv12_pixel(yp[(size_t)(y0 + r) * ys + x + c], uv[0], uv[1], px);
                                    for (int k = 0; k < 3; k++) bad += d[((size_t)r * w + c) * 3 + k] != px[k];
                                }
                            crops++;
                        }
        }
    printf("nv12 sweep: 16777216 triples x (pixel + 4 quad positions), %lld crops, %lld mismatches\n", crops, bad);
    return bad ? 1 : 0;
}
#endif
