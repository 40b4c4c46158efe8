// The video dataset's per-frame preparation (ldm/data/video_swap_dataset.py:135-240 of the reference; reface_amd/data.py VideoDataset) in one
// launch and one pass over the aligned crop: PIL's Image.resize((w, h)) (BICUBIC by default; any separable tap table works) of the u8 crop,
// ToTensor, Normalize(0.5, 0.5), the keep-mask of the label map and their product -- the model's three input tensors, bit for bit the host's.
// The resized u8 image exists only in LDS.  PIL resizes in two integer passes with a u8 image between them (Resample.c:
// ImagingResampleHorizontal_8bpc, then Vertical_8bpc, each clip8(((1 << 21) + sum k p) >> 22)); the rounding between the passes is part of
// the result, so both passes are kept.  The unit builds with -ffp-contract=off; the float part keeps the host's order of operations.
//
// A block owns VP_TH x VP_TW output pixels.  Per chunk of the input rows its vertical windows cover:
//   1. the rows' column span goes from global memory to LDS as one RGBx word per pixel (12 source bytes = 3 words -> 4 pixels = one 16-byte
//      LDS store; source words are read aligned and funnel-shifted when a row does not start on a word),
//   2. the horizontal pass runs out of LDS into LDS, one RGBx word per (input row, output column),
//   3. every thread adds the chunk's rows into the vertical sums of its 4 output pixels (column tid % 64, rows tid / 64 + 4 q).
// One chunk holds all rows at the dataset's 2:1 (38 rows x 140 pixels); larger ratios take more chunks, and a column span too wide for the
// LDS (a ratio beyond ~90:1) reads its taps from global memory instead.  Lanes of a wave hold consecutive columns of one row: every
// store is a 256-byte row segment of an NCHW plane.
#include "pil_u8.h"

namespace rf {

constexpr int VP_TW = 64, VP_TH = 16, VP_THREADS = 256, VP_Q = VP_TH / (VP_THREADS / VP_TW);
constexpr int VP_RAW_WORDS = 6144;          // 24 KiB of staged source pixels
constexpr int VP_TMP_ROWS = 48;             // 12 KiB of horizontally resampled rows

// 4 bytes at p (any alignment) of the buffer [lo, hi): aligned word loads where the words lie inside the buffer, bytes (0 outside) at its ends
__device__ __forceinline__ uint32_t load4_any(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    const unsigned s = (unsigned)((uintptr_t)p & 3);
    const uint8_t* a = p - s;
    if (s == 0 && p + 4 <= hi) return *(const uint32_t*)p;
    if (a >= lo && a + 8 <= hi) {
        const uint64_t two = ((uint64_t)(*(const uint32_t*)(a + 4)) << 32) | *(const uint32_t*)a;
        return (uint32_t)(two >> (8 * s));
    }
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p + k < hi) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

// bounds[2 i] = first input index, bounds[2 i + 1] = tap count of output index i, clipped to the table's width and to the axis
__device__ __forceinline__ void vp_window(const int* __restrict__ bounds, int i, int ksize, int n_in, int& lo, int& n) {
    lo = max(bounds[2 * i], 0);
    n = max(min(bounds[2 * i + 1], min(ksize, n_in - lo)), 0);
}

__global__ void __launch_bounds__(VP_THREADS)
video_prep_kernel(const uint8_t* __restrict__ crops, int B, int Hc, int Wc, const uint8_t* __restrict__ labels, const uint8_t* __restrict__ lut,
                  const int* __restrict__ xb, const int* __restrict__ xk, int xks, const int* __restrict__ yb, const int* __restrict__ yk, int yks,
                  float* __restrict__ target, float* __restrict__ mask, float* __restrict__ inpaint, int h, int w, int tiles_x, int tiles_y) {
    __shared__ __align__(16) uint32_t raw[VP_RAW_WORDS];
    __shared__ uint32_t tmp[VP_TMP_ROWS * VP_TW];
    __shared__ int span[4];          // min / max input column, min / max input row of the tile's windows
    const int tid = threadIdx.x, tx = tid % VP_TW, ty = tid / VP_TW;
    const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = bx * VP_TW, y0 = by * VP_TH;
    const int x = x0 + tx;
    const bool xok = x < w;
    if (tid == 0) {
        span[0] = span[2] = 0x7fffffff;
        span[1] = span[3] = 0;
    }
    __syncthreads();
    int xlo = 0, xn = 0;
    if (xok) vp_window(xb, x, xks, Wc, xlo, xn);
    if (tid < VP_TW && xn > 0) {
        atomicMin(&span[0], xlo);
        atomicMax(&span[1], xlo + xn);
    }
    if (tid >= VP_TW && tid < VP_TW + VP_TH && y0 + tid - VP_TW < h) {
        int lo, n;
        vp_window(yb, y0 + tid - VP_TW, yks, Hc, lo, n);
        if (n > 0) {
            atomicMin(&span[2], lo);
            atomicMax(&span[3], lo + n);
        }
    }
    __syncthreads();
    const int pbase = span[0] < span[1] ? span[0] & ~3 : 0, pend = span[0] < span[1] ? span[1] : 0;
    const int rbeg = span[2] < span[3] ? span[2] : 0, rend = span[2] < span[3] ? span[3] : 0;
    const int pitch = max(((pend - pbase) + 3) & ~3, 4);          // staged pixels (words) per row
    const bool direct = pitch > VP_RAW_WORDS;                     // the span does not fit: the horizontal taps read global memory
    const int R = direct ? VP_TMP_ROWS : min(VP_RAW_WORDS / pitch, VP_TMP_ROWS);
    const uint8_t* img = crops + (long long)b * Hc * Wc * 3;
    const uint8_t* buf_end = crops + (long long)B * Hc * Wc * 3;
    const int* kx = xk + (long long)x * xks;

    int ylo[VP_Q], yn[VP_Q], acc[VP_Q][3];
#pragma unroll
    for (int q = 0; q < VP_Q; ++q) {
        const int y = y0 + ty + (VP_THREADS / VP_TW) * q;
        ylo[q] = yn[q] = 0;
        if (y < h) vp_window(yb, y, yks, Hc, ylo[q], yn[q]);
        acc[q][0] = acc[q][1] = acc[q][2] = 1 << 21;
    }

    for (int r0 = rbeg; r0 < rend; r0 += R) {
        const int rows = min(R, rend - r0);
        if (!direct) {          // 1. source rows r0 .. r0 + rows, pixels pbase .. pbase + pitch, as RGBx words
            const int groups = pitch / 4;
            for (int it = tid; it < rows * groups; it += VP_THREADS) {
                const int rl = it / groups, g = it - rl * groups;
                const uint8_t* src = img + ((long long)(r0 + rl) * Wc + pbase + 4 * g) * 3;
                const uint32_t w0 = load4_any(src, crops, buf_end), w1 = load4_any(src + 4, crops, buf_end), w2 = load4_any(src + 8, crops, buf_end);
                uint4 px;
                px.x = w0 & 0xffffffu;
                px.y = (w0 >> 24) | ((w1 & 0xffffu) << 8);
                px.z = (w1 >> 16) | ((w2 & 0xffu) << 16);
                px.w = w2 >> 8;
                *(uint4*)&raw[rl * pitch + 4 * g] = px;
            }
            __syncthreads();
        }
        if (xok) {              // 2. PIL's horizontal pass of those rows for the tile's columns (it % VP_TW == tx: a thread keeps its column)
            for (int it = tid; it < rows * VP_TW; it += VP_THREADS) {
                const int rl = it / VP_TW;
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                if (!direct) {
                    const uint32_t* in = &raw[rl * pitch + (xlo - pbase)];
                    for (int i = 0; i < xn; ++i) {
                        const int k = kx[i];
                        const uint32_t p = in[i];
                        a0 += k * (int)(p & 255u);
                        a1 += k * (int)((p >> 8) & 255u);
                        a2 += k * (int)((p >> 16) & 255u);
                    }
                } else {
                    const uint8_t* in = img + ((long long)(r0 + rl) * Wc + xlo) * 3;
                    for (int i = 0; i < xn; ++i) {
                        const int k = kx[i];
                        a0 += k * (int)in[3 * i];
                        a1 += k * (int)in[3 * i + 1];
                        a2 += k * (int)in[3 * i + 2];
                    }
                }
                tmp[rl * VP_TW + tx] = (uint32_t)pil_clip8(a0) | ((uint32_t)pil_clip8(a1) << 8) | ((uint32_t)pil_clip8(a2) << 16);
            }
        }
        __syncthreads();
        if (xok) {              // 3. the chunk's share of the vertical pass
#pragma unroll
            for (int q = 0; q < VP_Q; ++q) {
                const int* ky = yk + (long long)(y0 + ty + (VP_THREADS / VP_TW) * q) * yks;
                const int rb = max(ylo[q], r0), re = min(ylo[q] + yn[q], r0 + rows);
                for (int r = rb; r < re; ++r) {
                    const int k = ky[r - ylo[q]];
                    const uint32_t p = tmp[(r - r0) * VP_TW + tx];
                    acc[q][0] += k * (int)(p & 255u);
                    acc[q][1] += k * (int)((p >> 8) & 255u);
                    acc[q][2] += k * (int)((p >> 16) & 255u);
                }
            }
        }
        if (r0 + R < rend) __syncthreads();          // the next chunk overwrites tmp (raw is free since the barrier above)
    }

    if (!xok) return;
    const long long hw = (long long)h * w;
#pragma unroll
    for (int q = 0; q < VP_Q; ++q) {
        const int y = y0 + ty + (VP_THREADS / VP_TW) * q;
        if (y >= h) continue;
        const long long p = (long long)y * w + x;
        // mask = 1 - ToTensor(255 * isin(label, keep)); image = (u8 / 255 - 0.5) / 0.5; inpaint = image * mask
        const float m = 1.0f - (lut[labels[(long long)b * hw + p]] ? 1.0f : 0.0f);
        mask[(long long)b * hw + p] = m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = ((float)pil_clip8(acc[q][c]) / 255.0f - 0.5f) / 0.5f;
            target[((long long)b * 3 + c) * hw + p] = v;
            inpaint[((long long)b * 3 + c) * hw + p] = v * m;
        }
    }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_video_prep_u8(const void* crops_u8, int B, int Hc, int Wc, int C, const void* labels_u8, const void* lut256_u8, const int* xbounds,
                                const int* xk, int xksize, const int* ybounds, const int* yk, int yksize, float* target, float* mask, float* inpaint,
                                int h, int w, void* stream) {
    RF_CHECK(crops_u8 && labels_u8 && lut256_u8 && xbounds && xk && ybounds && yk && target && mask && inpaint, "rf_video_prep_u8: null argument");
    RF_CHECK(B > 0 && Hc > 0 && Wc > 0 && h > 0 && w > 0 && xksize > 0 && yksize > 0, "rf_video_prep_u8: bad sizes (B=%d %dx%d -> %dx%d, ksize %d / %d)",
             B, Wc, Hc, w, h, xksize, yksize);
    RF_CHECK(C == 3, "rf_video_prep_u8: crop channels must be 3 (C=%d)", C);
    RF_CHECK(target != mask && target != inpaint && mask != inpaint, "rf_video_prep_u8: target, mask and inpaint must be three buffers");
    RF_CHECK((const void*)target != crops_u8 && (const void*)mask != crops_u8 && (const void*)inpaint != crops_u8 && (const void*)target != labels_u8 &&
             (const void*)mask != labels_u8 && (const void*)inpaint != labels_u8, "rf_video_prep_u8: an output cannot overwrite the crops or the labels");
    const int tiles_x = (w + VP_TW - 1) / VP_TW, tiles_y = (h + VP_TH - 1) / VP_TH;
    const long long blocks = (long long)B * tiles_x * tiles_y;
    RF_CHECK(blocks < (1LL << 31), "rf_video_prep_u8: too many tiles (%lld)", blocks);
    hipLaunchKernelGGL(video_prep_kernel, dim3((unsigned)blocks), dim3(VP_THREADS), 0, (hipStream_t)stream, (const uint8_t*)crops_u8, B, Hc, Wc,
                       (const uint8_t*)labels_u8, (const uint8_t*)lut256_u8, xbounds, xk, xksize, ybounds, yk, yksize, target, mask, inpaint, h, w,
                       tiles_x, tiles_y);
    RF_LAUNCH_CHECK("rf_video_prep_u8");
    return 0;
}
