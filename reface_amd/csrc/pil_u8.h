// PIL's byte arithmetic shared by the units that reproduce it (pasteback.hip: crop -> frame; align.hip: frame -> crop), operation for
// operation from libImaging/Geometry.c and Resample.c.  Every unit that includes this builds with -ffp-contract=off: none of the fp64
// expressions below may be contracted to an FMA.
#pragma once
#include "common.h"

namespace rf {

// Resample.c's clip8 of a 22-bit fixed-point sum (the caller starts the sum at 1 << 21)
__device__ __forceinline__ int pil_clip8(int s) { return min(max(s >> 22, 0), 255); }

// bilinear_filter32RGB after its bounds test: (sx, sy) inside [0, W) x [0, H) of an image of C-byte pixels (the first 3 are read) whose
// rows are `pitch` bytes apart.  u = sx - .5, x0 = floor(u), dx = u - x0 (same for y); v1 = a + (b - a) dx on row clamp(y0) at columns
// clamp(x0), clamp(x0 + 1); v2 likewise on row y0 + 1 when it exists (else v1); v = v1 + (v2 - v1) dy, truncated.
template <int C>
__device__ __forceinline__ void pil_bilinear_rgb(const uint8_t* __restrict__ img, int H, int W, long long pitch, double sx, double sy, uint8_t px[3]) {
    const double u = sx - 0.5, v = sy - 0.5;
    const double fx = floor(u), fy = floor(v);
    const int x0 = (int)fx, y0 = (int)fy;
    const double dx = u - fx, dy = v - fy;
    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x0 + 1, 0), W - 1), cy0 = min(max(y0, 0), H - 1);
    const bool row2 = y0 + 1 >= 0 && y0 + 1 < H;
    const uint8_t* r0 = img + (long long)cy0 * pitch;
    const uint8_t* r1 = row2 ? img + (long long)(y0 + 1) * pitch : r0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double a0 = (double)r0[cx0 * C + ch], b0 = (double)r0[cx1 * C + ch];
        const double v1 = a0 + (b0 - a0) * dx;
        double v2 = v1;
        if (row2) {
            const double a1 = (double)r1[cx0 * C + ch], b1 = (double)r1[cx1 * C + ch];
            v2 = a1 + (b1 - a1) * dx;
        }
        px[ch] = (uint8_t)(int)(v1 + (v2 - v1) * dy);
    }
}

// nq <= 4 consecutive Co-byte pixels (px[q][0 .. Co)) to o: Co 32-bit words when the group is whole and o is word-aligned, else per byte
template <int Co>
__device__ __forceinline__ void store_px4(uint8_t* o, const uint8_t px[4][4], int nq) {
    if (nq == 4 && ((uintptr_t)o & 3) == 0) {
        uint32_t* ow = (uint32_t*)o;
#pragma unroll
        for (int j = 0; j < Co; ++j) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) word |= (uint32_t)px[(4 * j + k) / Co][(4 * j + k) % Co] << (8 * k);
            ow[j] = word;
        }
    } else {
        for (int q = 0; q < nq; ++q)
#pragma unroll
            for (int ch = 0; ch < Co; ++ch) o[q * Co + ch] = px[q][ch];
    }
}

}  // namespace rf
