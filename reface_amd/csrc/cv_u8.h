// cv2.resize(img, (Wo, Ho), interpolation=cv2.INTER_LINEAR) of uint8 HWC images (albumentations' A.Resize), in OpenCV's integer arithmetic and
// operation order (resize.cpp: HResizeLinear<uchar, int, short, 2048> + the u8 VResizeLinear; cv2 itself is absent here: last bit unpinned):
// two taps per axis at half-pixel centres, 11-bit weights rounded to nearest-even, columns clamped with their weight ((s, f) = (0, 0) left
// of the image, (W - 1, 0) from the last column on), rows clipped with the weights kept;
//   out = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2,   Hk = S[yk][sx] * a0 + S[yk][sx + 1] * a1.
// An exact 2:1 reduction on both axes is OpenCV's fast-area case: (a + b + c + d + 2) >> 2.
// Shared by the units that reproduce cv2's bytes: elementwise.hip (rf_resize_u8_linear) and idscore.hip (rf_id_prep_u8).
#pragma once
#include "common.h"

namespace rf {

__device__ __forceinline__ void cv_linear_tap(int d, double scale, int n_src, bool clamp, int& s, int& w0, int& w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (clamp) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    }
    w1 = __float2int_rn(f * 2048.0f);
    w0 = __float2int_rn((1.0f - f) * 2048.0f);
}

// The C bytes of output pixel (dy, dx) of an H x W x C image (rows packed: W * C bytes) resized to Ho x Wo.
__device__ __forceinline__ void cv_resize_linear_px(const uint8_t* __restrict__ img, int H, int W, int C, int Ho, int Wo, int dy, int dx,
                                                    uint8_t* __restrict__ o) {
    if (H == 2 * Ho && W == 2 * Wo) {
        const uint8_t* p0 = img + ((long long)(2 * dy) * W + 2 * dx) * C;
        const uint8_t* p1 = p0 + (long long)W * C;
        for (int c = 0; c < C; ++c) o[c] = (uint8_t)(((int)p0[c] + (int)p0[C + c] + (int)p1[c] + (int)p1[C + c] + 2) >> 2);
        return;
    }
    int sx, a0, a1, sy, b0, b1;
    // (OpenCV's order: inv_scale = dsize / ssize, scale = 1. / inv_scale -- two roundings in double, as reface_amd/data.py:_linear_taps)
    cv_linear_tap(dx, 1.0 / ((double)Wo / (double)W), W, true, sx, a0, a1);
    cv_linear_tap(dy, 1.0 / ((double)Ho / (double)H), H, false, sy, b0, b1);
    const int sx1 = min(sx + 1, W - 1), y0 = min(max(sy, 0), H - 1), y1 = min(max(sy + 1, 0), H - 1);
    const uint8_t* r0 = img + (long long)y0 * W * C;
    const uint8_t* r1 = img + (long long)y1 * W * C;
    for (int c = 0; c < C; ++c) {
        const int h0 = ((int)r0[sx * C + c] * a0 + (int)r0[sx1 * C + c] * a1) >> 4;
        const int h1 = ((int)r1[sx * C + c] * a0 + (int)r1[sx1 * C + c] * a1) >> 4;
        o[c] = (uint8_t)((((b0 * h0) >> 16) + ((b1 * h1) >> 16) + 2) >> 2);
    }
}

}  // namespace rf
