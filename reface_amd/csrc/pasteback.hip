// Stage 3 of the video caller (scripts/inference_swap_video.py:705-724 of the reference): every swapped crop is enlarged to S x S with PIL's
// BILINEAR resize and warped back into its full frame with PIL's PERSPECTIVE transform (BILINEAR), then alpha-composited over the frame.
// Both are byte-level and memory-bound; each thread handles 4 consecutive output pixels so that a group's bytes leave in 32-bit words.
// The arithmetic is PIL's own (libImaging/Resample.c, Geometry.c), operation for operation; the unit builds with -ffp-contract=off, so none
// of the fp64 coordinate / lerp expressions below is contracted to an FMA (the only v_fma_f64 in the ISA are inside the two IEEE divisions).
#include "pil_u8.h"

namespace rf {

// ---- PIL resize, BILINEAR, upscale only (filterscale = 1, support = 1): taps of output index i along an axis of n_in -> n_out.
// center = (i + 0.5) * scale; xmin = max(int(center - 1 + 0.5), 0); xmax = min(int(center + 1 + 0.5), n_in); triangle weights at
// (x + xmin) - center + 0.5, normalised by their sum, then int(0.5 + w * 2^22).  For center >= 0.5 the window is floor(center + 1.5) -
// floor(center - 0.5) = 2 samples wide; below it is 1: never more than 2 taps.
__device__ __forceinline__ void pil_taps(int i, int n_in, int n_out, int& lo, int& n, int k[2]) {
    const double scale = (double)n_in / (double)n_out;
    const double center = ((double)i + 0.5) * scale;
    int xmin = (int)(center - 1.0 + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + 1.0 + 0.5);
    if (xmax > n_in) xmax = n_in;
    n = min(xmax - xmin, 2);
    lo = xmin;
    double w[2] = {0.0, 0.0}, ww = 0.0;
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        if (x < n) {
            double t = (double)(x + xmin) - center + 0.5;
            if (t < 0.0) t = -t;
            w[x] = t < 1.0 ? 1.0 - t : 0.0;
            ww += w[x];
        }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) k[x] = x < n ? (int)(0.5 + (ww != 0.0 ? w[x] / ww : w[x]) * (double)(1 << 22)) : 0;
}

// (255.f * x).astype(uint8) of the reference: fp32 product, truncation toward zero, low byte
__device__ __forceinline__ int u8_of(float v) { return (int)(255.0f * v) & 0xff; }

// One output pixel (b, Y, X) of the resize of fp32 NCHW [B, 3, h, w] to S x S: the horizontal pass (clipped to u8) of the <= 2 input rows
// the vertical taps read, then the vertical pass -- PIL's two passes, recomputed per pixel instead of staged through memory.
__device__ __forceinline__ void paste_crop_pixel(const float* __restrict__ x, int h, int w, int S, long long p, int out[3]) {
    const long long SS = (long long)S * S;
    const int b = (int)(p / SS);
    const int r = (int)(p - (long long)b * SS), Y = r / S, X = r - (r / S) * S;
    int xl, xn, kx[2], yl, yn, ky[2];
    pil_taps(X, w, S, xl, xn, kx);
    pil_taps(Y, h, S, yl, yn, ky);
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j >= yn) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* row = x + (((long long)b * 3 + c) * h + (yl + j)) * w + xl;
            int s = 1 << 21;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (i < xn) s += kx[i] * u8_of(row[i]);
            acc[c] += ky[j] * pil_clip8(s);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = pil_clip8(acc[c]);
}

// fp32 NCHW [B, 3, h, w] -> u8 HWC [B, S, S, 3]; thread t writes pixels 4t .. 4t + 3 of the flat B * S * S range (12 bytes = 3 words)
__global__ void paste_crop_kernel(const float* __restrict__ x, int B, int h, int w, int S, uint8_t* __restrict__ out) {
    const long long n = (long long)B * S * S;
    const long long p0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= n) return;
    int v[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (p0 + q < n) paste_crop_pixel(x, h, w, S, p0 + q, v[q]);
        else v[q][0] = v[q][1] = v[q][2] = 0;
    }
    uint8_t* o = out + p0 * 3;
    if (p0 + 4 <= n && ((uintptr_t)o & 3) == 0) {
        uint32_t* ow = (uint32_t*)o;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) word |= (uint32_t)v[(4 * j + k) / 3][(4 * j + k) % 3] << (8 * k);
            ow[j] = word;
        }
    } else {
        for (int q = 0; q < 4 && p0 + q < n; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[q * 3 + c] = (uint8_t)v[q][c];
    }
}

// ---- PIL Image.transform(size, PERSPECTIVE, c, BILINEAR) of the alpha-255 crop + alpha_composite onto the frame.  Per output pixel, in fp64:
// (xi, yi) = (x + .5, y + .5); d = c6 xi + c7 yi + 1; sx = (c0 xi + c1 yi + c2) / d; sy = (c3 xi + c4 yi + c5) / d.  Outside [0, S)^2 (or not
// finite) the frame pixel stays; inside, u = sx - .5, x0 = floor(u), dx = u - x0 (same for y), v1 = a + (b - a) dx on row clamp(y0) at columns
// clamp(x0), clamp(x0 + 1), v2 likewise on row y0 + 1 when it exists (else v1), v = v1 + (v2 - v1) dy truncated -- PIL's bilinear_filter32RGB.
// With alpha 255 everywhere, PIL's premultiplied detour and the composite reduce to "crop inside, frame outside"; alpha is 255 inside and
// the frame's own alpha (255 for RGB frames) outside.
template <int Cf, int Co>
__global__ void paste_back_kernel(const uint8_t* __restrict__ crops, int S, const double* __restrict__ coeffs, const uint8_t* frames, int H, int W,
                                  long long fstride, uint8_t* out, int B) {
    const long long HW = (long long)H * W, G = (HW + 3) / 4;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * G) return;
    const int b = (int)(t / G);
    const long long p0 = (t - (long long)b * G) * 4;
    const int nq = (int)min(4LL, HW - p0);
    const double* c = coeffs + (long long)b * 8;
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6], c7 = c[7];
    const uint8_t* crop = crops + (long long)b * S * S * 3;
    const uint8_t* fr = frames + (long long)b * fstride + p0 * Cf;
    uint8_t* o = out + ((long long)b * HW + p0) * Co;
    uint8_t px[4][4];
    bool inside[4];
    bool any_out = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        inside[q] = false;
        px[q][0] = px[q][1] = px[q][2] = 0;
        px[q][3] = 255;
        if (q >= nq) continue;
        const long long p = p0 + q;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const double xi = (double)x + 0.5, yi = (double)y + 0.5;
        const double d = c6 * xi + c7 * yi + 1.0;
        const double sx = (c0 * xi + c1 * yi + c2) / d;
        const double sy = (c3 * xi + c4 * yi + c5) / d;
        inside[q] = sx >= 0.0 && sx < (double)S && sy >= 0.0 && sy < (double)S;          // false for NaN
        if (!inside[q]) {
            any_out = true;
            continue;
        }
        pil_bilinear_rgb<3>(crop, S, S, (long long)S * 3, sx, sy, px[q]);
    }
    if (any_out) {                // the frame's bytes of this group: Cf words when aligned and whole, else per byte
        uint8_t fb[4 * Cf];
        if (nq == 4 && ((uintptr_t)fr & 3) == 0) {
            const uint32_t* fw = (const uint32_t*)fr;
#pragma unroll
            for (int j = 0; j < Cf; ++j) {
                const uint32_t word = fw[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) fb[4 * j + k] = (uint8_t)(word >> (8 * k));
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int ch = 0; ch < Cf; ++ch) fb[q * Cf + ch] = q < nq ? fr[q * Cf + ch] : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (!inside[q])
#pragma unroll
                for (int ch = 0; ch < Cf; ++ch) px[q][ch] = fb[q * Cf + ch];
    }
    store_px4<Co>(o, px, nq);
}

}  // namespace rf

using namespace rf;

extern "C" int rf_paste_crop_u8(const float* x, int B, int h, int w, int S, void* out_u8, void* stream) {
    RF_CHECK(x && out_u8 && B > 0 && h > 0 && w > 0 && S > 0, "rf_paste_crop_u8: bad arguments (B=%d h=%d w=%d S=%d)", B, h, w, S);
    RF_CHECK(S >= h && S >= w, "rf_paste_crop_u8: only upscaling is supported (%dx%d -> %d)", w, h, S);
    const long long groups = ((long long)B * S * S + 3) / 4;
    hipLaunchKernelGGL(paste_crop_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, B, h, w, S, (uint8_t*)out_u8);
    RF_LAUNCH_CHECK("rf_paste_crop_u8");
    return 0;
}

extern "C" int rf_paste_back_u8(const void* crops_u8, int B, int S, const double* coeffs, const void* frames_u8, int H, int W, int Cf,
                                int64_t frame_stride, void* out_u8, int Co, void* stream) {
    RF_CHECK(crops_u8 && coeffs && frames_u8 && out_u8 && B > 0 && S > 0 && H > 0 && W > 0,
             "rf_paste_back_u8: bad arguments (B=%d S=%d H=%d W=%d)", B, S, H, W);
    RF_CHECK((Cf == 3 || Cf == 4) && (Co == 3 || Co == 4), "rf_paste_back_u8: frame / output channels must be 3 or 4 (Cf=%d Co=%d)", Cf, Co);
    RF_CHECK(frame_stride >= (int64_t)H * W * Cf, "rf_paste_back_u8: frame stride %lld < H * W * Cf", (long long)frame_stride);
    RF_CHECK(out_u8 != frames_u8 || (Cf == Co && frame_stride == (int64_t)H * W * Cf),
             "rf_paste_back_u8: in place (out == frames) needs Cf == Co and packed frames");
    const long long n = (long long)B * (((long long)H * W + 3) / 4);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const uint8_t* cr = (const uint8_t*)crops_u8;
    const uint8_t* fr = (const uint8_t*)frames_u8;
    uint8_t* o = (uint8_t*)out_u8;
    const long long fs = (long long)frame_stride;
    hipStream_t st = (hipStream_t)stream;
    if (Cf == 3 && Co == 3) hipLaunchKernelGGL((paste_back_kernel<3, 3>), grid, block, 0, st, cr, S, coeffs, fr, H, W, fs, o, B);
    else if (Cf == 3 && Co == 4) hipLaunchKernelGGL((paste_back_kernel<3, 4>), grid, block, 0, st, cr, S, coeffs, fr, H, W, fs, o, B);
    else if (Cf == 4 && Co == 3) hipLaunchKernelGGL((paste_back_kernel<4, 3>), grid, block, 0, st, cr, S, coeffs, fr, H, W, fs, o, B);
    else hipLaunchKernelGGL((paste_back_kernel<4, 4>), grid, block, 0, st, cr, S, coeffs, fr, H, W, fs, o, B);
    RF_LAUNCH_CHECK("rf_paste_back_u8");
    return 0;
}
