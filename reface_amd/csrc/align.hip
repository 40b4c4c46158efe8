// Stage 1's pixel work (src/utils/alignmengt.py:crop_image of the reference): the oriented quad of a face, resampled from its full frame to an
// S x S crop with PIL's Image.transform(QUAD, BILINEAR), after PIL's LANCZOS shrink of the frame when the face is much larger than the crop.
// Paste-back's mirror image (pasteback.hip warps crop -> frame); the sampler and the 22-bit clip are shared through pil_u8.h.  The
// arithmetic is PIL's own (libImaging/Geometry.c: quad_transform, bilinear_filter32RGB; Resample.c: ImagingResampleHorizontal_8bpc /
// Vertical_8bpc), operation for operation; the unit builds with -ffp-contract=off, and there is no division here: the ISA holds no v_fma_f64.
#include "pil_u8.h"

namespace rf {

// ---- Image.transform((S, S), QUAD, quad, BILINEAR).  Per output pixel (x, y), in fp64 and in quad_transform's order:
// xin = x + .5, yin = y + .5; xs = a0 + a1 xin + a2 yin + a3 xin yin; ys = a4 + a5 xin + a6 yin + a7 xin yin.  Outside [0, w) x [0, h) of
// the source window (tested BEFORE the -.5 shift; false for NaN) the pixel is 0; inside, pil_bilinear_rgb.  The source window of frame b
// is win[b] = (ox, oy, w, h) in frame pixels (the reference's img.crop before the transform: the coefficients are in the window's
// coordinates), or the whole frame without `win`; a window that does not lie inside the frame gives an all-zero crop.
// Thread t of a frame writes pixels 4t .. 4t + 3 of its S * S range (12 bytes = 3 words).
template <int Cf>
__global__ void align_quad_kernel(const uint8_t* __restrict__ frames, int H, int W, long long fstride, const double* __restrict__ coeffs,
                                  const int* __restrict__ win, int S, uint8_t* __restrict__ out, int B) {
    const long long SS = (long long)S * S, G = (SS + 3) / 4;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * G) return;
    const int b = (int)(t / G);
    const long long p0 = (t - (long long)b * G) * 4;
    const int nq = (int)min(4LL, SS - p0);
    const double* a = coeffs + (long long)b * 8;
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
    int ox = 0, oy = 0, w = W, h = H;
    if (win) {
        ox = win[b * 4], oy = win[b * 4 + 1], w = win[b * 4 + 2], h = win[b * 4 + 3];
    }
    const bool ok = ox >= 0 && oy >= 0 && w > 0 && h > 0 && w <= W - ox && h <= H - oy;
    const long long pitch = (long long)W * Cf;
    const uint8_t* img = frames + (long long)b * fstride + (long long)oy * pitch + (long long)ox * Cf;
    uint8_t px[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        px[q][0] = px[q][1] = px[q][2] = px[q][3] = 0;
        if (q >= nq || !ok) continue;
        const long long p = p0 + q;
        const int y = (int)(p / S), x = (int)(p - (long long)y * S);
        const double xin = (double)x + 0.5, yin = (double)y + 0.5;
        const double xs = a0 + a1 * xin + a2 * yin + a3 * xin * yin;
        const double ys = a4 + a5 * xin + a6 * yin + a7 * xin * yin;
        if (xs >= 0.0 && xs < (double)w && ys >= 0.0 && ys < (double)h) pil_bilinear_rgb<Cf>(img, h, w, pitch, xs, ys, px[q]);
    }
    store_px4<3>(out + ((long long)b * SS + p0) * 3, px, nq);
}

// ---- Image.resize(size, LANCZOS) on 8-bit channels: two separable integer passes with the host's tap tables (PIL's precompute_coeffs /
// normalize_coeffs_8bpc: for output index i, `bounds[2 i]` = first input index, `bounds[2 i + 1]` = tap count <= ksize, taps at
// kk[i * ksize ...]); each pass is clip8(((1 << 21) + sum k p) >> 22), with u8 between the passes.  One thread per output pixel (C bytes).
template <int C>
__global__ void resample_h_kernel(const uint8_t* __restrict__ x, long long rows, int W, int w, const int* __restrict__ bounds,
                                  const int* __restrict__ kk, int ksize, uint8_t* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * w) return;
    const long long r = t / w;
    const int xo = (int)(t - r * w);
    const int lo = max(bounds[2 * xo], 0), n = min(bounds[2 * xo + 1], min(ksize, W - lo));          // (a table cannot make the loop leave the row)
    const int* k = kk + (long long)xo * ksize;
    const uint8_t* in = x + (r * W + lo) * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
    for (int i = 0; i < n; ++i) {
        const int ki = k[i];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += ki * (int)in[i * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[t * C + c] = (uint8_t)pil_clip8(acc[c]);
}

template <int C>
__global__ void resample_v_kernel(const uint8_t* __restrict__ x, int B, int H, int w, int h, const int* __restrict__ bounds,
                                  const int* __restrict__ kk, int ksize, uint8_t* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * h * w) return;
    const long long r = t / w;                     // b * h + yo
    const int xo = (int)(t - r * w), b = (int)(r / h), yo = (int)(r - (long long)b * h);
    const int lo = max(bounds[2 * yo], 0), n = min(bounds[2 * yo + 1], min(ksize, H - lo));          // (nor the column)
    const int* k = kk + (long long)yo * ksize;
    const uint8_t* in = x + (((long long)b * H + lo) * w + xo) * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
    for (int i = 0; i < n; ++i) {
        const int ki = k[i];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += ki * (int)in[(long long)i * w * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[t * C + c] = (uint8_t)pil_clip8(acc[c]);
}

}  // namespace rf

using namespace rf;

extern "C" int rf_align_quad_u8(const void* frames_u8, int B, int H, int W, int Cf, int64_t frame_stride, const double* coeffs, const int* windows,
                                int S, void* out_u8, void* stream) {
    RF_CHECK(frames_u8 && coeffs && out_u8 && B > 0 && H > 0 && W > 0 && S > 0, "rf_align_quad_u8: bad arguments (B=%d H=%d W=%d S=%d)", B, H, W, S);
    RF_CHECK(Cf == 3 || Cf == 4, "rf_align_quad_u8: frame channels must be 3 or 4 (Cf=%d)", Cf);
    RF_CHECK(frame_stride >= (int64_t)H * W * Cf, "rf_align_quad_u8: frame stride %lld < H * W * Cf", (long long)frame_stride);
    RF_CHECK(out_u8 != frames_u8, "rf_align_quad_u8: the crops cannot overwrite the frames");
    const long long n = (long long)B * (((long long)S * S + 3) / 4);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const uint8_t* fr = (const uint8_t*)frames_u8;
    hipStream_t st = (hipStream_t)stream;
    if (Cf == 3) hipLaunchKernelGGL((align_quad_kernel<3>), grid, block, 0, st, fr, H, W, (long long)frame_stride, coeffs, windows, S, (uint8_t*)out_u8, B);
    else hipLaunchKernelGGL((align_quad_kernel<4>), grid, block, 0, st, fr, H, W, (long long)frame_stride, coeffs, windows, S, (uint8_t*)out_u8, B);
    RF_LAUNCH_CHECK("rf_align_quad_u8");
    return 0;
}

extern "C" int rf_resample_u8(const void* x_u8, int B, int H, int W, int C, const int* xbounds, const int* xk, int xksize, const int* ybounds,
                              const int* yk, int yksize, void* tmp_u8, void* out_u8, int h, int w, void* stream) {
    RF_CHECK(x_u8 && xbounds && xk && ybounds && yk && tmp_u8 && out_u8, "rf_resample_u8: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && xksize > 0 && yksize > 0, "rf_resample_u8: bad sizes (B=%d %dx%d -> %dx%d, ksize %d / %d)",
             B, W, H, w, h, xksize, yksize);
    RF_CHECK(C == 3 || C == 4, "rf_resample_u8: channels must be 3 or 4 (C=%d)", C);
    RF_CHECK(tmp_u8 != x_u8 && tmp_u8 != out_u8 && out_u8 != x_u8, "rf_resample_u8: x, tmp and out must be three buffers");
    const uint8_t* x = (const uint8_t*)x_u8;
    uint8_t* tmp = (uint8_t*)tmp_u8;
    uint8_t* o = (uint8_t*)out_u8;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * H, n1 = rows * w, n2 = (long long)B * h * w;
    const dim3 g1((unsigned)((n1 + 255) / 256)), g2((unsigned)((n2 + 255) / 256)), block(256);
    if (C == 3) {
        hipLaunchKernelGGL((resample_h_kernel<3>), g1, block, 0, st, x, rows, W, w, xbounds, xk, xksize, tmp);
        hipLaunchKernelGGL((resample_v_kernel<3>), g2, block, 0, st, (const uint8_t*)tmp, B, H, w, h, ybounds, yk, yksize, o);
    } else {
        hipLaunchKernelGGL((resample_h_kernel<4>), g1, block, 0, st, x, rows, W, w, xbounds, xk, xksize, tmp);
        hipLaunchKernelGGL((resample_v_kernel<4>), g2, block, 0, st, (const uint8_t*)tmp, B, H, w, h, ybounds, yk, yksize, o);
    }
    RF_LAUNCH_CHECK("rf_resample_u8");
    return 0;
}
