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

// ---- The masked paste: an alpha plane made of the crop's face-parsing label map, and the paste through it.
// One separable pass over u8 planes [B, n, n], a block per ALPHA_TW x ALPHA_TH tile staged in LDS with its halo of `rad` <= ALPHA_RMAX
// samples along the pass's axis (x: VERT = false, y: VERT = true): the maximum (BOX = false) or the rounded mean (sum + rad) / (2 rad + 1)
// (BOX = true) of the 2 rad + 1 samples around each position.  Samples outside the plane are staged as 0: they never raise a maximum
// (the centre is inside and every value is >= 0) and count as 0 in the sum, so the mean falls off towards the border.  With `lut` the
// input is a label map and every sample is read as lut[label] ? 255 : 0.
constexpr int ALPHA_TW = 64, ALPHA_TH = 16, ALPHA_RMAX = 64;

template <bool VERT, bool BOX>
__global__ void __launch_bounds__(256) alpha_pass_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ lut, int n, int rad,
                                                         uint8_t* __restrict__ out) {
    constexpr int LW = VERT ? ALPHA_TW : ALPHA_TW + 2 * ALPHA_RMAX, LH = VERT ? ALPHA_TH + 2 * ALPHA_RMAX : ALPHA_TH;
    __shared__ uint8_t tile[LH * LW];
    const int x0 = blockIdx.x * ALPHA_TW, y0 = blockIdx.y * ALPHA_TH;
    const long long plane = (long long)blockIdx.z * n * n;
    const int w = VERT ? ALPHA_TW : ALPHA_TW + 2 * rad, h = VERT ? ALPHA_TH + 2 * rad : ALPHA_TH;
    const int ox = VERT ? x0 : x0 - rad, oy = VERT ? y0 - rad : y0;
    for (int i = threadIdx.x; i < w * h; i += 256) {
        const int ly = i / w, lx = i - ly * w, gx = ox + lx, gy = oy + ly;
        int v = 0;
        if (gx >= 0 && gx < n && gy >= 0 && gy < n) {
            v = in[plane + (long long)gy * n + gx];
            if (lut) v = lut[v] ? 255 : 0;
        }
        tile[ly * LW + lx] = (uint8_t)v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ALPHA_TW * ALPHA_TH / 256; ++k) {
        const int i = threadIdx.x + 256 * k, ly = i / ALPHA_TW, lx = i - ly * ALPHA_TW;
        if (x0 + lx >= n || y0 + ly >= n) continue;
        const uint8_t* t = tile + ly * LW + lx;
        int acc = BOX ? rad : 0;
        for (int j = 0; j <= 2 * rad; ++j) {
            const int v = t[VERT ? j * LW : j];
            acc = BOX ? acc + v : max(acc, v);
        }
        out[plane + (long long)(y0 + ly) * n + (x0 + lx)] = (uint8_t)(BOX ? acc / (2 * rad + 1) : acc);
    }
}

// One pixel of PIL's resize((S, S), BILINEAR) of the u8 planes [B, n, n] (mode L: the one-channel case of paste_crop_pixel); n == S copies
__device__ __forceinline__ int alpha_up_pixel(const uint8_t* __restrict__ m, int n, int S, long long p) {
    const long long SS = (long long)S * S;
    const int b = (int)(p / SS);
    const int r = (int)(p - (long long)b * SS), Y = r / S, X = r - (r / S) * S;
    const uint8_t* pl = m + (long long)b * n * n;
    if (n == S) return pl[(long long)Y * n + X];
    int xl, xn, kx[2], yl, yn, ky[2];
    pil_taps(X, n, S, xl, xn, kx);
    pil_taps(Y, n, S, yl, yn, ky);
    int acc = 1 << 21;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j >= yn) break;
        const uint8_t* row = pl + (long long)(yl + j) * n + xl;
        int s = 1 << 21;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (i < xn) s += kx[i] * row[i];
        acc += ky[j] * pil_clip8(s);
    }
    return pil_clip8(acc);
}

// u8 [B, n, n] -> u8 [B, S, S]; thread t writes pixels 4t .. 4t + 3 of the flat range as one word
__global__ void alpha_up_kernel(const uint8_t* __restrict__ m, int B, int n, int S, uint8_t* __restrict__ out) {
    const long long N = (long long)B * S * S;
    const long long p0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= N) return;
    uint8_t* o = out + p0;
    if (p0 + 4 <= N && ((uintptr_t)o & 3) == 0) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) word |= (uint32_t)alpha_up_pixel(m, n, S, p0 + q) << (8 * q);
        *(uint32_t*)o = word;
    } else {
        for (int q = 0; q < 4 && p0 + q < N; ++q) o[q] = (uint8_t)alpha_up_pixel(m, n, S, p0 + q);
    }
}

// libImaging's MULDIV255 and SHIFTFORDIV255: x * y / 255 and x / 255, rounded, without a division
__device__ __forceinline__ uint32_t pil_shift255(uint32_t x) { return ((x >> 8) + x) >> 8; }
__device__ __forceinline__ int pil_muldiv255(int x, int y) { return (int)pil_shift255((uint32_t)(x * y + 128)); }

// bilinear_filter32RGB (see pil_bilinear_rgb) on all four channels of the premultiplied image RGBa = (MULDIV255(c, a), a) of the crop RGB
// [S, S, 3] and its alpha plane [S, S]: the four taps are premultiplied as they are read, the RGBa crop is never stored.
__device__ __forceinline__ void pil_bilinear_premul(const uint8_t* __restrict__ crop, const uint8_t* __restrict__ alpha, int S, double sx, double sy,
                                                    int p[4]) {
    const double u = sx - 0.5, v = sy - 0.5;
    const double fx = floor(u), fy = floor(v);
    const int x0 = (int)fx, y0 = (int)fy;
    const double dx = u - fx, dy = v - fy;
    const int cx0 = min(max(x0, 0), S - 1), cx1 = min(max(x0 + 1, 0), S - 1), cy0 = min(max(y0, 0), S - 1);
    const bool row2 = y0 + 1 >= 0 && y0 + 1 < S;
    const long long r0 = (long long)cy0 * S, r1 = row2 ? (long long)(y0 + 1) * S : r0;
    const long long at[4] = {r0 + cx0, r0 + cx1, r1 + cx0, r1 + cx1};
    int a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = alpha[at[k]];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = (double)(ch < 3 ? pil_muldiv255(crop[at[k] * 3 + ch], a[k]) : a[k]);
        const double v1 = t[0] + (t[1] - t[0]) * dx;
        double v2 = v1;
        if (row2) v2 = t[2] + (t[3] - t[2]) * dx;
        p[ch] = (int)(v1 + (v2 - v1) * dy);
    }
}

// paste_back_kernel with the crop's alpha plane [B, S, S] in place of alpha 255: Image.transform of the RGBA crop (PIL warps its premultiplied
// form RGBa and converts back: c = min(255, 255 c / a) unless a is 0 or 255) and Image.alpha_composite over the frame (AlphaComposite.c, 7
// precision bits).  Where the warped alpha is 0 -- outside the quad, or where the four taps' alpha is 0 -- the frame pixel stays bit for bit.
template <int Cf, int Co>
__global__ void paste_back_alpha_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ alphas, int S, const double* __restrict__ coeffs,
                                        const uint8_t* frames, int H, int W, long long fstride, uint8_t* out, int B) {
    const long long HW = (long long)H * W, G = (HW + 3) / 4;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * G) return;
    const int b = (int)(t / G);
    const long long p0 = (t - (long long)b * G) * 4;
    const int nq = (int)min(4LL, HW - p0);
    const double* c = coeffs + (long long)b * 8;
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5], c6 = c[6], c7 = c[7];
    const uint8_t* crop = crops + (long long)b * S * S * 3;
    const uint8_t* al = alphas + (long long)b * S * S;
    const uint8_t* fr = frames + (long long)b * fstride + p0 * Cf;
    uint8_t* o = out + ((long long)b * HW + p0) * Co;
    uint8_t fb[4 * Cf];          // the frame's bytes of this group: Cf words when aligned and whole, else per byte
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
    uint8_t px[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        px[q][3] = 255;
#pragma unroll
        for (int ch = 0; ch < Cf; ++ch) px[q][ch] = fb[q * Cf + ch];
        if (q >= nq) continue;
        const long long p = p0 + q;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        const double xi = (double)x + 0.5, yi = (double)y + 0.5;
        const double d = c6 * xi + c7 * yi + 1.0;
        const double sx = (c0 * xi + c1 * yi + c2) / d;
        const double sy = (c3 * xi + c4 * yi + c5) / d;
        if (!(sx >= 0.0 && sx < (double)S && sy >= 0.0 && sy < (double)S)) continue;          // (also when not finite)
        int s[4];
        pil_bilinear_premul(crop, al, S, sx, sy, s);
        const uint32_t pa = (uint32_t)s[3];
        if (pa == 0) continue;
        const uint32_t da = px[q][3];
        const uint32_t blend = da * (255 - pa), outa255 = pa * 255 + blend;
        const uint32_t coef1 = pa * 255 * 255 * 128 / outa255, coef2 = 255 * 128 - coef1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t sc = pa == 255 ? (uint32_t)s[ch] : min(255u, 255u * (uint32_t)s[ch] / pa);
            px[q][ch] = (uint8_t)(pil_shift255(sc * coef1 + (uint32_t)px[q][ch] * coef2 + (0x80 << 7)) >> 7);
        }
        px[q][3] = (uint8_t)pil_shift255(outa255 + 0x80);
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

extern "C" int rf_paste_alpha_u8(const void* labels_u8, int B, int Sl, const void* lut256_u8, int dilate, int feather, int passes, void* scratch_u8,
                                 int64_t scratch_bytes, void* alpha_u8, int S, void* stream) {
    RF_CHECK(labels_u8 && lut256_u8 && scratch_u8 && alpha_u8 && B > 0 && B <= 65535 && Sl > 0 && S > 0,
             "rf_paste_alpha_u8: bad arguments (B=%d Sl=%d S=%d)", B, Sl, S);
    RF_CHECK(dilate >= 0 && dilate <= ALPHA_RMAX && feather >= 0 && feather <= ALPHA_RMAX,
             "rf_paste_alpha_u8: dilate and feather are 0 .. %d (dilate=%d feather=%d)", ALPHA_RMAX, dilate, feather);
    RF_CHECK(passes >= 1 && passes <= 3, "rf_paste_alpha_u8: passes is 1 .. 3, got %d", passes);
    RF_CHECK(S >= Sl, "rf_paste_alpha_u8: only upscaling is supported (%d -> %d)", Sl, S);
    const long long plane = (long long)B * Sl * Sl;
    RF_CHECK(scratch_bytes >= 2 * plane, "rf_paste_alpha_u8: scratch of %lld bytes < 2 * B * Sl * Sl = %lld", (long long)scratch_bytes, 2 * plane);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((Sl + ALPHA_TW - 1) / ALPHA_TW), (unsigned)((Sl + ALPHA_TH - 1) / ALPHA_TH), (unsigned)B), block(256);
    uint8_t* cur = (uint8_t*)scratch_u8;          // the two planes of the ping-pong: every pass reads one and writes the other
    uint8_t* nxt = cur + plane;
    hipLaunchKernelGGL((alpha_pass_kernel<false, false>), grid, block, 0, st, (const uint8_t*)labels_u8, (const uint8_t*)lut256_u8, Sl, dilate, cur);
    if (dilate > 0) {
        hipLaunchKernelGGL((alpha_pass_kernel<true, false>), grid, block, 0, st, (const uint8_t*)cur, (const uint8_t*)nullptr, Sl, dilate, nxt);
        std::swap(cur, nxt);
    }
    for (int k = 0; k < (feather > 0 ? passes : 0); ++k) {
        hipLaunchKernelGGL((alpha_pass_kernel<false, true>), grid, block, 0, st, (const uint8_t*)cur, (const uint8_t*)nullptr, Sl, feather, nxt);
        hipLaunchKernelGGL((alpha_pass_kernel<true, true>), grid, block, 0, st, (const uint8_t*)nxt, (const uint8_t*)nullptr, Sl, feather, cur);
    }
    const long long groups = ((long long)B * S * S + 3) / 4;
    hipLaunchKernelGGL(alpha_up_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, (const uint8_t*)cur, B, Sl, S, (uint8_t*)alpha_u8);
    RF_LAUNCH_CHECK("rf_paste_alpha_u8");
    return 0;
}

extern "C" int rf_paste_back_alpha_u8(const void* crops_u8, const void* alpha_u8, int B, int S, const double* coeffs, const void* frames_u8, int H,
                                      int W, int Cf, int64_t frame_stride, void* out_u8, int Co, void* stream) {
    RF_CHECK(crops_u8 && alpha_u8 && coeffs && frames_u8 && out_u8 && B > 0 && S > 0 && H > 0 && W > 0,
             "rf_paste_back_alpha_u8: bad arguments (B=%d S=%d H=%d W=%d)", B, S, H, W);
    RF_CHECK((Cf == 3 || Cf == 4) && (Co == 3 || Co == 4), "rf_paste_back_alpha_u8: frame / output channels must be 3 or 4 (Cf=%d Co=%d)", Cf, Co);
    RF_CHECK(frame_stride >= (int64_t)H * W * Cf, "rf_paste_back_alpha_u8: frame stride %lld < H * W * Cf", (long long)frame_stride);
    RF_CHECK(out_u8 != frames_u8 || (Cf == Co && frame_stride == (int64_t)H * W * Cf),
             "rf_paste_back_alpha_u8: in place (out == frames) needs Cf == Co and packed frames");
    const long long n = (long long)B * (((long long)H * W + 3) / 4);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const uint8_t* cr = (const uint8_t*)crops_u8;
    const uint8_t* al = (const uint8_t*)alpha_u8;
    const uint8_t* fr = (const uint8_t*)frames_u8;
    uint8_t* o = (uint8_t*)out_u8;
    const long long fs = (long long)frame_stride;
    hipStream_t st = (hipStream_t)stream;
    if (Cf == 3 && Co == 3) hipLaunchKernelGGL((paste_back_alpha_kernel<3, 3>), grid, block, 0, st, cr, al, S, coeffs, fr, H, W, fs, o, B);
    else if (Cf == 3 && Co == 4) hipLaunchKernelGGL((paste_back_alpha_kernel<3, 4>), grid, block, 0, st, cr, al, S, coeffs, fr, H, W, fs, o, B);
    else if (Cf == 4 && Co == 3) hipLaunchKernelGGL((paste_back_alpha_kernel<4, 3>), grid, block, 0, st, cr, al, S, coeffs, fr, H, W, fs, o, B);
    else hipLaunchKernelGGL((paste_back_alpha_kernel<4, 4>), grid, block, 0, st, cr, al, S, coeffs, fr, H, W, fs, o, B);
    RF_LAUNCH_CHECK("rf_paste_back_alpha_u8");
    return 0;
}
