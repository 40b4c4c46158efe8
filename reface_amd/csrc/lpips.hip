// The learned perceptual distance of the evaluation (eval_tool/lpips/{lpips,networks,utils}.py of the reference: LPIPS over AlexNet or VGG16
// features).  The convolutions run on rf_conv_gemm; the kernels around them:
//   rf_lpips_prep_u8 / rf_lpips_prep_f32   ToTensor + Normalize(0.5, 0.5) (u8 only) and BaseNet.z_score (networks.py:50-51) into the stem's layout;
//   rf_maxpool2d                           MaxPool2d(k, 2), k = 2 (VGG16) or 3 (AlexNet): no padding, floor mode;
//   rf_lpips_layer                         normalize_activation (utils.py:6-8) of both feature maps, (nx - ny)^2, the 1x1 `lin` convolution and
//                                          the spatial mean (lpips.py:32-33), in one read of the two maps;
//   rf_lpips_total                         the sum over layers per pair and over pairs (lpips.py:35).
#include "common.h"

namespace rf {

constexpr int LPIPS_CP = 8;                     // 3 channels stored in 8: the layout of the stems (cin_pad = 8)
constexpr int LPIPS_BLOCKS = RF_LPIPS_MAX_BLOCKS;          // blocks per image of rf_lpips_layer at the most (= partial sums per image in the scratch)

// BaseNet's buffers (networks.py:41-44), fp32 as torch.Tensor([...]) stores them
__device__ __forceinline__ float lpips_z(float x, int c) {
    const float mean[3] = {-.030f, -.088f, -.188f}, stdv[3] = {.458f, .448f, .450f};
    return (x - mean[c]) / stdv[c];
}

// ---- out[b, p, c] = z((float(byte) / 255 - 0.5) / 0.5), c < 3; 0 for c = 3..7.  Every step rounds to fp32 on its own (the unit builds with
// -ffp-contract=off).  One thread per pixel, pixels on lanes: a wave writes 64 consecutive 32-byte pixels.
__global__ __launch_bounds__(256) void lpips_prep_u8_kernel(const uint8_t* __restrict__ img, int B, long long HW, long long simg, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // over B * HW
    if (i >= (long long)B * HW) return;
    const long long b = i / HW, p = i - b * HW;
    const uint8_t* s = img + b * simg + p * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lpips_z(((float)s[c] / 255.0f - 0.5f) / 0.5f, c);
    float4* o = reinterpret_cast<float4*>(out + i * LPIPS_CP);
    o[0] = make_float4(v[0], v[1], v[2], 0.f);
    o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- the same z-score and layout from fp32 NCHW [B, 3, H, W]: a wave reads three runs of 64 consecutive floats
__global__ __launch_bounds__(256) void lpips_prep_f32_kernel(const float* __restrict__ x, int B, long long HW, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * HW) return;
    const long long b = i / HW, p = i - b * HW;
    const float* s = x + b * 3 * HW + p;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lpips_z(s[c * HW], c);
    float4* o = reinterpret_cast<float4*>(out + i * LPIPS_CP);
    o[0] = make_float4(v[0], v[1], v[2], 0.f);
    o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- MaxPool2d(K, stride 2): no padding, floor mode, so every window lies inside the image.  One thread per 16-byte vector of channels.
template <int K>
__global__ __launch_bounds__(256) void maxpool2d_kernel(const float* __restrict__ x, int B, int H, int W, int C4, int Ho, int Wo, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // over B * Ho * Wo * C4
    if (i >= (long long)B * Ho * Wo * C4) return;
    const int c = (int)(i % C4);
    const long long pix = i / C4;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const long long b = pix / ((long long)Wo * Ho);
    const float4* xv = reinterpret_cast<const float4*>(x);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const float4 v = xv[((b * H + (2 * oy + dy)) * W + (2 * ox + dx)) * C4 + c];
            m.x = fmaxf(m.x, v.x);
            m.y = fmaxf(m.y, v.y);
            m.z = fmaxf(m.z, v.z);
            m.w = fmaxf(m.w, v.w);
        }
    reinterpret_cast<float4*>(out)[i] = m;
}

// ---- part[b, k] = the sum over the pixels of block k of image pair b of sum_c w[c] (n(fx)[c] - n(fy)[c])^2, n(f) = f / (sqrt(sum_c f^2 + 1e-16) + 1e-10).
// A pixel's channels sit in the registers of a group of G lanes (G a power of two, 1..32): lane j of the group holds the 16-byte vectors
// j, j + G, .. (NV of them at the most) of both maps, so a group reads runs of 16 G consecutive bytes and every byte is read once.  The two
// squared norms meet over the group by xor shuffles; the vectors stay in registers between the norm pass and the difference pass.  The direct
// form (normalise, subtract, square, weight) is kept: the expanded five-sum form cancels for near-equal maps.  The features are fp32; what is
// computed FROM them is fp64 (norms, the two reciprocals per pixel, every difference, square and sum): the distance of near-equal maps is a
// difference of nearly equal normalised channels, and an fp32 rounding of each (6e-8 of the channel against a difference of 1e-3 of it) would
// leave a single pixel's sum off by about 1e-5.  At 8 bytes read per channel pair the fp64 work (7 operations) stays under the memory time.
// The lanes of the block meet in a fixed tree.  Nothing here depends on B: the grid is (blocks per image, B) and the blocks per image follow
// from HW and G alone, so a pair's sum has the same bits in any batch.
// An all-zero pixel has norm sqrt(1e-16) + 1e-10 and normalises to zeros; where fx == fy bit for bit every difference is exactly 0.
template <int NV>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ fx, const float* __restrict__ fy, long long HW, int C4, int G,
                                                          const float* __restrict__ w, double* __restrict__ part) {
    __shared__ double red[4];
    const int t = threadIdx.x, j = t & (G - 1), g = t / G;
    const int ppb = 256 / G;                                    // pixels per block and pass
    const long long b = blockIdx.y;
    const float4* x4 = reinterpret_cast<const float4*>(fx) + b * HW * C4;
    const float4* y4 = reinterpret_cast<const float4*>(fy) + b * HW * C4;
    float4 wv[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int v = j + q * G;
        wv[q] = v < C4 ? reinterpret_cast<const float4*>(w)[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double acc = 0.0;
    // the trip count is the same for every thread of the block: the shuffles below are never divergent
    for (long long base = (long long)blockIdx.x * ppb; base < HW; base += (long long)gridDim.x * ppb) {
        const long long p = base + g;
        const bool live = p < HW;
        float4 a[NV], c[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int v = j + q * G;
            const bool ok = live && v < C4;
            a[q] = ok ? x4[p * C4 + v] : make_float4(0.f, 0.f, 0.f, 0.f);
            c[q] = ok ? y4[p * C4 + v] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        double sa = 0.0, sc = 0.0;          // (the product of two widened fp32 values is exact in fp64)
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            sa += (double)a[q].x * (double)a[q].x;
            sa += (double)a[q].y * (double)a[q].y;
            sa += (double)a[q].z * (double)a[q].z;
            sa += (double)a[q].w * (double)a[q].w;
            sc += (double)c[q].x * (double)c[q].x;
            sc += (double)c[q].y * (double)c[q].y;
            sc += (double)c[q].z * (double)c[q].z;
            sc += (double)c[q].w * (double)c[q].w;
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            sa += __shfl_xor(sa, o, 64);
            sc += __shfl_xor(sc, o, 64);
        }
        const double ra = 1.0 / (sqrt(sa + 1e-16) + 1e-10), rc = 1.0 / (sqrt(sc + 1e-16) + 1e-10);
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            double d;
            d = (double)a[q].x * ra - (double)c[q].x * rc;
            s += (double)wv[q].x * (d * d);
            d = (double)a[q].y * ra - (double)c[q].y * rc;
            s += (double)wv[q].y * (d * d);
            d = (double)a[q].z * ra - (double)c[q].z * rc;
            s += (double)wv[q].z * (d * d);
            d = (double)a[q].w * ra - (double)c[q].w * rc;
            s += (double)wv[q].w * (d * d);
        }
        acc += s;          // (dead lanes hold zeros: s == 0)
    }
    acc = wave_sum_d(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) part[b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// vals[b * L + l] = (sum_k part[b, k], thread-strided partial sums and a tree: one fixed order) / HW, in fp64.  One block per image pair.
__global__ __launch_bounds__(256) void lpips_layer_finish_kernel(const double* __restrict__ part, int nblk, long long HW, double* __restrict__ vals, int L, int l) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long long b = blockIdx.x;
    double s = 0.0;
    for (int k = t; k < nblk; k += 256) s += part[b * nblk + k];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) vals[b * L + l] = red[0] / (double)HW;
}

// d[b] = sum_l vals[b, l], l ascending
__global__ __launch_bounds__(256) void lpips_pair_kernel(const double* __restrict__ vals, int B, int L, double* __restrict__ d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int l = 0; l < L; ++l) s += vals[(long long)b * L + l];
    d[b] = s;
}

// totals[0..1] = (sum_b d[b], b ascending: one thread, the order of the reference's own sum over the concatenated rows; B)
__global__ void lpips_totals_kernel(const double* __restrict__ d, int B, double* __restrict__ totals) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += d[b];
    totals[0] = s;
    totals[1] = (double)B;
}

static inline bool lpips_grid(long long n, dim3* g) {
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return false;
    *g = dim3((unsigned)blocks);
    return true;
}

}  // namespace rf

using namespace rf;

extern "C" int rf_lpips_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, float* out, void* stream) {
    RF_CHECK(images_u8 && out, "rf_lpips_prep_u8: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0, "rf_lpips_prep_u8: bad sizes (B=%d image %dx%d)", B, W, H);
    RF_CHECK(image_stride >= (int64_t)H * W * 3, "rf_lpips_prep_u8: image stride smaller than one image");
    RF_CHECK(((uintptr_t)out & 15) == 0, "rf_lpips_prep_u8: out must be 16-byte aligned");
    dim3 grid;
    RF_CHECK(lpips_grid((long long)B * H * W, &grid), "rf_lpips_prep_u8: B=%d images of %dx%d are too many for one launch", B, W, H);
    hipLaunchKernelGGL(lpips_prep_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, B, (long long)H * W, (long long)image_stride, out);
    RF_LAUNCH_CHECK("rf_lpips_prep_u8");
    return 0;
}

extern "C" int rf_lpips_prep_f32(const float* x_nchw, int B, int H, int W, float* out, void* stream) {
    RF_CHECK(x_nchw && out, "rf_lpips_prep_f32: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0, "rf_lpips_prep_f32: bad sizes (B=%d image %dx%d)", B, W, H);
    RF_CHECK(((uintptr_t)out & 15) == 0, "rf_lpips_prep_f32: out must be 16-byte aligned");
    dim3 grid;
    RF_CHECK(lpips_grid((long long)B * H * W, &grid), "rf_lpips_prep_f32: B=%d images of %dx%d are too many for one launch", B, W, H);
    hipLaunchKernelGGL(lpips_prep_f32_kernel, grid, dim3(256), 0, (hipStream_t)stream, x_nchw, B, (long long)H * W, out);
    RF_LAUNCH_CHECK("rf_lpips_prep_f32");
    return 0;
}

extern "C" int rf_maxpool2d(const float* x, int B, int H, int W, int C, int k, float* out, void* stream) {
    RF_CHECK(x && out, "rf_maxpool2d: null argument");
    RF_CHECK(k == 2 || k == 3, "rf_maxpool2d: window %d (2 or 3)", k);
    RF_CHECK(B > 0 && H >= k && W >= k && C > 0 && C % 4 == 0, "rf_maxpool2d: bad sizes (B=%d H=%d W=%d C=%d: H, W >= %d, C a multiple of 4)", B, H, W, C, k);
    RF_CHECK((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "rf_maxpool2d: x and out must be 16-byte aligned");
    const int Ho = (H - k) / 2 + 1, Wo = (W - k) / 2 + 1;
    dim3 grid;
    RF_CHECK(lpips_grid((long long)B * Ho * Wo * (C / 4), &grid), "rf_maxpool2d: too many outputs for one launch");
    if (k == 2) hipLaunchKernelGGL(maxpool2d_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, B, H, W, C / 4, Ho, Wo, out);
    else hipLaunchKernelGGL(maxpool2d_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, x, B, H, W, C / 4, Ho, Wo, out);
    RF_LAUNCH_CHECK("rf_maxpool2d");
    return 0;
}

extern "C" int rf_lpips_layer(const float* fx, const float* fy, int B, int64_t HW, int C, const float* w, double* scratch, int64_t scratch_doubles,
                              double* vals, int L, int l, void* stream) {
    RF_CHECK(fx && fy && w && scratch && vals, "rf_lpips_layer: null argument");
    RF_CHECK(B > 0 && B <= 65535 && HW > 0, "rf_lpips_layer: bad sizes (B=%d in 1..65535, HW=%lld)", B, (long long)HW);
    RF_CHECK(C >= 4 && C <= 512 && C % 4 == 0, "rf_lpips_layer: C=%d must be a multiple of 4 in 4..512", C);
    RF_CHECK(L > 0 && l >= 0 && l < L, "rf_lpips_layer: layer %d of %d", l, L);
    RF_CHECK((((uintptr_t)fx | (uintptr_t)fy | (uintptr_t)w) & 15) == 0, "rf_lpips_layer: fx, fy and w must be 16-byte aligned");
    const int C4 = C / 4;
    // lanes per pixel: enough for four vectors per lane at the most, and 16 (256 consecutive bytes per group) once the pixel is that long
    int G = 1;
    while (G * 4 < C4) G *= 2;
    while (G < 16 && G < C4) G *= 2;
    const int NV = (C4 + G - 1) / G, ppb = 256 / G;
    const long long want = (HW + ppb - 1) / ppb;
    const int nblk = (int)(want < LPIPS_BLOCKS ? want : LPIPS_BLOCKS);
    RF_CHECK(scratch_doubles >= (int64_t)B * nblk, "rf_lpips_layer: scratch of %lld doubles, %lld needed (B * min(RF_LPIPS_MAX_BLOCKS, pixel groups))",
             (long long)scratch_doubles, (long long)B * nblk);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk, (unsigned)B);
    switch (NV) {
        case 1: hipLaunchKernelGGL(lpips_layer_kernel<1>, grid, dim3(256), 0, st, fx, fy, (long long)HW, C4, G, w, scratch); break;
        case 2: hipLaunchKernelGGL(lpips_layer_kernel<2>, grid, dim3(256), 0, st, fx, fy, (long long)HW, C4, G, w, scratch); break;
        case 3: hipLaunchKernelGGL(lpips_layer_kernel<3>, grid, dim3(256), 0, st, fx, fy, (long long)HW, C4, G, w, scratch); break;
        default: hipLaunchKernelGGL(lpips_layer_kernel<4>, grid, dim3(256), 0, st, fx, fy, (long long)HW, C4, G, w, scratch); break;
    }
    hipLaunchKernelGGL(lpips_layer_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)scratch, nblk, (long long)HW, vals, L, l);
    RF_LAUNCH_CHECK("rf_lpips_layer");
    return 0;
}

extern "C" int rf_lpips_total(const double* vals, int B, int L, double* d, double* totals, void* stream) {
    RF_CHECK(vals && d && totals, "rf_lpips_total: null argument");
    RF_CHECK(B > 0 && L > 0, "rf_lpips_total: bad sizes (B=%d L=%d)", B, L);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_pair_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, vals, B, L, d);
    hipLaunchKernelGGL(lpips_totals_kernel, dim3(1), dim3(64), 0, st, (const double*)d, B, totals);
    RF_LAUNCH_CHECK("rf_lpips_total");
    return 0;
}
