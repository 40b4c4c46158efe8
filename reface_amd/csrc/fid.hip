// The FID of the evaluation (eval_tool/fid/fid_score.py of the reference, whose "inception" returns the `clip` ViT-B/32 image features): the
// two passes around the vision tower, which runs on rf_conv_gemm / rf_attention / rf_layernorm:
//   rf_fid_prep_u8   clip.load's `preprocess` on device bytes: Resize(224, BICUBIC) (PIL's two integer passes), CenterCrop(224), ToTensor,
//                    Normalize, NHWC in the engine's dtype, in one pass;
//   rf_fid_stats     np.mean(act, 0) and np.cov(act, rowvar=False) of the float64 activations: fp64 mean, then the centred Gram matrix on
//                    v_mfma_f64_16x16x4_f64 over the upper-triangle tiles.
// The vertical pass of the resize needs no intermediate in global memory at any source size: the horizontally resampled rows a tile's
// vertical windows cover pass through LDS in chunks of FP_TMP_ROWS rows (one chunk at 1024 -> 224 and below).
#include "pil_u8.h"

namespace rf {

constexpr int FID_S = 224;           // side of the tower's input
constexpr int FP_TW = 32, FP_TH = 16, FP_THREADS = 256, FP_Q = FP_TH / (FP_THREADS / FP_TW);
constexpr int FP_TMP_ROWS = 96;      // 12 KiB of horizontally resampled rows (RGBx words): the ~90 rows of a 16-row tile at 1024 -> 224

// bounds[2 i] = first input index, bounds[2 i + 1] = tap count of output index i, clipped to the table's width and to the axis: whatever the
// table holds, no tap lies outside [0, n_in)
__device__ __forceinline__ void fp_window(const int* __restrict__ bounds, int i, int ksize, int n_in, int& lo, int& n) {
    lo = min(max(bounds[2 * i], 0), n_in - 1);
    n = max(min(bounds[2 * i + 1], min(ksize, n_in - lo)), 0);
}

// torchvision's ToTensor and Normalize on one byte: float32(b) / 255, then (x - mean) / std, each operation rounded to fp32 (this unit builds
// without FMA contraction and with IEEE division)
__device__ __forceinline__ float fp_norm(int byte, float mean, float std) {
    const float x = (float)byte / 255.0f;
    return (x - mean) / std;
}

template <typename TO> __device__ __forceinline__ void fp_store(TO* o, float r, float g, float b);
template <> __device__ __forceinline__ void fp_store<float>(float* o, float r, float g, float b) {          // CP = 4: one 16-byte pixel
    *reinterpret_cast<float4*>(o) = make_float4(r, g, b, 0.f);
}
template <> __device__ __forceinline__ void fp_store<bf16_t>(bf16_t* o, float r, float g, float b) {        // CP = 8: one 16-byte pixel
    *reinterpret_cast<u32x4_t*>(o) = u32x4_t{pack_bf2(r, g), pack_bf2(b, 0.f), 0u, 0u};
}

// ---- out[b, y, x, c] = normalise(crop(resize(img)))[y, x, c], c < 3; 0 for the pad channels.  The host passes each axis's tap table already
// sliced to the 224 outputs inside the crop window, so nothing outside the crop is computed.  PIL resizes in two integer passes with a u8
// image between them (Resample.c: ImagingResampleHorizontal_8bpc, then Vertical_8bpc, each clip8(((1 << 21) + sum k p) >> 22)); the rounding
// between the passes is part of the result, so both are kept.  With the identity table of an unchanged axis (one tap of 1 << 22) a pass
// returns the byte.
// A block owns FP_TH x FP_TW output pixels (224 is a multiple of both).  Per chunk of the input rows its vertical windows cover:
//   1. the horizontal pass of those rows for the tile's 32 columns: global bytes -> one RGBx word per (row, column) in LDS,
//   2. every thread adds the chunk's rows into the vertical sums of its 2 output pixels (column tid % 32, rows tid / 32 + 8 q).
template <typename TO, int CP>
__global__ void __launch_bounds__(FP_THREADS)
fid_prep_kernel(const uint8_t* __restrict__ images, int H, int W, long long simg, const int* __restrict__ xb, const int* __restrict__ xk, int xks,
                const int* __restrict__ yb, const int* __restrict__ yk, int yks, TO* __restrict__ out) {
    __shared__ uint32_t tmp[FP_TMP_ROWS * FP_TW];
    constexpr int TX = FID_S / FP_TW, TY = FID_S / FP_TH, RS = FP_THREADS / FP_TW;
    static_assert(FID_S % FP_TW == 0 && FID_S % FP_TH == 0 && FP_THREADS % FP_TW == 0 && FP_TH % RS == 0, "tile shape");
    const int tid = threadIdx.x, tx = tid % FP_TW, ty = tid / FP_TW;
    const int bx = blockIdx.x % TX, by = (blockIdx.x / TX) % TY, b = blockIdx.x / (TX * TY);
    const int x = bx * FP_TW + tx, y0 = by * FP_TH;
    const uint8_t* img = images + (long long)b * simg;
    int xlo, xn;
    fp_window(xb, x, xks, W, xlo, xn);
    const int* kx = xk + (long long)x * xks;
    int rbeg = 0x7fffffff, rend = 0;          // the input rows of the tile's 16 vertical windows (the same in every thread)
    for (int i = 0; i < FP_TH; ++i) {
        int lo, n;
        fp_window(yb, y0 + i, yks, H, lo, n);
        if (n > 0) {
            rbeg = min(rbeg, lo);
            rend = max(rend, lo + n);
        }
    }
    int ylo[FP_Q], yn[FP_Q], acc[FP_Q][3];
#pragma unroll
    for (int q = 0; q < FP_Q; ++q) {
        fp_window(yb, y0 + ty + RS * q, yks, H, ylo[q], yn[q]);
        acc[q][0] = acc[q][1] = acc[q][2] = 1 << 21;
    }
    for (int r0 = rbeg; r0 < rend; r0 += FP_TMP_ROWS) {
        const int rows = min(FP_TMP_ROWS, rend - r0);
        for (int it = tid; it < rows * FP_TW; it += FP_THREADS) {          // (it % FP_TW == tx: a thread keeps its column)
            const int rl = it / FP_TW;
            const uint8_t* in = img + ((long long)(r0 + rl) * W + xlo) * 3;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int i = 0; i < xn; ++i) {
                const int k = kx[i];
                a0 += k * (int)in[3 * i];
                a1 += k * (int)in[3 * i + 1];
                a2 += k * (int)in[3 * i + 2];
            }
            tmp[rl * FP_TW + tx] = (uint32_t)pil_clip8(a0) | ((uint32_t)pil_clip8(a1) << 8) | ((uint32_t)pil_clip8(a2) << 16);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < FP_Q; ++q) {
            const int* ky = yk + (long long)(y0 + ty + RS * q) * yks;
            const int rb = max(ylo[q], r0), re = min(ylo[q] + yn[q], r0 + rows);
            for (int r = rb; r < re; ++r) {
                const int k = ky[r - ylo[q]];
                const uint32_t p = tmp[(r - r0) * FP_TW + tx];
                acc[q][0] += k * (int)(p & 255u);
                acc[q][1] += k * (int)((p >> 8) & 255u);
                acc[q][2] += k * (int)((p >> 16) & 255u);
            }
        }
        if (r0 + FP_TMP_ROWS < rend) __syncthreads();          // the next chunk overwrites tmp
    }
#pragma unroll
    for (int q = 0; q < FP_Q; ++q) {
        const int y = y0 + ty + RS * q;
        TO* o = out + (((long long)b * FID_S + y) * FID_S + x) * CP;          // 16-byte pixels of a 16-byte aligned buffer
        fp_store<TO>(o, fp_norm(pil_clip8(acc[q][0]), 0.48145466f, 0.26862954f), fp_norm(pil_clip8(acc[q][1]), 0.4578275f, 0.26130258f),
                     fp_norm(pil_clip8(acc[q][2]), 0.40821073f, 0.27577711f));
    }
}

// ---- mu[c] = (sum_i (double)x[i, c]) / N.  A block owns 16 columns: thread (r, c) = (tid / 16, tid % 16) sums rows r, r + 16, ... in
// ascending order (a wave reads four 64-byte row segments per step), then thread (0, c) adds the 16 partials in ascending r.  The order is
// fixed: the same bits on every run.
__global__ __launch_bounds__(256) void fid_mean_kernel(const float* __restrict__ x, int N, int D, double* __restrict__ mu) {
    __shared__ double part[16][16];
    const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + c;
    double s = 0.0;
    for (int i = r; i < N; i += 16) s += (double)x[(long long)i * D + col];
    part[r][c] = s;
    __syncthreads();
    if (r == 0) {
        double t = part[0][c];
        for (int k = 1; k < 16; ++k) t += part[k][c];
        mu[col] = t / (double)N;
    }
}

typedef __attribute__((ext_vector_type(4))) double f64x4_t;

// ---- sigma = sum_i (x_i - mu)(x_i - mu)^T * (1 / (N - 1)), values widened before the subtraction (np.cov: X -= avg; dot(X, X.T) * (1 / fact)).
// One wave per 16 x 16 tile (ti, tj), ti <= tj, of the upper triangle, the whole N in ascending order in that wave's accumulators: no atomics,
// no split of N, the same bits on every run.  v_mfma_f64_16x16x4_f64: lane l brings A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15],
// here A[i][k] = xc[k0 + k][16 ti + i] and B[k][j] = xc[k0 + k][16 tj + j] (rows k0 + k >= N enter as 0), and leaves with
// C[row = (l >> 4) + 4 reg][col = l & 15], reg < 4.  Each result is stored at (row, col) of tile (ti, tj) and at its mirror from the same
// register; a diagonal tile stores its row <= col half only, so sigma is symmetric in every bit.
__global__ __launch_bounds__(256) void fid_gram_kernel(const float* __restrict__ x, int N, int D, const double* __restrict__ mu, double* __restrict__ sigma) {
    const int T = D >> 4, npair = T * (T + 1) / 2;
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform
    if (pair >= npair) return;
    int ti = 0, rem = pair;
    while (rem >= T - ti) {
        rem -= T - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int l15 = lane & 15, l4 = lane >> 4;
    const double ma = mu[ti * 16 + l15], mb = mu[tj * 16 + l15];
    const float* xa = x + ti * 16 + l15;
    const float* xb = x + tj * 16 + l15;
    f64x4_t acc = {0.0, 0.0, 0.0, 0.0};
    int k0 = 0;
    for (; k0 + 16 <= N; k0 += 16) {          // four K steps per trip: eight independent loads in flight
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long row = (long long)(k0 + 4 * u + l4) * D;
            a[u] = (double)xa[row] - ma;
            b[u] = (double)xb[row] - mb;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    for (; k0 < N; k0 += 4) {                 // the tail, rows past N zero-filled
        const int k = k0 + l4;
        double a = 0.0, b = 0.0;
        if (k < N) {
            a = (double)xa[(long long)k * D] - ma;
            b = (double)xb[(long long)k * D] - mb;
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    const double inv = 1.0 / (double)(N - 1);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = l4 + 4 * reg, col = l15;
        if (ti != tj || row <= col) {
            const double acc_r = acc[reg];
            const double v = acc_r * inv;
            const long long gr = ti * 16 + row, gc = tj * 16 + col;
            sigma[gr * D + gc] = v;
            sigma[gc * D + gr] = v;
        }
    }
}

template <typename TO, int CP>
static int launch_fid_prep(const uint8_t* images, int B, int H, int W, long long simg, const int* xb, const int* xk, int xks, const int* yb, const int* yk,
                           int yks, void* out, hipStream_t st) {
    const long long blocks = (long long)B * (FID_S / FP_TW) * (FID_S / FP_TH);
    RF_CHECK(blocks < (1LL << 31), "rf_fid_prep_u8: B=%d is too large for one launch", B);
    hipLaunchKernelGGL((fid_prep_kernel<TO, CP>), dim3((unsigned)blocks), dim3(FP_THREADS), 0, st, images, H, W, simg, xb, xk, xks, yb, yk, yks, (TO*)out);
    RF_LAUNCH_CHECK("rf_fid_prep_u8");
    return 0;
}

}  // namespace rf

using namespace rf;

extern "C" int rf_fid_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, const int* xbounds, const int* xk, int xksize,
                              const int* ybounds, const int* yk, int yksize, int out_dtype, void* out, void* stream) {
    RF_CHECK(images_u8 && xbounds && xk && ybounds && yk && out, "rf_fid_prep_u8: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0 && xksize > 0 && yksize > 0, "rf_fid_prep_u8: bad sizes (B=%d image %dx%d, ksize %d / %d)", B, W, H, xksize, yksize);
    RF_CHECK(image_stride >= (int64_t)H * W * 3, "rf_fid_prep_u8: image stride smaller than one image");
    RF_CHECK(out_dtype == RF_F32 || out_dtype == RF_BF16, "rf_fid_prep_u8: out_dtype %d is neither RF_F32 nor RF_BF16", out_dtype);
    RF_CHECK(((uintptr_t)out & 15) == 0, "rf_fid_prep_u8: out must be 16-byte aligned");
    if (out_dtype == RF_F32)
        return launch_fid_prep<float, 4>((const uint8_t*)images_u8, B, H, W, (long long)image_stride, xbounds, xk, xksize, ybounds, yk, yksize, out, (hipStream_t)stream);
    return launch_fid_prep<bf16_t, 8>((const uint8_t*)images_u8, B, H, W, (long long)image_stride, xbounds, xk, xksize, ybounds, yk, yksize, out, (hipStream_t)stream);
}

extern "C" int rf_fid_stats(const float* feat, int N, int D, double* mu, double* sigma, void* stream) {
    RF_CHECK(feat && mu && sigma, "rf_fid_stats: null argument");
    RF_CHECK(N >= 2, "rf_fid_stats: N=%d: a covariance needs at least 2 rows", N);
    RF_CHECK(D > 0 && D % 16 == 0, "rf_fid_stats: D=%d must be a positive multiple of 16", D);
    RF_CHECK(D <= 16384, "rf_fid_stats: D=%d is too large (16384 at the most)", D);
    RF_CHECK((((uintptr_t)mu | (uintptr_t)sigma) & 7) == 0 && ((uintptr_t)feat & 3) == 0, "rf_fid_stats: misaligned operand");
    hipStream_t st = (hipStream_t)stream;
    const int T = D / 16, npair = T * (T + 1) / 2;
    hipLaunchKernelGGL(fid_mean_kernel, dim3((unsigned)T), dim3(256), 0, st, feat, N, D, mu);
    hipLaunchKernelGGL(fid_gram_kernel, dim3((unsigned)((npair + 3) / 4)), dim3(256), 0, st, feat, N, D, (const double*)mu, sigma);
    RF_LAUNCH_CHECK("rf_fid_stats");
    return 0;
}
