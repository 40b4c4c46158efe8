// The expression metric of the evaluation (eval_tool/Expression/expression_compare_face_recon.py of the reference): the 64 expression
// coefficients of Deep3DFaceRecon's net_recon of the swapped results against those of their targets.  Three kernels around the ResNet-50
// body, which runs on rf_conv_gemm:
//   rf_expr_prep_u8   ImagePathDataset.__getitem__ (:123-136) on device bytes: PIL's resize((512, 512), BICUBIC), / 255, NHWC, in one pass;
//   rf_expr_head      AdaptiveAvgPool2d((1, 1)) + the seven 1x1 final layers (networks.py:210-376), 257 coefficients per image;
//   rf_expr_distance  the L2 distance of the paired expression coefficients [80, 144) in fp64 and their sum (:300-384).
// The vertical pass of the resize needs no intermediate in global memory at any source size: the horizontally resampled rows a tile's
// vertical windows cover pass through LDS in chunks of EP_TMP_ROWS rows (one chunk at 1024 -> 512 and at 512 -> 512).
#include "pil_u8.h"

namespace rf {

constexpr int EXPR_S = 512;          // net_recon's input side in the reference's evaluation
constexpr int EXPR_CP = 8;           // 3 channels stored in 8: the layout of the 7x7 stem (cin_pad = 8)
constexpr int EXPR_C = 2048;         // channels of layer4
constexpr int EXPR_NCOEF = 257;      // id 80 | exp 64 | tex 80 | angle 3 | gamma 27 | tx, ty 2 | tz 1

constexpr int EP_TW = 64, EP_TH = 16, EP_THREADS = 256, EP_Q = EP_TH / (EP_THREADS / EP_TW);
constexpr int EP_TMP_ROWS = 48;      // 12 KiB of horizontally resampled rows (RGBx words)

// bounds[2 i] = first input index, bounds[2 i + 1] = tap count of output index i, clipped to the table's width and to the axis: whatever the
// table holds, no tap lies outside [0, n_in)
__device__ __forceinline__ void ep_window(const int* __restrict__ bounds, int i, int ksize, int n_in, int& lo, int& n) {
    lo = min(max(bounds[2 * i], 0), n_in - 1);
    n = max(min(bounds[2 * i + 1], min(ksize, n_in - lo)), 0);
}

// ---- out[b, y, x, c] = resize(img)[y, x, c] / 255, c < 3; 0 for c = 3..7.  PIL resizes in two integer passes with a u8 image between them
// (Resample.c: ImagingResampleHorizontal_8bpc, then Vertical_8bpc, each clip8(((1 << 21) + sum k p) >> 22)); the rounding between the
// passes is part of the result, so both are kept.  With the identity tables of a 512 x 512 source (one tap of 1 << 22) both passes return
// the byte.  float32(b / 255.0) of the reference's float64 division equals float32(b) / 255.0f for every byte.
// A block owns EP_TH x EP_TW output pixels (512 is a multiple of both).  Per chunk of the input rows its vertical windows cover:
//   1. the horizontal pass of those rows for the tile's 64 columns: global bytes -> one RGBx word per (row, column) in LDS,
//   2. every thread adds the chunk's rows into the vertical sums of its 4 output pixels (column tid % 64, rows tid / 64 + 4 q).
// Lanes of a wave hold consecutive pixels of one row: a wave stores 2 KB of consecutive NHWC pixels.
__global__ void __launch_bounds__(EP_THREADS)
expr_prep_kernel(const uint8_t* __restrict__ images, int H, int W, long long simg, const int* __restrict__ xb, const int* __restrict__ xk, int xks,
                 const int* __restrict__ yb, const int* __restrict__ yk, int yks, float* __restrict__ out) {
    __shared__ uint32_t tmp[EP_TMP_ROWS * EP_TW];
    constexpr int TX = EXPR_S / EP_TW, TY = EXPR_S / EP_TH;
    const int tid = threadIdx.x, tx = tid % EP_TW, ty = tid / EP_TW;
    const int bx = blockIdx.x % TX, by = (blockIdx.x / TX) % TY, b = blockIdx.x / (TX * TY);
    const int x = bx * EP_TW + tx, y0 = by * EP_TH;
    const uint8_t* img = images + (long long)b * simg;
    int xlo, xn;
    ep_window(xb, x, xks, W, xlo, xn);
    const int* kx = xk + (long long)x * xks;
    int rbeg = 0x7fffffff, rend = 0;          // the input rows of the tile's 16 vertical windows (the same in every thread)
    for (int i = 0; i < EP_TH; ++i) {
        int lo, n;
        ep_window(yb, y0 + i, yks, H, lo, n);
        if (n > 0) {
            rbeg = min(rbeg, lo);
            rend = max(rend, lo + n);
        }
    }
    int ylo[EP_Q], yn[EP_Q], acc[EP_Q][3];
#pragma unroll
    for (int q = 0; q < EP_Q; ++q) {
        ep_window(yb, y0 + ty + (EP_THREADS / EP_TW) * q, yks, H, ylo[q], yn[q]);
        acc[q][0] = acc[q][1] = acc[q][2] = 1 << 21;
    }
    for (int r0 = rbeg; r0 < rend; r0 += EP_TMP_ROWS) {
        const int rows = min(EP_TMP_ROWS, rend - r0);
        for (int it = tid; it < rows * EP_TW; it += EP_THREADS) {          // (it % EP_TW == tx: a thread keeps its column)
            const int rl = it / EP_TW;
            const uint8_t* in = img + ((long long)(r0 + rl) * W + xlo) * 3;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int i = 0; i < xn; ++i) {
                const int k = kx[i];
                a0 += k * (int)in[3 * i];
                a1 += k * (int)in[3 * i + 1];
                a2 += k * (int)in[3 * i + 2];
            }
            tmp[rl * EP_TW + tx] = (uint32_t)pil_clip8(a0) | ((uint32_t)pil_clip8(a1) << 8) | ((uint32_t)pil_clip8(a2) << 16);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < EP_Q; ++q) {
            const int* ky = yk + (long long)(y0 + ty + (EP_THREADS / EP_TW) * q) * yks;
            const int rb = max(ylo[q], r0), re = min(ylo[q] + yn[q], r0 + rows);
            for (int r = rb; r < re; ++r) {
                const int k = ky[r - ylo[q]];
                const uint32_t p = tmp[(r - r0) * EP_TW + tx];
                acc[q][0] += k * (int)(p & 255u);
                acc[q][1] += k * (int)((p >> 8) & 255u);
                acc[q][2] += k * (int)((p >> 16) & 255u);
            }
        }
        if (r0 + EP_TMP_ROWS < rend) __syncthreads();          // the next chunk overwrites tmp
    }
#pragma unroll
    for (int q = 0; q < EP_Q; ++q) {
        const int y = y0 + ty + (EP_THREADS / EP_TW) * q;
        float4* o = reinterpret_cast<float4*>(out + (((long long)b * EXPR_S + y) * EXPR_S + x) * EXPR_CP);          // 32-byte pixels of a 16-byte aligned buffer
        o[0] = make_float4((float)pil_clip8(acc[q][0]) / 255.0f, (float)pil_clip8(acc[q][1]) / 255.0f, (float)pil_clip8(acc[q][2]) / 255.0f, 0.f);
        o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// ---- one block of 256 threads per image; nothing in it depends on B, so an image's coefficients are the same bits in any batch.
//   1. m[c] = (sum_p x[b, p, c], p ascending) / P: thread t owns channels t, t + 256, ...; for a fixed p the block reads 2048 consecutive floats;
//   2. coef[j] = bias[j] + sum_k m[k] W[j, k], j < 257: wave w owns rows w, w + 4, ...; lane l sums k = 4 l + 256 q + (0..3), q ascending, into one
//      partial, the 64 partials meet in wave_sum's fixed tree.
__global__ __launch_bounds__(256) void expr_head_kernel(const float* __restrict__ x, int P, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                        float* __restrict__ coef) {
    __shared__ float s_m[EXPR_C];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int b = blockIdx.x;
    const float* xb = x + (long long)b * P * EXPR_C;
    for (int c = t; c < EXPR_C; c += 256) {
        float acc = 0.f;
        for (int p = 0; p < P; ++p) acc += xb[(long long)p * EXPR_C + c];
        s_m[c] = acc / (float)P;
    }
    __syncthreads();
    for (int j = w; j < EXPR_NCOEF; j += 4) {
        const float* wr = Wt + (long long)j * EXPR_C;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < EXPR_C / 256; ++q) {
            const int k = q * 256 + lane * 4;
            const float4 wv = *reinterpret_cast<const float4*>(wr + k);
            acc += s_m[k] * wv.x;
            acc += s_m[k + 1] * wv.y;
            acc += s_m[k + 2] * wv.z;
            acc += s_m[k + 3] * wv.w;
        }
        acc = wave_sum(acc);
        if (lane == 0) coef[(long long)b * EXPR_NCOEF + j] = acc + bias[j];
    }
}

// ---- dist[r] = |(double)tgt[labels[r], col0 .. col0 + ncols) - (double)res[r, col0 .. col0 + ncols)|_2: widened before the subtraction (the
// reference fills a float64 array), the squares summed in column order.  A label outside [0, N) reads nothing and gives NaN; the host wrapper
// refuses such labels before the launch.
__global__ __launch_bounds__(256) void expr_dist_kernel(const float* __restrict__ res, int M, const float* __restrict__ tgt, int N, int ld, int col0,
                                                        int ncols, const int* __restrict__ labels, double* __restrict__ dist) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const int lab = labels[r];
    if (lab < 0 || lab >= N) {
        dist[r] = __builtin_nan("");
        return;
    }
    const float* a = tgt + (long long)lab * ld + col0;
    const float* c = res + (long long)r * ld + col0;
    double s = 0.0;
    for (int k = 0; k < ncols; ++k) {
        const double d = (double)a[k] - (double)c[k];
        s += d * d;
    }
    dist[r] = sqrt(s);
}

// totals[0..1] = (sum of dist, M): one block, pose_totals_kernel's order (row-strided partial sums per thread, then a tree over the block), so
// the sum is the same bits on every run.
__global__ __launch_bounds__(256) void expr_totals_kernel(const double* __restrict__ dist, int M, double* __restrict__ totals) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int r = t; r < M; r += 256) s += dist[r];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        totals[0] = red[0];
        totals[1] = (double)M;
    }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_expr_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, const int* xbounds, const int* xk, int xksize,
                               const int* ybounds, const int* yk, int yksize, float* out, void* stream) {
    RF_CHECK(images_u8 && xbounds && xk && ybounds && yk && out, "rf_expr_prep_u8: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0 && xksize > 0 && yksize > 0, "rf_expr_prep_u8: bad sizes (B=%d image %dx%d, ksize %d / %d)", B, W, H, xksize, yksize);
    RF_CHECK(image_stride >= (int64_t)H * W * 3, "rf_expr_prep_u8: image stride smaller than one image");
    RF_CHECK(((uintptr_t)out & 15) == 0, "rf_expr_prep_u8: out must be 16-byte aligned");
    const long long blocks = (long long)B * (EXPR_S / EP_TW) * (EXPR_S / EP_TH);
    RF_CHECK(blocks < (1LL << 31), "rf_expr_prep_u8: B=%d is too large for one launch", B);
    hipLaunchKernelGGL(expr_prep_kernel, dim3((unsigned)blocks), dim3(EP_THREADS), 0, (hipStream_t)stream, (const uint8_t*)images_u8, H, W,
                       (long long)image_stride, xbounds, xk, xksize, ybounds, yk, yksize, out);
    RF_LAUNCH_CHECK("rf_expr_prep_u8");
    return 0;
}

extern "C" int rf_expr_head(const float* feat, int B, int P, const float* w257, const float* b257, float* coeffs, void* stream) {
    RF_CHECK(feat && w257 && b257 && coeffs, "rf_expr_head: null argument");
    RF_CHECK(B > 0, "rf_expr_head: bad batch %d", B);
    RF_CHECK(P > 0, "rf_expr_head: bad pixel count %d", P);
    RF_CHECK(((uintptr_t)w257 & 15) == 0, "rf_expr_head: the weights must be 16-byte aligned");
    hipLaunchKernelGGL(expr_head_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, feat, P, w257, b257, coeffs);
    RF_LAUNCH_CHECK("rf_expr_head");
    return 0;
}

extern "C" int rf_expr_distance(const float* coef_res, int M, const float* coef_tgt, int N, int ld, int col0, int ncols, const int* labels, double* dist,
                                double* totals, void* stream) {
    RF_CHECK(coef_res && coef_tgt && labels && dist && totals, "rf_expr_distance: null argument");
    RF_CHECK(M > 0 && N > 0, "rf_expr_distance: bad sizes (M=%d N=%d)", M, N);
    RF_CHECK(col0 >= 0 && ncols > 0 && col0 + ncols <= ld, "rf_expr_distance: columns [%d, %d) outside rows of %d", col0, col0 + ncols, ld);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(expr_dist_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, coef_res, M, coef_tgt, N, ld, col0, ncols, labels, dist);
    hipLaunchKernelGGL(expr_totals_kernel, dim3(1), dim3(256), 0, st, (const double*)dist, M, totals);
    RF_LAUNCH_CHECK("rf_expr_distance");
    return 0;
}
