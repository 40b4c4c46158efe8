// The identity metric of the evaluation (eval_tool/ID_retrieval/ID_retrieval.py of the reference): ArcFace ID retrieval of swapped results
// against their sources.  Two kernels around the ArcFace engine:
//   rf_id_prep_u8   MaskedImagePathDataset.__getitem__ (:189-228) on device bytes, one pass, no resized image or mask in memory;
//   rf_id_retrieve  calculate_id_given_paths' scoring (:362-390) without the M x N score matrix.
#include "cv_u8.h"

namespace rf {

// ---- out[b, c, y, x] = ((resize_u8(img)[y, x, c] / 255 - 0.5) / 0.5) * resize_f32(mask)[y, x]:
//   image  A.Resize(S, S) = cv2 INTER_LINEAR on uint8 (cv_u8.h), ToTensor (/ 255), Normalize(0.5, 0.5);
//   mask   isin(label, preserve) as 0 / 1 (the reference: 0 / 255 -> ToTensor), torchvision's tensor Resize = bilinear, align_corners = False, no
//          antialiasing, in fp32 and in PyTorch's order: scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0), the x lerps first.
// One thread per output pixel (3 channels).  The unit builds with -ffp-contract=off: every product and sum below rounds on its own.
__global__ void id_prep_kernel(const uint8_t* __restrict__ img, int B, int H, int W, long long simg, const uint8_t* __restrict__ lab, int Hl, int Wl,
                               long long slab, const uint8_t* __restrict__ lut, int S, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // over B * S * S
    const long long SS = (long long)S * S;
    if (i >= (long long)B * SS) return;
    const int b = (int)(i / SS);
    const int p = (int)(i - (long long)b * SS);
    const int dy = p / S, dx = p - dy * S;
    uint8_t px[3];
    cv_resize_linear_px(img + (long long)b * simg, H, W, 3, S, S, dy, dx, px);
    const float sy = (float)Hl / (float)S, sx = (float)Wl / (float)S;
    float fy = sy * ((float)dy + 0.5f) - 0.5f, fx = sx * ((float)dx + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = min((int)fy, Hl - 1), x0 = min((int)fx, Wl - 1);
    const int y1 = y0 + (y0 < Hl - 1 ? 1 : 0), x1 = x0 + (x0 < Wl - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const uint8_t* l = lab + (long long)b * slab;
    const float v00 = lut[l[(long long)y0 * Wl + x0]] ? 1.f : 0.f, v01 = lut[l[(long long)y0 * Wl + x1]] ? 1.f : 0.f;
    const float v10 = lut[l[(long long)y1 * Wl + x0]] ? 1.f : 0.f, v11 = lut[l[(long long)y1 * Wl + x1]] ? 1.f : 0.f;
    const float m = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((long long)b * 3 + c) * SS + p] = (((float)px[c] / 255.0f - 0.5f) / 0.5f) * m;
}

// ---- retrieval.  Order of the sources for one result row: score descending, ties to the LOWER index.
__device__ __forceinline__ bool id_better(double s, int j, double s2, int j2) { return s > s2 || (s == s2 && j < j2); }

constexpr int ID_ROWS = 4;          // result rows per block: one per wave
constexpr int ID_TN = 64;           // sources per tile: one per lane
constexpr int ID_KC = 64;           // K chunk of a staged source tile
constexpr int ID_DMAX = 1024;

// Block = 4 waves, wave w owns result row r = 4 blockIdx.x + w.  All scores are chains acc = fma((double)a[k], (double)b[k], acc), k ascending
// (fp32 features widened, fp64 products and sums: np.dot of the reference's float64 arrays up to the summation order).
//   1. the block stages its 4 result rows and their 4 label rows F_src[label] in LDS; per wave, the norms and the renormalised cosine
//      sum_k (a_k / |a|) (b_k / |b|) by lane-strided partial sums, and the label's score s_lab by lane 0 with the chain above;
//   2. source tiles of 64 (lane l of every wave scores source j0 + l against its wave's row, K in chunks of 64 through LDS); each lane
//      keeps the five best of the sources it has seen, and counts those that beat the label (id_better against (s_lab, label));
//   3. five rounds of a wave-wide arg-best over the lanes' list heads give top5[r][0..4] (fewer than five sources: -1 fills the rest);
//      rank[r] = the wave's count = the 0-based position of the label in the order above.
// A label outside [0, N) has rank N (no hit) and similarity 0; the host wrapper refuses such labels before the launch.
__global__ __launch_bounds__(256) void id_retrieve_kernel(const float* __restrict__ fres, int M, const float* __restrict__ fsrc, int N, int D,
                                                         const int* __restrict__ labels, int* __restrict__ top5, int* __restrict__ rank,
                                                         double* __restrict__ sim) {
    __shared__ float s_res[ID_ROWS][ID_DMAX];
    __shared__ float s_lab[ID_ROWS][ID_DMAX];
    __shared__ float s_src[ID_TN][ID_KC + 1];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int r = blockIdx.x * ID_ROWS + w;
    const bool rvalid = r < M;
    const int lab = rvalid ? labels[r] : -1;
    const bool lvalid = lab >= 0 && lab < N;
    for (int k = lane; k < D; k += 64) {
        s_res[w][k] = rvalid ? fres[(long long)r * D + k] : 0.f;
        s_lab[w][k] = lvalid ? fsrc[(long long)lab * D + k] : 0.f;
    }
    __syncthreads();
    double na = 0.0, nb = 0.0;
    for (int k = lane; k < D; k += 64) {
        const double a = (double)s_res[w][k], b = (double)s_lab[w][k];
        na = fma(a, a, na);
        nb = fma(b, b, nb);
    }
    na = sqrt(wave_sum_d(na));
    nb = sqrt(wave_sum_d(nb));
    double cs = 0.0;
    for (int k = lane; k < D; k += 64) cs = fma((double)s_res[w][k] / na, (double)s_lab[w][k] / nb, cs);
    cs = wave_sum_d(cs);
    double slab = 0.0;
    if (lane == 0)
        for (int k = 0; k < D; ++k) slab = fma((double)s_res[w][k], (double)s_lab[w][k], slab);
    slab = __shfl(slab, 0, 64);

    const double NEG = -__builtin_huge_val();
    double ls0 = NEG, ls1 = NEG, ls2 = NEG, ls3 = NEG, ls4 = NEG;
    int li0 = 0x7fffffff, li1 = 0x7fffffff, li2 = 0x7fffffff, li3 = 0x7fffffff, li4 = 0x7fffffff;
    int beat = 0;
    for (int j0 = 0; j0 < N; j0 += ID_TN) {
        double acc = 0.0;
        for (int kc = 0; kc < D; kc += ID_KC) {
            __syncthreads();          // the previous chunk has been read
#pragma unroll
            for (int q = 0; q < ID_TN * ID_KC / 256; ++q) {
                const int e = q * 256 + t, row = e / ID_KC, col = e - row * ID_KC;
                s_src[row][col] = (j0 + row < N) ? fsrc[(long long)(j0 + row) * D + kc + col] : 0.f;
            }
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < ID_KC; ++k) acc = fma((double)s_res[w][kc + k], (double)s_src[lane][k], acc);
        }
        const int j = j0 + lane;
        if (j < N) {
            if (lvalid && j != lab && id_better(acc, j, slab, lab)) ++beat;
            if (id_better(acc, j, ls4, li4)) {          // insert into the lane's sorted five
                ls4 = acc, li4 = j;
                if (id_better(ls4, li4, ls3, li3)) { const double a = ls3; const int b = li3; ls3 = ls4, li3 = li4, ls4 = a, li4 = b; }
                if (id_better(ls3, li3, ls2, li2)) { const double a = ls2; const int b = li2; ls2 = ls3, li2 = li3, ls3 = a, li3 = b; }
                if (id_better(ls2, li2, ls1, li1)) { const double a = ls1; const int b = li1; ls1 = ls2, li1 = li2, ls2 = a, li2 = b; }
                if (id_better(ls1, li1, ls0, li0)) { const double a = ls0; const int b = li0; ls0 = ls1, li0 = li1, ls1 = a, li1 = b; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) beat += __shfl_xor(beat, o, 64);
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        double bs = ls0;
        int bi = li0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (id_better(os, oi, bs, bi)) bs = os, bi = oi;
        }
        if (bi != 0x7fffffff && bi == li0) {          // the winning lane pops its head
            ls0 = ls1, li0 = li1, ls1 = ls2, li1 = li2, ls2 = ls3, li2 = li3, ls3 = ls4, li3 = li4, ls4 = NEG, li4 = 0x7fffffff;
        }
        if (lane == 0 && rvalid) top5[(long long)r * 5 + q] = bi == 0x7fffffff ? -1 : bi;
    }
    if (lane == 0 && rvalid) {
        rank[r] = lvalid ? beat : N;
        sim[r] = lvalid ? cs : 0.0;
    }
}

// totals[0..3] = (rows with rank 0, rows with rank < 5, sum of the similarities, M): one block, a fixed summation order (row-strided partial
// sums per thread, then a tree over the block), so the sum is the same on every run.
__global__ __launch_bounds__(256) void id_totals_kernel(const int* __restrict__ rank, const double* __restrict__ sim, int M, double* __restrict__ totals) {
    __shared__ double red[3][256];
    const int t = threadIdx.x;
    double h1 = 0.0, h5 = 0.0, s = 0.0;
    for (int r = t; r < M; r += 256) {
        h1 += rank[r] == 0 ? 1.0 : 0.0;
        h5 += rank[r] < 5 ? 1.0 : 0.0;
        s += sim[r];
    }
    red[0][t] = h1, red[1][t] = h5, red[2][t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
            red[2][t] += red[2][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        totals[0] = red[0][0], totals[1] = red[1][0], totals[2] = red[2][0], totals[3] = (double)M;
    }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_id_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, const void* labels_u8, int Hl, int Wl,
                             int64_t label_stride, const void* lut256_u8, float* out, int S, void* stream) {
    RF_CHECK(images_u8 && labels_u8 && lut256_u8 && out, "rf_id_prep_u8: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0 && Hl > 0 && Wl > 0 && S > 0 && S <= 4096, "rf_id_prep_u8: bad sizes (B=%d image %dx%d labels %dx%d S=%d)", B, W, H, Wl, Hl, S);
    RF_CHECK(image_stride >= (int64_t)H * W * 3 && label_stride >= (int64_t)Hl * Wl, "rf_id_prep_u8: image / label stride smaller than one image");
    const long long n = (long long)B * S * S;
    hipLaunchKernelGGL(id_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, B, H, W,
                       (long long)image_stride, (const uint8_t*)labels_u8, Hl, Wl, (long long)label_stride, (const uint8_t*)lut256_u8, S, out);
    RF_LAUNCH_CHECK("rf_id_prep_u8");
    return 0;
}

extern "C" int rf_id_retrieve(const float* f_res, int M, const float* f_src, int N, int D, const int* labels, int* top5, int* rank, double* sim,
                              double* totals, void* stream) {
    RF_CHECK(f_res && f_src && labels && top5 && rank && sim && totals, "rf_id_retrieve: null argument");
    RF_CHECK(M > 0 && N > 0 && D > 0 && D % ID_KC == 0 && D <= ID_DMAX, "rf_id_retrieve: bad sizes (M=%d N=%d D=%d; D a multiple of %d, at most %d)", M, N, D,
             ID_KC, ID_DMAX);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(id_retrieve_kernel, dim3((unsigned)((M + ID_ROWS - 1) / ID_ROWS)), dim3(256), 0, st, f_res, M, f_src, N, D, labels, top5, rank, sim);
    hipLaunchKernelGGL(id_totals_kernel, dim3(1), dim3(256), 0, st, (const int*)rank, (const double*)sim, M, totals);
    RF_LAUNCH_CHECK("rf_id_retrieve");
    return 0;
}
