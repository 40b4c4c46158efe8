// The pose metric of the evaluation (eval_tool/Pose/pose_compare.py of the reference): Hopenet head-pose angles of the swapped results
// against those of their targets.  Three kernels around the ResNet-50 body, which runs on rf_conv_gemm:
//   rf_pose_prep_u8   ImagePathDataset.__getitem__ (:91-99) on device bytes: ToTensor, tensor Resize((224, 224)), Normalize, in one pass;
//   rf_pose_head      AvgPool2d(7) + fc_yaw / fc_pitch / fc_roll (hopenet.py:66-72) + headpose_pred_to_degree (:101-108);
//   rf_pose_distance  the L2 distance of the paired degree vectors in fp64 and their sum (:320-323).
#include "common.h"

namespace rf {

constexpr int POSE_S = 224;          // Hopenet's input side
constexpr int POSE_CP = 8;           // 3 channels stored in 8: the layout of the 7x7 stem (cin_pad = 8)
constexpr int POSE_BINS = 66;
constexpr int POSE_HEADS = 3;
constexpr int POSE_C = 2048;         // channels of layer4
constexpr int POSE_PIX = 49;         // its 7 x 7 map

// ---- out[b, y, x, c] = (resize(img / 255)[y, x, c] - mean[c]) / std[c], c < 3; 0 for c = 3..7.
// torchvision's Resize on a tensor (0.12) = F.interpolate(bilinear, align_corners = False), no antialiasing at any size, in fp32 and in
// PyTorch's order: scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0), the upper tap clamped to the last pixel, the x lerps first.
// The reference resizes in its loader, on the CPU, where PyTorch's x86 build contracts three of these expressions into FMAs: the source
// coordinate fma(scale, dst + 0.5, -0.5) and both lerps fma(w0, v0, w1 * v1).  Without the first one a coordinate is off by an ulp of
// ~in (6e-5 at 300 -> 224 on noise); with all three the result equals F.interpolate's on the CPU bit for bit.  The unit builds with
// -ffp-contract=off, so the FMAs below are exactly the ones written and everything else rounds on its own.
// One thread per output pixel, pixels on lanes: a wave reads at most two source rows and writes 64 consecutive 32-byte pixels (2 KB).
__global__ __launch_bounds__(256) void pose_prep_kernel(const uint8_t* __restrict__ img, int B, int H, int W, long long simg, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // over B * 224 * 224
    constexpr int SS = POSE_S * POSE_S;
    if (i >= (long long)B * SS) return;
    const int b = (int)(i / SS);
    const int p = (int)(i - (long long)b * SS);
    const int dy = p / POSE_S, dx = p - dy * POSE_S;
    const float sy = (float)H / (float)POSE_S, sx = (float)W / (float)POSE_S;
    float fy = __builtin_fmaf(sy, (float)dy + 0.5f, -0.5f), fx = __builtin_fmaf(sx, (float)dx + 0.5f, -0.5f);
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const uint8_t* s = img + (long long)b * simg;
    const uint8_t* p00 = s + ((long long)y0 * W + x0) * 3;
    const uint8_t* p01 = s + ((long long)y0 * W + x1) * 3;
    const uint8_t* p10 = s + ((long long)y1 * W + x0) * 3;
    const uint8_t* p11 = s + ((long long)y1 * W + x1) * 3;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = (float)p00[c] / 255.0f, v01 = (float)p01[c] / 255.0f, v10 = (float)p10[c] / 255.0f, v11 = (float)p11[c] / 255.0f;
        const float top = __builtin_fmaf(hx, v00, lx * v01), bot = __builtin_fmaf(hx, v10, lx * v11);
        const float r = __builtin_fmaf(hy, top, ly * bot);
        v[c] = (r - mean[c]) / stdv[c];
    }
    float4* o = reinterpret_cast<float4*>(out + i * POSE_CP);          // out comes from the allocator (256-byte aligned) and a pixel is 32 bytes
    o[0] = make_float4(v[0], v[1], v[2], 0.f);
    o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- one block of 256 threads per image; nothing in it depends on B, so an image's degrees are the same bits in any batch.
//   1. m[c] = (sum_p x[b, p, c], p ascending) / 49: thread t owns channels t, t + 256, ...; for a fixed p the block reads 2048 consecutive floats;
//   2. logits[j] = bias[j] + sum_k m[k] W[j, k], j < 198: wave w owns rows w, w + 4, ...; lane l sums k = 4 l + 256 q + (0..3), q ascending, into one
//      partial, the 64 partials meet in wave_sum's fixed tree;
//   3. wave h < 3 owns head h (lane l: bins l and l + 64): softmax shifted by the head's maximum, p = e / sum e, degrees = (sum p * bin) * 3 - 99.
__global__ __launch_bounds__(256) void pose_head_kernel(const float* __restrict__ x, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                        float* __restrict__ deg, float* __restrict__ logits_out) {
    __shared__ float s_m[POSE_C];
    __shared__ float s_logit[POSE_HEADS * POSE_BINS];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int b = blockIdx.x;
    const float* xb = x + (long long)b * POSE_PIX * POSE_C;
    for (int c = t; c < POSE_C; c += 256) {
        float acc = 0.f;
        for (int p = 0; p < POSE_PIX; ++p) acc += xb[p * POSE_C + c];
        s_m[c] = acc / (float)POSE_PIX;
    }
    __syncthreads();
    for (int j = w; j < POSE_HEADS * POSE_BINS; j += 4) {
        const float* wr = Wt + (long long)j * POSE_C;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < POSE_C / 256; ++q) {
            const int k = q * 256 + lane * 4;
            const float4 wv = *reinterpret_cast<const float4*>(wr + k);
            acc += s_m[k] * wv.x;
            acc += s_m[k + 1] * wv.y;
            acc += s_m[k + 2] * wv.z;
            acc += s_m[k + 3] * wv.w;
        }
        acc = wave_sum(acc);
        if (lane == 0) s_logit[j] = acc + bias[j];
    }
    __syncthreads();
    if (logits_out)
        for (int j = t; j < POSE_HEADS * POSE_BINS; j += 256) logits_out[(long long)b * POSE_HEADS * POSE_BINS + j] = s_logit[j];
    if (w < POSE_HEADS) {
        const float* l = s_logit + w * POSE_BINS;
        const bool two = lane + 64 < POSE_BINS;
        const float a0 = l[lane], a1 = two ? l[lane + 64] : -INFINITY;
        const float mx = wave_max(fmaxf(a0, a1));
        const float e0 = expf(a0 - mx), e1 = two ? expf(a1 - mx) : 0.f;
        const float den = wave_sum(e0 + e1);
        const float ex = wave_sum((e0 / den) * (float)lane + (e1 / den) * (float)(lane + 64));
        if (lane == 0) deg[(long long)b * POSE_HEADS + w] = ex * 3.f - 99.f;
    }
}

// ---- dist[r] = |(double)deg_tgt[labels[r]] - (double)deg_res[r]|_2: widened before the subtraction (the reference fills a float64 array), the
// three squares summed in index order.  A label outside [0, N) reads nothing and gives NaN; the host wrapper refuses such labels before the launch.
__global__ __launch_bounds__(256) void pose_dist_kernel(const float* __restrict__ dres, int M, const float* __restrict__ dtgt, int N,
                                                        const int* __restrict__ labels, double* __restrict__ dist) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const int lab = labels[r];
    if (lab < 0 || lab >= N) {
        dist[r] = __builtin_nan("");
        return;
    }
    const double d0 = (double)dtgt[(long long)lab * 3] - (double)dres[(long long)r * 3];
    const double d1 = (double)dtgt[(long long)lab * 3 + 1] - (double)dres[(long long)r * 3 + 1];
    const double d2 = (double)dtgt[(long long)lab * 3 + 2] - (double)dres[(long long)r * 3 + 2];
    dist[r] = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

// totals[0..1] = (sum of dist, M): one block, a fixed summation order (row-strided partial sums per thread, then a tree over the block), so
// the sum is the same bits on every run.
__global__ __launch_bounds__(256) void pose_totals_kernel(const double* __restrict__ dist, int M, double* __restrict__ totals) {
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

extern "C" int rf_pose_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, float* out, void* stream) {
    RF_CHECK(images_u8 && out, "rf_pose_prep_u8: null argument");
    RF_CHECK(B > 0 && H > 0 && W > 0, "rf_pose_prep_u8: bad sizes (B=%d image %dx%d)", B, W, H);
    RF_CHECK(image_stride >= (int64_t)H * W * 3, "rf_pose_prep_u8: image stride smaller than one image");
    RF_CHECK(((uintptr_t)out & 15) == 0, "rf_pose_prep_u8: out must be 16-byte aligned");
    const long long n = (long long)B * POSE_S * POSE_S;
    RF_CHECK((n + 255) / 256 <= 0x7fffffffLL, "rf_pose_prep_u8: B=%d is too large for one launch", B);
    hipLaunchKernelGGL(pose_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, B, H, W,
                       (long long)image_stride, out);
    RF_LAUNCH_CHECK("rf_pose_prep_u8");
    return 0;
}

extern "C" int rf_pose_head(const float* feat, int B, const float* w198, const float* b198, float* degrees, float* logits, void* stream) {
    RF_CHECK(feat && w198 && b198 && degrees, "rf_pose_head: null argument");
    RF_CHECK(B > 0, "rf_pose_head: bad batch %d", B);
    RF_CHECK(((uintptr_t)w198 & 15) == 0, "rf_pose_head: the weights must be 16-byte aligned");
    hipLaunchKernelGGL(pose_head_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, feat, w198, b198, degrees, logits);
    RF_LAUNCH_CHECK("rf_pose_head");
    return 0;
}

extern "C" int rf_pose_distance(const float* deg_res, int M, const float* deg_tgt, int N, const int* labels, double* dist, double* totals, void* stream) {
    RF_CHECK(deg_res && deg_tgt && labels && dist && totals, "rf_pose_distance: null argument");
    RF_CHECK(M > 0 && N > 0, "rf_pose_distance: bad sizes (M=%d N=%d)", M, N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_dist_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, deg_res, M, deg_tgt, N, labels, dist);
    hipLaunchKernelGGL(pose_totals_kernel, dim3(1), dim3(256), 0, st, (const double*)dist, M, totals);
    RF_LAUNCH_CHECK("rf_pose_distance");
    return 0;
}
