// Side kernels of the BiSeNet face parser (pretrained/face_parsing/{model,resnet,face_parsing_demo}.py of the reference): the input
// preparation (ToTensor + BicubicDownSample(2) + clamp + ImageNet normalisation), the ResNet-18 max-pool, the BasicBlock tail, the ARM32
// context add and the output head (bilinear align_corners=True upsample + argmax + label LUT).  Every convolution of the network runs on
// rf_conv_gemm; these are the HBM-bound passes around it.  fp32 storage throughout, as the reference runs.
#include "common.h"

namespace rf {

// BicubicDownSample(factor=2) taps (face_parsing_demo.py:129-148): cubic kernel a = -0.5 at (i - 3.5) / 2, i = 0..7, divided by their sum (2).
// The values are dyadic, so the normalised taps are exact in fp32.
__constant__ float k_bicubic2[8] = {-0.01171875f, -0.03515625f, 0.11328125f, 0.43359375f, 0.43359375f, 0.11328125f, -0.03515625f, -0.01171875f};

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// One thread per (b, oy, ox): 8 x 8 window of u8 pixels, vertical taps first (stride 2 on rows, reflect pad 3 | 3), then horizontal taps
// (stride 2 on columns, reflect pad 3 | 3) on the unrounded vertical results, as the reference's two grouped conv2d passes.  Then
// clamp(0, 1) and (x - mean) / std.  Out: NHWC fp32 [B, H/2, W/2, 8], channels 3..7 zero.
__global__ void parse_prep_kernel(const uint8_t* __restrict__ x, int B, int H, int W, float* __restrict__ out) {
    const int Ho = H / 2, Wo = W / 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * Ho * Wo) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho), b = (int)(i / ((long long)Wo * Ho));
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    int rows[8], cols[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        rows[t] = reflect_idx(2 * oy - 3 + t, H);
        cols[t] = reflect_idx(2 * ox - 3 + t, W);
    }
    const uint8_t* img = x + (long long)b * H * W * 3;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint8_t* p = img + ((long long)rows[t] * W + cols[j]) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] += k_bicubic2[t] * ((float)p[c] / 255.f);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += k_bicubic2[j] * v[c];
    }
    float* o = out + i * 8;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (fminf(fmaxf(acc[c], 0.f), 1.f) - mean[c]) / stdv[c];
#pragma unroll
    for (int c = 3; c < 8; ++c) o[c] = 0.f;
}

// MaxPool2d(3, stride 2, padding 1) on NHWC fp32 (resnet.py:58); padded positions are -inf, so every window holds >= 1 real pixel.
__global__ void maxpool3x3s2_kernel(const float* __restrict__ x, int B, int H, int W, int Cc, int Ho, int Wo, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * Ho * Wo * Cc) return;
    const int c = (int)(i % Cc);
    const long long pix = i / Cc;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long long)Wo * Ho));
    float m = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
        if (iy < 0 || iy >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox - 1 + dx;
            if (ix < 0 || ix >= W) continue;
            m = fmaxf(m, x[(((long long)b * H + iy) * W + ix) * Cc + c]);
        }
    }
    out[i] = m;
}

// BasicBlock tail (resnet.py:41-47): out = relu(shortcut + residual)
__global__ void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ r, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fmaxf(a[i] + r[i], 0.f);
}

// ARM32 + global context (model.py:99,121-122): out[b, p, c] = x[b, p, c] * s[b, c] + v[b, c]
__global__ void scale_add_vec_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ v, float* __restrict__ out,
                                     int B, int HW, int Cc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * HW * Cc) return;
    const int c = (int)(i % Cc);
    const long long bc = (i / ((long long)HW * Cc)) * Cc + c;
    out[i] = x[i] * s[bc] + v[bc];
}

// Output head (model.py:252 + face_parsing_demo.py:293, 309-311): F.interpolate(bilinear, align_corners=True) of the logits to H x W,
// argmax over channels (first maximum wins) and a 256-entry label LUT, per output pixel -- the full-resolution logits never exist.
// Source coordinate and weights as PyTorch's CPU kernel forms them: scale = (in - 1) / (out - 1) in fp32, src = scale * dst, i0 = floor,
// i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; value = (v00 w0 + v01 w1) h0 + (v10 w0 + v11 w1) h1.
__global__ void parse_head_kernel(const float* __restrict__ lg, int B, int h, int w, int Cc, int ldl, int H, int W, const uint8_t* __restrict__ lut,
                                  uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * H * W) return;
    const int ox = (int)(i % W), oy = (int)((i / W) % H), b = (int)(i / ((long long)W * H));
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float fy = sy * (float)oy, fx = sx * (float)ox;
    const int y0 = min((int)floorf(fy), h - 1), x0 = min((int)floorf(fx), w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float h1 = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), w1 = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
    const float h0 = 1.f - h1, w0 = 1.f - w1;
    const float* base = lg + (long long)b * h * w * ldl;
    const float* p00 = base + ((long long)y0 * w + x0) * ldl;
    const float* p01 = base + ((long long)y0 * w + x1) * ldl;
    const float* p10 = base + ((long long)y1 * w + x0) * ldl;
    const float* p11 = base + ((long long)y1 * w + x1) * ldl;
    float best = 0.f;
    int arg = 0;
    for (int c = 0; c < Cc; ++c) {
        const float t0 = p00[c] * w0 + p01[c] * w1;
        const float t1 = p10[c] * w0 + p11[c] * w1;
        const float v = t0 * h0 + t1 * h1;
        if (c == 0 || v > best) { best = v; arg = c; }
    }
    out[i] = lut[arg];
}

static inline dim3 grid1(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace rf

using namespace rf;

extern "C" int rf_parse_prep(const void* x_u8, int B, int H, int W, float* out, void* stream) {
    RF_CHECK(x_u8 && out && B > 0 && H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "rf_parse_prep: bad arguments (B=%d H=%d W=%d; even H, W >= 4)", B, H, W);
    const long long n = (long long)B * (H / 2) * (W / 2);
    hipLaunchKernelGGL(parse_prep_kernel, grid1(n), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)x_u8, B, H, W, out);
    RF_LAUNCH_CHECK("rf_parse_prep");
    return 0;
}

extern "C" int rf_maxpool3x3s2(const float* x, int B, int H, int W, int C, float* out, void* stream) {
    RF_CHECK(x && out && B > 0 && H > 0 && W > 0 && C > 0, "rf_maxpool3x3s2: bad arguments");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long n = (long long)B * Ho * Wo * C;
    hipLaunchKernelGGL(maxpool3x3s2_kernel, grid1(n), dim3(256), 0, (hipStream_t)stream, x, B, H, W, C, Ho, Wo, out);
    RF_LAUNCH_CHECK("rf_maxpool3x3s2");
    return 0;
}

extern "C" int rf_add_relu(const float* a, const float* r, float* out, int64_t n, void* stream) {
    RF_CHECK(a && r && out && n > 0, "rf_add_relu: bad arguments");
    hipLaunchKernelGGL(add_relu_kernel, grid1(n), dim3(256), 0, (hipStream_t)stream, a, r, out, (long long)n);
    RF_LAUNCH_CHECK("rf_add_relu");
    return 0;
}

extern "C" int rf_scale_add_vec(const float* x, const float* s, const float* v, float* out, int B, int HW, int C, void* stream) {
    RF_CHECK(x && s && v && out && B > 0 && HW > 0 && C > 0, "rf_scale_add_vec: bad arguments");
    hipLaunchKernelGGL(scale_add_vec_kernel, grid1((long long)B * HW * C), dim3(256), 0, (hipStream_t)stream, x, s, v, out, B, HW, C);
    RF_LAUNCH_CHECK("rf_scale_add_vec");
    return 0;
}

extern "C" int rf_parse_head(const float* logits, int B, int h, int w, int C, int ldl, int H, int W, const void* lut256_u8, void* out_u8,
                             void* stream) {
    RF_CHECK(logits && lut256_u8 && out_u8 && B > 0 && h > 0 && w > 0 && C > 0 && C <= 256 && ldl >= C && H > 0 && W > 0,
             "rf_parse_head: bad arguments");
    const long long n = (long long)B * H * W;
    hipLaunchKernelGGL(parse_head_kernel, grid1(n), dim3(256), 0, (hipStream_t)stream, logits, B, h, w, C, ldl, H, W, (const uint8_t*)lut256_u8,
                       (uint8_t*)out_u8);
    RF_LAUNCH_CHECK("rf_parse_head");
    return 0;
}
