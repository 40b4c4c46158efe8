// crop_image's enable_padding branch (src/utils/alignmengt.py:129-140 of the reference; the FFHQ recipe): the crop window of a face that
// hangs over the frame's edge is reflect-padded (np.pad), blurred towards the border (scipy.ndimage.gaussian_filter), filled towards the
// channel medians (np.median) and quantised, byte for byte; rf_align_quad_u8 (align.hip) then transforms the padded image instead of the
// window.  With w x h the padded size, mask = max(mx[x], my[y]) and r the blur's radius, per frame:
//   img  = f32(u8 window, read through numpy's reflect fold)                                  (never materialised)
//   v    = f32(sum over rows of img, fp64)        vertical pass, scipy's reflect fold           pad_vblur_kernel
//   g    = f32(sum over columns of v, fp64)       horizontal pass
//   img1 = f32(f64(img) + f64(f32(g - img)) clip(3 mask + 1, 0, 1))                             pad_hblur_kernel
//   med  = the exact median of img1 per channel: 4-pass radix select over order-preserving keys pad_hist_kernel, pad_pick_kernel
//   out  = u8(clip(rint(f32(f64(img1) + f64(f32(med - img1)) clip(mask, 0, 1))), 0, 255))       pad_fill_kernel
// A pass is scipy's symmetric correlate1d: acc = x[i] w[r]; for j = -r .. -1: acc += (x[i + j] + x[i - j]) w[j + r].  The unit builds with
// -ffp-contract=off: only fp64 multiplies and adds, none of them contracted.  Where clip(3 mask + 1) is 0 (the window's interior) img1 is
// img exactly and neither pass runs.  The host (reface_amd.align.pad_tables) makes every index map, weight and clip profile: no fold and no
// division here.  One sequence of launches serves a batch: grid.y is the frame, and a 16-word descriptor per frame says where its tables are.
#include "common.h"

namespace rf {

enum { PD_OX, PD_OY, PD_W0, PD_H0, PD_W, PD_H, PD_R, PD_EXTROW, PD_COLMAP, PD_EXTCOL, PD_COLNEED, PD_WGT, PD_C1X, PD_C1Y, PD_C2X, PD_C2Y, PD_WORDS };
constexpr int PAD_BLOCK = 256, PAD_HIST_PX = 8;          // threads per block; pixels per thread of the histogram passes
constexpr int PAD_SEL = 6 * 256 + 12;                    // select words per frame: hist [3 channels][2 ranks][256], then (prefix, rank) x 6

struct PadArgs {
    const uint8_t* frames;          // u8 [B, H, W, Cf], frame b at + b * fstride
    int H, W, Cf;
    long long fstride;
    const int* desc;                // int32 [B, 16]
    const int* itab;                // the packed index maps, nI words
    const double* dtab;             // the packed weights and clip profiles, nD doubles
    int nI, nD, hmax, wmax;
};

// One frame's tables, checked: a descriptor that points outside the frame, the tables or the per-frame slot makes the frame a no-op.
struct PadFrame {
    int W0, H0, w, h, r;
    const uint8_t* img;          // the window's first pixel
    const int *extrow, *colmap, *extcol, *colneed;
    const double *wgt, *c1x, *c1y, *c2x, *c2y;
    bool ok;
};

__device__ __forceinline__ PadFrame pad_frame(const PadArgs& a, int b) {
    const int* d = a.desc + (long long)b * PD_WORDS;
    PadFrame f;
    const int ox = d[PD_OX], oy = d[PD_OY];
    f.W0 = d[PD_W0], f.H0 = d[PD_H0], f.w = d[PD_W], f.h = d[PD_H], f.r = d[PD_R];
    const long long r2 = 2LL * f.r, nI = a.nI, nD = a.nD;
    f.ok = ox >= 0 && oy >= 0 && f.W0 > 0 && f.H0 > 0 && f.W0 <= a.W - ox && f.H0 <= a.H - oy && f.w > 0 && f.h > 0 && f.w <= a.wmax && f.h <= a.hmax && f.r >= 0;
    f.ok = f.ok && d[PD_EXTROW] >= 0 && d[PD_EXTROW] + f.h + r2 <= nI && d[PD_COLMAP] >= 0 && d[PD_COLMAP] + (long long)f.w <= nI;
    f.ok = f.ok && d[PD_EXTCOL] >= 0 && d[PD_EXTCOL] + f.w + r2 <= nI && d[PD_COLNEED] >= 0 && d[PD_COLNEED] + (long long)f.w <= nI;
    f.ok = f.ok && d[PD_WGT] >= 0 && d[PD_WGT] + (long long)f.r + 1 <= nD && d[PD_C1X] >= 0 && d[PD_C1X] + (long long)f.w <= nD;
    f.ok = f.ok && d[PD_C1Y] >= 0 && d[PD_C1Y] + (long long)f.h <= nD && d[PD_C2X] >= 0 && d[PD_C2X] + (long long)f.w <= nD;
    f.ok = f.ok && d[PD_C2Y] >= 0 && d[PD_C2Y] + (long long)f.h <= nD;
    if (!f.ok) return f;
    f.img = a.frames + (long long)b * a.fstride + ((long long)oy * a.W + ox) * a.Cf;
    f.extrow = a.itab + d[PD_EXTROW], f.colmap = a.itab + d[PD_COLMAP], f.extcol = a.itab + d[PD_EXTCOL], f.colneed = a.itab + d[PD_COLNEED];
    f.wgt = a.dtab + d[PD_WGT], f.c1x = a.dtab + d[PD_C1X], f.c1y = a.dtab + d[PD_C1Y], f.c2x = a.dtab + d[PD_C2X], f.c2y = a.dtab + d[PD_C2Y];
    return f;
}

__device__ __forceinline__ int pad_clamp(int i, int n) { return min(max(i, 0), n - 1); }          // (a table cannot make a read leave its image)

// order-preserving key of an fp32 bit pattern (negative values included) and back
__device__ __forceinline__ uint32_t pad_key(float v) {
    const uint32_t u = as_u32(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pad_unkey(uint32_t k) { return as_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- vertical pass: thread = one padded pixel (3 channels), reading the u8 window through extrow (both folds) and colmap.  Written only
// where the horizontal pass reads: rows the mask blurs (c1y > 0) and columns a blurred column's taps land on (colneed).
__global__ void pad_vblur_kernel(PadArgs a, float* __restrict__ v) {
    const int b = blockIdx.y;
    const PadFrame f = pad_frame(a, b);
    const long long p = (long long)blockIdx.x * PAD_BLOCK + threadIdx.x;
    if (!f.ok || p >= (long long)f.w * f.h) return;
    const int y = (int)(p / f.w), x = (int)(p - (long long)y * f.w);
    if (!(f.c1y[y] > 0.0) && !f.colneed[x]) return;
    const long long pitch = (long long)a.W * a.Cf;
    const uint8_t* col = f.img + (long long)pad_clamp(f.colmap[x], f.W0) * a.Cf;
    const int* er = f.extrow + y + f.r;
    const uint8_t* p0 = col + pad_clamp(er[0], f.H0) * pitch;
    const double w0 = f.wgt[f.r];
    double acc0 = (double)p0[0] * w0, acc1 = (double)p0[1] * w0, acc2 = (double)p0[2] * w0;
    for (int j = -f.r; j < 0; ++j) {
        const uint8_t* pa = col + pad_clamp(er[j], f.H0) * pitch;
        const uint8_t* pb = col + pad_clamp(er[-j], f.H0) * pitch;
        const double wj = f.wgt[j + f.r];
        acc0 += ((double)pa[0] + (double)pb[0]) * wj;
        acc1 += ((double)pa[1] + (double)pb[1]) * wj;
        acc2 += ((double)pa[2] + (double)pb[2]) * wj;
    }
    float* o = v + ((long long)b * a.hmax * a.wmax + p) * 3;
    o[0] = (float)acc0, o[1] = (float)acc1, o[2] = (float)acc2;
}

// ---- horizontal pass over v through extcol, fused with the first mix
__global__ void pad_hblur_kernel(PadArgs a, const float* __restrict__ v, float* __restrict__ img1) {
    const int b = blockIdx.y;
    const PadFrame f = pad_frame(a, b);
    if (!f.ok) return;
    const long long n = (long long)f.w * f.h;
    const long long p = (long long)blockIdx.x * PAD_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int y = (int)(p / f.w), x = (int)(p - (long long)y * f.w);
    const uint8_t* px = f.img + pad_clamp(f.extrow[y + f.r], f.H0) * ((long long)a.W * a.Cf) + (long long)pad_clamp(f.colmap[x], f.W0) * a.Cf;
    float o[3] = {(float)px[0], (float)px[1], (float)px[2]};
    const double c1 = fmax(f.c1x[x], f.c1y[y]);
    if (c1 > 0.0) {
        const float* row = v + ((long long)b * a.hmax * a.wmax + (long long)y * f.w) * 3;
        const int* ec = f.extcol + x + f.r;
        const float* q0 = row + pad_clamp(ec[0], f.w) * 3;
        const double w0 = f.wgt[f.r];
        double acc0 = (double)q0[0] * w0, acc1 = (double)q0[1] * w0, acc2 = (double)q0[2] * w0;
        for (int j = -f.r; j < 0; ++j) {
            const float* qa = row + pad_clamp(ec[j], f.w) * 3;
            const float* qb = row + pad_clamp(ec[-j], f.w) * 3;
            const double wj = f.wgt[j + f.r];
            acc0 += ((double)qa[0] + (double)qb[0]) * wj;
            acc1 += ((double)qa[1] + (double)qb[1]) * wj;
            acc2 += ((double)qa[2] + (double)qb[2]) * wj;
        }
        const double acc[3] = {acc0, acc1, acc2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = (float)acc[c] - o[c];
            o[c] = (float)((double)o[c] + (double)d * c1);
        }
    }
    float* dst = img1 + ((long long)b * a.hmax * a.wmax + p) * 3;
    dst[0] = o[0], dst[1] = o[1], dst[2] = o[2];
}

// ---- exact median by radix select, 8 bits per pass from the top.  Per (frame, channel, rank) the select keeps (prefix, rank): the key
// bits fixed so far and the rank among the values that share them.  A pass counts the next digit of those values in LDS and adds the
// block's bins to the frame's histogram with ordinary vector atomics; pad_pick_kernel then walks the 256 bins.
__global__ void pad_rank_kernel(PadArgs a, uint32_t* __restrict__ sel) {          // one block per frame: empty bins, no prefix, the two middle ranks of w h values
    const int b = blockIdx.x;
    const PadFrame f = pad_frame(a, b);
    uint32_t* gs = sel + (long long)b * PAD_SEL;
    for (int i = threadIdx.x; i < 6 * 256; i += PAD_BLOCK) gs[i] = 0u;
    if (threadIdx.x < 6) {
        const long long n = f.ok ? (long long)f.w * f.h : 1;
        gs[6 * 256 + 2 * threadIdx.x] = 0u;
        gs[6 * 256 + 2 * threadIdx.x + 1] = (uint32_t)((threadIdx.x & 1) ? n / 2 : (n - 1) / 2);
    }
}

__global__ void pad_hist_kernel(PadArgs a, const float* __restrict__ img1, uint32_t* __restrict__ sel, int shift) {
    __shared__ uint32_t lh[6 * 256];
    const int b = blockIdx.y;
    const PadFrame f = pad_frame(a, b);
    if (!f.ok) return;
    const long long n = (long long)f.w * f.h, first = (long long)blockIdx.x * PAD_HIST_PX * PAD_BLOCK;
    if (first >= n) return;
    for (int i = threadIdx.x; i < 6 * 256; i += PAD_BLOCK) lh[i] = 0u;
    uint32_t* gs = sel + (long long)b * PAD_SEL;
    const uint32_t fixed = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    uint32_t pf[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pf[k] = gs[6 * 256 + 2 * k];
    __syncthreads();
    const float* src = img1 + (long long)b * a.hmax * a.wmax * 3;
    for (int i = 0; i < PAD_HIST_PX; ++i) {
        const long long p = first + (long long)i * PAD_BLOCK + threadIdx.x;
        if (p >= n) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t key = pad_key(src[p * 3 + c]);
            const uint32_t dig = (key >> shift) & 255u;
            if ((key & fixed) == pf[2 * c]) atomicAdd(&lh[(2 * c) * 256 + dig], 1u);
            if ((key & fixed) == pf[2 * c + 1]) atomicAdd(&lh[(2 * c + 1) * 256 + dig], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 6 * 256; i += PAD_BLOCK)
        if (lh[i]) atomicAdd(&gs[i], lh[i]);
}

// one block per (frame, channel, rank): find the bin that holds the rank, extend the prefix, and clear the bins for the next pass
__global__ void pad_pick_kernel(uint32_t* __restrict__ sel, int shift) {
    __shared__ uint32_t lh[256];
    const int b = blockIdx.x / 6, k = blockIdx.x - b * 6;
    uint32_t* gs = sel + (long long)b * PAD_SEL;
    lh[threadIdx.x] = gs[k * 256 + threadIdx.x];
    gs[k * 256 + threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* st = gs + 6 * 256 + 2 * k;
        uint32_t rank = st[1], cum = 0u;
        for (int d = 0; d < 256; ++d) {
            const uint32_t c = lh[d];
            if (rank - cum < c) {
                st[0] |= (uint32_t)d << shift;
                st[1] = rank - cum;
                break;
            }
            cum += c;
        }
    }
}

// ---- second mix towards the medians, rint (half to even), clip: the padded u8 image of frame b at out[b] with rows of wmax pixels
__global__ void pad_fill_kernel(PadArgs a, const float* __restrict__ img1, const uint32_t* __restrict__ sel, uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const PadFrame f = pad_frame(a, b);
    const long long n = (long long)f.w * f.h, p = (long long)blockIdx.x * PAD_BLOCK + threadIdx.x;
    if (!f.ok || p >= n) return;
    const int y = (int)(p / f.w), x = (int)(p - (long long)y * f.w);
    const uint32_t* st = sel + (long long)b * PAD_SEL + 6 * 256;
    const double c2 = fmax(f.c2x[x], f.c2y[y]);
    const float* src = img1 + ((long long)b * a.hmax * a.wmax + p) * 3;
    uint8_t* dst = out + (((long long)b * a.hmax + y) * a.wmax + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = pad_unkey(st[4 * c]), hi = pad_unkey(st[4 * c + 2]);
        const float med = (n & 1) ? lo : (lo + hi) * 0.5f;
        const float v = src[c], d = med - v;
        const float r = rintf((float)((double)v + (double)d * c2));
        dst[c] = (uint8_t)(int)fminf(fmaxf(r, 0.0f), 255.0f);
    }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_align_pad_u8(const void* frames_u8, int B, int H, int W, int Cf, int64_t frame_stride, const int* desc, const int* itab, int n_itab,
                               const double* dtab, int n_dtab, int hmax, int wmax, float* scratch_f32, int64_t scratch_floats, void* select_u32,
                               int64_t select_words, void* out_u8, int stages, void* stream) {
    RF_CHECK(frames_u8 && desc && itab && dtab && scratch_f32 && select_u32 && out_u8, "rf_align_pad_u8: null argument");
    RF_CHECK(B > 0 && B <= 65535 && H > 0 && W > 0 && hmax > 0 && wmax > 0 && n_itab > 0 && n_dtab > 0,
             "rf_align_pad_u8: bad sizes (B=%d H=%d W=%d hmax=%d wmax=%d tables %d / %d)", B, H, W, hmax, wmax, n_itab, n_dtab);
    RF_CHECK(Cf == 3 || Cf == 4, "rf_align_pad_u8: frame channels must be 3 or 4 (Cf=%d)", Cf);
    RF_CHECK(frame_stride >= (int64_t)H * W * Cf, "rf_align_pad_u8: frame stride %lld < H * W * Cf", (long long)frame_stride);
    const long long slot = (long long)hmax * wmax;
    RF_CHECK(slot <= (1LL << 28), "rf_align_pad_u8: a padded image of %dx%d is too large", wmax, hmax);
    RF_CHECK(scratch_floats >= 2 * (int64_t)B * slot * 3, "rf_align_pad_u8: scratch of %lld floats < 2 * B * hmax * wmax * 3", (long long)scratch_floats);
    RF_CHECK(select_words >= (int64_t)B * PAD_SEL, "rf_align_pad_u8: select scratch of %lld words < B * %d", (long long)select_words, PAD_SEL);
    RF_CHECK(out_u8 != frames_u8, "rf_align_pad_u8: the padded images cannot overwrite the frames");
    RF_CHECK(stages > 0 && stages < 16, "rf_align_pad_u8: stages is a mask of 1 (vertical blur), 2 (horizontal blur + mix), 4 (median), 8 (fill)");
    const PadArgs a = {(const uint8_t*)frames_u8, H, W, Cf, (long long)frame_stride, desc, itab, dtab, n_itab, n_dtab, hmax, wmax};
    float* v = scratch_f32;
    float* img1 = scratch_f32 + (long long)B * slot * 3;
    uint32_t* sel = (uint32_t*)select_u32;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(PAD_BLOCK), grid((unsigned)((slot + PAD_BLOCK - 1) / PAD_BLOCK), B);
    const dim3 hgrid((unsigned)((slot + PAD_BLOCK * PAD_HIST_PX - 1) / (PAD_BLOCK * PAD_HIST_PX)), B);
    if (stages & 1) hipLaunchKernelGGL(pad_vblur_kernel, grid, block, 0, st, a, v);
    if (stages & 2) hipLaunchKernelGGL(pad_hblur_kernel, grid, block, 0, st, a, (const float*)v, img1);
    if (stages & 4) {
        hipLaunchKernelGGL(pad_rank_kernel, dim3(B), block, 0, st, a, sel);
        for (int shift = 24; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(pad_hist_kernel, hgrid, block, 0, st, a, (const float*)img1, sel, shift);
            hipLaunchKernelGGL(pad_pick_kernel, dim3(B * 6), block, 0, st, sel, shift);
        }
    }
    if (stages & 8) hipLaunchKernelGGL(pad_fill_kernel, grid, block, 0, st, a, (const float*)img1, (const uint32_t*)sel, (uint8_t*)out_u8);
    RF_LAUNCH_CHECK("rf_align_pad_u8");
    return 0;
}
