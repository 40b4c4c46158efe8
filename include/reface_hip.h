/*
 * reface_hip.h -- C-ABI of the MI355X (gfx950) REFace inference kernels.
 *
 * The reference (Sanoojan/REFace) is 100 % Python: its "operator API" for the hot path is the
 * set of ATen calls issued by ldm/modules/diffusionmodules/openaimodel.py, ldm/modules/attention.py,
 * ldm/modules/diffusionmodules/model.py and ldm/models/diffusion/ddim.py.
 * Each entry point below replaces one family of those calls; the reference line it stands in for
 * is cited next to it.  The Python host layer (the modules of reface_amd) binds these with ctypes; the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers + sizes; no torch types.  All pointers are DEVICE pointers, 16-byte aligned.
 *   - the caller owns every buffer; kernels never allocate.
 *   - `stream` is a hipStream_t passed as void* (the caller's current PyTorch HIP stream).
 *   - every function returns 0 on success, non-zero on error; rf_last_error() gives the message.
 *   - activations are channels-last: a tensor [B, H, W, C] is a row-major matrix [B*H*W, C].
 *   - dtype codes: RF_F32 = 0 (fp32 storage, exact-fp32 MFMA), RF_BF16 = 1 (bf16 storage, fp32 accumulate), RF_F16 = 4 (IEEE fp16 storage on
 *     v_mfma_f32_32x32x16_f16, fp32 accumulate: the bf16 mode's kernels at the same matrix-core rate with 11 significant bits instead of 8 --
 *     the "fp16" throughput mode; accepted wherever RF_BF16 is unless an entry point says otherwise, never mixed with bf16 inside one call).
 */
#ifndef REFACE_HIP_H
#define REFACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { RF_F32 = 0, RF_BF16 = 1, RF_FP8_E4M3 = 2 /* OCP e4m3fn weights (rf_conv_gemm_desc.w_dtype only) */,
       RF_BF16X3 = 3 /* split-bf16 operand pairs, see rf_conv_gemm_desc.dtype and rf_split_bf16 */,
       RF_F16 = 4 /* IEEE binary16 storage (the "fp16" throughput mode) */ };

/* epilogue activations of rf_conv_gemm.  RF_ACT_ADD_RELU is the one code applied AFTER the residual: out = relu(alpha * acc + bias + rowvec
 * + residual), the tail of a ResNet block (never split-K; not with LayerNorm folding or fp8 output) */
enum { RF_ACT_NONE = 0, RF_ACT_GEGLU = 1, RF_ACT_SILU = 2, RF_ACT_QUICK_GELU = 3, RF_ACT_GELU = 4,
       RF_ACT_RELU = 5, RF_ACT_SIGMOID = 6, RF_ACT_PRELU = 7, RF_ACT_ADD_RELU = 8 };

const char* rf_last_error(void);
int rf_version(void);

/*
 * rf_conv_gemm -- implicit-GEMM convolution / linear layer on the matrix cores:
 *
 *     out[m, n] = act( alpha * sum_k A[m, k] * W[n, k] + bias[n] + rowvec[sample(m), n] ) + residual[m, n]
 *
 * A is never materialised: row m is output pixel (b, oy, ox); k = (ky*KW + kx) * (C0 + C1) + c
 * addresses input pixel (oy*stride - pad_t + ky, ox*stride - pad_l + kx) of a channels-last source,
 * optionally nearest-upsampled x2 on the fly (`ups`) and optionally the channel concatenation of two
 * sources [src0 | src1] (UNet skip connections).  KH = KW = 1 with B*Hin*Win = M gives a plain GEMM
 * (nn.Linear / 1x1 conv); `batch` > 1 runs independent problems (strides in elements).
 * Any KH x KW window (KH != KW included), any stride and any pad_t / pad_l, input pixels outside the image read as zero: the direct-to-LDS
 * main loop takes windows with Hout <= 1024, Wout <= 1024 and fewer than 4095 samples (its packed row descriptor sample:12 | oy:10 | ox:10),
 * the register loop everything beyond them and every K that is not whole K tiles per tap -- both pinned bit-exactly on either side of each
 * limit and at the towers' windows (7x7 s2, 11x11 s4, 5x5, 3x3 s2, 1x1 s2, patch = stride, 3 channels stored in 4 / 8) by tests/gemm_exact_refs.py.
 *
 * Replaces: F.conv2d 3x3 / 1x1 in ResBlock, Downsample, Upsample, UNet in/out convs
 * (openaimodel.py:107,116,151-153,204,230,241,669,835), nn.Linear in attention / GEGLU / time-embed
 * (attention.py:40,60,159-170; openaimodel.py:218-224,632-636), torch.cat([h, hs.pop()])
 * (openaimodel.py:898), F.interpolate nearest (openaimodel.py:116), the VAE convs
 * (model.py:60-79,97-121,155-174) and bmm in the VAE AttnBlock (model.py:186-198).
 */
typedef struct rf_conv_gemm_desc {
    /* dtype RF_BF16X3: every fp32 operand value x is stored as the bf16 pair hi = bf16(x), lo = bf16(x - hi) -- a src0 pixel is */
    /* [C0 hi | C0 lo] (ld0 >= 2 C0), a W row holds per 64-element K tile [64 hi | 64 lo | 64 hi] (3 K bf16; ldw >= 3 K) -- and a product is */
    /* accumulated in fp32 as hi hi + hi lo + lo hi on the bf16 MFMA (relative error 2^-16 per product; out_dtype RF_F32, one source, */
    /* K and C0 multiples of 64, K / C0 / ld0 given in REAL elements): the fast form of the fp32 VAE convolutions (model.py:60-121). */
    int32_t dtype;        /* RF_F32 | RF_BF16 | RF_F16: element type of src0/src1/W; RF_BF16X3: split-bf16 pairs (above) */
    int32_t out_dtype;    /* element type of out and residual */
    int32_t M, N, K;      /* GEMM view; K = KH*KW*(C0+C1) (may be padded up to a multiple of 8) */
    const void* src0;
    const void* src1;     /* optional second source (channel concat), NULL if unused */
    int32_t C0, C1;       /* channels taken from src0 / src1 */
    int32_t ld0, ld1;     /* pixel pitch (elements) of src0 / src1 */
    int32_t Hin, Win;     /* spatial size of the stored source (before `ups`) */
    int32_t Hout, Wout;   /* spatial size of the output; M = B*Hout*Wout */
    int32_t KH, KW, stride, pad_t, pad_l, ups;
    /* ups: 0 none.  1: the window runs over the nearest-x2 upsampled source (address >> 1; Hout x Wout = 2 Hin x 2 Win for 3x3 / stride 1 / pad 1). */
    /* 2: the same 3x3 convolution with the upsampling folded into the WEIGHTS: output pixel (2i + py, 2j + px) is a 2x2 window of the stored source */
    /* at (i - 1 + py + ty, j - 1 + px + tx) on phase weights Wf[py][px][n][ty][tx][c] = sum of the 3x3 taps that land on that source pixel (rows */
    /* {0}, {1, 2} for py = 0 and {0, 1}, {2} for py = 1, columns alike): K = 4 C0 instead of 9 C0.  Descriptor: KH = KW = 2, stride 1, pad_t = pad_l = 1 */
    /* (phase (0, 0)'s; phase (py, px) pads (1 - py, 1 - px)), Hout = 2 Hin, Wout = 2 Win, M = B Hout Wout with GEMM rows ordered (sample, phase = */
    /* 2 py + px, i, j) -- `out` is still addressed by pixel --, W = the four [N][ldw] matrices one behind the other.  bf16 / fp16 operands on the */
    /* direct-to-LDS loop (C0 a multiple of 64), one source, batch 1, korder 0 / 1, no srcx / residual / rowvec / LayerNorm fold / GEGLU / fp8, no */
    /* split-K, and Hin * Win a multiple of the tile rows (rf_conv_gemm_plan2 fails otherwise); fused GroupNorm statistics work as usual. */
    const void* W;        /* [N][K] row-major with row pitch ldw */
    int32_t ldw;          /* row pitch of W in elements (0 = K) */
    const float* bias;    /* [N] fp32 or NULL */
    const float* rowvec;  /* [M / rows_per_sample][ldv] fp32 or NULL */
    int32_t rows_per_sample, ldv;
    const void* residual; /* [M][ldr] (out_dtype) or NULL */
    int32_t ldr;
    int32_t act;          /* RF_ACT_* ; GEGLU: W rows interleaved in blocks of 32 (value|gate), out has N/2 columns */
    void* out;
    int32_t ldo;
    float alpha;
    int32_t batch;        /* >= 1 */
    int64_t sA, sW, sO, sR;   /* batch strides (elements) of src0, W, out, residual */
    const float* act_vec; /* [N] fp32 per-column activation parameter (PReLU slopes) or NULL */
    int32_t korder;       /* 0: k = tap*(C0+C1) + c;  1: k = ((c / BK)*KH*KW + tap)*BK + c % BK, BK = 64 (bf16) / 32 (fp32) */
    void* workspace;      /* optional fp32 scratch for split-K (small-M / long-K problems that cannot fill 256 CUs); NULL = never split */
    int64_t workspace_bytes;
    int32_t gn_rows;      /* > 0: also emit GroupNorm(32) partial sums of `out` (rows per sample = H*W) for up to two consumers, see below */
    double* gn_part0;     /* consumer 0: [M / gn_rows][gn_nchunks0][32][2] fp64 (sum, sumsq) in the rf_groupnorm_stats layout, or NULL */
    int32_t gn_cpg0, gn_coff0, gn_slot0, gn_nchunks0;   /* its channels per group, position of out column 0 in its channel space, first chunk slot, chunk slots per sample */
    double* gn_part1;     /* consumer 1 (e.g. the decoder norm over [h | skip], which groups the same channels differently), or NULL */
    int32_t gn_cpg1, gn_coff1, gn_slot1, gn_nchunks1;
    /* fp8 weight path (BASELINE configs[4]): w_dtype = RF_FP8_E4M3 with dtype = RF_BF16 -- W holds OCP e4m3fn bytes, [N][ldw] with */
    /* ldw (BYTES) a multiple of 128 and every row zero-padded to it, dequantised on the way from LDS to the bf16 MFMA as */
    /* w = fp8 * wscale[n], wscale[n] a power of two (rf_quantize_fp8_rows produces both).  0 = W has the element type `dtype`. */
    /* Replaces the same nn.Conv2d / nn.Linear weights (openaimodel.py:204,230,241; attention.py:40,60,159-170), half the bytes. */
    int32_t w_dtype;
    const float* wscale;  /* [N] fp32, powers of two */
    /* fp8 x fp8 path (the fp8 matrix pipe, v_mfma_scale_f32_32x32x64_f8f6f4): dtype = w_dtype = RF_FP8_E4M3.  src0 holds e4m3fn activation bytes */
    /* (ld0 / C0 / K in bytes = elements) and ascale one E8M0 byte (scale 2^(e - 127)) per (pixel, 32-channel block) with pixel pitch as_ld (a */
    /* multiple of 4, pad bytes = a valid code), both written by rf_quantize_fp8_act or by rf_groupnorm_apply / rf_layernorm with out_dtype = */
    /* RF_FP8_E4M3; W as in the w_dtype path with every filter tap's channel run zero-padded to a multiple of 128 (K counts the padded run; a */
    /* k x k window needs C0 % 128 == 0 -- a 1 x 1 / linear layer may over-read up to 127 bytes of the next pixel against zero weights). */
    /* out_dtype RF_BF16.  Replaces the same nn.Conv2d / nn.Linear calls with both operands in fp8 (BASELINE configs[4]). */
    const void* ascale;
    int32_t as_ld;
    /* out_dtype = RF_FP8_E4M3 (fp8 x fp8 path with act = GEGLU only): out receives the N/2 gated values as e4m3fn bytes (ldo in bytes) and oscale */
    /* one E8M0 byte per (row, 32 output columns), row pitch os_ld -- the A operand of the following ff.net.2 GEMM (attention.py:60). */
    void* oscale;
    int32_t os_ld;
    /* LayerNorm folded around two bf16 GEMMs (attention.py:231-233, 239-243: norm1 in front of to_q / to_k / to_v, norm3 in front of ff.net.0). */
    /* PRODUCER of the tensor to be normalised (direct epilogue, no split-K): ln_stats_out [M][ln_out_parts][2] fp32 receives, per row and per */
    /* column stripe of its wave tile (rf_conv_gemm_plan2's wave_cols; ln_out_parts = N / wave_cols), the (mean, M2 = sum of squared deviations) */
    /* of the values as stored.  CONSUMER (A = that tensor, un-normalised): out = act(rstd[m] * (alpha * acc - mean[m] * ln_u[n]) + bias[n]) with */
    /* mean / rstd of row m combined from ln_stats_in [M][ln_in_parts][2] (ln_in_cols columns per part, eps = ln_eps); the caller folds gamma */
    /* into W's columns, passes ln_u[n] = sum_k W[n, k] (of the folded, rounded W) and W beta (+ the layer's bias) as `bias`. */
    /* Replaces the nn.LayerNorm pass between the two GEMMs (one read + one write of [M, C] and a launch). */
    void* ln_stats_out;
    int32_t ln_out_parts;
    const void* ln_stats_in;
    int32_t ln_in_parts, ln_in_cols;
    float ln_eps;
    const float* ln_u;
    /* Per-sample weights (plain GEMM, dtype RF_BF16 / RF_F32, no w_dtype): rows [s * rows_per_sample, (s + 1) * rows_per_sample) multiply */
    /* W + s * w_sample_stride (elements); 0 = one W for all rows.  rows_per_sample must be a multiple of the tile rows (rf_conv_gemm_plan2's BM). */
    /* What rf_groupnorm_fold_linear writes: a GroupNorm folded into the weights of the Linear / 1x1 conv behind it. */
    int64_t w_sample_stride;
    /* Centre-tap tail source (dtype RF_BF16 / RF_F16, a k x k window of ONE source on the direct-to-LDS loop): with srcx != NULL the contraction */
    /* runs on behind the window, K = KH*KW*C0 + Cx, over the Cx channels of srcx at the OUTPUT pixel -- A[m, KH*KW*C0 + c] = srcx[pixel(m)][c] */
    /* -- against the Cx tail columns of every W row (behind the window's columns, which keep their korder).  stride 1, no ups, Hin = Hout, */
    /* Win = Wout, C1 = 0, batch 1, no fp8 / split-bf16 operands, C0 and Cx multiples of the K tile (64).  What it replaces: the 1x1 */
    /* skip_connection of a ResBlock whose channel count changes (openaimodel.py:241, 262) as a launch of its own, the write of its output and */
    /* the re-read of that tensor as the residual of out_layers.3 -- one contraction over [im2col(h) | x] with the two biases summed by the caller. */
    const void* srcx;
    int32_t Cx;
    int32_t ldx;
} rf_conv_gemm_desc;

int rf_conv_gemm(const rf_conv_gemm_desc* d, void* stream);

/* The epilogue tiling rf_conv_gemm would use for `d` -- rows / columns of the block that finishes an output tile (the GEMM tile, or
 * the tile of the split-K reduce pass when splitk > 1) -- and the split-K factor; no launch.  Fused GroupNorm statistics
 * (gn_rows > 0) need gn_rows % bm == 0; a launch then writes (gn_rows / bm) * ceil(N / bn) chunk slots per sample,
 * slot = gn_slot + (row tile within the sample) * ceil(N / bn) + column tile.  Replaces the separate statistics pass of
 * nn.GroupNorm (util.py:214-216) over a tensor this GEMM has just produced. */
int rf_conv_gemm_plan(const rf_conv_gemm_desc* d, int32_t* bm, int32_t* bn, int32_t* splitk);
/* The same query with the whole tile plan: info8 = {statistics rows, statistics cols, splitk, BM, BN, wave_cols (columns of one wave's tile),
 * epilogue form (1 = direct register -> global, 0 = staged), flags: bit 0 = split-K through fragment slabs, bit 1 = the call runs as TWO GEMM
 * kernels (a 256-wide launch whose last round of tiles is 20-60 % full is split along N; the query then also validates the second part)}. */
int rf_conv_gemm_plan2(const rf_conv_gemm_desc* d, int32_t* info8);
/* The same query with everything that names the kernels of the launch: info24[0..7] = rf_conv_gemm_plan2's words, then [8] waves per block (4 | 8),
 * [9] LDS stages of the main loop (2, or 4 for the ring of the 128 x 160 tile), [10] 1 = row-extended A tiles (korder 2), [11] 1 = direct-to-LDS main
 * loop (0: operands go through registers), [12] 1 = convolution addressing (0: plain GEMM), [13] LayerNorm role (0 none, 1 producer, 2 consumer),
 * [14] pm, [15] pn (the tile order inside an XCD's run: patches of pm x pn tiles), [16] reduce pass of split-K (0 none, 1 stripes of 8 rows,
 * 2 stripes of 32 rows, 3 fragment slabs), [17] [18] [19] BM, BN and waves of the SECOND kernel of a two-kernel N split (0 otherwise), [20] tile rows
 * and [21] tile columns of the grid, [22] columns of the first kernel of a two-kernel split, [23] epilogue form of its second kernel.  No launch. */
int rf_conv_gemm_plan3(const rf_conv_gemm_desc* d, int32_t* info24);

/* Fused transformer feed-forward at C = 320 (the 64x64 level):  out = (GEGLU(x W1^T + b1)) W2^T + b2 + residual, bf16 in / out, fp32
 * accumulate, GELU on the 16-bit modes' sigmoid form (degree-5 argument, <= 2.6e-5 from the erf form: csrc/common.h).  The [M, 4C] hidden tensor stays in registers (tokens on lanes, see ffn.hip).
 *   w1p / b1p : ff.net.0.proj [8C, C] / [8C] with rows interleaved in blocks of 32 (value | gate), as rf_conv_gemm's GEGLU takes them
 *   w2q       : ff.net.2 [C, 4C] with the columns of every 16-group in the order 0-3, 8-11, 4-7, 12-15
 *   ln_eps > 0: every row of x is LayerNorm-ed first, in registers (two-pass fp32 statistics, normalised values rounded to bf16 as
 *               rf_layernorm stores them; NO affine: the host folds norm3's gamma into w1p's columns and W1 beta into b1p) -- the kernel then
 *               also replaces `self.norm3` (attention.py:231-233, 243) and x is the un-normalised residual stream.
 * Replaces FeedForward.forward (attention.py:40-76) + the residual add of BasicTransformerBlock (attention.py:243). */
/* (bf16 only: the fp16 mode goes through rf_ffn_block with wpo = NULL and dtype = RF_F16) */
int rf_ffn_geglu(const void* x, int ldx, const void* w1p, const float* b1p, const void* w2q, const float* b2, const void* residual, int ldr,
                 void* out, int ldo, int M, int C, float ln_eps, void* stream);

/* The same kernel with SpatialTransformer.proj_out behind the feed-forward (attention.py:268-272, 288-289) -- the token-resident tail of the block:
 *   out = ((GEGLU(LN?(x) W1^T + b1)) W2^T + b2 + residual) Wpo^T + bpo + res2[row % res2_rows]
 * The feed-forward's output row (rounded to bf16 where the unfused path stores it) never leaves the CU: it is re-laid-out in registers as the B operand
 * of one more MFMA contraction against wpo [C][C] (plain rows, bf16), streamed through the W2 buffers.  res2 = the transformer's input x_in
 * (`return x + x_in`); res2_rows > 0: the residual has that many rows and is shared by the batch halves (the CFG-shared first block).  gn_*: the
 * GroupNorm(32) partial sums of `out` for up to two consumers, as rf_conv_gemm_desc.gn_* (one chunk slot per 128-token block: slot = gn_slot + block
 * within the sample; gn_rows = H*W a multiple of 128).  wpo = NULL: exactly rf_ffn_geglu.  Replaces FeedForward.forward + the residual add +
 * proj_out + `x + x_in` -- and the statistics pass of the GroupNorm that reads the block's output. */
typedef struct rf_ffn_desc {
    const void* x; int32_t ldx;
    const void* w1p; const float* b1p;
    const void* w2q; const float* b2;
    const void* residual; int32_t ldr;
    void* out; int32_t ldo;
    int32_t M, C;
    float ln_eps;
    const void* wpo; const float* bpo;
    const void* res2; int32_t ldr2, res2_rows;
    int32_t gn_rows;
    double* gn_part0;
    int32_t gn_cpg0, gn_coff0, gn_slot0, gn_nchunks0;
    double* gn_part1;
    int32_t gn_cpg1, gn_coff1, gn_slot1, gn_nchunks1;
    int32_t dtype;        /* element type of x / w1p / w2q / residual / out / wpo / res2: RF_BF16 (also 0: the descriptor as it was before the field) or RF_F16 */
    /* attn1.to_out IN FRONT of the feed-forward (attention.py:239-243; needs wpo): wo != NULL makes `x` the attention's output [front_rows or M][ldx] and the block first forms */
    /*   x1 = x Wo^T + bo + ctx[row / rows_per_sample0] + res0[row % front_rows]        (out-projection + the sample's cross-attention vector + the residual tok)             */
    /* rounds it to `dtype`, stores it to x1 -- which must be the same buffer as `residual` -- and continues with it as the feed-forward's input.  front_rows > 0: x / res0  */
    /* have that many rows and are shared by the batch halves (the CFG-shared first block); 0: M rows.  Replaces that rf_conv_gemm launch and the re-read of its output.    */
    const void* wo; const float* bo;
    const float* ctx; int32_t ldc, rows_per_sample0;
    const void* res0; int32_t ldr0, front_rows;
    void* x1; int32_t ldx1;
} rf_ffn_desc;
int rf_ffn_block(const rf_ffn_desc* d, void* stream);

/* The token-resident FRONT of a SpatialTransformer block at C = 320 (attention.py:262-266 `norm`, 276-279 `proj_in`, 231-233 `norm1`, 239 + 159-170 to_q / to_k / to_v)
 * in one kernel (round 6):
 *   tok = x W'_s^T + r_s                 W'_s / r_s: proj_in with the GroupNorm folded in per sample (rf_groupnorm_fold_linear's w_out / rowvec_out)
 *   qkv = LayerNorm(tok) Wqkv'^T + b'    LayerNorm without affine in registers (two-pass fp32 statistics of the STORED tok row, normalised values rounded to `dtype`);
 *                                        the host folds norm1's gamma into wqkv's columns and Wqkv beta into bqkv
 * x [M][ldx] un-normalised, tok [M][ldt] (written: the attention's out-projection reads it back as its residual), qkv [M][ldq] columns [0, 3C), all in `dtype`
 * (RF_BF16, also 0, or RF_F16); wpi [S][C][C] with w_sample_stride elements between samples (0: one matrix), rowvec fp32 [S][ldv], rows_per_sample a multiple of 128
 * dividing M; wqkv [3C][C], bqkv fp32 [3C].  Replaces two rf_conv_gemm launches whose K = 320 main loops are a quarter of their time, the re-read of tok and the
 * LayerNorm statistics exchange between them. */
typedef struct rf_attn_in_desc {
    const void* x; int32_t ldx;
    const void* wpi; int64_t w_sample_stride;
    const float* rowvec; int32_t ldv, rows_per_sample;
    void* tok; int32_t ldt;
    const void* wqkv; const float* bqkv;
    void* qkv; int32_t ldq;
    int32_t M, C;
    float ln_eps;
    int32_t dtype;
} rf_attn_in_desc;
int rf_attn_in(const rf_attn_in_desc* d, void* stream);

/* Per-row fp8 quantisation of a weight matrix for the w_dtype = RF_FP8_E4M3 path: w [N][K] fp32 (row pitch K) ->
 * q [N][ldq] e4m3fn bytes (ldq >= K, a multiple of 128; the pad bytes are written as zero) and scale [N] = the smallest power of
 * two with max|w[n,:]| / scale <= 448 (e4m3fn's largest finite value); q = round-to-nearest-even(w / scale), saturating.
 * Done once at engine build (torch's `.to(float8_e4m3fn)` is the CPU reference in the tests). */
int rf_quantize_fp8_rows(const float* w, int N, int K, int ldq, void* q, float* scale, void* stream);

/*
 * GroupNorm(32 groups) over channels-last [B, HW, C]  (+ optional SiLU), two launches:
 *   rf_groupnorm_stats : per (b, chunk, group) partial (sum, sumsq) in fp64 -> `partial`
 *                        partial must hold B * nchunks * 32 * 2 doubles.
 *   rf_groupnorm_apply : y = (x - mean) * rstd * gamma + beta, optional SiLU.
 * Replaces nn.GroupNorm / GroupNorm32 + nn.SiLU (util.py:214-216, attention.py:76-77,
 * model.py:33-39; openaimodel.py:201-203,225-227,832-834).
 */
int rf_groupnorm_stats(int dtype, const void* x, int B, int HW, int C, int ldx, int nchunks, double* partial, void* stream);
/* [B][nchunks][32][2] -> [B][1][32][2] in a fixed summation order: compacts the many chunk slots that GEMM-fused statistics produce
 * on large images (one slot per output tile) so that rf_groupnorm_apply reads one slot per sample. */
int rf_groupnorm_finalize(const double* partial_in, int B, int nchunks, double* partial_out, void* stream);
int rf_groupnorm_apply(int dtype, const void* x, int B, int HW, int C, int ldx, int nchunks, const double* partial,
                       const float* gamma, const float* beta, float eps, int silu, int out_dtype, void* out, int ldo, void* stream);
/* GroupNorm(32) folded into the Linear / 1x1 conv that follows it (SpatialTransformer: `norm` then `proj_in`, attention.py:262-266 / 276-279):
 *   Linear(GN(x))[m, n] = sum_k W'_s[n, k] x[m, k] + r_s[n]        for the rows m of sample s, with
 *   W'_s[n, k] = W[n, k] rstd[s, g(k)] gamma[k]    (rounded to out_dtype)        r_s[n] = bias[n] + sum_k W[n, k] beta[k] - sum_k W'_s[n, k] mean[s, g(k)]
 * (mean / rstd from the same `partial` records rf_groupnorm_apply reads; the mean's term uses the ROUNDED W' so that it cancels exactly what
 * the matrix pipe accumulates).  W fp32 [N][C]; w_out [B][N][C] (rf_conv_gemm_desc.w_sample_stride = N * C), rowvec_out fp32 [B][N] (the GEMM's
 * per-sample vector, no bias).  Replaces the rf_groupnorm_apply pass over [B, HW, C] in front of that Linear: a read + a write of the tensor. */
int rf_groupnorm_fold_linear(const float* W, int N, int C, int B, int HW, int nchunks, const double* partial, const float* gamma, const float* beta,
                             const float* bias, float eps, int out_dtype, void* w_out, float* rowvec_out, void* stream);

/* GroupNorm(32) + SiLU + 3x3 convolution (stride 1, pad 1) to No <= 4 output channels in one pass over the RAW tensor -- the UNet's `out` head
 * (openaimodel.py:737-741: normalization(ch), nn.SiLU(), conv_nd(dims, model_channels, out_channels, 3, padding=1)): x [B][H*W][ldx] un-normalised in
 * `dtype` (RF_BF16 | RF_F16), `partial` its GroupNorm partial sums (the records rf_groupnorm_apply reads), W [No][9 C] in `dtype` (k = tap * C + c),
 * out [B*H*W][ldo] fp32 or `dtype`.
 * Kernel 1 normalises + activates every pixel's C values in registers (rounded to bf16 as the apply pass stores them) and multiplies them with
 * all nine taps' weights on the matrix pipe (per-tap partial products, fp32, into `workspace`: B*H*W * 160 bytes); kernel 2 sums, per output pixel,
 * the taps whose source pixel lies inside the image.  Replaces rf_groupnorm_apply + rf_conv_gemm for this layer: one read of the tensor instead of a
 * write + nine tap-shifted reads.  C in {320, 128, 64}. */
int rf_gn_silu_conv3x3_small(int dtype, const void* x, int B, int H, int W, int C, int ldx, int nchunks, const double* partial, const float* gamma,
                             const float* beta, float eps, int silu, const void* w, const float* bias, int No, int out_dtype, void* out, int ldo,
                             float* workspace, long long workspace_bytes, void* stream);

/* The UNet's stem -- 3x3 convolution (stride 1, pad 1) from the 9 input channels (stored in 16) to C = model_channels (openaimodel.py:666-671:
 * TimestepEmbedSequential(conv_nd(dims, in_channels, model_channels, 3, padding=1))) -- as one pixels-on-lanes kernel: x bf16 [B][H*W][ldx]
 * (channels 0..15 of a pixel; pad channels zero), W bf16 [C][144] with k = tap * 16 + c, bias fp32 [C], out bf16 [B*H*W][ldo].
 * dup_off != 0: every output row is also stored at out + dup_off elements (classifier-free guidance feeds both batch halves the same latent: one
 * half is computed).  GroupNorm(32) partial sums of the values as stored for up to THREE consumers, as rf_conv_gemm_desc.gn_* (one chunk slot per
 * 128-pixel block: slot = gn_slot + block within the sample; sample b of the kernel writes sample b of gn_part -- point gn_part at the consumer's first
 * sample of this producer, e.g. the duplicate half).  H*W a multiple of 128; C in {320, 128, 64}.  Replaces rf_conv_gemm for this layer and the
 * rf_groupnorm_stats pass over its output. */
typedef struct rf_stem_desc {
    const void* x; int32_t ldx;
    int32_t B, H, W, C;
    const void* w; const float* bias;
    void* out; int32_t ldo;
    long long dup_off;
    double* gn_part0;
    int32_t gn_cpg0, gn_coff0, gn_slot0, gn_nchunks0;
    double* gn_part1;
    int32_t gn_cpg1, gn_coff1, gn_slot1, gn_nchunks1;
    double* gn_part2;
    int32_t gn_cpg2, gn_coff2, gn_slot2, gn_nchunks2;
    int32_t dtype;        /* element type of x / w / out: RF_BF16 (also 0) or RF_F16 */
} rf_stem_desc;
int rf_conv3x3_stem(const rf_stem_desc* d, void* stream);


/* LayerNorm over the last dim of [M, C] (eps, affine).  Replaces nn.LayerNorm (attention.py:231-233,
 * xf.py:22-28, HF CLIP layer norms). */
int rf_layernorm(int dtype, const void* x, int M, int C, int ldx, const float* gamma, const float* beta, float eps,
                 int out_dtype, void* out, int ldo, void* stream);

/*
 * Fused multi-head attention  out = softmax(scale * q k^T) v  without materialising the scores.
 * q/k/v/out are [B, N, heads*d] views with pixel pitches ldq/ldk/ldv/ldo (so q, k, v may live in
 * one fused [B, N, 3*heads*d] buffer).  Nq query tokens, Nk key tokens per batch element.
 * Replaces attention.py:206-220 (einsum + softmax + einsum) and HF CLIPAttention.
 */
int rf_attention(int dtype, const void* q, const void* k, const void* v, void* out,
                 int B, int heads, int d, int Nq, int Nk, int ldq, int ldk, int ldv, int ldo,
                 int64_t sq, int64_t sk, int64_t sv, int64_t so, float scale, void* stream);
/* The launch plan rf_attention takes for these sizes, as a host-only query (no pointers, no launch, no device needed; the decision is the one
 * rf_attention itself reads).  info12 = { kernel family (0 generic, 1 x3 = split-bf16 pairs, 2 dma = the in-wave pipelined LDS-DMA kernel),
 * storage dtype (RF_F32 for RF_BF16X3), D, 32-query blocks per wave, keys per LDS stage, waves per block, LDS stages (1 | 2; the ring depth
 * 3 | 7 for dma), softmax denominator accumulated by the MFMA (0 | 1), queries per block, grid blocks, dynamic LDS bytes, grid % 8 }.
 * A head dim that is not instantiated returns rf_attention's own error. */
int rf_attention_plan(int dtype, int B, int heads, int d, int Nq, int Nk, int32_t* info12);

/* fp8 activation producers of the fp8 x fp8 GEMM path (rf_conv_gemm_desc.ascale): bf16 in -> e4m3fn bytes q [rows][ldq] + one E8M0 scale byte per
 * (row, 32-channel block), scale [rows][lds]; the scale is the smallest power of two that brings the block's |max| under 448, values are
 * rounded to nearest even.  Bytes of q beyond C and scale bytes beyond C / 32 are NOT written (the caller keeps them 0 / 127).
 *   rf_quantize_fp8_act     : plain quantisation of x [M, C]
 *   rf_groupnorm_apply_fp8  : rf_groupnorm_apply (nn.GroupNorm + SiLU, util.py:214-216) with this output form
 *   rf_layernorm_fp8        : rf_layernorm (nn.LayerNorm, attention.py:231-233) with this output form */
int rf_quantize_fp8_act(const void* x, int64_t M, int C, int ldx, void* q, int ldq, void* scale, int lds, void* stream);
int rf_groupnorm_apply_fp8(const void* x, int B, int HW, int C, int ldx, int nchunks, const double* partial, const float* gamma,
                           const float* beta, float eps, int silu, void* q, int ldq, void* scale, int lds, void* stream);
int rf_layernorm_fp8(const void* x, int M, int C, int ldx, const float* gamma, const float* beta, float eps, void* q, int ldq, void* scale,
                     int lds, void* stream);

/* Row softmax over the last dim of [rows, cols] fp32, in place allowed (VAE AttnBlock, model.py:188). */
int rf_softmax_rows(float* x, int rows, int cols, int ld, void* stream);

/*
 * DDIM step glue (ddim.py:330-374):
 *   rf_ddim_pack_input : x_in[2B or B, h, w, Cpad] = [img | z_inpaint | mask | 0-pad], duplicated for CFG.
 *   rf_ddim_update     : e = e_u + s (e_c - e_u); pred_x0 = (x - sqrt(1-a_t) e) / sqrt(a_t);
 *                        x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) e + sigma * noise.
 *   All latent tensors are fp32 NCHW [B, 4, h, w] (the sampler's external layout); eps is the UNet
 *   output in channels-last fp32 [2B or B, h*w, ld_eps].  `coefs` is a DEVICE array of 5 fp32 step
 *   coefficients {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma}, so one captured
 *   hipGraph of a step can be replayed for every timestep.
 */
int rf_ddim_pack_input(const float* img, const float* z_inpaint, const float* mask, int B, int hw, int dup,
                       int out_dtype, void* x_in, int Cpad, void* stream);
int rf_ddim_update(const float* eps, int ld_eps, int cfg, float scale, float* img, float* pred_x0, const float* noise,
                   int B, int hw, const float* coefs, void* stream);

/*
 * DPM-Solver++ multistep update (data prediction), the few-step alternative to rf_ddim_update on the same layouts:
 *   e = e_u + s (e_c - e_u) when cfg;  m0 = (x - sigma_i e) / alpha_i;
 *   x' = A x + k0 m0 + k1 m1 + k2 m2 (in place into img);  then the history shifts: m2 <- m1, m1 <- m0.
 * `coefs` is a DEVICE array of 8 fp32 {alpha_i, sigma_i, A, k0, k1, k2, n_hist, 0} (reface_amd/dpm_solver.py::dpm_coefficients), so a captured
 * hipGraph of a step can be replayed for every step.  n_hist = 0, 1 or 2 says how many history terms enter the sum: the others are not read
 * into it (the buffers of a first step are uninitialised).  m1 doubles as the pred_x0 output.  m2 may be NULL when no row has n_hist = 2
 * (orders 1 and 2).  img, m1, m2: distinct fp32 NCHW [B, 4, hw] buffers.
 */
int rf_dpm_update(const float* eps, int ld_eps, int cfg, float scale, float* img, float* m1, float* m2, int B, int hw,
                  const float* coefs, void* stream);

/* Layout / dtype helpers. */
int rf_nchw_to_nhwc(const float* x, int B, int C, int HW, int out_dtype, void* out, int Cpad, void* stream);
int rf_nhwc_to_nchw(int dtype, const void* x, int B, int C, int HW, int ldx, float* out, void* stream);
int rf_cast(int in_dtype, const void* x, int out_dtype, void* out, int64_t n, void* stream);
/* fp32 [M, C] (row pitch ldx) -> split-bf16 pairs [M][C hi | C lo] (row pitch ldo >= 2C, bf16): hi = bf16(x), lo = bf16(x - hi), the
 * RF_BF16X3 operand form of rf_conv_gemm.  rf_groupnorm_apply writes the same form directly with out_dtype = RF_BF16X3; this pass is for
 * tensors that reach a convolution without a normalisation in between (VAE Upsample conv / nin_shortcut, model.py:53-57,117-121). */
int rf_split_bf16(const float* x, int64_t M, int C, int ldx, void* out, int ldo, void* stream);
/* sinusoidal timestep embedding [n, dim] = [cos(t f) | sin(t f)] (util.py:151-166); freqs [dim/2] fp32 */
int rf_timestep_embedding(const float* t, int n, int dim, const float* freqs, float* out, void* stream);
/* KL-VAE posterior sample (distributions.py:24-37, ddpm.py:857): moments NCHW [B, 2C, HW] = (mean | logvar),
 * eps NCHW [B, C, HW] or NULL (mode):  out = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) */
int rf_gaussian_sample(const float* moments, const float* eps, float scale, float* out, int B, int C, int HW, void* stream);
/*
 * Conditioning-encoder side kernels (ArcFace IR-SE50: src/Face_models/encoders/helpers.py:56-119, model_irse.py:20-69,
 * ldm/models/diffusion/ddpm.py:112-124; CLIP ViT: HF CLIPVisionEmbeddings; ddpm.py:907-912).
 *   rf_channel_affine  : y[m,c] = prelu(x[m,c]*a[c] + b[c])   (eval BatchNorm as affine, optional PReLU slopes)
 *   rf_spatial_mean    : [B,HW,C] -> fp32 [B,C]              (SE squeeze, AdaptiveAvgPool2d(1))
 *   rf_se_scale_add    : out = r * s[b,c] + shortcut[b, oy*stride, ox*stride, c]   (SE excite + MaxPool2d(1,stride) shortcut)
 *   rf_adaptive_avgpool: AdaptiveAvgPool2d over a crop window of NCHW fp32 with input affine; NCHW fp32 or NHWC out
 *   rf_bilinear_resize : F.interpolate(bilinear, align_corners=False, antialias=False) of NCHW fp32 with input affine
 *   rf_clip_tokens     : [cls + pos[0] ; patch + pos[1:]] token assembly
 *   rf_l2norm_rows     : x / ||x||_2 per row (fp32)
 */
int rf_channel_affine(int dtype, const void* x, int ldx, const float* a, const float* b, const float* slope, int out_dtype,
                      void* y, int ldy, int64_t M, int C, void* stream);
int rf_spatial_mean(int dtype, const void* x, int B, int HW, int C, int ldx, float* out, void* stream);
int rf_se_scale_add(int dtype, const void* r, const float* s, const void* sc, int ldsc, int Hs, int Ws, int stride, void* out,
                    int B, int Ho, int Wo, int C, void* stream);
int rf_adaptive_avgpool(const float* x, int B, int C, int Hf, int Wf, int y0, int x0, int hc, int wc, const float* a, const float* b,
                        int Ho, int Wo, int out_nhwc, int out_dtype, int Cpad, void* out, void* stream);
int rf_bilinear_resize(const float* x, int B, int C, int Hi, int Wi, const float* a, const float* b, int Ho, int Wo, float* out, void* stream);
int rf_clip_tokens(int dtype, const void* patch, const float* cls, const float* pos, void* out, int B, int NP, int C, void* stream);
int rf_l2norm_rows(const float* x, float* y, int rows, int cols, void* stream);
/* conditioning combine (ddpm.py:1038-1039): out = (a*wa + b*wb + c*wc) / den (den = 0: no division); b, c may be NULL */
int rf_combine3(const float* a, const float* b, const float* c, float wa, float wb, float wc, float den, float* out, int64_t n, void* stream);
/* y = clamp((x + 1) / 2, 0, 1)  (scripts/inference_test_bench.py:494) */
int rf_to_image(const float* x, float* y, int64_t n, void* stream);

/*
 * Input preparation on the device -- what the test-bench dataset does per image on the host (ldm/data/test_bench_dataset.py:283-355:
 * torchvision ToTensor + Normalize, np.isin label masks, tensor products).  Same float operation order => bit-identical tensors (the resized source mask: 1 ulp).
 *   rf_u8_to_norm : uint8 [B, HW, 3] (HWC) -> fp32 [B, 3, HW]: (x / 255 - mean[c]) / std[c]
 *   rf_label_mask : uint8 label map [n] -> fp32 {0, 1}: lut256[label] != 0, optionally inverted (target keep-mask = 1 - isin)
 *   rf_mul_mask   : out[b, c, p] = x[b, c, p] * mask[b, p]
 */
int rf_u8_to_norm(const void* x_u8, int B, int HW, const float* mean3, const float* std3, float* out, void* stream);
int rf_label_mask(const void* labels_u8, int64_t n, const void* lut256_u8, int invert, float* out, void* stream);
int rf_mul_mask(const float* x, const float* mask, int B, int C, int HW, float* out, void* stream);
/*
 * rf_resize_u8_linear : cv2.resize(img, (Wo, Ho), interpolation=cv2.INTER_LINEAR) of uint8 HWC images [B, H, W, C] (image b at
 * x + b * image_stride bytes) -> uint8 [B, Ho, Wo, C]: what albumentations' A.Resize(224, 224) runs on the source face
 * (ldm/data/test_bench_dataset.py:141-148, 324; scripts/inference_swap_selected.py:525-553).  OpenCV's integer algorithm and operation order (no cv2-generated golden exists here: last bit unpinned)
 * (half-pixel centres, two taps per axis, 11-bit weights, NO antialiasing; exact 2:1 -> the fast-area average); cv2 itself is a
 * third-party dependency absent from /root/reference and from this image: see reface_amd/data.py::resize_u8_linear for the restatement.
 */
/*
 * rf_compose_outputs_u8 : the CLI's output files as uint8 HWC arrays, one packed record per image:
 *     [result | mask (grey replicated) | GT | inpaint | ref]  5 x [H][W][3],  then (with_grid) the 4-panel make_grid image
 *     [H + 4][4 W + 10][3] of (GT, inpaint, ref, result) with 2-pixel padding (pad bytes untouched: zero them once).
 * Every conversion is the reference's (255. * x).astype(np.uint8) of fp32 values (scripts/inference_test_bench.py:500-552:
 * un_norm, un_norm_clip, make_grid, rearrange + astype): truncation toward zero, low byte.  Inputs NCHW fp32 on the device:
 * result01 = clamp((x + 1) / 2, 0, 1), target / inpaint in [-1, 1], mask [B, 1, H, W] in {0, 1}, ref = the CLIP-normalised source
 * already resized to H x W.  Replaces the per-image host float passes; the host then only PNG-encodes slices of one D2H copy.
 */
int rf_compose_outputs_u8(const float* result01, const float* target, const float* inpaint, const float* mask, const float* ref, int B, int H, int W,
                          int with_grid, void* out_u8, int64_t record_bytes, void* stream);
int rf_resize_u8_linear(const void* x_u8, int B, int H, int W, int C, int64_t image_stride, int Ho, int Wo, void* out_u8, void* stream);
/*
 * BiSeNet face parser (pretrained/face_parsing/{model,resnet,face_parsing_demo}.py): the passes around its rf_conv_gemm convolutions.
 * fp32 storage, channels-last.
 *   rf_parse_prep    : uint8 HWC crops [B, H, W, 3] (H, W even, >= 4) -> fp32 [B, H/2, W/2, 8]: ToTensor (x / 255), BicubicDownSample(2)
 *                      (8 cubic taps a = -0.5, reflect padding 3 | 3, vertical pass then horizontal pass, no rounding), clamp(0, 1),
 *                      (x - ImageNet mean) / std; channels 3..7 zero (face_parsing_demo.py:116-185, 270-279)
 *   rf_maxpool3x3s2  : MaxPool2d(3, 2, padding 1) of [B, H, W, C] -> [B, (H-1)/2+1, (W-1)/2+1, C], padding = -inf (resnet.py:58)
 *   rf_add_relu      : out = relu(a + r), n elements (BasicBlock tail, resnet.py:41-47)
 *   rf_scale_add_vec : out[b, p, c] = x[b, p, c] * s[b, c] + v[b, c] over [B, HW, C] (ARM32 + global context, model.py:99,121-122)
 *   rf_parse_head    : logits [B, h, w, C] (pixel pitch ldl) -> uint8 [B, H, W]: lut256[argmax_c bilinear(align_corners=True)] with the
 *                      first maximum winning; the upsampled logits are never stored (model.py:252, face_parsing_demo.py:293, 309-311)
 */
int rf_parse_prep(const void* x_u8, int B, int H, int W, float* out, void* stream);
int rf_maxpool3x3s2(const float* x, int B, int H, int W, int C, float* out, void* stream);
int rf_add_relu(const float* a, const float* r, float* out, int64_t n, void* stream);
int rf_scale_add_vec(const float* x, const float* s, const float* v, float* out, int B, int HW, int C, void* stream);
int rf_parse_head(const float* logits, int B, int h, int w, int C, int ldl, int H, int W, const void* lut256_u8, void* out_u8, void* stream);
/*
 * Video paste-back (stage 3 of scripts/inference_swap_video.py:705-724): PIL's arithmetic, byte for byte (libImaging/Resample.c, Geometry.c).
 *   rf_paste_crop_u8 : fp32 NCHW [B, 3, h, w] in [0, 1] (run_batch's result) -> u8 HWC [B, S, S, 3]: the reference's (255.f * x) truncation
 *                      to u8, then Image.resize((S, S), BILINEAR): separable, horizontal pass first, u8 between the passes; per axis
 *                      center = (i + .5) * in / out, taps [int(center - .5), int(center + 1.5)) clipped, triangle weights normalised to 1
 *                      and made int(w * 2^22 + .5); out = clip((2^21 + sum k x) >> 22, 0, 255).  Upscale only (S >= h, w; else rc 1).
 *   rf_paste_back_u8 : crops u8 [B, S, S, 3], coeffs fp64 [B, 8] (the inverse transforms of stage 1: frame -> crop), frames u8 [B, H, W, Cf]
 *                      (frame b at frames + b * frame_stride bytes) -> out u8 [B, H, W, Co] (packed), Cf, Co in {3, 4}: Image.transform(
 *                      (W, H), PERSPECTIVE, c, BILINEAR) of the alpha-255 crop alpha-composited over the frame.  Per pixel in fp64, PIL's
 *                      operation order: d = c6 (x+.5) + c7 (y+.5) + 1, sx = (c0 (x+.5) + c1 (y+.5) + c2) / d, sy likewise; outside
 *                      [0, S)^2 or not finite: the frame pixel (its alpha, or 255); inside: PIL's bilinear_filter32RGB (lerp along x on
 *                      rows clamp(y0) and y0 + 1 if it exists, then along y), truncated, alpha 255.  One launch for the batch.
 *                      out == frames is allowed when Cf == Co and frame_stride == H * W * Cf (every pixel is read before it is written);
 *                      any other overlap of out with crops or frames is undefined.
 */
int rf_paste_crop_u8(const float* x, int B, int h, int w, int S, void* out_u8, void* stream);
int rf_paste_back_u8(const void* crops_u8, int B, int S, const double* coeffs, const void* frames_u8, int H, int W, int Cf, int64_t frame_stride,
                     void* out_u8, int Co, void* stream);
/*
 * The masked paste-back: the swapped crop is composited through a feathered alpha plane made of its face-parsing label map, so that only
 * the region the model repaints (and a soft margin) replaces frame pixels.  Integer and PIL arithmetic throughout, byte for byte.
 *   rf_paste_alpha_u8      : label maps u8 [B, Sl, Sl], lut256 u8 [256] (non-zero = the label is repainted) -> alpha u8 [B, S, S], S >= Sl:
 *                              1. m = lut[label] ? 255 : 0;
 *                              2. dilate: m[y, x] = max of m over |dy| <= dilate, |dx| <= dilate inside the map (0: identity);
 *                              3. feather (skipped when feather = 0): `passes` times a horizontal, then a vertical 1-D box pass
 *                                 out[i] = (sum_{|k| <= feather, 0 <= i + k < Sl} in[i + k] + feather) / (2 feather + 1), integer division:
 *                                 positions outside the map count as 0, so alpha falls off towards the crop's border;
 *                              4. Image.resize((S, S), BILINEAR) of the 8-bit plane (rf_paste_crop_u8's tap arithmetic on one channel);
 *                                 S == Sl copies.
 *                            dilate, feather in 0 .. 64, passes in 1 .. 3, else rc 1.  The passes are separable and go through `scratch_u8`,
 *                            device memory of the caller's of scratch_bytes >= 2 * B * Sl * Sl bytes (two planes, read and written in turn).
 *   rf_paste_back_alpha_u8 : rf_paste_back_u8 with alpha u8 [B, S, S] beside the crops: Image.transform((W, H), PERSPECTIVE, c, BILINEAR) of
 *                            the RGBA image (crop, alpha) alpha-composited over the frame.  Coordinates and the inside test are
 *                            rf_paste_back_u8's (outside or not finite: the frame pixel).  Inside, PIL warps the premultiplied image:
 *                            the four taps are (MULDIV255(c, a), a), MULDIV255(x, y) = t = x y + 128, ((t >> 8) + t) >> 8, filtered by
 *                            bilinear_filter32RGB on all four channels to (pr, pg, pb, pa); unless pa is 0 or 255, c = min(255, 255 pc / pa);
 *                            then Image.alpha_composite over the frame pixel (dr, dg, db, da), da = 255 for 3-channel frames: pa = 0 keeps
 *                            the frame pixel bit for bit; else blend = da (255 - pa), outa255 = 255 pa + blend, coef1 = pa 255 255 128 /
 *                            outa255, coef2 = 255 128 - coef1, colour = SHIFT8(c coef1 + d coef2 + (0x80 << 7)) >> 7, alpha = SHIFT8(outa255
 *                            + 0x80), SHIFT8(x) = ((x >> 8) + x) >> 8.  Strides, channel counts and the in-place rule are rf_paste_back_u8's.
 */
int rf_paste_alpha_u8(const void* labels_u8, int B, int Sl, const void* lut256_u8, int dilate, int feather, int passes, void* scratch_u8,
                      int64_t scratch_bytes, void* alpha_u8, int S, void* stream);
int rf_paste_back_alpha_u8(const void* crops_u8, const void* alpha_u8, int B, int S, const double* coeffs, const void* frames_u8, int H, int W, int Cf,
                           int64_t frame_stride, void* out_u8, int Co, void* stream);
/*
 * Face alignment (stage 1 of the swap callers, src/utils/alignmengt.py:crop_image): PIL's arithmetic, byte for byte (libImaging/Geometry.c,
 * Resample.c) -- the mirror image of the paste-back above.
 *   rf_align_quad_u8 : frames u8 [B, H, W, Cf] (frame b at frames + b * frame_stride bytes, Cf in {3, 4}: only R, G, B are read), coeffs fp64
 *                      [B, 8] -> out u8 [B, S, S, 3]: Image.transform((S, S), QUAD, quad, BILINEAR), the coefficients being those PIL makes
 *                      of the quad (reface_amd.align.quad_coefficients).  Per output pixel in fp64, PIL's operation order: xin = x + .5,
 *                      yin = y + .5, xs = a0 + a1 xin + a2 yin + a3 xin yin, ys = a4 + a5 xin + a6 yin + a7 xin yin; outside the source
 *                      (tested before the -.5 shift) or not finite: 0; inside: PIL's bilinear_filter32RGB, truncated.  `windows` (int32
 *                      [B, 4] on the device, or NULL) gives per frame the sub-rectangle (ox, oy, w, h) that is the source image -- the
 *                      reference's img.crop(...) before the transform, without a copy; a window not inside the frame gives zeros.
 *                      One launch for the batch.  out must not overlap the frames.
 *   rf_resample_u8   : x u8 [B, H, W, C] -> out u8 [B, h, w, C], C in {3, 4}: PIL's two-pass integer resampler (horizontal pass into tmp u8
 *                      [B, H, w, C], then vertical) with the host's tap tables (reface_amd.align.resample_taps, PIL's precompute_coeffs +
 *                      normalize_coeffs_8bpc): per axis, bounds int32 [n_out, 2] = (first input index, tap count) and taps int32
 *                      [n_out, ksize], all on the device; each pass is clip8(((1 << 21) + sum k p) >> 22).  Tap windows are clipped to
 *                      the axis.  x, tmp and out are three distinct buffers.
 */
int rf_align_quad_u8(const void* frames_u8, int B, int H, int W, int Cf, int64_t frame_stride, const double* coeffs, const int* windows, int S,
                     void* out_u8, void* stream);
int rf_resample_u8(const void* x_u8, int B, int H, int W, int C, const int* xbounds, const int* xk, int xksize, const int* ybounds, const int* yk,
                   int yksize, void* tmp_u8, void* out_u8, int h, int w, void* stream);
/*
 * crop_image's enable_padding branch (alignmengt.py:129-140; reface_amd/csrc/align_pad.hip): the crop window of every frame reflect-padded
 * (np.pad), blurred towards the border (scipy.ndimage.gaussian_filter, fp64 accumulation, fp32 between the passes), filled towards the exact
 * channel medians (np.median) and quantised (rint, half to even) -- byte for byte what numpy / scipy give.
 *   rf_align_pad_u8 : frames u8 [B, H, W, Cf] as for rf_align_quad_u8 -> out u8 [B, hmax, wmax, 3]: frame b's padded image of w x h pixels in
 *                     the top-left corner of out[b] (rows of wmax pixels; the rest of out[b] is not written), which rf_align_quad_u8 then
 *                     reads with the window (0, 0, w, h).  desc int32 [B, 16] on the device, per frame: ox oy W0 H0 (the window in the
 *                     frame), w h (padded size, <= wmax, hmax), the blur's radius r, then offsets into itab (int32, n_itab words) of
 *                     extrow [h + 2 r], colmap [w], extcol [w + 2 r], colneed [w] and into dtab (fp64, n_dtab doubles) of the weights
 *                     [r + 1] and the clip profiles c1x [w], c1y [h], c2x [w], c2y [h] -- reface_amd.align.pad_tables makes all of them.
 *                     A descriptor that points outside the frame, the tables or its slot makes its frame a no-op; table entries are
 *                     clamped to the image they index.  scratch_f32: 2 * B * hmax * wmax * 3 floats; select_u32: B * 1548 words.
 *                     stages: a mask of 1 (vertical blur), 2 (horizontal blur + first mix), 4 (median select), 8 (second mix + quantise);
 *                     15 is the whole sequence, 12 launches for any B; a subset runs those kernels on what an earlier call left in the
 *                     scratch (tools/align_rate.py times them one by one).
 */
int rf_align_pad_u8(const void* frames_u8, int B, int H, int W, int Cf, int64_t frame_stride, const int* desc, const int* itab, int n_itab,
                    const double* dtab, int n_dtab, int hmax, int wmax, float* scratch_f32, int64_t scratch_floats, void* select_u32,
                    int64_t select_words, void* out_u8, int stages, void* stream);
/*
 * The video dataset's per-frame preparation (ldm/data/video_swap_dataset.py:135-240) in one launch and one pass over the crops:
 *   rf_video_prep_u8 : crops u8 [B, Hc, Wc, 3] (C must be 3), labels u8 [B, h, w], lut256 u8 [256] (non-zero = a label that is cut out) and the
 *                      two tap tables of rf_resample_u8 (x: Wc -> w, y: Hc -> h; reface_amd.align.resample_taps, "bicubic" for PIL's default
 *                      Image.resize) -> target fp32 [B, 3, h, w] = (resized / 255 - 0.5) / 0.5, mask fp32 [B, 1, h, w] = 1 - (lut[label] != 0),
 *                      inpaint fp32 [B, 3, h, w] = target * mask.  The resize is PIL's two integer passes (u8 between them) done in LDS: the
 *                      resized u8 image is never written to memory.  Bit for bit what the host dataset computes.  Tap windows are clipped to
 *                      the axis; any ratio >= 1 and any h, w.  The three outputs are distinct buffers that overlap neither input.
 */
int rf_video_prep_u8(const void* crops_u8, int B, int Hc, int Wc, int C, const void* labels_u8, const void* lut256_u8, const int* xbounds,
                     const int* xk, int xksize, const int* ybounds, const int* yk, int yksize, float* target, float* mask, float* inpaint, int h, int w,
                     void* stream);
/*
 * The identity metric of the evaluation (eval_tool/ID_retrieval/ID_retrieval.py of the reference: ArcFace ID retrieval and ID similarity of the
 * swapped results against their sources), the two passes around the ArcFace engine:
 *   rf_id_prep_u8  : images u8 [B, H, W, 3] (image b at images + b * image_stride bytes), labels u8 [B, Hl, Wl] (label_stride likewise) and
 *                    lut256 u8 [256] (non-zero = a preserved label) -> out fp32 [B, 3, S, S] = ((resized / 255 - 0.5) / 0.5) * mask: the image
 *                    through cv2's u8 INTER_LINEAR (the arithmetic of rf_resize_u8_linear: A.Resize(S, S)), the 0 / 1 preserved-label mask
 *                    through torchvision's tensor Resize (bilinear, align_corners = False, no antialiasing, fp32, the x lerps first).  One
 *                    pass: neither the resized image nor the mask is written (:189-228).  One size per call; callers group by size.
 *   rf_id_retrieve : f_res fp32 [M, D], f_src fp32 [N, D] (D a multiple of 64, at most 1024), labels i32 [M] in [0, N) -> per result row, over
 *                    the scores S[j] = sum_k f_res[r, k] f_src[j, k] (fp32 widened, fp64 products and sums, k ascending) ordered by score
 *                    descending with TIES TO THE LOWER INDEX: top5 i32 [M, 5] = the five best source indices, best first (-1 where N < 5;
 *                    top5[r][0] is the top-1), rank i32 [M] = the 0-based position of labels[r] in that order, sim fp64 [M] = the cosine of
 *                    f_res[r] and f_src[labels[r]], both renormalised in fp64; then totals fp64 [4] = (rows with rank 0, rows with rank < 5,
 *                    sum of sim, M) in a fixed summation order.  The M x N score matrix is never written (:362-390).  A label outside
 *                    [0, N) gets rank N and similarity 0.  Rows are expected to be non-zero (the engine's are unit-norm): a zero f_res row or
 *                    label row divides by a zero norm, as the reference does -- its sim is NaN and so is totals[2].
 */
int rf_id_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, const void* labels_u8, int Hl, int Wl, int64_t label_stride,
                  const void* lut256_u8, float* out, int S, void* stream);
int rf_id_retrieve(const float* f_res, int M, const float* f_src, int N, int D, const int* labels, int* top5, int* rank, double* sim, double* totals,
                   void* stream);
/*
 * The pose metric of the evaluation (eval_tool/Pose/pose_compare.py of the reference: Hopenet head-pose angles of the swapped results against
 * those of their targets), the three passes around the ResNet-50 body (which runs on rf_conv_gemm):
 *   rf_pose_prep_u8  : images u8 [B, H, W, 3] (image b at images + b * image_stride bytes; any H, W >= 1) -> out fp32 NHWC [B, 224, 224, 8]
 *                      (16-byte aligned) = (resize(u8 / 255) - mean) / std with the ImageNet constants in channels 0..2, zeros in 3..7 (the
 *                      7x7 stem's cin_pad = 8 layout).  The resize is torchvision's tensor Resize of 0.12: bilinear, align_corners = False,
 *                      no antialiasing at any size, fp32, src = max((dst + 0.5) * (in / out) - 0.5, 0), the upper tap clamped to the last
 *                      pixel, the x lerps first; the coordinate and both lerps are FMAs, as in PyTorch's CPU build, where the reference
 *                      resizes.  One pass, one size per call; callers group by size (:91-99).
 *   rf_pose_head     : feat fp32 [B, 7, 7, 2048] (layer4, NHWC), w198 fp32 [198, 2048] (fc_yaw | fc_pitch | fc_roll stacked on rows, 16-byte
 *                      aligned), b198 fp32 [198] -> degrees fp32 [B, 3] (yaw, pitch, roll) and, when `logits` is not null, logits fp32
 *                      [B, 198].  Per image: the mean of the 49 pixels, the 198 dot products, per 66-bin head a softmax shifted by the head's
 *                      maximum (finite for any finite logits) and degrees = sum(p * [0..65]) * 3 - 99 (:101-108).  One workgroup per image:
 *                      the summation order, hence every bit of an image's outputs, does not depend on B.
 *   rf_pose_distance : deg_res fp32 [M, 3], deg_tgt fp32 [N, 3], labels i32 [M] in [0, N) -> dist fp64 [M] = the L2 norm of
 *                      (double)deg_tgt[labels[r]] - (double)deg_res[r] (widened before the subtraction, squares summed in index order), then
 *                      totals fp64 [2] = (sum of dist, M) in a fixed summation order: equal bits on every run (:320-323).  A label outside
 *                      [0, N) is not dereferenced: its dist is NaN, and so is totals[0]; callers refuse such labels before the launch.
 */
int rf_pose_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, float* out, void* stream);
int rf_pose_head(const float* feat, int B, const float* w198, const float* b198, float* degrees, float* logits, void* stream);
int rf_pose_distance(const float* deg_res, int M, const float* deg_tgt, int N, const int* labels, double* dist, double* totals, void* stream);
/*
 * The expression metric of the evaluation (eval_tool/Expression/expression_compare_face_recon.py of the reference: the 64 expression
 * coefficients of Deep3DFaceRecon's net_recon of the swapped results against those of their targets), the three passes around the ResNet-50
 * body (which runs on rf_conv_gemm):
 *   rf_expr_prep_u8  : images u8 [B, H, W, 3] (image b at images + b * image_stride bytes; any H, W >= 1) and the tap tables of PIL's
 *                      Image.resize((512, 512), BICUBIC) per axis (bounds i32 [512, 2] = first input index and tap count, taps i32
 *                      [512, ksize], 22-bit fixed point) -> out fp32 NHWC [B, 512, 512, 8] (16-byte aligned) = resized byte / 255 in channels
 *                      0..2, zeros in 3..7.  PIL's two integer passes with the u8 rounding between them; the horizontally resampled rows live
 *                      in LDS only, for every source size (no intermediate in global memory).  A 512 x 512 source comes out as its own bytes.
 *   rf_expr_head     : feat fp32 [B, P, 2048] (layer4, NHWC, P pixels per image), w fp32 [257, 2048] (final_layers.0..6 stacked on rows, 16-byte
 *                      aligned), bias fp32 [257] -> coeffs fp32 [B, 257] = bias + w . (sum over the P pixels in ascending order / P).  One
 *                      workgroup per image: every bit of an image's coefficients is independent of B.
 *   rf_expr_distance : coef_res fp32 [M, ld], coef_tgt fp32 [N, ld], labels i32 [M] in [0, N) -> dist fp64 [M] = the L2 norm over columns
 *                      [col0, col0 + ncols) of (double)coef_tgt[labels[r]] - (double)coef_res[r] (widened before the subtraction, squares
 *                      summed in column order), then totals fp64 [2] = (sum of dist, M) in a fixed summation order.  Columns outside the range
 *                      are not read.  A label outside [0, N) is not dereferenced: its dist is NaN; callers refuse such labels before the launch.
 */
int rf_expr_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, const int* xbounds, const int* xk, int xksize,
                    const int* ybounds, const int* yk, int yksize, float* out, void* stream);
int rf_expr_head(const float* feat, int B, int P, const float* w257, const float* b257, float* coeffs, void* stream);
int rf_expr_distance(const float* coef_res, int M, const float* coef_tgt, int N, int ld, int col0, int ncols, const int* labels, double* dist,
                     double* totals, void* stream);

/*
 * The FID of the evaluation (eval_tool/fid/fid_score.py of the reference; its features are the `clip` ViT-B/32 image embeddings), the two
 * passes around the vision tower (which runs on rf_conv_gemm, rf_attention and rf_layernorm):
 *   rf_fid_prep_u8 : clip.load's preprocess.  images u8 [B, H, W, 3] (image b at images + b * image_stride bytes; any H, W >= 1) and the tap
 *                    tables of PIL's BICUBIC resize of each axis to Resize(224)'s size, SLICED to the 224 outputs of CenterCrop(224)
 *                    (xbounds / ybounds i32 [224, 2] = first input index and tap count, xk / yk i32 [224, ksize], 22-bit fixed point) ->
 *                    out NHWC [B, 224, 224, CP] (16-byte aligned), out_dtype RF_F32 (CP = 4) or RF_BF16 (CP = 8):
 *                    (float32(byte) / 255 - mean) / std in channels 0..2, each step rounded to fp32, zeros in the pad channels.  PIL's two
 *                    integer passes with the u8 rounding between them; the horizontally resampled rows live in LDS only.
 *   rf_fid_stats   : feat fp32 [N, D] (N >= 2, D a multiple of 16) -> mu fp64 [D] = the mean of the widened rows, sigma fp64 [D, D] =
 *                    sum_i (x_i - mu)(x_i - mu)^T / (N - 1) on the fp64 MFMA, upper-triangle tiles mirrored from the same registers (sigma
 *                    equals its transpose bit for bit).  Fixed summation order, no atomics: the same bits on every run.
 */
int rf_fid_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, const int* xbounds, const int* xk, int xksize,
                   const int* ybounds, const int* yk, int yksize, int out_dtype, void* out, void* stream);
int rf_fid_stats(const float* feat, int N, int D, double* mu, double* sigma, void* stream);
/*
 * The learned perceptual distance of the evaluation (eval_tool/lpips/{lpips,networks,utils}.py of the reference: LPIPS(net_type = 'alex' |
 * 'vgg')), the passes around the AlexNet / VGG16 feature stacks (which run on rf_conv_gemm):
 *   rf_lpips_prep_u8  : images u8 [B, H, W, 3] (image b at images + b * image_stride bytes; any H, W >= 1) -> out fp32 NHWC [B, H, W, 8]
 *                       (16-byte aligned): x = (float32(byte) / 255 - 0.5) / 0.5 (ToTensor + Normalize(0.5, 0.5): how the reference's datasets
 *                       bring images to [-1, 1]), then BaseNet.z_score (x - mean) / std with mean (-.030, -.088, -.188) and std
 *                       (.458, .448, .450) (networks.py:41-51); every step rounded to fp32 in that order.  Channels 0..2; zeros in 3..7 (the
 *                       stems' cin_pad = 8 layout).
 *   rf_lpips_prep_f32 : x fp32 NCHW [B, 3, H, W] (contiguous) -> the same z-score and layout (the module surface takes tensors in [-1, 1]).
 *   rf_maxpool2d      : x fp32 NHWC [B, H, W, C] (contiguous, 16-byte aligned, C a multiple of 4) -> out [B, (H - k) / 2 + 1, (W - k) / 2 + 1, C]:
 *                       MaxPool2d(k, stride 2), k = 2 or 3, no padding, floor mode (torchvision's vgg16 / alexnet features).  H, W >= k.
 *                       (rf_maxpool3x3s2 is the padding-1 pool of the ResNets.)
 *   rf_lpips_layer    : fx, fy fp32 NHWC [B, HW, C] (contiguous, 16-byte aligned; C a multiple of 4, 4 <= C <= 512; B <= 65535), w fp32 [C]
 *                       (16-byte aligned; the layer's `lin.<l>.1.weight`) -> vals[b * L + l] fp64 = mean over the HW pixels of
 *                       sum_c w[c] (n(fx)[c] - n(fy)[c])^2 with n(f) = f / (sqrt(sum_c f^2 + 1e-16) + 1e-10) (utils.py:6-8, lpips.py:32-33).
 *                       Each feature byte is read once; the direct form (normalise, subtract, square, weight), everything computed from
 *                       the fp32 features in fp64 (norms, differences, sums, the mean): near-equal maps keep their small difference.  No atomics: block partials go to `scratch` (fp64, at least
 *                       B * min(RF_LPIPS_MAX_BLOCKS, HW) entries; `scratch_doubles` is its size) and meet in a fixed order.  The blocks of a
 *                       pair depend on HW and C only: vals[b, l] has the same bits for every B and on every run.  A pixel whose channels are
 *                       all zero normalises to zeros; fx == fy gives exactly 0.
 *   rf_lpips_total    : vals fp64 [B, L] -> d fp64 [B] = sum_l vals[b, l] (l ascending) and totals fp64 [2] = (sum_b d[b], b ascending; B): the
 *                       reference's scalar is totals[0] / totals[1] (lpips.py:35).
 */
#define RF_LPIPS_MAX_BLOCKS 1024
int rf_lpips_prep_u8(const void* images_u8, int B, int H, int W, int64_t image_stride, float* out, void* stream);
int rf_lpips_prep_f32(const float* x_nchw, int B, int H, int W, float* out, void* stream);
int rf_maxpool2d(const float* x, int B, int H, int W, int C, int k, float* out, void* stream);
int rf_lpips_layer(const float* fx, const float* fy, int B, int64_t HW, int C, const float* w, double* scratch, int64_t scratch_doubles, double* vals,
                   int L, int l, void* stream);
int rf_lpips_total(const double* vals, int B, int L, double* d, double* totals, void* stream);
/* elementwise y = silu(x) on fp32 (emb path, openaimodel.py:219) */
int rf_silu_f32(const float* x, float* y, int64_t n, void* stream);

/*
 * PNG encoding of device-resident images (the CLIs' --gpu_png; reface_amd/pngenc.py wraps the result in the PNG signature and chunks).
 * The filtered stream of an image is cut into segments of RF_PNG_SEG bytes; a segment is coded without reference to any other and its bytes
 * land in a slot of RF_PNG_SLOT bytes (the stored worst case, segment + 5, rounded up to 16).  n is a stream's length in bytes and
 * nseg = ceil(n / RF_PNG_SEG); all streams of a call share n.
 *   rf_png_filter_u8        : images u8 [B, H, W, C], C = 1 | 3 | 4 (image b at images + b * image_stride, row y at + y * row_stride bytes)
 *                             -> out (stream b at out + b * out_stride): H rows of 1 + W * C bytes, the filter type then the filtered row.
 *                             None / Sub / Up / Average / Paeth in exact integer arithmetic; per row the filter with the smallest sum of
 *                             |residual as a signed byte| wins, ties to the lowest type.
 *   rf_png_deflate_segments : streams u8 (stream b at streams + b * stream_stride; any alignment) -> slots u8 [B, nseg, RF_PNG_SLOT] (16-byte
 *                             aligned), seg_bytes int32 [B, nseg] (the bytes written to each slot) and seg_adler uint32 [B, nseg] (the
 *                             segment's Adler-32 partial: sum of bytes | (sum of (len - i) * byte_i) << 16, each mod 65521).  Tokens as in
 *                             zlib's Z_RLE strategy (distance 1 only); one dynamic block per segment with a fixed-form header (HLIT = 29,
 *                             HDIST = 0, a complete 4-bit code-length code over 0..15); Huffman lengths by the two-queue construction over
 *                             leaves sorted by (count, symbol), the leaf taken on equal weight, counts halved (rounding up) while a code is
 *                             deeper than 15.  Every segment but the last ends with an empty stored block (byte aligned); the last one's block
 *                             carries BFINAL.  A segment that is not smaller than segment + 5 bytes this way is one stored block.
 *   rf_png_pack             : -> out u8 (stream b at out + b * out_stride, out_stride >= n + 5 * nseg + 6): the zlib header 78 01, the
 *                             segments back to back, the combined Adler-32; lengths int32 [B] = the stream's bytes.
 */
#define RF_PNG_SEG 32768
#define RF_PNG_SLOT 32784
int rf_png_filter_u8(const void* images_u8, int B, int H, int W, int C, int64_t image_stride, int64_t row_stride, void* out_u8, int64_t out_stride,
                     void* stream);
int rf_png_deflate_segments(const void* streams_u8, int B, int64_t n, int64_t stream_stride, void* slots_u8, int* seg_bytes, uint32_t* seg_adler,
                            void* stream);
int rf_png_pack(const void* slots_u8, const int* seg_bytes, const uint32_t* seg_adler, int B, int64_t n, void* out_u8, int64_t out_stride,
                int* lengths, void* stream);

/*
 * PNG decoding on the device (the callers' --gpu_png_decode; reface_amd/pngdec.py parses the chunks, uploads the IDAT bytes and raises the
 * error codes).  A batch is described by RF_PNGDEC_DESC int64 words per file, given twice: desc_host (read and range-checked by the entry
 * point before anything is launched) and desc (the same words in device memory, read by the kernels):
 *   0 comp_off, 1 comp_len   the file's zlib stream at comp + comp_off
 *   2 filt_off, 3 expect     its filtered stream at filt + filt_off (a multiple of 16); expect = H * (1 + W * bpp)
 *   4 H, 5 W, 6 bpp          bpp = 1 | 2 | 3 | 4 bytes per pixel (grey, grey + alpha, RGB, RGBA; 8 bits per sample, not interlaced)
 *   7 out_c                  channels written: bpp, or 1 | 3 from grey (+ alpha: dropped; the sample is replicated), or 3 from RGBA
 *   8 pix_off, 9 row_stride  the image's pixels at pix + pix_off, row y at + y * row_stride bytes
 *   10 cand_begin, 11 cand_count   the file's candidate piece starts: cand[cand_begin ...]; 0, or the stream start (offset 2) and the rest
 * status is int32 [B, 2]: the error code (0 = none; the codes of csrc/png_inflate.h) and the inflate plan taken (0 serial, 1 segments,
 * 2 blocks).
 *   rf_png_inflate     : zlib streams -> filtered streams.  Every read is bounded by comp_len, every write by expect, every distance by the
 *                        bytes produced so far; a damaged stream leaves an error code.  Serial plan: one wave per stream, the Huffman
 *                        symbols walked on wave-uniform values, the 32 KiB window and the tables in LDS, matches and stored blocks copied
 *                        by the whole wave.  Segmented plan, tried for files with cand_count >= 2: cand is int32 [2, ncand] (the file of
 *                        each candidate, ascending; then its offset in the file's stream, ascending per file; cand_host = the same words
 *                        on the host); one wave decodes each candidate into slots u8 [ncand, 32768] (16-byte aligned) up to an empty
 *                        stored block, a stored block that fills the slot, or the final block, and leaves pieces int32 [ncand, 5]
 *                        (end offset, bytes, Adler-32 partial as in rf_png_deflate_segments, flags, place in the chain).  A file is
 *                        taken from its pieces only if they chain up from offset 2 exactly: each usable (no error, no reference before its
 *                        own start), each but the last of 32768 bytes, each end offset a candidate, the total = expect and the combined
 *                        Adler-32 = the trailer; otherwise the serial kernel, enqueued behind, decodes it.  Candidates are hints only.
 *   rf_png_unfilter_u8 : filtered streams -> pixels (None / Sub / Up / Average / Paeth undone in exact integer arithmetic), one wave per
 *                        image, W <= 8192, H <= 2^20.  Files whose error code is set are skipped; a filter byte above 4 sets code 11.  status must
 *                        have been written by rf_png_inflate (or zeroed).
 *   rf_png_inflate_blocks : rf_png_inflate's sequence with the blocks plan (csrc/png_blocks.h) in front of the serial kernel, for the files
 *                        the caller names eligible (an opt-in: the plan only accepts a file; whatever it does not accept is decoded, and
 *                        its error code set, by the serial kernel behind it).  blk is int32 [3 B + nslot] (blk_host = the same words on the
 *                        host): per file the capacity in candidate slots (0 = not eligible; else >= 2, and comp_len < 2^28), its first
 *                        slot (the files' slots follow each other) and the first word of its candidate bitmap ((comp_len + 3) / 4 words
 *                        per eligible file, following each other); then the file of every slot.  bitmap is uint32 [bitmap_words], work
 *                        int32 [work_words >= 4 B + 11 nslot], marks uint16 [marks_count >= filt_bytes]: 2 bytes per output byte, at the
 *                        file's filt_off.  Five launches, no host round trip: search (one lane per bit offset of an eligible stream tests
 *                        whether a dynamic block header the serial plan would accept starts there; the bit behind the zlib header is
 *                        candidate 0 whatever stands there; a file with more hits than slots is not accepted), count (one wave per
 *                        candidate walks whole blocks to the next block boundary that is a candidate), chain (one thread per file, from
 *                        candidate 0 along the end bits: every chunk usable, the last one final, the total = expect, at least 2 chunks),
 *                        decode (one wave per chain chunk writes 16-bit symbols: a byte, or 256 + j = byte j of the 32 KiB in front of
 *                        the chunk), resolve (one workgroup per file, chunk by chunk; a marker in front of the stream's first byte or an
 *                        Adler-32 other than the trailer's rejects the file).  Files the segmented plan accepted are skipped.  After the
 *                        call work[4 f .. 4 f + 1] = the dynamic headers found in file f (candidate 0 not counted) and its chain length.
 */
#define RF_PNGDEC_DESC 12
int rf_png_inflate(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* filt_u8, int64_t filt_bytes,
                   const int* cand_host, const int* cand, int ncand, void* slots_u8, int* pieces, int* status, void* stream);
int rf_png_inflate_blocks(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* filt_u8, int64_t filt_bytes,
                          const int* cand_host, const int* cand, int ncand, void* slots_u8, int* pieces, int* status, const int* blk_host, const int* blk,
                          int nslot, void* bitmap_u32, int64_t bitmap_words, int* work, int64_t work_words, void* marks_u16, int64_t marks_count,
                          void* stream);
int rf_png_unfilter_u8(const void* filt_u8, int64_t filt_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* pix_u8, int64_t pix_bytes,
                       int* status, void* stream);

/*
 * Baseline JPEG encoding of device-resident images (scripts/inference_swap_video.py --write_video; reface_amd/mjpeg.py puts SOI .. SOS in
 * front of the result).  All arithmetic is 32-bit integer and restates libjpeg's: the scan is byte for byte the one libjpeg writes with the
 * same tables and one restart interval per MCU row.  subsampling is 420 (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr) or 444 (MCU 8 x 8: Y Cb Cr);
 * mcu_rows = ceil(H / MCU height), mcus = ceil(W / MCU width), nbr = mcus * blocks per MCU.  1 <= H, W <= 65535.
 *   rf_jpeg_blocks_u8 : images u8 [B, H, W, C], C = 3 | 4 (the 4th byte is ignored; image b at images + b * image_stride, row y at
 *                       + y * row_stride bytes) -> coef int16 [B, mcu_rows, 64, nbr]: element [z][j] of a tile is the quantised
 *                       coefficient at zigzag position z of block j of the MCU row, blocks in scan order -- coefficient-major, so that
 *                       the one-lane-per-block kernels on both sides touch it coalesced.  rgb_ycc_convert (16-bit fixed point), every
 *                       component edge-replicated to its size in blocks; at 420 the full-resolution chroma is edge-replicated, averaged
 *                       over 2 x 2 with the bias 1 (even output columns) / 2 (odd), and the downsampled plane's last row replicated down;
 *                       jfdctint ("islow", CONST_BITS 13, PASS1_BITS 2) on samples - 128; c = sign(d) * ((|d| + 4 q) / (8 q)).  quant is
 *                       int32 [2, 64] on the device: the luma and chroma tables in zigzag order.  Dummy blocks (past a component's size
 *                       in blocks, inside the last MCU column / row) carry the DC of the block before them in the MCU and no AC.
 *   rf_jpeg_entropy   : coef -> slots u8 [B, mcu_rows, slot_stride] and seg_bytes int32 [B, mcu_rows]: every MCU row is one restart
 *                       interval, coded from DC predictors of 0: DC difference category + amplitude bits, AC (run, size) symbols with ZRL
 *                       and EOB, bits most significant first, 00 behind every FF byte, the tail padded with 1-bits.  huff is uint32
 *                       [2, 272] on the device: per table class (luma, chroma) 16 DC then 256 AC entries, (code << 5) | length.
 *                       slot_stride >= RF_JPEG_SLOT(nbr), the bound for ANY coefficients and tables (values are clamped to the 8-bit
 *                       range of categories, lengths to 16): no input overflows a slot.
 *   rf_jpeg_pack      : -> out u8 (image b at out + b * out_stride, out_stride >= mcu_rows * (slot_stride + 2), below 2^31): the intervals
 *                       back to back, FF D0+(i mod 8) behind interval i, FF D9 behind the last; lengths int32 [B] = the bytes written.
 */
#define RF_JPEG_BLOCK_BITS (64 * 27)
#define RF_JPEG_SLOT(nbr) (2 * (((int64_t)(nbr) * RF_JPEG_BLOCK_BITS + 7) / 8 + 1))
#define RF_JPEG_HUFF_WORDS (2 * 272)
int rf_jpeg_blocks_u8(const void* images_u8, int B, int H, int W, int C, int64_t image_stride, int64_t row_stride, int subsampling, const int* quant,
                      int16_t* coef, void* stream);
int rf_jpeg_entropy(const int16_t* coef, int B, int mcu_rows, int mcus, int subsampling, const uint32_t* huff, void* slots_u8, int64_t slot_stride,
                    int* seg_bytes, void* stream);
int rf_jpeg_pack(const void* slots_u8, int64_t slot_stride, const int* seg_bytes, int B, int mcu_rows, void* out_u8, int64_t out_stride, int* lengths,
                 void* stream);

/*
 * Baseline JPEG decoding on the device (the callers' --gpu_jpeg_decode and --video_in; reface_amd/jpegdec.py parses the markers, builds the
 * tables, uploads the scans and raises the error codes).  8-bit sequential Huffman (SOF0), one interleaved scan, 1 component or 3 (YCbCr,
 * luma sampled 1x1, 2x1 or 2x2 against chroma 1x1), H, W <= RF_JPEGDEC_MAX_SIDE.  A batch is described by RF_JPEGDEC_DESC int64 words per
 * file, given twice: desc_host (read and range-checked by the entry point before anything is launched) and desc (the same words in device
 * memory, read by the kernels):
 *   0 scan_off, 1 scan_len   the entropy-coded bytes behind the SOS header up to EOI, at comp + scan_off
 *   2 H, 3 W, 4 ncomp        ncomp = 1 | 3
 *   5 hs, 6 vs               the luma sampling factors (1 | 2; 1 x 2 is not taken); chroma is 1 x 1
 *   7 ri                     MCUs per restart interval, 0 = no DRI
 *   8 coef_off               the file's first block in coef; its blocks follow in scan order (per MCU: hs * vs luma blocks, Cb, Cr)
 *   9 plane_off              its component planes at planes + plane_off (a multiple of 16): Y, Cb, Cr, each padded to whole MCUs
 *   10 out_c                 channels written: 3, or 1 for a 1-component file (which is replicated when out_c = 3)
 *   11 pix_off, 12 row_stride   the image's pixels at pix + pix_off, row y at + y * row_stride bytes
 *   13 tab_off               its tables at comp + tab_off (a multiple of 16), RF_JPEGDEC_TABLE_BYTES: 4 quantisation tables of 64 uint16
 *                            in natural order, then 4 DC and 4 AC Huffman tables of 912 bytes (csrc/jpeg_decode.h: HuffTab); files may share
 *   14 ivl_begin, 15 ivl_count   its intervals: ivl[ivl_begin ...]
 *   16 tq, 17 td, 18 ta      the quantisation / DC / AC table number (0 .. 3) of component c in bits 8 c .. 8 c + 7
 *   19 ss_begin, 20 ss_count, 21 ss_bytes, 22 ss_wg_begin   the selfsync plan (below); all 0 in a file that does not take it.  23 is spare (0)
 * status is int32 [B, 2]: the error code (0 = none; the codes of csrc/jpeg_decode.h) and, in bits 0 .. 1, the plan (0: one lane decodes
 * the whole scan, 1: one lane per restart interval, 2: selfsync), in bit 2 the selfsync plan's fallback flag, in bits 8 .. 15 its launches.
 *   rf_jpeg_entropy_decode  : scans -> coef int16 [coef_blocks, 64], natural (de-zigzagged) order, zero-filled here.  ivl is int32
 *                             [2, nivl] (the file of each interval, ascending; then the offset of its first byte in the file's scan: 0 for
 *                             the first, 2 behind every FF D0..D7 for the others; ivl_host = the same words on the host).  One lane per
 *                             interval, DC predictors 0 at its start; `lanes` (1 .. 64) lanes of every wave are used.  A file must hold
 *                             ceil(MCUs / ri) intervals and the marker in front of interval k must be RST((k - 1) mod 8); every read is
 *                             bounded by the interval's end, every write by its block range, every loop by blocks * 64 iterations; an
 *                             invalid code, a coefficient index past 63 and running out of data are error codes.  A lane that meets an
 *                             error stops and leaves its code (the first one of a file stays); the others are unaffected.  Writes status.
 *   rf_jpeg_idct_u8         : coef -> planes u8: dequantisation and libjpeg's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2; the result
 *                             + 128 clamped to 0 .. 255, which equals libjpeg's masked range-limit table for any file made from pixels).
 *   rf_jpeg_upsample_rgb_u8 : planes -> pixels: libjpeg's fancy (triangle) h2v1 / h2v2 chroma upsampling with the edges of the real
 *                             downsampled plane, and its 16-bit-table YCbCr -> RGB.  Files whose error code is set are skipped by both.
 */
#define RF_JPEGDEC_DESC 24
#define RF_JPEGDEC_TABLE_BYTES (512 + 8 * 912)
#define RF_JPEGDEC_MAX_SIDE 8192
int rf_jpeg_entropy_decode(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, const int* ivl_host,
                           const int* ivl, int nivl, int lanes, int16_t* coef, int64_t coef_blocks, int* status, void* stream);
/*
 * The self-synchronising plan (csrc/jpeg_sync.h) for files without DRI whose scan holds at least 2 * ss_bytes bytes: the scan is cut into
 * ss_count = ceil(scan_len / ss_bytes) sub-sequences of ss_bytes (16 .. 65536) bytes, one lane each, 64 to a workgroup; ss_begin / ss_wg_begin
 * are the file's first sub-sequence / workgroup among those of the batch (files in order, no gaps).  rf_jpeg_entropy_decode leaves such a
 * file alone; rf_jpeg_selfsync_decode, called behind it on the same stream with the same arguments, decodes it to the same coefficients and
 * the same error code.  `launches` (1 .. 16) sync launches iterate the lanes' start states towards their fixed point, which holds the
 * serial decoder's own states; a file whose last launch still moved a workgroup boundary is decoded by the serial lane in a launch appended
 * here (status word 1: plan 0 and the fallback flag), so the result never depends on `launches`.  `work` is device scratch of
 * rf_jpeg_selfsync_work_bytes(sum of ss_count, sum of ceil(ss_count / 64), B) bytes, initialised here.  `stages` selects what is enqueued
 * (RF_JPEGDEC_SS_ALL; the parts alone, in ascending order, for a caller that times them).
 */
#define RF_JPEGDEC_SS_SYNC 1
#define RF_JPEGDEC_SS_SCAN 2
#define RF_JPEGDEC_SS_WRITE 4
#define RF_JPEGDEC_SS_DC 8
#define RF_JPEGDEC_SS_SERIAL 16
#define RF_JPEGDEC_SS_ALL 31
int64_t rf_jpeg_selfsync_work_bytes(int64_t subseqs, int64_t workgroups, int B);
int rf_jpeg_selfsync_decode(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, const int* ivl_host,
                            const int* ivl, int nivl, int lanes, int launches, int stages, void* work, int64_t work_bytes, int16_t* coef,
                            int64_t coef_blocks, int* status, void* stream);
int rf_jpeg_idct_u8(const int16_t* coef, int64_t coef_blocks, const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc,
                    int B, void* planes_u8, int64_t plane_bytes, const int* status, void* stream);
int rf_jpeg_upsample_rgb_u8(const void* planes_u8, int64_t plane_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* pix_u8,
                            int64_t pix_bytes, const int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REFACE_HIP_H */
