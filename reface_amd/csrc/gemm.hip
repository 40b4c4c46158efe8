// Implicit-GEMM convolution / linear layer on the gfx950 matrix cores.
//
//   out[m, n] = act(alpha * sum_k A[m, k] W[n, k] + bias[n] + rowvec[sample(m), n]) + residual[m, n]
//   (RF_ACT_ADD_RELU alone acts after the residual: out = relu(alpha * sum + bias + rowvec + residual), direct and staged epilogues, no split-K)
//
// One kernel template serves both storage types through a common *byte* geometry: a K-tile is
// 128 bytes of K per row (64 bf16 or 32 fp32), LDS rows are 128 B with a 16-B-slot XOR swizzle,
// every lane feeds the MFMA from one 16-B fragment (lane l: row l&31, slot 2*kk + (l>>5)):
//   bf16 : 1 x v_mfma_f32_32x32x16_bf16 per fragment pair (8 k per lane-half)
//   fp16 : 1 x v_mfma_f32_32x32x16_f16  -- the same kernels instantiated for f16_t (RF_F16, the "fp16" throughput mode): identical geometry and
//          matrix-core rate, 11 significant bits per operand instead of 8; no fp8-weight (W8) and no split-operand (x3) variants
//   fp32 : 4 x v_mfma_f32_32x32x2_f32   per fragment pair (exact fp32 FMA chain, 157 TF peak)
// The A operand is gathered on the fly from channels-last source tensors (3x3 / 1x1, stride, asymmetric padding, nearest x2
// upsample folded into the addressing, 2-source channel concat).  Hot path (GLDS): both operands go global -> LDS directly
// (buffer_load_dwordx4 ... lds, no staging registers; the XOR swizzle is applied on the SOURCE side), two LDS stages, the pieces
// of tile kt+2 issued right behind the barrier that retires tile kt, a register-level fragment pipeline under the MFMAs.  Shapes the
// DMA cannot express (two sources, K tiles straddling a filter tap, fp32 operands with ragged K) take the register-staged loop
// (global -> registers -> LDS, next tile's loads issued before the current tile's MFMAs).  Epilogues: see the EPI parameter.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "gemm_plan.h"          // GemmParams, the tiles and the planner: host-only C++ (this file launches what it plans)

// The LDS-DMA pieces of tile kt+2 are issued between the MFMA columns of k-step 3, behind the barrier that frees their stage: the issue
// slots hide under the matrix pipe.  Issue orders measured against it (same-box A/B on the whole benchmark, r03):
//   one burst (both waves of every SIMD stall on ~9 x 60-180 issue cycles at the same time)        935.9 / 933.6 ms per batch
//   between the MFMA columns of k-step 3 (kept)                                                     921.4 / 920.0
//   as kept with the barrier ahead of all of k-step 3's columns                                    920.4 / 920.5 (vs 921.5 / 921.6 for the kept order on that box)
//   in thirds over k-step 3 and k-steps 0 / 1 of the next tile                                      965.3 / 964.1 (vs 939.9 / 937.0 for the kept order on that box)

namespace rf {
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// struct GemmParams, the kernels' argument block: gemm_plan.h

// 8 fp8 (e4m3fn) weights -> 8 bf16, times the row's power-of-two scale: v_cvt_scalef32_pk_bf16_fp8, one instruction per pair (exact:
// 3 mantissa bits fit in bf16's 7, a power-of-two scale only moves the exponent)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v_t;
__device__ __forceinline__ u32x4_t fp8x8_to_bf16x8(const u32x2_t& r, float scale) {
    u32x4_t o;
    o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[0], scale, false));
    o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[0], scale, true));
    o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[1], scale, false));
    o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[1], scale, true));
    return o;
}

template <typename T> struct MmaFrag;
template <> struct MmaFrag<bf16_t> {
    __device__ static __forceinline__ void mma(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct MmaFrag<f16_t> {
    __device__ static __forceinline__ void mma(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) { mma16<f16_t>(acc, a, b); }
};
template <> struct MmaFrag<fp8_t> {      // (the fp8 x fp8 path has its own main loop with block scales; this keeps the shared lambdas well-formed)
    __device__ static __forceinline__ void mma(f32x16_t&, const u32x4_t&, const u32x4_t&) {}
};
typedef int v8i_t __attribute__((ext_vector_type(8)));
// acc += (A row block, 64 K) x (B row block, 64 K)^T on the MX-scaled fp8 MFMA: each lane supplies 32 bytes per operand -- 16-byte slots h and
// 2 + h of the 64-byte K slice (h = lane >> 5) -- and ONE E8M0 scale per operand in byte 0 of sa / sb, which the hardware applies to the
// 32 consecutive K elements [32 h, 32 h + 32) of that lane's row (tools/mx_probe2.py pins this mapping on the chip)
__device__ __forceinline__ void mma_mx8(f32x16_t& acc, const u32x4_t& a0, const u32x4_t& a1, int sa, const u32x4_t& b0, const u32x4_t& b1, int sb) {
    const v8i_t a = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
    const v8i_t b = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
    // inline asm, volatile: as a builtin (a pure call) hipcc sinks all MFMAs of a K tile to the end of the loop body, past every fragment
    // load and the barrier -- three fragment sets live (256 VGPRs + scratch) and no LDS latency hidden under the matrix pipe.  Volatile
    // statements keep their order against each other and against the loop's wait / barrier statements.  (s_nop 1: wait states between a
    // VALU write of a scale / operand register and the MFMA that reads it, which the compiler does not pad inside asm.)
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]" : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(sb));
}
template <> struct MmaFrag<float> {
    __device__ static __forceinline__ void mma(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as_f32( a[q]), as_f32( b[q]), acc, 0, 0, 0);
    }
};

// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for vmcnt(0), i.e. for every outstanding
// global store to be acknowledged (~1-2 us each time in the chunked epilogue)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ int lds_off(int row, int slot) { return row * 128 + ((slot ^ ((row >> 1) & 7)) << 4); }

template <bool W8> __device__ __forceinline__ int w_stage(int t, int buf) { return W8 ? ((t >> 1) & 1) : buf; }
template <bool W8> __device__ __forceinline__ int w_soff(int t) { return (W8 ? (t >> 1) : t) * 128; }

template <typename TO> __device__ __forceinline__ void store_out(TO* p, float v);
template <> __device__ __forceinline__ void store_out<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_out<bf16_t>(bf16_t* p, float v) { *p = f2bf(v); }
template <> __device__ __forceinline__ void store_out<f16_t>(f16_t* p, float v) { *p = (f16_t)v; }
template <typename TO> __device__ __forceinline__ float load_out(const TO* p);
template <> __device__ __forceinline__ float load_out<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float load_out<bf16_t>(const bf16_t* p) { return bf2f(*p); }
template <> __device__ __forceinline__ float load_out<f16_t>(const f16_t* p) { return (float)*p; }
// 16-bit storage element (bf16 or fp16): the forms that differ only in their conversions share one code path
template <typename X> struct is16 { static constexpr bool value = std::is_same<X, bf16_t>::value || std::is_same<X, f16_t>::value; };

// EPI = 1: "direct" epilogue.  The MFMA operands are swapped (W fragment as the row operand, A fragment as the column operand)
// and the W rows of each 32-row block are read in the order  row(i') = 16*((i'>>2)&1) + 4*(i'>>3) + (i'&3), so that lane
// (m = l & 31, h = l >> 5) ends up with accumulator register r = output column 16*h + r of its row: 16 CONTIGUOUS columns per
// 32x32 block.  Bias / timestep vector / residual / GEGLU then happen in registers and every lane writes its row segments with 16-byte
// stores -- no staging pass of the tile through LDS (only the BN column constants are parked there, one barrier), and the waves
// retire independently.
// W8 = true: the weights are fp8 (e4m3fn) with one power-of-two scale per output channel.  A W tile in LDS keeps the 128-byte row
// geometry and therefore holds 128 K elements = the W operand of TWO consecutive A tiles: the W pieces are issued every other
// tile (half the weight bytes through L2 / LDS), and a W fragment is an 8-byte LDS read turned into 8 bf16 by 4 conversions
// (issued between the MFMAs of the previous fragment column).  The MFMA itself is the bf16 one: same matrix-core ceiling.
// LNF: LayerNorm role of the launch (rf_conv_gemm_desc.ln_*), a compile-time variant of the direct epilogue so that ordinary launches carry none
// of its registers: 0 none, 1 producer (row statistics of the stored output), 2 consumer (row affine; such launches have no residual)
// HX (round 4): 3x3 stride-1 convolutions with the K order (filter row dy, channel chunk, filter column dx) -- rf_conv_gemm_desc.korder = 2.  The three
// horizontal taps of one (dy, chunk) read the SAME image rows shifted by one pixel, so ONE row-extended A tile -- every image row of the output tile
// with one halo pixel on each side, (BM / Wout) * (Wout + 2) rows of 128 bytes -- is staged per group of three K tiles instead of one BM-row tile per
// K tile: a third of the A-operand fill (the per-CU operand fill is what caps these kernels).  Fragment reads address row  erow(pixel) + dx  of that
// tile (the XOR swizzle follows the row), the W side and everything behind the main loop are unchanged.
template <typename T, typename TO, int WM, int WN, int TM, int TN, bool CONV, bool GLDS, int NST, int EPI = 0, bool W8 = false, int LNF = 0, bool HX = false>
__global__ __launch_bounds__(WM* WN * 64) void conv_gemm_kernel(const GemmParams p) {
    static_assert(LNF == 0 || (EPI == 1 && !CONV && !W8 && sizeof(T) == 2 && sizeof(TO) == 2), "LayerNorm folding: bf16 linear layers on the direct epilogue");
    static_assert(!HX || (CONV && GLDS && NST == 2 && sizeof(T) == 2 && !W8), "row-extended A tiles: bf16 3x3 convolutions on the two-stage direct-to-LDS loop");
    static_assert(EPI == 0 || GLDS, "the direct epilogue is built on the direct-to-LDS main loop");
    static_assert(!W8 || (GLDS && std::is_same<T, bf16_t>::value), "fp8 weights: bf16 activations on the direct-to-LDS main loop");
    // A8: fp8 (e4m3fn) activations with one E8M0 scale per 32 channels x fp8 weights with one power-of-two scale per output channel on
    // v_mfma_scale_f32_32x32x64_f8f6f4: a K tile (128-byte rows) holds 128 K elements, two k-steps of 64
    constexpr bool A8 = std::is_same<T, fp8_t>::value;
    static_assert(!A8 || (GLDS && !W8 && NST == 2), "fp8 activations: direct-to-LDS main loop, two stages");
    constexpr int NT = WM * WN * 64;
    constexpr int BM = 32 * TM * WM;
    constexpr int BN = 32 * TN * WN;
    constexpr int VEC = elem<T>::VEC;
    constexpr int BK = 8 * VEC;          // elements of K per tile (128 bytes)
    constexpr int RPP = NT / 8;          // rows covered per staging pass
    constexpr int AXR = HX ? ((BM * 5 / 4 + RPP - 1) / RPP) * RPP : BM;      // rows of an A stage (HX: up to BM + 2 BM / Wout rows, Wout >= 8)
    constexpr int AV = AXR / RPP;        // A vectors per thread
    constexpr int BV = BN / RPP;         // B vectors per thread
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile/threads mismatch");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const ldsA = smem;                       // [2][AXR][128]
    char* const ldsB = smem + NST * AXR * 128;     // [NST][BN][128]
    char* const ldsS = smem + NST * (AXR + BN) * 128;     // A8: [2][8 waves][64 rows] scale dwords (4 E8M0 bytes = the 4 blocks of a K tile)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware tile order: XCD x (= block id mod 8 as dispatched) owns a contiguous run of tiles,
    // N-fastest inside the run, so the N-tiles that share an A panel hit the same L2.
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    // ... in 2-D patches: the ~32 tiles an XCD works on at any time (one block per CU) form a pm x pn patch, so that they share pm A panels and
    // pn W panels (a strip of 32 tiles along N touches every W panel of a wide layer: more than the 4 MB of L2 hold, re-streamed from the
    // Infinity Cache at ~7 TB/s -- tools/fill_probe.py: 11 B/clk/CU against 50 for L2 hits)
    int tile_m, tile_n;
    {
        const int srow = p.pm * p.tiles_n;                           // tiles per super-row of pm tile rows
        const int sr = bid / srow, rem = bid - sr * srow;
        const int h = min(p.pm, p.tiles_m - sr * p.pm);              // (the last super-row may be shorter)
        const int pw = h * p.pn;
        const int pc = rem / pw, r2 = rem - pc * pw;
        const int c = r2 / h;
        tile_m = sr * p.pm + (r2 - c * h);
        tile_n = pc * p.pn + c;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const long long zb = blockIdx.y;
    const T* src0 = (const T*)p.src0 + zb * p.sA;
    const T* src1 = (const T*)p.src1;
    const T* Wp = W8 ? (const T*)((const char*)p.W + zb * p.sW) : (const T*)p.W + zb * p.sW;
    if (!W8 && p.w_ps) Wp += (long long)(m0 / p.rows_per_sample) * p.w_ps;          // (a tile lies inside one sample: host)
    // ups == 2 (nearest-2x upsampling folded into 2x2 phase weights): rows are ordered (sample, phase = 2 py + px, source pixel) and a tile lies
    // inside one phase of one sample (host: Hin Win % BM == 0), so the phase, its padding (1 - py, 1 - px) and its weights W[phase] are block-uniform
    const int hw_in = p.Hin * p.Win;
    const int uph = (CONV && p.ups == 2) ? (m0 / hw_in) & 3 : 0;
    if (!W8 && uph) Wp += (long long)uph * p.N * p.ldw;
    const bool up2 = CONV && p.ups == 2;
    const int pad_t = up2 ? 1 - (uph >> 1) : p.pad_t, pad_l = up2 ? 1 - (uph & 1) : p.pad_l;
    // row of `out` that GEMM row `row` of this tile writes: the row itself, or (ups == 2) pixel (2 i + py, 2 j + px) of its sample
    auto out_row = [&](int row) -> int {
        if (!up2) return row;
        const int s4 = m0 / (4 * hw_in), r = row - (s4 * 4 + uph) * hw_in;
        const int i = r / p.Win, j = r - i * p.Win;
        return (s4 * p.Hout + 2 * i + (uph >> 1)) * p.Wout + 2 * j + (uph & 1);
    };

    // EPI 1: the per-column constants of this tile (bias + the tile's timestep / context vector) are fetched NOW, one column per
    // thread, and parked in LDS after the main loop: fetched in the epilogue they cost one exposed L2 / HBM round trip per
    // 32-column block (5 per tile: 25 of the 60 us of the 65536x960x320 qkv GEMM, no-store timing experiment r02g)
    float colc = 0.f;
    if constexpr (EPI == 1) {
        if (tid < BN && n0 + tid < p.N && p.splitk == 1) {
            if (p.bias) colc = p.bias[n0 + tid];
            if (p.rowvec) colc += p.rowvec[(long long)(m0 / p.rows_per_sample) * p.ldv + n0 + tid];
        }
    }
    float colu = 0.f;          // LayerNorm consumer: sum_k W[n, k] of this thread's column (the mean's coefficient)
    if constexpr (LNF == 2) {
        if (tid < BN && n0 + tid < p.N) colu = p.ln_u[n0 + tid];
    }
    const int r0 = tid >> 3;
    // GLDS: the LDS image of a direct-to-LDS load is lane-linear, so the XOR swizzle moves to the SOURCE: the lane that
    // lands on 16-byte position p of row r fetches k-slot p ^ ((r >> 1) & 7)  (r0 + 32*i keeps (r >> 1) & 7 for every i)
    const int slot = GLDS ? ((tid & 7) ^ ((r0 >> 1) & 7)) : (tid & 7);

    // ---- per-thread A row descriptors
    int a_pix[AV];     // CONV: b*Hin*Win ; plain: row index (or -1 invalid)
    int a_iy[AV], a_ix[AV];
#pragma unroll
    for (int i = 0; i < AV; ++i) {
        const int m = m0 + r0 + i * RPP;
        if (CONV) {
            const int hw = p.Hout * p.Wout;
            const int b = m / hw, rem = m - b * hw;
            const int oy = rem / p.Wout, ox = rem - oy * p.Wout;
            a_pix[i] = (m < p.M) ? b * p.Hin * p.Win : -1;
            a_iy[i] = oy * p.stride - p.pad_t;
            a_ix[i] = ox * p.stride - p.pad_l;
        } else {
            a_pix[i] = (m < p.M) ? m : -1;
            a_iy[i] = a_ix[i] = 0;
        }
    }
    // running K position of this thread's vector slot
    int kvec = slot * VEC;       // element index along K
    int cv = kvec, ky = 0, kx = 0;   // CONV: channel within tap, tap coords
    if (CONV) {
        while (cv >= p.Ctot) {
            cv -= p.Ctot;
            if (++kx == p.KW) { kx = 0; ++ky; }
        }
    }
    const int Hv = p.ups == 1 ? p.Hin * 2 : p.Hin, Wv = p.ups == 1 ? p.Win * 2 : p.Win;          // (ups == 2 addresses the stored grid)

    // advance this thread's K position to the next K tile
    auto advance_k = [&]() {
        kvec += BK;
        if (CONV) {
            if (p.korder) {       // channel-chunk-major K: the KH*KW taps of one BK-channel chunk are consecutive tiles
                if (++kx == p.KW) { kx = 0; if (++ky == p.KH) { ky = 0; cv += BK; } }
            } else {
                cv += BK;
                while (cv >= p.Ctot) {
                    cv -= p.Ctot;
                    if (++kx == p.KW) { kx = 0; ++ky; }
                }
            }
        }
    };

    u32x4_t ra[AV], rb[BV];

    auto load_tiles = [&]() {
        const bool kval = kvec < p.K;
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (CONV) {
                int iy = a_iy[i] + ky, ix = a_ix[i] + kx;
                const bool ok = kval && a_pix[i] >= 0 && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                if (ok) {
                    if (p.ups) { iy >>= 1; ix >>= 1; }
                    const long long pix = (long long)a_pix[i] + iy * p.Win + ix;
                    const T* ptr = (cv < p.C0) ? src0 + pix * p.ld0 + cv : src1 + pix * p.ld1 + (cv - p.C0);
                    v = *(const u32x4_t*)ptr;
                }
            } else {
                if (kval && a_pix[i] >= 0) v = *(const u32x4_t*)(src0 + (long long)a_pix[i] * p.ld0 + kvec);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int j = 0; j < BV; ++j) {
            const int n = n0 + r0 + j * RPP;
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (kval && n < p.N) v = *(const u32x4_t*)(Wp + (long long)n * p.ldw + kvec);
            rb[j] = v;
        }
        // advance to the next K tile
        advance_k();
    };
    auto store_tiles = [&](int buf) {
        char* a = ldsA + buf * BM * 128;
        char* b = ldsB + buf * BN * 128;
#pragma unroll
        for (int i = 0; i < AV; ++i) *(u32x4_t*)(a + lds_off(r0 + i * RPP, slot)) = ra[i];
#pragma unroll
        for (int j = 0; j < BV; ++j) *(u32x4_t*)(b + lds_off(r0 + j * RPP, slot)) = rb[j];
    };

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    int nk = (p.K + BK - 1) / BK;
    int kb0_tiles = 0;       // first K tile of this block (split-K)
    if (p.splitk > 1) {          // this block's K-tile range [kb0, kb0 + nk)
        int per = (nk + p.splitk - 1) / p.splitk;
        if (p.x3 || HX) per = (per + 2) / 3 * 3;          // whole groups of three tiles (split-bf16 passes / the three dx taps of an HX group)
        const int kb0 = blockIdx.z * per;
        nk = max(0, min(nk, kb0 + per) - kb0);
        kb0_tiles = kb0;
        if (!GLDS)
            for (int i = 0; i < kb0; ++i) advance_k();
    }
    // K-tile counts are wave-uniform, but hipcc's divergence analysis does not see it through the split-K arithmetic: everything derived from
    // them (the issue state, the SGPR offsets of the LDS-DMA pieces, the `more` conditions) would live in VGPRs, every DMA piece would sit in a
    // waterfall loop (v_readfirstlane / v_cmp / s_and_saveexec / branch: ~10 instructions and a serialisation point per piece, nine pieces per
    // tile right behind the barrier) and every `if (more)` would be an exec-masked region
    nk = __builtin_amdgcn_readfirstlane(nk);
    kb0_tiles = __builtin_amdgcn_readfirstlane(kb0_tiles);
    const int lrow = lane & 31, lhalf = lane >> 5;

    auto compute_tile = [&](int buf) {
        const char* a = ldsA + buf * BM * 128;
        const char* b = ldsB + buf * BN * 128;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int s = kk * 2 + lhalf;
            u32x4_t fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *(const u32x4_t*)(a + lds_off((wm * TM + i) * 32 + lrow, s));
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *(const u32x4_t*)(b + lds_off((wn * TN + j) * 32 + lrow, s));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) MmaFrag<T>::mma(acc[i][j], fa[i], fb[j]);
        }
    };

    if constexpr (GLDS) {
        // Direct global -> LDS staging (buffer_load_dwordx4 ... lds) with a register-level fragment pipeline.
        // Host guarantees (launch_typed): one source, K % BK == 0 and, for convs, Ctot % BK == 0 with tap-major K -- so a K tile
        // lies inside ONE filter tap and all of its addresses are  per-lane offset (fixed within a tap) + uniform K offset
        // (SGPR soffset).  Out-of-range rows / padding taps carry an out-of-range voffset: the buffer range check returns zeros.
        // XT: a centre-tap tail source may follow the window's K tiles (GemmParams.srcx): from tile xt0 on the A pieces come from srcx -- its own
        // buffer resource, per-lane offsets of the output pixel (computed once, on entering the tail), the usual SGPR K offset per tile.  All of
        // the tail's state is wave-uniform; launches without a tail (xt0 beyond every tile) run the loop as it was.
        constexpr bool XT = CONV && is16<T>::value && !W8;
        const int xt0 = XT ? p.xt0 : 0x7fffffff;
        __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)src0, 0, p.a_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Wp, 0, p.w_bytes, 0x00020000);
        constexpr int OOB = 0x7fffffff;
        constexpr int NP = AV + BV;
        static_assert(NP <= 20, "piece table too small");
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        const int lane_k = slot * VEC * (int)sizeof(T);       // byte offset of this lane's 16-byte K slot inside a K tile
        int offs[20];        // [0, AV): A pieces, [AV, NP): B pieces (fixed size: see the note on hipcc at `rowd`)
        unsigned rowd[8];    // CONV: packed (sample << 20 | oy << 10 | ox) of this thread's A rows, ~0u = row beyond M
        static_assert(AV <= 8, "row table too small");
        // A8: lane l of wave w also fetches the scale dword of tile row 64 w + l (one 4-byte piece per wave and K tile)
        const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)(A8 ? p.ascale : (const void*)src0), 0, A8 ? p.as_bytes : 0u, 0x00020000);
        unsigned srowd = ~0u;
        int soffs = OOB;
        if constexpr (A8) {
            static_assert(BM <= NT, "one scale row per thread");
            const int srow = wave_u * 64 + lane, m = m0 + srow;
            const bool sv = srow < BM && m < p.M;
            if (CONV) {
                const int hw = p.Hout * p.Wout;
                const int b = m / hw, rem = m - b * hw;
                const int oy = rem / p.Wout, ox = rem - oy * p.Wout;
                srowd = sv ? ((unsigned)b << 20 | (unsigned)oy << 10 | (unsigned)ox) : ~0u;
            } else {
                soffs = sv ? m * p.as_ld : OOB;
            }
        }
#pragma unroll
        for (int j = 0; j < BV; ++j) {
            const int n = n0 + r0 + j * RPP;
            offs[AV + j] = n < p.N ? n * p.ldw * (W8 ? 1 : (int)sizeof(T)) + lane_k : OOB;
        }
        // W8: W tile of A tile `t` = 128-byte tile (t >> 1) of the weight rows, kept in W stage ((t >> 1) & 1)
        // the W pieces of the first tile go out before the A row descriptors (two integer divisions per row) are computed
        if (nk > 0) {
            // (values computed OUTSIDE the builtin's argument list: a call expression inside it makes hipcc's host pass drop the
            // kernel's stub without a diagnostic)
            char* const b0 = ldsB + w_stage<W8>(kb0_tiles, 0) * BN * 128 + wave_u * 1024;
            const int so0 = __builtin_amdgcn_readfirstlane(w_soff<W8>(kb0_tiles));
#pragma unroll
            for (int j = 0; j < BV; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(b0 + j * (RPP * 128)), 16, offs[AV + j], so0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int m = m0 + r0 + i * RPP;
            if constexpr (HX) {
                // row j of the row-extended tile = image row (m0 / Wout + j / (Wout + 2)) over all samples, column code xc = j % (Wout + 2)
                // (input column xc - 1: the halo pixels are xc = 0 and xc = Wout + 1)
                const int j = r0 + i * RPP, we = p.Wout + 2;
                const int ir = j / we, xc = j - ir * we;
                const int R = m0 / p.Wout + ir;                       // (host: BM % Wout == 0, so m0 is the first pixel of an image row)
                const int b = R / p.Hout, oy = R - b * p.Hout;
                rowd[i] = (ir < BM / p.Wout && R * p.Wout < p.M) ? ((unsigned)b << 20 | (unsigned)oy << 10 | (unsigned)xc) : ~0u;
            } else if (CONV) {
                const int hw = p.Hout * p.Wout;
                const int b = m / hw;
                int rem = m - b * hw, wd = p.Wout;
                if (up2) { rem -= uph * hw_in; wd = p.Win; }          // (oy, ox): the pixel of the SOURCE grid inside this tile's phase
                const int oy = rem / wd, ox = rem - oy * wd;
                rowd[i] = m < p.M ? ((unsigned)b << 20 | (unsigned)oy << 10 | (unsigned)ox) : ~0u;
            } else {
                offs[i] = m < p.M ? m * p.ld0 * (int)sizeof(T) + lane_k : OOB;
            }
        }
        // HX: A-piece offsets of filter row dy (3x3, stride 1, pad 1: input row oy + dy - 1, input column xc - 1), once per dy
        // (ld: pixel pitch of the source the pieces read -- src0, or the tail source, whose row-extended tile is that of filter row 1)
        auto set_grp = [&](int dy, int ld) {
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                const unsigned d = rowd[i];
                const int iy = (int)((d >> 10) & 1023u) + dy - 1, ix = (int)(d & 1023u) - 1;
                const bool ok = d != ~0u && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
                offs[i] = ok ? (((int)(d >> 20) * p.Hin + iy) * p.Win + ix) * ld * (int)sizeof(T) + lane_k : OOB;
            }
        };
        // A-piece offsets of filter tap (ty, tx): padding / upsampling / stride live here, once per tap (ups == 2: a stride-1 2x2 window of the stored
        // grid with this tile's phase padding -- no shift)
        // (ld: pixel pitch of the source -- src0, or the tail source read at the tap (pad_t, pad_l), which is the output pixel: stride 1, no ups)
        auto set_tap = [&](int ty, int tx, int ld) {
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                const unsigned d = rowd[i];
                int iy = (int)((d >> 10) & 1023u) * p.stride - pad_t + ty;
                int ix = (int)(d & 1023u) * p.stride - pad_l + tx;
                const bool ok = d != ~0u && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                if (p.ups == 1) { iy >>= 1; ix >>= 1; }
                offs[i] = ok ? (((int)(d >> 20) * p.Hin + iy) * p.Win + ix) * ld * (int)sizeof(T) + lane_k : OOB;
            }
            if constexpr (A8) {
                const unsigned d = srowd;
                int iy = (int)((d >> 10) & 1023u) * p.stride - p.pad_t + ty;
                int ix = (int)(d & 1023u) * p.stride - p.pad_l + tx;
                const bool ok = d != ~0u && (unsigned)iy < (unsigned)Hv && (unsigned)ix < (unsigned)Wv;
                if (p.ups) { iy >>= 1; ix >>= 1; }
                soffs = ok ? (((int)(d >> 20) * p.Hin + iy) * p.Win + ix) * p.as_ld : OOB;
            }
        };
        // uniform K state of the NEXT tile to issue: absolute tile index, and for convs (tap, channel chunk inside the tap)
        const int tpt = CONV ? p.Ctot / BK : 1;     // K tiles per tap
        // korder 1 (channel-chunk-major K): the KH*KW taps of one BK-channel chunk are consecutive tiles, so the ~BM x 128 B of A
        // that a block touches per chunk stay L2-resident across the taps (tap-major K sweeps all channels between reuses)
        // X3OK: the split-bf16 mode (bf16 operand pairs, fp32 output) -- `it` counts virtual tiles (the W side), `ia` the real A tile,
        // `ph` the pass (0: hi x hi, 1: hi x lo, 2: lo x hi) of the tile being issued
        constexpr bool X3OK = sizeof(T) == 2 && sizeof(TO) == 4 && !W8 && NST == 2;
        const bool x3 = X3OK && p.x3;
        int it = kb0_tiles, ity = 0, itx = 0, ic = 0, ph = 0;
        int ia = x3 ? kb0_tiles / 3 : kb0_tiles;          // (split-K ranges of the split mode start on a multiple of 3)
        int hx_dx = 0, hx_ist = 0, hx_len = 3;             // HX issue state: position of tile `it` in its group, A stage of the group, tiles per group
        // the issue state moves to the tail source at its chunk c.  HX: a tail group is ONE tile -- the row-extended tile of srcx (filter row 1's
        // pixels), multiplied at column offset 1 -- so that staging and fragment addressing stay what they are and only the group length differs
        auto enter_tail = [&](int c) {
            rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.srcx, 0, p.x_bytes, 0x00020000);
            ic = c;
            if constexpr (HX) { hx_len = 1; set_grp(1, p.ldx); }
            else set_tap(p.pad_t, p.pad_l, p.ldx);
        };
        if (XT && kb0_tiles >= xt0) {                       // (a split-K slice may start inside the tail)
            enter_tail(kb0_tiles - xt0);
        } else
        if constexpr (HX) {
            const int grp = kb0_tiles / 3;                 // K order (dy, chunk, dx): group = dy * tpt + chunk
            ity = grp / tpt;
            ic = grp - ity * tpt;
            set_grp(ity, p.ld0);
        } else
        if (CONV) {
            const int ntap = p.KH * p.KW;
            const int tap = p.korder ? ia % ntap : ia / tpt;
            ic = p.korder ? ia / ntap : ia - tap * tpt;
            ity = tap / p.KW;
            itx = tap - ity * p.KW;
            set_tap(ity, itx, p.ld0);
        }
        auto next_tile = [&]() {     // advance the issue state by one K tile
            ++it;
            if constexpr (HX) {
                if (++hx_dx == hx_len) {
                    hx_dx = 0;
                    hx_ist ^= 1;
                    if (XT && it >= xt0) {
                        if (it == xt0) enter_tail(0);
                        else ++ic;
                    } else
                    if (++ic == tpt) { ic = 0; ++ity; set_grp(ity, p.ld0); }
                }
                return;
            }
            if (X3OK && x3) {
                if (++ph != 3) return;
                ph = 0;
            }
            ++ia;
            if (CONV) {
                if (XT && ia >= xt0) {
                    if (ia == xt0) enter_tail(0);
                    else ++ic;
                } else
                if (p.korder) {
                    if (++itx == p.KW) { itx = 0; if (++ity == p.KH) { ity = 0; ++ic; } }
                    set_tap(ity, itx, p.ld0);
                } else if (++ic == tpt) {
                    ic = 0;
                    if (++itx == p.KW) { itx = 0; ++ity; }
                    set_tap(ity, itx, p.ld0);
                }
            }
        };
        // issue pieces [q0, q1) of the issue-state tile into LDS stage `buf`
        auto issue_pieces = [&](int buf, int q0, int q1) {
            char* a = ldsA + (HX ? hx_ist : buf) * AXR * 128 + wave_u * 1024;          // (HX: the A stage belongs to the group of three tiles)
            char* b = ldsB + w_stage<W8>(it, buf) * BN * 128 + wave_u * 1024;
            const int soA = __builtin_amdgcn_readfirstlane((CONV ? ic : ia) * 128 + ((X3OK && ph == 2) ? p.lo_off : 0));
            const int soB = __builtin_amdgcn_readfirstlane(w_soff<W8>(it));
            if (W8 && (it & 1) && q1 > AV) q1 = AV;          // odd tile: its W half arrived with the even tile before it
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (q >= q0 && q < q1) {
                    if (q < AV) {
                        if (!(HX && hx_dx != 0))
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(a + q * (RPP * 128)), 16, offs[q], soA, 0, 0);
                    } else
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(b + (q - AV) * (RPP * 128)), 16, offs[q], soB, 0, 0);
                }
            }
            if (A8 && q0 == 0) {          // the call that starts a tile also issues its scale piece: NP + 1 pieces per wave and tile
                char* const sdst = ldsS + buf * 2048 + wave_u * 256;
                const int soS = __builtin_amdgcn_readfirstlane((CONV ? ic : ia) * 4);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsS, (__attribute__((address_space(3))) void*)sdst, 4, soffs, soS, 0, 0);
            }
        };
        if constexpr (A8) {
            // ---- fp8 x fp8 main loop: two k-steps of 64 per K tile, A fragments double-buffered, W fragments rotated in place (column j of
            // the next k-step is fetched right behind column j's MFMAs), one barrier per tile -- the structure of the bf16 loop below at twice
            // the K per tile and per MFMA (64 matrix-pipe cycles each)
            using std::integral_constant;
            constexpr int JS8 = TN > 2 ? 2 : 1;
            u32x4_t fa8[2][TM][2], fb8[TN][2];
            int sa8[2][TM], wsc[TN];
            const int lrow_ = lane & 31, lhalf_ = lane >> 5;
            const int frag_sw8 = (lrow_ >> 1) & 7;
            const int brow8 = EPI == 1 ? (16 * ((lrow_ >> 2) & 1) + 4 * (lrow_ >> 3) + (lrow_ & 3)) : lrow_;
            const int frag_swb8 = (brow8 >> 1) & 7;
            int fk8[2], fkb8[2], ssh[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                fk8[kk] = ((4 * kk + lhalf_) ^ frag_sw8) << 4;           // 16-byte slot 4 kk + h; the lane's second slot (4 kk + 2 + h) is this ^ 32
                fkb8[kk] = ((4 * kk + lhalf_) ^ frag_swb8) << 4;
                ssh[kk] = (2 * kk + lhalf_) * 8;                        // the lane's 32-channel block inside the K tile: byte 2 kk + h of the scale dword
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + (wn * TN + j) * 32 + brow8;
                wsc[j] = n < p.N ? (int)((as_u32(p.wscale[n]) >> 23) & 0xffu) : 127;          // power-of-two fp32 scale -> its E8M0 code
            }
            const char* curA = ldsA + (wm * TM) * 4096 + lrow_ * 128;
            const char* curB = ldsB + (wn * TN) * 4096 + brow8 * 128;
            const char* curS = ldsS + ((wm * TM) * 32 + lrow_) * 4;
            const char* othA = curA + BM * 128;
            const char* othB = curB + BN * 128;
            const char* othS = curS + 2048;
            auto ld_a = [&](int buf, const char* bA, const char* bS, int kk) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    fa8[buf][i][0] = *(const u32x4_t*)(bA + i * 4096 + fk8[kk]);
                    fa8[buf][i][1] = *(const u32x4_t*)(bA + i * 4096 + (fk8[kk] ^ 32));
                    sa8[buf][i] = (int)((*(const uint32_t*)(bS + i * 128) >> ssh[kk]) & 0xffu);
                }
            };
            auto ld_b = [&](int j, const char* bB, int kk) {
                fb8[j][0] = *(const u32x4_t*)(bB + j * 4096 + fkb8[kk]);
                fb8[j][1] = *(const u32x4_t*)(bB + j * 4096 + (fkb8[kk] ^ 32));
            };
            auto mma_col = [&](int buf, int j) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (EPI == 1) mma_mx8(acc[i][j], fb8[j][0], fb8[j][1], wsc[j], fa8[buf][i][0], fa8[buf][i][1], sa8[buf][i]);
                    else mma_mx8(acc[i][j], fa8[buf][i][0], fa8[buf][i][1], sa8[buf][i], fb8[j][0], fb8[j][1], wsc[j]);
                }
            };
            auto phase8 = [&](auto KK, int stage, bool more) {
                constexpr int kk = decltype(KK)::value;
                constexpr int cur = kk, nx = kk ^ 1, nkk = kk ^ 1;
                const char* const nA = kk == 0 ? curA : othA;
                const char* const nB = kk == 0 ? curB : othB;
                const char* const nS = kk == 0 ? curS : othS;
#pragma unroll
                for (int j = 0; j < JS8; ++j) mma_col(cur, j);
                if (kk == 1) {
                    // own pieces of the next tile have landed and every fragment of this tile is in registers; past the barrier that holds
                    // for all waves: this stage may be overwritten (tile kt+2) and the other stage may be read
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
                ld_a(nx, nA, nS, nkk);
#pragma unroll
                for (int j = 0; j < JS8; ++j) ld_b(j, nB, nkk);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = JS8; j < TN; ++j) {
                    mma_col(cur, j);
                    ld_b(j, nB, nkk);
                    if (kk == 1) {          // the pieces of tile kt+2 go out between the MFMA columns behind the barrier
                        constexpr int COLS = TN - JS8, PPC = (NP + COLS - 1) / COLS;
                        if (more) issue_pieces(stage, (j - JS8) * PPC, (j - JS8 + 1) * PPC < NP ? (j - JS8 + 1) * PPC : NP);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            if (nk > 0) {
                issue_pieces(0, 0, AV);               // (its W pieces are already in flight; + the scale piece)
                if (nk > 1) {
                    next_tile();
                    issue_pieces(1, 0, NP);
                    if (nk > 2) next_tile();
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP + 1) : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_s_barrier();
                ld_a(0, curA, curS, 0);
#pragma unroll
                for (int j = 0; j < TN; ++j) ld_b(j, curB, 0);
            }
            for (int kt = 0; kt < nk; ++kt) {
                const int stage = kt & 1;
                const bool more = kt + 2 < nk;
                phase8(integral_constant<int, 0>{}, stage, more);
                phase8(integral_constant<int, 1>{}, stage, more);
                if (kt + 3 < nk) next_tile();
                const char* t = curA; curA = othA; othA = t;
                t = curB; curB = othB; othB = t;
                t = curS; curS = othS; othS = t;
            }
            // the MFMAs are asm statements: hipcc's hazard recognizer pads nothing between the last of them (16 passes) and the epilogue's first
            // VALU read of an accumulator -- 2 x 16 wait states here cover the required 18 whatever the barrier below costs
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
            __syncthreads();
        } else {
        // Fragment pipeline: the ds_reads of k-step kk+1 are issued while the MFMAs of k-step kk run, so the matrix pipe does not
        // wait on LDS latency (all waves of a block are phase-locked by the per-tile barrier, nobody else would cover it).
        // Small wave tiles keep two full fragment sets; the 2x5 wave tile has no registers for that and rotates its B fragments
        // in place: column j of the next k-step is fetched right after column j's MFMAs have been issued.
        constexpr bool ROT = TM * TN > 8;
        constexpr int JS = ROT ? 2 : 0;       // B columns whose MFMAs go ahead of the first next-fragment reads
        u32x4_t fa[2][TM], fb[W8 ? 1 : 2][W8 ? 1 : TN];
        u32x2_t fbr[W8 ? 2 : 1][W8 ? TN : 1];          // W8: raw 8-byte fp8 fragments
        float ws[W8 ? TN : 1];                         // W8: scale of this lane's W row in each 32-row block
        const int frag_sw = (lrow >> 1) & 7;
        // W-tile row this lane reads for the row operand of its 32-row blocks (EPI = 1: permuted, see the kernel comment)
        const int brow = EPI == 1 ? (16 * ((lrow >> 2) & 1) + 4 * (lrow >> 3) + (lrow & 3)) : lrow;
        const int frag_swb = (brow >> 1) & 7;
        int fk[4], fkb[4];   // swizzled byte position of k-step kk inside a fragment row (A side, W side)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            fk[kk] = ((kk * 2 + lhalf) ^ frag_sw) << 4;
            // W8: one 16-byte slot per k-step (16 fp8), the lane half picks its 8 bytes; the A-tile parity flips address bit 6
            fkb[kk] = W8 ? (((kk ^ frag_swb) << 4) + lhalf * 8) : (((kk * 2 + lhalf) ^ frag_swb) << 4);
        }
        if constexpr (W8) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + (wn * TN + j) * 32 + brow;
                ws[j] = n < p.N ? p.wscale[n] : 1.0f;
            }
        }
        // fragment row bases of the stage being multiplied (cur) and of the other stage (oth); swapped after every tile.
        // The loop body is ONE straight-line block (no per-tile variants): branches around MFMAs make the register allocator
        // keep two copies of the accumulators.
        const char* curA = ldsA + (wm * TM) * 4096 + lrow * 128;
        // HX: this lane's row of block i in the row-extended tile for filter column 0 (erow), the A row pointer / swizzle term of the tile being
        // multiplied (hcb / hcs) and of the next one (hnb / hns), the filter column and A stage of the tile being multiplied
        int erow[TM];
        const char* hcb[TM];
        const char* hnb[TM];
        int hcs[TM], hns[TM], m_dx = 0, m_st = 0, m_len = 3, m_t = kb0_tiles;          // (+ tiles per group -- 1 in the tail --, absolute index of that tile)
        const int ks_[4] = {(0 + lhalf) << 4, (2 + lhalf) << 4, (4 + lhalf) << 4, (6 + lhalf) << 4};          // k-step kk -> 16-byte slot 2 kk + half
        auto hx_set = [&](const char** hb, int* hs, int st, int dx) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int e = erow[i] + dx;
                hb[i] = ldsA + st * (AXR * 128) + e * 128;
                hs[i] = ((e >> 1) & 7) << 4;
            }
        };
        if constexpr (HX) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int pm = (wm * TM + i) * 32 + lrow, ir = pm / p.Wout;
                erow[i] = ir * (p.Wout + 2) + (pm - ir * p.Wout);
            }
            if (XT && kb0_tiles >= xt0) {          // the slice starts inside the tail: every tile its own group, read at column offset 1
                m_len = 1;
                hx_set(hcb, hcs, 0, 1);
                hx_set(hnb, hns, 1, 1);
            } else {
                hx_set(hcb, hcs, 0, 0);
                hx_set(hnb, hns, 0, 1);
            }
        }
        const char* const wbase = ldsB + (wn * TN) * 4096 + brow * 128;
        const char* curB = wbase + w_stage<W8>(kb0_tiles, 0) * BN * 128;
        const char* othA = curA + BM * 128;
        const char* othB = wbase + w_stage<W8>(kb0_tiles + 1, 1) * BN * 128;       // W8: the NEXT tile's W stage (may equal the current one)
        int curPar = W8 ? (kb0_tiles & 1) * 64 : 0, othPar = W8 ? ((kb0_tiles + 1) & 1) * 64 : 0;
        int t_abs = kb0_tiles;                                                   // absolute index of the tile being multiplied
        auto load_b = [&](int set, int j, const char* ptr) {
            if constexpr (W8) fbr[set][j] = *(const u32x2_t*)ptr;
            else fb[set][j] = *(const u32x4_t*)ptr;
        };
        auto bfrag = [&](int set, int j) -> u32x4_t {
            if constexpr (W8) return fp8x8_to_bf16x8(fbr[set][j], ws[j]);
            else return fb[set][j];
        };
        // one k-step: its MFMAs, the fetch of the next step's fragments (k-step 3 fetches from the other stage, after the
        // barrier; on the last tile that fetch reads stale bytes that are never used) and, at k-step 3, the pieces of tile kt+2
        auto phase = [&](auto KK, int stage, bool more, bool deep) {
            constexpr int kk = decltype(KK)::value;
            constexpr int cur = kk & 1, nx = cur ^ 1;
            constexpr int fbc = ROT ? 0 : cur, fbn = ROT ? 0 : nx;
            constexpr int nkk = (kk + 1) & 3;
            const char* const nA = (kk < 3 ? curA : othA) + fk[nkk];
            const char* const nB = (kk < 3 ? curB : othB) + (fkb[nkk] ^ (kk < 3 ? curPar : othPar));
#pragma unroll
            for (int j = 0; j < JS; ++j) {
                const u32x4_t bj = bfrag(fbc, j);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (EPI == 1) MmaFrag<T>::mma(acc[i][j], bj, fa[cur][i]);
                    else MmaFrag<T>::mma(acc[i][j], fa[cur][i], bj);
                }
            }
            if (kk == 3) {
                // own pieces of the next tile have landed and every fragment of this tile is in registers; past the barrier
                // that holds for all waves: this stage may be overwritten (tile kt+2) and the other stage may be read
                // (NST > 2: tiles kt+2 .. kt+NST-1 stay in flight behind the one that must have landed -- `deep` says all of them exist)
                if (NST > 2 && deep) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * NP) : "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (HX) fa[nx][i] = *(const u32x4_t*)((kk < 3 ? hcb[i] : hnb[i]) + (ks_[nkk] ^ (kk < 3 ? hcs[i] : hns[i])));
                else fa[nx][i] = *(const u32x4_t*)(nA + i * 4096);
            }
#pragma unroll
            for (int j = 0; j < (ROT ? JS : TN); ++j) load_b(fbn, j, nB + j * 4096);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = JS; j < TN; ++j) {
                const u32x4_t bj = bfrag(fbc, j);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if constexpr (EPI == 1) MmaFrag<T>::mma(acc[i][j], bj, fa[cur][i]);
                    else MmaFrag<T>::mma(acc[i][j], fa[cur][i], bj);
                }
                if (ROT) load_b(0, j, nB + j * 4096);
                // the pieces of tile kt+2 ('more': it exists) go out between the MFMA columns of k-step 3 (their issue slots hide under the matrix
                // pipe) instead of in one burst behind the barrier, where both waves of a SIMD stall on ~9 x 60-180 issue cycles at the same time
                if (kk == 3) {
                    constexpr int COLS = TN - JS, PPC = (NP + COLS - 1) / COLS;
                    if (more) issue_pieces(stage, (j - JS) * PPC, (j - JS + 1) * PPC < NP ? (j - JS + 1) * PPC : NP);
                }
                if (ROT || kk == 3) __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        using std::integral_constant;
        if (nk > 0) {
            // prologue: tile 0 lands, its first fragments are fetched, the issue state points at the next tile to issue (tile NST)
            issue_pieces(0, 0, AV);               // (its W pieces are already in flight)
            if constexpr (NST > 2) {
                static_assert(!W8, "the deep ring is for bf16 / fp32 weights");
#pragma unroll
                for (int s = 1; s < NST; ++s)
                    if (s < nk) {
                        next_tile();
                        issue_pieces(s, 0, NP);
                    }
                if (nk > NST) next_tile();
                if (nk >= NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 1) * NP) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else if (nk > 1) {
                next_tile();
                issue_pieces(1, 0, NP);
                if (nk > 2) next_tile();
                if constexpr (W8) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // tile 1 may have had no W pieces: no fixed count
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HX ? BV : NP) : "memory");          // (HX: tile 1 -- filter column 1 -- has W pieces only)
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (HX) fa[0][i] = *(const u32x4_t*)(hcb[i] + (ks_[0] ^ hcs[i]));
                else fa[0][i] = *(const u32x4_t*)(curA + i * 4096 + fk[0]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) load_b(0, j, curB + j * 4096 + (fkb[0] ^ curPar));
        }
        if constexpr (NST > 2) {
            // ring of NST stages: tile kt is multiplied out of stage kt % NST while tiles kt+1 .. kt+NST-1 are in LDS or in flight; the
            // stage it frees takes tile kt+NST.  For launches of at most one block per CU, where no second block covers the latency
            // of the single tile of look-ahead that two stages give.
            const char* const baseA = curA;
            int sc = 0, so = 1;                   // stages of the tile being multiplied / of the next one
            for (int kt = 0; kt < nk; ++kt) {
                const bool more = kt + NST < nk, deep = kt + NST - 1 < nk;
                phase(integral_constant<int, 0>{}, sc, more, deep);
                phase(integral_constant<int, 1>{}, sc, more, deep);
                phase(integral_constant<int, 2>{}, sc, more, deep);
                phase(integral_constant<int, 3>{}, sc, more, deep);
                if (kt + NST + 1 < nk) next_tile();
                sc = so;
                so = so + 1 == NST ? 0 : so + 1;
                curA = othA; othA = baseA + so * (BM * 128);
                curB = othB; othB = wbase + so * (BN * 128);
            }
        } else {
        for (int kt = 0; kt < nk; ++kt) {
            const int stage = kt & 1;
            const bool more = kt + 2 < nk;
            phase(integral_constant<int, 0>{}, stage, more, false);
            phase(integral_constant<int, 1>{}, stage, more, false);
            phase(integral_constant<int, 2>{}, stage, more, false);
            phase(integral_constant<int, 3>{}, stage, more, false);
            if (kt + 3 < nk) next_tile();
            const char* t = curA; curA = othA; othA = t;
            if constexpr (HX) {          // the tile multiplied next becomes current; its successor: next filter column, or column 0 of the next group's stage
                ++m_t;
                if (++m_dx == m_len) { m_dx = 0; m_st ^= 1; if (XT && m_t >= xt0) m_len = 1; }
#pragma unroll
                for (int i = 0; i < TM; ++i) { hcb[i] = hnb[i]; hcs[i] = hns[i]; }
                const bool glast = m_dx + 1 == m_len, ntail = XT && m_t + 1 >= xt0;          // the successor opens a group / is a tail tile
                hx_set(hnb, hns, glast ? (m_st ^ 1) : m_st, ntail ? 1 : (glast ? 0 : m_dx + 1));
            }
            if constexpr (W8) {
                ++t_abs;
                curB = othB; curPar = othPar;
                othB = wbase + (((t_abs + 1) >> 1) & 1) * BN * 128;
                othPar = ((t_abs + 1) & 1) * 64;
            } else {
                t = curB; curB = othB; othB = t;
            }
        }
        }
        __syncthreads();
        }       // (!A8)
    } else {
        load_tiles();
        store_tiles(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) load_tiles();
            compute_tile(buf);
            if (kt + 1 < nk) store_tiles(buf ^ 1);
            __syncthreads();
        }
    }

    if constexpr (EPI == 1) {
        // ---- direct epilogue: lane (row lrow of its 32-row block, half lhalf) holds columns 16*lhalf .. 16*lhalf+15 of every
        // 32-column block of its wave tile.  Host guarantees (launch_typed): N % 16 == 0, 16-byte aligned rows of out / residual /
        // bias / rowvec, no PReLU, rowvec uniform per tile, fused GroupNorm statistics only with act NONE.
        if (p.splitk > 1) {
            // split-K partial sums in FRAGMENT order: slab [z][tile] = [wave][i][j][q][lane] x 16 bytes, so that every store instruction of a
            // wave writes one contiguous KiB (direct fp32 ROW segments -- 64 scattered 16-byte pieces per instruction -- measured slower than
            // the staged rows, 61.7 vs 56.3 us; this form needs neither LDS nor a barrier).  splitk_reduce_frag_kernel reads them back the same way.
            f32x4_t* const slab = (f32x4_t*)(p.ws + ((long long)blockIdx.z * (p.tiles_m * p.tiles_n) + (tile_m * p.tiles_n + tile_n)) * (long long)(BM * BN)) + lane;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    f32x4_t* const dst = slab + ((wave * TM + i) * TN + j) * 256;
#pragma unroll
                    for (int q = 0; q < 4; ++q) dst[q * 64] = f32x4_t{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                }
            return;
        }
        TO* const outp = (TO*)p.out + zb * p.sO;
        const TO* const resp = p.residual ? (const TO*)p.residual + zb * p.sR : nullptr;
        constexpr int OV = sizeof(TO) == 2 ? 2 : 4;      // 16-byte vectors per 16 output values
        auto store16 = [&](TO* dst, const float* v) {
            if constexpr (sizeof(TO) == 2) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    u32x4_t w;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = pack2<TO>(v[8 * h + 2 * e], v[8 * h + 2 * e + 1]);
                    ((u32x4_t*)dst)[h] = w;
                }
            } else {
#pragma unroll
                for (int h = 0; h < 4; ++h) ((u32x4_t*)dst)[h] = u32x4_t{as_u32(v[4 * h]), as_u32(v[4 * h + 1]), as_u32(v[4 * h + 2]), as_u32(v[4 * h + 3])};
            }
        };
        // column constants -> LDS (the main loop ended on a barrier: the operand stages are dead)
        float* const colc_lds = (float*)smem;
        float* const colu_lds = (float*)(smem + 12288);            // (behind the GroupNorm column sums at +2048 .. +12288)
        constexpr bool ln_c = LNF == 2;                             // this launch consumes a LayerNorm-ed operand: row affine in the epilogue
        if (tid < BN) {
            colc_lds[tid] = colc;
            if (ln_c) colu_lds[tid] = colu;
        }
        // row statistics of this lane's TM rows from the producer's per-stripe (mean, M2) records: equal counts per part, Chan's combination
        float ln_rs[TM], ln_rm[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) { ln_rs[i] = 1.f; ln_rm[i] = 0.f; }
        if constexpr (ln_c) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = m0 + (wm * TM + i) * 32 + lrow;
                if (row < p.M) {
                    const f32x2_t* const sp = (const f32x2_t*)p.ln_in + (long long)row * p.ln_in_parts;
                    float mean = 0.f;
                    for (int q = 0; q < p.ln_in_parts; ++q) mean += sp[q][0];
                    mean /= (float)p.ln_in_parts;
                    float m2 = 0.f;
                    for (int q = 0; q < p.ln_in_parts; ++q) { const float dq = sp[q][0] - mean; m2 += sp[q][1] + (float)p.ln_in_cols * dq * dq; }
                    const float rs = 1.0f / sqrtf(m2 / (float)(p.ln_in_cols * p.ln_in_parts) + p.ln_eps);
                    ln_rs[i] = rs;
                    ln_rm[i] = rs * mean;
                }
            }
        }
        lds_barrier();
        bool geglu = false;
        if constexpr (TN % 2 == 0) geglu = p.act == RF_ACT_GEGLU;
        if (geglu) {
            if constexpr (TN % 2 == 0) {
#pragma unroll
                for (int j = 0; j < TN; j += 2) {
                    const int cv = n0 + (wn * TN + j) * 32 + lhalf * 16;           // value columns (packed order); gate = +32
                    const int ocol = (n0 >> 1) + ((wn * TN + j) >> 1) * 32 + lhalf * 16;
                    const bool cok = cv + 32 < p.N;
                    float bv[16], bg[16], uv[16], ug[16];          // (uv / ug: LayerNorm consumers only -- untouched and eliminated otherwise)
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const f32x4_t a = ((const f32x4_t*)(colc_lds + (cv - n0)))[h], g = ((const f32x4_t*)(colc_lds + (cv - n0) + 32))[h];
#pragma unroll
                        for (int e = 0; e < 4; ++e) { bv[4 * h + e] = a[e]; bg[4 * h + e] = g[e]; }
                        if constexpr (ln_c) {
                            const f32x4_t ua = ((const f32x4_t*)(colu_lds + (cv - n0)))[h], ugg = ((const f32x4_t*)(colu_lds + (cv - n0) + 32))[h];
#pragma unroll
                            for (int e = 0; e < 4; ++e) { uv[4 * h + e] = ua[e]; ug[4 * h + e] = ugg[e]; }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int row = m0 + (wm * TM + i) * 32 + lrow;
                        if (row < p.M && cok) {
                            float v[16];
                            if constexpr (ln_c) {          // LayerNorm folded in: rstd (alpha acc - mean u) + b'  (gamma is in W, W beta in the bias)
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const float a_ = __builtin_fmaf(acc[i][j][r] * p.alpha, ln_rs[i], __builtin_fmaf(-ln_rm[i], uv[r], bv[r]));
                                    const float g_ = __builtin_fmaf(acc[i][j + 1][r] * p.alpha, ln_rs[i], __builtin_fmaf(-ln_rm[i], ug[r], bg[r]));
                                    v[r] = a_ * gelu_for<T>(g_);
                                }
                            } else {
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const float a_ = acc[i][j][r] * p.alpha + bv[r], g_ = acc[i][j + 1][r] * p.alpha + bg[r];
                                    v[r] = a_ * gelu_for<T>(g_);
                                }
                            }
                            if (!ln_c && resp) {
                                const u32x4_t* rp = (const u32x4_t*)(resp + (long long)row * p.ldr + ocol);
#pragma unroll
                                for (int h = 0; h < OV; ++h) {
                                    float f[16 / OV];
                                    unpack16<TO>(rp[h], f);
#pragma unroll
                                    for (int e = 0; e < 16 / OV; ++e) v[h * (16 / OV) + e] += f[e];
                                }
                            }
                            if constexpr (A8) {
                                if (p.oscale) {
                                    // fp8 output for the next fp8 x fp8 GEMM (ff.net.2): this lane holds columns [16 h, 16 h + 16) of a 32-column
                                    // block of its row, lane ^ 32 the other half: block amax across the two, one E8M0 code, 16 bytes per lane
                                    float m = 0.f;
#pragma unroll
                                    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(v[r]));
                                    const auto sw = __builtin_amdgcn_permlane32_swap(as_u32(m), as_u32(m), false, false);
                                    const int code = e8m0_for_amax(fmaxf(as_f32(sw[0]), as_f32(sw[1])));
                                    const u32x2_t q0 = quant8_fp8(v, code), q1 = quant8_fp8(v + 8, code);
                                    fp8_t* const qrow = (fp8_t*)p.out + (long long)row * p.ldo;
                                    *(u32x4_t*)(qrow + ocol) = u32x4_t{q0[0], q0[1], q1[0], q1[1]};
                                    if (lhalf == 0) ((fp8_t*)p.oscale)[(long long)row * p.os_ld + (ocol >> 5)] = (fp8_t)code;
                                    continue;
                                }
                            }
                            store16(outp + (long long)row * p.ldo + ocol, v);
                        }
                    }
                }
            }
        } else {
            // One 32x32 block at a time; the column constants come from LDS, the residual segments through a ring of PFD blocks in
            // flight.  sched_barrier(0) after every block keeps hipcc from hoisting every load of the unrolled nest to the top (the 2x5
            // wave tile then spills ~170 registers per lane).
            constexpr int NBLK = TM * TN;
            constexpr int PFD = sizeof(TO) == 2 ? (NBLK < 4 ? NBLK : 4) : 2;      // residual blocks in flight (8 / 16 registers each): the
                                                                                  // fragment registers of the main loop are free now
            u32x4_t rq[PFD][OV];
            auto load_res = [&](int blk, u32x4_t* r) {
                const int i = blk % TM, j = blk / TM;
                const int col = n0 + (wn * TN + j) * 32 + lhalf * 16;
                const int row = m0 + (wm * TM + i) * 32 + lrow;
                if (!ln_c && resp && row < p.M && col < p.N) {
                    const u32x4_t* rp = (const u32x4_t*)(resp + (long long)row * p.ldr + col);
#pragma unroll
                    for (int h = 0; h < OV; ++h) r[h] = rp[h];
                }
            };
#pragma unroll
            for (int b = 0; b < PFD; ++b) load_res(b, rq[b]);
            // Fused GroupNorm statistics (gn_rows > 0): per 32-column block the lane sums its 16 columns over its TM rows (values as stored),
            // a 5-stage butterfly over the 32 lanes of the half-wave leaves ONE column total per lane (lanes 0-15: sums, 16-31: sums of
            // squares), the wave rows meet in LDS and 64 threads form the 32 group sums per consumer in fp64 -- same slots, same
            // consumers as the staged epilogue.
            const bool gn_on = p.gn_rows > 0;
            constexpr bool ln_p = LNF == 1;                      // this launch also emits the LayerNorm row statistics of its output
            const bool keep_on = gn_on || ln_p;                  // the values as stored replace the (dead) accumulators
            float* const gcs = (float*)(smem + 2048);            // [2][WM][BN] column sums / sums of squares per wave row
            int orow[TM];                                        // rows of `out` this lane writes (ups == 2: the phase's pixels, out_row)
#pragma unroll
            for (int i = 0; i < TM; ++i) orow[i] = out_row(m0 + (wm * TM + i) * 32 + lrow);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + (wn * TN + j) * 32 + lhalf * 16;
                const bool cok = col < p.N;
                f32x4_t cb[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) cb[h] = ((const f32x4_t*)(colc_lds + (col - n0)))[h];
                // (LayerNorm consumer: rstd (alpha acc - mean u) + b' -- the row factors differ per i, the two column vectors are combined per element)
                f32x4_t cu[4];          // (LayerNorm consumers only)
                if constexpr (ln_c) {
#pragma unroll
                    for (int h = 0; h < 4; ++h) cu[h] = ((const f32x4_t*)(colu_lds + (col - n0)))[h];
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int blk = j * TM + i;
                    const int row = m0 + (wm * TM + i) * 32 + lrow;
                    const u32x4_t* const myr = rq[blk % PFD];
                    const bool live = row < p.M && cok;
                    if (live) {
                        TO* dst = outp + (long long)orow[i] * p.ldo + col;
#pragma unroll
                        for (int h = 0; h < OV; ++h) {
                            constexpr int E = 16 / OV;
                            float f[E], v[E];
                            if (resp) unpack16<TO>(myr[h], f);
                            if constexpr (ln_c) {          // (no residual on a LayerNorm consumer: host)
#pragma unroll
                                for (int e = 0; e < E; ++e)
                                    v[e] = __builtin_fmaf(acc[i][j][h * E + e] * p.alpha, ln_rs[i],
                                                          __builtin_fmaf(-ln_rm[i], cu[(h * E + e) >> 2][(h * E + e) & 3], cb[(h * E + e) >> 2][(h * E + e) & 3]));
                            } else {
#pragma unroll
                                for (int e = 0; e < E; ++e) v[e] = acc[i][j][h * E + e] * p.alpha + cb[(h * E + e) >> 2][(h * E + e) & 3] + (resp ? f[e] : 0.0f);
                                if (p.act == RF_ACT_ADD_RELU) {
#pragma unroll
                                    for (int e = 0; e < E; ++e) v[e] = fmaxf(v[e], 0.0f);
                                }
                            }
                            const u32x4_t w = pack16<TO>(v);
                            ((u32x4_t*)dst)[h] = w;
                            if (keep_on) {
                                float y[E];
                                unpack16<TO>(w, y);              // the values as stored replace the (dead) accumulators: no extra registers
#pragma unroll
                                for (int e = 0; e < E; ++e) acc[i][j][h * E + e] = y[e];
                            }
                        }
                    } else if (keep_on) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
                    }
                    if (blk + PFD < NBLK) load_res(blk + PFD, rq[blk % PFD]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                float gx[32];                                    // [0, 16): column sums, [16, 32): sums of squares (this lane's rows)
                if (gn_on) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        float a = 0.f, q = 0.f;
#pragma unroll
                        for (int i = 0; i < TM; ++i) { a += acc[i][j][k]; q += acc[i][j][k] * acc[i][j][k]; }
                        gx[k] = a;
                        gx[16 + k] = q;
                    }
                }
                if (gn_on) {
                    halfwave_reduce_scatter32(gx, lrow);
                    // lane lrow now holds the total of value index lrow: column lrow (sums) / column lrow - 16 (squares)
                    gcs[((lrow >> 4) * WM + wm) * BN + (wn * TN + j) * 32 + lhalf * 16 + (lrow & 15)] = gx[0];
                }
            }
            if (gn_on) {
                lds_barrier();
                if (tid < 64) {
                    const int c = tid >> 5, g = tid & 31;
                    if (p.gn_part[c]) {
                        const int cpg = p.gn_cpg[c], base = p.gn_coff[c] + n0;            // consumer channel of local column 0
                        const int lo = max(0, g * cpg - base), hi = min(min(BN, p.N - n0), (g + 1) * cpg - base);
                        double sa = 0.0, sq = 0.0;
                        for (int k = lo; k < hi; ++k)
#pragma unroll
                            for (int r = 0; r < WM; ++r) { sa += (double)gcs[r * BN + k]; sq += (double)gcs[(WM + r) * BN + k]; }
                        const int b = m0 / p.gn_rows, mt = (m0 - b * p.gn_rows) / BM;
                        double* o = p.gn_part[c] + (((long long)b * p.gn_nch[c] + p.gn_slot[c] + mt * p.tiles_n + tile_n) * 32 + g) * 2;
                        o[0] = sa;
                        o[1] = sq;
                    }
                }
            }
            if constexpr (ln_p) {
                // LayerNorm statistics of the rows this wave wrote, over its 32 TN columns (values as stored): the lane pair (row, half 0 / 1)
                // holds them all -- two-pass (mean, then squared deviations) in registers, the halves meet through v_permlane32_swap;
                // record = (mean, M2) per row and column stripe, combined by the consumer GEMM's epilogue
                const int part = (n0 + wn * TN * 32) / (TN * 32);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    float sm = 0.f;
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) sm += acc[i][j][e];
                    {
                        const auto sw = __builtin_amdgcn_permlane32_swap(as_u32(sm), as_u32(sm), false, false);
                        sm = as_f32(sw[0]) + as_f32(sw[1]);
                    }
                    const float mean = sm / (float)(TN * 32);
                    float sq = 0.f;
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) { const float dq = acc[i][j][e] - mean; sq += dq * dq; }
                    {
                        const auto sw = __builtin_amdgcn_permlane32_swap(as_u32(sq), as_u32(sq), false, false);
                        sq = as_f32(sw[0]) + as_f32(sw[1]);
                    }
                    const int row = m0 + (wm * TM + i) * 32 + lrow;
                    // (a WN = 2 tile whose BN does not divide N has a wave-tile stripe beyond N: no record -- part would be >= ln_out_parts)
                    if (lhalf == 0 && row < p.M && part < p.ln_out_parts) *(f32x2_t*)(p.ln_out + ((long long)row * p.ln_out_parts + part) * 2) = f32x2_t{mean, sq};
                }
            }
        }
        return;
    }

    // ---- epilogue: accumulators -> LDS (fp32 [ER][BN]) -> coalesced 16-byte row segments, in NCH row chunks
    // (the main loop ended on a barrier, so the operand tiles are dead and the LDS can be reused)
    constexpr int NCH = (BM * BN * 4 > 96 * 1024) ? WM : 1;      // big tiles: one chunk per wave row
    constexpr int ER = BM / NCH;
    float* const stage = (float*)smem;
    TO* outp = (TO*)p.out + zb * p.sO;
    const TO* resp = p.residual ? (const TO*)p.residual + zb * p.sR : nullptr;
    const bool partial_out = p.splitk > 1;
    const bool gn_on = p.gn_rows > 0;          // fused GroupNorm statistics of the values this block writes
    float gsum[4] = {0.f, 0.f, 0.f, 0.f}, gsq[4] = {0.f, 0.f, 0.f, 0.f};      // this thread's 4 columns, all of its rows
    for (int ch = 0; ch < NCH; ++ch) {
    if (NCH == 1 || wm == ch) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = ((NCH == 1 ? wm * TM : 0) + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
                    stage[rl * BN + (wn * TN + j) * 32 + lrow] = acc[i][j][r];
                }
    }
    lds_barrier();           // LDS-only barrier: the previous chunk's global stores may stay in flight
    const int mch = m0 + ch * ER;
    if (partial_out) {            // split-K: raw fp32 partial sums, coalesced; bias / activation / residual happen in the reduce pass
        constexpr int VPRS = BN / 4;
        float* wsz = p.ws + (long long)blockIdx.z * p.M * p.N;
        for (int idx = tid; idx < ER * VPRS; idx += NT) {
            const int rl = idx / VPRS, cl = (idx - rl * VPRS) * 4;
            const int row = mch + rl, col = n0 + cl;
            if (row >= p.M || col >= p.N) continue;
            const f32x4_t a4 = *(const f32x4_t*)(stage + rl * BN + cl);
            float* dst = wsz + (long long)row * p.N + col;
            if ((p.N & 3) == 0) *(f32x4_t*)dst = a4;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (col + e < p.N) dst[e] = a4[e];
            }
        }
    } else if (p.act == RF_ACT_GEGLU) {
        // same thread -> fixed column mapping as the general path below: the value / gate bias vectors are loaded once
        constexpr int OV = BN / 8;                      // output 4-column vectors per row (N/2 columns)
        constexpr int EROWS = NT / OV;
        constexpr int PASSES = (ER + EROWS - 1) / EROWS;
        const int oc = (tid % OV) * 4, er = tid / OV;
        const int lv = (oc >> 5) * 64 + (oc & 31), lg = lv + 32;      // local value / gate columns
        const int ocol = (n0 >> 1) + oc;
        const bool t_on = er < EROWS && n0 + lg < p.N;
        f32x4_t ba = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
        if (t_on && p.bias) {
            if (p.vec_ok) { ba = *(const f32x4_t*)(p.bias + n0 + lv); bg = *(const f32x4_t*)(p.bias + n0 + lg); }
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) { ba[e] = p.bias[n0 + lv + e]; bg[e] = p.bias[n0 + lg + e]; }
            }
        }
#pragma unroll 2
        for (int k = 0; k < PASSES; ++k) {
            const int rl = er + k * EROWS, row = mch + rl;
            if (!t_on || rl >= ER || row >= p.M) continue;
            const f32x4_t a4 = *(const f32x4_t*)(stage + rl * BN + lv);
            const f32x4_t g4 = *(const f32x4_t*)(stage + rl * BN + lg);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a_ = a4[e] * p.alpha + ba[e], g_ = g4[e] * p.alpha + bg[e];
                v[e] = a_ * gelu_for<T>(g_);
            }
            TO* dst = outp + (long long)row * p.ldo + ocol;
            if (p.vec_ok) {
                if (resp) {
                    float rr[4];
                    if constexpr (sizeof(TO) == 2) {
                        const u32x2_t q = *(const u32x2_t*)(resp + (long long)row * p.ldr + ocol);
                        const uint32_t q0 = q[0], q1 = q[1];
                        rr[0] = lo16<TO>(q0); rr[1] = hi16<TO>(q0); rr[2] = lo16<TO>(q1); rr[3] = hi16<TO>(q1);
                    } else {
                        const f32x4_t q = *(const f32x4_t*)(resp + (long long)row * p.ldr + ocol);
                        rr[0] = q[0]; rr[1] = q[1]; rr[2] = q[2]; rr[3] = q[3];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += rr[e];
                }
                if constexpr (sizeof(TO) == 2) {
                    u32x2_t w; w[0] = pack2<TO>(v[0], v[1]); w[1] = pack2<TO>(v[2], v[3]);
                    *(u32x2_t*)dst = w;
                } else {
                    *(f32x4_t*)dst = f32x4_t{v[0], v[1], v[2], v[3]};
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float y = v[e];
                    if (resp) y += load_out<TO>(resp + (long long)row * p.ldr + ocol + e);
                    store_out<TO>(dst + e, y);
                }
            }
        }
    } else {
        // thread -> one fixed 4-column segment and every EROWS-th row of the chunk: bias / timestep vector are loaded once, and
        // the residual loads of U rows are issued together BEFORE the first one is consumed.  (One load -> wait -> store per
        // row serialises the whole HBM / L2 latency per row: that alone made the K = C projection layers 2x slower in situ.)
        constexpr int VPR = BN / 4;
        constexpr int EROWS = NT / VPR;
        constexpr int PASSES = (ER + EROWS - 1) / EROWS;
        constexpr int U = sizeof(TO) == 2 ? 4 : 2;      // rows of residual loads in flight (fp32 rows cost 4 registers each)
        const int cs = tid % VPR, er = tid / VPR;
        const int cl = cs * 4, col = n0 + cl;
        const bool t_on = er < EROWS && col < p.N;
        const bool full = p.vec_ok && col + 3 < p.N;
        float cadd[4] = {0.f, 0.f, 0.f, 0.f};           // bias (+ per-sample vector when the chunk lies inside one sample)
        const bool rv_uniform = p.rowvec && (p.rows_per_sample % ER == 0);
        if (t_on) {
            const float* rvu = rv_uniform ? p.rowvec + (long long)(mch / p.rows_per_sample) * p.ldv : nullptr;
            if (full) {
                if (p.bias) { const f32x4_t b4 = *(const f32x4_t*)(p.bias + col); cadd[0] = b4[0]; cadd[1] = b4[1]; cadd[2] = b4[2]; cadd[3] = b4[3]; }
                if (rvu) { const f32x4_t r4 = *(const f32x4_t*)(rvu + col); cadd[0] += r4[0]; cadd[1] += r4[1]; cadd[2] += r4[2]; cadd[3] += r4[3]; }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < p.N) { if (p.bias) cadd[e] = p.bias[col + e]; if (rvu) cadd[e] += rvu[col + e]; }
            }
        }
        typedef typename std::conditional<sizeof(TO) == 2, u32x2_t, f32x4_t>::type resv_t;
        // ups == 2: this thread's rows are EROWS apart, so their pixels follow incrementally -- out_row (two divisions) once per chunk; a step of
        // (ostep_i source rows, ostep_j columns) with a carry over the source row's end: two rows of `out` further, 2 Win columns back = + Wout
        int orow_cur = 0, oj = 0, ostep = 0, ostep_j = 0;
        if (up2) {
            const int r = (mch + er) % hw_in, ostep_i = EROWS / p.Win;
            orow_cur = out_row(mch + er);
            oj = r % p.Win;
            ostep_j = EROWS - ostep_i * p.Win;
            ostep = 2 * ostep_i * p.Wout + 2 * ostep_j;
        }
#pragma unroll 1
        for (int k0 = 0; k0 < PASSES; k0 += U) {
            resv_t rq[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int rl = er + (k0 + u) * EROWS, row = mch + rl;
                ok[u] = t_on && (k0 + u) < PASSES && rl < ER && row < p.M;
                if (ok[u] && resp && full) rq[u] = *(const resv_t*)(resp + (long long)row * p.ldr + col);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int orow_u = orow_cur;
                if (up2) {
                    orow_cur += ostep; oj += ostep_j;
                    if (oj >= p.Win) { oj -= p.Win; orow_cur += p.Wout; }
                }
                if (!ok[u]) continue;
                const int rl = er + (k0 + u) * EROWS, row = mch + rl;
                const f32x4_t a4 = *(const f32x4_t*)(stage + rl * BN + cl);
                float v[4] = {a4[0] * p.alpha + cadd[0], a4[1] * p.alpha + cadd[1], a4[2] * p.alpha + cadd[2], a4[3] * p.alpha + cadd[3]};
                if (p.rowvec && !rv_uniform) {
                    const float* rv = p.rowvec + (long long)(row / p.rows_per_sample) * p.ldv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (col + e < p.N) v[e] += rv[col + e];
                }
                if (p.act != RF_ACT_NONE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float y = v[e];
                        if (p.act == RF_ACT_SILU) y = silu_exact(y);
                        else if (p.act == RF_ACT_QUICK_GELU) y = quick_gelu(y);
                        else if (p.act == RF_ACT_GELU) y = gelu_erf(y);
                        else if (p.act == RF_ACT_RELU) y = fmaxf(y, 0.0f);
                        else if (p.act == RF_ACT_SIGMOID) y = 1.0f / (1.0f + expf(-y));
                        else if (p.act == RF_ACT_PRELU) y = y >= 0.0f ? y : y * p.act_vec[min(col + e, p.N - 1)];
                        v[e] = y;
                    }
                }
                TO* dst = outp + (long long)(up2 ? orow_u : row) * p.ldo + col;
                if (full) {
                    if (resp) {
                        if constexpr (sizeof(TO) == 2) {
                            const uint32_t q0 = rq[u][0], q1 = rq[u][1];
                            v[0] += lo16<TO>(q0); v[1] += hi16<TO>(q0); v[2] += lo16<TO>(q1); v[3] += hi16<TO>(q1);
                        } else {
                            v[0] += rq[u][0]; v[1] += rq[u][1]; v[2] += rq[u][2]; v[3] += rq[u][3];
                        }
                    }
                    if (p.act == RF_ACT_ADD_RELU) { v[0] = fmaxf(v[0], 0.0f); v[1] = fmaxf(v[1], 0.0f); v[2] = fmaxf(v[2], 0.0f); v[3] = fmaxf(v[3], 0.0f); }
                    if constexpr (sizeof(TO) == 2) {
                        u32x2_t w; w[0] = pack2<TO>(v[0], v[1]); w[1] = pack2<TO>(v[2], v[3]);
                        *(u32x2_t*)dst = w;
                        if (gn_on) {      // statistics of the values AS STORED (what the apply pass and the unfused statistics pass read)
                            const uint32_t w0 = w[0], w1 = w[1];
                            v[0] = lo16<TO>(w0); v[1] = hi16<TO>(w0); v[2] = lo16<TO>(w1); v[3] = hi16<TO>(w1);
                        }
                    }
                    if (gn_on) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { gsum[e] += v[e]; gsq[e] += v[e] * v[e]; }
                    }
                    if constexpr (sizeof(TO) == 2) {
                    } else {
                        *(f32x4_t*)dst = f32x4_t{v[0], v[1], v[2], v[3]};
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e < p.N) {
                            float y = v[e];
                            if (resp) y += load_out<TO>(resp + (long long)row * p.ldr + col + e);
                            if (p.act == RF_ACT_ADD_RELU) y = fmaxf(y, 0.0f);
                            store_out<TO>(dst + e, y);
                            if (gn_on) {
                                float ys = y;
                                if constexpr (sizeof(TO) == 2) ys = round16<TO>(y);
                                gsum[e] += ys; gsq[e] += ys * ys;
                            }
                        }
                }
            }
        }
    }
    if (NCH > 1) lds_barrier();
    }
    if (gn_on) {
        // column sums of the tile: [EROWS][BN] per-thread partials -> 32 group sums per consumer -> one chunk slot (fp64)
        constexpr int VPR = BN / 4, EROWS = NT / VPR;
        float* const cs = stage;                       // [2][EROWS][BN]
        if (NCH == 1) lds_barrier();                   // every thread is done with the staged tile
        const int cs_ = tid % VPR, er = tid / VPR;
        if (er < EROWS) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cs[er * BN + cs_ * 4 + e] = gsum[e];
                cs[(EROWS + er) * BN + cs_ * 4 + e] = gsq[e];
            }
        }
        lds_barrier();
        if (tid < 64) {
            const int c = tid >> 5, g = tid & 31;
            if (p.gn_part[c]) {
                const int cpg = p.gn_cpg[c], base = p.gn_coff[c] + n0;            // consumer channel of local column 0
                const int lo = max(0, g * cpg - base), hi = min(min(BN, p.N - n0), (g + 1) * cpg - base);
                double sa = 0.0, sq = 0.0;
                for (int k = lo; k < hi; ++k)
#pragma unroll
                    for (int r = 0; r < EROWS; ++r) { sa += (double)cs[r * BN + k]; sq += (double)cs[(EROWS + r) * BN + k]; }
                const int b = m0 / p.gn_rows, mt = (m0 - b * p.gn_rows) / BM;
                double* o = p.gn_part[c] + (((long long)b * p.gn_nch[c] + p.gn_slot[c] + mt * p.tiles_n + tile_n) * 32 + g) * 2;
                o[0] = sa;
                o[1] = sq;
            }
        }
    }
}

// split-K second pass: out = act(alpha * sum_z ws[z] + bias + rowvec) + residual.  One block = SK_ROWS x SK_COLS of the output,
// thread -> one fixed 4-column segment and every 4th row, so the fused GroupNorm statistics reduce exactly as in the main epilogue
// (chunk slot = gn_slot + (row tile within the sample) * column tiles + column tile).
// (SK_ROWS, SK_COLS and sk_rows_for, the rows per reduce block: gemm_plan.h)
template <typename TO, int SKR>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmParams p) {
    const int tid = threadIdx.x;
    const int cl = (tid & 63) * 4, rp = tid >> 6;
    const int n0 = blockIdx.x * SK_COLS, m0 = blockIdx.y * SKR;
    const int col = n0 + cl;
    const bool vec = (p.N & 3) == 0 && p.vec_ok;
    const bool gn_on = p.gn_rows > 0;
    float gsum[4] = {0.f, 0.f, 0.f, 0.f}, gsq[4] = {0.f, 0.f, 0.f, 0.f};
    TO* outp = (TO*)p.out;
    const TO* resp = (const TO*)p.residual;
    if (col < p.N) {
        float cadd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p.bias && col + e < p.N) cadd[e] = p.bias[col + e];
        constexpr int U = SKR / 4 < 4 ? SKR / 4 : 4;          // rows in flight: the partial-sum loads of U rows are issued together (one row at a time
                                      // serialises the L2 / HBM latency SK_ROWS / 4 times per thread)
#pragma unroll 1
        for (int k0 = 0; k0 < SKR / 4; k0 += U) {
            float v[U][4];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ok[u] = m0 + rp + 4 * (k0 + u) < p.M;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[u][e] = 0.f;
            }
            // residual and per-sample vector of the U rows: issued with (not after) the partial-sum loads
            typedef typename std::conditional<sizeof(TO) == 2, u32x2_t, f32x4_t>::type resv_t;
            const bool full = vec && col + 3 < p.N;
            resv_t rq[U];
            f32x4_t rv4[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int row = m0 + rp + 4 * (k0 + u);
                rv4[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (ok[u] && full) {
                    if (resp) rq[u] = *(const resv_t*)(resp + (long long)row * p.ldr + col);
                    if (p.rowvec) rv4[u] = *(const f32x4_t*)(p.rowvec + (long long)(row / p.rows_per_sample) * p.ldv + col);
                }
            }
            for (int z = 0; z < p.splitk; ++z) {
                f32x4_t a[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float* src = p.ws + ((long long)z * p.M + (m0 + rp + 4 * (k0 + u))) * p.N + col;
                    a[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                    if (ok[u]) {
                        if (vec) a[u] = *(const f32x4_t*)src;
                        else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) if (col + e < p.N) a[u][e] = src[e];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) { v[u][0] += a[u][0]; v[u][1] += a[u][1]; v[u][2] += a[u][2]; v[u][3] += a[u][3]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                const int row = m0 + rp + 4 * (k0 + u);
                const float* rv = (p.rowvec && !full) ? p.rowvec + (long long)(row / p.rows_per_sample) * p.ldv : nullptr;
                float y4[4] = {0.f, 0.f, 0.f, 0.f}, r4[4] = {0.f, 0.f, 0.f, 0.f};
                if (resp && full) {
                    if constexpr (sizeof(TO) == 2) {
                        const uint32_t q0 = rq[u][0], q1 = rq[u][1];
                        r4[0] = lo16<TO>(q0); r4[1] = hi16<TO>(q0); r4[2] = lo16<TO>(q1); r4[3] = hi16<TO>(q1);
                    } else {
                        r4[0] = rq[u][0]; r4[1] = rq[u][1]; r4[2] = rq[u][2]; r4[3] = rq[u][3];
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = col + e;
                    if (c >= p.N) break;
                    float y = v[u][e] * p.alpha + cadd[e] + rv4[u][e];
                    if (rv) y += rv[c];
                    if (p.act == RF_ACT_SILU) y = silu_exact(y);
                    else if (p.act == RF_ACT_QUICK_GELU) y = quick_gelu(y);
                    else if (p.act == RF_ACT_GELU) y = gelu_erf(y);
                    else if (p.act == RF_ACT_RELU) y = fmaxf(y, 0.0f);
                    else if (p.act == RF_ACT_SIGMOID) y = 1.0f / (1.0f + expf(-y));
                    else if (p.act == RF_ACT_PRELU) y = y >= 0.0f ? y : y * p.act_vec[c];
                    if (resp) y += full ? r4[e] : load_out<TO>(resp + (long long)row * p.ldr + c);
                    if (gn_on) {          // statistics of the value as stored
                        float ys = y;
                        if constexpr (sizeof(TO) == 2) ys = round16<TO>(y);
                        gsum[e] += ys; gsq[e] += ys * ys;
                    }
                    y4[e] = y;
                    if (!full) store_out<TO>(outp + (long long)row * p.ldo + c, y);
                }
                if (full) {
                    TO* dst = outp + (long long)row * p.ldo + col;
                    if constexpr (sizeof(TO) == 2) {
                        u32x2_t w; w[0] = pack2<TO>(y4[0], y4[1]); w[1] = pack2<TO>(y4[2], y4[3]);
                        *(u32x2_t*)dst = w;
                    } else {
                        *(f32x4_t*)dst = f32x4_t{y4[0], y4[1], y4[2], y4[3]};
                    }
                }
            }
        }
    }
    if (gn_on) {
        __shared__ float cs[2][4][SK_COLS];
#pragma unroll
        for (int e = 0; e < 4; ++e) { cs[0][rp][cl + e] = gsum[e]; cs[1][rp][cl + e] = gsq[e]; }
        __syncthreads();
        if (tid < 64) {
            const int c = tid >> 5, g = tid & 31;
            if (p.gn_part[c]) {
                const int cpg = p.gn_cpg[c], base = p.gn_coff[c] + n0;
                const int lo = max(0, g * cpg - base), hi = min(min(SK_COLS, p.N - n0), (g + 1) * cpg - base);
                double sa = 0.0, sq = 0.0;
                for (int k = lo; k < hi; ++k)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { sa += (double)cs[0][r][k]; sq += (double)cs[1][r][k]; }
                const int b = m0 / p.gn_rows, mt = (m0 - b * p.gn_rows) / SKR;
                double* o = p.gn_part[c] + (((long long)b * p.gn_nch[c] + p.gn_slot[c] + mt * (int)gridDim.x + (int)blockIdx.x) * 32 + g) * 2;
                o[0] = sa;
                o[1] = sq;
            }
        }
    }
}

// Split-K second pass over FRAGMENT-ordered slabs (written by the direct-epilogue kernels, see there): one block = one 32-row stripe of one
// wave tile = TN waves, wave j owns the 32x32 block j of the stripe; lane (row lrow, half lhalf) sums its 16 columns over the z slices with
// contiguous-KiB loads, then does what the direct epilogue does: alpha, bias + per-sample vector, residual, 16-byte stores, and the fused
// GroupNorm statistics of the values as stored (slot = 32 rows x 32 TN columns).  act = NONE only (host).
template <typename TO, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(64 * TN) void splitk_reduce_frag_kernel(const GemmParams p) {
    constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    const int tid = threadIdx.x, lane = tid & 63, j = tid >> 6;
    const int lrow = lane & 31, lhalf = lane >> 5;
    const int tile = blockIdx.x, tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
    const int w = blockIdx.y / TM, i = blockIdx.y - w * TM, wm = w / WN, wn = w - wm * WN;
    const int row0 = tile_m * BM + (wm * TM + i) * 32, row = row0 + lrow;
    const int coln0 = tile_n * BN + wn * TN * 32;                    // first column of the stripe
    const int col = coln0 + j * 32 + lhalf * 16;
    const long long zstride = (long long)p.tiles_m * p.tiles_n * (BM * BN / 4);          // (16-byte units)
    const f32x4_t* src = (const f32x4_t*)p.ws + (long long)tile * (BM * BN / 4) + ((w * TM + i) * TN + j) * 256 + lane;
    f32x4_t a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = src[q * 64];
    for (int z = 1; z < p.splitk; ++z) {
        src += zstride;
        f32x4_t b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = src[q * 64];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += b[q];
    }
    const bool live = row < p.M && col < p.N;
    const bool gn_on = p.gn_rows > 0;
    constexpr int OV = sizeof(TO) == 2 ? 2 : 4, E = 16 / OV;
    float y[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) y[e] = 0.f;
    if (live) {
        TO* const dst = (TO*)p.out + (long long)row * p.ldo + col;
        const TO* const resp = p.residual ? (const TO*)p.residual + (long long)row * p.ldr + col : nullptr;
        const float* const rv = p.rowvec ? p.rowvec + (long long)(row / p.rows_per_sample) * p.ldv + col : nullptr;
        u32x4_t rq[OV];
        if (resp) {
#pragma unroll
            for (int h = 0; h < OV; ++h) rq[h] = ((const u32x4_t*)resp)[h];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4_t c = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) c = ((const f32x4_t*)(p.bias + col))[q];
            if (rv) c += ((const f32x4_t*)rv)[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[4 * q + e] = a[q][e] * p.alpha + c[e];
        }
#pragma unroll
        for (int h = 0; h < OV; ++h) {
            float f[E], v[E];
            if (resp) unpack16<TO>(rq[h], f);
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = y[h * E + e] + (resp ? f[e] : 0.0f);
            const u32x4_t wv = pack16<TO>(v);
            ((u32x4_t*)dst)[h] = wv;
            if (gn_on) {
                unpack16<TO>(wv, f);              // statistics of the values as stored
#pragma unroll
                for (int e = 0; e < E; ++e) y[h * E + e] = f[e];
            }
        }
    }
    if (gn_on) {
        __shared__ float gcs[2][32 * TN];             // column sums / sums of squares of the stripe
        float gx[32];
#pragma unroll
        for (int k = 0; k < 16; ++k) { gx[k] = y[k]; gx[16 + k] = y[k] * y[k]; }
        halfwave_reduce_scatter32(gx, lrow);          // (as in the direct epilogue)
        gcs[lrow >> 4][j * 32 + lhalf * 16 + (lrow & 15)] = gx[0];
        __syncthreads();
        if (tid < 64) {
            const int c = tid >> 5, g = tid & 31;
            // (a stripe of a ragged tile that lies beyond M or N has no slot: M < BM with split-K -- CFG off at the 8x8 level -- would otherwise
            //  write past the end of `partial`; slots are numbered by the GLOBAL 32 TN-column stripe, which is what the host sizes them by)
            if (p.gn_part[c] && row0 < p.M && coln0 < p.N) {
                const int cpg = p.gn_cpg[c], base = p.gn_coff[c] + coln0;            // consumer channel of the stripe's first column
                const int lo = max(0, g * cpg - base), hi = min(min(32 * TN, p.N - coln0), (g + 1) * cpg - base);
                double sa = 0.0, sq = 0.0;
                for (int k = lo; k < hi; ++k) { sa += (double)gcs[0][k]; sq += (double)gcs[1][k]; }
                const int b = row0 / p.gn_rows, mt = (row0 - b * p.gn_rows) / 32;
                const int nstripe = (p.N + 32 * TN - 1) / (32 * TN);
                double* o = p.gn_part[c] + (((long long)b * p.gn_nch[c] + p.gn_slot[c] + mt * nstripe + coln0 / (32 * TN)) * 32 + g) * 2;
                o[0] = sa;
                o[1] = sq;
            }
        }
    }
}

#ifdef RF_KERNEL_ONLY          // (diagnostics: tools/kernel_regs.sh compiles single instantiations of the kernels above)
}  // namespace rf
#else
// The launch of one planned part (gemm_plan.h: GemmPart) on tile GEMM_TILE[TI]: every kernel variant of (T, TO, tile, W8) is instantiated here, the
// plan picks among them.  Tile sizes, LDS sizes and what a tile can do are gemm_plan.h's constexpr functions, the same ones the planner ran.
template <typename T, typename TO, int TI, bool W8>
static int launch_cfg(const GemmPart& g, const GemmParams& p, bool conv, int batch, hipStream_t st) {
    constexpr GemmTile TILE = GEMM_TILE[TI];
    constexpr int WM = TILE.wm, WN = TILE.wn, TM = TILE.tm, TN = TILE.tn;
    constexpr GemmTypes TYPES{(int)sizeof(T), (int)sizeof(TO), W8, std::is_same<T, fp8_t>::value};
    constexpr bool A8 = TYPES.a8;
    constexpr int NST = 2, NSTD = tile_deep_stages(TILE, TYPES);
    constexpr int smem = tile_smem(TILE, TYPES), smem_hx = tile_smem_hx(TILE), smem_deep = tile_smem_deep(TILE, TYPES);
    constexpr bool HX_OK = tile_hx_ok(TILE, TYPES), DIRECT_OK = tile_direct_ok(TILE, TYPES), LN_OK = tile_ln_ok(TILE, TYPES);
    const bool deep = g.stages == 4, hx = g.hx;
    dim3 grid(p.tiles_m * p.tiles_n, batch, p.splitk), block(WM * WN * 64);
#define RF_LAUNCH_VARIANT_X(CONV_, GLDS_, EPI_, LNF_, HX_)                                                                      \
    {                                                                                                                            \
        constexpr int E_ = (EPI_ == 1 && DIRECT_OK) ? 1 : 0;                                                                     \
        if (GLDS_ && deep) {                                                                                                     \
            auto k = conv_gemm_kernel<T, TO, WM, WN, TM, TN, CONV_, GLDS_, (GLDS_ ? NSTD : 2), E_, (W8 && GLDS_), LNF_, false>; \
            RF_RAISE_LDS(k, smem_deep, "rf_conv_gemm");                                                                          \
            hipLaunchKernelGGL(k, grid, block, smem_deep, st, p);                                                                \
        } else {                                                                                                                 \
            auto k = conv_gemm_kernel<T, TO, WM, WN, TM, TN, CONV_, GLDS_, (GLDS_ ? NST : 2), E_, (W8 && GLDS_), LNF_, HX_>;    \
            constexpr int SM_ = HX_ ? smem_hx : smem;                                                                            \
            RF_RAISE_LDS(k, SM_, "rf_conv_gemm");                                                                                \
            hipLaunchKernelGGL(k, grid, block, SM_, st, p);                                                                      \
        }                                                                                                                        \
    }
#define RF_LAUNCH_VARIANT_LN(CONV_, GLDS_, EPI_, LNF_) RF_LAUNCH_VARIANT_X(CONV_, GLDS_, EPI_, LNF_, false)
#define RF_LAUNCH_VARIANT(CONV_, GLDS_, EPI_) RF_LAUNCH_VARIANT_LN(CONV_, GLDS_, EPI_, 0)
    const int esel = (g.direct || g.frag) ? 1 : 0;          // (fragment slabs are written by the direct-epilogue kernels)
    if constexpr (A8) {            // fp8 activations: direct-to-LDS kernels only, staged or direct epilogue
        if (conv) { if (esel == 1) RF_LAUNCH_VARIANT(true, true, 1) else RF_LAUNCH_VARIANT(true, true, 0) }
        else { if (esel == 1) RF_LAUNCH_VARIANT(false, true, 1) else RF_LAUNCH_VARIANT(false, true, 0) }
    } else
    if (conv && p.glds) {
        if (hx) {
            if constexpr (HX_OK) {          // (the planner checked it: korder 2 only reaches tiles that can take it)
                if (esel == 1) RF_LAUNCH_VARIANT_X(true, true, 1, 0, true)
                else RF_LAUNCH_VARIANT_X(true, true, 0, 0, true)
            }
        }
        else if (esel == 1) RF_LAUNCH_VARIANT(true, true, 1)
        else RF_LAUNCH_VARIANT(true, true, 0)
    } else if (conv) {
        RF_LAUNCH_VARIANT(true, false, 0)
    } else if (p.glds) {
        if (esel == 1) {
            // (LayerNorm roles: compile-time variants of the direct epilogue, bf16 linear layers only)
            if constexpr (LN_OK) {
                if (p.ln_in) RF_LAUNCH_VARIANT_LN(false, true, 1, 2)
                else if (p.ln_out) RF_LAUNCH_VARIANT_LN(false, true, 1, 1)
                else RF_LAUNCH_VARIANT(false, true, 1)
            } else RF_LAUNCH_VARIANT(false, true, 1)
        }
        else RF_LAUNCH_VARIANT(false, true, 0)
    } else {
        RF_LAUNCH_VARIANT(false, false, 0)
    }
#undef RF_LAUNCH_VARIANT
#undef RF_LAUNCH_VARIANT_LN
#undef RF_LAUNCH_VARIANT_X
    if (g.reduce == REDUCE_FRAG) {
        if constexpr (DIRECT_OK)
            hipLaunchKernelGGL((splitk_reduce_frag_kernel<TO, WM, WN, TM, TN>), dim3(p.tiles_m * p.tiles_n, WM * WN * TM), dim3(64 * TN), 0, st, p);
    } else if (g.reduce == REDUCE_STRIPE8)
        hipLaunchKernelGGL((splitk_reduce_kernel<TO, 8>), dim3((p.N + SK_COLS - 1) / SK_COLS, (p.M + 7) / 8), dim3(256), 0, st, p);
    else if (g.reduce == REDUCE_STRIPE32)
        hipLaunchKernelGGL((splitk_reduce_kernel<TO, 32>), dim3((p.N + SK_COLS - 1) / SK_COLS, (p.M + 31) / 32), dim3(256), 0, st, p);
    RF_LAUNCH_CHECK("rf_conv_gemm");
    return 0;
}

// The planned tile of an operand family -> its instantiation
template <typename T, typename TO, bool W8 = false>
static int launch_typed(const GemmPart& g, const GemmParams& p, bool conv, int batch, hipStream_t st) {
    switch (tile_index(g.tile)) {
    case 0:          // (fp8 x fp8 has no 256x320 tile: select_tile never picks it)
        if constexpr (!std::is_same<T, fp8_t>::value) return launch_cfg<T, TO, 0, W8>(g, p, conv, batch, st);
        break;
    case 1: return launch_cfg<T, TO, 1, W8>(g, p, conv, batch, st);
    case 2: return launch_cfg<T, TO, 2, W8>(g, p, conv, batch, st);
    case 3: return launch_cfg<T, TO, 3, W8>(g, p, conv, batch, st);
    case 4: return launch_cfg<T, TO, 4, W8>(g, p, conv, batch, st);
    case 5: return launch_cfg<T, TO, 5, W8>(g, p, conv, batch, st);
    case 6: return launch_cfg<T, TO, 6, W8>(g, p, conv, batch, st);
    }
    RF_CHECK(false, "rf_conv_gemm: no kernel for the planned %d x %d tile", tile_bm(g.tile), tile_bn(g.tile));
    return 1;
}

#ifdef RF_GEMM_F16_UNIT
// gemm_f16.hip: the fp16 (RF_F16) instantiations of the templates above as a compile unit of their own -- built beside gemm.hip instead of
// lengthening its four minutes of compile time by another two.  rf_conv_gemm and its planner stay in gemm.hip.
int launch_f16(GemmTypes e, const GemmPart& g, const GemmParams& p, bool conv, int batch, hipStream_t st) {
    if (e.so == 4) return launch_typed<f16_t, float>(g, p, conv, batch, st);
    return launch_typed<f16_t, f16_t>(g, p, conv, batch, st);
}
}  // namespace rf
#else
int launch_f16(GemmTypes e, const GemmPart& g, const GemmParams& p, bool conv, int batch, hipStream_t st);          // gemm_f16.hip
}  // namespace rf

extern "C" int rf_conv_gemm(const rf_conv_gemm_desc* d, void* stream) {
    using namespace rf;
    GemmParams p{}, q[2];
    GemmPlan pl;
    if (plan_conv_gemm(d, p, pl) != 0) return 1;
    // every part is planned and checked before the first one goes on the stream
    for (int i = 0; i < pl.nparts; ++i) {
        q[i] = part_params(d, p, pl.types, pl.part[i]);
        if (check_launch(d, q[i], pl.part[i]) != 0) return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const GemmTypes e = pl.types;
    const bool f32o = e.so == 4;
    for (int i = 0; i < pl.nparts; ++i) {
        const GemmPart& g = pl.part[i];
        int rc;
        if (d->dtype == RF_F16) rc = launch_f16(e, g, q[i], pl.conv, d->batch, st);
        else if (e.w8) rc = f32o ? launch_typed<bf16_t, float, true>(g, q[i], pl.conv, d->batch, st) : launch_typed<bf16_t, bf16_t, true>(g, q[i], pl.conv, d->batch, st);
        else if (e.a8) rc = launch_typed<fp8_t, bf16_t>(g, q[i], pl.conv, d->batch, st);
        else if (e.st == 4) rc = f32o ? launch_typed<float, float>(g, q[i], pl.conv, d->batch, st) : launch_typed<float, bf16_t>(g, q[i], pl.conv, d->batch, st);
        else rc = f32o ? launch_typed<bf16_t, float>(g, q[i], pl.conv, d->batch, st) : launch_typed<bf16_t, bf16_t>(g, q[i], pl.conv, d->batch, st);          // (also split-bf16: bf16 -> fp32)
        if (rc != 0) return rc;
    }
    return 0;
}

namespace rf {
// one block per weight row: amax -> power-of-two scale -> e4m3fn bytes (v_cvt_pk_fp8_f32: round-to-nearest-even, saturating)
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const float* __restrict__ w, int K, int ldq, uint8_t* __restrict__ q,
                                                                float* __restrict__ scale) {
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* row = w + (long long)n * K;
    float m = 0.f;
    for (int k = tid; k < K; k += 256) m = fmaxf(m, fabsf(row[k]));
    m = wave_max(m);
    __shared__ float sm[4];
    if ((tid & 63) == 0) sm[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    // smallest power of two s with m / s <= 448
    float s = 1.0f;
    if (m > 0.f) {
        int e;
        const float f = frexpf(m / 448.0f, &e);          // m / 448 = f * 2^e, f in [0.5, 1)
        s = ldexpf(1.0f, f == 0.5f ? e - 1 : e);
    }
    if (tid == 0) scale[n] = s;
    const float inv = 1.0f / s;                            // exact (power of two)
    uint8_t* qrow = q + (long long)n * ldq;
    for (int k4 = tid * 4; k4 < ldq; k4 += 1024) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (k4 + e < K) ? row[k4 + e] * inv : 0.f;
        int pk = 0;
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], pk, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], pk, true);
        *(int*)(qrow + k4) = pk;
    }
}
}  // namespace rf

extern "C" int rf_quantize_fp8_rows(const float* w, int N, int K, int ldq, void* q, float* scale, void* stream) {
    using namespace rf;
    RF_CHECK(w && q && scale && N > 0 && K > 0, "rf_quantize_fp8_rows: bad arguments");
    RF_CHECK(ldq >= K && ldq % 128 == 0 && (uintptr_t)q % 16 == 0, "rf_quantize_fp8_rows: ldq=%d must be a multiple of 128 >= K=%d", ldq, K);
    hipLaunchKernelGGL(quantize_fp8_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, w, K, ldq, (uint8_t*)q, scale);
    RF_LAUNCH_CHECK("rf_quantize_fp8_rows");
    return 0;
}

// The plan queries: the planner's answer as the words of include/reface_hip.h, no launch (a rejected call reports zeros)
static int plan_query(const rf_conv_gemm_desc* d, int32_t* words) {
    rf::GemmParams p{};
    rf::GemmPlan pl;
    const int rc = rf::plan_conv_gemm(d, p, pl);
    rf::plan_words(pl, p, words);
    return rc;
}

extern "C" int rf_conv_gemm_plan(const rf_conv_gemm_desc* d, int32_t* bm, int32_t* bn, int32_t* splitk) {
    using namespace rf;
    RF_CHECK(bm && bn && splitk, "rf_conv_gemm_plan: null output");
    int32_t w[RF_PLAN_WORDS];
    const int rc = plan_query(d, w);
    *bm = w[PW_STAT_ROWS]; *bn = w[PW_STAT_COLS]; *splitk = w[PW_SPLITK];
    return rc;
}

extern "C" int rf_conv_gemm_plan2(const rf_conv_gemm_desc* d, int32_t* info8) {
    using namespace rf;
    RF_CHECK(info8, "rf_conv_gemm_plan2: null output");
    int32_t w[RF_PLAN_WORDS];
    const int rc = plan_query(d, w);
    for (int i = 0; i < 8; ++i) info8[i] = w[i];
    return rc;
}

extern "C" int rf_conv_gemm_plan3(const rf_conv_gemm_desc* d, int32_t* info24) {
    using namespace rf;
    RF_CHECK(info24, "rf_conv_gemm_plan3: null output");
    return plan_query(d, info24);
}

#endif          // RF_GEMM_F16_UNIT
#endif          // RF_KERNEL_ONLY
