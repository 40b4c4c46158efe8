// rf_conv_gemm's planner: everything the host decides about a launch -- descriptor checks, kernel arguments, tile, split-K, tile order,
// epilogue form -- as plain C++17 without a HIP include.  gemm.hip compiles it into the library and launches what it plans;
// tests/gemm_plan_host_main.cpp compiles it with a host compiler under the sanitizers.  The tile arithmetic below is constexpr: the planner
// evaluates it at run time, the launcher as template arguments and LDS sizes of the kernels it instantiates.
#pragma once
#include <stdint.h>

#include "../../include/reface_hip.h"
#include "check.h"

namespace rf {

// The kernel-argument struct of conv_gemm_kernel and the split-K reduce kernels.  plan_conv_gemm fills everything but the six members a
// GemmPart decides (tiles_m, tiles_n, splitk, ws, pm, pn: part_params).
struct GemmParams {
    int M, N, K;
    const void* src0;
    const void* src1;
    int C0, Ctot, ld0, ld1;
    int Hin, Win, Hout, Wout, KH, KW, stride, pad_t, pad_l, ups;
    const void* W;
    int ldw;
    const float* bias;
    const float* rowvec;
    int rows_per_sample, ldv;
    const void* residual;
    int ldr, act;
    const float* act_vec;
    void* out;
    int ldo;
    float alpha;
    long long sA, sW, sO, sR;
    int tiles_m, tiles_n;
    unsigned a_bytes, w_bytes;   // extents of src0 / W (per batch element) for the buffer descriptors
    int glds;        // use the direct-to-LDS main loop
    int korder;      // 1: K is ordered (channel chunk of BK, tap, channel-in-chunk) instead of (tap, channel)
    int vec_ok;      // epilogue may use 16-byte (fp32) / 8-byte (bf16) vector accesses
    int splitk;      // > 1: blockIdx.z owns a K range and writes raw fp32 partial sums to `ws` (epilogue in splitk_reduce_kernel)
    float* ws;       // [splitk][M][N] fp32
    // fused GroupNorm statistics of `out` (rf_conv_gemm_desc.gn_*): up to two consumers with their own channel grouping
    int pm, pn;            // tile order inside an XCD's run: patches of pm x pn tiles (M-fastest inside a patch), patches N-fastest inside a super-row
                           // of pm tile rows.  (1, tiles_n) = N-fastest strips, (tiles_m, 1) = M-fastest strips; chosen per launch by estimated
                           // L2-miss traffic (plan_tile)
    int gn_rows;
    double* gn_part[2];
    int gn_cpg[2], gn_coff[2], gn_slot[2], gn_nch[2];
    int* plan;       // (placeholder, neither written nor read: it keeps the argument offsets of everything behind it)
    int epi2_ok;     // host only: operand alignment / feature set allow the direct (register -> global) epilogue
    const float* wscale;   // W8 kernels: per-output-channel power-of-two scale of the fp8 (e4m3fn) weights
    void* oscale;          // A8 kernels with GEGLU: `out` receives e4m3fn bytes (pitch ldo BYTES) and oscale one E8M0 code per (row, 32 output columns)
    int os_ld;
    const void* ascale;    // A8 kernels (fp8 activations): E8M0 scale bytes, one per (pixel, 32-channel block), pixel pitch as_ld bytes (a multiple of 4)
    int as_ld;
    unsigned as_bytes;
    // LayerNorm folded around two GEMMs (rf_conv_gemm_desc.ln_*).  Producer: per row and per 32 TN-column stripe of the wave tile, (mean, M2)
    // of the values as stored -> ln_out [M][ln_out_parts][2].  Consumer: out = rstd[m] (alpha acc - mean[m] ln_u[n]) + bias[n] with the row
    // statistics combined from ln_in's parts (Chan's formula); gamma rides in W, beta W^T in the bias (host).
    float* ln_out;
    int ln_out_parts;
    const float* ln_in;
    int ln_in_parts, ln_in_cols;
    float ln_eps;
    const float* ln_u;
    int x3;          // split-bf16 operands (RF_BF16X3): K counts VIRTUAL tiles, three per real 64-element K tile -- (A hi, W hi), (A hi, W lo),
                     // (A lo, W hi); W rows hold them in that order, the A lo plane lies lo_off bytes behind the hi plane of the same pixel
    int lo_off;
    long long w_ps;  // per-sample weights (rf_conv_gemm_desc.w_sample_stride, elements): the rows of sample s multiply W + s * w_ps; 0 = one W
    // centre-tap tail source (rf_conv_gemm_desc.srcx): K tiles [xt0, K / BK) read the channels of srcx at the output pixel; xt0 = 0x7fffffff: no tail
    const void* srcx;
    int ldx, xt0;
    unsigned x_bytes;
};

// ------------------------------------------------------------------------------------------------ tiles
// A block of wm x wn waves, each with a wave tile of tm x tn blocks of 32 x 32.
struct GemmTile { int wm, wn, tm, tn; };
constexpr int GEMM_TILES = 7;
constexpr GemmTile GEMM_TILE[GEMM_TILES] = {{4, 2, 2, 5}, {4, 2, 2, 4}, {4, 2, 1, 5}, {4, 2, 1, 4}, {4, 1, 1, 5}, {2, 2, 2, 2}, {4, 1, 1, 2}};
constexpr GemmTile TILE_256x320 = GEMM_TILE[0], TILE_256x256 = GEMM_TILE[1], TILE_128x320 = GEMM_TILE[2], TILE_128x256 = GEMM_TILE[3],
                   TILE_128x160 = GEMM_TILE[4], TILE_128x128 = GEMM_TILE[5], TILE_128x64 = GEMM_TILE[6];
// The element types of a kernel instantiation as far as a plan depends on them: bytes of an operand element (T) and of an output element (TO),
// fp8 weights under 16-bit activations (W8), fp8 x fp8 (A8 = T is fp8)
struct GemmTypes { int st, so; bool w8, a8; };

constexpr int tile_index(GemmTile t) {          // position in the list above (the launcher's switch)
    return t.wm * t.wn == 8 ? (t.tm == 2 ? (t.tn == 5 ? 0 : 1) : (t.tn == 5 ? 2 : 3)) : (t.tn == 5 ? 4 : (t.wn == 2 ? 5 : 6));
}
static_assert(tile_index(GEMM_TILE[0]) == 0 && tile_index(GEMM_TILE[1]) == 1 && tile_index(GEMM_TILE[2]) == 2 && tile_index(GEMM_TILE[3]) == 3 &&
              tile_index(GEMM_TILE[4]) == 4 && tile_index(GEMM_TILE[5]) == 5 && tile_index(GEMM_TILE[6]) == 6, "tile_index inverts GEMM_TILE");
constexpr int tile_bm(GemmTile t) { return 32 * t.tm * t.wm; }
constexpr int tile_bn(GemmTile t) { return 32 * t.tn * t.wn; }
constexpr int tile_waves(GemmTile t) { return t.wm * t.wn; }
constexpr int imax(int a, int b) { return a > b ? a : b; }
// LDS: two stages of (BM + BN) rows of 128 bytes in the main loop (3 stages of the big tiles at 1 block/CU measured slower), or the fp32 tile of the
// staged epilogue, in WM row chunks where it would not fit otherwise
constexpr int tile_smem_ep(GemmTile t) { return (tile_bm(t) / (tile_bm(t) * tile_bn(t) * 4 > 96 * 1024 ? t.wm : 1)) * tile_bn(t) * 4; }
constexpr int tile_smem(GemmTile t, GemmTypes e) { return imax(2 * (tile_bm(t) + tile_bn(t)) * 128 + (e.a8 ? 4096 : 0), tile_smem_ep(t)); }
// The 4-wave 128x160 tile also exists with a ring of 4 stages (147 KB: one block per CU), for grids of at most one block per CU
constexpr bool tile_deep_ok(GemmTile t, GemmTypes e) { return t.wm * t.wn == 4 && t.tm * t.tn == 5 && !e.w8 && !e.a8; }
constexpr int tile_deep_stages(GemmTile t, GemmTypes e) { return tile_deep_ok(t, e) ? 4 : 2; }
constexpr int tile_smem_deep(GemmTile t, GemmTypes e) { return imax(tile_deep_stages(t, e) * (tile_bm(t) + tile_bn(t)) * 128, tile_smem(t, e)); }
// HX (row-extended A tiles for 3x3 stride-1 convolutions, korder 2): bf16 -> bf16 / fp16 -> fp16 only; the stage of BM + BM / 4 rows must fit the 160 KB of LDS
constexpr int tile_hx_rpp(GemmTile t) { return t.wm * t.wn * 8; }
constexpr int tile_hx_rows(GemmTile t) { return ((tile_bm(t) * 5 / 4 + tile_hx_rpp(t) - 1) / tile_hx_rpp(t)) * tile_hx_rpp(t); }
constexpr int tile_smem_hx(GemmTile t) { return imax(2 * (tile_hx_rows(t) + tile_bn(t)) * 128, tile_smem_ep(t)); }
constexpr bool tile_hx_ok(GemmTile t, GemmTypes e) {
    return e.st == 2 && e.so == 2 && !e.w8 && !e.a8 && tile_smem_hx(t) <= 160 * 1024 && tile_hx_rows(t) / tile_hx_rpp(t) <= 8;
}
// The direct epilogue, and with it split-K through fragment-ordered slabs (splitk_reduce_frag_kernel), exists for the 8-wave tiles, the 128x160 tile
// and every fp8 x fp8 tile (whose GEGLU epilogue with fp8 output exists only in this form)
constexpr bool tile_direct_ok(GemmTile t, GemmTypes e) { return t.wm * t.wn == 8 || t.tm * t.tn == 5 || t.tm * t.tn >= 16 || e.a8; }
// LayerNorm folding lives in the direct epilogue only (16-bit linear layers: the LNF variants of the kernel)
constexpr bool tile_ln_ok(GemmTile t, GemmTypes e) { return tile_direct_ok(t, e) && e.st == 2 && e.so == 2 && !e.w8 && !e.a8; }

// split-K second pass (splitk_reduce_kernel): one block = SK_ROWS x SK_COLS of the output
constexpr int SK_ROWS = 32, SK_COLS = 256;
// Rows per reduce block: 32, or 8 when 32-row blocks would leave most of the chip idle (M = 1024 x N = 1280 is 160 blocks of 32 rows:
// 21 us for 39 MB of partial sums = 1.9 TB/s, 34 launches per step).
static inline int sk_rows_for(int M, int N) { return ((long long)((M + 31) / 32) * ((N + SK_COLS - 1) / SK_COLS) >= 512) ? 32 : 8; }

// ------------------------------------------------------------------------------------------------ the plan
enum GemmReduce { REDUCE_NONE = 0, REDUCE_STRIPE8 = 1, REDUCE_STRIPE32 = 2, REDUCE_FRAG = 3 };

// One GEMM kernel (+ its reduce pass) over the columns [n_off, n_off + n_len) of the call
struct GemmPart {
    int n_off, n_len;
    GemmTile tile;
    int tiles_m, tiles_n, splitk, pm, pn;
    bool direct, frag, hx;
    int stages;                  // LDS stages of the main loop: 2, or 4 for the ring
    int reduce;                  // GemmReduce
    int st_rows, st_cols;        // statistics tiling: the GEMM tile, or the reduce pass's tile when split-K moves the epilogue there
};
struct GemmPlan {
    int nparts = 0;              // 0: nothing planned (rejected); 2: a 256-wide launch whose last round of tiles is 20-60 % full, split along N
    GemmTypes types{};
    bool conv = false;           // convolution addressing (false: plain GEMM)
    GemmPart part[2]{};
};

// The words of rf_conv_gemm_plan3's info24 (include/reface_hip.h); _plan2 reports the first eight, _plan the first three.
enum GemmPlanWord {
    PW_STAT_ROWS, PW_STAT_COLS, PW_SPLITK, PW_BM, PW_BN, PW_WAVE_COLS, PW_DIRECT, PW_FLAGS /* bit 0 frag slabs, bit 1 two kernels */, PW_WAVES, PW_STAGES,
    PW_HX, PW_GLDS, PW_CONV, PW_LN_ROLE, PW_PM, PW_PN, PW_REDUCE, PW_TAIL_BM, PW_TAIL_BN, PW_TAIL_WAVES, PW_TILES_M, PW_TILES_N, PW_SPLIT_N, PW_TAIL_DIRECT,
    RF_PLAN_WORDS
};
static_assert(RF_PLAN_WORDS == 24, "rf_conv_gemm_plan3 reports 24 words");

// (a rejected call reports zeros -- or, when only the second part of a two-kernel split was rejected, the first part alone)
static inline void plan_words(const GemmPlan& pl, const GemmParams& p, int32_t* w) {
    for (int i = 0; i < RF_PLAN_WORDS; ++i) w[i] = 0;
    if (pl.nparts == 0) return;
    const GemmPart& g = pl.part[0];
    w[PW_STAT_ROWS] = g.st_rows; w[PW_STAT_COLS] = g.st_cols; w[PW_SPLITK] = g.splitk;
    w[PW_BM] = tile_bm(g.tile); w[PW_BN] = tile_bn(g.tile); w[PW_WAVE_COLS] = 32 * g.tile.tn;
    w[PW_DIRECT] = g.direct ? 1 : 0; w[PW_FLAGS] = (g.frag ? 1 : 0) | (pl.nparts == 2 ? 2 : 0);
    w[PW_WAVES] = tile_waves(g.tile); w[PW_STAGES] = g.stages; w[PW_HX] = g.hx ? 1 : 0;
    w[PW_GLDS] = p.glds ? 1 : 0; w[PW_CONV] = pl.conv ? 1 : 0; w[PW_LN_ROLE] = p.ln_in ? 2 : (p.ln_out ? 1 : 0);
    w[PW_PM] = g.pm; w[PW_PN] = g.pn; w[PW_REDUCE] = g.reduce; w[PW_TILES_M] = g.tiles_m; w[PW_TILES_N] = g.tiles_n;
    if (pl.nparts == 2) {
        const GemmPart& t = pl.part[1];
        w[PW_TAIL_BM] = tile_bm(t.tile); w[PW_TAIL_BN] = tile_bn(t.tile); w[PW_TAIL_WAVES] = tile_waves(t.tile);
        w[PW_SPLIT_N] = g.n_len; w[PW_TAIL_DIRECT] = t.direct ? 1 : 0;
    }
}

// The kernel arguments of one part: the call's, cut to the part's columns where there are two, with the members the part decides
static inline GemmParams part_params(const rf_conv_gemm_desc* d, const GemmParams& p, GemmTypes e, const GemmPart& g) {
    GemmParams q = p;
    if (g.n_len != p.N) {
        const int n_off = g.n_off, n_len = g.n_len;
        const int esw = e.w8 ? 1 : e.st;
        q.N = n_len;
        q.W = (const char*)p.W + (long long)n_off * p.ldw * esw;
        q.w_bytes = (unsigned)(e.w8 ? (long long)n_len * p.ldw : ((long long)(n_len - 1) * p.ldw + p.K) * esw);
        if (p.bias) q.bias = p.bias + n_off;
        if (p.rowvec) q.rowvec = p.rowvec + n_off;
        if (p.ln_u) q.ln_u = p.ln_u + n_off;
        if (p.wscale) q.wscale = p.wscale + n_off;
        if (p.act_vec) q.act_vec = p.act_vec + n_off;
        const int o_off = d->act == RF_ACT_GEGLU ? n_off / 2 : n_off;       // GEGLU: 32 value | 32 gate column blocks -> N / 2 output columns
        q.out = (char*)p.out + (long long)o_off * e.so;
        if (p.residual) q.residual = (const char*)p.residual + (long long)o_off * e.so;
    }
    q.tiles_m = g.tiles_m; q.tiles_n = g.tiles_n; q.splitk = g.splitk; q.pm = g.pm; q.pn = g.pn;
    if (g.splitk > 1) q.ws = (float*)d->workspace;
    return q;
}

// Split-K factor for a launch of `tiles` output tiles, by a two-term cost model: GEMM time at ~600 TFLOP/s stretched by the
// fraction of the 256 CUs left idle, plus the fp32 partial-sum traffic (write + re-read of sk * M * N floats at ~4 TB/s).
static inline int pick_splitk(const rf_conv_gemm_desc* d, const GemmParams& p, long long tiles, int bk) {
    const int nk = (p.K + bk - 1) / bk;
    if (!d->workspace || d->batch != 1 || d->act == RF_ACT_GEGLU || d->act == RF_ACT_ADD_RELU || tiles >= 200 || nk < 16) return 1;          // (ADD_RELU: the reduce passes act before the residual)
    int maxsk = nk / 8;
    if (maxsk > 16) maxsk = 16;
    const double t_gemm = 2.0 * p.M * p.N * (double)p.K / 6e14;
    int best = 1;
    double best_cost = 1e30;
    for (int sk = 1; sk <= maxsk; ++sk) {
        if ((long long)sk * p.M * p.N * 4 > d->workspace_bytes) break;
        // (more blocks than CUs: whole rounds -- 288 blocks of one block per CU are two rounds with the second 12 % full)
        const long long blocks = tiles * sk;
        const double fill = (double)blocks / (256.0 * (double)((blocks + 255) / 256));
        const double cost = t_gemm / fill + (sk > 1 ? (double)sk * p.M * p.N * 8.0 / 4e12 + 3e-6 : 0.0);
        if (cost < best_cost) { best_cost = cost; best = sk; }
    }
    return best;
}

// ------------------------------------------------------------------------------------------------ one kernel on one tile
// Everything a tile decides about the launch of `p` (the part's columns), and the rejections that depend on the tile.  Fills all of `g` but
// n_off / n_len.
static inline int plan_tile(const rf_conv_gemm_desc* d, const GemmParams& p, GemmTypes e, bool conv, GemmTile t, GemmPart& g) {
    const int BM = tile_bm(t), BN = tile_bn(t), WM = t.wm, WN = t.wn, TM = t.tm, TN = t.tn;
    const bool W8 = e.w8, A8 = e.a8;
    const bool DEEP_OK = tile_deep_ok(t, e), DIRECT_OK = tile_direct_ok(t, e);
    const int AXR_ = tile_hx_rows(t);
    const bool hx = p.korder == 2;
    g.tile = t;
    g.hx = hx;
    g.tiles_m = (p.M + BM - 1) / BM;
    g.tiles_n = (p.N + BN - 1) / BN;
    RF_CHECK(!p.w_ps || (p.rows_per_sample > 0 && p.rows_per_sample % BM == 0 && p.M % p.rows_per_sample == 0),
             "rf_conv_gemm: per-sample weights need rows_per_sample (%d) to be a multiple of the %d-row tile", p.rows_per_sample, BM);
    // split-K for launches that cannot fill the chip: each z-slice owns a K range, partial sums go through the caller's workspace
    g.splitk = pick_splitk(d, p, (long long)g.tiles_m * g.tiles_n, 128 / e.st);
    {
        // Tile order inside each XCD's contiguous run of tiles (8 XCDs, one 4 MB L2 each, 32 CUs): at any time the XCD works on ~`conc` consecutive
        // tiles of its run (x the K slices of split-K, which share nothing).  Estimated L2-miss bytes of a run ordered in pm x pn patches:
        // per super-row of pm tile rows the patches sweep along N -- the pm A panels stay resident if they fit beside the patch's pn W panels, the
        // W panels are streamed once per super-row unless all of W fits beside the A panels.  Strips along N (pm = 1) keep an A panel in one L2
        // (large images); strips along M (pn = 1) keep a W panel there -- at the 8x8 / 16x16 levels W is the big operand and N-fastest makes every
        // XCD stream ALL of it (1024 x 1280 x 11520: 239 MB instead of 69 MB through the fabric); wide layers at the 32x32 / 16x16 levels (GEGLU
        // 16384 x 5120 x 640: 20 W panels of 327 KB) want both bounded.
        const long long tiles = (long long)g.tiles_m * g.tiles_n, run = (tiles + 7) / 8;
        const double a_panel = (double)BM * (conv ? p.Ctot : p.K) * e.st, w_panel = (double)BN * p.K * (W8 ? 1 : e.st);
        // strips: the panels a run touches (the rule of rounds 2-4, kept as it was: every split-K and two-blocks-per-CU launch was tuned on it)
        const double n_mx = (double)((run + g.tiles_n - 1) / g.tiles_n + (run % g.tiles_n ? 1 : 0)), n_nx = (double)(run < g.tiles_n ? run : g.tiles_n);
        const double m_mx = (double)(run < g.tiles_m ? run : g.tiles_m), m_nx = (double)((run + g.tiles_m - 1) / g.tiles_m + (run % g.tiles_m ? 1 : 0));
        const double cost_n = n_mx * a_panel + n_nx * w_panel, cost_m = m_mx * a_panel + m_nx * w_panel;
        const bool mfast = cost_m < 0.8 * cost_n;
        int pm = mfast ? g.tiles_m : 1, pn = mfast ? 1 : g.tiles_n;
        // patches: only launches of several rounds of one 8-wave block per CU without split-K (measured, profiles/r05c_tile_order_fetch.txt: GEGLU
        // 16384 x 5120 x 640 296 -> 169 MB of fabric reads per launch, 4096 x 10240 x 1280 284 -> 243 MB and 129 -> 125 us, 4096 x 1280 x 5760
        // 346 -> 51 MB; the two-blocks-per-CU 128 x 160 launches and the split-K levels LOSE -- their whole run is in flight at once and the
        // dispatch-order neighbours that share an A panel stream it in step).  Estimated L2-miss bytes of a run: per super-row the patches sweep
        // along N -- the pm A panels stay resident if they fit beside the patch's pn W panels, the W panels are streamed once per super-row.
        // (bf16 / fp32 operands only: the fp8 x fp8 and fp8-weight kernels of configs[4] LOSE 3 % per batch on the same rule -- half the operand bytes per tile, other
        //  tile shapes; profiles/r05r_r04_vs_r05_same_box.txt)
        if (!W8 && !A8 && g.splitk == 1 && WM * WN == 8 && tiles >= 2 * 256) {
            const double conc = 32.0, cap = 3.0 * 1024 * 1024;          // tiles in flight per XCD; L2 bytes the operands may take (4 MB minus output lines)
            auto cost_of = [&](int h, int w) {
                const double nsr = (double)run / ((double)h * g.tiles_n) < 1.0 ? 1.0 : (double)run / ((double)h * g.tiles_n);          // super-rows per run
                const double npc = (double)g.tiles_n / w;                                                                            // patches per super-row
                const double a_t = (h * a_panel + w * w_panel <= cap) ? h * a_panel : npc * h * a_panel;
                return nsr * (a_t + g.tiles_n * w_panel);
            };
            double best = mfast ? cost_m : cost_n;
            const double strip_model = mfast ? cost_of(g.tiles_m, 1) : cost_of(1, g.tiles_n);
            if (strip_model > best) best = strip_model;
            for (int h = 2; h < g.tiles_m && h <= 32; h *= 2) {
                int w = (int)((conc + h - 1) / h);
                if (w < 1) w = 1;
                if (w >= g.tiles_n) continue;                        // (a full-width patch is the strip order)
                const double c = cost_of(h, w);
                if (c < 0.6 * best) { pm = h; pn = w; best = c / 0.6; }
            }
        }
        g.pm = pm;
        g.pn = pn;
    }
    // Split-K through fragment-ordered slabs (direct-epilogue kernels + splitk_reduce_frag_kernel): wherever the reduce pass has nothing to do
    // but alpha / bias / per-sample vector / residual (+ statistics) on 16-byte aligned rows
    g.frag = DIRECT_OK && g.splitk > 1 && p.glds && p.epi2_ok && d->act == RF_ACT_NONE && !p.oscale && d->batch == 1 &&
             (long long)g.splitk * g.tiles_m * g.tiles_n * BM * BN * 4 <= d->workspace_bytes;
    const int skr = sk_rows_for(p.M, p.N);
    g.st_rows = g.splitk > 1 ? (g.frag ? 32 : skr) : BM;
    g.st_cols = g.splitk > 1 ? (g.frag ? 32 * TN : SK_COLS) : BN;
    g.reduce = g.splitk > 1 ? (g.frag ? REDUCE_FRAG : (skr == 8 ? REDUCE_STRIPE8 : REDUCE_STRIPE32)) : REDUCE_NONE;
    if (W8 || A8) RF_CHECK(p.glds, "rf_conv_gemm: fp8 operands need the direct-to-LDS main loop (one source, K and channel count multiples of the K tile)");
    if (p.oscale)            // fp8 GEGLU output exists only in the direct epilogue: decided here so that rf_conv_gemm_plan reports it
        RF_CHECK(DIRECT_OK && TN % 2 == 0 && p.glds && p.epi2_ok && g.splitk == 1,
                 "rf_conv_gemm: fp8 output needs the direct epilogue (even TN, aligned rows, no split-K) -- this launch got a %d x %d tile", BM, BN);
    // Epilogue selection (timing decomposition + tools/bench_gemm.py A/B, r02c: the chunked fp32 staging costs 47 us of the 84 us
    // of the 65536x960x320 qkv GEMM).
    //   direct register -> global row segments: no LDS pass, no barriers; fastest wherever nothing needs the tile as a whole
    //          (qkv 86 -> 59 us, proj 33 -> 24, ff2 62 -> 52, GEGLU 196 -> 164).  8-wave tiles and the 128x160 tile.
    //   staged, the fp32 tile in row chunks: everything else (split-K partials, per-row timestep vectors, activations other than
    //          GEGLU, fp32 output with statistics, unaligned shapes).
    const bool ep_common = p.glds && p.epi2_ok && g.splitk == 1 && (!p.rowvec || p.rows_per_sample % BM == 0) &&
                           (d->act == RF_ACT_NONE || d->act == RF_ACT_ADD_RELU || (d->act == RF_ACT_GEGLU && TN % 2 == 0));
    const bool direct = g.direct = DIRECT_OK && ep_common && (p.gn_rows == 0 || d->act == RF_ACT_NONE);
    RF_CHECK(!hx || (tile_hx_ok(t, e) && conv && p.glds && p.KH == 3 && p.KW == 3 && p.stride == 1 && !p.ups && p.pad_t == 1 && p.pad_l == 1 && p.Hin == p.Hout &&
                     p.Win == p.Wout && p.Wout >= 16 && BM % p.Wout == 0 && (BM / p.Wout) * (p.Wout + 2) <= AXR_ &&
                     !(DEEP_OK && (long long)g.tiles_m * g.tiles_n * g.splitk <= 256)),
             "rf_conv_gemm: korder 2 (row-extended A tiles) needs a bf16 3x3 stride-1 pad-1 convolution, Wout >= 16, whose %d-row tile holds whole image rows (Wout = %d) "
             "and that does not take the 4-stage ring", BM, p.Wout);
    RF_CHECK(!(p.ln_out || p.ln_in) || (tile_ln_ok(t, e) && !conv),
             "rf_conv_gemm: LayerNorm folding needs a bf16 linear layer on a direct-epilogue tile (this launch: %d x %d, conv %d)", BM, BN, (int)conv);
    RF_CHECK(!p.ln_in || !d->residual, "rf_conv_gemm: a LayerNorm consumer takes no residual");
    RF_CHECK(!p.ln_out || (direct && d->act == RF_ACT_NONE && p.N % (32 * TN) == 0 && p.ln_out_parts == p.N / (32 * TN)),
             "rf_conv_gemm: ln_stats_out needs the direct epilogue (no split-K, act NONE) and ln_out_parts = N / %d (got %d; direct %d)", 32 * TN, p.ln_out_parts, (int)direct);
    RF_CHECK(!p.ln_in || (direct && p.ln_u && p.ln_in_parts >= 1 && p.ln_in_cols >= 1 && p.ln_eps > 0.f && BN <= 320),
             "rf_conv_gemm: ln_stats_in needs the direct epilogue (no split-K), ln_u, ln_in_parts / ln_in_cols >= 1 and ln_eps > 0 (direct %d)", (int)direct);
    RF_CHECK(p.ups != 2 || (g.splitk == 1 && (p.Hin * p.Win) % BM == 0),
             "rf_conv_gemm: ups 2 needs Hin * Win = %d to be a multiple of the %d-row tile (a tile inside one phase of one sample) and no split-K (this launch: %d)",
             p.Hin * p.Win, BM, g.splitk);
    // The ring of four stages for 128x160 launches of at most one block per CU (4096 x 1280 x K <= 6000: the projections, ff.net.2 and 1x1 skips
    // of the 16x16 level, 25 launches per step): nothing else covers the single tile of look-ahead there.  Alone (warm weights) it is neutral
    // (4096x1280x5120 68.3 -> 66.7 us); in situ, where every launch streams weights the previous ones pushed out of the caches, -0.9 % per batch
    // (tools/archive/exp_r03_10.sh: 921.7 -> 913.5 ms, same box, two runs each).  Forcing the 8x8 level (M = 1024) onto this tile + ring: neutral for the
    // 3x3 convs, +0.9 % for its small projections.
    const bool deep = DEEP_OK && p.glds && !p.x3 && !hx && (long long)g.tiles_m * g.tiles_n * d->batch * g.splitk <= 256;
    g.stages = deep ? tile_deep_stages(t, e) : 2;
    return 0;
}

// What only a real launch checks: rf_conv_gemm_plan answers before the caller has wired the statistics slots (it sizes them by the answer)
static inline int check_launch(const rf_conv_gemm_desc* d, const GemmParams& p, const GemmPart& g) {
    if (p.gn_rows > 0) {
        RF_CHECK(p.gn_rows % g.st_rows == 0 && p.M % p.gn_rows == 0 && d->batch == 1 && d->act != RF_ACT_GEGLU,
                 "rf_conv_gemm: fused GroupNorm statistics need gn_rows %% %d == 0 (%d), batch 1, no GEGLU -- ask rf_conv_gemm_plan", g.st_rows, p.gn_rows);
        const int need = (p.gn_rows / g.st_rows) * ((p.N + g.st_cols - 1) / g.st_cols);
        for (int c = 0; c < 2; ++c)
            RF_CHECK(!p.gn_part[c] || (p.gn_cpg[c] > 0 && p.gn_slot[c] >= 0 && p.gn_slot[c] + need <= p.gn_nch[c]),
                     "rf_conv_gemm: GroupNorm consumer %d: cpg=%d slot=%d needs %d slots of %d", c, p.gn_cpg[c], p.gn_slot[c], need, p.gn_nch[c]);
    }
    RF_CHECK(!p.oscale || g.direct, "rf_conv_gemm: fp8 output needs the direct epilogue (8-wave tile, aligned rows, no split-K)");
    return 0;
}

// ------------------------------------------------------------------------------------------------ tile selection
// The tile of a launch of `p`; *split_n > 0: as two kernels, the first over that many columns on the returned tile (a part is asked with
// split_n = nullptr: its partial round is below the 192 tiles at which the rule starts).
static inline GemmTile select_tile(const rf_conv_gemm_desc* d, const GemmParams& p, GemmTypes e, int* split_n) {
    const int N = p.N, bk = 128 / e.st;
    const bool geglu = d->act == RF_ACT_GEGLU;
    const long long mt256 = (p.M + 255) / 256, mt128 = (p.M + 127) / 128;
    if (e.a8) {
        // fp8 x fp8: 32-byte fragments (8 registers per 32-row block and k-step) leave no room for the 64-row wave tiles at two waves per
        // SIMD (they spill 260-940 bytes per lane): 128 x 320 / 128 x 256 blocks of 8 waves (wave tile 32 x 160 / 32 x 128), else the 4-wave tiles
        const bool n320 = !geglu && N % 320 == 0, n256 = N % 256 == 0 && !n320;
        const long long nt = n320 ? N / 320 : (n256 ? N / 256 : 0);
        if (n256 && mt256 * nt >= 192) return TILE_256x256;
        if (nt > 0 && mt128 * nt * pick_splitk(d, p, mt128 * nt, bk) >= 160) return n320 ? TILE_128x320 : TILE_128x256;
    } else if (p.glds && d->batch == 1) {
        // 8-wave blocks with 320- / 256-wide tiles: half the LDS and L2 traffic per FLOP of the 4-wave configs.  Take the tallest
        // tile (256 rows, wave tile 64 x 160 / 64 x 128) that still gives ~one block per CU, else the 128-row variant.
        bool n320 = !geglu && N % 320 == 0;
        if (n320 && N % 256 == 0 && mt256 * (N / 320) >= 192) {
            // both widths divide N: whole rounds of 256 blocks decide -- qkv of the 16x16 level (4096 x 3840) is 192 tiles of 256x320 (one
            // round, a quarter of the CUs idle) or 240 of 256x256
            const long long t320 = mt256 * (N / 320), t256 = mt256 * (N / 256);
            if (((t256 + 255) / 256) * 256 < ((t320 + 255) / 256) * 320) n320 = false;
        }
        const bool n256 = N % 256 == 0 && !n320;
        const long long nt = n320 ? N / 320 : (n256 ? N / 256 : 0);
        if (nt > 0) {
            if (mt256 * nt >= 192) {
                // wave quantisation: 288 tiles of 256 rows (M = 73728, the 96x96 level at B = 4) are two rounds with the second one
                // 12 % full; quarter-size tiles at two blocks per CU fill the tail (768^2 bench: GEMM family 17.32 -> 16.77 ms per step)
                // (also 1.5 rounds: qkv of the 32x32 level, 384 tiles -> 1536 quarter tiles = three full rounds at two blocks per CU; and the
                //  K = C projections with a residual at the 64x64 level -- 107 FLOP per byte of compulsory traffic, bandwidth-bound: two
                //  co-resident blocks keep loads, residual reads and stores of different tiles in flight together, 61 -> 48 us with cold
                //  operands; together -0.7 % per batch, tools/archive/exp_r03_14.sh)
                const double rounds = (double)(mt256 * nt) / 256.0, rfill = rounds / (double)((mt256 * nt + 255) / 256);
                // 256-wide tiles (GEGLU, N not a multiple of 320) whose last round is 20-60 % full -- 4096 x 10240 x 1280, the GEGLU projection of
                // the 16x16 level: 640 tiles = 2.5 rounds, three round times -- are split along N: the whole rounds on 256-row tiles, the columns of
                // the partial round as a second launch, which this dispatcher gives 128-row tiles (one full round of half-size tiles).  Launches
                // that carry nothing tile-numbered (no fused GroupNorm statistics, no LayerNorm producer role, no fp8 output, one W).
                const long long tiles_ = mt256 * nt, full_ = tiles_ / 256, rem_ = tiles_ - full_ * 256;
                // (... and whose tail still fills the chip with 8-wave 128-row tiles: smaller tails fall to 4-wave tiles without the direct epilogue a
                //  LayerNorm consumer needs)
                const long long tail_nt_ = full_ >= 1 && mt256 > 0 ? nt - full_ * 256 / mt256 : 0;
                if (split_n && !n320 && full_ >= 1 && rem_ * 5 >= 256 && rem_ * 5 <= 3 * 256 && (full_ * 256) % mt256 == 0 && mt128 * tail_nt_ >= 192 && p.gn_rows == 0 &&
                    !p.ln_out && !p.oscale && !p.w_ps && !p.x3 && p.ups != 2 && d->batch == 1 && (d->act == RF_ACT_NONE || d->act == RF_ACT_GEGLU)) {
                    *split_n = (int)(full_ * 256 / mt256) * 256;                       // columns of the whole rounds
                    return TILE_256x256;
                }
                if (n320 && (rfill < 0.6 || (rfill < 0.8 && rounds > 1.0) || (d->residual && p.K <= 320))) return TILE_128x160;
                return n320 ? TILE_256x320 : TILE_256x256;
            }
            // K up to ~90 tiles: two co-resident 4-wave 128x160 blocks per CU (each other's prologue / epilogue cover) beat one
            // 8-wave 128x320 block in situ (sweep: -1.2 % per batch at 6000, worse again from 11520).  Also when K is
            // too short for split-K to bring the 128x320 grid to size (4096 x 1280 x 1280: 23 us, against 26 us on 128x128 tiles).
            // (a launch with a tail source is judged by its WINDOW's K: 16384 x 640 x 5760 + 320..1920 stays on the tile the sweep above chose for
            //  the convolution it extends, instead of moving to 256x320 with split-K 2 -- partial sums the shorter loop never paid for)
            const int k_rule = p.xt0 != 0x7fffffff ? p.xt0 * bk : p.K;
            if (n320 && k_rule <= 6000 && mt128 * (N / 160) >= 256) return TILE_128x160;
            // 64-128 tiles of 256 rows (the 3x3 convs of the 16x16 level, the long-K N = 640 convs of the 32x32 level): split-K 2-4 over the
            // 256-row tiles rather than 128-row tiles -- the 64x160 wave tile's main loop runs 1.0-1.25 PF where the 32x160 one stays below
            // 0.95 (6 KB of fragment reads per 5 MFMAs), and the fragment-ordered slabs keep the partial sums cheap
            if (d->act == RF_ACT_NONE) {
                const long long blocks = mt256 * nt * pick_splitk(d, p, mt256 * nt, bk);
                if (blocks > mt256 * nt && blocks <= 4 * mt256 * nt && blocks >= 192 && blocks <= 256) return n320 ? TILE_256x320 : TILE_256x256;
            }
            if (mt128 * nt * pick_splitk(d, p, mt128 * nt, bk) >= 192) return n320 ? TILE_128x320 : TILE_128x256;
        }
    }
    if (geglu) return TILE_128x128;
    if (N <= 64) return TILE_128x64;
    const int pad128 = ((N + 127) / 128) * 128, pad160 = ((N + 159) / 160) * 160;
    return pad160 < pad128 ? TILE_128x160 : TILE_128x128;
}

// ------------------------------------------------------------------------------------------------ the whole call
// Descriptor checks, kernel arguments, tile selection and the per-tile plan of every part.  Returns 0 and a plan of one or two parts, or 1 with
// the reason in rf_last_error.
static inline int plan_conv_gemm(const rf_conv_gemm_desc* d, GemmParams& p, GemmPlan& pl) {
    pl = GemmPlan{};
    RF_CHECK(d != nullptr, "rf_conv_gemm: null descriptor");
    const bool oq = d->out_dtype == RF_FP8_E4M3;       // fp8 output + block scales (GEGLU of the fp8 x fp8 path)
    const bool x3 = d->dtype == RF_BF16X3;
    const bool h16 = d->dtype == RF_F16;             // fp16 operands: the bf16 kernels' geometry on v_mfma_f32_32x32x16_f16
    RF_CHECK(d->dtype == RF_F32 || d->dtype == RF_BF16 || h16 || x3 || d->dtype == RF_FP8_E4M3, "rf_conv_gemm: bad dtype %d", d->dtype);
    RF_CHECK(!h16 || ((d->out_dtype == RF_F16 || d->out_dtype == RF_F32) && d->w_dtype == 0),
             "rf_conv_gemm: fp16 operands write fp16 or fp32 and take fp16 weights (out_dtype %d, w_dtype %d)", d->out_dtype, d->w_dtype);
    RF_CHECK(d->out_dtype != RF_F16 || h16, "rf_conv_gemm: fp16 output needs fp16 operands (dtype %d)", d->dtype);
    RF_CHECK(d->dtype != RF_FP8_E4M3 || (d->w_dtype == RF_FP8_E4M3 && d->wscale && d->ascale && d->as_ld > 0 && d->as_ld % 4 == 0 && (d->out_dtype == RF_BF16 || oq) &&
                                         d->C1 == 0 && d->batch == 1 && d->korder == 0 && d->K % 128 == 0 && (d->C0 % 128 == 0 || (d->KH == 1 && d->KW == 1))),
             "rf_conv_gemm: fp8 activations need fp8 weights + wscale, ascale with a pitch that is a multiple of 4, bf16 output, one source, batch 1, "
             "K a multiple of 128 (zero-padded weights) and, for k x k windows, C0 a multiple of 128");
    RF_CHECK(!x3 || (d->out_dtype == RF_F32 && d->w_dtype == 0 && d->korder == 0 && d->C1 == 0 && d->batch == 1 && d->ld0 >= 2 * d->C0),
             "rf_conv_gemm: split-bf16 operands need fp32 output, one source with pixel pitch >= 2*C0, batch 1, tap-major K");
    RF_CHECK(d->out_dtype == RF_F32 || d->out_dtype == RF_BF16 || d->out_dtype == RF_F16 || oq, "rf_conv_gemm: bad out_dtype %d", d->out_dtype);
    RF_CHECK(!oq || (d->dtype == RF_FP8_E4M3 && d->act == RF_ACT_GEGLU && d->oscale && d->os_ld >= d->N / 64 && !d->residual && d->N % 64 == 0),
             "rf_conv_gemm: fp8 output is the GEGLU epilogue of the fp8 x fp8 path (oscale, no residual, N a multiple of 64)");
    const bool a8 = d->dtype == RF_FP8_E4M3;           // fp8 activations + E8M0 block scales x fp8 weights (MX-scaled MFMA)
    const int vec = d->dtype == RF_F32 ? 4 : (a8 ? 16 : 8);
    const int ctot = d->C0 + d->C1;
    RF_CHECK(d->M > 0 && d->N > 0 && d->K > 0 && d->batch >= 1, "rf_conv_gemm: bad sizes M=%d N=%d K=%d batch=%d", d->M, d->N, d->K, d->batch);
    RF_CHECK(d->src0 && d->W && d->out, "rf_conv_gemm: null operand");
    RF_CHECK(d->K % vec == 0 && ctot % vec == 0 && d->C0 % vec == 0 && d->ld0 % vec == 0,
             "rf_conv_gemm: K=%d C0=%d C1=%d ld0=%d must be multiples of %d", d->K, d->C0, d->C1, d->ld0, vec);
    RF_CHECK(d->C1 == 0 || (d->src1 && d->ld1 % vec == 0), "rf_conv_gemm: bad second source");
    const bool w8 = d->w_dtype == RF_FP8_E4M3 && d->dtype != RF_FP8_E4M3;          // W8A16: fp8 weights dequantised to bf16 in the fragment path
    RF_CHECK(d->w_dtype == 0 || d->w_dtype == RF_FP8_E4M3, "rf_conv_gemm: bad w_dtype %d", d->w_dtype);
    RF_CHECK(!w8 || (d->dtype == RF_BF16 && d->wscale && d->ldw % 128 == 0 && d->ldw >= d->K && d->batch == 1 && d->korder == 0),
             "rf_conv_gemm: fp8 weights need bf16 activations, wscale, batch 1 and ldw (bytes) a multiple of 128 >= K (ldw=%d K=%d)", d->ldw, d->K);
    RF_CHECK(w8 || d->ldw == 0 || (d->ldw >= (x3 ? 3 : 1) * d->K && d->ldw % vec == 0), "rf_conv_gemm: bad ldw=%d", d->ldw);
    RF_CHECK(!a8 || (d->ldw % 128 == 0 && d->ldw >= d->K), "rf_conv_gemm: fp8 x fp8 needs ldw (bytes) a multiple of 128 >= K");
    RF_CHECK(d->KH >= 1 && d->KW >= 1 && d->stride >= 1, "rf_conv_gemm: bad window");
    // centre-tap tail source: Cx more K elements behind the window's (kwin = the window's share of K)
    const bool xt = d->srcx != nullptr;
    RF_CHECK(!xt || ((d->dtype == RF_BF16 || h16) && d->w_dtype == 0 && d->batch == 1 && d->C1 == 0),
             "rf_conv_gemm: a tail source (srcx) needs bf16 / fp16 operands and weights, one window source and batch 1 (dtype %d, w_dtype %d, C1 %d, batch %d)",
             d->dtype, d->w_dtype, d->C1, d->batch);
    RF_CHECK(!xt || (d->stride == 1 && d->ups == 0 && d->Hin == d->Hout && d->Win == d->Wout && d->KH * d->KW > 1),
             "rf_conv_gemm: a tail source (srcx) needs a k x k window with stride 1, no ups and Hin x Win = Hout x Wout (stride %d, ups %d, %dx%d -> %dx%d)",
             d->stride, d->ups, d->Hin, d->Win, d->Hout, d->Wout);
    RF_CHECK(!xt || (d->Cx > 0 && d->Cx % (8 * vec) == 0 && d->Cx < d->K && d->ldx >= d->Cx && d->ldx % vec == 0 && (uintptr_t)d->srcx % 16 == 0),
             "rf_conv_gemm: tail source: Cx=%d must be a multiple of %d below K=%d, ldx=%d a multiple of %d >= Cx, srcx 16-byte aligned", d->Cx, 8 * vec, d->K, d->ldx, vec);
    const int kwin = xt ? d->K - d->Cx : d->K;
    RF_CHECK(!xt || kwin == d->KH * d->KW * ctot, "rf_conv_gemm: with a tail source K=%d must be KH*KW*C0 + Cx = %d", d->K, d->KH * d->KW * ctot + d->Cx);
    RF_CHECK(d->KH * d->KW * ctot <= kwin && kwin < d->KH * d->KW * ctot + 8 * vec,
             "rf_conv_gemm: K=%d inconsistent with KH*KW*(C0+C1)=%d", d->K, d->KH * d->KW * ctot);
    RF_CHECK(((uintptr_t)d->src0 | (uintptr_t)d->src1 | (uintptr_t)d->W) % 16 == 0, "rf_conv_gemm: operands must be 16-byte aligned");
    RF_CHECK(d->act != RF_ACT_GEGLU || (d->N % 64 == 0 && !d->rowvec), "rf_conv_gemm: GEGLU needs N %% 64 == 0 and no rowvec");
    RF_CHECK(!d->rowvec || d->rows_per_sample > 0, "rf_conv_gemm: rowvec needs rows_per_sample");
    RF_CHECK(d->korder == 0 || ((d->korder == 1 || d->korder == 2) && ctot % (8 * vec) == 0 && kwin == d->KH * d->KW * ctot),
             "rf_conv_gemm: korder=%d needs (C0+C1) to be a multiple of %d", d->korder, 8 * vec);
    RF_CHECK(d->korder != 2 || ((d->dtype == RF_BF16 || h16) && d->out_dtype == d->dtype && d->w_dtype == 0 && d->C1 == 0 && d->batch == 1),
             "rf_conv_gemm: korder=2 (row-extended A tiles) is built for bf16 -> bf16 / fp16 -> fp16 convolutions of one source");
    RF_CHECK(d->act != RF_ACT_PRELU || d->act_vec, "rf_conv_gemm: PReLU needs act_vec (per-column slopes)");
    RF_CHECK(d->act >= RF_ACT_NONE && d->act <= RF_ACT_ADD_RELU, "rf_conv_gemm: bad act %d", d->act);
    RF_CHECK(d->act != RF_ACT_ADD_RELU || (!d->ln_stats_in && !d->ln_stats_out && !oq),
             "rf_conv_gemm: ReLU after the residual (RF_ACT_ADD_RELU) does not combine with LayerNorm folding or fp8 output");
    const bool conv = !(d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad_t == 0 && d->pad_l == 0 && d->ups == 0 &&
                        d->C1 == 0 && d->Hin == d->Hout && d->Win == d->Wout);
    RF_CHECK(!conv || d->batch == 1, "rf_conv_gemm: batch > 1 only for plain GEMM");
    RF_CHECK(!conv || (d->Hout > 0 && d->Wout > 0 && d->M % (d->Hout * d->Wout) == 0), "rf_conv_gemm: M not a multiple of Hout*Wout");
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.src0 = d->src0; p.src1 = d->src1;
    p.C0 = d->C0; p.Ctot = ctot; p.ld0 = d->ld0; p.ld1 = d->ld1;
    p.Hin = d->Hin; p.Win = d->Win; p.Hout = d->Hout; p.Wout = d->Wout;
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad_t = d->pad_t; p.pad_l = d->pad_l; p.ups = d->ups;
    p.W = d->W; p.ldw = d->ldw > 0 ? d->ldw : (x3 ? 3 : 1) * d->K; p.bias = d->bias; p.rowvec = d->rowvec; p.rows_per_sample = d->rows_per_sample; p.ldv = d->ldv;
    p.residual = d->residual; p.ldr = d->ldr; p.act = d->act; p.act_vec = d->act_vec; p.out = d->out; p.ldo = d->ldo; p.alpha = d->alpha;
    p.sA = d->sA; p.sW = d->sW; p.sO = d->sO; p.sR = d->sR;
    p.gn_rows = (d->gn_part0 || d->gn_part1) ? d->gn_rows : 0;
    p.gn_part[0] = d->gn_part0; p.gn_cpg[0] = d->gn_cpg0; p.gn_coff[0] = d->gn_coff0; p.gn_slot[0] = d->gn_slot0; p.gn_nch[0] = d->gn_nchunks0;
    p.gn_part[1] = d->gn_part1; p.gn_cpg[1] = d->gn_cpg1; p.gn_coff[1] = d->gn_coff1; p.gn_slot[1] = d->gn_slot1; p.gn_nch[1] = d->gn_nchunks1;
    p.ln_out = (float*)d->ln_stats_out; p.ln_out_parts = d->ln_out_parts;
    p.ln_in = (const float*)d->ln_stats_in; p.ln_in_parts = d->ln_in_parts; p.ln_in_cols = d->ln_in_cols; p.ln_eps = d->ln_eps; p.ln_u = d->ln_u;
    RF_CHECK(!(p.ln_out || p.ln_in) || ((d->dtype == RF_BF16 || h16) && d->out_dtype == d->dtype && d->batch == 1 && !(p.ln_out && p.ln_in)),
             "rf_conv_gemm: LayerNorm folding is built for bf16 / fp16 GEMMs (batch 1, one role per launch)");
    RF_CHECK(!(d->gn_part0 || d->gn_part1) || d->gn_rows > 0, "rf_conv_gemm: gn_part set but gn_rows = %d", d->gn_rows);
    {
        const uintptr_t oa = d->out_dtype == RF_F32 ? 16 : 8;
        p.oscale = oq ? d->oscale : nullptr;
        p.os_ld = d->os_ld;
        const int nout = d->act == RF_ACT_GEGLU ? d->N / 2 : d->N;
        bool ok = (d->N % 4 == 0) && (nout % 4 == 0) && (d->ldo % 4 == 0) && ((uintptr_t)d->out % oa == 0) && (d->sO % 4 == 0);
        if (d->residual) ok = ok && (d->ldr % 4 == 0) && ((uintptr_t)d->residual % oa == 0) && (d->sR % 4 == 0);
        if (d->bias) ok = ok && ((uintptr_t)d->bias % 16 == 0);
        if (d->rowvec) ok = ok && (d->ldv % 4 == 0) && ((uintptr_t)d->rowvec % 16 == 0);
        p.vec_ok = ok ? 1 : 0;
        // direct epilogue: 16 contiguous output columns per lane, written / read as 16-byte vectors
        const int es_o = d->out_dtype == RF_F32 ? 4 : (oq ? 1 : 2);
        bool e2 = (d->N % 16 == 0) && (nout % 16 == 0) && ((long long)d->ldo * es_o % 16 == 0) && ((uintptr_t)d->out % 16 == 0) &&
                  ((long long)d->sO * es_o % 16 == 0) && d->act != RF_ACT_PRELU;
        if (d->residual) e2 = e2 && ((long long)d->ldr * es_o % 16 == 0) && ((uintptr_t)d->residual % 16 == 0) && ((long long)d->sR * es_o % 16 == 0);
        if (d->bias) e2 = e2 && ((uintptr_t)d->bias % 16 == 0);
        if (d->rowvec) e2 = e2 && (d->ldv % 4 == 0) && ((uintptr_t)d->rowvec % 16 == 0);
        p.epi2_ok = e2 ? 1 : 0;
    }
    {
        // direct-to-LDS main loop needs one source, 31-bit byte offsets ...
        const long long es = d->dtype == RF_F32 ? 4 : (a8 ? 1 : 2);
        const long long rows_a = conv ? (long long)(d->M / (d->Hout * d->Wout)) * d->Hin * d->Win : d->M;
        const long long ab = ((rows_a - 1) * d->ld0 + (conv ? d->C0 : d->K) + (x3 ? d->C0 : 0)) * es;
        const long long wb = (w8 || a8) ? (long long)d->N * p.ldw : ((long long)(d->N - 1) * p.ldw + (x3 ? 3 : 1) * d->K) * es;
        // ... and K tiles that never straddle a filter tap (uniform K offset per tile; rows packed as sample:12 | oy:10 | ox:10)
        const int bk = (int)(128 / es);
        const bool uniform = d->K % bk == 0 && (!conv || (ctot % bk == 0 && kwin == d->KH * d->KW * ctot &&
                                                         d->Hout <= 1024 && d->Wout <= 1024 && d->M / (d->Hout * d->Wout) < 4095));
        const long long xb = xt ? ((rows_a - 1) * d->ldx + d->Cx) * es : 0;
        p.glds = (d->C1 == 0 && uniform && ab < 0x7fff0000LL && wb < 0x7fff0000LL && xb < 0x7fff0000LL) ? 1 : 0;
        RF_CHECK(!xt || (conv && p.glds), "rf_conv_gemm: a tail source (srcx) needs the direct-to-LDS main loop (C0 a multiple of the K tile, 31-bit operand extents)");
        p.srcx = d->srcx; p.ldx = d->ldx;
        p.xt0 = xt ? kwin / bk : 0x7fffffff;
        p.x_bytes = (unsigned)xb;
        p.korder = d->korder;
        p.a_bytes = (unsigned)(p.glds ? ab : 0);
        p.w_bytes = (unsigned)(p.glds ? wb : 0);
        p.ascale = d->ascale; p.as_ld = d->as_ld;
        p.as_bytes = (unsigned)(a8 ? rows_a * d->as_ld : 0);
        p.x3 = x3 ? 1 : 0;
        p.lo_off = x3 ? d->C0 * 2 : 0;
        p.w_ps = d->w_sample_stride;
        RF_CHECK(d->w_sample_stride == 0 || (!conv && !w8 && !a8 && !x3 && d->batch == 1 && d->rows_per_sample > 0 && p.glds &&
                                             d->w_sample_stride >= (long long)(d->N - 1) * p.ldw + d->K),
                 "rf_conv_gemm: w_sample_stride needs a plain bf16 / fp32 GEMM on the direct-to-LDS loop, batch 1, rows_per_sample > 0 and a stride of at least one W");
        if (x3) {
            RF_CHECK(p.glds && (conv || d->C0 == d->K), "rf_conv_gemm: split-bf16 operands need the direct-to-LDS main loop (K and channel count multiples of 64) and C0 == K for plain GEMMs");
            p.K = 3 * d->K;          // virtual K: three passes per real K tile
        }
    }
    // ups == 2: nearest-2x upsampling folded into four 2x2 phase filters (W = [4][N][ldw], rows ordered (sample, phase, source pixel)); lives on the
    // direct-to-LDS loop of the 16-bit kernels alone (the tile condition -- Hin Win a multiple of the tile rows, no split-K -- is plan_tile's)
    RF_CHECK(d->ups >= 0 && d->ups <= 2, "rf_conv_gemm: bad ups %d (0 none, 1 nearest x2 in the addressing, 2 nearest x2 folded into 2x2 phase weights)", d->ups);
    if (d->ups == 2) {
        RF_CHECK((d->dtype == RF_BF16 || h16) && d->w_dtype == 0, "rf_conv_gemm: ups 2 needs bf16 / fp16 operands and weights (dtype %d, w_dtype %d)", d->dtype, d->w_dtype);
        RF_CHECK(d->KH == 2 && d->KW == 2 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1,
                 "rf_conv_gemm: ups 2 needs KH = KW = 2, stride 1 and pad_t = pad_l = 1, the padding of phase (0, 0) (got %dx%d, stride %d, pad %d %d)", d->KH, d->KW, d->stride, d->pad_t, d->pad_l);
        RF_CHECK(d->Hout == 2 * d->Hin && d->Wout == 2 * d->Win, "rf_conv_gemm: ups 2 needs Hout x Wout = 2 Hin x 2 Win (%dx%d -> %dx%d)", d->Hin, d->Win, d->Hout, d->Wout);
        RF_CHECK(d->C1 == 0 && d->batch == 1, "rf_conv_gemm: ups 2 needs one source and batch 1 (C1 %d, batch %d)", d->C1, d->batch);
        RF_CHECK(!xt && !d->residual && !d->rowvec && !d->ln_stats_in && !d->ln_stats_out && d->w_sample_stride == 0 && d->act != RF_ACT_GEGLU,
                 "rf_conv_gemm: ups 2 takes no tail source (srcx), residual, rowvec, LayerNorm fold, per-sample weights or GEGLU");
        RF_CHECK(d->korder == 0 || d->korder == 1, "rf_conv_gemm: ups 2 needs korder 0 or 1 (got %d)", d->korder);
        RF_CHECK(p.glds, "rf_conv_gemm: ups 2 needs the direct-to-LDS main loop (C0 = %d a multiple of 64, 31-bit operand extents)", d->C0);
    }
    p.wscale = d->wscale;
    // the kernels' element types: fp8 weights and split-bf16 operands ride the bf16 kernels, fp8 x fp8 writes bf16 (or fp8 bytes through the same kernels)
    const int so = d->out_dtype == RF_F32 ? 4 : 2;
    GemmTypes e;
    if (w8) e = GemmTypes{2, so, true, false};
    else if (x3) e = GemmTypes{2, 4, false, false};
    else if (h16) e = GemmTypes{2, so, false, false};
    else if (a8) e = GemmTypes{1, 2, false, true};
    else {
        RF_CHECK(d->out_dtype != RF_F16, "rf_conv_gemm: fp16 output needs fp16 operands");
        e = GemmTypes{d->dtype == RF_F32 ? 4 : 2, so, false, false};
    }
    pl.types = e;
    pl.conv = conv;
    int n1 = 0;
    const GemmTile t1 = select_tile(d, p, e, &n1);
    GemmPart& g1 = pl.part[0];
    g1.n_off = 0;
    g1.n_len = n1 ? n1 : p.N;
    // (a part is planned against its own columns: tiles, split-K and the tile order of N = n_len)
    if (plan_tile(d, part_params(d, p, e, g1), e, conv, t1, g1) != 0) return 1;
    pl.nparts = 1;
    if (n1) {
        // BOTH parts must be launchable (a LayerNorm consumer needs the direct epilogue in the tail too): a query validates the tail here, not
        // the first replay, and a launch before anything is on the stream
        GemmPart& g2 = pl.part[1];
        g2.n_off = n1;
        g2.n_len = p.N - n1;
        const GemmParams q2 = part_params(d, p, e, g2);
        if (plan_tile(d, q2, e, conv, select_tile(d, q2, e, nullptr), g2) != 0) return 1;
        pl.nparts = 2;
    }
    return 0;
}

}  // namespace rf
