// Baseline-JPEG decoding on the device (the callers' --gpu_jpeg_decode and --video_in; reface_amd/jpegdec.py parses the markers, builds the
// tables and uploads the scans of a batch).
//   rf_jpeg_entropy_decode    scan -> int16 coefficients [blocks, 64], natural order, blocks in scan order.  One LANE per restart interval
//                             (csrc/jpeg_decode.h, shared with the host test program); a file without DRI is one interval.  `lanes` of
//                             the 64 lanes of a wave are used, so that a small batch spreads over the CUs instead of sharing one wave.
//   rf_jpeg_idct_u8           dequantise + libjpeg's jpeg_idct_islow, 8 lanes per block: lane c takes column c, the workspace crosses
//                             through LDS, lane r takes row r and stores its 8 samples as one 8-byte word.
//   rf_jpeg_upsample_rgb_u8   one lane per pixel: libjpeg's fancy (triangle) chroma upsampling and its 16-bit YCbCr -> RGB.
//   rf_jpeg_selfsync_decode   the self-synchronising plan of files without DRI (csrc/jpeg_sync.h): one lane per sub-sequence of L bytes.
//                             `launches` x jpeg_sync_kernel (a workgroup = 64 sub-sequences of one file iterates to its own fixed point
//                             in LDS, publishes its outgoing boundary state and returns at once when its incoming state is the one it last
//                             ran with), jpeg_sync_scan_kernel (first block of every sub-sequence; a file whose last launch still moved a
//                             boundary is flagged), jpeg_sync_write_kernel (coefficients, DC differences), jpeg_sync_dc_kernel (DC prefix
//                             sums per component) and one more jpeg_entropy_decode_kernel in which the serial lane decodes flagged files.
//                             No kernel waits for another workgroup: every one ends on its own bounds whatever the data.
// All arithmetic is 32-bit integer.  Plain vector stores and ordinary atomics only.
#include "common.h"
#include "jpeg_sync.h"

namespace rf {
using namespace jpgdec;

__global__ __launch_bounds__(64) void jpeg_entropy_decode_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, const int* __restrict__ ivl,
                                                                 int nivl, int lanes, int16_t* __restrict__ coef, int* __restrict__ status, int fallback) {
    if ((int)threadIdx.x >= lanes) return;
    const long long g = (long long)blockIdx.x * lanes + threadIdx.x;
    if (g >= nivl) return;
    const int f = ivl[g];
    const long long* d = desc + (long long)f * DESC;
    // a file of the selfsync plan is not this launch's; in the launch appended behind that plan the lane decodes it if it was flagged
    if ((d[D_SS_COUNT] > 0) != (fallback != 0) || (fallback && !(status[2 * f + 1] & ST_FALLBACK))) return;
    const long long k = g - d[D_IVL_BEGIN], found = d[D_IVL_COUNT];
    const Geometry geo = geometry((int)d[D_H], (int)d[D_W], (int)d[D_NCOMP], (int)d[D_HS], (int)d[D_VS]);
    const long long expected = geo.intervals(d[D_RI]);
    const uint8_t* scan = comp + d[D_SCAN_OFF];
    const int* starts = ivl + nivl + d[D_IVL_BEGIN];
    if (k == 0 && !fallback) status[2 * f + 1] = d[D_RI] > 0 ? 1 : 0;
    int rc = check_interval(scan, starts, k, found, expected);
    if (rc == OK) {
        const uint32_t begin = (uint32_t)starts[k];
        const uint32_t end = k + 1 < found ? (uint32_t)starts[k + 1] - 2u : (uint32_t)d[D_SCAN_LEN];
        rc = decode_interval(scan, begin, end, d, comp + d[D_TAB_OFF], k, coef + d[D_COEF_OFF] * 64);
    }
    if (rc != OK) atomicCAS(&status[2 * f], 0, rc);          // the first code stays
}

// ------------------------------------------------------------------------------------------------ the selfsync plan (csrc/jpeg_sync.h)
// The work buffer of a batch with S sub-sequences in G workgroups: the states (slot i = the state sub-sequence i starts from; written by
// the lane of i - 1 alone), the incoming state every workgroup last ran with, the lowest (sub-sequence << 8 | code) of a file's write
// pass, the first block of every sub-sequence, its block count, and a "a boundary moved" word per file and launch.
struct SsWork {
    uint64_t* state;
    uint64_t* seen;
    unsigned long long* err;
    long long* first;
    int* cnt;
    int* chg;
};
static SsWork ss_work(void* base, int64_t S, int64_t G, int64_t B) {
    SsWork w;
    w.state = (uint64_t*)base;
    w.seen = w.state + S;
    w.err = (unsigned long long*)(w.seen + G);
    w.first = (long long*)(w.err + B);
    w.cnt = (int*)(w.first + S);
    w.chg = w.cnt + S;
    return w;
}
static int64_t ss_work_bytes(int64_t S, int64_t G, int64_t B) { return 8 * (S + G + B + S) + 4 * (S + B * SS_MAX_LAUNCHES); }

__device__ __forceinline__ uint64_t ss_load(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ss_store(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the file's 8 Huffman tables into LDS: 7296 bytes = 1824 words, 29 per lane
__device__ __forceinline__ void ss_stage_tables(HuffTab* tabs, const uint8_t* __restrict__ comp, const long long* d, int lane, int lanes) {
    const uint32_t* src = (const uint32_t*)(comp + d[D_TAB_OFF] + QUANT_BYTES);          // tab_off is a multiple of 16
    uint32_t* dst = (uint32_t*)tabs;
    for (int i = lane; i < 8 * (int)sizeof(HuffTab) / 4; i += lanes) dst[i] = src[i];
    __syncthreads();
}

// One workgroup = sub-sequences [64 x, 64 x + 64) of file y.  A Jacobi pass evaluates F for every lane whose input moved; 64 passes
// reach the workgroup's fixed point from any start, because pass t makes the input of lane t final.
__global__ __launch_bounds__(SS_LANES) void jpeg_sync_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, SsWork w, int launch) {
    __shared__ HuffTab tabs[8];
    __shared__ uint64_t sh[SS_LANES + 1];
    const int f = blockIdx.y, lane = threadIdx.x;
    const long long* d = desc + (long long)f * DESC;
    const long long n = d[D_SS_COUNT], g0 = (long long)blockIdx.x * SS_LANES, gi = g0 + lane;
    if (g0 >= n || d[D_IVL_COUNT] != 1) return;
    const uint64_t L = (uint64_t)d[D_SS_BYTES];
    const uint32_t len = (uint32_t)d[D_SCAN_LEN];
    const uint8_t* scan = comp + d[D_SCAN_OFF];
    uint64_t* st = w.state + d[D_SS_BEGIN];
    int* cnt = w.cnt + d[D_SS_BEGIN];
    uint64_t* seen = w.seen + d[D_SS_WG_BEGIN] + blockIdx.x;
    const uint64_t before = *seen;
    uint64_t incoming = blockIdx.x == 0 ? 0ull : ss_load(st + g0);
    if (incoming == SS_NEVER) incoming = ss_guess(scan, len, (uint64_t)g0 * L);
    const bool first_run = before == SS_NEVER;
    if (!first_run && incoming == before) return;          // (uniform) nothing moved in front of this workgroup since it last ran
    ss_stage_tables(tabs, comp, d, lane, SS_LANES);
    const SsFile file = ss_file(scan, d, tabs);
    const bool live = gi < n;
    const uint64_t bound = 8ull * (((uint64_t)gi + 1) * L < len ? ((uint64_t)gi + 1) * L : len);
    int mycnt = 0;
    uint64_t old_out = 0;
    if (live) {
        sh[lane] = lane == 0 ? incoming : (first_run ? ss_guess(scan, len, (uint64_t)gi * L) : st[gi]);
        if (!first_run) mycnt = cnt[gi];
    } else {
        sh[lane] = 0;
    }
    if (lane == SS_LANES - 1) {
        if (gi + 1 < n) {
            old_out = ss_load(st + gi + 1);
            if (old_out == SS_NEVER) old_out = ss_guess(scan, len, (uint64_t)(gi + 1) * L);
        }
        sh[SS_LANES] = old_out;
    }
    __syncthreads();
    bool dirty = live && (first_run || lane == 0);
    for (int pass = 0; pass < SS_LANES; ++pass) {          // 64 passes at the most
        const uint64_t in = sh[lane];
        uint64_t out = 0;
        bool moved = false;
        if (dirty) {
            out = ss_eval(file, in, bound, &mycnt);
            moved = out != sh[lane + 1];
        }
        __syncthreads();          // every lane has read its input and its neighbour's
        if (moved) sh[lane + 1] = out;
        const int any = __syncthreads_or(moved ? 1 : 0);
        dirty = live && lane > 0 && sh[lane] != in;
        if (!any) break;
    }
    if (live) {
        cnt[gi] = mycnt;
        if (gi + 1 < n) {
            if (lane < SS_LANES - 1) {
                st[gi + 1] = sh[lane + 1];
            } else {          // the outgoing boundary: the next workgroup's incoming state
                ss_store(st + gi + 1, sh[SS_LANES]);
                if (sh[SS_LANES] != old_out) atomicOr(&w.chg[f * SS_MAX_LAUNCHES + launch], 1);
            }
        }
    }
    if (lane == 0) *seen = incoming;
}

// One workgroup per file: the exclusive prefix sum of the block counts; the plan, the fallback flag and the launches that were needed
// into status word 1.  A file with restart markers and no DRI is the serial plan's E_RST_COUNT.
__global__ __launch_bounds__(256) void jpeg_sync_scan_kernel(const long long* __restrict__ desc, SsWork w, int launches, int* __restrict__ status) {
    __shared__ long long part[256];
    const int f = blockIdx.x, t = threadIdx.x;
    const long long* d = desc + (long long)f * DESC;
    const long long n = d[D_SS_COUNT];
    if (n <= 0) return;
    const int* chg = w.chg + f * SS_MAX_LAUNCHES;
    int last = -1;
    for (int k = 0; k < launches; ++k) last = chg[k] ? k : last;          // <= 16
    const bool fallback = last == launches - 1 && d[D_IVL_COUNT] == 1;
    if (t == 0) {
        const int used = last + 2 < launches ? last + 2 : launches;
        status[2 * f + 1] = (fallback ? ST_FALLBACK : PLAN_SELFSYNC) | (used << ST_LAUNCHES_SHIFT);
        if (d[D_IVL_COUNT] != 1) status[2 * f] = E_RST_COUNT;
    }
    if (fallback || d[D_IVL_COUNT] != 1) return;
    const int* cnt = w.cnt + d[D_SS_BEGIN];
    long long* first = w.first + d[D_SS_BEGIN];
    const long long chunk = (n + 255) / 256, a = t * chunk, b = a + chunk < n ? a + chunk : n;
    long long sum = 0;
    for (long long i = a; i < b; ++i) sum += cnt[i];          // <= chunk
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int i = 0; i < 256; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    long long run = part[t];
    for (long long i = a; i < b; ++i) {
        first[i] = run;
        run += cnt[i];
    }
}

__global__ __launch_bounds__(SS_LANES) void jpeg_sync_write_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, SsWork w,
                                                                   int16_t* __restrict__ coef, const int* __restrict__ status) {
    __shared__ HuffTab tabs[8];
    const int f = blockIdx.y, lane = threadIdx.x;
    const long long* d = desc + (long long)f * DESC;
    const long long n = d[D_SS_COUNT], g0 = (long long)blockIdx.x * SS_LANES, gi = g0 + lane;
    if (g0 >= n || d[D_IVL_COUNT] != 1 || (status[2 * f + 1] & ST_FALLBACK)) return;          // (uniform)
    const Geometry geo = geometry((int)d[D_H], (int)d[D_W], (int)d[D_NCOMP], (int)d[D_HS], (int)d[D_VS]);
    const long long blocks = geo.blocks();
    if (w.first[d[D_SS_BEGIN] + g0] >= blocks) return;          // (uniform) the first blocks ascend
    ss_stage_tables(tabs, comp, d, lane, SS_LANES);
    if (gi >= n) return;
    const uint64_t L = (uint64_t)d[D_SS_BYTES];
    const uint32_t len = (uint32_t)d[D_SCAN_LEN];
    const SsFile file = ss_file(comp + d[D_SCAN_OFF], d, tabs);
    const uint64_t bound = 8ull * (((uint64_t)gi + 1) * L < len ? ((uint64_t)gi + 1) * L : len);
    const uint64_t s = gi == 0 ? 0ull : w.state[d[D_SS_BEGIN] + gi];
    const int rc = ss_write(file, s, bound, gi == n - 1, w.first[d[D_SS_BEGIN] + gi], blocks, coef + d[D_COEF_OFF] * 64);
    if (rc != OK) atomicMin(&w.err[f], ((unsigned long long)gi << 8) | (unsigned long long)rc);          // the lowest sub-sequence's code: that lane began at a true state
}

// DC differences -> DC values: block (c, file) sums the differences of component c in scan order, mod 2^32 as decode_block does, and
// stores them as int16.  Block (0, file) first hands the write pass's code to the status word.
__global__ __launch_bounds__(256) void jpeg_sync_dc_kernel(const long long* __restrict__ desc, SsWork w, int16_t* __restrict__ coef, int* __restrict__ status) {
    __shared__ uint32_t part[256];
    const int f = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const long long* d = desc + (long long)f * DESC;
    if (d[D_SS_COUNT] <= 0 || d[D_IVL_COUNT] != 1 || (status[2 * f + 1] & ST_FALLBACK)) return;
    const unsigned long long e = w.err[f];
    if (e != ~0ull) {
        if (c == 0 && t == 0) atomicCAS(&status[2 * f], 0, (int)(e & 255ull));
        return;
    }
    const int ncomp = (int)d[D_NCOMP];
    if (c >= ncomp) return;
    const Geometry geo = geometry((int)d[D_H], (int)d[D_W], ncomp, (int)d[D_HS], (int)d[D_VS]);
    const int ny = ncomp == 3 ? (int)(d[D_HS] * d[D_VS]) : 1;
    const long long nb = geo.mcus() * (c == 0 ? ny : 1);
    int16_t* cf = coef + d[D_COEF_OFF] * 64;
    const long long chunk = (nb + 255) / 256, a = t * chunk, b = a + chunk < nb ? a + chunk : nb;
    uint32_t sum = 0;
    for (long long i = a; i < b; ++i) sum += (uint32_t)(int32_t)cf[ss_block_of(i, c, ny, geo.bpm) * 64];          // <= chunk
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const uint32_t v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    uint32_t pred = part[t];
    for (long long i = a; i < b; ++i) {
        int16_t* o = cf + ss_block_of(i, c, ny, geo.bpm) * 64;
        pred += (uint32_t)(int32_t)*o;
        *o = (int16_t)pred;
    }
}

// jpeg_idct_islow's 1-D pass on 8 values held in registers (CONST_BITS 13); the caller descales.  Products wrap as unsigned: hostile
// coefficients give garbage, not undefined behaviour.
__device__ __forceinline__ int mul(int a, int b) { return (int)((uint32_t)a * (uint32_t)b); }
__device__ __forceinline__ void idct_1d(const int (&in)[8], int (&out)[8]) {
    int z1 = mul(in[2] + in[6], 4433);
    const int tmp2 = z1 - mul(in[6], 15137), tmp3 = z1 + mul(in[2], 6270);
    const int tmp0 = (int)((uint32_t)(in[0] + in[4]) << 13), tmp1 = (int)((uint32_t)(in[0] - in[4]) << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = mul(z3 + z4, 9633);
    t0 = mul(t0, 2446);
    t1 = mul(t1, 16819);
    t2 = mul(t2, 25172);
    t3 = mul(t3, 12299);
    z1 = mul(z1, -7373);
    z2 = mul(z2, -20995);
    z3 = mul(z3, -16069) + z5;
    z4 = mul(z4, -3196) + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    out[0] = tmp10 + t3;
    out[7] = tmp10 - t3;
    out[1] = tmp11 + t2;
    out[6] = tmp11 - t2;
    out[2] = tmp12 + t1;
    out[5] = tmp12 - t1;
    out[3] = tmp13 + t0;
    out[4] = tmp13 - t0;
}

// where component c of a file lives in its planes: every component padded to whole MCUs
struct Planes {
    int lw, lh, cw, ch;          // the padded sizes of the luma plane and of a chroma plane
    __device__ __forceinline__ Planes(const Geometry& g, int ncomp, int hs, int vs) {
        lw = g.mcus_x * (ncomp == 3 ? hs : 1) * 8;
        lh = g.mcus_y * (ncomp == 3 ? vs : 1) * 8;
        cw = g.mcus_x * 8;
        ch = g.mcus_y * 8;
    }
    __device__ __forceinline__ int pw(int c) const { return c == 0 ? lw : cw; }
    __device__ __forceinline__ long long off(int c) const { return c == 0 ? 0ll : (long long)lw * lh + (long long)(c - 1) * cw * ch; }
};

constexpr int WS_ROW = 9;          // a workspace row padded to 9 words: the 8 lanes of a block read rows, not one bank

__global__ __launch_bounds__(64) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ comp, const long long* __restrict__ desc,
                                                       uint8_t* __restrict__ planes, const int* __restrict__ status) {
    __shared__ int ws[8][8 * WS_ROW];
    const int f = blockIdx.y, sub = threadIdx.x >> 3, i = threadIdx.x & 7;
    const long long* d = desc + (long long)f * DESC;
    const int ncomp = (int)d[D_NCOMP], hs = (int)d[D_HS], vs = (int)d[D_VS];
    const Geometry g = geometry((int)d[D_H], (int)d[D_W], ncomp, hs, vs);
    const long long bid = (long long)blockIdx.x * 8 + sub;
    const bool live = status[2 * f] == 0 && bid < g.blocks();          // (status and the bounds are uniform over a block's 8 lanes)
    const long long mcu = live ? bid / g.bpm : 0;
    const int j = live ? (int)(bid % g.bpm) : 0;
    const int ny = ncomp == 3 ? hs * vs : 1;
    const int c = j < ny ? 0 : j - ny + 1;
    if (live) {
        const uint16_t* q = (const uint16_t*)(comp + d[D_TAB_OFF]) + 64 * (((uint32_t)d[D_TQ] >> (8 * c)) & 3u);
        const int16_t* cf = coef + (d[D_COEF_OFF] + bid) * 64;
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = mul((int)cf[r * 8 + i], (int)q[r * 8 + i]);
        idct_1d(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[sub][r * WS_ROW + i] = (out[r] + (1 << 10)) >> 11;
    }
    __syncthreads();          // the columns of all 8 lanes before any of them reads a row
    if (!live) return;
    int in[8], out[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) in[x] = ws[sub][i * WS_ROW + x];
    idct_1d(in, out);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        int v = ((out[x] + (1 << 17)) >> 18) + 128;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        if (x < 4)
            lo |= (uint32_t)v << (8 * x);
        else
            hi |= (uint32_t)v << (8 * (x - 4));
    }
    const Planes P(g, ncomp, hs, vs);
    const int h = c == 0 ? (ncomp == 3 ? hs : 1) : 1, v = c == 0 ? (ncomp == 3 ? vs : 1) : 1;
    const int sx = c == 0 ? j % h : 0, sy = c == 0 ? j / h : 0;
    const int bx = (int)(mcu % g.mcus_x) * h + sx, by = (int)(mcu / g.mcus_x) * v + sy;
    uint8_t* o = planes + d[D_PLANE_OFF] + P.off(c) + (long long)(by * 8 + i) * P.pw(c) + bx * 8;
    *(u32x2_t*)o = u32x2_t{lo, hi};          // 8-byte aligned: the plane offsets and widths are multiples of 8
}

__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pw, int cw, int ch, int x, int y, int hs, int vs) {
    if (hs == 1) return p[(long long)y * pw + x];
    const int c = x >> 1;
    if (vs == 1) {          // h2v1
        const uint8_t* row = p + (long long)y * pw;
        const int cur = row[c];
        if (x & 1) return c == cw - 1 ? cur : (3 * cur + row[c + 1] + 2) >> 2;
        return c == 0 ? cur : (3 * cur + row[c - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    int rf = (y & 1) ? r + 1 : r - 1;
    rf = rf < 0 ? 0 : (rf > ch - 1 ? ch - 1 : rf);
    const uint8_t* near = p + (long long)r * pw;
    const uint8_t* far = p + (long long)rf * pw;
    const int cur = 3 * near[c] + far[c];
    if (x & 1) return c == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * near[c + 1] + far[c + 1] + 7) >> 4;
    return c == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * near[c - 1] + far[c - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void jpeg_upsample_rgb_kernel(const uint8_t* __restrict__ planes, const long long* __restrict__ desc, uint8_t* __restrict__ pix,
                                                                const int* __restrict__ status) {
    const int f = blockIdx.y;
    if (status[2 * f] != 0) return;
    const long long* d = desc + (long long)f * DESC;
    const int H = (int)d[D_H], W = (int)d[D_W], ncomp = (int)d[D_NCOMP], hs = (int)d[D_HS], vs = (int)d[D_VS], oc = (int)d[D_OUTC];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx % W);
    const Geometry g = geometry(H, W, ncomp, hs, vs);
    const Planes P(g, ncomp, hs, vs);
    const uint8_t* base = planes + d[D_PLANE_OFF];
    const int yy = base[(long long)y * P.lw + x];
    uint8_t* o = pix + d[D_PIX_OFF] + (long long)y * d[D_ROW_STRIDE] + (long long)x * oc;
    if (ncomp == 1) {
        o[0] = (uint8_t)yy;
        if (oc == 3) {
            o[1] = (uint8_t)yy;
            o[2] = (uint8_t)yy;
        }
        return;
    }
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;          // the real downsampled plane
    const int cb = chroma_at(base + P.off(1), P.cw, cw, ch, x, y, hs, vs) - 128;
    const int cr = chroma_at(base + P.off(2), P.cw, cw, ch, x, y, hs, vs) - 128;
    o[0] = (uint8_t)clamp8(yy + ((91881 * cr + 32768) >> 16));                      // FIX(1.402)
    o[1] = (uint8_t)clamp8(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));        // FIX(0.34414), FIX(0.71414)
    o[2] = (uint8_t)clamp8(yy + ((116130 * cb + 32768) >> 16));                     // FIX(1.772)
}

static long long plane_bytes_of(const Geometry& g, int ncomp, int hs, int vs) {
    const long long luma = (long long)g.mcus_x * g.mcus_y * 64 * (ncomp == 3 ? hs * vs : 1);
    return ncomp == 3 ? luma + 2ll * g.mcus_x * g.mcus_y * 64 : luma;
}

// what every entry point checks of a descriptor before anything is launched
static bool jpegdec_desc_ok(const int64_t* d, int64_t comp_bytes, int64_t coef_blocks, int64_t plane_bytes, int64_t pix_bytes, bool pixels) {
    const int64_t H = d[D_H], W = d[D_W], nc = d[D_NCOMP], hs = d[D_HS], vs = d[D_VS], oc = d[D_OUTC];
    if (H < 1 || W < 1 || H > RF_JPEGDEC_MAX_SIDE || W > RF_JPEGDEC_MAX_SIDE) return false;
    if (!((nc == 1 && hs == 1 && vs == 1) || (nc == 3 && (hs == 1 || hs == 2) && (vs == 1 || (vs == 2 && hs == 2))))) return false;
    if (d[D_RI] < 0 || d[D_RI] > 65535) return false;
    if (d[D_SCAN_OFF] < 0 || d[D_SCAN_LEN] < 0 || d[D_SCAN_LEN] >= (1ll << 31) || d[D_SCAN_OFF] + d[D_SCAN_LEN] > comp_bytes) return false;
    if (d[D_TAB_OFF] < 0 || (d[D_TAB_OFF] & 15) || d[D_TAB_OFF] + TABLE_BYTES > comp_bytes) return false;
    for (int c = 0; c < 3; ++c)
        if (((d[D_TQ] >> (8 * c)) & 255) > 3 || ((d[D_TD] >> (8 * c)) & 255) > 3 || ((d[D_TA] >> (8 * c)) & 255) > 3) return false;
    if (d[D_TQ] < 0 || d[D_TD] < 0 || d[D_TA] < 0 || d[D_TQ] >> 24 || d[D_TD] >> 24 || d[D_TA] >> 24) return false;
    const Geometry g = geometry((int)H, (int)W, (int)nc, (int)hs, (int)vs);
    if (d[D_COEF_OFF] < 0 || d[D_COEF_OFF] + g.blocks() > coef_blocks) return false;
    if (d[D_PLANE_OFF] < 0 || (d[D_PLANE_OFF] & 15) || d[D_PLANE_OFF] + plane_bytes_of(g, (int)nc, (int)hs, (int)vs) > plane_bytes) return false;
    if (pixels) {
        if (!(oc == 3 || (oc == 1 && nc == 1))) return false;
        if (d[D_PIX_OFF] < 0 || d[D_ROW_STRIDE] < W * oc || d[D_PIX_OFF] + (H - 1) * d[D_ROW_STRIDE] + W * oc > pix_bytes) return false;
    }
    return true;
}

}  // namespace rf

using namespace rf;

extern "C" int rf_jpeg_entropy_decode(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, const int* ivl_host,
                                      const int* ivl, int nivl, int lanes, int16_t* coef, int64_t coef_blocks, int* status, void* stream) {
    RF_CHECK(comp_u8 && desc_host && desc && ivl_host && ivl && coef && status && B > 0 && B <= 65535 && nivl >= B && lanes >= 1 && lanes <= 64,
             "rf_jpeg_entropy_decode: bad arguments (B=%d nivl=%d lanes=%d)", B, nivl, lanes);
    RF_CHECK(((uintptr_t)comp_u8 & 15) == 0 && coef_blocks > 0 && coef_blocks < (1ll << 31), "rf_jpeg_entropy_decode: comp must be 16-byte aligned, 0 < coef_blocks < 2^31");
    int64_t next = 0;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(jpegdec_desc_ok(d, comp_bytes, coef_blocks, 1ll << 62, 0, false), "rf_jpeg_entropy_decode: descriptor %d is out of range", f);
        const int64_t ib = d[D_IVL_BEGIN], in = d[D_IVL_COUNT];
        RF_CHECK(in >= 1 && ib == next && ib + in <= nivl, "rf_jpeg_entropy_decode: the intervals of file %d are not the next %lld of %d", f, (long long)in, nivl);
        for (int64_t k = ib; k < ib + in; ++k) {
            const int64_t s = ivl_host[nivl + k];
            RF_CHECK(ivl_host[k] == f && (k == ib ? s == 0 : (s >= 2 && s >= ivl_host[nivl + k - 1] + 2 && s <= d[D_SCAN_LEN])),
                     "rf_jpeg_entropy_decode: interval %lld of file %d is out of range or out of order", (long long)(k - ib), f);
        }
        next = ib + in;
    }
    RF_CHECK(next == nivl, "rf_jpeg_entropy_decode: %lld intervals belong to no file", (long long)(nivl - next));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(coef, 0, (size_t)coef_blocks * 128, st) != hipSuccess || hipMemsetAsync(status, 0, (size_t)B * 8, st) != hipSuccess) {
        rf::set_error("rf_jpeg_entropy_decode: hipMemsetAsync failed");
        return 2;
    }
    const unsigned grid = (unsigned)((nivl + lanes - 1) / lanes);
    hipLaunchKernelGGL(jpeg_entropy_decode_kernel, dim3(grid), dim3(64), 0, st, (const uint8_t*)comp_u8, (const long long*)desc, ivl, nivl, lanes, coef, status, 0);
    RF_LAUNCH_CHECK("rf_jpeg_entropy_decode");
    return 0;
}

extern "C" int64_t rf_jpeg_selfsync_work_bytes(int64_t subseqs, int64_t workgroups, int B) {
    return subseqs < 0 || workgroups < 0 || B < 0 ? -1 : ss_work_bytes(subseqs, workgroups, B);
}

extern "C" int rf_jpeg_selfsync_decode(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, const int* ivl_host, const int* ivl,
                                       int nivl, int lanes, int launches, int stages, void* work, int64_t work_bytes, int16_t* coef, int64_t coef_blocks, int* status,
                                       void* stream) {
    RF_CHECK(comp_u8 && desc_host && desc && ivl_host && ivl && work && coef && status && B > 0 && B <= 65535 && nivl >= B && lanes >= 1 && lanes <= 64,
             "rf_jpeg_selfsync_decode: bad arguments (B=%d nivl=%d lanes=%d)", B, nivl, lanes);
    RF_CHECK(launches >= 1 && launches <= SS_MAX_LAUNCHES && stages >= 1 && stages <= RF_JPEGDEC_SS_ALL, "rf_jpeg_selfsync_decode: 1 <= launches <= %d, 1 <= stages <= %d",
             SS_MAX_LAUNCHES, RF_JPEGDEC_SS_ALL);
    RF_CHECK(((uintptr_t)comp_u8 & 15) == 0 && ((uintptr_t)work & 7) == 0 && coef_blocks > 0 && coef_blocks < (1ll << 31),
             "rf_jpeg_selfsync_decode: comp must be 16-byte, work 8-byte aligned, 0 < coef_blocks < 2^31");
    int64_t S = 0, G = 0, maxn = 0, next = 0;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(jpegdec_desc_ok(d, comp_bytes, coef_blocks, 1ll << 62, 0, false), "rf_jpeg_selfsync_decode: descriptor %d is out of range", f);
        const int64_t ib = d[D_IVL_BEGIN], in = d[D_IVL_COUNT];          // (the serial lane of the last launch reads them)
        RF_CHECK(in >= 1 && ib == next && ib + in <= nivl, "rf_jpeg_selfsync_decode: the intervals of file %d are not the next %lld of %d", f, (long long)in, nivl);
        for (int64_t k = ib; k < ib + in; ++k) {
            const int64_t s = ivl_host[nivl + k];
            RF_CHECK(ivl_host[k] == f && (k == ib ? s == 0 : (s >= 2 && s >= ivl_host[nivl + k - 1] + 2 && s <= d[D_SCAN_LEN])),
                     "rf_jpeg_selfsync_decode: interval %lld of file %d is out of range or out of order", (long long)(k - ib), f);
        }
        next = ib + in;
        const int64_t n = d[D_SS_COUNT], L = d[D_SS_BYTES];
        if (n == 0) continue;
        RF_CHECK(L >= SS_MIN_BYTES && L <= SS_MAX_BYTES && d[D_RI] == 0 && d[D_SCAN_LEN] >= 2 * L && n == (d[D_SCAN_LEN] + L - 1) / L && d[D_SS_BEGIN] == S &&
                     d[D_SS_WG_BEGIN] == G,
                 "rf_jpeg_selfsync_decode: the sub-sequences of file %d (%lld of %lld bytes from slot %lld, workgroup %lld) do not fit its scan or the batch", f, (long long)n,
                 (long long)L, (long long)d[D_SS_BEGIN], (long long)d[D_SS_WG_BEGIN]);
        S += n;
        G += (n + SS_LANES - 1) / SS_LANES;
        maxn = n > maxn ? n : maxn;
    }
    RF_CHECK(S > 0 && S < (1ll << 31), "rf_jpeg_selfsync_decode: no file of the batch takes the plan (or 2^31 sub-sequences)");
    RF_CHECK(work_bytes >= ss_work_bytes(S, G, B), "rf_jpeg_selfsync_decode: work holds %lld bytes, %lld are needed", (long long)work_bytes, (long long)ss_work_bytes(S, G, B));
    const SsWork w = ss_work(work, S, G, B);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((maxn + SS_LANES - 1) / SS_LANES), (unsigned)B);
    if (stages & RF_JPEGDEC_SS_SYNC) {
        // no state, no workgroup has run, no error; then no boundary has moved
        if (hipMemsetAsync(work, 0xFF, (size_t)ss_work_bytes(S, G, B), st) != hipSuccess || hipMemsetAsync(w.chg, 0, (size_t)B * SS_MAX_LAUNCHES * 4, st) != hipSuccess) {
            rf::set_error("rf_jpeg_selfsync_decode: hipMemsetAsync failed");
            return 2;
        }
        for (int k = 0; k < launches; ++k) hipLaunchKernelGGL(jpeg_sync_kernel, grid, dim3(SS_LANES), 0, st, (const uint8_t*)comp_u8, (const long long*)desc, w, k);
    }
    if (stages & RF_JPEGDEC_SS_SCAN) hipLaunchKernelGGL(jpeg_sync_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, (const long long*)desc, w, launches, status);
    if (stages & RF_JPEGDEC_SS_WRITE)
        hipLaunchKernelGGL(jpeg_sync_write_kernel, grid, dim3(SS_LANES), 0, st, (const uint8_t*)comp_u8, (const long long*)desc, w, coef, (const int*)status);
    if (stages & RF_JPEGDEC_SS_DC) hipLaunchKernelGGL(jpeg_sync_dc_kernel, dim3(3, (unsigned)B), dim3(256), 0, st, (const long long*)desc, w, coef, status);
    if (stages & RF_JPEGDEC_SS_SERIAL)
        hipLaunchKernelGGL(jpeg_entropy_decode_kernel, dim3((unsigned)((nivl + lanes - 1) / lanes)), dim3(64), 0, st, (const uint8_t*)comp_u8, (const long long*)desc, ivl, nivl,
                           lanes, coef, status, 1);
    RF_LAUNCH_CHECK("rf_jpeg_selfsync_decode");
    return 0;
}

extern "C" int rf_jpeg_idct_u8(const int16_t* coef, int64_t coef_blocks, const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host,
                               const int64_t* desc, int B, void* planes_u8, int64_t plane_bytes, const int* status, void* stream) {
    RF_CHECK(coef && comp_u8 && desc_host && desc && planes_u8 && status && B > 0 && B <= 65535, "rf_jpeg_idct_u8: bad arguments (B=%d)", B);
    RF_CHECK(((uintptr_t)comp_u8 & 15) == 0 && ((uintptr_t)planes_u8 & 15) == 0, "rf_jpeg_idct_u8: comp and planes must be 16-byte aligned");
    int64_t maxb = 1;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(jpegdec_desc_ok(d, comp_bytes, coef_blocks, plane_bytes, 0, false), "rf_jpeg_idct_u8: descriptor %d is out of range", f);
        const int64_t nb = geometry((int)d[D_H], (int)d[D_W], (int)d[D_NCOMP], (int)d[D_HS], (int)d[D_VS]).blocks();
        maxb = nb > maxb ? nb : maxb;
    }
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((maxb + 7) / 8), (unsigned)B), dim3(64), 0, (hipStream_t)stream, coef, (const uint8_t*)comp_u8,
                       (const long long*)desc, (uint8_t*)planes_u8, status);
    RF_LAUNCH_CHECK("rf_jpeg_idct_u8");
    return 0;
}

extern "C" int rf_jpeg_upsample_rgb_u8(const void* planes_u8, int64_t plane_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* pix_u8,
                                       int64_t pix_bytes, const int* status, void* stream) {
    RF_CHECK(planes_u8 && desc_host && desc && pix_u8 && status && B > 0 && B <= 65535, "rf_jpeg_upsample_rgb_u8: bad arguments (B=%d)", B);
    int64_t maxp = 1;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(jpegdec_desc_ok(d, 1ll << 62, 1ll << 40, plane_bytes, pix_bytes, true), "rf_jpeg_upsample_rgb_u8: descriptor %d is out of range", f);
        maxp = d[D_H] * d[D_W] > maxp ? d[D_H] * d[D_W] : maxp;
    }
    hipLaunchKernelGGL(jpeg_upsample_rgb_kernel, dim3((unsigned)((maxp + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)planes_u8,
                       (const long long*)desc, (uint8_t*)pix_u8, status);
    RF_LAUNCH_CHECK("rf_jpeg_upsample_rgb_u8");
    return 0;
}
