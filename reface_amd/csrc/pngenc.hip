// PNG encoding of device-resident uint8 images (the CLIs' --gpu_png): what reaches the host is one finished zlib stream per image, which the
// host wraps in the PNG signature, IHDR, IDAT and IEND (reface_amd/pngenc.py).  Three stages, one entry point each:
//   rf_png_filter_u8          the five PNG row filters in exact integer arithmetic, one per row by the minimum-sum-of-|residual| heuristic
//   rf_png_deflate_segments   the stream cut into 32768-byte segments, one workgroup each; nothing refers back across a segment start
//   rf_png_pack               the segments of an image copied behind the zlib header, the Adler-32 combined and appended, the length written
// A segment is tokenised like zlib's Z_RLE strategy (matches at distance 1 only), coded with its own Huffman code in ONE dynamic block with a
// header of fixed form, and -- unless it is the image's last -- ends with an empty stored block (00 00 FF FF after padding), so that segments
// concatenate at byte granularity.  A segment that does not get smaller this way is written as one stored block.  Every tie-break below is
// fixed so that tests/pngenc_refs.py gives the same bytes.
#include "common.h"

namespace rf {

constexpr int PNG_SEG = 32768;                   // bytes of the stream per segment
constexpr int PNG_SLOT = 32784;                  // bytes of a segment's output slot: the stored worst case (32768 + 5) rounded up to 16
constexpr int PNG_DT = 1024;                     // threads of a deflate workgroup: 32 consecutive bytes each
constexpr int PNG_BUFW = 8200;                   // LDS words: the segment (8192), later the bit buffer (at most 32768 + 4 bytes are kept, + 1 word of spill)
constexpr int PNG_NSYM = 286;                    // literal/length symbols (HLIT = 29)
constexpr int PNG_HDR_BITS = 17 + 19 * 3 + 287 * 4;
constexpr uint32_t ADLER_MOD = 65521u;

// ---- workgroup scans / sums over one int per thread (any commutative op); `ws` holds one word per wave
template <bool REV, typename Op>
__device__ __forceinline__ int block_scan_excl(int v, Op op, int ident, int* ws, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = REV ? __shfl_down(inc, o, 64) : __shfl_up(inc, o, 64);
        if (REV ? lane + o < 64 : lane >= o) inc = op(inc, u);
    }
    int exc = REV ? __shfl_down(inc, 1, 64) : __shfl_up(inc, 1, 64);
    if (REV ? lane == 63 : lane == 0) exc = ident;
    __syncthreads();
    if (lane == (REV ? 0 : 63)) ws[wave] = inc;
    __syncthreads();
    int pre = ident, tot = ident;
    for (int w = 0; w < nw; ++w) {
        const int x = ws[w];
        tot = op(tot, x);
        if (REV ? w > wave : w < wave) pre = op(pre, x);
    }
    *total = tot;
    return op(pre, exc);
}
struct op_add { __device__ __forceinline__ int operator()(int a, int b) const { return a + b; } };
struct op_max { __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct op_min { __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; } };

__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, int* ws) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = (int)v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += (uint32_t)ws[w];
    return t;
}

// ================================================================================================ stage 1: filter
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int png_residual(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    return (x - pred) & 255;
}
__device__ __forceinline__ uint32_t sabs8(int r) { return (uint32_t)(r < 128 ? r : 256 - r); }

// one workgroup per row: pass 1 sums |residual| of the five filters, pass 2 writes the winner (ties: the lowest type)
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t* __restrict__ img, int n, int bpp, long long istride, long long rstride,
                                                         uint8_t* __restrict__ out, long long ostride) {
    __shared__ int ws[4];
    const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const uint8_t* row = img + (long long)b * istride + (long long)y * rstride;
    const uint8_t* up = row - rstride;
    const bool has_up = y > 0;
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += 256) {
        const int x = row[i], a = i >= bpp ? row[i - bpp] : 0, bb = has_up ? up[i] : 0, c = (has_up && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) s[t] += sabs8(png_residual(t, x, a, bb, c));
    }
    int best = 0;
    uint32_t bs = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const uint32_t tot = block_sum_u32(s[t], ws);
        if (t == 0 || tot < bs) {
            bs = tot;
            best = t;
        }
    }
    uint8_t* o = out + (long long)b * ostride + (long long)y * (1 + n);
    if (tid == 0) o[0] = (uint8_t)best;
    for (int i = tid; i < n; i += 256) {
        const int x = row[i], a = i >= bpp ? row[i - bpp] : 0, bb = has_up ? up[i] : 0, c = (has_up && i >= bpp) ? up[i - bpp] : 0;
        o[1 + i] = (uint8_t)png_residual(best, x, a, bb, c);
    }
}

// ================================================================================================ stage 2: segment deflate
// length 3 .. 258 -> (symbol - 257, extra bits, base) of RFC 1951 3.2.5
__device__ __forceinline__ void length_code(int len, int& k, int& ebits, int& base) {
    if (len == 258) {
        k = 28, ebits = 0, base = 258;
        return;
    }
    const int l = len - 3;
    if (l < 8) {
        k = l, ebits = 0, base = len;
        return;
    }
    const int hb = 31 - __clz(l);          // >= 3
    ebits = hb - 2;
    const int sub = (l >> ebits) & 3;
    k = 4 * ebits + 4 + sub;
    base = 3 + ((4 + sub) << ebits);
}

// The role of byte g of the segment from the run it lies in, [s, e): 0 = covered by a match, 1 = literal, >= 3 = head of a match of that length.
// The first byte of a run is a literal; of the R - 1 that remain, chunks of up to 258 are matches while at least 3 are left; 1 or 2 left are literals.
__device__ __forceinline__ int byte_role(int g, int s, int e) {
    const int p = g - s;
    if (p == 0) return 1;
    const int q = p - 1, rem = e - s - 1;
    const int k = q / 258, r = q - 258 * k, left = rem - 258 * k;
    if (left < 3) return 1;
    return r == 0 ? (left < 258 ? left : 258) : 0;
}

__device__ __forceinline__ void put_bits(uint32_t* buf, int off, uint32_t val, int nb) {
    const int w = off >> 5, sh = off & 31;
    atomicOr(&buf[w], val << sh);
    if (sh + nb > 32) atomicOr(&buf[w + 1], val >> (32 - sh));
}

__global__ __launch_bounds__(PNG_DT) void png_deflate_kernel(const uint8_t* __restrict__ streams, long long sstride, long long n_total, int nseg,
                                                             uint8_t* __restrict__ slots, int* __restrict__ seg_bytes, uint32_t* __restrict__ seg_adler) {
    __shared__ __align__(16) uint32_t buf[PNG_BUFW];          // (16-byte aligned: every thread reads its 32 bytes as two 128-bit LDS loads)
    __shared__ int cnt[288], sw[288], ssym[288], iw[288], par[576], clen[288], ccode[288];
    __shared__ int ws[16], sh_m, sh_maxd;
    const int tid = threadIdx.x, lane = tid & 63, seg = blockIdx.x, b = blockIdx.y;
    const long long soff = (long long)seg * PNG_SEG;
    const int n = (int)(n_total - soff < PNG_SEG ? n_total - soff : PNG_SEG);
    const uint8_t* src = streams + (long long)b * sstride + soff;
    const bool last = seg == nseg - 1;
    uint8_t* bufb = (uint8_t*)buf;

    // ---- the segment into LDS (zero beyond n), counts cleared
    for (int i = tid; i < PNG_BUFW; i += PNG_DT) buf[i] = 0;
    for (int i = tid; i < 288; i += PNG_DT) cnt[i] = 0;
    __syncthreads();
    if (((uintptr_t)src & 3) == 0) {
        const uint32_t* s4 = (const uint32_t*)src;
        for (int i = tid; i < (n >> 2); i += PNG_DT) buf[i] = s4[i];
        for (int i = (n & ~3) + tid; i < n; i += PNG_DT) bufb[i] = src[i];
    } else {
        for (int i = tid; i < n; i += PNG_DT) bufb[i] = src[i];
    }
    __syncthreads();

    // ---- this thread's 32 bytes, their run-start flags F (bit i: byte base + i differs from its predecessor) and Fe = F with position n flagged
    const int base = tid * 32;
    uint32_t w[8];
    {
        const u32x4_t lo = *(const u32x4_t*)&buf[tid * 8], hi = *(const u32x4_t*)&buf[tid * 8 + 4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = lo[i];
            w[4 + i] = hi[i];
        }
    }
    int prev = base > 0 ? (int)bufb[base - 1] : -1;
    uint32_t F = 0;
    uint32_t adA = 0, adB = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int v = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
        if (base + i < n) {
            if (v != prev) F |= 1u << i;
            adA += (uint32_t)v;
            adB += (uint32_t)(n - (base + i)) * (uint32_t)v;
        }
        prev = v;
    }
    const uint32_t Fe = (n >= base && n < base + 32) ? (F | (1u << (n - base))) : F;
    int dummy;
    const int carry_s = block_scan_excl<false>(F ? base + 31 - __clz((int)F) : -1, op_max(), -1, ws, &dummy);
    int carry_e = block_scan_excl<true>(Fe ? base + __ffs((int)Fe) - 1 : 0x7fffffff, op_min(), 0x7fffffff, ws, &dummy);
    if (carry_e > n) carry_e = n;

    // Adler-32 partial of the segment: A = sum of bytes, B = sum of (n - i) * byte_i (mod 65521), combined in order by the pack stage
    {
        const uint32_t A = block_sum_u32(adA, ws) % ADLER_MOD;
        const uint32_t Bs = block_sum_u32(adB % ADLER_MOD, ws) % ADLER_MOD;
        if (tid == 0) seg_adler[(long long)b * nseg + seg] = A | (Bs << 16);
    }

    // ---- histogram of the 286 literal/length symbols.  Flat content puts nearly all counts in one bin: the lanes that share the first active
    // lane's symbol are counted with one add, the rest add for themselves.  Only that ONE symbol is folded per step: on textured content
    // (many distinct symbols in a wave) this is up to 63 separate LDS atomics per step, i.e. no better than plain per-lane adds there.
    const int nvalid = n - base < 0 ? 0 : (n - base > 32 ? 32 : n - base);
    for (int i = 0; i < 32; ++i) {
        int sym = -1;
        if (i < nvalid) {
            const uint32_t below = F & (0xffffffffu >> (31 - i)), above = i < 31 ? (Fe & ~(0xffffffffu >> (31 - i))) : 0u;
            const int s = below ? base + 31 - __clz((int)below) : carry_s;
            const int e = above ? base + __ffs((int)above) - 1 : carry_e;
            const int role = byte_role(base + i, s, e);
            if (role == 1) sym = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
            else if (role >= 3) {
                int k, eb, lb;
                length_code(role, k, eb, lb);
                sym = 257 + k;
            }
        }
        const unsigned long long act = __ballot(sym >= 0);
        if (act) {
            const int lead = __shfl(sym, __ffsll((long long)act) - 1, 64);
            const unsigned long long same = __ballot(sym == lead);
            if (sym == lead) {
                if (lane == __ffsll((long long)same) - 1) atomicAdd(&cnt[lead], __popcll(same));
            } else if (sym >= 0) {
                atomicAdd(&cnt[sym], 1);
            }
        }
    }
    if (tid == 0) cnt[256] = 1;          // end of block
    __syncthreads();

    // ---- Huffman code lengths: leaves sorted by (count, symbol), two queues, the leaf on equal weight; halve the counts while a code is deeper than 15
    for (int round = 0;; ++round) {
        if (round > 0) {
            if (tid < PNG_NSYM && cnt[tid] > 0) cnt[tid] = (cnt[tid] + 1) >> 1;
            __syncthreads();
        }
        if (tid < PNG_NSYM) {
            const int c = cnt[tid];
            clen[tid] = 0;
            if (c > 0) {
                int rank = 0;
                for (int j = 0; j < PNG_NSYM; ++j) {
                    const int cj = cnt[j];
                    rank += (cj > 0 && (cj < c || (cj == c && j < tid))) ? 1 : 0;
                }
                sw[rank] = c;
                ssym[rank] = tid;
            }
        }
        if (tid == 0) {
            int m = 0;
            for (int j = 0; j < PNG_NSYM; ++j) m += cnt[j] > 0 ? 1 : 0;
            sh_m = m;
        }
        __syncthreads();
        const int m = sh_m;          // >= 2: the end-of-block symbol and at least one literal
        if (tid == 0) {
            // the two heads of each queue are kept in registers (INF = empty), so a pick waits for no LDS load: the value it needs was
            // fetched two picks earlier
            const int INF = 0x7fffffff;
            int i = 0, j = 0;
            int wl0 = sw[0], wl1 = m > 1 ? sw[1] : INF, wi0 = INF, wi1 = INF;
            for (int k = 0; k < m - 1; ++k) {
                int tot = 0;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (wl0 <= wi0) {          // the leaf on equal weight
                        par[i] = m + k;
                        tot += wl0;
                        ++i;
                        wl0 = wl1;
                        wl1 = i + 1 < m ? sw[i + 1] : INF;
                    } else {
                        par[m + j] = m + k;
                        tot += wi0;
                        ++j;
                        wi0 = wi1;
                        wi1 = j + 1 < k ? iw[j + 1] : INF;
                    }
                }
                iw[k] = tot;
                if (j == k) wi0 = tot;
                else if (j + 1 == k) wi1 = tot;
            }
            sh_maxd = 0;
        }
        __syncthreads();
        if (tid < m) {
            const int root = 2 * m - 2;
            int d = 0;
            for (int x = tid; x != root; x = par[x]) ++d;
            clen[ssym[tid]] = d;
            atomicMax(&sh_maxd, d);
        }
        __syncthreads();
        if (sh_maxd <= 15) break;
        __syncthreads();
    }
    // canonical codes (RFC 1951 3.2.2), stored bit-reversed: Huffman codes enter the stream most significant bit first
    if (tid < PNG_NSYM) {
        const int l = clen[tid];
        int code = 0;
        if (l > 0) {
            // first code of length l = sum over shorter lengths q of count(q) << (l - q); + the symbols of this length before this one
            int c = 0, before = 0;
            for (int j = 0; j < PNG_NSYM; ++j) {
                const int lj = clen[j];
                if (lj > 0 && lj < l) c += 1 << (l - lj);
                before += (lj == l && j < tid) ? 1 : 0;
            }
            code = c + before;
            code = (int)(__brev((uint32_t)code) >> (32 - l));
        }
        ccode[tid] = code;
    }
    __syncthreads();

    // ---- bit length of this thread's tokens, their offsets by an exclusive scan, and the choice between the coded and the stored form
    int mybits = 0;
    for (int i = 0; i < nvalid; ++i) {
        const uint32_t below = F & (0xffffffffu >> (31 - i)), above = i < 31 ? (Fe & ~(0xffffffffu >> (31 - i))) : 0u;
        const int s = below ? base + 31 - __clz((int)below) : carry_s;
        const int e = above ? base + __ffs((int)above) - 1 : carry_e;
        const int role = byte_role(base + i, s, e);
        if (role == 1) mybits += clen[(w[i >> 2] >> (8 * (i & 3))) & 0xffu];
        else if (role >= 3) {
            int k, eb, lb;
            length_code(role, k, eb, lb);
            mybits += clen[257 + k] + eb + 1;
        }
    }
    int tokbits;
    const int myoff = PNG_HDR_BITS + block_scan_excl<false>(mybits, op_add(), 0, ws, &tokbits);
    const int endbits = PNG_HDR_BITS + tokbits + clen[256];
    const int dyn_bytes = last ? (endbits + 7) >> 3 : ((endbits + 3 + 7) >> 3) + 4;
    uint32_t* slot = (uint32_t*)(slots + ((long long)b * nseg + seg) * PNG_SLOT);
    if (dyn_bytes >= n + 5) {
        // one stored block: BFINAL | BTYPE = 00, LEN, ~LEN, the bytes (the segment is still in LDS)
        const uint32_t hdr[5] = {last ? 1u : 0u, (uint32_t)n & 0xffu, (uint32_t)n >> 8, ~(uint32_t)n & 0xffu, (~(uint32_t)n >> 8) & 0xffu};
        for (int wd = tid; wd < (n + 5 + 3) >> 2; wd += PNG_DT) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * wd + j;
                const uint32_t byte = k < 5 ? hdr[k] : (k - 5 < n ? (uint32_t)bufb[k - 5] : 0u);
                v |= byte << (8 * j);
            }
            slot[wd] = v;
        }
        if (tid == 0) seg_bytes[(long long)b * nseg + seg] = n + 5;
        return;
    }
    __syncthreads();          // every thread holds its bytes in registers: the LDS buffer becomes the bit buffer
    for (int i = tid; i < PNG_BUFW; i += PNG_DT) buf[i] = 0;
    __syncthreads();
    // header: BFINAL, BTYPE = 10, HLIT = 29, HDIST = 0, HCLEN = 15; the code-length code (order 16 17 18 0 8 7 ...): 0 0 0, then 4 for each of 0 .. 15, so the
    // code of code length v is v in 4 bits; 286 literal/length code lengths and the one distance code of length 1
    if (tid == 0) put_bits(buf, 0, (last ? 1u : 0u) | (2u << 1) | (29u << 3) | (15u << 13), 17);
    if (tid < 16) put_bits(buf, 26 + 3 * tid, 4u, 3);
    if (tid <= PNG_NSYM) put_bits(buf, 74 + 4 * tid, __brev((uint32_t)(tid < PNG_NSYM ? clen[tid] : 1)) >> 28, 4);
    int off = myoff;
    for (int i = 0; i < nvalid; ++i) {
        const uint32_t below = F & (0xffffffffu >> (31 - i)), above = i < 31 ? (Fe & ~(0xffffffffu >> (31 - i))) : 0u;
        const int s = below ? base + 31 - __clz((int)below) : carry_s;
        const int e = above ? base + __ffs((int)above) - 1 : carry_e;
        const int role = byte_role(base + i, s, e);
        if (role == 1) {
            const int sym = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
            put_bits(buf, off, (uint32_t)ccode[sym], clen[sym]);
            off += clen[sym];
        } else if (role >= 3) {
            int k, eb, lb;
            length_code(role, k, eb, lb);
            const int l = clen[257 + k];
            put_bits(buf, off, (uint32_t)ccode[257 + k] | ((uint32_t)(role - lb) << l), l + eb + 1);          // the distance code is the single bit 0
            off += l + eb + 1;
        }
    }
    if (tid == 0) {
        put_bits(buf, PNG_HDR_BITS + tokbits, (uint32_t)ccode[256], clen[256]);
        if (!last) put_bits(buf, 8 * (dyn_bytes - 2), 0xffffu, 16);          // the empty stored block: 3 zero bits, padding, LEN = 0, ~LEN
        seg_bytes[(long long)b * nseg + seg] = dyn_bytes;
    }
    __syncthreads();
    for (int wd = tid; wd < (dyn_bytes + 3) >> 2; wd += PNG_DT) slot[wd] = buf[wd];
}

// ================================================================================================ stage 3: pack
// one workgroup per segment: its offset = 2 + the sizes before it; the image's last workgroup also combines the Adler-32 and writes the length
__global__ __launch_bounds__(256) void png_pack_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ seg_bytes, const uint32_t* __restrict__ seg_adler,
                                                       int nseg, long long n_total, uint8_t* __restrict__ out, long long ostride, int* __restrict__ lengths) {
    __shared__ int ws[4];
    const int tid = threadIdx.x, seg = blockIdx.x, b = blockIdx.y;
    const int* sizes = seg_bytes + (long long)b * nseg;
    uint32_t before = 0;
    for (int j = tid; j < seg; j += 256) before += (uint32_t)sizes[j];
    const long long off = 2 + (long long)block_sum_u32(before, ws);
    const int sz = sizes[seg];
    uint8_t* dst = out + (long long)b * ostride;
    const uint8_t* srcb = slots + ((long long)b * nseg + seg) * PNG_SLOT;
    const uint32_t* srcw = (const uint32_t*)srcb;
    uint8_t* d = dst + off;
    int head = (int)((4 - ((uintptr_t)d & 3)) & 3);
    if (head > sz) head = sz;
    if (tid < head) d[tid] = srcb[tid];
    const int nw = (sz - head) >> 2;
    uint32_t* dw = (uint32_t*)(d + head);
    for (int k = tid; k < nw; k += 256) {
        const int q = head + 4 * k;
        const uint64_t two = ((uint64_t)srcw[(q >> 2) + 1] << 32) | srcw[q >> 2];
        dw[k] = (uint32_t)(two >> (8 * (q & 3)));
    }
    const int t0 = head + 4 * nw;
    if (tid < sz - t0) d[t0 + tid] = srcb[t0 + tid];
    if (tid == 0 && seg == 0) {
        dst[0] = 0x78;          // CMF: deflate, 32 K window; FLG: check bits for level 0
        dst[1] = 0x01;
    }
    if (tid == 0 && seg == nseg - 1) {
        uint64_t s1 = 1, s2 = 0;
        for (int j = 0; j < nseg; ++j) {
            const uint32_t ab = seg_adler[(long long)b * nseg + j];
            const long long left = n_total - (long long)j * PNG_SEG;
            const uint64_t nj = (uint64_t)(left < PNG_SEG ? left : PNG_SEG);
            s2 = (s2 + nj * s1 + (ab >> 16)) % ADLER_MOD;
            s1 = (s1 + (ab & 0xffffu)) % ADLER_MOD;
        }
        uint8_t* t = d + sz;
        t[0] = (uint8_t)(s2 >> 8);
        t[1] = (uint8_t)s2;
        t[2] = (uint8_t)(s1 >> 8);
        t[3] = (uint8_t)s1;
        lengths[b] = (int)(off + sz + 4);
    }
}

}  // namespace rf

using namespace rf;

static inline long long png_nseg(long long n) { return (n + PNG_SEG - 1) / PNG_SEG; }

extern "C" int rf_png_filter_u8(const void* images_u8, int B, int H, int W, int C, int64_t image_stride, int64_t row_stride, void* out_u8,
                                int64_t out_stride, void* stream) {
    RF_CHECK(images_u8 && out_u8 && B > 0 && H > 0 && W > 0, "rf_png_filter_u8: bad arguments (B=%d H=%d W=%d)", B, H, W);
    RF_CHECK(C == 1 || C == 3 || C == 4, "rf_png_filter_u8: channels must be 1, 3 or 4 (C=%d)", C);
    RF_CHECK(B <= 65535 && (long long)W * C < (1 << 23), "rf_png_filter_u8: batch or row too large (B=%d, %lld bytes per row)", B, (long long)W * C);
    RF_CHECK(row_stride >= (int64_t)W * C && image_stride >= (int64_t)(H - 1) * row_stride + (int64_t)W * C,
             "rf_png_filter_u8: strides smaller than a row / an image");
    RF_CHECK(out_stride >= (int64_t)H * (1 + (int64_t)W * C), "rf_png_filter_u8: out stride %lld < H * (1 + W * C)", (long long)out_stride);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)H, (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, W * C, C,
                       (long long)image_stride, (long long)row_stride, (uint8_t*)out_u8, (long long)out_stride);
    RF_LAUNCH_CHECK("rf_png_filter_u8");
    return 0;
}

extern "C" int rf_png_deflate_segments(const void* streams_u8, int B, int64_t n, int64_t stream_stride, void* slots_u8, int* seg_bytes,
                                       uint32_t* seg_adler, void* stream) {
    RF_CHECK(streams_u8 && slots_u8 && seg_bytes && seg_adler && B > 0 && n > 0, "rf_png_deflate_segments: bad arguments (B=%d n=%lld)", B, (long long)n);
    RF_CHECK(B <= 65535 && stream_stride >= n && n < (1ll << 40), "rf_png_deflate_segments: bad batch / stride (B=%d stride=%lld n=%lld)", B,
             (long long)stream_stride, (long long)n);
    RF_CHECK(((uintptr_t)slots_u8 & 15) == 0, "rf_png_deflate_segments: the slots must be 16-byte aligned");
    const long long nseg = png_nseg(n);
    hipLaunchKernelGGL(png_deflate_kernel, dim3((unsigned)nseg, (unsigned)B), dim3(PNG_DT), 0, (hipStream_t)stream, (const uint8_t*)streams_u8,
                       (long long)stream_stride, (long long)n, (int)nseg, (uint8_t*)slots_u8, seg_bytes, seg_adler);
    RF_LAUNCH_CHECK("rf_png_deflate_segments");
    return 0;
}

extern "C" int rf_png_pack(const void* slots_u8, const int* seg_bytes, const uint32_t* seg_adler, int B, int64_t n, void* out_u8, int64_t out_stride,
                           int* lengths, void* stream) {
    RF_CHECK(slots_u8 && seg_bytes && seg_adler && out_u8 && lengths && B > 0 && n > 0, "rf_png_pack: bad arguments (B=%d n=%lld)", B, (long long)n);
    const long long nseg = png_nseg(n);
    RF_CHECK(B <= 65535 && out_stride >= n + 5 * nseg + 6 && n + 5 * nseg + 6 < (1ll << 31), "rf_png_pack: out stride %lld < the stored worst case %lld",
             (long long)out_stride, (long long)(n + 5 * nseg + 6));
    RF_CHECK(((uintptr_t)slots_u8 & 15) == 0, "rf_png_pack: the slots must be 16-byte aligned");
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)nseg, (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)slots_u8, seg_bytes, seg_adler,
                       (int)nseg, (long long)n, (uint8_t*)out_u8, (long long)out_stride, lengths);
    RF_LAUNCH_CHECK("rf_png_pack");
    return 0;
}
