// PNG decoding on the device (the callers' --gpu_png_decode; reface_amd/pngdec.py parses the chunks and uploads the IDAT bytes of a batch).
//   rf_png_inflate       zlib streams -> filtered streams.  The decoder itself is csrc/png_inflate.h, shared with the host test program.
//       serial plan      one wave per stream.  All 64 lanes walk the Huffman symbols on identical values (wave-uniform control flow, no
//                        exchange between lanes); lane 0 stores literals and table entries; matches, stored blocks and the write-out of
//                        the window are done by the whole wave.  The 32 KiB window and the decode tables live in LDS.
//       segmented plan   one wave per candidate start (the offsets behind 00 00 FF FF, found by the host) decodes one piece into a slot of
//                        its own; a chain kernel accepts a file whose pieces chain up exactly (png_inflate.h: chain_accept), a gather
//                        kernel moves the accepted pieces into place, and the serial kernel, enqueued behind them, skips accepted files.
//   rf_png_inflate_blocks  the same sequence with the blocks plan (csrc/png_blocks.h) in front of the serial kernel: search (one lane per
//                        bit offset tests for a dynamic block header), count (one wave per candidate walks to the next candidate
//                        boundary), chain (one thread per file), decode (one wave per chain chunk writes 16-bit symbols, bytes or markers
//                        into the window in front of the chunk, to global memory), resolve (one workgroup per file, chunk by chunk).
//   rf_png_unfilter_u8   filtered stream -> pixels, one wave per image: a band of 64 rows at a time, lane r on row r and r pixels behind
//                        lane r - 1, so that the pixel above arrives by __shfl_up; the band's last row waits in LDS for the next band.
// Lanes of one wave exchange bytes through LDS here (lane 0's literals read by a match, a chunk of a match read by the next chunk, lane 63's
// row read by lane 0).  The compiler's own waits do not order one lane's store before another lane's load: every such pair has a
// __syncthreads() (the workgroup is the one wave) between them, named where it stands.
#include "common.h"
#include "png_blocks.h"
#include "png_inflate.h"

namespace rf {
using namespace pnginf;

constexpr int DEC_HALF = WINDOW / 2;          // the window is written out in halves
constexpr uint32_t DEC_MASK = WINDOW - 1;
constexpr int DESC = RF_PNGDEC_DESC;
// descriptor fields (int64 each)
enum { D_COMP_OFF = 0, D_COMP_LEN, D_FILT_OFF, D_EXPECT, D_H, D_W, D_BPP, D_OUTC, D_PIX_OFF, D_ROW_STRIDE, D_CAND_BEGIN, D_CAND_COUNT };

struct DevSrc {
    const uint8_t* p;
    uint32_t n;
    __device__ __forceinline__ uint32_t size() const { return n; }
    __device__ __forceinline__ uint32_t byte(uint32_t i) const { return p[i]; }          // callers check i < n
    __device__ __forceinline__ uint32_t word(uint32_t i) const {                         // callers check i + 4 <= n; any alignment
        uint32_t v;
        __builtin_memcpy(&v, p + i, 4);
        return v;
    }
};

struct DevW {
    __device__ static __forceinline__ bool leader() { return (threadIdx.x & 63) == 0; }
    __device__ static __forceinline__ void sync() { __syncthreads(); }
    __device__ static __forceinline__ void note_block(int) {}
    __device__ static __forceinline__ void note_match(int, int) {}
    __device__ static __forceinline__ void note_empty_stored() {}
    __device__ static __forceinline__ void note_code_length(int) {}
};

// The output of one wave: a ring of WINDOW bytes in LDS (byte i of the output at i mod WINDOW), written out to `out` (16-byte aligned) half a
// ring at a time, the Adler-32 taken on the way.  Invariant between calls: pos - flushed < DEC_HALF, so nothing is overwritten before it is out.
struct WaveSink {
    uint8_t* ring;
    uint8_t* out;
    uint32_t capv, pos, flushed, a, b;
    int lane;
    __device__ __forceinline__ uint32_t cap() const { return capv; }
    __device__ __forceinline__ uint32_t produced() const { return pos; }

    // n <= DEC_HALF bytes from `flushed` (a multiple of DEC_HALF, so the span does not wrap)
    __device__ __forceinline__ void flush(uint32_t n) {
        __syncthreads();          // every lane's stores to the span before other lanes read it
        const uint32_t* rw = (const uint32_t*)(ring + (flushed & DEC_MASK));
        uint32_t* ow = (uint32_t*)(out + flushed);
        uint32_t sa = 0, sb = 0;          // per lane at most 256 bytes: sb <= 256 * 16384 * 255 < 2^31
        const uint32_t nw = n >> 2;
        for (uint32_t w = lane; w < nw; w += 64) {
            const uint32_t v = rw[w];
            ow[w] = v;
            const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24, r = n - 4 * w;
            sa += b0 + b1 + b2 + b3;
            sb += r * b0 + (r - 1) * b1 + (r - 2) * b2 + (r - 3) * b3;
        }
        const uint32_t i = 4 * nw + lane;
        if (lane < 3 && i < n) {
            const uint32_t v = ring[(flushed + i) & DEC_MASK];
            out[flushed + i] = (uint8_t)v;
            sa += v;
            sb += (n - i) * v;
        }
        sb %= ADLER_MOD;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sa += (uint32_t)__shfl_xor((int)sa, o, 64);          // <= 16384 * 255
            sb += (uint32_t)__shfl_xor((int)sb, o, 64);          // <= 64 * 65520
        }
        b = (b + n * a + sb) % ADLER_MOD;          // n * a <= 16384 * 65520 < 2^31
        a = (a + sa) % ADLER_MOD;
        flushed += n;
    }
    __device__ __forceinline__ bool literal(uint8_t v) {
        if (pos >= capv) return false;
        if (lane == 0) ring[pos & DEC_MASK] = v;
        ++pos;
        if (pos - flushed >= DEC_HALF) flush(DEC_HALF);
        return true;
    }
    // lane i copies byte i of the match.  Distances below 64: every byte of the match is a byte of the `dist` bytes in front of it
    // (i mod dist), so no chunk reads what this match wrote.  From 64 up a chunk may read the chunk before it: a barrier after each.
    __device__ __forceinline__ int match(int len, int dist) {
        if ((uint32_t)dist > pos) return E_DISTANCE;
        if ((uint32_t)len > capv - pos) return E_TOO_LONG;
        __syncthreads();          // the bytes written so far (lane 0's literals, earlier matches) before other lanes read them
        const uint32_t start = pos;
        for (int k = 0; k < len; k += 64) {          // <= 5 iterations
            const int i = k + lane;
            if (i < len) {
                const uint32_t src = dist < 64 ? start - (uint32_t)dist + (uint32_t)(i % dist) : start + (uint32_t)i - (uint32_t)dist;
                const uint8_t v = ring[src & DEC_MASK];
                ring[(start + (uint32_t)i) & DEC_MASK] = v;
            }
            if (dist >= 64) __syncthreads();
        }
        pos += (uint32_t)len;
        if (pos - flushed >= DEC_HALF) flush(DEC_HALF);
        return OK;
    }
    // a stored block's bytes; the caller has checked p + len <= src.size() and len <= cap() - produced().
    // Every iteration copies at least one byte: pos - flushed < DEC_HALF when it starts.
    __device__ __forceinline__ void copy(const DevSrc& src, uint32_t p, uint32_t len) {
        while (len) {
            const uint32_t room = DEC_HALF - (pos - flushed), n = len < room ? len : room;
            for (uint32_t i = lane; i < n; i += 64) ring[(pos + i) & DEC_MASK] = (uint8_t)src.byte(p + i);
            pos += n;
            p += n;
            len -= n;
            if (pos - flushed >= DEC_HALF) flush(DEC_HALF);
        }
    }
    __device__ __forceinline__ uint32_t finish() {
        if (pos > flushed) flush(pos - flushed);
        return (b << 16) | a;
    }
};

__global__ __launch_bounds__(64) void png_piece_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, const int* __restrict__ cand,
                                                       int ncand, uint8_t* __restrict__ slots, Piece* __restrict__ pieces) {
    __shared__ __align__(16) uint8_t ring[WINDOW];
    __shared__ Tables tables;
    const int c = blockIdx.x;
    const long long* d = desc + (long long)cand[c] * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    WaveSink sink{ring, slots + (long long)c * WINDOW, (uint32_t)WINDOW, 0u, 0u, 0u, 0u, (int)(threadIdx.x & 63)};
    inflate_piece<DevSrc, WaveSink, DevW>(src, (uint32_t)cand[ncand + c], sink, &tables, &pieces[c]);
}

// one thread per file: the status words (error code, plan) are initialised here for both plans
__global__ __launch_bounds__(64) void png_chain_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, int B, const int* __restrict__ cand,
                                                       int ncand, Piece* __restrict__ pieces, int* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= B) return;
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    const int cb = (int)d[D_CAND_BEGIN], cn = (int)d[D_CAND_COUNT];
    const int n = cn >= 2 ? chain_accept(src, cand + ncand + cb, pieces + cb, cn, (uint32_t)d[D_EXPECT]) : 0;
    status[2 * f] = 0;
    status[2 * f + 1] = n > 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void png_gather_kernel(const long long* __restrict__ desc, const int* __restrict__ cand, const uint8_t* __restrict__ slots,
                                                         const Piece* __restrict__ pieces, const int* __restrict__ status, uint8_t* __restrict__ filt) {
    const int c = blockIdx.x, f = cand[c];
    const Piece p = pieces[c];
    if (status[2 * f + 1] != 1 || p.k < 0) return;
    const long long* d = desc + (long long)f * DESC;
    // an accepted chain: k * WINDOW + count <= expect (every piece before this one produced WINDOW bytes)
    uint8_t* dst = filt + d[D_FILT_OFF] + (long long)p.k * WINDOW;
    const uint8_t* s = slots + (long long)c * WINDOW;
    const int n16 = p.count >> 4;
    for (int i = threadIdx.x; i < n16; i += 256) ((u32x4_t*)dst)[i] = ((const u32x4_t*)s)[i];
    const int i = 16 * n16 + (int)threadIdx.x;
    if (i < p.count) dst[i] = s[i];
}

__global__ __launch_bounds__(64) void png_inflate_serial_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, uint8_t* __restrict__ filt,
                                                                int* __restrict__ status) {
    __shared__ __align__(16) uint8_t ring[WINDOW];
    __shared__ Tables tables;
    const int f = blockIdx.x;
    if (status[2 * f + 1] != 0) return;          // accepted by the segmented plan (1) or by the blocks plan (2)
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    WaveSink sink{ring, filt + d[D_FILT_OFF], (uint32_t)d[D_EXPECT], 0u, 0u, 1u, 0u, (int)(threadIdx.x & 63)};
    const int rc = inflate_zlib<DevSrc, WaveSink, DevW>(src, sink, &tables);
    if ((threadIdx.x & 63) == 0) status[2 * f] = rc;
}

// ---- the blocks plan.  Per file (blk, int32 [B, 3], then the file of every slot): the capacity in candidate slots (0: not eligible), its
// first slot and the first word of its candidate bitmap (one bit per bit of the stream).  work: per file FH_WORDS words, then the slots'
// Chunk records, the lookup tables (two words per slot) and the chain order (one word per slot); zeroed by the entry point.
enum { BK_CAP = 0, BK_SLOT_BEGIN, BK_BITMAP_OFF, BK_WORDS };
enum { FH_FOUND = 0, FH_CHAIN, FH_WANT, FH_SPARE, FH_WORDS };          // dynamic headers found (candidate 0 not counted), chain length, trailer
constexpr int CHUNK_WORDS = (int)(sizeof(Chunk) / 4);
constexpr int RESOLVE_THREADS = 1024;

struct BitmapStop {
    const uint32_t* bm;
    uint32_t nbits;
    __device__ __forceinline__ bool operator()(uint32_t bit) const { return bit < nbits && ((bm[bit >> 5] >> (bit & 31u)) & 1u); }
};
struct StopAt {
    uint32_t bit;
    __device__ __forceinline__ bool operator()(uint32_t b) const { return b == bit; }
};

// The marker sink of one wave: the chunk's symbols live in global memory (2 bytes per output byte), so a wave needs the decode tables in LDS
// and no 64 KiB ring.  Lanes exchange symbols through that memory as WaveSink's do through LDS: the __syncthreads() (the workgroup is the one
// wave) orders one lane's stores before another lane's loads.
struct WaveMarkSink {
    uint16_t* sym;          // cap() symbols
    uint32_t capv, pos;
    int lane;
    __device__ __forceinline__ uint32_t cap() const { return capv; }
    __device__ __forceinline__ uint32_t produced() const { return pos; }
    __device__ __forceinline__ bool literal(uint8_t v) {
        if (pos >= capv) return false;
        if (lane == 0) sym[pos] = v;
        ++pos;
        return true;
    }
    // lane i copies symbol i of the match; a source in front of the chunk's first byte is the marker 256 + WINDOW + (its index, negative).
    // dist <= WINDOW, so that index is at least -WINDOW.  Distances below 64 and from 64 up as in WaveSink::match.
    __device__ __forceinline__ int match(int len, int dist) {
        if (dist > WINDOW) return E_DISTANCE;
        if ((uint32_t)len > capv - pos) return E_TOO_LONG;
        __syncthreads();          // the symbols written so far before other lanes read them
        const uint32_t start = pos;
        for (int k = 0; k < len; k += 64) {          // <= 5 iterations
            const int i = k + lane;
            if (i < len) {
                const int s = dist < 64 ? (int)start - dist + (i % dist) : (int)start + i - dist;          // < start + i
                sym[start + (uint32_t)i] = s < 0 ? (uint16_t)(256 + WINDOW + s) : sym[s];
            }
            if (dist >= 64) __syncthreads();
        }
        pos += (uint32_t)len;
        return OK;
    }
    __device__ __forceinline__ void copy(const DevSrc& src, uint32_t p, uint32_t len) {          // the caller checked both ranges
        for (uint32_t i = lane; i < len; i += 64) sym[pos + i] = (uint16_t)src.byte(p + i);
        pos += len;
    }
    __device__ __forceinline__ uint32_t finish() { return 0; }
};

// one lane per bit offset (blockIdx.y: the file).  The lane of FIRST_BIT fills slot 0, candidate 0; a hit takes the next slot, sets its bit
// in the bitmap (what the walkers ask) and enters the lookup from bit to slot (what the chain asks).
__global__ __launch_bounds__(256) void png_blk_search_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, const int* __restrict__ blk,
                                                            const int* __restrict__ status, uint32_t* __restrict__ bitmap, int* __restrict__ fhdr,
                                                            Chunk* __restrict__ chunks, int* __restrict__ hash) {
    const int f = blockIdx.y, cap = blk[BK_WORDS * f + BK_CAP];
    if (cap == 0 || status[2 * f + 1] == 1) return;          // not eligible, or taken by the segmented plan
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    const uint32_t bit = FIRST_BIT + blockIdx.x * 256u + threadIdx.x;          // the grid covers the longest eligible stream: < 2^31
    if (bit >= 8u * src.n) return;
    const int sb = blk[BK_WORDS * f + BK_SLOT_BEGIN];
    if (bit == FIRST_BIT) {
        if (zlib_header(src) == OK) chunks[sb].start = FIRST_BIT;
        return;
    }
    if (!dyn_header_at(src, bit)) return;
    atomicOr(&bitmap[blk[BK_WORDS * f + BK_BITMAP_OFF] + (int)(bit >> 5)], 1u << (bit & 31u));
    const int slot = 1 + atomicAdd(&fhdr[FH_WORDS * f + FH_FOUND], 1);
    if (slot >= cap) return;          // overflow: the chain kernel sees the count and leaves the file to the serial plan
    chunks[sb + slot].start = bit;
    int* tab = hash + 2 * sb;
    const uint32_t tsize = 2u * (uint32_t)cap;
    uint32_t h = blk_hash(bit, tsize);
    for (uint32_t i = 0; i < tsize; ++i) {          // the table has twice the slots: a free word exists
        if (atomicCAS(&tab[h], 0, slot + 1) == 0) break;
        h = h + 1 == tsize ? 0 : h + 1;
    }
}

// one wave per slot: the filled ones walk whole blocks up to the next candidate boundary and count
__global__ __launch_bounds__(64) void png_blk_count_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, const int* __restrict__ blk,
                                                          int B, const int* __restrict__ status, const uint32_t* __restrict__ bitmap,
                                                          const int* __restrict__ fhdr, Chunk* __restrict__ chunks) {
    __shared__ Tables tables;
    const int s = blockIdx.x, f = blk[BK_WORDS * B + s];
    const int cap = blk[BK_WORDS * f + BK_CAP], local = s - blk[BK_WORDS * f + BK_SLOT_BEGIN], found = 1 + fhdr[FH_WORDS * f + FH_FOUND];
    if (status[2 * f + 1] == 1 || found > cap || local >= found) return;
    const uint32_t start = chunks[s].start;
    if (start < FIRST_BIT) return;          // slot 0 of a stream without a zlib header
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    CountSink sink{(uint32_t)d[D_EXPECT], 0u};
    WalkResult r;
    walk_blocks<DevSrc, CountSink, DevW, BitmapStop>(src, start, sink, &tables, BitmapStop{bitmap + blk[BK_WORDS * f + BK_BITMAP_OFF], 8u * src.n}, &r);
    if ((threadIdx.x & 63) == 0) {
        chunks[s].end = r.end;
        chunks[s].count = r.count;
        chunks[s].flags = (r.status == OK ? 1 : 0) | (r.final ? 2 : 0);
    }
}

// one thread per file
__global__ __launch_bounds__(64) void png_blk_chain_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, const int* __restrict__ blk, int B,
                                                          const int* __restrict__ status, int* __restrict__ fhdr, Chunk* __restrict__ chunks,
                                                          const int* __restrict__ hash, int* __restrict__ order) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= B) return;
    const int cap = blk[BK_WORDS * f + BK_CAP], sb = blk[BK_WORDS * f + BK_SLOT_BEGIN], found = 1 + fhdr[FH_WORDS * f + FH_FOUND];
    if (cap == 0 || status[2 * f + 1] == 1 || found > cap) return;          // the chain length stays 0
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    uint32_t want = 0;
    const int n = blocks_chain_accept(src, chunks + sb, found, hash + 2 * sb, 2u * (uint32_t)cap, order + sb, (uint32_t)d[D_EXPECT], &want);
    fhdr[FH_WORDS * f + FH_CHAIN] = n;
    fhdr[FH_WORDS * f + FH_WANT] = (int)want;
}

// one wave per slot: a chunk on an accepted chain is walked again, to the end bit the count stage found, into its place among the symbols
__global__ __launch_bounds__(64) void png_blk_decode_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ desc, const int* __restrict__ blk,
                                                           int B, const int* __restrict__ fhdr, Chunk* __restrict__ chunks, uint16_t* __restrict__ marks) {
    __shared__ Tables tables;
    const int s = blockIdx.x, f = blk[BK_WORDS * B + s];
    if (fhdr[FH_WORDS * f + FH_CHAIN] <= 0) return;
    const Chunk c = chunks[s];
    if (c.k <= 0) return;
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    // an accepted chain: off + count <= expect, so the symbols stay inside the file's part of marks
    WaveMarkSink sink{marks + d[D_FILT_OFF] + c.off, c.count, 0u, (int)(threadIdx.x & 63)};
    WalkResult r;
    walk_blocks<DevSrc, WaveMarkSink, DevW, StopAt>(src, c.start, sink, &tables, StopAt{c.end}, &r);
    if ((threadIdx.x & 63) == 0 && r.status == OK && r.end == c.end && r.count == c.count) chunks[s].flags = c.flags | 4;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* sh) {          // v <= 65520 per thread; every thread gets the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    __syncthreads();          // the readers of the call before are done
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < RESOLVE_THREADS / 64; ++w) t += sh[w];
    return t;
}

// one workgroup per file: its chain chunks in order, every symbol of a chunk in parallel, a barrier between chunks (a marker reads bytes of
// the chunks before).  The plan word becomes 2 only if every marker pointed into the stream and the Adler-32 is the trailer's.
__global__ __launch_bounds__(RESOLVE_THREADS) void png_blk_resolve_kernel(const long long* __restrict__ desc, const int* __restrict__ blk,
                                                                         const int* __restrict__ fhdr, const Chunk* __restrict__ chunks,
                                                                         const int* __restrict__ order, const uint16_t* __restrict__ marks,
                                                                         uint8_t* __restrict__ filt, int* __restrict__ status) {
    __shared__ uint32_t sh[RESOLVE_THREADS / 64];
    const int f = blockIdx.x, n = fhdr[FH_WORDS * f + FH_CHAIN];
    if (n <= 0) return;
    const long long* d = desc + (long long)f * DESC;
    const int sb = blk[BK_WORDS * f + BK_SLOT_BEGIN];
    uint8_t* out = filt + d[D_FILT_OFF];
    const uint16_t* sym = marks + d[D_FILT_OFF];
    uint64_t s1 = 1, s2 = 0;
    uint32_t bad = 0;
    for (int k = 0; k < n; ++k) {          // n <= the file's slots
        const Chunk c = chunks[sb + order[sb + k]];
        if (!(c.flags & 4)) {          // (the same for every thread)
            bad = 1;
            break;
        }
        uint64_t a = 0, b = 0;          // per thread at most 2^21 bytes of a chunk below 2^31: b < 2^21 * 2^31 * 2^8
        for (uint32_t i0 = threadIdx.x; i0 < c.count; i0 += 4 * RESOLVE_THREADS) {
            uint32_t sv[4];
            uint8_t v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t i = i0 + j * RESOLVE_THREADS;
                sv[j] = i < c.count ? sym[c.off + i] : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = 0;
                if (!resolve_sym(sv[j], c.off, out, &v[j])) bad = 1;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t i = i0 + j * RESOLVE_THREADS;
                if (i < c.count) {
                    out[c.off + i] = v[j];
                    a += v[j];
                    b += (uint64_t)(c.count - i) * v[j];
                }
            }
        }
        const uint32_t ca = block_sum((uint32_t)(a % ADLER_MOD), sh) % ADLER_MOD, cb = block_sum((uint32_t)(b % ADLER_MOD), sh) % ADLER_MOD;
        adler_push(&s1, &s2, c.count, ca, cb);
        __syncthreads();          // this chunk's bytes before the markers of the next one read them
    }
    bad = block_sum(bad, sh);
    if (threadIdx.x == 0 && bad == 0 && (uint32_t)fhdr[FH_WORDS * f + FH_WANT] == (uint32_t)((s2 << 16) | s1)) status[2 * f + 1] = 2;
}

// One wave per image.  Pixels travel packed, byte c of a word = channel c.  At step t lane r (row band * 64 + r) is at pixel x = t - r; `cur`
// is the pixel it reconstructed last, so __shfl_up(cur) is the pixel above, and the value that was above one step earlier is above-left.
__global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* __restrict__ filt, const long long* __restrict__ desc, uint8_t* __restrict__ pix,
                                                          int* __restrict__ status) {
    extern __shared__ uint32_t prevrow[];          // the last row of the band before, W words
    const int f = blockIdx.x, lane = threadIdx.x & 63;
    if (status[2 * f] != 0) return;
    const long long* d = desc + (long long)f * DESC;
    const int H = (int)d[D_H], W = (int)d[D_W], bpp = (int)d[D_BPP], oc = (int)d[D_OUTC];
    const long long rowlen = 1 + (long long)W * bpp, rs = d[D_ROW_STRIDE];
    const uint8_t* fs = filt + d[D_FILT_OFF];
    uint8_t* po = pix + d[D_PIX_OFF];
    int bad = 0;
    for (int band = 0; band * 64 < H; ++band) {
        const int y = band * 64 + lane;
        const bool active = y < H;
        int ft = active ? (int)fs[(long long)y * rowlen] : 0;
        if (ft > 4) {
            bad = 1;
            ft = 0;
        }
        const uint8_t* r = fs + (long long)y * rowlen + 1;
        uint8_t* o = po + (long long)y * rs;
        uint32_t left = 0, up = 0, upleft = 0, cur = 0;
        __syncthreads();          // lane 63's stores of the band before, before lane 0 reads them
        for (int t = 0; t < W + 63; ++t) {
            const int x = t - lane;
            uint32_t above = (uint32_t)__shfl_up((int)cur, 1, 64);
            if (lane == 0) above = (band > 0 && x < W) ? prevrow[x] : 0u;
            upleft = up;
            up = above;
            if (x == 0) {
                upleft = 0;
                left = 0;
            }
            if (active && x >= 0 && x < W) {
                uint32_t v = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c < bpp) {
                        const int sh = 8 * c;
                        const int pred = png_predict(ft, (int)((left >> sh) & 255u), (int)((up >> sh) & 255u), (int)((upleft >> sh) & 255u));
                        v |= (((uint32_t)r[(long long)x * bpp + c] + (uint32_t)pred) & 255u) << sh;
                    }
                }
                cur = v;
                left = v;
                // the file's own channels, or, converting: grey (+ alpha) -> its one sample on every output channel, RGBA -> R, G, B
                const bool spread = bpp <= 2 && oc != bpp;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < oc) o[(long long)x * oc + j] = (uint8_t)(v >> (spread ? 0 : 8 * j));
                if (lane == 63) prevrow[x] = v;
            }
        }
    }
    if (__any(bad) && lane == 0) status[2 * f] = E_FILTER;
}

static bool pngdec_desc_ok(const int64_t* d, int64_t comp_bytes, int64_t filt_bytes, int64_t pix_bytes, bool pixels) {
    const int64_t H = d[D_H], W = d[D_W], bpp = d[D_BPP], oc = d[D_OUTC];
    if (d[D_EXPECT] < 1 || d[D_EXPECT] >= (1ll << 31)) return false;
    if (pixels && (H < 1 || W < 1 || bpp < 1 || bpp > 4 || W > 8192 || H > (1 << 20) || d[D_EXPECT] != H * (1 + W * bpp))) return false;
    if (d[D_COMP_OFF] < 0 || d[D_COMP_LEN] < 0 || d[D_COMP_LEN] >= (1ll << 31) || d[D_COMP_OFF] + d[D_COMP_LEN] > comp_bytes) return false;
    if (d[D_FILT_OFF] < 0 || (d[D_FILT_OFF] & 15) || d[D_FILT_OFF] + d[D_EXPECT] > filt_bytes) return false;
    if (pixels) {
        const bool conv = oc == bpp || (bpp <= 2 && (oc == 1 || oc == 3)) || (bpp == 4 && oc == 3);
        if (!conv || d[D_PIX_OFF] < 0 || d[D_ROW_STRIDE] < W * oc || d[D_PIX_OFF] + (H - 1) * d[D_ROW_STRIDE] + W * oc > pix_bytes) return false;
    }
    return true;
}

}  // namespace rf

using namespace rf;

// the checks and the launches both inflate entry points share: pieces -> chain -> gather (the segmented plan; the chain kernel also
// initialises the status words), and the serial kernel behind everything
static int png_inflate_front(const char* who, const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* filt_u8,
                             int64_t filt_bytes, const int* cand_host, const int* cand, int ncand, void* slots_u8, int* pieces, int* status, hipStream_t st) {
    RF_CHECK(comp_u8 && desc_host && desc && filt_u8 && status && B > 0 && B <= (1 << 20) && ncand >= 0, "%s: bad arguments (B=%d ncand=%d)", who, B, ncand);
    RF_CHECK(((uintptr_t)filt_u8 & 15) == 0 && ((uintptr_t)slots_u8 & 15) == 0, "%s: the filtered streams and the slots must be 16-byte aligned", who);
    RF_CHECK(ncand == 0 || (cand_host && cand && slots_u8 && pieces), "%s: candidates without their buffers", who);
    int next = 0;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(pngdec_desc_ok(d, comp_bytes, filt_bytes, 0, false), "%s: descriptor %d is out of range", who, f);
        const int64_t cb = d[D_CAND_BEGIN], cn = d[D_CAND_COUNT];
        RF_CHECK(cn >= 0 && cb == next && cb + cn <= ncand, "%s: the candidates of file %d are not the next %lld of %d", who, f, (long long)cn, ncand);
        for (int64_t c = cb; c < cb + cn; ++c) {
            const int64_t off = cand_host[ncand + c];
            RF_CHECK(cand_host[c] == f && off >= 2 && off <= d[D_COMP_LEN] && (c == cb || off > cand_host[ncand + c - 1]),
                     "%s: candidate %lld of file %d is out of range or out of order", who, (long long)c, f);
        }
        next = (int)(cb + cn);
    }
    RF_CHECK(next == ncand, "%s: %d candidates belong to no file", who, ncand - next);
    const uint8_t* comp = (const uint8_t*)comp_u8;
    const long long* dd = (const long long*)desc;
    if (ncand > 0) {
        hipLaunchKernelGGL(png_piece_kernel, dim3((unsigned)ncand), dim3(64), 0, st, comp, dd, cand, ncand, (uint8_t*)slots_u8, (Piece*)pieces);
        RF_LAUNCH_CHECK("rf_png_inflate (pieces)");
    }
    hipLaunchKernelGGL(png_chain_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, comp, dd, B, cand, ncand, (Piece*)pieces, status);
    RF_LAUNCH_CHECK("rf_png_inflate (chain)");
    if (ncand > 0) {
        hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)ncand), dim3(256), 0, st, dd, cand, (const uint8_t*)slots_u8, (const Piece*)pieces,
                           (const int*)status, (uint8_t*)filt_u8);
        RF_LAUNCH_CHECK("rf_png_inflate (gather)");
    }
    return 0;
}

static int png_inflate_serial(const void* comp_u8, const int64_t* desc, int B, void* filt_u8, int* status, hipStream_t st) {
    hipLaunchKernelGGL(png_inflate_serial_kernel, dim3((unsigned)B), dim3(64), 0, st, (const uint8_t*)comp_u8, (const long long*)desc, (uint8_t*)filt_u8, status);
    RF_LAUNCH_CHECK("rf_png_inflate (serial)");
    return 0;
}

extern "C" int rf_png_inflate(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* filt_u8,
                              int64_t filt_bytes, const int* cand_host, const int* cand, int ncand, void* slots_u8, int* pieces, int* status,
                              void* stream) {
    const int rc = png_inflate_front("rf_png_inflate", comp_u8, comp_bytes, desc_host, desc, B, filt_u8, filt_bytes, cand_host, cand, ncand, slots_u8, pieces,
                                     status, (hipStream_t)stream);
    return rc ? rc : png_inflate_serial(comp_u8, desc, B, filt_u8, status, (hipStream_t)stream);
}

extern "C" int rf_png_inflate_blocks(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* filt_u8,
                                     int64_t filt_bytes, const int* cand_host, const int* cand, int ncand, void* slots_u8, int* pieces, int* status,
                                     const int* blk_host, const int* blk, int nslot, void* bitmap_u32, int64_t bitmap_words, int* work, int64_t work_words,
                                     void* marks_u16, int64_t marks_count, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RF_CHECK(blk_host && blk && work && nslot >= 0 && nslot <= (1 << 24) && bitmap_words >= 0 && marks_count >= 0,
             "rf_png_inflate_blocks: bad arguments (nslot=%d)", nslot);
    RF_CHECK(nslot == 0 || (bitmap_u32 && marks_u16 && B <= 65535), "rf_png_inflate_blocks: slots without their buffers, or more than 65535 files (B=%d)", B);
    int rc = png_inflate_front("rf_png_inflate_blocks", comp_u8, comp_bytes, desc_host, desc, B, filt_u8, filt_bytes, cand_host, cand, ncand, slots_u8, pieces,
                               status, st);
    if (rc) return rc;          // (the descriptors are in range from here on)
    int64_t next = 0, next_bm = 0, max_len = 0;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        const int* b = blk_host + (int64_t)f * BK_WORDS;
        if (b[BK_CAP] == 0) continue;
        RF_CHECK(b[BK_CAP] >= 2 && d[D_COMP_LEN] < (int64_t)BLK_MAX_STREAM && b[BK_SLOT_BEGIN] == next && next + b[BK_CAP] <= nslot && b[BK_BITMAP_OFF] == next_bm,
                 "rf_png_inflate_blocks: the slots or the bitmap of file %d are out of range or out of order, or its stream is too long", f);
        for (int64_t s = next; s < next + b[BK_CAP]; ++s)
            RF_CHECK(blk_host[(int64_t)BK_WORDS * B + s] == f, "rf_png_inflate_blocks: slot %lld does not name file %d", (long long)s, f);
        next += b[BK_CAP];
        next_bm += (d[D_COMP_LEN] + 3) / 4;
        RF_CHECK(next_bm < (1ll << 31), "rf_png_inflate_blocks: the candidate bitmaps pass 2^31 words at file %d", f);
        max_len = d[D_COMP_LEN] > max_len ? d[D_COMP_LEN] : max_len;
    }
    RF_CHECK(next == nslot && next_bm <= bitmap_words, "rf_png_inflate_blocks: %lld of %d slots belong to a file, the bitmaps need %lld of %lld words",
             (long long)next, nslot, (long long)next_bm, (long long)bitmap_words);
    const int64_t used = (int64_t)FH_WORDS * B + (int64_t)(CHUNK_WORDS + 3) * nslot;
    RF_CHECK(work_words >= used && marks_count >= (nslot ? filt_bytes : 0), "rf_png_inflate_blocks: the work buffer needs %lld words, the symbols %lld",
             (long long)used, (long long)filt_bytes);
    RF_CHECK(hipMemsetAsync(work, 0, (size_t)used * 4, st) == hipSuccess, "rf_png_inflate_blocks: clearing the work buffer failed");
    if (nslot > 0 && max_len * 8 > (int64_t)FIRST_BIT) {
        RF_CHECK(hipMemsetAsync(bitmap_u32, 0, (size_t)next_bm * 4, st) == hipSuccess, "rf_png_inflate_blocks: clearing the bitmaps failed");
        const uint8_t* comp = (const uint8_t*)comp_u8;
        const long long* dd = (const long long*)desc;
        int* fhdr = work;
        Chunk* chunks = (Chunk*)(work + (int64_t)FH_WORDS * B);
        int* hash = (int*)(chunks + nslot);
        int* order = hash + 2 * (int64_t)nslot;
        const unsigned gx = (unsigned)((max_len * 8 - FIRST_BIT + 255) / 256);          // max_len < 2^28
        hipLaunchKernelGGL(png_blk_search_kernel, dim3(gx, (unsigned)B), dim3(256), 0, st, comp, dd, blk, (const int*)status, (uint32_t*)bitmap_u32, fhdr, chunks,
                           hash);
        RF_LAUNCH_CHECK("rf_png_inflate_blocks (search)");
        hipLaunchKernelGGL(png_blk_count_kernel, dim3((unsigned)nslot), dim3(64), 0, st, comp, dd, blk, B, (const int*)status, (const uint32_t*)bitmap_u32,
                           (const int*)fhdr, chunks);
        RF_LAUNCH_CHECK("rf_png_inflate_blocks (count)");
        hipLaunchKernelGGL(png_blk_chain_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, comp, dd, blk, B, (const int*)status, fhdr, chunks,
                           (const int*)hash, order);
        RF_LAUNCH_CHECK("rf_png_inflate_blocks (chain)");
        hipLaunchKernelGGL(png_blk_decode_kernel, dim3((unsigned)nslot), dim3(64), 0, st, comp, dd, blk, B, (const int*)fhdr, chunks, (uint16_t*)marks_u16);
        RF_LAUNCH_CHECK("rf_png_inflate_blocks (decode)");
        hipLaunchKernelGGL(png_blk_resolve_kernel, dim3((unsigned)B), dim3(RESOLVE_THREADS), 0, st, dd, blk, (const int*)fhdr, (const Chunk*)chunks,
                           (const int*)order, (const uint16_t*)marks_u16, (uint8_t*)filt_u8, status);
        RF_LAUNCH_CHECK("rf_png_inflate_blocks (resolve)");
    }
    return png_inflate_serial(comp_u8, desc, B, filt_u8, status, st);
}

extern "C" int rf_png_unfilter_u8(const void* filt_u8, int64_t filt_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* pix_u8,
                                  int64_t pix_bytes, int* status, void* stream) {
    RF_CHECK(filt_u8 && desc_host && desc && pix_u8 && status && B > 0 && B <= (1 << 20), "rf_png_unfilter_u8: bad arguments (B=%d)", B);
    int64_t maxw = 1;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(pngdec_desc_ok(d, 1ll << 62, filt_bytes, pix_bytes, true), "rf_png_unfilter_u8: descriptor %d is out of range", f);
        maxw = d[D_W] > maxw ? d[D_W] : maxw;
    }
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)B), dim3(64), (size_t)maxw * 4, (hipStream_t)stream, (const uint8_t*)filt_u8, (const long long*)desc,
                       (uint8_t*)pix_u8, status);
    RF_LAUNCH_CHECK("rf_png_unfilter_u8");
    return 0;
}
