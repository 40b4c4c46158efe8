// PNG decoding on the device (the callers' --gpu_png_decode; reface_amd/pngdec.py parses the chunks and uploads the IDAT bytes of a batch).
//   rf_png_inflate       zlib streams -> filtered streams.  The decoder itself is csrc/png_inflate.h, shared with the host test program.
//       serial plan      one wave per stream.  All 64 lanes walk the Huffman symbols on identical values (wave-uniform control flow, no
//                        exchange between lanes); lane 0 stores literals and table entries; matches, stored blocks and the write-out of
//                        the window are done by the whole wave.  The 32 KiB window and the decode tables live in LDS.
//       segmented plan   one wave per candidate start (the offsets behind 00 00 FF FF, found by the host) decodes one piece into a slot of
//                        its own; a chain kernel accepts a file whose pieces chain up exactly (png_inflate.h: chain_accept), a gather
//                        kernel moves the accepted pieces into place, and the serial kernel, enqueued behind them, skips accepted files.
//   rf_png_unfilter_u8   filtered stream -> pixels, one wave per image: a band of 64 rows at a time, lane r on row r and r pixels behind
//                        lane r - 1, so that the pixel above arrives by __shfl_up; the band's last row waits in LDS for the next band.
// Lanes of one wave exchange bytes through LDS here (lane 0's literals read by a match, a chunk of a match read by the next chunk, lane 63's
// row read by lane 0).  The compiler's own waits do not order one lane's store before another lane's load: every such pair has a
// __syncthreads() (the workgroup is the one wave) between them, named where it stands.
#include "common.h"
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
    if (status[2 * f + 1] == 1) return;          // the chain kernel accepted the segmented decode
    const long long* d = desc + (long long)f * DESC;
    const DevSrc src{comp + d[D_COMP_OFF], (uint32_t)d[D_COMP_LEN]};
    WaveSink sink{ring, filt + d[D_FILT_OFF], (uint32_t)d[D_EXPECT], 0u, 0u, 1u, 0u, (int)(threadIdx.x & 63)};
    const int rc = inflate_zlib<DevSrc, WaveSink, DevW>(src, sink, &tables);
    if ((threadIdx.x & 63) == 0) status[2 * f] = rc;
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

extern "C" int rf_png_inflate(const void* comp_u8, int64_t comp_bytes, const int64_t* desc_host, const int64_t* desc, int B, void* filt_u8,
                              int64_t filt_bytes, const int* cand_host, const int* cand, int ncand, void* slots_u8, int* pieces, int* status,
                              void* stream) {
    RF_CHECK(comp_u8 && desc_host && desc && filt_u8 && status && B > 0 && B <= (1 << 20) && ncand >= 0, "rf_png_inflate: bad arguments (B=%d ncand=%d)", B,
             ncand);
    RF_CHECK(((uintptr_t)filt_u8 & 15) == 0 && ((uintptr_t)slots_u8 & 15) == 0, "rf_png_inflate: the filtered streams and the slots must be 16-byte aligned");
    RF_CHECK(ncand == 0 || (cand_host && cand && slots_u8 && pieces), "rf_png_inflate: candidates without their buffers");
    int next = 0;
    for (int f = 0; f < B; ++f) {
        const int64_t* d = desc_host + (int64_t)f * DESC;
        RF_CHECK(pngdec_desc_ok(d, comp_bytes, filt_bytes, 0, false), "rf_png_inflate: descriptor %d is out of range", f);
        const int64_t cb = d[D_CAND_BEGIN], cn = d[D_CAND_COUNT];
        RF_CHECK(cn >= 0 && cb == next && cb + cn <= ncand, "rf_png_inflate: the candidates of file %d are not the next %lld of %d", f, (long long)cn, ncand);
        for (int64_t c = cb; c < cb + cn; ++c) {
            const int64_t off = cand_host[ncand + c];
            RF_CHECK(cand_host[c] == f && off >= 2 && off <= d[D_COMP_LEN] && (c == cb || off > cand_host[ncand + c - 1]),
                     "rf_png_inflate: candidate %lld of file %d is out of range or out of order", (long long)c, f);
        }
        next = (int)(cb + cn);
    }
    RF_CHECK(next == ncand, "rf_png_inflate: %d candidates belong to no file", ncand - next);
    hipStream_t st = (hipStream_t)stream;
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
    hipLaunchKernelGGL(png_inflate_serial_kernel, dim3((unsigned)B), dim3(64), 0, st, comp, dd, (uint8_t*)filt_u8, status);
    RF_LAUNCH_CHECK("rf_png_inflate (serial)");
    return 0;
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
