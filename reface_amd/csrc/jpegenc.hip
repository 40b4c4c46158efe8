// Baseline JPEG encoding of device-resident uint8 images (scripts/inference_swap_video.py --write_video): what reaches the host is the
// entropy-coded scan of every image, EOI included; reface_amd/mjpeg.py puts SOI .. SOS in front.  Three stages, one entry point each:
//   rf_jpeg_blocks_u8   pixels -> quantised DCT coefficients: libjpeg's rgb_ycc_convert, h2v2 downsample, jfdctint ("islow") and quantiser
//   rf_jpeg_entropy     Huffman coding with the tables the host passes (Annex K), one restart interval per MCU row, bytes stuffed
//   rf_jpeg_pack        the intervals of an image back to back, RSTn between them, EOI behind, the length written
// All arithmetic is 32-bit integer (no floating point anywhere): the bytes are libjpeg's, and tests/jpeg_refs.py restates them in numpy.
//
// Coefficient layout (RF_JPEG coef): int16, per (image b, MCU row r) a tile [64][nbr], nbr = MCUs per row * blocks per MCU; element
// [z][j] is the coefficient at zigzag position z of block j, blocks in the scan's order (per MCU Y00 Y01 Y10 Y11 Cb Cr at 4:2:0, Y Cb Cr
// at 4:4:4).  Both kernels run one lane per block, so lane j touches [z][j]: every access is coalesced over the lanes of a wave.
#include "common.h"

namespace rf {
namespace jpg {

constexpr int BLOCK_BITS = RF_JPEG_BLOCK_BITS;          // bound of a coded block whatever the tables: per coefficient a code of <= 16 bits and <= 11 amplitude bits (ZRL and EOB stand for zeros)
constexpr int ET = 128;                           // threads of an entropy workgroup = blocks coded per pass
constexpr int EBUFW = (7 + ET * BLOCK_BITS + 7 + 31) / 32 + 2;          // LDS words of the bit buffer: the carry, a pass's worst case, the tail padding, one word of spill
constexpr int HUFF_WORDS = RF_JPEG_HUFF_WORDS;

// natural (row-major) index of the coefficient at zigzag position z (mirrors reface_amd/mjpeg.py ZIGZAG; folded away where z is a constant)
__device__ __forceinline__ constexpr int zz_natural(int z) {
    constexpr unsigned char T[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return T[z];
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's rgb_ycc_convert: FIX(x) = int(x * 65536 + 0.5)
__device__ __forceinline__ int ycc(int comp, int r, int g, int b) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jfdctint's butterflies over 8 values; FIRST: the row pass (outputs scaled up by 2 bits), else the column pass
template <bool FIRST>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d0 = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d4 = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int z1 = (t12 + t13) * 4433;
    d2 = descale(z1 + t13 * 6270, N);
    d6 = descale(z1 - t12 * 15137, N);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int y1 = (t4 + t7) * -7373, y2 = (t5 + t6) * -20995, y3 = (t4 + t6) * -16069 + z5, y4 = (t5 + t7) * -3196 + z5;
    d7 = descale(t4 * 2446 + y1 + y3, N);
    d5 = descale(t5 * 16819 + y2 + y4, N);
    d3 = descale(t6 * 25172 + y2 + y3, N);
    d1 = descale(t7 * 12299 + y1 + y4, N);
}

// ================================================================================================ stage 1: blocks
// one lane per block of the scan.  A dummy block (past its component's size in blocks, inside the last MCU column / row: only Y blocks at
// 4:2:0) takes the DC of the block before it in the MCU and no AC, as libjpeg's coefficient controller does: the lane transforms that
// block again and keeps its DC.
__global__ __launch_bounds__(64) void jpeg_blocks_kernel(const uint8_t* __restrict__ img, int H, int W, int C, long long istride, long long rstride, int s420,
                                                         const int* __restrict__ quant, int16_t* __restrict__ coef, int mrows, int mcus) {
    __shared__ int q[128];
    const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    q[tid] = quant[tid] > 1 ? quant[tid] : 1;
    q[tid + 64] = quant[tid + 64] > 1 ? quant[tid + 64] : 1;
    __syncthreads();
    const int bpm = s420 ? 6 : 3, nbr = mcus * bpm;
    const int j = blockIdx.x * 64 + tid;
    if (j >= nbr) return;
    const int mcu = j / bpm;
    int k = j - mcu * bpm;
    int comp, by, bx;
    bool dummy = false;
    if (s420 && k < 4) {
        const bool col1 = 2 * mcu + 1 >= (W + 7) / 8, row1 = 2 * r + 1 >= (H + 7) / 8;          // the MCU's second block column / row is dummy
        if (k == 1 && col1) dummy = true, k = 0;
        else if (k == 2 && row1) dummy = true, k = col1 ? 0 : 1;
        else if (k == 3 && row1) dummy = true, k = col1 ? 0 : 1;
        else if (k == 3 && col1) dummy = true, k = 2;
        comp = 0, by = 2 * r + (k >> 1), bx = 2 * mcu + (k & 1);
    } else {
        comp = s420 ? k - 4 + 1 : k, by = r, bx = mcu;
    }
    const uint8_t* base = img + (long long)b * istride;
    int d[64];
    if (s420 && comp > 0) {
        // h2v2: the full-resolution chroma edge-replicated, 2 x 2 boxes averaged with the bias 1 on even and 2 on odd output columns; the
        // downsampled plane's last row replicated down
        const int hlast = (H + 1) / 2 - 1;
#pragma unroll
        for (int yy = 0; yy < 8; ++yy) {
            const int cy = imin(by * 8 + yy, hlast);
            const uint8_t* r0 = base + (long long)imin(2 * cy, H - 1) * rstride;
            const uint8_t* r1 = base + (long long)imin(2 * cy + 1, H - 1) * rstride;
#pragma unroll
            for (int xx = 0; xx < 8; ++xx) {
                const int cx = bx * 8 + xx;
                const long long x0 = (long long)imin(2 * cx, W - 1) * C, x1 = (long long)imin(2 * cx + 1, W - 1) * C;
                const int s = ycc(comp, r0[x0], r0[x0 + 1], r0[x0 + 2]) + ycc(comp, r0[x1], r0[x1 + 1], r0[x1 + 2]) +
                              ycc(comp, r1[x0], r1[x0 + 1], r1[x0 + 2]) + ycc(comp, r1[x1], r1[x1 + 1], r1[x1 + 2]);
                d[yy * 8 + xx] = ((s + 1 + (xx & 1)) >> 2) - 128;
            }
        }
    } else {
#pragma unroll
        for (int yy = 0; yy < 8; ++yy) {
            const uint8_t* row = base + (long long)imin(by * 8 + yy, H - 1) * rstride;
#pragma unroll
            for (int xx = 0; xx < 8; ++xx) {
                const long long x = (long long)imin(bx * 8 + xx, W - 1) * C;
                d[yy * 8 + xx] = ycc(comp, row[x], row[x + 1], row[x + 2]) - 128;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct8<true>(d[8 * i], d[8 * i + 1], d[8 * i + 2], d[8 * i + 3], d[8 * i + 4], d[8 * i + 5], d[8 * i + 6], d[8 * i + 7]);
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct8<false>(d[i], d[8 + i], d[16 + i], d[24 + i], d[32 + i], d[40 + i], d[48 + i], d[56 + i]);
    int16_t* out = coef + ((long long)b * mrows + r) * 64 * nbr + j;
    const int* qt = q + (comp > 0 ? 64 : 0);
#pragma unroll
    for (int z = 0; z < 64; ++z) {
        const int v = d[zz_natural(z)];
        const uint32_t q8 = 8u * (uint32_t)qt[z];
        const int m = (int)(((uint32_t)(v < 0 ? -v : v) + (q8 >> 1)) / q8);
        out[(long long)z * nbr] = (int16_t)((dummy && z > 0) ? 0 : (v < 0 ? -m : m));
    }
}

// ================================================================================================ stage 2: entropy coding
// exclusive sum over the ET threads of a workgroup; `ws` holds one word per wave
__device__ __forceinline__ int scan_excl(int v, int* ws, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < ET / 64; ++w) {
        const int x = ws[w];
        tot += x;
        if (w < wave) pre += x;
    }
    *total = tot;
    return pre + inc - v;
}

// `nb` (1 .. 27) bits of `val` at bit `off` of the buffer, most significant bit first: byte i of the stream is bits 31 - 8 (i & 3) .. of word i >> 2
__device__ __forceinline__ void put_be(uint32_t* buf, int off, uint32_t val, int nb) {
    const int w = off >> 5, sh = 32 - (off & 31) - nb;
    if (sh >= 0) {
        atomicOr(&buf[w], val << sh);
    } else {
        atomicOr(&buf[w], val >> -sh);
        atomicOr(&buf[w + 1], val << (32 + sh));
    }
}
__device__ __forceinline__ uint32_t byte_at(const uint32_t* buf, int i) { return (buf[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; }

// a value's category and amplitude bits (a negative v of category n is coded as v + 2^n - 1)
__device__ __forceinline__ void category(int v, int& n, uint32_t& amp) {
    n = v == 0 ? 0 : 32 - __clz(v < 0 ? -v : v);
    amp = (uint32_t)(v < 0 ? v + (1 << n) - 1 : v) & ((1u << n) - 1u);
}

// the bits of one block: DC difference, (run, size) symbols with ZRL and EOB.  WRITE: put them at bit `off` of buf; returns their number
template <bool WRITE>
__device__ __forceinline__ int code_block(const int16_t (&v)[64], int diff, const uint32_t* hdc, const uint32_t* hac, uint32_t* buf, int off) {
    int bits = 0, n;
    uint32_t amp;
    category(diff < -2047 ? -2047 : (diff > 2047 ? 2047 : diff), n, amp);          // (8-bit samples stay inside: the clamps only keep foreign coefficients within BLOCK_BITS)
    {
        const uint32_t e = hdc[n];
        const int len = (int)(e & 31u) + n;
        if (WRITE) put_be(buf, off, ((e >> 5) << n) | amp, len);
        bits += len;
    }
    int run = 0;
#pragma unroll
    for (int z = 1; z < 64; ++z) {
        const int x = v[z] < -1023 ? -1023 : (v[z] > 1023 ? 1023 : (int)v[z]);
        if (x == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            const uint32_t e = hac[0xF0];
            if (WRITE) put_be(buf, off + bits, e >> 5, (int)(e & 31u));
            bits += (int)(e & 31u);
            run -= 16;
        }
        category(x, n, amp);
        const uint32_t e = hac[(run << 4) | n];
        const int len = (int)(e & 31u) + n;
        if (WRITE) put_be(buf, off + bits, ((e >> 5) << n) | amp, len);
        bits += len;
        run = 0;
    }
    if (run > 0) {
        const uint32_t e = hac[0];
        if (WRITE) put_be(buf, off + bits, e >> 5, (int)(e & 31u));
        bits += (int)(e & 31u);
    }
    return bits;
}

// one workgroup per (MCU row, image) = one restart interval.  The row's blocks are coded ET at a time, one lane each: lengths, an exclusive
// scan for the bit offsets, the bits OR-ed into an LDS buffer (cleared to the length the scan gave), then the whole bytes of the buffer
// copied to the slot with a second scan for the 00 behind every FF; the 0 .. 7 bits left over open the next pass's buffer.  Nothing is
// sized by the content: the buffer holds ET blocks of BLOCK_BITS, the slot the row's worst case.
__global__ __launch_bounds__(ET) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, int mrows, int nbr, int bpm, const uint32_t* __restrict__ huff,
                                                          uint8_t* __restrict__ slots, long long slot_stride, int* __restrict__ seg_bytes) {
    __shared__ uint32_t buf[EBUFW];
    __shared__ uint32_t hf[HUFF_WORDS];
    __shared__ int ws[ET / 64];
    const int tid = threadIdx.x, r = blockIdx.x, b = blockIdx.y;
    const int16_t* rowc = coef + ((long long)b * mrows + r) * 64 * nbr;
    uint8_t* slot = slots + ((long long)b * mrows + r) * slot_stride;
    for (int i = tid; i < HUFF_WORDS; i += ET) {          // (whatever the caller's words hold, a length stays <= 16 and a code inside it: BLOCK_BITS holds)
        const uint32_t e = huff[i], len = (e & 31u) > 16u ? 16u : (e & 31u);
        hf[i] = (((e >> 5) & ((1u << len) - 1u)) << 5) | len;
    }
    int carry = 0, outpos = 0;
    uint32_t carry_val = 0;
    for (int c0 = 0; c0 < nbr; c0 += ET) {
        const int j = c0 + tid;
        const bool valid = j < nbr, last = c0 + ET >= nbr;
        int16_t v[64];
        int diff = 0, cls = 0;
        if (valid) {
#pragma unroll
            for (int z = 0; z < 64; ++z) v[z] = rowc[(long long)z * nbr + j];
            const int k = j % bpm;
            // the block of the same component before this one in the row (none: the interval starts with the predictor at 0)
            const int jp = bpm == 6 ? (k == 0 ? j - 3 : (k < 4 ? j - 1 : j - 6)) : j - 3;
            cls = bpm == 6 ? (k >= 4) : (k >= 1);
            diff = (int)v[0] - (jp >= 0 ? (int)rowc[jp] : 0);
        } else {
#pragma unroll
            for (int z = 0; z < 64; ++z) v[z] = 0;
        }
        const uint32_t* hdc = hf + 272 * cls;
        const uint32_t* hac = hdc + 16;
        __syncthreads();          // (the first pass: the tables are in LDS)
        const int mybits = valid ? code_block<false>(v, diff, hdc, hac, buf, 0) : 0;
        int total;
        const int myoff = carry + scan_excl(mybits, ws, &total);
        const int endbits = carry + total;
        const int tail = last ? (8 - (endbits & 7)) & 7 : 0;          // 1-bits that pad the interval to a byte
        const int nwords = (endbits + tail + 31) / 32 + 1;
        for (int i = tid; i < nwords; i += ET) buf[i] = 0;
        __syncthreads();
        if (tid == 0) {
            if (carry) put_be(buf, 0, carry_val, carry);
            if (tail) put_be(buf, endbits, (1u << tail) - 1u, tail);
        }
        if (valid) code_block<true>(v, diff, hdc, hac, buf, myoff);
        __syncthreads();
        const int nbytes = (endbits + tail) >> 3;
        const int per = (nbytes + ET - 1) / ET;
        const int i0 = imin(tid * per, nbytes), i1 = imin(i0 + per, nbytes);
        int ff = 0;
        for (int i = i0; i < i1; ++i) ff += byte_at(buf, i) == 0xffu ? 1 : 0;
        int fftotal;
        const int ffbefore = scan_excl(ff, ws, &fftotal);
        uint8_t* dst = slot + outpos + i0 + ffbefore;
        for (int i = i0; i < i1; ++i) {
            const uint32_t x = byte_at(buf, i);
            *dst++ = (uint8_t)x;
            if (x == 0xffu) *dst++ = 0;
        }
        carry = (endbits + tail) & 7;
        carry_val = carry ? byte_at(buf, nbytes) >> (8 - carry) : 0u;
        outpos += nbytes + fftotal;
        __syncthreads();          // every lane has read its bytes and the carry before the buffer is cleared again
    }
    if (tid == 0) seg_bytes[(long long)b * mrows + r] = outpos;
}

// ================================================================================================ stage 3: pack
// one workgroup per interval: its offset = the sizes before it + 2 per marker; RSTn behind every interval but the last, EOI behind that
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint8_t* __restrict__ slots, long long slot_stride, const int* __restrict__ seg_bytes, int mrows,
                                                        uint8_t* __restrict__ out, long long ostride, int* __restrict__ lengths) {
    __shared__ long long ws[4];
    const int tid = threadIdx.x, r = blockIdx.x, b = blockIdx.y;
    const int* sizes = seg_bytes + (long long)b * mrows;
    long long before = 0;
    for (int i = tid; i < r; i += 256) before += (long long)sizes[i] + 2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if ((tid & 63) == 0) ws[tid >> 6] = before;
    __syncthreads();
    const long long off = ws[0] + ws[1] + ws[2] + ws[3];
    const int sz = sizes[r];
    const uint8_t* src = slots + ((long long)b * mrows + r) * slot_stride;
    uint8_t* dst = out + (long long)b * ostride + off;
    for (int i = tid; i < sz; i += 256) dst[i] = src[i];
    if (tid == 0) {
        dst[sz] = 0xff;
        dst[sz + 1] = (uint8_t)(r == mrows - 1 ? 0xd9 : 0xd0 + (r & 7));
        if (r == mrows - 1) lengths[b] = (int)(off + sz + 2);
    }
}

}  // namespace jpg
}  // namespace rf

using namespace rf;

static int jpeg_geometry(const char* who, int H, int W, int subsampling, int* mrows, int* mcus, int* bpm) {
    RF_CHECK(subsampling == 420 || subsampling == 444, "%s: subsampling must be 420 or 444 (got %d)", who, subsampling);
    RF_CHECK(H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "%s: sizes are 1 .. 65535 (H=%d W=%d)", who, H, W);
    const int m = subsampling == 420 ? 16 : 8;
    *mrows = (H + m - 1) / m, *mcus = (W + m - 1) / m, *bpm = subsampling == 420 ? 6 : 3;
    return 0;
}

extern "C" int rf_jpeg_blocks_u8(const void* images_u8, int B, int H, int W, int C, int64_t image_stride, int64_t row_stride, int subsampling,
                                 const int* quant, int16_t* coef, void* stream) {
    RF_CHECK(images_u8 && quant && coef && B > 0 && B <= 65535, "rf_jpeg_blocks_u8: bad arguments (B=%d)", B);
    RF_CHECK(C == 3 || C == 4, "rf_jpeg_blocks_u8: channels must be 3 or 4 (C=%d)", C);
    int mrows, mcus, bpm;
    if (jpeg_geometry("rf_jpeg_blocks_u8", H, W, subsampling, &mrows, &mcus, &bpm)) return 1;
    RF_CHECK(row_stride >= (int64_t)W * C && image_stride >= (int64_t)(H - 1) * row_stride + (int64_t)W * C,
             "rf_jpeg_blocks_u8: strides smaller than a row / an image");
    hipLaunchKernelGGL(jpg::jpeg_blocks_kernel, dim3((unsigned)((mcus * bpm + 63) / 64), (unsigned)mrows, (unsigned)B), dim3(64), 0, (hipStream_t)stream,
                       (const uint8_t*)images_u8, H, W, C, (long long)image_stride, (long long)row_stride, subsampling == 420 ? 1 : 0, quant, coef, mrows, mcus);
    RF_LAUNCH_CHECK("rf_jpeg_blocks_u8");
    return 0;
}

extern "C" int rf_jpeg_entropy(const int16_t* coef, int B, int mcu_rows, int mcus, int subsampling, const uint32_t* huff, void* slots_u8, int64_t slot_stride,
                               int* seg_bytes, void* stream) {
    RF_CHECK(coef && huff && slots_u8 && seg_bytes && B > 0 && B <= 65535, "rf_jpeg_entropy: bad arguments (B=%d)", B);
    RF_CHECK(subsampling == 420 || subsampling == 444, "rf_jpeg_entropy: subsampling must be 420 or 444 (got %d)", subsampling);
    RF_CHECK(mcu_rows >= 1 && mcu_rows <= 8192 && mcus >= 1 && mcus <= 8192, "rf_jpeg_entropy: bad geometry (%d MCU rows of %d)", mcu_rows, mcus);
    const int bpm = subsampling == 420 ? 6 : 3;
    RF_CHECK(slot_stride >= (long long)RF_JPEG_SLOT((long long)mcus * bpm), "rf_jpeg_entropy: slot stride %lld < the worst case %lld", (long long)slot_stride,
             (long long)RF_JPEG_SLOT((long long)mcus * bpm));
    hipLaunchKernelGGL(jpg::jpeg_entropy_kernel, dim3((unsigned)mcu_rows, (unsigned)B), dim3(jpg::ET), 0, (hipStream_t)stream, coef, mcu_rows, mcus * bpm, bpm, huff,
                       (uint8_t*)slots_u8, (long long)slot_stride, seg_bytes);
    RF_LAUNCH_CHECK("rf_jpeg_entropy");
    return 0;
}

extern "C" int rf_jpeg_pack(const void* slots_u8, int64_t slot_stride, const int* seg_bytes, int B, int mcu_rows, void* out_u8, int64_t out_stride, int* lengths,
                            void* stream) {
    RF_CHECK(slots_u8 && seg_bytes && out_u8 && lengths && B > 0 && B <= 65535 && mcu_rows >= 1 && mcu_rows <= 8192, "rf_jpeg_pack: bad arguments (B=%d, %d MCU rows)", B,
             mcu_rows);
    RF_CHECK(slot_stride > 0 && out_stride >= (int64_t)mcu_rows * (slot_stride + 2) && out_stride < (1ll << 31),
             "rf_jpeg_pack: out stride %lld < %d full slots and their markers (or above 2^31)", (long long)out_stride, mcu_rows);
    hipLaunchKernelGGL(jpg::jpeg_pack_kernel, dim3((unsigned)mcu_rows, (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)slots_u8, (long long)slot_stride,
                       seg_bytes, mcu_rows, (uint8_t*)out_u8, (long long)out_stride, lengths);
    RF_LAUNCH_CHECK("rf_jpeg_pack");
    return 0;
}
