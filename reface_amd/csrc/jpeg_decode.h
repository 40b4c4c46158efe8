// The entropy-decoding core of the baseline-JPEG decoder (ITU-T T.81, sequential Huffman, 8 bits), compiled on BOTH sides: by hipcc into
// reface_amd/csrc/jpegdec.hip, where one lane runs it per restart interval, and by a plain host compiler into tests/jpegdec_host_main.cpp,
// where the same code meets damaged scans under sanitizers before it meets them on a GPU.
// A failure is an error code, never undefined behaviour: every read is checked against the interval's end, every write against the
// interval's block range, and every loop below states its bound.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_JD __host__ __device__ __forceinline__
#else
#define RF_JD inline
#endif

namespace rf {
namespace jpgdec {

enum : int {
    OK = 0,
    E_TRUNCATED = 1,         // the interval's data ran out inside a block
    E_BAD_CODE = 2,          // 16 bits that are no code of the table
    E_INDEX = 3,             // a coefficient behind a run that ends past index 63
    E_RST_COUNT = 4,         // the scan does not hold ceil(MCUs / Ri) intervals
    E_RST_ORDER = 5,         // the marker in front of an interval is not RST((k - 1) mod 8)
    E_SYMBOL = 6,            // a DC category above 15
    E_CAP = 7,               // the iteration cap or the block range was reached (cannot happen by construction; kept as the hard stop)
};

// descriptor fields (int64 each), RF_JPEGDEC_DESC per file
constexpr int DESC = 24;
enum { D_SCAN_OFF = 0, D_SCAN_LEN, D_H, D_W, D_NCOMP, D_HS, D_VS, D_RI, D_COEF_OFF, D_PLANE_OFF, D_OUTC, D_PIX_OFF, D_ROW_STRIDE, D_TAB_OFF,
       D_IVL_BEGIN, D_IVL_COUNT, D_TQ, D_TD, D_TA };

// One Huffman table as the decoder wants it: `look` over the next 8 bits, (length << 8) | symbol for codes of at most 8 bits and 0 where a
// longer code (or none) begins; for the longer ones libjpeg's maxcode / valptr walk (maxcode[l] = -1 where no code has l bits, valoff[l] =
// index of the first symbol of length l minus its code).
struct HuffTab {
    uint16_t look[256];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t vals[256];
};
static_assert(sizeof(HuffTab) == 912, "HuffTab layout");
constexpr int QUANT_BYTES = 4 * 64 * 2;                                 // 4 tables of 64 uint16, natural order
constexpr int TABLE_BYTES = QUANT_BYTES + 8 * (int)sizeof(HuffTab);      // then DC 0..3, AC 0..3

struct Geometry {
    int mcus_x, mcus_y, bpm;          // MCUs per row, MCU rows, blocks per MCU
    RF_JD long long mcus() const { return (long long)mcus_x * mcus_y; }
    RF_JD long long blocks() const { return mcus() * bpm; }
    RF_JD long long intervals(long long ri) const { return ri > 0 ? (mcus() + ri - 1) / ri : 1; }
};
RF_JD Geometry geometry(int H, int W, int ncomp, int hs, int vs) {
    Geometry g;
    g.mcus_x = (W + 8 * hs - 1) / (8 * hs);
    g.mcus_y = (H + 8 * vs - 1) / (8 * vs);
    g.bpm = ncomp == 1 ? 1 : hs * vs + 2;
    return g;
}

RF_JD int zigzag(int k) {
    constexpr uint8_t Z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return Z[k & 63];
}

// The bits of one interval, most significant first, 00 behind FF removed.  Behind the interval's last byte (or at a marker) zeros are fed and
// counted in `fake`: the real bits left are nbits - fake, and taking more than those is E_TRUNCATED.  Bytes come from an 8-byte chunk that
// is reloaded when the position leaves it.
struct Bits {
    const uint8_t* p;
    uint32_t pos, end;          // pos <= end always
    uint32_t acc;               // the next nbits bits, left aligned
    int nbits, fake;
    uint64_t chunk;
    uint32_t cbase;
    RF_JD Bits(const uint8_t* p_, uint32_t begin, uint32_t end_) : p(p_), pos(begin), end(end_), acc(0), nbits(0), fake(0), chunk(0), cbase(begin - 8u) {}
    RF_JD uint32_t byte(uint32_t i) {          // callers check i < end
        if (i - cbase >= 8u) {
            cbase = i;
            if (end - i >= 8u) {
                __builtin_memcpy(&chunk, p + i, 8);
            } else {
                chunk = 0;
                for (uint32_t j = 0; j < end - i; ++j) chunk |= (uint64_t)p[i + j] << (8 * j);          // <= 7 iterations
            }
        }
        return (uint32_t)(chunk >> (8 * (i - cbase))) & 255u;
    }
    RF_JD void fill() {          // <= 4 iterations: each adds 8 bits; afterwards nbits >= 25
        while (nbits <= 24) {
            uint32_t b = 0;
            if (pos < end) {
                b = byte(pos++);
                if (b == 0xFFu) {
                    if (pos < end && byte(pos) == 0u) {
                        ++pos;
                    } else {          // a marker, or FF as the last byte: the data ends here
                        pos = end;
                        b = 0;
                        fake += 8;
                    }
                }
            } else {
                fake += 8;
            }
            acc |= b << (24 - nbits);
            nbits += 8;
        }
    }
    RF_JD bool take(int n) {          // 0 <= n <= 16 <= nbits
        acc = n ? acc << n : acc;
        nbits -= n;
        return nbits >= fake;
    }
};

// -> the symbol (0 .. 255), or -E_BAD_CODE / -E_TRUNCATED.  Consumes at least one bit, none where the code is bad.  `Reader` is Bits, or the
// reader of csrc/jpeg_sync.h that knows its place in the stuffed scan: fill() leaves at least 25 bits in `acc`, take(n) says whether they were real.
template <class Reader>
RF_JD int decode_symbol(Reader& br, const HuffTab* t) {
    br.fill();
    const uint32_t lk = t->look[br.acc >> 24];
    int len = (int)(lk >> 8), sym = (int)(lk & 255u);
    if (len < 1 || len > 8) {
        len = 0;
        for (int l = 9; l <= 16; ++l) {          // 8 iterations
            const int32_t code = (int32_t)(br.acc >> (32 - l));
            if (code <= t->maxcode[l]) {
                sym = t->vals[(uint32_t)(t->valoff[l] + code) & 255u];
                len = l;
                break;
            }
        }
        if (!len) return -E_BAD_CODE;
    }
    return br.take(len) ? sym : -E_TRUNCATED;
}

// s bits as a signed amplitude (T.81 F.2.2.1 EXTEND); 0 <= s <= 15.  -> false when the data ran out
template <class Reader>
RF_JD bool receive_extend(Reader& br, int s, int32_t* v) {
    br.fill();
    const int32_t raw = s ? (int32_t)(br.acc >> (32 - s)) : 0;
    *v = s && raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
    return br.take(s);
}

// One 8 x 8 block into out[64] (natural order; zero on entry).  The AC loop advances k by at least 1 per iteration: <= 63 iterations.
RF_JD int decode_block(Bits& br, const HuffTab* dc, const HuffTab* ac, uint32_t* pred, int16_t* out, uint32_t* iters) {
    int s = decode_symbol(br, dc);
    if (s < 0) return -s;
    if (s > 15) return E_SYMBOL;
    int32_t v;
    if (!receive_extend(br, s, &v)) return E_TRUNCATED;
    *pred += (uint32_t)v;
    out[0] = (int16_t)*pred;
    int k = 1;
    while (k < 64) {
        ++*iters;
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return -rs;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;          // EOB
            k += 16;                     // ZRL
            continue;
        }
        k += r;
        if (k > 63) return E_INDEX;
        if (!receive_extend(br, s, &v)) return E_TRUNCATED;
        out[zigzag(k)] = (int16_t)v;
        ++k;
    }
    return OK;
}

// What every lane checks before it decodes interval k of a file: the count, and the marker in front of it.  starts[k] is the offset of
// interval k's first byte in the scan (the entry point has checked 2 <= starts[k] <= scan_len for k > 0 and that they ascend).
RF_JD int check_interval(const uint8_t* scan, const int32_t* starts, long long k, long long found, long long expected) {
    if (found != expected) return E_RST_COUNT;
    if (k > 0) {
        const uint32_t s = (uint32_t)starts[k];
        if (scan[s - 2] != 0xFFu || scan[s - 1] != (uint8_t)(0xD0u + (uint32_t)((k - 1) & 7))) return E_RST_ORDER;
    }
    return OK;
}

// Interval k of a file: MCUs [k * ri, min((k + 1) * ri, mcus)) (all of them where ri == 0), bytes [begin, end) of the scan, into the file's
// coefficients `coef` ([blocks, 64] int16, zero-filled by the caller).  d = the file's descriptor, tables = its table block.
// Bound: the MCU / component / block loops are counted; every block costs <= 64 symbol iterations, `iters` is the hard cap on top.
RF_JD int decode_interval(const uint8_t* scan, uint32_t begin, uint32_t end, const long long* d, const uint8_t* tables, long long k, int16_t* coef) {
    const int ncomp = (int)d[D_NCOMP], hs = (int)d[D_HS], vs = (int)d[D_VS];
    const Geometry g = geometry((int)d[D_H], (int)d[D_W], ncomp, hs, vs);
    const long long ri = d[D_RI], mcus = g.mcus();
    const long long m0 = ri > 0 ? k * ri : 0, m1 = ri > 0 && m0 + ri < mcus ? m0 + ri : mcus;
    if (m0 >= m1) return E_RST_COUNT;
    const HuffTab* huff = (const HuffTab*)(tables + QUANT_BYTES);
    const uint32_t td = (uint32_t)d[D_TD], ta = (uint32_t)d[D_TA];
    long long blk = m0 * g.bpm;
    const long long blk_end = m1 * g.bpm;
    const uint32_t cap = (uint32_t)((blk_end - blk) * 64 < 0x7FFFFFFFll ? (blk_end - blk) * 64 : 0x7FFFFFFFll);
    uint32_t iters = 0, pred[3] = {0u, 0u, 0u};
    Bits br(scan, begin, end);
    for (long long m = m0; m < m1; ++m) {
        for (int c = 0; c < ncomp; ++c) {
            const int nb = c == 0 && ncomp == 3 ? hs * vs : 1;
            const HuffTab* dc = huff + ((td >> (8 * c)) & 3u);
            const HuffTab* ac = huff + 4 + ((ta >> (8 * c)) & 3u);
            for (int b = 0; b < nb; ++b) {
                if (blk >= blk_end || iters > cap) return E_CAP;
                const int rc = decode_block(br, dc, ac, &pred[c], coef + blk * 64, &iters);
                if (rc != OK) return rc;
                ++blk;
            }
        }
    }
    return OK;
}

}  // namespace jpgdec
}  // namespace rf
