// The self-synchronising parallel plan of the baseline-JPEG entropy decoder ("selfsync"), compiled on BOTH sides like csrc/jpeg_decode.h: by
// hipcc into reface_amd/csrc/jpegdec.hip and by a host compiler into tests/jpegsync_host_main.cpp, which runs it under sanitizers first.
//
// The scan of a file without DRI is cut into sub-sequences of L bytes at the byte offsets B_i = i * L of the STUFFED scan; lane i owns
// sub-sequence i.  A decoder state at a symbol boundary is (p, c, z): p the bit position in the stuffed scan, c the block's index within
// the MCU (it selects the tables), z the next zigzag index (0: a DC symbol is next), packed into one 64-bit word.  F_i(s) = ss_eval decodes
// whole symbols from s until p >= 8 * B_{i+1} or the data ends and returns the state there and the blocks it completed.  F is total: what
// the serial decoder calls an error is resolved by a fixed rule (a bad code consumes one bit, a DC category keeps its low 4 bits, an index
// past 63 ends the block).  s[0] = (0, 0, 0) is true, s[i] starts as the guess (8 * B_i, 0, 0), and s[i + 1] <- F_i(s[i]) is repeated
// until nothing changes.  Given s[0] the fixed point is unique -- s[1] is forced, then s[2], ... -- so it holds the serial decoder's own
// states whether or not the bitstream ever synchronised; synchronisation only decides how few passes that takes.  ss_write then decodes
// every sub-sequence once more from its true state, with the serial decoder's checks in the serial decoder's order.
// Every loop states its bound, every read is below the scan's end, every write inside the file's block range.
#pragma once
#include "jpeg_decode.h"

namespace rf {
namespace jpgdec {

// descriptor fields 19 .. 22 (0 in a file that does not take this plan)
enum { D_SS_BEGIN = 19,          // the file's first slot in the state / count arrays
       D_SS_COUNT,               // its sub-sequences, ceil(scan_len / L) >= 2; 0: the file keeps the plan it had
       D_SS_BYTES,               // L
       D_SS_WG_BEGIN };          // its first workgroup: ceil(count / SS_LANES) of them
constexpr int SS_LANES = 64;                  // sub-sequences per workgroup
constexpr int SS_MIN_BYTES = 16;              // a symbol with its amplitude is <= 32 bits, <= 8 bytes stuffed: it never spans a sub-sequence
constexpr int SS_MAX_BYTES = 1 << 16;
constexpr int SS_MAX_LAUNCHES = 16;
constexpr int PLAN_SELFSYNC = 2;              // status word 1: the plan in bits 0 .. 1,
constexpr int ST_FALLBACK = 4;                // this flag (the serial lane decoded the file after all),
constexpr int ST_LAUNCHES_SHIFT = 8;          // and the sync launches that were needed in bits 8 .. 15
constexpr uint64_t SS_NEVER = ~0ull;          // no state: z = 127 does not occur

RF_JD uint64_t ss_pack(uint64_t p, int c, int z) { return p | (uint64_t)c << 40 | (uint64_t)z << 44; }
RF_JD uint64_t ss_pos(uint64_t s) { return s & ((1ull << 40) - 1); }

// The guess of sub-sequence i's state (i * L < len): its first byte, or the byte behind where the cut falls between FF and its stuffed 00.
RF_JD uint64_t ss_guess(const uint8_t* scan, uint32_t len, uint64_t at) {
    if (at > 0 && at < len && scan[at - 1] == 0xFFu && scan[at] == 0u) ++at;
    return ss_pack(8 * at, 0, 0);
}

// Bits that know where they are: the same window as Bits (acc / nbits / fake, zeros fed behind the data's end, a marker or a last FF ends
// the data), started at any bit of the stuffed scan.  `rd` is the next byte to load; it runs on over the virtual zero bytes behind the end,
// one per 8 fake bits.  `ff` remembers, youngest byte in bit 0, which loaded bytes had a stuffed 00 behind them: position() subtracts those
// that lie behind the next unconsumed bit.
struct SBits {
    const uint8_t* p;
    uint32_t rd, end;
    uint32_t acc;
    int nbits, fake;
    uint32_t ff;
    uint64_t chunk;
    uint32_t cbase;
    RF_JD SBits(const uint8_t* p_, uint32_t end_, uint64_t bitpos) : p(p_), rd((uint32_t)(bitpos >> 3)), end(end_), acc(0), nbits(0), fake(0), ff(0), chunk(0) {
        cbase = rd - 8u;
        fill();
        take((int)(bitpos & 7u));
    }
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
            uint32_t b = 0, stuffed = 0;
            if (rd < end) {
                b = byte(rd);
                if (b == 0xFFu) {
                    if (rd + 1 < end && byte(rd + 1) == 0u) {
                        stuffed = 1;
                    } else {          // a marker, or FF as the last byte: the data ends in front of it
                        end = rd;
                        b = 0;
                        fake += 8;
                    }
                }
            } else {
                fake += 8;
            }
            rd += 1 + stuffed;
            ff = (ff << 1) | stuffed;
            acc |= b << (24 - nbits);
            nbits += 8;
        }
    }
    RF_JD bool take(int n) {          // 0 <= n <= 16 <= nbits
        acc = n ? acc << n : acc;
        nbits -= n;
        return nbits >= fake;
    }
    RF_JD bool truncated() const { return nbits < fake; }
    // the next unconsumed bit's place in the stuffed scan (never a bit of a stuffed 00); meaningful while !truncated()
    RF_JD uint64_t position() const {
        const int held = (nbits + 7) >> 3;          // the youngest bytes that hold the unconsumed bits: 0 .. 4
        return 8ull * rd - (uint64_t)nbits - 8ull * (uint64_t)__builtin_popcount(ff & ((1u << held) - 1u));
    }
};

// what F and the write pass know of a file
struct SsFile {
    const uint8_t* scan;
    uint32_t len;                 // bytes of the stuffed scan
    const HuffTab* huff;          // DC 0..3, AC 0..3
    uint32_t td, ta;
    int ny, bpm;                  // luma blocks per MCU, blocks per MCU
    uint32_t cap;                 // symbol steps one evaluation may take: 8 L + 32
    RF_JD const HuffTab* dc(int c) const { return huff + ((td >> (8 * (c < ny ? 0 : c - ny + 1))) & 3u); }
    RF_JD const HuffTab* ac(int c) const { return huff + 4 + ((ta >> (8 * (c < ny ? 0 : c - ny + 1))) & 3u); }
};
RF_JD SsFile ss_file(const uint8_t* scan, const long long* d, const HuffTab* huff) {
    SsFile f;
    f.scan = scan;
    f.len = (uint32_t)d[D_SCAN_LEN];
    f.huff = huff;
    f.td = (uint32_t)d[D_TD];
    f.ta = (uint32_t)d[D_TA];
    f.ny = (int)d[D_NCOMP] == 3 ? (int)(d[D_HS] * d[D_VS]) : 1;
    f.bpm = (int)d[D_NCOMP] == 3 ? f.ny + 2 : 1;
    f.cap = 8u * (uint32_t)d[D_SS_BYTES] + 32u;
    return f;
}

// F: from state s to the first symbol boundary at or behind `bound` (bits), or to the data's end, where the state is (8 * len, 0, 0) and
// every later sub-sequence has nothing to do.  *blocks = the blocks completed on the way.
// Bound: every step consumes at least one bit, s is at most 8 L bits in front of `bound`, and f.cap = 8 L + 32 steps is the hard stop.
RF_JD uint64_t ss_eval(const SsFile& f, uint64_t s, uint64_t bound, int* blocks) {
    uint64_t p = ss_pos(s);
    int c = (int)(s >> 40) & 15, z = (int)(s >> 44) & 127, nb = 0;
    *blocks = 0;
    if (p >= bound) return s;
    if (c >= f.bpm) c = 0;
    SBits br(f.scan, f.len, p);
    int32_t v;
    for (uint32_t it = 0; it < f.cap; ++it) {
        if (z == 0) {
            const int sym = decode_symbol(br, f.dc(c));
            if (sym == -E_BAD_CODE) {
                br.take(1);
            } else if (sym >= 0) {
                receive_extend(br, sym & 15, &v);
                z = 1;
            }
        } else {
            const int rs = decode_symbol(br, f.ac(c));
            if (rs == -E_BAD_CODE) {
                br.take(1);
            } else if (rs >= 0) {
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    z = r == 15 ? z + 16 : 64;          // ZRL, EOB
                } else {
                    z += r + 1;
                    receive_extend(br, sz, &v);
                }
            }
        }
        if (br.truncated()) {
            *blocks = nb;
            return ss_pack(8ull * f.len, 0, 0);
        }
        if (z >= 64) {
            z = 0;
            c = c + 1 == f.bpm ? 0 : c + 1;
            ++nb;
        }
        p = br.position();
        if (p >= bound) break;
    }
    *blocks = nb;
    return ss_pack(p, c, z);
}

// The write pass of one sub-sequence from its TRUE state: coefficients de-zigzagged into coef[blk, 64] (zero-filled by the caller), the DC
// DIFFERENCE in slot 0, blocks from `blk` on and below `blocks`; it stops at the first symbol boundary at or behind `bound`, the last
// sub-sequence (`last`) only when the file's blocks are complete or the data has run out.  The checks are decode_block's, in its order, so
// the code is the one the serial plan gives.  Same bound as ss_eval; behind the data's end every step fails in take().
RF_JD int ss_write(const SsFile& f, uint64_t s, uint64_t bound, bool last, long long blk, long long blocks, int16_t* coef) {
    const uint64_t p = ss_pos(s);
    int c = (int)(s >> 40) & 15, z = (int)(s >> 44) & 127;
    if (blk < 0 || blk >= blocks || (!last && p >= bound)) return OK;
    if (c >= f.bpm || z > 63) return E_CAP;
    SBits br(f.scan, f.len, p);
    int32_t v;
    for (uint32_t it = 0; it < f.cap; ++it) {
        int16_t* out = coef + blk * 64;          // blk < blocks here
        if (z == 0) {
            const int sym = decode_symbol(br, f.dc(c));
            if (sym < 0) return -sym;
            if (sym > 15) return E_SYMBOL;
            if (!receive_extend(br, sym, &v)) return E_TRUNCATED;
            out[0] = (int16_t)v;
            z = 1;
        } else {
            const int rs = decode_symbol(br, f.ac(c));
            if (rs < 0) return -rs;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                z = r == 15 ? z + 16 : 64;
            } else {
                z += r;
                if (z > 63) return E_INDEX;
                if (!receive_extend(br, sz, &v)) return E_TRUNCATED;
                out[zigzag(z)] = (int16_t)v;
                ++z;
            }
        }
        if (z >= 64) {
            z = 0;
            c = c + 1 == f.bpm ? 0 : c + 1;
            if (++blk >= blocks) return OK;
        }
        if (!last && br.position() >= bound) return OK;
    }
    return E_CAP;
}

// the component of block b of a file, and the n-th block of component c in scan order (the DC prefix pass walks those)
RF_JD long long ss_block_of(long long n, int c, int ny, int bpm) { return c == 0 ? n / ny * bpm + n % ny : n * bpm + ny + c - 1; }

}  // namespace jpgdec
}  // namespace rf
