// The block-parallel inflate plan of the PNG decoder ("blocks"), compiled on BOTH sides like png_inflate.h: by hipcc into csrc/pngdec.hip and
// by a plain host compiler into tests/pngblocks_host_main.cpp, which runs the five stages over good and damaged streams under sanitizers.
//   search    dyn_header_at(src, bit) for every bit offset: the offsets at which inflate_blocks would accept a dynamic block header.  They
//             are the candidates; the bit behind the zlib header (FIRST_BIT) is candidate 0 whatever stands there.
//   count     walk_blocks from every candidate with a CountSink: whole blocks up to the next block boundary that is a candidate.
//   chain     blocks_chain_accept: from candidate 0 along the end bits; gives every chunk on the chain its output offset.
//   decode    walk_blocks again for the chunks on the chain, with a marker sink: 16-bit symbols, a byte or 256 + j = "byte j of the WINDOW
//             bytes in front of this chunk's first byte".
//   resolve   chunk by chunk in chain order: resolve_sym, the Adler-32 from per-chunk partials (adler_push), the trailer.
// The plan only accepts a file: whatever it does not accept is decoded by the serial plan, which also sets the error code.
// Every read is checked against size(); every loop states its bound; a failure is a code or a refusal, never undefined behaviour.
#pragma once
#include "png_inflate.h"

namespace rf {
namespace pnginf {

constexpr uint32_t FIRST_BIT = 16;                  // behind CMF and FLG
constexpr uint32_t BLK_MAX_STREAM = 1u << 28;       // eligible streams are shorter: bit offsets stay below 2^31

// What the count stage leaves per candidate slot (8 int32 words).
struct Chunk {
    uint32_t start;          // the bit of the block header's BFINAL (search); below FIRST_BIT: the slot is empty
    uint32_t end;            // the bit behind the chunk's last block
    uint32_t count;          // bytes produced
    int32_t flags;           // 1: usable (no error, ended on a candidate boundary or on the final block); 2: ended on the final block;
                             // 4: the decode stage reproduced end and count
    uint32_t off;            // (chain) the offset of its first byte in the file's output
    int32_t k;               // (chain) 1 + its place in the chain, 0 off the chain
    uint32_t adler;          // spare
    int32_t pad;
};

struct WalkResult {
    uint32_t end;            // the bit behind the last whole block
    uint32_t count;
    int status;              // OK or the error that stopped the walk
    int final;               // the last whole block carried BFINAL
};

// No storage: counts bytes, accepts every distance a deflate stream can code.
struct CountSink {
    uint32_t capv, pos;
    RF_HD uint32_t cap() const { return capv; }
    RF_HD uint32_t produced() const { return pos; }
    RF_HD bool literal(uint8_t) {
        if (pos >= capv) return false;
        ++pos;
        return true;
    }
    RF_HD int match(int len, int dist) {
        if (dist > WINDOW) return E_DISTANCE;
        if ((uint32_t)len > capv - pos) return E_TOO_LONG;
        pos += (uint32_t)len;
        return OK;
    }
    template <class Src> RF_HD void copy(const Src&, uint32_t, uint32_t len) { pos += len; }          // the caller checked len <= cap() - produced()
    RF_HD uint32_t finish() { return 0; }
};

// One 16-bit symbol per output byte, stored serially (the host program's; the device has a wave-parallel one of the same meaning).
// A match that reaches in front of the chunk's first byte yields markers; a match that copies markers copies them unchanged.
struct MarkerSink {
    uint16_t* sym;
    uint32_t capv, pos;
    RF_HD uint32_t cap() const { return capv; }
    RF_HD uint32_t produced() const { return pos; }
    RF_HD bool literal(uint8_t v) {
        if (pos >= capv) return false;
        sym[pos++] = v;
        return true;
    }
    RF_HD int match(int len, int dist) {
        if (dist > WINDOW) return E_DISTANCE;
        if ((uint32_t)len > capv - pos) return E_TOO_LONG;
        for (int i = 0; i < len; ++i, ++pos)          // <= 258 iterations
            sym[pos] = (uint32_t)dist > pos ? (uint16_t)(256 + WINDOW + (int)pos - dist) : sym[pos - (uint32_t)dist];
        return OK;
    }
    template <class Src> RF_HD void copy(const Src& src, uint32_t p, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) sym[pos++] = (uint16_t)src.byte(p + i);
    }
    RF_HD uint32_t finish() { return 0; }
};

// rc of huff_build for a code whose Kraft sum (in units of 2^-15) is `kraft` and whose longest code has `mx` bits, as inflate_blocks judges
// it for the literal/length and the distance code: complete, no code at all, or a single 1-bit code.
RF_HD bool kraft_accepted(uint32_t kraft, int mx) { return kraft <= 32768u && (kraft == 32768u || mx <= 1); }

// A necessary condition of dyn_header_at from the first 74 bits alone, without a reader and without a branch per length: BTYPE = 10, HLIT
// and HDIST in range, and the Kraft sum of the code-length code's lengths exactly 1.  It is what nearly every bit offset of the search stage
// ends on.  Within 12 bytes of the stream's end it says true and leaves truncation to the full test.
template <class Src> RF_HD bool dyn_header_maybe(const Src& src, uint32_t bitpos) {
    const uint32_t p = bitpos >> 3, sh = bitpos & 7u;
    if (src.size() < 12u || p > src.size() - 12u) return true;
    const uint32_t w0 = src.word(p), w1 = src.word(p + 4), w2 = src.word(p + 8);          // stream bits 8 p .. 8 p + 95: 89 or more from bitpos
    const uint64_t lo = (((uint64_t)w1 << 32 | w0) >> sh) | (sh ? (uint64_t)w2 << (64u - sh) : 0ull);          // bits 0 .. 63 from bitpos
    const uint32_t hi = w2 >> sh;                                                                             // bits 64 .. 88 or more
    const uint32_t head = (uint32_t)lo;
    if (((head >> 1) & 3u) != 2u || ((head >> 3) & 31u) > 29u || ((head >> 8) & 31u) > 29u) return false;
    const uint32_t ncode = ((head >> 13) & 15u) + 4u;
    const uint64_t x = ((lo >> 17) | ((uint64_t)hi << 47)) & ((1ull << (3u * ncode)) - 1ull);          // 3 ncode <= 57 bits: the lengths, 0 beyond
    const uint32_t xa = (uint32_t)x & 0x3fffffffu, xb = (uint32_t)(x >> 30);          // lengths 0 .. 9 and 10 .. 18
    uint32_t kraft = 0;          // in units of 2^-7; a length 0 adds nothing
    for (int i = 0; i < 10; ++i) kraft += (0x80u >> ((xa >> (3 * i)) & 7u)) & 0x7fu;
    for (int i = 0; i < 9; ++i) kraft += (0x80u >> ((xb >> (3 * i)) & 7u)) & 0x7fu;
    return kraft == 128u;
}

// True exactly when inflate_blocks would accept a dynamic block header whose BFINAL bit is bit `bitpos` of src: the checks of its type == 2
// branch up to and including the two huff_build verdicts and lens[256] != 0.  No tables: the code-length code is decoded canonically from
// its 19 lengths (3 bits each in one word), the two codes are judged by their Kraft sums.  One lane can run it.
template <class Src> RF_HD bool dyn_header_at(const Src& src, uint32_t bitpos) {
    if (!dyn_header_maybe(src, bitpos)) return false;
    BitReader<Src> br(src, 0);
    if (!br.seek_bit(bitpos) || !br.need(3)) return false;
    if ((br.take(3) >> 1) != 2u) return false;          // BFINAL either way, BTYPE = 10
    if (!br.need(14)) return false;
    const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    uint64_t cl = 0;             // length of code-length symbol s in bits 3 s .. 3 s + 2
    uint64_t cnts = 0;           // codes of length l in bits 5 l .. 5 l + 4 (at most 19)
    uint32_t kraft = 0;          // in units of 2^-7
    for (int i = 0; i < ncode; ++i) {          // <= 19 iterations
        if (!br.need(3)) return false;
        const uint32_t v = br.take(3);
        cl |= (uint64_t)v << (3 * cl_order(i));
        if (v) {
            cnts += 1ull << (5 * v);
            kraft += 128u >> v;
            if (kraft > 128u) return false;          // (early: the sum only grows)
        }
    }
    if (kraft != 128u) return false;          // huff_build != 0; or no code at all, on which the first huff_decode fails
    uint32_t klit = 0, kdist = 0;
    int mxlit = 0, mxdist = 0, idx = 0, last = 0;
    bool eob = false;
    while (idx < nlen + ndist) {          // every iteration consumes at least one bit or leaves
        br.refill();
        const uint32_t bits = (uint32_t)br.hold;
        int code = 0, first = 0, len = 1;
        for (; len <= 7; ++len) {          // the canonical walk of huff_decode
            code |= (int)((bits >> (len - 1)) & 1u);
            const int cnt = (int)((cnts >> (5 * len)) & 31u);
            if (code - cnt < first) break;
            first += cnt;
            first <<= 1;
            code <<= 1;
        }
        if (len > 7 || len > br.nbits) return false;
        br.take(len);
        int rank = code - first, s = 0;
        for (; s < 19; ++s) {          // the rank-th symbol of that length, in symbol order as huff_build lists them
            if ((int)((cl >> (3 * s)) & 7u) == len && rank-- == 0) break;
        }
        if (s >= 19) return false;          // (not reached: the code is complete)
        int rep = 1, val = s;
        if (s == 16) {
            if (idx == 0 || !br.need(2)) return false;
            val = last;
            rep = 3 + (int)br.take(2);
        } else if (s == 17) {
            if (!br.need(3)) return false;
            val = 0;
            rep = 3 + (int)br.take(3);
        } else if (s == 18) {
            if (!br.need(7)) return false;
            val = 0;
            rep = 11 + (int)br.take(7);
        }
        if (idx + rep > nlen + ndist) return false;
        if (val) {
            const int nl = idx >= nlen ? 0 : (idx + rep > nlen ? nlen - idx : rep), nd = rep - nl;
            klit += (uint32_t)nl << (15 - val);          // <= 286 * 2^14
            kdist += (uint32_t)nd << (15 - val);
            if (nl && val > mxlit) mxlit = val;
            if (nd && val > mxdist) mxdist = val;
            if (idx <= 256 && 256 < idx + rep) eob = true;
            // over-subscribed for good: the verdict of kraft_accepted below, taken early.  On bits that are no header the lengths are
            // arbitrary and this ends the walk within a few symbols, which is what keeps the search stage short.
            if (klit > 32768u || kdist > 32768u) return false;
        }
        idx += rep;
        last = val;
    }
    return eob && kraft_accepted(klit, mxlit) && kraft_accepted(kdist, mxdist);
}

// Whole blocks of any type from bit `start`.  Stops behind a block whose end is a boundary stop(bit) names (a candidate), behind the final
// block, on an error, or when the output passes the sink's cap (E_TOO_LONG).  Bound: every block consumes at least its 3 header bits.
template <class Src, class Sink, class W, class Stop>
RF_HD void walk_blocks(Src src, uint32_t start, Sink& sink, Tables* t, const Stop& stop, WalkResult* out) {
    BitReader<Src> br(src, 0);
    int rc = br.seek_bit(start) ? OK : E_TRUNCATED, fin = 0;
    uint32_t end = start;
    while (rc == OK) {
        int piece_end;
        rc = inflate_block<Src, Sink, W>(br, sink, t, true, &fin, &piece_end);
        if (rc != OK) break;
        end = br.bitpos();
        if (fin || stop(end)) break;
    }
    out->end = end;
    out->count = sink.produced();
    out->status = rc;
    out->final = rc == OK && fin;
}

// The lookup from a candidate's bit to its slot: open addressing over `tsize` words, 0 = empty, else 1 + the slot's index among the file's.
RF_HD uint32_t blk_hash(uint32_t bit, uint32_t tsize) { return ((bit * 2654435761u) >> 7) % tsize; }
RF_HD int blk_lookup(const Chunk* ch, const int32_t* hash, uint32_t tsize, uint32_t bit) {
    uint32_t h = blk_hash(bit, tsize);
    for (uint32_t i = 0; i < tsize; ++i) {          // <= tsize probes
        const int32_t e = hash[h];
        if (e == 0) return -1;
        if (ch[e - 1].start == bit) return e - 1;
        h = h + 1 == tsize ? 0 : h + 1;
    }
    return -1;
}

RF_HD void adler_push(uint64_t* s1, uint64_t* s2, uint32_t count, uint32_t a, uint32_t b) {          // as chain_accept combines its pieces
    *s2 = (*s2 + (uint64_t)count % ADLER_MOD * *s1 + b) % ADLER_MOD;
    *s1 = (*s1 + a) % ADLER_MOD;
}

// Walks a file's chunks from candidate 0 (slot 0 of ch) along their end bits; n = the filled slots, hash / tsize the lookup over them.
// Accepts (returns the chain's length, >= 2) only if every chunk on the chain is usable, every end bit is a candidate, the last chunk ended
// on the final block, the byte total is `expect` and the trailer can be read (*want).  It gives every chain chunk its output offset, the
// exclusive prefix sum, and its place, and lists the slots in chain order.  Otherwise 0.  At most n iterations: the start bits only grow.
template <class Src> RF_HD int blocks_chain_accept(const Src& src, Chunk* ch, int n, const int32_t* hash, uint32_t tsize, int32_t* order, uint32_t expect,
                                                   uint32_t* want) {
    if (n < 2 || zlib_header(src) != OK || ch[0].start != FIRST_BIT) return 0;
    uint64_t total = 0;
    int j = 0, k = 0;
    for (;;) {
        Chunk& c = ch[j];
        if (!(c.flags & 1) || c.end <= c.start || k >= n) return 0;
        c.off = (uint32_t)total;
        order[k] = j;
        c.k = ++k;
        total += c.count;
        if (total > expect) return 0;
        if (c.flags & 2) {
            if (total != expect || k < 2 || read_trailer(src, (c.end + 7u) >> 3, want) != OK) return 0;
            return k;
        }
        j = blk_lookup(ch, hash, tsize, c.end);
        if (j < 0 || j >= n) return 0;
    }
}

// Byte i of a chunk at output offset `off` from its symbol; out = the file's output, resolved up to `off`.  False: the marker points in front
// of the stream's first byte (the serial plan reports E_DISTANCE there).
RF_HD bool resolve_sym(uint32_t sym, uint32_t off, const uint8_t* out, uint8_t* v) {
    if (sym < 256u) {
        *v = (uint8_t)sym;
        return true;
    }
    const uint32_t j = sym - 256u;
    if (j >= (uint32_t)WINDOW || off + j < (uint32_t)WINDOW) return false;
    *v = out[off - (uint32_t)WINDOW + j];          // < off
    return true;
}

}  // namespace pnginf
}  // namespace rf
