// The zlib / deflate decoder core of the PNG decoder (RFC 1950, RFC 1951), compiled on BOTH sides: by hipcc into reface_amd/csrc/pngdec.hip,
// where one wave runs it per stream, and by a plain host compiler into tests/pngdec_host_main.cpp, where the same code meets damaged streams
// under sanitizers before it meets them on a GPU.  It is templated on
//   Src   the compressed bytes: size(), byte(i), word(i) = bytes i .. i + 3           (every read is checked against size())
//   Sink  the output: literal(v), match(len, dist), copy(src, pos, len), produced(), cap()   (every write is checked against cap(),
//         every distance against produced())
//   W     the execution policy: leader() says who stores into the shared tables, sync() orders those stores before the reads of the others
//         (on the device all 64 lanes run this code on identical values, so its control flow is wave-uniform; lane 0 is the leader and
//         sync() is the workgroup barrier), note_*() are the coverage counters of the host program (empty on the device).
// A failure is an error code, never undefined behaviour.  Every loop below states its bound.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_HD __host__ __device__ __forceinline__
#else
#define RF_HD inline
#endif

namespace rf {
namespace pnginf {

enum : int {
    OK = 0,
    E_TRUNCATED = 1,         // the stream ends inside a header, a block or the trailer
    E_ZHEADER = 2,           // CM != 8, window > 32 KiB, FCHECK wrong, or a preset dictionary
    E_BLOCK_TYPE = 3,        // BTYPE = 11
    E_STORED_LEN = 4,        // LEN != ~NLEN
    E_CODE_LENGTHS = 5,      // over-subscribed or (where zlib refuses it) incomplete code, bad repeat, too many symbols, no end-of-block code
    E_BAD_CODE = 6,          // a bit pattern that is no code, or a symbol that is none (length 286/287, distance 30/31)
    E_DISTANCE = 7,          // a distance beyond the bytes produced so far
    E_TOO_LONG = 8,          // more output than H * (1 + W * bpp)
    E_TOO_SHORT = 9,         // less output than that
    E_ADLER = 10,            // the Adler-32 of the output is not the trailer's
    E_FILTER = 11,           // a row's filter byte is above 4 (rf_png_unfilter_u8)
};

constexpr int WINDOW = 32768;
constexpr int FAST_BITS = 10;
constexpr uint32_t ADLER_MOD = 65521u;

// One canonical Huffman code: count[l] codes of length l, their symbols in canonical order, and a direct table over the next FAST_BITS bits
// of the stream: (symbol << 4) | length for codes of at most FAST_BITS bits, 0 where a longer code (or none) begins.
struct Huff {
    uint16_t count[16];
    uint16_t offs[16];
    uint16_t sym[288];
    uint16_t fast[1 << FAST_BITS];
};
struct Tables {
    Huff lit, dist;          // (dist also holds the code-length code while a dynamic header is read)
    uint8_t lens[320];
    int rc;
};

template <class Src> struct BitReader {
    Src src;
    uint64_t hold;           // bits above nbits are zero
    int nbits;
    uint32_t pos;            // next byte of src to load
    RF_HD BitReader(Src s, uint32_t start) : src(s), hold(0), nbits(0), pos(start) {}
    // Four bytes at a time (src.word(i) = bytes i .. i + 3, little endian) while four are left: 33 bits or more satisfy every need() below.
    // The last three bytes of a stream come one by one: at most 8 iterations, each adds 8 bits and stops above 56.  pos <= size() always.
    RF_HD void refill() {
        if (src.size() - pos >= 4) {
            if (nbits <= 32) {
                hold |= (uint64_t)src.word(pos) << nbits;
                pos += 4;
                nbits += 32;
            }
            return;
        }
        while (nbits <= 56 && pos < src.size()) {
            hold |= (uint64_t)src.byte(pos++) << nbits;
            nbits += 8;
        }
    }
    RF_HD bool need(int k) {          // k <= 32
        if (nbits < k) refill();
        return nbits >= k;
    }
    RF_HD uint32_t take(int k) {
        const uint32_t v = (uint32_t)(hold & ((1ull << k) - 1));
        hold >>= k;
        nbits -= k;
        return v;
    }
    RF_HD void align() { take(nbits & 7); }
    RF_HD uint32_t bytepos() const { return pos - (uint32_t)(nbits >> 3); }          // (after align(): the next unread byte)
    RF_HD void seek(uint32_t p) {
        hold = 0;
        nbits = 0;
        pos = p;
    }
    // The blocks plan (png_blocks.h) reads from a bit offset: bit < 2^31.  False where the offset lies behind the stream.
    RF_HD bool seek_bit(uint32_t bit) {
        const uint32_t p = bit >> 3;
        if (p > src.size()) {
            seek(src.size());
            return false;
        }
        seek(p);
        if (!need((int)(bit & 7))) return false;
        take((int)(bit & 7));
        return true;
    }
    RF_HD uint32_t bitpos() const { return 8u * pos - (uint32_t)nbits; }          // the next unread bit (pos < 2^28 on that plan)
};

RF_HD int cl_order(int i) {
    switch (i) {
        case 0: return 16;
        case 1: return 17;
        case 2: return 18;
        case 3: return 0;
        case 4: return 8;
        case 5: return 7;
        case 6: return 9;
        case 7: return 6;
        case 8: return 10;
        case 9: return 5;
        case 10: return 11;
        case 11: return 4;
        case 12: return 12;
        case 13: return 3;
        case 14: return 13;
        case 15: return 2;
        case 16: return 14;
        case 17: return 1;
        default: return 15;
    }
}

// Tables of the code with lengths lens[0 .. n), n <= 288, every length <= 15.  The leader builds; *rc (read by everybody after the sync):
// -1 over-subscribed, 0 complete (or no code at all, as zlib: every pattern is then a bad code), 1 incomplete with a single 1-bit code
// (zlib accepts it for the literal/length and the distance code), 2 incomplete otherwise.
template <class W> RF_HD int huff_build(Huff* h, const uint8_t* lens, int n, int* rc) {
    W::sync();          // the lengths were stored by the leader; the previous users of h are done
    if (W::leader()) {
        for (int l = 0; l < 16; ++l) h->count[l] = 0;
        for (int i = 0; i < n; ++i) h->count[lens[i] & 15]++;
        h->count[0] = 0;
        int left = 1, mx = 0;
        for (int l = 1; l < 16; ++l) {
            left <<= 1;
            left -= h->count[l];
            if (left < 0) break;
            if (h->count[l]) mx = l;
        }
        h->offs[1] = 0;
        for (int l = 1; l < 15; ++l) h->offs[l + 1] = (uint16_t)(h->offs[l] + h->count[l]);
        if (left >= 0) {
            for (int i = 0; i < n; ++i) {
                const int l = lens[i] & 15;
                if (l) h->sym[h->offs[l]++] = (uint16_t)i;          // offs[l] + count[l] <= n <= 288: the sum of the counts is at most n
            }
        }
        for (int i = 0; i < (1 << FAST_BITS); ++i) h->fast[i] = 0;
        if (left >= 0) {
            uint32_t code = 0;
            int idx = 0;
            for (int l = 1; l <= FAST_BITS; ++l) {
                for (int k = 0; k < (int)h->count[l]; ++k, ++idx, ++code) {
                    uint32_t rev = 0;
                    for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
                    // not over-subscribed, so code < 2^l and rev < 2^l <= 2^FAST_BITS
                    for (uint32_t j = rev; j < (1u << FAST_BITS); j += 1u << l) h->fast[j] = (uint16_t)((h->sym[idx] << 4) | l);
                }
                code <<= 1;
            }
        }
        *rc = left < 0 ? -1 : (left == 0 || mx == 0) ? 0 : (mx == 1 ? 1 : 2);
    }
    W::sync();
    return *rc;
}

// The next symbol (>= 0), or minus an error code.  At most 15 iterations.
template <class Src> RF_HD int huff_decode(const Huff* h, BitReader<Src>& br) {
    br.refill();
    const uint32_t bits = (uint32_t)br.hold;
    const uint32_t e = h->fast[bits & ((1u << FAST_BITS) - 1)];
    if (e) {
        const int l = (int)(e & 15);
        if (l > br.nbits) return -E_TRUNCATED;
        br.take(l);
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)((bits >> (len - 1)) & 1u);
        const int cnt = h->count[len];
        if (code - cnt < first) {
            if (len > br.nbits) return -E_TRUNCATED;
            br.take(len);
            return h->sym[index + (code - first)];          // index + code - first < index + cnt <= 288
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return br.nbits < 15 ? -E_TRUNCATED : -E_BAD_CODE;
}

template <class W> RF_HD void note_lengths(const uint8_t* lens, int n) {
    if (W::leader())
        for (int i = 0; i < n; ++i) W::note_code_length(lens[i]);
}

// The literal/length and distance symbols of one block, up to its end-of-block code.
// Bound: every iteration consumes at least one bit of a stream of size() bytes, or leaves with an error.
template <class Src, class Sink, class W> RF_HD int inflate_codes(BitReader<Src>& br, Sink& sink, const Tables* t) {
    for (;;) {
        int s = huff_decode(&t->lit, br);
        if (s < 0) return -s;
        if (s < 256) {
            if (!sink.literal((uint8_t)s)) return E_TOO_LONG;
            continue;
        }
        if (s == 256) return OK;
        s -= 257;
        if (s >= 29) return E_BAD_CODE;
        int len, eb;
        if (s < 8) len = 3 + s, eb = 0;
        else if (s == 28) len = 258, eb = 0;
        else eb = (s - 4) >> 2, len = 3 + ((4 + (s & 3)) << eb);
        if (!br.need(eb)) return E_TRUNCATED;
        len += (int)br.take(eb);
        const int d = huff_decode(&t->dist, br);
        if (d < 0) return -d;
        if (d >= 30) return E_BAD_CODE;
        int dist;
        if (d < 4) dist = 1 + d, eb = 0;
        else eb = (d - 2) >> 1, dist = 1 + ((2 + (d & 1)) << eb);
        if (!br.need(eb)) return E_TRUNCATED;
        dist += (int)br.take(eb);
        W::note_match(len, dist);
        const int rc = sink.match(len, dist);
        if (rc) return rc;
    }
}

// One block from the reader's position.  *fin: its BFINAL bit.  *piece_end (whole = false, a piece of the segmented plan): the block was a
// non-final stored block that is empty or that fills the sink to its cap; both end on a byte boundary with nothing pending.
template <class Src, class Sink, class W> RF_HD int inflate_block(BitReader<Src>& br, Sink& sink, Tables* t, bool whole, int* fin_out, int* piece_end) {
    *fin_out = 0;
    *piece_end = 0;
    if (!br.need(3)) return E_TRUNCATED;
    const int fin = (int)br.take(1), type = (int)br.take(2);
    W::note_block(type);
    if (type == 0) {
        br.align();
        if (!br.need(32)) return E_TRUNCATED;
        const uint32_t len = br.take(16), nlen = br.take(16);
        if ((len ^ 0xffffu) != nlen) return E_STORED_LEN;
        const uint32_t p = br.bytepos();
        if (len > br.src.size() - p) return E_TRUNCATED;          // p <= size()
        if (len > sink.cap() - sink.produced()) return E_TOO_LONG;
        sink.copy(br.src, p, len);
        br.seek(p + len);
        if (len == 0) W::note_empty_stored();
        if (!whole && !fin && (len == 0 || sink.produced() == sink.cap())) *piece_end = 1;
    } else if (type == 1) {
        W::sync();
        if (W::leader()) {
            for (int i = 0; i < 288; ++i) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
            for (int i = 288; i < 320; ++i) t->lens[i] = 5;
        }
        huff_build<W>(&t->lit, t->lens, 288, &t->rc);
        huff_build<W>(&t->dist, t->lens + 288, 32, &t->rc);
        const int rc = inflate_codes<Src, Sink, W>(br, sink, t);
        if (rc) return rc;
    } else if (type == 2) {
        if (!br.need(14)) return E_TRUNCATED;
        const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
        if (nlen > 286 || ndist > 30) return E_CODE_LENGTHS;
        W::sync();
        if (W::leader())
            for (int i = 0; i < 19; ++i) t->lens[i] = 0;
        for (int i = 0; i < ncode; ++i) {          // <= 19 iterations
            if (!br.need(3)) return E_TRUNCATED;
            const uint32_t v = br.take(3);
            if (W::leader()) t->lens[cl_order(i)] = (uint8_t)v;
        }
        if (huff_build<W>(&t->dist, t->lens, 19, &t->rc) != 0) return E_CODE_LENGTHS;          // zlib: the code-length code must be complete
        int idx = 0, last = 0;
        while (idx < nlen + ndist) {          // every iteration consumes at least one bit or leaves
            const int s = huff_decode(&t->dist, br);
            if (s < 0) return -s;
            if (s < 16) {
                if (W::leader()) t->lens[idx] = (uint8_t)s;
                last = s;
                ++idx;
                continue;
            }
            int rep, val = 0;
            if (s == 16) {
                if (idx == 0) return E_CODE_LENGTHS;
                if (!br.need(2)) return E_TRUNCATED;
                val = last;
                rep = 3 + (int)br.take(2);
            } else if (s == 17) {
                if (!br.need(3)) return E_TRUNCATED;
                rep = 3 + (int)br.take(3);
            } else {
                if (!br.need(7)) return E_TRUNCATED;
                rep = 11 + (int)br.take(7);
            }
            if (idx + rep > nlen + ndist) return E_CODE_LENGTHS;
            if (W::leader())
                for (int k = 0; k < rep; ++k) t->lens[idx + k] = (uint8_t)val;          // idx + rep <= 316 < 320
            idx += rep;
            last = val;
        }
        W::sync();
        if (t->lens[256] == 0) return E_CODE_LENGTHS;          // no end-of-block code
        note_lengths<W>(t->lens, nlen + ndist);
        int rc = huff_build<W>(&t->lit, t->lens, nlen, &t->rc);
        if (rc < 0 || rc == 2) return E_CODE_LENGTHS;
        rc = huff_build<W>(&t->dist, t->lens + nlen, ndist, &t->rc);
        if (rc < 0 || rc == 2) return E_CODE_LENGTHS;
        rc = inflate_codes<Src, Sink, W>(br, sink, t);
        if (rc) return rc;
    } else {
        return E_BLOCK_TYPE;
    }
    *fin_out = fin;
    return OK;
}

// Blocks from the reader's position.  whole = false also stops, with *ended = 2, behind a block that set *piece_end.  *ended = 1: the final
// block is done.  Bound: every block consumes at least its 3 header bits.
template <class Src, class Sink, class W> RF_HD int inflate_blocks(BitReader<Src>& br, Sink& sink, Tables* t, bool whole, int* ended) {
    *ended = 0;
    for (;;) {
        int fin, piece_end;
        const int rc = inflate_block<Src, Sink, W>(br, sink, t, whole, &fin, &piece_end);
        if (rc) return rc;
        if (piece_end) {
            *ended = 2;
            return OK;
        }
        if (fin) {
            *ended = 1;
            return OK;
        }
    }
}

template <class Src> RF_HD int zlib_header(const Src& src) {
    if (src.size() < 2) return E_TRUNCATED;
    const uint32_t cmf = src.byte(0), flg = src.byte(1);
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return E_ZHEADER;
    return OK;
}

template <class Src> RF_HD int read_trailer(const Src& src, uint32_t p, uint32_t* v) {
    if (p > src.size() || src.size() - p < 4) return E_TRUNCATED;
    *v = ((uint32_t)src.byte(p) << 24) | ((uint32_t)src.byte(p + 1) << 16) | ((uint32_t)src.byte(p + 2) << 8) | (uint32_t)src.byte(p + 3);
    return OK;
}

// A whole zlib stream into a sink of cap() == the expected length.  The sink's finish() completes its Adler-32 (started from A = 1, B = 0).
template <class Src, class Sink, class W> RF_HD int inflate_zlib(Src src, Sink& sink, Tables* t) {
    int rc = zlib_header(src);
    if (rc) return rc;
    BitReader<Src> br(src, 2);
    int ended;
    rc = inflate_blocks<Src, Sink, W>(br, sink, t, true, &ended);
    if (rc) return rc;
    if (sink.produced() != sink.cap()) return E_TOO_SHORT;
    br.align();
    uint32_t want;
    rc = read_trailer(src, br.bytepos(), &want);
    if (rc) return rc;
    return sink.finish() == want ? OK : E_ADLER;
}

// ---- the segmented plan.  A piece is what inflate_blocks(whole = false) decodes from one candidate start into a sink of WINDOW bytes whose
// Adler-32 partial starts from A = 0, B = 0 (A = sum of bytes, B = sum of (count - i) * byte_i: the partials rf_png_pack combines).
struct Piece {
    int32_t end;             // the offset in the stream behind the piece (the trailer's offset, for the final one)
    int32_t count;           // bytes produced
    uint32_t adler;          // A | B << 16
    int32_t flags;           // 1: usable (no error, no reference before its own start, <= WINDOW bytes); 2: ended with the final block
    int32_t k;               // its place in the accepted chain (the chain kernel's), or -1
};

template <class Src, class Sink, class W> RF_HD void inflate_piece(Src src, uint32_t start, Sink& sink, Tables* t, Piece* out) {
    BitReader<Src> br(src, start);
    int ended = 0;
    const int rc = start <= src.size() ? inflate_blocks<Src, Sink, W>(br, sink, t, false, &ended) : E_TRUNCATED;
    const uint32_t ad = sink.finish();
    br.align();
    if (W::leader()) {
        out->end = (int32_t)br.bytepos();
        out->count = (int32_t)sink.produced();
        out->adler = ad;
        out->flags = (rc == OK ? 1 : 0) | (ended == 1 ? 2 : 0);
        out->k = -1;
    }
}

// Walks a file's pieces from the stream start (cand[0] == 2, behind the zlib header) along their end offsets; cand is ascending.
// Accepts (returns the number of pieces, >= 2) only if every piece is usable, every piece but the last produced exactly WINDOW bytes, every
// end offset is a candidate start, the total is `expect` and the combined Adler-32 is the trailer's.  Otherwise 0: the serial plan decodes
// the file.  At most ncand iterations: j only grows.
template <class Src> RF_HD int chain_accept(const Src& src, const int32_t* cand, Piece* pieces, int ncand, uint32_t expect) {
    if (ncand < 2 || zlib_header(src) != OK || cand[0] != 2) return 0;
    uint64_t s1 = 1, s2 = 0, total = 0;
    int j = 0, k = 0;
    for (;;) {
        Piece& p = pieces[j];
        if (!(p.flags & 1)) return 0;
        const bool fin = (p.flags & 2) != 0;
        if (!fin && p.count != WINDOW) return 0;
        s2 = (s2 + (uint64_t)p.count * s1 + (p.adler >> 16)) % ADLER_MOD;
        s1 = (s1 + (p.adler & 0xffffu)) % ADLER_MOD;
        total += (uint64_t)p.count;
        if (total > expect) return 0;
        p.k = k++;
        if (fin) {
            uint32_t want;
            if (total != expect || k < 2 || read_trailer(src, (uint32_t)p.end, &want) != OK) return 0;
            return want == (uint32_t)((s2 << 16) | s1) ? k : 0;
        }
        const int32_t next = p.end;
        if (next <= cand[j]) return 0;          // (a piece consumes at least its 3 header bits)
        while (j < ncand && cand[j] < next) ++j;
        if (j >= ncand || cand[j] != next) return 0;
    }
}

RF_HD int paeth(int a, int b, int c) {          // as the encoder's
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
RF_HD int png_predict(int type, int a, int b, int c) { return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c); }

}  // namespace pnginf
}  // namespace rf
