"""numpy / Python restatement of the three stages of reface_amd/csrc/pngenc.hip (filter, segment deflate, pack), with the same tie-breaks:
the expected bytes of every device test in tests/test_pngenc_gpu.py.  tests/test_pngenc_cpu.py holds this file to zlib and PIL.

Format: the filtered stream is cut into segments of 32768 bytes; nothing refers back across a segment start.  A segment
is tokenised like zlib's Z_RLE (distance 1 only), coded with its own Huffman code in ONE dynamic block whose header has a fixed form, and
ends -- unless it is the last -- with an empty stored block, so segments concatenate at byte granularity.  A segment that does not get
smaller this way is one stored block.
"""
import struct
import zlib

import numpy as np

SEG = 32768
ADLER_MOD = 65521
HEADER_BITS = 17 + 19 * 3 + 287 * 4          # BFINAL/BTYPE/HLIT/HDIST/HCLEN, the code-length code, 286 + 1 code lengths of 4 bits
PNG_SIG = b"\x89PNG\r\n\x1a\n"
COLOR_TYPE = {1: 0, 3: 2, 4: 6}

# RFC 1951 3.2.5: length symbol 257 + k covers LEN_BASE[k] .. with LEN_EXTRA[k] extra bits
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_LEN_SYM = np.zeros(259, dtype=np.int64)
for _k, _b in enumerate(LEN_BASE):
    _LEN_SYM[_b:] = _k
LEN_BASE_A, LEN_EXTRA_A = np.array(LEN_BASE, dtype=np.int64), np.array(LEN_EXTRA, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ stage 1: filter
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_candidates(row, up, bpp):
    """The five filtered versions [5, n] (uint8) of one row (int arrays of n bytes; `up` is zeros for the first row)."""
    x = row.astype(np.int64)
    b = up.astype(np.int64)
    a = np.concatenate([np.zeros(bpp, np.int64), x[:-bpp]]) if len(x) > bpp else np.zeros_like(x)
    if len(x) > bpp:
        c = np.concatenate([np.zeros(bpp, np.int64), b[:-bpp]])
    else:
        c = np.zeros_like(x)
    a, c = a[:len(x)], c[:len(x)]
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]).astype(np.uint8)


def filter_image(img):
    """uint8 [H, W, C] -> (filtered stream: H rows of 1 + W*C bytes, the filter type of every row).  Per row the filter with the smallest
    sum of |residual as a signed byte| wins; ties go to the lowest type."""
    img = np.asarray(img, dtype=np.uint8)
    H, W, C = img.shape
    rows = img.reshape(H, W * C)
    out = np.empty((H, 1 + W * C), dtype=np.uint8)
    types = np.empty(H, dtype=np.uint8)
    zero = np.zeros(W * C, dtype=np.uint8)
    for y in range(H):
        cand = filter_candidates(rows[y], rows[y - 1] if y else zero, C)
        v = cand.astype(np.int64)
        sums = np.where(v < 128, v, 256 - v).sum(axis=1)
        t = int(np.argmin(sums))          # first minimum = lowest type
        types[y] = t
        out[y, 0] = t
        out[y, 1:] = cand[t]
    return out.reshape(-1), types


def unfilter(stream, H, W, C):
    """Inverse of filter_image (the PNG decoder's reconstruction), for the CPU tests."""
    n = W * C
    s = np.asarray(stream, dtype=np.uint8).reshape(H, 1 + n)
    out = np.zeros((H, n), dtype=np.int64)
    for y in range(H):
        t, r = int(s[y, 0]), s[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(n, np.int64)
        cur = out[y]
        for i in range(n):
            a = cur[i - C] if i >= C else 0
            b = up[i]
            c = up[i - C] if i >= C else 0
            if t == 0:
                p = 0
            elif t == 1:
                p = a
            elif t == 2:
                p = b
            elif t == 3:
                p = (a + b) >> 1
            else:
                p = int(_paeth(np.int64(a), np.int64(b), np.int64(c)))
            cur[i] = (r[i] + p) & 255
    return out.astype(np.uint8).reshape(H, W, C)


# ------------------------------------------------------------------------------------------------ stage 2: segment deflate
def tokenise(seg):
    """Roles of the bytes of one segment: (is_literal, is_match_head, match_length) arrays.  Each maximal run of R equal bytes: the first byte
    is a literal; of the remaining R - 1, chunks of up to 258 are matches at distance 1 while at least 3 remain; a tail of 1 or 2 is literals."""
    d = np.frombuffer(bytes(seg), dtype=np.uint8)
    n = len(d)
    idx = np.arange(n, dtype=np.int64)
    flag = np.ones(n, dtype=bool)
    flag[1:] = d[1:] != d[:-1]
    start = np.maximum.accumulate(np.where(flag, idx, -1))
    nxt = np.where(flag, idx, n)          # end of a run = the next run start after it
    end = np.empty(n, dtype=np.int64)
    end[:-1] = np.minimum.accumulate(nxt[::-1])[::-1][1:]
    end[-1] = n
    p, R = idx - start, end - start
    q, rem = p - 1, R - 1
    k = np.where(p > 0, q // 258, 0)
    left = rem - 258 * k
    in_match = (p > 0) & (left >= 3)
    head = in_match & (q - 258 * k == 0)
    lit = ~in_match
    mlen = np.where(head, np.minimum(left, 258), 0)
    return d, lit, head, mlen


def huffman_lengths(counts, limit=15):
    """Code lengths of the symbols with non-zero count: two-queue construction over the leaves sorted by (count, symbol), internal nodes in
    creation order, the leaf taken on equal weight; while the deepest code exceeds 15 bits every non-zero count becomes (count + 1) / 2."""
    c = [int(x) for x in counts]
    while True:
        leaves = sorted((c[s], s) for s in range(len(c)) if c[s] > 0)
        m = len(leaves)
        lens = [0] * len(c)
        if m == 1:
            lens[leaves[0][1]] = 1
            return lens
        w = [x[0] for x in leaves]
        iw, parent = [], [0] * (2 * m - 1)
        i = j = 0
        for k in range(m - 1):
            tot = 0
            for _ in range(2):
                if i < m and (j >= len(iw) or w[i] <= iw[j]):
                    node, wt = i, w[i]
                    i += 1
                else:
                    node, wt = m + j, iw[j]
                    j += 1
                parent[node] = m + k
                tot += wt
            iw.append(tot)
        depth = [0] * (2 * m - 1)
        for node in range(2 * m - 3, -1, -1):          # the root is the last node made; parents are made after their children
            depth[node] = depth[parent[node]] + 1
        if max(depth[:m]) <= limit:
            for r, (_, s) in enumerate(leaves):
                lens[s] = depth[r]
            return lens
        c = [(x + 1) // 2 if x > 0 else 0 for x in c]


def canonical_codes(lens):
    """RFC 1951 3.2.2: codes of the given lengths, then bit-reversed (Huffman codes go into the stream most significant bit first)."""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return out


def _pack_bits(vals, nbits):
    """LSB-first concatenation of vals[i] (nbits[i] bits each) -> (bytes, total bits)."""
    vals, nbits = np.asarray(vals, dtype=np.uint64), np.asarray(nbits, dtype=np.int64)
    w = int(nbits.max()) if len(nbits) else 0
    k = np.arange(w, dtype=np.uint64)
    bits = ((vals[:, None] >> k[None, :]) & np.uint64(1)).astype(np.uint8)
    keep = k[None, :].astype(np.int64) < nbits[:, None]
    flat = bits[keep]
    return np.packbits(flat, bitorder="little").tobytes(), int(nbits.sum())


def deflate_segment(seg, last):
    """The bytes of one segment (<= 32768 input bytes)."""
    seg = bytes(seg)
    n = len(seg)
    assert 0 < n <= SEG
    d, lit, head, mlen = tokenise(seg)
    lsym = _LEN_SYM[mlen]
    counts = np.bincount(d[lit], minlength=286) + np.bincount(257 + lsym[head], minlength=286)
    counts[256] = 1
    lens = huffman_lengths(counts)
    codes = canonical_codes(lens)
    lens_a, codes_a = np.array(lens, dtype=np.int64), np.array(codes, dtype=np.int64)
    tok = lit | head
    sym = np.where(lit, d.astype(np.int64), 257 + lsym)[tok]
    ishead = head[tok]
    ml = mlen[tok]
    ls = lsym[tok]
    ebits = np.where(ishead, LEN_EXTRA_A[ls], 0)
    extra = np.where(ishead, ml - LEN_BASE_A[ls], 0)
    val = codes_a[sym] | (extra << lens_a[sym])          # the distance code (one bit, 0) follows a length's extra bits
    nb = lens_a[sym] + ebits + ishead.astype(np.int64)
    # the header: BFINAL, BTYPE = 10, HLIT = 29, HDIST = 0, HCLEN = 15; code-length-code lengths in the order 16 17 18 0 8 7 ...: 0 0 0 then 4 x 16
    hv = [int(last) | (2 << 1) | (29 << 3) | (0 << 8) | (15 << 13)] + [0, 0, 0] + [4] * 16
    hn = [17] + [3] * 19
    rev4 = [int(format(v, "04b")[::-1], 2) for v in range(16)]          # the code of code length v is v itself, 4 bits
    hv += [rev4[l] for l in lens] + [rev4[1]]                            # 286 literal/length lengths, then the one distance code of length 1
    hn += [4] * 287
    vals = np.concatenate([np.array(hv, dtype=np.int64), val, [codes[256]]])
    nbs = np.concatenate([np.array(hn, dtype=np.int64), nb, [lens[256]]])
    body, nbit = _pack_bits(vals, nbs)
    if last:
        dyn = body
    else:
        nbytes = (nbit + 3 + 7) // 8          # the empty stored block's 3 header bits, padded to a byte
        dyn = body.ljust(nbytes, b"\0") + b"\x00\x00\xff\xff"
    if len(dyn) >= n + 5:
        return bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + seg
    return dyn


def adler_segment(seg):
    """(A, B) of a segment for the combine identity: A = sum of bytes, B = sum of (n - i) * byte_i, both mod 65521."""
    d = np.frombuffer(bytes(seg), dtype=np.uint8).astype(np.int64)
    n = len(d)
    return int(d.sum() % ADLER_MOD), int((d * (n - np.arange(n))).sum() % ADLER_MOD)


def deflate_segments(stream):
    """-> ([segment bytes], [(A, B, n)]) of a byte stream."""
    stream = bytes(stream)
    assert len(stream) > 0
    pieces = [stream[o:o + SEG] for o in range(0, len(stream), SEG)]
    segs = [deflate_segment(p, k == len(pieces) - 1) for k, p in enumerate(pieces)]
    return segs, [adler_segment(p) + (len(p),) for p in pieces]


# ------------------------------------------------------------------------------------------------ stage 3: pack
def pack(segs, adlers):
    s1, s2 = 1, 0
    for A, B, n in adlers:
        s2 = (s2 + n * s1 + B) % ADLER_MOD
        s1 = (s1 + A) % ADLER_MOD
    return b"\x78\x01" + b"".join(segs) + struct.pack(">I", (s2 << 16) | s1)


def zlib_stream(stream):
    """The complete zlib stream of a byte stream (what the device leaves per image)."""
    return pack(*deflate_segments(stream))


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def wrap_png(zstream, H, W, C):
    """The PNG file around one zlib stream: signature, IHDR, one IDAT, IEND."""
    ihdr = struct.pack(">IIBBBBB", W, H, 8, COLOR_TYPE[C], 0, 0, 0)
    return PNG_SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", bytes(zstream)) + _chunk(b"IEND", b"")


def encode_png(img):
    img = np.asarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    return wrap_png(zlib_stream(filter_image(img)[0].tobytes()), H, W, C)


# ------------------------------------------------------------------------------------------------ shared test inputs
def fibonacci_stream():
    """One segment whose byte counts follow the Fibonacci numbers (an unlimited Huffman code is ~20 bits deep): forces the 15-bit limit loop.
    Shuffled (seeded), then equal neighbours are swapped apart, so every byte is a literal and the symbol counts are exactly these."""
    fib = [1, 2]          # with the end-of-block symbol's count of 1 the leaves are 1 1 2 3 5 ...: a single chain
    while sum(fib) + fib[-1] + fib[-2] <= SEG:
        fib.append(fib[-1] + fib[-2])
    d = np.concatenate([np.full(c, v, dtype=np.int64) for v, c in enumerate(fib)])
    rng = np.random.RandomState(5)
    rng.shuffle(d)
    n = len(d)
    d = np.concatenate([[-1], d, [-2]])          # sentinels: every position has two neighbours
    while True:
        bad = np.nonzero(d[2:n + 1] == d[1:n])[0] + 2
        if len(bad) == 0:
            break
        for i in bad:
            while d[i] == d[i - 1] or d[i] == d[i + 1]:
                j = int(rng.randint(1, n + 1))
                if abs(j - i) > 1 and d[j] not in (d[i - 1], d[i + 1]) and d[i] not in (d[j - 1], d[j + 1]):
                    d[i], d[j] = d[j], d[i]
    return d[1:n + 1].astype(np.uint8).tobytes()


def runs_stream(lengths=(1, 2, 3, 4, 258, 259, 260, 261, 262, 516, 517)):
    """Runs of exactly the given lengths, separated by distinct bytes."""
    out = bytearray()
    for k, L in enumerate(lengths):
        out += bytes([7]) * L + bytes([100 + 2 * k, 101 + 2 * k])
    return bytes(out)


def photo_like(H, W, C, seed=0):
    """A smooth field plus a little noise: what a filtered photograph looks like to the coder (no image files are needed)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    chans = []
    for c in range(C):
        f = 128 + 80 * np.sin(x / (17.0 + 3 * c) + seed) * np.cos(y / (23.0 + 2 * c)) + 30 * np.sin((x + y) / 5.0)
        chans.append(f + rng.normal(0, 2.5, size=(H, W)))
    return np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)
