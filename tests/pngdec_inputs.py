"""The zlib-stream corpus of the PNG decoder's tests: good streams (zlib's own at several levels and strategies, flushed streams, hand-built
blocks that zlib never writes, the GPU encoder's streams from tests/pngenc_refs.py) and damaged ones derived from them.  Shared by
tests/test_pngdec_cpu.py (the sanitized host program around reface_amd/csrc/png_inflate.h) and tests/test_pngdec_gpu.py (the device), so both
meet the same bytes.  Built once per process."""
import functools
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngenc_refs as R  # noqa: E402

SEG = R.SEG


def rng_bytes(n, seed, hi=256):
    return np.random.RandomState(seed).randint(0, hi, size=n).astype(np.uint8).tobytes()


def _straddle(k):
    """as tests/test_pngenc_gpu.py: a run that starts k bytes before a segment boundary and runs 300 bytes past it"""
    head = rng_bytes(SEG - k, 11, hi=4)
    head = head[:-1] + bytes([200])
    return head + bytes([9]) * (k + 300) + rng_bytes(500, 12, hi=4)


# the encoder tests' streams (the lengths 1, 2, 32767, 32768, 32769, 65539 among them)
ENCODER_RAW = {
    "len1": b"\x2a",
    "len2": b"\x05\x05",
    "len32767": rng_bytes(32767, 1, hi=6),
    "len32768": rng_bytes(32768, 2, hi=6),
    "len32769": rng_bytes(32769, 3, hi=6),
    "len65539": rng_bytes(65536 + 3, 4, hi=6),
    "noise": rng_bytes(SEG + 17, 5),                   # a stored segment, then a short one
    "noise3": rng_bytes(2 * SEG + 9, 6),               # two stored segments in a row: no marker between them
    "zeros": bytes(2 * SEG + 3),                       # flat
    "runs": R.runs_stream(),
    "straddle1": _straddle(1),
    "straddle2": _straddle(2),
    "straddle3": _straddle(3),
    "fibonacci": R.fibonacci_stream(),                 # 15-bit codes
    "mixed": rng_bytes(SEG, 21, hi=3) + bytes(SEG) + rng_bytes(SEG, 22) + rng_bytes(5, 23, hi=3),          # coded, flat, stored, coded
    "seg3plus5": rng_bytes(3 * SEG + 5, 24, hi=5),     # 3 x 32768 + 5 bytes, every segment coded: exactly 3 markers
}


class BitWriter:
    """LSB-first bit packing; Huffman codes go in most significant bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> k) & 1 for k in range(n)]

    def code(self, value, n):
        self.bits += [(value >> (n - 1 - k)) & 1 for k in range(n)]

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)

    def bytes(self):
        self.align()
        return np.packbits(np.array(self.bits, dtype=np.uint8), bitorder="little").tobytes()


def _fixed_lit(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def _fixed_match(w, length, dist):
    k = max(i for i, b in enumerate(R.LEN_BASE) if b <= length) if length < 258 else 28
    _fixed_lit(w, 257 + k)
    w.put(length - R.LEN_BASE[k], R.LEN_EXTRA[k])
    d = 0 if dist < 5 else None
    if dist < 5:
        d, eb, base = dist - 1, 0, dist
    else:
        eb = (dist - 1).bit_length() - 2
        d = 2 * eb + 2 + (((dist - 1) >> eb) & 1)
        base = 1 + ((2 + (d & 1)) << eb)
    w.code(d, 5)
    w.put(dist - base, eb)


def zwrap(deflate, raw):
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def stored_block(data, final):
    return bytes([1 if final else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def fixed_block(tokens, final):
    """tokens: ints (literals) or (length, distance)"""
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            _fixed_match(w, *t)
        else:
            _fixed_lit(w, t)
    _fixed_lit(w, 256)
    return w.bytes()


def _compress(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, prev = b"", 0
    for p in flush_at:
        out += co.compress(raw[prev:p]) + co.flush(flush)
        prev = p
    return out + co.compress(raw[prev:]) + co.flush()


def _texty(n, seed):
    """compressible content with long and far matches: words from a small vocabulary, a zero run, and a repeat from far back"""
    rng = np.random.RandomState(seed)
    words = [rng_bytes(int(rng.randint(3, 12)), 100 + k, hi=64) for k in range(200)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.randint(0, 200))]
    out = bytes(out[:n])
    return out[:n // 3] + bytes(1000) + out[n // 3:n - 1500] + out[:500]


@functools.lru_cache(maxsize=None)
def good_streams():
    """name -> (zlib stream, raw bytes, expected inflate plan on the device)"""
    g = {}
    text = _texty(70000, 1)
    photo = R.filter_image(R.photo_like(48, 64, 3, seed=2))[0].tobytes()
    for level in (0, 1, 6, 9):
        g[f"zlib{level}_text"] = (_compress(text, level), text, "serial")
        g[f"zlib{level}_photo"] = (_compress(photo, level), photo, "serial")
    for name, strat in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman_only", zlib.Z_HUFFMAN_ONLY)):
        g[f"zlib_{name}"] = (_compress(text, 6, strat), text, "serial")
    fib = R.fibonacci_stream()          # symbol counts along the Fibonacci numbers: zlib's length-limited code for them reaches 15 bits
    g["zlib_fibonacci"] = (_compress(fib, 6, zlib.Z_HUFFMAN_ONLY), fib, "serial")
    g["sync_flush"] = (_compress(text, 6, flush_at=(20000, 50000)), text, "serial")
    g["full_flush"] = (_compress(text, 6, flush_at=(SEG,), flush=zlib.Z_FULL_FLUSH), text, "serial")
    # Z_SYNC_FLUSH keeps the window: the second half repeats the first, so its matches reach across the flush point
    half = rng_bytes(SEG, 31, hi=200)
    g["sync_flush_crossing"] = (_compress(half + half, 6, flush_at=(SEG,)), half + half, "serial")
    # the same 32768 + 32768 bytes with Z_FULL_FLUSH: two independent pieces of exactly a window each.  A foreign stream the chain accepts.
    g["full_flush_32768"] = (_compress(half + half, 6, flush_at=(SEG,), flush=zlib.Z_FULL_FLUSH), half + half, "segments")
    # a false candidate: the marker inside a stored block's payload
    pay = rng_bytes(300, 32) + b"\x00\x00\xff\xff" + rng_bytes(40000, 33)
    g["stored_payload_marker"] = (_compress(pay, 0), pay, "serial")
    # what zlib never writes: a match at distance 32768 (and of 258 bytes), by hand
    far = rng_bytes(SEG, 34)
    raw = far + far[:258] + b"\x07" + far[259:259 + 3]
    g["dist32768"] = (zwrap(stored_block(far, False) + fixed_block([(258, 32768), 7, (3, 32768)], True), raw), raw, "serial")
    # a distance-1 run over several maximal matches, and short distances below the wave width
    raw = b"ab" + b"b" * 700 + b"xyz" * 100 + b"q"
    g["run_dist1"] = (zwrap(fixed_block([97, 98, (258, 1), (258, 1), (184, 1), 120, 121, 122, (258, 3), (39, 3), 113], True), raw), raw, "serial")
    # an empty stored block in the middle and at the very start
    raw = b"hello"
    g["empty_stored_first"] = (zwrap(stored_block(b"", False) + stored_block(raw, True), raw), raw, "serial")
    # one distance in use (zlib itself pads its distance code to two codes; the encoder's streams have the incomplete one-code form)
    g["one_distance_code"] = (_compress(bytes(5000) + b"\x01", 6, zlib.Z_RLE), bytes(5000) + b"\x01", "serial")
    for name, raw in ENCODER_RAW.items():
        g[f"enc_{name}"] = (R.zlib_stream(raw), raw, "segments" if len(raw) > SEG else "serial")
    return g


def _dynamic_oversubscribed():
    """a dynamic block whose code-length code has 19 codes of one bit"""
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(15, 4)
    for _ in range(19):
        w.put(1, 3)
    w.put(0, 64)
    return w.bytes()


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """name -> (damaged stream, expected output length): each must give a non-zero error code, never a wrong image, a fault or a hang"""
    g = good_streams()
    d = {}
    z, raw, _ = g["zlib6_text"]
    n = len(raw)
    for k, cut in enumerate(np.linspace(0, len(z) - 1, 50).astype(int)):
        d[f"trunc{k:02d}_{cut}"] = (z[:cut], n)
    rng = np.random.RandomState(7)
    kept = 0
    for base in ("zlib6_text", "zlib_fixed", "enc_seg3plus5", "zlib0_photo", "sync_flush"):
        zb, rb, _ = g[base]
        for pos in rng.randint(0, 8 * len(zb), size=40):
            bad = bytearray(zb)
            bad[pos >> 3] ^= 1 << (pos & 7)
            bad = bytes(bad)
            try:
                zlib.decompress(bad)
            except zlib.error:
                d[f"flip_{base}_{pos}"] = (bad, len(rb))
                kept += 1
    assert kept >= 100, kept
    d["bad_adler"] = (z[:-1] + bytes([z[-1] ^ 1]), n)
    z0, r0, _ = g["zlib0_photo"]
    d["len_nlen_mismatch"] = (z0[:5] + bytes([z0[5] ^ 0x10]) + z0[6:], len(r0))
    d["oversubscribed"] = (zwrap(_dynamic_oversubscribed(), b""), 10)
    d["distance_before_start"] = (zwrap(fixed_block([65, 66, (4, 5)], True), b"ABABAB"), 6)
    d["output_longer"] = (z, n - 1)
    d["output_longer_far"] = (z, n // 2)
    d["output_shorter"] = (z, n + 1)
    d["bad_zlib_header"] = (b"\x78\x02" + z[2:], n)
    d["preset_dictionary"] = (b"\x78\x20" + z[2:], n)
    d["block_type_3"] = (zwrap(b"\x07" + bytes(8), b""), 4)
    d["empty"] = (b"", 4)
    d["one_byte"] = (b"\x78", 4)
    # the segmented plan on damaged chains: a piece of an encoder stream cut out / a byte of a middle piece changed
    ze, re_, _ = g["enc_seg3plus5"]
    cands = [2] + [i + 4 for i in range(len(ze)) if ze[i:i + 4] == b"\x00\x00\xff\xff"]
    d["enc_piece_removed"] = (ze[:cands[1]] + ze[cands[2]:], len(re_))
    mid = (cands[1] + cands[2]) // 2
    d["enc_piece_changed"] = (ze[:mid] + bytes([ze[mid] ^ 0x55]) + ze[mid + 1:], len(re_))
    for name, (zb, nb) in d.items():
        try:
            ok = len(zlib.decompress(zb)) == nb
        except zlib.error:
            ok = False
        assert not ok, name
    return d
