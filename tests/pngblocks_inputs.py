"""The streams of the block-parallel inflate plan's tests, on top of tests/pngdec_inputs.py: zlib streams of many short dynamic blocks (small
memLevel), far and overlapping matches across block borders, the smallest real PIL files with more than one block, dynamic headers inside a
stored payload (false candidates), and damaged streams.  Shared by tests/test_pngblocks_cpu.py (the sanitized host program around
reface_amd/csrc/png_blocks.h) and tests/test_pngblocks_gpu.py (the device), so both meet the same bytes.  Built once per process."""
import functools
import io
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngdec_inputs as I  # noqa: E402
import pngenc_refs as R  # noqa: E402

MIN_BYTES = 16384          # the tests' eligibility threshold: the streams below are 49152 bytes and more, most of pngdec_inputs' are shorter
BLOCK_BYTES = (64, 1024)   # the capacities the host program and the device are run at

# name -> the least number of dynamic blocks (counted with zlib 1.2.11; the tests print what they see)
MULTI_BLOCK = {"low_ml1": 154, "low_ml3": 39, "low_huff": 193, "per32k_ml3": 118, "const_ml1": 7, "pil160_l1": 2, "pil160_l6": 3, "pil160_l9": 3}


def _z(raw, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return co.compress(raw) + co.flush()


def noisy_photo(H, W, C, seed, amp=8):
    """R.photo_like with sensor-like noise of +-amp on top: zlib's level 1 then starts a second block within 160 x 160 x 3 bytes"""
    img = R.photo_like(H, W, C, seed=seed).astype(np.int32) + np.random.RandomState(seed + 1).randint(-amp, amp + 1, size=(H, W, C))
    return np.clip(img, 0, 255).astype(np.uint8)


def pil160_image():
    return noisy_photo(160, 160, 3, 5)


def pil_png(img, level=6):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG", compress_level=level)
    return buf.getvalue()


def pil_stream(img, level):
    """the zlib stream (the IDAT payloads) of the file PIL writes for img"""
    from reface_amd import pngdec
    data = pil_png(img, level)
    return pngdec.parse_png(data).idat(data)


def _stored_blocks(data):
    """non-final stored blocks around data, at most 65535 bytes each"""
    return b"".join(I.stored_block(data[o:o + 65535], False) for o in range(0, len(data), 65535))


@functools.lru_cache(maxsize=None)
def block_streams():
    """name -> (zlib stream, raw bytes)"""
    g = {}
    low = I.rng_bytes(49152, 61, hi=16)          # (this seed: zlib ends low_ml1 with a fixed block)
    g["low_ml1"] = (_z(low, 6, 1), low)
    g["low_ml3"] = (_z(low, 6, 3), low)
    g["low_huff"] = (_z(low, 6, 2, zlib.Z_HUFFMAN_ONLY), low)
    g["low_fixed"] = (_z(low, 6, 2, zlib.Z_FIXED), low)
    per = I.rng_bytes(32768, 42, hi=16) * 5
    g["per32k_ml3"] = (_z(per, 9, 3), per)
    const = bytes(200000)
    g["const_ml1"] = (_z(const, 6, 1), const)
    img = pil160_image()
    for level in (1, 6, 9):
        z = pil_stream(img, level)
        g[f"pil160_l{level}"] = (z, zlib.decompress(z))
    # dynamic headers inside a stored payload: raw deflate of A up to a sync flush, the whole low_ml3 stream as stored payload, raw deflate of B
    a, b, pay = I.rng_bytes(30000, 43, hi=16), I.rng_bytes(30000, 44, hi=16), g["low_ml3"][0]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 3)
    da = co.compress(a) + co.flush(zlib.Z_SYNC_FLUSH)
    raw = a + pay + b
    g["embedded"] = (I.zwrap(da + _stored_blocks(pay) + _z(b, 6, 3, wbits=-15), raw), raw)
    for name, (z, raw) in g.items():
        assert zlib.decompress(z) == raw, name
    return g


@functools.lru_cache(maxsize=None)
def damaged_block_streams():
    """name -> (damaged stream, expected output length): every one ends on the serial plan with the serial plan's code"""
    z, raw = block_streams()["low_ml3"]
    n, d = len(raw), {}
    d["blk_bad_adler"] = (z[:-1] + bytes([z[-1] ^ 0x40]), n)
    d["blk_cut_half"] = (z[:len(z) // 2], n)
    d["blk_cut_last3"] = (z[:-3], n)
    # a bit inside the codes of chunk 5 (the blocks of low_ml3 are of about equal size): the first one from there that zlib refuses
    pos = 8 * int(len(z) * 5.5 / MULTI_BLOCK["low_ml3"])
    while True:
        bad = bytearray(z)
        bad[pos >> 3] ^= 1 << (pos & 7)
        try:
            ok = zlib.decompress(bytes(bad)) == raw
        except zlib.error:
            ok = False
        if not ok:
            break
        pos += 1
    d["blk_flip_chunk5"] = (bytes(bad), n)
    # a second chunk whose first match reaches in front of the stream: the blocks zlib writes against a preset dictionary, behind a first
    # chunk that produced far less than the dictionary's length
    head, dic = I.rng_bytes(300, 45, hi=16), I.rng_bytes(30000, 46, hi=16)
    body = dic[1000:20000]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 3)
    d1 = co.compress(head) + co.flush(zlib.Z_FULL_FLUSH)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 3, zlib.Z_DEFAULT_STRATEGY, dic)
    d2 = co.compress(body) + co.flush()
    d["blk_distance_before_start"] = (I.zwrap(d1 + d2, head + body), len(head) + len(body))
    for name, (zb, nb) in d.items():
        try:
            ok = len(zlib.decompress(zb)) == nb
        except zlib.error:
            ok = False
        assert not ok, name
    return d


@functools.lru_cache(maxsize=None)
def corpus():
    """every stream both test files run: name -> (stream, expected length, raw bytes or None for a damaged one)"""
    c = {}
    for name, (z, raw, _) in I.good_streams().items():
        c[name] = (z, len(raw), raw)
    for name, (z, raw) in block_streams().items():
        c[name] = (z, len(raw), raw)
    for name, (z, n) in list(I.damaged_streams().items()) + list(damaged_block_streams().items()):
        c[name] = (z, n, None)
    return c
