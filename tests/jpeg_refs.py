"""numpy restatement of reface_amd/csrc/jpegenc.hip (libjpeg's integer arithmetic), the oracle of the JPEG tests, and an independent minimal
RIFF / AVI parser for the container tests.

Three stages, as on the device: ``coefficients`` (colour transform, h2v2 downsample, "islow" DCT, quantisation; blocks in scan order),
``intervals`` (one Huffman-coded, byte-stuffed string per MCU row) and ``pack`` (RSTn between the intervals, EOI behind).  ``encode`` puts
``reface_amd.mjpeg.jpeg_header`` in front; tests/test_mjpeg_cpu.py pins the whole file against PIL's.
"""
import functools
import struct

import numpy as np

from reface_amd import mjpeg as M

ZIGZAG = np.array(M.ZIGZAG)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    """libjpeg rgb_ycc_convert: uint8 [..., 3] -> int64 Y, Cb, Cr."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + 32768) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint's butterflies along the last axis of int64 [..., 8]; `first`: the row pass."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    n = 11 if first else 15
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _quantised_blocks(plane, qtable):
    """int64 sample plane [8 * by, 8 * bx] -> int64 [by, bx, 64] quantised coefficients in zigzag order."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128
    d = _fdct_1d(d, True)
    d = _fdct_1d(d.swapaxes(-1, -2), False).swapaxes(-1, -2)
    q8 = 8 * np.asarray(qtable, dtype=np.int64).reshape(8, 8)
    c = np.sign(d) * ((np.abs(d) + (q8 >> 1)) // q8)
    return c.reshape(by, bx, 64)[:, :, ZIGZAG]


def coefficients(img, quality, subsampling):
    """uint8 [H, W, 3 | 4] -> int16 [MCU rows, blocks per MCU row, 64] (zigzag order; per MCU Y00 Y01 Y10 Y11 Cb Cr or Y Cb Cr)."""
    H, W = img.shape[:2]
    mrows, mcus, bpm = M.geometry(H, W, subsampling)
    luma_q, chroma_q = M.quant_tables(quality)
    y, cb, cr = ycc(img[..., :3])
    s = 2 if subsampling == "420" else 1
    rows, cols = np.minimum(np.arange(mrows * 8 * s), H - 1), np.minimum(np.arange(mcus * 8 * s), W - 1)
    Y = _quantised_blocks(y[rows][:, cols], luma_q)
    if s == 1:
        C = [_quantised_blocks(c[rows][:, cols], chroma_q) for c in (cb, cr)]
        return np.stack([Y, C[0], C[1]], axis=2).reshape(mrows, mcus * 3, 64).astype(np.int16)
    # h2v2: the full-resolution plane is edge-replicated in both directions, 2 x 2 boxes are averaged with the bias 1, 2, 1, 2, ... along a row,
    # and the downsampled plane's last row is replicated down
    crow = np.minimum(np.arange(mrows * 8), (H + 1) // 2 - 1)
    r0, r1 = np.minimum(2 * crow, H - 1), np.minimum(2 * crow + 1, H - 1)
    ccol = np.arange(mcus * 8)
    c0, c1 = np.minimum(2 * ccol, W - 1), np.minimum(2 * ccol + 1, W - 1)
    bias = 1 + (ccol & 1)
    C = []
    for c in (cb, cr):
        small = (c[r0][:, c0] + c[r0][:, c1] + c[r1][:, c0] + c[r1][:, c1] + bias[None, :]) >> 2
        C.append(_quantised_blocks(small, chroma_q))
    # dummy Y blocks (past the component's own size in blocks): AC = 0, DC = the DC of the block before them in the MCU
    hib, wib = (H + 7) // 8, (W + 7) // 8
    out = np.zeros((mrows, mcus, 6, 64), dtype=np.int64)
    for k in range(4):
        blk = Y[k >> 1::2, k & 1::2].copy()
        by = 2 * np.arange(mrows)[:, None] + (k >> 1)
        bx = 2 * np.arange(mcus)[None, :] + (k & 1)
        dummy = (by >= hib) | (bx >= wib)
        if k:
            blk[dummy] = 0
            blk[dummy, 0] = out[:, :, k - 1, 0][dummy]
        out[:, :, k] = blk
    out[:, :, 4], out[:, :, 5] = C
    return out.reshape(mrows, mcus * 6, 64).astype(np.int16)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


_CODES = [M.huffman_codes(*t) for t in M.HUFF_TABLES]          # DC luma, AC luma, DC chroma, AC chroma


def _amplitude(v):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v + (1 << n) - 1)


def intervals(coefs, subsampling, stats=None):
    """int16 [MCU rows, blocks per row, 64] -> one byte string per MCU row.  `stats` (a dict) counts the ZRL symbols, EOB-only blocks and
    stuffed bytes met."""
    comp = (0, 0, 0, 0, 1, 2) if subsampling == "420" else (0, 1, 2)
    out = []
    for row in coefs.astype(np.int64):
        bw, pred = _Bits(), [0, 0, 0]
        for j, block in enumerate(row):
            c = comp[j % len(comp)]
            dc, ac = _CODES[2 * (c > 0)], _CODES[2 * (c > 0) + 1]
            n, amp = _amplitude(int(block[0]) - pred[c])
            pred[c] = int(block[0])
            bw.put(*dc[n])
            bw.put(amp, n)
            last = 0
            nz = np.flatnonzero(block[1:]) + 1
            for k in nz:
                run = int(k) - last - 1
                while run > 15:
                    bw.put(*ac[0xF0])
                    run -= 16
                    if stats is not None:
                        stats["zrl"] = stats.get("zrl", 0) + 1
                n, amp = _amplitude(int(block[k]))
                bw.put(*ac[(run << 4) | n])
                bw.put(amp, n)
                last = int(k)
            if last < 63:
                bw.put(*ac[0x00])
                if stats is not None and last == 0:
                    stats["eob_only"] = stats.get("eob_only", 0) + 1
        data = bw.finish()
        if stats is not None:
            stats["stuffed"] = stats.get("stuffed", 0) + data.count(b"\xff\x00")
        out.append(data)
    return out


def pack(parts):
    """The intervals back to back with RSTn between consecutive ones and EOI behind the last."""
    out = bytearray()
    for i, p in enumerate(parts):
        out += p
        out += bytes([0xFF, 0xD0 + (i & 7)]) if i < len(parts) - 1 else b"\xff\xd9"
    return bytes(out)


def encode(img, quality, subsampling, stats=None):
    H, W = img.shape[:2]
    return M.jpeg_header(H, W, quality, subsampling) + pack(intervals(coefficients(img, quality, subsampling), subsampling, stats))


# ------------------------------------------------------------------------------------------------ the test images
SIZES = [(1, 1), (8, 8), (16, 16), (33, 47), (17, 130), (100, 36), (48, 80), (160, 32)]
GPU_SIZES = SIZES + [(64, 520), (24, 2064)]
QUALITIES = (30, 75, 90, 100)
KINDS = ("noise", "smooth", "zeros", "ones")


@functools.lru_cache(maxsize=None)
def image(kind, H, W, C=3):
    rng = np.random.RandomState(H * 7919 + W * 31 + C)
    if kind == "noise":
        img = rng.randint(0, 256, (H, W, C))
    elif kind == "smooth":
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([128 + 100 * np.sin(xx / 23.0 + c) * np.cos(yy / 17.0 - c) for c in range(C)], axis=2) + rng.randint(-3, 4, (H, W, C))
        # every third block carries a fine checkerboard: a few of the highest-frequency coefficients behind long runs of zeros
        img += (((yy // 8 + xx // 8) % 3 == 0) * 70 * (1 - 2 * ((yy + xx) & 1)))[..., None]
        img = np.clip(np.rint(img), 0, 255)
    else:
        img = np.full((H, W, C), 0 if kind == "zeros" else 255)
    img = img.astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def model_coefficients(kind, H, W, quality, subsampling):
    c = coefficients(image(kind, H, W), quality, subsampling)
    c.setflags(write=False)
    return c


def pil_jpeg(img, quality, subsampling):
    """PIL's (libjpeg's) file for the same arguments: one restart interval per MCU row."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).convert("RGB").save(buf, "JPEG", quality=quality, subsampling={"420": 2, "444": 0}[subsampling],
                                                                   restart_marker_rows=1)
    return buf.getvalue()


# ------------------------------------------------------------------------------------------------ an independent RIFF / AVI reader
def _chunks(data, start, end):
    """[(fourcc, payload offset, size)] of the chunks in data[start:end]; every chunk starts on an even offset."""
    out, p = [], start
    while p < end:
        assert p % 2 == 0, f"chunk at odd offset {p}"
        assert p + 8 <= end, f"truncated chunk header at {p}"
        cc, size = data[p:p + 4], struct.unpack_from("<I", data, p + 4)[0]
        assert p + 8 + size <= end, f"chunk {cc} at {p} runs past its parent ({size} bytes)"
        out.append((cc, p + 8, size))
        p += 8 + size + (size & 1)
    assert p == end, f"chunks end at {p}, parent at {end}"
    return out


def parse_avi(data):
    """Walk a RIFF AVI file, asserting its structure; returns the header fields and the frames' bytes (read through idx1)."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    riff_size = struct.unpack_from("<I", data, 4)[0]
    assert riff_size + 8 == len(data), (riff_size, len(data))
    top = _chunks(data, 12, len(data))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"]
    (_, h0, hsize), (_, m0, msize), (_, i0, isize) = top
    assert data[h0:h0 + 4] == b"hdrl" and data[m0:m0 + 4] == b"movi"
    hdrl = _chunks(data, h0 + 4, h0 + hsize)
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"]
    avih = struct.unpack_from("<14I", data, hdrl[0][1])
    assert hdrl[0][2] == 56
    s0, ssize = hdrl[1][1], hdrl[1][2]
    assert data[s0:s0 + 4] == b"strl"
    strl = _chunks(data, s0 + 4, s0 + ssize)
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    strh = struct.unpack_from("<4s4sIHHIIIIIIII4H", data, strl[0][1])
    strf = struct.unpack_from("<IiiHH4sIiiII", data, strl[1][1])
    movi = _chunks(data, m0 + 4, m0 + msize)
    assert all(c[0] == b"00dc" for c in movi)
    assert isize % 16 == 0
    frames = []
    for k in range(isize // 16):
        cc, flags, off, size = struct.unpack_from("<4sIII", data, i0 + 16 * k)
        at = m0 + off          # offsets count from the `movi` tag
        assert cc == b"00dc" and flags & 0x10 and data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == size
        assert (at + 8, size) == movi[k][1:]
        frames.append(data[at + 8:at + 8 + size])
    assert len(frames) == len(movi)
    return {"usec_per_frame": avih[0], "flags": avih[3], "total_frames": avih[4], "streams": avih[6], "width": avih[8], "height": avih[9],
            "fcc_type": strh[0], "handler": strh[1], "scale": strh[6], "rate": strh[7], "length": strh[9],
            "bi_size": strf[0], "bi_width": strf[1], "bi_height": strf[2], "bi_planes": strf[3], "bi_bits": strf[4], "bi_compression": strf[5],
            "frames": frames}
