"""A pure numpy / Python integer JPEG decoder, the oracle of the GPU JPEG decoder's tests (reface_amd/jpegdec.py, csrc/jpegdec.hip), and
the corpus both test files share.

Four stages, as on the device: ``entropy_decode`` (Huffman scan -> coefficients, one restart interval at a time), ``idct_planes``
(dequantisation and libjpeg's jpeg_idct_islow), ``upsample`` (libjpeg's fancy h2v1 / h2v2) and ``ycc_rgb``.  ``decode`` chains them
and must equal PIL exactly: tests/test_jpegdec_cpu.py proves the restated arithmetic that way on a machine without a GPU.  The marker
walk is ``reface_amd.jpegdec.parse_jpeg``; everything behind it is restated here independently (bit-by-bit canonical Huffman decoding from
BITS / HUFFVAL, a byte split at the RSTn markers).
"""
import functools
import io
import re
import struct

import numpy as np
from PIL import Image

from reface_amd import jpegdec as J
from reface_amd import mjpeg as M

ZIGZAG = np.array(M.ZIGZAG)
E_TRUNCATED, E_BAD_CODE, E_INDEX, E_RST_COUNT, E_RST_ORDER, E_SYMBOL = 1, 2, 3, 4, 5, 6


class RefError(ValueError):
    def __init__(self, code):
        super().__init__(f"reference decoder: code {code}")
        self.code = code


# ------------------------------------------------------------------------------------------------ entropy decode
def _codebook(bits, vals):
    """{(length, code): symbol} of one table (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Reader:
    """The bits of one interval: 00 behind FF dropped, the data ends at the first marker; zeros behind the end, and reading them is an error."""

    def __init__(self, seg):
        m = re.search(rb"\xff[^\x00]", seg)
        if m:
            seg = seg[:m.start()]
        if seg.endswith(b"\xff"):
            seg = seg[:-1]
        seg = seg.replace(b"\xff\x00", b"\xff")
        self.bits = np.concatenate([np.unpackbits(np.frombuffer(seg, dtype=np.uint8)), np.zeros(64, dtype=np.uint8)]).tolist()
        self.n, self.pos = 8 * len(seg), 0

    def symbol(self, book):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bits[self.pos + length - 1]
            s = book.get((length, code))
            if s is not None:
                self.pos += length
                if self.pos > self.n:
                    raise RefError(E_TRUNCATED)
                return s
        raise RefError(E_BAD_CODE)

    def amplitude(self, s):
        v = 0
        for b in self.bits[self.pos:self.pos + s]:
            v = (v << 1) | b
        self.pos += s
        if self.pos > self.n:
            raise RefError(E_TRUNCATED)
        return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def split_intervals(scan):
    """The scan cut at its RSTn markers: ([interval bytes], [n of every RSTn])."""
    parts, nums, last = [], [], 0
    for m in re.finditer(rb"\xff[\xd0-\xd7]", scan):
        parts.append(scan[last:m.start()])
        nums.append(scan[m.start() + 1] - 0xD0)
        last = m.end()
    parts.append(scan[last:])
    return parts, nums


def entropy_decode(info, data):
    """-> int16 [blocks, 64]: natural order, blocks in scan order.  Raises RefError(code) where the device leaves a code."""
    scan = data[info.scan[0]:info.scan[0] + info.scan[1]]
    mx, my, bpm = info.geometry
    mcus, ri = mx * my, info.ri
    parts, nums = split_intervals(scan)
    if len(parts) != (-(-mcus // ri) if ri else 1):
        raise RefError(E_RST_COUNT)
    if nums != [k & 7 for k in range(len(nums))]:
        raise RefError(E_RST_ORDER)
    books = {k: _codebook(*t) for k, t in info.huff.items()}
    comps = [0] * (info.hs * info.vs) + [1, 2] if info.ncomp == 3 else [0]
    out = np.zeros((mcus * bpm, 64), dtype=np.int64)
    blk = 0
    for k, seg in enumerate(parts):
        rd, pred = _Reader(seg), [0, 0, 0]
        for _ in range(min(ri, mcus - k * ri) if ri else mcus):
            for c in comps:
                dc, ac = books[(0, info.td[c])], books[(1, info.ta[c])]
                s = rd.symbol(dc)
                if s > 15:
                    raise RefError(E_SYMBOL)
                pred[c] += rd.amplitude(s)
                out[blk, 0] = pred[c]
                i = 1
                while i < 64:
                    rs = rd.symbol(ac)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        i += 16
                        continue
                    i += r
                    if i > 63:
                        raise RefError(E_INDEX)
                    out[blk, ZIGZAG[i]] = rd.amplitude(s)
                    i += 1
                blk += 1
    return out.astype(np.int16)


# ------------------------------------------------------------------------------------------------ IDCT (jpeg_idct_islow)
def _idct_1d(d):
    """The butterflies along the last axis of int64 [..., 8]; the caller descales."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    tmp2, tmp3 = z1 - i6 * 15137, z1 + i2 * 6270
    tmp0, tmp1 = (i0 + i4) << 13, (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], axis=-1)


def idct_blocks(coef, q):
    """int [n, 64] coefficients, 64 quantisation values (natural order) -> uint8 [n, 8, 8]."""
    d = (coef.astype(np.int64) * np.asarray(q, dtype=np.int64)).reshape(-1, 8, 8)
    ws = (_idct_1d(d.swapaxes(1, 2)).swapaxes(1, 2) + (1 << 10)) >> 11          # columns
    out = ((_idct_1d(ws) + (1 << 17)) >> 18) + 128                               # rows
    return np.clip(out, 0, 255).astype(np.uint8)


def idct_planes(info, coef):
    """-> the component planes, each padded to whole MCUs."""
    mx, my, bpm = info.geometry
    c4 = coef.reshape(my, mx, bpm, 64)
    if info.ncomp == 1:
        px = idct_blocks(c4.reshape(-1, 64), info.quant[info.tq[0]]).reshape(my, mx, 8, 8)
        return [px.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)]
    hs, vs = info.hs, info.vs
    y = idct_blocks(c4[:, :, :hs * vs].reshape(-1, 64), info.quant[info.tq[0]]).reshape(my, mx, vs, hs, 8, 8)
    planes = [y.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)]
    for c in (1, 2):
        px = idct_blocks(c4[:, :, hs * vs + c - 1].reshape(-1, 64), info.quant[info.tq[c]]).reshape(my, mx, 8, 8)
        planes.append(px.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return planes


# ------------------------------------------------------------------------------------------------ upsampling and colour
def _h2v1(p):
    """libjpeg h2v1_fancy_upsample on int64 [h, w] -> [h, 2 w]."""
    prev, nxt = np.concatenate([p[:, :1], p[:, :-1]], axis=1), np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    left, right = (3 * p + prev + 1) >> 2, (3 * p + nxt + 2) >> 2
    left[:, 0], right[:, -1] = p[:, 0], p[:, -1]
    return np.stack([left, right], axis=2).reshape(p.shape[0], -1)


def _h2v2(p):
    """libjpeg h2v2_fancy_upsample on int64 [h, w] -> [2 h, 2 w]."""
    up, down = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    rows = np.stack([3 * p + up, 3 * p + down], axis=1).reshape(-1, p.shape[1])          # colsum of output rows 2r, 2r + 1
    last, nxt = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1), np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    left, right = (3 * rows + last + 8) >> 4, (3 * rows + nxt + 7) >> 4
    left[:, 0], right[:, -1] = (4 * rows[:, 0] + 8) >> 4, (4 * rows[:, -1] + 7) >> 4
    return np.stack([left, right], axis=2).reshape(rows.shape[0], -1)


def upsample(info, plane):
    """A padded chroma plane -> int64 [H, W]: cut to the real downsampled size first -- the edges are those of the real plane."""
    H, W, hs, vs = info.height, info.width, info.hs, info.vs
    p = plane[:-(-H // vs), :-(-W // hs)].astype(np.int64)
    if (hs, vs) == (2, 1):
        p = _h2v1(p)
    elif (hs, vs) == (2, 2):
        p = _h2v2(p)
    return p[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb - 128, cr - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data, mode=None):
    """A device-eligible file -> PIL's array: [H, W] for grey, [H, W, 3] for colour (or for ``mode="RGB"``)."""
    info = J.parse_jpeg(data)
    assert info.route == "gpu", info.reason
    planes = idct_planes(info, entropy_decode(info, data))
    H, W = info.height, info.width
    if info.ncomp == 1:
        g = planes[0][:H, :W]
        return np.stack([g] * 3, axis=2) if mode == "RGB" else g
    assert mode in (None, "RGB")
    return ycc_rgb(planes[0][:H, :W], upsample(info, planes[1]), upsample(info, planes[2]))


def pil_decode(data, mode=None):
    im = Image.open(io.BytesIO(data))
    if mode is not None:
        im = im.convert(mode)
    return np.asarray(im)


# ------------------------------------------------------------------------------------------------ the corpus
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (97, 131), (200, 256)]
SAMPLINGS = ("grey", "444", "422", "420")
QUALITIES = (30, 90, 100)
KINDS = ("noise", "smooth", "const", "checker")
RESTARTS = ({}, {"restart_marker_rows": 1}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3})
_SUB = {"444": 0, "422": 1, "420": 2}


@functools.lru_cache(maxsize=None)
def image(kind, H, W):
    """uint8 [H, W, 3]: noise, a smooth field plus noise (as tests/jpeg_refs.image), a constant, a 0 / 255 checker."""
    rng = np.random.RandomState(H * 7919 + W * 31 + len(kind))
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        img = rng.randint(0, 256, (H, W, 3))
    elif kind == "smooth":
        img = np.stack([128 + 100 * np.sin(xx / 23.0 + c) * np.cos(yy / 17.0 - c) for c in range(3)], axis=2) + rng.randint(-3, 4, (H, W, 3))
        img = np.clip(np.rint(img), 0, 255)
    elif kind == "const":
        img = np.full((H, W, 3), 0) + np.array([200, 30, 90])
    else:
        img = (((yy + xx) & 1) * 255)[..., None].repeat(3, axis=2)
    img = img.astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def pil_file(kind, H, W, sampling, quality, restart=0, optimize=False):
    """PIL's JPEG file of image(kind, H, W): `sampling` in SAMPLINGS, `restart` an index into RESTARTS."""
    im = Image.fromarray(image(kind, H, W))
    kw = dict(RESTARTS[restart])
    if sampling == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = _SUB[sampling]
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, optimize=optimize, **kw)
    return buf.getvalue()


def cases(full=False):
    """(kind, H, W, sampling, quality, restart, optimize): every value of every axis with every sampling; with `full` the whole product of
    sizes x samplings x restarts on top (the GPU decodes it in one launch)."""
    out = []
    for s in SAMPLINGS:
        axes = [[(k, 17, 33, s, 90, 0, False) for k in KINDS], [("smooth", H, W, s, 90, 0, False) for H, W in SIZES],
                [("noise", 17, 33, s, q, 0, False) for q in QUALITIES], [("smooth", 97, 131, s, 90, r, False) for r in range(len(RESTARTS))],
                [("noise", 17, 33, s, 30, 3, True), ("smooth", 97, 131, s, 100, 1, True), ("checker", 7, 9, s, 100, 2, False), ("const", 1, 1, s, 30, 3, False)]]
        for a in axes:
            out += a
        if full:
            out += [(k, H, W, s, q, r, r == 2) for (H, W), k, q in zip(SIZES, KINDS * 2, QUALITIES * 3) for r in range(len(RESTARTS))]
            out += [("checker", H, W, s, 100, 0, False) for H, W in SIZES[:5]] + [("noise", 200, 256, s, 100, 1, False)]
    return list(dict.fromkeys(out))


def strip_dht(data):
    """The file without its DHT segments (an AVI MJPG frame may omit them); None when its tables are not the Annex K ones."""
    info = J.parse_jpeg(data)
    if info.huff != J._STD_HUFF:
        return None
    out, pos = bytearray(data[:2]), 2
    while data[pos + 1] != 0xDA:
        n = struct.unpack_from(">H", data, pos + 2)[0]
        if data[pos + 1] != 0xC4:
            out += data[pos:pos + 2 + n]
        pos += 2 + n
    return bytes(out + data[pos:])


def _bits(pairs):
    bw = _BitWriter()
    for code, length in pairs:
        bw.put(code, length)
    return bw.finish()


class _BitWriter:
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


def _with_scan(data, scan):
    info = J.parse_jpeg(data)
    return data[:info.scan[0]] + scan


def _set_dri(data, ri):
    i = data.index(b"\xff\xdd\x00\x04")
    return data[:i + 4] + struct.pack(">H", ri) + data[i + 6:]


@functools.lru_cache(maxsize=None)
def damaged_files():
    """name -> a file whose header is good (``parse_jpeg`` routes it to the device) and whose scan is damaged: the reference decoder raises
    for every one of them (asserted in tests/test_jpegdec_cpu.py), and the device must leave a code.  The same bytes go through
    tests/jpegdec_host_main.cpp under sanitizers before they go to a GPU."""
    out = {}
    plain = pil_file("smooth", 97, 131, "420", 90)                      # Annex K tables, no DRI
    rows = pil_file("smooth", 97, 131, "420", 90, 1)                    # one interval per MCU row: 7 intervals
    grey = pil_file("noise", 17, 33, "grey", 90)
    ip, ir = J.parse_jpeg(plain), J.parse_jpeg(rows)
    sp, sr = plain[ip.scan[0]:ip.scan[0] + ip.scan[1]], rows[ir.scan[0]:ir.scan[0] + ir.scan[1]]
    for name, cut in (("cut_quarter", len(sp) // 4), ("cut_half", len(sp) // 2), ("cut_tail3", len(sp) - 3), ("cut_all", 0), ("cut_one", 1)):
        out[name] = _with_scan(plain, sp[:cut])
    out["cut_rows_half"] = _with_scan(rows, sr[:len(sr) // 2])
    out["trailing_ff"] = _with_scan(plain, sp[:len(sp) // 3] + b"\xff")
    # a flipped byte: the first position (from the middle on) at which the reference decoder meets an error
    for name, data, info in (("flip_plain", plain, ip), ("flip_rows", rows, ir), ("flip_grey", grey, J.parse_jpeg(grey))):
        s0, n = info.scan
        for at in range(n // 2, n - 2):
            if data[s0 + at] in (0xFF, 0x00) or data[s0 + at - 1] == 0xFF:
                continue
            bad = data[:s0 + at] + bytes([data[s0 + at] ^ 0x5A]) + data[s0 + at + 1:]
            bi = J.parse_jpeg(bad)
            if bi.route != "gpu":
                continue
            try:
                entropy_decode(bi, bad)
            except RefError:
                out[name] = bad
                break
    # nine 1-bits are no code of the Annex K luma DC table
    out["bad_code"] = _with_scan(plain, b"\xff\x00\xff\x00\xff\x00" + b"\xff\xd9")
    # DC category 0, three ZRL (k = 49), then (run 15, size 1): index 64
    dc, ac = M.huffman_codes(*M.DC_LUMA), M.huffman_codes(*M.AC_LUMA)
    out["run_past_63"] = _with_scan(plain, _bits([dc[0], ac[0xF0], ac[0xF0], ac[0xF0], ac[0xF1], (1, 1)]) + bytes(16) + b"\xff\xd9")
    i = sr.index(b"\xff\xd2")
    out["missing_rst"] = _with_scan(rows, sr[:i] + sr[i + 2:])
    j = sr.index(b"\xff\xd4")
    out["rst_out_of_order"] = _with_scan(rows, sr[:i] + b"\xff\xd4" + sr[i + 2:j] + b"\xff\xd2" + sr[j + 2:])
    out["rst_repeated"] = _with_scan(rows, sr[:i] + b"\xff\xd1" + sr[i + 2:])
    out["dri_larger_than_data"] = _set_dri(rows, 0xFFFF)
    out["dri_smaller"] = _set_dri(rows, 1)
    out["rst_without_dri"] = rows.replace(b"\xff\xdd\x00\x04" + rows[rows.index(b"\xff\xdd") + 4:rows.index(b"\xff\xdd") + 6], b"")
    return out


DAMAGED_CODES = {"bad_code": E_BAD_CODE, "run_past_63": E_INDEX, "missing_rst": E_RST_COUNT, "rst_out_of_order": E_RST_ORDER, "rst_repeated": E_RST_ORDER,
                 "dri_larger_than_data": E_RST_COUNT, "dri_smaller": E_RST_COUNT, "rst_without_dri": E_RST_COUNT, "cut_rows_half": E_RST_COUNT,
                 "cut_all": E_TRUNCATED, "cut_one": E_TRUNCATED}
