"""Baseline JPEG files from device-resident uint8 images, encoded on the GPU (reface_amd/csrc/jpegenc.hip), and the Motion-JPEG AVI
container around them: the playable end of scripts/inference_swap_video.py (``--write_video``).

The device leaves the entropy-coded scan of every image -- rf_jpeg_blocks_u8 (libjpeg's integer colour transform, h2v2 downsample, "islow"
DCT and quantisation), rf_jpeg_entropy (Annex K Huffman coding, one restart interval per MCU row), rf_jpeg_pack (intervals back to back
with RSTn between them and EOI behind) -- and the host puts ``jpeg_header`` in front.  All device arithmetic is 32-bit integer, so the file
is byte for byte the one libjpeg(-turbo) writes for ``quality``, ``subsampling`` and one restart interval per MCU row (PIL:
``save(f, "JPEG", quality=Q, subsampling=S, restart_marker_rows=1)``).

``JpegEncoder.encode_async`` enqueues the three kernels on the current stream, records an event and returns; ``JpegJob.result()`` -- meant
for a writer thread -- waits for the event and copies lengths and bytes through pinned memory on the encoder's copy stream.  ``AviWriter`` is
a plain RIFF writer (``hdrl`` / ``movi`` / ``idx1``), ``VideoSink`` the one thread that appends jobs' frames in submission order, and
``VideoOutput`` the three together as the CLI uses them.  There is no audio track.  ``AviReader`` is the way back: the frames of a
Motion-JPEG AVI file as bytes, for reface_amd/jpegdec.py to decode (``--video_in``).
"""
import os
import queue
import struct
import threading

# ------------------------------------------------------------------------------------------------ tables (ITU-T T.81 Annex K), defined once
# natural (row-major) index of the coefficient at each zigzag position
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# K.1 / K.2: the base quantisation tables, natural order
STD_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
STD_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# K.3 - K.6: (BITS: number of codes of length 1 .. 16, HUFFVAL: the symbols in code order)
_AC_TAIL = tuple((r << 4) | s for r in range(16) for s in range(1, 11))          # (not a table: the symbols both AC lists must hold)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
HUFF_TABLES = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)          # in the order of the DHT segments
for _bits, _vals in HUFF_TABLES:
    assert sum(_bits) == len(_vals) == len(set(_vals))
assert set(AC_LUMA[1]) == set(AC_CHROMA[1]) == set(_AC_TAIL) | {0x00, 0xF0}

BLOCK_BITS = 64 * 27          # bound of a coded block: per coefficient a code of at most 16 bits and at most 11 amplitude bits (csrc/jpegenc.hip)
SUBSAMPLINGS = ("420", "444")


def quant_tables(quality):
    """The two 64-entry tables of ``jpeg_set_quality(quality, force_baseline)``, natural order: (luma, chroma)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be 1 .. 100, got {quality}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(255, max(1, (b * scale + 50) // 100)) for b in base) for base in (STD_LUMA_Q, STD_CHROMA_Q))


def huffman_codes(bits, vals):
    """Annex C: {symbol: (code, length)} of one table."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def geometry(H, W, subsampling):
    """(MCU rows, MCUs per row, blocks per MCU) of an H x W image."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"JPEG subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG sizes are 1 .. 65535, got {H} x {W}")
    m = 16 if subsampling == "420" else 8
    return (H + m - 1) // m, (W + m - 1) // m, 6 if subsampling == "420" else 3


def _segment(marker, data):
    return struct.pack(">BBH", 0xFF, marker, len(data) + 2) + data


def jpeg_header(H, W, quality=90, subsampling="420"):
    """Everything from SOI through SOS, as libjpeg writes it: APP0 (JFIF 1.01, no density unit), DQT luma, DQT chroma, SOF0, DHT x 4,
    DRI (one restart interval per MCU row), SOS."""
    _, mcus, _ = geometry(H, W, subsampling)
    luma, chroma = quant_tables(quality)
    hv = 0x22 if subsampling == "420" else 0x11
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for i, t in enumerate((luma, chroma)):
        out.append(_segment(0xDB, bytes([i]) + bytes(t[z] for z in ZIGZAG)))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, hv, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, (bits, vals) in zip((0x00, 0x10, 0x01, 0x11), HUFF_TABLES):
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", mcus)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ the device encoder
HUFF_WORDS = 2 * 272          # RF_JPEG_HUFF_WORDS: per table class (luma, chroma) 16 DC entries then 256 AC entries, (code << 5) | length


def _up16(n):
    return (n + 15) // 16 * 16


def slot_bytes(nbr):
    """RF_JPEG_SLOT(nbr): bytes of one interval's slot, the worst case of nbr blocks with every byte stuffed, rounded up to 16."""
    return _up16(2 * ((nbr * BLOCK_BITS + 7) // 8 + 1))


def _device_tables(quality, device):
    import torch
    luma, chroma = quant_tables(quality)
    quant = torch.tensor([t[z] for t in (luma, chroma) for z in ZIGZAG], dtype=torch.int32)
    words = []
    for dc, ac in ((DC_LUMA, AC_LUMA), (DC_CHROMA, AC_CHROMA)):
        dcc, acc = huffman_codes(*dc), huffman_codes(*ac)
        words += [(dcc[s][0] << 5) | dcc[s][1] if s in dcc else 0 for s in range(16)]
        words += [(acc[s][0] << 5) | acc[s][1] if s in acc else 0 for s in range(256)]
    return quant.to(device), torch.tensor(words, dtype=torch.int32).to(device)


class _Scratch:
    """Device buffers of one in-flight encode of B images, sized from the worst case (every block BLOCK_BITS long, every byte stuffed): per
    8 x 8 block 128 bytes of coefficients and 2 x 432 bytes of slot and output (a 1080p frame at 4:2:0: 49 MB).  The pinned host buffer
    is sized from the lengths the device reports and grows on demand."""

    def __init__(self, B, H, W, subsampling, device):
        import torch
        self.key = (B, H, W, subsampling)
        self.mrows, self.mcus, self.bpm = geometry(H, W, subsampling)
        self.nbr = self.mcus * self.bpm
        self.slot = slot_bytes(self.nbr)
        self.ostride = _up16(self.mrows * (self.slot + 2))
        if self.ostride >= 1 << 31:
            raise ValueError(f"JpegEncoder: the worst-case scan of a {H} x {W} image ({self.ostride} bytes) is past 2^31; encode it in tiles")
        self.coef = torch.empty(B * self.mrows * 64 * self.nbr, dtype=torch.int16, device=device)
        self.slots = torch.empty(B * self.mrows * self.slot, dtype=torch.uint8, device=device)
        self.seg_bytes = torch.empty(B * self.mrows, dtype=torch.int32, device=device)
        self.out = torch.empty((B, self.ostride), dtype=torch.uint8, device=device)
        self.lengths = torch.empty(B, dtype=torch.int32, device=device)
        self.host_lengths = torch.empty(B, dtype=torch.int32).pin_memory()
        self.host_out = None


def _as_batch(images, who):
    import torch
    if images.dim() == 3:
        images = images.unsqueeze(0)
    if images.dim() != 4 or images.dtype != torch.uint8 or images.shape[3] not in (3, 4) or min(images.shape) < 1:
        raise ValueError(f"{who}: uint8 [B, H, W, C] with C in (3, 4) expected, got {images.dtype} {tuple(images.shape)}")
    B, H, W, C = images.shape
    if images.stride(3) != 1 or (W > 1 and images.stride(2) != C):
        images = images.contiguous()
    rs = images.stride(1) if H > 1 else W * C
    istr = images.stride(0) if B > 1 else (H - 1) * rs + W * C
    return images, rs, istr


def _launch_blocks(lib, images, rs, istr, sc, quant, sub, st):
    from . import _lib
    B, H, W, C = images.shape
    _lib.check(lib.rf_jpeg_blocks_u8(images.data_ptr(), B, H, W, C, istr, rs, int(sub), quant.data_ptr(), sc.coef.data_ptr(), st), "rf_jpeg_blocks_u8")


def coefficients(images, quality=90, subsampling="420"):
    """Stage 1 alone: uint8 device images [B, H, W, 3 | 4] -> int16 device tensor [B, MCU rows, blocks per MCU row, 64]: the quantised
    coefficients in zigzag order, blocks in the scan's order (per MCU: Y00 Y01 Y10 Y11 Cb Cr at 4:2:0, Y Cb Cr at 4:4:4)."""
    from . import _lib, ops
    ops._require_gpu(images)
    images, rs, istr = _as_batch(images, "coefficients")
    B, H, W, _ = images.shape
    sc = _Scratch(B, H, W, subsampling, images.device)
    quant, _ = _device_tables(quality, images.device)
    _launch_blocks(_lib.load(), images, rs, istr, sc, quant, subsampling, ops.stream_ptr())
    return sc.coef.view(B, sc.mrows, 64, sc.nbr).permute(0, 1, 3, 2).contiguous()


class JpegJob:
    """One enqueued encode of B images; ``result()`` (any thread, once) gives the B JPEG files."""

    def __init__(self, enc, sc, shape, event, keep):
        self.enc, self.sc, self.shape, self.event, self.keep = enc, sc, shape, event, keep

    def discard(self):
        """Give the scratch back without fetching anything (rate measurements)."""
        self.keep = None
        self.enc._release(self.sc)

    def result(self):
        import torch
        enc, sc = self.enc, self.sc
        B, H, W, _ = self.shape
        try:
            self.event.synchronize()
            with torch.cuda.device(enc.device), torch.cuda.stream(enc.copy_stream):
                sc.host_lengths.copy_(sc.lengths, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
                lengths = sc.host_lengths.tolist()
                offs = [0]
                for n in lengths:
                    offs.append(offs[-1] + _up16(n))
                if sc.host_out is None or sc.host_out.numel() < offs[-1]:
                    sc.host_out = torch.empty(max(offs[-1] * 5 // 4, 1 << 16), dtype=torch.uint8).pin_memory()
                for b in range(B):
                    sc.host_out[offs[b]:offs[b] + lengths[b]].copy_(sc.out[b, :lengths[b]], non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
            host = sc.host_out.numpy()
            head = jpeg_header(H, W, enc.quality, enc.subsampling)
            return [head + host[offs[b]:offs[b] + lengths[b]].tobytes() for b in range(B)]
        finally:
            self.keep = None
            enc._release(sc)


class JpegEncoder:
    """``encode(images_u8) -> list[bytes]``: complete baseline JPEG files of uint8 device images [B, H, W, C] (C = 3, or 4 with the alpha
    byte ignored; [H, W, C] is accepted), rows / images may be strided views.  Scratch is allocated once per (B, H, W) and in-flight
    encode, then reused."""

    MAX_FREE = 8

    def __init__(self, device="cuda", quality=90, subsampling="420"):
        import torch
        self.device = torch.device(device)
        quant_tables(quality)
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f"JPEG subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
        self.quality, self.subsampling = int(quality), subsampling
        self._free, self._lock = {}, threading.Lock()
        self.copy_stream = None
        self._tables = None

    def _acquire(self, key):
        with self._lock:
            pool = self._free.setdefault(key, [])
            if pool:
                return pool.pop()
        return _Scratch(*key, self.device)

    def _release(self, sc):
        with self._lock:
            pool = self._free.setdefault(sc.key, [])
            if len(pool) < self.MAX_FREE:
                pool.append(sc)

    def encode_async(self, images):
        import torch
        from . import _lib, ops
        ops._require_gpu(images)
        images, rs, istr = _as_batch(images, "JpegEncoder")
        B, H, W, C = images.shape
        geometry(H, W, self.subsampling)
        lib = _lib.load()
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(images.device)
            self.device = images.device
        if self._tables is None:
            self._tables = _device_tables(self.quality, images.device)
        quant, huff = self._tables
        sc = self._acquire((B, H, W, self.subsampling))
        st = torch.cuda.current_stream(images.device)
        sub = int(self.subsampling)
        _launch_blocks(lib, images, rs, istr, sc, quant, sub, st.cuda_stream)
        _lib.check(lib.rf_jpeg_entropy(sc.coef.data_ptr(), B, sc.mrows, sc.mcus, sub, huff.data_ptr(), sc.slots.data_ptr(), sc.slot,
                                       sc.seg_bytes.data_ptr(), st.cuda_stream), "rf_jpeg_entropy")
        _lib.check(lib.rf_jpeg_pack(sc.slots.data_ptr(), sc.slot, sc.seg_bytes.data_ptr(), B, sc.mrows, sc.out.data_ptr(), sc.ostride,
                                    sc.lengths.data_ptr(), st.cuda_stream), "rf_jpeg_pack")
        ev = torch.cuda.Event()
        ev.record(st)
        return JpegJob(self, sc, (B, H, W, C), ev, images)

    def encode(self, images):
        return self.encode_async(images).result()


# ------------------------------------------------------------------------------------------------ the container
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))          # the bytes of LIST hdrl behind its size field
_MOVI_AT = 12 + 8 + _HDRL          # file offset of LIST movi


class AviWriter:
    """Motion-JPEG in a RIFF ``AVI `` file: ``add(jpeg_bytes)`` in frame order, ``close() -> [(path, n_frames), ...]``.  Before a frame would
    push the file past `max_bytes` (a RIFF size is 32 bits; many readers stop at 2 GB) the file is closed and the frames continue in
    ``<stem>.002.avi``, ``<stem>.003.avi``, ...  Counts and sizes are patched when a file is closed."""

    def __init__(self, path, width, height, fps, max_bytes=0x7F000000):
        if not (fps > 0 and width > 0 and height > 0):
            raise ValueError(f"AviWriter: width, height and fps must be positive, got {width} x {height} at {fps}")
        self.path, self.width, self.height, self.fps, self.max_bytes = str(path), int(width), int(height), float(fps), int(max_bytes)
        self.rate, self.scale = int(round(self.fps * 1000)), 1000
        self.files, self.f, self.part = [], None, 0
        self._open()

    def _part_path(self):
        if self.part == 1:
            return self.path
        stem, ext = os.path.splitext(self.path)
        return f"{stem}.{self.part:03d}{ext or '.avi'}"

    def _header(self, n, total, largest):
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), int(largest * self.rate / self.scale) if n else 0, 0, AVIF_HASINDEX, n, 0, 1, largest,
                           self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, largest, 0xFFFFFFFF, 0, 0, 0,
                           self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        assert len(hdrl) == _HDRL
        return b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl

    def _open(self):
        self.part += 1
        self.cur = self._part_path()
        self.f = open(self.cur, "wb")
        self.f.write(b"\0" * _MOVI_AT)          # RIFF and hdrl: written by _finish, when the counts are known
        self.f.write(b"LIST\0\0\0\0movi")
        self.index, self.pos, self.largest = [], _MOVI_AT + 12, 0

    def _finish(self):
        f, n = self.f, len(self.index)
        movi_size = self.pos - (_MOVI_AT + 8)
        f.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size) for off, size in self.index))
        total = self.pos + 8 + 16 * n
        f.seek(0)
        f.write(self._header(n, total, self.largest))
        f.seek(_MOVI_AT + 4)
        f.write(struct.pack("<I", movi_size))
        f.close()
        self.f = None
        self.files.append((self.cur, n))

    def add(self, jpeg):
        if self.f is None:
            raise ValueError("AviWriter.add after close")
        size = len(jpeg)
        padded = size + (size & 1)
        if self.index and self.pos + 8 + padded + 8 + 16 * (len(self.index) + 1) > self.max_bytes:
            self._finish()
            self._open()
        self.f.write(b"00dc" + struct.pack("<I", size) + jpeg + (b"\0" if size & 1 else b""))
        self.index.append((self.pos - (_MOVI_AT + 8), size))          # relative to the `movi` tag
        self.pos += 8 + padded
        self.largest = max(self.largest, size)

    def close(self):
        if self.f is not None:
            self._finish()
        return list(self.files)


class AviReader:
    """The frames of a Motion-JPEG RIFF ``AVI `` file, as ``AviWriter`` (or any other muxer) writes them: ``width``, ``height``, ``fps`` (=
    ``rate`` / ``scale`` of the video stream header), ``len()``, ``frame(i) -> bytes`` and iteration.  The frames are the ``00dc`` / ``00db``
    chunks of ``LIST movi`` in file order (``LIST rec `` groups are entered); ``idx1`` is only a cross-check.  ``AviWriter``'s continuation
    parts (``<stem>.002.avi``, ...) are followed.  Every offset is checked against the file size; a malformed file raises ``ValueError``
    naming the file and the offset, and so does any codec other than MJPG."""

    def __init__(self, path):
        self.path = str(path)
        self.parts, self._open = [], {}
        head = self._parse(self.path)
        self.width, self.height, self.rate, self.scale = head["width"], head["height"], head["rate"], head["scale"]
        self.fps = self.rate / self.scale
        self.parts.append((self.path, head["frames"]))
        stem, ext = os.path.splitext(self.path)
        k = 2
        while os.path.exists(f"{stem}.{k:03d}{ext or '.avi'}"):
            part = f"{stem}.{k:03d}{ext or '.avi'}"
            h = self._parse(part)
            if (h["width"], h["height"], h["rate"], h["scale"]) != (self.width, self.height, self.rate, self.scale):
                raise ValueError(f"{part}: at offset 0: its size or rate is not that of {self.path}")
            self.parts.append((part, h["frames"]))
            k += 1
        self._starts = [0]
        for _, frames in self.parts:
            self._starts.append(self._starts[-1] + len(frames))

    @staticmethod
    def _parse(path):
        size = os.path.getsize(path)

        def bad(off, what):
            return ValueError(f"{path}: at offset {off}: {what}")

        with open(path, "rb") as f:
            def header(off, end):
                if off + 8 > end:
                    raise bad(off, "truncated chunk header")
                f.seek(off)
                cc, n = struct.unpack("<4sI", f.read(8))
                if off + 8 + n > end:
                    raise bad(off, f"chunk {cc!r} of {n} bytes runs past its parent (which ends at {end})")
                return cc, n

            def body(off, n):
                f.seek(off)
                return f.read(n)

            if size < 12:
                raise bad(0, "not a RIFF AVI file")
            riff, n, kind = struct.unpack("<4sI4s", body(0, 12))
            if riff != b"RIFF" or kind != b"AVI ":
                raise bad(0, "not a RIFF AVI file")
            if 8 + n > size:
                raise bad(4, f"the RIFF size {n} runs past the file's {size} bytes")
            end = 8 + n
            avih = strh = strf = movi = idx1 = None
            off = 12
            while off + 8 <= end:
                cc, n = header(off, end)
                if cc == b"LIST":
                    if n < 4:
                        raise bad(off, "LIST without a type")
                    kind = body(off + 8, 4)
                    if kind == b"hdrl":
                        p, hend, in_strl = off + 12, off + 8 + n, None
                        while p + 8 <= hend:
                            c2, n2 = header(p, hend)
                            if c2 == b"avih":
                                if n2 < 56:
                                    raise bad(p, "avih is shorter than 56 bytes")
                                avih = struct.unpack("<14I", body(p + 8, 56))
                            elif c2 == b"LIST" and n2 >= 4 and body(p + 8, 4) == b"strl":
                                q, send, sh, sf = p + 12, p + 8 + n2, None, None
                                while q + 8 <= send:
                                    c3, n3 = header(q, send)
                                    if c3 == b"strh":
                                        if n3 < 48:
                                            raise bad(q, "strh is shorter than 48 bytes")
                                        sh = struct.unpack("<4s4sIHHIIIIIIII", body(q + 8, 48))
                                    elif c3 == b"strf" and n3 >= 40:
                                        sf = struct.unpack("<IiiHH4sIiiII", body(q + 8, 40))
                                    q += 8 + n3 + (n3 & 1)
                                if sh is not None and sh[0] == b"vids" and strh is None:
                                    if sf is None:
                                        raise bad(p, "the video stream has no strf")
                                    strh, strf = sh, sf
                            p += 8 + n2 + (n2 & 1)
                    elif kind == b"movi" and movi is None:
                        movi = (off + 8, off + 8 + n)          # the `movi` tag, the list's end
                elif cc == b"idx1":
                    idx1 = (off + 8, n)
                off += 8 + n + (n & 1)
            if avih is None or strh is None:
                raise bad(12, "no avih or no video stream header")
            if movi is None:
                raise bad(12, "no LIST movi")
            codec = strf[5]
            if codec.upper() != b"MJPG" or strh[1].upper() not in (b"MJPG", b"\0\0\0\0"):
                raise bad(12, f"the video stream's codec is {codec!r} (handler {strh[1]!r}), not MJPG: only Motion-JPEG AVI files are read")
            if strh[6] == 0 or strh[7] == 0:
                raise bad(12, "the video stream's rate or scale is 0")
            frames, stack = [], [(movi[0] + 4, movi[1])]
            while stack:
                p, pend = stack.pop()
                while p + 8 <= pend:
                    cc, n = header(p, pend)
                    if cc == b"LIST" and n >= 4 and body(p + 8, 4) == b"rec ":
                        stack.append((p + 8 + n + (n & 1), pend))
                        p, pend = p + 12, p + 8 + n
                        continue
                    if cc in (b"00dc", b"00db") and n > 0:
                        frames.append((p + 8, n))
                    p += 8 + n + (n & 1)
            if idx1 is not None:
                i0, n = idx1
                ents = [struct.unpack_from("<4sIII", e) for e in (body(i0 + 16 * k, 16) for k in range(n // 16))]
                ents = [e for e in ents if e[0] in (b"00dc", b"00db") and e[3] > 0]
                if len(ents) != len(frames):
                    raise bad(i0, f"idx1 lists {len(ents)} frames, LIST movi holds {len(frames)}")
                base = movi[0] if not ents or ents[0][2] + movi[0] + 8 == frames[0][0] else 0          # offsets from the `movi` tag, or from the file start
                for k, (e, fr) in enumerate(zip(ents, frames)):
                    if (e[2] + base + 8, e[3]) != fr:
                        raise bad(i0 + 16 * k, f"idx1 entry {k} does not point at frame {k}")
        return {"width": int(strf[1]), "height": abs(int(strf[2])), "rate": strh[7], "scale": strh[6], "frames": frames, "total_frames": avih[4]}

    def __len__(self):
        return self._starts[-1]

    def frame(self, i):
        if not 0 <= i < len(self):
            raise IndexError(f"{self.path}: frame {i} of {len(self)}")
        k = max(j for j in range(len(self.parts)) if self._starts[j] <= i)
        path, frames = self.parts[k]
        f = self._open.get(k)
        if f is None:
            f = self._open[k] = open(path, "rb")
        off, n = frames[i - self._starts[k]]
        f.seek(off)
        data = f.read(n)
        if len(data) != n:
            raise ValueError(f"{path}: at offset {off}: frame {i} is cut short")
        return data

    def __iter__(self):
        return (self.frame(i) for i in range(len(self)))

    def close(self):
        for f in self._open.values():
            f.close()
        self._open = {}


class VideoSink:
    """The ordered end of the encoder: ONE thread takes jobs (anything with ``result() -> list of JPEG files``) from a FIFO and hands their
    frames to ``add`` in submission order.  ``submit`` blocks while `depth` jobs wait; the first exception of a job or of ``add`` is kept,
    later jobs are discarded, and ``close()`` raises it."""

    def __init__(self, add, depth=4):
        self.add, self.error, self.n = add, None, 0
        self.q = queue.Queue(maxsize=int(depth))
        self.thread = threading.Thread(target=self._run, name="VideoSink", daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            try:
                if self.error is not None:
                    if hasattr(job, "discard"):
                        job.discard()
                    continue
                for frame in job.result():
                    self.add(frame)
                    self.n += 1
            except BaseException as e:          # noqa: BLE001 -- resurfaces on close()
                if self.error is None:
                    self.error = e

    def submit(self, job):
        if self.thread is None:
            raise ValueError("VideoSink.submit after close")
        self.q.put(job)

    def close(self):
        """Drain, stop the thread, raise what a job raised; returns the number of frames handed on."""
        if self.thread is not None:
            self.q.put(None)
            self.thread.join()
            self.thread = None
        if self.error is not None:
            raise self.error
        return self.n


class VideoOutput:
    """What ``--write_video`` drives: ``push(frames)`` enqueues the JPEG encode of a batch of uint8 device frames (a [B, H, W, C] tensor or a
    list of [H, W, C] tensors of one size) on the current stream and hands the batch pushed BEFORE it to the sink, so that an encode sits
    behind the next batch in the stream before a thread waits for it; ``close() -> [(path, n_frames), ...]``."""

    def __init__(self, path, fps=25.0, quality=90, subsampling="420", device="cuda", max_bytes=0x7F000000):
        self.path, self.fps, self.max_bytes = str(path), float(fps), max_bytes
        self.encoder = JpegEncoder(device, quality, subsampling)
        self.writer = self.sink = self.held = self.size = None

    def push(self, frames):
        import torch
        if not torch.is_tensor(frames):
            frames = list(frames)
            if len({tuple(f.shape) for f in frames}) != 1:
                raise ValueError(f"VideoOutput: the frames of a video must have one size, got {sorted({tuple(f.shape) for f in frames})}")
            frames = torch.stack(frames)
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        size = (int(frames.shape[1]), int(frames.shape[2]))
        if self.size is None:
            self.size = size
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            self.writer = AviWriter(self.path, size[1], size[0], self.fps, self.max_bytes)
            self.sink = VideoSink(self.writer.add)
        elif size != self.size:
            raise ValueError(f"VideoOutput: the frames of a video must have one size, got {size} after {self.size}")
        job = self.encoder.encode_async(frames)
        self.flush()
        self.held = job

    def flush(self):
        if self.held is not None:
            self.sink.submit(self.held)
            self.held = None

    def close(self):
        if self.sink is None:
            return []
        self.flush()
        try:
            self.sink.close()
        finally:
            files = self.writer.close()
        return files
