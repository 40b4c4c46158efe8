"""PNG files from device-resident uint8 images, encoded on the GPU (reface_amd/csrc/pngenc.hip; the CLIs' ``--gpu_png``).

The device leaves one finished zlib stream per image -- rf_png_filter_u8 (row filters), rf_png_deflate_segments (32768-byte segments, one
dynamic Huffman block each over Z_RLE-style tokens), rf_png_pack (segments back to back, Adler-32) -- and the host copies only the
compressed bytes and wraps them in the PNG signature, IHDR, one IDAT and IEND (the chunk CRC-32 is zlib.crc32 over the compressed bytes).
PNG is lossless: the files decode to exactly the input pixels; their bytes differ from PIL's.

``PngEncoder.encode_async`` enqueues the three kernels on the current stream, records an event and returns at once; ``PngJob.result()``
-- meant for a writer thread -- waits for the event, reads the lengths and copies the streams through pinned memory on the encoder's own
copy stream.  The launch thread never waits for an encode.
"""
import struct
import threading
import zlib

import torch

from . import _lib, ops

SEG = 32768          # RF_PNG_SEG
SLOT = 32784         # RF_PNG_SLOT
PNG_SIG = b"\x89PNG\r\n\x1a\n"
COLOR_TYPE = {1: 0, 3: 2, 4: 6}          # channels -> PNG colour type (grey, RGB, RGBA), 8 bits per sample


def _up16(n):
    return (n + 15) // 16 * 16


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)) & 0xFFFFFFFF)


def wrap_png(zstream, H, W, C):
    """The PNG file around one zlib stream of the filtered rows."""
    ihdr = struct.pack(">IIBBBBB", W, H, 8, COLOR_TYPE[C], 0, 0, 0)
    return b"".join((PNG_SIG, _chunk(b"IHDR", ihdr), _chunk(b"IDAT", zstream), _chunk(b"IEND", b"")))


class _Scratch:
    """Device and pinned buffers of one in-flight encode of B streams of n bytes, sized from the worst case (every segment stored: bytes + 5).
    Per stream that is ~3 n bytes of device memory and, with `pinned`, n bytes of pinned host memory (a 1080p RGBA frame: 25 MB + 8.3 MB)."""

    def __init__(self, B, n, device, pinned=True):
        self.B, self.n = B, n
        self.nseg = (n + SEG - 1) // SEG
        self.fstride = _up16(n)
        self.ostride = _up16(n + 5 * self.nseg + 6)
        u8 = dict(dtype=torch.uint8, device=device)
        self.filt = torch.empty(B * self.fstride, **u8)
        self.slots = torch.empty(B * self.nseg * SLOT, **u8)
        self.seg_bytes = torch.empty(B * self.nseg, dtype=torch.int32, device=device)
        self.seg_adler = torch.empty(B * self.nseg, dtype=torch.int32, device=device)
        self.out = torch.empty((B, self.ostride), **u8)
        self.lengths = torch.empty(B, dtype=torch.int32, device=device)
        if pinned:
            self.host_lengths = torch.empty(B, dtype=torch.int32).pin_memory()
            self.host_out = torch.empty((B, self.ostride), dtype=torch.uint8).pin_memory()


def deflate_streams(streams):
    """Stages 2 and 3 on arbitrary byte streams: uint8 device tensor [B, n] (rows may be strided) -> list of B zlib streams (bytes)."""
    ops._require_gpu(streams)
    assert streams.dtype == torch.uint8 and streams.dim() == 2 and streams.stride(1) == 1 and streams.shape[1] > 0
    lib = _lib.load()
    B, n = streams.shape
    sc = _Scratch(B, n, streams.device, pinned=False)
    st = ops.stream_ptr()
    _lib.check(lib.rf_png_deflate_segments(streams.data_ptr(), B, n, streams.stride(0) if B > 1 else n, sc.slots.data_ptr(), sc.seg_bytes.data_ptr(),
                                           sc.seg_adler.data_ptr(), st), "rf_png_deflate_segments")
    _lib.check(lib.rf_png_pack(sc.slots.data_ptr(), sc.seg_bytes.data_ptr(), sc.seg_adler.data_ptr(), B, n, sc.out.data_ptr(), sc.ostride,
                               sc.lengths.data_ptr(), st), "rf_png_pack")
    lengths = sc.lengths.cpu().tolist()
    out = sc.out.cpu().numpy()
    return [out[b, :lengths[b]].tobytes() for b in range(B)]


def filter_images(images):
    """Stage 1 alone: uint8 device tensor [B, H, W, C] (rows and images may be strided) -> uint8 device tensor [B, H * (1 + W * C)]."""
    ops._require_gpu(images)
    B, H, W, C = images.shape
    assert images.dtype == torch.uint8 and images.stride(3) == 1 and (images.stride(2) == C or W == 1)
    lib = _lib.load()
    n = H * (1 + W * C)
    out = torch.empty((B, n), dtype=torch.uint8, device=images.device)
    _lib.check(lib.rf_png_filter_u8(images.data_ptr(), B, H, W, C, images.stride(0) if B > 1 else (H - 1) * images.stride(1) + W * C,
                                    images.stride(1) if H > 1 else W * C, out.data_ptr(), n, ops.stream_ptr()), "rf_png_filter_u8")
    return out


class PngJob:
    """One enqueued encode of B images; ``result()`` (any thread, once) gives the B PNG files."""

    def __init__(self, enc, sc, shape, event, keep):
        self.enc, self.sc, self.shape, self.event, self.keep = enc, sc, shape, event, keep

    def discard(self):
        """Give the scratch back without fetching anything (rate measurements)."""
        self.keep = None
        self.enc._release(self.sc)

    def result(self):
        enc, sc = self.enc, self.sc
        B, H, W, C = self.shape
        try:
            self.event.synchronize()
            with torch.cuda.device(enc.device), torch.cuda.stream(enc.copy_stream):
                sc.host_lengths.copy_(sc.lengths, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
                lengths = sc.host_lengths.tolist()
                for b in range(B):
                    sc.host_out[b, :lengths[b]].copy_(sc.out[b, :lengths[b]], non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
            host = sc.host_out.numpy()
            return [wrap_png(host[b, :lengths[b]].tobytes(), H, W, C) for b in range(B)]
        finally:
            self.keep = None
            enc._release(sc)


class PngEncoder:
    """``encode(images_u8) -> list[bytes]``: complete PNG files of uint8 device images [B, H, W, C] (C = 1, 3, 4; [H, W, C] and [B, H, W] are
    accepted), rows / images may be strided views.  Scratch is allocated once per (B, H, W, C) and in-flight encode, then reused."""

    MAX_FREE = 16

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._free, self._lock = {}, threading.Lock()
        self.copy_stream = None

    def _acquire(self, B, n):
        with self._lock:
            pool = self._free.setdefault((B, n), [])
            if pool:
                return pool.pop()
        return _Scratch(B, n, self.device)

    def _release(self, sc):
        # Scratch in use is bounded by the caller's jobs in flight (two batches in the test-bench CLI, PngWriter.depth files in the video
        # caller); of the sets that come back at most MAX_FREE per shape are kept for reuse, the rest are dropped and their memory returned.
        with self._lock:
            pool = self._free.setdefault((sc.B, sc.n), [])
            if len(pool) < self.MAX_FREE:
                pool.append(sc)

    def encode_async(self, images):
        ops._require_gpu(images)
        if images.dim() == 3:
            images = images.unsqueeze(0) if images.shape[2] in COLOR_TYPE else images.unsqueeze(3)
        B, H, W, C = images.shape
        if images.dtype != torch.uint8 or C not in COLOR_TYPE or B < 1 or H < 1 or W < 1:
            raise ValueError(f"PngEncoder: uint8 [B, H, W, C] with C in (1, 3, 4) expected, got {images.dtype} {tuple(images.shape)}")
        if images.stride(3) != 1 or (W > 1 and images.stride(2) != C):
            images = images.contiguous()
        lib = _lib.load()
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(images.device)
            self.device = images.device
        n = H * (1 + W * C)
        sc = self._acquire(B, n)
        st = torch.cuda.current_stream(images.device)
        rs = images.stride(1) if H > 1 else W * C
        istr = images.stride(0) if B > 1 else (H - 1) * rs + W * C
        _lib.check(lib.rf_png_filter_u8(images.data_ptr(), B, H, W, C, istr, rs, sc.filt.data_ptr(), sc.fstride, st.cuda_stream), "rf_png_filter_u8")
        _lib.check(lib.rf_png_deflate_segments(sc.filt.data_ptr(), B, n, sc.fstride, sc.slots.data_ptr(), sc.seg_bytes.data_ptr(), sc.seg_adler.data_ptr(),
                                               st.cuda_stream), "rf_png_deflate_segments")
        _lib.check(lib.rf_png_pack(sc.slots.data_ptr(), sc.seg_bytes.data_ptr(), sc.seg_adler.data_ptr(), B, n, sc.out.data_ptr(), sc.ostride,
                                   sc.lengths.data_ptr(), st.cuda_stream), "rf_png_pack")
        ev = torch.cuda.Event()
        ev.record(st)
        return PngJob(self, sc, (B, H, W, C), ev, images)

    def encode(self, images):
        return self.encode_async(images).result()
