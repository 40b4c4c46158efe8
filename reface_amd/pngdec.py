"""PNG files to device-resident uint8 images, inflated and unfiltered on the GPU (reface_amd/csrc/pngdec.hip; the callers' ``--gpu_png_decode``).

The host walks the chunks (``parse_png``), concatenates the IDAT payloads of a batch into one pinned buffer and uploads it once; the device
inflates every zlib stream (``rf_png_inflate``) and undoes the row filters (``rf_png_unfilter_u8``).  The result is exactly the array PIL
gives for the file.  The device takes 8-bit grey, grey + alpha, RGB and RGBA files that are not interlaced and have no ``tRNS``; every other
file (palette, 16-bit, 1/2/4-bit, Adam7, tRNS, APNG, anything PIL would refuse, anything that is no PNG at all) is decoded by PIL on the
host, file by file, so ``decode`` gives PIL's array or PIL's exception.

Two inflate plans (``job.report[i]["plan"]``): ``"serial"``, one wave per stream, and ``"segments"``, for streams that are chains of
independently decodable pieces as ``--gpu_png`` writes them: the host lists the offsets behind every ``00 00 FF FF`` (``list_candidates``),
one wave decodes from each, and the device accepts the file only if the pieces chain up exactly; otherwise the serial plan decodes it, in the
same launch sequence, without a host round trip.

A third plan, ``"blocks"``, is an opt-in (``PngDecoder(parallel=True)``, the callers' ``--gpu_png_parallel``) for the streams every other
writer leaves, which have no such markers: zlib starts a new dynamic Huffman block every few tens of KB, so the device looks for dynamic
block headers at every bit offset, decodes from every one it finds, and accepts the file only if the chunks chain up from the stream start to
the final block and the resolved bytes have the trailer's Adler-32 (``rf_png_inflate_blocks``; reface_amd/csrc/png_blocks.h).  The plan only
accepts: a file it does not take is decoded by the serial plan in the same launch sequence, so arrays and error codes are the same.

``PngDecoder.decode_async`` enqueues everything on the current stream and returns at once; ``PngDecodeJob.result()`` waits for the event,
reads the per-file error codes and raises ``PngDecodeError`` naming the file for a damaged stream.
"""
import io
import struct
import threading
import zlib

import numpy as np
import torch

from . import _lib

PNG_SIG = b"\x89PNG\r\n\x1a\n"
SEG = 32768
DESC = 12                                   # RF_PNGDEC_DESC
BPP = {0: 1, 4: 2, 2: 3, 6: 4}              # PNG colour type -> bytes per pixel at 8 bits per sample
MARKER = b"\x00\x00\xff\xff"
MAX_WIDTH = 8192                            # rf_png_unfilter_u8 keeps one row of packed pixels in LDS (32 KiB)
MAX_HEIGHT = 1 << 20                        # rf_png_unfilter_u8 refuses more rows
PLANS = {0: "serial", 1: "segments", 2: "blocks"}          # the plan word of the status
BLOCKS_MAX_STREAM = 1 << 28                                  # longer streams are not eligible for the blocks plan: bit offsets stay below 2^31
ERRORS = {1: "the stream is truncated", 2: "bad zlib header", 3: "invalid block type", 4: "stored block length mismatch",
          5: "invalid code lengths", 6: "invalid code", 7: "distance beyond the start of the output", 8: "more data than the image holds",
          9: "less data than the image holds", 10: "Adler-32 mismatch", 11: "filter type above 4"}


class PngDecodeError(ValueError):
    """A PNG file whose stream the device refused: ``name`` is the file, ``code`` the device's error code."""

    def __init__(self, name, code):
        super().__init__(f"{name}: damaged PNG data stream (device code {code}: {ERRORS.get(code, 'unknown')})")
        self.name, self.code = name, code


class PngInfo:
    """What ``parse_png`` found.  ``route`` is ``"gpu"`` or ``"host"`` (then ``reason`` says why); ``spans`` are the (offset, length) of the
    IDAT payloads inside the file, ``n_idat`` their number."""

    def __init__(self, route, reason=None, width=0, height=0, bit_depth=0, color_type=0, interlace=0, spans=()):
        self.route, self.reason = route, reason
        self.width, self.height, self.bit_depth, self.color_type, self.interlace = width, height, bit_depth, color_type, interlace
        self.spans = list(spans)
        self.n_idat = len(self.spans)
        self.bpp = BPP.get(color_type, 0) if bit_depth == 8 else 0

    @property
    def expect(self):
        return self.height * (1 + self.width * self.bpp)

    def idat(self, data):
        return b"".join(data[o:o + n] for o, n in self.spans)


def _host(reason, **kw):
    return PngInfo("host", reason, **kw)


def parse_png(data):
    """Walk the chunks of a PNG file.  The checks are PIL's: the signature, the CRC-32 of every chunk in front of the first IDAT (PIL does not
    check later ones), IHDR first.  IDAT chunks must follow each other directly -- PIL stops reading image data at the first other chunk.
    Whatever the device path does not take, and whatever PIL would refuse, is routed to the host, where PIL decides."""
    if len(data) < 8 or data[:8] != PNG_SIG:
        return _host("not a PNG file")
    pos, n = 8, len(data)
    ihdr, spans, seen_other_after_idat = None, [], False
    while True:
        if pos + 8 > n:
            return _host("truncated file")
        length, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = pos + 8
        if body + length + 4 > n:
            return _host("truncated file")
        if not spans and tag != b"IDAT":
            if zlib.crc32(data[pos + 4:body + length]) & 0xFFFFFFFF != struct.unpack(">I", data[body + length:body + length + 4])[0]:
                return _host(f"bad CRC in {tag!r}")
        if ihdr is None:
            if tag != b"IHDR" or length != 13:
                return _host("IHDR is not the first chunk")
            ihdr = struct.unpack(">IIBBBBB", data[body:body + 13])
        elif tag == b"IDAT":
            if seen_other_after_idat:
                return _host("IDAT chunks are not consecutive")
            spans.append((body, length))
        elif tag == b"IEND":
            break
        else:
            if tag in (b"tRNS", b"PLTE", b"acTL", b"fcTL", b"fdAT", b"IHDR"):
                return _host(f"{tag.decode()} chunk")
            if spans:
                seen_other_after_idat = True
        pos = body + length + 4
    w, h, depth, ctype, comp, filt, lace = ihdr
    kw = dict(width=w, height=h, bit_depth=depth, color_type=ctype, interlace=lace, spans=spans)
    if not spans:
        return _host("no IDAT", **kw)
    if w < 1 or h < 1 or comp != 0 or filt != 0:
        return _host("unsupported IHDR", **kw)
    if depth != 8 or ctype not in BPP:
        return _host(f"bit depth {depth}, colour type {ctype}", **kw)
    if lace != 0:
        return _host("interlaced", **kw)
    info = PngInfo("gpu", **kw)
    if w > MAX_WIDTH or h > MAX_HEIGHT or info.expect >= 2 ** 31 or sum(s[1] for s in spans) >= 2 ** 31:
        return _host("image too large for the device path", **kw)
    return info


def list_candidates(z):
    """The offsets in a zlib stream at which a piece of the segmented plan may start: behind every ``00 00 FF FF`` (the empty stored block that
    ends a segment of the GPU encoder's streams, or of any stream flushed with Z_SYNC_FLUSH / Z_FULL_FLUSH), and behind a non-final stored
    block of 32768 bytes that starts at the stream start or at such an offset (the encoder's stored segments carry no marker).  Hints only:
    the device checks every one."""
    out = set()
    i = z.find(MARKER, 2)
    while i >= 0:
        out.add(i + 4)
        i = z.find(MARKER, i + 1)
    for s in [2] + sorted(out):
        while s + 5 <= len(z) and (z[s] & 7) == 0 and z[s + 1:s + 5] == b"\x00\x80\xff\x7f" and s + 5 + SEG <= len(z):
            s += 5 + SEG
            if s in out:
                break
            out.add(s)
    return sorted(o for o in out if o <= len(z))


def counts_line(decoder, what="files"):
    """The line the callers print (on stderr) behind --gpu_png_decode."""
    return f"gpu_png_decode: {decoder.counts['gpu']} {what} decoded on the device, {decoder.counts['host']} on the host"


def _check_block_bytes(block_bytes):
    if int(block_bytes) != block_bytes or not 16 <= block_bytes <= 1 << 20:
        raise ValueError(f"PngDecoder: block_bytes must be an integer in 16 .. 2^20, got {block_bytes!r}")
    return int(block_bytes)


def _up16(n):
    return (n + 15) // 16 * 16


def _out_channels(bpp, mode):
    """Channels the device writes for a file of `bpp` bytes per pixel under `mode`, or None where the conversion is not an index operation."""
    if mode is None:
        return bpp
    if mode == "RGB":
        return 3
    if mode == "L":
        return 1 if bpp <= 2 else None          # RGB -> L is PIL's integer luma: left to PIL
    raise ValueError(f"PngDecoder: mode must be None, 'RGB' or 'L', got {mode!r}")


def _pil_decode(data, mode):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if mode is not None:
        im = im.convert(mode)
    a = np.asarray(im)
    if a.dtype != np.uint8:
        return torch.from_numpy(np.array(a))          # (16-bit files: PIL's own array, whatever its type)
    return torch.from_numpy(np.array(a.reshape(a.shape[0], a.shape[1], -1)))


class _Launched:
    """What ``PngDecoder._launch`` enqueued: the images (views of ``pix``), the status words, the event behind the last kernel, the staging
    buffer to give back, the tensors to keep alive, the stacked batch (or None) and the filtered streams with their offsets."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Staging:
    """One pinned host buffer: descriptors, candidates and the compressed bytes of a batch, uploaded in one copy."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.t = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.a = self.t.numpy()


class PngDecodeJob:
    """One enqueued decode; ``result()`` (any thread, once) gives the uint8 device tensors [H, W, C] in the order of the items, ``report``
    (complete after ``result()``) says per file where it was decoded and by which inflate plan."""

    def __init__(self, dec, names, outs, gpu_idx, status, event, staging, keep, report, blocks=None):
        self.dec, self.names, self.outs, self.gpu_idx, self.status, self.event = dec, names, outs, gpu_idx, status, event
        self.staging, self.keep, self.report = staging, keep, report
        self.blocks = blocks       # (the work buffer, the files' capacities) of a launch with the blocks plan on, else None
        self.batch = None          # the [B, H, W, C] tensor the images are views of, when all of them came from the device at one shape

    def discard(self):
        if self.event is not None:
            self.event.synchronize()
        self._release()

    def _release(self):
        if self.staging is not None:
            self.dec._release(self.staging)
        self.staging = self.keep = None

    def result(self):
        try:
            if self.event is not None:
                self.event.synchronize()
                st = self.status.cpu().tolist()
                fields = _block_fields(self.blocks, st)
                for k, i in enumerate(self.gpu_idx):
                    self.report[i]["plan"] = PLANS[st[2 * k + 1]]
                    self.report[i]["code"] = st[2 * k]
                    if fields is not None:
                        self.report[i].update(fields[k])
                for k, i in enumerate(self.gpu_idx):
                    if st[2 * k] != 0:
                        raise PngDecodeError(self.names[i], st[2 * k])
            return self.outs
        finally:
            self._release()


def _block_fields(blocks, st):
    """The report fields of the blocks plan, per file of a launch: the chain's length, the candidates found (candidate 0 among them) and
    whether an eligible file ended on the serial plan.  None when the plan was off."""
    if blocks is None:
        return None
    work, caps = blocks
    wk = work[:4 * len(caps)].cpu().tolist()
    return [{"chunks": wk[4 * k + 1] if st[2 * k + 1] == 2 else 0, "candidates": 1 + wk[4 * k] if c else 0, "fallback": bool(c) and st[2 * k + 1] == 0}
            for k, c in enumerate(caps)]


class PngDecoder:
    """``decode(items, mode=None) -> list of uint8 device tensors [H, W, C]``: items are paths or ``bytes``; ``mode`` in (None, "RGB", "L")
    reproduces ``Image.open(p)`` and ``.convert(mode)``.  ``parallel`` turns the blocks plan on for streams of at least ``min_bytes`` of
    output; a file has ``16 + len(stream) // block_bytes`` candidate slots and is left to the serial plan when the device finds more."""

    MAX_FREE = 4

    def __init__(self, device="cuda", parallel=False, block_bytes=1024, min_bytes=65536):
        self.device = torch.device(device)
        self.parallel = bool(parallel)
        self.block_bytes, self.min_bytes = _check_block_bytes(block_bytes), int(min_bytes)
        if self.min_bytes < 1:
            raise ValueError(f"PngDecoder: min_bytes must be at least 1, got {min_bytes}")
        self._free, self._lock = [], threading.Lock()
        self.counts = {"gpu": 0, "host": 0}          # files decoded so far, by where (the callers print them)

    # ---- pinned staging buffers, reused once the job that filled them is done
    def _acquire(self, nbytes):
        with self._lock:
            for k, s in enumerate(self._free):
                if s.nbytes >= nbytes:
                    return self._free.pop(k)
        return _Staging(max(1 << 20, 1 << (nbytes - 1).bit_length()))

    def _release(self, s):
        with self._lock:
            if len(self._free) < self.MAX_FREE:
                self._free.append(s)

    def _launch(self, streams, dims, out_cs, misalign=0, out=None, candidates=True, lengths=None, parallel=None, block_bytes=None):
        """Enqueue inflate + unfilter of zlib streams: dims[i] = (H, W, bpp).  -> _Launched.
        `out` (tests): a uint8 device tensor [B, H', W', C] with H' >= H, W' >= W whose [:, :H, :W] view receives the images.
        `lengths` (tests): the expected lengths of plain byte streams; then only the inflate stage runs and dims / out_cs are not used.
        `parallel`, `block_bytes`: overrides of the decoder's own."""
        lib = _lib.load()
        B = len(streams)
        pixels = lengths is None
        if pixels:
            lengths = [H * (1 + W * bpp) for H, W, bpp in dims]
        else:
            dims, out_cs = [(0, 0, 0)] * B, [0] * B
        cands = []
        for z, n in zip(streams, lengths):
            c = list_candidates(z) if candidates else []
            # a false candidate costs a wave: a stream with far more markers than segments is left to the serial plan
            cands.append([2] + c if c and len(c) <= 4 * (n // SEG + 2) else [])
        ncand = sum(len(c) for c in cands)
        parallel = self.parallel if parallel is None else bool(parallel)
        bb = self.block_bytes if block_bytes is None else _check_block_bytes(block_bytes)
        # the blocks plan: the capacity in candidate slots of every eligible file (0: not eligible)
        caps = [16 + len(z) // bb if parallel and n >= self.min_bytes and len(z) < BLOCKS_MAX_STREAM else 0 for z, n in zip(streams, lengths)]
        nslot = sum(caps)
        desc_bytes, cand_bytes, blk_bytes = B * DESC * 8, _up16(2 * ncand * 4), _up16((3 * B + nslot) * 4) if parallel else 0
        comp_off, o = [], desc_bytes + cand_bytes + blk_bytes
        for z in streams:
            comp_off.append(o + misalign)
            o = _up16(o + misalign + len(z))
        total = o
        filt_off, fo = [], 0
        for n in lengths:
            filt_off.append(fo)
            fo = _up16(fo + n)
        same = out is None and len({(d[0], d[1], c) for d, c in zip(dims, out_cs)}) == 1
        pix_off, rstride, po = [], [], 0
        if out is not None:
            assert out.dtype == torch.uint8 and out.is_cuda and out.dim() == 4 and out.shape[0] == B and out.stride(3) == 1 and out.stride(2) == out.shape[3]
            for b, ((H, W, bpp), c) in enumerate(zip(dims, out_cs)):
                assert out.shape[1] >= H and out.shape[2] >= W and out.shape[3] == c
                pix_off.append(b * out.stride(0))
                rstride.append(out.stride(1))
            pix_bytes = (B - 1) * out.stride(0) + (out.shape[1] - 1) * out.stride(1) + out.shape[2] * out.shape[3]
        else:
            for (H, W, bpp), c in zip(dims, out_cs):
                pix_off.append(po)
                rstride.append(W * c)
                po += H * W * c if same else _up16(H * W * c)
            pix_bytes = po
        sg = self._acquire(total)
        desc = sg.a[:desc_bytes].view(np.int64).reshape(B, DESC)
        cand = sg.a[desc_bytes:desc_bytes + 2 * ncand * 4].view(np.int32).reshape(2, ncand)
        cb = 0
        for b, (z, (H, W, bpp)) in enumerate(zip(streams, dims)):
            desc[b] = (comp_off[b] - desc_bytes - cand_bytes - blk_bytes, len(z), filt_off[b], lengths[b], H, W, bpp, out_cs[b], pix_off[b], rstride[b], cb,
                       len(cands[b]))
            cand[0, cb:cb + len(cands[b])] = b
            cand[1, cb:cb + len(cands[b])] = cands[b]
            cb += len(cands[b])
            sg.a[comp_off[b]:comp_off[b] + len(z)] = np.frombuffer(z, dtype=np.uint8)
        bm_words = 0
        if parallel:
            blk = sg.a[desc_bytes + cand_bytes:desc_bytes + cand_bytes + (3 * B + nslot) * 4].view(np.int32)
            sb = 0
            for b, (z, c) in enumerate(zip(streams, caps)):
                blk[3 * b:3 * b + 3] = (c, sb, bm_words) if c else (0, 0, 0)
                blk[3 * B + sb:3 * B + sb + c] = b
                sb += c
                bm_words += (len(z) + 3) // 4 if c else 0
        dev = self.device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            up = torch.empty(total, dtype=torch.uint8, device=dev)
            up.copy_(sg.t[:total], non_blocking=True)
            filt = torch.empty(max(fo, 16), dtype=torch.uint8, device=dev)
            slots = torch.empty(max(ncand, 1) * SEG, dtype=torch.uint8, device=dev)
            pieces = torch.empty(max(ncand, 1) * 5, dtype=torch.int32, device=dev)
            status = torch.empty(2 * B, dtype=torch.int32, device=dev)
            pix = out if out is not None else torch.empty(max(pix_bytes, 1), dtype=torch.uint8, device=dev)
            base = up.data_ptr()
            comp_ptr, comp_bytes = base + desc_bytes + cand_bytes + blk_bytes, total - desc_bytes - cand_bytes - blk_bytes
            args = (comp_ptr, comp_bytes, desc.ctypes.data, base, B, filt.data_ptr(), filt.numel(), cand.ctypes.data if ncand else None,
                    base + desc_bytes if ncand else None, ncand, slots.data_ptr(), pieces.data_ptr(), status.data_ptr())
            work = None
            if parallel:
                bitmap = torch.empty(max(bm_words, 1), dtype=torch.int32, device=dev)
                work = torch.empty(4 * B + 11 * nslot, dtype=torch.int32, device=dev)
                marks = torch.empty(filt.numel() if nslot else 1, dtype=torch.int16, device=dev)          # 2 bytes per output byte
                _lib.check(lib.rf_png_inflate_blocks(*args, blk.ctypes.data, base + desc_bytes + cand_bytes, nslot, bitmap.data_ptr(), bitmap.numel(),
                                                     work.data_ptr(), work.numel(), marks.data_ptr(), marks.numel(), st.cuda_stream), "rf_png_inflate_blocks")
            else:
                bitmap = marks = None
                _lib.check(lib.rf_png_inflate(*args, st.cuda_stream), "rf_png_inflate")
            if pixels:
                _lib.check(lib.rf_png_unfilter_u8(filt.data_ptr(), filt.numel(), desc.ctypes.data, base, B, pix.data_ptr(), pix_bytes, status.data_ptr(),
                                                  st.cuda_stream), "rf_png_unfilter_u8")
            ev = torch.cuda.Event()
            ev.record(st)
        images, batch = None, None
        if out is not None:
            images = [out[b, :d[0], :d[1]] for b, d in enumerate(dims)]
        elif pixels:
            images = [pix[pix_off[b]:pix_off[b] + d[0] * d[1] * c].view(d[0], d[1], c) for b, (d, c) in enumerate(zip(dims, out_cs))]
            batch = pix.view(B, dims[0][0], dims[0][1], out_cs[0]) if same else None
        return _Launched(images=images, status=status, event=ev, staging=sg, keep=(up, filt, slots, pieces, pix, bitmap, work, marks), batch=batch, filt=filt,
                         filt_off=filt_off, blocks=(work, caps) if parallel else None)

    def decode_async(self, items, mode=None):
        names, datas = [], []
        for k, it in enumerate(items):
            if torch.is_tensor(it):          # decoded on the host already (ByteFolder's workers): passed through
                names.append(f"<tensor #{k}>")
                datas.append(it)
            elif isinstance(it, (bytes, bytearray, memoryview)):
                names.append(f"<bytes #{k}>")
                datas.append(bytes(it))
            else:
                names.append(str(it))
                with open(it, "rb") as f:
                    datas.append(f.read())
        outs, report, gpu_idx, streams, dims, out_cs = [None] * len(datas), [], [], [], [], []
        for i, data in enumerate(datas):
            if torch.is_tensor(data):
                report.append({"where": "host", "plan": None, "reason": "decoded by the loader", "n_idat": 0})
                outs[i] = (data if data.dim() == 3 else data.unsqueeze(2)).to(self.device, non_blocking=False)
                continue
            info = parse_png(data)
            oc = _out_channels(info.bpp, mode) if info.route == "gpu" else None
            if info.route == "gpu" and oc is None:
                info = _host(f"{mode} from {info.bpp} bytes per pixel is not an index operation")
            report.append({"where": info.route, "plan": None, "reason": info.reason, "n_idat": info.n_idat})
            if info.route == "gpu":
                gpu_idx.append(i)
                streams.append(info.idat(data))
                dims.append((info.height, info.width, info.bpp))
                out_cs.append(oc)
            else:
                outs[i] = _pil_decode(data, mode).to(self.device, non_blocking=False)
        for r in report:
            self.counts[r["where"]] += 1
        if not gpu_idx:
            return PngDecodeJob(self, names, outs, [], None, None, None, None, report)
        L = self._launch(streams, dims, out_cs)
        for k, i in enumerate(gpu_idx):
            outs[i] = L.images[k]
        job = PngDecodeJob(self, names, outs, gpu_idx, L.status, L.event, L.staging, L.keep, report, L.blocks)
        job.batch = L.batch if len(gpu_idx) == len(datas) else None
        return job

    def decode(self, items, mode=None):
        return self.decode_async(items, mode).result()

    # ---- the two stages alone (tests, tools/pngdec_rate.py)
    def inflate(self, streams, lengths, misalign=0, check=True, parallel=None, block_bytes=None):
        """zlib streams of the given output lengths -> (list of uint8 device tensors, report).  `misalign` shifts every stream off its
        16-byte aligned place in the upload.  A damaged stream raises PngDecodeError naming its index, or, with check=False, only leaves
        its error code in the report.  `parallel` and `block_bytes` override the decoder's own (tests, tools/pngdec_rate.py)."""
        L = self._launch([bytes(z) for z in streams], None, None, misalign=misalign, lengths=list(lengths), parallel=parallel, block_bytes=block_bytes)
        filt, filt_off = L.filt, L.filt_off
        try:
            L.event.synchronize()
            st = L.status.cpu().tolist()
            fields = _block_fields(L.blocks, st)
        finally:
            self._release(L.staging)
        report = [{"where": "gpu", "plan": PLANS[st[2 * k + 1]], "code": st[2 * k]} for k in range(len(streams))]
        for k, r in enumerate(report if fields is not None else ()):
            r.update(fields[k])
        for k in range(len(streams)):
            if check and st[2 * k] != 0:
                raise PngDecodeError(f"<stream #{k}>", st[2 * k])
        return [filt[filt_off[k]:filt_off[k] + lengths[k]] for k in range(len(streams))], report

    def unfilter(self, filtered, dims, out=None):
        """Filtered streams (bytes; dims[i] = (H, W, bpp)) -> uint8 device tensors [H, W, bpp]: the streams travel as stored zlib streams, so
        the inflate stage in front only copies them."""
        streams = [stored_stream(bytes(f)) for f in filtered]
        L = self._launch(streams, dims, [d[2] for d in dims], out=out, candidates=False)
        images = L.images
        try:
            L.event.synchronize()
            st = L.status.cpu().tolist()
        finally:
            self._release(L.staging)
        for k in range(len(streams)):
            if st[2 * k] != 0:
                raise PngDecodeError(f"<stream #{k}>", st[2 * k])
        return images


class ByteFolder(torch.utils.data.Dataset):
    """The files of a folder for a loader whose consumer decodes on the device: an item is the file's bytes where the decoder of the file's
    kind (``kinds``: "png" for ``PngDecoder``, "jpeg" for ``jpegdec.JpegDecoder``; ``jpegdec.FileDecoder`` says which it holds) takes the
    file on the device under this ``mode``, and PIL's array (a host tensor [H, W, C], decoded here, in the worker) where it does not.
    The decoders' ``decode_async`` accepts both kinds of item."""

    def __init__(self, files, mode=None, kinds=("png",)):
        self.files, self.mode, self.kinds = list(files), mode, tuple(kinds)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        with open(self.files[i], "rb") as f:
            data = f.read()
        if device_file(data, self.mode, self.kinds):
            return data
        return _pil_decode(data, self.mode)


def device_file(data, mode, kinds=("png",)):
    """Whether the decoder of the file's kind (by signature), if it is among `kinds`, decodes these bytes on the device under `mode`."""
    if "png" in kinds and data[:8] == PNG_SIG:
        info = parse_png(data)
        return info.route == "gpu" and _out_channels(info.bpp, mode) is not None
    if "jpeg" in kinds and data[:2] == b"\xff\xd8":
        from . import jpegdec
        return jpegdec.route(data, mode)[0].route == "gpu"
    return False


def list_collate(items):
    return list(items)


def device_batches(decoder, files, batch, num_workers, mode):
    """The files of a folder as device uint8 images, one list (or, when all of a batch came from the device at one shape, one stacked
    tensor [B, H, W, C]) per loader batch: the workers read bytes, this process decodes them on the device."""
    loader = torch.utils.data.DataLoader(ByteFolder(files, mode, getattr(decoder, "kinds", ("png",))), batch_size=batch, shuffle=False, drop_last=False, num_workers=num_workers,
                                         collate_fn=list_collate)
    for items in loader:
        job = decoder.decode_async(items, mode)
        outs = job.result()
        yield job.batch if job.batch is not None else outs


def stored_stream(raw):
    """A zlib stream of stored blocks around `raw` (level 0)."""
    co = zlib.compressobj(0)
    return co.compress(raw) + co.flush()
