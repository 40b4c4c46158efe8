"""Baseline JPEG files to device-resident uint8 images, decoded on the GPU (reface_amd/csrc/jpegdec.hip; the callers' ``--gpu_jpeg_decode``
and ``scripts/inference_swap_video.py --video_in``).

The host walks the markers (``parse_jpeg``), builds the quantisation and Huffman tables, finds the restart markers with one vectorised
byte search (``FF D0..D7`` cannot occur inside stuffed entropy data) and uploads tables, interval starts and scans of a batch in one copy
from a pooled pinned buffer; the device decodes the Huffman scan (``rf_jpeg_entropy_decode``, one lane per restart interval), runs
libjpeg's integer "islow" IDCT (``rf_jpeg_idct_u8``) and its fancy chroma upsampling and colour conversion (``rf_jpeg_upsample_rgb_u8``).
All device arithmetic is 32-bit integer and restates libjpeg's, so the result is exactly the array PIL (libjpeg-turbo) gives for the file --
with one stated exception: libjpeg's C code masks an IDCT result into its range-limit table where its SIMD code and this decoder saturate.
The two agree whenever the value in front of the clamp lies inside the table's range, which holds for any file an encoder made from pixels;
equality with PIL is claimed for such files only.

The device takes 8-bit baseline sequential Huffman files (SOF0) with one interleaved scan, 1 component (grey) or 3 (YCbCr at 4:4:4, 4:2:2
(2x1) or 4:2:0 (2x2)), with or without DRI (any restart interval), with or without DHT (an AVI ``MJPG`` frame may omit it: the Annex K
tables of ``mjpeg.py`` apply), optimised tables included, up to ``MAX_SIDE`` x ``MAX_SIDE`` pixels.  Everything else -- progressive and
every other SOFn, 12-bit, 4 components, an Adobe APP14 marker whose transform is not YCbCr, other sampling factors, several scans, DNL,
RGB to ``L``, larger images, anything that is no JPEG at all -- is decoded by PIL on the host, file by file, counted and named with a
reason (``job.report``), so ``decode`` gives PIL's array or PIL's exception.

Three plans (``job.report[i]["plan"]``): ``"intervals"``, one lane per restart interval, as the files ``JpegEncoder`` / ``--write_video``
write (one interval per MCU row) decode; ``"serial"``, one lane for the whole scan of a file without DRI; and, opt-in
(``JpegDecoder(parallel=True)``, the callers' ``--gpu_jpeg_parallel``), ``"selfsync"`` for files without DRI whose scan holds at least two
sub-sequences of ``subseq_bytes``: one lane per sub-sequence decodes from a guessed bit offset, ``sync_launches`` launches iterate the
lanes' start states to their fixed point -- which holds the serial decoder's own states (csrc/jpeg_sync.h) -- and a write pass decodes every
sub-sequence from its true state.  A file whose last launch still moved a state is decoded by the serial lane after all
(``report[i]["fallback"]``), so the pixels never depend on the settings.

``JpegDecoder.decode_async`` enqueues everything on the current stream and returns at once; ``JpegDecodeJob.result()`` waits for the
event, reads the per-file error codes and raises ``JpegDecodeError`` naming the file for a damaged scan.
"""
import struct
import threading

import numpy as np
import torch

from . import _lib
from . import mjpeg as M
from . import pngdec

DESC = 24                                   # RF_JPEGDEC_DESC
HUFF_BYTES = 912                            # sizeof(HuffTab) in csrc/jpeg_decode.h
TABLE_BYTES = 512 + 8 * HUFF_BYTES          # RF_JPEGDEC_TABLE_BYTES
MAX_SIDE = 8192                             # RF_JPEGDEC_MAX_SIDE: 128 bytes of coefficients per block, 200 MB for one 8192 x 8192 file at 4:2:0
PLANS = ("serial", "intervals", "selfsync")
SS_LANES, SS_MIN_BYTES, SS_MAX_BYTES, SS_MAX_LAUNCHES = 64, 16, 1 << 16, 16          # csrc/jpeg_sync.h
SS_SYNC, SS_SCAN, SS_WRITE, SS_DC, SS_SERIAL, SS_ALL = 1, 2, 4, 8, 16, 31           # RF_JPEGDEC_SS_*
ST_FALLBACK, ST_LAUNCHES_SHIFT = 4, 8                                               # status word 1 behind the plan
SUBSEQ_BYTES = 128                          # the defaults of the selfsync plan (the sweep)
SYNC_LAUNCHES = 4
ERRORS = {1: "the scan is truncated", 2: "invalid Huffman code", 3: "coefficient index past 63", 4: "wrong number of restart intervals",
          5: "restart markers out of order", 6: "invalid DC category", 7: "iteration cap reached"}
_ZZ = np.array(M.ZIGZAG)
_SOF_OTHER = (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF)
_STD_HUFF = {(0, 0): M.DC_LUMA, (1, 0): M.AC_LUMA, (0, 1): M.DC_CHROMA, (1, 1): M.AC_CHROMA}


class JpegDecodeError(ValueError):
    """A JPEG file whose scan the device refused: ``name`` is the file, ``code`` the device's error code."""

    def __init__(self, name, code):
        super().__init__(f"{name}: damaged JPEG scan (device code {code}: {ERRORS.get(code, 'unknown')})")
        self.name, self.code = name, code


class JpegInfo:
    """What ``parse_jpeg`` found.  ``route`` is ``"gpu"`` or ``"host"`` (then ``reason`` says why).  For a device file: ``scan`` = (offset,
    length) of the entropy-coded bytes, ``starts`` the offsets of the restart intervals in it (int32, the first is 0), ``ri`` the restart
    interval in MCUs (0: none), ``hs`` / ``vs`` the luma sampling factors, ``quant`` {id: 64 values in natural order}, ``huff`` {(class, id):
    (BITS, HUFFVAL)}, ``tq`` / ``td`` / ``ta`` the table numbers of the components, ``std_huff`` whether the file had no DHT."""

    def __init__(self, route, reason=None, **kw):
        self.route, self.reason = route, reason
        self.width = self.height = self.ncomp = self.ri = 0
        self.hs = self.vs = 1
        self.scan, self.starts, self.quant, self.huff, self.tq, self.td, self.ta, self.std_huff = (0, 0), None, {}, {}, (), (), (), False
        self.__dict__.update(kw)

    @property
    def geometry(self):
        """(MCUs per row, MCU rows, blocks per MCU)"""
        return (self.width + 8 * self.hs - 1) // (8 * self.hs), (self.height + 8 * self.vs - 1) // (8 * self.vs), 1 if self.ncomp == 1 else self.hs * self.vs + 2

    @property
    def blocks(self):
        mx, my, bpm = self.geometry
        return mx * my * bpm

    @property
    def intervals(self):
        mx, my, _ = self.geometry
        return (mx * my + self.ri - 1) // self.ri if self.ri else 1

    @property
    def subsampling(self):
        return "grey" if self.ncomp == 1 else {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[(self.hs, self.vs)]


def _host(reason, **kw):
    return JpegInfo("host", reason, **kw)


def _huff_ok(bits, vals, dc):
    """libjpeg's own checks of a DHT table (jpeg_make_d_derived_tbl): at most 256 symbols, no code past the all-ones prefix, DC symbols <= 15."""
    if sum(bits) != len(vals) or len(vals) > 256:
        return False
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if bits[length - 1] and code >= 1 << length:
            return False
        code <<= 1
    return not dc or all(v <= 15 for v in vals)


def parse_jpeg(data):
    """Walk the markers of a JPEG file up to its first scan and search the scan for markers.  Whatever the device path does not take, and
    whatever PIL would refuse, is routed to the host, where PIL decides."""
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        return _host("not a JPEG file")
    pos, sof, sos, ri, adobe, jfif, quant, huff = 2, None, None, 0, None, False, {}, {}
    while sos is None:
        while pos < n and data[pos] == 0xFF and pos + 1 < n and data[pos + 1] == 0xFF:          # fill bytes in front of a marker
            pos += 1
        if pos + 4 > n:
            return _host("truncated file")
        if data[pos] != 0xFF:
            return _host("bytes between the segments")
        m = data[pos + 1]
        if m in (0x00, 0x01, 0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            return _host(f"marker FF{m:02X} in front of the scan")
        length = struct.unpack_from(">H", data, pos + 2)[0]
        if length < 2 or pos + 2 + length > n:
            return _host("truncated file")
        seg = data[pos + 4:pos + 2 + length]
        if m == 0xDB:
            k = 0
            while k < len(seg):
                if seg[k] >> 4:
                    return _host("16-bit quantisation table")
                if (seg[k] & 15) > 3 or k + 65 > len(seg):
                    return _host("bad DQT")
                t = np.zeros(64, dtype=np.uint16)
                t[_ZZ] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=k + 1)
                quant[seg[k] & 15] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg):
                    return _host("bad DHT")
                tc, th, bits = seg[k] >> 4, seg[k] & 15, tuple(seg[k + 1:k + 17])
                vals = tuple(seg[k + 17:k + 17 + sum(bits)])
                if tc > 1 or th > 3 or not _huff_ok(bits, vals, tc == 0):
                    return _host("bad DHT")
                huff[(tc, th)] = (bits, vals)
                k += 17 + len(vals)
        elif m == 0xC0 or m in _SOF_OTHER:
            if len(seg) < 6:
                return _host("bad SOF")
            if seg[0] != 8:
                return _host(f"{seg[0]}-bit samples")
            if m != 0xC0:
                return _host("progressive (SOF2)" if m == 0xC2 else f"SOF{m - 0xC0}")
            if sof is not None or len(seg) != 6 + 3 * seg[5]:
                return _host("bad SOF")
            H, W = struct.unpack_from(">HH", seg, 1)
            sof = (H, W, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
        elif m == 0xDD:
            if len(seg) != 2:
                return _host("bad DRI")
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xDC:
            return _host("DNL marker")
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                return _host("bad SOS")
            sos = ([(seg[1 + 2 * c], seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])], tuple(seg[-3:]))
        pos += 2 + length
    if sof is None:
        return _host("no frame header in front of the scan")
    H, W, comps = sof
    kw = dict(width=W, height=H, ncomp=len(comps), ri=ri)
    if H == 0:
        return _host("DNL marker", **kw)
    if W == 0:
        return _host("bad SOF", **kw)
    if len(comps) not in (1, 3):
        return _host(f"{len(comps)} components", **kw)
    if len(comps) == 3:
        if adobe is not None and adobe != 1:
            return _host(f"Adobe APP14 transform {adobe}", **kw)
        if adobe is None and not jfif and tuple(c[0] for c in comps) == (82, 71, 66):
            return _host("RGB component ids", **kw)
    hs, vs = comps[0][1], comps[0][2]
    kw.update(hs=hs, vs=vs)
    ok = (hs, vs) == (1, 1) if len(comps) == 1 else (hs, vs) in ((1, 1), (2, 1), (2, 2)) and all((c[1], c[2]) == (1, 1) for c in comps[1:])
    if not ok:
        return _host("sampling factors " + ",".join(f"{c[1]}x{c[2]}" for c in comps), **kw)
    scomps, (ss, se, ahal) = sos
    if len(scomps) != len(comps) or [c[0] for c in scomps] != [c[0] for c in comps]:
        return _host("more than one scan", **kw)
    if (ss, se, ahal) != (0, 63, 0):
        return _host("not a full sequential scan", **kw)
    std = not huff
    if std:
        huff = dict(_STD_HUFF)
    tq, td, ta = tuple(c[3] for c in comps), tuple(c[1] for c in scomps), tuple(c[2] for c in scomps)
    if any(q not in quant for q in tq) or any((0, t) not in huff for t in td) or any((1, t) not in huff for t in ta):
        return _host("a table the scan names is missing", **kw)
    if W > MAX_SIDE or H > MAX_SIDE:
        return _host("image too large for the device path", **kw)
    # the scan: every FF that is not followed by 00 is a marker (or a fill byte)
    a = np.frombuffer(data, dtype=np.uint8)[pos:]
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, dtype=np.int64)
    mk = ff[a[ff + 1] != 0]
    is_rst = (a[mk + 1] & 0xF8) == 0xD0
    other = mk[~is_rst]
    end = len(a)
    if len(other):
        end, code = int(other[0]), int(a[other[0] + 1])
        if code != 0xD9:
            return _host("DNL marker" if code == 0xDC else "fill bytes in the scan" if code == 0xFF else "more than one scan" if code in (0xDA, 0xC4, 0xDB, 0xDD)
                         else f"marker FF{code:02X} in the scan", **kw)
    if end >= 2 ** 31:
        return _host("image too large for the device path", **kw)
    rst = mk[is_rst]
    starts = np.concatenate([np.zeros(1, dtype=np.int32), (rst[rst < end] + 2).astype(np.int32)])
    return JpegInfo("gpu", scan=(pos, end), starts=starts, quant=quant, huff=huff, tq=tq, td=td, ta=ta, std_huff=std, **kw)


def huff_table(bits, vals):
    """One HuffTab (csrc/jpeg_decode.h) as bytes: look[256] uint16, maxcode[18] int32, valoff[18] int32, vals[256] uint8."""
    look, maxcode, valoff, v = np.zeros(256, dtype=np.uint16), np.full(18, -1, dtype=np.int32), np.zeros(18, dtype=np.int32), np.zeros(256, dtype=np.uint8)
    v[:len(vals)] = vals
    code = k = 0
    for length in range(1, 17):
        cnt = bits[length - 1]
        if cnt:
            valoff[length] = k - code
            for _ in range(cnt):
                if length <= 8:
                    look[code << (8 - length):(code + 1) << (8 - length)] = (length << 8) | vals[k]
                code += 1
                k += 1
            maxcode[length] = code - 1
        code <<= 1
    return look.tobytes() + maxcode.tobytes() + valoff.tobytes() + v.tobytes()


_EMPTY_HUFF = huff_table((0,) * 16, ())
_HUFF_CACHE, _BLOCK_CACHE = {}, {}


def table_block(info):
    """The RF_JPEGDEC_TABLE_BYTES of a file: 4 quantisation tables, 4 DC and 4 AC Huffman tables (absent ones empty).  Cached by content."""
    key = (tuple((i, t.tobytes()) for i, t in sorted(info.quant.items())), tuple(sorted(info.huff.items())))
    blk = _BLOCK_CACHE.get(key)
    if blk is None:
        parts = [info.quant[i].tobytes() if i in info.quant else bytes(128) for i in range(4)]
        for tc in (0, 1):
            for th in range(4):
                t = info.huff.get((tc, th))
                if t is None:
                    parts.append(_EMPTY_HUFF)
                else:
                    if t not in _HUFF_CACHE:
                        _HUFF_CACHE[t] = huff_table(*t)
                    parts.append(_HUFF_CACHE[t])
        blk = b"".join(parts)
        assert len(blk) == TABLE_BYTES
        if len(_BLOCK_CACHE) > 256:
            _BLOCK_CACHE.clear()
        _BLOCK_CACHE[key] = blk
    return blk


def counts_line(decoder, what="files"):
    """The line the callers print (on stderr) behind --gpu_jpeg_decode."""
    return f"gpu_jpeg_decode: {decoder.counts['gpu']} {what} decoded on the device, {decoder.counts['host']} on the host"


def subseqs_of(info, subseq_bytes):
    """The sub-sequences of a device file under the selfsync plan, 0 where it keeps the plan it has (DRI, or a scan below two of them)."""
    return -(-info.scan[1] // subseq_bytes) if info.ri == 0 and info.scan[1] >= 2 * subseq_bytes else 0


def _selfsync_settings(subseq_bytes, sync_launches):
    if not SS_MIN_BYTES <= subseq_bytes <= SS_MAX_BYTES:          # (16: a symbol with its stuffing never spans a whole sub-sequence)
        raise ValueError(f"JpegDecoder: subseq_bytes must be {SS_MIN_BYTES} .. {SS_MAX_BYTES}, got {subseq_bytes}")
    if not 1 <= sync_launches <= SS_MAX_LAUNCHES:
        raise ValueError(f"JpegDecoder: sync_launches must be 1 .. {SS_MAX_LAUNCHES}, got {sync_launches}")
    return int(subseq_bytes), int(sync_launches)


def _up16(n):
    return (n + 15) // 16 * 16


def _out_channels(ncomp, mode):
    """Channels the device writes for a file of `ncomp` components under `mode`, or None where PIL does the conversion."""
    if mode is None:
        return ncomp
    if mode == "RGB":
        return 3
    if mode == "L":
        return 1 if ncomp == 1 else None          # RGB -> L is PIL's integer luma: left to PIL, as the PNG decoder leaves it
    raise ValueError(f"JpegDecoder: mode must be None, 'RGB' or 'L', got {mode!r}")


def route(data, mode):
    """(info, out channels) of a file under `mode`: info.route says where ``JpegDecoder`` decodes it."""
    info = parse_jpeg(data)
    oc = _out_channels(info.ncomp, mode) if info.route == "gpu" else None
    if info.route == "gpu" and oc is None:
        info = _host(f"{mode} from {info.ncomp} components is PIL's conversion")
    return info, oc


_pil_decode = pngdec._pil_decode


class _Launched:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _status_report(code, word, subseqs):
    """The report fields the two status words of a file give; `subseqs` > 0 for a file that was given to the selfsync plan."""
    r = {"plan": PLANS[word & 3], "code": code}
    if subseqs:
        r.update(subseqs=subseqs, launches_used=(word >> ST_LAUNCHES_SHIFT) & 255, fallback=bool(word & ST_FALLBACK))
    return r


class JpegDecodeJob:
    """One enqueued decode; ``result()`` (any thread, once) gives the uint8 device tensors [H, W, C] in the order of the items, ``report``
    (complete after ``result()``) says per file where it was decoded, by which plan and, on the host, why."""

    def __init__(self, dec, names, outs, gpu_idx, status, event, staging, keep, report, subseqs=None):
        self.dec, self.names, self.outs, self.gpu_idx, self.status, self.event = dec, names, outs, gpu_idx, status, event
        self.staging, self.keep, self.report, self.subseqs = staging, keep, report, subseqs
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
                for k, i in enumerate(self.gpu_idx):
                    self.report[i].update(_status_report(st[2 * k], st[2 * k + 1], self.subseqs[k] if self.subseqs else 0))
                for k, i in enumerate(self.gpu_idx):
                    if st[2 * k] != 0:
                        raise JpegDecodeError(self.names[i], st[2 * k])
            return self.outs
        finally:
            self._release()


class JpegDecoder:
    """``decode(items, mode=None) -> list of uint8 device tensors [H, W, C]`` (C = 1 for grey): items are paths, ``bytes`` or
    ``(name, bytes)``; ``mode`` in (None, "RGB", "L") reproduces ``Image.open(p)`` and ``.convert(mode)``.  Files of any sizes and of both
    routes may share a call.  ``parallel`` gives files without DRI the selfsync plan (``subseq_bytes`` per lane, ``sync_launches`` launches)."""

    MAX_FREE = 4
    WAVES = 1024          # lanes per wave are chosen so that a launch has about this many waves (256 CUs x 4 SIMDs) before waves fill up

    def __init__(self, device="cuda", parallel=False, subseq_bytes=SUBSEQ_BYTES, sync_launches=SYNC_LAUNCHES):
        self.parallel, (self.subseq_bytes, self.sync_launches) = bool(parallel), _selfsync_settings(subseq_bytes, sync_launches)
        self.device = torch.device(device)
        self._free, self._lock = [], threading.Lock()
        self.counts = {"gpu": 0, "host": 0}          # files decoded so far, by where (the callers print them)
        self.reasons = {}                            # host reason -> files

    # ---- pinned staging buffers, reused once the job that filled them is done
    def _acquire(self, nbytes):
        with self._lock:
            for k, s in enumerate(self._free):
                if s.nbytes >= nbytes:
                    return self._free.pop(k)
        return pngdec._Staging(max(1 << 20, 1 << (nbytes - 1).bit_length()))

    def _release(self, s):
        with self._lock:
            if len(self._free) < self.MAX_FREE:
                self._free.append(s)

    def _launch(self, datas, infos, out_cs, misalign=0, timing=False, stages=3, parallel=None, subseq_bytes=None, sync_launches=None):
        """Enqueue the decode of device-eligible files.  `misalign` (tests) shifts every scan off its 16-byte aligned place in the upload;
        `timing` records an event around every kernel; `stages` < 3 stops behind the entropy decode (1) or the IDCT (2)."""
        lib = _lib.load()
        B = len(datas)
        blocks = {}
        for info in infos:
            blocks.setdefault(table_block(info), None)
        nivl = sum(len(i.starts) for i in infos)
        desc_bytes, ivl_bytes = B * DESC * 8, _up16(2 * nivl * 4)
        o = 0
        for blk in blocks:
            blocks[blk] = o
            o += TABLE_BYTES
        scan_off = []
        for info in infos:
            scan_off.append(o + misalign)
            o = _up16(o + misalign + info.scan[1])
        comp_bytes = o
        total = desc_bytes + ivl_bytes + comp_bytes
        same = len({(i.height, i.width, c) for i, c in zip(infos, out_cs)}) == 1
        coef_off, plane_off, pix_off, cb, pb, po = [], [], [], 0, 0, 0
        for info, c in zip(infos, out_cs):
            mx, my, bpm = info.geometry
            coef_off.append(cb)
            plane_off.append(pb)
            pix_off.append(po)
            cb += mx * my * bpm
            pb += mx * my * bpm * 64
            po += info.height * info.width * c if same else _up16(info.height * info.width * c)
        sg = self._acquire(total)
        desc = sg.a[:desc_bytes].view(np.int64).reshape(B, DESC)
        ivl = sg.a[desc_bytes:desc_bytes + 2 * nivl * 4].view(np.int32).reshape(2, nivl)
        comp0 = desc_bytes + ivl_bytes
        for blk, off in blocks.items():
            sg.a[comp0 + off:comp0 + off + TABLE_BYTES] = np.frombuffer(blk, dtype=np.uint8)
        # (the per-call switches of `coefficients` and the tests, checked like the constructor's)
        L_ss, launches = _selfsync_settings(self.subseq_bytes if subseq_bytes is None else subseq_bytes, self.sync_launches if sync_launches is None else sync_launches)
        subseqs = [subseqs_of(info, L_ss) if (self.parallel if parallel is None else parallel) else 0 for info in infos]
        ib = ss = wg = 0
        pack = lambda t: sum(int(v) << (8 * c) for c, v in enumerate(t))          # noqa: E731
        for b, (data, info, c) in enumerate(zip(datas, infos, out_cs)):
            ni = len(info.starts)
            desc[b] = (scan_off[b], info.scan[1], info.height, info.width, info.ncomp, info.hs, info.vs, info.ri, coef_off[b], plane_off[b], c, pix_off[b],
                       info.width * c, blocks[table_block(info)], ib, ni, pack(info.tq), pack(info.td), pack(info.ta),
                       *((ss, subseqs[b], L_ss, wg) if subseqs[b] else (0, 0, 0, 0)), 0)
            ss += subseqs[b]
            wg += -(-subseqs[b] // SS_LANES)
            ivl[0, ib:ib + ni] = b
            ivl[1, ib:ib + ni] = info.starts
            ib += ni
            s0 = comp0 + scan_off[b]
            sg.a[s0:s0 + info.scan[1]] = np.frombuffer(data, dtype=np.uint8, count=info.scan[1], offset=info.scan[0])
        lanes = min(64, max(1, -(-nivl // self.WAVES)))
        dev = self.device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            up = torch.empty(total, dtype=torch.uint8, device=dev)
            up.copy_(sg.t[:total], non_blocking=True)
            coef = torch.empty((cb, 64), dtype=torch.int16, device=dev)
            planes = torch.empty(max(pb, 16), dtype=torch.uint8, device=dev)
            pix = torch.empty(max(po, 1), dtype=torch.uint8, device=dev)
            status = torch.empty(2 * B, dtype=torch.int32, device=dev)
            base = up.data_ptr()
            comp_ptr = base + comp0
            evs, names, keep_work = [], ["entropy_decode"], ()

            def mark():
                if timing:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record(st)
                    evs.append(e)
            mark()
            _lib.check(lib.rf_jpeg_entropy_decode(comp_ptr, comp_bytes, desc.ctypes.data, base, B, ivl.ctypes.data, base + desc_bytes, nivl, lanes,
                                                  coef.data_ptr(), cb, status.data_ptr(), st.cuda_stream), "rf_jpeg_entropy_decode")
            mark()
            if ss:          # the selfsync plan of the files the launch above left alone; one call, or its parts with an event behind each
                nwork = lib.rf_jpeg_selfsync_work_bytes(ss, wg, B)
                work = torch.empty(nwork, dtype=torch.uint8, device=dev)
                for part in ((SS_SYNC, SS_SCAN, SS_WRITE, SS_DC, SS_SERIAL) if timing else (SS_ALL,)):
                    _lib.check(lib.rf_jpeg_selfsync_decode(comp_ptr, comp_bytes, desc.ctypes.data, base, B, ivl.ctypes.data, base + desc_bytes, nivl, lanes,
                                                           launches, part, work.data_ptr(), nwork, coef.data_ptr(), cb, status.data_ptr(),
                                                           st.cuda_stream), "rf_jpeg_selfsync_decode")
                    mark()
                names += ["sync", "subseq_scan", "write", "dc_prefix", "serial_fallback"]
                keep_work = (work,)
            if stages >= 2:
                _lib.check(lib.rf_jpeg_idct_u8(coef.data_ptr(), cb, comp_ptr, comp_bytes, desc.ctypes.data, base, B, planes.data_ptr(), planes.numel(),
                                               status.data_ptr(), st.cuda_stream), "rf_jpeg_idct_u8")
                mark()
                names.append("idct")
            if stages >= 3:
                _lib.check(lib.rf_jpeg_upsample_rgb_u8(planes.data_ptr(), planes.numel(), desc.ctypes.data, base, B, pix.data_ptr(), pix.numel(),
                                                       status.data_ptr(), st.cuda_stream), "rf_jpeg_upsample_rgb_u8")
                mark()
                names.append("upsample_rgb")
            ev = torch.cuda.Event()
            ev.record(st)
        images = [pix[pix_off[b]:pix_off[b] + i.height * i.width * c].view(i.height, i.width, c) for b, (i, c) in enumerate(zip(infos, out_cs))]
        batch = pix.view(B, infos[0].height, infos[0].width, out_cs[0]) if same else None
        return _Launched(images=images, status=status, event=ev, staging=sg, keep=(up, coef, planes, pix) + keep_work, batch=batch, coef=coef,
                         coef_off=coef_off, planes=planes, plane_off=plane_off, events=evs, event_names=names, lanes=lanes, nivl=nivl, subseqs=subseqs)

    def decode_async(self, items, mode=None):
        _out_channels(1, mode)
        names, datas = [], []
        for k, it in enumerate(items):
            if torch.is_tensor(it):          # decoded on the host already (ByteFolder's workers): passed through
                names.append(f"<tensor #{k}>")
                datas.append(it)
            elif isinstance(it, (bytes, bytearray, memoryview)):
                names.append(f"<bytes #{k}>")
                datas.append(bytes(it))
            elif isinstance(it, tuple):
                names.append(str(it[0]))
                datas.append(bytes(it[1]))
            else:
                names.append(str(it))
                with open(it, "rb") as f:
                    datas.append(f.read())
        outs, report, gpu_idx, infos, out_cs = [None] * len(datas), [], [], [], []
        for i, data in enumerate(datas):
            if torch.is_tensor(data):
                report.append({"where": "host", "plan": None, "reason": "decoded by the loader"})
                outs[i] = (data if data.dim() == 3 else data.unsqueeze(2)).to(self.device, non_blocking=False)
                continue
            info, oc = route(data, mode)
            report.append({"where": info.route, "plan": None, "reason": info.reason})
            if info.route == "gpu":
                gpu_idx.append(i)
                infos.append(info)
                out_cs.append(oc)
            else:
                outs[i] = _pil_decode(data, mode).to(self.device, non_blocking=False)
        for r in report:
            self.counts[r["where"]] += 1
            if r["where"] == "host":
                self.reasons[r["reason"]] = self.reasons.get(r["reason"], 0) + 1
        if not gpu_idx:
            return JpegDecodeJob(self, names, outs, [], None, None, None, None, report)
        L = self._launch([datas[i] for i in gpu_idx], infos, out_cs)
        for k, i in enumerate(gpu_idx):
            outs[i] = L.images[k]
        job = JpegDecodeJob(self, names, outs, gpu_idx, L.status, L.event, L.staging, L.keep, report, L.subseqs)
        job.batch = L.batch if len(gpu_idx) == len(datas) else None
        return job

    def decode(self, items, mode=None):
        return self.decode_async(items, mode).result()

    # ---- the stages alone (tests, tools/jpegdec_rate.py)
    def coefficients(self, files, misalign=0, check=True, parallel=None, subseq_bytes=None, sync_launches=None):
        """Device-eligible files (bytes) -> (list of int16 device tensors [blocks, 64] in natural order, report): the entropy decode alone.
        A damaged scan raises JpegDecodeError naming its index, or, with check=False, only leaves its code in the report.  The three
        switches of the constructor may be given for this call."""
        infos = [parse_jpeg(f) for f in files]
        for k, i in enumerate(infos):
            if i.route != "gpu":
                raise ValueError(f"<file #{k}>: not a device file ({i.reason})")
        L = self._launch(files, infos, [i.ncomp for i in infos], misalign=misalign, stages=1, parallel=parallel, subseq_bytes=subseq_bytes, sync_launches=sync_launches)
        try:
            L.event.synchronize()
            st = L.status.cpu().tolist()
        finally:
            self._release(L.staging)
        report = [{"where": "gpu", **_status_report(st[2 * k], st[2 * k + 1], L.subseqs[k])} for k in range(len(files))]
        for k in range(len(files)):
            if check and st[2 * k] != 0:
                raise JpegDecodeError(f"<file #{k}>", st[2 * k])
        return [L.coef[L.coef_off[k]:L.coef_off[k] + i.blocks] for k, i in enumerate(infos)], report


# ------------------------------------------------------------------------------------------------ PNG and JPEG behind one decoder
def kind_of(data):
    """"png", "jpeg" or None, by the file's signature."""
    if data[:8] == pngdec.PNG_SIG:
        return "png"
    if data[:2] == b"\xff\xd8":
        return "jpeg"
    return None


class FileDecoder:
    """The device decoders the eval tools share (--gpu_png_decode, --gpu_jpeg_decode, or both): ``decode_async(items, mode)`` sends every
    item to the decoder of its signature; a file of a kind that is not enabled, or of neither kind, is decoded by PIL.  ``kinds`` is what
    ``pngdec.ByteFolder`` asks to know which files travel as bytes."""

    def __init__(self, device="cuda", png=False, jpeg=False, jpeg_parallel=False, png_parallel=False):
        self.device = torch.device(device)
        self.png = pngdec.PngDecoder(device, parallel=png_parallel) if png else None
        self.jpeg = JpegDecoder(device, parallel=jpeg_parallel) if jpeg else None
        self.kinds = tuple(k for k, d in (("png", self.png), ("jpeg", self.jpeg)) if d is not None)

    def lines(self, what="files"):
        """The lines the callers print (on stderr), one per enabled decoder."""
        out = [pngdec.counts_line(self.png, what)] if self.png is not None else []
        return out + ([counts_line(self.jpeg, what)] if self.jpeg is not None else [])

    def decode_async(self, items, mode=None):
        items = list(items)
        groups = {"png": [], "jpeg": []}
        for k, it in enumerate(items):
            if torch.is_tensor(it):
                kind = self.kinds[0]          # decoded by the loader: passed through by whichever decoder is there
            else:
                if not isinstance(it, (bytes, bytearray, memoryview, tuple)):
                    with open(it, "rb") as f:
                        it = items[k] = (str(it), f.read())
                kind = kind_of(it[1] if isinstance(it, tuple) else it)
                if kind not in self.kinds:
                    kind = self.kinds[0]          # (that decoder routes what is not its own to PIL)
            groups[kind].append(k)
        jobs = []
        for kind, dec in (("png", self.png), ("jpeg", self.jpeg)):
            if groups[kind]:
                sub = [items[k] for k in groups[kind]]
                if kind == "png":
                    sub = [s[1] if isinstance(s, tuple) else s for s in sub]
                jobs.append((groups[kind], dec.decode_async(sub, mode)))
        return _MergedJob(len(items), jobs)

    def decode(self, items, mode=None):
        return self.decode_async(items, mode).result()


class _MergedJob:
    def __init__(self, n, jobs):
        self.n, self.jobs = n, jobs
        self.batch = jobs[0][1].batch if len(jobs) == 1 else None

    def result(self):
        outs, err = [None] * self.n, None
        for idx, job in self.jobs:
            try:
                for k, o in zip(idx, job.result()):
                    outs[k] = o
            except Exception as e:          # noqa: BLE001 -- every job gives its staging back before the first error is raised
                err = err or e
        if err is not None:
            raise err
        return outs

    def discard(self):
        for _, job in self.jobs:
            job.discard()
