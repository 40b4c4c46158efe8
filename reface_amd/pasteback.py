"""Stage 3 of the video caller on the GPU: swapped crops warped back into their full frames (scripts/inference_swap_video.py:705-724 of the
reference), with the reference's PIL arithmetic reproduced byte for byte by two HIP kernels (reface_amd/csrc/pasteback.hip):

  crop  = Image.fromarray((255. * x_hwc).astype(uint8)).resize((1024, 1024), BILINEAR)        rf_paste_crop_u8
  frame = Image.open(<Base_dir>/<video>/<int(sid)>.png)
  c     = np.load(<Base_dir>/<video>_inv_transforms.npy, allow_pickle=True)[int(sid)]
  crop.convert('RGBA') with alpha 255, transformed to frame.size (PERSPECTIVE, c, BILINEAR), alpha-composited over frame.convert('RGBA')
                                                                                              rf_paste_back_u8
The inverse transforms are stage 1's: ``alignment_coefficients(quad, 1024)`` of every frame's alignment quad (the reference's
calc_alignment_coefficients(quad + 0.5, crop corners), :81-84).  Frame decoding and PNG encoding are host work on thread pools; the
warp of a whole batch is one launch.

With a ``PasteMask`` (not in the reference, which replaces the whole oriented square around the face) the crop is composited through a
feathered alpha plane made of its face-parsing label map, so that only the labels the model repaints, and a soft margin, replace frame
pixels -- still PIL's arithmetic byte for byte, now of ``crop.putalpha(alpha)`` instead of alpha 255:

  alpha = 255 at the repainted labels, dilated, box-blurred, resized to 1024^2 (BILINEAR)                    rf_paste_alpha_u8
  (crop, alpha) transformed as above (PIL warps the premultiplied image) and alpha-composited over the frame  rf_paste_back_alpha_u8
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops
from .output import available_cpus

CROP_SIZE = 1024          # the reference aligns to, and pastes back from, 1024^2 crops


def alignment_coefficients(quad, size=CROP_SIZE):
    """The 8 PIL PERSPECTIVE coefficients c that map a frame point (x, y) onto the crop: crop_x = (c0 x + c1 y + c2) / (c6 x + c7 y + 1),
    crop_y = (c3 x + c4 y + c5) / (c6 x + c7 y + 1), such that the quad's corners (pixel centres: quad + 0.5) land on the crop's corners
    (0, 0), (0, size), (size, size), (size, 0) in that order -- what stage 1 stores per frame in ``<video>_inv_transforms.npy``.
    Each correspondence gives two linear equations in c (multiply out the denominator); four corners determine c exactly."""
    src = np.asarray(quad, dtype=np.float64).reshape(4, 2) + 0.5
    dst = np.array([[0, 0], [0, size], [size, size], [size, 0]], dtype=np.float64)
    A = np.zeros((8, 8), dtype=np.float64)
    for k, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        A[2 * k] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * k + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
    return np.linalg.solve(A, dst.reshape(8))


def stage3_paths(base_dir, target_video):
    """Where stage 1 of the reference leaves the full frames and their inverse transforms (:413, :496)."""
    video = os.path.basename(target_video).split(".")[0]
    return {"video_frames": os.path.join(base_dir, video), "inv_transforms": os.path.join(base_dir, video + "_inv_transforms.npy")}


def load_inv_transforms(path):
    """``<video>_inv_transforms.npy`` (a pickled object array of per-frame coefficient vectors, or a plain [N, 8] array) -> fp64 [N, 8]."""
    a = np.load(path, allow_pickle=True)
    out = np.stack([np.asarray(c, dtype=np.float64).reshape(8) for c in a]) if a.dtype == object else np.asarray(a, dtype=np.float64)
    if out.ndim != 2 or out.shape[1] != 8:
        raise ValueError(f"{path}: expected one 8-coefficient vector per frame, got shape {out.shape}")
    return out


def load_frame(frames_dir, sid):
    """Frame ``<frames_dir>/<int(sid)>.png`` as uint8 HWC with 3 or 4 channels (other modes are converted to RGBA, as the reference's
    ``orig_image.convert('RGBA')`` does)."""
    from PIL import Image
    im = Image.open(os.path.join(frames_dir, f"{int(sid)}.png"))
    if im.mode not in ("RGB", "RGBA"):
        im = im.convert("RGBA")
    return np.asarray(im, dtype=np.uint8)


def frame_item(frames_dir, sid):
    """What a loader hands to ``pngdec.PngDecoder.decode`` for frame ``sid`` (--gpu_png_decode): the file's bytes where the device decodes it
    to what ``load_frame`` gives (8-bit RGB and RGBA files), else ``load_frame``'s array as a host tensor."""
    from . import pngdec
    with open(os.path.join(frames_dir, f"{int(sid)}.png"), "rb") as f:
        data = f.read()
    info = pngdec.parse_png(data)
    if info.route == "gpu" and info.bpp in (3, 4):
        return data
    return torch.from_numpy(np.array(load_frame(frames_dir, sid)))


def load_frames_device(decoder, frames_dir, sids):
    """``load_frame`` of every id as uint8 device tensors [H, W, 3 | 4], decoded on the device."""
    return decoder.decode([frame_item(frames_dir, sid) for sid in sids])


class PasteMask:
    """The alpha plane of the masked paste: 255 where the crop's label map has one of ``remove_labels`` (the labels the model repaints:
    the dataset's ``remove_mask_tar_FFHQ``), grown by ``dilate`` label-map pixels, feathered by ``passes`` box blurs of radius ``feather``
    (positions outside the map count as 0: alpha falls to 0 towards the crop's border, so the border of the square cannot show) and enlarged
    to the crop (rf_paste_alpha_u8).  The defaults are a design choice for 512^2 label maps, not a measurement."""

    def __init__(self, remove_labels, dilate=8, feather=8, passes=2):
        self.dilate, self.feather, self.passes = int(dilate), int(feather), int(passes)
        if not 0 <= self.dilate <= 64 or not 0 <= self.feather <= 64:
            raise ValueError(f"dilate and feather are 0 .. 64 label-map pixels, got dilate={dilate} feather={feather}")
        if not 1 <= self.passes <= 3:
            raise ValueError(f"passes is 1 .. 3, got {passes}")
        labels = np.asarray(list(remove_labels), dtype=np.int64)
        if labels.size and (labels.min() < 0 or labels.max() > 255):
            raise ValueError(f"labels are 0 .. 255, got {list(remove_labels)}")
        self.lut_host = np.zeros(256, dtype=np.uint8)
        self.lut_host[labels] = 1
        self._lut = self._scratch = None

    def alpha(self, labels_u8, S):
        """Label maps uint8 [B, Sl, Sl] on the device -> alpha uint8 [B, S, S] on the device (S >= Sl)."""
        if not torch.is_tensor(labels_u8) or labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3 or labels_u8.shape[1] != labels_u8.shape[2]:
            raise ValueError(f"label maps are a uint8 tensor [B, Sl, Sl], got {getattr(labels_u8, 'dtype', type(labels_u8))} "
                             f"{tuple(getattr(labels_u8, 'shape', ()))}")
        B, Sl = labels_u8.shape[0], labels_u8.shape[1]
        if int(S) < Sl:
            raise ValueError(f"the alpha plane is enlarged to the crop, never reduced: label maps of {Sl}, crops of {S}")
        dev = labels_u8.device
        if self._lut is None or self._lut.device != dev:
            self._lut, self._scratch = torch.from_numpy(self.lut_host).to(dev), None
        if self._scratch is None or self._scratch.numel() < 2 * B * Sl * Sl:          # (launches of one stream: the passes of the next call wait)
            self._scratch = torch.empty(2 * B * Sl * Sl, dtype=torch.uint8, device=dev)
        out = torch.empty((B, int(S), int(S)), dtype=torch.uint8, device=dev)
        ops.paste_alpha_u8(labels_u8.contiguous(), self._lut, out, self._scratch, self.dilate, self.feather, self.passes)()
        return out


def load_labels(masks_dir, sid):
    """Label map ``<masks_dir>/<int(sid)>.png`` (stage 1's ``<video>mask_frames``) as uint8 [Sl, Sl]."""
    from PIL import Image
    return np.asarray(Image.open(os.path.join(masks_dir, f"{int(sid)}.png")).convert("L"), dtype=np.uint8)


def _labels_on(labels, B, dev):
    """The batch's label maps (a uint8 tensor [B, Sl, Sl] or B arrays / tensors [Sl, Sl], host or device) as one device tensor."""
    if labels is None:
        raise ValueError("a masked paste needs the crops' label maps (labels=...)")
    if not torch.is_tensor(labels):
        labels = torch.stack([l if torch.is_tensor(l) else torch.from_numpy(np.ascontiguousarray(l)) for l in labels])
    if labels.shape[0] != B:
        raise ValueError(f"{labels.shape[0]} label maps for a batch of {B}")
    return labels.to(dev)


def paste_on_device(result01, coeffs, frames, crop_size=CROP_SIZE, channels=4, labels=None, mask=None):
    """The device half of stage 3 for frames that are on the device already: run_batch's fp32 [B, 3, h, w] result, the frames' inverse
    transforms (fp64 [B, 8], host) and B uint8 device tensors [H, W, 3 | 4] (sizes and channel counts may differ within the batch) ->
    (pasted frames: B uint8 device tensors [H, W, channels]; the enlarged crops uint8 [B, S, S, 3] on the device -- the bytes of
    ``model_outputs/<id>.png``).  Nothing is copied to or from the host except the 8 coefficients per frame.  With ``mask`` (a PasteMask)
    the crops are pasted through the alpha planes of ``labels`` (their label maps, uint8 [B, Sl, Sl]); without it ``labels`` is not read."""
    B, S = result01.shape[0], int(crop_size)
    if len(frames) != B or len(coeffs) != B:
        raise ValueError(f"{len(frames)} frames and {len(coeffs)} transforms for a batch of {B}")
    dev = result01.device
    crops = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    ops.paste_crop_u8(result01.float().contiguous(), crops)()
    co = torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float64).reshape(B, 8)).to(dev)
    alpha = mask.alpha(_labels_on(labels, B, dev), S) if mask is not None else None
    out = [None] * B
    groups = {}
    for i, f in enumerate(frames):          # one launch per frame size (all frames of a video share one)
        groups.setdefault(tuple(f.shape), []).append(i)
    for shape, members in groups.items():
        whole = len(members) == B
        sel = torch.tensor(members, device=dev)
        fr = torch.stack([frames[i] for i in members])
        o = torch.empty(fr.shape[:3] + (int(channels),), dtype=torch.uint8, device=dev)
        cr, cs = (crops, co) if whole else (crops.index_select(0, sel).contiguous(), co.index_select(0, sel).contiguous())
        if alpha is None:
            ops.paste_back_u8(cr, cs, fr, o)()
        else:
            ops.paste_back_alpha_u8(cr, alpha if whole else alpha.index_select(0, sel).contiguous(), cs, fr, o)()
        for k, i in enumerate(members):
            out[i] = o[k]
    return out, crops


class PasteBack:
    """The device half of stage 3 for one video: ``prefetch(ids)`` starts decoding the frames of a batch on a thread pool; ``paste(result01,
    ids)`` turns run_batch's fp32 [B, 3, h, w] result into the pasted frames (uint8 [H, W, channels] host arrays, one per id).  With ``mask``
    (a PasteMask) the paste goes through the crops' label maps: those handed to ``paste`` / ``paste_device`` (``labels=``), else the files
    ``<masks_dir>/<int(id)>.png``, which ``prefetch`` then also reads on its pool."""

    def __init__(self, frames_dir, inv_transforms, crop_size=CROP_SIZE, channels=4, threads=None, mask=None, masks_dir=None):
        self.frames_dir, self.S, self.channels = frames_dir, int(crop_size), int(channels)
        self.mask, self.masks_dir, self._labels = mask, masks_dir, {}
        if mask is not None and not isinstance(mask, PasteMask):
            raise TypeError(f"mask is a PasteMask, got {type(mask).__name__}")
        self.coeffs = load_inv_transforms(inv_transforms) if isinstance(inv_transforms, str) else np.asarray(inv_transforms, dtype=np.float64)
        self.pool = ThreadPoolExecutor(max_workers=threads or max(2, min(8, available_cpus() // 2)))

    def prefetch(self, ids):
        if self.mask is not None and self.masks_dir is not None:          # (paste / paste_device take them from here)
            for sid in ids:
                self._labels[int(sid)] = self.pool.submit(load_labels, self.masks_dir, sid)
        return [self.pool.submit(load_frame, self.frames_dir, sid) for sid in ids]

    def _batch_labels(self, idx, labels, dev):
        """The label maps of the masked paste of frames `idx` on the device (None without a mask): `labels`, else the prefetched files."""
        if self.mask is None:
            return None
        if labels is None:
            if self.masks_dir is None:
                raise ValueError("a masked paste needs the crops' label maps: labels=..., or PasteBack(masks_dir=...)")
            futures = [self._labels.pop(i, None) for i in idx]
            labels = [f.result() if f is not None else load_labels(self.masks_dir, i) for f, i in zip(futures, idx)]
        return _labels_on(labels, len(idx), dev)

    def paste(self, result01, ids, frames=None, labels=None):
        ids = list(ids)
        if len(ids) != result01.shape[0]:
            raise ValueError(f"{len(ids)} ids for a batch of {result01.shape[0]}")
        idx = [int(s) for s in ids]
        bad = [s for s, i in zip(ids, idx) if not 0 <= i < len(self.coeffs)]
        if bad:
            raise IndexError(f"frames {bad} have no inverse transform ({len(self.coeffs)} in the file)")
        frames = [f.result() if hasattr(f, "result") else f for f in (frames if frames is not None else self.prefetch(ids))]
        dev = result01.device
        x = result01.float().contiguous()
        crops = torch.empty((len(ids), self.S, self.S, 3), dtype=torch.uint8, device=dev)
        ops.paste_crop_u8(x, crops)()
        coeffs = torch.from_numpy(self.coeffs[idx]).to(dev)
        labels = self._batch_labels(idx, labels, dev)
        alpha = self.mask.alpha(labels, self.S) if labels is not None else None
        out = [None] * len(ids)
        groups = {}
        for i, f in enumerate(frames):          # one launch per frame size (all frames of a video share one)
            groups.setdefault(f.shape, []).append(i)
        for shape, members in groups.items():
            sel = torch.tensor(members, device=dev)
            fr = torch.from_numpy(np.stack([frames[i] for i in members])).pin_memory().to(dev, non_blocking=True)
            o = torch.empty(fr.shape[:3] + (self.channels,), dtype=torch.uint8, device=dev)
            if alpha is None:
                ops.paste_back_u8(crops.index_select(0, sel).contiguous(), coeffs.index_select(0, sel).contiguous(), fr, o)()
            else:
                ops.paste_back_alpha_u8(crops.index_select(0, sel).contiguous(), alpha.index_select(0, sel).contiguous(),
                                        coeffs.index_select(0, sel).contiguous(), fr, o)()
            host = o.cpu().numpy()
            for k, i in enumerate(members):
                out[i] = host[k]
        return out

    def paste_device(self, result01, ids, frames, labels=None):
        """``paste`` for frames that are on the device already (B uint8 device tensors [H, W, 3 | 4]): the pasted frames stay there too
        (B uint8 device tensors [H, W, channels]); the same bytes as ``paste``."""
        ids = list(ids)
        if len(ids) != result01.shape[0]:
            raise ValueError(f"{len(ids)} ids for a batch of {result01.shape[0]}")
        idx = [int(s) for s in ids]
        bad = [s for s, i in zip(ids, idx) if not 0 <= i < len(self.coeffs)]
        if bad:
            raise IndexError(f"frames {bad} have no inverse transform ({len(self.coeffs)} in the file)")
        return paste_on_device(result01, self.coeffs[idx], frames, crop_size=self.S, channels=self.channels,
                               labels=self._batch_labels(idx, labels, result01.device), mask=self.mask)[0]

    def close(self):
        self.pool.shutdown(wait=True)


def paste_back(result01, ids, frames_dir, inv_transforms, outdir=None, crop_size=CROP_SIZE, channels=4):
    """Paste run_batch's swapped crops (fp32 [B, 3, h, w] in [0, 1] on the device) into their frames ``<frames_dir>/<int(id)>.png`` with the
    coefficients of ``inv_transforms`` (path of the .npy or an [N, 8] array).  Returns the pasted frames as uint8 HWC arrays (RGBA by default)
    and, with ``outdir``, also writes them as ``<outdir>/<id>.png``."""
    pb = PasteBack(frames_dir, inv_transforms, crop_size=crop_size, channels=channels)
    try:
        out = pb.paste(result01, ids)
    finally:
        pb.close()
    if outdir is not None:
        from PIL import Image
        os.makedirs(outdir, exist_ok=True)
        for sid, a in zip(ids, out):
            Image.fromarray(a).save(os.path.join(outdir, f"{sid}.png"))
    return out


class PngWriter:
    """PNG encodes of whole pasted frames off the launch thread (one job per file, like output.OutputWriter).  At most `depth` frames wait
    (``submit`` then blocks on the oldest: a 1080p RGBA frame is 8 MB of host memory); ``close`` drains and raises the first error."""

    def __init__(self, threads=None, depth=32, png_encoder=None):
        self.pool = ThreadPoolExecutor(max_workers=threads or max(2, min(8, available_cpus() // 2)))
        self.pending, self.depth, self.n = [], int(depth), 0
        # png_encoder (--gpu_png): a reface_amd.pngenc.PngEncoder for ``encode_device`` / ``submit_device``; ``submit`` stays the host path
        self.png_encoder = png_encoder

    @staticmethod
    def _save(path, arr):
        from PIL import Image
        Image.fromarray(arr).save(path)

    def _reap(self, block):
        while self.pending and (self.pending[0].done() or (block and len(self.pending) >= self.depth)):
            self.pending.pop(0).result()
            self.n += 1

    def submit(self, path, arr):
        self._reap(block=True)
        self.pending.append(self.pool.submit(self._save, path, arr))

    @staticmethod
    def _write(paths, png_job):
        for path, data in zip(paths, png_job.result()):
            with open(path, "wb") as f:
                f.write(data)

    def encode_device(self, frames):
        """Launch thread: enqueue the PNG encodes of uint8 DEVICE frames [H, W, 3 | 4] on the current stream, frames of one shape as ONE
        batched encode (3 launches per shape, not per frame) -> [(indices into `frames`, PngJob)].  Nothing waits."""
        if self.png_encoder is None:
            raise RuntimeError("PngWriter.encode_device needs a png_encoder")
        groups = {}
        for i, f in enumerate(frames):
            groups.setdefault(tuple(f.shape), []).append(i)
        return [(idx, self.png_encoder.encode_async(torch.stack([frames[i] for i in idx]))) for idx in groups.values()]

    def submit_device(self, paths, png_job):
        """Hand an enqueued encode to the pool: a worker waits for its event, copies the compressed bytes and writes the files `paths` (one per
        image of the job, in order)."""
        self._reap(block=True)
        self.pending.append(self.pool.submit(self._write, list(paths), png_job))
        self.n += len(paths) - 1          # (a reaped job counts once; its other files are counted here)

    def close(self):
        try:
            while self.pending:
                self.pending.pop(0).result()
                self.n += 1
        finally:
            self.pool.shutdown(wait=True)
        return self.n
