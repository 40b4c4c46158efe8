"""The video caller's three stages as one device-resident chain (scripts/inference_swap_video.py --stream): a decoded frame is uploaded once
and stays on the device until its pasted version is downloaded.

  frames u8 [H, W, 3 | 4] + landmarks -> Aligner.align          crops u8 [B, 1024, 1024, 3]                 (rf_resample_u8, rf_align_quad_u8)
                                      -> FaceParser.parse       label maps u8 [B, 512, 512]                 (BiSeNet on rf_conv_gemm)
                                      -> rf_video_prep_u8       target, keep-mask, masked target fp32       (the dataset's __getitem__)
  SwapRunner.run_batch                -> rf_paste_crop_u8       swapped crops u8 [B, 1024, 1024, 3]
                                      -> rf_paste_back_u8       pasted frames u8 [H, W, 4]
  (with a paste mask, instead)        -> rf_paste_alpha_u8      alpha u8 [B, 1024, 1024] of the batch's label maps
                                      -> rf_paste_back_alpha_u8 pasted frames u8 [H, W, 4]

The staged route passes every arrow through PNG files (``<video>cropped_face/``, ``<video>mask_frames/``, ``model_outputs/``) and decodes
every frame twice; each tensor here is the one the staged route would have decoded from its file, bit for bit: the crops and label maps come
from the same kernels, and rf_video_prep_u8 is ``VideoDataset.__getitem__`` (PIL's default BICUBIC resize 1024 -> 512, ToTensor,
Normalize(0.5, 0.5), the label keep-mask, their product).  The inverse transforms are host fp64 arithmetic on the landmarks alone.
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import ops
from .align import Aligner, fill_missing, quad_from_landmarks, resample_taps
from .pasteback import CROP_SIZE, alignment_coefficients, load_frame, paste_on_device


class FrameDataset(Dataset):
    """The host half of the stream: frame ``<frames_dir>/<i>.png`` decoded to a uint8 [H, W, 3 | 4] tensor, with the dataset's 12-digit id.
    Collate with ``reface_amd.data.raw_collate``: frames of one size are stacked, frames of different sizes stay a list."""

    def __init__(self, frames_dir, n, raw=False):
        self.frames_dir, self.n, self.raw = frames_dir, int(n), raw

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if self.raw:          # --gpu_png_decode: the file's bytes (pasteback.frame_item); collate with ``frame_items_collate``
            from .pasteback import frame_item
            return frame_item(self.frames_dir, i), str(i).zfill(12)
        return torch.from_numpy(np.array(load_frame(self.frames_dir, i))), str(i).zfill(12)


class AviFrameDataset(Dataset):
    """The host half of the stream for --video_in: the JPEG bytes of frame i of a Motion-JPEG AVI file (``mjpeg.AviReader``, opened in the
    process that reads), with the dataset's 12-digit id.  Collate with ``frame_items_collate``; ``VideoFrames`` decodes on the device."""

    def __init__(self, path, n):
        self.path, self.n, self._reader = str(path), int(n), None

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if self._reader is None:
            from .mjpeg import AviReader
            self._reader = AviReader(self.path)
        return self._reader.frame(i), str(i).zfill(12)

    def __getstate__(self):          # (a worker opens its own file)
        return {"path": self.path, "n": self.n, "_reader": None}


class VideoFrames:
    """The frames of a Motion-JPEG AVI file as uint8 RGB device tensors [H, W, 3] (what ``load_frame`` gives for the PNG of the same frame):
    ``reader`` an ``mjpeg.AviReader``, ``decoder`` a ``jpegdec.JpegDecoder``.  ``frames[i]`` and ``batch(ids)`` decode on demand; a damaged
    frame raises ``jpegdec.JpegDecodeError`` naming the file and the frame."""

    def __init__(self, reader, decoder):
        self.reader, self.decoder = reader, decoder

    def __len__(self):
        return len(self.reader)

    def items(self, ids, datas=None):
        """(name, bytes) of the frames `ids` for ``decoder.decode_async(..., "RGB")``; `datas`: their bytes when a loader has read them."""
        datas = [self.reader.frame(int(i)) for i in ids] if datas is None else datas
        return [(f"{self.reader.path}#{int(i)}", d) for i, d in zip(ids, datas)]

    def batch(self, ids):
        return self.decoder.decode(self.items(ids), "RGB")

    def __getitem__(self, i):
        return self.batch([i])[0]


def frame_items_collate(items):
    return [f for f, _ in items], [i for _, i in items]


def keep_lut(labels):
    """uint8 [256]: 1 at the face-parsing labels that are cut out of the target (``np.isin(label_map, labels)``)."""
    lut = np.zeros(256, dtype=np.uint8)
    lut[np.asarray(list(labels), dtype=np.int64)] = 1
    return lut


class VideoStream:
    """One video's device chain.  ``landmarks`` fp64 [N, 68, 2] of ALL frames (a non-finite row = no face: the frame uses the crop, label
    map and transform of the last frame that had one, across batches; a first frame without a face raises, here, before anything touches the
    GPU).  ``remove_labels``: the label list of the dataset's keep-mask (``remove_mask_tar_FFHQ``, or [2, 3, 5, 6, 7] without
    ``gray_outer_mask``).  ``parser``: a FaceParser (made on first use from ``seg_ckpt`` otherwise).  ``paste_mask``: a
    ``pasteback.PasteMask``; ``paste`` then composites every crop through the alpha plane of its label map (``state["labels"]``: a frame
    that repeats an earlier face uses that face's labels) instead of replacing the whole quad.

      prepare(frames, ids)  -> (test_batch, {"inpaint_image", "inpaint_mask"}, state)    frames: stacked uint8 tensor or list, host or device
      paste(x_img, state)   -> (pasted frames: B uint8 device tensors [H, W, channels], swapped crops uint8 [B, S, S, 3] on the device)

    ``state`` holds the batch's frames on the device, their indices and inverse transforms, and the crops / label maps (for --stream_keep)."""

    def __init__(self, landmarks, remove_labels, *, seg_ckpt=None, seg12=True, parser=None, image_size=512, crop_size=CROP_SIZE, channels=4,
                 device="cuda", paste_mask=None, pad_edges=False):
        lm = np.asarray(landmarks, dtype=np.float64)
        self.src_of = fill_missing(lm)
        self.quads = {i: quad_from_landmarks(lm[i])[3] for i in sorted(set(self.src_of))}
        coeffs = {i: alignment_coefficients(q, crop_size) for i, q in self.quads.items()}
        self.inv_transforms = np.stack([coeffs[s] for s in self.src_of]) if len(lm) else np.zeros((0, 8))
        self.S, self.size, self.channels, self.seg12 = int(crop_size), int(image_size), int(channels), bool(seg12)
        self.device, self.seg_ckpt, self.parser = torch.device(device), seg_ckpt, parser
        self.lut_host = keep_lut(remove_labels)
        self.paste_mask = paste_mask
        self.pad_edges, self.padded = bool(pad_edges), []          # crop_image's padding of faces at the frame's edge; the frames it padded so far
        self.aligner = self.lut = self.taps = None
        self.last = None          # (frame index, crop u8 [1, S, S, 3], labels u8 [1, S/2, S/2]) of the last frame that had a face

    def _setup(self):
        if self.aligner is None:
            from .parsing import FaceParser
            self.aligner = Aligner(self.S, device=self.device, pad_edges=True) if self.pad_edges else Aligner(self.S, device=self.device)
            self.parser = self.parser or FaceParser(self.seg_ckpt, device=self.device)
            self.lut = torch.from_numpy(self.lut_host).to(self.device)
            self.taps = tuple(torch.from_numpy(a).to(self.device) for a in resample_taps(self.S, self.size, "bicubic"))

    def _to_device(self, frames):
        """The batch's frames as B uint8 device tensors [H, W, C]: one upload per frame size."""
        if torch.is_tensor(frames):
            whole = frames if frames.is_cuda else (frames if frames.is_pinned() else frames.pin_memory()).to(self.device, non_blocking=True)
            return list(whole.unbind(0))
        frames = [f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f)) for f in frames]
        out, groups = [None] * len(frames), {}
        for i, f in enumerate(frames):
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] not in (3, 4):
                raise ValueError(f"frames are uint8 [H, W, 3 | 4], got {f.dtype} {tuple(f.shape)}")
            groups.setdefault(tuple(f.shape), []).append(i)
        for members in groups.values():
            host = [i for i in members if not frames[i].is_cuda]
            if host:
                up = torch.stack([frames[i] for i in host]).pin_memory().to(self.device, non_blocking=True)
                for k, i in enumerate(host):
                    out[i] = up[k]
            for i in members:
                if frames[i].is_cuda:
                    out[i] = frames[i]
        return out

    @torch.no_grad()
    def prepare(self, frames, ids):
        self._setup()
        idx = [int(s) for s in ids]
        fdev = self._to_device(frames)
        if len(fdev) != len(idx):
            raise ValueError(f"{len(idx)} ids for {len(fdev)} frames")
        bad = [i for i in idx if not 0 <= i < len(self.src_of)]
        if bad:
            raise IndexError(f"frames {bad} have no landmarks ({len(self.src_of)} rows)")
        faces = [j for j, i in enumerate(idx) if self.src_of[i] == i]
        # the pool's rows: the face carried over from earlier batches (when a frame of this batch repeats it), then this batch's faces
        pool_c, pool_l, where = [], [], {}
        if self.last is not None and any(self.src_of[i] == self.last[0] for i in idx):
            where[self.last[0]] = 0
            pool_c.append(self.last[1])
            pool_l.append(self.last[2])
        if faces:
            crops, _ = self.aligner.align([fdev[j] for j in faces], quads=np.stack([self.quads[idx[j]] for j in faces]))
            self.padded += [idx[faces[k]] for k in self.aligner.padded]
            labels = self.parser.parse(crops, seg12=self.seg12)
            for k, j in enumerate(faces):
                where[idx[j]] = len(pool_c) + k
            pool_c.append(crops)
            pool_l.append(labels)
            self.last = (idx[faces[-1]], crops[-1:].clone(), labels[-1:].clone())
        missing = [i for i in idx if self.src_of[i] not in where]
        if missing:
            raise ValueError(f"frames {missing} have no face and the frame whose crop they repeat ({[self.src_of[i] for i in missing]}) was not "
                             "streamed before them: frames are prepared in order")
        sel = [where[self.src_of[i]] for i in idx]
        pc, pl = (torch.cat(p) if len(p) > 1 else p[0] for p in (pool_c, pool_l))
        if sel != list(range(pc.shape[0])):
            s = torch.tensor(sel, device=self.device)
            pc, pl = pc.index_select(0, s), pl.index_select(0, s)
        crops_b, labels_b = pc, pl
        B, h = len(idx), self.size
        target = torch.empty((B, 3, h, h), dtype=torch.float32, device=self.device)
        mask = torch.empty((B, 1, h, h), dtype=torch.float32, device=self.device)
        inpaint = torch.empty_like(target)
        ops.video_prep_u8(crops_b.contiguous(), labels_b.contiguous(), self.lut, self.taps, self.taps, target, mask, inpaint)()
        state = {"frames": fdev, "index": idx, "inv_transforms": self.inv_transforms[idx], "crops": crops_b, "labels": labels_b}
        return target, {"inpaint_image": inpaint, "inpaint_mask": mask}, state

    @torch.no_grad()
    def paste(self, x_img, state):
        if self.paste_mask is None:
            return paste_on_device(x_img, state["inv_transforms"], state["frames"], crop_size=self.S, channels=self.channels)
        return paste_on_device(x_img, state["inv_transforms"], state["frames"], crop_size=self.S, channels=self.channels, labels=state["labels"],
                               mask=self.paste_mask)


def stream_paths(base_dir, target_video, outdir):
    """The staged route's directories that a stream run leaves out (and --stream_keep fills)."""
    video = os.path.basename(target_video).split(".")[0]
    return {"crops": os.path.join(base_dir, video + "cropped_face"), "masks": os.path.join(base_dir, video + "mask_frames"),
            "model_outputs": os.path.join(outdir, "model_outputs")}
