"""The identity score of a swap run: ArcFace ID retrieval (top-1, top-5) and mean ID similarity of the results against their sources --
the reference's eval_tool/ID_retrieval/ID_retrieval.py, on the HIP kernels.

  host     file lists in natural order, labels from the file names, decode (DataLoader workers), upload of the raw uint8 bytes
  device   rf_id_prep_u8 (cv2 INTER_LINEAR resize to 112x112, preserved-label mask, normalise, multiply: :189-228) ->
           ArcFace IR-SE50 engine, ``Backbone.forward_id112`` (pool 256 / crop / pool 112 / body: :124-135) ->
           rf_id_retrieve (fp64 scores, top-1 / top-5 / label rank / renormalised cosine per result, totals: :362-390)

``prep_host`` and ``score_host`` restate the same lines on the host (numpy / torch-CPU; float64 scores): they are what the CPU tests hold
against the reference's own outputs (tests/golden/idscore.npz) and what the GPU tests may compare the kernels with.  They are not a
fallback: ``IDScorer`` runs on the GPU only.

Third-party arithmetic that is restated, not pinned: cv2's resize (reface_amd/data.py:resize_u8_linear) and cv2's decoder (PIL decodes here;
lossless formats give the same bytes, JPEG decoders may differ in the last bit); ``natsort`` (natural_key below, for plain file names).
"""
import os
import re
import time

import numpy as np
import torch

from .data import resize_u8_linear

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}
# preserved face-parsing labels per --dataset (:202-209); any other name keeps labels 0 .. 20 ("no mask")
PRESERVE = {"celeba": [1, 2, 4, 5, 8, 9, 6, 7, 10, 11, 12], "ffhq": [1, 2, 3, 5, 6, 7, 9], "ff++": [1, 2, 4, 5, 8, 9]}
DEFAULT_ARCFACE_CKPT = "Other_dependencies/arcface/model_ir_se50.pth"
ARCFACE_TEST_SEED = 77          # `--arcface_ckpt none`: params.seeded_state_dict(params.arcface_param_specs(), 77), the weights of the fixtures
SIZE = 112


def preserve_labels(dataset):
    return list(PRESERVE.get(dataset, range(21)))


def natural_key(name):
    """Sort key of ``natsort.natsorted`` (default algorithm) for plain file names: the name split into text and digit runs, digit runs
    compared as integers, text as it is; equal keys ("07.png", "7.png") fall back to the name."""
    parts = re.split(r"(\d+)", str(name))
    return tuple(int(p) if i % 2 else p for i, p in enumerate(parts)), str(name)


def list_images(folder):
    """Every file of ``folder`` (not its sub-folders) with an image extension, in natural order of the names (:317-322)."""
    names = [n for n in os.listdir(folder) if "." in n and n.rsplit(".", 1)[1] in IMAGE_EXTENSIONS and os.path.isfile(os.path.join(folder, n))]
    return [os.path.join(folder, n) for n in sorted(names, key=natural_key)]


def parse_labels(files):
    """Identity labels of a sorted file list (:325-337): the first all-digit part of every file name split on ``[_/.-]``, minus the smallest
    such number of the folder.  A name without a number has no label (the list is then shorter than ``files``, as in the reference)."""
    numbers = []
    for f in files:
        digits = [int(p) for p in re.split(r"[_\/.-]", os.path.basename(str(f))) if p.isdigit()]
        if digits:
            numbers.append(digits[0])
    if not numbers:
        raise ValueError("no file name carries a number: identity labels cannot be read")
    lo = min(numbers)
    return [n - lo for n in numbers]


def read_pair(img_path, mask_path):
    """One item as raw bytes: the RGB image [H, W, 3] and its label map [Hl, Wl], uint8 (cv2.imread + BGR2RGB / PIL 'L' in the reference)."""
    from PIL import Image
    img = np.asarray(Image.open(img_path).convert("RGB"), dtype=np.uint8)
    lab = np.asarray(Image.open(mask_path).convert("L"), dtype=np.uint8)
    return img, lab


def prep_host(image_u8, labels_u8, preserve, size=SIZE):
    """``MaskedImagePathDataset.__getitem__`` (:189-228) on the host: uint8 [H, W, 3] image + uint8 [Hl, Wl] label map -> fp32 [3, size, size]."""
    mask = np.where(np.isin(labels_u8, list(preserve)), 255, 0).astype(np.uint8)
    m = torch.from_numpy(mask).float()[None, None] / 255.0
    # torchvision's Resize on a tensor: bilinear, align_corners=False, no antialias (torchvision 0.12)
    m = torch.nn.functional.interpolate(m, size=(size, size), mode="bilinear", align_corners=False)[0]
    img = resize_u8_linear(np.ascontiguousarray(image_u8), size, size)                       # A.Resize = cv2 INTER_LINEAR
    x = torch.from_numpy(img.transpose(2, 0, 1).copy()).float() / 255.0
    x = (x - 0.5) / 0.5
    return (x * m).numpy()


def score_host(f_src, f_res, labels):
    """The scores of ``calculate_id_given_paths`` (:362-390) in numpy float64.  f_src [N, 512], f_res [M, 512], labels [M] (indices into
    f_src).  Sources are ordered per result by score descending, ties to the lower index."""
    f1 = np.asarray(f_src, dtype=np.float64)
    f2 = np.asarray(f_res, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    if lab.shape != (f2.shape[0],) or lab.min() < 0 or lab.max() >= f1.shape[0]:
        raise IndexError(f"labels must be {f2.shape[0]} indices into the {f1.shape[0]} sources")
    dot = np.dot(f2, f1.T)
    order = np.stack([np.lexsort((np.arange(dot.shape[1]), -row)) for row in dot])          # best first, lower index first among equals
    pred = order[:, 0]
    rank = np.argmax(order == lab[:, None], axis=1)
    sel = f1[lab]
    sel = sel / np.linalg.norm(sel, axis=1, keepdims=True)
    f2n = f2 / np.linalg.norm(f2, axis=1, keepdims=True)
    sims = np.diagonal(np.dot(sel, f2n.T)).copy()
    return {"top1": float(np.sum(rank == 0) / len(lab)), "top5": float(np.sum(rank < 5) / len(lab)), "mean": float(np.mean(sims)),
            "similarities": sims, "pred": pred, "top5_idx": order[:, :5], "rank": rank, "n": int(len(lab))}


def boundary_gaps(f_src, f_res, labels):
    """Per result, how far the label's score is from changing a hit flag: the distance to the nearest score across the rank 1|2 boundary
    and across the rank 5|6 boundary (fixture generator: a fixture whose smallest gap is tiny would test the summation order, not the metric)."""
    dot = np.dot(np.asarray(f_res, dtype=np.float64), np.asarray(f_src, dtype=np.float64).T)
    gaps = np.empty((dot.shape[0], 2))
    for i, (row, l) in enumerate(zip(dot, labels)):
        others = np.sort(np.delete(row, l))[::-1]          # descending, without the label
        for c, k in enumerate((1, 5)):                      # the label is within the first k iff it beats others[k - 1]
            gaps[i, c] = abs(row[l] - others[k - 1]) if len(others) >= k else np.inf
    return gaps


def load_arcface_state(ckpt):
    from . import params as P
    if ckpt is None or str(ckpt).lower() == "none":
        return P.seeded_state_dict(P.arcface_param_specs(), ARCFACE_TEST_SEED)
    return torch.load(ckpt, map_location="cpu")


class _PairFolder(torch.utils.data.Dataset):
    """Images and label maps paired BY POSITION in their two sorted lists (:278, 190-199), as raw uint8 tensors."""

    def __init__(self, files, maskfiles):
        if len(maskfiles) < len(files):
            raise ValueError(f"{len(files)} images but only {len(maskfiles)} label maps")
        self.files, self.maskfiles = files, maskfiles

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        img, lab = read_pair(self.files[i], self.maskfiles[i])
        return torch.from_numpy(img.copy()), torch.from_numpy(lab.copy())


class _PairBytes(torch.utils.data.Dataset):
    """``_PairFolder`` for --gpu_png_decode: (image item, label-map item) as ``pngdec.ByteFolder`` gives them (file bytes where the device
    decodes the file, PIL's array where it does not)."""

    def __init__(self, files, maskfiles, kinds=("png",)):
        from . import pngdec
        self.img, self.lab = pngdec.ByteFolder(files, "RGB", kinds), pngdec.ByteFolder(maskfiles[:len(files)], "L", kinds)

    def __len__(self):
        return len(self.img)

    def __getitem__(self, i):
        return self.img[i], self.lab[i]


class IDScorer:
    """ArcFace identity scoring on the GPU.  ``state_dict``: IR-SE50 weights (model_ir_se50.pth layout); ``precision``: "full" (fp32, the
    default: this is a measurement) or "bf16" for the ArcFace engine; ``batch``: images per engine run (engines are built per batch size:
    full batches plus one tail engine)."""

    def __init__(self, state_dict, precision="full", batch=50, device="cuda"):
        from .encoders import Backbone
        if precision not in ("full", "bf16"):
            raise ValueError(f"precision must be 'full' or 'bf16', not {precision!r}")
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("reface_amd identity scoring runs on the GPU only (HIP kernels; there is no CPU fallback)")
        self.batch = int(batch)
        self.precision = precision
        self.net = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se",
                            compute_dtype=torch.bfloat16 if precision == "bf16" else torch.float32)
        self.net.load_state_dict(state_dict, strict=True)
        self.net.to(self.dev).eval()
        self._luts = {}
        self.png_decoder = None          # a pngdec.PngDecoder: images and label maps are then decoded on the device (--gpu_png_decode)

    def lut(self, preserve):
        key = tuple(sorted(int(p) for p in preserve))
        t = self._luts.get(key)
        if t is None:
            t = torch.zeros(256, dtype=torch.uint8)
            t[torch.tensor([p for p in key if 0 <= p < 256], dtype=torch.long)] = 1
            t = self._luts[key] = t.to(self.dev)
        return t

    @torch.no_grad()
    def prep_u8(self, images_u8, labels_u8, preserve, out=None):
        """uint8 images [B, H, W, 3] + label maps [B, Hl, Wl] (stacked tensors, or lists when sizes differ; host or device) -> the engine's
        input fp32 [B, 3, 112, 112] (rf_id_prep_u8: one launch per run of consecutive items of equal sizes)."""
        from . import ops
        lut = preserve if torch.is_tensor(preserve) else self.lut(preserve)
        B = len(images_u8)
        if out is None:
            out = torch.empty((B, 3, SIZE, SIZE), dtype=torch.float32, device=self.dev)
        if torch.is_tensor(images_u8) and torch.is_tensor(labels_u8):
            groups = [(images_u8, labels_u8, 0)]
        else:
            # mixed sizes: runs of consecutive items with equal image and label-map shapes are stacked (on the host when they arrive
            # there: one upload per run) and take one launch each, as DevicePrep.resize_sources groups its sources
            groups, i = [], 0
            while i < B:
                j = i + 1
                while j < B and images_u8[j].shape == images_u8[i].shape and labels_u8[j].shape == labels_u8[i].shape:
                    j += 1
                groups.append((torch.stack([images_u8[k] for k in range(i, j)]), torch.stack([labels_u8[k] for k in range(i, j)]), i))
                i = j
        for img, lab, i in groups:
            img = img.to(self.dev, non_blocking=True).contiguous()
            lab = lab.to(self.dev, non_blocking=True).contiguous()
            ops.id_prep_u8(img, lab, lut, out[i:i + img.shape[0]])()
        return out

    @torch.no_grad()
    def embed_u8(self, images_u8, labels_u8, preserve):
        """Device (or host) bytes -> unit-norm ArcFace features fp32 [B, 512] on the device."""
        B = len(images_u8)
        feats = torch.empty((B, 512), dtype=torch.float32, device=self.dev)
        for s in range(0, B, self.batch):
            e = min(B, s + self.batch)
            x = self.prep_u8(images_u8[s:e], labels_u8[s:e], preserve, out=self.net.id_input(e - s))
            feats[s:e] = self.net.forward_id112(x)[0]
        return feats

    @torch.no_grad()
    def score(self, f_src, f_res, labels):
        """rf_id_retrieve on device features: dict(top1, top5, mean, similarities [M] fp64, pred [M], top5_idx [M, 5], rank [M], n)."""
        from . import ops
        M, N = f_res.shape[0], f_src.shape[0]
        lab = np.asarray(labels, dtype=np.int64)
        if lab.shape != (M,) or lab.min() < 0 or lab.max() >= N:
            raise IndexError(f"labels must be {M} indices into the {N} sources")
        dev = self.dev
        labels_d = torch.from_numpy(lab.astype(np.int32)).to(dev)
        top5 = torch.empty((M, 5), dtype=torch.int32, device=dev)
        rank = torch.empty((M,), dtype=torch.int32, device=dev)
        sim = torch.empty((M,), dtype=torch.float64, device=dev)
        totals = torch.empty((4,), dtype=torch.float64, device=dev)
        ops.id_retrieve(f_res.to(dev, torch.float32).contiguous(), f_src.to(dev, torch.float32).contiguous(), labels_d, top5, rank, sim, totals)()
        t = totals.cpu().numpy()
        top5 = top5.cpu().numpy()
        return {"top1": float(t[0] / t[3]), "top5": float(t[1] / t[3]), "mean": float(t[2] / t[3]), "similarities": sim.cpu().numpy(),
                "pred": top5[:, 0].copy(), "top5_idx": top5, "rank": rank.cpu().numpy(), "n": int(t[3])}

    def embed_folder(self, folder, mask_folder, preserve, num_workers=0):
        """(features [n, 512] on the device, labels) of one image folder and its label-map folder."""
        from .data import raw_collate
        files, maskfiles = list_images(folder), list_images(mask_folder)
        if not files:
            raise ValueError(f"no image files in {folder}")
        labels = parse_labels(files)
        batch = min(self.batch, len(files))          # (:273-276: a batch larger than the folder becomes the folder)
        if self.png_decoder is not None:
            # the workers read bytes; images (.convert("RGB")) and label maps (.convert("L")) are decoded here, on the device
            from . import pngdec
            if len(maskfiles) < len(files):
                raise ValueError(f"{len(files)} images but only {len(maskfiles)} label maps")
            dec = self.png_decoder
            pairs = torch.utils.data.DataLoader(_PairBytes(files, maskfiles, getattr(dec, "kinds", ("png",))), batch_size=batch, shuffle=False, drop_last=False, num_workers=num_workers,
                                                collate_fn=pngdec.list_collate)
            loader = ((dec.decode([a for a, _ in items], "RGB"), [m[:, :, 0] for m in dec.decode([b for _, b in items], "L")]) for items in pairs)
        else:
            loader = torch.utils.data.DataLoader(_PairFolder(files, maskfiles), batch_size=batch, shuffle=False, drop_last=False,
                                                 num_workers=num_workers, collate_fn=raw_collate)
        feats = torch.empty((len(files), 512), dtype=torch.float32, device=self.dev)
        at = 0
        for img, lab in loader:
            n = len(img)
            x = self.prep_u8(img, lab, preserve, out=self.net.id_input(n))
            feats[at:at + n] = self.net.forward_id112(x)[0]
            at += n
        return feats, labels

    def score_folders(self, paths, dataset="celeba", num_workers=0):
        """paths = (source images, results, source label maps, result / target label maps), as the reference's four positionals.  The
        labels of the results index the sorted source list (:365-373)."""
        for p in paths:
            if not os.path.exists(p):
                raise RuntimeError("Invalid path: %s" % p)
        preserve = preserve_labels(dataset)
        # the engines the two folders need (full batch, tails) are built before the clock starts: `seconds` / `images_per_s` are decode + upload +
        # prep + ArcFace + retrieval, not engine construction
        for folder in paths[:2]:
            n = len(list_images(folder))
            for b in {min(self.batch, n), n % min(self.batch, n) if n else 0} - {0}:
                self.net.id_input(b)
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        f_src, src_labels = self.embed_folder(paths[0], paths[2], preserve, num_workers)
        f_res, res_labels = self.embed_folder(paths[1], paths[3], preserve, num_workers)
        if len(res_labels) != f_res.shape[0]:
            raise ValueError("a result file name carries no number: results and labels would be misaligned")
        out = self.score(f_src, f_res, res_labels)
        torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        n_img = int(f_src.shape[0] + f_res.shape[0])
        out.update({"labels": [int(l) for l in res_labels], "source_labels": [int(l) for l in src_labels], "images": n_img,
                    "images_per_s": n_img / dt, "seconds": dt})
        return out
