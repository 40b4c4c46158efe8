"""The pose score of a swap run: the L2 distance between the Hopenet head-pose angles (yaw, pitch, roll, in degrees) of every swapped result
and those of its target -- the reference's eval_tool/Pose/pose_compare.py over eval_tool/face_vid2vid/modules/hopenet.py, on the HIP kernels.

  host     file lists in natural order, labels from the LAST number of each file name, decode (DataLoader workers), upload of the raw bytes
  device   rf_pose_prep_u8 (ToTensor, tensor Resize((224, 224)) = bilinear without antialias, ImageNet Normalize: :91-99) ->
           ResNet-50 on rf_conv_gemm: 7x7/2 stem + BN + ReLU -> rf_maxpool3x3s2 -> 3 + 4 + 6 + 3 Bottlenecks
           relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + identity), stride on the 3x3 conv2, block tail on rf_add_relu ->
           rf_pose_head (AvgPool2d(7), fc_yaw / fc_pitch / fc_roll, max-shifted softmax, sum(p * bin) * 3 - 99: :101-108) ->
           rf_pose_distance (float64 norms of target[label] - result and their sum: :320-323)

Every convolution runs in fp32 with its BatchNorm folded into weights and bias, without split-K (an empty workspace), so an image's degrees
do not depend on the batch it is in.  ``fc_finetune`` is loaded (the checkpoint holds it) and never computed, as in the reference.  fp32 only.

``prep_host``, ``degrees_from_logits_host``, ``score_host`` and ``parse_labels_last`` restate the same lines on the host (torch-CPU / numpy
float64): they are what the CPU tests hold against the reference's own outputs (tests/golden/pose.npz) and what the GPU tests compare the
kernels with.  They are not a fallback: ``PoseScorer`` runs on the GPU only.

Third-party arithmetic that is restated, not pinned: torchvision 0.12's ``Bottleneck`` and its ToTensor / Resize / Normalize transforms
(tools/gen_golden.py:gen_pose restates them around the reference's own Hopenet), and ``natsort`` (idscore.natural_key, for plain file names).
"""
import os
import re
import time

import numpy as np
import torch

from . import ops
from .encoders import _bn_affine
from .idscore import list_images
from .params import hopenet_param_specs, hopenet_units, seeded_state_dict
from .unet import _Pool

F32 = torch.float32
SIZE = 224
N_BINS = 66
SEED = 53                  # seeded weights of ``ckpt = "none"`` (and of the golden fixture, tools/gen_golden.py::gen_pose)
DEFAULT_HOPENET_CKPT = "Other_dependencies/Hopenet_pose/hopenet_robust_alpha1.pkl"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HEADS = ("fc_yaw", "fc_pitch", "fc_roll")


def parse_labels_last(files):
    """Pose labels of a sorted file list (:269-281): the LAST all-digit part of every file name split on ``[_/.-]``, minus the smallest such
    number of the folder (the identity metric takes the first part: idscore.parse_labels).  A name without a number has no label (the list
    is then shorter than ``files``, as in the reference)."""
    numbers = []
    for f in files:
        digits = [int(p) for p in re.split(r"[_\/.-]", os.path.basename(str(f))) if p.isdigit()]
        if digits:
            numbers.append(digits[-1])
    if not numbers:
        raise ValueError("no file name carries a number: pose labels cannot be read")
    lo = min(numbers)
    return [n - lo for n in numbers]


def prep_host(image_u8):
    """``ImagePathDataset.__getitem__`` (:91-99) on the host: uint8 [H, W, 3] -> fp32 [3, 224, 224].  ToTensor, then torchvision 0.12's
    Resize on a tensor (bilinear, align_corners=False, no antialias at any size), then Normalize with the ImageNet constants."""
    x = torch.from_numpy(np.ascontiguousarray(image_u8).transpose(2, 0, 1).copy()).to(F32).div(255)
    x = torch.nn.functional.interpolate(x[None], size=(SIZE, SIZE), mode="bilinear", align_corners=False, antialias=False)[0]
    mean = torch.as_tensor(MEAN, dtype=F32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=F32).view(-1, 1, 1)
    return ((x - mean) / std).numpy()


def degrees_from_logits_host(logits):
    """``headpose_pred_to_degree`` (:101-108) per head in float64: logits [n, 198] (yaw | pitch | roll, 66 bins each) or [n, 3, 66] ->
    degrees float64 [n, 3] = sum(softmax(l) * [0..65]) * 3 - 99, the softmax shifted by the head's maximum."""
    l = np.asarray(logits, dtype=np.float64).reshape(-1, 3, N_BINS)
    e = np.exp(l - l.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    return (p * np.arange(N_BINS, dtype=np.float64)).sum(axis=2) * 3.0 - 99.0


def score_host(deg_target, deg_result, labels):
    """The score of ``calculate_id_given_paths`` (:320-323) in numpy float64: deg_target [N, 3], deg_result [M, 3], labels [M] (positions in
    the sorted target list) -> dict(pose_value, distances [M], n)."""
    f1 = np.asarray(deg_target, dtype=np.float64)
    f2 = np.asarray(deg_result, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    if lab.shape != (f2.shape[0],) or lab.min() < 0 or lab.max() >= f1.shape[0]:
        raise IndexError(f"labels must be {f2.shape[0]} indices into the {f1.shape[0]} targets")
    dist = np.linalg.norm(f1[lab] - f2, axis=1)
    return {"pose_value": float(np.mean(dist)), "distances": dist, "n": int(len(lab))}


def load_hopenet_state(ckpt):
    """State dict of Hopenet from a checkpoint path (``hopenet_robust_alpha1.pkl``), or the seeded weights when ``ckpt`` is None / "none".
    The key set must match hopenet_param_specs() exactly, as the reference's strict load_state_dict; a missing ``num_batches_tracked`` is
    accepted (PyTorch's BatchNorm loader accepts checkpoints written before it existed)."""
    if ckpt is None or str(ckpt).lower() == "none":
        return seeded_state_dict(hopenet_param_specs(), SEED)
    return check_hopenet_state(torch.load(ckpt, map_location="cpu"), ckpt)


def check_hopenet_state(sd, origin="state dict"):
    specs = hopenet_param_specs()
    unexpected = [k for k in sd if k not in specs]
    missing = [k for k in specs if k not in sd and not k.endswith(".num_batches_tracked")]
    if unexpected or missing:
        raise RuntimeError(f"Hopenet checkpoint {origin} does not match Hopenet(Bottleneck, [3, 4, 6, 3], 66): missing {missing[:5]}, unexpected {unexpected[:5]}")
    bad = [k for k in sd if tuple(sd[k].shape) != tuple(specs[k])]
    if bad:
        raise RuntimeError(f"Hopenet checkpoint {origin}: shape mismatch for {[(k, tuple(sd[k].shape), specs[k]) for k in bad[:5]]}")
    return sd


class _PoseEngine:
    """Prepared launch list of Hopenet for one batch size on the HIP kernels: u8-prepared input [B, 224, 224, 8] -> degrees [B, 3]."""
    CP = 8      # 3 input channels stored in 8

    def __init__(self, sd, B, device):
        self.B, self.dev = B, device
        self.pool = _Pool(device)
        self.sd = {k: v.detach().to(device=device, dtype=F32) for k, v in sd.items() if v.dtype.is_floating_point}
        self.launches = []
        # no split-K scratch: every GEMM then sums K in one fixed order whatever its M, so an image's degrees do not depend on the batch it is in
        self.ws = ops.new_workspace(device, nbytes=0)
        with ops.workspace_scope(self.ws):
            self._build()
        self.sd = None

    def _conv(self, x, key, cout, *, bn, ksize, stride=1, act=ops.ACT_RELU, cin_pad=None):
        """conv (no bias) with its BatchNorm folded into weights / bias."""
        B, Hin, Win, _ = x.shape
        a, bias = _bn_affine(self.sd, bn)
        w = self.sd[key] * a.view(-1, 1, 1, 1)
        pad = ksize // 2
        Ho, Wo = (Hin + 2 * pad - ksize) // stride + 1, (Win + 2 * pad - ksize) // stride + 1
        y = self.pool.get((B, Ho, Wo, cout), F32)
        self.launches.append(ops.conv2d(x, ops.pack_conv_weight(w, F32, cin_pad=cin_pad), y, bias, ksize=ksize, stride=stride, pad=(pad, pad), act=act, name=key))
        return y

    def _build(self):
        B, dev = self.B, self.dev
        self.x = torch.empty((B, SIZE, SIZE, self.CP), dtype=F32, device=dev)          # rf_pose_prep_u8 writes it in place
        # stem (hopenet.py:56-59)
        y = self._conv(self.x, "conv1.weight", 64, bn="bn1", ksize=7, stride=2, cin_pad=self.CP)
        Bn, Hs, Ws, Cs = y.shape
        x = self.pool.get((Bn, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1, Cs), F32)
        self.launches.append(ops.maxpool3x3s2(y, x, name="maxpool"))
        self.pool.put(y)
        # torchvision 0.12's Bottleneck: 1x1 -> 3x3 (stride) -> 1x1, each with BN, ReLU after the first two; out = relu(bn3(conv3) + identity).
        # rf_conv_gemm's epilogue is act(..) + residual, not relu(.. + identity): the block is closed by rf_add_relu
        for p, cin, planes, stride in hopenet_units():
            r1 = self._conv(x, f"{p}.conv1.weight", planes, bn=f"{p}.bn1", ksize=1)
            r2 = self._conv(r1, f"{p}.conv2.weight", planes, bn=f"{p}.bn2", ksize=3, stride=stride)
            self.pool.put(r1)
            r3 = self._conv(r2, f"{p}.conv3.weight", planes * 4, bn=f"{p}.bn3", ksize=1, act=ops.ACT_NONE)
            self.pool.put(r2)
            sc = x
            if stride != 1 or cin != planes * 4:
                sc = self._conv(x, f"{p}.downsample.0.weight", planes * 4, bn=f"{p}.downsample.1", ksize=1, stride=stride, act=ops.ACT_NONE)
            y = self.pool.get(tuple(r3.shape), F32)
            self.launches.append(ops.add_relu(r3, sc, y, name=f"{p}.add_relu"))
            self.pool.put(r3)
            if sc is not x:
                self.pool.put(sc)
            self.pool.put(x)
            x = y
        assert tuple(x.shape) == (B, 7, 7, 2048), tuple(x.shape)
        self.feat = x
        self.w198 = torch.cat([self.sd[f"{h}.weight"] for h in HEADS]).contiguous()
        self.b198 = torch.cat([self.sd[f"{h}.bias"] for h in HEADS]).contiguous()
        self.degrees = torch.empty((B, 3), dtype=F32, device=dev)
        self.logits = torch.empty((B, 3 * N_BINS), dtype=F32, device=dev)
        self.launches.append(ops.pose_head(self.feat, self.w198, self.b198, self.degrees, self.logits, name="pose_head"))

    def run(self):
        """The engine's input buffer ``x`` -> its degrees buffer [B, 3] (overwritten by the next run)."""
        ops.run(self.launches)
        return self.degrees


class _ImageFolder(torch.utils.data.Dataset):
    """The files of one folder as raw uint8 RGB tensors [H, W, 3] (``Image.open(p).convert('RGB')``, :98)."""

    def __init__(self, files):
        self.files = files

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        return torch.from_numpy(np.asarray(Image.open(self.files[i]).convert("RGB"), dtype=np.uint8).copy())


def _list_collate(items):
    return list(items)


class PoseScorer:
    """Hopenet pose scoring on the GPU.  ``state_dict``: Hopenet weights (hopenet_robust_alpha1.pkl layout, checked strictly); ``batch``:
    images per engine run (engines are built per batch size: full batches plus one tail engine).  fp32 only."""

    def __init__(self, state_dict, batch=20, device="cuda"):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("reface_amd pose scoring runs on the GPU only (HIP kernels; there is no CPU fallback)")
        if not torch.cuda.is_available():
            raise RuntimeError("reface_amd pose scoring runs on the GPU only (HIP kernels; there is no CPU fallback): no GPU is available")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be positive, not {batch}")
        self.sd = check_hopenet_state(state_dict)
        self._engines = {}
        self.png_decoder = None          # a pngdec.PngDecoder: the folders' files are then decoded on the device (--gpu_png_decode)

    def engine(self, B):
        eng = self._engines.get(B)
        if eng is None:
            eng = self._engines[B] = _PoseEngine(self.sd, B, self.dev)
        return eng

    @torch.no_grad()
    def prep_u8(self, images_u8, out=None):
        """uint8 images [B, H, W, 3] (a stacked tensor, or a list when sizes differ; host or device) -> the engine's input fp32 NHWC
        [B, 224, 224, 8] (rf_pose_prep_u8: one launch per run of consecutive items of equal size)."""
        B = len(images_u8)
        if out is None:
            out = torch.empty((B, SIZE, SIZE, 8), dtype=F32, device=self.dev)
        if torch.is_tensor(images_u8):
            groups = [(images_u8, 0)]
        else:
            # mixed sizes: runs of consecutive items of equal shape are stacked (on the host when they arrive there: one upload per run) and
            # take one launch each, as IDScorer.prep_u8 groups its items
            groups, i = [], 0
            while i < B:
                j = i + 1
                while j < B and images_u8[j].shape == images_u8[i].shape:
                    j += 1
                groups.append((torch.stack([torch.as_tensor(images_u8[k]) for k in range(i, j)]), i))
                i = j
        for img, i in groups:
            img = img.to(self.dev, non_blocking=True).contiguous()
            ops.pose_prep_u8(img, out[i:i + img.shape[0]])()
        return out

    @torch.no_grad()
    def degrees_u8(self, images_u8):
        """Device (or host) bytes -> (yaw, pitch, roll) in degrees, fp32 [B, 3] on the device."""
        B = len(images_u8)
        deg = torch.empty((B, 3), dtype=F32, device=self.dev)
        for s in range(0, B, self.batch):
            e = min(B, s + self.batch)
            eng = self.engine(e - s)
            self.prep_u8(images_u8[s:e], out=eng.x)
            deg[s:e] = eng.run()
        return deg

    @torch.no_grad()
    def score(self, deg_target, deg_result, labels):
        """rf_pose_distance on device degrees: dict(pose_value, distances [M] fp64, n).  The labels index ``deg_target``."""
        M, N = deg_result.shape[0], deg_target.shape[0]
        lab = np.asarray(labels, dtype=np.int64)
        if lab.shape != (M,) or M == 0 or lab.min() < 0 or lab.max() >= N:
            raise IndexError(f"labels must be {M} indices into the {N} targets")
        dev = self.dev
        labels_d = torch.from_numpy(lab.astype(np.int32)).to(dev)
        dist = torch.empty((M,), dtype=torch.float64, device=dev)
        totals = torch.empty((2,), dtype=torch.float64, device=dev)
        ops.pose_distance(deg_result.to(dev, F32).contiguous(), deg_target.to(dev, F32).contiguous(), labels_d, dist, totals)()
        t = totals.cpu().numpy()
        return {"pose_value": float(t[0] / t[1]), "distances": dist.cpu().numpy(), "n": int(t[1])}

    def degrees_folder(self, folder, num_workers=0):
        """(degrees [n, 3] on the device, labels) of one image folder, files in natural order."""
        if str(folder).endswith(".npz"):
            raise ValueError(f"{folder}: .npz statistics are not supported (the reference's .npz branch cannot run: it leaves its result undefined)")
        files = list_images(folder)
        if not files:
            raise ValueError(f"no image files in {folder}")
        labels = parse_labels_last(files)
        batch = min(self.batch, len(files))          # (:131-134: a batch larger than the folder becomes the folder)
        if self.png_decoder is not None:
            from . import pngdec
            loader = pngdec.device_batches(self.png_decoder, files, batch, num_workers, "RGB")
        else:
            loader = torch.utils.data.DataLoader(_ImageFolder(files), batch_size=batch, shuffle=False, drop_last=False, num_workers=num_workers,
                                                 collate_fn=_list_collate)
        deg = torch.empty((len(files), 3), dtype=F32, device=self.dev)
        at = 0
        for imgs in loader:
            n = len(imgs)
            eng = self.engine(n)
            self.prep_u8(imgs, out=eng.x)
            deg[at:at + n] = eng.run()
            at += n
        return deg, labels

    def score_folders(self, paths, num_workers=0):
        """paths = (targets, results), as the reference's two positionals.  The labels of the RESULTS index the sorted target list
        (:320); the targets' own labels are computed and not used, as in the reference."""
        for p in paths:
            if not os.path.exists(p):
                raise RuntimeError("Invalid path: %s" % p)
            if str(p).endswith(".npz"):
                raise ValueError(f"{p}: .npz statistics are not supported (the reference's .npz branch cannot run: it leaves its result undefined)")
        # the engines the two folders need (full batch, tails) are built before the clock starts: `seconds` / `images_per_s` are decode + upload +
        # prep + Hopenet + distance, not engine construction
        for folder in paths[:2]:
            n = len(list_images(folder))
            for b in {min(self.batch, n), n % min(self.batch, n) if n else 0} - {0}:
                self.engine(b)
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        deg_t, tgt_labels = self.degrees_folder(paths[0], num_workers)
        deg_r, res_labels = self.degrees_folder(paths[1], num_workers)
        if len(res_labels) != deg_r.shape[0]:
            raise ValueError("a result file name carries no number: results and labels would be misaligned")
        out = self.score(deg_t, deg_r, res_labels)
        torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        n_img = int(deg_t.shape[0] + deg_r.shape[0])
        out.update({"labels": [int(l) for l in res_labels], "target_labels": [int(l) for l in tgt_labels],
                    "degrees_target": deg_t.cpu().numpy(), "degrees_result": deg_r.cpu().numpy(), "images": n_img,
                    "images_per_s": n_img / dt, "seconds": dt})
        return out
