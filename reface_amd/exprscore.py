"""The expression score of a swap run: the L2 distance between the 64 expression coefficients Deep3DFaceRecon's ``net_recon`` predicts for
every swapped result and those of its target -- the reference's eval_tool/Expression/expression_compare_face_recon.py over
eval_tool/Deep3DFaceRecon_pytorch_edit/models/networks.py, on the HIP kernels.

  host     file lists in plain ``sorted()`` order, labels from the FIRST number of each file name, decode (DataLoader workers), upload of the
           raw bytes
  device   rf_expr_prep_u8 (PIL's resize((512, 512), BICUBIC) byte for byte, / 255, no mean / std: :123-136) ->
           ResNet-50 on rf_conv_gemm: 7x7/2 stem + BN + ReLU -> rf_maxpool3x3s2 -> 3 + 4 + 6 + 3 Bottlenecks
           relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + identity), stride on the 3x3 conv2; the block tail is conv3's own epilogue
           (ACT_ADD_RELU with ``residual=`` the identity or the downsample output: no rf_add_relu launches) ->
           rf_expr_head (AdaptiveAvgPool2d((1, 1)) over the 16 x 16 map, final_layers.0..6: 257 coefficients) ->
           rf_expr_distance (float64 norms over coefficients [80, 144) of target[label] - result and their sum: :366-375)

Every convolution runs in fp32 with its BatchNorm folded into weights and bias, without split-K (an empty workspace), so an image's
coefficients do not depend on the batch it is in.  fp32 only.

Engine batch size.  The reference's batch of 50 would make the stem's output 50 x 256 x 256 x 64 x 4 B = 839 MB and the layer1 tensors as
large.  An engine's own batch is capped at ``ENGINE_B`` = 25 images (its largest tensor is then 419 MB: no tensor reaches 2^31 bytes, which
is also what rf_conv_gemm's direct-to-LDS loop asks of an operand), and a larger batch runs as several engine batches; batch invariance
makes that invisible in the result.  The cap was not lifted: the kernels on the path were not audited for 64-bit offsets here.

``prep_host``, ``score_host`` and ``parse_labels_first`` restate the same lines on the host (PIL / numpy float64): they are what the CPU tests
hold against the reference's own outputs (tests/golden/expr.npz) and what the GPU tests compare the kernels with.  They are not a fallback:
``ExprScorer`` runs on the GPU only.
"""
import os
import re
import time

import numpy as np
import torch

from . import ops
from .align import resample_taps
from .encoders import _bn_affine
from .idscore import IMAGE_EXTENSIONS
from .params import RECON_FINAL_DIMS, hopenet_units, recon_param_specs, seeded_state_dict
from .posescore import _ImageFolder, _list_collate
from .unet import _Pool

F32 = torch.float32
SIZE = 512
N_COEF = 257
EXP0, EXP_N = 80, 64       # split_coeff (bfm.py:252-273): id [0, 80) | exp [80, 144) | tex | angle | gamma | trans
SEED = 59                  # seeded weights of ``ckpt = "none"`` (and of the golden fixture, tools/gen_golden.py::gen_expr)
ENGINE_B = 25              # images per engine run at the most (module docstring)
DEFAULT_RECON_CKPT = "Other_dependencies/face_recon/epoch_latest.pth"          # checkpoints_dir / name / epoch_<epoch>.pth of test_opt.txt
NPZ_REFUSED = ".npz statistics are not supported (the reference's .npz branch cannot run: it leaves its result undefined)"


def list_images_sorted(folder):
    """Every file of ``folder`` (not its sub-folders) with an image extension in plain ``sorted()`` order of the names, as the reference sorts
    its pathlib paths (:306-308; the pose and identity metrics take natural order instead)."""
    names = [n for n in os.listdir(folder) if "." in n and n.rsplit(".", 1)[1] in IMAGE_EXTENSIONS and os.path.isfile(os.path.join(folder, n))]
    return [os.path.join(folder, n) for n in sorted(names)]


def parse_labels_first(files):
    """Expression labels of a sorted file list (:311-324): the FIRST all-digit part of every file name split on ``[_/.-]``, minus the smallest
    such number of the folder (idscore.parse_labels' rule; the pose metric takes the last part).  A name without a number has no label
    (the list is then shorter than ``files``, as in the reference)."""
    numbers = []
    for f in files:
        digits = [int(p) for p in re.split(r"[_\/.-]", os.path.basename(str(f))) if p.isdigit()]
        if digits:
            numbers.append(digits[0])
    if not numbers:
        raise ValueError("no file name carries a number: expression labels cannot be read")
    lo = min(numbers)
    return [n - lo for n in numbers]


def prep_host(image_u8):
    """``ImagePathDataset.__getitem__`` (:123-136) on the host: uint8 [H, W, 3] -> fp32 [3, 512, 512].  PIL's resize((512, 512), BICUBIC),
    then ``np.array(im) / 255.`` in float64 cast to float32."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(image_u8)).resize((SIZE, SIZE), Image.BICUBIC)
    return (np.array(im) / 255.).astype(np.float32).transpose(2, 0, 1).copy()


def score_host(coef_target, coef_result, labels):
    """The score of ``calculate_id_given_paths`` (:366-375) in numpy float64: coef_target [N, 257 | 64], coef_result [M, 257 | 64] (all
    coefficients, or the expression ones alone), labels [M] (positions in the sorted target list) -> dict(expression_value, distances [M], n)."""
    f1 = np.asarray(coef_target, dtype=np.float64)
    f2 = np.asarray(coef_result, dtype=np.float64)
    if f1.shape[1] == N_COEF:
        f1, f2 = f1[:, EXP0:EXP0 + EXP_N], f2[:, EXP0:EXP0 + EXP_N]
    lab = np.asarray(labels, dtype=np.int64)
    if lab.shape != (f2.shape[0],) or lab.size == 0 or lab.min() < 0 or lab.max() >= f1.shape[0]:
        raise IndexError(f"labels must be {f2.shape[0]} indices into the {f1.shape[0]} targets")
    dist = np.sqrt(np.sum(np.power(f1[lab] - f2, 2), axis=-1))
    return {"expression_value": float(np.mean(dist)), "distances": dist, "n": int(len(lab))}


def seeded_recon_state():
    """The seeded weights of ``ckpt = "none"`` (tools/gen_golden.py::gen_expr checks that they make a usable fixture without any rescaling)."""
    return seeded_state_dict(recon_param_specs(), SEED)


def load_recon_state(ckpt):
    """State dict of ReconNetWrapper from a checkpoint path (``epoch_latest.pth``: its ``net_recon`` entry; a bare state dict is accepted
    too), or the seeded weights when ``ckpt`` is None / "none".  The key set must match recon_param_specs() exactly, as the reference's strict
    load_state_dict; a missing ``num_batches_tracked`` is accepted (PyTorch's BatchNorm loader accepts checkpoints written before it existed)."""
    if ckpt is None or str(ckpt).lower() == "none":
        return seeded_recon_state()
    sd = torch.load(ckpt, map_location="cpu")
    if isinstance(sd, dict) and "net_recon" in sd:
        sd = sd["net_recon"]
    return check_recon_state(sd, ckpt)


def check_recon_state(sd, origin="state dict"):
    specs = recon_param_specs()
    unexpected = [k for k in sd if k not in specs]
    missing = [k for k in specs if k not in sd and not k.endswith(".num_batches_tracked")]
    if unexpected or missing:
        raise RuntimeError(f"net_recon checkpoint {origin} does not match ReconNetWrapper('resnet50', use_last_fc=False): missing {missing[:5]}, unexpected {unexpected[:5]}")
    bad = [k for k in sd if tuple(sd[k].shape) != tuple(specs[k])]
    if bad:
        raise RuntimeError(f"net_recon checkpoint {origin}: shape mismatch for {[(k, tuple(sd[k].shape), specs[k]) for k in bad[:5]]}")
    return sd


class _ExprEngine:
    """Prepared launch list of net_recon for one batch size on the HIP kernels: u8-prepared input [B, 512, 512, 8] -> coefficients [B, 257].
    ``add_relu=True`` closes every block with the two launches of the pose engine (conv3, then rf_add_relu) instead of conv3's own
    ACT_ADD_RELU epilogue: the same bits, 16 launches more."""
    CP = 8      # 3 input channels stored in 8

    def __init__(self, sd, B, device, add_relu=False):
        self.B, self.dev, self.add_relu = B, device, bool(add_relu)
        assert 1 <= B <= ENGINE_B, B
        self.pool = _Pool(device)
        self.sd = {k: v.detach().to(device=device, dtype=F32) for k, v in sd.items() if v.dtype.is_floating_point}
        self.launches = []
        # no split-K scratch: every GEMM then sums K in one fixed order whatever its M, so an image's coefficients do not depend on its batch
        self.ws = ops.new_workspace(device, nbytes=0)
        with ops.workspace_scope(self.ws):
            self._build()
        self.sd = None

    def _conv(self, x, key, cout, *, bn, ksize, stride=1, act=ops.ACT_RELU, cin_pad=None, residual=None):
        """conv (no bias) with its BatchNorm folded into weights / bias."""
        B, Hin, Win, _ = x.shape
        a, bias = _bn_affine(self.sd, bn)
        w = self.sd[key] * a.view(-1, 1, 1, 1)
        pad = ksize // 2
        Ho, Wo = (Hin + 2 * pad - ksize) // stride + 1, (Win + 2 * pad - ksize) // stride + 1
        y = self.pool.get((B, Ho, Wo, cout), F32)
        self.launches.append(ops.conv2d(x, ops.pack_conv_weight(w, F32, cin_pad=cin_pad), y, bias, ksize=ksize, stride=stride, pad=(pad, pad), act=act,
                                        residual=residual, name=key))
        return y

    def _build(self):
        B, dev = self.B, self.dev
        self.x = torch.empty((B, SIZE, SIZE, self.CP), dtype=F32, device=dev)          # rf_expr_prep_u8 writes it in place
        y = self._conv(self.x, "backbone.conv1.weight", 64, bn="backbone.bn1", ksize=7, stride=2, cin_pad=self.CP)
        Bn, Hs, Ws, Cs = y.shape
        x = self.pool.get((Bn, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1, Cs), F32)
        self.launches.append(ops.maxpool3x3s2(y, x, name="maxpool"))
        self.pool.put(y)
        for u, cin, planes, stride in hopenet_units():
            p = f"backbone.{u}"
            r1 = self._conv(x, f"{p}.conv1.weight", planes, bn=f"{p}.bn1", ksize=1)
            r2 = self._conv(r1, f"{p}.conv2.weight", planes, bn=f"{p}.bn2", ksize=3, stride=stride)
            self.pool.put(r1)
            sc = x
            if stride != 1 or cin != planes * 4:
                sc = self._conv(x, f"{p}.downsample.0.weight", planes * 4, bn=f"{p}.downsample.1", ksize=1, stride=stride, act=ops.ACT_NONE)
            if self.add_relu:
                r3 = self._conv(r2, f"{p}.conv3.weight", planes * 4, bn=f"{p}.bn3", ksize=1, act=ops.ACT_NONE)
                y = self.pool.get(tuple(r3.shape), F32)
                self.launches.append(ops.add_relu(r3, sc, y, name=f"{p}.add_relu"))
                self.pool.put(r3)
            else:
                # out = relu(bn3(conv3) + identity) in conv3's epilogue: the residual is read where the tile is written
                y = self._conv(r2, f"{p}.conv3.weight", planes * 4, bn=f"{p}.bn3", ksize=1, act=ops.ACT_ADD_RELU, residual=sc)
            self.pool.put(r2)
            if sc is not x:
                self.pool.put(sc)
            self.pool.put(x)
            x = y
        assert tuple(x.shape) == (B, 16, 16, 2048), tuple(x.shape)
        self.feat = x
        n = len(RECON_FINAL_DIMS)
        self.w257 = torch.cat([self.sd[f"final_layers.{i}.weight"].reshape(-1, 2048) for i in range(n)]).contiguous()
        self.b257 = torch.cat([self.sd[f"final_layers.{i}.bias"] for i in range(n)]).contiguous()
        self.coeffs = torch.empty((B, N_COEF), dtype=F32, device=dev)
        self.launches.append(ops.expr_head(self.feat, self.w257, self.b257, self.coeffs, name="expr_head"))

    def run(self):
        """The engine's input buffer ``x`` -> its coefficient buffer [B, 257] (overwritten by the next run)."""
        ops.run(self.launches)
        return self.coeffs


class ExprScorer:
    """net_recon expression scoring on the GPU.  ``state_dict``: ReconNetWrapper weights (the ``net_recon`` entry of epoch_latest.pth,
    checked strictly); ``batch``: images per loader batch, run as engine batches of ENGINE_B at the most (engines are built per batch size);
    ``add_relu``: the unfused block tail (an A/B switch).  fp32 only."""

    def __init__(self, state_dict, batch=50, device="cuda", add_relu=False):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("reface_amd expression scoring runs on the GPU only (HIP kernels; there is no CPU fallback)")
        if not torch.cuda.is_available():
            raise RuntimeError("reface_amd expression scoring runs on the GPU only (HIP kernels; there is no CPU fallback): no GPU is available")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be positive, not {batch}")
        self.add_relu = bool(add_relu)
        self.sd = check_recon_state(state_dict)
        self._engines = {}
        self.png_decoder = None          # a pngdec.PngDecoder: the folders' files are then decoded on the device (--gpu_png_decode)
        self._taps = {}

    def engine(self, B):
        eng = self._engines.get(B)
        if eng is None:
            eng = self._engines[B] = _ExprEngine(self.sd, B, self.dev, add_relu=self.add_relu)
        return eng

    def taps(self, n_in):
        """PIL's BICUBIC tap table of one axis n_in -> 512 on the device (built once per source size)."""
        t = self._taps.get(n_in)
        if t is None:
            b, k = resample_taps(n_in, SIZE, "bicubic")
            t = self._taps[n_in] = (torch.from_numpy(b).to(self.dev).contiguous(), torch.from_numpy(k).to(self.dev).contiguous())
        return t

    def _engine_sizes(self, n):
        """Engine batch sizes that ``n`` images in loader batches of ``self.batch`` take."""
        sizes = set()
        if n:
            lb = min(self.batch, n)
            for chunk in {lb, n % lb} - {0}:
                sizes |= {min(chunk, ENGINE_B), chunk % ENGINE_B} - {0}
        return sizes

    @torch.no_grad()
    def prep_u8(self, images_u8, out=None):
        """uint8 images [B, H, W, 3] (a stacked tensor, or a list when sizes differ; host or device) -> the engine's input fp32 NHWC
        [B, 512, 512, 8] (rf_expr_prep_u8: one launch per run of consecutive items of equal size)."""
        B = len(images_u8)
        if out is None:
            out = torch.empty((B, SIZE, SIZE, 8), dtype=F32, device=self.dev)
        if torch.is_tensor(images_u8):
            groups = [(images_u8, 0)]
        else:
            groups, i = [], 0
            while i < B:
                j = i + 1
                while j < B and images_u8[j].shape == images_u8[i].shape:
                    j += 1
                groups.append((torch.stack([torch.as_tensor(images_u8[k]) for k in range(i, j)]), i))
                i = j
        for img, i in groups:
            img = img.to(self.dev, non_blocking=True).contiguous()
            ops.expr_prep_u8(img, self.taps(img.shape[2]), self.taps(img.shape[1]), out[i:i + img.shape[0]])()
        return out

    @torch.no_grad()
    def coeffs_u8(self, images_u8):
        """Device (or host) bytes -> the 257 coefficients, fp32 [B, 257] on the device, in engine batches of ENGINE_B at the most."""
        B = len(images_u8)
        coef = torch.empty((B, N_COEF), dtype=F32, device=self.dev)
        step = min(self.batch, ENGINE_B)
        for s in range(0, B, step):
            e = min(B, s + step)
            eng = self.engine(e - s)
            self.prep_u8(images_u8[s:e], out=eng.x)
            coef[s:e] = eng.run()
        return coef

    @torch.no_grad()
    def score(self, coef_target, coef_result, labels):
        """rf_expr_distance on device coefficients [N, 257] / [M, 257]: dict(expression_value, distances [M] fp64, n).  The labels index
        ``coef_target``; one outside [0, N) raises IndexError before the launch."""
        M, N = coef_result.shape[0], coef_target.shape[0]
        lab = np.asarray(labels, dtype=np.int64)
        if lab.shape != (M,) or M == 0 or lab.min() < 0 or lab.max() >= N:
            raise IndexError(f"labels must be {M} indices into the {N} targets")
        dev = self.dev
        labels_d = torch.from_numpy(lab.astype(np.int32)).to(dev)
        dist = torch.empty((M,), dtype=torch.float64, device=dev)
        totals = torch.empty((2,), dtype=torch.float64, device=dev)
        ops.expr_distance(coef_result.to(dev, F32).contiguous(), coef_target.to(dev, F32).contiguous(), labels_d, dist, totals, col0=EXP0, ncols=EXP_N)()
        t = totals.cpu().numpy()
        return {"expression_value": float(t[0] / t[1]), "distances": dist.cpu().numpy(), "n": int(t[1])}

    def coeffs_folder(self, folder, num_workers=0):
        """(coefficients [n, 257] on the device, labels) of one image folder, files in ``sorted()`` order."""
        if str(folder).endswith(".npz"):
            raise ValueError(f"{folder}: {NPZ_REFUSED}")
        files = list_images_sorted(folder)
        if not files:
            raise ValueError(f"no image files in {folder}")
        labels = parse_labels_first(files)
        batch = min(self.batch, len(files))          # (:168-171: a batch larger than the folder becomes the folder)
        if self.png_decoder is not None:
            from . import pngdec
            loader = pngdec.device_batches(self.png_decoder, files, batch, num_workers, "RGB")
        else:
            loader = torch.utils.data.DataLoader(_ImageFolder(files), batch_size=batch, shuffle=False, drop_last=False, num_workers=num_workers,
                                                 collate_fn=_list_collate)
        coef = torch.empty((len(files), N_COEF), dtype=F32, device=self.dev)
        at = 0
        for imgs in loader:
            n = len(imgs)
            coef[at:at + n] = self.coeffs_u8(imgs)
            at += n
        return coef, labels

    def score_folders(self, paths, num_workers=0):
        """paths = (targets, results), as the reference's two positionals.  The labels of the RESULTS index the sorted target list
        (:366); the targets' own labels are computed and not used, as in the reference."""
        for p in paths:
            if not os.path.exists(p):
                raise RuntimeError("Invalid path: %s" % p)
            if str(p).endswith(".npz"):
                raise ValueError(f"{p}: {NPZ_REFUSED}")
        # the engines the two folders need are built before the clock starts: `seconds` / `images_per_s` are decode + upload + prep + net_recon +
        # distance, not engine construction
        for folder in paths[:2]:
            for b in self._engine_sizes(len(list_images_sorted(folder))):
                self.engine(b)
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        coef_t, tgt_labels = self.coeffs_folder(paths[0], num_workers)
        coef_r, res_labels = self.coeffs_folder(paths[1], num_workers)
        if len(res_labels) != coef_r.shape[0]:
            raise ValueError("a result file name carries no number: results and labels would be misaligned")
        out = self.score(coef_t, coef_r, res_labels)
        torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        n_img = int(coef_t.shape[0] + coef_r.shape[0])
        out.update({"labels": [int(l) for l in res_labels], "target_labels": [int(l) for l in tgt_labels],
                    "exp_target": coef_t[:, EXP0:EXP0 + EXP_N].cpu().numpy(), "exp_result": coef_r[:, EXP0:EXP0 + EXP_N].cpu().numpy(), "images": n_img,
                    "images_per_s": n_img / dt, "seconds": dt})
        return out
