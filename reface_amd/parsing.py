"""BiSeNet face parser on the HIP kernels: the label maps every inpainting and source-face mask of REFace is derived from.

Interfaces mirror pretrained/face_parsing/face_parsing_demo.py:257-318 (``FaceParser``, ``faceParsing_demo``) over
pretrained/face_parsing/model.py + resnet.py (``BiSeNet(n_classes=19)``, eval mode).  What one image goes through:

  uint8 crop [H, W, 3] -> rf_parse_prep (ToTensor, BicubicDownSample(2), clamp, ImageNet normalise) -> [H/2, W/2, 8] fp32
  ResNet-18: 7x7/2 stem + BN + ReLU -> rf_maxpool3x3s2 -> 4 x 2 BasicBlocks  relu(shortcut + bn2(conv2(relu(bn1(conv1 x)))))
  context path: ARM32(feat32) * 1 + conv_avg(mean feat32) -> 2x nearest -> conv_head32; ARM16(feat16) + that -> 2x nearest -> conv_head16
  FFM: ConvBNReLU 1x1 of [feat8 | feat16_up] -> feat * sigmoid(W2 relu(W1 mean feat)) + feat
  conv_out: ConvBNReLU 3x3 -> 1x1 to 19 logits at H/16 -> rf_parse_head (bilinear align_corners=True to H/2, first-max argmax, label LUT)

Every convolution runs on rf_conv_gemm in fp32 with the BatchNorm folded into weights and bias; the global means are rf_spatial_mean, the
attention vectors ops.linear with a sigmoid / ReLU epilogue.  The auxiliary heads conv_out16 / conv_out32 are loaded (the checkpoint holds
them) but not computed: they do not reach the label map.  fp32 only, as the reference runs.
"""
import os

import numpy as np
import torch

from . import ops
from .encoders import _bn_affine
from .params import bisenet_param_specs, bisenet_units, seeded_state_dict
from .unet import _Pool

F32 = torch.float32
N_CLASSES = 19
SEED = 91                 # seeded weights of ``ckpt = "none"`` (and of the golden fixtures, tools/gen_golden.py::gen_bisenet)

# face_parsing_demo.py:72-113 (__ffhq_masks_to_faceParser_mask_detailed): 19 face-parsing classes -> the 12-class map (--seg12);
# classes it does not name (15 ear_r... 16 neck, 18 cloth and the rest) become 0 (background)
_SEG12 = {0: 0, 12: 1, 13: 1, 2: 2, 3: 2, 4: 3, 5: 3, 17: 4, 10: 5, 1: 6, 7: 7, 8: 7, 14: 8, 11: 9, 6: 10, 9: 11}


def seg12_lut():
    """uint8 [256] lookup table of the 19 -> 12 class conversion."""
    lut = np.zeros(256, dtype=np.uint8)
    for k, v in _SEG12.items():
        lut[k] = v
    return lut


def identity_lut():
    return np.arange(256, dtype=np.uint8)


def load_bisenet_state(ckpt):
    """State dict of BiSeNet(19) from a checkpoint path (``79999_iter.pth``), or the seeded weights when ``ckpt`` is None / "none".  The
    key set must match bisenet_param_specs() exactly, as the reference's strict load_state_dict; a missing ``num_batches_tracked`` is
    accepted (PyTorch's BatchNorm loader accepts checkpoints written before it existed)."""
    specs = bisenet_param_specs(N_CLASSES)
    if ckpt is None or str(ckpt).lower() == "none":
        return seeded_state_dict(specs, SEED)
    sd = torch.load(ckpt, map_location="cpu")
    unexpected = [k for k in sd if k not in specs]
    missing = [k for k in specs if k not in sd and not k.endswith(".num_batches_tracked")]
    if unexpected or missing:
        raise RuntimeError(f"face-parsing checkpoint {ckpt} does not match BiSeNet(n_classes=19): missing {missing[:5]}, unexpected {unexpected[:5]}")
    bad = [k for k in sd if tuple(sd[k].shape) != tuple(specs[k])]
    if bad:
        raise RuntimeError(f"face-parsing checkpoint {ckpt}: shape mismatch for {[(k, tuple(sd[k].shape), specs[k]) for k in bad[:5]]}")
    return sd


class _ParserEngine:
    """Prepared launch list of BiSeNet for one (batch, crop height, crop width) on the HIP kernels."""
    CP = 8      # 3 input channels stored in 8

    def __init__(self, sd, B, H, W, device):
        if H % 64 or W % 64:
            raise ValueError(f"face parser: crop sizes must be multiples of 64 (got {H}x{W}): the network runs at 1/32 of the half-size input")
        self.B, self.H, self.W, self.dev = B, H, W, device
        self.pool = _Pool(device)
        self.sd = {k: v.detach().to(device=device, dtype=F32) for k, v in sd.items() if v.dtype.is_floating_point}
        self.launches = []
        # no split-K scratch: every GEMM then sums K in one fixed order whatever its M, so an image's labels do not depend on the batch it is in
        self.ws = ops.new_workspace(device, nbytes=0)
        with ops.workspace_scope(self.ws):
            self._build()
        self.sd = None

    def _conv(self, x, key, cout, *, bn, ksize, stride=1, act=ops.ACT_RELU, ups=0, x2=None, cin_pad=None):
        """conv (no bias) with its BatchNorm folded into weights / bias (bn=None: plain conv), optional 2x nearest upsample of the source and
        optional second source concatenated on channels."""
        B, Hin, Win, _ = x.shape
        w, bias = self.sd[key], None
        if bn is not None:
            a, bias = _bn_affine(self.sd, bn)
            w = w * a.view(-1, 1, 1, 1)
        pad = ksize // 2
        Hv, Wv = (Hin * 2, Win * 2) if ups else (Hin, Win)
        Ho, Wo = (Hv + 2 * pad - ksize) // stride + 1, (Wv + 2 * pad - ksize) // stride + 1
        y = self.pool.get((B, Ho, Wo, cout), F32)
        self.launches.append(ops.conv2d(x, ops.pack_conv_weight(w, F32, cin_pad=cin_pad), y, bias, ksize=ksize, stride=stride, pad=(pad, pad), ups=ups,
                                        x2=x2, act=act, name=key))
        return y

    def _mean(self, x):
        """global mean of x [B, h, w, C] -> fp32 [B, C] (F.avg_pool2d over the whole map)"""
        m = torch.empty((x.shape[0], x.shape[3]), dtype=F32, device=self.dev)
        self.launches.append(ops.spatial_mean(x, m))
        return m

    def _fc(self, m, key, act, bn=None):
        """1x1 conv (no bias) on a [B, C] vector, optional BatchNorm folded in, then act."""
        w = self.sd[key]
        w = w.reshape(w.shape[0], -1)
        bias = None
        if bn is not None:
            a, bias = _bn_affine(self.sd, bn)
            w = w * a.view(-1, 1)
        out = torch.empty((m.shape[0], w.shape[0]), dtype=F32, device=self.dev)
        self.launches.append(ops.linear(m, w.contiguous(), out, bias, act=act, name=key))
        return out

    def _build(self):
        B, H, W, dev = self.B, self.H, self.W, self.dev
        self.x_u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        x = self.pool.get((B, H // 2, W // 2, self.CP), F32)
        self.launches.append(ops.parse_prep(self.x_u8, x))
        # ResNet-18 (resnet.py:66-74)
        y = self._conv(x, "cp.resnet.conv1.weight", 64, bn="cp.resnet.bn1", ksize=7, stride=2, cin_pad=self.CP)
        self.pool.put(x)
        Bn, Hs, Ws, Cs = y.shape
        x = self.pool.get((Bn, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1, Cs), F32)
        self.launches.append(ops.maxpool3x3s2(y, x, name="cp.resnet.maxpool"))
        self.pool.put(y)
        feats = []
        for p, cin, cout, stride in bisenet_units():
            r1 = self._conv(x, f"{p}.conv1.weight", cout, bn=f"{p}.bn1", ksize=3, stride=stride)
            r2 = self._conv(r1, f"{p}.conv2.weight", cout, bn=f"{p}.bn2", ksize=3, act=ops.ACT_NONE)
            self.pool.put(r1)
            sc = x
            if cin != cout or stride != 1:
                sc = self._conv(x, f"{p}.downsample.0.weight", cout, bn=f"{p}.downsample.1", ksize=1, stride=stride, act=ops.ACT_NONE)
            y = self.pool.get(tuple(r2.shape), F32)
            self.launches.append(ops.add_relu(sc, r2, y, name=f"{p}.add_relu"))
            self.pool.put(r2)
            if sc is not x:
                self.pool.put(sc)
            if not any(x is f for f in feats):
                self.pool.put(x)
            x = y
            if p.endswith(".1") and not p.startswith("cp.resnet.layer1"):
                feats.append(y)                     # layer2 / layer3 / layer4 outputs: 1/8, 1/16, 1/32
        feat8, feat16, feat32 = feats
        # context path (model.py:108-128)
        avg = self._fc(self._mean(feat32), "cp.conv_avg.conv.weight", ops.ACT_RELU, bn="cp.conv_avg.bn")     # ConvBNReLU 1x1 of the global mean
        f32a = self._conv(feat32, "cp.arm32.conv.conv.weight", 128, bn="cp.arm32.conv.bn", ksize=3)
        s32 = self._fc(self._mean(f32a), "cp.arm32.conv_atten.weight", ops.ACT_SIGMOID, bn="cp.arm32.bn_atten")
        sum32 = self.pool.get(tuple(f32a.shape), F32)
        self.launches.append(ops.scale_add_vec(f32a, s32, avg, sum32, name="cp.arm32.scale_add_avg"))
        self.pool.put(f32a)
        up32 = self._conv(sum32, "cp.conv_head32.conv.weight", 128, bn="cp.conv_head32.bn", ksize=3, ups=1)
        self.pool.put(sum32)
        f16a = self._conv(feat16, "cp.arm16.conv.conv.weight", 128, bn="cp.arm16.conv.bn", ksize=3)
        s16 = self._fc(self._mean(f16a), "cp.arm16.conv_atten.weight", ops.ACT_SIGMOID, bn="cp.arm16.bn_atten")
        sum16 = self.pool.get(tuple(f16a.shape), F32)
        self.launches.append(ops.se_scale_add(f16a, s16, up32, sum16, stride=1, name="cp.arm16.scale_add"))
        self.pool.put(f16a)
        self.pool.put(up32)
        up16 = self._conv(sum16, "cp.conv_head16.conv.weight", 128, bn="cp.conv_head16.bn", ksize=3, ups=1)
        self.pool.put(sum16)
        # feature fusion (model.py:205-216): the concat is rf_conv_gemm's second source
        feat = self._conv(feat8, "ffm.convblk.conv.weight", 256, bn="ffm.convblk.bn", ksize=1, x2=up16)
        att = self._fc(self._fc(self._mean(feat), "ffm.conv1.weight", ops.ACT_RELU), "ffm.conv2.weight", ops.ACT_SIGMOID)
        fuse = self.pool.get(tuple(feat.shape), F32)
        self.launches.append(ops.se_scale_add(feat, att, feat, fuse, stride=1, name="ffm.scale_add"))
        self.pool.put(feat)
        # output head (model.py:42-50, 252)
        c = self._conv(fuse, "conv_out.conv.conv.weight", 256, bn="conv_out.conv.bn", ksize=3)
        self.pool.put(fuse)
        self.logits = self._conv(c, "conv_out.conv_out.weight", N_CLASSES, bn=None, ksize=1, act=ops.ACT_NONE)
        self.pool.put(c)
        self.body = list(self.launches)
        self.labels = torch.empty((B, H // 2, W // 2), dtype=torch.uint8, device=dev)
        self.luts = {False: torch.from_numpy(identity_lut()).to(dev), True: torch.from_numpy(seg12_lut()).to(dev)}
        self.heads = {k: ops.parse_head(self.logits, lut, self.labels, name="parse_head") for k, lut in self.luts.items()}

    def run(self, crops_u8, seg12):
        """crops_u8: uint8 device tensor [B, H, W, 3] -> the engine's uint8 label buffer [B, H/2, W/2] (overwritten by the next run)."""
        self.x_u8.copy_(crops_u8)
        ops.run(self.body)
        self.heads[bool(seg12)]()
        return self.labels


class FaceParser:
    """Drop-in for the reference's ``FaceParser(seg_ckpt, size=1024)`` (face_parsing_demo.py:257-300) on the HIP engine.  ``seg_ckpt``:
    ``79999_iter.pth`` or "none" (seeded weights).  Calling it on a PIL image returns the 19-class label map as a device long tensor
    [H/2, W/2], as the reference's forward does; ``parse`` takes batches of uint8 crops."""

    def __init__(self, seg_ckpt, size=1024, device="cuda", max_batch=16):
        if not torch.cuda.is_available():
            raise RuntimeError("reface_amd FaceParser runs on the GPU only (HIP kernels; there is no CPU fallback)")
        if size != 1024:
            raise ValueError(f"FaceParser: size {size} is not supported (the reference's callers use 1024: a 2x bicubic downsample to 512)")
        self.seg_ckpt, self.size, self.max_batch = seg_ckpt, size, int(max_batch)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.sd = load_bisenet_state(seg_ckpt)
        self._engines = {}

    def _engine(self, B, H, W):
        key = (B, H, W)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._engines[key] = _ParserEngine(self.sd, B, H, W, self.device)
        return eng

    @torch.no_grad()
    def parse(self, crops, seg12=False):
        """crops: uint8 [B, H, W, 3] or [H, W, 3] (numpy or torch, RGB; H, W multiples of 64) -> uint8 device tensor [B, H/2, W/2] of
        face-parsing labels (19 classes, or the 12-class map with seg12=True).  Runs in device batches of at most ``max_batch``."""
        if isinstance(crops, np.ndarray) and not crops.flags.writeable:
            crops = crops.copy()                    # (a PIL image's array view is read-only)
        x = torch.as_tensor(crops)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"FaceParser.parse: expected uint8 RGB crops [B, H, W, 3], got {tuple(x.shape)} {x.dtype}")
        if x.shape[2] < 512:
            raise ValueError("FaceParser.parse: crops narrower than 512 px take the reference's resize branch, which is not built here")
        B, H, W = x.shape[:3]
        x = x.to(self.device)
        out = torch.empty((B, H // 2, W // 2), dtype=torch.uint8, device=self.device)
        for i in range(0, B, self.max_batch):
            n = min(self.max_batch, B - i)
            out[i:i + n].copy_(self._engine(n, H, W).run(x[i:i + n].contiguous(), seg12))
        return out

    def forward(self, img):
        """img: PIL image (RGB, width >= 512) -> 19-class label map, long device tensor [H/2, W/2] (face_parsing_demo.py:285-300)."""
        return self.parse(np.asarray(img.convert("RGB")))[0].long()

    __call__ = forward


def parse_label_maps(jobs, ckpt, *, seg12, batch=16, parser=None):
    """Stage 1's parsing half as the reference's callers run it (inference_swap_selected.py:466-470, inference_swap_video.py:452-453,
    esitmate_FFHQ_mask.py): every (crop path, label-map path) in ``jobs`` -- the crop read as RGB, resized to 1024^2 (PIL bilinear),
    parsed, its label map written as a PNG -- in device batches of ``batch``.  Returns the number of maps written."""
    from PIL import Image
    jobs = list(jobs)
    if not jobs:
        return 0
    parser = parser or FaceParser(ckpt, max_batch=batch)
    for i in range(0, len(jobs), batch):
        chunk = jobs[i:i + batch]
        crops = np.stack([np.asarray(Image.open(src).convert("RGB").resize((1024, 1024), Image.BILINEAR)) for src, _ in chunk])
        for (_, dst), m in zip(chunk, parser.parse(crops, seg12=seg12).cpu().numpy()):
            os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
            Image.fromarray(m).save(dst)
    return len(jobs)
