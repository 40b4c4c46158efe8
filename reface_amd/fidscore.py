"""The FID of a swap run as the reference computes it (eval_tool/fid/fid_score.py over eval_tool/fid/inception.py): the Frechet distance
between the Gaussians fitted to the ``clip`` ViT-B/32 image features (512 per image; the reference's "inception" returns
``clip_model.encode_image``, not InceptionV3 activations) of two image folders, on the HIP kernels.

  host     file lists (``glob('*.ext')`` per extension, sorted), decode (DataLoader workers), upload of the raw bytes
  device   rf_fid_prep_u8 (``clip.load``'s preprocess: Resize(224, BICUBIC) as PIL's two integer passes, CenterCrop(224), ToTensor,
           Normalize, straight into the patch convolution's NHWC operand) ->
           the vision tower: 32 x 32 / stride 32 patch conv on rf_conv_gemm -> rf_clip_tokens -> pre_layrnorm -> L x (ln1, qkv, rf_attention,
           out_proj + residual, ln2, fc1 QuickGELU, fc2 + residual) -> post_layernorm of the CLS rows -> visual_projection: [B, 512] fp32 ->
           rf_fid_stats (fp64 mean, centred covariance on the fp64 MFMA)
  host     ``frechet_distance``: one ``scipy.linalg.sqrtm`` of a 512 x 512 product, as the reference

The tower's arithmetic is HF ``CLIPVisionModelWithProjection(...).image_embeds``, which is ``clip``'s ``encode_image``; its dimensions come
from a ``CLIPVisionConfig`` (ViT-B/32: hidden 768, 12 layers, 12 heads of 64, patch 32, 50 tokens, projection 512).  Kernel coverage of this
tower: rf_attention instantiates d = 64 and takes any key count (Nk = 50 runs the generic kernel with a masked tail tile, as Nk = 257 of
ViT-L/14 does); rf_conv_gemm walks any KH x KW window, so the 32 x 32 patch convolution at K = 32 * 32 * CP runs the same main loop as the
14 x 14 one -- nothing had to be added to either.

``precision``: "full" (fp32, the default: this is a measurement) or "bf16".  fp16, what ``clip.load`` leaves on a GPU, is not offered:
rf_clip_tokens has no fp16 instantiation.  Every GEMM runs without split-K (an empty workspace), so an image's features do not depend on
its batch.

``prep_host``, ``stats_host`` and ``frechet_distance`` restate the reference's lines on the host (PIL / numpy float64 / scipy): they are what
the CPU tests hold against the reference's own outputs (tests/golden/fid.npz) and what the GPU tests compare the kernels with.  Only
``frechet_distance`` is part of the scoring path; the rest is not a fallback: ``FidScorer`` runs on the GPU only.
"""
import os
import pathlib
import re
import time

import numpy as np
import torch

from . import ops
from .align import resample_taps
from .encoders import CLIP_MEAN, CLIP_STD
from .idscore import IMAGE_EXTENSIONS
from .params import CLIPVisionConfig, fid_clip_param_specs, seeded_state_dict
from .posescore import _list_collate

F32 = torch.float32
SIZE = 224
SEED = 61                  # seeded weights of ``ckpt = "none"`` (and of the golden fixture, tools/gen_golden.py::gen_fid)
VIT_B32 = dict(hidden=768, intermediate=3072, layers=12, heads=12, patch=32, image=224, proj=512, mapper_layers=0)
# the tower of ``ckpt = "none"`` and of the fixture: ViT-B/32's patch, image, head width and token count at a fraction of its width and depth
FIXTURE_TOWER = dict(hidden=128, intermediate=512, layers=2, heads=2, patch=32, image=224, proj=32, mapper_layers=0)
DEFAULT_CLIP_CKPT = "~/.cache/clip/ViT-B-32.pt"          # where clip.load("ViT-B/32") keeps its download
BATCH_WARNING = "Warning: batch size is bigger than the data size. Setting batch size to data size"


# ---------------------------------------------------------------------------------------------------------------------------------
# host restatements
# ---------------------------------------------------------------------------------------------------------------------------------
def resized_size(h, w):
    """torchvision's Resize(224) of an h x w image: the shorter side becomes 224, the longer one int(224 * long / short).  (height, width)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = SIZE, int(SIZE * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def crop_offset(n):
    """torchvision's CenterCrop(224) along an axis of n >= 224 pixels: int(round((n - 224) / 2.0)), Python's rounding (half to even)."""
    return int(round((n - SIZE) / 2.0))


def crop_taps(n_in, n_resized):
    """PIL's BICUBIC tap table of one axis n_in -> n_resized, sliced to the 224 outputs inside the centre crop: (bounds int32 [224, 2],
    taps int32 [224, ksize])."""
    b, k = resample_taps(n_in, n_resized, "bicubic")
    o = crop_offset(n_resized)
    return np.ascontiguousarray(b[o:o + SIZE]), np.ascontiguousarray(k[o:o + SIZE])


def prep_host(image):
    """``clip.load``'s preprocess on the host: a PIL image of any mode (or uint8 [H, W, 3] / [H, W]) -> fp32 [3, 224, 224].
    Resize(224, BICUBIC) in the image's own mode, CenterCrop(224), convert("RGB"), ToTensor (float32(b) / 255), Normalize ((x - mean) / std
    in fp32)."""
    from PIL import Image
    im = image if isinstance(image, Image.Image) else Image.fromarray(np.ascontiguousarray(image))
    w, h = im.size
    nh, nw = resized_size(h, w)
    if (nh, nw) != (h, w):
        im = im.resize((nw, nh), Image.BICUBIC)
    top, left = crop_offset(nh), crop_offset(nw)
    im = im.crop((left, top, left + SIZE, top + SIZE)).convert("RGB")
    x = np.asarray(im, dtype=np.uint8).astype(np.float32) / np.float32(255)
    x = (x - np.asarray(CLIP_MEAN, dtype=np.float32)) / np.asarray(CLIP_STD, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def stats_host(features):
    """``calculate_activation_statistics`` after the activations (:212-213): features [N, D] -> (mu [D], sigma [D, D]) of the float64 array
    the reference fills."""
    act = np.empty(np.shape(features))          # float64, as the reference's pred_arr
    act[:] = features
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def frechet_terms(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """The four terms of ``calculate_frechet_distance`` (:139-190): |mu1 - mu2|^2, tr sigma1, tr sigma2, tr sqrtm(sigma1 sigma2), with the
    reference's ``scipy.linalg.sqrtm`` call, its eps retry on a non-finite root and its check of the imaginary part."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print("fid calculation produces singular product; adding %s to diagonal of cov estimates" % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff), np.trace(sigma1), np.trace(sigma2), np.trace(covmean)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)), summed in the reference's order."""
    d2, t1, t2, tc = frechet_terms(mu1, sigma1, mu2, sigma2, eps)
    return d2 + t1 + t2 - 2 * tc


def list_images(folder):
    """The reference's file list (:223-225): for each image extension ``glob('*.ext')`` of the folder itself, all of them sorted as paths."""
    path = pathlib.Path(folder)
    return [str(f) for f in sorted([f for ext in IMAGE_EXTENSIONS for f in path.glob("*.{}".format(ext))])]


def effective_batch(batch_size, n_files):
    """(:103-106) a batch larger than the folder becomes the folder, with the reference's warning line."""
    if batch_size > n_files:
        print(BATCH_WARNING)
        return n_files
    return batch_size


# ---------------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------------
def seeded_fid_state(cfg=None):
    """The seeded weights of ``ckpt = "none"``: the fixture tower unless another config is given."""
    return seeded_state_dict(fid_clip_param_specs(cfg or CLIPVisionConfig(**FIXTURE_TOWER)), SEED)


_OPENAI_BLOCK = {"attn.out_proj": "self_attn.out_proj", "ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2"}
_OPENAI_TOP = {"visual.conv1.weight": "vision_model.embeddings.patch_embedding.weight",
               "visual.class_embedding": "vision_model.embeddings.class_embedding",
               "visual.positional_embedding": "vision_model.embeddings.position_embedding.weight",
               "visual.ln_pre.weight": "vision_model.pre_layrnorm.weight", "visual.ln_pre.bias": "vision_model.pre_layrnorm.bias",
               "visual.ln_post.weight": "vision_model.post_layernorm.weight", "visual.ln_post.bias": "vision_model.post_layernorm.bias"}


def openai_to_hf(sd):
    """The vision tower of an OpenAI ``clip`` state dict in HF naming.  Every ``visual.*`` key must be one of the map's (anything else
    raises); keys of the text tower are ignored.  ``in_proj_{weight,bias}`` split into q / k / v; ``visual.proj`` [hidden, projection]
    becomes ``visual_projection.weight`` = its transpose."""
    out = {}
    for k, v in sd.items():
        if not k.startswith("visual."):
            continue
        v = v.detach().to(F32)
        if k in _OPENAI_TOP:
            out[_OPENAI_TOP[k]] = v
            continue
        if k == "visual.proj":
            hidden = sd["visual.class_embedding"].shape[0] if "visual.class_embedding" in sd else None
            if v.dim() != 2 or v.shape[0] != hidden:
                raise RuntimeError(f"clip checkpoint: visual.proj must be [hidden = {hidden}, projection], got {tuple(v.shape)}")
            out["visual_projection.weight"] = v.t().contiguous()
            continue
        m = re.fullmatch(r"visual\.transformer\.resblocks\.(\d+)\.(.+)\.(weight|bias)", k)
        m2 = re.fullmatch(r"visual\.transformer\.resblocks\.(\d+)\.attn\.in_proj_(weight|bias)", k)
        p = "vision_model.encoder.layers."
        if m2:
            if v.shape[0] % 3:
                raise RuntimeError(f"clip checkpoint: {k} has {v.shape[0]} rows, not 3 x hidden")
            h = v.shape[0] // 3
            for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
                out[f"{p}{m2.group(1)}.self_attn.{n}.{m2.group(2)}"] = v[j * h:(j + 1) * h].contiguous()
        elif m and m.group(2) in _OPENAI_BLOCK:
            out[f"{p}{m.group(1)}.{_OPENAI_BLOCK[m.group(2)]}.{m.group(3)}"] = v
        else:
            raise RuntimeError(f"clip checkpoint: unexpected vision key {k}")
    return out


def config_of(sd):
    """The tower's dimensions read off an HF-named state dict (heads = hidden / 64, ``clip``'s own rule)."""
    try:
        hidden = int(sd["vision_model.embeddings.class_embedding"].shape[0])
        patch = int(sd["vision_model.embeddings.patch_embedding.weight"].shape[-1])
        tokens = int(sd["vision_model.embeddings.position_embedding.weight"].shape[0])
        inter = int(sd["vision_model.encoder.layers.0.mlp.fc1.weight"].shape[0])
        proj = int(sd["visual_projection.weight"].shape[0])
    except KeyError as e:
        raise RuntimeError(f"clip checkpoint: missing vision key {e.args[0]}")
    layers = 1 + max(int(m.group(1)) for m in (re.match(r"vision_model\.encoder\.layers\.(\d+)\.", k) for k in sd) if m)
    grid = int(round((tokens - 1) ** 0.5))
    if hidden % 64 or grid * grid != tokens - 1:
        raise RuntimeError(f"clip checkpoint: hidden {hidden} is not a multiple of 64 or {tokens} tokens are not a square grid + CLS")
    return CLIPVisionConfig(hidden=hidden, intermediate=inter, layers=layers, heads=hidden // 64, patch=patch, image=grid * patch, proj=proj, mapper_layers=0)


def check_fid_state(sd, origin="state dict"):
    """An OpenAI- or HF-named state dict -> (HF-named fp32 vision state, its config), checked strictly against fid_clip_param_specs: a missing
    or misshapen vision key raises.  Text-tower keys, ``logit_scale`` and HF's ``position_ids`` buffers are ignored."""
    if any(k.startswith("visual.") for k in sd):
        sd = openai_to_hf(sd)
    else:
        sd = {k: v.detach().to(F32) for k, v in sd.items()
              if (k.startswith("vision_model.") or k.startswith("visual_projection.")) and not k.endswith("position_ids")}
    cfg = config_of(sd)
    specs = fid_clip_param_specs(cfg)
    missing = [k for k in specs if k not in sd]
    unexpected = [k for k in sd if k not in specs]
    if missing or unexpected:
        raise RuntimeError(f"clip checkpoint {origin} does not match the vision tower: missing {missing[:5]}, unexpected {unexpected[:5]}")
    bad = [(k, tuple(sd[k].shape), tuple(specs[k])) for k in specs if tuple(sd[k].shape) != tuple(specs[k])]
    if bad:
        raise RuntimeError(f"clip checkpoint {origin}: shape mismatch for {bad[:5]}")
    if cfg.image != SIZE:
        raise RuntimeError(f"clip checkpoint {origin}: the tower takes {cfg.image} x {cfg.image} images, the preprocess makes {SIZE} x {SIZE}")
    return {k: sd[k] for k in specs}, cfg


def load_fid_clip_state(ckpt):
    """(HF-named vision state, config) from the file ``clip.load`` caches (a TorchScript archive: ``torch.jit.load(...).state_dict()``; a
    plain state dict file is accepted too), or the seeded fixture tower when ``ckpt`` is None / "none"."""
    if ckpt is None or str(ckpt).lower() == "none":
        return check_fid_state(seeded_fid_state(), "seeded")
    path = os.path.expanduser(str(ckpt))
    if not os.path.exists(path):
        raise RuntimeError(f"clip checkpoint {path} does not exist (the file clip.load('ViT-B/32') downloads; this tool downloads nothing)")
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except RuntimeError:
        sd = torch.load(path, map_location="cpu")
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
    return check_fid_state(sd, path)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tower
# ---------------------------------------------------------------------------------------------------------------------------------
class _FidEngine:
    """Prepared launch list of the vision tower for one batch size: rf_fid_prep_u8's output ``x`` NHWC [B, 224, 224, CP] -> ``feat`` fp32
    [B, projection].  From post_layernorm on everything is fp32 whatever ``dtype`` is (B rows)."""

    def __init__(self, sd, cfg, B, dtype, device):
        self.cfg, self.B, self.dt, self.dev = cfg, B, dtype, device
        self.CP = 4 if dtype == F32 else 8          # 3 input channels stored in one 16-byte pixel
        self.sd = {k: v.detach().to(device=device, dtype=F32) for k, v in sd.items()}
        self.launches = []
        # no split-K scratch: every GEMM then sums K in one fixed order whatever its M, so an image's features do not depend on its batch
        self.ws = ops.new_workspace(device, nbytes=0)
        with ops.workspace_scope(self.ws):
            self._build()
        self.sd = None

    def w(self, k):
        return self.sd[k].to(self.dt).contiguous()

    def f(self, k):
        return self.sd[k].contiguous()

    def _ln(self, x, key, out):
        self.launches.append(ops.layernorm(x, self.f(f"{key}.weight"), self.f(f"{key}.bias"), out, name=key))

    def _build(self):
        cfg, B, dev, dt = self.cfg, self.B, self.dev, self.dt
        h, heads, P = cfg.hidden, cfg.heads, cfg.patch
        g = cfg.image // P
        NP, NT = g * g, g * g + 1
        v = "vision_model"
        self.x = torch.zeros((B, cfg.image, cfg.image, self.CP), dtype=dt, device=dev)          # rf_fid_prep_u8 writes it in place
        patch = torch.empty((B, g, g, h), dtype=dt, device=dev)
        self.launches.append(ops.conv2d(self.x, ops.pack_conv_weight(self.sd[f"{v}.embeddings.patch_embedding.weight"], dt, cin_pad=self.CP), patch, None,
                                        ksize=P, stride=P, pad=(0, 0), name="patch_embedding"))
        x = torch.empty((B, NT, h), dtype=dt, device=dev)
        self.launches.append(ops.clip_tokens(patch.view(B, NP, h), self.f(f"{v}.embeddings.class_embedding"),
                                             self.f(f"{v}.embeddings.position_embedding.weight"), x))
        M = B * NT
        x2 = x.view(M, h)
        xa = torch.empty((M, h), dtype=dt, device=dev)
        self._ln(x2, f"{v}.pre_layrnorm", xa)
        cur, other = xa, x2
        ln = torch.empty((M, h), dtype=dt, device=dev)
        qkv = torch.empty((M, 3 * h), dtype=dt, device=dev)
        att = torch.empty((M, h), dtype=dt, device=dev)
        mid = torch.empty((M, cfg.intermediate), dtype=dt, device=dev)
        d = h // heads
        for i in range(cfg.layers):
            p = f"{v}.encoder.layers.{i}"
            self._ln(cur, f"{p}.layer_norm1", ln)
            wqkv = torch.cat([self.sd[f"{p}.self_attn.{n}.weight"] for n in ("q_proj", "k_proj", "v_proj")], 0).to(dt).contiguous()
            bqkv = torch.cat([self.sd[f"{p}.self_attn.{n}.bias"] for n in ("q_proj", "k_proj", "v_proj")], 0).contiguous()
            self.launches.append(ops.linear(ln, wqkv, qkv, bqkv, name=f"{p}.qkv"))
            q3 = qkv.view(B, NT, 3 * h)
            self.launches.append(ops.attention(q3[..., :h], q3[..., h:2 * h], q3[..., 2 * h:], att.view(B, NT, h), heads=heads, scale=d ** -0.5,
                                               name=f"{p}.attn"))
            self.launches.append(ops.linear(att, self.w(f"{p}.self_attn.out_proj.weight"), other, self.f(f"{p}.self_attn.out_proj.bias"), residual=cur,
                                            name=f"{p}.out_proj"))
            cur, other = other, cur
            self._ln(cur, f"{p}.layer_norm2", ln)
            self.launches.append(ops.linear(ln, self.w(f"{p}.mlp.fc1.weight"), mid, self.f(f"{p}.mlp.fc1.bias"), act=ops.ACT_QUICK_GELU, name=f"{p}.fc1"))
            self.launches.append(ops.linear(mid, self.w(f"{p}.mlp.fc2.weight"), other, self.f(f"{p}.mlp.fc2.bias"), residual=cur, name=f"{p}.fc2"))
            cur, other = other, cur
        cls_rows = cur.view(B, NT, h)[:, 0, :]          # [B, h] view with row pitch NT * h
        pooled = torch.empty((B, h), dtype=F32, device=dev)
        self._ln(cls_rows, f"{v}.post_layernorm", pooled)
        self.feat = torch.empty((B, cfg.proj), dtype=F32, device=dev)
        self.launches.append(ops.linear(pooled, self.f("visual_projection.weight"), self.feat, None, name="visual_projection"))

    def run(self):
        """The engine's input buffer ``x`` -> its feature buffer [B, projection] (overwritten by the next run)."""
        ops.run(self.launches)
        return self.feat


class _FidFolder(torch.utils.data.Dataset):
    """The files of one folder as what the device preparation takes: ("u8", uint8 [H, W, 3]) for RGB, L (replicated) and RGBA with alpha 255
    everywhere (alpha dropped) -- for these the bytes PIL resizes in the image's own mode and then converts are the bytes of the RGB image
    resized -- and ("host", fp32 [3, 224, 224] from ``prep_host``) for every other mode or alpha."""

    def __init__(self, files, kinds=()):
        self.files, self.kinds = files, tuple(kinds)

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        if self.kinds:
            # --gpu_png_decode: RGB and grey PNG files travel as bytes, ("png", bytes), and are decoded on the device as
            # .convert("RGB") -- the "u8" cases above that need no look at the pixels; RGBA (alpha must be inspected) stays here.
            # --gpu_jpeg_decode: likewise the JPEG files the device takes (grey or YCbCr: PIL's modes L and RGB)
            from . import pngdec
            with open(self.files[i], "rb") as f:
                data = f.read()
            if "png" in self.kinds and data[:8] == pngdec.PNG_SIG:
                info = pngdec.parse_png(data)
                if info.route == "gpu" and info.bpp in (1, 3):
                    return "png", data
            elif pngdec.device_file(data, "RGB", tuple(k for k in self.kinds if k != "png")):
                return "png", data
        return decode_item(Image.open(self.files[i]))


def decode_item(im):
    if im.mode == "RGB":
        return "u8", torch.from_numpy(np.asarray(im, dtype=np.uint8).copy())
    if im.mode == "L":
        return "u8", torch.from_numpy(np.repeat(np.asarray(im, dtype=np.uint8)[:, :, None], 3, axis=2))
    if im.mode == "RGBA":
        a = np.asarray(im, dtype=np.uint8)
        if (a[:, :, 3] == 255).all():
            return "u8", torch.from_numpy(a[:, :, :3].copy())
    return "host", torch.from_numpy(prep_host(im))


class FidScorer:
    """CLIP-feature FID on the GPU.  ``state_dict``: the vision tower in OpenAI or HF naming (checked strictly; its dimensions are read off
    it); ``precision``: "full" (fp32) or "bf16"; ``batch``: images per engine run (engines are built per batch size)."""

    def __init__(self, state_dict, precision="full", batch=50, device="cuda"):
        self.dev = torch.device(device)
        if precision not in ("full", "bf16"):
            raise ValueError(f"precision must be 'full' or 'bf16', not {precision!r}")
        if self.dev.type != "cuda":
            raise RuntimeError("reface_amd FID scoring runs on the GPU only (HIP kernels; there is no CPU fallback)")
        if not torch.cuda.is_available():
            raise RuntimeError("reface_amd FID scoring runs on the GPU only (HIP kernels; there is no CPU fallback): no GPU is available")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be positive, not {batch}")
        self.precision = precision
        self.dt = torch.bfloat16 if precision == "bf16" else F32
        self.sd, self.cfg = check_fid_state(state_dict)
        self.dim = self.cfg.proj
        self._engines = {}
        self._taps = {}
        self.png_decoder = None          # a pngdec.PngDecoder: RGB and grey PNG files are then decoded on the device (--gpu_png_decode)

    def engine(self, B):
        eng = self._engines.get(B)
        if eng is None:
            eng = self._engines[B] = _FidEngine(self.sd, self.cfg, B, self.dt, self.dev)
        return eng

    def taps(self, h, w):
        """The cropped tap tables of an h x w source on the device, (x table, y table), built once per source size."""
        t = self._taps.get((h, w))
        if t is None:
            nh, nw = resized_size(h, w)
            t = self._taps[(h, w)] = tuple(tuple(torch.from_numpy(a).to(self.dev) for a in crop_taps(n, r)) for n, r in ((w, nw), (h, nh)))
        return t

    @torch.no_grad()
    def prep_u8(self, images_u8, out=None):
        """uint8 images [B, H, W, 3] (a stacked tensor, or a list when sizes differ; host or device) -> the engine's input NHWC
        [B, 224, 224, CP] (rf_fid_prep_u8: one launch per run of consecutive items of equal size)."""
        B = len(images_u8)
        if out is None:
            out = torch.empty((B, SIZE, SIZE, 4 if self.dt == F32 else 8), dtype=self.dt, device=self.dev)
        if torch.is_tensor(images_u8):
            groups = [(images_u8, 0)]
        else:
            groups, i = [], 0
            while i < B:
                j = i + 1
                while j < B and images_u8[j].shape == images_u8[i].shape:
                    j += 1
                run = [torch.as_tensor(images_u8[k]) for k in range(i, j)]
                if any(t.is_cuda for t in run):          # a run of device-decoded and host-decoded images of one size: the host ones go up first
                    run = [t.to(self.dev) for t in run]
                groups.append((torch.stack(run), i))
                i = j
        for img, i in groups:
            if not (img.is_cuda and img.dim() == 4 and img.stride(3) == 1 and img.stride(2) == 3 and img.stride(1) == img.shape[2] * 3):
                img = img.to(self.dev, non_blocking=True).contiguous()          # (a strided batch view on the device goes as it is)
            tx, ty = self.taps(img.shape[1], img.shape[2])
            ops.fid_prep_u8(img, tx, ty, out[i:i + img.shape[0]])()
        return out

    @torch.no_grad()
    def features_items(self, items):
        """Decoded items (``decode_item``'s pairs) -> features fp32 [B, projection] on the device (a view of the engine's buffer)."""
        B = len(items)
        eng = self.engine(B)
        i = 0
        while i < B:
            j = i + 1
            if items[i][0] == "u8":
                while j < B and items[j][0] == "u8":
                    j += 1
                self.prep_u8([t for _, t in items[i:j]], out=eng.x[i:j])
            else:          # prepared on the host: uploaded into the engine's layout, pad channels 0
                eng.x[i, :, :, :3] = items[i][1].to(self.dev).permute(1, 2, 0).to(self.dt)
                eng.x[i, :, :, 3:] = 0
            i = j
        return eng.run()

    def features_u8(self, images_u8):
        """uint8 RGB images (a list, or a stacked tensor) -> features fp32 [B, projection] on the device (a copy), in engine batches of
        ``batch`` at the most."""
        B = len(images_u8)
        feat = torch.empty((B, self.dim), dtype=F32, device=self.dev)
        for s in range(0, B, self.batch):
            e = min(B, s + self.batch)
            eng = self.engine(e - s)
            self.prep_u8(images_u8[s:e], out=eng.x)
            feat[s:e] = eng.run()
        return feat

    @torch.no_grad()
    def stats(self, feat):
        """rf_fid_stats on device features fp32 [N, D]: (mu [D], sigma [D, D]) as numpy float64."""
        N, D = feat.shape
        if N < 2:
            raise ValueError(f"a covariance needs at least 2 images, not {N}")
        mu = torch.empty((D,), dtype=torch.float64, device=self.dev)
        sigma = torch.empty((D, D), dtype=torch.float64, device=self.dev)
        ops.fid_stats(feat.to(self.dev, F32).contiguous(), mu, sigma)()
        return mu.cpu().numpy(), sigma.cpu().numpy()

    def features_folder(self, folder, num_workers=0):
        """(features [n, projection] on the device, number of images prepared on the host) of one image folder."""
        files = list_images(folder)
        if not files:
            raise ValueError(f"no image files in {folder}")
        batch = effective_batch(self.batch, len(files))
        loader = torch.utils.data.DataLoader(_FidFolder(files, () if self.png_decoder is None else getattr(self.png_decoder, "kinds", ("png",))), batch_size=batch, shuffle=False, drop_last=False,
                                             num_workers=num_workers, collate_fn=_list_collate)
        feat = torch.empty((len(files), self.dim), dtype=F32, device=self.dev)
        at = host = 0
        for items in loader:
            n = len(items)
            png = [k for k, (kind, _) in enumerate(items) if kind == "png"]
            if png:
                for k, t in zip(png, self.png_decoder.decode([items[k][1] for k in png], "RGB")):
                    items[k] = ("u8", t)
            feat[at:at + n] = self.features_items(items)
            host += sum(1 for kind, _ in items if kind == "host")
            at += n
        return feat, host

    def statistics_of_path(self, path, num_workers=0):
        """``compute_statistics_of_path`` (:217-229): (mu, sigma, images, host-prepared images); an ``.npz`` path is read for its ``mu`` and
        ``sigma``."""
        if str(path).endswith(".npz"):
            with np.load(path) as f:
                return f["mu"][:], f["sigma"][:], 0, 0
        feat, host = self.features_folder(path, num_workers)
        mu, sigma = self.stats(feat)
        return mu, sigma, int(feat.shape[0]), host

    def _warm(self, paths):
        """Builds the engines the folders need before the clock starts: ``seconds`` / ``images_per_s`` do not count engine construction."""
        for p in paths[:2]:
            if not str(p).endswith(".npz"):
                n = len(list_images(p))
                if n:
                    lb = min(self.batch, n)
                    for b in {lb, n % lb} - {0}:
                        self.engine(b)
        torch.cuda.synchronize(self.dev)

    def score_folders(self, paths, num_workers=0):
        """paths = two image folders or ``.npz`` statistics files, as the reference's two positionals -> dict(fid, the four terms, mu1,
        sigma1, image counts, host-prepared count, seconds and images/s from decode to value; engine construction excluded)."""
        for p in paths:
            if not os.path.exists(p):
                raise RuntimeError("Invalid path: %s" % p)
        self._warm(paths)
        t0 = time.perf_counter()
        m1, s1, n1, h1 = self.statistics_of_path(paths[0], num_workers)
        m2, s2, n2, h2 = self.statistics_of_path(paths[1], num_workers)
        d2, t1, t2, tc = frechet_terms(m1, s1, m2, s2)
        fid = d2 + t1 + t2 - 2 * tc
        dt = time.perf_counter() - t0
        return {"fid": float(fid), "mean_term": float(d2), "trace1": float(t1), "trace2": float(t2), "trace_covmean": float(tc), "mu1": m1, "sigma1": s1,
                "images1": n1, "images2": n2, "images": n1 + n2, "host_prepared": h1 + h2, "seconds": dt, "images_per_s": (n1 + n2) / dt}
