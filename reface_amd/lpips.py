"""The learned perceptual distance (LPIPS) between every swapped result and its target -- the reference's eval_tool/lpips/{lpips,networks,
utils}.py (``LPIPS(net_type='alex')``, optionally 'vgg'), on the HIP kernels.

  host     file lists in natural order, labels from the LAST number of each result's file name (a position in the sorted target list, as the
           pose and expression metrics pair them), decode (DataLoader workers), upload of the raw bytes
  device   rf_lpips_prep_u8 (ToTensor, Normalize(0.5, 0.5), BaseNet.z_score: networks.py:50-51) -> AlexNet / VGG16 ``features`` up to the
           fifth tap on rf_conv_gemm (bias + ReLU in the epilogue) and rf_maxpool2d -> per tap rf_lpips_layer (normalize_activation,
           (nx - ny)^2, the 1x1 ``lin`` convolution, the spatial mean: utils.py:6-8, lpips.py:32-33) -> rf_lpips_total (lpips.py:35)

One engine run takes 2B images: the x of B pairs in the first half of the batch, their y in the second.  Every convolution runs in fp32
without split-K (an empty workspace) and rf_lpips_layer's grid per pair does not depend on B, so a pair's distance has the same bits alone and
inside a batch.  fp32 only: the distance is a small difference of near-equal vectors.  An engine's batch is capped so that no tensor reaches
2^31 bytes (``engine_batch_cap``); larger requests run in chunks.

``prep_host``, ``features_host``, ``lpips_host`` and ``score_host`` restate the same lines on the host in float64 (torch-CPU / numpy): they
are what the CPU tests hold against the reference's own outputs (tests/golden/lpips.npz) and what the GPU tests compare the kernels with.
They are not a fallback: ``LPIPSScorer`` runs on the GPU only.

Third-party arithmetic that is restated, not pinned: torchvision's ``alexnet().features`` / ``vgg16().features`` (params.lpips_plan;
tools/gen_golden.py:gen_lpips restates them around the reference's own modules).  Nothing here downloads: the reference fetches both the
backbone and the linear weights from the network; here they come from a checkpoint (``load_lpips_state``).
"""
import collections
import os
import time

import numpy as np
import torch

from . import ops
from .idscore import list_images
from .params import lpips_param_specs, lpips_plan, seeded_state_dict
from .posescore import _ImageFolder, parse_labels_last
from .unet import _Pool

F32 = torch.float32
F64 = torch.float64
SEED = 61                  # seeded weights of ``ckpt = "none"`` (and of the golden fixture, tools/gen_golden.py::gen_lpips)
N_TAPS = 5
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)          # BaseNet's buffers (networks.py:41-44)
PREFIX = "lpips_loss."     # the module's attribute in LatentDiffusion (ddpm.py:633-634): its keys in a REFace Lightning checkpoint
NPZ_REFUSED = ".npz paths are not supported: the perceptual distance compares images pair by pair"
CP = 8                     # 3 input channels stored in 8


# ------------------------------------------------------------------------------------------------
# layer arithmetic
# ------------------------------------------------------------------------------------------------
def layer_shapes(net, H, W):
    """[(kind, h, w, c)] after every entry of lpips_plan(net) for an H x W image; h or w < 1 where the image is too small."""
    out, c = [], 3
    for p in lpips_plan(net):
        if p[0] == "conv":
            _, _, _, c, k, s, pad = p
            H, W = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        elif p[0] == "pool":
            k = p[1]
            H, W = ((H - k) // 2 + 1 if H >= k else 0), ((W - k) // 2 + 1 if W >= k else 0)
        out.append((p[0], H, W, c))
    return out


def min_size(net):
    """The smallest side at which every tap of ``net`` still has a pixel: 31 for 'alex' (conv 11/4 pad 2 and two 3/2 pools: 31 -> 7 -> 3 ->
    1), 16 for 'vgg' (four 2/2 pools)."""
    n = 1
    while min(min(h, w) for _, h, w, _ in layer_shapes(net, n, n)) < 1:
        n += 1
    return n


def check_size(net, H, W):
    m = min_size(net)
    if H < m or W < m:
        raise ValueError(f"LPIPS('{net}'): a {H} x {W} image is too small: the net needs at least {m} x {m} pixels (its last tap would be empty)")


def bytes_per_image(net, H, W):
    """Bytes of the largest fp32 tensor of one image in the engine: the padded input or a layer output."""
    return 4 * max([H * W * CP] + [h * w * c for _, h, w, c in layer_shapes(net, H, W)])


def engine_batch_cap(net, H, W):
    """Pairs per engine run at the most: the engine holds 2 B images per tensor and no tensor may reach 2^31 bytes (VGG16 at 512 x 512: relu1_2
    is 67 MB per image -> 15 pairs)."""
    return max(1, (2 ** 31 - 1) // (2 * bytes_per_image(net, H, W)))


# ------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------
def seeded_lpips_state(net="alex"):
    """The seeded stand-in for the published weights: the ``lin`` weights are made non-negative, as the published ones are, and the two
    buffers hold the reference's constants."""
    sd = seeded_state_dict(lpips_param_specs(net), SEED)
    for k in sd:
        if k.startswith("lin."):
            sd[k] = sd[k].abs()
    sd["net.mean"] = torch.tensor(MEAN, dtype=F32).view(1, 3, 1, 1)
    sd["net.std"] = torch.tensor(STD, dtype=F32).view(1, 3, 1, 1)
    return sd


def load_lpips_state(ckpt, net="alex"):
    """State dict of the reference's ``LPIPS(net)`` module: the seeded weights when ``ckpt`` is None / "none"; else a checkpoint path or a
    dict that is either the module's plain state dict or a REFace Lightning checkpoint (the keys ``lpips_loss.*`` under ``state_dict``).
    Checked strictly against lpips_param_specs(net)."""
    if ckpt is None or (isinstance(ckpt, str) and ckpt.lower() == "none"):
        return seeded_lpips_state(net)
    origin = ckpt if isinstance(ckpt, (str, os.PathLike)) else "state dict"
    sd = torch.load(ckpt, map_location="cpu") if isinstance(ckpt, (str, os.PathLike)) else ckpt
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        full = sd["state_dict"]
        sd = {k[len(PREFIX):]: v for k, v in full.items() if k.startswith(PREFIX)}
        if not sd:
            raise RuntimeError(f"LPIPS checkpoint {origin}: its state_dict has no '{PREFIX}*' keys ({len(full)} keys of other modules): "
                               f"it was written without the perceptual loss")
    elif isinstance(sd, dict) and any(str(k).startswith(PREFIX) for k in sd):
        sd = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
    return check_lpips_state(sd, net, origin)


def check_lpips_state(sd, net="alex", origin="state dict"):
    specs = lpips_param_specs(net)
    unexpected = [k for k in sd if k not in specs]
    missing = [k for k in specs if k not in sd]
    if unexpected or missing:
        raise RuntimeError(f"LPIPS checkpoint {origin} does not match LPIPS(net_type='{net}'): missing {missing[:5]}, unexpected {unexpected[:5]}")
    bad = [k for k in sd if tuple(sd[k].shape) != tuple(specs[k])]
    if bad:
        raise RuntimeError(f"LPIPS checkpoint {origin}: shape mismatch for {[(k, tuple(sd[k].shape), specs[k]) for k in bad[:5]]}")
    return sd


# ------------------------------------------------------------------------------------------------
# host restatements (float64; for the tests only)
# ------------------------------------------------------------------------------------------------
def prep_host(image_u8):
    """ToTensor + Normalize(0.5, 0.5) on the host: uint8 [H, W, 3] -> fp32 [3, H, W] in [-1, 1], each step rounded to fp32."""
    x = torch.from_numpy(np.ascontiguousarray(image_u8).transpose(2, 0, 1).copy()).to(F32).div(255)
    return ((x - 0.5) / 0.5).numpy()


def zscore_host(x, sd=None, dtype=F64):
    """BaseNet.z_score (networks.py:50-51): (x - mean) / std in ``dtype``, the fp32 constants widened."""
    x = torch.as_tensor(x).to(dtype)
    mean = (sd["net.mean"] if sd is not None else torch.tensor(MEAN, dtype=F32).view(1, 3, 1, 1)).to(dtype)
    std = (sd["net.std"] if sd is not None else torch.tensor(STD, dtype=F32).view(1, 3, 1, 1)).to(dtype)
    return (x - mean) / std


def features_host(sd, x, net="alex", dtype=F64):
    """BaseNet.forward without the normalisation: x [B, 3, H, W] in [-1, 1] -> the five tap activations (post-ReLU) in ``dtype``, NCHW."""
    Fn = torch.nn.functional
    h = zscore_host(x, sd, dtype)
    taps = []
    for p in lpips_plan(net):
        if p[0] == "conv":
            _, i, _, _, _, s, pad = p
            h = Fn.relu(Fn.conv2d(h, sd[f"net.layers.{i}.weight"].to(dtype), sd[f"net.layers.{i}.bias"].to(dtype), stride=s, padding=pad))
        elif p[0] == "pool":
            h = Fn.max_pool2d(h, p[1], 2)
        else:
            taps.append(h)
    return taps


def normalize_host(f, eps=1e-10):
    """normalize_activation (utils.py:6-8) over the channel axis 1."""
    f = torch.as_tensor(f)
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True) + 1e-16) + eps)


def lpips_host(feats_x, feats_y, lins):
    """v[b, l] = mean_hw(sum_c w_l[c] (n(fx) - n(fy))^2) in float64 (lpips.py:32-33): feats NCHW per tap, lins the five ``lin`` weights
    (any shape holding C values) -> numpy float64 [B, L]."""
    cols = []
    for fx, fy, w in zip(feats_x, feats_y, lins):
        fx, fy = torch.as_tensor(fx).to(F64), torch.as_tensor(fy).to(F64)
        d = (normalize_host(fx) - normalize_host(fy)) ** 2
        cols.append((d * torch.as_tensor(w).to(F64).reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(cols, dim=1).numpy()


def score_host(v):
    """v float64 [B, L] -> dict(distances [B] = the layers summed in order, lpips_value = their mean = the module's scalar sum(v) / B, n)."""
    v = np.asarray(v, dtype=np.float64)
    d = np.zeros(v.shape[0], dtype=np.float64)
    for l in range(v.shape[1]):
        d = d + v[:, l]
    return {"distances": d, "lpips_value": float(np.sum(d) / v.shape[0]), "n": int(v.shape[0])}


def distances_host(sd, x, y, net="alex"):
    """x, y fp32 [B, 3, H, W] in [-1, 1] -> v float64 [B, L] through the restatements above."""
    return lpips_host(features_host(sd, x, net), features_host(sd, y, net), [sd[f"lin.{l}.1.weight"] for l in range(N_TAPS)])


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
class _LPIPSEngine:
    """Prepared launch list of LPIPS(net) for B pairs of H x W images: the prepared input [2 B, H, W, 8] (x in the first half, y in the
    second) -> vals fp64 [B, 5], d fp64 [B], totals fp64 [2]."""

    def __init__(self, sd, net, B, H, W, device):
        check_size(net, H, W)
        cap = engine_batch_cap(net, H, W)
        if not 1 <= B <= cap:
            raise ValueError(f"LPIPS('{net}') engine: {B} pairs of {H} x {W} (at most {cap}: no tensor may reach 2^31 bytes)")
        self.net, self.B, self.H, self.W, self.dev = net, B, H, W, device
        self.pool = _Pool(device)
        self.sd = {k: v.detach().to(device=device, dtype=F32) for k, v in sd.items()}
        self.launches = []
        # no split-K scratch: every GEMM then sums K in one fixed order whatever its M, so a pair's distance does not depend on the batch it is in
        self.ws = ops.new_workspace(device, nbytes=0)
        with ops.workspace_scope(self.ws):
            self._build()
        self.sd = None

    def _build(self):
        B, dev = self.B, self.dev
        self.x = torch.empty((2 * B, self.H, self.W, CP), dtype=F32, device=dev)          # rf_lpips_prep_* write it in place
        self.vals = torch.empty((B, N_TAPS), dtype=F64, device=dev)
        self.d = torch.empty((B,), dtype=F64, device=dev)
        self.totals = torch.empty((2,), dtype=F64, device=dev)
        pix = max(h * w for k, h, w, _ in layer_shapes(self.net, self.H, self.W) if k == "tap")
        self.scratch = torch.empty((B * min(ops.LPIPS_MAX_BLOCKS, pix),), dtype=F64, device=dev)
        h, first = self.x, True
        for p in lpips_plan(self.net):
            Bn, Hin, Win, _ = h.shape
            if p[0] == "conv":
                _, i, cin, cout, k, s, pad = p
                y = self.pool.get((Bn, (Hin + 2 * pad - k) // s + 1, (Win + 2 * pad - k) // s + 1, cout), F32)
                wp = ops.pack_conv_weight(self.sd[f"net.layers.{i}.weight"], F32, cin_pad=CP if first else None)
                self.launches.append(ops.conv2d(h, wp, y, self.sd[f"net.layers.{i}.bias"].contiguous(), ksize=k, stride=s, pad=(pad, pad), act=ops.ACT_RELU,
                                                name=f"net.layers.{i}"))
                first = False
            elif p[0] == "pool":
                k = p[1]
                y = self.pool.get((Bn, (Hin - k) // 2 + 1, (Win - k) // 2 + 1, h.shape[3]), F32)
                self.launches.append(ops.maxpool2d(h, y, k=k, name=f"maxpool{k}"))
            else:
                l = p[1]
                w = self.sd[f"lin.{l}.1.weight"].reshape(-1).contiguous()
                self.launches.append(ops.lpips_layer(h[:B], h[B:], w, self.scratch, self.vals, l, name=f"lpips_layer{l}"))
                continue
            # the producer's input goes back to the pool once its consumers are queued (launch order == allocation order); a tapped tensor
            # feeds its rf_lpips_layer before the next layer is queued, so it may be reused after that layer
            if h is not self.x:
                self.pool.put(h)
            h = y
        self.launches.append(ops.lpips_total(self.vals, self.d, self.totals, name="lpips_total"))

    def run(self):
        """The engine's input buffer ``x`` -> its ``vals`` / ``d`` / ``totals`` buffers (overwritten by the next run)."""
        ops.run(self.launches)
        return self.d


# what a scorer call returns, all on the device: d fp64 [B] = the distance of every pair, layers fp64 [B, 5] = v[b, l], totals fp64 [2] =
# (sum of d in index order, B): the reference module's scalar is totals[0] / totals[1]
LPIPSResult = collections.namedtuple("LPIPSResult", ["d", "layers", "totals"])
MAX_ENGINES = 4            # engines a scorer keeps (each holds its whole activation pool): the least recently used one is dropped beyond that


def _pairs_collate(items):
    return list(items)


class _PairFolder(torch.utils.data.Dataset):
    """(target bytes, result bytes) of every result, the target picked by the result's label."""

    def __init__(self, targets, results, labels, folder=None):
        folder = folder or _ImageFolder          # (--gpu_png_decode: pngdec.ByteFolder, whose items are file bytes)
        self.t, self.r, self.labels = folder(targets), folder(results), labels

    def __len__(self):
        return len(self.r)

    def __getitem__(self, i):
        return self.t[self.labels[i]], self.r[i]


def _runs(shapes, step):
    """Index chunks [(start, stop)]: runs of consecutive equal ``shapes`` cut into pieces of ``step(shape)`` at the most."""
    out, i, n = [], 0, len(shapes)
    while i < n:
        j = i + 1
        while j < n and shapes[j] == shapes[i]:
            j += 1
        s = step(shapes[i])
        out += [(a, min(j, a + s)) for a in range(i, j, s)]
        i = j
    return out


class LPIPSScorer:
    """LPIPS on the GPU.  ``state_dict``: the reference module's weights (load_lpips_state; checked strictly); ``net``: 'alex' or 'vgg';
    ``batch``: pairs per engine run (capped per image size by engine_batch_cap).  Engines are built per (pairs, height, width) and hold
    their activation buffers; the scorer keeps the MAX_ENGINES most recently used and drops the rest, so a folder of many sizes does not
    grow device memory without bound.  fp32 only."""

    def __init__(self, state_dict, net="alex", batch=16, device="cuda"):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("reface_amd LPIPS scoring runs on the GPU only (HIP kernels; there is no CPU fallback)")
        if not torch.cuda.is_available():
            raise RuntimeError("reface_amd LPIPS scoring runs on the GPU only (HIP kernels; there is no CPU fallback): no GPU is available")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        lpips_plan(net)          # refuses 'squeeze' and unknown names
        self.net = net
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be positive, not {batch}")
        self.sd = check_lpips_state(state_dict, net)
        self._engines = collections.OrderedDict()
        self.png_decoder = None          # a pngdec.PngDecoder: the folders' files are then decoded on the device (--gpu_png_decode)

    def step(self, hw):
        """Pairs per engine run for images of size ``hw``."""
        return min(self.batch, engine_batch_cap(self.net, hw[0], hw[1]))

    def engine(self, B, H, W):
        key = (B, H, W)
        eng = self._engines.get(key)
        if eng is None:
            while len(self._engines) >= MAX_ENGINES:
                self._engines.popitem(last=False)          # the allocator gets the buffers back once the queued work has run
            eng = self._engines[key] = _LPIPSEngine(self.sd, self.net, B, H, W, self.dev)
        self._engines.move_to_end(key)
        return eng

    def _finish(self, vals):
        d = torch.empty((vals.shape[0],), dtype=F64, device=self.dev)
        totals = torch.empty((2,), dtype=F64, device=self.dev)
        ops.lpips_total(vals, d, totals)()
        return d, totals

    def _run(self, x, y, hw, prep, vals):
        """One run of equal-size pairs through the engines in chunks: ``prep(items, out)`` fills half of an engine's input."""
        n = len(x)
        step = self.step(hw)
        for s in range(0, n, step):
            e = min(n, s + step)
            eng = self.engine(e - s, hw[0], hw[1])
            prep(x[s:e], eng.x[:e - s])
            prep(y[s:e], eng.x[e - s:])
            eng.run()
            vals[s:e] = eng.vals

    def _prep_u8(self, items, out):
        img = items if torch.is_tensor(items) else torch.stack([torch.as_tensor(t) for t in items])
        ops.lpips_prep_u8(img.to(self.dev, non_blocking=True).contiguous(), out)()

    @staticmethod
    def _hw_u8(t):
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"images are uint8 [H, W, 3], not {tuple(t.shape)}")
        return int(t.shape[0]), int(t.shape[1])

    @torch.no_grad()
    def distances_u8(self, images_x, images_y):
        """uint8 images [B, H, W, 3] twice (stacked tensors, or lists when sizes differ; host or device) -> LPIPSResult on the
        device.  Runs of consecutive pairs of equal size share an engine; the x and y of a pair must have the
        same size."""
        B = len(images_x)
        if len(images_y) != B or B == 0:
            raise ValueError(f"{B} images against {len(images_y)}: LPIPS compares pairs")
        shapes = []
        for i in range(B):
            a, b = self._hw_u8(torch.as_tensor(images_x[i])), self._hw_u8(torch.as_tensor(images_y[i]))
            if a != b:
                raise ValueError(f"pair {i}: the images differ in size ({a[0]} x {a[1]} against {b[0]} x {b[1]}); LPIPS does not resize")
            check_size(self.net, *a)
            shapes.append(a)
        vals = torch.empty((B, N_TAPS), dtype=F64, device=self.dev)
        i = 0
        while i < B:
            j = i + 1
            while j < B and shapes[j] == shapes[i]:
                j += 1
            self._run(images_x[i:j], images_y[i:j], shapes[i], self._prep_u8, vals[i:j])
            i = j
        d, totals = self._finish(vals)
        return LPIPSResult(d, vals, totals)

    @torch.no_grad()
    def distances(self, x, y):
        """fp32 NCHW device tensors [B, 3, H, W] in [-1, 1] twice -> LPIPSResult on the device."""
        for t in (x, y):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise ops._lib.RefaceHipError("reface_amd ops need device tensors (no CPU fallback)")
        if x.shape != y.shape:
            raise ValueError(f"LPIPS compares tensors of equal shape, not {tuple(x.shape)} and {tuple(y.shape)}")
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != F32 or y.dtype != F32 or x.shape[0] < 1:
            raise ValueError(f"LPIPS takes fp32 tensors [B, 3, H, W], not {x.dtype} {tuple(x.shape)}")
        B, _, H, W = x.shape
        check_size(self.net, H, W)
        vals = torch.empty((B, N_TAPS), dtype=F64, device=self.dev)
        self._run(x.contiguous(), y.contiguous(), (H, W), lambda t, out: ops.lpips_prep_f32(t.contiguous(), out)(), vals)
        d, totals = self._finish(vals)
        return LPIPSResult(d, vals, totals)

    def score_folders(self, paths, num_workers=0):
        """paths = (targets, results).  Both folders are listed in natural order; a result's label (the last number of its name minus the
        folder's smallest) is a position in the target list: that target is the image the result is compared with.  Returns
        dict(lpips_value = the mean of the distances, distances fp64 [M], labels, images = 2 M (the images that went through the net),
        images_per_s, seconds)."""
        from PIL import Image
        for p in paths:
            if str(p).endswith(".npz"):
                raise ValueError(f"{p}: {NPZ_REFUSED}")
            if not os.path.exists(p):
                raise RuntimeError("Invalid path: %s" % p)
        targets, results = list_images(paths[0]), list_images(paths[1])
        if not targets or not results:
            raise ValueError(f"no image files in {paths[0] if not targets else paths[1]}")
        labels = parse_labels_last(results)
        if len(labels) != len(results):
            raise ValueError("a result file name carries no number: results and labels would be misaligned")
        if min(labels) < 0 or max(labels) >= len(targets):
            raise IndexError(f"labels must be {len(results)} indices into the {len(targets)} targets")
        # sizes from the file headers: pairs are checked and the engines built before the clock starts (`seconds` / `images_per_s` are decode +
        # upload + prep + net + distance, not engine construction)
        def size(f):
            with Image.open(f) as im:
                return im.size[1], im.size[0]
        tsize = {l: size(targets[l]) for l in sorted(set(labels))}
        shapes = []
        for f, l in zip(results, labels):
            hw = size(f)
            if hw != tsize[l]:
                raise ValueError(f"{f}: {hw[0]} x {hw[1]} differs in size from its target {targets[l]} ({tsize[l][0]} x {tsize[l][1]}); LPIPS does not resize")
            check_size(self.net, *hw)
            shapes.append(hw)
        chunks = _runs(shapes, self.step)
        first = list(dict.fromkeys((b - a,) + shapes[a] for a, b in chunks))[:MAX_ENGINES]
        for key in reversed(first):          # (a folder of more shapes than the scorer keeps engines builds the later ones inside the clock)
            self.engine(*key)
        vals = torch.empty((len(results), N_TAPS), dtype=F64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        dec = self.png_decoder
        folder = None
        if dec is not None:
            from . import pngdec
            folder = lambda files: pngdec.ByteFolder(files, "RGB", getattr(dec, "kinds", ("png",)))          # noqa: E731
        loader = torch.utils.data.DataLoader(_PairFolder(targets, results, labels, folder), batch_sampler=[list(range(a, b)) for a, b in chunks],
                                             num_workers=num_workers, collate_fn=_pairs_collate)
        with torch.no_grad():
            for (a, b), items in zip(chunks, loader):
                ts, rs = [t for t, _ in items], [r for _, r in items]
                if dec is not None:          # the workers read bytes: both sides of the chunk are decoded on the device in one batch
                    outs = dec.decode(ts + rs, "RGB")
                    ts, rs = outs[:len(ts)], outs[len(ts):]
                self._run(ts, rs, shapes[a], self._prep_u8, vals[a:b])
            d, totals = self._finish(vals)
        t = totals.cpu().numpy()
        torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        n_img = 2 * len(results)
        return {"lpips_value": float(t[0] / t[1]), "distances": d.cpu().numpy(), "labels": [int(l) for l in labels],
                "images": n_img, "images_per_s": n_img / dt, "seconds": dt}
