"""Seeded inputs of the FID fixture (tests/golden/fid.npz): shared by tools/gen_golden.py:gen_fid, which runs the reference on them, and by
tests/test_fid_{cpu,gpu}.py, which regenerate them (only outputs are stored).

Two populations of 48 images, "dataset" and "results": low-frequency random fields rendered as tests/expr_inputs.py renders its images
(per-pixel seeded noise blended in: high frequencies for the bicubic resampler), the results with a colour shift and more contrast, so the
two feature clouds differ in mean and in covariance.  Sizes are MIXED, every one a path of the preprocess of its own:
  512 x 512 (the 16:7 downscale), 224 x 224 (the identity), 300 x 260 and 260 x 300 (a crop along either axis), 57 x 40 (an upscale),
  224 x 225 and 224 x 227 (crop offsets 0.5 and 1.5: Python's rounding takes 0 and 2),
and each population holds one ``L`` image and one ``RGBA`` image whose alpha is 255 everywhere.  48 images per side keep the 32 x 32
covariances of the fixture tower at full rank.
"""
import os

import numpy as np

from idscore_inputs import _field, _upsample
from reface_amd.params import seeded_randn

SIZES = {"a": (512, 512), "b": (224, 224), "c": (300, 260), "d": (260, 300), "e": (57, 40), "f": (224, 225), "g": (224, 227)}          # (height, width)
# runs of equal sizes and single images: the scorer groups consecutive equal shapes into one launch
DATASET_SIZES = ("abbbcdbbbefbbbg" * 4)[:48]
RESULT_SIZES = ("bbabbcbdbebbfbg" * 4)[:48]
L_AT, RGBA_AT = 5, 9          # positions (in both populations) of the L and of the all-255 RGBA image
N = 48
PREP_SAMPLES = (0, 5, 9)          # dataset images whose prepared tensors the fixture stores: 512 x 512, the L (260 x 300), the RGBA (57 x 40)
B32_IMAGES = (0, 1, 4, 9)         # dataset images the ViT-B/32-sized tower of the fixture ran on
assert len(DATASET_SIZES) == len(RESULT_SIZES) == N


def _render(seed, hw, shift, contrast):
    """uint8 [H, W, 3]: 0.5 + shift[c] + contrast * smooth field + 0.06 * per-pixel noise, clamped and rounded."""
    h, w = hw
    smooth = _upsample(_field(seed), h, w)
    noise = seeded_randn((3, h, w), seed + 50000).numpy().astype(np.float64)
    x = np.clip(0.5 + np.asarray(shift, dtype=np.float64)[:, None, None] + contrast * smooth + 0.06 * noise, 0.0, 1.0)
    return np.floor(x * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0).copy()


def _population(seed0, sizes, shift, contrast):
    out = []
    for i, s in enumerate(sizes):
        im = _render(seed0 + i, SIZES[s], shift, contrast)
        if i == L_AT:
            im = im[:, :, 1].copy()                                                        # mode L
        elif i == RGBA_AT:
            im = np.concatenate([im, np.full(im.shape[:2] + (1,), 255, np.uint8)], 2)      # mode RGBA, alpha 255 everywhere
        out.append(im)
    return out


def build():
    """dict(dataset, results: lists of 48 uint8 arrays [H, W, 3] (one [H, W], one [H, W, 4] each); dataset_names, result_names: file names
    in the list order, which is their sorted order)."""
    return {"dataset": _population(9000, DATASET_SIZES, (0.0, 0.0, 0.0), 0.25),
            "results": _population(9500, RESULT_SIZES, (0.04, -0.03, 0.02), 0.30),
            "dataset_names": [f"{i:05d}.png" for i in range(N)], "result_names": [f"{i:05d}.png" for i in range(N)]}


def rgb(image):
    """The uint8 RGB bytes the device preparation takes for an image of build(): L replicated, the all-255 alpha dropped."""
    if image.ndim == 2:
        return np.repeat(image[:, :, None], 3, axis=2)
    return np.ascontiguousarray(image[:, :, :3])


def write_folders(root, data=None):
    """The two folders of the CLI under ``root`` as PNGs (lossless; the mode follows the array's shape): returns [dataset, results]."""
    from PIL import Image
    d = data or build()
    paths = [os.path.join(root, n) for n in ("dataset", "results")]
    for p, names, images in ((paths[0], d["dataset_names"], d["dataset"]), (paths[1], d["result_names"], d["results"])):
        os.makedirs(p, exist_ok=True)
        for name, img in zip(names, images):
            Image.fromarray(img).save(os.path.join(p, name))
    return paths
