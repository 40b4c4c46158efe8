"""Seeded inputs of the expression-score fixture (tests/golden/expr.npz): shared by tools/gen_golden.py:gen_expr, which runs the reference on
them, and by tests/test_expr_{cpu,gpu}.py, which regenerate them (only outputs are stored).

10 target and 8 result images are low-frequency random fields rendered as tests/idscore_inputs.py renders its faces, with per-pixel seeded
noise blended in (structure for the network to tell images apart, high frequencies for the bicubic resampler), at MIXED sizes: 512 x 512
(the identity: most of them), one 1024 x 1024 per folder (the 2:1 downscale), 600 x 540 (a non-square downscale) and 57 x 40 (an upscale).
What the file names are chosen to expose:
  * every name carries two numbers (``10_00505.png``): the expression label is the FIRST one minus the folder's smallest first one, the pose
    metric's label the last one -- the two labellings disagree;
  * the reference lists a folder with plain ``sorted()``: ``10_`` sorts before ``8_``, so the sorted order is not the natural one and a
    result's label is not its position; labels repeat and both ends (0 and 9) occur;
  * a result's label is a POSITION in the sorted target list, whatever the targets are called: pairing by position gives another value.
"""
import os

import numpy as np

from idscore_inputs import _field, _upsample
from reface_amd.params import seeded_randn

SIZES = {"a": (512, 512), "b": (1024, 1024), "c": (600, 540), "d": (57, 40)}          # (height, width)
TGT_SIZES = "aabacdaaca"                     # runs of equal sizes and single images: prep_u8 groups consecutive equal shapes
RES_SIZES = "aacadaab"
# names in sorted() order (the list order); "100_" < "98_" as strings
TGT_FIRST = [100, 101, 102, 103, 104, 105, 106, 107, 98, 99]
TGT_LAST0 = 300                                          # target k (position k in sorted order) is <first>_<300 + k>.png
RES_FIRST = [10, 10, 13, 15, 17, 8, 9, 9]                # first numbers of the result names in sorted() order: labels 2 2 5 7 9 0 1 1
RES_LAST = [500, 505, 503, 508, 501, 509, 504, 506]      # last numbers: last-number labels would be 0 5 3 8 1 9 4 6
RES_LABELS = [a - min(RES_FIRST) for a in RES_FIRST]


def _render(seed, hw):
    """uint8 [H, W, 3]: 0.5 + 0.25 * smooth field + 0.06 * per-pixel noise, clamped and rounded."""
    h, w = hw
    smooth = _upsample(_field(seed), h, w)
    noise = seeded_randn((3, h, w), seed + 50000).numpy().astype(np.float64)
    x = np.clip(0.5 + 0.25 * smooth + 0.06 * noise, 0.0, 1.0)
    return np.floor(x * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0).copy()


def build():
    """dict(tgt_images, res_images: lists of uint8 arrays [H, W, 3]; labels: [8] expression labels of the results; tgt_names, res_names: file
    names whose sorted() order is the list order)."""
    tgt = [_render(7000 + k, SIZES[s]) for k, s in enumerate(TGT_SIZES)]
    res = [_render(8100 + i, SIZES[s]) for i, s in enumerate(RES_SIZES)]
    d = {"tgt_images": tgt, "res_images": res, "labels": np.array(RES_LABELS, dtype=np.int64),
         "tgt_names": [f"{a}_{TGT_LAST0 + k:05d}.png" for k, a in enumerate(TGT_FIRST)],
         "res_names": [f"{a}_{l:05d}.png" for a, l in zip(RES_FIRST, RES_LAST)]}
    assert d["tgt_names"] == sorted(d["tgt_names"]) and d["res_names"] == sorted(d["res_names"])
    return d


def last_number_labels():
    """What the pose metric's labelling (last number minus the folder's smallest) would make of the result names."""
    return [l - min(RES_LAST) for l in RES_LAST]


def write_folders(root, data=None):
    """The two folders of the CLI under ``root`` as PNGs (lossless): returns [targets, results]."""
    from PIL import Image
    d = data or build()
    paths = [os.path.join(root, n) for n in ("targets", "results")]
    for p in paths:
        os.makedirs(p, exist_ok=True)
    for name, img in zip(d["tgt_names"], d["tgt_images"]):
        Image.fromarray(img).save(os.path.join(paths[0], name))
    for name, img in zip(d["res_names"], d["res_images"]):
        Image.fromarray(img).save(os.path.join(paths[1], name))
    return paths
