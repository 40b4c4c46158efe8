"""Seeded inputs of the pose-score fixture (tests/golden/pose.npz): shared by tools/gen_golden.py:gen_pose, which runs the reference on
them, and by tests/test_pose_{cpu,gpu}.py, which regenerate them (only outputs are stored).

10 target and 8 result images are low-frequency random fields, rendered as tests/idscore_inputs.py renders its faces (float64 numpy on
exactly rounded operations: the bytes are the same on every machine), at MIXED sizes: 256 x 256 and 300 x 260 (downscales to 224), 224 x 224
(the identity) and 57 x 40 (an upscale).  What the file names are chosen to expose:
  * every name carries two numbers (``7_00503.png``): the pose label is the LAST one minus the folder's smallest last one, the identity
    metric's label the first one -- the two labellings disagree on every result;
  * the first numbers put ``2`` before ``10`` under natural order only (lexicographic order would start with ``10_``);
  * a result's label is a POSITION in the sorted target list; several results point at the same target and the labels are permuted, so
    pairing results with targets by position gives another value.
"""
import os

import numpy as np

from idscore_inputs import _field, _render

SIZES = {"a": (256, 256), "b": (300, 260), "c": (224, 224), "d": (57, 40)}          # (height, width)
TGT_SIZES = "aabbcdabca"                     # runs of equal sizes and single images: prep_u8 groups consecutive equal shapes
RES_SIZES = "aaabdcca"
TGT_FIRST = [2, 2, 2, 3, 3, 9, 10, 10, 11, 11]          # first numbers of the target names, in natural order
TGT_LAST0 = 100                                          # target k (position k in natural order) is <first>_<100 + k>.png
RES_FIRST = [2, 3, 4, 6, 7, 9, 10, 11]                   # first numbers of the result names: first-number labels would be 0 1 2 4 5 7 8 9
RES_LABELS = [3, 0, 7, 3, 9, 1, 7, 5]                    # last number - 500: the position of each result's target
RES_LAST0 = 500
PREP_SAMPLES = {"tgt": [0, 5]}                           # the images whose prepared tensors the fixture stores: a downscale and the upscale


def build():
    """dict(tgt_images, res_images: lists of uint8 arrays [H, W, 3]; labels: [8] pose labels of the results; tgt_names, res_names: file
    names whose natural order is the list order)."""
    tgt = [_render(_field(5000 + k), SIZES[s]) for k, s in enumerate(TGT_SIZES)]
    res = [_render(_field(6100 + i), SIZES[s]) for i, s in enumerate(RES_SIZES)]
    return {"tgt_images": tgt, "res_images": res, "labels": np.array(RES_LABELS, dtype=np.int64),
            "tgt_names": [f"{a}_{TGT_LAST0 + k:05d}.png" for k, a in enumerate(TGT_FIRST)],
            "res_names": [f"{a}_{RES_LAST0 + l:05d}.png" for a, l in zip(RES_FIRST, RES_LABELS)]}


def first_number_labels():
    """What the identity metric's labelling (first number minus the folder's smallest) would make of the result names."""
    return [a - min(RES_FIRST) for a in RES_FIRST]


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
