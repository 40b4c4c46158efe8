"""Seeded inputs of the LPIPS fixture (tests/golden/lpips.npz): shared by tools/gen_golden.py:gen_lpips, which runs the reference on them,
and by tests/test_lpips_{cpu,gpu}.py, which regenerate them (only outputs are stored).

Images are low-frequency random fields, rendered as tests/idscore_inputs.py renders its faces (float64 numpy on exactly rounded operations:
the bytes are the same on every machine).  Five cases of four pairs each: (net, height, width) below -- 64 x 64 the plain case, 70 x 61 odd
sizes where a ceil-mode pool would keep a row and a column more, 35 x 33 close to AlexNet's minimum (its last three taps are 1 x 1).  In a
case, pairs 0..2 are ordinary (y = a mix of x's field with another field, the share of the other one growing), pair 3 is near-identical:
y = x with NEAR_BYTES bytes changed by 1.

The folder layout has the two-number names of the pose fixture (``7_00503.png``): the label of a result is the LAST number minus the
folder's smallest last one and is a POSITION in the naturally sorted target list.  The labels are permuted and several results point at one
target, so pairing results with targets by position gives another value.  A result has its target's size; the sizes are mixed.
"""
import os

import numpy as np

from idscore_inputs import _field, _render

CASES = [("alex", 64, 64), ("alex", 70, 61), ("alex", 35, 33), ("vgg", 64, 64), ("vgg", 35, 33)]
PAIRS = 4
NEAR = 3                                     # index of the near-identical pair of every case
NEAR_BYTES = 6
MIX = (0.5, 0.3, 0.15)                     # share of the other field in y for the ordinary pairs
FEATURE_CASE, FEATURE_PAIR = 2, 1            # the ('alex', 35, 33) pair whose normalised tap features the fixture stores

FOLDER_NET = "alex"
FOLDER_SIZES = {"a": (64, 64), "b": (70, 61)}
TGT_SIZES = "aabbab"
TGT_FIRST = [2, 2, 3, 9, 10, 11]             # first numbers of the target names, in natural order ("10_" would lead lexicographically)
TGT_LAST0 = 100
RES_FIRST = [2, 3, 4, 6, 9, 10]
RES_LABELS = [1, 4, 3, 3, 0, 2]              # last number - 500: the position of each result's target.  Permuted inside the size classes, so
                                             # the (wrong) pairing by position is between images of equal size as well and can be computed
RES_LAST0 = 500
RES_MIX = (0.5, 0.3, 0.2, 0.1, 0.4, 0.15)


def case_name(c):
    net, h, w = CASES[c]
    return f"{net}_{h}x{w}"


def _near(x, seed):
    """x with NEAR_BYTES bytes moved by one step (towards the middle of the range, so none wraps)."""
    y = x.copy()
    flat = y.reshape(-1)
    r = np.random.RandomState(seed)
    for i in r.choice(flat.size, NEAR_BYTES, replace=False):
        flat[i] = flat[i] + 1 if flat[i] < 128 else flat[i] - 1
    return y


def build_case(c):
    """(x, y): two lists of PAIRS uint8 arrays [H, W, 3]."""
    _, h, w = CASES[c]
    xs, ys = [], []
    for k in range(PAIRS):
        f = _field(7000 + 10 * c + k)
        x = _render(f, (h, w))
        if k == NEAR:
            y = _near(x, 7500 + c)
        else:
            y = _render((1.0 - MIX[k]) * f + MIX[k] * _field(7200 + 10 * c + k), (h, w))
        xs.append(x)
        ys.append(y)
    return xs, ys


def build_folders():
    """dict(tgt_images, res_images: lists of uint8 arrays [H, W, 3]; labels: [6] labels of the results; tgt_names, res_names: file names
    whose natural order is the list order)."""
    fields = [_field(7800 + k) for k in range(len(TGT_SIZES))]
    tgt = [_render(f, FOLDER_SIZES[s]) for f, s in zip(fields, TGT_SIZES)]
    res = [_render((1.0 - m) * fields[l] + m * _field(7900 + i), FOLDER_SIZES[TGT_SIZES[l]]) for i, (l, m) in enumerate(zip(RES_LABELS, RES_MIX))]
    return {"tgt_images": tgt, "res_images": res, "labels": np.array(RES_LABELS, dtype=np.int64),
            "tgt_names": [f"{a}_{TGT_LAST0 + k:05d}.png" for k, a in enumerate(TGT_FIRST)],
            "res_names": [f"{a}_{RES_LAST0 + l:05d}.png" for a, l in zip(RES_FIRST, RES_LABELS)]}


def write_folders(root, data=None):
    """The two folders of the CLI under ``root`` as PNGs (lossless): returns [targets, results]."""
    from PIL import Image
    d = data or build_folders()
    paths = [os.path.join(root, n) for n in ("targets", "results")]
    for p in paths:
        os.makedirs(p, exist_ok=True)
    for name, img in zip(d["tgt_names"], d["tgt_images"]):
        Image.fromarray(img).save(os.path.join(paths[0], name))
    for name, img in zip(d["res_names"], d["res_images"]):
        Image.fromarray(img).save(os.path.join(paths[1], name))
    return paths
