"""Seeded inputs of the identity-score fixture (tests/golden/idscore.npz): shared by tools/gen_golden.py:gen_idscore, which runs the
reference on them, and by tests/test_idscore_{cpu,gpu}.py, which regenerate them (only outputs are stored).

16 source ("gallery") faces are low-frequency random fields: 14 x 14 normal noise per channel, bilinear to the image size, clamped and
quantised to 8 bits.  16 results are mixed in the 14 x 14 domain and rendered the same way:
   8  easy     0.7 gallery[label] + 0.3 noise                    (label at rank 1)
   4  second   0.6 gallery[other] + 0.4 gallery[label]           (label at rank 2: a top-5 hit, not a top-1 hit)
   4  absent   noise only                                        (label anywhere)
so neither accuracy is 0 or 1.  Every image has a label map of another size with labels inside and outside every --dataset's preserve
list, so the mask and both resizes matter.  All arithmetic below is float64 numpy on exactly rounded operations (no library resampler):
the bytes are the same on every machine.  File names are chosen so that natural order differs from lexicographic order.
"""
import os

import numpy as np

from reface_amd.params import seeded_randn

N_SRC = 16
SRC_HW, SRC_LAB_HW = (160, 144), (120, 100)
RES_HW, RES_LAB_HW = (128, 128), (96, 112)
DATASET = "celeba"
# (kind, label, other): in the natural order of the result file names below
RESULTS = [("easy", l, None) for l in range(8)] + [("second", l, (l + 3) % N_SRC) for l in range(8, 12)] + [("absent", l, None) for l in range(12, 16)]
PREP_SAMPLES = {"src": [0, 7], "res": [0, 9, 14]}          # the images whose prepared tensors the fixture stores


def _field(seed):
    return seeded_randn((3, 14, 14), seed).numpy().astype(np.float64)


def _upsample(f, h, w):
    """[3, 14, 14] float64 -> [3, h, w]: bilinear at half-pixel centres, edge-clamped, written out (exactly rounded operations only)."""
    def taps(n_in, n_out):
        c = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
        c = np.clip(c, 0.0, n_in - 1.0)
        i0 = np.floor(c).astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, c - i0
    y0, y1, wy = taps(f.shape[1], h)
    x0, x1, wx = taps(f.shape[2], w)
    rows = f[:, y0, :] * (1.0 - wy)[None, :, None] + f[:, y1, :] * wy[None, :, None]
    return rows[:, :, x0] * (1.0 - wx)[None, None, :] + rows[:, :, x1] * wx[None, None, :]


def _render(f, hw):
    x = np.clip(0.5 + 0.25 * _upsample(f, *hw), 0.0, 1.0)
    return np.floor(x * 255.0 + 0.5).astype(np.uint8).transpose(1, 2, 0).copy()          # HWC


def _label_map(seed, hw):
    """A face-like label map: background 0, a hair band 13 above and a neck block 17 below (neither preserved by any dataset), and an
    ellipse of skin 1 holding nose 2, two eye boxes 4 / 5, brows 6 / 7 (celeba only), a 3 block (ffhq only) and lips 11 / 12."""
    h, w = hw
    r = seeded_randn((4,), seed).numpy().astype(np.float64)
    cy, cx = h * (0.5 + 0.04 * r[0]), w * (0.5 + 0.04 * r[1])
    ry, rx = h * (0.40 + 0.02 * r[2]), w * (0.36 + 0.02 * r[3])
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = (yy - cy) / ry, (xx - cx) / rx
    lab = np.zeros((h, w), dtype=np.uint8)
    lab[yy < h * 0.12] = 13
    lab[(yy > h * 0.9) & (np.abs(v) < 0.5)] = 17
    lab[u * u + v * v <= 1.0] = 1
    box = lambda u0, u1, v0, v1: (u >= u0) & (u < u1) & (v >= v0) & (v < v1)
    lab[box(-0.15, 0.25, -0.12, 0.12)] = 2
    lab[box(-0.40, -0.25, -0.55, -0.20)] = 4
    lab[box(-0.40, -0.25, 0.20, 0.55)] = 5
    lab[box(-0.55, -0.47, -0.55, -0.20)] = 6
    lab[box(-0.55, -0.47, 0.20, 0.55)] = 7
    lab[box(-0.05, 0.10, 0.45, 0.70)] = 3
    lab[box(0.40, 0.48, -0.30, 0.30)] = 11
    lab[box(0.48, 0.58, -0.30, 0.30)] = 12
    return lab


def build():
    """dict(src_images, src_labels, res_images, res_labels: lists of uint8 arrays; labels: [16] identity labels of the results;
    src_names, res_names: file names whose natural order is the list order)."""
    gallery = [_field(1000 + k) for k in range(N_SRC)]
    res_fields = []
    for i, (kind, l, other) in enumerate(RESULTS):
        noise = _field(2100 + i)
        if kind == "easy":
            res_fields.append(0.7 * gallery[l] + 0.3 * noise)
        elif kind == "second":
            res_fields.append(0.6 * gallery[other] + 0.4 * gallery[l])
        else:
            res_fields.append(noise)
    return {"src_images": [_render(f, SRC_HW) for f in gallery], "src_labels": [_label_map(3000 + k, SRC_LAB_HW) for k in range(N_SRC)],
            "res_images": [_render(f, RES_HW) for f in res_fields], "res_labels": [_label_map(4000 + i, RES_LAB_HW) for i in range(len(RESULTS))],
            "labels": np.array([l for _, l, _ in RESULTS], dtype=np.int64),
            "src_names": [f"{95 + k}.png" for k in range(N_SRC)],                                   # 95 .. 110: "100.png" < "95.png" as strings
            "res_names": [f"{7 + l}_{kind}.png" for kind, l, _ in RESULTS]}                          # 7 .. 22; label = number - 7


def write_folders(root, data=None):
    """The four folders of the CLI under ``root`` as PNGs (lossless): returns [sources, results, source masks, result masks]."""
    from PIL import Image
    d = data or build()
    paths = [os.path.join(root, n) for n in ("src", "results", "src_mask", "target_mask")]
    for p in paths:
        os.makedirs(p, exist_ok=True)
    for name, img, lab in zip(d["src_names"], d["src_images"], d["src_labels"]):
        Image.fromarray(img).save(os.path.join(paths[0], name))
        Image.fromarray(lab).save(os.path.join(paths[2], name))
    for name, img, lab in zip(d["res_names"], d["res_images"], d["res_labels"]):
        Image.fromarray(img).save(os.path.join(paths[1], name))
        Image.fromarray(lab).save(os.path.join(paths[3], name))
    return paths
