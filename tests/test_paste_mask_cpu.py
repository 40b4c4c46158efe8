"""The masked paste without a GPU: the numpy restatements of rf_paste_alpha_u8 / rf_paste_back_alpha_u8 (tests/paste_mask_refs.py) against
PIL and against hand-computed vectors, the CLI's flags and refusals, PasteMask's argument checks and the exports."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import paste_mask_refs as R  # noqa: E402
from reface_amd.pasteback import alignment_coefficients  # noqa: E402

EXTREMES = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)


def _random_quad(rng, W, H, kind):
    """A rotated and skewed quad, in frame coordinates: inside the frame, partly outside it, or wholly outside."""
    r = min(W, H) * rng.uniform(0.2, 0.45)
    t = rng.uniform(0, 2 * np.pi)
    Rm = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    q = np.array([[-r, -r], [-r, r], [r, r], [r, -r]]) @ Rm.T + rng.uniform(-0.25, 0.25, (4, 2)) * r
    centre = {"inside": [W * 0.5, H * 0.5], "partly": [W * rng.choice([0.0, 1.0]), H * rng.uniform(0.2, 0.8)], "outside": [3.0 * W, 3.0 * H]}[kind]
    return q + centre


def _mask(rng, S, kind):
    if kind == "random":
        m = rng.integers(0, 256, (S, S), dtype=np.uint8)
        m.reshape(-1)[:EXTREMES.size * 3] = np.tile(EXTREMES, 3)
        sel = rng.random((S, S)) < 0.3
        m[sel] = rng.choice(EXTREMES, int(sel.sum()))
        return m
    if kind == "blocks":          # runs of alpha 0 and 255 beside partial values
        m = rng.choice(EXTREMES, (S // 4 + 1, S // 4 + 1)).repeat(4, 0).repeat(4, 1)[:S, :S]
        return np.ascontiguousarray(m)
    yy, xx = np.mgrid[:S, :S]
    return np.clip(255.0 * (1.2 - np.hypot(yy - S / 2, xx - S / 2) / (S * 0.4)), 0, 255).astype(np.uint8)          # a smooth ramp


@pytest.mark.parametrize("seed", range(12))
def test_paste_restatement_is_pil(seed):
    rng = np.random.default_rng(100 + seed)
    W, H, S = int(rng.integers(40, 130)), int(rng.integers(30, 100)), int(rng.choice([16, 33, 64]))
    Cf = 3 + seed % 2
    kind = ("inside", "partly", "partly", "outside")[seed % 4]
    crop = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    alpha = _mask(rng, S, ("random", "blocks", "ramp")[seed % 3])
    frame = rng.integers(0, 256, (H, W, Cf), dtype=np.uint8)          # (RGBA frames: arbitrary alpha, 0 and 255 among them)
    if Cf == 4:
        frame[:4, :, 3] = np.tile(EXTREMES, W)[:4 * W].reshape(4, W)
    c = alignment_coefficients(_random_quad(rng, W, H, kind), S)
    for Co in (3, 4):
        ref = R._pil_paste_alpha(crop, alpha, c, frame, Co)
        got = R.paste_alpha(crop, alpha, c, frame, Co)
        assert got.shape == ref.shape and np.array_equal(got, ref), (Co, int((got != ref).sum()))
    touched = (R._pil_paste_alpha(crop, alpha, c, frame, 4)[..., :3] != frame[..., :3]).any()
    assert touched == (kind != "outside")
    # no support, no change: the frame bit for bit (its alpha too)
    keep = R.paste_alpha(crop, np.zeros_like(alpha), c, frame, 4)
    assert np.array_equal(keep[..., :Cf], frame) and (Cf == 4 or (keep[..., 3] == 255).all())
    zero = R.taps_alpha_zero(alpha, c, H, W)
    full = R.paste_alpha(crop, alpha, c, frame, 4)
    assert np.array_equal(full[zero][:, :Cf], frame[zero])


def test_paste_restatement_with_full_alpha_is_the_plain_paste():
    from test_paste_back_gpu import _pil_paste, _quads
    rng = np.random.default_rng(3)
    W, H, S = 97, 53, 64
    crop, frame = rng.integers(0, 256, (S, S, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    for q in _quads(W, H):
        c = alignment_coefficients(q, S)
        assert np.array_equal(R.paste_alpha(crop, np.full((S, S), 255, np.uint8), c, frame, 4), _pil_paste(crop, c, frame, 4))


@pytest.mark.parametrize("n,S", [(32, 64), (37, 37), (37, 100), (512, 1024), (5, 64), (1, 7)])
def test_resize_restatement_is_pil(n, S):
    rng = np.random.default_rng(n + S)
    m = rng.integers(0, 256, (n, n), dtype=np.uint8)
    m.reshape(-1)[:min(6, n * n)] = EXTREMES[:min(6, n * n)]
    assert np.array_equal(R.resize_bilinear_u8(m, S), np.asarray(Image.fromarray(m).resize((S, S), Image.BILINEAR)))


def test_alpha_steps_by_hand():
    lut = np.zeros(256, np.uint8)
    lut[[2, 7]] = 1
    # step 1: the LUT
    lab = np.array([[0, 2, 7], [1, 255, 2], [7, 7, 3]], dtype=np.uint8)
    assert R.mask_of_labels(lab, lut).tolist() == [[0, 255, 255], [0, 0, 255], [255, 255, 0]]
    # a single set pixel at (3, 4) of a 9 x 9 map, d = 1: the 3 x 3 square around it
    lab = np.zeros((9, 9), np.uint8)
    lab[3, 4] = 2
    m1 = R.dilate(R.mask_of_labels(lab, lut), 1)
    want = np.zeros((9, 9), np.uint8)
    want[2:5, 3:6] = 255
    assert np.array_equal(m1, want)
    # d = 0 is the identity, r = 0 skips the feather whatever `passes` says
    assert np.array_equal(R.dilate(R.mask_of_labels(lab, lut), 0), R.mask_of_labels(lab, lut))
    assert np.array_equal(R.feather(m1, 0, 3), m1)
    assert np.array_equal(R.alpha_small(lab, lut, 0, 0, 1), R.mask_of_labels(lab, lut))
    # one box pass r = 1 along x of the 3-wide run: sums 255, 510, 765, 510, 255 -> (s + 1) // 3 = 85, 170, 255, 170, 85
    h = R.box_1d(m1, 1, -1)
    assert h[3].tolist() == [0, 0, 85, 170, 255, 170, 85, 0, 0] and h[2].tolist() == h[3].tolist() == h[4].tolist() and not h[1].any()
    # then along y: column 4 holds 255 in rows 2 .. 4 -> the same profile down the column; the corner (1, 2): (85 + 1) // 3 = 28
    v = R.box_1d(h, 1, -2)
    assert v[:, 4].tolist() == [0, 85, 170, 255, 170, 85, 0, 0, 0] and v[1, 2] == 28 and v[2, 2] == (85 + 85 + 1) // 3 == 57
    assert np.array_equal(R.feather(m1, 1, 1), v)
    # a run touching the border: positions outside count as 0 in the sum but the divisor stays 2r + 1, so alpha falls off at the border
    row = np.zeros((1, 8), np.uint8)
    row[0, :3] = 255
    assert R.box_1d(row, 2, -1)[0].tolist() == [(765 + 2) // 5, (765 + 2) // 5, (765 + 2) // 5, (510 + 2) // 5, (255 + 2) // 5, 0, 0, 0]
    assert R.box_1d(row, 2, -1)[0].tolist() == [153, 153, 153, 102, 51, 0, 0, 0]
    assert R.box_1d(np.full((1, 8), 255, np.uint8), 2, -1)[0].tolist() == [153, 204, 255, 255, 255, 255, 204, 153]
    # the dilation is restricted to the map: a pixel in the corner grows into a (d + 1)^2 square
    lab = np.zeros((6, 6), np.uint8)
    lab[0, 5] = 7
    want = np.zeros((6, 6), np.uint8)
    want[:3, 3:] = 255
    assert np.array_equal(R.dilate(R.mask_of_labels(lab, lut), 2), want)
    # radii larger than the map
    assert (R.dilate(R.mask_of_labels(lab, lut), 64) == 255).all()
    assert R.box_1d(np.full((1, 4), 255, np.uint8), 64, -1)[0].tolist() == [(4 * 255 + 64) // 129] * 4


def _exit_message(argv):
    import inference_swap_video as cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code not in (0, None)
    return str(e.value.code)


def test_cli_flags_defaults_and_refusals(capsys):
    import inference_swap_video as cli
    d = cli.build_parser().parse_args([])
    assert d.paste_mask is False and d.paste_dilate == 8 and d.paste_feather == 8
    o = cli.build_parser().parse_args(["--stream", "--paste_mask", "--paste_dilate", "3", "--paste_feather", "0"])
    assert o.paste_mask is True and o.paste_dilate == 3 and o.paste_feather == 0
    for argv in (["--paste_mask"], ["--paste_mask", "--align"], ["--paste_mask", "--parse_masks", "--paste_dilate", "2"]):
        msg = _exit_message(argv)
        assert "--paste_mask" in msg and "needs --paste_back or --stream" in msg, msg
    for flag in ("--paste_dilate", "--paste_feather"):
        for lead in (["--paste_back"], ["--stream"]):
            msg = _exit_message(lead + [flag, "4"])
            assert flag in msg and "--paste_mask" in msg, msg
            assert flag in _exit_message(lead + [flag + "=4"])
        for bad in ("65", "-1", "1000"):
            msg = _exit_message(["--stream", "--paste_mask", flag, bad])
            assert flag in msg and "0 .. 64" in msg and bad in msg, msg
    capsys.readouterr()


def test_paste_mask_argument_checks():
    from reface_amd.pasteback import PasteBack, PasteMask, paste_on_device
    m = PasteMask([2, 3, 5, 6, 7])
    assert (m.dilate, m.feather, m.passes) == (8, 8, 2)
    assert m.lut_host.dtype == np.uint8 and m.lut_host.shape == (256,) and np.flatnonzero(m.lut_host).tolist() == [2, 3, 5, 6, 7]
    from reface_amd.stream import keep_lut
    assert np.array_equal(m.lut_host, keep_lut([2, 3, 5, 6, 7]))
    assert PasteMask([], 0, 0, 1).lut_host.sum() == 0 and PasteMask([1], 64, 64, 3).passes == 3
    for kw in (dict(dilate=-1), dict(dilate=65), dict(feather=-1), dict(feather=65)):
        with pytest.raises(ValueError, match="0 .. 64"):
            PasteMask([1], **kw)
    for p in (0, 4):
        with pytest.raises(ValueError, match="passes is 1 .. 3"):
            PasteMask([1], passes=p)
    with pytest.raises(ValueError, match="labels are 0 .. 255"):
        PasteMask([256])
    with pytest.raises(ValueError, match="uint8 tensor"):
        m.alpha(torch.zeros(1, 8, 8), 16)
    with pytest.raises(ValueError, match="uint8 tensor"):
        m.alpha(torch.zeros(1, 8, 9, dtype=torch.uint8), 16)
    with pytest.raises(ValueError, match="never reduced"):
        m.alpha(torch.zeros(1, 8, 8, dtype=torch.uint8), 4)
    with pytest.raises(TypeError, match="PasteMask"):
        PasteBack("nowhere", np.zeros((1, 8)), mask=[2, 3])
    pb = PasteBack("nowhere", np.zeros((1, 8)), mask=m)
    try:
        with pytest.raises(ValueError, match="label maps"):
            pb._batch_labels([0], None, "cpu")
        assert PasteBack("nowhere", np.zeros((1, 8)))._batch_labels([0], None, "cpu") is None          # no mask: label maps are not read
    finally:
        pb.close()
    assert paste_on_device.__defaults__[-2:] == (None, None)


def test_ops_refuse_host_tensors():
    from reface_amd import _lib, ops
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.paste_alpha_u8(u8(1, 8, 8), u8(256), u8(1, 16, 16), u8(128))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.paste_back_alpha_u8(u8(1, 16, 16, 3), u8(1, 16, 16), torch.zeros(1, 8, dtype=torch.float64), u8(1, 9, 7, 3), u8(1, 9, 7, 4))


def test_exports():
    from reface_amd import _lib
    names = ("rf_paste_alpha_u8", "rf_paste_back_alpha_u8")
    for name in names:
        assert name in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 110 and all(hasattr(lib, n) for n in names)
    header = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert all(f"int {n}(" in header for n in names)
