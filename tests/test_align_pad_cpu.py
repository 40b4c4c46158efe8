"""crop_image's enable_padding branch without a GPU (reface_amd/align.py: pad_plan, pad_image_host, pad_tables) against the reference's own
results (tests/golden/align_pad.npz, written by tools/gen_golden.py's `align_pad` group from crop_image(..., enable_padding=True)) and
against numpy / scipy / PIL, plus the front-ends' checks of --align_padding, which run before any model loads."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_align_cpu import _exit_message, _frames, _video_argv, np_resample, seeded_frame  # noqa: E402

PADDED = ("left_edge", "corner", "multi_reflect", "one_px", "shrunk")
CASES = PADDED + ("interior",)
# the issue's table: window (h, w), pads (left, top, right, bottom), blur to 3 decimals, padded (h, w)
EXPECT = {"left_edge": ((62, 41), (21, 19, 19, 19), 1.245, (100, 81)), "corner": ((32, 33), (16, 16, 21, 23), 1.047, (71, 70)),
          "multi_reflect": ((40, 122), (38, 41, 38, 41), 2.546, (122, 198)), "one_px": ((28, 1), (28, 9, 9, 9), 0.622, (46, 38)),
          "shrunk": ((34, 22), (12, 10, 10, 10), 0.660, (54, 44))}


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "align_pad.npz"))


def pad_case(G, name):
    """(frame uint8 [H, W, 3], quad, S) of a fixture case."""
    H, W, seed, S = (int(v) for v in G["frames"][list(G["names"]).index(name)])
    return seeded_frame(H, W, 3, seed), G[name + "_quad"], S


def case_window(G, name):
    """(window uint8 [H0, W0, 3] after any shrink, CropPlan, PadPlan | None, S): the LANCZOS shrink is tests/test_align_cpu.py's restatement."""
    from reface_amd.align import crop_plan, pad_plan
    frame, quad, S = pad_case(G, name)
    p = crop_plan(quad, (frame.shape[1], frame.shape[0]), S)
    img = np_resample(frame, p.rsize) if p.shrink > 1 else frame
    ox, oy, w, h = p.window
    return np.ascontiguousarray(img[oy:oy + h, ox:ox + w]), p, pad_plan(p, S), S


def test_fixture_holds_the_cases(G):
    assert tuple(G["names"]) == CASES
    for n in PADDED:
        assert G[n + "_padded"].shape == EXPECT[n][3] + (3,) and G[n + "_padded"].dtype == np.uint8
    assert G["interior_padded"].size == 0


@pytest.mark.parametrize("name", CASES)
def test_pad_plan_is_the_reference_decision(G, name):
    from reface_amd.align import quad_coefficients
    win, p, pp, S = case_window(G, name)
    if name == "interior":
        assert pp is None
        return
    (H0, W0), pad, blur, (h, w) = EXPECT[name]
    assert win.shape[:2] == (H0, W0) and pp.pad == pad and pp.size == (w, h) and round(pp.blur, 3) == blur
    assert pp.radius == int(4 * pp.blur + 0.5) and all(isinstance(v, int) for v in pp.pad)
    assert np.array_equal(pp.quad, p.quad + pad[:2]) and np.array_equal(pp.coeffs, quad_coefficients(pp.quad, S))
    assert (p.shrink == 6) == (name == "shrunk")


@pytest.mark.parametrize("name", PADDED)
def test_pad_image_host_is_the_reference_padding(G, name):
    """Zero differing bytes in the padded image, and in the crop PIL's QUAD transform makes of it."""
    from reface_amd.align import pad_image_host
    win, p, pp, S = case_window(G, name)
    got = pad_image_host(win, pp.pad, pp.blur)
    ref = G[name + "_padded"]
    assert got.dtype == np.uint8 and got.shape == ref.shape and np.array_equal(got, ref), int((got != ref).sum())
    crop = np.asarray(Image.fromarray(got).transform((S, S), Image.QUAD, (pp.quad + 0.5).flatten(), Image.BILINEAR))
    assert np.array_equal(crop, G[name + "_crop"]), int((crop != G[name + "_crop"]).sum())
    assert not (crop == 0).all(-1).any()          # no black wedge is left
    rgba = np.concatenate([win, np.full(win.shape[:2] + (1,), 7, np.uint8)], axis=2)          # alpha is not read
    assert np.array_equal(pad_image_host(rgba, pp.pad, pp.blur), got)


def test_interior_crop_is_the_unpadded_one(G):
    win, p, pp, S = case_window(G, "interior")
    crop = np.asarray(Image.fromarray(win).transform((S, S), Image.QUAD, (p.quad + 0.5).flatten(), Image.BILINEAR))
    assert pp is None and np.array_equal(crop, G["interior_crop"])


@pytest.mark.parametrize("sigma,shape", [(0.66, (31, 17, 3)), (2.7, (40, 33, 3)), (11.3, (23, 29, 3)), (40.0, (13, 7, 2))])
def test_host_blur_is_scipy_gaussian_filter(sigma, shape):
    """Bit equality on float32 input: a sigma below 1, one around 3, and radii (45, 160) beyond the image, where scipy's fold runs repeatedly."""
    from scipy.ndimage import gaussian_filter
    from reface_amd.align import gaussian_blur_host, gaussian_weights
    a = np.random.default_rng(int(sigma * 100)).uniform(0, 255, shape).astype(np.float32)
    got, ref = gaussian_blur_host(a, sigma), gaussian_filter(a, [sigma, sigma, 0])
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    w, r = gaussian_weights(sigma)
    assert r == int(4 * sigma + 0.5) and w.shape == (2 * r + 1,) and w.dtype == np.float64
    if sigma > 10:
        assert r > max(shape[:2])


def test_host_folds_and_median():
    from reface_amd.align import _fold_numpy, median_f32
    a = np.random.default_rng(1).integers(0, 255, (5, 1, 3)).astype(np.float32)
    ref = np.pad(a, ((12, 9), (7, 3), (0, 0)), "reflect")          # pads beyond n - 1, and an axis of length 1
    assert np.array_equal(ref, a[_fold_numpy(np.arange(26) - 12, 5)][:, _fold_numpy(np.arange(11) - 7, 1)])
    for n in (1, 2, 7, 10):
        v = np.random.default_rng(n).normal(size=n).astype(np.float32) * 100
        assert median_f32(v).dtype == np.float32 and median_f32(v) == np.median(v)


def test_pad_tables_layout():
    """The device tables: every offset inside its table, the index maps inside their images, and the per-axis clips whose maximum is the
    clip of the mask."""
    from reface_amd.align import PAD_DESC, pad_profiles, pad_tables
    items = [((3, 2, 37, 53), (40, 45, 50, 61), 20.0), ((0, 0, 1, 9), (4, 3, 2, 5), 0.1)]
    desc, itab, dtab, wmax, hmax, stats = pad_tables(items)
    assert desc.shape == (2, PAD_DESC) and desc.dtype == itab.dtype == np.int32 and dtab.dtype == np.float64
    assert (wmax, hmax) == (37 + 90, 53 + 106)
    for d, (win, pad, blur) in zip(desc, items):
        ox, oy, W0, H0, w, h, r = (int(v) for v in d[:7])
        assert (ox, oy, W0, H0) == win and w == W0 + pad[0] + pad[2] and h == H0 + pad[1] + pad[3] and r == int(4 * blur + 0.5)
        extrow, colmap, extcol = itab[d[7]:d[7] + h + 2 * r], itab[d[8]:d[8] + w], itab[d[9]:d[9] + w + 2 * r]
        assert extrow.min() >= 0 and extrow.max() < H0 and colmap.min() >= 0 and colmap.max() < W0 and extcol.min() >= 0 and extcol.max() < w
        assert np.array_equal(extcol[r:r + w], np.arange(w)) and d[10] + w <= itab.size and d[15] + h <= dtab.size
        mx, my = pad_profiles(W0, H0, pad)
        mask = np.maximum(mx[None], my[:, None])
        c1 = np.maximum(dtab[d[12]:d[12] + w][None], dtab[d[13]:d[13] + h][:, None])
        c2 = np.maximum(dtab[d[14]:d[14] + w][None], dtab[d[15]:d[15] + h][:, None])
        assert np.array_equal(c1, np.clip(mask * 3.0 + 1.0, 0.0, 1.0)) and np.array_equal(c2, np.clip(mask, 0.0, 1.0))
        assert abs(dtab[d[11]:d[11] + r].sum() * 2 + dtab[d[11] + r] - 1.0) < 1e-12
    assert 0.0 <= stats[0]["vblur_skipped"] <= stats[0]["hblur_skipped"] < 1.0
    with pytest.raises(ValueError, match=">= 1"):
        pad_tables([((0, 0, 4, 4), (0, 1, 1, 1), 1.0)])


def test_old_refusals_hold_and_new_keywords_exist():
    from reface_amd import _lib, ops
    from reface_amd.align import Aligner, crop_plan
    quad = np.array([[100.0, 100.0], [100.0, 200.0], [200.0, 200.0], [200.0, 100.0]])
    with pytest.raises(NotImplementedError, match="enable_padding"):
        crop_plan(quad, (640, 480), 128, enable_padding=True)
    with pytest.raises(NotImplementedError, match="enable_padding"):
        Aligner(128, enable_padding=True)
    al = Aligner(128, pad_edges=True, device="cpu")
    assert al.pad_edges is True and al.padded == [] and Aligner(128, device="cpu").pad_edges is False
    assert "rf_align_pad_u8" in _lib.EXPORTS
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)          # noqa: E731
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.align_pad_u8(z(1, 9, 7, 3), z(1, 16, dt=torch.int32), z(8, dt=torch.int32), z(8, dt=torch.float64), z(2 * 9 * 9 * 3, dt=torch.float32),
                         z(ops.PAD_SELECT_WORDS, dt=torch.int32), z(1, 9, 9, 3))


# ---- the front-ends: --align_padding is refused without the alignment it belongs to, before any model loads or the GPU is touched
def test_swap_video_align_padding_needs_align_or_stream(tmp_path, monkeypatch):
    import inference_swap_video as cli
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched before the inputs were checked"))
    assert cli.build_parser().parse_args([]).align_padding is False and cli.build_parser().parse_args(["--align_padding"]).align_padding is True
    base = tmp_path / "base"
    os.makedirs(base)
    _frames(base)
    argv = [a for a in _video_argv(tmp_path, base) if a != "--align"]
    msg = _exit_message(cli, argv + ["--align_padding"])
    assert "--align_padding" in msg and "--align or --stream" in msg
    # with --align or --stream the flag is accepted and the usual input checks answer (no landmarks here)
    for route in ("--align", "--stream"):
        msg = _exit_message(cli, argv + [route, "--align_padding", "--landmarks", str(tmp_path / "none.npy")])
        assert "does not exist" in msg and "--align_padding" not in msg


def test_swap_selected_align_padding_needs_align(tmp_path, monkeypatch):
    import inference_swap_selected as cli
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched before the inputs were checked"))
    assert cli.build_parser().parse_args([]).align_padding is False
    argv = ["--outdir", str(tmp_path / "out"), "--Base_dir", str(tmp_path / "base"), "--target_folder", str(tmp_path / "tar"), "--src_folder",
            str(tmp_path / "src"), "--config", str(tmp_path / "no_such_config.yaml"), "--ckpt", "none", "--align_padding"]
    msg = _exit_message(cli, argv)
    assert "--align_padding" in msg and "--align" in msg
    assert str(tmp_path / "tar") in _exit_message(cli, argv + ["--align"])          # accepted: the folder check answers


def test_the_flag_leaves_the_option_line_alone(capsys, tmp_path):
    """Without the flag the callers print the option line they printed before it existed."""
    import inference_swap_selected as sel
    import inference_swap_video as vid
    for cli, argv in ((vid, ["--paste_mask"]), (sel, ["--align", "--target_folder", str(tmp_path / "t"), "--src_folder", str(tmp_path / "s")])):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert "align_padding" not in capsys.readouterr().out
