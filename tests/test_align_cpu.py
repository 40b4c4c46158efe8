"""Face alignment (reface_amd/align.py) without a GPU: the FFHQ quad, crop_image's bookkeeping and PIL's LANCZOS tap tables against the
reference's own results (tests/golden/align.npz, written by tools/gen_golden.py's `align` group from src/utils/alignmengt.py) and against
PIL, plus the front-ends' argument and file checks, which run before any model loads."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (128, 256)
CASES = ("inside", "over_edges", "rgba", "shrink")


def seeded_frame(h, w, c, seed, block=4):
    """tools/gen_golden.py's frame of the same name: seeded noise in block x block tiles, alpha 255 as a fourth channel."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    a = torch.randint(0, 256, ((h + block - 1) // block, (w + block - 1) // block, 3), generator=g, dtype=torch.uint8).numpy()
    a = np.repeat(np.repeat(a, block, axis=0), block, axis=1)[:h, :w]
    return np.concatenate([a, np.full((h, w, 1), 255, np.uint8)], axis=2) if c == 4 else a


def golden_case(G, name):
    W, H, C, seed = (int(v) for v in G["frames"][list(G["names"]).index(name)])
    return seeded_frame(H, W, C, seed)


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "align.npz"))


# ---- numpy restatements of the two kernels (include/reface_hip.h: rf_resample_u8, rf_align_quad_u8), fp64 / int32 like the device code
def np_resample(img, size):
    from reface_amd.align import resample_taps
    w, h = size

    def one_axis(a, n_out):          # along axis 1
        bounds, taps = resample_taps(a.shape[1], n_out)
        out = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
        for i, ((lo, n), k) in enumerate(zip(bounds, taps)):
            acc = (1 << 21) + np.tensordot(a[:, lo:lo + n].astype(np.int64), k[:n].astype(np.int64), axes=([1], [0]))
            out[:, i] = np.clip(acc >> 22, 0, 255)
        return out
    return one_axis(one_axis(img, w).transpose(1, 0, 2), h).transpose(1, 0, 2)


def np_align_quad(img, coeffs, window, S):
    ox, oy, w, h = window
    src = img[oy:oy + h, ox:ox + w, :3].astype(np.float64)
    a = [np.float64(v) for v in coeffs]
    yin, xin = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5, indexing="ij")
    xs = a[0] + a[1] * xin + a[2] * yin + a[3] * xin * yin
    ys = a[4] + a[5] * xin + a[6] * yin + a[7] * xin * yin
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    u, v = np.where(inside, xs, 0.5) - 0.5, np.where(inside, ys, 0.5) - 0.5
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    dx, dy = (u - x0)[..., None], (v - y0)[..., None]
    cx0, cx1, cy0 = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1)
    row2 = ((y0 + 1 >= 0) & (y0 + 1 < h))[..., None]
    cy1 = np.clip(y0 + 1, 0, h - 1)
    v1 = src[cy0, cx0] + (src[cy0, cx1] - src[cy0, cx0]) * dx
    v2 = np.where(row2, src[cy1, cx0] + (src[cy1, cx1] - src[cy1, cx0]) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    return np.where(inside[..., None], out, 0).astype(np.uint8)


def np_crop(frame, quad, S):
    """crop_image through crop_plan and the two restatements."""
    from reface_amd.align import crop_plan
    p = crop_plan(quad, (frame.shape[1], frame.shape[0]), S)
    img = np_resample(frame, p.rsize) if p.shrink > 1 else frame
    return np_align_quad(img, p.coeffs, p.window, S), p


@pytest.mark.parametrize("name", CASES)
def test_quad_from_landmarks_is_compute_transform(G, name):
    """The same fp64 operations in the same order as the reference's compute_transform: equal, not close."""
    from reface_amd.align import quad_from_landmarks, smooth_quads
    c, x, y, quad = quad_from_landmarks(G[name + "_landmarks"])
    for got, key in ((c, "_c"), (x, "_x"), (y, "_y"), (quad, "_quad")):
        assert got.dtype == np.float64 and np.array_equal(got, G[name + key]), key
    c2, x2, y2, _ = quad_from_landmarks(G[name + "_landmarks"], scale=1.5)
    assert np.array_equal(c2, c) and np.array_equal(x2, x * 1.5)
    # crop_faces with both sigmas 0 (every caller of the reference) leaves the per-frame values alone
    cs, xs, ys, quads = smooth_quads(np.stack([c, c]), np.stack([x, x]), np.stack([y, y]))
    assert np.array_equal(quads, np.stack([quad, quad])) and np.array_equal(cs[0], c)
    with pytest.raises(ValueError, match="68 landmarks"):
        quad_from_landmarks(np.zeros((67, 2)))


def test_smooth_quads_is_gaussian_filter1d_over_frames():
    from scipy.ndimage import gaussian_filter1d
    from reface_amd.align import smooth_quads
    rng = np.random.default_rng(3)
    cs, xs, ys = rng.normal(size=(3, 12, 2))
    c2, x2, y2, q = smooth_quads(cs, xs, ys, center_sigma=1.5, xy_sigma=0.8)
    assert np.array_equal(c2, gaussian_filter1d(cs, sigma=1.5, axis=0)) and np.array_equal(x2, gaussian_filter1d(xs, sigma=0.8, axis=0))
    assert np.array_equal(q, np.stack([c2 - x2 - y2, c2 - x2 + y2, c2 + x2 + y2, c2 + x2 - y2], axis=1))
    c3, x3, _, _ = smooth_quads(cs, xs, ys, center_sigma=2.0)
    assert np.array_equal(x3, xs) and not np.array_equal(c3, cs)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_crop_plan_reproduces_the_reference_crop(G, name, S):
    """crop_plan's shrink, window and QUAD coefficients, and resample_taps, are right when the kernels' arithmetic restated in numpy gives
    the reference's crop_image bytes: zero differing bytes."""
    frame = golden_case(G, name)
    got, p = np_crop(frame, G[name + "_quad"], S)
    ref = G[f"{name}_crop{S}"]
    assert got.shape == ref.shape == (S, S, 3)
    assert np.array_equal(got, ref), int((got != ref).sum())
    H, W = frame.shape[:2]
    if name == "shrink":
        assert p.shrink == {128: 6, 256: 3}[S] and p.rsize == (int(np.rint(W / p.shrink)), int(np.rint(H / p.shrink)))
    else:
        assert p.shrink <= 1 and p.rsize is None
    ox, oy, w, h = p.window
    assert 0 <= ox and 0 <= oy and ox + w <= (p.rsize or (W, H))[0] and oy + h <= (p.rsize or (W, H))[1]
    if name == "over_edges":
        assert (ox, oy) == (0, 0) and (ref == 0).all(-1).mean() > 0.1          # part of the crop lies outside the frame
    if name == "inside":
        assert ox > 0 and oy > 0 and not (ref == 0).all(-1).any()


def test_crop_plan_arguments():
    from reface_amd.align import Aligner, crop_plan
    quad = np.array([[100.0, 100.0], [100.0, 200.0], [200.0, 200.0], [200.0, 100.0]])
    before = quad.copy()
    p = crop_plan(quad, (640, 480), 128)
    assert np.array_equal(quad, before)                     # the caller's quad is not modified (the reference passes quad.copy())
    assert np.array_equal(p.quad, quad - p.window[:2])
    with pytest.raises(NotImplementedError, match="enable_padding"):
        crop_plan(quad, (640, 480), 128, enable_padding=True)
    with pytest.raises(NotImplementedError, match="enable_padding"):
        Aligner(128, enable_padding=True)
    with pytest.raises(ValueError, match="not finite"):
        crop_plan(quad * np.nan, (640, 480), 128)
    with pytest.raises(ValueError, match="outside"):
        crop_plan(quad + 5000.0, (640, 480), 128)


@pytest.mark.parametrize("src,dst", [((1000, 777), (333, 259)), ((640, 480), (320, 240)), ((901, 603), (129, 86)), ((97, 53), (97, 20)),
                                     ((61, 47), (150, 99))])
def test_resample_taps_give_pil_lanczos(src, dst):
    """The host's tap tables (PIL's precompute_coeffs / normalize_coeffs_8bpc) in the two integer passes give Image.resize(LANCZOS)'s bytes."""
    from reface_amd.align import resample_taps
    rng = np.random.default_rng(src[0] + dst[0])
    for C in (3, 4):
        img = rng.integers(0, 256, (src[1], src[0], C), dtype=np.uint8)
        if C == 4:
            img[..., 3] = 255
        ref = np.asarray(Image.fromarray(img).resize(dst, Image.LANCZOS))
        got = np_resample(img, dst)
        assert np.array_equal(got, ref), int((got != ref).sum())
    bounds, taps = resample_taps(src[0], dst[0])
    assert bounds.dtype == taps.dtype == np.int32 and bounds.shape == (dst[0], 2) and taps.shape[0] == dst[0]
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= src[0]).all() and (bounds[:, 1] <= taps.shape[1]).all()
    assert np.abs(taps.sum(1) - (1 << 22)).max() <= taps.shape[1]          # normalised: each row sums to 1 up to the per-tap rounding


def _apply(c, pts):
    x, y = pts[:, 0], pts[:, 1]
    d = c[6] * x + c[7] * y + 1
    return np.stack([(c[0] * x + c[1] * y + c[2]) / d, (c[3] * x + c[4] * y + c[5]) / d], axis=1)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_inverse_transforms_map_the_quad_onto_the_crop(G, name, S):
    """As tests/test_paste_back_cpu.py checks alignment_coefficients: ours and the reference's (normal equations) are compared where they
    send the quad's corners, not coefficient by coefficient."""
    from reface_amd.align import Aligner
    quad = G[name + "_quad"]
    ours = Aligner(S, device="cpu").inverse_transforms(quad[None])
    assert ours.shape == (1, 8) and ours.dtype == np.float64
    corners = np.array([[0, 0], [0, S], [S, S], [S, 0]], dtype=np.float64)
    assert np.abs(_apply(ours[0], quad + 0.5) - corners).max() < 1e-9
    assert np.abs(_apply(G[f"{name}_inv{S}"], quad + 0.5) - corners).max() < 1e-9


def test_fill_missing_and_landmark_files(tmp_path):
    from reface_amd.align import fill_missing, landmarks_for, load_landmarks
    lm = np.zeros((5, 68, 2))
    lm[1, 3, 0] = np.nan
    lm[2] = np.inf
    lm[4, 67, 1] = np.nan
    assert fill_missing(lm) == [0, 0, 0, 3, 3]
    with pytest.raises(ValueError, match="first image has no face"):
        fill_missing(lm[1:])
    p = str(tmp_path / "lm.npy")
    np.save(p, lm)
    assert load_landmarks(p, 5).shape == (5, 68, 2)
    with pytest.raises(ValueError, match="5 landmark rows for 4 images"):
        load_landmarks(p, 4)
    np.save(p, np.zeros((68, 2), np.float32))
    assert load_landmarks(p, 1).shape == (1, 68, 2) and load_landmarks(p).dtype == np.float64
    np.save(p, np.zeros((5, 68, 3)))
    with pytest.raises(ValueError, match=r"\[N, 68, 2\]"):
        load_landmarks(p)
    with pytest.raises(ValueError, match="does not exist"):
        landmarks_for(["a.png"], str(tmp_path / "none.npy"), "the frames")


def test_align_ops_refuse_host_tensors():
    from reface_amd import _lib, ops
    assert {"rf_align_quad_u8", "rf_resample_u8"} <= set(_lib.EXPORTS)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.align_quad_u8(torch.zeros(1, 9, 7, 3, dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.float64), torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    t = (torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int32))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.resample_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), t, t, torch.zeros(1, 8, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


# ---- the front-ends: flags, and the input checks that run before any model (here: a config that does not exist) or the GPU is touched
def _video_argv(tmp_path, base, *extra):
    return ["--outdir", str(tmp_path / "out"), "--Base_dir", str(base), "--target_video", "videos/clip.mp4", "--src_image", str(base / "me.jpg"),
            "--config", str(tmp_path / "no_such_config.yaml"), "--ckpt", "none", "--n_samples", "2", "--align", *extra]


def _frames(base, n=3):
    os.makedirs(base / "clip")
    for i in range(n):
        Image.fromarray(np.full((40, 60, 3), 10 * i, np.uint8)).save(base / "clip" / f"{i}.png")
    Image.fromarray(np.zeros((50, 50, 3), np.uint8)).save(base / "me.jpg")


def _exit_message(cli, argv):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code not in (0, None)
    return str(e.value.code)


def test_swap_video_takes_align():
    import inference_swap_video as cli
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings}
    assert {"--align", "--landmarks", "--src_landmarks"} <= flags
    d = cli.build_parser().parse_args([])
    assert d.align is False and d.landmarks is None and d.src_landmarks is None
    assert cli.build_parser().parse_args(["--align"]).align is True


def test_swap_video_align_inputs_checked_before_any_model_loads(tmp_path, monkeypatch):
    import inference_swap_video as cli
    from reface_amd import align as A
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched before the inputs were checked"))
    base = tmp_path / "base"
    os.makedirs(base)
    # no frames, no source image
    msg = _exit_message(cli, _video_argv(tmp_path, base))
    assert os.path.join(str(base), "clip") in msg and "me.jpg" in msg
    _frames(base)
    lm, src = str(tmp_path / "lm.npy"), str(tmp_path / "src.npy")
    good = np.ones((3, 68, 2))
    np.save(lm, good)
    np.save(src, good[0])
    # no landmarks file and (in this environment) no dlib: a clear message, whichever of the two dlib lacks
    if A.dlib_available() is not None:
        msg = _exit_message(cli, _video_argv(tmp_path, base))
        assert "give a landmarks .npy file, or install dlib" in msg and "--landmarks" in msg and "--src_landmarks" in msg
        msg = _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", lm))
        assert "--src_landmarks" in msg and "the frames" not in msg
    # a landmarks file that does not exist
    assert "does not exist" in _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", str(tmp_path / "x.npy"), "--src_landmarks", src))
    # wrong shapes: rows != frames, not [N, 68, 2]
    np.save(lm, good[:2])
    assert "2 landmark rows for 3 images" in _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    np.save(lm, np.ones((3, 5, 2)))
    assert "[N, 68, 2]" in _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    # a non-finite first row: no earlier crop to repeat
    bad = good.copy()
    bad[0, 0, 0] = np.nan
    np.save(lm, bad)
    assert "first image has no face" in _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    # the same for the source image
    np.save(lm, good)
    np.save(src, bad[0])
    assert "first image has no face" in _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    # a hole in the frame numbering
    np.save(src, good[0])
    os.rename(base / "clip" / "1.png", base / "clip" / "7.png")
    assert os.path.join(str(base), "clip", "1.png") in _exit_message(cli, _video_argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    assert not os.path.exists(base / "clipcropped_face") and not os.path.exists(base / "clip_inv_transforms.npy")


def test_swap_selected_align_inputs_checked_before_any_model_loads(tmp_path, monkeypatch):
    import inference_swap_selected as cli
    from reface_amd import align as A
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched before the inputs were checked"))
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings}
    assert {"--align", "--landmarks", "--src_landmarks"} <= flags and cli.build_parser().parse_args([]).align is False
    tar, src = tmp_path / "tar", tmp_path / "src"
    argv = ["--outdir", str(tmp_path / "out"), "--Base_dir", str(tmp_path / "base"), "--target_folder", str(tar), "--src_folder", str(src),
            "--config", str(tmp_path / "no_such_config.yaml"), "--ckpt", "none", "--align"]
    msg = _exit_message(cli, argv)
    assert str(tar) in msg and str(src) in msg
    for d, n in ((tar, 2), (src, 1)):
        os.makedirs(d)
        for i in range(n):
            Image.fromarray(np.zeros((30, 30, 3), np.uint8)).save(d / f"{i}.png")
    if A.dlib_available() is not None:
        assert "give a landmarks .npy file, or install dlib" in _exit_message(cli, argv)
    lm, slm = str(tmp_path / "lm.npy"), str(tmp_path / "slm.npy")
    np.save(lm, np.ones((3, 68, 2)))
    np.save(slm, np.full((1, 68, 2), np.nan))
    msg = _exit_message(cli, argv + ["--landmarks", lm, "--src_landmarks", slm])
    assert "3 landmark rows for 2 images" in msg and "no image has a face" in msg
    assert not os.path.exists(tmp_path / "base" / "target_cropped")
