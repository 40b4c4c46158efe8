"""The streamed video route, host side (reface_amd/stream.py, rf_video_prep_u8): PIL's BICUBIC tap tables, a numpy restatement of the prep
kernel against the host dataset, the C-ABI entry and its op, and the --stream input checks that run before any model loads."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

TEST_ARGS = dict(gray_outer_mask=True, remove_mask_tar_FFHQ=[1, 2, 3, 5, 6, 7, 9], preserve_mask_src_FFHQ=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])


def np_resample(img, size, filt):
    """PIL's two integer passes with reface_amd.align.resample_taps (tests/test_align_cpu.py::np_resample, with the filter)."""
    from reface_amd.align import resample_taps
    w, h = size

    def one_axis(a, n_out):          # along axis 1
        bounds, taps = resample_taps(a.shape[1], n_out, filt)
        out = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
        for i, ((lo, n), k) in enumerate(zip(bounds, taps)):
            acc = (1 << 21) + np.tensordot(a[:, lo:lo + n].astype(np.int64), k[:n].astype(np.int64), axes=([1], [0]))
            out[:, i] = np.clip(acc >> 22, 0, 255)
        return out
    return one_axis(one_axis(img, w).transpose(1, 0, 2), h).transpose(1, 0, 2)


def np_video_prep(crop, labels, keep, size):
    """rf_video_prep_u8 in numpy: taps -> u8 image -> x / 255 -> (x - 0.5) / 0.5 -> keep-mask from the LUT -> product, all in fp32."""
    from reface_amd.stream import keep_lut
    u8 = np_resample(crop, size, "bicubic")
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    target = (x - np.float32(0.5)) / np.float32(0.5)
    mask = (np.float32(1.0) - (keep_lut(keep)[labels] != 0).astype(np.float32))[None]
    return torch.from_numpy(target), torch.from_numpy(mask), torch.from_numpy(target * mask)


def edge_crop(rng, H, W):
    """Noise whose first / last two rows and columns are a 0 / 255 checkerboard: the clipped edge windows and the bicubic overshoot."""
    c = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    edge = (yy < 2) | (yy >= H - 2) | (xx < 2) | (xx >= W - 2)
    c[edge] = board[edge]
    return c


@pytest.mark.parametrize("src,dst", [((1024, 1024), (512, 512)), ((130, 94), (65, 47)), ((333, 200), (100, 77)), ((97, 53), (97, 20))])
def test_bicubic_taps_give_pil_default_resize(src, dst):
    rng = np.random.default_rng(src[0] + dst[1])
    x = edge_crop(rng, src[1], src[0])
    got = np_resample(x, dst, "bicubic")
    assert np.array_equal(got, np.asarray(Image.fromarray(x).resize(dst)))
    assert np.array_equal(got, np.asarray(Image.fromarray(x).resize(dst, Image.BICUBIC)))


def test_bicubic_two_to_one_taps_and_lanczos_default():
    from reface_amd.align import resample_taps
    bounds, taps = resample_taps(1024, 512, "bicubic")
    inner = [-49152, -147456, 475136, 1818624, 1818624, 475136, -147456, -49152]
    for i in range(2, 510):
        assert tuple(bounds[i]) == (2 * i - 3, 8) and list(taps[i, :8]) == inner, i
    assert bounds[0, 0] == 0 and bounds[0, 1] < 8 and bounds[511, 0] + bounds[511, 1] == 1024
    assert all(int(taps[i, :bounds[i, 1]].sum()) in range((1 << 22) - 8, (1 << 22) + 9) for i in (0, 1, 510, 511))
    # the default is still LANCZOS: the cached call returns the very arrays, and they are not the bicubic ones
    b0, t0 = resample_taps(1024, 512)
    b1, t1 = resample_taps(1024, 512, "lanczos")
    assert np.array_equal(b0, b1) and np.array_equal(t0, t1) and resample_taps(1024, 512)[1] is t0
    assert t0.shape[1] == 13 and t0.shape != taps.shape
    x = np.random.default_rng(3).integers(0, 256, (64, 48, 3), dtype=np.uint8)
    assert np.array_equal(np_resample(x, (24, 32), "lanczos"), np.asarray(Image.fromarray(x).resize((24, 32), Image.LANCZOS)))
    with pytest.raises(ValueError, match="filter"):
        resample_taps(8, 4, "nearest")


@pytest.mark.parametrize("gray", [True, False])
def test_numpy_prep_is_the_host_dataset(tmp_path, gray):
    from reface_amd.data import VideoDataset
    rng = np.random.default_rng(5 + gray)
    os.makedirs(tmp_path / "crops")
    os.makedirs(tmp_path / "masks")
    crop = edge_crop(rng, 1024, 1024)
    labels = rng.integers(0, 19, (512, 512), dtype=np.uint8)
    labels[:16] = np.arange(256, dtype=np.uint8).repeat(32).reshape(16, 512)          # every LUT entry
    Image.fromarray(crop).save(tmp_path / "crops" / "0.png")
    Image.fromarray(labels).save(tmp_path / "masks" / "0.png")
    args = dict(TEST_ARGS, gray_outer_mask=gray)
    image, prior, kw, sid = VideoDataset(data_path=str(tmp_path / "crops"), mask_path=str(tmp_path / "masks"), **args)[0]
    keep = args["remove_mask_tar_FFHQ"] if gray else [2, 3, 5, 6, 7]
    target, mask, inpaint = np_video_prep(crop, labels, keep, (512, 512))
    assert sid == "000000000000"
    assert torch.equal(image, target) and torch.equal(kw["inpaint_mask"], mask) and torch.equal(kw["inpaint_image"], inpaint)
    assert 0.2 < float(mask.mean()) < 0.8


def test_video_prep_op_is_exported_and_refuses_host_tensors():
    from reface_amd import _lib, ops
    from reface_amd.align import resample_taps
    assert "rf_video_prep_u8" in _lib.EXPORTS
    t = tuple(torch.from_numpy(a) for a in resample_taps(8, 4, "bicubic"))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.video_prep_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(256, dtype=torch.uint8), t, t,
                          torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 3, 4, 4))


def test_video_stream_host_half():
    """Quads and inverse transforms of every frame come from the landmarks alone; a frame without a face repeats the last one's."""
    from reface_amd.align import quad_from_landmarks
    from reface_amd.pasteback import alignment_coefficients
    from reface_amd.stream import VideoStream, keep_lut
    rng = np.random.default_rng(1)
    lm = rng.uniform(20, 200, (5, 68, 2))
    lm[2] = np.nan
    lm[3, 7, 1] = np.inf
    vs = VideoStream(lm, [1, 2, 17])
    assert vs.src_of == [0, 1, 1, 1, 4] and vs.inv_transforms.shape == (5, 8) and vs.inv_transforms.dtype == np.float64
    for i, s in enumerate(vs.src_of):
        assert np.array_equal(vs.inv_transforms[i], alignment_coefficients(quad_from_landmarks(lm[s])[3], 1024)), i
    assert keep_lut([1, 2, 17]).sum() == 3 and keep_lut([1, 2, 17])[17] == 1
    lm[0] = np.nan
    with pytest.raises(ValueError, match="first image has no face"):
        VideoStream(lm, [1])


# ---- --stream: its input checks run before any model (here: a config that does not exist) or the GPU is touched
def _argv(tmp_path, base, *extra):
    return ["--outdir", str(tmp_path / "out"), "--Base_dir", str(base), "--target_video", "videos/clip.mp4", "--src_image", str(base / "me.jpg"),
            "--config", str(tmp_path / "no_such_config.yaml"), "--ckpt", "none", "--n_samples", "2", "--stream", *extra]


def _exit_message(cli, argv):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code not in (0, None)
    return str(e.value.code)


def test_swap_video_takes_stream():
    import inference_swap_video as cli
    d = cli.build_parser().parse_args([])
    assert d.stream is False and d.stream_keep is False
    o = cli.build_parser().parse_args(["--stream", "--stream_keep"])
    assert o.stream is True and o.stream_keep is True


def test_stream_inputs_checked_before_any_model_loads(tmp_path, monkeypatch):
    import inference_swap_video as cli
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched before the inputs were checked"))
    base = tmp_path / "base"
    os.makedirs(base)
    # no frames directory, no source image
    msg = _exit_message(cli, _argv(tmp_path, base))
    assert "--stream needs" in msg and os.path.join(str(base), "clip") in msg and "me.jpg" in msg
    os.makedirs(base / "clip")
    for i in range(3):
        Image.fromarray(np.full((40, 60, 3), 10 * i, np.uint8)).save(base / "clip" / f"{i}.png")
    Image.fromarray(np.zeros((50, 50, 3), np.uint8)).save(base / "me.jpg")
    lm, src = str(tmp_path / "lm.npy"), str(tmp_path / "src.npy")
    good = np.ones((3, 68, 2))
    np.save(src, good[0])
    # a landmark file with the wrong row count
    np.save(lm, good[:2])
    assert "2 landmark rows for 3 images" in _exit_message(cli, _argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    # a first frame without a face: no earlier crop to repeat
    bad = good.copy()
    bad[0, 0, 0] = np.nan
    np.save(lm, bad)
    assert "first image has no face" in _exit_message(cli, _argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    # a hole in the frame numbering
    np.save(lm, good)
    os.rename(base / "clip" / "1.png", base / "clip" / "7.png")
    assert os.path.join(str(base), "clip", "1.png") in _exit_message(cli, _argv(tmp_path, base, "--landmarks", lm, "--src_landmarks", src))
    assert not os.path.exists(base / "clip_inv_transforms.npy") and not os.path.exists(tmp_path / "out")
