"""Stage 3 of the video caller (paste-back) without a GPU: the inverse-transform fit, the CLI flag and its up-front input check, and the
ops' refusal of host tensors."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _apply(c, pts):
    x, y = pts[:, 0], pts[:, 1]
    d = c[6] * x + c[7] * y + 1
    return np.stack([(c[0] * x + c[1] * y + c[2]) / d, (c[3] * x + c[4] * y + c[5]) / d], axis=1)


QUADS = [
    np.array([[812.3, 240.7], [798.1, 905.2], [1450.6, 920.4], [1466.9, 251.0]]),        # near-axis-aligned face in a 1080p frame
    np.array([[120.0, 40.0], [40.0, 300.0], [310.0, 380.0], [390.0, 120.0]]),             # rotated by ~17 degrees
    np.array([[-50.5, 10.25], [20.0, 90.0], [70.75, 60.0], [60.0, -20.0]]),              # skewed, partly outside a small frame
]


@pytest.mark.parametrize("quad", QUADS)
def test_alignment_coefficients_map_quad_onto_crop(quad):
    from reface_amd.pasteback import alignment_coefficients
    S = 1024
    c = alignment_coefficients(quad, S)
    assert c.shape == (8,) and c.dtype == np.float64
    corners = np.array([[0, 0], [0, S], [S, S], [S, 0]], dtype=np.float64)
    assert np.abs(_apply(c, quad + 0.5) - corners).max() < 1e-9
    # the same 8 x 8 system, solved by least squares
    A, b = [], []
    for (x, y), (u, v) in zip(quad + 0.5, corners):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    ref = np.linalg.lstsq(np.array(A), np.array(b), rcond=None)[0]
    # (the system is badly conditioned in coefficient space: compare where the two fits send the frame's points, in crop pixels)
    grid = np.stack(np.meshgrid(np.linspace(quad[:, 0].min(), quad[:, 0].max(), 41), np.linspace(quad[:, 1].min(), quad[:, 1].max(), 41)), -1)
    grid = grid.reshape(-1, 2)
    assert np.abs(_apply(c, grid) - _apply(ref, grid)).max() < 1e-6
    assert np.abs(_apply(c, quad + 0.5) - corners).max() <= np.abs(_apply(ref, quad + 0.5) - corners).max() + 1e-12
    assert np.abs(_apply(alignment_coefficients(quad, 256), quad + 0.5) - corners / 4).max() < 1e-9


def test_load_inv_transforms_accepts_the_pickled_list(tmp_path):
    from reface_amd.pasteback import alignment_coefficients, load_inv_transforms
    cs = [alignment_coefficients(q) for q in QUADS]
    p = str(tmp_path / "v_inv_transforms.npy")
    obj = np.empty(len(cs), dtype=object)
    for i, c in enumerate(cs):
        obj[i] = c
    np.save(p, obj, allow_pickle=True)
    got = load_inv_transforms(p)
    assert got.dtype == np.float64 and got.shape == (3, 8) and np.array_equal(got, np.stack(cs))
    np.save(p, np.stack(cs))
    assert np.array_equal(load_inv_transforms(p), np.stack(cs))
    np.save(p, np.zeros((3, 7)))
    with pytest.raises(ValueError, match="8-coefficient"):
        load_inv_transforms(p)


def test_swap_video_takes_paste_back():
    import inference_swap_video as cli
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings}
    assert "--paste_back" in flags
    assert cli.build_parser().parse_args([]).paste_back is False
    assert cli.build_parser().parse_args(["--paste_back"]).paste_back is True
    opt = cli.build_parser().parse_args(["--Base_dir", "B", "--target_video", "x/clip7.mp4"])
    assert cli.pasteback_paths(opt) == {"video_frames": os.path.join("B", "clip7"), "inv_transforms": os.path.join("B", "clip7_inv_transforms.npy")}
    assert set(cli.prepared_paths(opt)) == {"frames", "masks", "src", "src_mask"}


def _tree(tmp_path, n=3):
    from test_host_cpu import _prepared_swap_tree
    base = tmp_path / "base"
    _prepared_swap_tree(str(base), n_tar=n, n_src=1)
    os.rename(base / "target_cropped", base / "clipcropped_face")
    os.rename(base / "mask_frames", base / "clipmask_frames")
    return base


def test_paste_back_inputs_checked_before_any_model_loads(tmp_path):
    """Without stage 1's frames / .npy, --paste_back exits non-zero naming them -- before the model (here: a config that does not exist) is
    touched and before the GPU is."""
    import inference_swap_video as cli
    base = _tree(tmp_path)
    argv = ["--outdir", str(tmp_path / "out"), "--Base_dir", str(base), "--target_video", "videos/clip.mp4", "--src_image", "faces/me.jpg",
            "--config", str(tmp_path / "no_such_config.yaml"), "--n_samples", "2", "--paste_back"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    msg = str(e.value.code)
    assert e.value.code not in (0, None)
    assert os.path.join(str(base), "clip") in msg and os.path.join(str(base), "clip_inv_transforms.npy") in msg
    # frames directory present, one frame of a swapped crop and the .npy rows missing: named too (frames 0, 1 are swapped; 2 is dropped)
    os.makedirs(base / "clip")
    from PIL import Image
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(base / "clip" / "0.png")
    np.save(base / "clip_inv_transforms.npy", np.zeros((1, 8)))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    msg = str(e.value.code)
    assert os.path.join(str(base), "clip", "1.png") in msg and "clip_inv_transforms.npy (rows for frames 0..1)" in msg
    assert os.path.join(str(base), "clip", "2.png") not in msg and os.path.join(str(base), "clip", "0.png") not in msg


def test_paste_ops_refuse_host_tensors():
    from reface_amd import _lib, ops
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.paste_crop_u8(torch.zeros(1, 3, 8, 8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.paste_back_u8(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.float64), torch.zeros(1, 9, 7, 3, dtype=torch.uint8),
                          torch.zeros(1, 9, 7, 4, dtype=torch.uint8))
