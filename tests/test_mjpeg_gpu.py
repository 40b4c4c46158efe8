"""The GPU JPEG encoder (reface_amd/csrc/jpegenc.hip, reface_amd/mjpeg.py) against the numpy restatement (coefficients, exactly) and against
PIL's file (byte for byte), and ``inference_swap_video.py --write_video`` end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_refs as R  # noqa: E402

from reface_amd import mjpeg as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4)
_IDS = [f"{s[0]}x{s[1]}" for s in R.GPU_SIZES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("subsampling", M.SUBSAMPLINGS)
@pytest.mark.parametrize("size", R.GPU_SIZES, ids=_IDS)
def test_coefficients_equal_model(size, subsampling):
    """64 x 520: 198 / 195 blocks per MCU row, more than the entropy coder takes per pass; 24 x 2064: 774, more than a 1080p row has."""
    H, W = size
    batch = _dev(np.stack([R.image(kind, H, W) for kind in R.KINDS]))
    for quality in R.QUALITIES:
        got = M.coefficients(batch, quality, subsampling).cpu().numpy()
        for b, kind in enumerate(R.KINDS):
            want = R.model_coefficients(kind, H, W, quality, subsampling)
            assert got[b].shape == want.shape and got[b].dtype == np.int16
            bad = np.argwhere(got[b] != want)
            assert bad.size == 0, (quality, kind, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("subsampling", M.SUBSAMPLINGS)
@pytest.mark.parametrize("size", R.GPU_SIZES, ids=_IDS)
def test_files_equal_pil(size, subsampling):
    H, W = size
    batch = _dev(np.stack([R.image(kind, H, W) for kind in R.KINDS]))
    for quality in R.QUALITIES:
        files = M.JpegEncoder(DEV, quality, subsampling).encode(batch)
        assert len(files) == len(R.KINDS)
        for b, kind in enumerate(R.KINDS):
            want = R.pil_jpeg(R.image(kind, H, W), quality, subsampling)
            if files[b] != want:
                first = next((i for i, (x, y) in enumerate(zip(files[b], want)) if x != y), min(len(want), len(files[b])))
                raise AssertionError(f"Q {quality} {kind}: {len(files[b])} bytes against PIL's {len(want)}, first difference at byte {first}")


def test_hard_cases_hold_stuffing_and_zrl():
    """The inputs of test_files_equal_pil that are there for the FF 00 stuffing and the longest codes (noise, Q = 100) and for ZRL runs and
    EOB-only blocks (smooth, Q = 30) really contain them, by the model's count."""
    stuffed = zrl = eob = 0
    for H, W in R.GPU_SIZES[3:]:
        for subsampling in M.SUBSAMPLINGS:
            s = {}
            R.intervals(R.model_coefficients("noise", H, W, 100, subsampling), subsampling, s)
            stuffed += s.get("stuffed", 0)
            s = {}
            R.intervals(R.model_coefficients("smooth", H, W, 30, subsampling), subsampling, s)
            zrl, eob = zrl + s.get("zrl", 0), eob + s.get("eob_only", 0)
    assert stuffed > 100 and zrl > 10 and eob > 100, (stuffed, zrl, eob)


def test_rgba_and_strided_views():
    rng = np.random.RandomState(3)
    H, W = 50, 70
    rgba = np.stack([np.concatenate([R.image(kind, H, W), rng.randint(0, 256, (H, W, 1)).astype(np.uint8)], axis=2) for kind in R.KINDS[:3]])
    big = rng.randint(0, 256, (3, H + 9, W + 13, 3)).astype(np.uint8)
    enc = M.JpegEncoder(DEV, 75, "420")
    files = enc.encode(_dev(rgba))
    for b in range(3):
        assert files[b] == R.pil_jpeg(rgba[b], 75, "420"), b          # (PIL's convert("RGB") drops the alpha byte)
    view = _dev(big)[:, 4:4 + H, 6:6 + W]          # rows and images strided
    assert not view.is_contiguous()
    files = enc.encode(view)
    for b in range(3):
        assert files[b] == R.pil_jpeg(big[b, 4:4 + H, 6:6 + W], 75, "420"), b
    one = enc.encode(_dev(big)[1, 4:4 + H, 6:6 + W])          # [H, W, C]
    assert one == [files[1]]
    for bad in (torch.zeros((2, 8, 8, 1), dtype=torch.uint8, device=DEV), torch.zeros((2, 8, 8, 3), dtype=torch.float32, device=DEV),
                torch.zeros((8, 8), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            enc.encode(bad)


def test_two_encodes_in_flight_and_pool():
    a = np.stack([R.image("noise", 48, 80), R.image("smooth", 48, 80)])
    b = a[::-1].copy()
    enc = M.JpegEncoder(DEV, 90, "444")
    ja, jb = enc.encode_async(_dev(a)), enc.encode_async(_dev(b))
    assert ja.sc is not jb.sc and not enc._free.get(ja.sc.key)
    fb, fa = jb.result(), ja.result()
    assert fa == [R.pil_jpeg(x, 90, "444") for x in a] and fb == [R.pil_jpeg(x, 90, "444") for x in b]
    assert len(enc._free[ja.sc.key]) == 2          # both sets of scratch are back
    jc = enc.encode_async(_dev(a))
    assert jc.sc in (ja.sc, jb.sc)
    jc.discard()
    assert len(enc._free[ja.sc.key]) == 2
    assert enc.encode(_dev(a)) == fa          # on reused scratch


# ------------------------------------------------------------------------------------------------ the CLI
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = os.path.join(d, f)
    return out


def _check_cli_pair(plain, video, out_plain, out_video, avi_rel, quality, subsampling, n_frames, bases=("", "")):
    """`video` is the run with --write_video: its AVI holds PIL's encodes of results/, every other file equals the plain run's, and so does
    every printed line but the closing one."""
    ta, tb = _tree(out_plain), _tree(out_video)
    assert sorted(tb) == sorted(list(ta) + [avi_rel])
    for rel, path in ta.items():
        if rel.endswith(".npz"):          # (a zip archive carries its members' times)
            x, y = np.load(path), np.load(tb[rel])
            assert sorted(x.files) == sorted(y.files) and all(np.array_equal(x[k], y[k]) for k in x.files), rel
        else:
            assert open(path, "rb").read() == open(tb[rel], "rb").read(), rel
    names = sorted(os.listdir(os.path.join(out_video, "results")))
    assert len(names) == n_frames
    a = R.parse_avi(open(tb[avi_rel], "rb").read())
    assert a["total_frames"] == len(a["frames"]) == n_frames and (a["rate"], a["scale"]) == (25000, 1000)
    for k, name in enumerate(names):
        im = Image.open(os.path.join(out_video, "results", name))
        assert (a["width"], a["height"]) == im.size
        assert a["frames"][k] == R.pil_jpeg(np.asarray(im), quality, subsampling), name
    la, lb = (s.replace(str(o), "OUT").replace(str(base) or "BASE", "BASE").splitlines()
              for s, o, base in ((plain, out_plain, bases[0]), (video, out_video, bases[1])))
    assert len(la) == len(lb) and la[:-1] == lb[:-1]
    assert "mux of the reference's stage 3 is not built" in la[-1] and "not built" not in lb[-1]
    assert f"video of {n_frames} frames written to OUT/{avi_rel} ({n_frames} frames)" in lb[-1] and "no audio track" in lb[-1]


def test_cli_stream_write_video(tmp_path):
    import test_stream_gpu as S
    S._make_inputs(tmp_path, 4, rgba=(1,), seed=12)
    for name in ("plain", "video"):
        S._copy_inputs(tmp_path, tmp_path / name / "base")
    plain = S._run(tmp_path, tmp_path / "plain" / "base", tmp_path / "plain" / "out", "--stream")
    video = S._run(tmp_path, tmp_path / "video" / "base", tmp_path / "video" / "out", "--stream", "--write_video")
    _check_cli_pair(plain, video, tmp_path / "plain" / "out", tmp_path / "video" / "out", "clip_swapped.avi", 90, "420", 4,
                    bases=(tmp_path / "plain" / "base", tmp_path / "video" / "base"))
    assert open(tmp_path / "plain" / "base" / "clip_inv_transforms.npy", "rb").read() == open(tmp_path / "video" / "base" / "clip_inv_transforms.npy", "rb").read()


def _paste_back_runner(tmp_path):
    """The prepared tree of the staged caller's smallest run (two 320 x 200 frames, one batch) -> run(out, *flags) -> stdout."""
    from test_host_cpu import _prepared_swap_tree
    from reface_amd.pasteback import alignment_coefficients
    base = tmp_path / "base"
    _prepared_swap_tree(str(base), n_tar=2, n_src=1)
    os.rename(base / "target_cropped", base / "clipcropped_face")
    os.rename(base / "mask_frames", base / "clipmask_frames")
    rng = np.random.default_rng(5)
    (base / "clip").mkdir()
    coeffs = []
    for i in range(2):
        W, H = 320, 200
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(base / "clip" / f"{i}.png")
        coeffs.append(alignment_coefficients(np.array([[40.0, 30.0], [40.0, 170.0], [180.0, 170.0], [180.0, 30.0]]) + 20 * i, 1024))
    np.save(base / "clip_inv_transforms.npy", coeffs)

    def run(out, *extra):
        (out / "temp_results").mkdir(parents=True)
        shutil.copy(base / "source_cropped" / "0.png", out / "temp_results" / "me.png")
        shutil.copy(base / "source_mask" / "0.png", out / "temp_results" / "me.jpg")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(out), "--Base_dir", str(base),
                            "--target_video", "videos/clip.mp4", "--src_image", "faces/me.jpg", "--config",
                            os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none", "--n_samples", "2", "--ddim_steps", "4",
                            "--scale", "3.5", "--precision", "full", "--num_workers", "0", "--clip_vision_config", json.dumps(SMALL_CLIP),
                            "--paste_back", *extra], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        return r.stdout

    return run


def test_cli_paste_back_gpu_png_write_video(tmp_path):
    run = _paste_back_runner(tmp_path)
    plain = run(tmp_path / "plain", "--gpu_png")
    video = run(tmp_path / "video", "--gpu_png", "--write_video", str(tmp_path / "video" / "sub" / "v.avi"), "--video_quality", "75",
                "--video_subsampling", "444")
    _check_cli_pair(plain, video, tmp_path / "plain", tmp_path / "video", os.path.join("sub", "v.avi"), 75, "444", 2)


@pytest.mark.parametrize("flags", [(), ("--gpu_png_decode",)], ids=["host_paste", "device_frames"])
def test_cli_paste_back_other_branches_write_video(tmp_path, flags):
    """The two --paste_back branches without --gpu_png (frames pasted on the host and uploaded once more; frames decoded and pasted on the
    device, PNGs encoded on the host): frame k of the AVI is PIL's encode of results/<id_k>.png."""
    out = tmp_path / "out"
    stdout = _paste_back_runner(tmp_path)(out, *flags, "--write_video", "--video_fps", "29.97")
    names = sorted(os.listdir(out / "results"))
    a = R.parse_avi(open(out / "clip_swapped.avi", "rb").read())
    assert len(names) == 2 == a["total_frames"] == len(a["frames"]) and (a["rate"], a["scale"]) == (29970, 1000)
    for k, name in enumerate(names):
        assert a["frames"][k] == R.pil_jpeg(np.asarray(Image.open(out / "results" / name)), 90, "420"), name
    assert "video of 2 frames written to" in stdout.splitlines()[-1] and "29.97 fps" in stdout.splitlines()[-1]
