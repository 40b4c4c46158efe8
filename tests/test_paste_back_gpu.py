"""Stage 3 of the video caller on the GPU (reface_amd/csrc/pasteback.hip): the crop enlargement and the perspective paste-back are byte
for byte the reference's PIL recipe (scripts/inference_swap_video.py:705-724), PIL itself being the oracle here."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from reface_amd import _lib, ops
from reface_amd.output import to_u8_hwc
from reface_amd.pasteback import alignment_coefficients

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4)


def _pil_paste(crop, c, frame, Co):
    """The reference's stage 3 on one frame (crop uint8 [S, S, 3], frame uint8 [H, W, 3 | 4])."""
    s = Image.fromarray(crop).convert("RGBA")
    s.putalpha(255)
    p = Image.fromarray(frame).convert("RGBA")
    p.alpha_composite(s.transform(p.size, Image.PERSPECTIVE, tuple(float(v) for v in c), Image.BILINEAR))
    a = np.asarray(p)
    return a if Co == 4 else a[..., :3]


def _quads(W, H):
    """Rotated, skewed and partly outside, entirely outside -- in frame coordinates."""
    cx, cy, r = W * 0.45, H * 0.5, min(W, H) * 0.3
    t = np.deg2rad(23.0)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    rot = np.array([[-r, -r], [-r, r], [r, r], [r, -r]]) @ R.T + [cx, cy]
    skew = np.array([[-0.2 * W, 0.1 * H], [0.05 * W, 0.9 * H], [0.5 * W, 1.15 * H], [0.35 * W, -0.05 * H]])
    away = np.array([[1.5 * W, 1.5 * H], [1.5 * W, 2.0 * H], [2.0 * W, 2.0 * H], [2.0 * W, 1.5 * H]])
    return [rot, skew, away]


@pytest.mark.parametrize("h,w,S,B", [(512, 512, 1024, 2), (96, 96, 1024, 1), (60, 100, 256, 3), (37, 37, 37, 1)])
def test_paste_crop_is_pil_bilinear_resize(h, w, S, B):
    g = torch.Generator().manual_seed(h * 7 + w)
    x = torch.rand((B, 3, h, w), generator=g)
    x[0, :, 0, :5] = torch.tensor([0.0, 1.0, 0.5, 1.0 / 255.0, 254.999 / 255.0])
    out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=DEV)
    ops.paste_crop_u8(x.to(DEV), out)()
    got = out.cpu().numpy()
    for b in range(B):
        ref = np.asarray(Image.fromarray(to_u8_hwc(x[b].numpy())).resize((S, S), Image.BILINEAR))
        assert np.array_equal(got[b], ref), (b, int((got[b] != ref).sum()))


def test_paste_crop_refuses_downscale():
    lib = _lib.load()
    x = torch.zeros((1, 3, 64, 64), device=DEV)
    out = torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device=DEV)
    assert lib.rf_paste_crop_u8(x.data_ptr(), 1, 64, 64, 32, out.data_ptr(), None) != 0
    assert b"only upscaling" in lib.rf_last_error()


@pytest.mark.parametrize("W,H,S", [(1920, 1080, 1024), (1279, 721, 1024), (97, 53, 64)])
@pytest.mark.parametrize("Cf,Co", [(3, 4), (3, 3), (4, 4), (4, 3)])
def test_paste_back_is_pil_perspective_composite(W, H, S, Cf, Co):
    rng = np.random.default_rng(W + 10 * Cf + Co)
    B = 3
    crops = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (B, H, W, Cf), dtype=np.uint8)
    coeffs = np.stack([alignment_coefficients(q, S) for q in _quads(W, H)])
    # frames strided: each one a slice of a taller buffer (frame stride > H * W * Cf)
    tall = torch.zeros((B, H + 3, W, Cf), dtype=torch.uint8, device=DEV)
    tall[:, :H] = torch.from_numpy(frames).to(DEV)
    out = torch.empty((B, H, W, Co), dtype=torch.uint8, device=DEV)
    dcrops, dco = torch.from_numpy(crops).to(DEV), torch.from_numpy(coeffs).to(DEV)
    ops.paste_back_u8(dcrops, dco, tall[:, :H], out)()
    got = out.cpu().numpy()
    for b in range(B):
        ref = _pil_paste(crops[b], coeffs[b], frames[b], Co)
        assert np.array_equal(got[b], ref), (b, int((got[b] != ref).any(-1).sum()))
    inside = (got[..., :3] != frames[..., :3]).any(-1)
    assert inside[0].mean() > 0.01 and inside[1].any() and not inside[2].any()          # the third quad lies wholly outside its frame
    # a batch of 3 gives every frame the bytes it gets alone
    for b in range(B):
        one = torch.empty((1, H, W, Co), dtype=torch.uint8, device=DEV)
        ops.paste_back_u8(dcrops[b:b + 1].contiguous(), dco[b:b + 1].contiguous(), tall[b:b + 1, :H], one)()
        assert np.array_equal(one.cpu().numpy()[0], got[b]), b
    if Cf == Co:                    # in place: out == frames (packed)
        fr = torch.from_numpy(frames).to(DEV)
        ops.paste_back_u8(dcrops, dco, fr, fr)()
        assert np.array_equal(fr.cpu().numpy(), got)


def test_paste_back_argument_checks():
    lib = _lib.load()
    crops = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    co = torch.zeros((1, 8), dtype=torch.float64, device=DEV)
    fr = torch.zeros((1, 9, 7, 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros((1, 9, 7, 4), dtype=torch.uint8, device=DEV)
    p = [t.data_ptr() for t in (crops, co, fr, out)]
    assert lib.rf_paste_back_u8(p[0], 1, 16, p[1], p[2], 9, 7, 4, 9 * 7 * 4, p[3], 4, None) == 0
    torch.cuda.synchronize()
    assert lib.rf_paste_back_u8(p[0], 1, 16, p[1], p[2], 9, 7, 5, 9 * 7 * 5, p[3], 4, None) != 0
    assert lib.rf_paste_back_u8(p[0], 1, 16, p[1], p[2], 9, 7, 4, 9 * 7 * 4, p[3], 2, None) != 0
    assert lib.rf_paste_back_u8(p[0], 1, 16, p[1], p[2], 9, 7, 4, 9 * 7 * 4 - 1, p[3], 4, None) != 0
    assert lib.rf_paste_back_u8(None, 1, 16, p[1], p[2], 9, 7, 4, 9 * 7 * 4, p[3], 4, None) != 0
    assert lib.rf_paste_back_u8(p[0], 1, 16, p[1], p[2], 9, 7, 4, 9 * 7 * 4, p[2], 3, None) != 0        # in place across channel counts
    assert b"in place" in lib.rf_last_error()
    # non-finite source coordinates (NaN, +-inf) keep the frame
    inf = float("inf")
    fr.random_(0, 256)
    for c in ([float("nan")] * 8, [inf, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, -inf, 0, 0], [inf, 0, -inf, 0, 1, 0, 0, 0]):
        ops.paste_back_u8(crops, torch.tensor([c], dtype=torch.float64, device=DEV), fr, out)()
        assert torch.equal(out, fr), c


def test_cli_swap_video_paste_back(tmp_path):
    """--paste_back on the tree stage 1 leaves (test_cli_swap_video's, plus the full frames and their inverse transforms): results/ holds
    exactly the swapped frames (drop_last) as RGBA PNGs, each PIL's paste of model_outputs/<id>.png onto its frame; model_outputs/ is what a
    run without the flag writes."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_cpu import _prepared_swap_tree
    base = tmp_path / "base"
    _prepared_swap_tree(str(base), n_tar=3, n_src=1)
    os.rename(base / "target_cropped", base / "clipcropped_face")
    os.rename(base / "mask_frames", base / "clipmask_frames")
    rng = np.random.default_rng(5)
    (base / "clip").mkdir()
    frames, coeffs = [], []
    for i, (W, H) in enumerate([(320, 200), (320, 200), (320, 200)]):
        f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(f).save(base / "clip" / f"{i}.png")
        frames.append(f)
        coeffs.append(alignment_coefficients(_quads(W, H)[i % 2], 1024))
    np.save(base / "clip_inv_transforms.npy", coeffs)          # the reference's np.save of its list of per-frame arrays: [N, 8] fp64

    def run(out, *extra):
        (out / "temp_results").mkdir(parents=True)
        shutil.copy(base / "source_cropped" / "0.png", out / "temp_results" / "me.png")
        shutil.copy(base / "source_mask" / "0.png", out / "temp_results" / "me.jpg")
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(out), "--Base_dir", str(base), "--target_video",
               "videos/clip.mp4", "--src_image", "faces/me.jpg", "--config", os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none",
               "--n_samples", "2", "--ddim_steps", "4", "--scale", "3.5", "--precision", "full", "--num_workers", "0", "--clip_vision_config",
               json.dumps(SMALL_CLIP), *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        return r.stdout

    out, plain = tmp_path / "out", tmp_path / "plain"
    log = run(out, "--paste_back")
    assert "2 pasted frames" in log
    run(plain)
    ids = [f"{i:012d}" for i in range(2)]                       # 3 frames, batches of 2, drop_last
    assert sorted(os.listdir(out / "results")) == [s + ".png" for s in ids]
    assert os.listdir(plain / "results") == []
    assert sorted(os.listdir(out / "model_outputs")) == sorted(os.listdir(plain / "model_outputs")) == [s + ".png" for s in ids]
    for i, sid in enumerate(ids):
        mo = np.asarray(Image.open(out / "model_outputs" / (sid + ".png")))
        assert np.array_equal(mo, np.asarray(Image.open(plain / "model_outputs" / (sid + ".png"))))
        im = Image.open(out / "results" / (sid + ".png"))
        assert im.mode == "RGBA" and im.size == (320, 200)
        ref = _pil_paste(mo, coeffs[i], frames[i], 4)
        got = np.asarray(im)
        assert np.array_equal(got, ref), (sid, int((got != ref).any(-1).sum()))
        assert (got[..., :3] != frames[i]).any(-1).mean() > 0.05
