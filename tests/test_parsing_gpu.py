"""Face parser (BiSeNet) on the GPU: the new kernels of reface_amd/csrc/parsing.hip on ragged shapes against PyTorch run here, and the whole
parser against outputs of the reference's own BiSeNet (tests/golden/bisenet.npz, tools/gen_golden.py::gen_bisenet)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from reface_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_u8(shape, seed):
    """The fixtures' input images (tools/gen_golden.py::seeded_u8)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randint(0, 256, tuple(shape), generator=g, dtype=torch.uint8)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "bisenet.npz"))


@pytest.fixture(scope="module")
def parser():
    from reface_amd.parsing import FaceParser
    return FaceParser("none")


def test_parse_prep_matches_reference(golden):
    x = seeded_u8((1, 96, 128, 3), int(golden["small_seed"])).to(DEV)
    out = torch.full((1, 48, 64, 8), float("nan"), device=DEV)
    ops.parse_prep(x, out)()
    got = out.cpu()
    assert (got[..., 3:] == 0).all()
    err = (got[..., :3].permute(0, 3, 1, 2) - torch.from_numpy(golden["prep_small"])).abs().max().item()
    assert err <= 1e-5, err


def test_maxpool3x3s2_odd_sizes():
    torch.manual_seed(0)
    for B, H, W, C in ((2, 7, 9, 5), (1, 13, 4, 64), (3, 1, 6, 3)):
        x = torch.randn(B, H, W, C, device=DEV)
        out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, device=DEV)
        ops.maxpool3x3s2(x, out)()
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(out, ref), (B, H, W, C)


def test_add_relu():
    torch.manual_seed(1)
    a, r = torch.randn(3, 5, 7, 13, device=DEV), torch.randn(3, 5, 7, 13, device=DEV)
    out = torch.empty_like(a)
    ops.add_relu(a, r, out)()
    assert torch.equal(out, torch.relu(a + r))


def test_scale_add_vec():
    torch.manual_seed(2)
    x = torch.randn(3, 5, 7, 13, device=DEV)
    s, v = torch.rand(3, 13, device=DEV), torch.randn(3, 13, device=DEV)
    out = torch.empty_like(x)
    ops.scale_add_vec(x, s, v, out)()
    assert torch.equal(out, x * s[:, None, None, :] + v[:, None, None, :])


def test_parse_head_ragged_with_ties():
    from reface_amd.parsing import identity_lut, seg12_lut
    torch.manual_seed(3)
    B, h, w, C, H, W = 2, 5, 7, 19, 11, 17
    lg = torch.randn(B, h, w, C)
    lg[:, 1:4, 2:6, 3] += 4.0
    lg[..., 7] = lg[..., 3]                          # channel 7 duplicates channel 3: every tie between them must go to 3 (first maximum)
    ref_up = F.interpolate(lg.permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=True)
    ref = ref_up.argmax(1)
    top = torch.cat([ref_up[:, :7], ref_up[:, 8:]], 1).topk(2, dim=1).values       # margin without the duplicate
    sure = (top[:, 0] - top[:, 1]) > 1e-5
    assert (ref == 3).sum() > 10 and (ref != 7).all()
    for lut in (identity_lut(), seg12_lut()):
        out = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
        ops.parse_head(lg.to(DEV), torch.from_numpy(lut).to(DEV), out)()
        got = out.cpu()
        exp = torch.from_numpy(lut)[ref]
        assert torch.equal(got[sure], exp[sure])
        assert float((got == exp).float().mean()) > 0.99
    # a pitched logits view (the channel run shorter than the pixel pitch)
    wide = torch.zeros(B, h, w, 24)
    wide[..., :C] = lg
    out = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    ops.parse_head(wide.to(DEV)[..., :C], torch.from_numpy(identity_lut()).to(DEV), out)()
    assert torch.equal(out.cpu()[sure], ref[sure].to(torch.uint8))


def _check_labels(got, gold_labels, margin_ok):
    agree = (got == gold_labels)
    assert agree[margin_ok].all(), int((~agree[margin_ok]).sum())
    assert agree.mean() >= 0.999, agree.mean()


def test_parser_vs_reference_golden(golden, parser):
    x = seeded_u8((2, 1024, 1024, 3), int(golden["big_seed"]))
    eng = parser._engine(2, 1024, 1024)
    raw = eng.run(x.to(DEV), seg12=False).cpu().numpy()
    logits = eng.logits.permute(0, 3, 1, 2).cpu()
    gl = torch.from_numpy(golden["logits"])
    amax = gl.abs().max().item()
    err = (logits - gl).abs().max().item()
    assert err <= 1e-4 * amax, (err, amax)
    up = F.interpolate(gl, (512, 512), mode="bilinear", align_corners=True).topk(2, dim=1).values
    margin_ok = ((up[:, 0] - up[:, 1]) > 1e-3 * amax).numpy()
    _check_labels(raw, golden["labels"], margin_ok)
    seg12 = parser.parse(x.numpy(), seg12=True).cpu().numpy()
    _check_labels(seg12, golden["labels_seg12"], margin_ok)
    # the drop-in demo module: PIL in, uint8 numpy [512, 512] out, as the reference's faceParsing_demo
    from PIL import Image
    sys.path.insert(0, ROOT)
    from pretrained.face_parsing.face_parsing_demo import faceParsing_demo
    m = faceParsing_demo(parser, Image.fromarray(x[1].numpy()), convert_to_seg12=False)
    assert m.dtype == np.uint8 and m.shape == (512, 512) and np.array_equal(m, raw[1])
    lab = parser(Image.fromarray(x[0].numpy()))
    assert lab.dtype == torch.long and lab.is_cuda and np.array_equal(lab.cpu().numpy(), raw[0])


def test_batch_of_three_equals_single_images(parser):
    x = seeded_u8((3, 1024, 1024, 3), 2024)
    together = parser.parse(x, seg12=False).cpu()
    for i in range(3):
        assert torch.equal(parser.parse(x[i:i + 1], seg12=False).cpu()[0], together[i]), i
    small = parser.__class__("none", max_batch=2)                 # chunked into device batches of 2 + 1
    assert torch.equal(small.parse(x, seg12=True).cpu(), parser.parse(x, seg12=True).cpu())


def test_swap_selected_parse_masks(tmp_path):
    """--parse_masks: a crop tree without label-map folders is parsed on the GPU (seeded weights), then the swap runs as usual."""
    import json
    from PIL import Image
    base, out = tmp_path / "base", tmp_path / "out"
    rng = np.random.default_rng(5)
    for d, n in (("target_cropped", 3), ("source_cropped", 1)):
        os.makedirs(base / d)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(base / d / f"{i}.png")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_selected.py"), "--outdir", str(out), "--Base_dir", str(base), "--config",
           os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none", "--n_samples", "2", "--ddim_steps", "2", "--scale", "3.5",
           "--H", "512", "--W", "512", "--precision", "full", "--num_workers", "0",
           "--clip_vision_config", json.dumps(dict(hidden=128, intermediate=512, layers=2, heads=4))]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode != 0 and "stage 1" in (r.stderr + r.stdout)                 # without the flag: unchanged
    r = subprocess.run(cmd + ["--parse_masks", "--faceParsing_ckpt", "none"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    for d, n in (("mask_frames", 3), ("source_mask", 1)):
        assert sorted(os.listdir(base / d)) == [f"{i}.png" for i in range(n)]
        for i in range(n):
            m = np.asarray(Image.open(base / d / f"{i}.png"))
            assert m.shape == (512, 512) and m.dtype == np.uint8 and m.max() <= 11          # --seg12 is on in this caller
    from reface_amd.parsing import FaceParser
    crop = np.asarray(Image.open(base / "target_cropped" / "1.png").convert("RGB").resize((1024, 1024), Image.BILINEAR))
    assert np.array_equal(np.asarray(Image.open(base / "mask_frames" / "1.png")), FaceParser("none").parse(crop, seg12=True)[0].cpu().numpy())
    assert sorted(os.listdir(out / "results" / "0")) == [f"{i:012d}.png" for i in range(3)]
