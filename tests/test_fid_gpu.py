"""The FID on the GPU (reface_amd/csrc/fid.hip, reface_amd/fidscore.py, eval_tool/fid/fid_score.py) against the reference's own outputs
(tests/golden/fid.npz) and the host restatements that tests/test_fid_cpu.py pins to them.

The yardstick of the tower's gates is the reference itself: e_ref_feat = max |f32 - f64| of the fixture is what ONE fp32 evaluation order of
the layers is away from float64; the GPU's order is another draw of the same rounding noise and gets 4 x e_ref (the rule of
tests/test_expr_gpu.py).  fid_tol is the fixture's measure of what 4 x e_ref on every feature can move the FID by, doubled.  Every test prints
its figure before it asserts (DESIGN.md section 8 keeps the record)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fid_inputs as I  # noqa: E402

from reface_amd import _lib  # noqa: E402
from reface_amd import fidscore as FS  # noqa: E402
from reface_amd import ops  # noqa: E402
from reface_amd.params import CLIPVisionConfig  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fid.npz"))


@pytest.fixture(scope="module")
def data():
    return I.build()


@pytest.fixture(scope="module")
def scorer():
    return FS.FidScorer(FS.seeded_fid_state(), batch=20, device=DEV)          # 48 images = 2 full batches + a tail of 8


@pytest.fixture(scope="module")
def scorer_bf16():
    return FS.FidScorer(FS.seeded_fid_state(), precision="bf16", batch=48, device=DEV)


@pytest.fixture(scope="module")
def folders(tmp_path_factory, data):
    return I.write_folders(str(tmp_path_factory.mktemp("fid_folders")), data)


def _edge_image(rng, H, W):
    """Noise whose first / last two rows and columns are a 0 / 255 checkerboard: the clipped edge windows and the bicubic overshoot."""
    c = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    edge = (yy < 2) | (yy >= H - 2) | (xx < 2) | (xx >= W - 2)
    c[edge] = board[edge]
    return c


def _taps(H, W):
    nh, nw = FS.resized_size(H, W)
    return [tuple(torch.from_numpy(t).to(DEV) for t in FS.crop_taps(n, r)) for n, r in ((W, nw), (H, nh))]


def _bare_scorer(dt=torch.float32):
    sc = FS.FidScorer.__new__(FS.FidScorer)
    sc.dev, sc.dt, sc._taps = torch.device(DEV, torch.cuda.current_device()), dt, {}
    return sc


@pytest.mark.parametrize("hw", [(512, 512), (224, 224), (1024, 1024), (300, 260), (260, 300), (57, 40), (224, 225), (224, 227), (1, 1)])
def test_fid_prep_is_the_preprocess_bit_for_bit(hw):
    """rf_fid_prep_u8 into a NaN-filled fp32 buffer against prep_host (PIL's resize and crop, then one fp32 division, subtraction and
    division per value on both sides): no tolerance, pad channel exactly 0.  The sizes cover the identity table, 21 taps, a crop along
    either axis, an upscale and both roundings of a half-integer crop offset."""
    H, W = hw
    rng = np.random.default_rng(1900 + H + W)
    imgs = np.stack([_edge_image(rng, H, W) for _ in range(2)])
    tx, ty = _taps(H, W)
    out = torch.full((2, 224, 224, 4), float("nan"), dtype=torch.float32, device=DEV)
    ops.fid_prep_u8(torch.from_numpy(imgs).to(DEV), tx, ty, out)()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = sum(int((got[b, :, :, :3].transpose(2, 0, 1).view(np.uint32) != FS.prep_host(imgs[b]).view(np.uint32)).sum()) for b in range(2))
    pad_ok = np.array_equal(got[..., 3].view(np.uint32), np.zeros((2, 224, 224), np.uint32))
    print(f"fid prep {hw}: taps {tx[1].shape[1]} x {ty[1].shape[1]}; {bad} of {2 * 224 * 224 * 3} values differ from prep_host in any bit; pad exactly 0: {pad_ok}")
    assert pad_ok and bad == 0


def test_fid_prep_bf16_operand():
    """The bf16 engine's operand: the fp32 values rounded to nearest even, 8 channels per pixel, pads exactly 0."""
    rng = np.random.default_rng(31)
    imgs = np.stack([_edge_image(rng, 300, 260) for _ in range(2)])
    tx, ty = _taps(300, 260)
    out = torch.full((2, 224, 224, 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.fid_prep_u8(torch.from_numpy(imgs).to(DEV), tx, ty, out)()
    got = out.cpu()
    want = torch.stack([torch.from_numpy(FS.prep_host(im)).permute(1, 2, 0).to(torch.bfloat16) for im in imgs])
    assert torch.equal(got[..., :3].view(torch.int16), want.view(torch.int16)) and torch.equal(got[..., 3:].view(torch.int16), torch.zeros((2, 224, 224, 5), dtype=torch.int16))


def test_fid_prep_strided_batch_and_scorer_grouping(data):
    """A batch that is a strided view (every second image of a stack) and the scorer's grouping of mixed sizes equal prep_host."""
    rng = np.random.default_rng(77)
    stack = torch.from_numpy(np.stack([_edge_image(rng, 40, 24) for _ in range(4)])).to(DEV)
    view = stack[::2]
    tx, ty = _taps(40, 24)
    out = torch.empty((2, 224, 224, 4), dtype=torch.float32, device=DEV)
    ops.fid_prep_u8(view, tx, ty, out)()
    for b in range(2):
        assert np.array_equal(out[b, :, :, :3].cpu().numpy().transpose(2, 0, 1), FS.prep_host(stack[2 * b].cpu().numpy()))
    sc = _bare_scorer()
    got2 = sc.prep_u8(view).cpu().numpy()          # the scorer passes a strided device view on as it is
    assert np.array_equal(got2, out.cpu().numpy())
    imgs = [I.rgb(data["dataset"][k]) for k in (3, 4, 5, 6, 7, 9, 10, 14)]          # 224, 300 x 260, 260 x 300 (L), 224, 224, 57 x 40 (RGBA), 224 x 225, 224 x 227
    got = sc.prep_u8([torch.from_numpy(im) for im in imgs]).cpu().numpy()
    assert {im.shape[:2] for im in imgs} == {(224, 224), (300, 260), (260, 300), (57, 40), (224, 225), (224, 227)}
    for b, im in enumerate(imgs):
        assert np.array_equal(got[b, :, :, :3].transpose(2, 0, 1), FS.prep_host(im)), im.shape
    assert not got[..., 3].any()


def _stats(x):
    N, D = x.shape
    mu = torch.full((D,), float("nan"), dtype=torch.float64, device=DEV)
    sigma = torch.full((D, D), float("nan"), dtype=torch.float64, device=DEV)
    ops.fid_stats(torch.from_numpy(x).to(DEV), mu, sigma)()
    torch.cuda.synchronize()
    return mu.cpu().numpy(), sigma.cpu().numpy()


@pytest.mark.parametrize("case", [(2, 16, 0.0, 1.0), (7, 32, 0.0, 1.0), (301, 512, 0.0, 1.0), (301, 512, 100.0, 0.01)])
def test_fid_stats_vs_numpy(case):
    """rf_fid_stats against np.mean / np.cov of the same fp32 features in float64.  Gates: |d mu| <= 4 (N + 3) 2^-53 max|x| and
    |d sigma_jk| <= 4 (N + 3) 2^-53 max_j sigma_jj: each side's N-term sum of products carries at most (N + 3) 2^-53 sum|terms| <=
    (N + 3) 2^-53 (N - 1) sqrt(sigma_jj sigma_kk); two sides, and a factor 2 for the mean's own rounding.  The last case (mean 100, std 0.01)
    is the one an uncentred sum x x^T - N mu mu^T fails by ten orders of magnitude.  NaN-filled outputs, sigma == sigma^T in every bit, two
    runs identical."""
    N, D, mean, std = case
    g = torch.Generator().manual_seed(N * 1000 + D + int(mean))
    x = (mean + std * torch.randn((N, D), generator=g) + 0.1 * std * torch.randn((1, D), generator=g)).to(torch.float32).numpy()
    mu, sigma = _stats(x)
    mu2, sigma2 = _stats(x)
    hm, hs = FS.stats_host(x)
    u = 4 * (N + 3) * 2.0 ** -53
    gm, gs = u * float(np.abs(x).max()), u * float(np.diag(hs).max())
    dm, ds = float(np.abs(mu - hm).max()), float(np.abs(sigma - hs).max())
    print(f"fid stats N={N} D={D} mean {mean} std {std}: max|d mu| = {dm:.3e} (gate {gm:.3e}), max|d sigma| = {ds:.3e} (gate {gs:.3e}), max sigma_jj {np.diag(hs).max():.3e}")
    assert np.isfinite(mu).all() and np.isfinite(sigma).all()
    assert dm <= gm and ds <= gs
    assert np.array_equal(sigma.view(np.uint64), sigma.T.copy().view(np.uint64))
    assert np.array_equal(mu.view(np.uint64), mu2.view(np.uint64)) and np.array_equal(sigma.view(np.uint64), sigma2.view(np.uint64))


def test_fid_stats_refuses_other_shapes():
    for N, D in ((1, 16), (5, 24)):
        with pytest.raises(_lib.RefaceHipError):
            ops.fid_stats(torch.zeros((N, D), device=DEV), torch.zeros((D,), dtype=torch.float64, device=DEV),
                          torch.zeros((D, D), dtype=torch.float64, device=DEV))()


def _features(sc, data):
    return {key: sc.features_u8([torch.from_numpy(I.rgb(im)) for im in data[key]]).cpu().numpy() for key in ("dataset", "results")}


def test_tower_features_vs_reference(scorer, golden, data):
    """prep + the fixture tower on the 96 images (mixed sizes; batch 20: full batches and a tail of 8) against the reference module in
    float64: every feature within 4 x e_ref_feat."""
    e_ref = float(golden["e_ref_feat"])
    worst = 0.0
    for key, f in _features(scorer, data).items():
        assert f.shape == (48, 32) and np.isfinite(f).all()
        d = float(np.abs(f - golden[f"feat_f64_{key}"]).max())
        worst = max(worst, d)
        print(f"fid features {key}: max|GPU - reference fp64| = {d:.3e}, max|GPU - reference fp32| = {float(np.abs(f - golden[f'feat_f32_{key}']).max()):.3e}")
    print(f"fid features: e_ref_feat = {e_ref:.3e}, gate 4 x e_ref = {4 * e_ref:.3e}, GPU max = {worst:.3e}")
    assert worst <= 4 * e_ref


def test_tower_is_batch_invariant(scorer, data):
    """No GEMM of the engine splits K: image 0 alone and image 0 among five give the same bits."""
    imgs = [torch.from_numpy(I.rgb(im)) for im in data["dataset"][:5]]
    e5 = scorer.engine(5)
    scorer.prep_u8(imgs, out=e5.x)
    f5 = e5.run().cpu().numpy()
    e1 = scorer.engine(1)
    for k in (0, 4):
        scorer.prep_u8(imgs[k:k + 1], out=e1.x)
        f1 = e1.run().cpu().numpy()
        assert np.array_equal(f1[0].view(np.uint32), f5[k].view(np.uint32)), (k, np.abs(f1[0] - f5[k]).max())


def test_vit_b32_sized_tower_vs_reference(golden, data):
    """The launch list at ViT-B/32's own dimensions (hidden 768, 12 layers, 12 heads, projection 512), seeded, on 4 images: within 4 x the
    e_ref the reference module has at these dimensions."""
    sc = FS.FidScorer(FS.seeded_fid_state(CLIPVisionConfig(**FS.VIT_B32)), batch=4, device=DEV)
    assert (sc.cfg.hidden, sc.cfg.layers, sc.cfg.heads, sc.cfg.proj, sc.cfg.tokens) == (768, 12, 12, 512, 50)
    f = sc.features_u8([torch.from_numpy(I.rgb(data["dataset"][i])) for i in golden["b32_index"]]).cpu().numpy()
    e_ref = float(golden["b32_e_ref"])
    d = float(np.abs(f - golden["b32_feat_f64"]).max())
    print(f"fid ViT-B/32-sized tower: max|GPU - reference fp64| = {d:.3e} (e_ref {e_ref:.3e}, gate {4 * e_ref:.3e}); {len(sc.engine(4).launches)} launches")
    assert f.shape == (4, 512) and np.isfinite(f).all() and d <= 4 * e_ref


def test_bf16_tower_vs_reference(scorer_bf16, golden, data):
    """precision="bf16": every feature within 4 x e_ref_feat_bf16 (the reference module cast to bfloat16 on the CPU, against float64)."""
    e_ref = float(golden["e_ref_feat_bf16"])
    worst = max(float(np.abs(f - golden[f"feat_f64_{key}"]).max()) for key, f in _features(scorer_bf16, data).items())
    print(f"fid bf16 features: max|GPU - reference fp64| = {worst:.3e} (e_ref_feat_bf16 {e_ref:.3e}, gate {4 * e_ref:.3e})")
    assert worst <= 4 * e_ref


def test_score_folders_end_to_end(scorer, scorer_bf16, folders, golden, capsys):
    """PNG folders (one L and one all-255 RGBA image each) -> the FID, per precision within that precision's fid_tol of the reference's; no
    image is prepared on the host; the folder of 48 under a batch of 50 prints the reference's warning."""
    for tag, sc in (("f32", scorer), ("bf16", scorer_bf16)):
        r = sc.score_folders(folders, num_workers=0)
        tol = float(golden[f"fid_tol_{tag}"])
        d = abs(r["fid"] - float(golden["fid"]))
        print(f"fid score_folders {tag}: FID {r['fid']:.9f}, reference {float(golden['fid']):.9f}, |d| = {d:.3e} (fid_tol {tol:.3e}); {r['images_per_s']:.1f} images/s")
        assert r["images"] == 96 and r["host_prepared"] == 0 and d <= tol
    capsys.readouterr()
    big = FS.FidScorer(scorer.sd, batch=50, device=DEV)
    rb = big.score_folders(folders)
    assert capsys.readouterr().out.count(FS.BATCH_WARNING) == 2 and rb["fid"] == scorer.score_folders(folders)["fid"]


def test_p_mode_image_is_prepared_on_the_host(scorer, folders, golden, data, tmp_path):
    """A third folder, the results with one image stored in mode P: it is prepared by prep_host and uploaded, reported, and the folder scores."""
    from PIL import Image
    third = I.write_folders(str(tmp_path), {**data, "dataset": data["dataset"][:2], "dataset_names": data["dataset_names"][:2]})[1]
    Image.fromarray(data["results"][1]).convert("P").save(os.path.join(third, data["result_names"][1]))
    r = scorer.score_folders([folders[0], third])
    print(f"fid with one P-mode image: FID {r['fid']:.9f} (all-RGB results: {float(golden['fid']):.9f}), host-prepared {r['host_prepared']}")
    assert r["host_prepared"] == 1 and r["images"] == 96 and np.isfinite(r["fid"]) and r["fid"] > 0
    assert abs(r["fid"] - float(golden["fid"])) < 0.5          # one palettised image of 48 moves it, a little


def test_cli_and_npz_round_trip(scorer, folders, golden, tmp_path):
    """The CLI in a fresh process: the printed line parses to --json's value, within fid_tol of the reference's, nothing prepared on the host;
    its --save-stats file as a first path gives the folder's FID to 1e-12 relative."""
    out_json, stats = str(tmp_path / "fid.json"), str(tmp_path / "dataset.npz")
    cmd = [sys.executable, os.path.join(ROOT, "eval_tool", "fid", "fid_score.py"), "--device", "cuda"] + folders + [
        "--clip_ckpt", "none", "--batch-size", "20", "--num-workers", "2", "--json", out_json, "--save-stats", stats]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("FID: ")]
    r = json.load(open(out_json))
    assert line == ["FID:  {}".format(r["fid"])] and float(line[0].split()[1]) == r["fid"]          # print('FID: ', v): two spaces
    d, tol = abs(r["fid"] - float(golden["fid"])), float(golden["fid_tol_f32"])
    print(f"fid CLI: FID {r['fid']:.9f}, |FID - reference| = {d:.3e} (fid_tol {tol:.3e}); host-prepared {r['host_prepared']}; {r['images_per_s']:.1f} images/s")
    assert d <= tol and r["host_prepared"] == 0 and r["images"] == 96 and r["images_per_s"] > 0
    assert r["fid"] == r["mean_term"] + r["trace1"] + r["trace2"] - 2 * r["trace_covmean"]
    r2 = scorer.score_folders([stats, folders[1]])
    print(f"fid .npz first path: {r2['fid']!r} against {r['fid']!r} from the folder")
    assert abs(r2["fid"] - r["fid"]) <= 1e-12 * r["fid"] and r2["images1"] == 0
