"""The streamed video route on the GPU: rf_video_prep_u8 is the host dataset's item bit for bit (and the four-launch chain it replaces), the
device-frames paste is PasteBack.paste, and ``inference_swap_video.py --stream`` feeds the sampler the tensors of the staged route
(``--align --parse_masks --paste_back``) and writes its bytes, without the intermediate files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from reface_amd import _lib, ops
from reface_amd.align import resample_taps
from reface_amd.data import VideoDataset, _normalize, _to_tensor
from reface_amd.pasteback import PasteBack, alignment_coefficients, paste_on_device
from reface_amd.stream import keep_lut

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4)
KEEP = [1, 2, 3, 5, 6, 7, 9]
TEST_ARGS = dict(gray_outer_mask=True, remove_mask_tar_FFHQ=KEEP, preserve_mask_src_FFHQ=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])


def _edge_crop(rng, H, W):
    """Noise whose first / last two rows and columns are a 0 / 255 checkerboard: the clipped edge windows and the bicubic overshoot."""
    c = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    board = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    edge = (yy < 2) | (yy >= H - 2) | (xx < 2) | (xx >= W - 2)
    c[edge] = board[edge]
    return c


def _labels(rng, h, w):
    lab = rng.integers(0, 19, (h, w), dtype=np.uint8)
    flat = lab.reshape(-1)
    n = min(flat.size, 256)
    flat[:n] = np.arange(n, dtype=np.uint8)          # every LUT entry (where the map is large enough)
    return lab


def _host_item(crop, labels, keep, size):
    """VideoDataset.__getitem__'s arithmetic on arrays, for any output size (the dataset itself is fixed to 512 x 512)."""
    image = _normalize(_to_tensor(Image.fromarray(crop).resize(size)), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    mask_img = Image.fromarray(np.where(np.isin(labels, keep), 255, 0).astype(np.uint8)).convert("L")
    mask = 1.0 - _to_tensor(mask_img)
    return image, mask, image * mask


def _dev_taps(n_in, n_out, filt="bicubic"):
    return tuple(torch.from_numpy(a).to(DEV) for a in resample_taps(n_in, n_out, filt))


def _prep(crops, labels, keep, size):
    w, h = size
    B, Hc, Wc, _ = crops.shape
    dc, dl = torch.from_numpy(crops).to(DEV), torch.from_numpy(labels).to(DEV)
    lut = torch.from_numpy(keep_lut(keep)).to(DEV)
    out = [torch.full((B, c, h, w), 7.0, dtype=torch.float32, device=DEV) for c in (3, 1, 3)]
    ops.video_prep_u8(dc, dl, lut, _dev_taps(Wc, w), _dev_taps(Hc, h), *out)()
    return out, (dc, dl, lut)


@pytest.mark.parametrize("src,dst", [((1024, 1024), (512, 512)), ((130, 94), (65, 47)), ((333, 200), (100, 77)), ((97, 53), (97, 20)), ((2000, 40), (9, 33)),
                                     ((7000, 20), (5, 10))])
def test_video_prep_is_the_host_dataset(src, dst, tmp_path):
    """All three outputs bit for bit the host dataset's, batched and alone, and the four-launch chain's.  The sizes: the dataset's 2:1, a
    ragged 2:1, a non-integer ratio, an unchanged axis, a ratio whose rows take several LDS chunks, and one whose column span does not fit the LDS."""
    rng = np.random.default_rng(src[0] + dst[1])
    B = 3
    crops = np.stack([_edge_crop(rng, src[1], src[0]) for _ in range(B)])
    labels = np.stack([_labels(rng, dst[1], dst[0]) for _ in range(B)])
    (target, mask, inpaint), (dc, dl, lut) = _prep(crops, labels, KEEP, dst)
    for b in range(B):
        ref = _host_item(crops[b], labels[b], KEEP, dst)
        for name, got, want in zip(("target", "mask", "inpaint"), (target, mask, inpaint), ref):
            g = got[b].cpu()
            assert torch.equal(g, want), (name, b, int((g != want).sum()), float((g - want).abs().max()))
    assert 0.0 < float(mask.mean()) < 1.0 and float(target.min()) >= -1.0 and float(target.max()) <= 1.0 and float(target.std()) > 0.0
    # a batch gives every image what it gets alone
    (t1, m1, i1), _ = _prep(crops[1:2], labels[1:2], KEEP, dst)
    assert torch.equal(t1[0], target[1]) and torch.equal(m1[0], mask[1]) and torch.equal(i1[0], inpaint[1])
    # the four launches it replaces
    w, h = dst
    tmp = torch.empty((B, src[1], w, 3), dtype=torch.uint8, device=DEV)
    small = torch.empty((B, h, w, 3), dtype=torch.uint8, device=DEV)
    ops.resample_u8(dc, _dev_taps(src[0], w), _dev_taps(src[1], h), tmp, small)()
    half = torch.full((3,), 0.5, dtype=torch.float32, device=DEV)
    t2, m2, i2 = (torch.empty_like(t) for t in (target, mask, inpaint))
    ops.u8_to_norm(small, half, half, t2)()
    ops.label_mask(dl, lut, m2, invert=True)()
    ops.mul_mask(t2, m2, i2)()
    assert torch.equal(t2, target) and torch.equal(m2, mask) and torch.equal(i2, inpaint)
    if dst == (512, 512):          # and the dataset itself, from PNG files
        os.makedirs(tmp_path / "c")
        os.makedirs(tmp_path / "m")
        Image.fromarray(crops[0]).save(tmp_path / "c" / "0.png")
        Image.fromarray(labels[0]).save(tmp_path / "m" / "0.png")
        for gray in (True, False):
            image, _, kw, _ = VideoDataset(data_path=str(tmp_path / "c"), mask_path=str(tmp_path / "m"), **dict(TEST_ARGS, gray_outer_mask=gray))[0]
            (t, m, i), _ = _prep(crops[:1], labels[:1], KEEP if gray else [2, 3, 5, 6, 7], dst)
            assert torch.equal(t[0].cpu(), image) and torch.equal(m[0].cpu(), kw["inpaint_mask"]) and torch.equal(i[0].cpu(), kw["inpaint_image"])


def test_video_prep_argument_checks():
    lib = _lib.load()
    rng = np.random.default_rng(0)
    crop = torch.from_numpy(rng.integers(1, 256, (1, 9, 7, 3), dtype=np.uint8)).to(DEV)
    lab = torch.zeros((1, 4, 3), dtype=torch.uint8, device=DEV)
    lut = torch.zeros(256, dtype=torch.uint8, device=DEV)
    xb, xk = _dev_taps(7, 3)
    yb, yk = _dev_taps(9, 4)
    t, i = (torch.zeros((1, 3, 4, 3), dtype=torch.float32, device=DEV) for _ in range(2))
    m = torch.zeros((1, 1, 4, 3), dtype=torch.float32, device=DEV)
    args = lambda x=crop.data_ptr(), C=3, ks=xk.shape[1], tt=t.data_ptr(), mm=m.data_ptr(), ii=i.data_ptr(), lb=lab.data_ptr(): (   # noqa: E731
        x, 1, 9, 7, C, lb, lut.data_ptr(), xb.data_ptr(), xk.data_ptr(), ks, yb.data_ptr(), yk.data_ptr(), yk.shape[1], tt, mm, ii, 4, 3, None)
    assert lib.rf_video_prep_u8(*args()) == 0
    torch.cuda.synchronize()
    want = _host_item(crop.cpu().numpy()[0], lab.cpu().numpy()[0], [1], (3, 4))
    assert torch.equal(t[0].cpu(), want[0]) and torch.equal(m[0].cpu(), want[1]) and torch.equal(i[0].cpu(), want[2])
    before = t.clone()
    assert lib.rf_video_prep_u8(*args(C=4)) != 0
    assert b"channels" in lib.rf_last_error()
    assert lib.rf_video_prep_u8(*args(x=None)) != 0
    assert lib.rf_video_prep_u8(*args(lb=None)) != 0
    assert lib.rf_video_prep_u8(*args(ks=0)) != 0
    assert lib.rf_video_prep_u8(*args(ii=t.data_ptr())) != 0
    assert b"three buffers" in lib.rf_last_error()
    assert lib.rf_video_prep_u8(*args(mm=i.data_ptr())) != 0
    assert lib.rf_video_prep_u8(*args(tt=crop.data_ptr())) != 0
    torch.cuda.synchronize()
    assert torch.equal(t, before)          # no launch


def test_paste_on_device_is_paste_back(tmp_path):
    """Frames that are on the device already (RGB and RGBA, two sizes in one batch) get the bytes PasteBack.paste gives the same frames from
    disk; the enlarged crops are rf_paste_crop_u8's."""
    rng = np.random.default_rng(4)
    shapes = [(200, 320, 3), (200, 320, 4), (240, 180, 3), (200, 320, 3)]
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    os.makedirs(tmp_path / "clip")
    for k, f in enumerate(frames):
        if f.shape[2] == 4:
            f[..., 3] = rng.integers(0, 256, f.shape[:2])
        Image.fromarray(f).save(tmp_path / "clip" / f"{k}.png")
    quads = [np.array([[30.0 + 5 * k, 20.0], [25.0, 150.0 + k], [160.0, 160.0], [150.0 + k, 25.0]]) for k in range(4)]
    inv = np.stack([alignment_coefficients(q, 1024) for q in quads])
    x = torch.rand((4, 3, 64, 64), device=DEV)
    ids = [f"{k:012d}" for k in range(4)]
    pb = PasteBack(str(tmp_path / "clip"), inv)
    try:
        want = pb.paste(x, ids)
        dev_frames = [torch.from_numpy(f).to(DEV) for f in frames]
        got = pb.paste_device(x, ids, dev_frames)
        got2, crops = paste_on_device(x, inv, dev_frames)
    finally:
        pb.close()
    ref_crops = torch.empty((4, 1024, 1024, 3), dtype=torch.uint8, device=DEV)
    ops.paste_crop_u8(x, ref_crops)()
    assert torch.equal(crops, ref_crops)
    for k in range(4):
        assert got[k].is_cuda and got[k].dtype == torch.uint8 and tuple(got[k].shape) == shapes[k][:2] + (4,)
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
        assert torch.equal(got2[k], got[k]), k
        assert (want[k][..., :3] != frames[k][..., :3]).any()
    with pytest.raises(ValueError, match="frames"):
        paste_on_device(x, inv, dev_frames[:3])


# ---- the CLI: staged (--align --parse_masks --paste_back) against --stream on the same inputs
def _landmarks_in(W, H, seed, centre=None, eye=None, deg=5.0):
    rng = np.random.default_rng(seed)
    eye = eye or 0.18 * min(W, H)
    cx, cy = centre or (0.5 * W, 0.42 * H)
    t = np.deg2rad(deg)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    lm = rng.uniform(-1.0, 1.0, (68, 2)) * eye
    lm[36:42] = np.array([-0.5, 0.0]) * eye + rng.uniform(-0.1, 0.1, (6, 2)) * eye
    lm[42:48] = np.array([0.5, 0.0]) * eye + rng.uniform(-0.1, 0.1, (6, 2)) * eye
    lm[48], lm[54] = np.array([-0.35, 0.9]) * eye, np.array([0.35, 0.9]) * eye
    return lm @ R.T + [cx, cy]


def _pil_paste(crop, c, frame):
    s = Image.fromarray(crop).convert("RGBA")
    s.putalpha(255)
    p = Image.fromarray(frame).convert("RGBA")
    p.alpha_composite(s.transform(p.size, Image.PERSPECTIVE, tuple(float(v) for v in c), Image.BILINEAR))
    return np.asarray(p)


def _make_inputs(root, N, rgba=(), seed=9):
    """N noise frames 320 x 200 (those in `rgba` with an alpha channel), frame 2 without a face, a source image, both landmark files."""
    rng = np.random.default_rng(seed)
    W, H = 320, 200
    os.makedirs(root / "clip")
    frames = []
    for i in range(N):
        f = rng.integers(0, 256, (H, W, 4 if i in rgba else 3), dtype=np.uint8)
        if i in rgba:
            f[..., 3] = 255          # (decoded video frames are opaque; the staged aligner does not read alpha either)
        Image.fromarray(f).save(root / "clip" / f"{i}.png")
        frames.append(f)
    lm = np.stack([_landmarks_in(W, H, 20 + i, centre=(150.0 + 8 * i, 90.0), deg=4.0 * i) for i in range(N)])
    lm[2] = np.nan
    np.save(root / "lm.npy", lm)
    Image.fromarray(rng.integers(0, 256, (180, 160, 3), dtype=np.uint8)).save(root / "me.jpg")
    np.save(root / "src_lm.npy", _landmarks_in(160, 180, 30))
    return frames


def _copy_inputs(src, dst):
    import shutil
    os.makedirs(dst)
    shutil.copytree(src / "clip", dst / "clip")


def _run(inputs, base, out, *flags):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(out), "--Base_dir", str(base), "--target_video",
           "videos/clip.mp4", "--src_image", str(inputs / "me.jpg"), "--config", os.path.join(ROOT, "tests", "configs", "reface_small.yaml"),
           "--ckpt", "none", "--n_samples", "2", "--ddim_steps", "4", "--scale", "3.5", "--precision", "full", "--num_workers", "0",
           "--clip_vision_config", json.dumps(SMALL_CLIP), "--landmarks", str(inputs / "lm.npy"), "--src_landmarks", str(inputs / "src_lm.npy"),
           "--faceParsing_ckpt", "none", "--dump_tensors", str(out / "dump"), *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return r.stdout


def _png(path):
    return np.asarray(Image.open(path))


def _same_dir(a, b, names):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == sorted(names), (sorted(os.listdir(a)), sorted(os.listdir(b)))
    for n in names:
        x, y = Image.open(os.path.join(a, n)), Image.open(os.path.join(b, n))
        assert x.mode == y.mode and np.array_equal(np.asarray(x), np.asarray(y)), (a, n)


def _compare_runs(staged, stream, n_batches):
    """The sampler's inputs exactly; its output exactly too: two staged runs of the parent commit with one seed are identical on the MI355X
    (the split-K reductions have a fixed order; measured, DESIGN.md section 6 'Streaming'), so the tolerance for x_img is zero."""
    for k in range(n_batches):
        a, b = (np.load(os.path.join(d, "dump", f"batch_{k:04d}.npz")) for d in (staged, stream))
        for name in ("test_batch", "inpaint_image", "inpaint_mask", "ref_imgs", "x_T", "post_noise"):
            assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), (k, name, float(np.abs(a[name] - b[name]).max()))
        d = float(np.abs(a["x_img"] - b["x_img"]).max())
        print(f"batch {k}: max |x_img staged - stream| = {d:.3e}")
        assert d == 0.0, (k, d)


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """4 frames, --n_samples 2: one staged run, one --stream --stream_keep run, one --stream run, each into its own tree."""
    root = tmp_path_factory.mktemp("stream_cli")
    frames = _make_inputs(root, 4)
    runs = {}
    for name, flags in (("staged", ("--align", "--parse_masks", "--paste_back")), ("keep", ("--stream", "--stream_keep")), ("stream", ("--stream",))):
        _copy_inputs(root, root / name / "base")
        runs[name] = {"base": root / name / "base", "out": root / name / "out",
                      "stdout": _run(root, root / name / "base", root / name / "out", *flags)}
    return frames, runs


def test_cli_stream_feeds_the_sampler_what_the_staged_route_feeds_it(cli_runs):
    frames, runs = cli_runs
    st, ke = runs["staged"], runs["keep"]
    inv_a, inv_b = np.load(st["base"] / "clip_inv_transforms.npy", allow_pickle=True), np.load(ke["base"] / "clip_inv_transforms.npy", allow_pickle=True)
    assert inv_a.dtype == inv_b.dtype == np.float64 and inv_a.shape == (4, 8) and np.array_equal(inv_a, inv_b)
    pngs = [f"{i}.png" for i in range(4)]
    _same_dir(st["base"] / "clipcropped_face", ke["base"] / "clipcropped_face", pngs)
    _same_dir(st["base"] / "clipmask_frames", ke["base"] / "clipmask_frames", pngs)
    _same_dir(st["out"] / "temp_results", ke["out"] / "temp_results", ["me.png", "me.jpg"])
    assert np.array_equal(_png(ke["base"] / "clipcropped_face" / "2.png"), _png(ke["base"] / "clipcropped_face" / "1.png"))          # no face in frame 2
    _compare_runs(st["out"], ke["out"], 2)
    ids = [f"{i:012d}.png" for i in range(4)]
    _same_dir(st["out"] / "model_outputs", ke["out"] / "model_outputs", ids)
    _same_dir(st["out"] / "results", ke["out"] / "results", ids)
    assert "4 of 4 frames swapped" in ke["stdout"] and "4 pasted frames" in ke["stdout"]


def test_cli_stream_results_are_pil_paste_of_its_own_outputs(cli_runs):
    frames, runs = cli_runs
    ke = runs["keep"]
    inv = np.load(ke["base"] / "clip_inv_transforms.npy", allow_pickle=True)
    for i in range(4):
        sid = f"{i:012d}.png"
        got = Image.open(ke["out"] / "results" / sid)
        assert got.mode == "RGBA"
        assert np.array_equal(np.asarray(got), _pil_paste(_png(ke["out"] / "model_outputs" / sid), inv[i], frames[i])), sid


def test_cli_stream_alone_writes_no_intermediate_files(cli_runs):
    frames, runs = cli_runs
    ke, so = runs["keep"], runs["stream"]
    _same_dir(ke["out"] / "results", so["out"] / "results", [f"{i:012d}.png" for i in range(4)])
    assert np.array_equal(np.load(ke["base"] / "clip_inv_transforms.npy"), np.load(so["base"] / "clip_inv_transforms.npy"))
    for d in (so["base"] / "clipcropped_face", so["base"] / "clipmask_frames", so["out"] / "model_outputs"):
        assert not os.path.isdir(d) or not os.listdir(d), d
    _same_dir(ke["out"] / "temp_results", so["out"] / "temp_results", ["me.png", "me.jpg"])
    _compare_runs(ke["out"], so["out"], 2)
    assert "no crops, label maps or model_outputs files were written" in so["stdout"]


def test_cli_stream_rgba_frame_and_trailing_frames(tmp_path):
    """5 frames, frame 1 RGBA, --n_samples 2: the fifth frame is never swapped (drop_last).  The transforms file still has its row; with
    --stream_keep its crop / label map are the one difference from the staged tree, which aligns and parses every frame."""
    _make_inputs(tmp_path, 5, rgba=(1,), seed=12)
    for name in ("staged", "keep"):
        _copy_inputs(tmp_path, tmp_path / name / "base")
    _run(tmp_path, tmp_path / "staged" / "base", tmp_path / "staged" / "out", "--align", "--parse_masks", "--paste_back")
    out = _run(tmp_path, tmp_path / "keep" / "base", tmp_path / "keep" / "out", "--stream", "--stream_keep")
    sb, so, kb, ko = (tmp_path / a / b for a in ("staged", "keep") for b in ("base", "out"))
    inv_a, inv_b = np.load(sb / "clip_inv_transforms.npy"), np.load(kb / "clip_inv_transforms.npy")
    assert inv_a.shape == (5, 8) and np.array_equal(inv_a, inv_b)
    _compare_runs(so, ko, 2)
    ids = [f"{i:012d}.png" for i in range(4)]
    _same_dir(so / "results", ko / "results", ids)
    _same_dir(so / "model_outputs", ko / "model_outputs", ids)
    for d in ("clipcropped_face", "clipmask_frames"):
        assert sorted(os.listdir(sb / d)) == [f"{i}.png" for i in range(5)] and sorted(os.listdir(kb / d)) == [f"{i}.png" for i in range(4)]
        for i in range(4):
            assert np.array_equal(_png(sb / d / f"{i}.png"), _png(kb / d / f"{i}.png")), (d, i)
    assert "4 of 5 frames swapped" in out and "1 trailing frames are not swapped" in out
