"""The masked paste on the GPU (reface_amd/csrc/pasteback.hip: rf_paste_alpha_u8, rf_paste_back_alpha_u8): the alpha plane equals its
integer definition (steps 1-3: tests/paste_mask_refs.py) and PIL's BILINEAR resize (step 4); the paste equals PIL's own chain
putalpha -> transform(PERSPECTIVE, BILINEAR) -> alpha_composite, zero differing bytes; ``inference_swap_video.py --paste_mask`` end to end."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paste_mask_refs as R  # noqa: E402
from test_paste_back_gpu import _quads  # noqa: E402

from reface_amd import _lib, ops  # noqa: E402
from reface_amd.pasteback import PasteMask, alignment_coefficients, paste_on_device  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
REMOVE = [1, 2, 3, 5, 6, 7, 9]          # tests/configs/reface_small.yaml: remove_mask_tar_FFHQ
KEPT = [0, 4, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 200, 255]
EXTREMES = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _label_maps(n, seed):
    """[5, n, n]: a disc, a disc cut by the border, a one-pixel checkerboard, all repainted, none repainted -- the repainted and the kept
    regions each a noise of several labels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:n, :n]
    on, off = rng.choice(REMOVE, (n, n)).astype(np.uint8), rng.choice(KEPT, (n, n)).astype(np.uint8)
    disc = np.hypot(yy - 0.45 * n, xx - 0.55 * n) < 0.27 * n
    cut = np.hypot(yy - 0.9 * n, xx - 0.05 * n) < 0.3 * n
    board = (yy + xx) % 2 == 0
    return np.stack([np.where(m, on, off) for m in (disc, cut, board, np.ones((n, n), bool), np.zeros((n, n), bool))])


def _alpha(labels, lut, S, d, r, passes):
    B, n = labels.shape[:2]
    out = torch.full((B, S, S), 77, dtype=torch.uint8, device=DEV)
    scratch = torch.empty(2 * B * n * n, dtype=torch.uint8, device=DEV)
    ops.paste_alpha_u8(labels, lut, out, scratch, d, r, passes)()
    return out.cpu().numpy()


@pytest.mark.parametrize("d,r,passes", [(0, 0, 1), (3, 4, 2), (1, 64, 1), (64, 1, 3), (8, 8, 2)])
@pytest.mark.parametrize("Sl,S", [(32, 64), (37, 37), (512, 1024)])
def test_alpha_plane_is_its_definition(Sl, S, d, r, passes):
    maps = _label_maps(Sl, Sl + d)
    lut_host = PasteMask(REMOVE).lut_host
    lut, dmaps = _dev(lut_host), _dev(maps)
    small = _alpha(dmaps, lut, Sl, d, r, passes)          # S == Sl: steps 1-3 alone
    batch = small if S == Sl else _alpha(dmaps, lut, S, d, r, passes)
    for b in range(maps.shape[0]):
        want = R.alpha_small(maps[b], lut_host, d, r, passes)
        assert np.array_equal(small[b], want), (b, int((small[b] != want).sum()))
        if S != Sl:
            ref = np.asarray(Image.fromarray(want).resize((S, S), Image.BILINEAR))
            assert np.array_equal(batch[b], ref), (b, int((batch[b] != ref).sum()))
        alone = _alpha(dmaps[b:b + 1].contiguous(), lut, S, d, r, passes)          # B = 1
        assert np.array_equal(alone[0], batch[b]), b
    assert small[3].any() and not small[4].any()
    # alpha falls off towards the border even where every label is repainted; without a feather it is 255 there
    assert small[3][0, 0] < 255 if r > 0 else (small[3] == 255).all()


def test_alpha_argument_checks():
    lib = _lib.load()
    lab = torch.zeros((1, 16, 16), dtype=torch.uint8, device=DEV)
    lut = torch.zeros(256, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros(2 * 256, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 32, 32), 9, dtype=torch.uint8, device=DEV)
    p = [t.data_ptr() for t in (lab, lut, scratch, out)]
    call = lambda lab=p[0], Sl=16, lut=p[1], d=8, r=8, n=2, sc=p[2], nb=512, out=p[3], S=32: lib.rf_paste_alpha_u8(lab, 1, Sl, lut, d, r, n, sc, nb, out, S, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert not out.any()
    out.fill_(9)
    for kw, msg in ((dict(d=-1), b"0 .. 64"), (dict(d=65), b"0 .. 64"), (dict(r=-1), b"0 .. 64"), (dict(r=65), b"0 .. 64"), (dict(n=0), b"passes"),
                    (dict(n=4), b"passes"), (dict(S=15), b"only upscaling"), (dict(lab=None), b"bad arguments"), (dict(lut=None), b"bad arguments"),
                    (dict(sc=None), b"bad arguments"), (dict(out=None), b"bad arguments"), (dict(nb=511), b"scratch")):
        assert call(**kw) != 0, kw
        assert msg in lib.rf_last_error(), (kw, lib.rf_last_error())
    torch.cuda.synchronize()
    assert (out == 9).all()          # no launch


def _masks(rng, S):
    """Random bytes with the extreme values in a third of the places; a smooth ramp that is 0 and 255 over parts of the crop."""
    rnd = rng.integers(0, 256, (S, S), dtype=np.uint8)
    sel = rng.random((S, S)) < 0.33
    rnd[sel] = rng.choice(EXTREMES, int(sel.sum()))
    yy, xx = np.mgrid[:S, :S]
    ramp = np.clip(255.0 * (1.25 - np.hypot(yy - 0.5 * S, xx - 0.45 * S) / (0.4 * S)), 0, 255).astype(np.uint8)
    return rnd, ramp


@pytest.mark.parametrize("W,H,S", [(97, 53, 64), (1279, 721, 256), (1920, 1080, 1024)])
@pytest.mark.parametrize("Cf,Co", [(3, 4), (3, 3), (4, 4), (4, 3)])
def test_paste_is_pil_putalpha_transform_composite(W, H, S, Cf, Co):
    rng = np.random.default_rng(W + 10 * Cf + Co)
    rot, skew, away = _quads(W, H)
    rnd, ramp = _masks(rng, S)
    quads, alphas = [rot, skew, away, rot, skew], np.stack([rnd, ramp, rnd, ramp, rnd])
    B = len(quads)
    crops = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (B, H, W, Cf), dtype=np.uint8)          # (RGBA frames: arbitrary alpha)
    if Cf == 4:
        frames[:, :6, :, 3] = EXTREMES[:, None]
    coeffs = np.stack([alignment_coefficients(q, S) for q in quads])
    tall = torch.zeros((B, H + 3, W, Cf), dtype=torch.uint8, device=DEV)          # strided frames: each a slice of a taller buffer
    tall[:, :H] = _dev(frames)
    out = torch.empty((B, H, W, Co), dtype=torch.uint8, device=DEV)
    dcrops, dal, dco = _dev(crops), _dev(alphas), _dev(coeffs)
    ops.paste_back_alpha_u8(dcrops, dal, dco, tall[:, :H], out)()
    got = out.cpu().numpy()
    for b in range(B):
        ref = R._pil_paste_alpha(crops[b], alphas[b], coeffs[b], frames[b], Co)
        assert np.array_equal(got[b], ref), (b, int((got[b] != ref).any(-1).sum()))
    changed = (got[..., :3] != frames[..., :3]).any(-1)
    assert changed[0].mean() > 0.01 and changed[1].any() and not changed[2].any()          # the third quad lies wholly outside its frame
    for b in range(B):          # the batch gives every frame the bytes it gets alone
        one = torch.empty((1, H, W, Co), dtype=torch.uint8, device=DEV)
        ops.paste_back_alpha_u8(dcrops[b:b + 1].contiguous(), dal[b:b + 1].contiguous(), dco[b:b + 1].contiguous(), tall[b:b + 1, :H], one)()
        assert torch.equal(one[0], out[b]), b
    if Cf == Co:          # in place: out == frames (packed)
        fr = _dev(frames)
        ops.paste_back_alpha_u8(dcrops, dal, dco, fr, fr)()
        assert torch.equal(fr, out)


@pytest.mark.parametrize("Cf,Co", [(3, 4), (4, 4), (4, 3)])
def test_mask_extremes(Cf, Co):
    W, H, S = 321, 203, 128
    rng = np.random.default_rng(7 + Cf + Co)
    quads = _quads(W, H)
    B = len(quads)
    crops = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (B, H, W, Cf), dtype=np.uint8)
    coeffs = np.stack([alignment_coefficients(q, S) for q in quads])
    dcrops, dco, dfr = _dev(crops), _dev(coeffs), _dev(frames)

    def paste(alpha):
        out = torch.empty((B, H, W, Co), dtype=torch.uint8, device=DEV)
        ops.paste_back_alpha_u8(dcrops, _dev(alpha), dco, dfr, out)()
        return out

    plain = torch.empty((B, H, W, Co), dtype=torch.uint8, device=DEV)
    ops.paste_back_u8(dcrops, dco, dfr, plain)()
    assert torch.equal(paste(np.full((B, S, S), 255, np.uint8)), plain)          # alpha 255 everywhere: the unmasked paste
    assert (plain.cpu().numpy()[..., :3] != frames[..., :3]).any()
    keep = paste(np.zeros((B, S, S), np.uint8)).cpu().numpy()          # alpha 0 everywhere: the frame (alpha 255 for RGB frames)
    n = min(Cf, Co)
    assert np.array_equal(keep[..., :n], frames[..., :n]) and (Cf == 4 or Co == 3 or (keep[..., 3] == 255).all())
    # blocks of 0 beside blocks of other values: every output pixel whose four taps have alpha 0 is the frame's pixel
    blocks = rng.choice(EXTREMES, (B, S // 8, S // 8)).repeat(8, 1).repeat(8, 2)
    got = paste(blocks).cpu().numpy()
    for b in range(B):
        zero = R.taps_alpha_zero(blocks[b], coeffs[b], H, W)
        assert b == 2 or (zero.any() and not zero.all())
        assert np.array_equal(got[b][zero][:, :n], frames[b][zero][:, :n]), b
        assert np.array_equal(got[b], R._pil_paste_alpha(crops[b], blocks[b], coeffs[b], frames[b], Co)), b


def test_paste_argument_checks():
    lib = _lib.load()
    crops = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    al = torch.full((1, 16, 16), 200, dtype=torch.uint8, device=DEV)
    co = torch.zeros((1, 8), dtype=torch.float64, device=DEV)
    fr = torch.zeros((1, 9, 7, 4), dtype=torch.uint8, device=DEV)
    out = torch.zeros((1, 9, 7, 4), dtype=torch.uint8, device=DEV)
    p = [t.data_ptr() for t in (crops, al, co, fr, out)]
    f = lib.rf_paste_back_alpha_u8
    assert f(p[0], p[1], 1, 16, p[2], p[3], 9, 7, 4, 9 * 7 * 4, p[4], 4, None) == 0
    torch.cuda.synchronize()
    assert f(p[0], p[1], 1, 16, p[2], p[3], 9, 7, 5, 9 * 7 * 5, p[4], 4, None) != 0
    assert f(p[0], p[1], 1, 16, p[2], p[3], 9, 7, 4, 9 * 7 * 4, p[4], 2, None) != 0
    assert b"channels must be 3 or 4" in lib.rf_last_error()
    assert f(p[0], p[1], 1, 16, p[2], p[3], 9, 7, 4, 9 * 7 * 4 - 1, p[4], 4, None) != 0
    assert b"frame stride" in lib.rf_last_error()
    assert f(None, p[1], 1, 16, p[2], p[3], 9, 7, 4, 9 * 7 * 4, p[4], 4, None) != 0
    assert f(p[0], None, 1, 16, p[2], p[3], 9, 7, 4, 9 * 7 * 4, p[4], 4, None) != 0
    assert b"rf_paste_back_alpha_u8: bad arguments" in lib.rf_last_error()
    assert f(p[0], p[1], 1, 16, p[2], p[3], 9, 7, 4, 9 * 7 * 4, p[3], 3, None) != 0          # in place across channel counts
    assert b"in place" in lib.rf_last_error()
    # non-finite source coordinates (NaN, +-inf) keep the frame
    inf = float("inf")
    fr.random_(0, 256)
    for c in ([float("nan")] * 8, [inf, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, -inf, 0, 0], [inf, 0, -inf, 0, 1, 0, 0, 0]):
        ops.paste_back_alpha_u8(crops, al, torch.tensor([c], dtype=torch.float64, device=DEV), fr, out)()
        assert torch.equal(out, fr), c


def test_paste_on_device_with_a_mask():
    """``paste_on_device(labels=, mask=)`` (frames of two sizes and channel counts in one batch) is the alpha op followed by the paste op;
    without a mask the label maps are not read and the bytes are the unmasked paste's."""
    rng = np.random.default_rng(11)
    shapes = [(200, 320, 3), (200, 320, 4), (240, 180, 3)]
    frames = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    quads = [np.array([[30.0 + 5 * k, 20.0], [25.0, 150.0 + k], [160.0, 160.0], [150.0 + k, 25.0]]) for k in range(3)]
    S, Sl = 128, 64
    inv = np.stack([alignment_coefficients(q, S) for q in quads])
    x = torch.rand((3, 3, 48, 48), device=DEV)
    labels = _label_maps(Sl, 3)[:3]
    mask = PasteMask(REMOVE, dilate=2, feather=3, passes=2)
    dframes = [_dev(f) for f in frames]
    got, crops = paste_on_device(x, inv, dframes, crop_size=S, labels=_dev(labels), mask=mask)
    plain, crops2 = paste_on_device(x, inv, dframes, crop_size=S)
    ignored, _ = paste_on_device(x, inv, dframes, crop_size=S, labels=_dev(labels))
    assert torch.equal(crops, crops2)
    hc = crops.cpu().numpy()
    for k in range(3):
        alpha = R.alpha_plane(labels[k], mask.lut_host, 2, 3, 2, S)
        assert np.array_equal(mask.alpha(_dev(labels[k:k + 1]), S).cpu().numpy()[0], alpha)
        assert np.array_equal(got[k].cpu().numpy(), R._pil_paste_alpha(hc[k], alpha, inv[k], frames[k], 4)), k
        assert torch.equal(plain[k], ignored[k]) and not torch.equal(plain[k], got[k])
    with pytest.raises(ValueError, match="label maps"):
        paste_on_device(x, inv, dframes, crop_size=S, mask=mask)
    with pytest.raises(ValueError, match="label maps for a batch"):
        paste_on_device(x, inv, dframes, crop_size=S, labels=_dev(labels[:2]), mask=mask)


# ---- the CLI
@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """4 frames (frame 1 RGBA, frame 2 without a face), --n_samples 2: a masked --stream --stream_keep --write_video run; a masked --paste_back
    run on the tree that run kept; an unmasked --stream run."""
    import test_stream_gpu as S
    root = tmp_path_factory.mktemp("paste_mask_cli")
    frames = S._make_inputs(root, 4, rgba=(1,), seed=12)
    runs = {}
    for name, flags in (("masked", ("--stream", "--stream_keep", "--paste_mask", "--write_video")), ("plain", ("--stream",))):
        S._copy_inputs(root, root / name / "base")
        runs[name] = {"base": root / name / "base", "out": root / name / "out", "stdout": S._run(root, root / name / "base", root / name / "out", *flags)}
    # the staged route on what the stream kept: crops, label maps, inverse transforms and the source's files
    shutil.copytree(runs["masked"]["base"], root / "staged" / "base")
    os.makedirs(root / "staged" / "out")
    shutil.copytree(runs["masked"]["out"] / "temp_results", root / "staged" / "out" / "temp_results")
    runs["staged"] = {"base": root / "staged" / "base", "out": root / "staged" / "out",
                      "stdout": S._run(root, root / "staged" / "base", root / "staged" / "out", "--paste_back", "--paste_mask", "--paste_dilate", "8")}
    return frames, runs


def _png(path):
    return np.asarray(Image.open(path))


def test_cli_stream_paste_mask_is_pil_of_the_kept_files(cli_runs):
    frames, runs = cli_runs
    ma = runs["masked"]
    inv = np.load(ma["base"] / "clip_inv_transforms.npy", allow_pickle=True)
    lut = PasteMask(REMOVE).lut_host
    assert sorted(os.listdir(ma["out"] / "results")) == [f"{i:012d}.png" for i in range(4)]
    for i in range(4):
        sid = f"{i:012d}.png"
        labels = _png(ma["base"] / "clipmask_frames" / f"{i}.png")
        assert labels.shape == (512, 512) and labels.dtype == np.uint8
        alpha = R.alpha_plane(labels, lut, 8, 8, 2, 1024)
        got = Image.open(ma["out"] / "results" / sid)
        assert got.mode == "RGBA"
        ref = R._pil_paste_alpha(_png(ma["out"] / "model_outputs" / sid), alpha, inv[i], frames[i], 4)
        assert np.array_equal(np.asarray(got), ref), (sid, int((np.asarray(got) != ref).any(-1).sum()))
    assert np.array_equal(_png(ma["base"] / "clipmask_frames" / "2.png"), _png(ma["base"] / "clipmask_frames" / "1.png"))          # no face in frame 2
    last = ma["stdout"].splitlines()[-1]
    assert "--paste_mask: dilate 8, feather 8" in last and "4 pasted frames" in last
    assert "--paste_mask" not in runs["plain"]["stdout"].splitlines()[-1]


def test_cli_paste_back_paste_mask_gives_the_streams_frames(cli_runs):
    frames, runs = cli_runs
    ma, st = runs["masked"], runs["staged"]
    names = [f"{i:012d}.png" for i in range(4)]
    assert sorted(os.listdir(st["out"] / "results")) == names
    for n in names:
        assert np.array_equal(_png(st["out"] / "model_outputs" / n), _png(ma["out"] / "model_outputs" / n)), n
        a, b = Image.open(st["out"] / "results" / n), Image.open(ma["out"] / "results" / n)
        assert a.mode == b.mode == "RGBA" and np.array_equal(np.asarray(a), np.asarray(b)), n
    assert "--paste_mask: dilate 8, feather 8" in st["stdout"].splitlines()[-1]


@pytest.mark.parametrize("flags", [("--gpu_png_decode",), ("--gpu_png",), ("--gpu_png", "--gpu_png_decode")], ids=["device_frames", "gpu_png", "both"])
def test_cli_paste_back_paste_mask_other_branches(cli_runs, tmp_path, flags):
    """The --paste_back branches that paste frames on the device (decoded there, or uploaded for the device PNG encoder; the label maps come
    from the prefetch pool or are read when the batch is pasted): the same decoded frames."""
    import test_stream_gpu as S
    frames, runs = cli_runs
    ma, st = runs["masked"], runs["staged"]
    out = tmp_path / "out"
    os.makedirs(out)
    shutil.copytree(ma["out"] / "temp_results", out / "temp_results")
    stdout = S._run(st["base"].parent.parent, st["base"], out, "--paste_back", "--paste_mask", *flags)
    names = [f"{i:012d}.png" for i in range(4)]
    assert sorted(os.listdir(out / "results")) == names
    for n in names:
        a, b = Image.open(out / "results" / n), Image.open(ma["out"] / "results" / n)
        assert a.mode == b.mode == "RGBA" and np.array_equal(np.asarray(a), np.asarray(b)), n
    assert "--paste_mask: dilate 8, feather 8" in stdout.splitlines()[-1]


def test_cli_paste_mask_video_holds_the_masked_frames(cli_runs):
    import jpeg_refs as J
    frames, runs = cli_runs
    ma = runs["masked"]
    a = J.parse_avi(open(ma["out"] / "clip_swapped.avi", "rb").read())
    assert a["total_frames"] == len(a["frames"]) == 4
    for i in range(4):
        assert a["frames"][i] == J.pil_jpeg(_png(ma["out"] / "results" / f"{i:012d}.png"), 90, "420"), i


def test_cli_paste_mask_with_video_in(cli_runs, tmp_path):
    """--video_in: the masked run's own AVI as the frames of another masked run (frames decoded on the GPU, no PNG frame on disk)."""
    import io
    import jpeg_refs as J
    import test_stream_gpu as S
    frames, runs = cli_runs
    avi = runs["masked"]["out"] / "clip_swapped.avi"
    base, out = tmp_path / "base", tmp_path / "out"
    os.makedirs(base)
    S._run(runs["masked"]["base"].parent.parent, base, out, "--stream", "--stream_keep", "--paste_mask", "--paste_feather", "3", "--video_in", str(avi))
    inv = np.load(base / "clip_inv_transforms.npy", allow_pickle=True)
    lut = PasteMask(REMOVE).lut_host
    jpegs = J.parse_avi(open(avi, "rb").read())["frames"]
    for i in range(4):
        sid = f"{i:012d}.png"
        frame = np.asarray(Image.open(io.BytesIO(jpegs[i])).convert("RGB"))
        alpha = R.alpha_plane(_png(base / "clipmask_frames" / f"{i}.png"), lut, 8, 3, 2, 1024)
        ref = R._pil_paste_alpha(_png(out / "model_outputs" / sid), alpha, inv[i], frame, 4)
        assert np.array_equal(_png(out / "results" / sid), ref), sid


def test_cli_paste_mask_changes_pixels_only_inside_the_quad(cli_runs):
    frames, runs = cli_runs
    ma, pl = runs["masked"], runs["plain"]
    inv = np.load(ma["base"] / "clip_inv_transforms.npy", allow_pickle=True)
    assert np.array_equal(inv, np.load(pl["base"] / "clip_inv_transforms.npy", allow_pickle=True))
    differ = 0
    for i in range(4):
        sid = f"{i:012d}.png"
        a, b = _png(ma["out"] / "results" / sid), _png(pl["out"] / "results" / sid)
        H, W = a.shape[:2]
        inside = _inside(inv[i], H, W)
        diff = (a != b).any(-1)
        assert not (diff & ~inside).any(), sid
        f = frames[i]
        assert np.array_equal(a[~inside][:, :3], f[~inside][:, :3]) and np.array_equal(b[~inside][:, :3], f[~inside][:, :3])
        differ += int(diff.sum())
    assert differ > 0


def _inside(c, H, W):
    """[H, W] bool: the output pixels whose source coordinates lie inside the 1024^2 crop (the quad)."""
    return R.taps_alpha_zero(np.zeros((1024, 1024), np.uint8), c, H, W)
