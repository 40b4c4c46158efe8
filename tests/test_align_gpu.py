"""Face alignment on the GPU (reface_amd/csrc/align.hip, reface_amd/align.py): the LANCZOS shrink and the QUAD / BILINEAR resampling are
byte for byte PIL's (PIL itself being the oracle), the Aligner reproduces the reference's crop_image crops (tests/golden/align.npz), and
align -> paste-back gives the bytes of the same chain in PIL."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from reface_amd import _lib, ops
from reface_amd.align import Aligner, crop_plan, quad_coefficients, quad_from_landmarks, resample_taps
from reface_amd.pasteback import alignment_coefficients

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_align_cpu import CASES, SIZES, golden_case  # noqa: E402


def _pil_quad(frame, quad, S):
    """The reference's transform step on one image (uint8 [H, W, 3 | 4]), kept as RGB."""
    return np.asarray(Image.fromarray(frame).transform((S, S), Image.QUAD, (np.asarray(quad) + 0.5).flatten(), Image.BILINEAR).convert("RGB"))


def _pil_paste(crop, c, frame):
    s = Image.fromarray(crop).convert("RGBA")
    s.putalpha(255)
    p = Image.fromarray(frame).convert("RGBA")
    p.alpha_composite(s.transform(p.size, Image.PERSPECTIVE, tuple(float(v) for v in c), Image.BILINEAR))
    return np.asarray(p)


def _quads(W, H):
    """In frame coordinates (nw, sw, se, ne): rotated inside, rotated the other way and hanging over the top-left corner, skewed over the
    bottom and right edges, entirely outside."""
    def rot(cx, cy, r, deg):
        t = np.deg2rad(deg)
        R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
        return np.array([[-r, -r], [-r, r], [r, r], [r, -r]]) @ R.T + [cx, cy]
    skew = np.array([[0.55 * W, 0.4 * H], [0.5 * W, 1.2 * H], [1.1 * W, 1.15 * H], [1.05 * W, 0.35 * H]])
    away = np.array([[1.5 * W, 1.5 * H], [1.5 * W, 2.0 * H], [2.0 * W, 2.0 * H], [2.0 * W, 1.5 * H]])
    return [rot(W * 0.45, H * 0.5, min(W, H) * 0.3, 23.0), rot(W * 0.1, H * 0.12, min(W, H) * 0.33, -31.0), skew, away]


def _dev_taps(n_in, n_out):
    return tuple(torch.from_numpy(a).to(DEV) for a in resample_taps(n_in, n_out))


@pytest.mark.parametrize("src,dst", [((5000, 3000), (385, 231)), ((1000, 777), (333, 259)), ((640, 480), (320, 240)), ((901, 603), (129, 86)),
                                     ((97, 53), (97, 20))])
@pytest.mark.parametrize("C", [3, 4])
def test_resample_is_pil_lanczos_resize(src, dst, C):
    rng = np.random.default_rng(src[0] + dst[1] + C)
    B = 1 if src[0] > 2000 else 2
    x = rng.integers(0, 256, (B, src[1], src[0], C), dtype=np.uint8)
    if C == 4:
        x[..., 3] = 255          # (PIL resizes RGBA premultiplied: the identity on opaque frames)
    dx = torch.from_numpy(x).to(DEV)
    tmp = torch.empty((B, src[1], dst[0], C), dtype=torch.uint8, device=DEV)
    out = torch.empty((B, dst[1], dst[0], C), dtype=torch.uint8, device=DEV)
    ops.resample_u8(dx, _dev_taps(src[0], dst[0]), _dev_taps(src[1], dst[1]), tmp, out)()
    got = out.cpu().numpy()
    for b in range(B):
        ref = np.asarray(Image.fromarray(x[b]).resize(dst, Image.LANCZOS))
        assert np.array_equal(got[b], ref), (b, int((got[b] != ref).sum()))
    al = Aligner(64)
    assert torch.equal(al.resize(dx, dst), out)


@pytest.mark.parametrize("W,H,S", [(1920, 1080, 256), (1279, 721, 1024), (97, 53, 64), (333, 500, 131)])
@pytest.mark.parametrize("Cf", [3, 4])
def test_align_quad_is_pil_quad_bilinear(W, H, S, Cf):
    rng = np.random.default_rng(W + 10 * Cf + S)
    quads = _quads(W, H)
    B = len(quads)
    frames = rng.integers(0, 256, (B, H, W, Cf), dtype=np.uint8)
    if Cf == 4:
        frames[..., 3] = 255          # (PIL transforms RGBA premultiplied: the identity on opaque frames, which decoded video frames are)
    coeffs = torch.from_numpy(np.stack([quad_coefficients(q, S) for q in quads])).to(DEV)
    # frames strided: each one a slice of a taller buffer (frame stride > H * W * Cf)
    tall = torch.zeros((B, H + 3, W, Cf), dtype=torch.uint8, device=DEV)
    tall[:, :H] = torch.from_numpy(frames).to(DEV)
    out = torch.full((B, S, S, 3), 7, dtype=torch.uint8, device=DEV)
    ops.align_quad_u8(tall[:, :H], coeffs, out)()
    got = out.cpu().numpy()
    for b in range(B):
        ref = _pil_quad(frames[b], quads[b], S)
        assert np.array_equal(got[b], ref), (b, int((got[b] != ref).any(-1).sum()))
    outside = (got == 0).all(-1).mean(axis=(1, 2))
    assert outside[0] < 0.01 and 0.1 < outside[1] < 0.9 and 0.1 < outside[2] < 0.9 and outside[3] == 1.0
    # a batch gives every frame the bytes it gets alone
    for b in range(B):
        one = torch.empty((1, S, S, 3), dtype=torch.uint8, device=DEV)
        ops.align_quad_u8(tall[b:b + 1, :H], coeffs[b:b + 1].contiguous(), one)()
        assert np.array_equal(one.cpu().numpy()[0], got[b]), b
    if Cf == 4:          # alpha is not read: any alpha gives PIL's transform of the R, G, B channels
        tall[..., 3] = torch.randint(0, 256, tall.shape[:3], dtype=torch.uint8, device=DEV)
        ops.align_quad_u8(tall[:, :H], coeffs, out)()
        assert np.array_equal(out.cpu().numpy(), got)
    # a window is PIL's crop before the transform
    ox, oy, w, h = W // 7, H // 5, W // 2, H // 2
    q = quads[0] - [ox, oy]
    win = torch.tensor([[ox, oy, w, h]], dtype=torch.int32, device=DEV)
    one = torch.empty((1, S, S, 3), dtype=torch.uint8, device=DEV)
    ops.align_quad_u8(tall[:1, :H], torch.from_numpy(quad_coefficients(q, S)[None]).to(DEV), one, windows=win)()
    ref = _pil_quad(np.ascontiguousarray(frames[0, oy:oy + h, ox:ox + w]), q, S)
    assert np.array_equal(one.cpu().numpy()[0], ref)


def test_align_argument_checks():
    lib = _lib.load()
    fr = torch.zeros((1, 9, 7, 4), dtype=torch.uint8, device=DEV).random_(1, 256)
    co = torch.from_numpy(quad_coefficients(np.array([[1.0, 1.0], [1.0, 6.0], [5.0, 6.0], [5.0, 1.0]]), 16)[None]).to(DEV)
    out = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    p = [t.data_ptr() for t in (fr, co, out)]
    assert lib.rf_align_quad_u8(p[0], 1, 9, 7, 4, 9 * 7 * 4, p[1], None, 16, p[2], None) == 0
    torch.cuda.synchronize()
    assert out.any()
    assert lib.rf_align_quad_u8(p[0], 1, 9, 7, 5, 9 * 7 * 5, p[1], None, 16, p[2], None) != 0
    assert b"channels" in lib.rf_last_error()
    assert lib.rf_align_quad_u8(p[0], 1, 9, 7, 4, 9 * 7 * 4 - 1, p[1], None, 16, p[2], None) != 0
    assert lib.rf_align_quad_u8(None, 1, 9, 7, 4, 9 * 7 * 4, p[1], None, 16, p[2], None) != 0
    assert lib.rf_align_quad_u8(p[0], 1, 9, 7, 4, 9 * 7 * 4, p[1], None, 0, p[2], None) != 0
    assert lib.rf_align_quad_u8(p[0], 1, 9, 7, 4, 9 * 7 * 4, p[1], None, 16, p[0], None) != 0
    # non-finite coordinates (NaN, +-inf) are outside: zeros
    inf = float("inf")
    for c in ([float("nan")] * 8, [inf, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, -inf, 1, 0, 0], [inf, -inf, 0, 0, 1, 0, 0, 0]):
        out.fill_(9)
        ops.align_quad_u8(fr, torch.tensor([c], dtype=torch.float64, device=DEV), out)()
        assert not out.any(), c
    # a window that does not lie inside the frame reads nothing: zeros
    for w in ([-1, 0, 4, 4], [0, 0, 8, 4], [3, 0, 5, 4], [0, 6, 4, 4], [0, 0, 0, 4], [2 ** 31 - 1, 0, 4, 4]):
        out.fill_(9)
        ops.align_quad_u8(fr, co, out, windows=torch.tensor([w], dtype=torch.int32, device=DEV))()
        assert not out.any(), w
    # rf_resample_u8
    xb, xk = (torch.from_numpy(a).to(DEV) for a in resample_taps(7, 3))
    yb, yk = (torch.from_numpy(a).to(DEV) for a in resample_taps(9, 4))
    tmp = torch.zeros((1, 9, 3, 4), dtype=torch.uint8, device=DEV)
    o = torch.zeros((1, 4, 3, 4), dtype=torch.uint8, device=DEV)
    args = lambda x=fr.data_ptr(), C=4, t=tmp.data_ptr(), oo=o.data_ptr(), ks=xk.shape[1]: (x, 1, 9, 7, C, xb.data_ptr(), xk.data_ptr(), ks, yb.data_ptr(),   # noqa: E731
                                                                                           yk.data_ptr(), yk.shape[1], t, oo, 4, 3, None)
    assert lib.rf_resample_u8(*args()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy()[0][..., :3], np.asarray(Image.fromarray(fr.cpu().numpy()[0][..., :3]).resize((3, 4), Image.LANCZOS)))
    assert lib.rf_resample_u8(*args(C=2)) != 0
    assert lib.rf_resample_u8(*args(x=None)) != 0
    assert lib.rf_resample_u8(*args(ks=0)) != 0
    assert lib.rf_resample_u8(*args(t=o.data_ptr())) != 0
    assert b"three buffers" in lib.rf_last_error()


@pytest.mark.parametrize("S", SIZES)
def test_aligner_reproduces_the_reference_crops(golden_dir, S):
    """End to end from landmarks, all four fixture cases in one call (three frame sizes, RGB and RGBA, one LANCZOS shrink): the reference's
    crop_image bytes and quads."""
    G = np.load(os.path.join(golden_dir, "align.npz"))
    al = Aligner(S)
    frames = [golden_case(G, n) for n in CASES]
    crops, quads = al.align(frames, landmarks=[G[n + "_landmarks"] for n in CASES])
    assert crops.shape == (len(CASES), S, S, 3) and crops.dtype == torch.uint8 and crops.is_cuda
    got = crops.cpu().numpy()
    for i, n in enumerate(CASES):
        assert np.array_equal(quads[i], G[n + "_quad"]), n
        ref = G[f"{n}_crop{S}"]
        assert np.array_equal(got[i], ref), (n, int((got[i] != ref).sum()))
    assert crop_plan(quads[3], (frames[3].shape[1], frames[3].shape[0]), S).shrink > 1
    inv = al.inverse_transforms()
    assert np.array_equal(inv, np.stack([alignment_coefficients(q, S) for q in quads]))
    # from quads, and from files on disk, the same crops
    again, _ = al.align(frames[:2], quads=quads[:2])
    assert torch.equal(again, crops[:2])


def test_aligner_shrinks_over_the_edge_like_pil(tmp_path):
    """A face that needs the LANCZOS shrink AND hangs over the frame's bottom-right corner, read from a PNG: crop_image's steps in PIL."""
    rng = np.random.default_rng(11)
    W, H, S = 1503, 1001, 64
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    path = str(tmp_path / "f.png")
    Image.fromarray(frame).save(path)
    t = np.deg2rad(-14.0)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    quad = np.array([[-350.0, -350.0], [-350.0, 350.0], [350.0, 350.0], [350.0, -350.0]]) @ R.T + [1300.0, 850.0]
    p = crop_plan(quad, (W, H), S)
    assert p.shrink == 7 and p.window[0] > 0 and p.window[1] > 0
    img = Image.fromarray(frame).resize(p.rsize, Image.LANCZOS)
    ox, oy, w, h = p.window
    ref = np.asarray(img.crop((ox, oy, ox + w, oy + h)).transform((S, S), Image.QUAD, (p.quad + 0.5).flatten(), Image.BILINEAR))
    crops, _ = Aligner(S).align([path], quads=[quad])
    got = crops.cpu().numpy()[0]
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert 0.05 < (got == 0).all(-1).mean() < 0.9


def test_align_then_paste_back_is_the_pil_chain():
    """Round trip: a frame aligned to a crop, the crop pasted back with the inverse transform.  The GPU chain (rf_align_quad_u8 ->
    rf_paste_back_u8) gives the bytes of the PIL chain (the reference's arithmetic); how close either comes to the original frame well
    inside the quad is printed, not asserted: it is a property of two bilinear resamplings, the same number for both chains."""
    W, H, S = 640, 480, 512
    yy, xx = np.mgrid[:H, :W]
    rng = np.random.default_rng(2)
    smooth = np.stack([127 + 100 * np.sin(xx / 17.0 + k) * np.cos(yy / 23.0 - k) for k in range(3)], -1)
    frame = np.clip(smooth + rng.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    quad = _quads(W, H)[0]
    crops, quads = Aligner(S).align([frame], quads=[quad])
    inv = alignment_coefficients(quad, S)
    out = torch.empty((1, H, W, 4), dtype=torch.uint8, device=DEV)
    ops.paste_back_u8(crops, torch.from_numpy(inv[None]).to(DEV), torch.from_numpy(np.stack([frame])).to(DEV), out)()
    got = out.cpu().numpy()[0]
    pil_crop = _pil_quad(frame, quad, S)
    assert np.array_equal(crops.cpu().numpy()[0], pil_crop)
    ref = _pil_paste(pil_crop, inv, frame)
    assert np.array_equal(got, ref), int((got != ref).any(-1).sum())
    # well inside the quad: the inner half of it, mapped through the inverse transform
    x, y = xx + 0.5, yy + 0.5
    d = inv[6] * x + inv[7] * y + 1
    u, v = (inv[0] * x + inv[1] * y + inv[2]) / d, (inv[3] * x + inv[4] * y + inv[5]) / d
    inner = (np.abs(u - S / 2) < S / 4) & (np.abs(v - S / 2) < S / 4)
    err = np.abs(got[..., :3].astype(int) - frame.astype(int))[inner]
    print(f"round trip inside the quad ({int(inner.sum())} px): max |d| = {err.max()}, mean |d| = {err.mean():.3f} grey levels (GPU == PIL chain)")
    assert inner.sum() > 1000


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


def _pil_crop_image(frame, lm, S=1024):
    """crop_image in PIL for a face that needs no shrink."""
    quad = quad_from_landmarks(lm)[3]
    p = crop_plan(quad, (frame.shape[1], frame.shape[0]), S)
    assert p.shrink <= 1
    ox, oy, w, h = p.window
    return _pil_quad(np.ascontiguousarray(frame[oy:oy + h, ox:ox + w]), p.quad, S), quad


def test_cli_swap_video_from_raw_frames(tmp_path):
    """--align --parse_masks --paste_back: raw frames + landmarks to pasted frames in one command.  The three products of the alignment
    are written in the reference's layout, the crops are PIL's, a frame without a face repeats the previous crop and transform, and the
    pasted frames are PIL's paste of the model outputs with those transforms."""
    base, out = tmp_path / "base", tmp_path / "out"
    (base / "clip").mkdir(parents=True)
    rng = np.random.default_rng(9)
    W, H, N = 320, 200, 4
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(base / "clip" / f"{i}.png")
    lm = np.stack([_landmarks_in(W, H, 20 + i, centre=(150.0 + 8 * i, 90.0), deg=4.0 * i) for i in range(N)])
    lm[2] = np.nan                                             # "no face" in frame 2
    np.save(tmp_path / "lm.npy", lm)
    src = rng.integers(0, 256, (180, 160, 3), dtype=np.uint8)
    Image.fromarray(src).save(tmp_path / "me.jpg")             # (.jpg: the source's label map is written as temp_results/<basename(src_image)>)
    src = np.asarray(Image.open(tmp_path / "me.jpg"))
    src_lm = _landmarks_in(160, 180, 30)
    np.save(tmp_path / "src_lm.npy", src_lm)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(out), "--Base_dir", str(base), "--target_video",
           "videos/clip.mp4", "--src_image", str(tmp_path / "me.jpg"), "--config", os.path.join(ROOT, "tests", "configs", "reface_small.yaml"),
           "--ckpt", "none", "--n_samples", "2", "--ddim_steps", "4", "--scale", "3.5", "--precision", "full", "--num_workers", "0",
           "--clip_vision_config", json.dumps(SMALL_CLIP), "--align", "--landmarks", str(tmp_path / "lm.npy"), "--src_landmarks",
           str(tmp_path / "src_lm.npy"), "--parse_masks", "--faceParsing_ckpt", "none", "--paste_back"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "4 frames aligned" in r.stdout and "4 pasted frames" in r.stdout
    # the three products
    assert sorted(os.listdir(base / "clipcropped_face")) == [f"{i}.png" for i in range(N)]
    inv = np.load(base / "clip_inv_transforms.npy", allow_pickle=True)
    assert inv.shape == (N, 8) and inv.dtype == np.float64
    got_src = Image.open(out / "temp_results" / "me.png")
    assert got_src.mode == "RGB" and np.array_equal(np.asarray(got_src), _pil_crop_image(src, src_lm)[0])
    for i in range(N):
        j = 1 if i == 2 else i
        ref, quad = _pil_crop_image(frames[j], lm[j])
        im = Image.open(base / "clipcropped_face" / f"{i}.png")
        assert im.mode == "RGB" and im.size == (1024, 1024)
        assert np.array_equal(np.asarray(im), ref), (i, int((np.asarray(im) != ref).sum()))
        assert np.array_equal(inv[i], alignment_coefficients(quad, 1024)), i
    # the parser filled in the label maps, and stage 3 pasted every swapped crop into its frame with the transforms written above
    assert sorted(os.listdir(base / "clipmask_frames")) == [f"{i}.png" for i in range(N)] and os.path.isfile(out / "temp_results" / "me.jpg")
    ids = [f"{i:012d}" for i in range(N)]
    assert sorted(os.listdir(out / "results")) == [s + ".png" for s in ids]
    for i, sid in enumerate(ids):
        mo = np.asarray(Image.open(out / "model_outputs" / (sid + ".png")))
        got = np.asarray(Image.open(out / "results" / (sid + ".png")))
        assert np.array_equal(got, _pil_paste(mo, inv[i], frames[i])), sid


def test_cli_swap_selected_align(tmp_path):
    """--align of the selected-swap caller: target and source folders to <Base_dir>/{target_cropped,source_cropped}, an image without a
    face skipped and the numbering closed up.  (Without label maps and --parse_masks the run then stops at its usual stage-1 message:
    no model is loaded here.)"""
    tar, srcd, base = tmp_path / "tar", tmp_path / "src", tmp_path / "base"
    tar.mkdir()
    srcd.mkdir()
    rng = np.random.default_rng(4)
    imgs = {}
    for d, names, size in ((tar, ["a.png", "b.png", "c.png"], (200, 240)), (srcd, ["s.png"], (150, 150))):
        for n in names:
            imgs[n] = rng.integers(0, 256, size + (3,), dtype=np.uint8)
            Image.fromarray(imgs[n]).save(d / n)
    lm = np.stack([_landmarks_in(240, 200, 40 + i) for i in range(3)])
    lm[1] = np.nan
    slm = _landmarks_in(150, 150, 50)[None]
    np.save(tmp_path / "lm.npy", lm)
    np.save(tmp_path / "slm.npy", slm)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_selected.py"), "--outdir", str(tmp_path / "out"), "--Base_dir", str(base),
           "--target_folder", str(tar), "--src_folder", str(srcd), "--config", os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt",
           "none", "--align", "--landmarks", str(tmp_path / "lm.npy"), "--src_landmarks", str(tmp_path / "slm.npy")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode != 0 and "mask_frames" in (r.stderr + r.stdout), r.stdout[-1500:] + r.stderr[-1500:]
    assert sorted(os.listdir(base / "target_cropped")) == ["0.png", "1.png"] and os.listdir(base / "source_cropped") == ["0.png"]
    for f, name, l in (("target_cropped/0.png", "a.png", lm[0]), ("target_cropped/1.png", "c.png", lm[2]), ("source_cropped/0.png", "s.png", slm[0])):
        assert np.array_equal(np.asarray(Image.open(base / f)), _pil_crop_image(imgs[name], l)[0]), f
