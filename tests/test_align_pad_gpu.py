"""crop_image's enable_padding branch on the GPU (reface_amd/csrc/align_pad.hip): rf_align_pad_u8 gives the bytes of the numpy / scipy
recipe (reface_amd.align.pad_image_host, itself pinned to the reference's crop_image by tests/test_align_pad_cpu.py), Aligner(pad_edges=True)
reproduces the reference's padded crops (tests/golden/align_pad.npz), and --stream --align_padding keeps crops that equal the host recipe."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from reface_amd import ops
from reface_amd.align import Aligner, crop_plan, pad_image_host, pad_plan, pad_tables, quad_from_landmarks

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_align_cpu import seeded_frame  # noqa: E402
from test_align_pad_cpu import CASES, PADDED, case_window, pad_case  # noqa: E402

GUARD, POISON = 4096, 0xA5


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "align_pad.npz"))


def _guarded(nbytes, dtype):
    """A poisoned device buffer of `nbytes` between two poisoned guard bands -> (whole uint8 buffer, the view of the middle as `dtype`)."""
    whole = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes].view(dtype)


def _run_pad(frames, items, stages=15):
    """rf_align_pad_u8 on host frames uint8 [B, H, W, C] with poisoned, guarded scratch and outputs.  Returns the padded images (list of
    [h, w, 3]) and img1 (list of fp32 [h, w, 3]); asserts that the guards and every output byte outside the padded images are untouched."""
    desc, itab, dtab, wmax, hmax, _ = pad_tables(items)
    B = len(items)
    fr = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    d, it, dt = (torch.from_numpy(a).to(DEV) for a in (desc, itab, dtab))
    n = B * hmax * wmax * 3
    w_out, out = _guarded(n, torch.uint8)
    w_scr, scratch = _guarded(2 * n * 4, torch.float32)
    w_sel, select = _guarded(B * ops.PAD_SELECT_WORDS * 4, torch.int32)
    ops.align_pad_u8(fr, d, it, dt, scratch, select, out.view(B, hmax, wmax, 3), stages=stages)()
    torch.cuda.synchronize()
    for whole in (w_out, w_scr, w_sel):
        assert bool((whole[:GUARD] == POISON).all()) and bool((whole[-GUARD:] == POISON).all()), "a guard band was written"
    got = out.view(B, hmax, wmax, 3).cpu().numpy()
    img1 = scratch[n:].view(B, hmax * wmax, 3).cpu().numpy()
    images, planes = [], []
    for b in range(B):
        w, h = int(desc[b, 4]), int(desc[b, 5])
        rest = got[b].copy()
        rest[:h, :w] = POISON
        assert (rest == POISON).all(), (b, "bytes outside the padded image were written")
        images.append(got[b, :h, :w])
        planes.append(img1[b, :h * w].reshape(h, w, 3))
    return images, planes


def _check(frames, items, what):
    images, planes = _run_pad(frames, items)
    for b, ((ox, oy, W0, H0), pad, blur) in enumerate(items):
        parts = {}
        ref = pad_image_host(frames[b][oy:oy + H0, ox:ox + W0], pad, blur, parts=parts)
        n1 = int((planes[b].view(np.uint32) != parts["img1"].view(np.uint32)).sum())
        n2 = int((images[b] != ref).sum())
        print(f"{what}[{b}]: {ref.shape[1]}x{ref.shape[0]} px, pads {pad}, blur {blur:.3f}: img1 words differing {n1}, bytes differing {n2}")
        assert images[b].shape == ref.shape and n1 == 0 and n2 == 0, (what, b, n1, n2)
    return images


def test_pad_op_gives_the_fixture_paddings(G):
    """The five padded fixture windows in ONE launch sequence: each window (after its shrink) sits at its own offset in a frame of a common
    size, so five descriptors with different windows, pads, radii and padded sizes (all of even pixel count) share the batch."""
    H, W = 72, 130
    frames = np.random.default_rng(0).integers(0, 256, (len(PADDED), H, W, 3), dtype=np.uint8)
    items = []
    for b, name in enumerate(PADDED):
        win, _, pp, _ = case_window(G, name)
        oy, ox = 3 + b, 2 * b + 1
        frames[b, oy:oy + win.shape[0], ox:ox + win.shape[1]] = win
        items.append(((ox, oy, win.shape[1], win.shape[0]), pp.pad, pp.blur))
    images = _check(frames, items, "fixture")
    for b, name in enumerate(PADDED):
        assert np.array_equal(images[b], G[name + "_padded"]), name


@pytest.mark.parametrize("sigma", [20.0, 40.0])
@pytest.mark.parametrize("Cf", [3, 4])
def test_pad_op_wide_blur(sigma, Cf):
    """A 37 x 53 window padded by (40, 45, 50, 61) to 143 x 143 (an odd pixel count): radius 80 is wider than a wave, radius 160 larger
    than the padded image (scipy's fold runs more than once).  Cf = 4: the alpha channel, random here, is not read."""
    rng = np.random.default_rng(int(sigma) + Cf)
    frames = rng.integers(0, 256, (1, 50, 60, Cf), dtype=np.uint8)
    items = [((5, 9, 53, 37), (40, 45, 50, 61), sigma)]
    images = _check(frames, items, f"sigma {sigma:g} Cf {Cf}")
    assert images[0].shape == (143, 143, 3) and int(4 * sigma + 0.5) in (80, 160)


def test_pad_op_median_edge_cases():
    """All ties (a constant image: every value in one bin of every pass), a two-valued image of even count whose two middle values differ
    (the median is their mean, which no pixel holds), and odd and even counts in one batch."""
    H, W = 12, 14
    frames = np.zeros((3, H, W, 3), dtype=np.uint8)
    frames[0] = (200, 0, 255)
    frames[1, :, :7], frames[1, :, 7:] = 10, 250          # mirror-symmetric halves: as many low values as high ones
    frames[2] = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    items = [((0, 0, W, H), (3, 3, 3, 3), 0.3), ((0, 0, W, H), (4, 2, 4, 2), 0.3), ((1, 1, 11, 9), (2, 3, 2, 3), 1.5)]
    parts = {}
    pad_image_host(frames[1], items[1][1], items[1][2], parts=parts)
    v = np.sort(parts["img1"][..., 0], axis=None)
    assert v.size % 2 == 0 and v[v.size // 2 - 1] != v[v.size // 2] and parts["med"][0] == 130.0
    assert (11 + 4) * (9 + 6) % 2 == 1
    images = _check(frames, items, "median")
    assert (images[0] == (200, 0, 255)).all()


def _expected_crops(G, S, names):
    out = []
    for n in names:
        frame, quad, s = pad_case(G, n)
        assert s == S
        out.append((frame, quad, G[n + "_crop"]))
    return out


def test_aligner_pad_edges_reproduces_the_reference_crops(G):
    """The fixture's six cases.  An Aligner has ONE output size and the fixture's cases were made at three (the shrink and with it the
    window depend on it), so they run as three mixed calls: S = 32 (two padded frames of two sizes and `interior`, which does not
    trigger), S = 16 (`one_px`, and `shrunk` through the LANCZOS path first), S = 24 (`corner`).  Frames go in as device tensors."""
    by_size = {32: ("left_edge", "multi_reflect", "interior"), 16: ("one_px", "shrunk"), 24: ("corner",)}
    assert sorted(n for v in by_size.values() for n in v) == sorted(CASES)
    padded_names = []
    for S, names in by_size.items():
        al = Aligner(S, pad_edges=True)
        cases = _expected_crops(G, S, names)
        frames = [torch.from_numpy(f).to(DEV) for f, _, _ in cases]
        upload = al._upload
        al._upload = lambda arrays: upload(arrays) if all(torch.is_tensor(a) and a.is_cuda for a in arrays) else pytest.fail("a device frame went through the host")
        crops, _ = al.align(frames, quads=np.stack([q for _, q, _ in cases]))
        got = crops.cpu().numpy()
        for i, (n, (_, _, ref)) in enumerate(zip(names, cases)):
            assert np.array_equal(got[i], ref), (n, int((got[i] != ref).sum()))
        padded_names += [names[i] for i in al.padded]
        if "interior" in names:
            plain, _ = Aligner(S).align([cases[2][0]], quads=[cases[2][1]])
            assert torch.equal(plain[0], crops[2])
        if "shrunk" in names:
            f, q, _ = cases[1]
            assert crop_plan(q, (f.shape[1], f.shape[0]), S).shrink == 6
    assert sorted(padded_names) == sorted(PADDED)


def _host_crop(frame, quad, S):
    """crop_image(..., enable_padding=True) in PIL and the host recipe (the live oracle), and whether it padded."""
    p = crop_plan(quad, (frame.shape[1], frame.shape[0]), S)
    img = np.asarray(Image.fromarray(frame).resize(p.rsize, Image.LANCZOS)) if p.shrink > 1 else frame
    ox, oy, w, h = p.window
    win, pp = np.ascontiguousarray(img[oy:oy + h, ox:ox + w]), pad_plan(p, S)
    src, quad = (win, p.quad) if pp is None else (pad_image_host(win, pp.pad, pp.blur), pp.quad)
    return np.asarray(Image.fromarray(src).transform((S, S), Image.QUAD, (quad + 0.5).flatten(), Image.BILINEAR).convert("RGB")), pp is not None


def test_aligner_pad_edges_mixed_batch_and_scratch_cap(G):
    """All six fixture frames (five sizes, host arrays) and three more of one size in ONE align() call at S = 16, against the host recipe;
    then the same call under a scratch cap that holds one padded frame, so the three frames of one size are padded in three
    sub-batches: the same bytes."""
    S = 16
    frames, quads = [], []
    for n in CASES:
        f, q, _ = pad_case(G, n)
        frames.append(f)
        quads.append(q)
    for k in range(3):          # one size, the face over the right edge, three different paddings
        frames.append(seeded_frame(90, 120, 3, 400 + k))
        c, half = np.array([112.0 - 3 * k, 40.0 + 5 * k]), 15.0 + 2 * k          # (a side of 2 sqrt(2) half < 64: no shrink at S = 16)
        quads.append(np.array([c + (-half, -half), c + (-half, half), c + (half, half), c + (half, -half)]))
    refs = [_host_crop(f, q, S) for f, q in zip(frames, quads)]
    al = Aligner(S, pad_edges=True)
    crops, _ = al.align(frames, quads=np.stack(quads))
    got = crops.cpu().numpy()
    for i, (ref, was_padded) in enumerate(refs):
        assert np.array_equal(got[i], ref), (i, int((got[i] != ref).sum()))
        assert (i in al.padded) == was_padded
    assert al.padded == [0, 1, 2, 3, 4, 6, 7, 8]
    calls = []
    pad = al.pad
    al.pad = lambda fr, items: calls.append(len(items)) or pad(fr, items)
    al.pad_scratch_bytes = 1
    again, _ = al.align(frames, quads=np.stack(quads))
    assert torch.equal(again, crops) and sorted(calls) == [1] * 8
    sizes = [pad_plan(crop_plan(q, (120, 90), S), S).size for q in quads[6:]]
    calls.clear()
    al.pad_scratch_bytes = 2 * max(w for w, _ in sizes) * max(h for _, h in sizes) * 27          # two of the three fit
    again, _ = al.align(frames[6:], quads=np.stack(quads[6:]))
    assert torch.equal(again, crops[6:]) and calls == [2, 1]
    # without the keyword the same frames keep today's bytes, black wedge included
    plain, _ = Aligner(S).align(frames, quads=np.stack(quads))
    assert torch.equal(plain[5], crops[5]) and not torch.equal(plain[0], crops[0]) and bool((plain[0] == 0).all(-1).any())


SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4)


def test_cli_stream_align_padding(tmp_path):
    """--stream --align_padding --stream_keep on three frames whose face hangs over the left edge: the kept crops are the host recipe's
    (not the unpadded ones), the closing line counts them, and <video>_inv_transforms.npy is what a run without the flag writes (--align
    alone: it aligns, writes the transforms and stops at its stage-1 message before any model loads)."""
    from test_align_gpu import _landmarks_in
    rng = np.random.default_rng(12)
    W, H, N = 240, 160, 3
    frames = [rng.integers(0, 256, (H // 4, W // 4, 3), dtype=np.uint8).repeat(4, 0).repeat(4, 1) for _ in range(N)]
    lm = np.stack([_landmarks_in(W, H, 60 + i, centre=(14.0 + 6 * i, 70.0), eye=22.0, deg=5.0 * i) for i in range(N)])
    np.save(tmp_path / "lm.npy", lm)
    Image.fromarray(rng.integers(0, 256, (120, 110, 3), dtype=np.uint8)).save(tmp_path / "me.jpg")
    np.save(tmp_path / "src_lm.npy", _landmarks_in(110, 120, 70))
    for name in ("pad", "plain"):
        (tmp_path / name / "base" / "clip").mkdir(parents=True)
        for i, f in enumerate(frames):
            Image.fromarray(f).save(tmp_path / name / "base" / "clip" / f"{i}.png")

    def run(name, *flags):
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(tmp_path / name / "out"), "--Base_dir",
               str(tmp_path / name / "base"), "--target_video", "videos/clip.mp4", "--src_image", str(tmp_path / "me.jpg"), "--config",
               os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none", "--n_samples", "3", "--ddim_steps", "2", "--scale", "3.5",
               "--precision", "full", "--num_workers", "0", "--clip_vision_config", json.dumps(SMALL_CLIP), "--landmarks", str(tmp_path / "lm.npy"),
               "--src_landmarks", str(tmp_path / "src_lm.npy"), "--faceParsing_ckpt", "none", *flags]
        return subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    r = run("pad", "--stream", "--stream_keep", "--align_padding")
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "--align_padding padded the crops of 3 frames" in r.stdout
    for i in range(N):
        quad = quad_from_landmarks(lm[i])[3]
        ref, was_padded = _host_crop(frames[i], quad, 1024)
        got = np.asarray(Image.open(tmp_path / "pad" / "base" / "clipcropped_face" / f"{i}.png"))
        assert was_padded and np.array_equal(got, ref), (i, int((got != ref).sum()))
    r = run("plain", "--align")
    assert r.returncode != 0 and "mask_frames" in (r.stderr + r.stdout) and "align_padding=" not in r.stdout and "--align_padding" not in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    inv_a, inv_b = (np.load(tmp_path / n / "base" / "clip_inv_transforms.npy", allow_pickle=True) for n in ("pad", "plain"))
    assert inv_a.shape == (N, 8) and np.array_equal(inv_a, inv_b)
    unpadded = np.asarray(Image.open(tmp_path / "plain" / "base" / "clipcropped_face" / "0.png"))
    assert (unpadded == 0).all(-1).mean() > 0.02          # the black wedge the flag removes
    shutil.rmtree(tmp_path / "pad" / "out")
