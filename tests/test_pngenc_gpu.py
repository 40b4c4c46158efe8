"""The GPU PNG encoder (reface_amd/csrc/pngenc.hip, reface_amd/pngenc.py) against its numpy / Python restatement (tests/pngenc_refs.py,
itself held to zlib and PIL by tests/test_pngenc_cpu.py): byte for byte per stage, decoded by zlib and PIL, and through the CLIs' --gpu_png."""
import io
import json
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngenc_refs as R  # noqa: E402
from reface_amd import pngenc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4)
SEG = R.SEG


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _deflate(streams):
    """list of equal-length byte strings -> the device's zlib streams"""
    a = np.stack([np.frombuffer(s, dtype=np.uint8) for s in streams])
    return pngenc.deflate_streams(_dev(a))


def _rng_bytes(n, seed, hi=256):
    return np.random.RandomState(seed).randint(0, hi, size=n).astype(np.uint8).tobytes()


def _straddle(k):
    """a run that starts k bytes before a segment boundary and runs 300 bytes past it, inside short-run content"""
    head = _rng_bytes(SEG - k, 11, hi=4)
    head = head[:-1] + bytes([200])          # the byte before the run differs from it
    return head + bytes([9]) * (k + 300) + _rng_bytes(500, 12, hi=4)


STREAMS = {
    "len1": b"\x2a",
    "len2": b"\x05\x05",
    "len32767": _rng_bytes(32767, 1, hi=6),
    "len32768": _rng_bytes(32768, 2, hi=6),
    "len32769": _rng_bytes(32769, 3, hi=6),
    "len65539": _rng_bytes(65536 + 3, 4, hi=6),
    "noise": _rng_bytes(SEG + 17, 5),                  # stored fallback
    "zeros": bytes(2 * SEG + 3),
    "ones": b"\xff" * (SEG + 100),
    "runs": R.runs_stream(),
    "straddle1": _straddle(1),
    "straddle2": _straddle(2),
    "straddle3": _straddle(3),
    "fibonacci": R.fibonacci_stream(),                 # the 15-bit limit loop
    "single_value": bytes([77]) * 5000,
    "gradient": (np.arange(3 * SEG) // 7 % 256).astype(np.uint8).tobytes(),
}


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_deflate_streams(name):
    data = STREAMS[name]
    got = _deflate([data])[0]
    assert zlib.decompress(got) == data
    want = R.zlib_stream(data)
    assert got == want, (len(got), len(want), next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if got[:len(want)] != want[:len(got)] else -1)


def test_deflate_batch_and_strided_rows():
    n = SEG + 1234
    streams = [_rng_bytes(n, 21, hi=3), bytes(n), _rng_bytes(n, 22)]          # coded, flat and stored segments in one launch
    got = _deflate(streams)
    for g, s in zip(got, streams):
        assert zlib.decompress(g) == s and g == R.zlib_stream(s)
    # rows of a wider buffer, at an odd byte offset (the kernel's unaligned load path)
    wide = np.zeros((3, n + 37), dtype=np.uint8)
    for k, s in enumerate(streams):
        wide[k, 5:5 + n] = np.frombuffer(s, dtype=np.uint8)
    got2 = pngenc.deflate_streams(_dev(wide)[:, 5:5 + n])
    assert got2 == got
    assert pngenc.deflate_streams(_dev(wide)[:, 5:5 + n]) == got          # two encodes give equal bytes


# ------------------------------------------------------------------------------------------------ filter
def _five_filter_image():
    """[10, 40, 3]: row pairs built so that each of None, Sub, Up, Average, Paeth wins at least one row."""
    rng = np.random.RandomState(3)
    H, W, C = 10, 40, 3
    img = np.zeros((H, W, C), dtype=np.int64)
    img[0] = rng.randint(0, 4, size=(W, C)) - 2                       # small values around 0: None
    img[1] = np.cumsum(rng.randint(5, 9, size=(W, C)), axis=0) + 7 * rng.randint(0, 30, size=(1, C))          # a ramp, unrelated to row 0: Sub
    img[2] = rng.randint(0, 256, size=(W, C))
    img[3] = img[2]                                                   # a copy of the row above: Up
    img[4] = rng.randint(0, 256, size=(W, C))
    a = np.zeros((W, C), dtype=np.int64)
    for x in range(W):                                                # each pixel the average of left and up (+ a little): Average
        left = a[x - 1] if x else 0
        a[x] = ((left + img[4][x]) >> 1) + rng.randint(0, 2, size=C)
    img[5] = a
    f = np.where((np.arange(W) // 6) % 2 == 0, 20, 120)                 # f(x) + g(y): left + up - upleft is exact, so Paeth pays min(|df|, |dg|)
    img[6:10] = f[None, :, None] + 30 * np.arange(4)[:, None, None]     # per pixel where Sub pays |df| = 100 at every step and Up |dg| = 30 everywhere
    return (img & 255).astype(np.uint8)


def _filter_dev(img_t):
    return pngenc.filter_images(img_t).cpu().numpy()


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 3), (7, 13, 4), (64, 171, 3)])
def test_filter_shapes(shape):
    H, W, C = shape
    rng = np.random.RandomState(H * W)
    imgs = np.stack([R.photo_like(H, W, C, seed=1), rng.randint(0, 256, size=shape).astype(np.uint8)])
    got = _filter_dev(_dev(imgs))
    for b in range(2):
        want, _ = R.filter_image(imgs[b])
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))


def test_filter_strided_every_filter_and_ties():
    img = _five_filter_image()
    want, types = R.filter_image(img)
    assert set(types.tolist()) == {0, 1, 2, 3, 4}, types                # every filter wins a row
    H, W, C = img.shape
    big = np.zeros((2, H + 3, W + 9, C), dtype=np.uint8)                 # a row- and image-strided view
    big[0, 1:1 + H, 4:4 + W] = img
    big[1, 1:1 + H, 4:4 + W] = img[::-1]
    got = _filter_dev(_dev(big)[:, 1:1 + H, 4:4 + W])
    assert np.array_equal(got[0], want)
    assert np.array_equal(got[1], R.filter_image(img[::-1])[0])
    # tied sums: a constant row above a constant row (Up, Average-of-equal and Paeth all give zeros after the first pixel; Sub ties with them
    # on a first row of zeros) -- the lowest type must win
    flat = np.zeros((3, 9, 3), dtype=np.uint8)
    flat[1:] = 50
    wt, tt = R.filter_image(flat)
    assert tt.tolist() == [0, 1, 2]                                       # None on zeros; Sub (50 once per channel) beats Up (50 everywhere); Up ties with Paeth
    assert np.array_equal(_filter_dev(_dev(flat[None]))[0], wt)


# ------------------------------------------------------------------------------------------------ whole files
def _file_images(shape, B):
    H, W, C = shape
    imgs = []
    for b in range(B):
        im = R.photo_like(H, W, C, seed=b + 1)
        if b % 3 == 1:
            im[H // 3:, W // 4:] = 255 if C != 4 else np.array([0, 0, 0, 255], dtype=np.uint8)          # a flat region: long runs, matches
        if b % 3 == 2:
            im[:H // 2] = np.random.RandomState(b).randint(0, 256, size=im[:H // 2].shape)             # noise: stored segments
        imgs.append(im)
    return np.stack(imgs)


@pytest.mark.parametrize("shape,B", [((1, 1, 1), 1), ((7, 13, 4), 2), ((64, 171, 3), 2), ((33, 1000, 4), 1), ((270, 480, 4), 1), ((512, 512, 3), 3)])
def test_whole_files(shape, B):
    H, W, C = shape
    imgs = _file_images(shape, B)
    enc = pngenc.PngEncoder(DEV)
    x = _dev(imgs)
    files = enc.encode(x)
    assert len(files) == B
    for b in range(B):
        im = Image.open(io.BytesIO(files[b]))
        assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[C] and im.size == (W, H)
        assert np.array_equal(np.array(im).reshape(H, W, C), imgs[b])
        assert files[b] == R.encode_png(imgs[b]), b
    assert enc.encode(x) == files                                        # two encodes (the second on reused scratch) give equal bytes
    jobs = [enc.encode_async(x), enc.encode_async(x[:, :, :, :1] if C > 1 else x)]          # two encodes in flight; a channel-strided view is made contiguous
    assert jobs[0].result() == files
    grey = jobs[1].result()
    assert np.array_equal(np.array(Image.open(io.BytesIO(grey[0]))), imgs[0][:, :, 0])


# ------------------------------------------------------------------------------------------------ CLIs
def _run(cmd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    if ok:
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return r


def _same_tree(a, b, mode=None):
    n = 0
    for sub in sorted(os.listdir(a)):
        if not os.path.isdir(os.path.join(a, sub)):
            continue
        fa, fb = sorted(os.listdir(os.path.join(a, sub))), sorted(os.listdir(os.path.join(b, sub)))
        assert fa == fb, (sub, fa, fb)
        for f in fa:
            if not f.endswith(".png"):
                continue
            ia, ib = Image.open(os.path.join(a, sub, f)), Image.open(os.path.join(b, sub, f))
            assert ia.mode == ib.mode and np.array_equal(np.asarray(ia), np.asarray(ib)), (sub, f)
            n += 1
    return n


def test_cli_test_bench_gpu_png(tmp_path):
    base = [sys.executable, os.path.join(ROOT, "scripts", "inference_test_bench.py"), "--config", os.path.join(ROOT, "tests", "configs", "reface_small.yaml"),
            "--ckpt", "none", "--dataset", "synthetic", "--n_items", "3", "--n_samples", "2", "--ddim_steps", "4", "--scale", "3.5", "--H", "256", "--W", "256",
            "--clip_vision_config", json.dumps(SMALL_CLIP)]
    _run(base + ["--outdir", str(tmp_path / "host")])
    _run(base + ["--outdir", str(tmp_path / "gpu"), "--gpu_png"])
    assert _same_tree(tmp_path / "host", tmp_path / "gpu") == 3 * 6
    # the device files are this encoder's: one IDAT whose stream starts 78 01
    raw = open(tmp_path / "gpu" / "results" / "000000000000.png", "rb").read()
    assert raw[37:41] == b"IDAT" and raw[41:43] == b"\x78\x01"
    r = _run(base + ["--outdir", str(tmp_path / "bad"), "--gpu_png", "--png_level", "1"], ok=False)
    assert r.returncode != 0 and "--gpu_png cannot be combined with --png_level" in (r.stdout + r.stderr)


def test_cli_swap_video_paste_back_gpu_png(tmp_path):
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
        q = np.array([[40.0, 30.0], [40.0, 170.0], [180.0, 170.0], [180.0, 30.0]]) + 20 * i
        coeffs.append(alignment_coefficients(q, 1024))
    np.save(base / "clip_inv_transforms.npy", coeffs)

    def run(out, *extra):
        (out / "temp_results").mkdir(parents=True)
        shutil.copy(base / "source_cropped" / "0.png", out / "temp_results" / "me.png")
        shutil.copy(base / "source_mask" / "0.png", out / "temp_results" / "me.jpg")
        _run([sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(out), "--Base_dir", str(base), "--target_video",
              "videos/clip.mp4", "--src_image", "faces/me.jpg", "--config", os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none",
              "--n_samples", "2", "--ddim_steps", "4", "--scale", "3.5", "--precision", "full", "--num_workers", "0", "--clip_vision_config",
              json.dumps(SMALL_CLIP), "--paste_back", *extra])

    run(tmp_path / "host")
    run(tmp_path / "gpu", "--gpu_png")
    fa, fb = sorted(os.listdir(tmp_path / "host" / "results")), sorted(os.listdir(tmp_path / "gpu" / "results"))
    assert fa == fb and len(fa) == 2
    for f in fa:
        ia, ib = Image.open(tmp_path / "host" / "results" / f), Image.open(tmp_path / "gpu" / "results" / f)
        assert ib.mode == "RGBA" and ia.mode == "RGBA" and np.array_equal(np.asarray(ia), np.asarray(ib)), f
        assert open(tmp_path / "gpu" / "results" / f, "rb").read()[41:43] == b"\x78\x01"


def test_cli_swap_video_stream_gpu_png(tmp_path):
    """--stream --gpu_png: the pasted frames are encoded from the device tensors; same files and pixels as the host writer's."""
    import test_stream_gpu as S
    S._make_inputs(tmp_path, 4, rgba=(1,), seed=12)
    for name in ("host", "gpu"):
        S._copy_inputs(tmp_path, tmp_path / name / "base")
    S._run(tmp_path, tmp_path / "host" / "base", tmp_path / "host" / "out", "--stream")
    out = S._run(tmp_path, tmp_path / "gpu" / "base", tmp_path / "gpu" / "out", "--stream", "--gpu_png")
    assert "4 pasted frames" in out
    names = [f"{i:012d}.png" for i in range(4)]
    S._same_dir(tmp_path / "host" / "out" / "results", tmp_path / "gpu" / "out" / "results", names)
    for n in names:
        assert Image.open(tmp_path / "gpu" / "out" / "results" / n).mode == "RGBA"
        assert open(tmp_path / "gpu" / "out" / "results" / n, "rb").read()[41:43] == b"\x78\x01"
    r = S._run(tmp_path, tmp_path / "gpu" / "base", tmp_path / "gpu" / "out2", "--stream", "--gpu_png", "--skip_save")
    assert os.listdir(tmp_path / "gpu" / "out2" / "results") == []


def test_cli_swap_selected_gpu_png(tmp_path):
    """inference_swap_selected.py --gpu_png: the per-source folders results/<s>/, grid/<s>/ and <s>/ hold the same files as the default run,
    every one decoding to the same pixels."""
    from test_host_cpu import _prepared_swap_tree
    base = str(tmp_path / "base")
    _prepared_swap_tree(base, n_tar=3, n_src=2)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_swap_selected.py"), "--Base_dir", base, "--config",
           os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none", "--n_samples", "2", "--ddim_steps", "4", "--scale", "3.5",
           "--H", "512", "--W", "512", "--precision", "full", "--num_workers", "0", "--clip_vision_config", json.dumps(SMALL_CLIP)]
    host, gpu = tmp_path / "host", tmp_path / "gpu"
    _run(cmd + ["--outdir", str(host)])
    _run(cmd + ["--outdir", str(gpu), "--gpu_png"])
    n = 0
    for s in ("0", "1"):
        for sub, count in ((os.path.join("results", s), 3), (os.path.join("grid", s), 3), (s, 12)):
            fa, fb = sorted(os.listdir(host / sub)), sorted(os.listdir(gpu / sub))
            assert fa == fb and len(fa) == count, (sub, fa, fb)
            for f in fa:
                ia, ib = Image.open(host / sub / f), Image.open(gpu / sub / f)
                assert ia.mode == ib.mode == "RGB" and np.array_equal(np.asarray(ia), np.asarray(ib)), (sub, f)
                assert open(gpu / sub / f, "rb").read()[41:43] == b"\x78\x01", (sub, f)          # this encoder's stream, not PIL's
                n += 1
    assert n == 2 * 18

