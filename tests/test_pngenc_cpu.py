"""The restatement of the GPU PNG encoder (tests/pngenc_refs.py) held to zlib and PIL: the streams it writes inflate to the filtered bytes,
un-filter to the pixels, open in PIL with the right mode, and stay within the size bound against zlib's Z_RLE on the same bytes."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngenc_refs as R  # noqa: E402


def _zlib_rle(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(bytes(data)) + c.flush()


def _mask(H=512, W=512):
    m = np.zeros((H, W, 1), dtype=np.uint8)
    m[H // 5:H // 2, W // 3:3 * W // 4] = 255
    return m


def _images():
    rng = np.random.RandomState(0)
    out = {"photo%d" % k: R.photo_like(512, 512, 3, seed=k) for k in range(4)}          # smooth field + noise: photograph-like residuals
    out["noise"] = rng.randint(0, 256, size=(96, 131, 3)).astype(np.uint8)
    out["zeros"] = np.zeros((200, 333, 4), dtype=np.uint8)
    out["mask"] = _mask()
    out["rgba"] = np.concatenate([R.photo_like(64, 171, 3, seed=9), np.full((64, 171, 1), 255, np.uint8)], axis=2)
    out["one"] = np.array([[[77]]], dtype=np.uint8)
    return out


IMAGES = _images()
STREAMS = {
    "two_bytes": b"\x05\x05",
    "fibonacci": R.fibonacci_stream(),
    "runs": R.runs_stream(),
    "noise": np.random.RandomState(1).randint(0, 256, size=R.SEG + 17).astype(np.uint8).tobytes(),
    "zeros": bytes(2 * R.SEG + 3),
    "straddle": bytes([1]) * (R.SEG - 2) + bytes([9]) * 5 + bytes(range(40)),
}


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_restatement_roundtrip_and_size(name):
    img = IMAGES[name]
    H, W, C = img.shape
    filt, types = R.filter_image(img)
    assert filt.size == H * (1 + W * C) and set(types.tolist()) <= {0, 1, 2, 3, 4}
    z = R.zlib_stream(filt.tobytes())
    assert zlib.decompress(z) == filt.tobytes()                      # zlib checks the Adler-32
    if H * W * C <= 64 * 171 * 4:
        assert np.array_equal(R.unfilter(filt, H, W, C), img)
    from PIL import Image
    im = Image.open(io.BytesIO(R.wrap_png(z, H, W, C)))               # PIL checks the chunk CRCs
    assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[C]
    got = np.asarray(im)
    assert np.array_equal(got.reshape(H, W, C), img)
    nseg = -(-filt.size // R.SEG)
    ref = len(_zlib_rle(filt.tobytes()))
    print(f"{name}: {len(z)} bytes, zlib Z_RLE {ref} ({len(z) / ref:.4f}x), level 1 {len(zlib.compress(filt.tobytes(), 1))}, {nseg} segments")
    assert len(z) <= 1.01 * ref + 200 * nseg


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_restatement_streams(name):
    data = STREAMS[name]
    z = R.zlib_stream(data)
    assert zlib.decompress(z) == data
    nseg = -(-len(data) // R.SEG)
    ref = len(_zlib_rle(data))
    print(f"{name}: {len(z)} bytes, zlib Z_RLE {ref}, {nseg} segments")
    assert len(z) <= 1.01 * ref + 200 * nseg


def test_depth_limit_and_stored_paths_are_taken():
    """The inputs above do reach the two special paths: the Fibonacci counts need the 15-bit loop, noise falls back to a stored block."""
    d, lit, head, mlen = R.tokenise(R.fibonacci_stream())
    counts = np.bincount(d[lit], minlength=286) + np.bincount(257 + R._LEN_SYM[mlen][head], minlength=286)
    counts[256] = 1
    lens = R.huffman_lengths(counts)
    assert max(lens) <= 15 and max(R.huffman_lengths(counts, limit=99)) > 15          # the unlimited code is deeper: the loop ran
    # Kraft sum of a complete code
    assert sum(2.0 ** -l for l in lens if l) == 1.0
    seg = STREAMS["noise"][:R.SEG]
    out = R.deflate_segment(seg, last=False)
    assert len(out) == R.SEG + 5 and out[0] == 0 and out[5:] == seg


def test_token_roles():
    """Runs of R equal bytes: a literal, then matches of 258 while >= 3 remain, then 1 or 2 literals."""
    for Rn, want in [(1, [1]), (2, [1, 1]), (3, [1, 1, 1]), (4, [1, 3]), (259, [1, 258]), (260, [1, 258, 1]), (261, [1, 258, 1, 1]), (262, [1, 258, 3]),
                     (517, [1, 258, 258]), (518, [1, 258, 258, 1])]:
        d, lit, head, mlen = R.tokenise(bytes([9]) + bytes([4]) * Rn + bytes([8]))
        toks = [1 if lit[i] else int(mlen[i]) for i in range(1, 1 + Rn) if lit[i] or head[i]]
        assert toks == want, (Rn, toks)


def test_png_encoder_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from reface_amd import _lib
    from reface_amd.pngenc import PngEncoder
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        PngEncoder("cpu").encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


def test_cli_swap_video_gpu_png_needs_pasted_frames(tmp_path):
    """--gpu_png without --paste_back / --stream has nothing to encode: refused before anything is loaded (no GPU needed)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "inference_swap_video.py"), "--outdir", str(tmp_path / "out"), "--Base_dir",
                        str(tmp_path / "base"), "--gpu_png"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode != 0 and "--gpu_png encodes the pasted frames" in (r.stdout + r.stderr)
