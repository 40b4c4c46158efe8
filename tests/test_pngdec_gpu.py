"""The GPU PNG decoder (reface_amd/csrc/pngdec.hip, reface_amd/pngdec.py): rf_png_inflate against zlib on the corpus that the sanitized host
program has passed (tests/test_pngdec_cpu.py), rf_png_unfilter_u8 against tests/pngenc_refs.py, whole files against PIL.  Every comparison
is equality of uint8 arrays, and where a file or a stream is decoded -- device or host, segmented or serial plan -- is asserted by name."""
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
import pngdec_inputs as I  # noqa: E402
import pngenc_refs as R  # noqa: E402
from reface_amd import pngdec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEG = R.SEG


@pytest.fixture(scope="module")
def dec():
    return pngdec.PngDecoder(DEV)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ inflate alone
@pytest.mark.parametrize("name", sorted(I.good_streams()))
def test_inflate_good_stream(dec, name):
    z, raw, plan = I.good_streams()[name]
    outs, report = dec.inflate([z], [len(raw)])
    assert report[0]["plan"] == plan and report[0]["code"] == 0
    assert _np(outs[0]).tobytes() == raw


def test_inflate_mixed_launch(dec):
    """streams of different lengths and both plans in one launch"""
    g = I.good_streams()
    names = sorted(g)
    outs, report = dec.inflate([g[n][0] for n in names], [len(g[n][1]) for n in names])
    for n, o, r in zip(names, outs, report):
        assert r["plan"] == g[n][2], n
        assert _np(o).tobytes() == g[n][1], n
    assert {r["plan"] for r in report} == {"segments", "serial"}


@pytest.mark.parametrize("misalign", [1, 3, 7])
def test_inflate_odd_offset(dec, misalign):
    g = I.good_streams()
    names = ["zlib6_text", "enc_seg3plus5", "enc_noise3", "dist32768", "zlib0_photo"]
    outs, report = dec.inflate([g[n][0] for n in names], [len(g[n][1]) for n in names], misalign=misalign)
    for n, o, r in zip(names, outs, report):
        assert r["plan"] == g[n][2] and _np(o).tobytes() == g[n][1], n


# ------------------------------------------------------------------------------------------------ unfilter alone
def _filtered(img, types):
    """the filtered stream of img [H, W, C] with the filter type of every row given"""
    H, W, C = img.shape
    rows = img.reshape(H, W * C)
    zero = np.zeros(W * C, dtype=np.uint8)
    out = np.empty((H, 1 + W * C), dtype=np.uint8)
    for y in range(H):
        out[y, 0] = types[y]
        out[y, 1:] = R.filter_candidates(rows[y], rows[y - 1] if y else zero, C)[types[y]]
    return out.reshape(-1).tobytes()


UNFILTER_SHAPES = [(1, 1), (5, 7), (64, 64), (130, 67)]


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", UNFILTER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unfilter(dec, shape, bpp):
    H, W = shape
    rng = np.random.RandomState(100 * H + W + bpp)
    img = rng.randint(0, 256, size=(H, W, bpp)).astype(np.uint8)
    choices = [rng.randint(0, 5, size=H)] + [np.full(H, t) for t in range(5)]          # seeded random, and each type for a whole image
    streams = [_filtered(img, t) for t in choices]
    assert np.array_equal(R.unfilter(np.frombuffer(streams[0], dtype=np.uint8), H, W, bpp), img)          # the reference undoes what the test built
    outs = dec.unfilter(streams, [(H, W, bpp)] * len(streams))
    for t, o in zip(choices, outs):
        assert o.shape == (H, W, bpp) and np.array_equal(_np(o), img), t[:8]


def test_unfilter_arbitrary_residuals_and_strided_batch(dec):
    """residual bytes that no encoder chose (every row random, all five types), written into a strided view of a wider batch tensor"""
    H, W, bpp, B = 70, 33, 3, 3
    rng = np.random.RandomState(9)
    streams, wants = [], []
    for b in range(B):
        s = rng.randint(0, 256, size=(H, 1 + W * bpp)).astype(np.uint8)
        s[:, 0] = rng.randint(0, 5, size=H)
        s[0, 0] = 4 - b          # Paeth, Average and Up on a first row
        streams.append(s.reshape(-1).tobytes())
        wants.append(R.unfilter(s.reshape(-1), H, W, bpp))
    wide = torch.full((B, H + 3, W + 5, bpp), 77, dtype=torch.uint8, device=DEV)
    outs = dec.unfilter(streams, [(H, W, bpp)] * B, out=wide)
    got = _np(wide)
    for b in range(B):
        assert np.array_equal(got[b, :H, :W], wants[b]) and np.array_equal(_np(outs[b]), wants[b])
    assert (got[:, H:] == 77).all() and (got[:, :, W:] == 77).all()          # nothing outside the view is touched


def test_unfilter_bad_filter_byte(dec):
    s = bytearray(_filtered(np.zeros((4, 4, 3), dtype=np.uint8), [0, 1, 2, 3]))
    s[2 * 13] = 5
    with pytest.raises(pngdec.PngDecodeError) as e:
        dec.unfilter([bytes(s)], [(4, 4, 3)])
    assert e.value.code == 11


# ------------------------------------------------------------------------------------------------ whole files
def _pil_png(arr, level):
    buf = io.BytesIO()
    Image.fromarray(arr.squeeze() if arr.shape[2] == 1 else arr).save(buf, format="PNG", compress_level=level)
    return buf.getvalue()


def _content(mode_c, kind):
    if kind == "noise":
        return np.random.RandomState(mode_c).randint(0, 256, size=(300, 300, mode_c)).astype(np.uint8)          # IDAT is split at 64 KiB
    return R.photo_like(97, 131, mode_c, seed=mode_c)


@pytest.fixture(scope="module")
def pil_files():
    """(name, file bytes) of PIL-written files: modes L, LA, RGB, RGBA at levels 1 and 6, noise and smooth content"""
    out = []
    for c in (1, 2, 3, 4):
        for level in (1, 6):
            for kind in ("noise", "photo"):
                out.append((f"{'L LA RGB RGBA'.split()[c - 1]}_l{level}_{kind}", _pil_png(_content(c, kind), level)))
    return out


def _pil(data, mode=None):
    im = Image.open(io.BytesIO(data))
    if mode:
        im = im.convert(mode)
    a = np.asarray(im)
    return a.reshape(a.shape[0], a.shape[1], -1)


@pytest.mark.parametrize("mode", [None, "RGB", "L"])
def test_pil_files_equal_pil(dec, pil_files, mode):
    datas = [d for _, d in pil_files]
    assert pngdec.parse_png(pil_files[4][1]).n_idat > 1
    job = dec.decode_async(datas, mode)
    outs = job.result()
    for (name, data), o, r in zip(pil_files, outs, job.report):
        on_device = not (mode == "L" and name.startswith("RGB"))          # RGB -> L is PIL's luma: documented as a host combination
        assert r["where"] == ("gpu" if on_device else "host"), (name, r)
        if on_device:
            assert r["plan"] == "serial", (name, r)
        assert o.is_cuda and o.dtype == torch.uint8 and np.array_equal(_np(o), _pil(data, mode)), (name, mode)


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 3), (97, 131, 4), (200, 256, 3), (130, 300, 1)], ids=str)
def test_encoder_files_equal_pil(dec, shape):
    """files of the GPU encoder's format (tests/pngenc_refs.py states its bytes): the segmented plan wherever there is more than one segment"""
    H, W, C = shape
    img = R.photo_like(H, W, C, seed=H)
    if H > 100:
        img[H // 2:] = np.random.RandomState(H).randint(0, 256, size=img[H // 2:].shape)          # noise: stored segments
    data = R.encode_png(img)
    job = dec.decode_async([data])
    out = job.result()[0]
    assert job.report[0]["where"] == "gpu"
    assert job.report[0]["plan"] == ("segments" if H * (1 + W * C) > SEG else "serial")
    assert np.array_equal(_np(out), _pil(data)) and np.array_equal(_np(out), img)


def test_widest_image_on_the_device(dec):
    """W = MAX_WIDTH: the unfilter's largest row buffer; one pixel more goes to the host.  Both equal PIL."""
    W = pngdec.MAX_WIDTH
    for w, where in ((W, "gpu"), (W + 1, "host")):
        data = _pil_png(np.random.RandomState(w).randint(0, 256, size=(3, w, 4)).astype(np.uint8), 1)
        job = dec.decode_async([data])
        out = job.result()[0]
        assert job.report[0]["where"] == where and np.array_equal(_np(out), _pil(data)), w


def test_gpu_encoder_round_trip(dec):
    from reface_amd import pngenc
    imgs = torch.from_numpy(np.stack([R.photo_like(120, 160, 3, seed=s) for s in range(3)])).to(DEV)
    files = pngenc.PngEncoder(DEV).encode(imgs)
    job = dec.decode_async(files, "RGB")
    outs = job.result()
    assert all(r["where"] == "gpu" and r["plan"] == "segments" for r in job.report)
    assert job.batch is not None and torch.equal(job.batch, imgs) and all(torch.equal(o, i) for o, i in zip(outs, imgs))


def test_paths_mixed_sizes_and_host_files(dec, tmp_path):
    """paths as items; a palette file, a 16-bit file and a JPEG go to the host and still equal PIL"""
    rgb = R.photo_like(40, 50, 3, seed=1)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    Image.fromarray(rgb).quantize(16).save(tmp_path / "palette.png")
    Image.fromarray((np.arange(30 * 20, dtype=np.uint16) * 100).reshape(30, 20)).save(tmp_path / "sixteen.png")
    Image.fromarray(rgb).save(tmp_path / "photo.jpg")
    Image.fromarray(R.photo_like(33, 21, 4, seed=2)).save(tmp_path / "rgba.png")
    names = ["rgb.png", "palette.png", "sixteen.png", "photo.jpg", "rgba.png"]
    paths = [str(tmp_path / n) for n in names]
    job = dec.decode_async(paths, "RGB")
    outs = job.result()
    assert [r["where"] for r in job.report] == ["gpu", "host", "host", "host", "gpu"]
    for p, o in zip(paths, outs):
        assert np.array_equal(_np(o), np.asarray(Image.open(p).convert("RGB"))), p
    o = dec.decode([paths[2]])[0]          # without a mode a 16-bit file is PIL's own array
    assert np.array_equal(_np(o).reshape(30, 20), np.asarray(Image.open(paths[2])))
    with pytest.raises(Exception) as e:
        dec.decode([b"not an image at all"])
    assert type(e.value).__name__ == "UnidentifiedImageError"          # PIL's own exception


# ------------------------------------------------------------------------------------------------ damaged streams
def test_damaged_streams_leave_codes(dec):
    """The corpus the sanitized host program has passed, in one launch: every stream must leave a non-zero code, the good one between them
    its bytes."""
    d = I.damaged_streams()
    z, raw, _ = I.good_streams()["zlib6_text"]
    entries = [(n, d[n][0], d[n][1]) for n in sorted(d)]
    entries.insert(len(entries) // 2, ("good", z, len(raw)))
    outs, report = dec.inflate([e[1] for e in entries], [e[2] for e in entries], check=False)
    by = {}
    for (name, _, _), o, r in zip(entries, outs, report):
        by[name] = r["code"]
        if name == "good":
            assert r["code"] == 0 and _np(o).tobytes() == raw
        else:
            assert r["code"] != 0 and r["plan"] == "serial", (name, r)
    assert (by["bad_adler"], by["len_nlen_mismatch"], by["oversubscribed"], by["distance_before_start"], by["output_longer"], by["output_shorter"]) == (10, 4, 5, 7, 8, 9)
    assert by["empty"] == 1 and by["block_type_3"] == 3 and by["bad_zlib_header"] == 2


def _wrap(z, H, W, C):
    return R.wrap_png(z, H, W, C)


def test_damaged_file_raises_naming_the_file(dec, tmp_path):
    img = R.photo_like(60, 70, 3, seed=3)
    z = zlib.compress(R.filter_image(img)[0].tobytes(), 6)
    good = tmp_path / "good.png"
    good.write_bytes(_wrap(z, 60, 70, 3))
    for name, bad in (("adler.png", z[:-1] + bytes([z[-1] ^ 1])), ("cut.png", z[:len(z) // 2]), ("short.png", zlib.compress(bytes(100)))):
        p = tmp_path / name
        p.write_bytes(_wrap(bad, 60, 70, 3))
        with pytest.raises(pngdec.PngDecodeError) as e:
            dec.decode([str(good), str(p)])
        assert name in str(e.value) and e.value.name == str(p) and e.value.code in (10, 1, 9)
    assert np.array_equal(_np(dec.decode([str(good)])[0]), img)          # the decoder is usable after a refusal


# ------------------------------------------------------------------------------------------------ callers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMING_KEYS = {"seconds", "images_per_s"}


def _cli(rel):
    import importlib.util
    spec = importlib.util.spec_from_file_location("pngdec_cli_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _twice(cli, argv, tmp_path, capsys):
    """The command with and without --gpu_png_decode, in this process and without loader workers (a test process that has the GPU open
    starts no further processes): (--json values, printed lines) of both, timing keys left out.  The flagged run must say, on stderr, that
    the fixture's files went through the device."""
    import re
    got = []
    for k, flag in enumerate(([], ["--gpu_png_decode"])):
        out_json = str(tmp_path / f"out{k}.json")
        capsys.readouterr()
        cli.main(argv + ["--num-workers", "0", "--json", out_json] + flag)
        cap = capsys.readouterr()
        r = json.load(open(out_json))
        got.append(({k: v for k, v in r.items() if k not in TIMING_KEYS}, cap.out.splitlines()))
        m = re.search(r"gpu_png_decode: (\d+) files decoded on the device, (\d+) on the host", cap.err)
        assert (m is not None) == bool(flag), cap.err[-500:]
    assert int(m.group(1)) >= r["images"] // 2 and int(m.group(2)) == 0, m.group(0)
    return got


def test_cli_pose_gpu_png_decode(tmp_path, capsys):
    import pose_inputs as PI
    paths = PI.write_folders(str(tmp_path / "folders"), PI.build())
    a, b = _twice(_cli("eval_tool/Pose/pose_compare.py"), ["--device", "cuda"] + paths + ["--hopenet_ckpt", "none", "--batch-size", "4"], tmp_path, capsys)
    assert a == b and "pose_value" in a[0]


def test_cli_expression_gpu_png_decode(tmp_path, capsys):
    import expr_inputs as EI
    paths = EI.write_folders(str(tmp_path / "folders"), EI.build())
    a, b = _twice(_cli("eval_tool/Expression/expression_compare_face_recon.py"),
                  ["--device", "cuda"] + paths + ["--recon_ckpt", "none", "--batch-size", "4", "--print_sim", "True"], tmp_path, capsys)
    assert a == b and "expression_value" in a[0]


def test_cli_id_retrieval_gpu_png_decode(tmp_path, capsys):
    import idscore_inputs as II
    paths = II.write_folders(str(tmp_path / "folders"), II.build())
    a, b = _twice(_cli("eval_tool/ID_retrieval/ID_retrieval.py"), ["--device", "cuda"] + paths + [
        "--dataset", II.DATASET, "--print_sim", "True", "--arcface", "True", "--arcface_ckpt", "none", "--batch-size", "5"], tmp_path, capsys)
    assert a == b and "top1" in a[0]


def test_cli_fid_gpu_png_decode(tmp_path, capsys):
    import fid_inputs as FI
    paths = FI.write_folders(str(tmp_path / "folders"), FI.build())
    a, b = _twice(_cli("eval_tool/fid/fid_score.py"), ["--device", "cuda"] + paths + ["--clip_ckpt", "none", "--batch-size", "20"], tmp_path, capsys)
    assert a == b and "fid" in a[0]


def test_cli_lpips_gpu_png_decode(tmp_path, capsys):
    import lpips_inputs as LI
    paths = LI.write_folders(str(tmp_path / "folders"), LI.build_folders())
    a, b = _twice(_cli("eval_tool/lpips/lpips_compare.py"), ["--device", "cuda"] + paths + [
        "--lpips_ckpt", "none", "--batch-size", "2", "--net", "alex", "--print_sim", "True"], tmp_path, capsys)
    assert a == b and "lpips_value" in a[0]


def test_cli_swap_video_stream_gpu_png_decode(tmp_path):
    """--stream --gpu_png_decode: the frames (one of them RGBA) reach the device chain as device tensors; the files written are those of
    the run without the flag, byte for byte.  Without --stream or --paste_back the flag is refused."""
    import test_stream_gpu as S
    S._make_inputs(tmp_path, 4, rgba=(1,), seed=12)
    for name in ("host", "gpu"):
        S._copy_inputs(tmp_path, tmp_path / name / "base")
    S._run(tmp_path, tmp_path / "host" / "base", tmp_path / "host" / "out", "--stream")
    out = S._run(tmp_path, tmp_path / "gpu" / "base", tmp_path / "gpu" / "out", "--stream", "--gpu_png_decode")
    assert "4 pasted frames" in out
    assert "gpu_png_decode: 4 frames decoded on the device, 0 on the host" in out          # the RGB frames and the RGBA one: none fell back
    names = [f"{i:012d}.png" for i in range(4)]
    S._same_dir(tmp_path / "host" / "out" / "results", tmp_path / "gpu" / "out" / "results", names)
    for n in names:
        assert open(tmp_path / "host" / "out" / "results" / n, "rb").read() == open(tmp_path / "gpu" / "out" / "results" / n, "rb").read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--gpu_png_decode", "--ckpt", "none"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--gpu_png_decode" in r.stderr and "--paste_back or --stream" in r.stderr


def test_cli_swap_video_paste_back_gpu_png_decode(tmp_path):
    """--paste_back --gpu_png_decode, alone and with --gpu_png: the same pasted frames as the host route."""
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
        Image.fromarray(rng.integers(0, 256, (H, W, 3 + i), dtype=np.uint8)).save(base / "clip" / f"{i}.png")          # an RGB and an RGBA frame
        q = np.array([[40.0, 30.0], [40.0, 170.0], [180.0, 170.0], [180.0, 30.0]]) + 20 * i
        coeffs.append(alignment_coefficients(q, 1024))
    np.save(base / "clip_inv_transforms.npy", coeffs)

    def run(out, *extra):
        (out / "temp_results").mkdir(parents=True)
        shutil.copy(base / "source_cropped" / "0.png", out / "temp_results" / "me.png")
        shutil.copy(base / "source_mask" / "0.png", out / "temp_results" / "me.jpg")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "inference_swap_video.py"), "--outdir", str(out), "--Base_dir", str(base),
                            "--target_video", "videos/clip.mp4", "--src_image", "faces/me.jpg", "--config",
                            os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none", "--n_samples", "2", "--ddim_steps", "4", "--scale",
                            "3.5", "--precision", "full", "--num_workers", "0", "--clip_vision_config",
                            json.dumps(dict(hidden=128, intermediate=512, layers=2, heads=4)), "--paste_back", *extra],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        return r.stdout

    assert "decoded on the device" not in run(tmp_path / "host")
    for out in (run(tmp_path / "dec", "--gpu_png_decode"), run(tmp_path / "both", "--gpu_png_decode", "--gpu_png")):
        assert "gpu_png_decode: 2 frames decoded on the device, 0 on the host" in out
    fa = sorted(os.listdir(tmp_path / "host" / "results"))
    assert len(fa) == 2
    for other in ("dec", "both"):
        assert sorted(os.listdir(tmp_path / other / "results")) == fa
        for f in fa:
            ia, ib = Image.open(tmp_path / "host" / "results" / f), Image.open(tmp_path / other / "results" / f)
            assert ia.mode == ib.mode and np.array_equal(np.asarray(ia), np.asarray(ib)), (other, f)
    for f in fa:          # decoded on the device, encoded on the host: the files themselves are the host route's
        assert open(tmp_path / "host" / "results" / f, "rb").read() == open(tmp_path / "dec" / "results" / f, "rb").read()
