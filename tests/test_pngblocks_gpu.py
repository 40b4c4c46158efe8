"""The block-parallel inflate plan of the GPU PNG decoder on the device (rf_png_inflate_blocks; ``PngDecoder(parallel=True)``, the callers'
--gpu_png_parallel).  The device is fed only the streams that tests/test_pngblocks_cpu.py runs through the sanitized host program, and
the plan, the chain length and the fallback of every stream must be what that program printed for the same bytes and capacity.  Every
comparison of bytes and pixels is equality; error codes must be those of the same decoder with the plan off."""
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngblocks_inputs as P  # noqa: E402
import pngenc_refs as R  # noqa: E402
from test_pngblocks_cpu import run_host_program  # noqa: E402
from reface_amd import pngdec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    return run_host_program(tmp_path_factory.mktemp("pngblocks"))


@pytest.fixture(scope="module")
def serial_codes():
    """the codes of the whole corpus with the plan off, in one launch"""
    c = P.corpus()
    names = sorted(c)
    _, report = pngdec.PngDecoder(DEV).inflate([c[n][0] for n in names], [c[n][1] for n in names], check=False)
    assert all(set(r) == {"where", "plan", "code"} for r in report)          # no new report field with the plan off
    return {n: (r["code"], r["plan"]) for n, r in zip(names, report)}


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ inflate alone
@pytest.mark.parametrize("bb,misalign", [(64, 0), (64, 1), (64, 3), (1024, 0)])
def test_inflate_corpus(host_run, serial_codes, bb, misalign):
    c = P.corpus()
    names = sorted(c)
    dec = pngdec.PngDecoder(DEV, parallel=True, block_bytes=64, min_bytes=P.MIN_BYTES)
    outs, report = dec.inflate([c[n][0] for n in names], [c[n][1] for n in names], misalign=misalign, check=False, block_bytes=bb)
    plans = set()
    for n, o, r in zip(names, outs, report):
        z, length, raw = c[n]
        h = host_run[(n, bb)]
        assert r["code"] == serial_codes[n][0] == int(h["code"]), (n, r, h)
        if raw is not None:
            assert r["code"] == 0 and _np(o).tobytes() == raw, n
        if serial_codes[n][1] == "segments":          # the segmented plan comes first and keeps its files
            assert r["plan"] == "segments" and r["chunks"] == 0 and not r["fallback"], (n, r)
            continue
        assert (r["plan"], r["chunks"], r["fallback"]) == (h["plan"], int(h["chunks"]), h["fallback"] == "1"), (n, r, h)
        assert r["candidates"] == int(h["candidates"]), (n, r, h)
        plans.add(r["plan"])
    assert plans == {"blocks", "serial"}
    by = dict(zip(names, report))
    if bb == 64:
        assert by["embedded"]["candidates"] > by["embedded"]["chunks"] >= 2          # false candidates, found and ignored
    else:
        assert by["low_ml1"]["fallback"] and by["low_ml1"]["candidates"] > 16 + len(c["low_ml1"][0]) // bb          # more hits than slots
    for n in ("blk_bad_adler", "blk_flip_chunk5", "blk_cut_half", "blk_cut_last3", "blk_distance_before_start", "low_fixed"):
        assert by[n]["plan"] == "serial" and by[n]["fallback"], (n, by[n])


def test_override_turns_the_plan_on_and_off():
    z, raw = P.block_streams()["low_ml3"]
    off = pngdec.PngDecoder(DEV, min_bytes=P.MIN_BYTES)
    on = pngdec.PngDecoder(DEV, parallel=True, min_bytes=P.MIN_BYTES)
    for dec, parallel, want in ((off, None, "serial"), (off, True, "blocks"), (on, None, "blocks"), (on, False, "serial")):
        outs, report = dec.inflate([z], [len(raw)], parallel=parallel)
        assert report[0]["plan"] == want and ("chunks" in report[0]) == (dec.parallel if parallel is None else parallel)
        assert _np(outs[0]).tobytes() == raw
    # a stream below min_bytes is not eligible whatever the capacity
    outs, report = pngdec.PngDecoder(DEV, parallel=True).inflate([z], [len(raw)])
    assert report[0] == {"where": "gpu", "plan": "serial", "code": 0, "chunks": 0, "candidates": 0, "fallback": False} and _np(outs[0]).tobytes() == raw


# ------------------------------------------------------------------------------------------------ whole files
def _pil(data, mode=None):
    im = Image.open(io.BytesIO(data))
    if mode:
        im = im.convert(mode)
    a = np.asarray(im)
    return a.reshape(a.shape[0], a.shape[1], -1)


@pytest.fixture(scope="module")
def pil_files():
    """(name, file bytes): the three pil160 files, a 512 x 512 RGB, a 256 x 256 RGBA and a grey file, all written by PIL"""
    img = P.pil160_image()
    out = [(f"pil160_l{level}", P.pil_png(img, level)) for level in (1, 6, 9)]
    out.append(("rgb512", P.pil_png(P.noisy_photo(512, 512, 3, 7))))
    out.append(("rgba256", P.pil_png(P.noisy_photo(256, 256, 4, 8))))
    out.append(("grey300", P.pil_png(P.noisy_photo(300, 310, 1, 9)[:, :, 0])))
    return out


@pytest.mark.parametrize("mode", [None, "RGB"])
def test_pil_files_equal_pil(pil_files, mode):
    dec = pngdec.PngDecoder(DEV, parallel=True, min_bytes=P.MIN_BYTES)          # the default block_bytes
    job = dec.decode_async([d for _, d in pil_files], mode)
    outs = job.result()
    for (name, data), o, r in zip(pil_files, outs, job.report):
        print(name, r)
        assert r["where"] == "gpu" and r["plan"] == "blocks" and r["chunks"] >= 2 and not r["fallback"], (name, r)
        assert o.is_cuda and o.dtype == torch.uint8 and np.array_equal(_np(o), _pil(data, mode)), (name, mode)


def test_guarded_output_is_untouched_around_the_images():
    """the three pil160 files into the [:, :160, :160] view of a wider tensor of 0xA5"""
    img = P.pil160_image()
    streams = [P.block_streams()[f"pil160_l{level}"][0] for level in (1, 6, 9)]
    dec = pngdec.PngDecoder(DEV, parallel=True, min_bytes=P.MIN_BYTES)
    wide = torch.full((3, 160 + 3, 160 + 5, 3), 0xA5, dtype=torch.uint8, device=DEV)
    L = dec._launch(streams, [(160, 160, 3)] * 3, [3] * 3, out=wide)
    L.event.synchronize()
    dec._release(L.staging)
    st = L.status.cpu().tolist()
    assert st == [0, 2] * 3
    got = _np(wide)
    for b in range(3):
        assert np.array_equal(got[b, :160, :160], img)
    assert (got[:, 160:] == 0xA5).all() and (got[:, :, 160:] == 0xA5).all()


def test_mixed_call_every_file_its_plan(tmp_path):
    enc_img = R.photo_like(200, 256, 3, seed=200)
    files = {"gpu_png.png": R.encode_png(enc_img), "pil.png": P.pil_png(P.noisy_photo(256, 256, 3, 11)), "small.png": P.pil_png(R.photo_like(32, 32, 3, seed=1))}
    buf = io.BytesIO()
    Image.fromarray(R.photo_like(64, 64, 3, seed=2)).quantize(16).save(buf, format="PNG")
    files["palette.png"] = buf.getvalue()
    z = P.block_streams()["pil160_l6"][0]          # its chain is whole: the changed Adler-32 is refused by the resolve stage
    files["damaged.png"] = R.wrap_png(z[:-1] + bytes([z[-1] ^ 1]), 160, 160, 3)
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    on, off = pngdec.PngDecoder(DEV, parallel=True, min_bytes=P.MIN_BYTES), pngdec.PngDecoder(DEV, min_bytes=P.MIN_BYTES)
    job = on.decode_async(paths)
    with pytest.raises(pngdec.PngDecodeError) as e:
        job.result()
    assert e.value.name == paths[4] and "damaged.png" in str(e.value) and e.value.code == 10
    job_off = off.decode_async(paths)
    with pytest.raises(pngdec.PngDecodeError) as e_off:
        job_off.result()
    assert (e_off.value.name, e_off.value.code) == (e.value.name, e.value.code)
    assert [r["where"] for r in job.report] == ["gpu", "gpu", "gpu", "host", "gpu"]
    assert [r["plan"] for r in job.report] == ["segments", "blocks", "serial", None, "serial"]
    assert [r.get("fallback") for r in job.report] == [False, False, False, None, True]
    assert [r["plan"] for r in job_off.report] == ["segments", "serial", "serial", None, "serial"] and "chunks" not in job_off.report[1]
    a, b = on.decode(paths[:4]), off.decode(paths[:4])
    for p, x, y in zip(paths, a, b):
        assert torch.equal(x, y) and np.array_equal(_np(x), _pil(open(p, "rb").read())), p


# ------------------------------------------------------------------------------------------------ callers
def test_cli_pose_gpu_png_parallel(tmp_path, capsys):
    """an eval tool with --gpu_png_decode and with --gpu_png_decode --gpu_png_parallel: stdout, stderr's count line and the --json values"""
    import pose_inputs as PI
    from test_pngdec_gpu import TIMING_KEYS, _cli
    paths = PI.write_folders(str(tmp_path / "folders"), PI.build())
    cli, got = _cli("eval_tool/Pose/pose_compare.py"), []
    for k, flags in enumerate((["--gpu_png_decode"], ["--gpu_png_decode", "--gpu_png_parallel"])):
        out_json = str(tmp_path / f"out{k}.json")
        capsys.readouterr()
        cli.main(["--device", "cuda"] + paths + ["--hopenet_ckpt", "none", "--batch-size", "4", "--num-workers", "0", "--json", out_json] + flags)
        cap = capsys.readouterr()
        r = json.load(open(out_json))
        got.append(({k: v for k, v in r.items() if k not in TIMING_KEYS}, cap.out, [ln for ln in cap.err.splitlines() if "gpu_png_decode" in ln]))
    assert got[0] == got[1] and "pose_value" in got[0][0] and len(got[0][2]) == 1


def test_cli_swap_video_paste_back_gpu_png_parallel(tmp_path):
    """--paste_back --gpu_png_decode with and without --gpu_png_parallel on photo-like frames (an RGB and an RGBA one): the same stdout but
    for the timings, the same files byte for byte"""
    import re
    from test_host_cpu import _prepared_swap_tree
    from reface_amd.pasteback import alignment_coefficients
    base = tmp_path / "base"
    _prepared_swap_tree(str(base), n_tar=2, n_src=1)
    os.rename(base / "target_cropped", base / "clipcropped_face")
    os.rename(base / "mask_frames", base / "clipmask_frames")
    (base / "clip").mkdir()
    coeffs = []
    for i in range(2):
        W, H = 320, 200
        Image.fromarray(P.noisy_photo(H, W, 3 + i, 20 + i)).save(base / "clip" / f"{i}.png")
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
                            json.dumps(dict(hidden=128, intermediate=512, layers=2, heads=4)), "--paste_back", "--gpu_png_decode", *extra],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        return r.stdout

    def plain(text, out):          # the output directory's name and the measured times are the runs' own
        return re.sub(r"\d+\.\d+", "#", text.replace(str(out), "<out>"))

    a, b = run(tmp_path / "serial"), run(tmp_path / "blocks", "--gpu_png_parallel")
    assert "gpu_png_decode: 2 frames decoded on the device, 0 on the host" in a
    assert plain(a, tmp_path / "serial") == plain(b, tmp_path / "blocks")
    fa = sorted(os.listdir(tmp_path / "serial" / "results"))
    assert len(fa) == 2 and sorted(os.listdir(tmp_path / "blocks" / "results")) == fa
    for f in fa:
        assert open(tmp_path / "serial" / "results" / f, "rb").read() == open(tmp_path / "blocks" / "results" / f, "rb").read(), f
