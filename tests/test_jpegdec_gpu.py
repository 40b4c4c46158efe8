"""The GPU JPEG decoder (reface_amd/csrc/jpegdec.hip, reface_amd/jpegdec.py) and the callers' --gpu_jpeg_decode / --video_in.  Everything
is compared for exact equality with PIL's decode of the same bytes; where a file is decoded -- device or host, one lane per restart
interval or one lane per scan -- is asserted by name.  The damaged files are the ones the sanitized host program has already run clean
(tests/test_jpegdec_cpu.py)."""
import io
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegdec_refs as R  # noqa: E402
from reface_amd import jpegdec as J  # noqa: E402
from reface_amd import mjpeg as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dec():
    return J.JpegDecoder(DEV)


def _np(t):
    return t.cpu().numpy()


def _same(t, data, mode=None):
    """the device tensor [H, W, C] against PIL's array of `data`"""
    want = R.pil_decode(data, mode)
    got = _np(t)
    return got.shape == want.shape + (() if want.ndim == 3 else (1,)) and np.array_equal(got.reshape(want.shape), want)


# ------------------------------------------------------------------------------------------------ files written by PIL
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_pil_files_equal_pil(dec, sampling):
    """every size, image kind, quality, restart layout and optimize with this sampling: one launch, mixed sizes and plans"""
    cases = [c for c in R.cases(full=True) if c[3] == sampling]
    assert {(c[1], c[2]) for c in cases} == set(R.SIZES) and {c[0] for c in cases} == set(R.KINDS) and {c[4] for c in cases} == set(R.QUALITIES)
    assert {c[5] for c in cases} == set(range(len(R.RESTARTS))) and {c[6] for c in cases} == {False, True}
    files = [R.pil_file(*c) for c in cases]
    job = dec.decode_async(files)
    outs = job.result()
    for c, f, o, r in zip(cases, files, outs, job.report):
        assert r["where"] == "gpu" and r["code"] == 0 and r["plan"] == ("intervals" if c[5] else "serial"), (c, r)
        assert _same(o, f), c


def test_entropy_decode_alone_equals_the_reference(dec):
    cases = [c for c in R.cases() if (c[1], c[2]) != (200, 256)]
    files = [R.pil_file(*c) for c in cases]
    outs, report = dec.coefficients(files)
    for c, f, o, r in zip(cases, files, outs, report):
        assert r["code"] == 0 and np.array_equal(_np(o), R.entropy_decode(J.parse_jpeg(f), f)), c


# ------------------------------------------------------------------------------------------------ batches and staging
MIXED = [("noise", 97, 131, "420", 90, 0, False), ("smooth", 17, 33, "grey", 30, 1, False), ("smooth", 200, 256, "422", 90, 3, True),
         ("checker", 7, 9, "444", 100, 2, False), ("noise", 1, 1, "420", 90, 0, False), ("smooth", 97, 131, "grey", 100, 0, True)]


@pytest.mark.parametrize("misalign", [1, 3, 7])
def test_odd_offsets_into_the_staging_buffer(dec, misalign):
    files = [R.pil_file(*c) for c in MIXED]
    infos = [J.parse_jpeg(f) for f in files]
    L = dec._launch(files, infos, [i.ncomp for i in infos], misalign=misalign)
    try:
        L.event.synchronize()
        assert L.status.cpu().tolist()[0::2] == [0] * len(files)
    finally:
        dec._release(L.staging)
    for c, f, o in zip(MIXED, files, L.images):
        assert _same(o, f), c


@pytest.mark.parametrize("mode", [None, "RGB", "L"])
def test_modes_mixed_sizes_and_routes(dec, mode, tmp_path):
    """paths, bytes and (name, bytes) in one call; grey files run on the device under every mode, RGB -> L is counted as host, and so is a
    progressive file"""
    files = [R.pil_file(*c) for c in MIXED]
    buf = io.BytesIO()
    Image.fromarray(R.image("smooth", 40, 56)).save(buf, "JPEG", quality=90, progressive=True)
    files.append(buf.getvalue())
    items = []
    for k, f in enumerate(files):
        if k % 3 == 0:
            p = tmp_path / f"{k}.jpg"
            p.write_bytes(f)
            items.append(str(p))
        else:
            items.append(f if k % 3 == 1 else (f"item{k}", f))
    before = dict(dec.counts)
    job = dec.decode_async(items, mode)
    outs = job.result()
    where = [r["where"] for r in job.report]
    grey = [c[3] == "grey" for c in MIXED]
    assert where == ["gpu" if (mode != "L" or g) else "host" for g in grey] + ["host"]
    assert job.report[-1]["reason"] == "progressive (SOF2)" and job.batch is None
    if mode == "L":
        assert "PIL's conversion" in job.report[0]["reason"]
    assert dec.counts["gpu"] - before["gpu"] == where.count("gpu") and dec.counts["host"] - before["host"] == where.count("host")
    for f, o in zip(files, outs):
        assert o.is_cuda and o.dtype == torch.uint8 and _same(o, f, mode)
    assert re.fullmatch(r"gpu_jpeg_decode: \d+ files decoded on the device, \d+ on the host", J.counts_line(dec))


def test_one_shape_gives_a_stacked_batch(dec):
    files = [R.pil_file(k, 97, 131, "420", 90, r, False) for k, r in (("smooth", 0), ("noise", 1), ("checker", 3))]
    job = dec.decode_async(files, "RGB")
    outs = job.result()
    assert job.batch is not None and tuple(job.batch.shape) == (3, 97, 131, 3)
    for k, f in enumerate(files):
        assert _same(job.batch[k], f, "RGB") and _same(outs[k], f, "RGB")


# ------------------------------------------------------------------------------------------------ the project's own files
@pytest.mark.parametrize("sub", ["420", "444"])
def test_jpeg_encoder_files_equal_pil(dec, sub):
    imgs = torch.from_numpy(np.stack([R.image(k, 100, 136) for k in ("smooth", "noise", "checker")])).to(DEV)
    files = M.JpegEncoder(DEV, quality=90, subsampling=sub).encode(imgs)
    job = dec.decode_async(files)
    outs = job.result()
    assert [r["plan"] for r in job.report] == ["intervals"] * 3 and [r["where"] for r in job.report] == ["gpu"] * 3
    for f, o in zip(files, outs):
        assert J.parse_jpeg(f).subsampling == sub and _same(o, f)


def test_video_output_read_back_and_frames_without_dht(dec, tmp_path):
    frames = torch.from_numpy(np.stack([np.roll(R.image("smooth", 72, 120), 5 * k, axis=1) for k in range(5)])).to(DEV)
    path = str(tmp_path / "v.avi")
    vo = M.VideoOutput(path, fps=12.0, quality=90, device=DEV)
    vo.push(frames[:3])
    vo.push(frames[3:])
    assert vo.close() == [(path, 5)]
    r = M.AviReader(path)
    assert (len(r), r.width, r.height, r.fps) == (5, 120, 72, 12.0)
    data = list(r)
    r.close()
    job = dec.decode_async([(f"{path}#{k}", d) for k, d in enumerate(data)], "RGB")
    outs = job.result()
    assert job.batch is not None and [x["plan"] for x in job.report] == ["intervals"] * 5
    for d, o in zip(data, outs):
        assert _same(o, d, "RGB")
    # an MJPG frame may omit its DHT segments: the Annex K tables apply
    stripped = [R.strip_dht(d) for d in data[:2]] + [R.strip_dht(R.pil_file("smooth", 97, 131, "422", 90))]
    assert all(s is not None and b"\xff\xc4" not in s[:J.parse_jpeg(s).scan[0]] for s in stripped)
    for s, full, o in zip(stripped, data[:2] + [R.pil_file("smooth", 97, 131, "422", 90)], dec.decode(stripped)):
        assert _same(o, full)


# ------------------------------------------------------------------------------------------------ damaged input
def test_damaged_scans_leave_codes_and_spare_their_neighbours(dec):
    dm = R.damaged_files()
    names = sorted(dm)
    good = [R.pil_file("smooth", 97, 131, "420", 90, 1), R.pil_file("noise", 17, 33, "grey", 90)]
    files = [good[0]] + [dm[n] for n in names] + [good[1]]
    infos = [J.parse_jpeg(f) for f in files]
    assert all(i.route == "gpu" for i in infos)
    L = dec._launch(files, infos, [i.ncomp for i in infos])
    try:
        L.event.synchronize()
        codes = L.status.cpu().tolist()[0::2]
    finally:
        dec._release(L.staging)
    assert codes[0] == 0 and codes[-1] == 0 and _same(L.images[0], good[0]) and _same(L.images[-1], good[1])
    for n, c in zip(names, codes[1:-1]):
        assert c > 0, n
        assert c == R.DAMAGED_CODES.get(n, c), n


def test_damaged_file_raises_naming_the_file(dec, tmp_path):
    p = tmp_path / "broken.jpg"
    p.write_bytes(R.damaged_files()["bad_code"])
    good = R.pil_file("smooth", 17, 33, "420", 90)
    with pytest.raises(J.JpegDecodeError, match="broken.jpg") as e:
        dec.decode([good, str(p)])
    assert e.value.code == R.E_BAD_CODE and e.value.name == str(p)
    with pytest.raises(J.JpegDecodeError, match="frame 3"):
        dec.decode([("frame 3", R.damaged_files()["missing_rst"])])
    assert _same(dec.decode([good])[0], good)          # the decoder goes on working


# ------------------------------------------------------------------------------------------------ callers
TIMING_KEYS = {"seconds", "images_per_s"}


def _cli(rel):
    import importlib.util
    spec = importlib.util.spec_from_file_location("jpegdec_cli_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _jpg_folder(path, names, images, progressive=()):
    """The images as .jpg files (grey arrays as grey files, RGBA without its alpha), restart markers in every second one."""
    os.makedirs(path)
    for k, (name, img) in enumerate(zip(names, images)):
        im = Image.fromarray(img[..., :3] if img.ndim == 3 else img)
        kw = {"progressive": True} if k in progressive else ({"restart_marker_rows": 1} if k % 2 else {})
        im.save(os.path.join(path, os.path.splitext(name)[0] + ".jpg"), "JPEG", quality=90, **kw)
    return str(path)


def _runs(cli, argv, flag_sets, tmp_path, capsys):
    """The command under every set of flags, in this process and without loader workers: [(--json values without timings, printed lines,
    stderr)]."""
    got = []
    for k, flags in enumerate(flag_sets):
        out_json = str(tmp_path / f"out{k}.json")
        capsys.readouterr()
        cli.main(argv + ["--num-workers", "0", "--json", out_json] + list(flags))
        cap = capsys.readouterr()
        r = json.load(open(out_json))
        got.append(({k: v for k, v in r.items() if k not in TIMING_KEYS}, cap.out.splitlines(), cap.err))
    return got


def test_cli_pose_gpu_jpeg_decode(tmp_path, capsys):
    """targets as .jpg (the CelebA-HQ layout), results as .png: --gpu_jpeg_decode alone and with --gpu_png_decode"""
    import pose_inputs as PI
    d = PI.build()
    png = PI.write_folders(str(tmp_path / "png"), d)
    tgt = _jpg_folder(tmp_path / "jpg", d["tgt_names"], d["tgt_images"])
    runs = _runs(_cli("eval_tool/Pose/pose_compare.py"), ["--device", "cuda", tgt, png[1], "--hopenet_ckpt", "none", "--batch-size", "4"],
                 ([], ["--gpu_jpeg_decode"], ["--gpu_jpeg_decode", "--gpu_png_decode"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] == runs[2][:2] and "pose_value" in runs[0][0]
    nt, nr = len(d["tgt_names"]), len(d["res_names"])
    assert "decoded on the device" not in runs[0][2]
    assert f"gpu_jpeg_decode: {nt} files decoded on the device, {nr} on the host" in runs[1][2] and "gpu_png_decode" not in runs[1][2]
    assert f"gpu_jpeg_decode: {nt} files decoded on the device, 0 on the host" in runs[2][2]
    assert f"gpu_png_decode: {nr} files decoded on the device, 0 on the host" in runs[2][2]


def test_cli_fid_gpu_jpeg_decode(tmp_path, capsys):
    """both folders as .jpg, grey files among them, one progressive file that stays with PIL"""
    import fid_inputs as FI
    d = FI.build()
    a = _jpg_folder(tmp_path / "dataset", d["dataset_names"], d["dataset"], progressive=(3,))
    b = _jpg_folder(tmp_path / "results", d["result_names"], d["results"])
    runs = _runs(_cli("eval_tool/fid/fid_score.py"), ["--device", "cuda", a, b, "--clip_ckpt", "none", "--batch-size", "20"],
                 ([], ["--gpu_jpeg_decode"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] and "fid" in runs[0][0]
    n = len(d["dataset_names"]) + len(d["result_names"])
    assert f"gpu_jpeg_decode: {n - 1} files decoded on the device, 0 on the host" in runs[1][2]          # (the progressive file never reaches the decoder)


def test_cli_swap_video_stream_video_in(tmp_path):
    """--stream --video_in X.avi writes the results/ files of the same command run on the PNG frames that PIL decodes from X.avi, and with
    --write_video the output takes the input's rate (and, the pasted frames being equal, is the same file)."""
    import test_stream_gpu as S
    frames = S._make_inputs(tmp_path, 4, seed=14)
    avi = str(tmp_path / "X.avi")
    w = M.AviWriter(avi, 320, 200, 12.0)
    for k, f in enumerate(frames):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=90, **({"restart_marker_rows": 1} if k % 2 else {}))
        w.add(buf.getvalue())
    w.close()
    os.makedirs(tmp_path / "png" / "base" / "clip")
    os.makedirs(tmp_path / "avi" / "base")
    for i, data in enumerate(M.AviReader(avi)):
        Image.open(io.BytesIO(data)).save(tmp_path / "png" / "base" / "clip" / f"{i}.png")
    S._run(tmp_path, tmp_path / "png" / "base", tmp_path / "png" / "out", "--stream", "--write_video", "--video_fps", "12")
    out = S._run(tmp_path, tmp_path / "avi" / "base", tmp_path / "avi" / "out", "--stream", "--video_in", avi, "--write_video")
    assert "4 pasted frames" in out and "gpu_jpeg_decode: 4 frames decoded on the device, 0 on the host" in out and "12 fps" in out
    names = [f"{i:012d}.png" for i in range(4)]
    S._same_dir(tmp_path / "png" / "out" / "results", tmp_path / "avi" / "out" / "results", names)
    for n in names:
        assert open(tmp_path / "png" / "out" / "results" / n, "rb").read() == open(tmp_path / "avi" / "out" / "results" / n, "rb").read()
    r = M.AviReader(str(tmp_path / "avi" / "out" / "clip_swapped.avi"))
    assert (r.fps, len(r), r.width, r.height) == (12.0, 4, 320, 200)
    r.close()
    assert open(tmp_path / "avi" / "out" / "clip_swapped.avi", "rb").read() == open(tmp_path / "png" / "out" / "clip_swapped.avi", "rb").read()


def _to_jpg(folder):
    """Every .png of a fixture folder rewritten as .jpg (restart markers in every second file), the names' numbers kept."""
    for k, name in enumerate(sorted(os.listdir(folder))):
        if name.endswith(".png"):
            im = Image.open(os.path.join(folder, name))
            im.load()
            im = im.convert("RGB") if im.mode not in ("RGB", "L") else im
            im.save(os.path.join(folder, name[:-4] + ".jpg"), "JPEG", quality=92, **({"restart_marker_rows": 1} if k % 2 else {}))
            os.remove(os.path.join(folder, name))
    return len(os.listdir(folder))


def test_cli_expression_gpu_jpeg_decode(tmp_path, capsys):
    import expr_inputs as EI
    paths = EI.write_folders(str(tmp_path / "folders"), EI.build())
    n = sum(_to_jpg(p) for p in paths)
    runs = _runs(_cli("eval_tool/Expression/expression_compare_face_recon.py"),
                 ["--device", "cuda"] + paths + ["--recon_ckpt", "none", "--batch-size", "4", "--print_sim", "True"], ([], ["--gpu_jpeg_decode"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] and "expression_value" in runs[0][0]
    assert f"gpu_jpeg_decode: {n} files decoded on the device, 0 on the host" in runs[1][2]


def test_cli_id_retrieval_gpu_jpeg_decode(tmp_path, capsys):
    """images as .jpg, label maps as .png: with both flags nothing is decoded on the host"""
    import idscore_inputs as II
    paths = II.write_folders(str(tmp_path / "folders"), II.build())
    n = sum(_to_jpg(p) for p in paths[:2])
    runs = _runs(_cli("eval_tool/ID_retrieval/ID_retrieval.py"), ["--device", "cuda"] + paths + [
        "--dataset", II.DATASET, "--print_sim", "True", "--arcface", "True", "--arcface_ckpt", "none", "--batch-size", "5"],
        ([], ["--gpu_jpeg_decode"], ["--gpu_jpeg_decode", "--gpu_png_decode"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] == runs[2][:2] and "top1" in runs[0][0]
    assert f"gpu_jpeg_decode: {n} files decoded on the device, {n} on the host" in runs[1][2]          # (the label maps: PNG files, PIL's)
    assert f"gpu_jpeg_decode: {n} files decoded on the device, 0 on the host" in runs[2][2]
    assert f"gpu_png_decode: {n} files decoded on the device, 0 on the host" in runs[2][2]


def test_cli_lpips_gpu_jpeg_decode(tmp_path, capsys):
    import lpips_inputs as LI
    paths = LI.write_folders(str(tmp_path / "folders"), LI.build_folders())
    for p in paths:
        _to_jpg(p)
    runs = _runs(_cli("eval_tool/lpips/lpips_compare.py"), ["--device", "cuda"] + paths + [
        "--lpips_ckpt", "none", "--batch-size", "2", "--net", "alex", "--print_sim", "True"], ([], ["--gpu_jpeg_decode"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] and "lpips_value" in runs[0][0]
    m = re.search(r"gpu_jpeg_decode: (\d+) files decoded on the device, 0 on the host", runs[1][2])
    assert m and int(m.group(1)) >= runs[1][0]["images"]


def test_cli_swap_video_staged_video_in(tmp_path):
    """--align --parse_masks --paste_back --video_in X.avi: the aligner and the paste-back take the AVI's frames from the device decoder; the
    crops, transforms and pasted frames are those of the same command on the PNG frames that PIL decodes from X.avi."""
    import test_stream_gpu as S
    frames = S._make_inputs(tmp_path, 4, seed=15)
    avi = str(tmp_path / "X.avi")
    w = M.AviWriter(avi, 320, 200, 25.0)
    for k, f in enumerate(frames):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=90, subsampling=k % 3, **({"restart_marker_rows": 1} if k % 2 else {}))
        w.add(buf.getvalue())
    w.close()
    os.makedirs(tmp_path / "png" / "base" / "clip")
    os.makedirs(tmp_path / "avi" / "base")
    for i, data in enumerate(M.AviReader(avi)):
        Image.open(io.BytesIO(data)).save(tmp_path / "png" / "base" / "clip" / f"{i}.png")
    flags = ("--align", "--parse_masks", "--paste_back")
    S._run(tmp_path, tmp_path / "png" / "base", tmp_path / "png" / "out", *flags)
    out = S._run(tmp_path, tmp_path / "avi" / "base", tmp_path / "avi" / "out", *flags, "--video_in", avi)
    assert "gpu_jpeg_decode: " in out and "0 on the host" in out and not os.path.exists(tmp_path / "avi" / "base" / "clip")
    names = [f"{i:012d}.png" for i in range(4)]
    S._same_dir(tmp_path / "png" / "out" / "results", tmp_path / "avi" / "out" / "results", names)
    S._same_dir(tmp_path / "png" / "base" / "clipcropped_face", tmp_path / "avi" / "base" / "clipcropped_face", [f"{i}.png" for i in range(4)])
    assert np.array_equal(np.load(tmp_path / "png" / "base" / "clip_inv_transforms.npy"), np.load(tmp_path / "avi" / "base" / "clip_inv_transforms.npy"))
