"""The self-synchronising plan of the GPU JPEG decoder (reface_amd/csrc/jpeg_sync.h, the jpeg_sync_* kernels of csrc/jpegdec.hip,
``JpegDecoder(parallel=True)``) and the callers' --gpu_jpeg_parallel.  Pixels are compared for exact equality with PIL's decode of the same
bytes, coefficients with the reference decoder's, error codes with the serial plan's run in the same test; which plan a file took, and
whether it fell back to the serial lane, is asserted by name.  The corpus is the one the sanitized host program has already run clean
(tests/test_jpegsync_cpu.py)."""
import io
import os
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
BIG = [("smooth", 200, 256, "420", 90), ("noise", 200, 256, "444", 100), ("smooth", 512, 512, "420", 90)]


@pytest.fixture(scope="module")
def dec():
    return J.JpegDecoder(DEV, parallel=True)


def _np(t):
    return t.cpu().numpy()


def _same(t, data, mode=None):
    """the device tensor [H, W, C] against PIL's array of `data`"""
    want = R.pil_decode(data, mode)
    got = _np(t)
    return got.shape == want.shape + (() if want.ndim == 3 else (1,)) and np.array_equal(got.reshape(want.shape), want)


def _expected_plan(c, data, L, r):
    """what the report of a file must say: the plan it has today unless it has no DRI and at least two sub-sequences"""
    n = J.subseqs_of(J.parse_jpeg(data), L)
    if c[5]:
        return r["plan"] == "intervals" and "fallback" not in r and n == 0
    if n == 0:
        return r["plan"] == "serial" and "fallback" not in r
    return r["subseqs"] == n and ((r["plan"] == "selfsync" and not r["fallback"]) or (r["plan"] == "serial" and r["fallback"])) and 1 <= r["launches_used"] <= J.SS_MAX_LAUNCHES


# ------------------------------------------------------------------------------------------------ files written by PIL
@pytest.mark.parametrize("subseq", [16, 32, J.SUBSEQ_BYTES])
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_pil_files_equal_pil(sampling, subseq):
    """every size, image kind, quality, restart layout and optimize with this sampling: one launch, mixed sizes and all three plans"""
    cases = [c for c in R.cases() if c[3] == sampling] + [c + (0, False) for c in BIG if c[3] == sampling]
    files = [R.pil_file(*c) for c in cases]
    job = J.JpegDecoder(DEV, parallel=True, subseq_bytes=subseq).decode_async(files)
    outs = job.result()
    plans = set()
    for c, f, o, r in zip(cases, files, outs, job.report):
        assert r["where"] == "gpu" and r["code"] == 0 and _expected_plan(c, f, subseq, r), (c, r)
        assert _same(o, f), (c, r)
        plans.add(r["plan"])
    assert plans == {"serial", "intervals", "selfsync"}


def test_entropy_decode_alone_equals_the_reference(dec):
    cases = [c for c in R.cases() if c[5] == 0 and (c[1], c[2]) != (200, 256)] + [c + (0, False) for c in BIG[:2]]
    files = [R.pil_file(*c) for c in cases]
    refs = [R.entropy_decode(J.parse_jpeg(f), f) for f in files]
    for kw in ({}, {"subseq_bytes": 16}, {"subseq_bytes": 32, "sync_launches": 2}, {"parallel": False}):
        outs, report = dec.coefficients(files, **kw)
        for c, f, o, r, want in zip(cases, files, outs, report, refs):
            assert r["code"] == 0 and np.array_equal(_np(o), want), (kw, c, r)
            if kw.get("parallel", True):
                assert _expected_plan(c, f, kw.get("subseq_bytes", J.SUBSEQ_BYTES), r), (kw, c, r)
            else:
                assert r["plan"] == "serial" and "fallback" not in r


MIXED = [("noise", 97, 131, "420", 90, 0, False), ("smooth", 17, 33, "grey", 30, 1, False), ("smooth", 200, 256, "422", 90, 3, True),
         ("checker", 7, 9, "444", 100, 2, False), ("noise", 1, 1, "420", 90, 0, False), ("smooth", 97, 131, "grey", 100, 0, True),
         ("smooth", 200, 256, "420", 90, 0, False)]


@pytest.mark.parametrize("misalign", [1, 3, 7])
def test_odd_offsets_into_the_staging_buffer(dec, misalign):
    files = [R.pil_file(*c) for c in MIXED]
    infos = [J.parse_jpeg(f) for f in files]
    L = dec._launch(files, infos, [i.ncomp for i in infos], misalign=misalign)
    try:
        L.event.synchronize()
        st = L.status.cpu().tolist()
    finally:
        dec._release(L.staging)
    assert st[0::2] == [0] * len(files) and [w & 3 for w in st[1::2]] == [2, 1, 1, 1, 0, 2, 2]
    for c, f, o in zip(MIXED, files, L.images):
        assert _same(o, f), c


def test_one_sync_launch_falls_back_and_stays_exact():
    """a file of several workgroups (the host model of tests/test_jpegsync_cpu.py: every such file of the corpus falls back at K = 1 --
    a boundary state moves off its guess in the first launch) is decoded by the serial lane, to the same pixels"""
    files = [R.pil_file(*BIG[0]), R.pil_file(*BIG[1]), R.pil_file("smooth", 17, 33, "420", 90)]
    assert [-(-J.subseqs_of(J.parse_jpeg(f), 32) // J.SS_LANES) for f in files[:2]] == [5, 103]
    job = J.JpegDecoder(DEV, parallel=True, subseq_bytes=32, sync_launches=1).decode_async(files)
    outs = job.result()
    for f, o, r in zip(files[:2], outs, job.report):
        assert (r["plan"], r["fallback"], r["launches_used"], r["code"]) == ("serial", True, 1, 0), r
        assert _same(o, f)
    r = job.report[2]          # one workgroup: nothing to publish, converged in the launch
    assert (r["plan"], r["fallback"], r["launches_used"]) == ("selfsync", False, 1) and _same(outs[2], files[2])


def test_smooth_files_do_not_fall_back_at_the_defaults(dec):
    """(tests/test_jpegsync_cpu.py asserts the same of the host model, whose launches are the slowest a device's can be)"""
    cases = [c for c in R.cases() if c[5] == 0 and c[0] == "smooth"] + [c + (0, False) for c in BIG if c[0] == "smooth"]
    files = [R.pil_file(*c) for c in cases]
    job = dec.decode_async(files)
    outs = job.result()
    taken = 0
    for c, f, o, r in zip(cases, files, outs, job.report):
        assert _same(o, f) and not r.get("fallback", False), (c, r)
        taken += r["plan"] == "selfsync"
    assert taken == sum(J.subseqs_of(J.parse_jpeg(f), J.SUBSEQ_BYTES) > 0 for f in files) >= 8 and job.report[-1]["subseqs"] > 3 * J.SS_LANES          # the 512 x 512 file: several workgroups


# ------------------------------------------------------------------------------------------------ damaged input
def test_damaged_scans_give_the_serial_plans_codes_and_spare_their_neighbours(dec):
    dm = R.damaged_files()
    names = sorted(dm)
    good = [R.pil_file(*BIG[0]), R.pil_file("noise", 97, 131, "grey", 90)]
    files = [good[0]] + [dm[n] for n in names] + [good[1]]
    infos = [J.parse_jpeg(f) for f in files]
    codes = {}
    for key, kw in (("serial", {"parallel": False}), ("selfsync", {}), ("selfsync16", {"subseq_bytes": 16}), ("fallback", {"subseq_bytes": 16, "sync_launches": 1})):
        L = dec._launch(files, infos, [i.ncomp for i in infos], **kw)
        try:
            L.event.synchronize()
            st = L.status.cpu().tolist()
        finally:
            dec._release(L.staging)
        codes[key] = st[0::2]
        assert st[0] == 0 and st[-2] == 0 and _same(L.images[0], good[0]) and _same(L.images[-1], good[1]), key
        words = st[3:-2:2]          # damaged files are among those the new plan decoded, and among those that fell back
        assert sum(w & 3 == 2 for w in words) >= {"serial": 0, "fallback": 3}.get(key, 7) and sum(w & 4 == 4 for w in words) >= {"fallback": 2}.get(key, 0), (key, words)
    for n, c in zip(names, codes["serial"][1:-1]):
        assert c > 0 and c == R.DAMAGED_CODES.get(n, c), n
    assert codes["selfsync"] == codes["serial"] and codes["selfsync16"] == codes["serial"] and codes["fallback"] == codes["serial"]


def test_damaged_file_raises_naming_the_file(dec, tmp_path):
    p = tmp_path / "broken.jpg"
    p.write_bytes(R.damaged_files()["cut_half"])
    good = R.pil_file(*BIG[0])
    with pytest.raises(J.JpegDecodeError, match="broken.jpg") as e:
        dec.decode([good, str(p)])
    assert e.value.code > 0 and e.value.name == str(p)
    assert _same(dec.decode([good])[0], good)          # the decoder goes on working


# ------------------------------------------------------------------------------------------------ one call, every route and plan
@pytest.mark.parametrize("mode", [None, "RGB"])
def test_mixed_batch_in_one_call(dec, mode):
    files = [R.pil_file(*c) for c in MIXED]
    buf = io.BytesIO()
    Image.fromarray(R.image("smooth", 40, 56)).save(buf, "JPEG", quality=90, progressive=True)
    files.append(buf.getvalue())
    job = dec.decode_async(files, mode)
    outs = job.result()
    assert [r["where"] for r in job.report] == ["gpu"] * len(MIXED) + ["host"] and job.report[-1]["reason"] == "progressive (SOF2)"
    assert [r["plan"] for r in job.report] == ["selfsync", "intervals", "intervals", "intervals", "serial", "selfsync", "selfsync", None]
    for f, o in zip(files, outs):
        assert o.is_cuda and o.dtype == torch.uint8 and _same(o, f, mode)
    same = [R.pil_file(k, 97, 131, "420", 90, r, False) for k, r in (("smooth", 0), ("noise", 1), ("checker", 0))]
    job = dec.decode_async(same, "RGB")
    outs = job.result()
    assert job.batch is not None and tuple(job.batch.shape) == (3, 97, 131, 3) and all(_same(job.batch[k], f, "RGB") for k, f in enumerate(same))


# ------------------------------------------------------------------------------------------------ callers
def test_cli_pose_gpu_jpeg_parallel(tmp_path, capsys):
    import pose_inputs as PI
    import test_jpegdec_gpu as G
    d = PI.build()
    png = PI.write_folders(str(tmp_path / "png"), d)
    tgt = G._jpg_folder(tmp_path / "jpg", d["tgt_names"], d["tgt_images"])
    runs = G._runs(G._cli("eval_tool/Pose/pose_compare.py"), ["--device", "cuda", tgt, png[1], "--hopenet_ckpt", "none", "--batch-size", "4"],
                   ([], ["--gpu_jpeg_decode"], ["--gpu_jpeg_decode", "--gpu_jpeg_parallel"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] == runs[2][:2] and "pose_value" in runs[0][0]
    assert runs[1][2] == runs[2][2] and "gpu_jpeg_decode: " in runs[2][2]          # the counts line is the same


def test_cli_fid_gpu_jpeg_parallel(tmp_path, capsys):
    import fid_inputs as FI
    import test_jpegdec_gpu as G
    d = FI.build()
    a = G._jpg_folder(tmp_path / "dataset", d["dataset_names"], d["dataset"], progressive=(3,))
    b = G._jpg_folder(tmp_path / "results", d["result_names"], d["results"])
    runs = G._runs(G._cli("eval_tool/fid/fid_score.py"), ["--device", "cuda", a, b, "--clip_ckpt", "none", "--batch-size", "20"],
                   ([], ["--gpu_jpeg_decode", "--gpu_jpeg_parallel"]), tmp_path, capsys)
    assert runs[0][:2] == runs[1][:2] and "fid" in runs[0][0]
    n = len(d["dataset_names"]) + len(d["result_names"])
    assert f"gpu_jpeg_decode: {n - 1} files decoded on the device, 0 on the host" in runs[1][2]


def test_cli_swap_video_video_in_gpu_jpeg_parallel(tmp_path):
    """an AVI whose frames PIL wrote without restart markers (a foreign MJPG file): results/ with --gpu_jpeg_parallel is byte for byte
    results/ without it"""
    import test_stream_gpu as S
    frames = S._make_inputs(tmp_path, 4, seed=16)
    avi = str(tmp_path / "X.avi")
    w = M.AviWriter(avi, 320, 200, 12.0)
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=90)
        assert J.subseqs_of(J.parse_jpeg(buf.getvalue()), J.SUBSEQ_BYTES) > J.SS_LANES
        w.add(buf.getvalue())
    w.close()
    os.makedirs(tmp_path / "a" / "base")
    os.makedirs(tmp_path / "b" / "base")
    out_a = S._run(tmp_path, tmp_path / "a" / "base", tmp_path / "a" / "out", "--stream", "--video_in", avi)
    out_b = S._run(tmp_path, tmp_path / "b" / "base", tmp_path / "b" / "out", "--stream", "--video_in", avi, "--gpu_jpeg_parallel")
    line = "gpu_jpeg_decode: 4 frames decoded on the device, 0 on the host"
    assert "4 pasted frames" in out_b and line in out_a and line in out_b
    names = [f"{i:012d}.png" for i in range(4)]
    assert sorted(os.listdir(tmp_path / "b" / "out" / "results")) == names
    for n in names:
        assert open(tmp_path / "a" / "out" / "results" / n, "rb").read() == open(tmp_path / "b" / "out" / "results" / n, "rb").read()
