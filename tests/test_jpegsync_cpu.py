"""The self-synchronising plan of the GPU JPEG decoder (reface_amd/csrc/jpeg_sync.h, ``JpegDecoder(parallel=True)``, the callers'
--gpu_jpeg_parallel) without a GPU.

tests/jpegsync_host_main.cpp compiles the shared core with a host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and
emulates the launch structure -- workgroups of 64 lanes, K launches that each start from the boundary states of the launch before, the
serial fallback -- as a child process, over good and damaged files, at sub-sequences of 16, 32 and 128 bytes and K = 1, 2 and the
default.  Good files must give the reference's coefficients under every setting, fallback or not; damaged files the code the serial core
gives the same bytes in the same program."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegdec_refs as R  # noqa: E402
from test_jpegdec_cpu import _compiler, _job  # noqa: E402
from reface_amd import jpegdec as J  # noqa: E402
from reface_amd import mjpeg as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSEQ = (16, 32, 128)
LAUNCHES = (1, 2, J.SYNC_LAUNCHES)
BIG = [("smooth", 200, 256, "420", 90), ("noise", 200, 256, "444", 100)]


def good_files():
    out = {f"c{k}": R.pil_file(*c) for k, c in enumerate(R.cases()) if c[5] == 0}
    out.update({f"big{k}": R.pil_file(*c) for k, c in enumerate(BIG)})
    return out


def damaged_files():
    return {n: d for n, d in R.damaged_files().items() if J.parse_jpeg(d).ri == 0}


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    """{(subseq_bytes, launches): {name: (fields, coefficients)}}: the program compiled once and run once per setting."""
    d = tmp_path_factory.mktemp("jpegsync")
    exe = str(d / "jpegsync_host_main")
    cxx, static = _compiler()
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    os.path.join(ROOT, "tests", "jpegsync_host_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    corpus = d / "corpus"
    corpus.mkdir()
    files = {**good_files(), **damaged_files()}
    for name, data in files.items():
        (corpus / f"{name}.job").write_bytes(_job(data))
    (corpus / "manifest.txt").write_text("\n".join(files) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    runs = {}
    for L in SUBSEQ:
        for K in sorted(set(LAUNCHES)):
            r = subprocess.run([exe, str(corpus), str(L), str(K)], capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (L, K, r.stderr[-4000:])          # no sanitizer report
            out = {}
            for line in r.stdout.splitlines():
                f = line.split()
                out[f[0]] = ({k: int(v) for k, v in (x.split("=", 1) for x in f[1:])}, np.fromfile(str(corpus / f"{f[0]}.coef"), dtype=np.int16).reshape(-1, 64))
            assert len(out) == len(files)
            runs[(L, K)] = out
    return runs


@pytest.fixture(scope="module")
def references():
    return {name: R.entropy_decode(J.parse_jpeg(data), data) for name, data in good_files().items()}


def test_good_scans_give_the_reference_coefficients_under_every_setting(host_runs, references):
    for (L, K), run in host_runs.items():
        for name, data in good_files().items():
            info = J.parse_jpeg(data)
            fields, coef = run[name]
            assert fields["code"] == 0 and fields["serial_code"] == 0 and fields["blocks"] == info.blocks, (L, K, name, fields)
            taken = info.scan[1] >= 2 * L
            assert fields["subseqs"] == (-(-info.scan[1] // L) if taken else 0) and fields["plan"] == (0 if not taken or fields["fallback"] else 2), (L, K, name, fields)
            assert np.array_equal(coef, references[name]), (L, K, name, fields)


def test_damaged_scans_give_the_serial_plans_code(host_runs):
    dm = damaged_files()
    assert {"cut_quarter", "cut_half", "cut_tail3", "trailing_ff", "flip_plain", "flip_grey", "bad_code", "run_past_63", "rst_without_dri", "cut_all", "cut_one"} <= set(dm)
    for (L, K), run in host_runs.items():
        for name in dm:
            fields = run[name][0]
            assert fields["code"] > 0 and fields["code"] == fields["serial_code"], (L, K, name, fields)
            assert fields["code"] == R.DAMAGED_CODES.get(name, fields["code"]), (L, K, name, fields)
    # some of them are met by the write pass of the new plan, not by its fallback or by a scan below the size floor
    for L in SUBSEQ:
        met = [n for n in dm if host_runs[(L, J.SYNC_LAUNCHES)][n][0]["plan"] == 2]
        assert {"cut_quarter", "cut_half", "cut_tail3", "trailing_ff", "flip_plain", "rst_without_dri"} <= set(met), (L, met)


def test_corpus_reaches_the_mechanisms(host_runs):
    good = good_files()
    K = J.SYNC_LAUNCHES
    for L in SUBSEQ:
        run = {n: host_runs[(L, K)][n][0] for n in good}
        assert any(f["straddle"] > 0 for f in run.values() if f["plan"] == 2), L               # symbols straddle the cuts
        assert any(f["subseqs"] == 0 and f["plan"] == 0 for f in run.values()), L              # a scan shorter than two sub-sequences stays serial
        assert any(f["wgs"] >= 3 for f in run.values()), L                                     # files of several workgroups
        assert any(f["plan"] == 2 and f["wgs"] >= 2 and not f["fallback"] for f in run.values()), L          # that converge within the default launches
        one = {n: host_runs[(L, 1)][n][0] for n in good}
        assert any(f["fallback"] and f["wgs"] >= 2 for f in one.values()), L                   # and fall back at K = 1
        assert all(not f["fallback"] for f in one.values() if f["wgs"] <= 1), L
    assert any(f[0]["ff_cut"] > 0 for n, f in host_runs[(16, K)].items() if n in good)          # a cut between FF and its stuffed 00
    # a code longer than 8 bits and a stuffed byte occur in files that take the plan
    data = good["big1"]
    info = J.parse_jpeg(data)
    assert b"\xff\x00" in data[info.scan[0]:info.scan[0] + info.scan[1]] and any(sum(t[0][8:]) > 0 for t in info.huff.values())


def test_smooth_files_do_not_fall_back_at_the_defaults(host_runs):
    """what tests/test_jpegsync_gpu.py asserts on the device, first on the host model (whose launches are the slowest a device can be: every
    workgroup sees only what the launch before published)"""
    run = host_runs[(J.SUBSEQ_BYTES, J.SYNC_LAUNCHES)] if (J.SUBSEQ_BYTES, J.SYNC_LAUNCHES) in host_runs else None
    assert run is not None, "the default sub-sequence size is one of the tested ones"
    smooth = [n for n, c in ((f"c{k}", c) for k, c in enumerate(R.cases())) if c[5] == 0 and c[0] == "smooth"] + ["big0"]
    assert len(smooth) > 20
    for n in smooth:
        assert not run[n][0]["fallback"], (n, run[n][0])


# ------------------------------------------------------------------------------------------------ the decoder's arguments, the CLIs, the exports
def test_decoder_arguments():
    assert J.PLANS == ("serial", "intervals", "selfsync") and J.SUBSEQ_BYTES >= 16 and 1 <= J.SYNC_LAUNCHES <= 16
    d = J.JpegDecoder("cpu", parallel=True, subseq_bytes=32, sync_launches=2)
    assert (d.parallel, d.subseq_bytes, d.sync_launches) == (True, 32, 2)
    d = J.JpegDecoder("cpu")
    assert (d.parallel, d.subseq_bytes, d.sync_launches) == (False, J.SUBSEQ_BYTES, J.SYNC_LAUNCHES)
    for kw in ({"subseq_bytes": 15}, {"subseq_bytes": 1 << 17}, {"sync_launches": 0}, {"sync_launches": 17}):
        with pytest.raises(ValueError):
            J.JpegDecoder("cpu", parallel=True, **kw)
    f = J.FileDecoder("cpu", jpeg=True, jpeg_parallel=True)
    assert f.jpeg.parallel and not J.FileDecoder("cpu", jpeg=True).jpeg.parallel
    # which files take the plan
    big, small, dri = R.pil_file(*BIG[0]), R.pil_file("smooth", 8, 8, "grey", 90), R.pil_file("smooth", 97, 131, "420", 90, 1)
    take = lambda data, L: J.subseqs_of(J.parse_jpeg(data), L)          # noqa: E731
    assert take(big, 128) == -(-J.parse_jpeg(big).scan[1] // 128) and take(small, 128) == 0 and take(dri, 16) == 0
    n = J.parse_jpeg(small).scan[1]
    assert take(small, 16) == (-(-n // 16) if n >= 32 else 0)


def _cli(rel):
    spec = importlib.util.spec_from_file_location("jpegsync_cli_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


EVAL_CLIS = ("eval_tool/Pose/pose_compare.py", "eval_tool/Expression/expression_compare_face_recon.py", "eval_tool/ID_retrieval/ID_retrieval.py",
             "eval_tool/fid/fid_score.py", "eval_tool/lpips/lpips_compare.py")


@pytest.mark.parametrize("rel", EVAL_CLIS)
def test_eval_clis_take_and_refuse_the_flag(rel):
    mod = _cli(rel)
    paths = ["a", "b", "c", "d"] if "ID_retrieval" in rel else ["a", "b"]
    args = mod.build_parser().parse_args(["--gpu_jpeg_decode", "--gpu_jpeg_parallel"] + paths)
    assert args.gpu_jpeg_decode and args.gpu_jpeg_parallel and not mod.build_parser().parse_args(["--gpu_jpeg_decode"] + paths).gpu_jpeg_parallel
    with pytest.raises(SystemExit, match="--gpu_jpeg_parallel .*--gpu_jpeg_decode"):
        mod.main(["--gpu_jpeg_parallel"] + paths)
    with pytest.raises(SystemExit, match="--gpu_jpeg_parallel .*--gpu_jpeg_decode"):
        mod.main(["--gpu_jpeg_parallel", "--gpu_png_decode"] + paths)


def test_video_cli_takes_and_refuses_the_flag():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import inference_swap_video as V
    opt = V.build_parser().parse_args(["--stream", "--video_in", "x.avi", "--gpu_jpeg_parallel"])
    assert opt.gpu_jpeg_parallel and not V.build_parser().parse_args(["--stream", "--video_in", "x.avi"]).gpu_jpeg_parallel
    assert "gpu_jpeg_parallel" in V.VIDEO_OPTIONS          # the Namespace line printed at the start stays what it was
    with pytest.raises(SystemExit, match="--gpu_jpeg_parallel .*--video_in"):
        V.main(["--gpu_jpeg_parallel", "--stream"])
    with pytest.raises(SystemExit, match="--gpu_jpeg_parallel .*--video_in"):
        V.main(["--gpu_jpeg_parallel"])


def test_exports_and_header_constants():
    from reface_amd import _lib
    names = ("rf_jpeg_selfsync_decode", "rf_jpeg_selfsync_work_bytes")
    assert all(n in _lib.EXPORTS for n in names)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 109 and all(hasattr(lib, n) for n in names)
        assert lib.rf_jpeg_selfsync_work_bytes(100, 2, 3) == 8 * (100 + 2 + 3 + 100) + 4 * (100 + 3 * 16) and lib.rf_jpeg_selfsync_work_bytes(-1, 0, 1) == -1
    header = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert f"#define RF_JPEGDEC_DESC {J.DESC}" in header and "#define RF_JPEGDEC_SS_ALL 31" in header and J.SS_ALL == 31
    assert all(n + "(" in header for n in names)
    core = open(os.path.join(ROOT, "reface_amd", "csrc", "jpeg_sync.h")).read()
    assert '#include "jpeg_decode.h"' in core and "D_SS_BEGIN = 19" in core and "constexpr int PLAN_SELFSYNC = 2;" in core and "constexpr int ST_FALLBACK = 4;" in core
    assert f"constexpr int SS_MIN_BYTES = {J.SS_MIN_BYTES};" in core and f"constexpr int SS_MAX_BYTES = 1 << {J.SS_MAX_BYTES.bit_length() - 1};" in core
    assert f"constexpr int SS_MAX_LAUNCHES = {J.SS_MAX_LAUNCHES};" in core and f"constexpr int SS_LANES = {J.SS_LANES};" in core
    assert J.PLANS[2] == "selfsync" and M.ZIGZAG[1] == 1
