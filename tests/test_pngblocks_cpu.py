"""The block-parallel inflate plan of the GPU PNG decoder (reface_amd/csrc/png_blocks.h; ``PngDecoder(parallel=True)``, the callers'
--gpu_png_parallel) without a GPU.

tests/pngblocks_host_main.cpp compiles the shared core with a host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and
emulates the five stages (search, count, chain, decode, resolve) as a child process over the corpus of tests/pngblocks_inputs.py at both
capacities the device test uses; what it prints (plan, chunks, candidates, fallback) is what tests/test_pngblocks_gpu.py expects of the
device for the same bytes."""
import hashlib
import importlib.util
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngblocks_inputs as P  # noqa: E402
from test_pngdec_cpu import _compiler  # noqa: E402
from reface_amd import _lib, jpegdec, pngdec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host_program(d):
    """Compile the program with the sanitizers, write the corpus into directory d, run it once: (name, block_bytes) -> its printed fields."""
    exe = str(d / "pngblocks_host_main")
    cxx, static = _compiler()
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    os.path.join(ROOT, "tests", "pngblocks_host_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    corpus = d / "corpus"
    corpus.mkdir()
    lines = []
    for name, (z, n, _) in P.corpus().items():
        (corpus / name).write_bytes(z)
        lines.append(f"{name} {n}")
    (corpus / "manifest.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(corpus), str(P.MIN_BYTES)] + [str(b) for b in P.BLOCK_BYTES], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        fields = {k: v for k, v in (x.split("=", 1) for x in f[1:])}
        out[(f[0], int(fields["bb"]))] = fields
    assert len(out) == len(lines) * len(P.BLOCK_BYTES)
    return out


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    return run_host_program(tmp_path_factory.mktemp("pngblocks"))


def test_good_streams_equal_zlib_under_every_setting(host_run):
    for name, (z, n, raw) in P.corpus().items():
        if raw is None:
            continue
        for bb in P.BLOCK_BYTES:
            r = host_run[(name, bb)]
            assert r["code"] == "0" and r["same"] == "1", (name, bb, r)
            assert r["sha"] == r["out"] == hashlib.sha256(raw).hexdigest(), (name, bb)


def test_multi_block_streams_take_the_plan_and_every_true_start_is_found(host_run):
    for name, least in P.MULTI_BLOCK.items():
        r = host_run[(name, 64)]
        dyn, chunks = int(r["dyn"]), int(r["chunks"])
        print(f"{name}: {dyn} dynamic of {r['blocks']} blocks, {r['candidates']} candidates, {chunks} chunks, max distance {r['maxdist']}")
        assert dyn >= least, (name, r)
        assert r["plan"] == "blocks" and r["fallback"] == "0", (name, r)
        assert int(r["dynfound"]) == dyn, (name, r)          # the candidate set contains every true dynamic-block start
        assert chunks == int(r["chaintrue"]) == dyn, (name, r)          # (these streams start with a dynamic block: candidate 0 is one of them)
    assert int(host_run[("low_ml1", 64)]["fixed"]) >= 1          # a fixed block inside a chunk
    assert int(host_run[("low_ml1", 64)]["maxdist"]) > 32000 and int(host_run[("per32k_ml3", 64)]["maxdist"]) > 32000


def test_false_candidates_in_a_stored_payload_are_ignored(host_run):
    r = host_run[("embedded", 64)]
    assert r["plan"] == "blocks" and int(r["candidates"]) > int(r["chunks"]) >= 2, r
    assert int(r["chunks"]) == int(r["chaintrue"]), r


def test_capacity_overflow_falls_back(host_run):
    r = host_run[("low_ml1", 1024)]
    z = P.block_streams()["low_ml1"][0]
    assert int(r["candidates"]) > 16 + len(z) // 1024, r
    assert r["plan"] == "serial" and r["eligible"] == "1" and r["fallback"] == "1", r
    assert host_run[("low_ml3", 1024)]["plan"] == "blocks"          # (the same bytes in fewer blocks fit)


def test_streams_that_are_not_taken(host_run):
    for bb in P.BLOCK_BYTES:
        r = host_run[("low_fixed", bb)]
        assert r["plan"] == "serial" and r["candidates"] == "1" and r["dyn"] == "0" and int(r["blocks"]) >= 77, r
    below = [name for name, (z, n, raw) in P.corpus().items() if n < P.MIN_BYTES]
    assert len(below) > 20
    for name in below:
        for bb in P.BLOCK_BYTES:
            r = host_run[(name, bb)]
            assert r["plan"] == "serial" and r["eligible"] == "0" and r["fallback"] == "0" and r["candidates"] == "0", (name, r)


def test_damaged_streams_end_on_the_serial_plan_with_its_code(host_run):
    n_eligible = 0
    for name, (z, n, raw) in P.corpus().items():
        if raw is not None:
            continue
        for bb in P.BLOCK_BYTES:
            r = host_run[(name, bb)]
            assert r["plan"] == "serial" and r["code"] != "0" and r["out"] == "-", (name, bb, r)
            n_eligible += r["eligible"] == "1"
    assert n_eligible > 200          # most of them went through the five stages before the serial plan had them
    assert host_run[("blk_bad_adler", 64)]["code"] == "10"
    assert host_run[("blk_cut_half", 64)]["code"] == "1" and host_run[("blk_cut_last3", 64)]["code"] == "1"
    assert host_run[("blk_distance_before_start", 64)]["code"] == "7"
    # the chain of these two is whole: they are refused by the resolve stage alone (the Adler-32; a marker in front of the stream)
    assert int(host_run[("blk_bad_adler", 64)]["candidates"]) >= 39 and int(host_run[("blk_distance_before_start", 64)]["dynfound"]) >= 1


# ------------------------------------------------------------------------------------------------ the Python side
def test_decoder_arguments():
    d = pngdec.PngDecoder("cpu", parallel=True)
    assert d.parallel and d.block_bytes == 1024 and d.min_bytes == 65536
    d = pngdec.PngDecoder("cpu", parallel=True, block_bytes=64, min_bytes=P.MIN_BYTES)
    assert (d.block_bytes, d.min_bytes) == (64, P.MIN_BYTES)
    assert not pngdec.PngDecoder("cpu").parallel
    for bad in (0, 15, 1.5, (1 << 20) + 1):
        with pytest.raises(ValueError, match="block_bytes"):
            pngdec.PngDecoder("cpu", parallel=True, block_bytes=bad)
    with pytest.raises(ValueError, match="min_bytes"):
        pngdec.PngDecoder("cpu", parallel=True, min_bytes=0)
    assert pngdec.PLANS == {0: "serial", 1: "segments", 2: "blocks"}
    f = jpegdec.FileDecoder("cpu", png=True, png_parallel=True)
    assert f.png.parallel and f.jpeg is None and not jpegdec.FileDecoder("cpu", png=True).png.parallel


def _load(rel):
    spec = importlib.util.spec_from_file_location("pngblocks_cli_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rel", ["eval_tool/Pose/pose_compare.py", "eval_tool/Expression/expression_compare_face_recon.py",
                                 "eval_tool/ID_retrieval/ID_retrieval.py", "eval_tool/fid/fid_score.py", "eval_tool/lpips/lpips_compare.py"])
def test_eval_tools_refuse_the_flag_without_gpu_png_decode(rel):
    mod = _load(rel)
    paths = ["a", "b", "c", "d"] if "ID_retrieval" in rel else ["a", "b"]
    args = mod.build_parser().parse_args(["--gpu_png_decode", "--gpu_png_parallel"] + paths)
    assert args.gpu_png_decode and args.gpu_png_parallel and not mod.build_parser().parse_args(["--gpu_png_decode"] + paths).gpu_png_parallel
    with pytest.raises(SystemExit, match="--gpu_png_parallel .*--gpu_png_decode"):
        mod.main(["--gpu_png_parallel"] + paths)
    with pytest.raises(SystemExit, match="--gpu_png_parallel .*--gpu_png_decode"):
        mod.main(["--gpu_png_parallel", "--gpu_jpeg_decode"] + paths)


def test_swap_video_refuses_the_flag_without_gpu_png_decode():
    V = _load("scripts/inference_swap_video.py")
    opt = V.build_parser().parse_args(["--stream", "--gpu_png_decode", "--gpu_png_parallel"])
    assert opt.gpu_png_parallel and not V.build_parser().parse_args(["--stream", "--gpu_png_decode"]).gpu_png_parallel
    assert "gpu_png_parallel" in V.VIDEO_OPTIONS          # the Namespace line printed at the start stays what it was
    with pytest.raises(SystemExit, match="--gpu_png_parallel .*--gpu_png_decode"):
        V.main(["--gpu_png_parallel", "--stream"])
    with pytest.raises(SystemExit, match="--gpu_png_parallel .*--gpu_png_decode"):
        V.main(["--gpu_png_parallel", "--paste_back"])


def test_library_exports_the_entry_point():
    assert "rf_png_inflate_blocks" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert "int rf_png_inflate_blocks(" in hdr and "#define RF_PNGDEC_DESC 12" in hdr
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 111 and hasattr(lib, "rf_png_inflate_blocks")
