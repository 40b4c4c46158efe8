"""The host side of the GPU JPEG decoder (reface_amd/jpegdec.py, reface_amd/mjpeg.py: AviReader) and its entropy-decoder core
(reface_amd/csrc/jpeg_decode.h) without a GPU.

* tests/jpegdec_refs.py, a pure numpy / Python integer decoder, must equal PIL exactly on the whole corpus: that proves the arithmetic the
  kernels restate (IDCT, fancy upsampling, colour) on this machine, before any GPU run.
* ``parse_jpeg`` names every host reason and routes device-eligible files to the device.
* ``AviReader`` reads back what ``AviWriter`` wrote, continuation parts included, and refuses damaged files and other codecs.
* The core is the code the device runs: tests/jpegdec_host_main.cpp compiles it with a host compiler under AddressSanitizer and
  UndefinedBehaviorSanitizer and runs it, as a child process, over good and damaged scans -- good ones must give the reference's coefficients,
  damaged ones an error code and a clean exit."""
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegdec_refs as R  # noqa: E402
from reface_amd import jpegdec as J  # noqa: E402
from reface_amd import mjpeg as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the integer reference decoder
def test_reference_decoder_equals_pil_on_the_corpus():
    cases = R.cases(full=True)
    assert len(cases) > 150
    for s in R.SAMPLINGS:          # every value of every axis with every sampling
        mine = [c for c in cases if c[3] == s]
        assert {c[0] for c in mine} == set(R.KINDS) and {(c[1], c[2]) for c in mine} == set(R.SIZES) and {c[4] for c in mine} == set(R.QUALITIES)
        assert {c[5] for c in mine} == set(range(len(R.RESTARTS))) and {c[6] for c in mine} == {False, True}
    for c in cases:
        data = R.pil_file(*c)
        info = J.parse_jpeg(data)
        assert info.route == "gpu" and info.subsampling == c[3], (c, info.reason)
        want = R.pil_decode(data)
        got = R.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), c
        assert np.array_equal(R.decode(data, "RGB"), R.pil_decode(data, "RGB")), c


def test_corpus_reaches_the_mechanisms():
    info = J.parse_jpeg(R.pil_file("smooth", 97, 131, "420", 90, 3))
    assert info.ri == 3 and info.intervals == len(info.starts) == 21 and info.intervals > 8          # RSTn wraps past 7; intervals straddle MCU rows (9 MCUs per row)
    assert J.parse_jpeg(R.pil_file("smooth", 97, 131, "444", 90, 2)).intervals == 13 * 17
    assert J.parse_jpeg(R.pil_file("noise", 17, 33, "420", 30, 3, True)).huff != J._STD_HUFF          # optimize=True: tables of the file's own
    assert J.parse_jpeg(R.pil_file("noise", 17, 33, "420", 30)).huff == J._STD_HUFF
    # codes longer than 8 bits (the slow path of the lookup) occur
    assert any(sum(t[0][8:]) > 0 for t in J.parse_jpeg(R.pil_file("noise", 17, 33, "444", 100)).huff.values())
    # a stuffed FF 00 occurs in some scan
    d = R.pil_file("noise", 200, 256, "420", 100, 1)
    i = J.parse_jpeg(d)
    assert b"\xff\x00" in d[i.scan[0]:i.scan[0] + i.scan[1]]


# ------------------------------------------------------------------------------------------------ parse_jpeg
def _save(img, **kw):
    buf = io.BytesIO()
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def _replace_segment(data, marker, new):
    """Replace the first segment with `marker` by `new` (bytes of whole segments; b"" removes it)."""
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + struct.unpack_from(">H", data, pos + 2)[0]
    n = 2 + struct.unpack_from(">H", data, pos + 2)[0]
    return data[:pos] + new + data[pos + n:]


def _segment(data, marker):
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + struct.unpack_from(">H", data, pos + 2)[0]
    return data[pos + 4:pos + 2 + struct.unpack_from(">H", data, pos + 2)[0]]


def test_parse_routes_device_files():
    for c in R.cases():
        info = J.parse_jpeg(R.pil_file(*c))
        assert (info.route, info.height, info.width, info.subsampling) == ("gpu", c[1], c[2], c[3]), c
        assert len(info.starts) == info.intervals and info.starts[0] == 0
    data = M.jpeg_header(16, 16, 90, "420") + b"\x00" * 8 + b"\xff\xd9"
    info = J.parse_jpeg(data)
    assert info.route == "gpu" and info.ri == 1 and not info.std_huff and info.scan == (len(data) - 10, 8)
    stripped = R.strip_dht(R.pil_file("smooth", 17, 33, "420", 90))
    info = J.parse_jpeg(stripped)
    assert b"\xff\xc4" not in stripped[:info.scan[0]] and info.route == "gpu" and info.std_huff and info.huff == J._STD_HUFF


def test_parse_names_every_host_reason():
    rgb = Image.fromarray(R.image("smooth", 40, 56))
    base = _save(rgb, quality=90, subsampling=2)
    assert J.parse_jpeg(base).route == "gpu"
    reason = lambda d: (J.parse_jpeg(d).route, J.parse_jpeg(d).reason)          # noqa: E731
    assert reason(_save(rgb, quality=90, progressive=True)) == ("host", "progressive (SOF2)")
    sof = _segment(base, 0xC0)
    assert reason(_replace_segment(base, 0xC0, _seg(0xC1, sof))) == ("host", "SOF1")                                      # extended sequential
    assert reason(_replace_segment(base, 0xC0, _seg(0xC9, sof))) == ("host", "SOF9")                                      # arithmetic coding
    assert reason(_replace_segment(base, 0xC0, _seg(0xC1, b"\x0c" + sof[1:]))) == ("host", "12-bit samples")
    assert reason(_save(rgb.convert("CMYK"), quality=90)) == ("host", "4 components")
    # PIL writes an RGB-coded file with an Adobe marker (transform 0) for keep_rgb
    adobe0 = _save(rgb, quality=90, keep_rgb=True)
    assert reason(adobe0)[0] == "host" and (reason(adobe0)[1] in ("Adobe APP14 transform 0", "RGB component ids"))
    adobe = _seg(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0))
    assert reason(base[:2] + adobe + base[2:]) == ("host", "Adobe APP14 transform 0")
    assert J.parse_jpeg(base[:2] + _seg(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 1)) + base[2:]).route == "gpu"
    assert reason(_replace_segment(base, 0xC0, _seg(0xC0, sof[:7] + b"\x41" + sof[8:]))) == ("host", "sampling factors 4x1,1x1,1x1")
    s440 = _replace_segment(base, 0xC0, _seg(0xC0, sof[:7] + b"\x12" + sof[8:]))
    assert reason(s440) == ("host", "sampling factors 1x2,1x1,1x1")
    # several scans: a non-interleaved file (one scan per component), and a second SOS behind the first scan
    sos = _segment(base, 0xDA)
    assert reason(_replace_segment(base, 0xDA, _seg(0xDA, b"\x01" + sos[1:3] + sos[-3:]))) == ("host", "more than one scan")
    assert reason(base[:-2] + _seg(0xDA, sos) + b"\x00\xff\xd9") == ("host", "more than one scan")
    assert reason(_replace_segment(base, 0xDA, _seg(0xDA, sos[:-3] + b"\x00\x05\x00"))) == ("host", "not a full sequential scan")
    # DNL: height 0 in SOF and the marker behind the scan; or the marker in front of it
    assert reason(_replace_segment(base, 0xC0, _seg(0xC0, sof[:1] + b"\x00\x00" + sof[3:]))) == ("host", "DNL marker")
    assert reason(base[:-2] + _seg(0xDC, struct.pack(">H", 40)) + b"\xff\xd9") == ("host", "DNL marker")
    # size cap
    big = _replace_segment(base, 0xC0, _seg(0xC0, sof[:1] + struct.pack(">HH", 40, J.MAX_SIDE + 1) + sof[5:]))
    assert reason(big) == ("host", "image too large for the device path")
    assert J.parse_jpeg(_replace_segment(base, 0xC0, _seg(0xC0, sof[:1] + struct.pack(">HH", J.MAX_SIDE, J.MAX_SIDE) + sof[5:]))).route == "gpu"
    dqt = _segment(base, 0xDB)
    assert reason(_replace_segment(base, 0xDB, _seg(0xDB, bytes([0x10 | dqt[0]]) + bytes(128)))) == ("host", "16-bit quantisation table")
    assert reason(_replace_segment(base, 0xDB, b""))[1] in ("a table the scan names is missing", "16-bit quantisation table")
    assert reason(b"\x89PNG\r\n\x1a\n" + bytes(32)) == ("host", "not a JPEG file")
    for cut in (0, 3, 20, 200):
        assert J.parse_jpeg(base[:cut]).route == "host", cut
    # RGB -> L is PIL's conversion; grey -> anything is the device's
    assert J.route(base, "L")[0].route == "host" and "PIL's conversion" in J.route(base, "L")[0].reason
    grey = _save(rgb.convert("L"), quality=90)
    assert [J.route(grey, m)[1] for m in (None, "RGB", "L")] == [1, 3, 1] and [J.route(base, m)[1] for m in (None, "RGB")] == [3, 3]
    with pytest.raises(ValueError):
        J.route(base, "CMYK")


def test_huff_table_layout():
    blk = J.table_block(J.parse_jpeg(R.pil_file("noise", 17, 33, "420", 90)))
    assert len(blk) == J.TABLE_BYTES == 512 + 8 * 912
    t = J.huff_table(*M.DC_LUMA)
    look = np.frombuffer(t, dtype=np.uint16, count=256)
    maxcode = np.frombuffer(t, dtype=np.int32, count=18, offset=512)
    codes = M.huffman_codes(*M.DC_LUMA)
    for sym, (code, length) in codes.items():
        if length <= 8:
            assert look[code << (8 - length)] == (length << 8) | sym and look[((code + 1) << (8 - length)) - 1] == (length << 8) | sym
    assert look[0xFF] == 0 and maxcode[9] == 0x1FE and maxcode[10] == -1 and maxcode[0] == -1
    assert J._huff_ok(*M.AC_LUMA, False) and not J._huff_ok((2,) + (0,) * 15, (1, 2), False) and not J._huff_ok((1,) + (0,) * 15, (16,), True)


# ------------------------------------------------------------------------------------------------ AviReader
def _frames(n, H=24, W=40):
    return [_save(Image.fromarray(np.roll(R.image("smooth", H, W), 3 * k, axis=1)), quality=85 + k % 3) for k in range(n)]


def test_avi_reader_reads_back_what_the_writer_wrote(tmp_path):
    frames = _frames(7)
    path = str(tmp_path / "v.avi")
    w = M.AviWriter(path, 40, 24, 12.5)
    for f in frames:
        w.add(f)
    assert w.close() == [(path, 7)]
    r = M.AviReader(path)
    assert (r.width, r.height, r.fps, len(r)) == (40, 24, 12.5, 7) and (r.rate, r.scale) == (12500, 1000)
    assert list(r) == frames and [r.frame(i) for i in (6, 0, 3)] == [frames[6], frames[0], frames[3]]
    with pytest.raises(IndexError):
        r.frame(7)
    r.close()
    empty = str(tmp_path / "e.avi")
    M.AviWriter(empty, 40, 24, 25).close()
    assert len(M.AviReader(empty)) == 0


def test_avi_reader_follows_continuation_parts(tmp_path):
    frames = _frames(9)
    path = str(tmp_path / "v.avi")
    w = M.AviWriter(path, 40, 24, 30, max_bytes=3 * max(len(f) for f in frames))
    for f in frames:
        w.add(f)
    files = w.close()
    assert len(files) >= 3 and files[1][0].endswith("v.002.avi") and sum(n for _, n in files) == 9
    r = M.AviReader(path)
    assert len(r.parts) == len(files) and len(r) == 9 and list(r) == frames and r.fps == 30.0
    r.close()


def test_avi_reader_refuses_damaged_files_and_other_codecs(tmp_path):
    frames = _frames(4)
    path = str(tmp_path / "v.avi")
    w = M.AviWriter(path, 40, 24, 25)
    for f in frames:
        w.add(f)
    w.close()
    good = open(path, "rb").read()

    def read(data, name="x.avi"):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        r = M.AviReader(p)
        out = list(r)
        r.close()
        return out

    assert read(good) == frames
    for cut in (0, 5, 11, 40, 200, M._MOVI_AT + 6, len(good) // 2, len(good) - 30, len(good) - 1):
        with pytest.raises(ValueError, match=r"x\.avi: at offset \d+"):
            read(good[:cut])
    with pytest.raises(ValueError, match="not a RIFF AVI file"):
        read(np.random.RandomState(0).bytes(4000))
    with pytest.raises(ValueError, match="not a RIFF AVI file"):
        read(b"RIFF" + struct.pack("<I", 100) + b"WAVE" + bytes(100))
    # a frame chunk whose size runs past the movi list
    at = M._MOVI_AT + 12
    assert good[at:at + 4] == b"00dc"
    with pytest.raises(ValueError, match=f"at offset {at}"):
        read(good[:at + 4] + struct.pack("<I", len(good)) + good[at + 8:])
    # an index that points elsewhere
    i0 = good.rindex(b"idx1")
    with pytest.raises(ValueError, match="idx1 entry 1"):
        read(good[:i0 + 8 + 16 + 8] + struct.pack("<I", 12345) + good[i0 + 8 + 16 + 12:])
    # another codec: handler and biCompression
    other = good.replace(b"MJPG", b"H264")
    assert other != good
    with pytest.raises(ValueError, match="not MJPG"):
        read(other)
    k = good.index(b"MJPG", good.index(b"strf"))
    with pytest.raises(ValueError, match="not MJPG"):
        read(good[:k] + b"XVID" + good[k + 4:])


# ------------------------------------------------------------------------------------------------ the decoder core under sanitizers
def _compiler():
    """(compiler, the flags that link the sanitizer runtimes statically into the program)"""
    for cxx, static in (("/opt/rocm/llvm/bin/clang++", ["-static-libsan"]), ("clang++", ["-static-libsan"]), ("g++", ["-static-libasan", "-static-libubsan"])):
        p = shutil.which(cxx) or (cxx if os.path.exists(cxx) else None)
        if p:
            return p, static
    raise RuntimeError("no host C++ compiler")


def _job(data):
    """One file as tests/jpegdec_host_main.cpp reads it: the descriptor the decoder would upload, the interval starts, the tables, the scan."""
    info = J.parse_jpeg(data)
    assert info.route == "gpu", info.reason
    pack = lambda t: sum(int(v) << (8 * c) for c, v in enumerate(t))          # noqa: E731
    desc = np.zeros(J.DESC, dtype=np.int64)
    desc[:19] = (0, info.scan[1], info.height, info.width, info.ncomp, info.hs, info.vs, info.ri, 0, 0, info.ncomp, 0, info.width * info.ncomp, 0, 0,
                 len(info.starts), pack(info.tq), pack(info.td), pack(info.ta))
    return desc.tobytes() + struct.pack("<i", len(info.starts)) + info.starts.astype("<i4").tobytes() + J.table_block(info) + \
        data[info.scan[0]:info.scan[0] + info.scan[1]]


def _good_files():
    out = {f"c{k}": R.pil_file(*c) for k, c in enumerate(R.cases())}
    out["stripped_dht"] = R.strip_dht(R.pil_file("smooth", 97, 131, "420", 90, 1))
    return out


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """Compile tests/jpegdec_host_main.cpp with the sanitizers, write the corpus, run the program once: name -> (fields, coefficients)."""
    d = tmp_path_factory.mktemp("jpegdec")
    exe = str(d / "jpegdec_host_main")
    cxx, static = _compiler()
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    os.path.join(ROOT, "tests", "jpegdec_host_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    corpus = d / "corpus"
    corpus.mkdir()
    files = {**_good_files(), **R.damaged_files()}
    for name, data in files.items():
        (corpus / f"{name}.job").write_bytes(_job(data))
    (corpus / "manifest.txt").write_text("\n".join(files) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(corpus)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        out[f[0]] = ({k: int(v) for k, v in (x.split("=", 1) for x in f[1:])}, np.fromfile(str(corpus / f"{f[0]}.coef"), dtype=np.int16).reshape(-1, 64))
    assert len(out) == len(files)
    return out


def test_core_good_scans_give_the_reference_coefficients(host_run):
    for name, data in _good_files().items():
        info = J.parse_jpeg(data)
        fields, coef = host_run[name]
        assert fields["code"] == 0 and fields["blocks"] == info.blocks and fields["plan"] == (1 if info.ri else 0), (name, fields)
        assert np.array_equal(coef, R.entropy_decode(info, data)), name


def test_core_damaged_scans_give_codes(host_run):
    dm = R.damaged_files()
    assert {"cut_quarter", "cut_half", "cut_tail3", "trailing_ff", "flip_plain", "flip_rows", "flip_grey", "bad_code", "run_past_63", "missing_rst",
            "rst_out_of_order", "dri_larger_than_data"} <= set(dm)
    for name, data in dm.items():
        with pytest.raises(R.RefError):
            R.entropy_decode(J.parse_jpeg(data), data)
        assert host_run[name][0]["code"] > 0, name
    for name, code in R.DAMAGED_CODES.items():
        assert host_run[name][0]["code"] == code, name


# ------------------------------------------------------------------------------------------------ the CLI's refusals, the exports
def test_cli_video_in_refusals(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import inference_swap_video as V
    with pytest.raises(SystemExit, match="--video_in supplies the video's full frames for --paste_back or --stream"):
        V.main(["--video_in", "x.avi"])
    with pytest.raises(SystemExit, match="--video_in supplies"):
        V.main(["--video_in", "x.avi", "--align"])
    with pytest.raises(SystemExit, match="--gpu_png_decode has no PNG frame to decode"):
        V.main(["--video_in", "x.avi", "--stream", "--gpu_png_decode"])
    bad = tmp_path / "bad.avi"
    bad.write_bytes(b"RIFF" + bytes(40))
    with pytest.raises(SystemExit, match=r"--video_in: .*bad\.avi: at offset 0: not a RIFF AVI file"):
        V.main(["--video_in", str(bad), "--stream"])
    with pytest.raises(SystemExit, match="--video_in: .*No such file"):
        V.main(["--video_in", str(tmp_path / "none.avi"), "--paste_back"])
    # a good file, no landmarks: dlib cannot read frames that are not files
    good = str(tmp_path / "good.avi")
    w = M.AviWriter(good, 40, 24, 12.5)
    for f in _frames(2):
        w.add(f)
    w.close()
    src = tmp_path / "me.jpg"
    src.write_bytes(_frames(1)[0])
    with pytest.raises(SystemExit, match="--landmarks"):
        V.main(["--video_in", good, "--stream", "--src_image", str(src), "--Base_dir", str(tmp_path)])
    capsys.readouterr()
    opt = V.build_parser().parse_args(["--stream", "--video_in", good])
    assert opt.video_in == good and opt.video_fps == 25 and V.build_parser().parse_args([]).video_in is None
    assert "video_in" in V.VIDEO_OPTIONS          # the Namespace line printed at the start stays what it was


def test_eval_clis_take_the_flag():
    import importlib.util
    for rel in ("eval_tool/Pose/pose_compare.py", "eval_tool/Expression/expression_compare_face_recon.py", "eval_tool/ID_retrieval/ID_retrieval.py",
                "eval_tool/fid/fid_score.py", "eval_tool/lpips/lpips_compare.py"):
        spec = importlib.util.spec_from_file_location("jpegdec_cli_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        paths = ["a", "b", "c", "d"] if "ID_retrieval" in rel else ["a", "b"]
        args = mod.build_parser().parse_args(["--gpu_jpeg_decode"] + paths)
        assert args.gpu_jpeg_decode and not args.gpu_png_decode and not mod.build_parser().parse_args(paths).gpu_jpeg_decode, rel


def test_byte_folder_dispatches_by_signature(tmp_path):
    from reface_amd import pngdec
    rgb = Image.fromarray(R.image("smooth", 24, 40))
    files = {"a.jpg": _save(rgb, quality=90), "b.jpg": _save(rgb, quality=90, progressive=True), "d.jpg": _save(rgb.convert("L"), quality=90)}
    buf = io.BytesIO()
    rgb.save(buf, "PNG")
    files["c.png"] = buf.getvalue()
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    kinds_of = lambda mode, kinds: ["bytes" if isinstance(it, bytes) else "array" for it in pngdec.ByteFolder(paths, mode, kinds)]          # noqa: E731
    assert kinds_of("RGB", ("png",)) == ["array", "array", "array", "bytes"]                     # as before this decoder existed
    assert kinds_of("RGB", ("jpeg",)) == ["bytes", "array", "bytes", "array"]                    # the progressive file stays with PIL
    assert kinds_of("RGB", ("png", "jpeg")) == ["bytes", "array", "bytes", "bytes"]
    assert kinds_of("L", ("png", "jpeg")) == ["array", "array", "bytes", "array"]                # RGB -> L is PIL's
    for it, p in zip(pngdec.ByteFolder(paths, "RGB", ()), paths):
        assert np.array_equal(it.numpy(), np.asarray(Image.open(p).convert("RGB")))
    assert [J.kind_of(d) for d in files.values()] == ["jpeg", "jpeg", "jpeg", "png"] and J.kind_of(b"GIF89a") is None


def test_exports():
    from reface_amd import _lib
    names = ("rf_jpeg_entropy_decode", "rf_jpeg_idct_u8", "rf_jpeg_upsample_rgb_u8")
    assert all(n in _lib.EXPORTS for n in names)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 108 and all(hasattr(lib, n) for n in names)
    header = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert f"#define RF_JPEGDEC_DESC {J.DESC}" in header and f"#define RF_JPEGDEC_MAX_SIDE {J.MAX_SIDE}" in header
    assert "#define RF_JPEGDEC_TABLE_BYTES (512 + 8 * 912)" in header and J.TABLE_BYTES == 512 + 8 * 912
    core = open(os.path.join(ROOT, "reface_amd", "csrc", "jpeg_decode.h")).read()
    assert f"constexpr int DESC = {J.DESC};" in core
    for code, text in J.ERRORS.items():          # the codes Python names are the header's
        assert f"= {code}," in core, (code, text)
