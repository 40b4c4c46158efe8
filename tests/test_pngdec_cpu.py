"""The host side of the GPU PNG decoder (reface_amd/pngdec.py) and its decoder core (reface_amd/csrc/png_inflate.h) without a GPU.

The core is the code the device runs: tests/pngdec_host_main.cpp compiles it with a host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and runs it, as a child process, over the corpus of tests/pngdec_inputs.py -- good streams must give zlib's bytes,
damaged ones an error code and a clean exit.  The program also runs the segmented plan (a piece per candidate start, then chain_accept)
exactly as the device does, so the plan each stream ends on is asserted here by name before any GPU sees it."""
import hashlib
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image, UnidentifiedImageError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngdec_inputs as I  # noqa: E402
import pngenc_refs as R  # noqa: E402
from reface_amd import pngdec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = R.SEG


# ------------------------------------------------------------------------------------------------ the chunk parser
def _chunk(tag, data, crc=None):
    c = zlib.crc32(tag + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", c)


def _png(w, h, depth, ctype, idats, lace=0, before=(), between=(), after=(), ihdr_crc=None):
    out = R.PNG_SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, lace), ihdr_crc)
    for c in before:
        out += c
    for k, d in enumerate(idats):
        out += _chunk(b"IDAT", d)
        if k == 0:
            for c in between:
                out += c
    for c in after:
        out += c
    return out + _chunk(b"IEND", b"")


def _rgb_stream(w=5, h=3):
    img = np.random.RandomState(0).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    return img, zlib.compress(R.filter_image(img)[0].tobytes())


def test_parse_several_idat_and_ancillary_chunks():
    img, z = _rgb_stream()
    cuts = [z[:7], z[7:8], b"", z[8:]]          # (an empty IDAT is allowed)
    text = _chunk(b"tEXt", b"Comment\0hello")
    data = _png(5, 3, 8, 2, cuts, before=[_chunk(b"gAMA", struct.pack(">I", 45455)), text], after=[text])
    info = pngdec.parse_png(data)
    assert (info.route, info.width, info.height, info.bpp, info.n_idat, info.expect) == ("gpu", 5, 3, 3, 4, 3 * 16)
    assert info.idat(data) == z
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)          # PIL reads the same file the same way


def test_parse_real_pil_file_is_split_at_64k():
    noise = np.random.RandomState(1).randint(0, 256, size=(300, 300, 3)).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(noise).save(buf, format="PNG")
    info = pngdec.parse_png(buf.getvalue())
    assert info.route == "gpu" and info.n_idat == 5
    assert len(zlib.decompress(info.idat(buf.getvalue()))) == info.expect == 300 * 901


def test_parse_routes_to_host_what_pil_decides():
    img, z = _rgb_stream()
    good = _png(5, 3, 8, 2, [z])
    assert pngdec.parse_png(good).route == "gpu"
    # an ancillary chunk between two IDATs: PIL stops reading image data there, so PIL decides what such a file is
    assert pngdec.parse_png(_png(5, 3, 8, 2, [z[:9], z[9:]], between=[_chunk(b"tEXt", b"a\0b")])).reason == "IDAT chunks are not consecutive"
    assert "bad CRC" in pngdec.parse_png(_png(5, 3, 8, 2, [z], ihdr_crc=12345)).reason
    assert "bad CRC" in pngdec.parse_png(_png(5, 3, 8, 2, [z], before=[_chunk(b"gAMA", b"\0\0\0\1", crc=1)])).reason
    with pytest.raises(UnidentifiedImageError):          # (PIL's own refusal of the same file)
        Image.open(io.BytesIO(_png(5, 3, 8, 2, [z], ihdr_crc=12345)))
    for cut in (0, 7, 8, 20, 33, len(good) - 13, len(good) - 1):
        assert pngdec.parse_png(good[:cut]).route == "host", cut
    assert pngdec.parse_png(b"\xff\xd8\xff\xe0 a jpeg").reason == "not a PNG file"
    assert pngdec.parse_png(_png(5, 3, 8, 2, [z], before=[_chunk(b"tRNS", bytes(6))])).reason == "tRNS chunk"
    assert pngdec.parse_png(_png(5, 3, 8, 3, [z], before=[_chunk(b"PLTE", bytes(6))])).route == "host"
    assert pngdec.parse_png(_png(5, 3, 8, 2, [z], lace=1)).reason == "interlaced"
    for depth in (1, 2, 4, 8, 16):
        for ctype in (0, 2, 3, 4, 6):
            want = "gpu" if depth == 8 and ctype != 3 else "host"
            assert pngdec.parse_png(_png(5, 3, depth, ctype, [z])).route == want, (depth, ctype)
    assert pngdec.parse_png(_png(pngdec.MAX_WIDTH, 3, 8, 2, [z])).route == "gpu"
    assert pngdec.parse_png(_png(pngdec.MAX_WIDTH + 1, 3, 8, 2, [z])).route == "host"          # wider than the device's row buffer
    assert pngdec.parse_png(_png(1, pngdec.MAX_HEIGHT, 8, 0, [z])).route == "gpu"
    assert pngdec.parse_png(_png(1, pngdec.MAX_HEIGHT + 1, 8, 0, [z])).route == "host"         # more rows than rf_png_unfilter_u8 takes


def test_out_channels():
    assert [pngdec._out_channels(b, None) for b in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert [pngdec._out_channels(b, "RGB") for b in (1, 2, 3, 4)] == [3, 3, 3, 3]
    assert [pngdec._out_channels(b, "L") for b in (1, 2, 3, 4)] == [1, 1, None, None]
    with pytest.raises(ValueError):
        pngdec._out_channels(3, "CMYK")


# ------------------------------------------------------------------------------------------------ candidate listing
def test_list_candidates():
    g = I.good_streams()
    z = g["enc_seg3plus5"][0]
    c = pngdec.list_candidates(z)
    assert len(c) == 3 and all(z[o - 4:o] == b"\x00\x00\xff\xff" for o in c)
    assert pngdec.list_candidates(g["enc_len32768"][0]) == []
    assert pngdec.list_candidates(g["zlib6_text"][0]) == []
    assert len(pngdec.list_candidates(g["sync_flush"][0])) == 2
    # stored segments carry no marker: the start of the second one is found from the first one's length
    assert pngdec.list_candidates(g["enc_noise"][0]) == [2 + 5 + SEG]
    assert pngdec.list_candidates(g["enc_noise3"][0]) == [2 + 5 + SEG, 2 + 2 * (5 + SEG)]
    z = g["stored_payload_marker"][0]
    # a false candidate inside the payload; zlib's level 0 also ends with an empty final stored block, in front of the trailer
    assert pngdec.list_candidates(z) == [2 + 5 + 300 + 4, len(z) - 4]


# ------------------------------------------------------------------------------------------------ the decoder core under sanitizers
def _compiler():
    """(compiler, the flags that link the sanitizer runtimes statically into the program)"""
    for cxx, static in (("/opt/rocm/llvm/bin/clang++", ["-static-libsan"]), ("clang++", ["-static-libsan"]), ("g++", ["-static-libasan", "-static-libubsan"])):
        p = shutil.which(cxx) or (cxx if os.path.exists(cxx) else None)
        if p:
            return p, static
    raise RuntimeError("no host C++ compiler")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """Compile tests/pngdec_host_main.cpp with the sanitizers, write the corpus, run the program once: name -> dict of its printed fields."""
    d = tmp_path_factory.mktemp("pngdec")
    exe = str(d / "pngdec_host_main")
    cxx, static = _compiler()
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static,
                    os.path.join(ROOT, "tests", "pngdec_host_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    corpus = d / "corpus"
    corpus.mkdir()
    lines = []
    for name, (z, raw, _) in I.good_streams().items():
        (corpus / name).write_bytes(z)
        c = pngdec.list_candidates(z)
        dims = " 48 64 3" if name.endswith("_photo") else ""
        lines.append(f"{name} {len(raw)}{dims}" + (" c " + " ".join(str(o) for o in [2] + c) if c else ""))
    for name, (z, n) in I.damaged_streams().items():
        (corpus / name).write_bytes(z)
        c = pngdec.list_candidates(z)
        lines.append(f"{name} {n}" + (" c " + " ".join(str(o) for o in [2] + c) if c else ""))
    (corpus / "manifest.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(corpus)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        out[f[0]] = {k: v for k, v in (x.split("=", 1) for x in f[1:])}
    assert len(out) == len(lines)
    return out


def test_core_good_streams_equal_zlib(host_run):
    for name, (z, raw, plan) in I.good_streams().items():
        assert zlib.decompress(z) == raw, name
        r = host_run[name]
        assert r["code"] == "0", (name, r)
        assert r["sha"] == hashlib.sha256(raw).hexdigest(), name
        assert r["plan"] == plan, (name, r)
        if plan == "segments":
            assert int(r["pieces"]) == (len(raw) + SEG - 1) // SEG, (name, r)


def test_core_unfilter_equals_reference(host_run):
    img = R.photo_like(48, 64, 3, seed=2)
    for level in (0, 1, 6, 9):
        assert host_run[f"zlib{level}_photo"]["pix"] == hashlib.sha256(img.tobytes()).hexdigest()


def test_core_damaged_streams_give_codes(host_run):
    d = I.damaged_streams()
    assert len(d) > 150
    for name in d:
        r = host_run[name]
        assert r["code"] != "0" and r["sha"] == "-", (name, r)
        assert r["plan"] == "serial", (name, r)          # no damaged chain is accepted
    assert host_run["bad_adler"]["code"] == "10"
    assert host_run["len_nlen_mismatch"]["code"] == "4"
    assert host_run["oversubscribed"]["code"] == "5"
    assert host_run["distance_before_start"]["code"] == "7"
    assert host_run["output_longer"]["code"] == "8" and host_run["output_longer_far"]["code"] == "8"
    assert host_run["output_shorter"]["code"] == "9"
    assert host_run["bad_zlib_header"]["code"] == "2" and host_run["preset_dictionary"]["code"] == "2"
    assert host_run["block_type_3"]["code"] == "3"
    assert host_run["empty"]["code"] == "1" and host_run["one_byte"]["code"] == "1"


def test_core_corpus_reaches_every_mechanism(host_run):
    g = {n: {k: int(v) for k, v in host_run[n].items() if v.lstrip("-").isdigit()} for n in I.good_streams()}
    assert any(r["stored"] > 0 for r in g.values()) and any(r["fixed"] > 0 for r in g.values()) and any(r["dynamic"] > 0 for r in g.values())
    assert g["zlib0_text"]["stored"] >= 2 and g["zlib0_text"]["dynamic"] == 0
    assert g["zlib_fixed"]["fixed"] >= 1 and g["zlib_fixed"]["dynamic"] == 0
    assert max(r["maxlen"] for r in g.values()) == 258 and g["dist32768"]["maxlen"] == 258
    assert g["dist32768"]["maxdist"] == 32768
    assert g["run_dist1"]["run1"] == 700 and g["enc_zeros"]["run1"] > 258
    assert g["zlib_fibonacci"]["maxcode"] == 15 and g["enc_fibonacci"]["maxcode"] > 10
    assert g["sync_flush"]["empty"] == 2 and g["empty_stored_first"]["empty"] == 1 and g["enc_seg3plus5"]["empty"] == 3
    assert len(I.good_streams()["enc_len1"][1]) == 1 and len(I.good_streams()["enc_len2"][1]) == 2
    assert g["zlib9_text"]["maxdist"] > 20000          # a far match that zlib found itself


def test_plan_logic_on_the_named_cases(host_run):
    g = I.good_streams()
    # the crossing Z_SYNC_FLUSH stream has a candidate, its second piece refers back before its own start: rejected
    assert len(pngdec.list_candidates(g["sync_flush_crossing"][0])) == 1 and host_run["sync_flush_crossing"]["plan"] == "serial"
    # the false candidate inside a stored payload: rejected
    assert host_run["stored_payload_marker"]["plan"] == "serial"
    # 3 x 32768 + 5 bytes from the encoder: 3 candidates, 4 pieces, accepted
    assert len(pngdec.list_candidates(g["enc_seg3plus5"][0])) == 3
    assert host_run["enc_seg3plus5"]["plan"] == "segments" and host_run["enc_seg3plus5"]["pieces"] == "4"
    # pieces that are decodable on their own but not of 32768 bytes each: rejected
    assert host_run["full_flush"]["plan"] == "serial" and host_run["sync_flush"]["plan"] == "serial"
    # a foreign stream that happens to have the encoder's structure is taken
    assert host_run["full_flush_32768"]["plan"] == "segments"
    for name in ("enc_noise", "enc_noise3", "enc_mixed", "enc_zeros", "enc_straddle1", "enc_straddle2", "enc_straddle3", "enc_len32769", "enc_len65539"):
        assert host_run[name]["plan"] == "segments", name


# ------------------------------------------------------------------------------------------------ the chain rule, restated on zlib
def _py_pieces(z, cands):
    """An independent piece table: zlib's own raw inflater, fresh (no window) at every candidate start, fed up to each later candidate until
    it has produced 32768 bytes there or met the final block within 32768 bytes.  start -> (end, bytes, final) of the usable pieces."""
    table, stops = {}, sorted(set(cands) | {len(z)})
    for s in cands:
        d, out, prev = zlib.decompressobj(-15), b"", s
        try:
            for c in (c for c in stops if c > s):
                out += d.decompress(z[prev:c])
                prev = c
                if d.eof:
                    if len(out) <= SEG:          # (a piece has a slot of 32768 bytes)
                        table[s] = (c - len(d.unused_data), out, True)
                    break
                if len(out) >= SEG:
                    if len(out) == SEG:
                        table[s] = (c, out, False)
                    break
        except zlib.error:          # a reference before the piece's own start, or no deflate data at all
            pass
    return table


def _py_chain_accepts(z, expect):
    """every piece usable, every piece but the last of 32768 bytes, every end a candidate, at least two pieces, total and Adler-32 right"""
    cands = [2] + pngdec.list_candidates(z)
    if len(cands) < 2 or z[:2] != b"\x78\x01" and (z[0] & 15 != 8 or ((z[0] << 8) | z[1]) % 31):
        return False
    table, off, out, k = _py_pieces(z, cands), 2, b"", 0
    while off in table:
        end, data, final = table[off]
        out, k, off = out + data, k + 1, end
        if final:
            return k >= 2 and len(out) == expect and z[end:end + 4] == struct.pack(">I", zlib.adler32(out) & 0xFFFFFFFF)
    return False


def test_chain_rule_against_zlib_reference(host_run):
    """The plan the shared C++ chain takes equals what the rule gives on a piece table made by zlib itself, for every stream of both corpora."""
    for name, (z, raw, plan) in I.good_streams().items():
        assert _py_chain_accepts(z, len(raw)) == (plan == "segments") == (host_run[name]["plan"] == "segments"), name
    for name, (z, n) in I.damaged_streams().items():
        assert not _py_chain_accepts(z, n) and host_run[name]["plan"] == "serial", name
    g = I.good_streams()
    assert not _py_chain_accepts(g["sync_flush_crossing"][0], 2 * SEG) and not _py_chain_accepts(g["stored_payload_marker"][0], len(g["stored_payload_marker"][1]))
    assert _py_chain_accepts(g["enc_seg3plus5"][0], 3 * SEG + 5) and len(pngdec.list_candidates(g["enc_seg3plus5"][0])) == 3
