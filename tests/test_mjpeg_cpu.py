"""The numpy restatement of the GPU JPEG encoder (tests/jpeg_refs.py) and ``reface_amd.mjpeg.jpeg_header`` held to PIL's (libjpeg's) file,
byte for byte; the AVI writer read back by an independent RIFF parser; the ordered sink; the CLI's refusals; the exports."""
import io
import os
import sys
import threading
import time

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_refs as R  # noqa: E402

from reface_amd import mjpeg as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the model and the header against PIL
@pytest.mark.parametrize("subsampling", M.SUBSAMPLINGS)
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_equals_pil(size, subsampling):
    H, W = size
    for quality in R.QUALITIES:
        head = M.jpeg_header(H, W, quality, subsampling)
        for kind in R.KINDS:
            img = R.image(kind, H, W)
            want = R.pil_jpeg(img, quality, subsampling)
            assert want[:len(head)] == head, (quality, kind)          # the tables, the geometry and DRI = MCUs per row
            assert R.encode(img, quality, subsampling) == want, (quality, kind)
            assert Image.open(io.BytesIO(want)).size == (W, H)


def test_restart_markers_wrap():
    """160 x 32: 10 intervals at 4:2:0, 20 at 4:4:4 -- RST7 is followed by RST0."""
    for subsampling, n in (("420", 10), ("444", 20)):
        parts = R.intervals(R.model_coefficients("noise", 160, 32, 75, subsampling), subsampling)
        assert len(parts) == n
        scan = R.pack(parts)
        p = 0
        for i, part in enumerate(parts[:-1]):
            p += len(part)
            assert scan[p:p + 2] == bytes([0xFF, 0xD0 + i % 8])
            p += 2
        assert scan.endswith(b"\xff\xd9") and any(scan[k:k + 2] == b"\xff\xd0" for k in range(len(parts[0]) + 2, len(scan)))


def test_hard_cases_are_hard():
    """Noise at Q = 100 stuffs bytes; the smooth image at Q = 30 has ZRL symbols and blocks that are an EOB alone: the cases the GPU tests
    lean on really hold them."""
    stats = {}
    R.encode(R.image("noise", 48, 80), 100, "444", stats)
    assert stats["stuffed"] > 0
    stats = {}
    R.encode(R.image("smooth", 100, 36), 30, "420", stats)
    assert stats.get("zrl", 0) > 0 and stats.get("eob_only", 0) > 0


def test_rgba_is_convert_rgb():
    rgba = np.concatenate([R.image("smooth", 33, 47), R.image("noise", 33, 47)[..., :1]], axis=2)
    assert R.encode(rgba, 90, "420") == R.pil_jpeg(rgba, 90, "420")          # (pil_jpeg converts to RGB: the alpha byte is dropped)


def test_quality_and_geometry_refusals():
    for bad in (0, 101):
        with pytest.raises(ValueError):
            M.quant_tables(bad)
    with pytest.raises(ValueError):
        M.jpeg_header(8, 8, 90, "422")
    with pytest.raises(ValueError):
        M.jpeg_header(0, 8, 90, "420")
    with pytest.raises(ValueError):
        M.jpeg_header(8, 65536, 90, "420")
    assert M.quant_tables(100) == ((1,) * 64, (1,) * 64) and max(M.quant_tables(1)[0]) == 255
    assert M.BLOCK_BITS >= 22 + 63 * 26


# ------------------------------------------------------------------------------------------------ the container
def _five_jpegs(W=48, H=32):
    """PIL-made frames of odd and even byte lengths."""
    out = []
    for k in range(5):
        buf = io.BytesIO()
        Image.fromarray(R.image("smooth" if k % 2 else "noise", H, W)).save(buf, "JPEG", quality=40 + 10 * k)
        data = buf.getvalue()
        out.append(data)
    want_odd = [0, 1, 0, 1, 1]
    for k, odd in enumerate(want_odd):          # a comment segment of 2 or 3 bytes behind SOI sets the parity without touching the image
        if len(out[k]) % 2 != odd:
            out[k] = out[k][:2] + b"\xff\xfe\x00\x03x" + out[k][2:]
    assert [len(d) % 2 for d in out] == want_odd
    return out


@pytest.mark.parametrize("fps,rate_scale", [(25, (25000, 1000)), (29.97, (29970, 1000))])
def test_avi_writer(tmp_path, fps, rate_scale):
    frames = _five_jpegs()
    w = M.AviWriter(tmp_path / "v.avi", 48, 32, fps)
    for f in frames:
        w.add(f)
    assert w.close() == [(str(tmp_path / "v.avi"), 5)]
    assert w.close() == [(str(tmp_path / "v.avi"), 5)]
    data = open(tmp_path / "v.avi", "rb").read()
    a = R.parse_avi(data)          # (asserts the RIFF / LIST sizes, the even alignment and the idx1 offsets)
    assert a["frames"] == frames
    assert a["total_frames"] == a["length"] == 5 and a["streams"] == 1 and a["flags"] & M.AVIF_HASINDEX
    assert (a["width"], a["height"], a["bi_width"], a["bi_height"]) == (48, 32, 48, 32)
    assert a["fcc_type"] == b"vids" and a["handler"] == b"MJPG" and a["bi_compression"] == b"MJPG" and a["bi_bits"] == 24 and a["bi_size"] == 40
    assert (a["rate"], a["scale"]) == rate_scale and a["rate"] * 1000 == round(fps * 1000) * a["scale"]
    assert a["usec_per_frame"] == round(1e6 / fps)
    for f in a["frames"]:
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (48, 32)
    with pytest.raises(ValueError):
        w.add(frames[0])


def test_avi_rollover(tmp_path):
    frames = _five_jpegs()
    two = max(len(frames[0]) + len(frames[1]), len(frames[2]) + len(frames[3]))
    overhead = len(open(_one_frame_file(tmp_path, frames[0]), "rb").read()) - len(frames[0])
    w = M.AviWriter(tmp_path / "r.avi", 48, 32, 25, max_bytes=two + overhead + 48)          # room for two frames, not for three
    for f in frames:
        w.add(f)
    files = w.close()
    assert files == [(str(tmp_path / "r.avi"), 2), (str(tmp_path / "r.002.avi"), 2), (str(tmp_path / "r.003.avi"), 1)]
    got = []
    for path, n in files:
        data = open(path, "rb").read()
        assert len(data) <= two + overhead + 48
        a = R.parse_avi(data)
        assert a["total_frames"] == a["length"] == n == len(a["frames"])
        got += a["frames"]
    assert got == frames


def _one_frame_file(tmp_path, frame):
    w = M.AviWriter(tmp_path / "one.avi", 48, 32, 25)
    w.add(frame)
    return w.close()[0][0]


# ------------------------------------------------------------------------------------------------ the ordered sink
class _FakeJob:
    """A job whose ``result()`` is ready after `ready` is set: the test sets them out of order."""

    def __init__(self, frames, error=None):
        self.frames, self.error, self.ready, self.discarded = frames, error, threading.Event(), False

    def result(self):
        assert self.ready.wait(10)
        if self.error is not None:
            raise self.error
        return self.frames

    def discard(self):
        self.discarded = True


def test_sink_keeps_submission_order():
    got = []
    sink = M.VideoSink(got.append, depth=8)
    jobs = [_FakeJob([f"{k}a".encode(), f"{k}b".encode()]) for k in range(4)]
    for j in jobs:
        sink.submit(j)
    for k in (3, 1, 2, 0):          # the encodes finish out of order
        jobs[k].ready.set()
        time.sleep(0.01)
    assert sink.close() == 8
    assert got == [b"0a", b"0b", b"1a", b"1b", b"2a", b"2b", b"3a", b"3b"]
    with pytest.raises(ValueError):
        sink.submit(jobs[0])


def test_sink_error_resurfaces_on_close():
    got = []
    sink = M.VideoSink(got.append, depth=2)
    jobs = [_FakeJob([b"0"]), _FakeJob([b"1"], error=RuntimeError("encode failed")), _FakeJob([b"2"]), _FakeJob([b"3"])]
    for j in jobs:
        j.ready.set()
    for j in jobs:
        sink.submit(j)          # (never blocks for good: the thread keeps draining after the error)
    with pytest.raises(RuntimeError, match="encode failed"):
        sink.close()
    assert got == [b"0"] and jobs[2].discarded and jobs[3].discarded


# ------------------------------------------------------------------------------------------------ the CLI's refusals, the exports
def test_cli_refusals(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import inference_swap_video as V
    with pytest.raises(SystemExit, match="--write_video .* needs --paste_back or --stream"):
        V.main(["--write_video"])
    with pytest.raises(SystemExit, match="--write_video .* needs --paste_back or --stream"):
        V.main(["--write_video", "out.avi", "--align"])
    for q in ("0", "101"):
        with pytest.raises(SystemExit, match="--video_quality is libjpeg's 1 .. 100"):
            V.main(["--paste_back", "--write_video", "--video_quality", q])
    with pytest.raises(SystemExit, match="--video_fps must be positive"):
        V.main(["--stream", "--write_video", "--video_fps", "0"])
    with pytest.raises(SystemExit):          # argparse: not one of 420 | 444
        V.main(["--stream", "--write_video", "--video_subsampling", "422"])
    capsys.readouterr()
    opt = V.build_parser().parse_args(["--stream", "--write_video"])
    assert opt.write_video == "" and opt.video_fps == 25 and opt.video_quality == 90 and opt.video_subsampling == "420"
    assert V.build_parser().parse_args([]).write_video is None


def test_exports():
    from reface_amd import _lib
    for name in ("rf_jpeg_blocks_u8", "rf_jpeg_entropy", "rf_jpeg_pack"):
        assert name in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 107 and all(hasattr(lib, n) for n in ("rf_jpeg_blocks_u8", "rf_jpeg_entropy", "rf_jpeg_pack"))
    header = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert "#define RF_JPEG_BLOCK_BITS (64 * 27)" in header and M.BLOCK_BITS == 64 * 27 and M.HUFF_WORDS == 2 * 272
