"""The perceptual distance on the GPU (reface_amd/csrc/lpips.hip, reface_amd/lpips.py, eval_tool/lpips/) against the reference's own outputs
(tests/golden/lpips.npz) and the host restatements that tests/test_lpips_cpu.py pins to them.

Gates.  GATE = 2e-5 relative is the project's fp32 limit for side kernels; the fixture's e_ref (the reference's own
fp32 evaluation against float64 over the ordinary v[b, l]) must satisfy 4 x e_ref <= GATE, so the gate is never tighter than the reference's
own rounding noise.  Near-identical pairs (y = x with six bytes moved by one) are held within 4 x e_ref_near, the margin the pose and
expression tests use over the reference's own fp32 - float64 distance.  Every output is a slice of a NaN-filled buffer whose guards must
stay NaN; every test prints its figure before it asserts (DESIGN.md section 8 keeps the record)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_inputs as I  # noqa: E402

from reface_amd import lpips as LP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GATE = 2e-5
GUARD = 64          # elements on either side of an output: a multiple of 16 bytes for every dtype used
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lpips.npz"))


@pytest.fixture(scope="module")
def scorers():
    return {net: LP.LPIPSScorer(LP.load_lpips_state("none", net), net=net, batch=4, device=DEV) for net in ("alex", "vgg")}


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _rel(a, b):
    return float((np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))).max())


# ---- prep ------------------------------------------------------------------------------------------------------------------------------
def _zscore_cpu(x):
    """BaseNet.z_score on torch CPU fp32, each step rounded on its own."""
    mean = torch.tensor(LP.MEAN, dtype=F32).view(1, 3, 1, 1)
    std = torch.tensor(LP.STD, dtype=F32).view(1, 3, 1, 1)
    return (x - mean) / std


def _all_bytes(B, H, W):
    """uint8 [B, H, W, 3] in which every channel of every image of >= 256 pixels holds all 256 byte values."""
    i = torch.arange(B * H * W * 3, dtype=torch.int64).view(B, H, W, 3)
    p = torch.arange(H * W, dtype=torch.int64).view(1, H, W, 1)
    c = torch.arange(3, dtype=torch.int64).view(1, 1, 1, 3)
    return ((p * (2 * c + 1) + 37 * c + 11 * (i // (H * W * 3))) % 256).to(torch.uint8)


@pytest.mark.parametrize("hw", [(64, 64), (35, 33), (1, 1)])
def test_prep_u8_bit_for_bit(hw):
    """rf_lpips_prep_u8 against torch CPU fp32 doing the same steps in the same order; packed and strided batches."""
    from reface_amd import ops
    H, W = hw
    B = 3
    img = _all_bytes(B, H + 2, W)          # two rows more per image: the strided batch below is its first H rows
    if H * W >= 256:
        assert all(len(torch.unique(img[b, :H, :, c])) == 256 for b in range(B) for c in range(3))
    for strided in (False, True):
        src = img.to(DEV)[:, :H] if strided else img[:, :H].contiguous().to(DEV)
        assert (src.stride(0) == (H + 2) * W * 3) == strided
        x = img[:, :H].permute(0, 3, 1, 2).to(F32)
        x = x / 255
        x = (x - 0.5) / 0.5
        want = _zscore_cpu(x).permute(0, 2, 3, 1).numpy()
        buf, out = _guarded((B, H, W, 8), F32)
        ops.lpips_prep_u8(src, out)()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert _intact(buf)
        assert np.array_equal(_bits(got[..., :3]), _bits(want)), float(np.abs(got[..., :3] - want).max())
        assert np.array_equal(_bits(got[..., 3:]), np.zeros((B, H, W, 5), dtype=np.uint32))          # exactly +0 (the buffer was NaN)


@pytest.mark.parametrize("hw", [(64, 64), (35, 33), (1, 1)])
def test_prep_f32_bit_for_bit(hw):
    from reface_amd import ops
    from reface_amd.params import seeded_randn
    H, W = hw
    x = seeded_randn((2, 3, H, W), 640 + H).clamp(-1, 1)
    x[0, :, 0, 0] = torch.tensor([-1.0, 0.0, 1.0])
    want = _zscore_cpu(x).permute(0, 2, 3, 1).numpy()
    buf, out = _guarded((2, H, W, 8), F32)
    ops.lpips_prep_f32(x.to(DEV), out)()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _intact(buf)
    assert np.array_equal(_bits(got[..., :3]), _bits(want)) and not got[..., 3:].any()


# ---- pools -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,hw", [(3, (15, 15)), (3, (16, 14)), (3, (8, 7)), (3, (3, 3)), (2, (70, 61)), (2, (35, 33)), (2, (2, 2))])
def test_maxpool2d_bit_for_bit(k, hw):
    """rf_maxpool2d against F.max_pool2d(k, 2) (no padding, floor mode) on negative and positive values: C = 64 and 192, B = 1 and 3."""
    from reface_amd import ops
    from reface_amd.params import seeded_randn
    H, W = hw
    for C in (64, 192):
        for B in (1, 3):
            x = seeded_randn((B, H, W, C), 650 + 7 * H + W + C + B)
            assert float(x.min()) < 0 < float(x.max())
            want = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), k, 2).permute(0, 2, 3, 1).contiguous().numpy()
            assert want.shape == (B, (H - k) // 2 + 1, (W - k) // 2 + 1, C)
            buf, out = _guarded(want.shape, F32)
            ops.maxpool2d(x.to(DEV), out, k=k)()
            torch.cuda.synchronize()
            assert _intact(buf)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (k, hw, C, B)


# ---- rf_lpips_layer ----------------------------------------------------------------------------------------------------------------------
def _layer(fx, fy, w, L=5, l=2):
    """vals[:, l] of rf_lpips_layer on host tensors [B, HW, C]; the other columns, the scratch's and the output's guards must stay NaN."""
    from reface_amd import ops
    B, HW, C = fx.shape
    vbuf, vals = _guarded((B, L), F64)
    sbuf, scratch = _guarded((B * min(ops.LPIPS_MAX_BLOCKS, HW),), F64)
    ops.lpips_layer(fx.to(DEV), fy.to(DEV), w.to(DEV), scratch, vals, l)()
    torch.cuda.synchronize()
    v = vals.cpu().numpy()
    assert _intact(vbuf) and _intact(sbuf)
    assert np.isnan(np.delete(v, l, axis=1)).all()
    return v[:, l]


def _layer_host(fx, fy, w):
    """float64 on the same inputs (LP.lpips_host takes NCHW)."""
    nchw = lambda f: f.permute(0, 2, 1)[..., None]
    return LP.lpips_host([nchw(fx)], [nchw(fy)], [w])[:, 0]


LAYER_SHAPES = [(1, 1, 64), (2, 225, 64), (3, 42, 192), (2, 6, 384), (2, 3, 256), (1, 4270, 64), (2, 17, 512), (1, 5, 4)]


@pytest.mark.parametrize("B,HW,C", LAYER_SHAPES, ids=[f"{b}x{p}x{c}" for b, p, c in LAYER_SHAPES])
def test_lpips_layer_vs_float64(B, HW, C):
    """Post-ReLU-like inputs (about half zeros), three images generated per shape and run at B, 1 and 3, every input within GATE of float64:
      * independent y, with an all-zero pixel in x only, in y only and in both (HW >= 3): finite;
      * y = x + 1e-3 noise at EVERY shape, from an x without all-zero pixels, so that the value is the small difference itself (about 1e-6)
        and an evaluation that cancels -- the expanded five-sum form in fp32 -- misses the gate by orders of magnitude;
      * y = x: exactly 0.0;
      * image 0 has the same bits at B = 1 and B = 3."""
    from reface_amd.params import seeded_randn
    x = torch.relu(seeded_randn((3, HW, C), 660 + HW + C))
    fy = torch.relu(seeded_randn((3, HW, C), 661 + HW + C))
    w = seeded_randn((C,), 662 + C).abs()
    assert 0.3 < float((x == 0).float().mean()) < 0.7 and 0.3 < float((fy == 0).float().mean()) < 0.7
    x[..., 0] = torch.where(x.sum(dim=2) == 0, torch.ones(()), x[..., 0])          # no pixel of x is all zero (at C = 4 one in sixteen would be)
    assert float(x.abs().sum(dim=2).min()) > 0
    near = torch.relu(x + 1e-3 * seeded_randn((3, HW, C), 663 + HW + C))
    fx = x.clone()
    if HW >= 3:
        fx[:, 0] = 0
        fy[:, 1] = 0
        fx[:, 2] = 0
        fy[:, 2] = 0
    worst = 0.0
    runs = {}
    for name, a, y in (("independent", fx, fy), ("near", x, near), ("same", fx, fx.clone())):
        want = _layer_host(a, y, w)
        if name == "near":
            assert want.max() < 1e-4, want          # the small difference, nothing else
        for b in sorted({B, 1, 3}):
            got = _layer(a[:b].contiguous(), y[:b].contiguous(), w)
            runs[(name, b)] = got
            assert got.dtype == np.float64 and np.isfinite(got).all()
            if name == "same":
                assert np.array_equal(_bits(got), np.zeros(b, dtype=np.uint64)), got          # exactly +0.0
            else:
                err = _rel(got, want[:b])
                worst = max(worst, err)
                print(f"lpips layer B={b} HW={HW} C={C} {name}: v[0] = {want[0]:.3e}, max rel |kernel - fp64| = {err:.2e}")
        assert np.array_equal(_bits(runs[(name, 1)][:1]), _bits(runs[(name, 3)][:1]))
    print(f"lpips layer HW={HW} C={C}: worst err / limit = {worst:.2e} / {GATE:.0e} = {worst / GATE:.3f}")
    assert worst <= GATE


def test_lpips_layer_refuses_bad_arguments():
    from reface_amd import _lib, ops
    z = lambda *s: torch.zeros(s, dtype=F32, device=DEV)
    d = lambda *s: torch.zeros(s, dtype=F64, device=DEV)
    with pytest.raises(_lib.RefaceHipError, match="multiple of 4 in 4..512"):
        ops.lpips_layer(z(1, 2, 516), z(1, 2, 516), z(516), d(8), d(1, 5), 0)()
    with pytest.raises(_lib.RefaceHipError, match="multiple of 4 in 4..512"):
        ops.lpips_layer(z(1, 2, 6), z(1, 2, 6), z(6), d(8), d(1, 5), 0)()
    with pytest.raises(_lib.RefaceHipError, match="layer 5 of 5"):
        ops.lpips_layer(z(1, 2, 8), z(1, 2, 8), z(8), d(8), d(1, 5), 5)()
    with pytest.raises(_lib.RefaceHipError, match="scratch"):
        ops.lpips_layer(z(2, 300, 8), z(2, 300, 8), z(8), d(4), d(2, 5), 0)()          # 2 pairs x 3 blocks of 128 pixels
    with pytest.raises(_lib.RefaceHipError, match="window 4"):
        ops.maxpool2d(z(1, 8, 8, 4), z(1, 3, 3, 4), k=4)()
    lib = _lib.load()
    assert lib.rf_maxpool2d(z(1, 2, 8, 4).data_ptr(), 1, 2, 8, 4, 3, z(4).data_ptr(), None) != 0 and b"bad sizes" in lib.rf_last_error()          # H < k
    assert lib.rf_maxpool2d(z(1, 8, 8, 6).data_ptr(), 1, 8, 8, 6, 3, z(4).data_ptr(), None) != 0 and b"multiple of 4" in lib.rf_last_error()
    assert lib.rf_lpips_layer(None, None, 1, 1, 4, None, None, 0, None, 5, 0, None) != 0 and b"null" in lib.rf_last_error()
    assert lib.rf_lpips_total(None, 1, 5, None, None, None) != 0 and b"null" in lib.rf_last_error()
    assert lib.rf_lpips_total(d(1, 5).data_ptr(), 0, 5, d(1).data_ptr(), d(2).data_ptr(), None) != 0 and b"bad sizes" in lib.rf_last_error()
    assert lib.rf_lpips_prep_u8(None, 1, 1, 1, 3, None, None) != 0 and b"null" in lib.rf_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,L", [(1, 5), (300, 5), (7, 3)])
def test_lpips_total_vs_numpy(B, L):
    from reface_amd import ops
    from reface_amd.params import seeded_randn
    vals = seeded_randn((B, L), 670 + B).double().abs() * 1e-2
    want = LP.score_host(vals.numpy())
    outs = []
    for _ in range(2):
        dbuf, d = _guarded((B,), F64)
        tbuf, totals = _guarded((2,), F64)
        ops.lpips_total(vals.to(DEV), d, totals)()
        torch.cuda.synchronize()
        assert _intact(dbuf) and _intact(tbuf)
        outs.append((d.cpu().numpy(), totals.cpu().numpy()))
    (d0, t0), (d1, t1) = outs
    assert np.array_equal(_bits(d0), _bits(d1)) and np.array_equal(_bits(t0), _bits(t1))
    assert np.array_equal(_bits(d0), _bits(want["distances"]))          # the layers summed in order: the same float64 additions
    assert t0[1] == B and abs(t0[0] / B / want["lpips_value"] - 1.0) <= 1e-14
    s = 0.0
    for b in range(B):
        s += float(d0[b])
    assert t0[0] == s          # index order


# ---- engine ------------------------------------------------------------------------------------------------------------------------------
def _u8(images):
    return [torch.from_numpy(im) for im in images]


@pytest.mark.parametrize("case", range(len(I.CASES)), ids=[I.case_name(c) for c in range(len(I.CASES))])
def test_engine_vs_reference(case, golden, scorers):
    """prep + feature stack + five rf_lpips_layer + rf_lpips_total on the fixture's pairs against the reference module in float64."""
    net = I.CASES[case][0]
    n = I.case_name(case)
    e_ref, e_near = float(golden["e_ref"]), float(golden["e_ref_near"])
    assert 4 * e_ref <= GATE
    xs, ys = I.build_case(case)
    r = scorers[net].distances_u8(_u8(xs), _u8(ys))
    d, v = r.d.cpu().numpy(), r.layers.cpu().numpy()
    assert v.shape == (I.PAIRS, 5) and np.isfinite(v).all()
    v64, d64 = golden[f"v_f64_{n}"], golden[f"d_f64_{n}"]
    ordinary = [k for k in range(I.PAIRS) if k != I.NEAR]
    e_v, e_d = _rel(v[ordinary], v64[ordinary]), _rel(d[ordinary], d64[ordinary])
    e_s = abs(float(d.mean()) / float(golden[f"scalar_f64_{n}"]) - 1.0)
    e_nv, e_nd = _rel(v[I.NEAR], v64[I.NEAR]), _rel(d[I.NEAR], d64[I.NEAR])
    print(f"lpips engine {n}: ordinary rel |GPU - reference fp64|: v {e_v:.2e}, d {e_d:.2e}, scalar {e_s:.2e}; worst err / limit = {max(e_v, e_d, e_s) / GATE:.3f} "
          f"(reference fp32: e_ref {e_ref:.2e})")
    print(f"lpips engine {n}: near-identical pair: v {e_nv:.2e}, d {e_nd:.2e}; err / (4 x e_ref_near = {4 * e_near:.2e}) = {max(e_nv, e_nd) / (4 * e_near):.3f}")
    assert max(e_v, e_d, e_s) <= GATE
    assert max(e_nv, e_nd) <= 4 * e_near


def test_engine_zero_and_batch_invariance(scorers):
    """LPIPS(x, x) is exactly 0.0; a pair's d has the same bits alone and among four (no split-K, a batch-independent rf_lpips_layer grid)."""
    for case in (1, 4):
        net = I.CASES[case][0]
        xs, ys = I.build_case(case)
        same = scorers[net].distances_u8(_u8(xs), _u8(xs)).d.cpu().numpy()
        assert np.array_equal(_bits(same), np.zeros(I.PAIRS, dtype=np.uint64)), same
        d4, v4, _ = scorers[net].distances_u8(_u8(xs), _u8(ys))
        for k in (0, 2, 3):
            d1, v1, _ = scorers[net].distances_u8(_u8(xs[k:k + 1]), _u8(ys[k:k + 1]))
            assert np.array_equal(_bits(v1.cpu().numpy()[0]), _bits(v4.cpu().numpy()[k])), (net, k)
            assert np.array_equal(_bits(d1.cpu().numpy()), _bits(d4.cpu().numpy()[k:k + 1]))
        # the two images of a pair may be swapped: (a - b)^2 == (b - a)^2 bit for bit
        assert np.array_equal(_bits(scorers[net].distances_u8(_u8(ys), _u8(xs)).d.cpu().numpy()), _bits(d4.cpu().numpy()))


def test_mixed_sizes_and_refusals(scorers):
    """Runs of consecutive pairs of equal size share an engine; stacked device tensors and host lists agree; a pair of unequal sizes and an
    image below the net's minimum are refused before any launch."""
    s = scorers["alex"]
    xa, ya = I.build_case(0)
    xb, yb = I.build_case(1)
    xs, ys = xa[:2] + xb[:3] + xa[2:3], ya[:2] + yb[:3] + ya[2:3]
    d = s.distances_u8(_u8(xs), _u8(ys)).d.cpu().numpy()
    da = s.distances_u8(torch.from_numpy(np.stack(xa)).to(DEV), torch.from_numpy(np.stack(ya)).to(DEV)).d.cpu().numpy()
    db = s.distances_u8(_u8(xb), _u8(yb)).d.cpu().numpy()
    assert np.array_equal(_bits(d), _bits(np.concatenate([da[:2], db[:3], da[2:3]])))
    with pytest.raises(ValueError, match="pair 1"):
        s.distances_u8(_u8(xa[:1] + xb[:1]), _u8(ya[:1] + ya[:1]))
    small = [torch.zeros((30, 40, 3), dtype=torch.uint8)]
    with pytest.raises(ValueError, match="at least 31 x 31"):
        s.distances_u8(small, small)
    with pytest.raises(ValueError, match="at least 16 x 16"):
        scorers["vgg"].distances(torch.zeros(1, 3, 15, 20, device=DEV), torch.zeros(1, 3, 15, 20, device=DEV))


def test_engine_cache_is_bounded():
    """A scorer keeps the MAX_ENGINES most recently used engines: many sizes do not pile up their activation pools; values do not change."""
    s = LP.LPIPSScorer(LP.load_lpips_state("none", "alex"), net="alex", batch=2, device=DEV)
    xs, ys = I.build_case(0)
    first = s.distances_u8(_u8(xs[:1]), _u8(ys[:1])).d.cpu().numpy()
    for cut in range(1, LP.MAX_ENGINES + 3):
        s.distances_u8(_u8([im[:64 - cut] for im in xs[:2]]), _u8([im[:64 - cut] for im in ys[:2]]))
        assert len(s._engines) <= LP.MAX_ENGINES
    assert (1, 64, 64) not in s._engines
    assert np.array_equal(_bits(s.distances_u8(_u8(xs[:1]), _u8(ys[:1])).d.cpu().numpy()), _bits(first))


@pytest.mark.parametrize("net,size", [("alex", 512), ("vgg", 128)])
def test_full_size_vs_float64(net, size, scorers):
    """Tile choice is size-driven: one pair at a full size against lpips_host in float64 on the same inputs, under the same gate."""
    from idscore_inputs import _field, _render
    f = _field(7950 + size)
    x = _render(f, (size, size))
    y = _render(0.7 * f + 0.3 * _field(7951 + size), (size, size))
    sd = LP.load_lpips_state("none", net)
    want = LP.distances_host(sd, torch.from_numpy(LP.prep_host(x))[None], torch.from_numpy(LP.prep_host(y))[None], net)
    d, v, _ = scorers[net].distances_u8(_u8([x]), _u8([y]))
    e_v = _rel(v.cpu().numpy(), want)
    e_d = _rel(d.cpu().numpy(), LP.score_host(want)["distances"])
    print(f"lpips {net} {size} x {size}: d = {float(d[0]):.6f}; rel |GPU - fp64 host|: v {e_v:.2e}, d {e_d:.2e}; worst err / limit = {max(e_v, e_d) / GATE:.3f}")
    assert max(e_v, e_d) <= GATE


# ---- the reference's surface and the CLI ---------------------------------------------------------------------------------------------------
def test_module_surface(golden, scorers):
    from eval_tool.lpips.lpips import LPIPS
    from reface_amd._lib import RefaceHipError
    m = LPIPS("alex")
    m.load_state_dict(LP.load_lpips_state("none", "alex"), strict=True)
    xs, ys = I.build_case(0)
    x = torch.from_numpy(np.stack([LP.prep_host(im) for im in xs])).to(DEV)
    y = torch.from_numpy(np.stack([LP.prep_host(im) for im in ys])).to(DEV)
    out = m(x, y)
    assert out.dim() == 0 and out.dtype == F32 and out.is_cuda
    d = scorers["alex"].distances_u8(_u8(xs), _u8(ys)).d.cpu().numpy()          # the bytes through rf_lpips_prep_u8: the same prepared input
    s = 0.0
    for k in range(I.PAIRS):
        s += float(d[k])
    assert float(out) == float(np.float32(s / I.PAIRS))
    assert abs(float(out) / float(golden["scalar_f64_alex_64x64"]) - 1.0) <= GATE
    assert float(m(x, x)) == 0.0
    # the packed weights follow the module's parameters: an in-place write is seen by the next call
    before = float(out)
    with torch.no_grad():
        m.lin[0]["1"].weight.mul_(2.0)
    doubled = float(m(x, y))
    v = scorers["alex"].distances_u8(_u8(xs), _u8(ys)).layers.cpu().numpy()
    assert abs(doubled / float((v.sum() + v[:, 0].sum()) / I.PAIRS) - 1.0) <= 1e-6 and doubled > before
    m.double()
    assert abs(float(m(x, y)) / doubled - 1.0) <= 1e-6          # (the engines take the weights as fp32 whatever the module holds)
    with pytest.raises(RefaceHipError, match="no CPU fallback"):
        m(x.cpu(), y.cpu())
    with pytest.raises(ValueError, match="equal shape"):
        m(x, y[:, :, :60])
    with pytest.raises(NotImplementedError, match="squeeze"):
        LPIPS("squeeze")
    assert float(LPIPS("vgg", ckpt="none")(x[:1], x[:1])) == 0.0


def test_cli_end_to_end(tmp_path, golden):
    """PNG folders -> the printed value, in a fresh process.  Labels equal the fixture's; every distance and LPIPS_value within the engine
    gate of the reference's float64 ones (pairing by position would move the value five-fold).  A result whose size differs from its
    target's is refused by name."""
    data = I.build_folders()
    paths = I.write_folders(str(tmp_path / "folders"), data)
    out_json = str(tmp_path / "lpips.json")
    cmd = [sys.executable, os.path.join(ROOT, "eval_tool", "lpips", "lpips_compare.py"), "--device", "cuda"] + paths + [
        "--lpips_ckpt", "none", "--batch-size", "2", "--num-workers", "2", "--net", "alex", "--print_sim", "True", "--json", out_json]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    r = json.load(open(out_json))
    assert "LPIPS_value:  {}".format(r["lpips_value"]) in lines          # print('LPIPS_value: ', v): two spaces
    assert ["{} : {}".format(i, v) for i, v in enumerate(r["distances"])] == lines[-len(r["distances"]):]
    assert r["labels"] == golden["labels"].tolist() and r["images"] == 12 and r["images_per_s"] > 0 and r["net"] == "alex"
    e_d = _rel(r["distances"], golden["folder_d_f64"])
    e_v = abs(r["lpips_value"] / float(golden["folder_value_f64"]) - 1.0)
    print(f"lpips CLI: rel |distance - reference| = {e_d:.2e}, rel |LPIPS_value - reference| = {e_v:.2e} (gate {GATE:.0e})")
    assert max(e_d, e_v) <= GATE
    # a result of another size than its target
    from PIL import Image
    victim = os.path.join(paths[1], data["res_names"][2])
    Image.fromarray(data["res_images"][2][:60]).save(victim)
    sys.path.insert(0, os.path.join(ROOT, "eval_tool", "lpips"))
    import lpips_compare as cli
    with pytest.raises(SystemExit, match=data["res_names"][2]):
        cli.main(paths + ["--lpips_ckpt", "none", "--num-workers", "0"])
