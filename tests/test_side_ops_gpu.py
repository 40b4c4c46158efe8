"""Op-level GPU tests of the encoder / sampler side kernels -- every export of encoder.hip, the glue kernels of elementwise.hip and
rf_softmax_rows -- against the plain fp64 references of tests/side_refs.py (pinned on the CPU by tests/test_side_ops_cpu.py), at the smallest
shapes at which each kernel can go wrong: odd sizes, pitched views, more than one block, every dtype pair and every optional argument.

Every output is a slice of a larger NaN-filled buffer: the guards on both sides must be untouched and no output element may still be NaN.
Tolerances (side_refs.limit*): fp32 outputs |got - ref| <= 2e-5 + 2e-5 |ref| (the file-level rule of test_ops_gpu.py; scale 0.1 / 0.01 for
the timestep embedding / softmax as there); 16-bit outputs one storage step on top, against the reference on the 16-bit-rounded inputs;
copies and single-operation kernels bit for bit.  Each test prints its worst err / limit ratio (DESIGN.md carries the table)."""
import math

import pytest
import torch

import side_refs as R
from reface_amd import _lib, ops
from reface_amd.params import seeded_randn as rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAD = 64                     # guard elements on each side of an output
WORST = {}                   # kernel -> worst err / limit seen in this run


def guarded(shape, dt):
    """(whole NaN-filled buffer, the output slice of it shaped `shape`)"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dt, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def fetch(buf, out):
    """after the launch: guards untouched, no sentinel left in the output -> the output on the host"""
    torch.cuda.synchronize()
    n = out.numel()
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all(), "wrote outside the output"
    assert not torch.isnan(out).any(), "output element not written"
    return out.cpu()


def record(kernel, got, ref, lim):
    err = (got.double() - ref).abs()
    assert torch.isfinite(got.double()).all()
    ratio = (err / lim).max().item()
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"[side_ops] {kernel}: worst err/limit {ratio:.4f}")
    assert ratio <= 1.0, f"{kernel}: err/limit {ratio:.3f} (max err {err.max().item():.3e})"


def name(kernel, out_dt):
    """the 16-bit-output forms report apart: their error is the storage rounding itself"""
    return kernel if out_dt == F32 else f"{kernel}->bf16"


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def dev(t):
    return None if t is None else t.to(DEV)


def test_step_table_is_the_ops_file_s():
    from test_ops_gpu import STEP
    assert R.STEP == STEP


# ------------------------------------------------------------------------------------------------ encoder.hip
@pytest.mark.parametrize("with_slope", [False, True])
@pytest.mark.parametrize("tin,tout", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
@pytest.mark.parametrize("case", R.CHANNEL_AFFINE_CASES, ids=lambda c: f"{c['M']}x{c['C']}")
def test_channel_affine(case, tin, tout, with_slope):
    i = R.channel_affine_inputs(case, rnd)
    C = case["C"]
    bufq = i["buf"].to(tin)
    x = bufq.to(DEV)[:, :C]                                    # pitched view (the 70-of-80 case); the output is packed
    slope = i["slope"] if with_slope else None
    buf, out = guarded((case["M"], C), tout)
    ops.channel_affine(x, dev(i["a"]), dev(i["b"]), out, slope=dev(slope))()
    got = fetch(buf, out)
    ref = R.channel_affine_ref(bufq[:, :C], i["a"], i["b"], slope)
    record(name("channel_affine", tout), got, ref, R.limit(ref, tout))
    assert (got[ref == 0] == 0).all() and (ref == 0).sum() >= 3          # x * a + b == 0 exactly stays 0 through the PReLU select


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", R.SPATIAL_MEAN_CASES, ids=lambda c: f"{c['B']}x{c['H'] * c['W']}x{c['C']}")
def test_spatial_mean(case, dt):
    bufq = R.spatial_mean_inputs(case, rnd)["buf"].to(dt)
    x = bufq.to(DEV)[..., :case["C"]]
    buf, out = guarded((case["B"], case["C"]), F32)
    ops.spatial_mean(x, out)()
    ref = R.spatial_mean_ref(bufq[..., :case["C"]])
    record("spatial_mean", fetch(buf, out), ref, R.limit_f32(ref))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", R.SE_SCALE_ADD_CASES, ids=lambda c: f"st{c['st']}-{c['Hs']}x{c['Ws']}-ld{c['pitch']}")
def test_se_scale_add(case, dt):
    i = R.se_scale_add_inputs(case, rnd)
    rq, bufq = i["r"].to(dt), i["buf"].to(dt)
    sc = bufq.to(DEV)[..., :R.SE_C]
    buf, out = guarded(tuple(rq.shape), dt)
    ops.se_scale_add(rq.to(DEV), dev(i["s"]), sc, out, stride=case["st"])()
    ref = R.se_scale_add_ref(rq, i["s"], bufq[..., :R.SE_C], case["st"])
    record(name("se_scale_add", dt), fetch(buf, out), ref, R.limit(ref, dt))


def _pool_id(c):
    return f"{c['Hf']}x{c['Wf']}-{c['Ho']}x{c['Wo']}{'-crop' if c['crop'] else ''}{'-affine' if c['affine'] else ''}" \
           f"-{'nhwc' if c['nhwc'] else 'nchw'}-{str(c['dt'])[6:]}"


@pytest.mark.parametrize("case", R.ADAPTIVE_AVGPOOL_CASES, ids=_pool_id)
def test_adaptive_avgpool(case):
    i = R.adaptive_avgpool_inputs(case, rnd)
    Ho, Wo, dt = case["Ho"], case["Wo"], case["dt"]
    shape = (R.POOL_B, Ho, Wo, case["Cpad"]) if case["nhwc"] else (R.POOL_B, R.POOL_C, Ho, Wo)
    buf, out = guarded(shape, dt)
    ops.adaptive_avgpool(dev(i["x"]), out, crop=case["crop"], a=dev(i["a"]), b=dev(i["b"]), nhwc=case["nhwc"])()
    got = fetch(buf, out)
    ref = R.adaptive_avgpool_ref(i["x"], Ho, Wo, crop=case["crop"], a=i["a"], b=i["b"], nhwc=case["nhwc"], Cpad=case.get("Cpad"))
    record(name("adaptive_avgpool", dt), got, ref, R.limit(ref, dt))
    if case["nhwc"]:
        assert (bits(got[..., R.POOL_C:]) == 0).all()          # the pad channels: exactly +0


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}x{c[3]}")
def test_bilinear_resize(case, affine):
    Hi, Wi, Ho, Wo = case
    i = R.bilinear_inputs(case, rnd)
    a, b = (i["a"], i["b"]) if affine else (None, None)
    buf, out = guarded((R.BILINEAR_B, R.BILINEAR_C, Ho, Wo), F32)
    ops.bilinear_resize(dev(i["x"]), out, a=dev(a), b=dev(b))()
    got = fetch(buf, out)
    ref = R.bilinear_resize_ref(i["x"], Ho, Wo, a, b)
    record("bilinear_resize", got, ref, R.limit_f32(ref))
    if (Hi, Wi) == (Ho, Wo) and not affine:
        assert torch.equal(got, i["x"])                        # the identity: weights 1 and 0


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", R.CLIP_TOKENS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_clip_tokens(case, dt):
    B, NP, C = case
    i = R.clip_tokens_inputs(case, rnd)
    pq = i["patch"].to(dt)
    buf, out = guarded((B, NP + 1, C), dt)
    ops.clip_tokens(pq.to(DEV), dev(i["cls"]), dev(i["pos"]), out)()
    got = fetch(buf, out)
    ref = R.clip_tokens_ref(pq, i["cls"], i["pos"])
    record(name("clip_tokens", dt), got, ref, R.limit(ref, dt))
    if dt == F32:                                              # one fp32 add per element: nothing to contract, so bit for bit torch's
        want = torch.cat([i["cls"].view(1, 1, C).expand(B, 1, C), pq], 1) + i["pos"][None]
        assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("case", R.L2NORM_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_l2norm_rows(case):
    x = R.l2norm_inputs(case, rnd)["x"]
    buf, out = guarded(tuple(x.shape), F32)
    ops.l2norm_rows(dev(x), out)()
    ref = R.l2norm_rows_ref(x)
    record("l2norm_rows", fetch(buf, out), ref, R.limit_f32(ref))


@pytest.mark.parametrize("n,form", R.COMBINE3_CASES, ids=lambda v: str(v) if isinstance(v, int) else "b%d-c%d-den%g" % (v[0], v[1], v[5]))
def test_combine3(n, form):
    hb, hc, wa, wb, wc, den = form
    i = R.combine3_inputs(n, rnd)
    a, b, c = i["a"], (i["b"] if hb else None), (i["c"] if hc else None)
    buf, out = guarded((n,), F32)
    ops.combine3(dev(a), dev(b), dev(c), out, wa=wa, wb=wb, wc=wc, den=den)()
    ref = R.combine3_ref(a, b, c, wa, wb, wc, den)
    record("combine3", fetch(buf, out), ref, R.limit_f32(ref))


def test_combine3_on_a_batch_slice():
    """q_sample's form (ddpm.py:334): x[b], noise[b] -> out[b], one item of a batch at a time"""
    x, noise = rnd((3, 4, 5, 7), 174), rnd((3, 4, 5, 7), 175)
    buf, out = guarded(tuple(x.shape), F32)
    xd, nd = dev(x), dev(noise)
    ops.combine3(xd[1], nd[1], None, out[1], wa=0.8, wb=0.6, wc=0.0, den=0.0)()
    torch.cuda.synchronize()
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all() and torch.isnan(out[0]).all() and torch.isnan(out[2]).all()
    got = out[1].cpu()
    assert not torch.isnan(got).any()
    ref = R.combine3_ref(x[1], noise[1], None, 0.8, 0.6, 0.0, 0.0)
    record("combine3", got, ref, R.limit_f32(ref))


# ------------------------------------------------------------------------------------------------ elementwise.hip
@pytest.mark.parametrize("n", R.CAST_N)
@pytest.mark.parametrize("src,dst", R.CAST_PAIRS, ids=lambda d: str(d)[6:])
def test_cast(src, dst, n):
    x = R.cast_input(src, n, rnd)
    buf, out = guarded((n,), dst)
    ops.cast(dev(x), out)()
    got = fetch(buf, out)
    want = x.to(dst)
    assert torch.equal(bits(got), bits(want)), f"first differing inputs: {x[bits(got) != bits(want)][:8].tolist()}"
    assert torch.equal(got.double(), R.cast_ref(x, dst))


def test_silu_f32():
    x = R.silu_input(rnd)
    buf, out = guarded(tuple(x.shape), F32)
    ops.silu_f32(dev(x), out)()
    ref = R.silu_ref(x)
    record("silu_f32", fetch(buf, out), ref, R.limit_f32(ref))


@pytest.mark.parametrize("with_eps", R.GAUSS_CASES)
def test_gaussian_sample(with_eps):
    i = R.gaussian_inputs(rnd)
    eps = i["eps"] if with_eps else None
    buf, out = guarded((R.GAUSS_B, R.GAUSS_C, R.GAUSS_H, R.GAUSS_W), F32)
    ops.gaussian_sample(dev(i["moments"]), dev(eps), out, scale=i["scale"])()
    got = fetch(buf, out)
    ref = R.gaussian_sample_ref(i["moments"], eps, i["scale"])
    record("gaussian_sample", got, ref, R.limit_f32(ref))
    if not with_eps:                                           # eps == NULL: scale * mean, whatever the logvar half holds
        assert torch.equal(got, torch.tensor(i["scale"], dtype=F32) * i["moments"][:, :R.GAUSS_C])


def test_to_image():
    x = R.to_image_input(rnd)
    buf, out = guarded(tuple(x.shape), F32)
    ops.to_image(dev(x), out)()
    got = fetch(buf, out)
    ref = R.to_image_ref(x)
    record("to_image", got, ref, R.limit_f32(ref))
    assert torch.equal(bits(got), bits(((x + 1.0) / 2.0).clamp(0.0, 1.0)))
    assert got.min() == 0 and got.max() == 1


@pytest.mark.parametrize("cfg,with_noise,with_px0,ld", R.DDIM_UPDATE_CASES)
def test_ddim_update(cfg, with_noise, with_px0, ld):
    i = R.ddim_update_inputs((cfg, with_noise, with_px0, ld), rnd)
    noise = i["noise"] if with_noise else None
    shape = tuple(i["img"].shape)
    ibuf, img = guarded(shape, F32)
    img.copy_(i["img"])
    pbuf, px0 = guarded(shape, F32) if with_px0 else (None, None)
    ops.ddim_update(dev(i["eps"]), img, px0, dev(noise), dev(i["coefs"]), cfg=cfg, scale=R.DDIM_SCALE)()
    rp, r0 = R.ddim_update_ref(i["eps"], i["img"], noise, i["coefs"], cfg, R.DDIM_SCALE)
    record("ddim_update", fetch(ibuf, img), rp, R.limit_f32(rp))
    if with_px0:
        record("ddim_update", fetch(pbuf, px0), r0, R.limit_f32(r0))


@pytest.mark.parametrize("dup,dt,Cpad", R.DDIM_PACK_CASES, ids=lambda v: str(v)[6:] if isinstance(v, torch.dtype) else str(v))
def test_ddim_pack_input(dup, dt, Cpad):
    i = R.ddim_pack_inputs(rnd)
    buf, out = guarded((dup * R.DDIM_B, R.DDIM_H, R.DDIM_W, Cpad), dt)
    ops.ddim_pack_input(dev(i["img"]), dev(i["z"]), dev(i["mask"]), out, dup=dup)()
    got = fetch(buf, out)
    want = R.ddim_pack_ref(i["img"], i["z"], i["mask"], dup, Cpad).float().to(dt)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("dt", R.LAYOUT_DTYPES, ids=lambda d: str(d)[6:])
def test_nchw_to_nhwc(dt):
    x = R.layout_input(rnd)
    buf, out = guarded((R.LAYOUT_B, R.LAYOUT_H, R.LAYOUT_W, R.LAYOUT_CPAD), dt)
    ops.nchw_to_nhwc(dev(x), out)()
    got = fetch(buf, out)
    assert torch.equal(bits(got), bits(R.nchw_to_nhwc_ref(x, R.LAYOUT_CPAD).float().to(dt)))


@pytest.mark.parametrize("dt", R.LAYOUT_DTYPES, ids=lambda d: str(d)[6:])
def test_nhwc_to_nchw_pitched_source(dt):
    """what every real caller passes: a 16-bit channels-last tensor of pitch 16 of which the first C = 5 channels count"""
    src = rnd((R.LAYOUT_B, R.LAYOUT_H, R.LAYOUT_W, R.LAYOUT_LDX), 232).to(dt)
    x = src.to(DEV)[..., :R.LAYOUT_C]
    buf, out = guarded((R.LAYOUT_B, R.LAYOUT_C, R.LAYOUT_H, R.LAYOUT_W), F32)
    ops.nhwc_to_nchw(x, out)()
    got = fetch(buf, out)
    assert torch.equal(bits(got), bits(R.nhwc_to_nchw_ref(src, R.LAYOUT_C).float()))


@pytest.mark.parametrize("n,dim", R.TIMESTEP_CASES)
def test_timestep_embedding(n, dim):
    i = R.timestep_inputs((n, dim))
    buf, out = guarded((n, dim), F32)
    ops.timestep_embedding(dev(i["t"]), dev(i["freqs"]), out)()
    got = fetch(buf, out)
    ref = R.timestep_embedding_ref(i["t"], i["freqs"], dim)
    record("timestep_embedding", got, ref, R.limit_f32(ref, scale=0.1))
    if dim % 2:
        assert (bits(got[:, -1]) == 0).all()                   # the odd-dim zero column: exactly 0


# ------------------------------------------------------------------------------------------------ norm.hip
@pytest.mark.parametrize("cols,ld", R.SOFTMAX_CASES)
def test_softmax_rows(cols, ld):
    x = R.softmax_inputs((cols, ld), rnd)["x"]
    buf, parent = guarded((R.SOFTMAX_ROWS, ld), F32)
    view = parent[:, :cols]
    view.copy_(x)
    ops.softmax_rows(view)()
    torch.cuda.synchronize()
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all() and torch.isnan(parent[:, cols:]).all()          # guards and the pitch gap
    got = view.cpu()
    ref = R.softmax_rows_ref(x)
    record("softmax_rows", got, ref, R.limit_f32(ref, scale=0.01))
    assert (got.double().sum(1) - 1).abs().max().item() <= 1e-5


# ------------------------------------------------------------------------------------------------ the wrappers' contract
def test_fp16_is_refused():
    """none of these kernels has an fp16 instantiation (the CLI's fp16 mode keeps the towers in fp32): rejected on the host, before any launch"""
    h = lambda *s: torch.zeros(s, dtype=F16, device=DEV)
    f = lambda *s: torch.zeros(s, dtype=F32, device=DEV)
    with pytest.raises(_lib.RefaceHipError):
        ops.channel_affine(h(4, 8), f(8), f(8), h(4, 8))()
    with pytest.raises(_lib.RefaceHipError):
        ops.channel_affine(f(4, 8), f(8), f(8), h(4, 8))()
    with pytest.raises(_lib.RefaceHipError):
        ops.spatial_mean(h(2, 3, 3, 8), f(2, 8))()
    with pytest.raises(_lib.RefaceHipError):
        ops.se_scale_add(h(2, 3, 3, 8), f(2, 8), h(2, 3, 3, 8), h(2, 3, 3, 8), stride=1)()
    with pytest.raises(_lib.RefaceHipError):
        ops.clip_tokens(h(2, 3, 8), f(8), f(4, 8), h(2, 4, 8))()
    with pytest.raises(_lib.RefaceHipError):
        ops.adaptive_avgpool(f(2, 3, 6, 6), h(2, 3, 3, 8), nhwc=True)()


def test_bad_shapes_are_refused():
    f = lambda *s: torch.zeros(s, dtype=F32, device=DEV)
    with pytest.raises(_lib.RefaceHipError):
        ops.softmax_rows(f(3, 8)[:, :6])()                     # cols = 6: not a multiple of the 4-wide vector
    with pytest.raises(_lib.RefaceHipError):
        ops.se_scale_add(f(2, 5, 7, 8), f(2, 8), f(2, 8, 13, 8), f(2, 5, 7, 8), stride=2)()          # (Ho - 1) * stride = 8 >= Hs = 8


def test_wrapper_asserts():
    f = lambda *s: torch.zeros(s, dtype=F32, device=DEV)
    with pytest.raises(AssertionError):
        ops.silu_f32(torch.zeros(8, dtype=BF16, device=DEV), f(8))
    with pytest.raises(AssertionError):
        ops.channel_affine(f(4, 8), f(8), f(9), f(4, 8))
    with pytest.raises(AssertionError):
        ops.l2norm_rows(f(2, 8), torch.zeros((2, 8), dtype=BF16, device=DEV))
    with pytest.raises(AssertionError):
        ops.spatial_mean(f(2, 3, 3, 8), f(2, 9))
    with pytest.raises(AssertionError):
        ops.clip_tokens(f(2, 3, 8), f(8), f(3, 8), f(2, 4, 8))
    with pytest.raises(AssertionError):
        ops.gaussian_sample(f(2, 8, 3, 3), None, f(2, 8, 3, 3), scale=1.0)
    with pytest.raises(AssertionError):
        ops.se_scale_add(f(2, 3, 3, 8), f(2, 8), f(2, 3, 3, 8), torch.zeros((2, 3, 3, 8), dtype=BF16, device=DEV), stride=1)


def test_zz_worst_ratios():
    """prints the table DESIGN.md records (run the file with -s); every kernel of the file must have reported"""
    for k in sorted(WORST):
        print(f"[side_ops] worst {k:20s} {WORST[k]:.4f}")
    if len(WORST) >= 17:          # the whole file ran (not a -k selection)
        assert all(v <= 1.0 for v in WORST.values())
