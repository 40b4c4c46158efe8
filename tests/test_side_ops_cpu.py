"""CPU checks of tests/side_refs.py, the references of tests/test_side_ops_gpu.py:
  a. every fp64 reference agrees with torch's own fp64 operator to 1e-12 over the GPU file's whole case table (the references are not
     self-certified);
  b. every index / edge mistake a kernel could make, written as a deliberately wrong variant of the *reference*, is told apart from the true
     reference by at least one case of that kernel's table, by more than the tolerance the GPU test applies (the table is not too weak).
No kernel is touched and nothing runs on a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import side_refs as R
from reface_amd.params import seeded_randn as rnd

F64 = torch.float64
AGREE = 1e-12


def agree(ref, other):
    assert ref.dtype == F64 and ref.shape == other.shape
    assert torch.isfinite(ref).all()
    assert (ref - other.double()).abs().max().item() <= AGREE


def caught(pairs):
    """pairs: (wrong, true, limit) per case -> True if some case shows the slip"""
    return any(R.differs(w, t, lim) for w, t, lim in pairs)


# ------------------------------------------------------------------------------------------------ a. references against torch fp64
def test_ref_channel_affine():
    for case in R.CHANNEL_AFFINE_CASES:
        i = R.channel_affine_inputs(case, rnd)
        x = i["buf"][:, :case["C"]]
        v = x.double() * i["a"].double() + i["b"].double()
        agree(R.channel_affine_ref(x, i["a"], i["b"]), v)
        ref = R.channel_affine_ref(x, i["a"], i["b"], i["slope"])
        agree(ref, F.prelu(v, i["slope"].double()))
        # the inputs the issue asks for: positive, zero and negative slopes, and v == 0 exactly (in fp32 and fp64 alike)
        assert (i["slope"] > 0).any() and (i["slope"] == 0).any() and (i["slope"] < 0).any()
        assert (v == 0).sum() >= 3 and ((x * i["a"] + i["b"]) == 0).sum() >= 3 and (v < 0).any()
        assert i["a"].unique().numel() == case["C"] and i["b"].unique().numel() > case["C"] // 2


def test_ref_spatial_mean():
    for case in R.SPATIAL_MEAN_CASES:
        x = R.spatial_mean_inputs(case, rnd)["buf"][..., :case["C"]]
        agree(R.spatial_mean_ref(x), F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), 1)[:, :, 0, 0])


def test_ref_se_scale_add():
    for case in R.SE_SCALE_ADD_CASES:
        i = R.se_scale_add_inputs(case, rnd)
        sc, st = i["buf"][..., :R.SE_C], case["st"]
        assert (R.SE_HO - 1) * st < case["Hs"] and (R.SE_WO - 1) * st < case["Ws"]
        other = i["r"].double() * i["s"].double()[:, None, None, :] + sc.double()[:, ::st, ::st][:, :R.SE_HO, :R.SE_WO]
        agree(R.se_scale_add_ref(i["r"], i["s"], sc, st), other)
    odd = [c for c in R.SE_SCALE_ADD_CASES if c["Hs"] % 2 and c["st"] == 2]
    assert odd and all(2 * (R.SE_HO - 1) == c["Hs"] - 1 and 2 * (R.SE_WO - 1) == c["Ws"] - 1 for c in odd)       # last row / column read at Hs - 1


def _pool_args(case):
    i = R.adaptive_avgpool_inputs(case, rnd)
    return i, dict(crop=case["crop"], a=i["a"], b=i["b"], nhwc=case["nhwc"], Cpad=case.get("Cpad"))


def test_ref_adaptive_avgpool():
    for case in R.ADAPTIVE_AVGPOOL_CASES:
        i, kw = _pool_args(case)
        x = i["x"].double()
        if i["a"] is not None:
            x = x * i["a"].double().view(1, -1, 1, 1) + i["b"].double().view(1, -1, 1, 1)
        if case["crop"] is not None:
            y0, x0, hc, wc = case["crop"]
            x = x[:, :, y0:y0 + hc, x0:x0 + wc]
        other = F.adaptive_avg_pool2d(x, (case["Ho"], case["Wo"]))
        ref = R.adaptive_avgpool_ref(i["x"], case["Ho"], case["Wo"], **kw)
        if case["nhwc"]:
            assert (ref[..., R.POOL_C:] == 0).all()
            ref = ref[..., :R.POOL_C].permute(0, 3, 1, 2)
        agree(ref, other)


def test_ref_bilinear_resize():
    for case in R.BILINEAR_CASES:
        Hi, Wi, Ho, Wo = case
        i = R.bilinear_inputs(case, rnd)
        for a, b in ((None, None), (i["a"], i["b"])):
            x = i["x"].double()
            if a is not None:
                x = x * a.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
            agree(R.bilinear_resize_ref(i["x"], Ho, Wo, a, b), F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False, antialias=False))
    x = R.bilinear_inputs((16, 16, 16, 16), rnd)["x"]
    assert torch.equal(R.bilinear_resize_ref(x, 16, 16), x.double())          # the identity case


def test_ref_clip_tokens():
    for case in R.CLIP_TOKENS_CASES:
        i = R.clip_tokens_inputs(case, rnd)
        B = case[0]
        other = torch.cat([i["cls"].double().view(1, 1, -1).expand(B, 1, -1), i["patch"].double()], 1) + i["pos"].double()[None]
        agree(R.clip_tokens_ref(**i), other)


def test_ref_l2norm_rows_and_extreme_rows_stay_finite():
    scales = set()
    for case in R.L2NORM_CASES:
        x = R.l2norm_inputs(case, rnd)["x"]
        ref = R.l2norm_rows_ref(x)
        agree(ref, F.normalize(x.double(), dim=1, eps=0.0))
        assert ((ref * ref).sum(1) - 1).abs().max() < 1e-12
        # the fp64 reference and a float32 emulation of the kernel's one-wave sum of squares both stay finite and non-zero: the 1e18 / 1e-18
        # rows are inside the kernel's contract (squares within fp32's range), and the emulated fp32 result is far inside the GPU bound
        s = R.l2norm_wave_sum_f32(x)
        assert np.isfinite(s).all() and (s > 0).all() and torch.isfinite(x).all()
        emu = x.double() / torch.from_numpy(np.sqrt(s)).double().view(-1, 1)
        assert not R.differs(emu, ref, 0.25 * R.limit_f32(ref))
        scales |= set(case[2])
    assert 1e18 in scales and 1e-18 in scales


def test_ref_combine3():
    for n, (hb, hc, wa, wb, wc, den) in R.COMBINE3_CASES:
        i = R.combine3_inputs(n, rnd)
        a, b, c = i["a"], (i["b"] if hb else None), (i["c"] if hc else None)
        other = a.double() * wa + (b.double() * wb if hb else 0.0) + (c.double() * wc if hc else 0.0)
        agree(R.combine3_ref(a, b, c, wa, wb, wc, den), other / den if den else other)
    forms = {(f[0], f[1], f[5] != 0) for f in R.COMBINE3_FORMS}
    assert {(True, False, False), (True, False, True), (True, True, True), (True, True, False), (False, False, False)} <= forms


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_ref_cast_is_torch_to():
    for src, dst in R.CAST_PAIRS:
        for n in R.CAST_N:
            x = R.cast_input(src, n, rnd)
            assert x.dtype == src and x.numel() == n
            want = x.to(dst)
            ref = R.cast_ref(x, dst)
            assert torch.equal(ref, want.double()) and torch.equal(torch.signbit(ref), torch.signbit(want))
            assert torch.equal(_bits(ref.to(dst)), _bits(want))
    # the edge list holds what the issue names
    x = R.cast_input(torch.float32, 255, rnd)
    h, b = x.to(torch.float16), x.to(torch.bfloat16)
    assert torch.isinf(x).sum() == 2 and (torch.isinf(h) & ~torch.isinf(x)).sum() >= 5 and (torch.isinf(b) & ~torch.isinf(x)).sum() >= 2
    assert ((h != 0) & (h.abs() < 2.0 ** -14)).sum() >= 4                        # fp16 subnormal results
    assert ((x != 0) & (h == 0)).sum() >= 2 and (x == 0).sum() == 2 and torch.signbit(x[x == 0]).sum() == 1
    assert (b.float() == 2.0).any() and (h.float() == 2.0).any()                 # rounded up across a binade


def test_ref_silu_and_to_image():
    x = R.silu_input(rnd)
    assert x.min() == -100 and x.max() == 100 and (x == 88).any() and (x == -88).any() and (x == 0).sum() >= 2 and x.numel() % 256
    agree(R.silu_ref(x), F.silu(x.double()))
    y = R.to_image_input(rnd)
    assert y.min() == -3 and y.max() == 3 and (y == -1).any() and (y == 1).any() and (y.abs() > 1).sum() > 50
    agree(R.to_image_ref(y), torch.clamp((y.double() + 1.0) / 2.0, 0.0, 1.0))


def test_ref_gaussian_sample():
    i = R.gaussian_inputs(rnd)
    m, eps, scale = i["moments"], i["eps"], i["scale"]
    Cc = R.GAUSS_C
    assert set(R.GAUSS_LOGVARS) <= set(m[:, Cc:].flatten().tolist())
    other = scale * (m.double()[:, :Cc] + torch.exp(0.5 * torch.clamp(m.double()[:, Cc:], -30.0, 20.0)) * eps.double())
    agree(R.gaussian_sample_ref(m, eps, scale), other)
    agree(R.gaussian_sample_ref(m, None, scale), scale * m.double()[:, :Cc])


def test_ref_ddim():
    for case in R.DDIM_UPDATE_CASES:
        cfg, with_noise, _, ld = case
        i = R.ddim_update_inputs(case, rnd)
        B = R.DDIM_B
        noise = i["noise"] if with_noise else None
        xp, px0 = R.ddim_update_ref(i["eps"], i["img"], noise, i["coefs"], cfg, R.DDIM_SCALE)
        e = i["eps"].double()[..., :4].permute(0, 3, 1, 2)
        if cfg:
            e = torch.lerp(e[:B], e[B:], torch.tensor(R.DDIM_SCALE, dtype=F64))
        c = i["coefs"].double()
        o0 = (i["img"].double() - c[1] * e) / c[0]
        op = c[2] * o0 + c[3] * e + (c[4] * noise.double() if with_noise else 0.0)
        assert (xp - op).abs().max() <= AGREE and (px0 - o0).abs().max() <= AGREE
    i = R.ddim_pack_inputs(rnd)
    for dup, dt, Cpad in R.DDIM_PACK_CASES:
        ref = R.ddim_pack_ref(i["img"], i["z"], i["mask"], dup, Cpad)
        one = torch.cat([i["img"], i["z"], i["mask"]], 1).permute(0, 2, 3, 1).double()
        agree(ref, F.pad(torch.cat([one] * dup, 0), (0, Cpad - 9)))


def test_ref_layouts():
    x = R.layout_input(rnd)
    nhwc = R.nchw_to_nhwc_ref(x, R.LAYOUT_CPAD)
    agree(nhwc, F.pad(x.double().permute(0, 2, 3, 1), (0, R.LAYOUT_CPAD - R.LAYOUT_C)))
    agree(R.nhwc_to_nchw_ref(nhwc, R.LAYOUT_C), x.double())
    for dt in R.LAYOUT_DTYPES:
        assert torch.equal(nhwc.to(dt)[..., :R.LAYOUT_C], x.permute(0, 2, 3, 1).to(dt))          # rounding commutes with the permutation


def test_ref_timestep_embedding():
    for case in R.TIMESTEP_CASES:
        n, dim = case
        i = R.timestep_inputs(case)
        args = (i["t"][:, None] * i["freqs"][None]).double()
        other = torch.cat([torch.cos(args), torch.sin(args)] + ([torch.zeros((n, 1), dtype=F64)] if dim % 2 else []), -1)
        ref = R.timestep_embedding_ref(i["t"], i["freqs"], dim)
        agree(ref, other)
        if dim % 2:
            assert (ref[:, -1] == 0).all()


def test_ref_softmax_rows():
    for case in R.SOFTMAX_CASES:
        x = R.softmax_inputs(case, rnd)["x"]
        ref = R.softmax_rows_ref(x)
        agree(ref, torch.softmax(x.double(), -1))
        assert (ref.sum(1) - 1).abs().max() < 1e-12 and ref[1, -1] > 0.99 and (ref[2] == 1.0 / case[0]).all()


# ------------------------------------------------------------------------------------------------ b. the case tables discriminate
def _variant_pairs(kernel, wrong):
    """(wrong variant's output, true reference, the GPU test's limit) for every case of `kernel`'s table"""
    f32 = torch.float32
    if kernel == "channel_affine":
        for case in R.CHANNEL_AFFINE_CASES:
            i = R.channel_affine_inputs(case, rnd)
            x = i["buf"][:, :case["C"]]
            for slope in (None, i["slope"]):
                t = R.channel_affine_ref(x, i["a"], i["b"], slope)
                yield wrong(x, i["a"], i["b"], slope), t, R.limit_f32(t)
    elif kernel == "spatial_mean":
        for case in R.SPATIAL_MEAN_CASES:
            x = R.spatial_mean_inputs(case, rnd)["buf"][..., :case["C"]]
            t = R.spatial_mean_ref(x)
            yield wrong(x), t, R.limit_f32(t)
    elif kernel == "se_scale_add":
        for case in R.SE_SCALE_ADD_CASES:
            i = R.se_scale_add_inputs(case, rnd)
            sc = i["buf"][..., :R.SE_C]
            t = R.se_scale_add_ref(i["r"], i["s"], sc, case["st"])
            yield wrong(i["r"], i["s"], sc, case["st"]), t, R.limit_f32(t)
    elif kernel == "adaptive_avgpool":
        for case in R.ADAPTIVE_AVGPOOL_CASES:
            i, kw = _pool_args(case)
            t = R.adaptive_avgpool_ref(i["x"], case["Ho"], case["Wo"], **kw)
            yield wrong(i["x"], case["Ho"], case["Wo"], **kw), t, R.limit(t, case["dt"])
    elif kernel == "bilinear_resize":
        for case in R.BILINEAR_CASES:
            i = R.bilinear_inputs(case, rnd)
            for a, b in ((None, None), (i["a"], i["b"])):
                t = R.bilinear_resize_ref(i["x"], case[2], case[3], a, b)
                yield wrong(i["x"], case[2], case[3], a, b), t, R.limit_f32(t)
    elif kernel == "clip_tokens":
        for case in R.CLIP_TOKENS_CASES:
            i = R.clip_tokens_inputs(case, rnd)
            t = R.clip_tokens_ref(**i)
            yield wrong(**i), t, R.limit_f32(t)
    elif kernel == "combine3":
        for n, (hb, hc, wa, wb, wc, den) in R.COMBINE3_CASES:
            i = R.combine3_inputs(n, rnd)
            args = (i["a"], i["b"] if hb else None, i["c"] if hc else None, wa, wb, wc, den)
            t = R.combine3_ref(*args)
            yield wrong(*args), t, R.limit_f32(t)
    elif kernel == "gaussian_sample":
        i = R.gaussian_inputs(rnd)
        for with_eps in R.GAUSS_CASES:
            eps = i["eps"] if with_eps else None
            t = R.gaussian_sample_ref(i["moments"], eps, i["scale"])
            yield wrong(i["moments"], eps, i["scale"]), t, R.limit_f32(t)
    elif kernel == "ddim_update":
        for case in R.DDIM_UPDATE_CASES:
            i = R.ddim_update_inputs(case, rnd)
            args = (i["eps"], i["img"], i["noise"] if case[1] else None, i["coefs"], case[0], R.DDIM_SCALE)
            t, w = R.ddim_update_ref(*args), wrong(*args)
            yield w[0], t[0], R.limit_f32(t[0])
            yield w[1], t[1], R.limit_f32(t[1])
    elif kernel == "softmax_rows":
        for case in R.SOFTMAX_CASES:
            x = R.softmax_inputs(case, rnd)["x"]
            t = R.softmax_rows_ref(x)
            yield wrong(x), t, R.limit_f32(t, scale=0.01)
    elif kernel == "timestep_embedding":
        for case in R.TIMESTEP_CASES:
            i = R.timestep_inputs(case)
            t = R.timestep_embedding_ref(i["t"], i["freqs"], case[1])
            yield wrong(i["t"], i["freqs"], case[1]), t, R.limit_f32(t, scale=0.1)
    else:
        raise KeyError(kernel)


VARIANTS = {"channel_affine": R.CHANNEL_AFFINE_VARIANTS, "spatial_mean": R.SPATIAL_MEAN_VARIANTS, "se_scale_add": R.SE_SCALE_ADD_VARIANTS,
            "adaptive_avgpool": R.ADAPTIVE_AVGPOOL_VARIANTS, "bilinear_resize": R.BILINEAR_VARIANTS, "clip_tokens": R.CLIP_TOKENS_VARIANTS,
            "combine3": R.COMBINE3_VARIANTS, "gaussian_sample": R.GAUSS_VARIANTS, "ddim_update": R.DDIM_UPDATE_VARIANTS,
            "softmax_rows": R.SOFTMAX_VARIANTS, "timestep_embedding": R.TIMESTEP_VARIANTS}


@pytest.mark.parametrize("kernel,variant", [(k, v) for k, vs in VARIANTS.items() for v in vs])
def test_table_catches_wrong_variant(kernel, variant):
    assert caught(_variant_pairs(kernel, VARIANTS[kernel][variant])), f"no case of the {kernel} table shows: {variant}"


@pytest.mark.parametrize("kernel", sorted(VARIANTS))
def test_true_reference_is_not_caught(kernel):
    """the harness itself: the true reference, passed as a `variant`, differs in no case"""
    true = {"channel_affine": R.channel_affine_ref, "spatial_mean": R.spatial_mean_ref, "se_scale_add": R.se_scale_add_ref,
            "adaptive_avgpool": R.adaptive_avgpool_ref, "bilinear_resize": R.bilinear_resize_ref, "clip_tokens": R.clip_tokens_ref,
            "combine3": R.combine3_ref, "gaussian_sample": R.gaussian_sample_ref, "ddim_update": R.ddim_update_ref,
            "softmax_rows": R.softmax_rows_ref, "timestep_embedding": R.timestep_embedding_ref}[kernel]
    assert not caught(_variant_pairs(kernel, true))


def test_pool_affine_after_the_mean_is_the_same_function():
    """`affine applied after the mean` cannot be told apart by any case: x -> x * a + b commutes with a mean, so mean(x) * a + b IS the
    reference (to fp64 round-off).  Asserted here so that the equivalence is checked rather than assumed; the slip that does change the
    result -- b added once per bin instead of once per pixel -- is in ADAPTIVE_AVGPOOL_VARIANTS."""
    seen = 0
    for case in R.ADAPTIVE_AVGPOOL_CASES:
        if case["affine"]:
            i, kw = _pool_args(case)
            agree(R.adaptive_avgpool_ref(i["x"], case["Ho"], case["Wo"], **kw), R.adaptive_avgpool_affine_after_mean(i["x"], case["Ho"], case["Wo"], **kw))
            seen += 1
    assert seen >= 2
