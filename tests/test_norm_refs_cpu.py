"""CPU pins of tests/norm_refs.py, the references, generators, tolerance and case tables of tests/test_norm_exact_gpu.py: the fp64 references
agree with torch.nn.functional in float64, every exact generator is exact (fp32 and fp64, two summation orders, identical bits), a plain
fp32 evaluation stays inside tol_apply, mutant references are caught by the cases the GPU file runs, and the tables reach every instantiation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import norm_refs as R
from norm_refs import BF16, F16, F32, F64, bits
from reface_amd import _lib


def test_type_codes_are_the_librarys():
    assert (R.RF_F32, R.RF_BF16, R.RF_BF16X3, R.RF_F16) == (_lib.RF_F32, _lib.RF_BF16, _lib.RF_BF16X3, _lib.RF_F16)


# ------------------------------------------------------------------------------------------------ 1: references vs torch.nn.functional in float64
@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_ref_is_torch_float64(silu):
    g = R._gen(1)
    x = torch.randn((2, 35, 96), generator=g, dtype=F64) * 2 + 0.7
    gamma, beta = R.random_affine(96, 2)
    ref = Fn.group_norm(x.permute(0, 2, 1), 32, gamma.to(F64), beta.to(F64), 1e-5).permute(0, 2, 1)
    ref = Fn.silu(ref) if silu else ref
    assert (R.groupnorm_ref(x, gamma, beta, 1e-5, silu) - ref).abs().max() < 1e-13
    # the chunked partial sums carry the same moments (var = sq / n - mean^2 in fp64), whatever the chunking, empty chunks included
    for nch in (1, 7, 32, 40):
        mean, var = R.moments_of_partials(R.chunk_partials(x, nch), 35, 96)
        m2, v2 = R.moments(x)
        assert (mean - m2).abs().max() < 1e-13 and (var - v2).abs().max() < 1e-12
        assert (R.gn_apply_ref(x, mean, var, gamma, beta, 1e-5, silu) - ref).abs().max() < 1e-12
    xsc, msc, bb = R.gn_apply_terms(x, m2, v2, gamma, beta, 1e-5)
    assert (xsc - msc + bb - R.gn_apply_ref(x, m2, v2, gamma, beta, 1e-5, False)).abs().max() < 1e-13


def test_chunk_layout_has_empty_trailing_chunks():
    x = torch.ones((1, 33, 32), dtype=F64)
    p = R.chunk_partials(x, 32)                                        # ppc = 2: chunks 0..15 two pixels, 16 one, 17..31 none
    assert p[0, :16, :, 0].eq(2).all() and p[0, 16, :, 0].eq(1).all() and p[0, 17:].eq(0).all()


def test_layernorm_and_softmax_refs_are_torch_float64():
    x = torch.randn((5, 264), generator=R._gen(3), dtype=F64) * 3 + 1
    gamma, beta = R.random_affine(264, 4)
    assert (R.layernorm_ref(x, gamma, beta, 1e-5) - Fn.layer_norm(x, (264,), gamma.to(F64), beta.to(F64), 1e-5)).abs().max() < 1e-13
    assert (R.softmax_rows_ref(x) - Fn.softmax(x, -1)).abs().max() < 1e-15


def test_fold_ref_is_groupnorm_then_linear():
    """x W'^T + r == Linear(GroupNorm(x)) with the unrounded W' (fp64 storage)"""
    g = R._gen(5)
    B, HW, C, N = 2, 9, 64, 7
    x = torch.randn((B, HW, C), generator=g, dtype=F64) + 3
    W, bias = torch.randn((N, C), generator=g), torch.randn((N,), generator=g)
    gamma, beta = R.random_affine(C, 6)
    mean, var = R.moments(x)
    wp, wps = R.fold_weights_ref(W, mean, var, gamma, 1e-6, F64)
    assert torch.equal(wp, wps)
    r, mag = R.fold_rowvec_ref(W, wps, mean, beta, bias)
    ref = Fn.linear(R.groupnorm_ref(x, gamma, beta, 1e-6, False), W.to(F64), bias.to(F64))
    assert (torch.einsum("bpc,bnc->bpn", x, wp) + r[:, None, :] - ref).abs().max() < 1e-11
    assert (mag >= r.abs() - 1e-12).all()
    assert (R.fold_weights_ref(W, mean, var, gamma, 1e-6, BF16)[1] - wp).abs().max() > 0          # the stored form is the rounded one


def test_split_pair_and_block_quantiser():
    y = torch.randn((6, 64), generator=R._gen(7)) * torch.tensor([1e-3, 0.1, 1, 7, 300, 5e4])[:, None]
    hi, lo = R.split_pair(y)
    ye = torch.arange(-1024, 1025).to(F32) / 16                        # 16-bit values (the exact cases'): lo is exact, so hi == RNE_bf16(hi + lo)
    he, le = R.split_pair(ye)
    assert torch.equal(he.float() + le.float(), ye) and torch.equal(he, (he.float() + le.float()).to(BF16)) and (le != 0).any()
    assert ((hi.double() + lo.double() - y.double()).abs() <= 2.0 ** -17 * y.double().abs()).all()
    rows = R.split_rows(y, 136)
    assert torch.equal(rows[:, :64], hi) and torch.equal(rows[:, 64:128], lo) and rows[:, 128:].eq(0).all()
    y[0, :32] = 0
    y[1, 5] = 448.0                                                     # amax on the boundary: mantissa 1.75 keeps the exponent
    y[2, 5] = 449.0
    q, code = R.quant_act_np(y.numpy())
    # torch's own float8 conversion on the same scale rule (test_ops_gpu._quant_act_ref)
    yb = y.reshape(6, 2, 32)
    amax = yb.abs().amax(-1)
    m, e = torch.frexp(amax)
    c = (e - 1 + 127 - 8 + (2 * m > 1.75).int()).clamp(0, 253)
    c = torch.where(amax > 0, c, torch.zeros_like(c))
    qt = (yb / torch.pow(2.0, c.float() - 127.0)[..., None]).reshape(6, 64).to(torch.float8_e4m3fn).view(torch.uint8)
    assert np.array_equal(code, c.to(torch.uint8).numpy()) and np.array_equal(q, qt.numpy())
    assert code[0, 0] == 0 and code[1, 0] == 127 and code[2, 0] == 128


# ------------------------------------------------------------------------------------------------ 2: the exact generators are exact
def _two_orders(x, cpg):
    """group sums of x [B, HW, C] in two different orders: channels then pixels; reversed pixels then reversed channels"""
    B, HW, C = x.shape
    a = x.reshape(B, HW, 32, cpg).sum(3).sum(1)
    b = x.flip(1).sum(1).reshape(B, 32, cpg).flip(2).sum(2)
    return a, b


@pytest.mark.parametrize("C,HW", [(32, 33), (320, 81), (4096, 1000)])
def test_stats_generator_is_exact(C, HW):
    x = R.stats_exact_input(2, HW, C, C + HW)
    k = x * 4
    assert torch.equal(k, k.round()) and k.abs().max() <= 16
    assert torch.equal(R.stored(x, BF16), x) and torch.equal(R.stored(x, F16), x)
    assert len(torch.unique(k[0, :, 0])) > 2 and (C == 32 or len(torch.unique(k[0, 0, :C // 32])) > 1)          # varies per pixel and per channel
    assert (R.moments(x)[0].abs() > 0.1).all()                                                    # non-zero mean per group
    for dt in R.STATS_DTYPES:
        for nch in (1, 7, 32):
            assert R.stats_exact_bound(dt, HW, C, nch) < 2 ** 24
    for v in (x, x * x):
        a64, b64 = _two_orders(v, C // 32)
        a32, b32 = _two_orders(v.to(F32), C // 32)
        assert a32.dtype == F32 and torch.equal(bits(a64), bits(b64)) and torch.equal(bits(a32), bits(b32)) and torch.equal(bits(a32.to(F64)), bits(a64))


def test_apply_generator_is_exact():
    B, HW, C = 3, 5, 320
    x, mean, (gamma, beta) = R.apply_exact_input(B, HW, C, 1), R.exact_means(B), R.exact_affine(C)
    assert set(gamma.abs().tolist()) == {0.5, 1.0, 2.0, 4.0} and (gamma < 0).any() and (gamma > 0).any()
    assert torch.equal(beta * 4, (beta * 4).round()) and torch.equal(mean, mean.round())
    assert torch.equal(R.stored(x, BF16), x) and torch.equal(R.stored(x, F16), x)
    for nch in (1, 9, 97):
        part = R.exact_partials(mean, HW, C, nch, nch)
        assert torch.equal(part, part.round())
        for p in (part, part.flip(1)):                                  # any order of the chunk sums
            m, v = R.moments_of_partials(p, HW, C)
            assert torch.equal(m, mean) and torch.equal(v, torch.full_like(v, 4.0))
    var = torch.full((B, 32), 4.0, dtype=F64)
    y = R.gn_apply_ref(x, mean, var, gamma, beta, 0.0, False)
    g = R.group_index(C)
    sc = (torch.tensor(0.5) * gamma)                                     # fp32, as the kernel: rstd gamma, beta - mean sc, x sc + sh
    sh = beta[None, :] - mean.to(F32)[:, g] * sc[None, :]
    y32a = x.to(F32) * sc + sh[:, None, :]
    y32b = (x.to(F32) - mean.to(F32)[:, g][:, None, :]) * sc + beta
    assert y32a.dtype == F32 and torch.equal(y32a.to(F64), y) and torch.equal(y32b.to(F64), y)
    assert torch.equal(y * 16, (y * 16).round()) and y.abs().max() < 64


@pytest.mark.parametrize("C,N", [(32, 320), (1056, 7), (1536, 9)])
def test_fold_generator_is_exact(C, N):
    B = R.FOLD_B
    W, bias = R.fold_exact_weights(N, C, C)
    gamma, beta = R.exact_affine(C)
    mean, var = R.exact_means(B), torch.full((B, 32), 4.0, dtype=F64)
    assert torch.equal(W * 4, (W * 4).round()) and W.abs().max() <= 8
    for dt in R.FOLD_OUT:
        wp, wps = R.fold_weights_ref(W, mean, var, gamma, 0.0, dt)
        assert torch.equal(wp, wps)
    r, mag = R.fold_rowvec_ref(W, wps, mean, beta, bias)
    assert mag.max() * 16 < 2 ** 24 and torch.equal(r * 16, (r * 16).round())                    # every partial sum: a multiple of 2^-4 below 2^20
    g = R.group_index(C)
    t = (W * beta)[None] - wps.to(F32) * mean.to(F32)[:, g][:, None, :]                          # fp32 terms, two summation orders
    assert t.dtype == F32
    ra = t.sum(2) + bias
    rb = t.flip(2).reshape(B, N, 8, C // 8).sum(3).sum(2) + bias
    assert torch.equal(ra.to(F64), r) and torch.equal(rb.to(F64), r)


@pytest.mark.parametrize("C", [4, 8, 520, 3072])
def test_layernorm_generator_is_exact(C):
    x, m, s = R.ln_exact_input(5, C, C)
    assert torch.equal(s.abs(), torch.ones_like(s)) and s.sum(1).eq(0).all() and len(torch.unique(m)) > 1
    assert torch.equal(R.stored(x, BF16), x) and torch.equal(R.stored(x, F16), x)
    gamma, beta = R.exact_affine(C)
    y = R.layernorm_ref(x, gamma, beta, 0.0)
    assert torch.equal(y, s * gamma.to(F64) + beta.to(F64))
    x32 = x.to(F32)
    for xs in (x32, x32.flip(1)):
        mean = xs.sum(1) / C
        var = ((xs - mean[:, None]) ** 2).sum(1) / C
        assert torch.equal(mean.to(F64), m) and var.eq(4).all()
    y32 = (x32 - m.to(F32)[:, None]) * 0.5 * gamma + beta
    assert torch.equal(y32.to(F64), y)


@pytest.mark.parametrize("cols,pad", R.SOFTMAX_CASES)
def test_softmax_generator_is_exact(cols, pad):
    x, ref = R.softmax_exact_input(R.SOFTMAX_ROWS, cols, cols)
    k = (x == 0).sum(1)
    assert len(torch.unique(k)) >= min(4, cols - 1) - (cols == 4) and x[0, -1] == 0 and x[1, 0] == 0 and ((x == 0) | (x == -1000)).all()
    assert torch.equal(R.softmax_rows_ref(x).to(F32), ref)               # fl32(1 / k) at the zeros, 0 elsewhere
    assert torch.equal(Fn.softmax(x, -1), ref)
    assert torch.equal(ref[x == 0], (1.0 / k.to(F32)).repeat_interleave(k))


# ------------------------------------------------------------------------------------------------ 3: a plain fp32 evaluation is inside tol_apply
def _c_case(pair, silu, eps, shape, **kw):
    i = R.apply_random_inputs(pair, silu, eps, shape, **kw)
    mean, var = R.moments_of_partials(i["partial"], shape["HW"], shape["C"])
    return i, mean, var


@pytest.mark.parametrize("pair,silu,eps", R.APPLY_RANDOM_CASES, ids=lambda v: R.PAIR_ID(v) if isinstance(v, tuple) else str(v))
def test_fp32_evaluation_is_inside_tol_apply(pair, silu, eps):
    in_dt, out = pair
    for shape in R.APPLY_RANDOM_SHAPES:
        i, mean, var = _c_case(pair, silu, eps, shape)
        xsc, msc, bb = R.gn_apply_terms(i["x"], mean, var, i["gamma"], i["beta"], eps)
        y = xsc - msc + bb
        ref, lim = (R.silu64(y) if silu else y), R.tol_apply(y, xsc, msc, bb, out, silu)
        g = R.group_index(shape["C"])
        sc = (1.0 / torch.sqrt(var + eps)).to(F32)[:, g] * i["gamma"]
        sh = i["beta"] - mean.to(F32)[:, g] * sc
        y32 = i["x"].to(F32) * sc[:, None, :] + sh[:, None, :]
        y32 = Fn.silu(y32) if silu else y32
        got = y32.to(F64)
        if out == "split":
            hi, lo = R.split_pair(y32)
            got = hi.to(F64) + lo.to(F64)
        elif out != F32:
            got = y32.to(out).to(F64)
        ratio = ((got - ref).abs() / lim).max().item()
        assert ratio <= 1.0, ratio
        assert (lim <= (R.STEP[out] + 3e-6) * ref.abs() + 2e-5).all()          # and the limit is of the rounding class, not a loose one


# ------------------------------------------------------------------------------------------------ 4: mutants
def _differs(a, b):
    return int((bits(a) != bits(b)).sum())


def test_mutant_drop_last_pixel_and_group_mod32_change_exact_partials():
    for C in R.STATS_C:
        for HW, nch, _ in R.STATS_SHAPES:
            x = R.stats_exact_input(R.STATS_B, HW, C, 17 * HW + C)
            ref = R.chunk_partials(x, nch)
            assert _differs(R.chunk_partials(x, nch, "drop_last_pixel"), ref) > 0, (C, HW, nch)
            if C > 32:                                                  # (one channel per group: c % 32 == c / cpg)
                assert _differs(R.chunk_partials(x, nch, "group_mod32"), ref) > 0, (C, HW, nch)


@pytest.mark.parametrize("pair", R.GN_PAIRS, ids=R.PAIR_ID)
def test_mutants_change_exact_apply_outputs(pair):
    in_dt, out = pair
    hit = {"group_mod32": 0, "affine_shift_vector": 0, "lo_plane": 0}
    for i, c in enumerate(R.apply_exact_cases(in_dt, out)):
        B, HW, C = c["B"], c["HW"], c["C"]
        if B > 3:
            continue
        x, mean, var = R.apply_exact_input(B, HW, C, 31 * i + C), R.exact_means(B), torch.full((B, 32), 4.0, dtype=F64)
        gamma, beta = R.exact_affine(C)
        y = R.gn_apply_ref(x, mean, var, gamma, beta, 0.0, False).reshape(-1, C).to(F32)
        st = (lambda v: R.split_rows(v, 2 * C)) if out == "split" else (lambda v: v.to(out))
        for mut in ("group_mod32", "affine_shift_vector"):
            ym = R.gn_apply_ref(x, mean, var, gamma, beta, 0.0, False, mutant=mut, vec=R.vec_of(in_dt)).reshape(-1, C).to(F32)
            if C > 32 or mut != "group_mod32":
                assert _differs(st(ym), st(y)) > 0, (mut, c)
                hit[mut] += 1
        if out == "split":
            assert _differs(R.split_rows(y, 2 * C, lo_at=C - 8), R.split_rows(y, 2 * C)) > 0
            hit["lo_plane"] += 1
    assert hit["group_mod32"] and hit["affine_shift_vector"] and (hit["lo_plane"] or out != "split")


def test_mutants_change_exact_fold_and_layernorm_outputs():
    B = R.FOLD_B
    for C, N, with_bias, nch in R.FOLD_CASES:
        W, bias = R.fold_exact_weights(N, C, 3 * C + N)
        gamma, beta = R.exact_affine(C)
        mean, var = R.exact_means(B), torch.full((B, 32), 4.0, dtype=F64)
        wp = R.fold_weights_ref(W, mean, var, gamma, 0.0, F32)[1]
        wm = R.fold_weights_ref(W, mean, var, torch.roll(gamma, -8), 0.0, F32)[1]
        assert _differs(wm, wp) > 0
        r = R.fold_rowvec_ref(W, wp, mean, beta, bias)[0]
        if C > 32:
            gm = torch.arange(C) % 32
            rm = (0 if bias is None else bias.to(F64))[None] + (W.to(F64) * beta.to(F64)).sum(1)[None] - (wp * mean[:, gm][:, None, :]).sum(2)
            assert _differs(rm, r) > 0
    for C in (8, 520):
        x, m, s = R.ln_exact_input(3, C, 7 * C + 3)
        gamma, beta = R.exact_affine(C)
        y = R.layernorm_ref(x, gamma, beta, 0.0)
        if C > 8:
            assert _differs(R.layernorm_ref(x, torch.roll(gamma, -8), torch.roll(beta, -8), 0.0), y) > 0


@pytest.mark.parametrize("pair", [p for p in R.GN_PAIRS if p[0] != F32], ids=R.PAIR_ID)
def test_mutant_statistics_of_unrounded_values_exceeds_tol_apply(pair):
    in_dt, out = pair
    for silu, eps in ((0, 1e-5), (1, 1e-6)):
        shape = R.APPLY_RANDOM_SHAPES[0]
        i, mean, var = _c_case(pair, silu, eps, shape)
        xsc, msc, bb = R.gn_apply_terms(i["x"], mean, var, i["gamma"], i["beta"], eps)
        y = xsc - msc + bb
        ref, lim = (R.silu64(y) if silu else y), R.tol_apply(y, xsc, msc, bb, out, silu)
        _, mm, vm = _c_case(pair, silu, eps, shape, unrounded_stats=True)
        mut = R.gn_apply_ref(i["x"], mm, vm, i["gamma"], i["beta"], eps, silu)
        assert ((mut - ref).abs() > lim).any()


@pytest.mark.parametrize("pair", R.GN_PAIRS, ids=R.PAIR_ID)
def test_mutants_exceed_tol_apply_on_random_cases(pair):
    in_dt, out = pair
    shape, silu, eps = R.APPLY_RANDOM_SHAPES[0], 1, 1e-5
    i, mean, var = _c_case(pair, silu, eps, shape)
    xsc, msc, bb = R.gn_apply_terms(i["x"], mean, var, i["gamma"], i["beta"], eps)
    y = xsc - msc + bb
    ref, lim = R.silu64(y), R.tol_apply(y, xsc, msc, bb, out, silu)
    for mut in ("group_mod32", "affine_shift_vector"):
        ym = R.gn_apply_ref(i["x"], mean, var, i["gamma"], i["beta"], eps, silu, mutant=mut, vec=R.vec_of(in_dt))
        assert ((ym - ref).abs() > lim).any(), mut
    pm = R.chunk_partials(i["x"], 7, "drop_last_pixel")
    mm, vm = R.moments_of_partials(pm, shape["HW"], shape["C"])
    assert ((R.gn_apply_ref(i["x"], mm, vm, i["gamma"], i["beta"], eps, silu) - ref).abs() > lim).any()


# ------------------------------------------------------------------------------------------------ 5: the tables reach every instantiation
def test_case_tables_reach_every_instantiation():
    geo = {(dt, C): R.gn_geometry(dt, C) for dt in R.STATS_DTYPES for C in R.STATS_C}
    assert {g["PL"] for g in geo.values()} >= {64, 32, 16, 6, 3, 1}
    assert geo[(BF16, 320)]["TV"] == 40 and geo[(BF16, 320)]["PL"] == 6 and geo[(BF16, 320)]["idle"] == 16          # the ragged split
    assert {g["ns"] for g in geo.values()} >= {1, 2, 4}
    assert max(g["lds"] for g in geo.values()) == 64 * 1024 and geo[(BF16, 4096)]["lds"] == 64 * 1024                # the LDS edge
    assert R.gn_geometry(BF16, 4128)["lds"] > 64 * 1024                                                              # (refused: case H)
    assert (33, 32, 2) in R.STATS_SHAPES and {s[0] for s in R.STATS_SHAPES} == {1, 2, 31, 33, 81, 1000} and {s[1] for s in R.STATS_SHAPES} == {1, 7, 32}
    for pair in R.GN_PAIRS + [(BF16, "fp8")]:
        cs = R.apply_exact_cases(*pair)
        assert [R.gn_geometry(pair[0], c["C"])["ns"] for c in cs[:4]] == [1, 2, 3, 4]
        assert {R.gn_geometry(pair[0], c["C"])["slots"] for c in cs} == {1, 2, 4}
        assert {c["HW"] for c in cs} >= {1, 2, 3, 33} and {c["B"] for c in cs} >= {1, 3, 600, 1025} and {c["nchunks"] for c in cs} >= {1, 9, 97}
        assert {R.apply_achunks(c["B"], c["HW"]) for c in cs} >= {1, 2, 17}
        assert any(c["xpad"] for c in cs) and any(c["opad"] for c in cs)
    assert R.gn_geometry(BF16, 4128)["ns"] == 3 and R.c_for_ns(BF16, 3) == 4128
    for dt, cs in R.LN_C.items():
        assert {R.ln_nv(dt, C) for C in cs} == {1, 2, 3, 6}
        assert R.ln_nv(dt, cs[0]) == 1 and cs[0] == R.vec_of(dt)                                  # one vector in one lane
    assert {R.ln_nv(BF16, C) for C in R.LN_C_FP8} == {1, 2, 3, 6} and all(C % 32 == 0 for C in R.LN_C_FP8)
    assert any(M % 4 for M in R.LN_M) and max(R.LN_M) > 128
    assert {R.fold_nit(c[0]) for c in R.FOLD_CASES if c[1] % 8} == {1, 2, 3} and {c[1] for c in R.FOLD_CASES} == {1, 7, 9, 320}
    assert {c[0] for c in R.FOLD_CASES} == {32, 512, 544, 1024, 1056, 1536} and {c[2] for c in R.FOLD_CASES} == {True, False}
    assert [c[0] for c in R.SOFTMAX_CASES] == [4, 8, 1020, 1024, 1028, 4096, 9216] and all(c[1] > 0 for c in R.SOFTMAX_CASES)
    assert len(R.APPLY_RANDOM_CASES) == 4 * len(R.GN_PAIRS)
    assert {R.gn_geometry(F32, s["C"])["slots"] for s in R.APPLY_RANDOM_SHAPES} == {1, 4} and {R.gn_geometry(BF16, s["C"])["slots"] for s in R.APPLY_RANDOM_SHAPES} == {1, 2}


# ------------------------------------------------------------------------------------------------ 6: the guard checker itself
@pytest.mark.parametrize("dt", [F32, BF16, F64, torch.uint8], ids=str)
def test_guarded_catches_every_kind_of_stray_write(dt):
    one = 1 if dt == torch.uint8 else 1.0
    G = R.guarded((5, 8), 12, dt, live_rows=3)
    G.view[:3] = one
    G.fetch("clean")
    for r, c in ((R.GUARD - 1, 0), (R.GUARD + 5, 0), (R.GUARD, 8), (R.GUARD + 3, 0)):          # front guard, back guard, pitch gap, unused row
        G = R.guarded((5, 8), 12, dt, live_rows=3)
        G.view[:3] = one
        G.buf[r, c] = one
        with pytest.raises(AssertionError):
            G.check("stray")
    if dt != torch.uint8:
        G = R.guarded((5, 8), 12, dt, live_rows=3)
        G.view[:2] = one
        with pytest.raises(AssertionError):
            G.filled("hole")
