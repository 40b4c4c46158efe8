"""The normalisation kernels of reface_amd/csrc/norm.hip pinned through the C ABI: exact cases bit for bit, real-valued cases against the fp64
references of tests/norm_refs.py (pinned on the CPU by tests/test_norm_refs_cpu.py, which also asserts that the case tables reach every
instantiation).  Every output is a view inside a NaN- / sentinel-filled allocation; the guard rows, the pitch gaps and the unused slots must
come back untouched, and inputs carry NaN in their own pitch gaps, so a read outside the tensor poisons the result.

A  rf_groupnorm_stats / rf_groupnorm_finalize: quarter-integer inputs, partial sums bit-equal to the fp64 chunk sums.
B  rf_groupnorm_apply / _apply_fp8 with host-written partials (integer means, var = 4, eps = 0): outputs bit-equal, every type pair.
C  the same pairs on real values, SiLU on / off, against fp64 within norm_refs.tol_apply (derived there, never fitted).
D  conditioning probes through ops.groupnorm: mean / std of the input in {0, 8, 64} (16-bit) and {0, 64, 1000} (fp32), bound = one storage
   rounding + 4 x the error of PyTorch's fp32 CPU group_norm on the same stored inputs (E32, printed).  The ratios are PROBES: the mean-to-spread
   ratios of the real checkpoint's activations are unmeasured, so these cases say how far the one-pass sums hold, not that they hold in use.
E  rf_layernorm / rf_layernorm_fp8: exact rows bit-equal; conditioned rows as in D with layer_norm as the yardstick.
F  rf_groupnorm_fold_linear: exact W' and row vector per sample; one real-valued case against fp64.
G  rf_softmax_rows: rows whose result is fl32(1 / k) or 0 exactly.
H  refusals: argument sets rejected on the host before any launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import norm_refs as R
from norm_refs import BF16, F16, F32, F64, bits
from reface_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PID = R.PAIR_ID


def L():
    return ops._lib.load()


def S():
    return ops.stream_ptr()


def err():
    return (L().rf_last_error() or b"").decode()


def ok(rc):
    assert rc == 0, err()
    torch.cuda.synchronize()


def rows_in(x64, dt, pad):
    """[.., C] fp64 values -> device rows [M, C + pad] in dt, the pitch gap NaN: (buffer, pitch)"""
    C = x64.shape[-1]
    r = x64.reshape(-1, C)
    buf = torch.full((r.shape[0], C + pad), float("nan"), dtype=dt, device=DEV)
    buf[:, :C] = r.to(dt)
    return buf, C + pad


def partial_in(p):
    """host partial sums -> device, NaN behind the last used slot"""
    buf = torch.full((p.numel() + 128,), float("nan"), dtype=F64, device=DEV)
    buf[:p.numel()] = p.reshape(-1)
    return buf


def worst(tag, got, ref, lim):
    e = (got.to(F64) - ref).abs()
    assert torch.isfinite(got.to(F64)).all(), tag
    ratio = (e / lim).max().item()
    print(f"[norm] {tag}: max err {e.max().item():.3e}, worst err/limit {ratio:.4f}")
    return e, ratio


# ------------------------------------------------------------------------------------------------ A: statistics
@pytest.mark.parametrize("C", R.STATS_C)
def test_a_stats_bit_equal(C):
    B = R.STATS_B
    for HW, nch, xp in R.STATS_SHAPES:
        x = R.stats_exact_input(B, HW, C, 17 * HW + C)
        ref = R.chunk_partials(x, nch)                                 # one reference, shared by the three input types
        for dt in R.STATS_DTYPES:
            tag = f"stats {dt} C={C} HW={HW} nchunks={nch}"
            assert R.stats_exact_bound(dt, HW, C, nch) < 2 ** 24
            xb, ldx = rows_in(x, dt, xp * R.vec_of(dt))
            P = R.guarded((B * nch + 5, 64), 64, F64, DEV, live_rows=B * nch)
            ok(L().rf_groupnorm_stats(R.CODE[dt], xb.data_ptr(), B, HW, C, ldx, nch, P.ptr(), S()))
            P.check(tag)
            P.filled(tag)
            got = P.view[:B * nch].cpu().reshape(B, nch, 32, 2)
            assert torch.equal(bits(got), bits(ref)), f"{tag}: {int((bits(got) != bits(ref)).sum())} partial sums differ"


@pytest.mark.parametrize("n", R.FINALIZE_CHUNKS)
def test_a_finalize_bit_equal(n):
    B = 3
    p = torch.randint(-2 ** 40, 2 ** 40, (B, n, 32, 2), generator=R._gen(n)).to(F64)
    P = R.guarded((B, 64), 64, F64, DEV)
    ok(L().rf_groupnorm_finalize(partial_in(p).data_ptr(), B, n, P.ptr(), S()))
    got = P.fetch(f"finalize {n}").reshape(B, 32, 2)
    assert torch.equal(bits(got), bits(p.sum(1)))


# ------------------------------------------------------------------------------------------------ B / C: apply
def launch_apply(in_dt, out, x, xpad, partial, nch, gamma, beta, eps, silu, opad):
    """-> list of Guarded outputs (one; two for fp8: bytes, codes), already run"""
    B, HW, C = x.shape
    xb, ldx = rows_in(x, in_dt, xpad)
    pb, g, bt = partial_in(partial), gamma.to(DEV), beta.to(DEV)
    M = B * HW
    if out == "fp8":
        Q, Sc = R.guarded((M, C), C + opad, torch.uint8, DEV), R.guarded((M, C // 32), C // 32 + 3, torch.uint8, DEV)
        ok(L().rf_groupnorm_apply_fp8(xb.data_ptr(), B, HW, C, ldx, nch, pb.data_ptr(), g.data_ptr(), bt.data_ptr(), eps, silu, Q.ptr(), Q.ld, Sc.ptr(), Sc.ld, S()))
        return [Q, Sc]
    w = 2 * C if out == "split" else C
    O = R.guarded((M, w), w + opad, R.out_torch_dtype(out), DEV)
    ok(L().rf_groupnorm_apply(R.CODE[in_dt], xb.data_ptr(), B, HW, C, ldx, nch, pb.data_ptr(), g.data_ptr(), bt.data_ptr(), eps, silu, R.CODE[out], O.ptr(), O.ld, S()))
    return [O]


def compare_exact(tag, outs, out, y64):
    """y64 [M, C]: exact fp64 results that fp32 holds exactly -> the stored output must be their RNE, bit for bit"""
    y32 = y64.to(F32)
    assert torch.equal(y32.to(F64), y64), f"{tag}: the case is not exact in fp32"
    C = y64.shape[1]
    if out == "fp8":
        q, code = R.quant_act_np(y32.numpy())
        gq, gs = outs[0].fetch(tag).numpy(), outs[1].fetch(tag).numpy()
        assert np.array_equal(gs, code), f"{tag}: {int((gs != code).sum())} scale codes differ"
        assert np.array_equal(gq, q), f"{tag}: {int((gq != q).sum())} fp8 bytes differ"
        return
    got = outs[0].fetch(tag)
    if out == "split":
        ref = R.split_rows(y32, 2 * C)
        hi, lo = got[:, :C], got[:, C:]
        assert torch.equal(bits(hi), bits((hi.float() + lo.float()).to(BF16))), f"{tag}: hi != RNE_bf16(hi + lo)"
    else:
        ref = y32.to(out)
    assert torch.equal(bits(got), bits(ref)), f"{tag}: {int((bits(got) != bits(ref)).sum())} elements differ"


@pytest.mark.parametrize("pair", R.GN_PAIRS + [(BF16, "fp8")], ids=PID)
def test_b_apply_exact(pair):
    in_dt, out = pair
    for i, c in enumerate(R.apply_exact_cases(in_dt, out)):
        B, HW, C, nch = c["B"], c["HW"], c["C"], c["nchunks"]
        tag = f"apply {PID(pair)} B={B} HW={HW} C={C} nchunks={nch}"
        x = R.apply_exact_input(B, HW, C, 31 * i + C)
        mean, var = R.exact_means(B), torch.full((B, 32), 4.0, dtype=F64)
        part = R.exact_partials(mean, HW, C, nch, i)
        gamma, beta = R.exact_affine(C)
        outs = launch_apply(in_dt, out, x, c["xpad"], part, nch, gamma, beta, 0.0, 0, c["opad"])
        compare_exact(tag, outs, out, R.gn_apply_ref(x, mean, var, gamma, beta, 0.0, False).reshape(B * HW, C))


@pytest.mark.parametrize("pair,silu,eps", R.APPLY_RANDOM_CASES, ids=lambda v: PID(v) if isinstance(v, tuple) else str(v))
def test_c_apply_random_vs_fp64(pair, silu, eps):
    in_dt, out = pair
    for shape in R.APPLY_RANDOM_SHAPES:
        B, HW, C = shape["B"], shape["HW"], shape["C"]
        i = R.apply_random_inputs(pair, silu, eps, shape)
        mean, var = R.moments_of_partials(i["partial"], HW, C)
        xsc, msc, bb = R.gn_apply_terms(i["x"], mean, var, i["gamma"], i["beta"], eps)
        y = xsc - msc + bb
        ref = (R.silu64(y) if silu else y).reshape(B * HW, C)
        lim = R.tol_apply(y, xsc, msc, bb, out, silu).reshape(B * HW, C)
        tag = f"apply {PID(pair)} silu={silu} eps={eps} C={C}"
        got = launch_apply(in_dt, out, i["x"], 8, i["partial"], i["nchunks"], i["gamma"], i["beta"], eps, silu, 8)[0].fetch(tag)
        if out == "split":
            got = got[:, :C].to(F64) + got[:, C:].to(F64)          # (lo is itself rounded here: hi == RNE(hi + lo) is a property of the exact cases)
        e, ratio = worst(tag, got, ref, lim)
        assert ratio <= 1.0, f"{tag}: err/limit {ratio:.3f} (max err {e.max().item():.3e})"


# ------------------------------------------------------------------------------------------------ D: conditioning
def _gn_e32(x, gamma, beta, eps):
    """max error of PyTorch's fp32 CPU group_norm on the stored values x [B, HW, C] (fp64) against the fp64 reference"""
    ref = R.groupnorm_ref(x, gamma, beta, eps, False)
    y32 = Fn.group_norm(x.to(F32).permute(0, 2, 1).contiguous(), 32, gamma, beta, eps).permute(0, 2, 1)
    return ref, (y32.to(F64) - ref).abs().max().item()


@pytest.mark.parametrize("dt,ratio", [(dt, r) for dt in (F32, BF16, F16) for r in R.RATIOS[dt]], ids=str)
def test_d_groupnorm_conditioning(dt, ratio):
    B, H, C = 2, 9, 64
    x = R.conditioned((B, H * H, C), ratio, dt, 40 + ratio)
    gamma, beta = R.random_affine(C, 41)
    ref, e32 = _gn_e32(x, gamma, beta, 1e-5)
    xb, _ = rows_in(x, dt, 0)
    O = R.guarded((B * H * H, C), C + 8, dt, DEV)
    part = torch.empty(B * ops.GN_MAX_CHUNKS * 64, dtype=F64, device=DEV)
    ops.run(ops.groupnorm(xb.view(B, H, H, C), gamma.to(DEV), beta.to(DEV), O.view.view(B, H, H, C), part, eps=1e-5, silu=False))
    torch.cuda.synchronize()
    tag = f"groupnorm {dt} mean/std={ratio}"
    got = O.fetch(tag)
    e, r = worst(f"{tag} E32={e32:.3e}", got, ref.reshape(-1, C), R.tol_yardstick(ref.reshape(-1, C), dt, e32))
    if dt != F32:
        print(f"[norm] {tag}: kernel distance beyond one storage rounding {(e - R.STEP[dt] * ref.reshape(-1, C).abs()).clamp_min(0).max().item():.3e}")
    assert r <= 1.0, f"{tag}: err/limit {r:.3f}, max err {e.max().item():.3e}, E32 {e32:.3e}"


@pytest.mark.parametrize("dt,ratio", [(dt, r) for dt in (BF16, F16) for r in R.RATIOS[dt]], ids=str)
def test_d_groupnorm_conditioning_512_pixels_per_thread(dt, ratio):
    """nchunks = 1 at C = 2048, HW = 512: one pixel lane, 512 pixels per thread in the fp32 running sums (the most the product reaches).
    With plain fp32 sums of x and x^2 this case measured err / limit 6.6 (bf16, mean/std 8), 49 (bf16, 64), 1.2 (fp16, 8) and 14 (fp16, 64):
    the variance was lost in the sum of squares.  gn_stats_kernel now sums (x - K) and (x - K)^2, K = the thread's first pixel."""
    B, HW, C = 1, 512, 2048
    assert R.gn_geometry(dt, C)["PL"] == 1
    x = R.conditioned((B, HW, C), ratio, dt, 50 + ratio)
    gamma, beta = R.random_affine(C, 51)
    ref, e32 = _gn_e32(x, gamma, beta, 1e-5)
    xb, ldx = rows_in(x, dt, 0)
    P, O = R.guarded((1, 64), 64, F64, DEV), R.guarded((HW, C), C + 8, dt, DEV)
    g, bt = gamma.to(DEV), beta.to(DEV)
    ok(L().rf_groupnorm_stats(R.CODE[dt], xb.data_ptr(), B, HW, C, ldx, 1, P.ptr(), S()))
    ok(L().rf_groupnorm_apply(R.CODE[dt], xb.data_ptr(), B, HW, C, ldx, 1, P.ptr(), g.data_ptr(), bt.data_ptr(), 1e-5, 0, R.CODE[dt], O.ptr(), O.ld, S()))
    tag = f"groupnorm 512 px/thread {dt} mean/std={ratio}"
    P.fetch(tag)
    got = O.fetch(tag)
    e, r = worst(f"{tag} E32={e32:.3e}", got, ref[0], R.tol_yardstick(ref[0], dt, e32))
    print(f"[norm] {tag}: kernel distance beyond one storage rounding {(e - R.STEP[dt] * ref[0].abs()).clamp_min(0).max().item():.3e}")
    assert r <= 1.0, f"{tag}: err/limit {r:.3f}, max err {e.max().item():.3e}, E32 {e32:.3e}"


# ------------------------------------------------------------------------------------------------ E: LayerNorm
def launch_ln(in_dt, out, x, xpad, gamma, beta, eps, opad):
    M, C = x.shape
    xb, ldx = rows_in(x, in_dt, xpad)
    g, bt = gamma.to(DEV), beta.to(DEV)
    if out == "fp8":
        Q, Sc = R.guarded((M, C), C + opad, torch.uint8, DEV), R.guarded((M, C // 32), C // 32 + 3, torch.uint8, DEV)
        ok(L().rf_layernorm_fp8(xb.data_ptr(), M, C, ldx, g.data_ptr(), bt.data_ptr(), eps, Q.ptr(), Q.ld, Sc.ptr(), Sc.ld, S()))
        return [Q, Sc]
    w = 2 * C if out == "split" else C
    O = R.guarded((M, w), (w + 7) // 8 * 8 + opad, R.out_torch_dtype(out), DEV)
    ok(L().rf_layernorm(R.CODE[in_dt], xb.data_ptr(), M, C, ldx, g.data_ptr(), bt.data_ptr(), eps, R.CODE[out], O.ptr(), O.ld, S()))
    return [O]


@pytest.mark.parametrize("pair", R.LN_PAIRS + [(BF16, "fp8")], ids=PID)
def test_e_layernorm_exact(pair):
    in_dt, out = pair
    k = 0
    for C in (R.LN_C_FP8 if out == "fp8" else R.LN_C[in_dt]):
        gamma, beta = R.exact_affine(C)
        for M in R.LN_M:
            k += 1
            x, m, s = R.ln_exact_input(M, C, 7 * C + M)
            tag = f"layernorm {PID(pair)} M={M} C={C}"
            outs = launch_ln(in_dt, out, x, R.vec_of(in_dt) * (k % 3), gamma, beta, 0.0, 8 * (k % 3))
            compare_exact(tag, outs, out, s * gamma.to(F64) + beta.to(F64))


@pytest.mark.parametrize("pair", R.LN_PAIRS, ids=PID)
def test_e_layernorm_conditioning(pair):
    in_dt, out = pair
    for C in ([260, 1536] if in_dt == F32 else [520, 3072]):
        gamma, beta = R.random_affine(C, C)
        for ratio in (0, R.RATIOS[in_dt][-1]):
            x = R.conditioned((5, C), ratio, in_dt, C + ratio)
            ref = R.layernorm_ref(x, gamma, beta, 1e-5)
            e32 = (Fn.layer_norm(x.to(F32), (C,), gamma, beta, 1e-5).to(F64) - ref).abs().max().item()
            tag = f"layernorm {PID(pair)} C={C} mean/std={ratio}"
            got = launch_ln(in_dt, out, x, R.vec_of(in_dt), gamma, beta, 1e-5, 8)[0].fetch(tag)
            if out == "split":
                got = got[:, :C].to(F64) + got[:, C:].to(F64)
            e, r = worst(f"{tag} E32={e32:.3e}", got, ref, R.tol_yardstick(ref, out, e32))
            assert r <= 1.0, f"{tag}: err/limit {r:.3f}, max err {e.max().item():.3e}, E32 {e32:.3e}"


# ------------------------------------------------------------------------------------------------ F: fold
def launch_fold(W, bias, partial, nch, gamma, beta, eps, out_dt, B, HW):
    N, C = W.shape
    Wd, g, bt, pb = W.to(DEV), gamma.to(DEV), beta.to(DEV), partial_in(partial)
    bd = None if bias is None else bias.to(DEV)
    Wo, Rv = R.guarded((B * N, C), C, out_dt, DEV), R.guarded((B * N, 1), 1, F32, DEV)
    ok(L().rf_groupnorm_fold_linear(Wd.data_ptr(), N, C, B, HW, nch, pb.data_ptr(), g.data_ptr(), bt.data_ptr(), None if bd is None else bd.data_ptr(), eps,
                                    R.CODE[out_dt], Wo.ptr(), Rv.ptr(), S()))
    return Wo, Rv


@pytest.mark.parametrize("out_dt", R.FOLD_OUT, ids=str)
def test_f_fold_exact(out_dt):
    B, HW = R.FOLD_B, 16
    for i, (C, N, with_bias, nch) in enumerate(R.FOLD_CASES):
        tag = f"fold {out_dt} C={C} N={N} bias={with_bias}"
        W, bias = R.fold_exact_weights(N, C, 3 * C + N)
        bias = bias if with_bias else None
        gamma, beta = R.exact_affine(C)
        mean, var = R.exact_means(B), torch.full((B, 32), 4.0, dtype=F64)
        Wo, Rv = launch_fold(W, bias, R.exact_partials(mean, HW, C, nch, i), nch, gamma, beta, 0.0, out_dt, B, HW)
        wp, wps = R.fold_weights_ref(W, mean, var, gamma, 0.0, out_dt)
        assert torch.equal(wp, wps), f"{tag}: W' is not exact in {out_dt}"
        r, _ = R.fold_rowvec_ref(W, wps, mean, beta, bias)
        assert torch.equal(r.to(F32).to(F64), r)
        gw, gr = Wo.fetch(tag).reshape(B, N, C), Rv.fetch(tag).reshape(B, N)
        for s in range(B):
            assert torch.equal(bits(gw[s]), bits(wps[s].to(out_dt))), f"{tag}: W' of sample {s} differs"
            assert torch.equal(bits(gr[s]), bits(r[s].to(F32))), f"{tag}: row vector of sample {s} differs"


def test_f_fold_random_vs_fp64():
    """W' within one storage rounding + the three fp32 roundings of rstd, rstd gamma and the product (2^-22 relative); the row vector against the
    fp64 sum over the W' the kernel STORED: 2C + 1 terms summed in fp32 in some order, (2C + 2) 2^-24 sum |terms|, with the fp32 rounding of mean"""
    B, HW, C, N, out_dt = 3, 16, 544, 9, BF16
    g = R._gen(77)
    W, bias = torch.randn((N, C), generator=g), torch.randn((N,), generator=g)
    gamma, beta = R.random_affine(C, 78)
    n = float(HW * (C // 32))
    m0, v0 = 2.0 * torch.randn((B, 32), generator=g, dtype=F64), 0.5 + torch.rand((B, 32), generator=g, dtype=F64)
    part = torch.stack([n * m0, n * (v0 + m0 * m0)], -1)[:, None]
    mean, var = R.moments_of_partials(part, HW, C)
    Wo, Rv = launch_fold(W, bias, part, 1, gamma, beta, 1e-6, out_dt, B, HW)
    gw, gr = Wo.fetch("fold random").reshape(B, N, C), Rv.fetch("fold random").reshape(B, N)
    wp, _ = R.fold_weights_ref(W, mean, var, gamma, 1e-6, out_dt)
    e, r = worst("fold random W'", gw, wp, (R.STEP[out_dt] + 2.0 ** -22) * wp.abs() + 1e-30)
    assert r <= 1.0
    rr, mag = R.fold_rowvec_ref(W, gw.to(F64), mean, beta, bias)
    e, r = worst("fold random row vector", gr, rr, (2 * C + 2) * 2.0 ** -24 * mag)
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ G: softmax
@pytest.mark.parametrize("cols,pad", R.SOFTMAX_CASES)
def test_g_softmax_exact(cols, pad):
    x, ref = R.softmax_exact_input(R.SOFTMAX_ROWS, cols, cols)
    G = R.guarded((R.SOFTMAX_ROWS, cols), cols + pad, F32, DEV)
    G.view.copy_(x)
    G.before = G.buf.clone()
    ok(L().rf_softmax_rows(G.ptr(), R.SOFTMAX_ROWS, cols, G.ld, S()))
    got = G.fetch(f"softmax cols={cols}")
    assert torch.equal(bits(got), bits(ref)), f"softmax cols={cols}: {int((bits(got) != bits(ref)).sum())} elements differ"


# ------------------------------------------------------------------------------------------------ H: refusals
def _refusals():
    """(id, function name, call(lib, buffers)) -- every argument set fails an RF_CHECK of the host code, before any launch"""
    X3 = R.RF_BF16X3
    f32, b16, f16 = R.RF_F32, R.RF_BF16, R.RF_F16

    def apply(dtype, C, ldo, odt, nch=1, ldx=None):
        return lambda l, p: l.rf_groupnorm_apply(dtype, p["x"], 1, 4, C, ldx or C, nch, p["part"], p["g"], p["b"], 1e-5, 0, odt, p["out"], ldo, S())

    def ln(dtype, C, ldo, odt):
        return lambda l, p: l.rf_layernorm(dtype, p["x"], 2, C, C, p["g"], p["b"], 1e-5, odt, p["out"], ldo, S())

    return [
        ("apply C=48", "rf_groupnorm_apply", apply(b16, 48, 48, b16)),
        ("stats C=48", "rf_groupnorm_stats", lambda l, p: l.rf_groupnorm_stats(b16, p["x"], 1, 4, 48, 48, 1, p["out"], S())),
        ("fp8 C=48", "rf_groupnorm_apply_fp8", lambda l, p: l.rf_groupnorm_apply_fp8(p["x"], 1, 4, 48, 48, 1, p["part"], p["g"], p["b"], 1e-5, 0, p["out"], 48, p["out2"], 2, S())),
        ("layernorm_fp8 C=48", "rf_layernorm_fp8", lambda l, p: l.rf_layernorm_fp8(p["x"], 2, 48, 48, p["g"], p["b"], 1e-5, p["out"], 48, p["out2"], 2, S())),
        ("fold C=48", "rf_groupnorm_fold_linear", lambda l, p: l.rf_groupnorm_fold_linear(p["x"], 2, 48, 1, 4, 1, p["part"], p["g"], p["b"], None, 1e-5, b16, p["out"], p["out2"], S())),
        ("apply ldo=68", "rf_groupnorm_apply", apply(b16, 64, 68, b16)),
        ("layernorm ldo=68", "rf_layernorm", ln(b16, 64, 68, b16)),
        ("apply split from bf16", "rf_groupnorm_apply", apply(b16, 64, 128, X3)),
        ("apply split from f16", "rf_groupnorm_apply", apply(f16, 64, 128, X3)),
        ("apply split ldo<2C", "rf_groupnorm_apply", apply(f32, 64, 120, X3)),
        ("layernorm split from bf16", "rf_layernorm", ln(b16, 64, 128, X3)),
        ("layernorm split ldo<2C", "rf_layernorm", ln(f32, 64, 120, X3)),
        ("apply bf16->f16", "rf_groupnorm_apply", apply(b16, 64, 64, f16)),
        ("apply f32->f16", "rf_groupnorm_apply", apply(f32, 64, 64, f16)),
        ("layernorm bf16->f16", "rf_layernorm", ln(b16, 64, 64, f16)),
        ("layernorm f32->f16", "rf_layernorm", ln(f32, 64, 64, f16)),
        ("stats C=4128 (LDS)", "rf_groupnorm_stats", lambda l, p: l.rf_groupnorm_stats(b16, p["x"], 1, 4, 4128, 4128, 1, p["out"], S())),
        ("fold C=1568", "rf_groupnorm_fold_linear", lambda l, p: l.rf_groupnorm_fold_linear(p["x"], 2, 1568, 1, 4, 1, p["part"], p["g"], p["b"], None, 1e-5, b16, p["out"], p["out2"], S())),
        ("softmax cols=6", "rf_softmax_rows", lambda l, p: l.rf_softmax_rows(p["out"], 2, 6, 8, S())),
        ("stats nchunks=0", "rf_groupnorm_stats", lambda l, p: l.rf_groupnorm_stats(b16, p["x"], 1, 4, 64, 64, 0, p["out"], S())),
        ("apply nchunks=0", "rf_groupnorm_apply", apply(b16, 64, 64, b16, nch=0)),
        ("fp8 nchunks=0", "rf_groupnorm_apply_fp8", lambda l, p: l.rf_groupnorm_apply_fp8(p["x"], 1, 4, 64, 64, 0, p["part"], p["g"], p["b"], 1e-5, 0, p["out"], 64, p["out2"], 2, S())),
        ("fold nchunks=0", "rf_groupnorm_fold_linear", lambda l, p: l.rf_groupnorm_fold_linear(p["x"], 2, 64, 1, 4, 0, p["part"], p["g"], p["b"], None, 1e-5, b16, p["out"], p["out2"], S())),
        ("finalize nchunks=0", "rf_groupnorm_finalize", lambda l, p: l.rf_groupnorm_finalize(p["part"], 1, 0, p["out"], S())),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_h_refused_before_any_launch(case):
    _, fn, call = case
    x = torch.zeros(4 * 8192, dtype=F32, device=DEV)
    part = torch.zeros(64, dtype=F64, device=DEV)
    g, b = torch.ones(8192, dtype=F32, device=DEV), torch.zeros(8192, dtype=F32, device=DEV)
    O, O2 = R.guarded((64, 256), 256, F32, DEV, live_rows=0), R.guarded((64, 256), 256, F32, DEV, live_rows=0)
    rc = call(L(), dict(x=x.data_ptr(), part=part.data_ptr(), g=g.data_ptr(), b=b.data_ptr(), out=O.ptr(), out2=O2.ptr()))
    torch.cuda.synchronize()
    assert rc != 0, f"{case[0]}: accepted"
    assert err().startswith(fn + ":"), f"{case[0]}: rf_last_error = {err()!r}"
    O.check(case[0])
    O2.check(case[0])
