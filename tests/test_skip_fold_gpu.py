"""The ResBlock skip convolution folded into the second 3x3 conv's K loop (rf_conv_gemm_desc.srcx, UNetEngine._res).

    y = conv3x3(t2; W2) + b2 + x Wsk^T + bsk  =  [ im2col(t2) | x ] [ W2 | Wsk ]^T + (b2 + bsk)

Op level: the folded launch, the chain it replaces (1x1 launch, then the 3x3 launch with `residual`) and an fp64 reference, all on the same
16-bit-rounded operands, at the shapes the benchmark's step runs (CFG batch 16 at 64x64 latents, CFG batch 8 at 96x96).  The folded result
may not be further from the reference than the chain is, times 1.1: the fold removes one 16-bit rounding (of `skip`), the 10 % covers fp32
reassociation under a different split-K plan.  Structure checks without a tolerance, the fused GroupNorm statistics, the engine against the CPU
oracle, and the descriptors the library must refuse.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from reface_amd import _lib, ops
from reface_amd.params import seeded_randn as rnd

from test_fullsize_gpu import _oracle_pair, _oracle_plan, _pair_inputs, full_unet  # noqa: F401  (the full-width model fixture and the oracle cache)
from test_ops_gpu import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
H16 = [torch.bfloat16, torch.float16]


def _operands(dt, B, H, W, cout, cin, seed):
    """16-bit-rounded device operands of one block tail + their fp32 parameters."""
    t2 = rnd((B, H, W, cout), seed).to(dt).to(DEV)
    x = rnd((B, H, W, cin), seed + 1).to(dt).to(DEV)
    w2 = (rnd((cout, cout, 3, 3), seed + 2) / math.sqrt(9 * cout)).to(dt).to(DEV)
    wsk = (rnd((cout, cin), seed + 3) / math.sqrt(cin)).to(dt).to(DEV)
    b2, bsk = rnd((cout,), seed + 4).to(DEV), rnd((cout,), seed + 5).to(DEV)
    return t2, x, w2, wsk, b2, bsk


def _reference(t2, x, w2, wsk, b2, bsk):
    """fp64 on the device: im2col + matmul (what F.conv2d(t2, W2, padding=1) + F.conv2d(x, Wsk) computes, with no library heuristics in between)."""
    B, H, W, cout = t2.shape
    a = F.unfold(t2.permute(0, 3, 1, 2).double(), 3, padding=1)                 # [B, cout * 9, H * W], K order (c, ky, kx)
    y = torch.matmul(w2.double().reshape(cout, cout * 9), a).permute(0, 2, 1)   # [B, HW, cout]
    y = y + torch.matmul(x.double().reshape(B, H * W, -1), wsk.double().t()) + (b2 + bsk).double()
    return y.reshape(B, H, W, cout)


def _korder(ko, t2, w2, out, tail_w=None, tail=None, **kw):
    """The launch in the K order `ko` ("auto": row-extended A tiles where the library's plan takes them, else tap-major -- what the engine does)."""
    def make(k):
        wp = ops.pack_conv_weight(w2, t2.dtype, korder=k)
        if tail is not None:
            wp = ops.pack_conv_tail(wp, tail_w)
        return ops.conv2d(t2, wp, out, korder=k, tail=tail, **kw)
    if ko != "auto":
        return make(ko), ko
    cand = make(2)
    try:
        ops.gemm_plan2(cand)
        return cand, 2
    except _lib.RefaceHipError:
        return make(0), 0


def _fold_and_chain(dt, B, H, W, cout, cin, ko, seed, slices=None):
    t2, x, w2, wsk, b2, bsk = _operands(dt, B, H, W, cout, cin, seed)
    ref = _reference(t2, x, w2, wsk, b2, bsk)
    y_f = torch.empty((B, H, W, cout), dtype=dt, device=DEV)
    y_c = torch.empty_like(y_f)
    skip = torch.empty_like(y_f)
    bsum = (b2 + bsk).contiguous()
    plans = []
    for a, b in (slices or [(0, B)]):
        lf, k = _korder(ko, t2[a:b], w2, y_f[a:b], tail_w=wsk, tail=x[a:b], bias=bsum, name="fold")
        l1 = ops.conv2d(x[a:b], wsk, skip[a:b], bsk, ksize=1, pad=(0, 0), name="skip")
        lc, kc = _korder(ko, t2[a:b], w2, y_c[a:b], bias=b2, residual=skip[a:b], name="chain")
        ops.run([lf, l1, lc])
        plans.append((k, ops.gemm_plan2(lf), kc, ops.gemm_plan2(lc)))
    torch.cuda.synchronize()
    rel = lambda y: ((y.double() - ref).norm() / ref.norm()).item()
    return rel(y_f), rel(y_c), plans, y_f


# (B, H, W, cout, cin, K order asked, K order the folded launch must end up with or None, its split-K: "split" / a number / None, sample slices)
CASES = [
    pytest.param(16, 64, 64, 320, 960, "auto", 2, None, None, id="65536x320_K2880+960"),
    pytest.param(16, 64, 64, 320, 640, "auto", 2, None, None, id="65536x320_K2880+640"),
    pytest.param(16, 32, 32, 640, 1920, "auto", 2, None, None, id="16384x640_K5760+1920"),
    pytest.param(16, 32, 32, 640, 320, "auto", 2, None, None, id="16384x640_K5760+320"),
    pytest.param(16, 16, 16, 1280, 2560, "auto", 2, "split", None, id="4096x1280_K11520+2560_splitk"),
    pytest.param(16, 16, 16, 1280, 640, "auto", 2, "split", None, id="4096x1280_K11520+640_splitk"),
    pytest.param(16, 8, 8, 1280, 2560, "auto", 0, 8, None, id="1024x1280_K11520+2560_splitk8_plain_tiles"),
    pytest.param(8, 96, 96, 320, 640, "auto", None, None, None, id="73728x320_quarter_tiles"),
    pytest.param(8, 96, 96, 320, 960, "auto", None, None, [(0, 7), (7, 8)], id="73728x320_sample_split_7+1"),
    pytest.param(8, 48, 48, 640, 960, "auto", None, None, None, id="18432x640_K5760+960"),
    pytest.param(13, 63, 64, 320, 640, "auto", 2, None, None, id="52416x320_ragged_M_row_extended"),
    pytest.param(1, 20, 16, 320, 640, "auto", None, None, None, id="320x320_ragged_M_small"),
    pytest.param(1, 24, 24, 320, 640, "auto", 0, None, None, id="576x320_ragged_M_plain_tiles"),
    pytest.param(16, 32, 32, 640, 960, 0, 0, None, None, id="16384x640_tap_major"),
    pytest.param(16, 16, 16, 1280, 1920, 0, 0, "split", None, id="4096x1280_tap_major_splitk"),
    pytest.param(16, 32, 32, 640, 1280, 1, 1, None, None, id="16384x640_chunk_major"),
]


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("B,H,W,cout,cin,ko,want_k,want_sk,slices", CASES)
def test_fold_not_further_from_fp_reference_than_chain(dt, B, H, W, cout, cin, ko, want_k, want_sk, slices):
    e_fold, e_chain, plans, _ = _fold_and_chain(dt, B, H, W, cout, cin, ko, 700, slices)
    for k, pf, kc, pc in plans:
        print(f"  fold: korder {k} tile {pf['bm']}x{pf['bn']} splitk {pf['splitk']} direct {pf['direct']} | chain: korder {kc} tile {pc['bm']}x{pc['bn']} splitk {pc['splitk']}")
    print(f"M={B * H * W} N={cout} K={9 * cout}+{cin} [{dt}]: rel L2 vs fp64  fold {e_fold:.4e}  chain {e_chain:.4e}  ratio {e_fold / e_chain:.3f}")
    if want_sk == "split":
        assert plans[0][1]["splitk"] > 1, plans[0][1]
    elif want_sk is not None:
        assert plans[0][1]["splitk"] == want_sk, plans[0][1]
    if want_k is not None:
        assert plans[0][0] == want_k, f"this case is meant to cover K order {want_k} (2 = row-extended A tiles), the library planned {plans[0][0]}"
    assert math.isfinite(e_fold) and e_fold <= 1.1 * e_chain, (e_fold, e_chain)


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("B,H,W,cout,cin,ko", [(16, 64, 64, 320, 960, "auto"), (16, 32, 32, 640, 1920, "auto"), (16, 32, 32, 640, 320, 0), (4, 16, 16, 1280, 2560, "auto"),
                                               (1, 24, 24, 320, 640, "auto")])
def test_zero_tail_is_bit_identical_to_plain_conv(dt, B, H, W, cout, cin, ko):
    """Wsk = 0, bsk = 0: the tail tiles add exact zeros behind the window's tiles -- same bits as the convolution alone, wherever both run
    on the same tile plan without split-K (a K split moves the slice boundaries with K, and with them the fp32 summation order)."""
    t2, x, w2, wsk, b2, _ = _operands(dt, B, H, W, cout, cin, 720)
    y_f = torch.empty((B, H, W, cout), dtype=dt, device=DEV)
    y_p = torch.empty_like(y_f)
    lf, k = _korder(ko, t2, w2, y_f, tail_w=torch.zeros_like(wsk), tail=x, bias=b2, name="fold0")
    lp, kp = _korder(ko, t2, w2, y_p, bias=b2, name="plain")
    for l_ in (lf, lp):          # no split-K scratch: both launches then run whole K loops on one tile plan, at every shape -- the bitwise statement always applies
        l_.keep[0].workspace, l_.keep[0].workspace_bytes = None, 0
    pf, pp = ops.gemm_plan2(lf), ops.gemm_plan2(lp)
    assert k == kp and pf == pp and pf["splitk"] == 1, f"different plans (fold korder {k} {pf}, plain korder {kp} {pp}): the bitwise case lost its plan"
    ops.run([lf, lp])
    torch.cuda.synchronize()
    assert torch.equal(y_f.view(torch.int16), y_p.view(torch.int16))


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("B,H,W,cout,cin", [(16, 64, 64, 320, 960), (16, 16, 16, 1280, 2560), (16, 32, 32, 640, 1280)])
def test_fused_groupnorm_statistics_of_folded_launch(dt, B, H, W, cout, cin):
    """The folded launch as the producer of a GroupNorm's statistics (direct epilogue and split-K reduce pass): the normalised tensor against
    torch's group_norm of the STORED output, to the tolerance of test_groupnorm_stats_fused_into_gemm."""
    t2, x, w2, wsk, b2, bsk = _operands(dt, B, H, W, cout, cin, 740)
    y = torch.empty((B, H, W, cout), dtype=dt, device=DEV)
    lf, _ = _korder("auto", t2, w2, y, tail_w=wsk, tail=x, bias=(b2 + bsk).contiguous(), name="fold")
    fused = ops.fuse_groupnorm_stats(y, [(lf, 0, B * H * W, 0, cout)])
    assert fused is not None
    ops.run([lf] + fused[2])
    g, be = rnd((cout,), 746) * 0.2 + 1, rnd((cout,), 747) * 0.2
    out = torch.empty_like(y)
    ops.groupnorm_apply(y, g.to(DEV), be.to(DEV), out, fused[0], fused[1], eps=1e-5, silu=True)()
    torch.cuda.synchronize()
    ref = F.silu(F.group_norm(y.float().cpu().permute(0, 3, 1, 2), 32, g, be, 1e-5)).permute(0, 2, 3, 1)
    check(out, ref, dt)


def test_tail_source_rejected_where_not_built():
    """fp8 / split-bf16 operands, fp8 weights, a strided window, a second window source: rf_conv_gemm returns an error and launches nothing."""
    dt = torch.bfloat16
    t2, x, w2, wsk, b2, bsk = _operands(dt, 2, 16, 16, 320, 640, 760)
    y = torch.full((2, 16, 16, 320), 7.0, dtype=dt, device=DEV)
    wp = ops.pack_conv_tail(ops.pack_conv_weight(w2, dt), wsk)

    def launch():
        return ops.conv2d(t2, wp, y, (b2 + bsk).contiguous(), tail=x, name="bad")
    mutations = {"fp8 activations": dict(dtype=_lib.RF_FP8_E4M3), "split-bf16 operands": dict(dtype=_lib.RF_BF16X3), "fp8 weights": dict(w_dtype=_lib.RF_FP8_E4M3),
                 "stride 2": dict(stride=2), "upsampled window": dict(ups=1), "two window sources": dict(C1=64), "batched": dict(batch=2),
                 "ragged tail": dict(Cx=72, K=9 * 320 + 72)}
    ok = launch()
    ops.gemm_plan2(ok)                    # (the unmutated descriptor is a valid one)
    for what, fields in mutations.items():
        l = launch()
        for f, v in fields.items():
            setattr(l.keep[0], f, v)
        with pytest.raises(_lib.RefaceHipError):
            l()
        with pytest.raises(_lib.RefaceHipError):
            ops.gemm_plan2(l)
        torch.cuda.synchronize()
        assert (y == 7.0).all(), what
    ok()
    torch.cuda.synchronize()
    assert not (y == 7.0).all()


@pytest.mark.parametrize("hw", [64, 96])
def test_unet_engine_folds_all_14_skips(full_unet, hw):
    """Full-width UNet, one CFG pair, bf16 and fp16 against oracle.unet.unet_forward under the bounds test_fullsize_gpu.py uses for these modes;
    every ResBlock whose channel count changes (input_blocks.4 / .7 and the twelve output_blocks) runs its skip inside out_layers.3."""
    m, sd = full_unet
    plan = _oracle_plan(sd, m.cfg)
    x, t, ctx = _pair_inputs(hw)
    ref = _oracle_pair(sd, plan, hw)
    scale = ref.abs().max().item()
    try:
        for dt, lim in ((torch.bfloat16, 0.02), (torch.float16, 0.004)):
            m.set_compute_dtype(dt)
            eng = m.engine(2, hw, hw, uniform_t=True, cfg_pair=True)
            ops.nchw_to_nhwc(x.to(DEV), eng.x_in)()
            eng.set_context(ctx.to(DEV))
            eng.set_timesteps(t[:1].to(DEV))
            eng.run()
            out = torch.empty((2, 4, hw, hw), dtype=torch.float32, device=DEV)
            ops.nhwc_to_nchw(eng.eps, out)()
            torch.cuda.synchronize()
            out = out.cpu()
            rel = ((out - ref).norm() / ref.norm()).item()
            emax = (out - ref).abs().max().item()
            print(f"UNet {hw}x{hw} [{dt}] with folded skips: rel L2 {rel:.5f}, max |d| {emax:.5f} of {scale:.2f}; {len(eng.main)} launches")
            assert torch.isfinite(out).all() and rel < lim and emax < 6.0 * lim * scale, (dt, rel, emax, scale)
            assert eng.n_skip_folded == 14, eng.n_skip_folded
            assert not [l.name for l in eng.main if l.name.endswith(".skip_connection")]
            folded = [l for l in eng.main if l.fn.__name__ == "rf_conv_gemm" and l.keep[0].srcx]
            assert len(folded) >= 14 and all(l.keep[0].residual is None for l in folded)
            m._engines.clear()
            del eng
            torch.cuda.empty_cache()
    finally:
        m._engines.clear()
        m.set_compute_dtype(torch.float32)


def test_fp32_engine_keeps_the_chain(full_unet):
    """The exact-fp32 mode has no tail source: its 14 skip convolutions stay launches of their own."""
    m, _ = full_unet
    m.set_compute_dtype(torch.float32)
    eng = m.engine(2, 32, 32, uniform_t=True, cfg_pair=True)
    try:
        assert eng.n_skip_folded == 0 and len([l for l in eng.main if l.name.endswith(".skip_connection")]) == 14
    finally:
        m._engines.clear()
        del eng
        torch.cuda.empty_cache()
