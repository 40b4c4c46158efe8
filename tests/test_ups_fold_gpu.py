"""Nearest-2x upsampling folded into 2x2 phase weights (rf_conv_gemm ups = 2, ops.fold_ups_weight, UNetEngine's Upsample convolutions).

Reference: F.conv2d(F.interpolate(x, 2, "nearest"), w, b, padding=1) in fp64 (evaluated as im2col + matmul on the device) on the 16-bit-rounded input and the fp32 MASTER weights -- the
two launches round the weights in their own ways (ups = 1: every tap once; ups = 2: every folded sum of up to four taps once), so neither
owns "the rounded weights".  The existing ups = 1 launch is measured against that reference in the same test and the folded launch may be
at most 2x further on the maximum and on the RMS error: same products, fp32 accumulation in another order, one rounding of the output.
Every launch writes a channel slice of a wider buffer (ldo > N) whose other columns are pre-filled and must stay untouched.

Measured on an MI355X (folded / ups = 1, max and RMS error against the fp64 reference): see profiles/ups_fold_ab.txt.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from reface_amd import _lib, ops
from reface_amd.params import seeded_randn as rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 3.0


def _case(dt, B, H, W, Ci, Co, seed):
    x = rnd((B, H, W, Ci), seed).to(dt)
    w = rnd((Co, Ci, 3, 3), seed + 1) / math.sqrt(9 * Ci)
    b = rnd((Co,), seed + 2)
    # fp64 on the device as im2col + matmul: what F.conv2d(F.interpolate(x, 2, "nearest"), w, b, padding=1) computes, with no library heuristics in between
    a = F.unfold(F.interpolate(x.to(DEV).double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest"), 3, padding=1)          # [B, Ci * 9, 4 H W], K order (c, ky, kx)
    ref = (torch.matmul(w.to(DEV).double().reshape(Co, Ci * 9), a).permute(0, 2, 1) + b.to(DEV).double()).reshape(B, 2 * H, 2 * W, Co)
    return x.to(DEV), w, b.to(DEV), ref


def _wide(dt, B, H, W, Co, pre=32, post=32):
    """[B, 2H, 2W, pre + Co + post] pre-filled; the launch writes columns [pre, pre + Co)."""
    return torch.full((B, 2 * H, 2 * W, pre + Co + post), FILL, dtype=dt, device=DEV)


def _errs(buf, pre, Co, ref):
    assert (buf[..., :pre] == FILL).all() and (buf[..., pre + Co:] == FILL).all(), "columns outside the slice were written"
    d = buf[..., pre:pre + Co].double() - ref
    assert torch.isfinite(d).all()
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _both(dt, B, H, W, Ci, Co, seed):
    """-> (folded launch, its buffer, ups = 1 buffer, reference): both launches prepared on the same operands, the ups = 1 one already run."""
    x, w, b, ref = _case(dt, B, H, W, Ci, Co, seed)
    y1, y2 = _wide(dt, B, H, W, Co), _wide(dt, B, H, W, Co)
    ops.conv2d(x, ops.pack_conv_weight(w, dt).to(DEV), y1[..., 32:32 + Co], b, ups=1, name="ups1")()
    l2 = ops.conv2d(x, ops.pack_ups_weight(w, dt).to(DEV), y2[..., 32:32 + Co], b, ups=2, name="ups2")
    return l2, y2, y1, ref


CASES = [
    pytest.param(torch.bfloat16, 2, 16, 16, 128, 320, id="bf16_2x16x16_128to320"),          # Hin Win = 256: whole tiles per phase and sample, direct epilogue
    pytest.param(torch.bfloat16, 3, 16, 32, 64, 64, id="bf16_3x16x32_64to64"),              # non-square, N below a tile, odd sample count, staged epilogue
    pytest.param(torch.float16, 3, 16, 32, 64, 64, id="fp16_3x16x32_64to64"),
    pytest.param(torch.bfloat16, 6, 32, 8, 64, 64, id="bf16_6x32x8_64to64"),               # same GEMM, 8-pixel source rows: a staged-epilogue thread's rows lie whole source rows apart
    pytest.param(torch.bfloat16, 3, 64, 64, 64, 320, id="bf16_3x64x64_64to320_256x320_tiles"),   # 192 tiles of 256 x 320: the 8-wave tile of the full-size UNet
]


@pytest.mark.parametrize("dt,B,H,W,Ci,Co", CASES)
def test_folded_launch_not_further_from_fp64_than_ups1(dt, B, H, W, Ci, Co):
    l2, y2, y1, ref = _both(dt, B, H, W, Ci, Co, 4100)
    pl = ops.gemm_plan2(l2)
    assert pl["splitk"] == 1 and (H * W) % pl["bm"] == 0, pl
    l2()
    torch.cuda.synchronize()
    m1, r1 = _errs(y1, 32, Co, ref)
    m2, r2 = _errs(y2, 32, Co, ref)
    print(f"ups fold M={4 * B * H * W} N={Co} K={4 * Ci} [{dt}] tile {pl['bm']}x{pl['bn']} direct {pl['direct']}: max err folded {m2:.4e} / ups1 {m1:.4e}, "
          f"rms folded {r2:.4e} / ups1 {r1:.4e} (ref absmax {ref.abs().max().item():.3f})")
    assert m2 <= 2.0 * m1 and r2 <= 2.0 * r1, (m2, m1, r2, r1)


def test_fused_groupnorm_statistics_two_consumers():
    """B = 2, 32x32 -> 64x64, C 64 -> 160 into columns [160, 320) of a concat buffer whose first half a 1x1 GEMM writes: the folded launch emits the
    statistics of the whole buffer (10 channels per group) and of its own half (5 per group).  Both against fp64 sums of the tensor AS STORED.
    Bound: a tile's rows (<= 256) and a group's columns are summed in fp32 before the fp64 slots: |error| <= n u sum|v| with n <= 256 + 32 additions
    per chain and u = 2^-24, i.e. 1.8e-5 sum|v| (sums) resp. 1.8e-5 sum v^2 plus one more rounding per square (squares): 2e-5 is asserted."""
    dt, B, H, W, Ci, Co = torch.bfloat16, 2, 32, 32, 64, 160
    x, w, b, ref = _case(dt, B, H, W, Ci, Co, 4200)
    buf = torch.full((B, 2 * H, 2 * W, 2 * Co + 32), FILL, dtype=dt, device=DEV)
    cat = buf[..., :2 * Co]
    xin = rnd((B, 2 * H, 2 * W, 64), 4203).to(dt).to(DEV)
    w1 = (rnd((Co, 64), 4204) / 8).to(dt).to(DEV)
    b1 = rnd((Co,), 4205).to(DEV)
    l1 = ops.conv2d(xin, w1, cat[..., :Co], b1, ksize=1, pad=(0, 0), name="half0")
    l2 = ops.conv2d(x, ops.pack_ups_weight(w, dt).to(DEV), cat[..., Co:], b, ups=2, name="ups2")
    M = 4 * B * H * W
    whole = ops.fuse_groupnorm_stats(cat, [(l1, 0, M, 0, Co), (l2, 0, M, Co, Co)])
    own = ops.fuse_groupnorm_stats(cat[..., Co:], [(l2, 0, M, 0, Co)])
    assert whole is not None and own is not None and l2.keep[0].gn_part0 and l2.keep[0].gn_part1
    ops.run([l1, l2] + whole[2] + own[2])
    # the same two launches without statistics, each into a buffer of its own: what l1 alone writes, and the ups = 1 launch as the error yardstick
    alone = torch.full((B, 2 * H, 2 * W, Co + 32), FILL, dtype=dt, device=DEV)
    ops.conv2d(xin, w1, alone[..., :Co], b1, ksize=1, pad=(0, 0), name="half0_alone")()
    y1 = _wide(dt, B, H, W, Co)
    ops.conv2d(x, ops.pack_conv_weight(w, dt).to(DEV), y1[..., 32:32 + Co], b, ups=1, name="ups1")()
    torch.cuda.synchronize()
    assert (buf[..., 2 * Co:] == FILL).all() and (alone[..., Co:] == FILL).all()
    assert torch.equal(cat[..., :Co], alone[..., :Co]), "the folded launch changed the half of the buffer that the 1x1 GEMM writes"
    # the pixel mapping of this epilogue (statistics on: values kept as stored): the same 2x bound against the ups = 1 launch as above
    m1, r1 = _errs(y1, 32, Co, ref)
    d = cat[..., Co:].double() - ref
    assert torch.isfinite(d).all()
    m2, r2 = d.abs().max().item(), d.pow(2).mean().sqrt().item()
    pl = ops.gemm_plan2(l2)
    print(f"ups fold + GroupNorm statistics M={M} N={Co} K={4 * Ci} tile {pl['bm']}x{pl['bn']} direct {pl['direct']}: max err folded {m2:.4e} / ups1 {m1:.4e}, "
          f"rms folded {r2:.4e} / ups1 {r1:.4e}")
    assert m2 <= 2.0 * m1 and r2 <= 2.0 * r1, (m2, m1, r2, r1)
    for name, (part, n, _), t in (("whole", whole, cat), ("own", own, cat[..., Co:])):
        v = t.double().cpu().reshape(B, 4 * H * W, 32, -1)                   # [B, pixels, group, channels of the group]
        want = torch.stack([v.sum((1, 3)), v.pow(2).sum((1, 3))], -1)        # [B, 32, 2]
        mag = torch.stack([v.abs().sum((1, 3)), v.pow(2).sum((1, 3))], -1)
        got = part.reshape(B, n, 32, 2).sum(1).cpu()
        rel = ((got - want).abs() / mag).max().item()
        print(f"  {name}: {n} slot(s) per sample, max |sum error| / sum of magnitudes {rel:.3e}")
        assert rel <= 2e-5, (name, rel)


def test_ineligible_requests_are_refused():
    """An 8x8 source (Hin Win = 64, below every tile) and descriptors outside the folded form return the library's error and launch nothing."""
    dt = torch.bfloat16
    x, w, b, _ = _case(dt, 2, 8, 8, 64, 64, 4300)
    y = _wide(dt, 2, 8, 8, 64)
    small = ops.conv2d(x, ops.pack_ups_weight(w, dt).to(DEV), y[..., 32:96], b, ups=2, name="ups2_8x8")
    with pytest.raises(_lib.RefaceHipError, match="multiple of the"):
        small()
    with pytest.raises(_lib.RefaceHipError):
        ops.gemm_plan2(small)
    x, w, b, _ = _case(dt, 2, 16, 16, 64, 64, 4310)
    y16 = _wide(dt, 2, 16, 16, 64)
    res = torch.zeros((2, 32, 32, 64), dtype=dt, device=DEV)
    rv = torch.zeros((2, 64), dtype=torch.float32, device=DEV)

    def launch():
        return ops.conv2d(x, ops.pack_ups_weight(w, dt).to(DEV), y16[..., 32:96], b, ups=2, name="bad")
    ops.gemm_plan2(launch())              # (the unmutated descriptor is a valid one)
    mutations = {"fp32 operands": dict(dtype=_lib.RF_F32), "split-bf16 operands": dict(dtype=_lib.RF_BF16X3), "fp8 activations": dict(dtype=_lib.RF_FP8_E4M3),
                 "fp8 weights": dict(w_dtype=_lib.RF_FP8_E4M3), "3x3 window": dict(KH=3, KW=3, K=9 * 64), "stride 2": dict(stride=2), "pad 0": dict(pad_t=0),
                 "two sources": dict(C1=64), "batched": dict(batch=2), "residual": dict(residual=res.data_ptr(), ldr=64),
                 "rowvec": dict(rowvec=rv.data_ptr(), ldv=64), "korder 2": dict(korder=2), "GEGLU": dict(act=ops.ACT_GEGLU), "output not 2x": dict(Hout=16, Wout=16, M=2 * 256),
                 "ups 3": dict(ups=3)}
    for what, fields in mutations.items():
        l = launch()
        for f, v in fields.items():
            setattr(l.keep[0], f, v)
        with pytest.raises(_lib.RefaceHipError):
            l()
        with pytest.raises(_lib.RefaceHipError):
            ops.gemm_plan2(l)
    torch.cuda.synchronize()
    assert (y == FILL).all() and (y16 == FILL).all()


def test_unet_engine_folds_the_eligible_upsamples(monkeypatch):
    """Reduced-width UNet (64 channels, multipliers 1 2 4 4) at 64x64 latents, one CFG pair, bf16: every `up` layer whose folded descriptor the library
    accepts (asked here with stand-alone launches of the layer's shape) is folded, the others keep ups = 1, and the result matches the engine built
    with REFACE_UPS_FOLD=0 to the bound the bf16 engine has against the oracle elsewhere in the suite (rel L2 0.02): both are bf16 evaluations of the
    same network that differ in the rounding of the Upsample weights and the summation order."""
    from reface_amd import params as P
    from reface_amd.unet import UNetModel
    dt, hw = torch.bfloat16, 64
    m = UNetModel(image_size=32, use_spatial_transformer=True, transformer_depth=1, use_checkpoint=True, legacy=False, in_channels=9, model_channels=64,
                  out_channels=4, num_res_blocks=2, attention_resolutions=(4, 2, 1), channel_mult=(1, 2, 4, 4), num_heads=8, context_dim=768)
    m.load_state_dict(P.seeded_state_dict(P.unet_param_specs(m.cfg), 7), strict=True)
    m.to(DEV)
    m.set_compute_dtype(dt)
    x, t, ctx = rnd((1, 9, hw, hw), 4400).repeat(2, 1, 1, 1), torch.tensor([500, 500]), rnd((2, 1, 768), 4401)
    # the `up` layers of this model: (channels, source size), from 8x8 upwards
    want = 0
    for c, s in ((256, 8), (256, 16), (128, 32)):
        cand = ops.conv2d(torch.zeros((2, s, s, c), dtype=dt, device=DEV), torch.zeros((4, c, 4 * c), dtype=dt, device=DEV),
                          torch.zeros((2, 2 * s, 2 * s, c), dtype=dt, device=DEV), None, ups=2)
        try:
            ops.gemm_plan2(cand)
            want += 1
        except _lib.RefaceHipError:
            pass
    assert want >= 1
    outs = {}
    try:
        for flag in ("1", "0"):
            monkeypatch.setenv("REFACE_UPS_FOLD", flag)
            m._engines.clear()
            eng = m.engine(2, hw, hw, uniform_t=True, cfg_pair=True)
            ups = [l.keep[0].ups for l in eng.main if l.fn.__name__ == "rf_conv_gemm" and l.keep[0].ups]
            assert len(ups) == 3 and eng.n_ups_folded == ups.count(2) == (want if flag == "1" else 0), (flag, ups, eng.n_ups_folded, want)
            ops.nchw_to_nhwc(x.to(DEV), eng.x_in)()
            eng.set_context(ctx.to(DEV))
            eng.set_timesteps(t[:1].to(DEV))
            eng.run()
            out = torch.empty((2, 4, hw, hw), dtype=torch.float32, device=DEV)
            ops.nhwc_to_nchw(eng.eps, out)()
            torch.cuda.synchronize()
            outs[flag] = out.cpu()
            del eng
    finally:
        m._engines.clear()
    rel = ((outs["1"] - outs["0"]).norm() / outs["0"].norm()).item()
    print(f"reduced-width UNet, {want} of 3 Upsample convolutions folded: rel L2 folded vs REFACE_UPS_FOLD=0 {rel:.5f}")
    assert torch.isfinite(outs["1"]).all() and rel < 0.02, rel
