"""The fp16 precision mode's kernels at the edges of fp16's range (tests/f16_range_cases.py): fp16 subnormal operands into the f16 MFMA (S-in),
results in the fp16 store band around the subnormals (S-out) and around 65504 (TOP).  The mode rests on three properties -- the f16 MFMA takes
subnormal A / B operands un-flushed, every 16-bit store rounds to nearest-even with gradual underflow, overflow becomes +-inf as Tensor.to(float16)
does -- and a changed compile flag, a truncating packed conversion, a clamp or a flushed P operand breaks one of them without any other suite
noticing.

rf_conv_gemm: the exact harness of test_gemm_exact_gpu.py with the range knobs set.  The plan is asserted by name through rf_conv_gemm_plan3 before
the launch, outputs / statistics / the split-K workspace sit in NaN-filled guarded allocations, and every output is compared BIT FOR BIT with
exp = ref.float().to(torch.float16) of the exactly known fp32 value.  rf_attention: the tail and tiny families under the harness's own limit_of,
guards as in test_attn_exact_gpu.py; worst err / limit is printed; the vsub family (V in S-in) bit for bit as well.  rf_ffn_geglu and rf_conv3x3_stem: the
launches and guards of test_tokres_exact_gpu.py on scaled inputs; the hidden value of the feed-forward is a subnormal made inside the kernel.  norm.hip:
the launch helpers of test_norm_exact_gpu.py.  The layout and pack kernels: the fp32 edge patterns of side_refs, bit for bit
against Tensor.to(float16).  Wherever a case's data is exact in bf16 too the same case runs in bf16 as a control.  Out of scope: the +-65504 clamp
of attention's reference point (logits beyond 45 000) and NaN input (-fno-honor-nans).  Each case prints its ledger line (DESIGN.md has the table)."""
import pytest
import torch

import attn_exact_refs as AR
import f16_range_cases as C
import gemm_exact_refs as R
import norm_refs as NR
import side_refs as SR
import test_norm_exact_gpu as NG
from reface_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
WORST = {}


# ------------------------------------------------------------------------------------------------ rf_conv_gemm
def _run_gemm(c, i, ref, note=""):
    G = R.geom(c)
    P = R.prepare(c, i, DEV)
    l = P["launch"]
    pl = ops.gemm_plan3(l)
    if c["gn"]:
        R.wire_stats(c, P, pl, DEV, i)
        pl = ops.gemm_plan3(l)
    lost = R.plan_matches(pl, c["expect"])
    assert not lost, f"the cells {c['cells']} lost their case {c['id']}: {lost}"
    assert (pl["splitk"] > 1) == ("reduce" in c["expect"]), (c["id"], pl)
    R.assert_exact(c, i, ref)
    odt = R.out_dtype(c)
    l()
    torch.cuda.synchronize()
    P["out"].check(f"{c['id']}: out")
    if P["ws"] is not None:
        P["ws"].check(f"{c['id']}: split-K workspace")
    got = torch.stack([v for v in P["out"].views], 0).cpu()
    exp = C.store16(ref, odt) if odt != F32 else ref.float()
    same = R._bits(got) == R._bits(exp)
    assert bool(same.all()), (f"{c['id']} ({c['op']}): {int((~same).sum())} of {same.numel()} outputs differ from the exact result, first at "
                              f"{(~same).nonzero()[0].tolist()}: got {got[~same][0].item()!r} expected {exp[~same][0].item()!r} (fp32 value "
                              f"{ref[~same][0].item()!r})")
    extra = ""
    if c["gn"]:
        stored = got[0].to(R.F64)
        for k, (cpg, coff) in enumerate(R.gn_consumers(c)):
            P["gn"][k].check(f"{c['id']}: GroupNorm partial sums of consumer {k}")
            want = R.gn_expected(stored, c, pl["stat_rows"], pl["stat_cols"], cpg, coff)
            have = P["gn"][k].view.cpu()
            assert torch.equal(have, want), f"{c['id']}: consumer {k}: {int((have != want).sum())} of {want.numel()} statistics differ"
            assert not torch.equal(want, R.gn_expected(stored, c, pl["stat_rows"], pl["stat_cols"], cpg, coff, mut_unrounded=ref[0]))
        extra = f" + 2 x {want.numel()} statistics of the stored values"
    words = " ".join(f"{k}={pl[k]}" for k in ("bm", "bn", "waves", "hx", "glds", "conv", "direct", "splitk", "reduce", "tail"))
    print(f"[f16_range] {c['id']} | {'; '.join(c['cells'])} | {c['op']}->{c['out']} M={G['M']} N={c['N']} K={G['K']} batch={c['batch']} | {words} | "
          f"{got.numel()} outputs bit-equal{extra}{note}")


@pytest.mark.parametrize("c", C.GEMM_CASES, ids=[c["id"] for c in C.GEMM_CASES])
def test_conv_gemm_range(c):
    i, ref = C.gemm_prepared(c)
    ctl = C.gemm_control(c)
    if ctl is not None:          # the control first: the same data through the bf16 instantiation
        _run_gemm(ctl, i, ref, " (bf16 control)")
    _run_gemm(c, i, ref)


def test_every_gemm_cell_has_a_case():
    have = {cell for c in C.GEMM_CASES for cell in c["range_cells"]}
    missing = [cell for cell in C.GEMM_CELLS if cell not in have]
    assert not missing, missing


# ------------------------------------------------------------------------------------------------ rf_attention
@pytest.mark.parametrize("c", C.ATTN_CASES, ids=[c["id"] for c in C.ATTN_CASES])
def test_attention_range(c):
    B, heads, d, Nq = c["B"], c["heads"], c["d"], c["Nq"]
    q, k, v, out, alloc, (q64, k64, v64) = AR.buffers(c, DEV)
    pl = ops.attention_plan(q, k, v, out, heads=heads, x3=False)
    lost = AR.plan_matches(pl, c["expect"])
    assert not lost, f"the cell {c['cell']} lost its case {c['id']}: {lost}"
    for x in (q64, k64, v64):          # the operands are held exactly by the case's own type
        assert bool((x.to(AR.TORCH_DT[c["dt"]]).to(AR.F64) == x).all())
    before = {n: AR.bits(t).clone() for n, t in alloc.items()}
    ops.attention(q, k, v, out, heads=heads, scale=ops.LN2, x3=False)()
    torch.cuda.synchronize()
    for n, t in alloc.items():
        now = AR.bits(t).clone()
        if n == "out":
            now[:, :Nq, AR.PAD:AR.PAD + heads * d] = 0
            before[n][:, :Nq, AR.PAD:AR.PAD + heads * d] = 0
        assert torch.equal(now, before[n]), f"{c['id']}: {int((now != before[n]).sum())} guard elements of the {n} allocation changed"
    assert bool(torch.isfinite(out.float()).all())
    got = out.to(AR.F64).view(B, Nq, heads, d).permute(0, 2, 1, 3).reshape(B * heads, Nq, d)
    worst, bad, margin, exact = 0.0, 0, float("inf"), 0
    for g0 in range(0, B * heads, 64):
        s = slice(g0, g0 + 64)
        ref, A, _, p = AR.reference(q64[s], k64[s], v64[s], check=False)
        lim = AR.limit_of(c, ref, A)
        if c["only"] == "tail":          # the family's condition, on every element of the launch: the e >= 15 keys weigh >= 16 fp16 limits
            sub = torch.where(p < C.NORMAL_MIN, p, torch.zeros_like(p))
            margin = min(margin, (((sub @ v64[s]) / p.sum(-1, keepdim=True)).abs() / AR.limit_of(dict(c, dt="fp16"), ref, A)).min().item())
        if c["only"] == "vsub":          # the output is a V row of the target class, on the 16-bit grid: bit equality (the limit is held as well)
            exp = ref.float().to(AR.TORCH_DT[c["dt"]])
            have = got[s].to(AR.TORCH_DT[c["dt"]])
            assert torch.equal(R._bits(have), R._bits(exp)), f"{c['id']}: {int((R._bits(have) != R._bits(exp)).sum())} outputs differ from the class's V row"
            exact += int(exp.numel())
        err = (got[s] - ref).abs()
        bad += int((err > lim).sum())
        worst = max(worst, (err / lim.clamp(min=1e-300)).max().item())
    if c["only"] == "tail":
        assert margin >= 16.0, (c["id"], margin)
    WORST[c["id"]] = worst
    print(f"[f16_range] {c['id']} | {' '.join(f'{w}={pl[w]}' for w in ops.ATTN_PLAN_KEYS)} | {got.numel()} outputs | worst err/limit {worst:.4f}"
          + (f" | e >= 15 keys weigh >= {margin:.1f} limits" if c["only"] == "tail" else "") + (f" | {exact} outputs bit-equal" if exact else ""))
    assert bad == 0, f"{c['id']}: {bad} of {got.numel()} outputs beyond the tolerance, worst err/limit {worst:.3f}"


# ------------------------------------------------------------------------------------------------ layout and pack kernels
def _guarded(shape, dt):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 128,), float("nan"), dtype=dt, device=DEV)
    return buf, buf[64:64 + n].view(shape)


def _fetch(buf, out):
    torch.cuda.synchronize()
    n = out.numel()
    assert torch.isnan(buf[:64]).all() and torch.isnan(buf[64 + n:]).all(), "wrote outside the output"
    return out.cpu()


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16-control"])
def test_nchw_to_nhwc_range(dt):
    x = C.layout_edge_input()
    buf, out = _guarded((SR.LAYOUT_B, SR.LAYOUT_H, SR.LAYOUT_W, SR.LAYOUT_CPAD), dt)
    ops.nchw_to_nhwc(x.to(DEV), out)()
    got = _fetch(buf, out)
    want = torch.zeros(got.shape, dtype=dt)
    want[..., :SR.LAYOUT_C] = x.permute(0, 2, 3, 1).to(dt)
    assert torch.equal(R._bits(got), R._bits(want)), f"{int((R._bits(got) != R._bits(want)).sum())} of {got.numel()} elements differ"
    print(f"[f16_range] rf_nchw_to_nhwc -> {dt}: {got.numel()} outputs bit-equal over {len(SR._F32_EDGE_BITS)} edge patterns")


@pytest.mark.parametrize("dup", [1, 2])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16-control"])
def test_ddim_pack_input_range(dt, dup):
    i = C.ddim_pack_edge_inputs()
    Cpad = 16
    buf, out = _guarded((dup * SR.DDIM_B, SR.DDIM_H, SR.DDIM_W, Cpad), dt)
    ops.ddim_pack_input(i["img"].to(DEV), i["z"].to(DEV), i["mask"].to(DEV), out, dup=dup)()
    got = _fetch(buf, out)
    want = torch.zeros(got.shape, dtype=dt)
    for r in range(dup):
        sl = slice(r * SR.DDIM_B, (r + 1) * SR.DDIM_B)
        want[sl, ..., 0:4] = i["img"].permute(0, 2, 3, 1).to(dt)
        want[sl, ..., 4:8] = i["z"].permute(0, 2, 3, 1).to(dt)
        want[sl, ..., 8:9] = i["mask"].permute(0, 2, 3, 1).to(dt)
    assert torch.equal(R._bits(got), R._bits(want)), f"{int((R._bits(got) != R._bits(want)).sum())} of {got.numel()} elements differ"
    print(f"[f16_range] rf_ddim_pack_input -> {dt} dup={dup}: {got.numel()} outputs bit-equal")


# ------------------------------------------------------------------------------------------------ norm.hip (launch helpers and guards of test_norm_exact_gpu.py)
PID = lambda p: f"{str(p[0])[6:]}-{str(p[1])[6:]}"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16-control"])
def test_groupnorm_stats_subnormal_inputs(dt):
    """S-in: fp64 partial sums of subnormal inputs bit-equal to the fp64 chunk sums, and rf_groupnorm_finalize of them"""
    for B, HW, C_, nch, xp in C.NORM_STATS_SHAPES:
        x = C.norm_stats_input(B, HW, C_, 17 * HW + C_)
        assert NR.stats_exact_bound(dt, HW, C_, nch) < 2 ** 24 and bool((C.is_sub16(x) | (x == 0)).all())
        ref = NR.chunk_partials(x, nch)
        tag = f"stats {dt} C={C_} HW={HW} nchunks={nch}"
        xb, ldx = NG.rows_in(x, dt, xp * NR.vec_of(dt))
        assert torch.equal(xb[:, :C_].cpu().to(NR.F64), x.reshape(-1, C_))
        P = NR.guarded((B * nch + 5, 64), 64, NR.F64, DEV, live_rows=B * nch)
        NG.ok(NG.L().rf_groupnorm_stats(NR.CODE[dt], xb.data_ptr(), B, HW, C_, ldx, nch, P.ptr(), NG.S()))
        P.check(tag)
        P.filled(tag)
        got = P.view[:B * nch].cpu().reshape(B, nch, 32, 2)
        assert torch.equal(NR.bits(got), NR.bits(ref)), f"{tag}: {int((NR.bits(got) != NR.bits(ref)).sum())} partial sums differ"
        Fz = NR.guarded((B, 64), 64, NR.F64, DEV)
        NG.ok(NG.L().rf_groupnorm_finalize(NG.partial_in(got).data_ptr(), B, nch, Fz.ptr(), NG.S()))
        assert torch.equal(NR.bits(Fz.fetch(tag).reshape(B, 32, 2)), NR.bits(ref.sum(1)))
        print(f"[f16_range] rf_groupnorm_stats {dt} B={B} HW={HW} C={C_} nchunks={nch}: {ref.numel()} partial sums of subnormal inputs bit-equal")


@pytest.mark.parametrize("cls", ["S-out", "TOP"])
@pytest.mark.parametrize("pair", C.NORM_PAIRS, ids=PID)
def test_groupnorm_apply_range(pair, cls):
    in_dt, out = pair
    for k, s in enumerate(C.NORM_APPLY_SHAPES):
        i = C.norm_apply_case(cls, s, 31 * k + s["C"])
        tag = f"apply {PID(pair)} {cls} B={s['B']} HW={s['HW']} C={s['C']} nchunks={s['nchunks']}"
        outs = NG.launch_apply(in_dt, out, i["x"], s["xpad"], i["partial"], s["nchunks"], i["gamma"], i["beta"], 0.0, 0, s["opad"])
        NG.compare_exact(tag, outs, out, i["y"])
        print(f"[f16_range] rf_groupnorm_apply {tag}: {i['y'].numel()} outputs bit-equal")


@pytest.mark.parametrize("cls", ["S-out", "TOP"])
@pytest.mark.parametrize("pair", C.NORM_PAIRS, ids=PID)
def test_layernorm_range(pair, cls):
    in_dt, out = pair
    for k, (M, C_) in enumerate(C.NORM_LN_SHAPES):
        i = C.norm_ln_case(cls, M, C_, 7 * C_ + M)
        tag = f"layernorm {PID(pair)} {cls} M={M} C={C_}"
        outs = NG.launch_ln(in_dt, out, i["x"], NR.vec_of(in_dt) * (k % 3), i["gamma"], i["beta"], 0.0, 8 * (k % 3))
        NG.compare_exact(tag, outs, out, i["y"])
        print(f"[f16_range] rf_layernorm {tag}: subnormal rows, {i['y'].numel()} outputs bit-equal")


@pytest.mark.parametrize("out_dt", [F16, BF16], ids=["fp16", "bf16-control"])
def test_groupnorm_fold_linear_range(out_dt):
    B = NR.FOLD_B
    for k, (C_, N, nch) in enumerate(C.NORM_FOLD_SHAPES):
        i = C.norm_fold_case(C_, N, nch, 3 * C_ + N)
        tag = f"fold {out_dt} S-out C={C_} N={N}"
        Wo, Rv = NG.launch_fold(i["W"], None, i["partial"], nch, i["gamma"], i["beta"], 0.0, out_dt, B, 16)
        wp, wps = NR.fold_weights_ref(i["W"], i["mean"], i["var"], i["gamma"], 0.0, out_dt)
        assert torch.equal(wp.float().to(NR.F64), wp)
        r, mag = NR.fold_rowvec_ref(i["W"], wps, i["mean"], i["beta"], None)
        assert torch.equal(r.float().to(NR.F64), r) and mag.max().item() / C.SUB < 2 ** 24
        gw, gr = Wo.fetch(tag).reshape(B, N, C_), Rv.fetch(tag).reshape(B, N)
        exp = wp.float().to(out_dt)
        assert torch.equal(NR.bits(gw), NR.bits(exp)), f"{tag}: {int((NR.bits(gw) != NR.bits(exp)).sum())} of {exp.numel()} folded weights differ"
        assert torch.equal(NR.bits(gr), NR.bits(r.float())), f"{tag}: the row vector differs"
        print(f"[f16_range] rf_groupnorm_fold_linear {tag}: {exp.numel()} weights and {r.numel()} row-vector entries bit-equal")


# ------------------------------------------------------------------------------------------------ rf_conv3x3_stem
@pytest.mark.parametrize("kind,shape", C.STEM_CASES, ids=[f"{k}-{s}" for k, s in C.STEM_CASES])
def test_conv3x3_stem_range(kind, shape):
    c, i, o = C.stem_range_inputs(kind, shape)
    for dt in (BF16, F16):          # the bf16 control first: x and the taps are m 2^e with m <= 3
        l, out = C.stem_prepare(c, i, dt, DEV)
        l()
        torch.cuda.synchronize()
        out.check(f"{c['id']} {kind}: out")
        exp = C.store16(o["out_exact"], dt)
        for k, v in enumerate(out.views):          # (the duplicated half holds the same rows)
            got = v.cpu()
            same = R._bits(got) == R._bits(exp)
            assert bool(same.all()), (f"{c['id']} {kind} {dt} view {k}: {int((~same).sum())} of {same.numel()} outputs differ, first got {got[~same][0].item()!r} "
                                      f"expected {exp[~same][0].item()!r} (fp32 value {o['out_exact'][~same][0].item()!r})")
        print(f"[f16_range] rf_conv3x3_stem {c['id']} | {kind} | {dt} | {len(out.views)} x {exp.numel()} outputs bit-equal")


# ------------------------------------------------------------------------------------------------ rf_ffn_geglu (fp16: the descriptor entry)
@pytest.mark.parametrize("kind,M", C.FFN_RANGE_CASES, ids=[f"{k}-M{m}" for k, m in C.FFN_RANGE_CASES])
def test_ffn_geglu_range(kind, M):
    import tokres_exact_refs as T
    c, i = C.ffn_range_inputs(kind, M)
    for dt in (BF16, F16):          # the bf16 control first (its hidden value is rounded to bf16: the reference is per type)
        o = C.ffn_range_reference(c, i, dt)
        P = T.ffn_prepare(c, i, dt, DEV)
        P["launch"]()
        torch.cuda.synchronize()
        P["out"].check(f"{c['id']} {dt}: out")
        got = P["out"].view.cpu()
        exp = C.store16(o["out_exact"], dt)
        same = R._bits(got) == R._bits(exp)
        assert bool(same.all()), (f"{c['id']} {dt}: {int((~same).sum())} of {same.numel()} outputs differ, first got {got[~same][0].item()!r} expected "
                                  f"{exp[~same][0].item()!r} (fp32 value {o['out_exact'][~same][0].item()!r})")
        sub_h = int(C.is_sub16(o["h"]).sum()) if dt == F16 else 0
        print(f"[f16_range] rf_ffn_geglu {c['id']} | {kind} | {dt} | {exp.numel()} outputs bit-equal" + (f" | {sub_h} subnormal hidden values" if sub_h else ""))


# ------------------------------------------------------------------------------------------------ rf_ffn_block, rf_attn_in, rf_gn_silu_conv3x3_small
def _bit_equal(got, exp, what, exact64):
    got = got.cpu()
    same = R._bits(got) == R._bits(exp)
    assert bool(same.all()), (f"{what}: {int((~same).sum())} of {same.numel()} values differ, first got {got[~same][0].item()!r} expected {exp[~same][0].item()!r} "
                              f"(fp32 value {exact64[~same][0].item()!r})")
    return same.numel()


@pytest.mark.parametrize("form,kind", C.BLOCK_CASES, ids=[f"{f}-{k}" for f, k in C.BLOCK_CASES])
def test_ffn_block_range(form, kind):
    import tokres_exact_refs as T
    c, i = C.block_range_inputs(form, kind)
    for dt in (BF16, F16):          # the bf16 control first; the reference is per type (x1, the hidden value and the feed-forward output are rounded to it)
        o = C.block_range_reference(c, i, dt)
        P = T.ffn_prepare(c, i, dt, DEV)
        P["launch"]()
        torch.cuda.synchronize()
        P["out"].check(f"{c['id']} {dt}: out")
        n = _bit_equal(P["out"].view, C.store16(o["out_exact"], dt), f"{c['id']} {dt}: out", o["out_exact"])
        if P["x1"] is not None:
            P["x1"].check(f"{c['id']} {dt}: x1")
            n += _bit_equal(P["x1"].view, C.store16(o["x1_exact"], dt), f"{c['id']} {dt}: x1", o["x1_exact"])
        sub = int(C.is_sub16(o["x2"]).sum()) if dt == F16 else 0
        print(f"[f16_range] rf_ffn_block {form} | {kind} | M={c['M']} | {dt} | {n} outputs bit-equal" + (f" | {sub} subnormal feed-forward outputs in front of proj_out" if sub else ""))


@pytest.mark.parametrize("kind,shape", C.ATTN_IN_CASES, ids=[f"{k}-{s[0]}x{s[1]}" for k, s in C.ATTN_IN_CASES])
def test_attn_in_range(kind, shape):
    import tokres_exact_refs as T
    c, i = C.attn_in_range_inputs(kind, shape)
    for dn, dt in (("bf16", BF16), ("f16", F16)):
        o = C.attn_in_range_reference(c, i, dt)
        P = T.attn_prepare(c, i, dt, DEV)
        P["launch"]()
        torch.cuda.synchronize()
        P["tok"].check(f"{c['id']} {dt}: tok")
        P["qkv"].check(f"{c['id']} {dt}: qkv")
        n = _bit_equal(P["tok"].view, C.store16(o["tok_exact"], dt), f"{c['id']} {dt}: tok", o["tok_exact"])
        extra = ""
        if c["two_level"]:
            n += _bit_equal(P["qkv"].view, C.store16(o["qkv_exact"], dt), f"{c['id']} {dt}: qkv", o["qkv_exact"])
        else:          # the general cases hold qkv to the harness's limit (test_tokres_exact_gpu.py), against fp64 from the stored tok
            got = P["qkv"].view.cpu().to(R.F64)
            assert bool(torch.isfinite(got).all())
            ratio = ((got - o["qkv_exact"]).abs() / T.limit_of(dict(out="16", op=dn), o["qkv_exact"])).max().item()
            WORST[f"{c['id']}-{dn}"] = ratio
            extra = f" | qkv worst err/limit {ratio:.4f}"
            assert ratio <= 1.0, f"{c['id']} {dt}: qkv err/limit {ratio:.3f}"
        print(f"[f16_range] rf_attn_in {kind} | samples={shape[0]} rows_per_sample={shape[1]} | {dt} | {n} outputs bit-equal{extra}")


@pytest.mark.parametrize("kind,j", C.HEAD_RANGE_CASES, ids=[f"{k}-{j}" for k, j in C.HEAD_RANGE_CASES])
def test_out_head_range(kind, j):
    import tokres_exact_refs as T
    c, i = C.head_range_inputs(kind, j)
    for dt in (BF16, F16):
        o = C.head_range_reference(c, i, dt)
        P = T.head_prepare(c, i, dt, DEV)
        P["launch"]()
        torch.cuda.synchronize()
        P["out"].check(f"{c['id']} {dt}: out")
        P["ws"].check(f"{c['id']} {dt}: per-tap workspace")
        n = _bit_equal(P["out"].view, C.store16(o["out_exact"], dt), f"{c['id']} {dt}: out", o["out_exact"])
        print(f"[f16_range] rf_gn_silu_conv3x3_small {kind} | B={c['B']} {c['H']}x{c['W']} C={c['C']} No={c['No']} nchunks={c['nchunks']} | {dt} | {n} outputs bit-equal")


def test_ledger():
    for cid, w in sorted(WORST.items()):
        print(f"[f16_range] ledger {cid}: worst err/limit {w:.4f}")
