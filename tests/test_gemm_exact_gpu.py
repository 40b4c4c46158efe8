"""rf_conv_gemm against exact integer operands (tests/gemm_exact_refs.py): every product and partial sum is an integer (times a power of two) below
2^24, so the expected output is ONE value whatever the tile, split-K factor or summation order -- and a dropped K element, a wrong tap, a halo
pixel from the neighbouring row or a slice boundary off by one changes it by at least one unit.

Every case names the launch plan it is there for and asserts it through rf_conv_gemm_plan3 BEFORE launching: a dispatch retune that moves a case
onto another kernel fails here by name instead of silently eroding coverage.  Outputs, GroupNorm partial sums, LayerNorm records and the split-K
workspace sit inside larger NaN-filled allocations; everything outside the region the plan names must be bit-identical afterwards.  The epilogues
that are not exact (SiLU, the GELUs, sigmoid, GEGLU's gate) keep an exact pre-activation and are held to 2e-5 + 2e-5 |ref| plus one storage
half-step (2^-8 |ref| for bf16: gemm_exact_refs.limit_of) for 16-bit outputs.  GEGLU's gate is the function the library documents per mode: erf GELU
for fp32 operands, the degree-5 sigmoid form of csrc/common.h for 16-bit operands (against the erf form that one is off by up to 2.6e-5 |value|,
25 x the fp32 rule at |value| ~ 20: printed per case as a figure, bounded by test_ops_gpu.py::test_geglu_negative_gates).  Each case prints its ledger line (DESIGN.md carries the table)."""
import pytest
import torch

import gemm_exact_refs as R
from reface_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                   # activation -> worst err / limit of the tolerance-checked epilogues in this run


def _ledger(c, pl, n, extra=""):
    G = R.geom(c)
    words = " ".join(f"{k}={pl[k]}" for k in ("bm", "bn", "waves", "stages", "hx", "glds", "conv", "direct", "splitk", "reduce", "ln_role", "pm", "pn", "tail"))
    print(f"[gemm_exact] {c['id']} | {'; '.join(c['cells'])} | {c['op']}->{c['out']} M={G['M']} N={c['N']} K={G['K']} batch={c['batch']} | {words} | {n} outputs{extra}")


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_conv_gemm_exact(c):
    _run(c)
    other = R.other_seed(c)          # 16-bit exact cases: the W-sparse AND the A-sparse seed, so that a fault at any k shows in some row
    if other is not None:
        _run(other, " (second seed)")


def _run(c, note=""):
    G = R.geom(c)
    i = R.make_inputs(c)
    P = R.prepare(c, i, DEV)
    l = P["launch"]
    pl = ops.gemm_plan3(l)
    if c["gn"] or c["ln"]:
        R.wire_stats(c, P, pl, DEV, i)
        pl = ops.gemm_plan3(l)
    lost = R.plan_matches(pl, c["expect"])
    assert not lost, f"the cells {c['cells']} lost their case {c['id']}: {lost}"
    assert (pl["splitk"] > 1) == ("reduce" in c["expect"]), (c["id"], pl)
    if R.is_window_case(c) and c["kh"] != c["kw"] and pl["splitk"] > 1:
        # a split non-square window: by the plan's own split some slice starts inside a window row, at a tap KH and KW decode differently
        starts, nk = R.slice_starts(c, pl["splitk"])
        assert nk == -(-G["K"] // R.bk_of(c)) and any(R.tap_of_tile(c, t0) % c["kw"] for t0 in starts[1:]), (c["id"], starts)
        assert R.window_mutant_applies("slice_start_tap", c, pl["splitk"]), c["id"]
    ref = R.reference(c, i, dev=DEV)
    if c["ln"] == "prod":
        ref = R.steer_stripe_means(c, i, ref.cpu(), pl["wave_cols"]).to(DEV)
        P["keep"][-1].copy_(i["res"].to(R.out_dtype(c)).to(DEV))
        assert torch.equal(ref, R.reference(c, i, dev=DEV))
    R.assert_exact(c, i, ref)
    odt = R.out_dtype(c)
    l()
    torch.cuda.synchronize()
    P["out"].check(f"{c['id']}: out")
    if P["ws"] is not None:
        P["ws"].check(f"{c['id']}: split-K workspace")
    got = torch.stack([v for v in P["out"].views], 0)
    exact = R.is_exact(c)
    extra = ""
    if exact:
        exp = ref.to(odt)                      # (the only rounding: the store of an exactly known value; none at all outside the alpha = 0.25 statistics cases)
        same = R._bits(got) == R._bits(exp)
        assert bool(same.all()), (f"{c['id']}: {int((~same).sum())} of {same.numel()} outputs differ from the exact result, first at "
                                  f"{(~same).nonzero()[0].tolist()}: got {got[~same][0].item()} expected {exp[~same][0].item()}")
    else:
        lim = R.limit_of(c, ref)
        err = (got.to(R.F64) - ref).abs()
        assert bool(torch.isfinite(got.float()).all())
        ratio = (err / lim).max().item()
        WORST[c["id"]] = ratio
        extra = f" | worst err/limit {ratio:.4f}"
        print(f"[gemm_exact] {c['id']}: worst err/limit {ratio:.4f} (max err {err.max().item():.3e})")
        if c["act"] == ops.ACT_GEGLU and c["op"] != "f32":
            # the 16-bit modes' gate is the sigmoid form of csrc/common.h, which the reference above restates.  Independently of that restatement the
            # result is held to the erf GELU of the module it replaces, at the distance the library documents for its form: 2.6e-5 per gate, times
            # |value| (the residual, if any, is in both), on top of the same limit
            erf = R.reference(c, i, "gate_erf", dev=DEV)
            val = R.reference(c, i, "gate_unit", dev=DEV) - (i["res"].to(DEV) if i["res"] is not None else 0.0)
            d_erf = (got.to(R.F64) - erf).abs()
            lim_erf = R.GATE_FORM_ERR * val.abs() + R.limit_of(c, erf)
            print(f"[gemm_exact] {c['id']}: against the erf gate: max |d| {d_erf.max().item():.3e}, {(d_erf / R.limit_of(c, erf)).max().item():.2f} x the plain limit, "
                  f"{(d_erf / lim_erf).max().item():.3f} x the limit with the documented 2.6e-5 |value|")
            assert bool((d_erf <= lim_erf).all()), f"{c['id']}: further from erf GELU than the documented 2.6e-5 |value|"
        assert ratio <= 1.0, f"{c['id']}: err/limit {ratio:.3f}"
    stored = got[0].to(R.F64)
    if c["gn"]:
        for k, (cpg, coff) in enumerate(R.gn_consumers(c)):
            P["gn"][k].check(f"{c['id']}: GroupNorm partial sums of consumer {k}")
            want = R.gn_expected(stored, c, pl["stat_rows"], pl["stat_cols"], cpg, coff)
            have = P["gn"][k].view.cpu()
            assert torch.equal(have, want), f"{c['id']}: consumer {k}: {int((have != want).sum())} of {want.numel()} statistics differ"
        extra += f" + 2 x {want.numel()} statistics"
    if c["ln"] == "prod":
        P["ln"].check(f"{c['id']}: LayerNorm records")
        want = R.ln_records(stored, pl["wave_cols"])
        assert want[..., 1].max().item() < R.EXACT_LIMIT
        have = P["ln"].view.view(want.shape).to(R.F64)
        assert torch.equal(have, want), f"{c['id']}: {int((have != want).sum())} of {want.numel()} LayerNorm record words differ"
        extra += f" + {want.numel()} record words"
    _ledger(c, pl, got.numel(), extra + note)


def test_every_cell_of_the_issue_has_a_case():
    """the ledger's completeness: every cell named in CELLS is claimed by at least one case (whose plan the test above asserts)"""
    have = {cell for c in R.CASES for cell in c["cells"]}
    missing = [cell for cell in R.CELLS if cell not in have]
    assert not missing, missing
