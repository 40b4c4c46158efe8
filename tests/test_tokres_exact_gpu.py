"""rf_ffn_geglu / rf_ffn_block, rf_attn_in, rf_conv3x3_stem and rf_gn_silu_conv3x3_small against exact operands (tests/tokres_exact_refs.py): every product
and partial sum is a whole number of units below 2^24, gates are 0 or saturated, LayerNorm rows are two-level, so the expected output is ONE value per
element whatever the order of the fp32 additions -- and a dropped product, a hidden unit from the neighbouring position, a stale LDS stage, a wrong bias
element, a tap from the adjacent image row or a statistics slot with a row missing changes it by at least one unit.  Outputs (out, x1, tok, qkv, the stem's
duplicate half), statistics buffers and the out head's workspace sit inside larger NaN-filled allocations; everything outside the region a launch should
write must be bit-identical afterwards, the rows >= M of ragged cases included.  Every bound of the generators is asserted on the CPU before the launch.

Not exact, and held to a stated limit instead: qkv of rf_attn_in's general-integer cases (gemm_exact_refs.limit_of against fp64 from the stored tok; the
generator keeps |qkv| >= 16 so that the limit, one storage half-step of |qkv|, stays above the few single-step differences that a normalised value next to a
rounding boundary costs: the kernel's fp32 LayerNorm and the fp64 one differ by ~2^-20 relative, the boundaries are 2^-8 / 2^-11 apart, so a few elements
in 10^4 round the other way, each moving an output by at most 2^-7 |xhat| |w| <= 0.02), and the gate sweep through the fused feed-forward (the rule and
constant of test_ops_gpu.py::test_geglu_negative_gates).  Each case prints its ledger line; the last test prints the totals (DESIGN.md carries them)."""
import pytest
import torch

import tokres_exact_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOTAL = dict(cases=0, launches=0, outputs=0, stats=0, toleranced=0)
DTN = list(R.DTS)


def _same(got, exp, what):
    same = R._bits(got.cpu()) == R._bits(exp)
    assert bool(same.all()), (f"{what}: {int((~same).sum())} of {same.numel()} values differ from the exact result, first at {(~same).nonzero()[0].tolist()}: "
                              f"got {got.cpu()[~same][0].item()} expected {exp[~same][0].item()}")
    return same.numel()


def _ledger(c, dn, form, shape, n_out, n_stat, extra=""):
    TOTAL["cases"] += 1
    TOTAL["outputs"] += n_out
    TOTAL["stats"] += n_stat
    print(f"[tokres_exact] {c['id']}/{dn} | {form} | {shape} | seeds {'+'.join(c['seeds'])} | {n_out} outputs bit for bit | {n_stat} statistics words{extra}")


def _prepared(c, seed, dt):
    k = c["kernel"]
    i = R.INPUTS[k](c, seed)
    o = R.REFERENCE[k](c, i, dt)
    R.ASSERT_EXACT[k](c, i, dt, o)          # the generator's bounds, on this data, before anything is launched
    P = R.PREPARE[k](c, i, dt, DEV)
    P["launch"]()
    torch.cuda.synchronize()
    TOTAL["launches"] += 1
    return i, o, P


@pytest.mark.parametrize("dn", DTN)
@pytest.mark.parametrize("c", R.FFN_CASES, ids=[c["id"] for c in R.FFN_CASES])
def test_ffn_exact(c, dn):
    dt = R.DTS[dn]
    n_out = n_stat = 0
    for seed in c["seeds"]:
        i, o, P = _prepared(c, seed, dt)
        what = f"{c['id']}/{seed}/{dn}"
        if c["form"] == "geglu":          # bf16 goes through the positional entry point, fp16 through the descriptor one: both must be hit
            assert P["launch"].fn.__name__ == ("rf_ffn_geglu" if dn == "bf16" else "rf_ffn_block"), P["launch"].fn.__name__
        P["out"].check(f"{what}: out")
        n_out += _same(P["out"].view, o["out"].to(dt), f"{what}: out")
        if P["x1"] is not None:
            P["x1"].check(f"{what}: x1")
            n_out += _same(P["x1"].view, o["x1"].to(dt), f"{what}: x1")
        for k, st in enumerate(P["stats"]):
            have = st.fetch(f"{what}: GroupNorm partial sums of consumer {k}")
            assert torch.equal(have, o["stats"][k]), f"{what}: consumer {k}: {int((have != o['stats'][k]).sum())} of {have.numel()} statistics words differ"
            n_stat += have.numel()
    form = {"geglu": "rf_ffn_geglu", "tail": "rf_ffn_block tail", "front": "rf_ffn_block FRONT"}[c["form"]] + (" ln_eps 1e-5" if c["ln"] else " ln_eps 0")
    _ledger(c, dn, form, f"M={c['M']} samples={c['S']} res2_rows={c['res2_rows']} front_rows={c['front_rows']} consumers={c['stats']}", n_out, n_stat)


@pytest.mark.parametrize("dn", DTN)
@pytest.mark.parametrize("c", R.ATTN_CASES, ids=[c["id"] for c in R.ATTN_CASES])
def test_attn_in_exact(c, dn):
    dt = R.DTS[dn]
    n_out, worst, n_tol = 0, 0.0, 0
    for seed in c["seeds"]:
        i, o, P = _prepared(c, seed, dt)
        what = f"{c['id']}/{seed}/{dn}"
        P["tok"].check(f"{what}: tok")
        P["qkv"].check(f"{what}: qkv")
        n_out += _same(P["tok"].view, o["tok"].to(dt), f"{what}: tok")
        if c["two_level"]:
            n_out += _same(P["qkv"].view, o["qkv"].to(dt), f"{what}: qkv")
        else:
            got = P["qkv"].view.cpu().to(R.F64)
            assert bool(torch.isfinite(got).all()), what
            lim = R.limit_of(dict(out="16", op=dn), o["qkv_exact"])
            ratio = ((got - o["qkv_exact"]).abs() / lim).max().item()
            worst, n_tol = max(worst, ratio), n_tol + got.numel()
            print(f"[tokres_exact] {what}: qkv worst err/limit {ratio:.4f}")
            assert ratio <= 1.0, f"{what}: qkv err/limit {ratio:.3f}"
    TOTAL["toleranced"] += n_tol
    _ledger(c, dn, "rf_attn_in", f"samples={c['S']} rows_per_sample={c['rps']}", n_out, 0, f" | qkv to limit_of: {n_tol} values, worst err/limit {worst:.4f}" if n_tol else "")


@pytest.mark.parametrize("dn", DTN)
@pytest.mark.parametrize("c", R.STEM_CASES, ids=[c["id"] for c in R.STEM_CASES])
def test_stem_exact(c, dn):
    dt = R.DTS[dn]
    n_out = n_stat = 0
    for seed in c["seeds"]:
        i, o, P = _prepared(c, seed, dt)
        what = f"{c['id']}/{seed}/{dn}"
        P["out"].check(f"{what}: out")
        n_out += _same(P["out"].views[0], o["out"].to(dt), f"{what}: out")
        if c["dup"]:
            assert torch.equal(R._bits(P["out"].views[1]), R._bits(P["out"].views[0])), f"{what}: the duplicate half differs from the computed one"
            n_out += P["out"].views[1].numel()
        for k, st in enumerate(P["stats"]):
            have = st.fetch(f"{what}: GroupNorm partial sums of consumer {k}")
            assert torch.equal(have, o["stats"][k]), f"{what}: consumer {k}: {int((have != o['stats'][k]).sum())} of {have.numel()} statistics words differ"
            n_stat += have.numel()
    _ledger(c, dn, "rf_conv3x3_stem", f"B={c['B']} {c['H']}x{c['W']} C={c['C']} dup={int(c['dup'])} consumers=3", n_out, n_stat)


@pytest.mark.parametrize("dn", DTN)
@pytest.mark.parametrize("c", R.HEAD_CASES, ids=[c["id"] for c in R.HEAD_CASES])
def test_out_head_exact(c, dn):
    dt = R.DTS[dn]
    odt = torch.float32 if c["out"] == "f32" else dt
    n_out = 0
    for seed in c["seeds"]:
        i, o, P = _prepared(c, seed, dt)
        what = f"{c['id']}/{seed}/{dn}"
        P["out"].check(f"{what}: out")
        P["ws"].check(f"{what}: per-tap workspace")
        n_out += _same(P["out"].view, o["out"].to(odt), f"{what}: out")
    _ledger(c, dn, "rf_gn_silu_conv3x3_small", f"B={c['B']} {c['H']}x{c['W']} C={c['C']} No={c['No']} {c['out']} silu={c['silu']} nchunks={c['nchunks']} (exact, no fallback)", n_out, 0)


@pytest.mark.parametrize("dn", DTN)
def test_gate_sweep_through_the_fused_kernel(dn):
    """ffn.hip's own call of gelu_sigmoid5, on its own accumulator layout: 1280 gates over [-9, 9] (+-7 and their fp32 neighbours among them), each attributed to
    one output column of one row type; |out - value gelu_erf(gate)| <= 2.6e-5 |value| + STEP |ref| + 1e-6, the rule of test_geglu_negative_gates"""
    dt = R.DTS[dn]
    i, value, gate = R.gate_sweep_inputs()
    c = R.ffn_case("gate-sweep", [], "geglu", 128, False, ("sweep",))
    P = R.ffn_prepare(c, i, dt, DEV)
    P["launch"]()
    torch.cuda.synchronize()
    P["out"].check("gate sweep: out")
    ref = value * R.gelu_erf(gate)
    err = (P["out"].view.cpu().to(R.F64) - ref).abs()
    lim = R.GATE_FORM_ERR * value.abs() + R.STEP[dt] * ref.abs() + 1e-6
    ratio = (err / lim).max().item()
    print(f"[tokres_exact] gate sweep/{dn}: 1280 gates x 32 rows, worst err/limit {ratio:.4f} (max err {err.max().item():.3e})")
    assert ratio <= 1.0, f"gate sweep {dn}: err/limit {ratio:.3f}"


def test_every_cell_of_the_issue_has_a_case():
    """the ledger's completeness: every mechanism named in CELLS is claimed by at least one case; then the totals of this run"""
    have = {cell for c in R.CASES for cell in c["cells"]}
    missing = [cell for cell in R.CELLS if cell not in have]
    assert not missing, missing
    print(f"[tokres_exact] totals of this run: {TOTAL['cases']} cases (case x type), {TOTAL['launches']} launches, {TOTAL['outputs']} outputs and {TOTAL['stats']} statistics "
          f"words compared bit for bit, {TOTAL['toleranced']} qkv values held to limit_of; no out-head case fell back to a tolerance")
