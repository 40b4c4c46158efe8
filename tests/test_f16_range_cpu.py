"""CPU checks of tests/f16_range_cases.py, the cases of tests/test_f16_range_gpu.py.  No kernel runs.
  a. the class tables restate the format: Tensor.to(float16) of every S-out / TOP value is what the table says;
  b. every case holds what it claims, before any launch: counts of subnormal operands, of results in every S-out / TOP class (both signs), at least
     one tie of each kind, results on both sides of every tie, all partial sums below 2^24 units, the exactly known result exact in fp32;
  c. the references: the scaled gemm reference against torch's fp64 conv2d / linear, the tail and tiny attention families against torch's fp64
     softmax, the store mutants' helper against side_refs.cast_ref;
  d. the mutants -- subnormal operands flushed (A, W, the 16-bit residual, attention's P and V, the token kernels' x / W1 / W2 / Wpo / Wo / W' / Wqkv / taps, separately), the 16-bit values
     re-rounded INSIDE a kernel (hidden value, feed-forward output, GroupNorm result) flushed or truncated, subnormal results flushed at the store, a
     truncating store, saturation instead of +-inf, statistics of the unrounded value -- each change at least one output bit of EVERY case that
     claims the matching class (attention: by more than limit_of): the GPU file would fail on a kernel that did any of it;
  e. every (path, class) cell is claimed, and every case names the plan the library reports (a host-only query);
  f. at their defaults the range knobs leave the exact harnesses' cases as they were (their own suites assert the rest)."""
import pytest
import torch
import torch.nn.functional as F

import attn_exact_refs as AR
import f16_range_cases as C
import gemm_exact_refs as R
import norm_refs as NR
import side_refs as SR
from reface_amd import ops

F64, F16, BF16 = torch.float64, torch.float16, torch.bfloat16
SMALL = [R.small_of(c) for c in C.GEMM_CASES]
IDS = [c["id"] for c in C.GEMM_CASES]


@pytest.fixture(scope="module")
def prepared():
    """inputs and steered fp64 reference of every gemm range case at its CPU size, computed once"""
    return {c["id"]: C.gemm_prepared(c) for c in SMALL}


# ------------------------------------------------------------------------------------------------ a. the class tables
def test_class_tables_restate_the_format():
    for name, v in C.S_OUT.items():
        for s in (1.0, -1.0):
            st = torch.tensor([s * v], dtype=torch.float32).to(F16)
            assert st.double().item() == s * C.S_OUT_STORED[name] and float(SR.cast_ref(torch.tensor([s * v], dtype=F64), F16)) == s * C.S_OUT_STORED[name], name
            if C.S_OUT_STORED[name] == 0.0:          # the sign of a zero result survives
                assert torch.signbit(st).item() == (s < 0)
    for name, v in C.TOP.items():
        for s in (1.0, -1.0):
            assert torch.tensor([s * v], dtype=torch.float32).to(F16).double().item() == s * C.TOP_STORED[name], name
    assert float(torch.tensor([2.0 ** -24]).to(F16).view(torch.int16)) == 1 and C.is_sub16(torch.tensor([1023 * C.SUB, C.SUB], dtype=F64)).all()
    assert not C.is_sub16(torch.tensor([2.0 ** -14, 0.0, 2.0 ** -25], dtype=F64)).any()


def test_store_mutants_are_what_they_say():
    x = C.edge_values_f32()
    x = x[torch.isfinite(x)].double()
    assert torch.equal(C.store16(x).double(), SR.cast_ref(x, F16))          # the true store is side_refs' definition of the format
    t = C.store16_trunc(x).double()
    fin = torch.isfinite(t)
    assert bool((t[fin].abs() <= x[fin].abs()).all()) and bool(((x[fin] - t[fin]).abs() < torch.maximum(x[fin].abs() * 2.0 ** -10, torch.tensor(C.SUB, dtype=F64))).all())
    assert C.store16_trunc(torch.tensor([3 * 2.0 ** -25, 65519.0, 65520.0, -65535.0, 65536.0], dtype=F64)).double().tolist() == [2.0 ** -24, 65504.0, 65504.0, -65504.0, float("inf")]
    assert C.store16_saturate(torch.tensor([65520.0, -1e9], dtype=F64)).double().tolist() == [65504.0, -65504.0]
    assert C.store16_flush(torch.tensor([1023 * C.SUB, -C.SUB, 2.0 ** -14], dtype=F64)).double().tolist() == [0.0, -0.0, 2.0 ** -14]


# ------------------------------------------------------------------------------------------------ b. the gemm cases hold what they claim
@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_gemm_case_holds_what_it_claims(c, prepared):
    i, ref = prepared[c["id"]]
    R.assert_exact(c, i, ref)                                      # partial sums below 2^24 units, the result exact in fp32, epilogue terms on the unit
    assert R.magnitude_bound(c, i)[0] / R.unit_of(c, i) < R.EXACT_LIMIT
    A_, W_, E_ = C.gemm_operands(c, i)
    cl = c["classes"]
    n_sub = lambda ts: sum(int(C.is_sub16(t).sum()) for t in ts)
    n_all = lambda ts: sum(int((t != 0).sum()) for t in ts)
    if "S-in A" in cl:          # every non-zero activation is an fp16 subnormal, thousands of them
        assert n_sub(A_) == n_all(A_) >= 1000, (c["id"], n_sub(A_), n_all(A_))
    if "S-in W" in cl:
        assert n_sub(W_) == n_all(W_) >= 1000, (c["id"], n_sub(W_), n_all(W_))
    if "S-in E" in cl:
        assert c["out"] == "16" and n_sub([i["res"]]) == n_all([i["res"]]) >= 1000 and n_sub([i["bias"]]) >= 32 and n_sub([i["rowvec"]]) >= 32
    if c["control"]:            # the bf16 control's condition: all 16-bit operands are exact in bf16 as well
        for t in A_ + W_ + ([i["res"]] if c["out"] == "16" and i["res"] is not None else []):
            assert torch.equal(t.to(BF16).to(F64), t), c["id"]
    else:
        assert c["a_hi"] > 255 or c["gn"], c["id"]
    if c["a_hi"] > 255:         # ... and the full 10-bit subnormal mantissa where it does not run
        assert max(float(t.abs().max()) for t in A_) / C.SUB > 255
    flat = ref.reshape(-1)
    if c["steer"]:
        table, stored = (C.S_OUT, C.S_OUT_STORED) if c["steer"] == "S-out" else (C.TOP, C.TOP_STORED)
        exp = C.store16(ref).double().reshape(-1)
        for name, v in table.items():
            for s in (1.0, -1.0):
                hit = flat == s * v
                assert int(hit.sum()) >= max(1, c["N"] // 2 // len(table) // 2), (c["id"], name, s, int(hit.sum()))
                assert bool((exp[hit] == s * stored[name]).all()) and (v != 0 or bool(hit.any()))
        if c["steer"] == "S-out":
            band = flat.abs() < 2.0 ** -13
            assert band.double().mean().item() > 0.9, c["id"]                           # the whole output lives in the band
            half = torch.remainder(flat / C.SUB, 1.0)
            ties, below, above = half == 0.5, (half > 0) & (half < 0.5), half > 0.5
            odd_tie = ties & (torch.remainder(torch.floor(flat.abs() / C.SUB), 2.0) == 1)
            assert int((ties & ~odd_tie).sum()) >= 1 and int(odd_tie.sum()) >= 1 and int(below.sum()) >= 100 and int(above.sum()) >= 100, c["id"]
            assert int(((exp == 0) & torch.signbit(exp)).sum()) >= 1 and int(((exp == 0) & ~torch.signbit(exp)).sum()) >= 1          # -0 and +0
        else:
            assert int(torch.isposinf(exp).sum()) >= 1 and int(torch.isneginf(exp).sum()) >= 1
            assert int(((flat.abs() > C.F16_MAX) & (flat.abs() < 65520)).sum()) >= 1 and int((exp.abs() == C.F16_MAX).sum()) >= 2
    if c["gn"]:
        st = C.store16(ref[0]).double()
        assert bool((st.abs() < C.NORMAL_MIN).all()) and int(C.is_sub16(st).sum()) > 0.9 * st.numel() and not torch.equal(st, ref[0])


# ------------------------------------------------------------------------------------------------ c. references
@pytest.mark.parametrize("kw", [dict(W=37, C0=72, N=40), dict(B=2, H=7, W=6, C0=64, N=24, ks=3, pad=R.P3, rowvec=True, res=True)], ids=["linear", "conv3x3"])
def test_scaled_gemm_reference_equals_torch_fp64(kw):
    """the harness's reference with the range knobs set, on its own scaled integers, against torch's fp64 conv2d: equal, not close"""
    c = R.case("scaled", (), {}, op="f16", a_exp=-24, w_exp=-11, e_exp=-24, a_hi=255, range16=True, **kw)
    i = R.make_inputs(c)
    assert int(C.is_sub16(i["x0"]).sum()) == i["x0"].numel() and float(i["w"].abs().max()) == 3 * 2.0 ** -11
    ks = c["ks"]
    w4 = i["w"][0].reshape(c["N"], ks, ks, c["C0"]).permute(0, 3, 1, 2)
    y = F.conv2d(F.pad(i["x0"].permute(0, 3, 1, 2), c["pad"][1:2] * 2 + c["pad"][0:1] * 2), w4).permute(0, 2, 3, 1).reshape(-1, c["N"]) + i["bias"][None]
    if c["rowvec"]:
        y = y + i["rowvec"].repeat_interleave(R.geom(c)["rps"], 0)
    if c["res"]:
        y = y + i["res"][0]
    assert torch.equal(R.reference(c, i)[0], y)
    assert R.unit_of(c, i) == 2.0 ** -35


def _attn_small(c, nq=37):
    """a range attention case cut to CPU size: the same keys, a few heads, fewer queries"""
    s = dict(c, Nq=min(c["Nq"], nq))
    return s, AR.operands(s, range(min(C.ATTN_CHECK_HEADS, c["B"] * c["heads"])))


@pytest.mark.parametrize("c", C.ATTN_CASES, ids=[c["id"] for c in C.ATTN_CASES])
def test_attention_families_hold_what_they_claim(c):
    s, (q, k, v) = _attn_small(c)
    dt = AR.TORCH_DT[c["dt"]]
    for x in (q, k, v):
        assert bool((x.to(dt).to(F64) == x).all())
    sc = q @ k.transpose(-1, -2)
    ref, A, l, p = AR.reference(q, k, v, check=False)
    want = torch.softmax(sc * AR.LN2, -1) @ v                      # plain torch fp64 softmax of the same scores (scale = ln 2)
    assert (ref - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    if c["only"] == "tail":
        assert bool((sc == sc.round()).all()) and sc.abs().max().item() <= 256
        e = -torch.log2(p)
        assert bool(((p == 1).sum(-1) == 1).all())                                      # one key at the row maximum
        rest = e[p < 1]
        assert rest.min().item() >= 9 and rest.max().item() <= 24 and bool((rest == rest.round()).all())
        assert bool((p.to(F16).to(F64) == p).all())                                     # every weight is exact in fp16 ...
        assert int(C.is_sub16(p).sum()) > 0.5 * p.numel()                               # ... and most are subnormal there
        T = c["expect"]["keys"]
        jm = p.argmax(-1)
        assert bool(((jm > 0) & (jm < c["Nk"] - 1)).all())                              # tail keys before and after the maximum ...
        for t0 in range(0, c["Nk"], T):                                                  # ... and in every staged key tile
            assert bool(C.is_sub16(p[..., t0:t0 + T]).any(-1).all()), (c["id"], t0)
        if c["Nk"] > 2 * T:          # both ends of e are met
            assert rest.min().item() == 9 and rest.max().item() == 24
        # the family's condition, in fp16 (the format it is about; bf16's store step is 8 x coarser and its P is never subnormal: a control)
        part, lim, _ = C.attn_tail_split(dict(s, dt="fp16"), q, k, v)
        assert (part / lim).min().item() >= 16.0, (c["id"], (part / lim).min().item())
    elif c["only"] == "vsub":
        AR.reference(q, k, v, check=True)                                                # integer scores, every weight live (1) or dead (<= 2^-30)
        n_live = (p == 1).sum(-1)
        assert bool((n_live >= 3).all()) and bool(((p == 1) | (p <= 2.0 ** -32)).all())
        sub = C.is_sub16(v)
        assert int(sub.sum()) >= 0.7 * v.numel() and int((~sub & (v != 0)).sum()) >= 0.2 * v.numel() and bool((v != 0).all())          # subnormal V, normal in every 4th column
        assert (v[sub].abs() / C.SUB).max().item() >= 250                                # the 8 bits the control allows are used
        # the output IS the V row of the query's class: every live key of a row carries the same row of V, and the store rounds back onto it
        first = p.argmax(-1)
        vrow = torch.gather(v, 1, first[..., None].expand(-1, -1, v.shape[-1]))
        live_rows = (p == 1)[..., None]
        assert bool(((v[:, None] == vrow[:, :, None]) | ~live_rows).all())
        for dt in (F16, BF16):
            assert torch.equal(R._bits(ref.float().to(dt)), R._bits(vrow.float().to(dt))) and torch.equal(vrow.float().to(dt).double(), vrow)
        # the mutant: V's subnormals flushed on the way into the P V product -- every subnormal output becomes 0, beyond bit equality AND the limit
        wrong = AR.reference(q, k, C.flush_sub(v), check=False)[0]
        assert C.bits_differ(wrong.float().to(F16), ref.float().to(F16))
        moved = (wrong - ref).abs() > AR.limit_of(dict(s, dt="fp16"), ref, A)
        assert bool(moved[C.is_sub16(vrow)].all())
    else:
        mx = sc.amax(-1)
        assert bool((sc / C.SUB == (sc / C.SUB).round()).all()) and int(C.is_sub16(q).sum()) >= q.shape[0] * q.shape[1]
        pos, neg = (mx > 0) & (mx < C.NORMAL_MIN), (mx < 0) & (mx > -C.NORMAL_MIN)
        assert bool((pos | neg).all()) and int(pos.sum()) >= 10 and int(neg.sum()) >= 10          # both untested branches of ceil16<f16_t>
        # the weights the kernel packs to 16 bits are 1 there; against the fp64 weights that is within a thousandth of the limit's A term alone
        assert (1 - p).max().item() <= 2.0 ** -21 and 2.0 ** -21 * 2 <= 2.0 ** -18 / 2


# ------------------------------------------------------------------------------------------------ d. mutants
MUTANT_CLASS = {"A subnormals flushed": "S-in A", "W subnormals flushed": "S-in W", "16-bit residual subnormals flushed": "S-in E", "results flushed at the store": "S-out",
                "store by truncation": ("S-out", "TOP"), "saturation to +-65504": "TOP", "statistics of the unrounded value": "S-out stats"}


@pytest.mark.parametrize("m", list(MUTANT_CLASS))
def test_gemm_mutant_is_told_apart_by_every_case_of_its_class(m, prepared):
    want = MUTANT_CLASS[m]
    want = (want,) if isinstance(want, str) else want
    cases = [c for c in SMALL if set(want) & set(c["classes"])]
    assert cases, m
    missed = []
    for c in cases:
        i, ref = prepared[c["id"]]
        odt = R.out_dtype(c)
        true = C.store16(ref) if odt == F16 else ref.float()
        if m.endswith("subnormals flushed"):
            wrong = C.gemm_mutant_ref(c, i, {"A": "A", "W": "W", "1": "E"}[m[0]])
            wrong = C.store16(wrong) if odt == F16 else wrong.float()
        elif m == "statistics of the unrounded value":
            bm, bn = c["expect"]["bm"], c["expect"]["bn"]
            st = true[0].double()
            same = all(torch.equal(R.gn_expected(st, c, bm, bn, cpg, coff), R.gn_expected(st, c, bm, bn, cpg, coff, mut_unrounded=ref[0])) for cpg, coff in R.gn_consumers(c))
            if same:
                missed.append(c["id"])
            continue
        else:
            wrong = {"results flushed at the store": C.store16_flush, "store by truncation": C.store16_trunc, "saturation to +-65504": C.store16_saturate}[m](ref)
        if not C.bits_differ(wrong, true):
            missed.append(c["id"])
    assert not missed, f"mutant {m} is not told apart by: {missed}"
    print(f"[f16_range] mutant {m}: told apart by all {len(cases)} cases of {want}")


@pytest.mark.parametrize("c", [c for c in C.ATTN_CASES if c["only"] == "tail" and c["dt"] == "fp16"], ids=lambda c: c["id"])
def test_attention_p_flush_mutant_exceeds_the_limit(c):
    """P's subnormals flushed to zero in the P V product -- with the denominator from the fp32 weights (ones = 0) or from the flushed ones (ones = 1):
    either way EVERY output element moves by more than its limit"""
    s, (q, k, v) = _attn_small(c)
    ref, A, l, p = AR.reference(q, k, v, check=False)
    lim = AR.limit_of(s, ref, A)
    pf = C.flush_sub(p)
    for den in (l, pf.sum(-1, keepdim=True)):
        assert bool((((pf @ v) / den - ref).abs() > lim).all()), c["id"]
    # the harness's own online-softmax walk with P through fp16 agrees with the reference (gradual underflow kept) ...
    T = c["expect"]["keys"]
    on = AR.online(q[0], k[0], v[0], T, dma=c["expect"]["family"] == "dma", pdt=F16)
    assert bool(((on - ref[0]).abs() <= lim[0]).all())


# ------------------------------------------------------------------------------------------------ norm.hip: claims, references, mutants
def _class_counts(y, cls, what):
    """every class value, both signs, is met; S-out: ties of both kinds and off-grid values on both sides; TOP: both infinities and a finite value above 65504"""
    flat = y.reshape(-1)
    exp = C.store16(y).double().reshape(-1)
    table, stored = (C.S_OUT, C.S_OUT_STORED) if cls == "S-out" else (C.TOP, C.TOP_STORED)
    for name, v in table.items():
        for s in (1.0, -1.0):
            hit = flat == s * v
            assert int(hit.sum()) >= 1 and bool((exp[hit] == s * stored[name]).all()), (what, name, s)
    if cls == "S-out":
        half = torch.remainder(flat / C.SUB, 1.0)
        odd = torch.remainder(torch.floor(flat.abs() / C.SUB), 2.0) == 1
        assert int(((half == 0.5) & odd).sum()) >= 1 and int(((half == 0.5) & ~odd).sum()) >= 1, what
    else:
        assert int(torch.isposinf(exp).sum()) >= 1 and int(torch.isneginf(exp).sum()) >= 1 and int(((flat.abs() > C.F16_MAX) & (flat.abs() < 65520)).sum()) >= 1, what
    for name, mut in (("truncation", C.store16_trunc),) + ((("flush", C.store16_flush),) if cls == "S-out" else (("saturation", C.store16_saturate),)):
        assert C.bits_differ(mut(y), C.store16(y)), (what, name)          # the store mutants of this class change an output bit


def test_norm_stats_cases_and_mutant():
    for B, HW, C_, nch, _ in C.NORM_STATS_SHAPES:
        x = C.norm_stats_input(B, HW, C_, 17 * HW + C_)
        assert bool((C.is_sub16(x) | (x == 0)).all()) and C.is_sub16(x).double().mean().item() > 0.9 and torch.equal(x.to(F16).to(F64), x) and torch.equal(x.to(BF16).to(F64), x)          # all subnormal, exact in both types
        for dt in (F16, BF16):
            assert NR.stats_exact_bound(dt, HW, C_, nch) < 2 ** 24
        ref = NR.chunk_partials(x, nch)
        assert torch.equal(ref[..., 0] / C.SUB, (ref[..., 0] / C.SUB).round()) and torch.equal(ref.float().to(F64), ref)
        # plain torch fp64: the chunk sums add up to the group sums of the whole tensor
        xg = x.reshape(B, HW, 32, C_ // 32)
        assert torch.equal(ref.sum(1)[..., 0], xg.sum((1, 3))) and torch.equal(ref.sum(1)[..., 1], (xg * xg).sum((1, 3)))
        assert not torch.equal(NR.chunk_partials(C.flush_sub(x), nch), ref) and bool((ref[..., 1] > 0).any())          # inputs flushed on load


@pytest.mark.parametrize("cls", ["S-out", "TOP"])
def test_norm_apply_and_layernorm_cases_hold_their_classes(cls):
    for k, s in enumerate(C.NORM_APPLY_SHAPES):
        i = C.norm_apply_case(cls, s, 31 * k + s["C"])
        B, HW, C_ = s["B"], s["HW"], s["C"]
        mean, var = NR.moments_of_partials(i["partial"], HW, C_)
        assert torch.equal(mean, i["mean"]) and torch.equal(var, i["var"])
        ref = NR.gn_apply_ref(i["x"], mean, var, i["gamma"], i["beta"], 0.0, False).reshape(B * HW, C_)
        assert torch.equal(ref, i["y"]) and torch.equal(i["y"].float().to(F64), i["y"])
        assert torch.equal(i["x"].to(BF16).to(F64), i["x"])
        _class_counts(i["y"], cls, f"apply {s}")
    for M, C_ in C.NORM_LN_SHAPES:
        i = C.norm_ln_case(cls, M, C_, 7 * C_ + M)
        assert bool(C.is_sub16(i["x"]).all()) and torch.equal(i["x"].to(BF16).to(F64), i["x"])
        ref = NR.layernorm_ref(i["x"], i["gamma"], i["beta"], 0.0)
        assert torch.equal(ref, i["y"]) and torch.equal(i["y"].float().to(F64), i["y"])
        want = torch.nn.functional.layer_norm(i["x"] * 2.0 ** 24, (C_,), i["gamma"].double(), i["beta"].double(), 0.0)          # torch's fp64 operator (scale-free)
        assert (want - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
        _class_counts(i["y"], cls, f"layernorm {M}x{C_}")
        assert not bool(torch.isfinite(NR.layernorm_ref(C.flush_sub(i["x"]), i["gamma"], i["beta"], 0.0)).any())          # inputs flushed on load: 0 / 0


def test_norm_fold_cases_hold_their_classes():
    for C_, N, nch in C.NORM_FOLD_SHAPES:
        i = C.norm_fold_case(C_, N, nch, 3 * C_ + N)
        wp, wps = NR.fold_weights_ref(i["W"], i["mean"], i["var"], i["gamma"], 0.0, F16)
        assert torch.equal(wp.float().to(F64), wp) and torch.equal(wps, C.store16(wp).double()) and not torch.equal(wp, wps)
        for name in ("2^-24", "2^-25 tie->0", "3*2^-25 tie->2^-23", "2^-25(1+2^-10)", "1023*2^-24", "2^-14"):
            for s in (1.0, -1.0):
                hit = wp == s * C.S_OUT[name]
                assert int(hit.sum()) >= 1 and bool((wps[hit] == s * C.S_OUT_STORED[name]).all()), (C_, N, name, s)
        r, mag = NR.fold_rowvec_ref(i["W"], wps, i["mean"], i["beta"], None)
        assert torch.equal(r.float().to(F64), r) and mag.max().item() / C.SUB < 2 ** 24
        # the row vector of the UNROUNDED W', of a flushed and of a truncated store all differ from it
        for other in (wp, C.store16_flush(wp).double(), C.store16_trunc(wp).double()):
            assert not torch.equal(other, wps)
            assert not torch.equal(NR.fold_rowvec_ref(i["W"], other, i["mean"], i["beta"], None)[0], r)


# ------------------------------------------------------------------------------------------------ rf_conv3x3_stem
@pytest.mark.parametrize("kind,shape", C.STEM_CASES, ids=[f"{k}-{s}" for k, s in C.STEM_CASES])
def test_stem_cases_hold_their_classes_and_mutants(kind, shape):
    import tokres_exact_refs as T
    cls, xe, we = C.STEM_KINDS[kind]
    c, i, o = C.stem_range_inputs(kind, shape)          # (asserts: every partial sum below 2^24 units, the result exact in fp32)
    y = o["out_exact"]
    x9, taps = i["x"][..., :9], i["w"].reshape(-1, 9, 16)
    for t in (i["x"], i["w"]):
        assert torch.equal(t.to(BF16).to(F64), t) and torch.equal(t.to(F16).to(F64), t)          # the control's condition
    assert bool((i["x"][..., 9:] == 0).all()) and bool((taps[..., 9:] != 0).all())                      # the padding contract stays visible
    # the reference on the scaled operands against torch's fp64 conv2d
    w4 = taps[..., :9].permute(0, 2, 1).reshape(c["C"], 9, 3, 3)
    want = F.conv2d(x9.permute(0, 3, 1, 2), w4, padding=1).permute(0, 2, 3, 1).reshape(-1, c["C"]) + i["bias"]
    assert torch.equal(want, y)
    true = C.store16(y)
    flushed = lambda key: C.store16(T.stem_reference(c, dict(i, **{key: C.flush_sub(i[key])}), F16)["out_exact"])
    if xe == -24:
        assert int(C.is_sub16(x9).sum()) == int((x9 != 0).sum()) >= 1000 and C.bits_differ(flushed("x"), true)
    if we == -24:
        assert int(C.is_sub16(taps).sum()) == int((taps != 0).sum()) >= 1000 and C.bits_differ(flushed("w"), true)
        assert bool(C.is_sub16(y[y != 0]).any()) and C.bits_differ(C.store16_flush(y), true)
    if cls:
        _class_counts(y, cls, f"{c['id']} {kind}")


# ------------------------------------------------------------------------------------------------ rf_ffn_geglu
@pytest.mark.parametrize("kind,M", C.FFN_RANGE_CASES, ids=[f"{k}-M{m}" for k, m in C.FFN_RANGE_CASES])
def test_ffn_cases_hold_their_classes_and_mutants(kind, M):
    import tokres_exact_refs as T
    k = C.FFN_KINDS[kind]
    c, i = C.ffn_range_inputs(kind, M)
    o = C.ffn_range_reference(c, i, F16)
    C.ffn_range_reference(c, i, BF16)                      # the control's conditions hold on the same data
    true = C.store16(o["out_exact"])
    # the reference against plain torch fp64 (value * gate with gates that GELU leaves unchanged)
    pre = F.linear(i["x"], i["w1"], i["b1"])
    h16 = (pre[:, :T.FF] * pre[:, T.FF:]).float().to(F16).double()
    want = F.linear(h16, i["w2"], i["b2"]) + (i["res"] if i["res"] is not None else 0.0)
    assert torch.equal(want, o["out_exact"]) and torch.equal(T.gelu_sigmoid5(pre[:, T.FF:]).float(), pre[:, T.FF:].float())
    wrong = lambda key, t: C.store16(T.ffn_reference(c, dict(i, **{key: t}), F16)["out_exact"])
    n_sub, n_nz = lambda t: int(C.is_sub16(t).sum()), lambda t: int((t != 0).sum())
    if k["x"] == -24:
        assert n_sub(i["x"]) == n_nz(i["x"]) >= 1000 and C.bits_differ(wrong("x", C.flush_sub(i["x"])), true)
    if k["wv"] == -24:
        wv = i["w1"][:T.FF]
        assert n_sub(wv) == n_nz(wv) >= 1000 and C.bits_differ(wrong("w1", C.flush_sub(i["w1"])), true)
    if k["w2"] == -21:
        assert n_sub(i["w2"]) == n_nz(i["w2"]) >= 1000 and C.bits_differ(wrong("w2", C.flush_sub(i["w2"])), true)
    if kind in ("S-in x, hidden S-out", "S-in W1"):
        # the hidden value, made inside the kernel, is (or rounds to) an fp16 subnormal: the second GEMM's A operand
        h, hs = o["h_exact"], o["h"]
        assert bool((h.abs() < C.NORMAL_MIN).all()) and n_sub(hs) >= 1000 and torch.equal(hs, C.store16(h).double())
        assert C.bits_differ(C.ffn_hidden_mutant(c, i, o, C.store16_flush), true)          # hidden value flushed at its store (or as the A operand)
        assert not C.bits_differ(C.ffn_hidden_mutant(c, i, o, C.store16), true)
    if kind == "S-in x, hidden S-out":
        half = torch.remainder(o["h_exact"].abs() / C.SUB, 1.0)
        odd = torch.remainder(torch.floor(o["h_exact"].abs() / C.SUB), 2.0) == 1
        assert int(((half == 0.5) & odd).sum()) >= 10 and int(((half == 0.5) & ~odd).sum()) >= 10 and int(((half > 0) & (half != 0.5)).sum()) >= 100
        assert C.bits_differ(C.ffn_hidden_mutant(c, i, o, C.store16_trunc), true)          # hidden value truncated instead of rounded
        assert torch.equal(true.double(), o["out_exact"])                                   # (the output itself is representable: what differs is the hidden store)
    if k["steer"]:
        _class_counts(o["out_exact"], k["steer"], f"{c['id']}")


# ------------------------------------------------------------------------------------------------ rf_ffn_block, rf_attn_in, rf_gn_silu_conv3x3_small
def _all_sub(t, least=500):
    return int(C.is_sub16(t).sum()) == int((t != 0).sum()) >= least


@pytest.mark.parametrize("form,kind", C.BLOCK_CASES, ids=[f"{f}-{k}" for f, k in C.BLOCK_CASES])
def test_block_cases_hold_their_classes_and_mutants(form, kind):
    import tokres_exact_refs as T
    k = C.BLOCK_KINDS[kind]
    c, i = C.block_range_inputs(form, kind)
    o = C.block_range_reference(c, i, F16)
    C.block_range_reference(c, i, BF16)                    # the control's conditions hold on the same data
    true = C.store16(o["out_exact"])
    # the last two stages against plain torch fp64: proj_out of the re-rounded feed-forward output, which is W2 of the re-rounded hidden value plus the residual
    resid = o["x1"] if c["form"] == "front" else i["x"]
    x2 = F.linear(o["h"], i["w2"], i["b2"]) + resid
    assert torch.equal(x2, o["x2_exact"]) and torch.equal(F.linear(x2.float().to(F16).double(), i["wpo"], i["bpo"]) + i["res2"][torch.arange(c["M"]) % i["res2"].shape[0]], o["out_exact"])
    wrong = lambda key: C.store16(T.ffn_reference(c, dict(i, **{key: C.flush_sub(i[key])}), F16)["out_exact"])
    if k.get("wpo") == -24:
        assert _all_sub(i["wpo"]) and C.bits_differ(wrong("wpo"), true)
    if k.get("wo") == -24:
        assert _all_sub(i["wo"]) and C.bits_differ(wrong("wo"), true) and _all_sub(o["x1"], 10000) and torch.equal(o["x1"], o["x1_exact"])
        assert not torch.equal(C.flush_sub(o["x1"]), o["x1"])                                # x1 is an output: flushed at its store it differs
    if k.get("x") == -24:
        assert _all_sub(i["x"]) and C.bits_differ(wrong("x"), true)
    if "x2 S-out" in kind:
        x2e = o["x2_exact"]
        half = torch.remainder(x2e.abs() / C.SUB, 1.0)
        odd = torch.remainder(torch.floor(x2e.abs() / C.SUB), 2.0) == 1
        assert bool((x2e.abs() < C.NORMAL_MIN).all()) and int(C.is_sub16(o["x2"]).sum()) >= 10000
        assert int(((half == 0.5) & odd).sum()) >= 10 and int(((half == 0.5) & ~odd).sum()) >= 10 and int(((half > 0) & (half != 0.5)).sum()) >= 100
        for mut in (C.store16_flush, C.store16_trunc):          # the feed-forward output flushed / truncated at its store in front of proj_out
            assert C.bits_differ(C.block_x2_mutant(c, i, o, mut), true), mut.__name__
        assert not C.bits_differ(C.block_x2_mutant(c, i, o, C.store16), true)
    if k.get("steer"):
        _class_counts(o["out_exact"], k["steer"], c["id"])


@pytest.mark.parametrize("kind,shape", C.ATTN_IN_CASES, ids=[f"{k}-{s[0]}x{s[1]}" for k, s in C.ATTN_IN_CASES])
def test_attn_in_cases_hold_their_classes_and_mutants(kind, shape):
    import tokres_exact_refs as T
    k = C.ATTN_IN_KINDS[kind]
    c, i = C.attn_in_range_inputs(kind, shape)
    o = C.attn_in_range_reference(c, i, F16)
    C.attn_in_range_reference(c, i, BF16)
    S, rps = shape
    tok = torch.cat([F.linear(i["x"][s * rps:(s + 1) * rps], i["w"][s], i["rv"][s]) for s in range(S)], 0)          # plain torch fp64
    assert torch.equal(tok, o["tok_exact"])
    assert torch.equal(F.linear(o["xh"], i["wqkv"], i["bqkv"]), o["qkv_exact"])
    wrong = lambda key: T.attn_reference(c, dict(i, **{key: C.flush_sub(i[key])}), F16)
    if k.get("wqkv") == -24:
        assert _all_sub(i["wqkv"]) and C.bits_differ(C.store16(wrong("wqkv")["qkv_exact"]), C.store16(o["qkv_exact"]))
    for key in ("x", "w"):
        if k.get(key) == -24:
            assert _all_sub(i[key]) and C.bits_differ(C.store16(wrong(key)["tok_exact"]), C.store16(o["tok_exact"]))
    if kind == "S-in W'":
        assert int(C.is_sub16(o["tok"]).sum()) > 0.9 * o["tok"].numel() and C.bits_differ(C.store16_flush(o["tok_exact"]), C.store16(o["tok_exact"]))
    if k.get("steer"):
        _class_counts(o["qkv_exact"] if k["steer"][0] == "bqkv" else o["tok_exact"], k["steer"][1], c["id"])


def test_head_cases_hold_their_classes_and_mutants():
    import tokres_exact_refs as T
    for kind, k in C.HEAD_KINDS.items():
        ys = []
        for j in range(len(T.HEAD_SHAPES)):
            c, i = C.head_range_inputs(kind, j)
            o = C.head_range_reference(c, i, F16)
            C.head_range_reference(c, i, BF16)
            true = C.store16(o["out_exact"])
            ys.append(o["out_exact"].reshape(-1))
            # plain torch fp64: group_norm with the moments the partial sums state (mean, var = 4 x^2-scale), then conv2d of the re-rounded result
            B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
            a16 = o["act"].reshape(B, H, W_, Cc).permute(0, 3, 1, 2)
            w4 = i["w"].reshape(c["No"], 9, Cc).permute(0, 2, 1).reshape(c["No"], Cc, 3, 3)
            want = F.conv2d(a16, w4, padding=1).permute(0, 2, 3, 1).reshape(-1, c["No"]) + i["bias"]
            assert torch.equal(want, o["out_exact"]), (kind, j)
            wrong = lambda key: C.store16(T.head_reference(c, dict(i, **{key: C.flush_sub(i[key])}), F16)["out_exact"])
            if k.get("w") == -24:
                assert _all_sub(i["w"], 30) and C.bits_differ(wrong("w"), true)
            if k.get("x") == -24:
                assert _all_sub(i["x"]) and not bool(torch.isfinite(T.head_reference(c, dict(i, x=C.flush_sub(i["x"])), F16)["out_exact"]).all() and torch.equal(wrong("x"), true))
            if kind == "GroupNorm result S-out":
                act = o["act_exact"]
                half = torch.remainder(act.abs() / C.SUB, 1.0)
                assert bool((act.abs() < C.NORMAL_MIN).all()) and int((half == 0.5).sum()) >= 3 and int(C.is_sub16(o["act"]).sum()) >= 3          # (the 2x5x1 image holds 30 live activations)
                for mut in (C.store16_flush, C.store16_trunc):
                    assert C.bits_differ(C.head_act_mutant(c, i, o, mut), true), (kind, j, mut.__name__)
                assert not C.bits_differ(C.head_act_mutant(c, i, o, C.store16), true)
        if k.get("steer"):
            _class_counts(torch.cat(ys), k["steer"], f"head {kind}")


# ------------------------------------------------------------------------------------------------ e. completeness and plans
def test_every_cell_has_a_case():
    have = {cell for c in C.GEMM_CASES for cell in c["range_cells"]}
    missing = [cell for cell in C.GEMM_CELLS if cell not in have]
    assert not missing, missing
    cells = {(c["cell"], c["only"], c["dt"]) for c in C.ATTN_CASES}
    for cell in ("g1", "g2x64", "g2x128", "dma40-kt128", "dma40-kt64", "dma80", "g8"):
        assert {(cell, "tail", "fp16"), (cell, "tail", "bf16"), (cell, "tiny", "fp16"), (cell, "vsub", "fp16"), (cell, "vsub", "bf16")} <= cells, cell
    # the token-resident and small-conv kernels that have range cases: every (kernel, operand or store class) cell is claimed by a kind, at every shape
    want = {("rf_ffn_geglu", "S-in x"), ("rf_ffn_geglu", "hidden S-out"), ("rf_ffn_geglu", "S-in W1"), ("rf_ffn_geglu", "S-in W2"), ("rf_ffn_geglu", "S-out"),
            ("rf_ffn_geglu", "TOP"), ("rf_conv3x3_stem", "S-in x"), ("rf_conv3x3_stem", "S-in taps"), ("rf_conv3x3_stem", "S-out"), ("rf_conv3x3_stem", "TOP")}
    have = {("rf_ffn_geglu", part) for kind, _ in C.FFN_RANGE_CASES for part in kind.split(", ")}
    have |= {("rf_conv3x3_stem", part) for kind, _ in C.STEM_CASES for part in kind.split(", ")}
    want |= {("rf_ffn_block " + f, p) for f in ("plain", "LayerNorm-fused", "to_out in front") for p in ("S-in Wpo", "S-out", "TOP")}
    want |= {("rf_ffn_block plain", "S-in x"), ("rf_ffn_block plain", "x2 S-out"), ("rf_ffn_block to_out in front", "S-in Wo"), ("rf_ffn_block to_out in front", "x1 and x2 S-out")}
    want |= {("rf_attn_in", p) for p in ("S-in Wqkv", "S-out", "TOP", "S-in x", "tok S-out", "S-in W'")}
    want |= {("rf_gn_silu_conv3x3_small", p) for p in ("S-in taps", "S-out", "TOP", "GroupNorm result S-out", "S-in x")}
    have |= {("rf_ffn_block " + f, part.split(",")[0] if part.startswith("TOP") else part) for f, kind in C.BLOCK_CASES for part in kind.replace("TOP, rows", "TOP: rows").split(", ")}
    have |= {("rf_ffn_block " + f, "TOP") for f, kind in C.BLOCK_CASES if kind.startswith("TOP")}
    have |= {("rf_attn_in", part) for kind, _ in C.ATTN_IN_CASES for part in kind.split(", ")}
    have |= {("rf_gn_silu_conv3x3_small", part) for kind, _ in C.HEAD_RANGE_CASES for part in kind.split(", ")}
    for kind in C.ATTN_IN_KINDS:          # every kind at every shape
        assert sum(k == kind for k, _ in C.ATTN_IN_CASES) == len(C.ATTN_IN_SHAPES)
    for kind in C.HEAD_KINDS:
        assert sum(k == kind for k, _ in C.HEAD_RANGE_CASES) == 4
    assert want <= have, sorted(want - have)
    assert {M for _, M in C.FFN_RANGE_CASES} == set(C.FFN_M) and all(sum(k == kind for k, _ in C.FFN_RANGE_CASES) == len(C.FFN_M) for kind in C.FFN_KINDS)


@pytest.mark.parametrize("c", C.GEMM_CASES, ids=IDS)
def test_gemm_case_names_the_plan_the_library_reports(c, monkeypatch):
    monkeypatch.setattr(ops, "_require_gpu", lambda *a: None)
    monkeypatch.setattr(R, "_ints", lambda g, shape, lo, hi, nonzero=True: torch.zeros(shape, dtype=F64))
    monkeypatch.setattr(R, "_keep", lambda g, t, n, cover=False, **kw: t)
    for cc in (c, C.gemm_control(c)):
        if cc is None:
            continue
        i = R.make_inputs(cc)
        P = R.prepare(cc, i, "cpu")
        pl = ops.gemm_plan3(P["launch"])
        if cc["gn"]:
            R.wire_stats(cc, P, pl, "cpu", i)
            pl = ops.gemm_plan3(P["launch"])
        assert not R.plan_matches(pl, cc["expect"]), (cc["id"], cc["op"], R.plan_matches(pl, cc["expect"]))
        assert (pl["splitk"] > 1) == ("reduce" in cc["expect"])


@pytest.mark.parametrize("c", C.ATTN_CASES, ids=[c["id"] for c in C.ATTN_CASES])
def test_attention_case_names_the_plan_the_library_reports(c):
    assert not AR.plan_matches(AR.plan_of(c, ops), c["expect"]), (c["id"], AR.plan_matches(AR.plan_of(c, ops), c["expect"]))


# ------------------------------------------------------------------------------------------------ f. the knobs at their defaults
def test_knobs_at_their_defaults_change_nothing():
    for cid in ("t128x64", "f16-hx", "gn-staged-4wave", "sk-stripe8"):
        c = R.small_of(R.BY_ID[cid])
        assert (c["a_exp"], c["w_exp"], c["e_exp"], c["a_hi"], c["w_hi"], c["range16"]) == (0, 0, 0, 3, 3, False)
        i = R.make_inputs(c)
        assert R.unit_of(c, i) == (0.25 if c["alpha"] == 0.25 else 1.0)
        assert i["x0"].abs().max().item() == 3 and torch.equal(i["x0"], i["x0"].round())
    c = AR.BY_ID["g1-16bit-fp16-d40-b2h3-q129-k65-r4"]
    assert "only" not in c
    q, k, v = AR.operands(c, range(6))
    assert AR.representable(q) and AR.representable(k) and AR.representable(v) and v.abs().max().item() <= 7
    AR.reference(q, k, v, check=True)


def test_layout_edge_inputs_hold_every_pattern():
    x = C.layout_edge_input()
    e = C.edge_values_f32()
    for ch in range(SR.LAYOUT_C):
        have = set(x[:, ch].reshape(-1).view(torch.int32).tolist())
        assert have == set(e.view(torch.int32).tolist()), ch
    i = C.ddim_pack_edge_inputs()
    for key in ("img", "z"):
        assert set(i[key].reshape(-1).view(torch.int32).tolist()) == set(e.view(torch.int32).tolist())
    # the store mutants: each changes a bit of what the GPU file compares, for the layout input and for both packed tensors
    for t in (x, i["img"], i["z"]):
        fin = torch.where(torch.isfinite(t), t, torch.zeros_like(t)).double()          # (the mutants restate finite values; the infinities pass through unchanged)
        for mut in (C.store16_flush, C.store16_trunc, C.store16_saturate):
            assert C.bits_differ(mut(fin), C.store16(fin)), mut.__name__
    assert C.bits_differ(C.store16_flush(i["mask"].double()), C.store16(i["mask"].double()))
    st = x.to(F16)
    assert int(torch.isinf(st).sum()) > int(torch.isinf(x).sum()) and int(C.is_sub16(st.double()).sum()) >= 4 * SR.LAYOUT_C          # overflow and subnormal results occur
