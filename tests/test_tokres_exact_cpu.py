"""CPU checks of tests/tokres_exact_refs.py, the generators, references and case table of tests/test_tokres_exact_gpu.py:
  a. every generator meets its stated bounds for every case, seed and 16-bit type: operands representable, partial sums below 2^24 units, gate
     pre-activations 0 or integers >= 7, two-level LayerNorm rows with r clear of a rounding boundary, SiLU levels clear of one, statistics sums
     exact, weights that no stale LDS stage reproduces, and the K coverage between the seeds;
  b. the fp64 references equal independent torch fp64 restatements (F.linear / F.layer_norm / F.conv2d chains) within 1e-12;
  c. every slip a kernel could make, written as a deliberately wrong variant of the *reference*, changes an expected output or statistics word of
     some case (a mutant that no case distinguishes fails by name);
  d. every mechanism the issue names has a case.
No kernel runs."""
import functools

import pytest
import torch
import torch.nn.functional as F

import norm_refs as NR
import tokres_exact_refs as R

F64 = torch.float64
C, FF = R.C, R.FF
IDS = [c["id"] for c in R.CASES]
BF = torch.bfloat16


@functools.lru_cache(maxsize=8)
def _inputs(cid, seed):
    c = R.BY_ID[cid]
    return R.INPUTS[c["kernel"]](c, seed)


def _ref(c, seed, dt, mut=None):
    return R.REFERENCE[c["kernel"]](c, _inputs(c["id"], seed), dt, mut)


# ------------------------------------------------------------------------------------------------ a. generators
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_generators_meet_their_bounds(c):
    k = c["kernel"]
    for seed in c["seeds"]:
        i = _inputs(c["id"], seed)
        for dt in R.DTS.values():
            R.ASSERT_EXACT[k](c, i, dt, _ref(c, seed, dt))
        if k == "ffn":
            assert R.ffn_periods(i), f"{c['id']}/{seed}: a weight tile repeats with the period of its LDS ring"
            for t in ("b1", "b2", "bpo", "bo"):
                assert i.get(t) is None or not bool((i[t] != 0).any()) or i[t].unique().numel() > 1
            if c["form"] == "front" and not c["ln"]:
                assert not torch.equal(i["ctx"][0], i["ctx"][1])
        if k == "attn_in":
            assert R.attn_periods(i), f"{c['id']}/{seed}"
            assert c["S"] == 1 or not torch.equal(i["w"][0], i["w"][1])


def test_layernorm_levels_in_fp32():
    """the kernel's route to r -- sq = 320 a^2 exactly, one division, one add, sqrtf, one reciprocal, one multiply, all fp32 -- lands on the storage value the
    fp64 reference rounds to, for every a the generators use; a >= 1/4 gives exactly 1; constant rows give 0 with a finite rstd"""
    a = torch.tensor([2.0 ** e for e in R.A_EXPS] + [8.0], dtype=torch.float32)
    sq = torch.zeros_like(a)
    for _ in range(C):
        sq = sq + a * a
    assert torch.equal(sq.double(), C * a.double() ** 2)
    rstd = 1.0 / torch.sqrt(sq / float(C) + torch.tensor(R.LN_EPS, dtype=torch.float32))
    r64 = a.double() / torch.sqrt(a.double() ** 2 + R.LN_EPS)
    for dt in R.DTS.values():
        got = (a * rstd).to(dt)
        assert torch.equal(got, r64.float().to(dt)), dt
        assert bool((got[a >= 0.25].double() == 1.0).all())
        assert R.boundary_margin(r64, dt) >= 2.0 ** -20
    assert bool(torch.isfinite(1.0 / torch.sqrt(torch.tensor(R.LN_EPS, dtype=torch.float32))))
    assert abs(r64[0].item() - 0.927) < 1e-3          # a = 2^-7: eps is visible


def test_silu_levels_clear_of_rounding_boundaries():
    assert R.silu_levels_ok() >= R.SILU_MARGIN, R.silu_levels_ok()
    # ... and the sums of the rounded activations stay exact: the smallest unit among them against the largest table row sum
    lv = torch.tensor([v for v in R.SILU_LEVELS if v], dtype=F64)
    for dt in R.DTS.values():
        assert 8.0 * 3 * 9 * 4 / R.unit_of(R.r16(NR.silu64(lv), dt)) < R.EXACT_LIMIT


def _union(covs):
    out = None
    for cv in covs:
        out = cv if out is None else {k: out[k] | cv[k] for k in cv}
    return out


@pytest.mark.parametrize("c", R.FFN_CASES, ids=[c["id"] for c in R.FFN_CASES])
def test_ffn_seeds_cover_every_k(c):
    """between the seeds of a case every k of every contraction -- W1 value and gate rows, W2, Wpo, Wo -- carries a non-zero product in some output, the
    first and the last k in many rows; and where a seed keeps a matrix dense (see the module docstring of the references), every (row, k) of it does"""
    cov = _union([R.ffn_coverage(c, _inputs(c["id"], s), _ref(c, s, BF)) for s in c["seeds"]])
    const_gate = c["ln"] or c["form"] == "front"
    for name, m in cov.items():
        parts = {"w1 value": m[:FF], "w1 gate": m[FF:]} if name == "w1" else {name: m}
        for pn, p in parts.items():
            if pn == "w1 gate" and const_gate:
                continue          # (the gate comes from b1 there: the gate rows of W1 are zero)
            assert bool(p.any(0).all()), f"{c['id']}: {pn}: k = {(~p.any(0)).nonzero().flatten().tolist()[:8]} never shows"
            perm = pn == "wo" and c["ln"]          # (a signed permutation: one entry per row and per k)
            assert perm or (int(p[:, 0].sum()) >= 8 and int(p[:, -1].sum()) >= 8), f"{c['id']}: {pn}: the ends of the contraction are live in too few rows"
            assert bool(p.any(1).all()), f"{c['id']}: {pn}: a weight row never shows"
    seeds = set(c["seeds"])
    if "A" in seeds and c["form"] != "front":
        assert bool(cov["w1"][:FF].all()), f"{c['id']}: W1 value rows: {int((~cov['w1'][:FF]).sum())} positions never show"
        assert c["ln"] or bool(cov["w1"][FF:].all()), f"{c['id']}: W1 gate rows"
    if "G" in seeds:
        assert bool(cov["w2"].all()), f"{c['id']}: W2: {int((~cov['w2']).sum())} positions never show"
    if "P" in seeds:
        assert bool(cov["wpo"].all()), f"{c['id']}: Wpo: {int((~cov['wpo']).sum())} positions never show"
    if c["form"] == "front" and "A" in seeds:
        assert bool(cov["wo"].all()), f"{c['id']}: Wo"


def test_attn_in_seeds_cover_every_position():
    for c in R.ATTN_CASES:
        seen_w, seen_q = torch.zeros((c["S"], C, C), dtype=torch.bool), torch.zeros((3 * C, C), dtype=torch.bool)
        for s in c["seeds"]:
            i, o = _inputs(c["id"], s), _ref(c, s, BF)
            for b in range(c["S"]):
                seen_w[b] |= (i["x"][b * c["rps"]:(b + 1) * c["rps"]] != 0).any(0)[None, :] & (i["w"][b] != 0)
            seen_q |= (o["xh"] != 0).any(0)[None, :] & (i["wqkv"] != 0)
        if c["two_level"]:          # W'_s is a signed permutation there: its one entry per row shows; Wqkv is dense in seed A
            assert bool(seen_w.any(2).all()) and bool(seen_q.all()), c["id"]
        else:
            assert bool(seen_w.all()) and bool(seen_q.all()), c["id"]


def test_conv_tables_are_covered():
    """between the seeds and images of a channel count, every (row, tap, channel) of the stem and out-head tables carries a non-zero product in some output
    (a tap shows at the pixels whose source lies inside the image: the reference's own tap tensor says where)"""
    for cases, key in ((R.STEM_CASES, "stem"), (R.HEAD_CASES, "head")):
        seen = dict()
        for c in cases:
            for s in c["seeds"]:
                i, o = _inputs(c["id"], s), _ref(c, s, BF)
                live = (o["A"] != 0).any(0)[None, :] & (i["w"] != 0)
                k = (c["C"], c.get("No", 0))
                seen[k] = live if k not in seen else seen[k] | live
        for k, live in seen.items():
            if key == "stem":
                live = live.reshape(-1, 9, 16)[..., :9]          # the pad channels never show: that is the contract
            assert bool(live.all()), f"{key} {k}: {int((~live).sum())} table positions never show"


# ------------------------------------------------------------------------------------------------ b. the references against torch fp64
def _close(a, b, what):
    assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), f"{what}: {float((a - b).abs().max())}"


def _group_sums(t, S, cpg, coff, width):
    """independent statement of the partial sums: the tensor placed at column coff of a `width`-channel buffer, summed per 128-row block and group of cpg channels"""
    M, n = t.shape
    wide = torch.zeros((M, 32 * cpg), dtype=F64)
    wide[:, coff:coff + n] = t
    blocks = wide.reshape(S, M // S // 128, 128, 32, cpg)
    return torch.stack([blocks.sum((2, 4)), (blocks * blocks).sum((2, 4))], -1)


@pytest.mark.parametrize("cid", ["geglu-M128-raw-res", "geglu-M300-ln-nores", "tail-b-stats-raw", "tail-b-stats-ln", "tail-c-pair-raw", "tail-a-ragged-ln", "front-d-raw",
                                 "front-e-pair-ln"])
def test_ffn_reference_against_torch(cid):
    c = R.BY_ID[cid]
    for seed in c["seeds"]:
        i = _inputs(cid, seed)
        for dt in R.DTS.values():
            o = _ref(c, seed, dt)
            st = lambda t: t.float().to(dt).to(F64)
            M = c["M"]
            if c["form"] == "front":
                reps = M // (c["front_rows"] or M)
                x1 = F.linear(i["att"].repeat(reps, 1), i["wo"], i["bo"]) + i["ctx"].repeat_interleave(c["rps0"], 0) + i["res0"].repeat(reps, 1)
                _close(o["x1_exact"], x1, f"{cid} x1")
                x = resid = st(x1)
            else:
                x = i["x"]
                resid = i["res"] if c["form"] == "geglu" else x
            xh = st(F.layer_norm(x, (C,), None, None, R.LN_EPS)) if c["ln"] else x
            a, g = F.linear(xh, i["w1"], i["b1"]).chunk(2, -1)
            h = st(a * R.gelu_sigmoid5(g))
            x2 = F.linear(h, i["w2"], i["b2"]) + (resid if resid is not None else 0.0)
            _close(o["x2_exact"], x2, f"{cid} feed-forward output")
            if c["form"] == "geglu":
                continue
            out = F.linear(st(x2), i["wpo"], i["bpo"]) + i["res2"].repeat(M // i["res2"].shape[0], 1)
            _close(o["out_exact"], out, f"{cid} out")
            for k, (cpg, coff) in enumerate(R.FFN_CONSUMERS[:c["stats"]]):
                _close(o["stats"][k], _group_sums(st(out), c["S"], cpg, coff, 32 * cpg), f"{cid} statistics {k}")


@pytest.mark.parametrize("c", R.ATTN_CASES, ids=[c["id"] for c in R.ATTN_CASES])
def test_attn_in_reference_against_torch(c):
    for seed in c["seeds"]:
        i = _inputs(c["id"], seed)
        for dt in R.DTS.values():
            o = _ref(c, seed, dt)
            st = lambda t: t.float().to(dt).to(F64)
            tok = torch.cat([F.linear(i["x"][s * c["rps"]:(s + 1) * c["rps"]], i["w"][s], i["rv"][s]) for s in range(c["S"])], 0)
            _close(o["tok_exact"], tok, "tok")
            xh = F.layer_norm(st(tok), (C,), None, None, R.LN_EPS)
            _close(o["xh_exact"], xh, "normalised tok")
            _close(o["qkv_exact"], F.linear(st(xh), i["wqkv"], i["bqkv"]), "qkv")


@pytest.mark.parametrize("c", R.STEM_CASES[::5] + R.HEAD_CASES[::7], ids=[c["id"] for c in R.STEM_CASES[::5] + R.HEAD_CASES[::7]])
def test_conv_references_against_torch(c):
    B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
    for seed in c["seeds"]:
        i = _inputs(c["id"], seed)
        for dt in R.DTS.values():
            o = _ref(c, seed, dt)
            if c["kernel"] == "stem":
                w4 = i["w"].reshape(Cc, 3, 3, 16)[..., :9].permute(0, 3, 1, 2)
                ref = F.conv2d(i["x"][..., :9].permute(0, 3, 1, 2), w4, i["bias"], padding=1).permute(0, 2, 3, 1).reshape(-1, Cc)
                _close(o["out_exact"], ref, c["id"])
                for k, (cpg, coff, s0, n) in enumerate(R.stem_consumers(c)):
                    _close(o["stats"][k], _group_sums(o["out"], B, cpg, coff, 32 * cpg), f"{c['id']} statistics {k}")
            else:
                # GroupNorm with the statistics the partial sums state (mean m, variance 4, eps 0), then SiLU, the storage rounding and the convolution
                mean = i["mean"].repeat_interleave(Cc // 32, 1)[:, None, None, :]
                y = (i["x"] - mean) / 2.0 * i["gamma"] + i["beta"]
                act = (F.silu(y) if c["silu"] else y).float().to(dt).to(F64)
                w4 = i["w"].reshape(c["No"], 3, 3, Cc).permute(0, 3, 1, 2)
                ref = F.conv2d(act.permute(0, 3, 1, 2), w4, i["bias"], padding=1).permute(0, 2, 3, 1).reshape(-1, c["No"])
                _close(o["out_exact"], ref, c["id"])


def test_gate_sweep_attribution():
    """the sweep's reference: row m returns value[m] * gelu(gate of hidden unit 320 (m % 4) + n) at column n -- checked against the fp64 chain"""
    i, value, gate = R.gate_sweep_inputs()
    a, g = F.linear(i["x"], i["w1"], i["b1"]).chunk(2, -1)
    out = F.linear(a * R.gelu_erf(g), i["w2"], i["b2"])
    _close(out, value * R.gelu_erf(gate), "gate sweep")
    gs = i["b1"][FF:]
    assert gs.min() == -9 and gs.max() == 9 and all(bool((gs == v).any()) for v in (7.0, -7.0))
    seven = torch.tensor(7.0)
    for nb in (torch.nextafter(seven, torch.tensor(0.0)), torch.nextafter(seven, torch.tensor(9.0))):
        assert bool((gs == nb.double()).any()) and bool((gs == -nb.double()).any())
    # the 16-bit modes' form against erf, over the reals: the constant the bound uses
    xs = torch.linspace(-9, 9, 200001, dtype=F64)
    assert float((R.gelu_sigmoid5(xs) - R.gelu_erf(xs)).abs().max()) <= R.GATE_FORM_ERR


# ------------------------------------------------------------------------------------------------ c. the reference has teeth
def _differs(a, b):
    keys = [k for k in ("x1", "out", "tok", "qkv") if k in a]
    if any(not torch.equal(a[k], b[k]) for k in keys):
        return True
    return any(not torch.equal(s, t) for s, t in zip(a.get("stats", []), b.get("stats", [])))


@pytest.mark.parametrize("kernel,mut", [(k, m) for k, ms in R.MUTANTS.items() for m in ms], ids=[f"{k}-{m}" for k, ms in R.MUTANTS.items() for m in ms])
def test_every_mutant_changes_an_expected_value(kernel, mut):
    """a deliberately wrong reference must disagree with the right one in some stored output or statistics word of some case: otherwise the GPU test could not
    see the kernel make that slip"""
    hits = []
    for c in R.CASES:
        if c["kernel"] != kernel:
            continue
        for seed in c["seeds"]:
            for dn, dt in R.DTS.items():
                if _differs(_ref(c, seed, dt), _ref(c, seed, dt, mut)):
                    hits.append(f"{c['id']}/{seed}/{dn}")
        if len(hits) >= 2:
            break
    assert hits, f"no case distinguishes the mutant {mut} of {kernel}"
    print(f"[tokres_exact] mutant {kernel}/{mut}: first seen by {hits[0]}")


# ------------------------------------------------------------------------------------------------ d. completeness
def test_every_cell_of_the_issue_has_a_case():
    have = {cell for c in R.CASES for cell in c["cells"]}
    missing = [cell for cell in R.CELLS if cell not in have]
    assert not missing, missing
    assert all(len(c["seeds"]) >= 2 for c in R.CASES)
    # the table of the issue, by count: 12 plain feed-forward cases, 3 tail shapes x 2 ln_eps, 2 FRONT cases, 3 + 3 rf_attn_in cases,
    # 3 C x 4 images x dup on / off stem cases, and every (C, No) of the out head on every image
    n = lambda k: sum(1 for c in R.CASES if c["kernel"] == k)
    assert (n("ffn"), n("attn_in"), n("stem")) == (20, 6, 24)
    assert {(c["C"], c["No"], c["H"], c["W"]) for c in R.HEAD_CASES} == {(Cc, No, H, W_) for Cc in (64, 128, 320) for No in (1, 3, 4) for _, H, W_ in R.HEAD_SHAPES}
    for Cc in (64, 128, 320):
        for No in (1, 3, 4):
            sub = [c for c in R.HEAD_CASES if (c["C"], c["No"]) == (Cc, No)]
            assert {c["out"] for c in sub} == {"f32", "16"} and {c["silu"] for c in sub} == {0, 1} and {c["nchunks"] for c in sub} == {1, 9}
