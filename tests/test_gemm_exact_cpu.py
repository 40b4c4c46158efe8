"""CPU checks of tests/gemm_exact_refs.py, the generators, reference and case table of tests/test_gemm_exact_gpu.py:
  a. every generator meets its stated bounds for every row of the case table (partial sums below 2^24 units, 16-bit outputs representable,
     statistics bounds, every k of the contraction visible in some row between the W-sparse and the A-sparse seed);
  b. the reference restatement equals torch's own fp64 conv2d / linear on random real-valued data within 1e-12, for every loop feature;
  c. every slip a kernel could make, written as a deliberately wrong variant of the *reference*, changes an output of EVERY case it applies to
     (a mutant that no case distinguishes fails by name);
  d. the plan every case names is the plan rf_conv_gemm_plan3 reports -- a host-only query, so a dispatch retune shows up without a GPU;
  e. the window cases (KH x KW, stride, pad_t / pad_l, channel-padded inputs, the limits of the packed row descriptor): their reference equals
     torch's fp64 conv2d on the case's own integers, and the window slips change a case exactly where its geometry has what they confuse --
     no slip idle, no case vacuous;
  f. ops.pack_conv_weight writes the [N, K] layout the reference multiplies, and every window a tower launches has a case (TOWER_WINDOWS).
No kernel runs."""
import pytest
import torch
import torch.nn.functional as F

import gemm_exact_refs as R
from reface_amd import ops
from reface_amd.params import seeded_randn as rnd

F64 = torch.float64
SMALL = [R.small_of(c) for c in R.CASES]
IDS = [c["id"] for c in R.CASES]
WC = {320: 160, 160: 160, 256: 128, 128: 64, 64: 64}          # wave_cols of a tile width


def _prepared(c):
    i = R.make_inputs(c)
    ref = R.reference(c, i)
    if c["ln"] == "prod":
        ref = R.steer_stripe_means(c, i, ref, WC[c["expect"]["bn"]])
        assert torch.equal(ref, R.reference(c, i))
    return i, ref


# ------------------------------------------------------------------------------------------------ a. generators
def static_bound(c):
    """the generator's worst case for a row at its FULL size, from the value ranges alone (units of unit_of): alpha K amax wmax + epilogue"""
    G = R.geom(c)
    if c["op"] == "x3":
        per = 263.0 * 263.0 / 16 + 3 * 263.0          # one entry in 16 of A is large; checked on the data below as well
    elif c["op"] == "a8":
        per = 2.0 * 6.0
    elif c["op"] == "w8":
        per = 3.0 * 6.0
    else:
        per = 9.0
    taps = 9 if c["ups"] == 2 else c["kh"] * c["kw"]
    k = taps * (c["C0"] + c["C1"]) + c["Cx"]
    return (abs(c["alpha"]) * k * per + 66 + 7 + 15 + 80) * (2.0 if c["act"] == ops.ACT_PRELU else 1.0) / (min(1.0, c["alpha"]) * (0.25 if c["act"] == ops.ACT_PRELU else 1.0))


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_generators_meet_their_bounds(c):
    s = R.small_of(c)
    if R.other_seed(s) is not None:          # both sparse seeds of a 16-bit case meet the bounds
        R.assert_exact(R.other_seed(s), *_prepared(R.other_seed(s)))
    i, ref = _prepared(s)
    R.assert_exact(s, i, ref)
    if c["op"] == "x3":          # (its worst case, every A entry large, is not what the generator makes: the bound of the row's own data, at full size)
        assert R.magnitude_bound(c, R.make_inputs(c))[0] < R.EXACT_LIMIT
    else:
        assert static_bound(c) < R.EXACT_LIMIT, static_bound(c)                     # the row as the GPU runs it
        assert R.magnitude_bound(s, i)[0] <= static_bound(s)
    for t in (i["x0"], i["x1"], i["xt"]):
        assert t is None or s["out"] == "16" or bool((t != 0).all())             # activations are non-zero (dense seeds)
    if c["op"] == "x3":
        hi, lo = R.split_hi_lo(i["x0"])
        assert bool((lo != 0).any()) and bool((R.split_hi_lo(i["w"])[1] != 0).all()) and torch.equal(hi + lo, i["x0"])
    if c["gn"]:
        assert ref.abs().max().item() <= 128 and s["expect"]["bm"] <= 256
        assert not torch.equal(ref.to(R.out_dtype(s)).to(F64), ref)             # ... and some stored value IS rounded: the stored / unrounded mutant has a witness
    if c["ln"] == "prod":
        wc = WC[c["expect"]["bn"]]
        rec = R.ln_records(ref[0], wc)
        assert torch.equal(rec[..., 0], rec[..., 0].round()) and rec[..., 1].max().item() < R.EXACT_LIMIT and ref.abs().max().item() <= 255
    # nothing constant along an index: bias / rowvec / residual / slopes / scales differ per column, rowvec per sample, residual per row
    for t in (i["bias"], i["slopes"], i.get("wscale")):
        assert t is None or t.unique().numel() > 1
    if i["rowvec"] is not None and s["B"] > 1:
        assert not torch.equal(i["rowvec"][0], i["rowvec"][1])
    if i["res"] is not None:
        assert not torch.equal(i["res"][0, 0], i["res"][0, 1])


def test_sparse_seeds_cover_every_k():
    """every exact 16-bit-output case runs a W-sparse and an A-sparse seed: between the two, every k of the contraction carries a non-zero product
    in some row.  A case without a second seed (dense fp32 output, tolerance epilogues) sees all of K, or -- a single sparse seed -- a good part"""
    for c in SMALL:
        if c["ups"] == 2 and c["korder"]:
            continue
        o = R.other_seed(c)
        if o is None and c["id"].endswith("-W"):
            o = R.small_of(R.BY_ID[c["id"][:-2] + "-A"])
        cov = R.k_coverage(c, R.make_inputs(c))
        if R.is_window_case(c):          # dense: exactly the k whose tap reaches the image and whose channel is a real one (the rest is zero by construction)
            assert torch.equal(cov, R.live_k(c)) and bool(cov.any()), c["id"]
        elif o is not None:
            cov = cov | R.k_coverage(o, R.make_inputs(o))
            assert bool(cov.all()), (c["id"], int((~cov).sum()), cov.numel())
        else:
            f = cov.double().mean().item()
            assert f == 1.0 or (c["out"] == "16" and f > 0.2), (c["id"], f)


# ------------------------------------------------------------------------------------------------ b. the reference against torch fp64
def _pack64(w4, korder, bk):
    """[N, C, kh, kw] fp64 -> [N, K] in rf_conv_gemm's K orders (the weight side of the statement im2col makes on the activation side)"""
    n, ci, kh, kw = w4.shape
    wp = w4.permute(0, 2, 3, 1)
    if korder == 1:
        wp = wp.reshape(n, kh * kw, ci // bk, bk).permute(0, 2, 1, 3)
    elif korder == 2:
        wp = wp.reshape(n, kh, kw, ci // bk, bk).permute(0, 1, 3, 2, 4)
    return wp.reshape(n, kh * kw * ci)


FEATURES = [dict(W=37, C0=72, N=40), dict(B=3, W=20, C0=64, N=48, wps=True, rowvec=True), dict(W=21, C0=64, N=32, batch=3, res=True),
            dict(B=2, H=7, W=6, C0=64, N=24, ks=3, pad=R.P3, rowvec=True, res=True), dict(B=2, H=7, W=6, C0=128, N=24, ks=3, pad=R.P3, korder=1),
            dict(B=2, H=7, W=6, C0=128, N=24, ks=3, pad=R.P3, korder=2), dict(op="f32", B=2, H=7, W=6, C0=64, N=24, ks=3, pad=R.P3, korder=1),
            dict(B=2, H=9, W=11, C0=64, N=24, ks=3, stride=2, pad=(0, 0, 1, 1)), dict(B=2, H=8, W=9, C0=64, N=24, ks=3, stride=2, pad=(1, 0, 0, 1)),
            dict(B=2, H=5, W=4, C0=64, N=24, ks=3, pad=R.P3, ups=1), dict(B=2, H=5, W=4, C0=64, N=24, ks=3, pad=R.P3, ups=2),
            dict(B=2, H=7, W=6, C0=40, C1=24, N=24, ks=3, pad=R.P3), dict(B=2, H=7, W=6, C0=64, Cx=64, N=24, ks=3, pad=R.P3),
            dict(B=2, H=7, W=6, C0=128, Cx=64, N=24, ks=3, pad=R.P3, korder=1), dict(B=1, H=6, W=6, C0=16, N=24, ks=1)]


@pytest.mark.parametrize("k", range(len(FEATURES)))
def test_reference_equals_torch_fp64(k):
    c = R.case(f"feature{k}", (), {}, **FEATURES[k])
    G = R.geom(c)
    i = R.make_inputs(c)
    seed = [500 + 10 * k]

    def real(t):
        seed[0] += 1
        return None if t is None else rnd(tuple(t.shape), seed[0]).double() + 1e-3 * rnd(tuple(t.shape), seed[0] + 100).double() ** 2
    for key in ("x0", "x1", "xt", "bias", "rowvec", "res"):
        i[key] = real(i[key])
    ct, ks, N = G["ctot"], c["ks"], c["N"]
    nb, B = c["batch"], c["B"]
    S = (B if c["wps"] else 1) * nb
    w4 = real(torch.zeros((S, N, ct, ks, ks)))
    wt = real(torch.zeros((N, c["Cx"]))) if c["Cx"] else None
    if c["ups"] == 2:
        i["w3"] = w4[0]
    else:
        i["w"] = torch.stack([torch.cat([_pack64(w4[s], c["korder"], R.bk_of(c))] + ([wt] if wt is not None else []), 1) for s in range(S)], 0)
    got = R.reference(c, i)
    want = []
    for b in range(nb):
        x = i["x0"][b * B:(b + 1) * B]
        if c["C1"]:
            x = torch.cat([x, i["x1"][b * B:(b + 1) * B]], -1)
        x = x.permute(0, 3, 1, 2)
        if c["ups"]:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        pt, pl, pb, pr = R.P3 if c["ups"] == 2 else c["pad"]
        x = F.pad(x, (pl, pr, pt, pb))
        ys = []
        for s in range(B if c["wps"] else 1):
            xs = x[s:s + 1] if c["wps"] else x
            ys.append(F.conv2d(xs, w4[b * (B if c["wps"] else 1) + s], stride=1 if c["ups"] == 2 else c["stride"]))
        y = torch.cat(ys, 0)
        if wt is not None:
            y = y + F.conv2d(i["xt"][b * B:(b + 1) * B].permute(0, 3, 1, 2), wt[:, :, None, None])
        y = y.permute(0, 2, 3, 1).reshape(G["M"], N) * c["alpha"] + i["bias"][None]
        if c["rowvec"]:
            y = y + i["rowvec"].repeat_interleave(G["rps"], 0)
        if c["res"]:
            y = y + i["res"][b]
        want.append(y)
    want = torch.stack(want, 0)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    if c["ups"] == 2:          # the folded statement of the header is the same function
        folded = R.ups2_folded(c, i["x0"], i["w3"]) * c["alpha"] + i["bias"][None]
        assert (folded - want[0]).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_reference_epilogues_equal_torch_fp64():
    c0 = R.case("epi", (), {}, W=33, N=128, res=True, rowvec=True, B=1)
    h = rnd((33, 128), 700).double() * 3
    i = dict(bias=rnd((128,), 701).double(), rowvec=rnd((1, 128), 702).double(), res_cur=rnd((33, 128), 703).double(), slopes=rnd((128,), 704).double().abs())
    pre = h + i["bias"][None] + i["rowvec"]
    for act, fn in ((ops.ACT_NONE, lambda v: v), (ops.ACT_SILU, F.silu), (ops.ACT_GELU, F.gelu), (ops.ACT_RELU, F.relu), (ops.ACT_SIGMOID, torch.sigmoid),
                    (ops.ACT_QUICK_GELU, lambda v: v * torch.sigmoid(1.702 * v)), (ops.ACT_PRELU, lambda v: F.prelu(v, i["slopes"]))):
        c = dict(c0, act=act)
        assert (R.epilogue(c, h, i) - (fn(pre) + i["res_cur"])).abs().max().item() <= 1e-12
    assert (R.epilogue(dict(c0, act=ops.ACT_ADD_RELU), h, i) - F.relu(pre + i["res_cur"])).abs().max().item() <= 1e-12
    cg = dict(c0, act=ops.ACT_GEGLU, rowvec=False, op="f32")
    ig = dict(i, rowvec=None)
    pre = (h + i["bias"][None]).reshape(33, 2, 2, 32)
    want = (pre[:, :, 0] * F.gelu(pre[:, :, 1])).reshape(33, 64) + i["res_cur"][:, :64]
    ig["res_cur"] = i["res_cur"][:, :64]
    assert (R.epilogue(cg, h, ig) - want).abs().max().item() <= 1e-12
    # the 16-bit modes' gate: the documented sigmoid form, <= 2.6e-5 from erf GELU over the reals
    xs = torch.linspace(-12, 12, 200001, dtype=F64)
    assert R.gate_of(dict(op="bf16")) is R.gelu_sigmoid5 and (R.gelu_sigmoid5(xs) - F.gelu(xs)).abs().max().item() <= 2.6e-5
    assert torch.equal(R.gelu_sigmoid5(torch.tensor([32.0, 64.0], dtype=F64)).float(), torch.tensor([32.0, 64.0]))          # saturated: the exact-gate cases
    # the packing ops.pack_geglu produces is the interleave the epilogue undoes
    w, b = rnd((128, 8), 705), rnd((128,), 706)
    wp, bp = ops.pack_geglu(w, b, torch.float32)
    x = rnd((5, 8), 707)
    a, g = F.linear(x, w, b).double().chunk(2, -1)
    assert (R.epilogue(dict(cg, res=False), F.linear(x, wp).double(), dict(bias=bp.double(), rowvec=None, res_cur=None)) - a * F.gelu(g)).abs().max().item() <= 1e-5


# ------------------------------------------------------------------------------------------------ c. mutants
def _sk(c):
    """the split-K factor a mutant is run at: the one the case froze from the plan, else 2 for a case with a workspace"""
    return c["expect"].get("splitk", 2) if c["ws"] else 1


def _applies(m, c):
    if m in R.WINDOW_MUTANTS:          # the window slips answer to the window cases (two-sided check below)
        return R.is_window_case(c) and R.window_mutant_applies(m, c, _sk(c))
    conv3 = c["ks"] == 3 or c["ups"] == 2
    if R.is_window_case(c) and m in ("drop_last_k", "tap_transposed", "halo_from_adjacent_row"):
        # dense window cases at extreme shapes: the slip must have something to confuse -- a live last k (not a zero weight column of a padded
        # channel, not a tap that only ever meets padding), two different off-diagonal taps inside the image, a neighbouring image row
        live = R.live_k(c)
        tt = c["H"] > 1 and c["W"] > 1 and c["kh"] == c["kw"] and c["kh"] > 1
        return {"drop_last_k": bool(live[-1]), "tap_transposed": tt, "halo_from_adjacent_row": conv3 and c["pad"][1] > 0 and c["H"] > 1}[m]
    return {"drop_last_k": True, "double_k_tile": _sk(c) > 1, "tap_transposed": conv3,
            "halo_from_adjacent_row": conv3 and (c["ups"] == 2 or c["pad"][1] > 0), "pad_top_bottom_swapped": c["pad"][0] != c["pad"][2],
            "phase_swapped": c["ups"] == 2, "phase00_padding": c["ups"] == 2, "concat_swapped": c["C1"] > 0, "tail_at_input_pixel": c["Cx"] > 0,
            "korder_confused": c["korder"] > 0 and c["ups"] != 2, "rowvec_neighbour": c["rowvec"] and c["B"] > 1, "residual_row_plus_1": c["res"],
            "nsplit_bias_offset": c["expect"].get("gemm_kernels") == 2, "geglu_swapped": c["act"] == ops.ACT_GEGLU, "wps_sample0": c["wps"],
            "stat_slot_plus_1": c["gn"], "stat_unrounded": c["gn"], "tile_permuted": "pm" in c["expect"]}[m]


def _differs(c, wrong, true):
    if R.is_exact(c):
        odt = R.out_dtype(c)
        return not torch.equal(wrong.to(odt), true.to(odt))
    lim = R.limit_of(c, true)
    return bool(((wrong - true).abs() > lim).any())


@pytest.mark.parametrize("m", R.MUTANTS)
def test_mutant_is_told_apart_by_every_case_it_applies_to(m):
    cases = [c for c in SMALL if _applies(m, c)]
    assert cases, f"mutant {m}: no case of the table applies"
    missed = []
    for c in cases:
        i, ref = _prepared(c)
        if m in ("stat_slot_plus_1", "stat_unrounded"):
            bm, bn = c["expect"]["bm"], c["expect"]["bn"]
            st = (32, WC[bn]) if c["ws"] else (bm, bn)
            stored = ref[0].to(R.out_dtype(c)).to(F64)
            for cpg, coff in R.gn_consumers(c):
                true = R.gn_expected(stored, c, st[0], st[1], cpg, coff)
                buf = torch.full((true.shape[0], true.shape[1] + 2, 32, 2), float("nan"), dtype=F64)
                want = buf.clone()
                want[:, 1:-1] = true
                if m == "stat_slot_plus_1":
                    buf[:, 2:] = true
                else:
                    buf[:, 1:-1] = R.gn_expected(stored, c, st[0], st[1], cpg, coff, mut_unrounded=ref[0])
                if torch.equal(torch.nan_to_num(buf, nan=-1.0), torch.nan_to_num(want, nan=-1.0)):
                    missed.append(c["id"])
            continue
        if m == "tile_permuted":
            bm, bn = c["expect"]["bm"], c["expect"]["bn"]
            wrong = ref.clone()
            wrong[:, :bm, :bn], wrong[:, :bm, bn:2 * bn] = ref[:, :bm, bn:2 * bn], ref[:, :bm, :bn]
        else:
            n_split = 256 if c["expect"].get("gemm_kernels") == 2 else 0          # (the scaled-down N split: whole 256-wide tiles, then the tail)
            wrong = R.reference(c, i, m, sk=_sk(c), n_split=n_split)
        if not _differs(c, wrong, ref):
            missed.append(c["id"])
    assert not missed, f"mutant {m} is not told apart by: {missed}"
    print(f"[gemm_exact] mutant {m}: told apart by all {len(cases)} cases it applies to")


# ------------------------------------------------------------------------------------------------ d. the plans, without a GPU
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_case_names_the_plan_the_library_reports(c, monkeypatch):
    monkeypatch.setattr(ops, "_require_gpu", lambda *a: None)          # a plan query reads sizes and alignments only
    monkeypatch.setattr(R, "_ints", lambda g, shape, lo, hi, nonzero=True: torch.zeros(shape, dtype=F64))
    monkeypatch.setattr(R, "_x3_values", lambda g, shape, every: torch.zeros(shape, dtype=F64))
    monkeypatch.setattr(R, "_keep", lambda g, t, n, cover=False, **kw: t)
    P = R.prepare(c, R.make_inputs(c), "cpu")
    pl = ops.gemm_plan3(P["launch"])
    if c["gn"] or c["ln"]:
        R.wire_stats(c, P, pl, "cpu", R.make_inputs(c))
        pl = ops.gemm_plan3(P["launch"])
    assert not R.plan_matches(pl, c["expect"]), (c["id"], R.plan_matches(pl, c["expect"]))
    assert (pl["splitk"] > 1) == ("reduce" in c["expect"])
    p2 = ops.gemm_plan2(P["launch"])
    assert all(pl[k] == v for k, v in p2.items())                      # plan3's first words are plan2's


def test_every_cell_has_a_case_and_plan3_is_exported():
    from reface_amd import _lib
    assert _lib.load().rf_version() >= 104 and "rf_conv_gemm_plan3" in _lib.EXPORTS
    have = {cell for c in R.CASES for cell in c["cells"]}
    assert not [cell for cell in R.CELLS if cell not in have]


# ------------------------------------------------------------------------------------------------ e. the window cases
WIN = R.WINDOW_CASES
WIN_IDS = [c["id"] for c in WIN]


@pytest.fixture(scope="module")
def win_refs():
    """inputs and fp64 reference of every window case, computed once"""
    return {c["id"]: _prepared(c) for c in WIN}


def _w4(c, i):
    """the [N, Cin, KH, KW] filter a case's [N, K] weight matrix is the packing of"""
    N, kh, kw, ct = c["N"], c["kh"], c["kw"], c["C0"]
    w = i["w"][0]
    if c["korder"] == 1:
        bk = R.bk_of(c)
        w = w.reshape(N, ct // bk, kh * kw, bk).permute(0, 2, 1, 3)
    assert c["korder"] < 2
    return w.reshape(N, kh, kw, ct).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("c", WIN, ids=WIN_IDS)
def test_window_reference_equals_conv2d_fp64(c, win_refs):
    """the KH x KW / stride / pad_t, pad_l reference against torch's own conv2d in float64 on the case's own integer operands: equal, not close"""
    i, ref = win_refs[c["id"]]
    pt, pl, pb, pr = c["pad"]
    x = F.pad(i["x0"].permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(x, _w4(c, i), stride=c["stride"]).permute(0, 2, 3, 1).reshape(-1, c["N"])
    assert y.shape[0] == R.geom(c)["M"]
    if i["bias"] is not None:
        y = y + i["bias"][None]
    if c["act"] == ops.ACT_ADD_RELU:
        y = F.relu(y + i["res"][0])
    else:
        assert c["act"] in (ops.ACT_NONE, ops.ACT_RELU) and not c["res"]
        y = F.relu(y) if c["act"] == ops.ACT_RELU else y
    assert torch.equal(ref[0], y)
    R.assert_exact(c, i, ref)                                      # all partial sums below 2^24
    assert R.magnitude_bound(c, i)[0] <= 9 * R.geom(c)["K"] + 7 + 15 < R.EXACT_LIMIT


def test_window_mutants_two_sided(win_refs):
    """every window slip changes an output of some window case, every window case is changed by some window slip -- and a slip changes a case exactly
    where the case's geometry has what the slip confuses (gemm_exact_refs.window_mutant_applies): no case is vacuous, no mutant is idle"""
    changed = set()
    for c in WIN:
        i, ref = win_refs[c["id"]]
        for m in R.WINDOW_MUTANTS:
            if _differs(c, R.reference(c, i, m, sk=_sk(c)), ref):
                changed.add((m, c["id"]))
    applies = {(m, c["id"]) for c in WIN for m in R.WINDOW_MUTANTS if R.window_mutant_applies(m, c, _sk(c))}
    assert changed == applies, (sorted(changed - applies), sorted(applies - changed))
    idle = [m for m in R.WINDOW_MUTANTS if not any(k[0] == m for k in changed)]
    vacuous = [c["id"] for c in WIN if not any(k[1] == c["id"] for k in changed)]
    assert not idle and not vacuous, (idle, vacuous)
    for m in R.WINDOW_MUTANTS:
        print(f"[gemm_exact] window mutant {m}: changes {sorted(k[1] for k in changed if k[0] == m)}")


def test_split_slices_start_inside_the_window():
    """the split-K cases of the non-square window: some slice starts at a tap that is not the first of a window row"""
    for cid in ("win-5x3-lds-k1", "win-5x3-lds-sk"):
        c = R.BY_ID[cid]
        starts, nk = R.slice_starts(c, c["expect"]["splitk"])
        assert nk == 30 and any(R.tap_of_tile(c, t0) % c["kw"] for t0 in starts[1:]), (cid, starts)


# ------------------------------------------------------------------------------------------------ f. host packing and the tower table
@pytest.mark.parametrize("c", WIN, ids=WIN_IDS)
def test_pack_conv_weight_gives_the_layout_the_reference_multiplies(c, win_refs):
    i, _ = win_refs[c["id"]]
    w4 = _w4(c, i)
    cr = c["creal"] or c["C0"]
    assert not bool(w4[:, cr:].any())
    got = ops.pack_conv_weight(w4[:, :cr].float(), R.TDT[c["op"]], cin_pad=c["C0"] if c["creal"] else None, korder=c["korder"])
    assert got.dtype == R.TDT[c["op"]] and got.is_contiguous() and torch.equal(got.double(), i["w"][0])


@pytest.mark.parametrize("kh,kw", [(1, 1), (3, 3), (5, 5), (7, 7), (11, 11), (14, 14), (5, 3), (1, 7)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_conv_weight_index_formula(kh, kw, dtype):
    """k = (ky KW + kx) Cin_pad + c (korder 0), ((c / BK) KH KW + tap) BK + c % BK (korder 1), ((ky (Cin_pad / BK) + c / BK) KW + kx) BK + c % BK (korder 2),
    restated as index arithmetic; pad channels are zero columns"""
    bk = 32 if dtype == torch.float32 else 64
    for ci, cp, korders in ((3, 8, (0,)), (3, 4, (0,)), (bk + 3, 2 * bk, (0, 1, 2)), (2 * bk, None, (0, 1, 2))):
        n = 5
        w = (torch.arange(n * ci * kh * kw) % 251 - 125).float().reshape(n, ci, kh, kw)          # integers bf16 holds exactly, no two neighbours alike
        cpad = cp or ci
        cc, ky, kx = torch.meshgrid(torch.arange(ci), torch.arange(kh), torch.arange(kw), indexing="ij")
        for ko in korders:
            k = {0: (ky * kw + kx) * cpad + cc, 1: ((cc // bk) * kh * kw + ky * kw + kx) * bk + cc % bk, 2: ((ky * (cpad // bk) + cc // bk) * kw + kx) * bk + cc % bk}[ko]
            want = torch.zeros((n, kh * kw * cpad))
            want[:, k.reshape(-1)] = w.reshape(n, -1)
            got = ops.pack_conv_weight(w, dtype, cin_pad=cp, korder=ko)
            assert got.shape == want.shape and got.dtype == dtype and torch.equal(got.float(), want), (kh, kw, ci, cp, ko)


def test_tower_windows_table_names_a_case_for_every_launched_window():
    from reface_amd.params import lpips_plan
    rows = {k[1:]: v for k, v in R.TOWER_WINDOWS.items()}
    for net in ("alex", "vgg"):
        first = True
        for p in lpips_plan(net):
            if p[0] != "conv":
                continue
            _, _, cin, _, k, s, pad = p
            stored = 8 if first else 64          # lpips.py: cin_pad=CP if first else None; every later layer has a multiple of 64 channels
            assert first or cin % 64 == 0
            assert (k, k, s, pad, stored, "f32") in rows, (net, p)
            first = False
    for (who, kh, kw, s, pad, stored, op), cid in R.TOWER_WINDOWS.items():
        c = R.BY_ID[cid]
        assert (c["kh"], c["kw"], c["stride"], c["pad"][0], c["pad"][1], c["op"]) == (kh, kw, s, pad, pad, op), (who, cid)
        assert (c["C0"] == stored if stored < 64 else c["C0"] % 64 == 0) and c["C1"] == 0 and c["ups"] == 0, (who, cid)
        assert c["expect"]["glds"] == (0 if stored < 64 else 1) and c["expect"]["conv"] == 1, (who, cid)
