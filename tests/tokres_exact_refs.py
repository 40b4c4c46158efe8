"""Exact-operand cases of the token-resident and small-conv kernels -- rf_ffn_geglu / rf_ffn_block (csrc/ffn.hip), rf_attn_in (csrc/attnin.hip),
rf_conv3x3_stem and rf_gn_silu_conv3x3_small (csrc/smallconv.hip) -- and their fp64 references: shared by tests/test_tokres_exact_gpu.py (launches)
and tests/test_tokres_exact_cpu.py (generator bounds, references against torch, mutants).  The scheme is that of tests/gemm_exact_refs.py:

  operands     small integers times a power of two, so that every product and every partial sum, in ANY order, is a whole number of one unit below
               2^24 units: fp32 accumulation is exact and the expected output is ONE value.  What a kernel rounds to 16 bits is either representable
               (<= 8 significant bits: bf16 and fp16 run the same data) or the round-to-nearest-even of an exactly known fp32 value.
  seeds        every case runs several seeds.  "W": dense activations against weight rows that keep a few non-zeros (the rows together cover every
               k, the first and the last k in many rows); "A": sparse activations against dense weights.  A chain of contractions cannot keep EVERY
               matrix dense under the representability rule (a dense matrix turns a sparse row into a dense one), so the fused feed-forward adds
               "G" (sparse open gates against a dense W2) and "P" (a sparse feed-forward output against a dense Wpo); LayerNorm cases, whose
               normalised rows are dense by nature, run "W", "V" (a second draw) and "A" (dense W1 value rows / Wqkv).
  GEGLU gate   pre-activations are exactly 0 (gate 0) or powers of two >= 8 (sigmoid = 1 in fp32): hidden = value * gate exactly
  LayerNorm    two-level rows +-a_m (a_m a power of two): mean 0, variance a^2, xhat = +-r with r = a / sqrt(a^2 + eps) rounded to the storage type
               (asserted to sit >= 2^-20 relative from a rounding boundary; the kernel's route to r is about five fp32 roundings).  a >= 1/4: r
               rounds to exactly 1; a = 2^-7: r ~ 0.927, so eps is visible.  Constant and all-zero rows: xhat = 0.
  statistics   the GroupNorm partial sums of the outputs AS STORED, in fp64, compared bit for bit at the slot the launch implies
  guards       every output and workspace is a pitched slice of a larger NaN-filled allocation; everything outside the named region stays bit-identical

`mut` selects a deliberately wrong variant of a reference (MUTANTS): the CPU file proves that each changes an expected output of some case."""
import torch
import torch.nn.functional as F

import gemm_exact_refs as GR
import norm_refs as NR
from gemm_exact_refs import GATE_FORM_ERR, STEP, Guarded, _bits, _ints, _keep, _sentinel, gelu_erf, gelu_sigmoid5, guarded_flat, guarded_rows, limit_of
from reface_amd import ops

F64 = torch.float64
DTS = {"bf16": torch.bfloat16, "f16": torch.float16}
C, FF = 320, 1280
LN_EPS = 1e-5
EXACT_LIMIT = 2 ** 24
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}
W2_IDX = (torch.arange(FF // 16)[:, None] * 16 + torch.tensor(ops.FFN_W2_PERM)[None]).reshape(-1)


def r16(t, dt):
    """the value as stored in `dt`: round-to-nearest-even of the fp32 value (the *_assert_exact functions prove that every correct intermediate IS an
    fp32 value, so that this is one rounding; a mutant's value may be rounded twice, which does not matter)"""
    return t.float().to(dt).to(F64)


def fits32(t):
    return torch.equal(t.float().to(F64), t)


def representable(t, dt):
    return torch.equal(r16(t, dt), t)


def unit_of(*ts):
    """the largest power of two <= 1 that divides every entry of the tensors"""
    for k in range(0, 64):
        if all(t is None or torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()) for t in ts):
            return 2.0 ** -k
    raise AssertionError("not dyadic")


def assert_contraction_exact(what, A, W, *extras):
    """sum_k A[m, k] W[n, k] + extras: every product is a multiple of unit(A) unit(W), every partial sum in any order is bounded by the L1 bound
    max_mn sum_k |A| |W| + sum |extras|: fewer than 2^24 units"""
    u = min([unit_of(A) * unit_of(W)] + [unit_of(e) for e in extras if e is not None])
    l1 = (A.abs() @ W.abs().T).max().item() + sum(e.abs().max().item() for e in extras if e is not None)
    assert l1 / u < EXACT_LIMIT, f"{what}: L1 bound {l1} at unit {u}"
    return l1 / u


def boundary_margin(v, dt):
    """relative distance of every non-zero fp64 value from the nearest rounding boundary (midpoint of two neighbours) of `dt`"""
    v = v[v != 0]
    if v.numel() == 0:
        return float("inf")
    _, e = torch.frexp(v.abs())                                   # |v| = m 2^e, m in [0.5, 1)
    spacing = torch.pow(2.0, (e - SIG_BITS[dt]).to(F64))
    near = v.float().to(dt).to(F64)
    return ((spacing / 2 - (v - near).abs()) / v.abs()).min().item()


def _gen(cid, seed):
    return torch.Generator().manual_seed(7919 * (1 + "WAGPV".index(seed)) + sum(map(ord, cid)))


def _signs(g, shape):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64)


def _rows_sparse(g, shape, nnz, lo, hi):
    """rows that keep `nnz` non-zeros of +-{lo .. hi}; together they cover every k (gemm_exact_refs._keep, cover)"""
    mag = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    return _keep(g, mag * _signs(g, shape), nnz - 1, cover=True)


def _pitched(t, dt, dev, extra=16):
    """an input as a pitched slice: `extra` more columns per row behind it; the values must be representable"""
    buf = torch.zeros(t.shape[:-1] + (t.shape[-1] + extra,), dtype=dt, device=dev)
    v = buf[..., :t.shape[-1]]
    v.copy_(t.to(dt))
    assert torch.equal(v.cpu().to(F64), t), "operand not representable"
    return v


def _image(v, B, H, W_):
    """the [B H W, n] row-pitched view as [B, H, W, n] with the strides the library asks for (explicit: a dimension of size 1 would report any stride)"""
    ld = v.stride(0)
    return torch.as_strided(v, (B, H, W_, v.shape[1]), (H * W_ * ld, W_ * ld, ld, 1), v.storage_offset())


def _f32(t, dev):
    assert torch.equal(t.float().to(F64), t)
    return t.float().to(dev).contiguous()


def _w16(t, dt, dev):
    w = t.to(dt).contiguous()
    assert torch.equal(w.to(F64), t), "weight not representable"
    return w.to(dev)


def gn_blocks(stored, S, rps, cpg, coff, unrounded=None):
    """fp64 [S, rps / 128, 32, 2] (sum, sum of squares) per sample, 128-row block and consumer group of the values as stored"""
    return GR.gn_expected(stored, GR.case("blocks", [], {}, B=S, W=rps, N=stored.shape[1]), 128, stored.shape[1], cpg, coff, mut_unrounded=unrounded)


def assert_stats_exact(what, stored):
    """the in-kernel column sums run over the 32 rows of a wave in fp32 (then in fp64): exact when 32 rows of squares stay below 2^24 units"""
    u = unit_of(stored)
    M, n = stored.shape
    sq = (stored * stored).reshape(M // 32, 32, n).sum(1).max().item()
    assert sq / (u * u) < EXACT_LIMIT, f"{what}: 32-row sum of squares {sq} at unit {u * u}"


class GuardedStats:
    """GroupNorm partial sums [S, need + 2, 32, 2] fp64, NaN-filled; the launch is given slot 1 and need + 2 chunks; samples [s0, s0 + n) are written"""

    def __init__(self, S, need, dev, s0=0, n=None):
        self.buf = _sentinel((S, need + 2, 32, 2), F64, dev)
        mask = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev)
        n = S - s0 if n is None else n
        mask[s0:s0 + n, 1:1 + need] = True
        self.g = Guarded(self.buf, self.buf[s0:s0 + n, 1:1 + need], mask)
        self.ptr, self.slot, self.nchunks = self.buf[s0:].data_ptr(), 1, need + 2

    def fetch(self, what):
        self.g.check(what)
        return self.g.view.cpu()


# ================================================================================================ LayerNorm rows
A_EXPS = (-7, -6, -5, -4, -3, -2, -1, 0, 1, 2)          # a_m = 2^e: eps is visible for the small ones (r ~ 0.927 at 2^-7), r rounds to 1 from 2^-2 on


def two_level_rows(g, M, coarse=False):
    """[M, C] rows +-a_m in a row-specific balanced sign pattern; every 11th row constant, every 13th all zero.  coarse: a_m >= 1/4 only (r = 1 exactly: the
    outputs stay on a quarter-integer grid, which the statistics cases need).  Returns (x, a [M]; a = 0 marks a constant or zero row)"""
    exps = torch.tensor([e for e in A_EXPS if e >= -2] if coarse else A_EXPS)
    a = torch.pow(2.0, exps[(torch.arange(M) * 7 + torch.randint(0, len(exps), (M,), generator=g)) % len(exps)].to(F64))
    order = torch.rand((M, C), generator=g).argsort(1)
    sign = torch.where(order < C // 2, 1.0, -1.0).to(F64)
    x = sign * a[:, None]
    m = torch.arange(M)
    const = (m % 11 == 5)
    x[const] = torch.tensor([1.0, -2.0, 0.5])[m[const] % 3].to(F64)[:, None]
    zero = (m % 13 == 7)
    x[zero] = 0.0
    a = torch.where(const | zero, torch.zeros_like(a), a)
    return x, a


def layernorm64(x, eps, half=False):
    xs = x[:, :x.shape[1] // 2] if half else x
    mu = xs.mean(1, keepdim=True)
    var = ((xs - mu) ** 2).mean(1, keepdim=True)
    rstd = torch.where(var + eps > 0, 1.0 / torch.sqrt((var + eps).clamp_min(1e-300)), torch.zeros_like(var))
    return (x - mu) * rstd


def assert_two_level(what, x, dt, eps=LN_EPS):
    """the LayerNorm input is two-level (or constant): the fp32 statistics are exact, and xhat = +-r sits clear of a rounding boundary"""
    assert representable(x, dt), what
    amax, amin = x.max(1).values, x.min(1).values
    two = (amax == -amin) & (amax > 0)
    const = amax == amin
    assert bool((two | const).all()), f"{what}: a row is neither two-level nor constant"
    assert bool(((x == amax[:, None]) | (x == amin[:, None])).all()) and bool((x[two].sum(1) == 0).all()), f"{what}: not balanced"
    a = amax[two]
    r = a / torch.sqrt(a * a + eps)
    assert boundary_margin(r, dt) >= 2.0 ** -20, f"{what}: r within 2^-20 of a rounding boundary ({boundary_margin(r, dt)})"
    assert bool((r16(r.float().to(F64), dt)[a >= 0.25] == 1.0).all()), f"{what}: r does not round to 1 for a >= 1/4"
    return a


# ================================================================================================ rf_ffn_geglu / rf_ffn_block
FFN_MUTANTS = ("w2_perm_omitted", "geglu_swapped", "drop_hidden_chunk", "drop_last_k", "b1_other_stage", "ln_half_row", "ln_eps_omitted", "res2_no_modulo",
               "front_no_modulo", "ctx_neighbour", "stat_unrounded", "stat_slot_plus_1")
FFN_CONSUMERS = ((10, 0), (20, 320))          # (cpg, coff): the tensor alone; the right half of a 640-channel concat


def ffn_case(id, cells, form, M, ln, seeds, res=False, S=1, stats=0, concat=False, res2_rows=0, front_rows=0, rps0=0):
    return dict(kernel="ffn", id=id, cells=tuple(cells), form=form, M=M, ln=ln, seeds=seeds, res=res, S=S, stats=stats, concat=concat, res2_rows=res2_rows,
                front_rows=front_rows, rps0=rps0)


def _kg():
    """the input channel that opens hidden unit j in the one-hot gate rows: every channel opens four units, one per hidden quarter"""
    j = torch.arange(FF)
    return (7 * j + j // C) % C


def _act_sparse(g, M, K, P, levels):
    """rows with exactly P = 4 non-zeros, all of one row-specific level: a run of three that, over the rows, covers every k (shifted by 37 on every wrap, as
    gemm_exact_refs._keep does), and the last k (every fourth row), the first k (every fourth) or a random one"""
    assert P == 4
    e = torch.tensor(levels, dtype=F64)[torch.randint(0, len(levels), (M,), generator=g)]
    r = torch.arange(M)
    base = (3 * r + 37 * ((3 * r) // K)) % K
    end = torch.where(r % 4 == 0, torch.full_like(r, K - 1), torch.where(r % 4 == 1, torch.zeros_like(r), torch.randint(0, K, (M,), generator=g)))
    end = torch.where(((end - base) % K) < 3, (base + K // 2) % K, end)
    idx = torch.stack([base, (base + 1) % K, (base + 2) % K, end], 1)
    return torch.zeros((M, K), dtype=F64).scatter_(1, idx, 1.0) * e[:, None]


def ffn_inputs(c, seed):
    """fp64 operands of a feed-forward case in the reference layout: w1 [2 FF, C] (value rows, then gate rows), b1, w2 [C, FF], b2 and, by form, res /
    wpo, bpo, res2 / att, wo, bo, ctx, res0.  See the module docstring for the seeds."""
    g = _gen(c["id"], seed)
    M, form, ln = c["M"], c["form"], c["ln"]
    i = dict(seed=seed)
    const_gate = ln or form == "front"          # the gate_const device: gate rows of W1 zero, the gate comes from b1
    if form == "front":
        Mf = c["front_rows"] or M
        if ln:          # x1 = att Wo^T + res0 two-level: Wo a signed permutation, att and res0 each carry half of +-a_m in the same sign pattern
            x1, _ = two_level_rows(g, Mf)
            perm, s = torch.randperm(C, generator=g), _signs(g, (C,))
            i["wo"] = torch.zeros((C, C), dtype=F64)
            i["wo"][torch.arange(C), perm] = s
            i["res0"] = x1 / 2
            i["att"] = torch.zeros((Mf, C), dtype=F64)
            i["att"][:, perm] = s[None] * x1 / 2
            i["bo"], i["ctx"] = torch.zeros(C, dtype=F64), torch.zeros((M // c["rps0"], C), dtype=F64)
        else:
            if seed == "A":
                i["att"] = _act_sparse(g, Mf, C, 4, (1.0,)) * _signs(g, (Mf, 1))
                i["wo"] = _signs(g, (C, C))
            else:
                i["att"] = _ints(g, (Mf, C), -2, 2)
                i["wo"] = _rows_sparse(g, (C, C), 3, 1, 1)
            i["bo"], i["res0"] = _ints(g, (C,), -1, 1, nonzero=False), _ints(g, (Mf, C), -1, 1, nonzero=False)
            i["ctx"] = _ints(g, (M // c["rps0"], C), -1, 1, nonzero=False)
    elif ln:
        i["x"], _ = two_level_rows(g, M, coarse=bool(c["stats"]))
    elif seed in ("W", "V"):
        i["x"] = torch.randint(1, 3, (M, C), generator=g).to(F64)
    else:
        i["x"] = _act_sparse(g, M, C, 4, (1.0,) if seed in ("G", "P") else (1.0, 2.0))
    # ---- W1 / b1
    wv_dense = seed in ("A", "G", "P") and form != "front"
    wv = _signs(g, (FF, C)) if wv_dense else _rows_sparse(g, (FF, C), 3, 1, 1)
    # (dense value rows: an odd bias under the row's four +-1 terms keeps the value away from zero -- an open gate then always shows)
    bv = _signs(g, (FF,)) if wv_dense and not ln else _ints(g, (FF,), -1, 1, nonzero=False)
    wg, bg = torch.zeros((FF, C), dtype=F64), torch.zeros((FF,), dtype=F64)
    if const_gate:
        bg = torch.tensor([8.0, 16.0], dtype=F64)[torch.randint(0, 2, (FF,), generator=g)]
        if seed != "A":          # a fifth of the gates is closed, another fifth in every seed (none where the value rows are dense: every position shows)
            bg[torch.arange(FF) % 5 == "WAGPV".index(seed)] = 0.0
    elif seed == "A":
        wg[:] = 8.0
    else:
        wg[torch.arange(FF), _kg()] = torch.tensor([8.0, 16.0], dtype=F64)[torch.randint(0, 2, (FF,), generator=g)]
    i["w1"], i["b1"] = torch.cat([wv, wg], 0), torch.cat([bv, bg], 0)
    # ---- W2 / b2 (+ the plain form's residual)
    if seed == "G":
        i["w2"] = _signs(g, (C, FF)) / 8
    elif seed == "P":          # column-sparse: hidden unit j feeds output j % C alone, so that a row's few open gates leave a sparse feed-forward output
        i["w2"] = torch.zeros((C, FF), dtype=F64)
        i["w2"][torch.arange(FF) % C, torch.arange(FF)] = _signs(g, (FF,)) / 8
    else:
        i["w2"] = _rows_sparse(g, (C, FF), 6, 1, 1) / (32 if seed == "A" else 8)
    i["b2"] = torch.zeros(C, dtype=F64) if seed == "P" else _ints(g, (C,), -3, 3, nonzero=False)
    i["res"] = _ints(g, (M, C), -7, 7, nonzero=False) if (form == "geglu" and c["res"]) else None
    if form == "geglu":
        return i
    # ---- proj_out
    i["wpo"] = _signs(g, (C, C)) if seed == "P" else _rows_sparse(g, (C, C), 3, 1, 1)
    i["bpo"] = _ints(g, (C,), -3, 3, nonzero=False)
    if c["stats"]:          # a lift that carries some outputs past 8 significant bits: the statistics must be those of the STORED values
        lift = (58.0 + torch.randint(0, 9, (C,), generator=g)) if ln else 4.0 * (70 + torch.randint(0, 9, (C,), generator=g)) + 1
        i["bpo"] = torch.where(torch.arange(C) % 4 == 1, lift.to(F64) * _signs(g, (C,)), i["bpo"])
    i["res2"] = _ints(g, (c["res2_rows"] or M, C), -7, 7, nonzero=False)
    return i


def ffn_reference(c, i, dt, mut=None):
    """fp64 restatement of include/reface_hip.h's formula with the roundings the kernel documents (x1, the normalised row, the hidden value, the
    feed-forward output in front of proj_out, the output).  Returns a dict: x1 / out as stored, their exact values, the intermediate stages and
    `stats` (one [S, blocks, 32, 2] per consumer)."""
    M, form = c["M"], c["form"]
    o = dict()
    rows = torch.arange(M)
    if form == "front":
        fr = c["front_rows"] or M
        att, res0 = i["att"][rows % fr], i["res0"][rows % fr]
        if mut == "front_no_modulo":          # rows past front_rows read past the buffer: modelled as zeros
            att, res0 = att * (rows < fr)[:, None], res0 * (rows < fr)[:, None]
        ctx = torch.roll(i["ctx"], 1, 0) if mut == "ctx_neighbour" else i["ctx"]
        o["x1_exact"] = att @ i["wo"].T + i["bo"] + ctx.repeat_interleave(c["rps0"], 0) + res0
        x = o["x1"] = r16(o["x1_exact"], dt)
        resid = x
        o["att_rows"] = att
    else:
        x = i["x"]
        resid = i["res"] if form == "geglu" else x
    xh = x
    if c["ln"]:
        xh = r16(layernorm64(x, 0.0 if mut == "ln_eps_omitted" else LN_EPS, half=mut == "ln_half_row").float().to(F64), dt)
    o["xh"] = xh
    if mut == "drop_last_k":
        xh = xh.clone()
        xh[:, 63] = 0
    b1 = i["b1"]
    if mut == "b1_other_stage":          # hidden chunk c reads the bias slot of the other stage: chunk c ^ 1's values
        b1 = b1.reshape(2, FF // 64, 64)[:, torch.arange(FF // 64) ^ 1].reshape(-1)
    pre = xh @ i["w1"].T + b1
    v, gt = pre[:, :FF], pre[:, FF:]
    if mut == "geglu_swapped":
        h = gt * gelu_sigmoid5(v)
    else:
        o["gate"] = gt
        h = v * gt          # gates are 0 or >= 8: gelu_sigmoid5(g) = g exactly (asserted by ffn_assert_exact)
    o["h_exact"] = h
    h16 = r16(h.float().to(F64), dt) if mut == "geglu_swapped" else r16(h, dt)
    if mut == "drop_hidden_chunk":
        h16 = h16.clone()
        h16[:, 7 * 64:8 * 64] = 0
    o["h"] = h16
    w2 = i["w2"][:, W2_IDX] if mut == "w2_perm_omitted" else i["w2"]
    x2 = h16 @ w2.T + i["b2"] + (resid if resid is not None else 0.0)
    o["x2_exact"] = x2
    if form == "geglu":
        o["out_exact"], o["out"] = x2, r16(x2, dt)
        return o
    o["x2"] = r16(x2, dt)
    rr = c["res2_rows"] or M
    res2 = i["res2"][rows % rr]
    if mut == "res2_no_modulo":
        res2 = res2 * (rows < rr)[:, None]
    o["out_exact"] = o["x2"] @ i["wpo"].T + i["bpo"] + res2
    o["out"] = r16(o["out_exact"], dt)
    o["stats"] = []
    for cpg, coff in FFN_CONSUMERS[:c["stats"]]:
        st = gn_blocks(o["out"], c["S"], M // c["S"], cpg, coff, unrounded=o["out_exact"] if mut == "stat_unrounded" else None)
        o["stats"].append(torch.roll(st, 1, 1) if mut == "stat_slot_plus_1" else st)
    return o


def ffn_assert_exact(c, i, dt, o):
    """the issue's rules, on the data of this case, seed and type (before any launch)"""
    what = f"{c['id']}/{i['seed']}/{dt}"
    for k in ("w1", "w2", "wpo", "wo", "x", "att", "res0", "res", "res2"):
        if i.get(k) is not None:
            assert representable(i[k], dt), f"{what}: {k}"
    gate = o["gate"]
    assert bool(((gate == 0) | ((gate >= 7) & (gate == gate.round()))).all()), f"{what}: a gate pre-activation is neither 0 nor an integer >= 7"
    assert bool((gate > 0).any()) and not torch.equal(i["w1"][:FF], i["w1"][FF:]), what
    if c["form"] == "front":
        assert_contraction_exact(what + " to_out", o["att_rows"], i["wo"], i["bo"], i["ctx"], i["res0"])
        assert representable(o["x1_exact"], dt), f"{what}: x1 not representable"
    x = o["x1"] if c["form"] == "front" else i["x"]
    if c["ln"]:
        assert_two_level(what, x, dt)
    assert_contraction_exact(what + " GEMM 1", o["xh"], i["w1"], i["b1"])
    for k in ("x1_exact", "h_exact", "x2_exact", "out_exact"):
        assert k not in o or fits32(o[k]), f"{what}: {k} is not an fp32 value"
    assert_contraction_exact(what + " GEMM 2", o["h"], i["w2"], i["b2"], i["res"] if c["form"] == "geglu" else x)
    if not c["ln"]:
        assert bool((o["h_exact"].abs() <= 1024).all()) and representable(o["h_exact"], dt), f"{what}: hidden value not representable"
        assert representable(o["x2_exact"], dt), f"{what}: feed-forward output not representable"
    if c["form"] != "geglu":
        assert_contraction_exact(what + " proj_out", o["x2"], i["wpo"], i["bpo"], i["res2"])
        if not c["ln"] and not c["stats"]:
            assert representable(o["out_exact"], dt), f"{what}: output not representable"
        if c["stats"]:
            assert_stats_exact(what, o["out"])
            assert unit_of(o["out"]) >= 0.25, what


def ffn_periods(i):
    """True when no LDS stage could reproduce the right answer from stale contents: W1 K tile g differs from tile g - 4 (the ring), W2 chunk c from chunk c - 2,
    Wpo / Wo K tile kt from tile kt - 3"""
    w1p, _ = ops.pack_geglu(i["w1"], i["b1"], F64)
    t1 = w1p.reshape(FF // 64, 128, C // 64, 64).permute(0, 2, 1, 3).reshape(-1, 128, 64)          # tile g = chunk * 5 + kt
    ok = all(not torch.equal(t1[g], t1[g - 4]) for g in range(4, t1.shape[0]))
    t2 = i["w2"].reshape(C, FF // 64, 64)
    ok = ok and all(not torch.equal(t2[:, k], t2[:, k - 2]) for k in range(2, FF // 64))
    for key in ("wpo", "wo"):
        if i.get(key) is not None:
            t = i[key].reshape(C, C // 64, 64)
            ok = ok and all(not torch.equal(t[:, k], t[:, k - 3]) for k in range(3, C // 64))
    return ok


def ffn_coverage(c, i, o):
    """per matrix, a bool tensor: True where (row, k) carries a non-zero product in some output of this seed"""
    live = lambda A, W: ((A != 0).to(F64).T @ torch.ones((A.shape[0], 1), dtype=F64) > 0).reshape(1, -1) & (W != 0)
    open_ = (o["gate"] != 0).to(F64)
    xh_nz = (o["xh"] != 0).to(F64)
    cov = dict()
    # a W1 row's product shows when its hidden unit is open in that token's row (value rows: and the gate alone does not decide it)
    both = (open_.T @ xh_nz) > 0                                                         # [FF, C]: some row has unit j open and x_k != 0
    cov["w1"] = torch.cat([both & (i["w1"][:FF] != 0), both & (i["w1"][FF:] != 0)], 0)
    cov["w2"] = live(o["h"], i["w2"])
    if c["form"] != "geglu":
        cov["wpo"] = live(o["x2"], i["wpo"])
    if c["form"] == "front":
        cov["wo"] = live(o["att_rows"], i["wo"])
    return cov


def ffn_prepare(c, i, dt, dev):
    """the launch of a feed-forward case on `dev`: out / x1 / statistics guarded, inputs pitched"""
    M, form = c["M"], c["form"]
    w1p, b1p = ops.pack_geglu(i["w1"], i["b1"], dt)
    assert torch.equal(w1p.to(F64), ops.pack_geglu(i["w1"], i["b1"], F64)[0])
    w2q = ops.pack_ffn_w2(_w16(i["w2"], dt, "cpu"), dt).to(dev)
    w1p, b1p, b2 = w1p.to(dev), b1p.to(dev), _f32(i["b2"], dev)
    eps = LN_EPS if c["ln"] else 0.0
    ld, col0 = (16 + 2 * C + 16, 16 + C) if c["concat"] else (16 + C + 16, 16)
    out = guarded_rows(M, C, ld, col0, dt, dev)
    P = dict(out=out, x1=None, stats=[])
    if form == "geglu":
        x = _pitched(i["x"], dt, dev)
        res = _pitched(i["res"], dt, dev) if i["res"] is not None else None
        P["launch"] = ops.ffn_geglu(x, w1p, b1p, w2q, b2, out.view, residual=res, ln_eps=eps, name=c["id"])
        return P
    kw = dict(wpo=_w16(i["wpo"], dt, dev), bpo=_f32(i["bpo"], dev), res2=_pitched(i["res2"], dt, dev), res2_rows=c["res2_rows"], ln_eps=eps, name=c["id"])
    if form == "tail":
        x = _pitched(i["x"], dt, dev)
        l = ops.ffn_block(x, w1p, b1p, w2q, b2, out.view, residual=x, **kw)
    else:
        P["x1"] = x1 = guarded_rows(M, C, 16 + C + 16, 16, dt, dev)
        front = dict(wo=_w16(i["wo"], dt, dev), bo=_f32(i["bo"], dev), ctx=_pitched(i["ctx"], torch.float32, dev, extra=4), rows_per_sample=c["rps0"],
                     res0=_pitched(i["res0"], dt, dev), front_rows=c["front_rows"], x1=x1.view)
        l = ops.ffn_block(_pitched(i["att"], dt, dev), w1p, b1p, w2q, b2, out.view, residual=x1.view, front=front, **kw)
    d = l.keep[0]
    if c["stats"]:
        rps = M // c["S"]
        d.gn_rows = rps
        for k, (cpg, coff) in enumerate(FFN_CONSUMERS[:c["stats"]]):
            st = GuardedStats(c["S"], rps // 128, dev)
            P["stats"].append(st)
            for f, v in (("part", st.ptr), ("cpg", cpg), ("coff", coff), ("slot", st.slot), ("nchunks", st.nchunks)):
                setattr(d, f"gn_{f}{k}", v)
    P["launch"] = l
    return P


FFN_CASES = []
for _M, _cells in ((128, ["ffn_geglu one block"]), (300, ["ffn_geglu ragged M"]), (1300, ["ffn_geglu 11 blocks (uneven XCD split, 20 live rows in the last block)"])):
    for _ln in (False, True):
        for _res in (False, True):
            FFN_CASES.append(ffn_case(f"geglu-M{_M}-{'ln' if _ln else 'raw'}-{'res' if _res else 'nores'}", _cells + [
                "ffn_geglu ln_eps > 0 (two-level rows, eps visible)" if _ln else "ffn_geglu ln_eps = 0", "ffn_geglu residual" if _res else "ffn_geglu no residual",
                "GEGLU exact gate in ffn.hip", "bf16 positional rf_ffn_geglu, fp16 descriptor entry"], "geglu", _M, _ln, ("W", "V", "A") if _ln else ("W", "A", "G"), res=_res))
for _ln in (False, True):
    _s, _n = (("W", "V", "A") if _ln else ("W", "A", "G", "P")), ("ln" if _ln else "raw")
    _lc = ["ffn_block ln_eps = 1e-5"] if _ln else ["ffn_block ln_eps = 0"]
    FFN_CASES.append(ffn_case(f"tail-a-ragged-{_n}", _lc + ["ffn_block tail ragged M", "ffn_block full res2", "proj_out dense Wpo seed"], "tail", 300, _ln, _s))
    FFN_CASES.append(ffn_case(f"tail-b-stats-{_n}", _lc + ["ffn_block tail + proj_out + GroupNorm statistics", "statistics two consumers (cpg 10 coff 0, cpg 20 coff 320)",
                                                        "out as the right half of a 640-wide buffer"], "tail", 768, _ln, ("W", "V") if _ln else ("W", "A"), S=3, stats=2, concat=True))
    FFN_CASES.append(ffn_case(f"tail-c-pair-{_n}", _lc + ["ffn_block CFG pair res2_rows", "statistics one block per sample"], "tail", 512, _ln,
                              ("W", "V") if _ln else ("W", "A"), S=4, stats=1, res2_rows=256))
FFN_CASES.append(ffn_case("front-d-raw", ["ffn_block FRONT (ctx per sample, bo, res0)", "ffn_block ln_eps = 0"], "front", 512, False, ("W", "A"), S=2, rps0=256))
FFN_CASES.append(ffn_case("front-e-pair-ln", ["ffn_block FRONT pair front_rows", "ffn_block ln_eps = 1e-5", "FRONT x1 two-level"], "front", 512, True, ("W", "V"), S=4,
                          res2_rows=256, front_rows=256, rps0=128))


# ---- the gate sweep through the fused kernel (not exact: held to the documented bound of the sigmoid-form GELU)
def gate_sweep_inputs():
    """x rows one-hot at channel t = row % 4 (amplitude by row), value rows of W1 pick channel (hidden unit // 320), gate rows zero, b1's gate entries a
    sweep over [-9, 9] with +-7 and their fp32 neighbours, W2[n, j] = 1 where j % 320 == n: row type t returns hidden units 320 t .. 320 t + 319, one per
    output column -- every one of the 1280 gate evaluations is attributed"""
    M = 128
    amp = torch.tensor([1.0, -2.0, 0.5, 3.0, -1.0, 2.0, -0.5, 1.5], dtype=F64)
    x = torch.zeros((M, C), dtype=F64)
    x[torch.arange(M), torch.arange(M) % 4] = amp[(torch.arange(M) // 4) % 8]
    wv, wg = torch.zeros((FF, C), dtype=F64), torch.zeros((FF, C), dtype=F64)
    wv[torch.arange(FF), torch.arange(FF) // C] = 1.0
    seven = torch.tensor(7.0)
    special = torch.stack([s * t for s in (1.0, -1.0) for t in (seven, torch.nextafter(seven, torch.tensor(0.0)), torch.nextafter(seven, torch.tensor(9.0)))])
    gates = torch.cat([torch.linspace(-9.0, 9.0, FF - special.numel()), special, ]).float()
    gates = gates[torch.randperm(FF, generator=torch.Generator().manual_seed(5))]
    i = dict(seed="sweep", x=x, w1=torch.cat([wv, wg], 0), b1=torch.cat([torch.zeros(FF, dtype=F64), gates.to(F64)]), b2=torch.zeros(C, dtype=F64), res=None)
    i["w2"] = torch.zeros((C, FF), dtype=F64)
    i["w2"][torch.arange(FF) % C, torch.arange(FF)] = 1.0
    value = x[torch.arange(M), torch.arange(M) % 4]                                      # [M]
    gate = gates.to(F64).reshape(4, C)[torch.arange(M) % 4]                              # [M, C]: the gate behind output column n of row m
    return i, value[:, None].expand(M, C), gate


# ================================================================================================ rf_attn_in
ATTN_MUTANTS = ("wps_neighbour", "qkv_swapped", "tok_unrounded", "drop_last_k", "ln_half_row", "ln_eps_omitted", "rowvec_neighbour")


def attn_case(id, cells, S, rps, two_level):
    return dict(kernel="attn_in", id=id, cells=tuple(cells), S=S, rps=rps, M=S * rps, two_level=two_level, seeds=("W", "A"))


def attn_inputs(c, seed):
    g = _gen(c["id"], seed)
    S, M = c["S"], c["M"]
    i = dict(seed=seed)
    if c["two_level"]:
        # W'_s a signed permutation with the sign attached to the INPUT column: tok = (t_s x)[perm_s]; x rows are t_s times a pattern balanced inside each
        # sign class of t_s, so that both x and tok are two-level and balanced; a constant tok row comes from x = c t_s
        w = torch.zeros((S, C, C), dtype=F64)
        xs = []
        for s in range(S):
            perm = torch.randperm(C, generator=g)
            t = torch.where(torch.rand(C, generator=g).argsort() < C // 2, 1.0, -1.0).to(F64)
            w[s, torch.arange(C), perm] = t[perm]
            tok, a = two_level_rows(g, c["rps"])
            x = torch.zeros_like(tok)
            x[:, perm] = tok * t[perm][None]
            xs.append(x)
        i["x"], i["w"] = torch.cat(xs, 0), w
        i["rv"] = torch.zeros((S, C), dtype=F64)
        i["wqkv"] = _signs(g, (3 * C, C)) * torch.randint(1, 4, (3 * C, C), generator=g).to(F64) if seed == "A" else _rows_sparse(g, (3 * C, C), 24, 1, 3)
        i["bqkv"] = _ints(g, (3 * C,), -7, 7)
    else:
        if seed == "W":
            i["x"], i["w"] = _ints(g, (M, C), -3, 3), _rows_sparse(g, (S, C, C), 24, 1, 3)
        else:
            i["x"], i["w"] = _keep(g, _ints(g, (M, C), -3, 3), 23, cover=True), _ints(g, (S, C, C), -3, 3)
        i["rv"] = _ints(g, (S, C), -7, 7)
        # every 8th column is lifted past 8 significant bits (odd, 301 .. 331): the stored tok is then the ROUNDED value, and norm1 must read that one
        lift = (301.0 + 2 * torch.randint(0, 16, (S, C), generator=g)).to(F64) * _signs(g, (S, C))
        i["rv"] = torch.where((torch.arange(C) % 8 == 3)[None], lift, i["rv"])
        # qkv is held to a tolerance here: weights of +-{1, 2, 3} / 16 and a bias of +-(32 .. 63) keep |qkv| >= 16, so that the limit (one storage
        # half-step of |qkv|) stays above the few one-step differences a normalised value near a rounding boundary may cost (see the GPU file)
        i["wqkv"] = _ints(g, (3 * C, C), -3, 3) / 16
        i["bqkv"] = (32.0 + torch.randint(0, 32, (3 * C,), generator=g)).to(F64) * _signs(g, (3 * C,))
    return i


def attn_reference(c, i, dt, mut=None):
    S, rps = c["S"], c["rps"]
    w = torch.roll(i["w"], 1, 0) if mut == "wps_neighbour" else i["w"]
    rv = torch.roll(i["rv"], 1, 0) if mut == "rowvec_neighbour" else i["rv"]
    x = i["x"]
    if mut == "drop_last_k":
        x = x.clone()
        x[:, C - 1] = 0
    o = dict()
    o["tok_exact"] = torch.cat([x[s * rps:(s + 1) * rps] @ w[s].T + rv[s] for s in range(S)], 0)
    o["tok"] = r16(o["tok_exact"], dt)
    src = o["tok_exact"] if mut == "tok_unrounded" else o["tok"]
    o["xh_exact"] = layernorm64(src, 0.0 if mut == "ln_eps_omitted" else LN_EPS, half=mut == "ln_half_row")
    o["xh"] = r16(o["xh_exact"].float().to(F64), dt)
    wq = i["wqkv"]
    if mut == "qkv_swapped":
        wq = torch.cat([wq[C:2 * C], wq[:C], wq[2 * C:]], 0)
    o["qkv_exact"] = o["xh"] @ wq.T + i["bqkv"]
    o["qkv"] = r16(o["qkv_exact"].float().to(F64), dt) if not c["two_level"] else r16(o["qkv_exact"], dt)
    return o


def attn_assert_exact(c, i, dt, o):
    what = f"{c['id']}/{i['seed']}/{dt}"
    for k in ("x", "w", "wqkv"):
        assert representable(i[k], dt), f"{what}: {k}"
    for s in range(c["S"]):
        assert_contraction_exact(what + " proj_in", i["x"][s * c["rps"]:(s + 1) * c["rps"]], i["w"][s], i["rv"][s])
    assert fits32(o["tok_exact"]), what
    if c["two_level"]:
        assert representable(o["tok_exact"], dt) and fits32(o["qkv_exact"]), what
        assert_two_level(what, o["tok"], dt)
        assert_contraction_exact(what + " qkv", o["xh"], i["wqkv"], i["bqkv"])
    else:
        assert bool((o["tok_exact"].abs() <= 2047).all()), what
        assert dt != torch.bfloat16 or not torch.equal(o["tok"], o["tok_exact"]), f"{what}: no tok value is rounded"
        assert o["qkv_exact"].abs().min().item() >= 16.0, f"{what}: |qkv| {o['qkv_exact'].abs().min().item()}"


def attn_periods(i):
    ok = True
    for w in list(i["w"]) + list(i["wqkv"].reshape(3, C, C)):
        t = w.reshape(C, C // 64, 64)
        ok = ok and all(not torch.equal(t[:, k], t[:, k - 3]) for k in range(3, C // 64))
    return ok


def attn_prepare(c, i, dt, dev):
    M, S = c["M"], c["S"]
    tok = guarded_rows(M, C, 16 + C + 16, 16, dt, dev)
    qkv = guarded_rows(M, 3 * C, 16 + 3 * C + 16, 16, dt, dev)
    rv = _pitched(i["rv"], torch.float32, dev, extra=4)
    l = ops.attn_in(_pitched(i["x"], dt, dev), _w16(i["w"], dt, dev), rv, tok.view, _w16(i["wqkv"], dt, dev), _f32(i["bqkv"], dev), qkv.view, rows_per_sample=c["rps"],
                    ln_eps=LN_EPS, name=c["id"])
    return dict(launch=l, tok=tok, qkv=qkv)


ATTN_CASES = []
for _tl in (False, True):
    _n, _cl = ("two-level", ["attn_in two-level tok, qkv bit for bit"]) if _tl else ("general", ["attn_in general-integer tok, qkv to limit_of"])
    ATTN_CASES.append(attn_case(f"attn-3x256-{_n}", _cl + ["attn_in per-sample W' and rowvec"], 3, 256, _tl))
    ATTN_CASES.append(attn_case(f"attn-1x128-{_n}", _cl + ["attn_in w_sample_stride = 0"], 1, 128, _tl))
    ATTN_CASES.append(attn_case(f"attn-11x128-{_n}", _cl + ["attn_in 11 blocks"], 11, 128, _tl))


# ================================================================================================ rf_conv3x3_stem
STEM_MUTANTS = ("hw_swapped_border", "tap_wraps_row", "pad_channels_read", "tap_transposed", "stat_unrounded", "stat_slot_plus_1", "sample_boundary")


def stem_case(Cc, B, H, W_, dup):
    cells = [f"stem C = {Cc}", f"stem image {H}x{W_}", "stem dup" if dup else "stem no dup", "stem three statistics consumers", "stem pad channels"]
    return dict(kernel="stem", id=f"stem-C{Cc}-{B}x{H}x{W_}-{'dup' if dup else 'nodup'}", cells=tuple(cells), C=Cc, B=B, H=H, W=W_, dup=dup, seeds=("W", "A"))


def stem_consumers(c):
    """(cpg, coff, first sample, samples of the consumer's buffer): the output alone; then, with dup, both halves as the right half of a 2 C concat (the
    computed half and the duplicate are two consumer entries of the one launch); without, a 2 C and a 3 C concat"""
    Cc, B = c["C"], c["B"]
    if c["dup"]:
        return ((Cc // 32, 0, 0, B), (2 * Cc // 32, Cc, 0, 2 * B), (2 * Cc // 32, Cc, B, 2 * B))
    return ((Cc // 32, 0, 0, B), (2 * Cc // 32, Cc, 0, B), (3 * Cc // 32, 2 * Cc, 0, B))


def stem_inputs(c, seed):
    g = _gen(c["id"], seed)
    B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
    x = torch.zeros((B, H, W_, 16), dtype=F64)
    w = _ints(g, (Cc, 9, 16), -3, 3)                                  # k = tap * 16 + channel; the weights on the pad channels 9 .. 15 are NOT zero
    if seed == "W":
        x[..., :9] = _ints(g, (B, H, W_, 9), -3, 3)
        live = _keep(g, w[..., :9].reshape(Cc, 81), 23, cover=True).reshape(Cc, 9, 9)
        w = torch.cat([live, w[..., 9:]], -1)
    else:
        x[..., :9] = _keep(g, _ints(g, (B, H, W_, 9), -3, 3), 1, cover=True)
    bias = _ints(g, (Cc,), -7, 7)
    lift = (301.0 + 2 * torch.randint(0, 16, (Cc,), generator=g)).to(F64) * _signs(g, (Cc,))          # (odd, past 8 significant bits: see attn_inputs)
    bias = torch.where(torch.arange(Cc) % 8 == 3, lift, bias)
    return dict(seed=seed, x=x, w=w.reshape(Cc, 144), bias=bias)


def conv3x3_taps(x, mut=None, H=None, W_=None):
    """[B, H, W, 9, Cin] fp64: tap t = 3 dy + dx of pixel (y, x) is the input pixel (y + dy - 1, x + dx - 1), zero outside the image"""
    B, H, W_, Ci = x.shape
    if mut == "tap_wraps_row":          # only the flat pixel index is tested: a tap beyond the row's end reads the adjacent image row
        flat = F.pad(x.reshape(B, H * W_, Ci), (0, 0, W_ + 1, W_ + 1))
        taps = [flat[:, W_ + 1 + (dy - 1) * W_ + (dx - 1):][:, :H * W_].reshape(B, H, W_, Ci) for dy in range(3) for dx in range(3)]
        return torch.stack(taps, 3)
    if mut == "sample_boundary":        # the rows above / below the image are the neighbouring sample's
        flat = F.pad(x.reshape(B * H, W_, Ci), (0, 0, 1, 1, 1, 1))
        taps = [flat[dy:dy + B * H, dx:dx + W_].reshape(B, H, W_, Ci) for dy in range(3) for dx in range(3)]
        return torch.stack(taps, 3)
    p = F.pad(x, (0, 0, 1, 1, 1, 1))
    taps = []
    for dy in range(3):
        for dx in range(3):
            t = p[:, dy:dy + H, dx:dx + W_]
            if mut == "hw_swapped_border":          # the border test with H and W exchanged: (unsigned) sy < W && sx < H
                yy, xx = torch.arange(H)[:, None] + dy - 1, torch.arange(W_)[None, :] + dx - 1
                t = t * ((yy >= 0) & (yy < W_) & (xx >= 0) & (xx < H))[None, :, :, None]
            taps.append(t)
    return torch.stack(taps, 3)


def stem_reference(c, i, dt, mut=None):
    B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
    x = i["x"]
    if mut == "pad_channels_read":          # the pad channels taken as data: the next pixel's first channels, as if the pixel pitch were 9
        flat = torch.cat([x[..., :9].reshape(-1), torch.zeros(16, dtype=F64)])
        x = torch.stack([flat[9 * p:9 * p + 16] for p in range(B * H * W_)]).reshape(B, H, W_, 16)
    T = conv3x3_taps(x, mut)
    if mut == "tap_transposed":
        T = T.reshape(B, H, W_, 3, 3, 16).transpose(3, 4).reshape(B, H, W_, 9, 16)
    o = dict(A=T.reshape(B * H * W_, 144))
    o["out_exact"] = o["A"] @ i["w"].T + i["bias"]
    o["out"] = r16(o["out_exact"], dt)
    o["stats"] = []
    for cpg, coff, s0, n in stem_consumers(c):
        st = gn_blocks(o["out"], B, H * W_, cpg, coff, unrounded=o["out_exact"] if mut == "stat_unrounded" else None)
        o["stats"].append(torch.roll(st, 1, 1) if mut == "stat_slot_plus_1" else st)
    return o


def stem_assert_exact(c, i, dt, o):
    what = f"{c['id']}/{i['seed']}/{dt}"
    assert representable(i["x"], dt) and representable(i["w"], dt)
    assert bool((i["x"][..., 9:] == 0).all()) and bool((i["w"].reshape(-1, 9, 16)[..., 9:] != 0).all()), f"{what}: the padding contract is not visible"
    assert_contraction_exact(what, o["A"], i["w"], i["bias"])
    assert fits32(o["out_exact"]), what
    plain = torch.arange(c["C"]) % 8 != 3
    assert representable(o["out_exact"][:, plain], dt), f"{what}: an output of an un-lifted channel is not representable"
    assert dt != torch.bfloat16 or not torch.equal(o["out"], o["out_exact"]), f"{what}: no stored value is rounded"
    assert_stats_exact(what, o["out"])


def stem_prepare(c, i, dt, dev):
    B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
    HW = H * W_
    nb = 2 if c["dup"] else 1
    out = guarded_rows(B * HW, Cc, 16 + Cc + 16, 16, dt, dev, nb=nb)
    v4 = lambda v: _image(v, B, H, W_)
    l = ops.conv3x3_stem(_pitched(i["x"], dt, dev), _w16(i["w"], dt, dev), _f32(i["bias"], dev), v4(out.views[0]), dup=v4(out.views[1]) if c["dup"] else None, name=c["id"])
    d, stats = l.keep[0], []
    for k, (cpg, coff, s0, n) in enumerate(stem_consumers(c)):
        st = GuardedStats(n, HW // 128, dev, s0=s0, n=B)
        stats.append(st)
        for f, v in (("part", st.ptr), ("cpg", cpg), ("coff", coff), ("slot", st.slot), ("nchunks", st.nchunks)):
            setattr(d, f"gn_{f}{k}", v)
    return dict(launch=l, out=out, stats=stats)


STEM_SHAPES = ((1, 8, 16), (2, 4, 96), (3, 32, 4), (2, 128, 1))
STEM_CASES = [stem_case(Cc, B, H, W_, dup) for Cc in (64, 128, 320) for (B, H, W_) in STEM_SHAPES for dup in (False, True)]


# ================================================================================================ rf_gn_silu_conv3x3_small (the out head)
HEAD_MUTANTS = ("table_transposed", "sample_boundary", "tap_wraps_row", "hw_swapped_border", "group_of_next_channel")
SILU_LEVELS = (-4, -2, -1, 0, 1, 2, 3, 4, 8)          # integer pre-activations whose SiLU sits clear of every 16-bit rounding boundary (asserted: silu_levels_ok)
SILU_MARGIN = 2.0 ** -17                               # 8 x the 1e-6 csrc/common.h states for silu_exact


def silu_levels_ok():
    y = torch.tensor(SILU_LEVELS, dtype=F64)
    s = NR.silu64(y)
    return min(boundary_margin(s, dt) for dt in DTS.values())


def head_case(Cc, No, B, H, W_, out, silu, nchunks):
    cells = [f"out head C = {Cc}", f"out head No = {No}", f"out head image {H}x{W_}", f"out head {out} output", f"out head silu = {silu}", f"out head nchunks = {nchunks}"]
    return dict(kernel="head", id=f"head-C{Cc}-No{No}-{B}x{H}x{W_}-{out}-silu{silu}-n{nchunks}", cells=tuple(cells), C=Cc, No=No, B=B, H=H, W=W_, out=out, silu=silu,
                nchunks=nchunks, seeds=("W", "A"))


def head_affine(c, seed):
    """gamma a power of two (norm_refs.GAMMAS), beta an integer chosen per channel so that at least two SILU_LEVELS are reachable: with rstd = 1/2 the
    scale is gamma / 2 and y = (x - mean) gamma / 2 + beta, x = mean + 4 k"""
    gamma = NR.exact_affine(c["C"])[0].to(F64)
    s4 = (2 * gamma).abs()                                           # |4 scale|: y = k * (+-s4) + beta
    ch = torch.arange(c["C"])
    beta = torch.where(s4 == 8, torch.tensor(4.0, dtype=F64), ((ch * 5 + ch // 32) % 3 - 1).to(F64) * torch.where(s4 >= 4, 4.0, 1.0).to(F64))
    if seed == "A":
        beta = torch.zeros_like(beta)                                # level 0 reachable in every channel: sparse activations
    return gamma, beta


def head_inputs(c, seed):
    g = _gen(c["id"], seed)
    B, H, W_, Cc, No = c["B"], c["H"], c["W"], c["C"], c["No"]
    HW = H * W_
    gamma, beta = head_affine(c, seed)
    mean = NR.exact_means(B)                                         # [B, 32] integers
    part = NR.exact_partials(mean, HW, Cc, c["nchunks"], 40 + sum(map(ord, c["id"])) % 1000)
    mch = mean.repeat_interleave(Cc // 32, 1)                        # [B, C]
    lv = torch.tensor(SILU_LEVELS, dtype=F64)
    # per channel the reachable levels: (level - beta) a multiple of 4 scale; per pixel one of them
    ok = ((lv[None, :] - beta[:, None]) % (2 * gamma).abs()[:, None]) == 0                       # [C, levels]
    if seed == "A":
        ok = ok & ((lv != 0)[None, :])
    assert bool((ok.sum(1) >= 1).all()), c["id"]
    pick = torch.rand((B, HW, Cc, len(SILU_LEVELS)), generator=g) * ok[None, None] - (~ok)[None, None].to(F64)
    y = lv[pick.argmax(-1)]                                          # [B, HW, C]
    if seed == "A":          # sparse activations: three channels per pixel leave level 0 (covering every channel)
        rk = dict(zip(("rank", "first"), GR._interior_rank(B, H, W_))) if H > 2 and W_ > 2 else {}          # (interior pixels first: only they show all nine taps)
        y = y * (_keep(g, torch.ones((B * HW, Cc), dtype=F64), 2, cover=True, **rk).reshape(B, HW, Cc) != 0)
        w = _ints(g, (No, 9, Cc), -2, 2)
    else:
        w = _keep(g, _ints(g, (No, 9 * Cc), -3, 3), 7, cover=True).reshape(No, 9, Cc)
    scale = gamma / 2
    x = mch[:, None, :] + (y - beta) / scale
    bias = _ints(g, (No,), -7, 7)
    return dict(seed=seed, x=x.reshape(B, H, W_, Cc), y=y, gamma=gamma, beta=beta, mean=mean, part=part, w=w.reshape(No, 9 * Cc), bias=bias)


def head_reference(c, i, dt, mut=None):
    """conv3x3(round16(act(GroupNorm(x)))) + bias with the statistics the partial sums state, fp64"""
    B, H, W_, Cc, No = c["B"], c["H"], c["W"], c["C"], c["No"]
    n = float(H * W_ * (Cc // 32))
    tot = i["part"].sum(1)                                           # [B, 32, 2]
    mean = tot[..., 0] / n
    var = tot[..., 1] / n - mean * mean
    grp = torch.arange(Cc) // (Cc // 32)
    if mut == "group_of_next_channel":
        grp = (torch.arange(Cc) + 1).clamp_max(Cc - 1) // (Cc // 32)
    scale = (1.0 / torch.sqrt(var))[:, grp] * i["gamma"][None]
    shift = i["beta"][None] - mean[:, grp] * scale
    y = i["x"].reshape(B, H * W_, Cc) * scale[:, None] + shift[:, None]
    o = dict(y=y)
    act = NR.silu64(y) if c["silu"] else y
    o["act_exact"] = act
    o["act"] = act16 = r16(act.float().to(F64), dt)
    T = conv3x3_taps(act16.reshape(B, H, W_, Cc), mut if mut in ("sample_boundary", "tap_wraps_row", "hw_swapped_border") else None)
    o["A"] = T.reshape(B * H * W_, 9 * Cc)
    w = i["w"]
    if mut == "table_transposed":          # table row tap * No + o read as o * 9 + tap
        w = w.reshape(No, 9, Cc).reshape(9, No, Cc).transpose(0, 1).reshape(No, 9 * Cc)
    o["out_exact"] = o["A"] @ w.T + i["bias"]
    o["out"] = o["out_exact"] if c["out"] == "f32" else r16(o["out_exact"], dt)
    return o


def head_assert_exact(c, i, dt, o):
    what = f"{c['id']}/{i['seed']}/{dt}"
    assert representable(i["x"], dt) and representable(i["w"], dt), what
    assert torch.equal(o["y"], i["y"]), f"{what}: the pre-activations are not the chosen levels"
    lv = torch.tensor(SILU_LEVELS, dtype=F64)
    assert bool((o["y"][..., None] == lv).any(-1).all()), what
    if c["silu"]:
        assert boundary_margin(o["act_exact"], dt) >= SILU_MARGIN, what
    else:
        assert representable(o["act_exact"], dt), what
    assert_contraction_exact(what, o["A"], i["w"], i["bias"])
    assert torch.equal(o["out_exact"].float().to(F64), o["out_exact"]), what
    assert c["B"] == 1 or not torch.equal(i["x"][0], i["x"][1]), what


def head_prepare(c, i, dt, dev):
    B, H, W_, Cc, No = c["B"], c["H"], c["W"], c["C"], c["No"]
    M = B * H * W_
    odt = torch.float32 if c["out"] == "f32" else dt
    out = guarded_rows(M, No, 16 + No + 16, 16, odt, dev)
    ws = guarded_flat(M * 40, torch.float32, dev)          # exactly the size the launch is told
    part = i["part"].to(dev)
    l = ops.gn_silu_conv3x3_small(_pitched(i["x"], dt, dev), _f32(i["gamma"], dev), _f32(i["beta"], dev), part, c["nchunks"], _w16(i["w"], dt, dev), _f32(i["bias"], dev),
                                  _image(out.view, B, H, W_), eps=0.0, silu=bool(c["silu"]), workspace=ws.view, name=c["id"])
    return dict(launch=l, out=out, ws=ws)


HEAD_SHAPES = ((2, 9, 7), (1, 1, 130), (3, 16, 8), (2, 5, 1))
HEAD_CASES = []
for _k, (_Cc, _No) in enumerate((Cc, No) for Cc in (64, 128, 320) for No in (1, 3, 4)):
    for _j, (_B, _H, _W) in enumerate(HEAD_SHAPES):          # every (C, No) on every image; output type, silu and nchunks rotate so that each pairing occurs
        _v = _k + _j
        HEAD_CASES.append(head_case(_Cc, _No, _B, _H, _W, ("f32", "16")[_v % 2], (_v // 2) % 2, (1, 9)[(_v + _j // 2) % 2]))
        HEAD_CASES.append(head_case(_Cc, _No, _B, _H, _W, ("f32", "16")[(_v + 1) % 2], 1 - (_v // 2) % 2, (1, 9)[(_v + _j // 2 + 1) % 2]))

CASES = FFN_CASES + ATTN_CASES + STEM_CASES + HEAD_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
MUTANTS = dict(ffn=FFN_MUTANTS, attn_in=ATTN_MUTANTS, stem=STEM_MUTANTS, head=HEAD_MUTANTS)
INPUTS = dict(ffn=ffn_inputs, attn_in=attn_inputs, stem=stem_inputs, head=head_inputs)
REFERENCE = dict(ffn=ffn_reference, attn_in=attn_reference, stem=stem_reference, head=head_reference)
ASSERT_EXACT = dict(ffn=ffn_assert_exact, attn_in=attn_assert_exact, stem=stem_assert_exact, head=head_assert_exact)
PREPARE = dict(ffn=ffn_prepare, attn_in=attn_prepare, stem=stem_prepare, head=head_prepare)

# the mechanisms of the issue: each must be claimed by a case (test_every_cell_of_the_issue_has_a_case)
CELLS = ("ffn_geglu one block", "ffn_geglu ragged M", "ffn_geglu 11 blocks (uneven XCD split, 20 live rows in the last block)", "ffn_geglu ln_eps = 0",
         "ffn_geglu ln_eps > 0 (two-level rows, eps visible)", "ffn_geglu residual", "ffn_geglu no residual", "GEGLU exact gate in ffn.hip",
         "bf16 positional rf_ffn_geglu, fp16 descriptor entry", "ffn_block ln_eps = 0", "ffn_block ln_eps = 1e-5", "ffn_block tail ragged M", "ffn_block full res2",
         "proj_out dense Wpo seed", "ffn_block tail + proj_out + GroupNorm statistics", "statistics two consumers (cpg 10 coff 0, cpg 20 coff 320)",
         "out as the right half of a 640-wide buffer", "ffn_block CFG pair res2_rows", "statistics one block per sample", "ffn_block FRONT (ctx per sample, bo, res0)",
         "ffn_block FRONT pair front_rows", "FRONT x1 two-level", "attn_in general-integer tok, qkv to limit_of", "attn_in two-level tok, qkv bit for bit",
         "attn_in per-sample W' and rowvec", "attn_in w_sample_stride = 0", "attn_in 11 blocks", "stem dup", "stem no dup", "stem three statistics consumers",
         "stem pad channels") + tuple(f"stem C = {Cc}" for Cc in (64, 128, 320)) + tuple(f"stem image {H}x{W_}" for _, H, W_ in STEM_SHAPES) + tuple(
    f"out head C = {Cc}" for Cc in (64, 128, 320)) + tuple(f"out head No = {No}" for No in (1, 3, 4)) + tuple(f"out head image {H}x{W_}" for _, H, W_ in HEAD_SHAPES) + (
    "out head f32 output", "out head 16 output", "out head silu = 0", "out head silu = 1", "out head nchunks = 1", "out head nchunks = 9")
