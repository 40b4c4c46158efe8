"""The exact attention cases (tests/attn_exact_refs.py) checked WITHOUT a GPU: that the operands are what the exactness argument needs, that the fp64
reference is softmax attention, that the suite is not vacuous (every key of every case matters beyond 4 x the tolerance; a list of plausible kernel
slips, applied to the reference, is caught by named cases), and the launch plans: every case's plan, the boundary pairs of the dispatch, the model's
own launches and the refusal of an uninstantiated head dim -- all through the host-only rf_attention_plan."""
import math

import pytest
import torch

import attn_exact_refs as R
from reface_amd import _lib, ops

IDS = [c["id"] for c in R.CASES]


def sample_heads(c):
    """global heads checked on the CPU: the first five (one of every family when the case has that many) and the last"""
    n = c["B"] * c["heads"]
    return sorted(set(range(min(n, len(R.FAMILIES)))) | {n - 1})


# ------------------------------------------------------------------------------------------------ operands and reference
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_operands_are_exact(c):
    """representable in bf16 and fp16, integer scores within +-256, every weight >= 2^-8 or <= 2^-30 (asserted inside reference())"""
    q, k, v = R.operands(c, sample_heads(c))
    assert R.representable(q) and R.representable(k) and R.representable(v)
    assert 1 <= v.abs().min().item() and v.abs().max().item() <= 8 and bool((v == v.round()).all())
    out, A, l, p = R.reference(q, k, v, check=True)
    assert bool(torch.isfinite(out).all()) and bool((A >= out.abs() - 1e-15).all())
    if c["B"] * c["heads"] > 1:          # operands differ per (batch, head) even between heads of the same family
        n = c["B"] * c["heads"]
        a, b = R.operands(c, [0]), R.operands(c, [len(R.FAMILIES) if n > len(R.FAMILIES) else n - 1])
        assert not torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


@pytest.mark.parametrize("cid", [IDS[0], IDS[7], IDS[40], IDS[100], IDS[200], "dma80-bf16-d80-b1h7-q100-k640-r1", "x3-x3-d40-b2h3-q129-k65-r5"])
def test_reference_is_softmax_attention(cid):
    c = R.BY_ID[cid]
    q, k, v = R.operands(c, sample_heads(c))
    out = R.reference(q, k, v)[0]
    ref = torch.softmax(q @ k.transpose(-1, -2) * R.LN2, -1) @ v
    assert (out - ref).abs().max().item() < 1e-12


# ------------------------------------------------------------------------------------------------ sensitivity
def _moves(c, q, k, v):
    """per key j: does dropping it / doubling it move some output by more than 4 x the tolerance?  [Nk] bools each"""
    out, A, l, p = R.reference(q, k, v)
    lim4 = 4 * R.limit_of(c, out, A)
    Nk = k.shape[0]
    drop, dup = torch.zeros(Nk, dtype=torch.bool), torch.zeros(Nk, dtype=torch.bool)
    for j0 in range(0, Nk, 64):
        pj = p[:, j0:j0 + 64, None]
        num = (pj * (v[None, j0:j0 + 64] - out[:, None, :])).abs()
        rest = (l[:, :, None] - pj).clamp(min=0.0)
        gone = (rest <= 0) & (pj > 0)          # the row's only key: nothing is left to average
        drop[j0:j0 + 64] = ((num > lim4[:, None, :] * rest) | gone).any(0).any(-1)
        dup[j0:j0 + 64] = (num > lim4[:, None, :] * (l[:, :, None] + pj)).any(0).any(-1)
    return drop, dup


def one_pad_key_is_visible(c):
    """a single zero pad key in a flat row scales the output by Nk / (Nk + 1): a relative change of 1 / (Nk + 1), which 4 x the store rounding of a
    16-bit type (4 * STEP / 2) swallows once (Nk + 1) * 2 * STEP >= 1 -- arithmetic, not a choice.  Asked for with a factor two in hand for the
    tolerance's second term: Nk + 1 < 1 / (4 STEP), i.e. up to 30 keys in bf16 and 254 in fp16, and at every size in fp32 / x3.  The longer 16-bit
    cases show a counted pad through their frozen heads, where it takes the row over, and through the pad-to-tile mutants below."""
    return c["dt"] not in R.STEP or (c["Nk"] + 1) * 4 * R.STEP[c["dt"]] < 1


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_every_key_matters(c):
    for g in sample_heads(c):
        q, k, v = (x[0] for x in R.operands(c, [g]))
        drop, dup = _moves(c, q, k, v)
        fam = R.family_of(c, g)
        assert bool(drop.all()), f"{c['id']} head {g} ({fam}): dropping key {(~drop).nonzero()[0].item()} stays within 4 x the tolerance"
        # (one key doubled is the same softmax when it is the only key)
        assert bool(dup.all()) or c["Nk"] == 1, f"{c['id']} head {g} ({fam}): doubling key {(~dup).nonzero()[0].item()} stays within 4 x the tolerance"
        if fam in ("flat", "frozen") and (fam == "frozen" or one_pad_key_is_visible(c)):
            out, A, l, p = R.reference(q, k, v)
            w = torch.exp2(-(q @ k.T).amax(-1, keepdim=True))          # a pad key scores 0
            moved = ((out * l / (l + w) - out).abs() > 4 * R.limit_of(c, out, A)).any(-1)
            assert bool(moved.all()), f"{c['id']} head {g} ({fam}): one admitted pad key goes unnoticed in row {(~moved).nonzero()[0].item()}"


# ------------------------------------------------------------------------------------------------ mutants of the reference
def _head(c, fam):
    return next(g for g in range(c["B"] * c["heads"]) if R.family_of(c, g) == fam)


def _caught(c, g, mutate):
    """does the mutated result of head g leave the case's tolerance somewhere?  mutate(q, k, v, out) -> out'"""
    q, k, v = (x[0] for x in R.operands(c, [g]))
    out, A, l, p = R.reference(q, k, v)
    got = mutate(q, k, v, out)
    return bool((~torch.isfinite(got)).any() or ((got - out).abs() > R.limit_of(c, out, A)).any())


def _plain(q, k, v):
    return R.reference(q, k, v, check=False)[0]


def _pad_to(T):
    def f(q, k, v, out):
        n = -k.shape[0] % T
        z = torch.zeros(n, k.shape[1], dtype=R.F64)
        return _plain(q, torch.cat([k, z]), torch.cat([v, z]))
    return f


def _swap16(q, k, v, out):
    idx = torch.arange(v.shape[0])
    j = idx % 16
    src = idx - j + torch.where((j >= 4) & (j < 8), j + 4, torch.where((j >= 8) & (j < 12), j - 4, j))
    return _plain(q, k, v[src.clamp(max=v.shape[0] - 1)])


def _swap_qblocks(q, k, v, out):
    o = out.clone()
    o[0:32], o[32:64] = out[32:64], out[0:32]
    return o


def _cols_minus_32(q, k, v, out):
    o = out.clone()
    o[:, 32:] = out[:, :out.shape[1] - 32]
    return o


C_G1 = "g1-16bit-bf16-d40-b2h3-q129-k65-r4"          # generic, two 64-key tiles, 129 queries, all five families
C_DMA64 = "dma40-kt64-bf16-d40-b2h128-q511-k1216-r6"
C_DMA128 = "dma40-kt128-bf16-d40-b2h128-q300-k1152-r3"
C_DMA64_F16 = "dma40-kt64-fp16-d40-b2h128-q511-k1216-r6"
C_G2 = "g2x128-bf16-d40-b2h128-q512-k1025-r1"
C_K63 = "g2x64-bf16-d40-b2h128-q257-k63"
ALL = R.FAMILIES
# mutant -> (mutation, [(case, families that must catch it, families that cannot see it by construction)])
MUTANTS = {
    "last key dropped": (lambda q, k, v, out: _plain(q, k[:-1], v[:-1]), [(C_G1, ALL, ()), (C_DMA64, ALL, ())]),
    "last 64-key tile dropped": (lambda q, k, v, out: _plain(q, k[:-64], v[:-64]), [(C_DMA64, ("flat", "frozen", "selector", "stair_up"), ())]),
    "last 128-key tile dropped": (lambda q, k, v, out: _plain(q, k[:-128], v[:-128]), [(C_DMA128, ("flat", "frozen", "selector", "stair_up"), ())]),
    "first 64-key tile counted twice": (lambda q, k, v, out: _plain(q, torch.cat([k[:64], k]), torch.cat([v[:64], v])),
                                        [(C_G1, ("flat", "frozen", "selector", "stair_down"), ()), (C_DMA64, ("flat", "frozen", "selector", "stair_down"), ())]),
    "pad keys to the next 32 counted": (_pad_to(32), [(C_G2, ("flat", "frozen"), ()), (C_G1, ("flat", "frozen"), ())]),
    "pad keys to the next 64 counted": (_pad_to(64), [(C_K63, ("flat", "frozen"), ()), (C_G1, ("flat", "frozen"), ())]),
    "pad keys to the next 128 counted": (_pad_to(128), [(C_G2, ("flat", "frozen"), ()), (C_G1, ("flat", "frozen"), ())]),
    "keys 4..7 and 8..11 of a 16-key group swapped in V only": (_swap16, [(C_G1, ("selector",), ("flat", "frozen")), (C_DMA64, ("selector",), ("flat", "frozen"))]),
    "two adjacent 32-query blocks exchanged": (_swap_qblocks, [(C_G1, ("selector", "stair_up", "stair_down"), ("flat", "frozen")), (C_DMA64, ("selector",), ("flat", "frozen"))]),
    "head-dim columns >= 32 read from column - 32": (_cols_minus_32, [(C_G1, ALL, ()), (C_DMA128, ALL, ())]),
    "q scaled by log2 e once more": (lambda q, k, v, out: _plain(q * math.log2(math.e), k, v), [(C_G1, ("stair_up", "stair_down"), ("flat",)), (C_DMA64, ("stair_up", "stair_down"), ("flat",))]),
    "O not rescaled when the running maximum moves": (lambda q, k, v, out: R.online(q, k, v, 64, skip_o=True), [(C_G1, ("stair_up",), ("flat", "frozen")), (C_G2, ("stair_up", "selector"), ("flat", "frozen"))]),
    "denominator not rescaled": (lambda q, k, v, out: R.online(q, k, v, 64, skip_l=True), [(C_G1, ("stair_up",), ("flat", "frozen")), (C_G2, ("stair_up", "selector"), ("flat", "frozen"))]),
    "O not rescaled when the DMA reference point moves": (lambda q, k, v, out: R.online(q, k, v, 32, dma=True, skip_o=True), [(C_DMA64, ("stair_up", "selector"), ("flat", "frozen"))]),
    # 2^-100 is a bf16 value but underflows in fp16: the fp16 case is the one that sees a reference point left at 0
    "reference point never lowered from 0 on the first unit": (lambda q, k, v, out: R.online(q, k, v, 32, dma=True, never_lower=True, pdt=torch.float16),
                                                               [(C_DMA64_F16, ("frozen",), ("flat",))]),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_reference_mutant_is_caught(name):
    mutate, where = MUTANTS[name]
    for cid, must, blind in where:
        c = R.BY_ID[cid]
        for fam in must:
            assert _caught(c, _head(c, fam), mutate), f"'{name}' passes the {fam} head of {cid}"
        for fam in blind:          # (recorded so that nobody counts on these heads for this slip)
            assert not _caught(c, _head(c, fam), mutate), f"'{name}' is visible in the {fam} head of {cid} after all: update the table"


def test_neighbouring_head_or_batch_is_caught():
    """head h reads V of head h + 1; batch b reads K of batch 0"""
    for cid in (C_G1, C_DMA64, "dma80-bf16-d80-b2h4-q257-k384-r2"):
        c = R.BY_ID[cid]
        for g in range(min(c["B"] * c["heads"] - 1, 5)):
            q, k, v = (x[0] for x in R.operands(c, [g]))
            v1 = R.operands(c, [g + 1])[2][0]
            assert _caught(c, g, lambda q, k, v, out: _plain(q, k, v1)), (cid, g)
    for cid in (C_DMA64, "dma80-bf16-d80-b2h4-q257-k384-r2", "g1-16bit-bf16-d8-b3h3-q33-k9-r2"):
        c = R.BY_ID[cid]
        seen = set()
        for g in range(c["heads"], min(c["B"] * c["heads"], c["heads"] + 5)):
            k0 = R.operands(c, [g % c["heads"]])[1][0]
            if _caught(c, g, lambda q, k, v, out: _plain(q, k0, v)):
                seen.add(R.family_of(c, g))
        assert "selector" in seen, (cid, seen)          # (flat rows have Q = 0 and cannot see K at all)


def test_online_emulation_is_the_reference():
    """the tile walkers the mutants are built on reproduce the reference when nothing is broken"""
    for cid, kw in ((C_G1, dict(T=64)), (C_DMA64, dict(T=32, dma=True)), (C_G2, dict(T=64))):
        c = R.BY_ID[cid]
        for fam in R.FAMILIES:
            assert not _caught(c, _head(c, fam), lambda q, k, v, out: R.online(q, k, v, **kw)), (cid, fam)


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_case_plan(c):
    lost = R.plan_matches(R.plan_of(c, ops), c["expect"])
    assert not lost, f"the cell {c['cell']} lost its case {c['id']}: {lost}"


def test_every_cell_has_a_case():
    missing = [cell for cell in R.REQUIRED_CELLS if not R.CELLS.get(cell)]
    assert not missing, missing
    fam_of = {"g1": "generic", "g2": "generic", "g8": "generic", "dm": "dma", "x3": "x3"}
    rem = {}
    for c in R.CASES:
        rem.setdefault(fam_of[c["cell"][:2]], set()).add(c["expect"]["grid_mod8"])
        n = c["B"] * c["heads"]
        assert n >= len(R.FAMILIES) or n == 1, c["id"]          # flat and frozen (and the rest) run in every launch ...
    for cell in R.REQUIRED_CELLS:                                 # ... and the single-head launches rotate through all of them
        fams = {R.family_of(c, g) for c in map(R.BY_ID.get, R.CELLS[cell]) for g in range(c["B"] * c["heads"])}
        assert fams == set(R.FAMILIES), (cell, fams)
        assert any(c["layout"] == "cross" for c in map(R.BY_ID.get, R.CELLS[cell])) or "single-stage" in cell, cell
    for fam, r in rem.items():
        assert 0 in r and r & {1, 3, 7}, (fam, r)          # both branches of the XCD block remap
    assert {1, 3, 7} <= rem["generic"] | rem["x3"] | rem["dma"]
    seen_q = {c["Nq"] for c in R.CASES if c["cell"].startswith("g1")}
    seen_k = {c["Nk"] for c in R.CASES if c["cell"].startswith("g1")}
    assert {1, 31, 33, 127, 129} <= seen_q and {1, 7, 9, 31, 33, 63, 64, 65, 127, 129, 200} <= seen_k


BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def _pl(dt, BH, d, Nq, Nk, x3=False):
    pl = ops.attention_plan_of(dt, 1, BH, d, Nq, Nk, x3=x3)
    return pl["family"], pl["qb"], pl["keys"], pl["waves"], pl["stages"]


@pytest.mark.parametrize("dt", [BF, HF])
def test_dispatch_boundaries(dt):
    g1, g2, g2k, g8 = ("generic", 1, 64, 4, 2), ("generic", 2, 64, 4, 2), ("generic", 2, 128, 4, 2), ("generic", 1, 128, 8, 2)
    d128, d64 = ("dma", 2, 128, 4, 3), ("dma", 2, 64, 4, 7)
    # 511 | 512 blocks of 256 queries at d = 40
    assert _pl(dt, 511, 40, 256, 1024) == g1 and _pl(dt, 512, 40, 256, 1024) == d128
    assert _pl(dt, 256, 40, 256, 1024) == g1 and _pl(dt, 256, 40, 257, 1024) == d128
    # Nk 1023 | 1024 | 1088 | 1089
    assert [_pl(dt, 512, 40, 256, nk) for nk in (960, 1023, 1024, 1088, 1089, 1152)] == [g2, g2, d128, d64, g2k, d128]
    assert [_pl(dt, 512, 32, 256, nk) for nk in (1023, 1024)] == [g2, g2k]          # no DMA kernel below d = 40
    # d = 80: Nk 383 | 384 | 512 | 513, 255 | 256 blocks
    assert [_pl(dt, 256, 80, 256, nk) for nk in (256, 383, 384, 511, 512, 513, 640)] == [g1, g1, d128, g1, d128, g8, d128]
    assert [_pl(dt, bh, 80, 256, 513) for bh in (255, 256)] == [g1, g8]
    assert _pl(dt, 1, 80, 1, 384) == d128          # (the DMA kernel takes any grid)
    # fp32 and x3 have one plan each, whatever the sizes
    assert _pl(F32, 512, 40, 512, 1024) == g1 and _pl(F32, 512, 40, 512, 1024, x3=True) == ("x3", 1, 64, 4, 2)
    assert _pl(F32, 512, 160, 512, 1024) == ("generic", 1, 64, 4, 1) and _pl(F32, 1, 160, 1, 1, x3=True) == ("x3", 1, 64, 4, 1)


def test_model_launch_plans():
    """the UNet's self-attention launches (CFG batch 16 x 8 heads at 64x64 / 32x32 / 16x16 / 8x8 latents) and the CLIP towers, as dispatched today"""
    for dt in (BF, HF):
        assert ops.attention_plan_of(dt, 16, 8, 40, 4096, 4096) == dict(family="dma", storage=ops.code(dt), d=40, qb=2, keys=128, waves=4, stages=3, ones=1, qpb=256,
                                                                        grid=2048, lds=71168, grid_mod8=0)
        assert ops.attention_plan_of(dt, 16, 8, 80, 1024, 1024) == dict(family="dma", storage=ops.code(dt), d=80, qb=2, keys=128, waves=4, stages=3, ones=1, qpb=256,
                                                                        grid=512, lds=142208, grid_mod8=0)
        for N, grid in ((256, 256), (64, 128)):
            assert ops.attention_plan_of(dt, 16, 8, 160, N, N) == dict(family="generic", storage=ops.code(dt), d=160, qb=1, keys=64, waves=4, stages=2, ones=0, qpb=128,
                                                                       grid=grid, lds=89088, grid_mod8=0)
    # ViT-L/14 of the ID / CLIP encoder (257 tokens, 16 heads of 64) and ViT-B/32 of the FID tower (50 tokens, 12 heads of 64, batches of 50)
    for dt in (BF, HF, F32):
        for B, heads, N in ((1, 16, 257), (50, 12, 50)):
            pl = ops.attention_plan_of(dt, B, heads, 64, N, N)
            assert (pl["family"], pl["qb"], pl["keys"], pl["waves"], pl["stages"], pl["ones"], pl["grid"]) == ("generic", 1, 64, 4, 2, 0, B * heads * -(-N // 128))
    assert ops.attention_plan_of(F32, 16, 8, 40, 4096, 4096, x3=True)["family"] == "x3"


def test_unsupported_head_dim_is_refused():
    with pytest.raises(_lib.RefaceHipError, match="head dim 24 not instantiated"):
        ops.attention_plan_of(BF, 1, 2, 24, 64, 64)
    with pytest.raises(_lib.RefaceHipError, match="alignment"):
        ops.attention_plan_of(BF, 1, 2, 20, 64, 64)
    with pytest.raises(_lib.RefaceHipError, match="bad arguments"):
        ops.attention_plan_of(BF, 1, 2, 40, 0, 64)


def test_plan_wrapper_and_asserts():
    """ops.attention_plan reads the sizes off the tensors (host tensors: nothing is launched) and carries the shape asserts of ops.attention"""
    q = torch.zeros(2, 33, 3 * 80, dtype=BF)
    out = torch.zeros(2, 33, 80, dtype=BF)
    pl = ops.attention_plan(q[..., :80], q[..., 80:160], q[..., 160:], out, heads=2)
    assert pl == ops.attention_plan_of(BF, 2, 2, 40, 33, 33)
    with pytest.raises(AssertionError):
        ops.attention_plan(q[..., :80], q[..., 80:160], q[:, :20, 160:], out, heads=2)          # k.shape != v.shape
    with pytest.raises(AssertionError):
        ops.attention_plan(q[..., :80], q[..., 80:160], q[..., 160:], out, heads=3)             # C % heads
    with pytest.raises(AssertionError):
        ops.attention_plan(q[..., 0:160:2], q[..., 80:160], q[..., 160:], out, heads=2)         # stride(-1) != 1
    with pytest.raises(AssertionError):
        ops.attention_plan(q[..., :80], q[..., 80:160], q[..., 160:], out[:, :32], heads=2)     # out.shape != q.shape
    with pytest.raises(AssertionError):
        ops.attention_plan(q[0, :, :80], q[0, :, 80:160], q[0, :, 160:], out[0], heads=2)       # three-dimensional views


def test_exports():
    lib = _lib.load()
    assert lib.rf_version() >= 105 and "rf_attention_plan" in _lib.EXPORTS and hasattr(lib, "rf_attention_plan")
