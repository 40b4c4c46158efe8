"""Exactly checkable inputs for rf_attention: operand generators, the fp64 reference, the derived tolerance, guarded buffers and the case table
shared by test_attn_exact_cpu.py (no GPU) and test_attn_exact_gpu.py.

Every case calls with scale = ln 2 (the kernels then skip the extra rounding of q * scale * log2 e: q . k IS the exp2-domain score) on small-integer
operands: every operand is representable in bf16 and fp16, every score is an integer with |s| <= 256, and every softmax weight relative to the
row's final maximum is a power of two that is either >= 2^-8 ("live") or <= 2^-30 ("dead").  exp2 of a live term is a power of two that the
16-bit pack of P cannot change, and the fp32 sums of P V and of the denominator are exact: what remains of the kernel's arithmetic is the
reciprocal, one multiply and the store rounding, which is what the tolerance (limit_of) allows -- nothing in it is fitted to a kernel.

FAMILIES.  One launch carries all of them: the (batch, head) with global index g = b * heads + h runs FAMILIES[(g + rot) % 5], and every generator
folds g into its index hashes, so a kernel that reads the neighbouring head or batch reads another family altogether.
  flat        Q = 0: every score is 0, the output is the mean of V over exactly Nk keys (K holds noise that must not matter).
  frozen      every real score is -100 (q[0] = -10, k[0] = 10): a zero-padded key (score 0) would take the row over.
  selector    keys carry the +-1 code of their class (j + 5 g) mod 2^b in the first b head-dim slots, query i carries 16 x the code of its target
              class: 16 b for the class, at most 16 b - 32 for every other key.  The targets run over all classes, high classes (whose first
              member sits in a late tile) on the early queries.  b is capped so that every class has >= 3 members and every class is targeted.
  stair_up    scores are rank-1, q[0] * level(j): levels rise by 3 per 32 keys twice, then jump by 30 to the next group (so the weights below the
  stair_down  final maximum are 1, 2^-3, 2^-6 and then <= 2^-30), from -219 up to +219 -- or fall the same way.  The generic kernels move their
              running maximum in every pass; the DMA kernels' reference point moves only when a score exceeds it by 8 (every third unit), and the
              first unit has to lower it from 0 to -219 (2^219 overflows: the clamp of the first move).  Every fourth query and the last one
              have q[0] = 0 (a flat row; the pattern shifts with every 32-query block), so that no key is dead for all queries.
V is the same construction for all: keys j and j + d of an even / odd rank pair are exact negatives (+-6 in one column that moves with the pair,
+-2 / +-3 elsewhere) plus a sparse 0 / 1 pattern, so column sums stay small (a single key is a large part of them: a dropped or doubled key
moves an output far beyond the tolerance) but not zero (a wrong denominator shows).  Values lie in [-6, 7] and are never 0: the softmax-weighted
|v| of the tolerance's second term is >= 1 in every element, which is what lets it cover the dead keys' mass (at most 96 keys at 2^-30 and a few
dozen at 2^-32, times 7: below 2^-20) and fp16's absolute spacing below 2^-14 where live terms cancel.
Head-dim slots a family does not use hold noise on ONE side (odd slots in K, even slots in Q) and zero on the other: the scores do not change,
a kernel that pairs the wrong k-steps does.

A case that carries `only` = "tail", "tiny" or "vsub" (tests/f16_range_cases.py) runs that range family in every head instead of the rotation; its weights
lie in the band the families above exclude, so its tests call reference(check=False) and assert the family's own conditions.  No case of the table
below names one."""
import math

import torch

F64 = torch.float64
LN2 = 0.6931471805599453
FAMILIES = ("flat", "frozen", "selector", "stair_up", "stair_down")
STEP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}          # spacing of the 16-bit storage types relative to the binade: STEP / 2 |ref| is one store rounding
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "x3": torch.float32}
LIVE, DEAD = 2.0 ** -8, 2.0 ** -30
_M31 = 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------ operands
def _hash(x):
    h = (x * 40503 + 977) & _M31
    h = h ^ (h >> 11)
    h = (h * 20011 + 3) & _M31
    h = h ^ (h >> 7)
    h = (h * 30011) & _M31
    return h ^ (h >> 13)


def _tri(x):
    return (_hash(x) % 3) - 1


def _pm23(x):
    h = _hash(x)
    return (2 + h % 2) * (1 - 2 * ((h >> 1) % 2))


def selector_bits(c):
    """b: the code width of the selector family -- at most min(d, 12) slots, every class targeted by some query (2^b <= Nq) and >= 3 keys per class"""
    b = min(c["d"], 12)
    while b > 0 and ((1 << b) > c["Nq"] or 3 * (1 << b) > c["Nk"]):
        b -= 1
    return b


def family_of(c, g):
    return FAMILIES[(g + c["rot"]) % len(FAMILIES)]


def operands(c, gs, device="cpu"):
    """q [G, Nq, d], k [G, Nk, d], v [G, Nk, d] (fp64, integer valued) of the global heads gs (a list of b * heads + h)"""
    d, Nq, Nk = c["d"], c["Nq"], c["Nk"]
    I = lambda n, shape: torch.arange(n, device=device, dtype=torch.int64).view(shape)
    g = torch.as_tensor(list(gs), device=device, dtype=torch.int64).view(-1, 1, 1)
    i, j, t = I(Nq, (1, -1, 1)), I(Nk, (1, -1, 1)), I(d, (1, 1, -1))
    # ---- V
    r = j // d
    sign = 1 - 2 * (r % 2)
    big = 6 * ((j % d + 3 * g + 5 * (r // 2)) % d == t)
    small = _pm23(((g * 131 + r // 2) * 4099 + j % d) * 211 + t)
    v = sign * torch.where(big != 0, big, small) + ((j + t + g) % 8 == 0)
    # ---- one-sided noise of the unused slots
    kj = _tri((g * 257 + j) * 173 + t + 7)
    qj = _tri((g * 263 + i) * 179 + t + 11)
    kn, qn = kj * (t % 2 == 1), qj * (t % 2 == 0)
    fam = (g + c["rot"]) % len(FAMILIES)
    zq = torch.zeros((g.shape[0], Nq, d), device=device, dtype=torch.int64)
    # flat
    q, k = zq, kj + 0 * g
    # frozen
    s0 = (t == 0)
    q = torch.where(fam == 1, torch.where(s0, -10, qn), q)
    k = torch.where(fam == 1, torch.where(s0, 10, kn), k)
    # selector
    b = selector_bits(c)
    nb = 1 << b
    code = lambda cls: 2 * ((cls >> torch.clamp(t, max=20)) & 1) - 1
    kcls = (j + 5 * g) % nb
    qcls = (nb - 1 - (i + (i // 32 if nb <= 32 else 0)) % nb + g) % nb          # (shifted per 32-query block: adjacent blocks are never alike)
    q = torch.where(fam == 2, torch.where(t < b, 16 * code(qcls), qn), q)
    k = torch.where(fam == 2, torch.where(t < b, code(kcls), kn), k)
    # staircases
    u = j // 32
    lev = -219 + 3 * (u % 3) + 36 * (u // 3) + (g % 5)
    a = (((i + g + i // 32) % 4 != 3) & (i != Nq - 1)).to(torch.int64)
    for f, sg in ((3, 1), (4, -1)):
        q = torch.where(fam == f, torch.where(s0, a, qn), q)
        k = torch.where(fam == f, torch.where(s0, sg * lev, kn), k)
    only = c.get("only")          # the range families (tests/f16_range_cases.py): a case that names one runs it in every head; no rotation
    if only == "tail":
        # one key jmax(g) at the row maximum (score 0, inside the key range: tail keys before and after it), every other key at score -(e + f (i % 2)),
        # e in [9, 22], f = j % 3: weights 2^-9 .. 2^-24, seven keys in eight at e >= 15 (fp16 subnormals as a packed P), in every key tile.  V: +-(200 .. 255)
        # with ONE sign per (column, head) on the tail keys -- they add up, nothing cancels --, -1 / 0 / 1 on the maximum's key
        h = _hash(g * 8191 + j)
        e = torch.where((h % 8 == 0) & (j != Nk - 1), 9 + (h >> 3) % 6, 15 + (h >> 3) % 8)          # (the last key: a last tile of one key has its subnormal too)
        jmax = Nk // 3 + (5 * g) % max(1, Nk // 3)
        top = j == jmax
        s1 = (t == 1)
        q = torch.where(s0, 1, torch.where(s1, i % 2, qn)) + 0 * g
        k = torch.where(top, 0 * kn, torch.where(s0, -e, torch.where(s1, -(j % 3), kn)))
        v = torch.where(top, _tri((g * 37 + 11) * 173 + t), (1 - 2 * ((t + g) % 2)) * (200 + _hash((g * 4099 + j) * 211 + t) % 56))
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    if only == "tiny":
        # Q is an fp16 subnormal +-m 2^-24 (m in 1 .. 3, the sign alternates per query) against K = 1 or 2 in slot 0, noise against zeros elsewhere: every
        # score is a multiple of 2^-24 below 2^-21, the row maximum lies in (0, 2^-14) on the even queries and in (-2^-14, 0) on the odd ones.  Every
        # weight is within 2^-21 of 1: the 16-bit pack of P rounds it to 1, 2^-21 A from the fp64 weights -- inside the unchanged limit_of.
        # What this family pins is that subnormal Q operands and reference points below 2^-14 (the two low branches of ceil16<f16_t>, used by the dma
        # kernels alone) are REACHED and give finite, correct output.  It cannot tell a wrong low branch from the right one: any reference point
        # within 2^-14 of the true one gives the same weights to 2^-14, far inside limit_of
        q = torch.where(s0, (1 - 2 * (i % 2)) * (1 + (i // 2 + g) % 3) * 2.0 ** -24, qn.to(F64))
        k = torch.where(s0, (1 + _hash(g * 8191 + j) % 2).to(F64), kn.to(F64))
    if only == "vsub":
        # V in S-in against live weights: the selector family's scores (the keys of the query's target class at weight 1, every other key at <= 2^-32)
        # with a V that depends on the key's CLASS alone: +-m 2^-24, m in 1 .. 255, an fp16 subnormal (2^-14 m, a normal value, in every fourth
        # column).  The output is the class's own V row: the mean of n equal rows, n v / n, 2^-22 relative from v after the fp32 reciprocal and the
        # dead keys' mass -- and v is ON the 16-bit grid, so the store rounds back to v itself: compared bit for bit
        assert b >= 1
        q, k = torch.where(t < b, 16 * code(qcls), qn).to(F64) + 0.0 * g, torch.where(t < b, code(kcls), kn).to(F64)
        hv = _hash((g * 4099 + kcls) * 211 + t)
        v = ((1 - 2 * ((hv >> 9) % 2)) * (1 + hv % 255)).to(F64) * torch.where(t % 4 == 3, 2.0 ** -14, 2.0 ** -24)
    return q, k, v


def representable(x):
    """every value survives a round trip through bf16 AND fp16"""
    return bool((x.to(torch.bfloat16).to(F64) == x).all() and (x.to(torch.float16).to(F64) == x).all())


# ------------------------------------------------------------------------------------------------ reference and tolerance
def reference(q, k, v, check=True):
    """plain fp64 softmax attention in the exp2 domain (scale = ln 2) of [..., Nq, d] x [..., Nk, d]: (out, A = sum_j p_j |v_jc| / l, l, P) with P relative
    to the row maximum.  check: the operand conditions -- integer scores within +-256, every weight live or dead."""
    s = q @ k.transpose(-1, -2)
    if check:
        assert bool((s == s.round()).all()) and s.abs().max().item() <= 256, "scores must be integers within +-256"
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    if check:
        assert bool(((p >= LIVE) | (p <= DEAD)).all()), "a softmax weight between 2^-30 and 2^-8"
    l = p.sum(-1, keepdim=True)
    return (p @ v) / l, (p @ v.abs()) / l, l, p


def limit_of(c, ref, A):
    """16-bit storage: one store rounding of the result, STEP / 2 * |ref|; on top 2^-18 A (fp32 and x3: 2^-16 A alone) for the fp32 reciprocal and
    multiply, the ISA's 1-ulp exp2 on the fp32 paths accumulated over <= 4096 terms, and the dead keys' mass (<= N 2^-30)"""
    if c["dt"] in STEP:
        return STEP[c["dt"]] / 2 * ref.abs() + 2.0 ** -18 * A
    return 2.0 ** -16 * A


# ------------------------------------------------------------------------------------------------ guarded device buffers
PAD = 8          # NaN columns between / around the operands (16-byte alignment for both element sizes)


def buffers(c, device):
    """Device tensors of one case inside NaN-filled allocations: (q, k, v, out views [B, N, C], dict of the whole allocations, the fp64 operands
    [B * heads, N, d]).  fused: one
    [B, R, 3 (C + PAD)] buffer, NaN pad columns after each of q, k and v, NaN rows beyond Nq (q) / Nk (k, v).  cross: three buffers with three
    different row pitches.  out: columns PAD .. PAD + C of a [B, Nq + 3, C + 2 PAD] NaN buffer."""
    B, heads, d, Nq, Nk = c["B"], c["heads"], c["d"], c["Nq"], c["Nk"]
    C_, dt = heads * d, TORCH_DT[c["dt"]]
    q, k, v = operands(c, range(B * heads), device)
    pack = lambda x, n: x.view(B, heads, n, d).permute(0, 2, 1, 3).reshape(B, n, C_).to(dt)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dt, device=device)
    if c["layout"] == "fused":
        big = nan(B, max(Nq, Nk) + 3, 3 * (C_ + PAD))
        qv, kv, vv = (big[:, :n, o * (C_ + PAD):o * (C_ + PAD) + C_] for o, n in ((0, Nq), (1, Nk), (2, Nk)))
        alloc = {"qkv": big}
    else:
        bq, bk, bv = nan(B, Nq + 2, C_ + PAD), nan(B, Nk + 5, C_ + 3 * PAD), nan(B, Nk + 1, 2 * C_ + 2 * PAD)
        qv, kv, vv = bq[:, :Nq, :C_], bk[:, :Nk, 2 * PAD:2 * PAD + C_], bv[:, :Nk, C_ + PAD:2 * C_ + PAD]
        alloc = {"q": bq, "k": bk, "v": bv}
    qv.copy_(pack(q, Nq))
    kv.copy_(pack(k, Nk))
    vv.copy_(pack(v, Nk))
    ob = nan(B, Nq + 3, C_ + 2 * PAD)
    alloc["out"] = ob
    return qv, kv, vv, ob[:, :Nq, PAD:PAD + C_], alloc, (q, k, v)


def bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------ mutants of the reference (CPU file)
def online(q, k, v, T, *, dma=False, pdt=None, skip_o=False, skip_l=False, never_lower=False):
    """Online softmax over T-key tiles in fp64, the way the kernels walk the keys.  generic: the running maximum follows every tile.  dma: the
    reference point starts at 0, is set from the first unit (never_lower: only raised) and afterwards raised only when a score exceeds it by 8.
    pdt: P passes through that storage type (underflow to zero included).  skip_o / skip_l: O / the denominator is not rescaled when the
    reference moves."""
    Nq, Nk = q.shape[0], k.shape[0]
    m = torch.zeros(Nq, 1, dtype=F64) if dma else torch.full((Nq, 1), -math.inf, dtype=F64)
    o, l = torch.zeros(Nq, v.shape[1], dtype=F64), torch.zeros(Nq, 1, dtype=F64)
    for t0 in range(0, Nk, T):
        s = q @ k[t0:t0 + T].T
        mx = s.amax(-1, keepdim=True)
        if dma:
            first = t0 == 0 and not never_lower
            m_new = torch.where((mx - m > 8) | first, mx if first else torch.maximum(mx, m), m)
        else:
            m_new = torch.maximum(m, mx)
        alpha = torch.exp2(torch.clamp(m - m_new, max=0.0))
        p = torch.exp2(s - m_new)
        if pdt is not None:
            p = p.to(pdt).to(F64)
        o = (o if skip_o else o * alpha) + p @ v[t0:t0 + T]
        l = (l if skip_l else l * alpha) + p.sum(-1, keepdim=True)
        m = m_new
    return o / l


# ------------------------------------------------------------------------------------------------ the case table
G1 = dict(family="generic", qb=1, keys=64, waves=4, qpb=128)
G2_64 = dict(family="generic", qb=2, keys=64, waves=4, qpb=256, stages=2)
G2_128 = dict(family="generic", qb=2, keys=128, waves=4, qpb=256, stages=2)
G8 = dict(family="generic", qb=1, keys=128, waves=8, qpb=256, stages=2)
DMA128 = dict(family="dma", qb=2, keys=128, waves=4, qpb=256, stages=3, ones=1)
DMA64 = dict(family="dma", qb=2, keys=64, waves=4, qpb=256, stages=7, ones=1)
X3 = dict(family="x3", qb=1, keys=64, waves=4, qpb=128)
# cell name -> what it is (the issue's table); every cell must be claimed by a case (test_every_cell_has_a_case)
CELLS = {}
CASES = []


def _add(cell, plan, dt, B, heads, d, Nq, Nk, *, layout="fused", rot=0, **more):
    exp = dict(plan, d=d, **more)
    if plan["family"] != "dma":
        exp.setdefault("ones", int(d % 32 != 0))
    exp.setdefault("stages", 2)
    exp["grid"] = -(-Nq // plan["qpb"]) * B * heads
    exp["grid_mod8"] = exp["grid"] % 8
    cid = f"{cell}-{dt}-d{d}-b{B}h{heads}-q{Nq}-k{Nk}" + ("" if layout == "fused" else "-cross") + (f"-r{rot}" if rot else "")
    CELLS.setdefault(cell, []).append(cid)
    CASES.append(dict(id=cid, cell=cell, dt=dt, B=B, heads=heads, d=d, Nq=Nq, Nk=Nk, layout=layout, rot=rot, expect=exp))


H16 = ("bf16", "fp16")
_BH = [(1, 5), (1, 7), (3, 3), (2, 4), (1, 11), (2, 3)]          # grids 5, 7, 9, 8, 11, 6 (x 2 at Nq = 129): remainders 1, 3, 7 and 0 among them
_NQ, _NK = (1, 31, 33, 127, 129), (1, 7, 9, 31, 33, 63, 64, 65, 127, 129, 200)
n = 0
for d_ in (8, 16, 32, 40, 64, 80, 160):          # generic, one query block per wave, 64-key stages, 4 waves: both denominator forms, all three types,
    for dt_ in ("bf16", "fp16", "f32"):          # EVERY key-count edge for every (d, type); the query-count edges and the grids rotate through them
        for nk_ in _NK:
            (B_, h_), nq_ = _BH[n % 6], _NQ[n % 5]
            one = dt_ == "f32" and d_ == 160          # the only single-stage LDS plan of the typed kernel
            _add("g1-f32-d160-single-stage" if one else f"g1-{'f32' if dt_ == 'f32' else '16bit'}", G1, dt_, B_, h_, d_, nq_, nk_, rot=n, stages=1 if one else 2)
            n += 1
for dt_ in H16:
    # two query blocks per wave, 64-key stages: >= 512 blocks of 256 queries and Nk < 1024
    for n, (d_, nq_, nk_) in enumerate([(40, 257, 63), (40, 300, 65), (40, 512, 960), (40, 512, 1023), (16, 257, 1023), (16, 300, 960), (16, 512, 65), (16, 512, 63)]):
        _add("g2x64", G2_64, dt_, 2, 128, d_, nq_, nk_, rot=n)
    # ... 128-key stages: 1025 = one key in the first pass of the last stage (the second pass is empty: the kvs >= Nk break), 1064 = 40 keys there,
    # 1151 = a full first pass and 63 of 64 keys in the second (partly masked)
    for n, (d_, nq_, nk_) in enumerate([(40, 512, 1025), (40, 300, 1056 + 8), (40, 257, 1151), (32, 300, 1024)]):
        _add("g2x128", G2_128, dt_, 2, 128, d_, nq_, nk_, rot=n + 1)
    _add("g2x128", G2_128, dt_, 4, 64, 40, 300, 1151, layout="cross", rot=2)
    _add("g2x64", G2_64, dt_, 4, 64, 40, 300, 65, layout="cross", rot=3)
    # the in-wave pipelined LDS-DMA kernel, d = 40: grid exactly 512, ragged last 256-query block and last wave
    for n, (nq_, nk_) in enumerate([(257, 1024), (300, 1152), (511, 1024), (300, 1088), (511, 1216), (257, 1088)]):
        _add("dma40-kt128" if nk_ % 128 == 0 else "dma40-kt64", DMA128 if nk_ % 128 == 0 else DMA64, dt_, 2, 128, 40, nq_, nk_, rot=n + 2)
    _add("dma40-kt64", DMA64, dt_, 4, 64, 40, 300, 1216, layout="cross", rot=1)
    _add("dma40-kt128", DMA128, dt_, 4, 64, 40, 300, 1152, layout="cross", rot=4)
    # ... d = 80: any grid; 384 keys = the shortest ring (3 tiles)
    for rot_ in range(5):
        _add("dma80", DMA128, dt_, 1, 1, 80, 1, 384, rot=rot_)
    for n, (B_, h_, nq_, nk_) in enumerate([(1, 5, 257, 512), (1, 7, 100, 640), (2, 4, 257, 384), (1, 11, 300, 512)]):
        _add("dma80", DMA128, dt_, B_, h_, 80, nq_, nk_, rot=n)
    _add("dma80", DMA128, dt_, 1, 7, 80, 257, 640, layout="cross", rot=3)
    # 8 waves per block, 128-key stages, d = 80: Nk >= 512 that is no multiple of 128, >= 256 blocks
    for n, (nq_, nk_) in enumerate([(257, 513), (300, 576), (257, 1000)]):
        _add("g8", G8, dt_, 2, 64, 80, nq_, nk_, rot=n + 3)
    _add("g8", G8, dt_, 4, 32, 80, 300, 1000, layout="cross", rot=4)
    _add("g1-16bit", G1, dt_, 2, 3, 64, 31, 200, layout="cross", rot=1)
    _add("g1-16bit", G1, dt_, 2, 3, 40, 129, 65, rot=4)          # (named by the CPU file's mutants: two key tiles, two query blocks, all families)
_add("g1-f32", G1, "f32", 1, 5, 40, 129, 65, layout="cross", rot=2)
n = 0
for d_ in (8, 40, 64, 80, 160):          # split-bf16 pairs on fp32 tensors; d = 160 is its single-stage plan
    for nq_, nk_ in ((127, 63), (129, 65), (33, 129), (129, 200)):
        B_, h_ = _BH[n % 6]
        _add("x3-d160-single-stage" if d_ == 160 else "x3", X3, "x3", B_, h_, d_, nq_, nk_, rot=n, stages=1 if d_ == 160 else 2)
        n += 1
_add("x3", X3, "x3", 1, 7, 40, 127, 129, layout="cross", rot=3)
del n, d_, dt_, B_, h_, nq_, nk_, rot_, one

REQUIRED_CELLS = ("g1-16bit", "g1-f32", "g1-f32-d160-single-stage", "g2x64", "g2x128", "dma40-kt128", "dma40-kt64", "dma80", "g8", "x3", "x3-d160-single-stage")
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def plan_of(c, ops):
    return ops.attention_plan_of(TORCH_DT[c["dt"]], c["B"], c["heads"], c["d"], c["Nq"], c["Nk"], x3=c["dt"] == "x3")


def plan_matches(pl, expect):
    """the words of `expect` that the reported plan does not carry"""
    return {k: (pl.get(k), v) for k, v in expect.items() if pl.get(k) != v}
