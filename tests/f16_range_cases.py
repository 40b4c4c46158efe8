"""Range cases of the fp16 precision mode: the kernels that have an fp16 instantiation, at the edges of fp16's range.  Shared by
tests/test_f16_range_cpu.py (generator assertions, references against torch fp64, mutants) and tests/test_f16_range_gpu.py (launches).

The exact suites run every case in bf16 AND fp16 on the same data, so their generators stay where both formats agree.  These cases sit on the
same harnesses (gemm_exact_refs, attn_exact_refs, side_refs) with the range knobs set, and enter the region where fp16 differs.  Value classes,
all derived from the format (10 mantissa bits, emin = -14, largest finite 65504), none fitted:
  S-in   an operand is an fp16 subnormal m 2^-24, 1 <= m <= 1023 (m <= 255 where the bf16 control runs); the other side is scaled so that products
         and sums stay integers times ONE unit, below 2^24 units: fp32 accumulation is exact whatever the order
  S-out  the exactly known fp32 result lies in the fp16 store band: 2^-24 (the smallest subnormal), 2^-25 (tie -> 0), 3 2^-25 (tie -> 2^-23),
         2^-25 (1 + 2^-10) (-> 2^-24), 1023 2^-24 (the largest subnormal), 2^-14 (the smallest normal), both signs, and a sum that cancels to zero
  TOP    the same store path at 65504, between 65504 and 65520 (-> 65504), at 65520 (tie -> +inf) and at -65520 (-> -inf)
The expected value stays ONE value: exp = ref.float().to(torch.float16) on the CPU of the exactly known fp32 result, compared bit for bit
(attention: the harness's derived limit_of, unchanged).  Where a case's data is exactly representable in bf16 too, the same case runs in bf16 as a
control: a failure in fp16 alone then points at the format edge, not at the case.

rf_conv_gemm: an output is alpha acc + bias[n] + ..., linear in the fp32 bias.  steer() sets bias[n] so that ONE row of column n -- a different row
for every column -- lands exactly on the column's target value; the other rows of the column lie a few hundred units around it, on both sides:
off-grid values next to every tie.  The unit of the S-out cases is 2^-35 (subnormal A times 2^-11 W), 2^11 units per fp16 subnormal step.

rf_attention: the "tail" family of attn_exact_refs -- one key at the row maximum, every other key at a weight 2^-e, e in [9, 24], all exact in fp16,
those with e >= 15 subnormal as a packed P operand -- and the "tiny" family, whose scores are subnormal-Q products below 2^-14 in magnitude.
The "vsub" family puts V in S-in against live weights: the keys of one class at weight 1, V a function of the class alone, so that the output IS
a V row, a subnormal on the 16-bit grid, compared bit for bit.  The tiny family pins reachability and finiteness of the low branches of ceil16<f16_t>
only (attn_exact_refs says why).  Out of scope: the clamp at +-65504 of the scaled logits (beyond 45 000) and NaN input (-fno-honor-nans).

norm.hip: subnormal inputs into rf_groupnorm_stats / _finalize (fp64 partial sums bit-equal) and rf_layernorm; rf_groupnorm_apply with host-written
partials and rf_layernorm with gamma / beta steered so that outputs land on every S-out and TOP value; rf_groupnorm_fold_linear's folded weights in
S-out, its row vector summed over the weights as stored.  The layout and pack kernels get side_refs' fp32 edge patterns.

rf_conv3x3_stem: tokres_exact_refs' stem inputs with x and the taps scaled (S-in), the bias steered into S-out and TOP.

rf_ffn_geglu: tokres_exact_refs' raw feed-forward inputs scaled per matrix (FFN_KINDS): S-in on x, W1 and W2, b2 steered into S-out and TOP, and the
hidden value -- the one fp16 store inside a kernel that no output comparison elsewhere sees -- placed in the S-out band, so that the second GEMM's
A operand is a subnormal produced inside the kernel.

rf_ffn_block (plain, LayerNorm-fused, to_out in front), rf_attn_in and rf_gn_silu_conv3x3_small: the same way (BLOCK_KINDS, ATTN_IN_KINDS, HEAD_KINDS) --
S-in on Wpo, Wo, W', Wqkv and the conv taps, every 16-bit store inside the kernels (x1, the feed-forward output in front of proj_out, tok, the GroupNorm
result) placed in the subnormal band, S-out and TOP outputs through the fp32 bias of the last contraction."""
import numpy as np
import torch

import attn_exact_refs as AR
import gemm_exact_refs as R
import norm_refs as NR
import side_refs as SR
import tokres_exact_refs as T
from reface_amd import ops

F64, F16, BF16 = torch.float64, torch.float16, torch.bfloat16
SUB = 2.0 ** -24            # the fp16 subnormal step
NORMAL_MIN = 2.0 ** -14     # the smallest fp16 normal
F16_MAX = 65504.0

# ------------------------------------------------------------------------------------------------ value classes
S_OUT = {"2^-24": 2.0 ** -24, "2^-25 tie->0": 2.0 ** -25, "3*2^-25 tie->2^-23": 3 * 2.0 ** -25, "2^-25(1+2^-10)": 2.0 ** -25 * (1 + 2.0 ** -10),
         "1023*2^-24": 1023 * 2.0 ** -24, "2^-14": 2.0 ** -14, "cancels to 0": 0.0}
TOP = {"65504": 65504.0, "65512 (-> 65504)": 65512.0, "65520 tie->+inf": 65520.0}
# what Tensor.to(float16) makes of each class value (restated from the format, asserted against torch in the CPU file)
S_OUT_STORED = {"2^-24": 2.0 ** -24, "2^-25 tie->0": 0.0, "3*2^-25 tie->2^-23": 2.0 ** -23, "2^-25(1+2^-10)": 2.0 ** -24, "1023*2^-24": 1023 * 2.0 ** -24,
                "2^-14": 2.0 ** -14, "cancels to 0": 0.0}
TOP_STORED = {"65504": 65504.0, "65512 (-> 65504)": 65504.0, "65520 tie->+inf": float("inf")}


def targets_of(cls):
    """the per-column target values of a class, both signs: column n gets targets[n % len]"""
    vals = {"S-out": S_OUT, "TOP": TOP}[cls]
    return torch.tensor([s * v for v in vals.values() for s in (1.0, -1.0)], dtype=F64)


def is_sub16(t):
    """True where a value is a non-zero fp16 subnormal: a multiple of 2^-24 below 2^-14"""
    a = t.abs()
    return (a > 0) & (a < NORMAL_MIN) & (a / SUB == (a / SUB).round())


def store16(ref, dt=F16):
    """THE expected value: Tensor.to(dt) on the CPU of the exactly known fp32 result"""
    return ref.float().to(dt)


# ------------------------------------------------------------------------------------------------ store / operand mutants (CPU file)
def flush_sub(t):
    """16-bit subnormal operands (or results) flushed to zero, sign kept"""
    return torch.where(t.abs() < NORMAL_MIN, torch.copysign(torch.zeros_like(t), t), t)


def store16_trunc(ref):
    """store by truncation (round toward zero) instead of nearest-even: nothing below 2^16 rounds up to inf"""
    v = ref.double().numpy()
    a = np.abs(v)
    _, e = np.frexp(np.where(a > 0, a, 1.0))
    q = np.exp2(np.maximum(e - 1, -14).astype(np.float64) - 10)
    t = np.floor(a / q) * q
    t = np.where(a >= 65536.0, np.inf, np.minimum(t, 65504.0))
    return torch.from_numpy(np.copysign(t, v)).to(F16)


def store16_saturate(ref):
    """saturation to +-65504 instead of +-inf"""
    s = store16(ref)
    return torch.where(torch.isinf(s), torch.copysign(torch.full_like(s, F16_MAX), s), s)


def store16_flush(ref):
    """subnormal results flushed at the store"""
    return flush_sub(store16(ref))


def bits_differ(a, b):
    return not torch.equal(R._bits(a), R._bits(b))


# ------------------------------------------------------------------------------------------------ rf_conv_gemm
GEMM_CASES = []
P3, MB = R.P3, R.MB
_t = R._t
# the data paths into the MFMA (smallest shapes of gemm_exact_refs at which the plan reports the loop) ...
LOOPS = {
    "linear direct-to-LDS": (_t(128, 128, 4, glds=1, conv=0, splitk=1), dict(W=200, C0=64, N=100)),
    "conv direct-to-LDS korder 0": (_t(128, 128, 4, glds=1, conv=1, hx=0, splitk=1), dict(B=2, H=9, W=9, C0=64, N=100, ks=3, pad=P3, rowvec=True)),
    "conv direct-to-LDS korder 1": (_t(128, 128, 4, glds=1, conv=1, hx=0, splitk=1), dict(B=3, H=9, W=9, C0=128, N=112, ks=3, pad=P3, korder=1)),
    # (korder 2 is built for 16-bit outputs: dense operands all the same, the expected value is the store rounding of the exact fp32 sum)
    "row-extended korder 2": (_t(128, 128, 4, hx=1, splitk=1), dict(B=3, H=8, W=16, C0=128, N=112, ks=3, pad=P3, korder=2, out="16", sparse="none")),
    "through registers: C1 concat": (_t(128, 128, 4, glds=0, conv=1, splitk=1), dict(B=2, H=9, W=9, C0=40, C1=24, N=100, ks=3, pad=P3)),
    "through registers: Cin = 16": (_t(128, 64, 4, glds=0, conv=1, splitk=1), dict(B=2, H=9, W=9, C0=16, N=40, ks=3, pad=P3)),
    "ups 2": (_t(128, 128, 4, glds=1, conv=1, splitk=1), dict(B=3, H=16, W=8, C0=64, N=112, ups=2, ks=3, pad=P3)),
    "per-sample W": (_t(128, 128, 4, glds=1, conv=0, splitk=1), dict(B=3, W=128, C0=64, N=112, wps=True, rowvec=True)),
    "batch > 1": (_t(128, 128, 4, conv=0, splitk=1), dict(W=100, C0=64, N=100, batch=3)),
}
# ... and the store paths
STORES = {
    "direct epilogue": (_t(128, 160, 4, direct=1, splitk=1), dict(W=200, N=144)),
    "staged epilogue": (_t(128, 160, 4, direct=0, splitk=1), dict(W=200, N=152, rowvec=True)),
    "split-K fragment slabs + reduce": (_t(128, 160, 4, reduce="frag"), dict(B=1, H=8, W=8, C0=256, N=304, ks=3, pad=P3, ws=4 * MB)),
    "split-K stripe reduce": (_t(128, 128, 4, reduce="stripe8"), dict(B=4, H=8, W=8, C0=128, N=112, ks=3, pad=P3, ws=MB, rowvec=True)),
    "two-kernel N split tail": (_t(256, 256, 8, gemm_kernels=2, tail=(128, 256, 8, 1), split_n=4096), dict(B=4, W=1024, N=5632, rowvec=True, small=dict(W=64, N=384))),
}
GN_CELL = "fused GroupNorm statistics of stored subnormals"
# every cell a case must claim (test_every_cell_has_a_case): (path, class)
GEMM_CELLS = tuple((f"loop {k}", cl) for k in LOOPS for cl in ("S-in A", "S-in W")) + tuple(
    (f"store {k}", cl) for k in STORES for cl in ("S-out", "TOP", "S-in both, fp32 out")) + (
    ("store staged epilogue", "S-in epilogue vectors"), (GN_CELL, "S-out"))


def _g(id, cells, expect, classes, steer=None, control=True, **kw):
    c = R.case(id, [f"{p} | {cl}" for p, cl in cells], expect, op="f16", range16=True, **kw)
    c.update(range_cells=tuple(cells), classes=tuple(classes), steer=steer, control=control)
    GEMM_CASES.append(c)


def _slug(s):
    return "".join(ch if ch.isalnum() else "-" for ch in s).strip("-").replace("--", "-")


for _k, (_e, _kw) in LOOPS.items():
    # fp32 output, dense operands: every k of the contraction carries a subnormal operand in every row
    _g(f"loop-{_slug(_k)}-sinA", [(f"loop {_k}", "S-in A")], _e, ["S-in A"], a_exp=-24, e_exp=-24, a_hi=255, **_kw)
    if _k != "ups 2":          # (ups 2's phase weights are sums of +-1 taps: the W side of that loop is scaled, its integers stay)
        _g(f"loop-{_slug(_k)}-sinW", [(f"loop {_k}", "S-in W")], _e, ["S-in W"], w_exp=-24, e_exp=-24, w_hi=255, **_kw)
    else:
        _g(f"loop-{_slug(_k)}-sinW", [(f"loop {_k}", "S-in W")], _e, ["S-in W"], w_exp=-24, e_exp=-24, **_kw)
for _k, (_e, _kw) in STORES.items():
    _res = dict(res=True) if _k in ("direct epilogue", "two-kernel N split tail") else {}
    # S-out: subnormal A (m <= 255) times W 2^-11: unit 2^-35.  The residual, where there is one, is a 16-bit tensor of subnormals (e_exp = -24)
    _g(f"store-{_slug(_k)}-sout", [(f"store {_k}", "S-out")], _e, ["S-in A", "S-out"], steer="S-out", out="16", a_exp=-24, w_exp=-11, e_exp=-24, a_hi=255,
       **_kw, **_res)
    _g(f"store-{_slug(_k)}-top", [(f"store {_k}", "TOP")], _e, ["TOP"], steer="TOP", out="16", **_kw, **_res)
    # both operands subnormal, m up to 1023 on the A side (no bf16 control: bf16 holds 8 bits); fp32 output in units of 2^-48
    _g(f"store-{_slug(_k)}-sin-f32", [(f"store {_k}", "S-in both, fp32 out")], _e, ["S-in A", "S-in W"], control=False, a_exp=-24, w_exp=-24, e_exp=-48, a_hi=1023,
       **_kw, **_res)
# the residual (16-bit, subnormal), bias and row vector at 2^-24 against products of 2^-24: outputs are exact subnormals and small normals
_g("store-staged-epilogue-sinE", [("store staged epilogue", "S-in epilogue vectors")], STORES["staged epilogue"][0], ["S-in A", "S-in E"], out="16", a_exp=-24, e_exp=-24,
   res=True, **STORES["staged epilogue"][1])
# fused GroupNorm statistics: alpha = 1/4, products of 2^-27, bias +-(58 .. 66) 2^-27: stored values up to 13 subnormal steps, most of them rounded
_g("gn-staged-sout", [(GN_CELL, "S-out")], _t(128, 128, 4, direct=0, splitk=1), ["S-in A", "S-out stats"], control=False, out="16", gn=True, alpha=0.25, rowvec=True,
   B=3, H=8, W=16, N=96, a_exp=-24, w_exp=-3, e_exp=-27)
GEMM_BY_ID = {c["id"]: c for c in GEMM_CASES}
assert len(GEMM_BY_ID) == len(GEMM_CASES)


def steer(c, i, ref):
    """set bias[n] so that row r(n) = (7 n + 3) mod rows of column n is exactly targets[n % T] (rows counted over all launches of a batch); returns
    the new reference.  ACT_NONE only: the output is linear in the bias."""
    if not c["steer"]:
        return ref
    assert c["act"] == ops.ACT_NONE and i["bias"] is not None
    tg = targets_of(c["steer"])
    nb, M, N = ref.shape
    n = torch.arange(N)
    flat = ref.reshape(nb * M, N)
    i["bias"] = i["bias"] + (tg[n % tg.numel()] - flat[(7 * n + 3) % (nb * M), n])
    new = R.reference(c, i)
    assert torch.equal(new.reshape(nb * M, N)[(7 * n + 3) % (nb * M), n], tg[n % tg.numel()]), c["id"]
    return new


def gemm_prepared(c):
    """(inputs, fp64 reference) of a gemm range case, steered"""
    i = R.make_inputs(c)
    return i, steer(c, i, R.reference(c, i))


def gemm_control(c):
    """the bf16 control of a case (the same data: asserted representable by the harness's own round-trip checks), or None"""
    return dict(c, op="bf16", id=c["id"]) if c["control"] else None


def gemm_operands(c, i):
    """(A side tensors, W side tensors, epilogue tensors) that are not None"""
    nn = lambda *ks: [i[k] for k in ks if i.get(k) is not None]
    return nn("x0", "x1", "xt"), nn("w", "w3"), nn("bias", "rowvec", "res")


def gemm_mutant_ref(c, i, side):
    """the reference on operands whose fp16 subnormals of one side ('A', 'W', 'E': the 16-bit residual) are flushed to zero"""
    j = dict(i)
    for k in {"A": ("x0", "x1", "xt"), "W": ("w", "w3"), "E": ("res",)}[side]:
        if j.get(k) is not None:
            j[k] = flush_sub(j[k])
    return R.reference(c, j)


# ------------------------------------------------------------------------------------------------ rf_attention
def _attn(cell, plan, d, B, heads, Nq, Nk, family, dt="fp16", **more):
    exp = dict(plan, d=d, **more)
    if plan["family"] != "dma":
        exp.setdefault("ones", int(d % 32 != 0))
    exp.setdefault("stages", 2)
    exp["grid"] = -(-Nq // plan["qpb"]) * B * heads
    return dict(id=f"{family}-{cell}-{dt}", cell=cell, dt=dt, B=B, heads=heads, d=d, Nq=Nq, Nk=Nk, layout="fused", rot=0, expect=exp, only=family)


# every plan family at its smallest listed shape: d / B x heads / Nq x Nk
ATTN_SHAPES = (("g1", AR.G1, 64, 2, 3, 31, 200), ("g2x64", AR.G2_64, 40, 2, 128, 257, 63), ("g2x128", AR.G2_128, 40, 2, 128, 300, 1064),
               ("dma40-kt128", AR.DMA128, 40, 2, 128, 257, 1024), ("dma40-kt64", AR.DMA64, 40, 2, 128, 257, 1088), ("dma80", AR.DMA128, 80, 1, 5, 257, 512),
               ("g8", AR.G8, 80, 2, 64, 257, 513))
ATTN_CASES = [_attn(*s, family=f, dt=dt) for s in ATTN_SHAPES for f, dts in (("tail", ("fp16", "bf16")), ("tiny", ("fp16",)), ("vsub", ("fp16", "bf16"))) for dt in dts]
ATTN_CHECK_HEADS = 6          # heads whose every element the CPU file checks for the tail condition (the GPU file checks all of them)


def attn_tail_split(c, q, k, v):
    """(contribution of the e >= 15 keys to every output element, limit_of of that element) of tail-family heads"""
    ref, A, l, p = AR.reference(q, k, v, check=False)
    sub = torch.where(p < NORMAL_MIN, p, torch.zeros_like(p))
    return ((sub @ v) / l).abs(), AR.limit_of(c, ref, A), p


# ------------------------------------------------------------------------------------------------ norm.hip
# (B, HW, C, nchunks, extra pitch in vectors): the smallest shapes of norm_refs.STATS_SHAPES with more than one chunk, a ragged pixel count, one chunk
NORM_STATS_SHAPES = [(3, 2, 32, 7, 1), (3, 33, 320, 32, 2), (3, 81, 32, 1, 1)]
# (B, HW, C, nchunks, xpad, opad): a one-slot and a two-slot launch of the apply pass (norm_refs.apply_exact_cases)
NORM_APPLY_SHAPES = [dict(B=3, HW=33, C=320, nchunks=9, xpad=16, opad=24), dict(B=2, HW=3, C=NR.c_for_ns(F16, 2), nchunks=1, xpad=8, opad=8)]
NORM_LN_SHAPES = [(3, 32), (3, 520), (5, 1544)]          # (M, C): one, two and the 6-vector form of rf_layernorm (norm_refs.ln_nv)
NORM_FOLD_SHAPES = [(32, 320, 1), (512, 7, 9)]           # (C, N, nchunks) of norm_refs.FOLD_CASES
NORM_PAIRS = [(F16, F16), (BF16, BF16)]                  # the case and its bf16 control (all data is exact in bf16: |k| <= 64)


def norm_stats_input(B, HW, C, seed):
    """S-in: x = k 2^-24, |k| <= 16 (norm_refs.stats_exact_input's quarter-integers times 2^-22): sums are multiples of 2^-24, sums of squares of 2^-48,
    the same integer counts as there -- far below 2^24 units (stats_exact_bound) and far above fp32's own underflow"""
    return NR.stats_exact_input(B, HW, C, seed) * 4 * SUB


def _steered(base, cls, offset=0):
    """beta[c] = target[c] - base[pixel p(c), c], p(c) = (7 c + 3) mod pixels: one pixel of every channel lands on the channel's target value
    (offset: where in the class's table channel 0 starts -- a kernel with four output channels walks the table over several cases)"""
    M, C_ = base.shape
    c = torch.arange(C_)
    tg = targets_of(cls)
    return tg[(c + offset) % tg.numel()] - base[(7 * c + 3) % M, c]


def norm_apply_case(cls, s, seed):
    """host-written partials (integer means, var = 4, eps = 0: rstd = 1/2), x = k / 4 with |k| <= 64, gamma = +-2^-32 (S-out: x sc is k 2^-35) or +-8
    (TOP: x sc is k), beta steered: y = (x - mean) sc + beta is a multiple of the unit below 2^24 units in every fp32 evaluation order the kernel
    may use (x sc, mean sc, beta - mean sc and the sums are all such multiples).  -> dict x, mean, var, partial, gamma, beta (fp32), y [B HW, C] fp64"""
    B, HW, C_ = s["B"], s["HW"], s["C"]
    unit, sc0 = (2.0 ** -35, 2.0 ** -33) if cls == "S-out" else (1.0, 4.0)
    x = NR.apply_exact_input(B, HW, C_, seed)
    mean, var = NR.exact_means(B), torch.full((B, 32), 4.0, dtype=F64)
    c = torch.arange(C_)
    sc = sc0 * (1.0 - 2.0 * ((c // 3) % 2)).to(F64)
    g = NR.group_index(C_)
    msc = mean[:, g][:, None, :] * sc
    base = (x * sc - msc).reshape(B * HW, C_)
    beta = _steered(base, cls)
    y = base + beta
    for t in (x * sc, msc, beta - msc, y):
        assert bool((t / unit == (t / unit).round()).all()) and t.abs().max().item() / unit < 2 ** 24
    assert torch.equal(beta.float().to(F64), beta)
    return dict(x=x, mean=mean, var=var, partial=NR.exact_partials(mean, HW, C_, s["nchunks"], seed), gamma=(2 * sc).float(), beta=beta.float(), y=y)


def norm_ln_case(cls, M, C_, seed):
    """S-in rows (m_row +- 2) 2^-24: mean = m 2^-24, var = 4 2^-48, eps = 0, (x - mean) rstd = +-1 exactly; y = +-gamma + beta with beta = (c % 3) steps
    and gamma = target - beta: the + entries of channel c land on its target, the - entries on -target + 2 beta"""
    x, m, s = NR.ln_exact_input(M, C_, seed)
    c = torch.arange(C_)
    tg = targets_of(cls)
    beta = (c % 3).to(F64) * (SUB if cls == "S-out" else 8.0)
    gamma = tg[c % tg.numel()] - beta
    assert torch.equal(gamma.float().to(F64), gamma)
    return dict(x=x * SUB, gamma=gamma.float(), beta=beta.float(), y=s * gamma + beta)


FOLD_GAMMAS = (2.0 ** -22, -2.0 ** -22 * (1 + 2.0 ** -10), 1023 * 2.0 ** -21, -2.0 ** -11, 2.0 ** -21)


def norm_fold_case(C_, N, nch, seed):
    """S-out for the folded weights: W = k / 4 (|k| <= 32), rstd = 1/2, gamma from FOLD_GAMMAS: W' = k gamma / 8 -- k 2^-25 (ties at every odd k),
    k 2^-25 (1 + 2^-10), k 1023 2^-24, k 2^-14, k 2^-24.  beta = 0 and no bias: the row vector is -sum_k W'_stored mean, multiples of 2^-24 below
    2^24 of them, so it stays exact in fp32 and shows whether the sum ran over the values as STORED.  (TOP is left to the other kernels: a W' of
    +-inf makes the row vector inf - inf.)"""
    W, _ = NR.fold_exact_weights(N, C_, seed)
    c = torch.arange(C_)
    gamma = torch.tensor(FOLD_GAMMAS, dtype=F64)[(c * 3 + c // 8) % len(FOLD_GAMMAS)].float()
    mean, var = NR.exact_means(NR.FOLD_B), torch.full((NR.FOLD_B, 32), 4.0, dtype=F64)
    return dict(W=W, gamma=gamma, beta=torch.zeros(C_), mean=mean, var=var, partial=NR.exact_partials(mean, 16, C_, nch, seed))


# ------------------------------------------------------------------------------------------------ rf_conv3x3_stem (tokres_exact_refs' stem cases)
STEM_SHAPES = ((64, 1, 8, 16, False), (128, 2, 4, 96, True))          # (C, B, H, W, dup): one 128-row block; six blocks, two samples, the duplicated half
STEM_KINDS = {"S-in x, S-out": ("S-out", -24, -11), "S-in taps": (None, 0, -24), "TOP": ("TOP", 0, 0)}          # kind -> (steered class, x exponent, w exponent)
STEM_CASES = [(kind, shape) for kind in STEM_KINDS for shape in STEM_SHAPES]


def stem_range_inputs(kind, shape):
    """tokres_exact_refs.stem_inputs (seed "W": dense pixels, the pad channels' weights non-zero) with x and the taps scaled by powers of two.  A
    steered class replaces the bias: row (7 n + 3) mod rows of channel n lands on the channel's target, the others within 216 units (2^-35 or 1) of it.
    "S-in taps": the bias is scaled with the products, every output a multiple of 2^-24.  -> (case, inputs, reference dict of stem_reference)"""
    cls, xe, we = STEM_KINDS[kind]
    c = T.stem_case(*shape)
    i = T.stem_inputs(c, "W")
    i["x"], i["w"] = i["x"] * 2.0 ** xe, i["w"] * 2.0 ** we
    if cls is None:
        i["bias"] = i["bias"] * 2.0 ** (xe + we)
    else:
        i["bias"] = torch.zeros_like(i["bias"])
        i["bias"] = _steered(T.stem_reference(c, i, F16)["out_exact"], cls)
    o = T.stem_reference(c, i, F16)
    T.assert_contraction_exact(f"{c['id']} {kind}", o["A"], i["w"], i["bias"])
    assert T.fits32(o["out_exact"]) and T.fits32(i["bias"])
    return c, i, o


def stem_prepare(c, i, dt, dev):
    """tokres_exact_refs.stem_prepare without the statistics consumers (rf_conv3x3_stem emits none when no buffer is named: the 32-row fp32 sums of
    squares of a column of 1024-step values would not be exact; statistics of stored subnormals are the gemm case's): the guarded, pitched output alone"""
    B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
    out = T.guarded_rows(B * H * W_, Cc, 16 + Cc + 16, 16, dt, dev, nb=2 if c["dup"] else 1)
    v4 = lambda v: T._image(v, B, H, W_)
    l = ops.conv3x3_stem(T._pitched(i["x"], dt, dev), T._w16(i["w"], dt, dev), T._f32(i["bias"], dev), v4(out.views[0]), dup=v4(out.views[1]) if c["dup"] else None,
                         name=c["id"])
    return l, out


# ------------------------------------------------------------------------------------------------ rf_ffn_geglu (tokres_exact_refs' feed-forward cases)
# kind -> exponents of x, the W1 value rows, their bias, W2, (b2, residual); const: the gate comes from b1 alone (gate rows of W1 zero, as tokres_exact_refs
# does for its LayerNorm cases: a subnormal x cannot open a gate of 8 through fp16 weights); steer: b2 is steered onto the class; res: with a residual
FFN_KINDS = {
    # x = m 2^-24 against value rows of +-2^-5: v = k 2^-29, hidden = v * gate (8 or 16) = k 2^-26 or k 2^-25, at most 3.5 subnormal steps -- the value the
    # kernel re-rounds to fp16 between its GEMMs lies in the S-out band, ties included, and the second GEMM's A operand is a subnormal made in the kernel.
    # W2 = +-2^10 lifts it to multiples of 2^-14 in the output, where a wrong hidden rounding is a whole output step
    "S-in x, hidden S-out": dict(x=-24, wv=-5, bv=-29, w2=13, e2=-14, const=True, steer=None, res=True),
    "S-in W1": dict(x=0, wv=-24, bv=-24, w2=13, e2=-14, const=True, steer=None, res=True),          # hidden = k 2^-24 gate: exact subnormals, up to 112 steps
    "S-in W2, S-out": dict(x=-14, wv=0, bv=-14, w2=-21, e2=0, const=True, steer="S-out", res=False),    # hidden k 2^-11 against W2 = +-2^-24: unit 2^-35
    "TOP": dict(x=0, wv=0, bv=0, w2=0, e2=0, const=False, steer="TOP", res=False),
}
FFN_M = (128, 300)          # one block; ragged M over three blocks
FFN_RANGE_CASES = [(kind, M) for kind in FFN_KINDS for M in FFN_M]


def ffn_range_inputs(kind, M):
    """-> (case, inputs): tokres_exact_refs.ffn_inputs of a raw rf_ffn_geglu case (seed "W"), scaled as FFN_KINDS says"""
    k = FFN_KINDS[kind]
    c = T.ffn_case(f"range-geglu-M{M}-{_slug(kind)}", [kind], "geglu", M, False, ("W",), res=k["res"])
    i = T.ffn_inputs(c, "W")
    FF = T.FF
    wv, wg, bv, bg = i["w1"][:FF] * 2.0 ** k["wv"], i["w1"][FF:], i["b1"][:FF] * 2.0 ** k["bv"], i["b1"][FF:]
    if k["const"]:
        g = torch.Generator().manual_seed(M + len(kind))
        wg = torch.zeros_like(wg)
        bg = torch.tensor([8.0, 16.0, 0.0, 16.0, 8.0], dtype=F64)[torch.randint(0, 5, (FF,), generator=g)]
    i["x"], i["w1"], i["b1"], i["w2"] = i["x"] * 2.0 ** k["x"], torch.cat([wv, wg], 0), torch.cat([bv, bg], 0), i["w2"] * 2.0 ** k["w2"]
    i["b2"] = i["b2"] * 2.0 ** k["e2"]
    if i["res"] is not None:
        i["res"] = i["res"] * 2.0 ** k["e2"]
    if k["steer"]:
        i["b2"] = torch.zeros_like(i["b2"])
        i["b2"] = _steered(T.ffn_reference(c, i, F16)["out_exact"], k["steer"])
        assert T.fits32(i["b2"])
    return c, i


def ffn_range_reference(c, i, dt):
    """tokres_exact_refs.ffn_reference for one storage type (the hidden value is rounded to THAT type), with the exactness rules asserted: gates 0 or an
    integer >= 8, both contractions below 2^24 units, every intermediate an fp32 value"""
    o = T.ffn_reference(c, i, dt)
    what = f"{c['id']}/{dt}"
    gate = o["gate"]
    assert bool(((gate == 0) | ((gate >= 8) & (gate == gate.round()))).all()) and bool((gate > 0).any()), what
    for key in ("x", "w1", "w2", "res"):
        assert i.get(key) is None or T.representable(i[key], dt), f"{what}: {key}"
    # (value and gate columns are separate accumulators, each with its own unit: a gate made by its bias alone is 0 + 8 or 0 + 16)
    T.assert_contraction_exact(what + " GEMM 1 value", o["xh"], i["w1"][:T.FF], i["b1"][:T.FF])
    if bool((i["w1"][T.FF:] != 0).any()):
        T.assert_contraction_exact(what + " GEMM 1 gate", o["xh"], i["w1"][T.FF:], i["b1"][T.FF:])
    T.assert_contraction_exact(what + " GEMM 2", o["h"], i["w2"], i["b2"], i["res"])
    for key in ("h_exact", "x2_exact", "out_exact"):
        assert T.fits32(o[key]), f"{what}: {key}"
    return o


def ffn_hidden_mutant(c, i, o, mut):
    """the output when the hidden value is stored by `mut` instead of the true fp16 store"""
    x2 = mut(o["h_exact"]).double() @ i["w2"].T + i["b2"] + (i["res"] if i["res"] is not None else 0.0)
    return store16(x2)


# ------------------------------------------------------------------------------------------------ rf_ffn_block: plain, LayerNorm-fused, to_out in front
# kind -> exponents per tensor (missing = 0).  e0: bo, ctx, res0 (to_out's epilogue); e3: res2; steer: bpo is steered onto the class (the output is linear in it)
_CHAIN = dict(wv=-5, bv=-29, b2=-27, wpo=10, e3=-14, bpo=-14, const=True)          # the feed-forward on a subnormal row, as in FFN_KINDS' hidden case; W2 = +-1/8 stays
BLOCK_KINDS = {
    "S-in Wpo, S-out": dict(wpo=-24, e3=-24, steer="S-out"),          # the re-rounded feed-forward output (a normal value) against subnormal Wpo: unit 2^-27, bpo on the ties
    "TOP": dict(steer="TOP"),
    # (two-level LayerNorm rows times 2^7: every a_m >= 1, the normalised row is +-1 exactly and the sums under a bias of 65520 stay whole eighths)
    "TOP, rows of a >= 1": dict(x=7, steer="TOP"),
    # x = m 2^-24: the hidden value is k 2^-26 / k 2^-25 and x2 = h W2^T + b2 + x a multiple of 2^-27 of a few subnormal steps -- the feed-forward output the kernel
    # re-rounds to fp16 in front of proj_out lies in the S-out band, ties included, and proj_out's A operand is a subnormal made in the kernel (Wpo = +-2^10 lifts it)
    "S-in x, x2 S-out": dict(x=-24, **_CHAIN),
    # to_out with Wo = +-2^-24: x1 = k 2^-24 is stored (checked bit for bit) and read back as the residual and the feed-forward's input
    "S-in Wo, x1 and x2 S-out": dict(wo=-24, e0=-24, **_CHAIN),
}
BLOCK_FORMS = {"plain": dict(form="tail", ln=False, M=300), "LayerNorm-fused": dict(form="tail", ln=True, M=300), "to_out in front": dict(form="front", ln=False, M=512, S=2, rps0=256)}
BLOCK_CASES = [(f, k) for f, ks in (("plain", ("S-in Wpo, S-out", "TOP", "S-in x, x2 S-out")), ("LayerNorm-fused", ("S-in Wpo, S-out", "TOP, rows of a >= 1")),
                                    ("to_out in front", ("S-in Wpo, S-out", "TOP", "S-in Wo, x1 and x2 S-out"))) for k in ks]


def block_range_inputs(form, kind):
    k, f = BLOCK_KINDS[kind], dict(BLOCK_FORMS[form])
    c = T.ffn_case(f"range-block-{_slug(form)}-{_slug(kind)}", [form, kind], f.pop("form"), f.pop("M"), f.pop("ln"), ("W",), **f)
    i = T.ffn_inputs(c, "W")
    e = lambda key: 2.0 ** k.get(key, 0)
    FF = T.FF
    wv, wg, bv, bg = i["w1"][:FF] * e("wv"), i["w1"][FF:], i["b1"][:FF] * e("bv"), i["b1"][FF:]
    if k.get("const") and bool((wg != 0).any()):          # (the front and LayerNorm forms already take their gates from the bias)
        g = torch.Generator().manual_seed(len(form) + len(kind))
        wg, bg = torch.zeros_like(wg), torch.tensor([8.0, 16.0, 0.0, 16.0, 8.0], dtype=F64)[torch.randint(0, 5, (FF,), generator=g)]
    i["w1"], i["b1"] = torch.cat([wv, wg], 0), torch.cat([bv, bg], 0)
    for key, ex in (("x", "x"), ("wo", "wo"), ("bo", "e0"), ("ctx", "e0"), ("res0", "e0"), ("w2", "w2"), ("b2", "b2"), ("wpo", "wpo"), ("bpo", "bpo"), ("res2", "e3")):
        if i.get(key) is not None:
            i[key] = i[key] * e(ex)
    if k.get("steer"):
        i["bpo"] = torch.zeros_like(i["bpo"])
        i["bpo"] = _steered(T.ffn_reference(c, i, F16)["out_exact"], k["steer"])
        assert T.fits32(i["bpo"])
    return c, i


def block_range_reference(c, i, dt):
    """tokres_exact_refs.ffn_reference of one type with the exactness rules asserted: every contraction below 2^24 units of its own unit, every
    intermediate an fp32 value, LayerNorm rows two-level, gates 0 or an integer >= 7 (the harness's rule)"""
    o = T.ffn_reference(c, i, dt)
    what = f"{c['id']}/{dt}"
    gate = o["gate"]
    assert bool(((gate == 0) | ((gate >= 7) & (gate == gate.round()))).all()) and bool((gate > 0).any()), what
    for key in ("w1", "w2", "wpo", "wo", "x", "att", "res0", "res2"):
        assert i.get(key) is None or T.representable(i[key], dt), f"{what}: {key}"
    if c["form"] == "front":
        T.assert_contraction_exact(what + " to_out", o["att_rows"], i["wo"], i["bo"], i["ctx"], i["res0"])
    x = o["x1"] if c["form"] == "front" else i["x"]
    if c["ln"]:
        T.assert_two_level(what, x, dt)
    T.assert_contraction_exact(what + " GEMM 1 value", o["xh"], i["w1"][:T.FF], i["b1"][:T.FF])
    if bool((i["w1"][T.FF:] != 0).any()):
        T.assert_contraction_exact(what + " GEMM 1 gate", o["xh"], i["w1"][T.FF:], i["b1"][T.FF:])
    T.assert_contraction_exact(what + " GEMM 2", o["h"], i["w2"], i["b2"], x)
    T.assert_contraction_exact(what + " proj_out", o["x2"], i["wpo"], i["bpo"], i["res2"])
    for key in ("x1_exact", "h_exact", "x2_exact", "out_exact"):
        assert key not in o or T.fits32(o[key]), f"{what}: {key}"
    return o


def block_x2_mutant(c, i, o, mut):
    """the output when the feed-forward output in front of proj_out is stored by `mut` instead of the true fp16 store"""
    return store16(mut(o["x2_exact"]).double() @ i["wpo"].T + i["bpo"] + i["res2"])


# ------------------------------------------------------------------------------------------------ rf_attn_in
# two-level cases (qkv bit for bit): the qkv store; general cases (tok bit for bit, qkv to the harness's limit): the tok store and proj_in's operands
ATTN_IN_KINDS = {
    "S-in Wqkv, S-out": dict(two_level=True, wqkv=-24, steer=("bqkv", "S-out")),          # normalised rows +-r against subnormal Wqkv, bqkv on the ties
    "TOP": dict(two_level=True, x=7, steer=("bqkv", "TOP")),          # (rows times 2^7: every a_m >= 1, the normalised row is +-1, qkv whole numbers)
    "S-in x, tok S-out": dict(two_level=False, x=-24, w=-11, steer=("rv", "S-out")),      # proj_in: unit 2^-35, the row vector steered: tok on the ties
    "S-in W'": dict(two_level=False, w=-24, rv=-24),                                       # tok = k 2^-24: exact subnormals and small normals
}
ATTN_IN_SHAPES = ((1, 128), (3, 256))          # (samples, rows per sample): w_sample_stride = 0; per-sample W' and row vector
ATTN_IN_CASES = [(kind, s) for kind in ATTN_IN_KINDS for s in ATTN_IN_SHAPES]


def attn_in_range_inputs(kind, shape):
    """(TOP is for qkv alone: a tok of +-inf has no LayerNorm.)  The general cases keep the harness's qkv generator: |qkv| >= 16 from the bias"""
    k = ATTN_IN_KINDS[kind]
    S, rps = shape
    c = T.attn_case(f"range-attn-{S}x{rps}-{_slug(kind)}", [kind], S, rps, k["two_level"])
    i = T.attn_inputs(c, "W")
    for key in ("x", "w", "rv", "wqkv"):
        i[key] = i[key] * 2.0 ** k.get(key, 0)
    if k.get("steer"):
        key, cls = k["steer"]
        i[key] = torch.zeros_like(i[key])
        o = T.attn_reference(c, i, F16)
        if key == "bqkv":
            i[key] = _steered(o["qkv_exact"], cls)
        else:          # one row of every sample and column on the column's class value
            i[key] = torch.stack([_steered(o["tok_exact"][s * rps:(s + 1) * rps], cls, offset=s) for s in range(S)], 0)
        assert T.fits32(i[key])
    return c, i


def attn_in_range_reference(c, i, dt):
    o = T.attn_reference(c, i, dt)
    what = f"{c['id']}/{dt}"
    for key in ("x", "w", "wqkv"):
        assert T.representable(i[key], dt), f"{what}: {key}"
    for s in range(c["S"]):
        T.assert_contraction_exact(what + " proj_in", i["x"][s * c["rps"]:(s + 1) * c["rps"]], i["w"][s], i["rv"][s])
    assert T.fits32(o["tok_exact"]), what
    if c["two_level"]:
        T.assert_two_level(what, o["tok"], dt)
        T.assert_contraction_exact(what + " qkv", o["xh"], i["wqkv"], i["bqkv"])
        assert T.fits32(o["qkv_exact"]), what
    else:
        assert o["qkv_exact"].abs().min().item() >= 16.0, what
    return o


# ------------------------------------------------------------------------------------------------ rf_gn_silu_conv3x3_small (silu = 0: the activation is the level itself)
# the kernel has at most four output channels: a class's table is walked over the four image shapes (offset = 4 x the shape's index)
HEAD_KINDS = {
    # GroupNorm result k / 4 against taps m 2^-24: unit 2^-26, a row's eight live taps move it by up to 48 subnormal steps; the bias on the ties
    "S-in taps, S-out": dict(w=-24, ga=-2, steer="S-out"),
    "TOP": dict(steer="TOP"),
    # gamma and beta times 2^-25: the GroupNorm result is level 2^-25, rounded to fp16 (odd levels are ties) and fed to the conv as a subnormal A operand;
    # taps of +-m 2^10 make one step of it 2^-14 in the output
    "GroupNorm result S-out": dict(ga=-25, w=10, bias=-14),
    "S-in x": dict(x=-24),                          # x and the partial sums' moments times 2^-24: rstd = 2^23, the same levels
}
HEAD_RANGE_CASES = [(kind, j) for kind in HEAD_KINDS for j in range(len(T.HEAD_SHAPES))]


def head_range_inputs(kind, j):
    k = HEAD_KINDS[kind]
    B, H, W_ = T.HEAD_SHAPES[j]
    c = T.head_case(64, 4, B, H, W_, "16", 0, (1, 9)[j % 2])
    c = dict(c, id=f"range-{c['id']}-{_slug(kind)}")
    i = T.head_inputs(c, "A")          # dense taps of +-{1, 2} on all nine positions against sparse activations (seed "W" keeps eight taps of a row, all at one position)
    e = lambda key: 2.0 ** k.get(key, 0)
    i["gamma"], i["beta"], i["w"], i["bias"] = i["gamma"] * e("ga"), i["beta"] * e("ga"), i["w"] * e("w"), i["bias"] * e("bias")
    if "x" in k:          # x 2^-24: mean 2^-24, sum of squares 2^-48; gamma / sqrt(var) is 2^24 times larger, y the same
        i["x"] = i["x"] * e("x")
        i["part"] = i["part"] * torch.tensor([e("x"), e("x") ** 2], dtype=F64)
    i["y_unit"] = e("ga")
    if k.get("steer"):
        i["bias"] = torch.zeros_like(i["bias"])
        i["bias"] = _steered(T.head_reference(c, i, F16)["out_exact"], k["steer"], offset=4 * j)
        assert T.fits32(i["bias"])
    return c, i


def head_range_reference(c, i, dt):
    o = T.head_reference(c, i, dt)
    what = f"{c['id']}/{dt}"
    assert T.representable(i["x"], dt) and T.representable(i["w"], dt), what
    lv = torch.tensor(T.SILU_LEVELS, dtype=F64)
    assert bool(((o["y"] / i["y_unit"])[..., None] == lv).any(-1).all())          # the levels, times the power of two the affine carries and T.fits32(o["y"]), what
    T.assert_contraction_exact(what, o["A"], i["w"], i["bias"])
    assert T.fits32(o["out_exact"]), what
    return o


def head_act_mutant(c, i, o, mut):
    """the output when the GroupNorm result is stored by `mut` instead of the true fp16 store"""
    B, H, W_, Cc = c["B"], c["H"], c["W"], c["C"]
    A = T.conv3x3_taps(mut(o["act_exact"]).double().reshape(B, H, W_, Cc)).reshape(B * H * W_, 9 * Cc)
    return store16(A @ i["w"].T + i["bias"])


# ------------------------------------------------------------------------------------------------ layout and pack kernels that write fp16
def edge_values_f32():
    """the fp32 edge patterns of side_refs (fp16 / bf16 ties, overflow, subnormals, infinities)"""
    return torch.from_numpy(np.array(SR._F32_EDGE_BITS, dtype=np.uint32).view(np.float32).copy())


def layout_edge_input():
    """[B, C, H, W] fp32 of side_refs' layout shape: the edge patterns, rotated through the channels so that every channel carries every pattern"""
    e = edge_values_f32()
    n = SR.LAYOUT_B * SR.LAYOUT_C * SR.LAYOUT_H * SR.LAYOUT_W
    idx = torch.arange(n).reshape(SR.LAYOUT_B, SR.LAYOUT_C, SR.LAYOUT_H, SR.LAYOUT_W)
    c = torch.arange(SR.LAYOUT_C).view(1, -1, 1, 1)
    return e[(idx + 7 * c) % e.numel()]


def ddim_pack_edge_inputs():
    """img, z [B, 4, h, w] and mask [B, 1, h, w] fp32 holding the edge patterns (z shifted against img); the mask keeps its 0 / 1 values plus the
    patterns a mask can meet: the smallest subnormal and the tie below it"""
    e = edge_values_f32()
    B, h, w = SR.DDIM_B, SR.DDIM_H, SR.DDIM_W
    idx = torch.arange(B * 4 * h * w).reshape(B, 4, h, w)
    img, z = e[idx % e.numel()], e[(idx * 3 + 11) % e.numel()]
    m = torch.tensor([0.0, 1.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25], dtype=torch.float32)
    mask = m[torch.arange(B * h * w).reshape(B, 1, h, w) % m.numel()]
    return dict(img=img, z=z, mask=mask)
