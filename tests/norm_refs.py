"""Test infrastructure of the normalisation kernels (reface_amd/csrc/norm.hip): fp64 references on the values as stored, exactly checkable
generators, guarded buffers, the derived tolerance and the case tables of tests/test_norm_exact_gpu.py.  Importable without a GPU; pinned on
the CPU by tests/test_norm_refs_cpu.py.

Layouts (include/reface_hip.h): activations channels-last [B][HW][C] with a row pitch; GroupNorm partial sums [B][nchunks][32][2] fp64
(sum, sum of squares per group and pixel chunk, chunk c = pixels [c ppc, min(HW, (c + 1) ppc)), ppc = ceil(HW / nchunks)); split-bf16 pairs
[C hi | C lo] per row; fp8 output = e4m3fn bytes + one E8M0 code per 32-channel block."""
import functools

import numpy as np
import torch

from e4m3_ref import e4m3fn_encode_rne_sat_np

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
RF_F32, RF_BF16, RF_BF16X3, RF_F16 = 0, 1, 3, 4          # include/reface_hip.h (test_norm_refs_cpu.py compares them with reface_amd._lib)
CODE = {F32: RF_F32, BF16: RF_BF16, F16: RF_F16, "split": RF_BF16X3}
STEP = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11, "split": 2.0 ** -16}          # relative rounding step of the storage (test_ops_gpu.STEP); a
# split pair carries 16 significant bits: |y - hi| <= 2^-9 |y| and lo = bf16(y - hi) is 2^-9 of that at the most
TINY = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -25, "split": 0.0}          # half the spacing of the fp16 subnormals (absolute floor of one storage rounding)
GUARD = 64                # guard rows / elements around every output region
GN_THREADS, GN_SLOTS, LN_MAXV = 256, 4, 6


def out_torch_dtype(out):
    return BF16 if out == "split" else (torch.uint8 if out == "fp8" else out)


def vec_of(dt):
    return 4 if dt == F32 else 8


# ------------------------------------------------------------------------------------------------ the host arithmetic of norm.hip, restated
def gn_geometry(in_dt, C):
    """thread geometry of gn_stats_kernel / gn_apply_kernel: TV channel-vector threads x PL pixel lanes, `idle` threads left over, ns vectors
    per thread (the apply pass instantiates 1, 2 or 4 slots), LDS bytes of the statistics pass"""
    vec = vec_of(in_dt)
    nvec = C // vec
    TV = min(nvec, GN_THREADS)
    PL = GN_THREADS // TV
    ns = -(-nvec // GN_THREADS)
    return dict(vec=vec, nvec=nvec, TV=TV, PL=PL, idle=GN_THREADS - TV * PL, ns=ns, slots=1 if ns <= 1 else (2 if ns <= 2 else GN_SLOTS),
                lds=2 * PL * C * 8)


def apply_achunks(B, HW):
    return max(1, min(-(-1024 // B), (HW + 1) // 2))


def ln_nv(in_dt, C):
    nv = -(-(C // vec_of(in_dt)) // 64)
    return nv if nv <= 3 else LN_MAXV


def fold_nit(C):
    return 1 if C <= 512 else (2 if C <= 1024 else 3)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def stored(x, dt):
    """the values as the storage type holds them, in fp64"""
    return x.to(dt).to(F64)


# ------------------------------------------------------------------------------------------------ fp64 references
def chunk_partials(x, nchunks, mutant=None):
    """x [B, HW, C] fp64 -> [B, nchunks, 32, 2] fp64 (sum, sum of squares).  Mutants: "drop_last_pixel" (of every chunk), "group_mod32"."""
    B, HW, C = x.shape
    cpg = C // 32
    ppc = -(-HW // nchunks)
    out = torch.zeros((B, nchunks, 32, 2), dtype=F64)
    for c in range(nchunks):
        p0, p1 = c * ppc, min(HW, c * ppc + ppc)
        if mutant == "drop_last_pixel":
            p1 -= 1
        if p1 <= p0:
            continue
        xs = x[:, p0:p1]
        xg = xs.reshape(B, p1 - p0, cpg, 32).permute(0, 1, 3, 2) if mutant == "group_mod32" else xs.reshape(B, p1 - p0, 32, cpg)
        out[:, c, :, 0] = xg.sum((1, 3))
        out[:, c, :, 1] = (xg * xg).sum((1, 3))
    return out


def moments_of_partials(partial, HW, C):
    """[B, nchunks, 32, 2] -> (mean, var) [B, 32]: var = sq / n - mean^2, clamped at 0 (what every consumer of the partials evaluates, in fp64)"""
    n = float(HW * (C // 32))
    s = partial.sum(1)
    mean = s[..., 0] / n
    return mean, (s[..., 1] / n - mean * mean).clamp_min(0.0)


def moments(x):
    """two-pass group moments of x [B, HW, C] fp64 -> (mean, var) [B, 32]"""
    B, HW, C = x.shape
    xg = x.reshape(B, HW, 32, C // 32)
    mean = xg.mean((1, 3))
    return mean, ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))


def silu64(y):
    return y * torch.sigmoid(y)


def group_index(C, mutant=None):
    c = torch.arange(C)
    return c % 32 if mutant == "group_mod32" else c // (C // 32)


def gn_apply_terms(x, mean, var, gamma, beta, eps, mutant=None, vec=8):
    """the per-element terms of the apply pass in fp64: (x sc, mean sc, beta) with sc = gamma / sqrt(var + eps); y = x sc - mean sc + beta.
    Mutants: "group_mod32", "affine_shift_vector" (gamma / beta read one 16-byte vector further on)."""
    C = x.shape[-1]
    g = group_index(C, mutant)
    gamma, beta = gamma.to(F64), beta.to(F64)
    if mutant == "affine_shift_vector":
        gamma, beta = torch.roll(gamma, -vec), torch.roll(beta, -vec)
    sc = (gamma / torch.sqrt(var + eps)[:, g])[:, None, :]
    return x * sc, mean[:, g][:, None, :] * sc, beta.expand_as(x)


def gn_apply_ref(x, mean, var, gamma, beta, eps, silu, mutant=None, vec=8):
    """GroupNorm(32) (+SiLU) of x [B, HW, C] fp64 with the given group moments"""
    C = x.shape[-1]
    g = group_index(C, mutant)
    gamma, beta = gamma.to(F64), beta.to(F64)
    if mutant == "affine_shift_vector":
        gamma, beta = torch.roll(gamma, -vec), torch.roll(beta, -vec)
    y = (x - mean[:, g][:, None, :]) / torch.sqrt(var + eps)[:, g][:, None, :] * gamma + beta
    return silu64(y) if silu else y


def groupnorm_ref(x, gamma, beta, eps, silu):
    mean, var = moments(x)
    return gn_apply_ref(x, mean, var, gamma, beta, eps, silu)


def layernorm_ref(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def softmax_rows_ref(x):
    e = torch.exp(x.to(F64) - x.to(F64).amax(-1, keepdim=True))
    return e / e.sum(-1, keepdim=True)


def fold_weights_ref(W, mean, var, gamma, eps, out_dt):
    """W'[s][n][k] = W[n][k] rstd[s][g(k)] gamma[k] in fp64 and as stored in out_dt (fp64 copy)"""
    C = W.shape[1]
    g = group_index(C)
    a = gamma.to(F64)[None, :] / torch.sqrt(var + eps)[:, g]          # [B, C]
    wp = W.to(F64)[None] * a[:, None, :]
    return wp, stored(wp, out_dt)


def fold_rowvec_ref(W, wp_stored, mean, beta, bias):
    """r[s][n] = bias[n] + sum_k W[n][k] beta[k] - sum_k W'_stored[s][n][k] mean[s][g(k)]; also the sum of the terms' magnitudes"""
    C = W.shape[1]
    g = group_index(C)
    t1 = W.to(F64) * beta.to(F64)[None, :]                            # [N, C]
    t2 = wp_stored * mean[:, g][:, None, :]                           # [B, N, C]
    b = torch.zeros(W.shape[0], dtype=F64) if bias is None else bias.to(F64)
    return b[None] + t1.sum(1)[None] - t2.sum(2), b.abs()[None] + t1.abs().sum(1)[None] + t2.abs().sum(2)


def split_pair(y32):
    """fp32 -> (hi, lo) bf16: hi = RNE(y), lo = RNE(y - hi) (y - hi is exact in fp32)"""
    hi = y32.to(BF16)
    return hi, (y32 - hi.float()).to(BF16)


def split_rows(y32, ld, lo_at=None):
    """rows [M, C] fp32 -> [M, ld] bf16 rows [C hi | C lo | zeros]; lo_at moves the lo plane (the "+C-8" mutant)"""
    M, C = y32.shape
    hi, lo = split_pair(y32)
    out = torch.zeros((M, ld), dtype=BF16)
    out[:, :C] = hi
    at = C if lo_at is None else lo_at
    out[:, at:at + C] = lo
    return out


def quant_act_np(y):
    """numpy restatement of the fp8 block quantiser (quant_block8 in csrc/common.h; test_ops_gpu._quant_act_ref's scale rule): per 32-channel
    block the E8M0 code of the smallest power of two 2^(code - 127) with amax / 2^(code - 127) <= 448, then e4m3fn RNE of y * 2^(127 - code).
    y: float array [..., C] of fp32-representable values -> (bytes uint8 [..., C], codes uint8 [..., C / 32])"""
    y = np.asarray(y, dtype=np.float64)
    *lead, C = y.shape
    yb = y.reshape(*lead, C // 32, 32)
    amax = np.abs(yb).max(-1)
    m, e = np.frexp(amax)                                             # amax = m 2^e, m in [0.5, 1): amax = (2m) 2^(e - 1)
    code = np.clip(e - 1 + 127 - 8 + (2 * m > 1.75), 0, 253)
    code = np.where(amax > 0, code, 0).astype(np.int64)
    q = e4m3fn_encode_rne_sat_np(yb * np.exp2(127.0 - code)[..., None])
    return q.reshape(*lead, C), code.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ guarded buffers
def bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


class Guarded:
    """`view` ([rows, cols], row pitch ld) inside a larger sentinel-filled allocation (NaN; 0xA5 for bytes): GUARD rows in front and behind,
    the pitch gap and whatever `live` leaves out.  check() proves everything outside the live region untouched, filled() that no sentinel is
    left inside it."""

    def __init__(self, rows, cols, ld, dtype, device="cpu", live_rows=None):
        assert ld >= cols
        self.byte = dtype == torch.uint8
        self.buf = torch.full((rows + 2 * GUARD, ld), 0xA5 if self.byte else float("nan"), dtype=dtype, device=device)
        self.view = self.buf[GUARD:GUARD + rows, :cols]
        self.mask = torch.zeros((rows + 2 * GUARD, ld), dtype=torch.bool, device=device)
        self.mask[GUARD:GUARD + (rows if live_rows is None else live_rows), :cols] = True
        self.before = self.buf.clone()
        self.ld = ld

    def ptr(self):
        return self.view.data_ptr()

    def check(self, what=""):
        same = bits(self.buf) == bits(self.before)
        bad = int((~same[~self.mask]).sum())
        assert bad == 0, f"{what}: wrote outside its region ({bad} elements changed)"

    def filled(self, what=""):
        if not self.byte:
            left = int(torch.isnan(self.buf[self.mask]).sum())
            assert left == 0, f"{what}: {left} output elements not written"

    def fetch(self, what=""):
        """guards checked -> the live view on the host"""
        self.check(what)
        self.filled(what)
        return self.view.cpu()


def guarded(shape, ld, dtype, device="cpu", live_rows=None):
    """shape = (rows, cols) of the view the kernel writes, ld its row pitch in elements"""
    return Guarded(shape[0], shape[1], ld, dtype, device, live_rows)


# ------------------------------------------------------------------------------------------------ the tolerance of the non-exact apply cases
def tol_apply(y, xsc, msc, beta, out, silu):
    """Limit of |kernel - fp64 reference| for the GroupNorm apply pass with GIVEN partial sums; y = xsc - msc + beta is the fp64 pre-activation
    value, out the output storage (a dtype or "split").  Derived from the kernel's arithmetic (u = 2^-24, no FMA contraction), not from its
    output:
      mean and rstd come out of fp64 and are rounded to fp32 once each (the fp64 cancellation in sq/n - mean^2 is 2^-53 (mean/std)^2, below
      1e-9 up to mean/std = 1000);  sc = fl(rstd gamma): 2u;  sh = fl(beta - fl(mean sc)): 4u |mean sc| + u (|beta| + |mean sc|);
      y = fl(fl(x sc) + sh): 3u |x sc| + u (|x sc| + |beta| + |mean sc|)   ->   |dy| <= u (4 |x sc| + 6 |mean sc| + 2 |beta|)
      <= 2^-21 (|x sc| + |mean sc| + |beta|) with room for the second-order terms.
      SiLU  y / (1 + 2^(-y log2 e))  on v_exp_f32 / v_rcp_f32 (csrc/common.h: about 1 ulp = 2^-23 each): |silu'| <= 1.1 carries dy through; the
      exponent's argument is rounded twice (2u |y| log2 e, times ln 2 in the exponential), and e = 2^(..) enters through e / (1 + e) =
      sigmoid(-y) = w:  relative  2^-23 w (v_exp) + 2^-23 |y| w (argument) + 2^-23 (v_rcp) + 2u (1 + e and the final product).
      One storage rounding STEP[out] |ref| (0 for fp32) and half an fp16 subnormal step on top."""
    dy = 2.0 ** -21 * (xsc.abs() + msc.abs() + beta.abs())
    if not silu:
        return STEP[out] * y.abs() + dy + TINY[out]
    ref, w = silu64(y), torch.sigmoid(-y)
    rel = 2.0 ** -23 * w + 2.0 ** -23 * y.abs() * w + 2.0 ** -23 + 2.0 ** -23
    return STEP[out] * ref.abs() + 1.1 * dy + rel * ref.abs() + TINY[out]


def tol_yardstick(ref, out, e32):
    """the bound of the conditioning cases: one storage rounding + 4 x the error of PyTorch's own fp32 CPU evaluation on the same stored inputs
    (the factor 4: a different but equally valid fp32 evaluation order)"""
    return STEP[out] * ref.abs() + 4.0 * e32 + TINY[out]


# ------------------------------------------------------------------------------------------------ exact generators
GAMMAS = (0.5, -1.0, 2.0, -4.0, -0.5, 1.0, -2.0, 4.0)


def exact_affine(C):
    """gamma in {+-0.5, +-1, +-2, +-4}, beta on a quarter-integer grid (|beta| <= 4), both varying with the channel with periods coprime to 8 / 32"""
    c = torch.arange(C)
    gamma = torch.tensor(GAMMAS, dtype=F32)[(c * 3 + c // 8) % 8]
    beta = (((c * 5 + c // 32) % 33) - 16).to(F32) / 4
    return gamma, beta


def stats_exact_input(B, HW, C, seed):
    """x = k / 4 with integer |k| <= 16, varying per pixel and channel, group offsets of 3 to 8 (a non-zero mean per group): every sum and sum of squares over any subset
    is an integer multiple of 2^-2 / 2^-4 far below 2^24 of them (stats_exact_bound), hence exact in fp32 and fp64 in any order"""
    off = torch.tensor([o if abs(o) >= 3 else (5 if g % 2 else -5) for g, o in ((g, ((g * 5) % 17) - 8) for g in range(32))])
    k = off.repeat_interleave(C // 32)[None, None, :] + torch.randint(-6, 7, (B, HW, C), generator=_gen(seed))
    return k.clamp(-16, 16).to(F64) / 4


def stats_exact_bound(in_dt, HW, C, nchunks):
    """the largest per-thread sum of k^2 the statistics pass can form for this shape: pixels per thread x 16^2 (must stay below 2^24)"""
    ppc = -(-HW // nchunks)
    return -(-ppc // gn_geometry(in_dt, C)["PL"]) * 256


def exact_means(B):
    """integer group means [B, 32], |m| <= 8"""
    b, g = torch.arange(B)[:, None], torch.arange(32)[None, :]
    return (((b * 11 + g * 3) % 17) - 8).to(F64)


def exact_partials(mean, HW, C, nchunks, seed):
    """host-written partial sums [B, nchunks, 32, 2] with group sum n m and sum of squares n (m^2 + 4) exactly (integers, split over the chunks
    as integers): var = 4 and, with eps = 0, rstd = 0.5 exactly"""
    B = mean.shape[0]
    n = float(HW * (C // 32))
    tot = torch.stack([n * mean, n * (mean * mean + 4.0)], -1)                       # [B, 32, 2]
    part = torch.randint(-1000, 1001, (B, nchunks, 32, 2), generator=_gen(seed)).to(F64)
    part[:, -1] = tot - part[:, :-1].sum(1)
    return part


def apply_exact_input(B, HW, C, seed):
    """x = k / 4, |k| <= 64: with sc = 0.5 gamma in +-{1/4 .. 2} and sh = beta - m sc, y = x sc + sh is a multiple of 2^-4 below 2^6: exact in fp32"""
    return torch.randint(-64, 65, (B, HW, C), generator=_gen(seed)).to(F64) / 4


def fold_exact_weights(N, C, seed):
    """W = k / 4, |k| <= 32 (|W| <= 8); bias on the quarter-integer grid"""
    g = _gen(seed)
    return (torch.randint(-32, 33, (N, C), generator=g).to(F32) / 4), (torch.randint(-16, 17, (N,), generator=g).to(F32) / 4)


@functools.lru_cache(maxsize=None)
def ln_exact_input(M, C, seed):
    """rows m_row +- 2 with as many + as -: mean = m_row, var = 4 and, with eps = 0, y = +-gamma + beta exactly"""
    g = _gen(seed)
    base = torch.cat([torch.ones(C // 2), -torch.ones(C - C // 2)])
    s = torch.stack([base[torch.randperm(C, generator=g)] for _ in range(M)])
    m = ((torch.arange(M) * 5) % 21 - 10).to(F64)
    return m[:, None] + 2.0 * s.to(F64), m, s.to(F64)


def softmax_exact_input(rows, cols, seed):
    """k zeros among entries of -1000 -> (x fp32 [rows, cols], expected fp32): fl32(1 / k) at the zeros, 0 elsewhere.  k differs per row; row 0
    holds its zero in the last column, row 1 in the first"""
    g = _gen(seed)
    x = torch.full((rows, cols), -1000.0, dtype=F32)
    ref = torch.zeros((rows, cols), dtype=F32)
    for r in range(rows):
        k = min(cols, (1, 2, 3, 7, 5, 4, 6)[r % 7])
        idx = torch.randperm(cols, generator=g)[:k]
        if r == 0:
            idx[0] = cols - 1
        if r == 1 and not bool((idx == 0).any()):
            idx[0] = 0
        x[r, idx] = 0.0
        ref[r, idx] = (torch.ones((), dtype=F32) / torch.tensor(float(k), dtype=F32))
    return x, ref


# ------------------------------------------------------------------------------------------------ case tables of tests/test_norm_exact_gpu.py
GN_PAIRS = [(F32, F32), (F32, BF16), (F32, "split"), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]
PAIR_ID = lambda p: f"{str(p[0])[6:]}-{p[1] if isinstance(p[1], str) else str(p[1])[6:]}"

# A: statistics.  (HW, nchunks, extra pitch in vectors)
STATS_DTYPES = [F32, BF16, F16]
STATS_C = [32, 64, 320, 1280, 2560, 4096]
STATS_SHAPES = [(1, 1, 0), (2, 7, 1), (31, 7, 0), (33, 32, 2), (81, 1, 1), (81, 7, 0), (1000, 32, 0), (1000, 1, 3)]
STATS_B = 3
FINALIZE_CHUNKS = [1, 9, 96, 97]


def c_for_ns(in_dt, ns):
    """the smallest channel count (a multiple of 32) that takes `ns` channel vectors per thread"""
    v = vec_of(in_dt)
    return {1: 32, 2: 257 * v + (-257 * v) % 32, 3: 513 * v + (-513 * v) % 32, 4: 769 * v + (-769 * v) % 32}[ns]


def apply_exact_cases(in_dt, out):
    """B: dicts B, HW, C, nchunks, xpad, opad (extra pitch in elements) of one type pair"""
    cases = []
    for ns in (1, 2, 3, 4):                                                        # the dispatch: 1 / 2 / 4-slot kernels (ns = 3 takes 4)
        cases.append(dict(B=2, HW=3, C=c_for_ns(in_dt, ns), nchunks=1, xpad=8, opad=8))
    for HW in (1, 2, 3, 33):
        cases.append(dict(B=3, HW=HW, C=320, nchunks=9, xpad=0 if HW == 2 else 16, opad=0 if HW == 3 else 24))
    for B in (1, 3, 600, 1025):                                                    # achunks = min(ceil(1024 / B), (HW + 1) / 2): 2, 2, 2, 1
        cases.append(dict(B=B, HW=4, C=32, nchunks=1 if B > 3 else 9, xpad=8, opad=8))
    for nchunks in (1, 9, 97):
        cases.append(dict(B=2, HW=33, C=64, nchunks=nchunks, xpad=8, opad=16))
    return cases


# C: random values against fp64, host-written fp64 partials of the stored x (nchunks = 7)
APPLY_RANDOM_SHAPES = [dict(B=2, HW=33, C=320), dict(B=2, HW=5, C=2560)]          # ragged PL; 2 slots (16-bit) / 3 -> 4 slots (fp32)
APPLY_RANDOM_CASES = [(p, silu, eps) for p in GN_PAIRS for silu in (0, 1) for eps in (1e-5, 1e-6)]


def apply_random_inputs(pair, silu, eps, shape, unrounded_stats=False):
    """inputs of a C case: x as stored (fp64), gamma / beta fp32, fp64 partials of the stored values (the "statistics of unrounded values"
    mutant takes them before the rounding to the storage type)"""
    in_dt = pair[0]
    B, HW, C = shape["B"], shape["HW"], shape["C"]
    g = _gen(1000 + 7 * GN_PAIRS.index(pair) + 3 * silu + (1 if eps < 5e-6 else 0) + C)
    raw = (torch.randn((B, HW, C), generator=g, dtype=F64) * 2.0 + 0.7)
    x = stored(raw, in_dt)
    gamma = (1.0 + 0.5 * torch.randn((C,), generator=g, dtype=F64)).to(F32)
    beta = (0.5 * torch.randn((C,), generator=g, dtype=F64)).to(F32)
    partial = chunk_partials(raw if unrounded_stats else x, 7)
    return dict(x=x, gamma=gamma, beta=beta, partial=partial, nchunks=7)


# D / E: conditioning probes (mean / std of the input)
RATIOS = {F32: (0, 64, 1000), BF16: (0, 8, 64), F16: (0, 8, 64)}


def conditioned(shape, ratio, in_dt, seed):
    """unit-spread values around `ratio`, as the storage type holds them (fp64)"""
    return stored(torch.randn(shape, generator=_gen(seed), dtype=F64) + float(ratio), in_dt)


def random_affine(C, seed):
    g = _gen(seed)
    return (1.0 + 0.5 * torch.randn((C,), generator=g, dtype=F64)).to(F32), (0.5 * torch.randn((C,), generator=g, dtype=F64)).to(F32)


# E: LayerNorm
LN_PAIRS = GN_PAIRS
LN_C = {F32: [4, 256, 260, 768, 772, 1536], BF16: [8, 32, 512, 520, 1024, 1032, 1536, 1544, 3072], F16: [8, 32, 512, 520, 1024, 1032, 1536, 1544, 3072]}
LN_C_FP8 = [32, 512, 544, 1024, 1056, 1536, 1568, 3072]                          # (the fp8 form needs whole 32-channel blocks)
LN_M = [1, 3, 5, 131]

# F: fold.  (C, N, with bias, nchunks)
FOLD_OUT = [BF16, F16, F32]
FOLD_CASES = [(32, 320, True, 1), (512, 7, False, 9), (544, 9, True, 1), (1024, 1, True, 9), (1056, 7, True, 1), (1536, 9, False, 9), (1536, 320, True, 1),
              (512, 9, True, 1), (1024, 7, False, 1)]
FOLD_B = 3

# G: softmax.  (cols, extra pitch)
SOFTMAX_CASES = [(4, 4), (8, 12), (1020, 4), (1024, 8), (1028, 4), (4096, 4), (9216, 16)]
SOFTMAX_ROWS = 5
