"""Exact-operand cases of rf_conv_gemm and their fp64 reference: shared by tests/test_gemm_exact_gpu.py (launches) and tests/test_gemm_exact_cpu.py
(generator bounds, reference against torch, mutants).

Every operand is a small integer times a power of two, so every product and every partial sum -- in ANY order, on any tile, split-K factor or
MFMA shape -- is a multiple of one unit below 2^24 units: fp32 accumulation is exact and the expected output is one value, not an interval.
  fp32 output : dense operands, activations in +-{1, 2, 3}, weights in +-{1, 2, 3}
  16-bit output: each W row (seed "W") or each A row (seed "A") keeps at most NNZ non-zeros, so that |out| <= 255 and the expected value is itself
                 representable in bf16 (asserted before any launch); between the two seeds every k carries a non-zero product in some row
  fp8          : e4m3 integers with per-row / per-block power-of-two scales; C = 320 cases carry the per-tap zero padding to 384
  split-bf16   : values with more than 8 significant bits (lo != 0); expected = hi hi + hi lo + lo hi in fp64 (lo lo is not formed)
  windows      : the win-* cases walk KH x KW / stride / pad_t, pad_l at the geometries of the metric towers (TOWER_WINDOWS), dense with fp32 output
The reference restates include/reface_hip.h's formula: explicit zero padding and slicing, nearest upsampling, channel concatenation, the tail
source, the K orders of `korder`, then ONE fp64 matmul and the epilogue.  `mut` selects a deliberately wrong variant (MUTANTS): the CPU file
proves that every one of them changes an output of some case."""
import math

import torch
import torch.nn.functional as F

from reface_amd import ops

F64 = torch.float64
TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "w8": torch.bfloat16, "x3": torch.bfloat16}
STEP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NNZ = 24                  # non-zero products per output of a 16-bit-output case: 24 * 3 * 3 = 216, + bias 7 + rowvec 7 + residual 15 <= 255
NNZ_STAT = 12             # ... of a case whose stripe sums are steered (LayerNorm records) or that carries the statistics bias: leaves room for that term
EXACT_LIMIT = 2 ** 24
LN_EPS, LN_IN_COLS = 1e-5, 64          # LayerNorm consumer cases: eps, columns per statistics part of the records they are given
GUARD = 64                # guard rows / elements around every output region
INEXACT_ACTS = (ops.ACT_SILU, ops.ACT_QUICK_GELU, ops.ACT_GELU, ops.ACT_SIGMOID)

_DEFAULTS = dict(op="bf16", out="f32", B=1, H=1, W=1, C0=64, C1=0, N=64, ks=1, kh=None, kw=None, creal=0, stride=1, pad=(0, 0, 0, 0), ups=0, korder=0, Cx=0, bias=True,
                 rowvec=False, res=False, act=ops.ACT_NONE, alpha=1.0, ws=0, gn=False, ln=None, wps=False, batch=1, col0=16, ldo_extra=16,
                 sparse="W", gate_const=False, expect={}, small=None,
                 # the range knobs (tests/f16_range_cases.py).  a_exp / w_exp / e_exp: power-of-two scales 2^exp of the activation, weight and epilogue-term
                 # (bias, rowvec, residual) sides, entering unit_of; a_hi / w_hi: the largest integer of the activation / weight side; range16: the
                 # expected 16-bit output is the store rounding of the exactly known fp32 value instead of a representable |out| <= 255.  At these
                 # defaults nothing of a case changes
                 a_exp=0, w_exp=0, e_exp=0, a_hi=3, w_hi=3, range16=False)


def case(id, cells, expect, **kw):
    c = dict(_DEFAULTS)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    # ks is the square shorthand; kh / kw name a window on their own (ks is then the side of a square one, 0 otherwise)
    if c["kh"] is None and c["kw"] is None:
        c["kh"] = c["kw"] = c["ks"]
    else:
        assert c["kh"] and c["kw"] and "ks" not in kw, id
        c["ks"] = c["kh"] if c["kh"] == c["kw"] else 0
    c.update(id=id, cells=tuple(cells), expect=dict(expect))
    return c


def bk_of(c):
    return 32 if c["op"] == "f32" else 64


def geom(c):
    """sizes of the GEMM view of a case"""
    kh, kw, s = c["kh"], c["kw"], c["stride"]
    pt, pl, pb, pr = c["pad"]
    up = 2 if c["ups"] else 1
    Hs, Ws = c["H"] * up, c["W"] * up
    Ho, Wo = (Hs + pt + pb - kh) // s + 1, (Ws + pl + pr - kw) // s + 1
    ctot = c["C0"] + c["C1"]
    taps = 9 if c["ups"] == 2 else kh * kw
    kwin = taps * ctot
    nout = c["N"] // 2 if c["act"] == ops.ACT_GEGLU else c["N"]
    return dict(Ho=Ho, Wo=Wo, M=c["B"] * Ho * Wo, rps=Ho * Wo, ctot=ctot, taps=taps, kwin=kwin, K=kwin + c["Cx"], nout=nout)


def out_dtype(c):
    if c["out"] == "f32":
        return torch.float32
    return torch.bfloat16 if c["op"] == "a8" else TDT[c["op"]]


# ------------------------------------------------------------------------------------------------ generators
def _ints(g, shape, lo, hi, nonzero=True):
    t = torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)
    if nonzero:
        s = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
        t = torch.where(t == 0, s * hi, t)
    return t.to(F64)


def _keep(g, t, n, cover=False, rank=None, first=None):
    """zero all but `n` random entries along the last dim (n + 1 with cover).  cover: the rows together keep EVERY entry -- row r's first
    ceil(width / rows) kept entries are the run that starts at r times that length (shifted by 37 on every wrap, so that an entry recurs at another
    row position), the rest stay random; and every fourth row keeps the LAST entry, every fourth the FIRST one: the two ends of the contraction are
    live in many rows.  rank / first: an order of the rows and how many of them count (interior pixels of a 3x3 window's source first: only those
    are read through all nine taps)"""
    wd = t.shape[-1]
    if n >= wd:
        return t
    idx = torch.rand(t.shape, generator=g).topk(n, dim=-1).indices
    if cover:
        rows = idx[..., 0].numel()
        r = (torch.arange(rows) if rank is None else rank).reshape(idx.shape[:-1])
        nd = min(n, -(-wd // (rows if first is None else max(1, first))))
        for j in range(nd):
            idx[..., j] = (r * nd + j + 37 * ((r * nd) // wd)) % wd
        end = torch.where(r % 4 == 0, torch.full_like(r, wd - 1), torch.where(r % 4 == 1, torch.zeros_like(r), idx[..., 0]))
        idx = torch.cat([idx, end[..., None]], -1)
    return t * torch.zeros_like(t).scatter_(-1, idx, 1.0)


def _interior_rank(nimg, H, W_):
    """(rank of every pixel with the interior pixels of all images first, number of interior pixels)"""
    y, x = torch.arange(H)[:, None].expand(H, W_), torch.arange(W_)[None, :].expand(H, W_)
    inner = ((y >= 1) & (y <= H - 2) & (x >= 1) & (x <= W_ - 2)).reshape(1, -1).expand(nimg, -1).reshape(-1)
    order = torch.argsort((~inner).to(torch.int64), stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel())
    return rank, int(inner.sum())


def _x3_values(g, shape, every):
    """integers with 9 significant bits (257 .. 263, odd: bf16 hi = the even neighbour, lo = +-1) at one entry in `every`, small ones elsewhere"""
    small = _ints(g, shape, -3, 3)
    big = (257 + 2 * torch.randint(0, 4, shape, generator=g)).to(F64) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return torch.where(torch.randint(0, every, shape, generator=g) == 0, big, small)


def make_inputs(c, seed=0):
    """fp64 CPU tensors of a case: x0 / x1 / xt [B, H, W, C], w [S, N, K] in the kernel's K order (w3 [N, C, 3, 3] for ups = 2), bias / rowvec / res /
    slopes, and the scales of the fp8 forms.  All values are integers times powers of two."""
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, c["id"])))
    G = geom(c)
    B, H, W_, C0, C1, Cx, N = c["B"], c["H"], c["W"], c["C0"], c["C1"], c["Cx"], c["N"]
    nb = c["batch"]
    lead = (nb * B,)
    sixteen = c["out"] == "16"
    sparse = c["sparse"] if sixteen else None
    # (fp8 forms: the power-of-two scales of {1, 2} double an operand's extreme; fp8 activations are +-1 so that a 3x3 window still fits)
    a_hi = 1 if c["op"] == "a8" else c["a_hi"]
    w_hi = c["w_hi"]
    pmax = min(a_hi, 3) * (2 if c["op"] == "a8" else 1) * 3 * (2 if c["op"] in ("w8", "a8") else 1)
    nnz = (NNZ_STAT if (c["ln"] == "prod" or c["gn"]) else NNZ) * 9 // pmax
    i = dict()
    if c["op"] == "x3":
        i["x0"] = _x3_values(g, lead + (H, W_, C0), 16)
    else:
        i["x0"] = _ints(g, lead + (H, W_, C0), -a_hi, a_hi)
    i["x1"] = _ints(g, lead + (H, W_, C1), -c["a_hi"], c["a_hi"]) if C1 else None
    i["xt"] = _ints(g, lead + (G["Ho"], G["Wo"], Cx), -c["a_hi"], c["a_hi"]) if Cx else None
    S = (B if c["wps"] else 1) * nb
    if c["ups"] == 2:
        # natural 3x3 weights in +-{1}: every phase sum (1, 2 or 4 taps) stays a small integer, exact in 16 bits
        w3 = _ints(g, (N, C0, 3, 3), -1, 1)
        if sparse == "W":
            w3 = _keep(g, w3.reshape(N, -1), nnz // 3, cover=True).reshape(N, C0, 3, 3)
        i["w3"] = w3
        i["w"] = None
    else:
        w = _x3_values(g, (S, N, G["K"]), 1) if c["op"] == "x3" else _ints(g, (S, N, G["K"]), -w_hi, w_hi)
        if sparse == "W":
            w = _keep(g, w, nnz - 1, cover=True)
        if c["creal"]:
            # `creal` real channels stored in C0: the activation's pad channels stay NON-zero, the weight's pad columns are zero, as
            # ops.pack_conv_weight(cin_pad=) writes them -- a read that slips by a channel or a tap meets a live value
            assert C1 == 0 and Cx == 0 and c["korder"] == 0
            w = w.reshape(S, N, G["taps"], C0).clone()
            w[..., c["creal"]:] = 0
            w = w.reshape(S, N, G["K"])
        i["w"] = w
    if sparse == "A":
        # at most nnz non-zero A entries per GEMM row: per source pixel nnz / taps channels (window sources) resp. the rest (tail)
        per = max(1, (nnz - (3 if Cx else 0)) // G["taps"] - 1)
        rk = dict(zip(("rank", "first"), _interior_rank(nb * B, H, W_))) if G["taps"] > 1 and H > 2 and W_ > 2 else {}
        if C1:
            cat = _keep(g, torch.cat([i["x0"], i["x1"]], -1), per, cover=True, **rk)
            i["x0"], i["x1"] = cat[..., :C0].contiguous(), cat[..., C0:].contiguous()
        else:
            i["x0"] = _keep(g, i["x0"], per, cover=True, **rk)
        if Cx:
            i["xt"] = _keep(g, i["xt"], 2, cover=True)
    # fp8 forms: power-of-two scales, different per weight row and per (pixel, 32-channel block)
    if c["op"] in ("w8", "a8"):
        i["wscale"] = torch.tensor([1.0, 2.0], dtype=F64)[torch.randint(0, 2, (N,), generator=g)]
    if c["op"] == "a8":
        cp = (C0 + 127) // 128 * 128
        i["ascale_code"] = torch.randint(127, 129, lead + (H, W_, cp // 32), generator=g, dtype=torch.int64)          # E8M0: 2^(code - 127) in {1, 2}
    if c["gate_const"]:            # GEGLU with gate weights zero: the gate factor is gelu(bias) = bias at a saturated sigmoid
        w = i["w"].reshape(S, N // 64, 2, 32, G["K"])
        w[:, :, 1] = 0
        i["w"] = w.reshape(S, N, G["K"])
    i["bias"] = _ints(g, (N,), -7, 7) if c["bias"] else None
    if c["gn"] and sixteen:
        # statistics cases (alpha = 0.25, |out| <= 100): a bias of +-(58 .. 66) lifts the quarter-integers above 64, where bf16's 8 bits round
        # them -- the stored value then differs from the unrounded one, and the statistics must be those of the STORED value
        i["bias"] = (58 + torch.randint(0, 9, (N,), generator=g)).to(F64) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
    if c["gate_const"]:
        b = i["bias"].reshape(N // 64, 2, 32)
        b[:, 1] = torch.tensor([32.0, 64.0], dtype=F64)[torch.randint(0, 2, (N // 64, 32), generator=g)]
        i["bias"] = b.reshape(N)
    i["rowvec"] = _ints(g, (B, N), -7, 7) if c["rowvec"] else None
    i["res"] = _ints(g, (nb, G["M"], G["nout"]), -15, 15) if c["res"] else None
    i["slopes"] = torch.tensor([0.25, 0.5, 2.0, 1.0], dtype=F64)[torch.randint(0, 4, (N,), generator=g)] if c["act"] == ops.ACT_PRELU else None
    if c["a_exp"] or c["w_exp"] or c["e_exp"]:
        # the range knobs: every side times its power of two (exact in fp64; prepare() asserts that the 16-bit operands hold the result)
        assert c["op"] in ("bf16", "f16") and not c["gate_const"] and c["ln"] is None, c["id"]
        for keys, e in ((("x0", "x1", "xt"), c["a_exp"]), (("w", "w3"), c["w_exp"]), (("bias", "rowvec", "res"), c["e_exp"])):
            for k in keys:
                if i.get(k) is not None:
                    i[k] = i[k] * 2.0 ** e
    return i


def operand_values(c, i):
    """the real values the kernel multiplies: scales applied, split-bf16 left as it is"""
    x0, w = i["x0"], i["w"]
    if c["op"] == "a8":
        s = torch.pow(2.0, (i["ascale_code"] - 127).to(F64)).repeat_interleave(32, dim=-1)[..., :c["C0"]]
        x0 = x0 * s
    if c["op"] in ("w8", "a8") and w is not None:
        w = w * i["wscale"][None, :, None]
    return x0, w


def split_hi_lo(x):
    hi = x.float().to(torch.bfloat16).to(F64)
    lo = (x - hi).float().to(torch.bfloat16).to(F64)
    return hi, lo


# ------------------------------------------------------------------------------------------------ reference
MUTANTS = ("drop_last_k", "double_k_tile", "tap_transposed", "halo_from_adjacent_row", "pad_top_bottom_swapped", "phase_swapped", "phase00_padding",
           "concat_swapped", "tail_at_input_pixel", "korder_confused", "rowvec_neighbour", "residual_row_plus_1", "nsplit_bias_offset", "geglu_swapped",
           "wps_sample0", "stat_slot_plus_1", "stat_unrounded", "tile_permuted")
# slips of the window addressing (KH x KW taps, stride, pad_t / pad_l, the channel pitch of a tap, the K tail, a split-K slice's first tap)
WINDOW_MUTANTS = ("kh_kw_swapped", "pad_t_l_swapped", "stride_rows_only", "border_clamped", "cin_pad_ignored", "partial_tile_overread", "slice_start_tap")
MUTANTS = MUTANTS + WINDOW_MUTANTS


def slice_starts(c, sk):
    """first K tile of every split-K slice (gemm.hip: per = ceil(tiles / splitk), slice z starts at z per), and the tile count"""
    nk = -(-geom(c)["K"] // bk_of(c))
    per = -(-nk // sk)
    return [z * per for z in range(sk) if z * per < nk], nk


def tap_of_tile(c, ia):
    """the window tap K tile `ia` lies in (a window whose taps hold whole K tiles): tap-major K (korder 0) or chunk-major K (korder 1)"""
    ntap, tpt = c["kh"] * c["kw"], (c["C0"] + c["C1"]) // bk_of(c)
    return ia % ntap if c["korder"] else ia // tpt


def im2col(c, x0, x1, xt, mut=None, sk=1):
    """A [B Ho Wo, K] fp64 in the K order of c['korder']: k = tap * Ctot + ch (0), (chunk, tap, ch % BK) (1), (ky, chunk, kx, ch % BK) (2), then the
    tail source's channels at the output pixel.  ups: the window runs over the nearest-2x upsampled source.  The window is KH x KW, tap = ky KW + kx
    reads input pixel (oy stride - pad_t + ky, ox stride - pad_l + kx), zero outside the image (the bottom / right padding is whatever the output
    extent reaches: rf_conv_gemm is told pad_t and pad_l alone)."""
    G = geom(c)
    kh, kw, s = (3, 3, 1) if c["ups"] == 2 else (c["kh"], c["kw"], c["stride"])
    pt, pl, pb, pr = (1, 1, 1, 1) if c["ups"] == 2 else c["pad"]
    if mut == "pad_top_bottom_swapped":
        pt, pb = pb, pt
    if mut == "pad_t_l_swapped":
        pt, pl = pl, pt
    sx = 1 if mut == "stride_rows_only" else s
    src = x0 if x1 is None else (torch.cat([x1, x0], -1) if mut == "concat_swapped" else torch.cat([x0, x1], -1))
    if c["ups"]:
        src = src.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, Hs, Ws, ct = src.shape
    Ho, Wo = G["Ho"], G["Wo"]
    if mut == "halo_from_adjacent_row" and pl + pr > 0:
        # the row-extended tile read as a flat run of pixels: the left halo is the previous image row's last pixel, the right one the next row's first
        flat = F.pad(src.reshape(B, Hs * Ws, ct), (0, 0, pl, pr))
        rows = [flat[:, y * Ws:y * Ws + Ws + pl + pr] for y in range(Hs)]
        p = F.pad(torch.stack(rows, 1), (0, 0, 0, 0, pt, pb))
    elif mut == "border_clamped":
        # every tap outside the image reads the nearest pixel: replicate padding over all that the true window reaches
        bot, rgt = max(pb, (Ho - 1) * s + kh - pt - Hs), max(pr, (Wo - 1) * s + kw - pl - Ws)
        p = F.pad(src.permute(0, 3, 1, 2), (pl, max(0, rgt), pt, max(0, bot)), mode="replicate").permute(0, 2, 3, 1)
    else:
        p = F.pad(src, (0, 0, pl, pr, pt, pb))

    def tap(ky, kx):
        """window element (ky, kx) of every output pixel [B, Ho, Wo, Ctot]; zero beyond what is padded (also for a walk that leaves the window)"""
        need_h, need_w = ky + (Ho - 1) * s + 1, kx + (Wo - 1) * sx + 1
        q = F.pad(p, (0, 0, 0, max(0, need_w - p.shape[2]), 0, max(0, need_h - p.shape[1])))
        return q[:, ky:need_h:s, kx:need_w:sx]

    def coords(t):
        if mut == "kh_kw_swapped":
            return t // kh, t % kh
        return (t % kw, t // kw) if mut == "tap_transposed" else (t // kw, t % kw)
    ntap, M = kh * kw, B * Ho * Wo
    ko = c["korder"] if c["ups"] != 2 else 0
    if mut == "korder_confused" and ko:
        ko = 3 - ko
    bk = bk_of(c)
    if mut == "cin_pad_ignored" and c["creal"]:
        # k decoded as (tap, channel) with the REAL channel count as a tap's pitch
        cr = c["creal"]
        A = torch.stack([tap(*coords(t))[..., :cr] for t in range(-(-ntap * ct // cr))], 3).reshape(M, -1)[:, :ntap * ct]
    elif mut == "slice_start_tap" and sk > 1 and ko < 2 and ct % bk == 0:
        # every split-K slice but the first decodes its first tap as (tap / KH, tap % KH) and walks on from there as the kernel does
        starts, nk = slice_starts(c, sk)
        tpt, cols = ct // bk, []
        for z, t0 in enumerate(starts):
            t = tap_of_tile(c, t0)
            ic = t0 // ntap if ko else t0 - t * tpt
            ty, tx = (t // kh, t % kh) if z else (t // kw, t % kw)
            for _ in range(min(nk, starts[z + 1] if z + 1 < len(starts) else nk) - t0):
                cols.append(tap(ty, tx)[..., ic * bk:(ic + 1) * bk])
                if ko:
                    tx += 1
                    if tx == kw:
                        tx, ty = 0, ty + 1
                        if ty == kh:
                            ty, ic = 0, ic + 1
                else:
                    ic += 1
                    if ic == tpt:
                        ic, tx = 0, tx + 1
                        if tx == kw:
                            tx, ty = 0, ty + 1
        A = torch.cat(cols, -1).reshape(M, ntap * ct)
    else:
        n_walk = ntap
        over = mut == "partial_tile_overread" and xt is None and not ko
        if over:          # the walk goes on to the end of the last K tile: the taps behind the window
            n_walk = -(-(-(-ntap * ct // bk) * bk) // ct)
        T = torch.stack([tap(*coords(t)) for t in range(n_walk)], 3)                                   # [B, Ho, Wo, taps, Ctot]
        if ko:
            T = T.reshape(B, Ho, Wo, kh, kw, ct // bk, bk)
            T = T.permute(0, 1, 2, 5, 3, 4, 6) if ko == 1 else T.permute(0, 1, 2, 3, 5, 4, 6)
        A = T.reshape(M, n_walk * ct)[:, :-(-ntap * ct // bk) * bk if over else ntap * ct]
    if xt is not None:
        if mut == "tail_at_input_pixel":          # read at the window's first input pixel instead of the output pixel
            xt = torch.roll(xt, shifts=(pt, pl), dims=(1, 2))
        A = torch.cat([A, xt.reshape(B * Ho * Wo, -1)], 1)
    return A


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_sigmoid5(x):
    """the gate function GEGLU applies in the 16-bit operand modes, as csrc/common.h documents it: x sigmoid(g(x)) with the odd degree-5 argument
    g(x) = x (1.5950158 + 0.0740113 x^2 - 0.00070303 x^4), its argument clamped to |x| <= 7 (<= 2.6e-5 from the erf form; the fp32 mode keeps erf)"""
    xc = x.clamp(-7.0, 7.0)
    x2 = xc * xc
    return x * torch.sigmoid(xc * (1.5950158 + 0.0740113 * x2 - 0.00070303 * x2 * x2))


def gate_of(c):
    return gelu_erf if c["op"] == "f32" else gelu_sigmoid5


GATE_FORM_ERR = 2.6e-5          # csrc/common.h: the 16-bit modes' sigmoid-form GELU is at most this far from erf GELU, over the reals


def limit_of(c, ref):
    """the bound of the epilogues that are not exact: the fp32 rule of tests/test_ops_gpu.py, 2e-5 + 2e-5 |ref|, plus for a 16-bit output one storage
    half-step -- a storage step of bf16 is 2^-7 |ref| at most (8 significant bits), a round-to-nearest store costs up to half of it = STEP |ref|:
    the rule of tests/side_refs.limit_16"""
    odt = out_dtype(c)
    return 2e-5 + 2e-5 * ref.abs() + (STEP[odt] * ref.abs() if odt != torch.float32 else 0.0)


def epilogue(c, acc, i, mut=None, n_split=0):
    """out = act(alpha acc + bias + rowvec[sample]) + residual  (ADD_RELU: the ReLU comes after the residual), fp64 [M, nout]"""
    G = geom(c)
    M, N = acc.shape
    h = c["alpha"] * acc
    if c["ln"] == "cons":
        # LayerNorm consumer (reface_hip.h): out = act(rstd[m] (alpha acc - mean[m] u[n]) + bias[n]), mean / rstd of row m of the un-normalised A over
        # all its K columns, u[n] = sum_k W[n, k] -- the same thing as LayerNorm(A) W^T + bias
        A = i["x0"].reshape(M, -1).to(h.device)
        mean = A.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((A - mean) ** 2).mean(1, keepdim=True) + LN_EPS)
        h = rstd * (h - mean * i["w"][0].sum(1).to(h.device)[None])
    if i["bias"] is not None:
        b = i["bias"].to(h.device)
        if mut == "nsplit_bias_offset" and n_split:
            b = torch.cat([b[:n_split], b[:N - n_split]])
        h = h + b[None]
    if i["rowvec"] is not None:
        rv = i["rowvec"].to(h.device)
        if mut == "rowvec_neighbour":
            rv = torch.roll(rv, 1, 0)
        h = h + rv.repeat_interleave(G["rps"], 0)[:M]
    a = c["act"]
    res = i["res_cur"].to(h.device) if i.get("res_cur") is not None else None
    if res is not None and mut == "residual_row_plus_1":
        res = torch.roll(res, -1, 0)
    if a == ops.ACT_ADD_RELU:
        return torch.relu(h + res)
    if a == ops.ACT_GEGLU:
        hb = h.reshape(M, N // 64, 2, 32)
        v, gt = (hb[:, :, 1], hb[:, :, 0]) if mut == "geglu_swapped" else (hb[:, :, 0], hb[:, :, 1])
        if c["gate_const"] and mut != "geglu_swapped":
            # gate weights zero, gate = its bias of 32 or 64: sigmoid(g(7)) is 1 to eleven digits, so the fp32 factor is the bias itself, exactly
            assert bool((gt >= 32).all())
            h = (v * gt).reshape(M, N // 2)
        else:
            gate = {"gate_erf": gelu_erf, "gate_unit": torch.ones_like}.get(mut, gate_of(c))          # (gate_unit: the value half alone)
            h = (v * gate(gt)).reshape(M, N // 2)
    elif a == ops.ACT_SILU:
        h = h * torch.sigmoid(h)
    elif a == ops.ACT_QUICK_GELU:
        h = h * torch.sigmoid(1.702 * h)
    elif a == ops.ACT_GELU:
        h = gelu_erf(h)
    elif a == ops.ACT_RELU:
        h = torch.relu(h)
    elif a == ops.ACT_SIGMOID:
        h = torch.sigmoid(h)
    elif a == ops.ACT_PRELU:
        h = torch.where(h >= 0, h, h * i["slopes"].to(h.device)[None])
    if res is not None:
        h = h + res
    return h


def contract(c, A, w, mut=None, sk=1):
    """acc [M, N] = A W^T in fp64.  w [S, N, K]: S > 1 = per-sample weights.  split-bf16: hi hi + hi lo + lo hi."""
    G = geom(c)
    K = A.shape[1]
    if mut == "drop_last_k":
        A = A.clone()
        A[:, K - 1] = 0
    if mut == "double_k_tile" and sk > 1:          # the K tile at the first split-K slice boundary counted by both slices
        bk = bk_of(c)
        k0 = ((K // bk + sk - 1) // sk) * bk
        A, w = torch.cat([A, A[:, k0:k0 + bk]], 1), torch.cat([w, w[:, :, k0:k0 + bk]], 2)
    if mut == "partial_tile_overread" and K > w.shape[2]:
        # A runs on to the end of its last K tile (im2col); so does the weight row, into the start of the row behind it (the last row: into row 0)
        w = torch.cat([w, torch.roll(w, -1, 1)[:, :, :K - w.shape[2]]], 2)
    def mm(a, b):
        if c["op"] == "x3":
            ah, al = split_hi_lo(a)
            bh, bl = split_hi_lo(b)
            return ah @ bh.T + ah @ bl.T + al @ bh.T
        return a @ b.T
    if w.shape[0] == 1:
        return mm(A, w[0])
    rps = G["rps"]
    return torch.cat([mm(A[s * rps:(s + 1) * rps], w[0 if mut == "wps_sample0" else s]) for s in range(w.shape[0])], 0)


def ups2_folded(c, x0, w3, mut=None):
    """the FOLDED statement of ups = 2 (reface_hip.h): output pixel (2i + py, 2j + px) = the 2x2 window of the stored source at (i - 1 + py + ty,
    j - 1 + px + tx) on the phase weights.  Equals the unfolded reference (CPU file); its two mutants are the phase slips."""
    wf = ops.fold_ups_weight(w3)                               # [4, N, 2, 2, C] fp64
    B, H, W_, C0 = x0.shape
    N = w3.shape[0]
    out = torch.zeros((B, 2 * H, 2 * W_, N), dtype=F64)
    p = F.pad(x0, (0, 0, 1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            wy, wx = (px, py) if mut == "phase_swapped" else (py, px)
            oy, ox = (0, 0) if mut == "phase00_padding" else (py, px)
            acc = 0
            for ty in range(2):
                for tx in range(2):
                    acc = acc + p[:, oy + ty:oy + ty + H, ox + tx:ox + tx + W_] @ wf[2 * wy + wx, :, ty, tx].T
            out[:, py::2, px::2] = acc
    return out.reshape(B * 4 * H * W_, N)


def reference(c, i, mut=None, dev="cpu", sk=1, n_split=0):
    """expected output(s) of a case in fp64: [batch, M, nout] (before any storage rounding)"""
    G = geom(c)
    x0v, wv = operand_values(c, i)
    outs = []
    nb, B = c["batch"], c["B"]
    S = B if c["wps"] else 1
    for b in range(nb):
        sl = slice(b * B, (b + 1) * B)
        x0 = x0v[sl].to(dev)
        x1 = i["x1"][sl].to(dev) if i["x1"] is not None else None
        xt = i["xt"][sl].to(dev) if i["xt"] is not None else None
        if c["ups"] == 2:
            if mut in ("phase_swapped", "phase00_padding"):
                acc = ups2_folded(c, x0.cpu(), i["w3"], mut).to(dev)
            else:
                w = i["w3"].permute(0, 2, 3, 1).reshape(1, c["N"], 9 * c["C0"]).to(dev)
                acc = contract(c, im2col(c, x0, None, None, mut), w, mut, sk)
        else:
            acc = contract(c, im2col(c, x0, x1, xt, mut, sk), wv[b * S:(b + 1) * S].to(dev), mut, sk)
        i["res_cur"] = i["res"][b] if i["res"] is not None else None
        outs.append(epilogue(c, acc, i, mut, n_split))
    return torch.stack(outs, 0)


def steer_stripe_means(c, i, ref, wc):
    """LayerNorm producer: add to the residual's last column of every stripe of `wc` columns what makes the stripe's sum a multiple of wc (an
    integer mean); returns the new reference"""
    nb, M, N = ref.shape
    r = ref.reshape(nb, M, N // wc, wc)
    s = r.sum(-1)
    d = -(torch.remainder(s + wc // 2, wc) - wc // 2)
    i["res"] = i["res"].reshape(nb, M, N // wc, wc).clone()
    i["res"][..., -1] += d
    i["res"] = i["res"].reshape(nb, M, N)
    r = r.clone()
    r[..., -1] += d
    return r.reshape(nb, M, N)


def ln_records(stored, wc):
    """(mean, M2) per row and stripe of wc columns of the stored values, fp64 [M, N / wc, 2]"""
    M, N = stored.shape
    r = stored.reshape(M, N // wc, wc)
    mean = r.mean(-1)
    return torch.stack([mean, ((r - mean[..., None]) ** 2).sum(-1)], -1)


def gn_expected(stored, c, st_rows, st_cols, cpg, coff, mut_unrounded=None):
    """fp64 [B, slots, 32, 2] (sum, sumsq) of the values as stored, slot = (row tile within the sample) * column tiles + column tile; a group a tile
    does not touch gets (0, 0) in that tile's slot"""
    G = geom(c)
    src = stored if mut_unrounded is None else mut_unrounded
    M, N = src.shape
    rps = G["rps"]
    nct, nrt = (N + st_cols - 1) // st_cols, rps // st_rows
    out = torch.zeros((M // rps, nrt * nct, 32, 2), dtype=F64)
    grp = (coff + torch.arange(N)) // cpg
    assert int(grp.max()) < 32
    src = src.cpu()
    for b in range(M // rps):
        for rt in range(nrt):
            rows = src[b * rps + rt * st_rows:b * rps + (rt + 1) * st_rows]
            both = torch.stack([rows.sum(0), (rows * rows).sum(0)], -1)                 # [N, 2]
            for ct in range(nct):
                sl = slice(ct * st_cols, min(N, (ct + 1) * st_cols))
                out[b, rt * nct + ct].index_add_(0, grp[sl], both[sl])
    return out


# ------------------------------------------------------------------------------------------------ bounds (asserted before any launch)
def unit_of(c, i):
    """the power of two every operand product, epilogue term and partial sum is a multiple of"""
    u = 1.0
    if c["act"] == ops.ACT_PRELU:
        u *= 0.25
    u *= min(1.0, c["alpha"])
    # (the range knobs: products are multiples of 2^(a_exp + w_exp) units, epilogue terms of 2^e_exp; 1.0 = min(1.0, 1.0) at the defaults)
    return min(u * 2.0 ** (c["a_exp"] + c["w_exp"]), u * 2.0 ** c["e_exp"])


def magnitude_bound(c, i):
    """an upper bound of |any partial sum|, in any summation order: alpha * sum_k |A| |W| + |bias| + |rowvec| + |residual| (times the largest
    PReLU slope), from the operands' own extremes -- no product is evaluated"""
    G = geom(c)
    x0v, wv = operand_values(c, i)
    pix = x0v.abs().sum(-1).max().item() + (i["x1"].abs().sum(-1).max().item() if i["x1"] is not None else 0.0)
    if c["ups"] == 2:
        a_l1, wmax = 9 * pix, i["w3"].abs().max().item()
        w_l1 = i["w3"].abs().reshape(c["N"], -1).sum(-1).max().item()
    else:
        a_l1, wmax = G["taps"] * pix, wv.abs().max().item()
        w_l1 = wv.abs().sum(-1).max().item()
    amax = x0v.abs().max().item()
    if i["xt"] is not None:
        a_l1 += i["xt"].abs().sum(-1).max().item()
        amax = max(amax, i["xt"].abs().max().item())
    if i["x1"] is not None:
        amax = max(amax, i["x1"].abs().max().item())
    acc = min(a_l1 * wmax, w_l1 * amax) * (1.0 if c["op"] != "x3" else 1.02)
    epi = sum(t.abs().max().item() for t in (i["bias"], i["rowvec"], i["res"]) if t is not None)
    return (abs(c["alpha"]) * acc + epi) * (2.0 if c["act"] == ops.ACT_PRELU else 1.0), acc


def is_exact(c):
    """False for the epilogues held to a tolerance: SiLU, the GELUs, sigmoid, GEGLU's gate, the LayerNorm consumer's rstd"""
    return not (c["act"] in INEXACT_ACTS or (c["act"] == ops.ACT_GEGLU and not c["gate_const"]) or c["ln"] == "cons")


def assert_exact(c, i, ref):
    """the issue's generator bounds: partial sums below 2^24 units; 16-bit outputs of the exact epilogues representable (|out| <= 255); statistics
    cases |out| <= 128 and at most 256 rows per statistics tile (BM <= 256 by construction)"""
    bound, acc = magnitude_bound(c, i)
    assert bound / unit_of(c, i) < EXACT_LIMIT, (c["id"], bound)
    if not is_exact(c):
        return                                                 # tolerance-checked epilogue: only the pre-activation is exact
    assert torch.equal(ref, ref.float().to(F64)), c["id"]
    if c["range16"]:
        # the range switch: the expected 16-bit output is Tensor.to(dtype) of the exactly known fp32 value (asserted above), whatever its size.  Every
        # epilogue term is a multiple of the unit (a steered bias included), and a statistics case stores only subnormal-band values: multiples of
        # 2^-24 whose squares, in units of 2^-48, sum below 2^24 per statistics tile
        u = unit_of(c, i)
        for t in (i["bias"], i["rowvec"], i["res"]):
            assert t is None or torch.equal((t / u).round() * u, t), c["id"]
        if c["gn"]:
            st_rows = 32 if c["ws"] else c["expect"]["bm"]
            st = ref[0].float().to(out_dtype(c)).to(F64)
            assert out_dtype(c) == torch.float16 and st.abs().max().item() < 2.0 ** -14 and st_rows <= 256, (
                f"{c['id']}: a range16 statistics case must store fp16 values below 2^-14 only (multiples of 2^-24: the unit the exactness of the "
                f"fp32 column sums is argued in); largest stored |value| {st.abs().max().item()}, {st_rows} rows per statistics tile")
            sq = (st * st).reshape(-1, st_rows, st.shape[-1]).sum(1).max().item()
            assert sq * 2.0 ** 48 < EXACT_LIMIT, (c["id"], sq)
        return
    if c["out"] == "16":
        dt = out_dtype(c)
        if c["gn"]:
            # (alpha = 0.25: the stored value is the RNE of the exact one.)  |out| <= 128; the fp32 column sums of a statistics tile are exact when
            # the tile's sum of squares stays below 2^24 units of (1/4)^2 -- squares are non-negative, so every partial sum is below the total
            assert ref.abs().max().item() <= 128, (c["id"], ref.abs().max().item())
            st_rows = 32 if c["ws"] else c["expect"]["bm"]
            st = ref[0].to(dt).to(F64)
            sq = (st * st).reshape(-1, st_rows, st.shape[-1]).sum(1).max().item()
            assert st_rows <= 256 and sq * 16 < EXACT_LIMIT and torch.equal(st * 4, (st * 4).round()), (c["id"], sq)
        else:
            assert ref.abs().max().item() <= 255 * (64.0 if c["gate_const"] else 1.0), (c["id"], ref.abs().max().item())
            assert torch.equal(ref.to(dt).to(F64), ref), f"{c['id']}: an expected output is not representable in {dt}"


def k_coverage(c, i):
    """True where column k of the contraction carries a non-zero product in some row (this seed)"""
    A = im2col(c, operand_values(c, i)[0][:c["B"]], i["x1"][:c["B"]] if i["x1"] is not None else None, i["xt"][:c["B"]] if i["xt"] is not None else None)
    w = i["w"][0] if i["w"] is not None else i["w3"].permute(0, 2, 3, 1).reshape(c["N"], -1)
    return (A != 0).any(0) & (w != 0).any(0)


# ------------------------------------------------------------------------------------------------ launches (any device: a plan query needs no GPU)
def _sentinel(shape, dt, dev):
    return torch.full(shape, float("nan"), dtype=dt, device=dev)


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


class Guarded:
    """a region inside a larger sentinel-filled allocation: `view` is what the kernel gets, check() proves the rest untouched"""

    def __init__(self, buf, view, mask):
        self.buf, self.view, self.mask, self.before = buf, view, mask, buf.clone()

    def check(self, what):
        same = _bits(self.buf) == _bits(self.before)
        assert bool(same[~self.mask].all()), f"{what}: wrote outside its region ({int((~same[~self.mask]).sum())} elements changed)"


def guarded_rows(rows, cols, ld, col0, dt, dev, nb=1):
    """nb blocks of [rows, cols] at column col0 of a [.., ld] buffer, GUARD rows in front, between and behind"""
    R = GUARD + nb * (rows + GUARD)
    buf = _sentinel((R, ld), dt, dev)
    mask = torch.zeros((R, ld), dtype=torch.bool, device=dev)
    views = []
    for b in range(nb):
        r0 = GUARD + b * (rows + GUARD)
        mask[r0:r0 + rows, col0:col0 + cols] = True
        views.append(buf[r0:r0 + rows, col0:col0 + cols])
    g = Guarded(buf, views[0], mask)
    g.views, g.block_stride = views, (rows + GUARD) * ld
    return g


def guarded_flat(n, dt, dev):
    buf = _sentinel((n + 2 * GUARD,), dt, dev)
    mask = torch.zeros((n + 2 * GUARD,), dtype=torch.bool, device=dev)
    mask[GUARD:GUARD + n] = True
    return Guarded(buf, buf[GUARD:GUARD + n], mask)


def _fp8_bytes(t):
    q = t.float().to(torch.float8_e4m3fn)
    assert torch.equal(q.float().to(F64), t), "not an e4m3 value"
    return q.view(torch.uint8)


def prepare(c, i, dev):
    """the rf_conv_gemm launch of a case on `dev`, every written region guarded.  Returns a dict: launch, out (Guarded), ws / gn0 / gn1 / ln
    (Guarded or None).  The LayerNorm / GroupNorm fields are wired by wire_stats once the plan is known."""
    G = geom(c)
    op, B, H, W_, C0, C1, Cx, N = c["op"], c["B"], c["H"], c["W"], c["C0"], c["C1"], c["Cx"], c["N"]
    nb, M, K, nout = c["batch"], G["M"], G["K"], G["nout"]
    odt = out_dtype(c)
    x3 = op == "x3"
    if op == "a8":
        a = ops.Fp8Act((nb * B, H, W_, C0), dev)
        a.q[..., :C0] = _fp8_bytes(i["x0"]).to(dev)
        a.scale[...] = i["ascale_code"].to(torch.uint8).to(dev)
        src0, cp = a, a.Cp
        wpad = torch.zeros((N, G["taps"], cp), dtype=F64)
        wpad[..., :C0] = i["w"][0].reshape(N, G["taps"], C0)
        Wt = ops.Fp8Weight(_fp8_bytes(wpad.reshape(N, G["taps"] * cp)).contiguous().to(dev), i["wscale"].float().to(dev), G["taps"] * cp)
        C0k, Kk, ld0 = cp, G["taps"] * cp, cp
    else:
        dt = TDT[op]
        if x3:
            hi, lo = split_hi_lo(i["x0"])
            src0 = torch.cat([hi, lo], -1).to(dt).to(dev)
        else:
            src0 = i["x0"].to(dt).to(dev)
            assert torch.equal(src0.cpu().to(F64), i["x0"])
        C0k, Kk, ld0 = C0, K, src0.shape[-1]
        if c["ups"] == 2:
            wf = ops.fold_ups_weight(i["w3"])                                        # fp64, exact: [4, N, 2, 2, C]
            assert torch.equal(wf.to(dt).to(F64), wf), "phase sums not exact in 16 bits"
            if c["korder"] == 1:
                wf = wf.reshape(4, N, 4, C0 // 64, 64).permute(0, 1, 3, 2, 4)
            Wt = wf.reshape(4, N, 4 * C0).to(dt).contiguous().to(dev)
        elif op == "w8":
            ldq = (K + 127) // 128 * 128
            q = torch.zeros((N, ldq), dtype=torch.uint8)
            q[:, :K] = _fp8_bytes(i["w"][0])
            Wt = ops.Fp8Weight(q.to(dev), i["wscale"].float().to(dev), K)
        elif x3:
            Wt = ops.pack_x3(i["w"][0].float()).to(dev)
        else:
            Wt = i["w"].to(dt).to(dev).contiguous()
            assert torch.equal(Wt.cpu().to(F64), i["w"])
            Wt = Wt if (c["wps"] or nb > 1) else Wt[0]
    src1 = i["x1"].to(TDT[op]).to(dev) if C1 else None
    srcx = i["xt"].to(TDT[op]).to(dev) if Cx else None
    f32 = lambda t: None if t is None else t.float().to(dev).contiguous()
    bias, rowvec, slopes = f32(i["bias"]), f32(i["rowvec"]), f32(i["slopes"])
    res = None
    if c["res"]:          # the residual is a column slice too: 16 more columns per row behind it
        res = torch.zeros((nb, M, nout + 16), dtype=odt, device=dev)
        res[..., :nout] = i["res"].to(odt).to(dev)
        assert not c["range16"] or torch.equal(res[..., :nout].cpu().to(F64), i["res"]), f"{c['id']}: a residual value is not representable in {odt}"
        res = res[..., :nout]
    ldo = c["col0"] + nout + c["ldo_extra"]
    out = guarded_rows(M, nout, ldo, c["col0"], odt, dev, nb)
    ws = guarded_flat(c["ws"] // 4, torch.float32, dev) if c["ws"] else None
    conv = not (c["kh"] == 1 and c["kw"] == 1 and c["stride"] == 1 and c["ups"] == 0 and C1 == 0 and c["pad"] == (0, 0, 0, 0))
    kw = dict(M=M, N=N, K=Kk, C0=C0k, ld0=ld0, src1=src1, C1=C1, ld1=C1, bias=bias, rowvec=rowvec, rows_per_sample=G["rps"], ldv=N if c["rowvec"] else 0,
              residual=res, ldr=nout + 16 if c["res"] else 0, act=c["act"], ldo=ldo, alpha=c["alpha"], act_vec=slopes, korder=c["korder"],
              workspace=ws.view if ws else None, x3=x3, srcx=srcx, Cx=Cx, ldx=Cx, name=c["id"])
    if conv:
        if c["ups"] == 2:
            kw.update(Hin=H, Win=W_, Hout=2 * H, Wout=2 * W_, KH=2, KW=2, stride=1, pad_t=1, pad_l=1, ups=2, M=4 * B * H * W_, K=4 * C0, rows_per_sample=4 * H * W_)
        else:
            kw.update(Hin=H, Win=W_, Hout=G["Ho"], Wout=G["Wo"], KH=c["kh"], KW=c["kw"], stride=c["stride"], pad_t=c["pad"][0], pad_l=c["pad"][1], ups=c["ups"])
    else:
        kw.update(Hin=1, Win=M, Hout=1, Wout=M)
    if nb > 1:
        kw.update(batch=nb, sA=B * H * W_ * ld0, sW=N * K, sO=out.block_stride, sR=M * (nout + 16))
    l = ops.conv_gemm(src0, Wt, out.view, **kw)
    d = l.keep[0]
    if not c["ws"]:
        d.workspace, d.workspace_bytes = None, 0
    if c["wps"]:
        d.w_sample_stride = N * K
    return dict(launch=l, out=out, ws=ws, gn=[None, None], ln=None, keep=(src0, Wt, src1, srcx, bias, rowvec, slopes, res))


def gn_consumers(c):
    """(cpg, coff) of the two GroupNorm consumers a statistics case feeds: the tensor itself, and a concat buffer that holds it from channel 64 on"""
    N = geom(c)["nout"]
    return ((N // 32, 0), ((N + 64) // 32, 64))


def wire_stats(c, P, pl, dev, i=None):
    """point the launch at guarded statistics buffers, sized by the plan: GroupNorm partial sums at slot 1 of need + 2 slots, LayerNorm records"""
    G, d = geom(c), P["launch"].keep[0]
    if c["gn"]:
        need = (G["rps"] // pl["stat_rows"]) * ((c["N"] + pl["stat_cols"] - 1) // pl["stat_cols"])
        d.gn_rows = G["rps"]
        for k, (cpg, coff) in enumerate(gn_consumers(c)):
            buf = _sentinel((c["B"], need + 2, 32, 2), F64, dev)
            mask = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
            mask[:, 1:1 + need] = True
            P["gn"][k] = Guarded(buf, buf[:, 1:1 + need], mask)
            for f, v in (("part", buf.data_ptr()), ("cpg", cpg), ("coff", coff), ("slot", 1), ("nchunks", need + 2)):
                setattr(d, f"gn_{f}{k}", v)
    if c["ln"] == "cons":
        # the records a producer with 64-column stripes would have left: (mean, M2) per row and part, exact in fp32 (means are multiples of 1 / 64)
        A = i["x0"].reshape(G["M"], -1)
        rec = ln_records(A, LN_IN_COLS)
        assert torch.equal(rec.float().to(F64), rec)
        P["keep"] += (rec.float().to(dev).contiguous(), i["w"][0].sum(1).float().to(dev).contiguous())
        d.ln_stats_in, d.ln_in_parts, d.ln_in_cols, d.ln_eps, d.ln_u = P["keep"][-2].data_ptr(), rec.shape[1], LN_IN_COLS, LN_EPS, P["keep"][-1].data_ptr()
    if c["ln"] == "prod":
        parts = c["N"] // pl["wave_cols"]
        P["ln"] = guarded_flat(G["M"] * parts * 2, torch.float32, dev)
        d.ln_stats_out, d.ln_out_parts = P["ln"].view.data_ptr(), parts


def plan_matches(pl, expect):
    """the plan words a case names, against the plan the library reports: list of mismatches"""
    return [f"{k}: expected {v}, plan says {pl.get(k)}" for k, v in expect.items() if pl.get(k) != v]


# ------------------------------------------------------------------------------------------------ the case table
A_, G_, P_ = ops.ACT_NONE, ops.ACT_GEGLU, ops.ACT_PRELU
MB = 1 << 20


def _t(bm, bn, waves, **kw):
    return dict(bm=bm, bn=bn, waves=waves, **kw)


CASES = []
P3 = (1, 1, 1, 1)
W64 = 64 * MB
_X = CASES.append
AR, RL, SI, QG, GE, SG = ops.ACT_ADD_RELU, ops.ACT_RELU, ops.ACT_SILU, ops.ACT_QUICK_GELU, ops.ACT_GELU, ops.ACT_SIGMOID

# ---- bf16 tiles: every instantiation launch_cfg can launch, direct and staged where both exist (shapes found by querying the plan)
_X(case("t256x320-direct", ["tile 256x320", "epilogue direct", "loop linear direct-to-LDS", "fp32 output", "edge ragged M", "edge pitched column slice"],
        _t(256, 320, 8, direct=1, splitk=1, stages=2, glds=1, conv=0), W=49000, C0=384, N=320, res=True, alpha=2.0,
        small=dict(W=300)))          # (K > 320: a K <= 320 launch with a residual goes to 128x160 tiles)
_X(case("t256x320-staged-rps", ["tile 256x320", "epilogue staged", "staged forced by rows_per_sample % BM", "16-bit output", "edge tile spans a sample boundary"],
        _t(256, 320, 8, direct=0, splitk=1), B=49, W=1000, N=320, rowvec=True, out="16", small=dict(B=3, W=200)))
_X(case("t256x256-direct", ["tile 256x256", "epilogue direct", "16-bit output", "edge ragged M"], _t(256, 256, 8, direct=1, splitk=1), W=49000, N=256, res=True,
        out="16", sparse="A", small=dict(W=300)))
_X(case("t256x256-staged-prelu", ["tile 256x256", "epilogue staged", "PReLU"], _t(256, 256, 8, direct=0, splitk=1), W=49000, N=256, act=P_, small=dict(W=300)))
_X(case("t128x320-direct", ["tile 128x320", "epilogue direct"], _t(128, 320, 8, direct=1, splitk=1), W=6144, C0=6016, N=1280, small=dict(W=300, C0=128, N=320)))
_X(case("t128x320-staged", ["tile 128x320", "epilogue staged", "edge ragged M"], _t(128, 320, 8, direct=0, splitk=1), W=6100, C0=6016, N=1280, act=RL,
        small=dict(W=300, C0=128, N=320)))
_X(case("t128x256-direct-addrelu", ["tile 128x256", "epilogue direct", "ADD_RELU", "16-bit output", "edge ragged M"], _t(128, 256, 8, direct=1, splitk=1),
        W=6200, N=1024, act=AR, res=True, out="16", small=dict(W=300)))
_X(case("t128x256-staged-prelu", ["tile 128x256", "epilogue staged", "PReLU", "16-bit output"], _t(128, 256, 8, direct=0, splitk=1), W=6200, N=1024, act=P_,
        out="16", sparse="A", small=dict(W=300)))
_X(case("t128x160-2stage-direct", ["tile 128x160 two stages", "epilogue direct", "edge ragged M"], _t(128, 160, 4, direct=1, stages=2, splitk=1), W=16600, N=304,
        res=True, small=dict(W=300)))
_X(case("t128x160-2stage-staged", ["tile 128x160 two stages", "epilogue staged", "16-bit output"], _t(128, 160, 4, direct=0, stages=2, splitk=1), W=16600, N=304,
        act=RL, out="16", small=dict(W=300)))
_X(case("t128x160-ring-direct", ["tile 128x160 ring (<= 256 blocks)", "epilogue direct", "edge ragged N"], _t(128, 160, 4, direct=1, stages=4, splitk=1), W=200, N=144,
        res=True))
_X(case("t128x160-ring-staged", ["tile 128x160 ring (<= 256 blocks)", "epilogue staged", "edge ragged N"], _t(128, 160, 4, direct=0, stages=4, splitk=1), W=200, N=152,
        res=True, out="16"))
_X(case("t128x128", ["tile 128x128", "edge ragged N", "edge tile spans a sample boundary"], _t(128, 128, 4, direct=0, splitk=1), B=2, W=100, N=100, rowvec=True,
        res=True, col0=4, ldo_extra=4))
_X(case("t128x64", ["tile 128x64", "edge ragged N", "16-bit output"], _t(128, 64, 4, direct=0, splitk=1), W=200, N=40, res=True, out="16"))
# ---- loops
_X(case("conv-k0", ["loop conv direct-to-LDS korder 0", "edge tile spans a sample boundary"], _t(128, 128, 4, glds=1, conv=1, hx=0), B=2, H=9, W=9, C0=64, N=100,
        ks=3, pad=P3, rowvec=True, res=True))
_X(case("conv-k1", ["loop conv direct-to-LDS korder 1"], _t(128, 128, 4, glds=1, conv=1, hx=0), B=3, H=9, W=9, C0=128, N=112, ks=3, pad=P3, korder=1, out="16",
        sparse="A"))
for _s in ("W", "A"):
    _X(case(f"hx-4wave-{_s}", ["loop row-extended korder 2", "16-bit output", "edge tile spans a sample boundary"], _t(128, 128, 4, glds=1, conv=1, hx=1), B=5, H=4,
            W=16, C0=128, N=112, ks=3, pad=P3, korder=2, out="16", sparse=_s, rowvec=True, res=True))
_X(case("hx-8wave", ["loop row-extended korder 2", "tile 128x256"], _t(128, 256, 8, glds=1, conv=1, hx=1, direct=1), B=6, H=32, W=32, C0=128, N=1024, ks=3, pad=P3,
        korder=2, out="16", sparse="A", small=dict(B=2, H=16, W=16, N=128)))
_X(case("conv-regs-concat", ["loop conv through registers: C1 concat"], _t(128, 128, 4, glds=0, conv=1), B=2, H=9, W=9, C0=40, C1=24, N=100, ks=3, pad=P3, res=True))
_X(case("conv-regs-cin16", ["loop conv through registers: Cin = 16"], _t(128, 64, 4, glds=0, conv=1), B=2, H=9, W=9, C0=16, N=40, ks=3, pad=P3, out="16"))
_X(case("linear-regs-k136", ["loop linear through registers: K % 64 != 0"], _t(128, 128, 4, glds=0, conv=0), W=200, C0=136, N=100, res=True))
_X(case("ups1", ["loop ups 1"], _t(128, 128, 4, glds=1, conv=1), B=2, H=5, W=5, C0=64, N=100, ks=3, pad=P3, ups=1))
for _s in ("W", "A"):
    _X(case(f"ups2-4wave-{_s}", ["loop ups 2 (four phases, borders, several samples)", "16-bit output"], _t(128, 128, 4, glds=1, conv=1, splitk=1), B=3, H=16, W=8,
            C0=64, N=112, ups=2, ks=3, pad=P3, out="16", sparse=_s))
_X(case("ups2-k1-ring", ["loop ups 2 (four phases, borders, several samples)", "fp32 output"], _t(128, 160, 4, glds=1, conv=1, direct=1), B=2, H=8, W=16, C0=128,
        N=144, ups=2, ks=3, pad=P3, korder=1))
_X(case("ups2-8wave", ["loop ups 2 (four phases, borders, several samples)", "tile 256x256"], _t(256, 256, 8, glds=1, conv=1, direct=1), B=3, H=64, W=32, C0=64,
        N=1024, ups=2, ks=3, pad=P3, out="16", sparse="A", small=dict(B=2, H=16, W=8, N=128)))
_X(case("stride2-asym-pad", ["loop stride 2 with asymmetric padding"], _t(128, 128, 4, glds=1, conv=1), B=3, H=9, W=11, C0=64, N=100, ks=3, stride=2, pad=(0, 0, 1, 1)))
_X(case("tail-k0", ["loop srcx tail"], _t(128, 128, 4, glds=1, conv=1), B=2, H=9, W=9, C0=64, Cx=64, N=100, ks=3, pad=P3, res=True))
_X(case("tail-k1", ["loop srcx tail"], _t(128, 128, 4, glds=1, conv=1), B=3, H=9, W=9, C0=128, Cx=128, N=112, ks=3, pad=P3, korder=1, out="16", sparse="A"))
_X(case("per-sample-w", ["loop per-sample W"], _t(128, 128, 4, glds=1, conv=0), B=3, W=128, C0=64, N=112, wps=True, rowvec=True))
_X(case("batch3", ["loop batch > 1"], _t(128, 128, 4, conv=0), W=100, C0=64, N=100, batch=3, res=True))
# ---- LayerNorm producer records and fused GroupNorm statistics (direct and staged epilogue)
_X(case("ln-producer-ring", ["ln_stats_out records", "16-bit output"], _t(128, 160, 4, direct=1, ln_role=1), W=200, N=320, out="16", res=True, ln="prod"))
_X(case("ln-producer-256x320", ["ln_stats_out records", "tile 256x320"], _t(256, 320, 8, direct=1, ln_role=1), W=49000, C0=384, N=320, out="16", res=True, ln="prod",
        sparse="A", small=dict(W=300)))
_X(case("ln-consumer-ring", ["ln_stats_in consumer", "tolerance-checked epilogue"], _t(128, 160, 4, direct=1, ln_role=2), W=200, C0=128, N=304, out="16", ln="cons",
        sparse="none"))
_X(case("ln-consumer-8wave-geglu", ["ln_stats_in consumer", "tolerance-checked epilogue", "GEGLU"], _t(128, 256, 8, direct=1, ln_role=2), W=6200, C0=128, N=1024,
        out="16", ln="cons", act=G_, alpha=1.0, sparse="none", small=dict(W=300)))
_X(case("gn-direct-8wave", ["fused GroupNorm statistics, direct epilogue"], _t(128, 256, 8, direct=1, splitk=1), B=25, H=16, W=16, N=1024, out="16", gn=True,
        alpha=0.25, rowvec=True, small=dict(B=2, N=256)))
_X(case("gn-staged-4wave", ["fused GroupNorm statistics, staged epilogue"], _t(128, 128, 4, direct=0, splitk=1), B=3, H=8, W=16, N=96, out="16", gn=True, alpha=0.25,
        rowvec=True))
# ---- split-K
_X(case("sk-stripe8", ["split-K 8-row stripe reduce"], _t(128, 128, 4, reduce="stripe8"), B=4, H=8, W=8, C0=128, N=112, ks=3, pad=P3, ws=MB, rowvec=True, res=True,
        out="16"))
_X(case("sk-stripe32", ["split-K 32-row stripe reduce", "tile 128x320"], _t(128, 320, 8, reduce="stripe32"), W=3840, C0=2048, N=1280, act=RL, ws=W64,
        small=dict(W=300, C0=1024, N=320, ws=MB)))
_X(case("sk-frag-m-below-bm", ["split-K fragment slabs, M < BM"], _t(128, 160, 4, reduce="frag"), B=1, H=8, W=8, C0=256, N=304, ks=3, pad=P3, ws=4 * MB, res=True))
_X(case("sk-frag-gn", ["split-K fragment slabs with fused statistics", "tile 128x320"], _t(128, 320, 8, reduce="frag"), B=8, H=16, W=16, C0=192, N=1280, ks=3, pad=P3,
        ws=W64, gn=True, out="16", alpha=0.25, small=dict(B=2, C0=64, N=320, ws=4 * MB)))
_X(case("sk-256x320", ["split-K fragment slabs", "tile 256x320"], _t(256, 320, 8, reduce="frag"), W=8000, C0=2048, N=640, ws=W64, res=True,
        small=dict(W=300, C0=1024, N=320, ws=4 * MB)))
_X(case("sk-256x256", ["split-K fragment slabs", "tile 256x256"], _t(256, 256, 8, reduce="frag"), W=4096, C0=2048, N=1024, ws=W64, out="16",
        small=dict(W=300, C0=1024, N=256, ws=4 * MB)))
# ---- dispatch specials
_X(case("nsplit", ["two-kernel N split (bias, rowvec, residual offsets in the tail)"], _t(256, 256, 8, gemm_kernels=2, tail=(128, 256, 8, 1), split_n=4096), B=4,
        W=1024, N=5632, rowvec=True, res=True, small=dict(W=64, N=384)))
_X(case("nsplit-geglu", ["two-kernel N split (bias, rowvec, residual offsets in the tail)", "GEGLU exact gate"], _t(256, 256, 8, gemm_kernels=2, split_n=4096),
        W=4096, N=5632, act=G_, gate_const=True, out="16", small=dict(W=200, N=384)))
_X(case("patch-order", ["pm > 1 and pn < tiles_n"], _t(256, 320, 8, pm=4, pn=8, tiles_n=16), W=8192, N=5120, out="16", small=dict(W=300, N=640)))
_X(case("sample-split-7", ["7 + 1 sample split at a 96x96 layer"], _t(256, 320, 8, conv=1, splitk=1), B=7, H=96, W=96, C0=128, N=320, ks=3, pad=P3, korder=1, out="16",
        rowvec=True, sparse="A", small=dict(B=2, H=16, W=16)))
_X(case("sample-split-1", ["7 + 1 sample split at a 96x96 layer"], _t(128, 160, 4, conv=1, stages=4, splitk=1), B=1, H=96, W=96, C0=128, N=320, ks=3, pad=P3, korder=1, out="16",
        rowvec=True, ws=W64, small=dict(H=16, W=16, ws=MB)))
# ---- epilogues that are not exact: exact pre-activation, the fp32 rule (+ a storage half-step) on the result
for _n, _a in (("silu", SI), ("quickgelu", QG), ("gelu", GE), ("sigmoid", SG)):
    _X(case(f"act-{_n}", ["tolerance-checked epilogue"], _t(128, 128, 4), W=200, N=112, act=_a, alpha=0.125, out="16" if _n in ("silu", "gelu") else "f32"))
_X(case("geglu-4wave", ["tolerance-checked epilogue", "GEGLU"], _t(128, 128, 4), W=200, N=192, act=G_, alpha=0.125))
_X(case("geglu-8wave", ["tolerance-checked epilogue", "GEGLU"], _t(256, 256, 8, direct=1), W=12288, N=1024, act=G_, alpha=0.125, out="16", small=dict(W=300)))
_X(case("geglu-f32-erf", ["tolerance-checked epilogue", "GEGLU"], _t(128, 128, 4), op="f32", W=200, N=192, act=G_, alpha=0.125))
_X(case("gelu-f32", ["tolerance-checked epilogue"], _t(128, 128, 4), op="f32", W=200, N=100, act=GE, alpha=0.125))
_X(case("geglu-exact-4wave", ["GEGLU exact gate"], _t(128, 128, 4), W=200, N=192, act=G_, gate_const=True))
# ---- other operand types: an 8-wave and a 4-wave tile each, split-K where the type allows it
for _op in ("f16", "f32", "w8", "x3"):
    _o = "16" if _op == "f16" else "f32"
    _X(case(f"{_op}-8wave", [f"{_op} 8-wave tile"], _t(128, 256, 8, direct=1), op=_op, W=6200, N=1024, res=True, out=_o, small=dict(W=300)))
    _X(case(f"{_op}-4wave-conv", [f"{_op} 4-wave tile"], _t(128, 160, 4, conv=1, glds=1), op=_op, B=3, H=9, W=9, C0=128, N=144, ks=3, pad=P3, rowvec=True, out=_o,
            korder=0 if _op in ("w8", "x3") else 1))
    _X(case(f"{_op}-sk-frag", [f"{_op} split-K"], _t(128, 320, 8, reduce="frag"), op=_op, W=2048, C0=1536, N=1280, ws=W64, out=_o, sparse="A",
            small=dict(W=300, C0=1024, N=320, ws=4 * MB)))
    _X(case(f"{_op}-sk-stripe8", [f"{_op} split-K"], _t(128, 128, 4, reduce="stripe8"), op=_op, W=100, C0=2048, N=112, ws=MB, res=True, out=_o))
_X(case("f16-hx", ["f16 4-wave tile", "loop row-extended korder 2"], _t(128, 128, 4, hx=1), op="f16", B=3, H=8, W=16, C0=128, N=112, ks=3, pad=P3, korder=2, out="16",
        sparse="A"))
_X(case("f16-ups2", ["f16 4-wave tile", "loop ups 2 (four phases, borders, several samples)"], _t(128, 128, 4), op="f16", B=3, H=16, W=8, C0=64, N=112, ups=2, ks=3,
        pad=P3, out="16"))
_X(case("a8-256x256", ["fp8 x fp8 8-wave tile"], _t(256, 256, 8, direct=1), op="a8", out="16", W=49000, C0=128, N=256, res=True, small=dict(W=300)))
_X(case("a8-128x320", ["fp8 x fp8 8-wave tile"], _t(128, 320, 8, direct=1), op="a8", out="16", W=10240, C0=128, N=640, sparse="A", small=dict(W=300)))
_X(case("a8-128x256", ["fp8 x fp8 8-wave tile"], _t(128, 256, 8, direct=1), op="a8", out="16", W=10240, C0=128, N=512, rowvec=True, B=1, small=dict(W=300)))
_X(case("a8-4wave-c320", ["fp8 x fp8 4-wave tile", "fp8 C = 320 padded to 384"], _t(128, 128, 4), op="a8", out="16", W=200, C0=320, N=112, res=True))
_X(case("a8-4wave-160", ["fp8 x fp8 4-wave tile"], _t(128, 160, 4), op="a8", out="16", W=200, C0=128, N=144, sparse="A"))
_X(case("a8-conv-c320", ["fp8 x fp8 4-wave tile", "fp8 C = 320 padded to 384"], _t(128, 128, 4, conv=1), op="a8", out="16", B=7, H=9, W=9, C0=320, N=112, ks=3, pad=P3,
        sparse="A", rowvec=True))
_X(case("a8-sk-frag", ["fp8 x fp8 split-K"], _t(128, 128, 4, reduce="frag"), op="a8", out="16", W=128, C0=2048, N=112, ws=MB, res=True))
# ---- windows: the geometries the metric towers and front-ends launch (TOWER_WINDOWS below).  Dense operands in +-{1, 2, 3} and fp32 output: every
# tap, channel and border pixel is live in every output row.  cp8: 3 real channels stored in 8 -- non-zero activations in the pad channels, zero weight
# columns.  Shapes are the smallest that cross every edge: odd and even extents on different axes, several samples, N ragged where the plan allows
_CP8 = dict(C0=8, creal=3)
P5, P7 = (2, 2, 2, 2), (3, 3, 3, 3)          # the "same" padding of a 5x5 and of a 7x7 window, as P3 is that of a 3x3
_X(case("win-7x7-s2-cp8", ["window 7x7 s2 p3 on the register loop"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=13, W=10, N=64, ks=7, stride=2,
        pad=P7, act=RL, **_CP8))                                                     # K = 392: four taps per K tile, 8 of 32 positions live in the last one
_X(case("win-11x11-s4-cp8", ["window 11x11 s4 p2 on the register loop"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=23, W=19, N=64, ks=11, stride=4,
        pad=P5, act=RL, bias=False, **_CP8))                                          # (H + 2p - k) % s != 0 on both axes: trailing rows / columns unread
for _op in ("f32", "bf16"):          # (VGG16's and the IResNet's first layer; not in the issue's list)
    _X(case(f"win-3x3-cp8-{_op}", ["window 3x3 p1 on the register loop (3 channels stored in 8)"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op=_op, B=2, H=7, W=6, N=64,
            ks=3, pad=P3, act=RL, **_CP8))
_X(case("win-5x5-c64", ["window 5x5 p2 direct-to-LDS"], _t(128, 128, 4, glds=1, conv=1, splitk=1), op="f32", B=2, H=9, W=7, C0=64, N=96, ks=5, pad=P5))
for _op in ("f32", "bf16"):
    # odd extent 9 -> 5 uses the bottom pad row; even extent 8 -> 4 never reads the right pad column
    _X(case(f"win-3x3-s2-p1-{_op}", ["3x3 s2 symmetric pad"], _t(128, 128, 4, glds=1, conv=1, splitk=1), op=_op, B=3, H=9, W=8, C0=64, N=100, ks=3, stride=2, pad=P3))
    _X(case(f"win-1x1-s2-{_op}", ["1x1 s2 with conv addressing"], _t(128, 128, 4, glds=1, conv=1, splitk=1), op=_op, B=3, H=9, W=8, C0=64, N=128, ks=1, stride=2,
            **(dict(res=True, act=AR) if _op == "bf16" else {})))                     # (bf16: the bottleneck's join)
    _X(case(f"win-patch14-{_op}", ["patch window, stride = window"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op=_op, B=2, H=28, W=42, N=64, ks=14, stride=14,
            bias=False, **_CP8))                                                      # M = 12 < BM
# K = 8192 on the register loop, M = 4: once without a workspace, once with one (guarded).  pick_splitk's cost model prices 2 M N K flops against
# the 3 us of a reduce pass, so with M = 4 rows it keeps splitk = 1 at any workspace size: that plan is what the second case asserts and checks
_X(case("win-patch32-f32", ["patch window, long K on the register loop"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=64, W=32, N=64, ks=32, stride=32,
        bias=False, **_CP8))
_X(case("win-patch32-f32-ws", ["patch window, long K on the register loop"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=64, W=32, N=64, ks=32, stride=32,
        bias=False, ws=MB, **_CP8))
_X(case("win-patch32-bf16", ["patch window, long K on the register loop"], _t(128, 64, 4, glds=0, conv=1, splitk=1), B=2, H=64, W=32, N=64, ks=32, stride=32, bias=False,
        **_CP8))
# the fp32 CLIP towers store the 3 channels in 4 -- a tap is ONE 16-byte vector, eight taps per K tile (not in the issue's list: encoders.py, fidscore.py)
_X(case("win-patch14-f32-cp4", ["patch window, 3 channels stored in 4 (one fp32 vector per tap)"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=28, W=42,
        C0=4, creal=3, N=64, ks=14, stride=14, bias=False))                           # K = 784: half of the last K tile live
_X(case("win-patch32-f32-cp4", ["patch window, 3 channels stored in 4 (one fp32 vector per tap)"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=64, W=32,
        C0=4, creal=3, N=64, ks=32, stride=32, bias=False))
_X(case("win-1x7-s2-regs", ["non-square window, pad_t != pad_l"], _t(128, 64, 4, glds=0, conv=1, splitk=1), op="f32", B=2, H=9, W=12, C0=8, N=64, kh=1, kw=7, stride=2,
        pad=(0, 3, 0, 3)))
_X(case("win-5x3-lds", ["non-square window, pad_t != pad_l"], _t(128, 128, 4, glds=1, conv=1, splitk=1), B=2, H=9, W=11, C0=64, N=100, kh=5, kw=3, pad=(2, 1, 2, 1)))
# split-K over a non-square window: 30 K tiles in three slices of 10, two tiles per tap -- the slices start at taps 0, 5 and 10 (korder 0) and at
# taps 0, 10 and 5 (korder 1), inside window rows 1 and 3 (a multiple of KW = 3 would be a row's first tap: the GPU test asserts it from the plan)
_X(case("win-5x3-lds-k1", ["non-square window under korder 1"], _t(128, 128, 4, glds=1, conv=1, splitk=3, reduce="stripe8"), B=1, H=8, W=8, C0=128, N=112, kh=5, kw=3, pad=(2, 1, 2, 1),
        korder=1, ws=MB))
_X(case("win-5x3-lds-sk", ["non-square window under split-K"], _t(128, 128, 4, glds=1, conv=1, splitk=3, reduce="stripe8"), B=1, H=8, W=8, C0=128, N=112, kh=5, kw=3, pad=(2, 1, 2, 1), ws=MB))
# the packed row descriptor sample:12 | oy:10 | ox:10 of the direct-to-LDS loop: the last shape it takes and the first that goes through registers
_X(case("win-hout-1024", ["packed row descriptor at its limit"], _t(128, 64, 4, glds=1, conv=1), H=1024, W=1, ks=3, pad=P3))
_X(case("win-hout-1025", ["packed row descriptor at its limit"], _t(128, 64, 4, glds=0, conv=1), H=1025, W=1, ks=3, pad=P3))
_X(case("win-wout-1024", ["packed row descriptor at its limit"], _t(128, 64, 4, glds=1, conv=1), H=1, W=1024, ks=3, pad=P3))          # (the ox field: not in the issue's list)
_X(case("win-wout-1025", ["packed row descriptor at its limit"], _t(128, 64, 4, glds=0, conv=1), H=1, W=1025, ks=3, pad=P3))
_X(case("win-samples-4094", ["packed sample field at its limit"], _t(128, 64, 4, glds=1, conv=1), B=4094, ks=3, pad=P3))
_X(case("win-samples-4095", ["packed sample field at its limit"], _t(128, 64, 4, glds=0, conv=1), B=4095, ks=3, pad=P3))
del _X

BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def other_seed(c):
    """the same case with the other sparse operand (16-bit-output exact cases come as a W-sparse and an A-sparse seed); None where it has none"""
    if c["out"] != "16" or not is_exact(c) or c["sparse"] not in ("W", "A") or c["id"][-2:] in ("-W", "-A"):
        return None
    return dict(c, sparse="A" if c["sparse"] == "W" else "W")


def small_of(c):
    """the scaled-down shape of a large case (same features, CPU-sized) for the generator and mutant checks; the case itself otherwise"""
    if not c["small"]:
        return c
    s = dict(c)
    s.update(c["small"])
    s["small"] = None
    return s


# the cells of the table: each must be claimed by a case (test_every_cell_of_the_issue_has_a_case)
CELLS = ("tile 256x320", "tile 256x256", "tile 128x320", "tile 128x256", "tile 128x160 two stages", "tile 128x160 ring (<= 256 blocks)", "tile 128x128", "tile 128x64",
         "loop linear direct-to-LDS", "loop conv direct-to-LDS korder 0", "loop conv direct-to-LDS korder 1", "loop row-extended korder 2",
         "loop conv through registers: C1 concat", "loop conv through registers: Cin = 16", "loop linear through registers: K % 64 != 0", "loop ups 1",
         "loop ups 2 (four phases, borders, several samples)", "loop stride 2 with asymmetric padding", "loop srcx tail", "loop per-sample W", "loop batch > 1",
         "epilogue direct", "epilogue staged", "staged forced by rows_per_sample % BM", "ADD_RELU", "PReLU", "16-bit output", "fp32 output", "ln_stats_out records",
         "ln_stats_in consumer", "fused GroupNorm statistics, direct epilogue", "fused GroupNorm statistics, staged epilogue",
         "split-K 8-row stripe reduce", "split-K 32-row stripe reduce", "split-K fragment slabs, M < BM", "split-K fragment slabs with fused statistics",
         "two-kernel N split (bias, rowvec, residual offsets in the tail)", "pm > 1 and pn < tiles_n", "7 + 1 sample split at a 96x96 layer",
         "tolerance-checked epilogue", "GEGLU", "GEGLU exact gate", "fp8 C = 320 padded to 384",
         "edge ragged M", "edge ragged N", "edge pitched column slice", "edge tile spans a sample boundary") + tuple(
    f"{op} {what}" for op in ("f16", "f32", "w8", "x3") for what in ("8-wave tile", "4-wave tile", "split-K")) + (
    "fp8 x fp8 8-wave tile", "fp8 x fp8 4-wave tile", "fp8 x fp8 split-K")
CELLS += ("window 7x7 s2 p3 on the register loop", "window 11x11 s4 p2 on the register loop", "window 3x3 p1 on the register loop (3 channels stored in 8)",
          "window 5x5 p2 direct-to-LDS", "3x3 s2 symmetric pad", "1x1 s2 with conv addressing", "patch window, stride = window",
          "patch window, 3 channels stored in 4 (one fp32 vector per tap)", "patch window, long K on the register loop", "non-square window, pad_t != pad_l",
          "non-square window under korder 1", "non-square window under split-K", "packed row descriptor at its limit", "packed sample field at its limit")


# ------------------------------------------------------------------------------------------------ the window cases
def is_window_case(c):
    return c["id"].startswith("win-")


WINDOW_CASES = [c for c in CASES if is_window_case(c)]


def live_k(c):
    """True where column k of a dense window case must carry a non-zero product in some row: its tap reaches into the image for some output pixel
    and its channel is a real one (not a zero weight column of a channel-padded input).  korder 0 / 1 only."""
    G = geom(c)
    reach = lambda k, pad, n_in, n_out: any(0 <= o * c["stride"] - pad + k < n_in for o in range(n_out))
    tap = torch.tensor([reach(t // c["kw"], c["pad"][0], c["H"], G["Ho"]) and reach(t % c["kw"], c["pad"][1], c["W"], G["Wo"]) for t in range(G["taps"])])
    ch = torch.arange(G["ctot"]) < (c["creal"] or G["ctot"])
    m = tap[:, None] & ch[None, :]
    if c["korder"] == 1:
        bk = bk_of(c)
        m = m.reshape(G["taps"], G["ctot"] // bk, bk).permute(1, 0, 2)
    assert c["korder"] < 2
    return m.reshape(-1)


def window_mutant_applies(m, c, sk=1):
    """whether slip `m` of the window addressing can show in window case c at all: the geometry has what the slip confuses"""
    G = geom(c)
    kh, kw, s = c["kh"], c["kw"], c["stride"]
    pt, pl = c["pad"][0], c["pad"][1]
    if m == "kh_kw_swapped":
        return kh != kw
    if m == "pad_t_l_swapped":
        return pt != pl
    if m == "stride_rows_only":
        return s > 1 and G["Wo"] > 1
    if m == "border_clamped":          # some tap of some output pixel lies outside the image
        return pt > 0 or pl > 0 or (G["Ho"] - 1) * s - pt + kh > c["H"] or (G["Wo"] - 1) * s - pl + kw > c["W"]
    if m == "cin_pad_ignored":
        return c["creal"] > 0
    if m == "partial_tile_overread":
        return G["K"] % bk_of(c) != 0
    if m == "slice_start_tap":          # some slice but the first starts at a tap that KH and KW decode differently
        if sk < 2 or G["ctot"] % bk_of(c) or c["korder"] > 1:
            return False
        taps = [tap_of_tile(c, t0) for t0 in slice_starts(c, sk)[0][1:]]
        return any((t // kh, t % kh) != (t // kw, t % kw) for t in taps)
    raise KeyError(m)


# who launches which window: (who, KH, KW, stride, pad, stored input channels, operand type) -> the case that pins it.  tests/test_gemm_exact_cpu.py walks
# reface_amd.params.lpips_plan against the rows; the ResNet / IResNet / patch rows restate the source lines named behind them
TOWER_WINDOWS = {
    ("Hopenet ResNet-50 conv1", 7, 7, 2, 3, 8, "f32"): "win-7x7-s2-cp8",                     # posescore.py: _conv(self.x, "conv1.weight", 64, ..., ksize=7, stride=2, cin_pad=self.CP)
    ("Deep3DFaceRecon ResNet-50 conv1", 7, 7, 2, 3, 8, "f32"): "win-7x7-s2-cp8",             # exprscore.py: _conv(self.x, "backbone.conv1.weight", 64, ..., ksize=7, stride=2, cin_pad=self.CP)
    ("BiSeNet ResNet-18 conv1", 7, 7, 2, 3, 8, "f32"): "win-7x7-s2-cp8",                     # parsing.py: _conv(x, "cp.resnet.conv1.weight", 64, ..., ksize=7, stride=2, cin_pad=self.CP)
    ("LPIPS AlexNet features.0", 11, 11, 4, 2, 8, "f32"): "win-11x11-s4-cp8",                # lpips.py: pack_conv_weight(..., cin_pad=CP if first else None), lpips_plan("alex")[0]
    ("LPIPS AlexNet features.3", 5, 5, 1, 2, 64, "f32"): "win-5x5-c64",
    ("LPIPS AlexNet features.6-10 / VGG16 features.2-28", 3, 3, 1, 1, 64, "f32"): "f32-4wave-conv",
    ("LPIPS VGG16 features.0", 3, 3, 1, 1, 8, "f32"): "win-3x3-cp8-f32",
    ("ArcFace IResNet input_layer.0", 3, 3, 1, 1, 8, "bf16"): "win-3x3-cp8-bf16",            # encoders.py: _conv(x, "input_layer.0.weight", 64, ..., cin_pad=self.CP)
    ("ResNet stage entry conv (fp32 towers)", 3, 3, 2, 1, 64, "f32"): "win-3x3-s2-p1-f32",   # posescore.py / exprscore.py: conv2 of a stage's first block, ksize=3, stride=stride; parsing.py: conv1
    ("IResNet stage entry res_layer.3 (ArcFace)", 3, 3, 2, 1, 64, "bf16"): "win-3x3-s2-p1-bf16",          # encoders.py: _conv(r1, "res_layer.3.weight", depth, stride=stride, ...)
    ("ResNet downsample.0 (fp32 towers)", 1, 1, 2, 0, 64, "f32"): "win-1x1-s2-f32",          # posescore.py / exprscore.py / parsing.py: "downsample.0.weight", ksize=1, stride=stride
    ("IResNet shortcut_layer.0 (ArcFace)", 1, 1, 2, 0, 64, "bf16"): "win-1x1-s2-bf16",       # encoders.py: _conv(x, "shortcut_layer.0.weight", depth, stride=stride, ksize=1, ...)
    ("CLIP ViT-L/14 patch embedding", 14, 14, 14, 0, 8, "bf16"): "win-patch14-bf16",          # encoders.py / fidscore.py: ksize=P, stride=P, pad=(0, 0), CP = 8 for 16-bit operands
    ("CLIP ViT-L/14 patch embedding", 14, 14, 14, 0, 4, "f32"): "win-patch14-f32-cp4",       # ... CP = 4 for fp32 operands (one 16-byte pixel)
    ("CLIP ViT-B/32 patch embedding (FID)", 32, 32, 32, 0, 4, "f32"): "win-patch32-f32-cp4",  # fidscore.py: ksize=P, stride=P, pad=(0, 0), self.CP = 4 if dtype == F32 else 8
    ("CLIP ViT-B/32 patch embedding (FID)", 32, 32, 32, 0, 8, "bf16"): "win-patch32-bf16",
}
