"""Test infrastructure: fp64 references, case tables and input builders of the encoder / sampler side kernels (encoder.hip, the glue of
elementwise.hip, rf_softmax_rows) -- shared by tests/test_side_ops_cpu.py (which pins the references against torch's own fp64 operators and
checks that the tables tell wrong variants apart) and tests/test_side_ops_gpu.py (which runs the kernels).  Every reference is written from the
formula in its kernel's comment with torch-CPU indexing only; nothing here imports the package under test (the input builders take the seeded
generator `rnd(shape, seed)` as an argument)."""
import math

import numpy as np
import torch

F64 = torch.float64
STEP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}          # relative rounding step of the 16-bit storage types (test_ops_gpu.STEP)


# ------------------------------------------------------------------------------------------------ tolerances
def limit_f32(ref, scale=1.0):
    """the file-level fp32 rule of tests/test_ops_gpu.py: |got - ref| <= 2e-5 * scale + 2e-5 * |ref|"""
    return 2e-5 * scale + 2e-5 * ref.abs()


def limit_16(ref, dt):
    """16-bit output of an elementwise kernel: one whole storage step (a round-to-nearest store costs half) on top of the fp32 bound"""
    return STEP[dt] * ref.abs() + limit_f32(ref)


def limit(ref, dt, scale=1.0):
    return limit_f32(ref, scale) if dt == torch.float32 else limit_16(ref, dt)


def differs(got, ref, lim):
    """True if `got` is outside the bound anywhere (a non-finite value counts as outside)"""
    return not bool(((got.double() - ref).abs() <= lim).all())


# ------------------------------------------------------------------------------------------------ channel_affine
CHANNEL_AFFINE_CASES = [dict(M=37, C=70, pitch=80), dict(M=3, C=512, pitch=512)]          # each run with and without slope, x = buf[:, :C]


def channel_affine_inputs(case, rnd):
    M, C = case["M"], case["C"]
    buf = rnd((M, case["pitch"]), 101)
    a = 1.0 + 0.5 * rnd((C,), 102)
    b = rnd((C,), 103)
    slope = 0.5 * rnd((C,), 104)
    slope[::3] = 0.0                              # positive, zero and negative slopes
    n0 = min(10, C)
    buf[M // 2, :n0] = 1.0                        # x * a + b == 0 exactly (1 * a - a, exact with or without contraction; 1.0 is a bf16 value)
    b[:n0] = -a[:n0]
    buf[0, :n0] = -1.0                            # and a negative v next to it
    return dict(buf=buf, a=a, b=b, slope=slope)


def channel_affine_ref(x, a, b, slope=None):
    v = x.double() * a.double() + b.double()
    if slope is not None:
        v = torch.where(v >= 0, v, v * slope.double())
    return v


def _ca_slope_on_positive(x, a, b, slope=None):
    v = x.double() * a.double() + b.double()
    return v if slope is None else torch.where(v > 0, v * slope.double(), v)


def _ca_slope_channel0(x, a, b, slope=None):
    v = x.double() * a.double() + b.double()
    return v if slope is None else torch.where(v >= 0, v, v * slope.double()[0])


def _ca_bias_after_prelu(x, a, b, slope=None):
    v = x.double() * a.double()
    if slope is not None:
        v = torch.where(v >= 0, v, v * slope.double())
    return v + b.double()


CHANNEL_AFFINE_VARIANTS = {"slope applied to v > 0": _ca_slope_on_positive, "slope of channel 0 for all": _ca_slope_channel0,
                           "b added after PReLU": _ca_bias_after_prelu}


# ------------------------------------------------------------------------------------------------ spatial_mean
# x = buf[..., :C] of [B, H, W, pitch]; the last case is the accumulation-accuracy one (HW = 112^2, inputs 2 * randn + 3)
SPATIAL_MEAN_CASES = [dict(B=2, H=1, W=1, C=3, pitch=3), dict(B=2, H=3, W=1, C=64, pitch=64), dict(B=3, H=1, W=5, C=70, pitch=70),
                      dict(B=2, H=7, W=7, C=130, pitch=136), dict(B=1, H=98, W=128, C=70, pitch=70, mul=2.0, add=3.0)]


def spatial_mean_inputs(case, rnd):
    buf = rnd((case["B"], case["H"], case["W"], case["pitch"]), 111) * case.get("mul", 1.0) + case.get("add", 0.0)
    return dict(buf=buf)


def spatial_mean_ref(x):
    B, H, W, C = x.shape
    return x.double().reshape(B, H * W, C).sum(1) / (H * W)


def _sm_div_padded(x):
    B, H, W, C = x.shape
    return x.double().reshape(B, H * W, C).sum(1) / (-(-(H * W) // 4) * 4)


def _sm_skip_tail(x):
    B, H, W, C = x.shape
    HW = H * W
    return x.double().reshape(B, HW, C)[:, :HW - HW % 4].sum(1) / HW


SPATIAL_MEAN_VARIANTS = {"divide by ceil(HW/4)*4": _sm_div_padded, "skip the last HW % 4 pixels": _sm_skip_tail}


# ------------------------------------------------------------------------------------------------ se_scale_add
# r, out [B, Ho, Wo, C] packed; shortcut = buf[..., :C] of [B, Hs, Ws, pitch]
SE_B, SE_HO, SE_WO, SE_C = 2, 5, 7, 70
SE_SCALE_ADD_CASES = [dict(st=1, Hs=5, Ws=7, pitch=70), dict(st=2, Hs=10, Ws=14, pitch=70), dict(st=2, Hs=9, Ws=13, pitch=70),
                      dict(st=2, Hs=9, Ws=13, pitch=80)]


def se_scale_add_inputs(case, rnd):
    r = rnd((SE_B, SE_HO, SE_WO, SE_C), 121)
    s = torch.sigmoid(rnd((SE_B, SE_C), 122))
    buf = rnd((SE_B, case["Hs"], case["Ws"], case["pitch"]), 123)
    return dict(r=r, s=s, buf=buf)


def _se(r, s, sc, rows, cols):
    return r.double() * s.double()[:, None, None, :] + sc.double()[:, rows][:, :, cols]


def se_scale_add_ref(r, s, sc, st):
    B, Ho, Wo, C = r.shape
    return _se(r, s, sc, torch.arange(Ho) * st, torch.arange(Wo) * st)


def _se_ox_for_row(r, s, sc, st):
    """row index taken from ox: out[b, oy, ox] reads sc[b, ox * st, ox * st] (wrapped into the shortcut so that the variant stays in bounds)"""
    B, Ho, Wo, C = r.shape
    cols = torch.arange(Wo) * st
    picked = sc.double()[:, cols % sc.shape[1], cols]                    # [B, Wo, C]
    return r.double() * s.double()[:, None, None, :] + picked[:, None]


def _se_no_stride(r, s, sc, st):
    B, Ho, Wo, C = r.shape
    return _se(r, s, sc, torch.arange(Ho), torch.arange(Wo))


def _se_s_of_batch0(r, s, sc, st):
    return se_scale_add_ref(r, s[:1].expand_as(s), sc, st)


SE_SCALE_ADD_VARIANTS = {"ox*st used for the row": _se_ox_for_row, "shortcut read without the stride": _se_no_stride,
                         "s[c] used for every b": _se_s_of_batch0}


# ------------------------------------------------------------------------------------------------ adaptive_avgpool
POOL_B, POOL_C = 2, 3
ADAPTIVE_AVGPOOL_CASES = [
    dict(Hf=7, Wf=5, Ho=3, Wo=4, crop=None, affine=False, nhwc=False, dt=torch.float32),
    dict(Hf=7, Wf=5, Ho=3, Wo=4, crop=None, affine=True, nhwc=False, dt=torch.float32),
    dict(Hf=6, Wf=6, Ho=8, Wo=8, crop=None, affine=False, nhwc=False, dt=torch.float32),          # upsampling pool: overlapping 1- and 2-pixel bins
    dict(Hf=20, Wf=18, Ho=5, Wo=6, crop=(3, 2, 11, 13), affine=False, nhwc=True, Cpad=8, dt=torch.float32),
    dict(Hf=20, Wf=18, Ho=5, Wo=6, crop=(3, 2, 11, 13), affine=False, nhwc=True, Cpad=8, dt=torch.bfloat16),
    dict(Hf=7, Wf=5, Ho=1, Wo=1, crop=None, affine=False, nhwc=False, dt=torch.float32),
    # beyond the issue's table: NCHW output with an affine and a crop together (a branch combination nothing reaches), and an affine whose
    # offset matters per pixel count
    dict(Hf=20, Wf=18, Ho=5, Wo=6, crop=(3, 2, 11, 13), affine=True, nhwc=False, dt=torch.float32),
]


def adaptive_avgpool_inputs(case, rnd):
    x = rnd((POOL_B, POOL_C, case["Hf"], case["Wf"]), 131)
    a = b = None
    if case["affine"]:
        a, b = 1.0 + 0.5 * rnd((POOL_C,), 132), rnd((POOL_C,), 133)
    return dict(x=x, a=a, b=b)


def _pool(x, crop, a, b, Ho, Wo, *, floor_end=False, drop_crop=False, bias_once=False):
    B, C, Hf, Wf = x.shape
    y0, x0, hc, wc = crop if crop is not None else (0, 0, Hf, Wf)
    if drop_crop:
        y0 = x0 = 0
    xd = x.double()
    sa = a.double().view(1, C, 1, 1) if a is not None else 1.0
    sb = b.double().view(1, C) if b is not None else 0.0
    out = torch.empty((B, C, Ho, Wo), dtype=F64)
    for oy in range(Ho):
        ys, ye = (oy * hc) // Ho, ((oy + 1) * hc) // Ho if floor_end else -((-(oy + 1) * hc) // Ho)
        for ox in range(Wo):
            xs, xe = (ox * wc) // Wo, ((ox + 1) * wc) // Wo if floor_end else -((-(ox + 1) * wc) // Wo)
            win = xd[:, :, y0 + ys:y0 + ye, x0 + xs:x0 + xe] * sa
            n = (ye - ys) * (xe - xs)
            if bias_once:
                out[:, :, oy, ox] = (win.sum((2, 3)) + sb) / n if n else float("nan")
            else:
                out[:, :, oy, ox] = (win + (sb.view(1, C, 1, 1) if b is not None else 0.0)).sum((2, 3)) / n if n else float("nan")
    return out


def _pool_layout(o, nhwc, Cpad):
    if not nhwc:
        return o
    B, C, Ho, Wo = o.shape
    out = torch.zeros((B, Ho, Wo, Cpad), dtype=F64)
    out[..., :C] = o.permute(0, 2, 3, 1)
    return out


def adaptive_avgpool_ref(x, Ho, Wo, crop=None, a=None, b=None, nhwc=False, Cpad=None):
    return _pool_layout(_pool(x, crop, a, b, Ho, Wo), nhwc, Cpad)


def _pool_hw_swapped(x, Ho, Wo, crop=None, a=None, b=None, nhwc=False, Cpad=None):
    """bins of the rows computed for Wo outputs and of the columns for Ho, written through the [Ho, Wo] index"""
    o = _pool(x, crop, a, b, Wo, Ho)
    return _pool_layout(o.reshape(o.shape[0], o.shape[1], Ho, Wo), nhwc, Cpad)


ADAPTIVE_AVGPOOL_VARIANTS = {
    "bin end floor instead of ceil": lambda x, Ho, Wo, crop=None, a=None, b=None, nhwc=False, Cpad=None:
        _pool_layout(_pool(x, crop, a, b, Ho, Wo, floor_end=True), nhwc, Cpad),
    "crop offset dropped": lambda x, Ho, Wo, crop=None, a=None, b=None, nhwc=False, Cpad=None:
        _pool_layout(_pool(x, crop, a, b, Ho, Wo, drop_crop=True), nhwc, Cpad),
    "b added once per bin instead of per pixel": lambda x, Ho, Wo, crop=None, a=None, b=None, nhwc=False, Cpad=None:
        _pool_layout(_pool(x, crop, a, b, Ho, Wo, bias_once=True), nhwc, Cpad),
    "H and W swapped": _pool_hw_swapped,
}


def adaptive_avgpool_affine_after_mean(x, Ho, Wo, crop=None, a=None, b=None, nhwc=False, Cpad=None):
    """mean(x) * a + b: NOT a wrong variant -- an affine map commutes with a mean, so this equals the reference (the CPU test asserts that)"""
    o = _pool(x, crop, None, None, Ho, Wo)
    if a is not None:
        o = o * a.double().view(1, -1, 1, 1) + b.double().view(1, -1, 1, 1)
    return _pool_layout(o, nhwc, Cpad)


# ------------------------------------------------------------------------------------------------ bilinear_resize
BILINEAR_B, BILINEAR_C = 2, 3
BILINEAR_CASES = [(7, 5, 5, 7), (5, 7, 13, 3), (1, 1, 3, 4), (3, 4, 1, 1), (33, 17, 32, 16), (16, 16, 16, 16), (24, 24, 7, 7)]   # Hi, Wi, Ho, Wo


def bilinear_inputs(case, rnd):
    Hi, Wi, Ho, Wo = case
    return dict(x=rnd((BILINEAR_B, BILINEAR_C, Hi, Wi), 141), a=1.0 + 0.5 * rnd((BILINEAR_C,), 142), b=rnd((BILINEAR_C,), 143))


def _axis(n_in, n_out, *, clamp0=True, inverse_scale=False, clamp_last=True):
    scale = n_out / n_in if inverse_scale else n_in / n_out
    f = scale * (torch.arange(n_out, dtype=F64) + 0.5) - 0.5
    if clamp0:
        f = f.clamp(min=0.0)
    i0 = f.trunc().long()                          # the kernel's (int) conversion truncates toward zero
    lam = f - i0.double()
    i0 = i0.clamp(0, n_in - 1) if inverse_scale else i0
    i1 = i0 + (i0 < n_in - 1).long() if clamp_last else i0 + 1
    return i0, i1, lam


def _bilinear(x, Ho, Wo, a, b, *, swap_lx=False, yk=None, xk=None):
    B, C, Hi, Wi = x.shape
    v = x.double()
    if a is not None:
        v = v * a.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1)
    y0, y1, ly = _axis(Hi, Ho, **(yk or {}))
    x0, x1, lx = _axis(Wi, Wo, **(xk or {}))
    v = torch.cat([v, torch.zeros((B, C, 1, Wi), dtype=F64)], 2)          # a row past the end for the unclamped-y1 variant (zeros, not the neighbour)
    hy, hx = 1.0 - ly, 1.0 - lx
    if swap_lx:
        lx, hx = hx, lx
    ly, hy, lx, hx = ly.view(Ho, 1), hy.view(Ho, 1), lx.view(1, Wo), hx.view(1, Wo)
    g = lambda yi, xi: v[:, :, yi][:, :, :, xi]
    return hy * (hx * g(y0, x0) + lx * g(y0, x1)) + ly * (hx * g(y1, x0) + lx * g(y1, x1))


def bilinear_resize_ref(x, Ho, Wo, a=None, b=None):
    return _bilinear(x, Ho, Wo, a, b)


BILINEAR_VARIANTS = {
    "lx and hx swapped": lambda x, Ho, Wo, a=None, b=None: _bilinear(x, Ho, Wo, a, b, swap_lx=True),
    "no clamp at 0": lambda x, Ho, Wo, a=None, b=None: _bilinear(x, Ho, Wo, a, b, yk=dict(clamp0=False), xk=dict(clamp0=False)),
    "scale Ho/Hi": lambda x, Ho, Wo, a=None, b=None: _bilinear(x, Ho, Wo, a, b, yk=dict(inverse_scale=True), xk=dict(inverse_scale=True)),
    "y1 not clamped at the last row": lambda x, Ho, Wo, a=None, b=None: _bilinear(x, Ho, Wo, a, b, yk=dict(clamp_last=False)),
}


# ------------------------------------------------------------------------------------------------ clip_tokens
CLIP_TOKENS_CASES = [(2, 1, 8), (3, 49, 70)]          # B, NP, C


def clip_tokens_inputs(case, rnd):
    B, NP, C = case
    return dict(patch=rnd((B, NP, C), 151), cls=rnd((C,), 152), pos=rnd((NP + 1, C), 153))


def clip_tokens_ref(patch, cls, pos):
    B, NP, C = patch.shape
    out = torch.empty((B, NP + 1, C), dtype=F64)
    out[:, 0] = cls.double() + pos.double()[0]
    out[:, 1:] = patch.double() + pos.double()[1:]
    return out


def _ct_pos_minus_1(patch, cls, pos):
    idx = (torch.arange(pos.shape[0]) - 1).clamp(min=0)
    return clip_tokens_ref(patch, cls, pos[idx])


def _ct_cls_every_row(patch, cls, pos):
    return clip_tokens_ref(cls.view(1, 1, -1).expand_as(patch), cls, pos)


CLIP_TOKENS_VARIANTS = {"pos[t-1]": _ct_pos_minus_1, "class token written per patch row": _ct_cls_every_row}


# ------------------------------------------------------------------------------------------------ l2norm_rows
# (rows, cols, per-row scale).  1e18 / 1e-18: the squares (1e36 / 1e-36) stay inside fp32's range, but only narrowly -- the sum of a 1e18 row's
# squares overflows fp32 beyond ~340 / E[x^2] columns, so the big row sits in the 63- and 64-column cases (l2norm_wave_sum_f32 checks this)
L2NORM_CASES = [(1, 1, (1.0,)), (3, 63, (1.0, 1e-18, 1e18)), (2, 64, (1e18, 1e-18)), (5, 513, (1.0, 1e-18, 1.0, 3.0, 0.01)),
                (4, 512, (1e-18, 1.0, 1.0, 100.0))]


def l2norm_inputs(case, rnd):
    rows, cols, scales = case
    return dict(x=rnd((rows, cols), 161) * torch.tensor(scales, dtype=torch.float32).view(rows, 1))


def l2norm_rows_ref(x):
    xd = x.double()
    return xd / (xd * xd).sum(1, keepdim=True).sqrt()


def l2norm_wave_sum_f32(x):
    """float32 emulation of the kernel's sum of squares: 64 lanes, each summing its columns c = lane, lane + 64, ... in order, then a butterfly"""
    xn = x.numpy().astype(np.float32)
    rows, cols = xn.shape
    lanes = np.zeros((rows, 64), dtype=np.float32)
    for c in range(cols):
        lanes[:, c % 64] = lanes[:, c % 64] + xn[:, c] * xn[:, c]
    w = 64
    while w > 1:
        w //= 2
        lanes = lanes[:, :w] + lanes[:, w:2 * w]
    return lanes[:, 0]


# ------------------------------------------------------------------------------------------------ combine3
# (b given, c given, wa, wb, wc, den): the call forms of plms.py:69-99, encoders.py:358-362 and ddpm.py:334
COMBINE3_FORMS = [(True, False, 1.0, -1.0, 0.0, 0.0), (True, False, 3.0, -1.0, 0.0, 2.0), (True, True, 23.0, -16.0, 5.0, 12.0),
                  (True, True, 55.0, -59.0, 37.0, 0.0), (False, False, 0.75, 0.0, 0.0, 0.0), (False, False, 1.0, 0.5, 0.25, 1.75),
                  (False, True, 1.0, 0.5, 0.25, 1.25)]
COMBINE3_N = [1, 1000]
COMBINE3_CASES = [(n, f) for n in COMBINE3_N for f in COMBINE3_FORMS]


def combine3_inputs(n, rnd):
    return dict(a=rnd((n,), 171), b=rnd((n,), 172), c=rnd((n,), 173))


def combine3_ref(a, b, c, wa, wb, wc, den):
    v = a.double() * wa
    if b is not None:
        v = v + b.double() * wb
    if c is not None:
        v = v + c.double() * wc
    return v / den if den != 0 else v


def _c3_always_divide(a, b, c, wa, wb, wc, den):
    return combine3_ref(a, b, c, wa, wb, wc, 0.0) / den


def _c3_no_wc(a, b, c, wa, wb, wc, den):
    return combine3_ref(a, b, None, wa, wb, wc, den)


COMBINE3_VARIANTS = {"division applied when den == 0": _c3_always_divide, "wc dropped": _c3_no_wc}


# ------------------------------------------------------------------------------------------------ cast
CAST_PAIRS = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
              (torch.float32, torch.float16), (torch.float16, torch.float32)]
CAST_N = [1, 255, 1025]
_F32_EDGE_BITS = [
    0x00000000, 0x80000000,                                      # +-0
    0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff,              # bf16 ties (to even: down, up), just above / below a tie
    0x3f801000, 0x3f803000, 0x3f801001, 0x3f800fff,              # fp16 ties (to even: down, up), just above / below a tie
    0x3fffffff, 0x3fff8000, 0x3ffff000,                          # round up across a binade (-> 2.0) in bf16 / fp16
    0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0x7f7f8000,              # largest finite fp32 (-> bf16 inf), largest bf16, the tie above it
    0x477fe000, 0x477fefff, 0x477ff000, 0x477ff001, 0xc77ff000,  # 65504, just below 65520, 65520 (tie -> fp16 inf), above, negative
    0x47c35000, 0x7149f2ca,                                      # 1e5, 1e30: overflow fp16
    0x33800000, 0x33000000, 0x33000001, 0x33c00000, 0xb3000000,  # 2^-24 (smallest fp16 subnormal), 2^-25 (tie -> 0), above it, 3 * 2^-25 (tie -> 2^-23)
    0x387fc000, 0x387fe000, 0x38800000, 0x32000000,              # largest fp16 subnormal, the tie above it, smallest fp16 normal, 2^-27 (-> 0)
    0x7f800000, 0xff800000,                                      # +-inf
]
_H16_EDGE_BITS = {          # zeros, smallest / largest subnormal, smallest normal, 1 and its neighbour, largest finite, infinities
    torch.float16: [0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x3c00, 0x3c01, 0x7bff, 0xfbff, 0x7c00, 0xfc00],
    torch.bfloat16: [0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x0080, 0x3f80, 0x3f81, 0x7f7f, 0xff7f, 0x7f80, 0xff80],
}


def cast_input(src_dt, n, rnd):
    """n values of `src_dt`: the edge patterns first (as many as fit), seeded values of mixed magnitude after them"""
    fill = rnd((n,), 181) * torch.pow(10.0, (rnd((n,), 182) * 2).clamp(-6, 6))
    if src_dt == torch.float32:
        edge = torch.from_numpy(np.array(_F32_EDGE_BITS, dtype=np.uint32).view(np.float32).copy())
        x = fill
    else:
        edge = torch.from_numpy(np.array(_H16_EDGE_BITS[src_dt], dtype=np.uint16).view(np.int16).copy()).view(src_dt)
        x = fill.to(src_dt)
    if n == 1:
        return x                                                  # a single ordinary value (the edges are in the larger sizes)
    k = min(n, edge.numel())
    x[:k] = edge[:k]
    return x


_FMT = {torch.float32: (23, -126, 127), torch.bfloat16: (7, -126, 127), torch.float16: (10, -14, 15)}          # mantissa bits, emin, emax


def cast_ref(x, dst_dt):
    """round-to-nearest-even conversion to `dst_dt`, from the format's definition in float64 (every step exact for <= 24-bit inputs);
    returns the VALUE as float64 (signed zeros and infinities included)"""
    mant, emin, emax = _FMT[dst_dt]
    v = x.double().numpy()
    a = np.abs(v)
    fin = np.isfinite(a)
    _, e = np.frexp(np.where(fin & (a > 0), a, 1.0))              # a = m * 2^e, m in [0.5, 1)
    quantum = np.exp2(np.maximum(e - 1, emin).astype(np.float64) - mant)
    q = np.rint(np.where(fin, a, 0.0) / quantum) * quantum        # np.rint: ties to even; the division is by a power of two
    q = np.where(q > (2.0 - 2.0 ** -mant) * 2.0 ** emax, np.inf, q)
    q = np.where(fin, q, a)
    return torch.from_numpy(np.copysign(q, v))


# ------------------------------------------------------------------------------------------------ silu / to_image
def silu_input(rnd):
    x = torch.cat([torch.linspace(-100.0, 100.0, 401), (rnd((600,), 191) * 30).clamp(-100, 100),
                   torch.tensor([0.0, -0.0, 88.0, -88.0, 100.0, -100.0])])
    return x          # 1007 values: not a multiple of 256


def silu_ref(x):
    xd = x.double()
    return xd / (1.0 + torch.exp(-xd))


def to_image_input(rnd):
    return torch.cat([(rnd((700,), 192) * 1.5).clamp(-3, 3), torch.tensor([-1.0, 1.0, -3.0, 3.0, 0.0, -0.0, -1.0000001, 0.99999994])])


def to_image_ref(x):
    return ((x.double() + 1.0) / 2.0).clamp(0.0, 1.0)


# ------------------------------------------------------------------------------------------------ gaussian_sample
GAUSS_B, GAUSS_C, GAUSS_H, GAUSS_W = 2, 4, 3, 3
GAUSS_LOGVARS = (-40.0, -30.0, 0.0, 20.0, 25.0)
GAUSS_CASES = [True, False]          # eps given / None


def gaussian_inputs(rnd):
    m = rnd((GAUSS_B, 2 * GAUSS_C, GAUSS_H, GAUSS_W), 201)
    eps = rnd((GAUSS_B, GAUSS_C, GAUSS_H, GAUSS_W), 202)
    lv = m[:, GAUSS_C:].reshape(GAUSS_B, -1)
    ev = eps.reshape(GAUSS_B, -1)
    for i, v in enumerate(GAUSS_LOGVARS):
        lv[:, 3 * i] = v
    ev[:, 0] = 1e6            # at logvar -40: exp(-15) * 1e6 (clamped) against exp(-20) * 1e6 -- makes the lower clamp visible at the fp32 bound
    m[:, GAUSS_C:] = lv.view(GAUSS_B, GAUSS_C, GAUSS_H, GAUSS_W)
    eps = ev.view(GAUSS_B, GAUSS_C, GAUSS_H, GAUSS_W)
    return dict(moments=m, eps=eps, scale=0.18215)


def gaussian_sample_ref(moments, eps, scale, lo=-30.0, hi=20.0, swap_halves=False):
    Cc = moments.shape[1] // 2
    mean, lv = moments.double()[:, :Cc], moments.double()[:, Cc:]
    if swap_halves:
        mean, lv = lv, mean
    if lo is not None:
        lv = torch.maximum(lv, torch.tensor(lo, dtype=F64))
    if hi is not None:
        lv = torch.minimum(lv, torch.tensor(hi, dtype=F64))
    x = mean if eps is None else mean + torch.exp(0.5 * lv) * eps.double()
    return scale * x


GAUSS_VARIANTS = {"clamp bounds swapped": lambda m, e, s: gaussian_sample_ref(m, e, s, lo=20.0, hi=-30.0),
                  "clamp missing": lambda m, e, s: gaussian_sample_ref(m, e, s, lo=None, hi=None),
                  "lower clamp missing": lambda m, e, s: gaussian_sample_ref(m, e, s, lo=None),
                  "upper clamp missing": lambda m, e, s: gaussian_sample_ref(m, e, s, hi=None),
                  "mean and logvar halves swapped": lambda m, e, s: gaussian_sample_ref(m, e, s, swap_halves=True)}


# ------------------------------------------------------------------------------------------------ ddim_update / ddim_pack
DDIM_B, DDIM_H, DDIM_W = 2, 3, 5
DDIM_UPDATE_CASES = [(cfg, noise, px0, ld) for cfg in (True, False) for noise in (True, False) for px0 in (True, False) for ld in (4, 16)]
DDIM_COEFS = (0.5, 0.6, 0.1)          # a_t, a_prev, sigma
DDIM_SCALE = 3.5


def ddim_coefs():
    a_t, a_prev, sig = DDIM_COEFS
    return torch.tensor([math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_prev), math.sqrt(1 - a_prev - sig ** 2), sig], dtype=torch.float32)


def ddim_update_inputs(case, rnd):
    cfg, _, _, ld = case
    B = DDIM_B
    return dict(eps=rnd(((2 * B if cfg else B), DDIM_H, DDIM_W, ld), 211), img=rnd((B, 4, DDIM_H, DDIM_W), 212),
                noise=rnd((B, 4, DDIM_H, DDIM_W), 213), coefs=ddim_coefs())


def ddim_update_ref(eps, img, noise, coefs, cfg, scale, swap_halves=False):
    """-> (x_prev, pred_x0); eps channels-last [(2B | B), h, w, ld], the first 4 channels count"""
    B = img.shape[0]
    e = eps.double()[..., :4].permute(0, 3, 1, 2)
    if cfg:
        eu, ec = (e[B:], e[:B]) if swap_halves else (e[:B], e[B:])
        e = eu + scale * (ec - eu)
    c = coefs.double()
    px0 = (img.double() - c[1] * e) / c[0]
    xp = c[2] * px0 + c[3] * e
    if noise is not None:
        xp = xp + c[4] * noise.double()
    return xp, px0


DDIM_UPDATE_VARIANTS = {"unconditional and conditional halves swapped":
                        lambda eps, img, noise, coefs, cfg, scale: ddim_update_ref(eps, img, noise, coefs, cfg, scale, swap_halves=True)}

DDIM_PACK_CASES = [(dup, dt, Cpad) for dup in (1, 2) for dt in (torch.float32, torch.bfloat16, torch.float16) for Cpad in (9, 16)]


def ddim_pack_inputs(rnd):
    B = DDIM_B
    return dict(img=rnd((B, 4, DDIM_H, DDIM_W), 221), z=rnd((B, 4, DDIM_H, DDIM_W), 222), mask=(rnd((B, 1, DDIM_H, DDIM_W), 223) > 0).float())


def ddim_pack_ref(img, z, mask, dup, Cpad):
    B, _, h, w = img.shape
    out = torch.zeros((dup * B, h, w, Cpad), dtype=F64)
    for r in range(dup):
        out[r * B:(r + 1) * B, ..., 0:4] = img.double().permute(0, 2, 3, 1)
        out[r * B:(r + 1) * B, ..., 4:8] = z.double().permute(0, 2, 3, 1)
        out[r * B:(r + 1) * B, ..., 8:9] = mask.double().permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------ layouts
LAYOUT_B, LAYOUT_C, LAYOUT_H, LAYOUT_W, LAYOUT_CPAD, LAYOUT_LDX = 2, 5, 6, 7, 8, 16
LAYOUT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def layout_input(rnd):
    return rnd((LAYOUT_B, LAYOUT_C, LAYOUT_H, LAYOUT_W), 231)


def nchw_to_nhwc_ref(x, Cpad):
    B, C, H, W = x.shape
    out = torch.zeros((B, H, W, Cpad), dtype=F64)
    for c in range(C):
        out[..., c] = x.double()[:, c]
    return out


def nhwc_to_nchw_ref(x, C):
    B, H, W, _ = x.shape
    out = torch.empty((B, C, H, W), dtype=F64)
    for c in range(C):
        out[:, c] = x.double()[..., c]
    return out


# ------------------------------------------------------------------------------------------------ timestep_embedding
TIMESTEP_CASES = [(n, dim) for n in (1, 4) for dim in (320, 6, 7)]
_TIMESTEPS = (981.0, 1.0, 500.0, 21.0)


def timestep_inputs(case):
    n, dim = case
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(0, half, dtype=torch.float32) / half)
    return dict(t=torch.tensor(_TIMESTEPS[:n], dtype=torch.float32), freqs=freqs)


def timestep_embedding_ref(t, freqs, dim, swap=False):
    args = (t[:, None] * freqs[None]).double()          # the product is formed in fp32 (as the kernel and the existing test do)
    first, second = (torch.sin(args), torch.cos(args)) if swap else (torch.cos(args), torch.sin(args))
    out = torch.zeros((t.shape[0], dim), dtype=F64)
    half = dim // 2
    out[:, :half], out[:, half:2 * half] = first, second
    return out


TIMESTEP_VARIANTS = {"sin and cos halves swapped": lambda t, freqs, dim: timestep_embedding_ref(t, freqs, dim, swap=True)}


# ------------------------------------------------------------------------------------------------ softmax_rows
SOFTMAX_CASES = [(cols, ld) for cols in (4, 36, 1028, 2052) for ld in (cols, cols + 4)]          # packed and a pitched view
SOFTMAX_ROWS = 4          # ordinary (3 * randn); +60 spike at the last column; all -1e4; +200 spike at the last column


def softmax_inputs(case, rnd):
    cols, _ = case
    x = rnd((SOFTMAX_ROWS, cols), 241) * 3
    x[1, -1] += 60.0
    x[2, :] = -1e4
    x[3, -1] += 200.0         # beyond fp32's exp range from the rest of the row: a maximum that misses this column overflows
    return dict(x=x)


def softmax_rows_ref(x):
    xd = x.double()
    e = torch.exp(xd - xd.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def _softmax_max_first_1024(x):
    """the maximum taken over the first 1024 columns only; the exponentials in float32 as in the kernel (in exact arithmetic softmax is
    shift-invariant: the slip shows only where exp(x - m) leaves fp32's range)"""
    m = x[:, :1024].max(1, keepdim=True).values
    e = torch.exp((x - m).float())
    return (e / e.sum(1, keepdim=True)).double()


SOFTMAX_VARIANTS = {"maximum over the first 1024 columns only": _softmax_max_first_1024}
