"""Numpy restatements of the masked paste (include/reface_hip.h: rf_paste_alpha_u8, rf_paste_back_alpha_u8) and the PIL chain they stand
for.  Integer arithmetic is int64 throughout; the fp64 expressions keep PIL's operation order."""
import numpy as np
from PIL import Image


# ---- the alpha plane
def mask_of_labels(labels, lut):
    """Step 1: 255 where lut[label] is set."""
    return np.where(np.asarray(lut)[np.asarray(labels)] != 0, 255, 0).astype(np.uint8)


def _shifted(m, k, axis, fill=0):
    """m moved by k along `axis` (out[i] = m[i + k]), positions from outside the map filled with `fill`."""
    out = np.full_like(m, fill)
    n = m.shape[axis]
    if abs(k) >= n:
        return out
    src = [slice(None)] * m.ndim
    dst = [slice(None)] * m.ndim
    src[axis] = slice(max(k, 0), n + min(k, 0))
    dst[axis] = slice(max(-k, 0), n - max(k, 0))
    out[tuple(dst)] = m[tuple(src)]
    return out


def dilate(m, d):
    """Step 2: the maximum over the (2d + 1)^2 square, restricted to the map (the values are >= 0, so an outside 0 never wins)."""
    m = np.asarray(m, dtype=np.int64)
    for axis in (-1, -2):
        src, m = m, m.copy()
        for k in range(-d, d + 1):
            m = np.maximum(m, _shifted(src, k, axis))
    return m.astype(np.uint8)


def box_1d(m, r, axis):
    """One box pass: (sum of the 2r + 1 samples, outside = 0, + r) // (2r + 1)."""
    m = np.asarray(m, dtype=np.int64)
    s = np.zeros_like(m)
    for k in range(-r, r + 1):
        s += _shifted(m, k, axis)
    return ((s + r) // (2 * r + 1)).astype(np.uint8)


def feather(m, r, passes):
    """Step 3: `passes` times a horizontal, then a vertical box pass; r = 0 skips the step."""
    if r == 0:
        return np.asarray(m, dtype=np.uint8)
    for _ in range(passes):
        m = box_1d(box_1d(m, r, -1), r, -2)
    return m


def alpha_small(labels, lut, d, r, passes):
    """Steps 1-3: the alpha plane at the label map's size."""
    return feather(dilate(mask_of_labels(labels, lut), d), r, passes)


def _taps(n_in, n_out):
    """PIL's BILINEAR coefficients of an upscale n_in -> n_out (Resample.c precompute_coeffs + normalize_coeffs_8bpc): per output index the
    first input index and the two 22-bit fixed-point weights (0 where the window holds one sample)."""
    scale = n_in / n_out
    lo, k = np.zeros(n_out, dtype=np.int64), np.zeros((n_out, 2), dtype=np.int64)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - 1.0 + 0.5), 0)
        xmax = min(int(center + 1.0 + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((x + xmin) - center + 0.5)) for x in range(xmax - xmin)]
        ww = sum(w)
        assert len(w) <= 2
        lo[i] = xmin
        for x, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            k[i, x] = int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22))
    return lo, k


def resize_bilinear_u8(m, S):
    """Step 4: Image.resize((S, S), BILINEAR) of an 8-bit plane [n, n]: the horizontal pass, clipped to u8, then the vertical pass."""
    m = np.asarray(m, dtype=np.int64)
    n = m.shape[0]
    if S == n:
        return m.astype(np.uint8)
    lo, k = _taps(n, S)
    hi = np.minimum(lo + 1, n - 1)          # (its weight is 0 where the window has one sample)
    clip8 = lambda s: np.clip(s >> 22, 0, 255)
    h = clip8((1 << 21) + m[:, lo] * k[:, 0][None, :] + m[:, hi] * k[:, 1][None, :])
    v = clip8((1 << 21) + h[lo, :] * k[:, 0][:, None] + h[hi, :] * k[:, 1][:, None])
    return v.astype(np.uint8)


def alpha_plane(labels, lut, d, r, passes, S):
    """rf_paste_alpha_u8 of one label map, step 4 done by PIL itself."""
    m = alpha_small(labels, lut, d, r, passes)
    return m.copy() if S == m.shape[0] else np.asarray(Image.fromarray(m).resize((S, S), Image.BILINEAR))


# ---- the paste
def _muldiv255(x, y):
    t = x * y + 128
    return ((t >> 8) + t) >> 8


def _shift8(x):
    return ((x >> 8) + x) >> 8


def paste_alpha(crop, alpha, c, frame, Co):
    """rf_paste_back_alpha_u8 of one frame: crop uint8 [S, S, 3], alpha uint8 [S, S], c the 8 coefficients, frame uint8 [H, W, 3 | 4]."""
    crop, alpha, frame = np.asarray(crop, dtype=np.int64), np.asarray(alpha, dtype=np.int64), np.asarray(frame)
    S, (H, W, Cf) = crop.shape[0], frame.shape
    c = [np.float64(v) for v in c]
    yy, xx = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        xi, yi = xx.astype(np.float64) + 0.5, yy.astype(np.float64) + 0.5
        d = c[6] * xi + c[7] * yi + 1.0
        sx = (c[0] * xi + c[1] * yi + c[2]) / d
        sy = (c[3] * xi + c[4] * yi + c[5]) / d
        inside = (sx >= 0.0) & (sx < float(S)) & (sy >= 0.0) & (sy < float(S))
    out = np.empty((H, W, 4), dtype=np.uint8)
    out[..., :3] = frame[..., :3]
    out[..., 3] = frame[..., 3] if Cf == 4 else 255
    sx, sy = sx[inside], sy[inside]
    u, v = sx - 0.5, sy - 0.5
    fx, fy = np.floor(u), np.floor(v)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    dx, dy = u - fx, v - fy
    cx0, cx1, cy0 = np.clip(x0, 0, S - 1), np.clip(x0 + 1, 0, S - 1), np.clip(y0, 0, S - 1)
    row2 = (y0 + 1 >= 0) & (y0 + 1 < S)
    cy1 = np.where(row2, y0 + 1, cy0)
    rgba = np.concatenate([_muldiv255(crop, alpha[..., None]), alpha[..., None]], axis=-1).astype(np.float64)          # the premultiplied image
    a0, b0, a1, b1 = rgba[cy0, cx0], rgba[cy0, cx1], rgba[cy1, cx0], rgba[cy1, cx1]
    v1 = a0 + (b0 - a0) * dx[:, None]
    v2 = np.where(row2[:, None], a1 + (b1 - a1) * dx[:, None], v1)
    p = (v1 + (v2 - v1) * dy[:, None]).astype(np.int64)          # truncation
    pa = p[:, 3]
    part = (pa != 0) & (pa != 255)
    col = p[:, :3].copy()
    col[part] = np.minimum(255, (255 * col[part]) // pa[part, None])
    dst = out[inside].astype(np.int64)
    da = dst[:, 3]
    blend = da * (255 - pa)
    outa255 = pa * 255 + blend
    safe = np.where(outa255 == 0, 1, outa255)
    coef1 = pa * 255 * 255 * 128 // safe
    coef2 = 255 * 128 - coef1
    res = np.empty_like(dst)
    res[:, :3] = _shift8(col * coef1[:, None] + dst[:, :3] * coef2[:, None] + (0x80 << 7)) >> 7
    res[:, 3] = _shift8(outa255 + 0x80)
    res[pa == 0] = dst[pa == 0]
    out[inside] = res.astype(np.uint8)
    return out if Co == 4 else out[..., :3]


def taps_alpha_zero(alpha, c, H, W):
    """[H, W] bool: the output pixels that lie inside the quad and whose four bilinear taps all have alpha 0."""
    alpha = np.asarray(alpha)
    S = alpha.shape[0]
    c = [np.float64(v) for v in c]
    yy, xx = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        xi, yi = xx + 0.5, yy + 0.5
        d = c[6] * xi + c[7] * yi + 1.0
        sx, sy = (c[0] * xi + c[1] * yi + c[2]) / d, (c[3] * xi + c[4] * yi + c[5]) / d
        inside = (sx >= 0.0) & (sx < float(S)) & (sy >= 0.0) & (sy < float(S))
    x0 = np.floor(np.where(inside, sx, 0.5) - 0.5).astype(np.int64)
    y0 = np.floor(np.where(inside, sy, 0.5) - 0.5).astype(np.int64)
    cx0, cx1, cy0, cy1 = (np.clip(v, 0, S - 1) for v in (x0, x0 + 1, y0, y0 + 1))
    return inside & (alpha[cy0, cx0] == 0) & (alpha[cy0, cx1] == 0) & (alpha[cy1, cx0] == 0) & (alpha[cy1, cx1] == 0)


def _pil_paste_alpha(crop, alpha, c, frame, Co):
    """The masked stage 3 on one frame with PIL itself: putalpha(mask) -> transform(PERSPECTIVE, BILINEAR) -> alpha_composite."""
    s = Image.fromarray(np.ascontiguousarray(crop)).convert("RGBA")
    s.putalpha(Image.fromarray(np.ascontiguousarray(alpha)))
    p = Image.fromarray(np.ascontiguousarray(frame)).convert("RGBA")
    p.alpha_composite(s.transform(p.size, Image.PERSPECTIVE, tuple(float(v) for v in c), Image.BILINEAR))
    a = np.asarray(p)
    return a if Co == 4 else a[..., :3]
