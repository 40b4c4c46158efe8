"""Stage 1's face alignment from 68 landmarks on: the FFHQ recipe of the reference (src/utils/alignmengt.py: compute_transform, crop_image,
crop_faces), with its per-frame PIL pixel work reproduced byte for byte by two HIP kernels (reface_amd/csrc/align.hip):

  c, x, y = compute_transform(landmarks)                    quad_from_landmarks      (host, fp64, the reference's order of operations)
  quad    = [c - x - y, c - x + y, c + x + y, c + x - y]
  shrink  = floor(qsize / output_size / 2); when > 1: img.resize(rsize, ANTIALIAS), quad /= shrink          crop_plan + rf_resample_u8
  img.crop(bounding box of the quad + border); quad -= its corner                                          crop_plan (a window, no copy)
  img.transform((S, S), QUAD, (quad + 0.5).flatten(), BILINEAR)                                            rf_align_quad_u8
  inverse transform = calc_alignment_coefficients(quad + 0.5, crop corners)                                pasteback.alignment_coefficients

crop_image's ``enable_padding`` branch (the FFHQ recipe's edge padding; off in every caller of the reference, on when FFHQ was aligned) is the
opt-in ``pad_edges`` of Aligner / align_to_disk (reface_amd/csrc/align_pad.hip), for crop windows the quad leaves by more than border - 4:

  pad  = max(pads of the quad's bounding box + border, rint(0.3 qsize));  np.pad(float32(img), pad, 'reflect')       pad_plan; index maps
  img += (gaussian_filter(img, [blur, blur, 0]) - img) * clip(3 mask + 1, 0, 1),  blur = 0.02 qsize                   rf_align_pad_u8:
  img += (median(img, axis=(0, 1)) - img) * clip(mask, 0, 1);  uint8(clip(rint(img), 0, 255));  quad += pad[:2]          blur, select, fill
  the transform then reads the padded image                                                                           rf_align_quad_u8

byte for byte numpy / scipy's (fp64 accumulation in scipy's order, float32 between the blur's passes, the mask in fp64 as numpy >= 2
promotes it, an exact median).  pad_image_host is the same recipe in numpy with every dtype written out: the tests' oracle.  Frames whose
plan does not pad keep their bytes.  What the padding does to swap quality is unmeasured.

Landmark DETECTION is not built: landmarks come from a file, or from dlib where it is installed (dlib_landmarks).
"""
import functools
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .pasteback import alignment_coefficients

DLIB_PREDICTOR = "Other_dependencies/DLIB_landmark_det/shape_predictor_68_face_landmarks.dat"          # alignmengt.py:191
PRECISION_BITS = 22          # Resample.c: 8-bit taps are 22-bit fixed point

CropPlan = namedtuple("CropPlan", "shrink rsize window quad coeffs qsize")
PadPlan = namedtuple("PadPlan", "pad size blur radius quad coeffs")
# Device scratch the padded path may hold at once: a batch is padded in sub-batches of as many frames as fit (a frame costs
# hmax * wmax * 3 * (1 + 4 + 4) bytes: the padded u8 image and two fp32 planes; a 700 px face pads to about 1400^2 = 53 MB, so ten fit).
PAD_SCRATCH_BYTES = 640 << 20


def quad_from_landmarks(lm68, scale=1.0):
    """compute_transform (alignmengt.py:148-175) of one face's 68 landmarks [68, 2] -> (c, x, y, quad): the crop's centre, its half-axes and
    the oriented quad [4, 2] (nw, sw, se, ne) in fp64."""
    lm = np.asarray(lm68, dtype=np.float64)
    if lm.shape != (68, 2):
        raise ValueError(f"expected 68 landmarks [68, 2], got {lm.shape}")
    lm_eye_left, lm_eye_right, lm_mouth_outer = lm[36:42], lm[42:48], lm[48:60]
    eye_left = np.mean(lm_eye_left, axis=0)
    eye_right = np.mean(lm_eye_right, axis=0)
    eye_avg = (eye_left + eye_right) * 0.5
    eye_to_eye = eye_right - eye_left
    mouth_avg = (lm_mouth_outer[0] + lm_mouth_outer[6]) * 0.5
    eye_to_mouth = mouth_avg - eye_avg
    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    x *= scale
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    return c, x, y, quad_of(c, x, y)


def quad_of(c, x, y):
    """[..., 4, 2] corners nw, sw, se, ne of centre(s) c and half-axes x, y (alignmengt.py:93, :215)."""
    c, x, y = (np.asarray(v, dtype=np.float64) for v in (c, x, y))
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y], axis=-2)


def smooth_quads(cs, xs, ys, center_sigma=0.0, xy_sigma=0.0):
    """crop_faces' temporal smoothing (alignmengt.py:206-215): gaussian_filter1d over the frame axis of the centres and of the half-axes,
    each when its sigma is not 0 (both are 0 in every caller of the reference) -> (cs, xs, ys, quads [N, 4, 2])."""
    cs, xs, ys = (np.asarray(v, dtype=np.float64) for v in (cs, xs, ys))
    if center_sigma != 0 or xy_sigma != 0:
        from scipy.ndimage import gaussian_filter1d
        if center_sigma != 0:
            cs = gaussian_filter1d(cs, sigma=center_sigma, axis=0)
        if xy_sigma != 0:
            xs = gaussian_filter1d(xs, sigma=xy_sigma, axis=0)
            ys = gaussian_filter1d(ys, sigma=xy_sigma, axis=0)
    return cs, xs, ys, quad_of(cs, xs, ys)


def quad_coefficients(quad, size):
    """The 8 coefficients PIL's Image.transform((size, size), QUAD, (quad + 0.5).flatten()) hands its C loop (Image.__transformer): corners
    nw, sw, se, ne, As = At = 1 / size; output pixel centre (u, v) reads the source at a0 + a1 u + a2 v + a3 u v, a4 + a5 u + a6 v + a7 u v."""
    d = (np.asarray(quad, dtype=np.float64).reshape(4, 2) + 0.5).flatten()
    nw, sw, se, ne = d[:2], d[2:4], d[4:6], d[6:8]
    x0, y0 = nw
    As = At = 1.0 / size
    return np.array([x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
                     y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At], dtype=np.float64)


def crop_plan(quad, image_size, output_size, enable_padding=False):
    """crop_image's bookkeeping (alignmengt.py:100-145) for a quad in an image of ``image_size`` = (W, H), without its pixels:
    shrink  the integer LANCZOS shrink factor (<= 1: none); rsize = (w, h) the image is resized to when shrink > 1, else None;
    window  (ox, oy, w, h): the sub-rectangle of the (resized) image the reference crops to before the transform;
    quad    the quad in that window's coordinates (divided by shrink, the window's corner subtracted);
    coeffs  quad_coefficients(quad, output_size);
    qsize   the quad's side after the shrink (what crop_image derives its border, pads and blur from: pad_plan)."""
    if enable_padding:
        raise NotImplementedError("crop_plan does not take enable_padding: crop_image's padding is pad_plan(crop_plan(...), output_size), "
                                  "and Aligner(pad_edges=True) runs it")
    quad = np.array(quad, dtype=np.float64).reshape(4, 2)
    if not np.isfinite(quad).all():
        raise ValueError("crop_plan: the quad is not finite")
    W, H = int(image_size[0]), int(image_size[1])
    x = (quad[3] - quad[1]) / 2
    qsize = np.hypot(*x) * 2
    shrink = int(np.floor(qsize / output_size * 0.5))
    rsize = None
    if shrink > 1:
        rsize = (int(np.rint(float(W) / shrink)), int(np.rint(float(H) / shrink)))
        W, H = rsize
        quad /= shrink
        qsize /= shrink
    border = max(int(np.rint(qsize * 0.1)), 3)
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))), int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, W), min(crop[3] + border, H))
    window = (0, 0, W, H)
    if crop[2] - crop[0] < W or crop[3] - crop[1] < H:
        if crop[2] <= crop[0] or crop[3] <= crop[1]:
            raise ValueError(f"crop_plan: the quad lies outside the {W}x{H} image")
        window = (crop[0], crop[1], crop[2] - crop[0], crop[3] - crop[1])
        quad -= crop[0:2]
    return CropPlan(shrink, rsize, window, quad, quad_coefficients(quad, output_size), float(qsize))


# ---- crop_image's enable_padding branch (alignmengt.py:125-140): reflect pad, blur towards the border, median fill --------------------------
def pad_plan(plan, output_size):
    """crop_image's pad decision for a CropPlan (host, fp64, the reference's order of operations): None when the branch does not run
    (max(pad) <= border - 4: the frame takes the unpadded path), else PadPlan:
    pad     (left, top, right, bottom), each >= rint(0.3 qsize);   size = (w, h) of the padded window;
    blur    the Gaussian's sigma, 0.02 qsize;   radius = int(4 blur + 0.5), scipy's truncation;
    quad    the plan's quad moved by (left, top);   coeffs = quad_coefficients(quad, output_size)."""
    quad, (_, _, W0, H0), qsize = plan.quad, plan.window, np.float64(plan.qsize)
    border = max(int(np.rint(qsize * 0.1)), 3)
    pad = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))), int(np.ceil(max(quad[:, 1]))))
    pad = (max(-pad[0] + border, 0), max(-pad[1] + border, 0), max(pad[2] - W0 + border, 0), max(pad[3] - H0 + border, 0))
    if not max(pad) > border - 4:
        return None
    pad = np.maximum(pad, int(np.rint(qsize * 0.3)))
    if pad.min() < 1:
        raise ValueError(f"pad_plan: a face of {float(qsize):.2f} px is too small to pad (the reference divides by a pad of 0)")
    blur = qsize * 0.02
    quad = quad + pad[:2]
    pad = tuple(int(v) for v in pad)
    return PadPlan(pad, (W0 + pad[0] + pad[2], H0 + pad[1] + pad[3]), float(blur), int(4.0 * float(blur) + 0.5), quad, quad_coefficients(quad, output_size))


def _fold_numpy(i, n):
    """np.pad's 'reflect' as an index map: the edge is not repeated (period 2 (n - 1)); an axis of length 1 repeats its pixel."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def _fold_scipy(i, n):
    """scipy.ndimage's 'reflect' as an index map: the edge is repeated (period 2 n)."""
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gaussian_weights(blur):
    """scipy.ndimage's _gaussian_kernel1d(blur, 0, radius)[::-1] in fp64, and the radius int(4 blur + 0.5)."""
    blur = float(blur)
    radius = int(4.0 * blur + 0.5)
    if radius == 0:
        return np.ones(1, dtype=np.float64), 0
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / (blur * blur) * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return np.ascontiguousarray(phi_x[::-1]), radius


def _blur_axis0(a32, weights, radius):
    """scipy's correlate1d along axis 0 of a float32 array, mode 'reflect', symmetric branch: fp64 accumulation, rounded to float32."""
    n = a32.shape[0]
    a, i = a32.astype(np.float64), np.arange(n)
    acc = a * weights[radius]
    for j in range(-radius, 0):
        acc += (a[_fold_scipy(i + j, n)] + a[_fold_scipy(i - j, n)]) * weights[j + radius]
    return acc.astype(np.float32)


def gaussian_blur_host(img32, blur):
    """scipy.ndimage.gaussian_filter(img32, [blur, blur, 0]) of a float32 [h, w, C] image, bit for bit: axis 0, then axis 1, float32 between."""
    weights, radius = gaussian_weights(blur)
    g = _blur_axis0(np.asarray(img32, dtype=np.float32), weights, radius)
    return np.ascontiguousarray(_blur_axis0(g.transpose(1, 0, 2), weights, radius).transpose(1, 0, 2))


def _check_pad(window_hw, pad, blur):
    pad = tuple(int(v) for v in pad)
    if len(pad) != 4 or min(pad) < 1:
        raise ValueError(f"pads are (left, top, right, bottom), each >= 1, got {pad}")
    if min(window_hw) < 1 or not (np.isfinite(blur) and blur >= 0):
        raise ValueError(f"a window of {window_hw[1]}x{window_hw[0]} px / a blur of {blur} cannot be padded")
    return pad


def pad_profiles(W0, H0, pad):
    """The mask of crop_image's padding as two 1-D profiles: mask[y, x] = max(mx[x], my[y]), fp64 (float32 / int64 promotes to it)."""
    left, top, right, bottom = pad
    w, h = W0 + left + right, H0 + top + bottom
    x, y = np.arange(w), np.arange(h)
    mx = 1.0 - np.minimum(np.float32(x).astype(np.float64) / np.float64(left), np.float32(w - 1 - x).astype(np.float64) / np.float64(right))
    my = 1.0 - np.minimum(np.float32(y).astype(np.float64) / np.float64(top), np.float32(h - 1 - y).astype(np.float64) / np.float64(bottom))
    return mx, my


def median_f32(plane32):
    """np.median of a float32 plane as float32: the middle element, or float32(a + b) / 2 of the two middle ones."""
    v = np.sort(np.asarray(plane32, dtype=np.float32), axis=None)
    n = v.size
    return v[n // 2] if n & 1 else np.float32(np.float32(v[n // 2 - 1] + v[n // 2]) / np.float32(2))


def pad_image_host(window_u8, pad, blur, parts=None):
    """crop_image's enable_padding branch on the crop window uint8 [H0, W0, 3 | 4] (alpha is not read) with pad = (left, top, right, bottom)
    and the Gaussian's sigma ``blur`` -> the padded uint8 image [h, w, 3].  Every dtype is written out, so the result does not depend on
    numpy's promotion rules.  ``parts`` (a dict) receives img1 (after the blur mix) and med (the channel medians)."""
    win = np.asarray(window_u8)
    if win.dtype != np.uint8 or win.ndim != 3 or win.shape[2] not in (3, 4):
        raise ValueError(f"the window is uint8 [H0, W0, 3 | 4], got {win.dtype} {win.shape}")
    H0, W0 = win.shape[:2]
    left, top, right, bottom = pad = _check_pad((H0, W0), pad, blur)
    w, h = W0 + left + right, H0 + top + bottom
    rows, cols = _fold_numpy(np.arange(h) - top, H0), _fold_numpy(np.arange(w) - left, W0)
    img = win[rows][:, cols, :3].astype(np.float32)
    mx, my = pad_profiles(W0, H0, pad)
    mask = np.maximum(mx[None, :], my[:, None])[..., None]
    g = gaussian_blur_host(img, blur)
    img1 = (img.astype(np.float64) + (g - img).astype(np.float64) * np.clip(mask * 3.0 + 1.0, 0.0, 1.0)).astype(np.float32)
    med = np.array([median_f32(img1[..., c]) for c in range(3)], dtype=np.float32)
    img2 = (img1.astype(np.float64) + (med - img1).astype(np.float64) * np.clip(mask, 0.0, 1.0)).astype(np.float32)
    if parts is not None:
        parts.update(img1=img1, med=med)
    return np.clip(np.rint(img2), 0, 255).astype(np.uint8)


PAD_DESC = 16          # int32 words per frame of the device table (align_pad.hip): ox oy W0 H0 w h radius + 9 offsets into the two tables


def pad_tables(items):
    """The device tables of a batch of padded frames.  items: per frame ((ox, oy, W0, H0) the window in its frame, (left, top, right, bottom),
    blur).  -> (desc int32 [B, 16], itab int32, dtab fp64, wmax, hmax, stats).  Per frame, itab holds the index maps (no fold and no division
    on the device): extrow[k + r] = the window row behind padded row k, k in [-r, h + r) (scipy's fold, then numpy's); colmap[x] the window
    column of padded column x; extcol[k + r] = scipy's fold of padded column k; colneed[x] = 1 where a horizontal tap of a blurred column
    lands.  dtab holds the weights w[0 .. r] and the four clip profiles: clip(3 max(mx, my) + 1) = max of the per-axis clips (monotone).
    stats: per frame the shares of the horizontal and vertical blur that the clip == 0 interior skips."""
    desc, itab, dtab, stats = np.zeros((len(items), PAD_DESC), dtype=np.int32), [], [], []
    ni = nd = 0

    def put(tab, a, n):
        tab.append(a)
        return n + a.size

    for b, (window, pad, blur) in enumerate(items):
        ox, oy, W0, H0 = (int(v) for v in window)
        left, top, right, bottom = pad = _check_pad((H0, W0), pad, blur)
        w, h = W0 + left + right, H0 + top + bottom
        weights, r = gaussian_weights(blur)
        extrow = _fold_numpy(_fold_scipy(np.arange(-r, h + r), h) - top, H0).astype(np.int32)
        colmap = _fold_numpy(np.arange(w) - left, W0).astype(np.int32)
        extcol = _fold_scipy(np.arange(-r, w + r), w).astype(np.int32)
        mx, my = pad_profiles(W0, H0, pad)
        c1x, c1y = np.clip(mx * 3.0 + 1.0, 0.0, 1.0), np.clip(my * 3.0 + 1.0, 0.0, 1.0)
        c2x, c2y = np.clip(mx, 0.0, 1.0), np.clip(my, 0.0, 1.0)
        colneed = np.zeros(w, dtype=np.int32)
        xs = np.nonzero(c1x > 0)[0]
        colneed[extcol[xs[:, None] + np.arange(2 * r + 1)[None, :]].ravel()] = 1
        desc[b, :7] = (ox, oy, W0, H0, w, h, r)
        for k, a in enumerate((extrow, colmap, extcol, colneed)):
            desc[b, 7 + k] = ni
            ni = put(itab, a, ni)
        for k, a in enumerate((weights[:r + 1], c1x, c1y, c2x, c2y)):
            desc[b, 11 + k] = nd
            nd = put(dtab, np.ascontiguousarray(a, dtype=np.float64), nd)
        fy, fx, fn = float((c1y > 0).mean()), float((c1x > 0).mean()), float(colneed.mean())
        stats.append({"hblur_skipped": (1 - fy) * (1 - fx), "vblur_skipped": (1 - fy) * (1 - fn)})
    wmax, hmax = (int(desc[:, 4].max()), int(desc[:, 5].max())) if len(items) else (0, 0)
    return desc, np.concatenate(itab), np.concatenate(dtab), wmax, hmax, stats


def _lanczos(x):
    def sinc(t):
        if t == 0.0:
            return 1.0
        t = t * math.pi
        return math.sin(t) / t
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x, a=-0.5):
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}          # Resample.c: the filter function and its support


@functools.lru_cache(maxsize=64)
def resample_taps(n_in, n_out, filter="lanczos"):
    """PIL's tap table of one axis resized n_in -> n_out (Resample.c: precompute_coeffs + normalize_coeffs_8bpc), in Python floats, for the
    LANCZOS filter or for BICUBIC (``filter="bicubic"``: what Image.resize takes when it is given no filter):
    bounds int32 [n_out, 2] = (first input index, tap count) and taps int32 [n_out, ksize], 22-bit fixed point.  An unchanged axis
    (PIL skips its pass) gets the identity table."""
    n_in, n_out = int(n_in), int(n_out)
    if filter not in _FILTERS:
        raise ValueError(f"resample_taps: filter must be one of {sorted(_FILTERS)}, got {filter!r}")
    fn, fsupport = _FILTERS[filter]
    if n_in == n_out:
        return np.stack([np.arange(n_out), np.ones(n_out, dtype=np.int64)], 1).astype(np.int32), np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = filterscale = n_in / n_out
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    taps = np.zeros((n_out, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, xmax)
        taps[i, :xmax] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return bounds, taps


def load_image(path_or_array):
    """A frame as uint8 HWC with 3 or 4 channels (other PIL modes become RGB)."""
    if isinstance(path_or_array, (str, os.PathLike)):
        from PIL import Image
        im = Image.open(path_or_array)
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)
    a = np.asarray(path_or_array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"frames are uint8 [H, W, 3 | 4] arrays or image paths, got {a.dtype} {a.shape}")
    return a


class Aligner:
    """The device half of the alignment: ``align(frames, landmarks)`` -> (crops uint8 [B, S, S, 3] on the device, quads fp64 [B, 4, 2]).
    Frames are uint8 HWC arrays (RGB or RGBA; alpha is not read: the reference keeps ``crop.convert("RGB")``, and its frames are opaque), image
    paths, or uint8 HWC tensors that are on the device already (they are not copied to the host); frames of one size share one launch, and those whose plan shrinks go through the LANCZOS resampler first."""

    def __init__(self, output_size=1024, enable_padding=False, device="cuda", pad_edges=False):
        if enable_padding:
            raise NotImplementedError("Aligner does not take enable_padding: crop_image's padding is the keyword pad_edges=True")
        self.S, self.device = int(output_size), torch.device(device)
        self._taps = {}
        self.pad_edges, self.pad_scratch_bytes = bool(pad_edges), PAD_SCRATCH_BYTES
        self.padded = []          # the frames of the last align() call whose crop window was padded

    def _dev_taps(self, n_in, n_out):
        key = (n_in, n_out)
        if key not in self._taps:
            self._taps[key] = tuple(torch.from_numpy(a).to(self.device) for a in resample_taps(n_in, n_out))
        return self._taps[key]

    def _upload(self, arrays):
        if torch.is_tensor(arrays[0]):          # frames that are on the device already stay there
            return torch.stack([a.to(self.device) for a in arrays])
        return torch.from_numpy(np.stack(arrays)).pin_memory().to(self.device, non_blocking=True)

    def resize(self, frames_u8, size):
        """PIL's ``resize(size, LANCZOS)`` of device frames uint8 [B, H, W, C] to size = (w, h)."""
        B, H, W, C = frames_u8.shape
        w, h = size
        tmp = torch.empty((B, H, w, C), dtype=torch.uint8, device=self.device)
        out = torch.empty((B, h, w, C), dtype=torch.uint8, device=self.device)
        ops.resample_u8(frames_u8.contiguous(), self._dev_taps(W, w), self._dev_taps(H, h), tmp, out)()
        return out

    def align(self, frames, landmarks=None, quads=None, scale=1.0):
        frames = [f if torch.is_tensor(f) else load_image(f) for f in frames]
        if (landmarks is None) == (quads is None):
            raise ValueError("Aligner.align takes either landmarks [B, 68, 2] or quads [B, 4, 2]")
        if quads is None:
            quads = np.stack([quad_from_landmarks(lm, scale)[3] for lm in landmarks]) if len(frames) else np.zeros((0, 4, 2))
        quads = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
        if len(quads) != len(frames):
            raise ValueError(f"{len(quads)} quads for {len(frames)} frames")
        plans = [crop_plan(q, (f.shape[1], f.shape[0]), self.S) for q, f in zip(quads, frames)]
        pads = [pad_plan(p, self.S) if self.pad_edges else None for p in plans]
        self.padded = [i for i, p in enumerate(pads) if p is not None]
        crops = torch.empty((len(frames), self.S, self.S, 3), dtype=torch.uint8, device=self.device)
        source = list(frames)          # per frame: the host array, or its shrunk image on the device
        groups = {}
        for i, (f, p) in enumerate(zip(frames, plans)):
            if p.shrink > 1:
                groups.setdefault((tuple(f.shape), p.rsize), []).append(i)
        for (_, rsize), members in groups.items():
            small = self.resize(self._upload([frames[i] for i in members]), rsize)
            for k, i in enumerate(members):
                source[i] = small[k]
        groups, pad_groups = {}, {}
        for i, s in enumerate(source):          # one launch per (resized) frame size: all frames of a video share one
            (groups if pads[i] is None else pad_groups).setdefault(tuple(s.shape), []).append(i)
        for members in pad_groups.values():
            self._align_padded(members, source, plans, pads, crops)
        for members in groups.values():
            fr = self._stack(source, members)
            co = torch.from_numpy(np.stack([plans[i].coeffs for i in members])).to(self.device)
            win = torch.tensor([plans[i].window for i in members], dtype=torch.int32, device=self.device)
            out = torch.empty((len(members), self.S, self.S, 3), dtype=torch.uint8, device=self.device)
            ops.align_quad_u8(fr, co, out, windows=win)()
            crops.index_copy_(0, torch.tensor(members, device=self.device), out)
        self.quads = quads
        return crops, quads

    def _stack(self, source, members):
        first = source[members[0]]
        return torch.stack([source[i] for i in members]) if isinstance(first, torch.Tensor) else self._upload([source[i] for i in members])

    def pad(self, frames_u8, items):
        """crop_image's padding of device frames uint8 [B, H, W, 3 | 4]; items as for pad_tables (window, pads, blur per frame).
        -> (padded uint8 [B, hmax, wmax, 3] with frame b's image in the top-left corner, sizes [(w, h)])."""
        desc, itab, dtab, wmax, hmax, _ = pad_tables(items)
        B = len(items)
        d, it, dt = (torch.from_numpy(a).to(self.device) for a in (desc, itab, dtab))
        out = torch.empty((B, hmax, wmax, 3), dtype=torch.uint8, device=self.device)
        scratch = torch.empty(2 * B * hmax * wmax * 3, dtype=torch.float32, device=self.device)
        select = torch.empty(B * ops.PAD_SELECT_WORDS, dtype=torch.int32, device=self.device)
        ops.align_pad_u8(frames_u8, d, it, dt, scratch, select, out)()
        return out, [(int(r[4]), int(r[5])) for r in desc]

    def _align_padded(self, members, source, plans, pads, crops):
        """The frames of one size whose plan pads: sub-batches of as many as pad_scratch_bytes holds (a frame that exceeds it alone runs
        alone), each one launch sequence of rf_align_pad_u8 and one rf_align_quad_u8 over the padded images."""
        batches, cur, wm, hm = [], [], 0, 0
        for i in members:
            w, h = pads[i].size
            if cur and (len(cur) + 1) * max(wm, w) * max(hm, h) * 27 > self.pad_scratch_bytes:
                batches.append(cur)
                cur, wm, hm = [], 0, 0
            cur.append(i)
            wm, hm = max(wm, w), max(hm, h)
        batches.append(cur)
        for sub in batches:
            padded, sizes = self.pad(self._stack(source, sub), [(plans[i].window, pads[i].pad, pads[i].blur) for i in sub])
            co = torch.from_numpy(np.stack([pads[i].coeffs for i in sub])).to(self.device)
            win = torch.tensor([(0, 0, w, h) for w, h in sizes], dtype=torch.int32, device=self.device)
            out = torch.empty((len(sub), self.S, self.S, 3), dtype=torch.uint8, device=self.device)
            ops.align_quad_u8(padded, co, out, windows=win)()
            crops.index_copy_(0, torch.tensor(sub, device=self.device), out)

    def inverse_transforms(self, quads=None):
        """Per frame, the 8 PERSPECTIVE coefficients of the paste-back (what the reference stores in ``<video>_inv_transforms.npy``)."""
        quads = self.quads if quads is None else np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
        return np.stack([alignment_coefficients(q, self.S) for q in quads]) if len(quads) else np.zeros((0, 8))


# ---- landmark sources of the front-ends ------------------------------------------------------------------------------------------------
def load_landmarks(path, n=None):
    """A landmarks file: fp64 [N, 68, 2] (``n`` rows expected), or [68, 2] for one image (returned as [1, 68, 2])."""
    a = np.asarray(np.load(path), dtype=np.float64)
    if a.shape == (68, 2):
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (68, 2):
        raise ValueError(f"{path}: expected landmarks of shape [N, 68, 2], got {a.shape}")
    if n is not None and len(a) != n:
        raise ValueError(f"{path}: {len(a)} landmark rows for {n} images")
    return a


def dlib_available(predictor_path=DLIB_PREDICTOR):
    """None when dlib imports and its 68-landmark predictor file exists, else the reason it cannot be used."""
    try:
        import dlib  # noqa: F401
    except ImportError:
        return "dlib is not installed"
    return None if os.path.isfile(predictor_path) else f"dlib's predictor file {predictor_path} does not exist"


def dlib_landmarks(paths, predictor_path=DLIB_PREDICTOR):
    """get_landmark (alignmengt.py:39-82) of every image: the first detected face's 68 points, or a NaN row where no face is found."""
    import dlib
    predictor, detector = dlib.shape_predictor(predictor_path), dlib.get_frontal_face_detector()
    out = np.full((len(paths), 68, 2), np.nan)
    for i, p in enumerate(paths):
        img = dlib.load_rgb_image(p)
        dets = detector(img)
        if len(dets):
            out[i] = [[pt.x, pt.y] for pt in predictor(img, dets[0]).parts()]
    return out


def landmarks_for(paths, landmarks_file, what):
    """The landmarks of `paths` from `landmarks_file` when given, else from dlib; raises ValueError naming what is missing."""
    if landmarks_file:
        if not os.path.isfile(landmarks_file):
            raise ValueError(f"landmarks file {landmarks_file} ({what}) does not exist")
        return load_landmarks(landmarks_file, len(paths))
    why = dlib_available()
    if why:
        raise ValueError(f"no landmarks for {what}: give a landmarks .npy file, or install dlib ({why})")
    return dlib_landmarks(paths)


def fill_missing(landmarks):
    """Per row, the index of the row whose face it uses: itself when its landmarks are finite, else the last finite row before it (the
    reference's ``except`` branch keeps the previous frame's crop and transform).  A non-finite first row is an error."""
    ok = np.isfinite(np.asarray(landmarks, dtype=np.float64).reshape(len(landmarks), -1)).all(axis=1)
    if len(ok) and not ok[0]:
        raise ValueError("the first image has no face (non-finite landmarks): there is no earlier crop to reuse")
    src, last = [], 0
    for i, good in enumerate(ok):
        last = i if good else last
        src.append(last)
    return src


def align_to_disk(paths, landmarks, out_paths, output_size=1024, batch=10, device="cuda", pad_edges=False, padded=None):
    """Align every image of `paths` by its landmarks and write the crops as PNGs to `out_paths` (a row without a face repeats the previous
    crop).  Returns the inverse transforms fp64 [N, 8].  ``pad_edges``: crop_image's padding for faces at the frame's edge; the list
    ``padded`` then receives the indices (into `paths`) of the images whose crop was padded."""
    from .pasteback import PngWriter
    src = fill_missing(landmarks)
    faces = sorted(set(src))
    al, writer = (Aligner(output_size, device=device, pad_edges=True) if pad_edges else Aligner(output_size, device=device)), PngWriter()
    users = {}
    for i, s in enumerate(src):
        users.setdefault(s, []).append(i)
    inv = np.zeros((len(paths), 8))
    try:
        for k in range(0, len(faces), batch):
            ids = faces[k:k + batch]
            crops, quads = al.align([paths[i] for i in ids], landmarks=[landmarks[i] for i in ids])
            host, coeffs = crops.cpu().numpy(), al.inverse_transforms(quads)
            if padded is not None:
                padded.extend(u for j in al.padded for u in users[ids[j]])
            for j, i in enumerate(ids):
                for u in users[i]:
                    inv[u] = coeffs[j]
                    writer.submit(out_paths[u], host[j])
    finally:
        writer.close()
    return inv
