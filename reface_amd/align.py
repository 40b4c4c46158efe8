"""Stage 1's face alignment from 68 landmarks on: the FFHQ recipe of the reference (src/utils/alignmengt.py: compute_transform, crop_image,
crop_faces), with its per-frame PIL pixel work reproduced byte for byte by two HIP kernels (reface_amd/csrc/align.hip):

  c, x, y = compute_transform(landmarks)                    quad_from_landmarks      (host, fp64, the reference's order of operations)
  quad    = [c - x - y, c - x + y, c + x + y, c + x - y]
  shrink  = floor(qsize / output_size / 2); when > 1: img.resize(rsize, ANTIALIAS), quad /= shrink          crop_plan + rf_resample_u8
  img.crop(bounding box of the quad + border); quad -= its corner                                          crop_plan (a window, no copy)
  img.transform((S, S), QUAD, (quad + 0.5).flatten(), BILINEAR)                                            rf_align_quad_u8
  inverse transform = calc_alignment_coefficients(quad + 0.5, crop corners)                                pasteback.alignment_coefficients

Landmark DETECTION is not built: landmarks come from a file, or from dlib where it is installed (dlib_landmarks).  ``enable_padding`` of
crop_image (reflect pad + blur + median fill; off in every caller of the reference) is not built either.
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

CropPlan = namedtuple("CropPlan", "shrink rsize window quad coeffs")


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
    coeffs  quad_coefficients(quad, output_size)."""
    if enable_padding:
        raise NotImplementedError("crop_image's enable_padding (reflect pad, blur, median fill) is not built; no caller of the reference turns it on")
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
    return CropPlan(shrink, rsize, window, quad, quad_coefficients(quad, output_size))


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

    def __init__(self, output_size=1024, enable_padding=False, device="cuda"):
        if enable_padding:
            raise NotImplementedError("crop_image's enable_padding (reflect pad, blur, median fill) is not built; no caller of the reference turns it on")
        self.S, self.device = int(output_size), torch.device(device)
        self._taps = {}

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
        groups = {}
        for i, s in enumerate(source):          # one launch per (resized) frame size: all frames of a video share one
            groups.setdefault(tuple(s.shape), []).append(i)
        for members in groups.values():
            first = source[members[0]]
            fr = torch.stack([source[i] for i in members]) if isinstance(first, torch.Tensor) else self._upload([source[i] for i in members])
            co = torch.from_numpy(np.stack([plans[i].coeffs for i in members])).to(self.device)
            win = torch.tensor([plans[i].window for i in members], dtype=torch.int32, device=self.device)
            out = torch.empty((len(members), self.S, self.S, 3), dtype=torch.uint8, device=self.device)
            ops.align_quad_u8(fr, co, out, windows=win)()
            crops.index_copy_(0, torch.tensor(members, device=self.device), out)
        self.quads = quads
        return crops, quads

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


def align_to_disk(paths, landmarks, out_paths, output_size=1024, batch=10, device="cuda"):
    """Align every image of `paths` by its landmarks and write the crops as PNGs to `out_paths` (a row without a face repeats the previous
    crop).  Returns the inverse transforms fp64 [N, 8]."""
    from .pasteback import PngWriter
    src = fill_missing(landmarks)
    faces = sorted(set(src))
    al, writer = Aligner(output_size, device=device), PngWriter()
    users = {}
    for i, s in enumerate(src):
        users.setdefault(s, []).append(i)
    inv = np.zeros((len(paths), 8))
    try:
        for k in range(0, len(faces), batch):
            ids = faces[k:k + batch]
            crops, quads = al.align([paths[i] for i in ids], landmarks=[landmarks[i] for i in ids])
            host, coeffs = crops.cpu().numpy(), al.inverse_transforms(quads)
            for j, i in enumerate(ids):
                for u in users[i]:
                    inv[u] = coeffs[j]
                    writer.submit(out_paths[u], host[j])
    finally:
        writer.close()
    return inv
