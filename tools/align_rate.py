#!/usr/bin/env python3
"""Alignment throughput: stage 1's device half (reface_amd/csrc/align.hip) for a batch of 1080p frames and S = 1024, timed with HIP events
around whole batches, data already on the device (no PNG decode / encode, no copies):
  plain   rf_align_quad_u8 of a ~660 px face (no shrink: what a 1080p video needs)
  shrink  rf_resample_u8 (LANCZOS, 1920x1080 -> 960x540) + rf_align_quad_u8 of the shrunk frames -- the work a shrink-2 plan costs; at
          S = 1024 the reference takes that branch only for faces >= 4096 px, so the 1080p frames stand in for larger ones
and the same two jobs in PIL on the host (one thread, as the reference runs them).  One JSON line.

`pad` as the first argument times crop_image's enable_padding branch instead (reface_amd/csrc/align_pad.hip): ten 1080p frames with a ~660 px
face crossing the left edge, rf_align_pad_u8 + rf_align_quad_u8 per batch and each kernel group of rf_align_pad_u8 on its own, against the
host recipe (np.pad, scipy.ndimage.gaussian_filter, np.median, PIL's QUAD; one thread) on the same frames, whose bytes the device run must equal.

Usage: python tools/align_rate.py [pad] [--batch 10] [--iters 20] [--warmup 3] [--host-iters 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reface_amd import ops  # noqa: E402
from reface_amd.align import Aligner, quad_coefficients  # noqa: E402


def timed(launches, iters, warmup):
    for _ in range(warmup):
        ops.run(launches)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        ops.run(launches)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def host_padded_crop(frame, plan, pp, S):
    """crop_image's padding branch and transform with numpy / scipy / PIL themselves, one frame."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    ox, oy, w0, h0 = plan.window
    left, top, right, bottom = pp.pad
    img = np.pad(np.float32(frame[oy:oy + h0, ox:ox + w0]), ((top, bottom), (left, right), (0, 0)), "reflect")
    h, w = img.shape[:2]
    y, x = np.ogrid[:h, :w]
    mask = np.maximum(1.0 - np.minimum(np.float32(x) / np.int64(left), np.float32(w - 1 - x) / np.int64(right)),
                      1.0 - np.minimum(np.float32(y) / np.int64(top), np.float32(h - 1 - y) / np.int64(bottom)))[..., None]
    img += (gaussian_filter(img, [pp.blur, pp.blur, 0]) - img) * np.clip(mask * 3.0 + 1.0, 0.0, 1.0)
    img += (np.median(img, axis=(0, 1)) - img) * np.clip(mask, 0.0, 1.0)
    padded = np.uint8(np.clip(np.rint(img), 0, 255))
    return np.asarray(Image.fromarray(padded).transform((S, S), Image.QUAD, (pp.quad + 0.5).flatten(), Image.BILINEAR))


def pad_job(a):
    from reface_amd.align import crop_plan, pad_plan, pad_tables
    B, H, W, S = a.batch, 1080, 1920, 1024
    g = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (B, H // 8, W // 8, 3), dtype=torch.uint8, generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
    frames = host.cuda()
    quad = np.array([[0.0, 200.0], [-60.0, 860.0], [600.0, 920.0], [660.0, 260.0]])          # a ~660 px face over the left edge, slightly rotated
    quads = [quad + 3 * i for i in range(B)]
    plans = [crop_plan(q, (W, H), S) for q in quads]
    pps = [pad_plan(p, S) for p in plans]
    assert all(p.shrink <= 1 for p in plans) and all(pp is not None for pp in pps)
    t0 = time.perf_counter()
    desc, itab, dtab, wmax, hmax, stats = pad_tables([(p.window, pp.pad, pp.blur) for p, pp in zip(plans, pps)])
    t_tables = (time.perf_counter() - t0) * 1e3
    d, it, dt = (torch.from_numpy(x).cuda() for x in (desc, itab, dtab))
    out = torch.empty((B, hmax, wmax, 3), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(2 * B * hmax * wmax * 3, dtype=torch.float32, device="cuda")
    select = torch.empty(B * ops.PAD_SELECT_WORDS, dtype=torch.int32, device="cuda")
    coeffs = torch.from_numpy(np.stack([pp.coeffs for pp in pps])).cuda()
    win = torch.tensor([(0, 0) + pp.size for pp in pps], dtype=torch.int32, device="cuda")
    crops = torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda")
    pad = lambda stages: ops.align_pad_u8(frames, d, it, dt, scratch, select, out, stages=stages)          # noqa: E731
    quad_launch = ops.align_quad_u8(out, coeffs, crops, windows=win)
    whole = timed([pad(15), quad_launch], a.iters, a.warmup)
    parts = {name: timed([pad(bit)], a.iters, a.warmup) for name, bit in ops.PAD_STAGES.items()}          # (each on what the whole run left in the scratch)
    parts["align_quad"] = timed([quad_launch], a.iters, a.warmup)
    ops.run([pad(15), quad_launch])
    got = crops.cpu().numpy()
    best, same = float("inf"), True
    for _ in range(a.host_iters):
        t0 = time.perf_counter()
        ref = [host_padded_crop(f, p, pp, S) for f, p, pp in zip(host.numpy(), plans, pps)]
        best = min(best, (time.perf_counter() - t0) * 1e3)
        same = same and all(np.array_equal(r, c) for r, c in zip(ref, got))
    print(json.dumps({"metric": "align_pad_ms_per_batch", "batch": B, "frame": f"{W}x{H}", "crop": S, "padded": f"{wmax}x{hmax}",
                      "radius": pps[0].radius, "device_ms": round(whole, 3), "kernels_ms": {k: round(v, 3) for k, v in parts.items()},
                      "tables_host_ms": round(t_tables, 2), "host_recipe_ms": round(best, 1), "host_bytes_equal": bool(same),
                      "hblur_skipped": round(float(np.mean([s["hblur_skipped"] for s in stats])), 4),
                      "vblur_skipped": round(float(np.mean([s["vblur_skipped"] for s in stats])), 4)}))
    if not same:
        sys.exit("align_rate pad: the device crops differ from the host recipe's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("job", nargs="?", default="align", choices=("align", "pad"))
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    a = ap.parse_args()
    if a.job == "pad":
        return pad_job(a)
    B, H, W, S = a.batch, 1080, 1920, 1024
    g = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    frames = host.cuda()
    quad = np.array([[700.0, 200.0], [640.0, 860.0], [1300.0, 920.0], [1360.0, 260.0]])          # a ~660 px face, slightly rotated
    quads = [quad + 3 * i for i in range(B)]
    coeffs = torch.from_numpy(np.stack([quad_coefficients(q, S) for q in quads])).cuda()
    crops = torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda")
    plain = timed([ops.align_quad_u8(frames, coeffs, crops)], a.iters, a.warmup)
    al = Aligner(S)
    w, h = W // 2, H // 2
    tmp = torch.empty((B, H, w, 3), dtype=torch.uint8, device="cuda")
    small = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
    coeffs2 = torch.from_numpy(np.stack([quad_coefficients(q / 2, S) for q in quads])).cuda()
    resample = ops.resample_u8(frames, al._dev_taps(W, w), al._dev_taps(H, h), tmp, small)
    t_res = timed([resample], a.iters, a.warmup)
    t_al2 = timed([ops.align_quad_u8(small, coeffs2, crops)], a.iters, a.warmup)
    from PIL import Image
    imgs = [Image.fromarray(f) for f in host.numpy()]
    pil = {}
    for name, shrink in (("plain", 1), ("shrink", 2)):
        best = float("inf")
        for _ in range(a.host_iters):
            t0 = time.perf_counter()
            for im, q in zip(imgs, quads):
                if shrink > 1:
                    im = im.resize((w, h), Image.LANCZOS)
                im.transform((S, S), Image.QUAD, (q / shrink + 0.5).flatten(), Image.BILINEAR)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        pil[name] = best
    print(json.dumps({"metric": "align_ms_per_batch", "batch": B, "frame": f"{W}x{H}", "crop": S, "align_quad_ms": round(plain, 3),
                      "shrink2_resample_ms": round(t_res, 3), "shrink2_align_quad_ms": round(t_al2, 3),
                      "pil_host_plain_ms": round(pil["plain"], 1), "pil_host_shrink2_ms": round(pil["shrink"], 1),
                      "frames_per_s_plain": round(B * 1000.0 / plain, 1)}))


if __name__ == "__main__":
    main()
