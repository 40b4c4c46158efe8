#!/usr/bin/env python3
"""Alignment throughput: stage 1's device half (reface_amd/csrc/align.hip) for a batch of 1080p frames and S = 1024, timed with HIP events
around whole batches, data already on the device (no PNG decode / encode, no copies):
  plain   rf_align_quad_u8 of a ~660 px face (no shrink: what a 1080p video needs)
  shrink  rf_resample_u8 (LANCZOS, 1920x1080 -> 960x540) + rf_align_quad_u8 of the shrunk frames -- the work a shrink-2 plan costs; at
          S = 1024 the reference takes that branch only for faces >= 4096 px, so the 1080p frames stand in for larger ones
and the same two jobs in PIL on the host (one thread, as the reference runs them).  One JSON line.

Usage: python tools/align_rate.py [--batch 10] [--iters 20] [--warmup 3] [--host-iters 2]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    a = ap.parse_args()
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
