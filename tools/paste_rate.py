#!/usr/bin/env python3
"""Paste-back throughput: frames/s of stage 3's device half (reface_amd/csrc/pasteback.hip) at 1080p, timed with HIP events around whole
batches: rf_paste_crop_u8 (512^2 fp32 result -> 1024^2 u8 crop) + rf_paste_back_u8 (RGB frames -> RGBA), data already on the device (no PNG
decode / encode, no copies).  One JSON line.

Usage: python tools/paste_rate.py [--batch 10] [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reface_amd import ops  # noqa: E402
from reface_amd.pasteback import alignment_coefficients  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B, H, W, S = a.batch, 1080, 1920, 1024
    g = torch.Generator().manual_seed(0)
    x = torch.rand((B, 3, 512, 512), generator=g).cuda()
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()
    quad = np.array([[700.0, 200.0], [640.0, 860.0], [1300.0, 920.0], [1360.0, 260.0]])          # a ~660 px face, slightly rotated
    coeffs = torch.from_numpy(np.stack([alignment_coefficients(quad + 3 * i, S) for i in range(B)])).cuda()
    crops = torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
    launches = [ops.paste_crop_u8(x, crops), ops.paste_back_u8(crops, coeffs, frames, out)]
    for _ in range(a.warmup):
        ops.run(launches)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        ops.run(launches)
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1) / a.iters
    print(json.dumps({"metric": "paste_back_frames_per_s", "batch": B, "frame": f"{W}x{H}", "crop": S, "ms_per_batch": round(ms, 3),
                      "frames_per_s": round(B * 1000.0 / ms, 1)}))


if __name__ == "__main__":
    main()
