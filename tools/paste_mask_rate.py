#!/usr/bin/env python3
"""What the masked paste costs: ten 1080p RGBA frames, 1024^2 crops, 512^2 label maps, data already on the device, timed with HIP events
around many launches in alternating rounds (a drift of the machine meets both settings):

  plain       rf_paste_back_u8
  masked      rf_paste_alpha_u8 (dilate 8, feather 8, 2 passes: 7 launches) + rf_paste_back_alpha_u8
  alpha_only  rf_paste_alpha_u8 alone (the share of `masked` that is the alpha plane)

Both pastes read and write every byte of the frames (83 MB per batch each way), so both are expected to be bound by the frame bytes; the
masked one also does the composite's integer division per covered pixel and reads the alpha plane.  Prints one JSON line: per setting the
median [min .. max] of the rounds in ms per batch, and the bytes the frames alone move over the median time.  The shader clock is
power-managed: a window of a few hundred ms right after an idle period runs faster than a long run, which is why the warm-up is as long as
a round and the rounds alternate.

Usage: python tools/paste_mask_rate.py [--batch 10] [--iters 2000] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reface_amd import ops  # noqa: E402
from reface_amd.pasteback import PasteMask, alignment_coefficients  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2000, help="batches per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per setting; the median is the figure")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paste_mask_rate: no GPU; a time measured elsewhere says nothing about the MI355X")
    B, H, W, S, Sl = a.batch, 1080, 1920, 1024, 512
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, H, W, 4), dtype=torch.uint8, generator=g).cuda()
    crops = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g).cuda()
    yy, xx = np.mgrid[:Sl, :Sl]
    face = np.hypot((yy - 0.52 * Sl) / 1.25, xx - 0.5 * Sl) < 0.3 * Sl          # an oval of repainted labels on a kept background
    labels = torch.from_numpy(np.where(face, 1, 0).astype(np.uint8)).cuda().expand(B, Sl, Sl).contiguous()
    quad = np.array([[700.0, 200.0], [640.0, 860.0], [1300.0, 920.0], [1360.0, 260.0]])          # a ~660 px face, slightly rotated
    coeffs = torch.from_numpy(np.stack([alignment_coefficients(quad + 3 * i, S) for i in range(B)])).cuda()
    mask = PasteMask([1], dilate=8, feather=8, passes=2)
    lut = torch.from_numpy(mask.lut_host).cuda()
    alpha = torch.empty((B, S, S), dtype=torch.uint8, device="cuda")
    scratch = torch.empty(2 * B * Sl * Sl, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, H, W, 4), dtype=torch.uint8, device="cuda")
    settings = {"plain": [ops.paste_back_u8(crops, coeffs, frames, out)],
                "alpha_only": [ops.paste_alpha_u8(labels, lut, alpha, scratch, mask.dilate, mask.feather, mask.passes)],
                "masked": [ops.paste_alpha_u8(labels, lut, alpha, scratch, mask.dilate, mask.feather, mask.passes),
                           ops.paste_back_alpha_u8(crops, alpha, coeffs, frames, out)]}
    for launches in settings.values():          # warm-up: every shape of the timed windows, for as long as a window
        for _ in range(a.iters):
            ops.run(launches)
    torch.cuda.synchronize()
    times = {k: [] for k in settings}
    for _ in range(a.rounds):
        for name, launches in settings.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                ops.run(launches)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.iters)
    frame_bytes = 2 * B * H * W * 4          # read once, written once
    res = {"metric": "paste_mask_ms_per_batch", "batch": B, "frame": f"{W}x{H}x4", "crop": S, "label_map": Sl, "iters": a.iters, "rounds": a.rounds}
    for name, t in times.items():
        med = float(np.median(t))
        res[name] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
        if name != "alpha_only":
            res[name]["frame_GB_per_s"] = round(frame_bytes / med / 1e6, 1)
    res["masked_over_plain"] = round(res["masked"]["median_ms"] / res["plain"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
