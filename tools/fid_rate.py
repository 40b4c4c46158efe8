#!/usr/bin/env python3
"""FID throughput (reface_amd/fidscore.py): rf_fid_prep_u8 + the ViT-B/32-sized vision tower on device-resident bytes, timed with HIP events
around whole runs (no decode, no copies), per precision at the CLI's batch of 50 for 512 x 512 images, and rf_fid_stats alone at
(30000, 512), the size of the reference's dataset folder.  Seeded weights; the clock figure of the box is printed beside the times.  One JSON
line.

Usage: python tools/fid_rate.py [--batch 50] [--batches 4] [--rounds 3] [--warmup 1] [--stats-n 30000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reface_amd import fidscore as FS  # noqa: E402
from reface_amd import ops  # noqa: E402
from reface_amd import params as P  # noqa: E402


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--batches", type=int, default=4, help="engine runs per timed run")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stats-n", type=int, default=30000)
    a = ap.parse_args()
    sd = FS.seeded_fid_state(P.CLIPVisionConfig(**FS.VIT_B32))
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (a.batch, 512, 512, 3), dtype=torch.uint8, generator=g).cuda()
    scorers = {p: FS.FidScorer(sd, precision=p, batch=a.batch) for p in ("full", "bf16")}
    runs = {}
    for tag, sc in scorers.items():
        def run(sc=sc):
            for _ in range(a.batches):
                sc.features_u8(img)
        runs[tag] = run
    ms = {tag: [] for tag in runs}
    clocks = []
    for r in range(a.rounds):
        for tag in runs:
            ms[tag].append(round(events(runs[tag], 1, a.warmup if r == 0 else 0), 3))
            clocks.append(clock_mhz())
    feat = P.seeded_randn((a.stats_n, 512), 5).cuda()
    mu = torch.empty((512,), dtype=torch.float64, device="cuda")
    sigma = torch.empty((512, 512), dtype=torch.float64, device="cuda")
    t_stats = events(ops.fid_stats(feat, mu, sigma), 5, 1)
    eng = scorers["full"].engine(a.batch)
    out = {"metric": "fidscore_images_per_s", "image": "512x512", "batch": a.batch, "batches": a.batches, "launches": len(eng.launches), "ms": ms,
           "stats_n": a.stats_n, "stats_ms": round(t_stats, 4), "clock_mhz": clocks}
    for tag in runs:
        out[f"images_per_s_{tag}"] = round(a.batches * a.batch * 1000.0 / min(ms[tag]), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
