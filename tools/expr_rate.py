#!/usr/bin/env python3
"""Expression-score throughput (reface_amd/exprscore.py): rf_expr_prep_u8 + the ResNet-50 engine at 512 x 512 + rf_expr_head +
rf_expr_distance on device-resident bytes, timed with HIP events around whole runs (no decode, no copies), for N targets and N results of
512 x 512 at the CLI's batch of 50 (two engine batches of 25), once with the fused block tail (conv3's ACT_ADD_RELU epilogue) and once with
``add_relu=True`` (conv3, then rf_add_relu): the A/B of the epilogue.  The two variants alternate, ``--rounds`` times each, and the clock
figure of the box is printed beside them.  One JSON line.

Usage: python tools/expr_rate.py [--n 100] [--batch 50] [--rounds 3] [--warmup 1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reface_amd import exprscore as ES  # noqa: E402
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
    ap.add_argument("--n", type=int, default=100, help="targets (and as many results)")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    sd = ES.load_recon_state("none")
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (a.batch, 512, 512, 3), dtype=torch.uint8, generator=g).cuda()
    nb = (2 * a.n + a.batch - 1) // a.batch          # targets + results
    scorers = {"fused": ES.ExprScorer(sd, batch=a.batch), "add_relu": ES.ExprScorer(sd, batch=a.batch, add_relu=True)}
    runs = {}
    for tag, sc in scorers.items():
        def run(sc=sc):
            for _ in range(nb):
                sc.coeffs_u8(img)
        runs[tag] = run
    c_t = P.seeded_randn((a.n, 257), 5).cuda()
    c_r = P.seeded_randn((a.n, 257), 6).cuda()
    labels = torch.arange(a.n, dtype=torch.int32, device="cuda")
    dist = torch.empty((a.n,), dtype=torch.float64, device="cuda")
    totals = torch.empty((2,), dtype=torch.float64, device="cuda")
    distance = ops.expr_distance(c_r, c_t, labels, dist, totals)
    ms = {tag: [] for tag in runs}
    clocks = []
    for r in range(a.rounds):
        for tag in runs:
            ms[tag].append(round(events(runs[tag], 1, a.warmup if r == 0 else 0), 2))
            clocks.append(clock_mhz())
    t_dist = events(distance, 10, 1)
    eng = scorers["fused"].engine(min(a.batch, ES.ENGINE_B))
    out = {"metric": "exprscore_images_per_s", "n_targets": a.n, "n_results": a.n, "image": "512x512", "batch": a.batch, "engine_batch": eng.B,
           "launches_fused": len(eng.launches), "launches_add_relu": len(scorers["add_relu"].engine(eng.B).launches),
           "ms": ms, "distance_ms": round(t_dist, 4), "clock_mhz": clocks}
    for tag in runs:
        best = min(ms[tag])
        out[f"images_per_s_{tag}"] = round(nb * a.batch * 1000.0 / (best + t_dist), 1)
    out["fused_over_add_relu"] = round(min(ms["fused"]) / min(ms["add_relu"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
