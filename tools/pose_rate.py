#!/usr/bin/env python3
"""Pose-score throughput (reface_amd/posescore.py): rf_pose_prep_u8 + the ResNet-50 engine + rf_pose_head + rf_pose_distance on
device-resident bytes, timed with HIP events around whole runs (no decode, no copies), for N targets and N results of 512 x 512, per batch
size; the three kernels alone; and the wall time of the CLI (eval_tool/Pose/pose_compare.py, a fresh process: imports, weights, engine
builds, PNG decode in the loader's workers, upload, scoring) on folders of 512 x 512 PNGs next to its own `scoring_s` (decode to score,
engines already built), so the host share is visible.  One JSON line.

Usage: python tools/pose_rate.py [--n 1000] [--batches 20,50] [--iters 2] [--warmup 1] [--cli-images 100] [--num-workers 8]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reface_amd import ops  # noqa: E402
from reface_amd import posescore as PS  # noqa: E402
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


def device_rates(n, batch, iters, warmup, sd):
    scorer = PS.PoseScorer(sd, batch=batch)
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (batch, 512, 512, 3), dtype=torch.uint8, generator=g).cuda()
    nb = (2 * n + batch - 1) // batch          # targets + results
    deg = torch.empty((nb * batch, 3), dtype=torch.float32, device="cuda")
    eng = scorer.engine(batch)
    prep = ops.pose_prep_u8(img, eng.x)
    head = eng.launches[-1]

    def prep_only():
        for _ in range(nb):
            prep()

    def head_only():
        for _ in range(nb):
            head()

    def degrees():
        for b in range(nb):
            prep()
            deg[b * batch:(b + 1) * batch] = eng.run()

    d_t = P.seeded_randn((n, 3), 5, 20.0).cuda()
    d_r = P.seeded_randn((n, 3), 6, 20.0).cuda()
    labels = torch.arange(n, dtype=torch.int32, device="cuda")
    dist = torch.empty((n,), dtype=torch.float64, device="cuda")
    totals = torch.empty((2,), dtype=torch.float64, device="cuda")
    distance = ops.pose_distance(d_r, d_t, labels, dist, totals)
    t_prep = events(prep_only, iters, warmup)
    t_head = events(head_only, iters, warmup)
    t_deg = events(degrees, iters, warmup)
    t_dist = events(distance, max(iters, 10), warmup)
    return {"batch": batch, "prep_ms": round(t_prep, 3), "head_ms": round(t_head, 3), "prep_hopenet_ms": round(t_deg, 2), "distance_ms": round(t_dist, 4),
            "images_per_s": round(2 * n * 1000.0 / (t_deg + t_dist), 1)}


def cli_wall(n, batch, workers):
    from PIL import Image
    g = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, d) for d in ("targets", "results")]
        for p in paths:
            os.makedirs(p)
        for i in range(n):
            for p in paths:
                base = g.integers(0, 256, (16, 16, 3), dtype=np.uint8)
                Image.fromarray(base).resize((512, 512), Image.BILINEAR).save(os.path.join(p, f"{i}.png"))
        cmd = [sys.executable, os.path.join(ROOT, "eval_tool", "Pose", "pose_compare.py"), "--device", "cuda"] + paths + [
            "--hopenet_ckpt", "none", "--batch-size", str(batch), "--num-workers", str(workers), "--json", os.path.join(tmp, "o.json")]
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, capture_output=True, timeout=1200)
        wall = time.perf_counter() - t0
        r = json.load(open(os.path.join(tmp, "o.json")))
    return {"images": r["images"], "batch": batch, "wall_s": round(wall, 2), "scoring_s": round(r["seconds"], 2), "scoring_images_per_s": round(r["images_per_s"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--batches", type=str, default="20,50")
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cli-images", type=int, default=100, help="images per folder of the CLI wall-time run (0 = skip)")
    ap.add_argument("--num-workers", type=int, default=min(8, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    sd = PS.load_hopenet_state("none")
    out = {"metric": "posescore_images_per_s", "n_targets": a.n, "n_results": a.n, "image": "512x512"}
    out["device"] = [device_rates(a.n, int(b), a.iters, a.warmup, sd) for b in a.batches.split(",")]
    if a.cli_images:
        out["cli"] = cli_wall(a.cli_images, 20, a.num_workers)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
