#!/usr/bin/env python3
"""Face-parser throughput: images/s of the BiSeNet engine (reface_amd/parsing.py) on 1024^2 uint8 crops already on the device, timed with
HIP events around whole batches (prep + network + head; no host decode, no copies).  Seeded weights.  One JSON line.

Usage: python tools/parse_rate.py [--batch 16] [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reface_amd import ops  # noqa: E402
from reface_amd.parsing import FaceParser  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    parser = FaceParser("none", max_batch=a.batch)
    eng = parser._engine(a.batch, 1024, 1024)
    eng.x_u8.copy_(torch.randint(0, 256, tuple(eng.x_u8.shape), dtype=torch.uint8))
    launches = eng.body + [eng.heads[True]]
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
    print(json.dumps({"metric": "face_parser_images_per_s", "batch": a.batch, "crop": 1024, "ms_per_batch": round(ms, 3),
                      "images_per_s": round(a.batch * 1000.0 / ms, 1), "launches_per_batch": len(launches)}))


if __name__ == "__main__":
    main()
