#!/usr/bin/env python3
"""Identity-score throughput (reface_amd/idscore.py): rf_id_prep_u8 + the ArcFace engine + rf_id_retrieve on device-resident bytes, timed
with HIP events around whole runs (no decode, no copies), for N sources and M results of 512 x 512 in batches of 50, in fp32 and bf16;
rf_id_retrieve alone; the wall time of the CLI (eval_tool/ID_retrieval/ID_retrieval.py, a fresh process: imports, weights, engine builds, PNG
decode in the loader's workers, upload, scoring) on folders of 512 x 512 PNGs next to its own `scoring_s` (decode to scores, engines already
built), so the host share is visible; and how far bf16 moves the metric on the
test fixture (tests/golden/idscore.npz) from fp32.  One JSON line.

Usage: python tools/idscore_rate.py [--n 1000] [--batch 50] [--iters 3] [--warmup 1] [--cli-images 100] [--num-workers 8]
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
from reface_amd import idscore as S  # noqa: E402
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


def device_rates(precision, n, batch, iters, warmup, sd):
    scorer = S.IDScorer(sd, precision=precision, batch=batch)
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (batch, 512, 512, 3), dtype=torch.uint8, generator=g).cuda()
    lab = torch.randint(0, 19, (batch, 512, 512), dtype=torch.uint8, generator=g).cuda()
    keep = scorer.lut(S.preserve_labels("celeba"))
    nb = (2 * n + batch - 1) // batch          # sources + results
    feats = torch.empty((nb * batch, 512), dtype=torch.float32, device="cuda")
    x = scorer.net.id_input(batch)

    def prep_only():
        for _ in range(nb):
            ops.id_prep_u8(img, lab, keep, x)()

    def embed():
        for b in range(nb):
            ops.id_prep_u8(img, lab, keep, x)()
            feats[b * batch:(b + 1) * batch] = scorer.net.forward_id112(x)[0]

    f_src = torch.nn.functional.normalize(P.seeded_randn((n, 512), 5), dim=1).cuda()
    f_res = torch.nn.functional.normalize(P.seeded_randn((n, 512), 6), dim=1).cuda()
    labels = torch.arange(n, dtype=torch.int32, device="cuda")
    top5 = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    rank = torch.empty((n,), dtype=torch.int32, device="cuda")
    sim = torch.empty((n,), dtype=torch.float64, device="cuda")
    totals = torch.empty((4,), dtype=torch.float64, device="cuda")
    retrieve = ops.id_retrieve(f_res, f_src, labels, top5, rank, sim, totals)
    t_prep = events(prep_only, iters, warmup)
    t_embed = events(embed, iters, warmup)
    t_ret = events(retrieve, max(iters, 10), warmup)
    return {"prep_ms": round(t_prep, 3), "prep_arcface_ms": round(t_embed, 2), "retrieve_ms": round(t_ret, 3),
            "images_per_s": round(2 * n * 1000.0 / (t_embed + t_ret), 1)}


def cli_wall(n, batch, workers):
    from PIL import Image
    g = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, d) for d in ("src", "res", "src_mask", "res_mask")]
        for p in paths:
            os.makedirs(p)
        yy, xx = np.mgrid[0:512, 0:512]
        for i in range(n):
            for pi, pm in ((paths[0], paths[2]), (paths[1], paths[3])):
                base = g.integers(0, 256, (16, 16, 3), dtype=np.uint8)
                Image.fromarray(base).resize((512, 512), Image.BILINEAR).save(os.path.join(pi, f"{i}.png"))
                Image.fromarray((((yy // 64) + (xx // 64) + i) % 19).astype(np.uint8)).save(os.path.join(pm, f"{i}.png"))
        cmd = [sys.executable, os.path.join(ROOT, "eval_tool", "ID_retrieval", "ID_retrieval.py"), "--device", "cuda"] + paths + [
            "--dataset", "celeba", "--arcface", "True", "--arcface_ckpt", "none", "--batch-size", str(batch), "--num-workers", str(workers),
            "--json", os.path.join(tmp, "o.json")]
        t0 = time.perf_counter()
        subprocess.run(cmd, check=True, capture_output=True, timeout=1200)
        wall = time.perf_counter() - t0
        r = json.load(open(os.path.join(tmp, "o.json")))
    return {"images": r["images"], "wall_s": round(wall, 2), "scoring_s": round(r["seconds"], 2), "scoring_images_per_s": round(r["images_per_s"], 1)}


def fixture_shift(sd):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import idscore_inputs as I
    g = np.load(os.path.join(ROOT, "tests", "golden", "idscore.npz"))
    d = I.build()
    keep = S.preserve_labels(I.DATASET)
    out = {"reference": {"top1": float(g["top1"]), "top5": float(g["top5"]), "mean": round(float(g["mean"]), 6)}}
    for prec in ("full", "bf16"):
        sc = S.IDScorer(sd, precision=prec, batch=16)
        f_src = sc.embed_u8(torch.from_numpy(np.stack(d["src_images"])), torch.from_numpy(np.stack(d["src_labels"])), keep)
        f_res = sc.embed_u8(torch.from_numpy(np.stack(d["res_images"])), torch.from_numpy(np.stack(d["res_labels"])), keep)
        r = sc.score(f_src, f_res, d["labels"])
        out[prec] = {"top1": r["top1"], "top5": r["top5"], "mean": round(r["mean"], 6),
                     "max_similarity_shift": float(np.abs(r["similarities"] - g["similarities"]).max()),
                     "max_feature_shift": float(np.abs(torch.cat([f_src, f_res]).cpu().numpy() - np.concatenate([g["f_src"], g["f_res"]])).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cli-images", type=int, default=100, help="images per folder of the CLI wall-time run (0 = skip)")
    ap.add_argument("--num-workers", type=int, default=min(8, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    sd = S.load_arcface_state("none")
    out = {"metric": "idscore_images_per_s", "n_sources": a.n, "n_results": a.n, "batch": a.batch, "image": "512x512"}
    for prec in ("full", "bf16"):
        out[prec] = device_rates(prec, a.n, a.batch, a.iters, a.warmup, sd)
    out["fixture"] = fixture_shift(sd)
    if a.cli_images:
        out["cli"] = cli_wall(a.cli_images, a.batch, a.num_workers)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
