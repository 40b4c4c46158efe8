#!/usr/bin/env python3
"""GPU PNG encoder rate (reface_amd/csrc/pngenc.hip) against PIL on the same images, inputs resident on the device:

  bench  : one test-bench batch -- 8 images x (five 512 x 512 x 3 panels + the 516 x 2058 x 3 grid), photo-like content + a mask panel
  frames : ten 1080p RGBA frames (a photo-like frame with a flat border)

Per workload: HIP events over --iters encodes (filter + deflate + pack of the whole workload), in a separate child under rocprofv3
--kernel-trace --stats the time per kernel, in a third child the thread-seconds of PIL.Image.save at level 6 and at level 1 for the same
images, and the file sizes of all three.  Every run is a child process under its own time limit.  One JSON line per measurement.

Usage: python tools/png_rate.py [--iters 200] [--out out/png_rate] [--no-rocprof]
"""
import argparse
import csv
import glob
import io
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pngenc_refs import photo_like  # noqa: E402  (the photo-like test content of the encoder's tests: one definition)


def workload(name):
    """-> list of uint8 arrays [B, H, W, C] (one encode call each)"""
    if name == "bench":
        B, S = 8, 512
        panels = [np.stack([photo_like(S, S, 3, 10 * k + b) for b in range(B)]) for k in range(4)]
        mask = np.full((B, S, S, 3), 127, dtype=np.uint8)
        mask[:, 100:400, 130:380] = 255
        grid = np.zeros((B, S + 4, 4 * S + 10, 3), dtype=np.uint8)
        for k in range(4):
            grid[:, 2:2 + S, 2 + k * (S + 2):2 + k * (S + 2) + S] = panels[k]
        return panels[:1] + [mask] + panels[1:] + [grid]
    frames = np.stack([np.concatenate([photo_like(1080, 1920, 3, b), np.full((1080, 1920, 1), 255, np.uint8)], axis=2) for b in range(10)])
    frames[:, :60] = np.array([16, 16, 16, 255], dtype=np.uint8)
    frames[:, -60:] = np.array([16, 16, 16, 255], dtype=np.uint8)
    return [frames]


def child_events(a):
    import torch
    from reface_amd.pngenc import PngEncoder
    sets = [torch.from_numpy(s).cuda() for s in workload(a.workload)]
    enc = PngEncoder("cuda")
    files = [f for s in sets for f in enc.encode(s)]
    from PIL import Image
    for f, img in zip(files, [im for s in workload(a.workload) for im in s]):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), img)
    jobs = [enc.encode_async(s) for s in sets]          # warm: scratch of every shape exists, nothing is allocated inside the timed loop
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        for j in jobs:
            j.discard()
        jobs = [enc.encode_async(s) for s in sets]
    t1.record()
    t1.synchronize()
    raw = sum(s.numel() for s in sets)
    ms = t0.elapsed_time(t1) / a.iters
    print(json.dumps({"metric": "gpu_png_encode", "workload": a.workload, "files": len(files), "raw_bytes": raw, "png_bytes": sum(len(f) for f in files),
                      "iters": a.iters, "ms_per_workload": round(ms, 4), "raw_GB_per_s": round(raw / ms / 1e6, 2)}))


def child_host(a):
    from PIL import Image
    imgs = [im for s in workload(a.workload) for im in s]
    out = {"metric": "pil_png_encode", "workload": a.workload, "files": len(imgs)}
    for level in (6, 1):
        t0, n = time.thread_time(), 0
        for im in imgs:
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, format="PNG", compress_level=level)
            n += buf.tell()
        out[f"level{level}_thread_s"] = round(time.thread_time() - t0, 3)
        out[f"level{level}_png_bytes"] = n
    print(json.dumps(out))


def run_child(args, limit, env=None):
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=limit, cwd=ROOT, env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"png_rate: child {' '.join(args[-4:])} did not finish within {limit} s and was killed; no further GPU work is started")
    if r.returncode != 0:
        raise SystemExit(f"png_rate: child {' '.join(args[-4:])} failed (rc={r.returncode}); no further GPU work is started\n" + r.stdout[-800:] + r.stderr[-1500:])
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "out", "png_rate"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", type=str, default=None, choices=["events", "host"])
    ap.add_argument("--workload", type=str, default="bench", choices=["bench", "frames"])
    a = ap.parse_args()
    if a.child == "events":
        return child_events(a)
    if a.child == "host":
        return child_host(a)
    os.makedirs(a.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    lines = []
    for wl in ("bench", "frames"):
        for line in run_child(me + ["--child", "events", "--workload", wl, "--iters", str(a.iters)], 300).splitlines():
            if line.startswith("{"):
                lines.append(line)
                print(line, flush=True)
        if not a.no_rocprof:          # a run of its own: the kernel trace slows the host side, so its numbers are not mixed with the event timing
            d = os.path.join(a.out, "trace_" + wl)
            run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "events", "--workload", wl, "--iters", "20"], 600)
            stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
            per = {}
            for row in csv.DictReader(open(stats[0])) if stats else []:
                if "png_" in row.get("Name", ""):
                    per[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
            line = json.dumps({"metric": "gpu_png_kernels", "workload": wl, "kernels": per})
            lines.append(line)
            print(line, flush=True)
        for line in run_child(me + ["--child", "host", "--workload", wl], 600).splitlines():
            if line.startswith("{"):
                lines.append(line)
                print(line, flush=True)
    with open(os.path.join(a.out, "png_rate.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
