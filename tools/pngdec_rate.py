#!/usr/bin/env python3
"""GPU PNG decoder rate (reface_amd/csrc/pngdec.hip) against PIL in 16 worker processes on the same files, on the same box, in the same call:

  pil512     : 512 x 512 RGB photo-like files written by PIL at level 6 (what the evaluation commands read)
  enc512     : the same images written by the GPU encoder (--gpu_png): the segmented inflate plan
  crop1024   : 1024 x 1024 RGB crops, PIL level 6
  frames1080 : ten 1080p RGBA frames, PIL level 6 (the video callers)

Per workload, one JSON line each: the decoder's wall time per batch as a caller sees it (parse, staging, upload, kernels, error codes) and
the HIP-event time of the same loop, the inflate plan taken; in a child of its own under rocprofv3 --kernel-trace --stats the time per
kernel; and the wall time of PIL decoding the same bytes in a pool of 16 processes.  Every run is a child process under its own time limit.

With --parallel every workload is decoded with the blocks plan off (``PngDecoder(parallel=False)``: the serial plan for PIL's files) and on
(``parallel=True``), the settings alternating in --rounds rounds inside one child; the lines give the median [min .. max] of the rounds per
setting, the plans taken, the chain chunks per file, the false candidates per MB of compressed data and the fallbacks.  frames1080 is also
run at block_bytes 256 and 4096.  PIL decodes the same bytes in 1 and in 16 processes, and the kernel trace is taken with the plan on.

Usage: python tools/pngdec_rate.py [--parallel] [--rounds 5] [--iters 20] [--out out/pngdec_rate] [--no-rocprof]
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
from pngenc_refs import photo_like  # noqa: E402  (the photo-like content of the codec tests: one definition)

WORKLOADS = ("pil512", "enc512", "crop1024", "frames1080")
HOST_PROCS = 16


def images(name):
    """-> (distinct uint8 images [n, H, W, C], files per batch)"""
    if name in ("pil512", "enc512"):
        return np.stack([photo_like(512, 512, 3, b) for b in range(16)]), 192
    if name == "crop1024":
        return np.stack([photo_like(1024, 1024, 3, b) for b in range(4)]), 48
    f = np.stack([np.concatenate([photo_like(1080, 1920, 3, b), np.full((1080, 1920, 1), 255, np.uint8)], axis=2) for b in range(2)])
    return f, 10


def files(name):
    """The batch's PNG files (bytes); distinct images are repeated up to the batch size."""
    from PIL import Image
    imgs, n = images(name)
    if name == "enc512":
        import torch
        from reface_amd.pngenc import PngEncoder
        distinct = PngEncoder("cuda").encode(torch.from_numpy(imgs).cuda())
    else:
        distinct = []
        for im in imgs:
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, format="PNG", compress_level=6)
            distinct.append(buf.getvalue())
    return [distinct[k % len(distinct)] for k in range(n)], imgs


def settings_of(a):
    """(name, PngDecoder keywords) of the settings one GPU child alternates between"""
    out = [("serial", dict(parallel=False))]
    if a.parallel:
        out.append(("blocks", dict(parallel=True)))
        if a.workload == "frames1080":
            out += [(f"blocks{bb}", dict(parallel=True, block_bytes=bb)) for bb in (256, 4096)]
    return [s for s in out if a.only is None or s[0] == a.only]


def child_gpu(a):
    import torch
    from reface_amd.pngdec import PngDecoder
    batch, imgs = files(a.workload)
    png_bytes = sum(len(f) for f in batch)
    raw = sum(int(np.prod(imgs[k % len(imgs)].shape)) for k in range(len(batch)))
    decs, info, times = {}, {}, {}
    for name, kw in settings_of(a):          # every setting decodes the batch once and must give the images
        dec = decs[name] = PngDecoder("cuda", **kw)
        job = dec.decode_async(batch)
        outs = job.result()
        for k, o in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), imgs[k % len(imgs)]), (name, k)
        rep = job.report
        info[name] = {"where": sorted({r["where"] for r in rep}), "plan": sorted({r["plan"] for r in rep})}
        if dec.parallel:
            false = sum(r["candidates"] - r["chunks"] for r in rep if r["plan"] == "blocks")
            info[name].update(block_bytes=dec.block_bytes, chunks_per_file=round(sum(r["chunks"] for r in rep) / len(rep), 1),
                              false_candidates_per_mb=round(false / (png_bytes / 1e6), 3), fallbacks=sum(bool(r["fallback"]) for r in rep))
        times[name] = []
    for _ in range(a.rounds):          # the settings alternate: a drift of the box shows in every one of them
        for name, dec in decs.items():
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for _ in range(a.iters):
                dec.decode(batch)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - w0) / a.iters * 1e3)
    for name, t in times.items():
        med = float(np.median(t))
        print(json.dumps({"metric": "gpu_png_decode", "workload": a.workload, "setting": name, "files": len(batch), "png_bytes": png_bytes, "raw_bytes": raw,
                          **info[name], "rounds": a.rounds, "iters": a.iters, "wall_ms_per_batch": round(med, 3),
                          "wall_ms_range": [round(min(t), 3), round(max(t), 3)], "files_per_s": round(len(batch) / med * 1e3, 1)}))
    with open(a.files_out, "wb") as f:          # the same bytes go to the host child
        import pickle
        pickle.dump(batch, f)


def _pil_one(data):
    from PIL import Image
    return int(np.asarray(Image.open(io.BytesIO(data))).sum() & 0)


def child_host(a):
    import multiprocessing as mp
    import pickle
    batch = pickle.load(open(a.files_out, "rb"))
    with mp.Pool(a.procs) as pool:
        pool.map(_pil_one, batch[:a.procs])          # the workers exist and have PIL loaded before the clock starts
        t0 = time.perf_counter()
        for _ in range(a.iters):
            pool.map(_pil_one, batch, chunksize=max(1, len(batch) // (4 * a.procs)))
        wall = (time.perf_counter() - t0) / a.iters * 1e3
    t1 = time.thread_time()
    for d in batch[:8]:
        _pil_one(d)
    per = (time.thread_time() - t1) / min(8, len(batch)) * 1e3
    print(json.dumps({"metric": "pil_png_decode", "workload": a.workload, "files": len(batch), "processes": a.procs, "iters": a.iters,
                      "wall_ms_per_batch": round(wall, 3), "files_per_s": round(len(batch) / wall * 1e3, 1), "thread_ms_per_file": round(per, 3)}))


def run_child(args, limit):
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"pngdec_rate: child {' '.join(args[-4:])} did not finish within {limit} s and was killed; no further GPU work is started")
    if r.returncode != 0:
        raise SystemExit(f"pngdec_rate: child {' '.join(args[-4:])} failed (rc={r.returncode}); no further GPU work is started\n" + r.stdout[-800:] + r.stderr[-1500:])
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "out", "pngdec_rate"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", type=str, default=None, choices=["gpu", "host"])
    ap.add_argument("--workload", type=str, default="pil512", choices=WORKLOADS)
    ap.add_argument("--files-out", dest="files_out", type=str, default=None)
    ap.add_argument("--parallel", action="store_true", help="also decode with the blocks plan (PngDecoder(parallel=True)), alternating with the serial plan")
    ap.add_argument("--rounds", type=int, default=None, help="rounds the settings alternate in (default: 5 with --parallel, else 1)")
    ap.add_argument("--only", type=str, default=None, help="(child) one setting alone: serial, blocks, blocks256, blocks4096")
    ap.add_argument("--procs", type=int, default=HOST_PROCS, help="(child) PIL's worker processes")
    a = ap.parse_args()
    if a.rounds is None:
        a.rounds = 5 if a.parallel else 1
    if a.child == "gpu":
        return child_gpu(a)
    if a.child == "host":
        return child_host(a)
    os.makedirs(a.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    lines = []

    def keep(text):
        for line in text.splitlines():
            if line.startswith("{"):
                lines.append(line)
                print(line, flush=True)

    for wl in WORKLOADS:
        fo = os.path.join(a.out, wl + ".files.pkl")
        par = ["--parallel"] if a.parallel else []
        keep(run_child(me + ["--child", "gpu", "--workload", wl, "--iters", str(a.iters), "--rounds", str(a.rounds), "--files-out", fo] + par, 900))
        for procs in ((1, HOST_PROCS) if a.parallel else (HOST_PROCS,)):
            keep(run_child(me + ["--child", "host", "--workload", wl, "--iters", str(max(2, a.iters // 4)), "--procs", str(procs), "--files-out", fo], 300))
        if not a.no_rocprof:          # a run of its own: the kernel trace slows the host side, so its numbers are not mixed with the timing above
            d = os.path.join(a.out, "trace_" + wl)
            run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                      ["--child", "gpu", "--workload", wl, "--iters", "5", "--rounds", "1", "--files-out", fo] + (par + ["--only", "blocks"] if par else []), 600)
            stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
            per = {}
            for row in csv.DictReader(open(stats[0])) if stats else []:
                if "png_" in row.get("Name", ""):
                    per[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
            keep(json.dumps({"metric": "gpu_png_decode_kernels", "workload": wl, "setting": "blocks" if par else "serial", "kernels": per}))
        os.remove(fo)
    with open(os.path.join(a.out, "pngdec_rate.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
