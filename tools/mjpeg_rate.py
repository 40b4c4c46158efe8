#!/usr/bin/env python3
"""GPU JPEG encoder rate (reface_amd/csrc/jpegenc.hip) against PIL (libjpeg-turbo) on the same images, inputs resident on the device:

  frames : ten 1080p RGBA frames (a photo-like frame with a flat border), one encode call
  bench  : a test-bench-like batch of eight 512 x 512 RGB images, one encode call

Per workload: HIP events over --iters enqueued encodes (blocks + entropy + pack, nothing fetched), the wall time and process CPU-seconds of
--iters complete encodes (bytes fetched, headers joined), the shader-clock probe of bench.py (tools/libclockprobe.so, where built) read
right behind the timed window, in a separate child under rocprofv3 --kernel-trace --stats the time per kernel, and in a third child PIL on
the same images (quality and subsampling as on the device, one restart interval per MCU row): one process, and 16 processes -- what a node
that feeds 8 ranks has per rank is less -- with wall time and CPU-seconds of both.  The device files are compared with PIL's, byte for
byte, before anything is timed.  Every run is a child process under its own time limit.  One JSON line per measurement.

Usage: python tools/mjpeg_rate.py [--iters 100] [--quality 90] [--subsampling 420] [--out out/mjpeg_rate] [--no-rocprof]
"""
import argparse
import csv
import ctypes
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
from pngenc_refs import photo_like  # noqa: E402  (the photo-like test content of the encoders' tests: one definition)

HOST_PROCS = 16
PROBE_ITERS = 20000


def workload(name):
    """-> uint8 array [B, H, W, C]"""
    if name == "bench":
        return np.stack([photo_like(512, 512, 3, 10 + b) for b in range(8)])
    frames = np.stack([np.concatenate([photo_like(1080, 1920, 3, b), np.full((1080, 1920, 1), 255, np.uint8)], axis=2) for b in range(10)])
    frames[:, :60] = np.array([16, 16, 16, 255], dtype=np.uint8)
    frames[:, -60:] = np.array([16, 16, 16, 255], dtype=np.uint8)
    return frames


def pil_jpeg(img, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).convert("RGB").save(buf, "JPEG", quality=quality, subsampling={"420": 2, "444": 0}[subsampling], restart_marker_rows=1)
    return buf.getvalue()


def clock_reading():
    """Shader clock as dependent-FMA iterations per 10 ns tick (tools/clock_probe.hip), queued on the current stream right behind whatever
    was launched last; None when the probe library is not built."""
    import torch
    path = os.path.join(ROOT, "tools", "libclockprobe.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    lib.clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    out = torch.zeros((2,), dtype=torch.int64, device="cuda")
    lib.clock_probe(out.data_ptr(), PROBE_ITERS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return round(PROBE_ITERS / float(out[0]), 3)


def child_gpu(a):
    import torch
    from reface_amd.mjpeg import JpegEncoder
    imgs = workload(a.workload)
    x = torch.from_numpy(imgs).cuda()
    enc = JpegEncoder("cuda", a.quality, a.subsampling)
    files = enc.encode(x)
    same = sum(f == pil_jpeg(im, a.quality, a.subsampling) for f, im in zip(files, imgs))
    job = enc.encode_async(x)          # warm: the scratch exists, nothing is allocated inside the timed loops
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        job.discard()
        job = enc.encode_async(x)
    t1.record()
    t1.synchronize()
    clock = clock_reading()
    job.discard()
    ms = t0.elapsed_time(t1) / a.iters
    w0, c0 = time.perf_counter(), time.process_time()
    for _ in range(a.iters):
        enc.encode(x)
    wall, cpu = (time.perf_counter() - w0) / a.iters, (time.process_time() - c0) / a.iters
    clock2 = clock_reading()
    print(json.dumps({"metric": "gpu_jpeg_encode", "workload": a.workload, "files": len(files), "shape": list(imgs.shape), "quality": a.quality,
                      "subsampling": a.subsampling, "raw_bytes": int(imgs.size), "jpeg_bytes": sum(len(f) for f in files), "equal_to_pil": f"{same}/{len(files)}",
                      "iters": a.iters, "event_ms_per_batch": round(ms, 4), "event_files_per_s": round(len(files) / ms * 1e3, 1),
                      "fetched_wall_ms_per_batch": round(wall * 1e3, 3), "fetched_cpu_s_per_batch": round(cpu, 5),
                      "fetched_files_per_s": round(len(files) / wall, 1), "clock_after_events": clock, "clock_after_fetch": clock2}))


_WORK = {}


def _pil_init(name, quality, subsampling):
    """Every worker holds the images itself: nothing but an index crosses the pipe."""
    _WORK.update(imgs=workload(name), quality=quality, subsampling=subsampling)


def _pil_one(k):
    """-> (file bytes, CPU-seconds of this encode in its process)"""
    c0 = time.process_time()
    n = len(pil_jpeg(_WORK["imgs"][k], _WORK["quality"], _WORK["subsampling"]))
    return n, time.process_time() - c0


def child_host(a):
    import multiprocessing as mp
    _pil_init(a.workload, a.quality, a.subsampling)
    work = list(range(len(_WORK["imgs"])))
    iters = max(1, a.iters // 10)
    w0, c0 = time.perf_counter(), time.process_time()
    for _ in range(iters):
        sizes = [_pil_one(w)[0] for w in work]
    wall1, cpu1 = (time.perf_counter() - w0) / iters, (time.process_time() - c0) / iters
    many = work * HOST_PROCS          # every process has a batch's worth to do
    with mp.Pool(HOST_PROCS, initializer=_pil_init, initargs=(a.workload, a.quality, a.subsampling)) as pool:
        pool.map(_pil_one, many[:HOST_PROCS])          # the workers exist and have PIL loaded before the clock starts
        w0, cpu16 = time.perf_counter(), 0.0
        for _ in range(iters):
            cpu16 += sum(c for _, c in pool.map(_pil_one, many, chunksize=len(work)))
        wall16 = (time.perf_counter() - w0) / iters / HOST_PROCS          # per batch
    cpu16 = cpu16 / iters / HOST_PROCS
    print(json.dumps({"metric": "pil_jpeg_encode", "workload": a.workload, "files": len(work), "jpeg_bytes": sum(sizes), "iters": iters,
                      "one_process_wall_ms_per_batch": round(wall1 * 1e3, 3), "one_process_cpu_s_per_batch": round(cpu1, 5),
                      "one_process_files_per_s": round(len(work) / wall1, 1), "processes": HOST_PROCS,
                      "many_process_wall_ms_per_batch": round(wall16 * 1e3, 3), "many_process_cpu_s_per_batch": round(cpu16, 5),
                      "many_process_files_per_s": round(len(work) / wall16, 1)}))


def run_child(args, limit):
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"mjpeg_rate: child {' '.join(args[-4:])} did not finish within {limit} s and was killed; no further GPU work is started")
    if r.returncode != 0:
        raise SystemExit(f"mjpeg_rate: child {' '.join(args[-4:])} failed (rc={r.returncode}); no further GPU work is started\n" + r.stdout[-800:] + r.stderr[-1500:])
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", type=str, default="420", choices=["420", "444"])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "out", "mjpeg_rate"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", type=str, default=None, choices=["gpu", "host"])
    ap.add_argument("--workload", type=str, default="frames", choices=["frames", "bench"])
    a = ap.parse_args()
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

    for wl in ("frames", "bench"):
        common = ["--workload", wl, "--quality", str(a.quality), "--subsampling", a.subsampling]
        keep(run_child(me + ["--child", "gpu", "--iters", str(a.iters)] + common, 300))
        if not a.no_rocprof:          # a run of its own: the kernel trace slows the host side, so its numbers are not mixed with the event timing
            d = os.path.join(a.out, "trace_" + wl)
            run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me + ["--child", "gpu", "--iters", "10"] + common, 600)
            stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
            per = {}
            for row in csv.DictReader(open(stats[0])) if stats else []:
                if "jpeg_" in row.get("Name", ""):
                    per[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
            keep(json.dumps({"metric": "gpu_jpeg_kernels", "workload": wl, "kernels": per}))
        keep(run_child(me + ["--child", "host", "--iters", str(a.iters)] + common, 600))
    with open(os.path.join(a.out, "mjpeg_rate.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
