#!/usr/bin/env python3
"""GPU JPEG decoder rate (reface_amd/csrc/jpegdec.hip) against PIL in 1 and in 16 worker processes on the same files, on the same box, in
the same call:

  celeba1024 : 16 files of 1024 x 1024 at 4:2:0 without restart markers, written by PIL (the CelebA-HQ shape): the serial plan
  enc1024    : the same 16 images written by JpegEncoder (one restart interval per MCU row): the interval plan
  frames1080 : ten 1080p frames read back from an AviWriter file (--write_video -> --video_in)
  pil512     : 192 files of 512 x 512 at 4:2:0 without restart markers, written by PIL

Per workload, one JSON line each: the decoder's wall time per batch as a caller sees it (parse, tables, staging, upload, kernels, error
codes), the HIP-event time of the same loop and of each of the three kernels, the plan taken; and the wall time of PIL decoding the same
bytes in one process and in a pool of 16.  Every decoded image is compared with PIL's before anything is timed.  Every run is a child
process under its own time limit.

Usage: python tools/jpegdec_rate.py [--iters 20] [--out out/jpegdec_rate]
"""
import argparse
import io
import json
import os
import pickle
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pngenc_refs import photo_like  # noqa: E402  (the photo-like content of the codec tests: one definition)

WORKLOADS = ("celeba1024", "enc1024", "frames1080", "pil512")
HOST_PROCS = (1, 16)
QUALITY = 90


def files(name, scratch):
    """The batch's JPEG files (bytes); distinct images are repeated up to the batch size."""
    import torch
    from PIL import Image
    from reface_amd import mjpeg as M
    if name in ("celeba1024", "enc1024"):
        imgs, n = np.stack([photo_like(1024, 1024, 3, b) for b in range(16)]), 16
    elif name == "pil512":
        imgs, n = np.stack([photo_like(512, 512, 3, b) for b in range(16)]), 192
    else:
        imgs, n = np.stack([photo_like(1080, 1920, 3, b) for b in range(2)]), 10
    if name == "enc1024":
        distinct = M.JpegEncoder("cuda", QUALITY, "420").encode(torch.from_numpy(imgs).cuda())
    elif name == "frames1080":
        path = os.path.join(scratch, "frames1080.avi")
        vo = M.VideoOutput(path, fps=25.0, quality=QUALITY, device="cuda")
        vo.push(torch.from_numpy(np.stack([imgs[k % len(imgs)] for k in range(n)])).cuda())
        vo.close()
        r = M.AviReader(path)
        distinct = list(r)
        r.close()
        os.remove(path)
    else:
        distinct = []
        for im in imgs:
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, format="JPEG", quality=QUALITY, subsampling=2)
            distinct.append(buf.getvalue())
    return [distinct[k % len(distinct)] for k in range(n)]


def child_gpu(a):
    import torch
    from PIL import Image
    from reface_amd.jpegdec import JpegDecoder, parse_jpeg
    batch = files(a.workload, os.path.dirname(a.files_out))
    dec = JpegDecoder("cuda")
    job = dec.decode_async(batch)
    outs = job.result()
    for k, (o, f) in enumerate(zip(outs, batch)):
        assert np.array_equal(o.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)))), k
    plans = sorted({r["plan"] for r in job.report})
    where = sorted({r["where"] for r in job.report})
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    for _ in range(a.iters):
        dec.decode(batch)
    t1.record()
    t1.synchronize()
    wall = (time.perf_counter() - w0) / a.iters * 1e3
    # the three kernels, by events around each launch
    infos = [parse_jpeg(f) for f in batch]
    per = np.zeros(3)
    for _ in range(a.iters):
        L = dec._launch(batch, infos, [i.ncomp for i in infos], timing=True)
        L.event.synchronize()
        dec._release(L.staging)
        per += [L.events[k].elapsed_time(L.events[k + 1]) for k in range(3)]
    per /= a.iters
    raw = sum(i.height * i.width * i.ncomp for i in infos)
    print(json.dumps({"metric": "gpu_jpeg_decode", "workload": a.workload, "files": len(batch), "jpeg_bytes": sum(len(f) for f in batch), "raw_bytes": raw,
                      "where": where, "plan": plans, "intervals": L.nivl, "lanes_per_wave": L.lanes, "iters": a.iters, "wall_ms_per_batch": round(wall, 3),
                      "event_ms_per_batch": round(t0.elapsed_time(t1) / a.iters, 3), "files_per_s": round(len(batch) / wall * 1e3, 1),
                      "kernel_ms": {"entropy_decode": round(float(per[0]), 3), "idct": round(float(per[1]), 3), "upsample_rgb": round(float(per[2]), 3)}}))
    with open(a.files_out, "wb") as f:          # the same bytes go to the host child
        pickle.dump(batch, f)


def _pil_one(data):
    from PIL import Image
    return int(np.asarray(Image.open(io.BytesIO(data))).sum() & 0)


def child_host(a):
    import multiprocessing as mp
    batch = pickle.load(open(a.files_out, "rb"))
    for procs in HOST_PROCS:
        with mp.Pool(procs) as pool:
            pool.map(_pil_one, batch[:procs])          # the workers exist and have PIL loaded before the clock starts
            t0 = time.perf_counter()
            for _ in range(a.iters):
                pool.map(_pil_one, batch, chunksize=max(1, len(batch) // (4 * procs)))
            wall = (time.perf_counter() - t0) / a.iters * 1e3
        print(json.dumps({"metric": "pil_jpeg_decode", "workload": a.workload, "files": len(batch), "processes": procs, "iters": a.iters,
                          "wall_ms_per_batch": round(wall, 3), "files_per_s": round(len(batch) / wall * 1e3, 1)}), flush=True)


def run_child(args, limit):
    try:
        r = subprocess.run(args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"jpegdec_rate: child {' '.join(args[-4:])} did not finish within {limit} s and was killed; no further GPU work is started")
    if r.returncode != 0:
        raise SystemExit(f"jpegdec_rate: child {' '.join(args[-4:])} failed (rc={r.returncode}); no further GPU work is started\n" + r.stdout[-800:] + r.stderr[-1500:])
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "out", "jpegdec_rate"))
    ap.add_argument("--child", type=str, default=None, choices=["gpu", "host"])
    ap.add_argument("--workload", type=str, default="celeba1024", choices=WORKLOADS)
    ap.add_argument("--files-out", dest="files_out", type=str, default=None)
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

    for wl in WORKLOADS:
        fo = os.path.join(a.out, wl + ".files.pkl")
        keep(run_child(me + ["--child", "gpu", "--workload", wl, "--iters", str(a.iters), "--files-out", fo], 300))
        keep(run_child(me + ["--child", "host", "--workload", wl, "--iters", str(max(2, a.iters // 4)), "--files-out", fo], 300))
        os.remove(fo)
    with open(os.path.join(a.out, "jpegdec_rate.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
