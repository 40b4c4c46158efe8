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

``--parallel`` adds the self-synchronising plan (``JpegDecoder(parallel=True)``): every workload is decoded, in the same child process and
in alternating rounds, on the plans it takes today ("serial" / "intervals": the decoder without the switch) and with the switch, one JSON
line per setting: the sub-sequences, the files that took the new plan, the sync launches they needed, the fallbacks to the serial lane, the
event time of every kernel, and the time of each round (the spread).  ``--subseq-bytes 64,128,256 --sync-launches 2,4,8`` sweeps the
settings on the workloads without restart markers; the two workloads with restart markers run at the defaults only (they do not take the plan).

Usage: python tools/jpegdec_rate.py [--iters 20] [--rounds 3] [--parallel [--subseq-bytes L,..] [--sync-launches K,..]] [--out out/jpegdec_rate]
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


NO_RESTARTS = ("celeba1024", "pil512")


def settings(a):
    """The decoder settings a workload is timed on: None (no switch), then (subseq_bytes, sync_launches) of --parallel."""
    from reface_amd.jpegdec import SUBSEQ_BYTES, SYNC_LAUNCHES
    if not a.parallel:
        return [None]
    if a.workload not in NO_RESTARTS:
        return [None, (SUBSEQ_BYTES, SYNC_LAUNCHES)]
    ls = [int(v) for v in a.subseq_bytes.split(",")] if a.subseq_bytes else [SUBSEQ_BYTES]
    ks = [int(v) for v in a.sync_launches.split(",")] if a.sync_launches else [SYNC_LAUNCHES]
    return [None] + [(L, K) for L in ls for K in ks]


def child_gpu(a):
    import torch
    from PIL import Image
    from reface_amd.jpegdec import JpegDecoder, parse_jpeg
    batch = files(a.workload, os.path.dirname(a.files_out))
    want = [np.asarray(Image.open(io.BytesIO(f))) for f in batch]
    infos = [parse_jpeg(f) for f in batch]
    raw = sum(i.height * i.width * i.ncomp for i in infos)
    runs = []
    for cfg in settings(a):
        dec = JpegDecoder("cuda") if cfg is None else JpegDecoder("cuda", parallel=True, subseq_bytes=cfg[0], sync_launches=cfg[1])
        job = dec.decode_async(batch)
        outs = job.result()
        for k, (o, w) in enumerate(zip(outs, want)):
            assert np.array_equal(o.cpu().numpy(), w), (cfg, k)
        dec.decode(batch)          # (warm: the staging buffer is pooled from here on)
        runs.append({"cfg": cfg, "dec": dec, "report": job.report, "wall": [], "event": []})
    torch.cuda.synchronize()
    for _ in range(a.rounds):          # the settings alternate, so that a drift of the box meets all of them
        for r in runs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            t0.record()
            for _ in range(a.iters):
                r["dec"].decode(batch)
            t1.record()
            t1.synchronize()
            r["wall"].append((time.perf_counter() - w0) / a.iters * 1e3)
            r["event"].append(t0.elapsed_time(t1) / a.iters)
    for r in runs:
        # the kernels, by events around each launch
        dec, per = r["dec"], None
        for _ in range(a.iters):
            L = dec._launch(batch, infos, [i.ncomp for i in infos], timing=True)
            L.event.synchronize()
            dec._release(L.staging)
            t = np.array([L.events[k].elapsed_time(L.events[k + 1]) for k in range(len(L.event_names))])
            per = t if per is None else per + t
        per /= a.iters
        rep = r["report"]
        wall, ev = float(np.median(r["wall"])), float(np.median(r["event"]))
        line = {"metric": "gpu_jpeg_decode", "workload": a.workload, "files": len(batch), "jpeg_bytes": sum(len(f) for f in batch), "raw_bytes": raw,
                "where": sorted({x["where"] for x in rep}), "plan": sorted({x["plan"] for x in rep}), "intervals": L.nivl, "lanes_per_wave": L.lanes,
                "iters": a.iters, "rounds": a.rounds, "wall_ms_per_batch": round(wall, 3), "event_ms_per_batch": round(ev, 3),
                "wall_ms_rounds": [round(v, 3) for v in r["wall"]], "event_ms_rounds": [round(v, 3) for v in r["event"]],
                "files_per_s": round(len(batch) / wall * 1e3, 1), "kernel_ms": {n: round(float(v), 3) for n, v in zip(L.event_names, per)}}
        if r["cfg"] is None:
            line["setting"] = "no switch"
        else:
            took = [x for x in rep if "subseqs" in x]
            line.update(setting="parallel", subseq_bytes=r["cfg"][0], sync_launches=r["cfg"][1], selfsync_files=len(took), subseqs=sum(x["subseqs"] for x in took),
                        launches_used=sorted({x["launches_used"] for x in took}), fallbacks=sum(x["fallback"] for x in took))
        print(json.dumps(line), flush=True)
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
    ap.add_argument("--rounds", type=int, default=3, help="timed windows of --iters batches per setting; their times are printed, the median is the figure")
    ap.add_argument("--parallel", action="store_true", help="also time JpegDecoder(parallel=True): the self-synchronising plan of files without restart markers")
    ap.add_argument("--subseq-bytes", dest="subseq_bytes", type=str, default=None, help="--parallel: sub-sequence sizes to sweep, e.g. 64,128,256")
    ap.add_argument("--sync-launches", dest="sync_launches", type=str, default=None, help="--parallel: sync launch counts to sweep, e.g. 2,4,8")
    ap.add_argument("--workloads", type=str, default=",".join(WORKLOADS), help="the workloads to run")
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

    extra = ["--rounds", str(a.rounds)] + (["--parallel"] if a.parallel else [])
    for key, val in (("--subseq-bytes", a.subseq_bytes), ("--sync-launches", a.sync_launches)):
        extra += [key, val] if val else []
    for wl in a.workloads.split(","):
        if wl not in WORKLOADS:
            raise SystemExit(f"jpegdec_rate: --workloads: {wl} is none of {', '.join(WORKLOADS)}")
        fo = os.path.join(a.out, wl + ".files.pkl")
        keep(run_child(me + ["--child", "gpu", "--workload", wl, "--iters", str(a.iters), "--files-out", fo] + extra, 600))
        keep(run_child(me + ["--child", "host", "--workload", wl, "--iters", str(max(2, a.iters // 4)), "--files-out", fo], 300))
        os.remove(fo)
    with open(os.path.join(a.out, "jpegdec_rate.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
