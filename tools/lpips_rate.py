#!/usr/bin/env python3
"""LPIPS throughput (reface_amd/lpips.py): rf_lpips_prep_u8 + the feature stack + five rf_lpips_layer + rf_lpips_total on device-resident
512 x 512 bytes, timed with HIP events around whole runs (no decode, no copies), for 'alex' and 'vgg'; and every rf_lpips_layer launch of
the engine alone, as GB/s of feature bytes read (2 maps x pairs x pixels x channels x 4: each byte is read once).  The comparison point of
those figures is the read-only line of tools/bw_probe.py on the same box.  Before timing, one pair per net is checked against lpips_host in
float64 on the same bytes and the difference printed.  The shader-clock probe of bench.py (tools/libclockprobe.so, where built) is read on the
idle chip and right behind the timed windows, so the figures carry the clock they were taken at.  One JSON line.

Usage: python tools/lpips_rate.py [--nets alex,vgg] [--pairs 8] [--iters 20] [--layer-iters 200] [--rounds 3] [--warmup 2] [--size 512] [--no-check]
"""
import argparse
import ctypes
import json
import os
import sys

import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reface_amd import lpips as LP  # noqa: E402
from reface_amd import ops  # noqa: E402


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


PROBE_ITERS = 20000
_PROBE = []


def clock_reading():
    """Shader clock as dependent-FMA iterations per 10 ns tick (tools/clock_probe.hip: a one-wave FMA chain timed against the constant 100 MHz
    counter), queued on the current stream right behind whatever was launched last; None when the probe library is not built."""
    if not _PROBE:
        path = os.path.join(ROOT, "tools", "libclockprobe.so")
        lib = None
        if os.path.exists(path):
            lib = ctypes.CDLL(path)
            lib.clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        _PROBE.append(lib)
    if _PROBE[0] is None:
        return None
    out = torch.zeros((2,), dtype=torch.int64, device="cuda")
    _PROBE[0].clock_probe(out.data_ptr(), PROBE_ITERS, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return PROBE_ITERS / float(out[0])


def images(n, size, seed):
    """Smooth uint8 images [n, size, size, 3]: a 16 x 16 random grid upsampled, so that the pairs are neither noise nor equal."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n, 3, 16, 16), generator=g)
    x = torch.nn.functional.interpolate(base, size=(size, size), mode="bilinear", align_corners=False)
    return (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def self_check(scorer, sd, net, x, y):
    r = scorer.distances_u8(x[:1].cuda(), y[:1].cuda())
    d, v = r.d, r.layers
    want = LP.distances_host(sd, torch.from_numpy(LP.prep_host(x[0].numpy()))[None], torch.from_numpy(LP.prep_host(y[0].numpy()))[None], net)
    rel = float((np.abs(v.cpu().numpy() - want) / want).max())
    print(f"[lpips_rate] {net}: d = {float(d[0]):.6f}, max rel |GPU - float64 host| over the five layers = {rel:.2e}", file=sys.stderr, flush=True)
    return rel


def rates(net, pairs, size, iters, layer_iters, rounds, warmup, check):
    sd = LP.load_lpips_state("none", net)
    scorer = LP.LPIPSScorer(sd, net=net, batch=pairs)
    B = scorer.step((size, size))
    x, y = images(B, size, 1), images(B, size, 2)
    out = {"net": net, "pairs": B, "image": f"{size}x{size}"}
    if check:
        out["check_rel_vs_float64"] = self_check(scorer, sd, net, x, y)
    eng = scorer.engine(B, size, size)
    xd, yd = x.cuda(), y.cuda()
    prep_x, prep_y = ops.lpips_prep_u8(xd, eng.x[:B]), ops.lpips_prep_u8(yd, eng.x[B:])

    def whole():
        prep_x()
        prep_y()
        eng.run()

    ts = [events(whole, iters, warmup) for _ in range(rounds)]
    under_load = clock_reading()          # right behind the last timed window
    out["ms_per_run"] = [round(t, 3) for t in ts]
    out["images_per_s"] = round(2 * B * 1000.0 / sorted(ts)[len(ts) // 2], 1)
    layers = []
    taps = [(h, w, c) for k, h, w, c in LP.layer_shapes(net, size, size) if k == "tap"]
    for launch, (h, w, c) in zip([l for l in eng.launches if l.name.startswith("lpips_layer")], taps):
        ms = sorted(events(launch, layer_iters, warmup) for _ in range(rounds))[rounds // 2]
        nbytes = 2 * B * h * w * c * 4
        layers.append({"layer": launch.name, "hw": h * w, "c": c, "mbytes": round(nbytes / 1e6, 2), "ms": round(ms, 4), "gb_per_s": round(nbytes / ms / 1e6, 1)})
    out["layers"] = layers
    out["layers_ms"] = round(sum(l["ms"] for l in layers), 3)
    after_layers = clock_reading()
    out["clock_fma_iters_per_tick"] = {"behind_whole_runs": under_load and round(under_load, 4), "behind_layer_launches": after_layers and round(after_layers, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", type=str, default="alex,vgg")
    ap.add_argument("--pairs", type=int, default=8, help="pairs per engine run (capped per net and size: no tensor reaches 2^31 bytes)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20, help="engine runs per timed window")
    ap.add_argument("--layer-iters", type=int, default=200, help="launches per timed window of one rf_lpips_layer")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per figure: every whole-run time is printed, the median makes the rate")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-check", action="store_true", help="skip the float64 host check (VGG16 at 512 x 512 takes the host a while)")
    a = ap.parse_args()
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    time.sleep(0.5)
    idle = clock_reading()          # the idle chip after a pause: the probe's one wave runs at the boost clock
    out = {"metric": "lpips_images_per_s", "clock_fma_iters_per_tick_idle": idle and round(idle, 4), "device": [rates(n, a.pairs, a.size, a.iters, a.layer_iters, a.rounds, a.warmup, not a.no_check) for n in a.nets.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
