#!/usr/bin/env python3
"""bench.py -- REFace hot path on MI355X: 512x512, 50-step DDIM images/sec (BASELINE.json metric).

One "step" = one batch of B synthetic image pairs through the timed region of SURVEY.md section 8d:
  50 x [pack 9-ch input x2 (CFG) -> UNet on 2B samples -> CFG + DDIM update]  +  fp32 KL-VAE decode + clamp.
Inputs (seeded, already resident in HBM): x_T ~ N(0,1), masked-image latent, ellipse keep-mask,
c ~ N(0,1) [B,1,768], learned-uncond vector, scale 3.5, eta 0.  Weights: seeded random init of the exact
REFace architecture (859.5 M-param UNet, 83.7 M-param VAE) -- no checkpoint is obtainable offline.

  python bench.py --gpus N --steps K --warmup W [--config c1|c2|c3|c4] [--dump-outputs DIR] [--full]
N > 1 without a launcher: this process spawns `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child
(before touching the GPU) and relays rank 0's line; under torch.distributed.run it reads RANK / LOCAL_RANK / WORLD_SIZE.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline line; --dump-outputs DIR
also writes what the last timed step computed as DIR/<name>.npy.  Everything else is measured only under --full: `roofline` with HIP
events per launch on the launch stream, the shader clock, the parity modes, the other configs, the conditioning stage, and
`cpu_baseline`, which times the CPU oracle (oracle/) on a bounded sample of the same workload.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F_UNET = {64: 796.94e9, 96: 2137.52e9}   # algorithmic FLOP per sample per UNet evaluation by latent side (SURVEY.md 8d / BASELINE.md 2)
F_VAE_DEC_512 = 2514.5e9      # fp32 VAE decode per 512x512 image
PEAK = {"bf16": 2500.0, "fp16": 2500.0, "f32": 157.3, "fp8": 5000.0, "fp8w": 2500.0, "fp8c": 5000.0}     # dense MFMA TFLOP/s of the instruction the dominant family issues
                                                         # (MI355X_MICROARCH.md): "fp8" = fp8 x fp8 on the MX-scaled fp8 MFMA (5 PF dense);
                                                         # "fp8w" dequantises fp8 weights to bf16 in the LDS read path -> bf16 MFMA rate
# BASELINE.json configs[i] -> per-GPU workload (configs[2] = configs[1] on every one of the N GPUs)
CONFIGS = {
    "c1": dict(idx=1, latent=64, batch=8, dtype="bf16"),
    # configs[1] with the UNet on fp16 storage / v_mfma_f32_32x32x16_f16 instead of bf16: the same kernels, launch list and matrix-core rate; quoted
    # beside the bf16 line because it is the throughput mode closest to the 1e-3 pixel gate (3 more mantissa bits per operand)
    "c1h": dict(idx=1, latent=64, batch=8, dtype="fp16"),
    "c2": dict(idx=2, latent=64, batch=8, dtype="bf16"),
    "c3": dict(idx=3, latent=96, batch=4, dtype="bf16"),
    # configs[4] as BASELINE.json states it ("fp8 MFMA UNet weights"): "fp8" = EVERY eligible UNet GEMM weight e4m3fn + fp8 activations into the
    # convolutions / proj_in / qkv / GEGLU on the fp8 MFMA.  "c4c" = the same config with only the 3x3 convolutions (85 % of the FLOPs) on fp8
    # ("fp8c": bf16 projections) -- 38.7 dB against the fp32 mode where "fp8" gives 30.7 dB, ON SEEDED RANDOM-INIT WEIGHTS (Gaussian weights: per-32-block
    # scales cannot help, profiles/r04a_fp8_weight_scale_ablation.json; the gap does not predict a trained checkpoint).  Both lines are printed.
    "c4": dict(idx=4, latent=64, batch=16, dtype="fp8"),
    "c4c": dict(idx=4, latent=64, batch=16, dtype="fp8c"),
}


DUMP_BYTES = 64_000_000      # --dump-outputs: at most this many bytes of float32 in all


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def dump_outputs(outdir, arrays):
    """Write each tensor of `arrays` as <outdir>/<name>.npy in float32.  When they hold more than DUMP_BYTES in all, each is cut to the
    same share of its flattened elements, picked by a fixed seed (the same indices from run to run)."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    total = 4 * sum(t.numel() for t in arrays.values())
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if total > DUMP_BYTES:
            k = a.size * DUMP_BYTES // total
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, k, replace=False))]
        np.save(os.path.join(outdir, name + ".npy"), a)


def synthetic_inputs(B, h, seed, device):
    from reface_amd.params import seeded_randn as rnd
    x_T = rnd((B, 4, h, h), seed)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(h), indexing="ij")
    ell = (((yy - h / 2) / (0.30 * h)) ** 2 + ((xx - h / 2) / (0.38 * h)) ** 2) <= 1.0
    mask = (~ell).float()[None, None].repeat(B, 1, 1, 1)          # 1 = keep (test_bench_dataset.py:347)
    z_inp = rnd((B, 4, h, h), seed + 1) * mask
    c = rnd((B, 1, 768), seed + 2)
    uc = rnd((1, 1, 768), 7).repeat(B, 1, 1)
    return [t.to(device) for t in (x_T, z_inp, mask, c, uc)]


def build_models(dtype, device, rank, world, keep_cpu_sd):
    """Full-width UNet + VAE with seeded weights; rank 0 generates, RCCL-broadcasts to the other ranks."""
    import types
    from reface_amd import params as P
    from reface_amd.schedule import ddpm_buffers
    from reface_amd.unet import UNetModel
    from reface_amd.vae import AutoencoderKL
    unet = UNetModel(image_size=32, in_channels=9, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                     num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1,
                     context_dim=768, use_checkpoint=True, legacy=False, compute_dtype=dtype)
    vae = AutoencoderKL(ddconfig=dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                                      ch_mult=[1, 2, 4, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0),
                        lossconfig={"target": "torch.nn.Identity"}, embed_dim=4)
    cpu_sd = None
    if rank == 0:
        t0 = time.time()
        usd = P.seeded_state_dict(P.unet_param_specs(unet.cfg), 1234)
        vsd = P.seeded_state_dict(P.vae_param_specs(vae.cfg), 55)
        unet.load_state_dict(usd, strict=True)
        vae.load_state_dict(vsd, strict=True)
        if keep_cpu_sd:
            cpu_sd = (usd, vsd)
        log(f"[bench] seeded weights generated in {time.time() - t0:.1f}s")
    unet.to(device)
    vae.to(device)
    if world > 1:
        from reface_amd.multigpu import broadcast_module
        n = sum(broadcast_module(mod, 0) for mod in (unet, vae))      # a few flat RCCL broadcasts over xGMI
        if rank == 0:
            log(f"[bench] weights broadcast in {n} collectives")
    b = ddpm_buffers(1000, 0.00085, 0.0120)
    ldm = types.SimpleNamespace(num_timesteps=1000, betas=b["betas"], alphas_cumprod=b["alphas_cumprod"],
                                alphas_cumprod_prev=b["alphas_cumprod_prev"], device=torch.device(device),
                                model=types.SimpleNamespace(diffusion_model=unet))
    return unet, vae, ldm, cpu_sd


def cpu_baseline(cpu_sd, cores):
    """Bounded CPU sample of the same workload on the host cores, via the oracle (a port, kind='port'):
    ONE CFG DDIM step (UNet on a CFG batch of 2 at latent 64x64, B = 1 image) + ONE fp32 VAE decode of a
    512x512 image; images/sec = 1 / (50 * t_step + t_decode)."""
    from oracle import unet as ounet, vae as ovae
    from reface_amd import params as P
    # pick the thread count that is actually fastest on this host (all logical CPUs oversubscribe badly)
    from reface_amd.output import available_cpus
    quota = available_cpus()          # the container's CFS quota (the test pool: 16 under a 256-CPU affinity mask): sustained work gets this many CPUs
    best, best_t, probe = cores, float("inf"), {}
    xs, ws = torch.randn(2, 320, 64, 64), torch.randn(320, 320, 3, 3)
    for n in sorted({cores, max(1, cores // 2), max(1, cores // 4), max(1, cores // 8), 32, 16, 8, quota}):
        if n > cores:
            continue
        torch.set_num_threads(n)
        torch.nn.functional.conv2d(xs, ws, padding=1)
        t0, k = time.time(), 0
        while k < 3 or time.time() - t0 < 0.4:          # >= 4 quota periods per candidate: a burst of a few ms is not throttled, the baseline's seconds are
            torch.nn.functional.conv2d(xs, ws, padding=1)
            k += 1
        dt = (time.time() - t0) / k
        probe[str(n)] = round(dt * 1e3, 2)
        if dt < best_t:
            best, best_t = n, dt
    cores = best
    torch.set_num_threads(cores)
    usd, vsd = cpu_sd
    ucfg, vcfg = P.UNetConfig(), P.VAEConfig()
    plan = ounet.plan_of(usd, ucfg.num_heads)          # the oracle reads the block structure off the checkpoint layout itself (oracle.unet.plan_from_shapes)
    x = P.seeded_randn((2, 9, 64, 64), 1)
    t = torch.full((2,), 981, dtype=torch.long)
    c = P.seeded_randn((2, 1, 768), 2)
    with torch.no_grad():
        ts = []
        for _ in range(2):          # two timed CFG steps (the first also pays the allocator / thread-pool warm-up): the faster one is scaled
            t0 = time.time()
            ounet.unet_forward(usd, plan, x, t, c)
            ts.append(time.time() - t0)
        t_step = min(ts)
        z = P.seeded_randn((1, 4, 64, 64), 3)
        t0 = time.time()
        ovae.decode_first_stage(vsd, vcfg, z)
        t_dec = time.time() - t0
    ips = 1.0 / (50 * t_step + t_dec)
    return {"value": ips, "unit": "images/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(), "cpus_under_cgroup_quota": quota,
            "thread_probe_ms": probe, "thread_probe_note": "ms per 3x3 conv (2 x 320 x 64 x 64 -> 320) by torch thread count, each count sustained for >= 0.4 s; the fastest count is the one used",
            "sample": f"B=1: 2 CFG DDIM steps (UNet batch 2, latent 64x64) = {ts[0]:.2f}s / {ts[1]:.2f}s, the faster scaled x50, + 1 fp32 VAE decode 512x512 = {t_dec:.2f}s"}


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def clock_under_load(sampler, one_batch_args, device):
    """Shader clock inside the DDIM loop relative to the idle chip (tools/clock_probe.hip: a one-wave dependent-FMA chain timed against the
    constant 100 MHz wall_clock64 counter, launched between the steps of one untimed batch).  Returns {idle, mean, min} in FMA iterations per
    tick and `frac` = in-loop mean / idle, or None when the probe library is not built.  The chip is power-managed on this workload: boxes of
    the pool differ by 10 % on identical code, and `roofline.frac` (priced at the nominal 2.4 GHz) moves with them; `frac_at_measured_clock`
    divides that out."""
    import ctypes
    path = os.path.join(ROOT, "tools", "libclockprobe.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    lib.clock_probe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    S = one_batch_args["S"]
    iters = 20000
    probes = torch.zeros((S, 2), dtype=torch.int64, device=device)

    def cb(px0, i):
        lib.clock_probe(probes[i].data_ptr(), iters, torch.cuda.current_stream().cuda_stream)

    # reference clock: the FASTEST of 32 back-to-back probes on the otherwise idle chip (a single wave draws no power: it runs at the boost clock unless
    # the chip has dropped into an idle state, which the first probes of the burst wake it from -- a single probe behind a sleep read 7 % LOW on one box)
    torch.cuda.synchronize()
    ref_probes = torch.zeros((32, 2), dtype=torch.int64, device=device)
    for k in range(32):
        lib.clock_probe(ref_probes[k].data_ptr(), iters, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a = one_batch_args
    sampler.sample(S=S, conditioning=a["c"], batch_size=a["B"], shape=[4, a["h"], a["h"]], verbose=False, unconditional_guidance_scale=a["scale"],
                   unconditional_conditioning=a["uc"], eta=0.0, x_T=a["x_T"], test_model_kwargs={"inpaint_image": a["z_inp"], "inpaint_mask": a["mask"]},
                   img_callback=cb)
    torch.cuda.synchronize()
    ticks = probes[:S, 0].double().cpu()
    rt = ref_probes[:, 0].double().cpu()
    if not ((ticks > 0).all() and (rt > 0).all()):
        return None
    r = iters / ticks
    idle = max(float((iters / rt).max()), float(r.max()))          # the highest clock seen anywhere
    return {"fma_iters_per_10ns_tick_boost": idle, "in_loop_mean": float(r.mean()), "in_loop_min": float(r.min()), "frac": float(r.mean()) / idle,
            "note": "dependent-FMA iterations per 100 MHz tick; in-loop = sampled between the steps of one untimed batch (per-step graph replays: an upper bound of "
                    "the clock the GEMMs see), boost = the fastest of 32 idle probes and of the in-loop samples"}


def conditioning_line(vae, B, h, device, enc_dtype=torch.float32):
    """the once-per-image conditioning stage as a separate line -- CLIP ViT-L/14 on the reference and on the
    (resized) target, ArcFace IR-SE50 on the reference, fp32 KL-VAE encode of the 512x512 masked target -- fp32, batch B."""
    from reface_amd import params as P
    from reface_amd.encoders import Backbone, FrozenCLIPEmbedder, target_to_clip_input
    clip = FrozenCLIPEmbedder(compute_dtype=enc_dtype)
    clip.load_state_dict(P.seeded_state_dict(P.clip_param_specs(clip.cfg), 88), strict=True)
    arc = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se", compute_dtype=enc_dtype)
    arc.load_state_dict(P.seeded_state_dict(P.arcface_param_specs(), 77), strict=True)
    clip.to(device)
    arc.to(device)
    ref = P.seeded_randn((B, 3, 224, 224), 71).to(device)
    tar = torch.tanh(P.seeded_randn((B, 3, 8 * h, 8 * h), 70)).to(device)

    vae.encode_dtype = None if enc_dtype == torch.float32 else enc_dtype

    def stage():
        z_ref = clip.encode(ref)
        z_tar = clip.encode(target_to_clip_input(tar))
        fid = arc.forward_from_clip_image(ref)
        post = vae.encode(tar)
        return z_ref, z_tar, fid, post

    stage()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        out = stage()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    vae.encode_dtype = None
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all() and torch.isfinite(out[3].mean).all()
    tag = "fp32" if enc_dtype == torch.float32 else "bf16"
    return {"metric": f"conditioning images/sec (2x CLIP ViT-L/14 + ArcFace IR-SE50 + VAE encode 512x512, {tag})", "value": B / dt,
            "unit": "images/s", "ms_per_batch": dt * 1e3, "batch": B, "algorithmic_gflop_per_image": 1116.7 + 2 * 155.53 + 12.59}


def lib_digest():
    """Short content hash of the HIP library this process runs (ties a committed PMC pass to a build)."""
    import hashlib
    from reface_amd import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def pmc_traffic(family, workload):
    """(bytes per launch, source file) of a kernel family's HBM-side traffic (read + write), or (None, reason).
    The PMC counters cannot be collected inside this process (rocprofv3 wraps the process): tools/pmc_traffic.sh runs this same
    command under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, FETCH_SIZE doubled as the gfx950 note in
    the microarchitecture guide prescribes) and commits profiles/rNN_pmc_hbm_traffic.json stamped with the library digest and
    the workload.  A pass of a different build or workload is NOT reported: the field is then null."""
    import glob
    import re

    def order(fn):
        # newest LAST, by what the pass itself says -- never by file time (a checkout sets those arbitrarily): the collection time the
        # script stamped into _meta, else the round tag of the file name (r03j < r04a)
        try:
            with open(fn) as f:
                t = json.load(f).get("_meta", {}).get("collected_unix")
        except Exception:
            t = None
        m = re.match(r"r(\d+)([a-z]*)", os.path.basename(fn))
        return (float(t) if t else 0.0, int(m.group(1)) if m else -1, m.group(2) if m else "")
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_hbm_traffic.json")), key=order)
    dig = lib_digest()
    stale = None
    for fn in reversed(files):
        try:
            with open(fn) as f:
                d = json.load(f)
            meta = d.get("_meta", {})
            fam = d.get(family)
            # (a pass collected with `tools/pmc_traffic.sh <tag> c1h|c4c` before round 6's last call stamped the CONFIG KEY where the bench line's id names the BASELINE config)
            wl = re.sub(r"^c1h:", "c1:", re.sub(r"^c4c:", "c4:", meta.get("workload") or ""))
            if wl != workload or fam is None:
                continue
            val = fam["hbm_read_bytes_per_launch"] + fam["hbm_write_bytes_per_launch_uncalibrated"]
            if family.startswith("rf_conv_gemm"):
                # a split-K rf_conv_gemm call is two kernels: the bytes of the reduce passes (their own kernel names in the PMC table) belong to
                # the GEMM launches that issued them -- all of them are charged to this (the dominant) GEMM family
                for k in ("rf_splitk_reduce", "rf_splitk_reduce_frag"):
                    if k in d:
                        val += (d[k]["hbm_read_bytes_per_launch"] + d[k]["hbm_write_bytes_per_launch_uncalibrated"]) * d[k]["launches"] / max(fam["launches"], 1)
            if meta.get("lib_digest") == dig:
                return val, os.path.basename(fn), False
            if stale is None:          # newest pass of the same workload by another build of the library: reported, flagged
                stale = (val, os.path.basename(fn) + f" (library {meta.get('lib_digest')}, running {dig})", True)
        except Exception:
            continue
    if stale is not None:
        return stale
    return None, f"no committed PMC pass for workload {workload}", False


def spawn_ranks(n):
    """`bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD
    process (this process has not touched the GPU; it never replaces itself) and relay rank 0's JSON line."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("[bench] spawning:", " ".join(cmd))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def image_parity(unet, vae, ldm, h, S, scale, device, B=2):
    """SURVEY 8(d) gate for the reduced-precision modes: the SAME full-width weights and seeds through `S` CFG DDIM steps + fp32
    decode in the throughput dtype and in the exact-fp32 parity mode; max / mean |d| and PSNR of the decoded [0, 1] images."""
    from reface_amd import ops
    from reface_amd.ddim import DDIMSampler
    x_T, z_inp, mask, c, uc = synthetic_inputs(B, h, 4242, device)
    ck = (B, h, S, scale)
    imgs = {torch.float32: image_parity.f32_cache[ck]} if ck in image_parity.f32_cache else {}
    fast = unet.compute_dtype
    keep_dec = vae.decode_mode
    for dt in (torch.float32, fast):
        if dt in imgs:
            continue
        unet.set_compute_dtype(dt)
        sampler = DDIMSampler(ldm)
        samples, _ = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False, unconditional_guidance_scale=scale,
                                    unconditional_conditioning=uc, eta=0.0, x_T=x_T, test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
        x = vae.decode(samples, inv_scale=1.0 / 0.18215)
        out = torch.empty_like(x)
        ops.to_image(x, out)()
        torch.cuda.synchronize()
        imgs[dt] = (out.double().cpu(), samples.double().cpu())
        del sampler
    image_parity.f32_cache[ck] = imgs[torch.float32]
    unet.set_compute_dtype(fast)
    vae.decode_mode = keep_dec
    torch.cuda.empty_cache()
    a, b = imgs[torch.float32][0], imgs[fast][0]
    mse = ((a - b) ** 2).mean().item()
    la, lb = imgs[torch.float32][1], imgs[fast][1]
    return {"images": B, "ddim_steps": S, "latent": h, "max_abs": (a - b).abs().max().item(), "mean_abs": (a - b).abs().mean().item(),
            "psnr_db": (10.0 * math.log10(1.0 / mse)) if mse > 0 else float("inf"),
            "latent_rel_l2": ((la - lb).norm() / la.norm()).item(),
            "note": "decoded images in [0,1], full-width weights, same seeds; reference = exact-fp32 MFMA mode of the same kernels "
                    "(that mode is the one pinned to the CPU oracle within 1e-3 by tests/test_fullsize_gpu.py)"}


image_parity.f32_cache = {}


def family_key(fam, dname):
    """The dominant GEMM family of a mode and the MFMA peak of the instruction THAT family issues (a run whose own family is absent
    falls back to the bf16 family and is then priced against the bf16 peak)."""
    key = {"bf16": "rf_conv_gemm[bf16]", "fp16": "rf_conv_gemm[f16]", "f32": "rf_conv_gemm[f32]", "fp8": "rf_conv_gemm[fp8]", "fp8w": "rf_conv_gemm[fp8w]",
           "fp8c": "rf_conv_gemm[fp8]", "f32x3": "rf_conv_gemm[bf16x3]"}[dname]
    peak_of = {"rf_conv_gemm[bf16]": PEAK["bf16"], "rf_conv_gemm[f16]": PEAK["fp16"], "rf_conv_gemm[f32]": PEAK["f32"], "rf_conv_gemm[fp8]": PEAK["fp8"],
               "rf_conv_gemm[fp8w]": PEAK["fp8w"], "rf_conv_gemm[bf16x3]": PEAK["bf16"] / 3.0}
    if key not in fam:
        key = "rf_conv_gemm[bf16]"
    return key, peak_of[key]


def roofline_of(fam, dname, cname, B, h, S, ms_per_step, dec_ms, step_ms, workload, with_traffic=True, raw_ms=None):
    """`frac` = the dominant family's algorithmic FLOP / its event-timed launch time (2.5 us of event cost subtracted per launch, capped: profiler.time_launches)
    / peak; `frac_raw` = the same with NOTHING subtracted from the event intervals (raw_ms: profiler.time_launches.last_raw_ms of the same pass)."""
    key, peak = family_key(fam, dname)
    dom = fam[key]
    unet_alg = F_UNET[h] * 2 * B if h in F_UNET else None
    traffic, tsrc, tstale = pmc_traffic(key, workload) if with_traffic else (None, "not collected for this line", False)
    roof = {"bound": "mfma", "kernel": key, "achieved": dom["tflops_per_s"], "peak": peak, "unit": "TFLOP/s",
            "frac": dom["tflops_per_s"] / peak, "traffic": traffic, "traffic_source": tsrc, "traffic_digest_mismatch": tstale,
            "launches_per_ddim_step": dom["calls"], "avg_launch_us": dom["ms"] / dom["calls"] * 1e3,
            "alg_flop_per_ddim_step": dom["flops"], "ddim_step_ms_sum_of_kernels": step_ms,
            "ddim_step_ms_wall": (ms_per_step - dec_ms) / S}
    if raw_ms and raw_ms.get(key):
        roof["achieved_raw"] = dom["flops"] / (raw_ms[key] * 1e-3) / 1e12
        roof["frac_raw"] = roof["achieved_raw"] / peak
        roof["frac_note"] = "frac: 2.5 us of event-record cost subtracted per launch (capped; an empty event interval measures ~4.7 us); frac_raw: uncorrected event intervals"
    if unet_alg:
        # whole-step utilisation is priced against the FLOP-weighted peak of the matrix instructions the step's GEMM families issue (bf16 2.5 PF;
        # fp8 5 PF; exact fp32 157 TF): a mode that runs 85 % of its FLOPs on the fp8 pipe and 15 % on the bf16 pipe has 1 / (0.85 / 5 + 0.15 / 2.5) PF
        peak_of = {"rf_conv_gemm[bf16]": PEAK["bf16"], "rf_conv_gemm[f16]": PEAK["fp16"], "rf_conv_gemm[f32]": PEAK["f32"], "rf_conv_gemm[fp8]": PEAK["fp8"], "rf_conv_gemm[fp8w]": PEAK["fp8w"],
                   "rf_conv_gemm[bf16x3]": PEAK["bf16"] / 3.0}
        main_peak = PEAK.get(dname, PEAK["bf16"] / 3.0 if dname == "f32x3" else PEAK["bf16"])
        fl = sum(v["flops"] for v in fam.values())
        t_at_peak = sum(v["flops"] / peak_of.get(k, PEAK["bf16"] / 3.0 if dname == "f32x3" else (PEAK["f32"] if dname == "f32" else PEAK["bf16"])) for k, v in fam.items())
        upeak = fl / t_at_peak if t_at_peak > 0 else main_peak
        roof["unet_peak_flop_weighted"] = upeak
        roof["unet_mfma_util_whole_step"] = unet_alg / (step_ms * 1e-3) / 1e12 / upeak
        roof["unet_mfma_util_wall"] = unet_alg / ((ms_per_step - dec_ms) / S * 1e-3) / 1e12 / upeak
    return roof


def other_config_line(oc, unet, vae, ldm, args, device, timed, steps=3, warmup=1):
    """One more BASELINE config on the models already resident: `steps` timed batches + the event-timed launch list of one DDIM step."""
    from reface_amd import ops, profiler
    from reface_amd.ddim import DDIMSampler
    conf = CONFIGS[oc]
    B, h, dname, S = conf["batch"], conf["latent"], conf["dtype"], args.ddim_steps
    unet.set_compute_dtype({"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "fp8": "fp8", "fp8w": "fp8w", "fp8c": "fp8c"}[dname])
    torch.cuda.empty_cache()
    sampler = DDIMSampler(ldm)
    x_T, z_inp, mask, c, uc = synthetic_inputs(B, h, 42, device)
    img_out = torch.empty((B, 3, 8 * h, 8 * h), dtype=torch.float32, device=device)
    cname = {"c4c": "c4", "c1h": "c1"}.get(oc, oc)          # (the id names the BASELINE config; the dtype field tells the two configs[4] lines apart)

    def one_batch():
        samples, _ = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False, unconditional_guidance_scale=args.scale,
                                    unconditional_conditioning=uc, eta=0.0, x_T=x_T, test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
        x = vae.decode(samples, inv_scale=1.0 / 0.18215)
        ops.to_image(x, img_out)()
        return img_out

    elapsed, out = timed(one_batch, warmup, steps)
    assert torch.isfinite(out).all(), f"{oc}: non-finite output image"
    ms_per_step = elapsed / steps * 1e3
    plan = list(sampler._plans.values())[0]
    timed_l = profiler.time_launches(plan["step"], reps=3)
    raw_ms = dict(profiler.time_launches.last_raw_ms)
    fam = profiler.summarize(timed_l)
    step_ms = sum(ms for _, ms in timed_l)
    dec_ms = sum(ms for _, ms in profiler.time_launches(vae._engine("dec", B, h, h).launches, reps=2))
    px = 8 * h
    workload = f"{cname}:{px}x{px}:S{S}:B{B}:{dname}"
    line = {"config": f"BASELINE configs[{conf['idx']}]", "id": workload, "value": B * steps / elapsed, "unit": "images/s", "ms_per_step": ms_per_step,
            "steps": steps, "warmup": warmup, "dtype": dname, "vae_decode_mode": vae.decode_mode,
            "roofline": roofline_of(fam, dname, oc, B, h, S, ms_per_step, dec_ms, step_ms, workload, raw_ms=raw_ms),
            "unet_step": {k: {"calls": v["calls"], "ms": round(v["ms"], 4), "tflops_per_s": round(v["tflops_per_s"], 2)} for k, v in fam.items() if v["ms"] > 0.05}}
    del sampler
    if (dname.startswith("fp8") or dname == "fp16") and not args.no_parity:
        # image distance of this mode from the exact-fp32 mode (S steps, B = 2, same seeds): quoted beside every fp8 / fp16 rate
        par = image_parity(unet, vae, ldm, h, S, args.scale, device)
        line["psnr_db_vs_f32"] = par["psnr_db"]
        line["max_abs_vs_f32"] = par["max_abs"]
        line["mean_abs_vs_f32"] = par["mean_abs"]
    if dname.startswith("fp8") and not args.no_parity:
        line["psnr_note"] = ("seeded RANDOM-INIT weights (Gaussian): per-32-block scales cannot help there (profiles/r04a_fp8_weight_scale_ablation.json), so the "
                             "fp8 / fp8c gap measured here does not predict a trained checkpoint")
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS), help="BASELINE.json configs[i]: c1 512x512 B=8 bf16 (default), "
                    "c2 = c1 per GPU on N GPUs (default for --gpus > 1), c3 768x768 B=4, c4 fp8 UNet B=16 (fp8c; --dtype fp8 / fp8w: the other fp8 forms)")
    ap.add_argument("--batch", type=int, default=None, help="image pairs per GPU per step (overrides the config)")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--latent", type=int, default=None, help="latent side (64 = 512x512 images; overrides the config)")
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp16", "f32", "f32x3", "fp8", "fp8w", "fp8c"], help="UNet compute mode (overrides the config)")
    ap.add_argument("--scale", type=float, default=3.5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-conditioning", action="store_true", help="skip the separate conditioning-stage (encoders) throughput line")
    ap.add_argument("--no-parity", action="store_true", help="skip the bf16-vs-fp32 image error report and the fp32 parity-mode line")
    ap.add_argument("--share-gpu", action="store_true", help="debug: every rank uses cuda:0 and the gloo backend (exercises the multi-rank path on one GPU)")
    ap.add_argument("--profile-json", default=None, help="write the per-kernel-family table here")
    ap.add_argument("--overlap-decode", action="store_true", help="run the VAE decode of a batch on a second stream beside the next batch's DDIM loop")
    ap.add_argument("--no-other-configs", dest="other_configs", action="store_false",
                    help="skip the short configs[3] (768x768) / configs[4] (fp8) lines the --full c1 run appends under `other_configs`")
    ap.add_argument("--full", action="store_true", help="after the headline line's steps, also measure and check everything else: shader clock, "
                    "roofline and per-kernel tables, parity modes, the other configs, the conditioning stage, the CPU baseline, the per-rank weight checksum "
                    "(each still subject to its --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed (decoded images, DDIM latents) "
                    "as DIR/<name>.npy in float32")
    args = ap.parse_args()
    if args.profile_json and not args.full:
        ap.error("--profile-json needs --full")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))          # nothing above touched the GPU
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    cname = args.config or ("c1" if world == 1 else "c2")
    conf = CONFIGS[cname]
    B = args.batch if args.batch is not None else conf["batch"]
    h = args.latent if args.latent is not None else conf["latent"]
    dname = args.dtype or conf["dtype"]
    S = args.ddim_steps
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(device))

    from reface_amd import ops
    from reface_amd.ddim import DDIMSampler
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "f32x3": "f32x3", "fp8": "fp8", "fp8w": "fp8w", "fp8c": "fp8c"}[dname]
    want_cpu = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    unet, vae, ldm, cpu_sd = build_models(dtype, device, rank, world, want_cpu)
    sampler = DDIMSampler(ldm)
    x_T, z_inp, mask, c, uc = synthetic_inputs(B, h, 42 + rank, device)
    img_out = torch.empty((B, 3, 8 * h, 8 * h), dtype=torch.float32, device=device)

    # --overlap-decode: the decode of batch i runs on a second HIP stream beside the DDIM loop of batch i + 1 (the CLI's serving form: the two
    # launch lists share nothing but the latents, handed over as a copy); the timed region still ends with a device-wide synchronize
    side = torch.cuda.Stream(device=device) if args.overlap_decode else None
    last = {}

    def one_batch():
        samples, _ = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False,
                                    unconditional_guidance_scale=args.scale, unconditional_conditioning=uc, eta=0.0, x_T=x_T,
                                    test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
        last["latents"] = samples
        if side is None:
            x = vae.decode(samples, inv_scale=1.0 / 0.18215)
            ops.to_image(x, img_out)()
            return img_out
        z = samples.clone()
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(side):
            side.wait_event(ev)
            x = vae.decode(z, inv_scale=1.0 / 0.18215)
            ops.to_image(x, img_out)()
            z.record_stream(side)
        return img_out

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, warmup, steps):
        for _ in range(warmup):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            o = fn()
        barrier()
        return time.perf_counter() - t0, o

    elapsed, out = timed(one_batch, args.warmup, args.steps)
    if world > 1:
        import torch.distributed as dist
        from reface_amd.multigpu import max_over_ranks
        elapsed = max_over_ranks(elapsed, "cpu" if args.share_gpu else device)
    assert torch.isfinite(out).all(), "non-finite output image"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"images": out, "latents": last["latents"]})
    wsums = None
    if world > 1 and args.full:
        # every rank must be running rank 0's weights (flat RCCL broadcast at start-up): one fp64 checksum per rank, gathered once
        import torch.distributed as dist
        cs = float(sum(p.detach().double().sum().item() for p in list(unet.parameters())[:64] + list(vae.parameters())[:64]))
        wsums = [None] * world
        dist.all_gather_object(wsums, cs)
    ms_per_step = elapsed / args.steps * 1e3
    value = world * B * args.steps / elapsed

    px = 8 * h
    wdesc = {"bf16": "bf16 UNet", "fp16": "fp16 UNet (the bf16 mode's kernels on fp16 storage and v_mfma_f32_32x32x16_f16, fp32 accumulate)", "f32": "exact-fp32 UNet",
             "f32x3": "fp32-storage UNet on split-bf16 operand pairs (three bf16 MFMA passes per product, GEMMs and attention; fp32 accumulate / softmax / norms)",
             "fp8": "fp8 (e4m3fn) UNet weights + fp8 activations (E8M0 block scales) into the ResBlock convs / proj_in / qkv / GEGLU on the fp8 MFMA, "
                    "bf16 residual stream, fp32 accumulate",
             "fp8w": "fp8 (e4m3fn) UNet weights, bf16 activations, fp32 accumulate",
             "fp8c": "fp8 (e4m3fn) weights + fp8 activations (E8M0 block scales) on the fp8 MFMA for the 3x3 convolutions (85 % of the FLOPs), bf16 projections, "
                     "fp32 accumulate"}[dname]
    workload = f"{cname}:{px}x{px}:S{S}:B{B}:{dname}"
    result = {
        "metric": f"{px}x{px} {S}-step DDIM images/sec", "value": value, "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": dname, "data": "synthetic",
        "config": {"workload": f"BASELINE configs[{conf['idx']}]: {px}x{px}, {S} DDIM steps, CFG scale {args.scale}, batch {B} per GPU"
                               f"{' x ' + str(world) + ' GPUs' if world > 1 else ''}, {wdesc} + fp32 VAE decode ({vae.decode_mode} MFMA operands), seeded random-init REFace weights",
                   "id": workload, "batch_per_gpu": B, "global_batch": B * world, "ddim_steps": S, "latent": h,
                   "parallelism": f"dp{world} (pairs sharded, no collective in the step loop)"},
    }

    # self-describing multi-GPU line: which collective library carried the start-up broadcast / barriers, and on how many ranks
    result["distributed"] = {"ranks": world, "backend": (("gloo (ranks share one GPU: debug form)" if args.share_gpu else "nccl = RCCL over xGMI") if world > 1 else None),
                             "rccl_ranks": (0 if (world == 1 or args.share_gpu) else world),
                             "collectives_in_step_loop": 0, "sharding": "image pairs r::world, seeds 42 + rank"}
    if wsums is not None:
        result["weights_checksum_per_rank"] = wsums
        result["weights_identical_on_all_ranks"] = all(w == wsums[0] for w in wsums)
    clk = None
    if rank == 0 and args.full and not args.no_roofline:
        try:
            clk = clock_under_load(sampler, dict(S=S, B=B, h=h, scale=args.scale, c=c, uc=uc, x_T=x_T, z_inp=z_inp, mask=mask), device)
        except Exception as e:          # a diagnostic: never in the way of the headline number
            clk = {"error": repr(e)}
        result["clock_under_load"] = clk
        if clk and "frac" in clk:
            result["clock_under_load_frac"] = clk["frac"]
            log(f"[bench] shader clock inside the DDIM loop: {clk['frac']:.3f} of the idle chip's (min {clk['in_loop_min'] / clk['fma_iters_per_10ns_tick_boost']:.3f})")
        one_batch()                     # (back to the whole-loop graph before the launch list is event-timed)
    if rank == 0 and args.full and not args.no_roofline:
        from reface_amd import profiler
        plan = list(sampler._plans.values())[0]
        log(f"[bench] UNet launches per DDIM step: {len(plan['step'])} (GroupNorm statistics fused into GEMM epilogues: {plan['eng'].gn_fused} of 61; "
            f"LayerNorm passes folded into neighbouring kernels: {plan['eng'].n_ln_folded} of 32)")
        result["fusion"] = {"launches_per_ddim_step": len(plan["step"]), "groupnorm_statistics_fused": plan["eng"].gn_fused, "layernorm_passes_folded": plan["eng"].n_ln_folded,
                            "convs_on_row_extended_a_tiles": plan["eng"].n_hx, "groupnorm_passes_folded_into_proj_in": plan["eng"].n_gn_folded,
                            "transformer_tails_fused_ffn_proj_out": getattr(plan["eng"], "n_tail_fused", 0),
                            "out_head_fused_gn_silu_conv": int(any(getattr(l.fn, "__name__", "") == "rf_gn_silu_conv3x3_small" for l in plan["step"])),
                            "stem_conv_pixels_on_lanes": getattr(plan["eng"], "n_stem_fused", 0),
                            "convs_split_by_samples": getattr(plan["eng"], "n_sample_split", 0),
                            "proj_out_folded_into_ff_net_2": getattr(plan["eng"], "n_po_folded", 0),
                            "transformer_fronts_fused_proj_in_norm1_qkv": getattr(plan["eng"], "n_front_fused", 0)}
        sk = [ops.gemm_plan2(l) for l in plan["step"] if getattr(l.fn, "__name__", "") == "rf_conv_gemm"]
        result["fusion"]["splitk_launches"] = sum(1 for q in sk if q["splitk"] > 1)
        timed_l = profiler.time_launches(plan["step"], reps=5)
        fam = profiler.summarize(timed_l)
        step_ms = sum(ms for _, ms in timed_l)
        raw_ms = dict(profiler.time_launches.last_raw_ms)
        audit = {"empty_event_interval_ms": profiler.time_launches.last_gap_ms, "event_gap_ms_subtracted_per_launch": profiler.time_launches.last_sub_ms,
                 "launches_at_half_floor": profiler.time_launches.last_floored,
                 "raw_ms_per_family": {k: round(v, 4) for k, v in profiler.time_launches.last_raw_ms.items()}}
        dec = vae._engine("dec", B, h, h)
        dtimed = profiler.time_launches(dec.launches, reps=3)
        dfam = profiler.summarize(dtimed)
        dec_ms = sum(ms for _, ms in dtimed)
        dec_f32 = None
        if vae.decode_mode != "f32":            # the exact-fp32 decode timed beside the split-bf16 one, and the distance between their images
            mode = vae.decode_mode
            zs = torch.randn((B, 4, h, h), device=device, generator=torch.Generator(device=device).manual_seed(5))
            fast_img = vae.decode(zs, inv_scale=1.0 / 0.18215)
            vae.decode_mode = "f32"
            e32 = vae._engine("dec", B, h, h)
            f32_img = vae.decode(zs, inv_scale=1.0 / 0.18215)
            d32 = profiler.time_launches(e32.launches, reps=2)
            dec_f32 = {"ms": sum(ms for _, ms in d32), "max_abs_diff_of_decoded_images": (fast_img - f32_img).abs().max().item(),
                       "families": {k: {"calls": v["calls"], "ms": round(v["ms"], 4), "tflops_per_s": round(v["tflops_per_s"], 2)}
                                    for k, v in profiler.summarize(d32).items() if v["flops"] > 0}}
            vae.decode_mode = mode
            vae._engines = {k: v for k, v in vae._engines.items() if v is not e32}
            del e32, f32_img, fast_img
            torch.cuda.empty_cache()
        roof = roofline_of(fam, dname, cname, B, h, S, ms_per_step, dec_ms, step_ms, workload, raw_ms=raw_ms)
        if clk and "frac" in clk:
            # `frac` stays priced at the nominal 2.4 GHz peak (guide); this is the same figure at the clock the chip actually held in the loop
            roof["frac_at_measured_clock"] = roof["frac"] / clk["frac"]
            if "unet_mfma_util_wall" in roof:
                roof["unet_mfma_util_wall_at_measured_clock"] = roof["unet_mfma_util_wall"] / clk["frac"]
        result["roofline"] = roof
        result["breakdown"] = {
            "ddim_step_ms": step_ms, "vae_decode_ms": dec_ms, "vae_decode_mode": vae.decode_mode, "vae_decode_exact_f32": dec_f32,
            "timing_audit": audit,
            "unet_step": {k: {"calls": v["calls"], "ms": round(v["ms"], 4), "tflops_per_s": round(v["tflops_per_s"], 2)} for k, v in fam.items()},
            "vae_decode": {k: {"calls": v["calls"], "ms": round(v["ms"], 4), "tflops_per_s": round(v["tflops_per_s"], 2)} for k, v in dfam.items()},
        }
        log("[bench] per-family (one DDIM step):")
        for k, v in fam.items():
            log(f"   {k:28s} calls {v['calls']:4d}  {v['ms']:9.3f} ms  {v['tflops_per_s']:8.1f} TFLOP/s")
        log(f"[bench] one DDIM step = {step_ms:.2f} ms (sum of kernels); VAE decode = {dec_ms:.2f} ms")
        for k, v in dfam.items():
            log(f"   dec {k:24s} calls {v['calls']:4d}  {v['ms']:9.3f} ms  {v['tflops_per_s']:8.1f} TFLOP/s")
        if args.profile_json:
            def row(l, ms):
                r = {"name": l.name, "family": profiler.launch_family(l), "ms": ms, "flop": profiler.gemm_flops(l) + profiler.attention_flops(l) + profiler.ffn_flops(l) + profiler.attn_in_flops(l),
                     "bytes": profiler.launch_bytes(l)}
                if l.fn.__name__ == "rf_attention":
                    a = l.args          # (dtype, q, k, v, out, B, heads, d, Nq, Nk, ...)
                    r.update(heads_x_batch=a[5] * a[6], d=a[7], Nq=a[8], Nk=a[9], exps=float(a[5]) * a[6] * a[8] * a[9])
                if l.fn.__name__ == "rf_conv_gemm":
                    d = l.keep[0]
                    pl = ops.gemm_plan2(l)
                    r.update(M=d.M, N=d.N, K=d.K, act=d.act, batch=d.batch, KH=d.KH, residual=bool(d.residual), splitk=pl["splitk"], bm=pl["bm"], bn=pl["bn"],
                             gemm_kernels=pl["gemm_kernels"])
                return r
            with open(args.profile_json, "w") as f:
                json.dump({"families": fam, "vae_families": dfam, "step_launches": [row(l, ms) for l, ms in timed_l],
                           "vae_launches": [row(l, ms) for l, ms in dtimed]}, f, indent=1)
    if rank == 0 and world == 1 and args.full and not args.no_parity and dname not in ("f32", "f32x3"):
        try:
            # (a) the reduced-precision mode's image error against the exact-fp32 mode, full width, full S
            result[f"parity_{dname}_vs_f32"] = image_parity(unet, vae, ldm, h, S, args.scale, device)
            log(f"[bench] {dname} vs fp32 decoded images: {result[f'parity_{dname}_vs_f32']}")
            # (b) the parity mode as a driver-visible throughput line (same workload, one timed batch)
            unet.set_compute_dtype(torch.float32)
            sampler = DDIMSampler(ldm)
            fast_decode = vae.decode_mode
            vae.decode_mode = "f32"                 # the parity mode is exact fp32 end to end: UNet AND decode on v_mfma_f32_32x32x2_f32
            el32, _ = timed(one_batch, 1, 1)
            result["parity_mode"] = {"dtype": "f32", "vae_decode_mode": vae.decode_mode, "value": B / el32, "unit": "images/s", "ms_per_step": el32 * 1e3,
                                     "steps": 1, "warmup": 1,
                                     "note": "exact-fp32 MFMA mode (v_mfma_f32_32x32x2_f32) for the UNet and the VAE decode, the mode the 1e-3 oracle gate is stated for"}
            vae.decode_mode = fast_decode
            log(f"[bench] fp32 parity mode: {B / el32:.3f} images/s")
            # (c) the fast form of the parity mode: fp32 storage / accumulation, split-bf16 GEMM operands (3 bf16 MFMA passes), fp32 attention
            unet.set_compute_dtype("f32x3")
            sampler = DDIMSampler(ldm)
            elx3, _ = timed(one_batch, 1, 1)
            result["parity_mode_f32x3"] = {"dtype": "f32x3", "vae_decode_mode": vae.decode_mode, "value": B / elx3, "unit": "images/s", "ms_per_step": elx3 * 1e3, "steps": 1, "warmup": 1,
                                           "vs_exact_f32": image_parity(unet, vae, ldm, h, S, args.scale, device),
                                           "note": "fp32 storage, split-bf16 operand pairs (hi + lo) in three bf16 MFMA passes, fp32 accumulate / attention; "
                                                   "pinned to the CPU oracle by tests/test_fullsize_gpu.py (1e-3-class bound)"}
            log(f"[bench] f32x3 parity mode: {B / elx3:.3f} images/s, vs exact fp32: {result['parity_mode_f32x3']['vs_exact_f32']}")
            unet.set_compute_dtype(dtype)
            del sampler
            torch.cuda.empty_cache()
        except Exception as e:
            result["parity_mode"] = {"error": repr(e)}
    if rank == 0 and world == 1 and args.full and args.other_configs and cname == "c1" and args.batch is None and args.latent is None and args.dtype is None:
        # BASELINE configs[3] / configs[4] as short driver-visible lines (inside this run's wall clock): same models, same timed region
        # (barrier + synchronize around `steps` whole batches), their own roofline from the same event-timed launch list
        result["other_configs"] = {}
        for oc in ("c1h", "c3", "c4", "c4c"):
            try:
                result["other_configs"][oc] = other_config_line(oc, unet, vae, ldm, args, device, timed)
                r = result["other_configs"][oc]
                log(f"[bench] {oc} [{r['dtype']}]: {r['value']:.3f} images/s, {r['ms_per_step']:.1f} ms per batch, dominant family frac {r['roofline']['frac']:.3f}"
                    + (f", PSNR vs fp32 {r['psnr_db_vs_f32']:.1f} dB" if "psnr_db_vs_f32" in r else ""))
            except Exception as e:
                result["other_configs"][oc] = {"error": repr(e)}
        unet.set_compute_dtype(dtype)
        vae._engines = {k: v for k, v in vae._engines.items() if (k[1], k[2]) == (B, h)}          # drop the other configs' decoders
        torch.cuda.empty_cache()
    if rank == 0 and world == 1 and args.full and not args.no_conditioning:
        try:
            result["conditioning"] = conditioning_line(vae, B, h, device)
            log(f"[bench] conditioning stage: {result['conditioning']['value']:.1f} images/s ({result['conditioning']['ms_per_batch']:.1f} ms per batch of {B})")
            if dname not in ("f32", "fp16"):         # what the CLI's --precision bf16 runs: bf16 towers and VAE encoder (decode stays fp32)
                result["conditioning_bf16"] = conditioning_line(vae, B, h, device, torch.bfloat16)
                log(f"[bench] conditioning stage, bf16: {result['conditioning_bf16']['value']:.1f} images/s")
        except Exception as e:        # the headline number must not depend on this side line
            result["conditioning"] = {"error": repr(e)}
    if want_cpu:
        cores = os.cpu_count() or 1
        try:
            cores = len(os.sched_getaffinity(0))
        except Exception:
            pass
        result["cpu_baseline"] = cpu_baseline(cpu_sd, cores)
    elif rank == 0:
        result["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
