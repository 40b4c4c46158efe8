#!/usr/bin/env python3
"""How many steps does a sampler need?  DDIM and DPM-Solver++ from the same x_T over a list of step counts (needs a GPU).

  python tools/sampler_steps.py                                   # seeded full-width weights at bench.py's c1 shape (B = 8, 512x512, bf16)
  python tools/sampler_steps.py --config C.yaml --ckpt last.ckpt   # a trained checkpoint, through the CLIs' model loader and batch body
  python tools/sampler_steps.py --S 10 20 50 --rounds 3            # three alternating rounds of every run: the spread of the timings

For every (sampler, S) it prints ms per batch (sampling loop + VAE decode), ms per sampling loop and per step, images/s, and -- against the
SAME family's own run at --S-ref (200) -- the RMS distance of the final latent and the PSNR of the decoded image: self-convergence, i.e. how
far the S-step result is from where that sampler itself converges.  On seeded random weights these figures describe the ODE of a random network,
not image quality; on a trained checkpoint they are how a user finds their S.

Every run is a fresh child process under its own time limit (--limit seconds); the first one that fails or runs out of time ends the tool
(nothing more is started on the GPU after a failure).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--S", type=int, nargs="+", default=[10, 20, 50], help="step counts to compare")
    p.add_argument("--S-ref", dest="S_ref", type=int, default=200, help="each family's own converged run (0: no distances, timings only)")
    p.add_argument("--samplers", nargs="+", default=["ddim", "dpm"], choices=["ddim", "dpm"])
    p.add_argument("--dpm_order", type=int, choices=[1, 2, 3], default=2)
    p.add_argument("--dpm_spacing", choices=["logsnr", "quad", "uniform"], default="logsnr")
    p.add_argument("--ckpt", default=None, help="checkpoint ('none': seeded weights of --config's architecture); default: bench.py's seeded full-width models")
    p.add_argument("--config", default=None, help="model YAML (with --ckpt)")
    p.add_argument("--clip_vision_config", default=None, help="JSON dict overriding the CLIP ViT dims (with --ckpt)")
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--H", type=int, default=512, help="image side (latent side = H / 8)")
    p.add_argument("--precision", choices=["full", "bf16", "fp16"], default="bf16")
    p.add_argument("--scale", type=float, default=3.5)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--reps", type=int, default=3, help="timed batches per run (the median is reported)")
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--rounds", type=int, default=1, help="alternating repetitions of the whole --S list (timing spread)")
    p.add_argument("--limit", type=float, default=300.0, help="time limit of one run (one child process), seconds")
    p.add_argument("--json", default=None, help="also write the table here")
    p.add_argument("--worker", nargs=3, metavar=("SAMPLER", "S", "OUT"), default=None, help=argparse.SUPPRESS)
    return p


# ------------------------------------------------------------------------------------------------ one run (child process)
def worker(opt, which, S, out_path):
    import numpy as np
    import torch
    dtype = {"full": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[opt.precision]
    dev = torch.device("cuda")
    torch.cuda.set_device(0)
    torch.manual_seed(opt.seed)
    h = opt.H // 8

    def make_sampler(ldm):
        if which == "ddim":
            from reface_amd.ddim import DDIMSampler
            return DDIMSampler(ldm)
        from reface_amd.dpm_solver import DPMSolverSampler
        return DPMSolverSampler(ldm, order=opt.dpm_order, spacing=opt.dpm_spacing)

    if opt.ckpt is None:
        import bench
        unet, vae, ldm, _ = bench.build_models(dtype, dev, 0, 1, False)
        x_T, z_inp, mask, c, uc = bench.synthetic_inputs(opt.batch, h, opt.seed, dev)
        sampler = make_sampler(ldm)

        def loop():
            z, _ = sampler.sample(S=S, conditioning=c, batch_size=opt.batch, shape=[4, h, h], verbose=False, unconditional_guidance_scale=opt.scale,
                                  unconditional_conditioning=uc, eta=0.0, x_T=x_T, test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
            return z

        decode = lambda z: vae.decode(z, inv_scale=1.0 / 0.18215)
    else:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import inference_test_bench as cli
        from reface_amd import config as rcfg
        from reface_amd.data import SyntheticPairs
        from reface_amd.pipeline import SwapRunner
        config = rcfg.load(opt.config)
        if opt.clip_vision_config:
            config.model.params.cond_stage_config["params"] = {"vision_config": json.loads(opt.clip_vision_config)}
        model = cli.load_model_from_config(config, opt.ckpt)
        if opt.precision == "bf16":
            model.set_compute_dtype(torch.bfloat16, encoders=True)
        elif opt.precision == "fp16":
            model.set_compute_dtype(torch.float16)
        ropt = argparse.Namespace(ddim_steps=S, scale=opt.scale, ddim_eta=0.0, C=4, H=opt.H, W=opt.H, f=8, dump_tensors=None)
        sampler = make_sampler(model)
        runner = SwapRunner(model, sampler, ropt)
        pairs = SyntheticPairs(n=opt.batch, image_size=opt.H, seed=opt.seed)
        items = [pairs[i] for i in range(opt.batch)]
        target = torch.stack([it[0] for it in items])
        kw = {k: torch.stack([it[2][k] for it in items]).to(dev) for k in items[0][2]}
        x_T = torch.randn([opt.batch, 4, h, h], device=dev)
        state = {}

        def loop():               # the CLIs' batch body: conditioning -> VAE encode -> sampling -> decode (one piece: timed as the batch)
            with model.ema_scope():
                x_img, inter = runner.run_batch(target, kw, kw["ref_imgs"].squeeze(1), start_code=x_T)
            state["img"] = x_img
            return inter["x_inter"][-1]

        decode = lambda z: state["img"]

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = fn()
        t1.record()
        t1.synchronize()
        return r, t0.elapsed_time(t1)

    with torch.no_grad():
        loops, batches = [], []
        for k in range(opt.warmup + opt.reps):
            z, ms_loop = timed(loop)
            img, ms_dec = timed(lambda: decode(z))
            if k >= opt.warmup:
                loops.append(ms_loop)
                batches.append(ms_loop + ms_dec)
    n_steps = len(sampler.dpm_nodes) - 1 if which == "dpm" else len(sampler.ddim_timesteps)          # (DDIM's grid has range(0, T, T // S) steps)
    med = lambda v: float(np.median(v))
    np.savez(out_path, latent=z.float().cpu().numpy(), image=img.float().cpu().numpy(), ms_batch=med(batches), ms_loop=med(loops),
             ms_batch_all=np.asarray(batches), finite=bool(torch.isfinite(z).all() and torch.isfinite(img).all()), n_steps=n_steps)
    print(f"[worker] {which} S={S}: {med(batches):.1f} ms per batch, {med(loops):.1f} ms per sampling loop", flush=True)


# ------------------------------------------------------------------------------------------------ the table (parent process: no GPU work of its own)
def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    opt = build_parser().parse_args(argv)
    if opt.worker:
        return worker(opt, opt.worker[0], int(opt.worker[1]), opt.worker[2])
    if (opt.ckpt is None) != (opt.config is None):
        raise SystemExit("sampler_steps: --ckpt and --config go together")
    import numpy as np
    work = tempfile.mkdtemp(prefix="sampler_steps_")
    passthrough = [a for a in argv]
    runs = [(w, S) for w in opt.samplers for S in ([opt.S_ref] if opt.S_ref else [])]
    for r in range(opt.rounds):                      # alternating: every family at every S, then again
        runs += [(w, S) for S in opt.S for w in opt.samplers if not (S == opt.S_ref and r == 0)]
    results = {}
    for n, (w, S) in enumerate(runs):
        out = os.path.join(work, f"run{n:03d}_{w}_S{S}.npz")
        cmd = [sys.executable, os.path.abspath(__file__)] + passthrough + ["--worker", w, str(S), out]
        t0 = time.time()
        try:
            r = subprocess.run(cmd, timeout=opt.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"sampler_steps: {w} S={S} ran into its time limit of {opt.limit:.0f} s: stopping here, nothing more is started")
        if r.returncode != 0:
            raise SystemExit(f"sampler_steps: {w} S={S} failed (exit status {r.returncode}): stopping here, nothing more is started")
        print(f"[sampler_steps] {w} S={S} done in {time.time() - t0:.0f} s", flush=True)
        results.setdefault((w, S), []).append(dict(np.load(out)))
    rows = []
    name = {"ddim": "DDIM", "dpm": f"DPM-Solver++ {opt.dpm_order} / {opt.dpm_spacing}"}
    print(f"\nbatch {opt.batch}, {opt.H}x{opt.H}, {opt.precision}, CFG {opt.scale}, " + ("seeded full-width weights" if opt.ckpt is None else f"--ckpt {opt.ckpt}")
          + (f"; distances to the same sampler's own S = {opt.S_ref} run" if opt.S_ref else ""))
    print(f"{'sampler':<28}{'S':>5}{'ms/batch':>12}{'(min..max)':>20}{'ms/loop':>10}{'ms/step':>9}{'img/s':>8}{'latent RMS':>12}{'PSNR dB':>9}")
    for w in opt.samplers:
        ref = results.get((w, opt.S_ref), [None])[0] if opt.S_ref else None
        for S in sorted(set(opt.S + ([opt.S_ref] if opt.S_ref else []))):
            rr = results.get((w, S))
            if not rr:
                continue
            ms = [float(x["ms_batch"]) for x in rr]
            ms_b, ms_l, steps = float(np.median(ms)), float(np.median([float(x["ms_loop"]) for x in rr])), int(rr[0]["n_steps"])
            rms = psnr = None
            if ref is not None and S != opt.S_ref:
                rms = float(np.sqrt(np.mean((rr[0]["latent"].astype(np.float64) - ref["latent"]) ** 2)))
                mse = float(np.mean((rr[0]["image"].astype(np.float64) - ref["image"]) ** 2))          # images in [-1, 1] or [0, 1]: peak = their range
                peak = 2.0 if ref["image"].min() < -0.01 else 1.0
                psnr = float(10 * np.log10(peak ** 2 / mse)) if mse > 0 else float("inf")
            assert all(bool(x["finite"]) for x in rr), f"{w} S={S}: non-finite result"
            rows.append(dict(sampler=w, S=S, steps=steps, ms_batch=ms_b, ms_batch_runs=ms, ms_loop=ms_l, ms_step=ms_l / steps, img_s=1e3 * opt.batch / ms_b,
                             latent_rms=rms, psnr_db=psnr))
            print(f"{name[w]:<28}{S:>5}{ms_b:>12.1f}{f'({min(ms):.1f}..{max(ms):.1f})':>20}{ms_l:>10.1f}{ms_l / steps:>9.2f}{1e3 * opt.batch / ms_b:>8.2f}"
                  + (f"{rms:>12.3e}{psnr:>9.2f}" if rms is not None else f"{'-':>12}{'-':>9}"))
    import shutil
    shutil.rmtree(work, ignore_errors=True)
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(dict(batch=opt.batch, H=opt.H, precision=opt.precision, scale=opt.scale, ckpt=opt.ckpt, S_ref=opt.S_ref, dpm_order=opt.dpm_order,
                           dpm_spacing=opt.dpm_spacing, rows=rows), f, indent=1)
    return rows


if __name__ == "__main__":
    main()
