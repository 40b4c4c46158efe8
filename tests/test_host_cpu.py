"""CPU tests of the host logic and the drop-in boundary (no kernel launches):
registry + import-path shim, config loading, checkpoint key layout, schedules vs reference golden,
C-ABI exports vs include/reface_hip.h, fail-loudly behaviour without a GPU, multi-process sharding (gloo)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_and_shim_paths():
    from ldm.util import instantiate_from_config, get_obj_from_str
    import reface_amd.unet, reface_amd.vae, reface_amd.ddpm, reface_amd.ddim, reface_amd.encoders
    assert get_obj_from_str("ldm.modules.diffusionmodules.openaimodel.UNetModel") is reface_amd.unet.UNetModel
    assert get_obj_from_str("ldm.models.autoencoder.AutoencoderKL") is reface_amd.vae.AutoencoderKL
    assert get_obj_from_str("ldm.models.diffusion.ddpm.LatentDiffusion") is reface_amd.ddpm.LatentDiffusion
    assert get_obj_from_str("ldm.models.diffusion.ddim.DDIMSampler") is reface_amd.ddim.DDIMSampler
    assert get_obj_from_str("ldm.modules.encoders.modules.FrozenCLIPEmbedder") is reface_amd.encoders.FrozenCLIPEmbedder
    assert get_obj_from_str("ldm.lr_scheduler.LambdaLinearScheduler")
    assert isinstance(instantiate_from_config({"target": "torch.nn.Identity"}), torch.nn.Identity)
    with pytest.raises(KeyError, match="Expected key `target` to instantiate."):      # ldm/util.py:84
        instantiate_from_config({"params": {}})
    assert instantiate_from_config("__is_first_stage__") is None


def _small_model():
    from reface_amd import config as rcfg
    from ldm.util import instantiate_from_config
    cfg = rcfg.load(os.path.join(ROOT, "tests", "configs", "reface_small.yaml"))
    cfg.model.params.cond_stage_config["params"] = {"vision_config": dict(hidden=128, intermediate=512, layers=2, heads=4)}
    return instantiate_from_config(cfg.model), cfg


def test_latent_diffusion_from_yaml_and_checkpoint_keys():
    """The YAML registry builds the pipeline; a checkpoint in the reference key layout loads with no unexpected key."""
    from reface_amd import params as P
    model, cfg = _small_model()
    assert model.Landmark_cond and model.ID_weight == 10.0 and model.clip_weight == 1.0 and model.Landmarks_weight == 0.05
    assert model.scale_factor == 0.18215 and model.num_timesteps == 1000 and model.first_stage_key == "inpaint"
    have = set(model.state_dict().keys())
    sd = {}
    sd.update(P.seeded_state_dict(P.unet_param_specs(model.model.diffusion_model.cfg), 7, "model.diffusion_model."))
    sd.update(P.seeded_state_dict(P.vae_param_specs(model.first_stage_model.cfg), 55, "first_stage_model."))
    sd.update(P.seeded_state_dict(P.clip_param_specs(model.cond_stage_model.cfg), 88, "cond_stage_model."))
    sd.update(P.seeded_state_dict(P.arcface_param_specs(), 77, "face_ID_model.facenet."))
    sd.update(P.seeded_state_dict(P.cond_head_specs(), 9))
    # keys a real REFace checkpoint also carries and this build ignores (last row)
    sd["cond_stage_model.model.text_projection.weight"] = torch.zeros(4, 4)
    sd["cond_stage_model.mapper.resblocks.0.ln_1.weight"] = torch.zeros(4)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert sorted(unexpected) == ["cond_stage_model.mapper.resblocks.0.ln_1.weight", "cond_stage_model.model.text_projection.weight"]
    sched = {"betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
             "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"}
    assert set(missing) == sched, set(missing) ^ sched          # schedule buffers: present in a real checkpoint, rebuilt by the ctor
    assert (set(sd) - set(unexpected)) | sched == have
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "learnable_vector", "ID_proj_out.weight", "landmark_proj_out.bias",
              "proj_out_source.weight", "proj_out_target.bias", "model.diffusion_model.input_blocks.0.0.weight",
              "first_stage_model.post_quant_conv.weight", "face_ID_model.facenet.body.23.res_layer.5.fc2.weight",
              "cond_stage_model.mapper2.resblocks.4.mlp.c_proj.bias", "cond_stage_model.final_ln2.weight"):
        assert k in have, k


def test_full_size_param_counts():
    from reface_amd import params as P
    n = lambda s: sum(int(np.prod(v)) for v in s.values())
    assert n(P.unet_param_specs(P.UNetConfig())) == 859_535_364           # 859.54 M
    assert n(P.vae_param_specs(P.VAEConfig())) == 83_653_863               # 83.65 M
    ib, mid, ob = P.unet_plan(P.UNetConfig())
    assert len(ib) == 12 and len(ob) == 12
    assert sum(l[0] == "res" for b in ib + [mid] + ob for l in b) == 22 and sum(l[0] == "st" for b in ib + [mid] + ob for l in b) == 16


def test_schedule_matches_reference_golden(golden_dir):
    from reface_amd import schedule as S
    g = np.load(os.path.join(golden_dir, "schedule.npz"))
    b = S.ddpm_buffers(1000, 0.00085, 0.0120)
    assert np.array_equal(b["alphas_cumprod"].numpy(), g["alphas_cumprod"])
    assert np.array_equal(S.make_beta_schedule("linear", 1000, 0.00085, 0.0120), g["betas"])
    for Sn in (5, 50):
        ts = S.make_ddim_timesteps("uniform", Sn, 1000, verbose=False)
        for eta in (0.0, 0.5):
            tag = f"S{Sn}_eta{int(eta*10)}"
            sig, a, ap = S.make_ddim_sampling_parameters(b["alphas_cumprod"], ts, eta, verbose=False)
            assert np.array_equal(ts, g[f"ts_{tag}"]) and np.array_equal(a.numpy(), g[f"alphas_{tag}"])
            assert np.array_equal(ap, g[f"alphas_prev_{tag}"]) and np.array_equal(sig, g[f"sigmas_{tag}"])
            co = S.ddim_step_coefficients(a, ap, sig)
            assert co.shape == (Sn, 5) and co.dtype == torch.float32
            # fp32 torch.sqrt runs in the host CPU's vector math library, which rounds differently by CPU (1 ulp from the stored value on some
            # hosts): bit-exact against the reference's expression evaluated on this host, <= 1 ulp from the value the reference stored
            assert np.array_equal(co[:, 1].numpy(), torch.sqrt(1.0 - torch.from_numpy(g[f"alphas_{tag}"])).numpy())
            np.testing.assert_array_max_ulp(co[:, 1].numpy(), g[f"sqrt1m_{tag}"], maxulp=1)
            np.testing.assert_allclose(co[:, 0].numpy(), np.sqrt(g[f"alphas_{tag}"]), rtol=1.2e-7)     # torch vs numpy sqrt: <= 1 ulp
    with pytest.raises(IndexError):          # S=3 -> timestep 1000 out of range: same failure mode as the reference
        ts = S.make_ddim_timesteps("uniform", 3, 1000, verbose=False)
        S.make_ddim_sampling_parameters(b["alphas_cumprod"], ts, 0.0, verbose=False)


def test_cabi_exports_match_header():
    from reface_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    declared = set(re.findall(r"\b(rf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libreface_hip.so not built in this checkout")
    lib = _lib.load()                        # loads the gfx950 library on the CPU box (no compute calls)
    for s in declared:
        assert hasattr(lib, s), s
    assert lib.rf_version() >= 100
    # descriptor layout guard: field order/size of the ctypes mirror vs the C struct
    m = re.search(r"typedef struct rf_conv_gemm_desc \{(.*?)\} rf_conv_gemm_desc;", hdr, re.S)
    cfields = []
    for line in m.group(1).split("\n"):
        line = line.split("/*")[0].strip().rstrip(";")
        if not line:
            continue
        names = line.split(None, 1)[1] if not line.startswith("const") else line.split("*", 1)[1]
        cfields += [n.strip().lstrip("*") for n in names.replace("*", " ").split(",") if n.strip()]
    assert [f[0] for f in _lib.ConvGemmDesc._fields_] == cfields, cfields
    # ... and of rf_ffn_desc (declarations separated by ';', several per line)
    m2 = re.search(r"typedef struct rf_ffn_desc \{(.*?)\} rf_ffn_desc;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m2.group(1), flags=re.S)
    ffields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split("*", 1)[1] if "*" in decl else decl.split(None, 1)[1]
        ffields += [n.strip().lstrip("*") for n in names.split(",") if n.strip()]
    assert [f[0] for f in _lib.FfnDesc._fields_] == ffields, ffields
    sizes = {"x": 8, "ldx": 4, "ln_eps": 4, "gn_part1": 8, "gn_nchunks1": 4}
    for f, t in _lib.FfnDesc._fields_:
        if f in sizes:
            assert ctypes.sizeof(t) == sizes[f], f
    # ... and of rf_stem_desc
    m3 = re.search(r"typedef struct rf_stem_desc \{(.*?)\} rf_stem_desc;", hdr, re.S)
    sfields = []
    for decl in re.sub(r"/\*.*?\*/", "", m3.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split("*", 1)[1] if "*" in decl else decl.rsplit(None, 1)[1] if "," not in decl else decl.split(None, 1)[1]
        sfields += [n.strip().lstrip("*") for n in names.split(",") if n.strip()]
    assert [f[0] for f in _lib.StemDesc._fields_] == sfields, sfields
    ssz = {"x": 8, "C": 4, "dup_off": 8, "gn_part2": 8, "gn_nchunks2": 4}
    for f, t in _lib.StemDesc._fields_:
        if f in ssz:
            assert ctypes.sizeof(t) == ssz[f], f
    # ... and of rf_attn_in_desc
    m4 = re.search(r"typedef struct rf_attn_in_desc \{(.*?)\} rf_attn_in_desc;", hdr, re.S)
    afields = []
    for decl in re.sub(r"/\*.*?\*/", "", m4.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split("*", 1)[1] if "*" in decl else decl.split(None, 1)[1]
        afields += [n.strip().lstrip("*") for n in names.split(",") if n.strip()]
    assert [f[0] for f in _lib.AttnInDesc._fields_] == afields, afields
    asz = {"x": 8, "w_sample_stride": 8, "rows_per_sample": 4, "ln_eps": 4, "dtype": 4}
    for f, t in _lib.AttnInDesc._fields_:
        if f in asz:
            assert ctypes.sizeof(t) == asz[f], f
    ad = _lib.AttnInDesc()
    assert lib.rf_attn_in(ctypes.byref(ad), None) != 0 and b"rf_attn_in" in lib.rf_last_error()
    sd = _lib.StemDesc()
    assert lib.rf_conv3x3_stem(ctypes.byref(sd), None) != 0 and b"rf_conv3x3_stem" in lib.rf_last_error()
    # argument validation happens before any launch, so it is testable without a GPU
    d = _lib.ConvGemmDesc()
    assert lib.rf_conv_gemm(ctypes.byref(d), None) != 0
    assert b"rf_conv_gemm" in lib.rf_last_error()
    assert lib.rf_attention(0, None, None, None, None, 1, 1, 40, 1, 1, 40, 40, 40, 40, 0, 0, 0, 0, 1.0, None) != 0


def test_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from reface_amd import ops, _lib
    from reface_amd.unet import UNetModel
    x = torch.zeros(4, 8)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.linear(x, torch.zeros(8, 8), torch.zeros(4, 8))
    # the round-5 entry points too: the fused transformer tail and the fused `out` head refuse host tensors before anything is launched
    bf = torch.bfloat16
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.ffn_block(torch.zeros(128, 320, dtype=bf), torch.zeros(2560, 320, dtype=bf), torch.zeros(2560), torch.zeros(320, 1280, dtype=bf), torch.zeros(320),
                      torch.zeros(128, 320, dtype=bf), residual=None, wpo=torch.zeros(320, 320, dtype=bf), bpo=torch.zeros(320), res2=None)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.gn_silu_conv3x3_small(torch.zeros(1, 8, 8, 64, dtype=bf), torch.ones(64), torch.zeros(64), torch.zeros(64, dtype=torch.float64), 1,
                                  torch.zeros(4, 576, dtype=bf), torch.zeros(4), torch.zeros(1, 8, 8, 4), eps=1e-5)
    with pytest.raises(_lib.RefaceHipError, match="no CPU fallback"):
        ops.conv3x3_stem(torch.zeros(1, 16, 8, 16, dtype=bf), torch.zeros(64, 144, dtype=bf), torch.zeros(64), torch.zeros(1, 16, 8, 64, dtype=bf))
    m = UNetModel(in_channels=9, model_channels=64, out_channels=4, num_res_blocks=2, attention_resolutions=(4, 2, 1),
                  channel_mult=(1, 2, 4, 4), num_heads=8, use_spatial_transformer=True, context_dim=768, legacy=False)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.zeros(1, 9, 8, 8), torch.zeros(1), context=torch.zeros(1, 1, 768))
    with pytest.raises(NotImplementedError):
        UNetModel(in_channels=9, model_channels=64, out_channels=4, num_res_blocks=2, attention_resolutions=(4,), num_heads=8,
                  use_spatial_transformer=True, context_dim=768, legacy=True)


def test_sampler_kwargs_contract():
    """ddim.py:334: 'kwargs must contain either 'test_model_kwargs' or 'rest' key'."""
    from reface_amd.ddim import DDIMSampler
    import types
    from reface_amd.schedule import ddpm_buffers
    b = ddpm_buffers(1000, 0.00085, 0.0120)
    stub = types.SimpleNamespace(num_timesteps=1000, betas=b["betas"], alphas_cumprod=b["alphas_cumprod"],
                                 alphas_cumprod_prev=b["alphas_cumprod_prev"], device=torch.device("cpu"), model=None)
    s = DDIMSampler(stub)
    with pytest.raises(Exception, match="kwargs must contain either 'test_model_kwargs' or 'rest' key"):
        s.sample(S=5, batch_size=1, shape=[4, 8, 8], conditioning=torch.zeros(1, 1, 768), verbose=False)
    assert list(s.ddim_timesteps) == [1, 201, 401, 601, 801]


def test_cli_flags_match_reference_surface():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import importlib
    cli = importlib.import_module("inference_test_bench")
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings}
    ref = {"--prompt", "--device_ID", "--outdir", "--skip_grid", "--skip_save", "--ddim_steps", "--plms", "--laion400m", "--fixed_code",
           "--Guidance", "--Start_from_target", "--target_start_noise_t", "--ddim_eta", "--n_iter", "--H", "--W", "--C", "--f", "--n_samples",
           "--n_rows", "--scale", "--dataset", "--dataset_dir", "--from-file", "--config", "--ckpt", "--seed", "--rank", "--precision"}
    assert ref <= flags, ref - flags
    d = cli.build_parser().parse_args([])
    assert (d.ddim_steps, d.H, d.W, d.C, d.f, d.ddim_eta, d.seed, d.precision) == (50, 512, 512, 4, 8, 0.0, 42, "full")


def test_fp16_mode_surface():
    """The fp16 throughput mode end to end on the host side (no GPU): the C-ABI dtype code, the ctypes descriptors' `dtype` fields, the library's argument
    checks (fp16 operands write fp16 or fp32, never mix with bf16), the UNet's compute-dtype switch and the CLI's --precision choice."""
    import ctypes
    from reface_amd import _lib, ops
    from reface_amd.unet import UNetModel
    hdr = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert re.search(r"RF_F16\s*=\s*4", hdr) and _lib.RF_F16 == 4 and ops.code(torch.float16) == 4
    assert "dtype" in [f for f, _ in _lib.FfnDesc._fields_] and [f for f, _ in _lib.StemDesc._fields_][-1] == "dtype"
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 101
        d = _lib.ConvGemmDesc()
        d.dtype, d.out_dtype, d.M, d.N, d.K = _lib.RF_F16, _lib.RF_BF16, 128, 128, 64
        assert lib.rf_conv_gemm(ctypes.byref(d), None) != 0 and b"fp16 operands write fp16 or fp32" in lib.rf_last_error()
        d.dtype, d.out_dtype = _lib.RF_BF16, _lib.RF_F16
        assert lib.rf_conv_gemm(ctypes.byref(d), None) != 0 and b"fp16 output needs fp16 operands" in lib.rf_last_error()
        fd = _lib.FfnDesc()
        fd.dtype = 7
        assert lib.rf_ffn_block(ctypes.byref(fd), None) != 0
        assert lib.rf_gn_silu_conv3x3_small(0, None, 1, 8, 8, 64, 64, 1, None, None, None, 1e-5, 1, None, None, 4, 0, None, 4, None, 0, None) != 0
    m = UNetModel(in_channels=9, model_channels=64, out_channels=4, num_res_blocks=2, attention_resolutions=(4, 2, 1), channel_mult=(1, 2, 4, 4), num_heads=8,
                  use_spatial_transformer=True, context_dim=768, legacy=False)
    m.set_compute_dtype(torch.float16)
    assert m.compute_dtype == torch.float16
    with pytest.raises(ValueError):
        m.set_compute_dtype(torch.float64)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import importlib
    for mod in ("inference_test_bench", "inference_swap_selected", "inference_swap_video"):
        cli = importlib.import_module(mod)
        assert cli.build_parser().parse_args(["--precision", "fp16"]).precision == "fp16"


def test_synthetic_dataset_contract_and_sharding():
    from reface_amd.data import SyntheticPairs, shard_indices
    ds = SyntheticPairs(n=5, image_size=64, seed=3)
    t, prior, kw, sid = ds[2]
    assert t.shape == (3, 64, 64) and kw["inpaint_mask"].shape == (1, 64, 64) and kw["ref_imgs"].shape == (1, 3, 224, 224)
    assert torch.equal(kw["inpaint_image"], t * kw["inpaint_mask"]) and set(kw["inpaint_mask"].unique().tolist()) <= {0.0, 1.0}
    assert sid == "000000000002" and torch.equal(ds[2][0], t)
    parts = [shard_indices(11, r, 4) for r in range(4)]
    assert sorted(sum(parts, [])) == list(range(11)) and all(len(p) in (2, 3) for p in parts)
    assert shard_indices(0, 0, 2) == [] and shard_indices(1, 1, 2) == []


_WORKER = r"""
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, %r)
from reface_amd.data import SyntheticPairs
from reface_amd.multigpu import broadcast_module, broadcast_tensors, max_over_ranks, shard_indices
from reface_amd import params as P
from reface_amd.vae import AutoencoderKL
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
# (1) weights: rank 0 holds them, the OTHER ranks start from zeros; bench.py / the CLI call exactly this function
vae = AutoencoderKL(ddconfig=dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4],
                                  num_res_blocks=2, attn_resolutions=[], dropout=0.0), lossconfig={}, embed_dim=4)
ref = P.seeded_state_dict(P.vae_param_specs(vae.cfg), 55)
if rank == 0:
    vae.load_state_dict(ref, strict=True)
ncall = broadcast_module(vae, 0)
got = vae.state_dict()
assert all(torch.equal(got[k], ref[k]) for k in ref), "broadcast mismatch"
assert ncall <= 2, ncall                      # flat buffers, not one collective per tensor (there are > 100 tensors)
# mixed dtypes / small chunks exercise the packing
ts = [torch.full((5,), float(rank)), torch.full((3, 2), rank, dtype=torch.int64), torch.full((7,), float(rank) + 1)]
n2 = broadcast_tensors(ts, 0, chunk_bytes=32)
assert all(float(t.double().sum()) == s for t, s in zip(ts, (0.0, 0.0, 7.0))) and n2 == 3
# (2) pairs shard r::world with no data-path collective
ds = SyntheticPairs(n=7, image_size=32, seed=42)
mine = shard_indices(len(ds), rank, world)
# (3) timing: barrier, max over ranks
dist.barrier(); t0 = time.perf_counter(); time.sleep(0.05 * (rank + 1)); dist.barrier()
el = max_over_ranks(time.perf_counter() - t0)
cnt = torch.tensor([len(mine)]); dist.all_reduce(cnt)
assert int(cnt) == 7 and el >= 0.05 * world - 1e-3
if rank == 0: print("GLOO_OK", int(cnt), len(mine))
dist.destroy_process_group()
"""


def test_multiprocess_sharding_gloo(tmp_path):
    """world_size-2 gloo run of the functions bench.py and the CLI use for the N > 1 path (reface_amd/multigpu.py)."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "GLOO_OK 7 4" in r.stdout


def test_bench_spawns_its_own_ranks(monkeypatch):
    """`bench.py --gpus N` without a launcher starts torch.distributed.run as a CHILD process (never re-execs itself) with
    the driver's rendezvous conventions and forwards its own flags."""
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    # configs: the metric label follows the workload
    assert bench.CONFIGS["c3"]["latent"] == 96 and bench.CONFIGS["c3"]["batch"] == 4 and bench.CONFIGS["c4"]["dtype"] in ("fp8", "fp8c")


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: one float32 <name>.npy per output, whole while they fit the byte cap; beyond it the same seeded
    sample of each output's elements from run to run, within the cap.  --profile-json is a --full table: refused without --full."""
    import bench
    from reface_amd import params as P
    outs = {"images": torch.linspace(0, 1, 2 * 3 * 8 * 8, dtype=torch.float64).reshape(2, 3, 8, 8), "latents": P.seeded_randn((2, 4, 2, 2), 5).bfloat16()}
    bench.dump_outputs(str(tmp_path / "whole"), outs)
    for k, t in outs.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy()), k
    monkeypatch.setattr(bench, "DUMP_BYTES", 200)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
        runs.append({k: np.load(tmp_path / d / f"{k}.npy") for k in outs})
    assert sum(4 * a.size for a in runs[0].values()) <= 200
    for k, t in outs.items():
        a = runs[0][k]
        assert a.dtype == np.float32 and 0 < a.size < t.numel() and np.array_equal(a, runs[1][k])
        assert np.isin(a, t.float().numpy().reshape(-1)).all()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "1", "--profile-json", str(tmp_path / "p.json")])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


def test_output_tree_composition():
    """reface_amd/output.py: the reference's file set (inference_test_bench.py:500-553) -- 4-panel make_grid with 2-pixel padding,
    mask as 255*(m+1)/2 (0 -> 127), truncating float -> uint8 conversion, un-clamped CLIP-un-normalised reference panel."""
    from reface_amd import output as O
    rng = np.random.default_rng(0)
    H = 16
    res = rng.random((3, H, H), dtype=np.float32)
    tgt = np.tanh(rng.standard_normal((3, H, H))).astype(np.float32)
    msk = (rng.random((1, H, H)) > 0.5).astype(np.float32)
    ref = rng.standard_normal((3, H, H)).astype(np.float32)
    o = O.compose(res, tgt, tgt * msk, msk, ref)
    assert set(o) == {"result", "mask", "GT", "inpaint", "ref", "grid"}
    assert o["grid"].shape == (H + 4, 4 * (H + 2) + 2, 3) and o["grid"].dtype == np.uint8
    assert set(np.unique(o["mask"])) <= {127, 255} and o["mask"].shape == (H, H, 3)
    assert np.array_equal(o["result"], (255.0 * res.transpose(1, 2, 0)).astype(np.uint8))
    for k, name in enumerate(("GT", "inpaint", "ref", "result")):          # panels in the reference's order, padding 2, pad value 0
        x0 = 2 + k * (H + 2)
        assert np.array_equal(o["grid"][2:2 + H, x0:x0 + H], o[name]), name
    assert (o["grid"][:2] == 0).all() and (o["grid"][:, :2] == 0).all() and (o["grid"][:, x0 + H:] == 0).all()
    assert np.array_equal(o["GT"], (255.0 * ((tgt + 1.0) / 2.0).transpose(1, 2, 0)).astype(np.uint8))


def test_output_writer_packed_records(tmp_path):
    """The packed uint8 record of rf_compose_outputs_u8 (reface_amd/output.record_layout: 5 panels + grid) through OutputWriter.submit_u8 gives
    the same PNG files as the host composition path (submit): same file set, identical decoded pixels; the writer's worker count is
    bounded by the process's share of the host."""
    from PIL import Image
    from reface_amd import output as O
    rng = np.random.default_rng(1)
    H, B = 16, 3
    res = rng.random((B, 3, H, H), dtype=np.float32)
    tgt = np.tanh(rng.standard_normal((B, 3, H, H))).astype(np.float32)
    msk = (rng.random((B, 1, H, H)) > 0.5).astype(np.float32)
    ref = rng.standard_normal((B, 3, H, H)).astype(np.float32) * 2          # out of [0, 1] after un-normalisation: the uint8 cast wraps
    nbytes, lay = O.record_layout(H, H)
    assert nbytes == 5 * H * H * 3 + (H + 4) * (4 * H + 10) * 3 and lay["grid"][1] == (H + 4, 4 * H + 10, 3)
    recs = np.zeros((B, nbytes), dtype=np.uint8)
    for i in range(B):
        o = O.compose(res[i], tgt[i], tgt[i] * msk[i], msk[i], ref[i])
        for k, (off, shp) in lay.items():
            recs[i, off:off + int(np.prod(shp))] = o[k].reshape(-1)
    ids = [f"{i:012d}" for i in range(B)]
    outs = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        for sub in ("samples", "results", "grid"):
            (d / sub).mkdir(parents=True)
        w = O.OutputWriter(str(d), threads=O.default_writer_threads(8), compress_level=1 if tag == "b" else None)
        if tag == "a":
            w.submit(ids, res, tgt, tgt * msk, msk, ref)
        else:
            w.submit_u8(ids, recs, H, H)
        assert w.close() == B
        outs.append(d)
    files = sorted(str(p.relative_to(outs[0])) for p in outs[0].rglob("*.png"))
    assert len(files) == 6 * B and files == sorted(str(p.relative_to(outs[1])) for p in outs[1].rglob("*.png"))
    for f in files:
        assert np.array_equal(np.asarray(Image.open(outs[0] / f)), np.asarray(Image.open(outs[1] / f))), f
    assert 2 <= O.default_writer_threads(8) <= 8 and 2 <= O.default_writer_threads(1) <= 8
    # --fast_aux_png (aux_compress_level): results/<id>.png keeps the reference's bytes (PIL's default level), the samples/ and grid/ files change level
    # only -- same pixels, other bytes
    d = tmp_path / "c"
    for sub in ("samples", "results", "grid"):
        (d / sub).mkdir(parents=True)
    w = O.OutputWriter(str(d), threads=2, aux_compress_level=1)
    w.submit_u8(ids, recs, H, H)
    assert w.close() == B
    for f in files:
        assert np.array_equal(np.asarray(Image.open(outs[0] / f)), np.asarray(Image.open(d / f))), f
        same = (outs[0] / f).read_bytes() == (d / f).read_bytes()
        assert same if f.startswith("results") else True, f
    assert any((outs[0] / f).read_bytes() != (d / f).read_bytes() for f in files if not f.startswith("results"))


def test_checkpoint_missing_engine_tensor_is_an_error():
    """A pruned checkpoint must not leave engine tensors at their zero initialisation: strict=False loading
    reports it through LatentDiffusion.check_engine_weights; keys the inference path never reads may be absent."""
    model, _ = _small_model()
    model.check_engine_weights(["betas", "cond_stage_model.model.text_projection.weight", "model_ema.decay"])     # fine
    with pytest.raises(RuntimeError, match="would stay zero"):
        model.check_engine_weights(["model.diffusion_model.out.2.weight"])
    with pytest.raises(RuntimeError, match="would stay zero"):
        model.check_engine_weights(["face_ID_model.facenet.input_layer.0.weight"])


def test_celeba_reader_contract(tmp_path):
    """CelebAdataset on a synthetic CelebAMask-HQ tree: tensor contract of test_bench_dataset.py:262-370 (shapes, ranges,
    mask semantics: target mask 1 = keep outside the removed labels, source face x its preserved-label mask, CLIP normalisation)."""
    from PIL import Image
    from reface_amd.data import CLIP_MEAN, CLIP_STD, CelebAdataset
    root = tmp_path / "CelebAMask-HQ"
    (root / "CelebA-HQ-img").mkdir(parents=True)
    (root / "CelebA-HQ-mask" / "Overall_mask").mkdir(parents=True)
    rng = np.random.default_rng(0)
    for i in (28000, 28001, 29000, 29001):
        Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(root / "CelebA-HQ-img" / f"{i}.jpg")
        lab = np.zeros((512, 512), np.uint8)
        lab[128:384, 160:352] = 1                 # skin
        lab[200:260, 230:280] = 2                 # nose
        lab[0:100, :] = 13                        # hair: kept in the source, not removed from the target
        Image.fromarray(lab).save(root / "CelebA-HQ-mask" / "Overall_mask" / f"{i}.png")
    ds = CelebAdataset(state="test", dataset_dir=str(root), gray_outer_mask=True, n_targets=2,
                       remove_mask_tar=[1, 2, 4, 5, 8, 9, 6, 7, 10, 11, 12, 17], preserve_mask_src=[1, 2, 4, 5, 8, 9, 6, 7, 10, 11, 12, 13, 17])
    assert len(ds) == 2
    tar, prior, kw, sid = ds[1]
    assert sid == "000000000001" and tar.shape == (3, 512, 512) and prior.shape == (3, 512, 512)
    assert -1.0 <= float(tar.min()) and float(tar.max()) <= 1.0
    m = kw["inpaint_mask"]
    assert m.shape == (1, 512, 512) and set(np.unique(m.numpy()).tolist()) == {0.0, 1.0}
    assert m[0, 256, 256] == 0 and m[0, 50, 50] == 1 and m[0, 450, 50] == 1          # face removed, hair / background kept
    assert torch.equal(kw["inpaint_image"], tar * m)
    ref = kw["ref_imgs"]
    assert ref.shape == (1, 3, 224, 224)
    zero = torch.tensor([(0 - mu) / sd for mu, sd in zip(CLIP_MEAN, CLIP_STD)]).view(3, 1, 1)
    assert torch.all(ref[0][:, 200:, :20] == 0)                                     # outside the preserved labels: multiplied by 0
    assert (ref[0][:, 100:150, 90:130] != 0).any() and float(ref.abs().max()) < 3.0
    black = CelebAdataset(state="test", dataset_dir=str(root), gray_outer_mask=False, n_targets=2, preserve_mask_src=[1, 2])
    _, _, kb, _ = black[0]
    assert (kb["ref_imgs"][0][:, 200:, :20] != 0).any()                             # full source image in the black-mask variant
    with pytest.raises(NotImplementedError):
        CelebAdataset(state="train", dataset_dir=str(root))


def test_ffhq_reader_layout(tmp_path):
    """FFHQdataset: images512/%05d.png + BiSeNet_mask/%05d.png, ids 68000.. / 69000.., *_FFHQ label lists; contract as CelebA."""
    from PIL import Image
    from reface_amd.data import FFHQdataset
    root = tmp_path / "FFHQ"
    (root / "images512").mkdir(parents=True)
    (root / "BiSeNet_mask").mkdir(parents=True)
    rng = np.random.default_rng(1)
    for i in (68000, 69000):
        Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)).save(root / "images512" / f"{i:05d}.png")
        lab = np.zeros((512, 512), np.uint8)
        lab[100:400, 100:400] = 1
        Image.fromarray(lab).save(root / "BiSeNet_mask" / f"{i:05d}.png")
    ds = FFHQdataset(state="test", dataset_dir=str(root), gray_outer_mask=True, n_targets=1, remove_mask_tar_FFHQ=[1], preserve_mask_src_FFHQ=[1])
    tar, _, kw, sid = ds[0]
    assert len(ds) == 1 and sid == "000000000000" and tar.shape == (3, 512, 512)
    assert kw["inpaint_mask"][0, 250, 250] == 0 and kw["inpaint_mask"][0, 10, 10] == 1 and kw["ref_imgs"].shape == (1, 3, 224, 224)


def test_ffpp_reader_layout(tmp_path):
    """FFdataset: Val_target / target_mask (0..) targets, Val / src_mask (500..) sources."""
    from PIL import Image
    from reface_amd.data import FFdataset
    root = tmp_path / "FF"
    for dname in ("Val_target", "target_mask", "Val", "src_mask"):
        (root / dname).mkdir(parents=True)
    rng = np.random.default_rng(2)
    lab = np.zeros((512, 512), np.uint8)
    lab[100:400, 100:400] = 1
    Image.fromarray(rng.integers(0, 256, (512, 512, 3), dtype=np.uint8)).save(root / "Val_target" / "0000.png")
    Image.fromarray(lab).save(root / "target_mask" / "0000.png")
    Image.fromarray(rng.integers(0, 256, (300, 300, 3), dtype=np.uint8)).save(root / "Val" / "0500.png")
    Image.fromarray(lab).save(root / "src_mask" / "0500.png")
    ds = FFdataset(state="test", dataset_dir=str(root), gray_outer_mask=True, n_targets=1, remove_mask_tar_FFHQ=[1], preserve_mask_src_FFHQ=[1])
    tar, _, kw, sid = ds[0]
    assert len(ds) == 1 and sid == "000000000000" and tar.shape == (3, 512, 512) and kw["ref_imgs"].shape == (1, 3, 224, 224)
    assert kw["inpaint_mask"][0, 250, 250] == 0 and kw["inpaint_mask"][0, 10, 10] == 1


def test_detect_landmarks_host_half():
    """LatentDiffusion.detect_landmarks: the dlib half of get_landmarks (ddpm.py:1068-1096) with a stand-in detector / predictor --
    68 (x, y) points flattened per image, zeros where no face is found, no GPU involved."""
    import types
    from reface_amd.ddpm import LatentDiffusion

    class Pt:
        def __init__(self, x, y):
            self.x, self.y = x, y

    calls = []

    def detector(img, upsample):
        calls.append((img.shape, img.dtype, upsample))
        return [object()] if img.mean() > 100 else []

    def predictor(img, face):
        return types.SimpleNamespace(parts=lambda: [Pt(i, 2 * i) for i in range(68)])

    host = types.SimpleNamespace(detector=detector, predictor=predictor)
    x = torch.stack([torch.full((3, 32, 32), 0.9), torch.full((3, 32, 32), -0.9)])
    lm = LatentDiffusion.detect_landmarks(host, x)
    assert lm.shape == (2, 136) and lm.dtype == torch.float32
    assert lm[0, :4].tolist() == [0.0, 0.0, 1.0, 2.0] and lm[0, -2:].tolist() == [67.0, 134.0] and float(lm[1].abs().sum()) == 0.0
    assert calls[0] == ((32, 32, 3), np.uint8, 1)
    host.detector = None
    assert float(LatentDiffusion.detect_landmarks(host, x).abs().sum()) == 0.0


def _prepared_swap_tree(root, n_tar=3, n_src=2, size=96):
    """<Base_dir>/{target_cropped,mask_frames,source_cropped,source_mask}/<i>.png as stage 1 of the reference writes it."""
    from PIL import Image
    rng = np.random.default_rng(1)
    for d, n in (("target_cropped", n_tar), ("mask_frames", n_tar), ("source_cropped", n_src), ("source_mask", n_src)):
        os.makedirs(os.path.join(root, d), exist_ok=True)
        for i in range(n):
            if "mask" in d:                                                        # label maps are 512x512 (the parser's output size)
                L = 512
                lab = np.zeros((L, L), np.uint8)
                lab[L // 4:3 * L // 4, L // 4:3 * L // 4] = 1                      # skin
                lab[L // 2 - 20:L // 2 + 20, L // 2 - 20:L // 2 + 20] = 2          # nose
                lab[:40, :] = 13                                                   # hair (not in the FFHQ lists)
                Image.fromarray(lab).save(os.path.join(root, d, f"{i}.png"))
            else:
                Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(root, d, f"{i}.png"))


def test_video_dataset_and_source_reference(tmp_path):
    """VideoDataset / source-face loader of the selected-swap callers (video_swap_dataset.py:86-295, inference_swap_selected.py:525-553)."""
    from reface_amd.data import CLIP_MEAN, CLIP_STD, VideoDataset, load_source_reference
    import ldm.data.video_swap_dataset as shim
    assert shim.VideoDataset is VideoDataset
    root = str(tmp_path / "base")
    _prepared_swap_tree(root)
    args = dict(gray_outer_mask=True, remove_mask_tar_FFHQ=[1, 2, 3, 5, 6, 7, 9], preserve_mask_src_FFHQ=[1, 2, 3, 5, 6, 7, 9])
    ds = VideoDataset(data_path=os.path.join(root, "target_cropped"), mask_path=os.path.join(root, "mask_frames"), **args)
    assert len(ds) == 3
    t, prior, kw, sid = ds[1]
    assert t.shape == (3, 512, 512) and -1.0 <= t.min() and t.max() <= 1.0 and torch.equal(prior, t) and sid == "000000000001"
    m = kw["inpaint_mask"]
    assert m.shape == (1, 512, 512) and set(m.unique().tolist()) <= {0.0, 1.0} and set(kw) == {"inpaint_image", "inpaint_mask"}
    assert m[0, 0, 0] == 1.0 and m[0, 256, 256] == 0.0                      # hair kept, face region cut out
    assert torch.equal(kw["inpaint_image"], t * m)
    blk = VideoDataset(data_path=os.path.join(root, "target_cropped"), mask_path=os.path.join(root, "mask_frames"), **dict(args, gray_outer_mask=False))
    assert blk[0][2]["inpaint_mask"][0, 200, 200] == 1.0 and blk[0][2]["inpaint_mask"][0, 256, 256] == 0.0     # only labels 2,3,5,6,7
    ref = load_source_reference(os.path.join(root, "source_cropped", "0.png"), os.path.join(root, "source_mask", "0.png"), args["preserve_mask_src_FFHQ"])
    assert ref.shape == (1, 3, 224, 224)
    assert (ref[0, :, 0, 0] == 0).all() and ref[0, :, 112, 112].abs().sum() > 0                # masked outside the preserved labels
    lo = [(0.0 - mu) / sd for mu, sd in zip(CLIP_MEAN, CLIP_STD)]
    assert ref[0, 0].min() >= lo[0] - 1e-5


def test_swap_selected_cli_surface(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import importlib
    cli = importlib.import_module("inference_swap_selected")
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings}
    ref = {"--prompt", "--outdir", "--Base_dir", "--skip_grid", "--skip_save", "--ddim_steps", "--plms", "--laion400m", "--fixed_code",
           "--Start_from_target", "--only_target_crop", "--target_start_noise_t", "--ddim_eta", "--n_iter", "--H", "--W", "--C", "--f",
           "--n_samples", "--n_rows", "--scale", "--target_folder", "--src_folder", "--src_image_mask", "--from-file", "--config", "--ckpt",
           "--seed", "--rank", "--precision", "--faceParser_name", "--faceParsing_ckpt", "--segnext_config", "--save_vis", "--seg12"}
    assert ref <= flags, ref - flags
    d = cli.build_parser().parse_args([])
    assert (d.ddim_steps, d.n_samples, d.scale, d.precision, d.Base_dir) == (50, 12, 5, "autocast", "results_video")


def test_swap_video_cli_surface(tmp_path):
    """the video caller keeps the reference's flag surface and the on-disk names its stage 1 writes (inference_swap_video.py)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import importlib
    cli = importlib.import_module("inference_swap_video")
    flags = {a.option_strings[0] for a in cli.build_parser()._actions if a.option_strings}
    ref = {"--prompt", "--outdir", "--Base_dir", "--skip_grid", "--skip_save", "--ddim_steps", "--plms", "--laion400m", "--fixed_code",
           "--Start_from_target", "--only_target_crop", "--target_start_noise_t", "--ddim_eta", "--n_iter", "--H", "--W", "--C", "--f",
           "--n_samples", "--n_rows", "--scale", "--target_video", "--src_image", "--src_image_mask", "--from-file", "--config", "--ckpt",
           "--seed", "--rank", "--precision", "--faceParser_name", "--faceParsing_ckpt", "--segnext_config", "--save_vis", "--seg12"}
    assert ref <= flags, ref - flags
    d = cli.build_parser().parse_args([])
    assert (d.ddim_steps, d.n_samples, d.scale, d.precision, d.fixed_code, d.target_video) == (50, 10, 5, "autocast", True, "examples/faceswap/Andy2.mp4")
    opt = cli.build_parser().parse_args(["--Base_dir", "B", "--outdir", "O", "--target_video", "x/clip7.mp4", "--src_image", "y/face.jpg"])
    assert cli.prepared_paths(opt) == {"frames": os.path.join("B", "clip7cropped_face"), "masks": os.path.join("B", "clip7mask_frames"),
                                       "src": os.path.join("O", "temp_results", "face.png"), "src_mask": os.path.join("O", "temp_results", "face.jpg")}


def test_one_inference_surface():
    """scripts/one_inference.py: the reference's function names around the shared stage 2; the web UI is refused with a pointer."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import one_inference as OI
    import inference_swap_selected as SEL
    assert OI.build_parser is SEL.build_parser and callable(OI.run_inference) and callable(OI.process_images)
    with pytest.raises(SystemExit, match="outside this build's scope"):
        OI.main(["--serve"])
    OI._ARGV = None
    with pytest.raises(RuntimeError, match="configure"):
        OI.run_inference()


def test_resize_u8_linear_is_cv2_inter_linear():
    """the source-face resize is cv2.resize(..., INTER_LINEAR) (A.Resize(224, 224), test_bench_dataset.py:141-148, 324).  cv2 is
    absent; `resize_u8_linear` restates OpenCV's uint8 algorithm.  Pinned here by (a) vectors computed by hand from the published
    formulas (half-pixel centres, 11-bit weights, the >> 4 / >> 16 / + 2 >> 2 vertical pass), (b) the properties the algorithm has --
    identity at equal size, constants preserved, replicated borders, the exact 2:1 fast-area average, separability -- (c) <= 1 grey
    level from the float bilinear (no antialias) of torch at arbitrary ratios and from PIL at an integer UPscale, where PIL's kernel has
    the same support, and (d) that it is NOT PIL's antialiased BILINEAR when shrinking."""
    from PIL import Image
    from reface_amd.data import _linear_taps, resize_u8_linear
    # (a) hand vectors: one row [0, 100, 200, 50]
    r = np.array([[0, 100, 200, 50]], dtype=np.uint8)
    assert resize_u8_linear(r, 1, 2).tolist() == [[50, 125]]                  # dx 0: f = 0.5 -> (0 + 100) / 2; dx 1: s = 2 -> (200 + 50) / 2
    assert resize_u8_linear(r, 1, 3).tolist() == [[17, 150, 75]]              # scale 4/3: f = 1/6, 1.5, 2 + 5/6
    assert resize_u8_linear(r, 1, 8).tolist() == [[0, 25, 75, 125, 175, 163, 88, 50]]      # x2 upscale: borders replicate, 1/4 - 3/4 blends
    # fixed-point weights: 5 -> 3 columns, f = 1/3 and 2/3 are not dyadic: 2048 / 3 = 682.67 -> 683, and the pair still sums to 2048
    s_, w0, w1 = _linear_taps(5, 3, True)
    assert s_.tolist() == [0, 2, 3] and w1.tolist() == [683, 0, 1365] and (w0 + w1 == 2048).all()
    c = np.array([[10, 20, 40, 80, 160]], dtype=np.uint8)
    # out = ((2048 * ((a * w0 + b * w1) >> 4)) >> 16 + 2) >> 2 with the row weights (2048, 0)
    exp = [(((2048 * ((10 * 1365 + 20 * 683) >> 4)) >> 16) + 2) >> 2, 40, (((2048 * ((80 * 683 + 160 * 1365) >> 4)) >> 16) + 2) >> 2]
    assert resize_u8_linear(c, 1, 3).tolist() == [exp] and exp == [13, 40, 133]
    # (b) properties
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(resize_u8_linear(a, 37, 53), a)
    assert (resize_u8_linear(np.full((20, 30, 3), 77, np.uint8), 224, 224) == 77).all()
    big = resize_u8_linear(a, 224, 224)
    assert big.shape == (224, 224, 3) and big.dtype == np.uint8
    assert np.array_equal(big[0, 0], a[0, 0]) and np.array_equal(big[-1, -1], a[-1, -1])        # corners: both taps on the border pixel
    e = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    v = e.astype(np.int32)
    assert np.array_equal(resize_u8_linear(e, 32, 24), ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    assert np.array_equal(resize_u8_linear(a[:, :, 1], 100, 90), resize_u8_linear(a, 100, 90)[:, :, 1])       # channels are independent
    # (c) against float bilinear without antialiasing (any ratio) and against PIL where its support is also two taps (integer upscale)
    for (H, W, oh, ow) in ((1024, 1024, 224, 224), (300, 500, 224, 224), (96, 80, 224, 224), (512, 512, 224, 224)):
        x = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        got = resize_u8_linear(x, oh, ow).astype(np.float32)
        ref = torch.nn.functional.interpolate(torch.from_numpy(x).permute(2, 0, 1)[None].float(), size=(oh, ow), mode="bilinear",
                                              align_corners=False)[0].permute(1, 2, 0).numpy()
        assert np.abs(got - ref).max() < 1.0, (H, W, np.abs(got - ref).max())
    x = rng.integers(0, 256, (56, 56, 3), dtype=np.uint8)
    pil = np.asarray(Image.fromarray(x).resize((224, 224), Image.BILINEAR)).astype(np.int32)
    assert np.abs(resize_u8_linear(x, 224, 224).astype(np.int32) - pil).max() <= 1
    # (d) shrinking: PIL's BILINEAR antialiases (support grows with the ratio), cv2's INTER_LINEAR does not -- different tensors
    x = rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    pil = np.asarray(Image.fromarray(x).resize((224, 224), Image.BILINEAR)).astype(np.int32)
    assert np.abs(resize_u8_linear(x, 224, 224).astype(np.int32) - pil).mean() > 20


def test_e4m3_numpy_reference_is_self_consistent():
    """The numpy e4m3fn reference of the GPU quantiser tests (tests/e4m3_ref.py): every finite code round-trips, midpoints go
    to the even neighbour, +-448 saturates."""
    import numpy as np
    from e4m3_ref import e4m3fn_decode_np, e4m3fn_encode_rne_sat_np
    codes = np.array([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=np.int64)
    vals = e4m3fn_decode_np(codes)
    back = e4m3fn_encode_rne_sat_np(vals)
    assert np.array_equal(back & 0x7f, (codes & 0x7f).astype(np.uint8)) and np.array_equal((back >> 7)[vals != 0], ((codes >> 7).astype(np.uint8))[vals != 0])
    pos = np.sort(vals[vals >= 0])
    mid = (pos[:-1] + pos[1:]) / 2
    enc = e4m3fn_encode_rne_sat_np(mid)
    assert (enc & 1 == 0).all()                               # ties land on the even mantissa
    assert e4m3fn_encode_rne_sat_np(np.array([1e9, -1e9, 448.0, 464.0, 479.9]))[0] == 0x7e and e4m3fn_encode_rne_sat_np(np.array([-1e9]))[0] == 0xfe
    # and it agrees with torch's own float8_e4m3fn cast on 100 k random values over 7 decades (finite range)
    x = (torch.randn(100000, generator=torch.Generator().manual_seed(5)) * torch.logspace(-4, 2.6, 100000)).clamp(-448, 448)
    assert np.array_equal(e4m3fn_encode_rne_sat_np(x.numpy()), x.to(torch.float8_e4m3fn).view(torch.uint8).numpy())


def test_worker_pools_are_sized_by_the_cgroup_quota(tmp_path, monkeypatch):
    """reface_amd/output.available_cpus: the affinity mask capped by the container's CFS quota (the GPU boxes of the test pool: 256 CPUs in the mask, a quota of 16 --
    profiles/r06i_host_half_stages.txt); default_writer_threads is that share / (2 x world), between 2 and 8."""
    import builtins
    import os
    from reface_amd import output as O
    n = O.available_cpus()
    assert 1 <= n <= len(os.sched_getaffinity(0))
    real_open, real_exists = builtins.open, os.path.exists
    f = tmp_path / "cpu.max"

    def fake_open(path, *a, **k):
        return real_open(str(f), *a, **k) if path == "/sys/fs/cgroup/cpu.max" else real_open(path, *a, **k)
    monkeypatch.setattr(os.path, "exists", lambda p: True if p == "/sys/fs/cgroup/cpu.max" else real_exists(p))
    monkeypatch.setattr(builtins, "open", fake_open)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(256)))
    f.write_text("1600000 100000\n")
    assert O.available_cpus() == 16 and O.default_writer_threads(1) == 8 and O.default_writer_threads(8) == 2
    f.write_text("max 100000\n")
    assert O.available_cpus() == 256 and O.default_writer_threads(8) == 8
    f.write_text("50000 100000\n")          # half a CPU: never below one
    assert O.available_cpus() == 1 and O.default_writer_threads(1) == 2
