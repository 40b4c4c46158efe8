#!/usr/bin/env python3
"""Generate golden input/output vectors by running the REFERENCE itself (/root/reference).

Build-container only.  Imports the reference's Python modules through tools/ref_shims.py,
loads them with weights from ``reface_amd.params.seeded_state_dict`` (strict key/shape match --
this also pins the checkpoint key layout), runs them on seeded inputs and stores inputs/outputs
as small ``.npz`` fixtures under tests/golden/.  Only DATA is stored (tensors + the seeds/configs
needed to regenerate the weights); no reference source is copied.

Usage:  python tools/gen_golden.py [group ...]     (groups: schedule unet_ops unet_small unet_full
                                                    ddim vae arcface clip e2e bisenet align align_pad idscore pose expr fid lpips)

One group records this project's own library instead of the reference and is run by name only:
        REFACE_HIP_LIB=<libreface_hip.so of the commit to record> python tools/gen_golden.py gemm_plans <commit>
writes tests/golden/gemm_plans.json, the answers of rf_conv_gemm_plan3 over the sweep of tests/gemm_plan_sweep.py.  It exists to pin the planner
ACROSS a change of its code: record at the commit before the change, never from the code the table is meant to check.
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()                      # puts /root/reference at sys.path[0]
sys.path.append(os.path.dirname(HERE))   # repo root AFTER the reference: `ldm` stays the reference's

from reface_amd import params as P  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
os.makedirs(OUT, exist_ok=True)
torch.set_grad_enabled(False)
torch.set_num_threads(int(os.environ.get("GEN_THREADS", "8")))


rnd = P.seeded_randn     # inputs are regenerated from (shape, seed) by the tests; only outputs are stored


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"  wrote {path}  ({os.path.getsize(path)/1024:.1f} KiB)")


def load_strict(module, sd):
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing[:5], unexpected[:5])


# ---------------------------------------------------------------------------------------------
def gen_schedule():
    from ldm.modules.diffusionmodules.util import (make_beta_schedule, make_ddim_timesteps,
                                                   make_ddim_sampling_parameters)
    betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120)
    ac = torch.tensor(np.cumprod(1.0 - betas, axis=0), dtype=torch.float32)   # ddpm.py:262-272
    out = {"betas": betas, "alphas_cumprod": ac}
    for S in (5, 50):
        ts = make_ddim_timesteps("uniform", S, 1000, verbose=False)
        for eta in (0.0, 0.5):
            sig, a, ap = make_ddim_sampling_parameters(ac, ts, eta, verbose=False)
            tag = f"S{S}_eta{int(eta*10)}"
            out[f"ts_{tag}"] = ts
            out[f"sigmas_{tag}"] = np.asarray(sig, dtype=np.float64)
            out[f"alphas_{tag}"] = a
            out[f"alphas_prev_{tag}"] = ap
            out[f"sqrt1m_{tag}"] = np.sqrt(1.0 - a)
    save("schedule", **out)


def _ref_unet(cfg: P.UNetConfig, seed):
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    m = UNetModel(image_size=32, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                  model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions),
                  num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult),
                  num_heads=cfg.num_heads, use_spatial_transformer=True, transformer_depth=1,
                  context_dim=cfg.context_dim, use_checkpoint=True, legacy=False,
                  add_conv_in_front_of_unet=False).eval()
    sd = P.seeded_state_dict(P.unet_param_specs(cfg), seed)
    load_strict(m, sd)
    return m, sd


def gen_unet_ops():
    """Single ResBlock / SpatialTransformer / timestep-embed at full REFace widths."""
    from ldm.modules.diffusionmodules.openaimodel import ResBlock, Downsample, Upsample
    from ldm.modules.attention import SpatialTransformer
    from ldm.modules.diffusionmodules.util import timestep_embedding
    import collections
    res = {}
    t = torch.tensor([981, 1, 500, 21], dtype=torch.long)
    res["temb_t"] = t
    res["temb_out"] = timestep_embedding(t, 320)
    for tag, cin, cout, hw in (("a", 320, 320, 16), ("b", 2560, 1280, 8), ("c", 960, 640, 8)):
        blk = ResBlock(cin, 1280, 0, out_channels=cout, dims=2, use_checkpoint=True).eval()
        s = collections.OrderedDict()
        P._res_specs(s, "r", cin, cout, 1280)
        sd = P.seeded_state_dict(s, 100)
        load_strict(blk, {k[2:]: v for k, v in sd.items()})
        x = rnd((2, cin, hw, hw), 1)
        emb = rnd((2, 1280), 2)
        res[f"res_{tag}_y"] = blk(x, emb)
    for tag, c, heads, hw in (("a", 320, 8, 16), ("b", 1280, 8, 8), ("c", 640, 8, 12)):
        st = SpatialTransformer(c, heads, c // heads, depth=1, context_dim=768).eval()
        s = collections.OrderedDict()
        P._st_specs(s, "s", c, 768)
        sd = P.seeded_state_dict(s, 101)
        load_strict(st, {k[2:]: v for k, v in sd.items()})
        x = rnd((2, c, hw, hw), 3)
        ctx = rnd((2, 1, 768), 4)
        res[f"st_{tag}_y"] = st(x, ctx)
    save("unet_ops", **res)


SMALL_UNET = dict(in_channels=9, model_channels=64, out_channels=4, num_res_blocks=2,
                  attention_resolutions=(4, 2, 1), channel_mult=(1, 2, 4, 4), num_heads=8, context_dim=768)


def gen_unet_small():
    cfg = P.UNetConfig(**SMALL_UNET)
    m, _ = _ref_unet(cfg, 7)
    x = rnd((2, 9, 16, 16), 10)
    t = torch.tensor([981, 41], dtype=torch.long)
    ctx = rnd((2, 1, 768), 11)
    save("unet_small", t=t, y=m(x, t, context=ctx), seed=7)
    x = rnd((2, 9, 24, 24), 12)          # non power-of-two grid (768-px style: 24 -> 12 -> 6 -> 3)
    save("unet_small_24", t=t, y=m(x, t, context=ctx), seed=7)


def gen_unet_full():
    cfg = P.UNetConfig()
    t0 = time.time()
    m, _ = _ref_unet(cfg, 1234)
    print(f"  full UNet built in {time.time()-t0:.1f}s")
    x = rnd((2, 9, 8, 8), 20)
    t = torch.tensor([961, 961], dtype=torch.long)
    ctx = rnd((2, 1, 768), 21)
    y = m(x, t, context=ctx)
    save("unet_full_8", t=t, y=y, seed=1234)
    x = rnd((1, 9, 16, 16), 22)
    t = torch.tensor([21], dtype=torch.long)
    ctx = rnd((1, 1, 768), 23)
    save("unet_full_16", t=t, y=m(x, t, context=ctx), seed=1234)


def gen_unet_keys():
    """{state-dict key: shape} of the REFERENCE's full-width UNetModel (openaimodel.py:666-830, the REFace configuration) and of a small
    configuration with a different channel_mult / attention pattern: what oracle.unet.plan_from_shapes reads the block structure from."""
    import json
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    out = {}
    for tag, cfg in (("full", P.UNetConfig()),
                     ("small", P.UNetConfig(model_channels=32, channel_mult=(1, 2, 4), attention_resolutions=(2, 1), num_res_blocks=1, num_heads=4, context_dim=32))):
        with torch.device("meta"):
            m = UNetModel(image_size=32, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                          attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult),
                          num_heads=cfg.num_heads, use_spatial_transformer=True, transformer_depth=1, context_dim=cfg.context_dim, use_checkpoint=True,
                          legacy=False, add_conv_in_front_of_unet=False)
        out[tag] = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.__dict__.items()},
                    "shapes": {k: list(v.shape) for k, v in m.state_dict().items()}}
    path = os.path.join(OUT, "unet_keys.json")
    json.dump(out, open(path, "w"), separators=(",", ":"), sort_keys=True)
    print(f"  wrote {path}  ({os.path.getsize(path)/1024:.1f} KiB, {len(out['full']['shapes'])} + {len(out['small']['shapes'])} keys)")


class _StubLDM:
    """What DDIMSampler reads from the model (ddim.py:100,113-119,207,345)."""

    def __init__(self, unet):
        from ldm.modules.diffusionmodules.util import make_beta_schedule
        betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.0120)
        ac = np.cumprod(1.0 - betas, axis=0)
        self.num_timesteps = 1000
        self.betas = torch.tensor(betas, dtype=torch.float32)
        self.alphas_cumprod = torch.tensor(ac, dtype=torch.float32)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32)
        self.device = torch.device("cpu")
        self.unet = unet

    def apply_model(self, x, t, c):
        return self.unet(x, t, context=c)


def gen_ddim():
    from ldm.models.diffusion.ddim import DDIMSampler
    DDIMSampler.register_buffer = lambda self, n, a: setattr(self, n, a)
    cfg = P.UNetConfig(**SMALL_UNET)
    m, _ = _ref_unet(cfg, 7)
    sampler = DDIMSampler(_StubLDM(m))
    B, h = 2, 16
    x_T = rnd((B, 4, h, h), 30)
    z_inp = rnd((B, 4, h, h), 31)
    mask = (rnd((B, 1, h, h), 32) > 0).float()
    c = rnd((B, 1, 768), 33)
    uc = rnd((1, 1, 768), 34).repeat(B, 1, 1)
    for S in (5, 50):
        samples, inter = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False,
                                        unconditional_guidance_scale=3.5, unconditional_conditioning=uc,
                                        eta=0.0, x_T=x_T, log_every_t=100,
                                        test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
        save(f"ddim_small_S{S}", samples=samples,
             pred_x0_last=inter["pred_x0"][-1], n_inter=len(inter["x_inter"]), seed=7, scale=3.5)
    # eta > 0 with recorded noise (RNG stream: one randn per step, util.py:264-267)
    torch.manual_seed(99)
    samples, _ = sampler.sample(S=5, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False,
                                unconditional_guidance_scale=3.5, unconditional_conditioning=uc,
                                eta=0.5, x_T=x_T,
                                test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
    torch.manual_seed(99)
    noises = torch.stack([torch.randn((B, 4, h, h)) for _ in range(5)])
    save("ddim_small_S5_eta5", samples=samples, noises=noises, seed=7, scale=3.5)


def gen_ddim_full():
    """SURVEY 8d gate at FULL S and FULL width: the reference's own UNet (859.5 M parameters, seeded weights 1234) under the reference's
    DDIMSampler (ddim.py:96-251, 323-375), S = 50, B = 2 at 64x64 latents, CFG scale 3.5, eta 0, inpainting kwargs -- then the reference's
    full-width AutoencoderKL.decode (seeded weights 55) of the samples / 0.18215 (ddpm.py:1102-1113).  ~20 minutes on 8 CPU threads.
    Stored: the latents after 50 steps, the last pred_x0 and every 8th pixel of the decoded images (the full images would be 6 MB:
    the test decodes the stored latents with the oracle and checks that decode against these pixels)."""
    from ldm.models.diffusion.ddim import DDIMSampler
    DDIMSampler.register_buffer = lambda self, n, a: setattr(self, n, a)
    m, _ = _ref_unet(P.UNetConfig(), 1234)
    sampler = DDIMSampler(_StubLDM(m))
    B, h, S = 2, 64, 50
    x_T = rnd((B, 4, h, h), 480)
    mask = (rnd((B, 1, h, h), 482) > 0).float()
    z_inp = rnd((B, 4, h, h), 481) * mask
    c = rnd((B, 1, 768), 483)
    uc = rnd((1, 1, 768), 484).repeat(B, 1, 1)
    t0 = time.time()
    samples, inter = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False, unconditional_guidance_scale=3.5,
                                    unconditional_conditioning=uc, eta=0.0, x_T=x_T, log_every_t=100,
                                    test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
    print(f"  reference DDIM S={S} B={B} full width: {time.time() - t0:.0f}s")
    del m, sampler
    vae, _ = _ref_vae(P.VAEConfig(), 55)
    img = vae.decode(samples / 0.18215)
    save("ddim_full_S50_B2", samples=samples, pred_x0_last=inter["pred_x0"][-1], image_stride8=img[:, :, ::8, ::8].contiguous(),
         image_absmax=img.abs().max(), seed_unet=1234, seed_vae=55, scale=3.5, S=S)


def gen_plms():
    """PLMSSampler (plms.py) with CFG on the reduced-width UNet, and LatentDiffusion.q_sample (ddpm.py:412-415)."""
    from ldm.models.diffusion.plms import PLMSSampler
    PLMSSampler.register_buffer = lambda self, n, a: setattr(self, n, a)
    cfg = P.UNetConfig(**SMALL_UNET)
    m, _ = _ref_unet(cfg, 7)
    ldm = _StubLDM(m)
    sampler = PLMSSampler(ldm)
    B, h = 2, 16
    x_T = rnd((B, 4, h, h), 30)
    z_inp = rnd((B, 4, h, h), 31)
    mask = (rnd((B, 1, h, h), 32) > 0).float()
    c = rnd((B, 1, 768), 33)
    uc = rnd((1, 1, 768), 34).repeat(B, 1, 1)
    for S in (5, 10):
        samples, inter = sampler.sample(S=S, conditioning=c, batch_size=B, shape=[4, h, h], verbose=False,
                                        unconditional_guidance_scale=3.5, unconditional_conditioning=uc, eta=0.0, x_T=x_T,
                                        test_model_kwargs={"inpaint_image": z_inp, "inpaint_mask": mask})
        save(f"plms_small_S{S}", samples=samples, pred_x0_last=inter["pred_x0"][-1], n_inter=len(inter["x_inter"]), seed=7, scale=3.5)
    # q_sample through the reference DDPM buffers (register_schedule, fp32)
    from ldm.models.diffusion.ddpm import DDPM
    from reface_amd.schedule import ddpm_buffers
    bufs = ddpm_buffers(1000, 0.00085, 0.0120)
    host = type("H", (), {})()
    host.sqrt_alphas_cumprod = bufs["sqrt_alphas_cumprod"]
    host.sqrt_one_minus_alphas_cumprod = bufs["sqrt_one_minus_alphas_cumprod"]
    z = rnd((B, 4, h, h), 35)
    noise = rnd((B, 4, h, h), 36)
    t = torch.tensor([999, 417])
    save("q_sample", x=DDPM.q_sample(host, z, t, noise), t=t)


SMALL_VAE = dict(ch=32, ch_mult=(1, 2, 4, 4), num_res_blocks=2, in_channels=3, out_ch=3, z_channels=4,
                 embed_dim=4, double_z=True, attn_resolutions=(), resolution=256)


def _ref_vae(cfg: P.VAEConfig, seed):
    from ldm.models.autoencoder import AutoencoderKL
    dd = dict(double_z=True, z_channels=cfg.z_channels, resolution=256, in_channels=cfg.in_channels,
              out_ch=cfg.out_ch, ch=cfg.ch, ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks,
              attn_resolutions=[], dropout=0.0)
    m = AutoencoderKL(ddconfig=dd, lossconfig={"target": "torch.nn.Identity"}, embed_dim=cfg.embed_dim).eval()
    sd = P.seeded_state_dict(P.vae_param_specs(cfg), seed)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing[:5], unexpected[:5])
    return m, sd


def gen_vae():
    import collections
    from ldm.modules.diffusionmodules.model import ResnetBlock, AttnBlock
    cfg = P.VAEConfig(**SMALL_VAE)
    m, _ = _ref_vae(cfg, 55)
    x = torch.tanh(rnd((2, 3, 64, 64), 40))
    post = m.encode(x)
    z = rnd((2, 4, 8, 8), 41)
    save("vae_small", mean=post.mean, logvar=post.logvar, dec=m.decode(z), seed=55)
    # full-width single blocks
    res = {}
    for tag, cin, cout, hw in (("a", 512, 512, 16), ("b", 512, 256, 16), ("c", 128, 128, 32)):
        blk = ResnetBlock(in_channels=cin, out_channels=cout, temb_channels=0, dropout=0.0).eval()
        s = collections.OrderedDict()
        P._vae_res(s, "r", cin, cout)
        sd = P.seeded_state_dict(s, 56)
        load_strict(blk, {k[2:]: v for k, v in sd.items()})
        xx = rnd((1, cin, hw, hw), 42)
        res[f"res_{tag}_y"] = blk(xx, None)
    ab = AttnBlock(512).eval()
    s = collections.OrderedDict()
    P._vae_attn(s, "a", 512)
    sd = P.seeded_state_dict(s, 57)
    load_strict(ab, {k[2:]: v for k, v in sd.items()})
    xx = rnd((1, 512, 16, 16), 43)
    res["attn_y"] = ab(xx)
    save("vae_blocks", **res)


def gen_arcface():
    from src.Face_models.encoders.model_irse import Backbone
    import ldm.models.diffusion.ddpm as ddpm
    net = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se").eval()
    sd = P.seeded_state_dict(P.arcface_param_specs(), 77)
    load_strict(net, sd)
    idl = ddpm.IDLoss.__new__(ddpm.IDLoss)
    torch.nn.Module.__init__(idl)
    idl.multiscale = False
    idl.face_pool_1 = torch.nn.AdaptiveAvgPool2d((256, 256))
    idl.face_pool_2 = torch.nn.AdaptiveAvgPool2d((112, 112))
    idl.facenet = net
    ref = rnd((2, 3, 224, 224), 50)
    feats = idl.extract_feats(ref)[0]
    x112 = rnd((2, 3, 112, 112), 51)
    save("arcface", feats=feats, feats112=net(x112)[0], seed=77)


SMALL_CLIP = dict(hidden=128, intermediate=512, layers=2, heads=4, patch=14, image=224, proj=768, mapper_layers=5)


def _hf_clip(cfg: P.CLIPVisionConfig):
    from transformers import CLIPConfig, CLIPModel
    c = CLIPConfig(projection_dim=cfg.proj,
                   vision_config=dict(hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                                      num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                                      patch_size=cfg.patch, image_size=cfg.image, hidden_act="quick_gelu"),
                   text_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                    num_attention_heads=2, vocab_size=100, max_position_embeddings=77,
                                    hidden_act="quick_gelu"))
    return CLIPModel(c)


def _ref_clip_embedder(cfg: P.CLIPVisionConfig, seed):
    import ldm.modules.encoders.modules as M
    from transformers import CLIPModel, CLIPTokenizer
    orig_m, orig_t = CLIPModel.from_pretrained, CLIPTokenizer.from_pretrained
    CLIPModel.from_pretrained = classmethod(lambda cls, *a, **k: _hf_clip(cfg))
    CLIPTokenizer.from_pretrained = classmethod(lambda cls, *a, **k: None)
    try:
        emb = M.FrozenCLIPEmbedder().eval()
    finally:
        CLIPModel.from_pretrained, CLIPTokenizer.from_pretrained = orig_m, orig_t
    sd = P.seeded_state_dict(P.clip_param_specs(cfg), seed)
    have = emb.state_dict()
    # HF >= 5 may nest the vision tower one level deeper; map our 4.19-layout keys onto it.
    remap = {}
    for k in sd:
        if k in have:
            remap[k] = k
        else:
            alt = k.replace("model.vision_model.", "model.vision_model.vision_model.")
            assert alt in have, k
            remap[k] = alt
    missing, unexpected = emb.load_state_dict({remap[k]: v for k, v in sd.items()}, strict=False)
    assert not unexpected, unexpected[:5]
    used = [k for k in missing if ("vision_model" in k or "visual_projection" in k or "mapper2" in k or "final_ln2" in k)
            and "position_ids" not in k]
    assert not used, used[:5]
    return emb, sd


def gen_clip():
    cfg = P.CLIPVisionConfig(**SMALL_CLIP)
    emb, _ = _ref_clip_embedder(cfg, 88)
    img = rnd((2, 3, 224, 224), 60)
    pooled = emb.model.vision_model(pixel_values=img).pooler_output
    save("clip_small", pooled=pooled, z=emb(img), seed=88)
    # one full-width ViT-L/14 layer stack (1 layer) to pin 1024/16-head shapes
    cfg1 = P.CLIPVisionConfig(layers=1)
    emb1, _ = _ref_clip_embedder(cfg1, 89)
    img1 = rnd((1, 3, 224, 224), 61)
    save("clip_l14_1layer", z=emb1(img1), seed=89)


def gen_e2e():
    """Whole reference chain (inference_test_bench.py:441-495) at reduced widths: LatentDiffusion
    built through the reference registry from a config dict shaped like configs/train.yaml."""
    import yaml
    from ldm.util import instantiate_from_config
    from ldm.models.diffusion.ddim import DDIMSampler
    from transformers import CLIPModel, CLIPTokenizer
    import tempfile
    DDIMSampler.register_buffer = lambda self, n, a: setattr(self, n, a)
    raw = yaml.safe_load(open("/root/reference/configs/train.yaml"))
    mp = raw["model"]["params"]
    mp["unet_config"]["params"]["model_channels"] = 64
    mp["first_stage_config"]["params"]["ddconfig"]["ch"] = 32
    ccfg = P.CLIPVisionConfig(**SMALL_CLIP)
    arc_sd = P.seeded_state_dict(P.arcface_param_specs(), 77)
    with tempfile.NamedTemporaryFile(suffix=".pth", delete=False) as f:
        torch.save(arc_sd, f.name)
        arc_path = f.name
    mp["cond_stage_config"]["other_params"]["arcface_path"] = arc_path
    cfg = ref_shims.to_attr(raw)
    orig_m, orig_t = CLIPModel.from_pretrained, CLIPTokenizer.from_pretrained
    CLIPModel.from_pretrained = classmethod(lambda cls, *a, **k: _hf_clip(ccfg))
    CLIPTokenizer.from_pretrained = classmethod(lambda cls, *a, **k: None)
    try:
        model = instantiate_from_config(cfg.model).eval()
    finally:
        CLIPModel.from_pretrained, CLIPTokenizer.from_pretrained = orig_m, orig_t
        os.unlink(arc_path)
    # our seeded weights under the checkpoint prefixes
    sd = {}
    sd.update(P.seeded_state_dict(P.unet_param_specs(P.UNetConfig(**SMALL_UNET)), 7, "model.diffusion_model."))
    sd.update(P.seeded_state_dict(P.vae_param_specs(P.VAEConfig(**SMALL_VAE)), 55, "first_stage_model."))
    csd = P.seeded_state_dict(P.clip_param_specs(ccfg), 88, "cond_stage_model.")
    have = model.state_dict()
    for k, v in csd.items():
        if k not in have:
            k = k.replace("model.vision_model.", "model.vision_model.vision_model.")
            assert k in have, k
        sd[k] = v
    sd.update({"face_ID_model.facenet." + k: v for k, v in arc_sd.items()})
    sd.update(P.seeded_state_dict(P.cond_head_specs(), 9))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected[:8]
    crit = [k for k in missing if not any(s in k for s in (
        "text_model", "text_projection", "logit_scale", "mapper.", "final_ln.", "projection_back", "position_ids",
        "betas", "alphas", "sqrt_", "log_one", "posterior", "logvar", "lvlb"))]
    assert not crit, crit[:8]
    print("  e2e model built; unused-at-inference params left at ctor init:", len(missing))

    B, H = 2, 256
    target = torch.tanh(rnd((B, 3, H, H), 70))
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
    ell = (((yy - H / 2) / (0.30 * H)) ** 2 + ((xx - H / 2) / (0.38 * H)) ** 2) <= 1.0
    inpaint_mask = (~ell).float()[None, None].repeat(B, 1, 1, 1)
    inpaint_image = target * inpaint_mask
    ref = rnd((B, 3, 224, 224), 71)
    x_T = rnd((B, 4, H // 8, H // 8), 72)

    sampler = DDIMSampler(model)
    uc = model.learnable_vector.repeat(B, 1, 1)
    landmarks = model.get_landmarks(target)                       # dlib stub: no faces -> zeros(136) -> proj
    c = model.conditioning_with_feat(ref, landmarks=landmarks, tar=target).float()
    torch.manual_seed(4242)
    z_inpaint = model.get_first_stage_encoding(model.encode_first_stage(inpaint_image)).detach()
    torch.manual_seed(4242)
    eps = torch.randn(z_inpaint.shape)
    post = model.encode_first_stage(inpaint_image)
    from torchvision.transforms import Resize
    mask64 = Resize([H // 8, H // 8])(inpaint_mask)
    samples, _ = sampler.sample(S=5, conditioning=c, batch_size=B, shape=[4, H // 8, H // 8], verbose=False,
                                unconditional_guidance_scale=3.5, unconditional_conditioning=uc, eta=0.0,
                                x_T=x_T, test_model_kwargs={"inpaint_image": z_inpaint, "inpaint_mask": mask64})
    x_dec = model.decode_first_stage(samples)
    x_img = torch.clamp((x_dec + 1.0) / 2.0, min=0.0, max=1.0)
    u8 = (255.0 * x_img.permute(0, 2, 3, 1).numpy()).astype(np.uint8)
    save("e2e_small", landmarks=landmarks, c=c, uc=uc, post_mean=post.mean, post_logvar=post.logvar, eps=eps,
         z_inpaint=z_inpaint, mask64=mask64, samples=samples, x_dec=x_dec, u8=u8)

    # ---- the on-disk output tree: the reference's OWN statements (scripts/inference_test_bench.py:500-552, read from the
    # reference tree at generation time, never stored) executed on this run's tensors; PIL's save is replaced by a recorder.
    import textwrap
    import types as _types
    from einops import rearrange
    from torchvision.utils import make_grid                   # tools/ref_shims.py restatement (torchvision is not installed)
    src = open("/root/reference/scripts/inference_test_bench.py").read().split("\n")
    assert src[499].strip() == "def un_norm(x):" and src[551].strip().startswith("ref_img.save("), (src[499], src[551])
    block = textwrap.dedent("\n".join(src[499:552]))
    written = {}

    class _Rec:
        def __init__(self, a):
            self.a = np.array(a)

        def save(self, path):
            written[os.path.basename(path)] = self.a

    cv2 = _types.SimpleNamespace(COLOR_GRAY2RGB=8, cvtColor=lambda a, code: np.repeat(a, 3, axis=2))      # GRAY2RGB replicates the channel
    ns = dict(torch=torch, np=np, os=os, rearrange=rearrange, make_grid=make_grid, Resize=lambda sz: Resize([H, H]), cv2=cv2,
              Image=_types.SimpleNamespace(fromarray=_Rec), opt=_types.SimpleNamespace(skip_save=False),
              x_checked_image_torch=x_img, test_batch=target, inpaint_image=inpaint_image, inpaint_mask=inpaint_mask,
              test_model_kwargs={"ref_imgs": ref.unsqueeze(1)}, segment_id_batch=["a", "b"], grid_path="g", result_path="r",
              sample_path="s", base_count=0)
    exec(block, ns)
    assert sorted(written) == ["a.png", "a_GT.png", "a_inpaint.png", "a_mask.png", "a_ref.png", "b.png", "b_GT.png", "b_inpaint.png",
                               "b_mask.png", "b_ref.png", "grid-a.png", "grid-b.png"], sorted(written)
    # item 0 only (random images do not compress): grid carries the GT / inpaint / ref / result panels
    g0 = written["grid-a.png"]
    for k, nm in enumerate(("a_GT.png", "a_inpaint.png", "a_ref.png", "a.png")):       # the individual files ARE the grid's panels
        assert np.array_equal(g0[2:2 + H, 2 + k * (H + 2):2 + k * (H + 2) + H], written[nm]), nm
    save("e2e_png", grid=g0, mask=written["a_mask.png"])


def seeded_u8(shape, seed):
    """Deterministic uint8 image tensor (the parser fixtures' inputs; tests/test_parsing_gpu.py regenerates them the same way)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randint(0, 256, tuple(shape), generator=g, dtype=torch.uint8)


def _import_face_parsing():
    """The reference's face parser modules, imported without network, GPU or OpenCV:
    * model.py moves seg_mean / seg_std to the GPU at import time: Tensor.cuda is the identity during that import only;
    * face_parsing_demo.py imports cv2 (absent here): a stub module;
    * Resnet18.__init__ calls model_zoo.load_url(resnet18_url), which would DOWNLOAD the ImageNet weights: load_url and
      load_state_dict_from_url are replaced by stubs returning an empty dict (no I/O) -- the seeded weights are loaded afterwards.
    The repository ships its own `pretrained` package (the drop-in demo module): `pretrained` is pinned to the reference tree."""
    import types
    import torch.hub
    import torch.utils.model_zoo
    no_io = lambda *a, **k: {}                  # noqa: E731
    torch.utils.model_zoo.load_url = no_io
    torch.hub.load_state_dict_from_url = no_io
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    pre = types.ModuleType("pretrained")
    pre.__path__ = ["/root/reference/pretrained"]
    sys.modules["pretrained"] = pre
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        import pretrained.face_parsing.model as fpm
        import pretrained.face_parsing.face_parsing_demo as fpd
    finally:
        torch.Tensor.cuda = cuda
    assert fpm.seg_mean.device.type == "cpu"
    return fpm, fpd


def gen_bisenet():
    """BiSeNet face parser (pretrained/face_parsing/): key layout, seg12 LUT, prep output and the 64^2 logits + 512^2 label maps of a 1024^2
    batch, all from the reference's own modules on CPU with seeded weights."""
    import json
    import torch.nn.functional as F
    fpm, fpd = _import_face_parsing()
    import torch.utils.model_zoo
    assert torch.utils.model_zoo.load_url("x") == {}            # never construct the net without the no-download stub
    net = fpm.BiSeNet(n_classes=19).eval()
    keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    sd = P.seeded_state_dict(P.bisenet_param_specs(), 91)
    load_strict(net, sd)
    path = os.path.join(OUT, "bisenet_keys.json")
    json.dump(keys, open(path, "w"), separators=(",", ":"))
    print(f"  wrote {path}  ({len(keys)} keys)")
    conv = getattr(fpd, "__ffhq_masks_to_faceParser_mask_detailed")        # module-level double-underscore name: no mangling
    lut = conv(np.arange(19, dtype=np.uint8))
    down = fpd.BicubicDownSample(factor=2, cuda=False)

    def prep(u8):                                # FaceParser.preprocess_img on a batch (>= 512 px branch): ToTensor -> downsample -> clamp -> normalise
        x = u8.permute(0, 3, 1, 2).float().div(255)
        return (down(x).clamp(0, 1) - fpm.seg_mean) / fpm.seg_std

    small = seeded_u8((1, 96, 128, 3), 92)
    prep_small = prep(small)
    big = seeded_u8((2, 1024, 1024, 3), 93)
    xb = prep(big)
    got = {}
    h = net.conv_out.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o))
    out = net(xb)[0]
    h.remove()
    labels = torch.argmax(out, dim=1).numpy().astype(np.uint8)
    assert np.array_equal(F.interpolate(got["logits"], (512, 512), mode="bilinear", align_corners=True).argmax(1).numpy(), labels)
    seg12 = np.stack([conv(l) for l in labels])
    save("bisenet", lut_seg12=lut, prep_small=prep_small, logits=got["logits"], labels=labels, labels_seg12=seg12,
         seed=91, small_seed=92, big_seed=93)


def seeded_frame(h, w, c, seed, block=4):
    """Deterministic uint8 frame [h, w, c]: seeded noise in block x block tiles (tests/test_align_cpu.py regenerates it the same way); a
    fourth channel is alpha 255 (a decoded video frame is opaque)."""
    a = seeded_u8(((h + block - 1) // block, (w + block - 1) // block, 3), seed).numpy()
    a = np.repeat(np.repeat(a, block, axis=0), block, axis=1)[:h, :w]
    return np.concatenate([a, np.full((h, w, 1), 255, np.uint8)], axis=2) if c == 4 else a


def synthetic_landmarks(centre, eye_dist, degrees, seed):
    """68 landmarks of a made-up face: eye centres eye_dist apart around `centre`, the mouth 0.9 eye_dist below them, turned by `degrees`;
    every point jittered by a seeded fraction of a pixel (non-integer coordinates)."""
    rng = np.random.default_rng(seed)
    t = np.deg2rad(degrees)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    lm = rng.uniform(-1.0, 1.0, (68, 2)) * eye_dist
    lm[36:42] = np.array([-0.5, 0.0]) * eye_dist + rng.uniform(-0.12, 0.12, (6, 2)) * eye_dist
    lm[42:48] = np.array([0.5, 0.0]) * eye_dist + rng.uniform(-0.12, 0.12, (6, 2)) * eye_dist
    lm[48:60] = np.array([0.0, 0.9]) * eye_dist + rng.uniform(-0.3, 0.3, (12, 2)) * eye_dist
    lm[48], lm[54] = np.array([-0.35, 0.9]) * eye_dist, np.array([0.37, 0.92]) * eye_dist
    return lm @ R.T + np.asarray(centre, dtype=np.float64)


# (name, W, H, channels, frame seed, face centre, eye distance, rotation in degrees): a quad well inside its frame, one hanging over the
# top and left edges, an RGBA frame, and a face large enough for crop_image's LANCZOS shrink at both output sizes (6 at 128, 3 at 256)
ALIGN_CASES = [("inside", 640, 480, 3, 201, (330.0, 215.0), 50.0, 12.0), ("over_edges", 700, 500, 3, 202, (120.0, 95.0), 90.0, -9.0),
               ("rgba", 640, 480, 4, 203, (300.0, 230.0), 60.0, -20.0), ("shrink", 2401, 1799, 3, 204, (1200.0, 800.0), 300.0, 7.0)]
ALIGN_SIZES = (128, 256)


def gen_align():
    """Face alignment (src/utils/alignmengt.py): c, x, y and the quad of compute_transform, crop_image's crops at two output sizes and
    calc_alignment_coefficients' inverse transforms, from the reference's own functions on synthetic frames and landmarks.  The packages
    that file imports and this container lacks (skimage, cv2; dlib is stubbed by ref_shims) carry no arithmetic used here."""
    import importlib
    import PIL.Image
    for name in ("skimage", "skimage.io", "cv2", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = ref_shims._mod(name)
            if name == "tqdm":
                m.tqdm = lambda it, **k: it
    if not hasattr(PIL.Image, "ANTIALIAS"):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS          # the name Pillow 10 dropped
    from src.utils import alignmengt as A
    out = {"names": np.array([c[0] for c in ALIGN_CASES]), "sizes": np.array(ALIGN_SIZES),
           "frames": np.array([c[1:5] for c in ALIGN_CASES], dtype=np.int64)}          # W, H, channels, seed
    for name, W, H, C, seed, centre, eye, deg in ALIGN_CASES:
        lm = synthetic_landmarks(centre, eye, deg, seed + 100)
        A.get_landmark = lambda *a, **k: lm
        c, x, y = A.compute_transform("unused", None)
        quad = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])
        frame = PIL.Image.fromarray(seeded_frame(H, W, C, seed))
        out.update({f"{name}_landmarks": lm, f"{name}_c": c, f"{name}_x": x, f"{name}_y": y, f"{name}_quad": quad})
        for S in ALIGN_SIZES:
            crop = A.crop_image(frame, S, quad.copy()).convert("RGB")
            assert crop.size == (S, S)
            out[f"{name}_crop{S}"] = np.asarray(crop)
            out[f"{name}_inv{S}"] = A.calc_alignment_coefficients(quad + 0.5, [[0, 0], [0, S], [S, S], [S, 0]])
    save("align", **out)


# (name, H, W, frame seed, quad centre, half-axis, rotation in degrees, output size): faces over the left edge and over a corner, pads
# larger than the window (numpy's reflect folds more than once), a window one pixel wide, a LANCZOS shrink before the pad, and a face
# inside its frame (the padding does not trigger: today's crop)
ALIGN_PAD_CASES = [("left_edge", 96, 128, 301, (10.3, 50.2), 22.0, 7.0, 32), ("corner", 80, 90, 302, (84.0, 75.5), 18.5, -12.0, 24),
                   ("multi_reflect", 40, 200, 303, (100.2, 20.1), 45.0, 3.0, 32), ("one_px", 64, 64, 304, (-13.5, 30.0), 11.0, 0.0, 16),
                   ("shrunk", 300, 400, 305, (30.0, 150.0), 70.0, 10.0, 16), ("interior", 128, 128, 306, (64.0, 64.0), 20.0, 5.0, 32)]


def pad_case_quad(centre, half, deg):
    a = np.radians(deg)
    c, x = np.asarray(centre, dtype=np.float64), half * np.array([np.cos(a), np.sin(a)])
    y = np.array([-x[1], x[0]])
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y])


def gen_align_pad():
    """crop_image(..., enable_padding=True) of the reference on ALIGN_PAD_CASES: per case the frame's seed and size, the quad, S, the crop and
    the padded u8 image the transform read (caught at PIL.Image.fromarray, which only the padding branch calls; empty when it did not run)."""
    import importlib
    import PIL.Image
    for name in ("skimage", "skimage.io", "cv2", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = ref_shims._mod(name)
            if name == "tqdm":
                m.tqdm = lambda it, **k: it
    if not hasattr(PIL.Image, "ANTIALIAS"):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
    from src.utils import alignmengt as A
    out = {"names": np.array([c[0] for c in ALIGN_PAD_CASES]), "frames": np.array([(c[1], c[2], c[3], c[7]) for c in ALIGN_PAD_CASES], dtype=np.int64)}
    fromarray, seen = PIL.Image.fromarray, []

    def spy(a, *args, **kw):
        seen.append(np.array(a))
        return fromarray(a, *args, **kw)
    for name, H, W, seed, centre, half, deg, S in ALIGN_PAD_CASES:
        quad = pad_case_quad(centre, half, deg)
        frame = fromarray(seeded_frame(H, W, 3, seed))
        del seen[:]
        PIL.Image.fromarray = spy
        try:
            crop = A.crop_image(frame, S, quad.copy(), enable_padding=True).convert("RGB")
        finally:
            PIL.Image.fromarray = fromarray
        assert crop.size == (S, S) and len(seen) == (name != "interior"), (name, len(seen))
        out.update({f"{name}_quad": quad, f"{name}_crop": np.asarray(crop), f"{name}_padded": seen[0] if seen else np.zeros((0, 0, 3), np.uint8)})
    save("align_pad", **out)


def _install_tv_transforms():
    """torchvision.transforms' ToTensor, Normalize, Compose and Resize (on a tensor: bilinear, align_corners=False, no antialias at any size --
    torchvision 0.12) restated on the stub ``torchvision`` of tools/ref_shims.py, for the evaluation tools of the reference."""
    import torch.nn.functional as F
    tvt = sys.modules["torchvision.transforms"]

    class ToTensor:
        def __call__(self, img):
            a = np.asarray(img, dtype=np.uint8)
            a = a[:, :, None] if a.ndim == 2 else a
            return torch.from_numpy(a.transpose(2, 0, 1).copy()).to(torch.float32).div(255)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, t):
            return sys.modules["torchvision.transforms.functional"].normalize(t, self.mean, self.std)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Resize:
        def __init__(self, size, *a, **k):
            self.size = tuple(size)

        def __call__(self, t):
            assert torch.is_tensor(t) and t.dim() == 3
            return F.interpolate(t[None], size=self.size, mode="bilinear", align_corners=False, antialias=False)[0]

    tvt.ToTensor, tvt.Normalize, tvt.Compose, tvt.Resize = ToTensor, Normalize, Compose, Resize
    sys.modules["torchvision"].transforms = tvt


def gen_idscore():
    """The identity metric (eval_tool/ID_retrieval/ID_retrieval.py): the reference's own MaskedImagePathDataset, IDLoss.extract_feats and
    calculate_id_given_paths on the seeded PNG folders of tests/idscore_inputs.py, ArcFace with the seeded weights (as gen_arcface).  The
    packages that file imports and this container lacks are stubbed: natsort (reface_amd.idscore.natural_key), albumentations' Resize and
    cv2 (imread / cvtColor over PIL on PNG inputs -- lossless, so the bytes are cv2's; A.Resize = cv2.resize INTER_LINEAR is RESTATED by
    reface_amd.data.resize_u8_linear, not run: cv2 is absent here, see README) and the torchvision transforms it uses (ToTensor,
    Normalize, Compose, Resize on a tensor = bilinear, align_corners=False, no antialias: torchvision 0.12).  Stored: the prepared tensors of
    a few images, all features, labels, top-1 / top-5 / mean / similarities, the label's rank per result and the boundary gaps (the score
    distance of the label to the nearest score across the rank 1|2 and 5|6 boundaries); a fixture whose smallest gap is below 1e-2 is
    refused, so that exact top-k agreement can be asked of every implementation."""
    import importlib
    import importlib.util
    import tempfile
    import types
    import PIL.Image
    import torch.nn.functional as F
    sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))
    import idscore_inputs as I
    from reface_amd import idscore as S
    from reface_amd.data import resize_u8_linear

    cv2 = ref_shims._mod("cv2")
    cv2.COLOR_BGR2RGB = 4
    cv2.imread = lambda path: np.asarray(PIL.Image.open(path).convert("RGB"), dtype=np.uint8)[:, :, ::-1].copy()
    cv2.cvtColor = lambda img, code: img[:, :, ::-1].copy()
    alb = ref_shims._mod("albumentations")
    alb.Resize = lambda height, width: (lambda image: resize_u8_linear(image, height, width))
    alb.Compose = lambda ts: (lambda image: {"image": ts[0](image)})
    ns = ref_shims._mod("natsort")
    ns.natsorted = lambda seq: sorted(seq, key=lambda f: S.natural_key(str(f)))
    for name in ("tqdm", "scipy"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = ref_shims._mod(name)
            m.tqdm = lambda it, **k: it
            m.linalg = None
    _install_tv_transforms()
    # by path: `eval_tool` is a stub module in ref_shims and a package of this repository; neither is the reference's
    spec = importlib.util.spec_from_file_location("ref_id_retrieval", "/root/reference/eval_tool/ID_retrieval/ID_retrieval.py")
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    net = R.Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode="ir_se").eval()
    load_strict(net, P.seeded_state_dict(P.arcface_param_specs(), S.ARCFACE_TEST_SEED))
    idl = R.IDLoss.__new__(R.IDLoss)
    torch.nn.Module.__init__(idl)
    idl.multiscale = True
    idl.face_pool_1 = torch.nn.AdaptiveAvgPool2d((256, 256))
    idl.face_pool_2 = torch.nn.AdaptiveAvgPool2d((112, 112))
    idl.facenet = net
    idl.eval()
    idl.cuda = lambda: idl
    R.IDLoss = lambda: idl

    data = I.build()
    with tempfile.TemporaryDirectory() as tmp:
        paths = I.write_folders(tmp, data)
        lists = [R.natsorted([os.path.join(p, n) for n in os.listdir(p)]) for p in paths]
        assert [os.path.basename(f) for f in lists[0]] == data["src_names"] and [os.path.basename(f) for f in lists[1]] == data["res_names"]
        ds_src = R.MaskedImagePathDataset(lists[0], maskfiles=lists[2], data_name=I.DATASET)
        ds_res = R.MaskedImagePathDataset(lists[1], maskfiles=lists[3], data_name=I.DATASET)
        x_src = torch.cat([ds_src[i] for i in range(len(ds_src))])
        x_res = torch.cat([ds_res[i] for i in range(len(ds_res))])
        f_src = idl.extract_feats(x_src)[-1]
        f_res = idl.extract_feats(x_res)[-1]
        args = types.SimpleNamespace(arcface=True)
        top1, top5, mean, sims = R.calculate_id_given_paths(paths, 16, torch.device("cpu"), 2048, 0, data_name=I.DATASET, args=args)
        ds_all = R.MaskedImagePathDataset(lists[0], maskfiles=lists[2], data_name="other")          # every label kept: the image resize alone
        x_nomask = torch.cat([ds_all[i] for i in I.PREP_SAMPLES["src"]])
    labels = data["labels"]
    h = S.score_host(f_src.numpy(), f_res.numpy(), labels)
    assert h["top1"] == top1 and h["top5"] == top5, (h["top1"], top1, h["top5"], top5)
    assert np.abs(h["similarities"] - sims).max() < 1e-12 and abs(h["mean"] - mean) < 1e-12
    gaps = S.boundary_gaps(f_src.numpy(), f_res.numpy(), labels)
    print(f"  top1 {top1:.4f}  top5 {top5:.4f}  mean {mean:.4f}  ranks {h['rank'].tolist()}")
    print(f"  similarities {np.round(sims, 3).tolist()}")
    print(f"  smallest boundary gap {gaps.min():.4f}")
    if gaps.min() < 1e-2:
        raise SystemExit(f"gen_idscore: smallest boundary gap {gaps.min():.3e} < 1e-2: not a fixture for exact top-k checks; change the seeds")
    assert 0.0 < top1 < top5 < 1.0, "the fixture must leave both accuracies non-trivial"
    save("idscore", prep_src=x_src[I.PREP_SAMPLES["src"]], prep_res=x_res[I.PREP_SAMPLES["res"]], prep_src_nomask=x_nomask,
         f_src=f_src, f_res=f_res, labels=labels, top1=np.float64(top1), top5=np.float64(top5), mean=np.float64(mean),
         similarities=np.asarray(sims, dtype=np.float64), rank=h["rank"], pred=h["pred"], gaps=gaps, seed=S.ARCFACE_TEST_SEED)


def _tv_bottleneck():
    """torchvision 0.12's ``models.resnet.Bottleneck`` restated (torchvision is absent here, see README): 1x1 -> 3x3 -> 1x1 convolutions
    without bias, each followed by BatchNorm, ReLU after the first two, the stride on the 3x3 ``conv2`` (the "v1.5" placement),
    ``out = relu(bn3(conv3(.)) + identity)`` with ``identity = downsample(x)`` where a downsample is given.  Module names, hence
    state-dict keys, are torchvision's."""
    nn = torch.nn

    class Bottleneck(nn.Module):
        expansion = 4

        def __init__(self, inplanes, planes, stride=1, downsample=None):
            super().__init__()
            self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
            self.bn1 = nn.BatchNorm2d(planes)
            self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
            self.bn2 = nn.BatchNorm2d(planes)
            self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
            self.bn3 = nn.BatchNorm2d(planes * self.expansion)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = downsample
            self.stride = stride

        def forward(self, x):
            identity = x if self.downsample is None else self.downsample(x)
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            return self.relu(out + identity)

    return Bottleneck


def gen_pose():
    """The pose metric (eval_tool/Pose/pose_compare.py over eval_tool/face_vid2vid/modules/hopenet.py): the reference's own Hopenet,
    ImagePathDataset, compute_features and calculate_id_given_paths on the seeded PNG folders of tests/pose_inputs.py, with the seeded
    weights in place of the checkpoint file.  Both files are loaded by path.  What this container lacks is stubbed: natsort
    (reface_amd.idscore.natural_key), the torchvision transforms (_install_tv_transforms) and torchvision.models.resnet.Bottleneck
    (_tv_bottleneck); torch.load of the checkpoint path returns the seeded state dict.  Stored: the state-dict key layout of the reference
    module, the labels, the prepared tensors of two images (a downscale and the upscale), the degrees of all images in fp32 (the reference
    as it runs) and from the same module and inputs in float64, and the distances and Pose_value of both.  A degenerate fixture is refused:
    every angle must vary by >= 0.1 degree (std) over the images, no softmax may be saturated (max <= 0.9), Pose_value >= 0.2 degree, and
    labelling by the first number or pairing by position must each move Pose_value by more than 0.05 degree."""
    import importlib
    import importlib.util
    import tempfile
    sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))
    import pose_inputs as I
    from reface_amd import idscore as S
    from reface_amd import posescore as PS

    ns = ref_shims._mod("natsort")
    ns.natsorted = lambda seq: sorted(seq, key=lambda f: S.natural_key(str(f)))
    for name in ("tqdm", "scipy"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = ref_shims._mod(name)
            m.tqdm = lambda it, **k: it
            m.linalg = None
    _install_tv_transforms()
    Bottleneck = _tv_bottleneck()
    tvr = ref_shims._mod("torchvision.models.resnet")
    tvr.Bottleneck = Bottleneck
    sys.modules["torchvision.models"].resnet = tvr
    # by path: `eval_tool` is a stub module in ref_shims and a package of this repository; neither is the reference's
    spec = importlib.util.spec_from_file_location("eval_tool.face_vid2vid.modules.hopenet", "/root/reference/eval_tool/face_vid2vid/modules/hopenet.py")
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    ref_shims._mod("eval_tool.face_vid2vid")
    ref_shims._mod("eval_tool.face_vid2vid.modules").hopenet = H
    sys.modules["eval_tool.face_vid2vid.modules.hopenet"] = H
    spec = importlib.util.spec_from_file_location("ref_pose_compare", "/root/reference/eval_tool/Pose/pose_compare.py")
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    net = H.Hopenet(Bottleneck, [3, 4, 6, 3], 66).eval()
    ref_sd = net.state_dict()
    keys = np.array(list(ref_sd.keys()))
    shapes = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
    assert len(keys) == 326, len(keys)
    sd = P.seeded_state_dict(P.hopenet_param_specs(), PS.SEED)
    net.load_state_dict(sd, strict=True)

    data = I.build()
    labels = data["labels"]
    with tempfile.TemporaryDirectory() as tmp:
        paths = I.write_folders(tmp, data)
        lists = [R.natsorted([os.path.join(p, n) for n in os.listdir(p)]) for p in paths]
        assert [os.path.basename(f) for f in lists[0]] == data["tgt_names"] and [os.path.basename(f) for f in lists[1]] == data["res_names"]
        load = torch.load
        torch.load = lambda *a, **k: sd          # the checkpoint path of calculate_id_given_paths
        try:
            value = float(R.calculate_id_given_paths(paths, 20, torch.device("cpu"), 2048, 0))
            _, ref_labels = R.compute_features_wrapp(paths[1], net, 20, 2048, torch.device("cpu"), 0)
        finally:
            torch.load = load
        assert list(ref_labels) == labels.tolist(), (ref_labels, labels)
        deg32 = [R.compute_features(files, net, 20, 2048, torch.device("cpu"), 0) for files in lists]
        x = [torch.stack([t for t in R.ImagePathDataset(files)]) for files in lists]
    prep = x[0][I.PREP_SAMPLES["tgt"]]
    net64 = H.Hopenet(Bottleneck, [3, 4, 6, 3], 66).eval()
    net64.load_state_dict(sd, strict=True)
    net64.double()
    deg64, pmax = [], 0.0
    for xs in x:
        heads = net64(xs.double())
        pmax = max([pmax] + [float(torch.softmax(h, dim=1).max()) for h in heads])
        deg64.append(torch.stack([R.headpose_pred_to_degree(h) for h in heads], dim=1).numpy())
    assert deg64[0].dtype == np.float64 and deg32[0].dtype == np.float64

    h32 = PS.score_host(deg32[0], deg32[1], labels)
    h64 = PS.score_host(deg64[0], deg64[1], labels)
    assert abs(h32["pose_value"] - value) < 1e-12, (h32["pose_value"], value)
    e_ref = max(float(np.abs(a - b).max()) for a, b in zip(deg32, deg64))
    std = np.concatenate(deg64).std(axis=0)
    by_first = PS.score_host(deg64[0], deg64[1], I.first_number_labels())["pose_value"]
    by_position = PS.score_host(deg64[0], deg64[1], list(range(len(labels))))["pose_value"]
    print(f"  Pose_value fp32 {value:.6f}  fp64 {h64['pose_value']:.6f}  E_ref = max|deg_f32 - deg_f64| = {e_ref:.3e}")
    print(f"  distances {np.round(h64['distances'], 3).tolist()}")
    print(f"  per-angle std {np.round(std, 3).tolist()}  largest softmax value {pmax:.3f}")
    print(f"  Pose_value with first-number labels {by_first:.4f}, paired by position {by_position:.4f}")
    if std.min() < 0.1 or pmax > 0.9 or h64["pose_value"] < 0.2:
        raise SystemExit(f"gen_pose: degenerate fixture (per-angle std {std.tolist()}, softmax max {pmax}, Pose_value {h64['pose_value']}); change the seeds")
    assert abs(by_first - h64["pose_value"]) > 0.05 and abs(by_position - h64["pose_value"]) > 0.05, "the fixture must expose a wrong labelling and a wrong pairing"
    save("pose", keys=keys, shapes=shapes, labels=labels, prep=prep, prep_index=np.array(I.PREP_SAMPLES["tgt"]),
         deg_f32_tgt=deg32[0], deg_f32_res=deg32[1], deg_f64_tgt=deg64[0], deg_f64_res=deg64[1],
         dist_f32=h32["distances"], dist_f64=h64["distances"], pose_value_f32=np.float64(value), pose_value_f64=np.float64(h64["pose_value"]),
         e_ref=np.float64(e_ref), seed=PS.SEED)


def gen_expr():
    """The expression metric (eval_tool/Expression/expression_compare_face_recon.py over Deep3DFaceRecon's models/networks.py): the reference's
    own ReconNetWrapper('resnet50', use_last_fc=False), ParametricFaceModel.split_coeff (bfm.py; it does not touch ``self``), ImagePathDataset,
    compute_features, compute_features_wrapp and calculate_id_given_paths on the seeded PNG folders of tests/expr_inputs.py, with the seeded
    weights of reface_amd.exprscore.seeded_recon_state in place of the checkpoint file.  All three files are loaded by path.  What was stubbed,
    exactly: ``kornia.geometry.warp_affine`` (imported by networks.py, used by the recognition net only), ``util.load_mats.transferBFM09``
    (imported by bfm.py, used by the face model's constructor only), ``cv2`` and the torchvision transforms (imported by the script; its
    ImagePathDataset builds two Compose objects it never applies), tqdm / scipy when absent, ``options.test_options.TestOptions`` (the script
    parses it at import; nothing of it is read here) and ``models.create_model``: the real FaceReconModel needs BFM_model_front.mat,
    nvdiffrast and trimesh, so a stand-in takes its place whose ``forward`` is the real one's two lines (facerecon_model.py:136-147),
    ``split_coeff(net_recon(x))``, and whose ``setup`` loads ``torch.load(...)['net_recon']`` strictly as base_model.load_networks does
    (torch.load returns the seeded state).  Stored: the state-dict key layout of the reference module, the labels, all 257 coefficients of
    every image in fp32 (the reference as it runs) and from the same module and inputs in float64, the distances and Expression_value of
    both, e_ref = max |exp_f32 - exp_f64| over the 18 x 64 expression coefficients and e_ref_all, the same over all 257.  A degenerate
    fixture is refused, against the distance gate of the tests (64 x e_ref): every expression coefficient must vary by >= 100 x e_ref (std)
    over the images, Expression_value >= 100 gates, and labelling by the last number or pairing by position must each move Expression_value
    by more than 10 gates."""
    import importlib
    import importlib.util
    import tempfile
    import types
    sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))
    import expr_inputs as I
    from reface_amd import exprscore as ES

    for name in ("tqdm", "scipy"):
        try:
            importlib.import_module(name)
        except ImportError:
            m = ref_shims._mod(name)
            m.tqdm = lambda it, **k: it
            m.linalg = None
    _install_tv_transforms()
    ref_shims._mod("cv2")
    ref_shims._mod("kornia.geometry").warp_affine = None
    ref_shims._mod("util")
    ref_shims._mod("util.load_mats").transferBFM09 = None
    D3 = "/root/reference/eval_tool/Deep3DFaceRecon_pytorch_edit"

    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    N = by_path("ref_d3_networks", D3 + "/models/networks.py")
    BFM = by_path("ref_d3_bfm", D3 + "/models/bfm.py")
    split_coeff = BFM.ParametricFaceModel.split_coeff
    sd = ES.seeded_recon_state()

    class StandIn(torch.nn.Module):
        """FaceReconModel without the renderer and the face model: net_recon + split_coeff."""

        def __init__(self, opt):
            super().__init__()
            self.net_recon = N.define_net_recon(net_recon="resnet50", use_last_fc=False, init_path=None)
            self.facemodel = types.SimpleNamespace(to=lambda *a, **k: None)

        def setup(self, opt):
            self.net_recon.load_state_dict(torch.load("Other_dependencies/face_recon/epoch_latest.pth", map_location="cpu")["net_recon"])

        def forward(self, x):
            return split_coeff(None, self.net_recon(x))

    ref_shims._mod("eval_tool.Deep3DFaceRecon_pytorch_edit")
    ref_shims._mod("eval_tool.Deep3DFaceRecon_pytorch_edit.options")
    to = ref_shims._mod("eval_tool.Deep3DFaceRecon_pytorch_edit.options.test_options")
    to.TestOptions = lambda *a, **k: types.SimpleNamespace(parse=lambda: types.SimpleNamespace())
    ref_shims._mod("eval_tool.Deep3DFaceRecon_pytorch_edit.models").create_model = StandIn
    R = by_path("ref_expression_compare", "/root/reference/eval_tool/Expression/expression_compare_face_recon.py")

    net = N.define_net_recon(net_recon="resnet50", use_last_fc=False, init_path=None).eval()
    ref_sd = net.state_dict()
    keys = np.array(list(ref_sd.keys()))
    shapes = np.array([",".join(str(d) for d in v.shape) for v in ref_sd.values()])
    net.load_state_dict(sd, strict=True)
    net64 = N.define_net_recon(net_recon="resnet50", use_last_fc=False, init_path=None).eval()
    net64.load_state_dict(sd, strict=True)
    net64.double()

    data = I.build()
    labels = data["labels"]
    dev = torch.device("cpu")
    with tempfile.TemporaryDirectory() as tmp:
        paths = I.write_folders(tmp, data)
        load = torch.load
        torch.load = lambda *a, **k: {"net_recon": sd}          # the checkpoint path of the stand-in's setup
        try:
            value, sims = R.calculate_id_given_paths(paths, 50, dev, 2048, 0)
            model = StandIn(None)
            model.setup(None)
        finally:
            torch.load = load
        model.eval()
        _, ref_labels = R.compute_features_wrapp(paths[1], model, 50, 2048, dev, 0)
        assert list(ref_labels) == labels.tolist(), (ref_labels, labels)
        lists = [sorted(os.path.join(p, n) for n in os.listdir(p)) for p in paths]
        assert [os.path.basename(f) for f in lists[0]] == data["tgt_names"] and [os.path.basename(f) for f in lists[1]] == data["res_names"]
        x = [[R.ImagePathDataset(files)[i] for i in range(len(files))] for files in lists]          # [1, 3, 512, 512] each
    coef32 = [net(torch.cat(xs)).numpy() for xs in x]          # one batch per folder, as the script ran them (its batch of 50 becomes the folder)
    coef64 = [torch.cat([net64(t.double()) for t in xs]).numpy() for xs in x]
    assert coef32[0].shape == (10, 257) and coef32[0].dtype == np.float32 and coef64[0].dtype == np.float64

    h32 = ES.score_host(coef32[0], coef32[1], labels)
    h64 = ES.score_host(coef64[0], coef64[1], labels)
    assert abs(h32["expression_value"] - float(value)) <= 1e-12 * abs(float(value)) and np.abs(np.asarray(sims) - h32["distances"]).max() <= 1e-12, (h32["expression_value"], value)
    sl = slice(ES.EXP0, ES.EXP0 + ES.EXP_N)
    e_ref = max(float(np.abs(a[:, sl] - b[:, sl]).max()) for a, b in zip(coef32, coef64))
    e_ref_all = max(float(np.abs(a - b).max()) for a, b in zip(coef32, coef64))
    gate = 64.0 * e_ref
    std = np.concatenate(coef64)[:, sl].std(axis=0)
    by_last = ES.score_host(coef64[0], coef64[1], I.last_number_labels())["expression_value"]
    by_position = ES.score_host(coef64[0], coef64[1], list(range(len(labels))))["expression_value"]
    print(f"  Expression_value fp32 {h32['expression_value']:.6f}  fp64 {h64['expression_value']:.6f}  e_ref {e_ref:.3e}  e_ref_all {e_ref_all:.3e}  gate {gate:.3e}")
    print(f"  distances {np.round(h64['distances'], 4).tolist()}")
    print(f"  per-coefficient std min {std.min():.3e} max {std.max():.3e}; max |coef| {np.abs(np.concatenate(coef64)).max():.3f}")
    print(f"  Expression_value with last-number labels {by_last:.6f}, paired by position {by_position:.6f}")
    if std.min() < 100 * e_ref or h64["expression_value"] < 100 * gate:
        raise SystemExit(f"gen_expr: degenerate fixture (std min {std.min():.3e} vs 100 e_ref {100 * e_ref:.3e}; value {h64['expression_value']:.3e} vs 100 gates {100 * gate:.3e})")
    assert abs(by_last - h64["expression_value"]) > 10 * gate and abs(by_position - h64["expression_value"]) > 10 * gate, "the fixture must expose a wrong labelling and a wrong pairing"
    save("expr", keys=keys, shapes=shapes, labels=labels, coef_f32_tgt=coef32[0], coef_f32_res=coef32[1], coef_f64_tgt=coef64[0], coef_f64_res=coef64[1],
         dist_f32=h32["distances"], dist_f64=h64["distances"], expression_value_f32=np.float64(h32["expression_value"]),
         expression_value_f64=np.float64(h64["expression_value"]), e_ref=np.float64(e_ref), e_ref_all=np.float64(e_ref_all), seed=ES.SEED)


def _hf_fid_tower(cfg: P.CLIPVisionConfig, sd):
    """HF ``CLIPVisionModelWithProjection`` of ``cfg`` carrying the HF-named vision state ``sd`` (strict)."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = CLIPVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.intermediate, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                         patch_size=cfg.patch, image_size=cfg.image, projection_dim=cfg.proj, hidden_act="quick_gelu")
    m = CLIPVisionModelWithProjection(c).eval()
    have = m.state_dict()
    remap = {k: (k if k in have else k.replace("vision_model.", "vision_model.vision_model.", 1)) for k in sd}
    missing, unexpected = m.load_state_dict({remap[k]: v for k, v in sd.items()}, strict=False)
    assert not unexpected and not [k for k in missing if "position_ids" not in k], (missing[:5], unexpected[:5])
    return m


def gen_fid():
    """The FID (eval_tool/fid/fid_score.py over eval_tool/fid/inception.py): the reference's own InceptionV3.forward (which returns
    ``clip_model.encode_image``), ImagePathDataset, get_activations, calculate_activation_statistics and calculate_frechet_distance on the
    seeded PNG folders of tests/fid_inputs.py.  Both files are loaded by path.  What was stubbed, exactly: ``clip.load`` returns a stand-in
    whose ``encode_image`` is the ``image_embeds`` of an HF ``CLIPVisionModelWithProjection`` (the fixture tower of reface_amd.fidscore with
    its seeded weights) and the restated ``preprocess`` (torchvision's Resize(224, BICUBIC) / CenterCrop(224) / convert("RGB") / ToTensor /
    Normalize: the sizes and the crop offset written out, PIL and torch doing the arithmetic); ``torchvision.models``' inception_v3,
    InceptionA / C / E and load_state_dict_from_url (the reference still BUILDS an InceptionV3 it never runs: the stand-in has Identity
    layers and loads nothing); and get_activations' hard-coded feature width, ``np.empty((n, 512))``, which becomes the fixture tower's
    projection width through a numpy proxy on the loaded module.  Stored: three prepared tensors, both feature sets in fp32 and from the same
    module in float64 and in bfloat16, e_ref_feat = max |f32 - f64| and e_ref_feat_bf16, mu / sigma / FID of the reference's float64 path,
    fid_tol per precision (the largest |dFID| over 8 seeded uniform perturbations of the float64 features by +- 4 e_ref, doubled), and the
    features of a ViT-B/32-sized seeded tower on 4 images with their own e_ref.  A degenerate fixture is refused: both covariances must have
    full rank and the reference's sqrtm must come out finite and real without the eps retry."""
    import contextlib
    import importlib.util
    import io
    import tempfile
    from PIL import Image
    sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))
    import fid_inputs as I
    from reface_amd import fidscore as FS

    sd, cfg = FS.load_fid_clip_state("none")
    hf = _hf_fid_tower(cfg, sd)

    def preprocess(im):
        w, h = im.size
        nh, nw = FS.resized_size(h, w)
        if (nh, nw) != (h, w):
            im = im.resize((nw, nh), Image.BICUBIC)
        top, left = FS.crop_offset(nh), FS.crop_offset(nw)
        im = im.crop((left, top, left + 224, top + 224)).convert("RGB")
        t = torch.from_numpy(np.asarray(im, dtype=np.uint8).transpose(2, 0, 1).copy()).to(torch.float32).div(255)
        return sys.modules["torchvision.transforms.functional"].normalize(t, (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))

    class ClipStandIn(torch.nn.Module):
        def __init__(self, tower):
            super().__init__()
            self.tower = tower

        def encode_image(self, x):
            return self.tower(pixel_values=x).image_embeds

    sys.modules["clip"].load = lambda name, device=None, **k: (ClipStandIn(hf), preprocess)
    _install_tv_transforms()
    tv, tvm = sys.modules["torchvision"], sys.modules["torchvision.models"]
    tv.__version__ = "0.12.0"

    class _Block(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    class _NoInception:
        """torchvision's inception_v3 as the reference needs it to build: any layer is an Identity, no weights are loaded."""

        def __getattr__(self, name):
            return torch.nn.Identity()

        def load_state_dict(self, sd):
            return None

    tvi = ref_shims._mod("torchvision.models.inception")
    tvi.InceptionA = tvi.InceptionC = tvi.InceptionE = _Block
    tvm.inception, tvm.inception_v3 = tvi, (lambda *a, **k: _NoInception())
    ref_shims._mod("torchvision.models.utils").load_state_dict_from_url = lambda *a, **k: {}
    try:
        import tqdm  # noqa: F401
    except ImportError:
        pass          # fid_score.py has its own fallback

    def by_path(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    by_path("inception", "/root/reference/eval_tool/fid/inception.py")
    R = by_path("ref_fid_score", "/root/reference/eval_tool/fid/fid_score.py")

    class _NP:
        """numpy, with get_activations' hard-coded 512 feature columns replaced by the fixture tower's projection width."""

        def __getattr__(self, name):
            return getattr(np, name)

        def empty(self, shape, *a, **k):
            return np.empty((shape[0], cfg.proj) if tuple(shape[1:]) == (512,) else shape, *a, **k)

    R.np = _NP()
    data = I.build()
    dev = torch.device("cpu")
    model = R.InceptionV3([R.InceptionV3.BLOCK_INDEX_BY_DIM[2048]]).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        paths = I.write_folders(tmp, data)
        files = [FS.list_images(p) for p in paths]
        assert [[os.path.basename(f) for f in fl] for fl in files] == [data["dataset_names"], data["result_names"]]
        act = [R.get_activations([__import__("pathlib").Path(f) for f in fl], model, 50, 2048, dev, 0) for fl in files]
        stats = [R.calculate_activation_statistics([__import__("pathlib").Path(f) for f in fl], model, 50, 2048, dev, 0) for fl in files]
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            fid = R.calculate_fid_given_paths(paths, 50, dev, 2048, 0)
        x = [torch.cat([R.ImagePathDataset(fl)[i] for i in range(len(fl))]) for fl in files]          # [48, 3, 224, 224] each
    assert act[0].shape == (48, cfg.proj) and act[0].dtype == np.float64
    assert "singular" not in said.getvalue(), said.getvalue()
    with contextlib.redirect_stdout(said):
        assert float(R.calculate_frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])) == float(fid)
    from scipy import linalg
    root, _ = linalg.sqrtm(stats[0][1].dot(stats[1][1]), disp=False)
    imag = float(np.abs(root.imag).max()) if np.iscomplexobj(root) else 0.0
    conds = [float(np.linalg.cond(s)) for _, s in stats]
    print(f"  FID {float(fid):.6f}; cond(sigma) {conds[0]:.3e} {conds[1]:.3e}; sqrtm finite {bool(np.isfinite(root).all())}, max |imag| {imag:.2e}")
    assert np.isfinite(root).all() and imag == 0.0 and max(conds) < 1e6, "degenerate fixture"

    # the same module on the same prepared tensors, in fp32 (one batch per folder, as the script ran them), float64 and bfloat16
    f32 = [hf(pixel_values=t).image_embeds.numpy() for t in x]
    assert all(np.array_equal(a.astype(np.float32), b) for a, b in zip(act, f32)), "get_activations must equal the module's own fp32 output"
    hf.double()
    f64 = [hf(pixel_values=t.double()).image_embeds.numpy() for t in x]
    hf.bfloat16()
    fbf = [hf(pixel_values=t.bfloat16()).image_embeds.float().numpy() for t in x]
    e_ref = max(float(np.abs(a - b).max()) for a, b in zip(f32, f64))
    e_bf = max(float(np.abs(a - b).max()) for a, b in zip(fbf, f64))
    for (mu, sg), a in zip(stats, act):
        hm, hs = FS.stats_host(a)
        assert np.array_equal(hm, mu) and np.array_equal(hs, sg)
    assert abs(FS.frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1]) - float(fid)) <= 1e-12 * abs(float(fid))

    def fid_of(fa, fb):
        (m1, s1), (m2, s2) = FS.stats_host(fa), FS.stats_host(fb)
        return float(FS.frechet_distance(m1, s1, m2, s2))

    fid64 = fid_of(f64[0], f64[1])
    tol = {}
    for tag, e in (("f32", e_ref), ("bf16", e_bf)):
        worst = 0.0
        for k in range(8):
            rng = np.random.default_rng(4100 + k)
            worst = max(worst, abs(fid_of(f64[0] + rng.uniform(-4 * e, 4 * e, f64[0].shape), f64[1] + rng.uniform(-4 * e, 4 * e, f64[1].shape)) - fid64))
        tol[tag] = 2.0 * worst
    print(f"  e_ref_feat {e_ref:.3e}  e_ref_feat_bf16 {e_bf:.3e}  FID f64 {fid64:.6f}  fid_tol f32 {tol['f32']:.3e} bf16 {tol['bf16']:.3e}; max |feature| {np.abs(f64[0]).max():.3f}")

    # ViT-B/32's own dimensions, seeded, on 4 images
    big_cfg = P.CLIPVisionConfig(**FS.VIT_B32)
    big_sd = FS.seeded_fid_state(big_cfg)
    big = _hf_fid_tower(big_cfg, big_sd)
    xb = x[0][list(I.B32_IMAGES)]
    b32 = big(pixel_values=xb).image_embeds.numpy()
    big.double()
    b64 = big(pixel_values=xb.double()).image_embeds.numpy()
    e_b32 = float(np.abs(b32 - b64).max())
    print(f"  ViT-B/32-sized tower: e_ref {e_b32:.3e}, max |feature| {np.abs(b64).max():.3f}")
    prep = np.stack([x[0][i].numpy() for i in I.PREP_SAMPLES])
    save("fid", prep=prep, prep_index=np.array(I.PREP_SAMPLES), feat_f32_dataset=f32[0], feat_f32_results=f32[1], feat_f64_dataset=f64[0], feat_f64_results=f64[1],
         e_ref_feat=np.float64(e_ref), e_ref_feat_bf16=np.float64(e_bf), mu_dataset=stats[0][0], sigma_dataset=stats[0][1], mu_results=stats[1][0],
         sigma_results=stats[1][1], fid=np.float64(fid), fid_f64=np.float64(fid64), fid_tol_f32=np.float64(tol["f32"]), fid_tol_bf16=np.float64(tol["bf16"]),
         b32_index=np.array(I.B32_IMAGES), b32_feat_f32=b32, b32_feat_f64=b64, b32_e_ref=np.float64(e_b32), seed=FS.SEED)


def _tv_feature_stacks():
    """torchvision's ``alexnet().features`` and ``vgg16().features`` restated (torchvision is absent here, see README): the module
    sequences of torchvision/models/alexnet.py and vgg.py (configuration "D", no batch norm), hence torchvision's state-dict indices.
    Returned as the two constructors the reference calls (``models.alexnet(True)``, ``models.vgg16(True)``): the ``pretrained`` flag is
    ignored -- nothing is downloaded, the weights are loaded afterwards."""
    nn = torch.nn

    class _Net(nn.Module):
        def __init__(self, features):
            super().__init__()
            self.features = features

    def alexnet(pretrained=False, **kw):
        return _Net(nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2)))

    def vgg16(pretrained=False, **kw):
        layers, cin = [], 3
        for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"):
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        return _Net(nn.Sequential(*layers))

    return alexnet, vgg16


def gen_lpips():
    """The perceptual distance (eval_tool/lpips/{lpips,networks,utils}.py): the reference's own LPIPS module -- BaseNet.forward,
    normalize_activation, LinLayers and LPIPS.forward -- on the seeded pairs of tests/lpips_inputs.py, for 'alex' and 'vgg'.  The three files
    are loaded by path (``eval_tool`` is a stub in ref_shims and a package of this repository; neither is the reference's).  What this
    container lacks is restated: torchvision's two feature stacks (_tv_feature_stacks, on the stub ``torchvision.models``); the two
    downloads are replaced: ``get_state_dict`` returns the seeded linear weights, and the whole module is then loaded strictly with
    reface_amd.lpips.load_lpips_state("none", net).  Inputs are ToTensor + Normalize(0.5, 0.5) of the bytes, as the reference's datasets
    prepare images.  Stored (tests/golden/lpips.npz): per case v[b, l], d[b] and the module's scalar from the module in fp32 (the reference as
    it runs) and from the same module and inputs in float64; the normalised tap features of one 'alex' pair (float64); the folder case's
    labels, v and d; e_ref = the largest relative |fp32 - fp64| over the v[b, l] of the ordinary pairs, e_ref_near the same over the
    near-identical pairs.  tests/golden/lpips_keys.json holds the module's state-dict keys and shapes, in order, for both nets.  A degenerate
    fixture is refused: every ordinary v[b, l] must exceed 1e-6, every near-identical d must be positive and below a tenth of the smallest
    ordinary d of its case, and pairing the folder's results by position must move its value by more than 1 %."""
    import importlib.util
    import json
    sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))
    import lpips_inputs as I
    from reface_amd import lpips as LP

    tvm = sys.modules["torchvision.models"]
    tvm.alexnet, tvm.vgg16 = _tv_feature_stacks()
    names = ["eval_tool.lpips.utils", "eval_tool.lpips.networks", "eval_tool.lpips.lpips"]
    saved = {n: sys.modules.get(n) for n in names}
    current = {}

    def load(name):
        spec = importlib.util.spec_from_file_location(name, "/root/reference/eval_tool/lpips/%s.py" % name.rsplit(".", 1)[1])
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    try:
        U = load(names[0])
        U.get_state_dict = lambda net_type="alex", version="0.1": {f"{l}.1.weight": current["sd"][f"lin.{l}.1.weight"] for l in range(LP.N_TAPS)}
        load(names[1])
        R = load(names[2])          # binds U.get_state_dict as patched above

        def module(net, dtype):
            current["sd"] = LP.load_lpips_state("none", net)
            m = R.LPIPS(net_type=net).eval()
            m.load_state_dict(current["sd"], strict=True)
            return m.to(dtype)

        def run(m, x, y):
            """v [B, L] and the scalar, by the lines of LPIPS.forward (lpips.py:30-35)."""
            x, y = x.to(next(m.parameters()).dtype), y.to(next(m.parameters()).dtype)
            feat_x, feat_y = m.net(x), m.net(y)
            diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
            res = [l(d).mean((2, 3), True) for d, l in zip(diff, m.lin)]
            v = torch.cat(res, 1)[:, :, 0, 0]
            scalar = m(x, y)
            assert scalar.dim() == 0 and abs(float(scalar) - float(torch.sum(torch.cat(res, 0)) / x.shape[0])) == 0.0
            return v.double().numpy(), float(scalar), feat_x, feat_y

        keys, mods = {}, {}
        for net in ("alex", "vgg"):
            mods[net] = (module(net, torch.float32), module(net, torch.float64))
            ref_sd = mods[net][0].state_dict()
            keys[net] = [[k, list(v.shape)] for k, v in ref_sd.items()]
            assert [k for k, _ in keys[net]] == list(P.lpips_param_specs(net)), "key order"
        assert len(keys["alex"]) == 17 and len(keys["vgg"]) == 33, (len(keys["alex"]), len(keys["vgg"]))

        def tensors(images):
            return torch.from_numpy(np.stack([LP.prep_host(im) for im in images]))

        out, e_ref, e_near = {}, 0.0, 0.0
        for c, (net, h, w) in enumerate(I.CASES):
            xs, ys = I.build_case(c)
            x, y = tensors(xs), tensors(ys)
            v32, s32, _, _ = run(mods[net][0], x, y)
            v64, s64, fx64, fy64 = run(mods[net][1], x, y)
            rel = np.abs(v32 - v64) / v64
            ordinary = [k for k in range(I.PAIRS) if k != I.NEAR]
            e_ref, e_near = max(e_ref, float(rel[ordinary].max())), max(e_near, float(rel[I.NEAR].max()))
            d64 = LP.score_host(v64)["distances"]
            print(f"  {I.case_name(c)}: scalar fp32 {s32:.8f} fp64 {s64:.8f}  d {np.array2string(d64, precision=6)}  "
                  f"rel |fp32 - fp64|: ordinary {rel[ordinary].max():.2e}, near {rel[I.NEAR].max():.2e}")
            if v64[ordinary].min() <= 1e-6 or not 0.0 < d64[I.NEAR] < 0.1 * d64[ordinary].min():
                raise SystemExit(f"gen_lpips: degenerate fixture in {I.case_name(c)}: v {v64.tolist()}; change the seeds")
            assert abs(LP.score_host(v64)["lpips_value"] - s64) <= 1e-12 * s64
            n = I.case_name(c)
            out.update({f"v_f32_{n}": v32, f"v_f64_{n}": v64, f"d_f32_{n}": LP.score_host(v32)["distances"], f"d_f64_{n}": d64,
                        f"scalar_f32_{n}": np.float64(s32), f"scalar_f64_{n}": np.float64(s64)})
            if c == I.FEATURE_CASE:
                for l in range(LP.N_TAPS):
                    out[f"nfeat_x_{l}"] = fx64[l][I.FEATURE_PAIR].numpy()
                    out[f"nfeat_y_{l}"] = fy64[l][I.FEATURE_PAIR].numpy()

        # the folder layout: a result is paired with the target at the position its label names; equal sizes run together
        data = I.build_folders()
        labels = data["labels"]
        fv32, fv64, fpos = [], [], []
        for i, l in enumerate(labels):
            y = tensors([data["res_images"][i]])
            x = tensors([data["tgt_images"][int(l)]])
            fv32.append(run(mods[I.FOLDER_NET][0], x, y)[0][0])
            fv64.append(run(mods[I.FOLDER_NET][1], x, y)[0][0])
            fpos.append(run(mods[I.FOLDER_NET][1], tensors([data["tgt_images"][i]]), y)[0][0])          # (the sizes agree by position too)
        fv32, fv64 = np.stack(fv32), np.stack(fv64)
        folder = LP.score_host(fv64)
        by_position = LP.score_host(np.stack(fpos))["lpips_value"]
        print(f"  folders paired by position: {by_position:.8f}")
        assert abs(by_position - folder["lpips_value"]) > 0.01 * folder["lpips_value"], "the fixture must expose a wrong pairing"
        e_ref = max(e_ref, float((np.abs(fv32 - fv64) / fv64).max()))
        print(f"  folders: LPIPS_value {folder['lpips_value']:.8f}  d {np.array2string(folder['distances'], precision=6)}")
        print(f"  e_ref {e_ref:.3e}  e_ref_near {e_near:.3e}")
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    path = os.path.join(OUT, "lpips_keys.json")
    json.dump(keys, open(path, "w"), separators=(",", ":"))
    print(f"  wrote {path}  ({os.path.getsize(path)/1024:.1f} KiB)")
    save("lpips", labels=labels, folder_v_f32=fv32, folder_v_f64=fv64, folder_d_f64=folder["distances"], folder_value_f64=np.float64(folder["lpips_value"]),
         folder_value_f32=np.float64(LP.score_host(fv32)["lpips_value"]), e_ref=np.float64(e_ref), e_ref_near=np.float64(e_near), seed=LP.SEED, **out)


def gen_gemm_plans(recorded_from="unknown"):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import gemm_plan_sweep
    from reface_amd import _lib
    n, nmsg, size = gemm_plan_sweep.record(recorded_from)
    print(f"  wrote {gemm_plan_sweep.GOLDEN}: {n} descriptors, {nmsg} distinct rejections, {size / 1024:.1f} KiB, asked of {_lib.LIB_PATH} ({recorded_from})")


GROUPS = dict(ddim_full=gen_ddim_full, unet_keys=gen_unet_keys, plms=gen_plms, schedule=gen_schedule, unet_ops=gen_unet_ops, unet_small=gen_unet_small, unet_full=gen_unet_full,
              ddim=gen_ddim, vae=gen_vae, arcface=gen_arcface, clip=gen_clip, e2e=gen_e2e,
              bisenet=gen_bisenet, align=gen_align, align_pad=gen_align_pad, idscore=gen_idscore, pose=gen_pose, expr=gen_expr, fid=gen_fid, lpips=gen_lpips)

if __name__ == "__main__":
    if sys.argv[1:2] == ["gemm_plans"]:          # (by name only, with the commit whose library is loaded: see the module's help text)
        print("[gemm_plans]")
        gen_gemm_plans(*sys.argv[2:3])
        sys.exit(0)
    sel = sys.argv[1:] or [g for g in GROUPS if g != "ddim_full"]          # (ddim_full: 20 minutes; ask for it by name)
    for g in sel:
        print(f"[{g}]")
        t0 = time.time()
        GROUPS[g]()
        print(f"  {time.time()-t0:.1f}s")
