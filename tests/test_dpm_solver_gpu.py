"""DPM-Solver++ multistep sampler on the GPU: the fused update kernel against fp64, order 1 on DDIM's grid against the DDIM sampler, orders
2 and 3 against the fp64 reference sampler (tests/dpm_refs.py) around the CPU oracle UNet, the three launch modes, and the CLI flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dpm_refs as R
from reface_amd import ops, params as P
from reface_amd.dpm_solver import DPMSolverSampler, dpm_coefficients, dpm_nodes
from reface_amd.schedule import ddpm_buffers
from test_pipeline_gpu import SMALL_UNET, _LDMStub, _ddim_inputs, make_unet, maxerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACP = ddpm_buffers(1000, 0.00085, 0.0120)["alphas_cumprod"].double().numpy()
SCALE = 3.5


@pytest.fixture(scope="module")
def unet():
    return make_unet(SMALL_UNET, 7)


def _kw(cfg=True, **extra):
    x_T, z_inp, mask, c, uc = _ddim_inputs()
    kw = dict(conditioning=c.to(DEV), batch_size=2, shape=[4, 16, 16], verbose=False, eta=0.0, x_T=x_T.to(DEV),
              test_model_kwargs={"inpaint_image": z_inp.to(DEV), "inpaint_mask": mask.to(DEV)})
    if cfg:
        kw.update(unconditional_guidance_scale=SCALE, unconditional_conditioning=uc.to(DEV))
    kw.update(extra)
    return kw


# ------------------------------------------------------------------------------------------------ 6. the kernel against fp64
# rows of a real third-order run (quad, S = 6): steps 0, 1, 2 read 0, 1, 2 history terms; step 0 sits at t = 999 (alpha = 0.07: the
# largest data predictions), and one synthetic row with every weight of order one
_ROWS = torch.from_numpy(np.concatenate([dpm_coefficients(ACP, dpm_nodes(ACP, 6, "quad"), 3)[:3],
                                         np.asarray([[0.8, 0.6, 0.9, -1.3, 1.7, -0.6, 2, 0]], dtype=np.float32)]))


@pytest.mark.parametrize("B,hw", [(2, 256), (1, 35)])          # more than one block / a grid tail that is no multiple of any vector width
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("ld", [4, 8])
def test_dpm_update_kernel(B, hw, cfg, ld):
    seed = 0
    for row in _ROWS:
        n_hist = int(row[6])
        for with_m2 in ([False, True] if n_hist < 2 else [True]):
            seed += 1
            i = R.update_inputs(B, hw, ld, cfg, 1000 * hw + 100 * ld + 10 * cfg + seed)
            dev = lambda t: t.reshape(B, 4, hw, 1).to(DEV).contiguous()
            eps, img, m1 = i["eps"].to(DEV), dev(i["img"]), dev(i["m1"])
            m2 = dev(i["m2"]) if with_m2 else None
            ops.dpm_update(eps, img, m1, m2, row.to(DEV), cfg=cfg, scale=SCALE)()
            torch.cuda.synchronize()
            xp, m0, lim_x, lim_m = R.update_ref(i["eps"], i["img"], i["m1"], i["m2"], row, cfg, SCALE)
            got_x, got_m = img.cpu().reshape(B, 4, hw).double(), m1.cpu().reshape(B, 4, hw).double()
            ex, em = (got_x - xp).abs(), (got_m - m0).abs()
            assert (ex <= lim_x).all(), (n_hist, with_m2, float((ex / lim_x).max()))
            assert (em <= lim_m).all(), (n_hist, with_m2, float((em / lim_m).max()))
            if with_m2:
                assert torch.equal(m2.cpu().reshape(B, 4, hw), i["m1"])          # the shift is an exact copy
            assert torch.equal(eps.cpu(), i["eps"])


@pytest.mark.parametrize("with_m2", [False, True])
def test_dpm_update_first_step_ignores_history(with_m2):
    """The history buffers of a first step hold whatever was there: an n_hist = 0 row must not read them into the sum (0 * NaN is NaN)."""
    B, hw, row = 1, 35, _ROWS[0]
    assert int(row[6]) == 0
    i = R.update_inputs(B, hw, 8, True, 77)
    dev = lambda t: t.reshape(B, 4, hw, 1).to(DEV).contiguous()
    nan = torch.full((B, 4, hw), float("nan"))
    img, m1, m2 = dev(i["img"]), dev(nan), (dev(nan) if with_m2 else None)
    ops.dpm_update(i["eps"].to(DEV), img, m1, m2, row.to(DEV), cfg=True, scale=SCALE)()
    torch.cuda.synchronize()
    xp, m0, lim_x, lim_m = R.update_ref(i["eps"], i["img"], nan, nan, row, True, SCALE)
    got_x, got_m = img.cpu().reshape(B, 4, hw).double(), m1.cpu().reshape(B, 4, hw).double()
    assert torch.isfinite(got_x).all() and torch.isfinite(got_m).all()
    assert ((got_x - xp).abs() <= lim_x).all() and ((got_m - m0).abs() <= lim_m).all()


# ------------------------------------------------------------------------------------------------ 7. order 1 / uniform is the DDIM sampler
@pytest.mark.parametrize("S,graph,tol", [(5, True, 2e-4), (5, "per_step", 2e-4), (5, False, 2e-4), (50, True, 1e-3)])
def test_order1_uniform_reproduces_ddim_sampler(unet, S, graph, tol, monkeypatch):
    from reface_amd.ddim import DDIMSampler
    if graph == "per_step":
        monkeypatch.setenv("REFACE_GRAPH_STEPS", "1")
    want, winter = DDIMSampler(_LDMStub(unet), use_graph=bool(graph)).sample(S=S, **_kw())
    got, ginter = DPMSolverSampler(_LDMStub(unet), order=1, spacing="uniform", use_graph=bool(graph)).sample(S=S, **_kw())
    d, dp = maxerr(got, want.cpu()), maxerr(ginter["pred_x0"][-1], winter["pred_x0"][-1].cpu())
    print(f"order 1 / uniform vs DDIMSampler, S = {S}, graph = {graph}: max |d| = {d:.2e} (pred_x0 {dp:.2e})")
    assert d < tol and dp < tol, (d, dp)
    assert len(ginter["x_inter"]) == len(winter["x_inter"]) and len(ginter["pred_x0"]) == len(winter["pred_x0"])


# ------------------------------------------------------------------------------------------------ 8. orders 2 and 3 against the fp64 reference sampler
@pytest.mark.parametrize("order,spacing,S,cfg", [(2, "logsnr", 5, True), (3, "quad", 6, False)])
def test_orders_2_3_match_fp64_reference_sampler(unet, order, spacing, S, cfg):
    """Reference: tests/dpm_refs.py::sample (fp64 solver in the D1 / D2 form) around oracle.unet.unet_forward.  Limit: max(3e-4, 2 d), 3e-4 being
    the PLMS parity tolerance and d the distance of the existing DDIMSampler to oracle.ddim.sample at the same S on the same inputs.
    Measured on an MI355X: order 2 / logsnr / S = 5 / CFG 1.63e-4 with d = 5.7e-5; order 3 / quad / S = 6 / no CFG 4.7e-5 with d = 4.2e-5."""
    from oracle import ddim as oddim, unet as ounet
    from reface_amd.ddim import DDIMSampler
    ucfg = P.UNetConfig(**SMALL_UNET)
    sd = P.seeded_state_dict(P.unet_param_specs(ucfg), 7)
    plan = ounet.plan_of(sd, ucfg.num_heads)
    eps_fn = lambda x, t, cc: ounet.unet_forward(sd, plan, x, t, cc, 64)
    x_T, z_inp, mask, c, uc = _ddim_inputs()
    uc, scale = (uc, SCALE) if cfg else (None, 1.0)
    with torch.no_grad():
        ddim_ref, _ = oddim.sample(eps_fn, S, x_T, c, uc, z_inp, mask, scale)
        nodes = dpm_nodes(ACP, S, spacing)
        ref, hist = R.sample(eps_fn, ACP, nodes, order, x_T, c, uc, z_inp, mask, scale)
    ddim_got, _ = DDIMSampler(_LDMStub(unet)).sample(S=S, **_kw(cfg))
    d = maxerr(ddim_got, ddim_ref)
    sampler = DPMSolverSampler(_LDMStub(unet), order=order, spacing=spacing)
    got, inter = sampler.sample(S=S, **_kw(cfg))
    assert list(sampler.dpm_nodes) == list(nodes)
    assert [int(v) + 1 for v in sampler.dpm_coefs[:, 6]] == [R.order_used(order, i, S) for i in range(S)]
    e, ep = maxerr(got, ref), maxerr(inter["pred_x0"][-1], hist[-1])
    lim = max(3e-4, 2 * d)
    print(f"order {order} / {spacing}, S = {S}, cfg = {cfg}: max |d| to the fp64 reference sampler = {e:.2e} (last pred_x0 {ep:.2e}); "
          f"DDIMSampler to oracle.ddim.sample at S = {S}: d = {d:.2e}; limit {lim:.2e}")
    assert e <= lim and ep <= lim, (e, ep, lim)
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 3 and torch.equal(inter["x_inter"][-1], got)      # x_T, first step, last step


# ------------------------------------------------------------------------------------------------ 9. the three launch modes
@pytest.mark.parametrize("order,spacing,S,log_every_t", [(2, "logsnr", 5, 100), (3, "quad", 6, 2)])
def test_launch_modes_are_bit_identical(unet, order, spacing, S, log_every_t, monkeypatch):
    runs = {}
    for mode in ("graph", "per_step", "eager"):
        if mode == "per_step":
            monkeypatch.setenv("REFACE_GRAPH_STEPS", "1")
        else:
            monkeypatch.delenv("REFACE_GRAPH_STEPS", raising=False)
        sampler = DPMSolverSampler(_LDMStub(unet), order=order, spacing=spacing, use_graph=mode != "eager")
        runs[mode] = sampler.sample(S=S, log_every_t=log_every_t, **_kw())
        again, _ = sampler.sample(S=S, log_every_t=log_every_t, **_kw())          # the cached graph, history buffers as the last run left them
        assert torch.equal(runs[mode][0], again), mode
    base, binter = runs["graph"]
    assert torch.isfinite(base).all()
    n_inter = 1 + len([i for i in range(S) if (S - i - 1) % log_every_t == 0 or i == 0])
    for mode in ("per_step", "eager"):
        got, inter = runs[mode]
        assert torch.equal(got, base), mode
        for k in ("x_inter", "pred_x0"):
            assert len(inter[k]) == len(binter[k]) == n_inter, (mode, k, len(inter[k]), n_inter)
            assert all(torch.equal(a, b) for a, b in zip(inter[k], binter[k])), (mode, k)


def test_x_T_is_one_draw(unet):
    """Not an algorithm of the reference: no generator state to mirror, so x_T = None costs exactly one torch.randn."""
    sampler = DPMSolverSampler(_LDMStub(unet))
    kw = _kw()
    kw.pop("x_T")
    torch.manual_seed(1234)
    got, _ = sampler.sample(S=5, x_T=None, **kw)
    after = torch.randn((2, 4, 16, 16), device=DEV)
    torch.manual_seed(1234)
    x_T = torch.randn((2, 4, 16, 16), device=DEV)
    expect_after = torch.randn((2, 4, 16, 16), device=DEV)
    assert torch.equal(after, expect_after)
    ref, _ = sampler.sample(S=5, x_T=x_T, **kw)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ 10. CLI
def test_cli_dpm_solver(tmp_path):
    from PIL import Image
    from test_e2e_gpu import SMALL_CLIP
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "inference_test_bench.py"), "--outdir", str(out), "--config",
           os.path.join(ROOT, "tests", "configs", "reface_small.yaml"), "--ckpt", "none", "--dataset", "synthetic", "--n_items", "2",
           "--n_samples", "2", "--ddim_steps", "5", "--scale", "3.5", "--H", "256", "--W", "256", "--dpm_solver", "--precision", "bf16",
           "--clip_vision_config", json.dumps(SMALL_CLIP)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "dpm_solver=True" in r.stdout
    assert sorted(os.listdir(out / "results")) == ["000000000000.png", "000000000001.png"]
    for f in sorted(os.listdir(out / "results")):
        im = np.asarray(Image.open(out / "results" / f)).astype(np.float64)
        assert im.shape == (256, 256, 3) and np.isfinite(im).all() and im.std() > 1.0, (f, im.std())
