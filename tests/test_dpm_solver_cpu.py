"""DPM-Solver++ multistep sampler, host side (no GPU): the coefficient table against the stepwise fp64 reference (tests/dpm_refs.py), order 1
on DDIM's grid against the DDIM step, the timestep grids, convergence on an analytic model with a closed solution, and the refusals / surface."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import dpm_refs as R
from reface_amd import _lib
from reface_amd.dpm_solver import DPMSolverSampler, dpm_coefficients, dpm_nodes
from reface_amd.schedule import ddim_step_coefficients, ddpm_buffers, make_ddim_sampling_parameters, make_ddim_timesteps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF = ddpm_buffers(1000, 0.00085, 0.0120)
ACP32 = BUF["alphas_cumprod"]                        # what the model hands the sampler (fp32)
ACP = ACP32.double().numpy()
SPACINGS = ("logsnr", "quad", "uniform")


def _stub():
    return types.SimpleNamespace(num_timesteps=1000, betas=BUF["betas"], alphas_cumprod=ACP32, alphas_cumprod_prev=BUF["alphas_cumprod_prev"],
                                 device=torch.device("cpu"), model=None)


# ------------------------------------------------------------------------------------------------ 1. table vs stepwise reference
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("spacing", SPACINGS)
def test_table_matches_stepwise_reference(order, spacing):
    g = np.random.default_rng(100 * order + SPACINGS.index(spacing))
    for S in (5, 6, 10, 20):
        nodes = dpm_nodes(ACP, S, spacing)
        n = len(nodes) - 1
        eps, x_T = g.standard_normal((n, 257)), g.standard_normal(257)
        _, want, _ = R.run(ACP, nodes, order, lambda x, i, t: eps[i], x_T)
        rows = dpm_coefficients(ACP, nodes, order, dtype=np.float64)
        got = R.table_run(rows, eps, x_T)
        assert rows.shape == (n, 8) and len(got) == n
        for i in range(n):
            rel = np.abs(got[i] - want[i]).max() / np.abs(want[i]).max()
            assert rel <= 1e-12, (S, i, rel)
        assert list(rows[:, 6]) == [R.order_used(order, i, n) - 1 for i in range(n)] and not rows[:, 7].any()
        # an unused history term has no weight either, and the shipped rows are ONE rounding of the fp64 ones
        assert all(rows[i, 4 + k] == 0 for i in range(n) for k in range(2) if k >= rows[i, 6])
        r32 = dpm_coefficients(ACP, nodes, order)
        assert r32.dtype == np.float32 and np.array_equal(r32, rows.astype(np.float32))


def test_order_sequence_of_a_third_order_run():
    rows = dpm_coefficients(ACP, dpm_nodes(ACP, 6, "quad"), 3)
    assert [int(v) + 1 for v in rows[:, 6]] == [1, 2, 3, 3, 2, 1]


# ------------------------------------------------------------------------------------------------ 2. order 1 on `uniform` is DDIM
@pytest.mark.parametrize("S", [5, 50])
def test_order1_uniform_is_ddim(S):
    ts = make_ddim_timesteps("uniform", S, 1000, verbose=False)
    sig, a, a_prev = make_ddim_sampling_parameters(ACP32, ts, 0.0, verbose=False)
    ddim = torch.flip(ddim_step_coefficients(a, a_prev, sig), dims=[0]).double().numpy()          # row i <-> step i, fp32 values
    nodes = dpm_nodes(ACP, S, "uniform")
    rows = dpm_coefficients(ACP, nodes, 1).astype(np.float64)                                     # fp32 values
    assert len(rows) == len(ddim) == S
    g = np.random.default_rng(S)
    for i in range(S):
        x, e = g.standard_normal(4096), g.standard_normal(4096)
        px0 = (x - ddim[i, 1] * e) / ddim[i, 0]
        want = ddim[i, 2] * px0 + ddim[i, 3] * e
        m0 = (x - rows[i, 1] * e) / rows[i, 0]
        got = rows[i, 2] * x + rows[i, 3] * m0
        assert np.abs(got - want).max() / np.abs(want).max() <= 1e-6, (i, np.abs(got - want).max() / np.abs(want).max())
        assert np.abs(m0 - px0).max() / np.abs(px0).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ 3. grids
def test_grids():
    assert list(dpm_nodes(ACP, 10, "logsnr")) == [999, 888, 757, 597, 413, 233, 103, 36, 11, 2, 0]
    for spacing in ("logsnr", "quad"):
        for S in range(1, 101):
            t = dpm_nodes(ACP, S, spacing)
            assert len(t) == S + 1 and t[0] == 999 and t[-1] == 0 and (np.diff(t) < 0).all(), (spacing, S, t)
    for S in (5, 20, 50):
        t = dpm_nodes(ACP, S, "uniform")
        assert list(t[:-1]) == list(np.flip(make_ddim_timesteps("uniform", S, 1000, verbose=False))) and t[-1] == 0
    for spacing in ("logsnr", "quad"):
        rows = dpm_coefficients(ACP, dpm_nodes(ACP, 1, spacing), 3)
        assert rows.shape == (1, 8) and rows[0, 6] == 0 and rows[0, 4] == 0 and rows[0, 5] == 0          # S = 1: one first-order step, 999 -> 0
    with pytest.raises(ValueError):
        dpm_nodes(ACP, 1000, "quad")                          # 1001 nodes do not fit into 1000 timesteps
    s = DPMSolverSampler(_stub(), order=2, spacing="logsnr")
    s.make_schedule(10, verbose=False)
    assert list(s.dpm_nodes) == [999, 888, 757, 597, 413, 233, 103, 36, 11, 2, 0] and tuple(s.dpm_coefs.shape) == (10, 8)
    assert s.dpm_coefs.dtype == torch.float32
    # the refusal of other DDIM discretisations stays where it was
    with pytest.raises(NotImplementedError):
        make_ddim_timesteps("quad", 10, 1000, verbose=False)


# ------------------------------------------------------------------------------------------------ 4. convergence on the analytic model
@pytest.mark.parametrize("s_lo", [0.2, 0.5])
def test_convergence_on_gaussian_model(s_lo):
    """Per-element Gaussian data (tests/dpm_refs.py::GaussianModel): exact eps, exact probability-flow solution."""
    M = R.GaussianModel(ACP, n=4096, s_lo=s_lo, seed=0)
    err = lambda S, order, spacing: M.rms_error(dpm_nodes(ACP, S, spacing), order)
    ddim50 = err(50, 1, "uniform")
    o2_20, o2_40 = err(20, 2, "logsnr"), err(40, 2, "logsnr")
    o1_20, o1_40 = err(20, 1, "logsnr"), err(40, 1, "logsnr")
    print(f"s ~ U({s_lo}, 1): order 1 / uniform S = 50 {ddim50:.3e}; logsnr order 2 S = 20 / 40 {o2_20:.3e} / {o2_40:.3e}; "
          f"order 1 S = 20 / 40 {o1_20:.3e} / {o1_40:.3e}")
    assert o2_20 < ddim50 / 4, (o2_20, ddim50)                 # (a)
    assert o2_20 >= 3 * o2_40, (o2_20, o2_40)                  # (b) second order: halving h quarters the error
    assert 1.5 <= o1_20 / o1_40 <= 2.5, (o1_20, o1_40)         # (c) first order halves it: the test tells the orders apart
    # the same figures through the shipped table (fp32 rows): what the GPU path computes
    x = R.table_run(dpm_coefficients(ACP, dpm_nodes(ACP, 20, "logsnr"), 2), lambda x, i: M.eps(x, int(dpm_nodes(ACP, 20, "logsnr")[i])), M.x_start(999))[-1]
    tab = float(np.sqrt(np.mean((x - M.exact(999, 0)) ** 2)))
    assert abs(tab - o2_20) <= 1e-3 * o2_20, (tab, o2_20)


# ------------------------------------------------------------------------------------------------ 5. refusals and surface
def test_refusals():
    kw = dict(S=5, batch_size=1, shape=[4, 8, 8], conditioning=torch.zeros(1, 1, 768), verbose=False)
    with pytest.raises(ValueError, match=r"ddim_eta must be 0 for DPM-Solver\+\+"):
        DPMSolverSampler(_stub()).sample(eta=0.5, **kw)
    with pytest.raises(ValueError, match="order"):
        DPMSolverSampler(_stub(), order=4)
    with pytest.raises(ValueError, match="order"):
        dpm_coefficients(ACP, dpm_nodes(ACP, 5), 4)
    with pytest.raises(ValueError, match="spacing"):
        DPMSolverSampler(_stub(), spacing="karras")
    with pytest.raises(ValueError, match="spacing"):
        dpm_nodes(ACP, 5, "karras")
    # the parent's contract still holds behind the new step rule
    with pytest.raises(Exception, match="kwargs must contain either 'test_model_kwargs' or 'rest' key"):
        DPMSolverSampler(_stub()).sample(**kw)


@pytest.mark.parametrize("script", ["inference_test_bench", "inference_swap_selected", "inference_swap_video", "one_inference"])
def test_cli_flags(script, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    cli = importlib.import_module(script)
    p = cli.build_parser()
    flags = {a.option_strings[0] for a in p._actions if a.option_strings}
    assert {"--dpm_solver", "--dpm_order", "--dpm_spacing", "--plms"} <= flags
    d = p.parse_args([])
    assert (d.dpm_solver, d.dpm_order, d.dpm_spacing, d.plms, d.ddim_steps) == (False, 2, "logsnr", False, 50)          # no default changes
    o = p.parse_args(["--dpm_solver", "--dpm_order", "3", "--dpm_spacing", "quad", "--ddim_steps", "20"])
    assert (o.dpm_solver, o.dpm_order, o.dpm_spacing, o.ddim_steps) == (True, 3, "quad", 20)
    for bad in (["--dpm_solver", "--plms"], ["--dpm_order", "4"], ["--dpm_spacing", "karras"]):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(bad)
    capsys.readouterr()


def test_dotted_path_and_exports():
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler as A
    from ldm.models.diffusion.dpm_solver.sampler import DPMSolverSampler as B
    from reface_amd.ddim import DDIMSampler
    assert A is B is DPMSolverSampler and issubclass(A, DDIMSampler)
    assert "rf_dpm_update" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "reface_hip.h")).read()
    assert "int rf_dpm_update(const float* eps, int ld_eps, int cfg, float scale, float* img, float* m1, float* m2, int B, int hw," in hdr
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.rf_version() >= 106 and hasattr(lib, "rf_dpm_update")
        # argument checks (host side, nothing is launched): null pointers, bad sizes, aliased buffers
        one = 4096
        assert lib.rf_dpm_update(None, 4, 0, 1.0, one, one * 2, None, 1, 16, one * 3, None) != 0
        assert b"rf_dpm_update" in lib.rf_last_error()
        assert lib.rf_dpm_update(one, 3, 0, 1.0, one * 2, one * 3, None, 1, 16, one * 4, None) != 0
        assert lib.rf_dpm_update(one, 4, 0, 1.0, one * 2, one * 2, None, 1, 16, one * 4, None) != 0
        assert lib.rf_dpm_update(one, 4, 0, 1.0, one * 2, one * 3, one * 3, 1, 16, one * 4, None) != 0
