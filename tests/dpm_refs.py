"""fp64 references of the DPM-Solver++ multistep sampler (reface_amd/dpm_solver.py).  TEST INFRASTRUCTURE.

Written step by step in the divided-difference form of the solver (D1 / D2, Lu et al. 2022, multistep data prediction) and NOT from the
coefficient table of dpm_solver.dpm_coefficients, so that the table -- and the kernel that consumes it -- is checked against something
that shares no algebra with it.  Also here: the analytic Gaussian model whose probability-flow ODE has a closed solution (the convergence
tests), the fp64 reference of one rf_dpm_update launch, and the sampler loop around the CPU oracle UNet.
"""
import numpy as np
import torch


def schedule(acp, nodes):
    """(alpha_k, sigma_k, lambda_k) at the nodes, fp64."""
    a = np.asarray(acp, dtype=np.float64)[np.asarray(nodes)]
    alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
    return alpha, sigma, np.log(alpha / sigma)


def order_used(order, i, S):
    return min(order, i + 1, S - i)


def step(x, eps, i, alpha, sigma, lam, order, hist):
    """One multistep step i: returns (x', m0).  ``hist``: data predictions of the earlier steps, newest last."""
    S = len(lam) - 1
    h = lam[i + 1] - lam[i]
    phi1 = np.expm1(-h)
    m0 = (x - sigma[i] * eps) / alpha[i]
    used = order_used(order, i, S)
    base = (sigma[i + 1] / sigma[i]) * x - alpha[i + 1] * phi1 * m0
    if used == 1:
        return base, m0
    m1 = hist[-1]
    r0 = (lam[i] - lam[i - 1]) / h
    if used == 2:
        D = (m0 - m1) / r0
        return base - 0.5 * alpha[i + 1] * phi1 * D, m0
    m2 = hist[-2]
    r1 = (lam[i - 1] - lam[i - 2]) / h
    D10, D11 = (m0 - m1) / r0, (m1 - m2) / r1
    D1 = D10 + r0 / (r0 + r1) * (D10 - D11)
    D2 = (D10 - D11) / (r0 + r1)
    phi2 = phi1 / h + 1.0
    phi3 = phi2 / h - 0.5
    return base + alpha[i + 1] * phi2 * D1 - alpha[i + 1] * phi3 * D2, m0


def run(acp, nodes, order, eps_fn, x_T):
    """The S-step loop: ``eps_fn(x, i, t_i) -> eps``.  Returns (x_final, [x_1 ... x_S], [m0 of every step])."""
    alpha, sigma, lam = schedule(acp, nodes)
    x, xs, hist = np.asarray(x_T, dtype=np.float64), [], []
    for i in range(len(nodes) - 1):
        x, m0 = step(x, eps_fn(x, i, int(nodes[i])), i, alpha, sigma, lam, order, hist)
        hist.append(m0)
        xs.append(x)
    return x, xs, hist


def table_run(rows, eps_seq, x_T):
    """numpy emulation of what the kernel does with the rows {alpha, sigma, A, k0, k1, k2, n_hist, 0}, in fp64: the trajectory [x_1 ... x_S]."""
    rows = np.asarray(rows, dtype=np.float64)
    x, m1, m2, xs = np.asarray(x_T, dtype=np.float64), None, None, []
    for i, (al, sg, A, k0, k1, k2, nh, _) in enumerate(rows):
        e = eps_seq(x, i) if callable(eps_seq) else eps_seq[i]
        m0 = (x - sg * e) / al
        xp = A * x + k0 * m0
        if nh >= 1:
            xp = xp + k1 * m1
        if nh >= 2:
            xp = xp + k2 * m2
        x, m2, m1 = xp, m1, m0
        xs.append(x)
    return xs


# ------------------------------------------------------------------------------------------------ the analytic model
class GaussianModel:
    """Per-element Gaussian data x0 ~ N(mu, s^2): the exact noise prediction is eps(x, t) = sigma_t (x - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2)
    and the probability-flow ODE from (T, x_T) has the solution x_t = alpha_t mu + sqrt(v_t / v_T) (x_T - alpha_T mu), v_t = alpha_t^2 s^2 + sigma_t^2."""

    def __init__(self, acp, n=4096, s_lo=0.2, seed=0):
        g = np.random.default_rng(seed)
        self.acp = np.asarray(acp, dtype=np.float64)
        self.mu = g.uniform(-1.0, 1.0, n)
        self.s = g.uniform(s_lo, 1.0, n)
        self.z = g.standard_normal(n)

    def _av(self, t):
        a = self.acp[t]
        return np.sqrt(a), a * self.s ** 2 + (1.0 - a)

    def x_start(self, T):
        al, v = self._av(T)
        return al * self.mu + np.sqrt(v) * self.z

    def eps(self, x, t):
        al, v = self._av(t)
        return np.sqrt(1.0 - self.acp[t]) * (x - al * self.mu) / v

    def exact(self, T, t):
        (aT, vT), (al, v) = self._av(T), self._av(t)
        return al * self.mu + np.sqrt(v / vT) * (self.x_start(T) - aT * self.mu)

    def rms_error(self, nodes, order):
        """RMS distance of the solver's final latent to the exact solution at the terminal node, from x_T at the first node."""
        T = int(nodes[0])
        x, _, _ = run(self.acp, nodes, order, lambda x, i, t: self.eps(x, t), self.x_start(T))
        return float(np.sqrt(np.mean((x - self.exact(T, int(nodes[-1]))) ** 2)))


# ------------------------------------------------------------------------------------------------ one rf_dpm_update launch
def update_inputs(B, hw, ld, cfg, seed):
    """eps [(2B|B), hw, ld] channels-last, img / m1 / m2 [B, 4, hw] -- seeded fp32 host tensors."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    return dict(eps=r((2 * B if cfg else B), hw, ld), img=r(B, 4, hw), m1=r(B, 4, hw), m2=r(B, 4, hw))


def update_ref(eps, img, m1, m2, row, cfg, scale):
    """fp64 reference of one launch on fp32 inputs and an fp32 row.  Returns (x', m0, limit of x', limit of m0): the limits are the file-level
    fp32 rule of tests/side_refs.py::limit_f32 applied to the terms of each sum, per element
    2e-5 (|A x| + |k0 m0| + |k1 m1| + |k2 m2|) + 2e-5 for x' and 2e-5 (|x / alpha| + |sigma e / alpha|) + 2e-5 for m0."""
    B = img.shape[0]
    e = eps.double()[..., :4]
    if cfg:
        e = e[:B] + float(np.float32(scale)) * (e[B:] - e[:B])
    e = e.permute(0, 2, 1)                                                  # -> [B, 4, hw]
    al, sg, A, k0, k1, k2, nh, _ = (float(v) for v in row.double())
    x = img.double()
    m0 = (x - sg * e) / al
    xp, terms = A * x + k0 * m0, (A * x).abs() + (k0 * m0).abs()
    if nh >= 1:
        xp, terms = xp + k1 * m1.double(), terms + (k1 * m1.double()).abs()
    if nh >= 2:
        xp, terms = xp + k2 * m2.double(), terms + (k2 * m2.double()).abs()
    return xp, m0, 2e-5 * terms + 2e-5, 2e-5 * ((x / al).abs() + (sg * e / al).abs()) + 2e-5


# ------------------------------------------------------------------------------------------------ the sampler around the oracle UNet
def sample(eps_fn, acp, nodes, order, x_T, cond, uc, z_inpaint, mask, scale):
    """The reference sampler: ``eps_fn(x9, t, ctx)`` is the (fp32, CPU) oracle UNet; everything around it -- CFG, data prediction, the
    solver -- is fp64.  Returns (final latent fp64 tensor, [m0 of every step])."""
    b = x_T.shape[0]

    def guided_eps(x, i, t):
        xin = torch.cat([torch.from_numpy(x).float(), z_inpaint, mask], dim=1)
        tt = torch.full((b,), t, dtype=torch.long)
        if uc is None or scale == 1.0:
            return eps_fn(xin, tt, cond).double().numpy()
        e_u, e_c = eps_fn(torch.cat([xin] * 2), torch.cat([tt] * 2), torch.cat([uc, cond])).double().chunk(2)
        return (e_u + scale * (e_c - e_u)).numpy()

    x, _, hist = run(acp, nodes, order, guided_eps, x_T.double().numpy())
    return torch.from_numpy(x), [torch.from_numpy(m) for m in hist]
