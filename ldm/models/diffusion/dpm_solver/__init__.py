"""``ldm.models.diffusion.dpm_solver`` -> reface_amd.dpm_solver (Stable Diffusion's dotted path; the CLIs' --dpm_solver)."""
from .sampler import DPMSolverSampler  # noqa: F401
