"""``ldm.models.diffusion.dpm_solver.sampler`` -> reface_amd.dpm_solver."""
from reface_amd.dpm_solver import DPMSolverSampler  # noqa: F401
