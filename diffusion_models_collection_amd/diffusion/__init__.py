"""Diffusion schedulers (diffusion/__init__.py of the reference, plus the DPM-Solver++ sampler)."""
from .ddpm import DDPM
from .ddim import DDIM
from .dpm_solver import DPMSolver

__all__ = ['DDPM', 'DDIM', 'DPMSolver']
