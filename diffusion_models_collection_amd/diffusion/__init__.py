"""Diffusion schedulers (diffusion/__init__.py of the reference, plus the DPM-Solver++ sampler and the training-time
timestep samplers)."""
from .ddpm import DDPM
from .ddim import DDIM
from .dpm_solver import DPMSolver
from .resample import LossSecondMomentResampler, UniformSampler, create_named_schedule_sampler

__all__ = ['DDPM', 'DDIM', 'DPMSolver', 'UniformSampler', 'LossSecondMomentResampler', 'create_named_schedule_sampler']
