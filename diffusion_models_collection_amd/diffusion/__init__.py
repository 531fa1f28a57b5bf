"""Diffusion schedulers (diffusion/__init__.py of the reference, plus the DPM-Solver++ sampler, the rectified flow and the
training-time timestep samplers)."""
from .ddpm import DDPM
from .ddim import DDIM
from .dpm_solver import DPMSolver
from .flow import RectifiedFlow
from .resample import LogitNormalSampler, LossSecondMomentResampler, UniformSampler, create_named_schedule_sampler

__all__ = ['DDPM', 'DDIM', 'DPMSolver', 'RectifiedFlow', 'UniformSampler', 'LossSecondMomentResampler',
           'LogitNormalSampler', 'create_named_schedule_sampler']
