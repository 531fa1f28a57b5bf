"""Drop-in shim: `from diffusion import DDPM, DDIM` resolves to the MI355X build (DPMSolver and RectifiedFlow are this
build's own)."""
from diffusion_models_collection_amd.diffusion import DDPM, DDIM, DPMSolver, RectifiedFlow  # noqa: F401

__all__ = ['DDPM', 'DDIM', 'DPMSolver', 'RectifiedFlow']
