"""Drop-in shim: `from diffusion import DDPM, DDIM` resolves to the MI355X build (DPMSolver is this build's own)."""
from diffusion_models_collection_amd.diffusion import DDPM, DDIM, DPMSolver  # noqa: F401

__all__ = ['DDPM', 'DDIM', 'DPMSolver']
