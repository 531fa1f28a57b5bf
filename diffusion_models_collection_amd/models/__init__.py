"""Backbone registry (models/__init__.py of the reference): `from models import UNet, DiT, DiM`.

UNet (the hot path), DiT and DiM run on the gfx950 kernels. The reference picks DiM's token
mixer by whether `mamba_ssm` imports on the host; here it is chosen explicitly (mixer="mamba" | "attention"): a bare
DiM() raises NotImplementedError and says so (models/dim.py).
"""
from .dim import DiM
from .dit import DiT
from .unet import UNet

__all__ = ['UNet', 'DiT', 'DiM']
