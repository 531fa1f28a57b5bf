"""Generate tests/golden/dim_tiny_attn.npz and dim_tiny_attn_grads.npz from the UNMODIFIED reference DiM.

Run ONLY in the build container (where /root/reference exists and `mamba_ssm` does not import, so the reference's
MambaBlock takes its nn.MultiheadAttention fallback, models/dim.py:11-17, :110-117):
    python tests/golden/gen_golden_dim.py

It imports sunyzhi55/Diffusion_Models_Collection from /root/reference (read-only, never shipped), runs its DiM on
CPU in fp32 and stores plain numpy arrays, in the layout of dit_tiny_cond.npz (tests/golden/gen_golden.py gen_dit):
  param/<key>   the state_dict: torch.manual_seed(1234) initialisation + the seeded N(0, 0.05) perturbation off the
                zero init (every adaLN projection and the final linear are zero-initialised, models/dim.py:288-298)
  x, t, y, cot  inputs and the cotangent; out, out_ynone (y=None) the outputs
  grad_x, grad/<key>   the gradients of sum(out * cot): in dim_tiny_attn_grads.npz (parameters and gradients are
                incompressible and together exceed the 1 MiB a committed file may have, so they are two files)
"""
import sys
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
CFG = dict(img_size=(16, 16), patch_size=2, in_channels=3, hidden_size=64, depth=2, state_size=16, mlp_ratio=4.0,
           num_classes=10, dropout=0.0)


def perturb(m, std, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.add_(std * torch.randn(p.shape, generator=g))


def main(B=2):
    sys.path.insert(0, str(REF))
    from models import dim as ref_dim  # noqa: E402  (reference)
    assert not ref_dim.MAMBA_AVAILABLE, "this fixture is the attention fallback: mamba_ssm must not import"
    torch.manual_seed(1234)
    m = ref_dim.DiM(**CFG).float()
    perturb(m, 0.05)
    m.train()   # dropout 0.0 -> deterministic
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, CFG["in_channels"], *CFG["img_size"], generator=g).requires_grad_(True)
    t = torch.tensor([17, 903, 500, 0][:B], dtype=torch.long)
    y = torch.tensor([0, 11, 3, 10][:B], dtype=torch.long)
    out = m(x, t, y)
    cot = torch.randn(out.shape, generator=g)
    (out * cot).sum().backward()
    arrs = {"x": x.detach(), "t": t, "y": y, "out": out.detach(), "cot": cot}
    with torch.no_grad():
        arrs["out_ynone"] = m(x.detach(), t, None)
    for k, v in m.state_dict().items():
        arrs["param/" + k] = v
    grads = {"grad_x": x.grad}
    for k, p in m.named_parameters():
        grads["grad/" + k] = p.grad
    for name, d in (("dim_tiny_attn.npz", arrs), ("dim_tiny_attn_grads.npz", grads)):
        clean = {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in d.items()}
        np.savez_compressed(OUT / name, **clean)
        print("wrote", OUT / name, sum(a.nbytes for a in clean.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    main()
