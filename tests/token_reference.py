"""Test reference -- never imported by the product path.

The token-wise kernels of csrc/dmc_dit.hip as plain torch, dtype-generic (run in fp64 or fp32 on the CPU); autograd
supplies the backward. These are the semantics the kernels are held to:

    ln_mod   xn = x + gate[b] * mask * scale * br            (the gated residual with branch dropout)
             y  = (xn - mean) * rstd [* gamma + beta]        (LayerNorm over C, biased variance, eps inside the sqrt)
             h  = y * (1 + scale_mod[b]) + shift[b]
    gelu     a  = 0.5 u (1 + erf(u / sqrt 2)) * mask * scale
    timestep_embedding   [cos(t f_k) | sin(t f_k) | 0 if dim is odd],  f_k = exp(fp32(-ln max_period) * k / half)

Dropout masks are the counter hash of dmc_common.h over the element index row * C + c -- the index every one of these
kernels uses, whatever the pitch of the rows it reads or writes."""
import math

import numpy as np
import torch


def drop_mask(rows, C, seed, thresh, seed_base=0):
    """Keep mask [rows, C] (bool numpy) of a dropout with the given host seed (+ the device seed word)."""
    from test_gpu_kernels import drop_keep_np
    idx = np.arange(rows * C, dtype=np.int64)
    return drop_keep_np(idx, (seed + seed_base) & 0xFFFFFFFF, thresh).reshape(rows, C)


def per_row(v, L):
    """[B, C] per-image rows -> [B * L, C] per-token rows."""
    return v.repeat_interleave(L, 0)


def gated_branch(br, gate, L, mask=None, scale=1.0, bias=None):
    """gate[b] * mask * scale * (br + bias): what ln_mod adds to x. br [T, C], gate [B, C], mask [T, C] of 0 / 1."""
    v = br if bias is None else br + bias
    if mask is not None:
        v = v * mask * scale
    return per_row(gate, L) * v


def ln_mod(x, shift, scale_mod, L, eps, br=None, gate=None, mask=None, scale=1.0, gamma=None, beta=None):
    """x [T, C]; shift, scale_mod, gate [B, C] -> (h, xn, mean [T], rstd [T])."""
    xn = x if br is None else x + gated_branch(br, gate, L, mask, scale)
    mean = xn.mean(-1, keepdim=True)
    var = ((xn - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xn - mean) * rstd
    if gamma is not None:
        y = y * gamma + beta
    h = y * (1 + per_row(scale_mod, L)) + per_row(shift, L)
    return h, xn, mean[:, 0], rstd[:, 0]


def gelu(u, mask=None, scale=1.0):
    a = 0.5 * u * (1 + torch.erf(u * (1.0 / math.sqrt(2.0))))
    return a if mask is None else a * mask * scale


def timestep_embedding(t, dim, max_period=10000.0, dtype=torch.float64):
    """t [B] integer steps -> [B, dim]."""
    half = dim // 2
    nl = float(np.float32(-math.log(max_period)))      # the Python double meets a float32 tensor: rounded first
    f = torch.exp(nl * torch.arange(half, dtype=dtype) / half)
    a = t.to(dtype)[:, None] * f[None]
    out = torch.cat([torch.cos(a), torch.sin(a)], dim=-1)
    if dim % 2:
        out = torch.cat([out, torch.zeros(t.shape[0], 1, dtype=dtype)], dim=-1)
    return out
