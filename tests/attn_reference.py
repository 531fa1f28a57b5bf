"""Plain-torch CPU references of multi-head self-attention, forward and backward, for the attention kernel tests.

Layout (models/unet.py AttentionBlock): qkv is [N, L, 3*C] with C = heads*hd and channel index (which, head, d), i.e.
qkv.view(N, L, 3, heads, hd); out / dout are [N, L, C] with channel index (head, d).

With S = Q K^T / sqrt(hd), P = softmax(S) (row-wise), the keep-mask M in {0, 1} and keep_scale = 1/(1-p_drop):
    Pm = P * M * keep_scale          O  = Pm V                lse   = logsumexp(S)   (of the undropped softmax)
    dP = (dO V^T) * M * keep_scale   dV = Pm^T dO             delta = rowsum(dO * O) (= rowsum(P * dP))
    dS = P * (dP - delta)            dQ = dS K / sqrt(hd)     dK    = dS^T Q / sqrt(hd)

attention_f64 evaluates this in float64; attention_yardstick evaluates the same formulas in fp32 and, for bf16,
rounds where a bf16 tensor-core implementation has to round (the P and dS matrix operands, the stored O that delta
is formed from, the stored outputs). It restates the arithmetic, not any kernel's tile order. No project imports.
"""
import math

import torch


def _split(qkv, dout, heads, hd, dtype):
    N, L, C3 = qkv.shape
    assert C3 == 3 * heads * hd and dout.shape == (N, L, heads * hd)
    t = qkv.to(dtype).view(N, L, 3, heads, hd).permute(2, 0, 3, 1, 4)
    do = dout.to(dtype).view(N, L, heads, hd).permute(0, 2, 1, 3)
    return t[0], t[1], t[2], do


def _merge(x):
    """[N, heads, L, hd] -> [N, L, heads*hd]"""
    N, H, L, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(N, L, H * D)


def _softmax_lse(s):
    m = s.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
    return torch.exp(s - lse), lse.squeeze(-1)


def attention_f64(qkv, dout, heads, hd, mask=None, keep_scale=1.0):
    """float64 reference. mask: keep-mask [N, heads, L, L] (1 = kept) or None.

    Returns a dict: o, dq, dk, dv [N, L, C]; lse, delta [N, heads, L]; p, dp [N, heads, L, L] (dp is the masked and
    scaled dP); s (the scaled scores) and the head-split inputs q, k, v."""
    f64 = torch.float64
    q, k, v, do = _split(qkv, dout, heads, hd, f64)
    scale = 1.0 / math.sqrt(hd)
    s = (q @ k.transpose(-2, -1)) * scale
    p, lse = _softmax_lse(s)
    mk = None if mask is None else mask.to(f64) * keep_scale
    pm = p if mk is None else p * mk
    o = pm @ v
    dp = do @ v.transpose(-2, -1)
    if mk is not None:
        dp = dp * mk
    delta = (do * o).sum(-1)
    ds = p * (dp - delta.unsqueeze(-1))
    dq = (ds @ k) * scale
    dk = (ds.transpose(-2, -1) @ q) * scale
    dv = pm.transpose(-2, -1) @ do
    return dict(o=_merge(o), lse=lse, dq=_merge(dq), dk=_merge(dk), dv=_merge(dv), p=p, dp=dp, delta=delta, s=s,
                q=q, k=k, v=v)


def attention_yardstick(dtype, qkv, dout, heads, hd, mask=None, keep_scale=1.0):
    """The formulas of attention_f64 in fp32 arithmetic; dtype = torch.bfloat16 adds the bf16 roundings listed in the
    module docstring. Inputs are expected to be representable in dtype. Returns o, lse, dq, dk, dv as fp32 tensors
    holding dtype-representable values (lse is fp32 in both modes)."""
    f32 = torch.float32
    bf = dtype == torch.bfloat16

    def r(x):   # rounding of a matrix operand / a stored tensor
        return x.to(torch.bfloat16).to(f32) if bf else x

    q, k, v, do = _split(qkv, dout, heads, hd, f32)
    scale = f32_scalar(1.0 / math.sqrt(hd))
    s = (q @ k.transpose(-2, -1)) * scale
    p, lse = _softmax_lse(s)
    mk = None if mask is None else mask.to(f32) * f32_scalar(keep_scale)
    pm = p if mk is None else p * mk
    o = r(r(pm) @ v)
    dp = do @ v.transpose(-2, -1)
    if mk is not None:
        dp = dp * mk
    delta = (do * o).sum(-1)
    ds = r(p * (dp - delta.unsqueeze(-1)))
    dq = r((ds @ k) * scale)
    dk = r((ds.transpose(-2, -1) @ q) * scale)
    dv = r(r(pm).transpose(-2, -1) @ do)
    return dict(o=_merge(o), lse=lse, dq=_merge(dq), dk=_merge(dk), dv=_merge(dv))


def f32_scalar(x):
    return torch.tensor(x, dtype=torch.float32)


def floors(ref, dtype):
    """Absolute error floors 2*eps*M per tensor, M = magnitude of the terms being summed, from the float64 reference
    only. lse is an fp32 tensor in both modes."""
    eps = torch.finfo(dtype).eps
    eps32 = torch.finfo(torch.float32).eps
    hd = ref["q"].shape[-1]
    scale = 1.0 / math.sqrt(hd)

    def mx(x):
        return x.abs().max().item() if x.numel() else 0.0

    ds = mx(ref["p"] * (ref["dp"] - ref["delta"].unsqueeze(-1)))
    return dict(o=2 * eps * mx(ref["o"]), lse=2 * eps32 * mx(ref["lse"]), dv=2 * eps * mx(ref["dv"]),
                dq=2 * eps * scale * ds * mx(ref["k"]), dk=2 * eps * scale * ds * mx(ref["q"]))
