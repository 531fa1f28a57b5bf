"""Test reference -- never imported by the product path.

The Mamba token mixer of the DiM as plain torch, dtype-generic (run in fp64 or fp32 on CPU), an explicit token loop;
autograd supplies the backward. These are the semantics the dmc_mamba.hip kernels are held to (the recurrence of
mamba_ssm's selective scan with delta_softplus, D and the z gate, written from the published algorithm):

    xz = h in_proj.W^T                      x = xz[..., :E], z = xz[..., E:]
    u_t = silu(conv1d.bias + sum_k conv1d.W[c,0,k] * x_{t-3+k})           x_{<0} = 0 per image
    dbc = u x_proj.W^T  -> [R | N | N] = dt_low, Bm, Cm
    delta = softplus(dt_low dt_proj.W^T + dt_proj.bias)                    torch softplus, threshold 20
    A = -exp(A_log);  s_t = exp(delta_t A) s_{t-1} + delta_t Bm_t u_t;  y_t = sum_n Cm_t s_t + D u_t
    out = (y * silu(z)) out_proj.W^T
"""
import torch
import torch.nn.functional as F

MAMBA_KEYS = ["A_log", "D", "in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight",
              "dt_proj.bias", "out_proj.weight"]


def causal_conv_silu(x, w, b):
    """x [B, L, E], w [E, 1, 4] (or [E, 4]), b [E] -> silu of the causal depthwise conv over L."""
    B, L, E = x.shape
    w = w.reshape(E, 4)
    xp = torch.cat([x.new_zeros(B, 3, E), x], dim=1)
    pre = b + sum(w[:, k] * xp[:, k:k + L] for k in range(4))
    return F.silu(pre)


def selective_scan(u, z, dpre, Bm, Cm, A_log, D, dt_bias):
    """u, z, dpre [B, L, E]; Bm, Cm [B, L, N]; A_log [E, N]; D, dt_bias [E] -> gated y [B, L, E]."""
    B, L, E = u.shape
    delta = F.softplus(dpre + dt_bias)
    A = -torch.exp(A_log)
    s = u.new_zeros(B, E, A.shape[1])
    ys = []
    for t in range(L):
        dA = torch.exp(delta[:, t, :, None] * A)
        s = dA * s + delta[:, t, :, None] * Bm[:, t, None, :] * u[:, t, :, None]
        ys.append((s * Cm[:, t, None, :]).sum(-1) + D * u[:, t])
    y = torch.stack(ys, dim=1)
    return y * F.silu(z)


class _BF16MatMul(torch.autograd.Function):
    """a @ b with the two operands of every GEMM rounded to bf16 and the products accumulated in the working dtype:
    the forward GEMM and the two GEMMs of its backward (dy b^T and a^T dy)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _rb(a) @ _rb(b)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        da = _rb(dy) @ _rb(b).transpose(-1, -2)
        db = _rb(a).transpose(-1, -2) @ _rb(dy)
        while db.dim() > b.dim():       # a weight broadcast over the batch
            db = db.sum(0)
        return da, db


def _rb(v):
    return v.to(torch.bfloat16).to(v.dtype)


def bf16_matmul(a, b):
    return _BF16MatMul.apply(a, b)


def mamba_block(h, p, mm=torch.matmul):
    """h [B, L, H]; p: the nine tensors of MAMBA_KEYS by name. mm: the matmul of the four projections
    (bf16_matmul for the bf16 yardstick)."""
    E, N = p["A_log"].shape
    R = p["dt_proj.weight"].shape[1]
    xz = mm(h, p["in_proj.weight"].T)
    x, z = xz[..., :E], xz[..., E:]
    u = causal_conv_silu(x, p["conv1d.weight"], p["conv1d.bias"])
    dbc = mm(u, p["x_proj.weight"].T)
    dt_low, Bm, Cm = dbc[..., :R], dbc[..., R:R + N], dbc[..., R + N:]
    dpre = mm(dt_low, p["dt_proj.weight"].T)
    y = selective_scan(u, z, dpre, Bm, Cm, p["A_log"], p["D"], p["dt_proj.bias"])
    return mm(y, p["out_proj.weight"].T)
