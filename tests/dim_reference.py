"""Test reference -- never imported by the product path.

A functional walk of the reference DiM (models/dim.py of sunyzhi55/Diffusion_Models_Collection) over a state_dict on
plain torch CPU ops, dtype-generic (fp32 or fp64; autograd supplies the backward), in the style of
oracle/dit_oracle.py, with both token mixers: the reference's nn.MultiheadAttention fallback (8 heads; pinned on
tests/golden/dim_tiny_attn.npz, which the reference itself produced) and the Mamba mixer of tests/mamba_reference.py.

bf16_gemm=True rounds the two operands of every GEMM the executor runs in its compute dtype (the token Linears, q k^T
and p v, and the two GEMMs of each one's backward; the conditioning MLP, the adaLN projection and the patch conv stay
fp32 there) to bf16 and leaves everything else in the working dtype: the yardstick for the kernels' bf16 mode.
"""
import math

import torch
import torch.nn.functional as F

from mamba_reference import MAMBA_KEYS, bf16_matmul, mamba_block


def timestep_embedding(t, dim, dtype, max_period=10000):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb.to(dtype)


class DiMReference:
    def __init__(self, sd, img_size=(32, 32), patch_size=2, in_channels=3, hidden_size=768, depth=12, state_size=16,
                 mlp_ratio=4.0, num_classes=None, dropout=0.1, mixer="attention", bf16_gemm=False):
        self.sd = sd
        if isinstance(img_size, int):
            img_size = (img_size, img_size)
        self.p, self.C, self.H, self.depth = patch_size, in_channels, hidden_size, depth
        self.num_classes = num_classes
        self.mixer = mixer
        self.heads = 8
        self.ht, self.wt = img_size[0] // patch_size, img_size[1] // patch_size
        self.mm = bf16_matmul if bf16_gemm else torch.matmul

    def w(self, k):
        return self.sd[k]

    def lin(self, x, wk, bk=None):
        y = self.mm(x, self.w(wk).T)
        return y if bk is None else y + self.w(bk)

    def ada(self, c, pre):
        return F.linear(F.silu(c), self.w(pre + "adaLN_modulation.1.weight"), self.w(pre + "adaLN_modulation.1.bias"))

    def norm(self, x, pre):
        return F.layer_norm(x, (self.H,), self.w(pre + ".weight"), self.w(pre + ".bias"), eps=1e-6)

    def mha(self, pre, h):
        B, L, H = h.shape
        hd = H // self.heads
        qkv = self.lin(h, pre + "in_proj_weight", pre + "in_proj_bias")
        q, k, v = qkv.split(H, dim=-1)
        q, k, v = (z.reshape(B, L, self.heads, hd).transpose(1, 2) for z in (q, k, v))
        a = torch.softmax(self.mm(q, k.transpose(-2, -1)) / math.sqrt(hd), dim=-1)
        o = self.mm(a, v).transpose(1, 2).reshape(B, L, H)
        return self.lin(o, pre + "out_proj.weight", pre + "out_proj.bias")

    def block(self, i, x, c):
        """models/dim.py:125-143, :165-173."""
        pre = f"blocks.{i}.mamba_block."
        shift, scale, gate = self.ada(c, pre).chunk(3, dim=-1)
        h = self.norm(x, pre + "norm") * (1 + scale[:, None]) + shift[:, None]
        if self.mixer == "attention":
            h = self.mha(pre + "mamba.", h)
        else:
            h = mamba_block(h, {k: self.w(pre + "mamba." + k) for k in MAMBA_KEYS}, self.mm)
        x = x + gate[:, None] * h
        pre = f"blocks.{i}.ff_block."
        shift, scale, gate = self.ada(c, pre).chunk(3, dim=-1)
        h = self.norm(x, pre + "norm") * (1 + scale[:, None]) + shift[:, None]
        h = self.lin(F.gelu(self.lin(h, pre + "mlp.0.weight", pre + "mlp.0.bias")), pre + "mlp.3.weight",
                     pre + "mlp.3.bias")
        return x + gate[:, None] * h

    def forward(self, x, t, y=None):
        """models/dim.py:314-346."""
        B = x.shape[0]
        p, C = self.p, self.C
        dtype = self.w("pos_embed").dtype
        x = x.to(dtype)
        h = F.conv2d(x, self.w("x_embedder.proj.weight"), self.w("x_embedder.proj.bias"), stride=p)
        h = h.flatten(2).transpose(1, 2) + self.w("pos_embed")
        te = timestep_embedding(t, self.w("t_embedder.mlp.0.weight").shape[1], dtype)
        te = F.linear(te, self.w("t_embedder.mlp.0.weight"), self.w("t_embedder.mlp.0.bias"))
        c = F.linear(F.silu(te), self.w("t_embedder.mlp.2.weight"), self.w("t_embedder.mlp.2.bias"))
        if self.num_classes is not None and y is not None:
            c = c + F.embedding(torch.clamp(y, 0, self.num_classes), self.w("y_embedder.embedding_table.weight"),
                                padding_idx=0)
        for i in range(self.depth):
            h = self.block(i, h, c)
        shift, scale = self.ada(c, "final_layer.").chunk(2, dim=-1)
        h = self.norm(h, "final_layer.norm_final") * (1 + scale[:, None]) + shift[:, None]
        h = self.lin(h, "final_layer.linear.weight", "final_layer.linear.bias")
        h = h.reshape(B, self.ht, self.wt, p, p, C)
        return torch.einsum("nhwpqc->nchpwq", h).reshape(B, C, self.ht * p, self.wt * p)


def make_reference(state_dict, cfg, dtype=torch.float32, requires_grad=False, **kw):
    sd = {k: v.detach().to(dtype).cpu().clone().requires_grad_(requires_grad) for k, v in state_dict.items()}
    cfg = {k: v for k, v in cfg.items() if k != "compute_dtype"}
    return DiMReference(sd, **cfg, **kw), sd


TINY_ATTN = dict(img_size=(16, 16), patch_size=2, in_channels=3, hidden_size=64, depth=2, state_size=16, mlp_ratio=4.0,
                 num_classes=10, dropout=0.0, mixer="attention")


def load_tiny_attn():
    """tests/golden/dim_tiny_attn.npz + dim_tiny_attn_grads.npz (gen_golden_dim.py: the reference's own DiM with the
    attention fallback) -> (arrays, params by state_dict key, gradients by parameter name)."""
    from conftest import load_golden
    g = load_golden("dim_tiny_attn")
    g.update(load_golden("dim_tiny_attn_grads"))
    params = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    grads = {k[len("grad/"):]: v for k, v in g.items() if k.startswith("grad/")}
    return g, params, grads


def perturb(m, std, seed=11):
    """Seeded N(0, std) added to every parameter in named_parameters order (off the zero init)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.add_(std * torch.randn(p.shape, generator=gen).to(p.device))
    return m
