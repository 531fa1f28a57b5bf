"""Executor of the DiT (models/dit.py of the reference, :87-295) on the gfx950 kernels, forward + backward.

Token rows [T = B * L, C] are the NHWC pixels of a [B, h_tokens, w_tokens, C] grid, so every Linear is a 1x1
implicit-GEMM conv (dmc_conv2d, MFMA) and the patch embedding the 2x2 stride-2 conv. Per forward:

  timestep embedding [cos|sin] -> Linear -> SiLU -> Linear (+ label embedding)            = c  [B, H]
  ONE GEMM for every block's adaLN_modulation and the final layer's (weights stacked)    = mod [B, 12*6H + 2H]
  patch conv (fp32) + pos_embed                                                          = x   (fp32 stream)
  per block:  h1 = LN(x) * (1 + scale_msa) + shift_msa            (dmc_ln_mod_fwd, fused with the previous
                                                                   block's gated MLP residual)
              qkv = h1 W_in^T + b -> flash attention (probability dropout in training) -> o W_out^T + b = ao
              x_mid = x + gate_msa * ao;  h2 = LN(x_mid) * (1 + scale_mlp) + shift_mlp   (one fused kernel)
              u = h2 W1^T + b1 -> a = Dropout(GELU(u)) -> mo = a W2^T + b2   (x_out = x_mid + gate_mlp * drop(mo)
                                                                              folded into the next LayerNorm)
  final: LN + modulation (fused with the last residual) -> Linear -> unpatchify (NCHW fp32)

The backward walks the tape in reverse with the same fused kernels (dmc_gate_bwd, dmc_ln_mod_bwd, dmc_gelu_bwd,
the conv dgrad/wgrad kernels, dmc_attn_bwd) and writes every parameter gradient into one flat fp32 buffer laid out
in the order the backward finishes them (data-parallel buckets, fused clip + AdamW + EMA: utils/trainer.py).
The residual stream stays fp32; GEMM operands are in the compute dtype (bf16 in perf mode).

TokenExecutor is that walk for any backbone of this shape (the DiM of _dim_exec.py is the other one): everything
around the blocks, the block forward and the attention mixer. A backbone supplies its parameters in completion order,
its LayerNorm kernels, its token mixer and its block backward.
"""
import os

import torch

from .. import _lib as L
from .. import kernels as K
from ._unet_exec import Act, ExecCore, _seed_from_torch

# GELU + Dropout in fc1's epilogue (training with MLP dropout) and their backward in fc2's input-gradient epilogue
# (A/B: DMC_GELU_DROP_EPI=0 keeps dmc_gelu_fwd / dmc_gelu_bwd)
# measured slower on the DiT train step (erf/exp in the GEMM epilogue cost more than the separate HBM-bound pass:
# 6958 -> 6874 img/s forward, -> 6839 backward), so off by default
_GELU_EPI_BITS = int(os.environ.get("DMC_GELU_DROP_EPI", "0") or 0)   # bit 0: forward, bit 1: backward
# inference / dropout-free training: GELU in fc1's epilogue (DMC_GELU_EPI=0: conv + dmc_gelu_fwd, for A/B)
_GELU_EPI = os.environ.get("DMC_GELU_EPI", "1") not in ("", "0")
_GELU_DROP_EPI = bool(_GELU_EPI_BITS & 1)
_DGELU_EPI = bool(_GELU_EPI_BITS & 2)


class _W:
    """A weight holder for the pack cache (nn.MultiheadAttention keeps in_proj_weight as a bare Parameter)."""

    def __init__(self, weight):
        self.weight = weight


class _Call:
    """The shapes of one forward or backward and its modulation rows mod2 [B, ada_total] (fp32)."""

    def __init__(self, m, B, device):
        self.B, self.ht, self.wt, self.dev = B, m.h_tokens, m.w_tokens, device
        self.Lt = self.ht * self.wt
        self.T = B * self.Lt
        self.mod2 = None


class _BlockRec:
    """What block i's forward leaves to its backward: the tape record. An inference forward fills ONE record block
    after block, so each buffer is released when the next block stores its successor (the allocation order of the
    captured sampling graphs: releasing a block's buffers together measured 1% slower on the DiM DDIM-50 line)."""

    __slots__ = ("i", "x_in", "h1", "mean1", "rstd1", "saved", "ao", "d0", "x_mid", "h2", "mean2", "rstd2", "d1", "a",
                 "u", "mo", "d2")


class TokenExecutor(ExecCore):
    """The adaLN token backbone shared by the DiT and the DiM. A subclass sets the class attributes below and has

      _final_params()                          the final layer's parameters in backward-completion order
      _block_params(blk)                       a block's, likewise (the gradient prefix is published after each list)
      _block_parts(blk)                        (norm before the mixer, norm before the MLP, the MLP Sequential)
      _ln_kernel(norm)                         (LN + modulation forward kernel, its arguments between eps and h)
      _ln_bwd(g, norm, dh, xs, mean, rstd, off_shift, dx, dmod, gv)
      _mixer_fwd(g, i, blk, h1)                -> (ao, saved, attention dropout spec or None)
      _block_bwd(g, r, dx, dmod, gv)           one _BlockRec backwards: dx, dmod and the block's gradients
    """
    name = None             # "DiT" / "DiM" in error messages
    # GELU + Dropout in fc1's epilogue (the forward half of DMC_GELU_DROP_EPI)
    gelu_drop_epi = False
    # Gradient rows that are summed over tokens stay fp32 in bf16 mode: the GEMMs in front of a LayerNorm backward
    # store fp32 (out_f32), the attention out_proj's bias gradient comes from dmc_gate_bwd_bias, the final linear's
    # from the fp32 cotangent. False: compute-dtype rows, every bias gradient from its weight-gradient kernel.
    f32_sums = False

    def __init__(self, model, ada):
        """ada: the blocks' adaLN Linears in stacking order, 6H rows per block (the final layer's 2H rows follow)."""
        self._setup(model)
        H = model.hidden_size
        self.H = H
        self.blocks = list(model.blocks)
        # stacked adaLN projections: block i's 6H rows at 6H*i, the final layer's 2H rows last
        self.ada = ada + [model.final_layer.adaLN_modulation[1]]
        self.ada_off = [6 * H * i for i in range(len(self.blocks))] + [6 * H * len(self.blocks)]
        self.ada_total = 6 * H * len(self.blocks) + 2 * H
        p = model.patch_size
        if p * p > 16:
            raise L.DMCError(f"{self.name}: patch size {p} (the implicit-GEMM conv takes at most 16 taps)")
        self.patch_taps = [(i, j) for i in range(p) for j in range(p)]   # Conv2d(k=p, s=p) as p*p taps
        self._layout_grads()

    # ---------------------------------------------------------------------------------------
    def _layout_grads(self):
        """Flat gradient layout in backward-completion order: the final layer, blocks last to first, pos_embed and
        the patch conv, the stacked adaLN weights and biases (rows in stacking order, so the stacked weight
        gradient lands in place), the timestep MLP, the label table."""
        m = self.m
        order = self._final_params()
        for b in reversed(self.blocks):
            order += self._block_params(b)
        order += [m.pos_embed, m.x_embedder.proj.weight, m.x_embedder.proj.bias]
        order += [lin.weight for lin in self.ada] + [lin.bias for lin in self.ada]
        order += [m.t_embedder.mlp[2].weight, m.t_embedder.mlp[2].bias, m.t_embedder.mlp[0].weight,
                  m.t_embedder.mlp[0].bias]
        if m.y_embedder is not None:
            order.append(m.y_embedder.embedding_table.weight)
        self._set_grad_order(order)
        self.order_ids = [id(p) for p in order]
        self.ada_w_off = self.goff[self.pindex[id(self.ada[0].weight)]]
        self.ada_b_off = self.goff[self.pindex[id(self.ada[0].bias)]]
        # publish points: the gradient prefix that is final after the final layer / after block i
        end = lambda p: self.goff[self.pindex[id(p)]] + p.numel()     # noqa: E731
        self.pub_final = end(self._final_params()[-1])
        self.pub_block = [end(self._block_params(b)[-1]) for b in self.blocks]

    def _ada_pack(self, dtype=torch.float32):
        """Packed [ada_total][1][Kc] forward weight of all adaLN projections."""
        H = self.H
        Kc = L.kc_for(H, dtype)

        def jobs(buf):
            out, off = [], 0
            for lin in self.ada:
                co = lin.weight.shape[0]
                out.append((lin.weight, buf, off * Kc, L.PACK_FWD, co, H, 1, 1, Kc, -1))
                off += co
            return out

        return self.packs.get(("ada", dtype), tuple(lin.weight for lin in self.ada),
                              lambda: torch.zeros(self.ada_total * Kc, dtype=dtype, device=self.ada[0].weight.device),
                              jobs)

    def _ada_pack_dgrad(self, dtype=torch.float32):
        H = self.H
        Kt = L.kc_for(self.ada_total, dtype)

        def jobs(buf):
            out, off = [], 0
            for lin in self.ada:
                co = lin.weight.shape[0]
                out.append((lin.weight, buf, 0, L.PACK_DGRAD, co, H, 1, 1, Kt, off))
                off += co
            return out

        return self.packs.get(("ada_dg", dtype), tuple(lin.weight for lin in self.ada),
                              lambda: torch.zeros(H * Kt, dtype=dtype, device=self.ada[0].weight.device), jobs)

    def _ada_bias(self):
        def jobs(buf):
            out, off = [], 0
            for lin in self.ada:
                co = lin.bias.shape[0]
                out.append((lin.bias, buf, off, L.PACK_FWD, co, 1, 1, 1, 1, -1))
                off += co
            return out

        return self.packs.get("ada_b", tuple(lin.bias for lin in self.ada),
                              lambda: torch.empty(self.ada_total, dtype=torch.float32, device=self.ada[0].bias.device),
                              jobs)

    def _drop(self, site):
        """The dropout spec of site 2i (block i's MLP activation), 2i + 1 (its MLP output) or 2 * depth + i (its
        attention probabilities); None outside training."""
        if self._drop_spec is None:
            return None
        d = ((self._seed_base + 7919 * site) & 0xFFFFFFFF, self._drop_spec[0], self._drop_spec[1])
        if self.seed_ptr is not None:
            d = d + (self.seed_ptr,)
        return d

    def _rows(self, g, C, dtype=None):
        return torch.empty(g.B, g.ht, g.wt, C, dtype=dtype or self.dt, device=g.dev)

    def _ln_rows(self, g):
        """The buffer of a gradient fed to _ln_bwd, and the out_f32 of the GEMM that fills it."""
        return self._rows(g, self.H, torch.float32 if self.f32_sums else self.dt), self.f32_sums

    # =========================================================================================
    def forward(self, x, t, y, keep):
        m = self.m
        self.device = x.device
        self.packs.refresh()
        f32 = torch.float32
        B, Cin, Hi, Wi = x.shape
        p = m.patch_size
        g = _Call(m, B, x.device)
        ht, wt = g.ht, g.wt
        H = self.H
        x = x.contiguous().float()
        t = t.to(device=x.device, dtype=torch.long).contiguous()
        tape = [] if keep else None
        if m.training and m.dropout > 0:
            pd = float(m.dropout)
            self._drop_spec = (min(int(round(pd * 4294967296.0)), 4294967295), 1.0 / (1.0 - pd) if pd < 1 else 0.0)
            self._seed_base = 0 if self.seed_ptr is not None else _seed_from_torch()
        else:
            self._drop_spec = None

        # ---- conditioning: c = MLP(timestep embedding) (+ label embedding) ----
        te = m.t_embedder
        fdim = te.frequency_embedding_size
        tf = torch.empty(B, 1, 1, fdim, dtype=f32, device=x.device)
        K.timestep_embedding(t, fdim, tf.view(B, fdim))
        A0 = Act(tf, 1, 1, fdim)
        A1 = self._new(B, 1, 1, H, f32)
        self._conv([A0], te.mlp[0], K.TAPS1, 1, 1, H, bias=te.mlp[0].bias, out=A1.t, dtype=f32)
        c = self._new(B, 1, 1, H, f32)
        ye = None
        if m.y_embedder is not None and y is not None:
            y = y.to(device=x.device, dtype=torch.long).contiguous()
            ye = torch.empty(B, 1, 1, H, dtype=f32, device=x.device)
            K.embed_fwd(y, m.y_embedder.embedding_table.weight, ye.view(B, H))   # clamps y to [0, num_classes]
        self._conv([A1], te.mlp[2], K.TAPS1, 1, 1, H, pro=(L.PRO_SILU, None, None), bias=te.mlp[2].bias, resid=ye,
                   out=c.t, dtype=f32)
        mod = torch.empty(B, 1, 1, self.ada_total, dtype=f32, device=x.device)
        self._conv([c], None, K.TAPS1, 1, 1, self.ada_total, pro=(L.PRO_SILU, None, None), bias=self._ada_bias(),
                   out=mod, dtype=f32, w=self._ada_pack(f32), Kc=L.kc_for(H, f32))
        g.mod2 = mod.view(B, self.ada_total)

        # ---- patch embedding (fp32) + pos_embed: the fp32 residual stream ----
        c4 = L.chunk_for(f32)
        xin = Act(K.pack_input(f32, x, (Cin + c4 - 1) // c4 * c4), Hi, Wi, Cin)
        x0 = torch.empty(B, ht, wt, H, dtype=f32, device=x.device)
        self._conv([xin], m.x_embedder.proj, self.patch_taps, ht, wt, H, stride=p, bias=m.x_embedder.proj.bias,
                   out=x0, dtype=f32)
        K.add_bcast(x0, m.pos_embed, B, g.Lt * H)
        if keep:
            tape.append(("embed", t, y, tf, A1, c, ye, mod, xin))

        xcur = x0
        pend = None            # (mo, gate offset, drop) of the previous block's MLP branch, not yet added
        r = _BlockRec()
        for i, blk in enumerate(self.blocks):
            if keep:
                r = _BlockRec()
                tape.append(r)
            xcur, pend = self._block_fwd(g, i, blk, xcur, pend, r, keep)
        # ---- final layer ----
        x_fin, hf, meanf, rstdf = self._ln(g, m.final_layer.norm_final, xcur, pend, self.ada_off[-1])
        fl = m.final_layer.linear
        K_out = fl.out_features
        ldo = (K_out + 3) // 4 * 4
        otok = torch.empty(B, ht, wt, ldo, dtype=f32, device=x.device)
        self._conv([Act(hf, ht, wt, H)], fl, K.TAPS1, ht, wt, K_out, bias=fl.bias, out=otok, out_f32=True)
        out = torch.empty(B, m.out_channels, Hi, Wi, dtype=f32, device=x.device)
        K.unpatchify(otok, ldo, B, ht, wt, p, m.out_channels, out)
        if keep:
            tape.append(("final", x_fin, hf, meanf, rstdf, ldo))
        return out, tape

    def _ln(self, g, norm, xs, pend, off_shift):
        """x_new = xs + gate * drop(br) (pend = (br, gate offset, drop) given), then LN + modulation by the rows at
        off_shift (shift) and off_shift + H (scale) -> (x_new, h, mean, rstd)."""
        br, off_gate, drop = pend if pend is not None else (None, 0, None)
        H = self.H
        f32 = torch.float32
        h = self._rows(g, H)
        mean = torch.empty(g.T, dtype=f32, device=g.dev)
        rstd = torch.empty(g.T, dtype=f32, device=g.dev)
        xo = self._rows(g, H, f32) if br is not None else None
        kernel, affine = self._ln_kernel(norm)
        kernel(self.dt, xs, g.T, H, g.Lt, g.mod2, self.ada_total, off_shift, off_shift + H, 1e-6, *affine, h, H, mean,
               rstd, br=br, ld_br=H, off_gate=off_gate, drop=drop, x_out=xo)
        return (xo if xo is not None else xs), h, mean, rstd

    def _block_fwd(self, g, i, blk, xcur, pend, r, keep):
        """Fills the record r -> (the stream before the MLP branch, the MLP branch still to be added to it)."""
        H = self.H
        norm1, norm2, mlp = self._block_parts(blk)
        mo_ = self.ada_off[i]
        r.i = i
        r.x_in, r.h1, r.mean1, r.rstd1 = self._ln(g, norm1, xcur, pend, mo_)
        r.ao, r.saved, r.d0 = self._mixer_fwd(g, i, blk, r.h1)
        r.x_mid, r.h2, r.mean2, r.rstd2 = self._ln(g, norm2, r.x_in, (r.ao.t, mo_ + 2 * H, None), mo_ + 3 * H)
        r.d1 = self._drop(2 * i)
        self._mlp_fwd(g, mlp, r, keep)
        r.d2 = self._drop(2 * i + 1)
        return r.x_mid, (r.mo.t, mo_ + 5 * H, r.d2)

    def _mlp_fwd(self, g, mlp, r, keep):
        """r.u = fc1(r.h2), r.a = Dropout(GELU(u)) (spec r.d1), r.mo = fc2(a). The pre-activation u is stored only
        when the backward or a separate GELU pass needs it (None otherwise)."""
        B, ht, wt, H = g.B, g.ht, g.wt, self.H
        Hm = mlp[0].out_features
        d1 = r.d1
        r.a = a = self._new(B, ht, wt, Hm)
        r.u = u = self._new(B, ht, wt, Hm) if keep or d1 is not None else None
        A2 = Act(r.h2, ht, wt, H)
        if d1 is None and _GELU_EPI:
            # GELU in fc1's epilogue
            self._conv([A2], mlp[0], K.TAPS1, ht, wt, Hm, bias=mlp[0].bias, out=a.t, act=L.ACT_GELU,
                       y_pre=None if u is None else u.t)
        elif d1 is not None and self.gelu_drop_epi:
            # GELU + the MLP Dropout in fc1's epilogue (bitwise dmc_gelu_fwd of the stored pre-activation)
            self._conv([A2], mlp[0], K.TAPS1, ht, wt, Hm, bias=mlp[0].bias, out=a.t, act=L.ACT_GELU_DROP, y_pre=u.t,
                       drop=d1)
        else:
            ub = u.t if u is not None else a.t
            self._conv([A2], mlp[0], K.TAPS1, ht, wt, Hm, bias=mlp[0].bias, out=ub)
            K.gelu_fwd(self.dt, ub, g.T, Hm, Hm, a.t, drop=d1)
        r.mo = mo = self._new(B, ht, wt, H)
        self._conv([a], mlp[3], K.TAPS1, ht, wt, H, bias=mlp[3].bias, out=mo.t)

    # ---- the attention mixer: at = the nn.MultiheadAttention, self.in_proj[i] its in_proj_weight holder ----
    def _attn_fwd(self, g, i, at, h1):
        B, ht, wt, H = g.B, g.ht, g.wt, self.H
        heads = self.m.num_heads
        qkv = self._new(B, ht, wt, 3 * H)
        self._conv([Act(h1, ht, wt, H)], self.in_proj[i], K.TAPS1, ht, wt, 3 * H, bias=at.in_proj_bias, out=qkv.t)
        o = self._new(B, ht, wt, H)
        lse = torch.empty(B * heads * g.Lt, dtype=torch.float32, device=g.dev)
        d0 = self._drop(2 * len(self.blocks) + i)      # attention-probability dropout (MHA dropout=p)
        K.attn_fwd(self.dt, qkv.t, 3 * H, B, g.Lt, heads, H // heads, o.t, H, lse, drop=d0)
        ao = self._new(B, ht, wt, H)
        self._conv([o], at.out_proj, K.TAPS1, ht, wt, H, bias=at.out_proj.bias, out=ao.t)
        return ao, (qkv, o, lse), d0

    def _attn_bwd(self, g, i, at, h1, saved, d0, dao, gv):
        """dao = the gradient of the mixer output [T, H] -> the gradient of h1 (_ln_rows); writes the mixer's
        parameter gradients (with f32_sums out_proj.bias is the caller's, from dmc_gate_bwd_bias)."""
        qkv, o, lse = saved
        ht, wt, H = g.ht, g.wt, self.H
        heads = self.m.num_heads
        op = at.out_proj
        self._wgrad([o], dao, H, K.TAPS1, ht, wt, H, gv(op.weight), dbias=None if self.f32_sums else gv(op.bias))
        do = self._rows(g, H)
        self._conv([Act(dao, ht, wt, H)], op, K.TAPS1, ht, wt, H, out=do, packmode=L.PACK_DGRAD)
        dqkv = self._rows(g, 3 * H)
        K.attn_bwd(self.dt, qkv.t, 3 * H, o.t, do, H, lse, g.B, g.Lt, heads, H // heads, dqkv, 3 * H, drop=d0)
        self._wgrad([Act(h1, ht, wt, H)], dqkv, 3 * H, K.TAPS1, ht, wt, 3 * H, gv(at.in_proj_weight),
                    dbias=gv(at.in_proj_bias))
        dh1, f32_out = self._ln_rows(g)
        self._conv([Act(dqkv, ht, wt, 3 * H)], self.in_proj[i], K.TAPS1, ht, wt, H, out=dh1, packmode=L.PACK_DGRAD,
                   out_f32=f32_out)
        return dh1

    def _gate_bwd(self, g, dx, br, off_gate, dmod, drop=None, dbias=None):
        """The branch of x + gate * drop(br): its gradient rows (compute dtype) from the stream gradient dx, the gate's
        into dmod; with dbias also the bias gradient of the branch's last Linear, summed from the fp32 dx instead of
        the stored rows."""
        H = self.H
        dbr = self._rows(g, H)
        if dbias is None:
            K.gate_bwd(self.dt, dx, br, H, g.mod2, self.ada_total, off_gate, g.T, H, g.Lt, dbr, H, dmod, off_gate,
                       drop=drop)
        else:
            K.gate_bwd_bias(self.dt, dx, br, H, g.mod2, self.ada_total, off_gate, g.T, H, g.Lt, dbr, H, dmod, off_gate,
                            dbias, drop=drop)
        return dbr

    # =========================================================================================
    def backward(self, tape, dout, x_requires_grad):
        m = self.m
        dt = self.dt
        f32 = torch.float32
        flat = self._grad_buffer(dout.device)
        gv = lambda p: self._gview(flat, p)  # noqa: E731
        B = dout.shape[0]
        p = m.patch_size
        dev = dout.device
        g = _Call(m, B, dev)
        ht, wt, Lt = g.ht, g.wt, g.Lt
        H = self.H
        emb = tape[0]
        g.mod2 = emb[7].view(B, self.ada_total)
        dmod = torch.empty(B, self.ada_total, dtype=f32, device=dev)
        hook = self.grad_hook

        def publish(pos, final):
            if hook is not None:
                hook(flat, pos, final)

        # ---- final layer ----
        _, x_fin, hf, meanf, rstdf, ldo = tape[-1]
        fl = m.final_layer.linear
        K_out = fl.out_features
        ldq = (K_out + self.chunk - 1) // self.chunk * self.chunk
        dtok = torch.empty(B, ht, wt, ldq, dtype=dt, device=dev)
        K.patchify_grad(dt, dout.contiguous(), B, ht, wt, p, m.out_channels, dtok, ldq)
        if self.f32_sums and dt != f32:
            # the output bias gradient is a plain sum of the fp32 cotangent: not taken from its bf16 copy
            self._wgrad([Act(hf, ht, wt, H)], dtok, ldq, K.TAPS1, ht, wt, K_out, gv(fl.weight))
            ld4 = (K_out + 3) // 4 * 4
            dtok32 = torch.empty(B, ht, wt, ld4, dtype=f32, device=dev)
            K.patchify_grad(f32, dout.contiguous(), B, ht, wt, p, m.out_channels, dtok32, ld4)
            K.channel_sum(f32, dtok32, B, Lt, K_out, ld4, out_c=gv(fl.bias))
        else:
            self._wgrad([Act(hf, ht, wt, H)], dtok, ldq, K.TAPS1, ht, wt, K_out, gv(fl.weight), dbias=gv(fl.bias))
        dhf, f32_out = self._ln_rows(g)
        self._conv([Act(dtok, ht, wt, K_out)], fl, K.TAPS1, ht, wt, H, out=dhf, packmode=L.PACK_DGRAD, out_f32=f32_out,
                   Kc=L.kc_for(K_out, dt))
        dx = torch.zeros(B, ht, wt, H, dtype=f32, device=dev)
        self._ln_bwd(g, m.final_layer.norm_final, dhf, x_fin, meanf, rstdf, self.ada_off[-1], dx, dmod, gv)
        publish(self.pub_final, False)

        # ---- blocks, last to first ----
        for r in reversed(tape[1:-1]):
            self._block_bwd(g, r, dx, dmod, gv)
            publish(self.pub_block[r.i], False)

        # ---- pos_embed and the patch conv (fp32): dx is the gradient of x0 = conv(x) + pos ----
        _, t, y, tf, A1, c, ye, _, xin = emb
        K.batch_sum(dx, B, Lt * H, gv(m.pos_embed))
        pe = m.x_embedder.proj
        dxin = None
        if x_requires_grad:
            dxin = torch.empty(B, m.in_channels, ht * p, wt * p, dtype=f32, device=dev)
            K.patch_dgrad(dx, H, pe.weight.detach(), B, ht, wt, p, m.in_channels, H, dxin)
        self._wgrad([xin], dx, H, self.patch_taps, ht, wt, H, gv(pe.weight), stride=p, dtype=f32, dbias=gv(pe.bias))
        # ---- stacked adaLN: mod = SiLU(c) W_ada^T + b ----
        Ta = self.ada_total
        dw_a = flat[self.ada_w_off:self.ada_w_off + Ta * H]
        self._wgrad([c], dmod, Ta, K.TAPS1, 1, 1, Ta, dw_a, pro=(L.PRO_SILU, None, None), dtype=f32,
                    dbias=flat[self.ada_b_off:self.ada_b_off + Ta])
        dc = torch.empty(B, 1, 1, H, dtype=f32, device=dev)
        self._conv([Act(dmod.view(B, 1, 1, Ta), 1, 1, Ta)], None, K.TAPS1, 1, 1, H, out=dc, dtype=f32,
                   w=self._ada_pack_dgrad(f32), Kc=L.kc_for(Ta, f32), silu_pre=c.t, ld_silu=H)
        # ---- timestep MLP and label embedding: c = Linear2(SiLU(Linear1(tf))) + label_emb ----
        te = m.t_embedder
        self._wgrad([A1], dc, H, K.TAPS1, 1, 1, H, gv(te.mlp[2].weight), pro=(L.PRO_SILU, None, None), dtype=f32,
                    dbias=gv(te.mlp[2].bias))
        de1 = torch.empty(B, 1, 1, H, dtype=f32, device=dev)
        self._conv([Act(dc, 1, 1, H)], te.mlp[2], K.TAPS1, 1, 1, H, out=de1, dtype=f32, packmode=L.PACK_DGRAD,
                   silu_pre=A1.t, ld_silu=H)
        self._wgrad([Act(tf, 1, 1, tf.shape[-1])], de1, H, K.TAPS1, 1, 1, H, gv(te.mlp[0].weight), dtype=f32,
                    dbias=gv(te.mlp[0].bias))
        if m.y_embedder is not None:
            tab = m.y_embedder.embedding_table.weight
            if ye is not None:
                K.embed_bwd(y, tab.shape[0], dc.view(B, H), gv(tab))
            else:
                gv(tab).zero_()
        publish(self.gtotal, True)
        grads = [self._gview(flat, q) for q in self.params]
        return dxin, grads


class DiTExecutor(TokenExecutor):
    name = "DiT"
    gelu_drop_epi = _GELU_DROP_EPI

    def __init__(self, model):
        self.in_proj = [_W(b.attn.in_proj_weight) for b in model.blocks]
        super().__init__(model, [b.adaLN_modulation[1] for b in model.blocks])

    def _final_params(self):
        fl = self.m.final_layer.linear
        return [fl.weight, fl.bias]

    def _block_params(self, b):
        return [b.mlp[3].weight, b.mlp[3].bias, b.mlp[0].weight, b.mlp[0].bias, b.attn.out_proj.weight,
                b.attn.out_proj.bias, b.attn.in_proj_weight, b.attn.in_proj_bias]

    def _block_parts(self, blk):
        return blk.norm1, blk.norm2, blk.mlp

    def _ln_kernel(self, norm):
        return K.ln_mod_fwd, ()

    def _ln_bwd(self, g, norm, dh, xs, mean, rstd, off_shift, dx, dmod, gv):
        H = self.H
        K.ln_mod_bwd(self.dt, dh, H, xs, mean, rstd, g.mod2, self.ada_total, off_shift + H, g.T, H, g.Lt, dx, dmod,
                     off_shift + H, off_shift)

    def _mixer_fwd(self, g, i, blk, h1):
        return self._attn_fwd(g, i, blk.attn, h1)

    def _block_bwd(self, g, r, dx, dmod, gv):
        i = r.i
        blk = self.blocks[i]
        dt = self.dt
        ht, wt, H = g.ht, g.wt, self.H
        mo_ = self.ada_off[i]
        Hm = blk.mlp[0].out_features
        # MLP branch: x_out = x_mid + gate_mlp * drop(mo)
        dmo = self._gate_bwd(g, dx, r.mo.t, mo_ + 5 * H, dmod, drop=r.d2)
        self._wgrad([r.a], dmo, H, K.TAPS1, ht, wt, H, gv(blk.mlp[3].weight), dbias=gv(blk.mlp[3].bias))
        du = self._rows(g, Hm)
        if _DGELU_EPI:
            # fc2's input gradient with the GELU (+ Dropout) backward in its epilogue (bitwise dmc_gelu_bwd)
            self._conv([Act(dmo, ht, wt, H)], blk.mlp[3], K.TAPS1, ht, wt, Hm, out=du, packmode=L.PACK_DGRAD,
                       act=L.ACT_DGELU, y_pre=r.u.t, drop=r.d1)
        else:
            da = self._rows(g, Hm)
            self._conv([Act(dmo, ht, wt, H)], blk.mlp[3], K.TAPS1, ht, wt, Hm, out=da, packmode=L.PACK_DGRAD)
            K.gelu_bwd(dt, da, r.u.t, g.T, Hm, Hm, du, drop=r.d1)
        self._wgrad([Act(r.h2, ht, wt, H)], du, Hm, K.TAPS1, ht, wt, Hm, gv(blk.mlp[0].weight),
                    dbias=gv(blk.mlp[0].bias))
        dh2 = self._rows(g, H)
        self._conv([Act(du, ht, wt, Hm)], blk.mlp[0], K.TAPS1, ht, wt, H, out=dh2, packmode=L.PACK_DGRAD)
        self._ln_bwd(g, blk.norm2, dh2, r.x_mid, r.mean2, r.rstd2, mo_ + 3 * H, dx, dmod, gv)
        # attention branch: x_mid = x_in + gate_msa * ao
        dao = self._gate_bwd(g, dx, r.ao.t, mo_ + 2 * H, dmod)
        dh1 = self._attn_bwd(g, i, blk.attn, r.h1, r.saved, r.d0, dao, gv)
        self._ln_bwd(g, blk.norm1, dh1, r.x_in, r.mean1, r.rstd1, mo_, dx, dmod, gv)


def dit_flops_per_image(model) -> float:
    """2*MACs of one DiT forward per image (linears, patch conv, attention matmuls; the per-sample conditioning
    GEMMs included)."""
    H = model.hidden_size
    Lt = model.h_tokens * model.w_tokens
    p = model.patch_size
    Hm = model.blocks[0].mlp[0].out_features
    f = 2.0 * Lt * (model.in_channels * p * p) * H
    per_block = 2.0 * Lt * (H * 3 * H + H * H + H * Hm + Hm * H) + 2 * 2.0 * Lt * Lt * H
    f += len(model.blocks) * per_block
    f += 2.0 * Lt * H * model.final_layer.linear.out_features
    te = model.t_embedder
    f += 2.0 * (te.mlp[0].in_features * H + H * H) + 2.0 * H * (6 * H * len(model.blocks) + 2 * H)
    return f
