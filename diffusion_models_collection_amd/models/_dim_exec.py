"""Executor of the DiM (models/dim.py of the reference, :94-346) on the gfx950 kernels, forward + backward.

The DiM is the DiT of _dit_exec.py with three differences, so this executor subclasses DiTExecutor (the stacked adaLN
packs, the dropout sites, the flat gradient buffer and its views are shared) and has its own forward / backward:

  * two adaLN heads of 3H rows per block (mamba_block, ff_block), each chunked (shift, scale, gate): stacked in that
    order they are the 6H rows per block of DiTExecutor's one adaLN GEMM, the final layer's 2H rows last;
  * affine LayerNorms (dmc_ln_affine_mod_fwd / bwd, gamma / beta gradients summed over the batch in a fixed order);
  * the token mixer: mamba_ssm.Mamba's recurrence (mixer="mamba") or the reference's nn.MultiheadAttention fallback
    with 8 heads (mixer="attention", the dmc_attn_* kernels as in the DiT).

Mamba mixer of block i on h = the modulated LayerNorm output [T, H] (E = 2H, R = dt_rank, N = 16, R8 = R rounded
up to 8):
  xz  = h in_proj^T                              [T, 2E]   (x | z)                 1x1 implicit GEMM
  u   = SiLU(causal depthwise conv4(x) + bias)   [T, E]                            dmc_causal_conv_silu_fwd
  dt_low = u x_proj[:R]^T                        [T, R8]   compute dtype, zero-padded (a ragged GEMM source next)
  Bm | Cm = u x_proj[R:]^T                       [T, 2N]   fp32 also in bf16 mode
  dpre = dt_low dt_proj^T                        [T, E]    fp32 also in bf16 mode (the bias is added inside the scan)
  y   = selective scan (softplus, recurrence, D skip, SiLU(z) gate)  [T, E]        dmc_selective_scan_fwd
  out = y out_proj^T                             [T, H]
The backward mirrors it: dmc_selective_scan_bwd recomputes the states chunk by chunk from the saved chunk-entry
states; every projection's gradients are the conv dgrad / wgrad kernels.
"""
import torch

from .. import _lib as L
from .. import kernels as K
from ._dit_exec import _GELU_EPI, DiTExecutor, _DiTFunction, _W
from ._unet_exec import Act, _PackCache, _seed_from_torch


class _Rows:
    """Rows [r0, r1) of a 2-D master weight as a pack-job source (resolved when the job array is built, so a moved
    parameter is followed)."""

    def __init__(self, w, r0, r1):
        self.w, self.r0, self.r1 = w, r0, r1

    def detach(self):
        return self.w.detach()[self.r0:self.r1]


class DiMExecutor(DiTExecutor):
    def __init__(self, model):
        self._bind_model(model)
        self.dt = model.compute_dtype
        self.cdt = L.dtype_code(self.dt)
        self.chunk = L.chunk_for(self.dt)
        self.wgen = 0
        self.packs = _PackCache(self)
        self.params = list(model.parameters())
        self.pindex = {id(p): i for i, p in enumerate(self.params)}
        self.training_grad_scale = 1.0
        self.grad_hook = None
        self.seed_ptr = None
        H = model.hidden_size
        self.H = H
        self.mixer = model.mixer
        self.blocks = list(model.blocks)
        if self.mixer == "attention":
            self.in_proj = [_W(b.mamba_block.mamba.in_proj_weight) for b in self.blocks]
        else:
            mm = self.blocks[0].mamba_block.mamba if self.blocks else None
            self.E = 2 * H
            self.N = model.state_size
            self.R = mm.dt_rank if mm is not None else (H + 15) // 16
            self.R8 = (self.R + 7) // 8 * 8
        self.ada = []
        for b in self.blocks:
            self.ada += [b.mamba_block.adaLN_modulation[1], b.ff_block.adaLN_modulation[1]]
        self.ada.append(model.final_layer.adaLN_modulation[1])
        self.ada_off = [6 * H * i for i in range(len(self.blocks))] + [6 * H * len(self.blocks)]
        self.ada_total = 6 * H * len(self.blocks) + 2 * H
        p = model.patch_size
        if p * p > 16:
            raise L.DMCError(f"DiM: patch size {p} (the implicit-GEMM conv takes at most 16 taps)")
        self.patch_taps = [(i, j) for i in range(p) for j in range(p)]
        self._layout_grads()

    # ---------------------------------------------------------------------------------------
    def _mixer_params(self, mb):
        mm = mb.mamba
        if self.mixer == "attention":
            return [mm.out_proj.weight, mm.out_proj.bias, mm.in_proj_weight, mm.in_proj_bias]
        return [mm.out_proj.weight, mm.A_log, mm.D, mm.dt_proj.weight, mm.dt_proj.bias, mm.x_proj.weight,
                mm.conv1d.weight, mm.conv1d.bias, mm.in_proj.weight]

    def _block_params(self, b):
        ff, mb = b.ff_block, b.mamba_block
        return ([ff.mlp[3].weight, ff.mlp[3].bias, ff.mlp[0].weight, ff.mlp[0].bias, ff.norm.weight, ff.norm.bias]
                + self._mixer_params(mb) + [mb.norm.weight, mb.norm.bias])

    def _layout_grads(self):
        """Flat gradient layout in backward-completion order (as DiTExecutor._layout_grads, with the LayerNorm
        affines behind the layer they precede)."""
        m = self.m
        fl = m.final_layer
        order = [fl.linear.weight, fl.linear.bias, fl.norm_final.weight, fl.norm_final.bias]
        for b in reversed(self.blocks):
            order += self._block_params(b)
        order += [m.pos_embed, m.x_embedder.proj.weight, m.x_embedder.proj.bias]
        order += [lin.weight for lin in self.ada] + [lin.bias for lin in self.ada]
        order += [m.t_embedder.mlp[2].weight, m.t_embedder.mlp[2].bias, m.t_embedder.mlp[0].weight,
                  m.t_embedder.mlp[0].bias]
        if m.y_embedder is not None:
            order.append(m.y_embedder.embedding_table.weight)
        assert len(order) == len(self.params) and {id(p) for p in order} == set(self.pindex), "DiM layout"
        self.order_ids = [id(p) for p in order]
        self.goff = [0] * len(self.params)
        off = 0
        for p in order:
            self.goff[self.pindex[id(p)]] = off
            off += p.numel()
        self.gtotal = off
        self.ada_w_off = self.goff[self.pindex[id(self.ada[0].weight)]]
        self.ada_b_off = self.goff[self.pindex[id(self.ada[0].bias)]]

    # ---- packs of the ragged Mamba projections (R and R + 2N are no multiples of the GEMM chunk) ----
    def _xproj_pack(self, i, which):
        """x_proj.weight [R + 2N, E] in the three forms its GEMMs take: "dt" the dt_low rows, zero-padded to R8
        output rows [R8][Kc(E)]; "bc" the Bm | Cm rows [2N][Kc(E)]; "dgrad" the input-gradient form [E][Kc(R8 + 2N)]
        over the virtual concat (d dt_low padded to R8 | dBm | dCm)."""
        w = self.blocks[i].mamba_block.mamba.x_proj.weight
        E, R, R8, N2 = self.E, self.R, self.R8, 2 * self.N
        if which == "dt":
            Kc = L.kc_for(E, self.dt)
            n = R8 * Kc
            jobs = lambda buf: [(_Rows(w, 0, R), buf, 0, L.PACK_FWD, R, E, 1, 1, Kc, -1)]                  # noqa: E731
        elif which == "bc":
            Kc = L.kc_for(E, self.dt)
            n = N2 * Kc
            jobs = lambda buf: [(_Rows(w, R, R + N2), buf, 0, L.PACK_FWD, N2, E, 1, 1, Kc, -1)]            # noqa: E731
        else:
            Kc = L.kc_for(R8 + N2, self.dt)
            n = E * Kc
            jobs = lambda buf: [(_Rows(w, 0, R), buf, 0, L.PACK_DGRAD, R, E, 1, 1, Kc, 0),                 # noqa: E731
                                (_Rows(w, R, R + N2), buf, 0, L.PACK_DGRAD, N2, E, 1, 1, Kc, R8)]
        return self.packs.get(("xproj", i, which, self.dt), (w,),
                              lambda: torch.zeros(n, dtype=self.dt, device=w.device), jobs)

    def _dtproj_pack_dgrad(self, i):
        """dt_proj.weight [E, R] for its input gradient, padded to R8 output rows (zeros)."""
        w = self.blocks[i].mamba_block.mamba.dt_proj.weight
        Kc = L.kc_for(self.E, self.dt)
        return self.packs.get(("dtproj_dg", i, self.dt), (w,),
                              lambda: torch.zeros(self.R8 * Kc, dtype=self.dt, device=w.device),
                              lambda buf: [(w, buf, 0, L.PACK_DGRAD, self.E, self.R, 1, 1, Kc, -1)])

    # =========================================================================================
    def run(self, x, t, y=None):
        params = self.params
        need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        if need_grad:
            return _DiTFunction.apply(self, x, t, y, *params)
        out, _ = self.forward(x, t, y, keep=False)
        return out

    def _mamba_fwd(self, i, h1, B, ht, wt):
        mm = self.blocks[i].mamba_block.mamba
        dt, dev, f32 = self.dt, self.device, torch.float32
        E, R, R8, N, H = self.E, self.R, self.R8, self.N, self.H
        Lt = ht * wt
        xz = self._new(B, ht, wt, 2 * E)
        self._conv([Act(h1, ht, wt, H)], mm.in_proj, K.TAPS1, ht, wt, 2 * E, out=xz.t)
        u = self._new(B, ht, wt, E)
        K.causal_conv_silu_fwd(dt, xz.t, 2 * E, mm.conv1d.weight, mm.conv1d.bias, B, Lt, E, u.t, E)
        # x_proj as two GEMMs over u: dt_low in the compute dtype (a GEMM operand next), Bm | Cm in fp32
        Kc = L.kc_for(E, dt)
        dtl = torch.empty(B, ht, wt, R8, dtype=dt, device=dev)
        self._conv([u], None, K.TAPS1, ht, wt, R8, out=dtl, w=self._xproj_pack(i, "dt"), Kc=Kc)
        bc = torch.empty(B, ht, wt, 2 * N, dtype=f32, device=dev)
        self._conv([u], None, K.TAPS1, ht, wt, 2 * N, out=bc, w=self._xproj_pack(i, "bc"), Kc=Kc, out_f32=True)
        dpre = torch.empty(B, ht, wt, E, dtype=f32, device=dev)
        self._conv([Act(dtl, ht, wt, R)], mm.dt_proj, K.TAPS1, ht, wt, E, out=dpre, out_f32=True)
        states = K.scan_states(B, Lt, E, N, dev)
        yg = self._new(B, ht, wt, E)
        K.selective_scan_fwd(dt, u.t, E, xz.t, 2 * E, E, dpre, E, bc, 2 * N, 0, N, mm.A_log, mm.D, mm.dt_proj.bias,
                             B, Lt, E, N, states, yg.t, E)
        ao = self._new(B, ht, wt, H)
        self._conv([yg], mm.out_proj, K.TAPS1, ht, wt, H, out=ao.t)
        return ao, (xz, u, dtl, bc, dpre, states, yg)

    def _mamba_bwd(self, i, h1, saved, dao, B, ht, wt, gv):
        """dao = the gradient of the mixer output [T, H] -> dh1; writes the mixer's parameter gradients."""
        mm = self.blocks[i].mamba_block.mamba
        xz, u, dtl, bc, dpre, states, yg = saved
        dt, dev = self.dt, dao.device
        E, R, R8, N, H = self.E, self.R, self.R8, self.N, self.H
        Lt = ht * wt
        new = lambda c: torch.empty(B, ht, wt, c, dtype=dt, device=dev)    # noqa: E731
        self._wgrad([yg], dao, H, K.TAPS1, ht, wt, H, gv(mm.out_proj.weight))
        dyg = new(E)
        self._conv([Act(dao, ht, wt, H)], mm.out_proj, K.TAPS1, ht, wt, E, out=dyg, packmode=L.PACK_DGRAD)
        du_s, dxz, ddpre, dbc, ddtl = new(E), new(2 * E), new(E), new(2 * N), new(R8)
        K.selective_scan_bwd(dt, dyg, E, u.t, E, xz.t, 2 * E, E, dpre, E, bc, 2 * N, 0, N, mm.A_log, mm.D,
                             mm.dt_proj.bias, B, Lt, E, N, states, du_s, E, dxz, 2 * E, E, ddpre, E, dbc, 2 * N, 0,
                             gv(mm.A_log), gv(mm.D))
        # dt_proj: dpre = dt_low W^T (+ bias inside the scan, so its gradient is the column sum of ddpre)
        self._wgrad([Act(dtl, ht, wt, R)], ddpre, E, K.TAPS1, ht, wt, E, gv(mm.dt_proj.weight),
                    dbias=gv(mm.dt_proj.bias))
        self._conv([Act(ddpre, ht, wt, E)], None, K.TAPS1, ht, wt, R8, out=ddtl, w=self._dtproj_pack_dgrad(i),
                   Kc=L.kc_for(E, dt))
        # x_proj: the dt_low rows and the Bm | Cm rows of its weight gradient are contiguous row blocks
        gx = gv(mm.x_proj.weight)
        self._wgrad([u], ddtl, R8, K.TAPS1, ht, wt, R, gx[:R])
        self._wgrad([u], dbc, 2 * N, K.TAPS1, ht, wt, 2 * N, gx[R:])
        du = new(E)
        self._conv([Act(ddtl, ht, wt, R8), Act(dbc, ht, wt, 2 * N)], None, K.TAPS1, ht, wt, E, out=du,
                   w=self._xproj_pack(i, "dgrad"), Kc=L.kc_for(R8 + 2 * N, dt), resid=du_s)
        K.causal_conv_silu_bwd(dt, du, E, xz.t, 2 * E, mm.conv1d.weight, mm.conv1d.bias, B, Lt, E, dxz, 2 * E,
                               gv(mm.conv1d.weight), gv(mm.conv1d.bias))
        self._wgrad([Act(h1, ht, wt, H)], dxz, 2 * E, K.TAPS1, ht, wt, 2 * E, gv(mm.in_proj.weight))
        dh1 = torch.empty(B, ht, wt, H, dtype=torch.float32, device=dev)
        self._conv([Act(dxz, ht, wt, 2 * E)], mm.in_proj, K.TAPS1, ht, wt, H, out=dh1, packmode=L.PACK_DGRAD,
                   out_f32=True)
        return dh1

    def forward(self, x, t, y, keep):
        m = self.m
        self.device = x.device
        self.packs.refresh()
        dt = self.dt
        f32 = torch.float32
        B, Cin, Hi, Wi = x.shape
        p = m.patch_size
        ht, wt = m.h_tokens, m.w_tokens
        Lt = ht * wt
        T = B * Lt
        H = self.H
        heads = m.num_heads
        hd = H // heads
        nb = len(self.blocks)
        x = x.contiguous().float()
        t = t.to(device=x.device, dtype=torch.long).contiguous()
        tape = [] if keep else None
        if m.training and m.dropout > 0:
            pd = float(m.dropout)
            self._drop_spec = (min(int(round(pd * 4294967296.0)), 4294967295), 1.0 / (1.0 - pd) if pd < 1 else 0.0)
            self._seed_base = 0 if self.seed_ptr is not None else _seed_from_torch()
        else:
            self._drop_spec = None

        # ---- conditioning: c = MLP(timestep embedding) (+ label embedding) (dim.py:326-336) ----
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
        mod2 = mod.view(B, self.ada_total)
        ldm = self.ada_total

        # ---- patch embedding (fp32) + pos_embed: the fp32 residual stream ----
        c4 = L.chunk_for(f32)
        xin = Act(K.pack_input(f32, x, (Cin + c4 - 1) // c4 * c4), Hi, Wi, Cin)
        x0 = torch.empty(B, ht, wt, H, dtype=f32, device=x.device)
        self._conv([xin], m.x_embedder.proj, self.patch_taps, ht, wt, H, stride=p, bias=m.x_embedder.proj.bias,
                   out=x0, dtype=f32)
        K.add_bcast(x0, m.pos_embed, B, Lt * H)
        if keep:
            tape.append(("embed", t, y, tf, A1, c, ye, mod, xin))

        def ln(norm, xs, br, off_gate, off_shift, off_scale, drop):
            """x_new = xs + gate * drop(br) (br given), then affine LN + modulation -> (x_new, h, mean, rstd)."""
            h = torch.empty(B, ht, wt, H, dtype=dt, device=x.device)
            mean = torch.empty(T, dtype=f32, device=x.device)
            rstd = torch.empty(T, dtype=f32, device=x.device)
            xo = None
            if br is not None:
                xo = torch.empty(B, ht, wt, H, dtype=f32, device=x.device)
            K.ln_affine_mod_fwd(dt, xs, T, H, Lt, mod2, ldm, off_shift, off_scale, 1e-6, norm.weight, norm.bias, h, H,
                                mean, rstd, br=br, ld_br=H, off_gate=off_gate, drop=drop, x_out=xo)
            return (xo if xo is not None else xs), h, mean, rstd

        xcur = x0
        pend = None            # (mo, gate offset, drop) of the previous block's MLP branch, not yet added
        for i, blk in enumerate(self.blocks):
            mb, ff = blk.mamba_block, blk.ff_block
            mo_ = self.ada_off[i]
            if pend is None:
                x_in, h1, mean1, rstd1 = ln(mb.norm, xcur, None, 0, mo_, mo_ + H, None)
            else:
                x_in, h1, mean1, rstd1 = ln(mb.norm, xcur, pend[0], pend[1], mo_, mo_ + H, pend[2])
            d0 = None
            if self.mixer == "attention":
                at = mb.mamba
                qkv = self._new(B, ht, wt, 3 * H)
                self._conv([Act(h1, ht, wt, H)], self.in_proj[i], K.TAPS1, ht, wt, 3 * H, bias=at.in_proj_bias,
                           out=qkv.t)
                o = self._new(B, ht, wt, H)
                lse = torch.empty(B * heads * Lt, dtype=f32, device=x.device)
                d0 = self._drop(2 * nb + i)      # attention-probability dropout (MHA dropout=p)
                K.attn_fwd(dt, qkv.t, 3 * H, B, Lt, heads, hd, o.t, H, lse, drop=d0)
                ao = self._new(B, ht, wt, H)
                self._conv([o], at.out_proj, K.TAPS1, ht, wt, H, bias=at.out_proj.bias, out=ao.t)
                saved = (qkv, o, lse)
            else:
                ao, saved = self._mamba_fwd(i, h1, B, ht, wt)
            x_mid, h2, mean2, rstd2 = ln(ff.norm, x_in, ao.t, mo_ + 2 * H, mo_ + 3 * H, mo_ + 4 * H, None)
            Hm = ff.mlp[0].out_features
            d1 = self._drop(2 * i)
            a = self._new(B, ht, wt, Hm)
            u = self._new(B, ht, wt, Hm) if keep or d1 is not None else None
            if d1 is None and _GELU_EPI:
                # GELU in fc1's epilogue; the pre-activation is stored only when the backward needs it
                self._conv([Act(h2, ht, wt, H)], ff.mlp[0], K.TAPS1, ht, wt, Hm, bias=ff.mlp[0].bias, out=a.t,
                           act=L.ACT_GELU, y_pre=None if u is None else u.t)
            else:
                ub = u.t if u is not None else a.t
                self._conv([Act(h2, ht, wt, H)], ff.mlp[0], K.TAPS1, ht, wt, Hm, bias=ff.mlp[0].bias, out=ub)
                K.gelu_fwd(dt, ub, T, Hm, Hm, a.t, drop=d1)
            mo = self._new(B, ht, wt, H)
            self._conv([a], ff.mlp[3], K.TAPS1, ht, wt, H, bias=ff.mlp[3].bias, out=mo.t)
            d2 = self._drop(2 * i + 1)
            if keep:
                tape.append(("block", i, x_in, h1, mean1, rstd1, saved, ao, x_mid, h2, mean2, rstd2, u, a, mo, d1, d2,
                             d0))
            xcur = x_mid
            pend = (mo.t, mo_ + 5 * H, d2)
        # ---- final layer ----
        fo = self.ada_off[-1]
        nf = m.final_layer.norm_final
        if pend is None:
            x_fin, hf, meanf, rstdf = ln(nf, xcur, None, 0, fo, fo + H, None)
        else:
            x_fin, hf, meanf, rstdf = ln(nf, xcur, pend[0], pend[1], fo, fo + H, pend[2])
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

    # =========================================================================================
    def backward(self, tape, dout, x_requires_grad):
        m = self.m
        dt = self.dt
        f32 = torch.float32
        flat = getattr(self, "_flat", None)
        if flat is None or flat.device != dout.device or any(p.grad is not None for p in self.params):
            flat = torch.empty(self.gtotal, dtype=f32, device=dout.device)
        self._flat = flat
        self.flat = flat
        gv = lambda p: self._gview(flat, p)  # noqa: E731
        B = dout.shape[0]
        p = m.patch_size
        ht, wt = m.h_tokens, m.w_tokens
        Lt = ht * wt
        T = B * Lt
        H = self.H
        heads = m.num_heads
        hd = H // heads
        dev = dout.device
        emb = tape[0]
        mod = emb[7]
        mod2 = mod.view(B, self.ada_total)
        ldm = self.ada_total
        dmod = torch.empty(B, self.ada_total, dtype=f32, device=dev)
        hook = self.grad_hook
        pos = [0]

        def publish(final):
            if hook is None:
                return
            hook(flat, pos[0], final)

        def ln_bwd(norm, dh, xs, mean, rstd, off_scale, off_shift):
            # dh rows are fp32 also in bf16 mode (their GEMMs store fp32): the modulation and LayerNorm-affine
            # gradients are sums of them over all tokens
            K.ln_affine_mod_bwd(f32, dh, H, xs, mean, rstd, mod2, ldm, off_scale, T, H, Lt, norm.weight, norm.bias, dx,
                                dmod, off_scale, off_shift, gv(norm.weight), gv(norm.bias))

        # ---- final layer ----
        _, x_fin, hf, meanf, rstdf, ldo = tape[-1]
        fl = m.final_layer.linear
        nf = m.final_layer.norm_final
        K_out = fl.out_features
        ldq = (K_out + self.chunk - 1) // self.chunk * self.chunk
        dtok = torch.empty(B, ht, wt, ldq, dtype=dt, device=dev)
        K.patchify_grad(dt, dout.contiguous(), B, ht, wt, p, m.out_channels, dtok, ldq)
        if dt == f32:
            self._wgrad([Act(hf, ht, wt, H)], dtok, ldq, K.TAPS1, ht, wt, K_out, gv(fl.weight), dbias=gv(fl.bias))
        else:
            # the output bias gradient is a plain sum of the fp32 cotangent: not taken from its bf16 copy
            self._wgrad([Act(hf, ht, wt, H)], dtok, ldq, K.TAPS1, ht, wt, K_out, gv(fl.weight))
            ld4 = (K_out + 3) // 4 * 4
            dtok32 = torch.empty(B, ht, wt, ld4, dtype=f32, device=dev)
            K.patchify_grad(f32, dout.contiguous(), B, ht, wt, p, m.out_channels, dtok32, ld4)
            K.channel_sum(f32, dtok32, B, Lt, K_out, ld4, out_c=gv(fl.bias))
        dhf = torch.empty(B, ht, wt, H, dtype=f32, device=dev)
        self._conv([Act(dtok, ht, wt, K_out)], fl, K.TAPS1, ht, wt, H, out=dhf, packmode=L.PACK_DGRAD, out_f32=True,
                   Kc=L.kc_for(K_out, dt))
        dx = torch.zeros(B, ht, wt, H, dtype=f32, device=dev)
        fo = self.ada_off[-1]
        ln_bwd(nf, dhf, x_fin, meanf, rstdf, fo + H, fo)
        pos[0] = self.goff[self.pindex[id(nf.bias)]] + nf.bias.numel()
        publish(False)

        # ---- blocks, last to first ----
        for rec in reversed(tape[1:-1]):
            (_, i, x_in, h1, mean1, rstd1, saved, ao, x_mid, h2, mean2, rstd2, u, a, mo, d1, d2, d0) = rec
            blk = self.blocks[i]
            mb, ff = blk.mamba_block, blk.ff_block
            mo_ = self.ada_off[i]
            Hm = ff.mlp[0].out_features
            # feed-forward branch: x_out = x_mid + gate_ff * drop(mo)
            dmo = torch.empty(B, ht, wt, H, dtype=dt, device=dev)
            # (the bias gradient of the branch's last Linear comes from the fp32 stream gradient, not the stored dmo)
            K.gate_bwd_bias(dt, dx, mo.t, H, mod2, ldm, mo_ + 5 * H, T, H, Lt, dmo, H, dmod, mo_ + 5 * H,
                            gv(ff.mlp[3].bias), drop=d2)
            self._wgrad([a], dmo, H, K.TAPS1, ht, wt, H, gv(ff.mlp[3].weight))
            du = torch.empty(B, ht, wt, Hm, dtype=dt, device=dev)
            da = torch.empty(B, ht, wt, Hm, dtype=f32, device=dev)
            self._conv([Act(dmo, ht, wt, H)], ff.mlp[3], K.TAPS1, ht, wt, Hm, out=da, packmode=L.PACK_DGRAD,
                       out_f32=True)
            K.gelu_bwd_f32in(dt, da, u.t, T, Hm, Hm, du, drop=d1)
            self._wgrad([Act(h2, ht, wt, H)], du, Hm, K.TAPS1, ht, wt, Hm, gv(ff.mlp[0].weight),
                        dbias=gv(ff.mlp[0].bias))
            dh2 = torch.empty(B, ht, wt, H, dtype=f32, device=dev)
            self._conv([Act(du, ht, wt, Hm)], ff.mlp[0], K.TAPS1, ht, wt, H, out=dh2, packmode=L.PACK_DGRAD,
                       out_f32=True)
            ln_bwd(ff.norm, dh2, x_mid, mean2, rstd2, mo_ + 4 * H, mo_ + 3 * H)
            # mixer branch: x_mid = x_in + gate_mixer * ao
            dao = torch.empty(B, ht, wt, H, dtype=dt, device=dev)
            if self.mixer == "attention":
                qkv, o, lse = saved
                at = mb.mamba
                op = at.out_proj
                K.gate_bwd_bias(dt, dx, ao.t, H, mod2, ldm, mo_ + 2 * H, T, H, Lt, dao, H, dmod, mo_ + 2 * H,
                                gv(op.bias))
                self._wgrad([o], dao, H, K.TAPS1, ht, wt, H, gv(op.weight))
                do = torch.empty(B, ht, wt, H, dtype=dt, device=dev)
                self._conv([Act(dao, ht, wt, H)], op, K.TAPS1, ht, wt, H, out=do, packmode=L.PACK_DGRAD)
                dqkv = torch.empty(B, ht, wt, 3 * H, dtype=dt, device=dev)
                K.attn_bwd(dt, qkv.t, 3 * H, o.t, do, H, lse, B, Lt, heads, hd, dqkv, 3 * H, drop=d0)
                self._wgrad([Act(h1, ht, wt, H)], dqkv, 3 * H, K.TAPS1, ht, wt, 3 * H, gv(at.in_proj_weight),
                            dbias=gv(at.in_proj_bias))
                dh1 = torch.empty(B, ht, wt, H, dtype=f32, device=dev)
                self._conv([Act(dqkv, ht, wt, 3 * H)], self.in_proj[i], K.TAPS1, ht, wt, H, out=dh1,
                           packmode=L.PACK_DGRAD, out_f32=True)
            else:
                K.gate_bwd(dt, dx, ao.t, H, mod2, ldm, mo_ + 2 * H, T, H, Lt, dao, H, dmod, mo_ + 2 * H)
                dh1 = self._mamba_bwd(i, h1, saved, dao, B, ht, wt, gv)
            ln_bwd(mb.norm, dh1, x_in, mean1, rstd1, mo_ + H, mo_)
            pos[0] = self.goff[self.pindex[id(mb.norm.bias)]] + mb.norm.bias.numel()
            publish(False)

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
        pos[0] = self.gtotal
        publish(True)
        grads = [self._gview(flat, q) for q in self.params]
        return dxin, grads


def dim_flops_per_image(model) -> float:
    """2*MACs of one DiM forward per image (linears, patch conv, the mixer; the conditioning GEMMs included)."""
    H = model.hidden_size
    Lt = model.h_tokens * model.w_tokens
    p = model.patch_size
    nb = len(model.blocks)
    Hm = model.blocks[0].ff_block.mlp[0].out_features if nb else 0
    f = 2.0 * Lt * (model.in_channels * p * p) * H
    if model.mixer == "attention":
        mix = 2.0 * Lt * (H * 3 * H + H * H) + 2 * 2.0 * Lt * Lt * H
    else:
        E, N = 2 * H, model.state_size
        R = (H + 15) // 16
        mix = 2.0 * Lt * (H * 2 * E + E * (R + 2 * N) + R * E + E * H) + Lt * E * (8.0 + 6.0 * N)
    f += nb * (mix + 2.0 * Lt * 2 * H * Hm)
    f += 2.0 * Lt * H * model.final_layer.linear.out_features
    te = model.t_embedder
    f += 2.0 * (te.mlp[0].in_features * H + H * H) + 2.0 * H * (6 * H * nb + 2 * H)
    return f
