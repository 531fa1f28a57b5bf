"""Executor of the DiM (models/dim.py of the reference, :94-346) on the gfx950 kernels, forward + backward.

The DiM is the DiT of _dit_exec.py with three differences. DiMExecutor is a TokenExecutor like DiTExecutor: the
conditioning, the patch embedding, the block forward (LayerNorm, mixer, LayerNorm, MLP, with the dropout sites), the
attention mixer, the final layer, the backward around the blocks and the flat gradient layout are TokenExecutor's. Here
are the parameter order, the Mamba mixer, the block backward and what the differences need:

  * two adaLN heads of 3H rows per block (mamba_block, ff_block), each chunked (shift, scale, gate): stacked in that
    order they are the 6H rows per block of TokenExecutor's one adaLN GEMM, the final layer's 2H rows last;
  * affine LayerNorms (dmc_ln_affine_mod_fwd / bwd, gamma / beta gradients summed over the batch in a fixed order);
    their backward and every other sum over tokens reads fp32 rows also in bf16 mode (TokenExecutor.f32_sums);
  * the token mixer: mamba_ssm.Mamba's recurrence (mixer="mamba") or the reference's nn.MultiheadAttention fallback
    with 8 heads (mixer="attention", TokenExecutor's attention mixer).

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

Scan orders (model.scan_orders, one 3-bit code per block): the conv and the scan are the only two ops that know the
token order, so a block with a non-zero code calls their _ord entry points with (ht, wt, code) and everything else,
every buffer included, is as for code 0. A block with code 0 calls exactly what it called before there were orders.
"""
import torch

from .. import _lib as L
from .. import kernels as K
from ._dit_exec import TokenExecutor, _W
from ._unet_exec import Act


class _Rows:
    """Rows [r0, r1) of a 2-D master weight as a pack-job source (resolved when the job array is built, so a moved
    parameter is followed)."""

    def __init__(self, w, r0, r1):
        self.w, self.r0, self.r1 = w, r0, r1

    def detach(self):
        return self.w.detach()[self.r0:self.r1]


class DiMExecutor(TokenExecutor):
    name = "DiM"
    f32_sums = True

    def __init__(self, model):
        H = model.hidden_size
        self.mixer = model.mixer
        self.scan_orders = tuple(getattr(model, "scan_orders", ())) or (0,) * len(model.blocks)
        if self.mixer == "attention":
            self.in_proj = [_W(b.mamba_block.mamba.in_proj_weight) for b in model.blocks]
        else:
            mm = model.blocks[0].mamba_block.mamba if len(model.blocks) else None
            self.E = 2 * H
            self.N = model.state_size
            self.R = mm.dt_rank if mm is not None else (H + 15) // 16
            self.R8 = (self.R + 7) // 8 * 8
        ada = []
        for b in model.blocks:
            ada += [b.mamba_block.adaLN_modulation[1], b.ff_block.adaLN_modulation[1]]
        super().__init__(model, ada)

    # ---------------------------------------------------------------------------------------
    def _final_params(self):
        fl = self.m.final_layer
        return [fl.linear.weight, fl.linear.bias, fl.norm_final.weight, fl.norm_final.bias]

    def _mixer_params(self, mb):
        mm = mb.mamba
        if self.mixer == "attention":
            return [mm.out_proj.weight, mm.out_proj.bias, mm.in_proj_weight, mm.in_proj_bias]
        return [mm.out_proj.weight, mm.A_log, mm.D, mm.dt_proj.weight, mm.dt_proj.bias, mm.x_proj.weight,
                mm.conv1d.weight, mm.conv1d.bias, mm.in_proj.weight]

    def _block_params(self, b):
        """The LayerNorm affines come behind the layer they precede."""
        ff, mb = b.ff_block, b.mamba_block
        return ([ff.mlp[3].weight, ff.mlp[3].bias, ff.mlp[0].weight, ff.mlp[0].bias, ff.norm.weight, ff.norm.bias]
                + self._mixer_params(mb) + [mb.norm.weight, mb.norm.bias])

    def _block_parts(self, blk):
        return blk.mamba_block.norm, blk.ff_block.norm, blk.ff_block.mlp

    def _ln_kernel(self, norm):
        return K.ln_affine_mod_fwd, (norm.weight, norm.bias)

    def _ln_bwd(self, g, norm, dh, xs, mean, rstd, off_shift, dx, dmod, gv):
        # dh rows are fp32 also in bf16 mode (their GEMMs store fp32): the modulation and LayerNorm-affine
        # gradients are sums of them over all tokens
        H = self.H
        K.ln_affine_mod_bwd(torch.float32, dh, H, xs, mean, rstd, g.mod2, self.ada_total, off_shift + H, g.T, H, g.Lt,
                            norm.weight, norm.bias, dx, dmod, off_shift + H, off_shift, gv(norm.weight), gv(norm.bias))

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

    def _mamba_fwd(self, i, h1, B, ht, wt):
        mm = self.blocks[i].mamba_block.mamba
        dt, dev, f32 = self.dt, self.device, torch.float32
        E, R, R8, N, H = self.E, self.R, self.R8, self.N, self.H
        Lt = ht * wt
        xz = self._new(B, ht, wt, 2 * E)
        self._conv([Act(h1, ht, wt, H)], mm.in_proj, K.TAPS1, ht, wt, 2 * E, out=xz.t)
        u = self._new(B, ht, wt, E)
        code = self.scan_orders[i]
        if code:
            K.causal_conv_silu_fwd_ord(dt, xz.t, 2 * E, mm.conv1d.weight, mm.conv1d.bias, B, ht, wt, code, E, u.t, E)
        else:
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
        if code:
            K.selective_scan_fwd_ord(dt, u.t, E, xz.t, 2 * E, E, dpre, E, bc, 2 * N, 0, N, mm.A_log, mm.D,
                                     mm.dt_proj.bias, B, ht, wt, code, E, N, states, yg.t, E)
        else:
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
        code = self.scan_orders[i]
        if code:
            K.selective_scan_bwd_ord(dt, dyg, E, u.t, E, xz.t, 2 * E, E, dpre, E, bc, 2 * N, 0, N, mm.A_log, mm.D,
                                     mm.dt_proj.bias, B, ht, wt, code, E, N, states, du_s, E, dxz, 2 * E, E, ddpre, E,
                                     dbc, 2 * N, 0, gv(mm.A_log), gv(mm.D))
        else:
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
        if code:
            K.causal_conv_silu_bwd_ord(dt, du, E, xz.t, 2 * E, mm.conv1d.weight, mm.conv1d.bias, B, ht, wt, code, E, dxz,
                                       2 * E, gv(mm.conv1d.weight), gv(mm.conv1d.bias))
        else:
            K.causal_conv_silu_bwd(dt, du, E, xz.t, 2 * E, mm.conv1d.weight, mm.conv1d.bias, B, Lt, E, dxz, 2 * E,
                                   gv(mm.conv1d.weight), gv(mm.conv1d.bias))
        self._wgrad([Act(h1, ht, wt, H)], dxz, 2 * E, K.TAPS1, ht, wt, 2 * E, gv(mm.in_proj.weight))
        dh1 = torch.empty(B, ht, wt, H, dtype=torch.float32, device=dev)
        self._conv([Act(dxz, ht, wt, 2 * E)], mm.in_proj, K.TAPS1, ht, wt, H, out=dh1, packmode=L.PACK_DGRAD,
                   out_f32=True)
        return dh1

    def _mixer_fwd(self, g, i, blk, h1):
        if self.mixer == "attention":
            return self._attn_fwd(g, i, blk.mamba_block.mamba, h1)
        ao, saved = self._mamba_fwd(i, h1, g.B, g.ht, g.wt)
        return ao, saved, None

    def _block_bwd(self, g, r, dx, dmod, gv):
        i = r.i
        blk = self.blocks[i]
        mb, ff = blk.mamba_block, blk.ff_block
        dt = self.dt
        ht, wt, H = g.ht, g.wt, self.H
        mo_ = self.ada_off[i]
        Hm = ff.mlp[0].out_features
        # feed-forward branch: x_out = x_mid + gate_ff * drop(mo)
        # (the bias gradient of the branch's last Linear comes from the fp32 stream gradient, not the stored dmo)
        dmo = self._gate_bwd(g, dx, r.mo.t, mo_ + 5 * H, dmod, drop=r.d2, dbias=gv(ff.mlp[3].bias))
        self._wgrad([r.a], dmo, H, K.TAPS1, ht, wt, H, gv(ff.mlp[3].weight))
        du = self._rows(g, Hm)
        da = self._rows(g, Hm, torch.float32)
        self._conv([Act(dmo, ht, wt, H)], ff.mlp[3], K.TAPS1, ht, wt, Hm, out=da, packmode=L.PACK_DGRAD,
                   out_f32=True)
        K.gelu_bwd_f32in(dt, da, r.u.t, g.T, Hm, Hm, du, drop=r.d1)
        self._wgrad([Act(r.h2, ht, wt, H)], du, Hm, K.TAPS1, ht, wt, Hm, gv(ff.mlp[0].weight),
                    dbias=gv(ff.mlp[0].bias))
        dh2, f32_out = self._ln_rows(g)
        self._conv([Act(du, ht, wt, Hm)], ff.mlp[0], K.TAPS1, ht, wt, H, out=dh2, packmode=L.PACK_DGRAD,
                   out_f32=f32_out)
        self._ln_bwd(g, ff.norm, dh2, r.x_mid, r.mean2, r.rstd2, mo_ + 3 * H, dx, dmod, gv)
        # mixer branch: x_mid = x_in + gate_mixer * ao
        if self.mixer == "attention":
            at = mb.mamba
            dao = self._gate_bwd(g, dx, r.ao.t, mo_ + 2 * H, dmod, dbias=gv(at.out_proj.bias))
            dh1 = self._attn_bwd(g, i, at, r.h1, r.saved, r.d0, dao, gv)
        else:
            dao = self._gate_bwd(g, dx, r.ao.t, mo_ + 2 * H, dmod)
            dh1 = self._mamba_bwd(i, r.h1, r.saved, dao, g.B, ht, wt, gv)
        self._ln_bwd(g, mb.norm, dh1, r.x_in, r.mean1, r.rstd1, mo_, dx, dmod, gv)


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
