"""Plain-torch restatement of dmc_conv_desc (include/dmc.h) for tests/test_gpu_conv_kernels.py: the convolution, its
weight gradient and its GroupNorm partials, each in three evaluations of the same formulas --

  mode "f64"   the reference: float64 throughout, no rounding;
  mode "yard"  the yardstick: fp32 throughout, and for bf16 exactly the roundings the format forces: the operands (the
               callers pass bf16-representable values), the prologue output before the MFMA, the stored output, and a
               stored bf16 y_pre (the activation is taken of that stored value, as the header defines it);
  mode "abs"   the floor's input: float64 on absolute values, so that every output element is the sum of the
               magnitudes of its terms.

It restates the descriptor, not the kernels: one gather per tap over the prologue-transformed virtual concat, a matrix
product per tap, the epilogue in the header's order. Nothing here knows of tiles, splits or families.

A spec is a plain dict (see `conv`); tensors are CPU, NHWC, without pitches (the test's launch() adds those).
"""
import math

import numpy as np
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
MODE_NORMAL, MODE_UPSAMPLE, MODE_DILATE = 0, 1, 2
PRO_NONE, PRO_AFFINE_SILU, PRO_SILU, PRO_AFFINE, PRO_GN_SILU = 0, 1, 2, 3, 4
ACT_NONE, ACT_GELU, ACT_GELU_DROP, ACT_DGELU = 0, 1, 2, 3
K_MARGIN = {F32: 4.0, BF16: 2.0}
NAME = {F32: "fp32", BF16: "bf16"}
GELU_LIPSCHITZ = 1.13   # max |gelu'| = 1.1289 (at u = sqrt(2) * 1.0 ...): |gelu(a) - gelu(b)| <= 1.13 |a - b|


def _work(mode):
    return F32 if mode == "yard" else F64


def _rnd(t, dt, mode):
    """the rounding a tensor stored (or fed to the MFMA) in dt forces on the yardstick; none on the other two"""
    return t.to(BF16).to(F32) if (mode == "yard" and dt == BF16) else t


def silu(t):
    return t * torch.sigmoid(t)


def silu_grad(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def gelu(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def keep_mask(shape_rows, ld, C, seed, thresh):
    """dropout keep mask [rows, C] over element index row * ld + c (drop_keep_np of test_gpu_kernels.py)"""
    from test_gpu_kernels import drop_keep_np
    idx = (np.arange(shape_rows, dtype=np.int64)[:, None] * ld + np.arange(C, dtype=np.int64)[None, :])
    return torch.from_numpy(drop_keep_np(idx.reshape(-1), seed, thresh).reshape(shape_rows, C).astype(np.float64))


def source(s, mode):
    """The prologue-transformed virtual concat [N, H, W, C1 + C2] (what the taps gather; padding is added later, so the
    prologue is never applied to it)."""
    wt, dt = _work(mode), s["dt"]
    x = s["x1"][..., :s["C1"]]
    if s["C2"]:
        x = torch.cat([x, s["x2"][..., :s["C2"]]], -1)
    x = x.to(wt)
    pro = s.get("pro", PRO_NONE)
    N, H, W, C = x.shape
    if pro == PRO_NONE:
        return x.abs() if mode == "abs" else x
    if pro in (PRO_AFFINE_SILU, PRO_AFFINE):
        a = x * s["pro_scale"].to(wt)[:, None, None, :C] + s["pro_shift"].to(wt)[:, None, None, :C]
        if pro == PRO_AFFINE_SILU:
            a = silu(a)
    elif pro == PRO_SILU:
        a = silu(x)
    else:   # PRO_GN_SILU: GroupNorm over the image's (H W C / G) groups, gamma / beta in pro_scale / pro_shift [C]
        G = s["pro_groups"]
        v = x.reshape(N, H * W, G, C // G)
        mean = v.mean(dim=(1, 3), keepdim=True)
        var = ((v - mean) ** 2).mean(dim=(1, 3), keepdim=True)
        a = ((v - mean) * torch.rsqrt(var + s["pro_eps"])).reshape(N, H, W, C)
        a = silu(a * s["pro_scale"].to(wt) + s["pro_shift"].to(wt))
    if s.get("drop"):
        seed, thresh, scale = s["drop"]
        keep = keep_mask(N * H * W, s["drop_ld"], C, seed, thresh).reshape(N, H, W, C).to(wt)
        a = a * keep * float(np.float32(scale))
    a = _rnd(a, dt, mode)
    return a.abs() if mode == "abs" else a


def tap_index(s, t):
    """(iy [OH], valid_y [OH], ix [OW], valid_x [OW]) of tap t: the header's coordinate rule, per axis."""
    out = []
    for o_n, src_n, off in ((s["OH"], s["H"], s["taps"][t][0]), (s["OW"], s["W"], s["taps"][t][1])):
        i = torch.arange(o_n) * s.get("stride", 1) + off
        m = s.get("mode", MODE_NORMAL)
        if m == MODE_UPSAMPLE:
            ok = (i >= 0) & (i < 2 * src_n)
            i = i >> 1
        elif m == MODE_DILATE:
            ok = (i >= 0) & (i % 2 == 0) & (i // 2 < src_n)
            i = i // 2
        else:
            ok = (i >= 0) & (i < src_n)
        out += [i.clamp(0, src_n - 1), ok]
    return out


def gather(s, a, t):
    """[N, OH, OW, C]: the source under tap t, zero where the tap falls into the padding"""
    iy, oky, ix, okx = tap_index(s, t)
    g = a[:, iy][:, :, ix]
    return g * (oky[:, None] & okx[None, :]).to(a.dtype)[None, :, :, None]


def conv(s, mode="f64", defect=None):
    """dmc_conv2d of spec s. Keys: dt (storage dtype), N H W C1 C2 OH OW Cout, taps [(dy, dx)], mode, stride, x1 x2
    [N, H, W, C], w [Cout, C1 + C2, ntaps], pro / pro_scale / pro_shift / pro_groups / pro_eps / drop (seed, thresh,
    scale) / drop_ld, bias [Cout], addvec [N, Cout], resid [N, OH, OW, Cout], silu_pre [N, OH, OW, Cout], Csplit, out_f32,
    out_nchw, act, y_pre (DGELU: the stored pre-activation, an input). Returns dict(y1, y2, y_pre) of [N, OH, OW, c]
    tensors (y1 NCHW with out_nchw), y2 / y_pre None where the descriptor has none.

    out = (acc + bias + addvec) * silu'(silu_pre) + resid, then act, then the split: the header puts the residual behind
    the silu' factor (an accumulated gradient is not scaled by this layer's SiLU backward).

    defect: the planted defects of test_planted_defects_are_rejected, applied inside the yardstick."""
    wt, dt = _work(mode), s["dt"]
    odt = F32 if (s.get("out_f32") or s.get("out_nchw")) else dt
    a = source(s, mode)
    w = s["w"].to(wt)
    if mode == "abs":
        w = w.abs()
    N, OH, OW, Cout = s["N"], s["OH"], s["OW"], s["Cout"]
    acc = torch.zeros(N * OH * OW, Cout, dtype=wt)
    for t in range(len(s["taps"])):
        g = gather(s, a, t)
        wt_t = w[:, :, t]
        if defect and defect[0] == "drop_product" and t == defect[1]:
            wt_t = wt_t.clone()
            wt_t[:, defect[2]] = 0
        if defect and defect[0] == "edge_tap" and t == defect[1]:   # the left image edge reads its neighbour, not zero
            iy, oky, ix, okx = tap_index(s, t)
            g = g.clone()
            g[:, :, 0] = a[:, iy][:, :, 1] * oky.to(a.dtype)[None, :, None]
        part = g.reshape(-1, g.shape[-1]) @ wt_t.t()
        if defect and defect[0] == "bf16_partial" and t == defect[1]:
            part = part.to(BF16).to(wt)
        acc += part
    v = acc.reshape(N, OH, OW, Cout)
    ab = (lambda z: z.abs()) if mode == "abs" else (lambda z: z)
    if s.get("bias") is not None:
        v = v + ab(s["bias"].to(wt))
    if s.get("addvec") is not None:
        v = v + ab(s["addvec"].to(wt))[:, None, None, :Cout]
    if s.get("silu_pre") is not None:
        v = v * ab(silu_grad(s["silu_pre"].to(wt)))
    if s.get("resid") is not None and not (defect and defect[0] == "resid_after_store"):
        v = v + ab(s["resid"].to(wt))
    act, y_pre = s.get("act", ACT_NONE), None
    if act in (ACT_GELU, ACT_GELU_DROP):
        y_pre = _rnd(v, odt, mode)
        v = GELU_LIPSCHITZ * y_pre if mode == "abs" else gelu(y_pre)
        if act == ACT_GELU_DROP and s.get("drop"):
            seed, thresh, scale = s["drop"]
            keep = keep_mask(N * OH * OW, Cout, Cout, seed, thresh).reshape(N, OH, OW, Cout).to(wt)
            v = v * keep * float(np.float32(scale))
    elif act == ACT_DGELU:
        m = torch.ones((), dtype=wt)
        if s.get("drop"):
            seed, thresh, scale = s["drop"]
            m = keep_mask(N * OH * OW, Cout, Cout, seed, thresh).reshape(N, OH, OW, Cout).to(wt) * float(np.float32(scale))
        v = _rnd(v, odt, mode) * m * ab(gelu_grad(s["y_pre"].to(wt)))
    v = _rnd(v, odt, mode)
    if defect and defect[0] == "resid_after_store":
        v = _rnd(v + s["resid"].to(wt), odt, mode)
    cs = s.get("Csplit", Cout)
    y1, y2 = v[..., :cs], (v[..., cs:] if cs < Cout else None)
    if s.get("out_nchw"):
        y1 = y1.permute(0, 3, 1, 2).contiguous()
    return dict(y1=y1, y2=y2, y_pre=y_pre)


def wgrad(s, dy, scale, mode="f64", defect=None):
    """dw [Cout, C, ntaps] = scale * sum_pix dy[pix, co] * prologue(x)[coord(pix, t), c] and dbias [Cout] = scale *
    sum_pix dy. dy [N, OH, OW, Cout]."""
    wt = _work(mode)
    a = source(s, mode)
    g = dy.to(wt).reshape(-1, s["Cout"])
    if mode == "abs":
        g = g.abs()
    if defect and defect[0] == "drop_pixel":
        g = g.clone()
        g[defect[1]] = 0
    sc = abs(float(np.float32(scale)))if mode == "abs" else float(np.float32(scale))
    dw = torch.stack([g.t() @ gather(s, a, t).reshape(g.shape[0], -1) for t in range(len(s["taps"]))], -1) * sc
    return dict(dw=dw, dbias=g.sum(0) * sc)


def gn_partials(y1, mode="f64"):
    """[M / 64, Cout / 8, 2] = (mean, M2) of a STORED y1 [N, OH, OW, Cout] over 64 consecutive pixels x 8 channels. The
    input is what the kernel stored, so this statistic is checked on its own, not through the conv's error. abs: the
    terms of each sum (|y| / 512 for the mean; M2 is a sum of squares, its own magnitude)."""
    wt = _work(mode)
    v = y1.to(wt).reshape(-1, 64, y1.shape[-1] // 8, 8)
    if mode == "abs":
        mean = v.abs().mean(dim=(1, 3))
        m2 = ((v - v.mean(dim=(1, 3), keepdim=True)) ** 2).sum(dim=(1, 3))
        return torch.stack([mean, m2], -1)
    mean = v.mean(dim=(1, 3), keepdim=True)
    return torch.stack([mean.reshape(mean.shape[0], -1), ((v - mean) ** 2).sum(dim=(1, 3))], -1)


def accept(case, tensor, got, ref64, yard, terms, dt, extra=0.0):
    """max|got - f64| <= k * max|yardstick - f64| + floor, k = 4 for an fp32 tensor and 2 for a
    bf16 one, floor = 2 * 2^-24 * max(sum |terms|) (+ extra): the accumulators are fp32 in both modes, and the bf16
    store is in the yardstick. NaN anywhere fails. Prints `conv-ratio <case> <dtype> <tensor> ratio [extra]`; returns
    (ok, ratio); the ratio err / (yardstick + floor / k) passes up to k."""
    k = K_MARGIN[dt]
    g = got.double()
    nan = bool(torch.isnan(g).any()) or g.shape != ref64.shape
    err = float("nan") if nan else ((g - ref64).abs().max().item() if g.numel() else 0.0)
    yerr = (yard.double() - ref64).abs().max().item() if g.numel() else 0.0
    fl = 2.0 * 2.0 ** -24 * (terms.max().item() if terms.numel() else 0.0) + extra
    den = yerr + fl / k
    ratio = err / den if den > 0 else (0.0 if err == 0 else math.inf)
    print(f"conv-ratio {case} {NAME[dt]} {tensor}: err {err:.3e} yardstick {yerr:.3e} floor {fl:.3e} ratio {ratio:.2f} "
          f"k {k:g}" + (f" extra {extra:.3e}" if extra else ""))
    return (not nan) and err <= k * yerr + fl, ratio
