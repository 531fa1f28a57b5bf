"""Torch restatement of learned variances (Nichol & Dhariwal 2021, arXiv:2102.09672 §3.1 and eq. 15-16): the hybrid
loss, the bound's per-timestep term with a learned log-variance and the sampler step; CPU only, no import from the
package. Written from the formulas, not from the kernels.

As tests/vlb_reference.py: the arithmetic is parameterised by a dtype (float64 the yardstick, float32 the measure of what
plain fp32 arithmetic does on the same inputs), the per-timestep constants are formed in float64 from the fp32
alphas_cumprod table and rounded to fp32 once (`table`), and gradients come from torch autograd.

Per timestep: lv_min = log pv[max(t, 1)], lv_max = log beta[t], R = lv_max - lv_min, the model's log-variance
lv_p = lv_min + (v + 1)/2 * R (not clamped), delta = x0 - x0_pred, and
    t >= 1:  term = 0.5 (d + expm1(-d)) + kmin exp(-d) delta^2,   d = lv_p - lv_min,  kmin = 0.5 c1^2 exp(-lv_min)
    t == 0:  term = -log max(P, 1e-12), P the decoder's Gaussian N(x0_pred, exp(lv_p)) discretised on the 8-bit grid
"""
import torch

from vlb_reference import LN2, cdf, schedule

F32, F64 = torch.float32, torch.float64


def coefficients(ac, ptype):
    """float64 dict of [T] constants. R is formed by log1p for t >= 1: the two logs' difference loses digits there."""
    a, acp, beta, pv, c1, _ = schedule(ac)
    if ptype == "eps":
        c_x, c_p = (1.0 / a).sqrt(), (1.0 / a - 1.0).sqrt()
    else:
        assert ptype == "v", ptype
        c_x, c_p = a.sqrt(), (1.0 - a).sqrt()
    lv_min = torch.cat([pv[1:2], pv[1:]]).log()
    lv_max = beta.log()
    R = lv_max - lv_min
    R[1:] = -torch.log1p((a[1:] - acp[1:]) / (1.0 - a[1:]))
    return {"c_x": c_x, "c_p": c_p, "c1": c1, "lv_min": lv_min, "R": R, "kmin": 0.5 * c1 * c1 * (-lv_min).exp(),
            "keps": a / (1.0 - a), "lv_max": lv_max}


COLUMNS = ("c_x", "c_p", "c1", "lv_min", "R", "kmin", "keps", "lv_max")


def table(ac, ptype):
    """The constants as the device reads them: rounded to fp32 once."""
    return {k: v.to(F32) for k, v in coefficients(ac, ptype).items()}


def _rows(dt, ac, ptype, t, rounded=True):
    return {k: v[t].to(dt).view(-1, 1) for k, v in (table if rounded else coefficients)(ac, ptype).items()}


def term(dt, co, t, x0, delta, v):
    """[N, per] of dtype dt, nats: the KL (t >= 1) or the decoder's -log p (t == 0). x0, delta, v already of dtype dt."""
    d = (v + 1.0) * 0.5 * co["R"]
    kl = 0.5 * (d + torch.expm1(-d)) + co["kmin"] * torch.exp(-d) * delta * delta
    isig = torch.exp(-0.5 * (co["lv_min"] + d))
    h = 1.0 / 255.0
    zp = (delta + h) * isig
    zm = (delta - h) * isig
    left = zm <= 0
    a = torch.where(left, zp, -zm)
    b = torch.where(left, zm, -zp)
    pr = torch.where(x0 < -0.999, cdf(zp), torch.where(x0 > 0.999, cdf(-zm), cdf(a) - cdf(b)))
    nll = -pr.clamp_min(1e-12).log()
    return torch.where((t == 0).view(-1, 1), nll, kl), pr


def simple_elem(loss_type, diff):
    if loss_type == "l2":
        return diff * diff
    if loss_type == "l1":
        return diff.abs()
    ad = diff.abs()
    return torch.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5)


def hybrid(dt, ac, ptype, t, out, x0, noise, loss_type="l2", w=None, vlb_weight=0.001, dloss=1.0, tabs=None):
    """(loss[3] = {total, simple, vlb}, dout [N, 2, per], pr) in dtype dt. out: [N, 2, per] fp32 (prediction, v);
    x0, noise: [N, per] fp32; w: None or the [T] fp32 weight table; tabs: (sa, s1) fp32 [T] tables for 'v'. The bound's
    term sends no gradient to the prediction half (the paper's stop-gradient)."""
    co = _rows(dt, ac, ptype, t)
    N, _, per = out.shape
    o = out.to(dt).clone().requires_grad_(True)
    pred, v = o[:, 0], o[:, 1]
    if ptype == "eps":
        tgt = noise.to(dt)
    else:
        sa, s1 = (tb[t].to(dt).view(-1, 1) for tb in tabs)
        tgt = sa * noise.to(dt) - s1 * x0.to(dt)
    per_sample = simple_elem(loss_type, tgt - pred).sum(1) / per
    if w is not None:
        per_sample = w[t].to(dt) * per_sample
    simple = per_sample.sum() / N
    delta = co["c_p"] * (pred.detach() - tgt)
    tm, pr = term(dt, co, t, x0.to(dt), delta, v)
    vb = tm.sum(1) / per / LN2
    vlb = vlb_weight * (vb.sum() / N)
    total = simple + vlb
    total.backward(torch.tensor(dloss, dtype=dt))
    return torch.stack([total, simple, vlb]).detach(), o.grad.detach(), pr.detach()


def vlb_step(dt, ac, ptype, t, x0, x_t, pred, v, clip):
    """One timestep's per-sample (vb, xstart_mse, eps_mse, x0_sq), each [N] of dtype dt, and pr [N, per]."""
    co = _rows(dt, ac, ptype, t)
    x0, x_t, pred, v = x0.to(dt), x_t.to(dt), pred.to(dt), v.to(dt)
    u = co["c_x"] * x_t - co["c_p"] * pred
    xp = u.clamp(-1.0, 1.0) if clip else u
    d = x0 - xp
    du = x0 - u
    tm, pr = term(dt, co, t, x0, d, v)
    per = x0.shape[1]
    return (tm.sum(1) / per / LN2, (d * d).sum(1) / per, co["keps"].view(-1) * ((du * du).sum(1) / per),
            (x0 * x0).sum(1) / per), pr


def ddpm_step(dt, ac, ptype_tabs, t, x, eps, v, z, clip, x0_in=None):
    """x_{t-1} in dtype dt: the mean from the samplers' four fp32 tables (sqrt_recip, sqrt_recipm1, coef1, coef2:
    ptype_tabs), plus [t != 0] exp(0.5 (lv_min + d)) z. The step kernel consumes an eps."""
    sra, srm1, c1, c2 = (tb[t].to(dt).view(-1, 1) for tb in ptype_tabs)
    co = _rows(dt, ac, "eps", t)
    xx = x.to(dt)
    x0 = sra * xx - srm1 * eps.to(dt) if x0_in is None else x0_in.to(dt)
    if clip:
        x0 = x0.clamp(-1, 1)
    mean = c1 * x0 + c2 * xx
    if z is None:
        return mean
    d = (v.to(dt) + 1.0) * 0.5 * co["R"]
    sd = torch.exp(0.5 * (co["lv_min"] + d))
    return mean + torch.where((t != 0).view(-1, 1), sd * z.to(dt), torch.zeros((), dtype=dt))
