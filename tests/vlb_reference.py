"""Torch restatement of the variational bound in bits per dimension, written from Ho et al. 2020 (arXiv:2006.11239
§3-4) and Nichol & Dhariwal 2021 (arXiv:2102.09672 §2-3); CPU only, no import from the package.

The per-element arithmetic is parameterised by a dtype: float64 is the yardstick, float32 the measure of what plain
fp32 arithmetic can do on the same inputs. The per-timestep constants are formed in float64 from the fp32 alphas_cumprod
table (coefficients) and, as the specification of the host table says, rounded to fp32 once (table): both dtypes start
from those fp32 constants, as they start from the same fp32 images. The rounding itself is held to half an ulp of the
float64 constants by tests/test_vlb_host.py; were the yardstick to use the unrounded constants instead, no fp32 table
could meet a 1e-5 bound where a good prediction makes x0 - x0_pred small against x0 (a relative 6e-8 in c_x moves
x0 - c_x x_t + c_p pred by 6e-8 |x0|, which at t = 0 and a prediction error of 0.05 is 1e-4 of its value).
"""
import math

import torch

F32, F64 = torch.float32, torch.float64
LN2 = math.log(2.0)


def schedule(ac):
    """float64 (ac, acp, beta, pv, c1, c2) from the fp32 table."""
    ac = ac.to(F32).to(F64)
    acp = torch.cat([torch.ones(1, dtype=F64), ac[:-1]])
    beta = 1.0 - ac / acp
    pv = beta * (1.0 - acp) / (1.0 - ac)
    c1 = beta * acp.sqrt() / (1.0 - ac)
    c2 = (1.0 - acp) * (1.0 - beta).sqrt() / (1.0 - ac)
    return ac, acp, beta, pv, c1, c2


def log_variances(ac, variance):
    """float64 (lv_p, lv_q); entry 0 of both is log pv[1]."""
    _, _, beta, pv, _, _ = schedule(ac)
    lv_q = torch.cat([pv[1:2], pv[1:]]).log()
    if variance == "fixed_small":
        return lv_q.clone(), lv_q
    assert variance == "fixed_large", variance
    return torch.cat([pv[1:2], beta[1:]]).log(), lv_q


def coefficients(ac, ptype, variance):
    """float64 dict of [T] constants: c_x, c_p, kprec, kvar, keps, isig."""
    a, acp, beta, pv, c1, _ = schedule(ac)
    lv_p, lv_q = log_variances(ac, variance)
    if ptype == "eps":
        c_x, c_p = (1.0 / a).sqrt(), (1.0 / a - 1.0).sqrt()
    else:
        assert ptype == "v", ptype
        c_x, c_p = a.sqrt(), (1.0 - a).sqrt()
    d = lv_p - lv_q
    return {"c_x": c_x, "c_p": c_p, "kprec": 0.5 * c1 * c1 * (-lv_p).exp(), "kvar": 0.5 * (d + torch.expm1(-d)),
            "keps": a / (1.0 - a), "isig": (-0.5 * lv_p).exp()}


def table(ac, ptype, variance):
    """The constants as the device reads them: rounded to fp32 once."""
    return {k: v.to(F32) for k, v in coefficients(ac, ptype, variance).items()}


def cdf(z):
    """Exact normal CDF."""
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0))


def vlb_step(dt, ac, ptype, variance, t, x0, x_t, pred, clip, rounded=True):
    """One timestep's per-sample (vb, xstart_mse, eps_mse, x0_sq), each [N] of dtype dt. x0, x_t, pred: [N, per] fp32;
    t: [N] int64. rounded=False takes the constants unrounded (the formulas alone, for the host-side checks)."""
    co = {k: v[t].to(dt).view(-1, 1) for k, v in (table if rounded else coefficients)(ac, ptype, variance).items()}
    x0, x_t, pred = x0.to(dt), x_t.to(dt), pred.to(dt)
    u = co["c_x"] * x_t - co["c_p"] * pred
    xp = u.clamp(-1.0, 1.0) if clip else u
    d = x0 - xp
    du = x0 - u
    kl = co["kvar"] + co["kprec"] * d * d
    h = 1.0 / 255.0
    zp = (d + h) * co["isig"]
    zm = (d - h) * co["isig"]
    left = zm <= 0
    a = torch.where(left, zp, -zm)
    b = torch.where(left, zm, -zp)
    pr = torch.where(x0 < -0.999, cdf(zp), torch.where(x0 > 0.999, cdf(-zm), cdf(a) - cdf(b)))
    nll = -pr.clamp_min(1e-12).log()
    term = torch.where((t == 0).view(-1, 1), nll, kl)
    per = x0.shape[1]
    return (term.sum(1) / per / LN2, (d * d).sum(1) / per, co["keps"].view(-1) * ((du * du).sum(1) / per),
            (x0 * x0).sum(1) / per)


def textbook_kl(ac, variance, t, x0, x0_pred, x_t):
    """float64 [N, per]: the KL of the true posterior from the model's, the textbook way: both means formed, then
    0.5 (-1 + lv_p - lv_q + exp(lv_q - lv_p) + (mu_q - mu_p)^2 exp(-lv_p))."""
    _, _, _, _, c1, c2 = schedule(ac)
    lv_p, lv_q = (v[t].view(-1, 1) for v in log_variances(ac, variance))
    c1, c2 = c1[t].view(-1, 1), c2[t].view(-1, 1)
    mu_q = c1 * x0.to(F64) + c2 * x_t.to(F64)
    mu_p = c1 * x0_pred.to(F64) + c2 * x_t.to(F64)
    return 0.5 * (-1.0 + lv_p - lv_q + (lv_q - lv_p).exp() + (mu_q - mu_p) ** 2 * (-lv_p).exp())


def prior_bpd(ac, x0):
    """float64 [N]: KL(q(x_T | x0) || N(0, I)) per dimension in bits, the textbook way from mean and log-variance."""
    a = schedule(ac)[0][-1]
    mu = a.sqrt() * x0.to(F64)
    lv = (1.0 - a).log()
    kl = 0.5 * (-1.0 - lv + lv.exp() + mu * mu)
    return kl.flatten(1).mean(1) / LN2


def grid_images(shape, g):
    """x0 on the 8-bit grid k/127.5 - 1 with -1 and +1 present in every sample (fp32)."""
    k = torch.randint(0, 256, shape, generator=g)
    flat = k.view(shape[0], -1)
    if flat.shape[1] >= 2:
        flat[:, -1] = 0
        flat[:, -2] = 255
    return (k.double() / 127.5 - 1.0).float()
