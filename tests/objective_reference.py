"""The training objective (v-prediction, min-SNR-gamma weights) and the v -> (eps, x0) conversion restated from their
formulas in plain torch / numpy, independently of diffusion/_objective.py, diffusion/ddpm.py and the kernels. Everything
here runs on the CPU (the element-wise restatements also take device tensors: eager torch ops round once each).

With a = alphas_cumprod[t], alpha = sqrt(a), sigma = sqrt(1 - a), SNR = a / (1 - a):

    v = alpha * eps - sigma * x0                 (Salimans & Ho 2022, arXiv:2202.00512)
    x0 = alpha * x_t - sigma * v                 eps = sigma * x_t + alpha * v
    w_eps = min(SNR, gamma) / SNR                w_v = min(SNR, gamma) / (SNR + 1)     (Hang et al. 2023,
                                                                                         arXiv:2303.09556)
    L = mean_n [ w(t_n) * mean_i f(target_ni - pred_ni) ]

Gaussian problem (tests/dpm_reference.py): data ~ N(0, s^2 I); the exact v-denoiser is alpha * eps_hat - sigma * x0_hat
with dpm_reference.gaussian_eps's x0_hat and eps_hat.
"""
import numpy as np
import torch

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------
# weights
# ------------------------------------------------------------------------------------------------------------
def textbook_weights(ac32, gamma, prediction_type):
    """float64 [T], the papers' forms through the SNR itself."""
    a = np.asarray(ac32, F32).astype(F64)
    snr = a / (1.0 - a)
    m = np.minimum(snr, float(gamma))
    return m / snr if prediction_type == "eps" else m / (snr + 1.0)


# ------------------------------------------------------------------------------------------------------------
# objective: target, loss, gradient (torch, precision dt; one op = one rounding)
# ------------------------------------------------------------------------------------------------------------
def target(dt, prediction_type, sa, s1, t, x0, noise):
    """[N, per] target in precision dt: noise, or a_ = sa*noise; b_ = s1*x0; a_ - b_."""
    N = noise.shape[0]
    if prediction_type == "eps":
        return noise.to(dt)
    a_ = sa.to(dt)[t].view(N, 1) * noise.to(dt)
    b_ = s1.to(dt)[t].view(N, 1) * x0.to(dt)
    return a_ - b_


def loss_term(kind, d):
    if kind == "l2":
        return d * d
    if kind == "l1":
        return d.abs()
    ad = d.abs()
    return torch.where(ad < 1, 0.5 * d * d, ad - 0.5)


def loss(dt, prediction_type, kind, pred, x0, noise, t, sa, s1, w):
    """Scalar loss in precision dt: per-sample means, weighted, then the mean over samples."""
    N = pred.shape[0]
    tg = target(dt, prediction_type, sa, s1, t, x0, noise)
    per_sample = loss_term(kind, tg - pred.to(dt)).mean(1)
    if w is not None:
        per_sample = w.to(dt)[t] * per_sample
    return per_sample.sum() / N


def grad(prediction_type, kind, pred, x0, noise, t, sa, s1, w, dloss):
    """dpred in fp32, the kernel's ops one at a time: g = dloss / (float)(N*per); scale_n = g * w[t_n] (no multiply
    without weights); dpred = v * scale_n with v = 2d | sign(d) | (|d| < 1 ? d : sign(d)), d = pred - target."""
    N, per = pred.shape
    tg = target(torch.float32, prediction_type, sa, s1, t, x0, noise)
    g = torch.tensor(dloss, dtype=torch.float32) / torch.tensor(float(N * per), dtype=torch.float32)
    scale = g.expand(N).view(N, 1)
    if w is not None:
        scale = g * w[t].view(N, 1)
    d = pred - tg
    if kind == "l2":
        v = 2.0 * d
    elif kind == "l1":
        v = torch.sign(d)
    else:
        v = torch.where(d.abs() < 1, d, torch.sign(d))
    return v * scale


def grad64(prediction_type, kind, pred, x0, noise, t, sa, s1, w):
    """d loss / d pred by autograd on the float64 loss (a check of grad() itself)."""
    p = pred.double().requires_grad_(True)
    loss(torch.float64, prediction_type, kind, p, x0, noise, t, sa, s1, w).backward()
    return p.grad


# ------------------------------------------------------------------------------------------------------------
# conversion
# ------------------------------------------------------------------------------------------------------------
def convert(dt, x, t, sa, s1, pred, reps=1):
    """(eps, x0) of a v output in precision dt, op by op: u = s1*x; q = sa*pred; eps = u + q; p = sa*x; r = s1*pred;
    x0 = p - r. pred: [reps*N, ...], row r*N + n pairs with x[n], t[n]. Works on any device."""
    N = x.shape[0]
    shape = (N,) + (1,) * (x.dim() - 1)
    san = sa.to(dt)[t].view(shape).repeat((reps,) + (1,) * (x.dim() - 1))
    s1n = s1.to(dt)[t].view(shape).repeat((reps,) + (1,) * (x.dim() - 1))
    xx = x.to(dt).repeat((reps,) + (1,) * (x.dim() - 1))
    pp = pred.to(dt)
    u = s1n * xx
    q = san * pp
    eps = u + q
    p = san * xx
    r = s1n * pp
    return eps, p - r


def v_of(dt, sa, s1, t, x0, eps):
    """v = sa*eps - s1*x0 in precision dt (the round-trip test builds it in float64 and rounds once)."""
    N = x0.shape[0]
    return sa.to(dt)[t].view(N, 1) * eps.to(dt) - s1.to(dt)[t].view(N, 1) * x0.to(dt)


# ------------------------------------------------------------------------------------------------------------
# the Gaussian v-denoiser and the samplers' loops in (eps, x0) form (numpy, precision dt)
# ------------------------------------------------------------------------------------------------------------
def gaussian_v(x, a, sa, s1, s2, one=1):
    """v of the exact denoiser for N(0, s2 I) data from +, -, *, / alone: dpm_reference.gaussian_eps's x0hat and eps,
    then sa*eps - s1*x0hat. numpy and torch arrays of one precision run the same op sequence."""
    x0hat = (sa * s2 * x) / (a * s2 + (one - a))
    eps = (x - sa * x0hat) / s1
    return sa * eps - s1 * x0hat


def gaussian_pair_fn(dt, ac32, sa32, s1_32, ts, s):
    """pair_fn(i, x) -> (eps, x0) of a v-prediction sampler with the Gaussian v-denoiser at timestep ts[i]. The
    denoiser holds a and its two square roots (correctly rounded in fp32, as tests' device denoiser; float64 ones in
    float64); the conversion reads the sampler's fp32 tables sa32 / s1_32, widened."""
    a32 = np.asarray(ac32, F32)[np.asarray(ts)]
    if dt == F32:
        a, ra, r1 = a32, np.sqrt(a32.astype(F64)).astype(F32), np.sqrt((F32(1) - a32).astype(F64)).astype(F32)
    else:
        a = a32.astype(F64)
        ra, r1 = np.sqrt(a), np.sqrt(1.0 - a)
    sa = np.asarray(sa32, F32)[np.asarray(ts)].astype(dt)
    s1 = np.asarray(s1_32, F32)[np.asarray(ts)].astype(dt)
    s2 = dt(s) * dt(s)

    def fn(i, x):
        v = gaussian_v(x, a[i], ra[i], r1[i], s2, dt(1)).astype(dt)
        u = s1[i] * x
        q = sa[i] * v
        p = sa[i] * x
        r = s1[i] * v
        return (u + q).astype(dt), (p - r).astype(dt)

    return fn


def ddim_loop(dt, x_T, pair_fn, ac32, ts):
    """DDIM, eta = 0, no clipping, x0 handed in: x' = sqrt(a_n) x0 + sqrt(1 - a_n) eps, a_n = 1 after the last one."""
    a = np.asarray(ac32, F32)[np.asarray(ts)].astype(dt)
    x = np.asarray(x_T).astype(dt)
    for i in range(len(a)):
        an = a[i + 1] if i + 1 < len(a) else dt(1)
        eps, x0 = pair_fn(i, x)
        x = (np.sqrt(an) * x0 + np.sqrt(dt(1) - an) * eps).astype(dt)
    return x


def solver_loop(dt, x_T, pair_fn, coef):
    """DPM-Solver++ (dpm_reference.solver_loop) with x0 handed in, no clipping."""
    c = np.asarray(coef).astype(dt)
    x = np.asarray(x_T).astype(dt)
    prev = None
    for i in range(len(c)):
        _, _, cx, c0, c1 = c[i]
        _, x0 = pair_fn(i, x)
        new = cx * x + c0 * x0
        if c1 != 0:
            new = new + c1 * prev
        x, prev = new.astype(dt), x0
    return x


def ddpm_loop(dt, x_T, pair_fn, c1_32, c2_32, logvar32, ts, z):
    """DDPM ancestral steps, x0 handed in, no clipping: mean = c1 x0 + c2 x; x' = mean + [t != 0] exp(lv / 2) z_i."""
    c1, c2, lv = (np.asarray(v, F32)[np.asarray(ts)].astype(dt) for v in (c1_32, c2_32, logvar32))
    x = np.asarray(x_T).astype(dt)
    for i in range(len(ts)):
        _, x0 = pair_fn(i, x)
        mean = c1[i] * x0 + c2[i] * x
        mask = dt(1) if ts[i] != 0 else dt(0)
        x = (mean + (mask * np.exp(dt(0.5) * lv[i])) * np.asarray(z[i]).astype(dt)).astype(dt)
    return x
