"""DPM-Solver++ (multistep, data prediction, orders 1 and 2) restated in numpy from its formulas, independently of
diffusion/_dpm.py and diffusion/dpm_solver.py: timesteps, coefficients, the sampling loop, DDIM's eta = 0 loop, and
the Gaussian test problem with its closed-form answer. Everything here runs on the CPU.

With a = alphas_cumprod[t] (the fp32 table, widened), alpha = sqrt(a), sigma = sqrt(1 - a), lam = log(alpha/sigma):

    h = lam[i+1] - lam[i]      r = (lam[i] - lam[i-1]) / h      E = alpha[i+1] * (1 - exp(-h)) = -alpha[i+1]*expm1(-h)
    order 1:  x' = (sigma[i+1]/sigma[i]) x + E x0
    order 2:  x' = (sigma[i+1]/sigma[i]) x + E (1 + 1/(2r)) x0 - E/(2r) x0_prev
    last evaluation: x' = x0

Gaussian problem: data ~ N(0, s^2 I). The exact denoiser is x0hat = sqrt(a) s^2 x / (a s^2 + 1 - a), and the
probability-flow ODE carries x_T at t = T-1 to x_T * s / sqrt(a_{T-1} s^2 + 1 - a_{T-1}) at a = 1.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def lam_of(a):
    a = np.asarray(a, F64)
    return np.log(np.sqrt(a) / np.sqrt(1.0 - a))


def ref_timesteps(ac32, T, S):
    """The 'logsnr' grid: S targets uniform in lam from lam[T-1] to lam[0], each mapped to the timestep whose lam is
    nearest, duplicates dropped. int64, decreasing. ('linspace' is DDIM's grid, _schedule.ddim_timesteps.)"""
    lam = lam_of(np.asarray(ac32, F32)[:T])
    out = []
    for k in range(S):
        target = lam[T - 1] + (lam[0] - lam[T - 1]) * k / (S - 1)
        t = int(np.argmin(np.abs(lam - target)))
        if not out or out[-1] != t:
            out.append(t)
    return np.array(out, np.int64)


def ref_coefficients(ac32, ts, order, lower_order_final):
    """[S', 5] float64 rows {sa, s1, cx, c0, c1}, unrounded. sa = sqrt(a) and s1 = sqrt(fl32(1 - a)): the product's
    s1 is the fp32 sqrt of the fp32 difference, so the difference is rounded to fp32 here too."""
    a32 = np.asarray(ac32, F32)[np.asarray(ts)]
    a = a32.astype(F64)
    alpha, sigma, lam = np.sqrt(a), np.sqrt(1.0 - a), lam_of(a)
    n = len(a)
    rows = np.zeros((n, 5), F64)
    for i in range(n):
        rows[i, 0] = math.sqrt(a[i])
        rows[i, 1] = math.sqrt(float(F32(1) - a32[i]))
        if i == n - 1:
            rows[i, 2:] = (0.0, 1.0, 0.0)
            continue
        h = lam[i + 1] - lam[i]
        E = -alpha[i + 1] * math.expm1(-h)
        rows[i, 2] = sigma[i + 1] / sigma[i]
        if order == 1 or i == 0 or (lower_order_final and i == n - 2):
            rows[i, 3], rows[i, 4] = E, 0.0
        else:
            r = (lam[i] - lam[i - 1]) / h
            rows[i, 3], rows[i, 4] = E + E / (2 * r), -E / (2 * r)
    return rows


def solver_loop(dt, x_T, eps_fn, coef, clip=False, trace=None):
    """The sampling loop in numpy precision dt, one rounding per op in the kernel's order. eps_fn(i, x) -> eps at the
    i-th timestep. coef: the [S', 5] table the loop is to use (cast to dt)."""
    c = np.asarray(coef).astype(dt)
    x = np.asarray(x_T).astype(dt)
    prev = None
    for i in range(len(c)):
        sa, s1, cx, c0, c1 = c[i]
        eps = eps_fn(i, x).astype(dt)
        x0 = (x - s1 * eps) / sa
        if clip:
            x0 = np.clip(x0, dt(-1), dt(1))
        new = cx * x + c0 * x0
        if c1 != 0:
            new = new + c1 * prev
        x, prev = new.astype(dt), x0
        if trace is not None:
            trace.append(x.copy())
    return x


def ddim_loop(dt, x_T, eps_fn, ac32, ts):
    """DDIM, eta = 0, no clipping: x' = sqrt(a_n) x0 + sqrt(1 - a_n) eps, a_n = 1 after the last timestep."""
    a = np.asarray(ac32, F32)[np.asarray(ts)].astype(dt)
    x = np.asarray(x_T).astype(dt)
    for i in range(len(a)):
        an = a[i + 1] if i + 1 < len(a) else dt(1)
        eps = eps_fn(i, x).astype(dt)
        x0 = (x - np.sqrt(dt(1) - a[i]) * eps) / np.sqrt(a[i])
        x = (np.sqrt(an) * x0 + np.sqrt(dt(1) - an) * eps).astype(dt)
    return x


def gaussian_eps(x, a, sa, s1, s2, one=1):
    """eps of the exact denoiser for N(0, s2 I) data, from +, -, *, / alone (sa = sqrt(a), s1 = sqrt(1 - a) are handed
    in), so numpy and torch arrays of one precision run the same op sequence."""
    x0hat = (sa * s2 * x) / (a * s2 + (one - a))
    return (x - sa * x0hat) / s1


def gaussian_eps_fn(dt, ac32, ts, s):
    """eps_fn for solver_loop / ddim_loop in precision dt. The square roots are the correctly rounded fp32 ones in
    fp32 (what a device model reading fp32 tables holds) and float64 ones in float64."""
    a32 = np.asarray(ac32, F32)[np.asarray(ts)]
    if dt == F32:
        a, sa, s1 = a32, np.sqrt(a32), np.sqrt(F32(1) - a32)
    else:
        a = a32.astype(F64)
        sa, s1 = np.sqrt(a), np.sqrt(1.0 - a)
    s2 = dt(s) * dt(s)
    return lambda i, x: gaussian_eps(x, a[i], sa[i], s1[i], s2, dt(1))


def gaussian_exact(x_T, ac32, T, s):
    aT = float(np.asarray(ac32, F32)[T - 1])
    return np.asarray(x_T, F64) * s / math.sqrt(aT * s * s + 1.0 - aT)
