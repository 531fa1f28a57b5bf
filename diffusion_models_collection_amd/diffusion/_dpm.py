"""DPM-Solver++ (Lu et al. 2022, arXiv:2211.01095) host side: inference timesteps and the per-step coefficient table.

Multistep solver in data-prediction form, orders 1 and 2 (2M). With a = alphas_cumprod[t], alpha = sqrt(a),
sigma = sqrt(1 - a) and the half log-SNR lambda = log(alpha / sigma) = 0.5 * log(a / (1 - a)), the update from
t_i to t_{i+1} is

    h = lambda_{i+1} - lambda_i,   r = (lambda_i - lambda_{i-1}) / h,   E = -alpha_{i+1} * expm1(-h)
    order 1:  x_{i+1} = (sigma_{i+1} / sigma_i) * x_i + E * x0_i
    order 2:  x_{i+1} = (sigma_{i+1} / sigma_i) * x_i + E * (1 + 1/(2r)) * x0_i - E / (2r) * x0_{i-1}

Everything transcendental happens here, in float64 numpy from the sampler's fp32 alphas_cumprod table, and each
coefficient is rounded to fp32 once. The device kernel (dmc_dpm_step) is left with multiplies, adds, one divide and
a clamp, so it can be tested bit for bit against an op-by-op restatement and needs no device libm.
"""
import numpy as np

from ._schedule import ddim_timesteps

_F = np.float32
SPACINGS = ("logsnr", "linspace")


def half_logsnr(alphas_cumprod):
    """lambda_t in float64 from the fp32 table; a_t of exactly 0 or 1 has none."""
    a = np.asarray(alphas_cumprod, _F)
    if bool(((a <= 0) | (a >= 1)).any()):
        raise ValueError("DPM-Solver++: alphas_cumprod must lie strictly between 0 and 1 in fp32 at every selected "
                         "timestep (the log-SNR is undefined otherwise)")
    a = a.astype(np.float64)
    return 0.5 * np.log(a / (1.0 - a))


def dpm_timesteps(num_timesteps, num_inference_steps, spacing, alphas_cumprod):
    """int64, strictly decreasing. 'linspace' is DDIM's grid; 'logsnr' takes num_inference_steps targets uniform in
    lambda from lambda_{T-1} to lambda_0, maps each to the timestep with the nearest lambda and drops duplicates
    (so the result can be shorter than requested: several targets fall between t = 0 and t = 1)."""
    a = np.asarray(alphas_cumprod, _F)
    if spacing == "linspace":
        ts = ddim_timesteps(num_timesteps, num_inference_steps)
    elif spacing == "logsnr":
        lam = half_logsnr(a[:num_timesteps])
        targets = np.linspace(lam[num_timesteps - 1], lam[0], num_inference_steps)
        ts = np.abs(lam[None, :] - targets[:, None]).argmin(axis=1).astype(np.int64)
        ts = ts[np.concatenate([[True], ts[1:] != ts[:-1]])]
    else:
        raise ValueError(f"Unknown timestep spacing: {spacing} (expected one of {SPACINGS})")
    ts = np.ascontiguousarray(ts, np.int64)
    if len(ts) > 1 and not bool((np.diff(ts) < 0).all()):
        raise ValueError(f"DPM-Solver++: timesteps are not strictly decreasing: {ts.tolist()}")
    half_logsnr(a[ts])
    return ts


def dpm_coefficients(alphas_cumprod, timesteps, solver_order=2, lower_order_final=True):
    """[S', 5] fp32 rows {sa, s1, cx, c0, c1} for the update t_i -> t_{i+1} (see the module docstring).

    sa = sqrt(a_i) and s1 = sqrt(1 - a_i) are the correctly rounded fp32 square roots of the fp32 values a_i and
    1 - a_i: what ddim_step_kernel forms on the device, so eps -> x0 matches DDIM's bit for bit. Row 0 (no history
    yet) and, with lower_order_final, row S'-2 are order 1. The last row is cx = 0, c0 = 1, c1 = 0: the last
    evaluation returns its x0 prediction, as DDIM's last step does with alpha_next = 1."""
    if solver_order not in (1, 2):
        raise ValueError(f"solver_order must be 1 or 2, got {solver_order}")
    ts = np.asarray(timesteps, np.int64)
    a32 = np.asarray(alphas_cumprod, _F)[ts]
    lam = half_logsnr(a32)
    a = a32.astype(np.float64)
    alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
    S = len(ts)
    coef = np.zeros((S, 5), np.float64)
    coef[:, 0] = np.sqrt(a32)                      # IEEE fp32 sqrt: correctly rounded
    coef[:, 1] = np.sqrt(_F(1) - a32)
    for i in range(S - 1):
        h = lam[i + 1] - lam[i]
        E = -alpha[i + 1] * np.expm1(-h)
        cx = sigma[i + 1] / sigma[i]
        first_order = solver_order == 1 or i == 0 or (lower_order_final and i == S - 2)
        if first_order:
            c0, c1 = E, 0.0
        else:
            r = (lam[i] - lam[i - 1]) / h
            c0, c1 = E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r)
        coef[i, 2:] = cx, c0, c1
    coef[S - 1, 2:] = 0.0, 1.0, 0.0
    return np.ascontiguousarray(coef.astype(_F))
