"""Rectified flow / flow matching, host side: the noise levels, the inference grid and the per-evaluation step table.
Not in the reference (Liu et al. 2022, arXiv:2209.03003; Lipman et al. 2022, arXiv:2210.02747; SiT, arXiv:2401.08740;
Esser et al. 2024, arXiv:2403.03206).

The path between data and noise is linear: level t in [0, T) has

    sigma_t = s*u / (1 + (s - 1)*u),   u = (t + 1)/T,   shift s >= 1      (SD3's resolution shift; s = 1: sigma = u)
    x_t = (1 - sigma_t)*x0 + sigma_t*eps,          target v = eps - x0

sigma_{T-1} is exactly 1 (the last level is pure noise, the state sampling starts from) and sigma_0 > 0 (nothing divides
by 0). The model keeps its int64 timestep index: a flow with T discrete levels calls model(x, t, y) as it is.

Sampling integrates dx/dsigma = v from sigma = 1 to 0 over S intervals on _schedule.trailing_timesteps (ts[0] = T-1),
the sigma list being sigma[ts] followed by a final 0. One table row per model evaluation, {sigma, h, hh, kind} with
h = sigma_next - sigma_this (negative) and hh = h/2:

    solver 'euler': S rows of kind 0:                 x <- x + h*v
    solver 'heun' (Karras et al. 2022, arXiv:2206.00364 alg. 1): every interval i < S-1 has a predictor row (kind 1,
                    evaluated at ts[i]):              xb <- x; d <- v; x <- x + h*v
                    and a corrector row (kind 2, evaluated at ts[i+1] on the predicted state, h and hh of interval i):
                                                      x <- xb + hh*(d + v)
                    the last interval is one Euler row (the model has no level for sigma = 0): 2S - 1 rows.

The sigma column is the level of the row's own evaluation (what dmc_flow_guide's threshold reads). Everything is float64
numpy from the fp32 sigma table, each entry rounded to fp32 once; the device kernels (dmc_flow_step, dmc_flow_guide) are
left with adds, multiplies and one divide.
"""
import math

import numpy as np

from ._schedule import trailing_timesteps

_F = np.float32
SOLVERS = ("euler", "heun")
KIND_EULER, KIND_PREDICTOR, KIND_CORRECTOR = 0, 1, 2


def check_num_timesteps(num_timesteps):
    T = num_timesteps
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError(f"num_timesteps must be an int >= 1, got {num_timesteps!r}")
    return int(T)


def check_shift(shift):
    s = shift
    if isinstance(s, (bool, str, bytes)) or not isinstance(s, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(s)) or float(s) < 1.0:
        raise ValueError(f"shift must be a finite number >= 1, got {shift!r}")
    return float(s)


def check_solver(solver):
    if solver not in SOLVERS:
        raise ValueError(f"Unknown solver: {solver!r} (expected one of {SOLVERS})")
    return solver


def check_inference_steps(num_timesteps, num_inference_steps):
    S = num_inference_steps
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= S <= num_timesteps:
        raise ValueError(f"num_inference_steps must be an int in [1, {num_timesteps}], got {num_inference_steps!r}")
    return int(S)


def flow_sigmas(num_timesteps, shift=1.0):
    """(sigmas, one_minus_sigmas), fp32 [T]: float64, rounded once each."""
    T, s = check_num_timesteps(num_timesteps), check_shift(shift)
    u = np.arange(1, T + 1, dtype=np.float64) / T
    sig = s * u / (1.0 + (s - 1.0) * u)
    return np.ascontiguousarray(sig.astype(_F)), np.ascontiguousarray((1.0 - sig).astype(_F))


def flow_timesteps(num_timesteps, num_inference_steps):
    """int64 [S], strictly decreasing from T-1."""
    T = check_num_timesteps(num_timesteps)
    return np.ascontiguousarray(trailing_timesteps(T, check_inference_steps(T, num_inference_steps)), np.int64)


def flow_steps(sigmas, timesteps, solver="euler"):
    """(step_coefficients fp32 [R, 4] rows {sigma, h, hh, kind}, step_timesteps int64 [R]); see the module docstring."""
    check_solver(solver)
    ts = np.asarray(timesteps, np.int64)
    S = len(ts)
    sg = np.concatenate([np.asarray(sigmas, _F)[ts].astype(np.float64), [0.0]])
    rows, tt = [], []
    for i in range(S):
        h = sg[i + 1] - sg[i]
        if solver == "heun" and i < S - 1:
            rows.append((sg[i], h, 0.5 * h, KIND_PREDICTOR))
            tt.append(ts[i])
            rows.append((sg[i + 1], h, 0.5 * h, KIND_CORRECTOR))
            tt.append(ts[i + 1])
        else:
            rows.append((sg[i], h, 0.5 * h, KIND_EULER))
            tt.append(ts[i])
    coef = np.ascontiguousarray(np.asarray(rows, np.float64).astype(_F))
    return coef, np.ascontiguousarray(np.asarray(tt, np.int64))
