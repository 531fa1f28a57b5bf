"""Training objective, host side: prediction types and the min-SNR-gamma weight table. Not in the reference.

v-prediction (Salimans & Ho 2022, arXiv:2202.00512): the network predicts v = alpha*eps - sigma*x0, with
alpha = sqrt(a), sigma = sqrt(1 - a), a = alphas_cumprod[t]. Then x0 = alpha*x_t - sigma*v and eps = sigma*x_t +
alpha*v: no division by alpha, where the eps form divides by sqrt(a_{T-1}) ~ 1/158 at the first sampling steps.

min-SNR-gamma (Hang et al. 2023, arXiv:2303.09556): each sample's loss is weighted by min(SNR_t, gamma) / SNR_t for an
eps target and min(SNR_t, gamma) / (SNR_t + 1) for a v target, SNR = a / (1 - a). The closed forms below need no
division by (1 - a) and no SNR:

    eps:  w = min(1, gamma * (1 - a) / a)
    v:    w = min(a, gamma * (1 - a))

The table is computed in float64 from the sampler's fp32 alphas_cumprod and rounded to fp32 once (the rule of
_dpm.py): the device (dmc_objective) only gathers w[t], so it needs no division or min of its own and stays testable
bit for bit. numpy only: importable without the compiled library.
"""
import math

import numpy as np

PREDICTION_TYPES = ("eps", "v")


def check_prediction_type(prediction_type):
    if prediction_type not in PREDICTION_TYPES:
        raise ValueError(f"Unknown prediction type: {prediction_type} (expected one of {PREDICTION_TYPES})")
    return prediction_type


def check_gamma(gamma):
    """gamma as a float; ValueError unless it is a finite real number > 0."""
    if isinstance(gamma, (bool, str, bytes)) or gamma is None:
        raise ValueError(f"snr_gamma must be a finite number > 0, got {gamma!r}")
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"snr_gamma must be a finite number > 0, got {gamma!r}") from None
    if not math.isfinite(g) or g <= 0:
        raise ValueError(f"snr_gamma must be a finite number > 0, got {gamma!r}")
    return g


def min_snr_weights(alphas_cumprod, gamma, prediction_type, zero_terminal=False):
    """float32 [T]: the min-SNR-gamma weight of every timestep for the given prediction type. zero_terminal=True admits
    the table of a zero-terminal-SNR schedule (arXiv:2305.08891), exactly one trailing alphas_cumprod = 0, for 'v' only:
    its closed form min(a, gamma * (1 - a)) is 0 there, where the eps form divides by a."""
    g = check_gamma(gamma)
    check_prediction_type(prediction_type)
    a = np.asarray(alphas_cumprod, np.float32).astype(np.float64)
    if zero_terminal:
        if prediction_type != "v" or a.ndim != 1 or a.size < 2 or a[-1] != 0:
            raise ValueError("min_snr_weights: zero_terminal=True needs prediction_type='v' and a [T >= 2] table whose "
                             "last entry, and no other, is 0 (a zero terminal SNR schedule)")
        w = min_snr_weights(a[:-1], g, prediction_type)
        return np.concatenate([w, np.zeros(1, np.float32)])
    if a.ndim != 1 or bool(((a <= 0) | (a >= 1)).any()):
        raise ValueError("min_snr_weights: alphas_cumprod must be a [T] table strictly between 0 and 1 in fp32 (the "
                         "SNR is undefined otherwise)")
    if prediction_type == "eps":
        w = np.minimum(1.0, g * (1.0 - a) / a)
    else:
        w = np.minimum(a, g * (1.0 - a))
    return w.astype(np.float32)
