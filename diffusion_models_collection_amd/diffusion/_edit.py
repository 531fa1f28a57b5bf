"""Editing samplers, host side: where image-to-image starts, the walk an inpainting loop executes, and the
coefficient table of the known-region blend (dmc_known_blend).

Image-to-image (SDEdit, Meng et al. 2021, arXiv:2108.01073) noises the given image up to the timestep of step i0 of
the sampler's list and runs the steps i0 .. S-1 from there. Inpainting (RePaint, Lugmayr et al. 2022,
arXiv:2201.09865, algorithm 1) runs every step, and after each one replaces the known region by the given image
noised to the level the step arrived at, t_{i+1}:

    known = sqrt(a_{t_{i+1}}) * image + sqrt(1 - a_{t_{i+1}}) * z          a = alphas_cumprod, a_{-1} = 1
    x     = mask * known + (1 - mask) * x

With resample = U > 1 each step is repeated U times (RePaint's jump length 1): every repetition but the last jumps
forward again from t_{i+1} to t_i,

    x = sqrt(a_{t_i} / a_{t_{i+1}}) * x + sqrt(1 - a_{t_i} / a_{t_{i+1}}) * z2

so the generated and the known region are harmonised at t_i once more. As in _dpm.py everything transcendental
happens here, in float64 numpy from the sampler's fp32 alphas_cumprod table, each coefficient rounded to fp32 once:
the device kernel is left with multiplies and adds.
"""
import numpy as np

_F = np.float32


def start_index(S, strength):
    """i0: image-to-image runs steps i0 .. S-1 of an S-step list, n_run = min(S, max(1, int(strength*S + 0.5))) of
    them. strength in (0, 1]; 1 runs the whole list."""
    s = float(strength)
    if not (0.0 < s <= 1.0):       # NaN fails both comparisons
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    S = int(S)
    if S < 1:
        raise ValueError(f"the sampler needs at least one step, got {S}")
    return S - min(S, max(1, int(s * S + 0.5)))


def edit_walk(S, i0, resample=1):
    """[(step i, renoise)]: for i in i0 .. S-1, `resample` times step i and blend; every repetition but the last
    re-noises back to step i's timestep (renoise = 1). (S - i0) * resample entries."""
    if isinstance(resample, bool) or int(resample) != resample or resample < 1:
        raise ValueError(f"resample must be an integer >= 1, got {resample}")
    if not 0 <= i0 < S:
        raise ValueError(f"start index {i0} outside the {S}-step list")
    U = int(resample)
    return [(i, int(u < U - 1)) for i in range(i0, S) for u in range(U)]


def blend_coefficients(alphas_cumprod, timesteps):
    """[2S, 4] fp32 rows {ka, kb, ra, rb} for a decreasing timestep list t_0 .. t_{S-1}; tn = t_{i+1}, and after the
    last step tn = -1 with a = 1. Rows 2i and 2i+1: ka = sqrt(a_tn), kb = sqrt(1 - a_tn) (the last step's are 1 and 0
    exactly: the known region comes back as given). Row 2i: ra = 1, rb = 0, no re-noise. Row 2i+1: ra =
    sqrt(a_ti / a_tn), rb = sqrt(1 - a_ti / a_tn), the forward jump from tn back to t_i."""
    ts = np.asarray(timesteps, np.int64)
    S = len(ts)
    if S < 1:
        raise ValueError("blend_coefficients: empty timestep list")
    a = np.asarray(alphas_cumprod, _F)[ts].astype(np.float64)
    an = np.concatenate([a[1:], [1.0]])
    if not bool(((a > 0) & (a <= an)).all()):
        raise ValueError("blend_coefficients: alphas_cumprod must be positive and non-increasing along the walk")
    q = a / an
    coef = np.zeros((2 * S, 4), np.float64)
    coef[0::2, 0] = coef[1::2, 0] = np.sqrt(an)
    coef[0::2, 1] = coef[1::2, 1] = np.sqrt(1.0 - an)
    coef[0::2, 2] = 1.0
    coef[1::2, 2] = np.sqrt(q)
    coef[1::2, 3] = np.sqrt(1.0 - q)
    return np.ascontiguousarray(coef.astype(_F))
