"""img2img / inpaint host arithmetic and loops restated in numpy from their formulas, independently of
diffusion/_edit.py and diffusion/_edit_loop.py. Everything here runs on the CPU.

With a = alphas_cumprod (the fp32 table, widened), t_i the sampler's i-th timestep, tn = t_{i+1} and a_{-1} = 1 after
the last step, walk entry (i, renoise) is

    x     = step_i(x)                                             the sampler's own update t_i -> tn
    known = sqrt(a_tn) image + sqrt(1 - a_tn) z                   (no z when a_tn = 1)
    x     = mask * known + (1 - mask) * x
    x     = sqrt(a_ti / a_tn) x + sqrt(1 - a_ti / a_tn) z2        only when the entry re-noises

The loops cover DDIM at eta = 0 and DDPM with injected draws, in a numpy precision dt with one rounding per op in the
kernels' order, so dt = float32 is the fp32 oracle and dt = float64 the reference of criterion 2.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def ref_start_index(S, strength):
    n_run = int(math.floor(float(strength) * S + 0.5))
    return S - min(S, max(1, n_run))


def ref_walk(S, i0, resample):
    out = []
    for i in range(i0, S):
        for u in range(resample):
            out.append((i, 1 if u != resample - 1 else 0))
    return out


def ref_blend_coefficients(ac32, ts):
    """[2S, 4] float64 rows {ka, kb, ra, rb}, unrounded."""
    a = [float(v) for v in np.asarray(ac32, F32)[np.asarray(ts)]]
    S = len(a)
    rows = np.zeros((2 * S, 4), F64)
    for i in range(S):
        an = a[i + 1] if i + 1 < S else 1.0
        for r in (2 * i, 2 * i + 1):
            rows[r, 0], rows[r, 1] = math.sqrt(an), math.sqrt(1.0 - an)
        rows[2 * i, 2], rows[2 * i, 3] = 1.0, 0.0
        rows[2 * i + 1, 2], rows[2 * i + 1, 3] = math.sqrt(a[i] / an), math.sqrt(1.0 - a[i] / an)
    return rows


def blend(dt, row, x, x0, m, z, z2):
    """dmc_known_blend's ops one at a time in precision dt for one coefficient row; z / z2 unread (may be None) where
    the row's kb / rb is 0."""
    ka, kb, ra, rb = (dt(v) for v in row)
    known = ka * x0
    if kb != 0:
        known = known + kb * z
    b = m * known + (dt(1) - m) * x
    if rb != 0:
        b = ra * b + rb * z2
    return b.astype(dt)


def ddim_step(dt, ac32, x, eps, t, tn, clip):
    """dmc_ddim_step at eta = 0: x0 from eps, clamp, sqrt(a_n) x0 + sqrt(1 - a_n) eps; a_n = 1 for tn < 0."""
    a = np.asarray(ac32, F32)
    at = dt(a[t])
    an = dt(a[tn]) if tn >= 0 else dt(1)
    x0 = (x - np.sqrt(dt(1) - at) * eps) / np.sqrt(at)
    if clip:
        x0 = np.clip(x0, dt(-1), dt(1))
    return (np.sqrt(an) * x0 + np.sqrt(dt(1) - an) * eps).astype(dt)


DDPM_TABS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
             "posterior_mean_coef2", "posterior_log_variance_clipped")


def ddpm_step(dt, tabs, x, eps, t, z, clip):
    """dmc_ddpm_step: x0 = sra x - srm1 eps, clamp, mean = c1 x0 + c2 x, + [t != 0] exp(0.5 logvar) z."""
    sra, srm1, c1, c2, lv = (dt(np.asarray(tabs[k], F32)[t]) for k in DDPM_TABS)
    x0 = sra * x - srm1 * eps
    if clip:
        x0 = np.clip(x0, dt(-1), dt(1))
    mean = c1 * x0 + c2 * x
    if t == 0:
        return mean.astype(dt)
    return (mean + np.exp(dt(0.5) * lv) * z).astype(dt)


def _step(dt, kind, tabs, ts, i, x, eps, z, clip):
    if kind == "ddim":
        return ddim_step(dt, tabs["alphas_cumprod"], x, eps, int(ts[i]), int(ts[i + 1]) if i + 1 < len(ts) else -1,
                         clip)
    return ddpm_step(dt, tabs, x, eps, int(ts[i]), z, clip)


def inpaint_loop(dt, kind, tabs, ts, coef, x_T, image, mask, resample, eps_fn, draw, clip=True, trace=None):
    """kind 'ddim' (eta = 0) or 'ddpm'; tabs: the sampler's fp32 tables; ts: its timestep list; coef: the [2S, 4]
    blend table the loop is to use; eps_fn(i, x) -> eps at ts[i]; draw(j, which) -> the injected draw of walk entry j
    (asked for only where the entry reads one); mask broadcasts against the image."""
    c = np.asarray(coef)
    x, img, m = (np.asarray(v).astype(dt) for v in (x_T, image, mask))
    for j, (i, renoise) in enumerate(ref_walk(len(ts), 0, resample)):
        z = draw(j, "step").astype(dt) if kind == "ddpm" else None
        x = _step(dt, kind, tabs, ts, i, x, eps_fn(i, x).astype(dt), z, clip)
        row = c[2 * i + renoise]
        zk = draw(j, "known").astype(dt) if row[1] != 0 else None
        z2 = draw(j, "renoise").astype(dt) if row[3] != 0 else None
        x = blend(dt, row, x, img, m, zk, z2)
        if trace is not None:
            trace.append(x.copy())
    return x


def img2img_loop(dt, kind, tabs, ts, strength, image, eps_fn, draw, clip=True):
    """q_sample to ts[i0] with the 'start' draw (the two fp32 square-root tables, as dmc_q_sample reads them), then
    steps i0 .. S-1; eps_fn(i, x) indexes the whole list."""
    i0 = ref_start_index(len(ts), strength)
    t0 = int(ts[i0])
    sa = dt(np.asarray(tabs["sqrt_alphas_cumprod"], F32)[t0])
    s1 = dt(np.asarray(tabs["sqrt_one_minus_alphas_cumprod"], F32)[t0])
    x = (sa * np.asarray(image).astype(dt) + s1 * draw(0, "start").astype(dt)).astype(dt)
    for j, i in enumerate(range(i0, len(ts))):
        z = draw(j, "step").astype(dt) if kind == "ddpm" else None
        x = _step(dt, kind, tabs, ts, i, x, eps_fn(i, x).astype(dt), z, clip)
    return x
