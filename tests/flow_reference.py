"""Rectified flow in numpy, written from the formulas alone (it shares no code with the package): the sigma tables, the
trailing inference grid, the per-evaluation row tables, dmc_flow_step and dmc_flow_guide one op at a time in a given
precision, the sampler loop, and the exact velocity field and answer for N(0, s^2 I) data.

    sigma_t = shift*u / (1 + (shift - 1)*u),  u = (t + 1)/T;   x_t = (1 - sigma_t) x0 + sigma_t eps;   v = eps - x0
    rows {sigma, h, hh, kind}: h = sigma_next - sigma_this, hh = h/2; kind 0 Euler, 1 Heun predictor, 2 Heun corrector
"""
import numpy as np

F32, F64 = np.float32, np.float64


def ref_sigmas(T, shift=1.0):
    """(sigma, 1 - sigma), fp32 [T], each the float64 value rounded once."""
    u = np.arange(1, T + 1, dtype=F64) / T
    sig = float(shift) * u / (1.0 + (float(shift) - 1.0) * u)
    return sig.astype(F32), (1.0 - sig).astype(F32)


def ref_timesteps(T, S):
    """'trailing' spacing: round(arange(T, 0, -T/S)) - 1."""
    return (np.round(np.arange(T, 0, -T / S)[:S]) - 1).astype(np.int64)


def ref_rows(sigmas, ts, solver):
    """(coef fp32 [R, 4], step timesteps int64 [R]). The sigma column is the level of the row's own evaluation."""
    S = len(ts)
    sg = list(np.asarray(sigmas, F32)[ts].astype(F64)) + [0.0]
    coef, tt = [], []
    for i in range(S):
        h = sg[i + 1] - sg[i]
        if solver == "heun" and i < S - 1:
            coef += [[sg[i], h, h / 2, 1.0], [sg[i + 1], h, h / 2, 2.0]]
            tt += [ts[i], ts[i + 1]]
        else:
            assert solver in ("euler", "heun")
            coef.append([sg[i], h, h / 2, 0.0])
            tt.append(ts[i])
    return np.asarray(coef, F64).astype(F32), np.asarray(tt, np.int64)


def _pick(dt, coef, step):
    R = coef.shape[0]
    rows = np.asarray(coef, F32)[np.clip(np.asarray(step, np.int64), 0, R - 1)].astype(dt)
    kind = rows[:, 3]
    kind = np.where((kind == 1) | (kind == 2), kind, 0).astype(np.int64)
    return rows[:, 0:1], rows[:, 1:2], rows[:, 2:3], kind


def guided(dt, pc, pu, scale):
    """g = pu + scale*(pc - pu), two roundings after the difference; pu None: pc."""
    if pu is None:
        return np.asarray(pc, F32).astype(dt)
    c, u = np.asarray(pc, F32).astype(dt), np.asarray(pu, F32).astype(dt)
    d = (c - u).astype(dt)
    m = (dt(np.float32(scale)) * d).astype(dt)
    return (u + m).astype(dt)


def flow_step_ref(dt, coef, step, x, pc, pu, scale, xb, dprev, xb_old=None, d_old=None):
    """dmc_flow_step's ops one at a time in precision dt on [N, per] arrays -> (out, xb_out, d_out). xb / dprev None: a
    corrector row gives NaN. xb_old / d_old: what the history outputs held before (kept on rows of kind 0 and 2)."""
    N = x.shape[0]
    _, h, hh, kind = _pick(dt, coef, step)
    g = guided(dt, pc, pu, scale)
    xx = np.asarray(x, F32).astype(dt)
    eul = (xx + (h * g).astype(dt)).astype(dt)
    nan = np.full(xx.shape, np.nan, dt)
    b = nan if xb is None or dprev is None else np.asarray(xb, F32).astype(dt)
    d = nan if xb is None or dprev is None else np.asarray(dprev, F32).astype(dt)
    with np.errstate(invalid="ignore"):
        s = (d + g).astype(dt)
        cor = (b + (hh * s).astype(dt)).astype(dt)
    k = kind.reshape(N, 1)
    out = np.where(k == 2, cor, eul)
    xb_old = nan if xb_old is None else np.asarray(xb_old, F32).astype(dt)
    d_old = nan if d_old is None else np.asarray(d_old, F32).astype(dt)
    return out, np.where(k == 1, xx, xb_old), np.where(k == 1, g, d_old)


def rescale_factor(dt, pc, g, phi):
    """Per row [N, 1]: phi*std(pc)/std(g) + (1 - phi); float64 from the unrounded sums of squared deviations, fp32 'the
    same arithmetic' with the sample standard deviations. A row without spread in g keeps factor 1."""
    N, per = g.shape
    ph = float(np.float32(phi))
    c = np.asarray(pc, F32).astype(dt)
    if dt == F64:
        m2c = ((c - c.mean(1, keepdims=True)) ** 2).sum(1)
        m2g = ((g - g.mean(1, keepdims=True)) ** 2).sum(1)
        ok = m2g > 0
        with np.errstate(all="ignore"):
            ratio = np.sqrt(m2c / m2g)
    elif per == 1:
        ratio, ok = np.ones(N, dt), np.zeros(N, bool)
    else:
        sg = g.std(1, ddof=1, dtype=dt)
        ok = sg > 0
        with np.errstate(all="ignore"):
            ratio = (c.std(1, ddof=1, dtype=dt) / sg).astype(dt)
    f = np.where(ok, dt(ph) * ratio + dt(1 - ph), dt(1)).astype(dt)
    return f.reshape(N, 1)


def quantile_scale(dt, x0, p):
    """max(quantile_p |x0|, 1) per row [N, 1]: linear interpolation at rank p*(per-1), the lerp taken from the nearer
    end (w < 0.5: a + w*(b - a), else b - (b - a)*(1 - w)), every op rounded to dt."""
    srt = np.sort(np.abs(x0), axis=1).astype(dt)
    per = srt.shape[1]
    rank = dt(dt(np.float32(p)) * dt(per - 1))
    lo = int(np.floor(rank))
    hi = int(np.ceil(rank))
    w = dt(rank - dt(lo))
    a, b = srt[:, lo], srt[:, hi]
    diff = (b - a).astype(dt)
    if w < dt(0.5):
        q = (a + (w * diff).astype(dt)).astype(dt)
    else:
        q = (b - (diff * dt(dt(1) - w)).astype(dt)).astype(dt)
    return np.maximum(q, dt(1)).reshape(-1, 1)


def flow_guide_ref(dt, coef, step, x, pc, pu, scale, phi, mode, p=None):
    """dmc_flow_guide's ops in precision dt. mode 'none': the guided (rescaled) velocity; 'clamp': x0 = x - sigma*g
    clamped to +-1; 'quantile': x0 = clamp(x0, -s, s)/s with s = quantile_scale; then g = (x - x0)/sigma."""
    sigma, _, _, _ = _pick(dt, coef, step)
    g = guided(dt, pc, pu, scale)
    if phi > 0:
        g = (g * rescale_factor(dt, pc, g, phi)).astype(dt)
    if mode == "none":
        return g
    xx = np.asarray(x, F32).astype(dt)
    x0 = (xx - (sigma * g).astype(dt)).astype(dt)
    if mode == "clamp":
        x0 = np.clip(x0, dt(-1), dt(1))
    else:
        assert mode == "quantile"
        s = quantile_scale(dt, x0, p)
        x0 = (np.clip(x0, -s, s) / s).astype(dt)
    return (((xx - x0).astype(dt)) / sigma).astype(dt)


# ------------------------------------------------------------------------------------------------------------
# the sampler loop and the Gaussian problem
# ------------------------------------------------------------------------------------------------------------
def gaussian_velocity(x, sigma, s2):
    """v(x, sigma) = (sigma - (1 - sigma) s^2) / ((1 - sigma)^2 s^2 + sigma^2) * x for x0 ~ N(0, s^2 I), eps ~ N(0, I):
    E[eps - x0 | x_t = x]. The op order is the one the device callable of the tests uses (numpy arrays or torch
    tensors in x's precision; sigma, s2 in the same precision)."""
    om = 1 - sigma
    num = sigma - om * s2
    den = om * om * s2 + sigma * sigma
    return num / den * x


def gaussian_velocity_fn(dt, sigmas, s):
    """velocity(x, t) in precision dt reading the fp32 sigma table."""
    s2 = dt(np.float32(s) * np.float32(s))
    tab = np.asarray(sigmas, F32)

    def fn(x, t):
        return gaussian_velocity(x, dt(tab[t]), s2).astype(dt)
    return fn


def point_velocity_fn(sigmas, c):
    """Point-mass data at c: v = (x - c)/sigma, float64."""
    tab = np.asarray(sigmas, F32).astype(F64)
    return lambda x, t: (x - c) / tab[t]


def sampler_loop(dt, xT, velocity, coef, step_ts):
    """The ODE loop over the row table in precision dt (every op rounded to dt)."""
    c = np.asarray(coef, F32).astype(dt)
    x = np.asarray(xT).astype(dt)
    xb = d = None
    for r in range(c.shape[0]):
        _, h, hh, kind = c[r]
        v = velocity(x, int(step_ts[r])).astype(dt)
        if kind == 2:
            x = (xb + (hh * (d + v).astype(dt)).astype(dt)).astype(dt)
        else:
            if kind == 1:
                xb, d = x, v
            x = (x + (h * v).astype(dt)).astype(dt)
    return x


def gaussian_exact(xT, s):
    """The ODE's exact solution at sigma = 0 from x_T at sigma = 1: the marginals are N(0, ((1-sigma)^2 s^2 + sigma^2) I)
    and the flow scales x by the ratio of their standard deviations, s / 1."""
    return float(s) * np.asarray(xT, F64)


def relative_errors(T, shift, s, xT):
    """{('euler', S) / ('heun', S): max per-element relative error of the float64 loop} for S in (10, 20)."""
    sig, _ = ref_sigmas(T, shift)
    exact = gaussian_exact(xT, s)
    out = {}
    for solver in ("euler", "heun"):
        for S in (10, 20):
            coef, tt = ref_rows(sig, ref_timesteps(T, S), solver)
            x = sampler_loop(F64, xT, gaussian_velocity_fn(F64, sig, s), coef, tt)
            out[solver, S] = float((np.abs(x - exact) / np.abs(exact)).max())
    return out


# ------------------------------------------------------------------------------------------------------------
# logit-normal timesteps
# ------------------------------------------------------------------------------------------------------------
def logit_normal_masses(T, mean, std):
    """p_t = Phi((logit((t+1)/T) - mean)/std) - Phi((logit(t/T) - mean)/std), float64, logit(0) = -inf, logit(1) = inf."""
    import math
    edges = [-math.inf] + [(math.log(k / T) - math.log1p(-k / T) - mean) / std for k in range(1, T)] + [math.inf]
    Phi = [0.5 * (1.0 + math.erf(e / math.sqrt(2.0))) for e in edges]
    return np.asarray([Phi[t + 1] - Phi[t] for t in range(T)], F64)
