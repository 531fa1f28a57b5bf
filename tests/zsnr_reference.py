"""Zero-terminal-SNR schedules, trailing timesteps and rescaled guidance (Lin et al. 2023, arXiv:2305.08891) restated in
float64 numpy from the paper's formulas, independently of diffusion/_schedule.py, _objective.py and the samplers: the
schedule rescale (Algorithm 1), the 'trailing' grid (table 2), the guided and rescaled prediction (eq. 14-16) with its
conversion to (eps, x0), the v-prediction DDIM loop, the v loss with min-SNR weights, and the Gaussian test
problem in v form. Everything here runs on the CPU; cpu_selfcheck() exercises all of it (tests/test_zsnr_host.py).

Conventions: ac32 is the sampler's fp32 alphas_cumprod table; sa = sqrt(ac) and s1 = sqrt(fl32(1 - ac)) are the
fp32 tables the device gathers, widened, so a float64 result differs from the device's by roundings alone.
"""
import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------
# schedule
# ------------------------------------------------------------------------------------------------------------
def ref_rescale(ac32):
    """Algorithm 1: float64 [T], unrounded. sqrt(ac) shifted so that the last entry is 0 and scaled so that the first
    is kept (the paper's two in-place lines, in their order)."""
    s = np.sqrt(np.asarray(ac32, F32).astype(F64))
    s0, sT = s[0], s[-1]
    s = s - sT
    s = s * (s0 / (s0 - sT))
    return s * s


def ref_trailing(T, S):
    """Table 2: round(arange(T, 0, -T/S)) - 1, listed element by element (Python's round is half to even too)."""
    return np.array([round(T - k * (T / S)) - 1 for k in range(S)], np.int64)


def ref_tables(ac32):
    """(sa, s1) fp32 tables of an alphas_cumprod table, as the samplers upload them (numpy's fp32 sqrt is IEEE)."""
    a = np.asarray(ac32, F32)
    return np.sqrt(a), np.sqrt(F32(1) - a)


def ref_min_snr_v(ac32, gamma):
    """min(SNR, gamma) / (SNR + 1) for a v target, SNR = a / (1 - a), from the SNR itself where it is defined and 0
    where a = 0. float64, unrounded."""
    a = np.asarray(ac32, F32).astype(F64)
    w = np.zeros_like(a)
    pos = a > 0
    snr = a[pos] / (1.0 - a[pos])
    w[pos] = np.minimum(snr, gamma) / (snr + 1.0)
    return w


# ------------------------------------------------------------------------------------------------------------
# guidance
# ------------------------------------------------------------------------------------------------------------
def guide_factor(pc, g, phi):
    """[N] float64: phi * std(pc) / std(g) + (1 - phi) per row (either normalisation of std: it cancels); 1 where the
    guided row has no spread (the public implementations return NaN there)."""
    pc, g = np.asarray(pc, F64), np.asarray(g, F64)
    m2c = ((pc - pc.mean(1, keepdims=True)) ** 2).sum(1)
    m2g = ((g - g.mean(1, keepdims=True)) ** 2).sum(1)
    ok = m2g > 0
    f = np.ones(pc.shape[0], F64)
    f[ok] = phi * np.sqrt(m2c[ok] / m2g[ok]) + (1.0 - phi)
    return f


def guide(dt, pred_type, x, pc, pu, scale, phi, sa, s1):
    """(eps, x0) [N, per] before any threshold, in numpy precision dt; sa, s1: [N] per-sample table values. The
    guided prediction g = pu + scale * (pc - pu) is formed in dt; the factor is always float64 from that g, rounded to
    fp32 (the device's one rounding) and applied in dt."""
    x, pc, pu = (np.asarray(v).astype(dt) for v in (x, pc, pu))
    sa, s1 = (np.asarray(v).astype(dt).reshape(-1, 1) for v in (sa, s1))
    g = pu + dt(scale) * (pc - pu)
    if phi > 0:
        f = guide_factor(pc, g, float(F32(phi))).astype(F32).astype(dt).reshape(-1, 1)
        g = g * f
    if pred_type == "v":
        return s1 * x + sa * g, sa * x - s1 * g
    with np.errstate(divide="ignore", invalid="ignore"):
        return g, (x - s1 * g) / sa


# ------------------------------------------------------------------------------------------------------------
# Gaussian test problem in v form
# ------------------------------------------------------------------------------------------------------------
def gaussian_v(x, a, sa, s1, s2, one=1):
    """v = sa * eps - s1 * x0hat of the exact denoiser for N(0, s2 I) data, from +, -, *, / alone (numpy or torch
    arrays of one precision run the same op sequence). Finite at a = 0: x0hat = 0, eps = x, v = 0 * x - 1 * 0."""
    x0hat = (sa * s2 * x) / (a * s2 + (one - a))
    eps = (x - sa * x0hat) / s1
    return sa * eps - s1 * x0hat


def gaussian_v_fn(dt, ac32, ts, s2):
    """v_fn(i, x) for the loops below in precision dt; s2: scalar or [N] per-sample data variance (the label)."""
    a32 = np.asarray(ac32, F32)[np.asarray(ts)]
    sa32, s132 = ref_tables(a32)
    a, sa, s1 = a32.astype(dt), sa32.astype(dt), s132.astype(dt)
    s2 = np.asarray(s2, F32).astype(dt)
    s2 = s2.reshape(-1, 1, 1, 1) if s2.ndim else s2
    return lambda i, x: gaussian_v(x, a[i], sa[i], s1[i], s2, dt(1))


# ------------------------------------------------------------------------------------------------------------
# loops
# ------------------------------------------------------------------------------------------------------------
def ddim_v_loop(dt, x_T, v_fn, ac32, ts, trace=None):
    """DDIM, eta = 0, no clipping, v-prediction: x0 = sa x - s1 v, eps = s1 x + sa v, x' = sqrt(a_n) x0 +
    sqrt(1 - a_n) eps, a_n = 1 after the last timestep. Nothing divides: a = 0 at the first step is an ordinary one."""
    a32 = np.asarray(ac32, F32)[np.asarray(ts)]
    sa32, s132 = ref_tables(a32)
    a, sa, s1 = a32.astype(dt), sa32.astype(dt), s132.astype(dt)
    x = np.asarray(x_T).astype(dt)
    for i in range(len(a)):
        an = a[i + 1] if i + 1 < len(a) else dt(1)
        v = v_fn(i, x).astype(dt)
        x0 = sa[i] * x - s1[i] * v
        eps = s1[i] * x + sa[i] * v
        x = (np.sqrt(an) * x0 + np.sqrt(dt(1) - an) * eps).astype(dt)
        if trace is not None:
            trace.append(x.copy())
    return x


# ------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------
def v_loss(pred, x0, noise, t, ac32, w=None, dt=F64):
    """(loss, dloss/dpred) in precision dt for the l2 loss on the v target: mean over samples of w[t_n] times the
    per-sample mean of (pred - (sa noise - s1 x0))^2. pred, x0, noise: [N, per]; w: a [T] weight table or None."""
    sa32, s132 = ref_tables(np.asarray(ac32, F32)[np.asarray(t)])
    sa, s1 = sa32.astype(dt).reshape(-1, 1), s132.astype(dt).reshape(-1, 1)
    pred, x0, noise = (np.asarray(v).astype(dt) for v in (pred, x0, noise))
    N, per = pred.shape
    wn = np.ones(N, dt) if w is None else np.asarray(w).astype(dt)[np.asarray(t)]
    d = pred - (sa * noise - s1 * x0)
    loss = (wn * (d * d).mean(1, dtype=dt)).mean(dtype=dt)
    return dt(loss), (dt(2) * d * wn.reshape(-1, 1) / dt(N * per)).astype(dt)


# ------------------------------------------------------------------------------------------------------------
def cpu_selfcheck():
    """The restatements against the paper's statements and against each other, on the CPU alone."""
    T = 1000
    betas = np.linspace(1e-4, 0.02, T, dtype=F64)
    ac32 = np.cumprod(1.0 - betas).astype(F32)
    r = ref_rescale(ac32)
    assert r[-1] == 0.0 and abs(r[0] - float(ac32[0])) < 1e-15 and bool((np.diff(r) < 0).all())
    # the rescale is affine in sqrt(ac): the ratios of sqrt differences are kept
    s, sr = np.sqrt(ac32.astype(F64)), np.sqrt(r)
    assert np.allclose((sr[1:-1] - sr[-1]) / (sr[0] - sr[-1]), (s[1:-1] - s[-1]) / (s[0] - s[-1]), rtol=1e-12)
    assert ref_trailing(1000, 50).tolist() == list(range(999, 0, -20))
    assert ref_trailing(1000, 3).tolist() == [999, 666, 332] and ref_trailing(1000, 1).tolist() == [999]
    assert ref_trailing(1000, 1000).tolist() == list(range(999, -1, -1))
    z32 = r.astype(F32)
    w = ref_min_snr_v(z32, 5.0)
    a = z32.astype(F64)
    assert w[-1] == 0 and np.allclose(w, np.minimum(a, 5.0 * (1 - a)), rtol=1e-12, atol=0)

    g = np.random.default_rng(0)
    N, per = 4, 96
    x, pc, pu = (g.standard_normal((N, per)) for _ in range(3))
    pu[1] = pc[1]
    pc[2] = 0.25
    pu[2] = 0.25
    t = np.array([0, 500, 999, 998])
    sa32, s132 = ref_tables(z32[t])
    for pt in ("v", "eps"):
        for phi in (0.0, 0.7, 1.0):
            e64, x64 = guide(F64, pt, x, pc, pu, 3.0, phi, sa32, s132)
            e32, x32 = guide(F32, pt, x, pc, pu, 3.0, phi, sa32, s132)
            ok = np.ones(N, bool) if pt == "v" else sa32 > 0
            assert bool(np.isfinite(e64[ok]).all()) and bool(np.isfinite(x64[ok]).all())
            assert np.abs(e32[ok] - e64[ok]).max() < 1e-4 and np.abs(x32[ok] - x64[ok]).max() < 2e-2
            if pt == "v":
                # (eps, x0) is a rotation of (x, g): eps^2 + x0^2 = x^2 + g^2
                gg = pu + 3.0 * (pc - pu)
                if phi > 0:
                    gg = gg * guide_factor(pc, gg, float(F32(phi))).astype(F32).astype(F64).reshape(-1, 1)
                a2 = (sa32.astype(F64) ** 2 + s132.astype(F64) ** 2).reshape(-1, 1)
                assert np.allclose(e64 ** 2 + x64 ** 2, a2 * (x ** 2 + gg ** 2), rtol=1e-9)
    f = guide_factor(pc, pu + 3.0 * (pc - pu), 1.0)
    assert f[1] == 1.0 and f[2] == 1.0      # pc == pu: ratio 1; a constant row: no spread, left alone
    gg = (pu + 3.0 * (pc - pu)) * f.reshape(-1, 1)
    assert np.allclose(gg[[0, 3]].std(1), pc[[0, 3]].std(1), rtol=1e-12)     # phi = 1 restores the conditional std

    ts = ref_trailing(T, 10)
    xT = g.standard_normal((2, 3, 4, 4))
    s2 = np.array([0.25, 2.0])
    tr64, tr32 = [], []
    o64 = ddim_v_loop(F64, xT, gaussian_v_fn(F64, z32, ts, s2), z32, ts, tr64)
    o32 = ddim_v_loop(F32, xT, gaussian_v_fn(F32, z32, ts, s2), z32, ts, tr32)
    assert all(bool(np.isfinite(v).all()) for v in tr64 + tr32) and np.abs(o32 - o64).max() < 1e-4
    # the probability-flow ODE of N(0, s2 I) data carries x_T ~ N(0, I) at a = 0 to x_T * s at a = 1; DDIM is first
    # order in the step: the relative error falls about as 1 / S (0.26, 0.057, 0.015 at S = 10, 50, 200)
    errs = []
    for S in (10, 50, 200):
        tsS = ref_trailing(T, S)
        o = ddim_v_loop(F64, xT, gaussian_v_fn(F64, z32, tsS, s2), z32, tsS)
        errs.append(np.abs(o / (xT * np.sqrt(s2).reshape(-1, 1, 1, 1)) - 1).max())
    assert errs[2] < 0.03 and errs[1] < errs[0] / 3 and errs[2] < errs[1] / 3, errs

    pred, x0, noise = (g.standard_normal((4, 12)) for _ in range(3))
    tt = np.array([999, 0, 400, 998])
    loss, grad = v_loss(pred, x0, noise, tt, z32, w)
    sa_l, _ = ref_tables(z32[tt])
    assert sa_l[0] == 0      # at T-1 the v target is -x0
    l0, _ = v_loss(-x0[:1], x0[:1], noise[:1], tt[:1], z32)
    assert l0 == 0.0
    h = 1e-6
    p2 = pred.copy()
    p2[2, 5] += h
    assert abs((v_loss(p2, x0, noise, tt, z32, w)[0] - loss) / h - grad[2, 5]) < 1e-5
    assert bool((grad[0] == 0).all())       # the min-SNR weight at T-1 is 0
    return True
