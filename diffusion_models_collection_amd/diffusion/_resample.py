"""Loss-aware timestep sampling, host side: argument checks and float64 numpy restatements of the two device kernels.
Not in the reference.

Nichol & Dhariwal 2021 (arXiv:2102.09672 §3.3): the terms L_t of the variational bound differ by orders of magnitude
over t, so a uniformly drawn t gives L_vlb a noisy gradient. Draw t with p_t ~ sqrt(E[L_t^2]) instead, E[L_t^2]
estimated from the last K = 10 losses seen at each t, and weight the sample's loss by 1/(T p_t): the estimator
(1/N) sum_n L_{t_n} / (T p_{t_n}) keeps the expectation (1/T) sum_t L_t of the uniform draw whatever p is, because
sum_t p_t * 1/(T p_t) * L_t = (1/T) sum_t L_t. Until every t has K losses the draw is uniform; afterwards a share
uniform_prob of the mass stays uniform so that no p_t reaches 0.

The device keeps the history as a ring (history_update below): slot count % K is overwritten, where the paper's code
shifts the row left and appends. After the same losses both hold the same K values per row in a different order, and
only the multiset enters sqrt(mean_k h^2).

dmc_ts_history_update and dmc_ts_sample (kernels.ts_history_update, kernels.ts_sample) do on the device what the two
functions here do on the host; nothing in training calls these: they are the statement the tests check the kernels
against, kept beside the checks the samplers use.

The logit-normal density (Esser et al. 2024, arXiv:2403.03206 §3.1) is not loss-aware and needs no kernel: its exact bin
masses and their CDF are built here once (logit_normal_masses, logit_normal_cdf) and the draw is one searchsorted on the
device table.
"""
import math

import numpy as np

SAMPLERS = ("uniform", "loss-second-moment", "logit-normal")


def check_sampler_name(name):
    if name not in SAMPLERS:
        raise ValueError(f"unknown schedule sampler {name!r}: expected one of {SAMPLERS}")
    return name


def check_history_per_term(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"history_per_term must be an int >= 1, got {k!r}")
    return int(k)


def check_uniform_prob(p):
    if isinstance(p, (bool, str)) or not isinstance(p, (int, float, np.floating)) or not 0.0 <= float(p) < 1.0:
        raise ValueError(f"uniform_prob must be a number in [0, 1), got {p!r}")
    return float(p)


def history_update(hist, count, t, loss):
    """The sequential loop of dmc_ts_history_update, in place: hist [T, K], count [T], t [N] (clamped into [0, T)),
    loss [N]."""
    T, K = hist.shape
    for tn, ln in zip(np.asarray(t).tolist(), np.asarray(loss).tolist()):
        tt = min(max(int(tn), 0), T - 1)
        hist[tt, int(count[tt]) % K] = ln
        count[tt] += 1
    return hist, count


def second_moment_weights(hist, count, uniform_prob):
    """(p, iw, cdf) of dmc_ts_sample in float64: hist [T, K], count [T]. uniform_prob enters as the fp32 value the
    kernel is handed. Uniform (p = 1/T, iw = 1, cdf = (i+1)/T) unless every count >= K and S = sum_t r_t is a positive
    finite number; cdf[T-1] is exactly 1."""
    hist = np.asarray(hist, dtype=np.float64)
    T, K = hist.shape
    up = float(np.float32(check_uniform_prob(uniform_prob)))
    with np.errstate(all="ignore"):
        r = np.sqrt(np.mean(hist * hist, axis=1))
        S = float(np.sum(r))
    if not np.all(np.asarray(count) >= K) or not (S > 0.0 and np.isfinite(S)):
        p = np.full(T, 1.0 / T)
        iw = np.ones(T)
        cdf = np.arange(1, T + 1, dtype=np.float64) / T
    else:
        q = r / S * (1.0 - up) + up / T
        p = q / np.sum(q)
        iw = 1.0 / (T * p)
        cdf = np.cumsum(p)
    cdf[T - 1] = 1.0
    return p, iw, cdf


def draw(cdf, u):
    """dmc_ts_sample's draw: the smallest i with cdf[i] > u."""
    return np.minimum(np.searchsorted(cdf, u, side="right"), len(cdf) - 1).astype(np.int64)


def check_logit_normal(mean, std):
    for name, v in (("mean", mean), ("std", std)):
        if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(v)):
            raise ValueError(f"logit-normal {name} must be a finite number, got {v!r}")
    if not float(std) > 0.0:
        raise ValueError(f"logit-normal std must be > 0, got {std!r}")
    return float(mean), float(std)


def logit_normal_masses(num_timesteps, mean=0.0, std=1.0):
    """p_t = Phi((logit((t+1)/T) - mean)/std) - Phi((logit(t/T) - mean)/std) in float64, t in [0, T): the mass a
    logit-normal variable on (0, 1) puts on the bin [t/T, (t+1)/T), with logit(0) = -inf and logit(1) = +inf. The
    differences are taken on the side of the mean where Phi is small (Phi(a) - Phi(b) = Phi(-b) - Phi(-a)), so the tail
    bins keep their relative precision."""
    T = int(num_timesteps)
    if T < 1:
        raise ValueError(f"num_timesteps must be >= 1, got {num_timesteps!r}")
    mean, std = check_logit_normal(mean, std)
    z = np.empty(T + 1, np.float64)
    z[0], z[T] = -np.inf, np.inf
    e = np.arange(1, T, dtype=np.float64) / T
    z[1:T] = (np.log(e) - np.log1p(-e) - mean) / std
    phi = np.vectorize(lambda v: 0.5 * math.erfc(-v / math.sqrt(2.0)), otypes=[np.float64])
    lo, hi = z[:-1], z[1:]
    upper = lo >= 0                       # the bin lies above the mean: work with the upper tails
    return np.where(upper, phi(-lo) - phi(-hi), phi(hi) - phi(lo))


def logit_normal_cdf(masses):
    """fp32 [T]: the float64 running sum of the masses rounded once, the last entry 1 (what the total is, up to the
    rounding of T additions)."""
    cdf = np.cumsum(np.asarray(masses, np.float64)).astype(np.float32)
    cdf[-1] = 1.0
    return np.ascontiguousarray(cdf)
