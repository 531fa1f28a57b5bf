"""The loss-second-moment timestep sampler (Nichol & Dhariwal 2021, arXiv:2102.09672 §3.3) restated in float64 numpy
from the paper and its published code's behaviour, independently of diffusion/_resample.py and of the kernels; CPU only, no
import from the package.

The paper's buffer: per timestep the last K losses; a new loss at a full row shifts the row left and goes last, at a row
with c < K entries it goes to slot c. Until EVERY row is full the draw is uniform. Then
    w_t = sqrt(mean_k L_{t,k}^2);  w /= sum w;  w = w * (1 - uniform_prob) + uniform_prob / T;  p = w / sum w
and a sample at t is weighted by 1 / (T p_t). A history whose second moments sum to 0 (or to no finite number) has no
p of this form: the draw is uniform there as well.
"""
import numpy as np

F64 = np.float64


class ShiftBuffer:
    """The paper's history: shift left and append."""

    def __init__(self, T, K):
        self.T, self.K = T, K
        self.hist = np.zeros((T, K), F64)
        self.count = np.zeros(T, np.int64)      # entries in the row, at most K

    def update(self, t, losses):
        for tt, l in zip(t, losses):
            tt = min(max(int(tt), 0), self.T - 1)
            if self.count[tt] == self.K:
                self.hist[tt, :-1] = self.hist[tt, 1:]
                self.hist[tt, -1] = l
            else:
                self.hist[tt, self.count[tt]] = l
                self.count[tt] += 1

    def warm(self):
        return bool((self.count == self.K).all())


def ring_update(hist, count, t, losses):
    """The ring the device keeps: slot count % K is overwritten, count is the number ever seen. In place."""
    T, K = hist.shape
    for tt, l in zip(t, losses):
        tt = min(max(int(tt), 0), T - 1)
        hist[tt, count[tt] % K] = l
        count[tt] += 1


def weights(hist, warm, uniform_prob):
    """(p, iw, cdf), float64 [T] each; uniform_prob as the fp32 value the device receives. Sums run one element at a
    time in index order."""
    hist = np.asarray(hist, F64)
    T, K = hist.shape
    up = F64(np.float32(uniform_prob))
    r = np.zeros(T, F64)
    for i in range(T):
        a = F64(0)
        for k in range(K):
            a += hist[i, k] * hist[i, k]
        r[i] = np.sqrt(a / K)
    S = F64(0)
    for i in range(T):
        S += r[i]
    if not warm or not (S > 0 and np.isfinite(S)):
        p = np.full(T, F64(1) / T)
        iw = np.ones(T, F64)
        cdf = np.arange(1, T + 1, dtype=F64) / T
    else:
        q = r / S * (1 - up) + up / T
        Q = F64(0)
        for i in range(T):
            Q += q[i]
        p = q / Q
        iw = 1 / (T * p)
        cdf = np.zeros(T, F64)
        c = F64(0)
        for i in range(T):
            c += p[i]
            cdf[i] = c
    cdf[T - 1] = 1
    return p, iw, cdf


def draw(cdf, u):
    """The smallest i with cdf[i] > u, one comparison at a time (cdf, u of one dtype)."""
    out = np.zeros(len(u), np.int64)
    for n, un in enumerate(u):
        i = 0
        while i < len(cdf) - 1 and not cdf[i] > un:
            i += 1
        out[n] = i
    return out
