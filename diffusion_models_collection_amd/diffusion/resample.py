"""Timestep samplers for training (not in the reference): the uniform draw, and the loss-second-moment resampler of
Nichol & Dhariwal 2021 (arXiv:2102.09672 §3.3) with its state on the device.

    sampler = create_named_schedule_sampler('loss-second-moment', diffusion)
    t, weights = sampler.sample(batch_size, device)
    loss = diffusion.p_losses(model, x0, t, y, schedule_sampler=sampler)   # weights the loss, feeds the history
    loss.backward()

The history of the last history_per_term losses per timestep (fp32 [T, K]), its counts (int32 [T]), the probabilities,
the CDF, the draw and the importance weights stay in HBM: sample() is one launch (dmc_ts_sample) on torch.rand's
draws, update_with_local_losses() one launch (dmc_ts_history_update), nothing is read back and everything is
deterministic given the draws. _resample.py has the formulas and their host restatement.

With several ranks each rank keeps the history of its own losses and weights by the p it drew from, so each rank's
estimator stays unbiased; gathering the losses across ranks (as the paper's code does) is not done. The history is
not part of the trainer's checkpoints: a resumed run draws uniformly until K * T losses have re-warmed it.

'logit-normal' (LogitNormalSampler) is the fixed density rectified flows are trained with (arXiv:2403.03206 §3.1): no
state, no importance weights, one searchsorted per draw.
"""
import torch

from .. import kernels as K
from . import _resample


class UniformSampler:
    """t uniform over [0, T), every weight 1: what the training loop does without a sampler."""

    def __init__(self, diffusion):
        self.num_timesteps = int(diffusion.num_timesteps)
        self._device = getattr(diffusion, "device", "cuda")

    def sample(self, batch_size, device=None, u=None):
        """(t int64 [B], weights fp32 [B] of ones). u: the draws in [0, 1) to use, t = floor(u * T)."""
        dev = torch.device(self._device if device is None else device)
        if u is None:
            t = torch.randint(0, self.num_timesteps, (batch_size,), device=dev).long()
        else:
            t = (u.to(dev).double() * self.num_timesteps).long().clamp_(0, self.num_timesteps - 1)
        return t, torch.ones(batch_size, dtype=torch.float32, device=dev)

    def update_with_local_losses(self, t, losses):
        pass

    def weights(self):
        """p [T] = 1/T, an fp32 tensor on the sampler's device, as LossSecondMomentResampler.weights()."""
        return torch.full((self.num_timesteps,), 1.0 / self.num_timesteps, dtype=torch.float32,
                          device=torch.device(self._device))

    def weight_table(self):
        """None: every importance weight is 1."""
        return None

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


class LossSecondMomentResampler:
    """p_t ~ sqrt(mean of the last K squared losses at t), mixed with uniform_prob of the uniform distribution; uniform
    until every timestep has K losses. The defaults are the paper's code's. uniform_prob = 0 is allowed, but a timestep
    whose K losses are all exactly 0 then has p = 0 and weight +inf: the draw skips it (T - 1, the search's fallback,
    excepted), a t handed to p_losses by hand does not. Keep uniform_prob > 0 where a loss can be exactly 0."""

    def __init__(self, diffusion, history_per_term=10, uniform_prob=0.001):
        self.num_timesteps = int(diffusion.num_timesteps)
        self.history_per_term = _resample.check_history_per_term(history_per_term)
        self.uniform_prob = _resample.check_uniform_prob(uniform_prob)
        self._device = getattr(diffusion, "device", "cuda")
        self._hist = self._count = self._p = self._iw = None

    def _state(self, device):
        """The device state, created on the first device seen."""
        if self._hist is None:
            dev = torch.device(self._device if device is None else device)
            if dev.type != "cuda":
                raise RuntimeError("the loss-second-moment resampler runs on the MI355X HIP kernels only: use a cuda device")
            if dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
            T = self.num_timesteps
            self._hist = torch.zeros(T, self.history_per_term, dtype=torch.float32, device=dev)
            self._count = torch.zeros(T, dtype=torch.int32, device=dev)
            self._p = torch.full((T,), 1.0 / T, dtype=torch.float32, device=dev)
            self._iw = torch.ones(T, dtype=torch.float32, device=dev)
        return self._hist, self._count

    def sample(self, batch_size, device=None, u=None):
        """(t int64 [B], weights fp32 [B] = iw[t]) from the current history. u: the draws in [0, 1) to use (fp32 [B] on
        the device), torch.rand's by default. Leaves p and iw for weights() / weight_table() in new tensors: a table a
        pending backward still holds is not written."""
        hist, count = self._state(device)
        if u is None:
            u = torch.rand(batch_size, dtype=torch.float32, device=hist.device)
        elif u.numel() != batch_size:
            raise ValueError(f"u holds {u.numel()} draws for a batch of {batch_size}")
        t, self._p, self._iw, _ = K.ts_sample(hist, count, self.uniform_prob, u.to(hist.device).float().contiguous())
        return t, self._iw[t]

    def update_with_local_losses(self, t, losses):
        """Feed this rank's per-sample losses (before the importance weight) at timesteps t into the history."""
        hist, count = self._state(losses.device)
        K.ts_history_update(t.to(hist.device).long().contiguous(), losses.detach().to(hist.device).float().contiguous(),
                            hist, count)

    def weights(self):
        """p [T], as left by the last sample() (uniform before the first)."""
        self._state(None)
        return self._p

    def weight_table(self):
        """iw [T] = 1 / (T p), as left by the last sample() (ones before the first)."""
        self._state(None)
        return self._iw

    def state_dict(self):
        hist, count = self._state(None)
        return {"history": hist.clone(), "count": count.clone()}

    def load_state_dict(self, state):
        h, c = state["history"], state["count"]
        shape = (self.num_timesteps, self.history_per_term)
        if tuple(h.shape) != shape or tuple(c.shape) != shape[:1]:
            raise ValueError(f"the sampler's history is {shape} with a count of {shape[:1]}, the state holds "
                             f"{tuple(h.shape)} and {tuple(c.shape)}")
        hist, count = self._state(h.device if h.is_cuda else None)
        hist.copy_(h)
        count.copy_(c)


class LogitNormalSampler:
    """t from the logit-normal density of Esser et al. 2024 (arXiv:2403.03206 §3.1), which puts the training weight on
    the middle noise levels of a rectified flow: u = sigmoid(mean + std * z), z ~ N(0, 1), t = floor(u * T). The exact
    bin masses and their CDF are built once on the host (_resample.logit_normal_masses); a draw is torch.rand and one
    torch.searchsorted on the device table. The loss is NOT re-weighted (the density is the weighting, as in SD3), so
    weight_table() is None and every weight is 1. Works with any scheduler object that has num_timesteps."""

    def __init__(self, diffusion, mean=0.0, std=1.0):
        self.num_timesteps = int(diffusion.num_timesteps)
        self.mean, self.std = _resample.check_logit_normal(mean, std)
        self._device = getattr(diffusion, "device", "cuda")
        self._masses = _resample.logit_normal_masses(self.num_timesteps, self.mean, self.std)
        self._cdf_host = torch.from_numpy(_resample.logit_normal_cdf(self._masses))
        self._cdf = None

    def cdf(self, device=None):
        """fp32 [T] on the device, uploaded once per device."""
        dev = torch.device(self._device if device is None else device)
        if self._cdf is None or self._cdf.device != dev:
            self._cdf = self._cdf_host.to(dev)
        return self._cdf

    def sample(self, batch_size, device=None, u=None):
        """(t int64 [B], weights fp32 [B] of ones). u: the draws in [0, 1) to use (fp32 [B]), torch.rand's by default;
        t is the smallest index whose CDF entry exceeds u."""
        cdf = self.cdf(device)
        if u is None:
            u = torch.rand(batch_size, dtype=torch.float32, device=cdf.device)
        elif u.numel() != batch_size:
            raise ValueError(f"u holds {u.numel()} draws for a batch of {batch_size}")
        t = torch.searchsorted(cdf, u.to(cdf.device).float().contiguous().view(-1), right=True)
        return t.clamp_(max=self.num_timesteps - 1), torch.ones(batch_size, dtype=torch.float32, device=cdf.device)

    def update_with_local_losses(self, t, losses):
        pass

    def weights(self):
        """p [T], an fp32 tensor on the sampler's device, as LossSecondMomentResampler.weights()."""
        return torch.from_numpy(self._masses.astype("float32")).to(torch.device(self._device))

    def weight_table(self):
        """None: every importance weight is 1."""
        return None

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


def create_named_schedule_sampler(name, diffusion, **kwargs):
    """'uniform', 'loss-second-moment' (kwargs: history_per_term, uniform_prob) or 'logit-normal' (kwargs: mean, std)."""
    name = _resample.check_sampler_name(name)
    if name == "uniform":
        return UniformSampler(diffusion, **kwargs)
    if name == "logit-normal":
        return LogitNormalSampler(diffusion, **kwargs)
    return LossSecondMomentResampler(diffusion, **kwargs)
