"""Bits-per-dimension evaluation for DDPM, DDIM and DPMSolver (not in the reference): the variational bound of
Ho et al. 2020 (arXiv:2006.11239) / Nichol & Dhariwal 2021 (arXiv:2102.09672) over the sampler's schedule tables.

The bound is a property of the schedule and the network, not of a sampler's step count: every one of the T timesteps
(or the ones asked for) costs one model evaluation at x_t ~ q(x_t | x0) and ONE fused launch (dmc_vlb_step) that
forms the x0 prediction, the clip, the KL or decoder term, the three per-sample means and, in the same pass, the next
step's x_t from x0 and the next draw. The loop runs through _graph.run_loop, so steps after the first replay one
captured HIP graph: the state is one flat buffer holding x_t followed by the step's four [B] rows, x0 and the labels are
const graph inputs, every random draw happens eagerly outside the graph.
"""
import torch
from tqdm import tqdm

from .. import kernels as K
from . import _vlb
from ._graph import StepGraph, cache_for, run_loop


class LikelihoodMixin:
    """Needs the sampler's alphas_cumprod, num_timesteps, prediction_type, q_sample and _tab (and, for
    variance='learned', ObjectiveMixin's variance_type, _lvar_table, _check_out and _pred_of)."""

    def _vlb_table(self, variance, dev):
        """[T, 6] fp32 device table of _vlb.vlb_coefficients, built and uploaded once per (prediction type,
        variance)."""
        if variance not in _vlb.VARIANCES:
            raise ValueError(f"Unknown variance: {variance!r} (expected one of {_vlb.VARIANCES + ('learned',)})")
        key = (self.prediction_type, variance)
        cache = self.__dict__.setdefault("_vlb_tables", {})
        c = cache.get(key)
        if c is None or c.device != dev:
            c = cache[key] = torch.from_numpy(
                _vlb.vlb_coefficients(self.alphas_cumprod.cpu().numpy(), *key)).to(dev)
        return c

    @torch.no_grad()
    def calc_bpd(self, model, x0, y=None, clip_denoised=True, variance='fixed_small', noise=None, timesteps=None):
        """The variational bound on -log2 p(x0) per dimension, term by term. x0: [B, ...] in [-1, 1] on the 8-bit grid
        k/127.5 - 1. Walks t = T-1 .. 0, or the given `timesteps` (distinct ints in [0, T), taken in descending
        order). variance: the model's fixed variance, 'fixed_small' (posterior variance) or 'fixed_large' (beta), or
        'learned' (a variance_type='learned_range' sampler only: the model's own, dmc_vlb_step_learned reading both
        halves of the output in place; on such a sampler the two fixed choices use the prediction half, so the three
        can be compared on one model).
        noise: None (torch.randn_like per step), a [T, B, ...] tensor indexed by t, or a callable t -> tensor: the draw
        that makes x_t. y gives the conditional bound (there is no guided variant: a guided score is no likelihood).
        Returns fp32 device tensors: vb, xstart_mse, eps_mse [B, S] (columns in the order walked), timesteps [S]
        (int64), prior_bpd [B], and total_bpd [B] = vb.sum(1) + prior_bpd when all T steps were walked, else None."""
        if getattr(self, "rescale_zero_snr", False):
            raise ValueError("calc_bpd is not defined on a zero terminal SNR schedule (rescale_zero_snr=True): the "
                             "bound's tables need 0 < alphas_cumprod")
        learned = variance == "learned"
        lr = getattr(self, "variance_type", "fixed") == "learned_range"
        if learned and not lr:
            raise ValueError("variance='learned' needs a sampler with variance_type='learned_range'")
        if not torch.is_tensor(x0) or x0.dim() < 2:
            raise ValueError("x0 must be a [B, ...] tensor")
        if not x0.is_cuda or (y is not None and not y.is_cuda):
            raise RuntimeError("the diffusion hot path runs on the MI355X HIP kernels only: use cuda tensors")
        if torch.is_tensor(timesteps):
            timesteps = timesteps.tolist()
        T = self.num_timesteps
        ts = _vlb.walk_timesteps(timesteps, T)
        x0 = x0.float().contiguous()
        dev, B, shape = x0.device, x0.shape[0], x0.shape
        S, n = len(ts), x0.numel()
        coef = self._lvar_table(dev) if learned else self._vlb_table(variance, dev)
        sa, s1 = self._tab("sqrt_alphas_cumprod", dev), self._tab("sqrt_one_minus_alphas_cumprod", dev)
        clip = bool(clip_denoised)
        has_y = y is not None
        if has_y:
            y = y.to(dev)
        walk = torch.from_numpy(ts).to(dev)
        tab = walk.view(-1, 1).expand(-1, B).contiguous()
        nxt = torch.cat([tab[1:], torch.full((1, B), -1, dtype=torch.long, device=dev)], 0)

        def draw(t):
            if noise is None:
                return torch.randn_like(x0)
            z = noise(t) if callable(noise) else noise[t]
            z = z.to(dev).float().contiguous()
            if z.shape != shape:
                raise ValueError(f"noise for t = {t} is {tuple(z.shape)}, expected {tuple(shape)}")
            return z

        # the state: x_t, then the step's rows vb, xstart_mse, eps_mse, x0_sq
        st = torch.zeros(n + 4 * B, dtype=torch.float32, device=dev)
        st[:n].copy_(self.q_sample(x0, tab[0], draw(int(ts[0]))).flatten())
        rows = torch.empty(S, 4, B, dtype=torch.float32, device=dev)

        def inputs(i, s):
            # the last step makes no next state: it gets any buffer of the right shape, unread
            z = draw(int(ts[i + 1])) if i + 1 < S else x0
            return (s, tab[i], nxt[i], z, x0) + ((y,) if has_y else ())

        def fn(s, t, tn, z, x0_, yy=None):
            x = s[:n].view(shape)
            pred = model(x, t, yy)
            new = torch.empty_like(s)
            out = new[n:].view(4, B)
            if learned:
                K.vlb_step_learned(x0_, x, self._check_out(pred, x).contiguous().float(), t, coef, clip=clip, z_next=z,
                                   t_next=tn, sa=sa, s1=s1, x_next=new[:n].view(shape),
                                   rows=(out[0], out[1], out[2], out[3]))
                return new
            pred = (self._pred_of(pred, x) if lr else pred).contiguous().float()
            K.vlb_step(x0_, x, pred, t, coef, clip=clip, z_next=z, t_next=tn, sa=sa, s1=s1, x_next=new[:n].view(shape),
                       out=(out[0], out[1], out[2], out[3]))
            return new

        bar = tqdm(total=S, desc='Evaluating bpd')

        def record(i, s):
            bar.update(1)
            rows[i].copy_(s[n:].view(4, B))

        key = ("bpd", self.prediction_type, getattr(self, "variance_type", "fixed"), variance, clip, has_y, tuple(shape), coef.data_ptr(),
               self.alphas_cumprod.data_ptr())
        run_loop(st, S, inputs, fn, StepGraph.eligible(model, x0, True, False), record,
                 cache=cache_for(model, key, self, st), const=(4, 5) if has_y else (4,))
        bar.close()
        A, Bc = _vlb.prior_constants(self.alphas_cumprod.cpu().numpy())
        vb = rows[:, 0].t().contiguous()
        prior = rows[0, 3] * Bc + A
        return {"vb": vb, "xstart_mse": rows[:, 1].t().contiguous(), "eps_mse": rows[:, 2].t().contiguous(),
                "timesteps": walk, "prior_bpd": prior, "total_bpd": vb.sum(1) + prior if S == T else None}
