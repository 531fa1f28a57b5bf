"""DDPM scheduler with the reference API (diffusion/ddpm.py of sunyzhi55/Diffusion_Models_Collection).

Same constructor (:27-34), attributes (betas, alphas_cumprod, ... :38-71) and methods (q_sample :84,
p_losses :106, _extract :142, p_mean_variance :151, p_sample :197, sample :222, sample_with_cfg :254).
Arithmetic runs in fused HIP kernels (libdmc.so):
  q_sample            -> dmc_q_sample
  p_losses loss       -> dmc_loss_fwd / dmc_loss_bwd (deterministic reduction), via _LossFn
  p_sample / mean     -> dmc_ddpm_step (x0 prediction, clip, posterior mean, noise, one launch)
  CFG + threshold     -> dmc_cfg_x0 (combine, x0, per-row quantile, clamp, one launch)
  v / min-SNR loss    -> dmc_objective (target, weight, loss and gradient in one pass), via _ObjectiveFn
  v model output      -> dmc_pred_convert (eps and x0 for the step kernels, one launch after the model call)
The cond/uncond forwards of CFG are batched into ONE 2B forward.

Schedule tables are built on the host by _schedule.py: the reference's op sequence as explicit IEEE fp32
numpy arithmetic (the same bits on any host whose libm log/cos are accurate to 64 double ulps: _schedule.py),
then uploaded once.

Extra optional keyword arguments (not in the reference, all default to the reference behaviour):
p_sample(noise=...), sample(x_T=...), sample_with_cfg(x_T=...) inject the Gaussian draws for parity tests.
DDPM(prediction_type='v') trains and samples a v-prediction network (arXiv:2202.00512), p_losses(snr_gamma=...)
weights each sample by min-SNR-gamma (arXiv:2303.09556); see _objective.py. With the defaults neither launches
anything new. img2img / inpaint (not in the reference either; _edit_loop.EditMixin, _edit.py, dmc_known_blend) run the
steps of sample / sample_with_cfg from, or around, a given image. calc_bpd (not in the reference; _likelihood.LikelihoodMixin,
_vlb.py, dmc_vlb_step) evaluates the variational bound in bits per dimension.
DDPM(variance_type='learned_range') (not in the reference; arXiv:2102.09672 §3.1) takes a model that returns 2C channels,
the prediction and the log-variance interpolation v:
  hybrid loss         -> dmc_hybrid_objective (L_simple + vlb_weight * L_vlb, both halves' gradient, one pass), via _HybridFn
  p_sample / mean     -> dmc_ddpm_step_learned (both halves of the model output read in place, the model's own sigma)
  calc_bpd 'learned'  -> dmc_vlb_step_learned
With the default 'fixed' nothing new is launched.
p_losses(schedule_sampler=...) (not in the reference; arXiv:2102.09672 §3.3, resample.py) weights each sample by the
sampler's importance weight and feeds its loss history:
  any loss            -> dmc_objective_is / dmc_hybrid_objective_is (the same kernels with iw[t] and the per-sample loss), via
                         _ObjectiveISFn / _HybridISFn, then dmc_ts_history_update
Without a sampler nothing new is launched.
DDPM(rescale_zero_snr=True) (not in the reference; arXiv:2305.08891) rescales the schedule to zero terminal SNR
(_schedule.build_tables; 'v' and 'fixed' only: ObjectiveMixin._set_types), and sample_with_cfg(guidance_rescale=...)
rescales the guided prediction:
  CFG on such a schedule, or rescaled -> dmc_cfg_guide (guidance, rescale, eps and x0 from the model's own 2B-row output,
                                         threshold: one launch where dmc_pred_convert + dmc_cfg_x0 stand)
With the defaults nothing new is launched.
"""
import numpy as np
import torch
import torch.nn.functional as F
from tqdm import tqdm

from .. import kernels as K
from . import _objective, _schedule, _vlb
from ._edit_loop import EditMixin
from ._graph import StepGraph, run_loop
from ._likelihood import LikelihoodMixin


def make_betas(num_timesteps, beta_start, beta_end, beta_schedule):
    """Beta schedule (diffusion/ddpm.py:39-46, cosine :73-82) as an fp32 CPU tensor (see _schedule.py)."""
    return torch.from_numpy(_schedule.make_betas(num_timesteps, beta_start, beta_end, beta_schedule))


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the diffusion hot path runs on the MI355X HIP kernels only: use cuda tensors")


class _LossFn(torch.autograd.Function):
    """F.l1_loss / F.mse_loss / F.smooth_l1_loss(noise, pred) with a fused fwd/bwd (ddpm.py:130-139)."""

    @staticmethod
    def forward(ctx, pred, target, loss_type):
        pred = pred.contiguous().float()
        target = target.contiguous().float()
        ctx.save_for_backward(pred, target)
        ctx.loss_type = loss_type
        return K.loss_fwd(loss_type, pred, target)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        g = g.contiguous().float()
        dpred = K.loss_bwd(ctx.loss_type, pred, target, g)
        dtarget = -dpred if ctx.needs_input_grad[1] else None
        return dpred, dtarget, None


def diffusion_loss(pred, target, loss_type):
    if loss_type not in ("l1", "l2", "huber"):
        raise ValueError(f"Unknown loss type: {loss_type}")
    return _LossFn.apply(pred, target, loss_type)


class _ObjectiveFn(torch.autograd.Function):
    """The loss for a v target and / or per-sample weights (dmc_objective): the forward is the kernel without a
    gradient output, the backward the same kernel with the upstream scalar."""

    @staticmethod
    def forward(ctx, pred, x0, noise, t, sa, s1, w, pred_type, loss_type):
        pred = pred.contiguous().float()
        ctx.save_for_backward(pred, x0, noise, t, sa, s1, w)
        ctx.types = (pred_type, loss_type)
        return K.objective(pred_type, loss_type, pred, x0, noise, t, sa, s1, w, grad=False)[0]

    @staticmethod
    def backward(ctx, g):
        pred, x0, noise, t, sa, s1, w = ctx.saved_tensors
        _, dpred = K.objective(*ctx.types, pred, x0, noise, t, sa, s1, w, dloss=g.contiguous().float())
        return (dpred,) + (None,) * 8


class _HybridFn(torch.autograd.Function):
    """L_hybrid of a network with a variance head (dmc_hybrid_objective), in the shape of _ObjectiveFn: the forward is the
    kernel without a gradient output, the backward the same kernel with the upstream scalar. Returns (total, simple,
    vlb); only the total carries a gradient."""

    @staticmethod
    def forward(ctx, out, x0, noise, t, sa, s1, w, coef, pred_type, loss_type, vlb_weight):
        out = out.contiguous().float()
        ctx.save_for_backward(out, x0, noise, t, sa, s1, w, coef)
        ctx.args = (pred_type, loss_type, vlb_weight)
        loss = K.hybrid_objective(pred_type, loss_type, out, x0, noise, t, sa, s1, coef, w, vlb_weight, grad=False)[0]
        total, simple, vlb = loss[0], loss[1], loss[2]
        ctx.mark_non_differentiable(simple, vlb)
        return total, simple, vlb

    @staticmethod
    def backward(ctx, g, *_):
        out, x0, noise, t, sa, s1, w, coef = ctx.saved_tensors
        pred_type, loss_type, vlb_weight = ctx.args
        _, dout = K.hybrid_objective(pred_type, loss_type, out, x0, noise, t, sa, s1, coef, w, vlb_weight,
                                     dloss=g.contiguous().float())
        return (dout,) + (None,) * 10


class _ObjectiveISFn(torch.autograd.Function):
    """_ObjectiveFn under a schedule sampler (dmc_objective_is): iw is the sampler's [T] importance weights (None: 1).
    Returns (loss, row_loss); row_loss, each sample's own loss before iw, carries no gradient."""

    @staticmethod
    def forward(ctx, pred, x0, noise, t, sa, s1, w, iw, pred_type, loss_type):
        pred = pred.contiguous().float()
        ctx.save_for_backward(pred, x0, noise, t, sa, s1, w, iw)
        ctx.types = (pred_type, loss_type)
        loss, row, _ = K.objective_is(pred_type, loss_type, pred, x0, noise, t, sa, s1, w, iw, grad=False)
        ctx.mark_non_differentiable(row)
        return loss, row

    @staticmethod
    def backward(ctx, g, *_):
        pred, x0, noise, t, sa, s1, w, iw = ctx.saved_tensors
        _, _, dpred = K.objective_is(*ctx.types, pred, x0, noise, t, sa, s1, w, iw, dloss=g.contiguous().float(),
                                     row_loss=False)
        return (dpred,) + (None,) * 9


class _HybridISFn(torch.autograd.Function):
    """_HybridFn under a schedule sampler (dmc_hybrid_objective_is). Returns (total, simple, vlb, row_loss); only the
    total carries a gradient."""

    @staticmethod
    def forward(ctx, out, x0, noise, t, sa, s1, w, iw, coef, pred_type, loss_type, vlb_weight):
        out = out.contiguous().float()
        ctx.save_for_backward(out, x0, noise, t, sa, s1, w, iw, coef)
        ctx.args = (pred_type, loss_type, vlb_weight)
        loss, row, _ = K.hybrid_objective_is(pred_type, loss_type, out, x0, noise, t, sa, s1, coef, w, iw, vlb_weight,
                                             grad=False)
        total, simple, vlb = loss[0], loss[1], loss[2]
        ctx.mark_non_differentiable(simple, vlb, row)
        return total, simple, vlb, row

    @staticmethod
    def backward(ctx, g, *_):
        out, x0, noise, t, sa, s1, w, iw, coef = ctx.saved_tensors
        pred_type, loss_type, vlb_weight = ctx.args
        _, _, dout = K.hybrid_objective_is(pred_type, loss_type, out, x0, noise, t, sa, s1, coef, w, iw, vlb_weight,
                                           dloss=g.contiguous().float(), row_loss=False)
        return (dout,) + (None,) * 11


class ObjectiveMixin:
    """prediction_type, variance_type, the min-SNR weight tables and the launches they need, shared by DDPM and DDIM
    (and so DPMSolver): both carry sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod and _tab()."""

    prediction_type = "eps"
    variance_type = "fixed"
    rescale_zero_snr = False

    def _set_types(self, prediction_type, variance_type):
        """Both types, checked together: a zero-terminal-SNR schedule (alphas_cumprod[T-1] = 0) has no eps form at
        T-1 and no learned-variance table (_vlb.learned_coefficients needs 0 < alphas_cumprod)."""
        prediction_type = _objective.check_prediction_type(prediction_type)
        variance_type = _vlb.check_variance_type(variance_type)
        if self.rescale_zero_snr and (prediction_type != "v" or variance_type != "fixed"):
            raise ValueError("a zero terminal SNR schedule (rescale_zero_snr=True) needs prediction_type='v' and "
                             f"variance_type='fixed', got {prediction_type!r} and {variance_type!r}: eps is not "
                             "defined where alphas_cumprod is 0")
        self.prediction_type, self.variance_type = prediction_type, variance_type

    @staticmethod
    def _guidance_rescale(guidance_rescale):
        """guidance_rescale as a float; ValueError unless it is a number in [0, 1] (arXiv:2305.08891 uses 0.7)."""
        g = guidance_rescale
        if isinstance(g, (bool, str, bytes)) or not isinstance(g, (int, float)) or not 0.0 <= float(g) <= 1.0:
            raise ValueError(f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}")
        return float(g)

    def set_prediction_type(self, prediction_type):
        """'eps' or 'v'. Drops the sampler's cached step graphs (their steps were captured for the old type)."""
        self._set_types(prediction_type, self.variance_type)
        self.__dict__.pop("_step_graphs", None)

    def set_variance_type(self, variance_type):
        """'fixed', or 'learned_range': the model returns 2C channels, the prediction and the variance interpolation v
        (arXiv:2102.09672 §3.1). Drops the sampler's cached step graphs, as set_prediction_type does."""
        self._set_types(self.prediction_type, variance_type)
        self.__dict__.pop("_step_graphs", None)

    def _lvar_table(self, dev):
        """[T, 8] fp32 device table of _vlb.learned_coefficients, built and uploaded once per prediction type."""
        cache = self.__dict__.setdefault("_lvar_tables", {})
        c = cache.get(self.prediction_type)
        if c is None or c.device != dev:
            c = cache[self.prediction_type] = torch.from_numpy(
                _vlb.learned_coefficients(self.alphas_cumprod.cpu().numpy(), self.prediction_type)).to(dev)
        return c

    @staticmethod
    def _vlb_weight(vlb_weight):
        w = 0.001 if vlb_weight is None else vlb_weight      # the paper's lambda
        if isinstance(w, (bool, str)) or not isinstance(w, (int, float)) or not 0.0 <= float(w) < float("inf"):
            raise ValueError(f"vlb_weight must be a finite number >= 0, got {vlb_weight!r}")
        return float(w)

    def _check_out(self, out, x):
        """A learned_range model returns [B', 2C, ...] for x = [B, C, ...] (B' = 2B under CFG)."""
        if out.dim() != x.dim() or out.shape[1] != 2 * x.shape[1] or out.shape[2:] != x.shape[2:]:
            raise ValueError(f"variance_type='learned_range' needs a model output with {2 * x.shape[1]} channels "
                             f"(prediction, then v), got {tuple(out.shape)} for an input {tuple(x.shape)}")
        return out

    def _pred_of(self, out, x):
        """The prediction of a model output: the output itself, or for learned_range its first C channels as ONE
        contiguous copy (the samplers with a sigma of their own, DDIM and DPM-Solver, ignore v)."""
        if self.variance_type != "learned_range":
            return out
        return self._check_out(out, x)[:, :x.shape[1]].contiguous()

    def _losses(self, out, x_start, noise, t, loss_type, snr_gamma, vlb_weight, return_parts, schedule_sampler=None):
        """p_losses after the model call."""
        if schedule_sampler is not None:
            return self._sampled_losses(out, x_start, noise, t, loss_type, snr_gamma, vlb_weight, return_parts,
                                        schedule_sampler)
        if self.variance_type != "learned_range":
            if vlb_weight is not None or return_parts:
                raise ValueError("vlb_weight and return_parts need variance_type='learned_range'")
            if self._default_objective(snr_gamma):
                return diffusion_loss(out, noise, loss_type)
            return self._objective_loss(out, x_start, noise, t, loss_type, snr_gamma)
        if loss_type not in ("l1", "l2", "huber"):
            raise ValueError(f"Unknown loss type: {loss_type}")
        vw = self._vlb_weight(vlb_weight)
        _require_cuda(out, x_start, noise)
        self._check_out(out, x_start)
        dev = out.device
        w = None if snr_gamma is None else self._snr_weights(snr_gamma, dev)
        total, simple, vlb = _HybridFn.apply(
            out, x_start.contiguous().float(), noise.contiguous().float(), t.to(dev).long().contiguous(),
            self._tab("sqrt_alphas_cumprod", dev), self._tab("sqrt_one_minus_alphas_cumprod", dev), w,
            self._lvar_table(dev), self.prediction_type, loss_type, vw)
        return (total, simple, vlb) if return_parts else total

    def _sampled_losses(self, out, x_start, noise, t, loss_type, snr_gamma, vlb_weight, return_parts, sampler):
        """_losses under a schedule sampler: every objective, the default one included, goes through the _is kernels with
        the sampler's importance weights, and (when grad is enabled) the per-sample losses feed the sampler's history."""
        learned = self.variance_type == "learned_range"
        if not learned and (vlb_weight is not None or return_parts):
            raise ValueError("vlb_weight and return_parts need variance_type='learned_range'")
        if loss_type not in ("l1", "l2", "huber"):
            raise ValueError(f"Unknown loss type: {loss_type}")
        _require_cuda(out, x_start, noise)
        dev = out.device
        w = None if snr_gamma is None else self._snr_weights(snr_gamma, dev)
        iw = sampler.weight_table()
        t = t.to(dev).long().contiguous()
        args = (x_start.contiguous().float(), noise.contiguous().float(), t, self._tab("sqrt_alphas_cumprod", dev),
                self._tab("sqrt_one_minus_alphas_cumprod", dev), w, iw)
        if learned:
            self._check_out(out, x_start)
            total, simple, vlb, row = _HybridISFn.apply(out, *args, self._lvar_table(dev), self.prediction_type,
                                                        loss_type, self._vlb_weight(vlb_weight))
            res = (total, simple, vlb) if return_parts else total
        else:
            res, row = _ObjectiveISFn.apply(out, *args, self.prediction_type, loss_type)
        if torch.is_grad_enabled():
            sampler.update_with_local_losses(t, row)
        return res

    def _snr_weights(self, gamma, dev):
        """[T] fp32 device table of min-SNR-gamma weights for the current prediction type, built and uploaded once
        per (gamma, prediction type)."""
        key = (_objective.check_gamma(gamma), self.prediction_type)
        cache = self.__dict__.setdefault("_snr_tables", {})
        w = cache.get(key)
        if w is None or w.device != dev:
            w = torch.from_numpy(_objective.min_snr_weights(self.alphas_cumprod.cpu().numpy(), *key,
                                                            zero_terminal=self.rescale_zero_snr)).to(dev)
            cache[key] = w
        return w

    def _default_objective(self, snr_gamma):
        return self.prediction_type == "eps" and snr_gamma is None

    def _objective_loss(self, pred, x_start, noise, t, loss_type, snr_gamma):
        if loss_type not in ("l1", "l2", "huber"):
            raise ValueError(f"Unknown loss type: {loss_type}")
        _require_cuda(pred, x_start, noise)
        dev = pred.device
        w = None if snr_gamma is None else self._snr_weights(snr_gamma, dev)
        return _ObjectiveFn.apply(pred, x_start.contiguous().float(), noise.contiguous().float(),
                                  t.to(dev).long().contiguous(), self._tab("sqrt_alphas_cumprod", dev),
                                  self._tab("sqrt_one_minus_alphas_cumprod", dev), w, self.prediction_type, loss_type)

    def _convert(self, out, x, t, want_x0=True):
        """(eps, x0 or None) from a v-prediction model output; out may hold 2B rows (CFG)."""
        _require_cuda(x, out)
        dev = x.device
        return K.pred_convert("v", x.contiguous().float(), t.to(dev).long().contiguous(),
                              self._tab("sqrt_alphas_cumprod", dev), self._tab("sqrt_one_minus_alphas_cumprod", dev),
                              out.contiguous().float(), want_x0=want_x0)

    def _cfg_pair(self, model, img, t, y):
        """DDPM._cfg_eps for either prediction type: a v output is converted to eps (both halves, one launch)
        before the guidance, which is affine with coefficients summing to 1 and so commutes with the conversion."""
        return self._cfg_pair_out(model, img, t, y)[:2]

    def _cfg_pair_out(self, model, img, t, y):
        """(eps_cond, eps_uncond, the batched model output). With learned_range the two prediction halves are copied
        contiguous first (one launch); the output's first B rows carry the conditional v, read in place by the step."""
        B = img.shape[0]
        if self.prediction_type == "eps" and self.variance_type == "fixed":
            return DDPM._cfg_eps(model, img, t, y) + (None,)
        both = model(torch.cat([img, img], 0), torch.cat([t, t], 0), torch.cat([y, torch.zeros_like(y)], 0))
        eps = self._pred_of(both, img)
        if self.prediction_type == "v":
            eps, _ = self._convert(eps, img, t, want_x0=False)
        return eps[:B], eps[B:], both

    def _use_guide(self, guidance_rescale):
        """dmc_cfg_guide stands in for the dmc_pred_convert + dmc_cfg_x0 path when the guidance is rescaled or the
        schedule reaches alphas_cumprod = 0 (which that path cannot represent); otherwise the step is unchanged."""
        return guidance_rescale > 0 or self.rescale_zero_snr

    def _cfg_guide(self, model, img, t, y, cfg_scale, guidance_rescale, p_threshold, want_eps=True):
        """(guided eps or None, guided and thresholded x0, the batched model output): ONE 2B forward, then ONE
        dmc_cfg_guide launch that reads the conditional and unconditional rows (for learned_range their prediction
        channels) in place."""
        B, C = img.shape[0], img.shape[1]
        both = model(torch.cat([img, img], 0), torch.cat([t, t], 0), torch.cat([y, torch.zeros_like(y)], 0))
        _require_cuda(img, both)
        both = both.contiguous().float()
        pred = self._check_out(both, img)[:, :C] if self.variance_type == "learned_range" else both
        dev = img.device
        eps, x0 = K.cfg_guide(self.prediction_type, img.contiguous().float(), pred[:B], pred[B:], cfg_scale,
                              guidance_rescale, t.to(dev).long().contiguous(), self._tab("sqrt_alphas_cumprod", dev),
                              self._tab("sqrt_one_minus_alphas_cumprod", dev), p_threshold, want_eps=want_eps)
        return eps, x0, both


class DDPM(ObjectiveMixin, EditMixin, LikelihoodMixin):
    """DDPM diffusion process (diffusion/ddpm.py:15-332)."""

    def __init__(self, num_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', device='cuda',
                 prediction_type='eps', variance_type='fixed', rescale_zero_snr=False):
        self.rescale_zero_snr = bool(rescale_zero_snr)
        self._set_types(prediction_type, variance_type)
        self.num_timesteps = num_timesteps
        self.device = device
        tabs = _schedule.build_tables(num_timesteps, beta_start, beta_end, beta_schedule,
                                      zero_terminal_snr=self.rescale_zero_snr)
        for k, v in tabs.items():
            setattr(self, k, torch.from_numpy(v).to(device))

    def _cosine_beta_schedule(self, timesteps, s=0.008, device='cuda'):
        return make_betas(timesteps, 0, 0, "cosine").to(device)

    def _tab(self, name, dev):
        v = getattr(self, name)
        if v.device != dev:
            v = v.to(dev)
            setattr(self, name, v)
        return v

    def q_sample(self, x_start, t, noise=None):
        """q(x_t | x_0) = sqrt(ac[t]) x_0 + sqrt(1 - ac[t]) noise (diffusion/ddpm.py:84-104)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        _require_cuda(x_start, noise)
        dev = x_start.device
        return K.q_sample(x_start.float(), noise.float(), t.to(dev).long().contiguous(),
                          self._tab("sqrt_alphas_cumprod", dev), self._tab("sqrt_one_minus_alphas_cumprod", dev))

    def p_losses(self, model, x_start, t, y=None, noise=None, loss_type='l2', snr_gamma=None, vlb_weight=None,
                 return_parts=False, schedule_sampler=None):
        """Training loss (diffusion/ddpm.py:106-140). Not in the reference: snr_gamma (min-SNR-gamma weighting) and
        the v target of prediction_type='v', both through dmc_objective; with variance_type='learned_range' the
        hybrid loss L_simple + vlb_weight * L_vlb (arXiv:2102.09672 eq. 16; vlb_weight None: 0.001) through
        dmc_hybrid_objective, and return_parts=True gives (total, simple, vlb_weight * L_vlb). schedule_sampler: the
        sampler t was drawn from (resample.py); the loss is then weighted by its importance weights and, when grad is
        enabled, the per-sample losses enter its history."""
        if noise is None:
            noise = torch.randn_like(x_start)
        x_noisy = self.q_sample(x_start, t, noise)
        predicted_noise = model(x_noisy, t, y)
        return self._losses(predicted_noise, x_start, noise, t, loss_type, snr_gamma, vlb_weight, return_parts,
                            schedule_sampler)

    def _extract(self, a, t, x_shape):
        batch_size = t.shape[0]
        a = a.to(t.device)
        out = a[t]
        return out.reshape(batch_size, *((1,) * (len(x_shape) - 1)))

    def _step(self, x, eps, t, clip, x0_pred, z):
        dev = x.device
        return K.ddpm_step(x.contiguous().float(), eps.contiguous().float(), t.to(dev).long().contiguous(),
                           self._tab("sqrt_recip_alphas_cumprod", dev), self._tab("sqrt_recipm1_alphas_cumprod", dev),
                           self._tab("posterior_mean_coef1", dev), self._tab("posterior_mean_coef2", dev),
                           self._tab("posterior_log_variance_clipped", dev), clip=clip,
                           x0=None if x0_pred is None else x0_pred.contiguous().float(),
                           z=None if z is None else z.contiguous().float())

    def _learned_inputs(self, model, x, t, y, eps, x0_pred, model_out):
        """(model output, eps or None, x0 or None) of a learned_range step: the output's halves are read in place by
        dmc_ddpm_step_learned unless an eps is given (guidance) or the prediction is v (converted from one contiguous
        copy of the prediction half)."""
        if eps is None:
            model_out = model(x, t, y)
            if self.prediction_type == "v":
                eps, x0_pred = self._convert(self._pred_of(model_out, x), x, t)
        elif model_out is None:
            raise ValueError("variance_type='learned_range': an eps given to the step needs model_out, the model "
                             "output whose second half is v")
        _require_cuda(x, model_out)
        return self._check_out(model_out, x).contiguous().float(), eps, x0_pred

    def _step_learned(self, x, out, t, clip, eps, x0_pred, z):
        dev = x.device
        return K.ddpm_step_learned(x.contiguous().float(), out, t.to(dev).long().contiguous(),
                                   self._tab("sqrt_recip_alphas_cumprod", dev),
                                   self._tab("sqrt_recipm1_alphas_cumprod", dev),
                                   self._tab("posterior_mean_coef1", dev), self._tab("posterior_mean_coef2", dev),
                                   self._lvar_table(dev), clip=clip,
                                   eps=None if eps is None else eps.contiguous().float(),
                                   x0=None if x0_pred is None else x0_pred.contiguous().float(),
                                   z=None if z is None else z.contiguous().float())

    def p_mean_variance(self, model, x, t, y=None, clip_denoised=True, eps=None, x0_pred=None, model_out=None):
        """Posterior mean / variance / log-variance (diffusion/ddpm.py:151-195). With learned_range the variance is the
        model's: exp(lv_min + (v + 1)/2 * R) per element, of the model output's second half."""
        if self.variance_type == "learned_range":
            out, eps, x0_pred = self._learned_inputs(model, x, t, y, eps, x0_pred, model_out)
            mean = self._step_learned(x, out, t, clip_denoised, eps, x0_pred, None)
            tab = self._lvar_table(x.device)
            logvar = (self._extract(tab[:, _vlb.L_LVMIN], t, x.shape)
                      + (out[:, x.shape[1]:] + 1.0) * 0.5 * self._extract(tab[:, _vlb.L_R], t, x.shape))
            return mean, logvar.exp(), logvar
        if eps is None:
            eps = model(x, t, y)
            if self.prediction_type == "v":
                eps, x0_pred = self._convert(eps, x, t)
        _require_cuda(x, eps)
        mean = self._step(x, eps, t, clip_denoised, x0_pred, None)
        var = self._extract(self.posterior_variance, t, x.shape)
        logvar = self._extract(self.posterior_log_variance_clipped, t, x.shape)
        return mean, var, logvar

    @torch.no_grad()
    def p_sample(self, model, x, t, y=None, clip_denoised=True, eps=None, x0_pred=None, noise=None, model_out=None):
        """x_{t-1} ~ p(x_{t-1} | x_t) (diffusion/ddpm.py:197-220), one fused kernel after the model call. With
        learned_range the noise is scaled by the model's own standard deviation (dmc_ddpm_step_learned); a given eps
        then comes with model_out, the model output that carries v."""
        if self.variance_type == "learned_range":
            out, eps, x0_pred = self._learned_inputs(model, x, t, y, eps, x0_pred, model_out)
            if noise is None:
                noise = torch.randn_like(x)
            _require_cuda(x, noise)
            return self._step_learned(x, out, t, clip_denoised, eps, x0_pred, noise)
        if eps is None:
            eps = model(x, t, y)
            if self.prediction_type == "v":
                eps, x0_pred = self._convert(eps, x, t)
        if noise is None:
            noise = torch.randn_like(x)
        _require_cuda(x, eps, noise)
        return self._step(x, eps, t, clip_denoised, x0_pred, noise)

    def _noise(self, noise, i, x):
        """Loop step i's Gaussian draw: the injected noise[i] (parity tests) or torch.randn_like(x)."""
        if noise is None:
            return torch.randn_like(x)
        return noise(i) if callable(noise) else noise[i].to(x.device)

    def _step_plain(self, model, x, t, y, z):
        """One step of sample(): shared with img2img / inpaint."""
        return self.p_sample(model, x, t, y, noise=z)

    def _step_cfg(self, model, x, t, y, z, cfg_scale, p_threshold, guidance_rescale=0.0):
        """One step of sample_with_cfg(): shared with img2img / inpaint."""
        dev = x.device
        if self._use_guide(guidance_rescale):
            eps_g, x0, both = self._cfg_guide(model, x, t, y, cfg_scale, guidance_rescale, p_threshold)
        else:
            eps_c, eps_u, both = self._cfg_pair_out(model, x, t, y)
            eps_g, x0 = K.cfg_x0(x.contiguous(), eps_c.contiguous(), eps_u.contiguous(), cfg_scale, t,
                                 self._tab("sqrt_recip_alphas_cumprod", dev),
                                 self._tab("sqrt_recipm1_alphas_cumprod", dev), 1, p_threshold)
        # learned_range: the variance is the conditional half's (DiT's convention), the output's first B rows
        cond = both[:x.shape[0]] if self.variance_type == "learned_range" else None
        return self.p_sample(model, x, t, y=None, clip_denoised=False, eps=eps_g, x0_pred=x0, noise=z, model_out=cond)

    def _edit_steps(self):
        return self.num_timesteps

    def _edit_step(self, model, B, dev, y, cfg_scale, p_threshold, i0):
        """For _edit_loop.EditMixin: (timesteps T-1-i0 .. 0, j -> the j-th of those steps' device inputs,
        step(x, args, y, z), the step draws noise, the graph key's tail)."""
        T = self.num_timesteps
        ts = np.arange(T - 1 - i0, -1, -1, dtype=np.int64)
        tab = torch.from_numpy(ts).to(dev).view(-1, 1).expand(-1, B).contiguous()

        def step(x, args, yy, z):
            if cfg_scale is None:
                return self._step_plain(model, x, args[0], yy, z)
            return self._step_cfg(model, x, args[0], yy, z, cfg_scale, p_threshold)

        key = ("ddpm", self.prediction_type, self.variance_type, T, y is not None, cfg_scale, p_threshold, self.alphas_cumprod.data_ptr())
        return ts, (lambda j: (tab[j],)), step, True, key

    @torch.no_grad()
    def sample(self, model, shape, y=None, return_all_timesteps=False, x_T=None, noise=None):
        """Ancestral sampling over all timesteps (diffusion/ddpm.py:222-252). Optional (not in the reference):
        x_T, and noise = [T, B, C, H, W] tensor or callable i -> tensor, the z of loop step i (t = T-1-i).
        Steps after the first replay one captured HIP graph (diffusion/_graph.py)."""
        batch_size = shape[0]
        device = self.device
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        T = self.num_timesteps
        ts = torch.arange(T, device=img.device).view(-1, 1).expand(-1, batch_size).contiguous()
        imgs = []
        bar = tqdm(total=T, desc='Sampling')

        def inputs(i, x):
            return x, ts[T - 1 - i], self._noise(noise, i, x)

        def fn(x, t, z):
            return self._step_plain(model, x, t, y, z)

        def record(i, x):
            bar.update(1)
            if return_all_timesteps:
                imgs.append(x.cpu())

        img = run_loop(img, T, inputs, fn, StepGraph.eligible(model, img, True, False), record)
        bar.close()
        if return_all_timesteps:
            return torch.stack(imgs, dim=0)
        return img

    @staticmethod
    def _cfg_eps(model, img, t, y):
        """eps_cond and eps_uncond from ONE batched forward (cond rows first, null label 0 second)."""
        B = img.shape[0]
        both = model(torch.cat([img, img], 0), torch.cat([t, t], 0), torch.cat([y, torch.zeros_like(y)], 0))
        return both[:B], both[B:]

    @torch.no_grad()
    def sample_with_cfg(self, model, shape, y, cfg_scale=3.0, p_threshold=0.995, return_all_timesteps=False,
                        x_T=None, noise=None, guidance_rescale=0.0):
        """Classifier-free guidance + dynamic thresholding (diffusion/ddpm.py:254-332); x_T / noise as sample().
        guidance_rescale (not in the reference; arXiv:2305.08891 §3.4, in [0, 1], the paper uses 0.7) pulls the guided
        prediction's per-sample standard deviation towards the conditional one's; above 0, or on a zero-terminal-SNR
        schedule, the step's guidance is ONE dmc_cfg_guide launch on the model's own output."""
        if y is None:
            raise ValueError("CFG sampling requires class labels y.")
        if p_threshold is not None and not (0.0 < float(p_threshold) < 1.0):
            raise ValueError("p_threshold must be in (0, 1) or None")
        rescale = self._guidance_rescale(guidance_rescale)
        batch_size = shape[0]
        device = self.device
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        imgs = []
        y = y.to(img.device)
        dev = img.device
        T = self.num_timesteps
        ts = torch.arange(T, device=dev).view(-1, 1).expand(-1, batch_size).contiguous()
        bar = tqdm(total=T, desc=f'DDPM Sampling with CFG scale {cfg_scale}')

        def inputs(i, x):
            return x, ts[T - 1 - i], self._noise(noise, i, x)

        def fn(x, t, z):
            return self._step_cfg(model, x, t, y, z, cfg_scale, p_threshold, rescale)

        def record(i, x):
            bar.update(1)
            if return_all_timesteps:
                imgs.append(x.cpu())

        img = run_loop(img, T, inputs, fn, StepGraph.eligible(model, img, True, False), record)
        bar.close()
        if return_all_timesteps:
            return torch.stack(imgs, dim=0)
        return img
