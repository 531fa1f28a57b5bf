"""DPM-Solver++ sampler (Lu et al. 2022, arXiv:2211.01095): multistep, data-prediction form, orders 1 and 2 (2M).

Not in the reference, whose samplers are DDPM (1000 evaluations) and DDIM (50). A second-order multistep solver on
a log-SNR grid reaches DDIM-50's discretisation error in about 20 evaluations. The class carries the same tables,
attributes and training methods as DDIM, so it can stand in as a DiffusionTrainer's `diffusion` object.

Host side (diffusion/_dpm.py): the inference timesteps and one [S', 5] fp32 coefficient row per step, computed in
float64 from the fp32 alphas_cumprod table. Device side: ONE fused kernel per step (dmc_dpm_step: x0 prediction,
clamp, update, history write). The loop state is a [2, B, C, H, W] tensor, x and the previous x0 prediction: it is
the step function's first input and its output, so the history rides through graph replays (diffusion/_graph.py)
and a cached graph that replays from step 0 starts from the caller's fresh state. Row 0 has c1 = 0 and never reads
the history, so the same captured step serves every i. CFG reuses dmc_cfg_x0 (guided eps, x0, dynamic threshold)
unchanged and hands its x0 to dmc_dpm_step. With prediction_type='v' (ddpm.py ObjectiveMixin) dmc_pred_convert turns
the model output into that x0 (plain path) or into the two eps halves (CFG) first. sample_with_cfg(guidance_rescale > 0)
takes its x0 from dmc_cfg_guide instead (arXiv:2305.08891 §3.4). A zero-terminal-SNR schedule is refused: the solver
steps in half-log-SNR, which is -inf there.
"""
import torch
from tqdm import tqdm

from .. import kernels as K
from . import _dpm
from ._graph import StepGraph, cache_for, run_loop
from .ddim import DDIM
from .ddpm import _require_cuda


class DPMSolver(DDIM):
    """DPM-Solver++ with DDIM's tables, q_sample / p_losses / _extract and sampling entry points."""

    SPACINGS = _dpm.SPACINGS

    def __init__(self, num_timesteps=1000, num_inference_steps=20, beta_start=0.0001, beta_end=0.02,
                 beta_schedule='linear', solver_order=2, timestep_spacing='logsnr', lower_order_final=True,
                 device='cuda', prediction_type='eps', variance_type='fixed', rescale_zero_snr=False):
        if rescale_zero_snr:
            raise ValueError("DPMSolver has no zero terminal SNR schedule (rescale_zero_snr=True): the solver steps in "
                             "half-log-SNR, which is -inf where alphas_cumprod is 0; use DDIM or DDPM")
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order}")
        if timestep_spacing not in _dpm.SPACINGS:
            raise ValueError(f"Unknown timestep spacing: {timestep_spacing} (expected one of {_dpm.SPACINGS})")
        self.solver_order = solver_order
        self.lower_order_final = bool(lower_order_final)
        super().__init__(num_timesteps, num_inference_steps, beta_start, beta_end, beta_schedule, eta=0.0,
                         device=device, prediction_type=prediction_type, variance_type=variance_type,
                         timestep_spacing=timestep_spacing)

    def _setup_inference_timesteps(self):
        """num_inference_steps keeps the request; with 'logsnr' len(inference_timesteps) can be below it."""
        ac = self.alphas_cumprod.cpu().numpy()
        ts = _dpm.dpm_timesteps(self.num_timesteps, self.num_inference_steps, self.timestep_spacing, ac)
        coef = _dpm.dpm_coefficients(ac, ts, self.solver_order, self.lower_order_final)
        self.inference_timesteps = torch.from_numpy(ts).to(self.device)
        self.step_coefficients = torch.from_numpy(coef).to(self.device)
        self.__dict__.pop("_truncated", None)

    def p_sample(self, *args, **kwargs):
        raise NotImplementedError("DPMSolver is a multistep solver: a step needs the previous x0 prediction; use "
                                  "sample / sample_with_cfg (kernels.dpm_step is the single update)")

    def _step_tables(self, batch_size, dev):
        """([S', B] timesteps, [S', B] row indices into the coefficient table), int64 on dev."""
        ts = self.inference_timesteps.to(dev)
        S = ts.shape[0]
        tab = ts.view(-1, 1).expand(-1, batch_size).contiguous()
        idx = torch.arange(S, dtype=torch.long, device=dev).view(-1, 1).expand(-1, batch_size).contiguous()
        return tab, idx

    @staticmethod
    def _state(img):
        """[2, B, C, H, W]: x_T and an (unread) zero history."""
        st = torch.zeros((2,) + tuple(img.shape), dtype=torch.float32, device=img.device)
        st[0].copy_(img)
        return st

    def _key(self, tag, coef, *rest):
        return (tag, self.prediction_type, self.variance_type, self.solver_order, self.timestep_spacing, self.lower_order_final,
                coef.shape[0], coef.data_ptr()) + rest

    def _run(self, model, st, S, inputs, fn, return_all_timesteps, key, const, desc):
        imgs = []
        bar = tqdm(total=S, desc=desc)

        def record(i, s):
            bar.update(1)
            if return_all_timesteps:
                imgs.append(s[0].cpu())

        cache = None if return_all_timesteps else cache_for(model, key, self, st)
        st = run_loop(st, S, inputs, fn, StepGraph.eligible(model, st[0], True, False), record, cache=cache,
                      const=const)
        bar.close()
        if return_all_timesteps:
            return torch.stack(imgs, dim=0)
        return st[0]

    def _step_plain(self, model, st, t, k, y, coef, shared_t, clip=True):
        """One step of sample(): shared with img2img / inpaint."""
        x = st[0]
        eps = self._pred_of(model(x, t[:1] if shared_t else t, y), x)    # learned_range: v is ignored, one copy
        new = torch.empty_like(st)
        if self.prediction_type == "v":
            _, x0 = self._convert(eps, x, t)
            K.dpm_step(x, None, k, coef, clip=clip, x0=x0, x0_prev=st[1], out=new[0], x0_out=new[1])
        else:
            K.dpm_step(x, eps.contiguous().float(), k, coef, clip=clip, x0_prev=st[1], out=new[0], x0_out=new[1])
        return new

    def _step_cfg(self, model, st, t, k, y, coef, cfg_scale, p_threshold, guidance_rescale=0.0):
        """One step of sample_with_cfg(): shared with img2img / inpaint."""
        x = st[0]
        if self._use_guide(guidance_rescale):
            _, x0, _ = self._cfg_guide(model, x, t, y, cfg_scale, guidance_rescale, p_threshold, want_eps=False)
        else:
            eps_c, eps_u = self._cfg_pair(model, x, t, y)
            _, x0 = K.cfg_x0(x, eps_c.contiguous(), eps_u.contiguous(), cfg_scale, t,
                             self._tab("alphas_cumprod", x.device), None, 0, p_threshold)
        new = torch.empty_like(st)
        K.dpm_step(x, None, k, coef, clip=False, x0=x0, x0_prev=st[1], out=new[0], x0_out=new[1])
        return new

    _edit_state = _state

    @staticmethod
    def _edit_image(st):
        return st[0]

    def _edit_resample(self, resample):
        if resample != 1:
            raise ValueError("DPMSolver.inpaint: resample must be 1 (the multistep history does not survive a "
                             "re-noise); use DDIM or DDPM to resample")

    def _truncated_coefficients(self, i0, dev):
        """The coefficient rows for the timesteps from i0 on, rebuilt so that the first executed row is first order
        (it has no history); built once per i0."""
        if i0 == 0:
            return self._tab("step_coefficients", dev)
        cache = self.__dict__.setdefault("_truncated", {})     # dropped with the timestep list
        c = cache.get(i0)
        if c is None or c.device != dev:
            coef = _dpm.dpm_coefficients(self.alphas_cumprod.cpu().numpy(), self.inference_timesteps[i0:].cpu().numpy(),
                                         self.solver_order, self.lower_order_final)
            c = cache[i0] = torch.from_numpy(coef).to(dev)
        return c

    def _edit_step(self, model, B, dev, y, cfg_scale, p_threshold, i0):
        """For _edit_loop.EditMixin: (inference timesteps from i0 on, j -> the j-th of those steps' device inputs,
        step(state, args, y, z), no noise drawn, the graph key's tail)."""
        tab, idx = self._step_tables(B, dev)
        tab = tab[i0:]
        coef = self._truncated_coefficients(i0, dev)
        shared_t = self._shared_t(model, y)

        def step(st, args, yy, z):
            if cfg_scale is None:
                return self._step_plain(model, st, args[0], args[1], yy, coef, shared_t)
            return self._step_cfg(model, st, args[0], args[1], yy, coef, cfg_scale, p_threshold)

        key = self._key("dpm", coef, shared_t, y is not None, cfg_scale, p_threshold, self.alphas_cumprod.data_ptr())
        return self.inference_timesteps[i0:].cpu().numpy(), (lambda j: (tab[j], idx[j])), step, False, key

    def invert(self, *args, **kwargs):
        raise NotImplementedError("DPMSolver has no inversion: the multistep update is not the eta = 0 DDIM map run "
                                  "backwards; use DDIM.invert")

    @torch.no_grad()
    def sample(self, model, shape, y=None, return_all_timesteps=False, x_T=None, clip_denoised=True):
        """S' model evaluations, S' = len(inference_timesteps); the last one returns its x0 prediction."""
        batch_size = shape[0]
        img = torch.randn(shape, device=self.device) if x_T is None else x_T.to(self.device).float()
        _require_cuda(img)
        dev = img.device
        tab, idx = self._step_tables(batch_size, dev)
        coef = self._tab("step_coefficients", dev)
        S = coef.shape[0]
        if y is not None:
            y = y.to(dev)
        has_y = y is not None
        clip = bool(clip_denoised)
        shared_t = self._shared_t(model, y)

        def inputs(i, st):
            return (st, tab[i], idx[i]) + ((y,) if has_y else ())

        def fn(st, t, k, yy=None):
            return self._step_plain(model, st, t, k, yy, coef, shared_t, clip)

        key = self._key("dpm", coef, clip, shared_t, has_y, self.alphas_cumprod.data_ptr())
        return self._run(model, self._state(img), S, inputs, fn, return_all_timesteps, key,
                         (3,) if has_y else (), 'DPM-Solver++ Sampling')

    @torch.no_grad()
    def sample_with_cfg(self, model, shape, y, cfg_scale=3.0, p_threshold=0.995, return_all_timesteps=False,
                        x_T=None, guidance_rescale=0.0):
        """Classifier-free guidance + dynamic thresholding as DDIM.sample_with_cfg: one 2B forward, dmc_cfg_x0 (with
        guidance_rescale > 0: dmc_cfg_guide) for the guided, thresholded x0, then the solver update from that x0."""
        if y is None:
            raise ValueError("CFG sampling requires class labels y.")
        if p_threshold is not None and not (0.0 < float(p_threshold) < 1.0):
            raise ValueError("p_threshold must be in (0, 1) or None")
        rescale = self._guidance_rescale(guidance_rescale)
        batch_size = shape[0]
        img = torch.randn(shape, device=self.device) if x_T is None else x_T.to(self.device).float()
        _require_cuda(img)
        dev = img.device
        y = y.to(dev)
        tab, idx = self._step_tables(batch_size, dev)
        coef = self._tab("step_coefficients", dev)
        ac = self._tab("alphas_cumprod", dev)
        S = coef.shape[0]

        def inputs(i, st):
            return (st, tab[i], idx[i], y)

        def fn(st, t, k, yy):
            return self._step_cfg(model, st, t, k, yy, coef, cfg_scale, p_threshold, rescale)

        key = self._key("dpm_cfg", coef, float(cfg_scale), p_threshold, rescale, ac.data_ptr())
        return self._run(model, self._state(img), S, inputs, fn, return_all_timesteps, key, (3,),
                         f"DPM-Solver++ sampling with CFG scale {cfg_scale}")
