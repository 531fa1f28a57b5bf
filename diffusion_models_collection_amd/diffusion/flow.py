"""Rectified flow / flow matching: training and Euler / Heun ODE sampling. Not in the reference (Liu et al. 2022,
arXiv:2209.03003; Lipman et al. 2022, arXiv:2210.02747; SiT, arXiv:2401.08740; Esser et al. 2024, arXiv:2403.03206).

The other family of processes beside the variance-preserving DDPM schedules: a linear path x_t = (1 - sigma_t) x0 +
sigma_t eps between data and noise, a velocity target v = eps - x0, and an ODE sampler that needs 10-20 evaluations.
The backbones are untouched: a flow with T discrete noise levels calls model(x, t, y) with the int64 level index, and
the class stands in as a DiffusionTrainer's `diffusion` object (eager step; see graphed_train_step below).

Host side (diffusion/_flow.py): the sigma tables, the inference timesteps and one [R, 4] fp32 row per model evaluation.
Device side, sampling: ONE fused launch per evaluation beside the model (dmc_flow_step: classifier-free guidance, the
Euler / Heun-predictor / Heun-corrector update and the history writes); with a guidance rescale or a dynamic threshold
dmc_flow_guide forms the guided velocity first. The loop state is a [1 or 3, B, C, H, W] tensor, x and for Heun the
interval's start state and first slope: it is the step function's first input and its output, so the history rides
through graph replays (diffusion/_graph.py) and a cached graph that replays from step 0 starts from the caller's fresh
state. One captured step serves every row: the row's kind is data the kernel reads.

Training launches NO new kernel: dmc_q_sample / dmc_pack_input take the two tables (1 - sigma, sigma), and dmc_objective /
dmc_objective_is with DMC_PRED_V and two [T] tables of ones form exactly eps - x0 (multiplying by 1.0f is exact), so the
loss, its gradient, their determinism and the schedule-sampler plumbing are the tested ones of ddpm.py.
"""
import torch
from tqdm import tqdm

from .. import kernels as K
from . import _flow
from ._graph import StepGraph, cache_for, run_loop
from .ddim import DDIM
from .ddpm import ObjectiveMixin, _ObjectiveFn, _ObjectiveISFn, _require_cuda


class RectifiedFlow:
    """Rectified flow with T discrete noise levels; see the module docstring.

    Training needs no kernel of its own, and has none: q_sample is dmc_q_sample on the tables (1 - sigma, sigma), and the
    loss is dmc_objective / dmc_objective_is with DMC_PRED_V on two [T] tables of ones, whose target 1*eps - 1*x0 is
    exactly eps - x0. Sampling adds dmc_flow_step (one launch per model evaluation) and dmc_flow_guide (only under a
    guidance rescale or a dynamic threshold)."""

    SOLVERS = _flow.SOLVERS
    # DiffusionTrainer's captured training step (utils/trainer.py GraphedTrainStep) builds the DDPM objectives only: it
    # would read prediction_type as 'eps' and train the wrong target, so the trainer runs this object's p_losses eagerly
    graphed_train_step = False

    def __init__(self, num_timesteps=1000, num_inference_steps=20, shift=1.0, solver='euler', device='cuda'):
        self.num_timesteps = _flow.check_num_timesteps(num_timesteps)
        self.num_inference_steps = _flow.check_inference_steps(self.num_timesteps, num_inference_steps)
        self.shift = _flow.check_shift(shift)
        self.solver = _flow.check_solver(solver)
        self.device = device
        sig, om = _flow.flow_sigmas(self.num_timesteps, self.shift)
        ts = _flow.flow_timesteps(self.num_timesteps, self.num_inference_steps)
        coef, step_ts = _flow.flow_steps(sig, ts, self.solver)
        self._kinds = coef[:, 3].astype(int).tolist()
        self.sigmas = torch.from_numpy(sig).to(device)
        self.one_minus_sigmas = torch.from_numpy(om).to(device)
        self.inference_timesteps = torch.from_numpy(ts).to(device)
        self.step_timesteps = torch.from_numpy(step_ts).to(device)
        self.step_coefficients = torch.from_numpy(coef).to(device)
        self._ones = torch.ones(self.num_timesteps, dtype=torch.float32, device=device)

    def _tab(self, name, dev):
        v = getattr(self, name)
        if v.device != dev:
            v = v.to(dev)
            setattr(self, name, v)
        return v

    # ------------------------------------------------------------------------------------------------------------
    # training
    # ------------------------------------------------------------------------------------------------------------
    def q_sample(self, x_start, t, noise=None):
        """x_t = (1 - sigma_t) x_0 + sigma_t noise (dmc_q_sample on the flow's two tables)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        _require_cuda(x_start, noise)
        dev = x_start.device
        return K.q_sample(x_start.float(), noise.float(), t.to(dev).long().contiguous(),
                          self._tab("one_minus_sigmas", dev), self._tab("sigmas", dev))

    def _check_out(self, out, x):
        if out.shape[1:] != x.shape[1:]:
            raise ValueError(f"RectifiedFlow needs a model that returns the velocity in the input's shape, got "
                             f"{tuple(out.shape)} for an input {tuple(x.shape)} (a learn_sigma / 2C-channel model has "
                             "no use here: a flow has no variance head)")
        return out

    def p_losses(self, model, x_start, t, y=None, noise=None, loss_type='l2', schedule_sampler=None, snr_gamma=None,
                 vlb_weight=None, return_parts=False):
        """Flow-matching loss: loss_type between model(x_t, t, y) and the velocity noise - x_start. schedule_sampler: the
        sampler t was drawn from (resample.py, e.g. 'logit-normal'); its importance weights (None: the density is the
        weighting) scale the loss and, when grad is enabled, the per-sample losses enter its history."""
        if snr_gamma is not None or vlb_weight is not None or return_parts:
            raise ValueError("RectifiedFlow.p_losses: a flow has no SNR weight or variance head (snr_gamma, vlb_weight "
                             "and return_parts belong to the DDPM family)")
        if loss_type not in ("l1", "l2", "huber"):
            raise ValueError(f"Unknown loss type: {loss_type}")
        if noise is None:
            noise = torch.randn_like(x_start)
        x_noisy = self.q_sample(x_start, t, noise)
        pred = self._check_out(model(x_noisy, t, y), x_start)
        _require_cuda(pred)
        dev = pred.device
        ones = self._tab("_ones", dev)
        t = t.to(dev).long().contiguous()
        args = (pred, x_start.contiguous().float(), noise.contiguous().float(), t, ones, ones, None)
        if schedule_sampler is None:
            return _ObjectiveFn.apply(*args, "v", loss_type)
        loss, row = _ObjectiveISFn.apply(*args, schedule_sampler.weight_table(), "v", loss_type)
        if torch.is_grad_enabled():
            schedule_sampler.update_with_local_losses(t, row)
        return loss

    # ------------------------------------------------------------------------------------------------------------
    # what a flow does not have
    # ------------------------------------------------------------------------------------------------------------
    def _no(self, what):
        raise NotImplementedError(f"RectifiedFlow has no {what}: the editing samplers and the variational bound are "
                                  "built on the DDPM posterior; use DDPM, DDIM or DPMSolver")

    def calc_bpd(self, *args, **kwargs):
        self._no("calc_bpd")

    def img2img(self, *args, **kwargs):
        self._no("img2img")

    def inpaint(self, *args, **kwargs):
        self._no("inpaint")

    def invert(self, *args, **kwargs):
        self._no("invert")

    # ------------------------------------------------------------------------------------------------------------
    # sampling
    # ------------------------------------------------------------------------------------------------------------
    def _step_tables(self, batch_size, dev):
        """([R, B] timesteps, [R, B] row indices into the coefficient table), int64 on dev."""
        ts = self._tab("step_timesteps", dev)
        R = ts.shape[0]
        tab = ts.view(-1, 1).expand(-1, batch_size).contiguous()
        idx = torch.arange(R, dtype=torch.long, device=dev).view(-1, 1).expand(-1, batch_size).contiguous()
        return tab, idx

    def _state(self, img):
        """[1, B, C, H, W] (Euler) or [3, B, C, H, W] (Heun): x_T and an (unread) zero history."""
        st = torch.zeros((3 if self.solver == "heun" else 1,) + tuple(img.shape), dtype=torch.float32,
                         device=img.device)
        st[0].copy_(img)
        return st

    def _update(self, st, pc, pu, scale, k, coef):
        """dmc_flow_step from the loop state into a new one. The history halves of the new state are written by
        predictor rows only, and read by the corrector row that follows one."""
        new = torch.empty_like(st)
        if st.shape[0] == 3:
            K.flow_step(st[0], pc, k, coef, pu=pu, scale=scale, xb=st[1], dprev=st[2], out=new[0], xb_out=new[1],
                        d_out=new[2])
        else:
            K.flow_step(st[0], pc, k, coef, pu=pu, scale=scale, out=new[0])
        return new

    def _step_plain(self, model, st, t, k, y, coef, shared_t):
        x = st[0]
        v = self._check_out(model(x, t[:1] if shared_t else t, y), x)
        _require_cuda(v)
        return self._update(st, v.contiguous().float(), None, 1.0, k, coef)

    def _step_cfg(self, model, st, t, k, y, coef, cfg_scale, p_threshold, guidance_rescale):
        """ONE batched 2B forward (null label 0 in the second half, as DDPM._cfg_eps), its halves read in place."""
        x = st[0]
        B = x.shape[0]
        both = model(torch.cat([x, x], 0), torch.cat([t, t], 0), torch.cat([y, torch.zeros_like(y)], 0))
        _require_cuda(both)
        both = self._check_out(both, x).contiguous().float()
        if p_threshold is None and guidance_rescale == 0:
            return self._update(st, both[:B], both[B:], cfg_scale, k, coef)
        g = K.flow_guide(x, both[:B], both[B:], cfg_scale, guidance_rescale, k, coef,
                         threshold=p_threshold is not None, p_threshold=p_threshold)
        return self._update(st, g, None, 1.0, k, coef)

    def _key(self, tag, coef, *rest):
        return (tag, self.solver, self.shift, self.num_timesteps, self.num_inference_steps, coef.shape[0],
                coef.data_ptr()) + rest

    def _run(self, model, st, inputs, fn, return_all_timesteps, key, const, desc):
        R = len(self._kinds)
        imgs = []
        bar = tqdm(total=R, desc=desc)

        def record(i, s):
            bar.update(1)
            if return_all_timesteps and self._kinds[i] != _flow.KIND_PREDICTOR:     # one image per interval
                imgs.append(s[0].cpu())

        cache = None if return_all_timesteps else cache_for(model, key, self, st)
        st = run_loop(st, R, inputs, fn, StepGraph.eligible(model, st[0], True, False), record, cache=cache,
                      const=const)
        bar.close()
        if return_all_timesteps:
            return torch.stack(imgs, dim=0)
        return st[0]

    def _start(self, shape, x_T):
        img = torch.randn(shape, device=self.device) if x_T is None else x_T.to(self.device).float()
        _require_cuda(img)
        return img.contiguous()

    @torch.no_grad()
    def sample(self, model, shape, y=None, return_all_timesteps=False, x_T=None):
        """R model evaluations, R = len(step_timesteps): S for Euler, 2S - 1 for Heun. return_all_timesteps gives the S
        states at the ends of the intervals."""
        img = self._start(shape, x_T)
        dev = img.device
        tab, idx = self._step_tables(shape[0], dev)
        coef = self._tab("step_coefficients", dev)
        if y is not None:
            y = y.to(dev)
        has_y = y is not None
        shared_t = DDIM._shared_t(model, y)

        def inputs(i, st):
            return (st, tab[i], idx[i]) + ((y,) if has_y else ())

        def fn(st, t, k, yy=None):
            return self._step_plain(model, st, t, k, yy, coef, shared_t)

        key = self._key("flow", coef, shared_t, has_y, None, None, 0.0)
        return self._run(model, self._state(img), inputs, fn, return_all_timesteps, key, (3,) if has_y else (),
                         f"Rectified flow sampling ({self.solver})")

    @torch.no_grad()
    def sample_with_cfg(self, model, shape, y, cfg_scale=3.0, p_threshold=None, return_all_timesteps=False, x_T=None,
                        guidance_rescale=0.0):
        """Classifier-free guidance on the velocity. With p_threshold None and guidance_rescale 0 the guidance happens
        inside dmc_flow_step (one launch beside the 2B forward); otherwise dmc_flow_guide forms the guided velocity
        (guidance_rescale: arXiv:2305.08891 §3.4; p_threshold: the dynamic threshold on the data prediction
        x - sigma v) and dmc_flow_step takes it."""
        if y is None:
            raise ValueError("CFG sampling requires class labels y.")
        if p_threshold is not None and (isinstance(p_threshold, (bool, str, bytes))
                                        or not isinstance(p_threshold, (int, float))
                                        or not 0.0 < float(p_threshold) < 1.0):
            raise ValueError(f"p_threshold must be in (0, 1) or None, got {p_threshold!r}")
        rescale = ObjectiveMixin._guidance_rescale(guidance_rescale)
        p_threshold = None if p_threshold is None else float(p_threshold)
        img = self._start(shape, x_T)
        dev = img.device
        y = y.to(dev)
        tab, idx = self._step_tables(shape[0], dev)
        coef = self._tab("step_coefficients", dev)

        def inputs(i, st):
            return (st, tab[i], idx[i], y)

        def fn(st, t, k, yy):
            return self._step_cfg(model, st, t, k, yy, coef, float(cfg_scale), p_threshold, rescale)

        key = self._key("flow_cfg", coef, False, True, float(cfg_scale), p_threshold, rescale)
        return self._run(model, self._state(img), inputs, fn, return_all_timesteps, key, (3,),
                         f"Rectified flow sampling ({self.solver}) with CFG scale {cfg_scale}")
