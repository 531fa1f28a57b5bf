"""img2img and inpaint for DDPM, DDIM and DPMSolver (not in the reference): the loops around each sampler's own step.

A sampler hands over its step through _edit_step(): the per-step device inputs, the step function its sample /
sample_with_cfg loops run, and whether that step draws noise. The loops here add what editing needs: the start from a
noised image (img2img) and ONE dmc_known_blend launch after every step (inpaint), inside the same replayed step graph
(diffusion/_graph.py). The given image and the mask are const graph inputs, the blend's row index is a device tensor,
so one captured graph serves every entry of the walk; every random draw happens eagerly outside the graph, in walk
order: the step's z, the known region's z, the re-noise z2.
"""
import collections

import torch
from tqdm import tqdm

from .. import kernels as K
from . import _edit
from ._graph import StepGraph, cache_for, run_loop

_TABLES_MAX = 4      # blend tables kept per sampler (one per timestep list)


def _check_cfg(y, cfg_scale, p_threshold):
    """sample_with_cfg's refusals; None runs the plain step."""
    if cfg_scale is None:
        return None
    if y is None:
        raise ValueError("CFG sampling requires class labels y.")
    if p_threshold is not None and not (0.0 < float(p_threshold) < 1.0):
        raise ValueError("p_threshold must be in (0, 1) or None")
    return float(cfg_scale)


def _drawer(noise):
    """draw(j, which, like): the injected noise(j, which) or torch.randn_like."""
    def draw(j, which, like):
        if noise is None:
            return torch.randn_like(like)
        return noise(j, which).to(like.device).float().contiguous()
    return draw


class EditMixin:
    """Needs the sampler's alphas_cumprod, device, q_sample, _tab and _edit_step (and, for a loop state that is more
    than the image, _edit_state / _edit_image)."""

    @staticmethod
    def _edit_state(img):
        return img

    @staticmethod
    def _edit_image(st):
        return st

    def _refuse_zero_terminal(self, what):
        """The blend table (_edit.blend_coefficients) needs 0 < alphas_cumprod along the walk, and an image noised to
        T-1 of a zero terminal SNR schedule is pure noise: nothing of it is left to edit."""
        if getattr(self, "rescale_zero_snr", False):
            raise ValueError(f"{what} is not defined on a zero terminal SNR schedule (rescale_zero_snr=True): "
                             "alphas_cumprod[T-1] is 0")

    def _edit_input(self, image):
        if image.dim() != 4:
            raise ValueError(f"image must be [B, C, H, W], got {tuple(image.shape)}")
        image = image.to(self.device).float().contiguous()
        if not image.is_cuda:
            raise RuntimeError("the diffusion hot path runs on the MI355X HIP kernels only: use cuda tensors")
        return image

    def _blend_table(self, ts, dev):
        """(host [2S, 4] fp32 table, its device copy) for the timestep list ts, built once per list."""
        cache = self.__dict__.setdefault("_blend_tables", collections.OrderedDict())
        key = ts.tobytes()
        hit = cache.get(key)
        if hit is None or hit[1].device != dev:
            host = _edit.blend_coefficients(self.alphas_cumprod.cpu().numpy(), ts)
            hit = cache[key] = (host, torch.from_numpy(host).to(dev))
            while len(cache) > _TABLES_MAX:
                cache.popitem(last=False)
        return hit

    def _edit_run(self, model, st, n, inputs, fn, key, const, return_all_timesteps, desc):
        imgs = []
        bar = tqdm(total=n, desc=desc)

        def record(j, s):
            bar.update(1)
            if return_all_timesteps:
                imgs.append(self._edit_image(s).cpu())

        x = self._edit_image(st)
        cache = None if return_all_timesteps else cache_for(model, key, self, st)
        st = run_loop(st, n, inputs, fn, StepGraph.eligible(model, x, True, False), record, cache=cache, const=const)
        bar.close()
        if return_all_timesteps:
            return torch.stack(imgs, dim=0)
        return self._edit_image(st)

    @torch.no_grad()
    def img2img(self, model, image, strength=0.5, y=None, cfg_scale=None, p_threshold=0.995, noise=None,
                return_all_timesteps=False):
        """Image-to-image (SDEdit, arXiv:2108.01073): the image noised to the timestep of step i0 =
        _edit.start_index(S, strength) of the sampler's list, then steps i0 .. S-1 of sample (cfg_scale None) or
        sample_with_cfg. noise: callable (j, which) -> tensor, which = 'start' (j = 0) or 'step' (the j-th executed
        step's z, for a sampler that draws one); None draws torch.randn_like."""
        self._refuse_zero_terminal("img2img")
        cfg = _check_cfg(y, cfg_scale, p_threshold)
        image = self._edit_input(image)
        dev, B = image.device, image.shape[0]
        if y is not None:
            y = y.to(dev)
        S = self._edit_steps()
        i0 = _edit.start_index(S, strength)
        ts, args, step, draws, key = self._edit_step(model, B, dev, y, cfg, p_threshold, i0)
        draw = _drawer(noise)
        t0 = torch.full((B,), int(ts[0]), dtype=torch.long, device=dev)
        st = self._edit_state(self.q_sample(image, t0, draw(0, "start", image)))
        has_y = y is not None

        def inputs(j, s):
            z = (draw(j, "step", image),) if draws else ()
            return (s,) + args(j) + ((y,) if has_y else ()) + z

        n_args = len(args(0))

        def fn(s, *a):
            return step(s, a[:n_args], a[n_args] if has_y else None, a[-1] if draws else None)

        return self._edit_run(model, st, len(ts), inputs, fn, ("img2img", i0) + key, (1 + n_args,) if has_y else (),
                              return_all_timesteps, "img2img")

    def _edit_mask(self, mask, shape):
        """[B, 1, H, W] or [B, C, H, W] fp32 on the device from anything that broadcasts to one of them."""
        B, C, H, W = shape
        mask = torch.as_tensor(mask).to(self.device).float()
        for target in ((B, 1, H, W), (B, C, H, W)):
            try:
                if tuple(torch.broadcast_shapes(tuple(mask.shape), target)) == target:
                    mask = mask.expand(target).contiguous()
                    break
            except RuntimeError:
                pass
        else:
            raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to {(B, 1, H, W)} or {(B, C, H, W)}")
        if not bool(((mask >= 0) & (mask <= 1)).all()):      # once per call; NaN fails it too
            raise ValueError("mask values must lie in [0, 1] (1 keeps the given image)")
        return mask

    @torch.no_grad()
    def inpaint(self, model, image, mask, y=None, cfg_scale=None, p_threshold=0.995, resample=1, x_T=None,
                noise=None, return_all_timesteps=False):
        """Inpainting (RePaint, arXiv:2201.09865): mask = 1 keeps the given image, the rest is generated. Every entry
        of _edit.edit_walk(S, 0, resample) is the model, the sampler's step kernel and one dmc_known_blend launch
        with row 2i + renoise of _edit.blend_coefficients. noise: callable (j, which) -> tensor for walk entry j,
        which = 'start' (j = 0, without x_T), 'step', 'known', 'renoise', asked for in that order and only where the
        entry reads the draw; None draws torch.randn_like."""
        self._refuse_zero_terminal("inpaint")
        cfg = _check_cfg(y, cfg_scale, p_threshold)
        image = self._edit_input(image)
        dev, B = image.device, image.shape[0]
        mask = self._edit_mask(mask, image.shape)
        if y is not None:
            y = y.to(dev)
        S = self._edit_steps()
        walk = _edit.edit_walk(S, 0, resample)
        self._edit_resample(resample)
        ts, args, step, draws, key = self._edit_step(model, B, dev, y, cfg, p_threshold, 0)
        host, coef = self._blend_table(ts, dev)
        rows = torch.arange(2 * S, dtype=torch.long, device=dev).view(-1, 1).expand(-1, B).contiguous()
        draw = _drawer(noise)
        if x_T is None:
            x = draw(0, "start", image)
        else:
            x = x_T.to(dev).float()
            if x.shape != image.shape:
                raise ValueError(f"x_T {tuple(x.shape)} is not the image's shape {tuple(image.shape)}")
        has_y = y is not None
        n_args = len(args(0))

        def inputs(j, s):
            i, renoise = walk[j]
            r = 2 * i + renoise
            z = (draw(j, "step", image),) if draws else ()
            # a row that reads no noise gets any buffer of the right shape: the tuple keeps its arity
            zk = draw(j, "known", image) if host[r, 1] != 0 else image
            z2 = draw(j, "renoise", image) if host[r, 3] != 0 else image
            return (s,) + args(i) + ((y,) if has_y else ()) + z + (image, mask, rows[r], zk, z2)

        def fn(s, *a):
            sa, (img0, m, row, zk, z2) = a[:-5], a[-5:]
            new = step(s, sa[:n_args], sa[n_args] if has_y else None, sa[-1] if draws else None)
            xi = self._edit_image(new)
            K.known_blend(xi, img0, m, row, coef, z=zk, z2=z2, out=xi)
            return new

        p_img = 1 + n_args + has_y + draws
        const = ((1 + n_args,) if has_y else ()) + (p_img, p_img + 1)
        return self._edit_run(model, self._edit_state(x), len(walk), inputs, fn,
                              ("inpaint", mask.shape[1], coef.data_ptr()) + key, const, return_all_timesteps,
                              "inpaint")

    def _edit_resample(self, resample):
        """A sampler whose step cannot be repeated after a re-noise refuses resample > 1 here."""
