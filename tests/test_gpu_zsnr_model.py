"""Zero-terminal-SNR schedules, trailing timesteps and rescaled guidance through the samplers and the loss, in small
loops (B = 4, S = 10): against the kernels composed by hand (bitwise), against the float64 numpy loop of
tests/zsnr_reference.py (criterion 2 of test_gpu_elem_kernels), finite from the first step, where alphas_cumprod is 0,
and graph replay against the eager loop on the tiny conditional UNet. The elementwise model is the exact denoiser of
N(0, s2 I) data in v form; its data variance depends on the label, so guidance has something to guide.

Every input builder and reference runs on the CPU alone: cpu_selfcheck() calls them all without a GPU.
"""
import functools

import numpy as np
import pytest
import torch

import zsnr_reference as Z
from test_gpu_dpm import GaussianDenoiser
from test_gpu_elem_kernels import DEV, F32, F64, dev, judge, rng, sqrt_cr

pytestmark = pytest.mark.gpu

SHAPE = (4, 3, 8, 8)
S2 = (0.5, 0.25, 2.0, 1.0, 4.0)      # data variance by label; label 0 is the null label of CFG
Y = (1, 2, 3, 4)
STEPS = 10


def _K():
    from diffusion_models_collection_amd import kernels as K
    return K


def _D():
    from diffusion_models_collection_amd import diffusion
    return diffusion


class GaussianV(GaussianDenoiser):
    """v of the exact denoiser for N(0, S2[y] I) data (y None: S2[0]) on a sampler's own alphas_cumprod table: the op
    sequence of zsnr_reference.gaussian_v in torch ops on the device, finite at alphas_cumprod = 0."""

    def __init__(self, alphas_cumprod):
        a = alphas_cumprod.detach().cpu().float()
        self.a, self.sa, self.s1 = dev(a), dev(sqrt_cr(a)), dev(sqrt_cr(1 - a))
        self.s2 = dev(torch.tensor(S2, dtype=F32))

    def __call__(self, x, t, y=None):
        pick = lambda tab: tab[t].view(-1, 1, 1, 1)   # noqa: E731
        s2 = self.s2[0] if y is None else self.s2[y].view(-1, 1, 1, 1)
        return Z.gaussian_v(x, pick(self.a), pick(self.sa), pick(self.s1), s2)


@functools.lru_cache(maxsize=None)
def x_T():
    """|x_T| in [0.5, 1.5): away from 0, as test_gpu_dpm.gauss_xT."""
    g = rng(177)
    sign = torch.randint(0, 2, SHAPE, generator=g).float() * 2 - 1
    return sign * (0.5 + torch.rand(SHAPE, generator=g))


def _ddim(spacing="trailing", zero=True, **kw):
    return _D().DDIM(1000, STEPS, device=DEV, prediction_type=kw.pop("prediction_type", "v"), rescale_zero_snr=zero,
                     timestep_spacing=spacing, **kw)


def _tabs(smp):
    return smp.sqrt_alphas_cumprod, smp.sqrt_one_minus_alphas_cumprod


def _t(v):
    return torch.full((SHAPE[0],), int(v), dtype=torch.long, device=DEV)


# ------------------------------------------------------------------------------------------------------------
# plain sampling
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["linspace", "trailing"])
def test_ddim_zero_snr_sample(spacing):
    """DDIM(rescale_zero_snr=True, 'v').sample: the kernels composed by hand bit for bit, the float64 loop under
    criterion 2 per sample, every step finite, the first included (alphas_cumprod[999] = 0)."""
    K = _K()
    smp = _ddim(spacing)
    ts = smp.inference_timesteps.cpu().numpy()
    assert ts[0] == 999 and float(smp.alphas_cumprod[999]) == 0.0
    assert ts[-1] == (0 if spacing == "linspace" else 99) and len(ts) == STEPS
    model = GaussianV(smp.alphas_cumprod)
    xT = dev(x_T())
    got = smp.sample(model, SHAPE, x_T=xT, clip_denoised=False)
    steps = smp.sample(model, SHAPE, x_T=xT, clip_denoised=False, return_all_timesteps=True)
    assert steps.shape == (STEPS,) + SHAPE and bool(steps.isfinite().all())
    assert torch.equal(steps[-1], got.cpu())

    sa, s1 = _tabs(smp)
    x = xT
    for i, t in enumerate(ts):
        tn = ts[i + 1] if i + 1 < len(ts) else -1
        eps, x0 = K.pred_convert("v", x, _t(t), sa, s1, model(x, _t(t)))
        x = K.ddim_step(x, eps, _t(t), _t(tn), smp.alphas_cumprod, eta=0.0, clip=False, x0=x0)
        assert torch.equal(x.cpu(), steps[i]), f"step {i} (t = {t}) is not the hand composition"

    ac = smp.alphas_cumprod.cpu().numpy()
    ref32 = Z.ddim_v_loop(np.float32, x_T().numpy(), Z.gaussian_v_fn(np.float32, ac, ts, S2[0]), ac, ts)
    ref64 = Z.ddim_v_loop(np.float64, x_T().numpy(), Z.gaussian_v_fn(np.float64, ac, ts, S2[0]), ac, ts)
    judge(f"zero-SNR DDIM {spacing}", got, torch.from_numpy(ref32), torch.from_numpy(ref64), rows=SHAPE[0])
    # the default clip and labels run too
    y = dev(torch.tensor(Y))
    assert bool(smp.sample(model, SHAPE, y, x_T=xT).isfinite().all())


def test_ddim_invert_then_sample_is_finite():
    """DDIM.invert on the rescaled schedule: the last upward jump lands on alphas_cumprod = 0, where the step kernel's
    r2 = -inf is clamped and out = 0 * x0 + 1 * eps. Every state finite, equal to the hand composition, and sampling
    from the latent is finite at every step."""
    K = _K()
    smp = _ddim("trailing")
    model = GaussianV(smp.alphas_cumprod)
    image = dev(x_T() * 0.5)
    up = smp.invert(model, image, return_all_timesteps=True)
    assert bool(up.isfinite().all()) and up.shape[0] == STEPS - 1
    ts = smp.inference_timesteps.cpu().numpy()[::-1]
    sa, s1 = _tabs(smp)
    x = image
    for k in range(STEPS - 1):
        eps, x0 = K.pred_convert("v", x, _t(ts[k]), sa, s1, model(x, _t(ts[k])))
        x = K.ddim_step(x, eps, _t(ts[k]), _t(ts[k + 1]), smp.alphas_cumprod, eta=0.0, clip=False, x0=x0)
        assert torch.equal(x.cpu(), up[k]), f"inversion step {k}"
    assert ts[-1] == 999 and torch.equal(x, eps)          # the state at T-1 is the last eps, exactly
    back = smp.sample(model, SHAPE, x_T=dev(up[-1]), clip_denoised=False, return_all_timesteps=True)
    assert bool(back.isfinite().all())


# ------------------------------------------------------------------------------------------------------------
# guidance
# ------------------------------------------------------------------------------------------------------------
def _hand_guide(K, smp, model, x, t, y, scale, phi, p, want_eps=True):
    B = x.shape[0]
    both = model(torch.cat([x, x], 0), torch.cat([t, t], 0), torch.cat([y, torch.zeros_like(y)], 0))
    sa, s1 = _tabs(smp)
    return K.cfg_guide(smp.prediction_type, x, both[:B], both[B:], scale, phi, t, sa, s1, p, want_eps=want_eps)


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("p", [0.995, None])
def test_ddim_zero_snr_cfg(phi, p):
    """DDIM.sample_with_cfg on the rescaled schedule (guidance_rescale 0 too: the eps-form path cannot represent it):
    model -> cfg_guide -> ddim_step composed by hand, bit for bit at every step."""
    K = _K()
    smp = _ddim("trailing")
    model = GaussianV(smp.alphas_cumprod)
    xT, y = dev(x_T()), dev(torch.tensor(Y))
    steps = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, p_threshold=p, x_T=xT, guidance_rescale=phi,
                                return_all_timesteps=True)
    assert bool(steps.isfinite().all())
    ts = smp.inference_timesteps.cpu().numpy()
    x = xT
    for i, t in enumerate(ts):
        tn = ts[i + 1] if i + 1 < len(ts) else -1
        eps, x0 = _hand_guide(K, smp, model, x, _t(t), y, 3.0, phi, p)
        x = K.ddim_step(x, eps, _t(t), _t(tn), smp.alphas_cumprod, eta=0.0, clip=False, x0=x0)
        assert torch.equal(x.cpu(), steps[i]), f"step {i} (t = {t})"
    got = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, p_threshold=p, x_T=xT, guidance_rescale=phi)
    assert torch.equal(got.cpu(), steps[-1])
    if phi > 0:
        other = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, p_threshold=p, x_T=xT)
        assert not torch.equal(other, got)            # the rescale did take part


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_ddpm_zero_snr_cfg(phi):
    """DDPM with T = 12 on its own rescaled table, noise injected: model -> cfg_guide -> ddpm_step by hand, bitwise."""
    K = _K()
    T = 12
    smp = _D().DDPM(T, device=DEV, prediction_type="v", rescale_zero_snr=True)
    assert float(smp.alphas_cumprod[T - 1]) == 0.0 and bool(smp.sqrt_recip_alphas_cumprod[T - 1].isinf())
    model = GaussianV(smp.alphas_cumprod)
    xT, y = dev(x_T()), dev(torch.tensor(Y))
    noise = torch.randn((T,) + SHAPE, generator=rng(178)).to(DEV)
    steps = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, x_T=xT, noise=noise, guidance_rescale=phi,
                                return_all_timesteps=True)
    assert bool(steps.isfinite().all())
    x = xT
    for i in range(T):
        t = _t(T - 1 - i)
        eps, x0 = _hand_guide(K, smp, model, x, t, y, 3.0, phi, 0.995)
        x = K.ddpm_step(x, eps, t, smp.sqrt_recip_alphas_cumprod, smp.sqrt_recipm1_alphas_cumprod,
                        smp.posterior_mean_coef1, smp.posterior_mean_coef2, smp.posterior_log_variance_clipped,
                        clip=False, x0=x0, z=noise[i])
        assert torch.equal(x.cpu(), steps[i]), f"step {i}"
    # plain ancestral sampling on the same schedule is finite from the first step as well
    plain = smp.sample(model, SHAPE, y, x_T=xT, noise=noise, return_all_timesteps=True)
    assert bool(plain.isfinite().all())


@pytest.mark.parametrize("pred_type", ["eps", "v"])
def test_ddpm_learned_range_guidance_rescale(pred_type):
    """DDPM(variance_type='learned_range') on an ordinary schedule with guidance_rescale = 0.7: dmc_cfg_guide reads the
    prediction channels of the 2B-row, 2C-channel output in place (row stride 2 * per), and the step still takes the
    conditional rows' v: model -> cfg_guide -> ddpm_step_learned by hand, bitwise."""
    K = _K()
    T, B, C = 12, SHAPE[0], SHAPE[1]
    smp = _D().DDPM(T, device=DEV, prediction_type=pred_type, variance_type="learned_range")
    inner = GaussianV(smp.alphas_cumprod)
    model = lambda x, t, y=None: torch.cat([inner(x, t, y), torch.tanh(x)], 1)   # noqa: E731
    xT, y = dev(x_T()), dev(torch.tensor(Y))
    noise = torch.randn((T,) + SHAPE, generator=rng(181)).to(DEV)
    steps = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, x_T=xT, noise=noise, guidance_rescale=0.7,
                                return_all_timesteps=True)
    assert bool(steps.isfinite().all())
    sa, s1 = _tabs(smp)
    x = xT
    for i in range(T):
        t = _t(T - 1 - i)
        both = model(torch.cat([x, x], 0), torch.cat([t, t], 0), torch.cat([y, torch.zeros_like(y)], 0))
        pc, pu = both[:B, :C], both[B:, :C]
        assert not pc.is_contiguous() and pc.stride(0) == 2 * x[0].numel()
        eps, x0 = K.cfg_guide(pred_type, x, pc, pu, 3.0, 0.7, t, sa, s1, 0.995)
        x = K.ddpm_step_learned(x, both[:B].contiguous(), t, smp.sqrt_recip_alphas_cumprod,
                                smp.sqrt_recipm1_alphas_cumprod, smp.posterior_mean_coef1, smp.posterior_mean_coef2,
                                smp._lvar_table(x.device), clip=False, eps=eps, x0=x0, z=noise[i])
        assert torch.equal(x.cpu(), steps[i]), f"step {i}"
    other = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, x_T=xT, noise=noise)
    assert not torch.equal(other.cpu(), steps[-1])


@pytest.mark.parametrize("pred_type", ["eps", "v"])
def test_dpm_cfg_guidance_rescale(pred_type):
    """DPMSolver.sample_with_cfg(guidance_rescale=0.7) on an ordinary schedule: model -> cfg_guide (no eps wanted) ->
    dpm_step by hand, bit for bit."""
    K = _K()
    smp = _D().DPMSolver(1000, STEPS, device=DEV, prediction_type=pred_type)
    model = GaussianV(smp.alphas_cumprod)       # read as eps it is just another elementwise function of (x, t, y)
    xT, y = dev(x_T()), dev(torch.tensor(Y))
    steps = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, x_T=xT, guidance_rescale=0.7, return_all_timesteps=True)
    assert bool(steps.isfinite().all())
    ts = smp.inference_timesteps.cpu().numpy()
    coef = smp.step_coefficients
    x, prev = xT, torch.zeros_like(xT)
    for i, t in enumerate(ts):
        _, x0 = _hand_guide(K, smp, model, x, _t(t), y, 3.0, 0.7, 0.995, want_eps=False)
        x, prev = K.dpm_step(x, None, _t(i), coef, clip=False, x0=x0, x0_prev=prev)
        assert torch.equal(x.cpu(), steps[i]), f"step {i} (t = {t})"
    other = smp.sample_with_cfg(model, SHAPE, y, cfg_scale=3.0, x_T=xT)
    assert not torch.equal(other.cpu(), steps[-1])


@pytest.mark.parametrize("pred_type", ["eps", "v"])
def test_guidance_rescale_zero_is_todays_path(pred_type, monkeypatch):
    """On an ordinary schedule guidance_rescale = 0 gives the bits of the call without the argument, and never
    launches dmc_cfg_guide."""
    K = _K()
    D = _D()
    xT, y = dev(x_T()), dev(torch.tensor(Y))
    noise = torch.randn((12,) + SHAPE, generator=rng(179)).to(DEV)
    samplers = [(D.DDIM(1000, STEPS, device=DEV, prediction_type=pred_type), {}),
                (D.DDPM(12, device=DEV, prediction_type=pred_type), {"noise": noise}),
                (D.DPMSolver(1000, STEPS, device=DEV, prediction_type=pred_type), {})]
    base = []
    for smp, kw in samplers:
        base.append(smp.sample_with_cfg(GaussianV(smp.alphas_cumprod), SHAPE, y, cfg_scale=3.0, x_T=xT, **kw))

    def refuse(*a, **k):
        raise AssertionError("dmc_cfg_guide launched with guidance_rescale = 0 on an ordinary schedule")

    monkeypatch.setattr(K, "cfg_guide", refuse)
    for (smp, kw), ref in zip(samplers, base):
        for phi in (0.0, 0):
            got = smp.sample_with_cfg(GaussianV(smp.alphas_cumprod), SHAPE, y, cfg_scale=3.0, x_T=xT,
                                      guidance_rescale=phi, **kw)
            assert bool(got.isfinite().all()) and torch.equal(got, ref), type(smp).__name__


# ------------------------------------------------------------------------------------------------------------
# the tiny conditional UNet: replay equals eager
# ------------------------------------------------------------------------------------------------------------
def test_unet_graph_replay_equals_eager(monkeypatch):
    """DDIM-10 (trailing, zero SNR, 'v') and DDPM with T = 12 on the tiny conditional UNet, eval mode, B = 4: sample,
    and sample_with_cfg with guidance_rescale 0 and 0.7 -- the replayed step (2B forward, dmc_cfg_guide, step kernel)
    gives the eager loop's bits, finite; the rescale is part of the graph key (0.7 after 0 is not 0's graph)."""
    from test_gpu_model import build
    m, _ = build("unet_tiny_cond")
    m.eval()
    shape = (4, 3, 16, 16)
    xT = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(41))
    y = torch.tensor(Y, device=DEV)
    noise = torch.randn((12,) + shape, device=DEV, generator=torch.Generator(DEV).manual_seed(42))
    ddim = _ddim("trailing")
    ddpm = _D().DDPM(12, device=DEV, prediction_type="v", rescale_zero_snr=True)

    def run(graph):
        monkeypatch.setenv("DMC_GRAPH", graph)
        return (ddim.sample(m, shape, y, x_T=xT),
                ddim.sample_with_cfg(m, shape, y, x_T=xT, guidance_rescale=0.0),
                ddim.sample_with_cfg(m, shape, y, x_T=xT, guidance_rescale=0.7),
                ddim.sample_with_cfg(m, shape, y, x_T=xT, guidance_rescale=0.7),      # the kept graph, from step 0
                ddpm.sample_with_cfg(m, shape, y, x_T=xT, noise=noise, guidance_rescale=0.7))

    eager = run("0")
    assert not ddim.__dict__.get("_step_graphs")
    graphed = run("1")
    assert ddim.__dict__.get("_step_graphs")
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert bool(a.isfinite().all()) and torch.equal(a, b), i
    assert not torch.equal(graphed[1], graphed[2]) and torch.equal(graphed[2], graphed[3])


# ------------------------------------------------------------------------------------------------------------
# the loss
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_inputs():
    g = rng(180)
    x0 = torch.rand(SHAPE, generator=g) * 2 - 1
    noise, pred = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    return x0, noise, pred, torch.tensor([999, 0, 400, 998])


@pytest.mark.parametrize("gamma", [None, 5])
@pytest.mark.parametrize("cls", ["DDPM", "DDIM"])
def test_p_losses_on_zero_snr_schedule(cls, gamma):
    """p_losses, 'v', rescaled schedule, t = {T-1, 0, 400, T-2}, with and without snr_gamma = 5: the loss and its
    gradient with respect to the prediction against the float64 restatement (criterion 2; ref32 the same in fp32)."""
    smp = getattr(_D(), cls)(device=DEV, prediction_type="v", rescale_zero_snr=True)
    x0, noise, pred, t = loss_inputs()
    leaf = dev(pred).requires_grad_(True)
    loss = smp.p_losses(lambda x, tt, yy: leaf, dev(x0), dev(t), noise=dev(noise), snr_gamma=gamma)
    loss.backward()
    ac = smp.alphas_cumprod.cpu().numpy()
    w = None if gamma is None else Z.ref_min_snr_v(ac, float(gamma))
    flat = lambda v: v.reshape(SHAPE[0], -1).numpy()   # noqa: E731
    refs = [Z.v_loss(flat(pred), flat(x0), flat(noise), t.numpy(), ac, w, dt) for dt in (np.float32, np.float64)]
    judge(f"{cls} zero-SNR v loss gamma={gamma}", loss.detach().reshape(1), torch.tensor([refs[0][0]]),
          torch.tensor([refs[1][0]], dtype=F64))
    judge(f"{cls} zero-SNR v loss gradient gamma={gamma}", leaf.grad, torch.from_numpy(refs[0][1]),
          torch.from_numpy(refs[1][1]), rows=SHAPE[0])
    assert bool(loss.isfinite()) and bool(leaf.grad.isfinite().all())
    if gamma is not None:
        assert bool((leaf.grad[0] == 0).all()) and bool((leaf.grad[1] != 0).any())     # min(a, gamma (1 - a)) = 0 at T-1


def test_target_at_terminal_step_is_minus_x0():
    """At T-1 of the rescaled schedule q_sample returns the noise itself and the v target is -x0: the loss of the
    prediction -x0 is exactly 0."""
    smp = _D().DDPM(device=DEV, prediction_type="v", rescale_zero_snr=True)
    x0, noise, _, _ = loss_inputs()
    t = _t(999)
    assert torch.equal(smp.q_sample(dev(x0), t, dev(noise)).cpu(), noise)
    loss = smp.p_losses(lambda x, tt, yy: -dev(x0), dev(x0), t, noise=dev(noise))
    assert float(loss) == 0.0


def cpu_selfcheck():
    """The builders and the numpy loops the tests above compare with, on the CPU: finite on the rescaled table from
    the first step, the two precisions agree to rounding, and the loss restatement's two precisions too."""
    from diffusion_models_collection_amd.diffusion import _schedule as S
    ac = S.build_tables(1000, 1e-4, 0.02, "linear", zero_terminal_snr=True)["alphas_cumprod"]
    for ts in (S.trailing_timesteps(1000, STEPS), S.ddim_timesteps(1000, STEPS)):
        tr = []
        r32 = Z.ddim_v_loop(np.float32, x_T().numpy(), Z.gaussian_v_fn(np.float32, ac, ts, S2[0]), ac, ts, tr)
        r64 = Z.ddim_v_loop(np.float64, x_T().numpy(), Z.gaussian_v_fn(np.float64, ac, ts, S2[0]), ac, ts)
        assert all(bool(np.isfinite(v).all()) for v in tr) and r32.dtype == np.float32
        assert float(np.abs(r32 - r64).max()) < 1e-5
    x0, noise, pred, t = loss_inputs()
    flat = lambda v: v.reshape(SHAPE[0], -1).numpy()   # noqa: E731
    w = Z.ref_min_snr_v(ac, 5.0)
    a = Z.v_loss(flat(pred), flat(x0), flat(noise), t.numpy(), ac, w, np.float32)
    b = Z.v_loss(flat(pred), flat(x0), flat(noise), t.numpy(), ac, w, np.float64)
    assert a[0].dtype == np.float32 and abs(float(a[0]) - float(b[0])) < 1e-6 * float(b[0])
    assert float(np.abs(a[1] - b[1]).max()) < 1e-6 * float(np.abs(b[1]).max())
    assert set(t.tolist()) >= {0, 999}
    return True
