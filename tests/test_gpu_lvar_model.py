"""Learned variances through the models, the samplers, the trainer and calc_bpd: a UNet with 2C output channels against
the oracle UNet, p_losses with variance_type='learned_range' against the float64 restatement (tests/lvar_reference.py),
DDPM sampling with the learned sigma (graph replay, teacher-forced
steps, CFG, inpainting), DDIM ignoring v, calc_bpd(variance='learned'), and DiT / DiM with learn_sigma.
"""
import math

import pytest
import torch

import lvar_reference as R
import vlb_reference as VR
from test_gpu_elem_kernels import F32, F64, dev, rng
from test_gpu_model import rel
from test_gpu_vlb import LOSS_RTOL, NoiseOracle, Recorder
from test_gpu_vlb import rel as rel_rows
from test_oracle import DIT, TINY, perturb_dit

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 3
CFG6 = {**TINY["unet_tiny_uncond"], "out_channels": 2 * C}
CFG6_COND = {**TINY["unet_tiny_cond"], "out_channels": 2 * C}


def unet6(cond=False, seed=11):
    from diffusion_models_collection_amd.models import UNet
    torch.manual_seed(seed)
    return UNet(**(CFG6_COND if cond else CFG6)).to(DEV).eval()


def _graphs(smp):
    return [e[1] for e in smp.__dict__.get("_step_graphs", {}).values()]


def test_unet_six_channels_matches_oracle():
    """out_channels = 2 * in_channels needs no new argument: forward within 2e-5, every gradient within 2e-4 of its
    absmax against the oracle UNet (the tiny-model bounds of tests/test_gpu_model.py)."""
    from oracle.unet_oracle import make_oracle
    m = unet6()
    m.train()
    orc, sd = make_oracle(m.state_dict(), CFG6, requires_grad=True)
    g = rng(3)
    x = torch.randn(4, C, 16, 16, generator=g)
    t = torch.tensor([0, 60, 400, 999])
    cot = torch.randn(4, 2 * C, 16, 16, generator=g)
    xr = x.clone().requires_grad_(True)
    ref = orc.forward(xr, t)
    (ref * cot).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = m(xd, t.to(DEV))
    assert out.shape == (4, 2 * C, 16, 16)
    assert rel(out, ref) < 2e-5, rel(out, ref)
    (out * cot.to(DEV)).sum().backward()
    assert rel(xd.grad, xr.grad) < 2e-4, rel(xd.grad, xr.grad)
    for k, p in m.named_parameters():
        assert rel(p.grad, sd[k].grad) < 2e-4, (k, rel(p.grad, sd[k].grad))


# ------------------------------------------------------------------------------------------------------------
# p_losses
# ------------------------------------------------------------------------------------------------------------
def _loss_inputs():
    g = rng(21)
    x0 = VR.grid_images((4, C, 16, 16), g)
    noise = torch.randn(4, C, 16, 16, generator=g)
    return x0, noise, torch.tensor([0, 60, 400, 999])


@pytest.mark.parametrize("ptype", ["eps", "v"])
def test_p_losses_learned_range(ptype):
    """The loss is the float64 restatement applied to the recorded model output (1e-5 relative); return_parts sums to the
    total; the gradient reaching the model output is dmc_hybrid_objective's."""
    from diffusion_models_collection_amd import kernels as K
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM
    m = unet6()
    x0, noise, t = _loss_inputs()
    smp = DDPM(device=DEV, prediction_type=ptype, variance_type="learned_range")
    seen = {}

    def model(x, tt, y=None):
        o = m(x, tt, y)
        o.retain_grad()
        seen["out"] = o
        return o

    total, simple, vlb = smp.p_losses(model, dev(x0), dev(t), noise=dev(noise), snr_gamma=5, return_parts=True)
    total.backward()
    out = seen["out"]
    B, per = 4, C * 256
    o3 = out.detach().float().cpu().reshape(B, 2, per)
    ac = smp.alphas_cumprod.cpu()
    tabs = (smp.sqrt_alphas_cumprod.cpu(), smp.sqrt_one_minus_alphas_cumprod.cpu())
    w = smp._snr_weights(5, torch.device(DEV)).cpu()
    r64, _, _ = R.hybrid(F64, ac, ptype, t, o3, x0.flatten(1), noise.flatten(1), "l2", w, 0.001, 1.0, tabs)
    got = torch.stack([total, simple, vlb]).detach()
    e = rel_rows(got, r64)
    print(f"p_losses learned_range {ptype}: {got.tolist()} rel err {e.tolist()}")
    assert bool((e <= LOSS_RTOL).all())
    assert float(vlb) > 0 and abs(float(simple) + float(vlb) - float(total)) <= 2e-7 * abs(float(total))
    assert not simple.requires_grad and not vlb.requires_grad
    one = torch.ones((), dtype=F32, device=DEV)
    _, dout = K.hybrid_objective(ptype, "l2", out.detach().contiguous(), dev(x0), dev(noise), dev(t), dev(tabs[0]),
                                 dev(tabs[1]), smp._lvar_table(torch.device(DEV)), w=dev(w), vlb_weight=0.001, dloss=one)
    assert torch.equal(out.grad, dout) and bool((dout[:, C:] != 0).any())
    # the plain return is the total; DDIM shares the path; vlb_weight changes it
    again = smp.p_losses(m, dev(x0), dev(t), noise=dev(noise), snr_gamma=5)
    assert torch.equal(again.detach(), total.detach())
    ddim = DDIM(device=DEV, prediction_type=ptype, variance_type="learned_range")
    assert torch.equal(ddim.p_losses(m, dev(x0), dev(t), noise=dev(noise), snr_gamma=5).detach(), total.detach())
    heavy = smp.p_losses(m, dev(x0), dev(t), noise=dev(noise), snr_gamma=5, vlb_weight=1.0, return_parts=True)
    assert torch.equal(heavy[1], simple) and float(heavy[2]) > 100 * float(vlb)
    # a model without the variance head is refused
    from diffusion_models_collection_amd.models import UNet
    torch.manual_seed(1)
    plain = UNet(**TINY["unet_tiny_uncond"]).to(DEV).eval()
    with pytest.raises(ValueError, match="6 channels"):
        smp.p_losses(plain, dev(x0), dev(t), noise=dev(noise))
    with pytest.raises(ValueError):
        DDPM(device=DEV).p_losses(plain, dev(x0), dev(t), noise=dev(noise), vlb_weight=0.001)


# ------------------------------------------------------------------------------------------------------------
# sampling
# ------------------------------------------------------------------------------------------------------------
T8, SHAPE = 8, (3, C, 16, 16)


def _sample_inputs():
    g = rng(41)
    return torch.randn(SHAPE, generator=g), torch.randn((T8,) + SHAPE, generator=g)


@pytest.mark.parametrize("ptype", ["eps", "v"])
def test_ddpm_sample_learned_sigma(ptype, monkeypatch):
    """sample() with injected x_T and noise: the graph replay equals the eager loop bit for bit, and each recorded step
    is dmc_ddpm_step_learned on the recorded output (teacher-forced), within criterion 2 of the float64 restatement."""
    from diffusion_models_collection_amd import kernels as K
    from diffusion_models_collection_amd.diffusion import DDPM
    from test_gpu_elem_kernels import DDPM_TABS, judge
    m = unet6()
    xT, noise = _sample_inputs()
    smp = DDPM(num_timesteps=T8, device=DEV, prediction_type=ptype, variance_type="learned_range")
    monkeypatch.setenv("DMC_GRAPH", "0")
    eager = smp.sample(m, SHAPE, x_T=dev(xT), noise=dev(noise))
    monkeypatch.setenv("DMC_GRAPH", "1")
    graphed = smp.sample(m, SHAPE, x_T=dev(xT), noise=dev(noise))
    assert bool(eager.isfinite().all()) and torch.equal(eager, graphed)
    rec = Recorder(m)
    monkeypatch.setenv("DMC_GRAPH", "0")
    allx = smp.sample(rec, SHAPE, x_T=dev(xT), noise=dev(noise), return_all_timesteps=True)
    assert torch.equal(allx[-1], eager.cpu()) and len(rec.seen) == T8
    tabs = tuple(getattr(smp, k) for k in DDPM_TABS[:4])
    coef = smp._lvar_table(torch.device(DEV))
    ac = smp.alphas_cumprod.cpu()
    sa, s1 = smp.sqrt_alphas_cumprod.cpu().double(), smp.sqrt_one_minus_alphas_cumprod.cpu().double()
    for i, (x, t, out) in enumerate(rec.seen):
        assert t.tolist() == [T8 - 1 - i] * SHAPE[0]
        z = noise[i]
        kw = {}
        if ptype == "v":
            eps, x0p = K.pred_convert("v", dev(x), dev(t), smp.sqrt_alphas_cumprod, smp.sqrt_one_minus_alphas_cumprod,
                                      dev(out[:, :C].contiguous()))
            kw = dict(eps=eps, x0=x0p)
        step = K.ddpm_step_learned(dev(x), dev(out), dev(t), *tabs, coef, clip=True, z=dev(z), **kw)
        assert torch.equal(step.cpu(), allx[i]), i
        if ptype == "eps":
            args = (ac, tuple(tb.cpu() for tb in tabs), t, x.flatten(1), out[:, :C].flatten(1), out[:, C:].flatten(1),
                    z.flatten(1), True)
            judge(f"sample step t={int(t[0])}", allx[i].flatten(1), R.ddpm_step(F32, *args), R.ddpm_step(F64, *args),
                  rows=SHAPE[0], quiet=True)
    # the learned sigma took part: a fixed sampler on the prediction half alone gives another image
    fixed = DDPM(num_timesteps=T8, device=DEV, prediction_type=ptype)
    other = fixed.sample(lambda x, t, y=None: m(x, t, y)[:, :C].contiguous(), SHAPE, x_T=dev(xT), noise=dev(noise))
    assert not torch.equal(other, eager)
    mean, var, logvar = smp.p_mean_variance(m, dev(xT), torch.full((SHAPE[0],), 5, device=DEV))
    assert mean.shape == var.shape == logvar.shape == SHAPE and torch.equal(var, logvar.exp())
    tab = coef.cpu()
    assert bool((logvar.cpu() >= tab[5, 3] - 0.25 * tab[5, 4] - 1e-5).all())      # |v| of a fresh network is far below 1.5
    with pytest.raises(ValueError, match="model_out"):
        smp.p_sample(m, dev(xT), torch.full((SHAPE[0],), 5, device=DEV), eps=dev(xT))


class HalvesDiffer:
    """A conditional model whose v half is a constant that depends on whether the row is conditional (label != 0)."""

    def __init__(self, model, v_cond, v_uncond):
        self.model, self.v_cond, self.v_uncond = model, v_cond, v_uncond

    def __call__(self, x, t, y=None):
        out = self.model(x, t, y).clone()
        cond = (y != 0).view(-1, 1, 1, 1)
        out[:, C:] = torch.where(cond, torch.full_like(out[:, C:], self.v_cond), torch.full_like(out[:, C:], self.v_uncond))
        return out


def test_sample_with_cfg_takes_the_conditional_variance(monkeypatch):
    """The guided eps comes from both prediction halves, the variance from the conditional rows: changing the
    unconditional rows' v changes nothing, changing the conditional rows' v does; the graph replay equals the eager loop."""
    from diffusion_models_collection_amd.diffusion import DDPM
    m = unet6(cond=True)
    xT, noise = _sample_inputs()
    y = torch.tensor([1, 2, 3], device=DEV)
    smp = DDPM(num_timesteps=T8, device=DEV, variance_type="learned_range")
    monkeypatch.setenv("DMC_GRAPH", "0")

    def run(model):
        return smp.sample_with_cfg(model, SHAPE, y, cfg_scale=2.0, x_T=dev(xT), noise=dev(noise))

    a = run(HalvesDiffer(m, 0.5, -0.5))
    b = run(HalvesDiffer(m, 0.5, 0.9))
    c = run(HalvesDiffer(m, -0.5, -0.5))
    assert bool(a.isfinite().all()) and torch.equal(a, b) and not torch.equal(a, c)
    eager = run(m)
    monkeypatch.setenv("DMC_GRAPH", "1")
    assert torch.equal(run(m), eager)


def test_inpaint_keeps_the_known_region(monkeypatch):
    """inpaint inherits the learned step: it runs, keeps the known region (the existing check's bound: exactly, after the
    final blend) and the graph replay equals the eager loop."""
    from diffusion_models_collection_amd.diffusion import DDPM
    m = unet6()
    g = rng(43)
    image = VR.grid_images(SHAPE, g)
    mask = torch.zeros(SHAPE[0], 1, 16, 16)
    mask[:, :, :, :8] = 1.0
    smp = DDPM(num_timesteps=T8, device=DEV, variance_type="learned_range")
    monkeypatch.setenv("DMC_GRAPH", "0")
    torch.manual_seed(9)
    out = smp.inpaint(m, dev(image), dev(mask))
    assert out.shape == SHAPE and bool(out.isfinite().all())
    keep = mask.expand(SHAPE).bool()
    assert torch.equal(out.cpu()[keep], image[keep])
    assert not torch.equal(out.cpu()[~keep], image[~keep])


def test_ddim_and_dpm_ignore_v(monkeypatch):
    """DDIM.sample / DPMSolver.sample on the 2C model equal, bit for bit, the same sampler (fixed) on a wrapper that
    returns only the prediction half."""
    from diffusion_models_collection_amd.diffusion import DDIM, DPMSolver
    m = unet6()
    xT, _ = _sample_inputs()
    half = lambda x, t, y=None: m(x, t, y)[:, :C].contiguous()   # noqa: E731
    for graph in ("0", "1"):
        monkeypatch.setenv("DMC_GRAPH", graph)
        for make in (lambda **kw: DDIM(1000, 6, device=DEV, **kw), lambda **kw: DPMSolver(1000, 6, device=DEV, **kw)):
            got = make(variance_type="learned_range").sample(m, SHAPE, x_T=dev(xT))
            ref = make().sample(half, SHAPE, x_T=dev(xT))
            assert bool(got.isfinite().all()) and torch.equal(got, ref)
    with pytest.raises(ValueError, match="6 channels"):
        DDIM(1000, 6, device=DEV, variance_type="learned_range").sample(half, SHAPE, x_T=dev(xT))


# ------------------------------------------------------------------------------------------------------------
# calc_bpd
# ------------------------------------------------------------------------------------------------------------
class OracleWithV(NoiseOracle):
    """NoiseOracle with a variance head that is -1 everywhere: the posterior variance."""

    def __call__(self, x, t, y=None):
        e = super().__call__(x, t, y)
        return torch.cat([e, torch.full_like(e, -1.0)], 1)


def test_calc_bpd_learned_oracle_model():
    """v = -1 everywhere reproduces test_calc_bpd_oracle_model's fixed_small figures: KL columns 0 within 1e-6, a real
    decoder NLL, eps_mse 0; and on the same sampler the two fixed variances use the prediction half."""
    from diffusion_models_collection_amd.diffusion import DDPM
    shape = (3, C, 8, 8)
    g = rng(21)
    x0 = VR.grid_images(shape, g)
    noise = dev(torch.randn((T8,) + shape, generator=g))
    smp = DDPM(num_timesteps=T8, device=DEV, variance_type="learned_range")
    out = smp.calc_bpd(OracleWithV(noise), dev(x0), variance="learned", noise=noise)
    small = DDPM(num_timesteps=T8, device=DEV).calc_bpd(NoiseOracle(noise), dev(x0), variance="fixed_small", noise=noise)
    kl = (out["timesteps"] > 0)
    print(f"learned oracle: vb max over KL columns {out['vb'][:, kl].abs().max():.2e}, decoder {out['vb'][:, ~kl].flatten().tolist()}")
    assert float(out["vb"][:, kl].abs().max()) <= 1e-6 and bool((out["vb"][:, ~kl] > 0).all())
    assert float(out["eps_mse"].max()) < 1e-10
    for k in ("vb", "xstart_mse", "eps_mse", "prior_bpd", "total_bpd"):
        e = (out[k].double() - small[k].double()).abs().max() / small[k].double().abs().max().clamp_min(1e-30)
        assert float(e) <= LOSS_RTOL or float((out[k] - small[k]).abs().max()) <= 1e-6, (k, float(e))
    for variance in ("fixed_small", "fixed_large"):
        got = smp.calc_bpd(OracleWithV(noise), dev(x0), variance=variance, noise=noise)
        ref = DDPM(num_timesteps=T8, device=DEV).calc_bpd(NoiseOracle(noise), dev(x0), variance=variance, noise=noise)
        for k in ("vb", "xstart_mse", "eps_mse", "total_bpd"):
            assert torch.equal(got[k], ref[k]), (variance, k)
    with pytest.raises(ValueError, match="learned_range"):
        DDPM(num_timesteps=T8, device=DEV).calc_bpd(NoiseOracle(noise), dev(x0), variance="learned", noise=noise)


@pytest.mark.parametrize("ptype", ["eps", "v"])
def test_calc_bpd_learned_teacher_forced_parity(ptype, monkeypatch):
    """Every step's (x_t, model output) through the float64 restatement; the graph replay equals the eager loop; DDIM
    gives DDPM's bits."""
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM
    m = unet6()
    g = rng(33)
    x0 = VR.grid_images(SHAPE, g)
    noise = torch.randn((T8,) + SHAPE, generator=g)
    smp = DDPM(num_timesteps=T8, device=DEV, prediction_type=ptype, variance_type="learned_range")
    rec = Recorder(m)
    kw = dict(variance="learned", noise=dev(noise))
    out = smp.calc_bpd(rec, dev(x0), **kw)
    assert len(rec.seen) == T8
    ac = smp.alphas_cumprod.cpu()
    total64 = VR.prior_bpd(ac, x0)
    for i, (x_t, t, o) in enumerate(rec.seen):
        assert t.tolist() == [T8 - 1 - i] * SHAPE[0]
        ins = (x0.flatten(1), x_t.flatten(1), o[:, :C].flatten(1), o[:, C:].flatten(1))
        r64, _ = R.vlb_step(F64, ac, ptype, t, *ins, True)
        r32, _ = R.vlb_step(F32, ac, ptype, t, *ins, True)
        e_vb, e_xs, e_eps = (rel_rows(out[k][:, i], r) for k, r in zip(("vb", "xstart_mse", "eps_mse"), r64))
        own = rel_rows(r32[1], r64[1])
        print(f"{ptype} t={int(t[0]):2d}: rel err vb {e_vb.max():.2e} eps_mse {e_eps.max():.2e} xstart_mse "
              f"{e_xs.max():.2e} (fp32 restatement {own.max():.2e})")
        assert bool((e_vb <= LOSS_RTOL).all()) and bool((e_eps <= LOSS_RTOL).all()), (i, e_vb, e_eps)
        assert bool((e_xs <= torch.clamp(4 * own, min=LOSS_RTOL)).all()), (i, e_xs, own)
        total64 = total64 + r64[0]
    e_tot = rel_rows(out["total_bpd"], total64)
    print(f"{ptype}: total_bpd {out['total_bpd'].tolist()}, rel err {e_tot.max():.2e}")
    assert bool((e_tot <= LOSS_RTOL).all())
    monkeypatch.setenv("DMC_GRAPH", "0")
    eager = smp.calc_bpd(m, dev(x0), **kw)
    assert not _graphs(smp)
    monkeypatch.setenv("DMC_GRAPH", "1")
    graphed = smp.calc_bpd(m, dev(x0), **kw)
    assert len(_graphs(smp)) == 1
    other = DDIM(num_timesteps=T8, num_inference_steps=4, device=DEV, prediction_type=ptype,
                 variance_type="learned_range").calc_bpd(m, dev(x0), **kw)
    for k in ("vb", "xstart_mse", "eps_mse", "prior_bpd", "total_bpd"):
        assert torch.equal(eager[k], out[k]) and torch.equal(graphed[k], out[k]) and torch.equal(other[k], out[k]), k
    # the three variances on one model
    small = smp.calc_bpd(m, dev(x0), variance="fixed_small", noise=dev(noise))
    assert not torch.equal(small["vb"], out["vb"]) and torch.equal(small["xstart_mse"], out["xstart_mse"])
    smp.set_variance_type("fixed")
    assert not _graphs(smp)


def test_evaluate_bpd_learned(tmp_path):
    """A two-batch loader: the image-weighted mean of the two calc_bpd(variance='learned') calls."""
    from diffusion_models_collection_amd.diffusion import DDPM
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer
    torch.manual_seed(3)
    m = UNet(**CFG6).to(DEV)
    smp = DDPM(num_timesteps=T8, device=DEV, variance_type="learned_range")
    cfg = {"epochs": 1, "save_dir": str(tmp_path / "ckpt"), "sample_dir": str(tmp_path / "smp"), "conditional": False,
           "num_classes": None, "model_type": "unet", "model_params": dict(CFG6)}
    tr = DiffusionTrainer(m, smp, None, torch.optim.AdamW(m.parameters(), lr=1e-3), None, device=DEV, config=cfg)
    g = rng(33)
    x0 = VR.grid_images((4, C, 16, 16), g)
    nd = dev(torch.randn((T8, 4, C, 16, 16), generator=g))
    loader = [x0[:3], x0[3:]]
    calls = {"i": 0}

    def per_t(t):
        lo, n = (0, 3) if calls["i"] < T8 else (3, 1)
        calls["i"] += 1
        return nd[t][lo:lo + n]

    got = tr.evaluate_bpd(loader, use_ema=False, variance="learned", noise=per_t)
    m.eval()
    a = smp.calc_bpd(m, dev(x0[:3]), variance="learned", noise=nd[:, :3].contiguous())
    b = smp.calc_bpd(m, dev(x0[3:]), variance="learned", noise=nd[:, 3:].contiguous())
    tot = torch.cat([a["total_bpd"], b["total_bpd"]]).double().mean().item()
    assert got["num_images"] == 4 and got["vb"].shape == (T8,)
    assert math.isclose(got["total_bpd"], tot, rel_tol=1e-12)


# ------------------------------------------------------------------------------------------------------------
# DiT / DiM with a variance head
# ------------------------------------------------------------------------------------------------------------
def _split_models(make, cfg):
    """(model with learn_sigma, plain model carrying the prediction rows, plain model carrying the v rows) of the final
    projection, whose rows go in (p, p, C_out) order."""
    big = make(cfg, True)
    p, Cin = cfg["patch_size"], cfg["in_channels"]
    sd = {k: v.detach().clone() for k, v in big.state_dict().items()}
    rows = torch.arange(p * p * 2 * Cin).view(p * p, 2 * Cin)
    halves = []
    for sel in (rows[:, :Cin].reshape(-1), rows[:, Cin:].reshape(-1)):
        small = make(cfg, False)
        part = dict(sd)
        part["final_layer.linear.weight"] = sd["final_layer.linear.weight"][sel].clone()
        part["final_layer.linear.bias"] = sd["final_layer.linear.bias"][sel].clone()
        small.load_state_dict(part)
        halves.append(small.to(DEV).train())
    return big.to(DEV).train(), halves[0], halves[1]


def _make_dit(cfg, learn_sigma):
    from diffusion_models_collection_amd.models import DiT
    torch.manual_seed(7)
    return perturb_dit(DiT(**cfg, learn_sigma=learn_sigma), 0.05)


def _make_dim(cfg, learn_sigma):
    from dim_reference import perturb
    from diffusion_models_collection_amd.models import DiM
    torch.manual_seed(7)
    return perturb(DiM(**cfg, learn_sigma=learn_sigma), 0.05)


@pytest.mark.parametrize("backbone", ["dit", "dim"])
def test_learn_sigma_is_two_plain_models(backbone):
    """The first C output channels equal a plain model carrying the matching rows of the final projection, the last C the
    other rows (forward within 2e-5, the tiny-model parity bound), and for dout = [g1, g2] every trunk gradient is the
    sum of the two plain models' gradients (2e-4 of its absmax); learn_sigma=False keeps today's state_dict."""
    if backbone == "dit":
        cfg, make = dict(DIT["dit_tiny_cond"]), _make_dit
    else:
        from test_gpu_dim import MAMBA
        cfg, make = dict(MAMBA["sq16"][0]), _make_dim
    big, ma, mb = _split_models(make, cfg)
    Cin = cfg["in_channels"]
    assert big.out_channels == 2 * Cin and ma.out_channels == Cin
    assert list(big.state_dict()) == list(ma.state_dict())
    g = rng(5)
    B = 3
    x = torch.randn(B, Cin, *cfg["img_size"], generator=g).to(DEV)
    t = torch.tensor([17, 903, 0], device=DEV)
    y = torch.tensor([0, 10, 3], device=DEV)
    g1, g2 = (torch.randn(B, Cin, *cfg["img_size"], generator=g).to(DEV) for _ in range(2))
    out = big(x, t, y)
    oa, ob = ma(x, t, y), mb(x, t, y)
    assert out.shape == (B, 2 * Cin) + tuple(cfg["img_size"])
    assert rel(out[:, :Cin], oa) < 2e-5 and rel(out[:, Cin:], ob) < 2e-5, (rel(out[:, :Cin], oa), rel(out[:, Cin:], ob))
    (out * torch.cat([g1, g2], 1)).sum().backward()
    (oa * g1).sum().backward()
    (ob * g2).sum().backward()
    pa, pb = dict(ma.named_parameters()), dict(mb.named_parameters())
    for k, p in big.named_parameters():
        if k.startswith("final_layer.linear."):
            continue
        ref = pa[k].grad + pb[k].grad
        assert rel(p.grad, ref) < 2e-4, (k, rel(p.grad, ref))
