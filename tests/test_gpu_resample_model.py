"""Loss-aware timestep sampling through the public interface: p_losses(schedule_sampler=...) on DDPM / DDIM with the tiny
UNets of tests/test_gpu_lvar_model.py, the samplers' state, and the trainer's 'schedule_sampler' key.
"""
import numpy as np
import pytest
import torch

import resample_reference as R
import vlb_reference as VR
from test_gpu_elem_kernels import F32, dev, rng
from test_gpu_lvar_model import C, unet6
from test_gpu_vlb import LOSS_RTOL
from test_oracle import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 4


def _diffusion():
    from diffusion_models_collection_amd import diffusion as D
    return D


def plain_unet(seed=11):
    from diffusion_models_collection_amd.models import UNet
    torch.manual_seed(seed)
    return UNet(**TINY["unet_tiny_uncond"]).to(DEV).eval()


def _inputs():
    g = rng(21)
    x0 = VR.grid_images((B, C, 16, 16), g)
    noise = torch.randn(B, C, 16, 16, generator=g)
    return dev(x0), dev(noise), dev(torch.tensor([0, 60, 400, 999]))


def recording(m, seen):
    def model(x, tt, y=None):
        seen["out"] = m(x, tt, y)
        return seen["out"]
    return model


def grads_of(m, loss):
    m.zero_grad(set_to_none=True)
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def same_grads(a, b):
    assert a.keys() == b.keys() and a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(bool((v != 0).any()) for v in a.values())


def warm(s, seed=5):
    """K losses at every timestep, their size falling 100x over t (fp32, from a CPU generator)."""
    T, Kh = s.num_timesteps, s.history_per_term
    g = rng(seed)
    t = torch.arange(T, device=DEV)
    scale = torch.logspace(0, -2, T)
    for _ in range(Kh):
        s.update_with_local_losses(t, dev((torch.rand(T, generator=g) + 0.5) * scale))
    return s


def tables_of(smp):
    d = torch.device(DEV, torch.cuda.current_device())
    return smp._tab("sqrt_alphas_cumprod", d), smp._tab("sqrt_one_minus_alphas_cumprod", d), d


# ------------------------------------------------------------------------------------------------------------
# p_losses
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype,kw", [("eps", {}), ("eps", {"snr_gamma": 5, "loss_type": "huber"}), ("v", {})],
                         ids=["default", "eps-gamma-huber", "v"])
def test_fresh_sampler_changes_no_bit(ptype, kw):
    """A sampler that has seen nothing weights by 1: the loss and every parameter gradient are those of the call without
    it. The default eps objective runs dmc_loss_fwd without a sampler, whose reduction order is another: there the loss is
    compared with dmc_objective on the same model output (the gradients with the call without the sampler)."""
    from diffusion_models_collection_amd import kernels as K
    D = _diffusion()
    m = plain_unet()
    x0, noise, t = _inputs()
    smp = D.DDPM(device=DEV, prediction_type=ptype)
    base = smp.p_losses(m, x0, t, noise=noise, **kw)
    g_base = grads_of(m, base)
    s = D.LossSecondMomentResampler(smp)
    seen = {}
    loss = smp.p_losses(recording(m, seen), x0, t, noise=noise, schedule_sampler=s, **kw)
    assert loss.shape == () and loss.dtype == F32
    same_grads(grads_of(m, loss), g_base)
    if smp._default_objective(kw.get("snr_gamma")):
        sa, s1, _ = tables_of(smp)
        ref, _ = K.objective("eps", "l2", seen["out"].detach().contiguous(), x0, noise, t, sa, s1, grad=False)
        assert torch.equal(loss.detach(), ref)
        assert abs(float(loss.detach()) - float(base.detach())) <= LOSS_RTOL * abs(float(base.detach()))
    else:
        assert torch.equal(loss.detach(), base.detach())
    assert int(s.state_dict()["count"].sum()) == B
    # the uniform sampler and DDIM share the path
    u = D.UniformSampler(smp)
    assert torch.equal(smp.p_losses(m, x0, t, noise=noise, schedule_sampler=u, **kw).detach(), loss.detach())
    ddim = D.DDIM(device=DEV, prediction_type=ptype)
    s2 = D.create_named_schedule_sampler("loss-second-moment", ddim)
    assert torch.equal(ddim.p_losses(m, x0, t, noise=noise, schedule_sampler=s2, **kw).detach(), loss.detach())


def test_weighted_loss_feeds_the_history():
    """With a warm history: weights = iw[t]; the loss is dmc_objective_is on the model output with the sampler's table,
    and mean(iw[t] * row_loss) of that kernel's rows; the history takes exactly the batch, as the sequential loop would;
    under no_grad it is untouched."""
    from diffusion_models_collection_amd import kernels as K
    D = _diffusion()
    m = plain_unet()
    x0, noise, _ = _inputs()
    smp = D.DDPM(device=DEV, prediction_type="v")
    s = warm(D.LossSecondMomentResampler(smp))
    t, wts = s.sample(B, DEV, u=dev(torch.tensor([0.0, 0.3, 0.3, 0.999])))
    iw, p = s.weight_table(), s.weights()
    assert t.dtype == torch.long and wts.dtype == F32 and torch.equal(wts, iw[t])
    assert int(t[1]) == int(t[2]) and float(iw.max() / iw.min()) > 10 and abs(float(p.double().sum()) - 1) < 1e-6
    assert int(t[0]) == 0 and int(t[3]) > int(t[1])
    before = {k: v.cpu().numpy() for k, v in s.state_dict().items()}
    seen = {}
    loss = smp.p_losses(recording(m, seen), x0, t, noise=noise, snr_gamma=5, schedule_sampler=s)
    sa, s1, d = tables_of(smp)
    w = smp._snr_weights(5, d)
    out = seen["out"].detach().contiguous()
    ref, row, _ = K.objective_is("v", "l2", out, x0, noise, t, sa, s1, w, iw, grad=False)
    assert torch.equal(loss.detach(), ref)
    mean64 = float((iw[t].double() * row.double()).sum() / B)
    got = float(loss.detach())
    print(f"weighted loss {got:.9g}, mean(iw[t] * row) {mean64:.9g}; unweighted {float(row.double().mean()):.9g}")
    assert abs(got - mean64) <= LOSS_RTOL * abs(mean64)
    assert abs(float(row.double().mean()) - mean64) > 1e-3 * abs(mean64)      # the weights did take part
    # the gradient reaching the model output carries iw as well
    one = torch.ones((), dtype=F32, device=DEV)
    seen["out"].retain_grad()
    loss.backward()
    _, _, dpred = K.objective_is("v", "l2", out, x0, noise, t, sa, s1, w, iw, dloss=one, row_loss=False)
    assert torch.equal(seen["out"].grad, dpred)
    after = {k: v.cpu().numpy() for k, v in s.state_dict().items()}
    R.ring_update(before["history"], before["count"], t.cpu().numpy(), row.cpu().numpy())
    assert np.array_equal(after["count"], before["count"]) and np.array_equal(after["history"], before["history"])
    assert int(after["count"].sum()) == s.num_timesteps * s.history_per_term + B
    with torch.no_grad():
        quiet = smp.p_losses(m, x0, t, noise=noise, snr_gamma=5, schedule_sampler=s)
    assert torch.equal(quiet, loss.detach())
    for k, v in s.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), after[k]), k


def test_sampler_state_round_trip():
    D = _diffusion()
    smp = D.DDPM(device=DEV)
    s = warm(D.LossSecondMomentResampler(smp, history_per_term=3, uniform_prob=0.01))
    sd = s.state_dict()
    assert sd["history"].shape == (1000, 3) and sd["history"].dtype == F32 and sd["count"].dtype == torch.int32
    u = dev(torch.rand(33, generator=rng(1)))
    t, wts = s.sample(33, u=u)
    for state in (sd, {k: v.cpu() for k, v in sd.items()}):
        s2 = D.LossSecondMomentResampler(smp, history_per_term=3, uniform_prob=0.01)
        assert torch.equal(s2.weight_table(), torch.ones(1000, device=DEV))      # fresh: ones
        s2.load_state_dict(state)
        t2, w2 = s2.sample(33, u=u)
        assert torch.equal(t2, t) and torch.equal(w2, wts) and torch.equal(s2.weights(), s.weights())
    s.update_with_local_losses(t, wts)      # the saved state is a copy
    assert not torch.equal(s.state_dict()["count"], sd["count"])
    with pytest.raises(ValueError):
        D.LossSecondMomentResampler(smp, history_per_term=4).load_state_dict(sd)
    # the uniform sampler: uniform draws, weights 1, nothing to save
    us = D.UniformSampler(smp)
    tu, wu = us.sample(5, DEV)
    assert tu.dtype == torch.long and tu.shape == (5,) and torch.equal(wu, torch.ones(5, device=DEV))
    assert us.weight_table() is None and us.state_dict() == {}
    assert us.weights().is_cuda and torch.equal(us.weights(), torch.full((1000,), 1e-3, device=DEV))
    assert torch.equal(us.sample(3, DEV, u=torch.tensor([0.0, 0.5, 0.9999]))[0].cpu(), torch.tensor([0, 500, 999]))


def test_learned_range_with_sampler():
    """The hybrid loss under a warm sampler is dmc_hybrid_objective_is on the model output; return_parts holds
    (total = simple + vlb, only the total differentiable); the history takes the batch."""
    from diffusion_models_collection_amd import kernels as K
    D = _diffusion()
    m = unet6()
    x0, noise, _ = _inputs()
    smp = D.DDPM(device=DEV, variance_type="learned_range")
    s = warm(D.LossSecondMomentResampler(smp))
    t, _ = s.sample(B, DEV, u=dev(torch.tensor([0.0, 0.2, 0.6, 0.9999])))
    iw = s.weight_table()
    seen = {}
    total, simple, vlb = smp.p_losses(recording(m, seen), x0, t, noise=noise, return_parts=True, schedule_sampler=s)
    sa, s1, d = tables_of(smp)
    out = seen["out"].detach().contiguous()
    ref, row, _ = K.hybrid_objective_is("eps", "l2", out, x0, noise, t, sa, s1, smp._lvar_table(d), None, iw,
                                        vlb_weight=0.001, grad=False)
    assert torch.equal(torch.stack([total, simple, vlb]).detach(), ref)
    tot = float(total.detach())
    assert float(vlb) > 0 and abs(float(simple) + float(vlb) - tot) <= 2e-7 * abs(tot)
    assert total.requires_grad and not simple.requires_grad and not vlb.requires_grad
    mean64 = float((iw[t].double() * row.double()).sum() / B)
    assert abs(tot - mean64) <= LOSS_RTOL * abs(mean64)
    g = grads_of(m, total)
    assert all(bool(v.isfinite().all()) for v in g.values()) and any(bool((v != 0).any()) for v in g.values())
    assert int(s.state_dict()["count"].sum()) == s.num_timesteps * s.history_per_term + B
    # a fresh sampler: the bits of the call without one
    base = smp.p_losses(m, x0, t, noise=noise, return_parts=True)
    fresh = smp.p_losses(m, x0, t, noise=noise, return_parts=True,
                         schedule_sampler=D.LossSecondMomentResampler(smp))
    for a, b in zip(base, fresh):
        assert torch.equal(a.detach(), b.detach())
    with pytest.raises(ValueError):
        D.DDPM(device=DEV).p_losses(plain_unet(), x0, t, noise=noise, return_parts=True, schedule_sampler=s)


# ------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, extra):
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer
    D = _diffusion()
    torch.manual_seed(0)
    mp = dict(TINY["unet_tiny_uncond"])
    m = UNet(**mp).to(DEV)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    cfg = {"epochs": 1, "save_dir": str(tmp_path / "ckpt"), "sample_dir": str(tmp_path / "smp"), "conditional": False,
           "num_classes": None, "model_type": "unet", "model_params": mp, **extra}
    tr = DiffusionTrainer(m, D.DDPM(device=DEV), None, opt, None, device=DEV, config=cfg)
    m.train()
    return tr, m


def test_trainer_with_the_resampler_runs_eager(tmp_path, monkeypatch):
    """Two steps on a 4-image loader: the sampler's counts sum to the images seen, the parameters move, and the captured
    step is not used although a trainer without the key would use it."""
    from diffusion_models_collection_amd.utils.trainer import GraphedTrainStep
    D = _diffusion()
    monkeypatch.setenv("DMC_GRAPH", "1")
    plain, _ = _trainer(tmp_path, {})
    assert plain.schedule_sampler is None and GraphedTrainStep.supported(plain) and plain._graph is not None
    tr, m = _trainer(tmp_path, {"schedule_sampler": "loss-second-moment"})
    assert isinstance(tr.schedule_sampler, D.LossSecondMomentResampler)
    assert tr._flat is not None and not GraphedTrainStep.supported(tr) and tr._graph is None
    x = torch.rand(4, 3, 16, 16, generator=rng(2)) * 2 - 1
    loader = [x[:2], x[2:]]
    w0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    seen = 0
    for i, batch in enumerate(loader):
        loss = tr.train_step(batch, i)
        assert loss.shape == () and bool(torch.isfinite(loss))
        seen += batch.shape[0]
        assert int(tr.schedule_sampler.state_dict()["count"].sum()) == seen
    assert seen == 4 and any(not torch.equal(w0[k], v.detach()) for k, v in m.named_parameters())
    with pytest.raises(ValueError):
        _trainer(tmp_path, {"schedule_sampler": "importance"})


@pytest.mark.parametrize("extra", [{}, {"schedule_sampler": None}, {"schedule_sampler": "uniform"}],
                         ids=["absent", "none", "uniform"])
def test_trainer_without_a_sampler_draws_as_before(extra, tmp_path, monkeypatch):
    """For a fixed seed the step's t is torch.randint's under that seed, and p_losses is not handed a sampler."""
    monkeypatch.setenv("DMC_GRAPH", "0")
    tr, m = _trainer(tmp_path, extra)
    assert tr.schedule_sampler is None
    got = {}
    inner = tr.diffusion.p_losses

    def spy(model, images, t, *a, **kw):
        got["t"], got["kw"] = t.clone(), kw
        return inner(model, images, t, *a, **kw)

    monkeypatch.setattr(tr.diffusion, "p_losses", spy)
    x = (torch.rand(4, 3, 16, 16, generator=rng(2)) * 2 - 1).to(DEV)
    torch.manual_seed(123)
    tr.train_step(x, 0)
    torch.manual_seed(123)
    ref = torch.randint(0, tr.diffusion.num_timesteps, (4,), device=DEV).long()
    assert torch.equal(got["t"], ref) and "schedule_sampler" not in got["kw"]
