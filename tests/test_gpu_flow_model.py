"""Rectified flow through the models, the step graphs and the trainer: graph replay against the eager loop on the tiny
UNets and the tiny DiT, p_losses + backward against the oracle UNet under autograd with the flow objective written in
torch on the host, the logit-normal sampler on the device, and DiffusionTrainer with a RectifiedFlow.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_reference as R
from test_gpu_elem_kernels import DEV, dev, rng
from test_gpu_model import build, rel
from test_oracle import TINY, split_params

pytestmark = pytest.mark.gpu
SHAPE = (2, 3, 16, 16)


def _D():
    from diffusion_models_collection_amd import diffusion as D
    return D


def _flow(steps=4, solver="euler", **kw):
    return _D().RectifiedFlow(1000, steps, solver=solver, device=DEV, **kw)


def _unet(name):
    from diffusion_models_collection_amd.models import UNet
    torch.manual_seed(11)
    return UNet(**TINY[name]).to(DEV).eval()


def _dit():
    import test_gpu_dit
    m, _ = test_gpu_dit.build("dit_tiny_cond")
    return m.eval()


def _graphs(smp):
    return [e[1] for e in smp.__dict__.get("_step_graphs", {}).values()]


def _three_ways(monkeypatch, smp, call):
    """call(k) -> the k-th of two sampling calls (different x_T / labels). Eager, first capture, cached replay: the same
    bits; one graph kept."""
    def run(graph):
        monkeypatch.setenv("DMC_GRAPH", graph)
        return [call(0), call(1)]

    eager = run("0")
    assert not _graphs(smp)
    graphed = run("1")
    kept = _graphs(smp)
    assert len(kept) == 1                                   # captured by the first call, replayed by the second
    again = run("1")
    assert _graphs(smp) == kept
    for a, b, c in zip(eager, graphed, again):
        assert bool(a.isfinite().all()) and torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(eager[0], eager[1])              # another x_T: another output
    return eager


# ------------------------------------------------------------------------------------------------------------
# graph replay against the eager loop
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_graph_equals_eager_unconditional(solver, monkeypatch):
    """Tiny unconditional UNet, 4 intervals (Heun: 7 rows, so the replayed step serves predictor, corrector and Euler
    rows and carries the history), and the eager loop == the model + kernels.flow_step composed by hand."""
    L, K = _kernels()
    m = _unet("unet_tiny_uncond")
    smp = _flow(4, solver)
    xs = [torch.randn(SHAPE, device=DEV) for _ in range(2)]
    eager = _three_ways(monkeypatch, smp, lambda k: smp.sample(m, SHAPE, x_T=xs[k]))
    monkeypatch.setenv("DMC_GRAPH", "0")
    x, xb, d = xs[0].clone(), torch.zeros_like(xs[0]), torch.zeros_like(xs[0])
    with torch.no_grad():
        for r, t in enumerate(smp.step_timesteps.tolist()):
            tt = torch.full((SHAPE[0],), t, dtype=torch.long, device=DEV)
            k = torch.full((SHAPE[0],), r, dtype=torch.long, device=DEV)
            v = m(x, tt[:1] if getattr(m, "shared_timestep", False) else tt, None).contiguous()    # as the sampler calls it
            x = K.flow_step(x, v, k, smp.step_coefficients, xb=xb, dprev=d, xb_out=xb, d_out=d)
    assert torch.equal(x, eager[0])


def _kernels():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_graph_equals_eager_conditional_sample(solver, monkeypatch):
    """sample(y=...) on the tiny conditional UNet: the labels are a constant graph input, replaced on the second call."""
    m = _unet("unet_tiny_cond")
    smp = _flow(3, solver)
    xs = [torch.randn(SHAPE, device=DEV) for _ in range(2)]
    ys = [torch.tensor([1, 2], device=DEV), torch.tensor([7, 5], device=DEV)]
    eager = _three_ways(monkeypatch, smp, lambda k: smp.sample(m, SHAPE, y=ys[k], x_T=xs[k]))
    monkeypatch.setenv("DMC_GRAPH", "0")
    assert not torch.equal(smp.sample(m, SHAPE, y=ys[1], x_T=xs[0]), eager[0])      # the label drives the result


@pytest.mark.parametrize("path", ["fused", "guide"])
@pytest.mark.parametrize("solver", ["euler", "heun"])
@pytest.mark.parametrize("backbone", ["unet", "dit"])
def test_graph_equals_eager_cfg(backbone, solver, path, monkeypatch):
    """sample_with_cfg: the fused-guidance path (one dmc_flow_step beside the 2B forward) and the guide path
    (p_threshold = 0.995, guidance_rescale = 0.7: dmc_flow_guide, then dmc_flow_step); eager == graphed == kept graph,
    and the eager loop == the batched forward + the kernels composed by hand."""
    L, K = _kernels()
    m = _unet("unet_tiny_cond") if backbone == "unet" else _dit()
    smp = _flow(3, solver)
    kw = {} if path == "fused" else dict(p_threshold=0.995, guidance_rescale=0.7)
    xs = [torch.randn(SHAPE, device=DEV) for _ in range(2)]
    ys = [torch.tensor([1, 2], device=DEV), torch.tensor([7, 5], device=DEV)]
    eager = _three_ways(monkeypatch, smp, lambda k: smp.sample_with_cfg(m, SHAPE, ys[k], x_T=xs[k], **kw))

    monkeypatch.setenv("DMC_GRAPH", "0")
    B = SHAPE[0]
    coef = smp.step_coefficients
    x, xb, d = xs[0].clone(), torch.zeros_like(xs[0]), torch.zeros_like(xs[0])
    with torch.no_grad():
        for r, t in enumerate(smp.step_timesteps.tolist()):
            tt = torch.full((2 * B,), t, dtype=torch.long, device=DEV)
            k = torch.full((B,), r, dtype=torch.long, device=DEV)
            both = m(torch.cat([x, x], 0), tt, torch.cat([ys[0], torch.zeros_like(ys[0])], 0)).contiguous()
            if path == "fused":
                x = K.flow_step(x, both[:B], k, coef, pu=both[B:], scale=3.0, xb=xb, dprev=d, xb_out=xb, d_out=d)
            else:
                g = K.flow_guide(x, both[:B], both[B:], 3.0, 0.7, k, coef, threshold=True, p_threshold=0.995)
                x = K.flow_step(x, g, k, coef, xb=xb, dprev=d, xb_out=xb, d_out=d)
    assert torch.equal(x, eager[0])
    other = smp.sample_with_cfg(m, SHAPE, ys[0], x_T=xs[0], **({} if path == "guide" else dict(guidance_rescale=0.7)))
    assert not torch.equal(other, eager[0])                 # the other path is another computation


@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_return_all_timesteps(solver):
    m = _unet("unet_tiny_uncond")
    smp = _flow(4, solver)
    xT = torch.randn(SHAPE, device=DEV)
    plain = smp.sample(m, SHAPE, x_T=xT)
    every = smp.sample(m, SHAPE, x_T=xT, return_all_timesteps=True)
    assert every.shape == (4,) + SHAPE                      # one image per interval
    assert torch.equal(every[-1], plain.cpu())
    assert not torch.equal(every[0], every[-1])
    assert not _graphs(smp) or len(_graphs(smp)) == 1       # the recording call keeps no graph of its own


def test_two_channel_model_is_refused():
    """A learn_sigma-style model (2C output channels) has no use in a flow: ValueError, from sampling and training."""
    m = _unet("unet_tiny_uncond")
    smp = _flow(2)

    def wide(x, t, y=None):
        v = m(x, t, y)
        return torch.cat([v, v], 1)

    x = torch.randn(SHAPE, device=DEV)
    with pytest.raises(ValueError, match="2C-channel"):
        smp.sample(wide, SHAPE, x_T=x)
    with pytest.raises(ValueError, match="2C-channel"):
        smp.p_losses(wide, x, torch.tensor([3, 900], device=DEV))


# ------------------------------------------------------------------------------------------------------------
# training
# ------------------------------------------------------------------------------------------------------------
def host_loss(kind, pred, target):
    if kind == "l1":
        return F.l1_loss(pred, target)
    if kind == "l2":
        return F.mse_loss(pred, target)
    return F.smooth_l1_loss(pred, target)


@pytest.mark.parametrize("kind", ["l1", "l2", "huber"])
def test_p_losses_matches_oracle(kind):
    """fp32, B = 4, dropout 0, shift 3: the loss within 1e-5 relative and every parameter gradient within 2e-4 of its
    absmax (the bounds of test_p_losses_v_min_snr_matches_oracle), against the oracle UNet under autograd with
    x_t = (1 - sigma) x0 + sigma eps and the target eps - x0 written in torch on the host. Levels include 0 and T-1."""
    from oracle.unet_oracle import make_oracle
    name = "unet_tiny_cond"
    m, g = build(name)
    m.train()
    orc, sd = make_oracle(split_params(g, "param/"), TINY[name], requires_grad=True)
    gen = torch.Generator().manual_seed(21)
    B = 4
    x0 = torch.rand(B, 3, 16, 16, generator=gen) * 2 - 1
    noise = torch.randn(B, 3, 16, 16, generator=gen)
    t = torch.tensor([0, 60, 400, 999])
    y = torch.tensor([3, 0, 10, 7])
    sig, om = (torch.from_numpy(v) for v in R.ref_sigmas(1000, 3.0))
    xt = om[t].view(B, 1, 1, 1) * x0 + sig[t].view(B, 1, 1, 1) * noise
    assert torch.equal(xt[3], noise[3])                     # the last level is pure noise
    lref = host_loss(kind, orc.forward(xt, t, y), noise - x0)
    lref.backward()
    smp = _flow(10, shift=3.0)
    assert torch.equal(smp.q_sample(x0.to(DEV), t.to(DEV), noise.to(DEV)).cpu(), xt)
    loss = smp.p_losses(m, x0.to(DEV), t.to(DEV), y.to(DEV), noise=noise.to(DEV), loss_type=kind)
    loss.backward()
    print(f"{kind}: loss {loss.item():.9g}, oracle {lref.item():.9g}")
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    for k, p in m.named_parameters():
        assert rel(p.grad, sd[k].grad) < 2e-4, (k, rel(p.grad, sd[k].grad))
    # the eps-target loss of the same call is another number: the velocity target did take part
    eps_loss = _D().DDPM(device=DEV).p_losses(m, x0.to(DEV), t.to(DEV), y.to(DEV), noise=noise.to(DEV), loss_type=kind)
    assert abs(eps_loss.item() - loss.item()) > 1e-3 * abs(loss.item())


def test_logit_normal_sampler_on_device():
    """The loss under the logit-normal sampler has the bits of the loss without one for the same t (weight_table() is
    None), the gradients too; sample(u=...) is numpy's searchsorted on the same fp32 CDF, bit for bit."""
    D = _D()
    m = _unet("unet_tiny_uncond")
    m.train()
    smp = _flow(10)
    s = D.create_named_schedule_sampler("logit-normal", smp, mean=-0.5, std=0.7)
    assert isinstance(s, D.LogitNormalSampler) and s.weight_table() is None
    u = torch.rand(4096, generator=rng(3))
    u[:4] = torch.tensor([0.0, 0.5, 1.0 - 2.0 ** -24, 2.0 ** -30])
    t, w = s.sample(4096, DEV, u=dev(u))
    assert t.is_cuda and t.dtype == torch.long and w.is_cuda and bool((w == 1).all())
    cdf = s.cdf(DEV).cpu().numpy()
    want = np.minimum(np.searchsorted(cdf, u.numpy(), side="right"), 999)
    assert np.array_equal(t.cpu().numpy(), want)
    t2, _ = s.sample(64, DEV)
    assert t2.shape == (64,) and 0 <= int(t2.min()) and int(t2.max()) <= 999

    g = rng(21)
    x0 = dev(torch.rand(4, 3, 16, 16, generator=g) * 2 - 1)
    noise = dev(torch.randn(4, 3, 16, 16, generator=g))
    tt = t[:4].contiguous()

    def grads(**kw):
        m.zero_grad(set_to_none=True)
        loss = smp.p_losses(m, x0, tt, noise=noise, **kw)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    la, ga = grads()
    lb, gb = grads(schedule_sampler=s)
    assert torch.equal(la, lb) and bool(la.isfinite())
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert any(bool((v != 0).any()) for v in ga.values())


# ------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, diffusion, extra=None):
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer
    torch.manual_seed(0)
    mp = dict(TINY["unet_tiny_uncond"])
    m = UNet(**mp).to(DEV)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    cfg = {"epochs": 1, "save_dir": str(tmp_path / "ckpt"), "sample_dir": str(tmp_path / "smp"), "conditional": False,
           "num_classes": None, "model_type": "unet", "model_params": mp, **(extra or {})}
    tr = DiffusionTrainer(m, diffusion, None, opt, None, device=DEV, config=cfg)
    m.train()
    return tr, m


def test_trainer_trains_a_flow_eagerly(tmp_path, monkeypatch):
    """With a RectifiedFlow the captured step is not used (it has no flow objective), with a DDPM it is, as before. The
    first step's loss under a fixed torch seed has the bits of p_losses called by hand with the same draws; three steps
    give finite losses and move the parameters. evaluate_bpd surfaces the flow's NotImplementedError."""
    from diffusion_models_collection_amd.utils.trainer import GraphedTrainStep
    D = _D()
    monkeypatch.setenv("DMC_GRAPH", "1")
    plain, _ = _trainer(tmp_path, D.DDPM(device=DEV))
    assert GraphedTrainStep.supported(plain) and plain._graph is not None
    tr, m = _trainer(tmp_path, _flow(4))
    assert tr._flat is not None and not GraphedTrainStep.supported(tr) and tr._graph is None
    x = (torch.rand(3, 4, 3, 16, 16, generator=rng(2)) * 2 - 1).to(DEV)

    ref_m = _trainer(tmp_path, _flow(4))[1]
    torch.manual_seed(123)
    t = torch.randint(0, 1000, (4,), device=DEV).long()
    want = tr.diffusion.p_losses(ref_m, x[0], t, None, loss_type="l2").detach()

    w0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    torch.manual_seed(123)
    losses = [tr.train_step(x[i], i) for i in range(3)]
    assert torch.equal(losses[0], want)
    assert all(v.shape == () and bool(torch.isfinite(v)) for v in losses)
    assert any(not torch.equal(w0[k], v.detach()) for k, v in m.named_parameters())
    with pytest.raises(NotImplementedError, match="RectifiedFlow"):
        tr.evaluate_bpd([x[0]], use_ema=False)

    # the trainer's 'schedule_sampler' key reaches the flow's p_losses
    tr2, _ = _trainer(tmp_path, _flow(4), {"schedule_sampler": "logit-normal"})
    assert isinstance(tr2.schedule_sampler, D.LogitNormalSampler) and tr2._graph is None
    assert bool(torch.isfinite(tr2.train_step(x[1], 0)))
