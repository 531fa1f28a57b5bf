"""The v-prediction / min-SNR objective through the model, the trainer and the sampling graphs, on the tiny conditional
UNet of the reference fixtures: p_losses + backward against the oracle UNet under autograd with
tests/objective_reference.py's loss, the captured training step against the eager one, the defaults against the
pre-existing loss path, and graphed sampling loops with prediction_type='v'.
"""
import pytest
import torch

import objective_reference as R
from test_gpu_model import build, rel
from test_oracle import TINY, split_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = "unet_tiny_cond"


@pytest.mark.parametrize("kind", ["l2", "huber"])
def test_p_losses_v_min_snr_matches_oracle(kind):
    """fp32, B = 4, dropout 0, prediction_type='v', snr_gamma=5: the loss within 1e-5 relative and every parameter
    gradient within 2e-4 of its absmax (the project's tiny-model bounds), against the oracle UNet under autograd with
    the restated loss on the host. Timesteps on both sides of SNR = 5."""
    from diffusion_models_collection_amd.diffusion import DDPM
    from oracle import diffusion_oracle as DO
    from oracle.unet_oracle import make_oracle
    m, g = build(NAME)
    m.train()
    orc, sd = make_oracle(split_params(g, "param/"), TINY[NAME], requires_grad=True)
    gen = torch.Generator().manual_seed(21)
    B = 4
    x0 = torch.rand(B, 3, 16, 16, generator=gen) * 2 - 1
    noise = torch.randn(B, 3, 16, 16, generator=gen)
    t = torch.tensor([0, 60, 400, 999])
    y = torch.tensor([3, 0, 10, 7])
    ddpm = DDPM(device=DEV, prediction_type="v")
    ac = ddpm.alphas_cumprod.cpu()
    sa, s1 = ddpm.sqrt_alphas_cumprod.cpu(), ddpm.sqrt_one_minus_alphas_cumprod.cpu()
    w = torch.from_numpy(R.textbook_weights(ac.numpy(), 5.0, "v")).float()
    snr = ac.double() / (1 - ac.double())
    assert snr[60] > 5 > snr[400]
    pred = orc.forward(DO.q_sample(DO.schedule(), x0, t, noise), t, y)
    lref = R.loss(torch.float32, "v", kind, pred.reshape(B, -1), x0.reshape(B, -1), noise.reshape(B, -1), t, sa, s1, w)
    lref.backward()
    loss = ddpm.p_losses(m, x0.to(DEV), t.to(DEV), y.to(DEV), noise=noise.to(DEV), loss_type=kind, snr_gamma=5)
    loss.backward()
    print(f"{kind}: loss {loss.item():.9g}, oracle {lref.item():.9g}")
    assert abs(loss.item() - lref.item()) <= 1e-5 * abs(lref.item())
    for k, p in m.named_parameters():
        assert rel(p.grad, sd[k].grad) < 2e-4, (k, rel(p.grad, sd[k].grad))
    # the eps-target loss of the same prediction is another number: the v target did take part
    eps_loss = DDPM(device=DEV).p_losses(m, x0.to(DEV), t.to(DEV), y.to(DEV), noise=noise.to(DEV), loss_type=kind)
    assert abs(eps_loss.item() - loss.item()) > 1e-3 * abs(loss.item())


# ------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------
def _train(monkeypatch, graph, extra, diffusion=None, steps=4, hold=False):
    """`steps` trainer steps on the tiny conditional UNet (fp32, FlatAdamW, EMA, label dropout): (losses, parameters,
    EMA parameters, trainer). Per-step inputs come from the same generators in the same order in every run."""
    from diffusion_models_collection_amd.diffusion import DDPM
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer
    monkeypatch.setenv("DMC_GRAPH", "1" if graph else "0")
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    mp = dict(TINY[NAME])
    m = UNet(**mp).to(DEV)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    cfg = {"epochs": 1, "save_dir": "/tmp/dmc_objective_ckpt", "sample_dir": "/tmp/dmc_objective_smp",
           "loss_type": "huber", "use_ema": True, "ema_decay": 0.99, "conditional": True, "num_classes": 10,
           "cfg_dropout_prob": 0.2, "model_type": "unet",
           "model_params": {k: v for k, v in mp.items() if k != "num_classes"}, **extra}
    tr = DiffusionTrainer(m, diffusion if diffusion is not None else DDPM(device=DEV), None, opt, None, device=DEV,
                          config=cfg)
    assert tr._flat is not None and (tr._graph is not None) == graph
    m.train()
    gen = torch.Generator().manual_seed(5)
    losses = []
    for i in range(steps):
        x = (torch.rand(8, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
        lab = torch.randint(0, 10, (8,), generator=gen).to(DEV)
        loss = tr.train_step((x, lab), i)
        losses.append(loss if hold else loss.detach().float().cpu().reshape(()))
    torch.cuda.synchronize()
    if graph:
        assert tr._graph.graph is not None and not tr._graph.failed and tr._graph.replays == steps - tr._graph.WARM
    losses = torch.stack([v.detach().float().cpu().reshape(()) for v in losses])
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ema = {k: v.detach().cpu().clone() for k, v in tr.ema_model.state_dict().items()}
    return losses, sd, ema, tr


def _same_run(a, b):
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert bool(a[0].isfinite().all())
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("extra,hold", [({"prediction_type": "v"}, False), ({"snr_gamma": 5}, False),
                                        ({"prediction_type": "v", "snr_gamma": 5}, False),
                                        ({"prediction_type": "v", "snr_gamma": 5}, True)],
                         ids=["v", "gamma", "v-gamma", "v-gamma-hold"])
def test_graphed_train_step_matches_eager(extra, hold, monkeypatch):
    """Four steps eager against two eager warm-up steps plus two replays of the captured step (one dmc_objective call
    in place of loss_fwd + loss_bwd): losses, parameters and EMA bit for bit; `hold`: the caller keeps every step's
    loss alive through the capture. The objective does change the run."""
    eager = _train(monkeypatch, False, extra, hold=hold)
    graphed = _train(monkeypatch, True, extra, hold=hold)
    _same_run(eager, graphed)
    tr = graphed[3]
    assert tr.diffusion.prediction_type == extra.get("prediction_type", "eps")
    assert tr.snr_gamma == extra.get("snr_gamma")
    if not hold:
        default = _train(monkeypatch, False, {})
        assert not torch.equal(default[0], eager[0])


def test_trainer_defaults_untouched(monkeypatch):
    """No new config key: eager and graphed steps give, bit for bit, what a trainer gives whose diffusion object
    carries the reference's p_losses (reference signature, q_sample -> model -> diffusion_loss)."""
    from diffusion_models_collection_amd.diffusion import DDPM
    from diffusion_models_collection_amd.diffusion.ddpm import diffusion_loss

    class ReferenceSignature(DDPM):
        def p_losses(self, model, x_start, t, y=None, noise=None, loss_type='l2'):
            if noise is None:
                noise = torch.randn_like(x_start)
            return diffusion_loss(model(self.q_sample(x_start, t, noise), t, y), noise, loss_type)

    ref = _train(monkeypatch, False, {}, diffusion=ReferenceSignature(device=DEV))
    _same_run(ref, _train(monkeypatch, False, {}))
    _same_run(ref, _train(monkeypatch, True, {}))


def test_p_losses_defaults_are_loss_fwd():
    from diffusion_models_collection_amd import kernels as K
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM
    m, g = build(NAME)
    m.eval()
    gen = torch.Generator().manual_seed(23)
    x0 = (torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
    noise = torch.randn(4, 3, 16, 16, generator=gen).to(DEV)
    t = torch.tensor([0, 60, 400, 999], device=DEV)
    y = torch.tensor([3, 0, 10, 7], device=DEV)
    for d in (DDPM(device=DEV), DDIM(device=DEV)):
        with torch.no_grad():
            pred = m(d.q_sample(x0, t, noise), t, y)
            got = d.p_losses(m, x0, t, y, noise=noise)
            assert torch.equal(got, K.loss_fwd("l2", pred.contiguous(), noise))


# ------------------------------------------------------------------------------------------------------------
# sampling graphs
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_v_sampling_graph_equals_eager(kind, monkeypatch):
    """DDIM-10 / DPMSolver-10, B = 4, eval mode, prediction_type='v': the replayed step (model, dmc_pred_convert, step
    kernel) gives the eager loop's bits, with labels and without (the shared-timestep forward); after
    set_prediction_type('eps') the cached v graph is not replayed: the output is a fresh eps sampler's."""
    from diffusion_models_collection_amd.diffusion import DDIM, DPMSolver
    m, _ = build(NAME)
    m.eval()
    make = (lambda **kw: DDIM(1000, 10, device=DEV, **kw)) if kind == "ddim" else (
        lambda **kw: DPMSolver(1000, 10, device=DEV, **kw))
    smp = make(prediction_type="v")
    shape = (4, 3, 16, 16)
    xT = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(31))
    y = torch.tensor([1, 2, 3, 4], device=DEV)

    def run(s, graph):
        monkeypatch.setenv("DMC_GRAPH", graph)
        return s.sample(m, shape, y, x_T=xT), s.sample(m, shape, None, x_T=xT)

    eager = run(smp, "0")
    assert not smp.__dict__.get("_step_graphs")
    graphed = run(smp, "1")
    assert len(smp.__dict__["_step_graphs"]) == 2
    for a, b in zip(eager, graphed):
        assert bool(a.isfinite().all()) and torch.equal(a, b)
    smp.set_prediction_type("eps")
    assert not smp.__dict__.get("_step_graphs")
    after = run(smp, "1")
    fresh = run(make(), "1")
    for a, b, c in zip(after, fresh, graphed):
        assert torch.equal(a, b) and not torch.equal(a, c)
