"""GPU parity of the DiM backbone (models/dim.py of the reference) for both token mixers.

  attention mixer, fp32: against tests/golden/dim_tiny_attn*.npz (the reference's own DiM with its attention fallback)
      at the DiT bounds of test_gpu_dit.py: output within 2e-5 of max |ref|, every gradient within 2e-4.
  Mamba mixer, fp32: against tests/dim_reference.py in fp64; bound = max(the DiT bounds, 4x dim_reference's own
      fp32-CPU error).
  bf16, both mixers: error against fp64 at most 2x the error of dim_reference with bf16-rounded GEMM operands, output
      cosine > 0.999, gradient cosine > 0.99.
  Batch independence, graphed DDIM sampling with CFG, graphed DiffusionTrainer steps with dropout, checkpoints.
"""
import functools

import pytest
import torch

from dim_reference import TINY_ATTN, load_tiny_attn, make_reference, perturb

pytestmark = pytest.mark.gpu
DEV = "cuda"

MAMBA = {
    "sq16": (dict(img_size=(16, 16), patch_size=2, in_channels=3, hidden_size=64, depth=2, state_size=16,
                  mlp_ratio=4.0, num_classes=10, dropout=0.0, mixer="mamba"), 2),
    "h40": (dict(img_size=(8, 24), patch_size=2, in_channels=3, hidden_size=40, depth=2, state_size=16,
                 mlp_ratio=2.0, num_classes=None, dropout=0.0, mixer="mamba"), 3),        # R = 3, E = 80, L = 48
    "l1": (dict(img_size=(2, 2), patch_size=2, in_channels=3, hidden_size=64, depth=1, state_size=16,
                mlp_ratio=4.0, num_classes=10, dropout=0.0, mixer="mamba"), 2),           # L = 1
}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


def cos(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return torch.nn.functional.cosine_similarity(a, b, dim=0).item()


def _model(cfg, dtype="fp32", seed=1234):
    from diffusion_models_collection_amd.models import DiM
    torch.manual_seed(seed)
    return perturb(DiM(**cfg, compute_dtype=dtype), 0.05)


def _inputs(cfg, B):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, cfg["in_channels"], *cfg["img_size"], generator=g)
    t = torch.tensor([17, 903, 500, 0][:B], dtype=torch.long)
    y = torch.tensor([0, 11, 3, 10][:B], dtype=torch.long) if cfg["num_classes"] is not None else None
    cot = torch.randn(x.shape, generator=g)
    return x, t, y, cot


def _ref_run(sd, cfg, x, t, y, cot, dtype, **kw):
    ref, p = make_reference(sd, cfg, dtype=dtype, requires_grad=True, **kw)
    xr = x.to(dtype).clone().requires_grad_(True)
    out = ref.forward(xr, t, y)
    (out * cot.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in p.items() if v.grad is not None}
    grads["x"] = xr.grad
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _references(key):
    """(state_dict, inputs, fp64 run, fp32 run, fp32 run with bf16-rounded GEMM operands) of one configuration, shared
    by the fp32 and bf16 tests."""
    cfg, B = MAMBA[key] if key in MAMBA else (TINY_ATTN, 2)
    sd = {k: v.detach().clone() for k, v in _model(cfg).state_dict().items()}
    inp = _inputs(cfg, B)
    runs = {"f64": _ref_run(sd, cfg, *inp, torch.float64), "f32": _ref_run(sd, cfg, *inp, torch.float32),
            "bf16": _ref_run(sd, cfg, *inp, torch.float32, bf16_gemm=True)}
    return cfg, sd, inp, runs


def _gpu_run(cfg, sd, inp, dtype):
    from diffusion_models_collection_amd.models import DiM
    m = DiM(**cfg, compute_dtype=dtype)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    x, t, y, cot = inp
    xg = x.to(DEV).requires_grad_(True)
    out = m(xg, t.to(DEV), None if y is None else y.to(DEV))
    (out * cot.to(DEV)).sum().backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["x"] = xg.grad
    return m, out.detach(), grads


def test_dim_attention_fp32_matches_reference_fixture():
    from diffusion_models_collection_amd.models import DiM
    g, params, grads = load_tiny_attn()
    m = DiM(**TINY_ATTN)
    m.load_state_dict(params)
    m = m.to(DEV).train()
    x = g["x"].to(DEV).requires_grad_(True)
    out = m(x, g["t"].to(DEV), g["y"].to(DEV))
    assert rel(out, g["out"]) < 2e-5, rel(out, g["out"])
    (out * g["cot"].to(DEV)).sum().backward()
    assert rel(x.grad, g["grad_x"]) < 2e-4, rel(x.grad, g["grad_x"])
    for k, p in m.named_parameters():
        assert rel(p.grad, grads[k]) < 2e-4, (k, rel(p.grad, grads[k]))
    m.eval()
    with torch.no_grad():
        o2 = m(g["x"].to(DEV), g["t"].to(DEV), None)
    assert rel(o2, g["out_ynone"]) < 2e-5


@pytest.mark.parametrize("key", list(MAMBA))
def test_dim_mamba_fp32_matches_fp64_reference(key):
    cfg, sd, inp, runs = _references(key)
    o64, g64 = runs["f64"]
    o32, g32 = runs["f32"]
    _, out, grads = _gpu_run(cfg, sd, inp, "fp32")
    e, y = rel(out, o64), rel(o32, o64)
    print(f"dim mamba {key} fp32: out {e:.2e} (fp32-CPU {y:.2e})")
    fails = []
    if not e <= max(2e-5, 4 * y):
        fails.append(("out", e, y))
    for k, r in g64.items():
        e, y = rel(grads[k], r), rel(g32[k], r)
        print(f"  grad {k}: {e:.2e} (fp32-CPU {y:.2e})")
        if not e <= max(2e-4, 4 * y):
            fails.append((k, e, y))
    assert not fails, fails


@pytest.mark.parametrize("key", ["sq16", "attn"])
def test_dim_bf16_cosines(key):
    """The DiT criteria of test_gpu_dit.py: output cosine > 0.999, every gradient's cosine > 0.99 (against fp64)."""
    cfg, sd, inp, runs = _references(key)
    o64, g64 = runs["f64"]
    _, out, grads = _gpu_run(cfg, sd, inp, "bf16")
    assert cos(out, o64) > 0.999, cos(out, o64)
    worst = min((cos(grads[k], r), k) for k, r in g64.items())
    assert worst[0] > 0.99, worst


@pytest.mark.parametrize("key", ["sq16", "attn"])
def test_dim_bf16_within_twice_the_bf16_gemm_reference(key):
    """Error against fp64, per tensor relative to its absmax, at most 2x that of dim_reference with bf16-rounded GEMM
    operands (forward and backward GEMMs). Floor: the fp32 bounds (2e-5 output, 2e-4 gradients) -- a tensor no bf16
    GEMM touches (the output bias gradient, a plain sum of the cotangent) has a yardstick of fp32 rounding noise,
    1e-7, and bf16 mode is not asked for more than fp32 mode is.

    The executor keeps fp32 what the criterion needs fp32: the gradient rows the LayerNorm backward sums over tokens
    (their GEMMs store fp32), the upstream gradient of the GELU backward, the branch bias gradients (taken from the
    fp32 stream gradient, dmc_gate_bwd_bias) and the output bias gradient. Measured: largest ratio 1.76
    (blocks.1.mamba_block.norm.weight 8.83e-3 / 5.01e-3), output 2.77e-3 / 2.31e-3 (Mamba), 3.35e-3 / 3.41e-3
    (attention)."""
    cfg, sd, inp, runs = _references(key)
    o64, g64 = runs["f64"]
    ob, gb = runs["bf16"]
    _, out, grads = _gpu_run(cfg, sd, inp, "bf16")
    e, y = rel(out, o64), rel(ob, o64)
    print(f"dim {key} bf16: out {e:.2e} (bf16-GEMM reference {y:.2e}) cos {cos(out, o64):.6f}")
    fails = []
    if not e <= max(2 * y, 2e-5):
        fails.append(("out", e, y))
    for k, r in g64.items():
        e, y = rel(grads[k], r), rel(gb[k], r)
        print(f"  grad {k}: {e:.2e} (bf16-GEMM reference {y:.2e}) ratio {e / max(y, 1e-30):.2f}")
        if not e <= max(2 * y, 2e-4):
            fails.append((k, f"{e:.2e}", f"{y:.2e}"))
    assert not fails, fails


@pytest.mark.parametrize("mixer", ["mamba", "attention"])
def test_dim_batch_independence_and_graphed_sampling(mixer, monkeypatch):
    """The fp32 rows of a B = 16 forward equal the B = 2 rows within 1e-5; DDIM-5 with CFG: the graphed loop equals
    the eager loop bitwise."""
    from diffusion_models_collection_amd.diffusion import DDIM
    cfg = dict(TINY_ATTN, mixer=mixer)
    m = _model(cfg).to(DEV).eval()
    torch.manual_seed(0)
    x = torch.randn(16, 3, 16, 16)
    t = torch.randint(0, 1000, (16,))
    y = torch.randint(0, 11, (16,))
    with torch.no_grad():
        a = m(x.to(DEV), t.to(DEV), y.to(DEV))
        b = m(x[:2].to(DEV), t[:2].to(DEV), y[:2].to(DEV))
    assert rel(b, a[:2]) < 1e-5, rel(b, a[:2])
    ddim = DDIM(1000, 5, device=DEV)
    xT = torch.randn(4, 3, 16, 16)
    yy = torch.tensor([1, 2, 3, 4])
    outs = []
    for gr in ("0", "1"):
        monkeypatch.setenv("DMC_GRAPH", gr)
        with torch.no_grad():
            outs.append(ddim.sample_with_cfg(m, (4, 3, 16, 16), yy.to(DEV), cfg_scale=3.0, x_T=xT.to(DEV)).cpu())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def _trainer(mixer, graph, monkeypatch, save_dir, dropout=0.1, dtype="bf16"):
    from diffusion_models_collection_amd.diffusion import DDPM
    from diffusion_models_collection_amd.models import DiM
    from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer
    mp = dict(TINY_ATTN, mixer=mixer, dropout=dropout)
    mp.pop("num_classes")
    monkeypatch.setenv("DMC_GRAPH", "1" if graph else "0")
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    m = perturb(DiM(**mp, num_classes=10, compute_dtype=dtype), 0.02).to(DEV)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    cfg = {"epochs": 1, "save_dir": str(save_dir), "sample_dir": str(save_dir), "loss_type": "l2", "use_ema": True,
           "ema_decay": 0.99, "conditional": True, "num_classes": 10, "cfg_dropout_prob": 0.2, "model_type": "dim",
           "model_params": dict(mp)}
    tr = DiffusionTrainer(m, DDPM(device=DEV), None, opt, None, device=DEV, config=cfg)
    m.train()
    return m, tr


def _steps(tr, n, seed=5):
    torch.manual_seed(seed)            # the trainer draws timesteps, noise and label dropout from torch's generators
    torch.cuda.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    losses = []
    for i in range(n):
        x = (torch.rand(8, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
        losses.append(tr.train_step((x, torch.randint(0, 10, (8,), generator=gen).to(DEV)), i).detach().float().cpu()
                      .reshape(()))
    torch.cuda.synchronize()
    return torch.stack(losses)


@pytest.mark.parametrize("mixer", ["mamba", "attention"])
def test_dim_train_step_graphed_matches_eager(mixer, monkeypatch, tmp_path):
    """DiffusionTrainer on a DiM (bf16, dropout 0.1: the two feed-forward dropouts and, for the attention mixer, the
    attention-probability dropout are inside the graph; EMA, label dropout): the fused flat AdamW and the HIP-graph
    step run for the DiM executor, and 3 graphed steps equal 3 eager steps bitwise."""
    res = []
    for graph in (False, True):
        m, tr = _trainer(mixer, graph, monkeypatch, tmp_path)
        assert tr._flat is not None and (tr._graph is not None) == graph
        losses = _steps(tr, 3)
        res.append((losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                    {k: v.detach().cpu().clone() for k, v in tr.ema_model.state_dict().items()}))
        if graph:
            assert tr._graph.graph is not None and not tr._graph.failed
    (le, se, ee), (lg, sg, eg) = res
    assert torch.isfinite(le).all()
    assert torch.equal(le, lg), (le, lg)
    for k in se:
        assert torch.equal(se[k], sg[k]), k
        assert torch.equal(ee[k], eg[k]), k


def test_dim_checkpoint_roundtrip(monkeypatch, tmp_path):
    """save_checkpoint -> fresh DiM and trainer -> load_checkpoint -> the next step's loss is identical."""
    m, tr = _trainer("mamba", False, monkeypatch, tmp_path, dropout=0.0, dtype="fp32")
    _steps(tr, 2)
    tr.save_checkpoint(1)
    nxt = _steps(tr, 1, seed=9)
    m2, tr2 = _trainer("mamba", False, monkeypatch, tmp_path, dropout=0.0, dtype="fp32")
    tr2.load_checkpoint(tmp_path / "current_model.pth")
    for k, v in m.state_dict().items():
        assert v.shape == m2.state_dict()[k].shape
    assert torch.equal(_steps(tr2, 1, seed=9), nxt)
