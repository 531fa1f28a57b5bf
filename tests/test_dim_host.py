"""CPU tests of the DiM backbone's host side: module tree and state_dict layout for both token mixers, mixer
selection, refused configurations, initialisation, and the test references themselves (tests/dim_reference.py against
the fixture the reference's own DiM produced, tests/mamba_reference.py's wiring around the scan)."""
import math

import pytest
import torch
import torch.nn.functional as F

from dim_reference import TINY_ATTN, load_tiny_attn, make_reference
from mamba_reference import MAMBA_KEYS, mamba_block

# mamba_ssm.Mamba(d_model=H, d_state=N, d_conv=4, expand=2).state_dict(), E = 2H, R = ceil(H / 16): written from
# knowledge of mamba_ssm, which is not a dependency -- unverified
MAMBA_STATE_DICT = [("A_log", lambda H, E, N, R: (E, N)), ("D", lambda H, E, N, R: (E,)),
                    ("in_proj.weight", lambda H, E, N, R: (2 * E, H)), ("conv1d.weight", lambda H, E, N, R: (E, 1, 4)),
                    ("conv1d.bias", lambda H, E, N, R: (E,)), ("x_proj.weight", lambda H, E, N, R: (R + 2 * N, E)),
                    ("dt_proj.weight", lambda H, E, N, R: (E, R)), ("dt_proj.bias", lambda H, E, N, R: (E,)),
                    ("out_proj.weight", lambda H, E, N, R: (H, E))]


def _dim(**kw):
    from diffusion_models_collection_amd.models import DiM
    return DiM(**kw)


def test_attention_state_dict_matches_reference_fixture():
    """Same keys, shapes, order and (seeded) values as the reference's DiM with its attention fallback."""
    from dim_reference import perturb
    _, params, _ = load_tiny_attn()
    torch.manual_seed(1234)
    sd = perturb(_dim(**TINY_ATTN), 0.05).state_dict()
    assert list(sd) == list(params)
    for k in sd:
        assert sd[k].shape == params[k].shape, k
        assert torch.equal(sd[k], params[k]), k
    mix = [k for k in sd if k.startswith("blocks.0.mamba_block.mamba.")]
    assert mix == ["blocks.0.mamba_block.mamba." + s for s in
                   ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")]


@pytest.mark.parametrize("H", [64, 40, 384])
def test_mamba_state_dict_is_the_pinned_list(H):
    m = _dim(img_size=(8, 8), hidden_size=H, depth=2, num_classes=10, mixer="mamba")
    dims = (H, 2 * H, 16, math.ceil(H / 16))
    sd = m.state_dict()
    for i in range(2):
        pre = f"blocks.{i}.mamba_block."
        keys = [k for k in sd if k.startswith(pre)]
        want = ([pre + "norm.weight", pre + "norm.bias"] + [pre + "mamba." + k for k, _ in MAMBA_STATE_DICT]
                + [pre + "adaLN_modulation.1.weight", pre + "adaLN_modulation.1.bias"])
        assert keys == want
        for k, shp in MAMBA_STATE_DICT:
            assert tuple(sd[pre + "mamba." + k].shape) == shp(*dims), k
    assert [k for k, _ in MAMBA_STATE_DICT] == MAMBA_KEYS
    # everything outside the mixer is the attention variant's tree
    a = _dim(img_size=(8, 8), hidden_size=64, depth=1, num_classes=10, mixer="attention").state_dict()
    b = _dim(img_size=(8, 8), hidden_size=64, depth=1, num_classes=10, mixer="mamba").state_dict()
    strip = lambda sd_: [(k, tuple(v.shape)) for k, v in sd_.items() if ".mamba_block.mamba." not in k]  # noqa: E731
    assert strip(a) == strip(b)


def test_mixer_selection():
    with pytest.raises(NotImplementedError, match=r"mamba_ssm.*model_params\['mixer'\]"):
        _dim()
    for mixer in ("mamba", "attention"):
        m = _dim(img_size=(8, 8), hidden_size=64, depth=1, mixer=mixer)
        assert m.mixer == mixer
        assert any(k.endswith("mamba.A_log") for k in m.state_dict()) == (mixer == "mamba")
    from diffusion_models_collection_amd._lib import DMCError
    with pytest.raises(DMCError, match="mixer"):
        _dim(img_size=(8, 8), hidden_size=64, depth=1, mixer="rnn")


def test_invalid_configurations_raise():
    from diffusion_models_collection_amd._lib import DMCError
    with pytest.raises(DMCError, match="head dim of at most 64"):
        _dim(hidden_size=768, depth=1, mixer="attention")          # 8 heads of 96
    with pytest.raises(DMCError, match="multiple of 8"):
        _dim(hidden_size=96, depth=1, mixer="attention", compute_dtype="bf16")   # head dim 12
    _dim(img_size=(8, 8), hidden_size=96, depth=1, mixer="attention", compute_dtype="fp32")
    for n in (8, 32):
        with pytest.raises(DMCError, match="state_size 16 only"):
            _dim(hidden_size=64, depth=1, state_size=n, mixer="mamba")
    m = _dim(img_size=(8, 8), hidden_size=64, depth=1, mixer="mamba")
    with pytest.raises(RuntimeError, match="cuda"):
        m(torch.zeros(1, 3, 8, 8), torch.zeros(1, dtype=torch.long))


def test_initialisation():
    m = _dim(img_size=(8, 8), hidden_size=64, depth=2, num_classes=10, mixer="mamba")
    for blk in m.blocks:
        mm = blk.mamba_block.mamba
        assert torch.equal(mm.A_log, torch.log(torch.arange(1, 17, dtype=torch.float32)).repeat(128, 1))
        assert torch.equal(mm.D, torch.ones(128))
        for lin in (mm.in_proj, mm.x_proj, mm.dt_proj, mm.out_proj):
            bound = math.sqrt(6.0 / (lin.in_features + lin.out_features))      # xavier_uniform_
            assert lin.weight.abs().max() <= bound and lin.weight.abs().max() > 0.5 * bound
        assert mm.in_proj.bias is None and mm.x_proj.bias is None and mm.out_proj.bias is None
        assert torch.count_nonzero(mm.dt_proj.bias) == 0           # the reference's init ignores _no_reinit
        assert mm.conv1d.weight.shape == (128, 1, 4) and mm.conv1d.weight.abs().max() <= 0.5   # torch default
        for sub in (blk.mamba_block, blk.ff_block):
            assert torch.count_nonzero(sub.adaLN_modulation[1].weight) == 0
            assert torch.count_nonzero(sub.adaLN_modulation[1].bias) == 0
            assert torch.equal(sub.norm.weight, torch.ones(64)) and torch.count_nonzero(sub.norm.bias) == 0
        assert torch.count_nonzero(blk.ff_block.mlp[0].bias) == 0
    fl = m.final_layer
    for p in (fl.adaLN_modulation[1].weight, fl.adaLN_modulation[1].bias, fl.linear.weight, fl.linear.bias):
        assert torch.count_nonzero(p) == 0
    assert 0.015 < m.pos_embed.std() < 0.025


def test_executor_gradient_layout_covers_every_parameter():
    """The flat gradient buffer (backward-completion order) holds every parameter exactly once, for both mixers; the
    stacked adaLN rows are adjacent (3H + 3H per block, the final 2H last)."""
    for mixer in ("mamba", "attention"):
        m = _dim(img_size=(8, 8), hidden_size=64, depth=2, num_classes=10, mixer=mixer)
        ex = m.executor
        spans = sorted((ex.goff[i], ex.goff[i] + p.numel()) for i, p in enumerate(ex.params))
        assert spans[0][0] == 0 and spans[-1][1] == ex.gtotal == sum(p.numel() for p in m.parameters())
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert ex.ada_total == 2 * 6 * 64 + 2 * 64 and ex.ada_off == [0, 384, 768]
        assert [lin.weight.shape[0] for lin in ex.ada] == [192, 192, 192, 192, 128]


def test_dim_reference_reproduces_reference_fixture():
    """tests/dim_reference.py (attention) against the reference's own DiM: forward, y=None forward and every
    gradient, at the bounds tests/test_oracle.py uses for the DiT oracle."""
    g, params, grads = load_tiny_attn()
    ref, sd = make_reference(params, TINY_ATTN, requires_grad=True)
    x = g["x"].clone().requires_grad_(True)
    out = ref.forward(x, g["t"], g["y"])
    torch.testing.assert_close(out, g["out"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ref.forward(g["x"], g["t"], None), g["out_ynone"], rtol=1e-5, atol=1e-5)
    (out * g["cot"]).sum().backward()
    torch.testing.assert_close(x.grad, g["grad_x"], rtol=1e-4, atol=1e-5)
    assert set(grads) == {k for k in sd if sd[k].grad is not None}
    for k, r in grads.items():
        torch.testing.assert_close(sd[k].grad, r, rtol=1e-4, atol=1e-5, msg=k)


def _mamba_params(H, gen, dtype=torch.float64):
    E, N, R = 2 * H, 16, math.ceil(H / 16)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=dtype)    # noqa: E731
    return {"A_log": torch.log(torch.arange(1, N + 1, dtype=dtype)).repeat(E, 1) + 0.1 * rn(E, N),
            "D": 1 + 0.1 * rn(E), "in_proj.weight": rn(2 * E, H) / math.sqrt(H), "conv1d.weight": 0.5 * rn(E, 1, 4),
            "conv1d.bias": 0.1 * rn(E), "x_proj.weight": rn(R + 2 * N, E) / math.sqrt(E),
            "dt_proj.weight": rn(E, R) / math.sqrt(R), "dt_proj.bias": 0.5 * rn(E),
            "out_proj.weight": rn(H, E) / math.sqrt(E)}


def test_mamba_reference_without_x_proj_is_the_skip_path():
    """x_proj.weight = 0 gives Bm = Cm = 0, so the state never leaves 0 and the block is out_proj((D u) silu(z)):
    guards the wiring around the scan (projection order, the x / z split, the causal conv's alignment)."""
    gen = torch.Generator().manual_seed(3)
    H, B, L = 24, 2, 9
    p = _mamba_params(H, gen)
    p["x_proj.weight"] = torch.zeros_like(p["x_proj.weight"])
    h = torch.randn(B, L, H, generator=gen, dtype=torch.float64)
    E = 2 * H
    xz = h @ p["in_proj.weight"].T
    x, z = xz[..., :E], xz[..., E:]
    u = torch.zeros_like(x)
    for t in range(L):          # the conv written out token by token: u_t sees x_{t-3..t} of its own image only
        pre = p["conv1d.bias"].clone().expand(B, E).clone()
        for k in range(4):
            if t - 3 + k >= 0:
                pre = pre + p["conv1d.weight"][:, 0, k] * x[:, t - 3 + k]
        u[:, t] = F.silu(pre)
    want = ((p["D"] * u) * F.silu(z)) @ p["out_proj.weight"].T
    torch.testing.assert_close(mamba_block(h, p), want, rtol=1e-12, atol=1e-12)


def test_mamba_reference_is_causal_and_per_image():
    """Changing token t changes no output before t, and no other image."""
    gen = torch.Generator().manual_seed(4)
    H, B, L = 16, 2, 12
    p = _mamba_params(H, gen)
    h = torch.randn(B, L, H, generator=gen, dtype=torch.float64)
    a = mamba_block(h, p)
    h2 = h.clone()
    h2[0, 7] += 1.0
    b = mamba_block(h2, p)
    assert torch.equal(a[0, :7], b[0, :7]) and torch.equal(a[1], b[1]) and not torch.equal(a[0, 7:], b[0, 7:])
