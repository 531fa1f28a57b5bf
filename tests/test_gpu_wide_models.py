"""Models whose attention head dim is above 64: the ADM-size UNet (model_channels=256 with channel_mult=(1, 2): 512
channels = 4 heads of 128 at its attention levels) and DiTs with hidden_size / num_heads of 72 (DiT-XL's 1152 / 16) and
128, through the 128-wide attention kernels of csrc/dmc_attn.hip. The patterns and tolerances are those of the tests
named in each docstring (tests/test_gpu_protocol.py, tests/test_gpu_model.py); the kernels on their own are in
tests/test_gpu_attn_wide.py."""
import pytest
import torch

from test_gpu_model import cos, rel
from test_oracle import perturb_dit

pytestmark = pytest.mark.gpu
DEV = "cuda"

# 8x8: head dim 64 at the 8x8 level (C = 256), 128 at the 4x4 level and in the middle block (C = 512, L = 16)
WIDE8 = dict(image_size=(8, 8), in_channels=3, model_channels=256, out_channels=3, num_res_blocks=1,
             attention_resolutions=(8, 4), dropout=0.0, channel_mult=(1, 2), num_classes=None, use_attention=True)
# 16x16: C = 512 = 4 heads of 128 at both levels, L = 256 and L = 64 (bf16: the row-resident kernels, one and four
# heads' rows per block)
WIDE16 = dict(WIDE8, image_size=(16, 16), channel_mult=(2, 2), attention_resolutions=(16, 8))


@pytest.fixture(scope="module")
def wide8_oracle_grads():
    """The oracle's fp32 forward + backward of one p_losses (B = 2) of the seed-7 WIDE8 network on the host, once for
    both dtypes: (x0, t, noise, loss, {name: grad})."""
    from diffusion_models_collection_amd.models import UNet
    from oracle.unet_oracle import make_oracle
    from oracle import diffusion_oracle as DO
    torch.manual_seed(7)
    m = UNet(**WIDE8)
    gen = torch.Generator().manual_seed(29)
    x0 = torch.rand(2, 3, 8, 8, generator=gen) * 2 - 1
    t = torch.tensor([5, 900])
    noise = torch.randn(2, 3, 8, 8, generator=gen)
    orc, sd = make_oracle(m.state_dict(), WIDE8, requires_grad=True)
    out = orc.forward(DO.q_sample(DO.schedule(), x0, t, noise), t, None, training=True)
    loss = ((out - noise) ** 2).mean()
    loss.backward()
    return x0, t, noise, loss.item(), {k: v.grad.detach().clone() for k, v in sd.items()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wide_unet_grads_match_oracle(dtype, wide8_oracle_grads):
    """One p_losses + backward of WIDE8 against the oracle, in the shape and with the tolerances of
    test_cifar_unet_b128_grads_match_oracle: fp32 -- loss within 1e-5 relative, every gradient within 5e-4 of its
    absmax; bf16 -- loss within 1e-3 relative, rel < 5e-2 and cosine > 0.999 for every gradient with a norm >= 1e-3 of
    the largest (the rest cosine > 0.99), the global gradient norm within 2e-3."""
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.diffusion import DDPM
    x0, t, noise, lref, gref = wide8_oracle_grads
    torch.manual_seed(7)
    m = UNet(**WIDE8, compute_dtype=dtype).to(DEV).train()
    loss = DDPM(device=DEV).p_losses(m, x0.to(DEV), t.to(DEV), noise=noise.to(DEV))
    loss.backward()
    got = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}
    assert set(got) == set(gref)
    lrel = abs(loss.item() - lref) / abs(lref)
    norms = {k: v.norm().item() for k, v in gref.items()}
    big = max(norms.values())
    worst, worst_rel, worst_cos = (0.0, ""), 0.0, 1.0
    for k, g in gref.items():
        if dtype == "fp32":
            e = (got[k] - g).abs().max().item() / max(g.abs().max().item(), 1e-30)
            worst = max(worst, (e, k))
            assert e < 5e-4, (k, e)
        else:
            c = cos(got[k], g)
            r = (got[k] - g).norm().item() / max(norms[k], 1e-30)
            if norms[k] >= 1e-3 * big:
                worst_rel, worst_cos = max(worst_rel, r), min(worst_cos, c)
                assert c > 0.999 and r < 0.05, (k, c, r)
            else:
                assert c > 0.99, (k, c, r)
    tot_r = sum(n * n for n in norms.values()) ** 0.5
    tot_g = sum(v.norm().item() ** 2 for v in got.values()) ** 0.5
    print(f"wide UNet {dtype} vs oracle: loss rel {lrel:.2e}; "
          + (f"worst grad err/absmax {worst[0]:.2e} ({worst[1]})" if dtype == "fp32" else
             f"worst rel {worst_rel:.3e}, worst cos {worst_cos:.6f}") + f"; grad norm {tot_g:.6f} vs {tot_r:.6f}")
    if dtype == "fp32":
        assert lrel < 1e-5, lrel
    else:
        assert lrel < 1e-3, lrel
        assert abs(tot_g - tot_r) < 2e-3 * tot_r


def test_wide_unet16_bf16_forward_matches_fp32():
    """WIDE16 in eval mode: the bf16 forward (128-wide resident attention at L = 256 and L = 64) against the fp32 HIP
    forward (the staged 128-wide kernels) of the same weights, at the bf16 row tolerance of
    test_cifar_unet_b128_rows_match_oracle: 5e-2 of max |ref| and cosine > 0.999."""
    from diffusion_models_collection_amd.models import UNet
    torch.manual_seed(9)
    ref_m = UNet(**WIDE16, compute_dtype="fp32").to(DEV).eval()
    m = UNet(**WIDE16, compute_dtype="bf16").to(DEV).eval()
    m.load_state_dict(ref_m.state_dict())
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, 16, 16, generator=gen).to(DEV)
    t = torch.tensor([17, 640], device=DEV)
    with torch.no_grad():
        ref = ref_m(x, t).float().cpu()
        got = m(x, t).float().cpu()
    e, c = rel(got, ref), cos(got, ref)
    print(f"wide UNet 16x16 bf16 vs fp32: rel {e:.3e} cos {c:.6f}")
    assert torch.isfinite(ref).all() and e < 5e-2 and c > 0.999, (e, c)


DITS = {"hd72": dict(img_size=(8, 8), patch_size=2, in_channels=3, hidden_size=1152, depth=1, num_heads=16,
                     mlp_ratio=4.0, num_classes=10, dropout=0.0),
        "hd128": dict(img_size=(8, 8), patch_size=2, in_channels=3, hidden_size=768, depth=1, num_heads=6,
                      mlp_ratio=4.0, num_classes=10, dropout=0.0)}


@pytest.mark.parametrize("name", list(DITS))
def test_wide_dit_backward_matches_oracle(name):
    """Loss and every parameter gradient (fp32, one block, B = 2) against the oracle, as
    test_dit_hidden768_backward_matches_oracle: loss within 1e-5, gradients rel < 5e-4."""
    from diffusion_models_collection_amd.models import DiT
    from diffusion_models_collection_amd.diffusion import DDPM
    from oracle import diffusion_oracle as DO
    from oracle.dit_oracle import make_oracle
    cfg = DITS[name]
    torch.manual_seed(3)
    m = perturb_dit(DiT(**cfg), 0.02).to(DEV).train()
    orc, sd = make_oracle(m.state_dict(), cfg, requires_grad=True)
    x0 = torch.rand(2, 3, 8, 8) * 2 - 1
    t = torch.tensor([3, 801])
    y = torch.tensor([0, 7])
    noise = torch.randn_like(x0)
    lref = DO.loss("l2", noise, orc.forward(DO.q_sample(DO.schedule(), x0, t, noise), t, y))
    lref.backward()
    loss = DDPM(device=DEV).p_losses(m, x0.to(DEV), t.to(DEV), y.to(DEV), noise=noise.to(DEV))
    loss.backward()
    assert abs(loss.item() - lref.item()) < 1e-5 * max(1.0, abs(lref.item()))
    worst = max((rel(p.grad, sd[k].grad), k) for k, p in m.named_parameters())
    print(f"wide DiT {name} vs oracle: loss {loss.item():.7f} vs {lref.item():.7f}; worst grad rel {worst[0]:.2e} "
          f"({worst[1]})")
    for k, p in m.named_parameters():
        assert rel(p.grad, sd[k].grad) < 5e-4, (k, rel(p.grad, sd[k].grad))


def test_wide_dit_trains_with_attention_dropout():
    """DiT-XL's head dim (72) in train mode with dropout 0.1, bf16: the attention-probability dropout of the 128-wide
    kernels inside a model. The step runs, loss and gradients are finite, the dropout is on (the loss differs from
    eval mode's), and the same seed gives the same bits."""
    from diffusion_models_collection_amd.models import DiT
    from diffusion_models_collection_amd.diffusion import DDPM
    cfg = dict(DITS["hd72"], dropout=0.1)
    torch.manual_seed(3)
    m = perturb_dit(DiT(**cfg, compute_dtype="bf16"), 0.02).to(DEV)
    gen = torch.Generator().manual_seed(41)
    x0 = (torch.rand(2, 3, 8, 8, generator=gen) * 2 - 1).to(DEV)
    noise = torch.randn(2, 3, 8, 8, generator=gen).to(DEV)
    t = torch.tensor([3, 801], device=DEV)
    y = torch.tensor([0, 7], device=DEV)
    ddpm = DDPM(device=DEV)

    def step(train):
        m.train() if train else m.eval()
        m.zero_grad(set_to_none=True)
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        loss = ddpm.p_losses(m, x0, t, y, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().float().cpu(), {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}

    l1, g1 = step(True)
    l2, g2 = step(True)
    le, _ = step(False)
    assert torch.isfinite(l1) and all(bool(torch.isfinite(g.float()).all()) for g in g1.values())
    assert torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    assert not torch.equal(l1, le)


def test_wide_unet_ddim_graph_matches_eager(monkeypatch):
    """DDIM with 3 inference steps on WIDE8 in bf16, B = 2: the replayed step graph gives the bits of the eager loop
    (the form of test_ddim_sample_graph_matches_eager)."""
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.diffusion import DDIM
    torch.manual_seed(3)
    m = UNet(**WIDE8, compute_dtype="bf16").to(DEV).eval()
    ddim = DDIM(1000, 3, device=DEV)
    xT = torch.randn(2, 3, 8, 8, device=DEV)
    outs = []
    for g in ("0", "1"):
        monkeypatch.setenv("DMC_GRAPH", g)
        with torch.no_grad():
            outs.append(ddim.sample(m, tuple(xT.shape), None, x_T=xT))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
