"""The output-parity folds of the two resampling convs (include/dmc.h dmc_conv_resample_fold, DMC_RESAMPLE_FOLD).

Upsample forward: after a nearest-x2 upsample output pixel (2i+a, 2j+b) is a 2x2-tap conv of the low-resolution input
with summed weights (DMC_PACK_UPFOLD). Downsample input gradient: dx(2i+a, 2j+b) takes only the taps that meet a
non-zero of the zero-stuffed dy (DMC_PACK_DOWNDGRAD). Both run as four classes in one launch of the LDS-DMA kernel.

Tolerances are those of test_gpu_kernels.py test_conv_forward / test_conv_dgrad_wgrad: bf16 rel_err < 2e-2 against an
fp32 CPU reference on dtype-rounded inputs; GroupNorm statistics 2e-5 (test_conv_epilogue_groupnorm_partials). The
plain form of these small shapes would split K, and the planner keeps a split-K plan unfolded, so the kernel tests run
with DMC_NO_SPLITK = 1 (in both arms of a comparison) and assert that the fold is in fact taken. The "default_plan"
cases are large enough (65536 output pixels) that plan_fold takes the fold with every option at its default.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def _lib():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12)).item()


def q(x):
    return x.to(BF).float()


# ---------------------------------------------------------------------------------------------------------
# packs
def _up_sets(par, r):
    """3x3 tap indices of parity `par` that read low-resolution offset par - 1 + r: floor((par + k - 1) / 2)."""
    return [k for k in range(3) if (par + k - 1) // 2 == par - 1 + r]


def ref_upfold(w, Kc):
    """[class a*2+b][Cout][tap r*2+c][Kc]: fp32 sum in ascending tap order, one rounding."""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(4, Cout, 4, Kc, dtype=BF, device=w.device)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for c in range(2):
                    v = torch.zeros(Cout, Cin, device=w.device)
                    for ky in _up_sets(a, r):
                        for kx in _up_sets(b, c):
                            v = v + w[:, :, ky, kx]
                    out[a * 2 + b, :, r * 2 + c, :Cin] = v.to(BF)
    return out.flatten()


def ref_downdgrad(w, Kc):
    """[class a*2+b][Cin][taps][Kc] over output-channel columns: parity 0 keeps tap 1, parity 1 the taps 0 and 2,
    ky-major."""
    Cout, Cin = w.shape[:2]
    blocks = []
    for a in range(2):
        for b in range(2):
            kys, kxs = ([0, 2] if a else [1]), ([0, 2] if b else [1])
            blk = torch.zeros(Cin, len(kys) * len(kxs), Kc, dtype=BF, device=w.device)
            for iy, ky in enumerate(kys):
                for ix, kx in enumerate(kxs):
                    blk[:, iy * len(kxs) + ix, :Cout] = w[:, :, ky, kx].t().to(BF)
            blocks.append(blk.flatten())
    return torch.cat(blocks)


@pytest.mark.parametrize("Cout,Cin", [(48, 24), (20, 72)])
def test_fold_packs_bitwise(Cout, Cin):
    """Both class-ordered packs, through dmc_pack_weight and through the batched dmc_pack_weights, are bitwise the
    torch reference ((20, 72): Kc pads 72 -> 128 input columns and 20 -> 64 output columns)."""
    L, K = _lib()
    torch.manual_seed(3)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV)
    for mode, Kc, ref in ((L.PACK_UPFOLD, L.kc_for(Cin, BF), ref_upfold), (L.PACK_DOWNDGRAD, L.kc_for(Cout, BF), ref_downdgrad)):
        want = ref(w, Kc)
        single = K.pack_weight(mode, BF, w, Kc)
        batch = torch.full_like(single, 7.0)
        K.PackBatch([(w, batch, 0, mode, Cout, Cin, 3, 3, Kc, -1)], DEV).launch()
        torch.cuda.synchronize()
        assert single.numel() == want.numel()
        assert torch.equal(single, want), mode
        assert torch.equal(batch, want), mode


# ---------------------------------------------------------------------------------------------------------
# folded forward
def _up_desc(L, K, dt, N, H, W, C, Cout, bias, resid, part):
    d = K.make_desc(dt, N, H, W, C, 0, C, 0, L.kc_for(C, dt), 2 * H, 2 * W, Cout, K.TAPS3, L.MODE_UPSAMPLE)
    K.set_epilogue(d, bias=bias, resid=resid, ld_res=0 if resid is None else Cout, ldy1=Cout, gn_part=part)
    return d


def _run_like_executor(L, K, d, dt, w, x, y, plain_pack):
    """What ExecCore._conv does with fold=True: ask, set, pass the matching pack. Returns the fold taken."""
    d.fold = K.conv_fold(d)
    wp = K.pack_weight(L.FOLD_PACK.get(d.fold, plain_pack), dt, w, d.Kc)
    K.conv(d, x, None, wp, y)
    return d.fold


# (N, low-res H, W, C, Cout): the issue's shape (H != W, three images, a ragged channel tile, 64 x 128 tiles, the
# GroupNorm partials from a pass); the same with whole channel tiles (partials from tile_epilogue8); 128 blocks (the
# 128 x 128 tile on the 3-stage ring, partials from reg_epilogue) and 320 blocks (the 2-stage ring); default options
UP_CASES = {"issue": (3, 8, 16, 64, 192), "epi8": (3, 8, 16, 64, 128), "tile128": (8, 16, 32, 64, 128),
            "ring2": (20, 16, 32, 64, 128), "default_plan": (64, 16, 16, 64, 128)}


@pytest.mark.parametrize("case", list(UP_CASES))
def test_folded_upsample_forward(case, dmc_opt):
    L, K = _lib()
    if case != "default_plan":
        dmc_opt("DMC_NO_SPLITK", 1)
    N, H, W, C, Cout = UP_CASES[case]
    G = 8
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(C * 9)
    bias = torch.randn(Cout, generator=g)
    resid = torch.randn(N, Cout, 2 * H, 2 * W, generator=g)
    ref = F.conv2d(F.interpolate(q(x), scale_factor=2, mode="nearest"), q(w), bias, padding=1) + q(resid)
    xd, rd = nhwc(x).to(BF).to(DEV), nhwc(resid).to(BF).to(DEV)
    y = torch.empty(N, 2 * H, 2 * W, Cout, dtype=BF, device=DEV)
    part = torch.empty(N * 4 * H * W // 64 * (Cout // 8) * 2, device=DEV)
    d = _up_desc(L, K, BF, N, H, W, C, Cout, bias.to(DEV), rd, part)
    assert _run_like_executor(L, K, d, BF, w.to(DEV), xd, y, L.PACK_FWD) == L.FOLD_UP
    plan = K.conv_plan(d)
    assert plan.grid[2] == 4 and L.CONV_FAMILIES[plan.family] == "glds"
    want_gn = L.GN_PART_PASS if case == "issue" else L.GN_PART_KERNEL
    assert plan.gn_part == want_gn, plan.gn_part
    torch.cuda.synchronize()
    got = nchw(y.float().cpu())
    e = rel_err(got, ref)
    print(f"{case}: rel_err {e:.3e}")
    assert e < 2e-2, e
    # the border rows and columns of every class on their own: a padding error must not hide in the mean
    for a in range(2):
        for b in range(2):
            gc, rc = got[:, :, a::2, b::2], ref[:, :, a::2, b::2]
            for name, sl in (("top", (slice(0, 1), slice(None))), ("bottom", (slice(-1, None), slice(None))),
                             ("left", (slice(None), slice(0, 1))), ("right", (slice(None), slice(-1, None)))):
                eb = rel_err(gc[:, :, sl[0], sl[1]], rc[:, :, sl[0], sl[1]])
                assert eb < 2e-2, (a, b, name, eb)
    # finalised GroupNorm statistics of the stored output: against torch, and against the statistics pass
    gamma, beta = torch.randn(Cout, generator=g).to(DEV), torch.randn(Cout, generator=g).to(DEV)
    sc, sh, mr = K.gn_finalize(part, Cout, None, 0, N, 4 * H * W, G, 1e-5, gamma, beta)
    rsc, rsh, rmr = K.gn_stats(BF, y, None, N, 4 * H * W, Cout, 0, Cout, 0, G, 1e-5, gamma, beta)
    torch.cuda.synchronize()
    yg = y.double().cpu().view(N, 4 * H * W, G, Cout // G)
    mean = yg.mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(yg.var(dim=(1, 3), unbiased=False) + 1e-5)
    mrc = mr.cpu().view(N, G, 2)
    assert rel_err(mrc[..., 0], mean) < 2e-5 and rel_err(mrc[..., 1], rstd) < 2e-5
    for a_, b_ in ((mr, rmr), (sc, rsc), (sh, rsh)):
        assert rel_err(a_, b_) < 2e-5, (case, rel_err(a_, b_))


# ---------------------------------------------------------------------------------------------------------
# folded stride-2 input gradient
# (N, dy H, W, forward Cin (dx channels), forward Cout (dy channels)): the issue's shape, then 128 x 128 tiles
DOWN_CASES = {"issue": (3, 8, 16, 64, 128), "tile128": (8, 16, 32, 64, 128), "ring2": (20, 16, 32, 128, 64),
              "default_plan": (64, 16, 16, 64, 128)}


@pytest.mark.parametrize("case", list(DOWN_CASES))
def test_folded_stride2_dgrad(case, dmc_opt):
    """Bitwise the dilated form (DMC_RESAMPLE_FOLD = 0), with and without the accumulating residual (in place, as the
    executor's gradient buffers), and within the bf16 tolerance of autograd."""
    L, K = _lib()
    if case != "default_plan":
        dmc_opt("DMC_NO_SPLITK", 1)
    N, H, W, Cin, Cout = DOWN_CASES[case]
    g = torch.Generator().manual_seed(9)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cout * 9 / 4)
    dy = torch.randn(N, Cout, H, W, generator=g)
    acc0 = torch.randn(N, Cin, 2 * H, 2 * W, generator=g)
    ref = F.conv_transpose2d(q(dy), q(w), stride=2, padding=1, output_padding=1)
    dyd, wd = nhwc(dy).to(BF).to(DEV), w.to(DEV)
    Kc = L.kc_for(Cout, BF)

    def run(fold_opt, accumulate):
        dmc_opt("DMC_RESAMPLE_FOLD", fold_opt)
        out = nhwc(acc0).to(BF).to(DEV) if accumulate else torch.empty(N, 2 * H, 2 * W, Cin, dtype=BF, device=DEV)
        d = K.make_desc(BF, N, H, W, Cout, 0, Cout, 0, Kc, 2 * H, 2 * W, Cin, K.TAPS3_DGRAD, L.MODE_DILATE)
        K.set_epilogue(d, resid=out if accumulate else None, ld_res=Cin if accumulate else 0, ldy1=Cin)
        fold = _run_like_executor(L, K, d, BF, wd, dyd, out, L.PACK_DGRAD)
        assert fold == (L.FOLD_DOWN_DGRAD if fold_opt else L.FOLD_NONE)
        assert K.conv_plan(d).splits == 1
        torch.cuda.synchronize()
        return out

    for accumulate in (False, True):
        folded, plain = run(1, accumulate), run(0, accumulate)
        assert torch.equal(folded, plain), (case, accumulate)
        want = ref + q(acc0) if accumulate else ref
        e = rel_err(nchw(folded.float().cpu()), want)
        print(f"{case} accumulate={accumulate}: rel_err {e:.3e}")
        assert e < 2e-2, e


# ---------------------------------------------------------------------------------------------------------
# fallbacks
@pytest.mark.parametrize("case", ["up_4x4", "down_odd", "up_fp32", "down_fp32", "up_splitk"])
def test_fold_fallbacks_keep_the_plain_path(case, dmc_opt):
    """A 4x4 low-resolution forward (no whole 64-pixel segment per class), an odd-sized input gradient, fp32, and a
    conv the planner splits K for are not folded: the same bits with the option on and off."""
    L, K = _lib()
    dt = torch.float32 if case.endswith("fp32") else BF
    if case != "up_splitk":
        dmc_opt("DMC_NO_SPLITK", 1)
    g = torch.Generator().manual_seed(13)
    N, C = 3, 64
    outs = []
    for opt in (1, 0):
        dmc_opt("DMC_RESAMPLE_FOLD", opt)
        if case.startswith("up"):
            H = W = 4 if case == "up_4x4" else 8
            x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(1)).to(dt).to(DEV)
            w = (torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(2)) * 0.05).to(DEV)
            y = torch.empty(N, 2 * H, 2 * W, C, dtype=dt, device=DEV)
            d = _up_desc(L, K, dt, N, H, W, C, C, None, None, None)
            fold = _run_like_executor(L, K, d, dt, w, x, y, L.PACK_FWD)
        else:
            OH = 15 if case == "down_odd" else 16       # dx 15x15 <- dy 8x8: the last row / column has no odd partner
            dy = torch.randn(N, 8, 8, C, generator=torch.Generator().manual_seed(1)).to(dt).to(DEV)
            w = (torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(2)) * 0.05).to(DEV)
            y = torch.empty(N, OH, OH, C, dtype=dt, device=DEV)
            d = K.make_desc(dt, N, 8, 8, C, 0, C, 0, L.kc_for(C, dt), OH, OH, C, K.TAPS3_DGRAD, L.MODE_DILATE)
            K.set_epilogue(d, ldy1=C)
            fold = _run_like_executor(L, K, d, dt, w, dy, y, L.PACK_DGRAD)
        assert fold == L.FOLD_NONE, case
        torch.cuda.synchronize()
        outs.append(y)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------
# executor level
TINY = dict(image_size=(16, 16), in_channels=3, model_channels=16, out_channels=3, num_res_blocks=1,
            attention_resolutions=(8,), dropout=0.0, channel_mult=(1, 2), num_classes=None, use_attention=True)


def _count_folds(monkeypatch, K):
    taken = []
    orig = K.conv_fold

    def counting(d):
        f = orig(d)
        taken.append(f)
        return f

    monkeypatch.setattr(K, "conv_fold", counting)
    return taken


@pytest.mark.parametrize("channels", [16, 64])
def test_unet_step_fold_on_off(channels, dmc_opt, monkeypatch):
    """The small two-level UNet (tests/golden/gen_golden.py unet_tiny_uncond, 16x16) at B = 2, one p_losses +
    backward in bf16 with the option on and off: the bf16 tolerance of test_gpu_protocol.py's gradient check (loss
    within 1e-3 relative; per tensor of norm >= 1e-3 of the largest cosine > 0.999 and relative error < 5e-2, the
    rest cosine > 0.99). With the golden config's 16 / 32 channels no conv has 64-channel sources, so nothing folds
    (the two runs take the same kernels); the 64-channel variant folds its Upsample forward (8x8 -> 16x16) and its
    Downsample input gradient, which is asserted."""
    L, K = _lib()
    from diffusion_models_collection_amd.diffusion import DDPM
    from diffusion_models_collection_amd.models import UNet
    dmc_opt("DMC_NO_SPLITK", 1)
    taken = _count_folds(monkeypatch, K)
    cfg = dict(TINY, model_channels=channels)
    gen = torch.Generator().manual_seed(21)
    x0 = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
    t = torch.tensor([100, 700], device=DEV)
    noise = torch.randn(2, 3, 16, 16, generator=gen).to(DEV)
    ddpm = DDPM(device=DEV)
    res = []
    for opt in (1, 0):
        dmc_opt("DMC_RESAMPLE_FOLD", opt)
        del taken[:]
        torch.manual_seed(0)
        m = UNet(**cfg, compute_dtype="bf16").to(DEV).train()
        loss = ddpm.p_losses(m, x0, t, None, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.item(), {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters()}))
        want = {L.FOLD_UP, L.FOLD_DOWN_DGRAD} if (opt and channels == 64) else set()
        assert set(taken) - {L.FOLD_NONE} == want, (opt, taken)
        del m
    (l1, g1), (l0, g0) = res
    assert abs(l1 - l0) < 1e-3 * abs(l0), (l1, l0)
    norms = {k: v.norm().item() for k, v in g0.items()}
    big = max(norms.values())
    for k in g0:
        c = F.cosine_similarity(g1[k].flatten(), g0[k].flatten(), dim=0).item()
        r = (g1[k] - g0[k]).norm().item() / max(norms[k], 1e-30)
        if norms[k] >= 1e-3 * big:
            assert c > 0.999 and r < 5e-2, (k, c, r)
        else:
            assert c > 0.99, (k, c, r)


def test_graphed_step_equals_eager_with_fold(dmc_opt, monkeypatch):
    """The HIP-graph training step equals the eager one bit for bit with the folds taken (64-channel two-level UNet,
    bf16, 5 steps: 2 eager warm-up steps, capture, replays)."""
    L, K = _lib()
    from diffusion_models_collection_amd.diffusion import DDPM
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.utils.trainer import DiffusionTrainer
    dmc_opt("DMC_NO_SPLITK", 1)
    taken = _count_folds(monkeypatch, K)
    mp = dict(TINY, model_channels=64)

    def run(graph):
        monkeypatch.setenv("DMC_GRAPH", "1" if graph else "0")
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        m = UNet(**mp, compute_dtype="bf16").to(DEV)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
        cfg = {"epochs": 1, "save_dir": "/tmp/dmc_fold_ckpt", "sample_dir": "/tmp/dmc_fold_smp", "loss_type": "l2",
               "use_ema": True, "ema_decay": 0.99, "conditional": False, "num_classes": None, "cfg_dropout_prob": 0.2, "model_type": "unet",
               "model_params": dict(mp)}
        tr = DiffusionTrainer(m, DDPM(device=DEV), None, opt, None, device=DEV, config=cfg)
        m.train()
        gen = torch.Generator().manual_seed(5)
        losses = []
        for i in range(5):
            x = (torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
            losses.append(tr.train_step(x, i).detach().float().cpu().reshape(()))
        torch.cuda.synchronize()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        return torch.stack(losses), sd, tr

    le, se, _ = run(False)
    lg, sg, trg = run(True)
    assert {L.FOLD_UP, L.FOLD_DOWN_DGRAD} <= set(taken)
    assert trg._graph.graph is not None and not trg._graph.failed
    assert torch.equal(le, lg), (le, lg)
    for k in se:
        assert torch.equal(se[k], sg[k]), k
