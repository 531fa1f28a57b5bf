"""Grouped weight gradients (dmc_conv2d_wgrad_group: several 3x3 convs of one map width in one wgrad3x3_pipe_kernel
launch, or several 1x1 convs in one wgrad1x1_glds_kernel launch, each conv split 1 / njobs as often) against
torch.nn.grad.conv2d_weight in fp32 on the same bf16-rounded operands (rel_err < 1e-5, the bound
test_wgrad_pipe_kernel applies to this kernel), and the executor's grouped backward against its ungrouped one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5


def rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12)).item()


# job: (N, H, C1, C2, Cout, dy pitch, bias); maps are H x H. A group runs at the default one-round block target
# (DMC_WG_HALO_TARGET = 256: at these sizes one tile per split) or at a smaller one that makes the planner share
# more than one tile per split, as the B = 128 layers do.
MIXED16 = [(2, 16, 64, 0, 64, 64, True), (3, 16, 64, 64, 200, 200, False), (2, 16, 128, 0, 3, 8, True)]
MIXED16_DEEP = [(3, 16, 64, 0, 64, 64, True), (5, 16, 64, 64, 200, 200, False), (2, 16, 128, 0, 3, 8, True)]
OW32 = [(1, 32, 64, 0, 64, 64, True), (1, 32, 128, 0, 64, 64, False)]
GROUPS = {
    # a group of one job: the single-conv plan
    "one": (0, [(2, 16, 64, 0, 64, 64, True)]),
    # job boundaries in the block table, concat sources, ragged Cout, a narrow Cout in a padded dy pitch, per-job
    # bias-partial offsets; 4 / 6 / 4 tiles: one tile per split (half 1 idle, 60 blocks) ...
    "mixed16": (0, MIXED16),
    # ... and the same layers with 6 / 10 / 4 tiles at three tiles per split: ragged last splits (10 = 3 + 3 + 3 + 1),
    # odd tile counts (half 1 one short), 38 blocks with the job boundaries at 2 and 34
    "mixed16_deep": (44, MIXED16_DEEP),
    # one tile in all (half 1 has none, splits = 1) next to a 3-tile job
    "single_tile8": (0, [(2, 8, 64, 0, 64, 64, True), (6, 8, 64, 0, 64, 64, False)]),
    # 8 tiles each: 24 blocks at one tile per split, 12 (no multiple of 8: the XCD remap's tail) at two
    "ow32": (0, OW32),
    "ow32_tps2": (20, OW32),
    # many splits from few output tiles
    "many_splits": (0, [(16, 16, 64, 0, 64, 64, True), (16, 16, 64, 0, 64, 64, False)]),
    # the 1x1 kind (wgrad1x1_glds_kernel): concat sources with a bias on 8x8 maps (M = 128: one split of two stages)
    # next to a ragged Cout on 16x16 maps (M = 1024: four splits), different map sizes in one launch
    "g1x1": (0, [(2, 8, 256, 128, 256, 256, True), (4, 16, 64, 0, 72, 72, False)], 1),
    # M = 5 x 64 pixels next to M = 128: a shared 256-pixel split leaves the first job a ragged second split
    "g1x1_320": (0, [(5, 8, 64, 0, 64, 64, True), (2, 8, 128, 0, 64, 64, False)], 1),
}


def _make(group):
    """Operands of a group on the device, the descriptors, and the fp32 references (computed once per group)."""
    from diffusion_models_collection_amd import _lib as L, kernels as K
    gen = torch.Generator().manual_seed(1000 + sum(sum(j[:6]) for j in GROUPS[group][1]))
    dt = torch.bfloat16
    jobs = []
    ks = GROUPS[group][2] if len(GROUPS[group]) > 2 else 3
    for N, H, C1, C2, Cout, ld, bias in GROUPS[group][1]:
        x = torch.randn(N, H, H, C1 + C2, generator=gen).to(dt)
        g = torch.randn(N, H, H, Cout, generator=gen).to(dt)
        gp = torch.zeros(N, H, H, ld, dtype=dt)
        gp[..., :Cout] = g
        xr, gr = x.permute(0, 3, 1, 2).float(), g.permute(0, 3, 1, 2).float()
        wr = torch.nn.grad.conv2d_weight(xr, (Cout, C1 + C2, ks, ks), gr, padding=ks // 2)
        br = gr.sum((0, 2, 3)) if bias else None
        d = K.make_desc(dt, N, H, H, C1, C2, C1, C2, L.kc_for(C1 + C2, dt), H, H, Cout, K.TAPS3 if ks == 3 else K.TAPS1)
        x1 = x[..., :C1].contiguous().to(DEV)
        x2 = x[..., C1:].contiguous().to(DEV) if C2 else None
        jobs.append(dict(d=d, dy=gp.to(DEV), ld=ld, x1=x1, x2=x2, Cout=Cout, Ctot=C1 + C2, bias=bias, wr=wr, br=br,
                         ks=ks))
    return jobs


_CACHE = {}


def _group(name, dmc_opt=None):
    """The group's jobs (operands and references shared by the tests and by the two targets of one job list)."""
    target, spec = GROUPS[name][:2]
    key = id(spec)
    if key not in _CACHE:
        _CACHE[key] = _make(name)
    if target:
        dmc_opt("DMC_WG_HALO_TARGET", target)
    return _CACHE[key]


def _run(jobs, defer=None):
    """One grouped call; outputs pre-filled with NaN so an unwritten element fails."""
    from diffusion_models_collection_amd import kernels as K
    outs, items = [], []
    for j in jobs:
        dw = torch.full((j["Cout"], j["Ctot"], j["ks"], j["ks"]), float("nan"), device=DEV)
        db = torch.full((j["Cout"],), float("nan"), device=DEV) if j["bias"] else None
        items.append((j["d"], j["dy"], j["ld"], j["x1"], j["x2"], dw, 1.0, db))
        outs.append((dw, db))
    K.wgrad_group(items, defer=defer)
    if defer is not None:
        defer.end_segment()
    torch.cuda.synchronize()
    return [(dw.cpu(), None if db is None else db.cpu()) for dw, db in outs]


def _check(jobs, got):
    for j, (dw, db) in zip(jobs, got):
        assert torch.isfinite(dw).all()
        e = rel_err(dw, j["wr"])
        print("dw rel_err", e)
        assert e < TOL, e
        if j["bias"]:
            assert torch.isfinite(db).all()
            e = rel_err(db, j["br"])
            print("dbias rel_err", e)
            assert e < TOL, e


def _same(a, b):
    for (aw, ab), (bw, bb) in zip(a, b):
        assert torch.equal(aw, bw)
        assert ab is None or torch.equal(ab, bb)


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_matches_fp32_reference(name, dmc_opt):
    """Every job of the group against the fp32 reference; twice with bitwise equal results; and through K.WgradDefer
    with every = 0 (all reductions in one batch), bitwise the direct call's."""
    from diffusion_models_collection_amd import kernels as K
    jobs = _group(name, dmc_opt)
    a = _run(jobs)
    _check(jobs, a)
    _same(a, _run(jobs))
    defer = K.WgradDefer()
    defer.every = 0
    _same(a, _run(jobs, defer))
    assert not defer.jobs and not defer.pending and not defer.pending1


@pytest.mark.parametrize("name,idx", [("one", 0), ("g1x1", 0), ("g1x1", 1), ("g1x1_320", 0)])
def test_group_of_one_bitwise_single(name, idx):
    """A group of one job, 3x3 or 1x1, has the single-layer plan: bitwise dmc_conv2d_wgrad of that job (g1x1_320:
    M = 320 pixels, where a shared 256-pixel split would differ from the single plan's one split of 320)."""
    from diffusion_models_collection_amd import kernels as K
    j = _group(name)[idx]
    (gw, gb), = _run([j])
    dw = torch.full((j["Cout"], j["Ctot"], j["ks"], j["ks"]), float("nan"), device=DEV)
    db = torch.full((j["Cout"],), float("nan"), device=DEV) if j["bias"] else None
    K.wgrad(j["d"], j["dy"], j["ld"], j["x1"], j["x2"], dw, 1.0, dbias=db)
    torch.cuda.synchronize()
    assert torch.equal(gw, dw.cpu()) and (gb is None or torch.equal(gb, db.cpu()))


def test_block_counts(dmc_opt):
    """The plans the shapes above are chosen for (host-side: the workspace query's per-job bytes give the splits)."""
    import ctypes
    from diffusion_models_collection_amd import _lib as L

    def splits(name):
        jobs = _group(name, dmc_opt)
        arr = (L.WgradGroupItem * len(jobs))()
        for i, j in enumerate(jobs):
            arr[i].d = ctypes.pointer(j["d"])
            arr[i].ld_dy = j["ld"]
        sizes = (ctypes.c_size_t * len(jobs))()
        assert L.LIB.dmc_conv2d_wgrad_group_workspace(arr, len(jobs), sizes)
        L.reset_options(from_env=False)
        out = []
        for j, s in zip(jobs, sizes):
            per = (j["Cout"] * j["Ctot"] * j["ks"] ** 2 + (j["Cout"] + 127) // 128 * 128) * 4
            assert s % per == 0
            out.append(s // per)
        return out

    def blocks(name):
        return sum(s * (j["Ctot"] // 64) * ((j["Cout"] + 63) // 64) for j, s in zip(_group(name, dmc_opt), splits(name)))

    assert splits("single_tile8") == [1, 3]
    assert splits("many_splits") == [32, 32]
    assert splits("mixed16") == [4, 6, 4] and blocks("mixed16") == 60
    assert splits("mixed16_deep") == [2, 4, 2] and blocks("mixed16_deep") == 38
    assert splits("ow32") == [8, 8] and blocks("ow32") == 24
    assert splits("ow32_tps2") == [4, 4] and blocks("ow32_tps2") == 12
    assert splits("g1x1") == [1, 4]     # 256 pixels per split: 3 x 2 x 1 + 1 x 1 x 4 = 10 blocks


def test_group_rejects_mixed_widths_and_ineligible_jobs():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    a, b = _group("one")[0], _group("single_tile8")[0]
    item = lambda j: (j["d"], j["dy"], j["ld"], j["x1"], j["x2"],   # noqa: E731
                      torch.empty(j["Cout"], j["Ctot"], 3, 3, device=DEV), 1.0, None)
    with pytest.raises(L.DMCError):
        K.wgrad_group([item(a), item(b)])
    with pytest.raises(L.DMCError):
        K.wgrad_group([item(a), item(_group("g1x1")[1])])      # a 3x3 and a 1x1 job
    d2 = K.make_desc(torch.bfloat16, 2, 16, 16, 64, 0, 64, 0, 64, 8, 8, 64, K.TAPS3, stride=2)
    assert L.LIB.dmc_conv2d_wgrad_group_ok(d2, 64) == 0
    assert L.LIB.dmc_conv2d_wgrad_group_ok(_group("g1x1")[1]["d"], 72) == 1
    assert L.LIB.dmc_conv2d_wgrad_group_ok(a["d"], 64) == 16


def _unet_grads(monkeypatch, group, hook=False):
    from diffusion_models_collection_amd.models import UNet
    from diffusion_models_collection_amd.diffusion import DDPM
    monkeypatch.setenv("DMC_WG_DEFER", group)
    torch.manual_seed(0)
    m = UNet(image_size=(16, 16), in_channels=3, model_channels=64, out_channels=3, num_res_blocks=1,
             attention_resolutions=(8,), dropout=0.1, channel_mult=(1, 2), use_attention=True,
             compute_dtype="bf16").to(DEV).train()
    ddpm = DDPM(device=DEV)
    gen = torch.Generator().manual_seed(9)
    x0 = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).to(DEV)
    t = torch.randint(0, 1000, (2,), generator=gen).to(DEV)
    noise = torch.randn(2, 3, 16, 16, generator=gen).to(DEV)
    seen = []
    if hook:
        def grad_hook(flat, hi, last):
            seen.append((hi, flat[:hi].clone()))
        m.executor.grad_hook = grad_hook
    ex = m.executor
    runs, hooks, flats = [], [], []
    for _ in range(2):
        torch.manual_seed(7)      # the dropout seeds follow torch's CPU generator
        m.zero_grad(set_to_none=True)
        # the flat gradient buffer is reused from backward to backward: poison it, so a gradient that is written late
        # (or never) shows as NaN at hook time and cannot be mistaken for the previous backward's equal value
        if getattr(ex, "_flat", None) is None:
            ex._flat = torch.empty(ex.gtotal, dtype=torch.float32, device=DEV)
        ex._flat.fill_(float("nan"))
        poisoned = ex._flat
        del seen[:]
        ddpm.p_losses(m, x0, t, noise=noise).backward()
        torch.cuda.synchronize()
        assert ex.flat is poisoned                     # the backward wrote the buffer that was poisoned
        runs.append([p.grad.clone() for p in m.parameters()])
        hooks.append(list(seen))
        flats.append(ex.flat.clone())
    assert ex._wg_arena.group == int(group if group else 4)
    return runs, hooks, flats


def test_executor_grouped_backward(monkeypatch):
    """A small train-mode UNet: the backward with the group switch at its default and at 1 agree on every parameter
    gradient (rel_err < 1e-5), each setting is bitwise reproducible, and with a grad_hook installed every published
    prefix of the flat gradient buffer is final when the hook sees it."""
    from diffusion_models_collection_amd import kernels as K
    monkeypatch.delenv("DMC_WG_DEFER", raising=False)
    default = str(K.WgradDefer().group)
    assert int(default) > 1
    K.wgrad_slab_bytes(reset=True)
    (g1, g1b), _, _ = _unet_grads(monkeypatch, "1")
    slab1 = K.wgrad_slab_bytes(reset=True)
    (gd, gdb), _, _ = _unet_grads(monkeypatch, default)
    slabd = K.wgrad_slab_bytes(reset=True)
    print("slab bytes per two backwards: group 1", slab1, "default", slabd)
    assert 0 < slabd <= slab1   # (equal here: at B = 2 every conv already has one tile per split)
    for a, b in zip(g1, g1b):
        assert torch.equal(a, b)
    for a, b in zip(gd, gdb):
        assert torch.equal(a, b)
    for i, (a, b) in enumerate(zip(gd, g1)):
        assert torch.isfinite(a).all()
        assert rel_err(a, b) < TOL, (i, tuple(a.shape), rel_err(a, b))
    (gh, ghb), hooks, flats = _unet_grads(monkeypatch, default, hook=True)
    for a, b, c in zip(gh, ghb, gd):
        assert torch.equal(a, c) and torch.equal(b, c)
    for seen, flat in zip(hooks, flats):               # both backwards, each into a NaN-poisoned buffer
        assert torch.isfinite(flat).all()
        assert len(seen) > 2 and seen[-1][0] == flat.numel()
        assert any(0 < hi < flat.numel() for hi, _ in seen)
        for hi, prefix in seen:
            assert torch.equal(prefix, flat[:hi]), hi   # (a NaN left at hook time is unequal to anything)
