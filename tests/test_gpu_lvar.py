"""Learned variances on the GPU, the kernels alone: dmc_hybrid_objective, dmc_ddpm_step_learned and
dmc_vlb_step_learned against the float64 restatement (tests/lvar_reference.py) and against the kernels already tested.

Bounds. Losses and the vb / eps_mse rows: relative error <= 1e-5 against float64 (the project's fp32-loss bound);
xstart_mse: max(1e-5, 4 x the float32 restatement's own error), as tests/test_gpu_vlb.py. Gradients and x_prev:
criterion 2 (tests/test_gpu_elem_kernels.py judge: per row, error <= 4 x the float32 restatement's error + 1 ulp); the
v gradient of a t = 0 row may instead be within 1e-5 x max|ref64| of the row, since the device's erfc and exp are not
the host's there. Every figure is printed before it is asserted.
"""
import functools

import pytest
import torch

import lvar_reference as R
from test_gpu_elem_kernels import (DEV, DDPM_TABS, F32, F64, dev, guard_ok, guarded, judge, same_bits, tables,
                                   ulp32)
from test_gpu_vlb import LOSS_RTOL, POOL, SHAPES, check_next, rel, vlb_inputs

pytestmark = pytest.mark.gpu

PTYPES = ["eps", "v"]
HAND = 3        # vlb_inputs hand-places the first three predictions of a sample (per >= 5): the last on the 1e-12 floor


def _lib():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


def ac():
    return tables()["alphas_cumprod"]


@functools.lru_cache(maxsize=None)
def lvar_table(ptype):
    from diffusion_models_collection_amd.diffusion import _vlb
    return torch.from_numpy(_vlb.learned_coefficients(ac().numpy(), ptype))


@functools.lru_cache(maxsize=None)
def snr_weights(ptype):
    from diffusion_models_collection_amd.diffusion import _objective
    return torch.from_numpy(_objective.min_snr_weights(ac().numpy(), 5.0, ptype))


@functools.lru_cache(maxsize=None)
def lvar_inputs(N, per, ptype, sigma=1.0, rot=0):
    """vlb_inputs plus the noise that made x_t (recovered in float64), v in [-1.5, 1.5] with -1 and +1 hand-placed, and
    out = [pred | v] as the model returns it, [N, 2 per]. CPU tensors, never modified."""
    x0, x_t, pred, t, z_next, t_next = vlb_inputs(N, per, ptype, sigma, rot)
    a = ac().double()[t].view(-1, 1)
    noise = ((x_t.double() - a.sqrt() * x0.double()) / (1 - a).sqrt()).float()
    g = torch.Generator().manual_seed(77 * N + per)
    v = torch.rand(N, per, generator=g) * 3 - 1.5
    v[:, per - 1] = -1.0
    if per >= 2:
        v[:, per // 2] = 1.0
    out = torch.cat([pred, v], 1).contiguous()
    return dict(x0=x0, x_t=x_t, pred=pred, t=t, z_next=z_next, t_next=t_next, noise=noise, v=v, out=out)


def obj_tabs():
    tb = tables()
    return tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"]


def floor_check(what, pr64, t, per):
    """From the float64 restatement: only hand-placed elements (the first HAND of a t = 0 row) sit on the 1e-12 floor,
    the third always does, and nothing else is near it."""
    on = (pr64 < 1e-12) & (t == 0).view(-1, 1)
    if per >= 5:
        assert bool(on[t == 0][:, HAND - 1].all()), what
        assert not bool(on[:, HAND:].any()), what
        others = pr64[t == 0][:, HAND:]
        assert others.numel() == 0 or float(others.min()) > 1e-9, (what, float(others.min()))
    else:
        assert not bool(on.any()), what
    return on


def judge_v(what, got, ref32, ref64, t):
    """Criterion 2 per row; a t = 0 row may instead be within LOSS_RTOL * max|ref64| of the row."""
    g, r32 = got.detach().cpu().double(), ref32.double()
    err = (g - ref64).abs().amax(1)
    cal = (r32 - ref64).abs().amax(1)
    big = ref64.abs().amax(1)
    bound = 4 * cal + ulp32(big)
    bound = torch.where(t == 0, torch.maximum(bound, LOSS_RTOL * big), bound)
    print(f"{what}: v-gradient err per row {err.tolist()}, fp32 restatement {cal.tolist()}, bound {bound.tolist()}")
    assert bool((err <= bound).all()), (what, err.tolist(), bound.tolist())


def run_hybrid(K, ins, ptype, loss_type, w, vlb_weight, dloss=1.0, grad=True):
    N = ins["x0"].shape[0]
    sa, s1 = obj_tabs()
    dout, dbuf = guarded(tuple(ins["out"].shape)) if grad else (None, None)
    g = torch.tensor(dloss, dtype=F32, device=DEV) if grad else None
    loss, _ = K.hybrid_objective(ptype, loss_type, dev(ins["out"]), dev(ins["x0"]), dev(ins["noise"]), dev(ins["t"]),
                                 dev(sa), dev(s1), dev(lvar_table(ptype)), w=dev(w), vlb_weight=vlb_weight, dloss=g,
                                 grad=grad, dout=dout)
    return loss, dout, dbuf


# ------------------------------------------------------------------------------------------------------------
# dmc_hybrid_objective
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", PTYPES)
@pytest.mark.parametrize("N,per", SHAPES)
def test_hybrid_objective(N, per, ptype):
    L, K = _lib()
    ins = lvar_inputs(N, per, ptype)
    t = ins["t"]
    if N >= 5:
        assert {0, 1, 500, 999} <= set(t.tolist())
    out3 = ins["out"].view(N, 2, per)
    for loss_type, w, vw, dl in (("l2", None, 0.001, 1.0), ("huber", snr_weights(ptype), 0.5, 0.37)):
        what = f"hybrid {N}x{per} {ptype} {loss_type} w={'snr' if w is not None else None} vlb_weight {vw}"
        r64, g64, pr64 = R.hybrid(F64, ac(), ptype, t, out3, ins["x0"], ins["noise"], loss_type, w, vw, dl, obj_tabs())
        r32, g32, _ = R.hybrid(F32, ac(), ptype, t, out3, ins["x0"], ins["noise"], loss_type, w, vw, dl, obj_tabs())
        assert r64.dtype == F64 and r32.dtype == F32
        on = floor_check(what, pr64, t, per)
        loss, dout, dbuf = run_hybrid(K, ins, ptype, loss_type, w, vw, dl)
        e = rel(loss, r64)
        print(f"{what}: loss {loss.tolist()} rel err {e.tolist()} (fp32 restatement {rel(r32, r64).tolist()})")
        assert loss.dtype == F32 and bool(loss.isfinite().all())
        assert bool((e <= LOSS_RTOL).all()), (what, e.tolist())
        d3 = dout.cpu().view(N, 2, per)
        assert bool(d3.isfinite().all()), what
        judge(f"{what}: prediction gradient", d3[:, 0], g32[:, 0], g64[:, 0], rows=N)
        judge_v(what, d3[:, 1], g32[:, 1], g64[:, 1], t)
        assert bool((d3[:, 1][on] == 0).all()) and bool((g64[:, 1][on] == 0).all()), what
        fwd, _, _ = run_hybrid(K, ins, ptype, loss_type, w, vw, grad=False)
        same_bits(f"{what}: forward alone", fwd, loss.cpu())
        loss2, dout2, dbuf2 = run_hybrid(K, ins, ptype, loss_type, w, vw, dl)
        same_bits(f"{what}: second run, loss", loss2, loss.cpu())
        same_bits(f"{what}: second run, gradient", dout2, dout.cpu())
        guard_ok(what, dbuf, dbuf2)


@pytest.mark.parametrize("ptype", PTYPES)
@pytest.mark.parametrize("N,per", SHAPES)
def test_hybrid_weight_zero_is_the_objective(N, per, ptype):
    """vlb_weight = 0: the prediction half's gradient and loss[1] have dmc_objective's bits, the v half's is all zeros."""
    L, K = _lib()
    ins = lvar_inputs(N, per, ptype)
    sa, s1 = (dev(v) for v in obj_tabs())
    for loss_type, w in (("l2", None), ("l1", snr_weights(ptype)), ("huber", None)):
        what = f"hybrid vlb_weight 0 {N}x{per} {ptype} {loss_type}"
        loss, dout, dbuf = run_hybrid(K, ins, ptype, loss_type, w, 0.0, 0.37)
        g = torch.tensor(0.37, dtype=F32, device=DEV)
        ref, dref = K.objective(ptype, loss_type, dev(ins["pred"]), dev(ins["x0"]), dev(ins["noise"]), dev(ins["t"]),
                                sa, s1, dev(w), dloss=g)
        d3 = dout.cpu().view(N, 2, per)
        same_bits(f"{what}: loss[1]", loss[1], ref.cpu())
        same_bits(f"{what}: loss[0]", loss[0], ref.cpu())
        same_bits(f"{what}: prediction gradient", d3[:, 0], dref.cpu())
        assert bool((d3[:, 1] == 0).all()) and float(loss[2]) == 0.0, what
        guard_ok(what, dbuf)


@pytest.mark.parametrize("which", ["out", "x0", "noise", "dout", "v_half"])
def test_hybrid_misaligned_base(which):
    """One operand starts 4 bytes into its buffer (or per % 4 != 0 puts the v half off 16 bytes): the element-wise path,
    the same bounds."""
    L, K = _lib()
    N, per = 3, 66 if which == "v_half" else 64
    ins = lvar_inputs(N, per, "eps")
    sa, s1 = (dev(v) for v in obj_tabs())
    ops = {"out": dev(ins["out"]), "x0": dev(ins["x0"]), "noise": dev(ins["noise"])}
    ops["dout"], dbuf = guarded((N, 2 * per))
    sbuf = None
    if which != "v_half":
        shifted, sbuf = guarded((ops[which].numel() + 1,))
        view = shifted[1:].view(ops[which].shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        if which != "dout":
            view.copy_(ops[which])
        ops[which] = view
    else:
        assert (ops["out"].data_ptr() + 4 * per) % 16 != 0
    g = torch.ones((), dtype=F32, device=DEV)
    loss, dout = K.hybrid_objective("eps", "l2", ops["out"], ops["x0"], ops["noise"], dev(ins["t"]), sa, s1,
                                    dev(lvar_table("eps")), vlb_weight=0.001, dloss=g, dout=ops["dout"])
    out3 = ins["out"].view(N, 2, per)
    r64, g64, _ = R.hybrid(F64, ac(), "eps", ins["t"], out3, ins["x0"], ins["noise"])
    r32, g32, _ = R.hybrid(F32, ac(), "eps", ins["t"], out3, ins["x0"], ins["noise"])
    e = rel(loss, r64)
    print(f"misaligned {which}: rel err {e.tolist()}")
    assert bool((e <= LOSS_RTOL).all())
    d3 = dout.cpu().view(N, 2, per)
    judge(f"hybrid misaligned {which}: prediction gradient", d3[:, 0], g32[:, 0], g64[:, 0], rows=N)
    judge_v(f"hybrid misaligned {which}", d3[:, 1], g32[:, 1], g64[:, 1], ins["t"])
    guard_ok(f"misaligned {which}", dbuf, *([sbuf] if sbuf is not None else []))
    if sbuf is not None:
        assert bool(shifted[:1].isnan().all())


def test_hybrid_wrapper_refusals():
    L, K = _lib()
    N, per = 3, 8
    ins = {k: dev(v) for k, v in lvar_inputs(N, per, "eps").items()}
    sa, s1 = (dev(v) for v in obj_tabs())
    coef = dev(lvar_table("eps"))
    dout, dbuf = guarded((N, 2 * per))
    g = torch.ones((), dtype=F32, device=DEV)
    o, x0, nz, t = ins["out"], ins["x0"], ins["noise"], ins["t"]

    def call(out=o, x0_=x0, noise=nz, t_=t, coef_=coef, sa_=sa, w=None, dloss=g, ptype="eps", lt="l2"):
        return K.hybrid_objective(ptype, lt, out, x0_, noise, t_, sa_, s1, coef_, w=w, dloss=dloss, dout=dout)

    bad = [
        ("out with C channels", lambda: call(out=ins["pred"])), ("out on the CPU", lambda: call(out=o.cpu())),
        ("out float64", lambda: call(out=o.double())), ("out strided", lambda: call(out=o.t().contiguous().t())),
        ("out rows", lambda: call(out=o[:2].contiguous())), ("x0 on the CPU", lambda: call(x0_=x0.cpu())),
        ("noise shape", lambda: call(noise=nz[:, :4].contiguous())), ("noise float64", lambda: call(noise=nz.double())),
        ("t int32", lambda: call(t_=t.int())), ("t length", lambda: call(t_=t[:2].contiguous())),
        ("no t", lambda: call(t_=None)), ("coef [T, 6]", lambda: call(coef_=coef[:, :6].contiguous())),
        ("coef strided", lambda: call(coef_=coef[::2])), ("coef on the CPU", lambda: call(coef_=coef.cpu())),
        ("w of another length", lambda: call(w=sa[:10].contiguous())), ("dloss float64", lambda: call(dloss=g.double())),
        ("no dloss", lambda: call(dloss=None)), ("prediction type", lambda: call(ptype="x0")),
        ("loss type", lambda: call(lt="l3")), ("v without tables", lambda: call(ptype="v", sa_=None)),
    ]
    for what, fn in bad:
        with pytest.raises(L.DMCError):
            fn()
        torch.cuda.synchronize()
        assert bool(dout.isnan().all()), what
    p = lambda v: v.data_ptr()   # noqa: E731
    ws = torch.empty(2 * L.OBJECTIVE_MAX_BLOCKS * N, dtype=F32, device=DEV)
    loss = torch.full((3,), float("nan"), device=DEV)

    def raw(outp=p(o), n=N, per_=per, T=1000, dl=p(g), ptype=0):
        return L.LIB.dmc_hybrid_objective(ptype, 1, outp, p(x0), p(nz), p(t), None, None, None, p(coef), T, n, per_,
                                          0.001, dl, p(loss), p(dout), p(ws), L.stream())

    for kw in (dict(outp=None), dict(n=0), dict(per_=0), dict(T=0), dict(dl=None), dict(ptype=1), dict(ptype=2)):
        assert raw(**kw) != 0 and b"hybrid_objective" in L.LIB.dmc_last_error(), kw
    torch.cuda.synchronize()
    assert bool(dout.isnan().all()) and bool(loss.isnan().all())
    guard_ok("refusals", dbuf)


# ------------------------------------------------------------------------------------------------------------
# dmc_ddpm_step_learned
# ------------------------------------------------------------------------------------------------------------
def step_tabs():
    tb = tables()
    return tuple(tb[k] for k in DDPM_TABS)


def run_step(K, ins, clip, z, out=None, x=None, res=None, eps=None, x0=None):
    sra, srm1, c1, c2, _ = (dev(v) for v in step_tabs())
    return K.ddpm_step_learned(dev(ins["x_t"]) if x is None else x, dev(ins["out"]) if out is None else out,
                               dev(ins["t"]), sra, srm1, c1, c2, dev(lvar_table("eps")), clip=clip, eps=eps, x0=x0,
                               z=z, res=res)


@pytest.mark.parametrize("N,per", SHAPES)
def test_ddpm_step_learned(N, per):
    L, K = _lib()
    ins = lvar_inputs(N, per, "eps")
    t, x, eps, v, z = ins["t"], ins["x_t"], ins["pred"], ins["v"], ins["z_next"]
    tabs = step_tabs()
    for clip in (False, True):
        what = f"ddpm_step_learned {N}x{per} clip {clip}"
        res, rbuf = guarded((N, per))
        run_step(K, ins, clip, None, res=res)
        mean = K.ddpm_step(dev(x), dev(eps), dev(t), *(dev(v_) for v_ in tabs), clip=clip).cpu()
        same_bits(f"{what}: z = None is dmc_ddpm_step", res, mean)
        res_z, zbuf = guarded((N, per))
        run_step(K, ins, clip, dev(z), res=res_z)
        judge(what, res_z, R.ddpm_step(F32, ac(), tabs[:4], t, x, eps, v, z, clip),
              R.ddpm_step(F64, ac(), tabs[:4], t, x, eps, v, z, clip), rows=N)
        again, abuf = guarded((N, per))
        run_step(K, ins, clip, dev(z), res=again)
        same_bits(f"{what}: second run", again, res_z.cpu())
        # rows with t = 0 add no noise, whatever z holds
        huge, hbuf = guarded((N, per))
        run_step(K, ins, clip, torch.full((N, per), 1e30, device=DEV), res=huge)
        same_bits(f"{what}: t = 0 rows ignore z", huge.cpu()[t == 0], mean[t == 0])
        # a given eps and x0 (the guided path) replace the output's prediction half
        x0_in = (torch.rand(N, per, generator=torch.Generator().manual_seed(5)) * 3 - 1.5)
        given, gbuf = guarded((N, per))
        run_step(K, ins, clip, dev(z), res=given, eps=dev(eps), x0=dev(x0_in))
        judge(f"{what}: given x0", given, R.ddpm_step(F32, ac(), tabs[:4], t, x, eps, v, z, clip, x0_in),
              R.ddpm_step(F64, ac(), tabs[:4], t, x, eps, v, z, clip, x0_in), rows=N)
        guard_ok(what, rbuf, zbuf, abuf, hbuf, gbuf)


@pytest.mark.parametrize("N,per", SHAPES)
def test_ddpm_step_learned_at_minus_one_is_the_fixed_step(N, per):
    """v = -1 everywhere is the posterior variance: on rows with t >= 1 the step is within criterion 2 of dmc_ddpm_step,
    dmc_ddpm_step's output being the fp32 yardstick: against the float64 restatement of the learned step, the learned
    kernel's error is at most 4 x the fixed kernel's + 1 ulp.

    The two are not the same number, and cannot be: lv_min is log pv[t] with beta = 1 - a_t / a_{t-1} recovered from the
    fp32 alphas_cumprod (diffusion/_vlb.py _schedule64), the fixed kernel's table is the samplers' fp32
    posterior_log_variance_clipped from the original betas. At t = 1 the recovered beta differs by a relative 5e-4 (an
    ulp of a_1 against beta_1 = 1.2e-4), elsewhere by an ulp of the logarithm. Measured on the MI355X, learned output
    against the float64 restatement of the FIXED step (the other reading of this check, which these definitions cannot
    meet): row error 1.0e-6 .. 2.2e-6 at t = 1 and 5.4e-8 at t = 999, against 4 x 1.2e-7 + 1.2e-7 and 4 x 9.5e-9 + 1.5e-8.
    The direct difference of the two kernels' outputs is printed."""
    L, K = _lib()
    ins = lvar_inputs(N, per, "eps", rot=1)
    t, x, eps, z = ins["t"], ins["x_t"], ins["pred"], ins["z_next"]
    live = t >= 1
    assert bool(live.any())      # rot = 1: the first sample has t = 999
    minus = torch.full_like(eps, -1.0)
    out = torch.cat([eps, minus], 1)
    res, rbuf = guarded((N, per))
    run_step(K, ins, True, dev(z), out=dev(out), res=res)
    tabs = step_tabs()
    fixed = K.ddpm_step(dev(x), dev(eps), dev(t), *(dev(v_) for v_ in tabs), clip=True, z=dev(z)).cpu()
    n = int(live.sum())
    got = res.cpu()[live]
    diff = (got.double() - fixed[live].double()).abs().amax(1)
    print(f"ddpm_step_learned v = -1 {N}x{per}: t {t[live].tolist()} max |learned - fixed| per row {diff.tolist()}")
    assert bool((diff <= 1e-3 * fixed[live].abs().amax(1)).all())
    ref64 = R.ddpm_step(F64, ac(), tabs[:4], t[live], x[live], eps[live], minus[live], z[live], True)
    judge(f"ddpm_step_learned v = -1 {N}x{per}", got, fixed[live], ref64, rows=n)
    guard_ok("v = -1", rbuf)


@pytest.mark.parametrize("which", ["x", "out", "z", "res", "v_half"])
def test_ddpm_step_learned_misaligned_base(which):
    L, K = _lib()
    N, per = 3, 66 if which == "v_half" else 64
    ins = lvar_inputs(N, per, "eps")
    ops = {"x": dev(ins["x_t"]), "out": dev(ins["out"]), "z": dev(ins["z_next"])}
    ops["res"], rbuf = guarded((N, per))
    sbuf = None
    if which != "v_half":
        shifted, sbuf = guarded((ops[which].numel() + 1,))
        view = shifted[1:].view(ops[which].shape)
        assert view.data_ptr() % 16 == 4
        if which != "res":
            view.copy_(ops[which])
        ops[which] = view
    run_step(K, ins, True, ops["z"], out=ops["out"], x=ops["x"], res=ops["res"])
    tabs = step_tabs()
    args = (ac(), tabs[:4], ins["t"], ins["x_t"], ins["pred"], ins["v"], ins["z_next"], True)
    judge(f"ddpm_step_learned misaligned {which}", ops["res"], R.ddpm_step(F32, *args), R.ddpm_step(F64, *args), rows=N)
    guard_ok(f"misaligned {which}", rbuf, *([sbuf] if sbuf is not None else []))


def test_ddpm_step_learned_wrapper_refusals():
    L, K = _lib()
    N, per = 3, 8
    ins = lvar_inputs(N, per, "eps")
    d = {k: dev(v) for k, v in ins.items()}
    res, rbuf = guarded((N, per))
    sra, srm1, c1, c2, _ = (dev(v) for v in step_tabs())
    coef = dev(lvar_table("eps"))

    def call(x=d["x_t"], out=d["out"], t=d["t"], sra_=sra, coef_=coef, z=d["z_next"], eps=None, x0=None):
        return K.ddpm_step_learned(x, out, t, sra_, srm1, c1, c2, coef_, eps=eps, x0=x0, z=z, res=res)

    bad = [
        ("x on the CPU", lambda: call(x=d["x_t"].cpu())), ("out with C channels", lambda: call(out=d["pred"])),
        ("out float64", lambda: call(out=d["out"].double())), ("out strided", lambda: call(out=d["out"].t().contiguous().t())),
        ("z shape", lambda: call(z=d["z_next"][:, :4].contiguous())), ("z float64", lambda: call(z=d["z_next"].double())),
        ("t int32", lambda: call(t=d["t"].int())), ("no t", lambda: call(t=None)),
        ("coef [T, 6]", lambda: call(coef_=coef[:, :6].contiguous())), ("coef on the CPU", lambda: call(coef_=coef.cpu())),
        ("table length", lambda: call(sra_=sra[:10].contiguous())), ("no table", lambda: call(sra_=None)),
        ("x0 without eps", lambda: call(x0=d["x0"])), ("eps strided", lambda: call(eps=d["pred"].t().contiguous().t())),
    ]
    for what, fn in bad:
        with pytest.raises(L.DMCError):
            fn()
        torch.cuda.synchronize()
        assert bool(res.isnan().all()), what
    p = lambda v: v.data_ptr()   # noqa: E731

    def raw(xp=p(d["x_t"]), n=N, per_=per, T=1000, vp=p(d["out"]) + 4 * per, ld=2 * per):
        return L.LIB.dmc_ddpm_step_learned(xp, p(d["out"]), ld, vp, ld, None, p(d["t"]), p(sra), p(srm1), p(c1), p(c2),
                                           p(coef), T, n, per_, 1, p(d["z_next"]), p(res), L.stream())

    for kw in (dict(xp=None), dict(n=0), dict(per_=0), dict(T=0), dict(vp=None), dict(ld=per - 1)):
        assert raw(**kw) != 0 and b"ddpm_step_learned" in L.LIB.dmc_last_error(), kw
    torch.cuda.synchronize()
    assert bool(res.isnan().all())
    guard_ok("refusals", rbuf)


# ------------------------------------------------------------------------------------------------------------
# dmc_vlb_step_learned
# ------------------------------------------------------------------------------------------------------------
def run_vlb(K, ins, ptype, clip, with_next=True, out=None, ops=None):
    N = ins["x0"].shape[0]
    tb = tables()
    o = {k: dev(ins[k]) for k in ("x0", "x_t", "out", "z_next")}
    o.update(ops or {})
    if out is not None:
        o["out"] = out
    rows, bufs = zip(*(guarded((N,)) for _ in range(4)))
    if "x_next" in o:
        xn, xb = o["x_next"], None
    else:
        xn, xb = guarded(tuple(ins["x0"].shape)) if with_next else (None, None)
    K.vlb_step_learned(o["x0"], o["x_t"], o["out"], dev(ins["t"]), dev(lvar_table(ptype)), clip=clip,
                       z_next=o["z_next"] if with_next else None, t_next=dev(ins["t_next"]) if with_next else None,
                       sa=dev(tb["sqrt_alphas_cumprod"]) if with_next else None,
                       s1=dev(tb["sqrt_one_minus_alphas_cumprod"]) if with_next else None, x_next=xn, rows=rows)
    return rows, bufs, xn, xb


def check_learned_rows(what, got, ins, ptype, clip, v=None):
    v = ins["v"] if v is None else v
    args = (ac(), ptype, ins["t"], ins["x0"], ins["x_t"], ins["pred"], v, clip)
    r64, pr64 = R.vlb_step(F64, *args)
    r32, _ = R.vlb_step(F32, *args)
    assert all(r.dtype == F64 for r in r64) and all(r.dtype == F32 for r in r32)
    e_vb, e_xs, e_eps, e_sq = (rel(g, r) for g, r in zip(got, r64))
    own = rel(r32[1], r64[1])
    bound_xs = torch.clamp(4 * own, min=LOSS_RTOL)
    print(f"{what}: rel err vb {e_vb.max():.2e} eps_mse {e_eps.max():.2e} xstart_mse {e_xs.max():.2e} "
          f"(fp32 restatement {own.max():.2e}) x0_sq {e_sq.max():.2e}; fp32 restatement vb {rel(r32[0], r64[0]).max():.2e}")
    for g in got:
        assert g.dtype == F32 and bool(g.isfinite().all()), what
    assert bool((e_vb <= LOSS_RTOL).all()), (what, "vb", e_vb.tolist())
    assert bool((e_eps <= LOSS_RTOL).all()), (what, "eps_mse", e_eps.tolist())
    assert bool((e_xs <= bound_xs).all()), (what, "xstart_mse", e_xs.tolist(), bound_xs.tolist())
    assert bool((e_sq <= 1e-6).all()), (what, "x0_sq", e_sq.tolist())
    return pr64


def vlb_ins(ins):
    return ins["x0"], ins["x_t"], ins["pred"], ins["t"], ins["z_next"], ins["t_next"]


@pytest.mark.parametrize("ptype", PTYPES)
@pytest.mark.parametrize("N,per", SHAPES)
def test_vlb_step_learned(N, per, ptype):
    L, K = _lib()
    for sigma in (0.05, 1.0):
        ins = lvar_inputs(N, per, ptype, sigma)
        for clip in (0, 1):
            what = f"vlb_step_learned {N}x{per} {ptype} sigma {sigma} clip {clip}"
            rows, bufs, xn, xb = run_vlb(K, ins, ptype, clip)
            pr64 = check_learned_rows(what, rows, ins, ptype, bool(clip))
            floor_check(what, pr64, ins["t"], per)
            check_next(what, K, vlb_ins(ins), xn)
            again, bufs2, xn2, xb2 = run_vlb(K, ins, ptype, clip)
            for a, b in zip(rows, again):
                same_bits(f"{what}: second run", b, a.cpu())
            assert torch.equal(xn.cpu().nan_to_num(nan=7.0), xn2.cpu().nan_to_num(nan=7.0))
            alone, bufs3, _, _ = run_vlb(K, ins, ptype, clip, with_next=False)
            for a, b in zip(rows, alone):
                same_bits(f"{what}: without x_next", b, a.cpu())
            guard_ok(what, *bufs, xb, *bufs2, xb2, *bufs3)


@pytest.mark.parametrize("ptype", PTYPES)
@pytest.mark.parametrize("N,per", SHAPES)
def test_vlb_step_learned_ends_are_the_fixed_variances(N, per, ptype):
    """v = -1 everywhere is 'fixed_small' on all four rows; v = +1 is 'fixed_large' on the rows with t >= 1."""
    from test_gpu_vlb import coef_table
    L, K = _lib()
    ins = lvar_inputs(N, per, ptype)
    x0, x_t, pred, t = (dev(ins[k]) for k in ("x0", "x_t", "pred", "t"))
    for vv, variance in ((-1.0, "fixed_small"), (1.0, "fixed_large")):
        out = torch.cat([ins["pred"], torch.full_like(ins["pred"], vv)], 1)
        rows, bufs, _, _ = run_vlb(K, ins, ptype, 1, with_next=False, out=dev(out))
        ref = K.vlb_step(x0, x_t, pred, t, dev(coef_table(ptype, variance)), clip=True)
        live = torch.ones_like(ins["t"], dtype=torch.bool) if vv < 0 else ins["t"] >= 1
        for name, g, r in zip(("vb", "xstart_mse", "eps_mse", "x0_sq"), rows, ref):
            g, r = g.cpu()[live].double(), r.cpu()[live].double()
            e = ((g - r).abs() / r.abs().clamp_min(1e-300))
            e = torch.where(r == 0, (g != 0).double(), e)
            print(f"v = {vv} against {variance} {N}x{per} {ptype}: {name} rel diff {e.tolist()}")
            assert bool((e <= LOSS_RTOL).all()), (vv, name, e.tolist())
        guard_ok("ends", *bufs)


@pytest.mark.parametrize("which", ["x0", "x_t", "out", "z_next", "x_next", "v_half"])
def test_vlb_step_learned_misaligned_base(which):
    L, K = _lib()
    N, per = 3, 66 if which == "v_half" else 64
    ins = lvar_inputs(N, per, "eps")
    ops, sbuf = {}, None
    xn, xb = guarded((N, per))
    ops["x_next"] = xn
    if which != "v_half":
        src = xn if which == "x_next" else dev(ins[which])
        shifted, sbuf = guarded((src.numel() + 1,))
        view = shifted[1:].view(src.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        if which != "x_next":
            view.copy_(src)
        ops[which] = view
    rows, bufs, xn, _ = run_vlb(K, ins, "eps", 1, ops=ops)
    check_learned_rows(f"vlb_step_learned misaligned {which}", rows, ins, "eps", True)
    check_next(f"misaligned {which}", K, vlb_ins(ins), xn)
    guard_ok(f"misaligned {which}", *bufs, xb, *([sbuf] if sbuf is not None else []))


def test_vlb_step_learned_wrapper_refusals():
    L, K = _lib()
    N, per = 3, 8
    ins = lvar_inputs(N, per, "eps")
    d = {k: dev(v) for k, v in ins.items()}
    coef = dev(lvar_table("eps"))
    tb = tables()
    sa, s1 = dev(tb["sqrt_alphas_cumprod"]), dev(tb["sqrt_one_minus_alphas_cumprod"])
    rows, bufs = zip(*(guarded((N,)) for _ in range(4)))
    xn, xb = guarded((N, per))
    nx = dict(z_next=d["z_next"], t_next=d["t_next"], sa=sa, s1=s1, x_next=xn)

    def call(x0=d["x0"], x_t=d["x_t"], out=d["out"], t=d["t"], coef_=coef, rows_=rows, **kw):
        return K.vlb_step_learned(x0, x_t, out, t, coef_, rows=rows_, **{**nx, **kw})

    bad = [
        ("x0 on the CPU", lambda: call(x0=d["x0"].cpu())), ("out with C channels", lambda: call(out=d["pred"])),
        ("out on the CPU", lambda: call(out=d["out"].cpu())), ("out float64", lambda: call(out=d["out"].double())),
        ("out strided", lambda: call(out=d["out"].t().contiguous().t())), ("x_t shape", lambda: call(x_t=d["x_t"][:, :4].contiguous())),
        ("t int32", lambda: call(t=d["t"].int())), ("no t", lambda: call(t=None)),
        ("t_next length", lambda: call(t_next=d["t_next"][:1].contiguous())),
        ("coef [T, 6]", lambda: call(coef_=coef[:, :6].contiguous())), ("coef float64", lambda: call(coef_=coef.double())),
        ("x_next without z_next", lambda: call(z_next=None)), ("x_next without tables", lambda: call(sa=None)),
        ("tables of another length", lambda: call(s1=s1[:10].contiguous())), ("three rows", lambda: call(rows_=rows[:3])),
        ("row length", lambda: call(rows_=(rows[0], rows[1], rows[2], rows[3][:2]))),
    ]
    for what, fn in bad:
        with pytest.raises(L.DMCError):
            fn()
        torch.cuda.synchronize()
        assert bool(xn.isnan().all()) and all(bool(r.isnan().all()) for r in rows), what
    p = lambda v: v.data_ptr()   # noqa: E731
    ws = torch.empty(4 * L.VLB_MAX_BLOCKS * N, dtype=F32, device=DEV)

    def raw(x0p=p(d["x0"]), n=N, per_=per, T=1000, vp=p(d["out"]) + 4 * per, ld=2 * per, znp=p(d["z_next"])):
        return L.LIB.dmc_vlb_step_learned(x0p, p(d["x_t"]), p(d["out"]), ld, vp, ld, p(d["t"]), p(coef), T, 1, znp,
                                          p(d["t_next"]), p(sa), p(s1), n, per_, p(xn), p(rows[0]), p(rows[1]),
                                          p(rows[2]), p(rows[3]), p(ws), L.stream())

    for kw in (dict(x0p=None), dict(n=0), dict(per_=0), dict(T=0), dict(vp=None), dict(ld=per - 1), dict(znp=None)):
        assert raw(**kw) != 0 and b"vlb_step_learned" in L.LIB.dmc_last_error(), kw
    torch.cuda.synchronize()
    assert bool(xn.isnan().all()) and all(bool(r.isnan().all()) for r in rows)
    guard_ok("refusals", *bufs, xb)
