"""The v-prediction / min-SNR objective on the GPU: dmc_objective and dmc_pred_convert against the restatements of
tests/objective_reference.py (dpred, eps and x0 bit for bit: criterion 1 of test_gpu_elem_kernels, the kernels have no
libm call and no fma; the loss against float64 within the project's fp32 loss bound, 1e-5 relative), and the three
samplers with prediction_type='v' on the Gaussian problem of test_gpu_dpm and under classifier-free guidance.
"""
import functools

import numpy as np
import pytest
import torch

import dpm_reference as DR
import objective_reference as R
from test_gpu_dpm import SHAPE, GaussianDenoiser, gauss_xT
from test_gpu_elem_kernels import DEV, F32, F64, dev, guard_ok, guarded, judge, rng, same_bits, tables

pytestmark = pytest.mark.gpu

GAMMA = 5.0
LOSS_RTOL = 1e-5        # an fp32 loss against float64
SHAPES = [(1, 1), (3, 7), (5, 192), (2, 3072), (4, 4100)]
KINDS = ("l1", "l2", "huber")
T_POOL = (0, 999, 50, 50, 500)      # first, last, a repeated value with SNR > 5 (t < 130), one with SNR < 5


def _lib():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


@functools.lru_cache(maxsize=None)
def obj_tables():
    """(sa, s1, {ptype: w}) as the diffusion objects upload them (fp32 CPU tensors; never modified)."""
    from diffusion_models_collection_amd.diffusion import _objective as O
    tb = tables()
    w = {p: torch.from_numpy(O.min_snr_weights(tb["alphas_cumprod"].numpy(), GAMMA, p)) for p in ("eps", "v")}
    snr = tb["alphas_cumprod"].double() / (1 - tb["alphas_cumprod"].double())
    assert snr[50] > GAMMA > snr[500]
    return tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"], w


def rots(N, per):
    return range(len(T_POOL)) if per < 100 else (0, 2)


@functools.lru_cache(maxsize=None)
def obj_inputs(N, per, rot, ptype):
    """pred, x0, noise, t. The first elements of pred sit at hand-made distances from the target (both sides of the
    huber threshold, zero, far away)."""
    from test_gpu_elem_kernels import loss_deltas
    sa, s1, _ = obj_tables()
    g = rng(1300 + N + per + rot)
    t = torch.tensor([T_POOL[(n + rot) % len(T_POOL)] for n in range(N)])
    x0 = torch.rand(N, per, generator=g) * 2 - 1
    noise = torch.randn(N, per, generator=g)
    pred = torch.randn(N, per, generator=g) * 1.5
    tg = R.target(F32, ptype, sa, s1, t, x0, noise)
    d = loss_deltas()
    k = min(N * per, d.numel())
    pred.view(-1)[:k] = tg.reshape(-1)[:k] + d[:k]
    return pred, x0, noise, t


def close_loss(what, got, ref64):
    got, ref = float(got), float(ref64)
    print(f"{what}: loss {got:.9g}, float64 {ref:.9g}, relative error {abs(got - ref) / abs(ref):.3e}")
    assert abs(got - ref) <= LOSS_RTOL * abs(ref), what


# ------------------------------------------------------------------------------------------------------------
# dmc_objective
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,per", SHAPES)
@pytest.mark.parametrize("ptype", ["eps", "v"])
def test_objective(N, per, ptype):
    """(3, 7): per % 4 != 0, the element-wise path with misaligned rows; (5, 192) and (2, 3072): the 16-byte path, one
    and three blocks per sample; (4, 4100): 16-byte path whose last block is ragged. dpred bitwise under dloss = 1 and
    2.5, written over NaN with the guard intact; the loss within 1e-5 of float64; a second run and the forward-only
    call give the same loss bits; eps without weights gives dmc_loss_bwd's bits."""
    L, K = _lib()
    sa, s1, wt = obj_tables()
    sad, s1d = dev(sa), dev(s1)
    for rot in rots(N, per):
        pred, x0, noise, t = obj_inputs(N, per, rot, ptype)
        pd, xd, nd, td = (dev(v) for v in (pred, x0, noise, t))
        for kind in KINDS:
            for w in (None, wt[ptype]):
                wd = dev(w)
                what = f"objective {ptype} {kind} w={'table' if w is not None else 'none'} rot={rot}"
                ref64 = R.loss(F64, ptype, kind, pred, x0, noise, t, sa, s1, w)
                for dl in (1.0, 2.5):
                    dloss = torch.tensor(dl, device=DEV)
                    out, buf = guarded((N, per))
                    loss, dp = K.objective(ptype, kind, pd, xd, nd, td, sad, s1d, wd, dloss=dloss, out=out)
                    assert loss.shape == () and loss.dtype == F32 and dp is out
                    guard_ok(what, buf)
                    same_bits(f"{what} dloss={dl}: dpred", dp, R.grad(ptype, kind, pred, x0, noise, t, sa, s1, w, dl))
                    if dl == 1.0:
                        first = loss.clone()
                    assert torch.equal(loss, first), what      # dloss does not touch the loss; a second run is equal
                close_loss(what, first, ref64)
                fwd, none = K.objective(ptype, kind, pd, xd, nd, td, sad, s1d, wd, grad=False)
                assert none is None and torch.equal(fwd, first), what
                if ptype == "eps" and w is None:
                    dloss = torch.tensor(2.5, device=DEV)
                    _, dp = K.objective(ptype, kind, pd, None, nd, td, sad, s1d, None, dloss=dloss)
                    assert torch.equal(dp, K.loss_bwd(kind, pd, nd, dloss)), what
    # the restatement itself: the fp32 gradient agrees with autograd on the float64 loss
    pred, x0, noise, t = obj_inputs(N, per, 0, ptype)
    for kind in KINDS:
        g32 = R.grad(ptype, kind, pred, x0, noise, t, sa, s1, wt[ptype], 1.0)
        g64 = R.grad64(ptype, kind, pred, x0, noise, t, sa, s1, wt[ptype])
        if kind == "l2":
            assert float((g32.double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
        else:       # sign / threshold functions: equal except where fp32 and float64 fall on different sides
            assert float(((g32.double() - g64).abs() > 1e-6 * g64.abs().max()).double().mean()) < 0.01 + 2.0 / (N * per)


def test_objective_clamps_timesteps():
    """t outside [0, T) reads the nearest table entry, never past the table."""
    L, K = _lib()
    sa, s1, wt = obj_tables()
    pred, x0, noise, _ = obj_inputs(5, 192, 0, "v")
    t_bad = torch.tensor([-7, 1000, 1 << 40, 999, 0])
    t_ok = t_bad.clamp(0, 999)
    args = [dev(v) for v in (pred, x0, noise)]
    one = torch.ones((), device=DEV)
    la, da = K.objective("v", "l2", *args, dev(t_bad), dev(sa), dev(s1), dev(wt["v"]), dloss=one)
    lb, db = K.objective("v", "l2", *args, dev(t_ok), dev(sa), dev(s1), dev(wt["v"]), dloss=one)
    assert torch.equal(la, lb) and torch.equal(da, db)


# ------------------------------------------------------------------------------------------------------------
# dmc_pred_convert
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_inputs(N, per, reps, rot):
    g = rng(1700 + N + per + reps + rot)
    t = torch.tensor([T_POOL[(n + rot) % len(T_POOL)] for n in range(N)])
    x = torch.randn(N, per, generator=g)
    pred = torch.randn(reps * N, per, generator=g)
    return x, pred, t


@pytest.mark.parametrize("N,per", SHAPES)
@pytest.mark.parametrize("reps", [1, 2])
def test_pred_convert(N, per, reps):
    L, K = _lib()
    sa, s1, _ = obj_tables()
    for rot in rots(N, per):
        x, pred, t = conv_inputs(N, per, reps, rot)
        ref_eps, ref_x0 = R.convert(F32, x, t, sa, s1, pred, reps)
        for want_x0 in (True, False):
            eps, eb = guarded((reps * N, per))
            x0, xb = guarded((reps * N, per))
            r = K.pred_convert("v", dev(x), dev(t), dev(sa), dev(s1), dev(pred), out=(eps, x0 if want_x0 else None))
            what = f"pred_convert reps={reps} rot={rot} x0={want_x0}"
            assert r[0] is eps and (r[1] is x0) == want_x0
            same_bits(what + " eps", eps, ref_eps)
            if want_x0:
                same_bits(what + " x0", x0, ref_x0)
            else:
                assert bool(x0.isnan().all())
            guard_ok(what, eb, xb)
        # allocating form
        eps, x0 = K.pred_convert("v", dev(x), dev(t), dev(sa), dev(s1), dev(pred))
        same_bits("pred_convert alloc eps", eps, ref_eps)
        same_bits("pred_convert alloc x0", x0, ref_x0)
        assert K.pred_convert("v", dev(x), dev(t), dev(sa), dev(s1), dev(pred), want_x0=False)[1] is None


@pytest.mark.parametrize("N,per", [(5, 192), (4, 4100)])
def test_pred_convert_round_trip(N, per):
    """v built in float64 from random (x0, eps) and rounded once; x_t likewise: the kernel returns both under
    criterion 2 (ref64: the conversion in float64 from the same fp32 inputs; ref32: its fp32 restatement), and the
    float64 conversion itself returns (eps, x0) to the rounding of its inputs."""
    L, K = _lib()
    sa, s1, _ = obj_tables()
    g = rng(1900 + N)
    t = torch.tensor([T_POOL[n % len(T_POOL)] for n in range(N)])
    x0 = torch.rand(N, per, generator=g) * 2 - 1
    eps = torch.randn(N, per, generator=g)
    v = R.v_of(F64, sa, s1, t, x0, eps).float()
    xt = (sa.double()[t].view(N, 1) * x0.double() + s1.double()[t].view(N, 1) * eps.double()).float()
    e64, x64 = R.convert(F64, xt, t, sa, s1, v)
    # sa^2 + s1^2 = 1 to the tables' rounding, and x_t, v carry one rounding each
    assert float((e64 - eps.double()).abs().max()) < 1e-6 and float((x64 - x0.double()).abs().max()) < 1e-6
    e32, x32 = R.convert(F32, xt, t, sa, s1, v)
    ge, gx = K.pred_convert("v", dev(xt), dev(t), dev(sa), dev(s1), dev(v))
    judge("round trip eps", ge, e32, e64, rows=N)
    judge("round trip x0", gx, x32, x64, rows=N)


# ------------------------------------------------------------------------------------------------------------
# misaligned bases and refusals
# ------------------------------------------------------------------------------------------------------------
def _shift(t):
    """A contiguous copy of t that starts 4 bytes into a 16-byte aligned buffer."""
    buf, whole = guarded((t.numel() + 1,))
    view = buf[1:].view(t.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    view.copy_(t)
    return view, whole


@pytest.mark.parametrize("which", ["pred", "x0", "noise", "dpred"])
def test_objective_misaligned_base(which):
    """per % 4 == 0 but one operand starts 4 bytes into its buffer: the element-wise path, the same dpred bits; the
    loss keeps the float64 bound (its partial sums group differently)."""
    L, K = _lib()
    N, per = 3, 64
    sa, s1, wt = obj_tables()
    pred, x0, noise, t = obj_inputs(N, per, 0, "v")
    ops = {"pred": dev(pred), "x0": dev(x0), "noise": dev(noise), "dpred": torch.empty(N, per, device=DEV)}
    ops[which], whole = _shift(ops[which])
    if which == "dpred":
        ops[which].fill_(float("nan"))
    one = torch.ones((), device=DEV)
    loss, dp = K.objective("v", "huber", ops["pred"], ops["x0"], ops["noise"], dev(t), dev(sa), dev(s1), dev(wt["v"]),
                           dloss=one, out=ops["dpred"])
    assert dp is ops["dpred"]
    same_bits(f"misaligned {which}: dpred", dp, R.grad("v", "huber", pred, x0, noise, t, sa, s1, wt["v"], 1.0))
    close_loss(f"misaligned {which}", loss, R.loss(F64, "v", "huber", pred, x0, noise, t, sa, s1, wt["v"]))
    guard_ok(f"misaligned {which}", whole)
    assert bool(whole[:1].isnan().all())


@pytest.mark.parametrize("which", ["x", "pred", "eps_out", "x0_out"])
def test_pred_convert_misaligned_base(which):
    L, K = _lib()
    N, per, reps = 3, 64, 2
    sa, s1, _ = obj_tables()
    x, pred, t = conv_inputs(N, per, reps, 0)
    ref_eps, ref_x0 = R.convert(F32, x, t, sa, s1, pred, reps)
    ops = {"x": dev(x), "pred": dev(pred)}
    ops["eps_out"], eb = guarded((reps * N, per))
    ops["x0_out"], xb = guarded((reps * N, per))
    if which in ("x", "pred"):
        ops[which], whole = _shift(ops[which])
    else:
        buf, whole = guarded((reps * N * per + 1,))
        ops[which] = buf[1:].view(reps * N, per)
        assert ops[which].data_ptr() % 16 == 4
    K.pred_convert("v", ops["x"], dev(t), dev(sa), dev(s1), ops["pred"], out=(ops["eps_out"], ops["x0_out"]))
    same_bits(f"misaligned {which}: eps", ops["eps_out"], ref_eps)
    same_bits(f"misaligned {which}: x0", ops["x0_out"], ref_x0)
    guard_ok(f"misaligned {which}", eb, xb, whole)
    assert bool(whole[:1].isnan().all())                    # the element before the view is untouched


def test_wrapper_refusals():
    """A wrong operand is a DMCError before anything is launched: NaN-filled outputs stay untouched."""
    L, K = _lib()
    N, per = 3, 8
    sa, s1, wt = (dev(v) if not isinstance(v, dict) else dev(v["v"]) for v in obj_tables())
    pred, x0, noise, t = (dev(v) for v in obj_inputs(N, per, 0, "v"))
    one = torch.ones((), device=DEV)
    eps_o, eb = guarded((N, per))
    x0_o, xb = guarded((N, per))
    out = (eps_o, x0_o)
    bad = [
        ("x0 shape", lambda: K.objective("v", "l2", pred, x0[:, :4].contiguous(), noise, t, sa, s1, wt, dloss=one)),
        ("noise rows", lambda: K.objective("v", "l2", pred, x0, noise[:2].contiguous(), t, sa, s1, wt, dloss=one)),
        ("t length", lambda: K.objective("v", "l2", pred, x0, noise, t[:2].contiguous(), sa, s1, wt, dloss=one)),
        ("t int32", lambda: K.objective("v", "l2", pred, x0, noise, t.int(), sa, s1, wt, dloss=one)),
        ("t on the CPU", lambda: K.objective("v", "l2", pred, x0, noise, t.cpu(), sa, s1, wt, dloss=one)),
        ("pred on the CPU", lambda: K.objective("v", "l2", pred.cpu(), x0, noise, t, sa, s1, wt, dloss=one)),
        ("noise on the CPU", lambda: K.objective("v", "l2", pred, x0, noise.cpu(), t, sa, s1, wt, dloss=one)),
        ("v without x0", lambda: K.objective("v", "l2", pred, None, noise, t, sa, s1, wt, dloss=one)),
        ("w length", lambda: K.objective("v", "l2", pred, x0, noise, t, sa, s1, wt[:10].contiguous(), dloss=one)),
        ("w float64", lambda: K.objective("v", "l2", pred, x0, noise, t, sa, s1, wt.double(), dloss=one)),
        ("no dloss", lambda: K.objective("v", "l2", pred, x0, noise, t, sa, s1, wt)),
        ("prediction type", lambda: K.objective("x0", "l2", pred, x0, noise, t, sa, s1, wt, dloss=one)),
        ("loss type", lambda: K.objective("v", "l3", pred, x0, noise, t, sa, s1, wt, dloss=one)),
        ("convert: eps", lambda: K.pred_convert("eps", noise, t, sa, s1, pred, out=out)),
        ("convert: pred shape", lambda: K.pred_convert("v", noise, t, sa, s1, pred[:, :4].contiguous(), out=out)),
        ("convert: pred rows", lambda: K.pred_convert("v", noise, t, sa, s1, pred[:2].contiguous(), out=out)),
        ("convert: out shape", lambda: K.pred_convert("v", noise, t, sa, s1, torch.cat([pred, pred]), out=out)),
        ("convert: t length", lambda: K.pred_convert("v", noise, t[:2].contiguous(), sa, s1, pred, out=out)),
        ("convert: t int32", lambda: K.pred_convert("v", noise, t.int(), sa, s1, pred, out=out)),
        ("convert: x on the CPU", lambda: K.pred_convert("v", noise.cpu(), t, sa, s1, pred, out=out)),
        ("convert: pred on the CPU", lambda: K.pred_convert("v", noise, t, sa, s1, pred.cpu(), out=out)),
        ("convert: table on the CPU", lambda: K.pred_convert("v", noise, t, sa.cpu(), s1, pred, out=out)),
    ]
    for what, call in bad:
        with pytest.raises(L.DMCError):
            call()
        torch.cuda.synchronize()
        assert bool(eps_o.isnan().all()) and bool(x0_o.isnan().all()), what
    guard_ok("refusals", eb, xb)
    # the C entry points refuse by themselves
    ws = torch.empty(64 * N, device=DEV)
    loss = torch.full((), float("nan"), device=DEV)
    p = lambda v: None if v is None else v.data_ptr()   # noqa: E731

    def objective_rc(ptype, kind, x0_, T, n, per_, dpred, dloss):
        return L.LIB.dmc_objective(ptype, kind, p(pred), p(x0_), p(noise), p(t), p(sa), p(s1), p(wt), T, n, per_,
                                   p(dloss), p(loss), p(dpred), p(ws), L.stream())

    assert objective_rc(2, 1, x0, 1000, N, per, None, None) != 0 and b"objective" in L.LIB.dmc_last_error()
    assert objective_rc(1, 3, x0, 1000, N, per, None, None) != 0
    assert objective_rc(1, 1, None, 1000, N, per, None, None) != 0
    assert objective_rc(1, 1, x0, 0, N, per, None, None) != 0
    assert objective_rc(1, 1, x0, 1000, 0, per, None, None) != 0
    assert objective_rc(1, 1, x0, 1000, N, 0, None, None) != 0
    assert objective_rc(1, 1, x0, 1000, N, per, eps_o, None) != 0       # a gradient without dloss
    rc = L.LIB.dmc_pred_convert(0, p(noise), p(t), p(sa), p(s1), 1000, p(pred), 1, N, per, p(eps_o), p(x0_o),
                                L.stream())
    assert rc != 0 and b"pred_convert" in L.LIB.dmc_last_error()
    assert L.LIB.dmc_pred_convert(1, p(noise), p(t), p(sa), p(s1), 1000, p(pred), 0, N, per, p(eps_o), p(x0_o),
                                  L.stream()) != 0
    torch.cuda.synchronize()
    assert bool(eps_o.isnan().all()) and bool(x0_o.isnan().all()) and bool(loss.isnan())


# ------------------------------------------------------------------------------------------------------------
# samplers on the Gaussian problem
# ------------------------------------------------------------------------------------------------------------
class GaussianVDenoiser(GaussianDenoiser):
    """v of the exact denoiser, the op sequence of objective_reference.gaussian_v on the device."""

    def __call__(self, x, t, y=None):
        pick = lambda tab: tab[t].view(-1, 1, 1, 1)   # noqa: E731
        return R.gaussian_v(x, pick(self.a), pick(self.sa), pick(self.s1), self.s2)


def _sampler(kind, ptype, steps=None):
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver
    if kind == "ddim":
        return DDIM(1000, steps or 50, device=DEV, prediction_type=ptype)
    if kind == "ddpm":
        return DDPM(steps or 1000, device=DEV, prediction_type=ptype)
    return DPMSolver(1000, steps or 20, solver_order=int(kind[-1]), device=DEV, prediction_type=ptype)


def _full(v):
    return torch.full((SHAPE[0],), int(v), dtype=torch.long, device=DEV)


def _ddim_run(smp, model, xT):
    ts = smp.inference_timesteps.tolist() + [-1]
    x = dev(xT)
    for i in range(len(ts) - 1):
        x = smp.p_sample(model, x, _full(ts[i]), _full(ts[i + 1]), clip_denoised=False)
    return x


DDPM_STEPS = 20


@functools.lru_cache(maxsize=None)
def ddpm_noise():
    return torch.randn((DDPM_STEPS,) + SHAPE, generator=rng(78))


def _run(kind, smp, model, xT):
    """The sampler's own entry points, no clipping: DDIM p_sample over its 50 timesteps, DDPM p_sample over the first
    20 with injected noise, DPMSolver.sample."""
    if kind == "ddim":
        return _ddim_run(smp, model, xT)
    if kind == "ddpm":
        x, z = dev(xT), dev(ddpm_noise())
        for i in range(DDPM_STEPS):
            x = smp.p_sample(model, x, _full(999 - i), clip_denoised=False, noise=z[i])
        return x
    return smp.sample(model, SHAPE, x_T=dev(xT), clip_denoised=False)


def _ref(kind, dt, smp, s, xT):
    tb = tables()
    ac = tb["alphas_cumprod"].numpy()
    sa, s1 = smp.sqrt_alphas_cumprod.cpu().numpy(), smp.sqrt_one_minus_alphas_cumprod.cpu().numpy()
    assert np.array_equal(smp.alphas_cumprod.cpu().numpy(), ac)
    if kind == "ddpm":
        ts = np.arange(999, 999 - DDPM_STEPS, -1)
        pair = R.gaussian_pair_fn(dt, ac, sa, s1, ts, s)
        return R.ddpm_loop(dt, xT.numpy(), pair, smp.posterior_mean_coef1.cpu().numpy(),
                           smp.posterior_mean_coef2.cpu().numpy(), smp.posterior_log_variance_clipped.cpu().numpy(),
                           ts, ddpm_noise().numpy())
    ts = smp.inference_timesteps.cpu().numpy()
    pair = R.gaussian_pair_fn(dt, ac, sa, s1, ts, s)
    if kind == "ddim":
        return R.ddim_loop(dt, xT.numpy(), pair, ac, ts)
    return R.solver_loop(dt, xT.numpy(), pair, smp.step_coefficients.cpu().numpy())


@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpm1", "dpm2"])
def test_v_sampler_matches_float64_loop(kind, s):
    """A prediction_type='v' sampler with the v-denoiser against the float64 loop of the same sampler in (eps, x0)
    form over the sampler's own tables; the fp32 loop calibrates (criterion 2, per sample)."""
    smp = _sampler(kind, "v")
    xT = gauss_xT()
    got = _run(kind, smp, GaussianVDenoiser(s), xT)
    assert got.shape == SHAPE and got.dtype == F32
    ref32 = _ref(kind, np.float32, smp, s, xT)
    ref64 = _ref(kind, np.float64, smp, s, xT)
    assert ref32.dtype == np.float32 and ref64.dtype == np.float64
    judge(f"v sampler {kind} s={s}", got, torch.from_numpy(ref32), torch.from_numpy(ref64), rows=SHAPE[0])


@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("kind", ["ddim", "dpm2"])
def test_v_sampler_error_equals_eps_sampler_error(kind, s):
    """DDIM-50 and DPMSolver-20: per element, the relative error against the closed-form answer is within 1 % of the
    eps sampler's with the eps denoiser. (The discretisation error is 1e-3 .. 8e-2 here; on the CPU the fp32 loops of
    the two parameterisations differ by about 1e-6.)"""
    xT = gauss_xT()
    exact = torch.from_numpy(DR.gaussian_exact(xT.numpy(), tables()["alphas_cumprod"].numpy(), 1000, s))

    def rel_err(out):
        return ((out.cpu().double() - exact).abs() / exact.abs()).flatten()

    ev = rel_err(_run(kind, _sampler(kind, "v"), GaussianVDenoiser(s), xT))
    ee = rel_err(_run(kind, _sampler(kind, "eps"), GaussianDenoiser(s), xT))
    worst = float(((ev - ee).abs() / ee).max())
    print(f"{kind} s={s}: relative error eps [{ee.min():.4e}, {ee.max():.4e}], v [{ev.min():.4e}, {ev.max():.4e}], "
          f"worst |v - eps| / eps {worst:.3e}")
    assert float(ee.min()) > 0
    assert bool(((ev - ee).abs() <= 0.01 * ee).all())


# ------------------------------------------------------------------------------------------------------------
# classifier-free guidance
# ------------------------------------------------------------------------------------------------------------
def v_model(x, t, y):
    """A conditional callable 'network': any fixed function of (x, t, y) serves."""
    c = 1.0 + 0.125 * y.view(-1, 1, 1, 1).float()
    return torch.tanh(x * c) + 0.001 * t.view(-1, 1, 1, 1).float()


class ConvertedEps:
    """v_model's output converted to eps op by op in torch on the device (objective_reference.convert), as an eps
    model for the eps-mode sampler."""

    def __init__(self, smp):
        self.sa, self.s1 = smp.sqrt_alphas_cumprod, smp.sqrt_one_minus_alphas_cumprod

    def __call__(self, x, t, y):
        return R.convert(F32, x, t, self.sa, self.s1, v_model(x, t, y))[0]


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpm2"])
def test_cfg_v_equals_eps_of_converted_model(kind):
    """sample_with_cfg, 3 steps: guidance is affine in the outputs with coefficients summing to 1, so a v sampler (one
    conversion of the 2B-row output, then dmc_cfg_x0 unchanged) equals the eps sampler fed the converted model, bit
    for bit."""
    shape = (4, 3, 8, 8)
    g = rng(81)
    xT = dev(torch.randn(shape, generator=g))
    y = torch.tensor([1, 2, 7, 5], device=DEV)
    kw = {}
    if kind != "dpm2":
        kw["noise"] = dev(torch.randn((3,) + shape, generator=g))      # DDPM: T = 3; DDIM: 3 steps, eta > 0
    sv, se = _sampler(kind, "v", 3), _sampler(kind, "eps", 3)
    if kind == "ddim":
        sv.eta = se.eta = 0.5
    got = sv.sample_with_cfg(v_model, shape, y, x_T=xT, **kw)
    ref = se.sample_with_cfg(ConvertedEps(se), shape, y, x_T=xT, **kw)
    assert got.shape == shape and bool(got.isfinite().all())
    assert torch.equal(got, ref)
    # and v_model's output is not already eps: the plain eps sampler on it differs
    assert not torch.equal(got, se.sample_with_cfg(v_model, shape, y, x_T=xT, **kw))
