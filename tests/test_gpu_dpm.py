"""DPM-Solver++ on the GPU: dmc_dpm_step bit for bit against an fp32 op-by-op restatement (criterion 1 of
test_gpu_elem_kernels: the kernel has no libm call and no fma), the sampler against the float64 numpy loop of
tests/dpm_reference.py (criterion 2), the accuracy conditions on the device, and graph replay against the eager loop.
"""
import functools

import numpy as np
import pytest
import torch

import dpm_reference as R
from test_gpu_elem_kernels import DEV, F32, F64, NAN, dev, guard_ok, guarded, judge, rng, same_bits, sqrt_cr, tables

pytestmark = pytest.mark.gpu


def _lib():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


# ------------------------------------------------------------------------------------------------------------
# the step kernel
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coef_table(order=2):
    """[20, 5] fp32 table of the 20-step log-SNR grid, from the float64 restatement rounded once (never modified).
    Order 2: row 0 first (c1 = 0), rows 1..17 order 2, row 18 lower-order final (c1 = 0), row 19 last."""
    ac = tables()["alphas_cumprod"].numpy()
    ts = R.ref_timesteps(ac, 1000, 20)
    assert len(ts) == 20
    c = torch.from_numpy(R.ref_coefficients(ac, ts, order, True).astype(np.float32))
    if order == 2:
        assert bool((c[[0, 18, 19], 4] == 0).all()) and bool((c[1:18, 4] != 0).all())
    else:
        assert bool((c[:, 4] == 0).all())
    return c


ROWS = (0, 7, 18, 19, 1, 17, 12)      # first, middle order 2, lower-order final, last, then more order-2 rows


def dpm_ref(dt, coef, step, x, eps, x0_in, x0_prev, clip):
    """dpm_step_kernel's ops one at a time in precision dt -> (out, x0_out). A row with c1 == 0 takes no history
    term, whatever x0_prev holds."""
    N = x.shape[0]
    sa, s1, cx, c0, c1 = (coef.to(dt)[step][:, k].view(N, 1) for k in range(5))
    xx = x.to(dt)
    if x0_in is None:
        num = xx - s1 * eps.to(dt)
        x0 = num / sa
    else:
        x0 = x0_in.to(dt)
    if clip:
        x0 = x0.clamp(-1, 1)
    out = cx * xx + c0 * x0
    if x0_prev is not None:
        out = torch.where(c1 != 0, out + c1 * x0_prev.to(dt), out)
    else:
        assert bool((c1 == 0).all())
    return out, x0


@functools.lru_cache(maxsize=None)
def dpm_inputs(N, per, rot=0):
    g = rng(900 + N + per)
    step = torch.tensor([ROWS[(n + rot) % len(ROWS)] for n in range(N)])
    x, eps, x0_prev = (torch.randn(N, per, generator=g) for _ in range(3))
    x0_in = torch.rand(N, per, generator=g) * 3 - 1.5          # both sides of the clamp
    return x, eps, x0_in, x0_prev, step


DPM_SHAPES = [(1, 1), (3, 3072), (5, 7), (300, 48)]


@pytest.mark.parametrize("N,per", DPM_SHAPES)
def test_dpm_step(N, per):
    """(5, 7): per % 4 != 0, the scalar path with misaligned rows; (3, 3072) and (300, 48): the 16-byte path, the
    second with more samples than a block has threads; (1, 1) is run once per row kind. Both outputs bitwise,
    written over NaN, guards intact."""
    L, K = _lib()
    coef = coef_table()
    cd = dev(coef)
    for rot in range(4 if N < 4 else 1):
        x, eps, x0_in, x0_prev, step = dpm_inputs(N, per, rot)
        if N >= 4:
            assert set(step.tolist()) >= {0, 7, 18, 19}
        xd, ed, x0d, pd, sd = (dev(v) for v in (x, eps, x0_in, x0_prev, step))
        for clip in (True, False):
            for use_x0 in (False, True):
                ref_out, ref_x0 = dpm_ref(F32, coef, step, x, None if use_x0 else eps, x0_in if use_x0 else None,
                                          x0_prev, clip)
                out, buf = guarded((N, per))
                x0o, buf0 = guarded((N, per))
                r = K.dpm_step(xd, None if use_x0 else ed, sd, cd, clip=clip, x0=x0d if use_x0 else None,
                               x0_prev=pd, out=out, x0_out=x0o)
                assert r[0] is out and r[1] is x0o
                what = f"dpm_step rot={rot} clip={clip} x0_in={use_x0}"
                same_bits(what + " out", out, ref_out)
                same_bits(what + " x0_out", x0o, ref_x0)
                guard_ok(what, buf, buf0)
    # the restatement itself: eps -> x0 is DDIM's, and the float64 version agrees to rounding
    x, eps, x0_in, x0_prev, step = dpm_inputs(N, per, 0)
    o32, _ = dpm_ref(F32, coef, step, x, eps, None, x0_prev, False)
    o64, _ = dpm_ref(F64, coef, step, x, eps, None, x0_prev, False)
    assert float((o32.double() - o64).abs().max()) < 1e-3


def test_dpm_step_never_reads_history_on_first_order_rows():
    """NaN in x0_prev for every sample whose row has c1 == 0: finite outputs with the right bits. Then no history
    buffer at all with an all-order-1 table."""
    L, K = _lib()
    for N, per in ((5, 7), (300, 48)):
        coef = coef_table()
        x, eps, x0_in, x0_prev, step = dpm_inputs(N, per)
        poisoned = x0_prev.clone()
        first_order = coef[step][:, 4] == 0
        assert 0 < int(first_order.sum()) < N
        poisoned[first_order] = NAN
        ref_out, ref_x0 = dpm_ref(F32, coef, step, x, eps, None, x0_prev, True)
        assert bool(ref_out.isfinite().all())
        out, buf = guarded((N, per))
        x0o, buf0 = guarded((N, per))
        K.dpm_step(dev(x), dev(eps), dev(step), dev(coef), clip=True, x0_prev=dev(poisoned), out=out, x0_out=x0o)
        assert bool(out.isfinite().all())
        same_bits("poisoned history: out", out, ref_out)
        same_bits("poisoned history: x0_out", x0o, ref_x0)
        guard_ok("poisoned history", buf, buf0)

        c1 = coef_table(1)
        ref_out, ref_x0 = dpm_ref(F32, c1, step, x, eps, None, None, True)
        out, buf = guarded((N, per))
        x0o, buf0 = guarded((N, per))
        K.dpm_step(dev(x), dev(eps), dev(step), dev(c1), clip=True, x0_prev=None, out=out, x0_out=x0o)
        same_bits("no history buffer: out", out, ref_out)
        same_bits("no history buffer: x0_out", x0o, ref_x0)
        guard_ok("no history buffer", buf, buf0)


@pytest.mark.parametrize("N,per", [(5, 7), (3, 3072)])
def test_dpm_step_history_written_in_place(N, per):
    """x0_out is the x0_prev tensor itself: the same bits as with separate buffers."""
    L, K = _lib()
    coef = coef_table()
    x, eps, x0_in, x0_prev, step = dpm_inputs(N, per)
    ref_out, ref_x0 = dpm_ref(F32, coef, step, x, eps, None, x0_prev, False)
    hist, hbuf = guarded((N, per))
    hist.copy_(x0_prev)
    out, buf = guarded((N, per))
    K.dpm_step(dev(x), dev(eps), dev(step), dev(coef), clip=False, x0_prev=hist, out=out, x0_out=hist)
    same_bits("aliased: out", out, ref_out)
    same_bits("aliased: x0_out", hist, ref_x0)
    guard_ok("aliased", buf, hbuf)


@pytest.mark.parametrize("which", ["x", "eps", "x0_prev", "out", "x0_out"])
def test_dpm_step_misaligned_base(which):
    """per % 4 == 0 but one operand starts 4 bytes into its buffer: the element-wise path, the same bits."""
    L, K = _lib()
    N, per = 3, 64
    coef = coef_table()
    x, eps, x0_in, x0_prev, step = dpm_inputs(N, per)
    ref_out, ref_x0 = dpm_ref(F32, coef, step, x, eps, None, x0_prev, True)
    ops = {"x": dev(x), "eps": dev(eps), "x0_prev": dev(x0_prev)}
    ops["out"], ob = guarded((N, per))
    ops["x0_out"], xb = guarded((N, per))
    shifted, sbuf = guarded((N * per + 1,))
    view = shifted[1:].view(N, per)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    if which in ("x", "eps", "x0_prev"):
        view.copy_(ops[which])
    ops[which] = view
    K.dpm_step(ops["x"], ops["eps"], dev(step), dev(coef), clip=True, x0_prev=ops["x0_prev"], out=ops["out"],
               x0_out=ops["x0_out"])
    same_bits(f"misaligned {which}: out", ops["out"], ref_out)
    same_bits(f"misaligned {which}: x0_out", ops["x0_out"], ref_x0)
    guard_ok(f"misaligned {which}", ob, xb, sbuf)
    assert bool(shifted[:1].isnan().all())                  # the element before the view is untouched


def test_dpm_step_wrapper_refusals():
    """A wrong operand is a DMCError before anything is launched: the NaN-filled outputs stay untouched."""
    L, K = _lib()
    N, per = 3, 8
    coef = dev(coef_table())
    x, eps, x0_in, x0_prev, step = (dev(v) for v in dpm_inputs(N, per))
    out, buf = guarded((N, per))
    x0o, buf0 = guarded((N, per))
    ok = dict(clip=True, x0_prev=x0_prev, out=out, x0_out=x0o)
    bad = [
        ("eps shape", lambda: K.dpm_step(x, eps[:, :4].contiguous(), step, coef, **ok)),
        ("x0_prev shape", lambda: K.dpm_step(x, eps, step, coef, **{**ok, "x0_prev": x0_prev[:2].contiguous()})),
        ("x0 on the CPU", lambda: K.dpm_step(x, None, step, coef, x0=x0_in.cpu(), **ok)),
        ("index on the CPU", lambda: K.dpm_step(x, eps, step.cpu(), coef, **ok)),
        ("index int32", lambda: K.dpm_step(x, eps, step.int(), coef, **ok)),
        ("index length", lambda: K.dpm_step(x, eps, step[:2].contiguous(), coef, **ok)),
        ("coef [S, 4]", lambda: K.dpm_step(x, eps, step, coef[:, :4].contiguous(), **ok)),
        ("coef flat", lambda: K.dpm_step(x, eps, step, coef.flatten(), **ok)),
        ("coef strided", lambda: K.dpm_step(x, eps, step, coef[::2], **ok)),
        ("coef float64", lambda: K.dpm_step(x, eps, step, coef.double(), **ok)),
        ("coef on the CPU", lambda: K.dpm_step(x, eps, step, coef.cpu(), **ok)),
        ("neither eps nor x0", lambda: K.dpm_step(x, None, step, coef, **ok)),
    ]
    for what, call in bad:
        with pytest.raises(L.DMCError):
            call()
        torch.cuda.synchronize()
        assert bool(out.isnan().all()) and bool(x0o.isnan().all()), what
    guard_ok("refusals", buf, buf0)
    # the C entry point refuses empty extents itself
    rc = L.LIB.dmc_dpm_step(x.data_ptr(), eps.data_ptr(), None, None, step.data_ptr(), coef.data_ptr(), 0, N, per, 1,
                            out.data_ptr(), x0o.data_ptr(), L.stream())
    assert rc != 0 and b"dpm_step" in L.LIB.dmc_last_error()
    for S, n, p in ((20, 0, per), (20, N, 0)):
        assert L.LIB.dmc_dpm_step(x.data_ptr(), eps.data_ptr(), None, None, step.data_ptr(), coef.data_ptr(), S, n, p,
                                  1, out.data_ptr(), x0o.data_ptr(), L.stream()) != 0
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(x0o.isnan().all())


# ------------------------------------------------------------------------------------------------------------
# the sampler on the Gaussian problem
# ------------------------------------------------------------------------------------------------------------
class GaussianDenoiser:
    """eps of the exact denoiser for N(0, s^2 I) data: a plain callable in torch ops on the device, reading fp32
    tables (a and its two correctly rounded square roots), the op sequence of dpm_reference.gaussian_eps."""

    def __init__(self, s):
        a = tables()["alphas_cumprod"]
        self.a, self.sa, self.s1 = dev(a), dev(sqrt_cr(a)), dev(sqrt_cr(1 - a))
        self.s2 = float(np.float32(s) * np.float32(s))

    def __call__(self, x, t, y=None):
        pick = lambda tab: tab[t].view(-1, 1, 1, 1)   # noqa: E731
        return R.gaussian_eps(x, pick(self.a), pick(self.sa), pick(self.s1), self.s2)


def _solver(steps=20, **kw):
    from diffusion_models_collection_amd.diffusion import DPMSolver
    return DPMSolver(1000, steps, device=DEV, **kw)


SHAPE = (4, 3, 8, 8)


@functools.lru_cache(maxsize=None)
def gauss_xT():
    """|x_T| in [0.5, 1.5): the map x_T -> sample is linear, and a relative error needs x_T away from 0."""
    g = rng(77)
    sign = torch.randint(0, 2, SHAPE, generator=g).float() * 2 - 1
    return sign * (0.5 + torch.rand(SHAPE, generator=g))


@pytest.mark.parametrize("order", [1, 2])
def test_sampler_matches_float64_loop(order):
    """DPMSolver.sample (20 log-SNR steps, no clipping) with the analytic denoiser against the numpy loop over the
    sampler's own fp32 table: float64 as ref64, fp32 as ref32, per sample."""
    smp = _solver(solver_order=order)
    ac = tables()["alphas_cumprod"].numpy()
    ts = smp.inference_timesteps.cpu().numpy()
    coef = smp.step_coefficients.cpu().numpy()
    assert len(ts) == 20 and np.array_equal(ts, R.ref_timesteps(ac, 1000, 20))
    xT = gauss_xT()
    s = 1.0
    got = smp.sample(GaussianDenoiser(s), SHAPE, x_T=dev(xT), clip_denoised=False)
    assert got.shape == SHAPE and got.dtype == F32
    ref32 = R.solver_loop(np.float32, xT.numpy(), R.gaussian_eps_fn(np.float32, ac, ts, s), coef)
    ref64 = R.solver_loop(np.float64, xT.numpy(), R.gaussian_eps_fn(np.float64, ac, ts, s), coef)
    assert ref32.dtype == np.float32 and ref64.dtype == np.float64
    judge(f"dpm sampler order {order}", got, torch.from_numpy(ref32), torch.from_numpy(ref64), rows=SHAPE[0])


@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
def test_accuracy_conditions_on_device(s):
    """Per-element relative error against the closed-form answer, held in the strictest reading (worst order-2 element
    against the best DDIM / order-1 element): (a) order 2 in 20 steps <= DDIM-50 / 1.5, (b) order 1 >= 4 x order 2."""
    from diffusion_models_collection_amd.diffusion import DDIM
    ac = tables()["alphas_cumprod"].numpy()
    xT = gauss_xT()
    exact = torch.from_numpy(R.gaussian_exact(xT.numpy(), ac, 1000, s))
    model = GaussianDenoiser(s)

    def rel_err(out):
        return ((out.cpu().double() - exact).abs() / exact.abs()).flatten()

    e = {}
    for order in (1, 2):
        smp = _solver(solver_order=order)
        assert smp.timestep_spacing == "logsnr" and smp.lower_order_final and len(smp.inference_timesteps) == 20
        e[order] = rel_err(smp.sample(model, SHAPE, x_T=dev(xT), clip_denoised=False))
    ddim = DDIM(1000, 50, device=DEV)
    ts = ddim.inference_timesteps.tolist() + [-1]
    x = dev(xT)
    for i in range(50):
        t = torch.full((SHAPE[0],), ts[i], dtype=torch.long, device=DEV)
        tn = torch.full((SHAPE[0],), ts[i + 1], dtype=torch.long, device=DEV)
        x = ddim.p_sample(model, x, t, tn, clip_denoised=False)
    ed = rel_err(x)
    print(f"s={s}: relative error DDIM-50 [{ed.min():.4e}, {ed.max():.4e}]  order 1 [{e[1].min():.4e}, "
          f"{e[1].max():.4e}]  order 2 [{e[2].min():.4e}, {e[2].max():.4e}]  (a) {ed.min() / e[2].max():.2f}  "
          f"(b) {e[1].min() / e[2].max():.2f}")
    assert float(e[2].max()) <= float(ed.min()) / 1.5
    assert float(e[1].min()) >= 4 * float(e[2].max())


# ------------------------------------------------------------------------------------------------------------
# graph replay against the eager loop
# ------------------------------------------------------------------------------------------------------------
def _unet(name):
    from diffusion_models_collection_amd.models import UNet
    from test_oracle import TINY
    torch.manual_seed(11)
    return UNet(**TINY[name]).to(DEV).eval()


def _graphs(smp):
    return [e[1] for e in smp.__dict__.get("_step_graphs", {}).values()]


def test_graph_equals_eager_unet(monkeypatch):
    """B = 2, 8 steps, tiny UNet: the replayed step gives the eager loop's bits; a second call on the sampler replays
    the kept graph from step 0, where the new x_T and a fresh history must reach it; an in-place weight change
    recaptures."""
    m = _unet("unet_tiny_uncond")
    smp = _solver(8)
    shape = (2, 3, 16, 16)
    xa, xb = (torch.randn(shape, device=DEV) for _ in range(2))

    def run(graph):
        monkeypatch.setenv("DMC_GRAPH", graph)
        return [smp.sample(m, shape, x_T=xa), smp.sample(m, shape, x_T=xb)]

    eager = run("0")
    assert not _graphs(smp)
    graphed = run("1")
    kept = _graphs(smp)
    assert len(kept) == 1                                   # captured by the first call, replayed by the second
    again = run("1")
    assert _graphs(smp) == kept
    for a, b, c in zip(eager, graphed, again):
        assert bool(a.isfinite().all()) and torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(eager[0], eager[1])
    with torch.no_grad():
        next(m.parameters()).mul_(1.01)
    eager2, graphed2 = run("0"), run("1")
    assert len([g for g in _graphs(smp) if g not in kept]) == 1    # the new weights' graph, beside the old one
    for a, b in zip(eager2, graphed2):
        assert torch.equal(a, b)
    assert not torch.equal(eager[0], eager2[0])             # the model does drive the result


@pytest.mark.parametrize("backbone", ["unet", "dit"])
def test_graph_equals_eager_cfg(backbone, monkeypatch):
    """sample_with_cfg: eager == graphed == graph kept across calls (new labels and x_T on the second call), and the
    eager loop == DDPM._cfg_eps + kernels.cfg_x0 + kernels.dpm_step composed by hand, step by step, bitwise."""
    from diffusion_models_collection_amd.diffusion import DDPM
    L, K = _lib()
    if backbone == "unet":
        m = _unet("unet_tiny_cond")
    else:
        import test_gpu_dit
        m, _ = test_gpu_dit.build("dit_tiny_cond")
        m.eval()
    smp = _solver(8)
    shape = (2, 3, 16, 16)
    xa, xb = (torch.randn(shape, device=DEV) for _ in range(2))
    ya, yb = torch.tensor([1, 2], device=DEV), torch.tensor([7, 5], device=DEV)

    def run(graph):
        monkeypatch.setenv("DMC_GRAPH", graph)
        return [smp.sample_with_cfg(m, shape, ya, x_T=xa), smp.sample_with_cfg(m, shape, yb, x_T=xb)]

    eager = run("0")
    assert not _graphs(smp)
    graphed = run("1")
    kept = _graphs(smp)
    assert len(kept) == 1
    again = run("1")
    assert _graphs(smp) == kept
    for a, b, c in zip(eager, graphed, again):
        assert bool(a.isfinite().all()) and torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(eager[0], eager[1])

    monkeypatch.setenv("DMC_GRAPH", "0")
    ts, coef, ac = smp.inference_timesteps, smp.step_coefficients, smp.alphas_cumprod
    x, hist = xa.clone(), None
    with torch.no_grad():
        for i in range(len(ts)):
            t = ts[i].repeat(shape[0])
            k = torch.full((shape[0],), i, dtype=torch.long, device=DEV)
            eps_c, eps_u = DDPM._cfg_eps(m, x, t, ya)
            _, x0 = K.cfg_x0(x, eps_c.contiguous(), eps_u.contiguous(), 3.0, t, ac, None, 0, 0.995)
            x, hist = K.dpm_step(x, None, k, coef, clip=False, x0=x0, x0_prev=hist)
    assert torch.equal(x, eager[0])


def test_return_all_timesteps():
    m = _unet("unet_tiny_uncond")
    smp = _solver(8)
    shape = (2, 3, 16, 16)
    xT = torch.randn(shape, device=DEV)
    plain = smp.sample(m, shape, x_T=xT)
    every = smp.sample(m, shape, x_T=xT, return_all_timesteps=True)
    n = len(smp.inference_timesteps)
    assert every.shape == (n,) + shape
    assert torch.equal(every[-1], plain.cpu())
    assert not torch.equal(every[0], every[-1])
