"""dmc_cfg_guide alone, through kernels.cfg_guide, at the shapes where it can go wrong, judged by the three criteria of
test_gpu_elem_kernels: bit for bit where the kernel has one rounding per op and no reduction (guidance_rescale = 0 without
the quantile), self-calibrating against a float64 restatement where it reduces (the rescale factor) or interpolates (the
quantile), and untouched memory throughout (NaN-prefilled outputs, guards, NaN in every float the kernel must not read).

Rows are read two ways: contiguous, and in place from a [2N, 2*per] buffer (row stride 2*per, the unconditional rows N
rows below the conditional ones): the layout of a batched learned_range model output. Timesteps cycle through T-1, 0 and
500; on the rescaled linear table T-1 has sqrt_alphas_cumprod = 0 exactly. Row kinds cycle too: ordinary, pc == pu
(factor 1), constant (no spread in the guided row: factor 1 by contract).

Every input builder and reference runs on the CPU alone: cpu_selfcheck() calls them all without a GPU.
"""
import functools

import numpy as np
import pytest
import torch

import zsnr_reference as Z
from test_gpu_elem_kernels import (DEV, F32, F64, NAN, RATIOS, SENT, cfg_ref, dev, guard_ok, guarded, judge, rng, same_bits,
                                   tables)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (5, 7), (3, 3072), (300, 48), (2, 12288), (2, 16384)]
LAYOUTS = ("contiguous", "strided")
SCALES = (0.0, 1.0, 3.0)
TS = (999, 0, 500)
ROTS = 5


def _lib():
    from diffusion_models_collection_amd import _lib as L, kernels as K
    return L, K


@functools.lru_cache(maxsize=None)
def guide_tables(zero_snr):
    """(sa, s1, alphas_cumprod) fp32 [1000] of the linear schedule, ordinary or rescaled (never modified)."""
    if not zero_snr:
        tb = tables()
    else:
        from diffusion_models_collection_amd.diffusion import _schedule as S
        tb = {k: torch.from_numpy(v.copy()) for k, v in S.build_tables(1000, 1e-4, 0.02, "linear",
                                                                      zero_terminal_snr=True).items()}
        assert tb["sqrt_alphas_cumprod"][999] == 0 and tb["sqrt_one_minus_alphas_cumprod"][999] == 1
    return tb["sqrt_alphas_cumprod"], tb["sqrt_one_minus_alphas_cumprod"], tb["alphas_cumprod"]


@functools.lru_cache(maxsize=None)
def guide_inputs(N, per, rot=0):
    """x, pc, pu [N, per], t [N]. Row n: t = TS[(n + rot) % 3]; kind (n + rot) % 5 == 1: pc == pu, == 3: constant rows
    (pc = 0.25, pu = -0.5). x is scaled so that x0 falls on both sides of 1."""
    g = rng(7000 + N + per)
    x, pc, pu = (torch.randn(N, per, generator=g) for _ in range(3))
    x = x * 1.5
    t = torch.tensor([TS[(n + rot) % 3] for n in range(N)])
    for n in range(N):
        kind = (n + rot) % 5
        if kind == 1:
            pu[n] = pc[n]
        elif kind == 3:
            pc[n] = 0.25
            pu[n] = -0.5
    return x, pc, pu, t


def rots(N):
    return range(ROTS if N < ROTS else 1)


def guided_ref(dt, pc, pu, scale, phi):
    """The guided, rescaled prediction in precision dt. The factor: in float64 from the sums of squared deviations,
    unrounded; in fp32 'the same arithmetic with torch.std'."""
    N = pc.shape[0]
    c, u = pc.to(dt), pu.to(dt)
    d = c - u
    g = u + scale * d
    if phi > 0:
        ph = float(np.float32(phi))
        if dt == F64:
            m2c = ((c - c.mean(1, keepdim=True)) ** 2).sum(1)
            m2g = ((g - g.mean(1, keepdim=True)) ** 2).sum(1)
            ratio = (m2c / m2g).sqrt()
            ok = m2g > 0
        elif c.shape[1] == 1:                 # torch.std of one element is NaN: no spread, the row is left alone
            ratio, ok = torch.ones(N, dtype=dt), torch.zeros(N, dtype=torch.bool)
        else:
            sg = g.std(1)
            ratio = c.std(1) / sg
            ok = sg > 0
        f = torch.where(ok, ph * ratio + (1 - ph), torch.ones_like(ratio)).view(N, 1)
        g = g * f
    return g


def guide_ref(dt, pred_type, x, pc, pu, scale, phi, t, sa, s1, p):
    """cfg_guide_kernel's ops one at a time in precision dt -> (eps, x0 before the threshold, x0_out)."""
    N = x.shape[0]
    xx = x.to(dt)
    g = guided_ref(dt, pc, pu, scale, phi)
    san, s1n = sa.to(dt)[t].view(N, 1), s1.to(dt)[t].view(N, 1)
    if pred_type == "v":
        eps = s1n * xx + san * g
        x0 = san * xx - s1n * g
    else:
        eps = g
        x0 = (xx - s1n * g) / san
    if p is None:
        return eps, x0, x0.clamp(-1, 1)
    q = torch.quantile(x0.abs(), torch.tensor(float(np.float32(p)), dtype=dt), dim=1)
    s = torch.maximum(q, torch.ones_like(q)).view(N, 1)
    return eps, x0, torch.clamp(x0, -s, s) / s


def lay_out(layout, pc, pu):
    """(pc, pu) on the device in the given layout; strided: views into a NaN-filled [2N, 2*per] buffer."""
    N, per = pc.shape
    if layout == "contiguous":
        return dev(pc), dev(pu)
    buf = torch.full((2 * N, 2 * per), NAN, device=DEV)
    buf[:N, :per] = dev(pc)
    buf[N:, :per] = dev(pu)
    c, u = buf[:N, :per], buf[N:, :per]
    assert (c.stride(0) == 2 * per or N == 1) and u.data_ptr() - c.data_ptr() == 4 * N * 2 * per
    return c, u


def run(K, pred_type, xd, cd, ud, scale, phi, td, sad, s1d, p, want_eps=True):
    N, per = xd.shape
    (eo, eb), (xo, xb) = guarded((N, per)), guarded((N, per))
    r = K.cfg_guide(pred_type, xd, cd, ud, scale, phi, td, sad, s1d, p, out=(eo if want_eps else None, xo))
    assert r[1] is xo and (r[0] is eo if want_eps else r[0] is None)
    torch.cuda.synchronize()
    guard_ok(f"cfg_guide {pred_type} scale={scale} phi={phi} p={p}", eb, xb)
    if not want_eps:
        assert bool(eo.isnan().all())          # never written
    return eo, xo


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N,per", SHAPES)
def test_no_rescale_bitwise(N, per, layout):
    """guidance_rescale = 0, clamp to +-1: 'eps' on the ordinary table is dmc_cfg_x0 mode 0 and the op-by-op
    restatement, bit for bit; 'v' on the rescaled table is the op-by-op restatement, finite at T-1. Without eps_out the
    x0 bits are the same. (5, 7): odd per, rows at odd offsets; (300, 48): more samples than a block has threads;
    (2, 12288) pads the sort buffer; (2, 16384) fills it."""
    L, K = _lib()
    for rot in rots(N):
        x, pc, pu, t = guide_inputs(N, per, rot)
        xd, td = dev(x), dev(t)
        cd, ud = lay_out(layout, pc, pu)
        for scale in SCALES:
            sa, s1, ac = guide_tables(False)
            e32, _, o32 = guide_ref(F32, "eps", x, pc, pu, scale, 0.0, t, sa, s1, None)
            eo, xo = run(K, "eps", xd, cd, ud, scale, 0.0, td, dev(sa), dev(s1), None)
            what = f"eps rot={rot} scale={scale}"
            same_bits(what + " eps_out", eo, e32)
            same_bits(what + " x0_out", xo, o32)
            e_old, x_old = K.cfg_x0(xd, dev(pc), dev(pu), scale, td, dev(ac), None, 0, None)
            same_bits(what + " eps_out vs cfg_x0", eo, e_old.cpu())
            same_bits(what + " x0_out vs cfg_x0", xo, x_old.cpu())
            ref = cfg_ref(F32, x, pc, pu, scale, t, ac, None, 0, None)
            same_bits(what + " x0_out vs cfg_ref", xo, ref[3])

            sa, s1, _ = guide_tables(True)
            e32, x32, o32 = guide_ref(F32, "v", x, pc, pu, scale, 0.0, t, sa, s1, None)
            assert bool(e32.isfinite().all()) and bool(x32.isfinite().all())
            eo, xo = run(K, "v", xd, cd, ud, scale, 0.0, td, dev(sa), dev(s1), None)
            what = f"v rot={rot} scale={scale}"
            same_bits(what + " eps_out", eo, e32)
            same_bits(what + " x0_out", xo, o32)
            last = t == 999
            if bool(last.any()):       # sa = 0, s1 = 1: eps = x and x0 = -g, exactly
                assert torch.equal(eo.cpu()[last], x[last])
            _, xo2 = run(K, "v", xd, cd, ud, scale, 0.0, td, dev(sa), dev(s1), None, want_eps=False)
            same_bits(what + " x0_out without eps_out", xo2, o32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N,per", SHAPES)
def test_quantile_threshold(N, per, layout):
    """p = 0.995 (criterion 2, per row; the kernel's lerp is two roundings, torch's an fma), with and without the
    rescale; eps_out is bitwise without it."""
    L, K = _lib()
    sa, s1, _ = guide_tables(True)
    for rot in rots(N):
        x, pc, pu, t = guide_inputs(N, per, rot)
        cd, ud = lay_out(layout, pc, pu)
        for phi in (0.0, 0.7):
            e32, _, o32 = guide_ref(F32, "v", x, pc, pu, 3.0, phi, t, sa, s1, 0.995)
            _, x64, o64 = guide_ref(F64, "v", x, pc, pu, 3.0, phi, t, sa, s1, 0.995)
            eo, xo = run(K, "v", dev(x), cd, ud, 3.0, phi, dev(t), dev(sa), dev(s1), 0.995)
            if phi == 0:
                same_bits("threshold eps_out", eo, e32)
            judge(f"cfg_guide p=0.995 phi={phi} x0_out", xo, o32, o64, rows=N)
            assert float(xo.abs().max()) <= 1.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N,per", SHAPES)
def test_rescale(N, per, layout):
    """guidance_rescale in {0.7, 1}: eps_out and x0_out per row against the float64 restatement (criterion 2; ref32 is
    the fp32 torch arithmetic with torch.std). With 1 and 'eps', each row's std of eps_out is that row's std of pc.
    'eps' divides by sqrt(alphas_cumprod[t]), 0.0064 at T-1 of the ordinary table: with the x of the other tests all
    but one or two x0 of such a row sit on the clamp and the row's calibration rests on those alone (seen at (300, 48),
    row 102: err 1.1e-5, a third of an ulp of g carried through the division, against a ref32 error of 1.7e-6). So x
    is built around the guided prediction, as test_gpu_elem_kernels.cfg_inputs does: x0 lands near the x0 wanted, on
    both sides of 1, and every element of a row takes part."""
    L, K = _lib()
    for rot in rots(N):
        x0t, pc, pu, t = guide_inputs(N, per, rot)
        cd, ud = lay_out(layout, pc, pu)
        for pred_type, zero in (("v", True), ("eps", False)):
            sa, s1, _ = guide_tables(zero)
            for phi in (0.7, 1.0):
                for scale in SCALES:
                    x = x0t
                    if pred_type == "eps":
                        x = sa[t].view(N, 1) * x0t + s1[t].view(N, 1) * guided_ref(F32, pc, pu, scale, phi)
                    e32, _, o32 = guide_ref(F32, pred_type, x, pc, pu, scale, phi, t, sa, s1, None)
                    e64, _, o64 = guide_ref(F64, pred_type, x, pc, pu, scale, phi, t, sa, s1, None)
                    eo, xo = run(K, pred_type, dev(x), cd, ud, scale, phi, dev(t), dev(sa), dev(s1), None)
                    assert bool(eo.isfinite().all()) and bool(xo.isfinite().all())
                    what = f"cfg_guide {pred_type} phi={phi}"
                    judge(what + " eps_out", eo, e32, e64, rows=N, quiet=True)
                    judge(what + " x0_out", xo, o32, o64, rows=N, quiet=True)
                    if phi == 1.0 and pred_type == "eps" and per > 1:
                        got = eo.cpu().double().std(1)
                        judge(what + " std(eps_out) == std(pc)", got, pc.std(1), pc.double().std(1), rows=N, quiet=True)
                    _, xo2 = run(K, pred_type, dev(x), cd, ud, scale, phi, dev(t), dev(sa), dev(s1), None,
                                 want_eps=False)
                    assert torch.equal(xo2, xo)        # fixed-order sums: the same bits again, with or without eps_out
    for k in sorted(RATIOS):
        if k.startswith("cfg_guide"):
            print(f"criterion 2  {k}: worst ratio {RATIOS[k]:.3f}")


def test_special_rows_take_factor_one():
    """pc == pu: the ratio is 1, so the row is the unrescaled one bit for bit. A guided row without spread (constant, or
    per = 1): factor 1 by contract, finite, again the unrescaled bits."""
    L, K = _lib()
    sa, s1, _ = guide_tables(True)
    for N, per in ((5, 7), (3, 3072), (1, 1)):
        x, pc, pu, t = guide_inputs(N, per, 0)
        e0, x0 = run(K, "v", dev(x), dev(pc), dev(pu), 3.0, 0.0, dev(t), dev(sa), dev(s1), None)
        e1, x1 = run(K, "v", dev(x), dev(pc), dev(pu), 3.0, 1.0, dev(t), dev(sa), dev(s1), None)
        special = torch.tensor([(n % 5) in (1, 3) or per == 1 for n in range(N)])
        assert bool(special.any())
        assert torch.equal(e0.cpu()[special], e1.cpu()[special]) and torch.equal(x0.cpu()[special], x1.cpu()[special])
        if N > 1:
            assert not torch.equal(e0.cpu()[~special], e1.cpu()[~special])


def test_limit_and_refusals():
    """per = 16385 is refused with nothing launched and the library stays usable; the wrapper's operand checks raise
    DMCError before any launch."""
    L, K = _lib()
    sa, s1, _ = guide_tables(True)
    sad, s1d = dev(sa), dev(s1)
    N, per = 2, 16385
    x = torch.randn(N, per, device=DEV)
    t = torch.tensor([3, 999], device=DEV)
    eo = torch.full((N, per), SENT, device=DEV)
    xo = torch.full((N, per), SENT, device=DEV)
    with pytest.raises(L.DMCError, match="16384"):
        K.cfg_guide("v", x, x, x, 1.0, 0.7, t, sad, s1d, 0.995, out=(eo, xo))
    torch.cuda.synchronize()
    assert bool((eo == SENT).all()) and bool((xo == SENT).all())

    N, per = 4, 12
    x, pc, pu = (torch.randn(N, per, device=DEV) for _ in range(3))
    t = torch.tensor([0, 999, 500, 7], device=DEV)
    ok = lambda **kw: dict(dict(pred_type="v", x=x, pc=pc, pu=pu, scale=3.0, rescale=0.7, t=t, sa=sad, s1=s1d,   # noqa: E731
                                p_threshold=0.995), **kw)
    wide = torch.randn(N, 2 * per, device=DEV)
    bad = {
        "pc dtype": ok(pc=pc.double()), "pu dtype": ok(pu=pu.half()), "x dtype": ok(x=x.double()),
        "pc device": ok(pc=pc.cpu()), "x device": ok(x=x.cpu()), "table device": ok(sa=sa),
        "pc inner stride": ok(pc=wide[:, ::2]), "pu transposed": ok(pu=torch.randn(per, N, device=DEV).t()),
        "pc overlapping rows": ok(pc=torch.randn(per + N, device=DEV).as_strided((N, per), (1, 1))),
        "pc shape": ok(pc=wide), "pu rows": ok(pu=torch.randn(N + 1, per, device=DEV)), "pc None": ok(pc=None),
        "t dtype": ok(t=t.int()), "t length": ok(t=t[:3]), "t None": ok(t=None),
        "table lengths": ok(s1=s1d[:999]), "table dtype": ok(sa=sad.double()), "no table": ok(s1=None),
        "rescale above 1": ok(rescale=1.5), "rescale below 0": ok(rescale=-0.1), "rescale nan": ok(rescale=NAN),
        "prediction type": ok(pred_type="x0"),
        "out shape": ok(out=(torch.empty(N, per, device=DEV), torch.empty(N, per + 1, device=DEV))),
        "out dtype": ok(out=(None, torch.empty(N, per, device=DEV, dtype=torch.float64))),
        "no x0 buffer": ok(out=(torch.empty(N, per, device=DEV), None)),
    }
    for what, kw in bad.items():
        with pytest.raises(L.DMCError):
            K.cfg_guide(**kw)
            pytest.fail(f"{what}: not refused")
    # a strided view of the right kind is taken, and the library still works after the refusals
    e1, x1 = K.cfg_guide(**ok(pc=wide[:, :per]))
    e2, x2 = K.cfg_guide(**ok(pc=wide[:, :per].contiguous()))
    assert torch.equal(e1, e2) and torch.equal(x1, x2) and bool(x1.isfinite().all())


def cpu_selfcheck():
    """Every builder and reference above without a GPU: the restatement agrees with tests/zsnr_reference.py's numpy one
    and with cfg_ref, its two precisions agree to rounding, and the inputs hold every row kind and timestep."""
    for N, per in SHAPES[:5]:
        for rot in rots(N):
            x, pc, pu, t = guide_inputs(N, per, rot)
            for pred_type, zero in (("v", True), ("eps", False)):
                sa, s1, ac = guide_tables(zero)
                for phi in (0.0, 0.7, 1.0):
                    e32, x32, o32 = guide_ref(F32, pred_type, x, pc, pu, 3.0, phi, t, sa, s1, 0.995)
                    e64, x64, o64 = guide_ref(F64, pred_type, x, pc, pu, 3.0, phi, t, sa, s1, 0.995)
                    assert bool(e64.isfinite().all()) and bool(o64.isfinite().all())
                    assert float((e32.double() - e64).abs().max()) < 1e-4 * max(1.0, float(e64.abs().max()))
                    en, xn = Z.guide(np.float64, pred_type, x.numpy(), pc.numpy(), pu.numpy(), 3.0, phi,
                                     sa[t].numpy(), s1[t].numpy())
                    assert np.allclose(en, e64.numpy(), rtol=1e-6, atol=1e-6 * float(e64.abs().max()))
                    assert np.allclose(xn, x64.numpy(), rtol=1e-6, atol=1e-6 * float(x64.abs().max()))
                if pred_type == "eps":
                    a = guide_ref(F32, "eps", x, pc, pu, 3.0, 0.0, t, sa, s1, None)
                    b = cfg_ref(F32, x, pc, pu, 3.0, t, ac, None, 0, None)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[3])
    x, pc, pu, t = guide_inputs(300, 48)
    assert set(t.tolist()) == set(TS) and bool((pc[1] == pu[1]).all()) and bool((pc[3] == 0.25).all())
    return True
