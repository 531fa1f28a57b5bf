"""Rectified flow, host side (diffusion/_flow.py, diffusion/flow.py, the logit-normal sampler of diffusion/_resample.py)
without a GPU: the tables against the numpy restatement in tests/flow_reference.py bit for bit, the solvers' orders of
accuracy on the Gaussian problem in float64, the logit-normal bin masses and draw, and every refusal."""
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import flow_reference as R

SHAPE = (4, 3, 8, 8)


def _flow():
    from diffusion_models_collection_amd.diffusion import _flow
    return _flow


def _rf(*args, **kw):
    from diffusion_models_collection_amd.diffusion import RectifiedFlow
    return RectifiedFlow(*args, device="cpu", **kw)


@functools.lru_cache(maxsize=None)
def gauss_xT():
    """|x_T| in [0.5, 1.5): the map x_T -> sample is linear, and a relative error needs x_T away from 0 (never
    modified)."""
    g = torch.Generator().manual_seed(77)
    sign = torch.randint(0, 2, SHAPE, generator=g).float() * 2 - 1
    return sign * (0.5 + torch.rand(SHAPE, generator=g))


# ------------------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [10, 1000])
@pytest.mark.parametrize("shift", [1, 3, 6.5])
def test_sigma_tables(T, shift):
    sig, om = _flow().flow_sigmas(T, shift)
    assert sig.dtype == np.float32 and om.dtype == np.float32 and sig.shape == om.shape == (T,)
    assert sig[T - 1] == np.float32(1.0) and om[T - 1] == 0
    assert sig[0] > 0 and bool((np.diff(sig) > 0).all())
    rs, ro = R.ref_sigmas(T, shift)
    assert sig.tobytes() == rs.tobytes() and om.tobytes() == ro.tobytes()
    if shift == 1:
        assert np.array_equal(sig, (np.arange(1, T + 1) / T).astype(np.float32))
    smp = _rf(T, min(T, 10), shift=shift)
    assert smp.sigmas.numpy().tobytes() == rs.tobytes() and smp.one_minus_sigmas.numpy().tobytes() == ro.tobytes()
    assert smp.num_timesteps == T and smp.device == "cpu"


@pytest.mark.parametrize("solver", ["euler", "heun"])
@pytest.mark.parametrize("T,S", [(1000, 1), (1000, 10), (10, 10), (1000, 7)])
def test_row_tables(T, S, solver):
    from diffusion_models_collection_amd.diffusion import _schedule
    smp = _rf(T, S, shift=3.0, solver=solver)
    ts = smp.inference_timesteps.numpy()
    assert ts.dtype == np.int64 and np.array_equal(ts, _schedule.trailing_timesteps(T, S))
    assert np.array_equal(ts, R.ref_timesteps(T, S)) and ts[0] == T - 1
    coef, tt = smp.step_coefficients.numpy(), smp.step_timesteps.numpy()
    rc, rt = R.ref_rows(R.ref_sigmas(T, 3.0)[0], R.ref_timesteps(T, S), solver)
    assert coef.dtype == np.float32 and tt.dtype == np.int64
    assert coef.shape == rc.shape and coef.tobytes() == rc.tobytes() and np.array_equal(tt, rt)
    Rn = S if solver == "euler" else 2 * S - 1
    assert coef.shape == (Rn, 4) and tt.shape == (Rn,)
    kind = coef[:, 3]
    if solver == "euler" or S == 1:
        assert bool((kind == 0).all())
    else:
        assert kind.tolist() == [1.0, 2.0] * (S - 1) + [0.0]
        assert np.array_equal(tt[0::2], ts) and np.array_equal(tt[1::2], ts[1:])      # the corrector sits at ts[i+1]
        assert np.array_equal(coef[0:-1:2, 1], coef[1::2, 1])                          # with interval i's h
    assert bool((coef[:, 1] < 0).all())
    assert np.array_equal(coef[:, 0], smp.sigmas.numpy()[tt])
    closing = coef[kind != 1, 1].astype(np.float64)
    assert len(closing) == S and abs(closing.sum() + 1.0) <= 1e-6
    assert np.array_equal(coef[:, 2] * np.float32(2), coef[:, 1])          # halving commutes with the rounding


def test_heun_single_step_is_one_euler_row():
    smp = _rf(1000, 1, solver="heun")
    assert smp.step_coefficients.tolist() == [[1.0, -1.0, -0.5, 0.0]] and smp.step_timesteps.tolist() == [999]


# ------------------------------------------------------------------------------------------------------------
# the float64 loop of the reference
# ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def errors64(s):
    return R.relative_errors(1000, 1.0, s, gauss_xT().numpy().astype(np.float64))


def check_conditions(e, what):
    """(a) Heun-10 (19 evaluations) <= Euler-20 / 3, (b) Euler halves (first order), (c) Heun quarters (second)."""
    a = e["euler", 20] / e["heun", 10]
    b = e["euler", 10] / e["euler", 20]
    c = e["heun", 10] / e["heun", 20]
    print(f"{what}: Euler-10 {e['euler', 10]:.4e} Euler-20 {e['euler', 20]:.4e} Heun-10 {e['heun', 10]:.4e} Heun-20 "
          f"{e['heun', 20]:.4e}  (a) {a:.2f}  (b) {b:.2f}  (c) {c:.2f}")
    assert e["heun", 10] <= e["euler", 20] / 3
    assert 1.7 <= b <= 2.3
    assert 3.5 <= c <= 5.5


@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
def test_accuracy_conditions_float64(s):
    check_conditions(errors64(s), f"float64 s={s}")


def test_point_mass_is_exact_for_euler():
    """v = (x - c)/sigma: every Euler step moves along the straight line to c, and the last one (h = -sigma) lands on it."""
    sig, _ = R.ref_sigmas(1000, 3.0)
    coef, tt = R.ref_rows(sig, R.ref_timesteps(1000, 7), "euler")
    xT = gauss_xT().numpy().astype(np.float64)
    c = 0.3
    x = R.sampler_loop(np.float64, xT, R.point_velocity_fn(sig, c), coef, tt)
    assert float(np.abs(x - c).max()) <= 1e-12


def test_step_mirror_precisions_agree():
    """flow_step_ref / flow_guide_ref: fp32 against float64 to rounding, and the kinds do what the formulas say."""
    g = np.random.default_rng(5)
    N, per = 6, 11
    x, pc, pu, xb, d = (g.standard_normal((N, per)).astype(np.float32) for _ in range(5))
    sig, _ = R.ref_sigmas(1000, 1.0)
    coef, _ = R.ref_rows(sig, R.ref_timesteps(1000, 10), "heun")
    step = np.array([0, 1, 18, 4, 5, 99])       # kinds 1, 2, 0, 1, 2 and an index past the table (clamped to row 18)
    o32 = R.flow_step_ref(np.float32, coef, step, x, pc, pu, 3.0, xb, d)
    o64 = R.flow_step_ref(np.float64, coef, step, x, pc, pu, 3.0, xb, d)
    for a, b in zip(o32, o64):
        m = ~np.isnan(b)
        assert a.dtype == np.float32 and b.dtype == np.float64 and float(np.abs(a[m] - b[m]).max()) < 1e-3
    out, xbo, do = o64
    gg = pu.astype(np.float64) + 3.0 * (pc.astype(np.float64) - pu)
    assert np.allclose(out[0], x[0] + coef[0, 1].astype(np.float64) * gg[0], rtol=1e-12)
    assert np.allclose(out[1], xb[1] + coef[1, 2].astype(np.float64) * (d[1] + gg[1]), rtol=1e-12)
    assert np.array_equal(out[5], out[5]) and np.allclose(out[5], x[5] + coef[18, 1].astype(np.float64) * gg[5])
    assert np.array_equal(xbo[0], x[0]) and np.array_equal(do[3], gg[3]) and np.isnan(xbo[1]).all() and np.isnan(do[2]).all()
    assert np.isnan(R.flow_step_ref(np.float32, coef, step, x, pc, None, 1.0, None, None)[0][[1, 4]]).all()
    for mode, p in (("none", None), ("clamp", None), ("quantile", 0.995)):
        for phi in (0.0, 0.7):
            a = R.flow_guide_ref(np.float32, coef, step, x, pc, pu, 3.0, phi, mode, p)
            b = R.flow_guide_ref(np.float64, coef, step, x, pc, pu, 3.0, phi, mode, p)
            assert a.dtype == np.float32 and float(np.abs(a - b).max()) < 1e-3 * max(1.0, float(np.abs(b).max()))


# ------------------------------------------------------------------------------------------------------------
# logit-normal timesteps
# ------------------------------------------------------------------------------------------------------------
def _resample():
    from diffusion_models_collection_amd.diffusion import _resample
    return _resample


class Sched:
    num_timesteps = 1000
    device = "cpu"


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (-0.5, 0.7)])
def test_logit_normal_masses_and_draw(mean, std):
    from diffusion_models_collection_amd import diffusion as D
    M = _resample()
    T = 1000
    p = M.logit_normal_masses(T, mean, std)
    assert p.dtype == np.float64 and p.shape == (T,) and bool((p > 0).all())
    assert abs(float(p.sum()) - 1.0) <= 1e-12
    ref = R.logit_normal_masses(T, mean, std)
    assert float(np.abs(p - ref).max()) <= 1e-15
    if mean == 0:
        assert float(np.abs(p - p[::-1]).max()) <= 1e-15
        assert p[T // 2] > 10 * p[0]                                         # the middle levels carry the weight
    cdf = M.logit_normal_cdf(p)
    assert cdf.dtype == np.float32 and bool((np.diff(cdf) >= 0).all()) and cdf[-1] == np.float32(1.0)

    smp = D.create_named_schedule_sampler("logit-normal", Sched(), mean=mean, std=std)
    assert isinstance(smp, D.LogitNormalSampler) and smp.weight_table() is None
    assert smp.cdf("cpu").numpy().tobytes() == cdf.tobytes()
    N = 100_000
    u = torch.from_numpy(((np.arange(N) + 0.5) / N).astype(np.float32))
    t, w = smp.sample(N, "cpu", u=u)
    assert t.dtype == torch.long and t.shape == (N,) and bool((w == 1).all()) and w.dtype == torch.float32
    assert np.array_equal(t.numpy(), np.minimum(np.searchsorted(cdf, u.numpy(), side="right"), T - 1))
    count = np.bincount(t.numpy(), minlength=T)
    assert float(np.abs(count - N * ref).max()) <= 2.0
    smp.update_with_local_losses(t, w)                                         # nothing to feed
    t2, _ = smp.sample(16, "cpu")
    assert t2.shape == (16,) and 0 <= int(t2.min()) and int(t2.max()) < T
    assert abs(float(smp.weights().double().sum()) - 1.0) < 1e-5


def test_logit_normal_refusals():
    from diffusion_models_collection_amd import diffusion as D
    M = _resample()
    for name in ("Uniform", "loss_second_moment", "", None, "importance", "logit_normal", "Logit-Normal"):
        with pytest.raises(ValueError):
            D.create_named_schedule_sampler(name, Sched())
    assert M.check_sampler_name("logit-normal") == "logit-normal"
    for kw in (dict(std=0.0), dict(std=-1.0), dict(std=math.nan), dict(std=math.inf), dict(mean=math.inf),
               dict(mean=math.nan), dict(mean="0"), dict(std=None), dict(std=True)):
        with pytest.raises(ValueError):
            D.create_named_schedule_sampler("logit-normal", Sched(), **kw)
    with pytest.raises(ValueError):
        D.LogitNormalSampler(Sched()).sample(4, "cpu", u=torch.rand(3))


# ------------------------------------------------------------------------------------------------------------
# refusals, no device touched
# ------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    for kw in (dict(solver="rk4"), dict(solver=None), dict(shift=0.5), dict(shift=math.nan), dict(shift=math.inf),
               dict(shift="3"), dict(shift=None), dict(num_inference_steps=0), dict(num_inference_steps=1001),
               dict(num_inference_steps=2.5), dict(num_timesteps=0)):
        with pytest.raises(ValueError):
            _rf(**kw)
    smp = _rf(10, 10, shift=1, solver="heun")
    assert smp.shift == 1.0 and smp.solver == "heun" and smp.num_inference_steps == 10
    assert len(smp.step_timesteps) == 19 and smp.graphed_train_step is False


def test_argument_refusals():
    smp = _rf(1000, 10)
    y = torch.tensor([1])
    shape = (1, 3, 8, 8)
    with pytest.raises(ValueError):
        smp.sample_with_cfg(None, shape, None)
    for p in (1.0, 0.0, -0.5, 1.5, "0.9"):
        with pytest.raises(ValueError):
            smp.sample_with_cfg(None, shape, y, p_threshold=p)
    for g in (-0.1, 1.5, math.nan, "0.7", None):
        with pytest.raises(ValueError):
            smp.sample_with_cfg(None, shape, y, guidance_rescale=g)
    x = torch.zeros(shape)
    t = torch.tensor([3])
    for kw in (dict(snr_gamma=5.0), dict(vlb_weight=0.001), dict(return_parts=True)):
        with pytest.raises(ValueError, match="no SNR weight or variance head"):
            smp.p_losses(None, x, t, **kw)
    with pytest.raises(ValueError):
        smp.p_losses(None, x, t, loss_type="l3")
    for name in ("calc_bpd", "img2img", "inpaint", "invert"):
        with pytest.raises(NotImplementedError, match="RectifiedFlow"):
            getattr(smp, name)(None, x)


def test_exports():
    from diffusion_models_collection_amd import diffusion as D
    assert {"RectifiedFlow", "LogitNormalSampler"} <= set(D.__all__)
    root = Path(__file__).resolve().parent.parent
    saved = {k: v for k, v in sys.modules.items() if k == "diffusion" or k.startswith("diffusion.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, str(root / "dropin"))
    try:
        import diffusion
        assert Path(diffusion.__file__).resolve() == root / "dropin" / "diffusion" / "__init__.py"
        assert diffusion.RectifiedFlow is D.RectifiedFlow and "RectifiedFlow" in diffusion.__all__
    finally:
        sys.path.remove(str(root / "dropin"))
        for k in [k for k in sys.modules if k == "diffusion" or k.startswith("diffusion.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_trainer_gate_defaults_to_supported():
    """GraphedTrainStep.supported reads the opt-out with a default: an object without the attribute answers as before."""
    from diffusion_models_collection_amd.diffusion import DDPM, RectifiedFlow
    assert getattr(DDPM, "graphed_train_step", True) is True
    assert RectifiedFlow.graphed_train_step is False
