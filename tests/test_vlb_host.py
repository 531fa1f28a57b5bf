"""Host side of the bits-per-dimension evaluation (diffusion/_vlb.py): the coefficient table and the prior constants
against the float64 restatement of the papers' forms (tests/vlb_reference.py), and argument validation. No GPU and no
kernel launch."""
import math

import numpy as np
import pytest
import torch

import vlb_reference as R

SCHEDULES = {"linear1000": (1000, "linear"), "cosine1000": (1000, "cosine"), "linear8": (8, "linear")}
VARIANCES = ("fixed_small", "fixed_large")
EPS32 = 2.0 ** -23


def _ac(name):
    from diffusion_models_collection_amd.diffusion import _schedule as S
    T, kind = SCHEDULES[name]
    return S.build_tables(T, 1e-4, 0.02, kind)["alphas_cumprod"]


def _V():
    from diffusion_models_collection_amd.diffusion import _vlb
    return _vlb


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_table_shape_and_variance_term(name):
    """[T, 6] fp32; kvar is exactly 0 for fixed_small, and > 0 for t >= 1 (0 at t = 0) with fixed_large."""
    V = _V()
    ac = _ac(name)
    T = ac.shape[0]
    for ptype in ("eps", "v"):
        small = V.vlb_coefficients(ac, ptype, "fixed_small")
        large = V.vlb_coefficients(ac, ptype, "fixed_large")
        for c in (small, large):
            assert c.dtype == np.float32 and c.shape == (T, 6) and c.flags["C_CONTIGUOUS"] and bool(np.isfinite(c).all())
        assert bool((small[:, V.KVAR] == 0).all())
        assert large[0, V.KVAR] == 0 and bool((large[1:, V.KVAR] > 0).all())
        # the variance choice moves nothing but kprec, kvar and isig; rows 0 agree entirely
        assert np.array_equal(small[:, [V.C_X, V.C_P, V.KEPS]], large[:, [V.C_X, V.C_P, V.KEPS]])
        assert np.array_equal(small[0], large[0])


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("variance", VARIANCES)
def test_table_identities(name, variance):
    """Row 0 has c1 = 1, so kprec[0] = 0.5 isig[0]^2; keps c_p^2 = 1 = a c_x^2 for 'eps'; every column is the float64
    restatement's rounded once."""
    V = _V()
    ac = _ac(name)
    c = V.vlb_coefficients(ac, "eps", variance).astype(np.float64)
    assert abs(c[0, V.KPREC] / (0.5 * c[0, V.ISIG] ** 2) - 1) <= 4 * EPS32
    # x0 - u = c_p (pred - eps), so keps turns the x0 error into the eps error iff keps c_p^2 = 1, which with
    # c_x^2 = 1 + c_p^2 reads keps (c_x^2 - 1) = 1 as well (loose at small t, where c_x^2 - 1 cancels)
    assert float(np.abs(c[:, V.KEPS] * c[:, V.C_P] ** 2 - 1).max()) <= 3 * EPS32       # three fp32 factors
    a = _ac(name).astype(np.float64)
    assert float(np.abs(c[:, V.C_X] ** 2 * a - 1).max()) <= 2 * EPS32
    assert float(np.abs((c[:, V.C_X] ** 2 - 1) / c[:, V.C_P] ** 2 - 1).max()) <= 4 * EPS32 / (1 - a[0])
    for ptype in ("eps", "v"):
        got = V.vlb_coefficients(ac, ptype, variance)
        ref = R.coefficients(torch.from_numpy(ac), ptype, variance)
        for col, k in enumerate(("c_x", "c_p", "kprec", "kvar", "keps", "isig")):
            r = ref[k].numpy()
            assert bool((np.abs(got[:, col].astype(np.float64) - r) <= EPS32 * np.abs(r) + 1e-30).all()), (ptype, k)


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("variance", VARIANCES)
def test_table_form_is_the_textbook_kl(name, variance):
    """float64: kvar + kprec (x0 - x0_pred)^2 equals the KL of the two Gaussians with both means formed, at every
    timestep >= 1, for a good and a bad x0 prediction."""
    ac = torch.from_numpy(_ac(name))
    T = ac.shape[0]
    g = torch.Generator().manual_seed(5)
    t = torch.arange(1, T)
    N, per = T - 1, 16
    x0 = R.grid_images((N, per), g)
    eps = torch.randn(N, per, generator=g)
    a = ac.double()[t].view(-1, 1)
    x_t = (a.sqrt() * x0 + (1 - a).sqrt() * eps).float()
    co = R.coefficients(ac, "eps", variance)
    for sigma in (0.05, 1.0):
        pred = eps + sigma * torch.randn(N, per, generator=g)
        x0_pred = co["c_x"][t].view(-1, 1) * x_t.double() - co["c_p"][t].view(-1, 1) * pred.double()
        table = co["kvar"][t].view(-1, 1) + co["kprec"][t].view(-1, 1) * (x0.double() - x0_pred) ** 2
        text = R.textbook_kl(ac, variance, t, x0, x0_pred, x_t)
        # the textbook form's own float64 error: the difference of the means loses |mu| / |mu_q - mu_p| of the digits
        # (and its square twice that), -1 + d + exp(-d) is good to a few ulps of 1
        _, _, _, _, c1, c2 = R.schedule(ac)
        mu = (c1[t].view(-1, 1) * x0.double()).abs() + (c2[t].view(-1, 1) * x_t.double()).abs()
        diff = (c1[t].view(-1, 1) * (x0.double() - x0_pred)).abs()
        tol = (1e-12 + 8 * 2.0 ** -52 * mu / diff) * text.abs() + 2e-15
        assert bool(((table - text).abs() <= tol).all()), (name, variance, sigma)
        assert float((mu / diff).max()) > 1e3            # the cancellation the table form avoids is there
        vb = R.vlb_step(torch.float64, ac, "eps", variance, t, x0, x_t, pred, False, rounded=False)[0]
        assert bool(((vb - text.mean(1) / R.LN2).abs() <= tol.mean(1) / R.LN2).all())


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_prior_constants(name):
    """A + Bc mean(x0^2) is KL(q(x_T | x0) || N(0, I)) in bits per dimension: at x0 = 0, at x0 = 1 and on an image."""
    V = _V()
    ac = _ac(name)
    A, Bc = V.prior_constants(ac)
    act = torch.from_numpy(ac)
    assert math.isclose(A, float(R.prior_bpd(act, torch.zeros(1, 12))[0]), rel_tol=1e-12, abs_tol=1e-300)
    assert math.isclose(A + Bc, float(R.prior_bpd(act, torch.ones(1, 12))[0]), rel_tol=1e-12)
    x0 = R.grid_images((2, 48), torch.Generator().manual_seed(3))
    ref = R.prior_bpd(act, x0)
    got = A + Bc * (x0.double() ** 2).mean(1)
    assert float(((got - ref).abs() / ref).max()) < 1e-12
    assert A >= 0 and Bc > 0


def test_refusals():
    """A bad variance, bad timesteps, a bad prediction type and a bad table are each a ValueError."""
    V = _V()
    ac = _ac("linear8")
    for variance in ("learned", "posterior", None, 0):
        with pytest.raises(ValueError):
            V.vlb_coefficients(ac, "eps", variance)
        with pytest.raises(ValueError):
            V.log_variances(ac, variance)
    for ptype in ("x0", "epsilon", None):
        with pytest.raises(ValueError):
            V.vlb_coefficients(ac, ptype, "fixed_small")
    for ts in ([], [8], [-1], [3, 3], [1.0, 2.0], ["1"], [True], 3, [0, 1, 9]):
        with pytest.raises(ValueError):
            V.walk_timesteps(ts, 8)
    for bad in (ac[:1], np.ones(4, np.float32), np.zeros(4, np.float32), ac[::-1], ac.reshape(2, 4)):
        with pytest.raises(ValueError):
            V.vlb_coefficients(bad, "eps", "fixed_small")
        with pytest.raises(ValueError):
            V.prior_constants(bad)
    assert V.walk_timesteps(None, 8).tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    assert V.walk_timesteps([0, 5, 3], 8).tolist() == [5, 3, 0]
    assert V.walk_timesteps(np.array([2, 7]), 8).tolist() == [7, 2]
    assert V.walk_timesteps(None, 8).dtype == np.int64


def test_public_classes_carry_calc_bpd():
    """DDPM, DDIM and DPMSolver share the one method; CPU tensors and bad arguments are refused before any launch."""
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver
    from diffusion_models_collection_amd.diffusion._likelihood import LikelihoodMixin
    from diffusion_models_collection_amd import _lib
    assert "dmc_vlb_step" in _lib.EXPORTS
    for cls in (DDPM, DDIM, DPMSolver):
        assert issubclass(cls, LikelihoodMixin) and cls.calc_bpd is LikelihoodMixin.calc_bpd
    d = DDPM(num_timesteps=8, device="cpu")
    with pytest.raises(RuntimeError):
        d.calc_bpd(lambda x, t, y=None: x, torch.zeros(2, 3, 4, 4))
