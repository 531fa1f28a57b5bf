"""Host side of learned variances (diffusion/_vlb.py learned_coefficients, variance_type on the samplers): the table
against the float64 restatement (tests/lvar_reference.py) and argument validation. No GPU and no kernel launch."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lvar_reference as R

SCHEDULES = {"linear1000": (1000, "linear"), "cosine1000": (1000, "cosine"), "linear8": (8, "linear")}
NEW = ("dmc_hybrid_objective", "dmc_vlb_step_learned", "dmc_ddpm_step_learned")


def _ac(name):
    from diffusion_models_collection_amd.diffusion import _schedule as S
    T, kind = SCHEDULES[name]
    return S.build_tables(T, 1e-4, 0.02, kind)["alphas_cumprod"]


def _V():
    from diffusion_models_collection_amd.diffusion import _vlb
    return _vlb


@pytest.mark.parametrize("ptype", ["eps", "v"])
@pytest.mark.parametrize("name", list(SCHEDULES))
def test_table_columns(name, ptype):
    """[T, 8] fp32, every column the float64 formula rounded once (half an ulp), R > 0 everywhere."""
    V = _V()
    ac = _ac(name)
    c = V.learned_coefficients(ac, ptype)
    T = ac.shape[0]
    assert c.dtype == np.float32 and c.shape == (T, 8) and c.flags["C_CONTIGUOUS"] and bool(np.isfinite(c).all())
    cols = (V.L_CX, V.L_CP, V.L_C1, V.L_LVMIN, V.L_R, V.L_KMIN, V.L_KEPS, V.L_LVMAX)
    assert cols == tuple(range(8))
    ref = R.coefficients(torch.from_numpy(ac), ptype)
    for k, col in zip(R.COLUMNS, cols):
        r64 = ref[k].numpy()
        assert np.array_equal(c[:, col], r64.astype(np.float32)), k
    assert bool((c[:, V.L_R] > 0).all())
    assert bool((ref["R"] > 0).all())


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_table_identities(name):
    """lv_min is log_variances' lv_q; R = lv_max - lv_min to float64 rounding of the difference, and the log1p form keeps
    the digits the difference loses; c1[0] = 1; the prediction type moves c_x and c_p only."""
    V = _V()
    ac = _ac(name)
    ref = R.coefficients(torch.from_numpy(ac), "eps")
    lv_p, lv_q = V.log_variances(ac, "fixed_small")
    assert np.array_equal(ref["lv_min"].numpy(), lv_q)
    c = V.learned_coefficients(ac, "eps")
    assert np.array_equal(c[:, V.L_LVMIN], lv_q.astype(np.float32))
    diff = (ref["lv_max"] - ref["lv_min"]).numpy()
    R64 = ref["R"].numpy()
    # each log carries half an ulp of its own value into the difference
    mag = np.abs(ref["lv_min"].numpy()) + np.abs(ref["lv_max"].numpy()) + 1.0
    assert bool((np.abs(diff - R64) <= 4 * np.finfo(np.float64).eps * mag).all())
    # against exact rational arithmetic on the fp32 table: R = -log((1 - a_prev) / (1 - a)) for t >= 1
    a = ac.astype(np.float64)
    exact = -np.log((1.0 - a[:-1]) / (1.0 - a[1:]))
    assert bool((np.abs(R64[1:] - exact) <= 1e-9 * np.abs(exact) + 1e-18).all())
    assert c[0, V.L_C1] == 1.0
    v = V.learned_coefficients(ac, "v")
    assert np.array_equal(c[:, 2:], v[:, 2:]) and not np.array_equal(c[:, :2], v[:, :2])
    # v = -1 is the posterior variance, v = +1 is beta
    assert bool((np.abs(ref["lv_min"].numpy()[1:] + R64[1:] - np.log(1.0 - a[1:] / a[:-1])) <= 1e-12).all())


def test_expm1_form_keeps_the_small_terms():
    """The finding behind the kernel's form: in fp32 the plain -1 + d + exp(-d) is exactly 0 at the noisy end of the linear
    schedule, the expm1 form is not."""
    ac = torch.from_numpy(_ac("linear1000"))
    Rt = R.table(ac, "eps")["R"]
    assert 0.6 < float(Rt[0]) < 0.62 and 8.0e-7 < float(Rt[999]) < 8.5e-7
    for t, frac in ((500, 0.25), (999, 0.5), (999, 1.25)):
        d = torch.tensor(frac, dtype=torch.float32) * Rt[t]
        plain = (-1.0 + d) + torch.exp(-d)
        good = d + torch.expm1(-d)
        d64 = d.double()
        ref = d64 + torch.expm1(-d64)
        assert float(plain) == 0.0 and float(good) > 0.0
        assert abs(float(good) - float(ref)) <= 0.5 * float(ref), (t, frac, float(good), float(ref))


def test_refusals():
    V = _V()
    ac = _ac("linear8")
    for ptype in ("x0", "epsilon", None):
        with pytest.raises(ValueError):
            V.learned_coefficients(ac, ptype)
    for bad in (ac[:1], np.ones(4, np.float32), np.zeros(4, np.float32), ac[::-1], ac.reshape(2, 4)):
        with pytest.raises(ValueError):
            V.learned_coefficients(bad, "eps")
    for vt in ("learned", "fixed_small", None, 0, "range"):
        with pytest.raises(ValueError):
            V.check_variance_type(vt)
    assert V.check_variance_type("fixed") == "fixed" and V.check_variance_type("learned_range") == "learned_range"


def test_samplers_carry_variance_type():
    """The constructor keyword, set_variance_type (which drops the cached step graphs), and the refusals that need no
    launch: an unknown type, variance='learned' on a fixed sampler, vlb_weight / return_parts on a fixed sampler."""
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver
    for cls in (DDPM, DDIM, DPMSolver):
        d = cls(num_timesteps=8, device="cpu")
        assert d.variance_type == "fixed"
        with pytest.raises(ValueError):
            cls(num_timesteps=8, device="cpu", variance_type="learned")
        with pytest.raises(ValueError):
            d.set_variance_type("fixed_small")
        with pytest.raises(ValueError, match="learned_range"):
            d.calc_bpd(lambda x, t, y=None: x, torch.zeros(2, 3, 4, 4), variance="learned")
        d.__dict__["_step_graphs"] = {"stale": None}
        d.set_variance_type("learned_range")
        assert d.variance_type == "learned_range" and "_step_graphs" not in d.__dict__
        assert cls(num_timesteps=8, device="cpu", variance_type="learned_range").variance_type == "learned_range"
        tab = d._lvar_table(torch.device("cpu"))
        assert tab.shape == (8, 8) and tab.dtype == torch.float32 and d._lvar_table(torch.device("cpu")) is tab
        for w in (-1.0, float("inf"), float("nan"), "0.1", True):
            with pytest.raises(ValueError):
                d._vlb_weight(w)
        assert d._vlb_weight(None) == 0.001 and d._vlb_weight(0) == 0.0
    fixed = DDPM(num_timesteps=8, device="cpu")
    x = torch.zeros(2, 3, 4, 4)
    for kw in (dict(vlb_weight=0.001), dict(return_parts=True)):
        with pytest.raises(ValueError):
            fixed._losses(x, x, x, torch.zeros(2, dtype=torch.long), "l2", None, kw.get("vlb_weight"),
                          kw.get("return_parts", False))
    lr = DDPM(num_timesteps=8, device="cpu", variance_type="learned_range")
    with pytest.raises(ValueError, match="6 channels"):
        lr._check_out(torch.zeros(2, 3, 4, 4), x)
    assert lr._pred_of(torch.arange(2 * 6 * 16.0).view(2, 6, 4, 4), x).shape == x.shape


def test_names_exported_and_declared():
    from diffusion_models_collection_amd import _lib
    header = (Path(__file__).resolve().parent.parent / "include" / "dmc.h").read_text()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint " + name + r"\(", header), name
    assert _lib.LIB.dmc_version() == 1
    assert f"#define DMC_LVAR_COLS {_lib.LVAR_COLS}" in header


def test_models_take_learn_sigma():
    """learn_sigma doubles the final projection and nothing else; False keeps today's keys and shapes."""
    from diffusion_models_collection_amd.models import DiM, DiT
    for cls, kw in ((DiT, dict(num_heads=2)), (DiM, dict(mixer="mamba"))):
        base = dict(img_size=(8, 8), patch_size=2, in_channels=3, hidden_size=32, depth=1, **kw)
        plain, off, on = cls(**base), cls(**base, learn_sigma=False), cls(**base, learn_sigma=True)
        sp, so, sn = plain.state_dict(), off.state_dict(), on.state_dict()
        assert list(sp) == list(so) == list(sn)
        assert all(sp[k].shape == so[k].shape for k in sp)
        assert plain.out_channels == off.out_channels == 3 and on.out_channels == 6
        for k in sp:
            if k.startswith("final_layer.linear."):
                assert sn[k].shape[0] == 2 * sp[k].shape[0] == 2 * 2 * 2 * 3
            else:
                assert sn[k].shape == sp[k].shape
