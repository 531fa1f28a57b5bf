"""Host side of the training objective (diffusion/_objective.py): the min-SNR-gamma weight table against the papers'
forms, argument validation, and the defaults of the public classes. No GPU and no kernel launch."""
import numpy as np
import pytest

import objective_reference as R

SCHEDULES = ("linear", "cosine", "quadratic")
GAMMAS = (1, 5, 20)


def _ac(schedule):
    from diffusion_models_collection_amd.diffusion import _schedule as S
    return S.build_tables(1000, 1e-4, 0.02, schedule)["alphas_cumprod"]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_weight_table_is_the_textbook_form_rounded_once(schedule, gamma):
    """Both prediction types: the division-free closed forms equal min(SNR, g)/SNR and min(SNR, g)/(SNR + 1) computed
    in float64 and rounded to fp32 once, bit for bit; eps weights are exactly 1 wherever SNR <= gamma; all in (0, 1]."""
    from diffusion_models_collection_amd.diffusion import _objective as O
    ac = _ac(schedule)
    assert ac.dtype == np.float32 and ac.shape == (1000,)
    snr = ac.astype(np.float64) / (1.0 - ac.astype(np.float64))
    assert 0 < int((snr > gamma).sum()) < 1000          # both branches of the min are taken
    for ptype in O.PREDICTION_TYPES:
        w = O.min_snr_weights(ac, gamma, ptype)
        assert w.dtype == np.float32 and w.shape == (1000,)
        ref = R.textbook_weights(ac, gamma, ptype).astype(np.float32)
        assert np.array_equal(w.view(np.uint32), ref.view(np.uint32)), (schedule, gamma, ptype)
        assert bool((w > 0).all()) and bool((w <= 1).all())
        if ptype == "eps":
            assert bool((w[snr <= gamma] == 1).all()) and bool((w[snr > gamma] < 1).all())
    if schedule == "linear" and gamma == 5:
        assert int((snr > gamma).sum()) == 130


def test_prediction_types():
    from diffusion_models_collection_amd.diffusion import _objective as O
    assert O.PREDICTION_TYPES == ("eps", "v")


@pytest.mark.parametrize("gamma", [0, -1, 0.0, float("nan"), float("inf"), -float("inf"), None, "5", True, [5]])
def test_bad_gamma(gamma):
    from diffusion_models_collection_amd.diffusion import _objective as O
    with pytest.raises(ValueError):
        O.min_snr_weights(_ac("linear"), gamma, "eps")


def test_bad_prediction_type():
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver, _objective as O
    with pytest.raises(ValueError):
        O.min_snr_weights(_ac("linear"), 5.0, "x0")
    for cls in (DDPM, DDIM, DPMSolver):
        with pytest.raises(ValueError, match="Unknown prediction type"):
            cls(device="cpu", prediction_type="x0")
        d = cls(device="cpu")
        with pytest.raises(ValueError, match="Unknown prediction type"):
            d.set_prediction_type("sample")
        assert d.prediction_type == "eps"


def test_defaults_and_keyword():
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver
    assert DDPM(device="cpu").prediction_type == "eps"
    assert DDIM(device="cpu").prediction_type == "eps"
    assert DPMSolver(device="cpu").prediction_type == "eps"
    for cls in (DDPM, DDIM, DPMSolver):
        d = cls(device="cpu", prediction_type="v")
        assert d.prediction_type == "v"
        d.set_prediction_type("eps")
        assert d.prediction_type == "eps"
    # the keyword trails the reference's positional parameters
    assert DDPM(1000, 0.0001, 0.02, "linear", "cpu").prediction_type == "eps"
    assert DDIM(1000, 50, 0.0001, 0.02, "linear", 0.0, "cpu").prediction_type == "eps"


def test_weight_table_cached_per_gamma_and_type():
    import torch
    from diffusion_models_collection_amd.diffusion import DDPM, _objective as O
    d = DDPM(device="cpu")
    cpu = torch.device("cpu")
    w5 = d._snr_weights(5, cpu)
    assert d._snr_weights(5.0, cpu) is w5
    assert d._snr_weights(1, cpu) is not w5
    d.set_prediction_type("v")
    wv = d._snr_weights(5, cpu)
    assert wv is not w5
    assert np.array_equal(wv.numpy(), O.min_snr_weights(d.alphas_cumprod.numpy(), 5, "v"))
    with pytest.raises(ValueError):
        d._snr_weights(0, cpu)


def test_exports():
    from diffusion_models_collection_amd import _lib
    assert {"dmc_objective", "dmc_pred_convert"} <= set(_lib.EXPORTS)
    assert _lib.LIB.dmc_version() == 1
