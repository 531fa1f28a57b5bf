"""img2img / inpaint host side (diffusion/_edit.py) without a GPU: the start index, the walk, the blend coefficient
table against the float64 restatement in tests/edit_reference.py, and every input builder and reference of
tests/test_gpu_edit.py."""
import numpy as np
import pytest

import edit_reference as E


def _edit():
    from diffusion_models_collection_amd.diffusion import _edit
    return _edit


def _ac():
    from diffusion_models_collection_amd.diffusion import _schedule as S
    return S.build_tables(1000, 1e-4, 0.02, "linear")["alphas_cumprod"]


def _lists():
    """The three timestep lists the samplers walk on the linear T = 1000 table: DDIM-50, DPM-20, DDPM-1000."""
    from diffusion_models_collection_amd.diffusion import _dpm, _schedule
    return {"ddim50": _schedule.ddim_timesteps(1000, 50), "dpm20": _dpm.dpm_timesteps(1000, 20, "logsnr", _ac()),
            "ddpm1000": np.arange(999, -1, -1, dtype=np.int64)}


@pytest.mark.parametrize("S", [1, 20, 50])
def test_start_index(S):
    """0.024 * 20 + 0.5 = 0.98 and 0.025 * 20 + 0.5 = 1.0 sit on either side of the first integer; 0.975 * 20 + 0.5 =
    20 on the last."""
    for strength in (1e-9, 0.024, 0.025, 0.5, 0.975, 1.0):
        i0 = _edit().start_index(S, strength)
        assert isinstance(i0, int) and i0 == E.ref_start_index(S, strength) and 0 <= i0 <= S - 1
    assert _edit().start_index(S, 1.0) == 0 and _edit().start_index(S, 1e-9) == S - 1
    if S == 50:
        assert [_edit().start_index(S, s) for s in (0.024, 0.025, 0.5, 0.975)] == [49, 49, 25, 1]
    for bad in (0, 0.0, -0.1, -1, 1.0000001, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _edit().start_index(S, bad)


def test_edit_walk():
    for S, i0, U in ((1, 0, 1), (5, 0, 1), (5, 2, 3), (50, 25, 2), (12, 0, 4)):
        walk = _edit().edit_walk(S, i0, U)
        assert walk == E.ref_walk(S, i0, U) and len(walk) == (S - i0) * U
        assert [i for i, _ in walk] == [i for i in range(i0, S) for _ in range(U)]
        for k, (i, renoise) in enumerate(walk):
            assert renoise == (0 if k % U == U - 1 else 1)      # every repetition but a step's last re-noises
        if U == 1:
            assert not any(r for _, r in walk)
    for bad in (0, -1, 1.5, "2", None, True):
        with pytest.raises((ValueError, TypeError)):
            _edit().edit_walk(5, 0, bad)
    for i0 in (-1, 5):
        with pytest.raises(ValueError):
            _edit().edit_walk(5, i0, 1)


@pytest.mark.parametrize("name", ["ddim50", "dpm20", "ddpm1000"])
def test_blend_coefficients(name):
    """Bitwise the float64 restatement rounded once. ka^2 + kb^2 and ra^2 + rb^2: each entry is within 2^-24 relative
    of its float64 value, so each sum of squares is within 2 * 2^-24 = one fp32 ulp of 1 to first order; 2 are
    allowed."""
    ac, ts = _ac(), _lists()[name]
    S = len(ts)
    c = _edit().blend_coefficients(ac, ts)
    assert c.shape == (2 * S, 4) and c.dtype == np.float32 and c.flags["C_CONTIGUOUS"]
    assert np.array_equal(c.view(np.int32), E.ref_blend_coefficients(ac, ts).astype(np.float32).view(np.int32))
    assert c[2 * S - 2, :2].tolist() == [1.0, 0.0] and c[2 * S - 1, :2].tolist() == [1.0, 0.0]
    assert bool((c[0::2, 2] == 1).all()) and bool((c[0::2, 3] == 0).all())
    assert bool((c[: 2 * S - 2, 1] > 0).all()) and bool((c[1::2, 3] > 0).all()) and bool((c[1::2, 2] < 1).all())
    assert np.array_equal(c[0::2, :2], c[1::2, :2])
    d = c.astype(np.float64)
    ulp = 2.0 ** -23
    assert float(np.abs(d[:, 0] ** 2 + d[:, 1] ** 2 - 1).max()) <= 2 * ulp
    assert float(np.abs(d[:, 2] ** 2 + d[:, 3] ** 2 - 1).max()) <= 2 * ulp
    # the re-noise row composes with the known row to the direct noising to t_i: ra * ka = sqrt(a_ti)
    a = ac[ts].astype(np.float64)
    assert float(np.abs(d[1::2, 2] * d[1::2, 0] - np.sqrt(a)).max()) <= 2 * ulp
    with pytest.raises(ValueError):
        _edit().blend_coefficients(ac, [])


def test_blend_coefficients_refuse_a_rising_list():
    with pytest.raises(ValueError):
        _edit().blend_coefficients(_ac(), [0, 999])           # a_ti / a_tn > 1: no forward jump


def test_samplers_carry_the_entry_points():
    from diffusion_models_collection_amd.diffusion import DDIM, DDPM, DPMSolver
    for smp in (DDPM(num_timesteps=12, device="cpu"), DDIM(1000, 50, device="cpu"), DPMSolver(1000, 20, device="cpu")):
        assert callable(smp.img2img) and callable(smp.inpaint)
        host, devc = smp._blend_table(np.arange(11, -1, -1), smp.alphas_cumprod.device)
        assert host.shape == (24, 4) and np.array_equal(devc.numpy(), host)
        assert smp._blend_table(np.arange(11, -1, -1), smp.alphas_cumprod.device)[1] is devc
    assert callable(DDIM.invert)
    with pytest.raises(NotImplementedError):
        DPMSolver(1000, 20, device="cpu").invert(None, None)
    import inspect
    assert inspect.signature(DDIM.sample).parameters["clip_denoised"].default is True
    for cls in (DDPM, DDIM, DPMSolver):
        p = inspect.signature(cls.inpaint).parameters
        assert p["resample"].default == 1 and p["cfg_scale"].default is None and p["p_threshold"].default == 0.995
        assert inspect.signature(cls.img2img).parameters["strength"].default == 0.5


def test_gpu_file_references_run_on_the_cpu():
    import test_gpu_edit
    assert test_gpu_edit.cpu_selfcheck() > 0
