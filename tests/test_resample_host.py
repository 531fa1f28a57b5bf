"""diffusion/_resample.py (the host restatement of dmc_ts_history_update / dmc_ts_sample and the samplers' argument
checks) against the independent float64 restatement of tests/resample_reference.py. No GPU."""
import numpy as np
import pytest

import resample_reference as R

F64 = np.float64


def _mod():
    from diffusion_models_collection_amd.diffusion import _resample
    return _resample


def _filled(T, K, seed, rounds=3, scale=None):
    """A ring history after `rounds` * K losses at every timestep (fp32 values), with its counts."""
    g = np.random.default_rng(seed)
    hist = np.zeros((T, K), np.float32)
    count = np.zeros(T, np.int32)
    scale = np.ones(T) if scale is None else scale
    for _ in range(rounds * K):
        t = g.permutation(T)
        R.ring_update(hist, count, t, (np.abs(g.standard_normal(T)) * scale[t]).astype(np.float32))
    return hist, count


def test_warm_up_is_uniform():
    """One row one loss short of K: p = 1/T, iw = 1 and cdf = (i+1)/T exactly; the row's last loss switches it."""
    M = _mod()
    T, K = 7, 3
    hist, count = _filled(T, K, 0, rounds=1)
    count[4] = K - 1
    p, iw, cdf = M.second_moment_weights(hist, count, 0.001)
    assert np.array_equal(p, np.full(T, 1.0 / T)) and np.array_equal(iw, np.ones(T))
    assert np.array_equal(cdf, np.append(np.arange(1, T) / T, 1.0))
    M.history_update(hist, count, [4], [2.0])
    p, iw, _ = M.second_moment_weights(hist, count, 0.001)
    assert count[4] == K and not np.array_equal(p, np.full(T, 1.0 / T)) and not np.array_equal(iw, np.ones(T))
    for c in (np.zeros(T, np.int32), np.full(T, K - 1, np.int32)):
        assert np.array_equal(M.second_moment_weights(hist, c, 0.001)[1], np.ones(T))


@pytest.mark.parametrize("T,K,N", [(5, 3, 17), (12, 10, 40), (9, 1, 9)])
def test_ring_matches_the_shift_left_buffer(T, K, N):
    """A random update sequence with wraparound (and out-of-range t, clamped): once warm, the ring's rows hold the
    shift-left buffer's multisets, the counts tell the same warm state, and p agrees to the summation order of K
    squares."""
    M = _mod()
    g = np.random.default_rng(T * 100 + K)
    buf = R.ShiftBuffer(T, K)
    hist = np.zeros((T, K), np.float32)
    count = np.zeros(T, np.int32)
    was_cold = False
    for step in range(6 * K):
        t = g.integers(-1, T + 1, N)
        losses = (g.standard_normal(N) * 10.0 ** g.integers(-3, 3, N)).astype(np.float32)
        buf.update(t, losses)
        M.history_update(hist, count, t, losses)
        warm = bool((count >= K).all())
        assert warm == buf.warm()
        was_cold |= not warm
        full = count >= K
        assert np.array_equal(np.sort(hist[full], axis=1), np.sort(buf.hist[full].astype(np.float32), axis=1))
        p, iw, cdf = M.second_moment_weights(hist, count, 0.001)
        rp, riw, rcdf = R.weights(buf.hist, buf.warm(), 0.001)
        np.testing.assert_allclose(p, rp, rtol=1e-14, atol=0)
        np.testing.assert_allclose(iw, riw, rtol=1e-14, atol=0)
        np.testing.assert_allclose(cdf, rcdf, rtol=1e-13, atol=0)
    assert warm and was_cold and int(count.max()) > 2 * K


@pytest.mark.parametrize("T,K,up", [(16, 10, 0.001), (1000, 10, 0.001), (7, 3, 0.25), (1, 4, 0.5), (33, 2, 0.0)])
def test_probabilities_and_the_unbiasedness_identity(T, K, up):
    """sum p = 1, p_t >= uniform_prob / T, sum_t p_t iw_t = 1 (the importance-weighted estimator has the uniform draw's
    expectation) and the cdf ends at exactly 1, on a history whose second moments span three decades."""
    M = _mod()
    hist, count = _filled(T, K, T + K, scale=np.logspace(-2, 1, T))
    p, iw, cdf = M.second_moment_weights(hist, count, up)
    assert p.dtype == F64 and abs(p.sum() - 1.0) < 1e-13
    assert bool((p >= np.float32(up) / T * (1 - 1e-12)).all()) and bool((p > 0).all())
    assert abs(float((p * iw).sum()) - 1.0) < 1e-12
    np.testing.assert_allclose(iw, 1.0 / (T * p), rtol=1e-15)
    assert cdf[-1] == 1.0 and bool((np.diff(cdf) >= 0).all())
    rp, riw, rcdf = R.weights(hist, True, up)
    np.testing.assert_allclose(p, rp, rtol=1e-13, atol=0)
    np.testing.assert_allclose(cdf, rcdf, rtol=1e-12, atol=0)
    if T > 1:
        assert p.max() / p.min() > 10
    u = np.array([0.0, np.nextafter(1.0, 0.0), cdf[0], cdf[T // 2]] + list(np.random.default_rng(3).random(50)))
    assert np.array_equal(M.draw(cdf, u), R.draw(cdf, u))


def test_zero_and_non_finite_history_is_uniform():
    """S = 0 (every loss 0), S = inf and S = nan give the uniform p."""
    M = _mod()
    T, K = 6, 2
    count = np.full(T, 5 * K, np.int32)
    for fill in (0.0, np.inf, np.nan, 3e38):      # 3e38 is finite in float64: the one that must NOT be uniform
        hist = np.full((T, K), fill, np.float32)
        hist[0] = 1.0
        if fill == 0.0:
            hist[0] = 0.0
        p, iw, cdf = M.second_moment_weights(hist, count, 0.001)
        uniform = np.array_equal(p, np.full(T, 1.0 / T)) and np.array_equal(iw, np.ones(T))
        assert uniform == (fill != 3e38), fill
        assert cdf[-1] == 1.0


def test_argument_errors():
    M = _mod()
    for k in (0, -1, 2.0, "10", None, True):
        with pytest.raises(ValueError):
            M.check_history_per_term(k)
    assert M.check_history_per_term(1) == 1 and M.check_history_per_term(np.int64(10)) == 10
    for p in (-0.001, 1.0, 1.5, "0.1", None, True, float("nan")):
        with pytest.raises(ValueError):
            M.check_uniform_prob(p)
    assert M.check_uniform_prob(0) == 0.0 and M.check_uniform_prob(0.999) == 0.999
    for name in ("Uniform", "loss_second_moment", "", None):
        with pytest.raises(ValueError):
            M.check_sampler_name(name)
    assert [M.check_sampler_name(n) for n in ("uniform", "loss-second-moment")] == ["uniform", "loss-second-moment"]


def test_samplers_check_their_arguments():
    """The public constructors refuse what _resample refuses, before touching a device."""
    from diffusion_models_collection_amd import diffusion as D

    class Diff:
        num_timesteps = 10
        device = "cuda"

    for bad in (dict(history_per_term=0), dict(uniform_prob=1.0), dict(history_per_term=1.5)):
        with pytest.raises(ValueError):
            D.LossSecondMomentResampler(Diff(), **bad)
    with pytest.raises(ValueError):
        D.create_named_schedule_sampler("importance", Diff())
    s = D.create_named_schedule_sampler("loss-second-moment", Diff())
    assert isinstance(s, D.LossSecondMomentResampler) and (s.history_per_term, s.uniform_prob) == (10, 0.001)
    assert isinstance(D.create_named_schedule_sampler("uniform", Diff()), D.UniformSampler)
