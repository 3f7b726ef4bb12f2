"""The evidence draws of ``samplers.logz_from_samples`` (n_draws > 0) on a NumPy stand-in for the GP, and the NumPy replay of
the device's normals (bobe_gp_posterior_sample with z = NULL).  No GPU: the stub draws from a covariance it is given."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from posterior_restatement import device_normals, mix64, u01  # noqa: E402

from bobe_amd import samplers  # noqa: E402
from bobe_amd.samplers import compute_integrals, logz_from_samples  # noqa: E402


class StubGP:
    """``predict_var_batched`` and ``sample_posterior(centered=True)`` of a GP whose joint posterior covariance at any set
    of points x is F F^T, F = ``factor_fn(x)``; records the points it was asked for."""

    def __init__(self, factor_fn, var=1e-2, minus_inf=None):
        self.factor_fn, self.var, self.asked = factor_fn, var, []
        if minus_inf is not None:
            self.minus_inf = minus_inf

    def predict_var_batched(self, x):
        return np.full(len(x), self.var)

    def sample_posterior(self, x, n_samples=1, seed=0, z=None, centered=False, return_jitter=False):
        assert centered
        x = np.asarray(x)
        self.asked.append(x.copy())
        F = self.factor_fn(x)
        z = np.random.default_rng(seed).standard_normal((n_samples, F.shape[1])) if z is None else z
        d = z @ F.T
        return (d, 0.0) if return_jitter else d


def _run(n=400, seed=0):
    """A nested-sampling-like run: samples in the unit square, logl rising with the shells, logvol of 100 live points."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, 2))
    logl = np.sort(-20.0 * np.sum((x - 0.5) ** 2, axis=1) + 0.01 * rng.standard_normal(n))
    logvol = -np.arange(1, n + 1) / 100.0
    mean = float(compute_integrals(logl=logl, logvol=logvol)[-1])
    return x, logl, logvol, mean


def test_zero_covariance_draws_are_the_mean():
    x, logl, logvol, mean = _run()
    gp = StubGP(lambda q: np.zeros((len(q), 1)))
    out = logz_from_samples(gp, x, logl, logvol, mean, 0.1, n_draws=16, draws_seed=3)
    assert out["draws"].shape == (16,)
    assert np.all(out["draws"] == mean)
    assert out["draws_std"] == 0.0 and out["draws_mean"] == mean
    assert out["draws_points"] == len(logl) and out["draws_jitter"] == 0.0


def test_rank_one_shift_moves_logz_by_the_shift():
    x, logl, logvol, mean = _run()
    gp = StubGP(lambda q: math.sqrt(0.3) * np.ones((len(q), 1)))
    n_draws = 8
    out = logz_from_samples(gp, x, logl, logvol, mean, 0.1, n_draws=n_draws, draws_seed=11)
    # covariance 0.3 * 1 1^T: every point of draw s is shifted by the same c_s
    delta = gp.sample_posterior(x, n_samples=n_draws, seed=11, centered=True)
    c = delta[:, 0]
    assert np.all(delta == c[:, None])
    np.testing.assert_allclose(out["draws"], mean + c, rtol=0, atol=1e-12 * (1 + abs(mean)))
    assert out["draws_std"] > 0


def test_gated_and_non_finite_points_are_held_fixed():
    x, logl, logvol, mean = _run()
    logl = logl.copy()
    gated = np.array([3, 10, 50])
    logl[gated] = -1e5
    logl[[7, 20]] = [-np.inf, np.nan]
    gp = StubGP(lambda q: np.eye(len(q)), minus_inf=-1e5)
    with np.errstate(invalid="ignore"):                 # (the NaN sample makes the integrals NaN; only the selection counts)
        out = logz_from_samples(gp, x, logl, logvol, mean, 0.1, n_draws=4, draws_seed=1)
    held = np.r_[gated, 7, 20]
    free = np.setdiff1d(np.arange(len(logl)), held)
    assert out["draws_points"] == len(free)
    np.testing.assert_array_equal(gp.asked[0], x[free])
    idx = samplers.draws_points(gp, logl, logvol)
    np.testing.assert_array_equal(idx, free)


def test_max_points_follow_the_weights():
    x, logl, logvol, mean = _run(n=600, seed=2)
    gp = StubGP(lambda q: 1e-2 * np.eye(len(q)))
    k = 50
    out = logz_from_samples(gp, x, logl, logvol, mean, 0.1, n_draws=3, draws_seed=5, draws_max_points=k)
    assert out["draws_points"] == k
    pad = np.concatenate([[-1e300], logl])
    dv = np.diff(logvol, prepend=0)
    logwt = np.logaddexp(pad[1:], pad[:-1]) + (logvol - dv + np.log1p(-np.exp(dv))) + math.log(0.5)
    top = np.sort(np.argsort(-logwt, kind="stable")[:k])
    np.testing.assert_array_equal(gp.asked[0], x[top])
    assert np.min(logwt[top]) >= np.max(np.delete(logwt, top))


def test_existing_keys_do_not_change_with_draws():
    x, logl, logvol, mean = _run()
    gp = StubGP(lambda q: 0.2 * np.eye(len(q)))
    plain = logz_from_samples(gp, x, logl, logvol, mean, 0.1)
    with_draws = logz_from_samples(gp, x, logl, logvol, mean, 0.1, n_draws=32, draws_seed=9)
    assert set(plain) == {"mean", "dlogz_sampler", "upper", "lower", "var", "std"}
    assert set(with_draws) == set(plain) | {"draws", "draws_mean", "draws_std", "draws_points", "draws_jitter"}
    for k, v in plain.items():
        assert np.array_equal(np.asarray(with_draws[k]), np.asarray(v)), k


def test_draw_keywords_are_keyword_only():
    import inspect
    sig = inspect.signature(logz_from_samples)
    for k in ("n_draws", "draws_seed", "draws_max_points"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(samplers.nested_sampling_Dy)
    for k in ("logz_draws", "logz_draws_seed"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["logz_draws"].default == 0
    assert inspect.signature(samplers.nested_sampling).parameters["logz_draws"].default == 0


def test_hash_replay_known_values_and_moments():
    # splitmix64's published first outputs for the state sequence 0x9E3779B97F4A7C15 * k (seed 0): mix64(k * golden)
    golden = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        firsts = mix64(np.arange(3, dtype=np.uint64) * golden)
    assert [int(v) for v in firsts] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert 0.0 < u01(np.uint64(0)) < u01(np.uint64(2 ** 64 - 1)) <= 1.0       # (u1 > 0: log u1 is finite)
    z = device_normals(12345, 1000, 1000).ravel()                 # 10^6 values
    n = z.size
    assert np.all(np.isfinite(z))
    assert abs(np.mean(z)) < 6.0 / math.sqrt(n)
    assert abs(np.var(z) - 1.0) < 6.0 * math.sqrt(2.0 / n)
    assert abs(np.mean(z ** 3)) < 6.0 * math.sqrt(15.0 / n)
    assert abs(np.mean(z ** 4) - 3.0) < 6.0 * math.sqrt(96.0 / n)
    # a draw's normals depend on (seed, s, c) only, and seeds / rows are not correlated
    np.testing.assert_array_equal(device_normals(12345, 10, 7, s0=990), device_normals(12345, 1000, 1000)[990:, :7])
    a, b = device_normals(1, 1, 20000).ravel(), device_normals(2, 1, 20000).ravel()
    assert abs(np.corrcoef(a, b)[0, 1]) < 6.0 / math.sqrt(20000)
