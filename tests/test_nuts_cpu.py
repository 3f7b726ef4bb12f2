"""The NUTS opt-in of sample_GP_NUTS without a GPU: the warm-up schedule, the keyword checks, the keyword-only plumbing,
and the NumPy restatement of the kernel (tests/nuts_restatement.py) checked on an analytic target."""
import inspect
import math

import numpy as np
import pytest


def test_adaptation_schedule_is_stans_windowed_rule():
    from bobe_amd.samplers import adaptation_schedule
    assert adaptation_schedule(256) == [(0, 74), (75, 99), (100, 205), (206, 255)]
    assert adaptation_schedule(512) == [(0, 74), (75, 99), (100, 149), (150, 249), (250, 461), (462, 511)]
    assert adaptation_schedule(100) == [(0, 14), (15, 89), (90, 99)]
    assert adaptation_schedule(10) == [(0, 9)]
    for n in list(range(1, 400)) + [1000, 2048, 5000]:
        s = adaptation_schedule(n)
        assert s[0][0] == 0 and s[-1][1] == n - 1, n
        assert all(b[0] == a[1] + 1 for a, b in zip(s, s[1:])), (n, s)          # no gaps, no overlaps
        assert all(a <= b for a, b in s), (n, s)


def test_window_metric_is_the_regularised_covariance():
    from bobe_amd.samplers import window_metric
    rng = np.random.default_rng(0)
    draws = rng.normal(size=(40, 3)) @ np.array([[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.2, -0.3, 0.7]])
    S = np.cov(draws, rowvar=False)
    want = 40 / 45 * S + 1e-3 * 5 / 45 * np.eye(3)
    assert np.allclose(window_metric(draws), want, rtol=1e-14, atol=1e-16)
    assert np.allclose(window_metric(draws, dense=False), np.diag(np.diag(want)), rtol=1e-14, atol=1e-16)


def test_sampler_keyword_is_checked_before_the_gp_is_used():
    from bobe_amd.samplers import sample_GP_NUTS
    with pytest.raises(ValueError):
        sample_GP_NUTS(None, sampler="bogus")
    with pytest.raises(ValueError):
        sample_GP_NUTS(None, sampler="nuts", device_chains=False)
    with pytest.raises(ValueError):
        sample_GP_NUTS(None, sampler="nuts", fused_trajectories=False)


def test_sampler_choice_is_keyword_only_and_defaults_to_hmc():
    from bobe_amd.acquisition import get_mc_samples
    from bobe_amd.bo import BOBE
    from bobe_amd.samplers import sample_GP_NUTS
    for fn, name in ((get_mc_samples, "sampler"), (BOBE.run, "mc_sampler")):
        p = inspect.signature(fn).parameters[name]
        assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default == "hmc", (fn, name)
    assert inspect.signature(sample_GP_NUTS).parameters["sampler"].default == "hmc"


def test_restatement_samples_a_correlated_gaussian():
    """The yardstick itself: NUTS with a dense metric on a 2-D Gaussian (correlation 0.95) on the logit scale."""
    import nuts_restatement as R
    rho_true = 0.95
    cov = np.array([[1.0, rho_true], [rho_true, 1.0]]) * 0.25
    prec = np.linalg.inv(cov)
    mu = np.array([0.3, -0.2])

    def lpg(u):
        du = u - mu
        return -0.5 * float(du @ prec @ du), -prec @ du, 0.0, u.copy()
    u = mu.copy()
    lp, g, _, _ = lpg(u)
    draws, depths = [], []
    for it in range(3000):
        r = R.transition(lpg, u, g, lp, 0.0, u, cov, 0.6, 6, seed=11, chain=0, iteration=it)
        u, g, lp = r["u"], r["g"], r["logp"]
        draws.append(u)
        depths.append(r["depth"])
        assert not r["diverging"] and r["n_leapfrog"] <= 2 ** r["depth"] - 1
    draws = np.array(draws[200:])
    n = len(draws)
    assert np.all(np.abs(draws.mean(0) - mu) < 5 * 0.5 / math.sqrt(n) * 2)
    assert np.allclose(draws.std(0), 0.5, rtol=0.06)
    assert abs(np.corrcoef(draws.T)[0, 1] - rho_true) < 0.01
    assert 1 <= np.mean(depths) <= 4
