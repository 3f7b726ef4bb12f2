"""No-U-Turn sampling on the device (bobe_gp_nuts_run, sample_GP_NUTS(sampler="nuts")): transitions replayed by the
NumPy restatement (tests/nuts_restatement.py), launch invariance, tree limits, posteriors, gates, ABI errors, BO loop."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.stats import qmc

import nuts_restatement as R

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                    # (BOBE_ERR_ARG, include/bobe_gp.h)


def _state(gp, U, temp):
    lpg = R.gp_target(gp, temp)
    rows = []
    for u in U:
        lp, g, mean, x = lpg(u)
        rows.append(np.concatenate([u, g, x, [lp, mean]]))
    return np.ascontiguousarray(np.array(rows))


def _adapt(P, eps):
    return np.tile(np.array([eps, math.log(10 * eps), 0.0, 0.0, 0.0]), (P, 1))


def _dense_metric(d, rng):
    A = rng.normal(size=(d, d)) / math.sqrt(d)
    S = 0.3 * (A @ A.T) + 0.4 * np.eye(d)
    return 0.5 * (S + S.T)


def test_nuts_transition_replayed_by_the_restatement():
    """One transition of 24 chains at every residency case of k_hmc_run's replay test (registers, + LDS, + streamed),
    with a diagonal and with a dense, non-diagonal metric: tree depth, leapfrog count and divergence equal, acceptance
    statistic to 1e-9, next state to 1e-10.  Then: 5 transitions in one launch == 3 + 2 in two == the first 8 chains."""
    from bobe_amd import GP
    for kernel, d, n in (("rbf", 2, 200), ("matern", 6, 200), ("rbf", 12, 200), ("rbf", 6, 1500), ("matern", 12, 2500),
                         ("rbf", 12, 3000), ("matern", 20, 1500)):
        rng = np.random.default_rng(10 + d)
        X = rng.uniform(size=(n, d))
        y = -15.0 * np.sum((X - 0.5) ** 2, axis=1)
        gp = GP(X, y, noise=1e-6, kernel=kernel, lengthscales=np.linspace(0.4, 0.9, d), kernel_variance=2.0)
        P, temp, eps, depth = 24, 1.0, 0.25, 6
        U0 = rng.normal(scale=0.5, size=(P, d))
        st0 = _state(gp, U0, temp)
        lpg = R.gp_target(gp, temp)
        for metric in (np.diag(rng.uniform(0.5, 2.0, size=d)), _dense_metric(d, rng)):
            st, ad = st0.copy(), _adapt(P, eps)
            _, _, stats, dbg = gp.nuts_run(st, ad, metric, depth, seed=1234, it0=7, niter=1, do_adapt=False, temp=temp,
                                           stats=True, debug=True)
            for c in range(P):
                s0 = st0[c]
                r = R.transition(lpg, s0[:d], s0[d:2 * d], s0[3 * d], s0[3 * d + 1], s0[2 * d:3 * d], metric, eps, depth,
                                 seed=1234, chain=c, iteration=7)
                assert np.allclose(dbg[c], r["p0"], rtol=1e-12, atol=1e-12), (kernel, d, n, c)
                assert stats[0, c, 0] == r["depth"] and stats[0, c, 1] == r["n_leapfrog"], (kernel, d, n, c, stats[0, c], r)
                assert stats[0, c, 2] == float(r["diverging"])
                assert stats[0, c, 3] == pytest.approx(r["accept_prob"], rel=1e-9, abs=1e-14)
                want = np.concatenate([r["u"], r["g"], r["x"], [r["logp"], r["mean"]]])
                assert np.allclose(st[c], want, rtol=1e-10, atol=1e-10), (kernel, d, n, c)
            assert np.array_equal(ad[:, 0], np.full(P, eps))
            assert np.mean(stats[0, :, 0]) >= 2                 # real trees, not single steps
        a, b, c8 = st0.copy(), st0.copy(), st0[:8].copy()
        aa, ab, ac = _adapt(P, eps), _adapt(P, eps), _adapt(8, eps)
        metric = _dense_metric(d, rng)
        gp.nuts_run(a, aa, metric, depth, 99, 0, 5, True, temp)
        gp.nuts_run(b, ab, metric, depth, 99, 0, 3, True, temp)
        gp.nuts_run(b, ab, metric, depth, 99, 3, 2, True, temp)
        gp.nuts_run(c8, ac, metric, depth, 99, 0, 5, True, temp)
        assert np.array_equal(a, b) and np.array_equal(aa, ab) and np.array_equal(a[:8], c8) and np.array_equal(aa[:8], ac)
        assert np.all(aa[:, 4] == 5)


def test_tree_depth_and_leapfrog_limits():
    from bobe_amd import GP
    rng = np.random.default_rng(4)
    d, P = 3, 32
    X = rng.uniform(size=(100, d))
    gp = GP(X, -10.0 * np.sum((X - 0.5) ** 2, axis=1), noise=1e-6, lengthscales=np.full(d, 0.6))
    st0 = _state(gp, rng.normal(scale=0.3, size=(P, d)), 1.0)
    for depth in (1, 6, 10):
        st = st0.copy()
        _, _, stats, _ = gp.nuts_run(st, _adapt(P, 1e-3), np.eye(d), depth, 3, 0, 4, False, stats=True)
        assert np.all(stats[:, :, 0] >= 1) and np.all(stats[:, :, 0] <= depth)
        assert np.all(stats[:, :, 1] <= 2.0 ** stats[:, :, 0] - 1) and np.all(stats[:, :, 1] >= stats[:, :, 0])
        assert np.any(stats[:, :, 0] == depth)                  # (a small step: the trees reach the limit)
        assert np.all(stats[:, :, 2] == 0) and np.all((stats[:, :, 3] > 0) & (stats[:, :, 3] <= 1))


def test_nuts_recovers_gaussian_posteriors():
    from bobe_amd import GP
    from bobe_amd.acquisition import get_mc_samples
    from bobe_amd.bo import gp_fit
    from bobe_amd.samplers import sample_GP_NUTS
    # the 3-D target of test_hmc_on_the_surrogate_recovers_a_gaussian_posterior, with its bounds
    d = 3
    mu, sig = np.array([0.45, 0.55, 0.5]), np.array([0.08, 0.12, 0.1])
    X = qmc.Sobol(d, scramble=True, seed=5).random(512)
    y = -0.5 * np.sum(((X - mu) / sig) ** 2, axis=1)
    gp = GP(X, y, noise=1e-8, lengthscales=[0.5] * d, kernel_variance=10.0)
    gp_fit(gp, maxiters=100, n_restarts=2, rng=np.random.default_rng(0))
    diag = {}
    s = sample_GP_NUTS(gp, np_rng=np.random.default_rng(1), num_chains=4, sampler="nuts", diagnostics=diag)
    assert set(s) == {"x", "logp", "best", "method"} and s["method"] == "MCMC"
    assert s["x"].shape == (4 * 1024 // 4, d) and s["logp"].shape == (1024,)
    assert np.all(s["x"] > 0) and np.all(s["x"] < 1)
    assert np.all(np.abs(s["x"].mean(0) - mu) < 0.02)
    assert np.all(np.abs(s["x"].std(0) / sig - 1.0) < 0.2)
    assert np.all(np.abs(s["best"] - mu) < 0.06)
    assert np.allclose(s["logp"][:50], gp.predict_mean_batched(s["x"][:50]), atol=1e-6)
    assert np.all(diag["stats"][:, :, 0] <= 6) and np.mean(diag["stats"][:, :, 3]) > 0.6
    s4 = sample_GP_NUTS(gp, np_rng=np.random.default_rng(2), num_chains=2, temp=4.0, num_samples=512, sampler="nuts")
    assert s4["x"].shape[0] == 2 * 512 // 4
    assert np.all(s4["x"].std(0) > 1.5 * sig)
    mc = get_mc_samples(gp, warmup_steps=128, num_samples=256, thinning=4, method="NUTS", num_chains=4,
                        np_rng=np.random.default_rng(3), sampler="nuts")
    assert mc["x"].shape == (256, d)
    # 6-D, correlation 0.9 between every pair: the dense metric
    d = 6
    mu6, sd, rho = np.full(d, 0.5), 0.06, 0.9
    cov = sd ** 2 * ((1 - rho) * np.eye(d) + rho * np.ones((d, d)))
    prec = np.linalg.inv(cov)
    X = qmc.Sobol(d, scramble=True, seed=6).random(2048)      # (1024 points fit this thin target badly: both samplers miss)
    dx = X - mu6
    y = -0.5 * np.einsum("ni,ij,nj->n", dx, prec, dx)
    gp6 = GP(X, y, noise=1e-8, lengthscales=[0.5] * d, kernel_variance=10.0)
    gp_fit(gp6, maxiters=100, n_restarts=2, rng=np.random.default_rng(0))
    s6 = sample_GP_NUTS(gp6, np_rng=np.random.default_rng(7), num_chains=4, sampler="nuts")
    x6 = s6["x"]
    assert np.all(np.abs(x6.mean(0) - mu6) < 0.02)
    assert np.all(np.abs(x6.std(0) / sd - 1.0) < 0.2)
    corr = np.corrcoef(x6.T)[np.triu_indices(d, 1)]
    assert np.all(np.abs(corr - rho) < 0.05), corr


@pytest.mark.parametrize("clf_type", ["svm", "ellipsoid"])
def test_gated_nuts_never_returns_an_infeasible_sample(clf_type):
    from bobe_amd.clf_gp import GPwithClassifier
    from bobe_amd.samplers import sample_GP_NUTS
    rng = np.random.default_rng(5)
    d = 2
    X = rng.uniform(size=(200, d))
    y = -800.0 * np.sum((X - np.array([0.45, 0.55])) ** 2, axis=1)
    kw = {} if clf_type == "svm" else {"clf_type": "ellipsoid"}
    gp = GPwithClassifier(X, y, clf_threshold=40.0, gp_threshold=120.0, noise=1e-6, lengthscales=np.full(d, 0.3), **kw)
    assert gp.use_clf and gp.minus_inf == -1e5
    s = sample_GP_NUTS(gp, np_rng=np.random.default_rng(1), num_chains=4, warmup_steps=200, num_samples=800, thinning=2,
                       sampler="nuts")
    assert np.all(s["logp"] > gp.minus_inf) and np.all(gp.predict_mean_batched(s["x"]) > gp.minus_inf)
    # at the default minus_inf a gated leaf is divergent: start every chain next to the region's edge, aimed outwards
    P = 32
    x0 = np.tile(np.array([0.45, 0.55]), (P, 1)) + rng.normal(scale=0.05, size=(P, d))
    st = _state(gp, np.log(x0) - np.log1p(-x0), 1.0)
    assert np.all(st[:, 2 * d + 1] > gp.minus_inf)
    _, _, stats, _ = gp.nuts_run(st, _adapt(P, 0.3), np.eye(d) * 4.0, 8, 5, 0, 6, False, stats=True)
    assert np.any(stats[:, :, 2] == 1)
    assert np.all(st[:, 2 * d + 1] > gp.minus_inf)
    # the divergent flag is the restatement's (gated leaves have mean minus_inf)
    st1 = _state(gp, np.log(x0) - np.log1p(-x0), 1.0)
    _, _, stats1, _ = gp.nuts_run(st1.copy(), _adapt(P, 0.3), np.eye(d) * 4.0, 8, 5, 0, 1, False, stats=True)
    lpg = R.gp_target(gp, 1.0)
    for c in range(P):
        s0 = st1[c]
        r = R.transition(lpg, s0[:d], s0[d:2 * d], s0[3 * d], s0[3 * d + 1], s0[2 * d:3 * d], np.eye(d) * 4.0, 0.3, 8,
                         seed=5, chain=c, iteration=0)
        assert stats1[0, c, 2] == float(r["diverging"]) and stats1[0, c, 1] == r["n_leapfrog"]


def test_nuts_abi_refuses_bad_arguments():
    import torch
    from bobe_amd import GP
    rng = np.random.default_rng(0)
    d, P = 3, 4
    X = rng.uniform(size=(50, d))
    gp = GP(X, -np.sum((X - 0.5) ** 2, axis=1), noise=1e-6, lengthscales=np.full(d, 0.7))
    st = _state(gp, rng.normal(size=(P, d)), 1.0)
    ad = _adapt(P, 0.1)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(metric, depth, state_ptr=None):
        return gp._lib.bobe_gp_nuts_run(gp._h, P, state_ptr or p(st), p(ad), p(np.ascontiguousarray(metric)), depth, 1, 0, 1,
                                        0, 1.0, 0.0, 1.0, 0, None, 1, None, None, None)
    assert call(np.eye(d), 6) == 0
    for depth in (0, 11):
        assert call(np.eye(d), depth) == ERR_ARG
    not_pd = np.eye(d)
    not_pd[2, 2] = -1.0
    asym = np.eye(d)
    asym[0, 1] = 0.3
    for m in (not_pd, asym, np.zeros((d, d))):
        assert call(m, 6) == ERR_ARG
    dev = torch.from_numpy(st).cuda()
    assert call(np.eye(d), 6, C.c_void_p(dev.data_ptr())) == ERR_ARG
    assert call(np.eye(d), 6) == 0                              # (the handle still works)


def test_bo_loop_with_nuts_integration_points():
    from bobe_amd.bo import BOBE
    sig = 0.2
    bounds = np.array([[0.0, 1.0], [0.0, 1.0]]).T
    bobe = BOBE(lambda x: -0.5 * float(np.sum(((x - 0.5) / sig) ** 2)), ["a", "b"], bounds, n_sobol_init=16, seed=5, save=False)
    res = bobe.run(acq="wipstd", max_evals=80, fit_n_points=4, batch_size=2, mc_points_size=64, mc_points_method="NUTS",
                   logz_threshold=0.05, min_evals=24, ns_n_points=8, mc_sampler="nuts")
    assert "logz" in res and res["logz"]["mean"] == pytest.approx(2 * 0.5 * math.log(2 * math.pi * sig ** 2), abs=0.25)
    assert res["n_evals"] <= 80
