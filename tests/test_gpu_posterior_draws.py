"""The joint posterior of the surrogate on the device: bobe_gp_predict_cov / GP.predict_cov against a dense restatement,
scikit-learn and the extended-precision truth of the conditioning ladder, and bobe_gp_posterior_sample / GP.sample_posterior
(caller and device normals, statistics, jitter, errors, memory), and the evidence draws of nested sampling end to end."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
from scipy.linalg import solve_triangular
from scipy.stats import qmc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from posterior_restatement import dense_cov, device_normals  # noqa: E402

pytestmark = pytest.mark.gpu


def _gp(n, d, kernel="rbf", noise=1e-4, kvar=1.3, seed=0, ls=None):
    from bobe_amd import GP
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, -1]) + 0.1 * rng.standard_normal(n)
    ls = np.full(d, 0.3 * math.sqrt(d)) if ls is None else np.asarray(ls, dtype=float)
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar), X, ls


CASES = [(n, c, k, d) for (n, c) in [(1, 1), (50, 7), (600, 300), (2000, 2500)] for k in ("rbf", "matern") for d in (2, 8, 32)]


@pytest.mark.parametrize("n,c,kernel,d", CASES, ids=[f"N{n}_C{c}_{k}_d{d}" for n, c, k, d in CASES])
def test_predict_cov_dense_restatement(n, c, kernel, d):
    gp, X, ls = _gp(n, d, kernel, seed=n + d)
    Q = np.random.default_rng(7 + c).uniform(size=(c, d))
    scale = gp.kernel_variance + gp.noise
    S = gp.predict_cov(Q) / gp.y_std ** 2
    R = dense_cov(kernel, X, Q, ls, gp.kernel_variance, gp.noise)
    assert S.shape == (c, c)
    assert np.array_equal(S, S.T)                                          # the mirror is exact
    assert np.max(np.abs(S - R)) <= 1e-10 * scale, np.max(np.abs(S - R))
    # the diagonal is bobe_gp_predict's variance (before its clip: compare where the clip does not act)
    _, var = gp._predict(Q, False, True, 0)
    dg = np.diag(S)
    np.testing.assert_allclose(np.maximum(dg, 1e-12), var, rtol=0, atol=1e-12 * scale)
    # the plain product (kappa < 0) and the forced substitution (kappa = 0) agree
    gp.refine_kappa = -1.0
    gp.recompute_cholesky()
    assert not gp.refining
    S_plain = gp.predict_cov(Q) / gp.y_std ** 2
    gp.refine_kappa = 0.0
    gp.recompute_cholesky()
    assert gp.refining
    S_sub = gp.predict_cov(Q) / gp.y_std ** 2
    assert np.array_equal(S_sub, S_sub.T)
    assert np.max(np.abs(S_plain - S_sub)) <= 1e-10 * scale
    assert np.max(np.abs(S_sub - R)) <= 1e-10 * scale


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_predict_cov_equals_scikit_learn(kernel):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern
    d = 3
    gp, X, ls = _gp(300, d, kernel, noise=1e-4, kvar=2.0, seed=4)
    Q = np.random.default_rng(5).uniform(size=(120, d))
    base = RBF(length_scale=ls) if kernel == "rbf" else Matern(length_scale=ls, nu=2.5)
    sk = GaussianProcessRegressor(ConstantKernel(gp.kernel_variance) * base, alpha=gp.noise, optimizer=None,
                                  normalize_y=False)
    sk.fit(X, np.asarray(gp.train_y).reshape(-1))
    _, cov = sk.predict(Q, return_cov=True)
    S = gp.predict_cov(Q) / gp.y_std ** 2
    np.testing.assert_allclose(S, cov + gp.noise * np.eye(len(Q)), rtol=0, atol=1e-9 * (gp.kernel_variance + gp.noise))


@pytest.mark.parametrize("rung", range(9))
def test_predict_cov_diagonal_on_the_conditioning_ladder(rung):
    from conditioning_common import LADDER, NOISE, TOL, _bo_like_design, _err, _floored, ladder_points
    from bobe_amd import GP
    from oracle import bobe_oracle as O
    from oracle import c_binding as CB
    n, kernel, ls, kvar = LADDER[rung]
    ls = np.array(ls)
    X, y, spare = _bo_like_design(n)
    cand, _ = ladder_points(X, spare, rung)
    og = O.OracleGP(X, y, noise=NOISE, kernel=kernel, lengthscales=ls, kernel_variance=kvar)
    ys = np.asarray(og.train_y).reshape(-1)
    tr = CB.gp_truth(0 if kernel == "rbf" else 1, X, ys, ls, kvar, NOISE, cand, None, want_grad=False)
    assert tr["info"] == 0
    truth = _floored(tr["var"])
    gp = GP(X, y, noise=NOISE, kernel=kernel, lengthscales=ls, kernel_variance=kvar)
    gp.pivot_floor_ulp = 0.0
    gp.recompute_cholesky()
    assert not gp.not_pd
    S = gp.predict_cov(cand) / gp.y_std ** 2
    hip = _err(_floored(np.diag(S)), truth, kvar + NOISE)
    _, var = gp._predict(cand, False, True, 0)
    hip_var = _err(var, truth, kvar + NOISE)
    # the diagonal and bobe_gp_predict's variance come from the same V: the same error to rounding
    assert _err(_floored(np.diag(S)), var, kvar + NOISE) <= 1e-12
    if np.all(np.isfinite(og.cholesky)):            # (where LAPACK's factorisation fails there is no bound to meet)
        vc = solve_triangular(og.cholesky, og._k12(cand), lower=True, check_finite=False)
        lap = _err(_floored(kvar + NOISE - np.sum(vc * vc, axis=0)), truth, kvar + NOISE)
        assert hip <= 4.0 * lap + TOL["var"], (hip, lap, hip_var)


def _mean_std(gp, Q):
    m, _ = gp._predict(Q, True, False, 0)
    return m


def test_draws_with_caller_normals_are_m_plus_chol_sigma_z():
    gp, X, _ = _gp(400, 4, "matern", seed=3)
    Q = np.random.default_rng(1).uniform(size=(150, 4))
    S = gp.predict_cov(Q) / gp.y_std ** 2
    m = _mean_std(gp, Q)
    z = np.random.default_rng(2).standard_normal((20, 150))
    draws, jit = gp.sample_posterior(Q, n_samples=20, z=z, return_jitter=True)
    ref = m + z @ np.linalg.cholesky(S).T
    assert jit == 0.0
    np.testing.assert_allclose((draws - gp.y_mean) / gp.y_std, ref, rtol=0, atol=1e-10 * (1 + np.max(np.abs(ref))))
    cen = gp.sample_posterior(Q, n_samples=20, z=z, centered=True)
    np.testing.assert_allclose(cen / gp.y_std, ref - m, rtol=0, atol=1e-10 * (1 + np.max(np.abs(ref))))


def test_device_normals_replay_and_determinism():
    import torch
    gp, X, _ = _gp(300, 3, seed=9)
    Q = np.random.default_rng(4).uniform(size=(200, 3))
    S_, C_ = 33, len(Q)
    a = gp.sample_posterior(Q, n_samples=S_, seed=2024, centered=True)
    b = gp.sample_posterior(Q, n_samples=S_, seed=2024, centered=True)
    assert np.array_equal(a, b)
    z = device_normals(2024, S_, C_)
    c = gp.sample_posterior(Q, n_samples=S_, z=z, centered=True)
    np.testing.assert_allclose(a, c, rtol=0, atol=1e-13 * gp.y_std * max(1.0, np.max(np.abs(c)) / gp.y_std))
    assert not np.array_equal(a, gp.sample_posterior(Q, n_samples=S_, seed=2025, centered=True))
    # host and device pointers give the same bits
    lib, h = gp._lib, gp._h
    xq = np.ascontiguousarray(Q)
    out_h = np.empty((S_, C_))
    jit = C.c_double(-1.0)
    assert lib.bobe_gp_posterior_sample(h, xq.ctypes.data, C_, S_, 2024, None, 0, out_h.ctypes.data, C.byref(jit)) == 0
    xd = torch.tensor(Q, dtype=torch.float64, device="cuda")
    out_d = torch.empty((S_, C_), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert lib.bobe_gp_posterior_sample(h, xd.data_ptr(), C_, S_, 2024, None, 0, out_d.data_ptr(), None) == 0
    lib.bobe_gp_sync(h)
    assert np.array_equal(out_h, out_d.cpu().numpy())
    assert np.array_equal(gp.y_mean + gp.y_std * out_h, gp.sample_posterior(Q, n_samples=S_, seed=2024))
    # a device covariance equals the host one
    cov_d = torch.empty((C_, C_), dtype=torch.float64, device="cuda")
    assert lib.bobe_gp_predict_cov(h, xd.data_ptr(), C_, cov_d.data_ptr()) == 0
    lib.bobe_gp_sync(h)
    assert np.array_equal(cov_d.cpu().numpy() * gp.y_std ** 2, gp.predict_cov(Q))


def test_draw_statistics():
    gp, X, _ = _gp(40, 2, seed=5, noise=1e-3)
    Q = np.random.default_rng(6).uniform(size=(6, 2))
    S = gp.predict_cov(Q) / gp.y_std ** 2
    m = _mean_std(gp, Q)
    n = 200000
    dr = (gp.sample_posterior(Q, n_samples=n, seed=77) - gp.y_mean) / gp.y_std
    sd = np.sqrt(np.diag(S))
    assert np.all(np.abs(dr.mean(0) - m) <= 6 * sd / math.sqrt(n))
    emp = np.cov(dr, rowvar=False)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / n)
    assert np.all(np.abs(emp - S) <= 6 * se)


def test_duplicated_queries_take_a_jitter():
    from bobe_amd import GP
    rng = np.random.default_rng(8)
    X = rng.uniform(size=(12, 2))
    gp = GP(X, np.sin(4 * X[:, 0]), noise=1e-300, lengthscales=[0.1, 0.1], kernel_variance=1.0)
    assert not gp.not_pd
    Q = np.repeat(rng.uniform(size=(3, 2)), 60, axis=0)
    draws, jit = gp.sample_posterior(Q, n_samples=5, seed=1, return_jitter=True)
    S = gp.predict_cov(Q) / gp.y_std ** 2
    assert jit > 0 and min(abs(jit / np.mean(np.diag(S)) / t - 1.0) for t in (1e-12, 1e-10, 1e-8, 1e-6)) < 1e-12
    assert np.all(np.isfinite(draws))
    # the duplicated rows draw the same value up to the jitter
    d = (draws - gp.y_mean) / gp.y_std
    assert np.max(np.abs(d[:, 0:60] - d[:, [0]])) <= 1e-3


def test_error_contract():
    from bobe_amd import GP, _lib
    lib = _lib.load()
    xq = np.random.default_rng(0).uniform(size=(10, 2))
    out = np.empty((10, 10))
    dr = np.empty((4, 10))
    # no factorised state
    h = C.c_void_p(0)
    assert lib.bobe_gp_create(C.byref(h), 0, 0, 2) == 0
    try:
        assert lib.bobe_gp_predict_cov(h, xq.ctypes.data, 10, out.ctypes.data) == -3
        assert lib.bobe_gp_posterior_sample(h, xq.ctypes.data, 10, 4, 0, None, 0, dr.ctypes.data, None) == -3
    finally:
        lib.bobe_gp_destroy(h)
    gp, X, _ = _gp(30, 2, seed=1)
    g = gp._h
    for c in (0, -1, 16385):
        assert lib.bobe_gp_predict_cov(g, xq.ctypes.data, c, out.ctypes.data) == -1
        assert lib.bobe_gp_posterior_sample(g, xq.ctypes.data, c, 4, 0, None, 0, dr.ctypes.data, None) == -1
    assert lib.bobe_gp_posterior_sample(g, xq.ctypes.data, 10, 0, 0, None, 0, dr.ctypes.data, None) == -1
    assert lib.bobe_gp_predict_cov(g, xq.ctypes.data, 10, None) == -1
    assert lib.bobe_gp_posterior_sample(g, xq.ctypes.data, 10, 4, 0, None, 0, None, None) == -1
    assert lib.bobe_gp_predict_cov(g, None, 10, out.ctypes.data) == -1
    # a NaN factor: duplicated training points without noise
    Xd = np.vstack([X[:5], X[:5]])
    bad = GP(Xd, np.arange(10.0), noise=0.0, lengthscales=[0.3, 0.3], kernel_variance=1.0, pivot_floor_ulp=64)
    assert bad.not_pd
    assert lib.bobe_gp_predict_cov(bad._h, xq.ctypes.data, 10, out.ctypes.data) == _lib.BOBE_NOT_PD
    assert np.all(np.isnan(out))
    jit = C.c_double(0.0)
    assert lib.bobe_gp_posterior_sample(bad._h, xq.ctypes.data, 10, 4, 0, None, 0, dr.ctypes.data,
                                        C.byref(jit)) == _lib.BOBE_NOT_PD
    assert np.all(np.isnan(dr)) and math.isnan(jit.value)
    assert np.all(np.isnan(bad.predict_cov(xq))) and np.all(np.isnan(bad.sample_posterior(xq, 2)))
    # the handle's own state is untouched by the calls: its predictions are the same bits as before
    m0, v0 = gp._predict(xq, True, True, 0)
    gp.predict_cov(np.random.default_rng(3).uniform(size=(500, 2)))
    gp.sample_posterior(np.random.default_rng(3).uniform(size=(500, 2)), n_samples=3)
    m1, v1 = gp._predict(xq, True, True, 0)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


def test_device_memory_is_returned():
    import torch
    from bobe_amd import _lib
    lib = _lib.load()
    gp, X, _ = _gp(500, 3, seed=2)
    c = 16384
    xd = torch.tensor(np.random.default_rng(9).uniform(size=(c, 3)), dtype=torch.float64, device="cuda")
    dr = torch.empty((4, c), dtype=torch.float64, device="cuda")
    cov = torch.empty((c, c), dtype=torch.float64, device="cuda")
    # (a first small call loads the kernels' code objects)
    assert lib.bobe_gp_posterior_sample(gp._h, xd.data_ptr(), 256, 4, 1, None, 0, dr.data_ptr(), None) == 0
    assert lib.bobe_gp_predict_cov(gp._h, xd.data_ptr(), 256, cov.data_ptr()) == 0
    lib.bobe_gp_sync(gp._h)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    jit = C.c_double(-1.0)
    assert lib.bobe_gp_posterior_sample(gp._h, xd.data_ptr(), c, 4, 1, None, 0, dr.data_ptr(), C.byref(jit)) == 0
    assert lib.bobe_gp_predict_cov(gp._h, xd.data_ptr(), c, cov.data_ptr()) == 0
    lib.bobe_gp_sync(gp._h)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) <= 64 << 20, (free0, free1)
    assert bool(torch.all(torch.isfinite(dr))) and jit.value >= 0.0
    # spot check of the big matrix: symmetric, and its diagonal is the predicted variance
    idx = torch.arange(0, c, 997, device="cuda")
    sub = cov[idx][:, idx].cpu().numpy()
    assert np.array_equal(sub, sub.T)
    _, var = gp._predict(xd[idx].cpu().numpy(), False, True, 0)
    np.testing.assert_allclose(np.maximum(np.diag(sub), 1e-12), var, rtol=0, atol=1e-12 * (gp.kernel_variance + gp.noise))


def _nested_pair(gp, seed):
    from bobe_amd.samplers import nested_sampling
    s0, z0, ok0 = nested_sampling(gp, mode="convergence", dlogz=0.05, rng=np.random.default_rng(seed), nlive=300)
    s1, z1, ok1 = nested_sampling(gp, mode="convergence", dlogz=0.05, rng=np.random.default_rng(seed), nlive=300,
                                  logz_draws=64, logz_draws_seed=5)
    return (s0, z0, ok0), (s1, z1, ok1)


def _replay(gp, s1, z1, nlive=300):
    from bobe_amd import samplers
    logl = s1["logl"]
    niter = z1["niter"]
    logvol_dead = -np.arange(1, niter + 1) / nlive
    logvol_live = (logvol_dead[-1] if niter else 0.0) + np.log1p(-(np.arange(nlive) + 1.0) / (nlive + 1.0))
    logvol = np.concatenate([logvol_dead, logvol_live])
    idx = samplers.draws_points(gp, logl, logvol)
    delta = gp.sample_posterior(s1["x"][idx], n_samples=64, seed=5, centered=True)
    out = np.empty(64)
    for s in range(64):
        ls = logl.copy()
        ls[idx] += delta[s]
        out[s] = samplers.compute_integrals(logl=ls, logvol=logvol)[-1]
    return out, len(idx)


def test_nested_sampling_reports_evidence_draws():
    from bobe_amd import GP
    d, sig = 2, 0.2
    # sparsely trained: the draws spread
    X = qmc.Sobol(d, scramble=True, seed=1).random(8)
    gp = GP(X, -0.5 * np.sum(((X - 0.5) / sig) ** 2, axis=1), noise=1e-8, lengthscales=[0.3, 0.3], kernel_variance=1.0)
    (s0, z0, ok0), (s1, z1, ok1) = _nested_pair(gp, 3)
    assert ok0 == ok1
    for k, v in s0.items():
        assert np.array_equal(np.asarray(s1[k]), np.asarray(v)) if k != "method" else s1[k] == v, k
    for k, v in z0.items():
        assert np.array_equal(np.asarray(z1[k]), np.asarray(v)), k
    assert set(z1) == set(z0) | {"draws", "draws_mean", "draws_std", "draws_points", "draws_jitter"}
    rep, npts = _replay(gp, s1, z1)
    assert z1["draws_points"] == npts
    assert np.array_equal(z1["draws"], rep)
    assert z1["draws_std"] > 0 and z1["draws_mean"] == pytest.approx(float(np.mean(rep)))
    # densely trained on a low-variance surface: the draws all but coincide
    X = qmc.Sobol(d, scramble=True, seed=2).random(256)
    y = -1.0 + 1e-3 * np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1])
    gp2 = GP(X, y, noise=1e-8, lengthscales=[0.5, 0.5], kernel_variance=1.0)
    _, (s2, z2, _) = _nested_pair(gp2, 4)
    assert 0 <= z2["draws_std"] < 1e-6, z2["draws_std"]
