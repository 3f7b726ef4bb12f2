"""GPU parity tests proper: the HIP path (through the C ABI / ctypes wrapper) against the CPU oracle
on identical seeded inputs, against the committed golden vectors, and — at BASELINE.json's full
sizes — through size-independent properties.

Tolerances (fp64): |dLML|/|LML| <= 1e-10, |dgrad|_inf/|grad|_inf <= 1e-8,
|dmu| <= 1e-8 max|y| (standardised y: max|y| ~ 3), |dvar| <= 1e-9 sigma^2 + 1e-7 var_ref,
identical argmin (unless the two best scores are closer than 1e-9 relative).
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest
from scipy.linalg import solve_triangular

pytestmark = pytest.mark.gpu

from oracle import bobe_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from bobe_amd import _lib
    lib = _lib.load()
    assert lib.bobe_device_count() >= 1, "native library loaded but no HIP device"
    return lib


def GP(*a, **k):
    from bobe_amd import GP as _GP
    return _GP(*a, **k)


def ref_data(n, d, seed=42):
    rng = np.random.RandomState(seed)           # reference tests/test_gp.py:21-27
    X = rng.uniform(0, 1, size=(n, d))
    y = -np.sum((X - 0.5) ** 2, axis=1).reshape(-1, 1)
    return X, y


def smooth_data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, -1]) * X[:, d // 2]
    return X, y


def both(X, y, **kw):
    return GP(X, y, **kw), O.OracleGP(X, y, **kw)


def assert_var_close(v, ref, kself):
    assert np.all(np.abs(v - ref) <= 1e-9 * kself + 1e-7 * np.abs(ref)), np.max(np.abs(v - ref))


def assert_argmin(idx, scores_ref):
    best = int(np.argmin(scores_ref))
    if idx != best:
        s = np.sort(scores_ref)
        assert abs(scores_ref[idx] - s[0]) <= 1e-9 * abs(s[0]), (idx, best)


# ------------------------------------------------------------------------------------------------
def test_mfma_gemm_core_exact(lib):
    from bobe_amd import _lib
    rng = np.random.default_rng(0)
    M, N, K = 256, 384, 176
    for la in (0, 1):
        for lb in (0, 1):
            A = rng.integers(-8, 9, size=(M, K)).astype(np.float64)
            B = rng.integers(-8, 9, size=(N, K)).astype(np.float64)     # asymmetric integer data: exact in fp64
            Aa = np.ascontiguousarray(A if la == 0 else A.T)
            Ba = np.ascontiguousarray(B if lb == 0 else B.T)
            Cc = np.full((M, N), np.nan)
            st = lib.bobe_debug_gemm(0, la, lb, M, N, K, _lib.ptr(Aa), Aa.shape[1], _lib.ptr(Ba), Ba.shape[1],
                                     _lib.ptr(Cc), N)
            assert st == 0, lib.bobe_last_error()
            assert np.array_equal(Cc, A @ B.T), (la, lb)
    assert lib.bobe_debug_gemm(0, 0, 0, 100, 128, 16, None, 16, None, 16, None, 128) < 0   # bad shape -> error code


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_kernel_matrix(kernel):
    rng = np.random.default_rng(1)
    A, B = rng.uniform(size=(150, 4)), rng.uniform(size=(37, 4))
    ls = np.array([0.2, 0.5, 1.0, 3.0])
    gp = GP(A, np.zeros(150), noise=1e-3, kernel=kernel, lengthscales=ls, kernel_variance=2.5)
    kf = O.get_kernel(kernel)
    assert np.allclose(gp.kernel(A, B, include_noise=False), kf(A, B, ls, 2.5, 1e-3, include_noise=False), rtol=1e-14, atol=1e-15)
    Kxx = gp.kernel(A, A, include_noise=True)
    assert np.allclose(Kxx, kf(A, A, ls, 2.5, 1e-3, include_noise=True), rtol=1e-14, atol=1e-15)
    assert np.all(np.diag(Kxx) == pytest.approx(2.5 + 1e-3, rel=1e-14))
    ls2 = np.array([1.0, 0.3, 0.3, 0.9])        # explicit hyper-parameters (acquisition.py:388 call form)
    assert np.allclose(gp.kernel(A, B, ls2, 0.7, 0.0, include_noise=False), kf(A, B, ls2, 0.7, 0.0, include_noise=False), rtol=1e-14, atol=1e-15)
    with pytest.raises(Exception):
        gp.kernel(A, B, include_noise=True)     # noise*eye needs a square matrix (gp.py:153)


@pytest.mark.parametrize("n,d", [(1, 1), (2, 2), (50, 2), (128, 3), (129, 3), (300, 6), (641, 8)])
def test_factor_ragged_sizes(lib, n, d):
    from bobe_amd import _lib
    X, y = smooth_data(n, d, seed=n)
    ls = np.full(d, 0.5)
    gp, og = both(X, y, noise=1e-6, lengthscales=ls, kernel_variance=1.2)
    assert not gp.not_pd
    L = gp.cholesky
    assert np.all(np.triu(L, 1) == 0)
    K = og.kernel(X, X, ls, 1.2, 1e-6, include_noise=True)
    assert np.max(np.abs(L @ L.T - K)) <= 1e-13
    assert np.allclose(L, og.cholesky, rtol=0, atol=1e-10)
    Li = np.empty((n, n))
    assert lib.bobe_debug_linv(gp._h, _lib.ptr(Li)) == 0
    assert np.max(np.abs(Li @ og.cholesky - np.eye(n))) <= 1e-8
    a, ao = gp.alphas.ravel(), og.alphas.ravel()
    assert np.max(np.abs(a - ao)) <= 1e-7 * np.max(np.abs(ao))
    assert np.allclose(gp.predict_mean_batched(X[:5]), og.predict_mean_batched(X[:5]), atol=1e-8 * max(1.0, np.max(np.abs(y))))


def test_not_positive_definite_gives_nan_not_exception():
    X = np.array([[0.1, 0.2], [0.1, 0.2], [0.7, 0.3]])           # duplicated point, zero noise -> singular K
    y = np.array([1.0, 2.0, 3.0])
    gp = GP(X, y, noise=0.0, lengthscales=[0.5, 0.5])
    assert gp.not_pd
    assert np.all(np.isnan(gp.cholesky)) and np.all(np.isnan(gp.alphas))
    f, g = gp.neg_mll_value_and_grad(np.log([0.5, 0.5, 1.0]))
    assert np.isnan(f) and np.all(np.isnan(g))                   # np.isfinite filter of optim.py:328,341 keeps working
    og = O.OracleGP(X, y, noise=0.0, lengthscales=[0.5, 0.5])
    assert np.isnan(og.neg_mll(np.log([0.5, 0.5, 1.0])))


def test_numerically_singular_kernel_matrix_counts_as_not_positive_definite():
    """The factorisation's rank test (gp_handle.hpp, pivot_floor; opted into with ``pivot_floor_ulp=64``, as the BO driver
    does - the GP class alone keeps the reference's sign-only rule): with the default noise of 1e-8 and a kernel variance
    of 1e7 at long length scales every trailing pivot is rounding noise (64 ulp of the diagonal is 1.4e-7 > noise); the
    log-determinant built on them is too small and draws the optimiser in (profiles/r04_config5.txt, section 9).  LAPACK -
    the reference's Cholesky - fails or passes on the last bit there; the library says BOBE_NOT_PD every time: NaN value and
    gradient from every evaluation path, a NaN state from bobe_gp_factor.  Moderate hyper-parameters on the same data are
    untouched and agree with the oracle."""
    from bobe_amd import _lib
    rng = np.random.default_rng(3)
    n, d = 500, 5
    X = rng.uniform(size=(n, d))
    y = -np.sum((X - 0.4) ** 2, axis=1) - 0.3 * np.prod(X[:, :2], axis=1)
    gp = GP(X, y, noise=1e-8, lengthscales=np.full(d, 0.5), kernel_variance=1.0, pivot_floor_ulp=64.0)
    og = O.OracleGP(X, y, noise=1e-8, lengthscales=np.full(d, 0.5), kernel_variance=1.0)
    assert not gp.not_pd and gp.pivot_floor_ulp == 64.0
    good, bad = (np.full(d, 0.5), 1.0), (np.full(d, 3.5), 1e7)
    m, g = gp.mll_data(*good)
    mo, go = O.cycle_value_and_grad(og.train_x, og.train_y.reshape(-1), good[0], good[1], 1e-8)
    assert abs(m - mo) <= 1e-9 * abs(mo) and np.all(np.isfinite(g))
    mb, gb = gp.mll_data(*bad)
    assert np.isnan(mb) and np.all(np.isnan(gb))
    ms, gs = gp.mll_data(*bad, slot=2)
    assert np.isnan(ms) and np.all(np.isnan(gs))
    mm, gg = gp.mll_data_batch(np.array([good[0], bad[0], good[0]]), np.array([good[1], bad[1], good[1]]))
    assert mm[0] == m and mm[2] == m and np.isnan(mm[1]) and np.all(np.isnan(gg[1])) and np.array_equal(gg[0], g)
    st = gp._lib.bobe_gp_mll(gp._h, _lib.ptr(bad[0]), bad[1], C.byref(C.c_double()), None)
    assert st == _lib.BOBE_NOT_PD and gp._lib.bobe_last_error()      # (a pivot <= 0 or one below the floor, whichever came first)
    f, gr = gp.neg_mll_value_and_grad(np.log(np.append(bad[0], bad[1])))
    assert np.isnan(f) and np.all(np.isnan(gr))                                 # what optimize_scipy's isfinite filter sees
    gp.update_hyperparams(np.log(np.append(bad[0], bad[1])))                    # the state: NaN factor, NaN predictions
    assert gp.not_pd and np.all(np.isnan(gp.alphas)) and np.all(np.isnan(gp.predict_mean_batched(X[:5])))
    gp.update_hyperparams(np.log(np.append(good[0], good[1])))                  # and back
    assert not gp.not_pd and np.allclose(gp.predict_mean_batched(X[:5]), og.predict_mean_batched(X[:5]), rtol=1e-7, atol=1e-9)
    # the floor itself, on a pair of points whose second pivot is known: kvar (1 - rho^2) with 1 - rho^2 ~ r^2 = 1e-15 is a
    # POSITIVE pivot below 64 ulp of the diagonal (1.4e-14): refused; r^2 = 1e-12 is above it: factorised, equal to the oracle
    for r2, refused in ((1e-15, True), (1e-12, False)):
        X3 = np.array([[0.3], [0.3 + 0.5 * np.sqrt(r2)], [0.9]])
        y3 = np.array([0.1, 0.1, -1.0])
        g3 = GP(X3, y3, noise=0.0, lengthscales=[0.5], kernel_variance=1.0, pivot_floor_ulp=64.0)
        assert g3.not_pd == refused
        v3, _ = g3.mll_data(np.array([0.5]), 1.0)
        if refused:
            assert np.isnan(v3) and b"numerically singular" in g3._lib.bobe_last_error()
        else:
            o3 = O.OracleGP(X3, y3, noise=0.0, lengthscales=[0.5], kernel_variance=1.0)
            w3, _ = O.cycle_value_and_grad(o3.train_x, o3.train_y.reshape(-1), np.array([0.5]), 1.0, 0.0)
            assert np.isfinite(v3) and abs(v3 - w3) <= 1e-3 * abs(w3)       # (cond ~ 1e12: three digits is what fp64 leaves)
    # a fit from the singular corner walks out of it, like the reference's would from a NaN start (optim.py:328, 341)
    res = gp.fit(x0=np.array([np.log(np.append(bad[0], bad[1])), np.log(np.append(good[0], good[1]))]), maxiter=20)
    assert np.isfinite(res["mll"]) and np.all(np.isfinite(res["params"]))


@pytest.mark.parametrize("kernel,prior,n,d", [("rbf", None, 200, 3), ("matern", None, 333, 4), ("rbf", "DSLP", 150, 2),
                                               ("rbf", "SAAS", 260, 9), ("matern", "SAAS", 140, 17)])
def test_mll_and_gradient(kernel, prior, n, d):
    X, y = smooth_data(n, d, seed=5)
    ls = 0.4 + 0.05 * np.arange(d)
    gp, og = both(X, y, noise=1e-6, kernel=kernel, lengthscales=ls, kernel_variance=1.4, lengthscale_prior=prior)
    for shift in (0.0, 0.08, -0.11):
        th = np.log(gp.get_hyperparams()) + shift * np.cos(np.arange(gp.num_hyperparams))
        f, g = gp.neg_mll_value_and_grad(th)
        fo, go = og.neg_mll_value_and_grad(th)
        assert abs(f - fo) <= 1e-10 * abs(fo)
        assert np.max(np.abs(g - go)) <= 1e-8 * np.max(np.abs(go)) + 1e-6 * (prior is not None)  # oracle prior grad is FD
        assert gp.neg_mll(th) == f
    # the factored state is not disturbed by mll evaluations
    assert np.allclose(gp.cholesky, og.cholesky, atol=1e-10)


def test_fixed_kernel_variance_parameterisation():
    X, y = smooth_data(120, 3, seed=2)
    gp, og = both(X, y, noise=1e-6, lengthscales=[0.5, 0.6, 0.7], kernel_variance=2.0, kernel_variance_prior="fixed")
    assert gp.num_hyperparams == 3 and gp.hyperparam_bounds.shape == (2, 3)
    th = np.log([0.45, 0.66, 0.71])
    f, g = gp.neg_mll_value_and_grad(th)
    fo, go = og.neg_mll_value_and_grad(th)
    assert abs(f - fo) <= 1e-10 * abs(fo) and np.max(np.abs(g - go)) <= 1e-8 * np.max(np.abs(go))


def test_fit_follows_oracle_trajectory():
    X, y = ref_data(60, 2)
    gp, og = both(X, y, noise=1e-6, lengthscale_bounds=[0.01, 10], kernel_variance_bounds=[1e-4, 1e4])
    rng = np.random.default_rng(3)
    x0 = O.restart_points(np.log(og.get_hyperparams()), og.hyperparam_bounds, 3, rng)     # pool.py:277-286
    r, ro = gp.fit(x0=x0, maxiter=60), og.fit(x0=x0, maxiter=60)
    assert r["mll"] is not None and np.isfinite(r["mll"])                                 # tests/test_gp.py:88
    assert r["mll"] == pytest.approx(ro["mll"], rel=1e-6)
    assert np.allclose(r["params"], ro["params"], atol=1e-4)
    gp.update_hyperparams(r["params"])
    og.update_hyperparams(ro["params"])
    q = np.random.default_rng(0).uniform(size=(20, 2))
    assert np.allclose(gp.predict_mean_batched(q), og.predict_mean_batched(q), atol=1e-6)


def test_predict_family_and_reference_invariants():
    X, y = ref_data(25, 2)
    gp, og = both(X, y, noise=1e-6)                       # default ls=1, kvar=1 (tests/test_gp.py:129-139)
    assert gp.predict_var_single(X[0]) < 1e-3
    q = np.random.default_rng(1).uniform(size=(64, 2))
    m, v = gp.predict_batched(q)
    mo, vo = og.predict_batched(q)
    assert m.shape == (64,) and v.shape == (64,) and np.all(v > 0)
    assert np.allclose(m, mo, atol=1e-8 * 3) and np.all(np.abs(v - vo) <= 1e-9 + 1e-7 * vo)
    assert np.allclose(gp.predict_mean_batched(q), og.predict_mean_batched(q), atol=1e-8 * np.max(np.abs(y)) + 1e-9)
    assert np.all(np.abs(gp.predict_var_batched(q) - og.predict_var_batched(q)) <= og.y_std ** 2 * (1e-9 + 1e-7 * vo))
    ms, vs = gp.predict_single(q[0])
    assert ms == m[0] and vs[0] == v[0]
    g1 = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=[0.2, 0.2])
    g2 = GP(X, y, noise=1e-6, kernel="matern", lengthscales=[0.2, 0.2])
    a, b = g1.predict_mean_single([0.5, 0.5]), g2.predict_mean_single([0.5, 0.5])
    assert abs(a - b) > 1e-6                                # tests/test_gp.py:295 — kernels really differ


def test_update_state_dict_copy(tmp_path):
    X, y = ref_data(30, 2)
    gp, og = both(X, y, noise=1e-6, lengthscales=[0.4, 0.6])
    new_x = np.array([[0.11, 0.93], [0.87, 0.07]])
    new_y = np.array([[-0.3], [-0.2]])
    gp.update(new_x, new_y)
    og.update(new_x, new_y)
    assert gp.npoints == 32
    gp.update(X[:1], y[:1])                                  # duplicate rejected (tests/test_gp.py:165-169)
    assert gp.npoints == 32
    assert gp.y_mean == pytest.approx(og.y_mean) and gp.y_std == pytest.approx(og.y_std)
    q = np.random.default_rng(2).uniform(size=(10, 2))
    assert np.allclose(gp.predict_mean_batched(q), og.predict_mean_batched(q), atol=1e-8)
    sd = gp.state_dict()
    assert set(sd) >= {"train_x", "train_y", "lengthscales", "kernel_variance", "noise", "tausq", "y_mean", "y_std",
                       "kernel_name", "cholesky", "alphas", "ndim", "gp_class", "lengthscale_bounds"}
    fn = str(tmp_path / "gp_state")
    gp.save(fn)
    from bobe_amd import GP as GPcls
    gp2 = GPcls.load(fn)
    assert np.allclose(gp2.predict_mean_batched(q), gp.predict_mean_batched(q), rtol=1e-6)     # tests/test_gp.py:228-244
    assert np.allclose(gp2.predict_var_batched(q), gp.predict_var_batched(q), rtol=1e-6, atol=1e-12)
    assert np.allclose(gp2.cholesky, gp.cholesky, atol=1e-12)
    gp3 = gp.copy()
    gp3.update(np.array([[0.5, 0.5]]), np.array([[0.0]]))
    assert gp3.npoints == 33 and gp.npoints == 32                                             # copy independence


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_sweep_against_oracle_and_literal(kernel):
    X, y = smooth_data(300, 4, seed=8)
    ls = [0.3, 0.5, 0.4, 0.6]
    gp, og = both(X, y * 3 + 1, noise=1e-6, kernel=kernel, lengthscales=ls, kernel_variance=1.1)
    rng = np.random.default_rng(9)
    cand, Z = rng.uniform(size=(500, 4)), rng.uniform(size=(70, 4))
    cand[0] = X[3]                                           # on top of a training point: s_c ~ noise
    r = gp.wip_sweep(cand, Z, want_mean_var=True)
    ro = O.wip_sweep(og, cand, Z)
    kself = 1.1 + 1e-6
    assert np.allclose(r["mean"], ro["mean"], atol=1e-8 * 3)
    assert_var_close(r["var"], ro["var"], kself)
    assert np.all(np.abs(r["wipv"] - ro["wipv"]) <= og.y_std ** 2 * (1e-9 * kself + 1e-7 * ro["wipv"] / og.y_std ** 2))
    assert np.all(np.abs(r["wipstd"] - ro["wipstd"]) <= 1e-7 * ro["wipstd"] + 1e-9 * og.y_std)
    assert_argmin(r["argmin_v"], ro["wipv"])
    assert_argmin(r["argmin_s"], ro["wipstd"])
    assert r["min_s"] == r["wipstd"][r["argmin_s"]] and r["min_v"] == r["wipv"][r["argmin_v"]]
    # literal (N+1)-factor fantasy variance of the reference (gp.py:552-576) for a few candidates
    fv = gp.fantasy_var(cand[:4], Z)
    lit = np.array([og.fantasy_var(c, Z, og._k12(Z)) for c in cand[:4]])
    assert np.all(np.abs(fv - lit) <= og.y_std ** 2 * (1e-9 * kself + 1e-6 * lit / og.y_std ** 2))
    assert np.allclose(gp.fantasy_var(cand[2], Z, None), lit[2], rtol=1e-6, atol=1e-9 * og.y_std ** 2)


def test_sweep_candidates_equal_integration_points_and_chunking(lib):
    """acquisition.py:394 maps over mc_points themselves; chunk size must not change any bit."""
    X, y = smooth_data(200, 3, seed=4)
    gp, og = both(X, y, noise=1e-6, lengthscales=[0.4, 0.4, 0.4])
    Z = np.random.default_rng(5).uniform(size=(300, 3))
    r1 = gp.wip_sweep(Z, Z)
    ro = O.wip_sweep(og, Z, Z)
    assert_argmin(r1["argmin_s"], ro["wipstd"])
    assert lib.bobe_gp_set_chunk(gp._h, 128) == 0
    r2 = gp.wip_sweep(Z, Z)
    assert np.array_equal(r1["wipv"], r2["wipv"]) and np.array_equal(r1["wipstd"], r2["wipstd"])
    assert r1["argmin_s"] == r2["argmin_s"]
    assert lib.bobe_gp_set_chunk(gp._h, 100) < 0


def test_device_pointers_equal_host_pointers():
    import torch
    X, y = smooth_data(150, 3, seed=6)
    gp = GP(X, y, noise=1e-6, lengthscales=[0.4, 0.5, 0.6])
    rng = np.random.default_rng(7)
    cand, Z = rng.uniform(size=(260, 3)), rng.uniform(size=(40, 3))
    rh = gp.wip_sweep(cand, Z)
    rd = gp.wip_sweep(torch.from_numpy(cand).cuda(), torch.from_numpy(Z).cuda())
    assert np.array_equal(rh["wipv"], rd["wipv"]) and rh["argmin_v"] == rd["argmin_v"]


def test_ei_and_log_ei_scorers():
    X, y = ref_data(30, 2)                                   # tests/test_acquisition.py:21-37 recipe
    y = -np.sum((X - 0.7) ** 2, axis=1, keepdims=True)
    gp, og = both(X, y, noise=1e-6, lengthscales=[0.3, 0.3], kernel_variance=1.0)
    q = np.random.default_rng(3).uniform(size=(100, 2))
    best = float(np.max(og.train_y))
    m, v = og.predict_batched(q)
    ei = gp.acq_ei(q, best)
    assert np.all(ei >= 0)                                    # tests/test_acquisition.py:92-95
    assert np.allclose(ei, O.ei_score(m, v, best), rtol=1e-6, atol=1e-12)
    le, leo = gp.acq_ei(q, best, log_ei=True), O.log_ei_score(m, v, best)
    assert np.all(np.isfinite(le))
    assert np.allclose(le, leo, rtol=1e-6, atol=1e-6)


def test_acquisition_classes_next_point_and_batch():
    from bobe_amd import WIPStd, WIPV, EI, get_mc_samples
    X, y = ref_data(40, 2)
    gp = GP(X, y, noise=1e-6, lengthscales=[0.3, 0.3])
    rng = np.random.default_rng(0)
    mc = get_mc_samples(gp, num_samples=256, method="uniform", np_rng=1)
    for cls in (WIPV, WIPStd):
        x, val = cls().get_next_point(gp, acq_kwargs={"mc_samples": mc, "mc_points_size": 64}, rng=rng, maxiter=20)
        assert np.shape(x) == (2,) and np.all(x >= 0) and np.all(x <= 1) and np.isfinite(val)
    xb, vb = WIPStd().get_next_batch(gp, n_batch=3, acq_kwargs={"mc_samples": mc, "mc_points_size": 64}, rng=rng, maxiter=10,
                                     n_restarts=1)      # bo.py:1274 calls with n_restarts=1
    assert xb.shape == (3, 2) and vb.shape == (3,)             # tests/test_acquisition.py:233-235
    x, val = EI().get_next_point(gp, acq_kwargs={}, n_restarts=4, maxiter=30, rng=rng)
    assert np.shape(x) == (2,) and val >= 0                    # tests/test_acquisition.py:156-158


GOLDEN = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz"))
                if not os.path.basename(p).startswith("loop_"))     # loop_*: BO-step fixtures (tests/test_gpu_loop_parity.py)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_hip_path_matches_golden_vectors(path):
    g = dict(np.load(path, allow_pickle=False))
    prior = None if str(g["prior"]) == "none" else str(g["prior"])
    gp = GP(g["X"], g["y"], noise=float(g["noise"]), kernel=str(g["kernel"]), lengthscales=g["lengthscales"],
            kernel_variance=float(g["kernel_variance"]), lengthscale_prior=prior)
    f, gr = gp.neg_mll_value_and_grad(g["theta"])
    assert abs(f - float(g["neg_mll"])) <= 1e-10 * abs(float(g["neg_mll"]))
    assert np.max(np.abs(gr - g["neg_mll_grad"])) <= 1e-6 * np.max(np.abs(g["neg_mll_grad"]))
    assert np.allclose(gp.cholesky, g["cholesky"], atol=1e-10)
    r = gp.wip_sweep(g["cand"], g["Z"], want_mean_var=True)
    kself = float(g["kernel_variance"]) + float(g["noise"])
    ys = float(g["y_std"])
    assert np.allclose(r["mean"], g["mean"], atol=3e-8)
    assert_var_close(r["var"], g["var"], kself)
    assert np.all(np.abs(r["wipv"] - g["wipv"]) <= ys ** 2 * 1e-9 * kself + 1e-7 * g["wipv"])
    assert np.all(np.abs(r["wipstd"] - g["wipstd"]) <= 1e-9 * ys + 1e-7 * g["wipstd"])
    assert_argmin(r["argmin_v"], g["wipv"])
    assert_argmin(r["argmin_s"], g["wipstd"])
    fv = gp.fantasy_var(g["cand"][:6], g["Z"])
    assert np.all(np.abs(fv - g["fantasy"]) <= ys ** 2 * 1e-9 * kself + 1e-6 * g["fantasy"])
    assert np.allclose(gp.predict_mean_batched(g["cand"]), g["pred_mean"], atol=1e-8 * np.max(np.abs(g["y"])) + 1e-9)
    assert np.allclose(gp.acq_ei(g["cand"], float(g["best_y"])), g["ei"], rtol=1e-5, atol=1e-10)


# ------------------------------------------------------------------------------------------------
# BASELINE.json sizes: oracle where it finishes in seconds (config 2), properties at config 3
# ------------------------------------------------------------------------------------------------
def test_small_config_against_oracle():
    from bobe_amd.synthetic import synthetic_problem, theta_schedule
    N, d, Cn, M = 1024, 6, 8192, 512
    X, y, cand, Z = synthetic_problem(N, d, Cn, M)
    th = theta_schedule(d)
    ls, kv = np.exp(th[-1, :d]), float(np.exp(th[-1, d]))
    gp, og = both(X, y, noise=1e-6, lengthscales=ls, kernel_variance=kv)
    for k in (0, 7, 19):
        f, g = gp.neg_mll_value_and_grad(th[k])
        fo, go = og.neg_mll_value_and_grad(th[k])
        assert abs(f - fo) <= 1e-10 * abs(fo)
        assert np.max(np.abs(g - go)) <= 1e-8 * np.max(np.abs(go))
    r = gp.wip_sweep(cand, Z, want_mean_var=True)
    ro = O.wip_sweep(og, cand, Z)
    assert np.max(np.abs(r["mean"] - ro["mean"])) <= 1e-8 * np.max(np.abs(y))
    assert_var_close(r["var"], ro["var"], kv + 1e-6)
    assert np.all(np.abs(r["wipv"] - ro["wipv"]) <= 1e-9 * (kv + 1e-6) + 1e-7 * ro["wipv"])
    assert np.all(np.abs(r["wipstd"] - ro["wipstd"]) <= 1e-9 + 1e-7 * ro["wipstd"])
    assert_argmin(r["argmin_v"], ro["wipv"])
    assert_argmin(r["argmin_s"], ro["wipstd"])


def test_headline_config_properties(lib):
    """N=4096, d=8, C=65536, M=512: size-independent properties (the oracle is only used for an O(N^3/3)
    Cholesky and O(N^2) checks here)."""
    from bobe_amd import _lib
    from bobe_amd.synthetic import synthetic_problem, theta_schedule
    N, d, Cn, M = 4096, 8, 65536, 512
    X, y, cand, Z = synthetic_problem(N, d, Cn, M)
    th = theta_schedule(d)
    ls, kv = np.exp(th[-1, :d]), float(np.exp(th[-1, d]))
    gp = GP(X, y, noise=1e-6, lengthscales=ls, kernel_variance=kv)
    assert not gp.not_pd
    # (1) L L^T = K and L matches LAPACK
    K = O.rbf_kernel(X, X, ls, kv, 1e-6, include_noise=True)
    L = gp.cholesky
    assert np.max(np.abs(L @ L.T - K)) <= 1e-12
    Lo = O.chol_nan(K)
    assert np.max(np.abs(L - Lo)) <= 1e-9
    # (2) MLL value against the LAPACK factor; gradient against a central difference of the GPU value
    alpha_o = solve_triangular(Lo, solve_triangular(Lo, y, lower=True), lower=True, trans="T")
    mll_o = -0.5 * y @ alpha_o - np.sum(np.log(np.diag(Lo))) - 0.5 * N * np.log(2 * np.pi)
    f, g = gp.neg_mll_value_and_grad(th[-1])
    mll_gpu, _ = gp.mll_data(ls, kv, want_grad=False)          # data term only (the default priors are constants)
    assert abs(mll_gpu - mll_o) <= 1e-10 * abs(mll_o)
    assert -f == pytest.approx(mll_gpu + gp.prior_func(ls, kv, 1.0), rel=1e-14)
    # full gradient against the oracle's LAPACK (dpotrf/dpotri) evaluation at the same theta (~5 s of CPU)
    mll_cpu, g_cpu = O.cycle_value_and_grad(X, y, ls, kv, 1e-6)
    _, g_gpu = gp.mll_data(ls, kv)
    assert abs(mll_gpu - mll_cpu) <= 1e-10 * abs(mll_cpu)
    assert np.max(np.abs(g_gpu - g_cpu)) <= 1e-8 * np.max(np.abs(g_cpu))
    # the concurrent evaluation of several theta (CU-partitioned streams, other tile sizes) returns the same bits
    lsb, kvb = np.exp(th[-4:, :d]), np.exp(th[-4:, d])
    mb, gb = gp.mll_data_batch(lsb, kvb)
    for b in range(4):
        m1, g1 = gp.mll_data(lsb[b], kvb[b])
        assert mb[b] == m1 and np.array_equal(gb[b], g1)
    assert mb[3] == mll_gpu
    e = 1e-4
    for j in (0, d):
        tp, tm = th[-1].copy(), th[-1].copy()
        tp[j] += e
        tm[j] -= e
        fd = (gp.neg_mll(tp) - gp.neg_mll(tm)) / (2 * e)
        assert g[j] == pytest.approx(fd, rel=1e-5)
    # (3) sweep properties
    r = gp.wip_sweep(cand, Z, want_mean_var=True)
    assert np.all(np.isfinite(r["wipv"])) and np.all(r["wipv"] > 0) and np.all(r["wipstd"] > 0)
    assert r["argmin_v"] == int(np.argmin(r["wipv"])) and r["argmin_s"] == int(np.argmin(r["wipstd"]))
    base = np.mean(gp.predict_batched(Z)[1])                 # current integrated variance
    assert np.all(r["wipv"] <= base * (1 + 1e-9))            # a fantasy point never increases posterior variance
    assert np.all(r["wipstd"] ** 2 <= r["wipv"] * (1 + 1e-12))   # Jensen: mean(sqrt(v))^2 <= mean(v)
    assert np.all(r["var"] <= kv + 1e-6 + 1e-12) and np.all(r["var"] >= 1e-12)
    # (4) spot-check 64 candidates against the oracle's triangular solves with the LAPACK factor
    idx = np.random.default_rng(0).choice(Cn, 64, replace=False)
    kc = O.rbf_kernel(X, cand[idx], ls, kv, 1e-6, include_noise=False)
    vc = solve_triangular(Lo, kc, lower=True)
    assert np.max(np.abs(r["mean"][idx] - kc.T @ alpha_o)) <= 1e-8 * np.max(np.abs(y))
    assert_var_close(r["var"][idx], np.maximum(kv + 1e-6 - np.sum(vc * vc, axis=0), 1e-12), kv + 1e-6)
    # (5) interpolation at training points and linearity of the mean in y
    m_tr = gp.predict_batched(X[:256])[0]
    assert np.max(np.abs(m_tr - y[:256])) <= 5e-3
    gp2 = GP(X, 2.0 * y + 1.0, noise=1e-6, lengthscales=ls, kernel_variance=kv)   # standardisation removes scale/shift
    assert np.allclose(gp2.predict_batched(cand[:512])[0], r["mean"][:512], atol=1e-9)
    assert np.allclose(gp2.predict_mean_batched(cand[:512]), 2.0 * (r["mean"][:512] * gp.y_std + gp.y_mean) + 1.0, atol=1e-8)
    # (6) the same sweep with v = L^-1 k SOLVED for (blocked forward substitution, the path an ill-conditioned factor takes:
    # two chunks of 32 768 candidates, 512-row panels, 128-row diagonal blocks): on this well-conditioned factor it must give
    # the plain product's scores to rounding, the same picks, and the oracle's triangular-solve variance on the spot check
    gp.refine_kappa = 0.0
    gp.recompute_cholesky()
    assert gp.refining
    rs = gp.wip_sweep(cand, Z, want_mean_var=True)
    assert np.array_equal(rs["mean"], r["mean"])                                   # (the mean never goes through the solve)
    for k in ("wipv", "wipstd"):
        assert np.max(np.abs(rs[k] - r[k]) / np.abs(r[k])) <= 1e-11, k
    assert rs["argmin_v"] == r["argmin_v"] and rs["argmin_s"] == r["argmin_s"]
    assert_var_close(rs["var"][idx], np.maximum(kv + 1e-6 - np.sum(vc * vc, axis=0), 1e-12), kv + 1e-6)


def test_negative_fantasy_pivot_floors_everything(lib):
    """gp.py:187: sqrt(k_self - v.v) is NaN when the pivot is negative, which floors every var+(.|c) at 1e-12.
    Forced here by restoring a deliberately shrunken factor (L/2 quadruples |L^-1 k|^2)."""
    from bobe_amd import GP as GPcls
    X, y = smooth_data(90, 2, seed=12)
    gp, og = both(X, y, noise=1e-6, lengthscales=[0.4, 0.4])
    sd = gp.state_dict()
    sd["cholesky"] = 0.5 * sd["cholesky"]
    bad = GPcls.from_state_dict(sd)
    og.cholesky = 0.5 * og.cholesky
    rng = np.random.default_rng(1)
    cand, Z = np.vstack([X[:6] + 1e-3, rng.uniform(size=(20, 2))]), rng.uniform(size=(12, 2))
    r = bad.wip_sweep(cand, Z, want_mean_var=True)
    ro = O.wip_sweep(og, cand, Z)
    neg = (1.0 + 1e-6) - np.sum(solve_triangular(og.cholesky, og._k12(cand), lower=True) ** 2, axis=0) < 0
    assert neg.sum() >= 6                                   # the near-training candidates have s_c < 0
    assert np.all(r["wipv"][neg] == pytest.approx(1e-12 * og.y_std ** 2, rel=1e-12))
    assert np.allclose(r["wipv"], ro["wipv"], rtol=1e-7, atol=1e-18)
    assert np.allclose(r["wipstd"], ro["wipstd"], rtol=1e-7, atol=1e-18)
    assert np.all(r["var"][neg] == 1e-12)                   # predict_single floor (gp.py:487-488)
    pv = bad.predict_var_batched(cand)
    assert np.all(pv[neg] == pytest.approx(1e-12 * og.y_std ** 2))   # clip (gp.py:465)


def test_state_dict_interop_with_reference_format(tmp_path):
    """A reference-format state (the keys of gp.py:597-634, here produced by the oracle) loads into the GPU GP
    without refactorisation and reproduces its predictions; the GPU GP's own npz has the same keys."""
    from bobe_amd import GP as GPcls
    X, y = ref_data(45, 3)
    og = O.OracleGP(X, y, noise=1e-6, lengthscales=[0.3, 0.5, 0.7], kernel_variance=1.2)
    state = {"train_x": og.train_x, "train_y": og.train_y * og.y_std + og.y_mean, "lengthscales": og.lengthscales,
             "kernel_variance": og.kernel_variance, "noise": og.noise, "tausq": 1.0, "y_mean": og.y_mean,
             "y_std": og.y_std, "kernel_name": "rbf", "lengthscale_prior_spec": None,
             "kernel_variance_prior_spec": None, "fixed_kernel_variance": False, "optimizer_method": "scipy",
             "optimizer_options": {}, "lengthscale_bounds": [0.01, 5], "kernel_variance_bounds": [1e-4, 1e8],
             "tausq_bounds": [1e-4, 1e4], "cholesky": og.cholesky, "alphas": og.alphas, "ndim": 3, "gp_class": "GP"}
    fn = str(tmp_path / "ref_state.npz")
    np.savez(fn, **state)
    gp = GPcls.load(fn)
    q = np.random.default_rng(4).uniform(size=(30, 3))
    assert np.allclose(gp.predict_mean_batched(q), og.predict_mean_batched(q), atol=1e-9)
    assert np.allclose(gp.predict_var_batched(q), og.predict_var_batched(q), rtol=1e-6, atol=1e-12)
    assert np.array_equal(gp.cholesky, og.cholesky)          # restored bit for bit, not refactorised
    assert set(gp.state_dict()) == set(state)


def test_two_handles_are_independent():
    """Distinct handles own their buffers and streams (SURVEY 8b threading contract)."""
    X1, y1 = smooth_data(140, 3, seed=21)
    X2, y2 = smooth_data(260, 5, seed=22)
    g1, o1 = both(X1, y1, noise=1e-6, lengthscales=[0.4, 0.5, 0.6])
    g2, o2 = both(X2, y2, noise=1e-6, kernel="matern", lengthscales=[0.5] * 5)
    q1, q2 = np.random.default_rng(1).uniform(size=(33, 3)), np.random.default_rng(2).uniform(size=(47, 5))
    for _ in range(2):                                   # interleave calls on the two handles
        m1 = g1.predict_mean_batched(q1)
        f2, gr2 = g2.neg_mll_value_and_grad(np.log(g2.get_hyperparams()) + 0.05)
        m2 = g2.predict_mean_batched(q2)
        f1, gr1 = g1.neg_mll_value_and_grad(np.log(g1.get_hyperparams()) - 0.05)
    assert np.allclose(m1, o1.predict_mean_batched(q1), atol=1e-8) and np.allclose(m2, o2.predict_mean_batched(q2), atol=1e-8)
    assert f1 == pytest.approx(o1.neg_mll_value_and_grad(np.log(o1.get_hyperparams()) - 0.05)[0], rel=1e-10)
    assert f2 == pytest.approx(o2.neg_mll_value_and_grad(np.log(o2.get_hyperparams()) + 0.05)[0], rel=1e-10)


def test_growing_training_set_reallocates_cleanly():
    """update() across the 128-padding boundary (N = 120 -> 126 -> 132 -> 138) keeps matching the oracle."""
    X, y = smooth_data(120, 2, seed=30)
    gp, og = both(X, y, noise=1e-6, lengthscales=[0.4, 0.4])
    rng = np.random.default_rng(31)
    for _ in range(3):
        nx = rng.uniform(size=(6, 2))
        ny = (np.sin(3 * nx[:, 0]) + np.cos(2 * nx[:, 1]) * nx[:, 1]).reshape(-1, 1)
        gp.update(nx, ny)
        og.update(nx, ny)
        q = rng.uniform(size=(20, 2))
        assert gp.npoints == og.npoints
        assert np.allclose(gp.predict_mean_batched(q), og.predict_mean_batched(q), atol=1e-7)
        assert np.allclose(gp.cholesky, og.cholesky, atol=1e-10)


def test_config4_candidate_count_single_gpu():
    """BASELINE.json config 4 candidate set (262 144) unsharded on one GPU: several scoring super-chunks; the
    first 65 536 scores must be bit-identical to a sweep over that prefix alone."""
    from bobe_amd.synthetic import synthetic_problem, theta_schedule
    N, d, M = 1024, 8, 512
    X, y, cand, Z = synthetic_problem(N, d, 262144, M)
    th = theta_schedule(d)[-1]
    gp = GP(X, y, noise=1e-6, lengthscales=np.exp(th[:d]), kernel_variance=1.0)
    r = gp.wip_sweep(cand, Z)
    rp = gp.wip_sweep(cand[:65536], Z)
    assert np.array_equal(r["wipstd"][:65536], rp["wipstd"]) and np.array_equal(r["wipv"][:65536], rp["wipv"])
    assert r["argmin_s"] == int(np.argmin(r["wipstd"])) and np.all(np.isfinite(r["wipv"]))


@pytest.mark.parametrize("kernel,d", [("rbf", 3), ("matern", 5), ("rbf", 12), ("matern", 9), ("rbf", 17), ("matern", 17)])
def test_predict_grad_against_central_differences(kernel, d):
    """bobe_gp_predict_grad = the JAX autodiff of gp.predict_single in the reference (acquisition.py:246-253)."""
    X, y = smooth_data(180, d, seed=40 + d)
    ls = 0.35 + 0.05 * np.arange(d)
    gp, og = both(X, y, noise=1e-6, kernel=kernel, lengthscales=ls, kernel_variance=1.3)
    q = np.random.default_rng(3).uniform(0.1, 0.9, size=(9, d))
    m, v, dm, dv = gp.predict_grad(q)
    mo, vo = og.predict_batched(q)
    assert np.allclose(m, mo, atol=3e-8) and np.all(np.abs(v - vo) <= 1e-9 * 1.3 + 1e-7 * vo)
    e = 1e-6
    for j in range(d):
        qp, qm = q.copy(), q.copy()
        qp[:, j] += e
        qm[:, j] -= e
        mp, vp = og.predict_batched(qp)
        mm, vm = og.predict_batched(qm)
        assert np.allclose(dm[:, j], (mp - mm) / (2 * e), rtol=2e-5, atol=1e-6)
        assert np.allclose(dv[:, j], (vp - vm) / (2 * e), rtol=2e-4, atol=1e-6)
    # at a training point the variance sits near the floor; on the floor the gradient is zero
    _, v0, _, dv0 = gp.predict_grad(X[:1])
    assert v0[0] >= 1e-12 and np.all(np.isfinite(dv0))


def test_predict_grad_mean_only_mode():
    """var = dvar = NULL: the one-kernel mode used by HMC returns the same mean and mean gradient."""
    X, y = smooth_data(333, 5, seed=9)
    gp = GP(X, y, noise=1e-6, kernel="matern", lengthscales=np.full(5, 0.6), kernel_variance=1.2)
    q = np.random.default_rng(1).uniform(size=(77, 5))
    m, v, dm, dv = gp.predict_grad(q)
    m1, v1, dm1, dv1 = gp.predict_grad(q, mean_only=True)
    assert v1 is None and dv1 is None
    assert np.allclose(m1, m, rtol=1e-12, atol=1e-12) and np.allclose(dm1, dm, rtol=1e-12, atol=1e-12)
    assert np.allclose(m1, gp.predict_batched(q)[0], rtol=1e-11, atol=1e-11)


def test_ei_analytic_gradient_matches_finite_differences():
    from bobe_amd import EI, LogEI
    X, y = ref_data(30, 2)
    y = -np.sum((X - 0.7) ** 2, axis=1, keepdims=True)
    gp = GP(X, y, noise=1e-6, lengthscales=[0.3, 0.3])
    best = float(np.max(gp.train_y))
    for cls in (EI, LogEI):
        vg = cls()._value_and_grad(gp, best, 0.01)
        for x0 in (np.array([0.55, 0.62]), np.array([0.2, 0.9])):
            f, g = vg(x0)
            fd = np.array([(vg(x0 + h)[0] - vg(x0 - h)[0]) / 2e-6 for h in (np.array([1e-6, 0]), np.array([0, 1e-6]))])
            assert np.allclose(g, fd, rtol=1e-3, atol=1e-7 * max(1.0, abs(f)))


@pytest.mark.parametrize("n,d,B", [(300, 4, 1), (300, 4, 3), (700, 6, 4), (129, 2, 11)])
def test_mll_batch_is_bitwise_the_single_evaluation(n, d, B):
    """bobe_gp_mll_batch = the same kernels per vector on private streams / workspaces: identical bits, any B
    (B above the slot count runs in rounds), and the factored state is left alone."""
    X, y = smooth_data(n, d, seed=11)
    gp = GP(X, y, noise=1e-6, lengthscales=np.full(d, 0.5))
    chol0 = gp.cholesky.copy()
    rng = np.random.default_rng(B)
    ls = np.exp(rng.uniform(np.log(0.2), np.log(1.5), size=(B, d)))
    kv = np.exp(rng.uniform(-0.5, 0.5, size=B))
    one = [gp.mll_data(ls[b], kv[b]) for b in range(B)]
    mll, grad = gp.mll_data_batch(ls, kv)
    for b in range(B):
        assert mll[b] == one[b][0]
        assert np.array_equal(grad[b], one[b][1])
    mll2, none = gp.mll_data_batch(ls, kv, want_grad=False)
    assert none is None and np.array_equal(mll2, mll)
    assert np.array_equal(gp.cholesky, chol0)
    og = O.OracleGP(X, y, noise=1e-6, lengthscales=np.full(d, 0.5))
    ref = O.gp_mll(O.rbf_kernel(og.train_x, og.train_x, ls[0], kv[0], noise=1e-6, include_noise=True), og.train_y, n)
    assert abs(mll[0] - ref) <= 1e-10 * abs(ref)


def test_mll_batch_not_pd_member_does_not_poison_the_others():
    X = np.array([[0.1, 0.2], [0.1, 0.2], [0.7, 0.3], [0.4, 0.9]])      # duplicated point
    y = np.array([1.0, 2.0, 3.0, 0.5])
    gp = GP(X, y, noise=1e-9, lengthscales=[0.5, 0.5])
    # huge length scales make K numerically singular for the middle member only
    ls = np.array([[0.5, 0.5], [1e9, 1e9], [0.3, 0.8]])
    kv = np.ones(3)
    mll, grad = gp.mll_data_batch(ls, kv)
    a, b = gp.mll_data(ls[0], 1.0), gp.mll_data(ls[2], 1.0)
    mid = gp.mll_data(ls[1], 1.0)
    assert mll[0] == a[0] and mll[2] == b[0] and np.array_equal(grad[0], a[1]) and np.array_equal(grad[2], b[1])
    assert (np.isnan(mll[1]) and np.all(np.isnan(grad[1]))) if np.isnan(mid[0]) else mll[1] == mid[0]


def test_slot_evaluations_from_threads_are_bitwise_the_single_evaluation():
    """bobe_gp_mll_submit / _wait from concurrent host threads, one slot each (what GP.fit does per restart)."""
    import threading
    X, y = smooth_data(900, 5, seed=4)
    gp = GP(X, y, noise=1e-6, lengthscales=np.full(5, 0.5))
    rng = np.random.default_rng(1)
    ls = np.exp(rng.uniform(np.log(0.2), np.log(1.5), size=(4, 6, 5)))      # 4 threads x 6 evaluations
    ref = [[gp.mll_data(ls[t, k], 1.0 + 0.1 * k) for k in range(6)] for t in range(4)]
    got = [[None] * 6 for _ in range(4)]

    def work(t):
        for k in range(6):
            got[t][k] = gp.mll_data(ls[t, k], 1.0 + 0.1 * k, slot=t)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    for t in range(4):
        for k in range(6):
            assert got[t][k][0] == ref[t][k][0] and np.array_equal(got[t][k][1], ref[t][k][1])
    v, g = gp.mll_data(ls[0, 0], 1.0, want_grad=False, slot=2)
    assert g is None and v == ref[0][0][0]
    from bobe_amd import _lib
    with pytest.raises(_lib.BobeLibraryError):                              # wait without a submit
        _lib.check(gp._lib.bobe_gp_mll_wait(gp._h, 3, C.byref(C.c_double()), None), "wait")


def test_fit_with_concurrent_restarts_equals_sequential_restarts():
    """GP.fit runs its restarts concurrently (a thread and an evaluation slot each); every restart sees the values
    it would see alone, so the result is exactly the sequential one (optim.py:335-354 order of acceptance)."""
    X, y = ref_data(80, 3)
    gp = GP(X, y, noise=1e-6, lengthscale_bounds=[0.01, 10], kernel_variance_bounds=[1e-4, 1e4])
    rng = np.random.default_rng(5)
    x0 = O.restart_points(np.log(gp.get_hyperparams()), gp.hyperparam_bounds, 5, rng)
    gp.concurrent_restarts = False
    seq = gp.fit(x0=x0, maxiter=40)
    gp.concurrent_restarts = True
    con = gp.fit(x0=x0, maxiter=40)
    assert con["mll"] == seq["mll"] and np.array_equal(con["params"], seq["params"])
    from bobe_amd.optim import optimize_scipy                               # the lock-step (batched) driver too
    bat = optimize_scipy(gp.neg_mll_value_and_grad, num_params=gp.num_hyperparams, bounds=gp.hyperparam_bounds, x0=x0,
                         maxiter=40, n_restarts=5, optimizer_options={},
                         batch_value_and_grad=gp.neg_mll_value_and_grad_batch)
    assert -bat[1] == seq["mll"] and np.array_equal(bat[0], seq["params"])


def test_midsize_ragged_factor_inverse_and_gradient(lib):
    """N = 2500 (20 blocks, not a power of two, last block ragged): exercises the 64x64/BK16 trailing update at a
    size where it runs several rounds, the odd splits of the recursive inverse and the padded last block."""
    from bobe_amd import _lib
    n, d = 2500, 5
    X, y = smooth_data(n, d, seed=21)
    ls, kv = np.array([0.5, 0.6, 0.7, 0.55, 0.65]), 1.3
    gp = GP(X, y, noise=1e-5, lengthscales=ls, kernel_variance=kv)
    assert not gp.not_pd
    K = O.rbf_kernel(X, X, ls, kv, 1e-5, include_noise=True)
    L = gp.cholesky
    assert np.all(np.triu(L, 1) == 0)
    assert np.max(np.abs(L @ L.T - K)) <= 1e-12
    Lo = O.chol_nan(K)
    assert np.max(np.abs(L - Lo)) <= 1e-9
    Li = np.empty((n, n))
    assert lib.bobe_debug_linv(gp._h, _lib.ptr(Li)) == 0
    assert np.max(np.abs(Li @ Lo - np.eye(n))) <= 1e-7
    ys = (y - y.mean()) / y.std()
    mll_cpu, g_cpu = O.cycle_value_and_grad(X, ys, ls, kv, 1e-5)
    mll_gpu, g_gpu = gp.mll_data(ls, kv)
    assert abs(mll_gpu - mll_cpu) <= 1e-10 * abs(mll_cpu)
    assert np.max(np.abs(g_gpu - g_cpu)) <= 1e-8 * np.max(np.abs(g_cpu))
    mb, gb = gp.mll_data_batch(np.tile(ls, (3, 1)) * np.array([[1.0], [0.9], [1.1]]), np.array([kv, kv, 1.0]))
    assert mb[0] == mll_gpu and np.array_equal(gb[0], g_gpu)


@pytest.mark.parametrize("kernel,d", [("rbf", 1), ("matern", 1), ("rbf", 32), ("matern", 32)])
def test_dimension_limits(kernel, d):
    """d = 1 and d = 32 (the library's maximum): value, gradient, posterior and sweep against the oracle."""
    n = 90
    X, y = smooth_data(n, d, seed=d)
    ls = np.full(d, 0.5 if d == 1 else 2.0) * (1.0 + 0.01 * np.arange(d))
    gp, og = both(X, y, noise=1e-6, kernel=kernel, lengthscales=ls, kernel_variance=0.9)
    th = np.log(gp.get_hyperparams())
    f, g = gp.neg_mll_value_and_grad(th)
    fo, go = og.neg_mll_value_and_grad(th)
    assert abs(f - fo) <= 1e-10 * abs(fo) and np.max(np.abs(g - go)) <= 1e-8 * np.max(np.abs(go))
    rng = np.random.default_rng(3)
    cand, Z = rng.uniform(size=(130, d)), rng.uniform(size=(33, d))
    r, ro = gp.wip_sweep(cand, Z, want_mean_var=True), O.wip_sweep(og, cand, Z)
    assert np.allclose(r["mean"], ro["mean"], atol=1e-8 * 3)
    assert_var_close(r["var"], ro["var"], 0.9 + 1e-6)
    assert np.all(np.abs(r["wipstd"] - ro["wipstd"]) <= 1e-7 * ro["wipstd"] + 1e-9 * og.y_std)
    assert_argmin(r["argmin_s"], ro["wipstd"])
    with pytest.raises(Exception):
        GP(np.zeros((4, 33)), np.zeros(4))                   # d > 32 is rejected, not truncated


def test_random_small_shapes_against_oracle():
    """Seeded random shapes (N, d, C, M, kernel): every padding / ragged-tile combination of the sweep."""
    rng = np.random.default_rng(2024)
    for case in range(12):
        n, d = int(rng.integers(1, 260)), int(rng.integers(1, 7))
        c, m = int(rng.integers(1, 400)), int(rng.integers(1, 150))
        kernel = "rbf" if case % 2 == 0 else "matern"
        X, y = smooth_data(n, d, seed=100 + case)
        ls = rng.uniform(0.3, 1.2, size=d)
        gp, og = both(X, y, noise=1e-6, kernel=kernel, lengthscales=ls, kernel_variance=float(rng.uniform(0.5, 2.0)))
        cand, Z = rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
        r, ro = gp.wip_sweep(cand, Z, want_mean_var=True), O.wip_sweep(og, cand, Z)
        kself = gp.kernel_variance + 1e-6
        assert r["wipv"].shape == (c,) and r["mean"].shape == (c,), (n, d, c, m)
        assert np.allclose(r["mean"], ro["mean"], atol=1e-8 * 3), (n, d, c, m)
        assert_var_close(r["var"], ro["var"], kself)
        assert np.all(np.abs(r["wipv"] - ro["wipv"]) <= og.y_std ** 2 * (1e-9 * kself + 1e-7 * ro["wipv"] / og.y_std ** 2)), (n, d, c, m)
        assert_argmin(r["argmin_v"], ro["wipv"])
        assert_argmin(r["argmin_s"], ro["wipstd"])


def test_large_n_spot_check():
    """N = 16 384 (2 GiB per matrix, 128 blocks): the factor and the inverse factor on random sub-blocks, and the
    posterior at training points — index arithmetic and padding at a size far beyond the headline."""
    n, d = 16384, 8
    rng = np.random.default_rng(77)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.normal(size=n)
    ls, kv, noise = np.full(d, 0.35), 1.0, 1e-2
    gp = GP(X, y, noise=noise, lengthscales=ls, kernel_variance=kv)
    assert not gp.not_pd
    L = gp.cholesky
    assert L.shape == (n, n) and np.all(np.isfinite(L))
    idx_i = np.sort(rng.choice(n, 192, replace=False))
    idx_j = np.sort(rng.choice(n, 192, replace=False))
    K_ij = O.rbf_kernel(X[idx_i], X[idx_j], ls, kv, noise, include_noise=False)
    K_ij[idx_i[:, None] == idx_j[None, :]] += noise
    assert np.max(np.abs(L[idx_i] @ L[idx_j].T - K_ij)) <= 1e-11
    assert np.all(np.triu(L[:512, :512], 1) == 0) and np.all(np.diag(L)[::97] > 0)
    # alpha solves K alpha = y_standardised: check a random set of rows of K alpha
    ys = (y - y.mean()) / y.std()
    rows = rng.choice(n, 64, replace=False)
    K_rows = O.rbf_kernel(X[rows], X, ls, kv, noise, include_noise=False)
    K_rows[np.arange(64), rows] += noise
    assert np.max(np.abs(K_rows @ gp.alphas.ravel() - ys[rows])) <= 1e-8
    m, v = gp.predict_batched(X[rows])
    assert np.max(np.abs(m - K_rows @ gp.alphas.ravel() + noise * gp.alphas.ravel()[rows])) <= 1e-8
    assert np.all(v > 0) and np.all(v < kv + noise)
    mll, g = gp.mll_data(ls, kv)
    assert np.isfinite(mll) and np.all(np.isfinite(g))


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_hip_path_against_the_plain_c_restatement(kernel):
    """The second, independently written CPU restatement (oracle/bobe_oracle_c.c: scalar loops, explicit inverse,
    literal (N+1)-factor fantasy variance) as the checker."""
    from oracle import c_binding as OC
    kid = 0 if kernel == "rbf" else 1
    n, d = 150, 4
    X, y = smooth_data(n, d, seed=31)
    ls, kv, noise = np.array([0.4, 0.55, 0.7, 0.5]), 1.25, 1e-6
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kv)
    ys = gp.train_y.ravel()
    info, mll_c, grad_c, L_c, alpha_c = OC.mll(kid, X, ys, ls, kv, noise)
    assert info == 0
    mll, grad = gp.mll_data(ls, kv)
    assert abs(mll - mll_c) <= 1e-10 * abs(mll_c)
    assert np.max(np.abs(grad - grad_c)) <= 1e-8 * np.max(np.abs(grad_c))
    assert np.max(np.abs(gp.cholesky - L_c)) <= 1e-10
    rng = np.random.default_rng(2)
    Xq, Z = rng.uniform(size=(40, d)), rng.uniform(size=(25, d))
    m, v = gp.predict_batched(Xq)
    m_c, v_c = OC.predict(kid, X, L_c, alpha_c, ls, kv, noise, Xq)
    assert np.max(np.abs(m - m_c)) <= 1e-8 * 3
    assert_var_close(v, v_c, kv + noise)
    fv = gp.fantasy_var(Xq[:6], Z)
    for i in range(6):
        f_c = OC.fantasy_var(kid, X, L_c, ls, kv, noise, Xq[i], Z, gp.y_std)
        assert np.all(np.abs(fv[i] - f_c) <= gp.y_std ** 2 * (1e-9 * (kv + noise) + 1e-6 * f_c / gp.y_std ** 2))


def test_module_level_kernel_helpers():
    """``from BOBE.gp import rbf_kernel, matern_kernel, kernel_diag`` keeps working (gp.py:98-168)."""
    from bobe_amd.gp import kernel_diag, matern_kernel, rbf_kernel
    rng = np.random.default_rng(6)
    A, B = rng.uniform(size=(37, 5)), rng.uniform(size=(140, 5))
    ls = rng.uniform(0.3, 1.0, size=5)
    assert np.allclose(rbf_kernel(A, B, ls, 1.3, 1e-6, include_noise=False),
                       O.rbf_kernel(A, B, ls, 1.3, 1e-6, include_noise=False), rtol=1e-13, atol=1e-15)
    assert np.allclose(matern_kernel(A, A, ls, 0.7, 1e-3, include_noise=True),
                       O.matern_kernel(A, A, ls, 0.7, 1e-3, include_noise=True), rtol=1e-13, atol=1e-15)
    assert np.array_equal(kernel_diag(A, 1.3, 1e-6), O.kernel_diag(A, 1.3, 1e-6))
    assert np.array_equal(kernel_diag(A, 1.3, 1e-6, include_noise=False), np.full(37, 1.3))


def test_first_order_fit_paths():
    """optimizer != 'scipy' selects the optax-style loop (gp.py:264-267); the vectorised variant drives every
    restart's evaluation through one bobe_gp_mll_batch per step and finds what the sequential loop finds."""
    from bobe_amd.optim import optimize_optax, optimize_optax_vmap
    X, y = ref_data(60, 2)
    gp = GP(X, y, noise=1e-6, optimizer="adam", optimizer_options={"name": "adam", "lr": 0.02, "early_stop_patience": 30})
    assert gp.mll_optimize is optimize_optax
    u0 = np.array([[0.5, 0.5, 0.5], [0.3, 0.6, 0.4], [0.7, 0.4, 0.6]])      # unit coordinates of the log-bounds
    f0 = min(gp.neg_mll(gp.hyperparam_bounds[0] + u * (gp.hyperparam_bounds[1] - gp.hyperparam_bounds[0])) for u in u0)
    r = gp.fit(x0=u0, maxiter=60)
    assert np.isfinite(r["mll"]) and -r["mll"] < f0                          # improved on the best start
    opts = {"name": "adam", "lr": 0.02, "early_stop_patience": 30}
    xs, fs = optimize_optax(gp.neg_mll_value_and_grad, (), {}, gp.num_hyperparams, gp.hyperparam_bounds, u0, dict(opts), 60, 3)
    xv, fv = optimize_optax_vmap(gp.neg_mll_value_and_grad, (), {}, gp.num_hyperparams, gp.hyperparam_bounds, u0,
                                 dict(opts), 60, 3, batch_value_and_grad=gp.neg_mll_value_and_grad_batch)
    assert fv == pytest.approx(fs, rel=1e-12)                                # same arithmetic, batched evaluations
    assert -r["mll"] == pytest.approx(fs, rel=1e-12)


@pytest.mark.parametrize("kernel,d,m", [("rbf", 3, 70), ("matern", 5, 300), ("rbf", 12, 33), ("matern", 9, 33), ("rbf", 17, 33),
                                        ("matern", 17, 33)])
def test_wip_gradient_against_values_and_central_differences(kernel, d, m):
    """bobe_gp_wip_grad: the scores equal the sweep's, the gradients equal central differences of the ORACLE's
    WIPV / WIPStd (the reference differentiates the same functions with jax.grad, acquisition.py:403-412)."""
    n = 160
    X, y = smooth_data(n, d, seed=17)
    ls = np.full(d, 0.6) * (1 + 0.05 * np.arange(d))
    gp, og = both(X, 2.0 * y + 0.5, noise=1e-6, kernel=kernel, lengthscales=ls, kernel_variance=1.4)
    rng = np.random.default_rng(5)
    cand, Z = rng.uniform(0.1, 0.9, size=(9, d)), rng.uniform(size=(m, d))
    wv, ws, dv, dsd = gp.wip_grad(cand, Z)
    r = gp.wip_sweep(cand, Z)
    assert np.allclose(wv, r["wipv"], rtol=1e-10) and np.allclose(ws, r["wipstd"], rtol=1e-10)
    e = 1e-5
    for c in range(3):
        for j in range(d):
            xp, xm = cand[c].copy(), cand[c].copy()
            xp[j] += e
            xm[j] -= e
            ro_p, ro_m = O.wip_sweep(og, xp[None, :], Z), O.wip_sweep(og, xm[None, :], Z)
            fd_v = (ro_p["wipv"][0] - ro_m["wipv"][0]) / (2 * e)
            fd_s = (ro_p["wipstd"][0] - ro_m["wipstd"][0]) / (2 * e)
            assert dv[c, j] == pytest.approx(fd_v, rel=2e-5, abs=1e-9 * og.y_std ** 2)
            assert dsd[c, j] == pytest.approx(fd_s, rel=2e-5, abs=1e-9 * og.y_std)
    # a candidate on top of a training point: s ~ noise, every fantasy variance is at or near its floor -> finite output
    wv0, ws0, dv0, ds0 = gp.wip_grad(X[:2], Z)
    assert np.all(np.isfinite(wv0)) and np.all(np.isfinite(dv0)) and np.all(np.isfinite(ds0))
    # up to 16 candidates take the matrix-vector path, more the batched (tile) path: same numbers from both
    big = np.vstack([cand, X[:2], rng.uniform(0.1, 0.9, size=(9, d))])
    bw = gp.wip_grad(big, Z)
    scale_v, scale_s = np.max(np.abs(bw[2])), np.max(np.abs(bw[3]))
    assert np.allclose(wv, bw[0][:9], rtol=1e-11) and np.allclose(ws, bw[1][:9], rtol=1e-11)
    assert np.allclose(dv, bw[2][:9], rtol=1e-8, atol=1e-7 * scale_v) and np.allclose(dsd, bw[3][:9], rtol=1e-8, atol=1e-7 * scale_s)
    assert np.allclose(wv0, bw[0][9:11], rtol=1e-11) and np.allclose(dv0, bw[2][9:11], rtol=1e-8, atol=1e-7 * scale_v)
    one = gp.wip_grad(cand[4], Z)                                          # a single candidate (what L-BFGS sends)
    assert np.array_equal(one[2][0], dv[4]) and one[0][0] == wv[4]      # a candidate does not depend on its batch


def test_plain_c_host_program_over_the_abi(tmp_path):
    """examples/c_abi_host.c — factor, value + gradient, posterior and the WIPV / WIPStd sweep from a C99 program that
    binds include/bobe_gp.h directly; its own checks (central differences, interpolation, argmin vs scores) must pass."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_lib_cpu import _build_c_host
    exe = _build_c_host(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all checks passed" in p.stdout
