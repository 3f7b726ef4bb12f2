"""Pathwise posterior draws of the surrogate on the device (bobe_gp_paths_* / GP.sample_paths / PosteriorPaths): values against
the long-double truth under the conditioning ladder's rule, the identity at the training points, the device's draw layout,
chunking and pointer kinds, ensemble statistics, the per-path argmax, the snapshot rule, memory, errors, and the consumers
(Thompson batches, the evidence distribution over all samples).

Figures measured on an MI355X are in the docstrings of the tests they belong to."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from paths_restatement import (TruthLD, device_arrays, ensemble_moments, features, paths_fp64,  # noqa: E402
                               spectral_frequencies)
from posterior_restatement import kernel  # noqa: E402

pytestmark = pytest.mark.gpu


def _gp(n, d, kernel="rbf", noise=1e-4, kvar=1.3, seed=0, ls=None):
    """the settings of tests/test_gpu_posterior_draws.py::_gp"""
    from bobe_amd import GP
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, -1]) + 0.1 * rng.standard_normal(n)
    ls = np.full(d, 0.3 * math.sqrt(d)) if ls is None else np.asarray(ls, dtype=float)
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar), X, ls


def _caller_arrays(kind, S, F, N, d, noise, seed):
    rng = np.random.default_rng(seed)
    u, phase = spectral_frequencies(kind, F, d, rng)
    return {"u": u, "phase": phase, "w": rng.standard_normal((S, F)), "eps": math.sqrt(noise) * rng.standard_normal((S, N))}


def _eval_std(ps, Q, centered=False):
    """bobe_gp_paths_eval itself: standardised units, no host arithmetic"""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    out = np.empty((ps.n_paths, len(Q)))
    assert ps._lib.bobe_gp_paths_eval(ps._h, Q.ctypes.data, len(Q), 1 if centered else 0, out.ctypes.data) == 0
    return out


def _err(a, truth):
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - truth)))


SIZES = [(1, 10, 1, 1), (50, 200, 5, 127), (130, 200, 5, 257), (400, 512, 20, 150), (600, 1000, 129, 300)]
VALUE_CASES = [(n, f, s, c, k, d) for (n, f, s, c) in SIZES for k in ("rbf", "matern") for d in (2, 8, 32)]


@pytest.mark.parametrize("n,f,s,c,kind,d", VALUE_CASES, ids=[f"N{n}_F{f}_S{s}_C{c}_{k}_d{d}" for n, f, s, c, k, d in VALUE_CASES])
def test_values_with_caller_arrays(n, f, s, c, kind, d):
    """err(device) <= 4 err(fp64 cho_solve restatement) + 1e-10 scale against the long-double path, scale = 1 + max |truth|, for
    the values and the centred values, with the default refine switch, the plain product and the forced substitution.

    Measured on an MI355X over all cases: device at most 2.9e-11 scale (N = 600), the restatement at most 4.5e-11 scale."""
    gp, X, ls = _gp(n, d, kind, seed=n + d)
    Q = np.random.default_rng(7 + c).uniform(size=(c, d))
    y = np.asarray(gp.train_y).reshape(-1)
    arr = _caller_arrays(kind, s, f, n, d, gp.noise, seed=11 * n + d)
    truth = TruthLD(kind, X, y, ls, gp.kernel_variance, gp.noise)
    refs = {}
    for cen in (False, True):
        t = truth.paths(Q, centered=cen, **arr)
        r = paths_fp64(kind, X, y, Q, ls, gp.kernel_variance, gp.noise, centered=cen, **arr)
        refs[cen] = (t, 1.0 + float(np.max(np.abs(t))), _err(r, t))
    for kappa in (None, -1.0, 0.0):
        if kappa is not None:
            gp.refine_kappa = kappa
            gp.recompute_cholesky()
            assert gp.refining == (kappa == 0.0)
        with gp.sample_paths(s, f, **arr) as ps:
            for cen in (False, True):
                t, scale, e_ref = refs[cen]
                e_dev = _err(_eval_std(ps, Q, cen), t)
                print(f"kappa={kappa} centered={cen}: device {e_dev / scale:.3g} restatement {e_ref / scale:.3g} (x scale)")
                assert e_dev <= 4.0 * e_ref + 1e-10 * scale, (kappa, cen, e_dev, e_ref, scale)
            # physical units of the wrapper
            phys = ps.evaluate(Q)
            np.testing.assert_allclose(phys, gp.y_mean + gp.y_std * _eval_std(ps, Q), rtol=1e-15, atol=0)


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_identity_at_the_training_points(kind):
    """f_s(X) = y - eps_s - noise v_s: the feature part cancels at the training points (it stays only in the small term noise
    v_s); same rule as the value test, for two sets of features."""
    n, d, s, f = 400, 8, 20, 512
    gp, X, ls = _gp(n, d, kind, seed=21)
    y = np.asarray(gp.train_y).reshape(-1)
    arr = _caller_arrays(kind, s, f, n, d, gp.noise, seed=5)
    arr2 = dict(arr, **dict(zip(("u", "phase"), spectral_frequencies(kind, f, d, np.random.default_rng(99)))))
    truth = TruthLD(kind, X, y, ls, gp.kernel_variance, gp.noise)
    LD = np.longdouble
    for a in (arr, arr2):
        t = (np.asarray(y, dtype=LD)[:, None] - np.asarray(a["eps"], dtype=LD).T - LD(gp.noise) * truth.v(**a)).T
        scale = 1.0 + float(np.max(np.abs(t)))
        e_ref = _err(paths_fp64(kind, X, y, X, ls, gp.kernel_variance, gp.noise, **a), t)
        with gp.sample_paths(s, f, **a) as ps:
            e_dev = _err(_eval_std(ps, X), t)
        print(f"device {e_dev / scale:.3g} restatement {e_ref / scale:.3g} (x scale)")
        assert e_dev <= 4.0 * e_ref + 1e-10 * scale, (e_dev, e_ref, scale)


def _law_holds(kind, d, u, phase, kvar=1.3):
    F = len(phase)
    P = np.random.default_rng(3).uniform(size=(30, d))
    ls = np.full(d, 0.3 * math.sqrt(d))
    Phi = features(P / ls, u, phase, kvar)
    dev = float(np.max(np.abs(Phi @ Phi.T - kernel(kind, P, P, ls, kvar)))) / (kvar / math.sqrt(F))
    print(f"{kind} d={d}: max |Phi Phi^T - k| = {dev:.2f} sigma^2 / sqrt(F)")
    return dev <= 8.0


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_device_draws_replay_and_determinism(kind):
    """The arrays equal the restatement's replay to 1e-13 relative, a set made from the replayed arrays has the seeded set's
    values to 1e-13 scale, the same seed gives the same bits, another seed differs.

    Shape: the replayed arrays differ from the device's in the last bits (two math libraries), and the values see that
    difference times cond(K).  At d = 32 (cond(K) ~ 6e2 with these settings) moving every replayed entry by one ulp moves the
    fp64 restatement itself by 6e-15 scale, well inside the bound; at d = 3 (cond(K) ~ 8e5) the same one-ulp change moves the
    restatement by 2.7e-12 scale, so no implementation could meet the bound there and that shape cannot check it."""
    n, d, s, f = 130, 32, 7, 200
    gp, X, ls = _gp(n, d, kind, seed=9)
    Q = np.random.default_rng(4).uniform(size=(257, d))
    with gp.sample_paths(s, f, seed=2024) as a, gp.sample_paths(s, f, seed=2024) as b, gp.sample_paths(s, f, seed=2025) as c:
        arr = a.arrays()
        rep = device_arrays(2024, s, f, n, d, kind, gp.noise)
        for k in ("u", "phase", "w", "eps"):
            assert arr[k].shape == rep[k].shape
            np.testing.assert_allclose(arr[k], rep[k], rtol=1e-13, atol=1e-13 * float(np.max(np.abs(rep[k]))), err_msg=k)
            assert np.array_equal(arr[k], b.arrays()[k]), k
        fa = _eval_std(a, Q)
        assert np.array_equal(fa, _eval_std(b, Q))
        assert not np.array_equal(fa, _eval_std(c, Q))
        assert not np.array_equal(arr["w"], c.arrays()["w"])
        # a set made from those arrays reproduces the seeded set
        with gp.sample_paths(s, f, **rep) as r:
            fr = _eval_std(r, Q)
        assert np.max(np.abs(fa - fr)) <= 1e-13 * (1.0 + np.max(np.abs(fr)))
        # a mix: the caller's w, everything else drawn
        with gp.sample_paths(s, f, seed=2024, w=rep["w"]) as m:
            got = m.arrays()
            assert np.array_equal(got["w"], rep["w"]) and np.array_equal(got["u"], arr["u"])
            assert np.array_equal(got["eps"], arr["eps"])


@pytest.mark.parametrize("kind,d", [("rbf", 2), ("rbf", 8), ("matern", 2), ("matern", 8)])
def test_device_frequencies_follow_the_kernel_law(kind, d):
    """max |Phi Phi^T - k| <= 8 sigma^2 / sqrt(F) at 30 points with the device's F = 65 536 frequencies and phases.
    Measured on an MI355X: 1.9 (rbf, d = 2), 2.7 (rbf, 8), 1.9 (matern, 2), 2.6 (matern, 8) in these units."""
    gp, X, ls = _gp(20, d, kind, seed=2)
    with gp.sample_paths(1, 65536, seed=17) as ps:
        arr = ps.arrays()
    assert np.all(arr["phase"] >= 0.0) and np.all(arr["phase"] < 2.0 * math.pi)
    assert _law_holds(kind, d, arr["u"], arr["phase"])


def test_chunking_and_pointer_kinds():
    import torch
    n, d, s, f, c = 130, 8, 20, 200, 300
    gp, X, ls = _gp(n, d, "matern", seed=6)
    Q = np.random.default_rng(8).uniform(size=(c, d))
    lib = gp._lib
    with gp.sample_paths(s, f, seed=3) as ps:
        one = _eval_std(ps, Q)
        one_c = _eval_std(ps, Q, True)
        assert lib.bobe_gp_set_chunk(gp._h, 128) == 0
        try:
            assert np.array_equal(_eval_std(ps, Q), one)
            assert np.array_equal(_eval_std(ps, Q, True), one_c)
        finally:
            assert lib.bobe_gp_set_chunk(gp._h, 0) == 0
        # device pointers: the same bits
        xd = torch.tensor(Q, dtype=torch.float64, device="cuda")
        out_d = torch.empty((s, c), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert lib.bobe_gp_paths_eval(ps._h, xd.data_ptr(), c, 0, out_d.data_ptr()) == 0
        assert np.array_equal(out_d.cpu().numpy(), one)
        assert np.array_equal(ps.evaluate(xd), ps.evaluate(Q))
        arr = ps.arrays()
        dev = {k: torch.tensor(v, dtype=torch.float64, device="cuda") for k, v in arr.items()}
        torch.cuda.synchronize()
        with gp.sample_paths(s, f, **dev) as pd, gp.sample_paths(s, f, **arr) as ph:
            assert np.array_equal(_eval_std(pd, Q), _eval_std(ph, Q))


def test_path_statistics():
    """Mean and covariance of 20 000 paths within 6 standard errors of the exact ensemble moments for the realised features
    (the threshold of test_draw_statistics).  Measured on an MI355X: mean 0.62, covariance 3.12 standard errors."""
    n, d, f, s = 40, 2, 256, 20000
    gp, X, ls = _gp(n, d, seed=5, noise=1e-3)
    Q = np.random.default_rng(6).uniform(size=(6, d))
    with gp.sample_paths(s, f, seed=77) as ps:
        arr = ps.arrays()
        dr = _eval_std(ps, Q)
    m, S = ensemble_moments("rbf", X, np.asarray(gp.train_y).reshape(-1), Q, ls, gp.kernel_variance, gp.noise, arr["u"],
                            arr["phase"])
    sd = np.sqrt(np.diag(S))
    zm = np.max(np.abs(dr.mean(0) - m) / (sd / math.sqrt(s)))
    emp = np.cov(dr, rowvar=False)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / s)
    zc = np.max(np.abs(emp - S) / se)
    print(f"mean {zm:.2f} covariance {zc:.2f} standard errors")
    assert zm <= 6.0 and zc <= 6.0


@pytest.mark.parametrize("s", [5, 40, 129])
@pytest.mark.parametrize("c", [129, 300])
def test_argmax(s, c):
    """argmax equals the argmax of evaluate (+ bias) wherever the top two differ by more than 1e-12 scale; best equals the
    maximum to that bound; one and three chunks."""
    n, d, f = 130, 8, 200
    gp, X, ls = _gp(n, d, "rbf", seed=12)
    Q = np.random.default_rng(c).uniform(size=(c, d))
    bias = np.random.default_rng(s).gumbel(size=(s, c))
    lib = gp._lib
    with gp.sample_paths(s, f, seed=31) as ps:
        fv = _eval_std(ps, Q)
        for b in (None, bias):
            tot = fv if b is None else fv + b
            scale = 1.0 + float(np.max(np.abs(tot)))
            srt = np.sort(tot, axis=1)
            clear = (srt[:, -1] - srt[:, -2]) > 1e-12 * scale
            for chunk in (0, 128):
                assert lib.bobe_gp_set_chunk(gp._h, chunk) == 0
                try:
                    idx = np.full(s, -1, dtype=np.int64)
                    best = np.empty(s)
                    bp = None if b is None else b.ctypes.data
                    assert lib.bobe_gp_paths_argmax(ps._h, Q.ctypes.data, c, bp, idx.ctypes.data, best.ctypes.data) == 0
                finally:
                    assert lib.bobe_gp_set_chunk(gp._h, 0) == 0
                assert np.all((idx >= 0) & (idx < c))
                assert np.array_equal(idx[clear], np.argmax(tot, axis=1)[clear])
                assert np.max(np.abs(best - tot.max(axis=1))) <= 1e-12 * scale
                assert np.max(np.abs(best - tot[np.arange(s), idx])) <= 1e-12 * scale
        i2, v2 = ps.argmax(Q, bias)
        assert np.array_equal(i2, idx) and np.allclose(v2, gp.y_mean + gp.y_std * best, rtol=1e-15, atol=0)


def test_argmax_ties_take_the_lower_index():
    n, d, s, f = 50, 2, 5, 200
    gp, X, ls = _gp(n, d, seed=14)
    base = np.random.default_rng(2).uniform(size=(150, d))
    Q = np.vstack([base, base])                        # row i + 150 duplicates row i: the same bits in both
    with gp.sample_paths(s, f, seed=4) as ps:
        fv = _eval_std(ps, Q)
        assert np.array_equal(fv[:, :150], fv[:, 150:])
        idx, _ = ps.argmax(Q)
        assert np.array_equal(idx, np.argmax(fv[:, :150], axis=1))
        assert gp._lib.bobe_gp_set_chunk(gp._h, 128) == 0
        try:
            idx3, _ = ps.argmax(Q)
        finally:
            assert gp._lib.bobe_gp_set_chunk(gp._h, 0) == 0
        assert np.array_equal(idx3, idx)


def test_snapshot_and_memory():
    import torch
    n, d, s, f = 500, 3, 16, 512
    gp, X, ls = _gp(n, d, seed=2)
    Q = np.random.default_rng(9).uniform(size=(1000, d))
    # a snapshot: an update of the parent (new data, new standardisation, new factor) leaves the set's values alone
    ps = gp.sample_paths(s, f, seed=1)
    before = ps.evaluate(Q)
    before_c = ps.evaluate(Q, centered=True)
    xn = np.random.default_rng(10).uniform(size=(3, d))
    gp.update(xn, np.array([[2.0], [-1.0], [0.5]]))
    assert gp.npoints == n + 3
    assert np.array_equal(ps.evaluate(Q), before) and np.array_equal(ps.evaluate(Q, centered=True), before_c)
    ps.close()
    ps.close()
    with pytest.raises(ValueError):
        ps.evaluate(Q)
    # memory: create, evaluate at many points, close
    xd = torch.tensor(np.random.default_rng(11).uniform(size=(65536, d)), dtype=torch.float64, device="cuda")
    with gp.sample_paths(s, f, seed=1) as warm:
        warm.argmax(xd[:256])
        warm.evaluate(xd[:256])
    gp._lib.bobe_gp_sync(gp._h)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    ps = gp.sample_paths(s, f, seed=1)
    vals = ps.evaluate(xd)
    idx, best = ps.argmax(xd)
    assert vals.shape == (s, 65536) and np.array_equal(np.argmax(vals, axis=1), idx)
    ps.close()
    gp._lib.bobe_gp_sync(gp._h)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) <= 64 << 20, (free0, free1)
    # the finaliser: a dropped set returns its memory too, and a GP dropped first closes its sets
    ps = gp.sample_paths(s, f, seed=1)
    del ps
    import gc
    gc.collect()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert abs(free2 - free0) <= 64 << 20, (free0, free2)


def test_error_contract():
    from bobe_amd import GP, BobeLibraryError, _lib
    lib = _lib.load()
    xq = np.random.default_rng(0).uniform(size=(10, 2))
    out = np.empty((4, 10))
    idx = np.empty(4, dtype=np.int64)
    best = np.empty(4)
    # no factorised state
    h = C.c_void_p(0)
    assert lib.bobe_gp_create(C.byref(h), 0, 0, 2) == 0
    try:
        p = C.c_void_p(123)
        assert lib.bobe_gp_paths_create(h, 4, 16, 0, None, None, None, None, C.byref(p)) == -3
        assert not p.value
    finally:
        lib.bobe_gp_destroy(h)
    gp, X, _ = _gp(30, 2, seed=1)
    g = gp._h
    for s, f in ((0, 16), (-1, 16), (4, 0), (4, 65537), (4, -3)):
        p = C.c_void_p(123)
        assert lib.bobe_gp_paths_create(g, s, f, 0, None, None, None, None, C.byref(p)) == -1
        assert not p.value
    assert lib.bobe_gp_paths_create(g, 4, 16, 0, None, None, None, None, None) == -1
    p = C.c_void_p(0)
    assert lib.bobe_gp_paths_create(g, 4, 65536, 0, None, None, None, None, C.byref(p)) == 0 and p.value
    lib.bobe_gp_paths_destroy(p)
    p = C.c_void_p(0)
    assert lib.bobe_gp_paths_create(g, 4, 16, 0, None, None, None, None, C.byref(p)) == 0 and p.value
    try:
        assert lib.bobe_gp_paths_eval(p, xq.ctypes.data, 10, 0, None) == -1
        assert lib.bobe_gp_paths_eval(p, None, 10, 0, out.ctypes.data) == -1
        assert lib.bobe_gp_paths_eval(p, xq.ctypes.data, 0, 0, out.ctypes.data) == -1
        assert lib.bobe_gp_paths_eval(None, xq.ctypes.data, 10, 0, out.ctypes.data) == -1
        assert lib.bobe_gp_paths_argmax(p, xq.ctypes.data, 10, None, None, best.ctypes.data) == -1
        assert lib.bobe_gp_paths_argmax(p, xq.ctypes.data, 10, None, idx.ctypes.data, None) == -1
        assert lib.bobe_gp_paths_argmax(p, xq.ctypes.data, 0, None, idx.ctypes.data, best.ctypes.data) == -1
        assert lib.bobe_gp_paths_get(None, None, None, None, None) == -1
        assert lib.bobe_gp_paths_get(p, None, None, None, None) == 0
        assert lib.bobe_gp_paths_eval(p, xq.ctypes.data, 10, 0, out.ctypes.data) == 0 and np.all(np.isfinite(out))
    finally:
        lib.bobe_gp_paths_destroy(p)
    lib.bobe_gp_paths_destroy(None)
    # a NaN factor: duplicated training points without noise - no set, BOBE_NOT_PD
    Xd = np.vstack([X[:5], X[:5]])
    bad = GP(Xd, np.arange(10.0), noise=0.0, lengthscales=[0.3, 0.3], kernel_variance=1.0, pivot_floor_ulp=64)
    assert bad.not_pd
    p = C.c_void_p(123)
    assert lib.bobe_gp_paths_create(bad._h, 4, 16, 0, None, None, None, None, C.byref(p)) == _lib.BOBE_NOT_PD
    assert not p.value
    with pytest.raises(BobeLibraryError):
        bad.sample_paths(4, 16)
    # the parent's own state is untouched by a set's calls
    m0, v0 = gp._predict(xq, True, True, 0)
    with gp.sample_paths(3, 64, seed=2) as ps:
        ps.evaluate(np.random.default_rng(3).uniform(size=(500, 2)))
        ps.argmax(np.random.default_rng(3).uniform(size=(500, 2)))
    m1, v1 = gp._predict(xq, True, True, 0)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


# ---------------------------------------------------------------------------------------------------------------- consumers
@pytest.mark.parametrize("mode", ["max", "posterior"])
def test_thompson_batches(mode):
    from bobe_amd.acquisition import PathwiseTS
    gp, X, ls = _gp(60, 2, seed=3)
    pool = np.random.default_rng(1).uniform(size=(700, 2))
    kw = {"candidates": pool, "ts_mode": mode, "ts_features": 512}
    acq = PathwiseTS()
    pts, vals = acq.get_next_batch(gp, n_batch=6, acq_kwargs=kw, rng=np.random.default_rng(42))
    assert pts.shape == (6, 2) and vals.shape == (6,) and np.all(np.isfinite(vals))
    rows = [int(np.flatnonzero(np.all(pool == p, axis=1))[0]) for p in pts]          # every pick is a pool row
    assert len(set(rows)) == 6
    pts2, vals2 = acq.get_next_batch(gp, n_batch=6, acq_kwargs=kw, rng=np.random.default_rng(42))
    assert np.array_equal(pts, pts2) and np.array_equal(vals, vals2)                  # reproducible from the generator state
    pts3, _ = acq.get_next_batch(gp, n_batch=6, acq_kwargs=kw, rng=np.random.default_rng(43))
    assert not np.array_equal(pts, pts3)
    # the pool of the sweep mode: all of mc_samples['x']; a pool as small as the batch is used up (the taken rule)
    small = pool[:4]
    pts4, _ = acq.get_next_batch(gp, n_batch=4, acq_kwargs={"mc_samples": {"x": small}, "ts_mode": mode, "ts_features": 64},
                                 rng=np.random.default_rng(1))
    assert sorted(map(tuple, pts4)) == sorted(map(tuple, small))
    x1, v1 = acq.get_next_point(gp, acq_kwargs=kw, rng=np.random.default_rng(5))
    assert x1.shape == (2,) and np.isfinite(v1)
    with pytest.raises(ValueError):
        acq.get_next_batch(gp, n_batch=2, acq_kwargs=dict(kw, ts_mode="nope"), rng=np.random.default_rng(0))


def _sparse_gaussian_gp():
    from scipy.stats import qmc
    from bobe_amd import GP
    X = qmc.Sobol(2, scramble=True, seed=1).random(8)
    return GP(X, -0.5 * np.sum(((X - 0.5) / 0.2) ** 2, axis=1), noise=1e-8, lengthscales=[0.3, 0.3], kernel_variance=1.0)


def test_evidence_draws_by_paths_agree_with_the_joint_draws():
    """Where both methods perturb the same points (fewer than 16 384 samples) their spreads of logZ agree within 6 Monte-Carlo
    standard errors of the two K = 256 estimates (se of a standard deviation: std / sqrt(2 (K - 1))).
    Measured on an MI355X: draws_std 0.1351 (joint) and 0.1291 (paths), 0.73 standard errors apart."""
    from bobe_amd.samplers import nested_sampling
    gp = _sparse_gaussian_gp()
    K = 256
    out = {}
    for method in ("joint", "paths"):
        s, z, ok = nested_sampling(gp, mode="convergence", dlogz=0.05, rng=np.random.default_rng(3), nlive=300,
                                   logz_draws=K, logz_draws_seed=5, logz_draws_method=method)
        out[method] = (s, z)
    (s0, z0), (s1, z1) = out["joint"], out["paths"]
    assert np.array_equal(s0["logl"], s1["logl"])                      # the run itself does not depend on the method
    assert set(z1) == (set(z0) - {"draws_jitter"}) | {"draws_features"}
    n_finite = int(np.sum(np.isfinite(s1["logl"])))
    assert z1["draws_points"] == n_finite == z0["draws_points"] and n_finite < 16384
    assert z1["draws_features"] == 2048 and z1["draws"].shape == (K,)
    se = math.sqrt(z0["draws_std"] ** 2 + z1["draws_std"] ** 2) / math.sqrt(2.0 * (K - 1))
    print(f"draws_std joint {z0['draws_std']:.4f} paths {z1['draws_std']:.4f}: {abs(z0['draws_std'] - z1['draws_std']) / se:.2f} se")
    assert abs(z0["draws_std"] - z1["draws_std"]) <= 6.0 * se
    assert abs(z0["draws_mean"] - z1["draws_mean"]) <= 6.0 * math.hypot(z0["draws_std"], z1["draws_std"]) / math.sqrt(K)


def test_evidence_draws_by_paths_perturb_every_sample(monkeypatch):
    """More than 16 384 samples (a long run by nlive): every finite one is perturbed - a path shifted by c everywhere moves logZ
    by c.  Measured on an MI355X: 23 135 samples, all finite and all perturbed."""
    from bobe_amd import samplers
    from bobe_amd.paths import PosteriorPaths
    gp = _sparse_gaussian_gp()
    nlive = 4000
    s, z, ok = samplers.nested_sampling(gp, mode="convergence", dlogz=0.05, rng=np.random.default_rng(3), nlive=nlive,
                                        logz_draws=4, logz_draws_seed=5, logz_draws_method="paths")
    n_finite = int(np.sum(np.isfinite(s["logl"])))
    print(f"{len(s['logl'])} samples, {n_finite} finite, draws_std {z['draws_std']:.4f}")
    assert z["draws_points"] == n_finite > 16384
    assert np.all(np.isfinite(z["draws"])) and z["draws_std"] > 0
    # the replay of the run's volumes (tests/test_gpu_posterior_draws.py::_replay)
    niter, logl = z["niter"], s["logl"]
    logvol_dead = -np.arange(1, niter + 1) / nlive
    logvol = np.concatenate([logvol_dead, logvol_dead[-1] + np.log1p(-(np.arange(nlive) + 1.0) / (nlive + 1.0))])
    n = gp.npoints
    zero = {"u": np.random.default_rng(0).standard_normal((64, 2)), "phase": np.zeros(64), "w": np.zeros((3, 64)),
            "eps": np.zeros((3, n))}
    with gp.sample_paths(3, 64, **zero) as ps:                             # zero weights and noise: the centred paths are 0
        assert np.array_equal(ps.evaluate(s["x"][:1000], centered=True), np.zeros((3, 1000)))
    base = samplers.logz_from_samples(gp, s["x"], logl, logvol, z["mean"], z["dlogz_sampler"], n_draws=3, draws_method="paths",
                                      draws_features=64, draws_arrays=zero)
    z_plain = samplers.compute_integrals(logl=logl, logvol=logvol)[-1]
    assert np.array_equal(base["draws"], np.full(3, z_plain))               # (their std is rounding of the mean at most)
    c = 0.75
    orig = PosteriorPaths.evaluate
    monkeypatch.setattr(PosteriorPaths, "evaluate", lambda self, x, centered=False: orig(self, x, centered) + c)
    moved = samplers.logz_from_samples(gp, s["x"], logl, logvol, z["mean"], z["dlogz_sampler"], n_draws=3, draws_method="paths",
                                       draws_features=64, draws_arrays=zero)
    assert np.max(np.abs(moved["draws"] - (z_plain + c))) <= 1e-12 * (1.0 + abs(z_plain))


def test_bo_run_with_thompson_batches():
    """Twelve iterations of BOBE.run(acq='ts') on a 2-D Gaussian: the run finishes and every design point lies in the unit cube."""
    from bobe_amd.acquisition import PathwiseTS
    from bobe_amd.bo import _ACQ, BOBE
    assert _ACQ["ts"] is PathwiseTS

    def gaussian(x):
        return float(-0.5 * np.sum(((np.asarray(x) - 0.3) / 0.4) ** 2))
    bounds = np.array([[-2.0, 2.0], [-2.0, 2.0]]).T
    bobe = BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False)
    res = bobe.run(acq="ts", max_evals=32, fit_n_points=4, batch_size=2, mc_points_size=64, num_mc_samples=256,
                   mc_points_method="uniform")
    assert isinstance(bobe.acquisition, PathwiseTS)
    assert bobe.current_iteration == 12 and len(res["acq_history"]) == 12 and all(np.isfinite(res["acq_history"]))
    tx = np.asarray(res["gp"].train_x)
    assert 8 < len(tx) <= 32 and np.all((tx >= 0.0) & (tx <= 1.0))
    assert res["best_val"] > -2.0                                   # (the maximum is 0; the initial design alone reaches about -0.3)
