"""Input gradients of posterior paths and the per-path maximiser on the device (bobe_gp_paths_grad /
PosteriorPaths.value_and_grad / PosteriorPaths.maximize / PathwiseTS with ``ts_polish``): values and gradients against the
long-double truth under the conditioning ladder's rule, the invariance of a point's bits, the snapshot rule, memory, the
error contract, the maximiser's guarantees and the polished Thompson batches.

Figures measured on an MI355X are in the docstrings of the tests they belong to."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from paths_grad_restatement import value_and_grad_fp64, value_and_grad_ld, weights_ld  # noqa: E402
from paths_restatement import TruthLD, spectral_frequencies  # noqa: E402

pytestmark = pytest.mark.gpu


def _gp(n, d, kernel="rbf", noise=1e-4, kvar=1.3, seed=0):
    """the settings of tests/test_gpu_paths.py::_gp"""
    from bobe_amd import GP
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, -1]) + 0.1 * rng.standard_normal(n)
    ls = np.full(d, 0.3 * math.sqrt(d))
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar), X, ls


def _caller_arrays(kind, S, F, N, d, noise, seed):
    rng = np.random.default_rng(seed)
    u, phase = spectral_frequencies(kind, F, d, rng)
    return {"u": u, "phase": phase, "w": rng.standard_normal((S, F)), "eps": math.sqrt(noise) * rng.standard_normal((S, N))}


def _queries(X, S, T, d, seed):
    """T points uniform in the cube, one of them a corner and one a training point (the Matern r = 0 guard) where T allows;
    path indices unsorted, with repeats, the last path never used (S > 1)"""
    rng = np.random.default_rng(seed)
    Q = rng.uniform(size=(T, d))
    if T >= 3:
        Q[1] = 1.0
        Q[2] = X[len(X) // 2]
    idx = rng.integers(0, max(S - 1, 1), size=T).astype(np.int64)
    if S >= 3 and T >= 3:
        idx[0], idx[-1], idx[1] = S - 2, 0, 0
        assert np.any(np.diff(idx) < 0) and len(set(idx.tolist())) < T and S - 1 not in idx
    return np.ascontiguousarray(Q), idx


def _grad_std(ps, Q, idx, centered=False, want_f=True, want_df=True):
    """bobe_gp_paths_grad itself: standardised units, host pointers, no host arithmetic"""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    t, d = Q.shape
    f, df = np.full(t, np.nan), np.full((t, d), np.nan)
    rc = ps._lib.bobe_gp_paths_grad(ps._h, Q.ctypes.data, t, idx.ctypes.data, 1 if centered else 0,
                                    f.ctypes.data if want_f else None, df.ctypes.data if want_df else None)
    assert rc == 0, rc
    return f, df


def _err(a, truth):
    return float(np.max(np.abs(np.asarray(a, dtype=np.longdouble) - truth)))


SIZES = [(1, 10, 1, 1), (50, 200, 5, 7), (130, 300, 3, 5), (257, 513, 129, 260)]
CASES = [(n, f, s, t, k, d) for (n, f, s, t) in SIZES for k in ("rbf", "matern") for d in (2, 9, 17, 32)]


@pytest.mark.parametrize("n,f,s,t,kind,d", CASES, ids=[f"N{n}_F{f}_S{s}_T{t}_{k}_d{d}" for n, f, s, t, k, d in CASES])
def test_values_and_gradients_against_the_long_double_truth(n, f, s, t, kind, d):
    """err(device) <= 4 err(fp64 cho_solve restatement) + 1e-10 scale against the long-double truth, scale = 1 + max |truth|,
    separately for the values and the gradients, centred and uncentred; at N = 130 also with the plain product
    (refine_kappa = -1) and the forced substitution (refine_kappa = 0).

    Measured on an MI355X over all cases (the largest at d = 2, where cond(K) is largest): values - device at most 1.5e-11
    scale, the restatement 1.9e-11 scale; gradients - device at most 1.3e-11 scale, the restatement 3.6e-11 scale."""
    gp, X, ls = _gp(n, d, kind, seed=n + d)
    y = np.asarray(gp.train_y).reshape(-1)
    arr = _caller_arrays(kind, s, f, n, d, gp.noise, seed=11 * n + d)
    Q, idx = _queries(X, s, t, d, seed=7 + t)
    truth = TruthLD(kind, X, y, ls, gp.kernel_variance, gp.noise)
    refs = {}
    for cen in (False, True):
        tf, tg = value_and_grad_ld(truth, Q, idx, centered=cen, **arr)
        rf, rg = value_and_grad_fp64(kind, X, y, Q, idx, ls, gp.kernel_variance, gp.noise, centered=cen, **arr)
        refs[cen] = ((tf, 1.0 + float(np.max(np.abs(tf))), _err(rf, tf)), (tg, 1.0 + float(np.max(np.abs(tg))), _err(rg, tg)))
    for kappa in ((None, -1.0, 0.0) if n == 130 else (None,)):
        if kappa is not None:
            gp.refine_kappa = kappa
            gp.recompute_cholesky()
            assert gp.refining == (kappa == 0.0)
        with gp.sample_paths(s, f, **arr) as ps:
            for cen in (False, True):
                got = _grad_std(ps, Q, idx, cen)
                for name, g, (tr, scale, e_ref) in zip(("value", "gradient"), got, refs[cen]):
                    e_dev = _err(g, tr)
                    print(f"kappa={kappa} centered={cen} {name}: device {e_dev / scale:.3g} restatement {e_ref / scale:.3g} (x scale)")
                    assert e_dev <= 4.0 * e_ref + 1e-10 * scale, (kappa, cen, name, e_dev, e_ref, scale)
            # physical units of the wrapper
            pf, pg = ps.value_and_grad(Q, idx)
            sf, sg = _grad_std(ps, Q, idx)
            assert np.array_equal(pf, gp.y_mean + gp.y_std * sf) and np.array_equal(pg, gp.y_std * sg)
            cf, cg = ps.value_and_grad(Q, idx, centered=True)
            sf, sg = _grad_std(ps, Q, idx, True)
            assert np.array_equal(cf, gp.y_std * sf) and np.array_equal(cg, gp.y_std * sg)


@pytest.mark.parametrize("kind,d", [("rbf", 9), ("matern", 32)])
def test_value_agrees_with_the_evaluation_product(kind, d):
    """the value of the gradient call and bobe_gp_paths_eval are the same function (two summation orders): 1e-11 scale"""
    gp, X, ls = _gp(130, d, kind, seed=4)
    with gp.sample_paths(6, 300, seed=9) as ps:
        Q, idx = _queries(X, 6, 40, d, seed=1)
        f, _ = ps.value_and_grad(Q, idx)
        full = ps.evaluate(Q)
        assert np.max(np.abs(f - full[idx, np.arange(len(idx))])) <= 1e-11 * (1.0 + np.max(np.abs(full)))


def test_a_points_bits_do_not_depend_on_the_call():
    """(f, df) of a point: alone, inside a call of 260 points, in another position, from host or device pointers, with f or df
    NULL - the same bits."""
    import torch
    n, f, s, t, d = 257, 513, 129, 260, 9
    gp, X, ls = _gp(n, d, "matern", seed=3)
    with gp.sample_paths(s, f, seed=5) as ps:
        Q, idx = _queries(X, s, t, d, seed=2)
        f_all, g_all = _grad_std(ps, Q, idx)
        assert np.all(np.isfinite(f_all)) and np.all(np.isfinite(g_all))
        for i in (0, 2, 17, 259):                                          # alone (row 2 is a training point)
            f1, g1 = _grad_std(ps, Q[i:i + 1], idx[i:i + 1])
            assert f1[0] == f_all[i] and np.array_equal(g1[0], g_all[i]), i
        perm = np.random.default_rng(0).permutation(t)                     # another position
        fp, gp_ = _grad_std(ps, Q[perm], idx[perm])
        assert np.array_equal(fp, f_all[perm]) and np.array_equal(gp_, g_all[perm])
        for cen in (False, True):                                          # a NULL output changes nothing else
            fc, gc = _grad_std(ps, Q, idx, cen)
            f_only, nog = _grad_std(ps, Q, idx, cen, want_df=False)
            nof, g_only = _grad_std(ps, Q, idx, cen, want_f=False)
            assert np.array_equal(f_only, fc) and np.array_equal(g_only, gc)
            assert np.all(np.isnan(nog)) and np.all(np.isnan(nof))
        assert not np.array_equal(fc, f_all)                               # (the centred flag does change them)
        # device pointers, all three
        xd = torch.tensor(Q, dtype=torch.float64, device="cuda")
        fd = torch.empty(t, dtype=torch.float64, device="cuda")
        gd = torch.empty((t, d), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert ps._lib.bobe_gp_paths_grad(ps._h, xd.data_ptr(), t, idx.ctypes.data, 0, fd.data_ptr(), gd.data_ptr()) == 0
        assert np.array_equal(fd.cpu().numpy(), f_all) and np.array_equal(gd.cpu().numpy(), g_all)
        # mixed: device queries, host outputs, through the wrapper
        pf, pg = ps.value_and_grad(xd, idx)
        hf, hg = ps.value_and_grad(Q, idx)
        assert np.array_equal(pf, hf) and np.array_equal(pg, hg)
        # one index for every row
        f7, g7 = ps.value_and_grad(Q[:5], 7)
        f7b, g7b = ps.value_and_grad(Q[:5], np.full(5, 7))
        assert np.array_equal(f7, f7b) and np.array_equal(g7, g7b)


def test_snapshot_and_memory():
    import torch
    n, d, s, f = 500, 3, 16, 512
    gp, X, ls = _gp(n, d, seed=2)
    Q, idx = _queries(X, s, 300, d, seed=9)
    ps = gp.sample_paths(s, f, seed=1)
    before = ps.value_and_grad(Q, idx)
    before_c = ps.value_and_grad(Q, idx, centered=True)
    gp.update(np.random.default_rng(10).uniform(size=(3, d)), np.array([[2.0], [-1.0], [0.5]]))
    assert gp.npoints == n + 3
    for a, b in zip(before + before_c, ps.value_and_grad(Q, idx) + ps.value_and_grad(Q, idx, centered=True)):
        assert np.array_equal(a, b)
    ps.close()
    ps.close()
    with pytest.raises(ValueError):
        ps.value_and_grad(Q, idx)
    with pytest.raises(ValueError):
        ps.maximize(np.zeros((s, 1, d)))
    # memory: create, take gradients (the transposed coefficients are made), close - the bound of tests/test_gpu_paths.py
    with gp.sample_paths(s, f, seed=1) as warm:
        warm.value_and_grad(Q, idx)
    gp._lib.bobe_gp_sync(gp._h)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    ps = gp.sample_paths(s, f, seed=1)
    big = np.random.default_rng(11).uniform(size=(4096, d))
    vals, grads = ps.value_and_grad(big, np.arange(4096) % s)
    assert vals.shape == (4096,) and grads.shape == (4096, d) and np.all(np.isfinite(grads))
    ps.close()
    gp._lib.bobe_gp_sync(gp._h)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) <= 64 << 20, (free0, free1)


def test_error_contract():
    gp, X, _ = _gp(30, 2, seed=1)
    lib = gp._lib
    xq = np.random.default_rng(0).uniform(size=(10, 2))
    idx = np.arange(10, dtype=np.int64) % 4
    f, df = np.empty(10), np.empty((10, 2))
    with gp.sample_paths(4, 16, seed=0) as ps:
        p = ps._h
        args = (xq.ctypes.data, 10, idx.ctypes.data, 0, f.ctypes.data, df.ctypes.data)
        assert lib.bobe_gp_paths_grad(p, *args) == 0
        assert lib.bobe_gp_paths_grad(None, *args) == -1
        assert lib.bobe_gp_paths_grad(p, None, 10, idx.ctypes.data, 0, f.ctypes.data, df.ctypes.data) == -1
        assert lib.bobe_gp_paths_grad(p, xq.ctypes.data, 10, None, 0, f.ctypes.data, df.ctypes.data) == -1
        assert lib.bobe_gp_paths_grad(p, xq.ctypes.data, 10, idx.ctypes.data, 0, None, None) == -1
        for t in (0, -3):
            assert lib.bobe_gp_paths_grad(p, xq.ctypes.data, t, idx.ctypes.data, 0, f.ctypes.data, df.ctypes.data) == -1
        for bad in (4, -1, 1 << 40):
            wrong = idx.copy()
            wrong[7] = bad
            assert lib.bobe_gp_paths_grad(p, xq.ctypes.data, 10, wrong.ctypes.data, 0, f.ctypes.data, df.ctypes.data) == -1
            assert b"path_idx" in lib.bobe_last_error()
        assert lib.bobe_gp_paths_grad(p, xq.ctypes.data, 10, idx.ctypes.data, 0, f.ctypes.data, None) == 0
        assert lib.bobe_gp_paths_grad(p, xq.ctypes.data, 10, idx.ctypes.data, 1, None, df.ctypes.data) == 0
        assert np.all(np.isfinite(f)) and np.all(np.isfinite(df))
        # the parent's own state is untouched by a set's gradient calls
        m0, v0 = gp._predict(xq, True, True, 0)
        ps.value_and_grad(xq, idx)
        m1, v1 = gp._predict(xq, True, True, 0)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


def test_maximize():
    """value >= start_value for every path, x inside the bounds, value = value_and_grad at (x, s) bit for bit, the same call
    twice gives the same bits; one device call per round.  Measured on an MI355X: 27 rounds, 277 evaluations for the 20
    runs; the five paths gain 0.12 to 1.97 over their best starts."""
    gp, X, ls = _gp(60, 3, "matern", seed=3)
    s, r = 5, 4
    starts = np.random.default_rng(1).uniform(size=(s, r, 3))
    with gp.sample_paths(s, 256, seed=8) as ps:
        calls = []
        orig = ps._grad_std
        ps._grad_std = lambda x, i, centered=False: (calls.append(len(i)), orig(x, i, centered))[1]
        a = ps.maximize(starts, maxiter=60)
        assert calls[0] == s * r and a["n_rounds"] == len(calls) and a["n_evaluations"] == sum(calls)
        b = ps.maximize(starts, maxiter=60)
        for k in ("x", "value", "start_value", "restart", "restart_x", "restart_value"):
            assert np.array_equal(a[k], b[k]), k
        assert a["x"].shape == (s, 3) and np.all((a["x"] >= 0.0) & (a["x"] <= 1.0))
        assert np.all(a["value"] >= a["start_value"])
        sv, _ = ps.value_and_grad(starts.reshape(-1, 3), np.repeat(np.arange(s), r))
        assert np.array_equal(a["start_value"], sv.reshape(s, r).max(axis=1))
        v, g = ps.value_and_grad(a["x"], np.arange(s))
        assert np.array_equal(v, a["value"])
        print(f"rounds {a['n_rounds']} evaluations {a['n_evaluations']} gain {np.round(a['value'] - a['start_value'], 4)}")
        assert np.all(a["value"] > a["start_value"])                       # (random starts: every path gains)
        lo = ps.maximize(starts, bounds=(0.2, 0.6), maxiter=20)
        assert np.all((lo["x"] >= 0.2) & (lo["x"] <= 0.6))
        with pytest.raises(ValueError):
            ps.maximize(starts[:2])


def _rng_state(rng):
    return rng.bit_generator.state["state"]


def test_thompson_batches_with_polish():
    from bobe_amd.acquisition import PathwiseTS, _TS_DUPLICATE_TOL
    gp, X, ls = _gp(60, 2, seed=3)
    pool = np.random.default_rng(1).uniform(size=(700, 2))
    kw = {"candidates": pool, "ts_features": 512}
    acq = PathwiseTS()
    r0, r1, r2 = (np.random.default_rng(42) for _ in range(3))
    pts, vals = acq.get_next_batch(gp, n_batch=6, acq_kwargs=kw, rng=r0)
    pts0, vals0 = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_polish=0), rng=r1)
    assert np.array_equal(pts, pts0) and np.array_equal(vals, vals0)        # the default, bit for bit
    ptsp, valsp = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_polish=4), rng=r2)
    assert _rng_state(r0) == _rng_state(r1) == _rng_state(r2)                 # the same amount drawn
    assert ptsp.shape == (6, 2) and np.all((ptsp >= 0.0) & (ptsp <= 1.0)) and np.all(np.isfinite(valsp))
    dist = np.max(np.abs(ptsp[:, None, :] - ptsp[None, :, :]), axis=2) + np.eye(6)
    assert np.all(dist > _TS_DUPLICATE_TOL)                                  # distinct: no replacement took place
    print(f"polish gain per member: {np.round(valsp - vals, 4)}")
    assert np.all(valsp >= vals)
    again, vagain = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_polish=4), rng=np.random.default_rng(42))
    assert np.array_equal(again, ptsp) and np.array_equal(vagain, valsp)
    with pytest.raises(ValueError):
        acq.get_next_batch(gp, n_batch=2, acq_kwargs=dict(kw, ts_polish=4, ts_mode="posterior"), rng=np.random.default_rng(0))
    x1, v1 = acq.get_next_point(gp, acq_kwargs=dict(kw, ts_polish=2), rng=np.random.default_rng(5))
    assert x1.shape == (2,) and np.isfinite(v1)


def test_polished_thompson_picks_are_feasible_under_the_gate():
    """the deep well of tests/test_gpu_clf_gp.py: the gate admits a disc around the centre, the paths' maxima may lie outside"""
    from bobe_amd.acquisition import PathwiseTS
    from bobe_amd.clf import gate_eval
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, size=(120, 2))
    y = -2000.0 * np.sum((X - 0.5) ** 2, axis=1, keepdims=True)
    g = GPwithClassifier(X, y, clf_threshold=150.0, gp_threshold=400.0, noise=1e-6, lengthscales=[0.3, 0.3])
    assert g.use_clf and g._gated()
    pool = np.random.default_rng(2).uniform(size=(400, 2))
    assert 0 < int(np.sum(gate_eval(g._lib, g._h, pool, 2)[1] > 0)) < 400
    for seed in (0, 1, 2):
        pts, vals = PathwiseTS().get_next_batch(g, n_batch=5, acq_kwargs={"candidates": pool, "ts_features": 256, "ts_polish": 3},
                                                rng=np.random.default_rng(seed))
        assert pts.shape == (5, 2) and np.all((pts >= 0.0) & (pts <= 1.0)) and np.all(np.isfinite(vals))
        assert np.all(gate_eval(g._lib, g._h, pts, 2)[1] > 0), pts
        dist = np.max(np.abs(pts[:, None, :] - pts[None, :, :]), axis=2) + np.eye(5)
        assert np.all(dist > 1e-12)


def test_bo_run_with_polished_thompson_batches():
    """the small problem of tests/test_gpu_paths.py::test_bo_run_with_thompson_batches with ts_polish=4"""
    from bobe_amd.bo import BOBE

    def gaussian(x):
        return float(-0.5 * np.sum(((np.asarray(x) - 0.3) / 0.4) ** 2))
    bounds = np.array([[-2.0, 2.0], [-2.0, 2.0]]).T
    bobe = BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False)
    res = bobe.run(acq="ts", max_evals=32, fit_n_points=4, batch_size=2, mc_points_size=64, num_mc_samples=256,
                   mc_points_method="uniform", ts_polish=4)
    assert bobe.ts_polish == 4
    assert bobe.current_iteration == 12 and len(res["acq_history"]) == 12 and all(np.isfinite(res["acq_history"]))
    tx = np.asarray(res["gp"].train_x)
    assert 8 < len(tx) <= 32 and np.all((tx >= 0.0) & (tx <= 1.0))
    assert res["best_val"] > -2.0
    with pytest.raises(ValueError):
        BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False).run(acq="ts", max_evals=12, ts_polish=-1)
