"""CPU checks of the path gradients and the per-path maximiser: the long-double gradient of tests/paths_grad_restatement.py
against central differences of the long-double value, the maximise driver (bobe_amd.paths.maximize_paths) against
``scipy.optimize.minimize`` restart for restart, its selection rule, and the ``ts_polish`` / ``ts_mode`` argument errors."""
import inspect
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from paths_grad_restatement import value_and_grad_fp64, value_and_grad_ld, weights_ld  # noqa: E402
from paths_restatement import TruthLD, spectral_frequencies  # noqa: E402


def _problem(n, f, s, t, kind, d, seed=0, noise=1e-4, kvar=1.3):
    """the data and hyper-parameters of tests/test_gpu_paths.py::_gp, the caller's arrays of its _caller_arrays"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, -1]) + 0.1 * rng.standard_normal(n)
    y = (y - y.mean()) / (y.std() if n > 1 else 1.0)
    ls = np.full(d, 0.3 * math.sqrt(d))
    r2 = np.random.default_rng(seed + 1)
    u, phase = spectral_frequencies(kind, f, d, r2)
    arr = {"u": u, "phase": phase, "w": r2.standard_normal((s, f)), "eps": math.sqrt(noise) * r2.standard_normal((s, n))}
    Q = r2.uniform(size=(t, d))
    idx = r2.integers(0, s, size=t)
    return X, y, ls, kvar, noise, arr, Q, idx


FD_CASES = [(n, f, s, t, k, d) for (n, f, s, t) in ((1, 10, 1, 1), (50, 200, 5, 7), (130, 300, 3, 5))
            for k in ("rbf", "matern") for d in (2, 9)]


@pytest.mark.parametrize("n,f,s,t,kind,d", FD_CASES, ids=[f"N{n}_F{f}_S{s}_T{t}_{k}_d{d}" for n, f, s, t, k, d in FD_CASES])
def test_long_double_gradient_is_the_derivative_of_the_long_double_value(n, f, s, t, kind, d):
    """Central differences of the long-double value, h = 1e-6, agree with the long-double gradient to 1e-8 (1 + max |grad|),
    centred and uncentred (the truncation error h^2 f''' / 6 and the rounding 2^-64 f / h are both far below that).
    Observed over these cases: at most 2.1e-10 (1 + max |grad|); 6.3e-10 with the larger shapes of the GPU test included."""
    X, y, ls, kvar, noise, arr, Q, idx = _problem(n, f, s, t, kind, d, seed=n + d)
    truth = TruthLD(kind, X, y, ls, kvar, noise)
    LD = np.longdouble
    h = LD(1e-6)
    for cen in (False, True):
        V = weights_ld(truth, centered=cen, **arr)
        _, g = value_and_grad_ld(truth, Q, idx, centered=cen, V=V, **arr)
        fd = np.zeros_like(g)
        for k in range(d):
            e = np.zeros(d, dtype=LD)
            e[k] = h
            fp, _ = value_and_grad_ld(truth, np.asarray(Q, dtype=LD) + e, idx, centered=cen, V=V, **arr)
            fm, _ = value_and_grad_ld(truth, np.asarray(Q, dtype=LD) - e, idx, centered=cen, V=V, **arr)
            fd[:, k] = (fp - fm) / (LD(2.0) * h)
        err = float(np.max(np.abs(fd - g))) / (1.0 + float(np.max(np.abs(g))))
        print(f"centered={cen}: |fd - grad| = {err:.3g} (1 + max |grad|)")
        assert err <= 1e-8
        # and the fp64 restatement is the same function
        f64, g64 = value_and_grad_fp64(kind, X, y, Q, idx, ls, kvar, noise, centered=cen, **arr)
        assert float(np.max(np.abs(g64 - g))) <= 1e-6 * (1.0 + float(np.max(np.abs(g))))


def _small_paths(kind="rbf", d=3, s=3):
    """a (point, path) -> (f, df) function of the fp64 restatement, evaluated point by point (the same bits alone or in a batch)"""
    X, y, ls, kvar, noise, arr, _, _ = _problem(30, 64, s, 1, kind, d, seed=5)

    def one(x, p):
        f, g = value_and_grad_fp64(kind, X, y, np.asarray(x, dtype=np.float64)[None, :], [int(p)], ls, kvar, noise, **arr)
        return float(f[0]), g[0]

    def batch(xs, idx):
        vals = [one(x, p) for x, p in zip(xs, idx)]
        return np.array([v[0] for v in vals]), np.array([v[1] for v in vals])
    return one, batch


@pytest.mark.parametrize("driver", ["stepped", "threads"])
def test_maximize_driver_is_scipy_minimize_restart_for_restart(driver):
    """Every restart of ``maximize_paths`` is ``scipy.optimize.minimize(method='L-BFGS-B', jac=True)`` on -f_s from the same
    start, bit for bit (iterate and value), with the stepped driver and with the thread driver; every round is one batch call,
    the first one on all S * R runs; the result is never below the best start."""
    from scipy.optimize import minimize
    from bobe_amd import optim
    from bobe_amd.paths import maximize_paths
    S, R, d = 3, 4, 3
    one, batch = _small_paths(d=d, s=S)
    starts = np.random.default_rng(2).uniform(size=(S, R, d))
    starts[1, 2] = [0.0, 1.0, 0.5]                                        # a start on the boundary
    sizes = []

    def counted(xs, idx):
        sizes.append(len(idx))
        return batch(xs, idx)
    assert optim._rc_available()
    saved = optim._RC_STATE["ok"]
    optim._RC_STATE["ok"] = driver == "stepped"
    try:
        for maxiter, opts in ((100, None), (3, {"ftol": 1e-12, "gtol": 1e-9})):
            del sizes[:]
            out = maximize_paths(counted, starts, bounds=(0.0, 1.0), maxiter=maxiter, options=opts)
            assert sizes[0] == S * R and out["n_rounds"] == len(sizes) and out["n_evaluations"] == sum(sizes)
            for s in range(S):
                for r in range(R):
                    ref = minimize(lambda x: tuple(-v for v in one(x, s)), starts[s, r], jac=True, method="L-BFGS-B",
                                   bounds=[(0.0, 1.0)] * d, options=dict(opts or {}, maxiter=maxiter))
                    assert np.array_equal(out["restart_x"][s, r], ref.x), (s, r)
                    assert out["restart_value"][s, r] == -ref.fun, (s, r)
                    assert out["start_values"][s, r] == one(starts[s, r], s)[0]
                k = int(np.argmax(out["restart_value"][s]))
                assert out["restart"][s] == k and np.array_equal(out["x"][s], out["restart_x"][s, k])
                assert out["value"][s] == out["restart_value"][s, k] == one(out["x"][s], s)[0]
                assert out["start_value"][s] == out["start_values"][s].max() and out["value"][s] >= out["start_value"][s]
            assert np.all((out["x"] >= 0.0) & (out["x"] <= 1.0))
    finally:
        optim._RC_STATE["ok"] = saved


def test_maximize_selection_rule():
    """Ties go to the lower restart, then to the start; a restart that raises or ends on a non-finite value is skipped; a
    start wins where no restart of its path finished."""
    from bobe_amd.paths import maximize_paths
    centre = np.array([0.25, 0.75])
    S, R, d = 4, 3, 2
    starts = np.random.default_rng(0).uniform(0.1, 0.9, size=(S, R, d))
    starts[0, 1] = starts[0, 0]                     # path 0: restarts 0 and 1 are the same run, restart 2 starts at the maximum
    starts[0, 2] = centre
    # path 2 depends on x_0 alone, so x_1 never moves and tags the restart: 0.1 marks restart 1, the one with the best start
    starts[2, 0], starts[2, 1], starts[2, 2] = [0.8, 0.3], [0.3, 0.1], [0.9, 0.6]

    def batch(xs, idx):
        f, g = [], []
        for x, p in zip(np.asarray(xs), idx):
            if p == 1 and not np.any(np.all(x == starts[1], axis=1)):
                raise RuntimeError("path 1 can be evaluated at its starts only")
            if p == 2 and x[1] == 0.1 and not np.array_equal(x, starts[2, 1]):
                raise RuntimeError("restart 1 of path 2 fails after its first evaluation")
            if p == 3 and not np.any(np.all(x == starts[3], axis=1)):
                f.append(float("nan"))
                g.append(np.full(d, np.nan))
                continue
            if p == 2:
                f.append(-float((x[0] - centre[0]) ** 2))
                g.append(np.array([-2.0 * (x[0] - centre[0]), 0.0]))
            else:
                f.append(-float(np.sum((x - centre) ** 2)))
                g.append(-2.0 * (x - centre))
        return np.array(f), np.array(g)

    out = maximize_paths(batch, starts, bounds=(0.0, 1.0), maxiter=50)
    # path 0: restart 2 sits on the maximum (value 0) and is met by the others to rounding at best - it ties only with itself;
    # restarts 0 and 1 tie with each other bit for bit
    assert np.array_equal(out["restart_x"][0, 0], out["restart_x"][0, 1])
    assert out["restart_value"][0, 0] == out["restart_value"][0, 1]
    assert out["restart_value"][0, 2] == 0.0 and out["start_values"][0, 2] == 0.0
    if out["restart_value"][0, 0] == 0.0:
        assert out["restart"][0] == 0                # the lower restart
    else:
        assert out["restart"][0] == 2                # the restart, not the start of the same value
    assert out["value"][0] == 0.0
    two = maximize_paths(batch, starts[:1, :2], bounds=(0.0, 1.0), maxiter=50)
    assert two["restart"][0] == 0 and np.array_equal(two["x"][0], two["restart_x"][0, 0])   # equal results: the lower restart
    # path 1: no restart finished - the best start wins
    assert np.all(np.isneginf(out["restart_value"][1])) and out["restart"][1] == -1
    k = int(np.argmax(out["start_values"][1]))
    assert np.array_equal(out["x"][1], starts[1, k]) and out["value"][1] == out["start_values"][1, k] == out["start_value"][1]
    # path 2: restart 1 raised and is skipped although its start is the best one; the others go on and reach the maximum
    assert np.isneginf(out["restart_value"][2, 1]) and np.all(np.isfinite(out["restart_value"][2, [0, 2]]))
    assert out["start_value"][2] == out["start_values"][2, 1] == -(0.3 - 0.25) ** 2
    assert out["restart"][2] == int(np.argmax(out["restart_value"][2])) and out["restart"][2] in (0, 2)
    assert out["value"][2] > out["start_value"][2] and out["x"][2][1] in (0.3, 0.6) and abs(out["x"][2][0] - 0.25) < 1e-6
    # path 3: every restart ended on NaN - skipped, a start wins
    assert np.all(np.isneginf(out["restart_value"][3])) and out["restart"][3] == -1
    assert out["value"][3] == out["start_value"][3] == out["start_values"][3].max()
    with pytest.raises(ValueError):
        maximize_paths(batch, starts[0], bounds=(0.0, 1.0))


def test_ts_polish_arguments():
    from bobe_amd.acquisition import PathwiseTS
    from bobe_amd.bo import BOBE
    pool = np.random.default_rng(0).uniform(size=(20, 2))
    acq = PathwiseTS()
    for kw in ({"ts_polish": 4, "ts_mode": "posterior"}, {"ts_polish": -1}, {"ts_polish": 1.5}, {"ts_polish": True},
               {"ts_polish": 2, "ts_mode": "nope"}):
        with pytest.raises(ValueError):
            acq.get_next_batch(None, n_batch=2, acq_kwargs=dict(kw, candidates=pool), rng=np.random.default_rng(0))
    p = inspect.signature(BOBE.run).parameters
    assert p["ts_polish"].kind is inspect.Parameter.KEYWORD_ONLY and p["ts_polish"].default == 0
