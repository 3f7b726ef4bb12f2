"""CPU checks of the weighted score gradients and their polish: the long-double restatement of
tests/weighted_grad_restatement.py against the weighted scores' own restatement and against central differences of its values,
the four rho closed forms against central differences in v+ alone, the ``weighted_polish`` argument rules and the selection
rule of ``WeightedIntegratedPosteriorBase._polished_point`` with stub GPs, and the interface."""
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import weighted_criteria_restatement as W  # noqa: E402
import weighted_grad_restatement as R  # noqa: E402

LD = np.longdouble
KEYS = R.KEYS


def _problem(kind, y_std, weighted, noise=1e-6, n=40, d=3, m=20, c=4, seed=0):
    rng = np.random.default_rng(seed)
    X, Z, cand = rng.uniform(size=(n, d)), rng.uniform(size=(m, d)), rng.uniform(size=(c, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=n)
    ys = (y - y.mean()) / y.std()
    lw = 5.0 * rng.normal(size=m) if weighted else None
    return X, ys, Z, cand, np.full(d, 0.4), 2.0, noise, lw


def _central_differences(st, cand, h):
    cand = np.asarray(cand, dtype=LD)
    fd = {k: np.zeros(cand.shape, dtype=LD) for k in KEYS}
    for j in range(cand.shape[1]):
        e = np.zeros(cand.shape[1], dtype=LD)
        e[j] = h
        p, q = R.value_and_grad(st, cand + e), R.value_and_grad(st, cand - e)
        for k in KEYS:
            fd[k][:, j] = (p[k] - q[k]) / (LD(2.0) * h)
    return fd


GRID = [(k, s, w) for k in ("rbf", "matern") for s in (1.0, 4e3) for w in (False, True)]
GRID_IDS = [f"{k}_ystd{s:g}_{'weights' if w else 'draws'}" for k, s, w in GRID]


@pytest.mark.parametrize("kind,y_std,weighted", GRID, ids=GRID_IDS)
def test_long_double_values_are_the_weighted_scores(kind, y_std, weighted):
    """The values of the gradient restatement (long double) equal ``weighted_criteria_restatement.weighted_scores`` (fp64
    LAPACK) to 1e-12 relative: N = 40 at noise 1e-6 keeps the fp64 side's own error there (observed: at most 1.3e-13)."""
    X, ys, Z, cand, ls, kvar, noise, lw = _problem(kind, y_std, weighted)
    out = R.value_and_grad(R.State(kind, X, ys, Z, ls, kvar, noise, y_std, lw, LD), cand)
    ref = W.weighted_scores(W.dense_state(kind, X, ys, cand, Z, ls, kvar, noise), y_std, lw)
    for k in KEYS:
        err = float(np.max(np.abs(out[k] - ref[k]) / np.abs(ref[k])))
        print(f"{k}: {err:.3g}")
        assert err <= 1e-12, (k, err)


@pytest.mark.parametrize("kind,y_std,weighted", GRID, ids=GRID_IDS)
def test_long_double_gradient_is_the_derivative_of_the_long_double_value(kind, y_std, weighted):
    """Central differences of the long-double value, h = 1e-6, agree with the long-double gradient to 1e-8 (1 + max |grad|),
    the step and bound of tests/test_paths_grad_cpu.py (truncation h^2 f''' / 6 and rounding 2^-64 f / h both far below).
    Observed: at most 7.1e-10 (1 + max |grad|).  The fp64 restatement is the same function."""
    X, ys, Z, cand, ls, kvar, noise, lw = _problem(kind, y_std, weighted)
    st = R.State(kind, X, ys, Z, ls, kvar, noise, y_std, lw, LD)
    out = R.value_and_grad(st, cand)
    assert not out["floored"].any()
    fd = _central_differences(st, cand, LD(1e-6))
    o64 = R.value_and_grad(R.State(kind, X, ys, Z, ls, kvar, noise, y_std, lw, np.float64), cand)
    for k in KEYS:
        g = out["d" + k]
        err = float(np.max(np.abs(fd[k] - g))) / (1.0 + float(np.max(np.abs(g))))
        print(f"{k}: |fd - grad| = {err:.3g} (1 + max |grad|)")
        assert err <= 1e-8, (k, err)
        assert float(np.max(np.abs(o64["d" + k] - g))) <= 1e-6 * (1.0 + float(np.max(np.abs(g)))), k


@pytest.mark.parametrize("kind", ["rbf", "matern"])
@pytest.mark.parametrize("y_std,weighted", [(1.0, False), (4e3, True)], ids=["ystd1_draws", "ystd4000_weights"])
def test_floored_integration_points_are_constants(kind, y_std, weighted):
    """Two integration points are training points.  For such a z, base_z = noise (2 - noise (K^-1)_zz) lies in [noise, 2 noise):
    it floors (< 1e-12) for EVERY candidate once noise < 5e-13, so the test takes noise = 1e-13 (long double only).
    Candidate 0 lies 1e-9 from one of them: its floored count is asserted (> 0, < M), its floored rows of d v+ / dx are exactly
    zero and everything is finite.  Its gradient is NOT compared with differences: there s(x) ~ noise + kvar |x - X_i|^2 /
    ls^2 varies a hundredfold over 1e-6, and the long-double value (condition number 2e13) carries ~5e-12 of rounding, so no
    step resolves the derivative to 1e-8 (h = 1e-10 .. 1e-12 gave 8e-6 .. 1.5e-3).  Candidate 1 is a generic point of the
    same state - the same two z floored, the same branch - and is held to the h = 1e-6 / 1e-8 rule above."""
    rng = np.random.default_rng(1)
    n, d, m = 30, 3, 16
    X, Z = rng.uniform(size=(n, d)), rng.uniform(size=(m, d))
    Z[3], Z[7] = X[5], X[11]
    cand = np.array([X[5] + 1e-9, rng.uniform(size=d)])
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2
    ys = (y - y.mean()) / y.std()
    lw = 5.0 * rng.normal(size=m) if weighted else None
    st = R.State(kind, X, ys, Z, np.full(d, 0.25), 2.0, 1e-13, y_std, lw, LD)
    assert np.all(st.base[[3, 7]] < 1e-12) and np.all(np.delete(st.base, [3, 7]) > 1e-12)
    out = R.value_and_grad(st, cand)
    for c in range(2):
        count = int(out["floored"][c].sum())
        print(f"candidate {c}: {count} of {m} integration points floored")
        assert 0 < count < m
        v, fl, dv = R.fantasy_var_and_grad(st, cand[c])
        assert np.all(dv[fl] == 0) and np.all(v[fl] == LD(1e-12) * LD(y_std) ** 2)
        assert all(np.all(np.isfinite(out[k][c])) and np.all(np.isfinite(out["d" + k][c])) for k in KEYS)
    fd = _central_differences(st, cand[1:2], LD(1e-6))
    for k in KEYS:
        g = out["d" + k][1]
        err = float(np.max(np.abs(fd[k][0] - g))) / (1.0 + float(np.max(np.abs(g))))
        print(f"{k}: |fd - grad| = {err:.3g} (1 + max |grad|)")
        assert err <= 1e-8, (k, err)


@pytest.mark.parametrize("kind,y_std,weighted", GRID, ids=GRID_IDS)
def test_rho_closed_forms_against_differences_in_v_alone(kind, y_std, weighted):
    """d score / d v+_z, one z at a time, by central differences of ``scores_from_v`` with the relative step h = 1e-6 v+_z in
    long double: truncation (h / v)^2 / 8 = 1e-13 of the derivative, rounding 2^-64 |score| / h; bound 1e-8 max_z |rho|."""
    X, ys, Z, cand, ls, kvar, noise, lw = _problem(kind, y_std, weighted)
    st = R.State(kind, X, ys, Z, ls, kvar, noise, y_std, lw, LD)
    v, _, _ = R.fantasy_var_and_grad(st, cand[0])
    rho = R.rho_from_v(v, st.a, st.omega, st.e)
    fd = {k: np.zeros(len(v), dtype=LD) for k in KEYS}
    for z in range(len(v)):
        h = LD(1e-6) * v[z]
        vp, vm = v.copy(), v.copy()
        vp[z] += h
        vm[z] -= h
        p, q = R.scores_from_v(vp, st.a, st.omega, st.e), R.scores_from_v(vm, st.a, st.omega, st.e)
        for k in KEYS:
            fd[k][z] = (p[k] - q[k]) / (LD(2.0) * h)
    for k in KEYS:
        err = float(np.max(np.abs(fd[k] - rho[k])) / np.max(np.abs(rho[k])))
        print(f"{k}: {err:.3g} max |rho|")
        assert err <= 1e-8, (k, err)
    assert abs(float(np.sum(rho["eiv"])) - 1.0) <= 1e-15 * len(v) and np.all(rho["imiqr"] >= 0)


# ---------------------------------------------------------------------------------------------- the polish, with stub GPs
class _QuadraticGP:
    """score(x) = |x - x0|^2 + c0 for every criterion; NaN where x[1] > nan_above"""

    device = 0

    def __init__(self, x0, c0=0.25, n=10, nan_above=np.inf):
        self.x0, self.c0, self.nan_above = np.asarray(x0, dtype=np.float64), c0, nan_above
        self.ndim = len(self.x0)
        self.train_x = np.zeros((n, self.ndim))
        self.grad_calls = []

    def _f(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        f = np.sum((x - self.x0) ** 2, axis=1) + self.c0
        return np.where(x[:, 1] > self.nan_above, np.nan, f), 2.0 * (x - self.x0)

    def wip_sweep(self, candidates, mc_points, want_mean_var=False, *, log_weights=None, criteria=None):
        f, _ = self._f(candidates)
        key = criteria[0]
        return {key: f, "argmin_" + key: int(np.nanargmin(f)), "min_" + key: float(np.nanmin(f))}

    def wip_grad_w(self, candidates, mc_points, *, log_weights=None, criteria=None):
        assert len(criteria) == 1
        self.grad_calls.append(len(np.atleast_2d(candidates)))
        f, g = self._f(candidates)
        return {criteria[0]: f, "d" + criteria[0]: g}


def _pool(seed=4, m=12, d=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 0.9, size=(m, d)), rng.normal(size=m)


@pytest.mark.parametrize("bad", [True, False, -1, 17, 2.5, 2.0, "3", None])
def test_weighted_polish_must_be_an_integer_from_0_to_16(bad):
    from bobe_amd.acquisition import EIV, IMIQR, WIPStd
    pool, lw = _pool()
    for acq in (IMIQR(), EIV(), WIPStd()):
        with pytest.raises(ValueError, match="weighted_polish"):
            acq.get_next_point(_QuadraticGP([0.5, 0.5, 0.5]),
                               acq_kwargs={"mc_points": pool, "mc_log_weights": lw, "weighted_polish": bad})


def test_bobe_run_takes_the_keyword():
    from bobe_amd.bo import BOBE
    p = inspect.signature(BOBE.run).parameters["weighted_polish"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0


def test_no_polish_is_the_pool_pick_and_draws_nothing():
    from bobe_amd.acquisition import IMIQR
    pool, lw = _pool()
    gp = _QuadraticGP([0.5, 0.5, 0.5])
    want = int(np.argmin(gp._f(pool)[0]))
    for kwargs in ({}, {"weighted_polish": 0}, {"weighted_polish": np.int64(0)}):
        rng = np.random.default_rng(3)
        before = rng.bit_generator.state
        x, v = IMIQR().get_next_point(gp, acq_kwargs=dict(mc_points=pool, mc_log_weights=lw, **kwargs), rng=rng)
        assert rng.bit_generator.state == before
        assert np.array_equal(x, pool[want]) and v == gp._f(pool[want])[0][0]
    assert gp.grad_calls == []


def test_polish_reaches_the_minimum_in_lock_step_and_draws_nothing():
    from bobe_amd.acquisition import EIV
    pool, lw = _pool()
    gp = _QuadraticGP([0.31, 0.62, 0.47])
    rng = np.random.default_rng(3)
    before = rng.bit_generator.state
    x, v = EIV().get_next_point(gp, acq_kwargs={"mc_points": pool, "mc_log_weights": lw, "weighted_polish": 4}, rng=rng)
    assert rng.bit_generator.state == before
    assert np.max(np.abs(x - gp.x0)) <= 1e-6 and abs(v - gp.c0) <= 1e-10 and v < np.min(gp._f(pool)[0])
    assert gp.grad_calls[0] == 4 and max(gp.grad_calls) == 4          # one call per round, on the runs still waiting
    assert np.all((x >= 0.0) & (x <= 1.0))
    # R larger than the pool: every row is a start
    gp2 = _QuadraticGP([0.31, 0.62, 0.47])
    EIV().get_next_point(gp2, acq_kwargs={"mc_points": pool[:3], "mc_log_weights": lw[:3], "weighted_polish": 16})
    assert gp2.grad_calls[0] == 3


def test_selection_rule_pool_pick_wins_ties_and_a_non_finite_restart_is_skipped():
    from bobe_amd.acquisition import IMIQR
    pool, lw = _pool()
    # the minimum IS a pool row: no restart can be strictly better, the pool pick itself comes back (its own array values)
    gp = _QuadraticGP(pool[5].copy())
    x, v = IMIQR().get_next_point(gp, acq_kwargs={"mc_points": pool, "mc_log_weights": lw, "weighted_polish": 3})
    assert np.array_equal(x, pool[5]) and v == gp.c0 and len(gp.grad_calls) > 0
    # one start sits where the gradient entry returns NaN (the sweep does not): its restart is skipped, the others finish
    pool2 = pool.copy()
    pool2[2] = [0.3, 0.97, 0.5]

    class _NanInGrad(_QuadraticGP):
        def wip_sweep(self, candidates, mc_points, want_mean_var=False, *, log_weights=None, criteria=None):
            saved, self.nan_above = self.nan_above, np.inf
            try:
                return super().wip_sweep(candidates, mc_points, log_weights=log_weights, criteria=criteria)
            finally:
                self.nan_above = saved

    gp = _NanInGrad([0.3, 0.5, 0.5], nan_above=0.96)
    x, v = IMIQR().get_next_point(gp, acq_kwargs={"mc_points": pool2, "mc_log_weights": lw, "weighted_polish": 12})
    assert gp.grad_calls[0] == 12 and np.max(np.abs(x - gp.x0)) <= 1e-6 and abs(v - gp.c0) <= 1e-10
    # every restart non-finite: the pool pick
    gp = _NanInGrad([0.3, 0.5, 0.5], nan_above=-1.0)
    x, v = IMIQR().get_next_point(gp, acq_kwargs={"mc_points": pool, "mc_log_weights": lw, "weighted_polish": 2})
    want = int(np.argmin(np.sum((pool - gp.x0) ** 2, axis=1)))
    assert np.array_equal(x, pool[want]) and v == np.sum((pool[want] - gp.x0) ** 2) + gp.c0


def test_a_design_above_the_limit_keeps_the_pool_pick():
    from bobe_amd.acquisition import IMIQR, WIP_GRAD_W_MAX_N
    pool, lw = _pool()
    gp = _QuadraticGP([0.31, 0.62, 0.47], n=WIP_GRAD_W_MAX_N + 1)
    x, v = IMIQR().get_next_point(gp, acq_kwargs={"mc_points": pool, "mc_log_weights": lw, "weighted_polish": 4})
    want = int(np.argmin(gp._f(pool)[0]))
    assert np.array_equal(x, pool[want]) and gp.grad_calls == []


# ---------------------------------------------------------------------------------------------------------- the interface
def test_header_binding_and_python_surface():
    from bobe_amd import GP, GPwithClassifier, _lib
    with open(os.path.join(HERE, "..", "include", "bobe_gp.h")) as fh:
        assert "int bobe_gp_wip_grad_w(" in fh.read()
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert len(sig["bobe_gp_wip_grad_w"][1]) == 9
    p = inspect.signature(GP.wip_grad_w).parameters
    assert list(p) == ["self", "candidates", "mc_points", "log_weights", "criteria"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("log_weights", "criteria"))
    assert GPwithClassifier.wip_grad_w is GP.wip_grad_w and GPwithClassifier.wip_grad is GP.wip_grad
