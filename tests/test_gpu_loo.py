"""Leave-one-out cross-validation on the device (bobe_gp_loo, bobe_gp_loo_objective, GP.loo / loo_data /
neg_loo_value_and_grad, fit_objective='loo', BOBE.run(loo_diagnostics=True)) against tests/loo_restatement.py.

The comparison rule is the conditioning ladder's (tests/conditioning_common.py, tests/test_gpu_conditioning.py):

    err(device vs truth) <= 4 x err(fp64 SciPy / torch restatement vs truth) + TOL,

both errors measured with ``_err`` against the np.longdouble closed form (hand-written Cholesky and triangular inverse; the
gradient's truth is the hand formula in longdouble, its fp64 side torch autograd).  TOL: value 1e-10, gradient 1e-8, mean 1e-8,
variance 1e-9.  Cases: the three golden shapes (also against N literal refits), ladder rungs 0 and 6 (N = 600, noise 1e-8),
and the hyper-parameters of rungs 2 and 3 on the first 600 points of their design (cond K ~ 2e14 and 1.6e15, where SciPy's own
error is 9e-5 and 1.2e-3).  At N = 1024 / 4096 (the benchmark's synthetic data) there is no longdouble truth: the device is
held to 4 x |loo_closed - loo_closed_inv| + TOL around loo_closed, the disagreement of two fp64 routes standing for their
error.  Every measured figure is printed before it is asserted; with BOBE_LOO_PARITY_OUT=<file> the table is written there
(committed as profiles/loo_parity.txt).
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import loo_restatement as R
from conditioning_common import LADDER, NOISE, _bo_like_design, _err

pytestmark = pytest.mark.gpu

TOL = {"value": 1e-10, "grad": 1e-8, "mean": 1e-8, "var": 1e-9}
GOLDEN = ["rbf_n50_d2", "matern_n130_d3", "rbf_n257_d5_saas"]
CASES = GOLDEN + ["rung0", "rung6", "rung2_first600", "rung3_first600"]
_ROWS = {}
_HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(kernel, X, y physical, ls, kvar, noise) of a named case."""
    if name in GOLDEN:
        z = np.load(os.path.join(_HERE, "golden", name + ".npz"), allow_pickle=True)
        return (str(z["kernel"]), z["X"], z["y"].reshape(-1), np.array(z["lengthscales"], dtype=float),
                float(z["kernel_variance"]), float(z["noise"]))
    rung = int(name[4])
    n, kernel, ls, kvar = LADDER[rung]
    X, y, _ = _bo_like_design(n)
    return kernel, X[:600], y[:600], np.array(ls), kvar, NOISE


def _gp(name, **kw):
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case(name)
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0, **kw)


@functools.lru_cache(maxsize=None)
def _truth(name):
    """The longdouble truth (gradient included) and the fp64 restatements, in the standardised units of the GP's own y."""
    kernel, X, y, ls, kvar, noise = _case(name)
    ys = (y - float(np.mean(y))) / float(np.std(y))              # GP._setup_training_data
    t = R.loo_closed_xp(kernel, X, ys, ls, kvar, noise, want_grad=True)
    m, v, l, s = R.loo_closed(kernel, X, ys, ls, kvar, noise)
    tv, tg = R.loo_objective_torch(kernel, X, ys, np.log(np.append(ls, kvar)), noise)
    return {"t": t, "sci": {"mean": m, "var": v, "lpd": l, "loo": s}, "torch": (tv, tg), "ys": ys}


def _phys(gp, mean, var, loo):
    """standardised (mean, var, L_LOO) -> the physical units GP.loo() reports (in the arrays' own precision)"""
    n = gp.npoints
    return mean * gp.y_std + gp.y_mean, var * gp.y_std ** 2, loo - n * math.log(gp.y_std)


def _record(name, **figs):
    _ROWS.setdefault(name, {}).update(figs)
    out = os.environ.get("BOBE_LOO_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        keys = ["mean", "var", "elpd", "value", "grad"]
        lines = ["# leave-one-out parity (tests/test_gpu_loo.py): errors against the np.longdouble truth, max |delta| / max |truth|",
                 "# dev = the device (GP.loo: mean / var / elpd; bobe_gp_loo_objective: value / grad), ref = the fp64 restatement "
                 "(SciPy cho_solve closed form; torch autograd for value / grad)",
                 "# N = 1024 / 4096 rows: dev = |device - loo_closed|, ref = |loo_closed_inv - loo_closed| (no truth at that size)",
                 "# rule: dev <= 4 x ref + TOL (value 1e-10, grad 1e-8, mean 1e-8, var 1e-9)", "",
                 f"{'case':<26}{'refining':>9} " + " ".join(f"{'dev_' + k:>11}{'ref_' + k:>11}" for k in keys)]
        for nm, r in _ROWS.items():
            cells = [f"{r[q]:>11.2e}" if q in r else f"{'-':>11}" for k in keys for q in ("dev_" + k, "ref_" + k)]   # '-': not measured
            lines.append(f"{nm:<26}{str(r.get('refining', '-')):>9} " + " ".join(a + b for a, b in zip(cells[::2], cells[1::2])))
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    except OSError:
        pass


def _check(name, figs, keys, tol_of):
    for k in keys:
        dev, ref = figs["dev_" + k], figs["ref_" + k]
        print(f"[loo parity] {name:<20} {k:<6} err(device) = {dev:.3e}   err(fp64 restatement) = {ref:.3e}   "
              f"ratio = {dev / ref if ref > 0 else float('inf'):.2f}")
    for k in keys:
        assert figs["dev_" + k] <= 4.0 * figs["ref_" + k] + TOL[tol_of[k]], (name, k, figs["dev_" + k], figs["ref_" + k])


# ---- 1. GP.loo() against the truth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_loo_against_the_extended_precision_truth(name):
    gp = _gp(name)
    assert not gp.not_pd
    r = gp.loo()
    T = _truth(name)
    assert np.array_equal(T["ys"], np.asarray(gp.train_y).reshape(-1))       # the same standardised targets
    tm, tv, te = _phys(gp, T["t"]["mean"], T["t"]["var"], T["t"]["loo"])
    sm, sv, se = _phys(gp, T["sci"]["mean"], T["sci"]["var"], T["sci"]["loo"])
    figs = {"refining": gp.refining,
            "dev_mean": _err(r["mean"], tm), "ref_mean": _err(sm, tm), "dev_var": _err(r["var"], tv), "ref_var": _err(sv, tv),
            "dev_elpd": _err(r["elpd"], te), "ref_elpd": _err(se, te)}
    _record(name, **figs)
    _check(name, figs, ["mean", "var", "elpd"], {"mean": "mean", "var": "var", "elpd": "value"})
    # the derived entries are what they are documented to be
    n = gp.npoints
    y = np.asarray(gp.train_y).reshape(-1) * gp.y_std + gp.y_mean
    assert r["mean"].shape == r["var"].shape == r["z"].shape == r["lpd"].shape == (n,)
    assert np.allclose(r["z"], (y - r["mean"]) / np.sqrt(r["var"]), rtol=1e-9, atol=1e-9)
    assert abs(r["elpd"] - np.sum(r["lpd"])) <= 1e-9 * abs(r["elpd"])
    assert abs(r["rmse"] - math.sqrt(np.mean((y - r["mean"]) ** 2))) <= 1e-9 * r["rmse"] + 1e-300
    assert r["max_abs_z"] == np.max(np.abs(r["z"]))
    assert 0.0 <= r["frac_within_1sigma"] <= r["frac_within_2sigma"] <= 1.0
    assert r["frac_within_2sigma"] == np.mean(np.abs(r["z"]) <= 2.0)
    if name in GOLDEN:
        # N literal refits, fp64 solves of (N-1) x (N-1) systems: their relative error is eps x cond(K) at best, and
        # cond(K) <= N kvar / noise; ten times that bounds the disagreement (written down before any run)
        kernel, X, _, ls, kvar, noise = _case(name)
        bm, bv, bl = R.loo_brute(kernel, X, T["ys"], ls, kvar, noise)
        pm, pv, pe = _phys(gp, bm, bv, float(np.sum(bl)))
        bound = 10.0 * 2.220446049250313e-16 * n * kvar / noise
        eb = (_err(r["mean"], pm), _err(r["var"], pv), _err(r["elpd"], pe))
        print(f"[loo parity] {name:<20} against {n} literal refits: mean {eb[0]:.3e} var {eb[1]:.3e} elpd {eb[2]:.3e} "
              f"(bound {bound:.1e})")
        assert max(eb) <= bound, (eb, bound)


# ---- 2. bobe_gp_loo_objective: value and gradient ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_loo_objective_value_and_gradient(name):
    gp = _gp(name)
    kernel, X, y, ls, kvar, noise = _case(name)
    T = _truth(name)
    val, grad = gp.loo_data(ls, kvar)
    val0, none = gp.loo_data(ls, kvar, want_grad=False)
    assert none is None and np.float64(val0).tobytes() == np.float64(val).tobytes()      # grad == NULL: the same value bits
    tv, tg = T["torch"]
    tt, gt = T["t"]["loo"], T["t"]["grad"]
    figs = {"dev_value": _err(val, tt), "ref_value": _err(tv, tt), "dev_grad": _err(grad, gt), "ref_grad": _err(tg, gt)}
    _record(name, **figs)
    _check(name, figs, ["value", "grad"], {"value": "value", "grad": "grad"})
    # the state's own LOO is the objective at the state's hyper-parameters (same kernels, same order: same bits)
    s = C.c_double(0.0)
    assert gp._lib.bobe_gp_loo(gp._h, None, None, None, C.byref(s)) == 0
    assert np.float64(s.value).tobytes() == np.float64(val).tobytes()


# ---- 3. the benchmark's sizes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
@pytest.mark.parametrize("n,d", [(1024, 6), (4096, 8)])
def test_loo_at_the_benchmark_sizes(n, d, kernel):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, _, _ = synthetic_problem(n, d, 1, 1)
    ls, kvar, noise = np.full(d, 0.6), 1.0, 1e-6
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0)
    assert not gp.not_pd
    r = gp.loo()
    val, _ = gp.loo_data(ls, kvar, want_grad=False)
    ys = np.asarray(gp.train_y).reshape(-1)
    a = R.loo_closed(kernel, X, ys, ls, kvar, noise)
    b = R.loo_closed_inv(kernel, X, ys, ls, kvar, noise)
    am, av, ae = _phys(gp, a[0], a[1], a[3])
    bm, bv, be = _phys(gp, b[0], b[1], b[3])
    name = f"synthetic_{kernel}_n{n}"
    figs = {"refining": gp.refining,
            "dev_mean": _err(r["mean"], am), "ref_mean": _err(bm, am), "dev_var": _err(r["var"], av), "ref_var": _err(bv, av),
            "dev_elpd": _err(r["elpd"], ae), "ref_elpd": _err(be, ae), "dev_value": _err(val, a[3]), "ref_value": _err(b[3], a[3])}
    _record(name, **figs)
    _check(name, figs, ["mean", "var", "elpd", "value"], {"mean": "mean", "var": "var", "elpd": "value", "value": "value"})


def test_gradient_on_128_tiles_follows_the_device_value():
    """From 49 block columns up (N > 6144) K^-1 and B^T B run on 128 x 128 tiles instead of 64 x 64 (lauum's rule: the order of
    the partial sums depends on N only).  No CPU reference at that size: the gradient is held to central differences of the
    device's own value, which does not pass through the tile product.  noise 1e-2 keeps cond(K) near 1e6, so the value carries
    ~1e-10 relative; with a step of 1e-4 in log theta the differences resolve the gradient to ~1e-6 of its largest component
    (truncation h^2 ~ 1e-8, rounding 1e-10 |L| / h); the bound is 1e-5."""
    from bobe_amd import GP
    n, d = 6272, 2
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(n, d))
    y = np.sin(5.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    ls, kvar = np.array([0.25, 0.4]), 1.2
    gp = GP(X, y, noise=1e-2, kernel="matern", lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0)
    th = np.log(np.append(ls, kvar))
    val, grad = gp.loo_data(ls, kvar)
    assert np.isfinite(val) and np.all(np.isfinite(grad))
    h = 1e-4
    fd = np.empty(3)
    for j in range(3):
        e = np.zeros(3)
        e[j] = h
        p, m = np.exp(th + e), np.exp(th - e)
        fd[j] = (gp.loo_data(p[:2], p[2], want_grad=False)[0] - gp.loo_data(m[:2], m[2], want_grad=False)[0]) / (2 * h)
    print(f"[loo parity] 128-tile gradient {grad} central differences {fd}")
    assert np.max(np.abs(grad - fd)) <= 1e-5 * np.max(np.abs(fd)), (grad, fd)


# ---- 4. state paths ---------------------------------------------------------------------------------------------------------
def _state_data(n=300, d=3, seed=8):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = 3.0 + 2.0 * (np.sin(4.0 * X[:, 0]) + X[:, 1] * X[:, 2]) + 0.01 * rng.standard_normal(n)
    return X, y, np.array([0.35, 0.5, 0.6]), 1.3, 1e-6


def _rule_against_fresh(label, gp, kernel, ls, kvar, noise):
    """loo() of ``gp`` (however its state was installed) under the rule, on the data it holds."""
    X = np.asarray(gp.train_x)
    ys = np.asarray(gp.train_y).reshape(-1)
    t = R.loo_closed_xp(kernel, X, ys, ls, kvar, noise)
    m, v, _, s = R.loo_closed(kernel, X, ys, ls, kvar, noise)
    r = gp.loo()
    tm, tv, te = _phys(gp, t["mean"], t["var"], t["loo"])
    sm, sv, se = _phys(gp, m, v, s)
    figs = {"refining": gp.refining,
            "dev_mean": _err(r["mean"], tm), "ref_mean": _err(sm, tm), "dev_var": _err(r["var"], tv), "ref_var": _err(sv, tv),
            "dev_elpd": _err(r["elpd"], te), "ref_elpd": _err(se, te)}
    _record("state_" + label, **figs)
    _check("state_" + label, figs, ["mean", "var", "elpd"], {"mean": "mean", "var": "var", "elpd": "value"})
    return r


def test_state_paths_agree_with_a_fresh_factorisation():
    from bobe_amd import GP
    X, y, ls, kvar, noise = _state_data()
    kw = dict(noise=noise, kernel="rbf", lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0)
    fresh = GP(X, y, **kw)
    rf = _rule_against_fresh("fresh", fresh, "rbf", ls, kvar, noise)
    # repeated calls: identical bits
    again = fresh.loo()
    for k in ("mean", "var", "lpd", "z"):
        assert np.array_equal(rf[k], again[k]), k
    assert rf["elpd"] == again["elpd"]
    # rank-b append
    grown = GP(X[:280], y[:280], **kw)
    grown.update(X[280:], y[280:].reshape(-1, 1))
    assert grown.npoints == 300 and not grown.not_pd
    ra = _rule_against_fresh("append", grown, "rbf", ls, kvar, noise)
    # (two fp64 routes to the same state: ten times eps x cond(K), cond(K) <= N kvar / noise)
    two_routes = 10.0 * 2.220446049250313e-16 * 300 * kvar / noise
    assert _err(ra["mean"], rf["mean"]) <= two_routes and _err(ra["elpd"], rf["elpd"]) <= two_routes
    # device clone: the same state, the same bits; then the kriging believer's step on it
    clone = fresh.copy()
    rc = clone.loo()
    assert np.array_equal(rc["mean"], rf["mean"]) and np.array_equal(rc["var"], rf["var"]) and rc["elpd"] == rf["elpd"]
    xb = np.random.default_rng(9).uniform(size=(2, 3))
    clone.update(xb, clone.predict_mean_batched(xb).reshape(-1, 1))
    assert clone.npoints == 302
    _rule_against_fresh("believer", clone, "rbf", ls, kvar, noise)
    assert fresh.npoints == 300 and np.array_equal(fresh.loo()["mean"], rf["mean"])      # the source is untouched
    # restored from a state dictionary (bobe_gp_set_chol: no refactorisation)
    restored = GP.from_state_dict(fresh.state_dict())
    restored.pivot_floor_ulp = 0.0
    rr = _rule_against_fresh("from_state_dict", restored, "rbf", ls, kvar, noise)
    assert _err(rr["mean"], rf["mean"]) <= two_routes


def test_loo_of_a_gp_with_classifier_is_its_gp_subset():
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(160, 2))
    y = -60.0 * ((X[:, 0] - 0.5) ** 2 + (X[:, 1] - 0.4) ** 2) * 20.0           # spans well beyond gp_threshold
    ls, kvar, noise = np.array([0.3, 0.3]), 1.0, 1e-6
    g = GPwithClassifier(X, y, clf_type="svm", clf_threshold=100.0, gp_threshold=200.0, noise=noise, kernel="matern",
                         lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0)
    assert g.npoints < g.clf_data_size and g._gated()
    r = _rule_against_fresh("gp_with_classifier", g, "matern", ls, kvar, noise)
    assert r["mean"].shape == (g.npoints,) and np.all(np.isfinite(r["mean"])) and np.all(r["var"] > 0)


def test_objective_leaves_the_factorised_state_alone():
    gp = _gp("matern_n130_d3")
    xq = np.random.default_rng(2).uniform(size=(40, 3))
    m0, v0 = gp.predict_batched(xq)
    l0 = gp.loo()
    kernel, X, y, ls, kvar, noise = _case("matern_n130_d3")
    gp.loo_data(ls * 1.3, kvar * 0.7)
    gp.neg_loo_value_and_grad(np.log(np.append(ls * 0.8, kvar * 2.0)))
    m1, v1 = gp.predict_batched(xq)
    l1 = gp.loo()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    assert np.array_equal(l0["mean"], l1["mean"]) and np.array_equal(l0["var"], l1["var"]) and l0["elpd"] == l1["elpd"]
    # and the marginal likelihood after an LOO evaluation keeps its bits
    a = gp.neg_mll_value_and_grad(np.log(np.append(ls, kvar)))
    gp.loo_data(ls * 1.1, kvar)
    b = gp.neg_mll_value_and_grad(np.log(np.append(ls, kvar)))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_neg_loo_assembles_priors_like_the_mll():
    """-(L_LOO + log prior) through the MLL's own ``_assemble_objective``: DSLP prior, a fixed kernel variance."""
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case("matern_n130_d3")
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, lengthscale_prior="DSLP")
    th = np.log(np.append(ls, kvar)) + 0.1
    f, g = gp.neg_loo_value_and_grad(th)
    lsv, kv, tau = gp._parse_hyperparams(th)
    val, gd = gp.loo_data(lsv, kv)
    lp, g_ls, g_kv, _ = gp._prior_and_grad(lsv, kv, tau)
    assert f == -(val + lp) and np.array_equal(g, -np.append(gd[:3] + g_ls * lsv, gd[3] + g_kv * kv))
    assert gp.neg_loo_value_and_grad(th, want_grad=False) == (f, None)
    fixed = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, kernel_variance_prior="fixed")
    f2, g2 = fixed.neg_loo_value_and_grad(np.log(ls))
    assert g2.shape == (3,) and np.isfinite(f2)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------
def test_error_contract():
    from bobe_amd import GP, _lib
    lib = _lib.load()
    X = np.random.default_rng(0).uniform(size=(30, 2))
    y = np.sin(3 * X[:, 0]) + X[:, 1]
    h = C.c_void_p(0)
    assert lib.bobe_gp_create(C.byref(h), 0, 0, 2) == 0
    out = np.empty(30)
    s = C.c_double(0.0)
    assert lib.bobe_gp_loo(h, out.ctypes.data, None, None, C.byref(s)) == -3            # BOBE_ERR_STATE: no data
    assert lib.bobe_gp_loo_objective(h, X[0].ctypes.data, 1.0, C.byref(s), None) == -3
    ys = np.ascontiguousarray((y - y.mean()) / y.std())
    assert lib.bobe_gp_set_data(h, X.ctypes.data, ys.ctypes.data, 30) == 0
    assert lib.bobe_gp_loo(h, out.ctypes.data, None, None, C.byref(s)) == -3            # data, but no factorised state
    assert "bobe_gp_factor" in _lib.last_error()
    assert lib.bobe_gp_loo(None, out.ctypes.data, None, None, None) == -1
    assert lib.bobe_gp_loo_objective(h, None, 1.0, C.byref(s), None) == -1
    assert lib.bobe_gp_loo_objective(h, X[0].ctypes.data, 1.0, None, None) == -1
    lib.bobe_gp_destroy(h)
    gp = GP(X, y, noise=1e-6, lengthscales=[0.4, 0.4], kernel_variance=1.0)
    assert lib.bobe_gp_loo(gp._h, None, None, None, None) == 0                          # all-NULL outputs are accepted
    # a non-PD theta: duplicated points without noise, under the rank test
    Xd = np.vstack([X[:5], X[:5]])
    bad = GP(Xd, np.arange(10.0), noise=0.0, lengthscales=[0.3, 0.3], kernel_variance=1.0, pivot_floor_ulp=64)
    assert bad.not_pd
    g = np.zeros(3)
    ls = np.array([0.3, 0.3])
    assert lib.bobe_gp_loo_objective(bad._h, ls.ctypes.data, 1.0, C.byref(s), g.ctypes.data) == _lib.BOBE_NOT_PD
    assert math.isnan(s.value) and np.all(np.isnan(g))
    v, gr = bad.loo_data(ls, 1.0)
    assert math.isnan(v) and np.all(np.isnan(gr))
    m10, v10, l10 = np.zeros(10), np.zeros(10), np.zeros(10)
    assert lib.bobe_gp_loo(bad._h, m10.ctypes.data, v10.ctypes.data, l10.ctypes.data, C.byref(s)) == _lib.BOBE_NOT_PD
    assert np.all(np.isnan(m10)) and np.all(np.isnan(v10)) and np.all(np.isnan(l10)) and math.isnan(s.value)
    # the handle stays usable
    assert np.isfinite(gp.loo()["elpd"])


def test_loo_outputs_may_live_on_the_device():
    import torch
    gp = _gp("rbf_n50_d2")
    r = gp.loo()
    n = gp.npoints
    m = torch.empty(n, dtype=torch.float64, device="cuda")
    v = torch.empty(n, dtype=torch.float64, device="cuda")
    s = torch.empty(1, dtype=torch.float64, device="cuda")
    assert gp._lib.bobe_gp_loo(gp._h, C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()), None, C.c_void_p(s.data_ptr())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy() * gp.y_std + gp.y_mean, r["mean"])
    assert np.array_equal(v.cpu().numpy() * gp.y_std ** 2, r["var"])
    assert float(s.cpu()[0]) - n * math.log(gp.y_std) == r["elpd"]


# ---- 6. the fit -------------------------------------------------------------------------------------------------------------
def _fit_case(name, prior):
    """fit_objective='loo' from four fixed starts against SciPy's L-BFGS-B (its defaults, the same bounds) driving the torch
    restatement from the same starts; both sides' end points are valued by the restatement."""
    from scipy.optimize import minimize

    from bobe_amd import GP
    from bobe_amd import priors as P
    kernel, X, y, ls, kvar, noise = _case(name)
    d = X.shape[1]
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, lengthscale_prior=prior,
            lengthscale_bounds=[0.05, 2.0], kernel_variance_bounds=[1e-2, 1e2], optimizer_options={"method": "L-BFGS-B"},
            fit_objective="loo")
    ys = np.asarray(gp.train_y).reshape(-1)
    th0 = np.log(np.append(ls, kvar))
    x0 = np.vstack([th0, th0 + np.random.default_rng(21).uniform(-0.6, 0.6, size=(3, d + 1))])
    x0 = np.clip(x0, gp.hyperparam_bounds[0], gp.hyperparam_bounds[1])
    dist = P.dslp(d) if prior == "DSLP" else None

    def restated(th):                                  # -(L_LOO + log prior) and its gradient; uniform priors are constants
        val, g = R.loo_objective_torch(kernel, X, ys, th, noise)
        if dist is not None:
            lsv = np.exp(th[:d])
            val += float(np.sum(dist.log_prob(lsv)))
            g[:d] += np.asarray(dist.dlog_prob(lsv)) * lsv
        return -val, -g

    res = gp.fit(x0=x0, maxiter=500)
    f_dev = restated(np.asarray(res["params"], dtype=float))[0]
    bounds = list(zip(gp.hyperparam_bounds[0], gp.hyperparam_bounds[1]))
    f_sci = min(minimize(restated, x, jac=True, method="L-BFGS-B", bounds=bounds, options={"maxiter": 500}).fun for x in x0)
    print(f"[loo fit] {name} prior={prior}: device theta valued at {f_dev:.10f}, SciPy on the restatement {f_sci:.10f}, "
          f"relative gap {(f_dev - f_sci) / abs(f_sci):.2e}")
    assert f_dev <= f_sci + 1e-6 * abs(f_sci), (f_dev, f_sci)
    # the 'mll' key holds -best_loss of the LOO objective
    assert abs(res["mll"] + gp.neg_loo_value_and_grad(res["params"], want_grad=False)[0]) <= 1e-9 * abs(res["mll"])
    return gp, res


def test_fit_with_the_loo_objective_matern():
    gp, res = _fit_case("matern_n130_d3", None)
    assert gp.fit_objective == "loo"


def test_fit_with_the_loo_objective_rbf_dslp():
    _fit_case("rbf_n257_d5_saas", "DSLP")


def test_fit_objective_is_validated_and_mll_is_the_default():
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case("matern_n130_d3")
    kw = dict(noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar)
    with pytest.raises(ValueError):
        GP(X, y, fit_objective="bogus", **kw)
    gp = GP(X, y, **kw)
    assert gp.fit_objective == "mll"
    with pytest.raises(ValueError):
        gp.fit_objective = "bogus"
    assert gp.fit_objective == "mll"
    explicit = GP(X, y, fit_objective="mll", **kw)
    x0 = np.log(np.append(ls, kvar))[None, :] + np.array([[0.0], [0.2]])
    a, b = gp.fit(x0=x0, maxiter=100), explicit.fit(x0=x0, maxiter=100)
    assert a["mll"] == b["mll"] and np.array_equal(a["params"], b["params"])      # the keyword's default is the attribute's
    gp.fit_objective = "loo"
    c = gp.fit(x0=x0, maxiter=100)
    print(f"[loo fit] mll optimum {a['params']} ({a['mll']:.6f}), loo optimum {c['params']} ({c['mll']:.6f})")
    # 'mll' of the result is -best_loss of the objective that was minimised: L_LOO + log prior here, the MLL's before
    assert abs(c["mll"] + gp.neg_loo_value_and_grad(c["params"], want_grad=False)[0]) <= 1e-9 * abs(c["mll"])
    assert abs(a["mll"] + gp.neg_mll_value_and_grad(a["params"], want_grad=False)[0]) <= 1e-9 * abs(a["mll"])
    # the LOO fit moved, downhill in its own objective, and not to the MLL's optimum
    assert -c["mll"] < min(gp.neg_loo_value_and_grad(x, want_grad=False)[0] for x in x0)
    assert not np.array_equal(c["params"], a["params"])


# ---- 7. the BO loop ---------------------------------------------------------------------------------------------------------
def _himmelblau(x):
    return -((x[0] ** 2 + x[1] - 11) ** 2 + (x[0] + x[1] ** 2 - 7) ** 2) / 10.0


def _run(refits=None, **kw):
    """One short 2-D run; ``refits`` (a list) receives one entry per hyper-parameter refit that ``run`` makes."""
    import bobe_amd.bo as bo
    from bobe_amd.bo import BOBE
    bounds = np.array([[-4.0, 4.0], [-4.0, 4.0]]).T
    gp_kwargs = kw.pop("gp_kwargs", None)
    bobe = BOBE(_himmelblau, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False, gp_kwargs=gp_kwargs)
    if refits is not None:
        orig = bo.gp_fit

        def counted(gp, *a, **k):
            refits.append(gp.npoints)
            return orig(gp, *a, **k)
        bo.gp_fit = counted
        try:
            return bobe, bobe.run(acq="wipstd", max_evals=28, fit_n_points=2, batch_size=2, mc_points_size=64,
                                  num_mc_samples=256, mc_points_method="uniform", **kw)
        finally:
            bo.gp_fit = orig
    res = bobe.run(acq="wipstd", max_evals=28, fit_n_points=2, batch_size=2, mc_points_size=64, num_mc_samples=256,
                   mc_points_method="uniform", **kw)
    return bobe, res


def test_bo_run_records_loo_diagnostics():
    _, plain = _run()
    _, off = _run(loo_diagnostics=False)
    refits = []
    bobe, on = _run(refits=refits, loo_diagnostics=True)
    assert "loo_history" not in plain and "loo_history" not in off
    for a in (off, on):                                 # the flag changes nothing the run computes
        assert np.array_equal(a["gp"].train_x, plain["gp"].train_x) and np.array_equal(a["gp"].train_y, plain["gp"].train_y)
        assert np.array_equal(a["lengthscales"], plain["lengthscales"]) and a["kernel_variance"] == plain["kernel_variance"]
        assert a["acq_history"] == plain["acq_history"]
    hist = on["loo_history"]
    assert len(hist) == len(refits) >= 3 and [e["n"] for e in hist] == refits      # one entry per refit
    assert set(hist[0]) == {"n", "elpd", "rmse", "max_abs_z", "frac_within_1sigma", "frac_within_2sigma"}
    ns = [e["n"] for e in hist]
    assert all(b > a for a, b in zip(ns, ns[1:])) and ns[-1] <= on["gp"].npoints
    assert all(np.isfinite(list(e.values())).all() for e in hist)


def test_bo_run_with_the_loo_fit_objective():
    bobe, res = _run(gp_kwargs={"fit_objective": "loo"}, loo_diagnostics=True)
    assert res["gp"].fit_objective == "loo" and np.isfinite(res["best_val"]) and res["loo_history"]
