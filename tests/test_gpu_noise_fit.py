"""The noise level as a fitted hyper-parameter on the device: bobe_gp_mll_noise(_batch), bobe_gp_loo_objective_noise(_batch),
GP(fit_noise=True) and BOBE(gp_kwargs={'fit_noise': True}), against tests/noise_restatement.py.

Parity rule (section 1): value |delta| / |value| <= 1e-10 and whole d + 2 gradient |delta|_inf / |grad|_inf <= 1e-8 against the
np.longdouble restatement (DESIGN.md section 2's tolerances), asserted for every case.  Only the cases listed in
FP64_LIMITED - where the NumPy fp64 restatement itself sits at the tolerance (cond K~ ~ N kvar / nu = 6e7: N = 50, d = 2, rbf,
nu = 1e-6: value 0.9e-10 / 1.0e-10 for the MLL / LOO objective, the device 1.9e-10 / 2.6e-10) - take the conditioning
ladder's rule instead: err(device) <= 4 x err(NumPy fp64 restatement) + the tolerance, both against the longdouble truth.
Every figure is printed before it is asserted.  The value and the first d + 1 gradient entries are compared BITWISE with bobe_gp_mll /
bobe_gp_loo_objective at the same noise installed by bobe_gp_set_hyper; batch members bitwise with their single calls.
"""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

import noise_restatement as NR

pytestmark = pytest.mark.gpu

TOL_VALUE, TOL_GRAD = 1e-10, 1e-8
SHAPES = [(2, 2, "rbf"), (50, 2, "rbf"), (128, 3, "matern"), (129, 3, "matern"), (257, 5, "rbf")]
NOISES = [1e-6, 1e-3, 1e-1]
OBJECTIVES = ["mll", "loo"]
# (N, d, kernel, nu, objective) where fp64 itself cannot reach the strict tolerances: the ladder rule applies to these alone
FP64_LIMITED = {(50, 2, "rbf", 1e-6, "mll"), (50, 2, "rbf", 1e-6, "loo")}


def _err(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def _data(n, d, kind):
    X, f, ls, kvar = NR.seeded_case(n, d, kind)
    for a in (X, f, ls):
        a.setflags(write=False)
    return X, f, ls, kvar


@functools.lru_cache(maxsize=None)
def _truth(n, d, kind, nu):
    """The longdouble truth and the NumPy fp64 restatement of both objectives, computed once per case."""
    X, f, ls, kvar = _data(n, d, kind)
    ys = NR.standardise(f)
    return (NR.noise_closed(kind, X, ys, ls, kvar, nu, np.longdouble), NR.noise_closed(kind, X, ys, ls, kvar, nu, np.float64), ys)


def _gp(n, d, kind, nu, **kw):
    from bobe_amd import GP
    X, f, ls, kvar = _data(n, d, kind)
    kw.setdefault("pivot_floor_ulp", 0.0)
    return GP(X, f, noise=nu, kernel=kind, lengthscales=ls, kernel_variance=kvar, **kw)


def _noise_fn(gp, objective, batch=False):
    return getattr(gp, ("mll" if objective == "mll" else "loo") + "_data_noise" + ("_batch" if batch else ""))


def _plain_fn(gp, objective, batch=False):
    return getattr(gp, ("mll" if objective == "mll" else "loo") + "_data" + ("_batch" if batch else ""))


# ---- 1. parity of the gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", NOISES)
@pytest.mark.parametrize("n,d,kind", SHAPES)
def test_parity_with_the_extended_precision_restatement(n, d, kind, nu):
    gp = _gp(n, d, kind, nu)
    assert not gp.not_pd
    t, c, ys = _truth(n, d, kind, nu)
    assert np.array_equal(ys, np.asarray(gp.train_y).reshape(-1))
    _, _, ls, kvar = _data(n, d, kind)
    for obj in OBJECTIVES:
        val, grad = _noise_fn(gp, obj)(ls, kvar, nu)
        assert grad.shape == (d + 2,) and np.isfinite(val) and np.all(np.isfinite(grad))
        dv, dg = _err(val, t[obj]), _err(grad, t[obj + "_grad"])
        rv, rg = _err(c[obj], t[obj]), _err(c[obj + "_grad"], t[obj + "_grad"])
        dn = abs(float(grad[-1] - t[obj + "_grad"][-1])) / float(np.max(np.abs(t[obj + "_grad"])))
        strict = (n, d, kind, nu, obj) not in FP64_LIMITED
        print(f"[noise parity] N={n} d={d} {kind} nu={nu:g} {obj}: value dev {dv:.2e} fp64 {rv:.2e} | grad dev {dg:.2e} "
              f"fp64 {rg:.2e} | d/dlog nu {grad[-1]:.9g} (dev {dn:.2e}) | {'strict' if strict else 'LADDER RULE'}")
        if strict:
            assert dv <= TOL_VALUE, (obj, dv, rv)
            assert dg <= TOL_GRAD, (obj, dg, rg)
        else:
            assert dv <= 4.0 * rv + TOL_VALUE, (obj, dv, rv)
            assert dg <= 4.0 * rg + TOL_GRAD, (obj, dg, rg)
        # the existing launch list, unchanged: the bits of the namesake at the same installed noise
        pv, pg = _plain_fn(gp, obj)(ls, kvar)
        assert val == pv and np.array_equal(grad[:d + 1], pg), (obj, val, pv, grad, pg)
        v0, none = _noise_fn(gp, obj)(ls, kvar, nu, want_grad=False)
        assert none is None and v0 == val


# ---- 2. batch equals single, bit for bit ------------------------------------------------------------------------------------
def _members(n, d, kind, B):
    _, _, ls, kvar = _data(n, d, kind)
    return (np.array([ls * (0.7 + 0.1 * b) for b in range(B)]), np.array([kvar * (0.5 + 0.25 * b) for b in range(B)]),
            np.array([NOISES[b % 3] for b in range(B)]))


def _raw_batch(gp, obj, ls, kv, nz, want_grad=True):
    from bobe_amd import _lib
    B, d = len(kv), gp.ndim
    fn = getattr(gp._lib, "bobe_gp_mll_noise_batch" if obj == "mll" else "bobe_gp_loo_objective_noise_batch")
    val, grad, status = np.zeros(B), np.zeros((B, d + 2)), np.full(B, -7, dtype=np.int32)
    st = fn(gp._h, B, _lib.ptr(np.ascontiguousarray(ls)), _lib.ptr(np.ascontiguousarray(kv)),
            _lib.ptr(np.ascontiguousarray(nz)), _lib.ptr(val), _lib.ptr(grad) if want_grad else None,
            C.c_void_p(status.ctypes.data))
    return st, val, grad, status


@pytest.mark.parametrize("obj", OBJECTIVES)
@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("n,d", [(130, 3), (257, 5)])
def test_batch_members_return_their_single_calls_bits(n, d, B, obj):
    from bobe_amd import _lib
    gp = _gp(n, d, "rbf", 1e-8, pivot_floor_ulp=64.0)
    ls, kv, nz = _members(n, d, "rbf", B)
    singles = [_noise_fn(gp, obj)(ls[b], kv[b], nz[b]) for b in range(B)]
    sv, sg = np.array([s[0] for s in singles]), np.array([s[1] for s in singles])
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(sg)) and len(set(sg[:, -1].tolist())) == B
    val, grad = _noise_fn(gp, obj, batch=True)(ls, kv, nz)
    assert grad.shape == (B, d + 2)
    assert np.array_equal(val, sv) and np.array_equal(grad, sg)
    v0, none = _noise_fn(gp, obj, batch=True)(ls, kv, nz, want_grad=False)
    assert none is None and np.array_equal(v0, sv)
    # one member not positive definite (a long length scale at a noise below the rank test's floor): NaN in its d + 2
    # entries and its own status, the others keep their bits
    bad = 1
    ls2, nz2 = ls.copy(), nz.copy()
    ls2[bad], nz2[bad] = 30.0, 1e-16
    one = np.empty(d + 2)
    v = C.c_double(0.0)
    single = getattr(gp._lib, "bobe_gp_mll_noise" if obj == "mll" else "bobe_gp_loo_objective_noise")
    assert single(gp._h, _lib.ptr(ls2[bad]), float(kv[bad]), float(nz2[bad]), C.byref(v), _lib.ptr(one)) == _lib.BOBE_NOT_PD
    assert np.isnan(v.value) and np.all(np.isnan(one))
    for want_grad in (True, False):
        st, val, grad, status = _raw_batch(gp, obj, ls2, kv, nz2, want_grad)
        assert st == _lib.BOBE_NOT_PD
        assert status.tolist() == [_lib.BOBE_NOT_PD if b == bad else _lib.BOBE_OK for b in range(B)]
        keep = [b for b in range(B) if b != bad]
        assert np.isnan(val[bad]) and np.array_equal(val[keep], sv[keep])
        if want_grad:
            assert np.all(np.isnan(grad[bad])) and np.array_equal(grad[keep], sg[keep])


# ---- 3. nothing else moves --------------------------------------------------------------------------------------------------
def test_the_installed_state_and_the_existing_calls_keep_their_bits():
    n, d = 257, 5
    gp = _gp(n, d, "rbf", 1e-6)
    ls, kv, nz = _members(n, d, "rbf", 3)
    Xq = np.random.default_rng(9).uniform(size=(40, d))

    def snapshot():
        m, v = gp.predict_batched(Xq)
        r = gp.loo()
        return [m, v, r["mean"], r["var"], r["lpd"], np.array(r["elpd"]), *gp.mll_data_batch(ls, kv), *gp.loo_data_batch(ls, kv),
                np.array(gp.mll_data(ls[0], kv[0])[0]), gp.loo_data(ls[0], kv[0])[1]]
    before = snapshot()
    for obj in OBJECTIVES:
        _noise_fn(gp, obj)(ls[1], kv[1], nz[1])
        _noise_fn(gp, obj, batch=True)(ls, kv, nz)
        _noise_fn(gp, obj, batch=True)(ls, kv, nz, want_grad=False)
    after = snapshot()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# ---- 4. adoption ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["single", "batch"])
def test_an_mll_evaluation_is_adopted_with_its_own_noise(form):
    from bobe_amd import GP
    n, d = 130, 3
    X, f, ls0, kvar0 = _data(n, d, "matern")
    gp = _gp(n, d, "matern", 1e-8)
    ls, kv, nz = _members(n, d, "matern", 3)
    Xq = np.random.default_rng(3).uniform(size=(25, d))
    pick = 2
    if form == "single":
        gp.mll_data_noise(ls[pick], kv[pick], nz[pick])
    else:
        gp.mll_data_noise_batch(ls, kv, nz)
    gp.lengthscales, gp.kernel_variance, gp.noise = np.array(ls[pick]), float(kv[pick]), float(nz[pick])
    gp.recompute_cholesky()
    src = gp._lib.bobe_debug_factor_source(gp._h)
    assert src in (1, 3) and src == (3 if form == "single" else 1), src
    fresh = GP(X, f, noise=float(nz[pick]), kernel="matern", lengthscales=ls[pick], kernel_variance=float(kv[pick]),
               pivot_floor_ulp=0.0)
    assert fresh._lib.bobe_debug_factor_source(fresh._h) == 0
    for a, b in zip(gp.predict_batched(Xq), fresh.predict_batched(Xq)):
        assert np.array_equal(a, b)
    assert np.array_equal(gp.predict_var_batched(Xq), fresh.predict_var_batched(Xq))
    # the LOO form leaves nothing to adopt
    if form == "single":
        gp.loo_data_noise(ls[0], kv[0], nz[0])
    else:
        gp.loo_data_noise_batch(ls, kv, nz)
    gp.lengthscales, gp.kernel_variance, gp.noise = np.array(ls[0]), float(kv[0]), float(nz[0])
    gp.recompute_cholesky()
    assert gp._lib.bobe_debug_factor_source(gp._h) == 0


# ---- 5. a fit recovers a known noise level ----------------------------------------------------------------------------------
def _noisy_data():
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(200, 2))
    f = np.sin(4.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]) + X[:, 0] + X[:, 1]
    y = f + 0.1 * np.std(f) * rng.standard_normal(200)
    return X, y, float((0.1 * np.std(f)) ** 2 / np.var(y))


def _handed_tolerances():
    """The stopping tolerances optimize_scipy hands to L-BFGS-B when no options are given, read from optim.py."""
    from bobe_amd import optim
    src = inspect.getsource(optim.optimize_scipy)
    return (float(re.search(r'"ftol":\s*([0-9.eE+-]+)', src).group(1)), float(re.search(r'"gtol":\s*([0-9.eE+-]+)', src).group(1)))


def _starts(gp, n_restarts, seed):
    """gp_fit's recipe: the incumbent, then uniform draws in the log-bounds (the noise coordinate: log-uniform in its bounds)."""
    init = np.log(gp.get_hyperparams())
    rng = np.random.default_rng(seed)
    return np.vstack([init, rng.uniform(gp.hyperparam_bounds[0], gp.hyperparam_bounds[1], size=(n_restarts - 1, len(init)))])


def _restatement_objective(obj, X, ys):
    def fun(th):
        try:
            r = NR.noise_closed_theta("rbf", X, ys, th, np.float64)
        except np.linalg.LinAlgError:
            return np.nan, np.full(len(th), np.nan)
        g = -np.asarray(r[obj + "_grad"], dtype=np.float64)
        v = -float(r[obj])
        return (v, g) if np.isfinite(v) and np.all(np.isfinite(g)) else (np.nan, np.full(len(th), np.nan))
    return fun


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_a_fit_recovers_a_known_noise_level(obj):
    from scipy.optimize import minimize
    from bobe_amd import GP
    X, y, nu_true = _noisy_data()
    assert abs(nu_true - 9.61e-3) < 5e-5
    ftol, gtol = _handed_tolerances()
    opts = {"method": "L-BFGS-B", "ftol": ftol, "gtol": gtol}
    gp = GP(X, y, kernel="rbf", fit_noise=True, fit_objective=obj, optimizer_options=opts)
    assert gp.noise == 1e-8 and gp.hyperparam_names[-1] == "noise"
    x0 = _starts(gp, 4, seed=1)
    res = gp.fit(x0=x0, maxiter=500)
    gp.update_hyperparams(res["params"])
    ratio = gp.noise / nu_true
    # the CPU restatement's own L-BFGS-B optimum from the same starts, with the same tolerances
    ys = NR.standardise(y)
    fun = _restatement_objective(obj, X, ys)
    bounds = [(float(lo), float(hi)) for lo, hi in gp.hyperparam_bounds.T]
    best = None
    for s in x0:
        if not np.isfinite(fun(s)[0]):
            continue
        r = minimize(fun, s, jac=True, method="L-BFGS-B", bounds=bounds, options={"ftol": ftol, "gtol": gtol, "maxiter": 500})
        if np.isfinite(r.fun) and (best is None or r.fun < best.fun):
            best = r
    f_dev, f_ref = fun(np.asarray(res["params"]))[0], float(best.fun)
    diff = abs(f_dev - f_ref) / abs(f_ref)
    print(f"[noise fit] {obj}: device nu = {gp.noise:.4e} (ratio {ratio:.3f} to the true {nu_true:.4e}); restatement nu = "
          f"{np.exp(best.x[-1]):.4e} (ratio {np.exp(best.x[-1]) / nu_true:.3f}); restatement objective at the device optimum "
          f"{f_dev:.10g}, at its own {f_ref:.10g}: relative difference {diff:.3e} (ftol {ftol:g})")
    assert 0.5 <= ratio <= 2.0, ratio
    assert gp.noise_bounds[0] <= gp.noise <= gp.noise_bounds[1] and not gp.not_pd
    assert diff <= ftol, (f_dev, f_ref, diff, ftol)
    # the same GP with the option off keeps its noise, and its fit is that of a GP built without the three keywords
    off = GP(X, y, kernel="rbf", fit_objective=obj, optimizer_options=opts, fit_noise=False, noise_bounds=[1e-9, 1e-2],
             noise_prior={"name": "LogNormal", "loc": -9.0, "scale": 1.0})
    bare = GP(X, y, kernel="rbf", fit_objective=obj, optimizer_options=opts)
    r1, r2 = off.fit(x0=x0[:, :-1], maxiter=100), bare.fit(x0=x0[:, :-1], maxiter=100)
    assert off.hyperparam_names == ["lengthscales", "kernel_variance"] and len(r1["params"]) == 3
    assert r1["mll"] == r2["mll"] and np.array_equal(r1["params"], r2["params"])
    off.update_hyperparams(r1["params"])
    bare.update_hyperparams(r2["params"])
    assert off.noise == 1e-8 and bare.noise == 1e-8
    Xq = np.random.default_rng(12).uniform(size=(16, 2))
    for a, b in zip(off.predict_batched(Xq), bare.predict_batched(Xq)):
        assert np.array_equal(a, b)


# ---- 6. lock step equals one after another ----------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", OBJECTIVES)
def test_lock_step_restarts_equal_sequential_ones(obj):
    from bobe_amd import GP
    from bobe_amd.optim import _rc_available
    if not _rc_available():
        pytest.fail("SciPy's L-BFGS-B routine cannot be stepped here: the lock-step fit is unavailable")
    X, y, _ = _noisy_data()
    out = []
    for mode in ("lockstep", "sequential", "slots"):
        gp = GP(X, y, kernel="rbf", fit_noise=True, fit_objective=obj, noise=1e-4)
        if mode == "sequential":
            gp.concurrent_restarts = False
        else:
            gp.restart_mode = mode                   # ('slots': no slot form of the noise calls - one after another)
        out.append(gp.fit(x0=_starts(gp, 4, seed=2), maxiter=60))
    for r in out[1:]:
        assert r["mll"] == out[0]["mll"] and np.array_equal(r["params"], out[0]["params"])
    assert np.isfinite(out[0]["mll"]) and len(out[0]["params"]) == 4


# ---- 7. round trips ---------------------------------------------------------------------------------------------------------
def test_round_trips_keep_the_option_and_the_fitted_noise(tmp_path):
    from bobe_amd import GP
    from bobe_amd.bo import gp_fit
    X, y, nu_true = _noisy_data()
    gp = GP(X[:150], y[:150], kernel="rbf", fit_noise=True, noise_bounds=[1e-9, 5e-2])
    gp_fit(gp, maxiters=100, n_restarts=2, rng=np.random.default_rng(4), distributed=False)
    nu = gp.noise
    assert 1e-9 <= nu <= 5e-2 and nu != 1e-8
    Xq = np.random.default_rng(6).uniform(size=(20, 2))
    want = gp.predict_mean_batched(Xq)
    gp.save(str(tmp_path / "g"))
    copies = {"from_state_dict": GP.from_state_dict(gp.state_dict()), "load": GP.load(str(tmp_path / "g")), "copy": gp.copy()}
    for name, c in copies.items():
        assert c.fit_noise is True and c.noise_bounds == [1e-9, 5e-2] and c.noise == nu, name
        assert c.hyperparam_names == gp.hyperparam_names and c.num_hyperparams == 4, name
        assert np.allclose(c.predict_mean_batched(Xq), want, rtol=1e-9, atol=1e-9), name
    assert np.array_equal(copies["copy"].predict_mean_batched(Xq), want)
    # an update with append_updates uses the fitted noise: the appended factor is the one a fresh GP at that noise builds
    c = copies["copy"]
    assert c.append_updates
    c.update(X[150:153], y[150:153].reshape(-1, 1))
    assert c.noise == nu and c.npoints == 153
    fresh = GP(X[:153], y[:153], kernel="rbf", noise=nu, lengthscales=gp.lengthscales, kernel_variance=gp.kernel_variance)
    assert np.allclose(c.predict_mean_batched(Xq), fresh.predict_mean_batched(Xq), rtol=1e-8, atol=1e-8)
    assert np.allclose(c.predict_var_batched(Xq), fresh.predict_var_batched(Xq), rtol=1e-6, atol=1e-12)


def test_a_classifier_gp_fits_its_noise_and_gates_as_before():
    from bobe_amd.bo import gp_fit
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, size=(120, 2))
    y = -2000.0 * np.sum((X - 0.5) ** 2, axis=1, keepdims=True) + 0.5 * rng.standard_normal((120, 1))
    kw = dict(clf_threshold=150.0, gp_threshold=400.0, lengthscales=[0.3, 0.3])
    g = GPwithClassifier(X, y, noise=1e-6, fit_noise=True, **kw)
    plain = GPwithClassifier(X, y, noise=1e-6, **kw)
    assert g.hyperparam_names[-1] == "noise" and plain.hyperparam_names[-1] != "noise"
    gp_fit(g, maxiters=60, n_restarts=2, rng=np.random.default_rng(8), distributed=False)
    assert g.noise_bounds[0] <= g.noise <= g.noise_bounds[1] and not g.not_pd
    q = np.array([[0.5, 0.5], [0.52, 0.47], [0.02, 0.03], [0.97, 0.99]])
    assert np.array_equal(g._clf_predict_func(q), plain._clf_predict_func(q))           # the same gate
    m = g.predict_mean_batched(q)
    assert np.all(np.isfinite(m[:2])) and np.all(m[2:] == g.minus_inf)
    st = g.state_dict()
    assert st["fit_noise"] is True and "fit_noise" not in plain.state_dict()
    back = GPwithClassifier.from_state_dict(st)
    assert back.fit_noise is True and back.noise == g.noise and back.hyperparam_names[-1] == "noise"


# ---- 8. the BO loop ---------------------------------------------------------------------------------------------------------
def test_the_bo_loop_runs_with_a_fitted_noise(tmp_path):
    from bobe_amd.bo import BOBE
    scatter = np.random.default_rng(17)

    def himmelblau(x):                                          # tests/test_gpu_bo.py's, plus seeded additive noise
        return -((x[0] ** 2 + x[1] - 11) ** 2 + (x[0] + x[1] ** 2 - 7) ** 2) / 10.0 + 0.05 * scatter.standard_normal()

    bounds = np.array([[-4.0, 4.0], [-4.0, 4.0]]).T
    bobe = BOBE(himmelblau, ["x", "y"], bounds, n_sobol_init=8, seed=2, likelihood_name="himmel", save=True,
                save_dir=str(tmp_path), save_step=1, gp_kwargs={"fit_noise": True})
    assert bobe.gp.fit_noise and bobe.gp.hyperparam_names[-1] == "noise"
    # the smallest budget of tests/test_gpu_bo.py: twelve evaluations, a refit every two points
    res = bobe.run(acq="wipstd", max_evals=12, fit_n_points=2, batch_size=2, mc_points_size=64, num_mc_samples=256,
                   mc_points_method="uniform", min_evals=100)
    assert res["n_evals"] == 12 and res["gp"].npoints == 12
    gp = res["gp"]
    hp = gp.hyperparams_dict()
    assert gp.noise_bounds[0] <= float(hp["noise"]) <= gp.noise_bounds[1]
    assert gp.noise_bounds[0] <= gp.noise <= gp.noise_bounds[1]
    assert all("noise" in h for h in bobe.gp_hyperparam_history)
    assert (tmp_path / "himmel_gp.npz").exists() and (tmp_path / "himmel_run.json").exists()
    z = np.load(tmp_path / "himmel_gp.npz", allow_pickle=True)
    assert bool(z["fit_noise"]) is True


# ---- 9. ABI errors ----------------------------------------------------------------------------------------------------------
def test_bad_noise_arguments_are_refused_and_leave_the_handle_usable():
    from bobe_amd import _lib
    n, d = 50, 2
    gp = _gp(n, d, "rbf", 1e-6)
    _, _, ls, kvar = _data(n, d, "rbf")
    lib, ERR_ARG = gp._lib, -1
    good = gp.mll_data_noise(ls, kvar, 1e-3)
    lsb, kvb = np.ascontiguousarray([ls, ls]), np.array([kvar, kvar])
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        for name in ("bobe_gp_mll_noise", "bobe_gp_loo_objective_noise"):
            v, g = C.c_double(0.0), np.empty(d + 2)
            assert getattr(lib, name)(gp._h, _lib.ptr(ls), kvar, bad, C.byref(v), _lib.ptr(g)) == ERR_ARG, (name, bad)
            assert "noise" in _lib.last_error()
        for name in ("bobe_gp_mll_noise_batch", "bobe_gp_loo_objective_noise_batch"):
            val, g = np.empty(2), np.empty((2, d + 2))
            nz = np.array([1e-3, bad])
            assert getattr(lib, name)(gp._h, 2, _lib.ptr(lsb), _lib.ptr(kvb), _lib.ptr(nz), _lib.ptr(val), _lib.ptr(g),
                                      None) == ERR_ARG, (name, bad)
            assert "noise" in _lib.last_error()
    for name in ("bobe_gp_mll_noise_batch", "bobe_gp_loo_objective_noise_batch"):
        val, g = np.empty(2), np.empty((2, d + 2))
        assert getattr(lib, name)(gp._h, 2, _lib.ptr(lsb), _lib.ptr(kvb), None, _lib.ptr(val), _lib.ptr(g), None) == ERR_ARG
        assert "NULL" in _lib.last_error()
    again = gp.mll_data_noise(ls, kvar, 1e-3)
    assert again[0] == good[0] and np.array_equal(again[1], good[1])
    assert np.all(np.isfinite(gp.predict_batched(np.full((1, d), 0.5))[0]))
