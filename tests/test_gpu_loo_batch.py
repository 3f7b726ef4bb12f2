"""The LOO objective for several hyper-parameter vectors in lock step (bobe_gp_loo_objective_batch, GP.loo_data_batch /
neg_loo_value_and_grad_batch, the lock-step ``fit_objective='loo'`` fit).

Every comparison here is bitwise: a batch member must return the bits of the single evaluation (``GP.loo_data`` /
bobe_gp_loo_objective on the same handle), whose own parity against the extended-precision truth tests/test_gpu_loo.py pins.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conditioning_common import LADDER, NOISE, _bo_like_design

pytestmark = pytest.mark.gpu

GOLDEN = ["rbf_n50_d2", "matern_n130_d3", "rbf_n257_d5_saas"]
CASES = GOLDEN + ["rung0_first600"]
WIDTHS = [1, 2, 3, 8, 11]                      # 11 = 8 + 3: two chunks of the batch workspace
_HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(kernel, X, y physical, ls, kvar, noise) of a named case."""
    if name in GOLDEN:
        z = np.load(os.path.join(_HERE, "golden", name + ".npz"), allow_pickle=True)
        return (str(z["kernel"]), z["X"], z["y"].reshape(-1), np.array(z["lengthscales"], dtype=float),
                float(z["kernel_variance"]), float(z["noise"]))
    n, kernel, ls, kvar = LADDER[0]
    X, y, _ = _bo_like_design(n)
    return kernel, X[:600], y[:600], np.array(ls), kvar, NOISE


@functools.lru_cache(maxsize=None)
def _gp(name):
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case(name)
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0)


def _members(name, B):
    """B distinct hyper-parameter vectors around the case's own: member b scales ls by 0.7 + 0.1 b, kvar by 0.5 + 0.25 b"""
    _, _, _, ls, kvar, _ = _case(name)
    return (np.array([ls * (0.7 + 0.1 * b) for b in range(B)]), np.array([kvar * (0.5 + 0.25 * b) for b in range(B)]))


@functools.lru_cache(maxsize=None)
def _singles(name):
    """The reference, computed once per case: the single evaluation at the 11 members, with and without a gradient."""
    gp = _gp(name)
    ls, kv = _members(name, max(WIDTHS))
    with_grad = [gp.loo_data(ls[b], kv[b]) for b in range(len(kv))]
    values = np.array([gp.loo_data(ls[b], kv[b], want_grad=False)[0] for b in range(len(kv))])
    vals, grads = np.array([v for v, _ in with_grad]), np.array([g for _, g in with_grad])
    assert np.array_equal(vals, values) and np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))
    vals.setflags(write=False)
    grads.setflags(write=False)
    return vals, grads


# ---- 1. members return the single evaluation's bits -------------------------------------------------------------------------
@pytest.mark.parametrize("B", WIDTHS)
@pytest.mark.parametrize("name", CASES)
def test_members_return_the_single_evaluations_bits(name, B):
    gp = _gp(name)
    sv, sg = _singles(name)
    ls, kv = _members(name, B)
    val, grad = gp.loo_data_batch(ls, kv)
    assert val.shape == (B,) and grad.shape == (B, gp.ndim + 1)
    assert np.array_equal(val, sv[:B]) and np.array_equal(grad, sg[:B])
    val0, none = gp.loo_data_batch(ls, kv, want_grad=False)
    assert none is None and np.array_equal(val0, sv[:B])
    again_v, again_g = gp.loo_data_batch(ls, kv)                       # the same call again: the same bits
    assert np.array_equal(again_v, val) and np.array_equal(again_g, grad)
    perm = np.random.default_rng(B).permutation(B)                     # member b of the batch is theta_b
    pv, pg = gp.loo_data_batch(ls[perm], kv[perm])
    assert np.array_equal(pv, sv[:B][perm]) and np.array_equal(pg, sg[:B][perm])


# ---- 2. 128 x 128 tiles -----------------------------------------------------------------------------------------------------
def test_members_on_128_tiles_return_the_single_evaluations_bits():
    """From 49 block columns up K^-1 and B^T B run on 128 x 128 tiles: the only shape where k_loo_grad<., ., 128> and the
    128-tile store of K^-1 run with a member stride."""
    from bobe_amd import GP
    n, d = 6272, 2
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(n, d))
    y = np.sin(5.0 * X[:, 0]) * np.cos(3.0 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    ls, kvar = np.array([0.25, 0.4]), 1.2
    gp = GP(X, y, noise=1e-2, kernel="matern", lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=0.0)
    lsb, kvb = np.array([ls, ls * 1.2]), np.array([kvar, kvar * 0.8])
    single = [gp.loo_data(lsb[b], kvb[b]) for b in range(2)]
    val, grad = gp.loo_data_batch(lsb, kvb)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    for b in range(2):
        assert val[b] == single[b][0] and np.array_equal(grad[b], single[b][1]), b


# ---- 3. a failing member does not touch its neighbours ----------------------------------------------------------------------
def test_a_failing_member_does_not_touch_its_neighbours():
    from bobe_amd import GP, _lib
    X = np.random.default_rng(31).uniform(size=(200, 2))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2
    gp = GP(X, y, noise=0.0, kernel="rbf", lengthscales=[0.05, 0.05], kernel_variance=1.0, pivot_floor_ulp=64)
    assert not gp.not_pd
    lib = gp._lib
    ls = np.ascontiguousarray([[0.05, 0.05], [3.0, 3.0], [0.08, 0.08]])
    kv = np.ones(3)
    sv, sg, sst = np.empty(3), np.empty((3, 3)), []
    for b in range(3):                                   # the precondition: OK, not PD, OK one at a time
        v = C.c_double(0.0)
        sst.append(lib.bobe_gp_loo_objective(gp._h, _lib.ptr(ls[b]), 1.0, C.byref(v), _lib.ptr(sg[b])))
        sv[b] = v.value
    assert sst == [_lib.BOBE_OK, _lib.BOBE_NOT_PD, _lib.BOBE_OK]
    assert np.isnan(sv[1]) and np.all(np.isnan(sg[1])) and np.all(np.isfinite(sv[[0, 2]])) and np.all(np.isfinite(sg[[0, 2]]))
    for want_grad in (True, False):
        val, grad, status = np.zeros(3), np.zeros((3, 3)), np.full(3, -7, dtype=np.int32)
        st = lib.bobe_gp_loo_objective_batch(gp._h, 3, _lib.ptr(ls), _lib.ptr(kv), _lib.ptr(val),
                                             _lib.ptr(grad) if want_grad else None, C.c_void_p(status.ctypes.data))
        assert st == _lib.BOBE_NOT_PD
        assert status.tolist() == [_lib.BOBE_OK, _lib.BOBE_NOT_PD, _lib.BOBE_OK]
        assert np.isnan(val[1]) and val[0] == sv[0] and val[2] == sv[2]
        if want_grad:
            assert np.all(np.isnan(grad[1])) and np.array_equal(grad[0], sg[0]) and np.array_equal(grad[2], sg[2])
    assert np.isfinite(gp.loo()["elpd"])                 # the handle stays usable


# ---- 4. state and records ---------------------------------------------------------------------------------------------------
def test_batch_leaves_the_state_alone_and_no_factor_to_adopt():
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case("matern_n130_d3")
    kw = dict(noise=noise, kernel=kernel, pivot_floor_ulp=0.0)
    gp = GP(X, y, lengthscales=ls, kernel_variance=kvar, **kw)
    xq = np.random.default_rng(2).uniform(size=(40, 3))
    m0, v0 = gp.predict_batched(xq)
    l0 = gp.loo()

    def state_is_untouched():
        m1, v1 = gp.predict_batched(xq)
        l1 = gp.loo()
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
        assert np.array_equal(l0["mean"], l1["mean"]) and np.array_equal(l0["var"], l1["var"]) and l0["elpd"] == l1["elpd"]

    thetas = [np.log(np.append(ls * (0.7 + 0.1 * b), kvar * (0.5 + 0.25 * b))) for b in range(4)]
    mll_before = gp.neg_mll_value_and_grad_batch(thetas)          # arms the batch workspace's records
    state_is_untouched()
    loo = gp.neg_loo_value_and_grad_batch(thetas)                 # overwrites the members' L: the records must go
    state_is_untouched()
    for t, (f, g) in zip(thetas, loo):
        fs, gs = gp.neg_loo_value_and_grad(t)
        assert f == fs and np.array_equal(g, gs)
    state_is_untouched()
    mll_after = gp.neg_mll_value_and_grad_batch(thetas)
    for (fa, ga), (fb, gb) in zip(mll_before, mll_after):
        assert fa == fb and np.array_equal(ga, gb)
    gp.neg_loo_value_and_grad_batch(thetas)                       # the records of that MLL batch are cleared again ...
    gp.update_hyperparams(thetas[0])                              # ... so this factorises instead of adopting B for L
    ls0, kv0, _ = gp._parse_hyperparams(thetas[0])
    fresh = GP(X, y, lengthscales=ls0, kernel_variance=kv0, **kw)
    ma, va = gp.predict_batched(xq)
    mb, vb = fresh.predict_batched(xq)
    la, lb = gp.loo(), fresh.loo()
    assert np.array_equal(ma, mb) and np.array_equal(va, vb)
    assert np.array_equal(la["mean"], lb["mean"]) and np.array_equal(la["var"], lb["var"]) and la["elpd"] == lb["elpd"]


# ---- 5. the fit -------------------------------------------------------------------------------------------------------------
def _fit_gp():
    """The GP and the four starts of test_gpu_loo.py's _fit_case on matern_n130_d3"""
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case("matern_n130_d3")
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, lengthscale_bounds=[0.05, 2.0],
            kernel_variance_bounds=[1e-2, 1e2], optimizer_options={"method": "L-BFGS-B"}, fit_objective="loo")
    th0 = np.log(np.append(ls, kvar))
    x0 = np.vstack([th0, th0 + np.random.default_rng(21).uniform(-0.6, 0.6, size=(3, X.shape[1] + 1))])
    return gp, np.clip(x0, gp.hyperparam_bounds[0], gp.hyperparam_bounds[1])


def test_lock_step_fit_is_the_sequential_fit(monkeypatch):
    from bobe_amd import _lib
    from bobe_amd.optim import _rc_available
    lib = _lib.load()
    orig = lib.bobe_gp_loo_objective_batch
    calls = []

    def counted(*a):
        calls.append(int(a[1]))
        return orig(*a)
    monkeypatch.setattr(lib, "bobe_gp_loo_objective_batch", counted)
    gp, x0 = _fit_gp()
    assert gp.concurrent_restarts and gp.restart_mode == "auto" and _rc_available()
    a = gp.fit(x0=x0, maxiter=500)
    n_lock = len(calls)
    seq, _ = _fit_gp()
    seq.concurrent_restarts = False
    b = seq.fit(x0=x0, maxiter=500)
    print(f"[loo batch] lock-step fit: {n_lock} batch calls, widths {sorted(set(calls))}; optimum {a['params']} ({a['mll']:.6f})")
    assert n_lock >= 1 and len(calls) == n_lock                     # the second fit never took the batch entry point
    assert a["mll"] == b["mll"] and np.array_equal(a["params"], b["params"])
    slots, _ = _fit_gp()                                            # no slot form: one restart after another, same result
    slots.restart_mode = "slots"
    c = slots.fit(x0=x0, maxiter=500)
    assert len(calls) == n_lock and c["mll"] == b["mll"] and np.array_equal(c["params"], b["params"])


def test_neg_loo_batch_assembles_priors_like_the_single_call():
    from bobe_amd import GP
    kernel, X, y, ls, kvar, noise = _case("matern_n130_d3")
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, lengthscale_prior="DSLP")
    thetas = [np.log(np.append(ls, kvar)) + 0.1 * (b - 1) for b in range(3)]
    for want_grad in (True, False):
        out = gp.neg_loo_value_and_grad_batch(thetas, want_grad=want_grad)
        for t, (f, g) in zip(thetas, out):
            fs, gs = gp.neg_loo_value_and_grad(t, want_grad=want_grad)
            assert f == fs and (g is None and gs is None if not want_grad else np.array_equal(g, gs))
    fixed = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, kernel_variance_prior="fixed")
    thetas = [np.log(ls) + 0.05 * b for b in range(3)]
    out = fixed.neg_loo_value_and_grad_batch(thetas)
    for t, (f, g) in zip(thetas, out):
        fs, gs = fixed.neg_loo_value_and_grad(t)
        assert g.shape == (3,) and f == fs and np.array_equal(g, gs)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------
def test_error_contract():
    from bobe_amd import _lib
    lib = _lib.load()
    X = np.random.default_rng(0).uniform(size=(30, 2))
    y = np.sin(3 * X[:, 0]) + X[:, 1]
    ys = np.ascontiguousarray((y - y.mean()) / y.std())
    ls, kv = np.full((2, 2), 0.4), np.ones(2)
    val, grad, status = np.zeros(2), np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    p = _lib.ptr
    h = C.c_void_p(0)
    assert lib.bobe_gp_create(C.byref(h), 0, 0, 2) == 0
    try:
        assert lib.bobe_gp_loo_objective_batch(h, 2, p(ls), p(kv), p(val), p(grad), None) == -3       # BOBE_ERR_STATE: no data
        assert lib.bobe_gp_set_data(h, p(X), p(ys), 30) == 0
        assert lib.bobe_gp_set_hyper(h, p(ls[0]), 1.0, 1e-6) == 0
        assert lib.bobe_gp_loo_objective_batch(None, 2, p(ls), p(kv), p(val), p(grad), None) == -1    # BOBE_ERR_ARG
        assert lib.bobe_gp_loo_objective_batch(h, 2, None, p(kv), p(val), p(grad), None) == -1
        assert lib.bobe_gp_loo_objective_batch(h, 2, p(ls), None, p(val), p(grad), None) == -1
        assert lib.bobe_gp_loo_objective_batch(h, 2, p(ls), p(kv), None, p(grad), None) == -1
        assert lib.bobe_gp_loo_objective_batch(h, 0, p(ls), p(kv), p(val), p(grad), None) == -1
        assert lib.bobe_gp_loo_objective_batch(h, -1, p(ls), p(kv), p(val), p(grad), None) == -1
        assert lib.bobe_gp_loo_objective_batch(h, 2, p(ls), p(kv), p(val), None, None) == 0           # grad, status may be NULL
        v0 = val.copy()
        assert lib.bobe_gp_loo_objective_batch(h, 2, p(ls), p(kv), p(val), p(grad), C.c_void_p(status.ctypes.data)) == 0
        assert np.array_equal(val, v0) and val[0] == val[1] and np.all(np.isfinite(grad)) and status.tolist() == [0, 0]
    finally:
        lib.bobe_gp_destroy(h)
