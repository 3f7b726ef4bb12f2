"""bobe_gp_acq_ei_grad (GP.acq_ei_grad) and the lock-step restarts of EI / LogEI built on it, against the 50-digit truth of
tests/ei_grad_restatement.py at the launch shapes of tests/ei_grad_cases.py: two query workgroups with a ragged second one,
d equal to a DCAP, a single query, N = 3, two chunks, the ill-conditioned family (u from -4500 to +1000), the variance floor.

The rule is the one of tests/test_gpu_posterior_grad.py, per case, (best_y, zeta) pair, mode and output,
over all of the case's queries and coordinates:

    max |device - truth| <= 4 max |fp64 restatement - truth| + 1e-8 max |truth|.

Every measured pair is printed before it is asserted; with BOBE_EI_GRAD_PARITY_OUT=<file> the table is written there
(committed as profiles/ei_grad_parity.txt).  tests/test_ei_grad_cpu.py holds the fp64 restatement of every case here within
1e-8 of the truth, so the ``4 x ref`` term cannot swallow an error above ~4e-8."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ei_grad_cases as EC  # noqa: E402
from test_gpu_posterior_grad import _Chunk, _make  # noqa: E402
from test_gpu_weighted_criteria import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
_ROWS = {}


def _record(label, rows):
    _ROWS[label] = rows
    out = os.environ.get("BOBE_EI_GRAD_PARITY_OUT")
    if not out:
        return
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    lines = ["# EI / LogEI values and input gradients (tests/test_gpu_ei_grad.py): max |delta| / max |truth| over the case's "
             "queries and coordinates, against the 50-digit truth on the long-double posterior",
             "# dev = the device, ref = the fp64 restatement (tests/ei_grad_restatement.py on SciPy's posterior); "
             "rule: dev <= 4 x ref + 1e-8", "",
             f"{'case':<62}{'output':<12}{'dev':>11}{'ref':>11}{'max|truth|':>12}"]
    for nm, rs in _ROWS.items():
        for key, dev, ref, scale in rs:
            lines.append(f"{nm:<62}{key:<12}{dev:>11.2e}{ref:>11.2e}{scale:>12.3e}")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _hold_to_the_rule(label, triples):
    """triples: (output, device, fp64 restatement, truth).  Prints and records every pair, then asserts the rule."""
    rows = []
    for key, dev, f64, truth in triples:
        dev = np.asarray(dev)
        assert dev.shape == truth.shape and np.all(np.isfinite(dev)), key
        scale = float(np.max(np.abs(truth)))
        e_dev, e_ref = EC.rel_err(dev, truth), EC.rel_err(f64, truth)
        rows.append((key, e_dev, e_ref, scale))
        print(f"[ei grad parity] {label:<62} {key:<11} err(device) = {e_dev:.3e}   err(fp64 restatement) = {e_ref:.3e}   "
              f"max |truth| = {scale:.3e}")
    _record(label, rows)
    for key, e_dev, e_ref, _ in rows:
        assert e_dev <= 4.0 * e_ref + 1e-8, (label, key, e_dev, e_ref)


@functools.lru_cache(maxsize=None)
def _gp(case):
    kernel, d, X, y, _, noise, ell, kvar, _ = EC.data(case)
    return _make(kernel, X, y, d, noise, ell, kvar)


# ------------------------------------------------------------------------------------------------- a. against the truth
@pytest.mark.parametrize("combo", EC.COMBOS, ids=[EC.combo_id(c) for c in EC.COMBOS])
def test_acq_ei_grad_against_the_truth(combo):
    case, pair, log_ei = combo
    _, d, _, _, Q, _, _, _, chunk = EC.data(case)
    best_y, zeta = EC.best_and_zeta(case, pair)
    r = EC.reference(case, pair, log_ei)
    (tv, tg, _), (fv, fg, _) = r["truth"], r["f64"]
    gp = _gp(case)
    with _Chunk(gp, chunk):
        val, grad = gp.acq_ei_grad(Q, best_y, zeta, log_ei=log_ei)
    assert val.shape == (len(Q),) and grad.shape == (len(Q), d)
    triples = [("val", val, fv, tv), ("grad", grad, fg, tg)]
    if EC.is_floor(case):
        # rows 0, 1 sit on the 1e-12 floor: no dsigma, and the truth of their gradient is A dm alone - Phi(u) dm in plain EI
        _, v, _, dv = gp.predict_grad(Q)
        assert v[0] == 1e-12 and v[1] == 1e-12 and np.all(dv[:2] == 0.0)
        if np.any(tg[:2] != 0.0):
            triples.append(("grad_floor", grad[:2], fg[:2], tg[:2]))
        else:                          # (both floored rows at u ~ -4e6 in plain EI: Phi(u) is 0 in any precision, no scale to hold to)
            assert np.all(grad[:2] == 0.0)
    _hold_to_the_rule(EC.combo_id(combo), triples)


# -------------------------------------------------------------------------------------------------- b. batch independence
@pytest.mark.parametrize("log_ei", EC.MODES, ids=["ei", "logei"])
def test_a_point_does_not_depend_on_its_batch(log_ei):
    """The chunked case: the second launch's rows are those of the same queries sent alone, with the chunk still set and with
    the default one; and a single row alone."""
    case = ("matern", 5, 300, 200, 128)
    Q = EC.data(case)[4]
    best_y, zeta = EC.best_and_zeta(case, "median")
    gp = _gp(case)
    with _Chunk(gp, 128):
        full = gp.acq_ei_grad(Q, best_y, zeta, log_ei=log_ei)
        tail = gp.acq_ei_grad(Q[128:], best_y, zeta, log_ei=log_ei)
    alone = gp.acq_ei_grad(Q[128:], best_y, zeta, log_ei=log_ei)
    one = gp.acq_ei_grad(Q[199:], best_y, zeta, log_ei=log_ei)
    for got, a, b, c in zip(full, tail, alone, one):
        assert same_bits(got[128:], a) and same_bits(got[128:], b) and same_bits(got[199:], c)


# ------------------------------------------------------------------------------------------------------------ c. the gates
def _set_svm_gate(gp, Q):
    from bobe_amd import _lib
    d = Q.shape[1]
    sv, dual, gamma = np.full((1, d), 0.5), np.array([1.0]), 2.0
    dec = np.exp(-gamma * np.sum((Q - 0.5) ** 2, axis=1))
    assert gp._lib.bobe_gp_set_gate(gp._h, _lib.ptr(sv), 1, _lib.ptr(dual), -float(np.median(dec)), gamma, 0.5, -1e5) == 0


def _set_ellipsoid_gate(gp, Q):
    from bobe_amd import _lib
    d = Q.shape[1]
    flat = np.zeros(d * (d + 1) // 2)                       # raw diagonal 0 -> softplus(0) + 1e-4, no off-diagonal terms
    mu = np.full(d, 0.5)
    md2 = (np.log(2.0) + 1e-4) ** 2 * np.sum((Q - 0.5) ** 2, axis=1)
    assert gp._lib.bobe_gp_set_gate_ellipsoid(gp._h, _lib.ptr(flat), _lib.ptr(mu), 1.0, float(np.median(md2)), 0.5, -1e5) == 0


@pytest.mark.parametrize("gate", ["svm", "ellipsoid"])
def test_gated_points_carry_the_value_of_acq_ei_and_no_gradient(gate):
    from bobe_amd.clf import gate_eval
    case, pair = EC.CASES[0], "best"
    _, d, _, _, Q, _, _, _, _ = EC.data(case)
    best_y, zeta = EC.best_and_zeta(case, pair)
    gp = _gp(case)
    try:
        (_set_svm_gate if gate == "svm" else _set_ellipsoid_gate)(gp, Q)
        ok = gate_eval(gp._lib, gp._h, Q, d)[1] == 1.0
        assert 10 < int(ok.sum()) < len(Q) - 10
        for log_ei in EC.MODES:
            val, grad = gp.acq_ei_grad(Q, best_y, zeta, log_ei=log_ei)
            assert same_bits(val[~ok], gp.acq_ei(Q, best_y, zeta, log_ei=log_ei)[~ok])
            assert np.all(grad[~ok] == 0.0) and np.all(np.isfinite(val))
            r = EC.reference(case, pair, log_ei)
            (tv, tg, _), (fv, fg, _) = r["truth"], r["f64"]
            _hold_to_the_rule(f"{EC.case_id(case)}-{pair}-{'logei' if log_ei else 'ei'}-{gate}_gate_feasible",
                              [("val", val[ok], fv[ok], tv[ok]), ("grad", grad[ok], fg[ok], tg[ok])])
    finally:
        assert gp._lib.bobe_gp_set_gate(gp._h, None, 0, None, 0.0, 0.0, 0.5, -1e5) == 0


# ------------------------------------------------------------------------------------------ d. predict_grad is left alone
def test_predict_grad_has_the_same_bits_before_and_after():
    case = ("matern", 5, 300, 200, 128)
    Q = EC.data(case)[4]
    gp = _gp(case)
    for chunk in (0, 128):
        with _Chunk(gp, chunk):
            before = gp.predict_grad(Q)
            gp.acq_ei_grad(Q, 0.3, 0.01, log_ei=True)
            after = gp.predict_grad(Q)
        for a, b in zip(before, after):
            assert same_bits(a, b)


# ------------------------------------------------------------------------------------------------- e. lock step, a real GP
class _Counted:
    """counts the calls of a GP's three entries and keeps the batch sizes of acq_ei_grad"""

    def __init__(self, gp):
        self.calls, self.rows = {"acq_ei_grad": 0, "predict_grad": 0, "acq_ei": 0}, []
        for name in self.calls:
            setattr(gp, name, self._wrap(name, getattr(gp, name)))

    def _wrap(self, name, fn):
        def counted(x, *a, **k):
            self.calls[name] += 1
            if name == "acq_ei_grad":
                self.rows.append(len(np.atleast_2d(x)))
            return fn(x, *a, **k)
        return counted


@pytest.mark.parametrize("name", ["EI", "LogEI"])
def test_lock_step_returns_the_bits_of_the_restarts_one_at_a_time(name, monkeypatch):
    from bobe_amd import GP
    from bobe_amd import acquisition as A
    rng = np.random.default_rng(60)
    X = rng.uniform(size=(60, 3))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2] * X[:, 0]
    gp = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(3, 0.4), kernel_variance=1.5)
    kw, args = {"zeta": 0.01, "ei_lockstep": True}, dict(maxiter=30, n_restarts=6, verbose=False)
    lock = _Counted(gp)
    x_lock, v_lock = getattr(A, name)().get_next_point(gp, acq_kwargs=dict(kw), rng=np.random.default_rng(2), **args)
    assert lock.calls["predict_grad"] == 0 and lock.calls["acq_ei"] == 0
    # the probe of the first start, the other five screened in one call, then one call per round: the restarts still running,
    # all six at first, fewer as they finish
    rounds = lock.rows[2:]
    assert lock.rows[:2] == [1, 5] and rounds[0] == 6 and all(a >= b for a, b in zip(rounds, rounds[1:]))
    real = A.optimize_scipy
    monkeypatch.setattr(A, "optimize_scipy", lambda fun, *a, batch_value_and_grad=None, **k: real(fun, *a, **k))
    gp1 = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(3, 0.4), kernel_variance=1.5)
    one = _Counted(gp1)
    x_one, v_one = getattr(A, name)().get_next_point(gp1, acq_kwargs=dict(kw), rng=np.random.default_rng(2), **args)
    monkeypatch.undo()
    assert set(one.rows) == {1} and len(one.rows) == sum(lock.rows)          # the same evaluations, one by one
    assert len(lock.rows) < len(one.rows)
    assert same_bits(x_lock, x_one) and same_bits(v_lock, v_one)
    print(f"{name}: {len(lock.rows)} device calls in lock step for {len(one.rows)} evaluations")


# ------------------------------------------------------------------------------------------------------ f. argument errors
def test_argument_errors_leave_the_handle_usable():
    from bobe_amd import GP, _lib
    case = EC.CASES[0]
    _, d, X, y, Q, _, _, _, _ = EC.data(case)
    gp = _gp(case)
    lib, h = gp._lib, gp._h
    q = np.ascontiguousarray(Q[:4])
    val, grad = np.empty(4), np.empty((4, d))
    want = gp.acq_ei_grad(q, 0.2, 0.0)
    for rc, text in ((lib.bobe_gp_acq_ei_grad(h, _lib.ptr(q), 0, 0.2, 0.0, 0, _lib.ptr(val), _lib.ptr(grad)), b"C must be"),
                     (lib.bobe_gp_acq_ei_grad(h, _lib.ptr(q), -3, 0.2, 0.0, 0, _lib.ptr(val), _lib.ptr(grad)), b"C must be"),):
        assert rc == ERR_ARG and text in lib.bobe_last_error()
    for mode in (2, -1):
        assert lib.bobe_gp_acq_ei_grad(h, _lib.ptr(q), 4, 0.2, 0.0, mode, _lib.ptr(val), _lib.ptr(grad)) == ERR_ARG
        assert b"mode" in lib.bobe_last_error()
    assert lib.bobe_gp_acq_ei_grad(h, _lib.ptr(q), 4, 0.2, 0.0, 0, None, _lib.ptr(grad)) == ERR_ARG
    assert lib.bobe_gp_acq_ei_grad(None, _lib.ptr(q), 4, 0.2, 0.0, 0, _lib.ptr(val), _lib.ptr(grad)) == ERR_ARG
    fresh = GP(X, y, noise=1e-6, kernel="matern", lengthscales=np.full(d, 0.4), kernel_variance=2.0, _factor=False)
    assert fresh._lib.bobe_gp_acq_ei_grad(fresh._h, _lib.ptr(q), 4, 0.2, 0.0, 0, _lib.ptr(val), _lib.ptr(grad)) == ERR_STATE
    assert fresh._lib.bobe_last_error()
    again = gp.acq_ei_grad(q, 0.2, 0.0)
    assert same_bits(want[0], again[0]) and same_bits(want[1], again[1])


# ------------------------------------------------------------------------------------------------------------ g. BOBE.run
def _gauss2d(x):
    return -0.5 * ((x[0] - 0.3) ** 2 / 0.04 + (x[1] + 0.2) ** 2 / 0.09)


def test_bo_run_with_lock_step_restarts():
    """plumbing, not parity: the run ends with the default run's result keys and a finite best value"""
    from bobe_amd.bo import BOBE
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]]).T
    kw = dict(max_evals=10, fit_n_points=4)
    res = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="ei", ei_lockstep=True, **kw)
    off = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="ei", **kw)
    assert set(res) == set(off)
    assert 8 < res["gp"].npoints <= 10 and np.isfinite(np.max(res["gp"].train_y))
    with pytest.raises(ValueError, match="ei_lockstep"):
        BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="wipstd", ei_lockstep=True, **kw)
