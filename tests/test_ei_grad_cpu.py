"""EI / LogEI input gradients without a device: the fp64 restatement of tests/ei_grad_restatement.py against its 50-digit truth
on every case of tests/test_gpu_ei_grad.py (so that the ``4 x ref`` term of the GPU rule cannot swallow a real error), the
truth against ``mpmath.diff`` of itself, two mistakes the cases have to see, the lock-step wiring of ``EI`` / ``LogEI`` on a
stand-in surrogate, and the declarations of ``bobe_gp_acq_ei_grad`` / ``BOBE.run(ei_lockstep=)``."""
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ei_grad_cases as EC  # noqa: E402
import ei_grad_restatement as ER  # noqa: E402

LD = np.longdouble
REF_BOUND = 1e-8          # fp64 restatement against the truth, relative to the largest component
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------- 1. the fp64 restatement and the truth
@pytest.mark.parametrize("combo", EC.COMBOS, ids=[EC.combo_id(c) for c in EC.COMBOS])
def test_fp64_restatement_holds_the_truth(combo):
    case, pair, log_ei = combo
    r = EC.reference(case, pair, log_ei)
    (tv, tg, tu), (fv, fg, _) = r["truth"], r["f64"]
    assert tv.dtype == LD and tg.dtype == LD and fv.dtype == np.float64 and fg.dtype == np.float64
    assert np.all(np.isfinite(fv)) and np.all(np.isfinite(fg))
    for name, f64, truth in (("val", fv, tv), ("grad", fg, tg)):
        err = EC.rel_err(f64, truth)
        print(f"[fp64 restatement] {EC.combo_id(combo):<58} {name:<5} {err:.3e}   max |truth| = {float(np.max(np.abs(truth))):.3e}"
              f"   u in [{float(np.min(tu)):.4g}, {float(np.max(tu)):.4g}]")
        assert err <= REF_BOUND, (EC.combo_id(combo), name, err)


def test_the_listing_leaves_out_what_it_says_and_the_ill_case_reaches_its_range():
    u = {(p, m): EC.reference(EC.ILL, p, m)["truth"][2] for p in EC.PAIRS for m in EC.MODES}
    for pair in EC.PAIRS:
        under = bool(np.all(u[pair, False] < -38.0))
        assert under == (not EC.listed(EC.ILL, pair, False)), pair
        if under:                                                            # EI and its gradient are 0 there, to the last row
            tv, tg, _ = EC.reference(EC.ILL, pair, False)["truth"]
            assert float(np.max(np.abs(tv))) < 1e-300 and float(np.max(np.abs(tg))) < 1e-300
    assert float(np.min(u["best_plus3_zeta", True])) <= -4500.0 and float(np.max(u["median", True])) >= 1000.0
    for kernel in ("rbf", "matern"):
        case = ("floor", kernel)
        floored = EC.posterior(case)[0][4]
        assert floored.tolist() == [True, True] + [False] * 7
        # a floored row in the lower branch of the LogEI gradient above and below log_ei_helper's -1e6, and far out on the right
        lows = [float(np.min(EC.reference(case, pair, True)["truth"][2][:2])) for pair in EC.PAIRS]
        assert -1e6 < lows[0] < -4500.0 and lows[1] < -1e6 and lows[2] > 1e5, (kernel, lows)
        assert all(EC.listed(case, pair, m) for pair in EC.PAIRS for m in EC.MODES)
    assert len(EC.COMBOS) == len(EC.CASES) * len(EC.PAIRS) * 2 - 2


# ---------------------------------------------------------------------------------------------- 2. the truth against itself
def test_truth_gradient_is_the_derivative_of_the_truth_value():
    """d val / dm = A and d val / dv = B / (2 sigma) by ``mpmath.diff`` of the value in (m, v): at least 30 of the 50 digits,
    on the first rows of the ill-conditioned case (u down to -4500, up to +1000) and of a well-conditioned one."""
    worst = 50.0
    for case in (EC.ILL, EC.CASES[0]):
        m, v = EC.posterior(case)[0][:2]
        for pair in EC.PAIRS:
            best_y, zeta = EC.best_and_zeta(case, pair)
            for log_ei in EC.MODES:
                if not EC.listed(case, pair, log_ei):
                    continue
                for c in range(min(3, len(m))):
                    assert v[c] > 1e-12
                    digits = ER.truth_self_check(m[c], v[c], best_y, zeta, log_ei)
                    worst = min(worst, digits)
                    assert digits >= 30.0, (EC.case_id(case), pair, log_ei, c, digits)
    print(f"truth self-check: at least {worst:.1f} digits")


# ------------------------------------------------------------------------------------------------- 3. mistakes made on purpose
def _breaks(case, pair, log_ei, **variant):
    f64 = EC.posterior(case)[1]
    best_y, zeta = EC.best_and_zeta(case, pair)
    _, tg, _ = EC.reference(case, pair, log_ei)["truth"]
    wrong = ER.value_and_grad_f64(*f64, best_y, zeta, log_ei, **variant)[1]
    return EC.rel_err(wrong, tg)


@pytest.mark.parametrize("case", [c for c in EC.CASES if not EC.is_floor(c)], ids=EC.case_id)
def test_a_doubled_dsigma_is_seen(case):
    """dsigma = dv / sigma instead of dv / (2 sigma): outside the bound in both modes of every posterior case, with the
    pair that has u of both signs (phi(u) is not negligible there).  The ill-conditioned case has no row with |u| < 38
    even then, so plain EI carries no phi(u) dsigma term at all and LogEI alone can show it."""
    for log_ei in ((True,) if case == EC.ILL else EC.MODES):
        err = _breaks(case, "median", log_ei, variant="dsigma_twice")
        print(f"{EC.case_id(case)} {'logei' if log_ei else 'ei'}: {err:.3e}")
        assert err > 1e3 * REF_BOUND


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_a_dsigma_on_the_floor_is_seen(kernel):
    """The two floored rows given a dsigma - from the dv of the two rows behind them, what a slip of the row index would
    hand them (their own dv arrives as 0): the row next to the best training point (u ~ -1e-8, phi(u) = 0.4, sigma = 1e-6)
    shows it in plain EI."""
    from scipy.special import ndtr
    case = ("floor", kernel)
    m, v, dm, dv, floored = EC.posterior(case)[1]
    assert floored.tolist() == [True, True] + [False] * 7 and np.all(dv[:2] == 0.0) and np.all(np.abs(dv[2:4]).max(axis=1) > 0.0)
    slipped = np.roll(dv, -2, axis=0)
    right = _breaks(case, "best", False)
    wrong = _breaks(case, "best", False, variant="floor_leak", dv_unfloored=slipped)
    print(f"floor_{kernel}: right {right:.3e}, floored rows with a dsigma {wrong:.3e}")
    assert right <= REF_BOUND and wrong > 1e3 * REF_BOUND
    # and what the GPU test states of those rows: grad = Phi(u) dm alone
    best_y, zeta = EC.best_and_zeta(case, "best")
    _, grad, u = ER.value_and_grad_f64(m, v, dm, dv, floored, best_y, zeta, False)
    assert np.array_equal(grad[:2], ndtr(u[:2])[:, None] * dm[:2])


# ------------------------------------------------------------------------------------------- 4. lock step on a stand-in GP
class _StandIn:
    """A surrogate with an analytic posterior in d = 3: m = 1 - 4 |x - c|^2, v = 0.02 + 0.3 |x - b|^2.  ``acq_ei_grad`` is the
    fp64 restatement over it; ``predict_grad`` / ``acq_ei`` serve the default path."""
    ndim = 3
    c = np.array([0.3, 0.6, 0.45])
    b = np.array([0.7, 0.2, 0.5])

    def __init__(self, grad_raises=False):
        g = np.random.default_rng(3)
        self.train_x = g.uniform(size=(12, 3))
        self.train_y = 1.0 - 4.0 * np.sum((self.train_x - self.c) ** 2, axis=1)
        self.calls = {"acq_ei_grad": 0, "predict_grad": 0, "acq_ei": 0}
        self.rows = []
        self.grad_raises = grad_raises

    def get_random_point(self, rng, nstd=None):
        return rng.uniform(size=self.ndim)

    def _posterior(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        m = 1.0 - 4.0 * np.sum((x - self.c) ** 2, axis=1)
        v = 0.02 + 0.3 * np.sum((x - self.b) ** 2, axis=1)
        return m, v, -8.0 * (x - self.c), 0.6 * (x - self.b)

    def predict_grad(self, x, mean_only=False):
        self.calls["predict_grad"] += 1
        return self._posterior(x)

    def acq_ei(self, x, best_y, zeta=0.0, log_ei=False):
        self.calls["acq_ei"] += 1
        m, v, dm, dv = self._posterior(x)
        return ER.value_and_grad_f64(m, v, dm, dv, np.zeros(len(m), bool), best_y, zeta, log_ei)[0]

    def acq_ei_grad(self, x, best_y, zeta=0.0, log_ei=False):
        if self.grad_raises:
            raise AssertionError("acq_ei_grad called with the option off")
        self.calls["acq_ei_grad"] += 1
        m, v, dm, dv = self._posterior(x)
        self.rows.append(len(m))
        val, grad, _ = ER.value_and_grad_f64(m, v, dm, dv, np.zeros(len(m), bool), best_y, zeta, log_ei)
        return val, grad


@pytest.mark.parametrize("name", ["EI", "LogEI"])
def test_lock_step_is_the_restarts_one_at_a_time(name, monkeypatch):
    from bobe_amd import acquisition as A
    kw = {"zeta": 0.01, "ei_lockstep": True}
    args = dict(maxiter=40, n_restarts=6, verbose=False)
    gp, r_lock = _StandIn(), np.random.default_rng(11)
    x_lock, v_lock = getattr(A, name)().get_next_point(gp, acq_kwargs=dict(kw), rng=r_lock, **args)
    assert gp.calls["predict_grad"] == 0 and gp.calls["acq_ei"] == 0
    # the probe of the first start alone, the other five screened together, then rounds of at most six
    assert gp.rows[0] == 1 and gp.rows[1] == 5 and max(gp.rows[2:]) <= 6 and gp.rows[2] == 6
    # the same call with optimize_scipy walking the restarts one after the other on the single-row objective
    real, seen = A.optimize_scipy, []

    def one_at_a_time(fun, *a, batch_value_and_grad=None, **k):
        seen.append(batch_value_and_grad is not None)
        return real(fun, *a, **k)
    monkeypatch.setattr(A, "optimize_scipy", one_at_a_time)
    gp1, r_one = _StandIn(), np.random.default_rng(11)
    x_one, v_one = getattr(A, name)().get_next_point(gp1, acq_kwargs=dict(kw), rng=r_one, **args)
    monkeypatch.undo()
    assert seen == [True] and set(gp1.rows) == {1}
    assert np.array_equal(np.asarray(x_lock), np.asarray(x_one)) and np.float64(v_lock).tobytes() == np.float64(v_one).tobytes()
    # the default path draws the same numbers from its generator, and never meets the new entry
    gp0, r_off = _StandIn(grad_raises=True), np.random.default_rng(11)
    x_off, v_off = getattr(A, name)().get_next_point(gp0, acq_kwargs={"zeta": 0.01}, rng=r_off, **args)
    assert r_off.bit_generator.state == r_lock.bit_generator.state == r_one.bit_generator.state
    assert gp0.calls["predict_grad"] > 0 and gp0.calls["acq_ei"] > 0 and np.all(np.isfinite(x_off)) and np.isfinite(v_off)
    x_f, v_f = getattr(A, name)().get_next_point(_StandIn(grad_raises=True), acq_kwargs={"zeta": 0.01, "ei_lockstep": False},
                                                 rng=np.random.default_rng(11), **args)
    assert np.array_equal(np.asarray(x_f), np.asarray(x_off)) and v_f == v_off


def test_lock_step_needs_the_scipy_optimiser():
    from bobe_amd import acquisition as A
    with pytest.raises(ValueError, match="ei_lockstep"):
        A.EI(optimizer="optax").get_next_point(_StandIn(), acq_kwargs={"ei_lockstep": True}, rng=np.random.default_rng(1),
                                               verbose=False)


# --------------------------------------------------------------------------------------------------------- 5. declarations
def test_the_entry_and_the_keyword_are_declared():
    from bobe_amd import _lib
    from bobe_amd.bo import BOBE
    from bobe_amd.gp import GP
    p = inspect.signature(BOBE.run).parameters["ei_lockstep"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    names = list(inspect.signature(BOBE.run).parameters)          # (earlier tests pin the last two keywords: it stands before them)
    assert names.index("logz_moments") < names.index("ei_lockstep") < names.index("zvar_polish")
    rows = [r for r in _lib.SIGNATURES if r[0] == "bobe_gp_acq_ei_grad"]
    assert len(rows) == 1 and len(rows[0][2]) == 8
    with open(os.path.join(ROOT, "include", "bobe_gp.h")) as fh:
        assert "int bobe_gp_acq_ei_grad(bobe_gp_t* gp, const double* Xq, int64_t C, double best_y, double zeta, int mode" \
            in fh.read()
    assert list(inspect.signature(GP.acq_ei_grad).parameters) == ["self", "x", "best_y", "zeta", "log_ei"]
