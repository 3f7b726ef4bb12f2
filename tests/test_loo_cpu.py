"""Leave-one-out cross-validation without a GPU: the restatements the GPU tests measure against (tests/loo_restatement.py)
agree with each other - the closed form with N literal refits, torch's autograd gradient with the hand formula in extended
precision - and the feature's interface exists: the two C symbols are declared and exported, the Python methods and the
``fit_objective`` keyword are there.
"""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import loo_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(kind, n=60, d=3, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2] + 0.05 * rng.standard_normal(n)
    y = (y - y.mean()) / y.std()
    ls = np.array([0.5, 0.8, 0.65])
    return kind, X, y, ls, 1.4, 1e-6


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_closed_form_is_the_literal_refits(kind):
    """The extended-precision closed form against N refits on N-1 points.  The refits are fp64 solves of matrices with
    cond(K) ~ 1e7 (RBF, noise 1e-6) - their own error bounds the agreement, not the closed form's."""
    c = _case(kind)
    bm, bv, bl = R.loo_brute(*c)
    t = R.loo_closed_xp(*c)
    assert np.max(np.abs(bm - t["mean"])) <= 1e-7 * np.max(np.abs(bm))
    assert np.max(np.abs(bv - t["var"]) / bv) <= 1e-6
    assert abs(np.sum(bl) - t["loo"]) <= 1e-7 * abs(np.sum(bl))
    for f in (R.loo_closed, R.loo_closed_inv):
        m, v, l, s = f(*c)
        assert np.max(np.abs(m - t["mean"])) <= 1e-7 and np.max(np.abs(v - t["var"]) / v) <= 1e-6
        assert abs(s - float(t["loo"])) <= 1e-7 * abs(s)


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_autograd_gradient_is_the_hand_formula(kind):
    """dL_LOO/dtheta = sum M dK/dtheta with M = -A diag(c) A - (w alpha^T + alpha w^T)/2 (extended precision) against
    torch-fp64 autograd through the closed form, which knows nothing of that formula."""
    kind, X, y, ls, kvar, noise = _case(kind)
    t = R.loo_closed_xp(kind, X, y, ls, kvar, noise, want_grad=True)
    val, g = R.loo_objective_torch(kind, X, y, np.log(np.append(ls, kvar)), noise)
    assert abs(val - float(t["loo"])) <= 1e-7 * abs(val)
    gt = t["grad"].astype(np.float64)
    assert np.max(np.abs(g - gt)) <= 1e-5 * np.max(np.abs(gt)), (g, gt)


def test_value_moves_as_the_gradient_says():
    """Central differences of the extended-precision value (step 1e-5 in log theta) against the hand formula."""
    kind, X, y, ls, kvar, noise = _case("matern")
    th = np.log(np.append(ls, kvar))
    g = R.loo_closed_xp(kind, X, y, ls, kvar, noise, want_grad=True)["grad"]
    h = 1e-5
    for j in range(th.size):
        e = np.zeros_like(th)
        e[j] = h
        p, m = np.exp(th + e), np.exp(th - e)
        fd = (R.loo_closed_xp(kind, X, y, p[:-1], p[-1], noise)["loo"] - R.loo_closed_xp(kind, X, y, m[:-1], m[-1], noise)["loo"]) \
            / (2 * h)
        assert abs(float(fd - g[j])) <= 1e-5 * float(np.max(np.abs(g))), (j, fd, g[j])


# ---- the interface (these fail without the feature) -----------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from bobe_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bobe_gp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int bobe_gp_loo(bobe_gp_t* gp, double* mean, double* var, double* lpd, double* sum_lpd);" in flat
    assert ("int bobe_gp_loo_objective(bobe_gp_t* gp, const double* lengthscales, double kernel_variance, double* loo, "
            "double* grad);") in flat
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {"bobe_gp_loo", "bobe_gp_loo_objective"} <= bound
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"bobe_gp_loo", "bobe_gp_loo_objective"} <= exported


def test_python_interface_exists():
    from bobe_amd import GP, BOBE
    from bobe_amd.clf_gp import GPwithClassifier
    for name in ("loo", "loo_data", "neg_loo_value_and_grad"):
        assert callable(getattr(GP, name)), name
    assert isinstance(GP.fit_objective, property)
    for cls in (GP, GPwithClassifier):
        p = inspect.signature(cls.__init__).parameters["fit_objective"]
        assert p.default == "mll"
    p = inspect.signature(BOBE.run).parameters["loo_diagnostics"]
    assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert list(inspect.signature(GP.loo_data).parameters)[1:] == ["lengthscales", "kernel_variance", "want_grad"]
    assert list(inspect.signature(GP.neg_loo_value_and_grad).parameters)[1:] == ["log_params", "want_grad"]
