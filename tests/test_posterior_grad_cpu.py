"""tests/posterior_grad_restatement.py held to itself, without a GPU: the long-double gradients against central differences of
the long-double values, the equal-weight score gradient of tests/weighted_grad_restatement.py against the chain rule through
this module's pieces, the fp64 restatement against the truth on every case of tests/test_gpu_posterior_grad.py (so that the
``4 x ref`` term of the rule cannot swallow a real error), the floor design, and the leapfrog against single evaluations."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import posterior_grad_cases as PC  # noqa: E402
import posterior_grad_restatement as PG  # noqa: E402
import weighted_grad_restatement as R  # noqa: E402
from test_gpu_weighted_criteria import case_data, standardise  # noqa: E402

LD = np.longdouble
REF_BOUND = 1e-8          # fp64 restatement against the truth, relative to the largest component


# -------------------------------------------------------------------------------------------------- 1. central differences
@pytest.mark.parametrize("kernel,d,n", [("matern", 5, 300), ("rbf", 12, 160), ("matern", 17, 160)])
def test_truth_gradients_are_central_differences_of_the_truth_values(kernel, d, n):
    """Step 1e-7 in long double: the truncation term h^2 / 6 f''' is ~1e-14 / ls^2 of the gradient, the rounding term
    2^-64 |f| / h ~ 5e-13 |f| (more where the variance cancels: var ~ 1e-3 kvar here); both far inside 1e-8 max |gradient|."""
    X, y, Q, _, _ = case_data(1000 + 10 * d + n, n, d, 4, 1)
    ys, _, _ = standardise(y)
    ls = 0.4 * (1.0 + 0.05 * np.arange(d))
    Q = 0.1 + 0.8 * Q
    h = LD(1e-7)
    pts = [np.asarray(Q, dtype=LD)]
    for j in range(d):
        for sgn in (1, -1):
            q = np.asarray(Q, dtype=LD).copy()
            q[:, j] += sgn * h
            pts.append(q)
    mean, var, dmean, dvar, floored = PG.posterior_and_grad(kernel, X, ys, np.concatenate(pts), ls, 2.0, 1e-6, LD)
    assert mean.dtype == LD and dvar.dtype == LD and not floored.any()
    C = len(Q)
    for name, val, grad in (("mean", mean, dmean[:C]), ("var", var, dvar[:C])):
        cd = np.stack([(val[(1 + 2 * j) * C:(2 + 2 * j) * C] - val[(2 + 2 * j) * C:(3 + 2 * j) * C]) / (2 * h) for j in range(d)],
                      axis=1)
        scale = float(np.max(np.abs(grad)))
        err = float(np.max(np.abs(cd - grad)))
        print(f"{kernel} d={d} N={n} d{name}: max |central difference - analytic| = {err:.3e}, max |gradient| = {scale:.3e}")
        assert err <= 1e-8 * scale


# ------------------------------------------------------------------------------------------------ 2. equal-weight identity
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_equal_weight_score_gradient_is_the_chain_rule_through_this_module(kernel):
    """One integration point z, omega = 1: wipv(x) = y_std^2 (base_z - cross^2 / s) with

        s = var(x),  ds = dvar(x)                                       posterior_and_grad at x
        base_z = var(z)                                                 posterior_and_grad at z
        cross = k(x, z) - m(x),  dcross = dk(x, z) / dx - dm(x)         posterior_and_grad at x with targets k(X, z)

    and weighted_grad_restatement states dk / dx on its own.  Both in fp64, to 1e-12 of the largest component; two fp64 routes
    to these pieces differ by ~eps cond(K), so the state is a well-conditioned one (noise 1e-2: cond(K) < N kvar / noise ~ 1e4,
    in practice far less).  The ill-conditioned families are held to the truth below instead."""
    n, d, noise, kvar = 60, 5, 1e-2, 2.0
    X, y, cand, Z, _ = case_data(1000 + 10 * d + n, n, d, 6, 1)
    ys, _, y_std = standardise(y)
    ls = 0.4 * (1.0 + 0.05 * np.arange(d))
    cand = 0.1 + 0.8 * cand
    st = R.State(kernel, X, ys, Z, ls, kvar, noise, y_std, None, np.float64)
    r = R.value_and_grad(st, cand)
    assert not r["floored"].any()
    kz = R._kernel(kernel, X, Z, ls, kvar, np.float64)[:, 0]
    _, s, _, ds, _ = PG.posterior_and_grad(kernel, X, ys, cand, ls, kvar, noise)
    base = PG.posterior_and_grad(kernel, X, ys, Z, ls, kvar, noise)[1][0]
    m, _, dm, _, _ = PG.posterior_and_grad(kernel, X, kz, cand, ls, kvar, noise)
    cross = R._kernel(kernel, cand, Z, ls, kvar, np.float64)[:, 0] - m
    dcross = np.stack([PG.dk_dq(kernel, cand[c], Z, ls, kvar, np.float64)[0] for c in range(len(cand))]) - dm
    wipv = y_std ** 2 * (base - cross ** 2 / s)
    dwipv = y_std ** 2 * ((-2.0 * cross / s)[:, None] * dcross + (cross ** 2 / s ** 2)[:, None] * ds)
    ev = float(np.max(np.abs(wipv - r["wipv"])) / np.max(np.abs(r["wipv"])))
    eg = float(np.max(np.abs(dwipv - r["dwipv"])) / np.max(np.abs(r["dwipv"])))
    print(f"{kernel}: wipv {ev:.3e}, dwipv {eg:.3e}")
    assert ev <= 1e-12 and eg <= 1e-12


# ------------------------------------------------------------------------------------- 3. the fp64 restatement and the truth
def _check(label, pairs):
    for name, f64, truth in pairs:
        err = PC.rel_err(f64, truth)
        print(f"[fp64 restatement] {label:<34} {name:<8} {err:.3e}   max |truth| = {float(np.max(np.abs(truth))):.3e}")
        assert truth.dtype == LD and np.asarray(f64).dtype == np.float64
        assert err <= REF_BOUND, (label, name, err)


@pytest.mark.parametrize("case", PC.PREDICT_CASES, ids=[PC.predict_id(c) for c in PC.PREDICT_CASES])
def test_fp64_restatement_of_predict_grad_cases(case):
    truth, f64 = PC.predict_reference(case)
    assert not truth[4].any() and not f64[4].any()
    _check(PC.predict_id(case), [(k, f64[i], truth[i]) for i, k in enumerate(("mean", "var", "dmean", "dvar"))])


@pytest.mark.parametrize("case", PC.WIP_CASES, ids=[PC.wip_id(c) for c in PC.WIP_CASES])
def test_fp64_restatement_of_wip_grad_cases(case):
    truth, f64 = PC.wip_reference(case)
    _check(PC.wip_id(case), [(k, f64[k], truth[k]) for k in PC.WIP_KEYS])
    _check(PC.wip_id(case) + "_first9", [(k, f64[k][:9], truth[k][:9]) for k in PC.WIP_KEYS])


@pytest.mark.parametrize("L", PC.HMC_STEPS)
@pytest.mark.parametrize("case", PC.HMC_CASES, ids=[f"{k}_d{d}_N{n}" for k, d, n in PC.HMC_CASES])
def test_fp64_restatement_of_leapfrog_cases(case, L):
    truth, f64 = PC.hmc_reference(case, L)
    assert np.max(np.abs(PC.hmc_data(case)[2])) <= 3.0
    assert np.all((truth["X"] > 1e-9) & (truth["X"] < 1.0 - 1e-9))           # the kernel's 1e-12 clip stays idle
    _check(PC.hmc_id(case, L), [(k, f64[k], truth[k]) for k in PC.HMC_KEYS])


# ----------------------------------------------------------------------------------------------------------- 4. the floor
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_floor_design_floors_exactly_its_two_rows(kernel):
    truth, f64 = PC.floor_reference(kernel)
    for label, (mean, var, dmean, dvar, floored) in (("truth", truth), ("fp64", f64)):
        print(f"{kernel} {label}: floored rows {np.flatnonzero(floored).tolist()}, min var elsewhere {float(np.min(var[2:])):.4f}")
        assert floored.tolist() == [True, True] + [False] * 7
        assert np.all(var[:2] == 1e-12) and np.all(dvar[:2] == 0.0) and np.all(var[2:] > 0.5)
        assert np.all(np.isfinite(dmean.astype(np.float64))) and np.any(dvar[2:] != 0.0)
    _check(f"floor_{kernel}", [("mean", f64[0], truth[0]), ("dmean", f64[2], truth[2]), ("var", f64[1][2:], truth[1][2:]),
                               ("dvar", f64[3][2:], truth[3][2:])])


# --------------------------------------------------------------------------------------------------------- 5. the leapfrog
def _leapfrog_args(case, dtype):
    kernel, d, _ = case
    X, y, U, Pm, im = PC.hmc_data(case)
    ys, y_mean, y_std = standardise(y)
    return kernel, X, ys, np.full(d, PC.ell_of(d)), PC.KVAR, PC.NOISE, y_mean, y_std, U, Pm, im


@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["fp64", "long_double"])
def test_one_leapfrog_step_is_one_evaluation_composed_by_hand(dtype):
    case = PC.HMC_CASES[1]
    args = _leapfrog_args(case, dtype)
    kernel, X, ys, ls, kvar, noise, y_mean, y_std, U, Pm, im = args
    D = dtype
    eps, temp = D(PC.HMC_EPS), D(PC.HMC_TEMP)
    u1 = np.asarray(U, dtype=D) + eps * np.asarray(im, dtype=D) * np.asarray(Pm, dtype=D)
    x1 = D(1.0) / (D(1.0) + np.exp(-u1))
    m, _, dm, _, _ = PG.posterior_and_grad(kernel, X, ys, x1, ls, kvar, noise, D)
    mean = m * D(y_std) + D(y_mean)
    logp = mean / temp + np.sum(np.log(x1) + np.log1p(-x1), axis=1)
    g = dm * D(y_std) / temp * x1 * (D(1.0) - x1) + (D(1.0) - D(2.0) * x1)
    hand = (u1, np.asarray(Pm, dtype=D) + D(0.5) * eps * g, logp, g, mean, x1)
    got = PG.leapfrog(*args, PC.HMC_EPS, 1, PC.HMC_TEMP, D)
    tol = 1e-13 if D is np.float64 else 1e-16        # alpha by cho_solve in both (fp64); one solve with two right-hand sides
    for k, a, b in zip(PC.HMC_KEYS, got, hand):      # against one with a single one (long double): rounding of the last place
        assert a.dtype == D and a.shape == b.shape
        assert PC.rel_err(a, b) <= tol, (k, PC.rel_err(a, b))


def test_leapfrog_round_trip_returns_to_the_start():
    """L = 9 forwards, then the same with -eps from the end state: the integrator is its own inverse.  The momentum handed in
    is the half-kicked one, so the way back starts from Pm' and arrives at the Pm handed in.

    The return is exact up to the rounding of the 19 gradient evaluations each way, ~2^-64 sum_n |alpha_n k(x, X_n)| apiece.
    That sum (printed) is 2 - 30 on the two well-conditioned families, which are held to 1e-15 (measured: 1e-19); on the
    ill-conditioned rbf d = 3 family the terms cancel from ~1e7 down to a mean of order 1 and the same recurrence returns to 4e-15
    (printed, not asserted: the figure is the conditioning of that state, not a property of the integrator)."""
    for case in PC.HMC_CASES[1:] + PC.HMC_CASES[:1]:
        args = _leapfrog_args(case, LD)
        U, Pm = np.asarray(args[8], dtype=LD), np.asarray(args[9], dtype=LD)
        # a whole trajectory: half kick, 9 steps (the last kick a half one) - then reversed
        g0 = PG.leapfrog(*args[:8], U, 0 * Pm, args[10], 0.0, 1, PC.HMC_TEMP, LD)[3]
        eps = LD(PC.HMC_EPS)
        u1, p1 = PG.leapfrog(*args[:8], U, Pm + LD(0.5) * eps * g0, args[10], eps, 9, PC.HMC_TEMP, LD)[:2]
        g1 = PG.leapfrog(*args[:8], u1, 0 * p1, args[10], 0.0, 1, PC.HMC_TEMP, LD)[3]
        u2, p2 = PG.leapfrog(*args[:8], u1, p1 - LD(0.5) * eps * g1, args[10], -eps, 9, PC.HMC_TEMP, LD)[:2]
        eu, ep = float(np.max(np.abs(u2 - U))), float(np.max(np.abs(p2 - Pm)))
        alpha = PG.solve_alpha(*args[:6], LD)
        x0 = LD(1.0) / (LD(1.0) + np.exp(-U))
        mass = float(np.max(R._kernel(args[0], x0, args[1], args[3], args[4], LD) @ np.abs(alpha)))
        print(f"{PC.hmc_id(case, 9)}: |u - u0| = {eu:.3e}, |p - p0| = {ep:.3e}, sum |alpha k| = {mass:.3e}")
        if case != PC.HMC_CASES[0]:
            assert mass < 1e2 and eu <= 1e-15 and ep <= 1e-15
