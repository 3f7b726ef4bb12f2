"""The expected evidence variance as a sweep criterion, without a GPU: the closed form of tests/zvar_restatement.py against
literal refits, its limits and invariances, the float64 restatement against the long-double truth on every case the device is
held to (tests/zvar_cases.py), what the cases can tell apart, and the wiring of ``acquisition.ZVar``.

Edge rules restated: |r_z| <= sqrt(b_z); a non-finite cross_z gives r_z = 0; a candidate whose s_c is not > 0 has every r_z =
0; T <= 0 gives zvar = +inf, which never wins an argmin over a finite score (all +inf: index 0)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zvar_cases as ZC  # noqa: E402
import zvar_restatement as R  # noqa: E402
from batch_select_restatement import masked_argmin  # noqa: E402

LD = np.longdouble


def small_case(n=14, m=9, d=2, c=6, seed=7, noise=1e-2):
    rng = np.random.default_rng(seed)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=n)
    return X, y, cand, Z, 0.7 * rng.normal(size=m), np.full(d, 0.5), 1.5, noise


def lognormal_var(ell, mu, cov):
    """Var of sum_z e^{l_z} e^{f_z}, f ~ N(mu, cov): sum_zz' A_z A_z' expm1(cov_zz'), A_z = e^{l_z + mu_z + cov_zz / 2}."""
    A = np.exp(ell + mu + np.diag(cov) / 2)
    return np.sum(np.outer(A, A) * np.expm1(cov))


def posterior_of_z(X, ys, Z, ls, kvar, noise, y_std):
    """(mu [M], cov [M x M]) of the noise-included process at Z in physical units, long double, by factorisation."""
    K = R.kernel("rbf", X, X, ls, kvar, LD) + LD(noise) * np.eye(X.shape[0], dtype=LD)
    L = R.cholesky_lower(K)
    kxz = R.kernel("rbf", X, Z, ls, kvar, LD)
    VZ = R.forward_sub(L, kxz)
    alpha = R.back_sub(L, R.forward_sub(L, np.asarray(ys, dtype=LD)))
    cov = R.kernel("rbf", Z, Z, ls, kvar, LD) + LD(noise) * np.eye(Z.shape[0], dtype=LD) - VZ.T @ VZ
    return LD(y_std) * (kxz.T @ alpha), LD(y_std) ** 2 * cov


def test_closed_form_against_gauss_hermite_refits():
    """E_xi[Var+ Z] = Var Z - E[Z]^2 T(c): the left side by an 80-node Gauss-Hermite average over the new observation of
    literal (N + 1)-point refits, N = 14, M = 9.  Asserted to 1e-8 relative (the closed form is exact; measured: see the
    printed figures), on candidates whose term is at least a hundredth of Var Z."""
    X, y, cand, Z, lw, ls, kvar, noise = small_case()
    ys, _, y_std = ZC.standardise(y)
    X, cand, Z, ys = (np.asarray(a, dtype=LD) for a in (X, cand, Z, ys))
    st = R.state("rbf", X, ys, cand, Z, ls, kvar, noise, LD)
    sc = R.zvar_scores(st, y_std, lw)
    mu, cov = posterior_of_z(X, ys, Z, ls, kvar, noise, y_std)
    var_z = lognormal_var(np.asarray(lw, dtype=LD), mu, cov)
    xi, wq = np.polynomial.hermite_e.hermegauss(80)
    wq = np.asarray(wq, dtype=LD) / np.sum(np.asarray(wq, dtype=LD))
    # the candidates' predictive mean and noise-included variance (standardised)
    K = R.kernel("rbf", X, X, ls, kvar, LD) + LD(noise) * np.eye(X.shape[0], dtype=LD)
    L = R.cholesky_lower(K)
    alpha = R.back_sub(L, R.forward_sub(L, ys))
    worst, sizeable = 0.0, 0
    for c in range(cand.shape[0]):
        kc = R.kernel("rbf", X, cand[c][None, :], ls, kvar, LD)[:, 0]
        mean_c, s_c = kc @ alpha, st["s"][c]
        lhs = LD(0)
        for node, w in zip(xi, wq):
            Xp = np.vstack([X, cand[c][None, :]])
            yp = np.append(ys, mean_c + np.sqrt(s_c) * LD(node))
            mu_p, cov_p = posterior_of_z(Xp, yp, Z, ls, kvar, noise, y_std)
            lhs += w * lognormal_var(np.asarray(lw, dtype=LD), mu_p, cov_p)
        gain = np.exp(2 * sc["log_ez"] - sc["zvar"][c])
        rhs = var_z - gain
        rel = float(abs(lhs - rhs) / abs(rhs))
        print("candidate %d: E[Var+] %.6e, closed form %.6e, relative %.2e, gain / Var Z %.3f" %
              (c, float(lhs), float(rhs), rel, float(gain / var_z)))
        worst = max(worst, rel)
        sizeable += int(gain > var_z / 100)
        assert 0 < gain < var_z
    assert worst <= 1e-8, worst
    assert sizeable >= 3, sizeable                     # the identity is not checked on terms too small to matter


def test_small_scale_limit_is_the_squared_weighted_sum():
    """T -> (sum_z omega_z r_z)^2 as y_std -> 0: at y_std = 1e-4 r is O(1e-4) and the two agree to O(r^2)."""
    X, y, cand, Z, lw, ls, kvar, noise = small_case()
    ys, _, _ = ZC.standardise(y)
    st = R.state("rbf", X, ys, cand, Z, ls, kvar, noise, LD)
    y_std = 1e-4
    sc = R.zvar_scores(st, y_std, lw)
    lam, b, _ = R.z_weights(st, y_std, lw)
    lin = (R.r_terms(st, y_std, b) @ np.exp(lam)) ** 2
    rel = np.abs(np.exp(-sc["zvar"]) / lin - 1)
    print("T against its linearisation at y_std = 1e-4:", float(np.max(rel)))
    assert np.all(rel <= 1e-6)
    # ... and at y_std = 5 (the difference grows as r^2) they differ: the criterion is not its linearisation in disguise
    sc1 = R.zvar_scores(st, 5.0, lw)
    lam1, b1, _ = R.z_weights(st, 5.0, lw)
    lin1 = (R.r_terms(st, 5.0, b1) @ np.exp(lam1)) ** 2
    assert np.max(np.abs(np.exp(-sc1["zvar"]) / lin1 - 1)) > 1e-3


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_one_integration_point(dtype):
    """M = 1: omega = 1 and T = expm1(r^2)."""
    X, y, cand, Z, lw, ls, kvar, noise = small_case(m=1)
    ys, _, y_std = ZC.standardise(y)
    st = R.state("rbf", X, ys, cand, Z, ls, kvar, noise, dtype)
    sc = R.zvar_scores(st, y_std, lw)
    _, b, _ = R.z_weights(st, y_std, lw)
    r = R.r_terms(st, y_std, b)[:, 0]
    want = -np.log(np.expm1(r * r))
    assert np.max(np.abs(sc["zvar"] - want)) <= 1e-12 * (1 + np.max(np.abs(want)))


def test_invariances():
    """A constant added to the log-weights moves log_ez by it and nothing else; y_mean does not enter at all."""
    X, y, cand, Z, lw, ls, kvar, noise = small_case()
    ys, _, y_std = ZC.standardise(y)
    st = R.state("rbf", X, ys, cand, Z, ls, kvar, noise, np.float64)
    a, b = R.zvar_scores(st, y_std, lw), R.zvar_scores(st, y_std, lw + 3.25)
    assert np.max(np.abs(a["zvar"] - b["zvar"])) <= 1e-12 and abs(b["log_ez"] - a["log_ez"] - 3.25) <= 1e-12
    ys2, _, y_std2 = ZC.standardise(y + 17.5)
    st2 = R.state("rbf", X, ys2, cand, Z, ls, kvar, noise, np.float64)
    c = R.zvar_scores(st2, y_std2, lw)
    assert np.max(np.abs(a["zvar"] - c["zvar"])) <= 1e-9 and abs(c["log_ez"] - a["log_ez"]) <= 1e-9
    # posterior-draw weights are the explicit l_z = -mu_z
    d0, d1 = R.zvar_scores(st, y_std, None), R.zvar_scores(st, y_std, -y_std * st["mu"])
    assert np.array_equal(d0["zvar"], d1["zvar"])


@pytest.mark.parametrize("case", ZC.SWEEP_CASES, ids=ZC.case_id)
def test_float64_restatement_against_the_long_double_truth(case):
    """Within 1e-7 (1 + |truth|) on every candidate of every case the device is held to, no infinities, and the two best
    scores more than 1e-6 apart (the precondition of asserting the device's argmin)."""
    ref = ZC.sweep_reference(case)
    truth = ref["truth"]
    assert np.all(np.isfinite(truth)) and np.all(np.isfinite(ref["f64"]))
    err = float(np.max(np.abs(ref["f64"].astype(LD) - truth) / (1 + np.abs(truth))))
    g = R.W.two_best_gap(truth) if truth.shape[0] > 1 else np.inf
    print("%s: float64 against long double %.3e, gap of the two best %.3e" % (ZC.case_id(case), err, g))
    assert err <= 1e-7, err
    assert g > ZC.GAP_MIN, g
    assert masked_argmin(ref["f64"]) == masked_argmin(truth)
    assert abs(ref["log_ez_f64"] - float(ref["log_ez"])) <= 1e-7 * (1 + abs(float(ref["log_ez"])))


def test_batch_reference_is_usable():
    (p64, s64, g64), (pld, sld, gld) = ZC.batch_reference()
    assert p64.tolist() == pld.tolist() and len(set(pld.tolist())) == len(pld)
    assert np.all(gld > ZC.GAP_MIN), gld
    assert np.max(np.abs(s64.astype(LD) - sld) / (1 + np.abs(sld))) <= 1e-7


# ---- what the cases can tell apart
def variant_scores(st, y_std, lw, variant):
    """-log T of every candidate, literally, in long double (no scaling: for moderate y_std only), with one mistake."""
    lam, b, _ = R.z_weights(st, y_std, lw)
    if variant == "no_half_b":
        mu = LD(y_std) * st["mu"]
        g = (-mu if lw is None else np.asarray(lw, dtype=LD)) + mu
        lam = g - R.lse(g)
    om = np.exp(lam)
    r = R.r_terms(st, y_std, b, capped=variant != "uncapped")
    if variant == "abs_r":
        r = np.abs(r)
    x = r[:, :, None] * r[:, None, :]
    ww = om[None, :, None] * om[None, None, :]
    term = ww * (np.exp(x) if variant == "exp" else np.expm1(x))
    eye = np.eye(len(om), dtype=bool)[None]
    if variant == "single_off_diagonal":
        T = np.sum(np.where(eye, term, term / 2), axis=(1, 2))
    elif variant == "no_diagonal":
        T = np.sum(np.where(eye, 0, term), axis=(1, 2))
    elif variant == "linearised":
        T = (r @ om) ** 2
    else:
        T = np.sum(term, axis=(1, 2))
    return -np.log(T)


VARIANTS = ("no_half_b", "abs_r", "single_off_diagonal", "no_diagonal", "exp", "linearised")


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_cases_tell_a_mistake_from_the_right_answer(variant):
    """On the y_std = 1 cases (where the literal sum needs no scaling) each mistaken variant misses the device's rule by a
    factor of at least a hundred on some candidate of at least one case - and the literal sum itself meets it."""
    told = []
    for case in [c for c in ZC.SWEEP_CASES if c[3] == 1.0 and c[0] != "m1"]:
        shape, kernel, weighted, y_std = case
        _, sld, _, std = ZC.states(shape, kernel, y_std)
        lw = ZC.case_data(shape, y_std)[4] if weighted else None
        truth = ZC.sweep_reference(case)["truth"]
        right = variant_scores(sld, std, lw, None)
        assert np.max(np.abs(right - truth) / (1 + np.abs(truth))) <= 1e-12
        with np.errstate(invalid="ignore"):            # (a variant whose T turns negative scores NaN: told)
            miss = float(np.max(np.abs(variant_scores(sld, std, lw, variant) - truth) / (1 + np.abs(truth))))
        told.append(not miss <= 1e-5)
        print("%s on %s: %.3e" % (variant, ZC.case_id(case), miss))
    assert any(told)
    # (b_z / 2 and the curvature of expm1 matter little where every r is small - M <= 9 next to 64 training points; the
    # structural mistakes show on every case)
    if variant not in ("no_half_b", "linearised"):
        assert all(told)


def test_the_cap_on_r_is_told_on_a_state_where_it_binds():
    """In exact arithmetic cross_z^2 < s_c b_z (Cauchy-Schwarz on the posterior covariance), so on a regular state the cap
    never binds: it is there for states where rounding left base_z at its floor.  Such a state is made here by hand - base_z
    of one point set below the floor - and told from the uncapped sum; on the regular cases the two agree exactly."""
    case = ("below_the_unroll", "rbf", True, 1.0)
    _, sld, _, std = ZC.states(case[0], case[1], case[3])
    lw = ZC.case_data(case[0], case[3])[4]
    assert np.array_equal(variant_scores(sld, std, lw, None), variant_scores(sld, std, lw, "uncapped"))
    st = dict(sld)
    st["base"] = sld["base"].copy()
    st["base"][2] = LD(-3e-17)
    capped, free = variant_scores(st, std, lw, None), variant_scores(st, std, lw, "uncapped")
    _, b, _ = R.z_weights(st, std, lw)
    assert float(b[2]) == 1e-12 * std ** 2
    assert np.max(np.abs(R.r_terms(st, std, b)[:, 2])) <= np.sqrt(b[2])
    assert np.max(np.abs(capped - free)) > 1e-5
    assert np.max(np.abs(R.zvar_scores(st, std, lw)["zvar"] - capped) / (1 + np.abs(capped))) <= 1e-12


def test_edge_rules_of_the_restatement():
    case = ("below_the_unroll", "rbf", True, 1.0)
    s64, _, _, std = ZC.states(case[0], case[1], case[3])
    lw = ZC.case_data(case[0], case[3])[4]
    st = {k: np.array(v) for k, v in s64.items()}
    st["s"][0] = 0.0                                   # s_c not > 0: every r_z = 0, T = 0, +inf
    st["s"][1] = np.nan
    st["kcz"][2, :] = np.inf                           # non-finite cross: r_z = 0
    sc = R.zvar_scores(st, std, lw)["zvar"]
    assert np.all(np.isposinf(sc[:3])) and np.all(np.isfinite(sc[3:]))
    assert masked_argmin(sc) == int(np.argmin(np.where(np.isfinite(sc), sc, np.inf))) >= 3
    assert masked_argmin(np.full(5, np.inf)) == 0      # all +inf: index 0


# ---- wiring
def test_zvar_wiring():
    from bobe_amd import acquisition as A
    from bobe_amd import bo
    assert set(bo._ACQ) == {"wipv", "wipstd", "ei", "logei", "imiqr", "eiv", "ts"}
    assert bo._ACQ_MORE == {"zvar": A.ZVar} and bo._acq_class("ZVar") is A.ZVar and bo._acq_class("wipstd") is A.WIPStd
    assert bo._acq_class("nope") is None
    acq = A.ZVar()
    assert issubclass(A.ZVar, A.WeightedIntegratedPosteriorBase) and acq._key == "zvar" and acq._weighted(None)
    assert not A.WIPStd()._weighted(None) and A.EIV()._weighted(None)
    with pytest.raises(ValueError):
        acq.get_next_point(None, acq_kwargs={"weighted_polish": 2})
    from bobe_amd.gp import GP
    assert GP.CRITERIA == ("wipv", "wipstd", "imiqr", "eiv")
    from bobe_amd import _lib
    names = [s[0] for s in _lib.SIGNATURES]
    assert "bobe_gp_wip_sweep_zvar" in names and "bobe_gp_wip_select_batch_zvar" in names
    import inspect
    assert list(inspect.signature(bo.BOBE.run).parameters)[-1] == "wip_batch_mode"
