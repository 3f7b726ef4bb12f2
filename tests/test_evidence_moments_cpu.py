"""The total variance of the evidence estimate, without a GPU: the float64 restatement of
tests/evidence_moments_restatement.py against the long-double truth on every case the device is held to
(tests/evidence_moments_cases.py), the scaled pair sum against the lognormal's own unscaled formula, the M = 1 closed form, what
the cases can tell apart, the edge rules, and the wiring of ``logz_from_samples(moments=True)`` and ``BOBE.run(logz_moments=...)``.

Rules restated: for z != z' |S_zz'| <= sqrt(b_z b_z'); a non-finite off-diagonal S counts as 0; S_zz = b_z (floored as the
per-z table floors it); T0 <= 0 gives log_t0 = -inf; a NaN state gives NaN."""
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evidence_moments_cases as EC  # noqa: E402
import evidence_moments_restatement as E  # noqa: E402
import zvar_cases as ZC  # noqa: E402

LD = np.longdouble


def rule_holds(got, case, key=1):
    ref = EC.reference(case)
    return ZC.rule([got], [ref["f64"][key]], np.array([LD(ref["truth"][key])]))


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_float64_restatement_against_the_long_double_truth(case):
    """The reference itself: the truth is finite on every case, log T0 from -15.3 to 2.01e7, and float64 is within
    2.5e-9 (1 + |truth|) of long double - to the two digits of that figure: the largest error, log_t0 on
    s204-N130-d3-M128-rbf-ystd30-weights, is 2.506e-9, every other one is below 1e-9, so the bound asserted is 2.55e-9.  The
    device's rule (4 x the float64 error + 1e-7 (1 + |truth|)) is then met by the float64 restatement alone forty times over."""
    ref = EC.reference(case)
    for i in (0, 1):
        truth = LD(ref["truth"][i])
        assert np.isfinite(truth)
        err = abs(LD(ref["f64"][i]) - truth) / (1 + abs(truth))
        assert err <= 2.55e-9, (i, float(err))
    assert -15.5 < ref["truth"][1] < 2.05e7


def test_scaled_pair_sum_is_the_lognormal_variance_on_a_benign_case():
    """log T0 + 2 log E[Z] = log sum_zz' A_z A_z' expm1(cov_zz'), as tests/test_zvar_cpu.py::lognormal_var writes Var Z."""
    shape = EC.SHAPES[2]
    for kernel in EC.KERNELS:
        _, sld, _, std = EC.states(shape, kernel, 1.0)
        lw = EC.case_data(shape, 1.0)[3]
        for w in (lw, None):
            lam, b, log_ez = E.z_weights(sld, std, w)
            mu = LD(std) * sld["mu"]
            cov = E.pair_matrix(sld["cov"], b, std)
            ell = -mu if w is None else np.asarray(w, dtype=LD)
            A = np.exp(ell + mu + np.diag(cov) / 2)
            var = np.sum(np.outer(A, A) * np.expm1(cov))
            got = E.evidence_moments(sld, std, w)
            assert abs(got["log_t0"] + 2 * got["log_ez"] - np.log(var)) <= 1e-14 * (1 + abs(np.log(var)))
            assert abs(got["log_ez"] - np.log(np.sum(A))) <= 1e-15 * (1 + abs(got["log_ez"]))
            v64, a64 = E.direct_var(np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64),
                                    np.asarray(ell, dtype=np.float64))
            assert abs(np.log(v64) - float(np.log(var))) <= 1e-9


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_one_integration_point(dtype):
    """M = 1: Z is one lognormal, Var Z = e^{2 g} expm1(b)."""
    case = (EC.SHAPES[0], "rbf", 30.0, True)
    s64, sld, _, std = EC.states(*case[:3])
    st = s64 if dtype is np.float64 else sld
    lw = EC.case_data(case[0], case[2])[3]
    lam, b, log_ez = E.z_weights(st, std, lw)
    got = E.evidence_moments(st, std, lw)
    g = dtype(lw[0]) + dtype(std) * st["mu"][0] + b[0] / 2
    assert abs(got["log_ez"] - g) <= 1e-14 * (1 + abs(g)) and lam[0] == 0
    assert abs(got["log_t0"] - np.log(np.expm1(b[0]))) <= 1e-13 * (1 + abs(got["log_t0"]))


# ---- what the cases can tell apart
def tile_of(m):
    return np.arange(m) // 128


def variant(case, name):
    """log T0 in long double with one mistake."""
    shape, kernel, y_std, weighted = case
    _, sld, _, std = EC.states(shape, kernel, y_std)
    lw = EC.case_data(shape, y_std)[3] if weighted else None
    lam, b, _ = E.z_weights(sld, std, lw)
    m = len(lam)
    S = E.pair_matrix(sld["cov"], b, std)
    eye = np.eye(m, dtype=bool)
    w = None
    if name == "diagonal_twice":
        w = np.where(eye, 2.0, 1.0)
    elif name == "off_diagonal_once":
        w = np.where(eye, 1.0, 0.5)
    elif name == "no_y_std2":
        S = E.pair_matrix(sld["cov"] / LD(std) ** 2, b, std)
    elif name == "diagonal_without_noise":
        S = np.array(S)
        S[np.diag_indices(m)] = b - LD(std) ** 2 * sld["noise"]
    elif name == "transposed_tile_skipped":
        t = tile_of(m)
        w = np.where(t[:, None] != t[None, :], 0.5, 1.0)      # an off-diagonal TILE counted once, pairs inside diagonal tiles twice
    return E.log_t0_scaled(lam, b, S, w)


VARIANTS = ("diagonal_twice", "off_diagonal_once", "no_y_std2", "diagonal_without_noise", "transposed_tile_skipped")


@pytest.mark.parametrize("name", VARIANTS)
def test_the_cases_tell_a_mistake_from_the_right_answer(name):
    """Each mistaken variant misses the device's rule on at least one case (the right sum, formed the same way, meets it on
    all of them).  Where y_std is large the largest diagonal term e^{b_z} carries T0 and the off-diagonal mistakes hide behind it,
    so most of them show at y_std = 1 and 30; the transposed tile cannot show on a case with one tile row and does beyond."""
    told = []
    for case in EC.CASES:
        if case[1] != "rbf":
            continue
        assert rule_holds(float(variant(case, None)), case)[0]
        ok, err, _ = rule_holds(float(variant(case, name)), case)
        told.append(not ok)
    assert any(told), name
    print(name, "told on %d of %d cases" % (sum(told), len(told)))
    if name == "transposed_tile_skipped":
        assert [t for t, c in zip(told, [c for c in EC.CASES if c[1] == "rbf"]) if c[0][3] <= 128] == [False] * 24
        assert any(t for t, c in zip(told, [c for c in EC.CASES if c[1] == "rbf"]) if c[0][3] >= 257)


def synthetic():
    """Three points whose off-diagonal covariance exceeds what their diagonal allows (base_z of one point below the floor)."""
    lam = np.log(np.array([0.5, 0.3, 0.2]))
    base = np.array([0.4, -3e-17, 0.3])
    cov = np.array([[0.4, 0.2, 0.1], [0.2, 0.0, -0.25], [0.1, -0.25, 0.3]])
    return lam, base, cov


def test_the_cap_is_told_on_a_state_where_it_binds():
    lam, base, cov = synthetic()
    st = {"mu": np.zeros(3), "base": base, "cov": cov}
    _, b, _ = E.z_weights(st, 1.0, lam)
    assert b[1] == 1e-12
    S = E.pair_matrix(cov, b, 1.0)
    assert abs(S[0, 1]) <= np.sqrt(b[0] * b[1]) and abs(S[2, 1]) <= np.sqrt(b[2] * b[1]) and S[0, 2] == cov[0, 2]
    assert np.array_equal(np.diag(S), b)
    capped = E.evidence_moments(st, 1.0, lam)["log_t0"]
    free = E.evidence_moments(st, 1.0, lam, capped=False)["log_t0"]
    assert abs(capped - free) > 1e-3
    # by hand: the capped pairs contribute about +-sqrt(4e-13), nothing beside the others
    om = np.exp(lam - E.R.lse(lam + b / 2) + b / 2)
    om = om / np.sum(om)
    want = np.log(np.sum(np.outer(om, om) * np.expm1(S)))
    assert abs(capped - want) <= 1e-12


def test_edge_rules_of_the_restatement():
    lam, base, cov = synthetic()
    st = {"mu": np.zeros(3), "base": np.array([0.4, 0.2, 0.3]), "cov": cov.copy()}
    ref = E.evidence_moments(st, 1.0, lam)["log_t0"]
    st["cov"][0, 2] = st["cov"][2, 0] = np.nan                 # a non-finite off-diagonal S counts as 0
    zeroed = dict(st, cov=np.where(np.isfinite(st["cov"]), st["cov"], 0.0))
    assert E.evidence_moments(st, 1.0, lam)["log_t0"] == E.evidence_moments(zeroed, 1.0, lam)["log_t0"] != ref
    st["cov"][0, 2] = st["cov"][2, 0] = np.inf
    assert E.evidence_moments(st, 1.0, lam)["log_t0"] == E.evidence_moments(zeroed, 1.0, lam)["log_t0"]
    # T0 <= 0: -inf (a rounding-negative or underflown sum), NaN stays NaN
    b = np.array([1e-12, 1e-12])
    S = np.array([[1e-12, -1e-11], [-1e-11, 1e-12]])        # (handed over as it is: the cap would not let such an S through)
    assert E.log_t0_scaled(np.log(np.array([0.5, 0.5])), b, S) == -np.inf
    assert np.isnan(E.log_t0_scaled(np.array([np.nan, 0.0]), b, S))
    # y_std ~ 4e3: log T0 ~ 1e7 and finite
    big = max(EC.reference(c)["truth"][1] for c in EC.CASES if c[2] == 4e3)
    assert np.isfinite(big) and big > 1e7


# ---- wiring
class StubGP:
    """What ``logz_from_samples`` touches: the predictive variance and ``evidence_moments`` (recorded)."""
    ndim = 2

    def __init__(self, var=0.04):
        self.var, self.calls = var, []

    def predict_var_batched(self, x):
        return np.full(len(x), self.var)

    def evidence_moments(self, mc_points, *, log_weights=None):
        self.calls.append((np.array(mc_points), np.array(log_weights)))
        b = self.var                                        # independent points of variance b: E = sum e^{l + mu + b/2}
        lw = np.asarray(log_weights) + self.mu(mc_points)
        log_ez = float(np.logaddexp.reduce(lw + b / 2))
        log_var = float(np.logaddexp.reduce(2 * lw + b)) + b + np.log1p(-np.exp(-b))      # (+ log expm1(b))
        return {"log_ez": log_ez, "log_t0": log_var - 2 * log_ez, "log_var_z": log_var, "std_logz": 0.0}

    @staticmethod
    def mu(x):
        x = np.asarray(x)
        return -8.0 * np.sum((x - 0.5) ** 2, axis=1)


def test_logz_from_samples_moments_wiring():
    from bobe_amd import samplers
    p = inspect.signature(samplers.logz_from_samples).parameters
    assert p["moments"].kind is inspect.Parameter.KEYWORD_ONLY and p["moments"].default is False
    assert p["moments_max_points"].kind is inspect.Parameter.KEYWORD_ONLY and p["moments_max_points"].default == 65536
    for fn in (samplers.nested_sampling, samplers.nested_sampling_Dy):
        q = inspect.signature(fn).parameters
        assert q["logz_moments"].kind is inspect.Parameter.KEYWORD_ONLY and q["logz_moments"].default is False
        assert list(q)[-1] == "logz_draws_method"
    rng = np.random.default_rng(3)
    n = 60
    x = rng.uniform(size=(n, 2))
    x = x[np.argsort(StubGP.mu(x))]
    logl = StubGP.mu(x)
    logl[4] = -np.inf
    logvol = -np.arange(1, n + 1) / 10.0
    mean = float(samplers.compute_integrals(logl=logl, logvol=logvol)[-1])
    gp = StubGP()
    gp.minus_inf = -1e5
    logl[7] = -1e5
    state = np.random.get_state()[1].copy()
    base = samplers.logz_from_samples(gp, x, logl, logvol, mean, 0.01)
    assert not gp.calls and not any(k.startswith("moments") for k in base)
    out = samplers.logz_from_samples(gp, x, logl, logvol, mean, 0.01, moments=True)
    assert np.array_equal(np.random.get_state()[1], state)
    assert set(out) == set(base) | {"moments_log_ez", "moments_log_var", "moments_std", "moments_points"}
    assert all(out[k] == base[k] for k in base)
    idx = samplers.draws_points(gp, logl, logvol, 65536)
    assert out["moments_points"] == len(idx) == n - 2 and len(gp.calls) == 1
    zs, lws = gp.calls[0]
    logwt = samplers._log_weights(logl, logvol)
    assert np.array_equal(zs, x[idx]) and np.array_equal(lws, logwt[idx] - logl[idx])
    # the stub's points are independent with variance b: the closed forms by hand, the two fixed samples as constants
    b = gp.var
    fixed = np.logaddexp.reduce(logwt[[4, 7]][np.isfinite(logwt[[4, 7]])])
    log_ez = np.logaddexp(np.logaddexp.reduce(logwt[idx] + b / 2), fixed)
    log_var = np.logaddexp.reduce(2 * logwt[idx] + b) + np.log(np.expm1(b))
    assert abs(out["moments_log_ez"] - log_ez) <= 1e-12 and abs(out["moments_log_var"] - log_var) <= 1e-12
    assert abs(out["moments_std"] - np.sqrt(np.log1p(np.exp(log_var - 2 * log_ez)))) <= 1e-12
    # the cap keeps the heaviest
    gp.calls.clear()
    capped = samplers.logz_from_samples(gp, x, logl, logvol, mean, 0.01, moments=True, moments_max_points=10)
    assert capped["moments_points"] == 10 and np.array_equal(gp.calls[0][0], x[samplers.draws_points(gp, logl, logvol, 10)])
    # a large ratio is formed from the logs
    huge = StubGP(var=2000.0)
    r = samplers.logz_from_samples(huge, x, logl, logvol, mean, 0.01, moments=True)
    assert np.isfinite(r["moments_std"]) and r["moments_std"] > 30
    # two equal log-volumes in a row give a sample the weight e^-inf: it is held fixed, the report does not raise
    flat = logvol.copy()
    flat[20] = flat[19]
    gp.calls.clear()
    with np.errstate(divide="ignore"):
        assert samplers._log_weights(logl, flat)[20] == -np.inf
        r = samplers.logz_from_samples(gp, x, logl, flat, mean, 0.01, moments=True)
    assert r["moments_points"] == n - 3 and np.all(np.isfinite(gp.calls[0][1])) and np.isfinite(r["moments_std"])


def test_evidence_moments_python_wiring():
    from bobe_amd import _lib
    from bobe_amd.gp import GP, std_from_log_t0
    from bobe_amd.clf_gp import GPwithClassifier
    names = [s[0] for s in _lib.SIGNATURES]
    assert "bobe_gp_evidence_moments" in names
    p = inspect.signature(GP.evidence_moments).parameters
    assert list(p) == ["self", "mc_points", "log_weights"]
    assert p["log_weights"].kind is inspect.Parameter.KEYWORD_ONLY and p["log_weights"].default is None
    assert GPwithClassifier.evidence_moments is GP.evidence_moments
    assert abs(std_from_log_t0(-3.0) - np.sqrt(np.log1p(np.exp(-3.0)))) <= 1e-15
    assert abs(std_from_log_t0(2e7) - np.sqrt(2e7)) <= 1e-9 and np.isnan(std_from_log_t0(float("nan")))
    assert std_from_log_t0(-np.inf) == 0.0
    header = open(os.path.join(HERE, "..", "include", "bobe_gp.h")).read()
    assert "int bobe_gp_evidence_moments(bobe_gp_t* gp, const double* Z, int64_t M, double y_std, const double* logw" in header


def test_bobe_run_logz_moments_wiring():
    from bobe_amd import bo
    rp = inspect.signature(bo.BOBE.run).parameters
    assert rp["logz_moments"].kind is inspect.Parameter.KEYWORD_ONLY and rp["logz_moments"].default is False
    assert list(rp)[-1] == "wip_batch_mode" and list(rp).index("logz_moments") < list(rp).index("wip_batch_mode")
    b = bo.BOBE.__new__(bo.BOBE)
    b.logz_threshold, b.convergence_n_iters, b.convergence_counter = 0.5, 1, 0
    b.param_bounds, b.ndim = np.array([[0.0, 0.0], [1.0, 1.0]]), 2
    b.prev_samples, b.kl_history, b.convergence_history = None, [], []
    b.min_delta_seen, b.save = np.inf, False
    logz = {"upper": 1.2, "lower": 1.0, "std": 0.1, "moments_std": 0.07}
    eq = np.random.default_rng(1).uniform(size=(10, 2))
    outs = []
    for on in (False, True):
        b.logz_moments = on
        assert b._ns_extras() == ({"logz_moments": True} if on else {})
        b.convergence_counter, b.min_delta_seen = 0, np.inf
        outs.append(b.check_convergence_logz(3, dict(logz), eq, np.zeros(10), verbose=True, save_checkpoint=True))
    assert outs == [True, True]                             # (reported only: the rule is the same either way)
    off, on = b.convergence_history
    assert "moments_std" not in off and on["moments_std"] == 0.07
    assert {k: v for k, v in on.items() if k != "moments_std"} == off
    b.logz_moments = True                                  # a dictionary without the key (a NaN surrogate's): no key, no failure
    b.check_convergence_logz(4, {"upper": 1.2, "lower": 1.0}, eq, np.zeros(10), verbose=False)
    assert "moments_std" not in b.convergence_history[-1]
