"""The total variance of the evidence estimate on the device (bobe_gp_evidence_moments, GP.evidence_moments,
samplers.logz_from_samples(moments=True)) against the long-double truth of tests/evidence_moments_restatement.py on the cases of
tests/evidence_moments_cases.py.

Rule (``zvar_cases.rule``), for log_t0 and for log_ez: |device - truth| <= 4 |float64 restatement - truth| + 1e-7 (1 + |truth|).
With BOBE_EVIDENCE_PARITY_OUT set to a file name, the module writes every case's measured errors and the worst ones there
(profiles/evidence_moments_parity.txt is such a run)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evidence_moments_cases as EC  # noqa: E402
import evidence_moments_restatement as E  # noqa: E402
import zvar_cases as ZC  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_OK, BOBE_ERR_ARG, BOBE_ERR_STATE = 0, -1, -3
PARITY = []


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    yield
    path = os.environ.get("BOBE_EVIDENCE_PARITY_OUT")
    if not path or not PARITY:
        return
    with open(path, "w") as f:
        f.write("bobe_gp_evidence_moments against the long-double truth, |error| / (1 + |truth|): device log_t0, float64 "
                "restatement log_t0, device log_ez, float64 restatement log_ez\n")
        for name, row in PARITY:
            f.write("%-64s %.3e %.3e %.3e %.3e\n" % ((name,) + row))
        w = np.max(np.array([r for _, r in PARITY]), axis=0)
        f.write("%-64s %.3e %.3e %.3e %.3e\n" % (("worst of %d" % len(PARITY),) + tuple(w)))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@functools.lru_cache(maxsize=4)
def make_gp(shape, kernel, y_std, refine=False):
    from bobe_amd import GP
    d = shape[2]
    X, y, Z, lw = EC.case_data(shape, y_std)
    gp = GP(X, y, noise=EC.NOISE, kernel=kernel, lengthscales=np.full(d, EC.lengthscale(d)), kernel_variance=EC.KVAR)
    if refine:
        gp.refine_kappa = 0.0
        gp.recompute_cholesky()
        assert gp.refining
    return gp, Z, lw


def check(r, case, tag=""):
    ref = EC.reference(case)
    row = []
    for key, i in (("log_t0", 1), ("log_ez", 0)):
        truth = np.longdouble(ref["truth"][i])
        ok, err, ref_err = ZC.rule([r[key]], [ref["f64"][i]], np.array([truth]))
        row += [err, ref_err]
        print("%-64s %s: device %.3e, float64 restatement %.3e (of 1 + |truth|)" % (EC.case_id(case) + tag, key, err, ref_err))
        assert np.isfinite(r[key]) and ok, (key, r[key], float(truth), err, ref_err)
    PARITY.append((EC.case_id(case) + tag, tuple(row)))


def raw(gp, Z, m, lw, want_ez=True, want_t0=True, y_std=None):
    """The C entry itself: (status, log_ez, log_t0), an output not asked for stays at its sentinel."""
    from bobe_amd import _lib
    lez, lt0 = C.c_double(-7.0), C.c_double(-7.0)
    lib = make_gp(EC.SHAPES[1], "rbf", 1.0)[0]._lib
    st = lib.bobe_gp_evidence_moments(gp._h if gp is not None else None, _lib.ptr(Z), m,
                                      float(gp.y_std if y_std is None else y_std), _lib.ptr(lw),
                                      C.byref(lez) if want_ez else None, C.byref(lt0) if want_t0 else None)
    return st, lez.value, lt0.value


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_matches_the_long_double_truth(case):
    shape, kernel, y_std, weighted = case
    gp, Z, lw = make_gp(shape, kernel, y_std)
    assert abs(gp.y_std / y_std - 1) < 1e-12
    r = gp.evidence_moments(Z, log_weights=lw if weighted else None)
    assert set(r) == {"log_ez", "log_t0", "log_var_z", "std_logz"}
    check(r, case)
    assert same_bits(r["log_var_z"], r["log_t0"] + 2.0 * r["log_ez"])
    t = r["log_t0"]
    want = np.sqrt(t + np.log1p(np.exp(-t))) if t > 30 else np.sqrt(np.log1p(np.exp(t)))
    assert np.isfinite(r["std_logz"]) and abs(r["std_logz"] - want) <= 1e-12 * want


SUBST = [c for c in EC.CASES if c[0][3] in (129, 300) and c[1] == "rbf" and c[2] in (1.0, 4e3) and c[3]]


@pytest.mark.parametrize("case", SUBST, ids=EC.case_id)
def test_on_the_substitution_path(case):
    """``refine_kappa = 0``: V_Z from the blocked substitution instead of the product with the inverse factor."""
    shape, kernel, y_std, weighted = case
    gp, Z, lw = make_gp(shape, kernel, y_std, True)
    check(gp.evidence_moments(Z, log_weights=lw), case, " substitution")


# ---------------------------------------------------------------------------------------------------- 2. bits
def test_log_ez_is_the_sweeps_and_the_bits_do_not_depend_on_the_call():
    import torch
    case = EC.CASES[[c[0][3] for c in EC.CASES].index(300)]
    shape, kernel, y_std, _ = case
    gp, Z, lw = make_gp(shape, kernel, y_std)
    m = Z.shape[0]
    other = np.random.default_rng(5).uniform(size=(77, shape[2]))
    for w in (lw, None):
        gp.wip_sweep(other, other, criteria=("wipv",))                         # Z's cache holds another set: a miss
        a = gp.evidence_moments(Z, log_weights=w)
        b = gp.evidence_moments(Z, log_weights=w)                              # a hit
        assert same_bits(a["log_t0"], b["log_t0"]) and same_bits(a["log_ez"], b["log_ez"])
        sw = gp.wip_sweep(Z[:40], Z, log_weights=w, criteria=("zvar",))        # the sweep on the same Z: its cache too
        assert same_bits(sw["log_ez"], a["log_ez"])
        c = gp.evidence_moments(Z, log_weights=w)
        assert same_bits(a["log_t0"], c["log_t0"]) and same_bits(a["log_ez"], c["log_ez"])
        gp.wip_sweep(other[:9], other, criteria=("zvar",))                     # after a sweep on another Z
        c = gp.evidence_moments(Z, log_weights=w)
        assert same_bits(a["log_t0"], c["log_t0"]) and same_bits(a["log_ez"], c["log_ez"])
        dz = torch.as_tensor(Z, device="cuda")
        dw = None if w is None else torch.as_tensor(w, device="cuda")
        c = gp.evidence_moments(dz, log_weights=dw)                            # device pointers (no cache)
        assert same_bits(a["log_t0"], c["log_t0"]) and same_bits(a["log_ez"], c["log_ez"])
        st, lez, lt0 = raw(gp, Z, m, w)
        assert st == BOBE_OK and same_bits(lez + gp.y_mean, a["log_ez"]) and same_bits(lt0, a["log_t0"])
        st, lez, lt0 = raw(gp, Z, m, w, want_ez=False)
        assert st == BOBE_OK and lez == -7.0 and same_bits(lt0, a["log_t0"])
        st, lez, lt0 = raw(gp, Z, m, w, want_t0=False)
        assert st == BOBE_OK and lt0 == -7.0 and same_bits(lez + gp.y_mean, a["log_ez"])


# ---------------------------------------------------------------------------------------------------- 3. the share
SHARE_SHAPES = ("tile_edge", "m1", "m7", "m64", "second_z_tile_of_one", "near_noise_m65", "reference_noise_130", "ragged_4chunks")


@pytest.mark.parametrize("case", [c for c in ZC.SWEEP_CASES if c[0] in SHARE_SHAPES] +
                         [("reference_noise_130", "rbf", True, 1.0)], ids=ZC.case_id)
def test_no_candidate_removes_more_than_the_whole_variance(case):
    """exp(-zvar[c] - log_t0) is a share: -zvar[c] <= log_t0 for every finite score of the sweep (in long double the closest
    approach on these cases is -5.4e-2; the bound leaves the project's 1e-7 (1 + |log_t0|) for the two roundings)."""
    from bobe_amd import GP
    shape, kernel, weighted, y_std = case
    _, n, d, c, m, chunk, noise, ell, kvar = ZC.SHAPES[shape]
    X, y, cand, Z, lw = ZC.case_data(shape, y_std)
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=np.full(d, ell), kernel_variance=kvar)
    w = lw if weighted else None
    sw = gp.wip_sweep(cand, Z, log_weights=w, criteria=("zvar",))
    mo = gp.evidence_moments(Z, log_weights=w)
    assert same_bits(sw["log_ez"], mo["log_ez"]) and np.isfinite(mo["log_t0"])
    z = sw["zvar"][np.isfinite(sw["zvar"])]
    assert len(z)
    print("%-50s log_t0 %.6g, largest share %.4f" % (ZC.case_id(case), mo["log_t0"], np.exp(np.max(-z) - mo["log_t0"])))
    assert np.all(-z <= mo["log_t0"] + 1e-7 * (1 + abs(mo["log_t0"])))


# ---------------------------------------------------------------------------------------------------- 4. the device's own Sigma
@pytest.mark.parametrize("case", [c for c in EC.CASES if c[2] == 1.0 and c[0][3] <= 300], ids=EC.case_id)
def test_against_predict_cov_and_predict_mean(case):
    """The host's DIRECT form - Var Z = sum_zz' A_z A_z' expm1(cov_zz'), E[Z] = sum_z A_z, A_z = e^{l_z + mu_z + cov_zz / 2},
    unscaled and uncapped (``evidence_moments_restatement.direct_var``) - on the device's own joint covariance and mean of the
    same points, under the same rule.  y_std = 1: every exponent is small, nothing needs the scaling."""
    shape, kernel, y_std, weighted = case
    gp, Z, lw = make_gp(shape, kernel, y_std)
    cov = np.atleast_2d(gp.predict_cov(Z))
    mu = np.asarray(gp.predict_mean_batched(Z)) - gp.y_mean
    var, ez = E.direct_var(mu, cov, lw if weighted else -mu)
    got = {"log_ez": np.log(ez) + gp.y_mean, "log_t0": np.log(var) - 2.0 * np.log(ez)}
    ref = EC.reference(case)
    for key, i in (("log_t0", 1), ("log_ez", 0)):
        ok, err, ref_err = ZC.rule([got[key]], [ref["f64"][i]], np.array([np.longdouble(ref["truth"][i])]))
        print("%-64s %s: direct form on the device's Sigma %.3e, float64 restatement %.3e" % (EC.case_id(case), key, err, ref_err))
        assert ok, (key, err, ref_err)


# ---------------------------------------------------------------------------------------------------- 5. errors and edges
def test_refusals_and_the_cap():
    from bobe_amd import GP, _lib
    shape = EC.SHAPES[1]
    gp, Z, lw = make_gp(shape, "rbf", 1.0)
    m = Z.shape[0]
    assert raw(gp, None, m, lw)[0] == BOBE_ERR_ARG and _lib.last_error()
    assert raw(gp, Z, 0, lw)[0] == BOBE_ERR_ARG
    assert raw(gp, Z, m, lw, want_ez=False, want_t0=False)[0] == BOBE_ERR_ARG
    assert raw(None, Z, m, lw, y_std=1.0)[0] == BOBE_ERR_ARG
    X, y, _, _ = EC.case_data(shape, 1.0)
    bare = GP(X, y, noise=EC.NOISE, lengthscales=np.full(shape[2], 0.4), kernel_variance=EC.KVAR, _factor=False)
    assert raw(bare, Z, m, lw, y_std=1.0) == (BOBE_ERR_STATE, -7.0, -7.0)
    # the cap: K(X,Z), V_Z and W_Z, Np x Mp doubles each, over 16 GiB in all (Np = 256 here: Mp > 2^31 / 768); nothing is read
    # or allocated before the refusal
    too_many = (2 ** 31 // (3 * 256) // 128 + 1) * 128
    assert raw(gp, Z, too_many, None) == (BOBE_ERR_ARG, -7.0, -7.0) and "16 GiB" in _lib.last_error()
    with pytest.raises(ValueError):
        gp.evidence_moments(Z, log_weights=lw[:-1])
    r = gp.evidence_moments(Z, log_weights=lw)
    assert np.isfinite(r["log_t0"])


def test_a_nan_state_returns_ok_with_nan_outputs():
    from bobe_amd import GP
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(40, 3))
    X[7] = X[3]
    Z = rng.uniform(size=(150, 3))
    gp = GP(X, np.sin(X[:, 0]), noise=1e-30, lengthscales=np.full(3, 0.5), kernel_variance=1.0, pivot_floor_ulp=64)
    assert gp.not_pd
    mu = np.asarray(gp.predict_mean_batched(Z))
    assert np.all(np.isnan(mu))
    st, lez, lt0 = raw(gp, Z, 150, np.zeros(150))                # (given weights: l_z + mu_z is NaN where mu_z is)
    assert st == BOBE_OK and np.isnan(lez) and np.isnan(lt0)
    assert np.isnan(gp.evidence_moments(Z, log_weights=np.zeros(150))["std_logz"])
    st, lez, lt0 = raw(gp, Z, 150, None)                          # (posterior-draw weights: l_z + mu_z = -mu_z + mu_z is NaN too)
    assert st == BOBE_OK and np.isnan(lez) and np.isnan(lt0)


# ---------------------------------------------------------------------------------------------------- 6. the nested-sampling report
def test_logz_from_samples_with_moments():
    from bobe_amd import samplers
    shape = EC.SHAPES[2]
    gp, _, _ = make_gp(shape, "rbf", 1.0)
    rng = np.random.default_rng(11)
    n = 400
    x = rng.uniform(size=(n, shape[2]))
    logl = np.sort(np.asarray(gp.predict_mean_batched(x), dtype=np.float64))
    x = x[np.argsort(np.asarray(gp.predict_mean_batched(x)))]
    logvol = -np.arange(1, n + 1) / 50.0
    mean = float(samplers.compute_integrals(logl=logl, logvol=logvol)[-1])
    state = np.random.get_state()[1].copy()
    base = samplers.logz_from_samples(gp, x, logl, logvol, mean, 0.01)
    out = samplers.logz_from_samples(gp, x, logl, logvol, mean, 0.01, moments=True)
    assert np.array_equal(np.random.get_state()[1], state)
    assert set(out) == set(base) | {"moments_log_ez", "moments_log_var", "moments_std", "moments_points"}
    for k in base:
        assert same_bits(base[k], out[k]), k
    assert all(np.isfinite(out[k]) for k in ("moments_log_ez", "moments_log_var", "moments_std"))
    assert out["moments_points"] == n and out["moments_std"] > 0
    # every sample free and logl the surrogate's own mean: E[Z] = sum_z e^{logwt_z + b_z / 2} >= Z(mean), and close to it
    assert out["moments_log_ez"] >= mean - 1e-9 and out["moments_log_ez"] - mean < 0.5 * float(np.max(gp.predict_var_batched(x))) + 1e-9
    # a gate: the marked samples and a cap hold the rest fixed
    gp.minus_inf = -1e5
    try:
        gated = logl.copy()
        gated[:25] = -1e5
        g = samplers.logz_from_samples(gp, x, gated, logvol, mean, 0.01, moments=True, moments_max_points=100)
        assert g["moments_points"] == 100
        g = samplers.logz_from_samples(gp, x, gated, logvol, mean, 0.01, moments=True)
        assert g["moments_points"] == n - 25 and np.isfinite(g["moments_std"])
    finally:
        del gp.minus_inf
