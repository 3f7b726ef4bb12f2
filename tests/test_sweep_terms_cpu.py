"""The checker of the sweep's intermediates (tests/sweep_terms_restatement.py, tests/sweep_terms_cases.py) has teeth, and its
yardsticks are what they are said to be.  No GPU: the float64 NumPy stages stand in for the device.

  - the float64 stages pass every Layer A bound on every case, on the product and on the substitution;
  - the kernel allowance's constant is four times what the float64 kernel needs;
  - an inverse factor with 64-ulp componentwise noise fails the inverse-factor check and pushes the evidence-variance score
    of the near-noise 2-D design past its rule, while the same noise on k(z, c) does not;
  - a crossT with one tile's columns shifted by one fails the cross check, a V with the last live row of a ragged row tile
    zeroed fails the V check (product and substitution), and s_c from another V fails its own;
  - Layer B's cases meet the preconditions of asserting the device's rule and argmin;
  - where the device misses the rule (sweep_terms_cases.KNOWN_MISSES), float64 NumPy's product with SciPy's inverse factor
    misses it as widely, and a substitution with 16-row diagonal blocks holds it.

What the inverse-factor check cannot see is recorded as well: its bound gamma_N |L^-1| |L| |L^-1| is at least gamma_N
|Linv_ij|, so relative noise below N / 2 ulp (N / 2: eps is half an ulp) stays at rho <= 1, inside the "+ 1" of rho <= 4 rho_ref
+ 1 - at N = 64 that is noise of 32 ulp, which already moves the score by 1e-6 (1 + |truth|).  Layer A names a stage that breaks
its rounding bound; a stage that keeps it can still lose the score, and that is Layer B's to catch."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sweep_terms_cases as SC  # noqa: E402
import sweep_terms_restatement as S  # noqa: E402
import zvar_cases as ZC  # noqa: E402
import zvar_restatement as R  # noqa: E402
from batch_select_restatement import masked_argmin  # noqa: E402

LD = np.longdouble
NEAR = ("near_noise_m63", "rbf", True, 30.0)


@pytest.mark.parametrize("substitution", (False, True), ids=("product", "substitution"))
@pytest.mark.parametrize("name", list(SC.CASES))
def test_float64_stages_pass_every_bound(name, substitution):
    res = SC.check(name, SC.float64_stages(name, substitution))
    print("\n" + "\n".join(SC.table_lines("%s float64 %s" % (name, "substitution" if substitution else "product"), res)))
    assert res["inverse"]["ok"] and res["inverse"]["rho"] <= 0.1          # (SciPy's own solve against itself)
    for k, v in S.stage_ratios(res).items():
        assert v <= 0.5, (k, v)                                              # (measured: 0.02 .. 0.24)


def test_the_kernel_allowance_is_four_times_what_float64_needs():
    need = 0.0
    for shape, kernel in SC.CASES.values():
        X, cand, Z, ls, kvar, _, _ = SC.shape_args(shape)
        need = max(need, S.kernel_constant_needed(kernel, X, cand, ls, kvar), S.kernel_constant_needed(kernel, X, Z, ls, kvar))
    print("the float64 kernel needs c_k = %.3f" % need)
    assert 0.95 * SC.CK_NEEDED <= need <= SC.CK_NEEDED and SC.CK == 4 * SC.CK_NEEDED


def test_gamma_and_the_s_check_policy():
    assert float(S.gamma(64)) == pytest.approx(64 * 2.0 ** -53, rel=1e-12) and S.gamma(64) > 64 * S.EPS
    V = np.array([[1.0, np.nan, 0.5], [0.5, 1.0, 0.25]])
    s = 2.0 - np.sum(V * V, axis=0)
    assert np.isnan(s[1]) and S.check_s(V, 2.0, s)[0] <= 1.0
    assert S.check_s(V, 2.0, np.where(np.isnan(s), 1e-12, s))[0] == np.inf       # a floor where the raw s is NaN
    assert S.check_s(V, 2.0, np.array([s[0], np.nan, np.nan]))[0] == np.inf
    assert S.check_s(V, 2.0, s + np.array([0.0, 0.0, 1e-15]))[0] > 1.0


# ---------------------------------------------------------------------------------------------------- teeth
def near_noise_parts():
    shape, kernel, weighted, y_std = NEAR
    X, cand, Z, ls, kvar, noise, _ = SC.shape_args(shape)
    base = S.float64_stages(kernel, X, cand, Z, ls, kvar, noise, False)
    kxc, kxz = R.kernel(kernel, X, cand, ls, kvar, np.float64), R.kernel(kernel, X, Z, ls, kvar, np.float64)
    s64, _, _, std = ZC.states(shape, kernel, y_std)
    lw = ZC.case_data(shape, y_std)[4]
    ref = ZC.sweep_reference(NEAR)

    def rule(st):
        return ZC.rule(R.zvar_scores(st, std, lw)["zvar"], ref["f64"], ref["truth"])
    return base, kxc, kxz, kvar + noise, s64, rule


def noisy(A, ulps, seed):
    """Componentwise relative noise, uniform in [-ulps, ulps] units in the last place of 1 (2^-52)."""
    return A * (1.0 + np.random.default_rng(seed).uniform(-ulps, ulps, size=A.shape) * 2.0 ** -52)


def test_noise_on_the_inverse_factor_is_caught_and_noise_on_kzc_is_harmless():
    base, kxc, kxz, kself, s64, rule = near_noise_parts()
    ok, err, ref_err = rule(S.state_from_stages(base, s64))
    print("float64 stages: %.3e of 1 + |truth| (LAPACK restatement %.3e)" % (err, ref_err))
    assert ok
    for seed in (0, 1, 2):
        t = S.stages_from(base["L"], noisy(base["Linv"], 64, seed), kxc, kxz, kself, False)
        inv = S.check_inverse(t["L"], t["Linv"])
        ok, err, _ = rule(S.state_from_stages(t, s64))
        half = S.check_inverse(base["L"], noisy(base["Linv"], 32, seed))
        print("seed %d: 64-ulp noise on Linv: rho %.3f (rho_ref %.3f), zvar %.3e; 32 ulp: rho %.3f" % (
            seed, inv["rho"], inv["rho_ref"], err, half["rho"]))
        assert not inv["ok"] and inv["rho"] > 1.9
        assert not ok and err > 5e-7
        # every later stage is judged on ITS inputs - the noisy inverse included - and stays at rounding level
        X, cand, Z, ls, kvar, noise, _ = SC.shape_args(NEAR[0])
        res = S.check_stages(t, NEAR[1], X, cand, Z, ls, kvar, noise, SC.CK)
        assert max(res[k][0] for k in ("V", "VZ", "crossT", "sc", "basez")) <= 0.5
        st = S.state_from_stages(base, s64)
        st["kcz"] = noisy(st["kcz"], 64, seed)
        ok, err, _ = rule(st)
        print("        the same noise on k(z, c): zvar %.3e" % err)
        assert ok


def test_a_shifted_cross_tile_is_caught():
    t = dict(SC.float64_stages("fused_ragged", False))
    x = t["crossT"].copy()
    x[:, 128:256] = t["crossT"][:, 129:257]
    t["crossT"] = x
    res = SC.check("fused_ragged", t)
    assert res["crossT"][0] > 1e6 and 128 <= res["crossT"][1][1] < 256
    assert max(res[k][0] for k in ("V", "VZ", "sc", "basez")) <= 0.5


@pytest.mark.parametrize("substitution", (False, True), ids=("product", "substitution"))
def test_a_dropped_last_live_row_is_caught(substitution):
    t = dict(SC.float64_stages("two_row_tiles", substitution))
    n = t["V"].shape[0]
    assert n % 128 == 2
    V = t["V"].copy()
    V[n - 1] = 0.0
    t["V"] = V
    res = SC.check("two_row_tiles", t)
    assert res["V"][0] > 1e6 and res["V"][1][0] == n - 1
    assert res["sc"][0] > 1.0 and res["crossT"][0] > 1.0                       # (formed from the full V)
    assert res["VZ"][0] <= 0.5 and res["basez"][0] <= 0.5


# ---------------------------------------------------------------------------------------------------- Layer B's cases
@pytest.mark.parametrize("case", SC.LAYER_B, ids=ZC.case_id)
def test_layer_b_cases_meet_the_rules_preconditions(case):
    ref = ZC.sweep_reference(case)
    truth = ref["truth"]
    assert np.all(np.isfinite(truth)) and np.all(np.isfinite(ref["f64"]))
    err = float(np.max(np.abs(ref["f64"].astype(LD) - truth) / (1 + np.abs(truth))))
    gap = R.W.two_best_gap(truth)
    print("%s: float64 against long double %.3e, gap of the two best %.3e" % (ZC.case_id(case), err, gap))
    assert err <= 1e-7 and gap > ZC.GAP_MIN
    assert masked_argmin(ref["f64"]) == masked_argmin(truth)


def test_the_product_with_the_inverse_loses_the_score_whoever_forms_it():
    """(kvar + noise) / smallest pivot of the 2-D designs is above the default refine_kappa of 1e6 - the handle substitutes
    there - and at the draw of seed 143 float64 NumPy's product with SciPy's inverse factor misses the rule by as much as the
    device does (1.9e-6), on the product path and - N = 64 <= one diagonal block: the same arithmetic, bit for bit - on the
    substitution with 128-row blocks: every stage at rounding level, the loss the product's own.  The same substitution with
    diagonal blocks of 16 rows (their inverses are the 16 x 16 diagonal blocks of the same inverse factor) holds the rule:
    what the device's diagonal-block step would have to do."""
    for name, kappa in (("near_noise_2d-rbf", 1.32e6), ("near_noise_2d-seed143", 1.37e6)):
        piv = np.min(np.diag(SC.float64_stages(name, False)["L"])) ** 2
        print("%s: (kvar + noise) / min pivot = %.4g" % (name, (2.0 + 1e-6) / piv))
        assert 1e6 < (2.0 + 1e-6) / piv and abs((2.0 + 1e-6) / piv / kappa - 1) < 0.05
    case = ("near_noise_s143_m63", "rbf", True, 30.0)
    assert case in SC.KNOWN_MISSES and set(SC.KNOWN_MISSES) <= set(SC.LAYER_B)
    assert all(set(v[1]) == set(SC.PATHS) for v in SC.KNOWN_MISSES.values())
    shape, kernel, _, y_std = case
    s64, _, _, std = ZC.states(shape, kernel, y_std)
    lw = ZC.case_data(shape, y_std)[4]
    ref = ZC.sweep_reference(case)

    def score(t):
        return ZC.rule(R.zvar_scores(S.state_from_stages(t, s64), std, lw)["zvar"], ref["f64"], ref["truth"])
    a, b = SC.float64_stages("near_noise_2d-seed143", False), SC.float64_stages("near_noise_2d-seed143", True)
    for k in ("V", "VZ", "crossT", "sc", "basez"):
        assert np.array_equal(a[k], b[k])
    ok, err, ref_err = score(a)
    print("float64 product with SciPy's inverse: %.3e of 1 + |truth| (LAPACK restatement %.3e)" % (err, ref_err))
    assert not ok and err > 1e-6
    X, cand, Z, ls, kvar, noise, _ = SC.shape_args(shape)
    kxc, kxz = R.kernel(kernel, X, cand, ls, kvar, np.float64), R.kernel(kernel, X, Z, ls, kvar, np.float64)
    V, VZ = S.substitute(a["L"], a["Linv"], kxc, rows=16), S.substitute(a["L"], a["Linv"], kxz, rows=16)
    ok, err, _ = score({"crossT": VZ.T @ V, "sc": kvar + noise - np.sum(V * V, axis=0),
                        "basez": kvar + noise - np.sum(VZ * VZ, axis=0)})
    print("float64 substitution with 16-row diagonal blocks: %.3e" % err)
    assert ok
    assert len(SC.LAYER_B) == 15 and sum(c[0].startswith("near_noise_") for c in SC.LAYER_B) == 9
