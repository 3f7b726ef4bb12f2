"""Appended and kriging-believer states in the regime the reference runs in: the conditioning ladder, after GP.update.

At unchanged hyper-parameters GP.update does not refactorise (gp.py:541 does): bobe_gp_append (gp_sweep.hip) grows the factor
in place.  V = L^-1 K(X_old, X_new) comes from solve_v (the plain product with the inverse factor, or the blocked substitution
where the factor counts as ill conditioned), W = Linv^T V from k_trimul_t, S = K22 + noise - V^T V from k_gram_small, factored
on the host with its own rank test; k_append_rows writes the new rows of L and of L^-1 (-L22^-1 W^T), alpha = Linv^T Linv y,
and the refinement decision is taken on the grown factor's smallest pivot.  The kriging believer picks members 2..n of a batch
on such states (acquisition.py, get_next_batch / _believer_gp); the BO loop appends up to 40 points between refits.

Every appended state is compared on its OWN grown data - gp.train_x / gp.train_y read after the update (update() re-standardises
y through a round trip, so the bits differ from a fresh GP(X, y)) - three ways: the extended-precision truth
(oracle.c_binding.gp_truth, x87 long double), the LAPACK form (dpotrf + solve_triangular) and the appended GPU state, under the
ladder's rule with its constants (tests/test_gpu_conditioning.py):

    err(append vs truth) <= 4 x err(LAPACK vs truth) + TOL[q]

for the posterior mean and variance, the fantasy variance, WIPV / WIPStd (the sweep's, and the values of the gradient entry
point on its few-candidate and batched paths), and the ladder's argmin rule.  A fresh GPU factorisation of the same data (a
device clone of the state, refactorised) is recorded beside it and must take the same refinement decision.  The rank test is
off (pivot_floor_ulp = 0, the reference's sign rule) except in the rank-verdict cases, which run at BOBE's 64 ulp.  The table
goes to build/append_conditioning.txt, or where BOBE_APPEND_CONDITIONING_OUT names (committed as
profiles/append_conditioning.txt).
"""
import functools
import os

import numpy as np
import pytest
from scipy.linalg import cho_solve, solve_triangular

from conditioning_common import LADDER, NOISE, TOL, _bo_like_design, _err, _quantities, ladder_points

pytestmark = pytest.mark.gpu

QS = ("mean", "var", "fantasy", "wipv", "wipstd")
REFINE_KAPPA = 1e6                      # the library's default threshold of the refinement decision
EPS = 2.220446049250313e-16
_ROWS, _RANK_ROWS = [], []


@functools.lru_cache(maxsize=None)
def _design(n):
    return _bo_like_design(n)


def _rung(rung):
    n, kernel, ls, kvar = LADDER[rung]
    return n, kernel, np.array(ls), kvar


def _ids(rungs):
    return [f"rung{r}_{LADDER[r][1]}_kvar{LADDER[r][3]:g}" for r in rungs]


def _gp(X, y, kernel, ls, kvar, noise=NOISE, ulp=0.0):
    from bobe_amd import GP
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar, pivot_floor_ulp=ulp)


def _update(gp, x, y):
    """GP.update(x, y); returns where the installed factor came from right after it (bobe_debug_factor_source): -1 = the
    rank-b append grew it, 0 = a factorisation (the append refused S, or was not taken)."""
    x = np.atleast_2d(x)
    n0 = gp.npoints
    gp.update(x, np.asarray(y, dtype=np.float64).reshape(-1, 1))
    assert gp.npoints == n0 + x.shape[0], "update()'s duplicate filter dropped a point"
    return gp._lib.bobe_debug_factor_source(gp._h)


def _state(gp, cand, Z):
    """The compared quantities of the factor installed on ``gp`` (None where it is not positive definite)."""
    if gp.not_pd:
        return None
    sw = gp.wip_sweep(cand, Z, want_mean_var=True)
    s = {"mean": sw["mean"], "var": sw["var"], "fantasy": gp.fantasy_var(cand, Z) / gp.y_std ** 2, "wipv": sw["wipv"],
         "wipstd": sw["wipstd"], "argmin_v": int(sw["argmin_v"]), "argmin_s": int(sw["argmin_s"]), "refining": gp.refining}
    for label, k in (("few", 3), ("batched", 20)):            # bobe_gp_wip_grad: <= 16 candidates take the vector path
        s["wipv_grad_" + label], s["wipstd_grad_" + label], _, _ = gp.wip_grad(cand[:k], Z)
    return s


def _fresh(gp, cand, Z):
    """The same quantities after a fresh GPU factorisation of gp's data: a device clone (the same X and y bits), refactorised."""
    fr = gp.copy()
    fr.recompute_cholesky()
    return _state(fr, cand, Z)


def _truth_and_lapack(gp, kernel, ls, kvar, cand, Z):
    """The truth and the LAPACK form (tests/test_gpu_conditioning.py (ii)) on gp's grown data and standardisation."""
    from oracle import bobe_oracle as O
    from oracle import c_binding as CB
    X, ys = gp.train_x, gp.train_y.reshape(-1)
    tr = CB.gp_truth(0 if kernel == "rbf" else 1, X, ys, ls, kvar, NOISE, cand, Z, want_grad=False)
    assert tr["info"] == 0 and tr["digits"] >= 64
    T = _quantities(np.nan, None, tr["mean"], tr["var"], tr["fantasy"], gp.y_std)
    kern = O.get_kernel(kernel)
    L = O.chol_nan(kern(X, X, ls, kvar, NOISE, include_noise=True))
    if not np.all(np.isfinite(L)):
        return tr, T, None
    kc, kz = kern(X, cand, ls, kvar, NOISE, include_noise=False), kern(X, Z, ls, kvar, NOISE, include_noise=False)
    vc = solve_triangular(L, kc, lower=True, check_finite=False)
    vz = solve_triangular(L, kz, lower=True, check_finite=False)
    kself = kvar + NOISE
    sc = kself - np.sum(vc * vc, axis=0)
    cross = kern(cand, Z, ls, kvar, NOISE, include_noise=False) - vc.T @ vz
    with np.errstate(all="ignore"):
        fant = (kself - np.sum(vz * vz, axis=0))[None, :] - cross * cross / sc[:, None]
    fant = np.where(sc[:, None] >= 0, fant, np.nan)
    alpha = cho_solve((L, True), ys, check_finite=False)
    return tr, T, _quantities(np.nan, None, kc.T @ alpha, sc, fant, gp.y_std)


def _measure(case, gp, kernel, ls, kvar, cand, Z):
    """One table row: the appended state on ``gp``, a fresh GPU factorisation of its data and LAPACK, each against the truth."""
    app = _state(gp, cand, Z)
    fresh = _fresh(gp, cand, Z)
    tr, T, lap = _truth_and_lapack(gp, kernel, ls, kvar, cand, Z)
    scales = {"mean": None, "var": kvar + NOISE, "fantasy": kvar + NOISE, "wipv": None, "wipstd": None}
    nan = float("nan")
    r = {"case": case, "N": gp.npoints, "kvar": kvar, "min_pivot": tr["min_pivot"], "ratio": (kvar + NOISE) / tr["min_pivot"]}
    for tag, s in (("app", app), ("fresh", fresh), ("lap", lap)):
        r[tag + "_ok"] = s is not None
        for q in QS:
            r[f"{tag}_{q}"] = _err(s[q], T[q], scales[q]) if s is not None else nan
        for key, name in (("wipv", "argmin_v"), ("wipstd", "argmin_s")):
            it = int(np.argmin(T[key]))
            pick = None if s is None else (int(np.argmin(s[key])) if tag == "lap" else s[name])
            r[f"{tag}_{name}"] = pick == it
            r[f"{tag}_gap_{name}"] = nan if pick is None else float((T[key][pick] - T[key][it]) / T[key][it])
        if tag != "lap":
            r[tag + "_refining"] = s is not None and s["refining"]
            for label, k in (("few", 3), ("batched", 20)):
                for key in ("wipv", "wipstd"):
                    r[f"{tag}_{key}_grad_{label}"] = (nan if s is None else
                                                      _err(s[f"{key}_grad_{label}"], T[key][:k], np.max(np.abs(T[key]))))
    r["violations"] = _violations(r) if r["app_ok"] and r["lap_ok"] else []
    _ROWS.append(r)
    _write_table()
    return r


def _violations(r):
    """What breaks the ladder's rule err(append) <= 4 x err(LAPACK) + TOL on the appended state."""
    bad = [q for q in QS if not r["app_" + q] <= 4.0 * r["lap_" + q] + TOL[q]]
    for key, name in (("wipv", "argmin_v"), ("wipstd", "argmin_s")):
        if not (r["app_" + name] or r["app_gap_" + name] <= 4.0 * r["lap_" + key] + TOL[key]):
            bad.append(name)
    for label in ("few", "batched"):
        for key in ("wipv", "wipstd"):
            if not r[f"app_{key}_grad_{label}"] <= 4.0 * r["lap_" + key] + TOL[key]:
                bad.append(f"{key}_grad_{label}")
    return bad


def _check(r):
    assert r["app_ok"] == r["fresh_ok"], ("the appended state's verdict is not the factorisation's", r)
    assert r["app_ok"] or not r["lap_ok"], ("the append fails where LAPACK's factorisation passes", r)
    if abs(np.log(r["ratio"] / REFINE_KAPPA)) > np.log(2.0):       # (not where the decision sits on the threshold)
        assert r["app_refining"] == r["fresh_refining"], ("refinement decision", r)
    if r["app_ok"] and r["lap_ok"]:                                # (where LAPACK fails: the verdicts above only)
        assert not r["violations"], r


CASE_A = [1, 2, 3, 4, 5, 7, 8]


@pytest.mark.parametrize("b", [1, 4])
@pytest.mark.parametrize("rung", CASE_A, ids=_ids(CASE_A))
def test_single_append_is_as_close_to_the_truth_as_lapack(rung, b):
    """The design's first N - b points factorised, its last b appended."""
    n, kernel, ls, kvar = _rung(rung)
    X, y, spare = _design(n)
    cand, Z = ladder_points(X, spare, rung)
    gp = _gp(X[:n - b], y[:n - b], kernel, ls, kvar)
    assert not gp.not_pd
    assert _update(gp, X[n - b:], y[n - b:]) == -1, "update() did not take the append route"
    _check(_measure(f"A rung{rung} b={b}", gp, kernel, ls, kvar, cand, Z))


@pytest.mark.parametrize("b", [1, 4])
def test_the_bound_rejects_the_plain_inverse_product_on_an_appended_state(b):
    """Negative control: case A on rung 3 with every V formed as the plain product with the inverse factor (refine_kappa = -1,
    in force from the factorisation of the N - b points on: the append's V and every later output).  The ladder records the
    raw WIPV 100 % wrong there against LAPACK's 1.5 %: the rule must reject the state, or the cases above could not fail."""
    rung = 3
    n, kernel, ls, kvar = _rung(rung)
    X, y, spare = _design(n)
    cand, Z = ladder_points(X, spare, rung)
    gp = _gp(X[:n - b], y[:n - b], kernel, ls, kvar)
    gp.refine_kappa = -1.0
    gp.recompute_cholesky()
    assert not gp.not_pd and not gp.refining
    assert _update(gp, X[n - b:], y[n - b:]) == -1, "update() did not take the append route"
    r = _measure(f"raw rung{rung} b={b} (control)", gp, kernel, ls, kvar, cand, Z)
    assert r["app_ok"] and r["lap_ok"] and not r["app_refining"]
    assert "wipv" in _violations(r), r


CASE_B = [2, 3, 4]


@pytest.mark.parametrize("rung", CASE_B, ids=_ids(CASE_B))
def test_believer_chain_is_as_close_to_the_truth_as_lapack(rung):
    """What get_next_batch does: one clone (_believer_gp), then three members, each the argmin of a sweep over the ladder's
    candidates, appended with the posterior mean there as its value - the most predictable points there are, the worst
    case for S.  Every state on the way is checked."""
    from bobe_amd.acquisition import _believer_gp
    n, kernel, ls, kvar = _rung(rung)
    X, y, spare = _design(n)
    cand, Z = ladder_points(X, spare, rung)
    gp = _gp(X, y, kernel, ls, kvar)
    dummy = _believer_gp(gp)
    for member in (1, 2, 3):
        x = cand[int(dummy.wip_sweep(cand, Z)["argmin_v"])]
        assert _update(dummy, x, dummy.predict_mean_single(x)) == -1, ("update() did not take the append route", member)
        _check(_measure(f"B rung{rung} member {member}", dummy, kernel, ls, kvar, cand, Z))


def test_forty_appends_across_a_tile_edge_end_as_close_to_the_truth_as_lapack():
    """40 single-point appends from N0 = 1760 on rung 3 (the BO loop between refits), across the 1792-row tile edge; the
    final state against its truth."""
    rung, n0 = 3, 1760
    n, kernel, ls, kvar = _rung(rung)
    X, y, spare = _design(n)
    cand, Z = ladder_points(X, spare, rung)
    gp = _gp(X[:n0], y[:n0], kernel, ls, kvar)
    for i in range(n0, n):
        assert _update(gp, X[i], y[i]) == -1, ("update() did not take the append route", i)
    _check(_measure(f"C rung{rung} 40 x b=1 from {n0}", gp, kernel, ls, kvar, cand, Z))


def test_wide_append_across_a_tile_edge_is_as_close_to_the_truth_as_lapack():
    """One append of b = 64 (update()'s largest) from N0 = 1750 on a design of 1814 points, rung 3's hyper-parameters."""
    rung, n, n0 = 3, 1814, 1750
    _, kernel, ls, kvar = _rung(rung)
    X, y, spare = _design(n)
    cand, Z = ladder_points(X, spare, rung)
    gp = _gp(X[:n0], y[:n0], kernel, ls, kvar)
    assert _update(gp, X[n0:], y[n0:]) == -1, "update() did not take the append route"
    _check(_measure(f"C rung{rung} b=64 from {n0}", gp, kernel, ls, kvar, cand, Z))


# (rung, noise).  Every pivot of K + noise I is at least the noise, so at noise 1e-8 the truth's smallest pivot cannot fall
# below floor / 4 (64 ulp of kvar + noise, over 4) on any rung here: the last case lowers the noise to reach that side too.
RANK = [(4, NOISE), (5, NOISE), (8, NOISE), (4, 1e-10)]
DISTANCES = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2)


@pytest.mark.parametrize("rung,noise", RANK, ids=[f"rung{r}_{LADDER[r][1]}_noise{nz:g}" for r, nz in RANK])
def test_rank_verdict_of_the_append_is_the_factorisations(rung, noise):
    """BOBE's rank test (pivot_floor_ulp = 64): the append tests S's pivots on the host, the factorisation its pivots in
    k_mll_terms.  A point 1e-4 ... 1e-2 from a training point (along one coordinate, by more than update()'s duplicate
    filter lets through); the truth's smallest pivot of the grown set against floor = 64 ulp of (kvar + noise): below
    floor / 4 the append and the refactorisation both refuse (not_pd, NaN state), above 4 floor both accept, in between
    the case is recorded.  After a refused append the next update must leave a usable handle (_refresh_after_update)."""
    from oracle import c_binding as CB
    n, kernel, ls, kvar = _rung(rung)
    X, y, spare = _design(n)
    base = _gp(X, y, kernel, ls, kvar, noise=noise, ulp=64.0)
    assert not base.not_pd
    floor = 64.0 * EPS * (kvar + noise)
    j = 64 + 100                                   # a point of the posterior bulk (the T = 1 chain)
    k = int(np.argmin(X[j, :-1]))                  # its smallest coordinate: the filter lets through |dx| > 1e-6 + 1e-4 |x|
    for dist in DISTANCES:
        x = X[j].copy()
        x[k] += dist if x[k] + dist <= 1.0 else -dist
        gp = base.copy()
        yx = gp.predict_mean_single(x)
        src = _update(gp, x, yx)
        ref = base.copy()
        ref.append_updates = False                 # update()'s refactorisation route, on the same data bits
        ref.update(x, np.array([[yx]]))
        tr = CB.gp_truth(0 if kernel == "rbf" else 1, gp.train_x, gp.train_y.reshape(-1), ls, kvar, noise, want_grad=False)
        assert tr["info"] == 0
        mp = tr["min_pivot"]
        band = "refuse" if mp < floor / 4 else ("accept" if mp > 4 * floor else "record")
        row = {"rung": rung, "kernel": kernel, "kvar": kvar, "noise": noise, "dist": dist, "min_pivot": mp, "floor": floor,
               "band": band, "append": src == -1, "not_pd": bool(gp.not_pd), "ref_not_pd": bool(ref.not_pd), "next": "-"}
        _RANK_ROWS.append(row)
        _write_table()
        if src != -1:                              # the append refused S: the library refactorised the grown data
            assert gp.not_pd == ref.not_pd, row
        if gp.not_pd:
            assert np.all(np.isnan(gp.cholesky)), row
            # the next update (a posterior sample off the design): no usable factor, so update() refactorises
            src2 = _update(gp, spare[0], y[j])
            chk = gp.copy()
            chk.recompute_cholesky()
            assert src2 == 0 and gp.not_pd == chk.not_pd, row
            if not gp.not_pd:
                assert np.all(np.isfinite(gp.predict_batched(spare[:8])[0])), row
            row["next"] = "not_pd" if gp.not_pd else "ok"
            _write_table()
        if band == "refuse":
            assert not row["append"] and row["not_pd"] and row["ref_not_pd"], row
        elif band == "accept":
            assert row["append"] and not row["not_pd"] and not row["ref_not_pd"], row


def _write_table():
    out = os.environ.get("BOBE_APPEND_CONDITIONING_OUT", os.path.join("build", "append_conditioning.txt"))
    try:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    except OSError:
        return

    def tf(*v):
        return "/".join("T" if b else "F" for b in v)
    lines = ["# appended and kriging-believer states (tests/test_gpu_append_conditioning.py): the conditioning ladder's design, "
             "rungs, candidates and integration points, noise 1e-8, rank test off",
             "# errors against the extended-precision truth (x87 long double) of the grown data: 'app' = the appended GPU state "
             "(bobe_gp_append), 'fresh' = a fresh GPU factorisation of the same data, 'lap' = LAPACK dpotrf + dtrsm",
             "# mean / wipv / wipstd: max |delta| / max |truth|;  var / fantasy: max |delta| / (kvar + noise);  grad_v / grad_s = "
             "the WIPV / WIPStd values of bobe_gp_wip_grad on the appended state (few: 3 candidates, batched: 20)",
             "# ratio = (kvar + noise) / the truth's smallest pivot;  refine a/f = the appended / fresh state solves for v by "
             "blocked substitution;  argmin a/f/l = picks the truth's candidate;  violations of err(app) <= 4 err(lap) + TOL", ""]
    lines.append(f"{'case':<30}{'N':>5}{'kvar':>9}{'ratio':>9} {'refine':>6} "
                 + " ".join(f"{q + '_app':>12}{'fresh':>9}{'lap':>9}" for q in QS)
                 + f" {'grad_v few':>10}{'batched':>9} {'grad_s few':>10}{'batched':>9} {'argv':>6} {'args':>6}  violations")
    for r in _ROWS:
        cells = " ".join(f"{r['app_' + q]:>12.2e}{r['fresh_' + q]:>9.2e}{r['lap_' + q]:>9.2e}" for q in QS)
        lines.append(f"{r['case']:<30}{r['N']:>5}{r['kvar']:>9.3g}{r['ratio']:>9.1e} {tf(r['app_refining'], r['fresh_refining']):>6} "
                     f"{cells} {r['app_wipv_grad_few']:>10.2e}{r['app_wipv_grad_batched']:>9.2e} "
                     f"{r['app_wipstd_grad_few']:>10.2e}{r['app_wipstd_grad_batched']:>9.2e} "
                     f"{tf(r['app_argmin_v'], r['fresh_argmin_v'], r['lap_argmin_v']):>6} "
                     f"{tf(r['app_argmin_s'], r['fresh_argmin_s'], r['lap_argmin_s']):>6}  {','.join(r['violations']) or '-'}")
    lines += ["", "# rank verdict (pivot_floor_ulp = 64): a point `dist` from a training point appended; minpiv = the truth's "
              "smallest pivot of the grown set, floor = 64 ulp of (kvar + noise); band: refuse < floor/4, accept > 4 floor",
              "# append = the append installed the grown factor (else it refused S and the library refactorised); not_pd = the "
              "GP's verdict after update(), ref = update()'s refactorisation route; next = the state after the following update()",
              f"{'rung':<26}{'noise':>8}{'dist':>8}{'minpiv':>10}{'floor':>10} {'band':>6} {'append':>6} {'not_pd':>6} {'ref':>6} "
              f"{'next':>6}"]
    for r in _RANK_ROWS:
        name = f"rung{r['rung']}_{r['kernel']}_kv{r['kvar']:g}"
        lines.append(f"{name:<26}{r['noise']:>8.0e}{r['dist']:>8.0e}{r['min_pivot']:>10.2e}{r['floor']:>10.2e} {r['band']:>6} "
                     f"{str(r['append']):>6} {str(r['not_pd']):>6} {str(r['ref_not_pd']):>6} {r['next']:>6}")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
