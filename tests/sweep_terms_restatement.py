"""What the acquisition sweep forms on the way to its scores (``bobe_debug_sweep_terms``: V = L^-1 K(X, C), V_Z, crossT = V_Z^T V,
s_c, base_z), restated stage by stage.  Shared by tests/test_sweep_terms_cpu.py and tests/test_gpu_sweep_terms.py; NumPy (and
SciPy's triangular solve as the yardstick of the inverse factor) only, nothing imported from bobe_amd.  The kernel, the
Cholesky factorisation and the substitution are tests/zvar_restatement.py's.

Each check takes the INPUTS OF ITS STAGE AS GIVEN - the factor L, the inverse factor Linv, V, V_Z as whoever is judged formed
them - and recomputes that one stage in ``np.longdouble``.  What is left between the two is the rounding of that stage alone,
and for a sum of k products in any order, with or without fused multiply-adds, that is at most gamma_k = k eps / (1 - k eps)
times the sum of the absolute products (eps = 2^-53).  Every check returns the worst ratio of the difference to its bound
(<= 1: within the bound) and where it was found.

  inverse factor   rho = max over the lower triangle of |Linv - inv(L)| / (gamma_N |L^-1| |L| |L^-1|), inv in long double.  A
                   blocked inverse has no componentwise guarantee of its own, so rho is held against the same ratio of
                   ``scipy.linalg.solve_triangular(L, I)``: rho <= 4 rho_ref + 1.
  V, product       |V - Linv k| <= gamma_N |Linv| |k| + |Linv| dk
  V, substitution  per block t of 128 rows |V_t - Linv_tt (k_t - sum_{j<t} L_tj V_j)| <= gamma_N |Linv_tt| (|k_t| + |L_t,<t| |V_<t|)
                   + |Linv_tt| dk_t.  With one block this IS the product.
  crossT           |crossT - V_Z^T V| <= gamma_N |V_Z|^T |V|
  s_c, base_z      |s - (kself - sum v^2)| <= gamma_N sum v^2 + eps kself.  The entry hands out k_predict_finalize's RAW s (its
                   1e-12 floor applies to the predictive variance only, and the scorers floor base_z themselves): a non-finite
                   column gives NaN on both sides, which counts as agreement.

k is the long-double kernel matrix of the same points and dk = c_k eps (1 + |exponent argument|) k the allowance for the
judged side's own float64 evaluation of it (``kernel_allowance``; c_k: tests/sweep_terms_cases.py).
"""
import numpy as np
import scipy.linalg

import zvar_restatement as R

LD = np.longdouble
EPS = LD(2.0) ** -53
ROWS = 128                         # rows of a diagonal block of the substitution (bobe_gp_get_solve_block's default)


def gamma(k):
    return LD(k) * EPS / (LD(1) - LD(k) * EPS)


def ld(a):
    return np.asarray(a, dtype=LD)


def exponent_argument(kind, A, B, ls):
    """|argument of the kernel's exponential|: r^2 / 2 (rbf), sqrt(5) r (Matern-5/2), r^2 from the long-double rbf value."""
    e = R.kernel("rbf", A, B, ls, 1.0, LD)
    r2 = np.maximum(-LD(2) * np.log(e), LD(0))
    return r2 / LD(2) if kind == "rbf" else np.sqrt(LD(5) * r2)


def kernel_truth(kind, A, B, ls, kvar):
    """(k, a): the long-double kernel matrix and (1 + |exponent argument|) k, the allowance's shape."""
    k = R.kernel(kind, A, B, ls, kvar, LD)
    return k, (LD(1) + exponent_argument(kind, A, B, ls)) * np.abs(k)


def kernel_constant_needed(kind, A, B, ls, kvar):
    """The smallest c with |float64 NumPy kernel - long double| <= c eps (1 + |exponent argument|) k everywhere."""
    k, a = kernel_truth(kind, A, B, ls, kvar)
    return float(np.max(np.abs(ld(R.kernel(kind, A, B, ls, kvar, np.float64)) - k) / (EPS * a)))


def kernel_allowance(shape_term, ck):
    return LD(ck) * EPS * shape_term


def _worst(diff, bound):
    """(worst ratio, its index); a bound of 0 admits a difference of 0 only."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff == 0, LD(0), LD(np.inf)))
    ratio = np.where(np.isnan(ratio), LD(np.inf), ratio)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


# ------------------------------------------------------------------------------------------------- the inverse factor
def inverse_truth(L):
    """(inv(L), gamma_N |L^-1| |L| |L^-1|) in long double."""
    Ll = ld(L)
    n = Ll.shape[0]
    inv = R.forward_sub(Ll, np.eye(n, dtype=LD))
    a = np.abs(inv)
    return inv, gamma(n) * (a @ np.abs(Ll) @ a)


def check_inverse(L, Linv):
    """{"rho", "rho_ref", "at": (i, j), "block16": (bi, bj), "block128": (bi, bj), "ok"} of an inverse factor of L; the strict
    upper triangle must be zero."""
    n = L.shape[0]
    inv, bound = inverse_truth(L)
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.all(np.asarray(Linv)[~low] == 0.0), "the inverse factor's strict upper triangle is not zero"

    def rho(M):
        return _worst(np.where(low, np.abs(ld(M) - inv), LD(0)), np.where(low, bound, LD(1)))
    r_dev, at = rho(Linv)
    r_ref, _ = rho(scipy.linalg.solve_triangular(np.asarray(L, dtype=np.float64), np.eye(n), lower=True))
    return {"rho": r_dev, "rho_ref": r_ref, "at": at, "block16": (at[0] // 16, at[1] // 16),
            "block128": (at[0] // 128, at[1] // 128), "ok": bool(r_dev <= 4 * r_ref + 1)}


# ------------------------------------------------------------------------------------------------- V
def check_v_product(Linv, k, dk, V):
    """(worst ratio, (row, column)) of V against Linv k; k [N x n], dk its allowance, both long double."""
    Li = ld(Linv)
    n = Li.shape[0]
    a = np.abs(Li)
    return _worst(np.abs(ld(V) - Li @ k), gamma(n) * (a @ np.abs(k)) + a @ dk)


def check_v_substitution(L, Linv, k, dk, V, rows=ROWS):
    """The same for the blocked substitution: block t against Linv_tt (k_t - L[t, <t] V[<t]), every input the judged side's."""
    Ll, Li, Vl = ld(L), ld(Linv), ld(V)
    n = Ll.shape[0]
    worst, at = 0.0, (0, 0)
    for r0 in range(0, n, rows):
        t = slice(r0, min(n, r0 + rows))
        b = k[t] - Ll[t, :r0] @ Vl[:r0]
        ab = np.abs(k[t]) + np.abs(Ll[t, :r0]) @ np.abs(Vl[:r0])
        a = np.abs(Li[t, t])
        w, (i, j) = _worst(np.abs(Vl[t] - Li[t, t] @ b), gamma(n) * (a @ ab) + a @ dk[t])
        if w >= worst:
            worst, at = w, (r0 + i, j)
    return worst, at


# ------------------------------------------------------------------------------------------------- crossT, s_c, base_z
def check_cross(VZ, V, crossT):
    """(worst ratio, (z, column)) of crossT [M x n] against V_Z^T V."""
    a, b = ld(VZ), ld(V)
    return _worst(np.abs(ld(crossT) - a.T @ b), gamma(a.shape[0]) * (np.abs(a).T @ np.abs(b)))


def check_s(V, kself, s):
    """(worst ratio, (column,)) of s against kself - sum_i V[i, .]^2; NaN where the column is not finite, on both sides."""
    v = ld(V)
    q = np.sum(v * v, axis=0)
    want = LD(kself) - q
    s = ld(s)
    bad = ~np.isfinite(want)
    if np.any(np.isnan(s) != bad):
        return float("inf"), (int(np.argmax(np.isnan(s) != bad)),)
    diff = np.where(bad, LD(0), np.abs(s - np.where(bad, LD(0), want)))
    return _worst(diff, np.where(bad, LD(1), gamma(v.shape[0]) * q + EPS * LD(kself)))


# ------------------------------------------------------------------------------------------------- the float64 stages
def substitute(L, Linv, B, rows=ROWS):
    """V_t = Linv_tt (B_t - L[t, <t] V[<t]) in the arrays' dtype."""
    n = L.shape[0]
    V = np.zeros_like(B)
    for r0 in range(0, n, rows):
        t = slice(r0, min(n, r0 + rows))
        V[t] = Linv[t, t] @ (B[t] - L[t, :r0] @ V[:r0])
    return V


def float64_stages(kind, X, cand, Z, ls, kvar, noise, substitution, cand_is_z=False):
    """The sweep's stages in float64 NumPy, laid out as ``bobe_debug_sweep_terms`` hands them out: {"L", "Linv", "V" [N x C],
    "VZ" [N x M], "crossT" [M x C], "sc" [C], "basez" [M], "substitution"}."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    L = R.cholesky_lower(R.kernel(kind, X, X, ls, kvar, np.float64) + noise * np.eye(n))
    Linv = scipy.linalg.solve_triangular(L, np.eye(n), lower=True)
    return stages_from(L, Linv, R.kernel(kind, X, cand, ls, kvar, np.float64), R.kernel(kind, X, Z, ls, kvar, np.float64),
                       kvar + noise, substitution, cand_is_z)


def stages_from(L, Linv, kxc, kxz, kself, substitution, cand_is_z=False):
    """The stages downstream of a given factor, inverse factor and kernel matrices, in float64."""
    solve = (lambda B: substitute(L, Linv, B)) if substitution else (lambda B: Linv @ B)
    VZ = solve(kxz)
    V = VZ if cand_is_z else solve(kxc)
    return {"L": L, "Linv": Linv, "V": V, "VZ": VZ, "crossT": VZ.T @ V, "sc": kself - np.sum(V * V, axis=0),
            "basez": kself - np.sum(VZ * VZ, axis=0), "substitution": bool(substitution)}


# ------------------------------------------------------------------------------------------------- every stage of one case
def check_stages(t, kind, X, cand, Z, ls, kvar, noise, ck, cols=None):
    """Every Layer A ratio of the terms ``t`` (a dictionary as ``float64_stages`` returns it): {"inverse": check_inverse's
    dictionary, "V", "VZ", "crossT", "sc", "basez": (ratio, where)}.  ``cols``: the candidate columns on which V and crossT
    are judged (all when None; s_c is judged on all of them either way)."""
    cols = np.arange(np.asarray(cand).shape[0]) if cols is None else np.asarray(cols)
    X, cc, Z = np.atleast_2d(X), np.atleast_2d(cand)[cols], np.atleast_2d(Z)
    kself = kvar + noise
    check_v = (lambda k, dk, V: check_v_substitution(t["L"], t["Linv"], k, dk, V)) if t["substitution"] else \
        (lambda k, dk, V: check_v_product(t["Linv"], k, dk, V))
    kz, az = kernel_truth(kind, X, Z, ls, kvar)
    kc, ac = kernel_truth(kind, X, cc, ls, kvar)
    Vc = np.asarray(t["V"])[:, cols]
    wv, atv = check_v(kc, kernel_allowance(ac, ck), Vc)
    wx, atx = check_cross(t["VZ"], Vc, np.asarray(t["crossT"])[:, cols])
    return {"inverse": check_inverse(t["L"], t["Linv"]),
            "V": (wv, (atv[0], int(cols[atv[1]]))),
            "VZ": check_v(kz, kernel_allowance(az, ck), t["VZ"]),
            "crossT": (wx, (atx[0], int(cols[atx[1]]))),
            "sc": check_s(t["V"], kself, t["sc"]),
            "basez": check_s(t["VZ"], kself, t["basez"])}


def stage_ratios(res):
    """{stage: ratio to its bound} with the inverse factor's rho / (4 rho_ref + 1): every entry <= 1 is a pass."""
    out = {k: res[k][0] for k in ("V", "VZ", "crossT", "sc", "basez")}
    out["inverse"] = res["inverse"]["rho"] / (4 * res["inverse"]["rho_ref"] + 1)
    return out


# ------------------------------------------------------------------------------------------------- Layer B's side figures
def r_figures(t, truth, y_std=1.0):
    """(worst |r - r_truth| / max_z |r_truth(c)| over the candidates, worst relative error of s_c, of base_z) of the terms
    ``t`` against the long-double state ``truth`` (zvar_restatement.state); r = (k(z, c) - crossT[z][c]) / sqrt(s_c) with the
    truth's k(z, c), uncapped."""
    kcz, s_t, b_t = truth["kcz"], truth["s"], truth["base"]
    with np.errstate(all="ignore"):
        r_true = LD(y_std) * (kcz - truth["G"].T) / np.sqrt(s_t)[:, None]
        r = LD(y_std) * (kcz - ld(t["crossT"]).T) / np.sqrt(ld(t["sc"]))[:, None]
        dr = np.max(np.abs(r - r_true), axis=1) / np.max(np.abs(r_true), axis=1)
        return (float(np.max(dr)), float(np.max(np.abs(ld(t["sc"]) - s_t) / np.abs(s_t))),
                float(np.max(np.abs(ld(t["basez"]) - b_t) / np.abs(b_t))))


def state_from_stages(t, st64):
    """zvar_restatement's state dictionary with the sweep's terms taken from ``t`` (k(z, c) and mu_z from the float64 state)."""
    return {"kcz": st64["kcz"], "G": np.asarray(t["crossT"], dtype=np.float64), "base": np.asarray(t["basez"], dtype=np.float64),
            "s": np.asarray(t["sc"], dtype=np.float64), "mu": st64["mu"]}
