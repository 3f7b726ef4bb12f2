"""Dense SciPy restatement of the importance-weighted sweep scores (``bobe_gp_wip_sweep_w``) and of their believer stages
(``bobe_gp_wip_select_batch_w``), shared by tests/test_weighted_criteria_cpu.py and tests/test_gpu_weighted_criteria.py.
Imports nothing from bobe_amd.

For candidate c and integration point z, in the standardised units of the training targets ys = (y - y_mean) / y_std:

    L = chol(K(X, X) + noise I)     V = L^-1 K(X, C)     V_Z = L^-1 K(X, Z)     alpha = K^-1 ys
    s_c = kvar + noise - |V[:, c]|^2        base_z = kvar + noise - |V_Z[:, z]|^2       cross = k(c, z) - V_Z[:, z] . V[:, c]
    v+(z | c) = (base_z - cross^2 / s_c  -> NaN / < 1e-12 -> 1e-12) * y_std^2
    b_z = y_std^2 * (base_z, non-finite / < 1e-12 -> 1e-12)      mu_z = y_std * (K(X, Z)^T alpha)_z      (no y_mean)
    l_z = log-weight of z (None: -mu_z)      a_z = l_z + mu_z      omega = softmax(a)      u = Phi^-1(3/4)

    wipv   = sum_z omega_z v+                      wipstd = sum_z omega_z sqrt(v+)
    imiqr  = logsumexp_z [a_z + log(2 sinh(u sqrt(v+)))]
    eiv    = -logsumexp_z [l_z + 2 mu_z + 2 b_z - v+]        log_s = logsumexp_z [l_z + 2 mu_z + 2 b_z]

  dense_state     (kcz, G, base, s, mu) of a GP on (X, ys) by factorisation
  weighted_scores the five quantities above from a state
  literal_batch   the believer stages by LITERAL refactorisation of the (N + j)-point GP, y_mean / y_std held fixed
  rank_one_batch  the same stages by the rank-one recursion of tests/batch_select_restatement.py
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular
from scipy.special import logsumexp

from batch_select_restatement import FLOOR, kernel, masked_argmin

U = 0.6744897501960817
KEYS = ("wipv", "wipstd", "imiqr", "eiv")


def dense_state(kind, X, ys, cand, Z, ls, kvar, noise):
    X, cand, Z = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (X, cand, Z))
    K = kernel(kind, X, X, ls, kvar) + noise * np.eye(X.shape[0])
    L = cholesky(K, lower=True)
    kxz = kernel(kind, X, Z, ls, kvar)
    V = solve_triangular(L, kernel(kind, X, cand, ls, kvar), lower=True, check_finite=False)
    VZ = solve_triangular(L, kxz, lower=True, check_finite=False)
    kself = kvar + noise
    alpha = cho_solve((L, True), np.asarray(ys, dtype=np.float64).reshape(-1))
    return {"kcz": kernel(kind, cand, Z, ls, kvar), "G": VZ.T @ V, "base": kself - np.sum(VZ * VZ, axis=0),
            "s": kself - np.sum(V * V, axis=0), "mu": kxz.T @ alpha, "V": V, "VZ": VZ}


def fantasy_var(st, y_std):
    """v+ [C x M] in physical units, the scorer's rules (gp.py:574-576)."""
    cross = st["kcz"] - st["G"].T
    with np.errstate(all="ignore"):
        var = st["base"][None, :] - cross * cross / st["s"][:, None]
    var = np.where(st["s"][:, None] >= 0, var, np.nan)
    var = np.where(np.isnan(var), FLOOR, var)
    var = np.where(var < FLOOR, FLOOR, var)
    return var * y_std ** 2


def z_terms(st, y_std, log_weights):
    """(mu, l, a, omega, e = l + 2 mu + 2 b) of the integration points."""
    mu = y_std * st["mu"]
    ell = -mu if log_weights is None else np.asarray(log_weights, dtype=np.float64)
    a = ell + mu
    omega = np.exp(a - logsumexp(a))
    base = st["base"]
    b = np.where(np.isfinite(base) & (base >= FLOOR), base, FLOOR) * y_std ** 2
    return mu, ell, a, omega, ell + 2.0 * mu + 2.0 * b


def weighted_scores(st, y_std, log_weights=None):
    v = fantasy_var(st, y_std)
    mu, ell, a, omega, e = z_terms(st, y_std, log_weights)
    x = U * np.sqrt(v)
    return {"wipv": v @ omega, "wipstd": np.sqrt(v) @ omega,
            "imiqr": logsumexp(a[None, :] + x + np.log1p(-np.exp(-2.0 * x)), axis=1),
            "eiv": -logsumexp(e[None, :] - v, axis=1), "log_s": float(logsumexp(e))}


def two_best_gap(scores, taken=()):
    """Absolute gap between the two smallest scores over the indices not in ``taken``."""
    v = np.array(scores, dtype=np.float64)
    v[list(taken)] = np.inf
    a, b = np.partition(v, 1)[:2]
    return b - a


def literal_batch(kind, X, ys, cand, Z, ls, kvar, noise, y_std, log_weights, n_batch, key):
    """Believer stages by refactorising the (N + j)-point GP: the pick joins X at its predicted (standardised) mean, y_mean
    and y_std stay.  The weights' a_z and omega are the first stage's (mu_z does not move under a believer append; asserted).
    Returns (picks, stage_scores [n_batch x C], gaps [n_batch])."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    ys = np.asarray(ys, dtype=np.float64).reshape(-1)
    cand = np.atleast_2d(np.asarray(cand, dtype=np.float64))
    picks, stages, gaps, mu0 = [], [], [], None
    for j in range(n_batch):
        st = dense_state(kind, X, ys, cand, Z, ls, kvar, noise)
        if mu0 is None:
            mu0 = st["mu"]
        assert np.max(np.abs(st["mu"] - mu0)) <= 1e-6 * (1.0 + np.max(np.abs(mu0))), "believer append moved the mean"
        st["mu"] = mu0
        sc = weighted_scores(st, y_std, log_weights)[key]
        stages.append(sc)
        gaps.append(two_best_gap(sc, picks))
        p = masked_argmin(sc, picks)
        picks.append(p)
        if j + 1 < n_batch:
            K = kernel(kind, X, X, ls, kvar) + noise * np.eye(X.shape[0])
            mean_p = kernel(kind, X, cand[p][None, :], ls, kvar)[:, 0] @ np.linalg.solve(K, ys)
            X = np.vstack([X, cand[p][None, :]])
            ys = np.append(ys, mean_p)
    return np.array(picks, dtype=np.int64), np.array(stages), np.array(gaps)


def rank_one_batch(kind, X, ys, cand, Z, ls, kvar, noise, y_std, log_weights, n_batch, key):
    """The same stages by rank-one downdates of (G, base, s), mu fixed.  Returns (picks, stage_scores)."""
    cand = np.atleast_2d(np.asarray(cand, dtype=np.float64))
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    st = dense_state(kind, X, ys, cand, Z, ls, kvar, noise)
    V, VZ = st["V"], st["VZ"]
    picks, stages, UC, UZ = [], [], [], []
    for j in range(n_batch):
        if j > 0:
            p = picks[-1]
            xs = cand[p][None, :]
            uc = kernel(kind, cand, xs, ls, kvar)[:, 0] - V.T @ V[:, p]
            uz = kernel(kind, Z, xs, ls, kvar)[:, 0] - VZ.T @ V[:, p]
            for pc, pz in zip(UC, UZ):
                uc = uc - pc * pc[p]
                uz = uz - pz * pc[p]
            uc, uz = uc / np.sqrt(st["s"][p]), uz / np.sqrt(st["s"][p])
            st["G"] = st["G"] + np.outer(uz, uc)
            st["base"] = st["base"] - uz * uz
            st["s"] = st["s"] - uc * uc
            UC.append(uc)
            UZ.append(uz)
        sc = weighted_scores(st, y_std, log_weights)[key]
        stages.append(sc)
        picks.append(masked_argmin(sc, picks))
    return np.array(picks, dtype=np.int64), np.array(stages)
