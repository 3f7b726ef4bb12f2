"""Dense NumPy restatement of the evidence-variance sweep score (``bobe_gp_wip_sweep_zvar``) and of its believer stages
(``bobe_gp_wip_select_batch_zvar``), shared by tests/test_zvar_cpu.py and tests/test_gpu_zvar.py.  Generic in the dtype: float64
builds on ``weighted_criteria_restatement.dense_state`` (SciPy's factorisation), ``np.longdouble`` - the truth the device is
held to - on a Cholesky factorisation and substitutions of its own.  Imports nothing from bobe_amd.

Notation of tests/weighted_criteria_restatement.py, physical units.  Z = sum_z e^{l_z} e^{f(z)}:

    b_z = y_std^2 (base_z, non-finite / < 1e-12 -> 1e-12)     g_z = l_z + mu_z + b_z / 2     log_ez = logsumexp_z g_z
    lambda_z = g_z - log_ez  (omega = exp(lambda))            r_z(c) = y_std cross_z / sqrt(s_c)
    |r_z| <= sqrt(b_z);  cross_z non-finite -> r_z = 0;  s_c not > 0 -> every r_z = 0
    T(c) = sum_z sum_z' omega_z omega_z' expm1(r_z r_z')      zvar = -log T   (T <= 0 -> +inf)

An observation at c moves mu_z by r_z xi, xi ~ N(0, 1), and lowers b_z by r_z^2, so E_xi[Var+ Z] = Var Z - exp(2 log_ez) T(c).
``zvar_scores`` takes no exponent above 0: with h_c = max_z (lambda_z + r_z^2 / 2), p_z = lambda_z - h_c, E_z = exp(p_z), a pair
with |r r'| < 1 adds E_z E_z' expm1(r r'), any other exp(p_z + p_z' + r r') - E_z E_z', and zvar = -(2 h_c + log sum).

  state               (kcz, G, base, s, mu) of a GP on (X, ys) in the given dtype
  zvar_scores         {"zvar": [C], "log_ez": float, "T_scaled", "h"} from a state
  literal_batch_zvar  the believer stages by LITERAL refactorisation of the (N + j)-point GP, mu_z held
"""
import numpy as np

import weighted_criteria_restatement as W
from batch_select_restatement import FLOOR, masked_argmin


def kernel(kind, A, B, ls, kvar, dtype):
    """``batch_select_restatement.kernel`` in ``dtype``."""
    ls = np.asarray(ls, dtype=dtype)
    a, b = np.asarray(A, dtype=dtype) / ls, np.asarray(B, dtype=dtype) / ls
    r2 = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    for j in range(a.shape[1]):
        df = a[:, j][:, None] - b[:, j][None, :]
        r2 += df * df
    kvar = dtype(kvar)
    if kind == "rbf":
        return kvar * np.exp(-r2 / dtype(2))
    s5 = np.sqrt(dtype(5))
    dd = np.sqrt(np.where(r2 < dtype(1e-30), dtype(1e-30), r2))
    return kvar * (dtype(1) + dd * (s5 + dd * dtype(5) / dtype(3))) * np.exp(-s5 * dd)


def cholesky_lower(K):
    """Lower Cholesky factor, column by column, in K's dtype."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        v = K[j:, j] - L[j:, :j] @ L[j, :j]
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def forward_sub(L, B):
    B = np.array(B, dtype=L.dtype)
    B2 = B.reshape(B.shape[0], -1)
    for i in range(L.shape[0]):
        B2[i] = (B2[i] - L[i, :i] @ B2[:i]) / L[i, i]
    return B2.reshape(B.shape)


def back_sub(L, B):
    """Solves L^T x = B."""
    B = np.array(B, dtype=L.dtype)
    B2 = B.reshape(B.shape[0], -1)
    for i in range(L.shape[0] - 1, -1, -1):
        B2[i] = (B2[i] - L[i + 1:, i] @ B2[i + 1:]) / L[i, i]
    return B2.reshape(B.shape)


def state(kind, X, ys, cand, Z, ls, kvar, noise, dtype=np.float64):
    """``dense_state``'s dictionary (plus alpha) in ``dtype``; float64 IS ``dense_state``."""
    if dtype is np.float64:
        st = W.dense_state(kind, X, ys, cand, Z, ls, kvar, noise)
        return {k: st[k] for k in ("kcz", "G", "base", "s", "mu")}
    X, cand, Z = (np.atleast_2d(np.asarray(a, dtype=dtype)) for a in (X, cand, Z))
    K = kernel(kind, X, X, ls, kvar, dtype) + dtype(noise) * np.eye(X.shape[0], dtype=dtype)
    L = cholesky_lower(K)
    kxz = kernel(kind, X, Z, ls, kvar, dtype)
    V = forward_sub(L, kernel(kind, X, cand, ls, kvar, dtype))
    VZ = forward_sub(L, kxz)
    kself = dtype(kvar) + dtype(noise)
    alpha = back_sub(L, forward_sub(L, np.asarray(ys, dtype=dtype).reshape(-1)))
    return {"kcz": kernel(kind, cand, Z, ls, kvar, dtype), "G": VZ.T @ V, "base": kself - np.sum(VZ * VZ, axis=0),
            "s": kself - np.sum(V * V, axis=0), "mu": kxz.T @ alpha, "alpha": alpha}


def lse(v):
    m = np.max(v)
    return m + np.log(np.sum(np.exp(v - m)))


def z_weights(st, y_std, log_weights):
    """(lambda, b, log_ez) in the state's dtype."""
    dt = st["base"].dtype.type
    y_std = dt(y_std)
    mu = y_std * st["mu"]
    ell = -mu if log_weights is None else np.asarray(log_weights, dtype=dt)
    base = st["base"]
    b = np.where(np.isfinite(base) & (base >= dt(FLOOR)), base, dt(FLOOR)) * y_std ** 2
    g = (ell + mu) + b / dt(2)
    log_ez = lse(g)
    return g - log_ez, b, log_ez


def r_terms(st, y_std, b, capped=True):
    """r [C x M] under the edge rules."""
    dt = st["base"].dtype.type
    cross = st["kcz"] - st["G"].T
    s = st["s"]
    with np.errstate(all="ignore"):
        r = dt(y_std) * cross / np.sqrt(s)[:, None]
    r = np.where(np.isfinite(cross), r, dt(0))
    r = np.where((s > 0)[:, None], r, dt(0))
    if capped:
        cap = np.sqrt(b)[None, :]
        r = np.clip(r, -cap, cap)
    return r


def zvar_scores(st, y_std, log_weights=None, block=32):
    dt = st["base"].dtype.type
    lam, b, log_ez = z_weights(st, y_std, log_weights)
    r = r_terms(st, y_std, b)
    h = np.max(lam[None, :] + r * r / dt(2), axis=1)
    p = lam[None, :] - h[:, None]
    E = np.exp(p)
    tot = np.zeros(r.shape[0], dtype=dt)
    for c0 in range(0, r.shape[0], block):
        sl = slice(c0, c0 + block)
        x = r[sl, :, None] * r[sl, None, :]
        ee = E[sl, :, None] * E[sl, None, :]
        pp = p[sl, :, None] + p[sl, None, :]
        small = np.abs(x) < 1
        with np.errstate(all="ignore"):
            term = np.where(small, ee * np.expm1(np.where(small, x, dt(0))), np.exp(np.where(small, dt(0), pp + x)) - ee)
        tot[sl] = np.sum(term, axis=(1, 2))
    with np.errstate(all="ignore"):
        zvar = np.where(tot > 0, -(dt(2) * h + np.log(np.where(tot > 0, tot, dt(1)))), np.where(tot <= 0, dt(np.inf), tot))
    return {"zvar": zvar, "log_ez": log_ez, "T_scaled": tot, "h": h}


def literal_batch_zvar(kind, X, ys, cand, Z, ls, kvar, noise, y_std, log_weights, n_batch, dtype=np.float64):
    """Believer stages by refactorising the (N + j)-point GP in ``dtype``: the pick joins X at its predicted (standardised)
    mean; y_mean, y_std and mu_z stay (mu_z does not move under a believer append; asserted).  omega's b_z part and the cap
    follow the refit's base_z.  Returns (picks, stage_scores [n_batch x C], gaps [n_batch])."""
    X = np.atleast_2d(np.asarray(X, dtype=dtype))
    ys = np.asarray(ys, dtype=dtype).reshape(-1)
    cand = np.atleast_2d(np.asarray(cand, dtype=dtype))
    picks, stages, gaps, mu0 = [], [], [], None
    for j in range(n_batch):
        st = state(kind, X, ys, cand, Z, ls, kvar, noise, dtype)
        if mu0 is None:
            mu0 = st["mu"]
        assert np.max(np.abs(st["mu"] - mu0)) <= 1e-6 * (1.0 + np.max(np.abs(mu0))), "believer append moved the mean"
        st["mu"] = mu0
        sc = zvar_scores(st, y_std, log_weights)["zvar"]
        stages.append(sc)
        gaps.append(W.two_best_gap(sc, picks))
        p = masked_argmin(sc, picks)
        picks.append(p)
        if j + 1 < n_batch:
            kp = kernel(kind, X, cand[p][None, :], ls, kvar, dtype)[:, 0]
            if dtype is np.float64:
                K = kernel(kind, X, X, ls, kvar, dtype) + noise * np.eye(X.shape[0])
                mean_p = kp @ np.linalg.solve(K, ys)
            else:
                mean_p = kp @ st["alpha"]
            X = np.vstack([X, cand[p][None, :]])
            ys = np.append(ys, mean_p)
    return np.array(picks, dtype=np.int64), np.array(stages), np.array(gaps, dtype=np.float64)
