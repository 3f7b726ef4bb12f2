"""Dense NumPy restatement of the total variance of the evidence estimate (``bobe_gp_evidence_moments``), shared by
tests/test_evidence_moments_cpu.py and tests/test_gpu_evidence_moments.py.  Generic in the dtype (float64, and ``np.longdouble`` -
the truth the device is held to), built on tests/zvar_restatement.py's kernel, Cholesky factorisation and substitutions.
Imports nothing from bobe_amd.

Notation of tests/zvar_restatement.py, physical units.  Z = sum_z e^{l_z} e^{f(z)} over M integration points:

    b_z = y_std^2 (base_z, non-finite / < 1e-12 -> 1e-12)     g_z = l_z + mu_z + b_z / 2     log_ez = logsumexp_z g_z
    lambda_z = g_z - log_ez  (omega = exp(lambda))
    S_zz' = y_std^2 (k(z,z') - V_z . V_z')  (z != z'; non-finite -> 0; |S_zz'| <= sqrt(b_z b_z')),   S_zz = b_z
    T0 = sum_z sum_z' omega_z omega_z' expm1(S_zz')   (all M^2 ordered pairs)     log_t0 = log T0   (T0 <= 0 -> -inf)

Var Z = exp(2 log_ez) T0.  ``log_t0_scaled`` takes no exponent above 0: with h = max_z (lambda_z + b_z / 2), p_z = lambda_z - h,
E_z = exp(p_z), a pair with |S| < 1 adds E_z E_z' expm1(S), any other exp(p_z + p_z' + S) - E_z E_z', and log_t0 = 2 h + log sum.

  state              (mu, base, cov) of a GP on (X, ys) at Z in the given dtype (standardised units)
  z_weights          (lambda, b, log_ez): ``zvar_restatement.z_weights``
  pair_matrix        S [M x M] in physical units under the rules
  log_t0_scaled      log T0 from (lambda, b, S), in row blocks; ``weights`` [M x M] multiplies the ordered pairs' terms
  evidence_moments   {"log_ez", "log_t0"} from a state
  direct_var         the unscaled sum_z sum_z' A_z A_z' expm1(cov_zz') (benign cases only)
"""
import numpy as np

import zvar_restatement as R


def state(kind, X, ys, Z, ls, kvar, noise, dtype=np.float64):
    """mu_z and base_z as ``zvar_restatement.state`` forms them, and cov = k(Z,Z) - V_Z^T V_Z (its diagonal is not used)."""
    X, Z = (np.atleast_2d(np.asarray(a, dtype=dtype)) for a in (X, Z))
    K = R.kernel(kind, X, X, ls, kvar, dtype) + dtype(noise) * np.eye(X.shape[0], dtype=dtype)
    L = R.cholesky_lower(K)
    kxz = R.kernel(kind, X, Z, ls, kvar, dtype)
    VZ = R.forward_sub(L, kxz)
    alpha = R.back_sub(L, R.forward_sub(L, np.asarray(ys, dtype=dtype).reshape(-1)))
    kself = dtype(kvar) + dtype(noise)
    return {"mu": kxz.T @ alpha, "base": kself - np.sum(VZ * VZ, axis=0),
            "cov": R.kernel(kind, Z, Z, ls, kvar, dtype) - VZ.T @ VZ, "noise": dtype(noise)}


z_weights = R.z_weights


def pair_matrix(cov, b, y_std, capped=True):
    """S in physical units: y_std^2 cov off the diagonal (non-finite -> 0, |S| <= sqrt(b b') when ``capped``), b on it."""
    dt = b.dtype.type
    with np.errstate(all="ignore"):
        S = dt(y_std) ** 2 * np.asarray(cov, dtype=dt)
    S = np.where(np.isfinite(S), S, dt(0))
    if capped:
        cap = np.sqrt(b[:, None] * b[None, :])
        S = np.clip(S, -cap, cap)
    S = np.array(S)
    S[np.diag_indices_from(S)] = b
    return S


def log_t0_scaled(lam, b, S, weights=None, block=64):
    """2 h + log sum over the ordered pairs, in row blocks; -inf when the sum is <= 0, NaN when it is NaN."""
    dt = b.dtype.type
    h = np.max(lam + b / dt(2))
    if h != h:
        return h
    p = lam - h
    E = np.exp(p)
    tot = dt(0)
    for r0 in range(0, len(lam), block):
        sl = slice(r0, r0 + block)
        x = S[sl]
        ee = E[sl, None] * E[None, :]
        pp = p[sl, None] + p[None, :]
        small = np.abs(x) < 1
        with np.errstate(all="ignore"):
            term = np.where(small, ee * np.expm1(np.where(small, x, dt(0))), np.exp(np.where(small, dt(0), pp + x)) - ee)
        if weights is not None:
            term = term * np.asarray(weights[sl], dtype=dt)
        tot = tot + np.sum(term)
    if tot > 0:
        return dt(2) * h + np.log(tot)
    return dt(-np.inf) if tot <= 0 else tot


def evidence_moments(st, y_std, log_weights=None, capped=True, weights=None):
    lam, b, log_ez = z_weights(st, y_std, log_weights)
    S = pair_matrix(st["cov"], b, y_std, capped)
    return {"log_ez": log_ez, "log_t0": log_t0_scaled(lam, b, S, weights)}


def direct_var(mu, cov_phys, logw):
    """Var Z = sum_z sum_z' A_z A_z' expm1(cov_zz'), A_z = exp(l_z + mu_z + cov_zz / 2): the lognormal's own formula, unscaled."""
    A = np.exp(logw + mu + np.diag(cov_phys) / 2)
    return float(A @ np.expm1(cov_phys) @ A), float(np.sum(A))
