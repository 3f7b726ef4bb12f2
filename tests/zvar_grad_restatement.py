"""Value and input gradient of the evidence-variance score (``bobe_gp_wip_grad_zvar``), stated once and generic in the dtype;
shared by tests/test_zvar_grad_cpu.py and tests/test_gpu_zvar_grad.py.  ``np.float64`` is the reference whose own error sets
the scale, ``np.longdouble`` the truth.  Built on tests/zvar_restatement.py (``state`` / ``z_weights`` / ``r_terms`` /
``zvar_scores``); imports nothing from bobe_amd.

Notation of tests/zvar_restatement.py, physical units, no y_mean.  omega_z = exp(lambda_z) and b_z do not depend on the
candidate; r_z(c) = y_std cross_z / sqrt(s_c); h_c = max_z (lambda_z + r_z^2 / 2), p_z = lambda_z - h_c, T_s the scaled pair
sum of ``zvar_scores`` (zvar = -(2 h_c + log T_s)).  With

    G_z = sum_z' r_z' exp(p_z + p_z' + r_z r_z')          (every exponent <= 0, the diagonal included)

    d zvar / dx_j = sum_z rho_z d r_z / dx_j,             rho_z = -2 G_z / T_s
    d r_z / dx_j = w1 d cross_z / dx_j + w2_z d s / dx_j,   w1 = y_std / sqrt(s),   w2_z = -r_z / (2 s)
    d cross_z / dx_j = d k(x, z) / dx_j - sum_n W[n][z] d k(x, X_n) / dx_j,      d s / dx_j = -2 sum_n u_n d k(x, X_n) / dx_j
    d k(x, p) / dx_j = Gk(x, p) (p_j - x_j) / ls_j^2      (W = K^-1 K(X, Z), u = K^-1 k(X, x); tests/weighted_grad_restatement.py)

Edge rules, "gradient of where": a z whose r_z was cut to its cap +-sqrt(b_z), or whose cross is not finite, is a constant - it
keeps its value in T and in G and has rho_z = 0; a candidate whose s is not > 0, or whose T <= 0, has zvar = +inf and a zero
gradient.

  grad_state      ``zvar_restatement.state``'s dictionary plus "dcross" [C x M x d] and "ds" [C x d]
  value_and_grad  {"zvar" [C], "dzvar" [C x d], "rho" [C x M], "const" [C x M], "T_scaled" [C], "log_ez"} from such a state
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

import zvar_restatement as R
from weighted_grad_restatement import _grad_factor


def grad_state(kind, X, ys, cand, Z, ls, kvar, noise, dtype=np.float64):
    """The fields of ``zvar_restatement.state`` (float64: SciPy's factorisation, the same bits) and the input derivatives of
    cross and s for every candidate, from ONE factorisation."""
    D = dtype
    X, cand, Z = (np.atleast_2d(np.asarray(a, dtype=D)) for a in (X, cand, Z))
    ls = np.asarray(ls, dtype=D)
    K = R.kernel(kind, X, X, ls, kvar, D) + D(noise) * np.eye(X.shape[0], dtype=D)
    kxz, kxc = R.kernel(kind, X, Z, ls, kvar, D), R.kernel(kind, X, cand, ls, kvar, D)
    yv = np.asarray(ys, dtype=D).reshape(-1)
    if D is np.float64:
        L = cholesky(K, lower=True)
        V = solve_triangular(L, kxc, lower=True, check_finite=False)
        VZ = solve_triangular(L, kxz, lower=True, check_finite=False)
        alpha = cho_solve((L, True), yv)
        U = solve_triangular(L.T, V, lower=False, check_finite=False)
        Wz = solve_triangular(L.T, VZ, lower=False, check_finite=False)
    else:
        L = R.cholesky_lower(K)
        V, VZ = R.forward_sub(L, kxc), R.forward_sub(L, kxz)
        alpha = R.back_sub(L, R.forward_sub(L, yv))
        U, Wz = R.back_sub(L, V), R.back_sub(L, VZ)
    kself = D(kvar) + D(noise)
    C, M, d = cand.shape[0], Z.shape[0], cand.shape[1]
    dcross, ds = np.zeros((C, M, d), dtype=D), np.zeros((C, d), dtype=D)
    for c in range(C):
        gn, dn = _grad_factor(kind, cand[c], X, ls, kvar, D)
        gz, dz = _grad_factor(kind, cand[c], Z, ls, kvar, D)
        dk_n = gn[:, None] * dn / ls[None, :]
        dcross[c] = gz[:, None] * dz / ls[None, :] - Wz.T @ dk_n
        ds[c] = -D(2) * (U[:, c] @ dk_n)
    return {"kcz": R.kernel(kind, cand, Z, ls, kvar, D), "G": VZ.T @ V, "base": kself - np.sum(VZ * VZ, axis=0),
            "s": kself - np.sum(V * V, axis=0), "mu": kxz.T @ alpha, "dcross": dcross, "ds": ds}


def value_and_grad(st, y_std, log_weights=None):
    """Everything in the state's dtype."""
    D = st["base"].dtype.type
    sc = R.zvar_scores(st, y_std, log_weights)
    lam, b, log_ez = R.z_weights(st, y_std, log_weights)
    r, r_free = R.r_terms(st, y_std, b), R.r_terms(st, y_std, b, capped=False)
    s, cross = st["s"], st["kcz"] - st["G"].T
    alive = s > 0
    const = (r != r_free) | ~np.isfinite(cross) | ~alive[:, None]
    p = lam[None, :] - sc["h"][:, None]
    tot = sc["T_scaled"]
    good = alive & (tot > 0)
    C, M = r.shape
    rho = np.zeros((C, M), dtype=D)
    dz = np.zeros((C, st["ds"].shape[1]), dtype=D)
    for c in np.nonzero(good)[0]:
        ex = np.exp(p[c][:, None] + p[c][None, :] + r[c][:, None] * r[c][None, :])
        Gz = ex @ r[c]
        rho[c] = np.where(const[c], D(0), -D(2) * Gz / tot[c])
        w1, w2 = D(y_std) / np.sqrt(s[c]), -r[c] / (D(2) * s[c])
        dz[c] = (rho[c] * w1) @ st["dcross"][c] + np.sum(rho[c] * w2) * st["ds"][c]
    with np.errstate(all="ignore"):
        zvar = np.where(good, sc["zvar"], D(np.inf))
    return {"zvar": zvar, "dzvar": dz, "rho": rho, "const": const, "T_scaled": tot, "log_ez": log_ez}
