"""Analytic posterior mean and variance with their input gradients (``bobe_gp_predict_grad``) and the leapfrog recurrence of
``bobe_gp_hmc_leapfrog``, stated once and generic in the dtype; shared by tests/test_posterior_grad_cpu.py and
tests/test_gpu_posterior_grad.py.  Imports nothing from bobe_amd.

  np.float64     LAPACK (``cholesky`` / ``cho_solve`` / ``solve_triangular``), the variance from the half-solved vectors
                 V = L^-1 k as ``weighted_grad_restatement.State.candidate`` forms it: the restatement whose own error sets
                 the scale of the rule
  np.longdouble  ``_kernel_ld`` / ``_chol_ld`` / ``_solve_ld`` of tests/paths_restatement.py: the truth

Standardised units, ys = (y - mean) / std, K = k(X, X) + noise I, alpha = K^-1 ys, for a query q with k = k(X, q):

    mean  = k . alpha                         dmean / dq_j = sum_n alpha_n dk(q, X_n) / dq_j
    var   = kvar + noise - k . K^-1 k         dvar / dq_j  = -2 sum_n (K^-1 k)_n dk(q, X_n) / dq_j
    dk(q, p) / dq_j = G(q, p) (p_j - q_j) / ls_j^2,   G = dk / d(-r^2 / 2)  (``weighted_grad_restatement._grad_factor``)

floored = not (var >= 1e-12): there var = 1e-12 and dvar = 0 (k_predict_grad's ``floored``, the gradient of jnp.where).

The leapfrog (the comment above k_hmc_leapfrog), on u = logit(x), one alpha per call:

    x = 1 / (1 + e^-u)        logp = (mean(x) y_std + y_mean) / temp + sum_j [log x_j + log1p(-x_j)]
    g = dmean / dx  y_std / temp  x (1 - x) + (1 - 2 x)
    per step: u += eps inv_mass p;  evaluate;  p += (eps | eps / 2 on the last step) g

without the kernel's clip of x to [1e-12, 1 - 1e-12]: |u| <= 27 keeps it idle.
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

from paths_restatement import _chol_ld, _solve_ld
from weighted_grad_restatement import _grad_factor, _kernel

FLOOR = 1e-12


def dk_dq(kind, q, P, ls, kvar, dtype):
    """d k(q, P_n) / dq_j  [len(P) x d]"""
    g, dif = _grad_factor(kind, q, P, ls, kvar, dtype)
    return g[:, None] * dif / np.asarray(ls, dtype=dtype)[None, :]


def _gram(kind, X, ls, kvar, noise, dtype):
    K = _kernel(kind, X, X, ls, kvar, dtype)
    K[np.diag_indices_from(K)] += dtype(noise)
    return K


def solve_alpha(kind, X, ys, ls, kvar, noise, dtype):
    """alpha = K^-1 ys"""
    K = _gram(kind, X, ls, kvar, noise, dtype)
    rhs = np.asarray(ys, dtype=dtype)
    if dtype is np.longdouble:
        return _solve_ld(_chol_ld(K), rhs[:, None])[:, 0]
    return cho_solve((cholesky(K, lower=True), True), rhs)


def mean_and_grad(kind, X, alpha, Q, ls, kvar, dtype):
    """(mean [C], dmean [C x d]) from the coefficients alone - what k_predict_grad's mean-only mode and the chain kernels sum"""
    D = dtype
    Q = np.atleast_2d(np.asarray(Q, dtype=D))
    mean = _kernel(kind, X, Q, ls, kvar, D).T @ alpha
    dmean = np.stack([alpha @ dk_dq(kind, Q[c], X, ls, kvar, D) for c in range(len(Q))])
    return mean, dmean


def posterior_and_grad(kind, X, ys, Q, ls, kvar, noise, dtype=np.float64):
    """(mean [C], var [C], dmean [C x d], dvar [C x d], floored [C] bool) at the rows of Q, all in ``dtype``"""
    D = dtype
    Q = np.atleast_2d(np.asarray(Q, dtype=D))
    C = len(Q)
    K = _gram(kind, X, ls, kvar, noise, D)
    kq = _kernel(kind, X, Q, ls, kvar, D)                                  # [N x C]
    kself = D(kvar) + D(noise)
    if D is np.longdouble:
        sol = _solve_ld(_chol_ld(K), np.concatenate([kq, np.asarray(ys, dtype=D).reshape(-1, 1)], axis=1))
        u, alpha = sol[:, :-1], sol[:, -1]
        var = kself - np.sum(kq * u, axis=0)
    else:
        L = cholesky(K, lower=True)
        alpha = cho_solve((L, True), np.asarray(ys, dtype=D))
        V = solve_triangular(L, kq, lower=True, check_finite=False)
        u = solve_triangular(L.T, V, lower=False, check_finite=False)
        var = kself - np.sum(V * V, axis=0)
    mean = kq.T @ alpha
    dmean, dvar = np.zeros((C, Q.shape[1]), dtype=D), np.zeros((C, Q.shape[1]), dtype=D)
    for c in range(C):
        dk = dk_dq(kind, Q[c], X, ls, kvar, D)
        dmean[c] = alpha @ dk
        dvar[c] = -D(2.0) * (u[:, c] @ dk)
    floored = ~(var >= D(FLOOR))
    return mean, np.where(floored, D(FLOOR), var), dmean, np.where(floored[:, None], D(0.0), dvar), floored


def leapfrog(kind, X, ys, ls, kvar, noise, y_mean, y_std, U, Pm, inv_mass, eps, L, temp, dtype=np.float64):
    """L leapfrog steps of the chains (U, Pm) [P x d]: (U', Pm', logp [P], grad [P x d], mean_phys [P], X' [P x d])"""
    D = dtype
    alpha = solve_alpha(kind, X, ys, ls, kvar, noise, D)
    u, p = np.array(U, dtype=D), np.array(Pm, dtype=D)
    im, eps, temp, y_mean, y_std = np.asarray(inv_mass, dtype=D), D(eps), D(temp), D(y_mean), D(y_std)
    logp = g = mean = x = None
    for s in range(int(L)):
        u = u + eps * im[None, :] * p
        x = D(1.0) / (D(1.0) + np.exp(-u))
        m, dm = mean_and_grad(kind, X, alpha, x, ls, kvar, D)
        mean = m * y_std + y_mean
        logp = mean / temp + np.sum(np.log(x) + np.log1p(-x), axis=1)
        g = dm * y_std / temp * (x * (D(1.0) - x)) + (D(1.0) - D(2.0) * x)
        p = p + (eps if s < L - 1 else D(0.5) * eps) * g
    return u, p, logp, g, mean, x
