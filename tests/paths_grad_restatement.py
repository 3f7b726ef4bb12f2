"""NumPy restatements shared by tests/test_paths_grad_cpu.py and tests/test_gpu_paths_grad.py: value and input gradient of a
posterior path per (point, path index) - bobe_gp_paths_grad, include/bobe_gp.h - in fp64 with the conditioning weights by
SciPy's ``cho_solve`` (as ``paths_fp64``) and in ``np.longdouble`` with the weights of ``TruthLD.v`` (the truth of the tests).
Standardised units:  xs = x / ls,  c_n = v_s[n] (centred: v_s[n] - alpha_n),  arg_j = u_j . xs + b_j,  amp = sqrt(2 kvar / F),
    f   = sum_n c_n k(r2_n) + amp sum_j w_sj cos(arg_j)
    df_k = (1 / ls_k) [ sum_n c_n G(r2_n) (xs_nk - xs_k) - amp sum_j w_sj sin(arg_j) u_jk ]
with G = k (RBF) or kvar (5/3) (1 + sqrt5 r) exp(-sqrt5 r) (Matern-5/2)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from paths_restatement import TruthLD, _solve_ld, features
from posterior_restatement import kernel


def _value_and_grad(kind, X, Q, ls, kvar, coef, u, phase, wsel, dtype):
    """coef (T x N): the kernel coefficients of every point's path; wsel (T x F): its feature weights"""
    D = dtype
    ls = np.asarray(ls, dtype=D)
    Xs, Qs = np.asarray(X, dtype=D) / ls, np.asarray(Q, dtype=D) / ls
    u, phase, coef, wsel = (np.asarray(a, dtype=D) for a in (u, phase, coef, wsel))
    diff = Xs[None, :, :] - Qs[:, None, :]                         # (T, N, d): xs_n - xs
    r2 = np.zeros(diff.shape[:2], dtype=D)
    for k in range(diff.shape[2]):
        r2 += diff[:, :, k] * diff[:, :, k]
    if kind == "rbf":
        kv = D(kvar) * np.exp(-D(0.5) * r2)
        gf = kv
    else:
        s5, r = np.sqrt(D(5.0)), np.sqrt(r2)
        e = np.exp(-s5 * r)
        kv = D(kvar) * (D(1.0) + s5 * r + D(5.0) / D(3.0) * r2) * e
        gf = D(kvar) * (D(5.0) / D(3.0)) * (D(1.0) + s5 * r) * e
    amp = np.sqrt(D(2.0) * D(kvar) / D(u.shape[0]))
    arg = Qs @ u.T + phase[None, :]                                # (T, F)
    f = np.sum(coef * kv, axis=1) + amp * np.sum(wsel * np.cos(arg), axis=1)
    g = np.einsum("tn,tnk->tk", coef * gf, diff) - amp * ((wsel * np.sin(arg)) @ u)
    return f, g / ls[None, :]


def value_and_grad_fp64(kind, X, y, Q, path_idx, ls, kvar, noise, u, phase, w, eps, centered=False):
    """(f (T,), df (T, d)) in fp64, the weights by cho_solve as in ``paths_fp64`` (y left out: centred)."""
    X, idx = np.asarray(X, dtype=np.float64), np.asarray(path_idx, dtype=np.int64)
    K = kernel(kind, X, X, ls, kvar) + noise * np.eye(len(X))
    R = -(features(X / ls, u, phase, kvar) @ np.asarray(w).T) - np.asarray(eps).T
    if not centered:
        R = R + np.asarray(y).reshape(-1, 1)
    V = cho_solve(cho_factor(K, lower=True), R, check_finite=False)
    return _value_and_grad(kind, X, Q, ls, kvar, V.T[idx], u, phase, np.asarray(w)[idx], np.float64)


def weights_ld(truth: TruthLD, u, phase, w, eps, centered=False):
    """V (N x S) in long double: ``TruthLD.v`` (centred: minus alpha = K^-1 y)"""
    V = truth.v(u, phase, w, eps)
    return V - _solve_ld(truth.L, truth.y) if centered else V


def value_and_grad_ld(truth: TruthLD, Q, path_idx, u, phase, w, eps, centered=False, V=None):
    """(f (T,), df (T, d)) in ``np.longdouble``; ``V``: the weights of ``weights_ld`` when the caller keeps them"""
    idx = np.asarray(path_idx, dtype=np.int64)
    V = weights_ld(truth, u, phase, w, eps, centered) if V is None else V
    return _value_and_grad(truth.kind, truth.X, Q, truth.ls, truth.kvar, V.T[idx], u, phase,
                           np.asarray(w, dtype=np.longdouble)[idx], np.longdouble)


__all__ = ["value_and_grad_fp64", "value_and_grad_ld", "weights_ld"]
