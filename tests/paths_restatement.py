"""NumPy restatements shared by tests/test_paths_cpu.py and tests/test_gpu_paths.py: the random Fourier features of
bobe_gp_paths_*, the device's draw layout (the contract above k_paths_draw_normals, bobe_amd/csrc/paths_kernels.hpp), a path by
SciPy's ``cho_solve``, the same path in ``np.longdouble`` (the truth of the value tests) and the exact moments of the path
ensemble for realised features."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from posterior_restatement import device_normals, kernel, mix64, u01

_U64 = np.uint64
PATHS_STREAM = 0x7061746873
TWO_PI = 6.283185307179586


def features(Xs, u, phase, kvar, dtype=np.float64):
    """Phi (n x F): phi_j(x) = sqrt(2 kvar / F) cos(u_j . xs + b_j) on coordinates already divided by the length scales."""
    Xs, u, phase = (np.asarray(a, dtype=dtype) for a in (Xs, u, phase))
    F = u.shape[0]
    return np.sqrt(dtype(2.0) * dtype(kvar) / dtype(F)) * np.cos(Xs @ u.T + phase[None, :])


def sub_seed(seed, a):
    with np.errstate(over="ignore"):
        return int(mix64(_U64(int(seed) & (2 ** 64 - 1)) ^ mix64(_U64(PATHS_STREAM + a))))


def device_arrays(seed, S, F, N, d, kind, noise):
    """u (F x d), phase (F), w (S x F), eps (S x N) as the device draws them from ``seed``."""
    g = device_normals(sub_seed(seed, 0), F, d)
    if kind == "rbf":
        u = g
    else:
        z = device_normals(sub_seed(seed, 1), F, 5)
        c = np.zeros(F)
        for k in range(5):
            c = c + z[:, k] * z[:, k]
        u = g * np.sqrt(5.0 / c)[:, None]
    j = np.arange(F, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = mix64(_U64(sub_seed(seed, 2)) ^ mix64(j))
    phase = TWO_PI * u01(mix64(key))
    w = device_normals(sub_seed(seed, 3), S, F)
    eps = np.sqrt(noise) * device_normals(sub_seed(seed, 4), S, N)
    return {"u": u, "phase": phase, "w": w, "eps": eps}


def paths_fp64(kind, X, y, Q, ls, kvar, noise, u, phase, w, eps, centered=False):
    """f (S x C) in fp64: phi(Q) w_s + k(Q, X) K^-1 (y - Phi(X) w_s - eps_s) by cho_solve (y left out: centred)."""
    K = kernel(kind, X, X, ls, kvar) + noise * np.eye(len(X))
    PX, PQ = features(X / ls, u, phase, kvar), features(Q / ls, u, phase, kvar)
    R = -(PX @ w.T) - eps.T
    if not centered:
        R = R + np.asarray(y).reshape(-1, 1)
    V = cho_solve(cho_factor(K, lower=True), R, check_finite=False)
    return (PQ @ w.T + kernel(kind, X, Q, ls, kvar).T @ V).T


def _kernel_ld(kind, A, B, ls, kvar):
    LD = np.longdouble
    a, b = np.asarray(A, dtype=LD) / np.asarray(ls, dtype=LD), np.asarray(B, dtype=LD) / np.asarray(ls, dtype=LD)
    r2 = np.zeros((len(a), len(b)), dtype=LD)
    for k in range(a.shape[1]):
        df = a[:, k][:, None] - b[:, k][None, :]
        r2 += df * df
    if kind == "rbf":
        return LD(kvar) * np.exp(-LD(0.5) * r2)
    r = np.sqrt(np.maximum(r2, LD(1e-30)))
    s5 = np.sqrt(LD(5.0))
    return LD(kvar) * (LD(1.0) + s5 * r + LD(5.0) / LD(3.0) * r2) * np.exp(-s5 * r)


def _chol_ld(K):
    """plain-loop Cholesky in long double (column by column, the inner products vectorised)"""
    n = len(K)
    L = np.zeros_like(K)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve_ld(L, B):
    n = len(L)
    Y = np.zeros_like(B)
    for i in range(n):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    Xo = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        Xo[i] = (Y[i] - L[i + 1:, i] @ Xo[i + 1:]) / L[i, i]
    return Xo


class TruthLD:
    """The long-double path of one problem (the factor is computed once and shared by the value tests)."""

    def __init__(self, kind, X, y, ls, kvar, noise):
        LD = np.longdouble
        self.kind, self.X, self.ls, self.kvar = kind, X, ls, kvar
        self.y = np.asarray(y, dtype=LD).reshape(-1, 1)
        K = _kernel_ld(kind, X, X, ls, kvar)
        K[np.diag_indices_from(K)] += LD(noise)
        self.L = _chol_ld(K)

    def paths(self, Q, u, phase, w, eps, centered=False):
        LD = np.longdouble
        ls = np.asarray(self.ls, dtype=LD)
        PX = features(np.asarray(self.X, dtype=LD) / ls, u, phase, self.kvar, dtype=LD)
        PQ = features(np.asarray(Q, dtype=LD) / ls, u, phase, self.kvar, dtype=LD)
        wl, el = np.asarray(w, dtype=LD), np.asarray(eps, dtype=LD)
        R = -(PX @ wl.T) - el.T
        if not centered:
            R = R + self.y
        V = _solve_ld(self.L, R)
        return (PQ @ wl.T + _kernel_ld(self.kind, self.X, Q, self.ls, self.kvar).T @ V).T

    def v(self, u, phase, w, eps):
        """v_s = K^-1 (y - Phi(X) w_s - eps_s), N x S"""
        LD = np.longdouble
        ls = np.asarray(self.ls, dtype=LD)
        PX = features(np.asarray(self.X, dtype=LD) / ls, u, phase, self.kvar, dtype=LD)
        return _solve_ld(self.L, self.y - PX @ np.asarray(w, dtype=LD).T - np.asarray(eps, dtype=LD).T)


def ensemble_moments(kind, X, y, Q, ls, kvar, noise, u, phase):
    """The exact mean and covariance of f_s(Q) over w ~ N(0, I), eps ~ N(0, noise I) for the REALISED features (u, phase):
    with B = k(Q, X) K^-1 and G = Phi(Q) - B Phi(X):  mean = B y,  cov = G G^T + noise B B^T."""
    K = kernel(kind, X, X, ls, kvar) + noise * np.eye(len(X))
    B = cho_solve(cho_factor(K, lower=True), kernel(kind, X, Q, ls, kvar), check_finite=False).T
    G = features(Q / ls, u, phase, kvar) - B @ features(X / ls, u, phase, kvar)
    return B @ np.asarray(y).reshape(-1), G @ G.T + noise * B @ B.T


def spectral_frequencies(kind, F, d, rng):
    """u (F x d) and phase (F) from a NumPy generator, by the law the device uses."""
    g = rng.standard_normal((F, d))
    if kind != "rbf":
        g = g * np.sqrt(5.0 / rng.chisquare(5, size=F))[:, None]
    return g, rng.uniform(0.0, TWO_PI, size=F)


__all__ = ["features", "sub_seed", "device_arrays", "paths_fp64", "TruthLD", "ensemble_moments", "spectral_frequencies"]
