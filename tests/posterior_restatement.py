"""NumPy restatements shared by tests/test_posterior_draws_cpu.py and tests/test_gpu_posterior_draws.py: the device's normals
of bobe_gp_posterior_sample (the contract above k_draw_normals, bobe_amd/csrc/posterior_kernels.hpp) and the dense joint
posterior covariance."""
import numpy as np
from scipy.linalg import solve_triangular

_U64 = np.uint64


def mix64(z):
    """splitmix64's finaliser on uint64 arrays (arithmetic modulo 2^64), hmc_mix64 of the kernels."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def u01(bits):
    """hmc_u01: the top 53 bits as a uniform in (0, 1)."""
    return ((np.asarray(bits, dtype=np.uint64) >> _U64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def device_normals(seed, S, C, s0=0):
    """z[s][c] for draws s0 .. s0+S-1 and points 0 .. C-1: key = mix(seed ^ mix(s)), u1 = u01(mix(key + 2c)),
    u2 = u01(mix(key + 2c + 1)), z = sqrt(-2 log u1) cos(2 pi u2)."""
    s = np.arange(s0, s0 + S, dtype=np.uint64)[:, None]
    c = np.arange(C, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        key = mix64(_U64(int(seed) & (2 ** 64 - 1)) ^ mix64(s))
        a = u01(mix64(key + _U64(2) * c))
        b = u01(mix64(key + _U64(2) * c + _U64(1)))
    return np.sqrt(-2.0 * np.log(a)) * np.cos(6.283185307179586 * b)


def kernel(kind, A, B, ls, kvar):
    """k(a, b) of the library (RBF or Matern-5/2) on coordinates scaled by the length scales."""
    a, b = np.asarray(A) / ls, np.asarray(B) / ls
    r2 = np.maximum(np.sum(a * a, 1)[:, None] + np.sum(b * b, 1)[None, :] - 2.0 * a @ b.T, 0.0)
    if kind == "rbf":
        return kvar * np.exp(-0.5 * r2)
    r = np.sqrt(np.maximum(r2, 1e-30))
    return kvar * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * np.exp(-np.sqrt(5.0) * r)


def dense_cov(kind, X, Q, ls, kvar, noise):
    """k(Q, Q) + noise I - V^T V with V = L^-1 k(X, Q), L = chol(k(X, X) + noise I): standardised units."""
    K = kernel(kind, X, X, ls, kvar) + noise * np.eye(len(X))
    L = np.linalg.cholesky(K)
    V = solve_triangular(L, kernel(kind, X, Q, ls, kvar), lower=True, check_finite=False)
    S = kernel(kind, Q, Q, ls, kvar) - V.T @ V
    S[np.diag_indices_from(S)] = kvar + noise - np.sum(V * V, axis=0)
    return S


__all__ = ["mix64", "u01", "device_normals", "kernel", "dense_cov"]
