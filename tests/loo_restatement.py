"""Restatements of leave-one-out cross-validation of a GP (Rasmussen & Williams, section 5.4.2) shared by
tests/test_loo_cpu.py and tests/test_gpu_loo.py.  Imports nothing from bobe_amd.  Standardised units throughout: the caller
passes the targets as the GP holds them; hyper-parameters, noise and standardisation are held fixed while a point is left out.

  loo_brute            N literal refits (scipy.linalg.cho_factor on the N-1 remaining points)
  loo_closed           the closed form in fp64 through cho_solve
  loo_closed_inv       the same through np.linalg.inv: a second fp64 evaluation by another route
  loo_closed_xp        np.longdouble, hand-written Cholesky and triangular inverse: the truth; with the hand formula of the
                       gradient of L_LOO wrt (log ls, log kvar)
  loo_objective_torch  torch-fp64 autograd through the closed form: the gradient's yardstick, independent of that formula
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

SQRT5 = 2.23606797749978969641
HALF_LOG_2PI = 0.91893853320467274178


def _sqdiffs(X, ls, dtype=np.float64):
    """D[j][a][b] = (x_aj / ls_j - x_bj / ls_j)^2 by direct differences (the reference's dist_sq on scaled coordinates)."""
    xs = np.asarray(X, dtype=dtype) / np.asarray(ls, dtype=dtype)
    return np.stack([(xs[:, j][:, None] - xs[:, j][None, :]) ** 2 for j in range(xs.shape[1])])


def kernel_from_r2(kind, r2, kvar):
    """k and dk / dlog ls_j = factor * D_j of the reference's kernels (RBF; Matern-5/2 with r^2 floored at 1e-30)."""
    dt = r2.dtype.type
    if kind == "rbf":
        k = dt(kvar) * np.exp(-dt(0.5) * r2)
        return k, k
    s5 = dt(SQRT5) if dt is np.float64 else np.sqrt(dt(5))
    dd = np.sqrt(np.where(r2 < dt(1e-30), dt(1e-30), r2))
    e = np.exp(-s5 * dd)
    k = dt(kvar) * (dt(1) + dd * (s5 + dd * dt(5) / dt(3))) * e
    fac = np.where(r2 < dt(1e-30), dt(0), dt(kvar) * (dt(5) / dt(3)) * (dt(1) + s5 * dd) * e)
    return k, fac


def kernel_matrix(kind, X, ls, kvar, noise, dtype=np.float64):
    D = _sqdiffs(X, ls, dtype)
    k, _ = kernel_from_r2(kind, np.sum(D, axis=0), kvar)
    return k + dtype(noise) * np.eye(k.shape[0], dtype=dtype)


def _terms(a, alpha, y):
    dt = a.dtype.type
    half = dt(0.5)
    half_log_2pi = dt(HALF_LOG_2PI) if dt is np.float64 else half * np.log(dt(8) * np.arctan(dt(1)))
    mean = y - alpha / a
    var = 1 / a
    lpd = half * np.log(a) - half * alpha * alpha / a - half_log_2pi
    return mean, var, lpd


def loo_brute(kind, X, y, ls, kvar, noise):
    """(mean, var, lpd) by N literal refits: the GP of the other N-1 points predicts point i (noise included)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    K = kernel_matrix(kind, X, ls, kvar, noise)
    n = K.shape[0]
    mean, var = np.empty(n), np.empty(n)
    for i in range(n):
        m = np.arange(n) != i
        cf = cho_factor(K[np.ix_(m, m)], lower=True, check_finite=False)
        ki = K[m, i]
        mean[i] = ki @ cho_solve(cf, y[m], check_finite=False)
        var[i] = K[i, i] - ki @ cho_solve(cf, ki, check_finite=False)
    lpd = -0.5 * np.log(var) - 0.5 * (y - mean) ** 2 / var - HALF_LOG_2PI
    return mean, var, lpd


def loo_closed(kind, X, y, ls, kvar, noise):
    """(mean, var, lpd, L_LOO) in fp64: A = K^-1 through cho_factor / cho_solve."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    K = kernel_matrix(kind, X, ls, kvar, noise)
    cf = cho_factor(K, lower=True, check_finite=False)
    A = cho_solve(cf, np.eye(K.shape[0]), check_finite=False)
    alpha = cho_solve(cf, y, check_finite=False)
    mean, var, lpd = _terms(np.diag(A).copy(), alpha, y)
    return mean, var, lpd, float(np.sum(lpd))


def loo_closed_inv(kind, X, y, ls, kvar, noise):
    """The same through np.linalg.inv (LU): another fp64 route."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    A = np.linalg.inv(kernel_matrix(kind, X, ls, kvar, noise))
    mean, var, lpd = _terms(np.diag(A).copy(), A @ y, y)
    return mean, var, lpd, float(np.sum(lpd))


def chol_xp(K):
    """Lower Cholesky factor in the dtype of K (column by column; no LAPACK: np.longdouble has none)."""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        v = K[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"not positive definite at column {j}")
        L[j:, j] = v / np.sqrt(v[0])
    return L


def tri_inv_xp(L):
    """Inverse of a lower-triangular matrix in its dtype (row by row forward substitution on the identity)."""
    n = L.shape[0]
    Li = np.zeros_like(L)
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1 / L[i, i]
    return Li


def loo_closed_xp(kind, X, y, ls, kvar, noise, want_grad=False):
    """The truth in np.longdouble: dict(mean, var, lpd, loo[, grad]).  grad: the hand formula
    dL/dtheta_j = sum_ab M_ab dK_ab/dtheta_j, M = -A diag(c) A - 1/2 (w alpha^T + alpha w^T), theta = (log ls, log kvar)."""
    xp = np.longdouble
    y = np.asarray(y, dtype=xp).reshape(-1)
    D = _sqdiffs(X, ls, xp)
    kt, fac = kernel_from_r2(kind, np.sum(D, axis=0), kvar)
    K = kt + xp(noise) * np.eye(kt.shape[0], dtype=xp)
    Li = tri_inv_xp(chol_xp(K))
    a = np.sum(Li * Li, axis=0)
    alpha = Li.T @ (Li @ y)
    mean, var, lpd = _terms(a, alpha, y)
    out = {"mean": mean, "var": var, "lpd": lpd, "loo": np.sum(lpd)}
    if want_grad:
        A = Li.T @ Li
        c = 1 / (2 * a) + alpha * alpha / (2 * a * a)
        b = -alpha / a
        w = A @ b
        M = -(A * c[None, :]) @ A - (np.outer(w, alpha) + np.outer(alpha, w)) / 2
        Mf = M * fac
        out["grad"] = np.array([np.sum(Mf * D[j]) for j in range(D.shape[0])] + [np.sum(M * kt)], dtype=xp)
    return out


def loo_objective_torch(kind, X, y, log_theta, noise):
    """(L_LOO, dL_LOO / dlog_theta) by torch-fp64 autograd through the closed form; log_theta = (log ls_1..d, log kvar)."""
    import torch
    X_t = torch.as_tensor(np.asarray(X, dtype=np.float64))
    y_t = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1))
    th = torch.tensor(np.asarray(log_theta, dtype=np.float64), requires_grad=True)
    d = X_t.shape[1]
    xs = X_t / torch.exp(th[:d])
    r2 = ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1)
    kvar = torch.exp(th[d])
    if kind == "rbf":
        k = kvar * torch.exp(-0.5 * r2)
    else:
        dd = torch.sqrt(torch.clamp(r2, min=1e-30))
        k = kvar * (1.0 + dd * (SQRT5 + dd * 5.0 / 3.0)) * torch.exp(-SQRT5 * dd)
    K = k + noise * torch.eye(k.shape[0], dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    A = torch.cholesky_inverse(L)
    a = torch.diagonal(A)
    alpha = A @ y_t
    val = (0.5 * torch.log(a) - 0.5 * alpha * alpha / a - HALF_LOG_2PI).sum()
    (g,) = torch.autograd.grad(val, th)
    return float(val.detach()), g.numpy().copy()
