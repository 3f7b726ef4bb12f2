"""Restatements of the two fit objectives with the noise level as a hyper-parameter, shared by tests/test_noise_fit_cpu.py and
tests/test_gpu_noise_fit.py.  Imports nothing from bobe_amd.  theta = (log ls_1..d, log kvar, log nu), K~ = K + nu I,
standardised targets:

  MLL   = -1/2 y^T K~^-1 y - 1/2 log det K~ - N/2 log 2 pi
  L_LOO = sum_i 1/2 log a_i - alpha_i^2 / (2 a_i) - 1/2 log 2 pi,   a = diag K~^-1, alpha = K~^-1 y

  noise_closed         the closed forms of both values and of both gradients (d + 2 entries) in the dtype asked for: fp64
                       through LAPACK (cho_factor / cho_solve), np.longdouble through the hand-written Cholesky and triangular
                       inverse of tests/loo_restatement.py - the truth
  noise_torch          torch-fp64 autograd through the two values: independent of the gradient formulas
  central_difference   of either value in one coordinate of theta

The last gradient entries are  dMLL / dlog nu = 1/2 nu (|alpha|^2 - tr K~^-1)  and  dL_LOO / dlog nu = nu tr M =
-nu (sum_k c_k (A^2)_kk + w^T alpha)  with the c, b, w, M of loo_restatement.loo_closed_xp.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from loo_restatement import HALF_LOG_2PI, SQRT5, _sqdiffs, chol_xp, kernel_from_r2, tri_inv_xp


def split_theta(log_theta, d):
    t = np.asarray(log_theta)
    return np.exp(t[:d]), np.exp(t[d]), np.exp(t[d + 1])


def noise_closed(kind, X, y, ls, kvar, noise, dtype=np.float64):
    """dict(mll, mll_grad, loo, loo_grad) in ``dtype``; the gradients wrt (log ls_1..d, log kvar, log nu)."""
    xp = dtype
    y = np.asarray(y, dtype=xp).reshape(-1)
    n = y.shape[0]
    D = _sqdiffs(X, ls, xp)
    kt, fac = kernel_from_r2(kind, np.sum(D, axis=0), kvar)
    nu = xp(noise)
    K = kt + nu * np.eye(n, dtype=xp)
    half = xp(0.5)
    if xp is np.float64:
        cf = cho_factor(K, lower=True, check_finite=False)
        A = cho_solve(cf, np.eye(n), check_finite=False)
        alpha = cho_solve(cf, y, check_finite=False)
        logdet_half = float(np.sum(np.log(np.diag(cf[0]))))
        half_log_2pi = HALF_LOG_2PI
    else:
        L = chol_xp(K)
        Li = tri_inv_xp(L)
        A = Li.T @ Li
        alpha = Li.T @ (Li @ y)
        logdet_half = np.sum(np.log(np.diag(L)))
        half_log_2pi = half * np.log(xp(8) * np.arctan(xp(1)))
    a = np.diag(A).copy()

    def contract(M):          # sum_ab M_ab dK~_ab / dtheta_j for the d + 2 coordinates
        Mf = M * fac
        return np.array([np.sum(Mf * D[j]) for j in range(D.shape[0])] + [np.sum(M * kt), nu * np.trace(M)], dtype=xp)

    mll = -half * (y @ alpha) - logdet_half - n * half_log_2pi
    mll_grad = contract(half * (np.outer(alpha, alpha) - A))
    loo = np.sum(half * np.log(a) - half * alpha * alpha / a - half_log_2pi)
    c = 1 / (2 * a) + alpha * alpha / (2 * a * a)
    b = -alpha / a
    w = A @ b
    M = -(A * c[None, :]) @ A - (np.outer(w, alpha) + np.outer(alpha, w)) / 2
    return {"mll": mll, "mll_grad": mll_grad, "loo": loo, "loo_grad": contract(M)}


def noise_closed_theta(kind, X, y, log_theta, dtype=np.float64):
    ls, kvar, nu = split_theta(np.asarray(log_theta, dtype=dtype), np.asarray(X).shape[1])
    return noise_closed(kind, X, y, ls, kvar, nu, dtype)


def noise_torch(kind, X, y, log_theta):
    """dict(mll, mll_grad, loo, loo_grad) by torch-fp64 autograd; log_theta = (log ls_1..d, log kvar, log nu)."""
    import torch
    X_t = torch.as_tensor(np.asarray(X, dtype=np.float64))
    y_t = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1))
    d, n = X_t.shape[1], X_t.shape[0]
    out = {}
    for which in ("mll", "loo"):
        th = torch.tensor(np.asarray(log_theta, dtype=np.float64), requires_grad=True)
        xs = X_t / torch.exp(th[:d])
        r2 = ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1)
        kvar = torch.exp(th[d])
        if kind == "rbf":
            k = kvar * torch.exp(-0.5 * r2)
        else:
            dd = torch.sqrt(torch.clamp(r2, min=1e-30))
            k = kvar * (1.0 + dd * (SQRT5 + dd * 5.0 / 3.0)) * torch.exp(-SQRT5 * dd)
        K = k + torch.exp(th[d + 1]) * torch.eye(n, dtype=torch.float64)
        L = torch.linalg.cholesky(K)
        if which == "mll":
            wv = torch.linalg.solve_triangular(L, y_t[:, None], upper=False)[:, 0]
            val = -0.5 * (wv @ wv) - torch.log(torch.diagonal(L)).sum() - n * HALF_LOG_2PI
        else:
            A = torch.cholesky_inverse(L)
            a = torch.diagonal(A)
            alpha = A @ y_t
            val = (0.5 * torch.log(a) - 0.5 * alpha * alpha / a - HALF_LOG_2PI).sum()
        (g,) = torch.autograd.grad(val, th)
        out[which], out[which + "_grad"] = float(val.detach()), g.numpy().copy()
    return out


def central_difference(kind, X, y, log_theta, which, j, h=1e-4, dtype=np.longdouble):
    """(f(theta + h e_j) - f(theta - h e_j)) / 2h of ``which`` ('mll' / 'loo'), evaluated in ``dtype``."""
    t = np.asarray(log_theta, dtype=dtype)
    e = np.zeros_like(t)
    e[j] = dtype(h)
    return (noise_closed_theta(kind, X, y, t + e, dtype)[which] - noise_closed_theta(kind, X, y, t - e, dtype)[which]) / (2 * dtype(h))


def seeded_case(n, d, kind, seed=None):
    """Seeded data of a parity case, in the style of the golden generators: X uniform in the unit cube, a smooth function of
    it plus a little seeded scatter, standardised; length scales and a kernel variance of order one."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    X = rng.uniform(size=(n, d))
    f = np.sin(3.0 * X[:, 0]) + np.sum(X[:, 1:] ** 2, axis=1) - 0.5 * X[:, 0] * X[:, -1] + 0.05 * rng.standard_normal(n)
    ls = 0.3 + 0.5 * rng.uniform(size=d)
    kvar = 0.8 + 0.7 * rng.uniform()
    return X, f, ls, float(kvar)


def standardise(y):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return (y - float(np.mean(y))) / float(np.std(y))
