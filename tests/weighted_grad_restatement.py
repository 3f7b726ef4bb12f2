"""Analytic value-and-gradient of the four importance-weighted scores (``bobe_gp_wip_grad_w``) with respect to the candidate's
coordinates, stated once and generic in the dtype; shared by tests/test_weighted_grad_cpu.py and
tests/test_gpu_weighted_grad.py.  Imports nothing from bobe_amd.

  np.float64     LAPACK (``cholesky`` / ``cho_solve`` / ``solve_triangular``), the quadratic forms from the half-solved
                 vectors V = L^-1 k as the reference forms them: the restatement whose own error sets the scale
  np.longdouble  ``_kernel_ld`` / ``_chol_ld`` / ``_solve_ld`` of tests/paths_restatement.py: the truth

For candidate x, integration point z, in the standardised units of the targets (notation of
tests/weighted_criteria_restatement.py), with u = K^-1 k(X, x), W = K^-1 K(X, Z):

    s = kvar + noise - k_x . u        base_z = kvar + noise - k_z . W_z        cross_z = k(x, z) - k_x . W_z
    v+_z = y_std^2 (base_z - cross_z^2 / s),  NaN / < 1e-12 / s < 0 -> 1e-12 y_std^2: FLOORED, a constant with zero gradient
    d v+_z / dx_j = y_std^2 [-2 cross_z / s d cross_z / dx_j + cross_z^2 / s^2 d s / dx_j]
    d k(x, p) / dx_j = G(x, p) (p_j - x_j) / ls_j^2,  G = dk / d(-r^2 / 2)  (k itself for RBF, kvar 5/3 (1 + sqrt5 r) e^{-sqrt5 r})
    d cross_z / dx_j = d k(x, z) / dx_j - sum_n W[n][z] d k(x, X_n) / dx_j,      d s / dx_j = -2 sum_n u_n d k(x, X_n) / dx_j

Each score is a function of the v+_z alone (``scores_from_v``), d score / d v+_z = rho_z (``rho_from_v``):

    wipv   sum omega v+                                   rho = omega
    wipstd sum omega sqrt(v+)                             rho = omega / (2 sqrt(v+))
    imiqr  LSE_z t_z, t = a + x + log1p(-e^{-2x}), x = u sqrt(v+)     rho = exp(t - imiqr) coth(x) u / (2 sqrt(v+))
    eiv    -LSE_z (e - v+)                                rho = exp(e - v+ + eiv)

Both log-sum-exps are normalised by their maximum in both dtypes (exp(1e5) overflows long double too).  No y_mean: the shifts
``GP.wip_sweep`` adds to imiqr / eiv are constants.
"""
import numpy as np
from scipy.linalg import cho_solve, cholesky, solve_triangular

from paths_restatement import _chol_ld, _kernel_ld, _solve_ld

FLOOR = 1e-12
U = 0.6744897501960817
KEYS = ("wipv", "wipstd", "imiqr", "eiv")


def _kernel(kind, A, B, ls, kvar, dtype):
    if dtype is np.longdouble:
        return _kernel_ld(kind, A, B, ls, kvar)
    a = np.asarray(A, dtype=np.float64) / np.asarray(ls, dtype=np.float64)
    b = np.asarray(B, dtype=np.float64) / np.asarray(ls, dtype=np.float64)
    r2 = np.zeros((a.shape[0], b.shape[0]))
    for j in range(a.shape[1]):
        df = a[:, j][:, None] - b[:, j][None, :]
        r2 += df * df
    if kind == "rbf":
        return kvar * np.exp(-0.5 * r2)
    r = np.sqrt(np.maximum(r2, 1e-30))
    s5 = np.sqrt(5.0)
    return kvar * (1.0 + s5 * r + 5.0 / 3.0 * r2) * np.exp(-s5 * r)


def _grad_factor(kind, x, P, ls, kvar, dtype):
    """G(x, p) = dk / d(-r^2 / 2) for the rows p of P, and the scaled differences (p - x) / ls [P x d]."""
    D = dtype
    dif = (np.asarray(P, dtype=D) - np.asarray(x, dtype=D)[None, :]) / np.asarray(ls, dtype=D)[None, :]
    r2 = np.sum(dif * dif, axis=1)
    if kind == "rbf":
        return D(kvar) * np.exp(-D(0.5) * r2), dif
    r = np.sqrt(np.maximum(r2, D(1e-30)))
    s5 = np.sqrt(D(5.0))
    return D(kvar) * D(5.0) / D(3.0) * (D(1.0) + s5 * r) * np.exp(-s5 * r), dif


def lse(t):
    """log sum exp(t), normalised by the maximum (any dtype)"""
    m = np.max(t)
    return m + np.log(np.sum(np.exp(t - m)))


class State:
    """What does not depend on the candidate: K^-1 applied to y and to K(X, Z), base_z, the per-z table."""

    def __init__(self, kind, X, ys, Z, ls, kvar, noise, y_std, log_weights=None, dtype=np.float64):
        D = self.dtype = dtype
        self.kind, self.ls, self.kvar, self.noise = kind, np.asarray(ls, dtype=D), D(kvar), D(noise)
        self.X, self.Z, self.y_std = np.asarray(X, dtype=D), np.asarray(Z, dtype=D), D(y_std)
        K = _kernel(kind, X, X, ls, kvar, D)
        K[np.diag_indices_from(K)] += D(noise)
        kxz = _kernel(kind, X, Z, ls, kvar, D)
        rhs = np.concatenate([kxz, np.asarray(ys, dtype=D).reshape(-1, 1)], axis=1)
        self.kself = D(kvar) + D(noise)
        if D is np.longdouble:
            self.L = _chol_ld(K)
            sol = _solve_ld(self.L, rhs)
            self.W, alpha = sol[:, :-1], sol[:, -1]
            self.VZ = None
            self.base = self.kself - np.sum(kxz * self.W, axis=0)
        else:
            self.L = cholesky(K, lower=True)
            alpha = cho_solve((self.L, True), rhs[:, -1])
            self.VZ = solve_triangular(self.L, kxz, lower=True, check_finite=False)
            self.W = solve_triangular(self.L.T, self.VZ, lower=False, check_finite=False)
            self.base = self.kself - np.sum(self.VZ * self.VZ, axis=0)
        # the per-z table (weighted_criteria_restatement.z_terms)
        self.mu = self.y_std * (kxz.T @ alpha)
        self.ell = -self.mu if log_weights is None else np.asarray(log_weights, dtype=D)
        self.a = self.ell + self.mu
        self.omega = np.exp(self.a - lse(self.a))
        b = np.where(np.isfinite(self.base) & (self.base >= D(FLOOR)), self.base, D(FLOOR)) * self.y_std ** 2
        self.e = self.ell + D(2.0) * self.mu + D(2.0) * b

    def candidate(self, kx, kxz):
        """(u = K^-1 k_x, s, cross [M]) from k_x = k(X, x) and k(x, Z)"""
        if self.dtype is np.longdouble:
            u = _solve_ld(self.L, kx[:, None])[:, 0]
            return u, self.kself - kx @ u, kxz - kx @ self.W
        v = solve_triangular(self.L, kx, lower=True, check_finite=False)
        u = solve_triangular(self.L.T, v, lower=False, check_finite=False)
        return u, self.kself - v @ v, kxz - self.VZ.T @ v


def scores_from_v(v, a, omega, e):
    """The four scores as functions of the fantasy variances v+ [M] (physical units) and the per-z table."""
    D = v.dtype.type
    sr = np.sqrt(v)
    x = D(U) * sr
    return {"wipv": np.sum(omega * v), "wipstd": np.sum(omega * sr), "imiqr": lse(a + x + np.log1p(-np.exp(-D(2.0) * x))),
            "eiv": -lse(e - v)}


def rho_from_v(v, a, omega, e):
    """d score / d v+_z of the four scores, the closed forms of the module docstring."""
    D = v.dtype.type
    sr = np.sqrt(v)
    x = D(U) * sr
    em = np.exp(-D(2.0) * x)
    t = a + x + np.log1p(-em)
    coth = (D(1.0) + em) / (-np.expm1(-D(2.0) * x))
    te = e - v
    return {"wipv": omega + D(0.0) * v, "wipstd": omega / (D(2.0) * sr), "imiqr": np.exp(t - lse(t)) * coth * D(U) / (D(2.0) * sr),
            "eiv": np.exp(te - lse(te))}


def fantasy_var_and_grad(st, x):
    """(v+ [M], floored [M] bool, d v+ / dx [M x d]) of one candidate; floored rows of the gradient are zero."""
    D = st.dtype
    x = np.asarray(x, dtype=D)
    kx = _kernel(st.kind, st.X, x[None, :], st.ls, st.kvar, D)[:, 0]
    u, s, cross = st.candidate(kx, _kernel(st.kind, st.Z, x[None, :], st.ls, st.kvar, D)[:, 0])
    with np.errstate(all="ignore"):
        v = st.base - cross * cross / s
    floored = ~(s >= 0) | np.isnan(v) | (v < D(FLOOR))
    v = np.where(floored, D(FLOOR), v) * st.y_std ** 2
    gn, dn = _grad_factor(st.kind, x, st.X, st.ls, st.kvar, D)
    gz, dz = _grad_factor(st.kind, x, st.Z, st.ls, st.kvar, D)
    dk_n = gn[:, None] * dn / st.ls[None, :]                       # d k(x, X_n) / dx_j   [N x d]
    dk_z = gz[:, None] * dz / st.ls[None, :]                       # d k(x, z) / dx_j     [M x d]
    dcross = dk_z - st.W.T @ dk_n
    ds = -D(2.0) * (u @ dk_n)
    with np.errstate(all="ignore"):
        dv = st.y_std ** 2 * ((-D(2.0) * cross / s)[:, None] * dcross + (cross * cross / (s * s))[:, None] * ds[None, :])
    dv = np.where(floored[:, None], D(0.0), dv)
    return v, floored, dv


def value_and_grad(st, cand):
    """dict: ``<key>`` (C,), ``d<key>`` (C, d) for the four scores, ``floored`` (C, M) - all in st.dtype."""
    cand = np.atleast_2d(np.asarray(cand, dtype=st.dtype))
    C, d = cand.shape
    out = {k: np.zeros(C, dtype=st.dtype) for k in KEYS}
    out.update({"d" + k: np.zeros((C, d), dtype=st.dtype) for k in KEYS})
    out["floored"] = np.zeros((C, len(st.Z)), dtype=bool)
    for c in range(C):
        v, fl, dv = fantasy_var_and_grad(st, cand[c])
        val = scores_from_v(v, st.a, st.omega, st.e)
        rho = rho_from_v(v, st.a, st.omega, st.e)
        out["floored"][c] = fl
        for k in KEYS:
            out[k][c] = val[k]
            out["d" + k][c] = rho[k] @ dv
    return out
