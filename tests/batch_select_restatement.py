"""Restatement of the one-sweep batch selection for WIPV / WIPStd (``bobe_gp_wip_select_batch``) in NumPy fp64, shared by
tests/test_batch_select_cpu.py and tests/test_gpu_batch_select.py.  Imports nothing from bobe_amd.

The scores read the design points only.  With L = chol(K(X, X) + noise I), V = L^-1 K(X, C), V_Z = L^-1 K(X, Z):

    s_c = kvar + noise - |V[:, c]|^2        base_z = kvar + noise - |V_Z[:, z]|^2        G[z][c] = V_Z[:, z] . V[:, c]
    cross(c, z) = k(c, z) - G[z][c]         var+(z | c) = base_z - cross^2 / s_c  -> NaN / < 1e-12 -> 1e-12 -> * y_std^2

Appending the pick c* at its believed mean changes them by the rank-one term

    u(.) = (k(., c*) - V(.)^T V[:, c*] - sum_{i<j} u_i(.) u_i(c*)) / sqrt(s_{c*})
    G[z][c] += u(z) u(c)        base_z -= u(z)^2        s_c -= u(c)^2

which is what a sweep on the (N+j)-point believer surrogate computes (``literal_loop`` below refactors instead).

  select_batch   the downdate recursion
  literal_loop   the believer loop on a GP object with ``update`` / ``predict_mean_single`` and a sweep function
  masked_argmin  first occurrence of the minimum over the indices not taken yet; NaN counts as minimal (jnp.argmin)
  score_state    WIPV / WIPStd of every candidate from (kcz, G, base, s)
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

SQRT5 = 2.23606797749978969641
FLOOR = 1e-12


def kernel(kind, A, B, ls, kvar):
    """k(a, b) without noise: RBF, or Matern-5/2 with r^2 floored at 1e-30 (direct differences of the scaled coordinates)."""
    a = np.asarray(A, dtype=np.float64) / np.asarray(ls, dtype=np.float64)
    b = np.asarray(B, dtype=np.float64) / np.asarray(ls, dtype=np.float64)
    r2 = np.zeros((a.shape[0], b.shape[0]))
    for j in range(a.shape[1]):
        df = a[:, j][:, None] - b[:, j][None, :]
        r2 += df * df
    if kind == "rbf":
        return kvar * np.exp(-0.5 * r2)
    dd = np.sqrt(np.where(r2 < 1e-30, 1e-30, r2))
    return kvar * (1.0 + dd * (SQRT5 + dd * 5.0 / 3.0)) * np.exp(-SQRT5 * dd)


def masked_argmin(v, taken=()):
    """Index of the first minimum of v over the indices not in ``taken``; a NaN counts as smaller than everything."""
    best, bi = None, -1
    taken = set(int(t) for t in taken)
    for i, x in enumerate(np.asarray(v, dtype=np.float64)):
        if i in taken:
            continue
        if bi < 0:
            best, bi = x, i
        elif not np.isnan(best) and (np.isnan(x) or x < best):
            best, bi = x, i
    return bi


def score_state(kcz, G, base, s, y_std):
    """(wipv, wipstd) of all candidates: kcz [C x M] = k(c, z), G [M x C], base [M], s [C] (gp.py:552-576, 574-576)."""
    cross = kcz - G.T
    with np.errstate(all="ignore"):
        var = base[None, :] - cross * cross / s[:, None]
    var = np.where(s[:, None] >= 0, var, np.nan)            # sqrt(negative) is NaN in fast_update_cholesky (gp.py:187)
    var = np.where(np.isnan(var), FLOOR, var)
    var = np.where(var < FLOOR, FLOOR, var)
    var = var * y_std ** 2
    return np.mean(var, axis=1), np.mean(np.sqrt(var), axis=1)


def select_batch(kind, X, cand, Z, ls, kvar, noise, n_batch, criterion, y_std=1.0):
    """The downdate recursion.  Returns (picks [n_batch], stage_scores [n_batch x C]); criterion 'wipv' or 'wipstd'."""
    X, cand, Z = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (X, cand, Z))
    K = kernel(kind, X, X, ls, kvar) + noise * np.eye(X.shape[0])
    L = cholesky(K, lower=True)
    V = solve_triangular(L, kernel(kind, X, cand, ls, kvar), lower=True, check_finite=False)
    VZ = solve_triangular(L, kernel(kind, X, Z, ls, kvar), lower=True, check_finite=False)
    kself = kvar + noise
    s = kself - np.sum(V * V, axis=0)
    base = kself - np.sum(VZ * VZ, axis=0)
    G = VZ.T @ V
    kcz = kernel(kind, cand, Z, ls, kvar)
    picks, stages, UC, UZ = [], [], [], []
    for j in range(n_batch):
        if j > 0:
            p = picks[-1]
            xs = cand[p][None, :]
            uc = kernel(kind, cand, xs, ls, kvar)[:, 0] - V.T @ V[:, p]
            uz = kernel(kind, Z, xs, ls, kvar)[:, 0] - VZ.T @ V[:, p]
            for pc, pz in zip(UC, UZ):
                uc = uc - pc * pc[p]
                uz = uz - pz * pc[p]
            uc, uz = uc / np.sqrt(s[p]), uz / np.sqrt(s[p])
            G = G + np.outer(uz, uc)
            base = base - uz * uz
            s = s - uc * uc
            UC.append(uc)
            UZ.append(uz)
        wv, ws = score_state(kcz, G, base, s, y_std)
        sc = wv if criterion == "wipv" else ws
        stages.append(sc)
        picks.append(masked_argmin(sc, picks))
    return np.array(picks, dtype=np.int64), np.array(stages)


def best_two_gap(scores, taken=()):
    """Relative gap between the two smallest scores over the indices not in ``taken``."""
    v = np.array(scores, dtype=np.float64)
    v[list(taken)] = np.inf
    a, b = np.partition(v, 1)[:2]
    return (b - a) / abs(a)


def literal_loop(gp, sweep, cand, n_batch, power):
    """The kriging-believer loop: sweep, pick (a picked index is masked: ``update`` would drop it as a duplicate), append
    the pick at its predicted mean (``gp.update`` refactors the N+j points and standardises again), sweep again.
    ``sweep(gp)`` returns the scores of all candidates in the surrogate's units; they are divided by y_std^power, so every
    stage is in standardised units.  Returns (picks, stage_scores [n_batch x C], gaps [n_batch])."""
    picks, stages, gaps = [], [], []
    for j in range(n_batch):
        sc = np.asarray(sweep(gp), dtype=np.float64) / float(gp.y_std) ** power
        stages.append(sc)
        gaps.append(best_two_gap(sc, picks))
        p = masked_argmin(sc, picks)
        picks.append(p)
        if j + 1 < n_batch:
            n0 = gp.train_x.shape[0]
            gp.update(cand[p], gp.predict_mean_single(cand[p]))
            assert gp.train_x.shape[0] == n0 + 1, "the believer surrogate dropped the pick as a duplicate"
    return np.array(picks, dtype=np.int64), np.array(stages), np.array(gaps)
