"""The later stages of the one-sweep batch selection (``bobe_gp_wip_select_batch`` and its ``_w`` / ``_zvar`` forms), restated
for ``bobe_debug_batch_terms``.  Shared by tests/test_batch_terms_cpu.py and tests/test_gpu_batch_terms.py; NumPy (and SciPy's
log-sum-exp for float64, its triangular solve for the float64 stage 0) only, nothing imported from bobe_amd.  The kernel, the
factorisation and the substitutions are tests/zvar_restatement.py's; gamma, the kernel allowance and ``_worst``
tests/sweep_terms_restatement.py's.

After stage 0 the selection never refactorises.  With p the previous stage's pick, v* = V[:, p] and s_p its s_c BEFORE the
downdate, stage j (1-based, j - 1 earlier u rows) forms on the candidate side and on the Z side

    u(.) = ((k(., p) - V(.)^T v*) - sum_{i < j-1} u_i(.) u_i(p)) / sqrt(s_p)
    s_c -= u_c(c)^2        base_z -= u_z(z)^2        crossT[z][c] += u_z(z) u_c(c)

Layer A: each of these alone, recomputed in ``np.longdouble`` FROM THE JUDGED SIDE'S OWN INPUTS of that stage (V and V_Z of
``bobe_debug_sweep_terms``, the state before the stage and the earlier u rows of ``bobe_debug_batch_terms``), against a bound
that is a-priori and admits fused multiply-adds and any order of the sums.  eps = 2^-53, gamma_k = k eps / (1 - k eps).

  u rows   t = k - V^T v* - sum u_i u_i(p) is a sum of N + (j - 1) products and the kernel value, formed in the order row
           block partial sums (k_gemv_t_part), their sum, kv - q, the loop over the earlier rows, one subtraction: at most
           N + j + 1 roundings on any term, so |fl(t) - t| <= gamma_{N+j+2} (|k| + |V|^T |v*| + sum |u_i| |u_i(p)|) + dk with dk
           the allowance for the device's own kernel evaluation.  The square root and the division add one rounding each to
           u = fl(t) / sqrt(s_p): |u - t / sqrt(s_p)| <= bound_t / sqrt(s_p) + 3 eps |u| (2 eps (1 + eps) < 3 eps).
           s_p is read from the state BEFORE the stage: the teeth for the copy k_batch_gather makes (k_batch_u overwrites s_p).
  s, base  s_new = fl(s_old - u u): the product rounds once and the difference once, or the two fuse into one rounding;
           either way |s_new - (s_old - u^2)| <= eps u^2 + eps (|s_old| + u^2)(1 + eps) <= 2 eps (|s_old| + u^2).
  crossT   x_new = fl(x_old + u_z u_c), the same shape: <= 2 eps (|x_old| + |u_z u_c|).

The entry hands out its arrays without padding, so the padding columns of a u row (zero by k_batch_u's rule) are not seen.

Layer B: the stage scores end to end against the LITERAL REFIT of the (N + j)-point believer surrogate in long double
(``literal_batch``), under tests/zvar_cases.py's rule with the float64 literal refit as the yardstick (``rule``).

  weighted_scores  tests/weighted_criteria_restatement.py's in the state's dtype (float64: the same bits)
  scores           one of the five criteria from a state
  literal_batch    believer stages by refactorising, picks by argmin or along given picks
  recursion        the downdate recursion in float64 NumPy laid out as the entry hands it out (the CPU file's subject)
  check_terms      every Layer A ratio of such a dictionary
"""
import numpy as np
from scipy.special import logsumexp

import sweep_terms_restatement as S
import weighted_criteria_restatement as W
import zvar_restatement as R
from batch_select_restatement import FLOOR, masked_argmin

LD = np.longdouble
EPS = S.EPS
KEYS = ("wipv", "wipstd", "imiqr", "eiv", "zvar")           # the entry's criterion 0 .. 4
LOG_KEYS = ("imiqr", "eiv", "zvar")


# ------------------------------------------------------------------------------------------------- the scores, any dtype
def _lse(a, axis=None):
    """log sum exp (max, exp of the differences, sum, log, + max) in a's dtype; float64 goes to scipy.special.logsumexp, whose
    bits tests/weighted_criteria_restatement.py's scores have (it does not take long double on every platform)."""
    if a.dtype == np.float64:
        return logsumexp(a, axis=axis)
    m = np.max(a, axis=axis, keepdims=True)
    with np.errstate(divide="ignore"):
        out = np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True)) + m
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def fantasy_var(st, y_std):
    dt = st["base"].dtype.type
    cross = st["kcz"] - st["G"].T
    with np.errstate(all="ignore"):
        var = st["base"][None, :] - cross * cross / st["s"][:, None]
    var = np.where(st["s"][:, None] >= 0, var, dt(np.nan))
    var = np.where(np.isnan(var), dt(FLOOR), var)
    var = np.where(var < dt(FLOOR), dt(FLOOR), var)
    return var * dt(y_std) ** 2


def weighted_scores(st, y_std, log_weights=None):
    """``weighted_criteria_restatement.weighted_scores`` in the dtype of the state."""
    dt = st["base"].dtype.type
    v = fantasy_var(st, y_std)
    mu = dt(y_std) * st["mu"]
    ell = -mu if log_weights is None else np.asarray(log_weights, dtype=dt)
    a = ell + mu
    omega = np.exp(a - _lse(a))
    base = st["base"]
    b = np.where(np.isfinite(base) & (base >= dt(FLOOR)), base, dt(FLOOR)) * dt(y_std) ** 2
    e = ell + dt(2) * mu + dt(2) * b
    x = dt(W.U) * np.sqrt(v)
    return {"wipv": v @ omega, "wipstd": np.sqrt(v) @ omega,
            "imiqr": _lse(a[None, :] + x + np.log1p(-np.exp(-dt(2) * x)), axis=1),
            "eiv": -_lse(e[None, :] - v, axis=1), "log_s": _lse(e)}


def scores(st, y_std, log_weights, key):
    """The scores [C] of criterion ``key`` from a state, in the state's dtype."""
    if key == "zvar":
        return R.zvar_scores(st, y_std, log_weights)["zvar"]
    return weighted_scores(st, y_std, log_weights)[key]


# ------------------------------------------------------------------------------------------------- the truth: literal refits
def literal_batch(kind, X, ys, cand, Z, ls, kvar, noise, y_std, log_weights, n_batch, key, dtype=LD, follow=None):
    """Believer stages by refactorising the (N + j)-point surrogate in ``dtype`` (``zvar_restatement.literal_batch_zvar`` for any
    criterion): the pick joins X at its predicted standardised mean; y_mean, y_std and mu_z stay.  ``follow``: picks to apply
    instead of the stage's own argmin (the stage's argmin under their mask is returned all the same).
    Returns (picks applied [n_batch], stage_scores [n_batch x C], gaps [n_batch], argmins [n_batch])."""
    X = np.atleast_2d(np.asarray(X, dtype=dtype))
    ys = np.asarray(ys, dtype=dtype).reshape(-1)
    cand = np.atleast_2d(np.asarray(cand, dtype=dtype))
    picks, stages, gaps, mins, mu0 = [], [], [], [], None
    for j in range(n_batch):
        st = R.state(kind, X, ys, cand, Z, ls, kvar, noise, dtype)
        if mu0 is None:
            mu0 = st["mu"]
        assert np.max(np.abs(st["mu"] - mu0)) <= 1e-6 * (1.0 + np.max(np.abs(mu0))), "believer append moved the mean"
        st["mu"] = mu0
        sc = scores(st, y_std, log_weights, key)
        stages.append(sc)
        gaps.append(gap(sc, picks, key))
        mins.append(masked_argmin(sc, picks))
        p = mins[-1] if follow is None or j >= len(follow) else int(follow[j])
        picks.append(p)
        if j + 1 < n_batch:
            kp = R.kernel(kind, X, cand[p][None, :], ls, kvar, dtype)[:, 0]
            if dtype is np.float64:
                K = R.kernel(kind, X, X, ls, kvar, dtype) + noise * np.eye(X.shape[0])
                mean_p = kp @ np.linalg.solve(K, ys)
            else:
                mean_p = kp @ st["alpha"]
            X = np.vstack([X, cand[p][None, :]])
            ys = np.append(ys, mean_p)
    return (np.array(picks, dtype=np.int64), np.array(stages), np.array(gaps, dtype=np.float64),
            np.array(mins, dtype=np.int64))


def append_batch(kind, X, ys, cand, Z, ls, kvar, noise, y_std, log_weights, n_batch, key, follow=None):
    """``literal_batch`` in long double with the refit's factor extended by a row instead of recomputed: the Cholesky factor of
    the (N + j)-point matrix IS the factor of the N + j - 1 points with the row [l^T, d] under it, l = L^-1 k(X+, p),
    d = sqrt(k(p, p) + noise - l.l), so V, V_Z gain the row (k(p, .) - l^T V) / d and G, base, s its products.  O(N^2) a stage
    where the refit is O(N^3); tests/test_batch_terms_cpu.py holds it to the refits at 1e-15.  Same returns."""
    dt = LD
    X, cand, Z = (np.atleast_2d(np.asarray(a, dtype=dt)) for a in (X, cand, Z))
    st = R.state(kind, X, ys, cand, Z, ls, kvar, noise, dt)
    L = R.cholesky_lower(R.kernel(kind, X, X, ls, kvar, dt) + dt(noise) * np.eye(X.shape[0], dtype=dt))
    V, VZ = R.forward_sub(L, R.kernel(kind, X, cand, ls, kvar, dt)), R.forward_sub(L, R.kernel(kind, X, Z, ls, kvar, dt))
    kself = dt(kvar) + dt(noise)
    picks, stages, gaps, mins = [], [], [], []
    for j in range(n_batch):
        sc = scores(st, y_std, log_weights, key)
        stages.append(sc)
        gaps.append(gap(sc, picks, key))
        mins.append(masked_argmin(sc, picks))
        p = mins[-1] if follow is None or j >= len(follow) else int(follow[j])
        picks.append(p)
        if j + 1 < n_batch:
            xp = cand[p][None, :]
            lrow = R.forward_sub(L, R.kernel(kind, X, xp, ls, kvar, dt)[:, 0])
            dd = np.sqrt(kself - lrow @ lrow)
            vc = (R.kernel(kind, xp, cand, ls, kvar, dt)[0] - lrow @ V) / dd
            vz = (R.kernel(kind, xp, Z, ls, kvar, dt)[0] - lrow @ VZ) / dd
            n = L.shape[0]
            L = np.block([[L, np.zeros((n, 1), dtype=dt)], [lrow[None, :], np.full((1, 1), dd, dtype=dt)]])
            X, V, VZ = np.vstack([X, xp]), np.vstack([V, vc[None, :]]), np.vstack([VZ, vz[None, :]])
            st = dict(st, G=st["G"] + np.outer(vz, vc), base=st["base"] - vz * vz, s=st["s"] - vc * vc)
    return (np.array(picks, dtype=np.int64), np.array(stages), np.array(gaps, dtype=np.float64),
            np.array(mins, dtype=np.int64))


def gap(sc, taken, key):
    """The distance between the two best unmasked scores: relative for wipv / wipstd, absolute for the log scores."""
    v = np.array(sc, dtype=np.float64)
    v[list(taken)] = np.inf
    a, b = np.partition(v, 1)[:2]
    return float(b - a) if key in LOG_KEYS else float((b - a) / abs(a))


def rule(got, f64, truth, key):
    """tests/zvar_cases.py's rule per candidate, |got - truth| <= 4 |float64 literal refit - truth| + 1e-7 scale, scale =
    |truth| for wipv / wipstd and 1 + |truth| for the log scores.  Returns (holds, worst |got - truth| / scale, worst
    |f64 - truth| / scale)."""
    got, f64, truth = (np.asarray(a, dtype=LD) for a in (got, f64, truth))
    scale = (LD(1) + np.abs(truth)) if key in LOG_KEYS else np.abs(truth)
    err, ref = np.abs(got - truth), np.abs(f64 - truth)
    fin = np.isfinite(truth)                           # (+inf zvar: a candidate that teaches nothing, on both sides)
    same = np.all(np.asarray(got)[~fin] == np.asarray(truth)[~fin])
    ok = bool(same and np.all(err[fin] <= 4 * ref[fin] + LD(1e-7) * scale[fin]))
    return ok, float(np.max(err[fin] / scale[fin])), float(np.max(ref[fin] / scale[fin]))


# ------------------------------------------------------------------------------------------------- the float64 recursion
def recursion(kind, X, cand, Z, ls, kvar, noise, picks, cand_is_z=False, solve=False, terms0=None):
    """The downdate recursion along ``picks`` in float64 NumPy, laid out as the entries hand it out: {"V" [N x C], "VZ" [N x M],
    "picks" [n], "UC" [n x C], "UZ" [n x M], "crossT": n + 1 arrays [M x C], "sc": n + 1 [C], "basez": n + 1 [M]}; entry j of
    the three lists is the state after j downdates.  Stage 0 is sweep_terms_restatement.float64_stages' product with the
    inverse factor, or with ``solve`` SciPy's triangular solve (weighted_criteria_restatement.dense_state: the stage 0 of the
    float64 literal refit, so that what is left against it is the recursion alone), or ``terms0``: {"V", "VZ", "crossT", "sc",
    "basez"} as given (the device's, from ``bobe_debug_sweep_terms``: what float64 NumPy makes of the device's own stage 0)."""
    if terms0 is not None:
        t = terms0
    elif solve:
        d = W.dense_state(kind, X, np.zeros(np.atleast_2d(X).shape[0]), cand, Z, ls, kvar, noise)
        t = {"V": d["V"], "VZ": d["VZ"], "crossT": d["G"], "sc": d["s"], "basez": d["base"]}
    else:
        t = S.float64_stages(kind, X, cand, Z, ls, kvar, noise, False, cand_is_z=cand_is_z)
    cand, Z = np.atleast_2d(np.asarray(cand, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    V, VZ = t["V"], t["VZ"]
    out = {"V": V, "VZ": VZ, "picks": np.asarray(picks, dtype=np.int64), "UC": np.zeros((len(picks), cand.shape[0])),
           "UZ": np.zeros((len(picks), Z.shape[0])), "crossT": [t["crossT"]], "sc": [t["sc"]], "basez": [t["basez"]]}
    for j, p in enumerate(out["picks"]):
        xs = cand[p][None, :]
        uc = R.kernel(kind, cand, xs, ls, kvar, np.float64)[:, 0] - V.T @ V[:, p]
        uz = R.kernel(kind, Z, xs, ls, kvar, np.float64)[:, 0] - VZ.T @ V[:, p]
        ec, ez = np.zeros_like(uc), np.zeros_like(uz)
        for i in range(j):
            ec += out["UC"][i] * out["UC"][i][p]
            ez += out["UZ"][i] * out["UC"][i][p]
        root = np.sqrt(out["sc"][j][p])
        uc, uz = (uc - ec) / root, (uz - ez) / root
        out["UC"][j], out["UZ"][j] = uc, uz
        out["crossT"].append(out["crossT"][j] + np.outer(uz, uc))
        out["sc"].append(out["sc"][j] - uc * uc)
        out["basez"].append(out["basez"][j] - uz * uz)
    return out


def state_of(t, j, kcz, mu):
    """zvar_restatement's state dictionary from the terms after j downdates (k(z, c) and mu_z given)."""
    return {"kcz": kcz, "G": np.asarray(t["crossT"][j], dtype=np.float64), "base": np.asarray(t["basez"][j], dtype=np.float64),
            "s": np.asarray(t["sc"][j], dtype=np.float64), "mu": mu}


# ------------------------------------------------------------------------------------------------- Layer A
def check_u(V, v_star, k, dk, U_prev, u_prev_p, s_p, u, j):
    """(worst ratio, (column,)) of the u row of stage j over the columns given: V [N x n], k and dk [n] long double, U_prev
    [j - 1 x n] the side's earlier rows, u_prev_p [j - 1] the candidate side's earlier rows at the pick."""
    Vl, vs, Up, upp, ul = S.ld(V), S.ld(v_star), S.ld(U_prev), S.ld(u_prev_p), S.ld(u)
    t = k - Vl.T @ vs - Up.T @ upp
    mag = np.abs(k) + np.abs(Vl).T @ np.abs(vs) + np.abs(Up).T @ np.abs(upp)
    root = np.sqrt(LD(s_p))
    with np.errstate(all="ignore"):
        bound = (S.gamma(Vl.shape[0] + j + 2) * mag + dk) / root + LD(3) * EPS * np.abs(ul)
        return S._worst(np.abs(ul - t / root), bound)


def check_downdate(old, new, a, b):
    """(worst ratio, index) of new against old + a b (crossT: a = u_z [:, None], b = u_c [None, :]; s and base_z: a = -u, b = u)."""
    o, prod = S.ld(old), S.ld(a) * S.ld(b)
    return S._worst(np.abs(S.ld(new) - (o + prod)), LD(2) * EPS * (np.abs(o) + np.abs(prod)))


def check_terms(t, kind, X, cand, Z, ls, kvar, ck, cols=None):
    """Every Layer A ratio of the terms ``t`` (``recursion``'s dictionary): {"uc", "uz", "sc", "basez", "crossT": (worst ratio,
    (stage j, index ...)), "stages": {the same keys: [(ratio, index) of stage 1 .. n]}}, stage j = 1 .. n the one that applies
    picks[j - 1].  ``cols``: the candidate columns on which u_c
    and crossT are judged (all when None; they must hold the picks); s_c is judged on all of them either way."""
    cand, Z, X = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (cand, Z, X))
    cols = np.arange(cand.shape[0]) if cols is None else np.asarray(cols)
    picks = np.asarray(t["picks"])
    assert np.all(np.isin(picks, cols))
    V, VZ, UC, UZ = np.asarray(t["V"]), np.asarray(t["VZ"]), np.asarray(t["UC"]), np.asarray(t["UZ"])
    Vc, UCc = V[:, cols], UC[:, cols]
    worst = {k: (0.0, (0,)) for k in ("uc", "uz", "sc", "basez", "crossT")}
    worst["stages"] = {k: [] for k in worst}

    def keep(key, w, at):
        worst["stages"][key].append((w, at[1:]))
        if w >= worst[key][0]:
            worst[key] = (w, at)
    for j in range(1, len(picks) + 1):
        p = int(picks[j - 1])
        xs = cand[p][None, :]
        s_p = t["sc"][j - 1][p]
        upp = UC[:j - 1, p]
        kc, ac = S.kernel_truth(kind, cand[cols], xs, ls, kvar)
        kz, az = S.kernel_truth(kind, Z, xs, ls, kvar)
        w, at = check_u(Vc, V[:, p], kc[:, 0], S.kernel_allowance(ac[:, 0], ck), UCc[:j - 1], upp, s_p, UCc[j - 1], j)
        keep("uc", w, (j, int(cols[at[0]])))
        w, at = check_u(VZ, V[:, p], kz[:, 0], S.kernel_allowance(az[:, 0], ck), UZ[:j - 1], upp, s_p, UZ[j - 1], j)
        keep("uz", w, (j, at[0]))
        w, at = check_downdate(t["sc"][j - 1], t["sc"][j], -UC[j - 1], UC[j - 1])
        keep("sc", w, (j, at[0]))
        w, at = check_downdate(t["basez"][j - 1], t["basez"][j], -UZ[j - 1], UZ[j - 1])
        keep("basez", w, (j, at[0]))
        w, at = check_downdate(np.asarray(t["crossT"][j - 1])[:, cols], np.asarray(t["crossT"][j])[:, cols],
                               UZ[j - 1][:, None], UCc[j - 1][None, :])
        keep("crossT", w, (j, at[0], int(cols[at[1]])))
    return worst
