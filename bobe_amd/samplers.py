"""Evidence (logZ) and MC-point consumers of the GPU GP — counterpart of ``BOBE/samplers.py``.

The reference hands the jitted ``gp.predict_mean_single`` to dynesty, one point per call
(samplers.py:112-115, 157-160) — the worst pattern for a GPU.  Here a static nested sampler runs on the host
and asks the GP for *batches*: replacement candidates are drawn uniformly inside an enlarged bounding
ellipsoid of the live points (clipped to the unit cube), a few thousand at a time, and scored with ONE
``bobe_gp_predict`` call.  Everything downstream follows the reference:
  * ``compute_integrals``  — the dynesty trapezoid evidence integral (samplers.py:27-50);
  * logZ bounds from the GP standard deviation at the samples, logl +- std  (samplers.py:172-176), and the
    variance estimate (samplers.py:178-183);  the BO loop's convergence test is (upper-lower)/2 < threshold
    (bo.py:886-891);
  * result dictionaries with the reference's keys (samplers.py:184-194).
dynesty is not re-implemented (no multi-ellipsoid decomposition); NumPyro's NUTS is, on the device, as the opt-in
``sample_GP_NUTS(sampler="nuts")``.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
from scipy.special import expit

from .utils import get_logger, get_numpy_rng, renormalise_log_weights  # noqa: F401 (re-exported)

log = get_logger("sampler")


def compute_integrals(logl=None, logvol=None, reweight=None, squared=False):
    """samplers.py:27-50 (dynesty utility): cumulative log-evidence by the trapezoid rule in prior volume."""
    if logl is None or logvol is None:
        raise ValueError("logl and logvol are required")                  # (the reference asserts, samplers.py:28-29)
    logl = np.asarray(logl, dtype=np.float64)
    logvol = np.asarray(logvol, dtype=np.float64)
    loglstar_pad = np.concatenate([[-1.0e300], logl])
    dlogvol = np.diff(logvol, prepend=0)
    logdvol = logvol - dlogvol + np.log1p(-np.exp(dlogvol))
    if squared:
        logdvol = 2 * logdvol
    logdvol2 = logdvol + math.log(0.5)
    saved_logwt = np.logaddexp(loglstar_pad[1:], loglstar_pad[:-1]) + logdvol2
    if reweight is not None:
        saved_logwt = saved_logwt + reweight
    return np.logaddexp.accumulate(saved_logwt)


def resample_equal(samples, logl, weights, rng=None):
    """Systematic resampling to equal weights (dynesty.utils.resample_equal, used at samplers.py:187-188)."""
    rng = rng if rng is not None else get_numpy_rng()
    n = len(weights)
    positions = (rng.random() + np.arange(n)) / n
    cum = np.cumsum(weights)
    cum[-1] = 1.0
    idx = np.searchsorted(cum, positions)
    return samples[idx], logl[idx]


def _bounding_ellipsoid(live: np.ndarray, enlarge: float):
    """Mean, Cholesky factor of the scaled covariance and its volume factor: {x : |A^-1 (x-mu)| <= 1}."""
    mu = live.mean(axis=0)
    d = live.shape[1]
    cov = np.cov(live, rowvar=False).reshape(d, d) + 1e-12 * np.eye(d)
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, (live - mu).T)
    r = math.sqrt(float(np.max(np.sum(z * z, axis=0)))) * enlarge
    return mu, L * r


def _draw_in_ellipsoid(mu, A, n, rng):
    d = mu.shape[0]
    g = rng.standard_normal((n, d))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    u = rng.random(n) ** (1.0 / d)
    x = mu + (g * u[:, None]) @ A.T
    return x[np.all((x >= 0.0) & (x <= 1.0), axis=1)]


def logz_from_samples(gp, samples_x, logl, logvol, mean: float, logz_err: float, *, n_draws: int = 0,
                      draws_seed: int = 0, draws_max_points: int = 16384, draws_method: str = "joint",
                      draws_features: int = 2048, draws_arrays: Optional[Dict] = None, moments: bool = False,
                      moments_max_points: int = 65536) -> Dict:
    """The logZ dictionary of a finished run (samplers.py:172-183): the GP's predictive variance at every sample —
    ONE batched ``bobe_gp_predict`` call instead of the reference's ``lax.map`` over points — turns into
    logl +- std for the upper / lower evidence integrals and into the variance estimate of logZ.

    ``upper`` / ``lower`` treat the GP's errors at the samples as perfectly correlated, ``var`` / ``std`` as independent.
    ``n_draws > 0`` adds the distribution the GP itself implies (``_logz_draws``): ``draws`` (logZ of ``n_draws`` joint
    posterior draws of the surrogate at the samples), ``draws_mean``, ``draws_std``, ``draws_points``, ``draws_jitter``.
    The other keys do not depend on it, and the run's generator is not used.

    ``draws_method``: 'joint' (default) perturbs the ``draws_max_points`` heaviest samples by a draw from their dense joint
    covariance (``GP.sample_posterior``, at most 16384 points); 'paths' perturbs EVERY sample with a finite, ungated logl by a
    centred pathwise draw of the surrogate (``GP.sample_paths`` with ``draws_features`` random Fourier features, cost linear
    in the number of samples, no cap) and reports ``draws_features`` in the place of ``draws_jitter``.  ``draws_arrays``
    ('paths' only): the caller's ``u`` / ``phase`` / ``w`` / ``eps`` for ``GP.sample_paths`` instead of the seeded ones.

    ``moments=True`` adds the GP's own answer in closed form (``_logz_moments``, ``GP.evidence_moments``: the exact mean and
    variance of the lognormal evidence estimate under the JOINT posterior of the surrogate at the samples, nothing drawn, no
    cap of 16384): ``moments_log_ez``, ``moments_log_var``, ``moments_std`` (of log Z) and ``moments_points``, the number of
    samples that enter as random (``draws_points`` with ``moments_max_points``; the rest are constants).  The other keys do
    not depend on it either."""
    if draws_method not in ("joint", "paths"):
        raise ValueError(f"draws_method must be 'joint' or 'paths', not {draws_method!r}")
    logl = np.asarray(logl, dtype=np.float64)
    var = np.asarray(gp.predict_var_batched(samples_x), dtype=np.float64)
    std = np.sqrt(var)
    upper = compute_integrals(logl=logl + std, logvol=logvol)
    lower = compute_integrals(logl=logl - std, logvol=logvol)
    var = np.clip(var, 1e-12, 1e12)
    log_var_delta = compute_integrals(logl=2 * logl + np.log(var), logvol=logvol, squared=True)[-1]
    var_logz = math.exp(float(np.clip(log_var_delta - 2 * mean, -100, 100)))
    out = {"mean": float(mean), "dlogz_sampler": float(logz_err), "upper": float(upper[-1]), "lower": float(lower[-1]),
           "var": var_logz, "std": 2 * math.sqrt(var_logz)}
    if n_draws > 0 and draws_method == "paths":
        out.update(_logz_draws_paths(gp, samples_x, logl, logvol, int(n_draws), int(draws_seed), int(draws_features),
                                     draws_arrays))
    elif n_draws > 0:
        out.update(_logz_draws(gp, samples_x, logl, logvol, int(n_draws), int(draws_seed), int(draws_max_points)))
    if moments:
        out.update(_logz_moments(gp, samples_x, logl, logvol, int(moments_max_points)))
    return out


def _log_weights(logl, logvol):
    """The trapezoid weights of ``compute_integrals`` per sample (what ``nested_sampling`` reports as logwt)."""
    pad = np.concatenate([[-1e300], logl])
    dv = np.diff(logvol, prepend=0)
    return np.logaddexp(pad[1:], pad[:-1]) + (logvol - dv + np.log1p(-np.exp(dv))) + math.log(0.5)


def draws_points(gp, logl, logvol, max_points: int = 16384) -> np.ndarray:
    """Indices (ascending) of the samples whose logl the evidence draws perturb: those with the largest weight ``logwt``,
    at most ``max_points`` of them (ties: the earlier sample).  A sample with a non-finite logl or the gate's mark
    ``gp.minus_inf`` is held fixed."""
    logl = np.asarray(logl, dtype=np.float64)
    free = np.isfinite(logl)
    minus_inf = getattr(gp, "minus_inf", None)
    if minus_inf is not None:
        free &= logl != float(minus_inf)
    idx = np.flatnonzero(free)
    if len(idx) > max_points:
        logwt = _log_weights(logl, np.asarray(logvol, dtype=np.float64))
        idx = np.sort(idx[np.argsort(-logwt[idx], kind="stable")[:max_points]])
    return idx


def _logz_moments(gp, samples_x, logl, logvol, max_points: int) -> Dict:
    """Mean and variance of Z = sum_z e^{logwt_z} e^{f(z) - logl_z} over the free samples (``draws_points``: finite, ungated,
    the ``max_points`` heaviest; a sample whose weight logwt is not finite - two equal log-volumes in a row - is held fixed like
    the gated ones and adds nothing) plus the constants e^{logwt_z} of the others, from ``gp.evidence_moments`` with
    l_z = logwt_z - logl_z (the convention of ``get_mc_points(weighted=True)``).  std: of log Z, lognormal-matched, from logs."""
    from .gp import std_from_log_t0
    logl = np.asarray(logl, dtype=np.float64)
    logvol = np.asarray(logvol, dtype=np.float64)
    logwt = _log_weights(logl, logvol)
    idx = draws_points(gp, logl, logvol, max_points)
    idx = idx[np.isfinite(logwt[idx])]
    fixed = np.ones(len(logl), dtype=bool)
    fixed[idx] = False
    fw = logwt[fixed]
    fw = fw[np.isfinite(fw)]
    log_fixed = float(np.logaddexp.reduce(fw)) if len(fw) else -math.inf
    if not len(idx):
        return {"moments_log_ez": log_fixed, "moments_log_var": -math.inf, "moments_std": 0.0, "moments_points": 0}
    m = gp.evidence_moments(np.asarray(samples_x)[idx], log_weights=logwt[idx] - logl[idx])
    log_ez = float(np.logaddexp(m["log_ez"], log_fixed))
    log_var = float(m["log_t0"] + 2.0 * m["log_ez"])
    # log (Var Z / E[Z]^2) of the whole sum -> the standard deviation of log Z
    return {"moments_log_ez": log_ez, "moments_log_var": log_var, "moments_std": float(std_from_log_t0(log_var - 2.0 * log_ez)),
            "moments_points": int(len(idx))}


def _logz_draws(gp, samples_x, logl, logvol, n_draws: int, seed: int, max_points: int) -> Dict:
    """logZ of ``n_draws`` draws of the surrogate: draw s integrates logl + delta_s, delta_s a CENTRED joint posterior draw
    of the GP at the perturbed samples (``draws_points``; ``gp.sample_posterior(..., centered=True)``, seeded by ``seed``)
    and 0 elsewhere."""
    logl = np.asarray(logl, dtype=np.float64)
    idx = draws_points(gp, logl, logvol, max_points)
    delta, jitter = np.zeros((n_draws, 0)), 0.0
    if len(idx):
        delta, jitter = gp.sample_posterior(np.asarray(samples_x)[idx], n_samples=n_draws, seed=seed, centered=True,
                                            return_jitter=True)
    draws = np.empty(n_draws)
    for s in range(n_draws):
        ls = logl.copy()
        ls[idx] += delta[s]
        draws[s] = compute_integrals(logl=ls, logvol=logvol)[-1]
    return {"draws": draws, "draws_mean": float(np.mean(draws)), "draws_std": float(np.std(draws)),
            "draws_points": int(len(idx)), "draws_jitter": float(jitter)}


def _logz_draws_paths(gp, samples_x, logl, logvol, n_draws: int, seed: int, n_features: int, arrays: Optional[Dict]) -> Dict:
    """``_logz_draws`` without the cap: delta_s is path s of ``gp.sample_paths`` minus the posterior mean
    (``evaluate(..., centered=True)``) at EVERY sample ``draws_points`` leaves free; gated and non-finite samples stay fixed."""
    logl = np.asarray(logl, dtype=np.float64)
    idx = draws_points(gp, logl, logvol, max_points=len(logl))
    delta = np.zeros((n_draws, 0))
    if len(idx):
        with gp.sample_paths(n_draws, n_features, seed=seed, **(arrays or {})) as paths:
            delta = paths.evaluate(np.asarray(samples_x)[idx], centered=True)
    draws = np.empty(n_draws)
    for s in range(n_draws):
        ls = logl.copy()
        ls[idx] += delta[s]
        draws[s] = compute_integrals(logl=ls, logvol=logvol)[-1]
    return {"draws": draws, "draws_mean": float(np.mean(draws)), "draws_std": float(np.std(draws)),
            "draws_points": int(len(idx)), "draws_features": int(n_features)}


def _rwalk_pool(loglike, live, live_logl, worst, lstar, rng, n_walkers, walks, scale, gp=None):
    """Replacement candidates by constrained random walks, the proposal dynesty's 'rwalk' uses (the reference's choice,
    samplers.py:64, 152) — run as ONE batch: ``n_walkers`` walkers start from random live points and take ``walks``
    Metropolis steps inside {L > L*, unit cube}.  Steps are drawn from the live points' covariance ellipsoid scaled by
    ``scale``.  With a surrogate that has ``rwalk`` (the GPU GP) ALL steps of all walkers are one launch
    (``bobe_gp_rwalk``); otherwise every step is one batched ``loglike`` call.  Returns (points, logl, calls, acceptance
    rate); walkers that never moved are dropped (they would duplicate a live point)."""
    nlive, d = live.shape
    ok = np.ones(nlive, dtype=bool)
    ok[worst] = False
    cov = np.cov(live[ok], rowvar=False).reshape(d, d) + 1e-14 * np.eye(d)
    A = np.linalg.cholesky(cov)
    start = rng.choice(np.flatnonzero(ok), size=n_walkers)
    x, lx = live[start].copy(), live_logl[start].copy()
    if gp is not None and hasattr(gp, "rwalk") and d == gp.ndim:       # (a caller-chosen ``ndim`` walks on the host)
        x, lx, nacc, nin = gp.rwalk(x, lx, scale * A, lstar, walks, int(rng.integers(0, 2 ** 62)))
        moved = nacc > 0
        perm = rng.permutation(np.flatnonzero(moved))
        return x[perm], lx[perm], int(nin.sum()), float(nacc.sum()) / float(n_walkers * walks)
    moved = np.zeros(n_walkers, dtype=bool)
    n_acc, calls = 0, 0
    for _ in range(walks):
        prop = x + scale * (rng.standard_normal((n_walkers, d)) @ A.T)
        inside = np.all((prop >= 0.0) & (prop <= 1.0), axis=1)
        lp = np.full(n_walkers, -np.inf)
        if inside.any():
            lp[inside] = loglike(prop[inside])
            calls += int(inside.sum())
        acc = inside & (lp > lstar)
        x[acc], lx[acc] = prop[acc], lp[acc]
        moved |= acc
        n_acc += int(acc.sum())
    perm = rng.permutation(np.flatnonzero(moved))
    return x[perm], lx[perm], calls, n_acc / float(n_walkers * walks)


def nested_sampling(gp, ndim: Optional[int] = None, mode: str = "convergence", dlogz: float = 0.01,
                    maxcall: int = int(5e6), equal_weights: bool = False, rng=None, batch: int = 8192,
                    enlarge: float = 1.25, nlive: Optional[int] = None, sample_method: str = "auto",
                    walks: Optional[int] = None, device_walks: bool = True, logz_draws: int = 0,
                    logz_draws_seed: int = 0, *, keep_weights: bool = False, logz_moments: bool = False,
                    logz_draws_method: str = "joint") -> Tuple[Dict, Dict, bool]:
    """Static nested sampling of exp(GP mean) over the unit cube -> (samples_dict, logz_dict, success).

    Settings follow ``nested_sampling_Dy`` (samplers.py:119-126): mode 'acq' uses nlive = max(100, min(500, 20 d))
    and dlogz = 0.1 with equal-weight samples; otherwise nlive = max(500, 40 d).
    ``sample_method``: 'ellipsoid' = uniform draws in the enlarged bounding ellipsoid of the live points (exact, cheap
    in a few dimensions), 'rwalk' = batched constrained random walks (``_rwalk_pool``; what the reference asks dynesty
    for), 'auto' = ellipsoid up to 4 dimensions, rwalk above.  ``device_walks``: whole walks in one launch where the
    surrogate offers ``rwalk`` (``bobe_gp_rwalk``); False steps them from the host, one batched prediction per step.
    ``logz_draws`` > 0: the logZ dictionary also holds the evidence of that many joint posterior draws of the surrogate
    (``logz_from_samples``, seeded by ``logz_draws_seed``); reported only, nothing else depends on them.
    ``keep_weights``: mode 'acq' returns the weighted samples as they are instead of resampling them to equal weights.
    ``logz_draws_method``: 'joint' (default) or 'paths' - how those draws are made (``logz_from_samples``, ``draws_method``).
    ``logz_moments``: True adds the closed-form ``moments_*`` keys of ``logz_from_samples(moments=True)``; reported only."""
    if logz_draws_method not in ("joint", "paths"):
        raise ValueError(f"logz_draws_method must be 'joint' or 'paths', not {logz_draws_method!r}")
    rng = rng if rng is not None else get_numpy_rng()
    ndim = ndim if ndim is not None else gp.ndim
    if mode == "acq":
        nlive = nlive or max(100, min(500, 20 * ndim))
        dlogz, equal_weights = 0.1, not keep_weights
    else:
        nlive = nlive or max(500, 40 * ndim)

    def loglike(x):
        return np.asarray(gp.predict_mean_batched(x), dtype=np.float64)

    live = rng.uniform(size=(nlive, ndim))
    live_logl = loglike(live)
    if not np.all(np.isfinite(live_logl)):               # a NaN surrogate (factor not positive definite): no evidence
        log.warning("nested sampling skipped: the surrogate returns non-finite values")
        nan = float("nan")
        logz_nan = {"mean": nan, "dlogz_sampler": nan, "upper": nan, "lower": nan, "var": nan, "std": nan}
        if logz_draws > 0:
            logz_nan.update(draws=np.full(int(logz_draws), nan), draws_mean=nan, draws_std=nan, draws_points=0)
            logz_nan.update({"draws_features": 0} if logz_draws_method == "paths" else {"draws_jitter": nan})
        if logz_moments:
            logz_nan.update(moments_log_ez=nan, moments_log_var=nan, moments_std=nan, moments_points=0)
        return ({"x": live, "weights": np.ones(nlive), "logl": live_logl, "best": live[0], "method": "nested"},
                logz_nan, False)
    use_rwalk = sample_method == "rwalk" or (sample_method == "auto" and ndim > 4)
    walks = walks if walks is not None else max(25, 4 * ndim)           # dynesty's default is 25
    rw_scale = 2.38 / math.sqrt(ndim)
    ncall = nlive
    dead_x, dead_logl = [], []
    logz = -np.inf
    pool_x = np.empty((0, ndim))
    pool_l = np.empty(0)
    pool_pos = 0
    since_update = 0
    it = 0
    update_every = max(1, nlive // 5)
    gave_up = truncated = False
    log_shell = math.log1p(-math.exp(-1.0 / nlive))

    def logaddexp(a, b):                                  # np.logaddexp's formula on Python floats (thousands of calls)
        if a == -math.inf:
            return b
        hi, lo = (a, b) if a > b else (b, a)
        return hi + math.log1p(math.exp(lo - hi))
    lmax = float(np.max(live_logl))                       # (only ever rises: the retired point is the lowest)
    while True:
        worst = int(np.argmin(live_logl))
        lstar = float(live_logl[worst])
        # Stop BEFORE the worst point is retired — it then stays among the final live points and is counted once
        # (dynesty checks at the top of its iteration too).  Remaining evidence bound (dynesty's stopping rule):
        # dlogz = log(z + Lmax X) - log z.
        if it > 0 and logaddexp(logz, lmax - it / nlive) - logz < dlogz:
            break
        if ncall >= maxcall:
            truncated = True
            break
        logdx = -it / nlive + log_shell                                 # log(X_{i-1} - X_i)
        logz_before = logz
        logz = logaddexp(logz, lstar + logdx)
        dead_x.append(live[worst].copy())
        dead_logl.append(lstar)
        it += 1
        # replacement with L > L*: pop pre-scored proposals, refill the pool in GPU batches.  Two ways out without one:
        # the call budget (``maxcall``) - handled like the check at the top of the loop, a TRUNCATED run, reported the way
        # dynesty's would be - and 200 fruitless refills (a plateau / degenerate surrogate): the run is unsuccessful.
        # Either way the pool just generated is scanned before giving up.
        found = False
        tries = 0
        out_of_calls = False
        gave_up = False                                       # (per replacement search: a hit on the last refill is a hit)
        while not found:
            while pool_pos < len(pool_l):
                if pool_l[pool_pos] > lstar:
                    live[worst] = pool_x[pool_pos]
                    live_logl[worst] = pool_l[pool_pos]
                    lmax = max(lmax, float(pool_l[pool_pos]))
                    pool_pos += 1
                    found = True
                    break
                pool_pos += 1
            if found or gave_up or out_of_calls:
                break
            if use_rwalk:
                pool_x, pool_l, calls, rate = _rwalk_pool(loglike, live, live_logl, worst, lstar, rng,
                                                          n_walkers=max(256, min(batch // 8, 2 * nlive)), walks=walks,
                                                          scale=rw_scale, gp=gp if device_walks else None)
                pool_pos = 0
                ncall += calls
                # keep the acceptance rate of a step near one half (dynesty adapts its scale the same way)
                rw_scale = float(np.clip(rw_scale * math.exp((rate - 0.5) / max(ndim, 1) * 4.0), 1e-4, 4.0))
            else:
                if since_update >= update_every or tries > 0 or len(pool_l) == 0:
                    mask = np.ones(nlive, dtype=bool)
                    mask[worst] = False
                    mu, A = _bounding_ellipsoid(live[mask], enlarge)
                    since_update = 0
                x = _draw_in_ellipsoid(mu, A, batch, rng)
                if len(x) == 0:
                    x = rng.uniform(size=(batch, ndim))
                pool_x, pool_l, pool_pos = x, loglike(x), 0
                ncall += len(x)
            tries += 1
            gave_up = tries > 200                             # plateau / degenerate surrogate
            out_of_calls = ncall >= maxcall                   # (the refreshed pool is still scanned once)
        if found:
            gave_up = False                                   # (the flag describes the search that ENDED the run)
        if not found:
            # No replacement: the point just retired is still a live point.  Take the retirement back (it is counted once,
            # among the final live points) and end the run as TRUNCATED - its evidence is not a converged one.
            dead_x.pop()
            dead_logl.pop()
            it -= 1
            logz = logz_before
            truncated = True
            if gave_up:
                log.warning("nested sampling: no acceptable replacement found; stopping early (run marked unsuccessful)")
            break
        since_update += 1
    # final live points, appended in order of increasing logl (dynesty add_final_live)
    order = np.argsort(live_logl)
    niter = len(dead_logl)
    logvol_dead = -np.arange(1, niter + 1) / nlive
    logvol_live = (logvol_dead[-1] if niter else 0.0) + np.log1p(-(np.arange(nlive) + 1.0) / (nlive + 1.0))
    samples_x = np.vstack([np.array(dead_x).reshape(-1, ndim), live[order]])
    logl = np.concatenate([np.array(dead_logl), live_logl[order]])
    logvol = np.concatenate([logvol_dead, logvol_live])
    cum = compute_integrals(logl=logl, logvol=logvol)
    mean = float(cum[-1])
    # information and the sampler's own error estimate sqrt(H / nlive)
    dv = np.diff(logvol, prepend=0)
    logwt = np.logaddexp(np.concatenate([[-1e300], logl])[1:], np.concatenate([[-1e300], logl])[:-1]) + \
        (logvol - dv + np.log1p(-np.exp(dv))) + math.log(0.5)
    w = np.exp(logwt - mean)
    h_info = float(np.sum(w * (logl - mean)))
    logz_err = math.sqrt(max(h_info, 0.0) / nlive)
    # samplers.py:167; a run that ended because no replacement could be found is NOT a successful one: bo.py must not
    # call logZ converged on it (a run cut by maxcall alone is reported the way dynesty's would be, with a flag)
    success = bool(~np.all(logl == logl[0])) and not gave_up

    logz_dict = logz_from_samples(gp, samples_x, logl, logvol, mean, logz_err, n_draws=logz_draws,
                                  draws_seed=logz_draws_seed, draws_method=logz_draws_method, moments=bool(logz_moments))
    logz_dict.update(ncall=int(ncall), niter=int(niter), truncated=bool(truncated))
    best_pt = samples_x[int(np.argmax(logl))]
    weights = renormalise_log_weights(logwt)
    if equal_weights:
        samples_x, logl = resample_equal(samples_x, logl, weights, rng=rng)
        weights = np.ones(samples_x.shape[0])
    samples_dict = {"x": samples_x, "weights": weights, "logl": logl, "best": best_pt, "method": "nested"}
    return samples_dict, logz_dict, success


# --------------------------------------------------------------------------------------------------------------
# MCMC on the surrogate (samplers.py:196-360)
# --------------------------------------------------------------------------------------------------------------
def prior_transform(x):
    """samplers.py:52-53: the unit cube is the prior."""
    return x


def nested_sampling_Dy(gp, mode: str = "acq", ndim: int = 1, dlogz: float = 0.1, dynamic: bool = False,
                       maxcall: Optional[int] = int(5e6), print_progress: Optional[bool] = True,
                       equal_weights: bool = False, sample_method: str = "rwalk", rng=None, *, logz_draws: int = 0,
                       logz_draws_seed: int = 0, logz_moments: bool = False, logz_draws_method: str = "joint"):
    """The reference's entry point name and keywords (samplers.py:55-65) on ``nested_sampling`` above; ``dynamic``,
    ``print_progress`` are dynesty options without a counterpart here; ``sample_method='rwalk'`` (the reference's
    default) maps to 'auto': exact ellipsoid draws in up to 4 dimensions, batched random walks above.  ``logz_draws``,
    ``logz_draws_seed``, ``logz_moments``, ``logz_draws_method``: see ``nested_sampling``."""
    return nested_sampling(gp, ndim=ndim if ndim and ndim > 1 else gp.ndim, mode=mode, dlogz=dlogz,
                           maxcall=maxcall if maxcall is not None else int(5e6), equal_weights=equal_weights, rng=rng,
                           sample_method="auto" if sample_method == "rwalk" else sample_method, logz_draws=logz_draws,
                           logz_draws_seed=logz_draws_seed, logz_moments=logz_moments, logz_draws_method=logz_draws_method)


def get_hmc_settings(ndim, warmup_steps=None, num_samples=None, thinning=None):
    """samplers.py:196-214."""
    warmup_steps = warmup_steps if warmup_steps is not None else (256 if ndim <= 9 else 512)
    num_samples = num_samples if num_samples is not None else (1024 if ndim <= 9 else 2048)
    thinning = thinning if thinning is not None else 4
    return warmup_steps, num_samples, thinning


def adaptation_schedule(num_steps: int):
    """Stan's windowed warm-up, the rule of NumPyro's ``build_adaptation_schedule``: inclusive (start, end) windows - an
    initial fast window (75 steps), slow windows of 25, 50, 100, ... steps (the last one stretched to the terminal
    buffer when three times its size would overrun it) and a terminal fast window (50 steps).  Below 150 steps the
    buffers are 15 % / 10 % of the steps around one slow window; below 20 steps there is one window."""
    n = int(num_steps)
    if n <= 0:
        return []
    if n < 20:
        return [(0, n - 1)]
    init_buffer, term_buffer, base_window = 75, 50, 25
    if n < init_buffer + term_buffer + base_window:
        init_buffer, term_buffer = int(0.15 * n), int(0.1 * n)
        base_window = n - init_buffer - term_buffer
    schedule = [(0, init_buffer - 1)]
    end_window_start = n - term_buffer
    next_size, next_start = base_window, init_buffer
    while next_start < end_window_start:
        cur_start, cur_size = next_start, next_size
        if 3 * cur_size <= end_window_start - cur_start:
            next_size = 2 * cur_size
        else:
            cur_size = end_window_start - cur_start
        next_start = cur_start + cur_size
        schedule.append((cur_start, next_start - 1))
    schedule.append((end_window_start, n - 1))
    return schedule


def window_metric(draws: np.ndarray, dense: bool = True) -> np.ndarray:
    """The inverse metric at the end of a slow window (Stan's regularised estimate, NumPyro's welford_covariance):
    Sigma = n / (n + 5) S + 1e-3 * 5 / (n + 5) I from the n draws (rows) of the window; ``dense=False`` keeps the
    diagonal."""
    n, d = draws.shape
    cov = np.cov(draws, rowvar=False).reshape(d, d) if n > 1 else np.zeros((d, d))
    cov = 0.5 * (cov + cov.T)
    if not dense:
        cov = np.diag(np.diag(cov))
    return n / (n + 5.0) * cov + 1e-3 * 5.0 / (n + 5.0) * np.eye(d)


def sample_GP_NUTS(gp, np_rng=None, rng_key=None, num_chains: int = 4, temp: float = 1.0, sampler: str = "hmc", **kwargs):
    """Samples of the posterior whose log-density is the GP mean / ``temp`` over the unit cube — the target, keywords
    and return dict of samplers.py:216-360 (``'x'`` of shape (num_chains * num_samples / thinning, d), ``'logp'``,
    ``'best'``, ``'method'``).

    Deviation: NumPyro's NUTS (one JAX call per leapfrog step and chain) is replaced by Hamiltonian Monte Carlo run
    as ONE batch of ``16 * num_chains`` chains that live on the device: a warm-up window or the whole sampling phase
    (momentum draws, 4-12 leapfrog steps per trajectory, Metropolis tests, per-chain step-size adaptation) is a single
    ``bobe_gp_hmc_run`` launch; ``device_chains=False`` steps trajectory by trajectory from the host
    (``bobe_gp_hmc_leapfrog``), ``fused_trajectories=False`` calls ``bobe_gp_predict_grad`` once per leapfrog step.  A
    classifier-gated GP takes the same paths: its gate lives in the library (``bobe_gp_set_gate``) and is applied inside
    the kernels.  Same stationary distribution; the per-chain length shrinks by the same factor so the number of returned
    samples is the reference's.  The cube constraint is handled like NumPyro does it, by sampling u = logit(x) with
    the Jacobian term; step size by dual averaging to 0.8 acceptance and a diagonal mass matrix from the warm-up
    spread of the chains.  Chains start at the best training point and at ``gp.get_random_point`` draws
    (samplers.py:296-300); a chain that is still tens of log units below the others at a warm-up window restarts from a
    healthy chain's state (``cull_lost_chains``, see the loop).  Works for ``GPwithClassifier`` too: infeasible points carry ``minus_inf`` and are never
    accepted.

    ``sampler="nuts"`` (opt-in; the default ``"hmc"`` is the path above) runs the reference's algorithm instead: NumPyro's
    multinomial No-U-Turn sampler with the generalised U-turn criterion, ``max_tree_depth`` (default 6) doublings at most
    and a dense metric (``dense_mass``, default True; False keeps its diagonal), whole transitions of the same chains in
    ``bobe_gp_nuts_run`` launches.  Warm-up follows Stan's windowed schedule (``adaptation_schedule``, one launch per
    window): per-chain dual averaging of the step size, and at the end of every slow window the regularised covariance of
    the window's draws (``window_metric``) pooled over the healthy chains - NumPyro estimates it per chain - then a
    restarted dual averaging.  NumPyro's ``find_reasonable_step_size`` is not run: the step size starts at 0.1 as on the
    HMC path.  There is no host-stepped NUTS: ``device_chains=False`` or ``fused_trajectories=False`` with it raise
    ``ValueError``."""
    if sampler not in ("hmc", "nuts"):
        raise ValueError(f"sampler must be 'hmc' or 'nuts', not {sampler!r}")
    if sampler == "nuts" and not (kwargs.get("device_chains", True) and kwargs.get("fused_trajectories", True)):
        raise ValueError("sampler='nuts' runs on the device only: device_chains and fused_trajectories must stay True")
    rng = np_rng if isinstance(np_rng, np.random.Generator) else np.random.default_rng(np_rng)
    d = gp.ndim
    warmup_steps, num_samples, thinning = get_hmc_settings(d, kwargs.get("warmup_steps"), kwargs.get("num_samples"),
                                                           kwargs.get("thinning"))
    mult = int(kwargs.get("chain_multiplier", 16))        # (64 = one chain per CU: no faster, profiles/HISTORY.md round 6)
    P = mult * max(1, int(num_chains))
    n_keep_total = max(1, (int(num_chains) * num_samples) // thinning)
    keep_per_chain = -(-n_keep_total // P)
    base_gp_grad = getattr(gp, "predict_grad")
    gated = hasattr(gp, "use_clf")
    # trajectories run on the device (bobe_gp_hmc_leapfrog / bobe_gp_hmc_run), gated or not: the library applies the
    # classifier's gate inside the kernels
    fused = hasattr(gp, "hmc_leapfrog") and kwargs.get("fused_trajectories", True)
    on_device = fused and hasattr(gp, "hmc_run") and kwargs.get("device_chains", True)

    def logp_and_grad(U):
        X = np.clip(expit(U), 1e-12, 1.0 - 1e-12)
        m, _, dm, _ = base_gp_grad(X, mean_only=True)
        mean = m * gp.y_std + gp.y_mean
        gx = dm * gp.y_std
        if gated:                                              # classifier gate (clf_gp.py:173-205): the library has
            bad = m <= gp.minus_inf                            # set the mean to minus_inf and zeroed its gradient
            mean = np.where(bad, gp.minus_inf, mean)
            gx = np.where(bad[:, None], 0.0, gx)
        jac = np.sum(np.log(X) + np.log1p(-X), axis=1)
        lp = mean / temp + jac
        g = gx / temp * (X * (1.0 - X)) + (1.0 - 2.0 * X)
        return lp, g, mean, X

    best = gp.train_x[int(np.argmax(gp.train_y))]
    inits = np.vstack([np.clip(best + 1e-3 * rng.normal(size=d), 1e-6, 1 - 1e-6)] +
                      [gp.get_random_point(rng=rng) for _ in range(P - 1)])
    inits = np.clip(inits, 1e-6, 1.0 - 1e-6)
    U = np.log(inits) - np.log1p(-inits)
    lp, g, mean, X = logp_and_grad(U)
    inv_mass = np.ones(d)
    total = warmup_steps + keep_per_chain * thinning
    if sampler == "nuts":
        if not hasattr(gp, "nuts_run"):
            raise ValueError("sampler='nuts' needs a surrogate with nuts_run (the GPU GP)")
        return _nuts_chains(gp, rng, U, g, X, lp, mean, warmup_steps, keep_per_chain, n_keep_total, thinning, temp,
                            int(kwargs.get("max_tree_depth", 6)), bool(kwargs.get("dense_mass", True)), kwargs)
    if on_device:
        # Whole chains on the device (bobe_gp_hmc_run): the host only cuts the warm-up at the mass-matrix windows and
        # pools the chains' spread there; every chain adapts its OWN step size (NumPyro does the same per chain).
        state = np.ascontiguousarray(np.concatenate([U, g, X, lp[:, None], mean[:, None]], axis=1))
        adapt = np.tile(np.array([0.1, math.log(1.0), 0.0, 0.0, 0.0]), (P, 1))
        seed = int(rng.integers(0, 2 ** 62))
        cuts = sorted({int(warmup_steps * f) for f in (0.25, 0.5, 0.75)} | {warmup_steps})
        it = 0
        for cut in cuts:
            n_it = cut - it
            if n_it <= 0:
                continue
            last = cut == warmup_steps
            hist, _, _ = gp.hmc_run(state, adapt, inv_mass, seed, it, n_it, True, temp,
                                    hist_from=None if last else n_it // 2)
            it = cut
            # Chains that never found the posterior: with 16 x num_chains chains started at uniform random points (the
            # reference's recipe, samplers.py:296-300) one now and then spends the whole warm-up on a plateau tens of log units
            # below the others (after the notebook run's first fit the surface is -103 everywhere but within a length scale of
            # the best point, -34.8: 3 of 8 runs kept one such chain, 1.6 % of the samples where the target puts e^-68).  At
            # every window such a chain restarts from the state of a randomly chosen healthy one (fresh momenta decorrelate
            # them within the window); ``cull_lost_chains=False`` switches this off.
            healthy = np.ones(P, dtype=bool)
            if kwargs.get("cull_lost_chains", True):
                lp_now = state[:, 3 * d]
                lost = ~(lp_now >= np.nanmax(lp_now) - (20.0 + 2.0 * d))
                if lost.any() and not lost.all():
                    healthy = ~lost
                    src = rng.choice(np.flatnonzero(healthy), size=int(lost.sum()))
                    state[lost] = state[src]
                    adapt[lost] = adapt[src]
            if not last:                                       # mass matrix from the spread of the batch (healthy chains)
                inv_mass = np.var(hist[:, healthy, :].reshape(-1, d), axis=0) + 1e-3
                # restart the dual averaging for the new metric (NumPyro / Stan do at every window): mu, hbar,
                # log_eps_bar AND the step counter m - with m left at several hundred, eta = m^-0.75 is ~0.01 and the
                # zeroed log_eps_bar keeps a quarter of its weight to the end of the warm-up (step size biased to 1)
                adapt[:, 1] = np.log(10.0 * adapt[:, 0])
                adapt[:, 2] = 0.0
                adapt[:, 3] = 0.0
                adapt[:, 4] = 0.0
        if warmup_steps > 0:                                   # the averaged step size of the warm-up
            adapt[:, 0] = np.where(adapt[:, 3] != 0.0, np.clip(np.exp(adapt[:, 3]), 1e-4, 2.0), adapt[:, 0])
        if isinstance(kwargs.get("diagnostics"), dict):        # (tests: the state the sampling phase starts from)
            kwargs["diagnostics"].update(eps=adapt[:, 0].copy(), inv_mass=np.array(inv_mass), state=state.copy(),
                                         adapt=adapt.copy(), seed=seed, it=it)
        _, keep, _ = gp.hmc_run(state, adapt, inv_mass, seed, it, keep_per_chain * thinning, False, temp, thin=thinning)
        samples_x = keep[:, :, :d].reshape(-1, d)[:n_keep_total]
        logps = keep[:, :, d].reshape(-1)[:n_keep_total]
        return {"x": samples_x, "logp": logps, "best": samples_x[int(np.argmax(logps))], "method": "MCMC"}
    # dual averaging (Hoffman & Gelman 2014, as NumPyro's warm-up does) on one step size shared by the batch
    eps, mu, hbar, log_eps_bar, t0, gamma, kappa, target = 0.1, math.log(1.0), 0.0, 0.0, 10.0, 0.05, 0.75, 0.8
    windows = {int(warmup_steps * f) for f in (0.25, 0.5, 0.75)}
    recent = []
    xs, lps = [], []
    da_start = 0                                               # first iteration of the current dual-averaging run
    for it in range(total):
        L = int(rng.integers(4, 13))
        p0 = rng.normal(size=U.shape) / np.sqrt(inv_mass)
        if fused:                                              # the whole trajectory of every chain in ONE launch
            Un, pn, lpn, gn, meann, Xn = gp.hmc_leapfrog(U, p0 + 0.5 * eps * g, inv_mass, eps, L, temp)
        else:
            Un, pn, gn = U.copy(), p0 + 0.5 * eps * g, g
            for s in range(L):
                Un = Un + eps * inv_mass * pn
                lpn, gn, meann, Xn = logp_and_grad(Un)
                pn = pn + (eps if s < L - 1 else 0.5 * eps) * gn
        h0 = lp - 0.5 * np.sum(p0 * p0 * inv_mass, axis=1)
        h1 = lpn - 0.5 * np.sum(pn * pn * inv_mass, axis=1)
        with np.errstate(over="ignore", invalid="ignore"):
            acc_prob = np.where(np.isfinite(h1), np.minimum(1.0, np.exp(h1 - h0)), 0.0)
        accept = rng.uniform(size=P) < acc_prob
        U = np.where(accept[:, None], Un, U)
        g = np.where(accept[:, None], gn, g)
        lp = np.where(accept, lpn, lp)
        mean = np.where(accept, meann, mean)
        X = np.where(accept[:, None], Xn, X)
        if it < warmup_steps:
            m_ = it + 1 - da_start                             # steps since the averaging was (re)started
            hbar = (1.0 - 1.0 / (m_ + t0)) * hbar + (target - float(np.mean(acc_prob))) / (m_ + t0)
            log_eps = mu - math.sqrt(m_) / gamma * hbar
            eta = m_ ** (-kappa)
            log_eps_bar = eta * log_eps + (1.0 - eta) * log_eps_bar
            eps = float(np.clip(math.exp(log_eps), 1e-4, 2.0))
            recent.append(U.copy())
            if it + 1 in windows:                              # mass matrix from the spread of the batch
                pool = np.concatenate(recent[len(recent) // 2:], axis=0)
                inv_mass = np.var(pool, axis=0) + 1e-3
                recent = []
                mu, hbar, log_eps_bar = math.log(10.0 * eps), 0.0, 0.0
                da_start = it + 1                              # ... and its step counter (see the device path)
            if it + 1 == warmup_steps:
                eps = float(np.clip(math.exp(log_eps_bar), 1e-4, 2.0)) if log_eps_bar != 0.0 else eps
        elif (it - warmup_steps + 1) % thinning == 0:
            xs.append(X.copy())
            lps.append(mean.copy())
    samples_x = np.concatenate(xs, axis=0)[:n_keep_total]
    logps = np.concatenate(lps, axis=0)[:n_keep_total]
    return {"x": samples_x, "logp": logps, "best": samples_x[int(np.argmax(logps))], "method": "MCMC"}


def _nuts_chains(gp, rng, U, g, X, lp, mean, warmup_steps, keep_per_chain, n_keep_total, thinning, temp, max_tree_depth,
                 dense_mass, kwargs) -> Dict:
    """The NUTS path of ``sample_GP_NUTS``: the chains of the HMC path, windowed warm-up, then the sampling launch."""
    P, d = U.shape
    state = np.ascontiguousarray(np.concatenate([U, g, X, lp[:, None], mean[:, None]], axis=1))
    adapt = np.tile(np.array([0.1, math.log(1.0), 0.0, 0.0, 0.0]), (P, 1))
    inv_metric = np.eye(d)
    seed = int(rng.integers(0, 2 ** 62))
    schedule = adaptation_schedule(warmup_steps)
    for w, (start, end) in enumerate(schedule):
        slow = 0 < w < len(schedule) - 1
        hist, _, _, _ = gp.nuts_run(state, adapt, inv_metric, max_tree_depth, seed, start, end - start + 1, True, temp,
                                    hist_from=0 if slow else None)
        healthy = np.ones(P, dtype=bool)
        if kwargs.get("cull_lost_chains", True):               # (as on the HMC path)
            lp_now = state[:, 3 * d]
            lost = ~(lp_now >= np.nanmax(lp_now) - (20.0 + 2.0 * d))
            if lost.any() and not lost.all():
                healthy = ~lost
                src = rng.choice(np.flatnonzero(healthy), size=int(lost.sum()))
                state[lost] = state[src]
                adapt[lost] = adapt[src]
        if slow:                                               # pooled metric, restarted dual averaging
            inv_metric = window_metric(hist[:, healthy, :].reshape(-1, d), dense=dense_mass)
            adapt[:, 1] = np.log(10.0 * adapt[:, 0])
            adapt[:, 2:5] = 0.0
    if warmup_steps > 0:                                       # the averaged step size of the warm-up
        adapt[:, 0] = np.where(adapt[:, 3] != 0.0, np.clip(np.exp(adapt[:, 3]), 1e-4, 2.0), adapt[:, 0])
    if isinstance(kwargs.get("diagnostics"), dict):
        kwargs["diagnostics"].update(eps=adapt[:, 0].copy(), inv_metric=inv_metric.copy(), state=state.copy(),
                                     adapt=adapt.copy(), seed=seed, it=warmup_steps, schedule=schedule)
    _, keep, stats, _ = gp.nuts_run(state, adapt, inv_metric, max_tree_depth, seed, warmup_steps,
                                    keep_per_chain * thinning, False, temp, thin=thinning,
                                    stats=isinstance(kwargs.get("diagnostics"), dict))
    if stats is not None:
        kwargs["diagnostics"].update(stats=stats)
    samples_x = keep[:, :, :d].reshape(-1, d)[:n_keep_total]
    logps = keep[:, :, d].reshape(-1)[:n_keep_total]
    return {"x": samples_x, "logp": logps, "best": samples_x[int(np.argmax(logps))], "method": "MCMC"}


# --------------------------------------------------------------------------------------------------------------
# HMC on pathwise posterior draws of the surrogate (PosteriorPaths.hmc_run, bobe_gp_paths_hmc_run)
# --------------------------------------------------------------------------------------------------------------
def _check_paths_hmc_args(n_paths, d, chains_per_path, warmup_steps, num_samples, thinning, temp, init):
    """The argument rules of ``sample_paths_hmc``; returns ``init`` as an (S, R, d) array or None.  Raises ``ValueError``
    before anything touches the device."""
    if int(chains_per_path) != chains_per_path or chains_per_path < 1:
        raise ValueError(f"chains_per_path must be a positive integer, not {chains_per_path!r}")
    if not (np.isfinite(temp) and temp > 0.0):
        raise ValueError(f"temp must be positive and finite, not {temp!r}")
    if warmup_steps is not None and warmup_steps < 0:
        raise ValueError("warmup_steps must be non-negative")
    if num_samples is not None and num_samples < 1:
        raise ValueError("num_samples must be positive")
    if thinning is not None and thinning < 1:
        raise ValueError("thinning must be positive")
    if init is None:
        return None
    init = np.asarray(init, dtype=np.float64)
    R = int(chains_per_path)
    if init.shape == (R, d):
        init = np.broadcast_to(init, (n_paths, R, d))
    if init.shape != (n_paths, R, d):
        raise ValueError(f"init must have shape ({R}, {d}) or ({n_paths}, {R}, {d}), not {init.shape}")
    if not np.all(np.isfinite(init)) or np.any(init < 0.0) or np.any(init > 1.0):
        raise ValueError("init must lie in the unit cube")
    return np.array(init)


def _pool_paths_window(state, adapt, hist, inv_mass, n_paths, rng, cull, update_mass):
    """What ``sample_paths_hmc`` does at the end of a warm-up window, PER PATH (chains s R .. (s + 1) R - 1 belong to path
    s): a chain more than 20 + 2 d log units below its path's best restarts from the state of a randomly chosen healthy
    chain of the SAME path (``cull``); with ``update_mass`` the rows of ``inv_mass`` of the path become the variance of the
    window's recorded positions ``hist`` (T, P, d) over its healthy chains + 1e-3.  In place; returns the healthy mask."""
    P, d = inv_mass.shape
    R = P // n_paths
    healthy_all = np.ones(P, dtype=bool)
    for s in range(n_paths):
        sel = np.arange(s * R, (s + 1) * R)
        healthy = np.ones(R, dtype=bool)
        if cull:
            lp_now = state[sel, 3 * d]
            with np.errstate(invalid="ignore"):
                top = np.max(np.where(np.isnan(lp_now), -np.inf, lp_now))
                lost = ~(lp_now >= top - (20.0 + 2.0 * d))
            if lost.any() and not lost.all():
                healthy = ~lost
                src = rng.choice(sel[healthy], size=int(lost.sum()))
                state[sel[lost]] = state[src]
                adapt[sel[lost]] = adapt[src]
        if update_mass:
            inv_mass[sel] = np.var(hist[:, sel[healthy], :].reshape(-1, d), axis=0) + 1e-3
        healthy_all[sel] = healthy
    return healthy_all


def sample_paths_hmc(paths, chains_per_path: int = 16, warmup_steps=None, num_samples=None, thinning=None,
                     temp: float = 1.0, rng=None, init=None, cull_lost_chains: bool = True, diagnostics=None) -> Dict:
    """HMC samples of the posterior implied by every DRAW of the surrogate: for each of the S paths of ``paths`` (a
    ``PosteriorPaths`` set) the density exp(f_s(x) / temp) over the unit cube, f_s in the snapshot's physical units.

    S x ``chains_per_path`` chains run as ONE batch on the device (``PosteriorPaths.hmc_run``: a warm-up window or the whole
    sampling phase is one launch), with the window cuts (25 / 50 / 75 / 100 % of the warm-up) and the dual-averaging
    restarts of the device branch of ``sample_GP_NUTS``.  The diagonal mass matrix and the lost-chain cull are pooled PER
    PATH: paths differ in shape, so a path's chains share one inverse mass and a lost chain restarts from a healthy chain
    of its own path.  Starts: ``init`` (shape (R, d), the same for every path, or (S, R, d); unit-cube coordinates), else per
    path the best training point of the set's GP and R - 1 ``get_random_point`` draws.  ``warmup_steps``, ``num_samples``,
    ``thinning``: ``get_hmc_settings``; every path returns n = max(1, num_samples // thinning) samples.  ``rng``: a NumPy
    generator or a seed.  A classifier gate set on the GP at call time applies (the gate is not part of the snapshot).

    Returns ``{'x': (S, n, d), 'logp': (S, n) - y_mean + y_std f_s at the samples -, 'best': (S, d), 'method': 'MCMC-paths'}``."""
    S, d = int(paths.n_paths), int(paths.ndim)
    init = _check_paths_hmc_args(S, d, chains_per_path, warmup_steps, num_samples, thinning, temp, init)
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    warmup_steps, num_samples, thinning = get_hmc_settings(d, warmup_steps, num_samples, thinning)
    warmup_steps, num_samples, thinning = int(warmup_steps), int(num_samples), int(thinning)
    R = int(chains_per_path)
    P = S * R
    n_keep = max(1, num_samples // thinning)
    keep_per_chain = -(-n_keep // R)
    path_index = np.repeat(np.arange(S, dtype=np.int64), R)
    if init is None:
        gp = paths.gp
        best = gp.train_x[int(np.argmax(gp.train_y))]
        init = np.empty((S, R, d))
        for s in range(S):
            init[s, 0] = np.clip(best + 1e-3 * rng.normal(size=d), 1e-6, 1 - 1e-6)
            for r in range(1, R):
                init[s, r] = gp.get_random_point(rng=rng)
    X0 = np.clip(init.reshape(P, d), 1e-6, 1.0 - 1e-6)
    U = np.log(X0) - np.log1p(-X0)
    state = paths.hmc_state(U, path_index, temp)
    adapt = np.tile(np.array([0.1, math.log(1.0), 0.0, 0.0, 0.0]), (P, 1))
    inv_mass = np.ones((P, d))
    seed = int(rng.integers(0, 2 ** 62))
    cuts = sorted({int(warmup_steps * f) for f in (0.25, 0.5, 0.75)} | {warmup_steps})
    it = 0
    for cut in cuts:
        n_it = cut - it
        if n_it <= 0:
            continue
        last = cut == warmup_steps
        hist, _, _ = paths.hmc_run(state, adapt, inv_mass, path_index, seed, it, n_it, True, temp,
                                   hist_from=None if last else n_it // 2)
        it = cut
        _pool_paths_window(state, adapt, hist, inv_mass, S, rng, cull_lost_chains, not last)
        if not last:                                           # restarted dual averaging for the new metric
            adapt[:, 1] = np.log(10.0 * adapt[:, 0])
            adapt[:, 2:5] = 0.0
    if warmup_steps > 0:                                       # the averaged step size of the warm-up
        adapt[:, 0] = np.where(adapt[:, 3] != 0.0, np.clip(np.exp(adapt[:, 3]), 1e-4, 2.0), adapt[:, 0])
    if isinstance(diagnostics, dict):
        diagnostics.update(eps=adapt[:, 0].copy(), inv_mass=inv_mass.copy(), state=state.copy(), adapt=adapt.copy(),
                           seed=seed, it=it, path_index=path_index.copy())
    _, keep, _ = paths.hmc_run(state, adapt, inv_mass, path_index, seed, it, keep_per_chain * thinning, False, temp,
                               thin=thinning)
    keep = keep.reshape(keep_per_chain, S, R, d + 1).transpose(1, 0, 2, 3).reshape(S, keep_per_chain * R, d + 1)[:, :n_keep]
    x, logp = np.ascontiguousarray(keep[:, :, :d]), np.ascontiguousarray(keep[:, :, d])
    if isinstance(diagnostics, dict):                          # (per-chain means: the tests' standard errors)
        diagnostics.update(chains_per_path=R, keep_per_chain=keep_per_chain)
    best = x[np.arange(S), np.argmax(logp, axis=1)]
    return {"x": x, "logp": logp, "best": best, "method": "MCMC-paths"}


def path_posterior_summary(samples, param_bounds=None) -> Dict:
    """Moments of the per-path posteriors ``sample_paths_hmc`` returns (its dict, or an (S, n, d) array of samples in the
    unit cube; ``param_bounds`` (2, d) maps them to physical parameters first): ``mean`` (S, d), ``cov`` (S, d, d) and
    ``std`` (S, d) per path, and the surrogate-induced uncertainty of the constraints - ``mean_of_means`` (d,),
    ``std_of_means`` (d,) and ``std_of_stds`` (d,), the across-path standard deviations (ddof 1; 0 for a single path) of
    the per-path means and marginal standard deviations - with ``mean_of_stds`` (d,) and ``n_paths``."""
    x = np.asarray(samples["x"] if isinstance(samples, dict) else samples, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] < 2:
        raise ValueError(f"samples must have shape (S, n >= 2, d), not {x.shape}")
    S, n, d = x.shape
    if param_bounds is not None:
        b = np.asarray(param_bounds, dtype=np.float64)
        if b.shape != (2, d):
            raise ValueError(f"param_bounds must have shape (2, {d}), not {b.shape}")
        x = b[0] + x * (b[1] - b[0])
    mean = x.mean(axis=1)
    dev = x - mean[:, None, :]
    cov = np.einsum("sni,snj->sij", dev, dev) / (n - 1)
    std = np.sqrt(np.einsum("sii->si", cov))
    ddof = 1 if S > 1 else 0
    return {"mean": mean, "cov": cov, "std": std, "mean_of_means": mean.mean(axis=0), "std_of_means": mean.std(axis=0, ddof=ddof),
            "mean_of_stds": std.mean(axis=0), "std_of_stds": std.std(axis=0, ddof=ddof), "n_paths": S}
