"""Acquisition functions on top of the GPU GP — counterpart of BOBE/acquisition.py.

WIPV / WIPStd evaluate every candidate in ONE call of ``bobe_gp_wip_sweep`` (the reference maps
``fun`` over the candidates sequentially with ``lax.map``, acquisition.py:390-394).  EI / LogEI are
pointwise scorers on the batched posterior (``bobe_gp_acq_ei``).

Where the reference differentiates ``fun`` with JAX the build has explicit gradient entry points: EI / LogEI
restarts (acquisition.py:281-290) use the analytic posterior gradients of ``bobe_gp_predict_grad``, the WIPV /
WIPStd local refinement for N <= 500 (acquisition.py:403-412) the analytic score gradients of
``bobe_gp_wip_grad``.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np
from scipy.stats import qmc

from . import _lib
from .gp import GP
from .optim import optimize_optax, optimize_scipy
from .utils import get_logger, get_numpy_rng

log = get_logger("acq")



class AcquisitionFunction:
    """BOBE/acquisition.py:79-196."""

    name: str = "BaseAcquisitionFunction"

    def __init__(self, optimizer: str = "scipy", optimizer_options: Optional[Dict[str, Any]] = None):
        self.optimizer = optimizer
        self.optimizer_options = optimizer_options if optimizer_options is not None else {}
        self.acq_optimize = optimize_scipy if optimizer == "scipy" else optimize_optax      # acquisition.py:101-104

    def fun(self, x, *args, **kwargs):
        raise NotImplementedError

    def get_next_point(self, gp: GP, acq_kwargs=None, maxiter=500, n_restarts=8, verbose=True,
                       early_stop_patience=25, rng=None):
        raise NotImplementedError("Base class get_next() not implemented")

    def get_next_batch(self, gp: GP, n_batch: int = 1, acq_kwargs=None, maxiter: int = 500, n_restarts: int = 8,
                       verbose: bool = True, early_stop_patience: int = 25, rng=None):
        """Kriging-believer batch (BOBE/acquisition.py:147-196)."""
        rng = rng if rng is not None else get_numpy_rng()
        acq_kwargs = acq_kwargs if acq_kwargs is not None else {}
        x_batch, acq_vals = [], []
        x_next, val = self.get_next_point(gp, acq_kwargs=acq_kwargs, maxiter=maxiter, n_restarts=n_restarts,
                                          verbose=verbose, early_stop_patience=early_stop_patience, rng=rng)
        x_batch.append(np.asarray(x_next))
        acq_vals.append(val)
        if n_batch > 1:
            dummy_gp = _believer_gp(gp)                                        # acquisition.py:175-180
            dummy_gp.update(x_next, dummy_gp.predict_mean_single(x_next))
            for member in range(1, n_batch):
                x_next, val = self.get_next_point(dummy_gp, acq_kwargs=acq_kwargs, maxiter=maxiter,
                                                  n_restarts=n_restarts, verbose=verbose,
                                                  early_stop_patience=early_stop_patience, rng=rng)
                x_batch.append(np.asarray(x_next))
                acq_vals.append(val)
                if member + 1 < n_batch:      # (the reference also updates after the LAST member, acquisition.py:194: the dummy
                    dummy_gp.update(x_next, dummy_gp.predict_mean_single(x_next))     # GP is dropped right after - not done here)
        return np.array(x_batch), np.array(acq_vals)


def _believer_gp(gp: GP) -> GP:
    """The plain GP the kriging believer works on (acquisition.py:175-180: same data, kernel and hyper-parameters as ``gp``,
    default priors).  The reference constructs a new one per batch, i.e. standardises and factorises again; here ONE scratch
    GP per surrogate is kept and brought to ``gp``'s state on the device (``bobe_gp_clone_state``: data, L, L^-1, alpha
    copied, no factorisation).  Creating and destroying a handle costs ~40 hipMalloc / hipFree calls - 6 of the 16 ms of a
    batch of five at N = 400 (tools/acq_host_profile.py)."""
    if gp._pushed_hyper != gp._hyper_key():          # attributes changed by hand since the last factorisation: the reference's
        return GP(train_x=gp.train_x, train_y=gp.train_y * gp.y_std + gp.y_mean, noise=gp.noise, kernel=gp.kernel_name,
                  lengthscales=gp.lengthscales, kernel_variance=gp.kernel_variance, device=gp.device)   # dummy sees the new ones
    d = getattr(gp, "_believer_scratch", None)
    if d is None or d.ndim != gp.ndim or d.kernel_name != gp.kernel_name or d.device != gp.device:
        d = GP(train_x=gp.train_x, train_y=gp.train_y * gp.y_std + gp.y_mean, noise=gp.noise, kernel=gp.kernel_name,
               lengthscales=gp.lengthscales, kernel_variance=gp.kernel_variance, device=gp.device, _factor=False)
        gp._believer_scratch = d
    d.train_x, d.train_y = np.array(gp.train_x), np.array(gp.train_y)
    d.y_mean, d.y_std = gp.y_mean, gp.y_std
    d.lengthscales, d.kernel_variance, d.noise = np.array(gp.lengthscales), float(gp.kernel_variance), float(gp.noise)
    _lib.check(d._lib.bobe_gp_clone_state(d._h, gp._h), "bobe_gp_clone_state")
    d.not_pd = bool(gp.not_pd)
    d._pushed_hyper = gp._pushed_hyper
    d._chol_cache = d._alpha_cache = None
    return d


class EI(AcquisitionFunction):
    """BOBE/acquisition.py:199-291."""

    name: str = "EI"
    _log = False

    def fun(self, x, gp, best_y, zeta):
        """-EI(x) (acquisition.py:226-253); x may be (d,) or (C, d)."""
        val = -gp.acq_ei(np.atleast_2d(x), best_y, zeta, log_ei=self._log)
        return val[0] if np.ndim(x) == 1 else val

    def _value_and_grad(self, gp, best_y, zeta):
        """(-EI, d(-EI)/dx) or (-logEI, ...) from the GPU's analytic posterior gradients (bobe_gp_predict_grad):
        dEI = Phi(u) dmu + phi(u) dsigma, u = (mu - zeta - best)/sigma; logEI through log-space ratios."""
        from scipy.special import log_ndtr
        lo = 1e-18 if self._log else 1e-20                      # acquisition.py:247, 324

        def vg(x):
            x = np.asarray(x, dtype=np.float64)
            m, v, dm, dv = gp.predict_grad(x[None, :])
            m, v, dm, dv = float(m[0]), float(v[0]), dm[0], dv[0]
            clipped = v < lo
            v = max(v, lo)
            sigma = np.sqrt(v)
            dsig = np.zeros_like(dv) if clipped else dv / (2.0 * sigma)
            u = (m - zeta - best_y) / sigma
            log_phi = -0.5 * u * u - 0.5 * np.log(2.0 * np.pi)
            log_Phi = float(log_ndtr(u))
            if not self._log:
                val = -float(gp.acq_ei(x[None, :], best_y, zeta, log_ei=False)[0])
                return val, -(np.exp(log_Phi) * dm + np.exp(log_phi) * dsig)
            log_ei = float(gp.acq_ei(x[None, :], best_y, zeta, log_ei=True)[0])       # = log h(u) + log sigma
            # d logEI = (Phi dmu + phi dsigma) / EI, with EI = exp(log_ei)
            grad = np.exp(log_Phi - log_ei) * dm + np.exp(log_phi - log_ei) * dsig
            return -log_ei, -grad
        return vg

    def _lockstep_value_and_grad(self, gp, best_y, zeta):
        """(vg, batch_vg) on ``GP.acq_ei_grad``: the negated value and gradient of one point, and of every point handed
        over in ONE device call - value and gradient from the same posterior, nothing assembled on the host."""
        def batch_vg(xs):
            val, grad = gp.acq_ei_grad(np.asarray(xs, dtype=np.float64), best_y, zeta, log_ei=self._log)
            return [(-float(v), -g) for v, g in zip(val, grad)]

        def vg(x):
            return batch_vg([np.asarray(x, dtype=np.float64)])[0]
        return vg, batch_vg

    def get_next_point(self, gp, acq_kwargs=None, maxiter: int = 250, n_restarts: int = 20, verbose: bool = True,
                       early_stop_patience: int = 25, rng=None):
        """``acq_kwargs['ei_lockstep']`` (default off: the loop below as ever, one restart after the other on
        ``predict_grad`` + ``acq_ei``): the same starts, drawn by the same calls on ``rng``, with all restarts advancing in
        lock step on ``GP.acq_ei_grad`` - the screening and every L-BFGS-B round are one device call
        (``optimize_scipy(batch_value_and_grad=)``); restart order, acceptance rule and return value are unchanged."""
        rng = rng if rng is not None else get_numpy_rng()
        acq_kwargs = acq_kwargs if acq_kwargs is not None else {}
        lockstep = bool(acq_kwargs.get("ei_lockstep", False))
        if lockstep and self.optimizer != "scipy":
            raise ValueError(f"acq_kwargs['ei_lockstep'] needs optimizer='scipy', not {self.optimizer!r}")
        zeta = acq_kwargs.get("zeta", 0.0)
        best_y = acq_kwargs.get("best_y", float(np.max(gp.train_y)))
        best_x = gp.train_x[int(np.argmax(gp.train_y))]
        if n_restarts > 1:                                                     # acquisition.py:271-278
            n_random = int(n_restarts / 2)
            x0 = np.vstack([gp.get_random_point(rng, nstd=5) for _ in range(n_random)])
            x0 = np.vstack([x0, np.full((n_restarts - n_random, gp.ndim), best_x)])
        else:
            x0 = np.atleast_2d(best_x)
        x0 = np.clip(x0 + rng.normal(0.0, 0.005, size=x0.shape), 0.0, 1.0)
        if lockstep:
            vg, batch_vg = self._lockstep_value_and_grad(gp, best_y, zeta)
            pts, vals = optimize_scipy(vg, num_params=gp.ndim, x0=x0, bounds=[0, 1],
                                       optimizer_options=dict(self.optimizer_options), maxiter=maxiter,
                                       n_restarts=n_restarts, verbose=verbose, batch_value_and_grad=batch_vg)
            return pts, -vals
        pts, vals = self.acq_optimize(self._value_and_grad(gp, best_y, zeta), num_params=gp.ndim, x0=x0,
                                      bounds=[0, 1], optimizer_options=dict(self.optimizer_options),
                                      maxiter=maxiter, n_restarts=n_restarts, verbose=verbose)
        return pts, -vals


class LogEI(EI):
    """BOBE/acquisition.py:293-330."""

    name: str = "LogEI"
    _log = True


class WeightedIntegratedPosteriorBase(AcquisitionFunction):
    """BOBE/acquisition.py:333-412."""

    _key = "wipv"
    _pool_only_logged = False

    def _weighted(self, log_weights) -> bool:
        """True where the scores come from ``bobe_gp_wip_sweep_w`` / ``bobe_gp_wip_sweep_zvar``: IMIQR / EIV / ZVar, or
        integration points with log-weights."""
        return self._key in ("imiqr", "eiv", "zvar") or log_weights is not None

    def fun(self, x, gp, mc_points=None, k_train_mc=None, *, log_weights=None):
        if self._weighted(log_weights):
            r = gp.wip_sweep(np.atleast_2d(x), mc_points, log_weights=log_weights, criteria=(self._key,))
        else:
            r = gp.wip_sweep(np.atleast_2d(x), mc_points)
        return r[self._key][0] if np.ndim(x) == 1 else r[self._key]

    def sweep(self, gp, candidates, mc_points, *, log_weights=None):
        """Scores of all candidates and the argmin (acquisition.py:394-398)."""
        if self._weighted(log_weights):
            r = gp.wip_sweep(candidates, mc_points, log_weights=log_weights, criteria=(self._key,))
            return r[self._key], r["argmin_" + self._key]
        r = gp.wip_sweep(candidates, mc_points)
        idx = r["argmin_v"] if self._key == "wipv" else r["argmin_s"]
        return r[self._key], idx

    def sweep_best(self, gp, candidates, mc_points, group=None, *, log_weights=None):
        """(best score, index of the best candidate).  With an initialised ``torch.distributed`` group of G > 1
        ranks every rank scores its contiguous shard of the candidates on its own GPU (same factor everywhere) and
        one all-gather of (min score, global index) picks the winner, ties to the lowest index like
        ``jnp.argmin`` (acquisition.py:397)."""
        from .dist_sweep import dist_info, sharded_wip_sweep
        world, _, coll_dev = dist_info(group, gp.device)
        if world > 1 and candidates.shape[0] >= world:
            _, gmin, gidx = sharded_wip_sweep(lambda c: self.sweep(gp, c, mc_points, log_weights=log_weights), candidates,
                                              group=group, device=coll_dev)
            return float(gmin), int(gidx)
        vals, idx = self.sweep(gp, candidates, mc_points, log_weights=log_weights)
        return float(vals[idx]), int(idx)

    @staticmethod
    def _integration_points(acq_kwargs, rng):
        """(mc_points, log_weights).  ``acq_kwargs['mc_log_weights']`` belongs to explicit ``acq_kwargs['mc_points']`` (what
        ``get_mc_points(weighted=True)`` returns); without it the points are drawn as ever (``acq_kwargs['mc_points']`` is not
        looked at) and carry no weights."""
        lw = acq_kwargs.get("mc_log_weights")
        if lw is not None:
            if acq_kwargs.get("mc_points") is None:
                raise ValueError("acq_kwargs['mc_log_weights'] needs the points it belongs to in acq_kwargs['mc_points']")
            return np.asarray(acq_kwargs["mc_points"]), lw
        return get_mc_points(acq_kwargs.get("mc_samples"), mc_points_size=acq_kwargs.get("mc_points_size", 128), rng=rng), None

    def get_next_batch(self, gp: GP, n_batch: int = 1, acq_kwargs=None, maxiter: int = 500, n_restarts: int = 8,
                       verbose: bool = True, early_stop_patience: int = 25, rng=None, *, batch_mode: str = "believer"):
        """``batch_mode='believer'`` (default): the inherited kriging-believer loop, unchanged - ``n_batch`` sweeps of the
        integration points, each on a surrogate that gained the previous pick.

        ``batch_mode='sweep'``: the same believer batch out of ONE sweep (``GP.wip_select_batch``).  One set of integration
        points is drawn (one ``get_mc_points`` call, where the loop draws one per member); the candidates are
        ``acq_kwargs['candidates']`` or, without that key, all of ``mc_samples['x']``; the picks are rows of that pool (no
        L-BFGS polish, whatever the size of the design).  Returns ``(x_batch (n_batch, d), acq_vals (n_batch,))`` like the
        loop, the values in the caller's units (``y_std`` held fixed over the batch)."""
        if batch_mode == "believer":
            return super().get_next_batch(gp, n_batch=n_batch, acq_kwargs=acq_kwargs, maxiter=maxiter,
                                          n_restarts=n_restarts, verbose=verbose,
                                          early_stop_patience=early_stop_patience, rng=rng)
        if batch_mode != "sweep":
            raise ValueError(f"batch_mode must be 'believer' or 'sweep', not {batch_mode!r}")
        acq_kwargs = acq_kwargs if acq_kwargs is not None else {}
        mc_samples = acq_kwargs.get("mc_samples")
        mc_points, log_weights = self._integration_points(acq_kwargs, rng)
        candidates = acq_kwargs.get("candidates")
        if candidates is None:
            candidates = mc_samples["x"]
        if log_weights is None and self._key != "zvar":
            r = gp.wip_select_batch(candidates, mc_points, n_batch, criterion=self._key)
        else:
            r = gp.wip_select_batch_w(candidates, mc_points, n_batch, criterion=self._key, log_weights=log_weights)
        return np.array(r["points"]), np.array(r["scores"])

    def get_next_point(self, gp, acq_kwargs=None, maxiter: int = 100, n_restarts: int = 1, verbose: bool = True,
                       early_stop_patience: int = 25, rng=None):
        """``acq_kwargs['weighted_polish'] = R`` (default 0: the pool pick, as ever) carries a weighted pick - IMIQR / EIV, or
        integration points with log-weights - to the continuum: ``_polished_point``."""
        acq_kwargs = acq_kwargs if acq_kwargs is not None else {}
        polish = _weighted_polish(acq_kwargs)
        mc_points, log_weights = self._integration_points(acq_kwargs, rng)
        if polish > 0 and self._weighted(log_weights):
            vals, idx = self.sweep(gp, mc_points, mc_points, log_weights=log_weights)      # every score: the starts come from them
            return self._polished_point(gp, np.asarray(mc_points), log_weights, np.asarray(vals), int(idx), polish,
                                        int(acq_kwargs.get("weighted_polish_maxiter", 100)))
        best_val, idx = self.sweep_best(gp, mc_points, mc_points, log_weights=log_weights)   # candidates == integration points
        best_x = np.array(mc_points[idx])
        if self._weighted(log_weights):
            # (without acq_kwargs['weighted_polish'] the weighted scores stay on the pool)
            if not self._pool_only_logged:                 # (once per acquisition object: BOBE.run makes one per stage)
                log.info(f"{self.name}: weighted scores pick from the candidate pool, without the L-BFGS polish")
                self._pool_only_logged = True
            return best_x, best_val
        if gp.train_x.shape[0] > 500:                                          # acquisition.py:400-401
            return best_x, best_val

        def vg(x):                                    # value and exact gradient in one call (bobe_gp_wip_grad)
            wv, ws, dv, ds = gp.wip_grad(np.asarray(x, dtype=np.float64)[None, :], mc_points)
            return (float(wv[0]), dv[0]) if self._key == "wipv" else (float(ws[0]), ds[0])
        return self.acq_optimize(vg, num_params=gp.ndim, x0=best_x, bounds=[0, 1],
                                 optimizer_options=dict(self.optimizer_options), maxiter=maxiter,
                                 n_restarts=n_restarts, verbose=verbose)

    _grad_entry = "bobe_gp_wip_grad_w"

    def _score_and_grad(self, gp, x, mc_points, log_weights):
        """(scores (C,), gradients (C, d)) of this criterion alone at the rows of x: what ``_polished_point`` minimises."""
        r = gp.wip_grad_w(x, mc_points, log_weights=log_weights, criteria=(self._key,))
        return r[self._key], r["d" + self._key]

    def _polished_point(self, gp, mc_points, log_weights, vals, idx, n_starts, maxiter):
        """``weighted_polish`` (ZVar: ``zvar_polish``) = R > 0: SciPy's L-BFGS-B on the score over the unit cube from the R pool rows with the lowest
        score (ties: the lower index), all runs in lock step (the drivers of optim.py) - every round ONE ``GP.wip_grad_w``
        (ZVar: ``GP.wip_grad_zvar``) call on the points still waiting, this criterion alone.  Returns the lowest value among the restarts that finished and
        the pool pick itself; ties go to the pool pick, then to the lower restart; a restart that raised or ended non-finite is
        skipped - never worse than the pool pick.  Nothing is drawn from a generator.  A design above the entry's limit on N
        keeps the pool pick (one log line).  Not gated (nor is the equal-weight polish)."""
        from .optim import _minimize_concurrently
        best_x, best_val = np.array(mc_points[idx]), float(vals[idx])
        if gp.train_x.shape[0] > WIP_GRAD_W_MAX_N:
            log.info(f"{self.name}: {gp.train_x.shape[0]} training points exceed {self._grad_entry}'s limit of "
                     f"{WIP_GRAD_W_MAX_N}; the pick stays on the candidate pool")
            return best_x, best_val
        d = mc_points.shape[1]
        order = np.argsort(vals, kind="stable")[:min(int(n_starts), len(vals))]
        starts = np.clip(np.asarray(mc_points[order], dtype=np.float64), 0.0, 1.0)

        def batch(ids, xs):
            fs, gs = self._score_and_grad(gp, np.array(xs, dtype=np.float64).reshape(len(ids), d), mc_points, log_weights)
            return [(float(f), np.array(g, dtype=np.float64)) for f, g in zip(fs, gs)]

        results = _minimize_concurrently(batch, starts, True, with_ids=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * d,
                                         options={"maxiter": int(maxiter)})
        for res in results:
            if isinstance(res, Exception) or res is None or not np.isfinite(res.fun) or not np.all(np.isfinite(res.x)):
                continue
            if float(res.fun) < best_val:
                best_x, best_val = np.clip(np.array(res.x, dtype=np.float64), 0.0, 1.0), float(res.fun)
        return best_x, best_val


class WIPV(WeightedIntegratedPosteriorBase):
    """BOBE/acquisition.py:415-440."""
    name: str = "WIPV"
    _key = "wipv"


class WIPStd(WeightedIntegratedPosteriorBase):
    """BOBE/acquisition.py:443-465."""
    name: str = "WIPStd"
    _key = "wipstd"


class IMIQR(WeightedIntegratedPosteriorBase):
    """The integrated median interquartile range of the lognormal likelihood estimate exp(f) (Jarvenpaa, Gutmann, Vehtari,
    Marttinen, Bayesian Analysis 2021; no counterpart in the reference): ``log sum_z e^{a_z} 2 sinh(u sqrt(v+))``, of which
    WIPStd is the small-sigma linearisation.  Picks from the candidate pool; ``acq_kwargs['weighted_polish']`` refines the pick."""
    name: str = "IMIQR"
    _key = "imiqr"


class EIV(WeightedIntegratedPosteriorBase):
    """The expected integrated variance of exp(f) (same paper), as the negative log of the candidate's gain R(c): EIV = S -
    R(c) with log S = ``wip_sweep(...)['log_eiv_total']``.  Picks from the candidate pool; ``acq_kwargs['weighted_polish']`` refines
    the pick."""
    name: str = "EIV"
    _key = "eiv"


class ZVar(WeightedIntegratedPosteriorBase):
    """The expected posterior variance of the evidence estimate Z = sum_z e^{l_z} e^{f(z)} after one more evaluation - the
    Bayesian-quadrature criterion for the lognormal estimate exp(f), which counts the correlation of the surrogate's errors
    between integration points where WIPV / WIPStd / IMIQR / EIV integrate a pointwise variance (no counterpart in the
    reference).  The score is ``zvar`` = -log T(c) of ``GP.wip_sweep(criteria=('zvar',))``: the expected reduction of Var Z is
    ``exp(2 log_ez - zvar)``.  Picks from the candidate pool; ``acq_kwargs['zvar_polish'] = R`` (1 ... 16; default 0: the
    pool pick, as ever) refines the pick as ``_polished_point`` does for the weighted scores - L-BFGS-B on the unit cube from
    the R best pool rows in lock step, one ``GP.wip_grad_zvar`` call per round (M^2 work per point: a cost of another order
    than the weighted scores', hence a key of its own), at most ``acq_kwargs['zvar_polish_maxiter']`` (100) iterations; a
    restart that meets a +inf score ends non-finite and is skipped.  ``acq_kwargs['weighted_polish']`` > 0 stays a
    ValueError: it names the weighted scores' polish."""
    name: str = "ZVar"
    _key = "zvar"
    _grad_entry = "bobe_gp_wip_grad_zvar"

    def _score_and_grad(self, gp, x, mc_points, log_weights):
        r = gp.wip_grad_zvar(x, mc_points, log_weights=log_weights)
        return r["zvar"], r["dzvar"]

    def get_next_point(self, gp, acq_kwargs=None, maxiter: int = 100, n_restarts: int = 1, verbose: bool = True,
                       early_stop_patience: int = 25, rng=None):
        kw = acq_kwargs if acq_kwargs is not None else {}
        if _weighted_polish(kw) > 0:
            raise ValueError("ZVar's polish is acq_kwargs['zvar_polish']: weighted_polish must be 0")
        polish = _zvar_polish(kw)
        if polish == 0:
            return super().get_next_point(gp, acq_kwargs=acq_kwargs, maxiter=maxiter, n_restarts=n_restarts, verbose=verbose,
                                          early_stop_patience=early_stop_patience, rng=rng)
        mc_points, log_weights = self._integration_points(kw, rng)
        vals, idx = self.sweep(gp, mc_points, mc_points, log_weights=log_weights)          # every score: the starts come from them
        return self._polished_point(gp, np.asarray(mc_points), log_weights, np.asarray(vals), int(idx), polish,
                                    int(kw.get("zvar_polish_maxiter", 100)))


class PathwiseTS(AcquisitionFunction):
    """Thompson sampling by pathwise posterior draws of the surrogate (``GP.sample_paths``; no counterpart in the reference):
    member s of a batch is the pool row that maximises path s - one draw of the surrogate per member, evaluated over the
    whole pool on the device (``PosteriorPaths.argmax``).  The pool is ``acq_kwargs['candidates']`` or, without that key, all
    of ``mc_samples['x']`` (the choice of ``batch_mode='sweep'``).  ``acq_kwargs['ts_mode']``: 'max' (default), classic
    Thompson sampling, or 'posterior': a Gumbel-max draw from the pool reweighted from exp(mean) to exp(f_s) - the bias
    handed to the argmax is Gumbel noise minus the surrogate mean.  ``acq_kwargs['ts_features']``: random Fourier features
    per path (2048).  The paths are seeded by one ``rng.integers`` draw.  Values: the paths at their picks.
    ``acq_kwargs['ts_polish'] = R`` (default 0: the pool picks above, bit for bit) carries the argmax to the continuum: member
    s starts from the R best pool rows of path s and takes the maximum of its path over the unit cube
    (``PosteriorPaths.maximize``, at most ``acq_kwargs['ts_polish_maxiter']`` = 100 L-BFGS-B iterations; ``_polished_batch``
    has the replacement rule); it needs ``ts_mode='max'`` and draws the same numbers from ``rng``.
    ``acq_kwargs['ts_chain_steps'] = n`` (default 0 or absent: the pool picks above, bit for bit, and the same numbers from
    ``rng``) turns the Gumbel-max pick into a Thompson sample from exp(f_s) in the continuum: member s starts at its pool
    pick and runs ``acq_kwargs['ts_chain_warmup']`` (default 50) adapting HMC iterations, then n more, on path s
    (``PosteriorPaths.hmc_run``: all members in one launch per phase; inverse masses from the pool's spread in logit
    coordinates; one more ``rng.integers`` draw seeds the chains) and returns the chain's end state.  It needs
    ``ts_mode='posterior'``.  An end point that is infeasible under the GP's gate or within 1e-12 of an earlier member's falls
    back to the member's pool pick."""

    name: str = "PathwiseTS"

    def get_next_point(self, gp, acq_kwargs=None, maxiter: int = 100, n_restarts: int = 1, verbose: bool = True,
                       early_stop_patience: int = 25, rng=None):
        pts, vals = self.get_next_batch(gp, n_batch=1, acq_kwargs=acq_kwargs, rng=rng)
        return pts[0], float(vals[0])

    def get_next_batch(self, gp: GP, n_batch: int = 1, acq_kwargs=None, maxiter: int = 500, n_restarts: int = 8,
                       verbose: bool = True, early_stop_patience: int = 25, rng=None):
        rng = rng if rng is not None else get_numpy_rng()
        acq_kwargs = acq_kwargs if acq_kwargs is not None else {}
        mode = acq_kwargs.get("ts_mode", "max")
        if mode not in ("max", "posterior"):
            raise ValueError(f"ts_mode must be 'max' or 'posterior', not {mode!r}")
        polish = _ts_polish(acq_kwargs, mode)
        chain_steps, chain_warmup = _ts_chain_steps(acq_kwargs, mode)
        pool = acq_kwargs.get("candidates")
        if pool is None:
            pool = acq_kwargs["mc_samples"]["x"]
        on_device = hasattr(pool, "data_ptr")
        pool_host = pool.detach().cpu().numpy() if on_device else _lib.as_f64(np.atleast_2d(pool))
        if not on_device:
            pool = pool_host
        n_pool, n_batch = int(pool_host.shape[0]), int(n_batch)
        if n_pool < n_batch:
            raise ValueError(f"a batch of {n_batch} needs a pool of at least that many rows, not {n_pool}")
        seed = int(rng.integers(0, 2 ** 63))
        bias = None
        if mode == "posterior":          # argmax_c y_std (f_s - m)(c) + G_sc, in the standardised units of the paths
            mean, _ = gp._predict(pool_host, True, False, 0)
            bias = rng.gumbel(size=(n_batch, n_pool)) / gp.y_std - mean[None, :]
        with gp.sample_paths(n_batch, int(acq_kwargs.get("ts_features", 2048)), seed=seed) as paths:
            if polish > 0:
                return self._polished_batch(gp, paths, pool, pool_host, n_batch, polish,
                                            int(acq_kwargs.get("ts_polish_maxiter", 100)))
            picks, vals = paths.argmax(pool, bias)
            taken = set()
            for s in range(n_batch):
                if int(picks[s]) in taken:           # the path's best row among those no earlier member took
                    row = (paths.evaluate(pool)[s] - paths.y_mean) / paths.y_std
                    if bias is not None:
                        row = row + bias[s]
                    row[list(taken)] = -np.inf
                    picks[s] = int(np.argmax(row))
                    vals[s] = paths.y_mean + paths.y_std * row[picks[s]]
                taken.add(int(picks[s]))
            if chain_steps > 0:
                return self._chain_batch(gp, paths, pool_host, picks, vals, chain_steps, chain_warmup,
                                         int(rng.integers(0, 2 ** 62)))
        return np.array(pool_host[picks]), np.array(vals)

    @staticmethod
    def _chain_batch(gp, paths, pool_host, picks, vals, n_steps, n_warmup, seed):
        """``ts_chain_steps`` = n > 0: member s runs one HMC chain on path s from its pool pick - ``n_warmup`` adapting
        iterations, then n with the averaged step size - and takes the end state (value: the path there).  The inverse mass
        of every chain is the variance of the pool in logit coordinates + 1e-3.  An end point that the GP's gate refuses, or
        that lies within 1e-12 (max-norm) of an earlier member's point, is replaced by the member's pool pick."""
        n_batch, d = len(picks), pool_host.shape[1]
        logit = lambda x: np.log(x) - np.log1p(-x)
        inv_mass = np.var(logit(np.clip(pool_host, 1e-6, 1.0 - 1e-6)), axis=0) + 1e-3
        idx = np.arange(n_batch, dtype=np.int64)
        state = paths.hmc_state(logit(np.clip(pool_host[picks], 1e-6, 1.0 - 1e-6)), idx, 1.0)
        adapt = np.tile(np.array([0.1, 0.0, 0.0, 0.0, 0.0]), (n_batch, 1))
        if n_warmup > 0:
            paths.hmc_run(state, adapt, inv_mass, idx, seed, 0, n_warmup, True)
            adapt[:, 0] = np.where(adapt[:, 3] != 0.0, np.clip(np.exp(adapt[:, 3]), 1e-4, 2.0), adapt[:, 0])
        paths.hmc_run(state, adapt, inv_mass, idx, seed, n_warmup, n_steps, False)
        x_end, v_end = state[:, 2 * d:3 * d], state[:, 3 * d + 1]
        gated = bool(getattr(gp, "_gated", lambda: False)())
        ok = np.ones(n_batch, dtype=bool)
        if gated:
            from .clf import gate_eval
            ok = gate_eval(gp._lib, gp._h, np.ascontiguousarray(x_end), gp.ndim)[1] > 0.0
        pts, out_vals = [], []
        for s in range(n_batch):
            x, v = x_end[s], v_end[s]
            if not (ok[s] and np.isfinite(v) and all(np.max(np.abs(x - q)) > _TS_DUPLICATE_TOL for q in pts)):
                x, v = pool_host[picks[s]], vals[s]
            pts.append(np.array(x))
            out_vals.append(float(v))
        return np.array(pts), np.array(out_vals)

    @staticmethod
    def _polished_batch(gp, paths, pool, pool_host, n_batch, n_starts, maxiter):
        """``ts_polish`` = R > 0: member s starts from the R best pool rows of path s (ties: the lower index) and takes the
        maximum of its path over the unit cube (``PosteriorPaths.maximize``).  A polished point within 1e-12 (max-norm) of an
        earlier member's pick, or infeasible under the GP's gate, is replaced by the path's next-best admissible restart
        result, then by its pool pick: the best pool row no earlier member took (feasible, where the gate leaves one)."""
        fpool = paths.evaluate(pool)                                             # (S, C), physical units
        order = np.argsort(-fpool, axis=1, kind="stable")                        # descending, ties by the lower index
        r = min(int(n_starts), pool_host.shape[0])
        res = paths.maximize(pool_host[order[:, :r]], bounds=(0.0, 1.0), maxiter=maxiter)
        gated = bool(getattr(gp, "_gated", lambda: False)())

        def feasible(x):
            if not gated:
                return np.ones(len(x), dtype=bool)
            from .clf import gate_eval
            return gate_eval(gp._lib, gp._h, x, gp.ndim)[1] > 0.0

        pts, vals, taken = [], [], set()

        def admissible(x):
            return all(np.max(np.abs(x - q)) > _TS_DUPLICATE_TOL for q in pts) and bool(feasible(x[None, :])[0])

        for s in range(n_batch):
            ranked = [k for k in np.argsort(-res["restart_value"][s], kind="stable") if np.isfinite(res["restart_value"][s, k])]
            cands = [(res["x"][s], res["value"][s])] + [(res["restart_x"][s, k], res["restart_value"][s, k]) for k in ranked]
            pick = next(((x, v) for x, v in cands if admissible(x)), None)
            if pick is None:
                free = [int(c) for c in order[s] if int(c) not in taken]
                ok = feasible(pool_host[free])
                row = next((c for c, f in zip(free, ok) if f), free[0])
                taken.add(row)
                pick = (pool_host[row], fpool[s, row])
            else:
                hit = np.flatnonzero(np.all(pool_host == pick[0], axis=1))        # (a start that won is a pool row)
                taken.update(int(c) for c in hit)
            pts.append(np.array(pick[0]))
            vals.append(float(pick[1]))
        return np.array(pts), np.array(vals)


_TS_DUPLICATE_TOL = 1e-12       # max-norm distance below which a polished Thompson pick counts as an earlier member's


def _ts_polish(acq_kwargs, mode) -> int:
    """``acq_kwargs['ts_polish']``: restarts of the L-BFGS-B polish per path, 0 (default) = none"""
    r = acq_kwargs.get("ts_polish", 0)
    if isinstance(r, bool) or int(r) != r or int(r) < 0:
        raise ValueError(f"ts_polish must be a non-negative integer, not {r!r}")
    if int(r) > 0 and mode == "posterior":
        raise ValueError("ts_polish needs ts_mode='max': a Gumbel-max draw from a pool has no continuum form")
    return int(r)


WIP_GRAD_W_MAX_N = 4096         # bobe_gp_wip_grad_w's / bobe_gp_wip_grad_zvar's limit on the training points (its matrix-vector chain has no tile path)


def _weighted_polish(acq_kwargs) -> int:
    """``acq_kwargs['weighted_polish']``: starts of the L-BFGS-B polish of a weighted pick, an integer 0 (default: none) ... 16"""
    r = acq_kwargs.get("weighted_polish", 0)
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) <= 16:
        raise ValueError(f"weighted_polish must be an integer between 0 and 16, not {r!r}")
    return int(r)


def _zvar_polish(acq_kwargs) -> int:
    """``acq_kwargs['zvar_polish']``: starts of the L-BFGS-B polish of a ZVar pick, an integer 0 (default: none) ... 16"""
    r = acq_kwargs.get("zvar_polish", 0)
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) <= 16:
        raise ValueError(f"zvar_polish must be an integer between 0 and 16, not {r!r}")
    return int(r)


def _ts_chain_steps(acq_kwargs, mode):
    """``acq_kwargs['ts_chain_steps']`` / ``['ts_chain_warmup']``: HMC iterations of a Thompson member on its path, 0 (default)
    = none.  Checked before anything touches the device."""
    n, w = acq_kwargs.get("ts_chain_steps", 0), acq_kwargs.get("ts_chain_warmup", 50)
    for name, v in (("ts_chain_steps", n), ("ts_chain_warmup", w)):
        if isinstance(v, bool) or int(v) != v or int(v) < 0:
            raise ValueError(f"{name} must be a non-negative integer, not {v!r}")
    if int(n) > 0 and mode != "posterior":
        raise ValueError("ts_chain_steps needs ts_mode='posterior': the chain continues a draw from exp(f_s), not an argmax")
    return int(n), int(w)


def get_mc_samples(gp: GP, warmup_steps=512, num_samples=1024, thinning=4, method="NUTS", num_chains=4,
                   np_rng=None, rng_key=None, *, sampler="hmc", weighted=False):
    """BOBE/acquisition.py:468-482: 'NUTS' (Hamiltonian Monte Carlo on the surrogate, batched on the GPU), 'NS'
    (nested sampling on the surrogate) or 'uniform' (scrambled Sobol).  ``sampler`` picks the chains of 'NUTS':
    'hmc' (the default) or 'nuts' (No-U-Turn transitions on the device, ``sample_GP_NUTS``).  ``weighted`` ('NS' only): keep
    the nested samples with their weights instead of resampling them to equal weights (``get_mc_points(weighted=True)``)."""
    if method == "uniform":
        return {"x": qmc.Sobol(gp.ndim, scramble=True, seed=np_rng).random(num_samples)}
    if method == "NS":                                   # acquisition.py:473-475, batched on the GPU GP
        from .samplers import nested_sampling
        rng = np_rng if isinstance(np_rng, np.random.Generator) else np.random.default_rng(np_rng)
        if weighted:
            samples, _, _ = nested_sampling(gp, ndim=gp.ndim, mode="acq", rng=rng, keep_weights=True)
        else:
            samples, _, _ = nested_sampling(gp, ndim=gp.ndim, mode="acq", rng=rng)
        return samples
    if method == "NUTS":                                 # acquisition.py:470-472, batched HMC on the GPU GP
        from .samplers import sample_GP_NUTS
        rng = np_rng if isinstance(np_rng, np.random.Generator) else np.random.default_rng(np_rng)
        return sample_GP_NUTS(gp, np_rng=rng, rng_key=rng_key, num_chains=num_chains, warmup_steps=warmup_steps,
                              num_samples=num_samples, thinning=thinning, sampler=sampler)
    raise ValueError(f"Unknown method {method} for sampling GP")          # acquisition.py:481


def get_mc_points(mc_samples, mc_points_size=128, rng=None, *, weighted=False):
    """BOBE/acquisition.py:485-489.  ``weighted=True``: the ``mc_points_size`` heaviest samples by ``mc_samples['weights']``
    (ties by index; nothing is drawn from the generator) and their log-weights under the flat prior measure, ``log(weights) -
    logl`` - returns ``(points, log_weights)``, what ``GP.wip_sweep(log_weights=)`` takes."""
    if weighted:
        if mc_samples.get("weights") is None or mc_samples.get("logl") is None:
            raise ValueError("weighted integration points need mc_samples['weights'] and mc_samples['logl']")
        w = np.asarray(mc_samples["weights"], dtype=np.float64).reshape(-1)
        idxs = np.argsort(-w, kind="stable")[:mc_points_size]
        idxs = idxs[w[idxs] > 0.0]
        with np.errstate(divide="ignore"):
            lw = np.log(w[idxs]) - np.asarray(mc_samples["logl"], dtype=np.float64).reshape(-1)[idxs]
        return np.asarray(mc_samples["x"])[idxs], lw
    mc_size = max(mc_samples["x"].shape[0], mc_points_size)
    rng = rng if rng is not None else get_numpy_rng()
    idxs = rng.choice(mc_size, size=mc_points_size, replace=False)
    return mc_samples["x"][idxs]
