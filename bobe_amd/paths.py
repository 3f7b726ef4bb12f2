"""``PosteriorPaths`` - a set of pathwise posterior draws of a ``GP``'s latent surrogate (``bobe_gp_paths_*``,
include/bobe_gp.h): functions that can be evaluated at any points, maximised over a pool or added to a sampler's log
likelihoods, differentiated with respect to the input and maximised over the cube.  Created by ``GP.sample_paths``."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib


def maximize_paths(batch_value_and_grad, starts, bounds=(0.0, 1.0), maxiter=100, options=None) -> dict:
    """SciPy's L-BFGS-B on -f_s from every start, all S * R runs in lock step (the drivers of optim.py: the stepped one where it
    is available, one ``minimize`` per thread otherwise).  ``starts``: (S, R, d), run (s, r) maximises path s.
    ``batch_value_and_grad(x (T, d), path_index (T,)) -> (f (T,), df (T, d))`` serves one round: the points of the runs still
    waiting, in run order - ONE call per round.  ``options``: L-BFGS-B options (SciPy's defaults; ``maxiter`` is set from the
    argument).

    Selection, per path: the largest value among the results of the restarts that finished and the (clipped) starts
    themselves, the values of the starts being those of the first round; ties go to the lower restart, then to the lower
    start; a restart that raised or ended on a non-finite value is skipped - so a path's result is never below its best
    start.  Returns ``x`` (S, d), ``value`` (S,), ``start_value`` (S,), ``restart`` (S,) (-1: a start won), ``n_rounds``,
    ``n_evaluations``, and the material of the selection: ``restart_x`` (S, R, d) / ``restart_value`` (S, R) (-inf: skipped)
    and ``start_x`` (S, R, d) / ``start_values`` (S, R) (-inf: the start's evaluation raised or was not finite)."""
    from .optim import _minimize_concurrently, _setup_bounds
    starts = np.array(starts, dtype=np.float64)
    if starts.ndim != 3:
        raise ValueError(f"starts must have shape (S, R, d), not {starts.shape}")
    S, R, d = starts.shape
    b = _setup_bounds(bounds, d)
    scipy_bounds = None if b is None else [(float(b[0, i]), float(b[1, i])) for i in range(d)]
    opts = dict(options or {})
    opts["maxiter"] = int(maxiter)
    count = {"rounds": 0, "evals": 0}
    start_x = np.array(starts.reshape(S * R, d) if b is None else np.clip(starts.reshape(S * R, d), b[0], b[1]))
    start_values = np.full(S * R, -np.inf)
    seen = np.zeros(S * R, dtype=bool)

    def batch(ids, xs):
        ids = np.asarray(ids, dtype=np.int64)
        count["rounds"] += 1
        count["evals"] += len(ids)
        f, g = batch_value_and_grad(np.array(xs, dtype=np.float64).reshape(len(ids), d), ids // R)
        f, g = np.asarray(f, dtype=np.float64).reshape(-1), np.asarray(g, dtype=np.float64).reshape(len(ids), d)
        for i, fi in zip(ids, f):                  # a run's first evaluation is at its start
            if not seen[i]:
                seen[i] = True
                if np.isfinite(fi):
                    start_values[i] = fi
        return [(-float(fi), -gi) for fi, gi in zip(f, g)]

    results = _minimize_concurrently(batch, start_x, True, with_ids=True, method="L-BFGS-B", bounds=scipy_bounds,
                                     options=opts)
    restart_x = np.array(start_x).reshape(S, R, d)
    restart_value = np.full((S, R), -np.inf)
    for i, res in enumerate(results):
        if isinstance(res, Exception) or res is None or not np.isfinite(res.fun):
            continue
        restart_x[i // R, i % R] = res.x
        restart_value[i // R, i % R] = -float(res.fun)
    start_x, start_values = start_x.reshape(S, R, d), start_values.reshape(S, R)
    x, value, which = np.empty((S, d)), np.empty(S), np.empty(S, dtype=np.int64)
    for s in range(S):
        # (np.argmax keeps the first of equal values: restarts in order, then the starts in order)
        both = np.concatenate([restart_value[s], start_values[s]])
        k = int(np.argmax(both))
        value[s] = both[k]
        which[s] = k if k < R else -1
        x[s] = restart_x[s, k] if k < R else start_x[s, k - R]
    return {"x": x, "value": value, "start_value": start_values.max(axis=1), "restart": which,
            "n_rounds": count["rounds"], "n_evaluations": count["evals"], "restart_x": restart_x,
            "restart_value": restart_value, "start_x": start_x, "start_values": start_values}


def _destroy(lib, handle: C.c_void_p) -> None:
    if handle.value:
        lib.bobe_gp_paths_destroy(handle)
        handle.value = None


class PosteriorPaths:
    """S draws f_s of the posterior of the latent surrogate, f_s(x) = phi(x)^T w_s + k(x, X) K^-1 (y - Phi(X) w_s - eps_s) with F
    random Fourier features.  A snapshot of the GP at the time of ``GP.sample_paths``: later ``update`` / ``fit`` calls on the
    GP do not change it.  Holds device memory until ``close()`` (or the end of a ``with`` block, or collection); it is
    destroyed before its GP's handle.  ``evaluate`` / ``argmax`` / ``value_and_grad`` / ``maximize`` are not gated; ``hmc_run`` /
    ``sample`` apply the GP's classifier gate as it is set when they are called (the gate is not part of the snapshot)."""

    def __init__(self, gp, n_paths, n_features, seed, u=None, phase=None, w=None, eps=None):
        self._gp = gp
        self._lib = gp._lib
        s, f = int(n_paths), int(n_features)
        n, d = int(self._lib.bobe_gp_npoints(gp._h)), gp.ndim      # (the handle's own count: the plain GP subset of a GPwithClassifier)
        arrs = []
        for a, shape in ((u, (f, d)), (phase, (f,)), (w, (s, f)), (eps, (s, n))):
            if a is not None and not hasattr(a, "data_ptr"):
                a = _lib.as_f64(a, shape)
            arrs.append(a)
        self._h = C.c_void_p(0)
        st = _lib.check(self._lib.bobe_gp_paths_create(gp._h, s, f, int(seed) & (2 ** 64 - 1), _lib.ptr(arrs[0]),
                                                       _lib.ptr(arrs[1]), _lib.ptr(arrs[2]), _lib.ptr(arrs[3]),
                                                       C.byref(self._h)), "bobe_gp_paths_create")
        if st == _lib.BOBE_NOT_PD or not self._h.value:
            raise _lib.BobeLibraryError("bobe_gp_paths_create: " + _lib.last_error())
        self.n_paths, self.n_features = s, f
        self._n, self._d = n, d
        # physical units of the snapshot (the GP standardises again at every update)
        self.y_mean, self.y_std = float(gp.y_mean), float(gp.y_std)
        self._finalizer = weakref.finalize(self, _destroy, self._lib, self._h)
        gp._paths.add(self)

    @property
    def ndim(self) -> int:
        return self._d

    @property
    def gp(self):
        """The GP the set was drawn from (its training data give the samplers their starts, its gate applies to them)."""
        return self._gp

    def _handle(self):
        if not self._h.value:
            raise ValueError("the path set is closed")
        return self._h

    def close(self) -> None:
        """Return the set's device memory (idempotent)."""
        self._finalizer()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def arrays(self) -> dict:
        """The set's random arrays: ``u`` (F, d) unit-length-scale frequencies, ``phase`` (F,), ``w`` (S, F), ``eps`` (S, N)."""
        s, f = self.n_paths, self.n_features
        out = {"u": np.empty((f, self._d)), "phase": np.empty(f), "w": np.empty((s, f)), "eps": np.empty((s, self._n))}
        _lib.check(self._lib.bobe_gp_paths_get(self._handle(), _lib.ptr(out["u"]), _lib.ptr(out["phase"]), _lib.ptr(out["w"]),
                                               _lib.ptr(out["eps"])), "bobe_gp_paths_get")
        return out

    @staticmethod
    def _points(x):
        return x if hasattr(x, "data_ptr") else _lib.as_f64(np.atleast_2d(x))

    def evaluate(self, x, centered=False) -> np.ndarray:
        """The paths at the C rows of ``x`` (NumPy array or torch CUDA tensor): an (S, C) array in physical units,
        y_mean + y_std f_s(x); ``centered=True``: y_std (f_s(x) - m(x)) with m the posterior mean."""
        x = self._points(x)
        c = int(x.shape[0])
        out = np.empty((self.n_paths, c))
        _lib.check(self._lib.bobe_gp_paths_eval(self._handle(), _lib.ptr(x), c, 1 if centered else 0, _lib.ptr(out)),
                   "bobe_gp_paths_eval")
        return self.y_std * out if centered else self.y_mean + self.y_std * out

    def _grad_std(self, x, path_index, centered=False):
        """``bobe_gp_paths_grad``: (f (T,), df (T, d)) in the set's standardised units"""
        x = self._points(x)
        t = int(x.shape[0])
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(path_index, dtype=np.int64).reshape(-1), (t,)))
        f, df = np.empty(t), np.empty((t, self._d))
        _lib.check(self._lib.bobe_gp_paths_grad(self._handle(), _lib.ptr(x), t, _lib.ptr(idx), 1 if centered else 0, _lib.ptr(f),
                                                _lib.ptr(df)), "bobe_gp_paths_grad")
        return f, df

    def value_and_grad(self, x, path_index, centered=False):
        """(values (T,), grads (T, d)): path ``path_index[t]`` and its gradient with respect to the input at row t of ``x``
        (NumPy array or torch CUDA tensor; one index serves every row), in physical units: y_mean + y_std f_s(x) and
        y_std grad f_s(x); ``centered=True``: the path minus the posterior mean, without y_mean.  Analytic, on the device
        (``bobe_gp_paths_grad``); the bits at a point do not depend on the other points of the call."""
        f, df = self._grad_std(x, path_index, centered)
        return (self.y_std * f if centered else self.y_mean + self.y_std * f), self.y_std * df

    def maximize(self, starts, bounds=(0.0, 1.0), maxiter=100, options=None) -> dict:
        """The maximum of every path by L-BFGS-B from R starts each (``starts``: (S, R, d); ``maximize_paths`` has the
        driver, the selection rule and the keys of the result).  Every round of the S * R runs is one ``bobe_gp_paths_grad``
        call on the points still waiting, in standardised units; ``value`` / ``start_value`` / ``restart_value`` /
        ``start_values`` come back in physical units, y_mean + y_std f.  A path's result is never below its best start."""
        starts = np.asarray(starts, dtype=np.float64)
        if starts.ndim != 3 or starts.shape[0] != self.n_paths or starts.shape[2] != self._d:
            raise ValueError(f"starts must have shape ({self.n_paths}, R, {self._d}), not {starts.shape}")
        self._handle()
        out = maximize_paths(self._grad_std, starts, bounds=bounds, maxiter=maxiter, options=options)
        for k in ("value", "start_value", "restart_value", "start_values"):
            out[k] = self.y_mean + self.y_std * out[k]
        return out

    def chain_layout(self) -> dict:
        """Where a chain workgroup of ``hmc_run`` keeps this set's training rows (``bobe_debug_paths_chain_layout``):
        ``registers`` / ``lds`` / ``streamed`` row counts and ``features_per_thread``."""
        info = (C.c_int * 4)()
        _lib.check(self._lib.bobe_debug_paths_chain_layout(self._handle(), info), "bobe_debug_paths_chain_layout")
        return {"registers": int(info[0]), "lds": int(info[1]), "streamed": int(info[2]), "features_per_thread": int(info[3])}

    def hmc_run(self, state, adapt, inv_mass, path_index, seed: int, it0: int, niter: int, do_adapt: bool, temp: float = 1.0,
                hist_from=None, thin: int = 0, debug: bool = False):
        """``GP.hmc_run`` on paths: ``niter`` whole HMC trajectories of every chain in ONE launch (``bobe_gp_paths_hmc_run``),
        chain c on the posterior implied by the draw ``path_index[c]`` (one index serves every chain), in the snapshot's units
        (its ``y_std`` / ``y_mean``).  ``state`` (P, 3d+2) = [u, dlogp/du, x, logp, mean] and ``adapt`` (P, 5) are updated in
        place; ``inv_mass`` is per chain, (P, d) (a (d,) vector serves every chain).  Returns (hist, keep, dbg) as
        ``GP.hmc_run`` does.  The parent GP's classifier gate, as set at call time, applies: it is not part of the snapshot."""
        P, d = state.shape[0], self._d
        if state.shape != (P, 3 * d + 2) or adapt.shape != (P, 5) or not (state.flags.c_contiguous and adapt.flags.c_contiguous) \
                or state.dtype != np.float64 or adapt.dtype != np.float64:
            raise ValueError("state must be a C-contiguous float64 (P, 3d+2) array and adapt a (P, 5) one")
        im = np.ascontiguousarray(np.broadcast_to(_lib.as_f64(inv_mass), (P, d)))
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(path_index, dtype=np.int64).reshape(-1), (P,)))
        niter = int(niter)
        if hist_from is not None and not 0 <= int(hist_from) <= niter:
            raise ValueError("hist_from must be in [0, niter]")
        if thin < 0 or niter < 1:
            raise ValueError("niter must be positive and thin non-negative")
        hist = np.empty((niter - int(hist_from), P, d)) if hist_from is not None else None
        keep = np.empty((niter // thin, P, d + 1)) if thin else None
        dbg = np.empty((P, d + 3)) if debug else None
        _lib.check(self._lib.bobe_gp_paths_hmc_run(self._handle(), P, _lib.ptr(idx), _lib.ptr(state), _lib.ptr(adapt),
                                                   _lib.ptr(im), int(seed) & (2 ** 64 - 1), int(it0), niter,
                                                   int(bool(do_adapt)), float(self.y_std), float(self.y_mean), float(temp),
                                                   int(hist_from or 0), _lib.ptr(hist) if hist is not None else None,
                                                   int(thin) if thin else 1, _lib.ptr(keep) if keep is not None else None,
                                                   _lib.ptr(dbg) if dbg is not None else None), "bobe_gp_paths_hmc_run")
        return hist, keep, dbg

    def hmc_state(self, U, path_index, temp: float = 1.0) -> np.ndarray:
        """The (P, 3d+2) chain state [u, dlogp/du, x, logp, mean] of ``hmc_run`` at the logit positions ``U`` (P, d), chain c
        on path ``path_index[c]``: values and gradients from ``value_and_grad``; a point the parent GP's gate refuses gets
        mean = minus_inf and no gradient, as in the kernel."""
        U = _lib.as_f64(U)
        X = np.clip(1.0 / (1.0 + np.exp(-U)), 1e-12, 1.0 - 1e-12)
        mean, gx = self.value_and_grad(X, path_index)
        gp = self._gp
        if hasattr(gp, "_gated") and gp._gated():
            bad = ~(np.asarray(gp._device_proba(X)).reshape(-1) >= gp.probability_threshold)
            mean = np.where(bad, gp.minus_inf, mean)
            gx = np.where(bad[:, None], 0.0, gx)
        lp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
        g = gx / temp * (X * (1.0 - X)) + (1.0 - 2.0 * X)
        return np.ascontiguousarray(np.concatenate([U, g, X, lp[:, None], mean[:, None]], axis=1))

    def sample(self, **kwargs) -> dict:
        """``samplers.sample_paths_hmc(self, **kwargs)``: HMC samples of the posterior implied by every path of the set."""
        from .samplers import sample_paths_hmc
        return sample_paths_hmc(self, **kwargs)

    def argmax(self, x, bias=None):
        """(indices (S,), values (S,)): for every path the row of ``x`` that maximises f_s(x) + bias[s] (``bias``: (S, C), in the
        standardised units of f_s, or None) and that maximum, found on the device without forming the (S, C) matrix.  The
        values are y_mean + y_std (f_s + bias).  Ties go to the lower index."""
        x = self._points(x)
        c = int(x.shape[0])
        b = bias
        if b is not None and not hasattr(b, "data_ptr"):
            b = _lib.as_f64(b, (self.n_paths, c))
        idx = np.empty(self.n_paths, dtype=np.int64)
        best = np.empty(self.n_paths)
        _lib.check(self._lib.bobe_gp_paths_argmax(self._handle(), _lib.ptr(x), c, _lib.ptr(b), _lib.ptr(idx), _lib.ptr(best)),
                   "bobe_gp_paths_argmax")
        return idx, self.y_mean + self.y_std * best
