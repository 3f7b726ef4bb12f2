"""``PosteriorPaths`` - a set of pathwise posterior draws of a ``GP``'s latent surrogate (``bobe_gp_paths_*``,
include/bobe_gp.h): functions that can be evaluated at any points, maximised over a pool or added to a sampler's log
likelihoods.  Created by ``GP.sample_paths``."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib


def _destroy(lib, handle: C.c_void_p) -> None:
    if handle.value:
        lib.bobe_gp_paths_destroy(handle)
        handle.value = None


class PosteriorPaths:
    """S draws f_s of the posterior of the latent surrogate, f_s(x) = phi(x)^T w_s + k(x, X) K^-1 (y - Phi(X) w_s - eps_s) with F
    random Fourier features.  A snapshot of the GP at the time of ``GP.sample_paths``: later ``update`` / ``fit`` calls on the
    GP do not change it.  Holds device memory until ``close()`` (or the end of a ``with`` block, or collection); it is
    destroyed before its GP's handle.  Not gated."""

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
