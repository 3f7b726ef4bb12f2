"""``GP`` — MI355X-resident counterpart of ``BOBE.gp.GP`` (BOBE/gp.py:199-772).

Same constructor keywords, attributes and methods as the reference class; all O(N^2)/O(N^3)
arithmetic (kernel assembly, Cholesky, solves, MLL + gradient, batched prediction, fantasy
variance) runs on the GPU through libbobe_gp.so (include/bobe_gp.h).  Host side keeps only what
the reference also keeps on the host: y standardisation, priors, bounds, the L-BFGS-B loop.

There is no CPU fallback: constructing a GP without the library or without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
import weakref
from typing import List, Optional

import numpy as np

from . import _lib
from . import priors as P
from .optim import optimize_optax, optimize_scipy
from .utils import get_logger, get_numpy_rng

log = get_logger("gp")

safe_noise_floor = 1e-12  # BOBE/gp.py:16

KERNEL_IDS = {"rbf": 0, "matern": 1}


def _tofloat(x) -> float:
    return float(np.asarray(x).reshape(-1)[0]) if np.ndim(x) else float(x)


# ---- module-level helpers of the reference's gp.py, same names and arguments --------------------------------
DummyDistribution = P.Dummy                      # gp.py:22-25
make_distribution = P.make_distribution          # gp.py:27-55 (numpyro's names and keywords, priors.py)


def saas_prior_logprob(lengthscales, kernel_variance, tausq):
    """gp.py:57-78: the SAAS prior's log-density (O(d) host arithmetic, priors.py)."""
    return P.saas_logprob_and_grad(np.asarray(lengthscales, dtype=np.float64), float(kernel_variance), float(tausq))[0]


_KERNEL_HANDLES: dict = {}


_FREE_LOCK = threading.RLock()     # the module-level functions share handles: one caller at a time


def _free_handle(kernel_id: int, d: int, device: int = 0):
    """The cached data-less handle per (kernel, d, device) behind the module-level kernel / distance functions (they hold
    O(n1 n2) scratch only).  Callers hold ``_FREE_LOCK`` for the duration of the library call."""
    lib = _lib.load()
    key = (kernel_id, d, device)
    if key not in _KERNEL_HANDLES:
        h = C.c_void_p(0)
        _lib.check(lib.bobe_gp_create(C.byref(h), device, kernel_id, d), "bobe_gp_create")
        _KERNEL_HANDLES[key] = h
    return lib, _KERNEL_HANDLES[key]


class _scratch_handle:
    """A data-less handle for ONE call of a matrix-input function (``gp_mll``, ``fast_update_cholesky``): the library sizes a
    factorisation workspace of several n^2 doubles for it, which goes back to the device when the call is over."""

    def __init__(self, device: int = 0):
        self.device = device

    def __enter__(self):
        self.lib = _lib.load()
        self.h = C.c_void_p(0)
        _lib.check(self.lib.bobe_gp_create(C.byref(self.h), self.device, KERNEL_IDS["rbf"], 1), "bobe_gp_create")
        return self.lib, self.h

    def __exit__(self, *exc):
        self.lib.bobe_gp_destroy(self.h)
        return False


def std_from_log_t0(log_t0: float) -> float:
    """sqrt(log1p(exp(log_t0))): the standard deviation of log Z of the lognormal whose squared coefficient of variation is
    exp(log_t0).  Formed from the log where the exponential would overflow: log1p(e^t) = t + log1p(e^-t)."""
    t = float(log_t0)
    if t != t:
        return t
    return math.sqrt(t + math.log1p(math.exp(-t))) if t > 30.0 else math.sqrt(math.log1p(math.exp(t)))


def dist_sq(x, y):
    """gp.py:80-96: squared Euclidean distances (n1, n2) of the rows of ``x`` and ``y``, on the GPU (bobe_gp_dist_sq)."""
    x = _lib.as_f64(np.atleast_2d(x))
    y = _lib.as_f64(np.atleast_2d(y))
    if x.shape[1] != y.shape[1]:
        raise ValueError("x and y must have the same number of columns")
    out = np.empty((x.shape[0], y.shape[0]))
    with _FREE_LOCK:
        lib, h = _free_handle(KERNEL_IDS["rbf"], x.shape[1])
        _lib.check(lib.bobe_gp_dist_sq(h, _lib.ptr(x), x.shape[0], _lib.ptr(y), y.shape[0], _lib.ptr(out)), "bobe_gp_dist_sq")
    return out


def gp_mll(k, train_y, num_points):
    """gp.py:170-178: the marginal log-likelihood of ``train_y`` under the kernel matrix ``k`` handed in (Cholesky, solves
    and reductions on the GPU, bobe_gp_mll_from_k); NaN when ``k`` is not positive definite, as XLA's Cholesky gives."""
    k = _lib.as_f64(k)
    y = _lib.as_f64(train_y).reshape(-1)
    n = int(num_points)
    if k.shape != (n, n) or y.shape[0] != n:
        raise ValueError(f"k must be ({n}, {n}) and train_y must hold {n} values")
    mll = C.c_double(0.0)
    with _scratch_handle() as (lib, h):
        _lib.check(lib.bobe_gp_mll_from_k(h, _lib.ptr(k), n, _lib.ptr(y), C.byref(mll)), "bobe_gp_mll_from_k")
    return float(mll.value)


def fast_update_cholesky(L, k, k_self):
    """gp.py:181-197: the (n+1) x (n+1) factor after appending one point - last row ``[L^-1 k, sqrt(k_self - |L^-1 k|^2)]``,
    the solve on the GPU (bobe_gp_chol_row_update)."""
    L = _lib.as_f64(L)
    n = L.shape[0]
    k = _lib.as_f64(k).reshape(-1)
    if L.shape != (n, n) or k.shape[0] != n:
        raise ValueError("L must be (n, n) and k must hold n values")
    v = np.empty(n)
    diag = C.c_double(0.0)
    with _scratch_handle() as (lib, h):
        _lib.check(lib.bobe_gp_chol_row_update(h, _lib.ptr(L), n, _lib.ptr(k), _tofloat(k_self), _lib.ptr(v), C.byref(diag)),
                   "bobe_gp_chol_row_update")
    new_L = np.zeros((n + 1, n + 1))
    new_L[:n, :n] = L
    new_L[n, :n] = v
    new_L[n, n] = diag.value
    return new_L


def _kernel_on_gpu(kernel_id: int, xa, xb, lengthscales, kernel_variance, noise, include_noise, device: int = 0):
    """K(xa, xb) through bobe_gp_kernel on a cached data-less handle per (kernel, d, device)."""
    xa = _lib.as_f64(np.atleast_2d(xa))
    xb = _lib.as_f64(np.atleast_2d(xb))
    d = xa.shape[1]
    ls = _lib.as_f64(lengthscales).reshape(-1)
    if ls.size == 1 and d > 1:
        ls = np.full(d, float(ls[0]))
    out = np.empty((xa.shape[0], xb.shape[0]))
    with _FREE_LOCK:
        lib, handle = _free_handle(kernel_id, d, device)
        _lib.check(lib.bobe_gp_kernel(handle, _lib.ptr(xa), xa.shape[0], _lib.ptr(xb), xb.shape[0],
                                      _lib.ptr(ls), float(kernel_variance), float(noise), 1 if include_noise else 0,
                                      _lib.ptr(out)), "bobe_gp_kernel")
    return out


def rbf_kernel(xa, xb, lengthscales, kernel_variance, noise, include_noise=True):
    """BOBE/gp.py:124-154, evaluated on the GPU."""
    return _kernel_on_gpu(KERNEL_IDS["rbf"], xa, xb, lengthscales, kernel_variance, noise, include_noise)


def matern_kernel(xa, xb, lengthscales, kernel_variance, noise, include_noise=True):
    """BOBE/gp.py:156-168 (Matérn-5/2), evaluated on the GPU."""
    return _kernel_on_gpu(KERNEL_IDS["matern"], xa, xb, lengthscales, kernel_variance, noise, include_noise)


def kernel_diag(x, kernel_variance, noise, include_noise=True):
    """BOBE/gp.py:98-122: the constant diagonal of a stationary kernel (O(n) host vector)."""
    diag = float(kernel_variance) * np.ones(np.atleast_2d(x).shape[0])
    return diag + float(noise) if include_noise else diag


class GP:
    def __init__(self, train_x, train_y, noise=1e-8, kernel="rbf", optimizer="scipy", optimizer_options={},
                 kernel_variance_bounds=[1e-4, 1e8], lengthscale_bounds=[0.01, 5], lengthscales=None,
                 kernel_variance=None, kernel_variance_prior=None, lengthscale_prior=None, tausq=None,
                 tausq_bounds=[1e-4, 1e4], param_names: Optional[List[str]] = None, device: int = 0,
                 pivot_floor_ulp: Optional[float] = None, _factor: bool = True, fit_objective: str = "mll",
                 fit_noise: bool = False, noise_bounds=[1e-10, 1e-1], noise_prior=None):
        """Same keywords as BOBE/gp.py:201-203 plus ``device`` (HIP device index) and ``pivot_floor_ulp`` (None: the
        library's default, 0 = the reference's rule - a factorisation fails only on a pivot <= 0, gp.py:175, 549; 64 is
        what ``BOBE(...)`` passes, see the property).  ``_factor=False`` (internal) leaves the factorisation to the caller,
        which is about to install a known one (``from_state_dict``, ``copy``).  ``fit_objective``: what ``fit`` minimises,
        'mll' (the reference's -(MLL + log prior)) or 'loo' (see the ``fit_objective`` property).  ``fit_noise=True`` (a build
        addition; off, nothing changes) makes the noise level the last hyper-parameter of ``fit``: ``noise`` is then its
        start value, ``noise_bounds`` its box and ``noise_prior`` a ``make_distribution`` spec (None: Uniform over the
        bounds, a constant)."""
        self._lib = _lib.load()
        self._h = C.c_void_p(0)
        self._paths = weakref.WeakSet()        # live path sets (sample_paths): closed before the handle they work on
        self.device = int(device)
        self._setup_training_data(train_x, train_y)
        self.param_names = param_names if param_names is not None else ["x_" + str(i) for i in range(self.ndim)]

        self.kernel_name = kernel if kernel == "rbf" else "matern"              # gp.py:251
        self.lengthscales = (np.array(lengthscales, dtype=np.float64).reshape(-1) if lengthscales is not None
                             else np.ones(self.ndim))
        self.kernel_variance = float(kernel_variance) if kernel_variance is not None else 1.0
        self.noise = float(noise)

        _lib.check(self._lib.bobe_gp_create(C.byref(self._h), self.device, KERNEL_IDS[self.kernel_name], self.ndim),
                   "bobe_gp_create")

        self.optimizer_method = optimizer
        self.mll_optimize = optimize_scipy if optimizer == "scipy" else optimize_optax          # gp.py:264-267
        self.optimizer_options = optimizer_options
        self.concurrent_restarts = True        # fit(): the restarts run concurrently ...
        self.restart_slots = 4                 # ... this many evaluations in flight at once (more oversubscribes the queues)
        # ... advancing in lock step, one bobe_gp_mll_batch call per round, the L-BFGS-B routines stepped by one thread
        # ("lockstep"), or each in its own thread on an evaluation slot ("slots").  Same trajectories and result either
        # way; "auto" = lock step where SciPy's routine can be stepped (optim._rc_available), else slots: measured
        # 33.7 vs 53.5 ms at N = 100, 39.5 vs 45.7 at 600, 124 vs 141 at 2048, 457 vs 461 at 4096 for a 4-restart fit
        self.restart_mode = "auto"
        self.fit_objective = fit_objective

        self.lengthscale_bounds = lengthscale_bounds
        self.kernel_variance_bounds = kernel_variance_bounds
        self.tausq = float(tausq) if tausq is not None else 1.0
        self.tausq_bounds = tausq_bounds
        self.fit_noise = bool(fit_noise)
        self.noise_bounds = [float(b) for b in np.asarray(noise_bounds, dtype=np.float64).reshape(-1).tolist()]
        self.noise_prior_spec = noise_prior
        self.noise_prior_dist = (P.make_distribution(noise_prior) if noise_prior is not None
                                 else P.Uniform(self.noise_bounds[0], self.noise_bounds[1]))

        self._setup_kernel_variance_prior(kernel_variance_prior)
        self._setup_lengthscale_prior(lengthscale_prior)
        self._setup_optimization_parameters()

        self.append_updates = True             # update(): rank-b append (O(b N^2)) instead of a full refactorisation
        self._chol_cache = self._alpha_cache = None
        self._pushed_hyper = None              # hyper-parameters of the factor on the device (set by _push_hyper)
        self.not_pd = False
        self._rank_test_noted = False
        if pivot_floor_ulp is not None:
            self.pivot_floor_ulp = pivot_floor_ulp
        self._push_data()
        if _factor:
            self.recompute_cholesky()                                           # gp.py:257-260

    def __del__(self):
        try:
            for ps in list(getattr(self, "_paths", ())):
                ps.close()
            if getattr(self, "_h", None) is not None and self._h.value:
                self._lib.bobe_gp_destroy(self._h)
                self._h = C.c_void_p(0)
        except Exception:
            pass

    # ------------------------------------------------------------------ data
    def _setup_training_data(self, train_x, train_y):
        """BOBE/gp.py:283-307."""
        train_x = np.asarray(train_x, dtype=np.float64)
        train_y = np.asarray(train_y, dtype=np.float64)
        if train_x.shape[0] != train_y.shape[0]:
            raise ValueError("train_x and train_y must have the same number of points")
        if train_y.ndim != 2:
            train_y = train_y.reshape(-1, 1)
        if train_x.ndim != 2:
            raise ValueError("train_x must be 2D")
        self.ndim = train_x.shape[1]
        self.y_mean = float(np.mean(train_y)) if train_y.size > 0 else 0.0
        self.y_std = float(np.std(train_y)) if train_y.size > 0 else 1.0
        if self.y_std == 0:
            log.warning("Training targets have zero variance. Setting std to 1.0 to avoid division by zero.")
            self.y_std = 1.0
        self.train_x = np.array(train_x)
        self.train_y = (train_y - self.y_mean) / self.y_std

    def _push_data(self):
        x = _lib.as_f64(self.train_x)
        y = _lib.as_f64(self.train_y).reshape(-1)
        _lib.check(self._lib.bobe_gp_set_data(self._h, _lib.ptr(x), _lib.ptr(y), x.shape[0]), "bobe_gp_set_data")

    def _push_hyper(self):
        ls = _lib.as_f64(self.lengthscales).reshape(-1)
        _lib.check(self._lib.bobe_gp_set_hyper(self._h, _lib.ptr(ls), float(self.kernel_variance), float(self.noise)),
                   "bobe_gp_set_hyper")
        self._pushed_hyper = self._hyper_key()

    def _hyper_key(self):
        """The hyper-parameters as the device holds them after a ``_push_hyper`` (what the current factor was built with)."""
        return (tuple(np.asarray(self.lengthscales, dtype=np.float64).reshape(-1).tolist()), float(self.kernel_variance),
                float(self.noise))

    # ------------------------------------------------------------------ priors / bounds
    def _setup_kernel_variance_prior(self, kernel_variance_prior):
        """BOBE/gp.py:309-320."""
        self.kernel_variance_prior_spec = kernel_variance_prior
        if self.kernel_variance_prior_spec is None:
            self.kernel_variance_prior_spec = {"name": "Uniform", "low": self.kernel_variance_bounds[0],
                                               "high": self.kernel_variance_bounds[1]}
        self.fixed_kernel_variance = (self.kernel_variance_prior_spec == "fixed")
        self.kernel_variance_prior_dist = (P.Dummy() if self.fixed_kernel_variance
                                           else P.make_distribution(self.kernel_variance_prior_spec))

    def _setup_lengthscale_prior(self, lengthscale_prior):
        """BOBE/gp.py:322-337."""
        self.lengthscale_prior_spec = lengthscale_prior
        if self.lengthscale_prior_spec is None:
            self.lengthscale_prior_spec = {"name": "Uniform", "low": self.lengthscale_bounds[0],
                                           "high": self.lengthscale_bounds[1]}
        if self.lengthscale_prior_spec == "DSLP":
            self.lengthscale_prior_dist = P.dslp(self.ndim)
        elif self.lengthscale_prior_spec == "SAAS":
            self.lengthscale_prior_dist = None
        else:
            self.lengthscale_prior_dist = P.make_distribution(self.lengthscale_prior_spec)

    def _setup_optimization_parameters(self):
        """BOBE/gp.py:339-355."""
        self.hyperparam_names = ["lengthscales"]
        bounds = [self.lengthscale_bounds] * self.ndim
        if not self.fixed_kernel_variance:
            self.hyperparam_names.append("kernel_variance")
            bounds.append(self.kernel_variance_bounds)
        if self.lengthscale_prior_spec == "SAAS":
            self.hyperparam_names.append("tausq")
            bounds.append(self.tausq_bounds)
        if self.fit_noise:                     # always the last entry
            self.hyperparam_names.append("noise")
            bounds.append(self.noise_bounds)
        self.hyperparam_bounds = np.log(np.array(bounds, dtype=np.float64).T)
        self.num_hyperparams = self.hyperparam_bounds.shape[1]

    def prior_func(self, lengthscales, kernel_variance, tausq=None) -> float:
        """BOBE/gp.py:357-366."""
        return self._prior_and_grad(lengthscales, kernel_variance, tausq)[0]

    def _prior_and_grad(self, lengthscales, kernel_variance, tausq):
        """log prior and its derivative wrt (ls, kvar, tausq) (not yet in log space)."""
        ls = np.asarray(lengthscales, dtype=np.float64)
        if self.lengthscale_prior_spec == "SAAS":
            return P.saas_logprob_and_grad(ls, kernel_variance, tausq)
        # the reference's default - Uniform on both (gp.py:313, 326) - is a constant with zero gradient: evaluated once (a
        # fit asks thousands of times), by the same expressions as below so that the value keeps its bits
        flat = (type(self.kernel_variance_prior_dist), type(self.lengthscale_prior_dist)) == (P.Uniform, P.Uniform)
        key = flat and (self.kernel_variance_prior_dist.low, self.kernel_variance_prior_dist.high,
                        self.lengthscale_prior_dist.low, self.lengthscale_prior_dist.high, ls.shape)
        if flat and getattr(self, "_flat_prior_key", None) == key:
            return self._flat_prior
        lp = float(np.sum(self.kernel_variance_prior_dist.log_prob(kernel_variance)))
        g_kvar = float(np.sum(self.kernel_variance_prior_dist.dlog_prob(kernel_variance)))
        lp += float(np.sum(self.lengthscale_prior_dist.log_prob(ls)))
        g_ls = np.asarray(self.lengthscale_prior_dist.dlog_prob(ls), dtype=np.float64)
        if flat:
            g_ls.setflags(write=False)
            self._flat_prior_key, self._flat_prior = key, (lp, g_ls, g_kvar, 0.0)
        return lp, g_ls, g_kvar, 0.0

    def _parse_hyperparams(self, log_params):
        """BOBE/gp.py:368-383."""
        hp = np.exp(np.asarray(log_params, dtype=np.float64))
        if self.fit_noise and len(hp) == self.num_hyperparams:
            hp = hp[:-1]                       # (the noise is the last entry: _parse_noise)
        ls = hp[:self.ndim]
        if self.fixed_kernel_variance:
            kvar = self.kernel_variance
            if "tausq" in self.hyperparam_names:
                tausq = hp[self.ndim] if len(hp) > self.ndim else self.tausq
            else:
                tausq = self.tausq
        else:
            kvar = hp[self.ndim]
            tausq = hp[self.ndim + 1] if len(hp) > self.ndim + 1 else self.tausq
        return ls, float(kvar), float(tausq)

    def _parse_noise(self, log_params) -> float:
        """The noise level of a hyper-parameter vector: its last entry with ``fit_noise``, else the GP's own."""
        if self.fit_noise and len(log_params) == self.num_hyperparams:
            return float(np.exp(np.asarray(log_params, dtype=np.float64)[-1]))
        return float(self.noise)

    # ------------------------------------------------------------------ objective
    def mll_data(self, lengthscales, kernel_variance, want_grad=True, slot=None):
        """Data term of the MLL (gp_mll, gp.py:170-178) and its gradient wrt (log ls, log kvar) on the GPU.
        ``slot`` (0..7): evaluate on that private stream / workspace (bobe_gp_mll_submit + _wait) so that several
        host threads — the restarts of ``fit`` — can have evaluations in flight together; same bits either way."""
        ls = _lib.as_f64(lengthscales).reshape(-1)
        mll = C.c_double(0.0)
        grad = np.empty(self.ndim + 1) if want_grad else None
        if slot is None:
            st = self._lib.bobe_gp_mll(self._h, _lib.ptr(ls), float(kernel_variance), C.byref(mll), _lib.ptr(grad))
            _lib.check(st, "bobe_gp_mll")
        else:
            _lib.check(self._lib.bobe_gp_mll_submit(self._h, int(slot), _lib.ptr(ls), float(kernel_variance),
                                                    int(want_grad)), "bobe_gp_mll_submit")
            _lib.check(self._lib.bobe_gp_mll_wait(self._h, int(slot), C.byref(mll), _lib.ptr(grad)), "bobe_gp_mll_wait")
        return mll.value, grad

    def mll_data_batch(self, lengthscales, kernel_variances, want_grad=True):
        """``mll_data`` for B hyper-parameter vectors evaluated concurrently on the GPU (bobe_gp_mll_batch).
        Vectors whose kernel matrix is not positive definite come back as NaN, like ``mll_data``."""
        ls = _lib.as_f64(lengthscales).reshape(-1, self.ndim)
        B = ls.shape[0]
        kv = _lib.as_f64(kernel_variances).reshape(B)
        mll = np.empty(B)
        grad = np.empty((B, self.ndim + 1)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        st = self._lib.bobe_gp_mll_batch(self._h, B, _lib.ptr(ls), _lib.ptr(kv), _lib.ptr(mll), _lib.ptr(grad),
                                         C.c_void_p(status.ctypes.data))
        _lib.check(st, "bobe_gp_mll_batch")
        return mll, grad

    def _noise_call(self, name, lengthscales, kernel_variance, noise, want_grad):
        ls = _lib.as_f64(lengthscales).reshape(-1)
        val = C.c_double(0.0)
        grad = np.empty(self.ndim + 2) if want_grad else None
        _lib.check(getattr(self._lib, name)(self._h, _lib.ptr(ls), float(kernel_variance), float(noise), C.byref(val),
                                            _lib.ptr(grad)), name)
        return val.value, grad

    def _noise_call_batch(self, name, lengthscales, kernel_variances, noises, want_grad):
        ls = _lib.as_f64(lengthscales).reshape(-1, self.ndim)
        B = ls.shape[0]
        kv = _lib.as_f64(kernel_variances).reshape(B)
        nz = _lib.as_f64(noises).reshape(B)
        val = np.empty(B)
        grad = np.empty((B, self.ndim + 2)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        _lib.check(getattr(self._lib, name)(self._h, B, _lib.ptr(ls), _lib.ptr(kv), _lib.ptr(nz), _lib.ptr(val),
                                            _lib.ptr(grad), C.c_void_p(status.ctypes.data)), name)
        return val, grad

    def mll_data_noise(self, lengthscales, kernel_variance, noise, want_grad=True):
        """``mll_data`` at an explicit noise level, with the gradient wrt (log ls, log kvar, log noise) - ndim + 2 entries
        (``bobe_gp_mll_noise``).  The value and the first ndim + 1 entries have ``mll_data``'s bits at the same noise."""
        return self._noise_call("bobe_gp_mll_noise", lengthscales, kernel_variance, noise, want_grad)

    def mll_data_noise_batch(self, lengthscales, kernel_variances, noises, want_grad=True):
        """``mll_data_noise`` for B vectors in lock step (``bobe_gp_mll_noise_batch``); a member has its single call's bits."""
        return self._noise_call_batch("bobe_gp_mll_noise_batch", lengthscales, kernel_variances, noises, want_grad)

    def loo_data_noise(self, lengthscales, kernel_variance, noise, want_grad=True):
        """``loo_data`` at an explicit noise level, with ndim + 2 gradient entries (``bobe_gp_loo_objective_noise``)."""
        return self._noise_call("bobe_gp_loo_objective_noise", lengthscales, kernel_variance, noise, want_grad)

    def loo_data_noise_batch(self, lengthscales, kernel_variances, noises, want_grad=True):
        """``loo_data_noise`` for B vectors in lock step (``bobe_gp_loo_objective_noise_batch``)."""
        return self._noise_call_batch("bobe_gp_loo_objective_noise_batch", lengthscales, kernel_variances, noises, want_grad)

    def _value_and_grad(self, objective, log_params, want_grad, slot=None):
        """One theta through the data term of ``objective`` ('mll' / 'loo') - the noise forms with ``fit_noise``."""
        log_params = np.asarray(log_params, dtype=np.float64)
        ls, kvar, tausq = self._parse_hyperparams(log_params)
        noise = None
        if self.fit_noise:
            noise = self._parse_noise(log_params)
            val, g_data = (self.mll_data_noise if objective == "mll" else self.loo_data_noise)(ls, kvar, noise, want_grad)
        elif objective == "mll":
            val, g_data = self.mll_data(ls, kvar, want_grad, slot=slot)
        else:
            val, g_data = self.loo_data(ls, kvar, want_grad)
        return self._assemble_objective(log_params, ls, kvar, tausq, val, g_data, want_grad, noise=noise)

    def _value_and_grad_batch(self, objective, log_params_list, want_grad):
        thetas = [np.asarray(t, dtype=np.float64) for t in log_params_list]
        parsed = [self._parse_hyperparams(t) for t in thetas]
        lss, kvs = np.array([p[0] for p in parsed]), np.array([p[1] for p in parsed])
        noises = [None] * len(thetas)
        if self.fit_noise:
            noises = [self._parse_noise(t) for t in thetas]
            fn = self.mll_data_noise_batch if objective == "mll" else self.loo_data_noise_batch
            val, g_data = fn(lss, kvs, np.array(noises), want_grad)
        else:
            val, g_data = (self.mll_data_batch if objective == "mll" else self.loo_data_batch)(lss, kvs, want_grad)
        return [self._assemble_objective(t, p[0], p[1], p[2], float(val[i]), None if g_data is None else g_data[i],
                                         want_grad, noise=noises[i]) for i, (t, p) in enumerate(zip(thetas, parsed))]

    def neg_mll(self, log_params):
        """BOBE/gp.py:385-398."""
        return self.neg_mll_value_and_grad(log_params, want_grad=False)[0]

    def neg_mll_value_and_grad(self, log_params, want_grad=True, slot=None):
        """(f, df/dtheta) with f = -(MLL + log prior), theta = log hp — the closure optim.py:306-309 builds."""
        return self._value_and_grad("mll", log_params, want_grad, slot=slot)

    def neg_mll_value_and_grad_batch(self, log_params_list, want_grad=True):
        """``neg_mll_value_and_grad`` for several theta at once (the concurrently running restarts of ``fit``);
        returns a list of (f, grad) pairs with exactly the values of the one-at-a-time call."""
        return self._value_and_grad_batch("mll", log_params_list, want_grad)

    def _assemble_objective(self, log_params, ls, kvar, tausq, mll, g_data, want_grad, noise=None):
        """``noise`` (with ``fit_noise``): the vector's noise level - its prior joins the value, and the last gradient
        entry is the data term's d / d log noise plus the prior's by the chain rule."""
        lp, g_ls, g_kvar, g_tau = self._prior_and_grad(ls, kvar, tausq)
        if noise is not None:
            lp = lp + float(np.sum(self.noise_prior_dist.log_prob(noise)))
        val = -(mll + lp)
        if not want_grad:
            return val, None
        grad = np.zeros(len(log_params))
        grad[:self.ndim] = g_data[:self.ndim] + g_ls * ls                     # chain rule: d/dlog x = x d/dx
        idx = self.ndim
        if not self.fixed_kernel_variance:
            grad[idx] = g_data[self.ndim] + g_kvar * kvar
            idx += 1
        if "tausq" in self.hyperparam_names and len(log_params) > idx:
            grad[idx] = g_tau * tausq
        if noise is not None:
            grad[-1] = g_data[self.ndim + 1] + float(np.sum(self.noise_prior_dist.dlog_prob(noise))) * noise
        return val, -grad

    # ------------------------------------------------------------------ leave-one-out cross-validation
    @property
    def fit_objective(self) -> str:
        """What ``fit`` minimises: 'mll' (default) = -(MLL + log prior), the reference's objective, or 'loo' = -(L_LOO + log
        prior) with L_LOO the leave-one-out log pseudo-likelihood (``neg_loo_value_and_grad``), which is more robust to a
        mis-specified kernel.  With 'loo' the restarts go through the same ``mll_optimize`` driver and, under the
        conditions of the MLL fit's lock-step mode, advance in lock step (``neg_loo_value_and_grad_batch``, one
        ``bobe_gp_loo_objective_batch`` call per round); the LOO objective has no slot form, so ``restart_mode='slots'``
        runs the restarts one after another.  Same iterates and result either way.  The ``'mll'`` key of ``fit``'s result
        - callers read it - holds ``-best_loss`` of the LOO objective, i.e. L_LOO + log prior at the optimum, not a
        marginal likelihood."""
        return self._fit_objective

    @fit_objective.setter
    def fit_objective(self, value: str) -> None:
        if value not in ("mll", "loo"):
            raise ValueError(f"fit_objective must be 'mll' or 'loo', not {value!r}")
        self._fit_objective = value

    def loo(self) -> dict:
        """Leave-one-out cross-validation of the fitted surrogate at its training points (Rasmussen & Williams 5.4.2), from
        the factor on the device (``bobe_gp_loo``: one pass over the stored inverse factor, no refit, no refactorisation -
        also on a GP made by ``copy`` / ``from_state_dict`` or grown by ``update``).  Hyper-parameters, noise and the
        y-standardisation are held fixed while a point is left out.  Physical units:
        ``mean`` (N) mu_-i y_std + y_mean; ``var`` (N) sigma^2_-i y_std^2 (noise included); ``z`` (N) the standardised
        residual (y_i - mu_-i) / sigma_-i; ``lpd`` (N) log predictive density of y_i (the standardised one minus log y_std);
        ``elpd`` their sum; and the summaries ``rmse`` (of y_i - mu_-i), ``max_abs_z``, ``frac_within_1sigma``,
        ``frac_within_2sigma``.  A ``GPwithClassifier`` reports on its thresholded GP subset; the gate is not applied.
        A NaN state gives NaN."""
        n = self.npoints
        mean, var, lpd = np.empty(n), np.empty(n), np.empty(n)
        s = C.c_double(0.0)
        _lib.check(self._lib.bobe_gp_loo(self._h, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(lpd), C.byref(s)), "bobe_gp_loo")
        y = np.asarray(self.train_y, dtype=np.float64).reshape(-1)
        resid = y - mean                                             # standardised
        z = resid / np.sqrt(var)
        log_ystd = math.log(self.y_std)
        az = np.abs(z)
        return {"mean": mean * self.y_std + self.y_mean, "var": var * self.y_std ** 2, "z": z, "lpd": lpd - log_ystd,
                "elpd": float(s.value) - n * log_ystd, "rmse": float(np.sqrt(np.mean(resid ** 2)) * self.y_std),
                "max_abs_z": float(np.max(az)), "frac_within_1sigma": float(np.mean(az <= 1.0)),
                "frac_within_2sigma": float(np.mean(az <= 2.0))}

    def loo_data(self, lengthscales, kernel_variance, want_grad=True):
        """Data term of the LOO objective: L_LOO = sum_i lpd_i (standardised units) at the given hyper-parameters and its
        gradient wrt (log ls, log kvar) on the GPU (``bobe_gp_loo_objective``) - the counterpart of ``mll_data``.  Does not
        disturb the factorised state.  Not positive definite: NaN."""
        ls = _lib.as_f64(lengthscales).reshape(-1)
        val = C.c_double(0.0)
        grad = np.empty(self.ndim + 1) if want_grad else None
        _lib.check(self._lib.bobe_gp_loo_objective(self._h, _lib.ptr(ls), float(kernel_variance), C.byref(val),
                                                   _lib.ptr(grad)), "bobe_gp_loo_objective")
        return val.value, grad

    def loo_data_batch(self, lengthscales, kernel_variances, want_grad=True):
        """``loo_data`` for B hyper-parameter vectors evaluated in lock step on the GPU (``bobe_gp_loo_objective_batch``) -
        the counterpart of ``mll_data_batch``.  Every member has the bits of its ``loo_data`` call; vectors whose kernel
        matrix is not positive definite come back as NaN."""
        ls = _lib.as_f64(lengthscales).reshape(-1, self.ndim)
        B = ls.shape[0]
        kv = _lib.as_f64(kernel_variances).reshape(B)
        val = np.empty(B)
        grad = np.empty((B, self.ndim + 1)) if want_grad else None
        status = np.zeros(B, dtype=np.int32)
        st = self._lib.bobe_gp_loo_objective_batch(self._h, B, _lib.ptr(ls), _lib.ptr(kv), _lib.ptr(val), _lib.ptr(grad),
                                                   C.c_void_p(status.ctypes.data))
        _lib.check(st, "bobe_gp_loo_objective_batch")
        return val, grad

    def neg_loo_value_and_grad(self, log_params, want_grad=True):
        """(f, df/dtheta) with f = -(L_LOO + log prior), theta = log hp: ``neg_mll_value_and_grad`` with the LOO log
        pseudo-likelihood in the place of the marginal likelihood (priors, a fixed kernel variance and tausq handled by the
        same ``_assemble_objective``)."""
        return self._value_and_grad("loo", log_params, want_grad)

    def neg_loo_value_and_grad_batch(self, log_params_list, want_grad=True):
        """``neg_loo_value_and_grad`` for several theta at once (the restarts of a ``fit_objective='loo'`` fit advancing in
        lock step); returns a list of (f, grad) pairs with exactly the values of the one-at-a-time call."""
        return self._value_and_grad_batch("loo", log_params_list, want_grad)

    def fit(self, x0: np.ndarray = None, maxiter: int = 500) -> dict:
        """BOBE/gp.py:400-437.  With ``fit_objective='loo'`` the returned ``'mll'`` is L_LOO + log prior at the optimum."""
        if x0 is None:
            x0 = np.log(self.get_hyperparams())[None, :]
        x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
        optimizer_options = dict(self.optimizer_options)
        # restarts are independent L-BFGS-B runs: they advance in lock step, or each gets a host thread and an evaluation
        # slot of the library
        extra = {}
        lockstep = False
        if self.concurrent_restarts and x0.shape[0] > 1 and self.mll_optimize is optimize_scipy:
            from .optim import _rc_available
            lockstep = self.restart_mode == "lockstep" or (self.restart_mode == "auto" and _rc_available())
        if self.fit_objective == "loo":
            if lockstep:                       # (no slot form of the LOO objective: otherwise one restart after another)
                extra = {"batch_value_and_grad": self.neg_loo_value_and_grad_batch}
            best_params_log, best_loss = self.mll_optimize(
                self.neg_loo_value_and_grad, num_params=self.num_hyperparams, bounds=self.hyperparam_bounds, x0=x0,
                maxiter=maxiter, n_restarts=x0.shape[0], optimizer_options=optimizer_options, **extra)
            return {"mll": -best_loss, "params": best_params_log}
        if self.concurrent_restarts and x0.shape[0] > 1 and self.mll_optimize is optimize_scipy:
            if lockstep:
                extra = {"batch_value_and_grad": self.neg_mll_value_and_grad_batch}
            elif self.fit_noise:
                extra = {}                     # (no slot form of the noise entry points: one restart after another)
            else:
                extra = {"slot_value_and_grad": lambda x, slot: self.neg_mll_value_and_grad(x, slot=slot),
                         "n_slots": self.restart_slots}
        best_params_log, best_loss = self.mll_optimize(
            self.neg_mll_value_and_grad, num_params=self.num_hyperparams, bounds=self.hyperparam_bounds, x0=x0,
            maxiter=maxiter, n_restarts=x0.shape[0], optimizer_options=optimizer_options, **extra)
        return {"mll": -best_loss, "params": best_params_log}

    def update_hyperparams(self, hyperparams):
        """BOBE/gp.py:439-448."""
        ls, kvar, tausq = self._parse_hyperparams(hyperparams)
        self.lengthscales = np.array(ls)
        if not self.fixed_kernel_variance:
            self.kernel_variance = kvar
        self.tausq = tausq
        if self.fit_noise:
            self.noise = float(np.clip(self._parse_noise(hyperparams), self.noise_bounds[0], self.noise_bounds[1]))
        self.recompute_cholesky()

    def recompute_cholesky(self):
        """BOBE/gp.py:544-550 — K, L, alpha on the GPU.  Not-PD leaves NaNs, like XLA."""
        self._push_hyper()
        st = _lib.check(self._lib.bobe_gp_factor(self._h), "bobe_gp_factor")
        self._chol_cache = None
        self._alpha_cache = None
        self.not_pd = (st == _lib.BOBE_NOT_PD)
        if self.not_pd:
            self._note_rank_test()

    def _note_rank_test(self) -> None:
        """Logged once per GP: a factorisation was refused by the rank test (a positive pivot below ``pivot_floor_ulp``
        machine epsilons of k(x,x) + noise), i.e. where LAPACK's sign test - the reference's rule - may have passed."""
        if not self._rank_test_noted and "rank test" in _lib.last_error():
            self._rank_test_noted = True
            log.warning(f"{_lib.last_error()} at kernel variance {self.kernel_variance:.3g}, noise {self.noise:.3g}: "
                        "treated as not positive definite (NaN).  pivot_floor_ulp = 0 (GP attribute, or "
                        "BOBE(gp_kwargs={'pivot_floor_ulp': 0})) restores the reference's sign-only test.")

    @property
    def refine_kappa(self) -> float:
        """Where (kernel_variance + noise) / smallest pivot of the factor exceeds this, v = L^-1 k is solved for by blocked
        forward substitution (the reference's ``solve_triangular``, gp.py:462, 484, 571) instead of multiplied out with the
        inverse factor (include/bobe_gp.h, bobe_gp_set_refine_kappa).  1e6 by default, 0 = always, negative = never; takes
        effect at the next factorisation."""
        k = C.c_double()
        _lib.check(self._lib.bobe_gp_get_refine(self._h, C.byref(k), None), "bobe_gp_get_refine")
        return float(k.value)

    @refine_kappa.setter
    def refine_kappa(self, kappa: float) -> None:
        _lib.check(self._lib.bobe_gp_set_refine_kappa(self._h, float(kappa)), "bobe_gp_set_refine_kappa")

    @property
    def solve_block(self) -> int:
        """Rows of the diagonal blocks of that substitution (a positive multiple of 128, default 128: the accuracy of
        LAPACK's triangular solve or better; include/bobe_gp.h, bobe_gp_set_solve_block)."""
        return int(self._lib.bobe_gp_get_solve_block(self._h))

    @solve_block.setter
    def solve_block(self, rows: int) -> None:
        _lib.check(self._lib.bobe_gp_set_solve_block(self._h, int(rows)), "bobe_gp_set_solve_block")

    @property
    def refining(self) -> bool:
        """Whether the current factor counts as ill conditioned: v = L^-1 k is solved for, not multiplied out."""
        a = C.c_int()
        _lib.check(self._lib.bobe_gp_get_refine(self._h, None, C.byref(a)), "bobe_gp_get_refine")
        return bool(a.value)

    @property
    def pivot_floor_ulp(self) -> float:
        """The rank test's factor (include/bobe_gp.h, "Conventions"): 0 by default = the reference's rule (only a pivot <= 0
        fails, as LAPACK's dpotrf reports it, gp.py:175, 549); u > 0: a positive pivot below u machine epsilons of k(x,x) +
        noise fails too (``BOBE(...)`` runs its surrogate with 64).  Takes effect at the next factorisation / MLL
        evaluation."""
        return float(self._lib.bobe_gp_get_pivot_floor_ulp(self._h))

    @pivot_floor_ulp.setter
    def pivot_floor_ulp(self, ulp: float) -> None:
        _lib.check(self._lib.bobe_gp_set_pivot_floor_ulp(self._h, float(ulp)), "bobe_gp_set_pivot_floor_ulp")

    # ------------------------------------------------------------------ state on the host (lazy)
    @property
    def cholesky(self) -> np.ndarray:
        """GP.cholesky (gp.py:259): N x N lower factor, fetched from the GPU on demand."""
        if self._chol_cache is None:
            n = self.npoints
            L = np.empty((n, n))
            _lib.check(self._lib.bobe_gp_get_chol(self._h, _lib.ptr(L), None), "bobe_gp_get_chol")
            self._chol_cache = L
        return self._chol_cache

    @property
    def alphas(self) -> np.ndarray:
        """GP.alphas (gp.py:260): (N, 1)."""
        if self._alpha_cache is None:
            a = np.empty(self.npoints)
            _lib.check(self._lib.bobe_gp_get_chol(self._h, None, _lib.ptr(a)), "bobe_gp_get_chol")
            self._alpha_cache = a.reshape(-1, 1)
        return self._alpha_cache

    # ------------------------------------------------------------------ kernel
    def kernel(self, xa, xb, lengthscales=None, kernel_variance=None, noise=None, include_noise=True):
        """GP.kernel(xa, xb, ls, kvar, noise, include_noise) (gp.py:124-168; call site acquisition.py:388).

        Evaluated on the GPU with the hyper-parameters passed (defaults: the GP's own)."""
        xa = _lib.as_f64(np.atleast_2d(xa))
        xb = _lib.as_f64(np.atleast_2d(xb))
        ls = _lib.as_f64(lengthscales if lengthscales is not None else self.lengthscales).reshape(-1)
        kvar = float(kernel_variance if kernel_variance is not None else self.kernel_variance)
        nz = float(noise if noise is not None else self.noise)
        out = np.empty((xa.shape[0], xb.shape[0]))
        _lib.check(self._lib.bobe_gp_kernel(self._h, _lib.ptr(xa), xa.shape[0], _lib.ptr(xb), xb.shape[0],
                                            _lib.ptr(ls), kvar, nz, 1 if include_noise else 0, _lib.ptr(out)),
                   "bobe_gp_kernel")
        return out

    # ------------------------------------------------------------------ prediction
    def _predict(self, x, want_mean, want_var, policy):
        x = _lib.as_f64(np.atleast_2d(x))
        c = x.shape[0]
        mean = np.empty(c) if want_mean else None
        var = np.empty(c) if want_var else None
        _lib.check(self._lib.bobe_gp_predict(self._h, _lib.ptr(x), c, _lib.ptr(mean), _lib.ptr(var), policy),
                   "bobe_gp_predict")
        return mean, var

    def predict_mean_batched(self, x):
        """BOBE/gp.py:450-457, 468-470."""
        m, _ = self._predict(x, True, False, 0)
        return m * self.y_std + self.y_mean

    def predict_mean_single(self, x):
        return self.predict_mean_batched(x)[0]

    def predict_var_batched(self, x):
        """BOBE/gp.py:459-466, 472-474 (clip keeps NaN)."""
        _, v = self._predict(x, False, True, 0)
        return self.y_std ** 2 * v

    def predict_var_single(self, x):
        return self.predict_var_batched(x)[0]

    def predict_batched(self, x):
        """BOBE/gp.py:476-493 — standardised (mean, var), NaN / < 1e-12 -> 1e-12."""
        return self._predict(x, True, True, 1)

    def predict_single(self, x):
        m, v = self.predict_batched(x)
        return m[0], v[0:1]

    # ------------------------------------------------------------------ joint posterior
    def predict_cov(self, x):
        """The joint posterior covariance of f + noise at the C rows of ``x`` (C x C, physical units: x y_std^2):
        k(x_i, x_j) + noise [i = j] - v_i . v_j with v = L^-1 k(X, x) - scikit-learn's ``predict(return_cov=True)`` plus
        noise I.  Its diagonal is ``predict_var_batched`` before the clip.  1 <= C <= 16384.  Not gated: a
        ``GPwithClassifier`` returns the plain GP's covariance.  A NaN state gives a NaN matrix."""
        x = _lib.as_f64(np.atleast_2d(x))
        c = x.shape[0]
        out = np.empty((c, c))
        _lib.check(self._lib.bobe_gp_predict_cov(self._h, _lib.ptr(x), c, _lib.ptr(out)), "bobe_gp_predict_cov")
        return self.y_std ** 2 * out

    def sample_posterior(self, x, n_samples=1, seed=0, z=None, centered=False, return_jitter=False):
        """``n_samples`` correlated draws of the posterior at the C rows of ``x``, an (n_samples, C) array in physical
        units: y_mean + y_std (m + L z_s), or y_std L z_s with ``centered=True`` (m: ``predict_mean_batched``'s mean in
        standardised units, L: the Cholesky factor of the standardised ``predict_cov`` with the smallest jitter that
        factorises).  ``z``: (n_samples, C) standard normals; None draws them on the device from ``seed`` (a counter
        hash: the same seed gives the same draws).  ``return_jitter``: also return the jitter added to the standardised
        covariance.  Not gated (like ``predict_cov``).  A covariance that does not factorise gives NaN draws."""
        x = _lib.as_f64(np.atleast_2d(x))
        c, s = x.shape[0], int(n_samples)
        zz = None if z is None else _lib.as_f64(z, (s, c))
        out = np.empty((s, c))
        jit = C.c_double(0.0)
        _lib.check(self._lib.bobe_gp_posterior_sample(self._h, _lib.ptr(x), c, s, int(seed) & (2 ** 64 - 1), _lib.ptr(zz),
                                                      1 if centered else 0, _lib.ptr(out), C.byref(jit)),
                   "bobe_gp_posterior_sample")
        out = self.y_std * out if centered else self.y_mean + self.y_std * out
        return (out, jit.value) if return_jitter else out

    def sample_paths(self, n_paths, n_features=2048, seed=0, *, u=None, phase=None, w=None, eps=None):
        """``n_paths`` pathwise draws of the posterior of the LATENT surrogate (no observation noise added, unlike
        ``predict_cov`` / ``sample_posterior``) as a ``PosteriorPaths`` set: functions f_s(x) = phi(x)^T w_s + k(x, X) K^-1 (y -
        Phi(X) w_s - eps_s) with ``n_features`` random Fourier features (Matheron's rule; include/bobe_gp.h,
        bobe_gp_paths_create).  Creating the set costs a few passes through the factor; evaluating it is linear in the number
        of points and has no cap.  ``u`` (F, d), ``phase`` (F,), ``w`` (S, F), ``eps`` (S, N): the caller's arrays (NumPy or
        torch CUDA tensors) instead of the device's draws from ``seed`` (the same seed gives the same paths).  The set is a
        snapshot: later ``update`` / ``fit`` calls do not change it.  Not gated: on a ``GPwithClassifier`` these are the plain
        GP's paths.  Raises ``BobeLibraryError`` on a state that is not positive definite."""
        from .paths import PosteriorPaths
        return PosteriorPaths(self, n_paths, n_features, seed, u=u, phase=phase, w=w, eps=eps)

    # ------------------------------------------------------------------ update
    def update(self, new_x, new_y):
        """BOBE/gp.py:495-541 — duplicate filter, re-standardise, full refactor."""
        new_x = np.atleast_2d(np.asarray(new_x, dtype=np.float64))
        new_y = np.atleast_2d(np.asarray(new_y, dtype=np.float64))
        pts, vals = [], []
        for i in range(new_x.shape[0]):
            if np.any(np.all(np.isclose(self.train_x, new_x[i], atol=1e-6, rtol=1e-4), axis=1)):
                log.debug(f"Point {new_x[i]} already exists in the training set, not updating")
            else:
                pts.append(new_x[i])
                vals.append(new_y[i])
        if pts:
            self.train_x = np.vstack([self.train_x, np.array(pts)])
            y_orig = np.vstack([self.train_y * self.y_std + self.y_mean, np.array(vals).reshape(-1, 1)])
            self.y_mean = float(np.mean(y_orig))
            self.y_std = float(np.std(y_orig))
            if self.y_std == 0:
                log.warning("Training targets have zero variance. Setting std to 1.0 to avoid division by zero.")
                self.y_std = 1.0
            self.train_y = (y_orig - self.y_mean) / self.y_std
            self._refresh_after_update(len(pts))

    def _refresh_after_update(self, n_new: int):
        """K, L, alpha for the grown training set (gp.py:541).  While the hyper-parameters are the ones the factor on
        the device was built with, the factor of the old points is still valid: the new rows are appended on the GPU
        (``bobe_gp_append``, the b-row form of the reference's own ``fast_update_cholesky``, gp.py:181-197) and alpha
        is re-solved for the re-standardised targets — O(b N^2) instead of O(N^3).  Everything else takes the
        reference's route, ``recompute_cholesky()`` from the CURRENT attributes (gp.py:541-550, "useful if
        hyperparameters are changed manually"): lengthscales / kernel_variance / noise set by hand since the last
        factorisation, no usable factor (NaN state), a large batch, or an append that failed."""
        if (self.append_updates and not self.not_pd and 1 <= n_new <= 64 and self.train_x.shape[0] > n_new
                and self._pushed_hyper == self._hyper_key()):
            try:
                st = self._append_rows(n_new)
            except _lib.BobeLibraryError as e:
                # (the library leaves a failed append as an empty handle: rebuild it from the host copy of the data)
                log.warning(f"append of {n_new} rows failed ({e}); refactorising")
            else:
                self._chol_cache = self._alpha_cache = None
                self.not_pd = (st == _lib.BOBE_NOT_PD)
                return
        self._push_data()
        self.recompute_cholesky()

    def _append_rows(self, n_new: int) -> int:
        xn = _lib.as_f64(self.train_x[-n_new:])
        ya = _lib.as_f64(self.train_y).reshape(-1)
        return _lib.check(self._lib.bobe_gp_append(self._h, _lib.ptr(xn), n_new, _lib.ptr(ya)), "bobe_gp_append")

    # ------------------------------------------------------------------ fantasy variance / sweep
    def fantasy_var(self, new_x, mc_points, k_train_mc=None):
        """BOBE/gp.py:552-576.  ``k_train_mc`` is accepted for signature parity and recomputed on the GPU.
        ``new_x`` may hold several candidates; the result is then (C, M)."""
        new_x = _lib.as_f64(np.atleast_2d(new_x))
        z = _lib.as_f64(np.atleast_2d(mc_points))
        out = np.empty((new_x.shape[0], z.shape[0]))
        _lib.check(self._lib.bobe_gp_fantasy_var(self._h, _lib.ptr(new_x), new_x.shape[0], _lib.ptr(z), z.shape[0],
                                                 float(self.y_std), _lib.ptr(out)), "bobe_gp_fantasy_var")
        return out[0] if out.shape[0] == 1 else out

    CRITERIA = ("wipv", "wipstd", "imiqr", "eiv")

    @staticmethod
    def _log_weights(log_weights, m):
        """``log_weights`` as what the library takes: None, a contiguous float64 torch CUDA tensor of M entries, or a finite
        float64 array.  A device tensor is not read here: that its entries are finite is the caller's responsibility."""
        if log_weights is None:
            return None
        if hasattr(log_weights, "data_ptr"):
            import torch
            if int(log_weights.numel()) != m:
                raise ValueError(f"log_weights must have one entry per integration point ({m})")
            if log_weights.dtype != torch.float64 or not log_weights.is_cuda or not log_weights.is_contiguous():
                raise ValueError("a log_weights tensor must be a contiguous float64 CUDA tensor")
            return log_weights
        lw = _lib.as_f64(np.asarray(log_weights, dtype=np.float64).reshape(-1))
        if lw.shape[0] != m or not np.all(np.isfinite(lw)):
            raise ValueError(f"log_weights must be {m} finite values")
        return lw

    def _wip_sweep_w(self, cand, z, log_weights, criteria):
        """``bobe_gp_wip_sweep_w``: the requested scores in physical units, their argmins / minima and log S; the key 'zvar'
        goes to ``bobe_gp_wip_sweep_zvar`` (a sweep of its own)."""
        keys = self.CRITERIA if criteria is None else tuple(criteria)
        for k in keys:
            if k not in self.CRITERIA and k != "zvar":
                raise ValueError(f"criteria must be among {self.CRITERIA + ('zvar',)}, not {k!r}")
        c, m = int(cand.shape[0]), int(z.shape[0])
        lw = self._log_weights(log_weights, m)
        out = {}
        if any(k in self.CRITERIA for k in keys) or not keys:
            arrs = [np.empty(c) if k in keys else None for k in self.CRITERIA]
            log_s = C.c_double(0.0)
            am, mn = np.full(4, -1, dtype=np.int64), np.empty(4)
            _lib.check(self._lib.bobe_gp_wip_sweep_w(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std),
                                                     _lib.ptr(lw), *[_lib.ptr(a) for a in arrs], C.byref(log_s), _lib.ptr(am),
                                                     _lib.ptr(mn)), "bobe_gp_wip_sweep_w")
            # exp(f) lives on the physical scale: the y_mean the library leaves out shifts the log scores by a constant
            shift = {"wipv": 0.0, "wipstd": 0.0, "imiqr": float(self.y_mean), "eiv": -2.0 * float(self.y_mean)}
            for i, k in enumerate(self.CRITERIA):
                if k in keys:
                    out[k] = arrs[i] + shift[k] if shift[k] else arrs[i]
                    out["argmin_" + k], out["min_" + k] = int(am[i]), float(mn[i]) + shift[k]
            out["log_eiv_total"] = log_s.value + 2.0 * float(self.y_mean)
        if "zvar" in keys:
            zv = np.empty(c)
            lez, zmin, zam = C.c_double(0.0), C.c_double(0.0), C.c_int64(-1)
            _lib.check(self._lib.bobe_gp_wip_sweep_zvar(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std),
                                                        _lib.ptr(lw), _lib.ptr(zv), C.byref(lez), C.byref(zam),
                                                        C.byref(zmin)), "bobe_gp_wip_sweep_zvar")
            # (omega is normalised: no y_mean in the score; log E[Z] is on the physical scale)
            out["zvar"], out["argmin_zvar"], out["min_zvar"] = zv, int(zam.value), float(zmin.value)
            out["log_ez"] = lez.value + float(self.y_mean)
        return out

    def wip_sweep(self, candidates, mc_points, want_mean_var=False, *, log_weights=None, criteria=None):
        """All-candidate WIPV / WIPStd scores (acquisition.py:385-398 + 438-465) in one GPU call.

        ``candidates`` / ``mc_points`` may be NumPy arrays or torch CUDA tensors (no copy then).
        Returns dict(wipv, wipstd, argmin_v, min_v, argmin_s, min_s[, mean, var]).

        ``log_weights`` (M finite log quadrature weights of the integration points under the flat prior on the unit cube, up to
        a constant; None: the points are draws of the surrogate posterior) and / or ``criteria`` (a subset of ``wipv, wipstd,
        imiqr, eiv``; None with weights: all four) select ``bobe_gp_wip_sweep_w`` instead: the result then holds the requested
        scores (to minimise, physical units), ``argmin_<key>`` / ``min_<key>`` for each, and ``log_eiv_total`` = log S (the
        expected integrated variance of a candidate is ``exp(log_eiv_total) - exp(-eiv)``).

        ``criteria`` also accepts ``'zvar'`` (never implied by None): ``zvar`` = -log T(c), the candidate's term of the expected
        posterior variance of the evidence estimate Z after one more evaluation (``bobe_gp_wip_sweep_zvar``; to minimise), with
        ``argmin_zvar`` / ``min_zvar`` and ``log_ez`` = log E[Z]: the expected reduction of Var Z is ``exp(2 log_ez - zvar)``.
        Its scoring pass grows with M^2 (a pair sum over the integration points).  Requested together with other keys it costs
        a second device sweep; the other keys' values are those of a call without it, bit for bit."""
        dev = hasattr(candidates, "data_ptr")
        cand = candidates if dev else _lib.as_f64(np.atleast_2d(candidates))
        z = mc_points if hasattr(mc_points, "data_ptr") else _lib.as_f64(np.atleast_2d(mc_points))
        if log_weights is not None or criteria is not None:
            if want_mean_var:
                raise ValueError("want_mean_var goes with the equal-weight sweep only")
            return self._wip_sweep_w(cand, z, log_weights, criteria)
        c, m = int(cand.shape[0]), int(z.shape[0])
        wipv, wipstd = np.empty(c), np.empty(c)
        mean = np.empty(c) if want_mean_var else None
        var = np.empty(c) if want_mean_var else None
        av, asd = C.c_int64(-1), C.c_int64(-1)
        mv, ms = C.c_double(0.0), C.c_double(0.0)
        _lib.check(self._lib.bobe_gp_wip_sweep(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std),
                                               _lib.ptr(wipv), _lib.ptr(wipstd), _lib.ptr(mean), _lib.ptr(var),
                                               C.byref(av), C.byref(mv), C.byref(asd), C.byref(ms)),
                   "bobe_gp_wip_sweep")
        out = {"wipv": wipv, "wipstd": wipstd, "argmin_v": av.value, "min_v": mv.value, "argmin_s": asd.value,
               "min_s": ms.value}
        if want_mean_var:
            out["mean"], out["var"] = mean, var
        return out

    def evidence_moments(self, mc_points, *, log_weights=None):
        """Mean and TOTAL variance of the evidence estimate Z = sum_z e^{l_z} e^{f(z)} over the integration points under the
        surrogate's joint posterior (``bobe_gp_evidence_moments``): the closed form of the lognormal estimate, with the
        posterior covariance of every pair of points formed on the fly - nothing is stored, factorised or drawn, so M is
        bounded by what ``wip_sweep`` holds for the same points, not by M^2.

        ``mc_points``: NumPy array or torch CUDA tensor; ``log_weights`` as in ``wip_sweep`` (None: l_z = -mu_z).  Returns
        ``log_ez`` = log E[Z] (physical: y_mean added; ``wip_sweep(criteria=('zvar',))``'s), ``log_t0`` = log (Var Z /
        E[Z]^2), ``log_var_z`` = log_t0 + 2 log_ez and ``std_logz`` = sqrt(log1p(exp(log_t0))), the standard deviation of
        log Z of the lognormal with these two moments.  ``exp(-zvar[c] - log_t0)`` is the share of the evidence variance that an
        evaluation at candidate c is expected to remove (``zvar`` of ``wip_sweep`` on the same points and weights)."""
        z = mc_points if hasattr(mc_points, "data_ptr") else _lib.as_f64(np.atleast_2d(mc_points))
        m = int(z.shape[0])
        lw = self._log_weights(log_weights, m)
        lez, lt0 = C.c_double(0.0), C.c_double(0.0)
        _lib.check(self._lib.bobe_gp_evidence_moments(self._h, _lib.ptr(z), m, float(self.y_std), _lib.ptr(lw), C.byref(lez),
                                                      C.byref(lt0)), "bobe_gp_evidence_moments")
        log_ez, log_t0 = lez.value + float(self.y_mean), lt0.value
        return {"log_ez": log_ez, "log_t0": log_t0, "log_var_z": log_t0 + 2.0 * log_ez, "std_logz": std_from_log_t0(log_t0)}

    def wip_select_batch(self, candidates, mc_points, n_batch, criterion="wipstd", return_stage_scores=False):
        """A kriging-believer batch of ``n_batch`` WIPV / WIPStd picks out of ``candidates`` from ONE sweep
        (``bobe_gp_wip_select_batch``): stage 0 is ``wip_sweep`` (same bits), every later member a rank-one downdate of the
        sweep's retained intermediates on the device instead of a sweep on a surrogate that gained the pick.  A picked
        candidate is not picked again.  ``y_std`` is held fixed over the batch (the believer loop standardises again after
        every member; in standardised units the two agree).  Not gated.

        ``candidates`` / ``mc_points``: NumPy arrays or torch CUDA tensors.  Returns dict(indices (n_batch,), points
        (n_batch, d), scores (n_batch,) - the winning score of every stage[, stage_scores (n_batch, C) - every stage's scores
        of all candidates]).

        ``criterion`` 'imiqr' / 'eiv' (see ``wip_sweep``) are ``wip_select_batch_w`` without weights."""
        return self.wip_select_batch_w(candidates, mc_points, n_batch, criterion, return_stage_scores)

    def wip_select_batch_w(self, candidates, mc_points, n_batch, criterion="wipstd", return_stage_scores=False, *,
                           log_weights=None):
        """``wip_select_batch`` with importance-weighted integration points (``log_weights``, see ``wip_sweep``) and the four
        criteria 'wipv', 'wipstd', 'imiqr', 'eiv' (``bobe_gp_wip_select_batch_w``): stage 0 is the weighted ``wip_sweep``
        (same bits), the scores are physical ones as there.  Without weights 'wipv' / 'wipstd' take the equal-weight entry.
        ``criterion='zvar'`` (see ``wip_sweep``) goes to ``bobe_gp_wip_select_batch_zvar``."""
        if criterion not in self.CRITERIA and criterion != "zvar":
            raise ValueError(f"criterion must be one of {self.CRITERIA + ('zvar',)}, not {criterion!r}")
        dev = hasattr(candidates, "data_ptr")
        cand = candidates if dev else _lib.as_f64(np.atleast_2d(candidates))
        z = mc_points if hasattr(mc_points, "data_ptr") else _lib.as_f64(np.atleast_2d(mc_points))
        c, m, nb = int(cand.shape[0]), int(z.shape[0]), int(n_batch)
        picks = np.full(max(nb, 1), -1, dtype=np.int64)
        scores = np.empty(max(nb, 1))
        stage = np.empty((max(nb, 1), c)) if return_stage_scores else None
        if criterion == "zvar":
            lw = self._log_weights(log_weights, m)
            _lib.check(self._lib.bobe_gp_wip_select_batch_zvar(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std),
                                                               _lib.ptr(lw), nb, _lib.ptr(picks), _lib.ptr(scores),
                                                               _lib.ptr(stage)), "bobe_gp_wip_select_batch_zvar")
        elif log_weights is None and criterion in ("wipv", "wipstd"):
            _lib.check(self._lib.bobe_gp_wip_select_batch(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std), nb,
                                                          0 if criterion == "wipv" else 1, _lib.ptr(picks), _lib.ptr(scores),
                                                          _lib.ptr(stage)), "bobe_gp_wip_select_batch")
        else:
            lw = self._log_weights(log_weights, m)
            _lib.check(self._lib.bobe_gp_wip_select_batch_w(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std),
                                                            _lib.ptr(lw), nb, self.CRITERIA.index(criterion), _lib.ptr(picks),
                                                            _lib.ptr(scores), _lib.ptr(stage)), "bobe_gp_wip_select_batch_w")
            shift = {"imiqr": float(self.y_mean), "eiv": -2.0 * float(self.y_mean)}.get(criterion, 0.0)
            if shift:
                scores += shift
                if stage is not None:
                    stage += shift
        pts = cand[picks.tolist()].detach().cpu().numpy() if dev else np.array(cand[picks])
        out = {"indices": picks, "points": pts, "scores": scores}
        if return_stage_scores:
            out["stage_scores"] = stage
        return out

    def acq_ei(self, x, best_y, zeta=0.0, log_ei=False):
        """+EI / +log EI at x (acquisition.py:226-253, 318-330), standardised units."""
        x = _lib.as_f64(np.atleast_2d(x))
        out = np.empty(x.shape[0])
        _lib.check(self._lib.bobe_gp_acq_ei(self._h, _lib.ptr(x), x.shape[0], float(best_y), float(zeta),
                                            1 if log_ei else 0, _lib.ptr(out)), "bobe_gp_acq_ei")
        return out

    def acq_ei_grad(self, x, best_y, zeta=0.0, log_ei=False):
        """(val (C,), grad (C, d)): +EI / +log EI at the rows of x with their input gradients, standardised units like
        ``acq_ei`` - one device call (``bobe_gp_acq_ei_grad``: ``predict_grad``'s chain and one kernel behind it, value and
        gradient from the same posterior).  A point's row does not depend on the rest of the batch; under a classifier gate
        an infeasible point has ``acq_ei``'s value and a zero gradient."""
        x = _lib.as_f64(np.atleast_2d(x))
        c = x.shape[0]
        val, grad = np.empty(c), np.empty((c, self.ndim))
        _lib.check(self._lib.bobe_gp_acq_ei_grad(self._h, _lib.ptr(x), c, float(best_y), float(zeta), 1 if log_ei else 0,
                                                 _lib.ptr(val), _lib.ptr(grad)), "bobe_gp_acq_ei_grad")
        return val, grad

    def wip_grad(self, candidates, mc_points):
        """(wipv, wipstd, dwipv/dx, dwipstd/dx) of the candidates — values and input gradients of ``WIPV.fun`` /
        ``WIPStd.fun`` (acquisition.py:438-465), the gradient being what the reference takes with ``jax.grad`` in the
        local refinement (acquisition.py:403-412).  Physical units (the y_std factors of gp.py:576 included)."""
        cand = _lib.as_f64(np.atleast_2d(candidates))
        z = _lib.as_f64(np.atleast_2d(mc_points))
        c = cand.shape[0]
        wipv, wipstd = np.empty(c), np.empty(c)
        dv, ds = np.empty((c, self.ndim)), np.empty((c, self.ndim))
        _lib.check(self._lib.bobe_gp_wip_grad(self._h, _lib.ptr(cand), c, _lib.ptr(z), z.shape[0], float(self.y_std),
                                              _lib.ptr(wipv), _lib.ptr(wipstd), _lib.ptr(dv), _lib.ptr(ds)),
                   "bobe_gp_wip_grad")
        return wipv, wipstd, dv, ds

    def wip_grad_w(self, candidates, mc_points, *, log_weights=None, criteria=None):
        """Values and input gradients of the weighted scores (``bobe_gp_wip_grad_w``): a dict with ``<key>`` (C,) and
        ``d<key>`` (C, d) for every requested criterion (``criteria``: a subset of ``wipv, wipstd, imiqr, eiv``; None: all
        four).  ``candidates`` / ``mc_points``: NumPy arrays or torch CUDA tensors.  ``log_weights`` and the units are those
        of ``wip_sweep(log_weights=, criteria=)``: physical, the y_mean shifts of ``imiqr`` / ``eiv`` included in the values
        (constants: the gradients do not see them).  Matrix-vector work in groups of 16 candidates, for at most 4096 training
        points."""
        keys = self.CRITERIA if criteria is None else tuple(criteria)
        for k in keys:
            if k not in self.CRITERIA:
                raise ValueError(f"criteria must be among {self.CRITERIA}, not {k!r}")
        cand = candidates if hasattr(candidates, "data_ptr") else _lib.as_f64(np.atleast_2d(candidates))
        z = mc_points if hasattr(mc_points, "data_ptr") else _lib.as_f64(np.atleast_2d(mc_points))
        c, m = int(cand.shape[0]), int(z.shape[0])
        lw = self._log_weights(log_weights, m)
        vals = [np.empty(c) if k in keys else None for k in self.CRITERIA]
        grads = [np.empty((c, self.ndim)) if k in keys else None for k in self.CRITERIA]
        pv = (C.c_void_p * 4)(*[_lib.ptr(a).value for a in vals])
        pg = (C.c_void_p * 4)(*[_lib.ptr(a).value for a in grads])
        _lib.check(self._lib.bobe_gp_wip_grad_w(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std), _lib.ptr(lw),
                                                pv, pg), "bobe_gp_wip_grad_w")
        shift = {"wipv": 0.0, "wipstd": 0.0, "imiqr": float(self.y_mean), "eiv": -2.0 * float(self.y_mean)}
        out = {}
        for i, k in enumerate(self.CRITERIA):
            if k in keys:
                out[k] = vals[i] + shift[k] if shift[k] else vals[i]
                out["d" + k] = grads[i]
        return out

    def wip_grad_zvar(self, candidates, mc_points, *, log_weights=None):
        """Value and input gradient of the evidence-variance score (``bobe_gp_wip_grad_zvar``): ``{"zvar": (C,), "dzvar":
        (C, d), "log_ez": float}``.  ``candidates`` / ``mc_points``: NumPy arrays or torch CUDA tensors.  ``log_weights`` and
        the units are those of ``wip_sweep(criteria=('zvar',))``: physical, y_mean added to ``log_ez``, no shift in the score.
        A candidate whose score is +inf (it teaches nothing) has a zero gradient.  Matrix-vector work in groups of 16
        candidates, for at most 4096 training points; the pair stage grows with M^2 per candidate."""
        cand = candidates if hasattr(candidates, "data_ptr") else _lib.as_f64(np.atleast_2d(candidates))
        z = mc_points if hasattr(mc_points, "data_ptr") else _lib.as_f64(np.atleast_2d(mc_points))
        c, m = int(cand.shape[0]), int(z.shape[0])
        lw = self._log_weights(log_weights, m)
        zv, dz = np.empty(c), np.empty((c, self.ndim))
        lez = C.c_double(0.0)
        _lib.check(self._lib.bobe_gp_wip_grad_zvar(self._h, _lib.ptr(cand), c, _lib.ptr(z), m, float(self.y_std), _lib.ptr(lw),
                                                   _lib.ptr(zv), _lib.ptr(dz), C.byref(lez)), "bobe_gp_wip_grad_zvar")
        return {"zvar": zv, "dzvar": dz, "log_ez": lez.value + float(self.y_mean)}

    def predict_grad(self, x, mean_only=False):
        """Standardised (mean, var, dmean/dx, dvar/dx) of ``predict_single`` (gp.py:476-489) for C points: what the
        reference gets by JAX autodiff through the GP (acquisition.py:246-253, samplers.py:268-276).
        ``mean_only``: (mean, None, dmean/dx, None) from one small kernel — the HMC sampler's call."""
        x = _lib.as_f64(np.atleast_2d(x))
        c = x.shape[0]
        if mean_only:
            mean, dmean = np.empty(c), np.empty((c, self.ndim))
            _lib.check(self._lib.bobe_gp_predict_grad(self._h, _lib.ptr(x), c, _lib.ptr(mean), None, _lib.ptr(dmean),
                                                      None), "bobe_gp_predict_grad")
            return mean, None, dmean, None
        mean, var = np.empty(c), np.empty(c)
        dmean, dvar = np.empty((c, self.ndim)), np.empty((c, self.ndim))
        _lib.check(self._lib.bobe_gp_predict_grad(self._h, _lib.ptr(x), c, _lib.ptr(mean), _lib.ptr(var),
                                                  _lib.ptr(dmean), _lib.ptr(dvar)), "bobe_gp_predict_grad")
        return mean, var, dmean, dvar

    def hmc_leapfrog(self, U, Pm, inv_mass, eps: float, L: int, temp: float = 1.0):
        """``L`` leapfrog steps of P Hamiltonian-Monte-Carlo chains on the surrogate's mean in ONE GPU launch
        (``bobe_gp_hmc_leapfrog``): U, Pm are (P, d) positions in logit space and momenta (Pm = p0 + eps/2 * grad).
        Returns (U', Pm', logp, grad, mean (physical units), X')."""
        U = _lib.as_f64(np.atleast_2d(U)).copy()
        Pm = _lib.as_f64(np.atleast_2d(Pm)).copy()
        im = _lib.as_f64(inv_mass).reshape(-1)
        P = U.shape[0]
        logp, mean = np.empty(P), np.empty(P)
        grad, X = np.empty_like(U), np.empty_like(U)
        _lib.check(self._lib.bobe_gp_hmc_leapfrog(self._h, P, _lib.ptr(U), _lib.ptr(Pm), _lib.ptr(im), float(eps), int(L),
                                                  float(self.y_std), float(self.y_mean), float(temp), _lib.ptr(logp),
                                                  _lib.ptr(grad), _lib.ptr(mean), _lib.ptr(X)), "bobe_gp_hmc_leapfrog")
        return U, Pm, logp, grad, mean, X

    def hmc_run(self, state, adapt, inv_mass, seed: int, it0: int, niter: int, do_adapt: bool, temp: float = 1.0,
                hist_from: Optional[int] = None, thin: int = 0, debug: bool = False):
        """``niter`` whole HMC trajectories of every chain in ONE GPU launch (``bobe_gp_hmc_run``): ``state`` (P, 3d+2) =
        [u, dlogp/du, x, logp, mean] and ``adapt`` (P, 5) = [eps, mu, hbar, log_eps_bar, m] are updated in place.
        Returns (hist, keep, dbg): u after the iterations >= ``hist_from`` (niter - hist_from, P, d), [x, mean] after
        every ``thin``-th iteration (niter // thin, P, d+1), and the last iteration's draws (P, d+3) - each None
        unless asked for."""
        P, d = state.shape[0], self.ndim
        assert state.shape == (P, 3 * d + 2) and adapt.shape == (P, 5) and state.flags.c_contiguous and adapt.flags.c_contiguous
        im = _lib.as_f64(inv_mass).reshape(-1)
        hist = np.empty((niter - hist_from, P, d)) if hist_from is not None else None
        keep = np.empty((niter // thin, P, d + 1)) if thin else None
        dbg = np.empty((P, d + 3)) if debug else None
        _lib.check(self._lib.bobe_gp_hmc_run(self._h, P, _lib.ptr(state), _lib.ptr(adapt), _lib.ptr(im), int(seed), int(it0),
                                             int(niter), int(bool(do_adapt)), float(self.y_std), float(self.y_mean), float(temp),
                                             int(hist_from or 0), _lib.ptr(hist) if hist is not None else None,
                                             int(thin) if thin else 1, _lib.ptr(keep) if keep is not None else None,
                                             _lib.ptr(dbg) if dbg is not None else None), "bobe_gp_hmc_run")
        return hist, keep, dbg

    def nuts_run(self, state, adapt, inv_metric, max_tree_depth: int, seed: int, it0: int, niter: int, do_adapt: bool,
                 temp: float = 1.0, hist_from: Optional[int] = None, thin: int = 0, stats: bool = False,
                 debug: bool = False):
        """``niter`` No-U-Turn transitions of every chain in ONE GPU launch (``bobe_gp_nuts_run``; the reference's NUTS,
        samplers.py:216-330): ``state`` (P, 3d+2) and ``adapt`` (P, 5) as in ``hmc_run``, updated in place;
        ``inv_metric`` the (d, d) inverse metric.  Returns (hist, keep, stats, dbg): u after the iterations >=
        ``hist_from`` (niter - hist_from, P, d), [x, mean] after every ``thin``-th iteration (niter // thin, P, d+1), per
        transition [tree depth, leapfrog steps, divergent, acceptance statistic] (niter, P, 4) and the last transition's
        momentum draw (P, d) - each None unless asked for."""
        P, d = state.shape[0], self.ndim
        assert state.shape == (P, 3 * d + 2) and adapt.shape == (P, 5) and state.flags.c_contiguous and adapt.flags.c_contiguous
        im = np.ascontiguousarray(_lib.as_f64(inv_metric).reshape(d, d))
        hist = np.empty((niter - hist_from, P, d)) if hist_from is not None else None
        keep = np.empty((niter // thin, P, d + 1)) if thin else None
        st = np.empty((niter, P, 4)) if stats else None
        dbg = np.empty((P, d)) if debug else None
        _lib.check(self._lib.bobe_gp_nuts_run(self._h, P, _lib.ptr(state), _lib.ptr(adapt), _lib.ptr(im),
                                              int(max_tree_depth), int(seed), int(it0), int(niter), int(bool(do_adapt)),
                                              float(self.y_std), float(self.y_mean), float(temp), int(hist_from or 0),
                                              _lib.ptr(hist) if hist is not None else None, int(thin) if thin else 1,
                                              _lib.ptr(keep) if keep is not None else None,
                                              _lib.ptr(st) if st is not None else None,
                                              _lib.ptr(dbg) if dbg is not None else None), "bobe_gp_nuts_run")
        return hist, keep, st, dbg

    def rwalk(self, x, logl, step, lstar: float, walks: int, seed: int, debug: bool = False):
        """Constrained random walks of P walkers on the surrogate's mean in ONE GPU launch (``bobe_gp_rwalk``): the
        replacement search of nested sampling (dynesty's 'rwalk', samplers.py:64, 152).  ``x`` (P, d) start points with
        their physical-unit means ``logl``; ``step`` (d, d) lower-triangular proposal factor; a step is accepted inside the
        unit cube above ``lstar`` (and inside the classifier's region when a gate is set).
        Returns (x', logl', n_accepted, n_inside[, last proposals])."""
        x = _lib.as_f64(np.atleast_2d(x)).copy()
        if x.shape[1] != self.ndim:
            raise ValueError(f"walkers have {x.shape[1]} coordinates, the GP has {self.ndim}")
        lg = _lib.as_f64(logl).reshape(-1).copy()
        st = _lib.as_f64(step).reshape(self.ndim, self.ndim)
        P = x.shape[0]
        nacc, nin = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        dbg = np.empty_like(x) if debug else None
        _lib.check(self._lib.bobe_gp_rwalk(self._h, P, _lib.ptr(x), _lib.ptr(lg), _lib.ptr(st), float(lstar), int(walks),
                                           int(seed), float(self.y_std), float(self.y_mean), C.c_void_p(nacc.ctypes.data),
                                           C.c_void_p(nin.ctypes.data), _lib.ptr(dbg) if debug else None), "bobe_gp_rwalk")
        return (x, lg, nacc, nin, dbg) if debug else (x, lg, nacc, nin)

    def get_random_point(self, rng=None, nstd=None):
        """BOBE/gp.py:578-585."""
        rng = rng if rng is not None else get_numpy_rng()
        return rng.uniform(0, 1, size=self.train_x.shape[1])

    # ------------------------------------------------------------------ state (gp.py:587-750)
    def state_dict(self, with_factor: bool = True):
        """Same keys as BOBE/gp.py:597-634 (npz-interchangeable).  ``with_factor=False`` (internal, ``copy``) leaves
        the N x N factor on the GPU."""
        state = {
            "train_x": np.array(self.train_x),
            "train_y": np.array(self.train_y * self.y_std + self.y_mean),
            "lengthscales": np.array(self.lengthscales),
            "kernel_variance": float(self.kernel_variance),
            "noise": float(self.noise),
            "tausq": float(self.tausq),
            "y_mean": float(self.y_mean),
            "y_std": float(self.y_std),
            "kernel_name": self.kernel_name,
            "lengthscale_prior_spec": self.lengthscale_prior_spec,
            "kernel_variance_prior_spec": self.kernel_variance_prior_spec,
            "fixed_kernel_variance": self.fixed_kernel_variance,
            "optimizer_method": self.optimizer_method,
            "optimizer_options": self.optimizer_options,
            "lengthscale_bounds": self.lengthscale_bounds,
            "kernel_variance_bounds": self.kernel_variance_bounds,
            "tausq_bounds": self.tausq_bounds,
            "cholesky": np.array(self.cholesky) if with_factor else None,
            "alphas": np.array(self.alphas) if with_factor else None,
            "ndim": self.ndim,
            "gp_class": "GP",
        }
        if self.fit_noise:                     # (off: key for key the reference's dictionary)
            state.update(self._noise_state())
        return state

    def _noise_state(self) -> dict:
        return {"fit_noise": True, "noise_bounds": list(self.noise_bounds), "noise_prior": self.noise_prior_spec}

    @classmethod
    def from_state_dict(cls, state, device: int = 0, _clone_of=None):
        """BOBE/gp.py:638-677 — L and alpha are restored on the GPU without refactorising (``_clone_of``: take them
        from that GP's device state instead of ``state``)."""
        def plain(v):
            return v.item() if isinstance(v, np.ndarray) and v.shape == () else v
        gp = cls(train_x=state["train_x"], train_y=state["train_y"], noise=plain(state["noise"]),
                 kernel=plain(state["kernel_name"]), optimizer=plain(state["optimizer_method"]),
                 optimizer_options=plain(state["optimizer_options"]), lengthscales=state["lengthscales"],
                 kernel_variance=plain(state["kernel_variance"]),
                 lengthscale_bounds=list(np.asarray(state["lengthscale_bounds"]).tolist()),
                 kernel_variance_bounds=list(np.asarray(state["kernel_variance_bounds"]).tolist()),
                 kernel_variance_prior=plain(state.get("kernel_variance_prior_spec")),
                 lengthscale_prior=plain(state.get("lengthscale_prior_spec")),
                 tausq=plain(state.get("tausq", 1.0)),
                 tausq_bounds=list(np.asarray(state.get("tausq_bounds", [1e-4, 1e4])).tolist()), device=device,
                 _factor=False, fit_noise=bool(plain(state.get("fit_noise", False))),
                 noise_bounds=list(np.asarray(state.get("noise_bounds", [1e-10, 1e-1])).tolist()),
                 noise_prior=plain(state.get("noise_prior")))
        L, a = state.get("cholesky"), state.get("alphas")
        if _clone_of is not None:
            _lib.check(gp._lib.bobe_gp_clone_state(gp._h, _clone_of._h), "bobe_gp_clone_state")
            gp.not_pd = bool(_clone_of.not_pd)
            # the host copy of the standardisation too, bit for bit (a state_dict round trip re-derives it)
            gp.train_y, gp.y_mean, gp.y_std = np.array(_clone_of.train_y), _clone_of.y_mean, _clone_of.y_std
            gp._pushed_hyper = _clone_of._pushed_hyper       # (the clone carries the source's device hyper-parameters)
            gp._chol_cache, gp._alpha_cache = None, None
        elif L is not None and a is not None and np.all(np.isfinite(np.asarray(L, dtype=np.float64))):
            L = _lib.as_f64(L)
            a = _lib.as_f64(a).reshape(-1)
            gp._push_hyper()
            _lib.check(gp._lib.bobe_gp_set_chol(gp._h, _lib.ptr(L), _lib.ptr(a)), "bobe_gp_set_chol")
            gp._chol_cache, gp._alpha_cache = None, None
        else:
            gp.recompute_cholesky()
        return gp

    @classmethod
    def load(cls, filename, **kwargs):
        """BOBE/gp.py:679-721; further keywords override entries of the stored state, as there.  One keyword is this
        build's own: ``device`` (HIP device of the restored GP, default 0)."""
        device = int(kwargs.pop("device", 0))
        if not filename.endswith(".npz"):
            filename += ".npz"
        data = np.load(filename, allow_pickle=True)
        state = {}
        for key in data.files:
            value = data[key]
            state[key] = value.item() if isinstance(value, np.ndarray) and value.shape == () else value
        state.update(kwargs)
        return cls.from_state_dict(state, device=device)

    def save(self, filename="gp"):
        """BOBE/gp.py:723-737."""
        if not filename.endswith(".npz"):
            filename += ".npz"
        np.savez(filename, **self.state_dict())

    def copy(self):
        """BOBE/gp.py:740-750 — an independent GP with the same data, hyper-parameters and factor.  The reference goes
        through ``state_dict`` / ``from_state_dict``; here the device state is duplicated on the GPU
        (``bobe_gp_clone_state``): no N x N host round trip, no factorisation."""
        state = self.state_dict(with_factor=False)
        new = self.__class__.from_state_dict(state, device=self.device, _clone_of=self)
        return new

    @property
    def npoints(self):
        return self.train_x.shape[0]

    def get_hyperparams(self):
        """BOBE/gp.py:756-762."""
        hp = np.array(self.lengthscales, dtype=np.float64)
        if not self.fixed_kernel_variance:
            hp = np.hstack([hp, self.kernel_variance])
        if self.lengthscale_prior_spec == "SAAS":
            hp = np.hstack([hp, self.tausq])
        if self.fit_noise:
            hp = np.hstack([hp, self.noise])
        return hp

    def hyperparams_dict(self):
        """BOBE/gp.py:764-772."""
        ls_str = {name: f"{float(val):.4f}" for name, val in zip(self.param_names, self.lengthscales)}
        out = {"lengthscales": ls_str, "kernel_variance": f"{float(self.kernel_variance):.4f}"}
        if "tausq" in self.hyperparam_names:
            out["tausq"] = f"{float(self.tausq):.4f}"
        if self.fit_noise:
            out["noise"] = f"{float(self.noise):.4e}"
        return out
