"""Classifier functions - counterpart of BOBE/clf.py: the SVM (train_svm_classifier clf.py:36-69,
get_svm_predict_proba_fn :71-78, CLASSIFIER_REGISTRY :169-182, svm_predict / svm_predict_proba :188-213) and the ellipsoid
(train_ellipsoid_classifier :125-156, get_ellipsoid_predict_proba_fn :158-166, train_with_restarts :221-285,
EllipsoidClassifier :375-412, train_ellipsoid :415-466, train_ellipsoid_multiple_restarts :468-472).

scikit-learn trains the SVM, as in the reference; its decision function is evaluated by the library on the device, by
direct differences in one fixed summation order (``bobe_gp_set_gate`` / ``bobe_gp_gate_eval``, k_gate): a handle that
carries nothing but the gate serves the module-level functions.  The ellipsoid classifier is trained ON THE DEVICE:
every restart's whole AdamW run in one launch (``bobe_gp_train_ellipsoid``, k_ellipsoid_train); the host draws the
restart seeds, the initial parameters and the batch permutations exactly as the reference draws them, and picks the
restart.  Its gate (``bobe_gp_set_gate_ellipsoid``) is evaluated by the same device functions as the SVM's.
The Flax-MLP classifier of clf.py:84-123, 287-372 is not built; ``CLASSIFIER_REGISTRY`` lists the SVM only,
GPwithClassifier dispatches the ellipsoid itself."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .utils import get_logger, get_numpy_rng

log = get_logger("clf")


def train_svm_classifier(X, Y, settings=None, init_params=None, **kwargs):
    """clf.py:36-69: SVC(kernel='rbf', gamma='scale', C=1e7); returns (params, metrics, predict_proba_fn) - the third
    member evaluates ``svm_predict_proba`` of the fitted parameters on the device.  ``init_params`` / further keywords are
    accepted for the reference's call signature and unused, as there."""
    from sklearn.svm import SVC
    settings = settings or {}
    C = settings.get("C", 1e7)
    clf = SVC(kernel=settings.get("kernel", "rbf"), gamma=settings.get("gamma", "scale"), C=C)
    clf.fit(np.asarray(X), np.asarray(Y))
    params = {"support_vectors": np.array(clf.support_vectors_), "dual_coef": np.array(clf.dual_coef_[0]),
              "intercept": float(clf.intercept_[0]), "gamma_eff": float(clf._gamma)}
    metrics = {"n_support_vectors": len(params["support_vectors"]), "gamma": f"{params['gamma_eff']:.2e}",
               "C": f"{C:.2e}", "intercept": f"{params['intercept']:.2e}"}
    return params, metrics, get_svm_predict_proba_fn(params, device=int(kwargs.get("device", 0)))


def get_svm_predict_proba_fn(params, device: int = 0) -> Callable[[np.ndarray], np.ndarray]:
    """clf.py:71-78: the probability function of stored SVM parameters (``svm_predict_proba``, clf.py:210-213) — evaluated
    by the library (``bobe_gp_gate_eval`` on a data-less handle that carries only the gate)."""
    return _DeviceSVM(params, device).proba


def svm_predict(x, support_vectors, dual_coef, intercept: float, gamma: float):
    """clf.py:188-209: decision(x) = sum_i dual_coef[i] exp(-gamma |support_vectors[i] - x|^2) + intercept, on the device.
    One point (n_features,) gives a scalar, as there; a batch (n, n_features) gives n values."""
    x = np.asarray(x, dtype=np.float64)
    dec = _DeviceSVM({"support_vectors": support_vectors, "dual_coef": dual_coef, "intercept": intercept,
                      "gamma_eff": gamma}).decision(x)
    return float(dec[0]) if x.ndim == 1 else dec


def svm_predict_proba(x, support_vectors, dual_coef, intercept: float, gamma: float):
    """clf.py:211-213: 1.0 where the decision function is >= 0, else 0.0."""
    dec = svm_predict(x, support_vectors, dual_coef, intercept, gamma)
    return np.where(np.asarray(dec) >= 0, 1.0, 0.0) if np.ndim(dec) else (1.0 if dec >= 0 else 0.0)


CLASSIFIER_REGISTRY = {                       # clf.py:169-182 ('nn' is not built; GPwithClassifier dispatches the ellipsoid)
    "svm": {"train_fn": train_svm_classifier, "predict_fn": get_svm_predict_proba_fn},
}


class _DeviceSVM:
    """A library handle holding nothing but a classifier gate: decision values / probabilities of stored parameters."""

    def __init__(self, params, device: int = 0):
        import ctypes as C
        from . import _lib
        self._lib = _lib.load()
        self._ndim = int(np.asarray(params["support_vectors"]).shape[1])
        self._h = C.c_void_p(0)
        _lib.check(self._lib.bobe_gp_create(C.byref(self._h), int(device), 0, self._ndim), "bobe_gp_create")
        install_gate(self._lib, self._h, params, 0.5, 0.0)

    def __del__(self):
        try:
            if self._h.value:
                self._lib.bobe_gp_destroy(self._h)
        except Exception:
            pass

    def decision(self, x):
        return gate_eval(self._lib, self._h, x, self._ndim)[0]

    def proba(self, x):
        return gate_eval(self._lib, self._h, x, self._ndim)[1]


def install_gate(lib, handle, params, probability_threshold: float, minus_inf: float) -> None:
    """Hand the trained SVM to the library (``bobe_gp_set_gate``); ``params=None`` clears the gate."""
    from . import _lib
    if params is None:
        _lib.check(lib.bobe_gp_set_gate(handle, None, 0, None, 0.0, 0.0, float(probability_threshold), float(minus_inf)),
                   "bobe_gp_set_gate")
        return
    sv = _lib.as_f64(np.atleast_2d(np.asarray(params["support_vectors"])))
    dual = _lib.as_f64(np.asarray(params["dual_coef"])).reshape(-1)
    _lib.check(lib.bobe_gp_set_gate(handle, _lib.ptr(sv), sv.shape[0], _lib.ptr(dual), float(params["intercept"]),
                                    float(params["gamma_eff"]), float(probability_threshold), float(minus_inf)),
               "bobe_gp_set_gate")


def gate_eval(lib, handle, x, ndim: int):
    """(decision, feasible) of the points ``x`` from the gate held by ``handle`` (``bobe_gp_gate_eval``)."""
    from . import _lib
    x = _lib.as_f64(np.atleast_2d(np.asarray(x, dtype=np.float64)).reshape(-1, ndim))
    dec, ok = np.empty(x.shape[0]), np.empty(x.shape[0])
    _lib.check(lib.bobe_gp_gate_eval(handle, _lib.ptr(x), x.shape[0], _lib.ptr(dec), _lib.ptr(ok)), "bobe_gp_gate_eval")
    return dec, ok


def gate_proba(lib, handle, x, ndim: int):
    """The gate's probability of the points ``x`` (``bobe_gp_gate_proba``: SVM 0 / 1, ellipsoid sigmoid(logit))."""
    from . import _lib
    x = _lib.as_f64(np.atleast_2d(np.asarray(x, dtype=np.float64)).reshape(-1, ndim))
    out = np.empty(x.shape[0])
    _lib.check(lib.bobe_gp_gate_proba(handle, _lib.ptr(x), x.shape[0], _lib.ptr(out)), "bobe_gp_gate_proba")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Ellipsoid classifier (clf.py:375-472): logit = -alpha (x - mu)^T L L^T (x - mu) + beta around the best point mu
# ---------------------------------------------------------------------------------------------------------------------
MAX_ELLIPSOID_DIM = 32                  # the library's dimension limit (bobe_gp.h)


class EllipsoidClassifier:
    """clf.py:377-412: the configuration of the ellipsoid classifier (the reference's Flax module fields and defaults).
    ``patience``, ``val_frac``, ``seed_offset`` and ``split_seed`` are accepted and unused, as there.  An unknown keyword
    raises ``TypeError``, as constructing the module with it does.  ``init`` / ``apply`` stand for the module's: the initial
    parameter tree of a seed (flat_L ~ Normal(0, init_scale) drawn by ``np.random.default_rng(seed)``, alpha = 1,
    beta = 0) and the logits of points, evaluated on the device."""

    def __init__(self, d, mu, init_scale: float = 0.1, lr: float = 1e-2, weight_decay: float = 1e-4, n_epochs: int = 1000,
                 batch_size: int = 64, patience: int = 25, n_restarts: int = 2, val_frac: float = 0.1, seed_offset: int = 0,
                 split_seed: int = 42):
        d = int(d)
        if not 1 <= d <= MAX_ELLIPSOID_DIM:
            raise ValueError(f"the ellipsoid classifier supports 1 <= d <= {MAX_ELLIPSOID_DIM} (got d = {d})")
        self.d, self.mu = d, np.asarray(mu, dtype=np.float64).reshape(d)
        self.init_scale, self.lr, self.weight_decay = float(init_scale), float(lr), float(weight_decay)
        self.n_epochs, self.batch_size, self.patience = int(n_epochs), int(batch_size), patience
        self.n_restarts, self.val_frac, self.seed_offset, self.split_seed = int(n_restarts), val_frac, seed_offset, split_seed

    @property
    def n_tril(self) -> int:
        return self.d * (self.d + 1) // 2

    def init(self, seed) -> dict:
        flat_L = np.random.default_rng(int(seed)).normal(0.0, self.init_scale, size=self.n_tril)
        return {"params": {"flat_L": flat_L, "alpha": np.float64(1.0), "beta": np.float64(0.0)}}

    def apply(self, params, x, train: bool = False, device: int = 0):
        return _DeviceEllipsoid(params, self.d, self.mu, device=device).decision(x)


def _ell_theta(params, d: int) -> np.ndarray:
    """The parameter tree ({'params': {flat_L, alpha, beta}}, optionally 'mu') as the flat vector the library trains."""
    p = params["params"]
    flat = np.asarray(p["flat_L"], dtype=np.float64).reshape(-1)
    if flat.shape[0] != d * (d + 1) // 2:
        raise ValueError(f"flat_L has {flat.shape[0]} entries, d = {d} needs {d * (d + 1) // 2}")
    return np.concatenate([flat, [float(p["alpha"]), float(p["beta"])]])


def _ell_tree(theta: np.ndarray, mu: np.ndarray) -> dict:
    t = len(theta) - 2
    return {"params": {"flat_L": np.array(theta[:t]), "alpha": np.float64(theta[t]), "beta": np.float64(theta[t + 1])},
            "mu": np.array(mu, dtype=np.float64)}


def ellipsoid_permutations(seed, n: int, n_epochs: int, batch_size: int) -> np.ndarray:
    """clf.py:446-452: the rows of every batch of one training run - ``np.random.RandomState(seed)``, one permutation
    per epoch, batch i = perm[i B:(i + 1) B], the tail dropped (one batch of all rows when n < B).
    Shape (n_epochs, steps * min(B, n)), int32."""
    steps = max(1, n // batch_size)
    width = steps * min(batch_size, n)
    rs = np.random.RandomState(int(seed))
    out = np.empty((n_epochs, width), dtype=np.int32)
    for e in range(n_epochs):
        out[e] = rs.permutation(n)[:width]
    return out


def _select_best(results):
    """clf.py:268-281: the restart with the smallest full-data loss as formatted "%.2e", strict < (a tie keeps the
    first)."""
    best_loss, best_params, best_metrics = np.inf, None, {}
    for params, metrics in results:
        loss = float(metrics["train_loss"])
        if loss < best_loss:
            best_loss, best_params, best_metrics = loss, params, metrics
    return best_params, best_metrics


def _device_train(model: EllipsoidClassifier, x, y, inits, perms, handle=None, device: int = 0):
    """All restarts of ``inits`` (R, P) / ``perms`` (R, n_epochs, width) in one ``bobe_gp_train_ellipsoid`` launch:
    [(params tree, metrics)] in restart order."""
    from . import _lib
    x = _lib.as_f64(np.asarray(x, dtype=np.float64).reshape(-1, model.d))
    y = _lib.as_f64(np.asarray(y, dtype=np.float64).reshape(-1))
    if y.shape[0] != x.shape[0]:
        raise ValueError("x and y have different numbers of rows")
    inits = _lib.as_f64(np.asarray(inits, dtype=np.float64).reshape(len(inits), -1))
    perms = np.ascontiguousarray(perms, dtype=np.int32)
    nr = inits.shape[0]
    n = x.shape[0]
    width = max(1, n // max(1, model.batch_size)) * min(model.batch_size, n)
    if inits.shape[1] != model.n_tril + 2 or perms.shape != (nr, model.n_epochs, width):
        raise ValueError(f"initial parameters {inits.shape} / permutation table {perms.shape} do not match "
                         f"({nr}, {model.n_tril + 2}) / ({nr}, {model.n_epochs}, {width})")
    out, loss = np.empty_like(inits), np.empty(nr)
    mu = _lib.as_f64(model.mu)
    own = None
    if handle is None:
        own = _DeviceEllipsoid(None, model.d, model.mu, device=device)
        handle = (own._lib, own._h)
    lib, h = handle
    _lib.check(lib.bobe_gp_train_ellipsoid(h, _lib.ptr(x), _lib.ptr(y), x.shape[0], _lib.ptr(mu), nr, _lib.ptr(inits),
                                           perms.ctypes.data_as(_lib.C.c_void_p), model.n_epochs, model.batch_size,
                                           model.lr, model.weight_decay, _lib.ptr(out), _lib.ptr(loss)),
               "bobe_gp_train_ellipsoid")
    return [(_ell_tree(out[r], model.mu), {"train_loss": f"{loss[r]:.2e}", "epochs": model.n_epochs}) for r in range(nr)]


def train_with_restarts(train_fn: Callable, x, y, n_restarts: int = 2, seed_offset: int = 0, split_seed: int = 42,
                        init_params=None, **train_kwargs):
    """clf.py:221-285: ``n_restarts`` calls of ``train_fn(x_train=x, y_train=y, seed=s, init_params=...)`` - the seeds
    drawn from the global NumPy generator in restart order (``integers(0, 2**32 - 1)``), restart 0 from
    ``init_params`` - and the restart of the smallest "%.2e" loss (strict <).  ``seed_offset`` / ``split_seed`` are
    unused, as there.  (The ellipsoid's own wrapper runs its restarts concurrently with the same draws.)"""
    rng = get_numpy_rng()
    results = []
    for i in range(n_restarts):
        seed = rng.integers(0, 2 ** 32 - 1)
        results.append(train_fn(x_train=x, y_train=y, seed=seed, init_params=init_params if i == 0 else None,
                                **train_kwargs))
    return _select_best(results)


def train_ellipsoid(model: EllipsoidClassifier, x_train, y_train, seed: int = 0, init_params=None, **kwargs):
    """clf.py:415-466: one AdamW run on the device (``bobe_gp_train_ellipsoid`` with one restart): from
    ``init_params`` or ``model.init(seed)``, batches from ``np.random.RandomState(seed)``.  Returns (params, metrics)
    with metrics = {'train_loss': "%.2e" of the full-data loss, 'epochs': n_epochs}."""
    n = int(np.asarray(x_train).shape[0])
    theta = _ell_theta(init_params if init_params is not None else model.init(seed), model.d)
    perms = ellipsoid_permutations(seed, n, model.n_epochs, model.batch_size)
    return _device_train(model, x_train, y_train, theta[None], perms[None], handle=kwargs.get("handle"),
                         device=int(kwargs.get("device", 0)))[0]


def train_ellipsoid_multiple_restarts(model: EllipsoidClassifier, x, y, **kwargs):
    """clf.py:468-472 (``train_with_restarts`` of ``train_ellipsoid``), the restarts in ONE launch: the same seed draws
    from the global generator, in order, the same initial parameters and permutations per restart, the same choice.
    Keywords: ``init_params`` (restart 0), and this build's ``device`` / ``handle``."""
    n = int(np.asarray(x).shape[0])
    rng = get_numpy_rng()
    seeds = [rng.integers(0, 2 ** 32 - 1) for _ in range(model.n_restarts)]
    init_params = kwargs.get("init_params")
    inits = np.stack([_ell_theta(init_params if (i == 0 and init_params is not None) else model.init(s), model.d)
                      for i, s in enumerate(seeds)])
    perms = np.stack([ellipsoid_permutations(s, n, model.n_epochs, model.batch_size) for s in seeds])
    return _select_best(_device_train(model, x, y, inits, perms, handle=kwargs.get("handle"),
                                      device=int(kwargs.get("device", 0))))


def train_ellipsoid_classifier(X, Y, settings=None, init_params=None, **kwargs):
    """clf.py:125-156: (params, metrics, predict_proba_fn) of the ellipsoid centred at ``kwargs['best_pt']`` (default
    0.5 ones(d), as there); ``settings`` are EllipsoidClassifier fields.  params = {'params': {'flat_L', 'alpha',
    'beta'}, 'mu': the centre} - the centre travels with the parameters."""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    mu = np.asarray(kwargs.get("best_pt", 0.5 * np.ones(d)), dtype=np.float64)
    model = EllipsoidClassifier(d=d, mu=mu, **(settings or {}))
    params, metrics = train_ellipsoid_multiple_restarts(model, X, Y, init_params=init_params, handle=kwargs.get("handle"),
                                                        device=int(kwargs.get("device", 0)))
    return params, metrics, get_ellipsoid_predict_proba_fn(params, settings, d, best_pt=mu,
                                                           device=int(kwargs.get("device", 0)))


def get_ellipsoid_predict_proba_fn(params, settings, d, **kwargs):
    """clf.py:158-166: sigmoid(logit) of stored parameters, on the device.  The centre is ``kwargs['best_pt']``, else
    the one saved in ``params['mu']``, else 0.5 ones(d) (the reference's only choice on reload)."""
    mu = kwargs.get("best_pt")
    if mu is None:
        mu = params.get("mu") if isinstance(params, dict) else None
    if mu is None:
        mu = 0.5 * np.ones(int(d))
    EllipsoidClassifier(d=d, mu=mu, **(settings or {}))                     # (the reference's keyword check)
    device, gate = int(kwargs.get("device", 0)), []

    def predict_proba_fn(x):
        if not gate:                                      # (the device handle is made on first use)
            gate.append(_DeviceEllipsoid(params, int(d), mu, device=device))
        return gate[0].proba(x)
    return predict_proba_fn


class _DeviceEllipsoid:
    """A library handle holding nothing but an ellipsoid gate (or none yet: a trainer)."""

    def __init__(self, params, d: int, mu, device: int = 0):
        import ctypes as C
        from . import _lib
        self._lib = _lib.load()
        self._ndim = int(d)
        self._h = C.c_void_p(0)
        _lib.check(self._lib.bobe_gp_create(C.byref(self._h), int(device), 0, self._ndim), "bobe_gp_create")
        if params is not None:
            install_ellipsoid_gate(self._lib, self._h, params, mu, 0.5, 0.0)

    def __del__(self):
        try:
            if self._h.value:
                self._lib.bobe_gp_destroy(self._h)
        except Exception:
            pass

    def decision(self, x):
        return gate_eval(self._lib, self._h, x, self._ndim)[0]

    def proba(self, x):
        return gate_proba(self._lib, self._h, x, self._ndim)


def install_ellipsoid_gate(lib, handle, params, mu, probability_threshold: float, minus_inf: float) -> None:
    """Hand a trained ellipsoid to the library (``bobe_gp_set_gate_ellipsoid``: the raw flat_L, the library transforms
    the diagonal); ``mu=None`` takes the centre saved in ``params``."""
    from . import _lib
    p = params["params"]
    d = int(round((np.sqrt(8 * np.asarray(p["flat_L"]).size + 1) - 1) / 2))
    flat = _lib.as_f64(np.asarray(p["flat_L"], dtype=np.float64).reshape(-1))
    centre = _lib.as_f64(np.asarray(params["mu"] if mu is None else mu, dtype=np.float64).reshape(d))
    _lib.check(lib.bobe_gp_set_gate_ellipsoid(handle, _lib.ptr(flat), _lib.ptr(centre), float(p["alpha"]),
                                              float(p["beta"]), float(probability_threshold), float(minus_inf)),
               "bobe_gp_set_gate_ellipsoid")
