"""The cases of tests/test_gpu_posterior_grad.py with their references (the np.longdouble truth and the fp64 restatement), each
computed once; tests/test_posterior_grad_cpu.py holds the fp64 restatement of the same cases to the truth.  Imports nothing
from bobe_amd.

Data: ``case_data(1000 + 10 d + n, n, d, c, m)`` of tests/test_gpu_weighted_criteria.py, kernel variance 2, noise 1e-6,
lengthscale 0.4 (0.8 at d = 32, where k(x, X) would otherwise sink below ~1e-2 of the kernel variance)."""
import functools

import numpy as np

import posterior_grad_restatement as PG
import weighted_grad_restatement as R
from test_gpu_weighted_criteria import case_data, standardise

NOISE, KVAR = 1e-6, 2.0
DTYPES = (np.longdouble, np.float64)               # (truth, fp64 restatement) throughout


def ell_of(d):
    return 0.8 if d == 32 else 0.4


# ---------------------------------------------------------------------------------------------------------- predict_grad
# (kernel, d, N, C, chunk): what each shape is there for stands beside it
PREDICT_CASES = [
    ("rbf", 3, 160, 9, 0),         # the ill-conditioned family (variances ~1e-5 of the kernel variance)
    ("matern", 5, 300, 65, 0),     # two workgroups, the second with one live query; training tiles 128 / 128 / 44
    ("rbf", 8, 129, 64, 0),        # d = DCAP 8; the second tile holds one row: slices 1-3 idle there
    ("matern", 16, 160, 1, 0),     # d = DCAP 16; a single query
    ("rbf", 12, 160, 9, 0),        # DCAP 16
    ("matern", 17, 160, 9, 0),     # DCAP 32
    ("rbf", 32, 160, 9, 0),        # d = DCAP 32
    ("matern", 2, 3, 5, 0),        # N = 3: fewer rows than slices
    ("matern", 5, 300, 200, 128),  # two launches of 128 + 72 queries
]


def predict_id(case):
    k, d, n, c, chunk = case
    return f"{k}_d{d}_N{n}_C{c}" + (f"_chunk{chunk}" if chunk else "")


@functools.lru_cache(maxsize=None)
def predict_data(case):
    """(X, y, Q) of a predict_grad case"""
    _, d, n, c, _ = case
    X, y, Q, _, _ = case_data(1000 + 10 * d + n, n, d, c, 1)
    if n == 3:
        y = X[:, 0] + X[:, 1]
    return X, y, Q


@functools.lru_cache(maxsize=None)
def predict_reference(case):
    """((mean, var, dmean, dvar, floored) of the truth, the same of the fp64 restatement)"""
    kernel, d, _, _, _ = case
    X, y, Q = predict_data(case)
    ys, _, _ = standardise(y)
    return tuple(PG.posterior_and_grad(kernel, X, ys, Q, np.full(d, ell_of(d)), KVAR, NOISE, dt) for dt in DTYPES)


# ------------------------------------------------------------------------------------------------------------- the floor
FLOOR_N, FLOOR_D, FLOOR_KVAR, FLOOR_NOISE = 40, 5, 1.0, 1e-14
FLOOR_ELL = {"rbf": 0.12, "matern": 0.05}


@functools.lru_cache(maxsize=None)
def floor_data(kernel):
    """(X, y, Q): query 0 lies 1e-9 from X[0], query 1 IS X[1] - both on the 1e-12 floor at noise 1e-14 -, seven more in
    [0.1, 0.9], which at these lengthscales see next to nothing of the 40 training points (var > 0.5)."""
    rng = np.random.default_rng(77)
    X = rng.uniform(size=(FLOOR_N, FLOOR_D))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2] * X[:, 3] + 0.1 * rng.normal(size=FLOOR_N)
    Q = rng.uniform(0.1, 0.9, size=(9, FLOOR_D))
    Q[0] = X[0] + 1e-9
    Q[1] = X[1]
    return X, y, Q


@functools.lru_cache(maxsize=None)
def floor_reference(kernel, noise=FLOOR_NOISE):
    X, y, Q = floor_data(kernel)
    ys, _, _ = standardise(y)
    return tuple(PG.posterior_and_grad(kernel, X, ys, Q, np.full(FLOOR_D, FLOOR_ELL[kernel]), FLOOR_KVAR, noise, dt)
                 for dt in DTYPES)


# -------------------------------------------------------------------------------------------------- wip_grad, batched path
# (kernel, d, N, M, C, chunk)
WIP_KEYS = ("wipv", "wipstd", "dwipv", "dwipstd")
WIP_CASES = [
    ("matern", 5, 300, 300, 17, 0),    # one chunk; last tile 44 rows = 5 x 8 + a tail of 4; two z passes
    ("rbf", 3, 131, 33, 17, 0),        # last tile 3 rows: the tail only
    ("rbf", 12, 160, 70, 200, 128),    # two chunks of 128 + 72 candidates
]


def wip_id(case):
    k, d, n, m, c, chunk = case
    return f"{k}_d{d}_N{n}_M{m}_C{c}" + (f"_chunk{chunk}" if chunk else "")


@functools.lru_cache(maxsize=None)
def wip_data(case):
    """(X, y, candidates in [0.1, 0.9], Z)"""
    _, d, n, m, c, _ = case
    X, y, cand, Z, _ = case_data(1000 + 10 * d + n, n, d, c, m)
    return X, y, 0.1 + 0.8 * cand, Z


@functools.lru_cache(maxsize=None)
def wip_reference(case):
    """(truth, fp64 restatement): dicts with wipv / wipstd (C,), dwipv / dwipstd (C, d) in physical units - the equal-weight
    scores of tests/weighted_grad_restatement.py, omega = 1 / M"""
    kernel, d, _, _, _, _ = case
    X, y, cand, Z = wip_data(case)
    ys, _, y_std = standardise(y)
    out = []
    for dt in DTYPES:
        st = R.State(kernel, X, ys, Z, np.full(d, ell_of(d)), KVAR, NOISE, y_std, None, dt)
        r = R.value_and_grad(st, cand)
        out.append({k: r[k] for k in WIP_KEYS})
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------ the leapfrog
HMC_KEYS = ("U", "Pm", "logp", "grad", "mean", "X")
HMC_CASES = [("rbf", 3, 160), ("matern", 8, 300), ("rbf", 17, 160)]
HMC_STEPS = (1, 9)
HMC_P, HMC_EPS, HMC_TEMP = 7, 0.07, 1.3


def hmc_id(case, L):
    k, d, n = case
    return f"{k}_d{d}_N{n}_L{L}"


@functools.lru_cache(maxsize=None)
def hmc_data(case):
    """(X, y, U ~ N(0, 0.5^2) clipped to +-3, Pm ~ N(0, 1), inv_mass in [0.5, 2])"""
    _, d, n = case
    X, y, _, _, _ = case_data(1000 + 10 * d + n, n, d, 1, 1)
    rng = np.random.default_rng(7000 + 10 * d + n)
    U = np.clip(0.5 * rng.normal(size=(HMC_P, d)), -3.0, 3.0)
    return X, y, U, rng.normal(size=(HMC_P, d)), rng.uniform(0.5, 2.0, size=d)


@functools.lru_cache(maxsize=None)
def hmc_reference(case, L):
    """(truth, fp64 restatement): dicts over HMC_KEYS"""
    kernel, d, _ = case
    X, y, U, Pm, im = hmc_data(case)
    ys, y_mean, y_std = standardise(y)
    return tuple(dict(zip(HMC_KEYS, PG.leapfrog(kernel, X, ys, np.full(d, ell_of(d)), KVAR, NOISE, y_mean, y_std, U, Pm, im,
                                                 HMC_EPS, L, HMC_TEMP, dt))) for dt in DTYPES)


def rel_err(a, truth):
    """max |a - truth| / max |truth|"""
    t = np.asarray(truth)
    return float(np.max(np.abs(np.asarray(a, dtype=t.dtype) - t)) / np.max(np.abs(t)))
