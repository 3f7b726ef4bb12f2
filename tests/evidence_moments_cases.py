"""The cases of the evidence-moments tests (tests/test_evidence_moments_cpu.py, tests/test_gpu_evidence_moments.py) and their
references, each computed once per process: the float64 restatement and the long-double truth of
tests/evidence_moments_restatement.py.  Imports nothing from bobe_amd."""
import functools

import numpy as np

import evidence_moments_restatement as E

NOISE, KVAR = 1e-6, 2.0
# (seed, N, d, M): one element, two, the tile edge (127, 128, 129), three and four tile rows of the pair matrix (257, 300, 385:
# non-adjacent off-diagonal tiles), d up to 8
SHAPES = [(201, 130, 3, 1), (202, 130, 3, 2), (203, 130, 3, 127), (204, 130, 3, 128), (205, 130, 3, 129), (206, 64, 2, 257),
          (207, 257, 5, 300), (208, 40, 8, 385)]
KERNELS = ("rbf", "matern")
Y_STDS = (1.0, 30.0, 4e3)
CASES = [(s, k, y, w) for s in SHAPES for k in KERNELS for y in Y_STDS for w in (True, False)]


def case_id(case):
    (seed, n, d, m), kernel, y_std, weighted = case
    return "s%d-N%d-d%d-M%d-%s-ystd%g-%s" % (seed, n, d, m, kernel, y_std, "weights" if weighted else "posterior_draws")


def lengthscale(d):
    return 0.4 if d <= 3 else 0.8


def case_data(shape, y_std):
    """``zvar_cases.case_data``'s recipe without candidates: uniform points, the same target function rescaled to the standard
    deviation ``y_std`` (mean kept), log-weights 1.5 N(0, 1)."""
    seed, n, d, m = shape
    rng = np.random.default_rng(seed)
    X, Z = rng.uniform(size=(n, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    lw = 1.5 * rng.normal(size=m)
    y = (y - np.mean(y)) / np.std(y) * y_std + np.mean(y)
    return X, y, Z, lw


def standardise(y):
    mean, std = float(np.mean(y)), float(np.std(y))
    return (y - mean) / std, mean, std


@functools.lru_cache(maxsize=None)
def states(shape, kernel, y_std):
    """(float64 state, long-double state, y_mean, y_std as standardised)."""
    d = shape[2]
    X, y, Z, _ = case_data(shape, y_std)
    ys, y_mean, std = standardise(y)
    ls = np.full(d, lengthscale(d))
    return (E.state(kernel, X, ys, Z, ls, KVAR, NOISE, np.float64), E.state(kernel, X, ys, Z, ls, KVAR, NOISE, np.longdouble),
            y_mean, std)


@functools.lru_cache(maxsize=None)
def reference(case):
    """{"f64": (log_ez, log_t0), "truth": (log_ez, log_t0)} - log_ez physical (y_mean added) - and "y_std" of a case."""
    shape, kernel, y_std, weighted = case
    s64, sld, y_mean, std = states(shape, kernel, y_std)
    lw = case_data(shape, y_std)[3] if weighted else None
    a, b = E.evidence_moments(s64, std, lw), E.evidence_moments(sld, std, lw)
    return {"f64": (float(a["log_ez"]) + y_mean, float(a["log_t0"])),
            "truth": (b["log_ez"] + np.longdouble(y_mean), b["log_t0"]), "y_std": std}
