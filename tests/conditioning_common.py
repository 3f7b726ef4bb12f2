"""The conditioning ladder's design, rungs, tolerances and error measures, shared by tests/test_gpu_conditioning.py (fresh
factorisations) and tests/test_gpu_append_conditioning.py (appended and kriging-believer states): see the former's
docstring for what the rungs are and why the comparison is err(HIP) <= 4 x err(LAPACK) + TOL."""
import numpy as np
from scipy.stats import qmc

D = 10
FLOOR = 1e-12          # gp.py:16


def _rosen10(x):
    return -np.sum(100.0 * (x[..., 1:] - x[..., :-1] ** 2) ** 2 + (1.0 - x[..., :-1]) ** 2, axis=-1) / 20.0


def _bo_like_design(n, seed=0):
    """A training set with the character of a BO run on config 5's likelihood (bounds [-2, 2]^10, unit-cube coordinates):
    64 scrambled-Sobol points, then states of tempered random-walk Metropolis chains on the likelihood (T = 1, 4, 16:
    a BO design crowds the posterior bulk and thins out around it).  Deterministic on the CPU; also returns posterior
    samples (T = 1) that are NOT in the design, as integration / query points."""
    rng = np.random.default_rng(seed)
    pts = [qmc.Sobol(D, scramble=True, seed=seed).random(64)]
    spare = []
    per = (n - 64 + 2) // 3
    for T in (1.0, 4.0, 16.0):
        u = np.full(D, 0.75)                                   # x = 1: the maximum
        lu = _rosen10(4 * u - 2)
        keep, step, it = [], 0.015 * np.sqrt(T), 0
        while len(keep) < per + (256 if T == 1.0 else 0):
            it += 1
            prop = u + step * rng.standard_normal(D)
            if np.all((prop > 0) & (prop < 1)):
                lp = _rosen10(4 * prop - 2)
                if np.log(rng.uniform()) < (lp - lu) / T:
                    u, lu = prop, lp
                    if it % 7 == 0:
                        keep.append(u.copy())
        pts.append(np.array(keep[:per]))
        if T == 1.0:
            spare = np.array(keep[per:])
    X = np.vstack(pts)[:n]
    return X, _rosen10(4 * X - 2), spare


def ladder_points(X, spare, rung):
    """The ladder's 96 candidates (32 near training points, 32 posterior samples off the design, 32 Sobol points) and 64
    integration points for rung ``rung`` on the design ``X`` and its spare posterior samples."""
    n = X.shape[0]
    rng = np.random.default_rng(100 + rung)
    near = np.clip(X[rng.choice(n, 32, replace=False)] + 0.02 * rng.standard_normal((32, D)), 0.0, 1.0)
    cand = np.vstack([near, spare[:32], qmc.Sobol(D, scramble=True, seed=5).random(32)])
    return cand, spare[64:128]


# (N, kernel, length scales, kernel variance): the first nine dimensions share the first number, as the fits of the run did
LADDER = [
    (600, "rbf", [0.70, 0.79, 0.84, 0.87, 0.78, 0.80, 0.83, 0.74, 0.69, 3.10], 10.6),
    (1200, "rbf", [1.25] * 9 + [5.0], 432.0),
    (1800, "rbf", [2.31, 2.27, 2.27, 2.27, 2.27, 2.27, 2.27, 2.27, 2.27, 5.0], 4.67e4),
    (1800, "rbf", [2.99, 2.94, 2.93, 2.93, 2.93, 2.93, 2.93, 2.93, 2.93, 5.0], 3.5e5),
    (1800, "rbf", [3.35, 3.28, 3.28, 3.28, 3.28, 3.29, 3.29, 3.29, 3.30, 5.0], 8.51e5),
    (1800, "rbf", [3.80, 3.73, 3.72, 3.73, 3.73, 3.73, 3.74, 3.74, 3.75, 5.0], 2.48e6),
    (600, "matern", [0.70, 0.79, 0.84, 0.87, 0.78, 0.80, 0.83, 0.74, 0.69, 3.10], 10.6),
    (1800, "matern", [2.31, 2.27, 2.27, 2.27, 2.27, 2.27, 2.27, 2.27, 2.27, 5.0], 4.67e4),
    (1800, "matern", [3.35, 3.28, 3.28, 3.28, 3.28, 3.29, 3.29, 3.29, 3.30, 5.0], 1.0e6),
]
NOISE = 1e-8
# the floor of the assertion: the fp64 parity tolerances of SURVEY.md 8(d) (|dLML| / |LML| <= 1e-10, gradient 1e-8, mean 1e-8,
# variance 1e-9 relative ... 1e-7) - an error inside them passes whatever LAPACK's happens to be on a well-conditioned rung
TOL = {"mll": 1e-10, "grad": 1e-8, "mean": 1e-8, "var": 1e-9, "fantasy": 1e-9, "wipv": 1e-7, "wipstd": 1e-7}


def _floored(v):
    v = np.where(np.isnan(v), FLOOR, v)
    return np.where(v < FLOOR, FLOOR, v)


def _quantities(mll, grad, mean, var, fant, y_std):
    """The compared quantities from (standardised, unfloored) ingredients, floors applied as the reference does."""
    f = _floored(fant) * y_std ** 2
    return {"mll": mll, "grad": grad, "mean": mean, "var": _floored(var), "fantasy": _floored(fant),
            "wipv": np.mean(f, axis=1), "wipstd": np.mean(np.sqrt(f), axis=1)}


def _err(a, truth, scale=None):
    a, truth = np.asarray(a, dtype=float), np.asarray(truth, dtype=float)
    s = np.max(np.abs(truth)) if scale is None else scale
    d = np.abs(a - truth)
    return float(np.max(np.where(np.isnan(d), np.inf, d)) / s)
