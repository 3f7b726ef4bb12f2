"""The cases of tests/test_gpu_ei_grad.py with their references (the 50-digit truth on the long-double posterior and the fp64
restatement on the fp64 posterior), each computed once; tests/test_ei_grad_cpu.py holds the fp64 restatement of the same
cases to the truth.  Imports nothing from bobe_amd.

The posteriors are those of tests/posterior_grad_cases.py (``predict_data`` / ``predict_reference``, ``floor_data`` /
``floor_reference``): the smallest shapes that reach each hazard of the call."""
import functools

import numpy as np

import ei_grad_restatement as ER
import posterior_grad_cases as PC
from test_gpu_weighted_criteria import standardise

# (kernel, d, N, C, chunk) of posterior_grad_cases.PREDICT_CASES, or ("floor", kernel)
CASES = [
    ("matern", 5, 300, 65, 0),     # two query workgroups, the second with one live query
    ("rbf", 8, 129, 64, 0),        # d = DCAP 8
    ("matern", 16, 160, 1, 0),     # C = 1
    ("rbf", 32, 160, 9, 0),        # d = DCAP 32
    ("matern", 2, 3, 5, 0),        # N = 3
    ("matern", 5, 300, 200, 128),  # two chunks of 128 + 72 queries
    ("rbf", 3, 160, 9, 0),         # the ill-conditioned family (variances ~1e-5 of the kernel variance): u from -4500 to +1000
    ("floor", "rbf"),              # rows 0, 1 on the 1e-12 variance floor: their gradient is Phi(u) dm alone
    ("floor", "matern"),
]
PAIRS = ("best", "best_plus3_zeta", "median")      # (best_y, zeta) = (max ys, 0) | (max ys + 3, 0.01) | (median ys, 0)
MODES = (False, True)                              # log_ei


def is_floor(case):
    return case[0] == "floor"


def case_id(case):
    return f"floor_{case[1]}" if is_floor(case) else PC.predict_id(case)


def data(case):
    """(kernel, d, X, y, Q, noise, lengthscale, kernel variance, chunk)"""
    if is_floor(case):
        X, y, Q = PC.floor_data(case[1])
        return case[1], PC.FLOOR_D, X, y, Q, PC.FLOOR_NOISE, PC.FLOOR_ELL[case[1]], PC.FLOOR_KVAR, 0
    kernel, d, _, _, chunk = case
    X, y, Q = PC.predict_data(case)
    return kernel, d, X, y, Q, PC.NOISE, PC.ell_of(d), PC.KVAR, chunk


def posterior(case):
    """((m, v, dm, dv, floored) of the long-double truth, the same in fp64)"""
    return PC.floor_reference(case[1]) if is_floor(case) else PC.predict_reference(case)


def best_and_zeta(case, pair):
    ys = standardise(data(case)[3])[0]
    return {"best": (float(np.max(ys)), 0.0), "best_plus3_zeta": (float(np.max(ys)) + 3.0, 0.01),
            "median": (float(np.median(ys)), 0.0)}[pair]


@functools.lru_cache(maxsize=None)
def reference(case, pair, log_ei):
    """{"truth": (val, grad, u) as long doubles, "f64": (val, grad, u)}"""
    truth, f64 = posterior(case)
    best_y, zeta = best_and_zeta(case, pair)
    return {"truth": ER.value_and_grad_truth(*truth, best_y, zeta, log_ei),
            "f64": ER.value_and_grad_f64(*f64, best_y, zeta, log_ei)}


ILL = ("rbf", 3, 160, 9, 0)


def listed(case, pair, log_ei):
    """Every case x pair x mode, but for plain EI on the ill-conditioned case with the two pairs at and above max ys: every
    u < -38 there, EI and its gradient underflow (the truth is 0 throughout); those pairs are LogEI's alone
    (tests/test_ei_grad_cpu.py holds the reason to the truth's own u).  The floor designs put a floored row (sigma = 1e-6)
    at u ~ -1e6 and -4e6 with those two pairs and at +1e6 with the median one: the lower branch of the LogEI gradient on
    both sides of log_ei_helper's -1e6, with dsigma = 0."""
    if case == ILL and not log_ei:
        return pair == "median"
    return True


COMBOS = [(c, p, m) for c in CASES for p in PAIRS for m in MODES if listed(c, p, m)]


def combo_id(combo):
    case, pair, log_ei = combo
    return f"{case_id(case)}-{pair}-{'logei' if log_ei else 'ei'}"


def rel_err(a, truth):
    return PC.rel_err(a, truth)
