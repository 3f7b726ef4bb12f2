"""The input gradients the samplers and the refinements consume - bobe_gp_predict_grad in both modes, the batched path of
bobe_gp_wip_grad (and its few-candidate chain beside it), bobe_gp_hmc_leapfrog - against the np.longdouble restatements of
tests/posterior_grad_restatement.py and tests/weighted_grad_restatement.py, at the launch shapes of
tests/posterior_grad_cases.py: more than one workgroup and a ragged last one, more than one chunk, training tiles with fewer
live rows than slices, the scalar tail of k_wip_grad's unrolled loop, d equal to a DCAP, the variance floor.

The rule is the one of tests/test_gpu_weighted_grad.py, per case and output array, over all of the
case's queries / candidates / chains and coordinates:

    max |device - truth| <= 4 max |fp64 restatement - truth| + 1e-8 max |truth|.

Every measured pair is printed before it is asserted; with BOBE_POSTERIOR_GRAD_PARITY_OUT=<file> the table is written there
(committed as profiles/posterior_grad_parity.txt).  tests/test_posterior_grad_cpu.py holds the fp64 restatement of every case
here within 1e-8 of the truth, so the ``4 x ref`` term cannot swallow an error above ~4e-8."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import posterior_grad_cases as PC  # noqa: E402
from test_gpu_weighted_criteria import make_gp, same_bits, standardise  # noqa: E402

pytestmark = pytest.mark.gpu

_ROWS = {}


def _record(case, rows):
    _ROWS[case] = rows
    out = os.environ.get("BOBE_POSTERIOR_GRAD_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        lines = ["# posterior input gradients (tests/test_gpu_posterior_grad.py): max |delta| / max |truth| over the case's queries / "
                 "candidates / chains and coordinates, against the np.longdouble truth",
                 "# dev = the device, ref = the fp64 restatement (SciPy cholesky / solve_triangular / cho_solve); "
                 "rule: dev <= 4 x ref + 1e-8", "",
                 f"{'case':<46}{'output':<9}{'refining':>9}{'dev':>11}{'ref':>11}{'max|truth|':>12}"]
        for nm, rs in _ROWS.items():
            for key, refining, dev, ref, scale in rs:
                lines.append(f"{nm:<46}{key:<9}{str(refining):>9}{dev:>11.2e}{ref:>11.2e}{scale:>12.3e}")
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    except OSError:
        pass


def _hold_to_the_rule(case, gp, triples):
    """triples: (output, device, fp64 restatement, truth).  Prints and records every pair, then asserts the rule."""
    rows = []
    for key, dev, f64, truth in triples:
        dev = np.asarray(dev)
        assert dev.shape == truth.shape and np.all(np.isfinite(dev)), key
        scale = float(np.max(np.abs(truth)))
        e_dev, e_ref = PC.rel_err(dev, truth), PC.rel_err(f64, truth)
        rows.append((key, bool(gp.refining), e_dev, e_ref, scale))
        print(f"[posterior grad parity] {case:<46} {key:<8} err(device) = {e_dev:.3e}   err(fp64 restatement) = {e_ref:.3e}   "
              f"max |truth| = {scale:.3e}   refining = {bool(gp.refining)}")
    _record(case, rows)
    for key, _, e_dev, e_ref, _ in rows:
        assert e_dev <= 4.0 * e_ref + 1e-8, (case, key, e_dev, e_ref)


def _make(kernel, X, y, d, noise, ell, kvar):
    gp = make_gp(X, y, d, noise, ell, kvar, kernel)
    y_std = standardise(y)[2]
    assert abs(gp.y_std - y_std) <= 1e-14 * y_std and not gp.not_pd
    return gp


class _Chunk:
    """bobe_gp_set_chunk for the body, the default again afterwards"""

    def __init__(self, gp, chunk):
        self.gp, self.chunk = gp, chunk

    def __enter__(self):
        if self.chunk:
            assert self.gp._lib.bobe_gp_set_chunk(self.gp._h, self.chunk) == 0

    def __exit__(self, *exc):
        if self.chunk:
            assert self.gp._lib.bobe_gp_set_chunk(self.gp._h, 0) == 0


# ------------------------------------------------------------------------------------------------------- a. predict_grad
@pytest.mark.parametrize("mean_only", [False, True], ids=["full", "mean_only"])
@pytest.mark.parametrize("case", PC.PREDICT_CASES, ids=[PC.predict_id(c) for c in PC.PREDICT_CASES])
def test_predict_grad_against_the_long_double_truth(case, mean_only):
    kernel, d, n, c, chunk = case
    X, y, Q = PC.predict_data(case)
    truth, f64 = PC.predict_reference(case)
    gp = _make(kernel, X, y, d, PC.NOISE, PC.ell_of(d), PC.KVAR)
    with _Chunk(gp, chunk):
        m, v, dm, dv = gp.predict_grad(Q, mean_only=mean_only)
        tail = gp.predict_grad(Q[128:], mean_only=mean_only) if chunk else None
    assert m.shape == (c,) and dm.shape == (c, d)
    triples = [("mean", m, f64[0], truth[0]), ("dmean", dm, f64[2], truth[2])]
    if mean_only:
        assert v is None and dv is None
    else:
        assert not truth[4].any() and np.all(v > 1e-12)
        triples += [("var", v, f64[1], truth[1]), ("dvar", dv, f64[3], truth[3])]
    _hold_to_the_rule(PC.predict_id(case) + ("_mean_only" if mean_only else "_full"), gp, triples)
    if chunk:
        # a query does not depend on its batch: the second launch's rows are those of the same queries sent alone, with the
        # chunk still set and with the default one
        alone = gp.predict_grad(Q[128:], mean_only=mean_only)
        for got, a, b in zip((m, v, dm, dv), tail, alone):
            if got is not None:
                assert same_bits(got[128:], a) and same_bits(got[128:], b)


# ------------------------------------------------------------------------------------------------------------ b. the floor
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_the_variance_floor_has_no_gradient(kernel):
    """Noise 1e-14: the query 1e-9 from a training point and the one ON a training point have var < 1e-12 - the floor, whose
    gradient is zero (k_predict_grad's ``floored``); the other seven see next to nothing of the data."""
    X, y, Q = PC.floor_data(kernel)
    truth, f64 = PC.floor_reference(kernel)
    assert truth[4].tolist() == f64[4].tolist() == [True, True] + [False] * 7
    gp = _make(kernel, X, y, PC.FLOOR_D, PC.FLOOR_NOISE, PC.FLOOR_ELL[kernel], PC.FLOOR_KVAR)
    m, v, dm, dv = gp.predict_grad(Q)
    print(f"{kernel}: device var rows 0, 1 = {v[0]!r}, {v[1]!r}; min elsewhere {np.min(v[2:]):.4f}")
    assert v[0] == 1e-12 and v[1] == 1e-12                                   # the precondition
    assert np.all(dv[:2] == 0.0) and np.any(dv[2:] != 0.0)
    m1, _, dm1, _ = gp.predict_grad(Q, mean_only=True)
    _hold_to_the_rule(f"floor_{kernel}", gp, [("mean", m, f64[0], truth[0]), ("dmean", dm, f64[2], truth[2]),
                                              ("var", v[2:], f64[1][2:], truth[1][2:]), ("dvar", dv[2:], f64[3][2:], truth[3][2:])])
    _hold_to_the_rule(f"floor_{kernel}_mean_only", gp, [("mean", m1, f64[0], truth[0]), ("dmean", dm1, f64[2], truth[2])])


# ------------------------------------------------------------------------------------------------ c. wip_grad, batched path
@pytest.mark.parametrize("case", PC.WIP_CASES, ids=[PC.wip_id(c) for c in PC.WIP_CASES])
def test_wip_grad_batched_and_few_against_the_long_double_truth(case):
    kernel, d, n, m, c, chunk = case
    X, y, cand, Z = PC.wip_data(case)
    truth, f64 = PC.wip_reference(case)
    gp = _make(kernel, X, y, d, PC.NOISE, PC.ell_of(d), PC.KVAR)
    assert c > 16                                                            # the batched path
    with _Chunk(gp, chunk):
        batched = gp.wip_grad(cand, Z)
        tail = gp.wip_grad(cand[128:], Z) if chunk else None
    few = gp.wip_grad(cand[:9], Z)                                           # the few-candidate chain, on its own
    _hold_to_the_rule(PC.wip_id(case) + "_batched", gp, [(k, batched[i], f64[k], truth[k]) for i, k in enumerate(PC.WIP_KEYS)])
    _hold_to_the_rule(PC.wip_id(case) + "_few9", gp, [(k, few[i], f64[k][:9], truth[k][:9]) for i, k in enumerate(PC.WIP_KEYS)])
    if chunk:
        assert c - 128 > 16
        alone = gp.wip_grad(cand[128:], Z)
        for got, a, b in zip(batched, tail, alone):
            assert same_bits(got[128:], a) and same_bits(got[128:], b)


# ----------------------------------------------------------------------------------------------------------- d. the leapfrog
@pytest.mark.parametrize("L", PC.HMC_STEPS)
@pytest.mark.parametrize("case", PC.HMC_CASES, ids=[f"{k}_d{d}_N{n}" for k, d, n in PC.HMC_CASES])
def test_hmc_leapfrog_against_the_long_double_truth(case, L):
    """The ref term is the fp64 trajectory's: L steps amplify an error, and the fp64 recurrence sets that scale."""
    kernel, d, n = case
    X, y, U, Pm, im = PC.hmc_data(case)
    truth, f64 = PC.hmc_reference(case, L)
    gp = _make(kernel, X, y, d, PC.NOISE, PC.ell_of(d), PC.KVAR)
    U0, Pm0 = U.copy(), Pm.copy()
    got = gp.hmc_leapfrog(U, Pm, im, PC.HMC_EPS, L, PC.HMC_TEMP)
    assert np.array_equal(U, U0) and np.array_equal(Pm, Pm0)                 # the wrapper works on copies
    _hold_to_the_rule(PC.hmc_id(case, L), gp, [(k, got[i], f64[k], truth[k]) for i, k in enumerate(PC.HMC_KEYS)])
