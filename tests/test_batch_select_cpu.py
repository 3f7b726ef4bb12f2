"""The algebra of the one-sweep batch selection (``bobe_gp_wip_select_batch``) on the CPU: the downdate recursion of
tests/batch_select_restatement.py against the literal kriging-believer loop, in which every member refactors the N+j points
(``OracleGP.update``: SciPy's Cholesky) and the scores are the oracle's fantasy variance.  No GPU is touched.

All candidates of a stage are scored with ``oracle.wip_sweep`` (the rank-one form of ``fantasy_var`` on the refactored
surrogate); the literal ``OracleGP.fantasy_var`` (gp.py:552-576, the (N+1)-row factor) is evaluated on top of it for every
stage's winner and runner-up and a few more candidates - O(N^2 M) per candidate, so not for all of them.

Tolerances: picks identical at every stage under the asserted precondition that the literal loop's best two unmasked scores
differ by more than 1e-6 relative; all-candidate scores within 1e-7 relative, the project's score tolerance (SURVEY section
8(d)).
"""
import os
import re

import numpy as np
import pytest

import batch_select_restatement as R
from oracle import bobe_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, N, d, C, M, b, noise, lengthscale, kernel variance): uniform-random X, candidates and integration points in the
# unit cube, RBF kernel
CASES = [
    (11, 300, 4, 2000, 128, 6, 1e-6, 0.4, 2.0),
    (12, 300, 4, 2000, 128, 6, 1e-8, 0.6, 10.0),
    (13, 700, 8, 4000, 256, 8, 1e-6, 0.8, 5.0),
    (14, 257, 5, 1500, 100, 5, 1e-8, 1.2, 50.0),
]
SCORE_RTOL = 1e-7
GAP_MIN = 1e-6


def make_case(case, kernel="rbf"):
    seed, n, d, c, m, b, noise, ell, kvar = case
    rng = np.random.default_rng(seed)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    ls = np.full(d, ell)
    og = O.OracleGP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar)
    return X, y, cand, Z, ls, og


@pytest.mark.parametrize("criterion", ["wipv", "wipstd"])
@pytest.mark.parametrize("case", CASES, ids=[f"N{c[1]}_d{c[2]}_C{c[3]}_b{c[5]}" for c in CASES])
def test_downdate_recursion_is_the_literal_believer_loop(case, criterion):
    X, y, cand, Z, ls, og = make_case(case)
    b, noise, kvar = case[5], case[6], case[8]
    power = 2 if criterion == "wipv" else 1
    rng = np.random.default_rng(case[0] + 100)
    checked = []

    def sweep(gp):
        r = O.wip_sweep(gp, cand, Z)
        sc = r[criterion]
        # the literal (N+1)-row fantasy variance on the best two and three random candidates of the stage
        k_train_mc = gp._k12(Z)
        for i in list(np.argsort(sc)[:2]) + list(rng.integers(0, cand.shape[0], size=3)):
            fv = gp.fantasy_var(cand[i], Z, k_train_mc)
            lit = np.mean(fv) if criterion == "wipv" else np.mean(np.sqrt(fv))
            assert abs(lit - sc[i]) <= SCORE_RTOL * abs(lit), (i, lit, sc[i])
            checked.append(i)
        return sc

    picks_l, stages_l, gaps = R.literal_loop(og, sweep, cand, b, power)
    assert len(checked) == 5 * b
    # the test's own precondition: an unambiguous winner at every stage, no index twice
    print("smallest relative gap between the best two scores of a stage: %.3e" % gaps.min())
    assert np.all(gaps > GAP_MIN), gaps
    assert len(set(picks_l.tolist())) == b
    picks_r, stages_r = R.select_batch("rbf", X, cand, Z, ls, kvar, noise, b, criterion)
    err = np.max(np.abs(stages_r - stages_l) / np.abs(stages_l), axis=1)
    print("largest relative score difference per stage:", " ".join("%.2e" % e for e in err))
    assert picks_r.tolist() == picks_l.tolist()                      # every stage, none excused
    assert np.all(err <= SCORE_RTOL), err


@pytest.mark.parametrize("criterion", ["wipv", "wipstd"])
def test_every_candidate_against_the_literal_fantasy_var(criterion):
    """A case small enough for the literal (N+1)-row ``OracleGP.fantasy_var`` (gp.py:552-576) on EVERY candidate of every
    stage: the loop refactors N+j points and scores with nothing but that function."""
    case = (17, 150, 3, 400, 48, 4, 1e-6, 0.5, 2.0)
    X, y, cand, Z, ls, og = make_case(case)

    def sweep(gp):
        k_train_mc = gp._k12(Z)
        fv = np.array([gp.fantasy_var(x, Z, k_train_mc) for x in cand])
        return np.mean(fv, axis=1) if criterion == "wipv" else np.mean(np.sqrt(fv), axis=1)

    picks_l, stages_l, gaps = R.literal_loop(og, sweep, cand, 4, 2 if criterion == "wipv" else 1)
    print("smallest relative gap: %.3e" % gaps.min())
    assert np.all(gaps > GAP_MIN), gaps
    assert len(set(picks_l.tolist())) == 4
    picks_r, stages_r = R.select_batch("rbf", X, cand, Z, ls, 2.0, 1e-6, 4, criterion)
    err = np.max(np.abs(stages_r - stages_l) / np.abs(stages_l), axis=1)
    print("largest relative score difference per stage:", " ".join("%.2e" % e for e in err))
    assert picks_r.tolist() == picks_l.tolist()
    assert np.all(err <= SCORE_RTOL), err


def test_matern_kernel_and_physical_units():
    """The recursion does not depend on the kernel; y_std scales WIPV by its square and WIPStd linearly."""
    case = (21, 200, 3, 600, 64, 4, 1e-6, 0.5, 3.0)
    X, y, cand, Z, ls, og = make_case(case, kernel="matern")
    picks_l, stages_l, gaps = R.literal_loop(og, lambda gp: O.wip_sweep(gp, cand, Z)["wipstd"], cand, 4, 1)
    assert np.all(gaps > GAP_MIN)
    picks_r, stages_r = R.select_batch("matern", X, cand, Z, ls, 3.0, 1e-6, 4, "wipstd")
    assert picks_r.tolist() == picks_l.tolist()
    assert np.max(np.abs(stages_r - stages_l) / np.abs(stages_l)) <= SCORE_RTOL
    _, s3 = R.select_batch("matern", X, cand, Z, ls, 3.0, 1e-6, 2, "wipstd", y_std=3.0)
    _, v3 = R.select_batch("matern", X, cand, Z, ls, 3.0, 1e-6, 2, "wipv", y_std=3.0)
    _, v1 = R.select_batch("matern", X, cand, Z, ls, 3.0, 1e-6, 2, "wipv")
    assert np.allclose(s3, 3.0 * stages_r[:2], rtol=1e-14) and np.allclose(v3, 9.0 * v1, rtol=1e-14)


def test_masking_and_tie_rule():
    v = np.array([3.0, 1.0, 2.0, 1.0, 5.0])
    assert R.masked_argmin(v) == 1                         # first occurrence of the minimum
    assert R.masked_argmin(v, [1]) == 3                    # a picked index never wins again ...
    assert R.masked_argmin(v, [1, 3]) == 2
    assert R.masked_argmin(np.array([1.0, 1.0, 1.0]), [0]) == 1
    assert R.masked_argmin(np.array([2.0, np.nan, 1.0, np.nan])) == 1          # NaN counts as minimal, first one
    assert R.masked_argmin(np.array([2.0, np.nan, 1.0, np.nan]), [1]) == 3
    # ... although its score is still computed: a pick's later-stage score is an ordinary entry of stage_scores
    case = (31, 60, 2, 40, 16, 3, 1e-6, 0.5, 1.0)
    X, y, cand, Z, ls, og = make_case(case)
    cand[7] = cand[3]                                       # an exact tie between two candidates at every stage
    picks, stages = R.select_batch("rbf", X, cand, Z, ls, 1.0, 1e-6, 3, "wipv")
    assert np.all(stages[:, 7] == stages[:, 3]) and np.all(np.isfinite(stages))
    assert 7 not in picks[:1]                               # (index 3 comes first)
    assert len(set(picks.tolist())) == 3
    for j in range(1, 3):                                   # the masked entries are the smallest of their stage or not: both occur
        assert R.masked_argmin(stages[j], picks[:j]) == picks[j]


def test_floor_and_nan_rules():
    kcz = np.array([[0.5, 0.2], [0.9, 0.1], [0.3, 0.3]])
    G = np.zeros((2, 3))
    base = np.array([0.25, 1e-13])
    s = np.array([1.0, -1.0, np.nan])
    wv, ws = R.score_state(kcz, G, base, s, y_std=2.0)
    # candidate 0: var+ = (0.25 - 0.25, 1e-13 - 0.04) -> both below the floor -> 1e-12 * y_std^2
    assert wv[0] == 4e-12 and ws[0] == 2e-6
    # s_c < 0 (sqrt of a negative number is NaN in the reference) and s_c NaN: every var+ sits at the floor
    assert wv[1] == 4e-12 and wv[2] == 4e-12 and ws[1] == 2e-6 and ws[2] == 2e-6
    wv, _ = R.score_state(kcz, G, np.array([0.5, 0.5]), np.array([1.0, 1.0, 1.0]), y_std=1.0)
    assert wv[0] == pytest.approx(((0.5 - 0.25) + (0.5 - 0.04)) / 2, rel=1e-15)


def test_symbol_is_declared_bound_and_exported():
    from bobe_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bobe_gp.h")).read()
    assert "y_std is the CALLER's at every stage" in txt            # the units rule is part of the contract
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+bobe_gp_wip_select_batch\s*\(", txt)
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert "bobe_gp_wip_select_batch" in sig and len(sig["bobe_gp_wip_select_batch"][1]) == 11
    assert os.path.exists(_lib.LIB_PATH), "libbobe_gp.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    assert hasattr(_lib.load(), "bobe_gp_wip_select_batch")


def test_python_surface_signatures():
    import inspect
    from bobe_amd import GP
    from bobe_amd.acquisition import AcquisitionFunction, WIPStd
    from bobe_amd.bo import BOBE
    from bobe_amd.clf_gp import GPwithClassifier
    p = inspect.signature(GP.wip_select_batch).parameters
    assert list(p) == ["self", "candidates", "mc_points", "n_batch", "criterion", "return_stage_scores"]
    assert p["criterion"].default == "wipstd" and p["return_stage_scores"].default is False
    assert GPwithClassifier.wip_select_batch is GP.wip_select_batch
    base = list(inspect.signature(AcquisitionFunction.get_next_batch).parameters)
    ours = inspect.signature(WIPStd.get_next_batch).parameters
    assert list(ours)[:len(base)] == base and list(ours)[len(base):] == ["batch_mode"]
    assert ours["batch_mode"].kind is inspect.Parameter.KEYWORD_ONLY and ours["batch_mode"].default == "believer"
    run = inspect.signature(BOBE.run).parameters
    assert list(run)[-1] == "wip_batch_mode" and run["wip_batch_mode"].default == "believer"
    assert run["wip_batch_mode"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError):
        WIPStd().get_next_batch(None, n_batch=2, batch_mode="other")
