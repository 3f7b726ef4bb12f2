"""One-sweep batch selection for WIPV / WIPStd on the device (bobe_gp_wip_select_batch, GP.wip_select_batch,
get_next_batch(batch_mode="sweep"), BOBE.run(wip_batch_mode="sweep")): stage 0 against bobe_gp_wip_sweep bit for bit, every
stage against the existing believer machinery on the device (copy, update at the predicted mean, wip_sweep), the refine
switch, determinism, the Python surface and the refusals.

Tolerances: identical picks at every stage under the asserted precondition that the literal loop's best two unmasked
scores differ by more than 1e-6 relative; all-candidate scores within 1e-7 relative (the project's score tolerance, SURVEY
section 8(d)), both sides in standardised units (divided by their own y_std power)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_select_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_STATE = -1, -3
SCORE_RTOL = 1e-7
GAP_MIN = 1e-6
KEYS = ("wipv", "wipstd")

# (seed, N, d, C, M, b, noise, lengthscale, kernel variance): tests/test_batch_select_cpu.py's cases and one with N > 1024
# and C > 8192 (more than one chunk of the default width)
CASES = [
    (11, 300, 4, 2000, 128, 6, 1e-6, 0.4, 2.0),
    (12, 300, 4, 2000, 128, 6, 1e-8, 0.6, 10.0),
    (13, 700, 8, 4000, 256, 8, 1e-6, 0.8, 5.0),
    (14, 257, 5, 1500, 100, 5, 1e-8, 1.2, 50.0),
    (15, 1100, 6, 9000, 200, 4, 1e-6, 0.7, 3.0),
]


def case_arrays(case):
    """(X, y, cand, Z) of a case."""
    seed, n, d, c, m = case[:5]
    rng = np.random.default_rng(seed)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    return X, y, cand, Z


def make_case(case, kernel="rbf"):
    from bobe_amd import GP
    seed, n, d, c, m, b, noise, ell, kvar = case
    X, y, cand, Z = case_arrays(case)
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=np.full(d, ell), kernel_variance=kvar)
    return gp, cand, Z


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def raw_call(gp, cand, Z, n_batch, criterion, picks, pick_scores, stage_scores, c=None):
    from bobe_amd import _lib
    return gp._lib.bobe_gp_wip_select_batch(gp._h, _lib.ptr(cand), int(cand.shape[0]) if c is None else c, _lib.ptr(Z),
                                            int(Z.shape[0]), float(gp.y_std), n_batch, criterion, _lib.ptr(picks),
                                            _lib.ptr(pick_scores), _lib.ptr(stage_scores))


# ---------------------------------------------------------------------------------------------------- 1. bitwise stage 0
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
@pytest.mark.parametrize("n,d,c,m,chunk", [(333, 5, 1001, 100, 256), (130, 3, 300, 77, 0), (1030, 6, 9100, 200, 0),
                                           (150, 4, 70001, 64, 0)],
                         ids=["ragged_4chunks", "one_chunk", "two_default_chunks", "two_super_chunks"])
def test_stage0_is_wip_sweep_bit_for_bit(kernel, n, d, c, m, chunk):
    import torch
    from bobe_amd import GP
    rng = np.random.default_rng(n + c)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.5 * X[:, -1]
    gp = GP(X, y, noise=1e-6, kernel=kernel, lengthscales=np.full(d, 0.45), kernel_variance=1.4)
    if chunk:
        assert gp._lib.bobe_gp_set_chunk(gp._h, chunk) == 0
    sw = gp.wip_sweep(cand, Z)
    for key in KEYS:
        r = gp.wip_select_batch(cand, Z, 1, criterion=key, return_stage_scores=True)
        assert r["stage_scores"].shape == (1, c) and r["points"].shape == (1, d)
        assert same_bits(r["stage_scores"][0], sw[key])
        assert r["indices"][0] == sw["argmin_" + key[3]] and same_bits(r["scores"][0], sw["min_" + key[3]])
        assert np.array_equal(r["points"][0], cand[r["indices"][0]])
        # a longer batch starts with the same stage
        r3 = gp.wip_select_batch(cand, Z, 3, criterion=key, return_stage_scores=True)
        assert same_bits(r3["stage_scores"][0], sw[key]) and r3["indices"][0] == r["indices"][0]
    # device pointers for the inputs and for every output
    dc, dz = torch.as_tensor(cand, device="cuda"), torch.as_tensor(Z, device="cuda")
    swd = gp.wip_sweep(dc, dz)
    assert same_bits(swd["wipstd"], sw["wipstd"])
    picks = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    vals = torch.zeros(2, dtype=torch.float64, device="cuda")
    stage = torch.zeros((2, c), dtype=torch.float64, device="cuda")
    assert raw_call(gp, dc, dz, 2, 1, picks, vals, stage) == 0
    torch.cuda.synchronize()
    assert same_bits(stage[0].cpu().numpy(), sw["wipstd"])
    assert int(picks[0]) == sw["argmin_s"] and same_bits(vals[:1].cpu().numpy(), [sw["min_s"]])
    rh = gp.wip_select_batch(cand, Z, 2, criterion="wipstd", return_stage_scores=True)
    assert same_bits(stage.cpu().numpy(), rh["stage_scores"]) and picks.cpu().tolist() == rh["indices"].tolist()
    rd = gp.wip_select_batch(dc, dz, 2, criterion="wipstd")
    assert np.array_equal(rd["points"], cand[rh["indices"]]) and same_bits(rd["scores"], rh["scores"])
    if chunk:
        assert gp._lib.bobe_gp_set_chunk(gp._h, 0) == 0


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_stage0_candidates_are_the_integration_points(kernel):
    """``candidates is mc_points``: the sweep forms no V of its own then (V_C = V_Z)."""
    gp, _, Z = make_case((41, 400, 4, 10, 128, 4, 1e-6, 0.5, 2.0), kernel)
    sw = gp.wip_sweep(Z, Z)
    for key in KEYS:
        r = gp.wip_select_batch(Z, Z, 4, criterion=key, return_stage_scores=True)
        assert same_bits(r["stage_scores"][0], sw[key]) and r["indices"][0] == sw["argmin_" + key[3]]
        assert same_bits(r["scores"][0], sw["min_" + key[3]])
        _compare(r, _literal(gp, Z, Z, 4, key), gp.y_std ** (2 if key == "wipv" else 1))
        # two separate device copies of the same points take the general path (V formed for the candidates): same batch
        import torch
        r2 = gp.wip_select_batch(torch.as_tensor(Z, device="cuda"), torch.as_tensor(Z, device="cuda").clone(), 4,
                                 criterion=key, return_stage_scores=True)
        assert r2["indices"].tolist() == r["indices"].tolist()
        assert np.max(np.abs(r2["stage_scores"] - r["stage_scores"]) / np.abs(r["stage_scores"])) <= SCORE_RTOL


# ---------------------------------------------------------------------------------------------------- 2. literal loop
def _literal(gp, cand, Z, b, key):
    """The existing believer machinery on the device: copy, update at the predicted mean, wip_sweep."""
    return R.literal_loop(gp.copy(), lambda g: g.wip_sweep(cand, Z)[key], cand, b, 2 if key == "wipv" else 1)


def _compare(r, lit, y_std_power=None):
    picks_l, stages_l, gaps = lit
    print("smallest relative gap of the literal loop's best two: %.3e" % gaps.min())
    assert np.all(gaps > GAP_MIN), gaps                     # the precondition: an unambiguous winner at every stage
    assert len(set(picks_l.tolist())) == len(picks_l)
    stages = r["stage_scores"] if y_std_power is None else r["stage_scores"] / y_std_power
    err = np.max(np.abs(stages - stages_l) / np.abs(stages_l), axis=1)
    print("largest relative score difference per stage:", " ".join("%.2e" % e for e in err))
    assert r["indices"].tolist() == picks_l.tolist()        # every stage
    assert np.all(err <= SCORE_RTOL), err


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
@pytest.mark.parametrize("case", CASES, ids=[f"N{c[1]}_d{c[2]}_C{c[3]}_b{c[5]}" for c in CASES])
def test_later_stages_are_the_literal_believer_loop(case, kernel, key):
    gp, cand, Z = make_case(case, kernel)
    b = case[5]
    r = gp.wip_select_batch(cand, Z, b, criterion=key, return_stage_scores=True)
    p = 2 if key == "wipv" else 1
    _compare(r, _literal(gp, cand, Z, b, key), gp.y_std ** p)
    # pick_scores: every stage's winning score; a picked index keeps a computed (finite) score in the later stages
    st = r["stage_scores"]
    assert same_bits(r["scores"], [st[j, r["indices"][j]] for j in range(b)])
    assert np.all(np.isfinite(st))
    # ... and against the fp64 restatement of the recursion
    pr, sr = R.select_batch(kernel, gp.train_x, cand, Z, gp.lengthscales, gp.kernel_variance, gp.noise, b, key)
    assert pr.tolist() == r["indices"].tolist()
    assert np.max(np.abs(st / gp.y_std ** p - sr) / np.abs(sr)) <= SCORE_RTOL


# ---------------------------------------------------------------------------------------------------- 3. refine switch
@pytest.mark.parametrize("key", KEYS)
def test_forced_substitution_gives_the_same_batch(key):
    case = CASES[2]
    plain, cand, Z = make_case(case)
    forced, _, _ = make_case(case)
    plain.refine_kappa = -1.0
    plain.recompute_cholesky()
    forced.refine_kappa = 0.0
    forced.recompute_cholesky()
    assert forced.refining and not plain.refining
    a = plain.wip_select_batch(cand, Z, case[5], criterion=key, return_stage_scores=True)
    b = forced.wip_select_batch(cand, Z, case[5], criterion=key, return_stage_scores=True)
    assert same_bits(b["stage_scores"][0], forced.wip_sweep(cand, Z)[key])          # stage 0: that path's own sweep
    err = np.max(np.abs(a["stage_scores"] - b["stage_scores"]) / np.abs(a["stage_scores"]))
    print("substitution against plain product: %.2e" % err)
    assert a["indices"].tolist() == b["indices"].tolist()
    assert err <= SCORE_RTOL


# ---------------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("key", KEYS)
def test_same_state_same_bits_and_the_handle_is_left_alone(key):
    gp, cand, Z = make_case(CASES[0])
    lib = gp._lib
    source = lib.bobe_debug_factor_source(gp._h)
    before = gp.wip_sweep(cand, Z, want_mean_var=True)
    chol, alphas = np.array(gp.cholesky), np.array(gp.alphas)
    a = gp.wip_select_batch(cand, Z, 6, criterion=key, return_stage_scores=True)
    b = gp.wip_select_batch(cand, Z, 6, criterion=key, return_stage_scores=True)
    assert a["indices"].tolist() == b["indices"].tolist() and same_bits(a["scores"], b["scores"])
    assert same_bits(a["stage_scores"], b["stage_scores"])
    short = gp.wip_select_batch(cand, Z, 3, criterion=key, return_stage_scores=True)       # a prefix of the longer batch
    assert short["indices"].tolist() == a["indices"][:3].tolist() and same_bits(short["stage_scores"], a["stage_scores"][:3])
    after = gp.wip_sweep(cand, Z, want_mean_var=True)
    for k in ("wipv", "wipstd", "mean", "var"):
        assert same_bits(before[k], after[k]), k
    assert (before["argmin_v"], before["argmin_s"]) == (after["argmin_v"], after["argmin_s"])
    gp._chol_cache = gp._alpha_cache = None
    assert same_bits(gp.cholesky, chol) and same_bits(gp.alphas, alphas)
    assert lib.bobe_debug_factor_source(gp._h) == source
    assert gp.npoints == CASES[0][1]


# ---------------------------------------------------------------------------------------------------- 5. Python surface
@pytest.mark.parametrize("acq_name", ["WIPV", "WIPStd"])
def test_get_next_batch_sweep_mode(acq_name):
    from bobe_amd import acquisition as A
    gp, cand, _ = make_case((51, 120, 3, 800, 64, 4, 1e-6, 0.5, 2.0))
    acq = getattr(A, acq_name)()
    pool = np.random.default_rng(8).uniform(size=(700, 3))
    kw = {"mc_samples": {"x": pool}, "mc_points_size": 48}
    xb, vals = acq.get_next_batch(gp, n_batch=4, acq_kwargs=kw, rng=np.random.default_rng(5), batch_mode="sweep")
    assert xb.shape == (4, 3) and vals.shape == (4,) and np.all(np.isfinite(vals))
    rows = [int(np.flatnonzero(np.all(pool == x, axis=1))[0]) for x in xb]             # rows of the pool ...
    assert len(set(rows)) == 4                                                            # ... all different
    Z = A.get_mc_points(kw["mc_samples"], mc_points_size=48, rng=np.random.default_rng(5))    # ONE draw of integration points
    r = gp.wip_select_batch(pool, Z, 4, criterion=acq._key)
    assert rows == r["indices"].tolist() and same_bits(vals, r["scores"])
    xc, vc = acq.get_next_batch(gp, n_batch=3, acq_kwargs=dict(kw, candidates=cand), rng=np.random.default_rng(5),
                                batch_mode="sweep")
    assert xc.shape == (3, 3) and all(np.any(np.all(cand == x, axis=1)) for x in xc)
    with pytest.raises(ValueError):
        acq.get_next_batch(gp, n_batch=2, acq_kwargs=kw, batch_mode="greedy")
    # the default mode is the base class's loop, bit for bit, and draws the same numbers from the generator
    g1, g2 = np.random.default_rng(9), np.random.default_rng(9)
    x1, v1 = acq.get_next_batch(gp, n_batch=3, acq_kwargs=kw, maxiter=20, n_restarts=1, verbose=False, rng=g1)
    x2, v2 = A.AcquisitionFunction.get_next_batch(acq, gp, n_batch=3, acq_kwargs=kw, maxiter=20, n_restarts=1, verbose=False, rng=g2)
    assert same_bits(x1, x2) and same_bits(v1, v2) and g1.random() == g2.random()


def test_gp_with_classifier_inherits_the_method():
    from bobe_amd.clf_gp import GPwithClassifier
    from bobe_amd import GP
    assert GPwithClassifier.wip_select_batch is GP.wip_select_batch


def test_bo_run_with_the_sweep_batch_mode():
    from bobe_amd.bo import BOBE

    def himmelblau(x):
        return -((x[0] ** 2 + x[1] - 11) ** 2 + (x[0] + x[1] ** 2 - 7) ** 2) / 10.0
    bounds = np.array([[-4.0, 4.0], [-4.0, 4.0]]).T
    kw = dict(acq="wipstd", max_evals=28, fit_n_points=2, batch_size=4, mc_points_size=64, num_mc_samples=256,
              mc_points_method="uniform")
    bobe = BOBE(himmelblau, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False)
    res = bobe.run(wip_batch_mode="sweep", **kw)
    assert 8 < res["gp"].npoints <= 28 and res["n_evals"] == res["gp"].npoints
    assert len(res["acq_history"]) == 5 and all(np.isfinite(res["acq_history"]))
    with pytest.raises(ValueError):
        BOBE(himmelblau, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(wip_batch_mode="other", **kw)


# ---------------------------------------------------------------------------------------------------- 6. refusals
@pytest.fixture(scope="module")
def small():
    gp, cand, Z = make_case((61, 64, 3, 40, 16, 2, 1e-6, 0.5, 1.0))
    return gp, cand, Z


def _refused(gp, cand, Z, code, n_batch=2, criterion=1, picks="own", c=None):
    from bobe_amd import _lib
    pk = np.full(max(n_batch, 1), -7, dtype=np.int64) if isinstance(picks, str) else picks
    st = raw_call(gp, cand, Z, n_batch, criterion, pk, None, None, c=c)
    assert st == code, (st, _lib.last_error())
    assert _lib.last_error()
    if pk is not None:
        assert np.all(pk == -7)                             # nothing was written
    r = gp.wip_select_batch(cand, Z, 2)                     # the handle still works
    assert len(set(r["indices"].tolist())) == 2


@pytest.mark.parametrize("n_batch", [0, -1, 65, 41])
def test_refuses_a_batch_size_out_of_range(small, n_batch):
    gp, cand, Z = small                                     # (41: more picks than the 40 candidates)
    _refused(gp, cand, Z, BOBE_ERR_ARG, n_batch=n_batch)


def test_accepts_the_largest_batch(small):
    gp, cand, Z = small
    r = gp.wip_select_batch(cand, Z, 40, criterion="wipv")                     # min(C, 64) = C: every candidate, once
    assert sorted(r["indices"].tolist()) == list(range(40))
    case = (62, 64, 3, 100, 16, 2, 1e-6, 0.5, 1.0)
    gp2, cand2, Z2 = make_case(case)
    r = gp2.wip_select_batch(cand2, Z2, 64, return_stage_scores=True)
    assert len(set(r["indices"].tolist())) == 64
    # all 63 downdates against the literal refit of the (N + j)-point believer surrogate in long double, under the rule of
    # tests/test_gpu_batch_terms.py: the truth's pick at every stage (its two best more than GAP_MIN apart: asserted) and
    # |device - truth| <= 4 |float64 literal refit - truth| + 1e-7 |truth| for every candidate
    import batch_terms_restatement as BT
    X, y, _, _ = case_arrays(case)
    d = case[2]
    ys, std = (y - np.mean(y)) / np.std(y), float(np.std(y))
    assert abs(gp2.y_std / std - 1) < 1e-12
    args = ("rbf", X, ys, cand2, Z2, np.full(d, case[7]), case[8], case[6], std, None, 64, "wipstd")
    picks, truth, gaps, _ = BT.append_batch(*args)
    f64 = BT.literal_batch(*args, dtype=np.float64, follow=picks)[1]
    assert np.all(gaps > GAP_MIN), gaps.min()
    assert r["indices"].tolist() == picks.tolist()
    worst = 0.0
    for j in range(64):
        ok, err, ref_err = BT.rule(r["stage_scores"][j], f64[j], truth[j], "wipstd")
        worst = max(worst, err)
        assert ok, (j, err, ref_err)
    print("\nthe largest batch: worst relative error of a stage score against the long-double literal refit %.2e, smallest gap "
          "%.2e" % (worst, gaps.min()))


@pytest.mark.parametrize("criterion", [-1, 2])
def test_refuses_an_unknown_criterion(small, criterion):
    gp, cand, Z = small
    _refused(gp, cand, Z, BOBE_ERR_ARG, criterion=criterion)
    with pytest.raises(ValueError):
        gp.wip_select_batch(cand, Z, 2, criterion="ei")


def test_refuses_null_picks(small):
    gp, cand, Z = small
    _refused(gp, cand, Z, BOBE_ERR_ARG, picks=None)


def test_refuses_a_pool_above_the_cap(small):
    """The buffers that grow with C above 16 GiB: refused before anything is allocated or read; 262 144 candidates at
    N = 4096 are within the cap whatever the batch (the arithmetic of the documented rule: V, crossT, coordinates, s_c,
    partial sums, u rows, staged score rows)."""
    gp, cand, Z = small
    _refused(gp, cand, Z, BOBE_ERR_ARG, c=10_000_000)       # (128 + 128 + 4 + 1 + 1) x 1e7 x 8 bytes = 21 GB
    assert ((4096 + 512 + 32 + 1) + (32 + 63) + 64) * 262144 * 8 <= 16 * 2 ** 30
    # just inside and just outside the documented figure for N = 4096, M = 512, d = 8, n_batch = 64, host stage scores
    per_candidate = (4096 + 512 + 8 + 1) + (32 + 63) + 64
    assert per_candidate * 449536 <= 2 ** 31 < per_candidate * (449536 + 128)


def test_a_nan_state_behaves_as_in_wip_sweep():
    """A factor that is not positive definite (duplicate rows, no noise to speak of, the rank test on): BOBE_OK like
    bobe_gp_wip_sweep, stage 0 its bits, and the masked argmin's rules on the device - every score equal (or NaN: NaN counts
    as minimal), so the picks are the first indices not taken yet."""
    from bobe_amd import GP
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(40, 3))
    X[7] = X[3]
    cand, Z = rng.uniform(size=(300, 3)), rng.uniform(size=(32, 3))
    gp = GP(X, np.sin(X[:, 0]), noise=1e-30, lengthscales=np.full(3, 0.5), kernel_variance=1.0, pivot_floor_ulp=64)
    assert gp.not_pd                                         # the test's precondition
    sw = gp.wip_sweep(cand, Z)
    for key, crit in (("wipv", 0), ("wipstd", 1)):
        picks, vals, stage = np.full(4, -7, dtype=np.int64), np.zeros(4), np.zeros((4, 300))
        assert raw_call(gp, cand, Z, 4, crit, picks, vals, stage) == 0
        assert same_bits(stage[0], sw[key]) and picks[0] == sw["argmin_" + key[3]] and same_bits(vals[:1], [sw["min_" + key[3]]])
        for j in range(4):
            assert picks[j] == R.masked_argmin(stage[j], picks[:j])
            assert same_bits(vals[j], stage[j, picks[j]])
        assert len(set(picks.tolist())) == 4


def test_refuses_a_handle_without_a_factor():
    from bobe_amd import GP, _lib
    rng = np.random.default_rng(3)
    X, cand, Z = rng.uniform(size=(30, 2)), rng.uniform(size=(20, 2)), rng.uniform(size=(8, 2))
    gp = GP(X, X[:, 0], noise=1e-6, lengthscales=np.full(2, 0.5), kernel_variance=1.0, _factor=False)
    pk = np.full(2, -7, dtype=np.int64)
    assert raw_call(gp, cand, Z, 2, 1, pk, None, None) == BOBE_ERR_STATE and np.all(pk == -7)
    assert "bobe_gp_factor" in _lib.last_error()
