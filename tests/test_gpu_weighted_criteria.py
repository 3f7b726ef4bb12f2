"""Importance-weighted integration points and the IMIQR / EIV criteria on the device (bobe_gp_wip_sweep_w,
bobe_gp_wip_select_batch_w, GP.wip_sweep(log_weights=, criteria=), GP.wip_select_batch_w(log_weights=), acquisition.IMIQR / EIV,
BOBE.run(acq='imiqr', mc_weighted=True)) against the dense SciPy restatement (tests/weighted_criteria_restatement.py).

Tolerances: wipv / wipstd 1e-7 relative (the project's score tolerance); imiqr / eiv / log S
|delta| <= 1e-7 (1 + |ref|); identical argmin / picks under the ASSERTED precondition that the restatement's two best scores
differ by more than 1e-6 (absolute for the log scores, relative for the others): a hundred times the library's agreement
with the restatement at least ten times over."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import weighted_criteria_restatement as W  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_STATE = -1, -3
SCORE_RTOL = 1e-7
GAP_MIN = 1e-6
KEYS = W.KEYS

# name: (seed, N, d, C, M, chunk, noise, lengthscale, kernel variance)
SWEEP_CASES = {
    "tile_edge": (103, 130, 3, 300, 77, 0, 1e-6, 0.4, 2.0),        # N crosses a 128-row tile, M no multiple of the 4 x 8 z-loop
    "ragged_4chunks": (100, 333, 5, 1001, 100, 256, 1e-6, 0.4, 2.0),
    "second_z_tile_of_one": (100, 150, 4, 640, 129, 0, 1e-8, 0.6, 10.0),
    "below_the_unroll": (138, 64, 2, 40, 5, 0, 1e-6, 0.4, 2.0),
}
# (seed, N, d, C, M, b, noise, lengthscale, kernel variance)
BATCH_CASES = {"n300": (201, 300, 4, 2000, 128, 6, 1e-6, 0.4, 2.0), "n257": (304, 257, 5, 1500, 100, 5, 1e-6, 0.6, 2.0)}
SCALE_SEED = 103


def case_data(seed, n, d, c, m, y_scale=1.0):
    """tests/test_gpu_batch_select.py::make_case's data, then the log-weights 1.5 N(0, 1)."""
    rng = np.random.default_rng(seed)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    return X, y * y_scale, cand, Z, 1.5 * rng.normal(size=m)


def standardise(y):
    mean, std = float(np.mean(y)), float(np.std(y))
    return (y - mean) / std, mean, std


@functools.lru_cache(maxsize=None)
def sweep_reference(name, kernel, weighted, y_scale=1.0, seed=None):
    """The restatement's physical scores of a sweep case (y_mean applied as GP.wip_sweep applies it), computed once."""
    sd, n, d, c, m, _, noise, ell, kvar = SWEEP_CASES[name]
    X, y, cand, Z, lw = case_data(sd if seed is None else seed, n, d, c, m, y_scale)
    ys, y_mean, y_std = standardise(y)
    st = W.dense_state(kernel, X, ys, cand, Z, np.full(d, ell), kvar, noise)
    ref = W.weighted_scores(st, y_std, lw if weighted else None)
    ref["imiqr"] = ref["imiqr"] + y_mean
    ref["eiv"] = ref["eiv"] - 2.0 * y_mean
    ref["log_s"] = ref["log_s"] + 2.0 * y_mean
    return ref


@functools.lru_cache(maxsize=None)
def batch_reference(name, key, kernel="rbf"):
    sd, n, d, c, m, b, noise, ell, kvar = BATCH_CASES[name]
    X, y, cand, Z, lw = case_data(sd, n, d, c, m)
    ys, y_mean, y_std = standardise(y)
    picks, stages, gaps = W.literal_batch(kernel, X, ys, cand, Z, np.full(d, ell), kvar, noise, y_std, lw, b, key)
    return picks, stages + {"imiqr": y_mean, "eiv": -2.0 * y_mean}.get(key, 0.0), gaps


def make_gp(X, y, d, noise, ell, kvar, kernel):
    from bobe_amd import GP
    return GP(X, y, noise=noise, kernel=kernel, lengthscales=np.full(d, ell), kernel_variance=kvar)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def score_error(key, got, ref):
    """The figure the tolerance bounds: relative for wipv / wipstd, |delta| / (1 + |ref|) for the log scores."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if key in ("wipv", "wipstd"):
        return float(np.max(np.abs(got - ref) / np.abs(ref)))
    return float(np.max(np.abs(got - ref) / (1.0 + np.abs(ref))))


def gap(key, scores, taken=()):
    g = W.two_best_gap(scores, taken)
    if key in ("wipv", "wipstd"):
        v = np.array(scores, dtype=np.float64)
        v[list(taken)] = np.inf
        return g / abs(np.min(v))
    return g


def check_sweep(r, ref, keys=KEYS):
    for key in keys:
        assert np.all(np.isfinite(r[key])), key
        err = score_error(key, r[key], ref[key])
        g = gap(key, ref[key])
        print("%-6s error %.3e, the restatement's gap %.3e" % (key, err, g))
        assert err <= SCORE_RTOL, (key, err)
        assert g > GAP_MIN, (key, g)                           # the precondition of asserting the pick
        assert r["argmin_" + key] == W.masked_argmin(ref[key]), key
        assert same_bits(r["min_" + key], r[key][r["argmin_" + key]])
    err = abs(r["log_eiv_total"] - ref["log_s"]) / (1.0 + abs(ref["log_s"]))
    print("log S  error %.3e" % err)
    assert np.isfinite(r["log_eiv_total"]) and err <= SCORE_RTOL


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
@pytest.mark.parametrize("weighted", [False, True], ids=["posterior_draws", "weights"])
@pytest.mark.parametrize("name", list(SWEEP_CASES))
def test_sweep_matches_the_restatement(name, weighted, kernel):
    sd, n, d, c, m, chunk, noise, ell, kvar = SWEEP_CASES[name]
    X, y, cand, Z, lw = case_data(sd, n, d, c, m)
    gp = make_gp(X, y, d, noise, ell, kvar, kernel)
    if chunk:
        assert gp._lib.bobe_gp_set_chunk(gp._h, chunk) == 0
    r = gp.wip_sweep(cand, Z, log_weights=lw if weighted else None, criteria=KEYS)
    check_sweep(r, sweep_reference(name, kernel, weighted))


# ---------------------------------------------------------------------------------------------------- 2. scale
@pytest.mark.parametrize("weighted", [False, True], ids=["posterior_draws", "weights"])
def test_targets_scaled_by_1e4(weighted):
    """y_std about 4.3e3: v+ up to 1e7, exponents up to 1e5 - only a log-sum-exp with a per-candidate maximum stays finite,
    and 1 - exp(-v+) would tie every candidate."""
    sd, n, d, c, m, _, noise, ell, kvar = SWEEP_CASES["tile_edge"]
    X, y, cand, Z, lw = case_data(SCALE_SEED, n, d, c, m, 1e4)
    gp = make_gp(X, y, d, noise, ell, kvar, "rbf")
    assert 3e3 < gp.y_std < 6e3
    r = gp.wip_sweep(cand, Z, log_weights=lw if weighted else None, criteria=KEYS)
    check_sweep(r, sweep_reference("tile_edge", "rbf", weighted, 1e4, SCALE_SEED))


# ---------------------------------------------------------------------------------------------------- 3. anchors
@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_anchors_and_invariance(kernel):
    import torch
    sd, n, d, c, m, _, noise, ell, kvar = SWEEP_CASES["ragged_4chunks"]
    X, y, cand, Z, lw = case_data(sd, n, d, c, m)
    gp = make_gp(X, y, d, noise, ell, kvar, kernel)
    old = gp.wip_sweep(cand, Z)
    r0 = gp.wip_sweep(cand, Z, criteria=KEYS)
    # equal weights: the existing scorer's bits
    assert same_bits(r0["wipv"], old["wipv"]) and same_bits(r0["wipstd"], old["wipstd"])
    assert (r0["argmin_wipv"], r0["argmin_wipstd"]) == (old["argmin_v"], old["argmin_s"])
    assert same_bits(r0["min_wipv"], old["min_v"]) and same_bits(r0["min_wipstd"], old["min_s"])
    only = gp.wip_sweep(cand, Z, criteria=("imiqr",))
    assert set(only) == {"imiqr", "argmin_imiqr", "min_imiqr", "log_eiv_total"} and same_bits(only["imiqr"], r0["imiqr"])
    # explicit weights -mu_z are the posterior-draw weights
    mu = gp.predict_mean_batched(Z) - gp.y_mean
    rmu = gp.wip_sweep(cand, Z, log_weights=-np.asarray(mu), criteria=KEYS)
    for key in KEYS:
        err = score_error(key, rmu[key], r0[key])
        print("%-6s explicit -mu_z against None: %.3e" % (key, err))
        assert err <= 1e-12, key
    # chunk width, pointer kinds, repetition: the same bits
    rw = gp.wip_sweep(cand, Z, log_weights=lw)
    assert set(KEYS) <= set(rw)
    assert gp._lib.bobe_gp_set_chunk(gp._h, 128) == 0
    rc = gp.wip_sweep(cand, Z, log_weights=lw)
    assert gp._lib.bobe_gp_set_chunk(gp._h, 0) == 0
    dev = [torch.as_tensor(a, device="cuda") for a in (cand, Z, lw)]
    rd = gp.wip_sweep(dev[0], dev[1], log_weights=dev[2])
    rr = gp.wip_sweep(cand, Z, log_weights=lw)
    for other in (rc, rd, rr):
        for key in KEYS:
            assert same_bits(other[key], rw[key]) and other["argmin_" + key] == rw["argmin_" + key], key
        assert same_bits(other["log_eiv_total"], rw["log_eiv_total"])
    # device outputs through the C interface
    from bobe_amd import _lib
    outs = [torch.zeros(c, dtype=torch.float64, device="cuda") for _ in KEYS]
    ls = torch.zeros(1, dtype=torch.float64, device="cuda")
    am, mn = np.full(4, -7, dtype=np.int64), np.zeros(4)
    assert gp._lib.bobe_gp_wip_sweep_w(gp._h, _lib.ptr(dev[0]), c, _lib.ptr(dev[1]), m, float(gp.y_std), _lib.ptr(dev[2]),
                                       *[_lib.ptr(o) for o in outs], _lib.ptr(ls), _lib.ptr(am), _lib.ptr(mn)) == 0
    torch.cuda.synchronize()
    shift = {"imiqr": gp.y_mean, "eiv": -2.0 * gp.y_mean}
    for i, key in enumerate(KEYS):
        assert same_bits(outs[i].cpu().numpy() + shift.get(key, 0.0), rw[key]) and am[i] == rw["argmin_" + key]
    # the log scores move with a constant added to the weights, nothing else does
    rs = gp.wip_sweep(cand, Z, log_weights=lw + 3.25)
    for key in ("wipv", "wipstd"):
        assert score_error(key, rs[key], rw[key]) <= 1e-13
    assert score_error("imiqr", rs["imiqr"] - 3.25, rw["imiqr"]) <= 1e-13
    assert score_error("eiv", rs["eiv"] + 3.25, rw["eiv"]) <= 1e-13
    assert all(rs["argmin_" + key] == rw["argmin_" + key] for key in KEYS)
    with pytest.raises(ValueError):
        gp.wip_sweep(cand, Z, log_weights=lw[:-1])
    with pytest.raises(ValueError):
        gp.wip_sweep(cand, Z, log_weights=np.where(np.arange(m) == 3, np.inf, lw))
    with pytest.raises(ValueError):
        gp.wip_sweep(cand, Z, criteria=("ei",))


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
def test_candidates_are_the_integration_points(kernel):
    """``candidates is mc_points`` (N = 400, d = 4, M = 128): the sweep forms no V of its own."""
    n, d, m, noise, ell, kvar = 400, 4, 128, 1e-6, 0.5, 2.0
    X, y, _, Z, lw = case_data(41, n, d, 10, m)
    gp = make_gp(X, y, d, noise, ell, kvar, kernel)
    ys, y_mean, y_std = standardise(y)
    ref = W.weighted_scores(W.dense_state(kernel, X, ys, Z, Z, np.full(d, ell), kvar, noise), y_std, lw)
    ref["imiqr"], ref["eiv"], ref["log_s"] = ref["imiqr"] + y_mean, ref["eiv"] - 2 * y_mean, ref["log_s"] + 2 * y_mean
    r = gp.wip_sweep(Z, Z, log_weights=lw)
    check_sweep(r, ref)
    old = gp.wip_sweep(Z, Z)
    assert same_bits(gp.wip_sweep(Z, Z, criteria=("wipstd",))["wipstd"], old["wipstd"])
    for key in KEYS:
        b = gp.wip_select_batch_w(Z, Z, 3, criterion=key, return_stage_scores=True, log_weights=lw)
        assert same_bits(b["stage_scores"][0], r[key]) and b["indices"][0] == r["argmin_" + key]


# ---------------------------------------------------------------------------------------------------- 4. batch selection
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", list(BATCH_CASES))
def test_batch_against_literal_refits(name, key):
    sd, n, d, c, m, b, noise, ell, kvar = BATCH_CASES[name]
    X, y, cand, Z, lw = case_data(sd, n, d, c, m)
    gp = make_gp(X, y, d, noise, ell, kvar, "rbf")
    before = gp.wip_sweep(cand, Z, want_mean_var=True)
    sw = gp.wip_sweep(cand, Z, log_weights=lw, criteria=(key,))
    r = gp.wip_select_batch_w(cand, Z, b, criterion=key, return_stage_scores=True, log_weights=lw)
    assert same_bits(r["stage_scores"][0], sw[key]) and r["indices"][0] == sw["argmin_" + key]
    assert same_bits(r["scores"][0], sw["min_" + key])
    picks, stages, gaps = batch_reference(name, key)
    taken = []
    for j in range(b):
        g = gap(key, stages[j], taken)
        err = score_error(key, r["stage_scores"][j], stages[j])
        print("stage %d: error %.3e, the literal refit's gap %.3e" % (j, err, g))
        assert g > GAP_MIN, (j, g)
        assert err <= SCORE_RTOL, (j, err)
        assert r["indices"][j] == picks[j], j
        assert same_bits(r["scores"][j], r["stage_scores"][j, picks[j]])
        taken.append(int(picks[j]))
    # same state, same bits; the handle is left alone
    r2 = gp.wip_select_batch_w(cand, Z, b, criterion=key, return_stage_scores=True, log_weights=lw)
    assert same_bits(r2["stage_scores"], r["stage_scores"]) and r2["indices"].tolist() == r["indices"].tolist()
    after = gp.wip_sweep(cand, Z, want_mean_var=True)
    for k in ("wipv", "wipstd", "mean", "var"):
        assert same_bits(before[k], after[k]), k
    assert gp.npoints == n
    # the blocked substitution in place of the plain product: the same batch
    forced = make_gp(X, y, d, noise, ell, kvar, "rbf")
    forced.refine_kappa = 0.0
    forced.recompute_cholesky()
    assert forced.refining
    rf = forced.wip_select_batch_w(cand, Z, b, criterion=key, return_stage_scores=True, log_weights=lw)
    assert rf["indices"].tolist() == r["indices"].tolist()
    assert score_error(key, rf["stage_scores"], r["stage_scores"]) <= SCORE_RTOL
    assert same_bits(rf["stage_scores"][0], forced.wip_sweep(cand, Z, log_weights=lw, criteria=(key,))[key])


def test_equal_weight_batch_is_the_old_entry():
    sd, n, d, c, m, b, noise, ell, kvar = BATCH_CASES["n257"]
    X, y, cand, Z, _ = case_data(sd, n, d, c, m)
    gp = make_gp(X, y, d, noise, ell, kvar, "rbf")
    from bobe_amd import _lib
    for crit, key in enumerate(("wipv", "wipstd")):
        a = gp.wip_select_batch(cand, Z, 3, criterion=key, return_stage_scores=True)
        picks, vals, stage = np.full(3, -7, dtype=np.int64), np.zeros(3), np.zeros((3, c))
        assert gp._lib.bobe_gp_wip_select_batch_w(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std), None, 3, crit,
                                                  _lib.ptr(picks), _lib.ptr(vals), _lib.ptr(stage)) == 0
        assert picks.tolist() == a["indices"].tolist() and same_bits(stage, a["stage_scores"]) and same_bits(vals, a["scores"])


# ---------------------------------------------------------------------------------------------------- 5. errors
def _raw_batch(gp, cand, Z, lw, n_batch, criterion, picks):
    from bobe_amd import _lib
    return gp._lib.bobe_gp_wip_select_batch_w(gp._h, _lib.ptr(cand), int(cand.shape[0]), _lib.ptr(Z), int(Z.shape[0]),
                                              float(gp.y_std), _lib.ptr(lw), n_batch, criterion, _lib.ptr(picks), None, None)


def test_refusals():
    from bobe_amd import GP, _lib
    sd, n, d, c, m, _, noise, ell, kvar = SWEEP_CASES["below_the_unroll"]
    X, y, cand, Z, lw = case_data(sd, n, d, c, m)
    gp = make_gp(X, y, d, noise, ell, kvar, "rbf")
    for n_batch, criterion, null_picks in ((2, -1, False), (2, 4, False), (2, 2, True), (0, 2, False), (65, 3, False),
                                           (41, 3, False)):
        pk = None if null_picks else np.full(max(n_batch, 1), -7, dtype=np.int64)
        assert _raw_batch(gp, cand, Z, lw, n_batch, criterion, pk) == BOBE_ERR_ARG, (n_batch, criterion)
        assert _lib.last_error() and (pk is None or np.all(pk == -7))
    with pytest.raises(ValueError):
        gp.wip_select_batch_w(cand, Z, 2, criterion="ei", log_weights=lw)
    assert len(set(gp.wip_select_batch_w(cand, Z, 2, criterion="eiv", log_weights=lw)["indices"].tolist())) == 2
    bare = GP(X, y, noise=noise, lengthscales=np.full(d, ell), kernel_variance=kvar, _factor=False)
    pk = np.full(2, -7, dtype=np.int64)
    assert _raw_batch(bare, cand, Z, lw, 2, 2, pk) == BOBE_ERR_STATE and np.all(pk == -7)
    o = np.zeros(c)
    assert bare._lib.bobe_gp_wip_sweep_w(bare._h, _lib.ptr(cand), c, _lib.ptr(Z), m, 1.0, None, None, None, _lib.ptr(o), None,
                                         None, None, None) == BOBE_ERR_STATE


def test_a_nan_state_behaves_as_in_wip_sweep():
    """Not positive definite under the rank test: BOBE_OK as from bobe_gp_wip_sweep, and equal weights still give its bits."""
    from bobe_amd import GP
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(40, 3))
    X[7] = X[3]
    cand, Z = rng.uniform(size=(300, 3)), rng.uniform(size=(32, 3))
    gp = GP(X, np.sin(X[:, 0]), noise=1e-30, lengthscales=np.full(3, 0.5), kernel_variance=1.0, pivot_floor_ulp=64)
    assert gp.not_pd
    old = gp.wip_sweep(cand, Z)
    r = gp.wip_sweep(cand, Z, criteria=KEYS)
    assert same_bits(r["wipv"], old["wipv"]) and same_bits(r["wipstd"], old["wipstd"])
    b = gp.wip_select_batch_w(cand, Z, 3, criterion="imiqr", log_weights=np.zeros(32), return_stage_scores=True)
    for j in range(3):
        assert b["indices"][j] == W.masked_argmin(b["stage_scores"][j], b["indices"][:j])


# ---------------------------------------------------------------------------------------------------- 6. callers
@pytest.mark.parametrize("acq_name", ["IMIQR", "EIV"])
def test_get_next_batch_sweep_mode(acq_name):
    from bobe_amd import acquisition as A
    X, y, _, _, _ = case_data(51, 120, 3, 10, 8)
    gp = make_gp(X, y, 3, 1e-6, 0.5, 2.0, "rbf")
    acq = getattr(A, acq_name)()
    rng = np.random.default_rng(8)
    pool = rng.uniform(size=(700, 3))
    samples = {"x": pool, "weights": rng.uniform(0.1, 1.0, size=700), "logl": rng.normal(size=700)}
    kw = {"mc_samples": samples, "mc_points_size": 48}
    xb, vals = acq.get_next_batch(gp, n_batch=4, acq_kwargs=kw, rng=np.random.default_rng(5), batch_mode="sweep")
    rows = [int(np.flatnonzero(np.all(pool == x, axis=1))[0]) for x in xb]
    Z = A.get_mc_points(samples, mc_points_size=48, rng=np.random.default_rng(5))
    r = gp.wip_select_batch(pool, Z, 4, criterion=acq._key)
    assert rows == r["indices"].tolist() and same_bits(vals, r["scores"]) and np.all(np.isfinite(vals))
    # importance-weighted integration points
    Zw, lw = A.get_mc_points(samples, mc_points_size=48, weighted=True)
    xw, vw = acq.get_next_batch(gp, n_batch=3, acq_kwargs=dict(kw, mc_points=Zw, mc_log_weights=lw), batch_mode="sweep",
                                rng=np.random.default_rng(5))
    rw = gp.wip_select_batch_w(pool, Zw, 3, criterion=acq._key, log_weights=lw)
    assert np.array_equal(xw, pool[rw["indices"]]) and same_bits(vw, rw["scores"])
    x1, v1 = acq.get_next_point(gp, acq_kwargs=dict(kw, mc_points=Zw, mc_log_weights=lw), rng=np.random.default_rng(5),
                                verbose=False)
    sw = gp.wip_sweep(Zw, Zw, log_weights=lw, criteria=(acq._key,))
    assert np.array_equal(np.asarray(x1).reshape(-1), Zw[sw["argmin_" + acq._key]])


def _gauss2d(x):
    return -0.5 * ((x[0] - 0.3) ** 2 / 0.04 + (x[1] + 0.2) ** 2 / 0.09)


def test_bo_run_with_imiqr_on_weighted_nested_samples():
    from bobe_amd.bo import BOBE
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]]).T
    kw = dict(max_evals=24, fit_n_points=4, batch_size=4, mc_points_size=32, mc_points_method="NS")
    bobe = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False)
    res = bobe.run(acq="imiqr", mc_weighted=True, wip_batch_mode="sweep", **kw)
    assert 8 < res["gp"].npoints <= 24 and all(np.isfinite(res["acq_history"]))
    assert np.all(np.isfinite(res["gp"].train_y))


def test_default_wipstd_run_is_the_parent_commits():
    """``BOBE.run(acq='wipstd')`` with the default keywords (no ``mc_weighted``, the default ``wip_batch_mode``), for the
    integration-point methods 'NS' and 'uniform': the evaluated points, their values, the acquisition history and the state
    the run leaves its generator in are the ones recorded from the commit before the weighted criteria
    (tests/golden/default_wipstd_run.json, floats as hex), bit for bit."""
    import json
    from bobe_amd.bo import BOBE
    gold = json.load(open(os.path.join(HERE, "golden", "default_wipstd_run.json")))
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]]).T
    for method in ("NS", "uniform"):
        bobe = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=3, save=False)
        res = bobe.run(acq="wipstd", max_evals=20, fit_n_points=4, batch_size=4, mc_points_size=32, num_mc_samples=256,
                       mc_points_method=method)
        g, ref = res["gp"], gold[method]
        want_x = np.array([[float.fromhex(v) for v in row] for row in ref["train_x"]])
        assert g.train_x.shape == want_x.shape and same_bits(g.train_x, want_x), method
        y = np.asarray(g.train_y).reshape(-1) * g.y_std + g.y_mean
        assert same_bits(y, [float.fromhex(v) for v in ref["train_y_physical"]]), method
        assert same_bits(res["acq_history"], [float.fromhex(v) for v in ref["acq_history"]]), method
        st = bobe.np_rng.bit_generator.state
        assert st["bit_generator"] == ref["bit_generator"]
        assert {"state": str(st["state"]["state"]), "inc": str(st["state"]["inc"]), "has_uint32": int(st["has_uint32"]),
                "uinteger": int(st["uinteger"])} == ref["rng_state"], method


def test_argument_rules_of_the_python_surface():
    import torch
    from bobe_amd import acquisition as A
    from bobe_amd.bo import BOBE
    sd, n, d, c, m, _, noise, ell, kvar = SWEEP_CASES["below_the_unroll"]
    X, y, cand, Z, lw = case_data(sd, n, d, c, m)
    gp = make_gp(X, y, d, noise, ell, kvar, "rbf")
    good = torch.as_tensor(lw, device="cuda")
    assert same_bits(gp.wip_sweep(cand, Z, log_weights=good)["imiqr"], gp.wip_sweep(cand, Z, log_weights=lw)["imiqr"])
    wide = torch.as_tensor(np.repeat(lw, 2), device="cuda")
    for bad in (good.float(), good.cpu(), wide[::2], good[:-1]):          # float32, host memory, strided, too short
        with pytest.raises(ValueError):
            gp.wip_sweep(cand, Z, log_weights=bad)
    # integration points given without weights are not looked at: the draw is the usual one
    pool = np.random.default_rng(8).uniform(size=(200, d))
    kw = {"mc_samples": {"x": pool}, "mc_points_size": 16}
    acq = A.WIPStd()
    a = acq.get_next_batch(gp, n_batch=2, acq_kwargs=kw, rng=np.random.default_rng(5), batch_mode="sweep")
    b = acq.get_next_batch(gp, n_batch=2, acq_kwargs=dict(kw, mc_points=Z), rng=np.random.default_rng(5), batch_mode="sweep")
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    with pytest.raises(ValueError):
        acq.get_next_batch(gp, n_batch=2, acq_kwargs=dict(kw, mc_log_weights=lw), batch_mode="sweep")
    with pytest.raises(ValueError):
        BOBE(_gauss2d, ["x", "y"], np.array([[-1.0, 1.0], [-1.0, 1.0]]).T, n_sobol_init=8, seed=1, save=False).run(
            acq="imiqr", max_evals=12, mc_points_method="uniform", mc_weighted=True)
