"""The expected evidence variance as a sweep criterion on the device (bobe_gp_wip_sweep_zvar, bobe_gp_wip_select_batch_zvar,
GP.wip_sweep(criteria=('zvar',)), GP.wip_select_batch_w(criterion='zvar'), acquisition.ZVar, BOBE.run(acq='zvar')) against the
long-double truth of tests/zvar_restatement.py on the cases of tests/zvar_cases.py.

Rule, per candidate: |device - truth| <= 4 |float64 restatement - truth| + 1e-7 (1 + |truth|) (the project's log-score
tolerance, with the float64 restatement's own error as the yardstick of what fp64 can deliver on the case); the same argmin
as the truth under the precondition - asserted in tests/test_zvar_cpu.py - that the truth's two best scores differ by more than
1e-6; log_ez to 1e-7 (1 + |truth|).

Edge rules restated: |r_z| <= sqrt(b_z); a non-finite cross_z gives r_z = 0; a candidate whose s_c is not > 0 has every r_z =
0; T <= 0 gives zvar = +inf, which never wins an argmin over a finite score (all +inf: index 0); a NaN state: BOBE_OK."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zvar_cases as ZC  # noqa: E402
from batch_select_restatement import masked_argmin  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_STATE = -1, -3
KEYS = ("wipv", "wipstd", "imiqr", "eiv")


def make_gp(shape, kernel, y_std, refine=False):
    from bobe_amd import GP
    _, n, d, c, m, chunk, noise, ell, kvar = ZC.SHAPES[shape]
    X, y, cand, Z, lw = ZC.case_data(shape, y_std)
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=np.full(d, ell), kernel_variance=kvar)
    if refine:
        gp.refine_kappa = 0.0
        gp.recompute_cholesky()
        assert gp.refining
    if chunk:
        assert gp._lib.bobe_gp_set_chunk(gp._h, chunk) == 0
    return gp, cand, Z, lw


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def check_sweep(r, case):
    ref = ZC.sweep_reference(case)
    ok, err, ref_err = ZC.rule(r["zvar"], ref["f64"], ref["truth"])
    lez = abs(r["log_ez"] - float(ref["log_ez"])) / (1 + abs(float(ref["log_ez"])))
    print("%-50s device %.3e, float64 restatement %.3e (of 1 + |truth|), log_ez %.3e" % (ZC.case_id(case), err, ref_err, lez))
    assert np.all(np.isfinite(r["zvar"]))
    assert ok, (err, ref_err)
    assert r["argmin_zvar"] == masked_argmin(ref["truth"])
    assert same_bits(r["min_zvar"], r["zvar"][r["argmin_zvar"]])
    assert lez <= 1e-7, lez


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", ZC.SWEEP_CASES, ids=ZC.case_id)
def test_sweep_matches_the_long_double_truth(case):
    shape, kernel, weighted, y_std = case
    gp, cand, Z, lw = make_gp(shape, kernel, y_std)
    assert abs(gp.y_std / y_std - 1) < 1e-12
    r = gp.wip_sweep(cand, Z, log_weights=lw if weighted else None, criteria=("zvar",))
    assert set(r) == {"zvar", "argmin_zvar", "min_zvar", "log_ez"}
    check_sweep(r, case)


@pytest.mark.parametrize("case", [ZC.SWEEP_CASES[0], ZC.SWEEP_CASES[7]], ids=ZC.case_id)
def test_sweep_on_the_substitution_path(case):
    """``set_refine_kappa(0)``: V from the blocked substitution instead of the product with the inverse factor."""
    shape, kernel, weighted, y_std = case
    gp, cand, Z, lw = make_gp(shape, kernel, y_std, refine=True)
    check_sweep(gp.wip_sweep(cand, Z, log_weights=lw if weighted else None, criteria=("zvar",)), case)


# ---------------------------------------------------------------------------------------------------- 2. bits
def test_same_bits_whatever_the_call_shape():
    """Chunk width, host or device pointers, repetition, and C = 1 against the same candidate inside a large C."""
    import torch
    from bobe_amd import _lib
    case = ("ragged_4chunks", "rbf", True, 30.0)
    gp, cand, Z, lw = make_gp(*case[:2], case[3])
    c, m = cand.shape[0], Z.shape[0]
    r = gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    for chunk in (128, 0):
        assert gp._lib.bobe_gp_set_chunk(gp._h, chunk) == 0
        o = gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
        assert same_bits(o["zvar"], r["zvar"]) and o["argmin_zvar"] == r["argmin_zvar"] and same_bits(o["log_ez"], r["log_ez"])
    dev = [torch.as_tensor(a, device="cuda") for a in (cand, Z, lw)]
    o = gp.wip_sweep(dev[0], dev[1], log_weights=dev[2], criteria=("zvar",))
    assert same_bits(o["zvar"], r["zvar"]) and o["argmin_zvar"] == r["argmin_zvar"] and same_bits(o["log_ez"], r["log_ez"])
    out = torch.zeros(c, dtype=torch.float64, device="cuda")
    am, mn, lez = np.full(1, -7, dtype=np.int64), np.zeros(1), np.zeros(1)
    assert gp._lib.bobe_gp_wip_sweep_zvar(gp._h, _lib.ptr(dev[0]), c, _lib.ptr(dev[1]), m, float(gp.y_std), _lib.ptr(dev[2]),
                                          _lib.ptr(out), lez.ctypes.data_as(_lib.c_double_p),
                                          am.ctypes.data_as(_lib.c_int64_p), mn.ctypes.data_as(_lib.c_double_p)) == 0
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), r["zvar"]) and am[0] == r["argmin_zvar"] and same_bits(mn[0], r["min_zvar"])
    assert same_bits(lez[0] + gp.y_mean, r["log_ez"])
    for i in (0, 517, c - 1):
        one = gp.wip_sweep(cand[i:i + 1], Z, log_weights=lw, criteria=("zvar",))
        assert same_bits(one["zvar"][0], r["zvar"][i]) and one["argmin_zvar"] == 0
    # every output pointer may be NULL
    assert gp._lib.bobe_gp_wip_sweep_zvar(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std), None, None, None, None,
                                          None) == 0


def test_invariances_on_the_device():
    case = ("tile_edge", "rbf", True, 1.0)
    gp, cand, Z, lw = make_gp(*case[:2], case[3])
    r = gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    rs = gp.wip_sweep(cand, Z, log_weights=lw + 3.25, criteria=("zvar",))
    assert np.max(np.abs(rs["zvar"] - r["zvar"])) <= 1e-10 and abs(rs["log_ez"] - 3.25 - r["log_ez"]) <= 1e-10
    assert rs["argmin_zvar"] == r["argmin_zvar"]
    # y_mean: the score does not move, log_ez moves with it
    from bobe_amd import GP
    _, n, d, c, m, _, noise, ell, kvar = ZC.SHAPES[case[0]]
    X, y, _, _, _ = ZC.case_data(case[0], case[3])
    gp2 = GP(X, y + 17.5, noise=noise, kernel="rbf", lengthscales=np.full(d, ell), kernel_variance=kvar)
    r2 = gp2.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    assert np.max(np.abs(r2["zvar"] - r["zvar"])) <= 1e-7 and abs(r2["log_ez"] - 17.5 - r["log_ez"]) <= 1e-7
    # posterior-draw weights are the explicit l_z = -mu_z
    mu = np.asarray(gp.predict_mean_batched(Z)) - gp.y_mean
    r0, rmu = gp.wip_sweep(cand, Z, criteria=("zvar",)), gp.wip_sweep(cand, Z, log_weights=-mu, criteria=("zvar",))
    assert np.max(np.abs(r0["zvar"] - rmu["zvar"])) <= 1e-9


# ---------------------------------------------------------------------------------------------------- 3. the batch entry
def test_batch_against_literal_refits():
    shape, kernel, weighted, y_std, b = ZC.BATCH_CASE
    gp, cand, Z, lw = make_gp(shape, kernel, y_std)
    before = gp.wip_sweep(cand, Z, want_mean_var=True)
    sw = gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    r = gp.wip_select_batch_w(cand, Z, b, criterion="zvar", return_stage_scores=True, log_weights=lw)
    assert same_bits(r["stage_scores"][0], sw["zvar"]) and r["indices"][0] == sw["argmin_zvar"]
    assert same_bits(r["scores"][0], sw["min_zvar"])
    (p64, s64, _), (pld, sld, gaps) = ZC.batch_reference()
    assert len(set(r["indices"].tolist())) == b
    for j in range(b):
        ok, err, ref_err = ZC.rule(r["stage_scores"][j], s64[j], sld[j])
        print("stage %d: device %.3e, float64 literal refit %.3e, the truth's gap %.3e" % (j, err, ref_err, gaps[j]))
        assert gaps[j] > ZC.GAP_MIN
        assert ok, (j, err, ref_err)
        assert r["indices"][j] == pld[j], j
        assert same_bits(r["scores"][j], r["stage_scores"][j, pld[j]])
    r2 = gp.wip_select_batch_w(cand, Z, b, criterion="zvar", return_stage_scores=True, log_weights=lw)
    assert same_bits(r2["stage_scores"], r["stage_scores"]) and r2["indices"].tolist() == r["indices"].tolist()
    after = gp.wip_sweep(cand, Z, want_mean_var=True)
    for k in ("wipv", "wipstd", "mean", "var"):
        assert same_bits(before[k], after[k]), k
    # cand is Z, without weights, through the acquisition's route
    gz, _, Zz, lwz = make_gp("cand_is_z", "rbf", 1.0)
    sz = gz.wip_sweep(Zz, Zz, criteria=("zvar",))
    bz = gz.wip_select_batch_w(Zz, Zz, 3, criterion="zvar", return_stage_scores=True)
    assert same_bits(bz["stage_scores"][0], sz["zvar"]) and len(set(bz["indices"].tolist())) == 3


# ---------------------------------------------------------------------------------------------------- 4. existing outputs
def test_existing_outputs_keep_their_bits_beside_zvar():
    case = ("tile_edge", "matern", True, 30.0)
    gp, cand, Z, lw = make_gp(*case[:2], case[3])
    for weights in (lw, None):
        a = gp.wip_sweep(cand, Z, log_weights=weights, criteria=KEYS)
        b = gp.wip_sweep(cand, Z, log_weights=weights, criteria=KEYS + ("zvar",))
        assert set(b) == set(a) | {"zvar", "argmin_zvar", "min_zvar", "log_ez"}
        for k in a:
            assert same_bits(a[k], b[k]) if isinstance(a[k], (np.ndarray, float)) else a[k] == b[k], k
        assert same_bits(b["zvar"], gp.wip_sweep(cand, Z, log_weights=weights, criteria=("zvar",))["zvar"])
    e1 = gp.wip_select_batch_w(cand, Z, 3, criterion="eiv", return_stage_scores=True, log_weights=lw)
    gp.wip_select_batch_w(cand, Z, 3, criterion="zvar", log_weights=lw)
    e2 = gp.wip_select_batch_w(cand, Z, 3, criterion="eiv", return_stage_scores=True, log_weights=lw)
    assert same_bits(e1["stage_scores"], e2["stage_scores"]) and e1["indices"].tolist() == e2["indices"].tolist()
    with pytest.raises(ValueError):
        gp.wip_grad_w(cand[:2], Z, log_weights=lw, criteria=("zvar",))
    with pytest.raises(ValueError):
        gp.wip_sweep(cand, Z, criteria=("zvar", "ei"))
    assert gp.CRITERIA == KEYS


# ---------------------------------------------------------------------------------------------------- 5. edges and errors
def test_a_candidate_on_a_training_point_at_noise_1e_30():
    """s_c of such a candidate is rounding (about 1e-16, either sign).  Not > 0: every r_z = 0 and the score is +inf.  Tiny
    and positive: r is capped at sqrt(b_z).  Either way the score is no NaN, and a +inf does not win the argmin."""
    from bobe_amd import GP
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(40, 3))
    cand, Z = rng.uniform(size=(70, 3)), rng.uniform(size=(33, 3))
    cand[0], cand[37], cand[69] = X[3], X[11], X[39]
    Z[5] = X[7]
    gp = GP(X, np.sin(3 * X[:, 0]) + X[:, 1], noise=1e-30, lengthscales=np.full(3, 0.3), kernel_variance=1.0)
    if gp.not_pd:
        pytest.fail("the design did not factorise: choose another one")
    r = gp.wip_sweep(cand, Z, criteria=("zvar",))
    z = r["zvar"]
    print("on training points:", z[[0, 37, 69]], " others: min %.3f max %.3f" % (np.min(z[1:37]), np.max(z[1:37])))
    assert not np.any(np.isnan(z)) and not np.any(np.isneginf(z)) and np.isfinite(r["log_ez"])
    assert np.any(np.isfinite(z)) and np.isfinite(z[r["argmin_zvar"]]) and r["argmin_zvar"] == masked_argmin(z)
    b = gp.wip_select_batch_w(cand, Z, 3, criterion="zvar", return_stage_scores=True)
    for j in range(3):
        assert not np.any(np.isnan(b["stage_scores"][j]))
        assert b["indices"][j] == masked_argmin(b["stage_scores"][j], b["indices"][:j])


def test_a_nan_state_returns_ok():
    from bobe_amd import GP
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(40, 3))
    X[7] = X[3]
    cand, Z = rng.uniform(size=(300, 3)), rng.uniform(size=(32, 3))
    gp = GP(X, np.sin(X[:, 0]), noise=1e-30, lengthscales=np.full(3, 0.5), kernel_variance=1.0, pivot_floor_ulp=64)
    assert gp.not_pd
    r = gp.wip_sweep(cand, Z, criteria=("zvar",))
    assert np.all(np.isnan(r["zvar"]) | np.isposinf(r["zvar"])) and r["argmin_zvar"] == masked_argmin(r["zvar"])
    b = gp.wip_select_batch_w(cand, Z, 2, criterion="zvar", log_weights=np.zeros(32))
    assert len(set(b["indices"].tolist())) == 2


def test_refusals():
    from bobe_amd import GP, _lib
    gp, cand, Z, lw = make_gp("below_the_unroll", "rbf", 1.0)
    c, m = cand.shape[0], Z.shape[0]
    o, pk = np.zeros(c), np.full(2, -7, dtype=np.int64)
    L = gp._lib

    def sweep(h, cd, cc, zz, mm):
        return L.bobe_gp_wip_sweep_zvar(h, _lib.ptr(cd), cc, _lib.ptr(zz), mm, 1.0, _lib.ptr(lw), _lib.ptr(o), None, None, None)

    def batch(h, cd, cc, zz, mm, nb, picks):
        return L.bobe_gp_wip_select_batch_zvar(h, _lib.ptr(cd), cc, _lib.ptr(zz), mm, 1.0, _lib.ptr(lw), nb, _lib.ptr(picks),
                                               None, None)
    for args in ((None, c, Z, m), (cand, c, None, m), (cand, 0, Z, m), (cand, c, Z, 0)):
        assert sweep(gp._h, *args) == BOBE_ERR_ARG and _lib.last_error()
        assert batch(gp._h, *args, 2, pk) == BOBE_ERR_ARG and np.all(pk == -7)
    assert sweep(None, cand, c, Z, m) == BOBE_ERR_ARG
    for nb, picks in ((0, pk), (65, np.full(65, -7, dtype=np.int64)), (41, np.full(41, -7, dtype=np.int64)), (2, None)):
        assert batch(gp._h, cand, c, Z, m, nb, picks) == BOBE_ERR_ARG, nb
    _, n, d, _, _, _, noise, ell, kvar = ZC.SHAPES["below_the_unroll"]
    X, y, _, _, _ = ZC.case_data("below_the_unroll", 1.0)
    bare = GP(X, y, noise=noise, lengthscales=np.full(d, ell), kernel_variance=kvar, _factor=False)
    assert sweep(bare._h, cand, c, Z, m) == BOBE_ERR_STATE
    assert batch(bare._h, cand, c, Z, m, 2, pk) == BOBE_ERR_STATE and np.all(pk == -7)
    assert np.all(o == 0.0)
    with pytest.raises(ValueError):
        gp.wip_select_batch_w(cand, Z, 2, criterion="zv")
    assert len(set(gp.wip_select_batch_w(cand, Z, 2, criterion="zvar", log_weights=lw)["indices"].tolist())) == 2


# ---------------------------------------------------------------------------------------------------- 6. callers
def _gauss2d(x):
    return -0.5 * ((x[0] - 0.3) ** 2 / 0.04 + (x[1] + 0.2) ** 2 / 0.09)


def test_zvar_acquisition_picks_from_the_pool():
    from bobe_amd import acquisition as A
    gp, _, _, _ = make_gp("tile_edge", "rbf", 1.0)
    acq = A.ZVar()
    rng = np.random.default_rng(8)
    pool = rng.uniform(size=(400, 3))
    samples = {"x": pool, "weights": rng.uniform(0.1, 1.0, size=400), "logl": rng.normal(size=400)}
    kw = {"mc_samples": samples, "mc_points_size": 48}
    Zw, lw = A.get_mc_points(samples, mc_points_size=48, weighted=True)
    x1, v1 = acq.get_next_point(gp, acq_kwargs=dict(kw, mc_points=Zw, mc_log_weights=lw), rng=np.random.default_rng(5),
                                verbose=False)
    sw = gp.wip_sweep(Zw, Zw, log_weights=lw, criteria=("zvar",))
    assert np.array_equal(np.asarray(x1).reshape(-1), Zw[sw["argmin_zvar"]]) and same_bits(v1, sw["min_zvar"])
    xb, vb = acq.get_next_batch(gp, n_batch=3, acq_kwargs=kw, rng=np.random.default_rng(5), batch_mode="sweep")
    Z = A.get_mc_points(samples, mc_points_size=48, rng=np.random.default_rng(5))
    rb = gp.wip_select_batch_w(pool, Z, 3, criterion="zvar")
    assert np.array_equal(xb, pool[rb["indices"]]) and same_bits(vb, rb["scores"])
    with pytest.raises(ValueError):
        acq.get_next_point(gp, acq_kwargs=dict(kw, weighted_polish=2), rng=np.random.default_rng(5), verbose=False)


def test_bo_run_with_zvar_on_weighted_nested_samples():
    from bobe_amd.bo import BOBE
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]]).T
    kw = dict(max_evals=24, fit_n_points=4, batch_size=4, mc_points_size=32, mc_points_method="NS")
    bobe = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False)
    res = bobe.run(acq="zvar", mc_weighted=True, **kw)
    assert 8 < res["gp"].npoints <= 24 and all(np.isfinite(res["acq_history"]))
    assert np.all(np.isfinite(res["gp"].train_y))
    with pytest.raises(ValueError):
        BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="zvar", weighted_polish=2, **kw)
    with pytest.raises(ValueError):
        BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="zv", **kw)
