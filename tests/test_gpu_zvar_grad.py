"""Value and input gradient of the evidence-variance score on the device (bobe_gp_wip_grad_zvar, GP.wip_grad_zvar) and the
polish built on them (acq_kwargs['zvar_polish'], BOBE.run(zvar_polish=)) against tests/zvar_grad_restatement.py.

Rule (the project's rule for gradients, tests/test_gpu_weighted_grad.py), per case and per output over the case's candidates,
the truth being the np.longdouble restatement:

    gradient   max |device - truth| <= 4 max |fp64 restatement - truth| + 1e-8 max |truth|
    value      |device - truth|_c   <= 4 max |fp64 restatement - truth| + 1e-8 (1 + |truth_c|)

Designs follow tests/zvar_cases.py::case_data (noise 1e-6, lengthscale 0.4, kernel variance 2): N = 160 / 300 (Np = 256 / 384: a
ragged last block), d = 2, 3, 5, both kernels, y_std = 1, 30, 4e3, with and without log-weights, C = 9 and 17 (a second group
of one), and M = 1, 63, 64, 65, 77, 257 - the pair kernel's lane (64 per workgroup) and tile (256 z') edges."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zvar_cases as ZC  # noqa: E402
import zvar_grad_restatement as ZG  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_STATE = -1, -3
NOISE, ELL, KVAR = 1e-6, 0.4, 2.0
# (N, d, kernel, y_std, log-weights given, C, M, the candidates are the integration points)
CASES = [
    (160, 2, "rbf", 1.0, True, 9, 1, False),
    (160, 3, "matern", 30.0, False, 17, 63, False),
    (160, 5, "rbf", 4e3, True, 9, 64, False),
    (300, 3, "matern", 1.0, True, 17, 65, False),
    (300, 3, "rbf", 30.0, False, 9, 77, False),
    (160, 2, "matern", 4e3, False, 17, 257, False),
    (300, 5, "rbf", 1.0, False, 9, 257, False),
    (160, 3, "rbf", 30.0, True, 63, 63, True),
    (300, 2, "matern", 30.0, True, 17, 64, False),
    (160, 5, "matern", 1.0, False, 9, 65, False),
    (300, 5, "matern", 4e3, True, 17, 77, False),
    (160, 3, "rbf", 4e3, False, 17, 1, False),
]
SWEEP_CASE = CASES[4]                                  # N = 300, d = 3


def _case_id(c):
    n, d, k, ys, w, cc, m, cz = c
    return f"N{n}_d{d}_{k}_ystd{ys:g}_{'weights' if w else 'draws'}_C{cc}_M{m}" + ("_cand_is_Z" if cz else "")


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@functools.lru_cache(maxsize=None)
def _data(case):
    """tests/zvar_cases.py::case_data's recipe: (X, y, cand, Z, log-weights or None)."""
    n, d, _, y_std, weighted, c, m, cand_is_z = case
    rng = np.random.default_rng(7000 + 10 * n + 100 * d + m)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    lw = 1.5 * rng.normal(size=m)
    y = (y - np.mean(y)) / np.std(y) * y_std + np.mean(y)
    return X, y, (Z if cand_is_z else cand), Z, (lw if weighted else None)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(long-double truth, fp64 restatement): value_and_grad dicts, computed once and left alone"""
    n, d, kernel = case[:3]
    X, y, cand, Z, lw = _data(case)
    ys, _, std = ZC.standardise(y)
    return tuple(ZG.value_and_grad(ZG.grad_state(kernel, X, ys, cand, Z, np.full(d, ELL), KVAR, NOISE, dt), std, lw)
                 for dt in (np.longdouble, np.float64))


def _gp(case):
    from bobe_amd import GP
    n, d, kernel = case[:3]
    X, y, cand, Z, lw = _data(case)
    return GP(X, y, noise=NOISE, kernel=kernel, lengthscales=np.full(d, ELL), kernel_variance=KVAR), cand, Z, lw


def _raw(gp, cand, c, Z, m, lw, zvar, dzvar, log_ez=None):
    from bobe_amd import _lib
    lez = None if log_ez is None else log_ez.ctypes.data_as(_lib.c_double_p)
    return gp._lib.bobe_gp_wip_grad_zvar(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std), _lib.ptr(lw), _lib.ptr(zvar),
                                         _lib.ptr(dzvar), lez)


def _same(a, b, row_a=slice(None), row_b=slice(None)):
    return same_bits(a["zvar"][row_a], b["zvar"][row_b]) and same_bits(a["dzvar"][row_a], b["dzvar"][row_b])


# ------------------------------------------------------------------------------------------------------------- 1. the truth
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_value_and_gradient_against_the_long_double_truth(case):
    n, d, kernel, y_std, weighted, c, m, _ = case
    gp, cand, Z, lw = _gp(case)
    assert abs(gp.y_std / y_std - 1) < 1e-12
    truth, f64 = _reference(case)
    assert np.all(np.isfinite(truth["zvar"])) and not np.any(truth["const"])
    r = gp.wip_grad_zvar(cand, Z, log_weights=lw)
    assert set(r) == {"zvar", "dzvar", "log_ez"} and r["zvar"].shape == (c,) and r["dzvar"].shape == (c, d)
    LD = np.longdouble
    tv, tg = truth["zvar"], truth["dzvar"]
    dev_v, ref_v = np.abs(r["zvar"].astype(LD) - tv), float(np.max(np.abs(f64["zvar"].astype(LD) - tv)))
    gs = float(np.max(np.abs(tg)))
    dev_g = float(np.max(np.abs(r["dzvar"].astype(LD) - tg))) / gs
    ref_g = float(np.max(np.abs(f64["dzvar"].astype(LD) - tg))) / gs
    lez = abs(r["log_ez"] - gp.y_mean - float(truth["log_ez"])) / (1 + abs(float(truth["log_ez"])))
    print(f"[zvar grad parity] {_case_id(case):<52} value dev = {float(np.max(dev_v / (1 + np.abs(tv)))):.3e} ref = "
          f"{float(np.max(np.abs(f64['zvar'].astype(LD) - tv) / (1 + np.abs(tv)))):.3e} (of 1 + |truth|)   gradient dev = "
          f"{dev_g:.3e} ref = {ref_g:.3e} (of max |truth| = {gs:.3e})   log_ez {lez:.3e}")
    assert np.all(np.isfinite(r["zvar"])) and np.all(np.isfinite(r["dzvar"]))
    assert np.all(dev_v <= 4 * ref_v + LD(1e-8) * (1 + np.abs(tv))), (float(np.max(dev_v)), ref_v)
    assert dev_g <= 4.0 * ref_g + 1e-8, (dev_g, ref_g)
    assert lez <= 1e-7, lez


def test_agreement_with_the_sweep_is_reported():
    """The sweep forms cross_z through crossT and the tile passes, this entry through the matrix-vector chain: each is held
    to the truth by its own rule, so the figure is printed, not asserted."""
    gp, cand, Z, lw = _gp(SWEEP_CASE)
    r = gp.wip_grad_zvar(cand, Z, log_weights=lw)
    sw = gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    print(f"[zvar grad parity] max |value - sweep| / (1 + |zvar|) = {float(np.max(np.abs(r['zvar'] - sw['zvar']) / (1 + np.abs(sw['zvar'])))):.3e}")
    assert same_bits(r["log_ez"], sw["log_ez"])


# ------------------------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=[_case_id(CASES[3]), _case_id(CASES[5])])
def test_a_candidates_bits_are_its_own(case):
    import torch
    n, d, kernel, _, _, c, m, _ = case
    gp, cand, Z, lw = _gp(case)
    assert c == 17
    full = gp.wip_grad_zvar(cand, Z, log_weights=lw)
    # alone, and at another place of a C = 17 call (the lone member of the second group becomes member 3 of the first)
    for i in (4, 16):
        assert _same(gp.wip_grad_zvar(cand[i:i + 1], Z, log_weights=lw), full, row_b=slice(i, i + 1)), i
    moved = np.ascontiguousarray(np.roll(cand, 4, axis=0))
    assert _same(gp.wip_grad_zvar(moved, Z, log_weights=lw), full, row_a=slice(3, 4), row_b=slice(16, 17))
    # device pointers, inputs and outputs
    dev = [torch.as_tensor(a, device="cuda") for a in (cand, Z)] + [None if lw is None else torch.as_tensor(lw, device="cuda")]
    zv, dz = torch.zeros(c, dtype=torch.float64, device="cuda"), torch.zeros((c, d), dtype=torch.float64, device="cuda")
    lez = np.zeros(1)
    assert _raw(gp, dev[0], c, dev[1], m, dev[2], zv, dz, lez) == 0
    torch.cuda.synchronize()
    assert same_bits(zv.cpu().numpy(), full["zvar"]) and same_bits(dz.cpu().numpy(), full["dzvar"])
    assert same_bits(lez[0] + gp.y_mean, full["log_ez"])
    # one output NULL; a device output beside a host one
    v1, g1 = np.zeros(c), np.zeros((c, d))
    assert _raw(gp, cand, c, Z, m, lw, v1, None) == 0 and _raw(gp, cand, c, Z, m, lw, None, g1) == 0
    assert same_bits(v1, full["zvar"]) and same_bits(g1, full["dzvar"])
    v2, g2 = np.zeros(1), torch.zeros((1, d), dtype=torch.float64, device="cuda")
    assert _raw(gp, cand[4:5], 1, Z, m, lw, v2, g2) == 0
    torch.cuda.synchronize()
    assert same_bits(v2, full["zvar"][4:5]) and same_bits(g2.cpu().numpy(), full["dzvar"][4:5])


def test_the_shared_caches_change_no_bit_of_anyone():
    case = CASES[3]
    gp, cand, Z, lw = _gp(case)
    fresh = _gp(case)[0]
    w0 = fresh.wip_grad_w(cand[:9], Z, log_weights=lw, criteria=("wipstd", "eiv"))     # on a handle that never saw zvar
    s0 = fresh.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    first = gp.wip_grad_zvar(cand, Z, log_weights=lw)            # a miss: fills prepare_z's cache and the table, lambda row too
    assert _same(gp.wip_grad_zvar(cand, Z, log_weights=lw), first)                      # a hit
    w1 = gp.wip_grad_w(cand[:9], Z, log_weights=lw, criteria=("wipstd", "eiv"))          # the sibling on the zvar-made table
    s1 = gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))
    assert all(same_bits(w1[k], w0[k]) for k in w0) and same_bits(s1["zvar"], s0["zvar"]) and same_bits(s1["log_ez"], s0["log_ez"])
    after = gp.wip_grad_zvar(cand, Z, log_weights=lw)            # after the sweep rewrote the Z side
    assert _same(after, first) and same_bits(after["log_ez"], first["log_ez"])
    # the other way round: the table made by wip_grad_w (no lambda row) gains it on a hit
    w2 = fresh.wip_grad_w(cand[:9], Z, log_weights=lw, criteria=("wipstd", "eiv"))
    z2 = fresh.wip_grad_zvar(cand, Z, log_weights=lw)
    w3 = fresh.wip_grad_w(cand[:9], Z, log_weights=lw, criteria=("wipstd", "eiv"))
    assert _same(z2, first) and same_bits(z2["log_ez"], first["log_ez"])
    assert all(same_bits(w2[k], w0[k]) and same_bits(w3[k], w0[k]) for k in w0)
    # other weights with the same Z: another result, and back
    lw2 = lw.copy()
    lw2[3] += 2.0
    assert not same_bits(gp.wip_grad_zvar(cand, Z, log_weights=lw2)["zvar"], first["zvar"])
    assert _same(gp.wip_grad_zvar(cand, Z, log_weights=lw), first)
    assert not same_bits(gp.wip_grad_zvar(cand, Z)["zvar"], first["zvar"])
    assert _same(gp.wip_grad_zvar(cand, Z, log_weights=lw), first)


# ------------------------------------------------------------------------------------------------- 3. edges and refusals
def test_refusals_leave_the_outputs_alone():
    from bobe_amd import GP, _lib
    from bobe_amd.acquisition import WIP_GRAD_W_MAX_N, ZVar
    case = CASES[4]
    gp, cand, Z, lw = _gp(case)
    c, m = cand.shape[0], Z.shape[0]
    v, g, lez = np.full(c, -7.0), np.full((c, 3), -7.0), np.full(1, -7.0)
    assert _raw(gp, cand, c, Z, m, lw, None, None, lez) == BOBE_ERR_ARG and "zvar and dzvar" in _lib.last_error()
    assert _raw(gp, None, c, Z, m, lw, v, g, lez) == BOBE_ERR_ARG
    assert _raw(gp, cand, c, None, m, lw, v, g, lez) == BOBE_ERR_ARG
    assert _raw(gp, cand, 0, Z, m, lw, v, g, lez) == BOBE_ERR_ARG
    assert _raw(gp, cand, c, Z, 0, lw, v, g, lez) == BOBE_ERR_ARG
    X, y = _data(case)[:2]
    bare = GP(X, y, noise=NOISE, lengthscales=np.full(3, ELL), kernel_variance=KVAR, _factor=False)
    assert _raw(bare, cand, c, Z, m, lw, v, g, lez) == BOBE_ERR_STATE
    rng = np.random.default_rng(12)
    Xb = rng.uniform(size=(WIP_GRAD_W_MAX_N + 1, 2))
    big = GP(Xb, np.sin(3.0 * Xb[:, 0]) + Xb[:, 1], noise=1e-2, lengthscales=np.full(2, 0.3), kernel_variance=1.0)
    Zb = rng.uniform(size=(16, 2))
    assert _raw(big, Zb[:1], 1, Zb, 16, None, v, g, lez) == BOBE_ERR_ARG and str(WIP_GRAD_W_MAX_N) in _lib.last_error()
    assert np.all(v == -7.0) and np.all(g == -7.0) and lez[0] == -7.0
    with pytest.raises(ValueError):
        gp.wip_grad_zvar(cand, Z, log_weights=np.zeros(m - 1))
    # the polish keeps the pool pick above the limit
    lwb = rng.normal(size=16)
    x, val = ZVar().get_next_point(big, acq_kwargs={"mc_points": Zb, "mc_log_weights": lwb, "zvar_polish": 2})
    sw = big.wip_sweep(Zb, Zb, log_weights=lwb, criteria=("zvar",))
    assert np.array_equal(x, Zb[sw["argmin_zvar"]]) and same_bits(val, sw["min_zvar"])


def test_a_nan_state_is_ok_and_a_training_point_gives_no_nan():
    from bobe_amd import GP
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(40, 3))
    cand, Z = rng.uniform(size=(5, 3)), rng.uniform(size=(32, 3))
    Xd = X.copy()
    Xd[7] = Xd[3]
    nan_gp = GP(Xd, np.sin(Xd[:, 0]), noise=1e-30, lengthscales=np.full(3, 0.5), kernel_variance=1.0, pivot_floor_ulp=64)
    assert nan_gp.not_pd
    v, g = np.zeros(5), np.zeros((5, 3))
    assert _raw(nan_gp, cand, 5, Z, 32, None, v, g) == 0
    # a candidate ON a training point where the noise is 1e-30: s_c is rounding noise of either sign
    # (the Matern kernel: its matrix on 40 points keeps its pivots far above the rank test's floor, the state is finite)
    gp = GP(X, np.sin(X[:, 0]), noise=1e-30, kernel="matern", lengthscales=np.full(3, 0.5), kernel_variance=1.0,
            pivot_floor_ulp=64)
    assert not gp.not_pd
    on = np.vstack([X[1:2], cand[:2], X[5:6]])
    r = gp.wip_grad_zvar(on, Z)
    print("on a training point: zvar", r["zvar"], "max |gradient|", np.max(np.abs(r["dzvar"]), axis=1))
    assert not np.any(np.isnan(r["dzvar"]))
    assert np.all(np.isfinite(r["zvar"]) | np.isposinf(r["zvar"]))
    assert np.all(r["dzvar"][np.isposinf(r["zvar"])] == 0.0)


# --------------------------------------------------------------------------------------------------------------- 4. callers
def _gauss2d(x):
    return -0.5 * ((x[0] - 0.3) ** 2 / 0.04 + (x[1] + 0.2) ** 2 / 0.09)


def test_zvar_polish_in_the_acquisition():
    """tests/test_gpu_zvar.py::test_zvar_acquisition_picks_from_the_pool's setup."""
    from bobe_amd import GP
    from bobe_amd import acquisition as A
    _, n, d, _, _, _, noise, ell, kvar = ZC.SHAPES["tile_edge"]
    X, y = ZC.case_data("tile_edge", 1.0)[:2]
    gp = GP(X, y, noise=noise, kernel="rbf", lengthscales=np.full(d, ell), kernel_variance=kvar)
    rng = np.random.default_rng(8)
    pool = rng.uniform(size=(400, 3))
    samples = {"x": pool, "weights": rng.uniform(0.1, 1.0, size=400), "logl": rng.normal(size=400)}
    Zw, lw = A.get_mc_points(samples, mc_points_size=48, weighted=True)
    kw = {"mc_samples": samples, "mc_points_size": 48, "mc_points": Zw, "mc_log_weights": lw}
    r0, r1, r3, r4 = (np.random.default_rng(5) for _ in range(4))
    x_pool, v_pool = A.ZVar().get_next_point(gp, acq_kwargs=dict(kw), rng=r0, verbose=False)
    x_zero, v_zero = A.ZVar().get_next_point(gp, acq_kwargs=dict(kw, zvar_polish=0), rng=r1, verbose=False)
    assert np.array_equal(x_pool, x_zero) and same_bits(v_pool, v_zero)
    sw = gp.wip_sweep(Zw, Zw, log_weights=lw, criteria=("zvar",))
    assert np.array_equal(np.asarray(x_pool).reshape(-1), Zw[sw["argmin_zvar"]]) and same_bits(v_pool, sw["min_zvar"])
    x, v = A.ZVar().get_next_point(gp, acq_kwargs=dict(kw, zvar_polish=3), rng=r3, verbose=False)
    x2, v2 = A.ZVar().get_next_point(gp, acq_kwargs=dict(kw, zvar_polish=3), rng=r4, verbose=False)
    print(f"ZVar: pool pick {v_pool:.6g} -> polished {v:.6g} (moved {np.max(np.abs(x - x_pool)):.3g})")
    assert x.shape == (3,) and np.all((x >= 0.0) & (x <= 1.0)) and v <= v_pool
    assert np.array_equal(x, x2) and same_bits(v, v2)
    assert r3.bit_generator.state == r0.bit_generator.state == r1.bit_generator.state     # the polish draws nothing
    at = gp.wip_grad_zvar(np.asarray(x)[None, :], Zw, log_weights=lw)["zvar"][0]
    assert same_bits(at, v) or np.array_equal(x, x_pool)
    with pytest.raises(ValueError, match="zvar_polish"):
        A.ZVar().get_next_point(gp, acq_kwargs=dict(kw, weighted_polish=2), rng=np.random.default_rng(5), verbose=False)


def test_bo_run_with_the_zvar_polish():
    from bobe_amd.bo import BOBE
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]]).T
    kw = dict(max_evals=24, fit_n_points=4, batch_size=4, mc_points_size=32, mc_points_method="NS")
    bobe = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False)
    res = bobe.run(acq="zvar", mc_weighted=True, zvar_polish=2, **kw)
    assert 8 < res["gp"].npoints <= 24 and all(np.isfinite(res["acq_history"]))
    assert np.all(np.isfinite(res["gp"].train_y))
    with pytest.raises(ValueError, match="zvar_polish"):
        BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="wipstd", zvar_polish=2, **kw)
    with pytest.raises(ValueError):
        BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False).run(acq="zvar", zvar_polish=17, **kw)
