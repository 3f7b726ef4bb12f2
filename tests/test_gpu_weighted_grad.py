"""Input gradients of the weighted criteria on the device (bobe_gp_wip_grad_w, GP.wip_grad_w) and the polish built on them
(acq_kwargs['weighted_polish'], BOBE.run(weighted_polish=)) against tests/weighted_grad_restatement.py.

Gradients follow the conditioning ladder's rule with the project's gradient tolerance: per criterion and
case, over the case's candidates,

    max |device - truth| <= 4 max |fp64 restatement - truth| + 1e-8 max |truth|,

the truth being the np.longdouble restatement.  Every measured pair is printed before it is asserted; with
BOBE_WEIGHTED_GRAD_PARITY_OUT=<file> the table is written there (committed as profiles/weighted_grad_parity.txt).

All cases: N = 160 or 300 (Np = 256 / 384: a ragged last block), noise = 1e-6.  At that noise no integration point floors: a z
that is a training point has base_z in [noise, 2 noise), eight orders above the 1e-12 floor, and v+ >= ~noise for every
candidate - the "floored-z candidate" of the CPU test (tests/test_weighted_grad_cpu.py, noise 1e-13) is here the candidate
1e-9 from such a z, held to the same rule, with the truth's floored count printed (0).  The floor branch of the kernels runs
in the NaN-state test.
Lengthscale 0.4, kernel variance 2 (the sweep cases of tests/test_gpu_weighted_criteria.py): the fantasy variances stay above
~1e-4 of k(x, x).  Two fp64 routes to v+ = base - cross^2 / s differ by ~eps k(x, x) / v+ relative, so the 1e-10 agreement of the
values with the sweep presupposes v+ >~ 1e-5 k(x, x); at lengthscale 0.6 and d = 3 these 160 points pin the surrogate down to
v+ ~ 1e-6 k(x, x), where the sweep and the matrix-vector chain - each as close to the truth as fp64 allows - agree to 1.2e-10."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import weighted_grad_restatement as R  # noqa: E402
from test_gpu_weighted_criteria import case_data, make_gp, same_bits, standardise  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_STATE = -1, -3
KEYS = R.KEYS
NOISE, ELL, KVAR = 1e-6, 0.4, 2.0
GRID = [("rbf", 3, 70), ("matern", 5, 300), ("rbf", 12, 33), ("matern", 17, 33)]
GRID_IDS = [f"{k}_d{d}_M{m}" for k, d, m in GRID]
_ROWS = {}


def _n_of(m):
    return 300 if m == 300 else 160


@functools.lru_cache(maxsize=None)
def _data(kernel, d, m, y_scale=1.0, special=False):
    """(X, y, cand (9, d), Z, log-weights) of a grid case.  special: Z[0] is the training point X[0], candidate 0 lies 1e-9
    from it and candidate 1 IS the training point X[1]."""
    X, y, cand, Z, lw = case_data(1000 + 10 * d + m, _n_of(m), d, 9, m, y_scale)
    cand = 0.1 + 0.8 * cand
    if special:
        Z, cand = Z.copy(), cand.copy()
        Z[0] = X[0]
        cand[0] = X[0] + 1e-9
        cand[1] = X[1]
    return X, y, cand, Z, lw


@functools.lru_cache(maxsize=None)
def _reference(kernel, d, m, weighted, y_scale=1.0, special=False):
    """(long-double truth, fp64 restatement) of a case: value_and_grad dicts, computed once"""
    X, y, cand, Z, lw = _data(kernel, d, m, y_scale, special)
    ys, _, y_std = standardise(y)
    out = []
    for dt in (np.longdouble, np.float64):
        st = R.State(kernel, X, ys, Z, np.full(d, ELL), KVAR, NOISE, y_std, lw if weighted else None, dt)
        out.append(R.value_and_grad(st, cand))
    return tuple(out)


def _gp(kernel, d, m, y_scale=1.0, special=False, refine=False):
    X, y, cand, Z, lw = _data(kernel, d, m, y_scale, special)
    gp = make_gp(X, y, d, NOISE, ELL, KVAR, kernel)
    if refine:
        gp.refine_kappa = 0.0
        gp.recompute_cholesky()
        assert gp.refining
    return gp, cand, Z, lw


def _record(name, figs):
    _ROWS[name] = figs
    out = os.environ.get("BOBE_WEIGHTED_GRAD_PARITY_OUT")
    if not out:
        return
    try:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        lines = ["# weighted score gradients (tests/test_gpu_weighted_grad.py): max |delta| / max |truth| over the case's candidates "
                 "and coordinates, against the np.longdouble truth",
                 "# dev = bobe_gp_wip_grad_w, ref = the fp64 restatement (SciPy cholesky / solve_triangular); rule: dev <= 4 x ref + 1e-8",
                 "", f"{'case':<44}{'refining':>9} " + " ".join(f"{'dev_' + k:>11}{'ref_' + k:>11}" for k in KEYS)]
        for nm, r in _ROWS.items():
            lines.append(f"{nm:<44}{str(r['refining']):>9} " + " ".join(f"{r['dev_' + k]:>11.2e}{r['ref_' + k]:>11.2e}" for k in KEYS))
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("weighted", [False, True], ids=["posterior_draws", "weights"])
@pytest.mark.parametrize("kernel,d,m", GRID, ids=GRID_IDS)
def test_values_are_the_sweeps(kernel, d, m, weighted):
    """M = 70: Mp = 128, two k_wg_cross_w workgroups, one half empty; M = 300: five of six; M = 33: a lone partial one and an
    empty one."""
    gp, cand, Z, lw = _gp(kernel, d, m)
    w = lw if weighted else None
    r = gp.wip_grad_w(cand, Z, log_weights=w)
    sw = gp.wip_sweep(cand, Z, log_weights=w, criteria=KEYS)
    assert set(r) == set(KEYS) | {"d" + k for k in KEYS}
    for k in KEYS:
        err = float(np.max(np.abs(r[k] - sw[k]) / np.abs(sw[k])))
        print(f"{k}: {err:.3e}")
        assert r[k].shape == (9,) and r["d" + k].shape == (9, d) and np.all(np.isfinite(r["d" + k]))
        assert np.allclose(r[k], sw[k], rtol=1e-10, atol=0.0), (k, err)


# -------------------------------------------------------------------------------------------- 2. gradients against the truth
TRUTH_CASES = [(k, d, m, w, 1.0, False, False) for (k, d, m) in GRID for w in (False, True)] + [
    ("rbf", 3, 70, False, 1e4, False, False), ("matern", 5, 300, True, 1e4, False, False),       # y_std ~ 4e3
    ("rbf", 3, 70, True, 1.0, True, False), ("matern", 17, 33, False, 1.0, True, False),         # next to / on a training point
    ("rbf", 12, 33, True, 1.0, False, True), ("matern", 5, 300, False, 1.0, False, True)]        # the refinement step on


def _case_id(c):
    k, d, m, w, ys, sp, rf = c
    return f"{k}_d{d}_M{m}_{'weights' if w else 'draws'}" + ("_y1e4" if ys != 1.0 else "") + ("_at_training_point" if sp else "") \
        + ("_refined" if rf else "")


@pytest.mark.parametrize("case", TRUTH_CASES, ids=[_case_id(c) for c in TRUTH_CASES])
def test_gradients_against_the_long_double_truth(case):
    kernel, d, m, weighted, y_scale, special, refine = case
    gp, cand, Z, lw = _gp(kernel, d, m, y_scale, special, refine)
    if y_scale != 1.0:
        assert 3e3 < gp.y_std < 6e3
    truth, f64 = _reference(kernel, d, m, weighted, y_scale, special)
    r = gp.wip_grad_w(cand, Z, log_weights=lw if weighted else None)
    rows = slice(None)
    if special:
        print(f"truth: {int(truth['floored'][0].sum())} of {m} integration points floored for the candidate 1e-9 from Z[0] = X[0]")
        assert all(np.all(np.isfinite(r[k])) and np.all(np.isfinite(r["d" + k])) for k in KEYS)      # candidate 1 included
        rows = [0] + list(range(2, 9))                # candidate 1 sits ON a training point: finite outputs are what is asked
    figs = {"refining": bool(gp.refining)}
    for k in KEYS:
        t = truth["d" + k][rows]
        scale = float(np.max(np.abs(t)))
        figs["dev_" + k] = float(np.max(np.abs(r["d" + k][rows] - t))) / scale
        figs["ref_" + k] = float(np.max(np.abs(f64["d" + k][rows] - t))) / scale
        print(f"[weighted grad parity] {_case_id(case):<44} {k:<6} err(device) = {figs['dev_' + k]:.3e}   err(fp64 restatement) = "
              f"{figs['ref_' + k]:.3e}   max |truth| = {scale:.3e}")
    _record(_case_id(case), figs)
    for k in KEYS:
        assert figs["dev_" + k] <= 4.0 * figs["ref_" + k] + 1e-8, (k, figs["dev_" + k], figs["ref_" + k])


# ------------------------------------------------------------------------------------------------- 3. equal-weight anchor
@pytest.mark.parametrize("kernel,d,m", GRID, ids=GRID_IDS)
def test_equal_weights_are_wip_grad(kernel, d, m):
    """Without log-weights omega_z is 1 / M: wipv / wipstd and their gradients are ``GP.wip_grad``'s, up to where the division
    by M is taken."""
    gp, cand, Z, _ = _gp(kernel, d, m)
    wv, ws, dv, ds = gp.wip_grad(cand, Z)
    r = gp.wip_grad_w(cand, Z, criteria=("wipv", "wipstd"))
    assert set(r) == {"wipv", "wipstd", "dwipv", "dwipstd"}
    for val, grad, key in ((wv, dv, "wipv"), (ws, ds, "wipstd")):
        tol = 1e-10 * float(np.max(np.abs(grad)))
        print(f"{key}: value {np.max(np.abs(r[key] - val)):.3e}, gradient {np.max(np.abs(r['d' + key] - grad)):.3e}, bound {tol:.3e}")
        assert np.max(np.abs(r[key] - val)) <= tol and np.max(np.abs(r["d" + key] - grad)) <= tol


# ----------------------------------------------------------------------------------------------------------------- 4. bits
def _raw(gp, cand, c, Z, m, lw, scores, grads):
    from bobe_amd import _lib
    ps = (C.c_void_p * 4)(*[_lib.ptr(a).value for a in scores])
    pg = (C.c_void_p * 4)(*[_lib.ptr(a).value for a in grads])
    return gp._lib.bobe_gp_wip_grad_w(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std), _lib.ptr(lw), ps, pg)


def _same(a, b, keys=KEYS, row_a=slice(None), row_b=slice(None)):
    return all(same_bits(a[k][row_a], b[k][row_b]) and same_bits(a["d" + k][row_a], b["d" + k][row_b]) for k in keys)


@pytest.mark.parametrize("kernel,d,m", [GRID[0], GRID[3]], ids=[GRID_IDS[0], GRID_IDS[3]])
def test_a_candidates_bits_are_its_own(kernel, d, m):
    import torch
    gp, cand, Z, lw = _gp(kernel, d, m)
    rng = np.random.default_rng(9)
    x = cand[4:5]
    alone = gp.wip_grad_w(x, Z, log_weights=lw)
    # its place in a group of 16, and in the second of three groups
    for pos in (0, 7, 15):
        grp = rng.uniform(0.1, 0.9, size=(16, d))
        grp[pos] = x[0]
        assert _same(gp.wip_grad_w(grp, Z, log_weights=lw), alone, row_a=slice(pos, pos + 1)), pos
    big = rng.uniform(0.1, 0.9, size=(40, d))
    big[20] = x[0]
    rb = gp.wip_grad_w(big, Z, log_weights=lw)
    assert _same(rb, alone, row_a=slice(20, 21))
    assert all(np.all(np.isfinite(rb["d" + k])) for k in KEYS)
    # one criterion requested, values only, gradients only
    for k in KEYS:
        assert _same(gp.wip_grad_w(x, Z, log_weights=lw, criteria=(k,)), alone, keys=(k,)), k
    s1, g1 = np.zeros(1), np.zeros((1, d))
    assert _raw(gp, x, 1, Z, m, lw, [None, None, s1, None], [None] * 4) == 0
    assert _raw(gp, x, 1, Z, m, lw, [None] * 4, [None, None, None, g1]) == 0
    assert same_bits(s1 + gp.y_mean, alone["imiqr"]) and same_bits(g1, alone["deiv"])
    # torch device pointers, inputs and outputs
    dev = [torch.as_tensor(a, device="cuda") for a in (big, Z, lw)]
    sc = [torch.zeros(40, dtype=torch.float64, device="cuda") for _ in KEYS]
    gr = [torch.zeros((40, d), dtype=torch.float64, device="cuda") for _ in KEYS]
    assert _raw(gp, dev[0], 40, dev[1], m, dev[2], sc, gr) == 0
    torch.cuda.synchronize()
    shift = {"imiqr": gp.y_mean, "eiv": -2.0 * gp.y_mean}
    for i, k in enumerate(KEYS):
        assert same_bits(sc[i].cpu().numpy() + shift.get(k, 0.0), rb[k]) and same_bits(gr[i].cpu().numpy(), rb["d" + k]), k
    # mixed: host inputs, one device output beside host ones
    g2, s2 = torch.zeros((1, d), dtype=torch.float64, device="cuda"), np.zeros(1)
    assert _raw(gp, x, 1, Z, m, lw, [s2, None, None, None], [None, g2, None, None]) == 0
    torch.cuda.synchronize()
    assert same_bits(s2, alone["wipv"]) and same_bits(g2.cpu().numpy(), alone["dwipstd"])
    assert _same(gp.wip_grad_w(dev[0][20:21].contiguous(), dev[1], log_weights=dev[2]), alone)


def test_the_caches_change_no_bit_and_their_key_works():
    gp, cand, Z, lw = _gp("rbf", 3, 70)
    X, y, _, _, _ = _data("rbf", 3, 70)
    first = gp.wip_grad_w(cand, Z, log_weights=lw)              # fills prepare_z's cache and the per-z table
    cached = gp.wip_grad_w(cand, Z, log_weights=lw)
    assert _same(cached, first)
    # another Z and back: the first call after forget_z
    other = gp.wip_grad_w(cand, Z[::-1].copy(), log_weights=lw)
    assert not _same(other, first)
    assert _same(gp.wip_grad_w(cand, Z, log_weights=lw), first)
    # the sweep in between leaves the table alone or rebuilds it - the same bits either way
    gp.wip_sweep(cand, Z, log_weights=lw)
    assert _same(gp.wip_grad_w(cand, Z, log_weights=lw), first)
    # changed log-weights with the same Z: the result changes (and comes back)
    lw2 = lw.copy()
    lw2[3] += 2.0
    changed = gp.wip_grad_w(cand, Z, log_weights=lw2)
    assert not same_bits(changed["wipv"], first["wipv"]) and not same_bits(changed["dimiqr"], first["dimiqr"])
    fresh = make_gp(X, y, 3, NOISE, ELL, KVAR, "rbf")
    assert _same(fresh.wip_grad_w(cand, Z, log_weights=lw2), changed)
    none = gp.wip_grad_w(cand, Z)                               # weights absent after weights present
    assert _same(fresh.wip_grad_w(cand, Z), none) and not same_bits(none["wipv"], first["wipv"])
    assert _same(gp.wip_grad_w(cand, Z, log_weights=lw), first)
    # an update() in between: a refactored state drops both caches
    gp.update(np.full((1, 3), 0.123), np.array([0.4]))
    after = gp.wip_grad_w(cand, Z, log_weights=lw)
    assert not _same(after, first)
    assert _same(gp.wip_grad_w(cand, Z, log_weights=lw), after)


# ------------------------------------------------------------------------------------------------ 5. refusals and states
def test_refusals():
    from bobe_amd import GP, _lib
    gp, cand, Z, lw = _gp("rbf", 3, 70)
    s, g = np.full(9, -7.0), np.full((9, 3), -7.0)
    assert _raw(gp, cand, 9, Z, 70, lw, [None] * 4, [None] * 4) == BOBE_ERR_ARG and "criterion" in _lib.last_error()
    assert gp._lib.bobe_gp_wip_grad_w(gp._h, _lib.ptr(cand), 9, _lib.ptr(Z), 70, 1.0, None, None, None) == BOBE_ERR_ARG
    assert _raw(gp, cand, 0, Z, 70, lw, [s, None, None, None], [g, None, None, None]) == BOBE_ERR_ARG
    assert _raw(gp, cand, 9, Z, 0, lw, [s, None, None, None], [g, None, None, None]) == BOBE_ERR_ARG
    assert _raw(gp, None, 9, Z, 70, lw, [s, None, None, None], [g, None, None, None]) == BOBE_ERR_ARG
    X, y, _, _, _ = _data("rbf", 3, 70)
    bare = GP(X, y, noise=NOISE, lengthscales=np.full(3, ELL), kernel_variance=KVAR, _factor=False)
    assert _raw(bare, cand, 9, Z, 70, lw, [s, None, None, None], [g, None, None, None]) == BOBE_ERR_STATE
    assert np.all(s == -7.0) and np.all(g == -7.0)
    with pytest.raises(ValueError):
        gp.wip_grad_w(cand, Z, criteria=("ei",))
    with pytest.raises(ValueError):
        gp.wip_grad_w(cand, Z, log_weights=lw[:-1])


def test_more_training_points_than_the_chain_takes():
    from bobe_amd import GP, _lib
    from bobe_amd.acquisition import IMIQR, WIP_GRAD_W_MAX_N
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(WIP_GRAD_W_MAX_N + 1, 2))
    gp = GP(X, np.sin(3.0 * X[:, 0]) + X[:, 1], noise=1e-2, lengthscales=np.full(2, 0.3), kernel_variance=1.0)
    Z, s = rng.uniform(size=(16, 2)), np.zeros(1)
    assert _raw(gp, Z[:1], 1, Z, 16, None, [s, None, None, None], [None] * 4) == BOBE_ERR_ARG
    assert str(WIP_GRAD_W_MAX_N) in _lib.last_error()
    # the polish keeps the pool pick there
    lw = rng.normal(size=16)
    x, v = IMIQR().get_next_point(gp, acq_kwargs={"mc_points": Z, "mc_log_weights": lw, "weighted_polish": 2})
    sw = gp.wip_sweep(Z, Z, log_weights=lw, criteria=("imiqr",))
    assert np.array_equal(x, Z[sw["argmin_imiqr"]]) and same_bits(v, sw["min_imiqr"])


def test_a_nan_state_behaves_as_in_wip_grad():
    """Not positive definite under the rank test (tests/test_gpu_weighted_criteria.py's state): the status, and for the two
    scores bobe_gp_wip_grad knows the NaN-ness, are bobe_gp_wip_grad's - every fantasy variance at its floor, no gradient."""
    from bobe_amd import GP, _lib
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(40, 3))
    X[7] = X[3]
    cand, Z = rng.uniform(size=(5, 3)), rng.uniform(size=(32, 3))
    gp = GP(X, np.sin(X[:, 0]), noise=1e-30, lengthscales=np.full(3, 0.5), kernel_variance=1.0, pivot_floor_ulp=64)
    assert gp.not_pd
    old = [np.zeros(5), np.zeros(5), np.zeros((5, 3)), np.zeros((5, 3))]
    st_old = gp._lib.bobe_gp_wip_grad(gp._h, _lib.ptr(cand), 5, _lib.ptr(Z), 32, float(gp.y_std), *[_lib.ptr(a) for a in old])
    sc, gr = [np.zeros(5) for _ in KEYS], [np.zeros((5, 3)) for _ in KEYS]
    st_new = _raw(gp, cand, 5, Z, 32, None, sc, gr)
    assert st_new == st_old == 0
    for a, b in ((sc[0], old[0]), (sc[1], old[1]), (gr[0], old[2]), (gr[1], old[3])):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.allclose(a, b, rtol=1e-12, atol=0.0, equal_nan=True)


# --------------------------------------------------------------------------------------------- 6. the polish on the device
def _gauss2d(x):
    return -0.5 * ((x[0] - 0.3) ** 2 / 0.04 + (x[1] + 0.2) ** 2 / 0.09)


@functools.lru_cache(maxsize=None)
def _toy():
    rng = np.random.default_rng(21)
    X = rng.uniform(size=(60, 2))
    y = np.array([_gauss2d(2.0 * x - 1.0) for x in X])
    return X, y


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("weighted", [False, True], ids=["posterior_draws", "weights"])
@pytest.mark.parametrize("acq_name", ["IMIQR", "EIV"])
def test_polish_on_the_toy(acq_name, weighted, seed):
    from bobe_amd import acquisition as A
    X, y = _toy()
    gp = make_gp(X, y, 2, NOISE, 0.3, 2.0, "rbf")
    rng = np.random.default_rng(100 + seed)
    pool = rng.uniform(size=(400, 2))
    samples = {"x": pool, "weights": rng.uniform(0.1, 1.0, size=400), "logl": rng.normal(size=400)}
    kw = {"mc_samples": samples, "mc_points_size": 64}
    if weighted:
        kw["mc_points"], kw["mc_log_weights"] = A.get_mc_points(samples, mc_points_size=64, weighted=True)
    key = getattr(A, acq_name)._key
    # R = 0: the pool pick, and the generator where the unpolished path leaves it
    r0, r1, r8 = (np.random.default_rng(5 + seed) for _ in range(3))
    x_pool, v_pool = getattr(A, acq_name)().get_next_point(gp, acq_kwargs=dict(kw), rng=r0, verbose=False)
    x_zero, v_zero = getattr(A, acq_name)().get_next_point(gp, acq_kwargs=dict(kw, weighted_polish=0), rng=r1, verbose=False)
    assert np.array_equal(x_pool, x_zero) and same_bits(v_pool, v_zero)
    assert r0.bit_generator.state == r1.bit_generator.state
    x, v = getattr(A, acq_name)().get_next_point(gp, acq_kwargs=dict(kw, weighted_polish=8), rng=r8, verbose=False)
    assert r8.bit_generator.state == r0.bit_generator.state            # the polish draws nothing
    Zp = kw["mc_points"] if weighted else A.get_mc_points(samples, mc_points_size=64, rng=np.random.default_rng(5 + seed))
    lw = kw.get("mc_log_weights")
    at = gp.wip_sweep(np.asarray(x)[None, :], Zp, log_weights=lw, criteria=(key,))[key][0]
    print(f"{acq_name} seed {seed}: pool pick {v_pool:.6g} -> polished {v:.6g} (moved {np.max(np.abs(x - x_pool)):.3g})")
    assert v <= v_pool and np.all((x >= 0.0) & (x <= 1.0)) and x.shape == (2,)
    assert abs(v - at) <= 1e-10 * abs(at)


def test_bo_run_with_the_polish_on_weighted_nested_samples():
    from bobe_amd.bo import BOBE
    bounds = np.array([[-1.0, 1.0], [-1.0, 1.0]]).T
    kw = dict(max_evals=20, fit_n_points=4, batch_size=4, mc_points_size=32, mc_points_method="NS")
    bobe = BOBE(_gauss2d, ["x", "y"], bounds, n_sobol_init=8, seed=1, save=False)
    res = bobe.run(acq="imiqr", mc_weighted=True, weighted_polish=4, **kw)
    assert 8 < res["gp"].npoints <= 20 and all(np.isfinite(res["acq_history"]))
    assert np.all(np.isfinite(res["gp"].train_y))
