"""Whole HMC chains on pathwise posterior draws of the surrogate (bobe_gp_paths_hmc_run / PosteriorPaths.hmc_run /
samplers.sample_paths_hmc): one iteration replayed on the host through PosteriorPaths.value_and_grad, the invariance of a
chain's bits, the collapse to GP.hmc_run for a set without randomness, the sampled distribution against quadrature, the
classifier gate and the error contract.

Figures measured on an MI355X are in the docstrings of the tests they belong to."""
import math
import os
import sys

import numpy as np
import pytest
from scipy.special import expit

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def _gp(n, d, kernel, seed):
    """the surface of test_device_chain_iteration_replayed_on_the_host (tests/test_gpu_samplers.py)"""
    from bobe_amd import GP
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = -15.0 * np.sum((X - 0.5) ** 2, axis=1)
    return GP(X, y, noise=1e-6, kernel=kernel, lengthscales=np.linspace(0.4, 0.9, d), kernel_variance=2.0), rng


def _adapt(P, eps):
    return np.tile(np.array([eps, 0.0, 0.0, 0.0, 0.0]), (P, 1))


def _target(ps, U, idx, temp):
    """logp, dlogp/du, mean and x at the logit positions U, chain c on path idx[c]: PosteriorPaths.value_and_grad (held to a
    long-double truth by tests/test_gpu_paths_grad.py) and the logit map's Jacobian"""
    X = np.clip(expit(U), 1e-12, 1 - 1e-12)
    mean, gx = ps.value_and_grad(X, idx)
    lp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
    return lp, gx / temp * (X * (1 - X)) + (1 - 2 * X), mean, X


def _home(layout):
    if layout["streamed"]:
        return "streamed"
    return "registers+lds" if layout["lds"] else "registers"


# kernel, d, N (never a multiple of 256), F (below 256 / no multiple of 256 / several per thread), the home of the rows
REPLAY = [("rbf", 2, 203, 40, "registers"), ("matern", 6, 203, 300, "registers"), ("rbf", 6, 3701, 1024, "registers+lds"),
          ("matern", 12, 1901, 300, "registers+lds"), ("rbf", 12, 3003, 40, "streamed"), ("matern", 20, 1501, 1024, "streamed"),
          ("rbf", 20, 203, 300, "registers"), ("matern", 2, 203, 300, "registers")]
assert {c[4] for c in REPLAY} == {"registers", "registers+lds", "streamed"}
assert {c[0] for c in REPLAY} == {"rbf", "matern"} and {c[1] for c in REPLAY} == {2, 6, 12, 20}
assert {c[3] for c in REPLAY} == {40, 300, 1024} and all(c[2] % 256 for c in REPLAY)


@pytest.mark.parametrize("kernel,d,n,F,home", REPLAY, ids=[f"{k}_d{d}_N{n}_F{f}" for k, d, n, f, _ in REPLAY])
def test_one_iteration_replayed_on_the_host(kernel, d, n, F, home):
    """One iteration of bobe_gp_paths_hmc_run with its draws (momentum, L, uniform) read back: the same leapfrog steps on the
    host through PosteriorPaths.value_and_grad and the Metropolis rule must give the same acceptance probability (rel 1e-9)
    and the same next state (1e-10), the tolerances of test_device_chain_iteration_replayed_on_the_host.  S = 3 with chains
    on paths 0 and S - 1 and repeated indices, per-chain inverse masses; the case's rows live where ``home`` says
    (bobe_debug_paths_chain_layout), and the cases together cover registers only, registers + LDS and a streamed rest.

    Measured on an MI355X, largest deviation over the cases: acceptance probability rel 4.0e-11 and state 0.26 of its
    tolerance (rbf, d = 6, N = 3701, the worst-conditioned case), 1.4e-11 / 0.12 at d = 2, N = 203; every other case stays below
    2e-13 / 0.003."""
    gp, rng = _gp(n, d, kernel, seed=10 + d)
    S, P, temp, eps = 3, 24, 1.0, 0.05
    with gp.sample_paths(S, F, seed=5 + d) as ps:
        lay = ps.chain_layout()
        assert _home(lay) == home, lay
        assert lay["registers"] + lay["lds"] + lay["streamed"] == n and lay["features_per_thread"] == -(-F // 256)
        idx = rng.integers(0, S, size=P).astype(np.int64)
        idx[0], idx[1], idx[2], idx[3] = 0, S - 1, S - 1, 0
        inv_mass = rng.uniform(0.5, 2.0, size=(P, d))
        U0 = rng.normal(scale=0.5, size=(P, d))
        st = ps.hmc_state(U0, idx, temp)
        st0 = st.copy()
        g0, X0, lp0, mean0 = st0[:, d:2 * d], st0[:, 2 * d:3 * d], st0[:, 3 * d], st0[:, 3 * d + 1]
        adapt = _adapt(P, eps)
        _, _, dbg = ps.hmc_run(st, adapt, inv_mass, idx, seed=1234, it0=7, niter=1, do_adapt=False, temp=temp, debug=True)
        p0, L, r, ap = dbg[:, :d], dbg[:, d].astype(int), dbg[:, d + 1], dbg[:, d + 2]
        assert np.all((L >= 4) & (L <= 12)) and np.all((r > 0) & (r < 1))
        # the leapfrog steps of all chains side by side; a chain stops after its own L steps
        Un, pn = U0.copy(), p0 + 0.5 * eps * g0
        lpn, gn, meann, Xn = lp0.copy(), g0.copy(), mean0.copy(), X0.copy()
        for s in range(int(L.max())):
            act = L > s
            Un[act] = Un[act] + eps * inv_mass[act] * pn[act]
            lp_s, g_s, m_s, x_s = _target(ps, Un[act], idx[act], temp)
            lpn[act], gn[act], meann[act], Xn[act] = lp_s, g_s, m_s, x_s
            pn[act] = pn[act] + np.where(s < L[act] - 1, eps, 0.5 * eps)[:, None] * g_s
        h0 = lp0 - 0.5 * np.sum(p0 ** 2 * inv_mass, axis=1)
        h1 = lpn - 0.5 * np.sum(pn ** 2 * inv_mass, axis=1)
        ap_host = np.where(np.isfinite(h1), np.minimum(1.0, np.exp(np.minimum(h1 - h0, 0.0))), 0.0)
        acc = r < ap
        want = np.where(acc[:, None], np.concatenate([Un, gn, Xn, lpn[:, None], meann[:, None]], axis=1), st0)
        dev_ap = float(np.max(np.abs(ap - ap_host) / np.maximum(ap_host, 1e-300)))
        dev_st = float(np.max(np.abs(st - want) / (1e-10 + 1e-10 * np.abs(want))))
        print(f"replay {kernel} d={d} N={n} F={F} {home}: acceptance rel {dev_ap:.3g}, state {dev_st:.3g} of its tolerance; "
              f"accepted {int(acc.sum())}/{P}")
        assert 0 < acc.sum()
        for c in range(P):
            assert ap[c] == pytest.approx(ap_host[c], rel=1e-9, abs=1e-12)
        assert np.allclose(st, want, rtol=1e-10, atol=1e-10)
        assert np.array_equal(adapt[:, 0], np.full(P, eps))                     # no adaptation asked for


@pytest.mark.parametrize("kernel,d,n,F", [("rbf", 6, 203, 300), ("matern", 12, 3003, 40), ("rbf", 20, 1501, 300)])
def test_a_chains_bits_depend_on_nothing_but_its_own_inputs(kernel, d, n, F):
    """5 iterations in one launch == 3 + 2 in two launches; the first 8 chains alone == the first 8 of 24; exchanging the
    OTHER chains' path indices changes nothing - array_equal on state and adapt, with adaptation on."""
    gp, rng = _gp(n, d, kernel, seed=30 + d)
    S, P, temp, eps = 3, 24, 1.3, 0.05
    with gp.sample_paths(S, F, seed=2) as ps:
        idx = rng.integers(0, S, size=P).astype(np.int64)
        idx[:3] = (0, S - 1, 1)
        inv_mass = rng.uniform(0.5, 2.0, size=(P, d))
        st0 = ps.hmc_state(rng.normal(scale=0.5, size=(P, d)), idx, temp)
        a, b, c8, e = st0.copy(), st0.copy(), st0[:8].copy(), st0.copy()
        aa, ab, ac, ae = _adapt(P, eps), _adapt(P, eps), _adapt(8, eps), _adapt(P, eps)
        ps.hmc_run(a, aa, inv_mass, idx, 99, 0, 5, True, temp)
        ps.hmc_run(b, ab, inv_mass, idx, 99, 0, 3, True, temp)
        ps.hmc_run(b, ab, inv_mass, idx, 99, 3, 2, True, temp)
        ps.hmc_run(c8, ac, inv_mass[:8], idx[:8], 99, 0, 5, True, temp)
        other = idx.copy()
        other[8:] = (idx[8:] + 1 + np.arange(P - 8) % (S - 1)) % S
        assert np.all(other[8:] != idx[8:])
        ps.hmc_run(e, ae, inv_mass, other, 99, 0, 5, True, temp)
        assert np.array_equal(a, b) and np.array_equal(aa, ab)
        assert np.array_equal(a[:8], c8) and np.array_equal(aa[:8], ac)
        assert np.array_equal(a[:8], e[:8]) and np.array_equal(aa[:8], ae[:8]) and not np.array_equal(a[8:], e[8:])
        assert np.all(aa[:, 4] == 5) and not np.array_equal(aa[:, 0], np.full(P, eps))   # every chain adapted its step
        assert not np.array_equal(a, st0)


@pytest.mark.parametrize("kernel,d,n,F", [("rbf", 6, 203, 300), ("matern", 12, 1901, 40), ("rbf", 20, 1501, 1024)])
def test_a_set_without_randomness_collapses_to_the_mean_sampler(kernel, d, n, F):
    """w = 0 and eps = 0 make every path the posterior mean: one iteration must then agree with GP.hmc_run from the same
    state and seed (the same counter hash, hence the same momentum, L and uniform) within the replay's tolerances - a check
    that does not go through paths_grad.

    Measured on an MI355X: acceptance probability within 1.5e-13, state within 0.001 of its tolerance."""
    gp, rng = _gp(n, d, kernel, seed=50 + d)
    S, P, temp, eps = 2, 16, 1.0, 0.05
    with gp.sample_paths(S, F, seed=3, w=np.zeros((S, F)), eps=np.zeros((S, n))) as ps:
        idx = (np.arange(P) % S).astype(np.int64)
        im = rng.uniform(0.5, 2.0, size=d)
        U0 = rng.normal(scale=0.5, size=(P, d))
        X = np.clip(expit(U0), 1e-12, 1 - 1e-12)
        m, _, dm, _ = gp.predict_grad(X, mean_only=True)
        mean = m * gp.y_std + gp.y_mean
        lp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
        g = dm * gp.y_std / temp * (X * (1 - X)) + (1 - 2 * X)
        st0 = np.ascontiguousarray(np.concatenate([U0, g, X, lp[:, None], mean[:, None]], axis=1))
        a, b = st0.copy(), st0.copy()
        _, _, da = gp.hmc_run(a, _adapt(P, eps), im, seed=77, it0=3, niter=1, do_adapt=False, temp=temp, debug=True)
        _, _, db = ps.hmc_run(b, _adapt(P, eps), im, idx, seed=77, it0=3, niter=1, do_adapt=False, temp=temp, debug=True)
        assert np.array_equal(da[:, :d + 2], db[:, :d + 2])                      # momentum, L, uniform: the same draws
        print(f"collapse {kernel} d={d} N={n}: acceptance {np.max(np.abs(da[:, d + 2] - db[:, d + 2])):.3g}, "
              f"state {np.max(np.abs(a - b) / (1e-10 + 1e-10 * np.abs(a))):.3g} of its tolerance")
        for c in range(P):
            assert db[c, d + 2] == pytest.approx(da[c, d + 2], rel=1e-9, abs=1e-12)
        assert np.allclose(b, a, rtol=1e-10, atol=1e-10) and not np.array_equal(a, st0)


@pytest.mark.parametrize("kernel", ["rbf", "matern"])
@pytest.mark.parametrize("n,d", [(200, 3), (2500, 12), (1500, 20)])
def test_the_same_chain_under_both_kernels(kernel, n, d):
    """k_hmc_run and k_paths_hmc_run are the same HMC transition on two targets (the second through hmc_chain_run, the first
    written out: chain_common.hpp, consumer_kernels.hpp).  A set created with W = 0 and eps = 0 has V_c = 0, hence c_n =
    alpha_n exactly, and its feature terms add exact zeros; with every inv_mass row equal to one vector the path chain IS
    the mean chain: 4 iterations with adaptation from the same state, adapt, seed and it0.  No behaviour may belong to one
    of the two only.  Rows in registers only (200, 3), registers + LDS (2500, 12) and a streamed rest (1500, 20, where the
    two kernels keep different numbers of rows in registers but visit them in the same ascending order).

    The draws (momentum, L, uniform) must be the same bits.  State, adapt, hist and keep are NOT the same bits:
    k_paths_hmc_run spells its multiply-adds as explicit fmas, k_hmc_run leaves them to the compiler's contraction, and each
    keeps its arithmetic (a k_hmc_run built with explicit fmas gave a difference of exactly 0 in all six cases).  They are
    held to the tolerance this file and tests/test_gpu_samplers.py hold one chain iteration computed in two ways to, rtol =
    atol = 1e-10.  Measured on an MI355X, largest deviation as a fraction of that tolerance, state / adapt / hist / keep:
    rbf d = 3 0.40 / 0.13 / 0.37 / 0.25 (1e-10 absolute in the state), matern d = 3 0.040 / 0.0013 / 0.019 / 0.013, rbf
    d = 12 0.022 / 0.0015 / 0.016 / 0.011, matern d = 12 0.0037 / 0.0005 / 0.0019 / 0.0036, d = 20 below 0.009 for both
    families - the same figures before and after k_paths_hmc_run moved onto the shared body."""
    gp, rng = _gp(n, d, kernel, seed=70 + d)
    S, P, temp, eps = 2, 8, 1.0, 0.05
    with gp.sample_paths(S, 300, seed=3, w=np.zeros((S, 300)), eps=np.zeros((S, n))) as ps:
        idx = (np.arange(P) % S).astype(np.int64)
        im = rng.uniform(0.5, 2.0, size=d)
        U0 = rng.normal(scale=0.5, size=(P, d))
        X = np.clip(expit(U0), 1e-12, 1 - 1e-12)
        m, _, dm, _ = gp.predict_grad(X, mean_only=True)
        mean = m * gp.y_std + gp.y_mean
        lp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
        g = dm * gp.y_std / temp * (X * (1 - X)) + (1 - 2 * X)
        st0 = np.ascontiguousarray(np.concatenate([U0, g, X, lp[:, None], mean[:, None]], axis=1))
        a, b, aa, ab = st0.copy(), st0.copy(), _adapt(P, eps), _adapt(P, eps)
        ha, ka, da = gp.hmc_run(a, aa, im, seed=77, it0=3, niter=4, do_adapt=True, temp=temp, hist_from=0, thin=2, debug=True)
        hb, kb, db = ps.hmc_run(b, ab, np.tile(im, (P, 1)), idx, seed=77, it0=3, niter=4, do_adapt=True, temp=temp,
                                hist_from=0, thin=2, debug=True)
        assert np.array_equal(da[:, :d + 2], db[:, :d + 2])                      # momentum, L, uniform: the same draws
        for name, p, q in (("state", a, b), ("adapt", aa, ab), ("hist", ha, hb), ("keep", ka, kb)):
            print(f"same chain {kernel} d={d} N={n}: {name} differs by at most {np.max(np.abs(p - q)):.3g}, "
                  f"{np.max(np.abs(p - q) / (1e-10 + 1e-10 * np.abs(p))):.3g} of the tolerance")
            assert p.shape == q.shape and np.allclose(q, p, rtol=1e-10, atol=1e-10), name
        assert ha.shape == (4, P, d) and ka.shape == (2, P, d + 1)
        assert not np.array_equal(a, st0) and np.all(aa[:, 4] == 4) and np.all(ab[:, 4] == 4)


def _grid(G):
    g = (np.arange(G) + 0.5) / G
    a, b = np.meshgrid(g, g, indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1)


def _grid_moments(f, Q, temp):
    w = np.exp((f - f.max()) / temp)
    w /= w.sum()
    m = w @ Q
    return m, w @ (Q - m) ** 2


@pytest.mark.parametrize("temp", [1.0, 2.0])
def test_the_chains_sample_the_density_of_their_own_path(temp):
    """d = 2, N = 8, S = 4: per-path means and variances of sample_paths_hmc against midpoint quadrature of exp(f_s / temp)
    on a 256 x 256 grid of PosteriorPaths.evaluate.  Bound: 5 standard errors (from the spread of the 32 per-chain
    estimates of a path) + the grid error (the difference between the 128^2 and 256^2 grids).  The test is honest only if the
    paths' densities differ from the posterior mean's by far more than that: asserted for at least two paths at 10 standard
    errors (tests/paths_restatement.py gave, for this surface and seed, shifts of the mean of 0.05 - 0.11 at temp 1 and
    0.04 - 0.08 at temp 2 for all four paths, against standard errors of ~ 0.003).

    Measured on an MI355X: every deviation is at most 0.43 of its bound; the standard errors of the means are
    0.0016 - 0.0029, the grid errors below 5e-6, and every path's mean lies 18 - 70 standard errors from the mean's density in
    at least one coordinate (so all four paths count)."""
    from bobe_amd import GP
    from bobe_amd.samplers import sample_paths_hmc
    rng = np.random.default_rng(102)
    N, S, R, per_chain, thin = 8, 4, 32, 256, 4
    X = rng.uniform(size=(N, 2))
    y = -25.0 * np.sum((X - np.array([0.45, 0.55])) ** 2, axis=1)
    gp = GP(X, y, noise=1e-4, kernel="rbf", lengthscales=np.array([0.3, 0.35]), kernel_variance=1.0)
    with gp.sample_paths(S, 512, seed=9) as ps:
        grids = {}
        for G in (128, 256):
            Q = _grid(G)
            f = ps.evaluate(Q)
            grids[G] = [_grid_moments(f[s], Q, temp) for s in range(S)] + [_grid_moments(gp.predict_mean_batched(Q), Q, temp)]
        out = sample_paths_hmc(ps, chains_per_path=R, warmup_steps=300, num_samples=R * per_chain * thin, thinning=thin,
                               temp=temp, rng=np.random.default_rng(1))
        x = out["x"]
        assert x.shape == (S, R * per_chain, 2) and out["logp"].shape == (S, R * per_chain) and out["best"].shape == (S, 2)
        assert out["method"] == "MCMC-paths" and np.all((x > 0) & (x < 1))
        # 'logp' holds the path's own value at the sample
        pick = np.arange(0, R * per_chain, 997)
        for s in range(S):
            assert np.allclose(out["logp"][s, pick], ps.value_and_grad(x[s, pick], s)[0], rtol=1e-9, atol=1e-9)
        honest, worst = 0, 0.0
        for s in range(S):
            chains = x[s].reshape(per_chain, R, 2)                               # sample i of a path comes from chain i % R
            mean = x[s].mean(axis=0)
            se_m = chains.mean(axis=0).std(axis=0, ddof=1) / math.sqrt(R)
            v_r = ((chains - mean) ** 2).mean(axis=0)
            var, se_v = v_r.mean(axis=0), v_r.std(axis=0, ddof=1) / math.sqrt(R)
            (gm, gv), (gm2, gv2) = grids[256][s], grids[128][s]
            em, ev = np.abs(gm - gm2), np.abs(gv - gv2)
            shift = np.abs(gm - grids[256][S][0])
            honest += bool(np.any(shift > 10.0 * se_m))
            zm, zv = np.abs(mean - gm) / (5.0 * se_m + em), np.abs(var - gv) / (5.0 * se_v + ev)
            worst = max(worst, float(zm.max()), float(zv.max()))
            print(f"temp {temp} path {s}: mean {mean} grid {gm} se {se_m}; var {var} grid {gv} se {se_v}; shift from the "
                  f"mean's density {shift / se_m} se; grid error {em.max():.2g} / {ev.max():.2g}; of the bound {zm} {zv}")
            assert np.all(np.abs(mean - gm) <= 5.0 * se_m + em), (s, mean, gm, se_m)
            assert np.all(np.abs(var - gv) <= 5.0 * se_v + ev), (s, var, gv, se_v)
        assert honest >= 2, honest
        # same generator, same samples
        again = sample_paths_hmc(ps, chains_per_path=R, warmup_steps=300, num_samples=R * per_chain * thin, thinning=thin,
                                 temp=temp, rng=np.random.default_rng(1))
        assert np.array_equal(again["x"], x)


@pytest.mark.parametrize("clf_type", ["svm", "ellipsoid"])
def test_no_kept_sample_is_infeasible_under_a_gate(clf_type):
    """The parent's gate at call time applies inside k_paths_hmc_run: with the SVM gate and with the ellipsoid gate every kept
    sample is feasible and carries a mean above minus_inf; chains started outside the region (mean = minus_inf in the
    start state) move in and none ends outside.  Without the gate (use_clf off at call time: the gate is not part of the
    snapshot) the same chains do leave the region."""
    from bobe_amd.clf_gp import GPwithClassifier
    from bobe_amd.samplers import sample_paths_hmc
    rng = np.random.default_rng(5)
    d = 2
    X = rng.uniform(size=(200, d))
    y = -800.0 * np.sum((X - np.array([0.45, 0.55])) ** 2, axis=1)
    kw = {} if clf_type == "svm" else {"clf_type": "ellipsoid"}
    gp = GPwithClassifier(X, y, clf_threshold=40.0, gp_threshold=120.0, noise=1e-6, lengthscales=np.full(d, 0.3), **kw)
    assert gp.use_clf
    thr = gp.probability_threshold
    with gp.sample_paths(3, 256, seed=4) as ps:
        s = sample_paths_hmc(ps, chains_per_path=16, warmup_steps=200, num_samples=800, thinning=2, temp=4.0,
                             rng=np.random.default_rng(1))
        xs = s["x"].reshape(-1, d)
        assert s["x"].shape == (3, 400, d)
        assert np.all(gp._clf_predict_func(xs) >= thr) and np.all(s["logp"] > gp.minus_inf)
        # a hot target (temp 200) walks far: gated it stays inside, ungated it leaves
        P = 48
        x0 = np.tile(np.array([0.45, 0.55]), (P, 1)) + rng.normal(scale=0.02, size=(P, d))
        idx = (np.arange(P) % 3).astype(np.int64)
        U = np.log(x0) - np.log1p(-x0)
        st = ps.hmc_state(U, idx, 200.0)
        assert np.all(st[:, 3 * d + 1] > gp.minus_inf)
        ad = _adapt(P, 0.3)
        _, keep, _ = ps.hmc_run(st, ad, np.ones(d), idx, 3, 0, 60, False, 200.0, thin=1)
        assert np.all(gp._clf_predict_func(keep[:, :, :d].reshape(-1, d)) >= thr) and np.all(keep[:, :, d] > gp.minus_inf)
        assert np.std(keep[-1, :, :d], axis=0).max() > 0.03                     # (they did move)
        gp.use_clf = False
        st2 = ps.hmc_state(U, idx, 200.0)
        _, keep2, _ = ps.hmc_run(st2, _adapt(P, 0.3), np.ones(d), idx, 3, 0, 60, False, 200.0, thin=1)
        gp.use_clf = True
        assert np.any(gp._clf_predict_func(keep2[:, :, :d].reshape(-1, d)) < thr)
        # a start outside the region: mean = minus_inf, no gradient of the path; the chain may only move inside
        far = np.full((4, d), 0.03)
        st3 = ps.hmc_state(np.log(far) - np.log1p(-far), np.zeros(4, dtype=np.int64), 1.0)
        assert np.all(st3[:, 3 * d + 1] == gp.minus_inf)


def test_error_contract():
    """Bad P, niter, it0, temp, thin or hist_from, a NULL or out-of-range path_idx, NULL arrays, a device pointer: a negative
    status with a message, and the process goes on; a closed set raises ValueError in the wrapper."""
    import ctypes as C
    import torch
    from bobe_amd import _lib
    gp, rng = _gp(60, 3, "rbf", seed=1)
    d, S, P = 3, 2, 4
    ps = gp.sample_paths(S, 64, seed=1)
    lib, h = ps._lib, ps._h
    idx = np.array([0, 1, 1, 0], dtype=np.int64)
    st = ps.hmc_state(rng.normal(scale=0.3, size=(P, d)), idx, 1.0)
    ad, im = _adapt(P, 0.05), np.ones((P, d))
    p = lambda a: a.ctypes.data

    def call(hh=h, P_=P, idx_=p(idx), st_=p(st), ad_=p(ad), im_=p(im), it0=0, niter=2, temp=1.0, hist_from=0, hist=None,
             thin=1, keep=None):
        return lib.bobe_gp_paths_hmc_run(hh, P_, idx_, st_, ad_, im_, 1, it0, niter, 1, 1.0, 0.0, temp, hist_from, hist, thin,
                                         keep, None)

    assert call() == 0
    good = st.copy()
    for name, kw in (("P = 0", dict(P_=0)), ("P < 0", dict(P_=-3)), ("niter = 0", dict(niter=0)), ("it0 < 0", dict(it0=-1)),
                     ("temp = 0", dict(temp=0.0)), ("temp < 0", dict(temp=-1.0)), ("temp NaN", dict(temp=float("nan"))),
                     ("thin = 0", dict(thin=0)), ("hist_from < 0", dict(hist_from=-1)), ("hist_from > niter", dict(hist_from=3)),
                     ("NULL set", dict(hh=None)), ("NULL path_idx", dict(idx_=None)), ("NULL state", dict(st_=None)),
                     ("NULL adapt", dict(ad_=None)), ("NULL inv_mass", dict(im_=None))):
        assert call(**kw) < 0, name
        assert lib.bobe_last_error(), name
    for bad in (np.array([0, 1, 2, 0], dtype=np.int64), np.array([0, -1, 1, 0], dtype=np.int64)):
        assert call(idx_=p(bad)) < 0
    dev = torch.zeros(P * (3 * d + 2), dtype=torch.float64, device="cuda")
    assert call(st_=dev.data_ptr()) < 0                                          # host pointers only
    assert np.array_equal(st, good)                                              # a refused call changes nothing
    info = (C.c_int * 4)()
    assert lib.bobe_debug_paths_chain_layout(None, info) < 0 and lib.bobe_debug_paths_chain_layout(h, None) < 0
    with pytest.raises(ValueError):
        ps.hmc_run(st, ad, im, idx, 1, 0, 2, True, hist_from=5)
    with pytest.raises(_lib.BobeLibraryError):
        ps.hmc_run(st, ad, im, np.array([0, 1, 5, 0]), 1, 0, 2, True)
    with pytest.raises(_lib.BobeLibraryError):
        ps.hmc_run(st, ad, im, idx, 1, 0, 2, True, temp=0.0)
    assert call() == 0                                                           # the process goes on
    ps.close()
    with pytest.raises(ValueError):
        ps.hmc_run(st, ad, im, idx, 1, 0, 2, True)
    with pytest.raises(ValueError):
        ps.chain_layout()


def _rng_state(r):
    st = r.bit_generator.state
    return st["state"]["state"], st["state"]["inc"], st["has_uint32"], st["uinteger"]


def test_thompson_members_as_chains_on_their_paths():
    """PathwiseTS with ``ts_chain_steps``: absent or 0 the picks (and the numbers drawn from the generator) are today's, bit
    for bit; with n > 0 the picks are inside the cube, distinct, reproducible for a seeded generator, at least one is not a
    pool row, and their values are their own paths there; any mode but 'posterior' raises ValueError."""
    from bobe_amd import GP
    from bobe_amd.acquisition import PathwiseTS, _TS_DUPLICATE_TOL
    rng = np.random.default_rng(3)
    X = rng.uniform(size=(60, 2))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, 1]) + 0.1 * rng.standard_normal(60)
    gp = GP(X, y, noise=1e-4, lengthscales=np.full(2, 0.3 * math.sqrt(2)), kernel_variance=1.3)
    pool = np.random.default_rng(1).uniform(size=(700, 2))
    kw = {"candidates": pool, "ts_features": 512, "ts_mode": "posterior"}
    acq = PathwiseTS()
    r0, r1, r2 = (np.random.default_rng(42) for _ in range(3))
    pts, vals = acq.get_next_batch(gp, n_batch=6, acq_kwargs=kw, rng=r0)
    pts0, vals0 = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_chain_steps=0), rng=r1)
    assert np.array_equal(pts, pts0) and np.array_equal(vals, vals0) and _rng_state(r0) == _rng_state(r1)
    assert all(np.any(np.all(pool == p, axis=1)) for p in pts)                  # (pool rows)
    ptc, valc = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_chain_steps=20), rng=r2)
    r0.integers(0, 2 ** 62)
    assert _rng_state(r2) == _rng_state(r0)                                      # one more draw: the chains' seed
    assert ptc.shape == (6, 2) and np.all((ptc > 0.0) & (ptc < 1.0)) and np.all(np.isfinite(valc))
    dist = np.max(np.abs(ptc[:, None, :] - ptc[None, :, :]), axis=2) + np.eye(6)
    assert np.all(dist > _TS_DUPLICATE_TOL)
    moved = [not np.any(np.all(pool == p, axis=1)) for p in ptc]
    assert sum(moved) >= 1
    again, vagain = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_chain_steps=20), rng=np.random.default_rng(42))
    assert np.array_equal(again, ptc) and np.array_equal(vagain, valc)
    short, _ = acq.get_next_batch(gp, n_batch=6, acq_kwargs=dict(kw, ts_chain_steps=20, ts_chain_warmup=0),
                                  rng=np.random.default_rng(42))
    assert short.shape == (6, 2) and not np.array_equal(short, ptc)
    for bad in (dict(ts_mode="max"), dict(ts_mode="max", ts_polish=2)):
        with pytest.raises(ValueError):
            acq.get_next_batch(gp, n_batch=2, acq_kwargs=dict(kw, ts_chain_steps=5, **bad), rng=np.random.default_rng(0))
    with pytest.raises(ValueError):
        acq.get_next_batch(gp, n_batch=2, acq_kwargs={"candidates": pool, "ts_chain_steps": 5}, rng=np.random.default_rng(0))


def test_thompson_chain_picks_are_feasible_under_the_gate():
    """the deep well of tests/test_gpu_clf_gp.py: the gate admits a disc around the centre; chains started at feasible pool
    picks end feasible (the kernel never accepts an infeasible point, and the fall-back is the pool pick)"""
    from bobe_amd.acquisition import PathwiseTS
    from bobe_amd.clf import gate_eval
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, size=(120, 2))
    y = -2000.0 * np.sum((X - 0.5) ** 2, axis=1, keepdims=True)
    g = GPwithClassifier(X, y, clf_threshold=150.0, gp_threshold=400.0, noise=1e-6, lengthscales=[0.3, 0.3])
    assert g.use_clf and g._gated()
    pool = np.random.default_rng(2).uniform(size=(400, 2))
    pool = pool[gate_eval(g._lib, g._h, pool, 2)[1] > 0]
    assert 10 < len(pool) < 400
    for seed in (0, 1):
        pts, vals = PathwiseTS().get_next_batch(g, n_batch=5, acq_kwargs={"candidates": pool, "ts_features": 256,
                                                                         "ts_mode": "posterior", "ts_chain_steps": 30},
                                                rng=np.random.default_rng(seed))
        assert pts.shape == (5, 2) and np.all((pts > 0.0) & (pts < 1.0)) and np.all(np.isfinite(vals))
        assert np.all(gate_eval(g._lib, g._h, pts, 2)[1] > 0), pts
        assert np.all(vals > g.minus_inf)
        dist = np.max(np.abs(pts[:, None, :] - pts[None, :, :]), axis=2) + np.eye(5)
        assert np.all(dist > 1e-12)


def test_bo_run_with_chain_members_and_the_path_posterior():
    """BOBE.run(ts_chain_steps=n) reaches PathwiseTS; BOBE.run(path_posterior=2) returns the summary with the documented
    shapes, in physical parameters; with the option off the result has no such key, the same evaluations were made and the
    run's generator is one draw behind."""
    from bobe_amd.bo import BOBE

    def gaussian(x):
        return float(-0.5 * np.sum(((np.asarray(x) - 0.3) / 0.4) ** 2))
    bounds = np.array([[-2.0, 2.0], [-2.0, 2.0]]).T
    kw = dict(acq="ts", max_evals=20, fit_n_points=4, batch_size=2, mc_points_size=64, num_mc_samples=256,
              mc_points_method="uniform", num_hmc_warmup=100, num_hmc_samples=256, thinning=2)
    off = BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False)
    res0 = off.run(**kw)
    on = BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False)
    res2 = on.run(path_posterior=2, **kw)
    assert "path_posterior" not in res0 and set(res2) == set(res0) | {"path_posterior"}
    assert np.array_equal(res0["gp"].train_x, res2["gp"].train_x) and res0["acq_history"] == res2["acq_history"]
    off.np_rng.integers(0, 2 ** 62)
    assert _rng_state(off.np_rng) == _rng_state(on.np_rng)
    pp = res2["path_posterior"]
    assert pp["n_paths"] == 2 and pp["mean"].shape == (2, 2) and pp["cov"].shape == (2, 2, 2) and pp["std"].shape == (2, 2)
    for k in ("mean_of_means", "std_of_means", "mean_of_stds", "std_of_stds"):
        assert pp[k].shape == (2,) and np.all(np.isfinite(pp[k]))
    assert np.all(pp["mean"] > -2.0) and np.all(pp["mean"] < 2.0) and np.all(pp["std"] > 0.05)
    assert np.all(np.abs(pp["mean_of_means"] - 0.3) < 0.5) and np.all(pp["std_of_means"] > 0)
    chained = BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False)
    res3 = chained.run(ts_chain_steps=10, ts_chain_warmup=20, **kw)
    assert chained.ts_chain_steps == 10 and all(np.isfinite(res3["acq_history"]))
    tx = np.asarray(res3["gp"].train_x)
    assert 8 < len(tx) <= 20 and np.all((tx >= 0.0) & (tx <= 1.0)) and not np.array_equal(tx, res0["gp"].train_x)
    for bad in (dict(ts_chain_steps=-1), dict(path_posterior=-2), dict(ts_chain_steps=3, ts_polish=2)):
        with pytest.raises(ValueError):
            BOBE(gaussian, ["x", "y"], bounds, n_sobol_init=8, seed=2, save=False).run(**dict(kw, **bad))
