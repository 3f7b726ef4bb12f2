"""The ellipsoid feasibility classifier (BOBE/clf.py:375-472, clf_gp.py clf_type='ellipsoid') on the GPU: the gate's
values, the one-launch AdamW trainer against the test restatement (tests/ellipsoid_restatement.py), the global NumPy
stream, what the default settings learn, the gate inside every entry point, the state round trip and a BO run."""
import numpy as np
import pytest

import ellipsoid_restatement as R

pytestmark = pytest.mark.gpu


def _labels_problem(n, d, seed):
    """Points in the unit cube with 0 / 1 labels of a tilted ball around a point near the centre (both classes)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    c = 0.5 + rng.uniform(-0.1, 0.1, size=d)
    A = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    q = np.sum(((X - c) @ A) ** 2, axis=1)
    y = (q < np.quantile(q, 0.35)).astype(np.float64)
    mu = X[np.argmin(q)]
    return X, y, mu


def _theta(p):
    return np.concatenate([np.asarray(p["flat_L"], np.float64).ravel(), [float(p["alpha"]), float(p["beta"])]])


def _close(dev_params, ref_params, rel=1e-9):
    a, b = _theta(dev_params), _theta(ref_params)
    return np.max(np.abs(a - b)) <= rel * np.max(np.abs(b)), float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- 1. gate values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8, 32])
def test_gate_logits_against_the_restatement(d):
    """bobe_gp_gate_eval's logit (|L^T diff|^2, one fixed order) against the reference's L L^T einsum, 4096 points:
    |delta| <= 1e-12 (|alpha| md2 + |beta| + 1); feasibility agrees except within 1e-10 of the boundary; the probability
    is sigmoid(logit)."""
    from bobe_amd.clf import _DeviceEllipsoid
    rng = np.random.default_rng(100 + d)
    flat = rng.normal(0.0, 0.6, size=d * (d + 1) // 2)
    mu = rng.uniform(0.2, 0.8, size=d)
    alpha = 2.5
    q = rng.uniform(size=(4096, d))
    _, md2 = R.logits(flat, alpha, 0.0, mu, q)
    md2 = md2.numpy()
    beta = float(np.median(alpha * md2))                              # (half the points on either side)
    params = {"params": {"flat_L": flat, "alpha": alpha, "beta": beta}, "mu": mu}
    g = _DeviceEllipsoid(params, d, mu)
    dev = g.decision(q)
    ref = R.logits(flat, alpha, beta, mu, q)[0].numpy()
    tol = 1e-12 * (abs(alpha) * md2 + abs(beta) + 1.0)
    assert np.all(np.abs(dev - ref) <= tol), float(np.max(np.abs(dev - ref) / tol))
    p = g.proba(q)
    clear = np.abs(ref) >= 1e-10
    assert np.array_equal((p >= 0.5)[clear], (ref >= 0)[clear])
    assert 0.3 < np.mean(p >= 0.5) < 0.7
    assert np.allclose(p, 1.0 / (1.0 + np.exp(-ref)), rtol=1e-12, atol=1e-15)


def test_ellipsoid_gate_through_the_c_abi():
    """bobe_gp_set_gate_ellipsoid / bobe_gp_gate_proba as a host program calls them: the raw flat_L (the library
    transforms the diagonal), host or device pointers, NULL arguments refused, the threshold honoured, NaN infeasible,
    bobe_gp_set_gate(NULL) clears a gate of either kind."""
    import ctypes as C
    import torch
    from bobe_amd import GP, _lib
    rng = np.random.default_rng(7)
    d = 5
    X = rng.uniform(size=(60, d))
    gp = GP(X, np.sin(X.sum(1)), noise=1e-6, lengthscales=np.full(d, 0.5))
    lib, h = gp._lib, gp._h
    flat = np.ascontiguousarray(rng.normal(0, 0.5, size=15))
    mu = np.ascontiguousarray(rng.uniform(0.3, 0.7, size=d))
    q = np.ascontiguousarray(rng.uniform(size=(300, d)))
    ref = R.logits(flat, 3.0, 1.2, mu, q)[0].numpy()
    assert lib.bobe_gp_set_gate_ellipsoid(h, None, _lib.ptr(mu), 3.0, 1.2, 0.5, -1e5) < 0
    assert lib.bobe_gp_set_gate_ellipsoid(h, _lib.ptr(flat), _lib.ptr(mu), 3.0, 1.2, 0.5, -1e5) == 0
    dec, ok, pr = np.empty(300), np.empty(300), np.empty(300)
    assert lib.bobe_gp_gate_eval(h, _lib.ptr(q), 300, _lib.ptr(dec), _lib.ptr(ok)) == 0
    assert lib.bobe_gp_gate_proba(h, _lib.ptr(q), 300, _lib.ptr(pr)) == 0
    assert np.allclose(dec, ref, rtol=1e-12, atol=1e-12) and np.array_equal(ok, (pr >= 0.5).astype(float))
    assert 0 < ok.sum() < 300
    # device pointers
    fd, md = torch.from_numpy(flat).cuda(), torch.from_numpy(mu).cuda()
    assert lib.bobe_gp_set_gate_ellipsoid(h, C.c_void_p(fd.data_ptr()), C.c_void_p(md.data_ptr()), 3.0, 1.2, 0.5, -1e5) == 0
    dec2 = np.empty(300)
    assert lib.bobe_gp_gate_eval(h, _lib.ptr(q), 300, _lib.ptr(dec2), None) == 0 and np.array_equal(dec2, dec)
    m, v = gp.predict_batched(q)
    assert np.all(np.isneginf(m[ok == 0])) and np.all(v[ok == 0] == 1e-12) and np.all(np.isfinite(m[ok == 1]))
    # the threshold: a probability is in (0, 1)
    assert lib.bobe_gp_set_gate_ellipsoid(h, _lib.ptr(flat), _lib.ptr(mu), 3.0, 1.2, 0.9, -1e5) == 0
    assert lib.bobe_gp_gate_eval(h, _lib.ptr(q), 300, None, _lib.ptr(ok)) == 0
    assert np.array_equal(ok, (pr >= 0.9).astype(float))
    qn = q[:4].copy()
    qn[2, 1] = np.nan
    assert lib.bobe_gp_gate_eval(h, _lib.ptr(qn), 4, None, _lib.ptr(ok[:4])) == 0 and ok[2] == 0.0
    # NULL clears
    assert lib.bobe_gp_set_gate(h, None, 0, None, 0.0, 0.0, 0.5, -1e5) == 0
    assert np.all(np.isfinite(gp.predict_batched(q)[0]))
    assert lib.bobe_gp_gate_proba(h, _lib.ptr(q), 300, _lib.ptr(pr)) < 0 and b"no classifier gate" in lib.bobe_last_error()


# ---- 2. the trainer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 300, 1000])
@pytest.mark.parametrize("d", [2, 8, 32])
def test_trainer_against_the_restatement(n, d):
    """20 epochs, 2 restarts, the same seeds / permutations / init: every restart's parameters to 1e-9 relative and its
    loss; the same restart chosen; restart 0 warm-started from given parameters."""
    from bobe_amd import clf
    from bobe_amd.utils import set_global_seed
    X, y, mu = _labels_problem(n, d, seed=n + d)
    model = clf.EllipsoidClassifier(d=d, mu=mu, n_epochs=20)
    set_global_seed(1000 + n + d)
    best_dev, metrics = clf.train_ellipsoid_multiple_restarts(model, X, y)
    runs, best, seeds = R.train_restarts(X, y, mu, np.random.default_rng(1000 + n + d), n_epochs=20)
    for i, s in enumerate(seeds):
        p_i, m_i = clf.train_ellipsoid(model, X, y, seed=s)
        ok, err = _close(p_i["params"], runs[i][0])
        assert ok, (i, err)
        assert abs(float(m_i["train_loss"]) - runs[i][1]) <= 0.006 * runs[i][1]      # (3 significant digits)
    ok, err = _close(best_dev["params"], runs[best][0])
    assert ok, ("chosen restart", best, err)
    assert metrics == {"train_loss": f"{runs[best][1]:.2e}", "epochs": 20}
    assert np.array_equal(best_dev["mu"], mu)
    # warm start: restart 0 from given parameters (the one-launch path with one restart, and the single run)
    start = R.init_params(12345, d, 0.3)
    start["alpha"], start["beta"] = 1.7, 0.2
    seed0 = np.random.default_rng(77).integers(0, 2 ** 32 - 1)
    r0, _ = R.train_one(X, y, mu, start, seed0, n_epochs=20)
    set_global_seed(77)
    one = clf.EllipsoidClassifier(d=d, mu=mu, n_epochs=20, n_restarts=1)
    pw, _ = clf.train_ellipsoid_multiple_restarts(one, X, y, init_params={"params": start})
    p0, _ = clf.train_ellipsoid(model, X, y, seed=seed0, init_params={"params": start})
    for p in (pw, p0):
        ok, err = _close(p["params"], r0)
        assert ok, err


def test_device_loss_matches_the_restatement_closely():
    """The full-data loss itself (not only its "%.2e" string) agrees to rounding."""
    from bobe_amd import clf
    X, y, mu = _labels_problem(700, 6, seed=3)
    model = clf.EllipsoidClassifier(d=6, mu=mu, n_epochs=10)
    start = R.init_params(5, 6)
    out = clf._device_train(model, X, y, np.concatenate([start["flat_L"], [1.0, 0.0]])[None],
                            clf.ellipsoid_permutations(5, 700, 10, 64)[None])
    _, loss = R.train_one(X, y, mu, start, 5, n_epochs=10)
    assert float(out[0][1]["train_loss"]) == float(f"{loss:.2e}")


def test_restart_tie_at_three_digits_keeps_the_first():
    """A constructed tie: restart 0 starts a hair away from restart 1's own initial parameters, 0 epochs, so the two
    losses differ only beyond "%.2e" - restart 1 strictly better at full precision - and restart 0 is chosen, by the
    device path as by the restatement."""
    from bobe_amd import clf
    from bobe_amd.utils import set_global_seed
    d = 4
    X, y, mu = _labels_problem(200, d, seed=11)
    model = clf.EllipsoidClassifier(d=d, mu=mu, n_epochs=0)
    draws = np.random.default_rng(5)
    seeds = [draws.integers(0, 2 ** 32 - 1) for _ in range(2)]
    base = R.init_params(seeds[1], d)
    chosen = None
    for sign in (1.0, -1.0):
        start = dict(base, flat_L=base["flat_L"] * (1.0 + sign * 1e-6))
        l0 = float(R.bce(R.logits(start["flat_L"], 1.0, 0.0, mu, X)[0], y))
        l1 = float(R.bce(R.logits(base["flat_L"], 1.0, 0.0, mu, X)[0], y))
        if l0 > l1 and f"{l0:.2e}" == f"{l1:.2e}":
            chosen = start
            break
    assert chosen is not None
    set_global_seed(5)
    params, metrics = clf.train_ellipsoid_multiple_restarts(model, X, y, init_params={"params": chosen})
    assert np.array_equal(params["params"]["flat_L"], chosen["flat_L"])
    runs, best, _ = R.train_restarts(X, y, mu, np.random.default_rng(5), init=chosen, n_epochs=0)
    assert best == 0 and runs[0][1] > runs[1][1]


# ---- 3. the global NumPy stream ------------------------------------------------------------------------------------
def test_global_stream_advances_by_n_restarts_draws():
    from bobe_amd import clf
    from bobe_amd.utils import get_numpy_rng, set_global_seed
    X, y, mu = _labels_problem(100, 3, seed=2)
    for n_restarts in (2, 3):
        set_global_seed(21)
        clf.train_ellipsoid_classifier(X, y, {"n_epochs": 3, "n_restarts": n_restarts}, best_pt=mu)
        nxt = get_numpy_rng().integers(0, 2 ** 32 - 1)
        r = np.random.default_rng(21)
        for _ in range(n_restarts):
            r.integers(0, 2 ** 32 - 1)
        assert nxt == r.integers(0, 2 ** 32 - 1)


# ---- 4. the default settings learn the region ----------------------------------------------------------------------
def _gaussian_problem(d, seed, n=1000, n_held=2000, nsig=3.0):
    """A correlated Gaussian log-likelihood (correlation 0.6, widths 0.08) around a point near the centre; the training
    set half uniform, half drawn around the peak (as a BO run concentrates there); labels by clf_threshold = nsig^2 / 2
    below the best value seen, the held-out truth by the same level."""
    rng = np.random.default_rng(seed)
    c = np.full(d, 0.5) + rng.uniform(-0.05, 0.05, d)
    S = (0.6 * np.ones((d, d)) + 0.4 * np.eye(d)) * 0.08 ** 2
    Si = np.linalg.inv(S)

    def ll(x):
        z = x - c
        return -0.5 * np.einsum("ni,ij,nj->n", z, Si, z)

    def draw(m):
        return np.clip(np.vstack([rng.uniform(size=(m // 2, d)), rng.multivariate_normal(c, 4 * S, size=m - m // 2)]), 0, 1)
    X = draw(n)
    v = ll(X)
    thr = 0.5 * nsig ** 2
    Xh = draw(n_held)
    return X, v, thr, Xh, (ll(Xh) > v.max() - thr)


@pytest.mark.parametrize("d,min_acc,min_held", [(2, 0.98, 0.97), (6, 0.97, 0.96)])
def test_default_settings_learn_the_region(d, min_acc, min_held):
    """1000 epochs, 2 restarts (the defaults): training accuracy and agreement with the true ellipsoidal region on 2000
    held-out points (fixed seeds).  d = 2: >= 0.98 / >= 0.97.  d = 6: >= 0.97 / >= 0.96 - lowered because the centre is
    not trained: it is the best of the 1000 points, which in six dimensions lies a fraction of a width off the true
    centre, and a ball around it cannot follow the true boundary on every side.  The test restatement trained with the
    same seeds, draws and permutations gives the same numbers (0.976 / 0.9675), so this is the model's reach, not the
    device's; 18 problem variants measured 0.96-0.98 / 0.95-0.97 at d = 6."""
    from bobe_amd import clf
    from bobe_amd.utils import set_global_seed
    X, v, thr, Xh, truth = _gaussian_problem(d, seed=d)
    labels = (v > v.max() - thr).astype(np.float64)
    set_global_seed(0)
    params, metrics, proba = clf.train_ellipsoid_classifier(X, labels, None, best_pt=X[np.argmax(v)])
    assert metrics["epochs"] == 1000
    acc = np.mean((proba(X) >= 0.5) == (labels == 1))
    held = np.mean((proba(Xh) >= 0.5) == truth)
    assert acc >= min_acc and held >= min_held, (acc, held)


# ---- 5. the gate inside every entry point --------------------------------------------------------------------------
def _gated_gp(seed=11, d=3, minus_inf=-1e10):
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(150, d))
    y = -600.0 * np.sum((X - 0.5) ** 2, axis=1)
    gp = GPwithClassifier(X, y, clf_type="ellipsoid", clf_threshold=80.0, gp_threshold=160.0, noise=1e-6,
                          lengthscales=np.full(d, 0.4), minus_inf=minus_inf)
    return rng, X, y, gp


def _ref_probs(gp, q):
    p = gp.clf_params
    lg = R.logits(p["params"]["flat_L"], p["params"]["alpha"], p["params"]["beta"], p["mu"], q)[0].numpy()
    return 1.0 / (1.0 + np.exp(-lg)), lg


def test_gate_inside_every_entry_point_against_the_oracle_gate():
    """clf_gp.py:173-205 with the restatement's probabilities and the oracle's GP: predict (physical and standardised),
    the posterior gradients (zero where gated), EI / LogEI."""
    from bobe_amd import GP
    from oracle import bobe_oracle as O
    from oracle import bobe_oracle_loop as OL
    rng, X, y, gp = _gated_gp()
    assert gp.use_clf and gp.clf_type == "ellipsoid" and gp._gated()
    d = X.shape[1]
    mask = y > y.max() - 160.0
    og = O.OracleGP(X[mask], y[mask], noise=1e-6, lengthscales=np.full(d, 0.4), lengthscale_prior="DSLP")
    q = rng.uniform(size=(400, d))
    probs, lg = _ref_probs(gp, q)
    clear = np.abs(lg) >= 1e-10
    q, probs = q[clear], probs[clear]
    ok = probs >= 0.5
    assert 20 < ok.sum() < len(q) - 20
    assert np.allclose(gp._clf_predict_func(q), probs, rtol=1e-12, atol=1e-15)
    wm, wv = OL.clf_gate(og.predict_mean_batched(q), og.predict_var_batched(q), probs, 0.5, -1e10)
    gm, gv = gp.predict_mean_batched(q), gp.predict_var_batched(q)
    assert np.array_equal(gm[~ok], wm[~ok]) and np.array_equal(gv[~ok], wv[~ok])
    assert np.allclose(gm[ok], wm[ok], rtol=1e-7, atol=1e-6) and np.allclose(gv[ok], wv[ok], rtol=1e-6, atol=1e-9 * og.y_std ** 2)
    ms, vs = og.predict_batched(q)
    wm2, wv2 = OL.clf_gate(ms, vs, probs, 0.5, -1e10)
    m, v = gp.predict_batched(q)
    assert np.array_equal(m[~ok], wm2[~ok]) and np.array_equal(v[~ok], wv2[~ok])
    assert np.allclose(m[ok], wm2[ok], rtol=1e-7, atol=1e-7) and np.allclose(v[ok], wv2[ok], rtol=1e-6, atol=1e-12)
    plain = GP(X[mask], y[mask], noise=1e-6, lengthscales=np.full(d, 0.4), lengthscale_prior="DSLP")
    for mean_only in (True, False):
        a = gp.predict_grad(q, mean_only=mean_only)
        b = plain.predict_grad(q, mean_only=mean_only)
        assert np.array_equal(a[0][~ok], np.full((~ok).sum(), -1e10)) and np.array_equal(a[0][ok], b[0][ok])
        assert np.all(a[2][~ok] == 0.0) and np.array_equal(a[2][ok], b[2][ok])
        if not mean_only:
            assert np.all(a[1][~ok] == 1e-12) and np.all(a[3][~ok] == 0.0) and np.array_equal(a[3][ok], b[3][ok])
    best = float(np.max(gp.train_y))
    for log_ei in (False, True):
        got = gp.acq_ei(q, best, 0.01, log_ei=log_ei)
        want = O.log_ei_score(wm2, wv2, best, 0.01) if log_ei else O.ei_score(wm2, wv2, best, 0.01)
        assert np.allclose(got[ok], want[ok], rtol=1e-6, atol=1e-12)
        assert np.allclose(got[~ok], want[~ok], rtol=1e-9, atol=0.0) if log_ei else np.all(got[~ok] == 0.0)
    gp.use_clf = False
    assert np.allclose(gp.predict_mean_batched(q), plain.predict_mean_batched(q), atol=1e-9)
    gp.use_clf = True
    assert np.array_equal(gp.predict_mean_batched(q)[~ok], wm[~ok])


def test_gated_hmc_and_rwalk_with_the_ellipsoid():
    """hmc_leapfrog against the host-stepped path through predict_grad (whose gate is the same device function), the
    device chains inside the region, and nested sampling's random walks: no accepted point is infeasible."""
    from scipy.special import expit
    from bobe_amd import samplers
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.default_rng(5)
    d = 2
    X = rng.uniform(size=(200, d))
    y = -800.0 * np.sum((X - np.array([0.45, 0.55])) ** 2, axis=1)
    gp = GPwithClassifier(X, y, clf_type="ellipsoid", clf_threshold=40.0, gp_threshold=120.0, noise=1e-6,
                          lengthscales=np.full(d, 0.3), minus_inf=-1e10)
    assert gp.use_clf and gp._gated()
    P, L, eps = 64, 6, 0.15
    x0 = rng.uniform(0.02, 0.98, size=(P, d))
    U = np.log(x0) - np.log1p(-x0)
    inv_mass = np.ones(d)

    def host_logp_grad(Uc):
        Xc = np.clip(expit(Uc), 1e-12, 1 - 1e-12)
        m, _, dm, _ = gp.predict_grad(Xc, mean_only=True)
        bad = m <= gp.minus_inf
        mean = np.where(bad, gp.minus_inf, m * gp.y_std + gp.y_mean)
        gx = np.where(bad[:, None], 0.0, dm * gp.y_std)
        return mean + np.sum(np.log(Xc) + np.log1p(-Xc), axis=1), gx * (Xc * (1 - Xc)) + (1 - 2 * Xc), mean, Xc

    _, g0, _, _ = host_logp_grad(U)
    p0 = rng.normal(size=U.shape)
    Un, pn, lpn, gn, meann, Xn = gp.hmc_leapfrog(U, p0 + 0.5 * eps * g0, inv_mass, eps, L, 1.0)
    Uh, ph = U.copy(), p0 + 0.5 * eps * g0
    for s_ in range(L):
        Uh = Uh + eps * inv_mass * ph
        lph, gh, meanh, Xh = host_logp_grad(Uh)
        ph = ph + (eps if s_ < L - 1 else 0.5 * eps) * gh
    gated_end = meanh <= gp.minus_inf
    assert 0 < gated_end.sum() < P
    assert np.array_equal(meann <= gp.minus_inf, gated_end) and np.all(meann[gated_end] == gp.minus_inf)
    assert np.allclose(Un, Uh, rtol=1e-9, atol=1e-9) and np.allclose(lpn[~gated_end], lph[~gated_end], rtol=1e-9, atol=1e-7)
    assert np.allclose(gn, gh, rtol=1e-8, atol=1e-8)
    dev = samplers.sample_GP_NUTS(gp, np_rng=np.random.default_rng(1), num_chains=4, warmup_steps=200, num_samples=800,
                                  thinning=2)
    host = samplers.sample_GP_NUTS(gp, np_rng=np.random.default_rng(2), num_chains=4, warmup_steps=200, num_samples=800,
                                   thinning=2, fused_trajectories=False)
    for smp in (dev, host):
        assert np.all(gp._clf_predict_func(smp["x"]) >= 0.5)
        assert np.all(_ref_probs(gp, smp["x"])[1] >= -1e-10)
        assert np.all(smp["logp"] > gp.minus_inf)
    assert np.allclose(dev["x"].mean(0), host["x"].mean(0), atol=0.02)
    assert np.allclose(dev["x"].std(0), host["x"].std(0), rtol=0.25)
    # random walks: start inside the region, a threshold far below every mean - only the gate (and the cube) rejects
    inside = X[(_ref_probs(gp, X)[0] >= 0.5)][:32]
    logl = gp.predict_mean_batched(inside)
    step = 0.08 * np.eye(d)
    xw, lw, nacc, nin = gp.rwalk(inside, logl, step, float(np.min(logl)) - 1e4, 40, 9)
    assert np.all(nacc > 0) and np.all(np.isfinite(lw)) and np.all(lw > gp.minus_inf)
    assert np.all(_ref_probs(gp, xw)[1] >= -1e-10)
    assert np.sum(nacc) < np.sum(nin)                           # (some proposals inside the cube fell outside the gate)


# ---- 6. state round trip -------------------------------------------------------------------------------------------
def test_state_round_trip_restores_the_trained_gate(tmp_path, monkeypatch):
    """state_dict -> from_state_dict, save -> load and copy give bit-identical decisions without retraining; the centre
    is the trained best point, not 0.5."""
    from bobe_amd import clf_gp
    from bobe_amd.clf_gp import GPwithClassifier
    rng, X, y, gp = _gated_gp(seed=3)
    q = rng.uniform(size=(500, X.shape[1]))
    dec = gp.clf_decision(q)
    assert np.array_equal(gp.clf_params["mu"], X[np.argmax(y)]) and not np.allclose(gp.clf_params["mu"], 0.5)

    def no_training(*a, **k):
        raise AssertionError("retrained")
    monkeypatch.setitem(clf_gp._CLF_KINDS["ellipsoid"], "train", no_training)
    g2 = GPwithClassifier.from_state_dict(gp.state_dict())
    gp.save(str(tmp_path / "ell"))
    g3 = GPwithClassifier.load(str(tmp_path / "ell"))
    g4 = gp.copy()
    for g in (g2, g3, g4):
        assert g.clf_type == "ellipsoid" and g._gated()
        assert np.array_equal(g.clf_decision(q), dec)
        assert np.array_equal(g.predict_mean_batched(q), gp.predict_mean_batched(q))
    # the module-level function of the reference's load path, with the saved centre
    from bobe_amd.clf import get_ellipsoid_predict_proba_fn
    f = get_ellipsoid_predict_proba_fn(g3.clf_params, {}, X.shape[1])
    assert np.array_equal(f(q), gp._clf_predict_func(q))


# ---- 7. end to end -------------------------------------------------------------------------------------------------
def _rosenbrock(x):
    return -((1 - x[0]) ** 2 + 100 * (x[1] - x[0] ** 2) ** 2)


def test_bobe_with_the_ellipsoid_classifier(tmp_path):
    """The 2-D Rosenbrock run of test_bobe_with_classifier with clf_type='ellipsoid': it completes, its checkpoint
    reloads as an ellipsoid-gated GPwithClassifier with the same decisions."""
    from bobe_amd.bo import BOBE
    from bobe_amd.clf_gp import GPwithClassifier
    bobe = BOBE(loglikelihood=_rosenbrock, param_list=["x", "y"], param_bounds=np.array([[-2, 2], [-2, 2]]).T,
                likelihood_name="rosenbrock_ell_test", n_sobol_init=4, save=True, save_dir=str(tmp_path),
                use_clf=True, clf_type="ellipsoid", clf_use_size=10, seed=456, verbosity="WARNING")
    results = bobe.run(acq="wipstd", min_evals=20, max_evals=50, max_gp_size=50, logz_threshold=0.5, fit_n_points=6,
                       ns_n_points=12, batch_size=1)
    g = results["gp"]
    assert g.clf_type == "ellipsoid" and results["best_pt"].shape == (2,) and np.isfinite(results["best_val"])
    assert g.use_clf and g.clf_params is not None and set(g.clf_params["params"]) == {"flat_L", "alpha", "beta"}
    re = GPwithClassifier.load(str(tmp_path / "rosenbrock_ell_test_gp"))
    assert re.clf_type == "ellipsoid" and re.clf_data_size == g.clf_data_size
    q = np.random.default_rng(0).uniform(size=(200, 2))
    if re.use_clf and re.clf_params is not None:
        assert np.array_equal(re.clf_decision(q), g.clf_decision(q))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------
def test_refusals():
    from bobe_amd import clf
    from bobe_amd.clf_gp import GPwithClassifier
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(30, 33))
    with pytest.raises(ValueError, match="32"):
        GPwithClassifier(X, -np.sum(X ** 2, axis=1), clf_type="ellipsoid")
    X2 = rng.uniform(size=(30, 2))
    with pytest.raises(ValueError):
        GPwithClassifier(X2, -np.sum(X2 ** 2, axis=1), clf_type="nn")
    g = GPwithClassifier(X2, -500.0 * np.sum((X2 - 0.5) ** 2, axis=1), clf_type="Ellipsoid", clf_threshold=30.0,
                         noise=1e-6)
    assert g.clf_type == "ellipsoid"
    assert set(clf.CLASSIFIER_REGISTRY) == {"svm"}
