"""CPU-side checks of the path sampler (samplers.sample_paths_hmc / path_posterior_summary, PathwiseTS's ``ts_chain_steps``):
the argument rules fire before any device use, the summary against NumPy, the driver's per-path pooling on a fake path set
with Gaussian targets, and the header's documentation of the new entry."""
import math
import os
import re

import numpy as np
import pytest
from scipy.special import expit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoDevice:
    """a path set whose every device entry raises: the argument checks must come first"""
    n_paths, ndim = 3, 2

    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("kw", [dict(chains_per_path=0), dict(chains_per_path=2.5), dict(temp=0.0), dict(temp=-1.0),
                                dict(temp=float("nan")), dict(warmup_steps=-1), dict(num_samples=0), dict(thinning=0),
                                dict(init=np.zeros((4, 2))), dict(init=np.zeros((3, 16, 3))), dict(init=np.zeros((2, 16, 2))),
                                dict(init=np.full((16, 2), 1.5)), dict(init=np.full((16, 2), np.nan))])
def test_sample_paths_hmc_checks_its_arguments_before_any_device_use(kw):
    from bobe_amd.samplers import sample_paths_hmc
    with pytest.raises(ValueError):
        sample_paths_hmc(_NoDevice(), **kw)


def test_the_chain_option_of_the_thompson_batches_checks_its_mode_first():
    """``ts_chain_steps`` > 0 with any mode but 'posterior' (the default 'max' included), a negative or fractional count: a
    ValueError before the pool or the GP is looked at; 0 or an absent key pass the rule."""
    from bobe_amd.acquisition import PathwiseTS, _ts_chain_steps
    acq = PathwiseTS()
    for kw in (dict(ts_chain_steps=5), dict(ts_chain_steps=5, ts_mode="max"), dict(ts_chain_steps=-1, ts_mode="posterior"),
               dict(ts_chain_steps=2.5, ts_mode="posterior"), dict(ts_chain_steps=True, ts_mode="posterior"),
               dict(ts_chain_steps=3, ts_chain_warmup=-1, ts_mode="posterior")):
        with pytest.raises(ValueError):
            acq.get_next_batch(_NoDevice(), n_batch=2, acq_kwargs=dict(kw, candidates=_NoDevice()), rng=np.random.default_rng(0))
    assert _ts_chain_steps({}, "max") == (0, 50) and _ts_chain_steps({"ts_chain_steps": 0}, "max") == (0, 50)
    assert _ts_chain_steps({"ts_chain_steps": 7, "ts_chain_warmup": 3}, "posterior") == (7, 3)


def test_path_posterior_summary_against_numpy():
    from bobe_amd.samplers import path_posterior_summary
    rng = np.random.default_rng(0)
    S, n, d = 5, 400, 3
    x = rng.uniform(size=(S, n, d)) * rng.uniform(0.2, 1.0, size=(S, 1, d))
    for arg in (x, {"x": x, "logp": np.zeros((S, n))}):
        out = path_posterior_summary(arg)
        for s in range(S):
            assert np.allclose(out["mean"][s], x[s].mean(axis=0), rtol=1e-13)
            assert np.allclose(out["cov"][s], np.cov(x[s], rowvar=False), rtol=1e-12, atol=1e-15)
            assert np.allclose(out["std"][s], x[s].std(axis=0, ddof=1), rtol=1e-12)
        means, stds = x.mean(axis=1), x.std(axis=1, ddof=1)
        assert np.allclose(out["mean_of_means"], means.mean(axis=0)) and np.allclose(out["std_of_means"], means.std(axis=0, ddof=1))
        assert np.allclose(out["mean_of_stds"], stds.mean(axis=0)) and np.allclose(out["std_of_stds"], stds.std(axis=0, ddof=1))
        assert out["n_paths"] == S
    # physical parameters: an affine map of every coordinate
    b = np.array([[-2.0, 0.0, 10.0], [2.0, 5.0, 11.0]])
    phys = path_posterior_summary(x, param_bounds=b)
    w = b[1] - b[0]
    assert np.allclose(phys["mean"], b[0] + out["mean"] * w) and np.allclose(phys["std"], out["std"] * w)
    assert np.allclose(phys["cov"], out["cov"] * w[:, None] * w[None, :]) and np.allclose(phys["std_of_means"], out["std_of_means"] * w)
    one = path_posterior_summary(x[:1])
    assert np.all(one["std_of_means"] == 0.0) and np.all(one["std_of_stds"] == 0.0)
    for bad in (x[0], x[:, :1], np.zeros((2, 3))):
        with pytest.raises(ValueError):
            path_posterior_summary(bad)
    with pytest.raises(ValueError):
        path_posterior_summary(x, param_bounds=np.zeros((3, 2)))


class _GaussianPaths:
    """A stand-in for PosteriorPaths with the kernel's contract restated in NumPy: path s is the Gaussian log-density
    -0.5 |(x - mu_s) / sig_s|^2 over the unit cube, sampled on u = logit(x) with the Jacobian; state (P, 3d+2), adapt (P, 5),
    per-chain inverse masses, 4 - 12 leapfrog steps, the chain's own dual averaging (t0 10, gamma 0.05, kappa 0.75, target
    0.8, eps in [1e-4, 2]).  Random numbers come from one NumPy generator per launch instead of the device's counter hash."""

    def __init__(self, mu, sig):
        self.mu, self.sig = np.asarray(mu, dtype=float), np.asarray(sig, dtype=float)
        self.n_paths, self.ndim = self.mu.shape
        self.inv_mass_seen = []

    def _target(self, U, idx, temp):
        X = np.clip(expit(U), 1e-12, 1 - 1e-12)
        z = (X - self.mu[idx]) / self.sig[idx]
        mean = -0.5 * np.sum(z * z, axis=1)
        lp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
        g = (-z / self.sig[idx]) / temp * (X * (1 - X)) + (1 - 2 * X)
        return lp, g, mean, X

    def hmc_state(self, U, path_index, temp=1.0):
        lp, g, mean, X = self._target(U, path_index, temp)
        return np.ascontiguousarray(np.concatenate([U, g, X, lp[:, None], mean[:, None]], axis=1))

    def hmc_run(self, state, adapt, inv_mass, path_index, seed, it0, niter, do_adapt, temp=1.0, hist_from=None, thin=0,
                debug=False):
        P, d = state.shape[0], self.ndim
        im = np.broadcast_to(np.asarray(inv_mass, dtype=float), (P, d))
        self.inv_mass_seen.append(np.array(im))
        rng = np.random.default_rng([int(seed), int(it0)])
        hist, keep = [], []
        for it in range(niter):
            U, g, lp = state[:, :d].copy(), state[:, d:2 * d].copy(), state[:, 3 * d].copy()
            eps = adapt[:, 0][:, None]
            p0 = rng.normal(size=(P, d)) / np.sqrt(im)
            L = rng.integers(4, 13, size=P)
            pn = p0 + 0.5 * eps * g
            lpn, gn, meann, Xn = lp.copy(), g.copy(), state[:, 3 * d + 1].copy(), state[:, 2 * d:3 * d].copy()
            for s in range(int(L.max())):
                act = L > s
                U[act] = U[act] + eps[act] * im[act] * pn[act]
                a, b, c, e = self._target(U[act], path_index[act], temp)
                lpn[act], gn[act], meann[act], Xn[act] = a, b, c, e
                pn[act] = pn[act] + np.where(s < L[act] - 1, 1.0, 0.5)[:, None] * eps[act] * b
            h0 = lp - 0.5 * np.sum(p0 * p0 * im, axis=1)
            h1 = lpn - 0.5 * np.sum(pn * pn * im, axis=1)
            ap = np.where(np.isfinite(h1), np.exp(np.minimum(h1 - h0, 0.0)), 0.0)
            acc = rng.uniform(size=P) < ap
            state[acc] = np.concatenate([U, gn, Xn, lpn[:, None], meann[:, None]], axis=1)[acc]
            if do_adapt:
                m = adapt[:, 4] + 1.0
                hbar = (1.0 - 1.0 / (m + 10.0)) * adapt[:, 2] + (0.8 - ap) / (m + 10.0)
                le = adapt[:, 1] - np.sqrt(m) / 0.05 * hbar
                eta = m ** -0.75
                adapt[:, 2], adapt[:, 3], adapt[:, 4] = hbar, eta * le + (1.0 - eta) * adapt[:, 3], m
                adapt[:, 0] = np.clip(np.exp(le), 1e-4, 2.0)
            if hist_from is not None and it >= hist_from:
                hist.append(state[:, :d].copy())
            if thin and (it + 1) % thin == 0:
                keep.append(np.concatenate([state[:, 2 * d:3 * d], state[:, 3 * d + 1:3 * d + 2]], axis=1))
        return (np.array(hist) if hist_from is not None else None), (np.array(keep) if thin else None), None


def test_the_drivers_per_path_pooling_recovers_gaussian_moments():
    """sample_paths_hmc on the NumPy stand-in: three Gaussian targets of different widths.  The inverse masses the driver
    hands to the sampling launch are pooled PER PATH (equal within a path, ordered like the targets' widths, restated here
    from the window's positions), a lost chain restarts from a chain of its own path, and the samples recover every
    target's mean and standard deviation."""
    from bobe_amd.samplers import _pool_paths_window, sample_paths_hmc
    mu = np.array([[0.3, 0.6], [0.5, 0.5], [0.7, 0.35]])
    sig = np.array([[0.03, 0.06], [0.08, 0.08], [0.05, 0.02]])
    fake = _GaussianPaths(mu, sig)
    S, R, d = 3, 8, 2
    init = np.clip(mu[:, None, :] + 0.02 * np.random.default_rng(5).normal(size=(S, R, d)), 0.01, 0.99)
    diag = {}
    out = sample_paths_hmc(fake, chains_per_path=R, warmup_steps=200, num_samples=1600, thinning=2, rng=np.random.default_rng(7),
                           init=init, diagnostics=diag)
    assert out["x"].shape == (S, 800, d) and out["logp"].shape == (S, 800) and out["best"].shape == (S, d)
    assert out["method"] == "MCMC-paths"
    for s in range(S):
        n_eff = 800 / 4.0                                                        # (a cautious effective sample size)
        assert np.all(np.abs(out["x"][s].mean(axis=0) - mu[s]) < 5.0 * sig[s] / math.sqrt(n_eff)), s
        assert np.allclose(out["x"][s].std(axis=0), sig[s], rtol=0.25), s
        assert np.array_equal(out["best"][s], out["x"][s][np.argmax(out["logp"][s])])
    im = diag["inv_mass"]
    assert im.shape == (S * R, d) and np.array_equal(fake.inv_mass_seen[-1], im)
    for s in range(S):
        assert np.all(im[s * R:(s + 1) * R] == im[s * R])                       # one inverse mass per path
    # logit-space spread ~ sig / (mu (1 - mu)): the pooled masses follow the targets' widths, path by path
    want = (sig / (mu * (1 - mu))) ** 2
    assert np.allclose(im[::R], want, rtol=0.6)
    assert np.all(fake.inv_mass_seen[0] == 1.0) and len(fake.inv_mass_seen) == 5   # four windows, then the sampling launch
    # the window rule itself, restated: variance of the healthy chains' recorded positions per path + 1e-3; a chain 20 + 2 d
    # below its own path's best restarts from a chain of ITS path, whatever the other paths' levels
    rng = np.random.default_rng(1)
    P = S * R
    state = rng.normal(size=(P, 3 * d + 2))
    state[:, 3 * d] = np.repeat([-5.0, -500.0, -50.0], R) + rng.uniform(0, 1, size=P)
    state[3, 3 * d] -= 100.0                                                     # lost on path 0
    state[R + 2, 3 * d] = np.nan                                                 # lost on path 1
    adapt = rng.uniform(size=(P, 5))
    hist = rng.normal(size=(6, P, d)) * np.repeat([1.0, 2.0, 3.0], R)[None, :, None]
    st0, ad0 = state.copy(), adapt.copy()
    inv_mass = np.ones((P, d))
    healthy = _pool_paths_window(state, adapt, hist, inv_mass, S, np.random.default_rng(2), True, True)
    assert list(np.flatnonzero(~healthy)) == [3, R + 2]
    for lost, s in ((3, 0), (R + 2, 1)):
        src = [c for c in range(s * R, (s + 1) * R) if c != lost and np.array_equal(state[lost], st0[c])]
        assert len(src) == 1 and np.array_equal(adapt[lost], ad0[src[0]])
    keep = np.ones(P, dtype=bool)
    keep[[3, R + 2]] = False
    assert np.array_equal(state[keep], st0[keep]) and np.array_equal(adapt[keep], ad0[keep])
    for s in range(S):
        sel = [c for c in range(s * R, (s + 1) * R) if healthy[c]]
        assert np.allclose(inv_mass[s * R:(s + 1) * R], np.var(hist[:, sel, :].reshape(-1, d), axis=0) + 1e-3, rtol=1e-13)
    # switched off: nothing moves, the masses stay
    s2, a2, m2 = st0.copy(), ad0.copy(), np.ones((P, d))
    assert np.all(_pool_paths_window(s2, a2, hist, m2, S, np.random.default_rng(2), False, False))
    assert np.array_equal(s2, st0, equal_nan=True) and np.array_equal(a2, ad0) and np.all(m2 == 1.0)


def test_the_header_documents_the_path_sampler():
    txt = open(os.path.join(ROOT, "include", "bobe_gp.h")).read()
    assert re.search(r"int bobe_gp_paths_hmc_run\(bobe_paths_t\* p, int64_t P, const int64_t\* path_idx, double\* state", txt)
    assert re.search(r"int bobe_debug_paths_chain_layout\(bobe_paths_t\* p, int\* info4\);", txt)
    comment = txt[txt.index("PATHWISE posterior draws"):txt.index("typedef struct bobe_paths bobe_paths_t;")]
    for word in ("hmc_run:", "path_idx[c]", "PER CHAIN", "[P][d]", "not part of the snapshot", "HOST memory", "BOBE_ERR_ARG",
                 "minus_inf"):
        assert word in comment, word
    from bobe_amd import _lib
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {"bobe_gp_paths_hmc_run", "bobe_debug_paths_chain_layout"} <= bound
