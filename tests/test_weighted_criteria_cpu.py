"""The algebra behind the importance-weighted criteria on the CPU (no GPU, nothing from oracle/): the closed forms of EIV and
IMIQR against Gauss-Hermite quadrature over the new observation with LITERAL (N+1)-point refits, the equal-weight anchors, the
behaviour under a constant added to the log-weights, the rank-one believer stages against literal refits, the weighted
integration points of ``get_mc_points``, and the declared surface."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky
from scipy.stats import lognorm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import weighted_criteria_restatement as W  # noqa: E402
from batch_select_restatement import kernel  # noqa: E402


def small_case(kind, seed=3, n=12, d=2, c=6, m=5, y_std=0.8):
    rng = np.random.default_rng(seed)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    ys = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=n)
    ys = (ys - ys.mean()) / ys.std()
    return X, ys, cand, Z, 1.5 * rng.normal(size=m), np.full(d, 0.5), 1.3, 1e-2, y_std


def refit(kind, X, ys, xc, ystar, Z, ls, kvar, noise):
    """Posterior mean and noise-included variance at Z of the (N+1)-point GP that gained (xc, ystar): plain factorisation."""
    X1, y1 = np.vstack([X, xc[None, :]]), np.append(ys, ystar)
    L = cholesky(kernel(kind, X1, X1, ls, kvar) + noise * np.eye(X1.shape[0]), lower=True)
    kz = kernel(kind, X1, Z, ls, kvar)
    return kz.T @ cho_solve((L, True), y1), kvar + noise - np.sum(kz * cho_solve((L, True), kz), axis=0)


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_closed_forms_against_gauss_hermite_with_literal_refits(kind):
    """EIV(c) = sum_z e^{l_z} E_y*[Var exp(f_z)] = S - R(c) and the IMIQR integrand e^{l_z} median_y*[IQR exp(f_z)] =
    e^{a_z} 2 sinh(u sqrt(v+)), y* ~ N(m_c, s_c) the predictive of the new observation.  N = 12, d = 2, M = 5; 1e-10 relative."""
    X, ys, cand, Z, lw, ls, kvar, noise, y_std = small_case(kind)
    st = W.dense_state(kind, X, ys, cand, Z, ls, kvar, noise)
    sc = W.weighted_scores(st, y_std, lw)
    mu, ell, a, _, _ = W.z_terms(st, y_std, lw)
    v = W.fantasy_var(st, y_std)
    L = cholesky(kernel(kind, X, X, ls, kvar) + noise * np.eye(X.shape[0]), lower=True)
    nodes, wts = np.polynomial.hermite.hermgauss(60)
    for c in range(cand.shape[0]):
        kc = kernel(kind, X, cand[c][None, :], ls, kvar)[:, 0]
        m_c = kc @ cho_solve((L, True), ys)
        assert abs(st["s"][c] - (kvar + noise - kc @ cho_solve((L, True), kc))) <= 1e-12
        eiv, log_iqr = 0.0, np.zeros(Z.shape[0])
        for x, wt in zip(nodes, wts):
            mean1, var1 = refit(kind, X, ys, cand[c], m_c + np.sqrt(2.0 * st["s"][c]) * x, Z, ls, kvar, noise)
            mp, vp = y_std * mean1, y_std ** 2 * var1
            np.testing.assert_allclose(vp, v[c], rtol=1e-9)             # the fantasy variance does not depend on y*
            eiv += wt / np.sqrt(np.pi) * np.sum(np.exp(lw + 2.0 * mp + vp) * np.expm1(vp))
            iqr = lognorm.ppf(0.75, s=np.sqrt(vp), scale=np.exp(mp)) - lognorm.ppf(0.25, s=np.sqrt(vp), scale=np.exp(mp))
            log_iqr += wt / np.sqrt(np.pi) * np.log(iqr)                 # log IQR is linear in y*: its mean is its median
        closed = np.exp(sc["log_s"]) - np.exp(-sc["eiv"][c])
        assert abs(eiv - closed) <= 1e-10 * abs(closed), (c, eiv, closed)
        imiqr = np.log(np.sum(np.exp(lw + log_iqr)))
        assert abs(imiqr - sc["imiqr"][c]) <= 1e-10 * (1.0 + abs(imiqr)), (c, imiqr, sc["imiqr"][c])
        # and the median itself: the refit at the predictive median y* = m_c
        mean0, var0 = refit(kind, X, ys, cand[c], m_c, Z, ls, kvar, noise)
        np.testing.assert_allclose(y_std * mean0, mu, rtol=0, atol=1e-10)
        direct = np.log(np.sum(np.exp(a) * 2.0 * np.sinh(W.U * y_std * np.sqrt(var0))))
        assert abs(direct - sc["imiqr"][c]) <= 1e-10 * (1.0 + abs(direct))


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_uniform_weights_are_the_unweighted_formulas(kind):
    X, ys, cand, Z, _, ls, kvar, noise, y_std = small_case(kind, c=40, m=9)
    st = W.dense_state(kind, X, ys, cand, Z, ls, kvar, noise)
    v = W.fantasy_var(st, y_std)
    # a_z constant: explicit weights -mu_z, and no weights at all
    for lw in (None, -y_std * st["mu"] + 0.7):
        sc = W.weighted_scores(st, y_std, lw)
        np.testing.assert_allclose(sc["wipv"], v.mean(axis=1), rtol=1e-13)
        np.testing.assert_allclose(sc["wipstd"], np.sqrt(v).mean(axis=1), rtol=1e-13)
        shift = 0.0 if lw is None else 0.7
        np.testing.assert_allclose(sc["imiqr"], shift + np.log(np.sum(2.0 * np.sinh(W.U * np.sqrt(v)), axis=1)), rtol=1e-12)
    # WIPStd is the small-sigma linearisation of IMIQR: 2 sinh(u s) -> 2 u s
    tiny = W.weighted_scores(st, 1e-4, None)
    np.testing.assert_allclose(np.exp(tiny["imiqr"]), 2.0 * W.U * Z.shape[0] * tiny["wipstd"], rtol=1e-6)


def test_a_constant_added_to_the_log_weights():
    X, ys, cand, Z, lw, ls, kvar, noise, y_std = small_case("rbf", c=50, m=11)
    st = W.dense_state("rbf", X, ys, cand, Z, ls, kvar, noise)
    a, b = W.weighted_scores(st, y_std, lw), W.weighted_scores(st, y_std, lw + 4.5)
    for key in ("wipv", "wipstd"):
        np.testing.assert_allclose(b[key], a[key], rtol=1e-13)
    np.testing.assert_allclose(b["imiqr"], a["imiqr"] + 4.5, rtol=1e-13)
    np.testing.assert_allclose(b["eiv"], a["eiv"] - 4.5, rtol=1e-13)
    assert abs(b["log_s"] - a["log_s"] - 4.5) <= 1e-12
    for key in W.KEYS:
        assert W.masked_argmin(a[key]) == W.masked_argmin(b[key])


def test_the_log_scores_do_not_saturate():
    """y_std = 4e3: 1 - exp(-v+) is 1 for every candidate, -log R(c) still orders them; everything stays finite."""
    X, ys, cand, Z, lw, ls, kvar, noise, _ = small_case("rbf", c=50, m=11)
    sc = W.weighted_scores(W.dense_state("rbf", X, ys, cand, Z, ls, kvar, noise), 4e3, lw)
    assert all(np.all(np.isfinite(sc[k])) for k in W.KEYS) and np.isfinite(sc["log_s"])
    assert len(np.unique(sc["eiv"])) == 50 and np.all(sc["eiv"] > -sc["log_s"])


@pytest.mark.parametrize("key", W.KEYS)
@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_rank_one_stages_are_the_literal_refits(kind, key):
    rng = np.random.default_rng(17)
    n, d, c, m, b = 40, 3, 200, 24, 5
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    ys = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2]
    ys = (ys - ys.mean()) / ys.std()
    lw, ls = 1.5 * rng.normal(size=m), np.full(d, 0.5)
    pl, sl, gaps = W.literal_batch(kind, X, ys, cand, Z, ls, 2.0, 1e-4, 1.7, lw, b, key)
    pr, sr = W.rank_one_batch(kind, X, ys, cand, Z, ls, 2.0, 1e-4, 1.7, lw, b, key)
    assert np.all(gaps > 1e-7), gaps
    assert pl.tolist() == pr.tolist() and len(set(pl.tolist())) == b
    np.testing.assert_allclose(sr, sl, rtol=1e-8, atol=1e-8)


def test_weighted_integration_points():
    from bobe_amd.acquisition import get_mc_points
    rng = np.random.default_rng(2)
    x, logl = rng.uniform(size=(50, 3)), rng.normal(size=50)
    w = rng.uniform(0.1, 1.0, size=50)
    w[[7, 30]] = 2.0                                            # a tie among the heaviest: by index
    w[11] = 0.0
    samples = {"x": x, "weights": w, "logl": logl}
    state = rng.bit_generator.state
    pts, lw = get_mc_points(samples, mc_points_size=8, rng=rng, weighted=True)
    assert rng.bit_generator.state == state                     # nothing drawn
    order = sorted(range(50), key=lambda i: (-w[i], i))[:8]
    assert order[:2] == [7, 30]
    assert np.array_equal(pts, x[order]) and np.array_equal(lw, np.log(w[order]) - logl[order])
    pts_all, lw_all = get_mc_points(samples, mc_points_size=64, weighted=True)
    assert pts_all.shape == (49, 3) and np.all(np.isfinite(lw_all))   # the weightless sample is left out
    with pytest.raises(ValueError):
        get_mc_points({"x": x}, mc_points_size=8, weighted=True)
    # the default draw is what it was
    g1, g2 = np.random.default_rng(5), np.random.default_rng(5)
    assert np.array_equal(get_mc_points(samples, 8, g1), x[g2.choice(50, size=8, replace=False)])


def test_declared_surface():
    from bobe_amd import EIV, IMIQR, GP, _lib
    from bobe_amd.acquisition import WeightedIntegratedPosteriorBase, get_mc_points
    from bobe_amd.bo import _ACQ, BOBE
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bobe_gp.h")).read(), flags=re.S)
    sig = {n: a for n, _, a in _lib.SIGNATURES}
    for name, nargs in (("bobe_gp_wip_sweep_w", 14), ("bobe_gp_wip_select_batch_w", 12)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt) and len(sig[name]) == nargs
        assert hasattr(_lib.load(), name)
    assert issubclass(IMIQR, WeightedIntegratedPosteriorBase) and IMIQR._key == "imiqr"
    assert issubclass(EIV, WeightedIntegratedPosteriorBase) and EIV._key == "eiv"
    assert _ACQ["imiqr"] is IMIQR and _ACQ["eiv"] is EIV
    p = inspect.signature(GP.wip_sweep).parameters
    assert list(p)[-2:] == ["log_weights", "criteria"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("log_weights", "criteria"))
    p = inspect.signature(GP.wip_select_batch_w).parameters
    assert p["log_weights"].kind is inspect.Parameter.KEYWORD_ONLY and p["log_weights"].default is None
    p = inspect.signature(get_mc_points).parameters
    assert p["weighted"].kind is inspect.Parameter.KEYWORD_ONLY and p["weighted"].default is False
    p = inspect.signature(BOBE.run).parameters
    assert p["mc_weighted"].kind is inspect.Parameter.KEYWORD_ONLY and p["mc_weighted"].default is False
