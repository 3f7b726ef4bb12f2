"""CPU-side checks of the pathwise posterior draws: the ABI declares and binds the five entry points, the consumers' new
keywords are keyword-only and default to the earlier behaviour, and the NumPy restatement (tests/paths_restatement.py) is right
where it can be checked without a device - its ensemble moments against brute-force draws and the spectral law of its
frequencies against the kernel."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from paths_restatement import (TruthLD, device_arrays, ensemble_moments, features, paths_fp64,  # noqa: E402
                               spectral_frequencies)
from posterior_restatement import kernel  # noqa: E402

SYMBOLS = ["bobe_gp_paths_create", "bobe_gp_paths_get", "bobe_gp_paths_eval", "bobe_gp_paths_argmax", "bobe_gp_paths_destroy"]


def test_header_declares_and_binding_lists_the_five_symbols():
    from bobe_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bobe_gp.h")).read()
    assert "typedef struct bobe_paths bobe_paths_t;" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound, name
    assert len(bound["bobe_gp_paths_create"][1]) == 9 and bound["bobe_gp_paths_destroy"][0] is None
    # the header says which process the paths describe
    comment = txt[:txt.index("typedef struct bobe_paths")]
    assert "LATENT" in comment[comment.rindex("/*"):]
    units = open(os.path.join(ROOT, "bobe_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\bgp_paths\b", units, flags=re.M)


def test_thompson_sampling_is_registered():
    from bobe_amd.acquisition import AcquisitionFunction, PathwiseTS
    from bobe_amd.bo import _ACQ
    assert _ACQ["ts"] is PathwiseTS and issubclass(PathwiseTS, AcquisitionFunction)
    assert set(_ACQ) == {"wipv", "wipstd", "ei", "logei", "imiqr", "eiv", "ts"}


def test_new_keywords_are_keyword_only_and_default_to_the_joint_draws():
    from bobe_amd import GP, samplers
    kw = inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(samplers.logz_from_samples).parameters
    assert p["draws_method"].kind is kw and p["draws_method"].default == "joint"
    for fn in (samplers.nested_sampling, samplers.nested_sampling_Dy):
        q = inspect.signature(fn).parameters
        assert q["logz_draws_method"].kind is kw and q["logz_draws_method"].default == "joint"
        assert list(q)[-1] == "logz_draws_method"
    g = inspect.signature(GP.sample_paths).parameters
    assert list(g)[:4] == ["self", "n_paths", "n_features", "seed"] and g["n_features"].default == 2048 and g["seed"].default == 0
    assert all(g[k].kind is kw and g[k].default is None for k in ("u", "phase", "w", "eps"))
    with pytest.raises(ValueError):
        samplers.logz_from_samples(None, None, np.zeros(3), np.zeros(3), 0.0, 0.0, draws_method="dense")


@pytest.mark.parametrize("kind", ["rbf", "matern"])
def test_ensemble_moments_agree_with_brute_force_draws(kind):
    """mean = B y and cov = G G^T + noise B B^T against 40 000 paths drawn in NumPy (6 standard errors), and the fp64 path
    against the long-double one."""
    n, d, f, s = 25, 2, 64, 40000
    rng = np.random.default_rng(1)
    X, Q = rng.uniform(size=(n, d)), rng.uniform(size=(5, d))
    y = np.sin(3 * X[:, 0]) + np.cos(2 * X[:, 1])
    ls, kvar, noise = np.full(d, 0.3 * math.sqrt(d)), 1.3, 1e-3
    u, phase = spectral_frequencies(kind, f, d, rng)
    w, eps = rng.standard_normal((s, f)), math.sqrt(noise) * rng.standard_normal((s, n))
    dr = paths_fp64(kind, X, y, Q, ls, kvar, noise, u, phase, w, eps)
    m, S = ensemble_moments(kind, X, y, Q, ls, kvar, noise, u, phase)
    assert np.all(np.abs(dr.mean(0) - m) <= 6 * np.sqrt(np.diag(S) / s))
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S ** 2) / s)
    assert np.all(np.abs(np.cov(dr, rowvar=False) - S) <= 6 * se)
    t = TruthLD(kind, X, y, ls, kvar, noise).paths(Q, u, phase, w[:50], eps[:50])
    assert float(np.max(np.abs(dr[:50] - t))) <= 1e-11 * (1.0 + float(np.max(np.abs(t))))
    cen = paths_fp64(kind, X, y, Q, ls, kvar, noise, u, phase, w[:50], eps[:50], centered=True)
    np.testing.assert_allclose(dr[:50] - cen, np.tile(m, (50, 1)), rtol=0, atol=1e-10)


@pytest.mark.parametrize("kind,d", [("rbf", 2), ("rbf", 8), ("matern", 2), ("matern", 8)])
def test_spectral_law(kind, d):
    """max |Phi Phi^T - k| <= 8 sigma^2 / sqrt(F) at 30 points with F = 65 536, for the NumPy law and for the replayed device
    draws (a wrong number of degrees of freedom or a missing 1 / ls costs >= 0.05 sigma^2 = 12.8 in these units)."""
    F, kvar = 65536, 1.3
    P = np.random.default_rng(3).uniform(size=(30, d))
    ls = np.full(d, 0.3 * math.sqrt(d))
    k = kernel(kind, P, P, ls, kvar)
    u, phase = spectral_frequencies(kind, F, d, np.random.default_rng(11))
    rep = device_arrays(17, 1, F, 1, d, kind, 1e-4)
    for uu, pp in ((u, phase), (rep["u"], rep["phase"])):
        Phi = features(P / ls, uu, pp, kvar)
        assert float(np.max(np.abs(Phi @ Phi.T - k))) <= 8.0 * kvar / math.sqrt(F)
    # the check has teeth: unscaled coordinates, or Gaussian frequencies under the Matern kernel, miss it
    assert float(np.max(np.abs(features(P, u, phase, kvar) @ features(P, u, phase, kvar).T - k))) > 8.0 * kvar / math.sqrt(F)
    if kind == "matern":
        g = np.random.default_rng(11).standard_normal((F, d))
        Phi = features(P / ls, g, phase, kvar)
        assert float(np.max(np.abs(Phi @ Phi.T - k))) > 8.0 * kvar / math.sqrt(F)


def test_device_layout_is_a_function_of_seed_row_and_column():
    a = device_arrays(5, 4, 32, 10, 3, "matern", 1e-4)
    b = device_arrays(5, 7, 48, 12, 3, "matern", 1e-4)
    assert np.array_equal(a["u"], b["u"][:32]) and np.array_equal(a["phase"], b["phase"][:32])
    assert np.array_equal(a["w"], b["w"][:4, :32]) and np.array_equal(a["eps"], b["eps"][:4, :10])
    c = device_arrays(6, 4, 32, 10, 3, "matern", 1e-4)
    assert not np.array_equal(a["w"], c["w"]) and not np.array_equal(a["w"][:, :10] * 1e-2, a["eps"])
