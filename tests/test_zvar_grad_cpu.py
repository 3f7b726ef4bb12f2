"""The input gradient of the evidence-variance score without a device: the formula of tests/zvar_grad_restatement.py against
central differences of ``zvar_restatement.zvar_scores`` in long double, its edge rules, and the wiring of
``bobe_gp_wip_grad_zvar`` / ``GP.wip_grad_zvar`` / ``acq_kwargs['zvar_polish']`` / ``BOBE.run(zvar_polish=)``.

The difference quotient: step 1e-7 in long double (eps 1.1e-19) leaves a truncation error O(step^2) ~ 1e-14 times the third
derivative's scale and a rounding error ~ eps |zvar| / step ~ 1e-11: the bound is 1e-8 of max |gradient| (measured <= 6.4e-10)."""
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zvar_cases as ZC  # noqa: E402
import zvar_grad_restatement as ZG  # noqa: E402
import zvar_restatement as R  # noqa: E402

N, M, D, C = 40, 23, 3, 4
NOISE, ELL, KVAR = 1e-6, 0.4, 2.0
STEP = np.longdouble(1e-7)
COMBOS = [(k, ys, w) for k in ("rbf", "matern") for ys in (1.0, 30.0, 4e3) for w in (True, False)]


def _design(y_std):
    """tests/zvar_cases.py::case_data's recipe at N = 40, M = 23, d = 3."""
    rng = np.random.default_rng(4023)
    X, cand, Z = rng.uniform(size=(N, D)), rng.uniform(size=(C, D)), rng.uniform(size=(M, D))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % D] * X[:, 3 % D] + 0.1 * rng.normal(size=N)
    lw = 1.5 * rng.normal(size=M)
    y = (y - np.mean(y)) / np.std(y) * y_std + np.mean(y)
    return X, y, cand, Z, lw


@pytest.mark.parametrize("kernel,y_std,weighted", COMBOS,
                         ids=[f"{k}-ystd{ys:g}-{'weights' if w else 'posterior_draws'}" for k, ys, w in COMBOS])
def test_gradient_is_the_central_difference_in_long_double(kernel, y_std, weighted):
    X, y, cand, Z, lw = _design(y_std)
    ys, _, std = ZC.standardise(y)
    ls, w = np.full(D, ELL), (lw if weighted else None)
    LD = np.longdouble
    got = ZG.value_and_grad(ZG.grad_state(kernel, X, ys, cand, Z, ls, KVAR, NOISE, LD), std, w)
    assert np.all(np.isfinite(got["zvar"])) and not np.any(got["const"])
    fd = np.zeros((C, D), dtype=LD)
    for j in range(D):
        e = np.zeros(D, dtype=LD)
        e[j] = STEP
        cl = np.asarray(cand, dtype=LD)
        up = R.zvar_scores(R.state(kernel, X, ys, cl + e, Z, ls, KVAR, NOISE, LD), std, w)["zvar"]
        dn = R.zvar_scores(R.state(kernel, X, ys, cl - e, Z, ls, KVAR, NOISE, LD), std, w)["zvar"]
        fd[:, j] = (up - dn) / (2 * STEP)
    err = float(np.max(np.abs(got["dzvar"] - fd)) / np.max(np.abs(fd)))
    print(f"relative disagreement with the central difference: {err:.3e}")
    assert err <= 1e-8, err
    # the value is zvar_scores' itself, and the float64 state is zvar_restatement.state's, bit for bit
    assert np.array_equal(got["zvar"], R.zvar_scores(R.state(kernel, X, ys, cand, Z, ls, KVAR, NOISE, LD), std, w)["zvar"])
    a, b = ZG.grad_state(kernel, X, ys, cand, Z, ls, KVAR, NOISE), R.state(kernel, X, ys, cand, Z, ls, KVAR, NOISE)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    f64 = ZG.value_and_grad(a, std, w)
    assert float(np.max(np.abs(f64["dzvar"] - got["dzvar"])) / np.max(np.abs(got["dzvar"]))) <= 1e-4


def _edge_state(dtype=np.float64):
    X, y, cand, Z, lw = _design(1.0)
    ys, _, std = ZC.standardise(y)
    return ZG.grad_state("rbf", X, ys, cand, Z, np.full(D, ELL), KVAR, NOISE, dtype), std, lw


def test_edge_rules_of_the_gradient():
    st, std, lw = _edge_state()
    base = ZG.value_and_grad(st, std, lw)
    ed = {k: np.array(v) for k, v in st.items()}
    ed["s"][0] = 0.0                                   # s_c not > 0: +inf and a zero gradient
    ed["s"][1] = np.nan
    ed["kcz"][2, 5] = np.inf                           # a non-finite cross: that z contributes nothing
    got = ZG.value_and_grad(ed, std, lw)
    assert np.all(np.isposinf(got["zvar"][:2])) and np.all(got["dzvar"][:2] == 0.0) and np.all(got["rho"][:2] == 0.0)
    assert np.isfinite(got["zvar"][2]) and got["rho"][2, 5] == 0.0 and got["const"][2, 5]
    # ... nothing: candidate 2's score and gradient are those of the design without that integration point's r
    keep = np.arange(M) != 5
    r2 = R.r_terms(ed, std, R.z_weights(ed, std, lw)[1])[2]
    assert r2[5] == 0.0 and np.all(np.isfinite(got["dzvar"][2]))
    assert np.all(got["rho"][2, keep] != 0.0)
    assert same(got["zvar"][3], base["zvar"][3]) and same(got["dzvar"][3], base["dzvar"][3])
    # a z forced to its cap: rho_z = 0, but it still enters T (the score moves with it)
    cp = {k: np.array(v) for k, v in st.items()}
    lam, b, _ = R.z_weights(cp, std, lw)
    cp["kcz"][3, 7] += 10.0 * np.sqrt(b[7]) * np.sqrt(cp["s"][3]) / std + abs(cp["kcz"][3, 7] - cp["G"][7, 3])
    capped = ZG.value_and_grad(cp, std, lw)
    r3 = R.r_terms(cp, std, b)[3]
    assert r3[7] == np.sqrt(b[7]) and capped["const"][3, 7] and capped["rho"][3, 7] == 0.0
    assert np.sum(capped["const"][3]) == 1 and np.all(capped["rho"][3, np.arange(M) != 7] != 0.0)
    assert np.isfinite(capped["zvar"][3]) and capped["zvar"][3] != base["zvar"][3]
    drop = {k: np.array(v) for k, v in cp.items()}
    drop["kcz"][3, 7] = np.inf                         # the same z contributing nothing: another T
    assert ZG.value_and_grad(drop, std, lw)["zvar"][3] != capped["zvar"][3]
    # the cap's z is a constant: the other z's gradient part is what differentiating them alone gives
    w1 = std / np.sqrt(cp["s"][3])
    w2 = -r3 / (2.0 * cp["s"][3])
    want = (capped["rho"][3] * w1) @ cp["dcross"][3] + np.sum(capped["rho"][3] * w2) * cp["ds"][3]
    assert np.allclose(capped["dzvar"][3], want, rtol=1e-14, atol=0.0)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_zvar_grad_wiring():
    from bobe_amd import _lib
    from bobe_amd import acquisition as A
    from bobe_amd import bo
    from bobe_amd.gp import GP
    sig = {s[0]: s for s in _lib.SIGNATURES}
    assert "bobe_gp_wip_grad_zvar" in sig and len(sig["bobe_gp_wip_grad_zvar"][2]) == 10
    with open(os.path.join(HERE, "..", "include", "bobe_gp.h")) as fh:
        assert "int bobe_gp_wip_grad_zvar(" in fh.read()
    p = inspect.signature(GP.wip_grad_zvar).parameters
    assert list(p) == ["self", "candidates", "mc_points", "log_weights"]
    assert p["log_weights"].kind is inspect.Parameter.KEYWORD_ONLY and p["log_weights"].default is None
    rp = inspect.signature(bo.BOBE.run).parameters
    assert rp["zvar_polish"].default == 0 and rp["zvar_polish"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(rp)[-2:] == ["zvar_polish", "wip_batch_mode"]
    acq = A.ZVar()
    with pytest.raises(ValueError, match="zvar_polish"):
        acq.get_next_point(None, acq_kwargs={"weighted_polish": 2})
    for bad in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match="zvar_polish"):
            acq.get_next_point(None, acq_kwargs={"zvar_polish": bad})
    assert A._zvar_polish({}) == 0 and A._zvar_polish({"zvar_polish": 16}) == 16
    assert A.ZVar._grad_entry == "bobe_gp_wip_grad_zvar" and A.IMIQR._grad_entry == "bobe_gp_wip_grad_w"
