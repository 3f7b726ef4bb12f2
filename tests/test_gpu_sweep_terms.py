"""What the acquisition sweep forms on the device on the way to its scores - V = L^-1 K(X, C), V_Z, crossT = V_Z^T V, s_c, base_z
(``bobe_debug_sweep_terms``), with the factor (``bobe_gp_get_chol``) and the inverse factor (``bobe_debug_linv``) behind them -
held to a long-double truth stage by stage, and the evidence-variance score that rests on them end to end.

Layer A (tests/sweep_terms_restatement.py): every stage is recomputed in long double FROM THE DEVICE'S OWN INPUTS of that stage
and must lie within the a-priori rounding bound of that stage alone (gamma_N times the sum of the absolute products, plus the
allowance for the device's kernel evaluation); the inverse factor, which has no componentwise bound of its own, within
rho <= 4 rho_ref + 1 of SciPy's triangular solve on the device's factor.  Every case of tests/sweep_terms_cases.py, on the path
the handle chooses, on the forced substitution (refine_kappa = 0) and on the forced product (refine_kappa < 0).

Layer B: zvar of ``GP.wip_sweep`` under tests/zvar_cases.py's rule |device - truth| <= 4 |float64 restatement - truth| +
1e-7 (1 + |truth|), the truth's argmin and log_ez to 1e-7, on the same three paths.  Printed beside it, device and float64
restatement side by side (recorded, not asserted): the worst |r - r_truth| / max_z |r_truth(c)| over the candidates and the
worst relative errors of s_c and base_z.  profiles/sweep_terms_parity.txt is this file's output on an MI355X.

Measured there: every Layer A stage of every case and path at 0.01 .. 0.23 of its bound (inverse factor rho <= 0.036, SciPy's
0.009 .. 0.021).  Layer B holds on twelve of its fifteen cases on all three paths and misses on three, on every path - 64 points
in 2-D at the draws of seed 143 (1.94e-6 where the rule allows 2.0e-7) and 145 (4.08e-7), 130 points at noise 1e-8 (3.4e-7):
strict expected failures (sweep_terms_cases.KNOWN_MISSES).  With every stage at rounding level the loss is the algorithm's, the
product with the explicit inverse factor (tests/test_sweep_terms_cpu.py reproduces it in NumPy), which the substitution's
128-row diagonal blocks are as well; DESIGN.md section 8."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sweep_terms_cases as SC  # noqa: E402
import sweep_terms_restatement as S  # noqa: E402
import zvar_cases as ZC  # noqa: E402
from batch_select_restatement import masked_argmin  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_HIP, BOBE_ERR_STATE = -1, -2, -3


def make_gp(shape, kernel, y_std, path):
    from bobe_amd import GP
    _, n, d, c, m, chunk, noise, ell, kvar = ZC.SHAPES[shape]
    X, y, cand, Z, lw = ZC.case_data(shape, y_std)
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=np.full(d, ell), kernel_variance=kvar)
    if SC.KAPPA[path] is not None:
        gp.refine_kappa = SC.KAPPA[path]
        gp.recompute_cholesky()
        assert gp.refining == (path == "substitution")
    if chunk:
        assert gp._lib.bobe_gp_set_chunk(gp._h, chunk) == 0
    assert not gp.not_pd
    return gp, np.ascontiguousarray(cand), np.ascontiguousarray(Z), lw


def device_terms(gp, cand, Z):
    """The dictionary of sweep_terms_restatement.float64_stages, from the device."""
    from bobe_amd import _lib
    n, c, m = gp.npoints, cand.shape[0], Z.shape[0]
    t = {"L": np.empty((n, n)), "Linv": np.empty((n, n)), "V": np.empty((n, c)), "VZ": np.empty((n, m)),
         "crossT": np.empty((m, c)), "sc": np.empty(c), "basez": np.empty(m), "substitution": gp.refining}
    assert gp._lib.bobe_gp_get_chol(gp._h, _lib.ptr(t["L"]), None) == 0
    assert gp._lib.bobe_debug_linv(gp._h, _lib.ptr(t["Linv"])) == 0
    rc = gp._lib.bobe_debug_sweep_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, *(_lib.ptr(t[k]) for k in
                                        ("V", "VZ", "crossT", "sc", "basez")))
    if rc == BOBE_ERR_HIP:                     # a device error: nothing more of this file is to run on that device
        pytest.exit("bobe_debug_sweep_terms: " + _lib.last_error(), returncode=3)
    assert rc == 0, _lib.last_error()
    return t


# ---------------------------------------------------------------------------------------------------- Layer A
@pytest.mark.parametrize("path", SC.PATHS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_every_stage_within_its_rounding_bound(name, path):
    shape, kernel = SC.CASES[name]
    gp, cand, Z, _ = make_gp(shape, kernel, 1.0, path)
    t = device_terms(gp, cand, Z)
    res = SC.check(name, t)
    label = "%s %s (%s)" % (name, path, "substitution" if t["substitution"] else "product")
    print("\n" + "\n".join(SC.table_lines(label, res)))
    for k in ("V", "VZ", "crossT", "sc", "basez"):
        assert np.all(np.isfinite(t[k])), k
    ratios = S.stage_ratios(res)
    assert res["inverse"]["ok"], res["inverse"]
    for k in ("V", "VZ", "crossT", "sc", "basez"):
        assert ratios[k] <= 1.0, (k, res[k])


def test_the_entry_writes_what_the_sweep_scores_from_and_only_what_is_asked():
    """The terms of a sweep reproduce its WIPV through the float64 formula; NULL outputs are skipped, the others keep their
    bits; a later sweep on the handle is what it was before the call."""
    from bobe_amd import _lib
    gp, cand, Z, _ = make_gp("tile_edge", "rbf", 1.0, "default")
    c, m = cand.shape[0], Z.shape[0]
    before = gp.wip_sweep(cand, Z)
    t = device_terms(gp, cand, Z)
    after = gp.wip_sweep(cand, Z)
    assert np.array_equal(before["wipv"], after["wipv"]) and np.array_equal(before["wipstd"], after["wipstd"])
    _, _, _, ls, kvar, noise, _ = SC.shape_args("tile_edge")
    cross = S.R.kernel("rbf", cand, Z, ls, kvar, np.float64) - t["crossT"].T
    wipv = gp.y_std ** 2 * np.mean(np.maximum(t["basez"][None, :] - cross ** 2 / t["sc"][:, None], 1e-12), axis=1)
    # (the scorer's own k(z, c) differs from NumPy's by an ulp or two of k, which 2 cross / s_c <= 2 sqrt(2 / s_c) < 3e3
    # multiplies: 1e-10 leaves a factor of ten and is seven decades below any term read from a wrong address)
    assert np.max(np.abs(wipv - before["wipv"])) <= 1e-10 * gp.y_std ** 2 * (kvar + noise)
    only = np.full((m, c), -7.0)
    assert gp._lib.bobe_debug_sweep_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, None, None, _lib.ptr(only), None, None) == 0
    assert np.array_equal(only, t["crossT"])
    assert gp._lib.bobe_debug_sweep_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, None, None, None, None, None) == 0


def test_refusals():
    from bobe_amd import GP, _lib
    gp, cand, Z, _ = make_gp("near_noise_m63", "rbf", 1.0, "default")
    c, m = cand.shape[0], Z.shape[0]
    out = np.full(c, -7.0)

    def call(h, cd, cc, zz, mm):
        return gp._lib.bobe_debug_sweep_terms(h, _lib.ptr(cd), cc, _lib.ptr(zz), mm, None, None, None, _lib.ptr(out), None)
    for args in ((None, c, Z, m), (cand, c, None, m), (cand, 0, Z, m), (cand, c, Z, 0), (cand, -1, Z, m)):
        assert call(gp._h, *args) == BOBE_ERR_ARG and _lib.last_error()
    assert call(None, cand, c, Z, m) == BOBE_ERR_ARG
    # the cap of bobe_gp_wip_select_batch's buffers: (Np + Mp + d + 1) x Cp + C doubles over 16 GiB (nothing is read before)
    too_many = (16 << 30) // 8 // (128 + 128 + 2 + 1) + 128
    assert call(gp._h, cand, too_many, Z, m) == BOBE_ERR_ARG and "16 GiB" in _lib.last_error()
    _, n, d, _, _, _, noise, ell, kvar = ZC.SHAPES["near_noise_m63"]
    X, y, _, _, _ = ZC.case_data("near_noise_m63", 1.0)
    bare = GP(X, y, noise=noise, lengthscales=np.full(d, ell), kernel_variance=kvar, _factor=False)
    assert call(bare._h, cand, c, Z, m) == BOBE_ERR_STATE
    assert np.all(out == -7.0)
    assert call(gp._h, cand, c, Z, m) == 0 and np.all(out != -7.0)


# ---------------------------------------------------------------------------------------------------- Layer B
def layer_b_params():
    for case in SC.LAYER_B:
        for path in SC.PATHS:
            marks = ()
            if case in SC.KNOWN_MISSES:
                kappa, err = SC.KNOWN_MISSES[case]
                marks = pytest.mark.xfail(strict=True, raises=AssertionError,
                                          reason="stage 'V': the product with the explicit inverse factor (on the "
                                          "substitution: its 128-row diagonal block) at (kvar + noise) / min pivot = %.1e "
                                          "leaves zvar %.2e (1 + |truth|) off; every Layer A ratio of the run is below 0.3"
                                          % (kappa, err[path]))
            yield pytest.param(case, path, marks=marks, id="%s-%s" % (ZC.case_id(case), path))


@pytest.mark.parametrize("case,path", list(layer_b_params()))
def test_zvar_holds_its_rule_on_every_path(case, path):
    shape, kernel, weighted, y_std = case
    gp, cand, Z, lw = make_gp(shape, kernel, y_std, path)
    assert abs(gp.y_std / y_std - 1) < 1e-12
    r = gp.wip_sweep(cand, Z, log_weights=lw if weighted else None, criteria=("zvar",))
    ref = ZC.sweep_reference(case)
    s64, sld, _, std = ZC.states(shape, kernel, y_std)
    ok, err, ref_err = ZC.rule(r["zvar"], ref["f64"], ref["truth"])
    lez = abs(r["log_ez"] - float(ref["log_ez"])) / (1 + abs(float(ref["log_ez"])))
    fd = S.r_figures(device_terms(gp, cand, Z), sld, std)
    ff = S.r_figures({"crossT": s64["G"], "sc": s64["s"], "basez": s64["base"]}, sld, std)
    print("\n%-46s %-12s zvar device %.3e float64 %.3e (of 1 + |truth|)  log_ez %.1e  r %.2e / %.2e  s_c %.2e / %.2e  base_z "
          "%.2e / %.2e" % (ZC.case_id(case), "substitution" if gp.refining else "product", err, ref_err, lez, fd[0], ff[0], fd[1],
                           ff[1], fd[2], ff[2]))
    assert np.all(np.isfinite(r["zvar"]))
    assert ok, (err, ref_err)
    assert r["argmin_zvar"] == masked_argmin(ref["truth"])
    assert lez <= 1e-7, lez
