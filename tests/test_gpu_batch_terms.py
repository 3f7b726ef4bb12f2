"""The later stages of the one-sweep batch selection on the device - the u rows and the rank-one downdates of crossT, s_c and
base_z that ``bobe_gp_wip_select_batch`` and its ``_w`` / ``_zvar`` forms apply instead of refactorising - held to a long-double
truth: each stage alone on the device's own inputs, and the stage scores end to end against literal refits.

``bobe_debug_batch_terms`` runs the selection's own code with n_stage downdates, optionally along forced picks, and hands out the
downdated state.  The state after j downdates comes from a call with n_stage = j along the same picks (same state, same bits:
asserted), V and V_Z from ``bobe_debug_sweep_terms``.

Layer A (tests/batch_terms_restatement.py): every u row against k(., p) - V^T v* - sum u_i u_i(p) over sqrt(s_p), s_p from the
state BEFORE the stage, and every downdate against the device's own u, each within the a-priori rounding bound of that step
alone.  The cases of tests/batch_terms_cases.py along the device's own picks, two cases along forced picks (either side of
candidate 65536; the strip, tile and workgroup edges), on the path the handle chooses, the forced substitution and the forced
product.

Layer B: the stage scores of the shipped entries against the literal refit of the (N + j)-point believer surrogate in long
double under tests/zvar_cases.py's rule, |device - truth| <= 4 |float64 literal refit - truth| + 1e-7 scale (scale: |truth|
for wipv / wipstd, 1 + |truth| for the log scores), with the truth's pick at every stage under the asserted precondition that
the truth's two best unmasked scores differ by more than 1e-6.  Beside the device every stage prints what float64 NumPy
running the same recursion makes of the device's own stage-0 terms.  profiles/batch_terms_parity.txt is this file's output on
an MI355X.

Measured there.  Layer A: the u rows at 0.01 .. 0.068 of their bound, the downdates at 0.33 .. 0.50 (two roundings of the four
the bound admits), on every case and path.  Layer B: the truth's pick at every stage of every run.  Of the 34 (case, criterion)
pairs 28 hold the rule on all three paths (worst device / float64 literal refit: wipv over 63 downdates 7.0e-10 / 2.1e-10
relative, zvar over 63 downdates 1.3e-7 / 1.1e-8 of 1 + |truth|), and so does wipstd on the pool with duplicates.  Six pairs and
zvar on the duplicates miss, on every path.  Each such run is then judged by Layer A along its own picks (every ratio below 1:
asserted before the expected failure counts), and float64 NumPy on the device's stage-0 terms must miss as well
(batch_terms_cases.KNOWN_MISSES; strict expected failures that may raise ``RuleMissed`` only) - device / NumPy / float64
literal refit, worst over the stages:
  dim1 zvar, from stage 0                 1.78e-5 / 1.78e-5 / 5.7e-8   stage 0 itself: no downdate involved.  NumPy scoring the
  ill_conditioned zvar, from stage 0      2.58e-3 / 4.36e-3 / 7.2e-4   device's stage-0 terms is as far off, so the loss is put
                                                                       down to the sweep's terms (the product with the inverse
                                                                       factor of tests/sweep_terms_cases.py: inferred)
  near_noise_m65 zvar, from stage 9       4.52e-7 / 4.40e-7 / 1.5e-7   stage 0 holds the rule; its error is carried by a
  reference_noise_300 zvar, from stage 50 3.31e-7 / 2.94e-7 / 4.2e-7   recursion that shrinks base_z and s_c towards the noise
  ill_conditioned wipv, from stage 25     2.65e-7 / 2.50e-7 / 1.8e-7   (marginal where the literal refit is as far off: the rule
  ill_conditioned wipstd, from stage 30   1.32e-7 / 1.25e-7 / 9.2e-8   is per candidate; NumPy from stage 27 / 26 on wipv)
  duplicates zvar, from stage 8           4.20e-7 / 4.16e-7 / 2.7e-7
Not covered: the padding columns of the u rows (zero by k_batch_u's rule) - the entry hands its arrays out unpadded.
No kernel of the later stages is at fault."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_terms_cases as BC  # noqa: E402
import batch_terms_restatement as B  # noqa: E402
import sweep_terms_cases as SC  # noqa: E402
from batch_select_restatement import FLOOR, masked_argmin  # noqa: E402

pytestmark = pytest.mark.gpu

BOBE_ERR_ARG, BOBE_ERR_HIP, BOBE_ERR_STATE = -1, -2, -3


class RuleMissed(AssertionError):
    """Layer B's rule on the scores is missed - and nothing else: what a strict expected failure of this file may raise."""


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def make_gp(shape, kernel, path, y_std=1.0):
    from bobe_amd import GP
    X, y, cand, Z, lw = BC.case_data(shape, y_std)
    ls, kvar, noise, chunk = BC.hyper(shape)
    gp = GP(X, y, noise=noise, kernel=kernel, lengthscales=ls, kernel_variance=kvar)
    if SC.KAPPA[path] is not None:
        gp.refine_kappa = SC.KAPPA[path]
        gp.recompute_cholesky()
        assert gp.refining == (path == "substitution")
    if chunk:
        assert gp._lib.bobe_gp_set_chunk(gp._h, chunk) == 0
    assert not gp.not_pd
    return gp, np.ascontiguousarray(cand), np.ascontiguousarray(Z), np.ascontiguousarray(lw)


def batch_terms(gp, cand, Z, lw, key, n_stage, forced=None, state=True, scores=True):
    """One call of the entry: {"picks" [n_stage + 1], "scores" [(n_stage + 1) x C], "crossT", "sc", "basez", "UC", "UZ"}."""
    from bobe_amd import _lib
    c, m = cand.shape[0], Z.shape[0]
    out = {"picks": np.full(n_stage + 1, -1, dtype=np.int64), "scores": np.empty((n_stage + 1, c)) if scores else None}
    for k, shp in (("crossT", (m, c)), ("sc", (c,)), ("basez", (m,)), ("UC", (n_stage, c)), ("UZ", (n_stage, m))):
        out[k] = np.empty(shp) if state else None
    f = None if forced is None else np.ascontiguousarray(forced, dtype=np.int64)
    rc = gp._lib.bobe_debug_batch_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std), _lib.ptr(lw),
                                        B.KEYS.index(key), n_stage, _lib.ptr(f), _lib.ptr(out["crossT"]), _lib.ptr(out["sc"]),
                                        _lib.ptr(out["basez"]), _lib.ptr(out["UC"]), _lib.ptr(out["UZ"]), _lib.ptr(out["picks"]),
                                        _lib.ptr(out["scores"]))
    if rc == BOBE_ERR_HIP:                     # a device error: nothing more of this file is to run on that device
        pytest.exit("bobe_debug_batch_terms: " + _lib.last_error(), returncode=3)
    assert rc == 0, _lib.last_error()
    return out


def shipped(gp, cand, Z, lw, key, b):
    """(picks, stage scores) of the shipped entry that serves (key, lw), through the C ABI (no y_mean shift)."""
    from bobe_amd import _lib
    c, m = cand.shape[0], Z.shape[0]
    picks, stage = np.full(b, -1, dtype=np.int64), np.empty((b, c))
    head = (gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std))
    if key == "zvar":
        rc = gp._lib.bobe_gp_wip_select_batch_zvar(*head, _lib.ptr(lw), b, _lib.ptr(picks), None, _lib.ptr(stage))
    elif lw is None and key in ("wipv", "wipstd"):
        rc = gp._lib.bobe_gp_wip_select_batch(*head, b, B.KEYS.index(key), _lib.ptr(picks), None, _lib.ptr(stage))
    else:
        rc = gp._lib.bobe_gp_wip_select_batch_w(*head, _lib.ptr(lw), b, B.KEYS.index(key), _lib.ptr(picks), None,
                                                _lib.ptr(stage))
    if rc == BOBE_ERR_HIP:
        pytest.exit("batch selection: " + _lib.last_error(), returncode=3)
    assert rc == 0, _lib.last_error()
    return picks, stage


def device_terms(gp, cand, Z, lw, key, n, forced=None):
    """batch_terms_restatement.recursion's dictionary from the device: V and V_Z of bobe_debug_sweep_terms, the u rows and the
    picks of a run with n downdates, the state after j downdates from a run with n_stage = j along the same picks."""
    from bobe_amd import _lib
    nn, c, m = gp.npoints, cand.shape[0], Z.shape[0]
    V, VZ = np.empty((nn, c)), np.empty((nn, m))
    rc = gp._lib.bobe_debug_sweep_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, _lib.ptr(V), _lib.ptr(VZ), None, None, None)
    if rc == BOBE_ERR_HIP:
        pytest.exit("bobe_debug_sweep_terms: " + _lib.last_error(), returncode=3)
    assert rc == 0, _lib.last_error()
    full = batch_terms(gp, cand, Z, lw, key, n, forced)
    picks = full["picks"][:n]
    if forced is not None:
        assert picks.tolist() == list(forced)
    t = {"V": V, "VZ": VZ, "picks": picks, "UC": full["UC"], "UZ": full["UZ"], "crossT": [], "sc": [], "basez": [],
         "scores": full["scores"], "last_pick": int(full["picks"][n])}
    for j in range(n):
        part = batch_terms(gp, cand, Z, lw, key, j, picks[:j], scores=False)
        if j == n - 1:                         # same state, same bits: what makes reading stage j from its own call legitimate
            assert same_bits(part["UC"], full["UC"][:j]) and same_bits(part["UZ"], full["UZ"][:j])
            assert part["picks"].tolist() == full["picks"][:j + 1].tolist() or forced is not None
        for k in ("crossT", "sc", "basez"):
            t[k].append(part[k])
    for k in ("crossT", "sc", "basez"):
        t[k].append(full[k])
    return t


def judge(label, shape, kernel, t):
    res = BC.check(shape, kernel, t)
    print("\n" + BC.table_line(label, res))
    for k in ("UC", "UZ"):
        assert np.all(np.isfinite(t[k])), k
    for k in ("uc", "uz", "sc", "basez", "crossT"):
        assert res[k][0] <= 1.0, (k, res[k])
    return res


# ---------------------------------------------------------------------------------------------------- Layer A
@pytest.mark.parametrize("path", BC.PATHS)
@pytest.mark.parametrize("name,key", BC.LAYER_A, ids=["%s-%s" % a for a in BC.LAYER_A])
def test_every_downdate_within_its_rounding_bound(name, key, path):
    shape, kernel, weighted, y_std, bs = BC.CASES[name]
    gp, cand, Z, lw = make_gp(shape, kernel, path, y_std)
    t = device_terms(gp, cand, Z, lw if weighted else None, key, bs[key] - 1)
    judge("%s %s b=%d %s (%s)" % (name, key, bs[key], path, "substitution" if gp.refining else "product"), shape, kernel, t)


@pytest.mark.parametrize("path", BC.PATHS)
@pytest.mark.parametrize("name", list(BC.FORCED))
def test_every_downdate_along_forced_picks(name, path):
    shape, kernel, key, forced = BC.FORCED[name]
    gp, cand, Z, _ = make_gp(shape, kernel, path)
    t = device_terms(gp, cand, Z, None, key, len(forced), forced)
    judge("%s forced %s (%s)" % (name, path, "substitution" if gp.refining else "product"), shape, kernel, t)
    assert t["last_pick"] not in forced                  # the forced picks are the later argmins' mask
    assert t["last_pick"] == masked_argmin(t["scores"][-1], forced)


# ---------------------------------------------------------------------------------------------------- Layer B
def numpy_on_device_terms(gp, cand, Z, shape, kernel, y_std, lw, key, picks):
    """The stage scores that float64 NumPy running the downdate recursion makes of the DEVICE's stage-0 terms along ``picks``
    (k(z, c) and mu_z from the float64 state): where the device misses the rule and this misses it as well, the loss is the
    recursion's arithmetic (or, at stage 0, the sweep's), not a kernel's."""
    from bobe_amd import _lib
    X, y, _, _, _ = BC.case_data(shape, y_std)
    ls, kvar, noise, _ = BC.hyper(shape)
    ys, _, std = BC.ZC.standardise(y)
    nn, c, m = gp.npoints, cand.shape[0], Z.shape[0]
    t0 = {"V": np.empty((nn, c)), "VZ": np.empty((nn, m)), "crossT": np.empty((m, c)), "sc": np.empty(c), "basez": np.empty(m)}
    assert gp._lib.bobe_debug_sweep_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, *(_lib.ptr(t0[k]) for k in
                                          ("V", "VZ", "crossT", "sc", "basez"))) == 0
    t = B.recursion(kernel, X, cand, Z, ls, kvar, noise, picks[:-1], terms0=t0)
    s64 = B.R.state(kernel, X, ys, cand, Z, ls, kvar, noise, np.float64)
    return np.array([B.scores(B.state_of(t, j, s64["kcz"], s64["mu"]), std, lw, key) for j in range(len(picks))])


def stage_table(label, key, got, ref, gaps=None, numpy_rows=None):
    """Prints per stage the device's error, float64 NumPy's on the device's stage-0 terms, the float64 literal refit's and the
    gap; returns the stages at which the device misses the rule and those at which NumPy on its terms does."""
    missed, np_missed, worst = [], [], (0.0, 0.0, 0.0, 0)
    for j in range(got.shape[0]):
        ok, err, ref_err = B.rule(got[j], ref["f64"][j], ref["truth"][j], key)
        ok_np, err_np, _ = B.rule(numpy_rows[j], ref["f64"][j], ref["truth"][j], key)
        worst = max(worst, (err, err_np, ref_err, j))
        print("%-50s stage %2d  device %.3e%s  numpy on its terms %.3e%s  float64 literal %.3e  gap %s" % (
            label, j, err, " " if ok else "*", err_np, " " if ok_np else "*", ref_err,
            "%.3e" % gaps[j] if gaps is not None else "-"))
        if not ok:
            missed.append((j, err, ref_err))
        if not ok_np:
            np_missed.append((j, err_np, ref_err))
    print("%-50s all %2d stages: device worst %.3e at stage %d (numpy on its terms %.3e, float64 literal %.3e there)  smallest "
          "gap %s" % (label, got.shape[0], worst[0], worst[3], worst[1], worst[2],
                      "%.3e at stage %d" % (np.min(gaps), int(np.argmin(gaps))) if gaps is not None else "-"))
    if missed or np_missed:
        print("%-50s misses the rule from stage %s (worst %.3e), numpy on its terms from stage %s (worst %.3e)" % (
            label, missed[0][0] if missed else None, max([e[1] for e in missed], default=0.0),
            np_missed[0][0] if np_missed else None, max([e[1] for e in np_missed], default=0.0)))
    return missed, np_missed


def known_miss_mark(pair, path):
    if pair not in BC.KNOWN_MISSES:
        return ()
    stage, what, figures = BC.KNOWN_MISSES[pair]
    dev, npy, np_stage = figures[path]
    return pytest.mark.xfail(strict=True, raises=RuleMissed,
                             reason="the rule is missed from stage %d on (%s): device %.2e; float64 NumPy on the device's "
                             "stage-0 terms from stage %d on: %.2e; every Layer A ratio of the run is asserted below 1"
                             % (stage, what, dev, np_stage, npy))


def settle(pair, path, missed, np_missed, layer_a):
    """What a miss of the rule has to pass before it may count as an expected failure: Layer A along this run's own picks
    (``layer_a``: a ratio above 1 is a kernel's fault and fails the test whatever its mark); on a recorded pair, float64 NumPy
    on the device's stage-0 terms missing as well, and neither the device nor NumPy missing from an earlier stage than
    recorded.  Then ``RuleMissed``, the one thing the mark accepts."""
    if not missed:
        return
    layer_a()
    if pair in BC.KNOWN_MISSES:
        stage, _, figures = BC.KNOWN_MISSES[pair]
        assert np_missed, "the device misses the rule and float64 NumPy on its stage-0 terms does not"
        assert missed[0][0] >= stage, ("the device misses from an earlier stage than recorded", missed[0], stage)
        assert np_missed[0][0] >= min(stage, figures[path][2]), ("NumPy misses from an earlier stage", np_missed[0])
    raise RuleMissed(missed)


def layer_b_params():
    for name, key in BC.LAYER_B:
        for path in BC.PATHS:
            yield pytest.param(name, key, path, marks=known_miss_mark((name, key), path), id="%s-%s-%s" % (name, key, path))


@pytest.mark.parametrize("name,key,path", list(layer_b_params()))
def test_stage_scores_against_literal_refits(name, key, path):
    shape, kernel, weighted, y_std, bs = BC.CASES[name]
    b = bs[key]
    gp, cand, Z, lw = make_gp(shape, kernel, path, y_std)
    lw = lw if weighted else None
    assert abs(gp.y_std / y_std - 1) < 1e-12
    picks, stage = shipped(gp, cand, Z, lw, key, b)
    ref = BC.truth(name, key)
    rows = numpy_on_device_terms(gp, cand, Z, shape, kernel, y_std, lw, key, picks)
    label = "%s %s %s (%s)" % (name, key, path, "substitution" if gp.refining else "product")
    print()
    missed, np_missed = stage_table(label, key, stage, ref, ref["gaps"], rows)
    assert np.all(ref["gaps"] > BC.GAP_MIN), ref["gaps"]
    assert not np.any(np.isnan(stage))
    assert picks.tolist() == ref["picks"].tolist()
    settle((name, key), path, missed, np_missed,
           lambda: judge(label + " b=%d, Layer A of this run" % b, shape, kernel, device_terms(gp, cand, Z, lw, key, b - 1)))


@pytest.mark.parametrize("key,path", [pytest.param(k, p, marks=known_miss_mark(("duplicates", k), p), id="%s-%s" % (k, p))
                                      for k in BC.DUP_KEYS for p in BC.PATHS])
def test_a_pool_that_holds_its_picks_again(key, path):
    """Exact and 1e-7-shifted copies of the truth's first four picks stand in the pool: a copy ties with its original, so the
    truth runs along the device's picks, each of which must score within 1e-9 of the truth's best (relative; the log score's
    difference).  After its original is picked a copy's s_c is about 2 noise: positive and finite.  The rule on the scores is
    settled last: everything above it holds where the rule is a known miss as well."""
    gp, cand, Z, _ = make_gp("duplicates", "rbf", path)
    pool, originals = BC.duplicates_pool()
    c0 = cand.shape[0] - 2 * len(originals)
    picks, stage = shipped(gp, cand, Z, None, key, BC.DUP_B)
    truth, f64, _ = BC.duplicates_truth(key, tuple(picks.tolist()))
    rows = numpy_on_device_terms(gp, cand, Z, "duplicates", "rbf", 1.0, None, key, picks)
    label = "duplicates %s %s (%s)" % (key, path, "substitution" if gp.refining else "product")
    print()
    missed, np_missed = stage_table(label, key, stage, {"truth": truth, "f64": f64}, None, rows)
    for j, p in enumerate(picks):
        v = np.array(truth[j], dtype=np.longdouble)
        v[picks[:j]] = np.inf
        best = np.min(v)
        excess = float(v[p] - best) if key in B.LOG_KEYS else float((v[p] - best) / abs(best))
        assert excess <= BC.DUP_TOL, ("pick", j, int(p), excess)
    t = device_terms(gp, cand, Z, None, key, BC.DUP_B - 1)
    judge(label, "duplicates", "rbf", t)
    _, _, noise, _ = BC.hyper("duplicates")
    taken = set(picks.tolist())
    for i, p in enumerate(originals):
        group = {int(p), c0 + 2 * i, c0 + 2 * i + 1}
        if group & taken:                                # one of the three went: the two others sit at about 2 noise
            left = sorted(group - taken)
            s = t["sc"][-1][left]
            print("%s: s_c of the copies of %d after the batch: %s" % (label, p, s))
            assert np.all(np.isfinite(s)) and np.all(s > 0) and np.all(s < 1e3 * noise), ("copies", p, s)
    assert any({int(p), c0 + 2 * i, c0 + 2 * i + 1} & taken for i, p in enumerate(originals))
    settle(("duplicates", key), path, missed, np_missed, lambda: None)          # (Layer A of this run: judged above)


# ---------------------------------------------------------------------------------------------------- the entry itself
@pytest.mark.parametrize("key,weighted", [("wipv", False), ("wipstd", False), ("wipstd", True), ("imiqr", False), ("eiv", True),
                                          ("zvar", True)])
def test_the_entry_is_the_shipped_selection_bit_for_bit(key, weighted):
    """With forced equal to the shipped entry's own picks, and with none, the stage scores are the shipped entry's bits; the
    handle is left alone."""
    gp, cand, Z, lw = make_gp("tile_edge", "rbf", "default")
    lw = lw if weighted else None
    before = gp.wip_sweep(cand, Z)
    picks, stage = shipped(gp, cand, Z, lw, key, 9)
    free = batch_terms(gp, cand, Z, lw, key, 8)
    forced = batch_terms(gp, cand, Z, lw, key, 8, picks[:8])
    for r in (free, forced):
        assert same_bits(r["scores"], stage) and r["picks"].tolist() == picks.tolist()
    for k in ("crossT", "sc", "basez", "UC", "UZ"):
        assert same_bits(free[k], forced[k]), k
    only = batch_terms(gp, cand, Z, lw, key, 8, state=False)
    assert same_bits(only["scores"], stage)
    after = gp.wip_sweep(cand, Z)
    assert same_bits(before["wipv"], after["wipv"]) and same_bits(before["wipstd"], after["wipstd"])
    assert same_bits(shipped(gp, cand, Z, lw, key, 9)[1], stage)


@pytest.mark.parametrize("shape,kernel", [("tile_edge", "rbf"), ("cand_is_z", "matern"), ("ragged_4chunks", "rbf")])
def test_without_a_downdate_the_entry_is_the_sweep_terms_entry(shape, kernel):
    from bobe_amd import _lib
    gp, cand, Z, lw = make_gp(shape, kernel, "default")
    c, m = cand.shape[0], Z.shape[0]
    x, s, bz = np.empty((m, c)), np.empty(c), np.empty(m)
    assert gp._lib.bobe_debug_sweep_terms(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, None, None, _lib.ptr(x), _lib.ptr(s),
                                          _lib.ptr(bz)) == 0
    for key, w in (("wipstd", None), ("eiv", lw), ("zvar", None)):
        r = batch_terms(gp, cand, Z, w, key, 0)
        assert same_bits(r["crossT"], x) and same_bits(r["sc"], s) and same_bits(r["basez"], bz), key
        assert r["UC"].shape == (0, c) and r["picks"][0] == masked_argmin(r["scores"][0])


def test_refusals():
    from bobe_amd import GP, _lib
    gp, cand, Z, _ = make_gp("near_noise_m63", "rbf", "default")
    c, m = cand.shape[0], Z.shape[0]
    sc, picks = np.full(c, -7.0), np.full(64, -7, dtype=np.int64)

    def call(h=gp._h, cd=cand, cc=c, zz=Z, mm=m, crit=1, n_stage=3, forced=None):
        f = None if forced is None else np.ascontiguousarray(forced, dtype=np.int64)
        return gp._lib.bobe_debug_batch_terms(h, _lib.ptr(cd), cc, _lib.ptr(zz), mm, 1.0, None, crit, n_stage, _lib.ptr(f), None,
                                              _lib.ptr(sc), None, None, None, _lib.ptr(picks), None)
    bad = [dict(cd=None), dict(zz=None), dict(cc=0), dict(mm=0), dict(cc=-1), dict(h=None), dict(crit=-1), dict(crit=5),
           dict(n_stage=-1), dict(n_stage=64), dict(n_stage=c), dict(forced=[0, 1, c]), dict(forced=[0, -1, 2]),
           dict(forced=[5, 1, 5])]
    for kw in bad:
        assert call(**kw) == BOBE_ERR_ARG and _lib.last_error(), kw
    # bobe_gp_wip_select_batch's cap at n_batch = n_stage + 1 (nothing is read before)
    too_many = (16 << 30) // 8 // (128 + 128 + 2 + 1 + 1 + 3 + 1) + 128
    assert call(cc=too_many) == BOBE_ERR_ARG and "16 GiB" in _lib.last_error()
    X, y, _, _, _ = BC.case_data("near_noise_m63")
    ls, kvar, noise, _ = BC.hyper("near_noise_m63")
    bare = GP(X, y, noise=noise, lengthscales=ls, kernel_variance=kvar, _factor=False)
    assert call(h=bare._h) == BOBE_ERR_STATE
    assert np.all(sc == -7.0) and np.all(picks == -7)
    assert call(forced=[5, 1, 7]) == 0 and np.all(sc != -7.0) and picks[:3].tolist() == [5, 1, 7]
    assert picks[3] not in (5, 1, 7)


# ---------------------------------------------------------------------------------------------------- a pick without variance
@pytest.mark.parametrize("key", ["wipv", "wipstd"])
def test_a_pick_whose_variance_is_not_positive(key):
    """Eight candidates ON training points at noise 1e-30: their s_c is rounding noise around 0.  Where it comes out negative the
    scorer gives the candidate the floor score and the selection picks it; the next stage divides by sqrt(s_p).  Pinned here:
    no score row holds a NaN, every pick is ``masked_argmin`` of the device's own row, every row is what the float64
    restatement's rules (``score_state``: a negative s, a NaN or sub-floor variance -> the floor) give on the device's own
    downdated state, a pick with s_p < 0 leaves a state without a finite entry and every later row at the floor, and the handle
    is left alone."""
    from bobe_amd import GP
    import batch_select_restatement as BS
    rng = np.random.default_rng(160)
    n, d, c, m, b = 24, 3, 40, 20, 6
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    cand[:8] = X[:8]
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2
    ls, kvar = np.full(d, 0.25), 2.0
    gp = GP(X, y, noise=1e-30, kernel="rbf", lengthscales=ls, kernel_variance=kvar)
    assert not gp.not_pd
    cand, Z = np.ascontiguousarray(cand), np.ascontiguousarray(Z)
    before = gp.wip_sweep(cand, Z)
    picks, stage = shipped(gp, cand, Z, None, key, b)
    floor = (FLOOR * gp.y_std ** 2) ** (1.0 if key == "wipv" else 0.5)
    assert not np.any(np.isnan(stage))
    taken = []
    for j in range(b):
        assert picks[j] == masked_argmin(stage[j], taken), j
        taken.append(int(picks[j]))
    kcz = BS.kernel("rbf", cand, Z, ls, kvar)
    dead = False                                           # a pick with s_p < 0 was applied
    for j in range(b):
        t = batch_terms(gp, cand, Z, None, key, j, picks[:j], scores=False)
        wv, ws = BS.score_state(kcz, t["crossT"], t["basez"], t["sc"], gp.y_std)
        want = wv if key == "wipv" else ws
        err = np.max(np.abs(stage[j] - want) / want)
        print("no-variance pick %s stage %d: pick %d with s_p %.3e, score %.3e (floor %.3e), row against the rules %.1e, "
              "finite s_c %d of %d" % (key, j, picks[j], t["sc"][picks[j]], stage[j, picks[j]], floor, err,
                                       int(np.sum(np.isfinite(t["sc"]))), c))
        assert err <= 1e-7, (j, err)
        if dead:
            assert not np.any(np.isfinite(t["sc"])) and not np.any(np.isfinite(t["basez"]))
            assert np.all(np.abs(stage[j] / floor - 1) <= 1e-12)
        if j == 0 and np.any(t["sc"][:8] < 0):
            assert picks[0] < 8 and t["sc"][picks[0]] < 0 and abs(stage[0, picks[0]] / floor - 1) <= 1e-12
        dead = dead or not t["sc"][picks[j]] >= 0
    after = gp.wip_sweep(cand, Z)
    assert same_bits(before["wipv"], after["wipv"]) and same_bits(before["wipstd"], after["wipstd"]) and gp.npoints == n
