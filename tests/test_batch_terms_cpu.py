"""The checker of the batch selection's later stages (tests/batch_terms_restatement.py, tests/batch_terms_cases.py) has teeth, and
its truth is what it is said to be.  No GPU: the float64 NumPy recursion, laid out as ``bobe_debug_batch_terms`` hands the
device's out, stands in for the device.

  - the float64 recursion passes every Layer A bound, along forced picks on the tile edges, along a truth's picks, and where
    the candidates are the integration points;
  - each planted fault is flagged with a ratio above 1 at the planted place: a u row shifted by one column, s_c downdated with
    the previous stage's u, u divided by the root of the already downdated s_p, the rank-one update skipping its last group of
    16 rows, the sum over the earlier u rows dropping its last row, one entry a few bounds off (a downdate: 8 ulps of its
    bound's scale);
  - the truth's row-append form equals the literal refits to 1e-15 at b = 4;
  - the gap table: every Layer B case keeps the truth's two best unmasked scores more than GAP_MIN apart at every stage of its
    batch, with the figures tests/batch_terms_cases.py records, and the float64 recursion holds the device's rule there;
  - the dtype-generic ``weighted_scores`` is tests/weighted_criteria_restatement.py's bit for bit in float64."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_terms_cases as BC  # noqa: E402
import batch_terms_restatement as B  # noqa: E402
import weighted_criteria_restatement as W  # noqa: E402
import zvar_cases as ZC  # noqa: E402
import zvar_restatement as R  # noqa: E402

LD = np.longdouble
EDGES = BC.FORCED["tile_edge-edges"]
STAGE_KEYS = ("uc", "uz", "sc", "basez", "crossT")


def edge_terms():
    shape, kernel, _, forced = EDGES
    t = BC.recursion(shape, kernel, forced)
    return {k: ([a.copy() for a in v] if isinstance(v, list) else v.copy()) for k, v in t.items()}


def ratios(shape, kernel, t):
    res = BC.check(shape, kernel, t)
    print("\n" + BC.table_line("%s float64 recursion" % shape, res))
    return res


# ---------------------------------------------------------------------------------------------------- the recursion passes
@pytest.mark.parametrize("shape,kernel,picks", [
    (EDGES[0], EDGES[1], EDGES[3]), ("cand_is_z", "matern", [5, 76, 0, 64, 63, 31]),
    ("near_noise_m65", "rbf", list(range(39, 23, -1))), ("dim17", "rbf", [3, 59, 0]),
    ("reference_noise_130", "rbf", [149, 0, 128, 127, 64])], ids=["tile_edges", "cand_is_z", "near_noise", "dim17", "noise_1e-8"])
def test_float64_recursion_passes_every_bound(shape, kernel, picks):
    res = ratios(shape, kernel, BC.recursion(shape, kernel, picks))
    for k in STAGE_KEYS:                                       # (measured: u rows 0.02 .. 0.04; a downdate in two roundings 0.5)
        assert res[k][0] <= (0.1 if k in ("uc", "uz") else 0.51), (k, res[k])


def test_the_recursion_along_a_truths_picks_passes_and_scores_as_the_select_batch_restatement():
    import batch_select_restatement as BS
    ref = BC.truth("near_noise_m64", "wipstd")
    shape, kernel, weighted, _, bs = BC.CASES["near_noise_m64"]
    assert not weighted
    t = BC.recursion(shape, kernel, ref["picks"][:-1])
    res = ratios(shape, kernel, t)
    for k in STAGE_KEYS:
        assert res[k][0] <= (0.1 if k in ("uc", "uz") else 0.51), (k, res[k])
    X, _, cand, Z, _ = BC.case_data(shape)
    ls, kvar, noise, _ = BC.hyper(shape)
    picks, stages = BS.select_batch(kernel, X, cand, Z, ls, kvar, noise, bs["wipstd"], "wipstd")
    assert picks.tolist() == ref["picks"].tolist()
    kcz = BS.kernel(kernel, cand, Z, ls, kvar)
    for j in range(bs["wipstd"]):
        ws = BS.score_state(kcz, t["crossT"][j], t["basez"][j], t["sc"][j], 1.0)[1]
        assert np.max(np.abs(ws - stages[j]) / stages[j]) <= 1e-9, j


# ---------------------------------------------------------------------------------------------------- teeth
def flagged(t, key, stage, where=None):
    """The ratio of ``key`` AT THE PLANTED STAGE is above 1 (and found at the planted entry); returns it."""
    res = BC.check(EDGES[0], EDGES[1], t)
    ratio, at = res["stages"][key][stage - 1]
    print("  %s stage %d: ratio %.3g at %s" % (key, stage, ratio, at))
    assert ratio > 1.0, (key, ratio, at)
    if where is not None:
        assert where(at), (key, ratio, at)
    return ratio


def test_a_u_row_shifted_by_one_column_is_flagged():
    t = edge_terms()
    t["UC"][4] = np.roll(t["UC"][4], 1)
    flagged(t, "uc", 5)
    t = edge_terms()
    t["UZ"][2][1:] = t["UZ"][2][:-1].copy()
    flagged(t, "uz", 3)


def test_s_c_downdated_with_the_previous_stages_u_is_flagged():
    t = edge_terms()
    t["sc"][4] = t["sc"][3] - t["UC"][2] ** 2
    flagged(t, "sc", 4)
    t = edge_terms()
    t["basez"][4] = t["basez"][3] - t["UZ"][2] ** 2
    flagged(t, "basez", 4)


def test_u_divided_by_the_root_of_the_downdated_s_p_is_flagged():
    """What k_batch_u would do if it read s_p from s_c (which it overwrites) instead of k_batch_gather's copy."""
    t = edge_terms()
    j, p = 3, t["picks"][2]
    scale = np.sqrt(t["sc"][j - 1][p] / t["sc"][j][p])
    assert scale > 10                                              # (the pick's own s_c falls to about 2 noise)
    t["UC"][j - 1] = t["UC"][j - 1] * scale
    t["UZ"][j - 1] = t["UZ"][j - 1] * scale
    flagged(t, "uc", j)
    flagged(t, "uz", j)


def test_a_rank_one_update_that_skips_its_last_group_of_16_rows_is_flagged():
    t = edge_terms()
    m = t["UZ"].shape[1]
    first = (m - 1) // 16 * 16                                     # rows 64 .. 76 of 77: the last group with live rows
    t["crossT"][6][first:] = t["crossT"][5][first:]
    flagged(t, "crossT", 6, lambda at: at[0] >= first)


def test_a_sum_over_the_earlier_rows_that_drops_its_last_row_is_flagged():
    t = edge_terms()
    j, p = 5, t["picks"][4]
    root = np.sqrt(t["sc"][j - 1][p])
    t["UC"][j - 1] = t["UC"][j - 1] + t["UC"][j - 2] * t["UC"][j - 2][p] / root
    flagged(t, "uc", j)
    t = edge_terms()
    t["UZ"][j - 1] = t["UZ"][j - 1] + t["UZ"][j - 2] * t["UC"][j - 2][p] / root
    flagged(t, "uz", j)


@pytest.mark.parametrize("key", ["uc", "uz", "sc", "basez", "crossT"])
def test_one_entry_a_few_bounds_off_is_flagged(key):
    """A downdate is moved by 8 ulps (16 eps) of the scale its bound multiplies, |s_old| + u^2: 8 bounds.  A u row's bound is
    gamma_{N+j+2} of its scale (|k| + |V|^T |v*| + sum |u_i| |u_i(p)|) / sqrt(s_p), not 2 eps of it, so 8 ulps of that scale lie
    inside it: there the fault is 8 gamma-bounds (8 ulps times (N + j + 2) / 2) plus 16 x 8 ulps of |u|, which comes out at 20 to
    30 times the whole bound - small, and not "8 ulps of the scale"."""
    t = edge_terms()
    j, c, z = 4, 200, 70
    ulp8 = 16 * 2.0 ** -53
    if key in ("sc", "basez"):
        i, u = (c, t["UC"][j - 1][c]) if key == "sc" else (z, t["UZ"][j - 1][z])
        t[key][j][i] += ulp8 * (abs(t[key][j - 1][i]) + u * u)
        assert 7 <= flagged(t, key, j, lambda at: at == (i,)) <= 9
    elif key == "crossT":
        t[key][j][z, c] += ulp8 * (abs(t[key][j - 1][z, c]) + abs(t["UZ"][j - 1][z] * t["UC"][j - 1][c]))
        assert 7 <= flagged(t, key, j, lambda at: at == (z, c)) <= 9
    else:
        p = t["picks"][j - 1]
        side, i = ("V", c) if key == "uc" else ("VZ", z)
        U = t["UC"] if key == "uc" else t["UZ"]
        n = t["V"].shape[0]
        mag = abs(t[side][:, i]) @ abs(t["V"][:, p]) + abs(U[:j - 1, i]) @ abs(t["UC"][:j - 1, p]) + 2.0
        U[j - 1][i] += ulp8 * (n + j + 2) / 2 * mag / np.sqrt(t["sc"][j - 1][p]) + 16 * ulp8 * abs(U[j - 1][i])
        assert 8 <= flagged(t, key, j, lambda at: at == (i,)) <= 64


# ---------------------------------------------------------------------------------------------------- the truth
def test_the_row_append_form_is_the_literal_refit():
    """1e-15 on the four scores that are sums over the integration points; zvar = -log T is held to 1e-14 (T is a difference:
    the two long-double routes differ by 3.5e-15 (1 + |zvar|) there)."""
    shape, kernel, weighted, y_std, _ = BC.CASES["tile_edge"]
    args = BC._args(shape, kernel, weighted, y_std)
    for key in B.KEYS:
        a, l = B.append_batch(*args, 4, key), B.literal_batch(*args, 4, key, dtype=LD)
        scale = (1 + np.abs(l[1])) if key in B.LOG_KEYS else np.abs(l[1])
        err = float(np.max(np.abs(a[1] - l[1]) / scale))
        print("row append against refits, %s: %.2e" % (key, err))
        assert a[0].tolist() == l[0].tolist() and a[3].tolist() == l[3].tolist()
        assert err <= (1e-14 if key == "zvar" else 1e-15), (key, err)
        assert np.allclose(a[2], l[2], rtol=1e-9, atol=0)
    # along given picks as well (the duplicates case's form)
    follow = (7, 270, 3)
    a, l = B.append_batch(*args, 4, "wipstd", follow=follow), B.literal_batch(*args, 4, "wipstd", dtype=LD, follow=follow)
    assert a[0][:3].tolist() == list(follow) == l[0][:3].tolist() and a[3].tolist() == l[3].tolist()
    assert float(np.max(np.abs(a[1] - l[1]) / np.abs(l[1]))) <= 1e-15


def test_weighted_scores_in_float64_is_the_original_bit_for_bit():
    for shape, kernel, y_std in (("tile_edge", "rbf", 30.0), ("near_noise_m64", "matern", 1.0)):
        s64, sld, _, std = ZC.states(shape, kernel, y_std)
        lw = ZC.case_data(shape, y_std)[4]
        for w in (lw, None):
            old, new, ld = W.weighted_scores(s64, std, w), B.weighted_scores(s64, std, w), B.weighted_scores(sld, std, w)
            for k in W.KEYS + ("log_s",):
                assert np.array_equal(np.asarray(old[k]), np.asarray(new[k])), k
                assert np.asarray(ld[k]).dtype == LD
                assert np.max(np.abs(np.asarray(new[k]) - ld[k]) / (1 + np.abs(ld[k]))) <= 1e-8, k


@pytest.mark.parametrize("name,key", BC.LAYER_B, ids=["%s-%s" % a for a in BC.LAYER_B])
def test_gap_table(name, key):
    """The precondition of asserting the truth's pick at every stage, with the recorded figures; beside it the float64
    recursion's error against the truth, which must hold the device's rule."""
    shape, kernel, weighted, y_std, bs = BC.CASES[name]
    ref = BC.truth(name, key)
    b, gap, at, f64_err = BC.GAPS[(name, key)]
    assert b == bs[key] == len(ref["gaps"]) and (b >= 16 or name in BC.SHORT)
    assert np.all(ref["gaps"] > BC.GAP_MIN), ref["gaps"]
    assert int(np.argmin(ref["gaps"])) == at and abs(ref["gaps"].min() / gap - 1) <= 0.01, (ref["gaps"].min(), gap)
    args = BC._args(shape, kernel, weighted, y_std)
    t = BC.recursion(shape, kernel, ref["picks"][:-1], solve=True)
    s64 = R.state(kernel, *args[1:8], np.float64)
    worst, ref_worst, missed = 0.0, 0.0, []
    for j in range(b):
        got = B.scores(B.state_of(t, j, s64["kcz"], s64["mu"]), args[8], args[9], key)
        ok, err, ref_err = B.rule(got, ref["f64"][j], ref["truth"][j], key)
        worst, ref_worst = max(worst, err), max(ref_worst, ref_err)
        if not ok:
            missed.append(j)
        taken = ref["picks"][:j]
        assert BC.B.masked_argmin(got, taken) == ref["picks"][j], j
    print("\n%-20s %-6s b %2d  min gap %.2e at stage %2d  float64 recursion %.2e  float64 literal refit %.2e" % (
        name, key, b, ref["gaps"].min(), at, worst, ref_worst))
    assert abs(ref_worst / f64_err - 1) <= 0.5 or abs(ref_worst - f64_err) <= 1e-15
    # the float64 recursion holds the device's rule at every stage, but on the recorded cases (printed there, not asserted:
    # the misses are marginal and NumPy's sums are the BLAS library's to order)
    if (name, key) in BC.RECURSION_MISSES:
        print("%-20s %-6s the float64 recursion misses the rule at stages %s" % (name, key, missed))
    else:
        assert not missed, missed


def test_the_batches_are_as_long_as_asked():
    assert sum(1 for c in BC.CASES.values() if max(c[4].values()) >= 48) >= 2
    assert set(BC.CASES["tile_edge"][4]) == set(B.KEYS)
    assert set(BC.CASES["ill_conditioned"][4]) | set(BC.CASES["ill_conditioned_4e3"][4]) == set(B.KEYS)
    assert BC.CASES["tile_edge"][4]["wipstd"] == 64 and BC.CASES["reference_noise_300"][4]["wipv"] >= 48


def test_the_duplicates_pool():
    pool, originals = BC.duplicates_pool()
    assert pool.shape == (308, 3) and len(set(originals.tolist())) == 4
    for i, p in enumerate(originals):
        assert np.array_equal(pool[300 + 2 * i], pool[p])
        assert np.allclose(pool[301 + 2 * i] - pool[p], BC.DUP_SHIFT, rtol=1e-6, atol=0)
    # a copy ties with its original at the stage that picks it, and after the pick its s_c is about 2 noise
    args = BC._args("duplicates", "rbf", False)
    noise = args[7]
    _, stages, gaps, _ = B.append_batch(*args, 2, "wipstd")
    assert gaps[0] < BC.GAP_MIN
    t = BC.recursion("duplicates", "rbf", [int(originals[0])])
    s = t["sc"][1][[300, 301]]
    print("s_c of the copies after their original is picked: %s (noise %.0e)" % (s, noise))
    assert np.all(s > 0) and np.all(s < 1e3 * noise)
