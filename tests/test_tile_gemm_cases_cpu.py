"""The tile-core harness's cases (tests/tile_gemm_cases.py) can tell a wrong kernel from a right one: checked with NumPy
alone, before anything runs on a GPU.  For every variant the harness must have and every case: the data are what the
embedding promises, the expected C is exact, and each wrong computation of `mutations()` gives a different C."""
import numpy as np
import pytest

import tile_gemm_cases as G

VARIANTS = G.expected_variants()
# data do not depend on the core: one of a row's two variants is enough here
ROWS = [v for v in VARIANTS if not (v.glds == 0 and G.has_glds_core(v.T, v.BK) and v._replace(glds=1) in VARIANTS)]
ALL_MUTATIONS = {"k+BK", "k-BK", "k one step short", "m0 and n0 exchanged", "A in the other layout", "B in the other layout",
                 "NEGA inverted", "TRIL block strictly lower", "alpha and beta exchanged", "preload inverted",
                 "groups exchanged"}


def vid(v):
    return "T%d_BK%d_%s%s%s%s%s%s" % (v.T, v.BK, "KR"[v.la], "KR"[v.lb], "_nega" if v.nega else "", "_tril" if v.tril else "",
                                     "_2groups" if v.groups == 2 else "", "_1buf" if v.single_buffer else "")


def test_variant_table():
    assert len(VARIANTS) == len(set(VARIANTS)) == 18
    for row in G.two_core_rows():
        T, BK, la, lb, nega, tril, groups, sb = row
        assert {G.Variant(T, BK, g, la, lb, nega, tril, groups, sb) for g in (0, 1)} <= set(VARIANTS)
    assert all(v.glds == 0 for v in VARIANTS if not G.has_glds_core(v.T, v.BK))
    assert len(ROWS) == 12


@pytest.mark.parametrize("v", ROWS, ids=vid)
def test_case_list(v):
    cs = {c.name: c for c in G.cases(v)}
    T, BK = v.T, v.BK
    assert len(cs) == len(G.cases(v)), "case names repeat"
    want_steps = (1,) if v.single_buffer else (1, 2, 3, 5, 24)
    for s in want_steps:
        c = cs[f"steps{s}"]
        assert c.steps == s and (c.tiles_m, c.tiles_n) == (2, 2)
        assert min(c.m0, c.n0, c.kbeg) > 0 and c.m0 % T == c.n0 % T == c.kbeg % T == 0
    if v.single_buffer:
        assert all(c.steps == 1 for c in cs.values())
    o = cs["origin"]
    assert (o.m0, o.n0, o.kbeg, o.tiles_m, o.tiles_n) == (0, 0, 0, 1, v.groups)
    for alpha, beta in ((1, 0), (-1, 1), (-1, 0), (3, -2)):
        c = cs[f"alpha{alpha}_beta{beta}"]
        assert (c.alpha, c.beta, c.preload) == (alpha, beta, 0)
    assert (cs["preload"].alpha, cs["preload"].beta, cs["preload"].preload) == (1, 0, 1)
    assert ("inplace" in cs) == (v.la == G.KC and v.lb == G.KC and bool(v.nega))
    if "inplace" in cs:
        c = cs["inplace"]
        assert c.A is c.B and c.B is c.C0 and c.preload == 1 and c.inplace
        assert c.m0 > c.n0 + (c.tiles_n - 1) * T, "every tile lies strictly below the diagonal"
        assert 0 < c.kbeg < c.kend <= c.n0, "the K range lies left of the tiles' column blocks"
    if v.tril:
        assert [cs[n].kend - cs[n].kbeg for n in ("tril_T", "tril_T+BK", "tril_3T", "tril_T/2")] == [T, T + BK, 3 * T, T // 2]
    assert all(c.tiles_n % v.groups == 0 for c in cs.values())
    if v.groups == 2:
        assert all((c.tiles_m, c.tiles_n) == (2, 2) for c in cs.values() if c.name != "origin")


@pytest.mark.parametrize("v", ROWS, ids=vid)
def test_embedding_and_exactness(v):
    T, BK = v.T, v.BK
    for c in G.cases(v):
        m1, n1 = c.m0 + c.tiles_m * T, c.n0 + c.tiles_n * T
        assert (c.kend - c.kbeg) % BK == 0 and c.kend > c.kbeg
        for X in (c.A, c.B):
            E = X.shape[0]
            assert X.shape == (E, E + 16) and X.shape[1] % 2 == 0, "ld = extent + 16, even"
            assert E >= max(m1, n1, c.kend + BK), "both layouts, a shifted K range and exchanged offsets are readable"
            assert np.array_equal(X, np.rint(X)) and np.abs(X).max() <= 8
            assert abs(X.mean()) > 0.2, "the draw is asymmetric"
        if not c.inplace:
            assert c.A is not c.B and not np.array_equal(c.A, c.B)
            # what surrounds the operands is other integers, not zeros: fewer than one in eight anywhere but the TRIL zeros
            Bv = G.opview(c.B, v.lb)
            assert (Bv == 0).mean() < 0.125
            if not v.tril:
                assert (c.A == 0).mean() < 0.125
            # C: integers in [-64, 64] in the tiles, the sentinel everywhere else; T guard rows below and as many as the
            # offsets allow above, 16 guard columns or more on either side (none left of n0 = 0)
            guard = np.ones(c.C0.shape, bool)
            guard[c.m0:m1, c.n0:n1] = False
            assert np.all(c.C0[guard] == G.SENTINEL) and np.all(c.expected[guard] == G.SENTINEL)
            tiles = c.C0[c.m0:m1, c.n0:n1]
            assert np.array_equal(tiles, np.rint(tiles)) and np.abs(tiles).max() <= 64
            assert c.C0.shape[0] == m1 + T and c.C0.shape[1] >= n1 + 16 and c.C0.shape[1] % 2 == 0
            assert c.m0 == 0 or c.m0 >= T
            assert c.n0 == 0 or c.n0 >= 16
        if v.tril:
            Av = G.opview(c.A, v.la)
            for p in range(c.tiles_m):
                for k in range(max(c.kbeg, c.kend - T), c.kend):
                    cc = k - (c.kend - T)
                    col = Av[c.m0 + p * T:c.m0 + (p + 1) * T, k]
                    assert np.all(col[:cc] == 0.0) and np.all(col[cc:] != 0.0)
        assert isinstance(c.alpha, int) and isinstance(c.beta, int)
        assert c.exact_bound() < 2 ** 53
        exp_i = G.compute(c, np.int64)
        assert np.abs(exp_i).max() <= max(c.exact_bound(), G.SENTINEL)
        assert c.expected.dtype == np.float64 and np.array_equal(c.expected, exp_i.astype(np.float64))
        assert np.array_equal(exp_i, c.expected.astype(np.int64))


@pytest.mark.parametrize("v", ROWS, ids=vid)
def test_cases_tell_wrong_kernels_apart(v):
    seen = set()
    for c in G.cases(v):
        names = {n for n, _ in G.mutations(c)}
        # nothing is left out but what does not exist for the case
        absent = ALL_MUTATIONS - names
        allowed = set()
        if c.kbeg == 0:
            allowed.add("k-BK")
        if c.m0 == c.n0:
            allowed.add("m0 and n0 exchanged")
        if not v.tril:
            allowed.add("TRIL block strictly lower")
        if v.groups != 2:
            allowed.add("groups exchanged")
        assert absent == allowed, (c.name, absent, allowed)
        assert c.name == "origin" or not ({"k-BK", "m0 and n0 exchanged"} & absent)
        for name, kw in G.mutations(c):
            wrong = G.compute(c, np.int64, **kw)
            assert not np.array_equal(wrong, c.expected), f"{vid(v)} / {c.name} cannot see: {name}"
        seen |= names
    assert seen == ALL_MUTATIONS - ({"TRIL block strictly lower"} if not v.tril else set()) - \
        ({"groups exchanged"} if v.groups != 2 else set())


def test_real_case_bound_is_meaningful():
    """The real-data case: the bound is zero on the guards, tiny against the entries, and a misread operand breaks it."""
    for row in G.two_core_rows():
        v = G.Variant(row[0], row[1], 1, *row[2:])
        c = G.real_case(v)
        bound = G.real_bound(c)
        T = v.T
        tiles = (slice(c.m0, c.m0 + 2 * T), slice(c.n0, c.n0 + 2 * T))
        assert c.steps == 5 and (c.tiles_m, c.tiles_n) == (2, 2)
        mask = np.ones(bound.shape, bool)
        mask[tiles] = False
        assert np.all(bound[mask] == 0) and np.all(c.expected[mask] == G.SENTINEL)
        assert 0 < bound[tiles].min() and bound[tiles].max() < 1e-11      # gamma_83 = 9.2e-15 times sums of order 10 .. 100
        c64 = G.compute(c, np.float64)                   # NumPy's own fp64 product obeys the bound ...
        assert np.all(np.abs(c64 - c.expected) <= bound)
        for kw in (dict(kshift=v.BK), dict(kshort=1), dict(swap_mn=True), dict(flip_sign=True)):   # ... a wrong one does not
            assert not np.all(np.abs(G.compute(c, np.float64, **kw) - c.expected) <= bound), kw
