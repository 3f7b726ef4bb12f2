"""Every tile_gemm instantiation the library ships, one at a time, against an exact product.

bobe_debug_tile_gemm (bobe_amd/csrc/gp_tile_harness.hip) runs one instantiation - acc = load_tile(C) or 0, tile_gemm,
store_tile - on caller-supplied operands with the dynamic LDS of the launch that ships it.  The cases of
tests/tile_gemm_cases.py are small integers embedded in arrays of other integers, so the expected C, guards included, is
exact and the comparison is np.array_equal; tests/test_tile_gemm_cases_cpu.py shows on the CPU that each case tells the wrong
kernels it lists from the right one.  A new tile_gemm instantiation gets a row in the harness's table and in
tile_gemm_cases.SHIPPED_ROWS.

The TRIL case shorter than T (K = T / 2) is legal for both cores: they read the columns [kbeg, kend) only and take column k
as column k - (kend - T) of the closing block, so the range simply begins inside the block (kd = kbeg, the first step has
rel = T - (kend - kbeg)); the zeros are placed accordingly.  No shipped launch does this (their K ranges end at (ti + 1) T
and begin at 0), the harness allows it.
"""
import ctypes as C

import numpy as np
import pytest

import tile_gemm_cases as G

pytestmark = pytest.mark.gpu

VARIANTS = G.expected_variants()


def vid(v):
    return "T%d_BK%d_%s_%s%s%s%s%s%s" % (v.T, v.BK, "glds" if v.glds else "regs", "KR"[v.la], "KR"[v.lb],
                                         "_nega" if v.nega else "", "_tril" if v.tril else "",
                                         "_2groups" if v.groups == 2 else "", "_1buf" if v.single_buffer else "")


@pytest.fixture(scope="module")
def lib():
    from bobe_amd import _lib
    lib = _lib.load()
    assert lib.bobe_device_count() >= 1, "native library loaded but no HIP device"
    return lib


@pytest.fixture(scope="module")
def index(lib):
    """info tuple -> variant number, as the library reports them"""
    out = {}
    for i in range(lib.bobe_debug_tile_gemm_count()):
        info = (C.c_int * 9)()
        assert lib.bobe_debug_tile_gemm_info(i, info) == 0, lib.bobe_last_error()
        v = G.Variant(*info)
        assert v not in out, f"variant {tuple(v)} is compiled twice"
        out[v] = i
    return out


def run(lib, variant, c, **over):
    """One harness call on copies of the case's arrays; returns (status, C)."""
    from bobe_amd import _lib
    a = dict(tiles_m=c.tiles_m, tiles_n=c.tiles_n, m0=c.m0, n0=c.n0, kbeg=c.kbeg, kend=c.kend, alpha=c.alpha, beta=c.beta,
             preload=c.preload, lda=c.A.shape[1], ldb=c.B.shape[1], ldc=c.C0.shape[1])
    a.update(over)
    Cc = np.ascontiguousarray(c.C0.copy())
    A = Cc if c.inplace else np.ascontiguousarray(c.A)
    B = Cc if c.inplace else np.ascontiguousarray(c.B)
    st = lib.bobe_debug_tile_gemm(0, variant, a["tiles_m"], a["tiles_n"], a["m0"], a["n0"], a["kbeg"], a["kend"],
                                  _lib.ptr(A), a["lda"], A.shape[0], _lib.ptr(B), a["ldb"], B.shape[0],
                                  _lib.ptr(Cc), a["ldc"], Cc.shape[0], float(a["alpha"]), float(a["beta"]), a["preload"])
    return st, Cc


def test_every_shipped_variant_is_compiled(lib, index):
    assert lib.bobe_debug_tile_gemm_count() == len(index) >= len(VARIANTS)
    for v in VARIANTS:
        assert v in index, f"the harness has no variant {vid(v)}"
    for row in G.two_core_rows():
        T, BK, la, lb, nega, tril, groups, sb = row
        for glds in (0, 1):
            assert G.Variant(T, BK, glds, la, lb, nega, tril, groups, sb) in index
    bad = (C.c_int * 9)()
    for i in (-1, lib.bobe_debug_tile_gemm_count()):
        assert lib.bobe_debug_tile_gemm_info(i, bad) == -1 and lib.bobe_last_error()


@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_tile_gemm_exact(lib, index, v):
    cs = G.cases(v)
    failed = []
    for c in cs:
        st, got = run(lib, index[v], c)
        assert st == 0, (c.name, lib.bobe_last_error())
        if not np.array_equal(got, c.expected):
            bad = np.argwhere(got != c.expected)
            failed.append((c.name, len(bad), tuple(bad[0]), got[tuple(bad[0])], c.expected[tuple(bad[0])]))
    assert not failed, f"{vid(v)}: (case, wrong elements, first at, got, expected) = {failed}"


@pytest.mark.parametrize("row", G.two_core_rows(), ids=lambda r: vid(G.Variant(r[0], r[1], 1, *r[2:])).replace("_glds", ""))
def test_both_cores_same_bits_and_within_rounding(lib, index, row):
    """Real operands: the two cores of a row return the same bits (gemm_f64.hpp: "the same MFMAs in the same order"), and
    they lie within gamma_(K+3) (|alpha| |A| |B|^T + |beta| |C0|) of the product formed in np.longdouble - a bound that holds
    for any order of summation, fused or not, so anything beyond it is a wrong operand, not rounding."""
    got = []
    for glds in (1, 0):
        v = G.Variant(row[0], row[1], glds, *row[2:])
        c = G.real_case(v)
        st, out = run(lib, index[v], c)
        assert st == 0, lib.bobe_last_error()
        got.append(out)
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64)), \
        "%d elements differ between the cores" % int((got[0].view(np.uint64) != got[1].view(np.uint64)).sum())
    err = np.abs(got[0].astype(np.longdouble) - c.expected)
    bound = G.real_bound(c)
    over = err > bound
    print("max |C - C_ld| / bound over the tiles: %.3g" % float(np.max(err[bound > 0] / bound[bound > 0])))
    assert not over.any(), "%d elements beyond the rounding bound, worst %.3g" % (int(over.sum()), float(err.max()))


def test_refusals_leave_c_untouched(lib, index):
    """Each refusal: BOBE_ERR_ARG (-1), a message, nothing launched - the C passed in comes back as it went."""
    def pick(**kw):
        return next(v for v in VARIANTS if all(getattr(v, k) == x for k, x in kw.items()))
    v = pick(T=64, BK=16, glds=1, la=G.KC, lb=G.RC)
    c = G.cases(v)[1]
    T, BK = v.T, v.BK
    sb = pick(single_buffer=1)
    two = pick(groups=2)
    tril = pick(tril=1, glds=1)
    trials = [
        ("unknown variant (-1)", -1, c, {}),
        ("unknown variant (count)", lib.bobe_debug_tile_gemm_count(), c, {}),
        ("odd lda", index[v], c, dict(lda=c.A.shape[1] - 1)),
        ("odd ldb", index[v], c, dict(ldb=c.B.shape[1] - 1)),
        ("odd ldc", index[v], c, dict(ldc=c.C0.shape[1] - 1)),
        ("m0 off the tile grid", index[v], c, dict(m0=c.m0 + T // 2)),
        ("n0 off the tile grid", index[v], c, dict(n0=c.n0 + 16)),
        ("kbeg off the tile grid", index[v], c, dict(kbeg=c.kbeg - BK)),
        ("K range not a multiple of BK", index[v], c, dict(kend=c.kend + BK // 2)),
        ("empty K range", index[v], c, dict(kend=c.kbeg)),
        ("negative K range", index[v], c, dict(kend=c.kbeg - BK)),
        ("two steps on one buffer", index[sb], G.cases(sb)[0], dict(kend=G.cases(sb)[0].kend + sb.BK)),
        ("odd tiles_n on two groups", index[two], G.cases(two)[0], dict(tiles_n=1)),
        ("tiles past the end of C", index[v], c, dict(tiles_m=4)),
    ]
    for what, variant, case, over in trials:
        st, got = run(lib, variant, case, **over)
        assert st == -1, f"{what}: status {st}"
        assert lib.bobe_last_error(), what
        assert np.array_equal(got, case.C0), f"{what}: C was written"
    # in place, a K range that runs into the tiles being written is refused too
    ip = next(x for x in G.cases(pick(T=64, BK=16, glds=0, nega=1)) if x.inplace)
    st, got = run(lib, index[pick(T=64, BK=16, glds=0, nega=1)], ip, kend=ip.n0 + 16)
    assert st == -1 and lib.bobe_last_error() and np.array_equal(got, ip.C0)
    # legal, not a refusal: a TRIL range shorter than T (it is a case of test_tile_gemm_exact)
    short = next(x for x in G.cases(tril) if x.name == "tril_T/2")
    assert short.kend - short.kbeg < tril.T
    st, got = run(lib, index[tril], short)
    assert st == 0 and np.array_equal(got, short.expected)
