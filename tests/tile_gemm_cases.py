"""Cases for the tile-core harness (bobe_debug_tile_gemm): NumPy only, no GPU.

For a variant's info tuple (T, BK, glds, la, lb, nega, tril, groups, single_buffer) `cases()` yields Case objects: the
operands embedded in larger arrays of other random integers, the call arguments and the expected C.  All data are small
integers, so every partial sum is an integer far below 2^53 and the expected C is exact in fp64 whatever the order of
summation: the GPU test compares with np.array_equal.

`compute()` is the plain model of what the harness does; its keyword arguments also state the WRONG computations a case has
to tell from the right one (`mutations()`), which tests/test_tile_gemm_cases_cpu.py checks on the CPU.

Conventions of the embedding
  * A and B are square arrays of E x (E + 16) random integers in [-8, 8] (ld = extent + 16), E large enough that either
    layout, a K range shifted by one K-step and exchanged m0 / n0 can all be read from them: a misread finds other
    integers, never zeros and never the end of the array.
  * C is SENTINEL everywhere except the tiles, which hold integers in [-64, 64]: T guard rows below, 16 guard columns to the
    right, and above / to the left everything up to m0 / n0 (at least T rows and T >= 16 columns wherever m0, n0 > 0; the one
    case at the origin can have no guard above or to the left, the harness takes m0 and n0 from the array's corner).
  * In-place cases pass ONE square matrix of integers in [-8, 8] as A, B and C; what surrounds the tiles is the guard.
  * A TRIL variant requires of EVERY call that the last T columns of A's K range are lower triangular per tile row, so every
    case of such a variant has that structure: non-zero on and below the diagonal, exact zeros above.
"""
import zlib
from collections import namedtuple

import numpy as np

KC, RC = 0, 1
SENTINEL = 7777.0
Variant = namedtuple("Variant", "T BK glds la lb nega tril groups single_buffer")

# The instantiations the library ships, as data: (T, BK, la, lb, nega, tril, groups, single_buffer).  For rows whose tile has
# a direct-to-LDS core (T in {64, 128}, BK = 16) the harness holds both cores, so both are expected.  Each kernel runs one
# core, fixed at compile time.  The three 64-tile rows with two cores ship direct-to-LDS only: their register-staged harness
# variants belong to no shipped launch and remain as the reference of the same-bits comparison between the cores.
# DEBUG_ROWS are the remaining layouts of k_debug_gemm (register-staged only).
SHIPPED_ROWS = (
    (128, 16, RC, RC, 0, 0, 1, 0),   # sweep cross products, LOO, posterior covariance, paths, k_lauum_grad<., ., 128>
    (128, 16, KC, RC, 0, 0, 1, 0),   # k_trtri_T/R<128>, blocked solve (kbeg > 0)
    (128, 16, KC, RC, 0, 1, 1, 0),   # Linv x B in the sweep and the posterior
    (64, 16, RC, RC, 0, 0, 1, 0),    # sweep, LOO, paths, k_lauum_grad<., ., 64> (direct-to-LDS only)
    (64, 16, KC, RC, 0, 0, 1, 0),    # k_trtri_T/R<64>, 64-tile solve (direct-to-LDS only)
    (64, 16, KC, KC, 1, 0, 1, 0),    # k_syrk_trail<64, 16> (preload, in place; direct-to-LDS only)
    (64, 32, KC, KC, 1, 0, 2, 0),    # panel fillers: two groups per workgroup
    (32, 32, RC, RC, 0, 0, 1, 0),    # k_lauum_tiles32, k_paths_tiles<32>
    (32, 32, KC, RC, 0, 0, 1, 0),    # k_trtri_T/R<32>
    (32, 128, KC, KC, 1, 0, 1, 1),   # k_syrk_trail<32, 128>: one LDS buffer, one K-step
)
DEBUG_ROWS = (
    (128, 16, KC, KC, 0, 0, 1, 0),
    (128, 16, RC, KC, 0, 0, 1, 0),
)


def has_glds_core(T, BK):
    return T in (64, 128) and BK == 16


def expected_variants():
    """Every Variant the harness must report: both cores for the shipped rows that have two."""
    out = []
    for (T, BK, la, lb, nega, tril, groups, sb) in SHIPPED_ROWS:
        for glds in ((1, 0) if has_glds_core(T, BK) else (0,)):
            out.append(Variant(T, BK, glds, la, lb, nega, tril, groups, sb))
    for (T, BK, la, lb, nega, tril, groups, sb) in DEBUG_ROWS:
        out.append(Variant(T, BK, 0, la, lb, nega, tril, groups, sb))
    return out


def two_core_rows():
    return [r for r in SHIPPED_ROWS if has_glds_core(r[0], r[1])]


def opview(arr, layout):
    """[r, k] view of a stored operand: KC element (r, k) at arr[r, k], RC at arr[k, r]."""
    return arr if layout == KC else arr.T


class Case:
    """One harness call: arrays, arguments, expected C.  `inplace`: A, B and C are the same array."""

    def __init__(self, name, v, A, B, C0, tiles_m, tiles_n, m0, n0, kbeg, kend, alpha, beta, preload, inplace=False):
        self.name, self.v, self.A, self.B, self.C0 = name, v, A, B, C0
        self.tiles_m, self.tiles_n, self.m0, self.n0, self.kbeg, self.kend = tiles_m, tiles_n, m0, n0, kbeg, kend
        self.alpha, self.beta, self.preload, self.inplace = alpha, beta, preload, inplace
        self.expected = compute(self, np.float64)

    @property
    def steps(self):
        return (self.kend - self.kbeg) // self.v.BK

    def exact_bound(self):
        """Largest magnitude any intermediate can reach: 8 * 8 * K * |alpha| + 64 * (|beta| + 1)."""
        return 8 * 8 * (self.kend - self.kbeg) * abs(self.alpha) + 64 * (abs(self.beta) + 1)


def compute(case, dtype=np.int64, *, kshift=0, kshort=0, swap_mn=False, la=None, lb=None, flip_sign=False,
            tril_strict=False, swap_ab=False, flip_preload=False, swap_groups=False):
    """The harness's result for `case` from its stored arrays, in `dtype`; the keywords select one wrong computation each.
    kshift: both ends of the K range moved; kshort: K-steps dropped at the end; swap_mn: the operands' row offsets exchanged
    (C stays where it is); la / lb: an operand read in this layout; flip_sign: NEGA inverted; tril_strict: the diagonal of
    the closing triangular block treated as zero (one MFMA group too many skipped); swap_ab: alpha and beta exchanged;
    flip_preload: preload inverted; swap_groups: each group multiplies with the B rows of its workgroup's other group."""
    v = case.v
    T = v.T
    kbeg, kend = case.kbeg + kshift, case.kend + kshift - kshort * v.BK
    am0, bn0 = (case.n0, case.m0) if swap_mn else (case.m0, case.n0)
    Av = opview(case.A, v.la if la is None else la)
    Bv = opview(case.B, v.lb if lb is None else lb)
    sign = -1 if bool(v.nega) != flip_sign else 1
    alpha, beta = (case.beta, case.alpha) if swap_ab else (case.alpha, case.beta)
    preload = bool(case.preload) != flip_preload
    C0 = case.C0.astype(dtype)
    C = C0.copy()
    for p in range(case.tiles_m):
        for q in range(case.tiles_n):
            r, c = case.m0 + p * T, case.n0 + q * T
            ar, bc = am0 + p * T, bn0 + (q ^ 1 if swap_groups else q) * T
            assert kbeg >= 0 and max(ar, bc) + T <= min(Av.shape[0], Bv.shape[0]) and kend <= min(Av.shape[1], Bv.shape[1])
            At = Av[ar:ar + T, kbeg:kend].astype(dtype)
            Bt = Bv[bc:bc + T, kbeg:kend].astype(dtype)
            if tril_strict:
                for k in range(max(kbeg, kend - T), kend):
                    At[k - (kend - T), k - kbeg] = 0
            acc = C0[r:r + T, c:c + T] if preload else np.zeros((T, T), dtype)
            acc = acc + sign * (At @ Bt.T)
            C[r:r + T, c:c + T] = alpha * acc + beta * C0[r:r + T, c:c + T]
    return C


def mutations(case):
    """(name, keywords of compute) of every wrong computation that `case` must tell from the right one.  Left out only
    where the wrong computation does not exist: a K range shifted below 0, m0 and n0 exchanged when they are equal, the
    triangular block on a variant without TRIL, the groups on a one-group variant."""
    v = case.v
    out = [("k+BK", dict(kshift=v.BK)), ("k one step short", dict(kshort=1)),
           ("A in the other layout", dict(la=1 - v.la)), ("B in the other layout", dict(lb=1 - v.lb)),
           ("NEGA inverted", dict(flip_sign=True)), ("alpha and beta exchanged", dict(swap_ab=True)),
           ("preload inverted", dict(flip_preload=True))]
    if case.kbeg >= v.BK:
        out.append(("k-BK", dict(kshift=-v.BK)))
    if case.m0 != case.n0:
        out.append(("m0 and n0 exchanged", dict(swap_mn=True)))
    if v.tril:
        out.append(("TRIL block strictly lower", dict(tril_strict=True)))
    if v.groups == 2:
        out.append(("groups exchanged", dict(swap_groups=True)))
    return out


# ---- generation ---------------------------------------------------------------------------------------------------------
def _rng(v, name):
    # the same data for both cores of a row: the seed leaves `glds` out
    key = repr((v.T, v.BK, v.la, v.lb, v.nega, v.tril, v.groups, v.single_buffer, name))
    return np.random.default_rng(zlib.crc32(key.encode()))


def _ints(rng, shape):
    """Integers in [-8, 8], asymmetric: a quarter of the draws are forced positive."""
    a = rng.integers(-8, 9, size=shape)
    return np.where(rng.random(shape) < 0.25, rng.integers(1, 9, size=shape), a).astype(np.float64)


def _impose_tril(rng, A, v, tiles_m, m0, kbeg, kend):
    """Per tile row, A's last T columns of the K range - block column cc = k - (kend - T), for the k that lie in the range -
    become lower triangular: zeros for cc > r, non-zero (zeros redrawn) for cc <= r."""
    T = v.T
    Av = opview(A, v.la)
    for p in range(tiles_m):
        r0 = m0 + p * T
        for k in range(max(kbeg, kend - T), kend):
            cc = k - (kend - T)
            col = Av[r0:r0 + T, k]
            col[:cc] = 0.0
            low = col[cc:]
            zero = low == 0.0
            low[zero] = rng.integers(1, 9, size=int(zero.sum())) * rng.choice([-1.0, 1.0], size=int(zero.sum()))


def _case(v, name, tiles_m, tiles_n, m0, n0, kbeg, steps, alpha=1, beta=0, preload=0):
    rng = _rng(v, name)
    T = v.T
    kend = kbeg + steps * v.BK
    m1, n1 = m0 + tiles_m * T, n0 + tiles_n * T
    E = max(m1, n1, kend + v.BK) + 16
    A, B = _ints(rng, (E, E + 16)), _ints(rng, (E, E + 16))
    if v.tril:
        _impose_tril(rng, A, v, tiles_m, m0, kbeg, kend)
    C0 = np.full((m1 + T, n1 + 16), SENTINEL)
    C0[m0:m1, n0:n1] = rng.integers(-64, 65, size=(m1 - m0, n1 - n0))
    return Case(name, v, A, B, C0, tiles_m, tiles_n, m0, n0, kbeg, kend, alpha, beta, preload)


def _inplace_case(v, steps):
    """k_syrk_trail's form: one matrix is A, B and C; the tiles sit at blocks (a .. a + 1, b .. b + 1) with a = b + 2 (all
    four strictly below the diagonal), the K range lies left of column block b; acc = C, acc -= A B^T, C = acc."""
    name = "inplace"
    rng = _rng(v, name)
    T = v.T
    kbeg = T * max(1, v.BK // T)        # (a whole K-step in front of the range, as in cases())
    kend = kbeg + steps * v.BK
    b = -(-kend // T)
    n0, m0 = b * T, (b + 2) * T
    E = m0 + 3 * T
    M = _ints(rng, (E, E + 16))
    return Case(name, v, M, M, M, 2, 2, m0, n0, kbeg, kend, 1, 0, 1, inplace=True)


EPILOGUES = ((1, 0), (-1, 1), (-1, 0), (3, -2))


def cases(v):
    """Every case of variant `v` (a Variant or its 9-tuple)."""
    v = Variant(*v)
    T = v.T
    k1 = T * max(1, v.BK // T)          # the smallest non-zero multiple of T that leaves a whole K-step in front of the range
    out = []
    # 1. K-step counts: both parities of the double buffer, the lone step, a long run; offsets at non-zero multiples of T,
    #    m0 != n0, 2 x 2 tiles (so each of a two-group workgroup's groups has a tile of its own)
    for steps in ((1,) if v.single_buffer else (1, 2, 3, 5, 24)):
        out.append(_case(v, f"steps{steps}", 2, 2, T, 2 * T, k1, steps))
    #    and once from the origin, one tile (one workgroup: two tiles side by side on a two-group variant)
    out.append(_case(v, "origin", 1, v.groups, 0, 0, 0, 1 if v.single_buffer else 2))
    # 2. epilogues
    es = 1 if v.single_buffer else 3
    for alpha, beta in EPILOGUES:
        out.append(_case(v, f"alpha{alpha}_beta{beta}", 2, 2, 2 * T, T, 2 * k1, es, alpha, beta, 0))
    out.append(_case(v, "preload", 2, 2, 2 * T, T, 2 * k1, es, 1, 0, 1))
    # 3. in place
    if v.la == KC and v.lb == KC and v.nega:
        out.append(_inplace_case(v, 1 if v.single_buffer else min(3, T // v.BK)))
    # 4. the closing triangular block: K = T (the whole range is the block), T + BK (one plain step before it), 3 T, and T / 2
    #    (the range begins inside the block: kd = kbeg, the first step has rel = T / 2)
    if v.tril:
        for name, klen in (("tril_T", T), ("tril_T+BK", T + v.BK), ("tril_3T", 3 * T), ("tril_T/2", T // 2)):
            out.append(_case(v, name, 2, 2, T, 2 * T, k1, klen // v.BK, -1, 1, 0))
    return out


def real_case(v, seed=2024):
    """Real operands (standard normal), 2 x 2 tiles, 5 K-steps, alpha = 1.5, beta = -0.5: for the same-bits test of a row's
    two cores and the rounding bound.  `expected` is the product formed in np.longdouble."""
    v = Variant(*v)
    rng = np.random.default_rng(seed)
    T = v.T
    tiles, m0, n0, kbeg = 2, T, 2 * T, T
    kend = kbeg + 5 * v.BK
    E = max(m0, n0) + tiles * T + 16
    E = max(E, kend + 16)
    A, B = rng.standard_normal((E, E + 16)), rng.standard_normal((E, E + 16))
    if v.tril:
        Av = opview(A, v.la)
        for p in range(tiles):
            for k in range(max(kbeg, kend - T), kend):
                Av[m0 + p * T:m0 + p * T + (k - (kend - T)), k] = 0.0
    C0 = np.full((m0 + tiles * T + T, n0 + tiles * T + 16), SENTINEL)
    C0[m0:m0 + tiles * T, n0:n0 + tiles * T] = rng.standard_normal((tiles * T, tiles * T))
    c = Case.__new__(Case)
    c.name, c.v, c.A, c.B, c.C0 = "real", v, A, B, C0
    c.tiles_m = c.tiles_n = tiles
    c.m0, c.n0, c.kbeg, c.kend, c.alpha, c.beta, c.preload, c.inplace = m0, n0, kbeg, kend, 1.5, -0.5, 0, False
    c.expected = compute(c, np.longdouble)
    return c


def real_bound(case):
    """Elementwise gamma_n (|alpha| |A| |B|^T + |beta| |C0|) over the tiles, n = K + 3, u = 2^-53: one rounding per product (none
    if fused), K - 1 additions, alpha's and beta's products and the last addition, in any order.  Zero on the guards."""
    v = case.v
    n = (case.kend - case.kbeg) + 3
    u = np.longdouble(2.0) ** -53
    gam = n * u / (1 - n * u)
    T = v.T
    r0, r1 = case.m0, case.m0 + case.tiles_m * T
    c0, c1 = case.n0, case.n0 + case.tiles_n * T
    Aa = np.abs(opview(case.A, v.la)[r0:r1, case.kbeg:case.kend]).astype(np.longdouble)
    Ba = np.abs(opview(case.B, v.lb)[c0:c1, case.kbeg:case.kend]).astype(np.longdouble)
    bound = np.zeros(case.C0.shape, np.longdouble)
    bound[r0:r1, c0:c1] = gam * (abs(case.alpha) * (Aa @ Ba.T) + abs(case.beta) * np.abs(case.C0[r0:r1, c0:c1]))
    return bound
