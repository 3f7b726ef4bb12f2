"""bobe_gp_factor adopts the factor an evaluation left in its workspace (a lock-step batch slot, an evaluation slot, the single
evaluation's own buffers) when that evaluation ran at the same hyper-parameters, bit for bit, on the same data: the fit has
just evaluated the theta the refactor asks for.  The adopted state must be the bits a fresh factorisation gives - L, alpha,
the sweep, the refinement decision, the not-PD status and its text - and every kind of miss must factorise."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORISED, BATCH, SLOT, SINGLE = 0, 1, 2, 3


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _lib():
    from bobe_amd import _lib as L
    return L, L.load()


def _problem(n, d, seed=0, dup=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    if dup:
        X[-dup:] = X[:dup]                              # repeated points: K(X, X) is singular without noise
    y = np.sin(3.0 * X).sum(axis=1) + 0.1 * rng.normal(size=n)
    return np.ascontiguousarray(X), np.ascontiguousarray(y)


def _handle(X, y, noise, kern=0, pivot_ulp=None):
    """a handle on (X, y) whose evaluations use `noise` (they take it from the handle's hyper-parameters)"""
    L, lib = _lib()
    h = C.c_void_p()
    L.check(lib.bobe_gp_create(C.byref(h), 0, kern, X.shape[1]), "create")
    if pivot_ulp is not None:
        L.check(lib.bobe_gp_set_pivot_floor_ulp(h, float(pivot_ulp)), "pivot floor")
    L.check(lib.bobe_gp_set_data(h, _p(X), _p(y), X.shape[0]), "set_data")
    L.check(lib.bobe_gp_set_hyper(h, _p(np.ones(X.shape[1])), 1.0, float(noise)), "set_hyper")
    return h


def _factor(h, ls, kvar, noise):
    L, lib = _lib()
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    L.check(lib.bobe_gp_set_hyper(h, _p(ls), float(kvar), float(noise)), "set_hyper")
    st = lib.bobe_gp_factor(h)
    assert st >= 0, L.last_error()
    return st, (L.last_error() if st == L.BOBE_NOT_PD else None), lib.bobe_debug_factor_source(h)


def _state(h, n, cand, Z):
    """what a consumer sees of the installed factor: L, alpha, the refinement decision and a whole sweep"""
    L, lib = _lib()
    Lc, al = np.empty((n, n)), np.empty(n)
    L.check(lib.bobe_gp_get_chol(h, _p(Lc), _p(al)), "get_chol")
    active = C.c_int()
    L.check(lib.bobe_gp_get_refine(h, None, C.byref(active)), "get_refine")
    out = {"L": Lc, "alpha": al, "refine": active.value}
    if cand is not None:
        c = cand.shape[0]
        wipv, wipstd, mean, var = np.empty(c), np.empty(c), np.empty(c), np.empty(c)
        av, asd, mv, ms = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        L.check(lib.bobe_gp_wip_sweep(h, _p(cand), c, _p(Z), Z.shape[0], 1.0, _p(wipv), _p(wipstd), _p(mean), _p(var),
                                      C.byref(av), C.byref(mv), C.byref(asd), C.byref(ms)), "sweep")
        out.update(wipv=wipv, wipstd=wipstd, mean=mean, var=var, argmins=(av.value, asd.value),
                   mins=(mv.value, ms.value))
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def _fresh(X, y, ls, kvar, noise, cand, Z, kern=0, pivot_ulp=None):
    _, lib = _lib()
    h = _handle(X, y, noise, kern, pivot_ulp)
    try:
        st, txt, src = _factor(h, ls, kvar, noise)
        assert src == FACTORISED
        return st, txt, _state(h, X.shape[0], cand, Z)
    finally:
        lib.bobe_gp_destroy(h)


def _thetas(d, B, seed=1):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.exp(rng.uniform(np.log(0.3), np.log(1.2), size=(B, d)))), \
        np.ascontiguousarray(np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=B)))


def _batch(h, ls, kv, grad=True):
    L, lib = _lib()
    B, d = ls.shape
    mll, g, st = np.empty(B), (np.empty((B, d + 1)) if grad else None), np.zeros(B, np.int32)
    r = lib.bobe_gp_mll_batch(h, B, _p(ls), _p(kv), _p(mll), _p(g), C.c_void_p(st.ctypes.data))
    assert r >= 0, L.last_error()
    return st


@pytest.mark.parametrize("n", [100, 1024, 4096])
def test_every_evaluation_path_hands_over_the_bits_of_a_fresh_factor(n):
    L, lib = _lib()
    d, noise = 6, 1e-6
    X, y = _problem(n, d)
    rng = np.random.default_rng(2)
    cand, Z = np.ascontiguousarray(rng.uniform(size=(1536, d))), np.ascontiguousarray(rng.uniform(size=(64, d)))
    ls, kv = _thetas(d, 7)
    h = _handle(X, y, noise)
    try:
        assert (_batch(h, ls[:4], kv[:4]) == 0).all()                 # lock step: theta 2 sits in batch slot 2
        m, g = C.c_double(), np.empty(d + 1)
        L.check(lib.bobe_gp_mll_submit(h, 1, _p(ls[4]), float(kv[4]), 1), "submit")
        L.check(lib.bobe_gp_mll_wait(h, 1, C.byref(m), _p(g)), "wait")
        L.check(lib.bobe_gp_mll(h, _p(ls[5]), float(kv[5]), C.byref(m), _p(g)), "mll")
        L.check(lib.bobe_gp_mll(h, _p(ls[6]), float(kv[6]), C.byref(m), None), "mll (value only)")
        for k, source in ((2, BATCH), (4, SLOT), (6, SINGLE), (0, BATCH)):
            st, txt, src = _factor(h, ls[k], kv[k], noise)
            assert (st, src) == (0, source), k
            fst, ftxt, fresh = _fresh(X, y, ls[k], kv[k], noise, cand, Z)
            assert (st, txt) == (fst, ftxt)
            _same(_state(h, n, cand, Z), fresh)
        # theta 5's single evaluation was overwritten by theta 6's: factorised again
        assert _factor(h, ls[5], kv[5], noise)[2] == FACTORISED
    finally:
        lib.bobe_gp_destroy(h)


def test_every_kind_of_miss_factorises():
    L, lib = _lib()
    n, d, noise = 300, 4, 1e-6
    X, y = _problem(n, d, seed=3)
    ls, kv = _thetas(d, 6, seed=4)
    h = _handle(X, y, noise)
    try:
        _batch(h, ls[:4], kv[:4])
        bumped = ls[1].copy()
        bumped[0] = np.nextafter(bumped[0], np.inf)               # one ulp in one length scale
        for what, (l_, k_, n_) in {"ls + 1 ulp": (bumped, kv[1], noise),
                                   "kvar + 1 ulp": (ls[1], np.nextafter(kv[1], 0.0), noise),
                                   "other noise": (ls[1], kv[1], 2 * noise)}.items():
            st, txt, src = _factor(h, l_, k_, n_)
            assert src == FACTORISED, what
            fst, ftxt, fresh = _fresh(X, y, l_, k_, n_, None, None)
            assert (st, txt) == (fst, ftxt), what
            _same(_state(h, n, None, None), fresh)
        assert _factor(h, ls[1], kv[1], noise)[2] == BATCH         # (the batch slot is still intact)
        # a later, narrower batch overwrites slots 0 and 1 only
        _batch(h, ls[4:6], kv[4:6])
        assert _factor(h, ls[1], kv[1], noise)[2] == FACTORISED
        st, _, src = _factor(h, ls[3], kv[3], noise)
        assert src == BATCH
        _same(_state(h, n, None, None), _fresh(X, y, ls[3], kv[3], noise, None, None)[2])
        # new data - even the same data - and a rank-b append make every record stale
        L.check(lib.bobe_gp_set_data(h, _p(X), _p(y), n), "set_data")
        assert _factor(h, ls[3], kv[3], noise)[2] == FACTORISED
        m = C.c_double()
        L.check(lib.bobe_gp_mll(h, _p(ls[2]), float(kv[2]), C.byref(m), None), "mll")
        Xn, yn = _problem(n + 3, d, seed=3)
        L.check(lib.bobe_gp_append(h, _p(np.ascontiguousarray(Xn[n:])), 3, _p(yn)), "append")
        st, _, src = _factor(h, ls[2], kv[2], noise)
        assert src == FACTORISED
        _same(_state(h, n + 3, None, None), _fresh(Xn, yn, ls[2], kv[2], noise, None, None)[2])
    finally:
        lib.bobe_gp_destroy(h)


def test_matern_adopts_its_own_evaluations():
    _, lib = _lib()
    n, d, noise = 700, 5, 1e-6
    X, y = _problem(n, d, seed=5)
    rng = np.random.default_rng(6)
    cand, Z = np.ascontiguousarray(rng.uniform(size=(1024, d))), np.ascontiguousarray(rng.uniform(size=(32, d)))
    ls, kv = _thetas(d, 3, seed=7)
    h = _handle(X, y, noise, kern=1)
    try:
        _batch(h, ls, kv, grad=False)                               # (value-only evaluations hold the same factor)
        st, txt, src = _factor(h, ls[1], kv[1], noise)
        assert src == BATCH
        fst, ftxt, fresh = _fresh(X, y, ls[1], kv[1], noise, cand, Z, kern=1)
        assert (st, txt) == (fst, ftxt)
        _same(_state(h, n, cand, Z), fresh)
    finally:
        lib.bobe_gp_destroy(h)


@pytest.mark.parametrize("noise,dup", [(-1.0, 0), (0.0, 20)])
def test_a_not_positive_definite_evaluation_gives_the_same_status_and_text(noise, dup):
    """a negative first pivot (noise -1 against kernel variance <= 0.6: the info word's column), and repeated points without
    noise (a pivot at the rounding level: the rank test, whose text carries the pivot)"""
    L, lib = _lib()
    n, d = 260, 3
    X, y = _problem(n, d, seed=8, dup=dup)
    ls, kv = _thetas(d, 2, seed=9)
    kv = np.ascontiguousarray(0.3 * kv)
    h = _handle(X, y, noise, pivot_ulp=64)
    try:
        st = _batch(h, ls, kv)
        if noise < 0:
            assert (st == L.BOBE_NOT_PD).all()
        for k in range(2):
            fst, ftxt, fresh = _fresh(X, y, ls[k], kv[k], noise, None, None, pivot_ulp=64)
            assert fst == st[k]
            got, txt, src = _factor(h, ls[k], kv[k], noise)
            assert src == BATCH and (got, txt) == (fst, ftxt)
            _same(_state(h, n, None, None), fresh)                   # (all NaN when not PD)
    finally:
        lib.bobe_gp_destroy(h)


def test_an_ill_conditioned_factor_makes_the_same_refinement_decision():
    """kernel variance 50, noise 1e-8 and long length scales: (kvar + noise) / smallest pivot passes 1e6 and the sweep takes the
    blocked substitution - decided from the adopted evaluation's smallest pivot, as from a fresh factor's"""
    _, lib = _lib()
    n, d = 400, 2
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(n, d))
    y = np.ascontiguousarray(np.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.5 * X[:, -1])
    rng = np.random.default_rng(11)
    cand, Z = np.ascontiguousarray(rng.uniform(size=(512, d))), np.ascontiguousarray(rng.uniform(size=(32, d)))
    ls, kv = np.full((2, d), 1.5), np.array([50.0, 40.0])
    h = _handle(X, y, 1e-8)
    try:
        _batch(h, ls, kv)
        st, txt, src = _factor(h, ls[0], kv[0], 1e-8)
        assert src == BATCH
        fst, ftxt, fresh = _fresh(X, y, ls[0], kv[0], 1e-8, cand, Z)
        assert fresh["refine"] == 1
        assert (st, txt) == (fst, ftxt)
        _same(_state(h, n, cand, Z), fresh)
    finally:
        lib.bobe_gp_destroy(h)


def test_the_process_switch_turns_adoption_off():
    code = ("import ctypes as C, numpy as np\n"
            "from bobe_amd import _lib as L\n"
            "lib = L.load(); h = C.c_void_p(); d = 3\n"
            "X = np.random.default_rng(0).uniform(size=(200, d)); y = X.sum(1)\n"
            "L.check(lib.bobe_gp_create(C.byref(h), 0, 0, d), 'c'); L.check(lib.bobe_gp_set_data(h, L.ptr(X), L.ptr(y), 200), 's')\n"
            "L.check(lib.bobe_gp_set_hyper(h, L.ptr(np.ones(d)), 1.0, 1e-6), 'h')\n"
            "ls = np.full((2, d), 0.5); kv = np.ones(2); m = np.empty(2)\n"
            "L.check(lib.bobe_gp_mll_batch(h, 2, L.ptr(ls), L.ptr(kv), L.ptr(m), None, None), 'b')\n"
            "L.check(lib.bobe_gp_set_hyper(h, L.ptr(ls[0]), 1.0, 1e-6), 'h'); L.check(lib.bobe_gp_factor(h), 'f')\n"
            "print('source', lib.bobe_debug_factor_source(h)); lib.bobe_gp_destroy(h)\n")
    for env, want in (({"BOBE_FACTOR_REUSE": "0"}, FACTORISED), ({}, BATCH)):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert f"source {want}" in out.stdout, (env, out.stdout)


def _mll(h, ls, kv, d):
    L, lib = _lib()
    m, g = C.c_double(), np.empty(d + 1)
    L.check(lib.bobe_gp_mll(h, _p(ls), float(kv), C.byref(m), _p(g)), "mll")
    return m.value, g


def _walk(batch_on_slots):
    """One handle through a change of Np, then a change of N at the same Np; after each, an evaluation on slot 1, a batch of
    three and a single evaluation, then bobe_gp_factor at one theta of each.  Runs in a process of its own (__main__ below)."""
    L, lib = _lib()
    d, noise = 3, 1e-6
    ls, kv = _thetas(d, 5, seed=12)
    rng = np.random.default_rng(13)
    cand, Z = np.ascontiguousarray(rng.uniform(size=(256, d))), np.ascontiguousarray(rng.uniform(size=(32, d)))
    # theta 2 is member 1 of the batch: batch member 1 in lock step; slot 1 when the batch runs on slots (member i takes slot
    # i), where it overwrote theta 0's factor - no workspace holds theta 0 then.  Theta 4 stays in the handle's own workspace.
    want = {2: SLOT if batch_on_slots else BATCH, 0: FACTORISED if batch_on_slots else SLOT, 4: SINGLE}
    X0, y0 = _problem(200, d, seed=14)            # Np 256
    X1, y1 = _problem(300, d, seed=15)            # Np 384: every workspace reallocates, a captured graph's signature is stale
    X2, y2 = _problem(302, d, seed=15)            # the same rows and two more: Np stays, only N changes
    assert np.array_equal(X2[:300], X1)
    h = _handle(X0, y0, noise)
    try:
        for step, (X, y) in enumerate(((X0, y0), (X1, y1), (X2, y2))):
            n = X.shape[0]
            if step == 1:
                L.check(lib.bobe_gp_set_data(h, _p(X), _p(y), n), "set_data")
            elif step == 2:
                L.check(lib.bobe_gp_append(h, _p(np.ascontiguousarray(X[300:])), 2, _p(y)), "append")
            got = {}
            m, g = C.c_double(), np.empty(d + 1)
            L.check(lib.bobe_gp_mll_submit(h, 1, _p(ls[0]), float(kv[0]), 1), "submit")
            L.check(lib.bobe_gp_mll_wait(h, 1, C.byref(m), _p(g)), "wait")
            got[0] = (m.value, g)
            mb, gb, st = np.empty(3), np.empty((3, d + 1)), np.zeros(3, np.int32)
            L.check(lib.bobe_gp_mll_batch(h, 3, _p(ls[1:4]), _p(kv[1:4]), _p(mb), _p(gb), C.c_void_p(st.ctypes.data)), "batch")
            assert (st == 0).all()
            for k in range(3):
                got[1 + k] = (mb[k], gb[k])
            got[4] = _mll(h, ls[4], kv[4], d)
            ref = _handle(X, y, noise)
            try:
                for k in range(5):
                    mr, gr = _mll(ref, ls[k], kv[k], d)
                    assert got[k][0] == mr and np.array_equal(got[k][1], gr), (step, k, got[k], mr, gr)
            finally:
                lib.bobe_gp_destroy(ref)
            for k in (2, 0, 4):
                st_, txt, src = _factor(h, ls[k], kv[k], noise)
                assert (st_, src) == (0, want[k]), (step, k, st_, src)
                fst, ftxt, fresh = _fresh(X, y, ls[k], kv[k], noise, cand, Z)
                assert (st_, txt) == (fst, ftxt)
                _same(_state(h, n, cand, Z), fresh)
    finally:
        lib.bobe_gp_destroy(h)
    print("walk ok")


@pytest.mark.parametrize("env", [{}, {"BOBE_LOCKSTEP_MIN_N": "100000"}], ids=["lockstep", "slots"])
def test_one_handle_keeps_its_workspaces_right_across_a_change_of_np_and_of_n(env):
    """set_data to another Np, then an append that changes N alone: the slot, the batch and the handle's own workspace must
    each return the bits of bobe_gp_mll on a fresh handle and hand bobe_gp_factor the bits of a fresh factorisation.  With
    BOBE_LOCKSTEP_MIN_N above the sizes the batch runs on the evaluation slots (as graph replays at these sizes).  The library
    reads its environment once per process: each form runs in a child."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "walk", "slots" if env else "lockstep"],
                         env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "walk ok" in out.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert sys.argv[1] == "walk"
    _walk(sys.argv[2] == "slots")
