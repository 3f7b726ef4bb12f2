"""Child process of tests/test_gpu_inverse_side_stream.py (the library reads BOBE_INV_SIDE once per process: the parent sets
it to 2, the fork forced wherever a matrix has two block columns).  Runs the cases that go through the Python binding and
prints one JSON line:
  bad_lead / bad_trail   a lock-step batch of three whose middle member is not positive definite, the failing pivot in the
                         leading / the trailing half of the factor
  repeat                 four batch evaluations at different theta, then the first again
  interleave             the entry points that share a handle's own workspace and its installed factor, one after the other
                         on one handle, against each of them alone on a fresh handle (N = 300, d = 3 and N = 641, d = 5)
  lifetime               twenty create / evaluate / destroy rounds and the device memory they leave behind"""
import ctypes as C
import gc
import json
import os
import re
import sys

import numpy as np
import torch  # (before the library: both bring a HIP runtime, and torch finds no device when it comes second)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bobe_amd import GP, _lib  # noqa: E402

N, D = 300, 3            # three block columns: the leading half is block 0 (columns 0 .. 127), the trailing half the rest


def batch_with_status(gp, ls, kv):
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    kv = np.ascontiguousarray(kv, dtype=np.float64)
    B = ls.shape[0]
    mll, grad, status = np.empty(B), np.empty((B, gp.ndim + 1)), np.zeros(B, dtype=np.int32)
    st = gp._lib.bobe_gp_mll_batch(gp._h, B, _lib.ptr(ls), _lib.ptr(kv), _lib.ptr(mll), _lib.ptr(grad),
                                   C.c_void_p(status.ctypes.data))
    return st, mll, grad, status, _lib.last_error()


def hexes(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes().hex()


def bad_member_case(dup_rows, src_rows):
    """Rows dup_rows repeat rows src_rows in every coordinate but the first.  A member whose first length scale is 1e30
    does not see that coordinate: its kernel matrix has exactly repeated rows there, and with a noise of 1e-12 under a
    kernel variance of 1e6 the pivots of the repeated rows are rounding noise around zero - the factorisation fails in
    their neighbourhood (the test reads the reported column and asserts only which half of the factor it lies in)."""
    rng = np.random.default_rng(7)
    X = rng.uniform(size=(N, D))
    X[dup_rows, 1:] = X[src_rows, 1:]
    y = np.sin(3.0 * X.sum(1))
    gp = GP(X, y, noise=1e-12, kernel="matern", lengthscales=np.full(D, 0.3))
    ls = np.array([[0.30, 0.32, 0.28], [1e30, 0.30, 0.30], [0.27, 0.31, 0.33]])
    kv = np.array([1.1, 1e6, 0.9])
    st, mll, grad, status, err = batch_with_status(gp, ls, kv)
    col = re.search(r"at column (\d+)", err)
    singles = [gp.mll_data(ls[b], kv[b]) for b in (0, 2)]
    bad_single = gp.mll_data(ls[1], kv[1])
    return {"ret": int(st), "status": status.tolist(), "column": int(col.group(1)) if col else None, "error": err,
            "bad_mll_nan": bool(np.isnan(mll[1])), "bad_grad_nan": bool(np.all(np.isnan(grad[1]))),
            "bad_single_nan": bool(np.isnan(bad_single[0]) and np.all(np.isnan(bad_single[1]))),
            "members": [hexes(mll[b]) + hexes(grad[b]) for b in (0, 2)],
            "singles": [hexes(m) + hexes(g) for m, g in singles]}


def repeat_case():
    n, d = 641, 5                                   # six block columns, the last one ragged
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=n)
    gp = GP(X, y, noise=1e-5, kernel="rbf", lengthscales=np.full(d, 0.5))
    calls = []
    for r in (0, 1, 2, 3, 0):
        ls = np.full((4, d), 0.35 + 0.05 * r) + 0.02 * np.arange(4)[:, None]
        mll, grad = gp.mll_data_batch(ls, np.full(4, 1.0 + 0.1 * r))
        calls.append(hexes(mll) + hexes(grad))
    return calls


def lifetime_case():
    def one_round(seed):
        rng = np.random.default_rng(seed)
        X = rng.uniform(size=(N, D))
        gp = GP(X, np.sin(X.sum(1)), noise=1e-6, lengthscales=np.full(D, 0.5))
        gp.mll_data_batch(np.full((4, D), 0.4) + 0.01 * np.arange(4)[:, None], np.ones(4))
        gp.mll_data(np.full(D, 0.45), 1.2)
        del gp
        gc.collect()

    one_round(0)
    one_round(1)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for s in range(20):
        one_round(2 + s)
    torch.cuda.synchronize()
    return int(free0 - torch.cuda.mem_get_info(0)[0])


def interleave_case(n, d, kern):
    """Nine calls in sequence on ONE handle - they share its own evaluation workspace and the installed factor - and each
    of them again alone on a fresh handle (`single`); the two free functions also by the binding's own route, a data-less
    handle per call (`free`).  A step is (name, call(gp) -> arrays); the saved factor and the matrices are made up front."""
    from bobe_amd.gp import fast_update_cholesky, gp_mll
    rng = np.random.default_rng(100 + n)
    X = rng.uniform(size=(n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=n)
    xq = rng.uniform(size=(200, d))
    kvec = 0.5 * np.exp(-np.sum((X - 0.5) ** 2, axis=1))

    def fresh():
        return GP(X, y, noise=1e-5, kernel=kern, lengthscales=np.full(d, 0.5))

    saved = fresh()
    L, alpha = np.array(saved.cholesky), np.array(saved.alphas).reshape(-1)
    K, ys = L @ L.T, np.array(saved.train_y).reshape(-1)
    ls1, ls4 = np.full(d, 0.45), np.full((4, d), 0.4) + 0.03 * np.arange(4)[:, None]

    # the free functions' entry points on g's handle (a handle with data takes matrices of its data's size)
    def row_update(g):
        v, diag = np.empty(n), C.c_double(0.0)
        _lib.check(g._lib.bobe_gp_chol_row_update(g._h, _lib.ptr(L), n, _lib.ptr(kvec), 2.0, _lib.ptr(v), C.byref(diag)),
                   "bobe_gp_chol_row_update")
        return v, diag.value

    def mll_of_k(g):
        mll = C.c_double(0.0)
        _lib.check(g._lib.bobe_gp_mll_from_k(g._h, _lib.ptr(K), n, _lib.ptr(ys), C.byref(mll)), "bobe_gp_mll_from_k")
        return (mll.value,)

    def restore(g):
        _lib.check(g._lib.bobe_gp_set_chol(g._h, _lib.ptr(L), _lib.ptr(alpha)), "bobe_gp_set_chol")
        g._chol_cache = g._alpha_cache = None
        return (g.cholesky, g.alphas) + g.predict_batched(xq)

    def refit(g):
        g.recompute_cholesky()
        return (g.cholesky, g.alphas) + g.predict_batched(xq)

    def loo(g):
        r = g.loo()
        return r["mean"], r["var"], r["lpd"], r["elpd"]

    steps = [("mll_data", lambda g: g.mll_data(ls1, 1.3)),
             ("fast_update_cholesky", row_update),
             ("gp_mll", mll_of_k),
             ("set_chol", restore),
             ("refit", refit),
             ("loo", loo),
             ("mll_data_batch", lambda g: g.mll_data_batch(ls4, np.ones(4))),
             ("sample_posterior", lambda g: (g.sample_posterior(xq, n_samples=3, seed=20240),)),
             ("mll_data again", lambda g: g.mll_data(ls1, 1.3))]

    def digest(arrays):
        flat = np.concatenate([np.ravel(np.asarray(a, dtype=np.float64)) for a in arrays])
        return {"hex": hexes(flat), "finite": bool(np.all(np.isfinite(flat)))}

    gp = fresh()
    shared = [digest(call(gp)) for _, call in steps]
    single = [digest(call(fresh())) for _, call in steps]
    new_row = fast_update_cholesky(L, kvec, 2.0)[n]          # the binding's own route: a data-less handle per call
    free = [digest((new_row[:n], new_row[n])), digest((gp_mll(K, ys, n),))]
    return {"steps": [name for name, _ in steps], "shared": shared, "single": single, "free": free}


if __name__ == "__main__":
    out = {"bad_lead": bad_member_case(np.arange(40, 100), np.arange(0, 60)),
           "bad_trail": bad_member_case(np.arange(200, 300), np.arange(0, 100)),
           "repeat": repeat_case(),
           "interleave": [interleave_case(300, 3, "matern"), interleave_case(641, 5, "rbf")],
           "lifetime": lifetime_case()}
    print(json.dumps(out))
