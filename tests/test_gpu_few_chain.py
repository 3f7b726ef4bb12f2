"""The few-candidate chain of bobe_gp_wip_grad (C <= 16: wg_front -> k_wg_cross -> k_wg_rows<., ., 2> -> k_wg_final) through
the raw ABI, on bits: what a candidate returns depends on the candidate alone - not on C or its place in the group, not on
which of the four outputs were asked for, not on where the outputs go home (the pinned result block, one staged block, the
caller's device memory) and not on the kind of the pointers.

Shapes, the smallest at which every stage has a ragged edge (noise 1e-6, lengthscales 0.7):

    N = 130, d = 3,  rbf      Np = 256, 33 rows workgroups (the last with 2 of 4 rows), d cap 8
    N = 257, d = 9,  matern   Np = 384, 65 rows workgroups (the last with 1 row),       d cap 16; once more with
                              refine_kappa = 0 (wg_front's refinement step)
    N = 130, d = 17, rbf      Np = 256, 33 rows workgroups,                             d cap 32

    M = 70: two cross workgroups, the second with 6 live points; M = 33: the second workgroup empty.

Output sizes at d = 9: C = 4 is 80 doubles and C = 6 with dwipv alone 54 (both in the pinned result block), C = 16 is 320 (one
staged block, one copy)."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_weighted_criteria import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

NOISE, ELL = 1e-6, 0.7
SHAPES = [(130, 3, "rbf", False), (257, 9, "matern", False), (257, 9, "matern", True), (130, 17, "rbf", False)]
SHAPE_IDS = [f"N{n}_d{d}_{k}" + ("_refining" if r else "") for n, d, k, r in SHAPES]
MS = [70, 33]
NAMES = ("wipv", "wipstd", "dwipv", "dwipstd")


@functools.lru_cache(maxsize=None)
def _gp(n, d, kernel, refine):
    from bobe_amd import GP
    rng = np.random.default_rng(100 * n + d)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    gp = GP(X, y, noise=NOISE, kernel=kernel, lengthscales=np.full(d, ELL))
    if refine:
        gp.refine_kappa = 0.0
        gp.recompute_cholesky()
        assert gp.refining
    return gp


@functools.lru_cache(maxsize=None)
def _points(d, m):
    """(16 candidates, m integration points) of dimension d"""
    rng = np.random.default_rng(7000 + 10 * d + m)
    return rng.uniform(0.1, 0.9, size=(16, d)), rng.uniform(size=(m, d))


def _shape(c, d):
    return {"wipv": (c,), "wipstd": (c,), "dwipv": (c, d), "dwipstd": (c, d)}


def _raw(gp, cand, c, Z, m, outs):
    """bobe_gp_wip_grad on outs = (wipv, wipstd, dwipv, dwipstd): NumPy arrays, torch tensors or None"""
    from bobe_amd import _lib
    st = gp._lib.bobe_gp_wip_grad(gp._h, _lib.ptr(cand), c, _lib.ptr(Z), m, float(gp.y_std), *[_lib.ptr(a) for a in outs])
    assert st == 0, gp._lib.bobe_last_error()


def _host_call(gp, cand, Z, want=NAMES):
    """name -> array of the outputs in `want`, host pointers; what is not asked for is passed as NULL.  (The arrays start as
    NaN: an output that was not written cannot pass for a result.)"""
    c, d = cand.shape
    outs = {k: np.full(_shape(c, d)[k], np.nan) for k in want}
    _raw(gp, np.ascontiguousarray(cand), c, Z, Z.shape[0], [outs.get(k) for k in NAMES])
    return outs


@functools.lru_cache(maxsize=None)
def _all_four(shape, m, c):
    """the all-host, all-four call of the first c candidates: computed once, shared, never written to"""
    n, d, kernel, refine = shape
    cand, Z = _points(d, m)
    r = _host_call(_gp(n, d, kernel, refine), cand[:c], Z)
    for a in r.values():
        assert np.all(np.isfinite(a))
        a.flags.writeable = False
    return r


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_a_row_of_sixteen_is_the_candidate_alone(shape, m):
    n, d, kernel, refine = shape
    gp = _gp(n, d, kernel, refine)
    cand, Z = _points(d, m)
    grp = _all_four(shape, m, 16)
    for i in range(16):
        one = _host_call(gp, cand[i:i + 1], Z)
        for k in NAMES:
            assert same_bits(grp[k][i:i + 1], one[k]), (i, k)


SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(NAMES, r)]


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("c", [4, 16])
def test_a_subset_of_the_outputs_has_the_bits_of_all_four(c, m):
    shape = SHAPES[1]
    n, d, kernel, refine = shape
    gp = _gp(n, d, kernel, refine)
    cand, Z = _points(d, m)
    full = _all_four(shape, m, c)
    assert len(SUBSETS) == 15
    for want in SUBSETS:
        got = _host_call(gp, cand[:c], Z, want)
        for k in want:
            assert same_bits(got[k], full[k]), (want, k)


@pytest.mark.parametrize("m", MS)
def test_one_gradient_of_six_candidates(m):
    shape = SHAPES[1]
    n, d, kernel, refine = shape
    cand, Z = _points(d, m)
    got = _host_call(_gp(n, d, kernel, refine), cand[:6], Z, ("dwipv",))
    assert same_bits(got["dwipv"], _all_four(shape, m, 16)["dwipv"][:6])


@pytest.mark.parametrize("c", [4, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_device_pointers_have_the_host_bits(shape, c):
    import torch
    n, d, kernel, refine = shape
    m = MS[0]
    gp = _gp(n, d, kernel, refine)
    cand, Z = _points(d, m)
    full = _all_four(shape, m, c)
    sizes = _shape(c, d)

    def dev_out(k):
        return torch.full(sizes[k], float("nan"), dtype=torch.float64, device="cuda")

    # everything on the device: candidates, integration points and the four outputs
    dc, dz = torch.as_tensor(np.ascontiguousarray(cand[:c]), device="cuda"), torch.as_tensor(Z, device="cuda")
    outs = [dev_out(k) for k in NAMES]
    _raw(gp, dc, c, dz, m, outs)
    torch.cuda.synchronize()
    for k, a in zip(NAMES, outs):
        assert same_bits(a.cpu().numpy(), full[k]), k
    # a mix: host inputs, the scores to host arrays, the gradients to device memory
    outs = [np.full(sizes["wipv"], np.nan), np.full(sizes["wipstd"], np.nan), dev_out("dwipv"), dev_out("dwipstd")]
    _raw(gp, np.ascontiguousarray(cand[:c]), c, Z, m, outs)
    torch.cuda.synchronize()
    for k, a in zip(NAMES, outs):
        assert same_bits(a if isinstance(a, np.ndarray) else a.cpu().numpy(), full[k]), k
