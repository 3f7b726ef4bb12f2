"""chol_solve may run the leading half of the triangular inverse on a side stream beside the factorisation's late panels
(BOBE_INV_SIDE: 0 off, 1 where inv_side_pays says so, 2 wherever there are two block columns; gp_factor.hip).  Where a
launch runs must not change what it computes, the join must hold from call to call, a member that is not positive
definite must not disturb the others, and the stream and its events go back with the handle.  The library reads its
tuning environment once per process: every variant is a fresh process (tests/test_gpu_paths_bitwise.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# nb = 2 (the smallest split), nb = 3 (halves of different depth, a depth without a leading problem), nb = 6 with a ragged
# last block, nb = 12
SIZES = "200:3:rbf,300:4:matern,641:5:rbf,1500:8:matern"


def _json_of(cmd, extra_env, timeout=600):
    env = dict(os.environ, **extra_env)
    out = subprocess.run([sys.executable] + cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def _digests(extra_env):
    env = dict({"BITS_SIZES": SIZES, "BOBE_LOCKSTEP_MIN_N": "200"}, **extra_env)
    return _json_of([os.path.join(ROOT, "tools", "bits_snapshot.py"), "print"], env)


@pytest.fixture(scope="module")
def unforked():
    base = _digests({"BOBE_INV_SIDE": "0"})
    assert len(base) == 4 * 7 + 4                     # (seven outputs and a sweep per size)
    return base


@pytest.mark.parametrize("mode", ["2", "1"])
@pytest.mark.parametrize("graph", [None, "0"])
def test_fork_does_not_move_a_bit(unforked, mode, graph):
    env = {"BOBE_INV_SIDE": mode}
    if graph is not None:
        env["BOBE_GRAPH_MAX_N"] = graph
    other = _digests(env)
    assert unforked.keys() == other.keys()
    differing = [k for k in unforked if unforked[k] != other[k]]
    assert not differing, (env, differing)


def test_unforked_without_graphs_too(unforked):
    other = _digests({"BOBE_INV_SIDE": "0", "BOBE_GRAPH_MAX_N": "0"})
    assert not [k for k in unforked if unforked[k] != other[k]]


@pytest.fixture(scope="module")
def forced():
    return _json_of([os.path.join(ROOT, "tests", "inverse_side_stream_cases.py")], {"BOBE_INV_SIDE": "2"})


@pytest.mark.parametrize("case,lo,hi", [("bad_lead", 0, 128), ("bad_trail", 128, 300)])
def test_a_member_that_is_not_positive_definite(forced, case, lo, hi):
    r = forced[case]
    print(case, r["column"], r["error"])
    assert r["ret"] == 1 and r["status"] == [0, 1, 0], r          # BOBE_NOT_PD for the middle member only
    assert r["column"] is not None and lo <= r["column"] < hi, r   # the failing pivot lies in the half the case is about
    assert r["bad_mll_nan"] and r["bad_grad_nan"] and r["bad_single_nan"]
    assert r["members"] == r["singles"]                            # the others: the single evaluation's bits


def test_consecutive_evaluations_keep_their_bits(forced):
    calls = forced["repeat"]
    assert len(calls) == 5 and len(set(calls[:4])) == 4
    assert calls[4] == calls[0]                       # (a missing join shows as a changed Tmp / Linv)


@pytest.mark.parametrize("which", [0, 1])
def test_entry_points_sharing_a_handle_keep_their_bits(forced, which):
    """What the factorisation hands to the inverse travels by value: no entry point finds what another one left on the
    handle's own workspace.  N = 300, d = 3 (three block columns, ragged) and N = 641, d = 5, the fork forced."""
    r = forced["interleave"][which]
    assert r["steps"] == ["mll_data", "fast_update_cholesky", "gp_mll", "set_chol", "refit", "loo", "mll_data_batch",
                          "sample_posterior", "mll_data again"]
    assert all(s["finite"] for s in r["shared"] + r["single"] + r["free"]), r["steps"]
    differing = [name for name, a, b in zip(r["steps"], r["shared"], r["single"]) if a["hex"] != b["hex"]]
    assert not differing, differing                    # each call: the bits it has alone on a fresh handle
    assert [s["hex"] for s in r["shared"][1:3]] == [s["hex"] for s in r["free"]]      # ... and on a data-less one
    assert r["shared"][8]["hex"] == r["shared"][0]["hex"]                             # the last mll_data equals the first


def test_handles_return_the_side_stream(forced):
    # one leaked N x N buffer per handle would be 20 x 1.2 MB; the allowance is the allocator's granularity
    assert forced["lifetime"] < 4 << 20, f"{forced['lifetime'] / 2 ** 20:.1f} MiB over twenty handles"
