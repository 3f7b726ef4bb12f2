"""The sweep's 128-tile GEMMs (k_trimul, k_cross_vv<128>) run on one of two tile cores, selected once per process by
BOBE_GEMM_GLDS: operands loaded straight into LDS with fragments read a sub-step ahead (1, the default) or staged through
registers (0).  Both issue the same MFMAs in the same K order, so every factorisation-dependent output and every sweep
output must carry the same bits; each variant runs tools/bits_snapshot.py in its own process, as
tests/test_gpu_paths_bitwise.py does for the other switches."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digests(extra_env, timeout=900):
    env = dict(os.environ, **extra_env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bits_snapshot.py"), "print"], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def _same(base, other):
    assert base.keys() == other.keys()
    differing = [k for k in base if base[k] != other[k]]
    assert not differing, differing


def test_both_tile_cores_give_the_same_bits_at_small_sizes():
    env = {"BITS_MAX_N": "2048"}          # three-chunk sweeps (fused cross tiles) at every size
    base = _digests(dict(env, BOBE_GEMM_GLDS="0"))
    assert sum(k.startswith("sw_") for k in base) == 6
    _same(base, _digests(dict(env, BOBE_GEMM_GLDS="1")))


def test_both_tile_cores_give_the_same_bits_on_a_multi_chunk_sweep_at_n4096():
    env = {"BITS_SIZES": "4096:8:rbf", "BITS_BIG_SWEEP": "1"}
    base = _digests(dict(env, BOBE_GEMM_GLDS="0"))
    assert "sw_4096" in base
    _same(base, _digests(dict(env, BOBE_GEMM_GLDS="1")))
