"""The 64-tile GEMMs (k_syrk_trail<64, 16>, k_trtri_T/R<64>, k_lauum_grad<., ., 64>, k_cross_vv<64>, k_trimul_v64,
k_trimul_t64) run on one of two tile cores, selected once per process by BOBE_GEMM64_GLDS: operands loaded straight into
LDS with fragments read a sub-step ahead (1, the default) or staged through registers (0).  Both issue the same MFMAs in
the same K order, so every factorisation-dependent output, every gradient and every sweep output must carry the same
bits.  Each variant runs tools/bits_snapshot.py in its own process, as tests/test_gpu_gemm_loop_bitwise.py does for the
128-tile core."""
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


def _same_under_both_cores(env):
    base = _digests(dict(env, BOBE_GEMM64_GLDS="0"))
    other = _digests(dict(env, BOBE_GEMM64_GLDS="1"))
    assert base.keys() == other.keys()
    differing = [k for k in base if base[k] != other[k]]
    assert not differing, differing
    return base


def test_both_64_tile_cores_give_the_same_bits_at_small_sizes():
    # slots, lock-step batches and graph replay up to N = 1500, three-chunk sweeps and the score gradients
    base = _same_under_both_cores({"BITS_MAX_N": "1500", "BITS_WIP_GRAD": "1"})
    assert sum(k.startswith("sw_") for k in base) == 5 and sum(k.startswith("wg_") for k in base) == 5


def test_both_64_tile_cores_give_the_same_bits_at_n4096_and_n8192():
    base = _same_under_both_cores({"BITS_SIZES": "4096:8:rbf,8192:8:matern", "BITS_B8": "1"})
    assert "m8_8192" in base


def test_both_64_tile_cores_give_the_same_bits_with_64_tiles_everywhere():
    # every level of the triangular inverse and every trailing update on 64 x 64 tiles
    _same_under_both_cores({"BITS_MAX_N": "4096", "BITS_B8": "1", "BITS_WIP_GRAD": "1", "BOBE_TRTRI64": "100000",
                            "BOBE_SYRK32_BELOW": "0"})
