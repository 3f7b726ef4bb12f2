"""Time of the constrained random walks (bobe_gp_rwalk) per step, on the benchmark's synthetic data (RBF) at N = 1500,
d = 10 with P = 256 walkers and 30 walks per call - timed as tools/paths_hmc_timing.py times the chains: HIP events around
whole calls (host pointers: the copies of a call belong to it), one warm-up call, median of 7.

  python tools/rwalk_timing.py          prints one line"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, D, P, WALKS = 1500, 10, 256, 30


def main():
    import torch  # noqa: F401  (before the library, as in paths_hmc_timing.py: the timing events are torch's)
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    from paths_hmc_timing import _timed
    X, y, cand, _ = synthetic_problem(N, D, P, 8)
    gp = GP(X, y, noise=1e-6, lengthscales=np.full(D, 0.6), kernel_variance=1.0)
    x0 = np.clip(np.ascontiguousarray(cand[:P]), 0.05, 0.95)
    logl = gp.predict_mean_batched(x0)
    step = 0.02 * np.eye(D)
    res = gp.rwalk(x0, logl, step, -1e30, WALKS, 5)
    ms = _timed(lambda: gp.rwalk(x0, logl, step, -1e30, WALKS, 5))
    print(f"rwalk N = {N}, d = {D}, P = {P}, {WALKS} walks: {1e3 * ms / WALKS:7.2f} us per step "
          f"({int(res[3].sum())} of {P * WALKS} proposals inside the cube)")


if __name__ == "__main__":
    main()
