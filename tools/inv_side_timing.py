"""Wall time of one evaluation round (value + gradient) per size and batch width: the A/B behind inv_side_pays (gp_factor.hip).
The library reads BOBE_INV_SIDE once per process, so one run measures one setting:
   BOBE_INV_SIDE=0 python tools/inv_side_timing.py --sizes 2048,4096 --batches 1,4,8
   BOBE_INV_SIDE=2 python tools/inv_side_timing.py --sizes 2048,4096 --batches 1,4,8
prints one JSON line {"<N>x<B>": [median ms, min ms], ...}.  B = 1 is the single evaluation on the handle's stream, B > 1
the lock-step batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bobe_amd.gp import GP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2048,3072,4096,6144,8192")
ap.add_argument("--batches", default="1,4,8")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--d", type=int, default=8)
args = ap.parse_args()

out = {}
for N in (int(s) for s in args.sizes.split(",")):
    rng = np.random.default_rng(N)
    X = rng.uniform(size=(N, args.d))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=N)
    gp = GP(X, y, noise=1e-5, kernel="rbf", lengthscales=np.full(args.d, 0.5))
    for B in (int(b) for b in args.batches.split(",")):
        ls = np.full((B, args.d), 0.4) + 0.03 * np.arange(B)[:, None]
        kv = np.ones(B)
        run = (lambda: gp.mll_data(ls[0], 1.0)) if B == 1 else (lambda: gp.mll_data_batch(ls, kv))
        for _ in range(3):
            run()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[f"{N}x{B}"] = [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4)]
    del gp
print(json.dumps(out))
