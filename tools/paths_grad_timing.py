"""Time of the path gradients on the benchmark's synthetic data at N = 4096, d = 8 (RBF): one bobe_gp_paths_grad call at T in
{8, 64, 512, 4096} points for F in {2048, 4096} features, beside it bobe_gp_predict_grad in mean-only mode at the same T (the
nearest existing kernel: N terms per point instead of N + F - a yardstick to read the new figure against, not a threshold),
and a whole PosteriorPaths.maximize for S in {4, 8} paths with R = 8 restarts: time, rounds and evaluations.

  python tools/paths_grad_timing.py [TABLE]        TABLE defaults to profiles/paths_grad_timing.txt

HIP events around whole calls (host pointers: the copies of a call belong to it), one warm-up call, medians of 21."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, REPS = 4096, 8, 21
F_LIST, T_LIST, S_LIST, R = (2048, 4096), (8, 64, 512, 4096), (4, 8), 8


def _timed(fn, reps=REPS):
    import torch
    fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return min(t), float(np.median(t)), max(t)


def main(table):
    import torch
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, cand, _ = synthetic_problem(N, D, max(T_LIST), 8)
    gp = GP(X, y, noise=1e-6, lengthscales=np.full(D, 0.6), kernel_variance=1.0)
    lib = gp._lib
    torch.cuda.synchronize()
    lines = [f"# path gradients at N = {N}, d = {D} (bench's synthetic data, RBF, ls 0.6, noise 1e-6); ms, min / median / max of",
             f"# {REPS} calls after a warm-up, HIP events around whole calls, host pointers.  S = 8 paths, the points' paths cycle.",
             "# predict_grad: bobe_gp_predict_grad, mean only, the same points (N terms per point; paths_grad has N + F)", "",
             f"{'F':>5s} {'T':>5s} | {'paths_grad':>23s} | {'predict_grad (mean)':>23s} | {'ratio':>5s} | {'us/point':>8s}"]
    for f in F_LIST:
        with gp.sample_paths(8, f, seed=1) as ps:
            for t in T_LIST:
                q = np.ascontiguousarray(cand[:t])
                idx = (np.arange(t) % 8).astype(np.int64)
                fo, go, mo = np.empty(t), np.empty((t, D)), np.empty(t)

                def pg():
                    assert lib.bobe_gp_paths_grad(ps._h, q.ctypes.data, t, idx.ctypes.data, 0, fo.ctypes.data, go.ctypes.data) == 0

                def mg():
                    assert lib.bobe_gp_predict_grad(gp._h, q.ctypes.data, t, mo.ctypes.data, None, go.ctypes.data, None) == 0
                a, b = _timed(pg), _timed(mg)
                lines.append(f"{f:5d} {t:5d} | {a[0]:7.3f} {a[1]:7.3f} {a[2]:7.3f} | {b[0]:7.3f} {b[1]:7.3f} {b[2]:7.3f} | "
                             f"{a[1] / b[1]:5.2f} | {1e3 * a[1] / t:8.2f}")
                print(lines[-1], flush=True)
    lines += ["", f"# PosteriorPaths.maximize, R = {R} starts per path (the best rows of a 1024-row pool), maxiter 100, the cube's bounds;",
              "# ms of the whole call (min / median / max of 5 after a warm-up), rounds = device calls, evaluations = points in them",
              f"{'F':>5s} {'S':>3s} | {'maximize':>26s} | {'rounds':>6s} {'evals':>6s} | {'ms/round':>8s} | gain of the paths' maxima over the pool's"]
    pool = np.ascontiguousarray(cand[:1024])
    for f in F_LIST:
        for s in S_LIST:
            with gp.sample_paths(s, f, seed=2) as ps:
                order = np.argsort(-ps.evaluate(pool), axis=1, kind="stable")[:, :R]
                starts = pool[order]
                res = {}

                def mx():
                    res["r"] = ps.maximize(starts)
                tm = _timed(mx, 5)
                r = res["r"]
                gain = r["value"] - r["start_value"]
                lines.append(f"{f:5d} {s:3d} | {tm[0]:8.1f} {tm[1]:8.1f} {tm[2]:8.1f} | {r['n_rounds']:6d} {r['n_evaluations']:6d} | "
                             f"{tm[1] / r['n_rounds']:8.3f} | min {gain.min():.3g} median {np.median(gain):.3g} max {gain.max():.3g}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(table)), exist_ok=True)
    open(table, "w").write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paths_grad_timing.txt"))
