"""Time of whole HMC chains on posterior paths (bobe_gp_paths_hmc_run) per leapfrog step, on the benchmark's synthetic data
(RBF) at (N, d) = (600, 2), (1500, 10), (4096, 8), for F in {1024, 4096} features and P in {64, 256, 2048} chains, beside
  - bobe_gp_hmc_run at the same N, d and P (the mean target: N terms per step instead of N + F), and
  - the host-stepped loop, the only way to run such a chain without the kernel: ONE bobe_gp_paths_grad call per leapfrog
    step for the P points of the batch (its device time alone: the host arithmetic between the calls is not counted).

  python tools/paths_hmc_timing.py [TABLE]        TABLE defaults to profiles/paths_hmc_timing.txt

HIP events around whole calls (host pointers: the copies of a call belong to it), one warm-up call, medians of 7.  A launch is
NITER iterations of 4 - 12 leapfrog steps (8 on average, drawn per chain and iteration): us per step = time / (NITER * 8)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, F_LIST, P_LIST, S, NITER, REPS = ((600, 2), (1500, 10), (4096, 8)), (1024, 4096), (64, 256, 2048), 8, 16, 7


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
    return float(np.median(t))


def main(table):
    import torch
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    lines = [f"# whole HMC chains on posterior paths, us per leapfrog step of the whole batch (median of {REPS} launches of {NITER}",
             "# iterations after a warm-up, HIP events around whole calls, host pointers; 8 steps per iteration on average).",
             f"# bench's synthetic data, RBF, ls 0.6, noise 1e-6, S = {S} paths, the chains' paths cycle, eps 0.02, no adaptation.",
             "# paths_hmc: bobe_gp_paths_hmc_run.  hmc: bobe_gp_hmc_run, the mean target (N terms per step, not N + F).",
             "# host-stepped: one bobe_gp_paths_grad call on the P points per leapfrog step (device time of the call alone).",
             "# rows: where a chain's workgroup keeps the set's training rows (registers / LDS / streamed), features per thread", "",
             f"{'N':>5s} {'d':>3s} {'F':>5s} {'P':>5s} | {'paths_hmc':>9s} | {'hmc':>8s} | {'host-stepped':>12s} | "
             f"{'vs hmc':>6s} | {'vs host':>7s} | rows"]
    for n, d in SIZES:
        X, y, cand, _ = synthetic_problem(n, d, max(P_LIST), 8)
        gp = GP(X, y, noise=1e-6, lengthscales=np.full(d, 0.6), kernel_variance=1.0)
        lib = gp._lib
        torch.cuda.synchronize()
        for f in F_LIST:
            with gp.sample_paths(S, f, seed=1) as ps:
                lay = ps.chain_layout()
                for p in P_LIST:
                    x0 = np.clip(np.ascontiguousarray(cand[:p]), 0.05, 0.95)
                    idx = (np.arange(p) % S).astype(np.int64)
                    U = np.log(x0) - np.log1p(-x0)
                    st_p = ps.hmc_state(U, idx, 1.0)
                    m, _, dm, _ = gp.predict_grad(x0, mean_only=True)
                    mean = m * gp.y_std + gp.y_mean
                    st_m = np.ascontiguousarray(np.concatenate(
                        [U, dm * gp.y_std * (x0 * (1 - x0)) + (1 - 2 * x0), x0,
                         (mean + np.sum(np.log(x0) + np.log1p(-x0), axis=1))[:, None], mean[:, None]], axis=1))
                    adapt = np.tile(np.array([0.02, 0.0, 0.0, 0.0, 0.0]), (p, 1))
                    im = np.ones((p, d))
                    fo, go = np.empty(p), np.empty((p, d))

                    def run_paths():
                        ps.hmc_run(st_p.copy(), adapt.copy(), im, idx, 3, 0, NITER, False)

                    def run_mean():
                        gp.hmc_run(st_m.copy(), adapt.copy(), im[0], 3, 0, NITER, False)

                    def one_grad():
                        assert lib.bobe_gp_paths_grad(ps._h, x0.ctypes.data, p, idx.ctypes.data, 0, fo.ctypes.data,
                                                      go.ctypes.data) == 0
                    a, b, c = _timed(run_paths), _timed(run_mean), _timed(one_grad)
                    steps = NITER * 8.0
                    ua, ub, uc = 1e3 * a / steps, 1e3 * b / steps, 1e3 * c
                    lines.append(f"{n:5d} {d:3d} {f:5d} {p:5d} | {ua:9.1f} | {ub:8.1f} | {uc:12.1f} | {ua / ub:6.2f} | {uc / ua:7.2f} | "
                                 f"{lay['registers']}/{lay['lds']}/{lay['streamed']}, {lay['features_per_thread']}")
                    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(table)), exist_ok=True)
    open(table, "w").write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paths_hmc_timing.txt"))
