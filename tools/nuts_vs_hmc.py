"""NUTS (sample_GP_NUTS(sampler="nuts")) against the default HMC chains on two surrogates: wall time, microseconds per
leapfrog step of the chain kernels, mean tree depth and effective sample size per second of the slowest coordinate.
Prints a text report (profiles/nuts_vs_hmc.txt).  Usage: python tools/nuts_vs_hmc.py [--quick]"""
import os
import sys
import time

import numpy as np
from scipy.stats import qmc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ess(chains):
    """Effective sample size of (n, P) draws: Geyer's initial positive sequence on the chain-averaged autocorrelation."""
    n, P = chains.shape
    x = chains - chains.mean(0)
    var = x.var(0).mean()
    if var <= 0:
        return float("nan")
    f = np.fft.rfft(x, n=2 * n, axis=0)
    ac = np.fft.irfft(f * np.conj(f), axis=0)[:n].mean(1) / (n * var)
    s, k = 0.0, 1
    while k + 1 < n:
        pair = ac[k] + ac[k + 1]
        if pair <= 0:
            break
        s += pair
        k += 2
    return n * P / (1.0 + 2.0 * s)


def surfaces(quick):
    from bobe_amd import GP
    rng = np.random.default_rng(0)
    X = qmc.Sobol(2, scramble=True, seed=1).random(600)
    y = -0.5 * np.sum(((X - np.array([0.45, 0.55])) / 0.1) ** 2, axis=1)
    yield "2-D Gaussian surrogate, N = 600", GP(X, y, noise=1e-8, lengthscales=[0.3, 0.3], kernel_variance=20.0)
    D = 10
    n = 600 if quick else 1500
    Z = rng.normal(size=(n, D)) * 0.08 + 0.5 + 0.25 * 0.25           # around the mode x = 1 of [-2, 2]^10 (unit 0.75)
    Z = np.clip(Z, 0.0, 1.0)
    t = -2.0 + 4.0 * Z
    yr = -np.sum(100.0 * (t[:, 1:] - t[:, :-1] ** 2) ** 2 + (1.0 - t[:, :-1]) ** 2, axis=1) / 20.0
    yield f"10-D Rosenbrock surrogate, N = {n}", GP(Z, yr, noise=1e-6, lengthscales=np.full(D, 0.25), kernel_variance=float(np.var(yr)))


def main():
    from bobe_amd.samplers import sample_GP_NUTS
    quick = "--quick" in sys.argv
    lines = []
    for name, gp in surfaces(quick):
        d = gp.ndim
        for sampler in ("hmc", "nuts"):
            diag = {}
            sample_GP_NUTS(gp, np_rng=np.random.default_rng(0), num_chains=4, sampler=sampler, warmup_steps=64,
                           num_samples=64)                                  # (warm the library up)
            t0 = time.perf_counter()
            s = sample_GP_NUTS(gp, np_rng=np.random.default_rng(1), num_chains=4, sampler=sampler, diagnostics=diag)
            wall = time.perf_counter() - t0
            P = diag["state"].shape[0]
            x = s["x"]
            nk = x.shape[0] // P
            xc = x[:nk * P].reshape(nk, P, d)
            e = [ess(xc[:, :, j]) for j in range(d)]
            # time of the sampling launch alone, and its leapfrog steps
            st, ad = diag["state"].copy(), diag["adapt"].copy()
            n_it = nk * 4
            if sampler == "nuts":
                t1 = time.perf_counter()
                _, _, stats, _ = gp.nuts_run(st, ad, diag["inv_metric"], 6, diag["seed"], diag["it"], n_it, False, 1.0,
                                             stats=True)
                tl = time.perf_counter() - t1
                leaps = float(stats[:, :, 1].sum()) / P
                depth = float(stats[:, :, 0].mean())
                extra = f"mean tree depth {depth:.2f}, divergent {100 * stats[:, :, 2].mean():.2f} %, " \
                        f"mean acceptance {stats[:, :, 3].mean():.3f}"
            else:
                t1 = time.perf_counter()
                gp.hmc_run(st, ad, diag["inv_mass"], diag["seed"], diag["it"], n_it, False, 1.0)
                tl = time.perf_counter() - t1
                leaps = 8.0 * n_it                                       # (4 + 9 / 2 - 1 / 2 steps on average)
                extra = ""
            lines.append(f"{name} | {sampler:4s} | {P} chains | sample_GP_NUTS {wall:6.3f} s | sampling launch "
                         f"{1e6 * tl / leaps:6.2f} us per leapfrog step | ESS min {min(e):7.1f} "
                         f"({min(e) / wall:8.1f} /s) | {extra}")
            print(lines[-1], flush=True)
    return lines


if __name__ == "__main__":
    main()
