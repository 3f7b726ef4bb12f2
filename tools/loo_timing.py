"""Time of the leave-one-out entry points on the benchmark's synthetic data (RBF, ls 0.6, noise 1e-6) at N = 1024 (d = 6) and
N = 4096 (d = 8): bobe_gp_loo on the factorised state (sum only: no output copy), and one bobe_gp_loo_objective
value-and-gradient beside one bobe_gp_mll value-and-gradient.  Each number is the median host time of REPS calls after a
warm-up call; every entry point synchronises before it returns.  With a second argument the kernels of the N = 4096
evaluations are listed from a rocprofv3 --kernel-trace --stats run of their own (one profiled process per entry point).

  python tools/loo_timing.py table [OUT]        OUT defaults to profiles/loo_timing.txt
  python tools/loo_timing.py table OUT TRACEDIR also the kernel lists (rocprofv3 output goes under TRACEDIR)
  python tools/loo_timing.py run loo|objective|mll N D REPS   what a profiled process runs

Counted work: the objective is one MLL evaluation (N^3 / 3 potrf + N^3 / 3 inverse + N^3 / 3 K^-1) plus the dense B^T B,
N^3 flop on the lower tiles (6.9e10 at N = 4096), a symmetric matrix-vector product and O(N) passes; bobe_gp_loo reads the
lower triangle of the inverse factor once, 4 N^2 bytes."""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 6), (4096, 8)]
REPS = 9


def _setup(n, d):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, _, _ = synthetic_problem(n, d, 1, 1)
    return GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(d, 0.6), kernel_variance=1.0)


def _time(gp, what, d, reps):
    lib, h = gp._lib, gp._h
    ls = np.full(d, 0.55)
    val, grad = C.c_double(0.0), np.empty(d + 1)

    def call():
        if what == "loo":
            st = lib.bobe_gp_loo(h, None, None, None, C.byref(val))
        elif what == "objective":
            st = lib.bobe_gp_loo_objective(h, ls.ctypes.data, 1.1, C.byref(val), grad.ctypes.data)
        else:
            st = lib.bobe_gp_mll(h, ls.ctypes.data, 1.1, C.byref(val), grad.ctypes.data)
        assert st == 0 and np.isfinite(val.value), (what, st)
    call()                                               # warm-up: code objects, first allocations
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3


def _kernel_stats(tracedir, what, n, d):
    out = os.path.join(tracedir, f"{what}_n{n}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                    os.path.abspath(__file__), "run", what, str(n), str(d), "3"], check=True, timeout=600,
                   stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel stats under {out}"
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].split("(")[0].replace("void ", "").replace("bobe::", "").strip()
        rows.append((float(r["TotalDurationNs"]) / 1e6, int(r["Calls"]), name))
    return sorted(rows, reverse=True)


def table(out, tracedir=None):
    lines = ["# leave-one-out timing (tools/loo_timing.py): bench's synthetic data, RBF, noise 1e-6; median [min, max] host ms of "
             f"{REPS} calls after a warm-up, every call ends in a stream synchronise",
             "# loo = bobe_gp_loo on the factorised state (sum only); objective = bobe_gp_loo_objective value + gradient; "
             "mll = bobe_gp_mll value + gradient", "",
             f"{'N':>6} {'d':>3} | {'loo ms':>24} | {'objective ms':>24} | {'mll ms':>24} | {'objective / mll':>15}"]
    for n, d in SIZES:
        gp = _setup(n, d)
        t = {w: _time(gp, w, d, REPS) for w in ("loo", "objective", "mll")}
        cell = {w: f"{v[0]:8.3f} [{v[1]:.3f}, {v[2]:.3f}]" for w, v in t.items()}
        lines.append(f"{n:>6} {d:>3} | {cell['loo']:>24} | {cell['objective']:>24} | {cell['mll']:>24} | "
                     f"{t['objective'][0] / t['mll'][0]:>15.2f}")
        del gp
    if tracedir:
        n, d = SIZES[-1]
        for what in ("objective", "mll", "loo"):
            lines += ["", f"# kernels of `{what}` at N = {n} (rocprofv3 --kernel-trace --stats; the GP's set-up and 4 calls - warm-up "
                      "+ 3 - in the process): total ms, calls, kernel"]
            for ms, calls, name in _kernel_stats(tracedir, what, n, d)[:14]:
                lines.append(f"{ms:10.3f} {calls:6d}  {name[:150]}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        what, n, d, reps = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
        _time(_setup(n, d), what, d, reps)
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "loo_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
