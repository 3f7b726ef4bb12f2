"""Time of the LOO objective in lock step (bobe_gp_loo_objective_batch) on the benchmark's synthetic data (RBF, ls 0.6, noise
1e-6) at N = 1024 (d = 6) and N = 4096 (d = 8), value and gradient, in tools/loo_timing.py's scheme: each number is the median
host time of REPS calls after a warm-up call; every entry point synchronises before it returns.

  B single bobe_gp_loo_objective calls against one bobe_gp_loo_objective_batch of B, B = 4 and 8 (distinct theta per member);
  one GP.fit with fit_objective='loo' from four starts (MAXITER iterations at most), lock step against
  concurrent_restarts = False;
  the single call alone, RUNS times in a fresh process each, alternating between this tree's library and - when PARENT_LIB
  is given - a libbobe_gp.so built from the parent commit: the run-to-run spread, and the single call before / after.

  python tools/loo_batch_timing.py table [OUT [PARENT_LIB]]      OUT defaults to profiles/loo_batch_timing.txt
  python tools/loo_batch_timing.py single N D REPS [LIB]         what a child process runs: prints median min max (ms)
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 6), (4096, 8)]
REPS = 9
RUNS = 5
FIT_REPS = 3
MAXITER = 10


def _setup(n, d, **kw):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, _, _ = synthetic_problem(n, d, 1, 1)
    return GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(d, 0.6), kernel_variance=1.0, **kw)


def _median(call, reps):
    call()                                               # warm-up: code objects, first allocations
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3


def _members(d, B):
    return (np.ascontiguousarray(np.full((B, d), 0.55) + 0.01 * np.arange(B)[:, None]), 1.1 + 0.05 * np.arange(B, dtype=float))


def _time_single(gp, d, reps, B=1):
    lib, h = gp._lib, gp._h
    ls, kv = _members(d, B)
    val, grad = C.c_double(0.0), np.empty(d + 1)

    def call():
        for b in range(B):
            st = lib.bobe_gp_loo_objective(h, ls[b].ctypes.data, float(kv[b]), C.byref(val), grad.ctypes.data)
            assert st == 0 and np.isfinite(val.value), st
    return _median(call, reps)


def _time_batch(gp, d, reps, B):
    lib, h = gp._lib, gp._h
    ls, kv = _members(d, B)
    val, grad = np.empty(B), np.empty((B, d + 1))

    def call():
        st = lib.bobe_gp_loo_objective_batch(h, B, ls.ctypes.data, kv.ctypes.data, val.ctypes.data, grad.ctypes.data, None)
        assert st == 0 and np.all(np.isfinite(val)), st
    return _median(call, reps)


def _time_fit(n, d, lockstep):
    gp = _setup(n, d, fit_objective="loo", lengthscale_bounds=[0.05, 2.0], kernel_variance_bounds=[1e-2, 1e2],
                optimizer_options={"method": "L-BFGS-B"})
    gp.concurrent_restarts = lockstep
    th0 = np.log(np.append(np.full(d, 0.6), 1.0))
    x0 = np.vstack([th0, th0 + np.random.default_rng(21).uniform(-0.3, 0.3, size=(3, d + 1))])
    res = []
    t = _median(lambda: res.append(gp.fit(x0=x0, maxiter=MAXITER)), FIT_REPS)
    return t, res[-1]


def _single_in_child(n, d, lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "single", str(n), str(d), str(REPS)] + ([lib_path] if lib_path else [])
    out = subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.PIPE, text=True).stdout.split()
    return tuple(float(v) for v in out[-3:])


def _cell(v):
    return f"{v[0]:8.3f} [{v[1]:.3f}, {v[2]:.3f}]"


def table(out, parent_lib=None):
    lines = ["# LOO objective in lock step (tools/loo_batch_timing.py): bench's synthetic data, RBF, noise 1e-6, value + gradient; "
             f"median [min, max] host ms of {REPS} calls after a warm-up, every call ends in a stream synchronise",
             "# singles = B bobe_gp_loo_objective calls one after another; batch = one bobe_gp_loo_objective_batch of B", "",
             f"{'N':>6} {'d':>3} {'B':>2} | {'singles ms':>26} | {'batch ms':>26} | {'batch / singles':>15}"]
    for n, d in SIZES:
        gp = _setup(n, d)
        for B in (4, 8):
            s, b = _time_single(gp, d, REPS, B), _time_batch(gp, d, REPS, B)
            lines.append(f"{n:>6} {d:>3} {B:>2} | {_cell(s):>26} | {_cell(b):>26} | {b[0] / s[0]:>15.2f}")
        del gp
    lines += ["", f"# GP.fit(fit_objective='loo'), four starts, maxiter {MAXITER}: median [min, max] host ms of {FIT_REPS} fits "
              "after a warm-up fit; the two fits return the same bits", "",
              f"{'N':>6} {'d':>3} | {'lock step ms':>30} | {'one after another ms':>30} | {'ratio':>6}"]
    for n, d in SIZES:
        (a, ra), (b, rb) = _time_fit(n, d, True), _time_fit(n, d, False)
        assert ra["mll"] == rb["mll"] and np.array_equal(ra["params"], rb["params"])
        lines.append(f"{n:>6} {d:>3} | {_cell(a):>30} | {_cell(b):>30} | {a[0] / b[0]:>6.2f}")
    lines += ["", f"# the single call, {RUNS} runs in a fresh process each (median [min, max] of {REPS} calls per run)"
              + (", alternating with a library built from the parent commit" if parent_lib else ""),
              "# spread = largest minus smallest of the runs' medians", ""]
    for n, d in SIZES:
        runs = {"this tree": [], "parent": []}
        for _ in range(RUNS):
            if parent_lib:
                runs["parent"].append(_single_in_child(n, d, parent_lib))
            runs["this tree"].append(_single_in_child(n, d, None))
        for who, r in runs.items():
            if not r:
                continue
            med = [v[0] for v in r]
            lines.append(f"{n:>6} {d:>3} {who:>10} | medians " + " ".join(f"{m:.3f}" for m in med) +
                         f" | median of medians {float(np.median(med)):.3f} | spread {max(med) - min(med):.3f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    if sys.argv[1] == "single":
        n, d, reps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
        if len(sys.argv) > 5:                            # another build of the library (it may lack the newer entry points)
            from bobe_amd import _lib
            _lib.LIB_PATH = os.path.abspath(sys.argv[5])
            have = C.CDLL(_lib.LIB_PATH)
            _lib.SIGNATURES = [s for s in _lib.SIGNATURES if hasattr(have, s[0])]
        print("%.4f %.4f %.4f" % _time_single(_setup(n, d), d, reps))
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "loo_batch_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
