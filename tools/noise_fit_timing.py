"""Cost of the noise component of the two gradients (bobe_gp_mll_noise, bobe_gp_loo_objective_noise) on the benchmark's
synthetic data (RBF, ls 0.6, noise 1e-6, d = 8) at N = 1024 and 4096, value and gradient.  Every number is the median of REPS
calls after a warm-up call, in milliseconds between two HIP events recorded on the handle's stream around the call (the call
ends in a stream synchronise).

  the value-and-gradient with the noise component beside bobe_gp_mll's, and the LOO pair likewise (one process);
  bobe_gp_mll / bobe_gp_loo_objective alone, RUNS times in a fresh process each, alternating between this tree's library and
  - when PARENT_LIB is given - a libbobe_gp.so built from the parent commit: the run-to-run spread, and the existing calls
  before / after.

  python tools/noise_fit_timing.py table [OUT [PARENT_LIB]]      OUT defaults to profiles/noise_fit_timing.txt
  python tools/noise_fit_timing.py single N D REPS [LIB]         what a child process runs: prints the two medians (ms)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 8), (4096, 8)]
REPS = 21
RUNS = 5
LS, KVAR, NOISE = 0.55, 1.1, 1e-6


def _setup(n, d):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, _, _ = synthetic_problem(n, d, 1, 1)
    return GP(X, y, noise=NOISE, kernel="rbf", lengthscales=np.full(d, 0.6), kernel_variance=1.0)


class Events:
    """Elapsed milliseconds between two HIP events recorded on the handle's stream."""

    def __init__(self, gp):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.stream = C.c_void_p(gp._lib.bobe_gp_get_stream(gp._h))
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0.0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)

    def stats(self, fn, reps):
        fn()                                                 # warm-up: code objects, first allocations
        t = [self.time(fn) for _ in range(reps)]
        return float(np.median(t)), float(np.min(t)), float(np.max(t))


def _calls(gp, d):
    """The four calls at one theta: name -> closure (the noise forms only where the library has them)."""
    lib, h = gp._lib, gp._h
    ls = np.full(d, LS)
    val, g1, g2 = C.c_double(0.0), np.empty(d + 1), np.empty(d + 2)

    def plain(name):
        def call():
            st = getattr(lib, name)(h, ls.ctypes.data, KVAR, C.byref(val), g1.ctypes.data)
            assert st == 0 and np.isfinite(val.value), (name, st)
        return call

    def noisy(name):
        def call():
            st = getattr(lib, name)(h, ls.ctypes.data, KVAR, NOISE, C.byref(val), g2.ctypes.data)
            assert st == 0 and np.isfinite(val.value) and np.isfinite(g2[-1]), (name, st)
        return call
    out = {"mll": plain("bobe_gp_mll"), "loo": plain("bobe_gp_loo_objective")}
    if hasattr(lib, "bobe_gp_mll_noise"):
        out["mll_noise"], out["loo_noise"] = noisy("bobe_gp_mll_noise"), noisy("bobe_gp_loo_objective_noise")
    return out


def _single_in_child(n, d, lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "single", str(n), str(d), str(REPS)] + ([lib_path] if lib_path else [])
    out = subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.PIPE, text=True).stdout.split()
    return float(out[-2]), float(out[-1])


def _cell(v):
    return f"{v[0]:8.4f} [{v[1]:.4f}, {v[2]:.4f}]"


def table(out, parent_lib=None):
    lines = ["# the noise component of the gradients (tools/noise_fit_timing.py): bench's synthetic data, RBF, noise 1e-6, d = 8, "
             f"value + gradient; median [min, max] ms of {REPS} calls after a warm-up, HIP events on the handle's stream",
             "# plain = bobe_gp_mll / bobe_gp_loo_objective (d + 1 entries); noise = bobe_gp_mll_noise / "
             "bobe_gp_loo_objective_noise (d + 2 entries)", "",
             f"{'N':>6} {'objective':>9} | {'plain ms':>30} | {'noise ms':>30} | {'added ms':>9} | {'noise / plain':>13}"]
    for n, d in SIZES:
        gp = _setup(n, d)
        ev, calls = Events(gp), _calls(gp, d)
        for obj in ("mll", "loo"):
            p, q = ev.stats(calls[obj], REPS), ev.stats(calls[obj + "_noise"], REPS)
            lines.append(f"{n:>6} {obj:>9} | {_cell(p):>30} | {_cell(q):>30} | {q[0] - p[0]:>9.4f} | {q[0] / p[0]:>13.4f}")
        del gp
    lines += ["", f"# the existing calls, {RUNS} runs in a fresh process each (median of {REPS} calls per run)"
              + (", alternating with a library built from the parent commit" if parent_lib else ""),
              "# spread = largest minus smallest of the runs' medians", ""]
    for n, d in SIZES:
        runs = {"this tree": [], "parent": []}
        for _ in range(RUNS):
            if parent_lib:
                runs["parent"].append(_single_in_child(n, d, parent_lib))
            runs["this tree"].append(_single_in_child(n, d, None))
        for k, obj in enumerate(("bobe_gp_mll", "bobe_gp_loo_objective")):
            for who, r in runs.items():
                if not r:
                    continue
                med = [v[k] for v in r]
                lines.append(f"{n:>6} {obj:>22} {who:>10} | medians " + " ".join(f"{m:.4f}" for m in med) +
                             f" | median of medians {float(np.median(med)):.4f} | spread {max(med) - min(med):.4f}")
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
        gp = _setup(n, d)
        ev, calls = Events(gp), _calls(gp, d)
        print("%.4f %.4f" % (ev.stats(calls["mll"], reps)[0], ev.stats(calls["loo"], reps)[0]))
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "noise_fit_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
