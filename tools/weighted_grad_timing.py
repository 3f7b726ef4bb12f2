"""Cost of the weighted score gradients (bobe_gp_wip_grad_w) beside bobe_gp_wip_grad, and of the polish built on them, on the
benchmark's synthetic data (RBF, ls 0.6, noise 1e-6, d = 8).  Every library figure is the median of REPS calls after a warm-up
call, in milliseconds between two HIP events recorded on the handle's stream around the whole call (it ends in a stream
synchronise); host pointers throughout.

  one call at C in {1, 8, 16}, N in {400, 1024, 4096}, M in {128, 512} of (a) bobe_gp_wip_grad, (b) bobe_gp_wip_grad_w with one
  criterion (imiqr), (c) with all four - each with the z-side caches hit (the same Z again) and missed (two Z sets in turn:
  every call is the first after forget_z);
  bobe_gp_wip_grad alone, RUNS times in a fresh process each, alternating between this tree's library and - when PARENT_LIB is
  given - a libbobe_gp.so built from the parent commit: the run-to-run spread, and the existing call before / after;
  one IMIQR.get_next_point with acq_kwargs['weighted_polish'] = 8 beside the unpolished one (N = 400, M = 128; wall clock,
  the call includes the pool sweep) and how far the score moves, on three seeds.

  python tools/weighted_grad_timing.py table [OUT [PARENT_LIB]]     OUT defaults to profiles/weighted_grad_timing.txt
  python tools/weighted_grad_timing.py single N M C REPS [LIB]      what a child process runs: prints two medians (ms)
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS, MS, CS, D = (400, 1024, 4096), (128, 512), (1, 8, 16), 8
PARENT_SIZES = [(400, 128, 1), (1024, 128, 1), (4096, 512, 1), (4096, 512, 16)]
REPS = 21
RUNS = 5


def _setup(n, d=D):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, _, _ = synthetic_problem(n, d, 1, 1)
    return GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(d, 0.6), kernel_variance=1.0)


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

    def median(self, fn, reps):
        fn()                                                 # warm-up: code objects, first allocations
        fn()
        return float(np.median([self.time(fn) for _ in range(reps)]))


def _calls(gp, m, c, seed=0):
    """name -> closure(miss): the three calls on host arrays; miss alternates between two sets of integration points"""
    from bobe_amd import _lib
    lib, h, d = gp._lib, gp._h, gp.ndim
    rng = np.random.default_rng(seed)
    cand, lw = rng.uniform(0.1, 0.9, size=(c, d)), 1.5 * rng.normal(size=m)
    Zs = [rng.uniform(size=(m, d)), rng.uniform(size=(m, d))]
    turn = [0]
    vals, grads = [np.empty(c) for _ in range(4)], [np.empty((c, d)) for _ in range(4)]
    ystd = float(gp.y_std)

    def z(miss):
        turn[0] ^= 1 if miss else 0
        return Zs[turn[0]]

    def old(miss=False):
        st = lib.bobe_gp_wip_grad(h, _lib.ptr(cand), c, _lib.ptr(z(miss)), m, ystd, _lib.ptr(vals[0]), _lib.ptr(vals[1]),
                                  _lib.ptr(grads[0]), _lib.ptr(grads[1]))
        assert st == 0 and np.all(np.isfinite(grads[0]))

    def new(keys):
        ps = (C.c_void_p * 4)(*[vals[k].ctypes.data if k in keys else None for k in range(4)])
        pg = (C.c_void_p * 4)(*[grads[k].ctypes.data if k in keys else None for k in range(4)])

        def call(miss=False):
            st = lib.bobe_gp_wip_grad_w(h, _lib.ptr(cand), c, _lib.ptr(z(miss)), m, ystd, _lib.ptr(lw), ps, pg)
            assert st == 0 and all(np.all(np.isfinite(grads[k])) for k in keys)
        return call
    out = {"wip_grad": old}
    if hasattr(lib, "bobe_gp_wip_grad_w"):
        out["one"], out["four"] = new((2,)), new((0, 1, 2, 3))
    return out


def _single_in_child(n, m, c, lib_path):
    cmd = [sys.executable, os.path.abspath(__file__), "single", str(n), str(m), str(c), str(REPS)] + ([lib_path] if lib_path else [])
    out = subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.PIPE, text=True).stdout.split()
    return float(out[-2]), float(out[-1])


def _polish_rows():
    from bobe_amd.acquisition import IMIQR
    gp = _setup(400)
    rows = []
    for seed in (0, 1, 2):
        rng = np.random.default_rng(40 + seed)
        kw = {"mc_samples": {"x": rng.uniform(size=(1024, D))}, "mc_points_size": 128}
        t = {}
        for r in (0, 8):
            IMIQR().get_next_point(gp, acq_kwargs=dict(kw, weighted_polish=r), rng=np.random.default_rng(seed), verbose=False)
            t0 = time.perf_counter()
            x, v = IMIQR().get_next_point(gp, acq_kwargs=dict(kw, weighted_polish=r), rng=np.random.default_rng(seed),
                                          verbose=False)
            t[r] = (1e3 * (time.perf_counter() - t0), float(v), np.array(x))
        rows.append(f"{seed:>4} | {t[0][0]:>12.3f} | {t[8][0]:>11.3f} | {t[0][1]:>14.8f} | {t[8][1]:>14.8f} | "
                    f"{t[0][1] - t[8][1]:>10.3e} | {float(np.max(np.abs(t[8][2] - t[0][2]))):>9.3e}")
    return rows


def table(out, parent_lib=None):
    lines = ["# weighted score gradients (tools/weighted_grad_timing.py): bench's synthetic data, RBF, noise 1e-6, d = 8; median ms of "
             f"{REPS} whole calls after two warm-up calls, HIP events on the handle's stream, host pointers",
             "# a = bobe_gp_wip_grad, b = bobe_gp_wip_grad_w with one criterion (imiqr), c = with all four; hit = the same Z again "
             "(z-side caches and the per-z table kept), miss = another Z every call (the first call after forget_z)", "",
             f"{'N':>5} {'M':>4} {'C':>3} | {'a hit':>8} {'b hit':>8} {'c hit':>8} | {'b - a':>8} {'c - a':>8} | "
             f"{'a miss':>8} {'b miss':>8} {'c miss':>8}"]
    for n in NS:
        gp = _setup(n)
        ev = Events(gp)
        for m in MS:
            for c in CS:
                calls = _calls(gp, m, c)
                hit = {k: ev.median(f, REPS) for k, f in calls.items()}
                miss = {k: ev.median(lambda f=f: f(True), REPS) for k, f in calls.items()}
                lines.append(f"{n:>5} {m:>4} {c:>3} | {hit['wip_grad']:>8.4f} {hit['one']:>8.4f} {hit['four']:>8.4f} | "
                             f"{hit['one'] - hit['wip_grad']:>8.4f} {hit['four'] - hit['wip_grad']:>8.4f} | "
                             f"{miss['wip_grad']:>8.4f} {miss['one']:>8.4f} {miss['four']:>8.4f}")
        del gp
    lines += ["", f"# bobe_gp_wip_grad (hit, miss), {RUNS} runs in a fresh process each (median of {REPS} calls per run)"
              + (", alternating with a library built from the parent commit" if parent_lib else ""),
              "# spread = largest minus smallest of the runs' medians", ""]
    for n, m, c in PARENT_SIZES:
        runs = {"this tree": [], "parent": []}
        for _ in range(RUNS):
            if parent_lib:
                runs["parent"].append(_single_in_child(n, m, c, parent_lib))
            runs["this tree"].append(_single_in_child(n, m, c, None))
        for k, mode in enumerate(("hit", "miss")):
            for who, r in runs.items():
                if not r:
                    continue
                med = [v[k] for v in r]
                lines.append(f"{n:>5} {m:>4} {c:>3} {mode:>5} {who:>10} | medians " + " ".join(f"{x:.4f}" for x in med) +
                             f" | median of medians {float(np.median(med)):.4f} | spread {max(med) - min(med):.4f}")
    lines += ["", "# IMIQR.get_next_point, N = 400, M = 128, a pool of 1024 uniform samples: acq_kwargs['weighted_polish'] = 0 / 8 "
              "(wall clock of the whole call, the second of two), the scores and how far the pick moves (max-norm)", "",
              f"{'seed':>4} | {'unpolished ms':>12} | {'polished ms':>11} | {'pool score':>14} | {'polished score':>14} | "
              f"{'gain':>10} | {'moved':>9}"] + _polish_rows()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    if sys.argv[1] == "single":
        n, m, c, reps = (int(v) for v in sys.argv[2:6])
        if len(sys.argv) > 6:                            # another build of the library (it may lack the newer entry points)
            from bobe_amd import _lib
            _lib.LIB_PATH = os.path.abspath(sys.argv[6])
            have = C.CDLL(_lib.LIB_PATH)
            _lib.SIGNATURES = [s for s in _lib.SIGNATURES if hasattr(have, s[0])]
        gp = _setup(n)
        ev, old = Events(gp), _calls(gp, m, c)["wip_grad"]
        print("%.4f %.4f" % (ev.median(old, reps), ev.median(lambda: old(True), reps)))
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_grad_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
