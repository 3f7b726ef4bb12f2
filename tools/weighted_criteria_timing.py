"""Cost of the importance-weighted scoring pass (bobe_gp_wip_sweep_w, bobe_gp_wip_select_batch_w) at bench's synthetic data:
N = 4096, d = 8, M = 512, RBF, ls 0.6, noise 1e-6; candidate pools C = 8192 and 65 536.  HIP events on the handle's stream
around whole calls (each ends in a stream synchronise); every figure is the median [min, max] of 21 calls after a warm-up.

  (a) wip_sweep                                   the equal-weight sweep, as it was
  (b) wip_sweep(log_weights=, criteria=...)       per criterion set, with log-weights
  (c) a later stage of wip_select_batch_w         (call with n_batch = 5 - call with n_batch = 1) / 4, imiqr and eiv; wipstd of
                                                  wip_select_batch beside it
  (d) the scoring launches alone                  bobe_gp_profile_select(cross) around the same calls: k_wip_score for (a),
                                                  k_wip_score_w for (b), with the Mp x C x 8 bytes of crossT they read and the
                                                  candidate-point pairs per second
  (e) wip_sweep on this build and on a library built from the parent commit (PARENT_LIB), alternating fresh processes

  python tools/weighted_criteria_timing.py table [OUT [PARENT_LIB]]     OUT defaults to profiles/weighted_criteria_timing.txt
  python tools/weighted_criteria_timing.py rows C                       the rows of one pool (what `table` starts)
  python tools/weighted_criteria_timing.py sweep C [LIB]                median wip_sweep ms of one fresh process (for (e))

Every GPU step is a process of its own under `timeout -k 10`; `table` stops at the first that fails.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, M = 4096, 8, 512
POOLS = (8192, 65536)
REPS = 21
SETS = (("wipv", "wipstd"), ("imiqr",), ("eiv",), ("wipv", "wipstd", "imiqr", "eiv"))
AB_ROUNDS = 3


def _setup(c):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, cand, Z = synthetic_problem(N, D, c, M, noise=1e-6)
    gp = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(D, 0.6), kernel_variance=1.0)
    lw = 1.5 * np.random.default_rng(1).normal(size=M)
    return gp, np.ascontiguousarray(cand), np.ascontiguousarray(Z), lw


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

    def stats(self, fn, reps=REPS):
        fn()                                                 # warm-up
        t = [self.time(fn) for _ in range(reps)]
        return float(np.median(t)), float(np.min(t)), float(np.max(t))


def _cell(v):
    return f"{v[0]:8.3f} [{v[1]:.3f}, {v[2]:.3f}]"


def _scoring_ms(gp, fn, reps=REPS):
    """Mean milliseconds per call of the launches inside the sweep's scoring bracket (profile class `cross`)."""
    from bobe_amd import _lib
    fn()
    gp._lib.bobe_gp_profile_select(gp._h, _lib.PROF["cross"])
    for _ in range(reps):
        fn()
    tot, n = C.c_double(), C.c_int64()
    gp._lib.bobe_gp_profile_read(gp._h, C.byref(tot), C.byref(n))
    gp._lib.bobe_gp_profile_select(gp._h, 0)
    return tot.value / reps


def rows(c):
    gp, cand, Z, lw = _setup(c)
    ev = Events(gp)
    mp = -(-M // 128) * 128
    gb = mp * c * 8 / 1e9
    out = []
    ta = ev.stats(lambda: gp.wip_sweep(cand, Z))
    sa = _scoring_ms(gp, lambda: gp.wip_sweep(cand, Z))
    out.append(f"{c:>6} | (a) wip_sweep                      {_cell(ta)} ms | scoring {sa * 1e3:8.1f} us, "
               f"{gb / sa:6.3f} TB/s of crossT, {c * M / sa / 1e6:7.2f} G pairs/s")
    for keys in SETS:
        f = lambda: gp.wip_sweep(cand, Z, log_weights=lw, criteria=keys)   # noqa: E731
        tb = ev.stats(f)
        sb = _scoring_ms(gp, f)
        out.append(f"{c:>6} | (b) weighted {'+'.join(keys):<21}{_cell(tb)} ms | scoring {sb * 1e3:8.1f} us, "
                   f"{gb / sb:6.3f} TB/s of crossT, {c * M / sb / 1e6:7.2f} G pairs/s | call / (a) = {tb[0] / ta[0]:.3f}")
    t1 = ev.stats(lambda: gp.wip_select_batch(cand, Z, 1, criterion="wipstd"))
    t5 = ev.stats(lambda: gp.wip_select_batch(cand, Z, 5, criterion="wipstd"))
    out.append(f"{c:>6} | (c) later stage, wipstd (equal weights)  {(t5[0] - t1[0]) / 4:8.3f} ms")
    for key in ("imiqr", "eiv"):
        t1 = ev.stats(lambda: gp.wip_select_batch_w(cand, Z, 1, criterion=key, log_weights=lw))
        t5 = ev.stats(lambda: gp.wip_select_batch_w(cand, Z, 5, criterion=key, log_weights=lw))
        out.append(f"{c:>6} | (c) later stage, {key:<6} (weights)        {(t5[0] - t1[0]) / 4:8.3f} ms")
    for ln in out:
        print("ROW " + ln, flush=True)


def sweep_only(c, lib=None):
    if lib:
        from bobe_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)
        have = C.CDLL(_lib.LIB_PATH)                         # (an older library lacks the entry points added since)
        _lib.SIGNATURES[:] = [sg for sg in _lib.SIGNATURES if hasattr(have, sg[0])]
    gp, cand, Z, _ = _setup(c)
    print("SWEEP %.4f" % Events(gp).stats(lambda: gp.wip_sweep(cand, Z))[0], flush=True)


def _child(args, limit=400):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + [str(a) for a in args],
                       capture_output=True, text=True)
    if p.returncode != 0:                                    # (nothing more is started on the GPU after a failed step)
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{args} failed with status {p.returncode}")
    return p.stdout.splitlines()


def table(out, parent_lib=None):
    lines = [f"# weighted criteria timing (tools/weighted_criteria_timing.py): bench's synthetic data, N = {N}, d = {D}, M = {M}, "
             "RBF, noise 1e-6",
             f"# HIP events on the handle's stream around whole calls; median [min, max] ms of {REPS} calls after a warm-up",
             "# scoring: the launches inside the sweep's scoring bracket (k_wip_score / k_wip_score_w), mean per call", ""]
    for c in POOLS:
        lines += [ln[4:] for ln in _child(["rows", c]) if ln.startswith("ROW ")]
    if parent_lib:
        lines += ["", f"# (e) wip_sweep, median ms of {REPS} calls per fresh process, this build and the parent commit's library "
                      f"alternating, {AB_ROUNDS} processes each"]
        for c in POOLS:
            new, old = [], []
            for _ in range(AB_ROUNDS):
                new.append(float([ln for ln in _child(["sweep", c]) if ln.startswith("SWEEP")][0].split()[1]))
                old.append(float([ln for ln in _child(["sweep", c, parent_lib]) if ln.startswith("SWEEP")][0].split()[1]))
            lines.append(f"{c:>6} | this build {' '.join('%.3f' % v for v in new)} | parent {' '.join('%.3f' % v for v in old)}"
                         f" | medians {np.median(new):.3f} / {np.median(old):.3f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    if sys.argv[1] == "rows":
        rows(int(sys.argv[2]))
    elif sys.argv[1] == "sweep":
        sweep_only(int(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_criteria_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
