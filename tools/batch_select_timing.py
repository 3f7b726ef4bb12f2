"""Time of a WIPV / WIPStd batch at bench's synthetic data (N = 4096, d = 8, M = 512, RBF, ls 0.6, noise 1e-6; candidates
C = 8192 and 65 536, batches of b = 4 and 8), HIP events on the handle's stream around calls that end in a synchronise:

  (a) one plain GP.wip_sweep;
  (b) the literal believer loop from the existing calls - copy, then per member wip_sweep, pick (a picked index masked),
      update at the predicted mean (none after the last member);
  (c) GP.wip_select_batch: stage 0 = the call with n_batch = 1 (the sweep with its intermediates kept, the call-local
      allocations included), the mean later stage = (the call with n_batch = b - stage 0) / (b - 1);
  (d) the later stage's achieved bytes/s against the (Np + 3 Mp) C 8 bytes it has to move (one pass over the retained V, a
      read-modify-write of crossT and the scorer's read of it).

Each figure is the median of REPS timed calls after a warm-up call (code objects, first allocations); min and max beside it.
Every GPU step is a process of its own under `timeout -k 10`: `table` starts one child per candidate pool (`rows C`) and one
profiled child, each under its own limit, and stops at the first that fails; run `table` itself the same way,

  timeout -k 10 900 python tools/batch_select_timing.py table && ...

  python tools/batch_select_timing.py table [OUT]           OUT defaults to profiles/batch_select_timing.txt
  python tools/batch_select_timing.py table OUT TRACEDIR    also the kernels of one C = 65 536, b = 8 call from a
                                                            rocprofv3 --kernel-trace --stats run of its own
  python tools/batch_select_timing.py rows C                the table rows of one candidate pool (what `table` starts)
  python tools/batch_select_timing.py run C B               what the profiled process runs: the GP's set-up, then ONE warm-up
                                                            call and ONE more call of wip_select_batch (two calls in all)
"""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, M = 4096, 8, 512
POOLS = (8192, 65536)
BATCHES = (4, 8)
REPS = 5
KEY = "wipstd"


def _setup(c):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, cand, Z = synthetic_problem(N, D, c, M, noise=1e-6)
    gp = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(D, 0.6), kernel_variance=1.0)
    return gp, np.ascontiguousarray(cand), np.ascontiguousarray(Z)


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


def believer_loop(gp, cand, Z, b):
    """The literal loop from the existing calls; returns the picks."""
    g = gp.copy()
    picks = []
    for j in range(b):
        sc = np.array(g.wip_sweep(cand, Z)[KEY])
        sc[picks] = np.inf
        p = int(np.argmin(sc))
        picks.append(p)
        if j + 1 < b:
            g.update(cand[p], g.predict_mean_single(cand[p]))
    return picks


def _kernel_stats(tracedir, c, b):
    out = os.path.join(tracedir, f"select_C{c}_b{b}")
    subprocess.run(["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                    os.path.abspath(__file__), "run", str(c), str(b)], check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel stats under {out}"
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].split("(")[0].replace("void ", "").replace("bobe::", "").strip()
        rows.append((float(r["TotalDurationNs"]) / 1e6, int(r["Calls"]), name))
    return sorted(rows, reverse=True)


def table(out, tracedir=None):
    lines = [f"# batch selection timing (tools/batch_select_timing.py): bench's synthetic data, N = {N}, d = {D}, M = {M}, RBF, "
             f"noise 1e-6, {KEY}",
             f"# HIP events on the handle's stream; median [min, max] ms of {REPS} calls after a warm-up; every call ends in a "
             "stream synchronise",
             "# (a) wip_sweep   (b) believer loop: copy + b x wip_sweep + (b - 1) x update   (c) wip_select_batch: stage 0 = the",
             "# call with n_batch = 1, later = (call with n_batch = b - stage 0) / (b - 1)   (d) (Np + 3 Mp) C 8 bytes / later",
             "",
             f"{'C':>6} {'b':>2} | {'(a) sweep ms':>22} | {'(b) believer loop ms':>24} | {'(c) select_batch ms':>24} | "
             f"{'stage 0 ms':>10} {'later ms':>9} | {'(d) GB':>7} {'TB/s':>6} | {'(b) / (c)':>9} | same picks"]
    failed = False
    for c in POOLS:
        p = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "rows", str(c)],
                           capture_output=True, text=True)
        if p.returncode != 0:                                # (nothing more is started on the GPU after a failed step)
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"the rows of C = {c} failed with status {p.returncode}")
        lines += [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        failed = failed or any("SLOWER" in ln for ln in p.stdout.splitlines())
    _finish(lines, out, tracedir, failed)


def rows(c):
    """The table rows of one candidate pool, printed as `ROW ...` lines."""
    np_, mp = -(-N // 128) * 128, -(-M // 128) * 128
    lines, slower = [], []
    gp, cand, Z = _setup(c)
    ev = Events(gp)
    ta = ev.stats(lambda: gp.wip_sweep(cand, Z))
    t0 = ev.stats(lambda: gp.wip_select_batch(cand, Z, 1, criterion=KEY))
    for b in BATCHES:
        tb = ev.stats(lambda: believer_loop(gp, cand, Z, b))
        tc = ev.stats(lambda: gp.wip_select_batch(cand, Z, b, criterion=KEY))
        same = believer_loop(gp, cand, Z, b) == gp.wip_select_batch(cand, Z, b, criterion=KEY)["indices"].tolist()
        later = (tc[0] - t0[0]) / (b - 1)
        gb = (np_ + 3 * mp) * c * 8 / 1e9
        cell = [f"{v[0]:8.2f} [{v[1]:.2f}, {v[2]:.2f}]" for v in (ta, tb, tc)]
        lines.append(f"{c:>6} {b:>2} | {cell[0]:>22} | {cell[1]:>24} | {cell[2]:>24} | {t0[0]:>10.2f} {later:>9.3f} | "
                     f"{gb:>7.3f} {gb / later:>6.2f} | {tb[0] / tc[0]:>9.2f} | {'yes' if same else 'NO'}")
        if not tc[0] < tb[0]:
            slower.append((c, b))
    del gp, ev
    for ln in lines:
        print("ROW " + ln, flush=True)
    for cb in slower:
        print("SLOWER", cb, flush=True)


def _finish(lines, out, tracedir, failed):
    if tracedir:
        c, b = POOLS[-1], BATCHES[-1]
        lines += ["", f"# kernels of a process that sets the GP up and makes TWO calls of wip_select_batch(C = {c}, n_batch = {b}) "
                  "- a warm-up and one more - (rocprofv3 --kernel-trace --stats): total ms over both calls, launches, kernel"]
        for ms, calls, name in _kernel_stats(tracedir, c, b)[:16]:
            lines.append(f"{ms:10.3f} {calls:6d}  {name[:150]}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)
    assert not failed, "wip_select_batch is not faster than the believer loop at every size (see the table)"


if __name__ == "__main__":
    if sys.argv[1] == "rows":
        rows(int(sys.argv[2]))
    elif sys.argv[1] == "run":
        c, b = int(sys.argv[2]), int(sys.argv[3])
        gp, cand, Z = _setup(c)
        for _ in range(2):
            gp.wip_select_batch(cand, Z, b, criterion=KEY)
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "batch_select_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
