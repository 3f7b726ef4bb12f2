"""Cost of the evidence-variance sweep (bobe_gp_wip_sweep_zvar, bobe_gp_wip_select_batch_zvar) at bench's synthetic data:
N = 4096, d = 8, RBF, ls 0.6, noise 1e-6; candidate pools C = 8192 and 65 536, integration points M = 128 and 512.  HIP events
on the handle's stream around whole calls (each ends in a stream synchronise); every figure is the median [min, max] of REPS
calls after a warm-up.

  (a) wip_sweep(log_weights=, criteria=('eiv',))   the weighted sweep it rides on, one criterion
  (b) wip_sweep(log_weights=, criteria=('zvar',))  the same sweep with the pair scorer instead
  (c) the scoring launches alone                   bobe_gp_profile_select(cross) around the same calls: k_wip_score_w for (a),
                                                   k_wip_score_zz for (b), with the pair terms C M (M + 1) / 2 per second
  (d) a batch of 4                                 wip_select_batch_w(n_batch=4), eiv and zvar
  (e) the eiv-only sweep on this build and on a library built from the parent commit (PARENT_LIB), alternating fresh processes

  python tools/zvar_timing.py table [OUT [PARENT_LIB]]     OUT defaults to profiles/zvar_timing.txt
  python tools/zvar_timing.py rows C M                     the rows of one shape (what `table` starts)
  python tools/zvar_timing.py eiv C M [LIB]                median eiv-only sweep ms of one fresh process (for (e))

Every GPU step is a process of its own under `timeout -k 10`; `table` stops at the first that fails.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from weighted_criteria_timing import Events, _cell, _scoring_ms  # noqa: E402

N, D = 4096, 8
SHAPES = ((8192, 128), (8192, 512), (65536, 128), (65536, 512))
REPS = 11
AB_ROUNDS = 3


def _setup(c, m):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, cand, Z = synthetic_problem(N, D, c, m, noise=1e-6)
    gp = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(D, 0.6), kernel_variance=1.0)
    lw = 1.5 * np.random.default_rng(1).normal(size=m)
    return gp, np.ascontiguousarray(cand), np.ascontiguousarray(Z), lw


def rows(c, m):
    gp, cand, Z, lw = _setup(c, m)
    ev = Events(gp)
    pairs = c * m * (m + 1) / 2
    out = []
    fe = lambda: gp.wip_sweep(cand, Z, log_weights=lw, criteria=("eiv",))      # noqa: E731
    fz = lambda: gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",))     # noqa: E731
    te, tz = ev.stats(fe, REPS), ev.stats(fz, REPS)
    se, sz = _scoring_ms(gp, fe, REPS), _scoring_ms(gp, fz, REPS)
    head = f"{c:>6} x {m:>3}"
    out.append(f"{head} | (a) sweep, eiv only   {_cell(te)} ms | scoring {se:9.3f} ms")
    out.append(f"{head} | (b) sweep, zvar       {_cell(tz)} ms | scoring {sz:9.3f} ms, {pairs / sz / 1e6:8.2f} G pair terms/s"
               f" | call / (a) = {tz[0] / te[0]:.2f}")
    be = ev.stats(lambda: gp.wip_select_batch_w(cand, Z, 4, criterion="eiv", log_weights=lw), REPS)
    bz = ev.stats(lambda: gp.wip_select_batch_w(cand, Z, 4, criterion="zvar", log_weights=lw), REPS)
    out.append(f"{head} | (d) batch of 4, eiv   {_cell(be)} ms")
    out.append(f"{head} | (d) batch of 4, zvar  {_cell(bz)} ms")
    for ln in out:
        print("ROW " + ln, flush=True)


def eiv_only(c, m, lib=None):
    if lib:
        from bobe_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)
        have = C.CDLL(_lib.LIB_PATH)                         # (an older library lacks the entry points added since)
        _lib.SIGNATURES[:] = [sg for sg in _lib.SIGNATURES if hasattr(have, sg[0])]
    gp, cand, Z, lw = _setup(c, m)
    t = Events(gp).stats(lambda: gp.wip_sweep(cand, Z, log_weights=lw, criteria=("eiv",)), 21)
    print("EIV %.4f" % t[0], flush=True)


def _child(args, limit=400):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + [str(a) for a in args],
                       capture_output=True, text=True)
    if p.returncode != 0:                                    # (nothing more is started on the GPU after a failed step)
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{args} failed with status {p.returncode}")
    return p.stdout.splitlines()


def table(out, parent_lib=None):
    lines = [f"# evidence-variance sweep timing (tools/zvar_timing.py): bench's synthetic data, N = {N}, d = {D}, RBF, noise 1e-6",
             f"# HIP events on the handle's stream around whole calls; median [min, max] ms of {REPS} calls after a warm-up",
             "# scoring: the launches inside the sweep's scoring bracket (k_wip_score_w / k_wip_score_zz), mean ms per call",
             "# C x M", ""]
    for c, m in SHAPES:
        got = [ln[4:] for ln in _child(["rows", c, m]) if ln.startswith("ROW ")]
        for ln in got:
            print(ln, flush=True)
        lines += got
    if parent_lib:
        lines += ["", "# (e) the eiv-only sweep, median ms of 21 calls per fresh process, this build and the parent commit's library "
                      f"alternating, {AB_ROUNDS} processes each"]
        for c, m in ((8192, 512), (65536, 512)):
            new, old = [], []
            for _ in range(AB_ROUNDS):
                new.append(float([ln for ln in _child(["eiv", c, m]) if ln.startswith("EIV")][0].split()[1]))
                old.append(float([ln for ln in _child(["eiv", c, m, parent_lib]) if ln.startswith("EIV")][0].split()[1]))
            ln = (f"{c:>6} x {m:>3} | this build {' '.join('%.3f' % v for v in new)} | parent {' '.join('%.3f' % v for v in old)}"
                  f" | medians {np.median(new):.3f} / {np.median(old):.3f}")
            print(ln, flush=True)
            lines.append(ln)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)


if __name__ == "__main__":
    if sys.argv[1] == "rows":
        rows(int(sys.argv[2]), int(sys.argv[3]))
    elif sys.argv[1] == "eiv":
        eiv_only(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] if len(sys.argv) > 4 else None)
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "zvar_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
