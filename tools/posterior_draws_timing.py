"""Time of the joint posterior entry points at N = 4096, d = 8: bobe_gp_predict_cov at C = 1024 / 4096 / 16384 and
bobe_gp_posterior_sample (device normals, with the mean) at S = 64 / 1024 for C = 4096 / 16384, split into legs from
rocprofv3 --kernel-trace --stats (one profiled process per configuration), with the wall time per call of an unprofiled
process beside them.  Outputs are device buffers (hipMalloc), so the wall time holds no copy of the C x C result.

  python tools/posterior_draws_timing.py profile OUTDIR [TABLE]   all of it; TABLE defaults to OUTDIR/posterior_draws.txt
  python tools/posterior_draws_timing.py run cov|sample|setup C S REPS  one configuration (what the profiled processes run;
                                                                  setup: the GP alone, taken off the others)
  python tools/posterior_draws_timing.py wall                     the wall times of every configuration, one JSON line each

Work counted (flop): V = L^-1 K(X, Q) N^2 C (triangular), Sigma C^2 N (lower triangle of V^T V), potrf C^3 / 3 per
factorisation, TRMM S C^2; the fraction is of the nominal fp64 MFMA peak, 78.6 TF/s."""
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, REPS = 4096, 8, 3
PEAK = 78.6e12
CONFIGS = [("cov", 1024, 0), ("cov", 4096, 0), ("cov", 16384, 0),
           ("sample", 4096, 64), ("sample", 4096, 1024), ("sample", 16384, 64), ("sample", 16384, 1024)]
LEGS = {"V": ("k_kernel_matrix", "k_trimul", "k_blk_step", "k_colsum_parts", "k_scale_coords"),
        "Sigma": ("k_sigma_tiles",),
        "potrf": ("k_chol_panel", "k_potf2", "k_trsm_panel", "k_syrk_trail", "k_copy_diag", "k_sigma_load_jitter",
                  "k_mll_terms"),
        "TRMM": ("k_trmm_draws", "k_draw_normals", "k_zero_diag_upper")}


def _setup():
    from bobe_amd import GP
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(N, D))
    gp = GP(X, np.sin(X.sum(1)), noise=1e-4, lengthscales=np.full(D, 0.6))
    hip = C.CDLL("libamdhip64.so")
    return gp, hip, rng


def _dev(hip, nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
    return p


def _call(gp, what, q, c, s, out, seed):
    if what == "cov":
        st = gp._lib.bobe_gp_predict_cov(gp._h, q.ctypes.data, c, out)
    else:
        st = gp._lib.bobe_gp_posterior_sample(gp._h, q.ctypes.data, c, s, seed, None, 0, out, None)
    assert st == 0, (what, c, s, st)


def run(what, c, s, reps, gp=None, hip=None, rng=None):
    if gp is None:
        gp, hip, rng = _setup()
    if what == "setup":
        return 0.0
    q = np.ascontiguousarray(rng.uniform(size=(c, D)))
    out = _dev(hip, 8 * (c * c if what == "cov" else s * c))
    _call(gp, what, q, c, s, out, 0)                    # warm-up (code objects, the first allocations)
    t = []
    for i in range(reps):
        t0 = time.perf_counter()
        _call(gp, what, q, c, s, out, i + 1)            # (both entry points synchronise before they return)
        t.append(time.perf_counter() - t0)
    hip.hipFree(out)
    return float(np.median(t)) * 1e3


def _stats(d):
    """kernel milliseconds per leg of a profiled process"""
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel stats under {d}"
    legs = {k: 0.0 for k in LEGS}
    legs["other"] = 0.0
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].split("(")[0].split("<")[0].replace("void ", "").replace("bobe::", "").strip()
        leg = next((k for k, v in LEGS.items() if name in v), "other")
        legs[leg] += float(r["TotalDurationNs"]) / 1e6
    return legs


def _profiled(outdir, what, c, s, reps):
    d = os.path.join(outdir, f"{what}_C{c}_S{s}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                    os.path.abspath(__file__), "run", what, str(c), str(s), str(reps)], check=True, timeout=600,
                   stdout=subprocess.DEVNULL)
    return _stats(d)


def profile(outdir, table):
    os.makedirs(outdir, exist_ok=True)
    wall = subprocess.run([sys.executable, os.path.abspath(__file__), "wall"], capture_output=True, text=True, timeout=600,
                          check=True).stdout.strip().splitlines()
    wall = {(w["what"], w["C"], w["S"]): w["ms"] for w in map(json.loads, wall)}
    # (the set-up - the GP's own factorisation at N = 4096 - is profiled alone and taken off every configuration)
    base = _profiled(outdir, "setup", 0, 0, 0)
    rows = []
    for what, c, s in CONFIGS:
        legs = _profiled(outdir, what, c, s, REPS)
        legs = {k: max(0.0, v - base[k]) / (REPS + 1) for k, v in legs.items()}      # ms per call (warm-up included)
        rows.append((what, c, s, legs, wall[(what, c, s)]))
    work = {"V": lambda c, s: N * N * c, "Sigma": lambda c, s: c * c * N, "potrf": lambda c, s: c ** 3 / 3.0,
            "TRMM": lambda c, s: s * c * c}
    lines = ["# joint posterior at N = 4096, d = 8 (RBF, noise 1e-4, plain product: the factor's kappa is below 1e6):",
             "# bobe_gp_predict_cov (cov) and bobe_gp_posterior_sample (sample: device normals, mean added)",
             "# ms per call and leg: rocprofv3 --kernel-trace --stats (kernel time of 4 calls, the warm-up included, less a",
             "# profiled set-up-only process, / 4);",
             "# wall: median host time of 3 calls in an unprofiled process (device outputs).  TF/s = counted work / leg time;",
             "# %pk = fraction of the nominal fp64 MFMA peak 78.6 TF/s.  Work: V N^2 C, Sigma C^2 N, potrf C^3/3, TRMM S C^2",
             "",
             f"{'call':7s} {'C':>6s} {'S':>5s} | {'V ms':>8s} {'TF/s':>6s} {'%pk':>5s} | {'Sigma ms':>8s} {'TF/s':>6s} {'%pk':>5s} | "
             f"{'potrf ms':>8s} {'TF/s':>6s} {'%pk':>5s} | {'TRMM ms':>8s} {'TF/s':>6s} {'%pk':>5s} | {'other':>6s} | {'wall ms':>8s}"]
    for what, c, s, legs, w in rows:
        cells = []
        for k in ("V", "Sigma", "potrf", "TRMM"):
            ms = legs[k]
            if ms <= 0 or (what == "cov" and k in ("potrf", "TRMM")):
                cells.append(f"{'-':>8s} {'-':>6s} {'-':>5s}")
                continue
            tf = work[k](c, s) / (ms * 1e-3) / 1e12
            cells.append(f"{ms:8.2f} {tf:6.1f} {100 * tf * 1e12 / PEAK:5.1f}")
        lines.append(f"{what:7s} {c:6d} {s:5d} | " + " | ".join(cells) + f" | {legs['other']:6.2f} | {w:8.1f}")
    text = "\n".join(lines) + "\n"
    open(table, "w").write(text)
    print(text)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "run":
        run(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    elif mode == "wall":
        gp, hip, rng = _setup()
        for what, c, s in CONFIGS:
            print(json.dumps({"what": what, "C": c, "S": s, "ms": run(what, c, s, REPS, gp, hip, rng)}), flush=True)
    else:
        out = sys.argv[2]
        profile(out, sys.argv[3] if len(sys.argv) > 3 else os.path.join(out, "posterior_draws.txt"))
