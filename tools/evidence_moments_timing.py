"""Cost of the total evidence variance (bobe_gp_evidence_moments) at bench's synthetic data: d = 8, RBF, ls 0.6, noise 1e-6;
N = 4096 with M = 512, 4096, 16 384, 65 536 integration points and N = 1024 with M = 512, 4096.  HIP events on the handle's
stream around whole calls (each ends in a stream synchronise); every figure is the median [min, max] of REPS calls after a
warm-up.

  (a) evidence_moments, a fresh Z every call    prepare_z (assembly, solve), the per-z table, the three launches
  (b) evidence_moments, the same host Z again   the cache of Z's quantities hit: the table and the three launches
  (c) the pair launch alone                     bobe_gp_profile_select(crossvv) around (b): k_evid_pairs, with the fraction of
                                                the fp64 MFMA peak its product alone amounts to (nt (nt + 1) / 2 tiles x
                                                2 x 128 x 128 x Np flops; PEAK_TFLOPS) and the pair terms per second
  (d) the yardstick, M <= 16 384                bobe_gp_predict_cov into device memory at the same points, and its Sigma pass
                                                alone (k_sigma_tiles, the same bracket): the same product with two stores per
                                                element where the pair launch has one transcendental and no store
  (e) bobe_gp_wip_sweep_zvar (C = 8192, M = 512) and bobe_gp_predict_cov (C = 4096) on this build and on a library built from
      the parent commit (PARENT_LIB), alternating fresh processes

  python tools/evidence_moments_timing.py table [OUT [PARENT_LIB]]   OUT defaults to profiles/evidence_moments_timing.txt
  python tools/evidence_moments_timing.py rows N M                   the rows of one shape (what `table` starts)
  python tools/evidence_moments_timing.py ab [LIB]                   (e)'s two medians of one fresh process
  python tools/evidence_moments_timing.py one N M                    five calls of (b) and one of (d): a kernel-statistics run

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
from weighted_criteria_timing import Events, _cell  # noqa: E402

D = 8
SHAPES = ((4096, 512), (4096, 4096), (4096, 16384), (4096, 65536), (1024, 512), (1024, 4096))
REPS = 21
AB_ROUNDS = 3
PEAK_TFLOPS = 78.6          # MI355X, fp64 matrix (the data sheet's figure)
SIGMA_MAX = 16384


def _setup(n, m, c=16):
    from bobe_amd import GP
    from bobe_amd.synthetic import synthetic_problem
    X, y, cand, Z = synthetic_problem(n, D, c, m, noise=1e-6)
    gp = GP(X, y, noise=1e-6, kernel="rbf", lengthscales=np.full(D, 0.6), kernel_variance=1.0)
    lw = 1.5 * np.random.default_rng(1).normal(size=m)
    return gp, np.ascontiguousarray(cand), np.ascontiguousarray(Z), lw


def _bracket_ms(gp, fn, reps):
    """Mean milliseconds per call of the launches inside the handle's `crossvv` bracket (k_evid_pairs / k_sigma_tiles)."""
    from bobe_amd import _lib
    fn()
    gp._lib.bobe_gp_profile_select(gp._h, _lib.PROF["crossvv"])
    for _ in range(reps):
        fn()
    tot, cnt = C.c_double(), C.c_int64()
    gp._lib.bobe_gp_profile_read(gp._h, C.byref(tot), C.byref(cnt))
    gp._lib.bobe_gp_profile_select(gp._h, 0)
    return tot.value / reps


def _predict_cov_dev(gp, Z):
    import torch
    from bobe_amd import _lib
    m = Z.shape[0]
    out = torch.empty((m, m), dtype=torch.float64, device="cuda")

    def call():
        _lib.check(gp._lib.bobe_gp_predict_cov(gp._h, _lib.ptr(Z), m, _lib.ptr(out)), "bobe_gp_predict_cov")
    return call


def rows(n, m):
    gp, _, Z, lw = _setup(n, m)
    ev = Events(gp)
    Z2 = np.ascontiguousarray(Z[::-1])
    flip = [0]

    def fresh():                                             # (two point sets in turn: every call misses the cache)
        flip[0] ^= 1
        gp.evidence_moments(Z2 if flip[0] else Z, log_weights=lw)

    def again():
        gp.evidence_moments(Z, log_weights=lw)
    ta, tb = ev.stats(fresh, REPS), ev.stats(again, REPS)
    pm = _bracket_ms(gp, again, REPS)
    nt = -(-m // 128)
    npad = -(-n // 128) * 128
    tiles = nt * (nt + 1) // 2
    tf = tiles * 2.0 * 128 * 128 * npad / (pm * 1e-3) / 1e12
    r = gp.evidence_moments(Z, log_weights=lw)
    head = f"N {n:>4} M {m:>5}"
    out = [f"{head} | (a) fresh Z      {_cell(ta)} ms | (b) cached Z {_cell(tb)} ms | log_t0 {r['log_t0']:.6g}",
           f"{head} | (c) k_evid_pairs {pm:9.3f} ms, {tiles} tiles, {tf:6.2f} TFLOP/s = {100 * tf / PEAK_TFLOPS:5.1f} % of the fp64 "
           f"MFMA peak, {m * (m + 1) / 2 / pm / 1e6:8.2f} G pair terms/s"]
    if m <= SIGMA_MAX:
        pc = _predict_cov_dev(gp, Z)
        tc = ev.stats(pc, REPS)
        sm = _bracket_ms(gp, pc, REPS)
        out.append(f"{head} | (d) predict_cov  {_cell(tc)} ms | k_sigma_tiles {sm:9.3f} ms | pair launch / Sigma pass = {pm / sm:.2f}")
    for ln in out:
        print("ROW " + ln, flush=True)


def ab(lib=None):
    if lib:
        from bobe_amd import _lib
        _lib.LIB_PATH = os.path.abspath(lib)
        have = C.CDLL(_lib.LIB_PATH)                         # (an older library lacks the entry points added since)
        _lib.SIGNATURES[:] = [sg for sg in _lib.SIGNATURES if hasattr(have, sg[0])]
    gp, cand, Z, lw = _setup(4096, 512, 8192)
    ev = Events(gp)
    tz = ev.stats(lambda: gp.wip_sweep(cand, Z, log_weights=lw, criteria=("zvar",)), 11)
    tc = ev.stats(_predict_cov_dev(gp, np.ascontiguousarray(cand[:4096])), REPS)
    print("AB %.4f %.4f" % (tz[0], tc[0]), flush=True)


def one(n, m):
    gp, _, Z, lw = _setup(n, m)
    for _ in range(5):
        gp.evidence_moments(Z, log_weights=lw)
    if m <= SIGMA_MAX:
        _predict_cov_dev(gp, Z)()


def _child(args, limit=400):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + [str(a) for a in args],
                       capture_output=True, text=True)
    if p.returncode != 0:                                    # (nothing more is started on the GPU after a failed step)
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"{args} failed with status {p.returncode}")
    return p.stdout.splitlines()


def table(out, parent_lib=None):
    lines = [f"# total evidence variance timing (tools/evidence_moments_timing.py): bench's synthetic data, d = {D}, RBF, noise 1e-6",
             f"# HIP events on the handle's stream around whole calls; median [min, max] ms of {REPS} calls after a warm-up",
             "# (c), k_sigma_tiles: the launches inside the handle's crossvv bracket, mean ms per call", ""]
    for n, m in SHAPES:
        got = [ln[4:] for ln in _child(["rows", n, m]) if ln.startswith("ROW ")]
        for ln in got:
            print(ln, flush=True)
        lines += got
    if parent_lib:
        lines += ["", "# (e) wip_sweep(criteria=('zvar',)) at C = 8192, M = 512 (median of 11) and predict_cov at C = 4096 (median of "
                      f"{REPS}), ms per fresh process, this build and the parent commit's library alternating, {AB_ROUNDS} processes each"]
        new, old = [], []
        for _ in range(AB_ROUNDS):
            new.append([float(v) for v in [ln for ln in _child(["ab"]) if ln.startswith("AB")][0].split()[1:]])
            old.append([float(v) for v in [ln for ln in _child(["ab", parent_lib]) if ln.startswith("AB")][0].split()[1:]])
        for k, name in enumerate(("wip_sweep zvar", "predict_cov   ")):
            a, b = [v[k] for v in new], [v[k] for v in old]
            ln = (f"{name} | this build {' '.join('%.3f' % v for v in a)} | parent {' '.join('%.3f' % v for v in b)}"
                  f" | medians {np.median(a):.3f} / {np.median(b):.3f}")
            print(ln, flush=True)
            lines.append(ln)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)


if __name__ == "__main__":
    if sys.argv[1] == "rows":
        rows(int(sys.argv[2]), int(sys.argv[3]))
    elif sys.argv[1] == "ab":
        ab(sys.argv[2] if len(sys.argv) > 2 else None)
    elif sys.argv[1] == "one":
        one(int(sys.argv[2]), int(sys.argv[3]))
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "evidence_moments_timing.txt"),
              sys.argv[3] if len(sys.argv) > 3 else None)
