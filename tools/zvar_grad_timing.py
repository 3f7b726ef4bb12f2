"""Cost of the evidence-variance score's gradient (bobe_gp_wip_grad_zvar) beside bobe_gp_wip_grad_w, and of the polish built on
it, on the benchmark's synthetic data (RBF, ls 0.6, noise 1e-6, d = 8).  Every library figure is the median of REPS calls after
two warm-up calls, in milliseconds between two HIP events recorded on the handle's stream around the whole call (it ends in a
stream synchronise); host pointers throughout, the z-side caches hit (the same Z again: what a polish sees after its first
round).

  one call at C in {1, 16}, N in {400, 4096}, M in {64, 512, 4096} of (a) bobe_gp_wip_grad_w with one criterion (wipstd) and
  (b) bobe_gp_wip_grad_zvar, on the same handle, Z, log-weights and candidates - the two share every stage but the middle
  one, so b - a is the pair pass (M^2 terms per candidate) and its two small neighbours against k_wg_weights_w;
  one ZVar.get_next_point with acq_kwargs['zvar_polish'] = 4 beside the unpolished one, which is the pool sweep it starts
  from (N = 400, M = 128; wall clock of the whole call, the second of two) and how far the score moves, on three seeds.

  python tools/zvar_grad_timing.py [OUT]          OUT defaults to profiles/zvar_grad_timing.txt
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from weighted_grad_timing import D, Events, _setup  # noqa: E402

NS, MS, CS = (400, 4096), (64, 512, 4096), (1, 16)
REPS = 15


def _calls(gp, m, c, seed=0):
    from bobe_amd import _lib
    lib, h, d = gp._lib, gp._h, gp.ndim
    rng = np.random.default_rng(seed)
    cand, lw, Z = rng.uniform(0.1, 0.9, size=(c, d)), 1.5 * rng.normal(size=m), rng.uniform(size=(m, d))
    val, grad = np.empty(c), np.empty((c, d))
    ystd = float(gp.y_std)
    ps, pg = (C.c_void_p * 4)(None, val.ctypes.data, None, None), (C.c_void_p * 4)(None, grad.ctypes.data, None, None)

    def wipstd():
        assert lib.bobe_gp_wip_grad_w(h, _lib.ptr(cand), c, _lib.ptr(Z), m, ystd, _lib.ptr(lw), ps, pg) == 0
        assert np.all(np.isfinite(grad))

    def zvar():
        assert lib.bobe_gp_wip_grad_zvar(h, _lib.ptr(cand), c, _lib.ptr(Z), m, ystd, _lib.ptr(lw), _lib.ptr(val), _lib.ptr(grad),
                                         None) == 0
        assert not np.any(np.isnan(grad))
    return wipstd, zvar


def _polish_rows():
    from bobe_amd.acquisition import ZVar
    gp = _setup(400)
    rows = []
    for seed in (0, 1, 2):
        rng = np.random.default_rng(40 + seed)
        kw = {"mc_samples": {"x": rng.uniform(size=(1024, D))}, "mc_points_size": 128}
        t = {}
        for r in (0, 4):
            ZVar().get_next_point(gp, acq_kwargs=dict(kw, zvar_polish=r), rng=np.random.default_rng(seed), verbose=False)
            t0 = time.perf_counter()
            x, v = ZVar().get_next_point(gp, acq_kwargs=dict(kw, zvar_polish=r), rng=np.random.default_rng(seed), verbose=False)
            t[r] = (1e3 * (time.perf_counter() - t0), float(v), np.array(x))
        rows.append(f"{seed:>4} | {t[0][0]:>13.3f} | {t[4][0]:>11.3f} | {t[0][1]:>14.8f} | {t[4][1]:>14.8f} | "
                    f"{t[0][1] - t[4][1]:>10.3e} | {float(np.max(np.abs(t[4][2] - t[0][2]))):>9.3e}")
    return rows


def table(out):
    lines = ["# the evidence-variance score's gradient (tools/zvar_grad_timing.py): bench's synthetic data, RBF, noise 1e-6, d = 8; "
             f"median ms of {REPS} whole calls after two warm-up calls, HIP events on the handle's stream, host pointers, z-side "
             "caches hit",
             "# a = bobe_gp_wip_grad_w with one criterion (wipstd), b = bobe_gp_wip_grad_zvar: the same handle, Z, log-weights "
             "and candidates", "", f"{'N':>5} {'M':>5} {'C':>3} | {'a':>9} {'b':>9} | {'b - a':>9} | {'(b - a) / (C M^2) ns':>21}"]
    for n in NS:
        gp = _setup(n)
        ev = Events(gp)
        for m in MS:
            for c in CS:
                wipstd, zvar = _calls(gp, m, c)
                a, b = ev.median(wipstd, REPS), ev.median(zvar, REPS)
                lines.append(f"{n:>5} {m:>5} {c:>3} | {a:>9.4f} {b:>9.4f} | {b - a:>9.4f} | {1e6 * (b - a) / (c * m * m):>21.5f}")
        del gp
    lines += ["", "# ZVar.get_next_point, N = 400, M = 128, a pool of 1024 uniform samples: acq_kwargs['zvar_polish'] = 0 (the pool "
              "sweep alone) / 4 (wall clock of the whole call, the second of two), the scores and how far the pick moves (max-norm)",
              "", f"{'seed':>4} | {'unpolished ms':>13} | {'polished ms':>11} | {'pool score':>14} | {'polished score':>14} | "
              f"{'gain':>10} | {'moved':>9}"] + _polish_rows()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    table(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "zvar_grad_timing.txt"))
