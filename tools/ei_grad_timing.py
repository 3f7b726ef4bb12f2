"""Time of the EI / LogEI input gradients on the benchmark's synthetic data at d = 8 (RBF):

  1. one GP.acq_ei_grad call beside the pair it replaces, GP.predict_grad + GP.acq_ei on the same points, for C in
     {1, 16, 50} points at N in {400, 1200, 4096};
  2. one whole EI.get_next_point and LogEI.get_next_point (50 restarts, maxiter 1000: what BOBE.run_EI asks for) with
     acq_kwargs['ei_lockstep'] on and off, on the same GP and the same seed, at N in {400, 1200}.  The off path is the
     default, untouched: the baseline.

  python tools/ei_grad_timing.py [TABLE]        TABLE defaults to profiles/ei_grad_timing.txt

Wall-clock time around whole calls (every call ends with its own stream synchronisation and hands back host arrays, and the
host's share is what the comparison is about); one warm-up call, then min / median / max of 21 calls (part 1) or 9 (part 2).  The
median is the figure; the maximum shows single slow calls (one of ~30 ms among the 0.7 ms ones recurs at N = 1200, C = 1, LogEI in
two runs; its cause was not looked for)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
N_CALL, C_LIST, REPS_CALL = (400, 1200, 4096), (1, 16, 50), 21
N_LOOP, REPS_LOOP, RESTARTS, MAXITER = (400, 1200), 9, 50, 1000


def _timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return min(t), float(np.median(t)), max(t)


class _Count:
    """device calls of a GP, by entry"""

    def __init__(self, gp):
        self.n = {"acq_ei_grad": 0, "predict_grad": 0, "acq_ei": 0}
        for name in self.n:
            setattr(gp, name, self._wrap(name, getattr(gp, name)))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return counted

    def total(self):
        return sum(self.n.values())

    def reset(self):
        for k in self.n:
            self.n[k] = 0


def main(table):
    from bobe_amd import GP
    from bobe_amd import acquisition as A
    from bobe_amd.synthetic import synthetic_problem
    lines = [f"# EI / LogEI input gradients at d = {D} (bench's synthetic data, RBF, ls 0.6, noise 1e-6); wall-clock ms around whole",
             f"# calls with host arrays in and out, min / median / max of {REPS_CALL} calls after a warm-up.",
             "# pair = GP.predict_grad + GP.acq_ei on the same points (the two device calls of the default EI._value_and_grad)",
             "# (the median is the figure; a maximum far above it is one slow call among the 21, its cause not looked for)", "",
             f"{'N':>5s} {'C':>3s} {'mode':>5s} | {'acq_ei_grad':>23s} | {'predict_grad + acq_ei':>23s} | {'pair/new':>8s}"]
    gps = {}
    for n in N_CALL:
        X, y, cand, _ = synthetic_problem(n, D, max(C_LIST), 8)
        gp = gps[n] = GP(X, y, noise=1e-6, lengthscales=np.full(D, 0.6), kernel_variance=1.0)
        best = float(np.max(gp.train_y))
        for c in C_LIST:
            q = np.ascontiguousarray(cand[:c])
            for log_ei in (False, True):
                a = _timed(lambda: gp.acq_ei_grad(q, best, 0.01, log_ei=log_ei), REPS_CALL)
                b = _timed(lambda: (gp.predict_grad(q), gp.acq_ei(q, best, 0.01, log_ei=log_ei)), REPS_CALL)
                lines.append(f"{n:5d} {c:3d} {'logei' if log_ei else 'ei':>5s} | {a[0]:7.3f} {a[1]:7.3f} {a[2]:7.3f} | "
                             f"{b[0]:7.3f} {b[1]:7.3f} {b[2]:7.3f} | {b[1] / a[1]:8.2f}")
                print(lines[-1], flush=True)
    lines += ["", f"# one get_next_point, {RESTARTS} restarts, maxiter {MAXITER}, zeta 0.01, the same GP and generator seed on and off; wall-clock",
              f"# ms of the whole call, min / median / max of {REPS_LOOP} after a warm-up; calls = device calls of one get_next_point;",
              "# value = the acquisition value returned (the two paths walk different roundings of the same objective)",
              f"{'N':>5s} {'acq':>6s} {'lockstep':>8s} | {'get_next_point':>29s} | {'calls':>7s} | {'value':>13s}"]
    for n in N_LOOP:
        gp = gps[n]
        cnt = _Count(gp)
        for name in ("EI", "LogEI"):
            med = {}
            for on in (False, True):
                kw = {"zeta": 0.01}
                if on:
                    kw["ei_lockstep"] = True
                res = {}

                def run():
                    cnt.reset()
                    res["r"] = getattr(A, name)().get_next_point(gp, acq_kwargs=dict(kw), maxiter=MAXITER, n_restarts=RESTARTS,
                                                                verbose=False, rng=np.random.default_rng(7))
                t = _timed(run, REPS_LOOP)
                med[on] = t[1]
                lines.append(f"{n:5d} {name:>6s} {'on' if on else 'off':>8s} | {t[0]:9.1f} {t[1]:9.1f} {t[2]:9.1f} | {cnt.total():7d} | "
                             f"{float(res['r'][1]):13.6e}")
                print(lines[-1], flush=True)
            lines.append(f"{n:5d} {name:>6s}   off/on | {med[False] / med[True]:9.2f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(table)), exist_ok=True)
    with open(table, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ei_grad_timing.txt"))
