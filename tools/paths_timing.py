"""Time of the pathwise posterior draws at N = 4096, d = 8 (RBF, noise 1e-4): bobe_gp_paths_create, bobe_gp_paths_eval and
bobe_gp_paths_argmax for S in {16, 128} paths, F in {1024, 4096} features and C in {16 384, 65 536, 262 144} queries, with
bobe_gp_posterior_sample at its cap C = 16 384 and one bobe_gp_predict sweep (k_trimul's rate) beside them.

  python tools/paths_timing.py [TABLE]        TABLE defaults to profiles/paths_timing.txt

Wall times: host time around a call that synchronises the handle's stream before it returns (device inputs and outputs: no
copy of the S x C result), one warm-up call, then REPS calls: min / median / max.  The legs inside bobe_gp_paths_eval come from
the library's event timer (bobe_gp_profile_select: `kxc` = K(Q, X) and Phi(Q) assembly, `crossvv` = the tile product) summed
over the chunks of one further call.  GEMM rate: 2 C Sp (Np + Fp) flop, Sp = S padded to the tile edge picked from S (32 / 64 /
128), over the product's time, against the nominal fp64 MFMA peak of 78.6 TF/s."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, REPS = 4096, 8, 5
PEAK = 78.6e12
S_LIST, F_LIST, C_LIST = (16, 128), (1024, 4096), (16384, 65536, 262144)


def _timed(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t)), max(t)


def _leg(gp, tag, fn):
    from bobe_amd import _lib
    tot, n = C.c_double(0.0), C.c_int64(0)
    gp._lib.bobe_gp_profile_select(gp._h, _lib.PROF[tag])
    fn()
    gp._lib.bobe_gp_profile_read(gp._h, C.byref(tot), C.byref(n))
    gp._lib.bobe_gp_profile_select(gp._h, 0)
    return tot.value


def main(table):
    import torch
    from bobe_amd import GP
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(N, D))
    gp = GP(X, np.sin(X.sum(1)), noise=1e-4, lengthscales=np.full(D, 0.6))
    lib = gp._lib
    xq = torch.tensor(rng.uniform(size=(max(C_LIST), D)), dtype=torch.float64, device="cuda")
    out = torch.empty(max(S_LIST) * max(C_LIST), dtype=torch.float64, device="cuda")
    idx = torch.empty(max(S_LIST), dtype=torch.int64, device="cuda")
    best = torch.empty(max(S_LIST), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lines = [f"# pathwise posterior draws at N = {N}, d = {D} (RBF, noise 1e-4, plain product); ms, min / median / max of {REPS} calls",
             "# after a warm-up; device inputs and outputs; kxc / gemm: the assembly and tile-product legs of one eval call",
             "# (library event timer, summed over its chunks); TF/s = 2 C Sp (Np + Fp) / gemm time, %pk of 78.6 TF/s", "",
             f"{'S':>4s} {'F':>5s} {'C':>7s} | {'create':>20s} | {'eval':>23s} | {'argmax':>23s} | {'kxc':>8s} {'gemm':>8s} {'TF/s':>6s} {'%pk':>5s}"]
    for s in S_LIST:
        for f in F_LIST:
            holder = {}

            def create():
                if "p" in holder:
                    holder.pop("p").close()
                holder["p"] = gp.sample_paths(s, f, seed=1)
            tc = _timed(create, 3)
            ps = holder["p"]
            sp = 32 if s <= 32 else (64 if s <= 64 else 128 * ((s + 127) // 128))
            fp = 32 * ((f + 31) // 32)
            for c in C_LIST:
                def ev():
                    assert lib.bobe_gp_paths_eval(ps._h, xq.data_ptr(), c, 0, out.data_ptr()) == 0

                def am():
                    assert lib.bobe_gp_paths_argmax(ps._h, xq.data_ptr(), c, None, idx.data_ptr(), best.data_ptr()) == 0
                te, ta = _timed(ev), _timed(am)
                kxc, gemm = _leg(gp, "kxc", ev), _leg(gp, "crossvv", ev)
                tf = 2.0 * c * sp * (N + fp) / (gemm * 1e-3) / 1e12
                lines.append(f"{s:4d} {f:5d} {c:7d} | {tc[0]:6.1f} {tc[1]:6.1f} {tc[2]:6.1f} | {te[0]:7.1f} {te[1]:7.1f} {te[2]:7.1f} | "
                             f"{ta[0]:7.1f} {ta[1]:7.1f} {ta[2]:7.1f} | {kxc:8.2f} {gemm:8.2f} {tf:6.2f} {100 * tf * 1e12 / PEAK:5.1f}")
                print(lines[-1], flush=True)
            ps.close()
    # beside them: the dense joint draws at their cap, and the sweep's triangular product (N^2 C flop) of one prediction
    c = 16384
    lines += ["", "# bobe_gp_posterior_sample (dense C x C covariance and its factor) at its cap C = 16384, device normals, with the mean"]
    for s in S_LIST:
        def dense():
            assert lib.bobe_gp_posterior_sample(gp._h, xq.data_ptr(), c, s, 1, None, 0, out.data_ptr(), None) == 0
        t = _timed(dense, 3)
        lines.append(f"{s:4d} {'-':>5s} {c:7d} | {t[0]:7.1f} {t[1]:7.1f} {t[2]:7.1f}")
        print(lines[-1], flush=True)
    mean = torch.empty(c, dtype=torch.float64, device="cuda")
    var = torch.empty(c, dtype=torch.float64, device="cuda")

    def predict():
        assert lib.bobe_gp_predict(gp._h, xq.data_ptr(), c, mean.data_ptr(), var.data_ptr(), 1) == 0
    predict()
    tri = _leg(gp, "trimul", predict)
    tf = float(N) * N * c / (tri * 1e-3) / 1e12
    lines += ["", f"# k_trimul of bobe_gp_predict at C = {c} (N^2 C flop): {tri:.2f} ms, {tf:.1f} TF/s, {100 * tf * 1e12 / PEAK:.1f} % of peak"]
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(table)), exist_ok=True)
    open(table, "w").write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paths_timing.txt"))
