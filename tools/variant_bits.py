"""Snapshot / compare the bits of every entry point whose kernel is picked per (kernel family, dimension cap): both
families at the two sides of each cap boundary and at the maximum (d = 8, 9, 16, 17, 32), N = 150.  bits_snapshot.py stays
at d <= 8; this tool is for changes to the host's variant dispatch, which must not move a bit.
   python tools/variant_bits.py save|check FILE        (`print` writes the digests as one JSON line to stdout)"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bobe_amd import clf  # noqa: E402
from bobe_amd.gp import GP, dist_sq  # noqa: E402

N, P, ITERS = 150, 8, 3
out = {}


def cat(*arrays):
    return np.concatenate([np.ravel(np.asarray(a, dtype=np.float64)) for a in arrays if a is not None])


def chain_state(gp, U, temp=1.0):
    """(P, 3d+2) rows [u, dlogp/du, x, logp, mean] of the chain kernels, from the mean-only posterior gradient"""
    X = 1.0 / (1.0 + np.exp(-U))
    m, _, dm, _ = gp.predict_grad(X, mean_only=True)
    mean = m * gp.y_std + gp.y_mean
    logp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
    grad = dm * gp.y_std / temp * (X * (1 - X)) + (1 - 2 * X)
    return np.ascontiguousarray(np.hstack([U, grad, X, logp[:, None], mean[:, None]]))


def adapt(eps):
    return np.tile(np.array([eps, np.log(10 * eps), 0.0, 0.0, 0.0]), (P, 1))


def solve_entries(gp, tag, cand, Z, few, q):
    """the entries that go through solve_v (and the few-candidate chains): sweep, wip_grad on both paths and its two siblings,
    predict_grad"""
    gp._lib.bobe_gp_set_chunk(gp._h, 128)
    r = gp.wip_sweep(cand, Z, want_mean_var=True)                # 300 candidates at chunk 128: three chunks, k_wip_score
    out[f"sweep_{tag}"] = cat(r["wipv"], r["wipstd"], r["mean"], r["var"], [r["argmin_v"], r["argmin_s"], r["min_v"], r["min_s"]])
    rz = gp.wip_sweep(Z, Z)                                      # candidates = integration points
    out[f"sweepz_{tag}"] = cat(rz["wipv"], rz["wipstd"], [rz["argmin_v"], rz["argmin_s"]])
    gp._lib.bobe_gp_set_chunk(gp._h, 0)
    out[f"wgfew_{tag}"] = cat(*gp.wip_grad(few, Z))              # 3 candidates: the matrix-vector path
    lw = 1.5 * np.random.default_rng(Z.shape[0]).normal(size=Z.shape[0])   # its two siblings, log-weights given
    rw = gp.wip_grad_w(few, Z, log_weights=lw)
    out[f"wgw_{tag}"] = cat(*[rw[k] for k in gp.CRITERIA], *[rw["d" + k] for k in gp.CRITERIA])
    rv = gp.wip_grad_zvar(few, Z, log_weights=lw)
    out[f"wgzv_{tag}"] = cat(rv["zvar"], rv["dzvar"], [rv["log_ez"]])
    out[f"wgtile_{tag}"] = cat(*gp.wip_grad(cand[:40], Z))       # 40: the tile path
    out[f"pg_{tag}"] = cat(*gp.predict_grad(q))
    out[f"pgm_{tag}"] = cat(*gp.predict_grad(q, mean_only=True))


for kern in ("rbf", "matern"):
    for d in (8, 9, 16, 17, 32):
        tag = f"{kern}_{d}"
        rng = np.random.default_rng(N)
        X = rng.uniform(size=(N, d))
        y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=N)
        ls = np.full(d, 0.5) * np.sqrt(d / 4.0)                  # (keeps the correlations of the d = 4 scale at every d)
        gp = GP(X, y, noise=1e-5, kernel=kern, lengthscales=ls)
        out[f"L_{tag}"] = np.array(gp.cholesky)
        out[f"mll_{tag}"] = cat(*gp.mll_data(0.9 * ls, 1.3))
        out[f"loo_{tag}"] = cat(*gp.loo_data(0.9 * ls, 1.3))
        A, B = rng.uniform(size=(37, d)), rng.uniform(size=(130, d))
        out[f"kern_{tag}"] = gp.kernel(A, B, include_noise=False)
        out[f"dist_{tag}"] = dist_sq(A, B)
        q = rng.uniform(size=(50, d))
        out[f"pred_{tag}"] = cat(*gp.predict_batched(q))
        cand, Z, few = rng.uniform(size=(300, d)), rng.uniform(size=(40, d)), rng.uniform(0.1, 0.9, size=(3, d))
        solve_entries(gp, tag, cand, Z, few, q[:9])
        out[f"fant_{tag}"] = gp.fantasy_var(cand[:5], Z)
        sb = gp.wip_select_batch(cand, Z, 3, return_stage_scores=True)
        out[f"batch_{tag}"] = cat(sb["indices"], sb["scores"], sb["stage_scores"])
        out[f"ei_{tag}"] = cat(gp.acq_ei(q, float(np.max(gp.train_y)), 0.01), gp.acq_ei(q, float(np.max(gp.train_y)), 0.01, log_ei=True))
        # the chain kernels: counter-based random numbers, fixed seeds
        U = rng.normal(scale=0.5, size=(P, d))
        st0 = chain_state(gp, U)
        p0 = rng.normal(size=(P, d))
        out[f"leap_{tag}"] = cat(*gp.hmc_leapfrog(U, p0 + 0.05 * st0[:, d:2 * d], np.ones(d), 0.1, 4))
        st, ad = st0.copy(), adapt(0.1)
        hist, keep, dbg = gp.hmc_run(st, ad, np.ones(d), 77, 0, ITERS, True, hist_from=0, thin=1, debug=True)
        out[f"hmc_{tag}"] = cat(st, ad, hist, keep, dbg)
        st, ad = st0.copy(), adapt(0.1)
        res = gp.nuts_run(st, ad, np.eye(d) + 0.1, 5, 78, 0, ITERS, True, hist_from=0, thin=1, stats=True, debug=True)
        out[f"nuts_{tag}"] = cat(st, ad, *res)
        x0 = rng.uniform(0.05, 0.95, size=(P, d))
        out[f"rwalk_{tag}"] = cat(*gp.rwalk(x0, gp.predict_mean_batched(x0), 0.05 * np.eye(d), -1e30, 6, 79, debug=True))
        # the classifier gate: an SVM of 5 support vectors
        sv = rng.uniform(size=(5, d))
        params = {"support_vectors": sv, "dual_coef": np.array([1.0, -0.8, 0.6, -0.5, 0.7]), "intercept": -0.05,
                  "gamma_eff": 1.0 / d}
        clf.install_gate(gp._lib, gp._h, params, 0.5, -1e5)
        out[f"gate_{tag}"] = cat(*clf.gate_eval(gp._lib, gp._h, q, d), clf.gate_proba(gp._lib, gp._h, q, d),
                                 *gp.predict_batched(q))
        clf.install_gate(gp._lib, gp._h, None, 0.5, -1e5)
        # the substitution path (refine_kappa = 0: always), one pass over the entries that call solve_v
        gp.refine_kappa = 0.0
        gp.recompute_cholesky()
        solve_entries(gp, "sub_" + tag, cand, Z, few, q[:9])

out = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in out.items()}
if sys.argv[1] == "print":
    print(json.dumps(out))
elif sys.argv[1] == "save":
    json.dump(out, open(sys.argv[2], "w"), indent=0)
    print("saved", len(out), "digests")
else:
    ref = json.load(open(sys.argv[2]))
    bad = [k for k in out if k not in ref or out[k] != ref[k]]
    print("not in the reference:", [k for k in out if k not in ref])
    print("BITS DIFFER in:" if bad else f"all {len(out)} digests identical", bad)
    sys.exit(1 if bad else 0)
