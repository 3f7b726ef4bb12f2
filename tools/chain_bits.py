"""Snapshot / compare the bits of the four chain kernels (k_hmc_run, k_nuts_run, k_rwalk, k_paths_hmc_run) at the smallest
sizes at which each home of a chain workgroup's training rows is in use - registers only, registers + LDS, a streamed rest
as well - for every dimension cap and both kernel families.  For changes to the code these kernels share
(chain_common.hpp), which must not move a bit.
   python tools/chain_bits.py save|check FILE        (`print` writes the digests as one JSON line to stdout)

The cases, (d, N), and where the rows live (256 x ChainRows rows per workgroup in registers, then chain_lds_groups groups of
256 in LDS, the rest streamed):
   d (cap)   N      hmc_run / paths_hmc_run       nuts_run                  rwalk
   3 (8)     200    registers                     registers                 registers
   12 (16)   200    registers                     registers                 registers
   12 (16)   2500   1536 reg + 964 LDS            768 + 1280 + 452 streamed 2048 reg + 452 LDS
   12 (16)   3000   1536 + 1280 + 184 streamed    768 + 1280 + 952 streamed 2048 reg + 952 LDS
   20 (32)   200    registers                     registers                 registers
   20 (32)   700    512 reg + 188 LDS (paths: 256 + 444)   256 + 444 LDS    registers (1024)
   20 (32)   1500   512 + 768 + 220 streamed (paths: 256 + 768 + 476)   256 + 768 + 476 streamed   1024 reg + 476 LDS
k_rwalk keeps the most rows in registers, so none of these sizes reaches its streamed rest: two more sizes, (12, 3500) and
(20, 2000), run the walk alone (2048 + 1280 + 172 streamed, 1024 + 768 + 208 streamed).  The paths kernel's layout is read
from the library (PosteriorPaths.chain_layout) and printed.

Per case, P = 12 chains: hmc_run, 6 iterations with adaptation and hist / keep (thin 2) / dbg, ungated and under an
ellipsoid gate; nuts_run, 3 transitions with stats; rwalk, 30 walks; paths_hmc_run on S = 3 paths of F = 300 features (a
ragged last feature group), chains cycling over the paths, every chain its own inv_mass row."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bobe_amd import clf  # noqa: E402
from bobe_amd.gp import GP  # noqa: E402

P, S, F = 12, 3, 300
CASES = [(3, 200), (12, 200), (12, 2500), (12, 3000), (20, 200), (20, 700), (20, 1500)]
WALK_ONLY = [(12, 3500), (20, 2000)]
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


def surface(kern, d, n):
    rng = np.random.default_rng(1000 * d + n)
    X = rng.uniform(size=(n, d))
    y = -15.0 * np.sum((X - 0.5) ** 2, axis=1)
    return GP(X, y, noise=1e-6, kernel=kern, lengthscales=np.linspace(0.4, 0.9, d), kernel_variance=2.0), rng


def walk(gp, rng, d, tag):
    x0 = rng.uniform(0.05, 0.95, size=(P, d))
    step = 0.03 * (np.eye(d) + np.tril(np.full((d, d), 0.1), -1))
    logl = gp.predict_mean_batched(x0)
    res = gp.rwalk(x0, logl, step, float(np.min(logl)) - 0.5, 30, 79, debug=True)
    out[f"rwalk_{tag}"] = cat(*res)
    return int(res[2].sum()), int(res[3].sum())


for kern in ("rbf", "matern"):
    for d, n in CASES:
        tag = f"{kern}_d{d}_N{n}"
        gp, rng = surface(kern, d, n)
        U = rng.normal(scale=0.5, size=(P, d))
        st0 = chain_state(gp, U)
        im = rng.uniform(0.5, 2.0, size=d)
        st, ad = st0.copy(), adapt(0.05)
        hist, keep, dbg = gp.hmc_run(st, ad, im, 77, 3, 6, True, hist_from=0, thin=2, debug=True)
        out[f"hmc_{tag}"] = cat(st, ad, hist, keep, dbg)
        moved = int(np.sum(np.any(st != st0, axis=1)))
        # the ellipsoid gate: beta puts the boundary through the cloud of start points (two of twelve start outside)
        X0 = st0[:, 2 * d:3 * d]
        ell = {"params": {"flat_L": 0.1 * rng.normal(size=d * (d + 1) // 2), "alpha": 1.0, "beta": 0.0}, "mu": np.full(d, 0.5)}
        clf.install_ellipsoid_gate(gp._lib, gp._h, ell, None, 0.5, -1e5)
        md2 = -clf.gate_eval(gp._lib, gp._h, X0, d)[0]
        ell["params"]["beta"] = float(np.sort(md2)[-3] + np.sort(md2)[-2]) / 2
        clf.install_ellipsoid_gate(gp._lib, gp._h, ell, None, 0.5, -1e5)
        st, ad = st0.copy(), adapt(0.05)
        hist, keep, dbg = gp.hmc_run(st, ad, im, 77, 3, 6, True, hist_from=0, thin=2, debug=True)
        out[f"hmc_gated_{tag}"] = cat(st, ad, hist, keep, dbg)
        clf.install_gate(gp._lib, gp._h, None, 0.5, -1e5)
        st, ad = st0.copy(), adapt(0.05)
        res = gp.nuts_run(st, ad, np.diag(im) + 0.1, 5, 78, 2, 3, True, hist_from=0, thin=1, stats=True, debug=True)
        out[f"nuts_{tag}"] = cat(st, ad, *res)
        nacc, nin = walk(gp, rng, d, tag)
        with gp.sample_paths(S, F, seed=5 + d) as ps:
            lay = ps.chain_layout()
            idx = (np.arange(P) % S).astype(np.int64)
            imp = rng.uniform(0.5, 2.0, size=(P, d))
            st, ad = ps.hmc_state(U, idx), adapt(0.05)
            hist, keep, dbg = ps.hmc_run(st, ad, imp, idx, 81, 3, 6, True, hist_from=0, thin=2, debug=True)
            out[f"paths_{tag}"] = cat(st, ad, hist, keep, dbg)
        print(f"{tag}: hmc moved {moved}/{P} chains, nuts leapfrogs {int(res[2][:, :, 1].sum())}, rwalk accepted {nacc} of "
              f"{nin} inside, paths rows {lay['registers']} reg + {lay['lds']} LDS + {lay['streamed']} streamed")
    for d, n in WALK_ONLY:
        gp, rng = surface(kern, d, n)
        nacc, nin = walk(gp, rng, d, f"{kern}_d{d}_N{n}")
        print(f"{kern}_d{d}_N{n}: rwalk accepted {nacc} of {nin} inside")

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
