"""Times of the ellipsoid classifier: one training run (train_ellipsoid_classifier, default settings: 2 restarts x 1000
epochs) split into the host's share (seed draws, initial parameters, RandomState permutation table) and the device call
(bobe_gp_train_ellipsoid: copies + one k_ellipsoid_train launch); the same loop stepped by torch on the GPU (the test
restatement, one restart, a few epochs, extrapolated); and the samplers' kernels without a gate, with the SVM gate (at the
n_sv the SVM reaches on the same labels) and with the ellipsoid gate.

    python tools/clf_train_timing.py [out.json]        (default profiles/clf_train_timing.json)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bobe_amd import clf  # noqa: E402
from bobe_amd.clf_gp import GPwithClassifier  # noqa: E402
from bobe_amd.utils import get_numpy_rng, set_global_seed  # noqa: E402


def problem(n, d, seed=0):
    rng = np.random.default_rng(seed)
    c = 0.5 + rng.uniform(-0.05, 0.05, d)
    S = (0.6 * np.ones((d, d)) + 0.4 * np.eye(d)) * 0.08 ** 2
    X = np.clip(np.vstack([rng.uniform(size=(n // 2, d)), rng.multivariate_normal(c, 4 * S, size=n - n // 2)]), 0, 1)
    z = X - c
    v = -0.5 * np.einsum("ni,ij,nj->n", z, np.linalg.inv(S), z)
    return X, v


def time_training(n, d, reps=3):
    X, v = problem(n, d)
    labels = (v > v.max() - 4.5).astype(np.float64)
    mu = X[np.argmax(v)]
    model = clf.EllipsoidClassifier(d=d, mu=mu)
    trainer = clf._DeviceEllipsoid(None, d, mu)
    handle = (trainer._lib, trainer._h)
    set_global_seed(0)
    host, dev, total = [], [], []
    for _ in range(reps + 1):                                   # (the first call warms the kernel up, not counted)
        t0 = time.perf_counter()
        rng = get_numpy_rng()
        seeds = [rng.integers(0, 2 ** 32 - 1) for _ in range(model.n_restarts)]
        inits = np.stack([clf._ell_theta(model.init(s), d) for s in seeds])
        perms = np.stack([clf.ellipsoid_permutations(s, n, model.n_epochs, model.batch_size) for s in seeds])
        t1 = time.perf_counter()
        clf._device_train(model, X, labels, inits, perms, handle=handle)
        t2 = time.perf_counter()
        set_global_seed(0)
        clf.train_ellipsoid_classifier(X, labels, None, best_pt=mu, handle=handle)
        t3 = time.perf_counter()
        host.append(t1 - t0)
        dev.append(t2 - t1)
        total.append(t3 - t2)
    return {"n": n, "d": d, "host_s": float(np.median(host[1:])), "device_s": float(np.median(dev[1:])),
            "train_ellipsoid_classifier_s": float(np.median(total[1:])), "steps_per_restart": model.n_epochs * max(1, n // 64)}


def time_torch_restatement(n, d, epochs=5):
    import torch
    import ellipsoid_restatement as R
    X, v = problem(n, d)
    labels = (v > v.max() - 4.5).astype(np.float64)
    mu = X[np.argmax(v)]
    dev = torch.device("cuda")
    x, y, m = (torch.tensor(a, dtype=torch.float64, device=dev) for a in (X, labels, mu))
    p = R.init_params(1, d)
    fl = torch.tensor(p["flat_L"], device=dev, requires_grad=True)
    al = torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
    be = torch.tensor(0.0, dtype=torch.float64, device=dev, requires_grad=True)
    opt = torch.optim.AdamW([fl, al, be], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    rows, cols = np.tril_indices(d)
    rows_t, cols_t = torch.tensor(rows, device=dev), torch.tensor(cols, device=dev)
    diag = torch.tensor(rows == cols, device=dev)

    def loss_of(idx):
        L = torch.zeros((d, d), dtype=torch.float64, device=dev)
        L = L.index_put((rows_t, cols_t), torch.where(diag, torch.nn.functional.softplus(fl) + 1e-4, fl))
        diff = x[idx] - m
        md2 = torch.einsum("...i,ij,...j->...", diff, L @ L.T, diff)
        return torch.nn.functional.binary_cross_entropy_with_logits(-al * md2 + be, y[idx])
    rs = np.random.RandomState(1)
    steps = max(1, n // 64)
    times = []
    for e in range(epochs + 1):
        perm = torch.tensor(rs.permutation(n), device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            opt.zero_grad()
            loss_of(perm[i * 64:(i + 1) * 64]).backward()
            opt.step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    per_epoch = float(np.median(times[1:]))
    return {"n": n, "d": d, "epochs_timed": epochs, "per_step_s": per_epoch / steps,
            "extrapolated_2x1000_epochs_s": 2 * 1000 * per_epoch}


def time_samplers(n_clf, d):
    """hmc_run / rwalk of one GP (the classifier set's points within gp_threshold) ungated, SVM-gated, ellipsoid-gated."""
    X, v = problem(n_clf, d, seed=1)
    out = {"n_clf": n_clf, "d": d}
    for kind in ("none", "svm", "ellipsoid"):
        g = GPwithClassifier(X, v, clf_type="svm" if kind == "none" else kind, clf_threshold=4.5, gp_threshold=30.0,
                             noise=1e-6, lengthscales=np.full(d, 0.2))
        if kind == "none":
            g.use_clf = False
        elif kind == "svm":
            out["n_sv"] = int(g.clf_metrics["n_support_vectors"])
        out["n_gp"] = int(g.npoints)
        P = 256
        rng = np.random.default_rng(3)
        x0 = g.train_x[np.argsort(-g.train_y.ravel())[:1]].repeat(P, axis=0) + 0.001 * rng.normal(size=(P, d))
        x0 = np.clip(x0, 0.01, 0.99)
        u0 = np.log(x0) - np.log1p(-x0)
        state = np.zeros((P, 3 * d + 2))
        state[:, :d] = u0
        state[:, 2 * d:3 * d] = x0
        state[:, 3 * d] = -1e30
        state[:, 3 * d + 1] = -1e30
        adapt = np.tile(np.array([0.05, 0.0, 0.0, 0.0, 0.0]), (P, 1))
        logl = g.predict_mean_batched(x0)
        step = 0.02 * np.eye(d)
        th, tw = [], []
        for rep in range(4):
            s, a = state.copy(), adapt.copy()
            t0 = time.perf_counter()
            g.hmc_run(s, a, np.ones(d), 11 + rep, 0, 50, False)
            t1 = time.perf_counter()
            g.rwalk(x0, logl, step, float(np.min(logl)) - 1e3, 50, 5 + rep)
            t2 = time.perf_counter()
            th.append(t1 - t0)
            tw.append(t2 - t1)
        out[kind] = {"hmc_run_256x50_s": float(np.median(th[1:])), "rwalk_256x50_s": float(np.median(tw[1:]))}
    return out


def main():
    import torch
    torch.zeros(1, device="cuda")                               # (torch's device first, then the library's)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clf_train_timing.json")
    res = {"training": [], "torch_restatement": [], "samplers": []}
    for n in (256, 1024, 4096):
        for d in (2, 8, 16):
            r = time_training(n, d)
            res["training"].append(r)
            print(json.dumps(r), flush=True)
    for n, d in ((1024, 8), (4096, 16)):
        r = time_torch_restatement(n, d)
        res["torch_restatement"].append(r)
        print(json.dumps(r), flush=True)
    for n, d in ((1024, 4), (1024, 8)):
        r = time_samplers(n, d)
        res["samplers"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
