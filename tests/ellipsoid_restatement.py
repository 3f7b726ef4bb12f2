"""An independent NumPy / torch-fp64 restatement of the reference's ellipsoid classifier (BOBE/clf.py:221-285, 375-472),
the yardstick of tests/test_clf_ellipsoid_cpu.py and tests/test_gpu_clf_ellipsoid.py.  It imports nothing from bobe_amd.

  L       = tril(flat_L) with softplus(.) + 1e-4 on the diagonal (jnp.tril_indices order)
  logit   = -alpha * einsum("...i,ij,...j->...", diff, L @ L.T, diff) + beta,   diff = x - mu
  loss    = optax.sigmoid_binary_cross_entropy(logit, y).mean()
  optimiser: optax.adamw(lr, weight_decay=wd) == torch.optim.AdamW(betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
  batches: np.random.RandomState(seed).permutation(N) per epoch, batch i = perm[i B:(i + 1) B], tail dropped
  restarts: seeds rng.integers(0, 2**32 - 1) in order; restart 0 from init_params, the others from
            flat_L ~ default_rng(seed).normal(0, init_scale), alpha = 1, beta = 0; best = smallest "%.2e" loss, strict <
"""
import numpy as np
import torch

B1, B2, EPS = 0.9, 0.999, 1e-8


def unpack_L(flat_L, d):
    flat_L = torch.as_tensor(flat_L, dtype=torch.float64)
    rows, cols = np.tril_indices(d)
    vals = torch.where(torch.as_tensor(rows == cols), torch.nn.functional.softplus(flat_L) + 1e-4, flat_L)
    L = torch.zeros((d, d), dtype=torch.float64)
    L[rows, cols] = vals
    return L


def logits(flat_L, alpha, beta, mu, x):
    """The reference's forward pass (clf.py:404-411): the L L^T einsum form."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    mu = torch.as_tensor(np.asarray(mu), dtype=torch.float64)
    d = x.shape[-1]
    L = unpack_L(flat_L, d)
    diff = x - mu
    md2 = torch.einsum("...i,ij,...j->...", diff, L @ L.T, diff)
    return -torch.as_tensor(alpha, dtype=torch.float64) * md2 + torch.as_tensor(beta, dtype=torch.float64), md2


def bce(logit, y):
    """optax.sigmoid_binary_cross_entropy(logit, y).mean()."""
    y = torch.as_tensor(np.asarray(y), dtype=torch.float64)
    return torch.nn.functional.binary_cross_entropy_with_logits(logit, y)


def proba(flat_L, alpha, beta, mu, x):
    return torch.sigmoid(logits(flat_L, alpha, beta, mu, x)[0]).numpy()


def analytic_grad(flat_L, alpha, beta, mu, x, y):
    """d loss / d (flat_L, alpha, beta) by hand: g_b = (sigmoid(logit) - y) / B; dlogit/dalpha = -md2, dlogit/dbeta = 1,
    dlogit/dL[i][j] = -2 alpha diff_i (L^T diff)_j (lower triangle), times sigmoid(flat) on the diagonal."""
    x, mu, y = np.asarray(x, np.float64), np.asarray(mu, np.float64), np.asarray(y, np.float64)
    d = x.shape[1]
    flat_L = np.asarray(flat_L, np.float64)
    L = unpack_L(flat_L, d).numpy()
    diff = x - mu
    u = diff @ L
    md2 = np.sum(u * u, axis=1)
    logit = -alpha * md2 + beta
    g = (1.0 / (1.0 + np.exp(-logit)) - y) / len(y)
    GL = -2.0 * alpha * (diff * g[:, None]).T @ u
    rows, cols = np.tril_indices(d)
    gf = GL[rows, cols]
    diag = rows == cols
    gf[diag] *= 1.0 / (1.0 + np.exp(-flat_L[diag]))
    return gf, float(np.sum(g * -md2)), float(np.sum(g))


def init_params(seed, d, init_scale=0.1):
    return {"flat_L": np.random.default_rng(int(seed)).normal(0.0, init_scale, size=d * (d + 1) // 2), "alpha": 1.0,
            "beta": 0.0}


def train_one(x, y, mu, start, seed, n_epochs=1000, batch_size=64, lr=1e-2, wd=1e-4):
    """One training run (clf.py:415-466) from ``start`` = {'flat_L', 'alpha', 'beta'}: (params, full-data loss)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[0]
    fl = torch.tensor(np.asarray(start["flat_L"], np.float64), requires_grad=True)
    al = torch.tensor(float(start["alpha"]), dtype=torch.float64, requires_grad=True)
    be = torch.tensor(float(start["beta"]), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([fl, al, be], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd)
    steps = max(1, n // batch_size)
    rs = np.random.RandomState(int(seed))
    for _ in range(n_epochs):
        perm = rs.permutation(n)
        for i in range(steps):
            idx = perm[i * batch_size:(i + 1) * batch_size]
            opt.zero_grad()
            loss = bce(logits(fl, al, be, mu, x[idx])[0], y[idx])
            loss.backward()
            opt.step()
    with torch.no_grad():
        full = float(bce(logits(fl, al, be, mu, x)[0], y))
    return {"flat_L": fl.detach().numpy().copy(), "alpha": al.item(), "beta": be.item()}, full


def train_restarts(x, y, mu, rng, n_restarts=2, init=None, n_epochs=1000, batch_size=64, lr=1e-2, wd=1e-4,
                   init_scale=0.1):
    """clf.py:221-285 with ``rng`` the global generator: (per-restart [(params, loss)], chosen index, seeds)."""
    d = np.asarray(x).shape[1]
    seeds = [rng.integers(0, 2 ** 32 - 1) for _ in range(n_restarts)]
    runs = []
    for i, s in enumerate(seeds):
        start = init if (i == 0 and init is not None) else init_params(s, d, init_scale)
        runs.append(train_one(x, y, mu, start, s, n_epochs, batch_size, lr, wd))
    best, best_loss = None, np.inf
    for i, (_, loss) in enumerate(runs):
        if float(f"{loss:.2e}") < best_loss:
            best, best_loss = i, float(f"{loss:.2e}")
    return runs, best, seeds
