"""An independent NumPy restatement of one No-U-Turn transition of ``k_nuts_run`` (consumer_kernels.hpp): the kernel's
counter-hash draws recomputed in uint64, the leapfrog with a dense inverse metric, multinomial NUTS with the generalised
U-turn criterion as NumPyro's ``iterative_build_tree`` builds it.  The target is any ``logp_and_grad(u) -> (logp, grad,
mean, x)`` on the logit scale; ``gp_target`` makes the one ``sample_GP_NUTS`` samples (``predict_grad`` as
``samplers.logp_and_grad`` uses it, gated GPs included)."""
import math

import numpy as np
from scipy.special import expit

M64 = (1 << 64) - 1


def mix64(z: int) -> int:
    """hmc_mix64: the splitmix64 finaliser."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u01(bits: int) -> float:
    return ((bits >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def iter_key(seed: int, chain: int, iteration: int) -> int:
    ckey = mix64(seed ^ mix64(chain))
    return (ckey + (iteration << 14)) & M64


def draw(ikey: int, index: int) -> int:
    return mix64((ikey + index) & M64)


def momentum_normals(ikey: int, d: int) -> np.ndarray:
    a = np.array([u01(draw(ikey, 2 * t)) for t in range(d)])
    b = np.array([u01(draw(ikey, 2 * t + 1)) for t in range(d)])
    return np.sqrt(-2.0 * np.log(a)) * np.cos(6.283185307179586 * b)


def direction_right(ikey: int, j: int) -> bool:
    return (draw(ikey, 64 + j) >> 63) == 1


def select_uniform(ikey: int, j: int, k: int) -> float:
    """k = 0: the merge uniform of doubling j; k >= 1: the selection uniform of leaf k of subtree j."""
    return u01(draw(ikey, 128 + 1024 * j + k))


def gp_target(gp, temp: float = 1.0):
    def logp_and_grad(u):
        X = np.clip(expit(np.atleast_2d(u)), 1e-12, 1.0 - 1e-12)
        m, _, dm, _ = gp.predict_grad(X, mean_only=True)
        mean = m * gp.y_std + gp.y_mean
        gx = dm * gp.y_std
        if hasattr(gp, "use_clf"):
            bad = m <= gp.minus_inf
            mean = np.where(bad, gp.minus_inf, mean)
            gx = np.where(bad[:, None], 0.0, gx)
        lp = mean / temp + np.sum(np.log(X) + np.log1p(-X), axis=1)
        g = gx / temp * (X * (1.0 - X)) + (1.0 - 2.0 * X)
        return float(lp[0]), g[0], float(mean[0]), X[0]
    return logp_and_grad


def _logaddexp(a, b):
    hi, lo = (a, b) if a > b else (b, a)
    if hi == -math.inf:
        return hi
    return hi + math.log1p(math.exp(lo - hi))


def _turning(sigma, p_left, p_right, rho):
    r = rho - 0.5 * (p_left + p_right)
    return float((sigma @ p_left) @ r) <= 0.0 or float((sigma @ p_right) @ r) <= 0.0


def transition(logp_and_grad, u0, g0, lp0, mean0, x0, sigma, eps, max_tree_depth, seed, chain, iteration):
    """One transition from (u0, g0, lp0, mean0, x0).  Returns a dict: depth, n_leapfrog, diverging, accept_prob, p0 and
    the next state (u, g, x, logp, mean)."""
    d = len(u0)
    sigma = np.asarray(sigma, dtype=np.float64)
    C = np.linalg.cholesky(np.linalg.inv(sigma))
    ikey = iter_key(seed, chain, iteration)
    p0 = C @ momentum_normals(ikey, d)
    H0 = -lp0 + 0.5 * float(p0 @ sigma @ p0)
    left = right = (np.array(u0, dtype=np.float64), p0, np.array(g0, dtype=np.float64))
    rho = p0.copy()
    prop = (np.array(u0), np.array(g0), np.array(x0), lp0, mean0)
    W, sum_acc, n_leap, depth, diverging = 0.0, 0.0, 0, 0, False
    for j in range(max_tree_depth):
        go_right = direction_right(ikey, j)
        e = eps if go_right else -eps
        u, p, g = right if go_right else left
        Ws, rs, sub, sub_turning = -math.inf, np.zeros(d), None, False
        ck_p, ck_r = {}, {}
        for k in range(1 << j):
            ph = p + 0.5 * e * g
            u = u + e * (sigma @ ph)
            lp, g, mean, x = logp_and_grad(u)
            p = ph + 0.5 * e * g
            dH = (0.5 * float(p @ sigma @ p) - lp) - H0
            if math.isnan(dH):
                dH = math.inf
            w = -dH
            dvg = not math.isfinite(dH) or dH > 1000.0
            sum_acc += 1.0 if dH <= 0.0 else math.exp(-dH)
            n_leap += 1
            if k == 0:
                take, Ws = True, w
            else:
                Wn = _logaddexp(Ws, w)
                with np.errstate(invalid="ignore"):
                    take = select_uniform(ikey, j, k) < math.exp(w - Wn) if math.isfinite(w - Wn) else False
                Ws = Wn
            if take:
                sub = (u.copy(), g.copy(), x.copy(), lp, mean)
            rs = rs + p
            imax = bin(k >> 1).count("1")
            if k % 2 == 0:
                ck_p[imax], ck_r[imax] = p.copy(), rs.copy()
            else:
                ntrail = 0
                while (k >> ntrail) & 1:
                    ntrail += 1
                for i in range(imax, imax - ntrail, -1):
                    r = rs - ck_r[i] + ck_p[i] - 0.5 * (ck_p[i] + p)
                    if float((sigma @ ck_p[i]) @ r) <= 0.0 or float((sigma @ p) @ r) <= 0.0:
                        sub_turning = True
                        break
            diverging = dvg
            if dvg or sub_turning:
                break
        usable = not sub_turning and not diverging
        pr = (1.0 if Ws >= W else math.exp(Ws - W)) if usable else 0.0
        if select_uniform(ikey, j, 0) < pr:
            prop = sub
        W = _logaddexp(W, Ws)
        rho = rho + rs
        if go_right:
            right = (u, p, g)
        else:
            left = (u, p, g)
        depth = j + 1
        if sub_turning or _turning(sigma, left[1], right[1], rho) or diverging:
            break
    u1, g1, x1, lp1, mean1 = prop
    return {"depth": depth, "n_leapfrog": n_leap, "diverging": diverging, "accept_prob": sum_acc / n_leap, "p0": p0,
            "u": u1, "g": g1, "x": x1, "logp": lp1, "mean": mean1}


def dual_averaging(adapt, accept_prob):
    """The per-chain step-size update k_hmc_run / k_nuts_run apply while adapting: adapt = [eps, mu, hbar, leb, m]."""
    t0, gamma, kappa, target = 10.0, 0.05, 0.75, 0.8
    eps, mu, hbar, leb, m = adapt
    m = m + 1.0
    hbar = (1.0 - 1.0 / (m + t0)) * hbar + (target - accept_prob) / (m + t0)
    le = mu - math.sqrt(m) / gamma * hbar
    eta = m ** (-kappa)
    leb = eta * le + (1.0 - eta) * leb
    return np.array([min(max(math.exp(le), 1e-4), 2.0), mu, hbar, leb, m])
