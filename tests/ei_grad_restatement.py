"""EI / LogEI with their input gradients (``bobe_gp_acq_ei_grad``), stated twice from a posterior ``(m, v, dm, dv, floored)``
in standardised units; shared by tests/test_ei_grad_cpu.py and tests/test_gpu_ei_grad.py.  Imports nothing from bobe_amd.

  value_and_grad_f64   NumPy / SciPy (``ndtr``, ``erfcx``) in fp64, statement for statement what k_ei_grad computes - the
                       branches of the reference's ``_log_ei_helper`` and the two-branch LogEI gradient included: the
                       restatement whose own error sets the scale of the rule
  value_and_grad_truth the same quantities from their definitions at 50 digits (``mpmath``: ``ncdf`` / ``npdf``), from
                       long-double inputs: the truth

With lo = 1e-18 (LogEI) / 1e-20 (EI):

    sigma = sqrt(max(v, lo)),  dsigma = dv / (2 sigma), and 0 where v < lo or the posterior sits on its 1e-12 floor
    u = (m - zeta - best_y) / sigma,  h(u) = phi(u) + u Phi(u)
    EI:     val = sigma h          grad = Phi dm + phi dsigma
    LogEI:  val = log h + log sigma,  grad = A dm + B dsigma,  A = Phi / (sigma h),  B = phi / (sigma h)
            fp64, u <= -1:  R = Phi / phi = sqrt(pi / 2) erfcx(-u / sqrt 2),  g = h / phi = 1 - |u| R - from |u| = 30 on by
                            its series 1/u^2 - 3/u^4 + 15/u^6 - ... (nine terms) -,  B = 1 / (sigma g),  A = R B
"""
import numpy as np

LOG_2PI = 1.83787706640934548356
HALF_LOG_HALF_PI = 0.22579135264472743236          # log sqrt(pi / 2)
SQRT_HALF_PI = 1.25331413731550025121
INV_SQRT2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


def clip_floor(log_ei):
    return 1e-18 if log_ei else 1e-20


# ------------------------------------------------------------------------------------------------------- the fp64 restatement
def _pdf(u):
    return np.exp(-0.5 * u * u) * INV_SQRT_2PI


def _ei_helper(u):
    from scipy.special import ndtr
    return _pdf(u) + u * ndtr(u)


def _log1mexp(x):
    x = np.abs(x)
    with np.errstate(all="ignore"):
        return np.where(x < 0.69314718055994530942, np.log(-np.expm1(-x)), np.log1p(-np.exp(-x)))


def log_ei_helper(u):
    """the reference's ``_log_ei_helper`` (BOBE/acquisition.py:21-75), its branches as the device has them: the direct form
    above u = -1, the erfcx form down to -1e6, the asymptotic one below"""
    from scipy.special import erfcx
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        direct = np.log(_ei_helper(u))
        u_eps = np.maximum(u, -1e6)
        w = np.log(np.abs(u_eps) * erfcx(-INV_SQRT2 * u_eps)) + HALF_LOG_HALF_PI
        log_phi = -0.5 * (u * u + LOG_2PI)
        second = np.where(u > -1e6, _log1mexp(w), -2.0 * np.log(np.abs(u)))
        return np.where(u > -1.0, direct, log_phi + second)


def value_and_grad_f64(m, v, dm, dv, floored, best_y, zeta, log_ei, *, variant=None, dv_unfloored=None):
    """(val [C], grad [C x d], u [C]) in fp64.  ``variant`` states a mistake on purpose, for tests/test_ei_grad_cpu.py:
    'dsigma_twice' - dsigma = dv / sigma; 'floor_leak' - the floored rows get the dsigma of ``dv_unfloored``."""
    from scipy.special import erfcx, ndtr
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    dm, dv = np.asarray(dm, dtype=np.float64), np.asarray(dv, dtype=np.float64)
    floored = np.asarray(floored, dtype=bool)
    lo = clip_floor(log_ei)
    clipped = v < lo
    v = np.maximum(v, lo)
    sigma = np.sqrt(v)
    dsig = dv / ((1.0 if variant == "dsigma_twice" else 2.0) * sigma)[:, None]
    dsig = np.where((clipped | floored)[:, None], 0.0, dsig)
    if variant == "floor_leak":
        dsig = np.where(floored[:, None], np.asarray(dv_unfloored, dtype=np.float64) / (2.0 * sigma)[:, None], dsig)
    u = (m - zeta - best_y) / sigma
    with np.errstate(all="ignore"):
        if not log_ei:
            val = _ei_helper(u) * sigma
            a, b = ndtr(u), _pdf(u)
        else:
            leh = log_ei_helper(u)
            val = leh + np.log(sigma)
            sh = sigma * _ei_helper(u)
            x = np.maximum(-u, 1.0)                                     # (the lower branch's argument; idle above u = -1)
            r = SQRT_HALF_PI * erfcx(INV_SQRT2 * x)
            t = 1.0 / (x * x)
            series = t * (1.0 - t * (3.0 - t * (15.0 - t * (105.0 - t * (945.0 - t * (10395.0 - t * (
                135135.0 - t * (2027025.0 - t * 34459425.0))))))))
            g = np.where(x < 30.0, 1.0 - x * r, series)
            b_low = 1.0 / (sigma * g)
            a_low = r * b_low
            a = np.where(u > -1.0, ndtr(u) / sh, a_low)
            b = np.where(u > -1.0, _pdf(u) / sh, b_low)
    return val, a[:, None] * dm + b[:, None] * dsig, u


# ------------------------------------------------------------------------------------------------------------------ the truth
DIGITS = 50


def _mpf(x):
    """a long double (or a double) as an mpf, exactly: its leading 53 bits and the rest"""
    import mpmath as mp
    x = np.longdouble(x)
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


def _to_ld(x):
    """an mpf as a long double, rounded twice at most: leading double and the remainder"""
    import mpmath as mp
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - mp.mpf(hi)))


def truth_value(m, v, best_y, zeta, log_ei):
    """the value alone at mpf arguments, from the definitions (what ``truth_self_check`` differentiates)"""
    import mpmath as mp
    lo = mp.mpf(clip_floor(log_ei))
    sigma = mp.sqrt(v if v > lo else lo)
    u = (m - zeta - best_y) / sigma
    h = mp.npdf(u) + u * mp.ncdf(u)
    return mp.log(h) + mp.log(sigma) if log_ei else sigma * h


def truth_coefficients(m, v, best_y, zeta, log_ei):
    """(val, A, B, u) at mpf arguments: grad = A dm + B dsigma in closed form"""
    import mpmath as mp
    lo = mp.mpf(clip_floor(log_ei))
    sigma = mp.sqrt(v if v > lo else lo)
    u = (m - zeta - best_y) / sigma
    Phi, phi = mp.ncdf(u), mp.npdf(u)
    h = phi + u * Phi
    if log_ei:
        return mp.log(h) + mp.log(sigma), Phi / (sigma * h), phi / (sigma * h), u
    return sigma * h, Phi, phi, u


def value_and_grad_truth(m, v, dm, dv, floored, best_y, zeta, log_ei):
    """(val [C], grad [C x d], u [C]) as long doubles, computed at 50 digits from the long-double posterior"""
    import mpmath as mp
    C, d = np.shape(dm)
    val, grad, us = np.zeros(C, np.longdouble), np.zeros((C, d), np.longdouble), np.zeros(C, np.longdouble)
    with mp.workdps(DIGITS):
        by, zt = _mpf(best_y), _mpf(zeta)
        lo = mp.mpf(clip_floor(log_ei))
        for c in range(C):
            mc, vc = _mpf(m[c]), _mpf(v[c])
            f, A, B, u = truth_coefficients(mc, vc, by, zt, log_ei)
            val[c], us[c] = _to_ld(f), _to_ld(u)
            sigma = mp.sqrt(vc if vc > lo else lo)
            still = bool(floored[c]) or vc < lo
            for j in range(d):
                dsig = mp.mpf(0) if still else _mpf(dv[c, j]) / (2 * sigma)
                grad[c, j] = _to_ld(A * _mpf(dm[c, j]) + B * dsig)
    return val, grad, us


def truth_self_check(m, v, best_y, zeta, log_ei):
    """digits (base 10) to which the truth's closed-form coefficients agree with ``mpmath.diff`` of its own value in (m, v):
    d val / dm = A and d val / dv = B / (2 sigma), taken together as one gradient.  (m, v) must not sit on the clip."""
    import mpmath as mp
    with mp.workdps(DIGITS):
        mc, vc, by, zt = _mpf(m), _mpf(v), _mpf(best_y), _mpf(zeta)
        _, A, B, _ = truth_coefficients(mc, vc, by, zt, log_ei)
        sigma = mp.sqrt(vc)
        nm = mp.diff(lambda a, b: truth_value(a, b, by, zt, log_ei), (mc, vc), (1, 0))
        nv = mp.diff(lambda a, b: truth_value(a, b, by, zt, log_ei), (mc, vc), (0, 1))
        # as one gradient in the scaled coordinates (m / sigma, log v), relative to its larger component: far out on the
        # right phi(u) is 10^-200000 of Phi(u), and no derivative of the sum can show such a component to 30 digits of its own
        closed = (A * sigma, B / (2 * sigma) * vc)
        numeric = (nm * sigma, nv * vc)
        scale = max(abs(closed[0]), abs(closed[1]))
        rel = max(abs(closed[0] - numeric[0]), abs(closed[1] - numeric[1])) / scale
        return float(DIGITS) if rel == 0 else float(-mp.log10(rel))
