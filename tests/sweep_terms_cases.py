"""The cases of the sweep-intermediate tests (tests/test_sweep_terms_cpu.py, tests/test_gpu_sweep_terms.py).  The designs are
tests/zvar_cases.py's (``SHAPES`` / ``case_data``); imports nothing from bobe_amd.

Layer A (tests/sweep_terms_restatement.py: each stage alone, on the judged side's own inputs) runs on every entry of ``CASES``
and on each of the three paths; Layer B (the zvar score end to end under zvar_cases.rule) on ``LAYER_B``, same paths.

  near_noise_2d      64 points in 2-D, posterior variances within two decades of the noise: one row tile, the design on which
                     the evidence-variance score first missed its rule (at the draw of seed 143; the draw of seed 138 held it)
  two_row_tiles      130 points: a second row tile with 2 live rows, the 64-tile Z side
  fused_ragged       chunks of 256 over 818 candidates: cross tiles riding in the next chunk's solve, the last chunk (one
                     column tile) narrower than the pending one (two), three diagonal blocks when substituting
  cross128           16384 + 128 candidates against 512 points in chunks of 16384: 128 x 4 cross tiles (at least twice the
                     compute units: the 128-tile cross kernel, alone when substituting, riding in the solve otherwise) and a
                     tail of one column tile on the 64-tile cross kernel
  second_superchunk  65536 + 200 candidates: the second super-chunk's addresses of crossT, s_c and the scaled candidates
  cand_is_z          the candidates ARE the integration points: s_c from V_Z's column sums, V_Z^T V_Z
  reference_noise_*  noise 1e-8: substitution by default, one (N = 130: two row tiles) and three (N = 300) diagonal blocks
"""
import functools

import numpy as np

import sweep_terms_restatement as S
import zvar_cases as ZC

PATHS = ("default", "substitution", "product")       # refine_kappa as set, 0 (always substitute), -1 (never)
KAPPA = {"default": None, "substitution": 0.0, "product": -1.0}

# name -> (zvar_cases shape, kernel)
CASES = {
    "near_noise_2d-rbf": ("near_noise_m63", "rbf"),
    "near_noise_2d-matern": ("near_noise_m63", "matern"),
    "near_noise_2d-seed143": ("near_noise_s143_m63", "rbf"),
    "two_row_tiles": ("tile_edge", "rbf"),
    "fused_ragged": ("fused_ragged", "matern"),
    "cross128": ("cross128", "rbf"),
    "second_superchunk": ("second_superchunk", "rbf"),
    "cand_is_z": ("cand_is_z", "matern"),
    "reference_noise_130": ("reference_noise_130", "rbf"),
    "reference_noise_300": ("reference_noise_300", "matern"),
}

# (zvar_cases sweep case) of Layer B: the near-noise design at M = 63, 64, 65 on the draw of seed 138 (in zvar_cases.SWEEP_CASES
# as well) and on the draws the M-edge cases once had there (seeds 143 .. 145, with those cases' kernels and scales), two row
# tiles, the candidates as integration points, the reference's noise
LAYER_B = [c for c in ZC.SWEEP_CASES if c[0].startswith("near_noise_m")] + [
    ("near_noise_s143_m63", "rbf", True, 30.0), ("near_noise_s144_m64", "matern", False, 1.0),
    ("near_noise_s145_m65", "rbf", True, 4e3),
    ("tile_edge", "rbf", True, 1.0), ("tile_edge", "matern", True, 30.0),
    ("cand_is_z", "rbf", True, 1.0), ("cand_is_z", "matern", False, 30.0),
    ("reference_noise_130", "rbf", True, 30.0), ("reference_noise_300", "matern", False, 1.0),
]

# Where the score misses its rule: case -> ((kvar + noise) / smallest pivot, {path: the device's worst |zvar - truth| /
# (1 + |truth|) on an MI355X}).  Strict expected failures of Layer B.  The stage is "V": the product with the explicit inverse
# factor, error eps |L^-1| |k| - on the product path the whole of Linv, on the substitution the 128-row diagonal block
# inv(L_tt), which for N <= 128 is the same arithmetic (the same figures) and for N = 130 nearly so.  All three factors sit
# above refine_kappa = 1e6, so the handle substitutes.  No kernel is at fault: every Layer A stage of these runs is at 0.02 ..
# 0.25 of its bound, the inverse factor at rho = 0.02 .. 0.04 beside SciPy's 0.01 .. 0.02, a backward-stable solve with the
# device's own factor scores 2.7e-8 / 7.0e-8 / 9.4e-8, and float64 NumPy's product with SciPy's inverse loses as much as the
# device (1.4e-6 on the first; tests/test_sweep_terms_cpu.py).  DESIGN.md section 8 has what was tried.
KNOWN_MISSES = {
    ("near_noise_s143_m63", "rbf", True, 30.0): (1.4e6, {"default": 1.94e-6, "substitution": 1.94e-6, "product": 1.94e-6}),
    ("near_noise_s145_m65", "rbf", True, 4e3): (1.3e6, {"default": 4.08e-7, "substitution": 4.08e-7, "product": 4.08e-7}),
    ("reference_noise_130", "rbf", True, 30.0): (3.7e6, {"default": 3.37e-7, "substitution": 3.37e-7, "product": 3.38e-7}),
}

# The allowance for the judged side's own evaluation of the kernel, dk = CK eps (1 + |exponent argument|) k: four times the
# smallest constant that the float64 NumPy evaluation of the same formula (scaled coordinates x / ls, squared differences
# summed over the dimensions, exp) needs against the long-double one over K(X, C) and K(X, Z) of every case above.  That
# smallest constant is 4.10 (two_row_tiles' K(X, C), 4.03 on cross128's, 2 .. 4 on the others; test_sweep_terms_cpu.py
# recomputes it and asserts that it lies within CK_NEEDED and not 5 % below): the differences of scaled coordinates carry
# eps |x / ls| each, up to 2.5 eps here, into the exponent, whatever the exponent's own size.
CK_NEEDED = 4.10
CK = 4 * CK_NEEDED


def shape_args(shape):
    """(X, cand, Z, ls, kvar, noise, chunk) of a zvar_cases shape (targets at unit standard deviation are case_data's)."""
    _, n, d, c, m, chunk, noise, ell, kvar = ZC.SHAPES[shape]
    X, _, cand, Z, _ = ZC.case_data(shape, 1.0)
    return X, cand, Z, np.full(d, ell), kvar, noise, chunk


def columns(shape):
    """The candidate columns on which V and crossT of a LARGE case are judged (None: all).  cross128: 256 columns with the
    first and last of the first, a middle and the last 128-tile; second_superchunk: the first tile, the last tile of the first
    super-chunk, the whole second super-chunk and 128 more."""
    c = ZC.SHAPES[shape][3]
    rng = np.random.default_rng(7)
    if shape == "cross128":
        fixed = [0, 127, 64 * 128, 64 * 128 + 127, 16384, c - 1]
        rest = rng.choice(np.setdiff1d(np.arange(c), fixed), 256 - len(fixed), replace=False)
        return np.sort(np.concatenate([fixed, rest]))
    if shape == "second_superchunk":
        fixed = np.concatenate([np.arange(128), np.arange(65536 - 128, c)])
        rest = rng.choice(np.setdiff1d(np.arange(c), fixed), 128, replace=False)
        return np.sort(np.concatenate([fixed, rest]))
    return None


@functools.lru_cache(maxsize=None)
def float64_stages(name, substitution):
    shape, kernel = CASES[name]
    X, cand, Z, ls, kvar, noise, _ = shape_args(shape)
    return S.float64_stages(kernel, X, cand, Z, ls, kvar, noise, substitution, cand_is_z=shape == "cand_is_z")


def check(name, terms):
    """Layer A on the terms of a case (sweep_terms_restatement.check_stages' dictionary)."""
    shape, kernel = CASES[name]
    X, cand, Z, ls, kvar, noise, _ = shape_args(shape)
    return S.check_stages(terms, kernel, X, cand, Z, ls, kvar, noise, CK, cols=columns(shape))


def table_lines(label, res, width=44):
    """The printed table: one line per stage."""
    inv = res["inverse"]
    lines = ["%-*s inverse  rho %.3e  rho_ref %.3e  ratio %.3f  at %s  block16 %s  block128 %s" % (
        width, label, inv["rho"], inv["rho_ref"], inv["rho"] / (4 * inv["rho_ref"] + 1), inv["at"], inv["block16"],
        inv["block128"])]
    for k in ("V", "VZ", "crossT", "sc", "basez"):
        lines.append("%-*s %-8s ratio %.3f  at %s" % (width, label, k, res[k][0], res[k][1]))
    return lines
