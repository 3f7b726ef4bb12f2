"""The cases of the batch selection's later-stage tests (tests/test_batch_terms_cpu.py, tests/test_gpu_batch_terms.py) and their
truths, each computed once per process.  The designs are tests/zvar_cases.py's where one fits; imports nothing from bobe_amd.

Layer A (tests/batch_terms_restatement.py: each u row and each downdate alone, on the judged side's own inputs) runs on the
three paths of ``sweep_terms_cases.PATHS``; Layer B (the stage scores against literal long-double refits) on the same paths.

  tile_edge            130 points, 300 candidates, 77 integration points, 63 downdates: two row blocks of partial sums (2 live
                       rows in the second), 8 groups of 16 rows with 51 padding rows, Cp = 384 (k_batch_u's second workgroup
                       half padding), all 63 u rows (the pick record's slots 1 .. 63 beside the coordinate slots at 64)
  reference_noise_300  noise 1e-8, three row blocks, the substitution by default
  near_noise_m63 / m64 / m65   posterior variances within two decades of the noise, M across 64, a batch that is 40 % of the pool
  cand_is_z            the candidates ARE the integration points: V_used = V_Z with ldv = Mp, every pick an integration point too
  ragged_4chunks       picks gathered from a V retained across chunks of 256
  ill_conditioned      257 points in 5-D at lengthscale 1.2, kvar 50, noise 1e-8: the float64 literal refit itself is 2e-7 off
                       (eiv on targets of standard deviation 4e3, where its gaps hold for the whole batch)
  dim1 / dim8 / dim9 / dim16 / dim17   the plain loop over d in k_batch_u beside the scorer's templates on the dimension caps
                       (8, 16, 32: either side of both boundaries)
  second_superchunk    65536 + 200 candidates, forced picks either side of index 65536 (Layer A only)
  tile_edge-edges      forced picks on the strip (64), tile (128) and workgroup (256) edges of the three kernels (Layer A only)
  duplicates           tile_edge at noise 1e-8 with exact and 1e-7-shifted copies of the truth's first four picks in the pool

``CASES`` holds per (case, criterion) the batch size b the case runs at: the issue's, or where a gap closes before it the largest at which the truth
alone keeps the gap between its two best unmasked scores above GAP_MIN at every stage; ``GAPS`` the figures, which
tests/test_batch_terms_cpu.py recomputes.
"""
import functools

import numpy as np

import batch_terms_restatement as B
import sweep_terms_cases as SC
import zvar_cases as ZC

GAP_MIN = ZC.GAP_MIN
CK = SC.CK
PATHS = SC.PATHS

# shape: (seed, N, d, C, M, chunk, noise, lengthscale, kernel variance), zvar_cases.SHAPES' layout and recipe
NEW_SHAPES = {
    "ill_conditioned": (14, 257, 5, 400, 100, 0, 1e-8, 1.2, 50.0),
    "tile_edge_1e-8": (103, 130, 3, 300, 77, 0, 1e-8, 0.4, 2.0),
    "dim1": (151, 64, 1, 60, 20, 0, 1e-6, 0.15, 2.0),
    "dim8": (152, 64, 8, 60, 20, 0, 1e-6, 0.7, 2.0),
    "dim9": (153, 64, 9, 60, 20, 0, 1e-6, 0.7, 2.0),
    "dim16": (154, 64, 16, 60, 20, 0, 1e-6, 1.0, 2.0),
    "dim17": (155, 64, 17, 60, 20, 0, 1e-6, 1.0, 2.0),
}
SHAPES = dict(ZC.SHAPES, **NEW_SHAPES)


def case_data(shape, y_std=1.0):
    """(X, y, cand, Z, log-weights): zvar_cases.case_data, whose recipe the new shapes follow (with every column index taken
    modulo d, so that d = 1 has targets too)."""
    if shape in ZC.SHAPES:
        return ZC.case_data(shape, y_std)
    if shape == "duplicates":
        return duplicates_data(y_std)
    seed, n, d, c, m = SHAPES[shape][:5]
    rng = np.random.default_rng(seed)
    X, cand, Z = rng.uniform(size=(n, d)), rng.uniform(size=(c, d)), rng.uniform(size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1 % d] ** 2 - X[:, 2 % d] * X[:, 3 % d] + 0.1 * rng.normal(size=n)
    lw = 1.5 * rng.normal(size=m)
    y = (y - np.mean(y)) / np.std(y) * y_std + np.mean(y)
    return X, y, cand, Z, lw


def hyper(shape):
    """(lengthscales, kvar, noise, chunk)."""
    _, n, d, c, m, chunk, noise, ell, kvar = SHAPES["tile_edge_1e-8" if shape == "duplicates" else shape]
    return np.full(d, ell), kvar, noise, chunk


# name -> (shape, kernel, log-weights given, y_std, {criterion: b}).  b is the issue's batch where the truth alone keeps every
# gap above GAP_MIN there, else the largest that does; GAPS has the figures.
# The two log scores that read y_std^2 v+ (imiqr, eiv) need targets of some scale for their gaps: at y_std = 1 eiv's gap falls
# below GAP_MIN at stage 7 (tile_edge) and 1 (ill_conditioned), at 30 at stage 44 and 13, at 4e3 (zvar_cases' third scale) not
# within the batch.  wipv / wipstd gaps are relative and do not move with y_std.
CASES = {
    "tile_edge": ("tile_edge", "rbf", False, 30.0, {"wipv": 64, "wipstd": 64, "imiqr": 64, "eiv": 44, "zvar": 64}),
    "reference_noise_300": ("reference_noise_300", "matern", False, 1.0, {"wipv": 64, "wipstd": 54, "zvar": 64}),
    "near_noise_m63": ("near_noise_m63", "matern", True, 1.0, {"wipstd": 16, "zvar": 16}),
    "near_noise_m64": ("near_noise_m64", "matern", False, 1.0, {"wipstd": 16, "zvar": 16}),
    "near_noise_m65": ("near_noise_m65", "rbf", True, 1.0, {"wipstd": 16, "zvar": 16}),
    "cand_is_z": ("cand_is_z", "matern", False, 1.0, {"wipstd": 16, "zvar": 16}),
    "ragged_4chunks": ("ragged_4chunks", "rbf", True, 1.0, {"wipstd": 8, "zvar": 8}),
    "ill_conditioned": ("ill_conditioned", "rbf", True, 30.0, {"wipv": 32, "wipstd": 32, "imiqr": 32, "zvar": 32}),
    "ill_conditioned_4e3": ("ill_conditioned", "rbf", True, 4e3, {"eiv": 32}),
    "dim1": ("dim1", "rbf", False, 1.0, {"wipstd": 4, "zvar": 4}),
    "dim8": ("dim8", "matern", True, 1.0, {"wipstd": 4, "zvar": 4}),
    "dim9": ("dim9", "rbf", True, 1.0, {"wipstd": 4, "zvar": 4}),
    "dim16": ("dim16", "matern", False, 1.0, {"wipstd": 4, "zvar": 4}),
    "dim17": ("dim17", "rbf", False, 1.0, {"wipstd": 4, "zvar": 4}),
}
LAYER_B = [(name, key) for name, c in CASES.items() for key in c[4]]
SHORT = ("ragged_4chunks", "dim1", "dim8", "dim9", "dim16", "dim17")      # the cases whose batch is below 16 by design

# (case, criterion) -> (b, the truth's smallest gap over the b stages, its stage, the float64 literal refit's worst error
# against the truth over all stages and candidates: relative for wipv / wipstd, over 1 + |truth| for the log scores).
# tests/test_batch_terms_cpu.py recomputes every row.  Where b is below the issue's the next stage's gap is
# below GAP_MIN: reference_noise_300 wipstd at stage 54 (8.4e-7), tile_edge eiv at stage 44.
GAPS = {
    ("tile_edge", "wipv"): (64, 5.47e-05, 54, 2.1e-10),
    ("tile_edge", "wipstd"): (64, 2.85e-05, 62, 8.6e-11),
    ("tile_edge", "imiqr"): (64, 1.16e-05, 62, 2.6e-11),
    ("tile_edge", "eiv"): (44, 1.05e-06, 23, 8.3e-11),
    ("tile_edge", "zvar"): (64, 0.00164, 39, 5.9e-08),
    ("reference_noise_300", "wipv"): (64, 2.28e-06, 53, 6e-14),
    ("reference_noise_300", "wipstd"): (54, 5.67e-06, 19, 6.2e-14),
    ("reference_noise_300", "zvar"): (64, 0.000366, 25, 4.2e-07),
    ("near_noise_m63", "wipstd"): (16, 1.16e-05, 7, 6.4e-13),
    ("near_noise_m63", "zvar"): (16, 0.00107, 4, 3.4e-09),
    ("near_noise_m64", "wipstd"): (16, 0.000137, 14, 3.8e-13),
    ("near_noise_m64", "zvar"): (16, 0.038, 10, 5.1e-10),
    ("near_noise_m65", "wipstd"): (16, 5.23e-05, 12, 4.4e-10),
    ("near_noise_m65", "zvar"): (16, 0.00389, 5, 1.5e-07),
    ("cand_is_z", "wipstd"): (16, 9.77e-05, 15, 4.3e-13),
    ("cand_is_z", "zvar"): (16, 0.00243, 0, 5.1e-10),
    ("ragged_4chunks", "wipstd"): (8, 0.000723, 5, 6.2e-13),
    ("ragged_4chunks", "zvar"): (8, 0.105, 6, 9.9e-10),
    ("ill_conditioned", "wipv"): (32, 8.37e-05, 13, 1.8e-07),
    ("ill_conditioned", "wipstd"): (32, 4.2e-05, 13, 9.2e-08),
    ("ill_conditioned", "imiqr"): (32, 4.2e-05, 13, 1.3e-08),
    ("ill_conditioned", "zvar"): (32, 0.00174, 13, 0.00072),
    ("ill_conditioned_4e3", "eiv"): (32, 0.0506, 31, 3.1e-08),
    ("dim1", "wipstd"): (4, 3.42e-05, 2, 9.6e-11),
    ("dim1", "zvar"): (4, 0.0242, 3, 5.7e-08),
    ("dim8", "wipstd"): (4, 0.000104, 1, 7.4e-16),
    ("dim8", "zvar"): (4, 0.0686, 1, 1e-10),
    ("dim9", "wipstd"): (4, 0.000575, 3, 6.2e-16),
    ("dim9", "zvar"): (4, 0.00472, 3, 1.8e-10),
    ("dim16", "wipstd"): (4, 1.51e-05, 1, 5.5e-16),
    ("dim16", "zvar"): (4, 0.0138, 3, 7.5e-11),
    ("dim17", "wipstd"): (4, 2.52e-05, 1, 5.5e-16),
    ("dim17", "zvar"): (4, 0.127, 3, 2.3e-10),
}

# Layer A with forced picks: name -> (shape, kernel, criterion, forced picks)
FORCED = {
    "second_superchunk": ("second_superchunk", "rbf", "wipstd", [65536, 0, 65735, 65535, 8191, 8192]),
    "tile_edge-edges": ("tile_edge", "matern", "wipstd", [0, 63, 64, 127, 128, 255, 256, 299]),
}
# Layer A along the device's own picks: (case, criterion); the largest batches and one case per design otherwise
LAYER_A = [("tile_edge", "wipstd"), ("tile_edge", "eiv"), ("reference_noise_300", "wipv"), ("near_noise_m63", "wipstd"),
           ("near_noise_m64", "zvar"), ("near_noise_m65", "wipstd"), ("cand_is_z", "wipstd"), ("ragged_4chunks", "wipstd"),
           ("ill_conditioned", "wipstd"), ("dim1", "wipstd"), ("dim8", "wipstd"), ("dim9", "zvar"), ("dim16", "wipstd"),
           ("dim17", "wipstd")]

# Where float64 NumPy running the downdate recursion from a triangular solve's stage 0 misses the rule itself: (case, criterion)
# -> the first stage that misses.  On the ill-conditioned design, where the float64 literal refit is 1e-7 off too and the rule is
# judged per candidate: zvar 8.5e-7 (1 + |truth|) at stage 1 where the literal refit is 4.7e-7 off, wipv from stage 25 and
# wipstd at stage 30 marginally (2.3e-7 against 1.8e-7, 1.2e-7 against 9.2e-8 overall).  On 300 points at noise 1e-8 zvar from
# stage 35 (3.1e-7 overall beside a literal refit 4.2e-7 off).
RECURSION_MISSES = {("ill_conditioned", "zvar"): 1, ("ill_conditioned", "wipv"): 25, ("ill_conditioned", "wipstd"): 30,
                    ("reference_noise_300", "zvar"): 35}

# Where the DEVICE misses Layer B's rule with every Layer A ratio of the run below 1: (case, criterion) -> (first stage that
# misses, what loses it, {path: (the device's worst error over the missing stages, float64 NumPy's running the recursion on the
# device's own stage-0 terms, the first stage at which that NumPy run misses)}).  Strict expected failures of
# tests/test_gpu_batch_terms.py, which runs Layer A along the picks of every run that misses; figures from an MI355X.
# Two kinds.  "the sweep's terms": stage 0 itself misses - no downdate has run, and NumPy scoring the device's stage-0 terms is
# as far off: the loss of the product with the explicit inverse factor that tests/sweep_terms_cases.py records (KNOWN_MISSES
# there, stage "V").  "carried by the recursion": stage 0 holds the rule and a later stage does not; float64 NumPy running the
# same downdates on the device's stage-0 terms misses from the same stage (or within two) by the same amount, so no kernel of
# the later stages is at fault.  On near_noise_m65 the recursion from a triangular solve's stage 0 holds the rule (2.1e-7
# against the literal refit's 1.5e-7; tests/test_batch_terms_cpu.py): the device's stage-0 error, inside the rule there, grows
# relative to base_z and s_c as the downdates shrink them.  On the ill-conditioned design, on 300 points at noise 1e-8 and on the
# duplicates the float64 recursion misses from any stage 0 (RECURSION_MISSES), beside a float64 literal refit that is 1e-7 off
# itself.  That the stage-0 misses are the inverse-factor product's is inferred from NumPy scoring the device's terms as far
# off; tests/test_gpu_sweep_terms.py's Layer A was not run on those two shapes.
_ALL = lambda *f: {"default": f, "substitution": f, "product": f}          # noqa: E731
KNOWN_MISSES = {
    ("near_noise_m65", "zvar"): (9, "carried by the recursion", _ALL(4.52e-7, 4.40e-7, 9)),
    ("ill_conditioned", "wipv"): (25, "carried by the recursion", {"default": (2.65e-7, 2.50e-7, 27), "substitution":
                                                                    (2.65e-7, 2.50e-7, 27), "product": (2.55e-7, 2.32e-7, 26)}),
    ("ill_conditioned", "wipstd"): (30, "carried by the recursion", {"default": (1.32e-7, 1.25e-7, 30), "substitution":
                                                                      (1.32e-7, 1.25e-7, 30), "product": (1.28e-7, 1.16e-7, 31)}),
    ("ill_conditioned", "zvar"): (0, "the sweep's terms", {"default": (2.58e-3, 4.36e-3, 0), "substitution": (2.58e-3, 4.36e-3, 0),
                                                           "product": (2.38e-3, 3.46e-3, 0)}),
    ("reference_noise_300", "zvar"): (50, "carried by the recursion", {"default": (3.31e-7, 2.94e-7, 50), "substitution":
                                                                        (3.24e-7, 3.01e-7, 9), "product": (3.31e-7, 2.94e-7, 50)}),
    ("dim1", "zvar"): (0, "the sweep's terms", _ALL(1.78e-5, 1.78e-5, 0)),
    ("duplicates", "zvar"): (8, "carried by the recursion", {"default": (4.20e-7, 4.16e-7, 8), "substitution":
                                                             (4.20e-7, 4.16e-7, 8), "product": (4.70e-7, 4.69e-7, 9)}),
}

DUP_B = 16                                   # the duplicates case's batch
DUP_KEYS = ("wipstd", "zvar")
DUP_SHIFT = 1e-7
DUP_TOL = 1e-9                               # DESIGN section 2's argmin rule


def columns(shape, picks=()):
    """The candidate columns on which u_c and crossT are judged (None: all): sweep_terms_cases.columns plus the picks."""
    cols = SC.columns(shape) if shape in ZC.SHAPES else None
    return None if cols is None else np.union1d(cols, np.asarray(picks, dtype=np.int64))


def _args(shape, kernel, weighted, y_std=1.0):
    X, y, cand, Z, lw = case_data(shape, y_std)
    ys, _, std = ZC.standardise(y)
    ls, kvar, noise, _ = hyper(shape)
    return (kernel, X, ys, cand, Z, ls, kvar, noise, std, lw if weighted else None)


@functools.lru_cache(maxsize=None)
def truth(name, key, b=None):
    """{"picks", "truth" [b x C] long double, "gaps" [b], "f64" [b x C]: the float64 literal refit along the truth's picks} of a
    Layer B case.  The truth is the literal refit in its row-append form (batch_terms_restatement.append_batch)."""
    shape, kernel, weighted, y_std, bs = CASES[name]
    b = bs[key] if b is None else b
    args = _args(shape, kernel, weighted, y_std)
    picks, stages, gaps, _ = B.append_batch(*args, b, key)
    _, f64, _, _ = B.literal_batch(*args, b, key, dtype=np.float64, follow=picks)
    return {"picks": picks, "truth": stages, "gaps": gaps, "f64": f64}


@functools.lru_cache(maxsize=None)
def duplicates_pool():
    """The candidates of the duplicates case: tile_edge's at noise 1e-8, then for each of the first four picks of the WIPStd
    truth on that pool an exact copy and a copy moved by 1e-7 per coordinate."""
    X, y, cand, Z, lw = case_data("tile_edge_1e-8")
    ys, _, std = ZC.standardise(y)
    ls, kvar, noise, _ = hyper("tile_edge_1e-8")
    picks = B.append_batch("rbf", X, ys, cand, Z, ls, kvar, noise, std, None, 4, "wipstd")[0]
    extra = [row for p in picks for row in (cand[p], cand[p] + DUP_SHIFT)]
    return np.ascontiguousarray(np.vstack([cand] + extra)), picks


def duplicates_data(y_std=1.0):
    X, y, _, Z, lw = case_data("tile_edge_1e-8", y_std)
    return X, y, duplicates_pool()[0], Z, lw


def duplicates_truth(key, device_picks):
    """The truth along the device's picks (a pick's copy ties with it, so the truth's own argmin is not defined to 1e-6):
    (truth [b x C], float64 literal refit [b x C], the truth's argmins)."""
    args = _args("duplicates", "rbf", False)
    b = len(device_picks)
    _, stages, _, mins = B.append_batch(*args, b, key, follow=device_picks)
    _, f64, _, _ = B.literal_batch(*args, b, key, dtype=np.float64, follow=device_picks)
    return stages, f64, mins


def recursion(name_or_shape, kernel, picks, solve=False):
    """batch_terms_restatement.recursion (float64 NumPy) on a shape along ``picks``."""
    X, _, cand, Z, _ = case_data(name_or_shape)
    ls, kvar, noise, _ = hyper(name_or_shape)
    return B.recursion(kernel, X, cand, Z, ls, kvar, noise, picks, cand_is_z=name_or_shape == "cand_is_z", solve=solve)


def check(shape, kernel, terms):
    """Layer A on the terms of a shape (batch_terms_restatement.check_terms' dictionary)."""
    X, _, cand, Z, _ = case_data(shape)
    ls, kvar, _, _ = hyper(shape)
    return B.check_terms(terms, kernel, X, cand, Z, ls, kvar, CK, cols=columns(shape, terms["picks"]))


def table_line(label, res, width=52):
    return "%-*s %s" % (width, label, "  ".join("%s %.3f at %s" % (k, res[k][0], res[k][1])
                                                for k in ("uc", "uz", "sc", "basez", "crossT")))
