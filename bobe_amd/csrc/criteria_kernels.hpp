// Kernels of the importance-weighted scoring pass (bobe_gp_wip_sweep_w, bobe_gp_wip_select_batch_w) and of the scores' input
// gradients (bobe_gp_wip_grad_w, at the end of the file); gfx950.  Included by gp_criteria.hip only.  (The gradients' chain
// takes its rows stage and its cross kernel's front from wg_kernels.hpp, as bobe_gp_wip_grad's does.)
//
// The sweep scores candidate c against integration point z through the fantasy variance v+(z|c) (k_wip_score,
// sweep_kernels.hpp).  Here every z also carries a log-weight l_z (the log of its quadrature weight under the flat prior on
// the unit cube, up to a constant; without one the points count as draws of the surrogate posterior, l_z = -mu_z), and with
//   mu_z = y_std (K(X,Z)^T alpha)_z,   b_z = y_std^2 base_z (floored as the scorer floors),   a_z = l_z + mu_z,
//   omega = softmax(a),   u = Phi^-1(3/4)
// four scores are formed in one pass over crossT:
//   0 wipv    sum_z omega_z v+                     1 wipstd   sum_z omega_z sqrt(v+)
//   2 imiqr   LSE_z [a_z + x + log1p(-exp(-2x))],  x = u sqrt(v+)        (= log sum_z e^{a_z} 2 sinh(u sqrt(v+)))
//   3 eiv     -LSE_z [l_z + 2 mu_z + 2 b_z - v+]                         (= -log of the candidate's GAIN R(c); EIV = S - R)
// The two log scores are running-maximum log-sum-exps per candidate: no shift chosen ahead of the pass survives a dominant z
// whose v+ collapses for one candidate only.  Every sum runs in a fixed order: same state, same bits.
// Domain: finite inputs and y_std > 0.  Then every term of the two log-sum-exps is finite (v+ >= 1e-12 y_std^2 > 0, so x > 0
// and log1p(-exp(-2x)) is finite) and so are the results.  y_std = 0 makes x = 0 and every IMIQR term -inf: lse_add then
// returns NaN (exp(-inf - (-inf))), as it does for two +inf terms - the NaN marks an input outside the contract.
#pragma once
#include "kernels_common.hpp"
#include "wg_kernels.hpp"

namespace bobe {

constexpr double IMIQR_U = 0.6744897501960817;    // Phi^-1(3/4)
static_assert(ZTERM_ROWS == 6, "k_wip_zterms / k_wip_score_w / k_wip_score_zz address the table's rows mu, a, omega, e, l, lambda by number");

// one term more in a running-maximum log-sum-exp (mx = -inf, s = 0 to start with; t finite, see "Domain" above)
__device__ __forceinline__ void lse_add(double& mx, double& s, double t) {
  if (t > mx) {
    s = s * exp(mx - t) + 1.0;
    mx = t;
  } else {
    s += exp(t - mx);
  }
}

// red[0 .. 255] -> red[0], pairwise in a fixed order; MAX: the maximum instead of the sum.  Ends synchronised.
template <bool MAX>
__device__ __forceinline__ double block_fold256(double* red, double v) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double x = red[threadIdx.x], y = red[threadIdx.x + o];
      red[threadIdx.x] = MAX ? ((y > x || y != y) ? y : x) : (x + y);
    }
    __syncthreads();
  }
  return red[0];
}

// The per-z table zt [ZTERM_ROWS x ldt] and log S, ONE workgroup of 256 (thread t owns z = t, t + 256, ...).
//   first: mu_z = y_std * sum_rb part[rb][z] (the row-block partial sums of K(X,Z)^T alpha, block 0 first), l_z = logw[z] or
//          -mu_z, a_z, omega = softmax(a) (maximum, then the sum of exp(a - max))
//   always: e_z = l_z + 2 mu_z + 2 b_z with b_z = y_std^2 * base_z (non-finite or < 1e-12 -> 1e-12), and
//          *log_s = LSE_z e_z = log sum_z exp(l_z + 2 mu_z + 2 b_z)
//   lam:   in addition row 5, lambda_z = g_z - *log_ez with g_z = l_z + mu_z + b_z / 2 and *log_ez = LSE_z g_z = log E[Z] (it
//          follows b_z like the e row: written on every call that asks for it)
// A later stage of the batch selection calls it with first = 0 on its downdated base_z: mu, a, omega stay.
static __global__ __launch_bounds__(256) void k_wip_zterms(const double* __restrict__ part, int64_t ldp, int nrb, int64_t m,
                                                           double ystd, const double* __restrict__ logw,
                                                           const double* __restrict__ basez, double* __restrict__ zt,
                                                           int64_t ldt, int first, double* __restrict__ log_s, int lam,
                                                           double* __restrict__ log_ez) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double* mu = zt;
  double* a = zt + ldt;
  double* om = zt + 2 * ldt;
  double* e3 = zt + 3 * ldt;
  double* ell = zt + 4 * ldt;
  if (first) {
    double amax = -INFINITY;
    for (int64_t z = t; z < m; z += 256) {
      double q = 0.0;
      for (int rb = 0; rb < nrb; ++rb) q += part[(int64_t)rb * ldp + z];
      const double muz = ystd * q;
      const double l = logw ? logw[z] : -muz;
      const double az = l + muz;
      mu[z] = muz;
      ell[z] = l;
      a[z] = az;
      amax = (az > amax || az != az) ? az : amax;
    }
    amax = block_fold256<true>(red, amax);
    double s = 0.0;
    for (int64_t z = t; z < m; z += 256) s += exp(a[z] - amax);
    s = block_fold256<false>(red, s);
    for (int64_t z = t; z < m; z += 256) om[z] = exp(a[z] - amax) / s;
  }
  const double ystd2 = ystd * ystd;
  double emax = -INFINITY;
  for (int64_t z = t; z < m; z += 256) {
    double b = basez[z];
    if (!(b >= NOISE_FLOOR) || b > 1.79769313486231571e308) b = NOISE_FLOOR;
    const double e = ell[z] + 2.0 * mu[z] + 2.0 * (b * ystd2);
    e3[z] = e;
    emax = (e > emax || e != e) ? e : emax;
  }
  emax = block_fold256<true>(red, emax);
  double s = 0.0;
  for (int64_t z = t; z < m; z += 256) s += exp(e3[z] - emax);
  s = block_fold256<false>(red, s);
  if (t == 0) *log_s = emax + log(s);
  if (!lam) return;                                // (uniform)
  // row 5, for k_wip_score_zz: lambda_z = g_z - LSE_z g_z with g_z = l_z + mu_z + b_z / 2, the log of z's share of E[Z]
  double* lm = zt + 5 * ldt;
  double gmax = -INFINITY;
  for (int64_t z = t; z < m; z += 256) {
    double b = basez[z];
    if (!(b >= NOISE_FLOOR) || b > 1.79769313486231571e308) b = NOISE_FLOOR;
    const double g = (ell[z] + mu[z]) + 0.5 * (b * ystd2);
    lm[z] = g;
    gmax = (g > gmax || g != g) ? g : gmax;
  }
  gmax = block_fold256<true>(red, gmax);
  double sg = 0.0;
  for (int64_t z = t; z < m; z += 256) sg += exp(lm[z] - gmax);
  sg = block_fold256<false>(red, sg);
  const double lez = gmax + log(sg);
  for (int64_t z = t; z < m; z += 256) lm[z] -= lez;
  if (t == 0) *log_ez = lez;
}

// ---- the evidence-variance scorer (bobe_gp_wip_sweep_zvar): zvar[c] = -log T(c),
//   T(c) = sum_z sum_z' omega_z omega_z' expm1(r_z r_z'),   omega_z = exp(lambda_z) (the table's row 5),
//   r_z(c) = y_std cross_z / sqrt(s_c), cross_z formed exactly as k_wip_score_w forms it.
// The expected variance of Z = sum_z e^{l_z} e^{f(z)} after one observation at c is Var Z - E[Z]^2 T(c) (the law of total
// variance for the lognormal e^f: the observation moves mu_z by r_z xi, xi ~ N(0, 1), and lowers b_z by r_z^2); the
// c-independent Var Z is not formed.  Rules:
//   |r_z| <= sqrt(b_z), b_z = y_std^2 base_z floored as k_wip_zterms floors it (so b+ >= 0: the counterpart of v+ >= 1e-12);
//   a non-finite cross_z gives r_z = 0; a candidate whose s_c is not > 0 has every r_z = 0;
//   T <= 0 (every r_z = 0, T underflown or rounding-negative) gives zvar = +inf: the candidate teaches nothing.
// No exponent above 0 is taken: with h_c = max_z (lambda_z + r_z^2 / 2) every pair has lambda_z + lambda_z' + r_z r_z' <=
// 2 h_c (r r' <= (r^2 + r'^2) / 2), so with p_z = lambda_z - h_c and E_z = exp(p_z) a pair with |r r'| < 1 adds
// E_z E_z' expm1(r r'), any other exp(p_z + p_z' + r r') - E_z E_z', and zvar = -(2 h_c + log sum).  One transcendental per
// pair, C M^2 / 2 of them per launch: the cost grows with the SQUARE of M where the other scorers' grows with M.
// Shape: one workgroup = ZZ_G candidates (lane within a half-wave) x ZZ_S interleaved z-slices.  Pass 1 finds h_c (one O(M)
// pass, the slices' maxima folded through LDS).  Pass 2 walks the z' tiles J of ZZ_T points - r and E of the tile for the
// workgroup's candidates in LDS, [z'][candidate]: a half-wave reads 32 consecutive doubles, conflict-free - and under every J
// the tiles I <= J, where a thread forms r, p, E of its own z = slice, slice + ZZ_S, ... again from crossT (one kernel
// evaluation per ZZ_T pairs) and sums over z' in J (z' > z on the diagonal tile; the diagonal pair apart): off-diagonal pairs
// count twice.  Every sum runs in a fixed order that depends on M and the candidate alone; the slices are combined in order.
constexpr int ZZ_G = 32, ZZ_S = 8, ZZ_T = 64;
static_assert(ZZ_G * ZZ_S == 256 && ZZ_S == 8 && ZZ_T % ZZ_S == 0,
              "k_wip_score_zz: 256 threads = candidates x 8 slices (combined by name at the end), whole rounds per tile");

template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_wip_score_zz(const double* __restrict__ crossT, int64_t ldx,
                                                      const double* __restrict__ CsT, int64_t ldc,
                                                      const double* __restrict__ ZsT, int64_t ldz, int64_t m,
                                                      const double* __restrict__ sc, const double* __restrict__ basez,
                                                      const double* __restrict__ zt, int64_t ldt, int64_t ncols, Hyper h,
                                                      double ystd, double* __restrict__ out) {
  __shared__ double rs[ZZ_T][ZZ_G], es[ZZ_T][ZZ_G], ls[ZZ_T], red[ZZ_S][ZZ_G];
  const int t = threadIdx.x, cx = t % ZZ_G, sl = t / ZZ_G;
  const int64_t c = (int64_t)blockIdx.x * ZZ_G + cx;
  const bool live = c < ncols;
  const double* lam = zt + 5 * ldt;
  double xc[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xc[j] = (live && j < h.d) ? CsT[j * ldc + c] : 0.0;
  const double s = live ? sc[c] : 1.0;
  const double scale = (s > 0.0) ? ystd / sqrt(s) : 0.0;
  const bool dead = !(s > 0.0);
  const double ystd2 = ystd * ystd;
  // r_z of this thread's candidate (z < m, live)
  auto r_of = [&](int64_t z) {
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      if (j < h.d) {
        const double df = xc[j] - ZsT[j * ldz + z];
        r2 += df * df;
      }
    }
    const double cross = kern_eval<KERN>(r2, h.kvar) - crossT[z * ldx + c];
    double b = basez[z];
    if (!(b >= NOISE_FLOOR) || b > 1.79769313486231571e308) b = NOISE_FLOOR;
    const double cap = sqrt(b * ystd2);
    double r = cross * scale;
    if (dead || !(fabs(cross) <= 1.79769313486231571e308)) r = 0.0;
    if (r > cap) r = cap;
    if (r < -cap) r = -cap;
    return r;
  };
  // pass 1: h_c
  double hm = -INFINITY;
  if (live) {
    for (int64_t z = sl; z < m; z += ZZ_S) {
      const double r = r_of(z);
      const double q = lam[z] + 0.5 * (r * r);
      hm = (q > hm || q != q) ? q : hm;
    }
  }
  red[sl][cx] = hm;
  __syncthreads();
  hm = red[0][cx];
#pragma unroll
  for (int k = 1; k < ZZ_S; ++k) {
    const double y = red[k][cx];
    hm = (y > hm || y != y) ? y : hm;
  }
  // pass 2: the pair sum
  double off = 0.0, dia = 0.0;
  auto pair = [&](double x, double ee, double pp) {
    return (fabs(x) < 1.0) ? ee * expm1(x) : exp(pp + x) - ee;
  };
  for (int64_t j0 = 0; j0 < m; j0 += ZZ_T) {
    __syncthreads();
    const int zn = (m - j0 < ZZ_T) ? (int)(m - j0) : ZZ_T;
    for (int zz = sl; zz < ZZ_T; zz += ZZ_S) {
      const bool in = live && zz < zn;
      const double r = in ? r_of(j0 + zz) : 0.0;
      rs[zz][cx] = r;
      es[zz][cx] = in ? exp(lam[j0 + zz] - hm) : 0.0;
    }
    if (t < ZZ_T) ls[t] = (t < zn) ? lam[j0 + t] : 0.0;
    __syncthreads();
    if (!live) continue;
    for (int64_t i0 = 0; i0 <= j0; i0 += ZZ_T) {
      const bool diag = i0 == j0;
      const int in_ = (m - i0 < ZZ_T) ? (int)(m - i0) : ZZ_T;
      for (int iz = sl; iz < in_; iz += ZZ_S) {
        const double r = r_of(i0 + iz);
        const double p = lam[i0 + iz] - hm;
        const double e = exp(p);
        if (diag) dia += pair(r * r, e * e, p + p);
        for (int zz = diag ? iz + 1 : 0; zz < zn; ++zz)
          off += pair(r * rs[zz][cx], e * es[zz][cx], p + (ls[zz] - hm));
      }
    }
  }
  __syncthreads();
  red[sl][cx] = 2.0 * off + dia;
  __syncthreads();
  if (sl == 0 && live) {
    const double tot = ((red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx])) +
                       ((red[4][cx] + red[5][cx]) + (red[6][cx] + red[7][cx]));
    out[c] = (tot > 0.0) ? -(2.0 * hm + log(tot)) : ((tot <= 0.0) ? INFINITY : tot);
  }
}

// ---- the weighted scorer: k_wip_score's shape (64 candidates x 4 interleaved z-slices per workgroup, z tiles of 128 through
// LDS, eight crossT rows in flight per thread) with omega_z, a_z, e_z riding in the LDS tile next to base_z and one
// accumulator per requested criterion (out_* = NULL: not requested, nothing computed for it).  v+ is formed exactly as
// k_wip_score forms it.  The four slices of a candidate are combined in a fixed order.
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_wip_score_w(const double* __restrict__ crossT, int64_t ldx,
                                                     const double* __restrict__ CsT, int64_t ldc,
                                                     const double* __restrict__ ZsT, int64_t ldz, int64_t m,
                                                     const double* __restrict__ sc, const double* __restrict__ basez,
                                                     const double* __restrict__ zt, int64_t ldt, int64_t ncols, Hyper h,
                                                     double ystd2, double* __restrict__ out_v, double* __restrict__ out_s,
                                                     double* __restrict__ out_i, double* __restrict__ out_e) {
  extern __shared__ double zsm[];          // [d][ZT] + base[ZT] + omega[ZT] + a[ZT] + e[ZT]
  constexpr int ZT = 128;
  __shared__ double red[6][4][64];
  const int t = threadIdx.x, cx = t & 63, sl = t >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cx;
  const bool live = c < ncols;
  const bool do_v = out_v != nullptr, do_s = out_s != nullptr, do_i = out_i != nullptr, do_e = out_e != nullptr;
  double xc[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xc[j] = (live && j < h.d) ? CsT[j * ldc + c] : 0.0;
  const double s = live ? sc[c] : 1.0;
  const bool sbad = !(s >= 0.0);
  double sv = 0.0, ss = 0.0;
  double mi = -INFINITY, si = 0.0, me = -INFINITY, se = 0.0;
  double* const zb = zsm + h.d * ZT;       // base, omega, a, e
  for (int64_t z0 = 0; z0 < m; z0 += ZT) {
    __syncthreads();
    for (int e = t; e < h.d * ZT; e += 256) {
      const int j = e / ZT, zz = e % ZT;
      zsm[j * ZT + zz] = (z0 + zz < m) ? ZsT[j * ldz + z0 + zz] : 0.0;
    }
    if (t < ZT) {
      const bool in = z0 + t < m;
      zb[t] = in ? basez[z0 + t] : 0.0;
      zb[ZT + t] = in ? zt[2 * ldt + z0 + t] : 0.0;
      zb[2 * ZT + t] = in ? zt[ldt + z0 + t] : 0.0;
      zb[3 * ZT + t] = in ? zt[3 * ldt + z0 + t] : 0.0;
    }
    __syncthreads();
    const int zn = (m - z0 < ZT) ? (int)(m - z0) : ZT;
    if (live) {
      auto score = [&](int zz, double ct) {
        double r2 = 0.0;
#pragma unroll
        for (int j = 0; j < DCAP; ++j) {
          if (j < h.d) {
            const double df = xc[j] - zsm[j * ZT + zz];
            r2 += df * df;
          }
        }
        const double cross = kern_eval<KERN>(r2, h.kvar) - ct;
        double v = zb[zz] - (cross * cross) / s;
        if (sbad) v = NOISE_FLOOR;
        if (v != v) v = NOISE_FLOOR;
        if (v < NOISE_FLOOR) v = NOISE_FLOOR;
        v *= ystd2;
        const double om = zb[ZT + zz];
        if (do_v) sv += om * v;
        if (do_s || do_i) {
          const double rv = sqrt(v);
          if (do_s) ss += om * rv;
          if (do_i) {
            const double x = IMIQR_U * rv;
            lse_add(mi, si, zb[2 * ZT + zz] + x + log1p(-exp(-2.0 * x)));
          }
        }
        if (do_e) lse_add(me, se, zb[3 * ZT + zz] - v);
      };
      const double* cp = crossT + z0 * ldx + c;
      int zz = sl;
      for (; zz + 28 < zn; zz += 32) {
        double ct[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) ct[q] = cp[(int64_t)(zz + 4 * q) * ldx];
#pragma unroll
        for (int q = 0; q < 8; ++q) score(zz + 4 * q, ct[q]);
      }
      for (; zz < zn; zz += 4) score(zz, cp[(int64_t)zz * ldx]);
    }
  }
  red[0][sl][cx] = sv;
  red[1][sl][cx] = ss;
  red[2][sl][cx] = mi;
  red[3][sl][cx] = si;
  red[4][sl][cx] = me;
  red[5][sl][cx] = se;
  __syncthreads();
  if (sl == 0 && live) {
    if (do_v) out_v[c] = (red[0][0][cx] + red[0][1][cx]) + (red[0][2][cx] + red[0][3][cx]);
    if (do_s) out_s[c] = (red[1][0][cx] + red[1][1][cx]) + (red[1][2][cx] + red[1][3][cx]);
    // the slices' (maximum, sum) pairs: a slice without a point has (-inf, 0) and adds 0 (m >= 1: slice 0 has one)
    auto fold = [&](int r) {
      double mx = red[r][0][cx];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const double y = red[r][k][cx];
        mx = (y > mx || y != y) ? y : mx;
      }
      double p[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double sk = red[r + 1][k][cx];
        p[k] = (sk == 0.0) ? 0.0 : sk * exp(red[r][k][cx] - mx);
      }
      return mx + log((p[0] + p[1]) + (p[2] + p[3]));
    };
    if (do_i) out_i[c] = fold(2);
    if (do_e) out_e[c] = -fold(4);
  }
}

// ---- input gradients of the four scores for a HANDFUL of candidates (bobe_gp_wip_grad_w) ---------------------------------
// The few-candidate chain of bobe_gp_wip_grad (sweep_kernels.hpp, "the same for a HANDFUL of candidates") with one stage more;
// the front of the cross kernel and the rows stage are that chain's own (wg_kernels.hpp).
// Each score is a function of the v+_z alone, so d score_k / dx_j = sum_z rho^k_z d v+_z / dx_j with
//   rho^0 = omega_z        rho^1 = omega_z / (2 sqrt(v+))        rho^3 = exp(e_z - v+ + eiv)
//   rho^2 = exp(t_z - imiqr) coth(x) u / (2 sqrt(v+)),  t_z = a_z + x + log1p(-e^{-2x}),  x = u sqrt(v+)
// The two softmax weights need the candidate's FINISHED log-sum-exp over all z (exponents reach 1e5 at y_std ~ 4e3: only
// exp(t - LSE) <= 1 is ever formed), which the single pass of k_wg_cross cannot supply: it forms the weights while it forms v+.
// So k_wg_cross_w stops at cross_z, v+_z, the floored flag and one (maximum, sum) pair per workgroup, k_wg_weights_w folds
// the pairs, forms rho^k w1 (w1 = d v+ / d cross, w2 = d v+ / d s: k_wg_cross's) and the z-side sums, k_wg_rows contracts
// q = W_Z (rho^k w1) with T[j][n] for every requested criterion in one read of W_Z, k_wg_final_w combines.  A floored z is a
// constant: it contributes its value and no gradient.  No atomics, every sum in a fixed order that depends on the
// candidate alone - not on C, its place in the group, the pointer kinds or the other criteria requested.
constexpr int WGW_ZS = 2 + MAX_D;           // doubles per (candidate, criterion) of k_wg_weights_w: sum rho w2, the score, Dz[j]

struct WgwOut {
  double* score[4];
  double* grad[4];
};

// k_wg_cross up to the per-z quantities (wg_cross_front, wg_vplus).  Writes cross_z, v+_z (floored, times y_std^2) and the floored flag
// (padding: 0, 0, 1), s_c (workgroup 0), and - mask bits 2 / 3 - the workgroup's (maximum, sum of exp(t - maximum)) of the
// IMIQR / EIV terms into pairs[(c * gridDim.x + blockIdx.x) * 4 + {0, 1} / {2, 3}]; a workgroup without a point: (-inf, 0).
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_wg_cross_w(const double* __restrict__ ZsT, int64_t ldz, int64_t m,
                                                    const double* __restrict__ VZ, int64_t ldw, int64_t n, int64_t np,
                                                    const double* __restrict__ v, const double* __restrict__ cand, Hyper h,
                                                    double kself, const double* __restrict__ basez, double ystd2,
                                                    const double* __restrict__ zt, int64_t ldt, int mask,
                                                    double* __restrict__ crossA, double* __restrict__ vplusA,
                                                    double* __restrict__ flagA, int64_t lda, double* __restrict__ sA,
                                                    double* __restrict__ pairs) {
  extern __shared__ double kcs[];                 // [n]: v = L^-1 k_c
  __shared__ double red[4], redz[4][64], fold[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = blockIdx.y, z = (int64_t)blockIdx.x * 64 + lane;
  double wk;
  const double s = wg_cross_front(v + c * np, n, VZ, ldw, z, kself, kcs, red, redz, wk);
  const bool sbad = !(s >= 0.0);
  if (wave != 0 && !(mask & 12)) return;          // (uniform per wave; the two maxima below are folded by the whole workgroup)
  double cross = 0.0, vs = 0.0, fl = 1.0, ti = -INFINITY, te = -INFINITY;
  if (wave == 0 && z < m) {
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      const double dz = (j < h.d) ? ZsT[j * ldz + z] - cand[c * h.d + j] / h.ls[j] : 0.0;
      r2 += dz * dz;
    }
    const WgVplus f = wg_vplus(kern_eval<KERN>(r2, h.kvar), wk, s, sbad, basez[z]);
    cross = f.cross;
    vs = f.vp * ystd2;
    fl = f.floored ? 1.0 : 0.0;
    if (mask & 4) {
      const double x = IMIQR_U * sqrt(vs);
      ti = zt[ldt + z] + x + log1p(-exp(-2.0 * x));
    }
    if (mask & 8) te = zt[3 * ldt + z] - vs;
  }
  if (wave == 0) {
    crossA[c * lda + z] = cross;
    vplusA[c * lda + z] = vs;
    flagA[c * lda + z] = fl;
    if (blockIdx.x == 0 && lane == 0) sA[c] = s;
  }
  // the pairs: the maximum is exact in any order (block_fold256 over wave 0's terms, -inf elsewhere), the sum of
  // exp(t - maximum) <= 1 runs in chain_wave_sum's order
  double* pp = pairs + (c * gridDim.x + blockIdx.x) * 4;
  const bool in = wave == 0 && z < m;
  if (mask & 4) {                                 // uniform
    const double mx = block_fold256<true>(fold, ti);
    if (wave == 0) {
      const double sm = chain_wave_sum(in ? exp(ti - mx) : 0.0);
      if (lane == 0) {
        pp[0] = mx;
        pp[1] = (mx == -INFINITY) ? 0.0 : sm;
      }
    }
  }
  if (mask & 8) {
    const double mx = block_fold256<true>(fold, te);
    if (wave == 0) {
      const double sm = chain_wave_sum(in ? exp(te - mx) : 0.0);
      if (lane == 0) {
        pp[2] = mx;
        pp[3] = (mx == -INFINITY) ? 0.0 : sm;
      }
    }
  }
}

// One workgroup of 256 per candidate: the workgroups' pairs -> imiqr, eiv (ascending workgroup order: the maximum, then the
// sum of s_w exp(m_w - maximum)); then, criterion by criterion (mask), thread t owning z = t, t + 256, ...: rho^k_z, the
// weight vector rho^k w1 into wv[(vidx * ctot + c) * lda + z] (vidx: the criterion's rank among the requested ones; padding
// and floored z: 0), and this thread's share of sum rho w2, of the value (criteria 0, 1) and of Dz[j] = sum rho w1 G_z (s_zj -
// s_xj) - G_z and the differences recomputed from ZsT.  The shares are summed lanes first (chain_wave_sum), then the four waves
// in order.  zs[(c * 4 + k) * WGW_ZS + ...]: sum rho w2, the score, Dz[j].
// equal: no log-weights were given - omega_z is 1 / M itself, not the table's (the same bits for a finite state: a_z = -mu_z +
// mu_z = 0 exactly; on a NaN state - alpha is NaN then - wipv / wipstd stay at the floor with zero gradients, as
// bobe_gp_wip_grad leaves them, instead of turning NaN through mu_z).
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_wg_weights_w(const double* __restrict__ ZsT, int64_t ldz, int64_t m, int64_t mp,
                                                      const double* __restrict__ cand, Hyper h, double ystd2,
                                                      const double* __restrict__ zt, int64_t ldt, int mask, int equal,
                                                      const double* __restrict__ crossA, const double* __restrict__ vplusA,
                                                      const double* __restrict__ flagA, int64_t lda,
                                                      const double* __restrict__ sA, const double* __restrict__ pairs,
                                                      int nzw, int64_t ctot, double* __restrict__ wv,
                                                      double* __restrict__ zs) {
  __shared__ double red[4][WGW_ZS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c = blockIdx.x;
  crossA += c * lda;
  vplusA += c * lda;
  flagA += c * lda;
  const double s = sA[c];
  const double inv_m = 1.0 / (double)m;
  const double* pp = pairs + c * nzw * 4;
  double lse[2] = {0.0, 0.0};                      // LSE of the IMIQR terms, of the EIV terms (every thread, same bits)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (!(mask & (4 << r))) continue;
    double mx = -INFINITY;
    for (int w = 0; w < nzw; ++w) {
      const double y = pp[w * 4 + 2 * r];
      mx = (y > mx || y != y) ? y : mx;
    }
    double sm = 0.0;
    for (int w = 0; w < nzw; ++w) {
      const double sw = pp[w * 4 + 2 * r + 1];
      sm += (sw == 0.0) ? 0.0 : sw * exp(pp[w * 4 + 2 * r] - mx);
    }
    lse[r] = mx + log(sm);
  }
  double xc[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xc[j] = (j < h.d) ? cand[c * h.d + j] / h.ls[j] : 0.0;
  int vidx = 0;
  for (int k = 0; k < 4; ++k) {
    if (!(mask & (1 << k))) continue;              // uniform
    double* wk = wv + (vidx * ctot + c) * lda;
    ++vidx;
    double s2 = 0.0, val = 0.0, dzs[DCAP];
#pragma unroll
    for (int j = 0; j < DCAP; ++j) dzs[j] = 0.0;
    for (int64_t z = t; z < mp; z += 256) {
      if (z >= m) {
        wk[z] = 0.0;
        continue;
      }
      const double cross = crossA[z], vs = vplusA[z];
      const bool floored = flagA[z] != 0.0;
      const double sr = sqrt(vs);
      double rho;
      if (k == 0) {
        rho = equal ? inv_m : zt[2 * ldt + z];
        val += rho * vs;
      } else if (k == 1) {
        const double om = equal ? inv_m : zt[2 * ldt + z];
        rho = om / (2.0 * sr);
        val += om * sr;
      } else if (k == 2) {
        const double x = IMIQR_U * sr, em = exp(-2.0 * x);
        const double tz = zt[ldt + z] + x + log1p(-em);
        rho = exp(tz - lse[0]) * ((1.0 + em) / (-expm1(-2.0 * x))) * (IMIQR_U / (2.0 * sr));
      } else {
        rho = exp(zt[3 * ldt + z] - vs - lse[1]);
      }
      if (floored) {
        wk[z] = 0.0;
        continue;
      }
      const double w1 = -2.0 * cross / s * ystd2, w2 = (cross * cross) / (s * s) * ystd2;
      const double a = rho * w1;
      wk[z] = a;
      s2 += rho * w2;
      double dz[DCAP];
      double r2 = 0.0;
#pragma unroll
      for (int j = 0; j < DCAP; ++j) {
        dz[j] = (j < h.d) ? ZsT[j * ldz + z] - xc[j] : 0.0;
        r2 += dz[j] * dz[j];
      }
      const double kz = kern_eval<KERN>(r2, h.kvar);
      const double ag = a * kern_grad_factor<KERN>(r2, h.kvar, kz);
#pragma unroll
      for (int j = 0; j < DCAP; ++j) dzs[j] = __builtin_fma(ag, dz[j], dzs[j]);
    }
    __syncthreads();                               // (the previous criterion's readers of red are through)
    {
      const double a = chain_wave_sum(s2), b = chain_wave_sum(val);
      if (lane == 0) {
        red[wave][0] = a;
        red[wave][1] = b;
      }
    }
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      if (j < h.d) {                               // uniform
        const double a = chain_wave_sum(dzs[j]);
        if (lane == 0) red[wave][2 + j] = a;
      }
    }
    __syncthreads();
    if (t < 2 + h.d) {
      double r = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
      if (t == 1 && k == 2) r = lse[0];
      if (t == 1 && k == 3) r = -lse[1];
      zs[(c * 4 + k) * WGW_ZS + t] = r;
    }
  }
}

// the n-side partials of k_wg_rows (nnw of them, nv + 1 rows each) and the z-side sums of k_wg_weights_w -> scores and
// gradients of candidate blockIdx.x, in k_wg_final's order: thread (j = t & 31, part = t >> 5) adds the partials part,
// part + 8, ... of coordinate j, the eight parts are combined in order.  The outputs of criterion k at out.score[k] + c0 + c,
// out.grad[k] + (c0 + c) d (NULL: not written).
__global__ __launch_bounds__(256) void k_wg_final_w(const double* __restrict__ zs, const double* __restrict__ partN, int nnw,
                                                    int nv, int mask, Hyper h, int64_t c0, WgwOut out) {
  __shared__ double acc[8][5][32];
  const int t = threadIdx.x, j = t & 31, part = t >> 5;
  const int64_t c = blockIdx.x;
  const double* pn = partN + c * nnw * (nv + 1) * MAX_D;
  {
    // (all rows of four partials are loaded before any is added: one row after the other, one partial per trip, left this
    // stage waiting on (nv + 1) nnw / 8 load latencies in a row - 73 us at N = 4096 with one criterion.  Each row's sum keeps
    // its order.)
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int nr = nv + 1;
    int w = part;
    for (; w + 24 < nnw; w += 32) {
      double x[4][5];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 5; ++r) x[q][r] = (r < nr) ? pn[((w + 8 * q) * nr + r) * MAX_D + j] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 5; ++r) a[r] += x[q][r];
    }
    for (; w < nnw; w += 8)
#pragma unroll
      for (int r = 0; r < 5; ++r) a[r] += (r < nr) ? pn[(w * nr + r) * MAX_D + j] : 0.0;
#pragma unroll
    for (int r = 0; r < 5; ++r) acc[part][r][j] = a[r];
  }
  __syncthreads();
  if (part != 0) return;
  for (int r = 0; r <= nv; ++r) {                // the totals stay in LDS (column j is this thread's alone): no indexed registers
    double v = acc[0][r][j];
#pragma unroll
    for (int q = 1; q < 8; ++q) v += acc[q][r][j];
    acc[0][r][j] = v;
  }
  const double dsj = (j < h.d) ? -2.0 * acc[0][nv][j] / h.ls[j] : 0.0;
  int vidx = 0;
  for (int k = 0; k < 4; ++k) {
    if (!(mask & (1 << k))) continue;
    const double* zk = zs + (c * 4 + k) * WGW_ZS;
    if (j == 0 && out.score[k]) out.score[k][c0 + c] = zk[1];
    if (j < h.d && out.grad[k]) out.grad[k][(c0 + c) * h.d + j] = (zk[2 + j] - acc[0][vidx][j]) / h.ls[j] + zk[0] * dsj;
    ++vidx;
  }
}

// ---- input gradient of the evidence-variance score for a HANDFUL of candidates (bobe_gp_wip_grad_zvar) --------------------
// zvar = -log T(c) (k_wip_score_zz above) is a function of the r_z alone: with h_c, p_z, E_z and the scaled pair sum T_s as
// there (zvar = -(2 h_c + log T_s)) and
//   G_z = sum_z' r_z' exp(p_z + p_z' + r_z r_z')        (the diagonal included; every exponent <= 0, nothing subtracted)
//   d zvar / dx_j = sum_z rho_z d r_z / dx_j,   rho_z = -2 G_z / T_s,   d r_z / dx_j = w1 d cross_z / dx_j + w2_z d s / dx_j,
//   w1 = y_std / sqrt(s),   w2_z = -r_z / (2 s)
// - the chain above with other weights: wg_front and k_wg_cross_w (mask 1: cross_z and s_c, no log-sum-exp pairs) in front,
// k_wg_rows<., ., 1> and k_wg_final_w (criterion slot 0) behind, and three stages in place of k_wg_weights_w:
//   k_wg_zv_r     per candidate: r_z under k_wip_score_zz::r_of's rules with the "constant" flag, h_c, p_z, E_z
//   k_wg_zv_pair  the hot one, M^2 pairs per candidate: G_z and z's row t_z = sum_z' pair(z, z') of the pair sum
//   k_wg_zv_fold  per candidate: T_s, the score, rho_z, rho w1 into wv and sum rho w2, D_z[j] into zs (k_wg_weights_w's layout)
// "Gradient of where": a z whose r_z was cut to its cap, whose cross_z is not finite, or whose candidate has s_c not > 0, is a
// constant - it keeps its value in T and G and has rho_z = 0.  T_s <= 0 (or NaN): the score is k_wip_score_zz's (+inf, NaN)
// and every rho_z is 0.  No atomics; every sum runs in a fixed order that depends on the candidate and M alone.
constexpr int ZV_T = 256;                   // z' per LDS tile of k_wg_zv_pair (one per thread to load)

// One workgroup of 256 per candidate, thread t owning z = t, t + 256, ... (padding: r = 0, constant, p = 0, E = 0).
__global__ __launch_bounds__(256) void k_wg_zv_r(const double* __restrict__ crossA, int64_t lda,
                                                 const double* __restrict__ sA, const double* __restrict__ basez,
                                                 const double* __restrict__ zt, int64_t ldt, int64_t m, int64_t mp,
                                                 double ystd, double* __restrict__ rA, double* __restrict__ pA,
                                                 double* __restrict__ eA, double* __restrict__ constA,
                                                 double* __restrict__ hA) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  crossA += c * lda;
  rA += c * lda;
  pA += c * lda;
  eA += c * lda;
  constA += c * lda;
  const double* lam = zt + 5 * ldt;
  const double s = sA[c];
  const double scale = (s > 0.0) ? ystd / sqrt(s) : 0.0;
  const bool dead = !(s > 0.0);
  const double ystd2 = ystd * ystd;
  double hm = -INFINITY;
  for (int64_t z = t; z < mp; z += 256) {
    if (z >= m) {
      rA[z] = 0.0;
      constA[z] = 1.0;
      continue;
    }
    const double cross = crossA[z];
    double b = basez[z];
    if (!(b >= NOISE_FLOOR) || b > 1.79769313486231571e308) b = NOISE_FLOOR;
    const double cap = sqrt(b * ystd2);
    double r = cross * scale;
    bool cst = dead || !(fabs(cross) <= 1.79769313486231571e308);
    if (cst) r = 0.0;
    if (r > cap) { r = cap; cst = true; }
    if (r < -cap) { r = -cap; cst = true; }
    rA[z] = r;
    constA[z] = cst ? 1.0 : 0.0;
    const double q = lam[z] + 0.5 * (r * r);
    hm = (q > hm || q != q) ? q : hm;
  }
  hm = block_fold256<true>(red, hm);
  for (int64_t z = t; z < mp; z += 256) {
    const double p = (z < m) ? lam[z] - hm : 0.0;
    pA[z] = p;
    eA[z] = (z < m) ? exp(p) : 0.0;
  }
  if (t == 0) hA[c] = hm;
}

// The pair pass: one workgroup = 64 integration points z (lane) x 4 interleaved quarters of the z' (wave: z' = wave, wave + 4,
// ...), grid (mp / 64, candidates) - a handful of candidates still fills the chip.  The z' pass through LDS in tiles of ZV_T
// (r, p, E of the tile; every lane of a wave reads the same z': a broadcast, no bank conflict), so M is not capped.  A pair
// costs one transcendental: |x| < 1 (x = r_z r_z') takes u = E E' expm1(x) for the pair sum and E E' + u = E E' e^x for G,
// any other pair v = exp(p + p' + x) for G and v - E E' for the pair sum (k_wip_score_zz's pair()).  Every quarter sums its
// z' in ascending order; the quarters are combined as (0 + 1) + (2 + 3).  Padding lanes write 0.
__global__ __launch_bounds__(256) void k_wg_zv_pair(const double* __restrict__ rA, const double* __restrict__ pA,
                                                    const double* __restrict__ eA, int64_t lda, int64_t m,
                                                    double* __restrict__ tA, double* __restrict__ gA) {
  __shared__ double rs[ZV_T], ps[ZV_T], es[ZV_T], redt[4][64], redg[4][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c = blockIdx.y, z = (int64_t)blockIdx.x * 64 + lane;
  rA += c * lda;
  pA += c * lda;
  eA += c * lda;
  const bool in = z < m;
  const double r = in ? rA[z] : 0.0, p = in ? pA[z] : 0.0, e = in ? eA[z] : 0.0;
  double tz = 0.0, gz = 0.0;
  for (int64_t j0 = 0; j0 < m; j0 += ZV_T) {
    __syncthreads();
    const int zn = (m - j0 < ZV_T) ? (int)(m - j0) : ZV_T;
    if (t < zn) {
      rs[t] = rA[j0 + t];
      ps[t] = pA[j0 + t];
      es[t] = eA[j0 + t];
    }
    __syncthreads();
    for (int k = wave; k < zn; k += 4) {            // (ZV_T is a multiple of 4: k and j0 + k fall into the same quarter)
      const double rp = rs[k], x = r * rp, ee = e * es[k];
      double pr, ex;
      if (fabs(x) < 1.0) {
        pr = ee * expm1(x);
        ex = ee + pr;
      } else {
        ex = exp((p + ps[k]) + x);
        pr = ex - ee;
      }
      tz += pr;
      gz = __builtin_fma(rp, ex, gz);
    }
  }
  redt[wave][lane] = tz;
  redg[wave][lane] = gz;
  __syncthreads();
  if (wave == 0) {
    tA[c * lda + z] = in ? (redt[0][lane] + redt[1][lane]) + (redt[2][lane] + redt[3][lane]) : 0.0;
    gA[c * lda + z] = in ? (redg[0][lane] + redg[1][lane]) + (redg[2][lane] + redg[3][lane]) : 0.0;
  }
}

// One workgroup of 256 per candidate, thread t owning z = t, t + 256, ... as in k_wg_weights_w, whose sums' order (the
// thread's own z ascending, lanes by chain_wave_sum, then the four waves) and whose outputs it keeps: T_s = sum_z t_z, the
// score (k_wip_score_zz's last line), rho_z, the weight vector rho w1 into wv[c * lda + z] (constants and padding: 0) and sum
// rho w2, the score, Dz[j] = sum rho w1 G_z (s_zj - s_xj) into zs[(c * 4 + 0) * WGW_ZS + ...]: criterion slot 0 of k_wg_final_w.
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_wg_zv_fold(const double* __restrict__ ZsT, int64_t ldz, int64_t m, int64_t mp,
                                                    const double* __restrict__ cand, Hyper h, double ystd,
                                                    const double* __restrict__ rA, const double* __restrict__ constA,
                                                    const double* __restrict__ tA, const double* __restrict__ gA,
                                                    int64_t lda, const double* __restrict__ sA,
                                                    const double* __restrict__ hA, double* __restrict__ wv,
                                                    double* __restrict__ zs) {
  __shared__ double red[4][WGW_ZS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c = blockIdx.x;
  rA += c * lda;
  constA += c * lda;
  tA += c * lda;
  gA += c * lda;
  double* wk = wv + c * lda;
  double tot = 0.0;
  for (int64_t z = t; z < m; z += 256) tot += tA[z];
  tot = chain_wave_sum(tot);
  if (lane == 0) red[wave][0] = tot;
  __syncthreads();
  tot = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
  const bool ok = tot > 0.0;
  const double s = sA[c];
  const double w1 = (s > 0.0) ? ystd / sqrt(s) : 0.0;
  double xc[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xc[j] = (j < h.d) ? cand[c * h.d + j] / h.ls[j] : 0.0;
  double s2 = 0.0, dzs[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) dzs[j] = 0.0;
  for (int64_t z = t; z < mp; z += 256) {
    if (z >= m || !ok || constA[z] != 0.0) {
      wk[z] = 0.0;
      continue;
    }
    const double rho = -2.0 * gA[z] / tot;
    const double a = rho * w1;
    wk[z] = a;
    s2 += rho * (-rA[z] / (2.0 * s));
    double dz[DCAP];
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      dz[j] = (j < h.d) ? ZsT[j * ldz + z] - xc[j] : 0.0;
      r2 += dz[j] * dz[j];
    }
    const double kz = kern_eval<KERN>(r2, h.kvar);
    const double ag = a * kern_grad_factor<KERN>(r2, h.kvar, kz);
#pragma unroll
    for (int j = 0; j < DCAP; ++j) dzs[j] = __builtin_fma(ag, dz[j], dzs[j]);
  }
  __syncthreads();                                 // (the readers of red[.][0] are through)
  {
    const double a = chain_wave_sum(s2);
    if (lane == 0) red[wave][0] = a;
  }
#pragma unroll
  for (int j = 0; j < DCAP; ++j) {
    if (j < h.d) {                                 // uniform
      const double a = chain_wave_sum(dzs[j]);
      if (lane == 0) red[wave][2 + j] = a;
    }
  }
  __syncthreads();
  if (t < 2 + h.d && t != 1) zs[c * 4 * WGW_ZS + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  if (t == 1) zs[c * 4 * WGW_ZS + 1] = ok ? -(2.0 * hA[c] + log(tot)) : ((tot <= 0.0) ? INFINITY : tot);
}

}  // namespace bobe
