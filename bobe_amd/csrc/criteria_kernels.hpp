// Kernels of the importance-weighted scoring pass (bobe_gp_wip_sweep_w, bobe_gp_wip_select_batch_w; gfx950).  Included by
// gp_criteria.hip only.
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

namespace bobe {

constexpr double IMIQR_U = 0.6744897501960817;    // Phi^-1(3/4)
static_assert(ZTERM_ROWS == 5, "k_wip_zterms / k_wip_score_w address the table's rows mu, a, omega, e, l by number");

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
// A later stage of the batch selection calls it with first = 0 on its downdated base_z: mu, a, omega stay.
static __global__ __launch_bounds__(256) void k_wip_zterms(const double* __restrict__ part, int64_t ldp, int nrb, int64_t m,
                                                           double ystd, const double* __restrict__ logw,
                                                           const double* __restrict__ basez, double* __restrict__ zt,
                                                           int64_t ldt, int first, double* __restrict__ log_s) {
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

}  // namespace bobe
