// Kernels of the total variance of the evidence estimate (bobe_gp_evidence_moments; gfx950).  Included by gp_criteria.hip only,
// after criteria_kernels.hpp (block_fold256, the per-z table's rows).
//
// With the per-z table's lambda row (k_wip_zterms: lambda_z = l_z + mu_z + b_z / 2 - log E[Z], omega_z = exp(lambda_z)) and
// the posterior covariance S_zz' of two integration points in physical units (S_zz = b_z),
//   Var Z = E[Z]^2 T0,   T0 = sum_z sum_z' omega_z omega_z' expm1(S_zz')      (all M^2 ordered pairs),
// and the entry returns log T0.  S_zz' <= (b_z + b_z') / 2 under the Cauchy-Schwarz cap, so with h = max_z (lambda_z + b_z / 2),
// p_z = lambda_z - h and E_z = exp(p_z) no pair exponent p_z + p_z' + S_zz' is above 0: the pair term is k_wip_score_zz's
// (|S| < 1: E E' expm1(S); else exp(p + p' + S) - E E') and log T0 = 2 h + log sum.  One transcendental per pair.
//   k_evid_h      h, and the rows p, E, b padded to Mp                                         1 workgroup
//   k_evid_pairs  one 128 x 128 tile of the lower triangle of the pair matrix per workgroup     nt (nt + 1) / 2 workgroups
//   k_evid_fold   the tiles' sums in ascending order, log T0                                    1 workgroup
// Every sum runs in a fixed order that depends on M alone; no atomics, nothing is stored per pair.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

constexpr int EVID_ROWS = 3;       // the rows of k_evid_h's table: p, E, b (ld = Mp), h behind them

// ev [EVID_ROWS x ldm] + h, ONE workgroup of 256 (thread t owns z = t, t + 256, ...).  b_z = y_std^2 base_z under
// k_wip_zterms' floor, h = max_z (lambda_z + b_z / 2) with a NaN propagated as block_fold256<true> does; padding: p = E = b = 0.
static __global__ __launch_bounds__(256) void k_evid_h(const double* __restrict__ lam, const double* __restrict__ basez,
                                                       int64_t m, int64_t ldm, double ystd, double* __restrict__ ev) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double* pr = ev;
  double* er = ev + ldm;
  double* br = ev + 2 * ldm;
  const double ystd2 = ystd * ystd;
  double hm = -INFINITY;
  for (int64_t z = t; z < m; z += 256) {
    double b = basez[z];
    if (!(b >= NOISE_FLOOR) || b > 1.79769313486231571e308) b = NOISE_FLOOR;
    b *= ystd2;
    br[z] = b;
    const double q = lam[z] + 0.5 * b;
    hm = (q > hm || q != q) ? q : hm;
  }
  hm = block_fold256<true>(red, hm);
  for (int64_t z = t; z < ldm; z += 256) {
    const bool in = z < m;
    const double p = in ? lam[z] - hm : 0.0;
    pr[z] = p;
    er[z] = in ? exp(p) : 0.0;
    if (!in) br[z] = 0.0;
  }
  if (t == 0) ev[EVID_ROWS * ldm] = hm;
}

static_assert(2 * (MAX_D + 2) * TILE <= GEMM_SMEM_DOUBLES,
              "k_evid_pairs stages d + 2 rows of 128 (coordinates, p, b) for the tile's rows and for its columns in the product's LDS");

// ---- parts[tile] = sum over the tile's pairs (z, z') with z' <= z of  w E_z E_z' pair(S_zz'),  w = 2 (z' < z) or 1 (z' = z) --
// A sibling of k_sigma_tiles (posterior_kernels.hpp): one workgroup = tile (ti, tj <= ti) of the lower triangle, rows
// z = 128 ti + [0, 128), columns z' = 128 tj + [0, 128); V_z . V_z' on the sweep's 128-tile core over the whole padded K = Np
// (V = V_Z, Np x ldv: its padded rows are 0).  The epilogue stages the scaled coordinates of the rows and of the columns
// (ZsT, d x 128 each) and their p and b in the LDS the product is done with, evaluates k(z, z') as the assembly does (fma
// over the dimensions) and forms S = y_std^2 (k - V.V) for z' != z: non-finite -> 0, |S| capped at sqrt(b_z b_z'); S_zz = b_z
// from the table.  Inside a diagonal tile only z' <= z is taken.  Rows / columns >= m are not taken.
// Order: a lane adds its elements in the fragment order (i, j, r); the 64 lanes of a wave fold in one fixed tree (offsets
// 32, 16, .. 1); the four waves are added in order.
template <int KERN>
__global__ __launch_bounds__(256, 2) void k_evid_pairs(const double* __restrict__ V, int64_t ldv, int64_t kend,
                                                       const double* __restrict__ ZsT, int64_t ldz,
                                                       const double* __restrict__ ev, int64_t ldm, int64_t m, Hyper h,
                                                       double ystd, double* __restrict__ parts) {
  extern __shared__ double smem[];
  int ti, tj;
  tri_decode((int)blockIdx.x, ti, tj);
  v4d acc[4][4];
  acc_zero(acc);
  tile_gemm<true, RC, RC, TILE>(acc, V, ldv, (int64_t)ti * TILE, V, ldv, (int64_t)tj * TILE, 0, kend, smem);
  const int64_t gi0 = (int64_t)ti * TILE, gj0 = (int64_t)tj * TILE;
  double* qa = smem;                             // [d][128] rows, then their p and b
  double* qb = smem + (MAX_D + 2) * TILE;        // [d][128] columns, then their p and b
  double* pa = qa + MAX_D * TILE;
  double* ba = pa + TILE;
  double* pb = qb + MAX_D * TILE;
  double* bb = pb + TILE;
  __syncthreads();                               // (the product's last LDS reads are done)
  for (int e = threadIdx.x; e < h.d * TILE; e += 256) {
    const int j = e / TILE, r = e % TILE;
    qa[j * TILE + r] = ZsT[(int64_t)j * ldz + gi0 + r];
    qb[j * TILE + r] = ZsT[(int64_t)j * ldz + gj0 + r];
  }
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    pa[r] = ev[gi0 + r];
    ba[r] = ev[2 * ldm + gi0 + r];
  } else {
    const int r = threadIdx.x - TILE;
    pb[r] = ev[gj0 + r];
    bb[r] = ev[2 * ldm + gj0 + r];
  }
  __syncthreads();
  const bool on_diag = ti == tj;
  const double ystd2 = ystd * ystd;
  const double* er = ev + ldm;
  double ecol[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ecol[j] = er[gj0 + acc_col(j)];
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double erow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) erow[r] = er[gi0 + acc_row(i, r)];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = acc_row(i, r), cl = acc_col(j);
        const int64_t gi = gi0 + rl, gj = gj0 + cl;
        if (gi >= m || gj >= m || (on_diag && cl > rl)) continue;
        const double bi = ba[rl];
        double s, wgt;
        if (gi == gj) {
          s = bi;
          wgt = 1.0;
        } else {
          double r2 = 0.0;
          for (int jd = 0; jd < h.d; ++jd) {
            const double df = qa[jd * TILE + rl] - qb[jd * TILE + cl];
            r2 = __builtin_fma(df, df, r2);
          }
          s = ystd2 * (kern_eval<KERN>(r2, h.kvar) - acc[i][j][r]);
          if (!(fabs(s) <= 1.79769313486231571e308)) s = 0.0;
          const double bij = bi * bb[cl];
          if (s * s > bij) s = copysign(sqrt(bij), s);
          wgt = 2.0;
        }
        const double ee = erow[r] * ecol[j];
        const double pp = pa[rl] + pb[cl];
        const double term = (fabs(s) < 1.0) ? ee * expm1(s) : exp(pp + s) - ee;
        sum += wgt * term;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  __syncthreads();                               // (every wave is through with the staged rows)
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

// log T0 = 2 h + log sum_tiles parts (thread t adds tiles t, t + 256, ... ascending, then block_fold256); a sum <= 0
// (underflown or rounding-negative) gives -inf, a NaN stays.  res[0] = log T0; res[1] = *log_ez, the table's log E[Z], so that
// one copy brings both home.  ONE workgroup of 256.
static __global__ __launch_bounds__(256) void k_evid_fold(const double* __restrict__ parts, int64_t ntiles,
                                                          const double* __restrict__ hp, const double* __restrict__ log_ez,
                                                          double* __restrict__ res) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < ntiles; k += 256) s += parts[k];
  s = block_fold256<false>(red, s);
  if (threadIdx.x == 0) {
    res[0] = (s > 0.0) ? 2.0 * hp[0] + log(s) : ((s <= 0.0) ? -INFINITY : s);
    res[1] = log_ez[0];
  }
}

}  // namespace bobe
