// Kernels of the one-sweep batch selection (bobe_gp_wip_select_batch; gfx950).  Included by gp_batch.hip only.
//
// WIPV / WIPStd read the design points only.  Appending the pick c* at its believed mean is therefore a rank-one change of
// everything the scorer (k_wip_score) reads.  With s* = s_{c*}, the pick's noise-included posterior variance, and
//     u(.) = (k(., c*) - V(.)^T v* - sum_{i<j} u_i(.) u_i(c*)) / sqrt(s*),        v* = V[:, c*],
// the state after pick j is crossT[z][c] += u(z) u(c), base_z -= u(z)^2, s_c -= u(c)^2: what a sweep on the (N+j)-point
// believer surrogate computes, without its factorisation, triangular product and K(X, C) assembly.
// A later stage: k_batch_gather -> k_gemv_t_part (V_C^T v*, V_Z^T v*: kernels_common.hpp, partial sums per row block) ->
// k_batch_u (candidates, integration points) -> k_batch_rank1 -> k_wip_score -> k_argmin_masked.  Every thread owns a
// column (candidate or integration point), so V, crossT and the u rows are read coalesced; every sum runs in a fixed order:
// same state, same bits.  The previous pick is read from device memory, so the stages queue up without a host round trip.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

constexpr int BATCH_MAX = 64;                 // picks per call (bobe_gp.h)
constexpr int BATCH_PIN = BATCH_MAX + MAX_D;  // doubles of the per-stage pick record (below)

// The pick's record for one stage.  p = *pick (the previous stage's argmin):
//   vstar[n] = V[n][p] (n < np);  pin[0] = s_p;  pin[1 + i] = u_i(p), i < nprev;  pin[BATCH_MAX + j] = scaled coordinate j of p.
// A copy, because k_batch_u overwrites s_p while other threads still need it.  grid ceil(np / 256).
static __global__ __launch_bounds__(256) void k_batch_gather(const double* __restrict__ V, int64_t ldv, int64_t np,
                                                             const double* __restrict__ CsT, int64_t ldc, int d,
                                                             const double* __restrict__ sc, const double* __restrict__ U,
                                                             int64_t ldu, int nprev, const int64_t* __restrict__ pick,
                                                             double* __restrict__ vstar, double* __restrict__ pin) {
  const int64_t p = *pick;
  const int t = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * 256 + t;
  if (n < np) vstar[n] = V[n * ldv + p];
  if (blockIdx.x == 0) {
    if (t == 0) pin[0] = sc[p];
    else if (t <= nprev) pin[t] = U[(int64_t)(t - 1) * ldu + p];
    if (t >= BATCH_MAX && t < BATCH_MAX + d) pin[t] = CsT[(int64_t)(t - BATCH_MAX) * ldc + p];
  }
}

// u of the stage for the columns of one side (candidates: XT = CsT, sdown = s_c; integration points: XT = ZsT, sdown =
// base_z) and that side's downdate sdown[c] -= u(c)^2.  part: k_gemv_t_part's partial sums of V^T v* [nrb x ldp], added up
// in k_colsum_parts' order (row block 0 first); Uprev [nprev x ldu]: the side's earlier u rows.  Padding columns (c >= nvalid)
// get u = 0.  grid ceil(npad / 256).
static __global__ __launch_bounds__(256) void k_batch_u(const double* __restrict__ part, int64_t ldp, int nrb,
                                                        const double* __restrict__ XT, int64_t ldc, int64_t nvalid,
                                                        int64_t npad, Hyper h, const double* __restrict__ pin,
                                                        const double* __restrict__ Uprev, int64_t ldu, int nprev,
                                                        double* __restrict__ urow, double* __restrict__ sdown) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= npad) return;
  if (c >= nvalid) {
    urow[c] = 0.0;
    return;
  }
  double r2 = 0.0;
  for (int j = 0; j < h.d; ++j) {
    const double df = XT[(int64_t)j * ldc + c] - pin[BATCH_MAX + j];
    r2 += df * df;
  }
  const double kv = h.kern == 0 ? kern_eval<0>(r2, h.kvar) : kern_eval<1>(r2, h.kvar);
  double q = 0.0;
  for (int rb = 0; rb < nrb; ++rb) q += part[(int64_t)rb * ldp + c];
  double e = 0.0;
  for (int i = 0; i < nprev; ++i) e += Uprev[(int64_t)i * ldu + c] * pin[1 + i];
  const double u = ((kv - q) - e) / sqrt(pin[0]);
  urow[c] = u;
  sdown[c] -= u * u;
}

// crossT[z][c] += uz[z] uc[c] for z < nz, c < ncols: a thread owns a column and walks 16 rows.  grid (ceil(ncols / 256), nz / 16)
// (nz is a multiple of 128).
static __global__ __launch_bounds__(256) void k_batch_rank1(double* __restrict__ crossT, int64_t ldx, int64_t ncols,
                                                            const double* __restrict__ uz, const double* __restrict__ uc) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncols) return;
  const double ucv = uc[c];
  const int64_t z0 = (int64_t)blockIdx.y * 16;
  double* col = crossT + z0 * ldx + c;
  double x[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) x[k] = col[(int64_t)k * ldx];
#pragma unroll
  for (int k = 0; k < 16; ++k) col[(int64_t)k * ldx] = x[k] + uz[z0 + k] * ucv;
}

// k_argmin (sweep_kernels.hpp: first occurrence, NaN counts as minimal) over the entries whose index is not among
// picks[0, npicked); the winner goes to picks[npicked] / best_val.  One workgroup of 1024.
static __global__ __launch_bounds__(1024) void k_argmin_masked(const double* __restrict__ v, int64_t n, int64_t* picks,
                                                               int npicked, double* __restrict__ best_val) {
  __shared__ double sv[1024];
  __shared__ int64_t si[1024];
  __shared__ int64_t taken[BATCH_MAX];
  if ((int)threadIdx.x < npicked) taken[threadIdx.x] = picks[threadIdx.x];
  __syncthreads();
  double bv = 0.0;
  int64_t bi = -1;
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    bool masked = false;
    for (int k = 0; k < npicked; ++k) masked |= (taken[k] == i);
    if (masked) continue;
    const double x = v[i];
    const bool xnan = (x != x);
    const bool bnan = (bi >= 0) && (bv != bv);
    if (bi < 0 || (!bnan && (xnan || x < bv))) {
      bv = x;
      bi = i;
    }
  }
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double x = sv[threadIdx.x + o];
      const int64_t xi = si[threadIdx.x + o];
      const double b = sv[threadIdx.x];
      const int64_t bi2 = si[threadIdx.x];
      bool take = false;
      if (xi >= 0) {
        if (bi2 < 0) take = true;
        else {
          const bool xnan = (x != x), bnan = (b != b);
          if (xnan && bnan) take = xi < bi2;
          else if (xnan) take = true;
          else if (bnan) take = false;
          else take = (x < b) || (x == b && xi < bi2);
        }
      }
      if (take) {
        sv[threadIdx.x] = x;
        si[threadIdx.x] = xi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *best_val = sv[0];
    picks[npicked] = si[0];
  }
}

}  // namespace bobe
