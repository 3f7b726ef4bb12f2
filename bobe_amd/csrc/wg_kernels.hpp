// What the two few-candidate gradient chains share on the device; gfx950.  Included by gp_sweep.hip (bobe_gp_wip_grad:
// k_wg_cross -> k_wg_rows<., ., 2> -> k_wg_final, sweep_kernels.hpp) and by gp_criteria.hip (bobe_gp_wip_grad_w /
// bobe_gp_wip_grad_zvar: k_wg_cross_w -> k_wg_weights_w or k_wg_zv_* -> k_wg_rows<., ., nv> -> k_wg_final_w,
// criteria_kernels.hpp); both run behind bobe_gp::wg_front.
//   wg_cross_front, wg_vplus   the front of the two cross kernels: s_c, this lane's (VZ^T v)_z, the floored fantasy variance
//   k_wg_rows                  the n-side sums for NV weight vectors in one read of W_Z
// Every sum runs in a fixed order.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

// The front of a cross kernel - one workgroup = 64 integration points (lane) x 4 interleaved quarters of the training points
// (wave): v = L^-1 k_c into kcs[n] with its sum of squares, s = kself - v.v (returned), then the quarter's share of
// (VZ^T v)_z, eight rows in flight, and wk = the four quarters' sum for this lane's z.  red[4], redz[4][64]: the kernel's LDS.
__device__ __forceinline__ double wg_cross_front(const double* __restrict__ v, int64_t n, const double* __restrict__ VZ,
                                                 int64_t ldw, int64_t z, double kself, double* kcs, double* red,
                                                 double (*redz)[64], double& wk) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sq = 0.0;
  for (int64_t i = t; i < n; i += 256) {
    const double vi = v[i];
    kcs[i] = vi;
    sq += vi * vi;
  }
  sq = wave_sum(sq);
  if (lane == 0) red[wave] = sq;
  __syncthreads();
  const double s = kself - ((red[0] + red[1]) + (red[2] + red[3]));
  double acc = 0.0;
  {
    const double* wp = VZ + z;
    int64_t i = wave;
    for (; i + 28 < n; i += 32) {                 // eight rows in flight per thread
      double w8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) w8[q] = wp[(i + 4 * q) * ldw];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = __builtin_fma(w8[q], kcs[i + 4 * q], acc);
    }
    for (; i < n; i += 4) acc = __builtin_fma(wp[i * ldw], kcs[i], acc);
  }
  redz[wave][lane] = acc;
  __syncthreads();
  wk = (redz[0][lane] + redz[1][lane]) + (redz[2][lane] + redz[3][lane]);
  return s;
}

// cross_z = k_z - wk and the fantasy variance v+_z = base_z - cross^2 / s, floored at NOISE_FLOOR (floored: s is not >= 0 -
// sbad -, v+ is NaN or below the floor; a floored z is a constant of the gradient).  (Returned by value: with reference
// outputs k_wg_cross<matern, .> took 4 - 6 VGPRs more and lost a wave of occupancy at d cap 16.)
struct WgVplus {
  double cross, vp;
  bool floored;
};
__device__ __forceinline__ WgVplus wg_vplus(double kz, double wk, double s, bool sbad, double bz) {
  const double cross = kz - wk;
  double vp = bz - (cross * cross) / s;
  bool floored = sbad;
  if (vp != vp) floored = true;
  if (vp < NOISE_FLOOR) floored = true;
  if (floored) vp = NOISE_FLOOR;
  return {cross, vp, floored};
}

// one workgroup = WG_ROWS training points, one per wave; lanes run over the integration points, and W_Z's row is read once
// whatever NV (1 .. 4 weight vectors, wv[(r * ctot + c) * lda + z]) is.  partN[(c * gridDim.x + blockIdx.x) * (NV + 1) * MAX_D +
// r * MAX_D + j]: r < NV the n-side sum Q_r[j] = sum_n q_r[n] T[j][n], q_r = W_Z wv_r; r = NV ds[j] = sum_n u_n T[j][n].
// (Sixteen per wave - 64 per workgroup - left a refinement step at N = 400 on seven CUs for 41 of its 90 us.)
constexpr int WG_ROWS = 4;
template <int KERN, int DCAP, int NV>
__global__ __launch_bounds__(256) void k_wg_rows(const double* __restrict__ XsT, int64_t ldx, int64_t n, int64_t np,
                                                 const double* __restrict__ cand, Hyper h,
                                                 const double* __restrict__ W, int64_t ldw, int64_t mp,
                                                 const double* __restrict__ wv, int64_t lda, int64_t ctot,
                                                 const double* __restrict__ u, double* __restrict__ partN) {
  __shared__ double red[4][NV + 1][DCAP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c = blockIdx.y;
  u += c * np;
  const double xl = (lane < h.d) ? cand[c * h.d + lane] / h.ls[lane] : 0.0;      // this lane's coordinate (lane = j)
  double xc[DCAP];                                                                 // the candidate, scaled (every lane)
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xc[j] = (j < h.d) ? cand[c * h.d + j] / h.ls[j] : 0.0;
  double aq[NV], au = 0.0;
#pragma unroll
  for (int r = 0; r < NV; ++r) aq[r] = 0.0;
  const int64_t i = (int64_t)blockIdx.x * WG_ROWS + wave;
  if (i < n) {                                    // uniform per wave
    double q[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) q[r] = 0.0;
    for (int64_t z = lane; z < mp; z += 64) {
      const double w = W[i * ldw + z];
#pragma unroll
      for (int r = 0; r < NV; ++r) q[r] = __builtin_fma(wv[(r * ctot + c) * lda + z], w, q[r]);
    }
#pragma unroll
    for (int r = 0; r < NV; ++r) q[r] = chain_wave_sum(q[r]);
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      const double df = (j < h.d) ? XsT[j * ldx + i] - xc[j] : 0.0;
      r2 += df * df;
    }
    const double kv = kern_eval<KERN>(r2, h.kvar);
    const double tj = (lane < h.d) ? kern_grad_factor<KERN>(r2, h.kvar, kv) * (XsT[lane * ldx + i] - xl) : 0.0;
#pragma unroll
    for (int r = 0; r < NV; ++r) aq[r] = __builtin_fma(q[r], tj, aq[r]);
    au = __builtin_fma(u[i], tj, au);
  }
  if (lane < DCAP) {
#pragma unroll
    for (int r = 0; r < NV; ++r) red[wave][r][lane] = aq[r];
    red[wave][NV][lane] = au;
  }
  __syncthreads();
  if (t < (NV + 1) * DCAP) {
    const int k = t / DCAP, j = t % DCAP;
    partN[(c * gridDim.x + blockIdx.x) * (NV + 1) * MAX_D + k * MAX_D + j] =
        (red[0][k][j] + red[1][k][j]) + (red[2][k][j] + red[3][k][j]);
  }
}

}  // namespace bobe
