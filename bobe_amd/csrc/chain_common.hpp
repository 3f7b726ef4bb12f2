// What the chain kernels of two translation units share (gfx950): the classifier gate's per-point arithmetic and the homes
// of a chain workgroup's training rows.  Included by consumer_kernels.hpp (k_hmc_run, k_nuts_run, k_rwalk, k_gate) and by
// paths_kernels.hpp (k_paths_hmc_run).  Inline device functions and constants only: no kernel lives here.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

// ---- the classifier gate of GPwithClassifier (clf_gp.py:173-205) ---------------------------------------------------
// One 256-thread workgroup per point, ONE summation order everywhere (the batch kernel and the HMC / random-walk kernels
// share gate_partial / gate_combine): gate_partial's per-thread value, lanes by chain_wave_sum, then the four waves
// ((r0 + r1) + r2) + r3 in gate_combine.  A point near the boundary is therefore classified the same way by every entry
// point.  x: the point's d raw (unit-cube) coordinates, readable by every thread.
//   GATE_SVM        (clf.py:188-213, by DIRECT DIFFERENCES, as the reference computes it: diff = support_vectors - x;
//                   norm_sq = sum_j diff_j^2; decision = sum_i dual_i exp(-gamma norm_sq_i) + intercept): thread t adds
//                   the vectors t, t + 256, ... in ascending order; + intercept after the waves.
//   GATE_ELLIPSOID  (clf.py:377-412): thread t < d computes u_t = sum_{i >= t} L[i][t] (x_i - mu_i) in ascending i and
//                   contributes u_t^2 (md2 = |L^T diff|^2 = diff^T L L^T diff); logit = -alpha md2 + beta after the waves.
template <int DCAP>
__device__ __forceinline__ double gate_partial(const Gate& gt, const double* x, int d, int t) {
  double s = 0.0;
  if (gt.kind == GATE_ELLIPSOID) {
    if (t < d) {
      double u = 0.0;
      for (int i = t; i < d; ++i) u = fma(gt.Lt[i * d + t], x[i] - gt.mu[i], u);
      s = u * u;
    }
    return chain_wave_sum(s);
  }
  double xr[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xr[j] = (j < d) ? x[j] : 0.0;
  for (int i = t; i < gt.n_sv; i += 256) {
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      if (j < d) {
        const double df = gt.svT[j * gt.ld + i] - xr[j];
        r2 += df * df;
      }
    }
    s += gt.dual[i] * exp(-gt.gamma * r2);
  }
  return chain_wave_sum(s);
}
// red[4]: the four waves' sums (written by lane 0 of each wave, followed by a barrier) -> the decision value (the SVM's
// decision function, the ellipsoid's logit)
__device__ __forceinline__ double gate_combine(const Gate& gt, const double* red) {
  const double r = ((red[0] + red[1]) + red[2]) + red[3];
  if (gt.kind == GATE_ELLIPSOID) return fma(-gt.alpha, r, gt.beta);
  return r + gt.intercept;
}
// the classifier's probability: svm_predict_proba (clf.py:210-213) or sigmoid(logit) (clf.py:134-136)
__device__ __forceinline__ double gate_proba(const Gate& gt, double decision) {
  if (gt.kind == GATE_ELLIPSOID) return 1.0 / (1.0 + exp(-decision));
  return (decision >= 0.0) ? 1.0 : 0.0;
}
// ... against the probability threshold (clf_gp.py:179): NaN decisions are infeasible (a NaN probability compares false)
__device__ __forceinline__ bool gate_feasible(const Gate& gt, double decision) {
  return gate_proba(gt, decision) >= gt.threshold;
}

// ---- the homes of a chain workgroup's training rows -------------------------------------------------------------------
// Training points a thread of a 256-thread chain workgroup keeps in registers for the whole launch (a launch is hundreds
// of leapfrog / random-walk steps over the same points): 256 x RESIDENT rows, the rest is streamed from L2 every step.
// (One wave per SIMD: the 512 unified registers of a lane hold them; chosen as the largest counts without scratch spills.)
template <int DCAP>
struct ChainRows {
  static constexpr int HMC = DCAP == 8 ? 14 : (DCAP == 16 ? 6 : 2);
  static constexpr int WALK = DCAP == 8 ? 16 : (DCAP == 16 ? 8 : 4);
  static constexpr int STREAM = DCAP == 32 ? 1 : 2;      // streamed rows in flight per thread
  static constexpr int NUTS = DCAP == 8 ? 10 : (DCAP == 16 ? 3 : 1);   // (k_nuts_run: its tree needs ~50 more registers)
  static constexpr int PATHS = DCAP == 8 ? 14 : (DCAP == 16 ? 6 : 1);  // (k_paths_hmc_run: its resource note)
};
// ... and as many more as the CU's LDS holds next to them: groups of 256 rows of d coordinates + alpha, [d + 1][rows]
// (a lane reads consecutive doubles: no bank conflicts).  Host side: the group count for n points and `resident` register rows.
constexpr int CHAIN_LDS_BYTES = 148 * 1024;                            // (of 160 KB: the kernels' static arrays stay below 10 KB)
inline int chain_lds_groups(int64_t n, int d, int resident, int bytes = CHAIN_LDS_BYTES) {
  const int64_t left = n - 256 * (int64_t)resident;
  if (left <= 0) return 0;
  const int64_t cap = bytes / (8 * (int64_t)(d + 1)) / 256;
  const int64_t want = (left + 255) / 256;
  return (int)(want < cap ? want : cap);
}

}  // namespace bobe
