// Kernels of the pathwise posterior draws of the surrogate (bobe_gp_paths_*; gfx950): the random arrays of a path set, the
// random-Fourier-feature assembly, the right-hand sides of the conditioning solve and the tile product that evaluates S
// paths at a chunk of query points (values, or a per-path running maximum).  Included by gp_paths.hip only.
#pragma once
#include "chain_common.hpp"

namespace bobe {

constexpr double PATHS_TWO_PI = 6.283185307179586;
constexpr double PATHS_INV_TWO_PI = 0.15915494309189535;

// ---- the random arrays of a path set ----------------------------------------------------------------------------------------
// Contract of the device's draws (what a caller replays to reproduce a set; tests/paths_restatement.py does).  With mix =
// hmc_mix64, u01 = hmc_u01 and the normal of k_draw_normals (posterior_kernels.hpp)
//   normal(sd, r, c) = sqrt(-2 log u01(mix(key + 2 c))) cos(2 pi u01(mix(key + 2 c + 1))),   key = mix(sd ^ mix(r)),
// every array has a sub-stream of its own, sd_a = mix(seed ^ mix(PATHS_STREAM + a)):
//   a = 0   g[j][k]   = normal(sd_0, j, k)                       (F x d)
//   a = 1   c_j       = sum_{k < 5} normal(sd_1, j, k)^2          (chi^2 with 5 degrees of freedom, summed k = 0 .. 4 in order)
//           u[j][k]   = g[j][k]                       (RBF),      g[j][k] sqrt(5 / c_j)   (Matern-5/2: multivariate Student-t, nu = 5)
//   a = 2   phase[j]  = 2 pi u01(mix(mix(sd_2 ^ mix(j))))         (F)
//   a = 3   w[s][j]   = normal(sd_3, s, j)                        (S x F)
//   a = 4   eps[s][n] = sqrt(noise) normal(sd_4, s, n)            (S x N)
// All integer arithmetic is modulo 2^64.  An entry depends on (seed, array, row, column) alone - not on the other sizes or
// the launch - so the same seed gives the same bits.
constexpr unsigned long long PATHS_STREAM = 0x7061746873ull;     // "paths"
__device__ __forceinline__ unsigned long long paths_sub_seed(unsigned long long seed, int a) {
  return hmc_mix64(seed ^ hmc_mix64(PATHS_STREAM + (unsigned long long)a));
}
__device__ __forceinline__ double paths_normal(unsigned long long sd, unsigned long long r, unsigned long long c) {
  const unsigned long long key = hmc_mix64(sd ^ hmc_mix64(r));
  const double a = hmc_u01(hmc_mix64(key + 2ull * c));
  const double b = hmc_u01(hmc_mix64(key + 2ull * c + 1ull));
  return sqrt(-2.0 * log(a)) * cos(PATHS_TWO_PI * b);
}

// out[r * cols + c] = scale * normal(sd_a, r, c)          (w: a = 3, scale 1; eps: a = 4, scale sqrt(noise))
// grid (rows, ceil(cols / 256))
__global__ void k_paths_draw_normals(double* __restrict__ out, int64_t rows, int64_t cols, unsigned long long seed, int a,
                                     double scale) {
  const int64_t c = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.x;
  if (r >= rows || c >= cols) return;
  out[r * cols + c] = scale * paths_normal(paths_sub_seed(seed, a), (unsigned long long)r, (unsigned long long)c);
}

// u[j * d + k] (matern: scaled by sqrt(5 / c_j)) and phase[j]; either may be NULL (the caller's array is kept)
__global__ void k_paths_draw_freq(double* __restrict__ u, double* __restrict__ phase, int64_t F, int d, int matern,
                                  unsigned long long seed) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= F) return;
  if (u) {
    double sc = 1.0;
    if (matern) {
      const unsigned long long s1 = paths_sub_seed(seed, 1);
      double c = 0.0;
      for (int k = 0; k < 5; ++k) {
        const double z = paths_normal(s1, (unsigned long long)j, (unsigned long long)k);
        c += z * z;
      }
      sc = sqrt(5.0 / c);
    }
    const unsigned long long s0 = paths_sub_seed(seed, 0);
    for (int k = 0; k < d; ++k) u[j * d + k] = paths_normal(s0, (unsigned long long)j, (unsigned long long)k) * sc;
  }
  if (phase) {
    const unsigned long long key = hmc_mix64(paths_sub_seed(seed, 2) ^ hmc_mix64((unsigned long long)j));
    phase[j] = PATHS_TWO_PI * hmc_u01(hmc_mix64(key));
  }
}

// WT[j * ldw + s] = W[s * F + j] for j < F, s < S; 0 in the padding (j < Fp, s < ldw): the weights as the K rows of an RC operand
// grid (Fp, ceil(ldw / 256))
__global__ void k_paths_pack_w(const double* __restrict__ W, int64_t S, int64_t F, double* __restrict__ WT, int64_t ldw) {
  const int64_t s = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int64_t j = blockIdx.x;
  if (s >= ldw) return;
  WT[j * ldw + s] = (s < S && j < F) ? W[s * F + j] : 0.0;
}

// ---- random Fourier features: PhiT[j * ldo + i] = sqrt(2 kvar / F) cos(u_j . xs_i + b_j) --------------------------------------
// xs: the SCALED coordinates the handle keeps (XsT[k * ldx + i] = x_ik / ls_k), so u_j are unit-length-scale frequencies.
// Points i >= n and features j >= F are written as 0 (rows j < Fp, columns i < npad: the K rows of an RC operand).
// One workgroup = 128 points x 64 features: a thread owns one point (its DCAP coordinates stay in registers), the two
// 128-thread halves take 32 features each; a wave's lanes share the feature, so u_j and b_j are wave-uniform loads and the
// stores are coalesced (512 B per wave per feature).  The argument is reduced here, t = arg / 2 pi - rint(arg / 2 pi) in
// [-1/2, 1/2], and cos(2 pi t) taken as cospi(2 t): no large-argument path of the library's cos, no scratch.
// grid (npad / 128, Fp / 64 rounded up).
template <int DCAP>
__global__ __launch_bounds__(256) void k_paths_features(const double* __restrict__ XsT, int64_t ldx, int64_t n, int d,
                                                        const double* __restrict__ U, const double* __restrict__ phase,
                                                        int64_t F, int64_t Fp, double amp, double* __restrict__ PhiT,
                                                        int64_t ldo) {
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * TILE + (t & 127);
  const int half = __builtin_amdgcn_readfirstlane(t >> 7);
  double x[DCAP];
#pragma unroll
  for (int k = 0; k < DCAP; ++k) x[k] = (k < d) ? XsT[(int64_t)k * ldx + i] : 0.0;
  const int64_t j0 = (int64_t)blockIdx.y * 64 + half * 32;
  for (int jj = 0; jj < 32; ++jj) {
    const int64_t j = j0 + jj;
    if (j >= Fp) break;
    double v = 0.0;
    if (j < F && i < n) {
      const double* uj = U + j * d;
      double arg = phase[j];
#pragma unroll
      for (int k = 0; k < DCAP; ++k)
        if (k < d) arg = __builtin_fma(uj[k], x[k], arg);
      double tt = arg * PATHS_INV_TWO_PI;
      tt -= rint(tt);
      v = amp * cospi(2.0 * tt);
    }
    PhiT[j * ldo + i] = v;
  }
}

// ---- the right-hand sides of the conditioning solve: Rc[n][s] = -(Phi(X) w_s)[n] - eps_s[n]  (= R - y 1^T of the issue) -------
// grid (ldr / 128 path tiles, Np / 128 row tiles); the product runs over the padded feature count Fp on the 128-tile core
// (PhiXT: Fp x Np, WT: Fp x ldr, both RC).  Rows n >= N and columns s >= S come out 0 (the features and weights are 0 there
// and eps is not read).  E: the dense S x N noise draws.
__global__ __launch_bounds__(256, 2) void k_paths_rhs(const double* __restrict__ PhiXT, int64_t ldp,
                                                      const double* __restrict__ WT, int64_t ldw, int64_t Fp,
                                                      const double* __restrict__ E, int64_t N, int64_t S,
                                                      double* __restrict__ Rc, int64_t ldr) {
  extern __shared__ double smem[];
  const int ts = blockIdx.x, tn = blockIdx.y;
  v4d acc[4][4];
  acc_zero(acc);
  tile_gemm<false, RC, RC, TILE>(acc, PhiXT, ldp, (int64_t)tn * TILE, WT, ldw, (int64_t)ts * TILE, 0, Fp, smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = (int64_t)tn * TILE + acc_row(i, r), s = (int64_t)ts * TILE + acc_col(j);
        Rc[n * ldr + s] = (n < N && s < S) ? -acc[i][j][r] - E[s * N + n] : 0.0;
      }
}

// ---- S paths at a chunk of queries: f[s][c] = sum_k VW[k][s] OP[k][c]  (+ mean[c]) ------------------------------------------------
// OP [kend x ldo]: the operand the assembly kernels wrote for the chunk, K(X, Q_chunk) in rows [0, Np) and Phi(Q_chunk) in rows
// [Np, Np + Fp); VW [kend x ldv]: V_c in rows [0, Np), W^T below.  One workgroup = one T x T tile (rows: paths, columns:
// queries, so a path's values are stored contiguously); T = 32 / 64 / 128 is picked from S on the host.  grid (ncp / T, Sp / T).
// mean (NULL: centred values) = K(X, Q)^T alpha of the chunk.  ARGMAX = false: out[s * ldout + c] for s < S, c < nc.
// ARGMAX = true: nothing of the S x C matrix is stored; the tile's maximum of f + bias[s * ldb + c] (bias may be NULL) per path
// and its column land in pmax / pidx[s * npt + tile] (ties: the lower column; NaN never wins; no valid entry: -inf, column 0),
// k_paths_argmax_merge folds them.  The reduction: every lane keeps the best of its four fragments per row, the 32 lane
// candidates of a row (16 lanes x the two column halves) meet in LDS - smem is free once the product is done - and one thread
// per row scans them.  Tile core: direct-to-LDS where the tile has one (T = 128 and 64; T = 32: register-staged).
template <int T, bool ARGMAX>
__global__ __launch_bounds__(256, 2) void k_paths_tiles(const double* __restrict__ VW, int64_t ldv,
                                                        const double* __restrict__ OP, int64_t ldo, int64_t kend,
                                                        const double* __restrict__ mean, int64_t S, int64_t nc,
                                                        double* __restrict__ out, int64_t ldout,
                                                        const double* __restrict__ bias, int64_t ldb,
                                                        double* __restrict__ pmax, int* __restrict__ pidx, int npt) {
  extern __shared__ double smem[];
  constexpr int FR = T / 32;
  const int tq = blockIdx.x, ts = blockIdx.y;
  v4d acc[FR][FR];
  acc_zero(acc);
  tile_gemm<true, RC, RC, T>(acc, VW, ldv, (int64_t)ts * T, OP, ldo, (int64_t)tq * T, 0, kend, smem);
  if (!ARGMAX) {
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t s = (int64_t)ts * T + acc_row<T>(i, r);
        if (s >= S) continue;
#pragma unroll
        for (int j = 0; j < FR; ++j) {
          const int64_t c = (int64_t)tq * T + acc_col<T>(j);
          if (c < nc) out[s * ldout + c] = acc[i][j][r] + (mean ? mean[c] : 0.0);
        }
      }
    return;
  }
  // 32 candidates per row: slot = 16 * (column half) + (lane & 15)
  double* cv = smem;                                        // [T][32] values
  int* ci = reinterpret_cast<int*>(smem + T * 32);          // [T][32] columns inside the tile
  __syncthreads();                                          // (the product's last LDS reads are done)
  const int slot = 16 * ((threadIdx.x >> 6) & 1) + (threadIdx.x & 15);
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rl = acc_row<T>(i, r);
      const int64_t s = (int64_t)ts * T + rl;
      double bv = -INFINITY;
      int bc = T;
#pragma unroll
      for (int j = 0; j < FR; ++j) {                        // (ascending columns: a strict > keeps the lower one on ties)
        const int cl = acc_col<T>(j);
        const int64_t c = (int64_t)tq * T + cl;
        if (s < S && c < nc) {
          double v = acc[i][j][r] + (mean ? mean[c] : 0.0);
          if (bias) v += bias[s * ldb + c];
          if (v > bv || (bc == T && v == bv)) {
            bv = v;
            bc = cl;
          }
        }
      }
      cv[rl * 32 + slot] = bv;
      ci[rl * 32 + slot] = bc;
    }
  __syncthreads();
  if ((int)threadIdx.x < T) {
    const int rl = threadIdx.x;
    const int64_t s = (int64_t)ts * T + rl;
    if (s < S) {
      double bv = -INFINITY;
      int bc = T;
      for (int q = 0; q < 32; ++q) {
        const double v = cv[rl * 32 + q];
        const int c = ci[rl * 32 + q];
        if (c < T && (v > bv || (v == bv && c < bc))) {
          bv = v;
          bc = c;
        }
      }
      pmax[s * npt + tq] = bv;
      pidx[s * npt + tq] = bc < T ? bc : 0;
    }
  }
}

// the second stage: best[s] / idx[s] (running over the chunks of a call, armed with -inf / 0) against the npt tile results of
// this chunk, tiles in ascending order - a strict > keeps the earlier (lower) index on ties.  c0: the chunk's first query.
template <int T>
__global__ void k_paths_argmax_merge(const double* __restrict__ pmax, const int* __restrict__ pidx, int npt, int64_t S,
                                     int64_t c0, double* __restrict__ best, int64_t* __restrict__ idx) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  double bv = best[s];
  int64_t bi = idx[s];
  for (int t = 0; t < npt; ++t) {
    const double v = pmax[s * npt + t];
    if (v > bv) {
      bv = v;
      bi = c0 + (int64_t)t * T + pidx[s * npt + t];
    }
  }
  best[s] = bv;
  idx[s] = bi;
}

__global__ void k_paths_argmax_arm(double* __restrict__ best, int64_t* __restrict__ idx, int64_t S) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  best[s] = -INFINITY;
  idx[s] = 0;
}

// ---- value and input gradient of one path per query point (bobe_gp_paths_grad) -------------------------------------------------
// VcT[s * ldt + n] = VW[n * ldv + s] for s < S, n < Np: a path's coefficients as one contiguous row.  Built once per set, at
// its first gradient call.  grid (S, ceil(Np / 256))
__global__ void k_paths_transpose_vc(const double* __restrict__ VW, int64_t ldv, int64_t Np, double* __restrict__ VcT,
                                     int64_t ldt) {
  const int64_t n = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int64_t s = blockIdx.x;
  if (n >= Np) return;
  VcT[s * ldt + n] = VW[n * ldv + s];
}

// With xs = x / ls, c_n = VcT[s][n] + alpha[n] (centred: VcT[s][n] alone), amp = sqrt(2 kvar / F), arg_j = u_j . xs + b_j:
//   f[t]      = sum_n c_n k(r2_n) + amp sum_j w_sj cos(arg_j)
//   df[t][k]  = (1 / ls_k) [ sum_n c_n G(r2_n) (xs_nk - xs_k) - amp sum_j w_sj sin(arg_j) u_jk ],   G = kern_grad_factor
// for the point x = Xq[t] and the path s = pidx[t] (a wave-uniform load).  One 256-thread workgroup per point.  Thread tau
// adds the kernel terms n = tau, tau + 256, ... < N and then the feature terms j = tau, tau + 256, ... < F, each in
// ascending order, into ONE set of 1 + d accumulators (the feature terms enter as (amp w_sj) cos and -(amp w_sj) sin u_jk).
// The training coordinates come from XsT (coalesced); the argument is reduced as in k_paths_features, t = arg / 2 pi -
// rint(arg / 2 pi), and the pair taken as sincospi(2 t): no large-argument path, no scratch.  The 256 partials of every
// component are added in one fixed tree: chain_wave_sum (f) and wave_sum_components (the DCAP gradient components) within a
// wave, then the four waves through LDS as ((w0 + w1) + w2) + w3; the division by ls_k happens once, at the store.  No
// atomics: the bits of (f, df) at a point depend on the set, the point, its path and the centred flag alone - not on T, the
// other points of the call or the pointer kinds.  f or df may be NULL (nothing else changes).
// The set is read again by every workgroup (L2-resident at the sizes of a polish: tens to thousands of points).
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950), rbf / matern: DCAP 8: 94 / 117 VGPRs (5 / 4 waves per
// SIMD), DCAP 16: 166 / 166 (3), DCAP 32: 241 / 246 (2); no AGPRs, scratch 0 in all six, LDS 4 * (DCAP + 1) doubles.
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_paths_grad(const double* __restrict__ XsT, int64_t ldx, int64_t N, Hyper h,
                                                    const double* __restrict__ alpha, const double* __restrict__ VcT,
                                                    int64_t ldt, const double* __restrict__ U,
                                                    const double* __restrict__ phase, const double* __restrict__ W,
                                                    int64_t F, double amp, const double* __restrict__ Xq,
                                                    const int64_t* __restrict__ pidx, int centered,
                                                    double* __restrict__ f, double* __restrict__ df) {
  __shared__ double red[4][DCAP + 1];
  const int tau = threadIdx.x, lane = tau & 63, wave = tau >> 6;
  const int64_t t = blockIdx.x;
  const int64_t s = pidx[t];
  const int d = h.d;
  double xs[DCAP], acc[DCAP], v[DCAP];
  double af = 0.0;
  // (constant indices into h.ls: a runtime index would send the by-value struct through scratch memory)
#pragma unroll
  for (int k = 0; k < DCAP; ++k) {
    xs[k] = (k < d) ? Xq[t * d + k] / h.ls[k] : 0.0;
    acc[k] = 0.0;
  }
  const double* vc = VcT + s * ldt;
  for (int64_t n = tau; n < N; n += 256) {
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      v[k] = (k < d) ? XsT[(int64_t)k * ldx + n] - xs[k] : 0.0;
      r2 = __builtin_fma(v[k], v[k], r2);
    }
    const double c = centered ? vc[n] : vc[n] + alpha[n];
    const double kv = kern_eval<KERN>(r2, h.kvar);
    const double cg = c * kern_grad_factor<KERN>(r2, h.kvar, kv);
    af = __builtin_fma(c, kv, af);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) acc[k] = __builtin_fma(cg, v[k], acc[k]);
  }
  const double* ws = W + s * F;
  for (int64_t j = tau; j < F; j += 256) {
    const double* uj = U + j * d;
    double arg = phase[j];
#pragma unroll
    for (int k = 0; k < DCAP; ++k) {
      v[k] = (k < d) ? uj[k] : 0.0;
      arg = __builtin_fma(v[k], xs[k], arg);
    }
    double tt = arg * PATHS_INV_TWO_PI;
    tt -= rint(tt);
    double sn, cs;
    sincospi(2.0 * tt, &sn, &cs);
    const double wa = amp * ws[j];
    af = __builtin_fma(wa, cs, af);
    const double ms = -(wa * sn);
#pragma unroll
    for (int k = 0; k < DCAP; ++k) acc[k] = __builtin_fma(ms, v[k], acc[k]);
  }
  // the wave's sums: f in every lane, gradient component (lane >> SH) in the lanes of its group
  constexpr int SH = DCAP == 8 ? 3 : (DCAP == 16 ? 2 : 1);
  af = chain_wave_sum(af);
  const double gk = wave_sum_components<DCAP>(acc, lane);
  if ((lane & ((1 << SH) - 1)) == 0) red[wave][lane >> SH] = gk;
  if (lane == 0) red[wave][DCAP] = af;
  __syncthreads();
  if (tau < d) {
    if (df) {
      double lk = h.ls[0];
#pragma unroll
      for (int k = 1; k < DCAP; ++k) lk = (tau == k) ? h.ls[k] : lk;
      df[t * d + tau] = (((red[0][tau] + red[1][tau]) + red[2][tau]) + red[3][tau]) / lk;
    }
  } else if (tau == 64) {
    if (f) f[t] = ((red[0][DCAP] + red[1][DCAP]) + red[2][DCAP]) + red[3][DCAP];
  }
}

// ---- whole HMC chains on a posterior PATH (bobe_gp_paths_hmc_run) ---------------------------------------------------------------
// hmc_chain_run (chain_common.hpp: the contract, the state / adapt / hist / keep / dbg layouts, the random numbers) on a
// target of its own: chain c samples the posterior implied by the path s = pidx[c] of the set instead of the posterior mean.  With
// xs = x / ls, c_n = VcT[s][n] + alpha[n], amp = sqrt(2 kvar / F):
//   f(x)      = sum_n c_n k(r2_n) + amp sum_j w_sj cos(u_j . xs + b_j)
//   df/dx_k   = (1 / ls_k) [ sum_n c_n G(r2_n) (xs_nk - xs_k) - amp sum_j w_sj sin(u_j . xs + b_j) u_jk ]      (k_paths_grad)
//   mean slot = ymean + ystd f,   logp(u) = mean / temp + sum_k [log x_k + log(1 - x_k)],   u = logit(x)
// inv_mass is PER CHAIN, [P][d] - paths differ in shape and the host pools the spread per path.  The coefficients c_n are
// formed once per launch (CoefPath) and live where k_hmc_run keeps alpha, ChainRows<DCAP>::PATHS rows per thread in
// registers.  After its kernel terms thread t adds the features j = t, t + 256, ... < F in ascending order into the same 1 + d
// accumulators (extra), the argument reduced as in k_paths_features (tt = arg / 2 pi - rint(arg / 2 pi), sincospi(2 tt)); U,
// phase and the path's row of W are streamed from L2 in every step (U alone is 256 KB at F = 4096, d = 8: more than a CU's
// LDS).  The feature loop keeps ChainRows<DCAP>::STREAM features in flight per thread (2; 1 at DCAP 32): all loads of the
// group first, as the streamed rows do - one wave per SIMD hides no latency by itself.  A feature past F enters with weight 0;
// coordinates >= d of the point read as 0 (chain_load_point).  The gate is the PARENT handle's at call time (it is not part of the
// snapshot).  A chain's bits depend on the set, its path index, its own state / adapt / inv_mass rows, the seed, its chain
// number and the iteration numbers - not on P, the other chains' paths or where launches are cut.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950; profiles/chain_core_unify_resources.txt), rbf / matern,
// with ChainRows<DCAP>::PATHS = 14 / 6 / 1 rows in registers: DCAP 8: 256 VGPRs + 228 / 236 AGPRs, DCAP 16: 256 + 246 / 252,
// DCAP 32: 256 + 187 / 191; one wave per SIMD and scratch 0 in all six.  One row more: 7 rows at DCAP 16 spill 100 / 156
// bytes per lane and 2 rows at DCAP 32 spill 12 bytes per lane in the Matern variant (next to the 32 frequencies of a
// feature); 15 rows at DCAP 8 would fit (246 / 254 AGPRs) and are not taken here.  LDS: 704 / 1280 / 2432 bytes static.
template <int DCAP>
struct HmcPathTarget {
  static constexpr int RMAX = ChainRows<DCAP>::PATHS, FUN = ChainRows<DCAP>::STREAM;
  static constexpr bool FMA = true;
  const double* alpha;
  const double* vc;                            // this chain's path: its row of VcT ...
  const double* U;
  const double* phase;
  const double* ws;                            // ... and of W
  int64_t F;
  double amp;
  const double* inv_mass;                      // this chain's row
  __device__ __forceinline__ CoefPath coef() const { return {vc, alpha}; }
  __device__ __forceinline__ void extra(const double (&xs)[DCAP], int d, int t, double& ms, double (&gm)[DCAP]) const {
    for (int64_t j = t; j < F; j += FUN * 256) {               // this thread's features, ascending, FUN in flight
      double uv[FUN][DCAP], ph[FUN], wv[FUN];
#pragma unroll
      for (int q = 0; q < FUN; ++q) {                          // (all loads of the group first; a feature past F has weight 0)
        const int64_t jq = j + q * 256;
        ph[q] = (jq < F) ? phase[jq] : 0.0;
        wv[q] = (jq < F) ? ws[jq] : 0.0;
#pragma unroll
        for (int k = 0; k < DCAP; ++k) uv[q][k] = (k < d && jq < F) ? U[jq * d + k] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < FUN; ++q) {
        double arg = ph[q];
#pragma unroll
        for (int k = 0; k < DCAP; ++k) arg = __builtin_fma(uv[q][k], xs[k], arg);
        double tt = arg * PATHS_INV_TWO_PI;
        tt -= rint(tt);
        double sn, cs;
        sincospi(2.0 * tt, &sn, &cs);
        const double wa = amp * wv[q];
        ms = __builtin_fma(wa, cs, ms);
        const double mw = -(wa * sn);
#pragma unroll
        for (int k = 0; k < DCAP; ++k) gm[k] = __builtin_fma(mw, uv[q][k], gm[k]);
      }
    }
  }
};

template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_paths_hmc_run(const double* __restrict__ XsT, int64_t ldx, int64_t n, Hyper h,
                                                       const double* __restrict__ alpha, const double* __restrict__ VcT,
                                                       int64_t ldt, const double* __restrict__ U,
                                                       const double* __restrict__ phase, const double* __restrict__ W,
                                                       int64_t F, double amp, const int64_t* __restrict__ pidx, int64_t P,
                                                       double* __restrict__ S, double* __restrict__ adapt,
                                                       const double* __restrict__ inv_mass, unsigned long long seed,
                                                       int64_t it0, int niter, int do_adapt, double ystd, double ymean,
                                                       double temp, int hist_from, double* __restrict__ hist, int thin,
                                                       double* __restrict__ keep, double* __restrict__ dbg, Gate gt,
                                                       int lgroups) {
  const int64_t c = blockIdx.x, s_path = pidx[c];
  const HmcPathTarget<DCAP> tg{alpha, VcT + s_path * ldt, U, phase, W + s_path * F, F, amp, inv_mass + c * h.d};
  hmc_chain_run<KERN, DCAP>(tg, XsT, ldx, n, h, P, S, adapt, seed, it0, niter, do_adapt, ystd, ymean, temp, hist_from, hist,
                            thin, keep, dbg, gt, lgroups);
}

}  // namespace bobe
