// Kernels of the joint posterior of the surrogate at C query points (bobe_gp_predict_cov, bobe_gp_posterior_sample; gfx950):
// the C x C covariance, the normals of the draws and the triangular product that turns them into draws.  Included by
// gp_posterior.hip only.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

// ---- Sigma[i][j] = k(q_i, q_j) + noise [i = j] - V_i . V_j,   V = L^-1 K(X, Q) (Np x ldv, column c = query c) ----------
// One workgroup = one 128 x 128 tile of the LOWER triangle.  Its rows are queries i0 + 128 ti + [0, 128) of the column chunk VI,
// its columns queries j0 + 128 tj + [0, 128) of VJ.  diag = 1 (VI and VJ are the same chunk): the ntI (ntI + 1) / 2 tile pairs
// tj <= ti; else every tile of the ntI x ntJ block.  The product runs on the sweep's 128-tile core (direct-to-LDS, RC x RC
// like k_cross_vv) over the whole padded K = Np: V's padded rows are 0.  The epilogue stages the tile's scaled coordinates
// (QsT[j * ldq + c] = q_cj / ls_j, d x 128 for the rows and for the columns) in the LDS the product is done with, evaluates
// k(q_i, q_j) as the kernel-matrix assembly does (fma over the dimensions; kvar + noise on the diagonal, the kself of
// bobe_gp_predict) and stores every element of the lower triangle AND its mirror from the same register: the upper triangle is
// the lower one bit for bit.  Inside a tile on the diagonal of Sigma only i >= j is stored.  Rows / columns >= C are not stored.
template <int KERN>
__global__ __launch_bounds__(256, 2) void k_sigma_tiles(const double* __restrict__ VI, const double* __restrict__ VJ,
                                                        int64_t ldv, int64_t kend, const double* __restrict__ QsT,
                                                        int64_t ldq, int64_t i0, int64_t j0, int ntJ, int diag, int64_t C,
                                                        Hyper h, double* __restrict__ out, int64_t ldo) {
  extern __shared__ double smem[];
  int ti, tj;
  if (diag) {
    tri_decode((int)blockIdx.x, ti, tj);
  } else {
    ti = (int)blockIdx.x / ntJ;
    tj = (int)blockIdx.x % ntJ;
  }
  v4d acc[4][4];
  acc_zero(acc);
  tile_gemm<true, RC, RC, TILE>(acc, VI, ldv, (int64_t)ti * TILE, VJ, ldv, (int64_t)tj * TILE, 0, kend, smem);
  const int64_t gi0 = i0 + (int64_t)ti * TILE, gj0 = j0 + (int64_t)tj * TILE;
  double* qa = smem;                       // [d][128] rows
  double* qb = smem + MAX_D * TILE;        // [d][128] columns   (2 x 32 x 128 doubles <= GEMM_SMEM_DOUBLES)
  __syncthreads();                         // (the product's last LDS reads are done)
  for (int e = threadIdx.x; e < h.d * TILE; e += 256) {
    const int j = e / TILE, r = e % TILE;
    qa[j * TILE + r] = QsT[(int64_t)j * ldq + gi0 + r];
    qb[j * TILE + r] = QsT[(int64_t)j * ldq + gj0 + r];
  }
  __syncthreads();
  const bool on_diag = diag && ti == tj;
  const double kself = h.kvar + h.noise;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = acc_row(i, r), cl = acc_col(j);
        const int64_t gi = gi0 + rl, gj = gj0 + cl;
        if (gi >= C || gj >= C || (on_diag && cl > rl)) continue;
        double kv;
        if (gi == gj) {
          kv = kself;
        } else {
          double r2 = 0.0;
          for (int jd = 0; jd < h.d; ++jd) {
            const double df = qa[jd * TILE + rl] - qb[jd * TILE + cl];
            r2 = __builtin_fma(df, df, r2);
          }
          kv = kern_eval<KERN>(r2, h.kvar);
        }
        const double v = kv - acc[i][j][r];
        out[gi * ldo + gj] = v;
        if (gi != gj) out[gj * ldo + gi] = v;
      }
}

// ---- the normals of the draws, transposed and padded: Zt[c * ldz + s] (c < Cp rows, s < ldz columns) --------------------
// Contract of the device's normals (what a caller replays to reproduce a draw; tests/test_posterior_draws_cpu.py does):
//   key(s)   = hmc_mix64(seed ^ hmc_mix64(s))                         (one stream per draw s, as one per chain in k_hmc_run)
//   u1, u2   = hmc_u01(hmc_mix64(key(s) + 2 c)), hmc_u01(hmc_mix64(key(s) + 2 c + 1))
//   z[s][c]  = sqrt(-2 log u1) cos(2 pi u2)                           (Box-Muller in fp64, cosine branch only)
// all arithmetic on unsigned 64-bit integers modulo 2^64; hmc_u01(b) = ((b >> 11) + 0.5) / 2^53.  A draw depends on (seed, s, c)
// alone: not on S, C's padding or the launch.  zin != nullptr: the caller's normals zin[s * C + c] (S x C) instead.
// Entries with s >= S or c >= C are 0 (they meet the identity padding of the factor).
__global__ void k_draw_normals(double* __restrict__ Zt, int64_t ldz, int64_t S, int64_t C, unsigned long long seed,
                               const double* __restrict__ zin) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t c = blockIdx.y;
  if (s >= ldz) return;
  double v = 0.0;
  if (s < S && c < C) {
    if (zin) {
      v = zin[s * C + c];
    } else {
      const unsigned long long key = hmc_mix64(seed ^ hmc_mix64((unsigned long long)s));
      const double a = hmc_u01(hmc_mix64(key + 2ull * (unsigned long long)c));
      const double b = hmc_u01(hmc_mix64(key + 2ull * (unsigned long long)c + 1ull));
      v = sqrt(-2.0 * log(a)) * cos(6.283185307179586 * b);
    }
  }
  Zt[c * ldz + s] = v;
}

// ---- draws[s * ldd + c] = m_c + sum_{k <= c} L[c][k] Zt[k][s]  (TRMM with the factor of Sigma) ----------------------------
// grid (ldz / 128 draw tiles, nbC row tiles of L), row tiles heaviest first.  The tile core and K range are k_trimul's: the
// K range of row tile tc ends with its diagonal block, so the zero tiles above the diagonal are never read, and the fragments
// right of the diagonal inside it are skipped (TRIL; the factor's strict upper part of its diagonal blocks must be 0).
// mean == nullptr: centred draws.  Rows c >= C and columns s >= S are not stored.
__global__ __launch_bounds__(256, 2) void k_trmm_draws(const double* __restrict__ L, int64_t ldl, int nbC,
                                                       const double* __restrict__ Zt, int64_t ldz,
                                                       const double* __restrict__ mean, int64_t S, int64_t C,
                                                       double* __restrict__ draws, int64_t ldd) {
  extern __shared__ double smem[];
  const int ts = blockIdx.x;
  const int tc = nbC - 1 - (int)blockIdx.y;
  v4d acc[4][4];
  acc_zero(acc);
  tile_gemm<true, KC, RC, TILE, false, true>(acc, L, ldl, (int64_t)tc * TILE, Zt, ldz, (int64_t)ts * TILE, 0,
                                             (int64_t)(tc + 1) * TILE, smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t c = (int64_t)tc * TILE + acc_row(i, r);
      if (c >= C) continue;
      const double m = mean ? mean[c] : 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t s = (int64_t)ts * TILE + acc_col(j);
        if (s < S) draws[s * ldd + c] = m + acc[i][j][r];
      }
    }
}

// ---- small helpers of the two entry points ----------------------------------------------------------------------------
// A[i][j] = Sig[i][j] + jit [i = j] for i, j < C, the identity in the padding (both triangles: the factorisation's input)
__global__ void k_sigma_load_jitter(const double* __restrict__ Sig, int64_t lds, int64_t C, double jit,
                                    double* __restrict__ A, int64_t lda, int64_t Cp) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (i >= Cp || j >= Cp) return;
  double v;
  if (i < C && j < C) v = Sig[i * lds + j] + (i == j ? jit : 0.0);
  else v = (i == j) ? 1.0 : 0.0;
  A[i * lda + j] = v;
}

// the strict upper part of the 128 x 128 diagonal blocks of a factor -> 0 (grid: one workgroup per block)
__global__ void k_zero_diag_upper(double* __restrict__ A, int64_t lda) {
  double* blk = A + (int64_t)blockIdx.x * TILE * lda + (int64_t)blockIdx.x * TILE;
  for (int e = threadIdx.x; e < TILE * TILE; e += blockDim.x) {
    const int r = e / TILE, c = e % TILE;
    if (c > r) blk[(int64_t)r * lda + c] = 0.0;
  }
}

// dg[i] = Sig[i][i], i < C
__global__ void k_take_diag(const double* __restrict__ Sig, int64_t lds, int64_t C, double* __restrict__ dg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) dg[i] = Sig[i * lds + i];
}

}  // namespace bobe
