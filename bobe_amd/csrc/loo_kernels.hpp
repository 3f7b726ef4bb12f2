// Kernels of the leave-one-out cross-validation (gp_loo.hip; Rasmussen & Williams section 5.4.2).
// With A = K^-1 (noise included), a_i = A_ii and alpha = A y, everything in standardised units:
//   mu_-i = y_i - alpha_i / a_i,   sigma^2_-i = 1 / a_i,   lpd_i = 1/2 log a_i - alpha_i^2 / (2 a_i) - 1/2 log 2 pi
//   L_LOO = sum_i lpd_i,   dL_LOO / dtheta_j = sum_ab M_ab dK_ab / dtheta_j   with
//   c_i = 1 / (2 a_i) + alpha_i^2 / (2 a_i^2),  b_i = -alpha_i / a_i,  w = A b,
//   M = -A diag(c) A - 1/2 (w alpha^T + alpha w^T).
// a_i is the column sum of squares of the triangular inverse factor (no product, no cancellation); A diag(c) A = B^T B with
// B = diag(sqrt c) A is a dense tile product on the cores of gemm_f64.hpp, fused with the gradient epilogue of k_lauum_grad
// (W there = 2 M here).  Every sum has a fixed order that depends on N only.
// Every kernel takes the member of a lock-step batch from its last grid dimension (k_loo_grad: from blockIdx.x, as
// k_lauum_grad) and works on base + member * stride of what it is given (strides in doubles); one member with stride 0 is
// the plain call, and a member's arithmetic does not depend on the batch it runs in.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

// part[rb * ldp + c] = sum over the rows k >= c of row block rb (128 rows) of Linv[k][c]^2, row blocks rb >= c / 128 only:
// the launch shape and the summation order of k_gemv_t_part (four runs of 32 rows, then ((r0 + r1) + r2) + r3), followed by
// k_colsum_parts(lower = 1).  grid.x = column strips of 64, grid.y = row blocks, grid.z = batch members.  Elements above the
// diagonal are never read.
static __global__ __launch_bounds__(256) void k_loo_colsq_part(const double* __restrict__ Linv, int64_t ld,
                                                                double* __restrict__ part, int64_t ldp, int64_t bsL = 0,
                                                                int64_t bsP = 0) {
  Linv += blockIdx.z * bsL;
  part += blockIdx.z * bsP;
  __shared__ double red[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cx;
  const int rb = blockIdx.y;
  double s = 0.0;
  if (rb >= (int)(blockIdx.x * 64 / TILE)) {
    const int64_t k0 = (int64_t)rb * TILE + ry * 32;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const double v = (k0 + k >= c) ? Linv[(k0 + k) * ld + c] : 0.0;
      s = __builtin_fma(v, v, s);
    }
  }
  red[ry][cx] = s;
  __syncthreads();
  if (ry == 0) part[(int64_t)rb * ldp + c] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

// The per-point terms from a (the diagonal of K^-1), alpha and y; one thread per padded point.  mean / var / lpd: [np]
// (0 in the padding).  sqc / bs (both or neither): sqrt(c_i) and b_i / sqrt(c_i), 0 in the padding - the row scaling of B
// and the vector whose product with B^T is w = A b.  grid.y = batch members: alpha strides by bsA, the six vectors of the
// LOO block by bsV; y is shared.
static __global__ __launch_bounds__(256) void k_loo_point(const double* __restrict__ a, const double* __restrict__ alpha,
                                                           const double* __restrict__ y, int64_t n, int64_t np,
                                                           double* __restrict__ mean, double* __restrict__ var,
                                                           double* __restrict__ lpd, double* __restrict__ sqc,
                                                           double* __restrict__ bs, int64_t bsA = 0, int64_t bsV = 0) {
  const int64_t mo = blockIdx.y * bsV;
  a += mo;
  alpha += blockIdx.y * bsA;
  mean += mo;
  var += mo;
  lpd += mo;
  if (sqc) {
    sqc += mo;
    bs += mo;
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double m = 0.0, v = 0.0, l = 0.0, sc = 0.0, b = 0.0;
  if (i < n) {
    const double ai = a[i], al = alpha[i];
    const double r = al / ai;
    m = y[i] - r;
    v = 1.0 / ai;
    l = 0.5 * log(ai) - 0.5 * (al * r) - 0.91893853320467274178;      // 1/2 log 2 pi
    const double c = 0.5 * v + 0.5 * (r * r);
    sc = sqrt(c);
    b = -r / sc;
  }
  mean[i] = m;
  var[i] = v;
  lpd[i] = l;
  if (sqc) {
    sqc[i] = sc;
    bs[i] = b;
  }
}

// *out = sum_{i < n} lpd[i]: one workgroup per batch member (grid.y), thread-strided partial sums, wave_sum,
// ((w0 + w1) + w2) + w3
static __global__ __launch_bounds__(256) void k_loo_sum(const double* __restrict__ lpd, int64_t n, double* __restrict__ out,
                                                         int64_t bsV = 0, int64_t bsO = 0) {
  lpd += blockIdx.y * bsV;
  out += blockIdx.y * bsO;
  __shared__ double r[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += lpd[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((r[0] + r[1]) + r[2]) + r[3];
}

// B = diag(sqc) A, dense, from the LOWER triangle of A = K^-1 as k_lauum_grad stores it (elements above the diagonal of
// Kinv are never read): workgroup = one lower 32 x 32 tile (ti >= tj), written scaled to B[ti][tj] and, transposed through
// LDS, to B[tj][ti].  Kinv and B must not overlap.  grid.y = batch members (Kinv and B stride by bsM, sqc by bsV).
static __global__ __launch_bounds__(256) void k_loo_make_b(const double* __restrict__ Kinv, int64_t ld,
                                                            const double* __restrict__ sqc, double* __restrict__ B,
                                                            int64_t bsM = 0, int64_t bsV = 0) {
  Kinv += blockIdx.y * bsM;
  B += blockIdx.y * bsM;
  sqc += blockIdx.y * bsV;
  __shared__ double s[32][33];
  int ti, tj;
  tri_decode((int)blockIdx.x, ti, tj);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t r0 = (int64_t)ti * 32, c0 = (int64_t)tj * 32;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    s[r][tx] = Kinv[(r0 + r) * ld + c0 + tx];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    const double v = (ti != tj || r >= tx) ? s[r][tx] : s[tx][r];
    B[(r0 + r) * ld + c0 + tx] = sqc[r0 + r] * v;
  }
  if (ti != tj) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = ty + 8 * q;                      // row c0 + r of B, column r0 + tx: A[r0 + tx][c0 + r]
      B[(c0 + r) * ld + r0 + tx] = sqc[c0 + r] * s[tx][r];
    }
  }
}

// ---- B^T B fused with the gradient reduction of the LOO objective ---------------------------------------------------------
// lower T x T tile (ti >= tj): G = sum over ALL k of B[k][ti]^T B[k][tj] (B dense: the full K range, unlike the triangular
// operand of k_lauum_grad);  W = 2 M = -2 G - (w alpha^T + alpha w^T) on the tile.
// partial[tile * (DCAP + 1) + j] = sum_ab W_ab dK_ab / dlog ls_j (j < d), [DCAP] = sum_ab W_ab Kt_ab (Kt: without noise),
// off-diagonal tiles weighted x2: the layout and the epilogue arithmetic of k_lauum_grad, reduced by k_mll_grad_reduce
// (x 1/2).  One tile per workgroup; the tile core as in k_lauum_grad (direct-to-LDS for T = 64).
// Batch: one grid dimension, tile-major - workgroup id = tile * nbatch + member, the order k_lauum_grad takes (here every
// tile has the same K length, so the order is a convention, not a schedule).  hp: the members' hyper-parameters on the
// device (NULL: h by value); B strides by bsB, alpha by bsV, w by bsW, XsT by bsX, partial by bsP.
template <int KERN, int DCAP, int T>
__global__ __launch_bounds__(256, 2) void k_loo_grad(const double* __restrict__ B, int64_t ldb, int64_t np, int64_t n,
                                                     const double* __restrict__ alpha, const double* __restrict__ wv,
                                                     const double* __restrict__ XsT, int64_t ldx, Hyper h,
                                                     double* __restrict__ partial, const Hyper* __restrict__ hp = nullptr,
                                                     int64_t bsB = 0, int64_t bsV = 0, int64_t bsW = 0, int64_t bsX = 0,
                                                     int64_t bsP = 0, int nbatch = 1) {
  extern __shared__ double smem[];
  const int tile = (int)(blockIdx.x / nbatch), slot = (int)(blockIdx.x % nbatch);
  if (hp) h = hp[slot];
  B += slot * bsB;
  alpha += slot * bsV;
  wv += slot * bsW;
  XsT += slot * bsX;
  partial += slot * bsP;
  int ti, tj;
  tri_decode(tile, ti, tj);
  v4d acc[T / 32][T / 32];
  acc_zero(acc);
  tile_gemm<T == 64, RC, RC, T>(acc, B, ldb, (int64_t)ti * T, B, ldb, (int64_t)tj * T, (int64_t)0, np, smem);
  __syncthreads();                    // (every wave is through with the GEMM's LDS images)
  double* xa = smem;                  // [d][T]
  double* xb = smem + MAX_D * T;      // [d][T]
  double* aa = smem + 2 * MAX_D * T;  // [T] alpha of the tile's rows, then of its columns, then w likewise
  double* ab = aa + T;
  double* wa = ab + T;
  double* wb = wa + T;
  double* red = wb + T;               // [4][DCAP+1]
  static_assert((2 * MAX_D * T + 4 * T + 4 * (DCAP + 1)) * 8 <= (T == 128 ? GEMM_SMEM_BYTES : GEMM64_SMEM_BYTES),
                "the epilogue's staging must fit the tile core's LDS");
  const int t = threadIdx.x;
  for (int e = t; e < h.d * T; e += 256) {
    const int j = e / T, c = e % T;
    xa[j * T + c] = XsT[j * ldx + (int64_t)ti * T + c];
    xb[j * T + c] = XsT[j * ldx + (int64_t)tj * T + c];
  }
  if (t < T) {
    aa[t] = alpha[(int64_t)ti * T + t];
    ab[t] = alpha[(int64_t)tj * T + t];
    wa[t] = wv[(int64_t)ti * T + t];
    wb[t] = wv[(int64_t)tj * T + t];
  }
  __syncthreads();
  double g[DCAP + 1];
#pragma unroll
  for (int j = 0; j <= DCAP; ++j) g[j] = 0.0;
#pragma unroll
  for (int i = 0; i < T / 32; ++i)
#pragma unroll
    for (int jj = 0; jj < T / 32; ++jj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = acc_row<T>(i, r), b = acc_col<T>(jj);
        const int64_t ga = (int64_t)ti * T + a, gb = (int64_t)tj * T + b;
        if (ga < n && gb < n) {
          const double w = -2.0 * acc[i][jj][r] - (wa[a] * ab[b] + aa[a] * wb[b]);
          double dsq[DCAP];
          double r2 = 0.0;
#pragma unroll
          for (int j = 0; j < DCAP; ++j) {
            if (j < h.d) {
              const double df = xa[j * T + a] - xb[j * T + b];
              dsq[j] = df * df;
              r2 += dsq[j];
            } else {
              dsq[j] = 0.0;
            }
          }
          const double kv = kern_eval<KERN>(r2, h.kvar);
          const double wf = w * kern_grad_factor<KERN>(r2, h.kvar, kv);
#pragma unroll
          for (int j = 0; j < DCAP; ++j) g[j] += wf * dsq[j];
          g[DCAP] += w * kv;
        }
      }
  const double wt = (ti == tj) ? 1.0 : 2.0;
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int j = 0; j <= DCAP; ++j) {
    const double s = wave_sum(g[j]);
    if (lane == 0) red[wave * (DCAP + 1) + j] = s;
  }
  __syncthreads();
  if (t <= DCAP) {
    const double s = ((red[t] + red[(DCAP + 1) + t]) + red[2 * (DCAP + 1) + t]) + red[3 * (DCAP + 1) + t];
    partial[(int64_t)tile * (DCAP + 1) + t] = wt * s;
  }
}

// ---- the noise component of the two gradients (bobe_gp_mll_noise, bobe_gp_loo_objective_noise) ----------------------------
// theta_{d+1} = log nu with K~ = K + nu I, dK~ / dlog nu = nu I: the component is nu times the trace of the matrix the other
// components contract with dK,
//   dMLL / dlog nu   = 1/2 nu (sum_i alpha_i^2 - sum_i a_i)                  (tr K~^-1 = sum_i a_i = |L^-1|_F^2)
//   dL_LOO / dlog nu = nu tr M = -nu (|B|_F^2 + w^T alpha)                   (|B|_F^2 = sum_k c_k (A^2)_kk)
// over the true n x n block only: the identity padding of the factor would add np - n to tr K~^-1.  Bandwidth-bound
// reductions, launched AFTER everything the evaluation queues without them; a thread owns a column, every order is fixed.
// nu: hp[member].noise (the lock-step batch's device copy), else `noise` by value.

// *out = 1/2 nu (sum_{i < n} alpha[i]^2 - sum_{i < n} a[i]): one workgroup per batch member (grid.y), k_loo_sum's order for
// both sums.  a strides by bsV, alpha by bsA, out by bsO.
static __global__ __launch_bounds__(256) void k_noise_mll_grad(const double* __restrict__ a, const double* __restrict__ alpha,
                                                                int64_t n, double noise, const Hyper* __restrict__ hp,
                                                                double* __restrict__ out, int64_t bsV = 0, int64_t bsA = 0,
                                                                int64_t bsO = 0) {
  a += blockIdx.y * bsV;
  alpha += blockIdx.y * bsA;
  out += blockIdx.y * bsO;
  if (hp) noise = hp[blockIdx.y].noise;
  __shared__ double r[2][4];
  double s2 = 0.0, sa = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double al = alpha[i];
    s2 = __builtin_fma(al, al, s2);
    sa += a[i];
  }
  s2 = wave_sum(s2);
  sa = wave_sum(sa);
  if ((threadIdx.x & 63) == 0) {
    r[0][threadIdx.x >> 6] = s2;
    r[1][threadIdx.x >> 6] = sa;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t2 = ((r[0][0] + r[0][1]) + r[0][2]) + r[0][3], ta = ((r[1][0] + r[1][1]) + r[1][2]) + r[1][3];
    *out = 0.5 * noise * (t2 - ta);
  }
}

// part[rb * ldp + c] = sum over the rows k < n of row block rb (128 rows) of B[k][c]^2 for the columns c < n, 0 for the
// padding columns: k_loo_colsq_part's launch shape and order on a DENSE matrix (every row block).  grid.x = column strips of
// 64, grid.y = row blocks, grid.z = batch members.
static __global__ __launch_bounds__(256) void k_loo_bsq_part(const double* __restrict__ B, int64_t ld, int64_t n,
                                                              double* __restrict__ part, int64_t ldp, int64_t bsB = 0,
                                                              int64_t bsP = 0) {
  B += blockIdx.z * bsB;
  part += blockIdx.z * bsP;
  __shared__ double red[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + cx;
  const int rb = blockIdx.y;
  double s = 0.0;
  if (c < n) {
    const int64_t k0 = (int64_t)rb * TILE + ry * 32;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const double v = (k0 + k < n) ? B[(k0 + k) * ld + c] : 0.0;
      s = __builtin_fma(v, v, s);
    }
  }
  red[ry][cx] = s;
  __syncthreads();
  if (ry == 0) part[(int64_t)rb * ldp + c] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

// *out = -nu (sum_{c < n} sum_rb part[rb * ldp + c] + sum_{c < n} w[c] alpha[c]): one workgroup per batch member (grid.y);
// a thread sums its columns' row blocks in ascending order (k_colsum_parts), then k_loo_sum's order across the threads.
// part strides by bsP, w by bsW, alpha by bsA, out by bsO.
static __global__ __launch_bounds__(256) void k_noise_loo_grad(const double* __restrict__ part, int64_t ldp, int nrb,
                                                                const double* __restrict__ wv, const double* __restrict__ alpha,
                                                                int64_t n, double noise, const Hyper* __restrict__ hp,
                                                                double* __restrict__ out, int64_t bsP = 0, int64_t bsW = 0,
                                                                int64_t bsA = 0, int64_t bsO = 0) {
  part += blockIdx.y * bsP;
  wv += blockIdx.y * bsW;
  alpha += blockIdx.y * bsA;
  out += blockIdx.y * bsO;
  if (hp) noise = hp[blockIdx.y].noise;
  __shared__ double r[2][4];
  double sb = 0.0, sw = 0.0;
  for (int64_t c = threadIdx.x; c < n; c += 256) {
    double col = 0.0;
    for (int rb = 0; rb < nrb; ++rb) col += part[(int64_t)rb * ldp + c];
    sb += col;
    sw = __builtin_fma(wv[c], alpha[c], sw);
  }
  sb = wave_sum(sb);
  sw = wave_sum(sw);
  if ((threadIdx.x & 63) == 0) {
    r[0][threadIdx.x >> 6] = sb;
    r[1][threadIdx.x >> 6] = sw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tb = ((r[0][0] + r[0][1]) + r[0][2]) + r[0][3], tw = ((r[1][0] + r[1][1]) + r[1][2]) + r[1][3];
    *out = -noise * (tb + tw);
  }
}

}  // namespace bobe
