// fp64 MFMA tile GEMM core for gfx950 (MI355X / CDNA4).
//
// One workgroup = 256 threads = 4 waves (2x2), output tile TM x TN (128 or 64 each), K-step BK (16 or 32).
// Each wave owns a (TM/2)x(TN/2) sub-tile = (TM/32)x(TN/32) fragments of v_mfma_f64_16x16x4_f64.
// Operands are staged global -> registers -> LDS (double-buffered, one barrier per K-step) and
// read back as MFMA fragments with conflict-free ds_read_b64:
//
//   layout KC ("k contiguous"):   element (r,k) at p[r*ld + k]   LDS image [R][BK+2]
//   layout RC ("row contiguous"): element (r,k) at p[k*ld + r]   LDS image [BK][R+16]
//
// where r is the m index for the A operand (R = TM) and the n index for the B operand (R = TN), so
// C[m][n] = sum_k A(m,k) * B(n,k) in both cases.
//
// v_mfma_f64_16x16x4_f64 fragment maps (cdna_hip_programming.md section 3):
//   A: lane l holds A[l&15][l>>4]        B: lane l holds B[k=l>>4][n=l&15]
//   D: lane l, reg r holds D[(l>>4)+4r][l&15]
//
// The 128x128 tile has the best arithmetic intensity (16 flop per LDS-staged byte); the 64x64 tile
// quarters the work per workgroup and is used where a launch has too few or too unequal tiles to
// fill 256 CUs (one CU delivers only ~0.3 TFLOP/s of fp64 MFMA, so balance beats tile efficiency).
//
// All matrices handled by this core are padded to multiples of 128 (rows) and 16 (K) with 16-byte
// aligned bases and even leading dimensions, so there are no bounds checks in the inner loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace bobe {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int TILE = 128;          // padding granule and default output tile edge
constexpr int TK = 16;             // K granule (every K range is a multiple of 16)
constexpr int GEMM_THREADS = 256;

enum Layout { KC = 0, RC = 1 };

// LDS image of one operand tile: R rows x BK k.  KC rows are padded by 2 doubles (stride = 4 mod 64
// dwords), RC k-rows by 16 doubles (stride = 32 mod 64 dwords): both make the fragment reads of a
// 32-lane ds_read_b64 group hit 32 distinct bank pairs.
template <int L, int R, int BK>
struct Img {
  static constexpr int stride = (L == KC) ? (BK + 2) : (R + 16);
  static constexpr int doubles = (L == KC) ? R * (BK + 2) : BK * (R + 16);
};
constexpr int imax(int a, int b) { return a > b ? a : b; }
// LDS doubles needed by gemm_tile<.,.,TM,TN,BK> (worst case over layouts), two buffers
template <int TM, int TN, int BK>
constexpr int gemm_smem_doubles() {
  return 2 * (imax(Img<KC, TM, BK>::doubles, Img<RC, TM, BK>::doubles) +
              imax(Img<KC, TN, BK>::doubles, Img<RC, TN, BK>::doubles));
}
// exact LDS doubles for a given layout pair (gemm_tile lays the two operand images out back to back)
template <int LA, int LB, int TM, int TN, int BK>
constexpr int gemm_smem_doubles_exact() {
  return 2 * (Img<LA, TM, BK>::doubles + Img<LB, TN, BK>::doubles);
}
#ifndef BOBE_BK128
#define BOBE_BK128 16
#endif
constexpr int BK128 = BOBE_BK128;   // 128x128 tiles: 73,728 B of LDS at BK = 16 -> two workgroups per CU
#ifndef BOBE_BK64
#define BOBE_BK64 16
#endif
constexpr int BK64 = BOBE_BK64;   // 64x64 tiles: 40,960 B of LDS -> FOUR workgroups per CU.  (Round 3: BK = 32 - 80 KB, two per CU -
                                  // made the inverse and K^-1 launches 5-8 % slower: fit 32.8 -> 31.8 ms; BK = 8: 32.5 ms)
constexpr int GEMM_SMEM_DOUBLES = gemm_smem_doubles<128, 128, BK128>();
constexpr int GEMM_SMEM_BYTES = GEMM_SMEM_DOUBLES * 8;
constexpr int GEMM64_SMEM_BYTES = gemm_smem_doubles<64, 64, BK64>() * 8;
// 32 x 32 tiles serve launches that are bound by the latency of ONE workgroup's K loop (few MFMAs per K-step): K-steps of 32
// halve the global -> LDS round trips (49,152 B of LDS, three workgroups per CU)
constexpr int BK32 = 32;
template <int T> struct TileCfg { static constexpr int bk = (T == 128) ? BK128 : (T == 64 ? BK64 : BK32); };
constexpr int GEMM32_SMEM_BYTES = gemm_smem_doubles<32, 32, BK32>() * 8;
// The Cholesky's trailing update (k_syrk_trail, chol_kernels.hpp) and the update fillers of its panel launch
// (k_chol_panel<true, .>) take K-steps and LDS budgets of their own.  They sit here so that the launches (gp_factor.hip) and
// the tile-core harness (gp_tile_harness.hip) read the same numbers.
constexpr int SYRK32_BK = 128, SYRK64_BK = 16;   // BK = 128 = the whole panel: one stage, one LDS buffer
constexpr int SYRK32_SMEM = gemm_smem_doubles_exact<KC, KC, 32, 32, SYRK32_BK>() * 8 / 2;  //  66,560 B (single buffer)
constexpr int SYRK64_SMEM = gemm_smem_doubles_exact<KC, KC, 64, 64, SYRK64_BK>() * 8;      //  36,864 B -> four workgroups per CU
constexpr int FILL_BK = 32;
constexpr int FILL_SMEM_DOUBLES = gemm_smem_doubles_exact<KC, KC, 64, 64, FILL_BK>();   // per group; two groups fit the panel's 150 KB

// ---- global -> register staging (R*BK/512 x 16 B per thread per operand) -----------------------
template <int L, int R, int BK>
__device__ __forceinline__ void stage_load(v2d (&reg)[R * BK / 512], const double* __restrict__ p, int64_t ld,
                                           int64_t r0, int64_t k0, int t) {
  if (L == KC) {
    constexpr int VPR = BK / 2;            // 16-byte vectors per row
    const int kq = t % VPR;
    const int r = t / VPR;
#pragma unroll
    for (int i = 0; i < R * BK / 512; ++i)
      reg[i] = *reinterpret_cast<const v2d*>(p + (r0 + r + (256 / VPR) * i) * ld + k0 + 2 * kq);
  } else {
    constexpr int VPR = R / 2;             // 16-byte vectors per k-row
    const int c = t % VPR;
    const int k = t / VPR;
#pragma unroll
    for (int i = 0; i < R * BK / 512; ++i)
      reg[i] = *reinterpret_cast<const v2d*>(p + (k0 + k + (256 / VPR) * i) * ld + r0 + 2 * c);
  }
}

template <int L, int R, int BK>
__device__ __forceinline__ void stage_store(const v2d (&reg)[R * BK / 512], double* img, int t) {
  if (L == KC) {
    constexpr int VPR = BK / 2;
    const int kq = t % VPR;
    const int r = t / VPR;
#pragma unroll
    for (int i = 0; i < R * BK / 512; ++i)
      *reinterpret_cast<v2d*>(img + (r + (256 / VPR) * i) * (BK + 2) + 2 * kq) = reg[i];
  } else {
    constexpr int VPR = R / 2;
    const int c = t % VPR;
    const int k = t / VPR;
#pragma unroll
    for (int i = 0; i < R * BK / 512; ++i)
      *reinterpret_cast<v2d*>(img + (k + (256 / VPR) * i) * (R + 16) + 2 * c) = reg[i];
  }
}

// fragment read: 16-row sub-tile s of the wave's rows starting at woff, k-step ks (0..BK/4-1)
template <int L, int R, int BK>
__device__ __forceinline__ double frag_read(const double* img, int woff, int s, int ks, int lane) {
  if (L == KC)
    return img[(woff + 16 * s + (lane & 15)) * (BK + 2) + 4 * ks + (lane >> 4)];
  else
    return img[(4 * ks + (lane >> 4)) * (R + 16) + woff + 16 * s + (lane & 15)];
}

template <int FM, int FN>
__device__ __forceinline__ void acc_zero(v4d (&acc)[FM][FN]) {
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
}

// ---- in-kernel stamps of the K loop (diagnostic build only: tools/gemm_stamps.hip defines BOBE_GEMM_STAMPS) --------------
// Per wave: s_memtime / s_memrealtime around the loop and s_memtime sums of four segments per K-step,
//   0 first-fragment wait    1 MFMA body    2 staging wait (+ ds_write on the register-staged loop)    3 barrier
// written by lane 0 into g_stamps[((blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 8 + ...] with ordinary vector
// stores; no output reads them.  Each stamp waits lgkmcnt(0), so the stamped build is slower than the product.
#ifdef BOBE_GEMM_STAMPS
__device__ unsigned long long* g_stamps;
__device__ __forceinline__ unsigned long long stamp_time() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
__device__ __forceinline__ unsigned long long stamp_real() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
struct Stamps {
  unsigned long long t0, r0, last, seg[4], steps;
  __device__ __forceinline__ void begin() {
    r0 = stamp_real();
    t0 = last = stamp_time();
    seg[0] = seg[1] = seg[2] = seg[3] = steps = 0;
  }
  __device__ __forceinline__ void mark(int i) {
    const unsigned long long t = stamp_time();
    seg[i] += t - last;
    last = t;
  }
  __device__ __forceinline__ void end(int tid) {
    const unsigned long long t1 = stamp_time(), r1 = stamp_real();
    if ((tid & 63) == 0 && g_stamps) {
      unsigned long long* o = g_stamps + ((blockIdx.y * gridDim.x + blockIdx.x) * 4 + (tid >> 6)) * 8;
      o[0] = t1 - t0;
      o[1] = r1 - r0;
      o[2] = seg[0];
      o[3] = seg[1];
      o[4] = seg[2];
      o[5] = seg[3];
      o[6] = steps;
      o[7] = 1;
    }
  }
};
#define BOBE_STAMPS_DECL Stamps st_; st_.begin();
#define BOBE_STAMP(i) st_.mark(i)
#define BOBE_STAMP_STEP() (++st_.steps)
#define BOBE_STAMP_VMWAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define BOBE_STAMPS_END(tid) st_.end(tid)
#else
#define BOBE_STAMPS_DECL
#define BOBE_STAMP(i)
#define BOBE_STAMP_STEP()
#define BOBE_STAMP_VMWAIT()
#define BOBE_STAMPS_END(tid)
#endif

// acc += A(m0.., k) * B(n0.., k) for k in [kbeg, kend); (kend - kbeg) must be a multiple of BK
// (K ranges are multiples of 128 for the 128x128 callers and of 64 for the 64x64 callers).
// smem: gemm_smem_doubles<TM,TN,BK>() doubles.  All 256 threads must call.  `tid` (0..255) is the thread's index
// inside its 256-thread tile group: threadIdx.x for the one-tile-per-workgroup kernels; the filler groups of the panel
// launch (k_chol_panel<true, .>) are two tile groups in one 512-thread workgroup, each with its own smem slice - the
// barriers inside are workgroup-wide, so both groups must run the same number of K-steps.
// NEGA: accumulate -A*B (the A fragment is negated on the way into the MFMA).
// TRIL: the A operand is LOWER TRIANGULAR in its last TM columns of K (A(m0 + r, kend - TM + c) = 0 for c > r: the
// diagonal block of a triangular matrix closes the K range).  In those K-steps the MFMAs of 4-column groups that lie wholly
// right of a 16-row fragment's last row are skipped - exact zeros times finite numbers: the accumulators keep their bits
// (up to the sign of a zero).  The steps before the block run the plain loop body (a predicate in every step cost the
// sweep GEMM 2.7 %; this form gains it 1.2 %; on 64 x 64 tiles - the inverse's launches - the skips cost more than they
// save: 4 MFMAs per K group and fragment row there).
template <int LA, int LB, int TM = 128, int TN = 128, int BK = BK128, bool NEGA = false, bool TRIL = false>
__device__ __forceinline__ void gemm_tile(v4d (&acc)[TM / 32][TN / 32], const double* __restrict__ A, int64_t lda,
                                          int64_t m0, const double* __restrict__ B, int64_t ldb, int64_t n0,
                                          int64_t kbeg, int64_t kend, double* smem, int tid = threadIdx.x) {
  constexpr int FM = TM / 32, FN = TN / 32;
  constexpr int IA = Img<LA, TM, BK>::doubles;
  constexpr int IB = Img<LB, TN, BK>::doubles;
  const int t = tid;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int wm = (wave >> 1) * (TM / 2);
  const int wn = (wave & 1) * (TN / 2);
  if (kend <= kbeg) return;
  v2d ra[TM * BK / 512], rb[TN * BK / 512];
  stage_load<LA, TM, BK>(ra, A, lda, m0, kbeg, t);
  stage_load<LB, TN, BK>(rb, B, ldb, n0, kbeg, t);
  stage_store<LA, TM, BK>(ra, smem, t);
  stage_store<LB, TN, BK>(rb, smem + IA, t);
  __syncthreads();
  BOBE_STAMPS_DECL
  int buf = 0;
  // one K-step: next step's operands on their way, this step's MFMAs, next step's LDS image.  IN (a constant): the step
  // lies inside the closing diagonal block of a TRIL operand, `rel` = its first column there
  const int wmu = TRIL ? __builtin_amdgcn_readfirstlane(wm) : 0;
  auto kstep = [&](int64_t k0, auto in_c, int rel) {
    constexpr bool IN = decltype(in_c)::value;
    const bool more = (k0 + BK) < kend;
    if (more) {
      stage_load<LA, TM, BK>(ra, A, lda, m0, k0 + BK, t);
      stage_load<LB, TN, BK>(rb, B, ldb, n0, k0 + BK, t);
    }
    const double* ia = smem + buf * (IA + IB);
    const double* ib = ia + IA;
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      double a[FM], b[FN];
#pragma unroll
      for (int s = 0; s < FM; ++s) {
        a[s] = frag_read<LA, TM, BK>(ia, wm, s, ks, lane);
        if (NEGA) a[s] = -a[s];
      }
#pragma unroll
      for (int s = 0; s < FN; ++s) b[s] = frag_read<LB, TN, BK>(ib, wn, s, ks, lane);
      if (ks == 0) BOBE_STAMP(0);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if (IN && rel + 4 * ks > wmu + 16 * i + 15) continue;       // columns right of the fragment's rows: zeros
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    BOBE_STAMP(1);
    if (more) {
      double* na = smem + (buf ^ 1) * (IA + IB);
      stage_store<LA, TM, BK>(ra, na, t);
      stage_store<LB, TN, BK>(rb, na + IA, t);
    }
    BOBE_STAMP(2);
    __syncthreads();
    BOBE_STAMP(3);
    BOBE_STAMP_STEP();
    buf ^= 1;
  };
  const int64_t kd = TRIL ? (kend - TM > kbeg ? kend - TM : kbeg) : kend;      // start of the closing diagonal block
  for (int64_t k0 = kbeg; k0 < kd; k0 += BK) kstep(k0, std::false_type(), 0);
  if (TRIL)
    for (int64_t k0 = kd; k0 < kend; k0 += BK) kstep(k0, std::true_type(), (int)(k0 - (kend - TM)));
  BOBE_STAMPS_END(t);
}

// ---- 128 x 128 and 64 x 64 tiles, BK = 16: operands straight into LDS, fragments one sub-step ahead -------------------
// The same MFMAs as gemm_tile<LA, LB, T, T, 16, NEGA, TRIL> in the same order for every accumulator, so the same bits; what
// differs is how the operands get there.
//   * Staging: buffer_load_dwordx4 ... lds (16 B per lane straight into LDS; the destination is the wave-uniform base +
//     16 B x lane).  One wave-instruction carries 1 KiB, so an operand tile of T x 16 is T / 8 of them, T / 32 per wave.  No
//     staging registers (32 VGPRs at 128 x 16 x 2 operands) and no vmcnt-gated ds_write block at the end of a K-step: the
//     next step's loads are issued at the top of the step and waited for by the barrier that closes it.
//   * A KC image cannot keep gemm_tile's 2-double row pad (an instruction covers 8 rows of 128 B), so it is [T][16] unpadded
//     with the 16-byte chunk c of row r stored at chunk c ^ ((r >> 1) & 7): each lane's SOURCE address carries the
//     permutation, the fragment read applies it again (an involution).  A 32-lane ds_read_b64 group still hits 32
//     distinct bank pairs: rows r and r + 1 differ by 32 banks, the eight row pairs by the chunk permutation.
//   * An RC image of T = 128 keeps gemm_tile's [BK][R + 16] layout: one k-row (128 doubles = 1 KiB) is one wave-instruction.
//   * An RC image of T = 64: a 64-wide k-row is only 512 B, so one instruction carries k-rows 2g and 2g + 1 and the row pad
//     cannot be kept.  The image is [16][64] with the chunks of every ODD k-row stored at c ^ 8 (element (k, r) at
//     k * 64 + (r ^ 16 (k & 1))); the source address carries the permutation, the read applies it again.  A 32-lane
//     ds_read_b64 group reads k-rows 4 ks and 4 ks + 1 at 16 consecutive r from a multiple of 16: 32 dwords each, which the
//     XOR puts in opposite halves of the 64 banks (unpadded, k-rows k and k + 1 are 128 dwords apart: the same 32 banks, a
//     two-way conflict).
//   * Fragments are double-buffered: the reads of sub-step ks + 1 are issued ahead of the MFMAs of ks.  The barrier
//     comes after the MFMAs of the third sub-step; the first sub-step of the next K-step is read right behind it, under
//     the MFMAs of the fourth.  Every fragment read has the MFMAs of one sub-step (16 at T = 128) to land in.
// One barrier per K-step (its fence drains the step's LDS loads with vmcnt(0)).  T = 128: 73,728 B of LDS or less, so two
// workgroups per CU as with gemm_tile.  T = 64: 32,768 B (two buffers of two 8 KiB images), within GEMM64_SMEM_BYTES and
// k_syrk_trail's SYRK64_SMEM, so the launches keep their occupancy.  The last K-step reloads its own slice into the idle
// buffer rather than branching round the loads (a branch there costs the fragment reads their counted waits).
// Which tiles have this core (the one place that says so; tile_gemm below asks it):
template <int T, int BK = TileCfg<T>::bk>
constexpr bool has_glds_core = (T == 64 || T == 128) && BK == 16;

template <int L, int T>
struct ImgGlds {
  static constexpr int doubles = (L == RC && T == 128) ? 16 * (128 + 16) : T * 16;
};
template <int LA, int LB, int T>
constexpr int gemm_glds_smem_doubles() { return 2 * (ImgGlds<LA, T>::doubles + ImgGlds<LB, T>::doubles); }
static_assert(gemm_glds_smem_doubles<RC, RC, 128>() <= GEMM_SMEM_DOUBLES && gemm_glds_smem_doubles<KC, RC, 128>() <= GEMM_SMEM_DOUBLES,
              "the 128-tile LDS images must fit the launches' GEMM_SMEM_BYTES");
static_assert(gemm_glds_smem_doubles<RC, RC, 64>() * 8 <= GEMM64_SMEM_BYTES, "the 64-tile LDS images must fit GEMM64_SMEM_BYTES");

// global -> LDS, one operand tile of T x 16: T / 32 wave-instructions per wave (wave w, g = w + 4i: KC rows 8g .. 8g + 7;
// RC k-row g at T = 128, k-rows 2g and 2g + 1 at T = 64)
template <int L, int T>
__device__ __forceinline__ void glds_stage(const double* __restrict__ p, int64_t ld, int64_t r0, int64_t k0, double* img,
                                           int wave, int lane) {
  // (a buffer load into LDS rather than global_load_lds: the compiler treats the latter as a FLAT access that may return
  // out of order and then waits lgkmcnt(0) for every fragment read; the resource is based at the tile's corner, so the
  // 32-bit offsets stay below 128 x ld x 8 bytes)
  const double* base = (L == KC) ? p + r0 * ld + k0 : p + k0 * ld + r0;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int i = 0; i < T / 32; ++i) {
    const int g = wave + 4 * i;
    unsigned off;
    double* dst;
    if (L == KC) {
      const int r = 8 * g + (lane >> 3);
      off = (unsigned)((r * ld + 2 * ((lane & 7) ^ ((r >> 1) & 7))) * 8);
      dst = img + 128 * g;
    } else if (T == 128) {
      off = (unsigned)((g * ld + 2 * lane) * 8);
      dst = img + (128 + 16) * g;
    } else {
      const int h = lane >> 5;                                     // k-row 2 g + h, LDS chunk lane & 31
      off = (unsigned)(((2 * g + h) * ld + 2 * ((lane & 31) ^ (8 * h))) * 8);
      dst = img + 128 * g;
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
  }
}

// fragment read from a T x 16 image: 16-row sub-tile s of the wave's rows at woff, sub-step ks.  KC: the lane's row is
// woff + 16 s + (lane & 15), its chunk 2 ks + (lane >> 5) (= 2 ks ^ (lane >> 5)), permuted by ((lane & 15) >> 1)
template <int L, int T>
__device__ __forceinline__ double frag_read_glds(const double* img, int woff, int s, int ks, int lane) {
  if (L == KC) {
    const int h = (lane >> 5) ^ ((lane & 15) >> 1);
    return img[(woff + 16 * s + (lane & 15)) * 16 + 2 * ((2 * ks) ^ h) + ((lane >> 4) & 1)];
  } else if (T == 128) {
    return img[(4 * ks + (lane >> 4)) * (128 + 16) + woff + 16 * s + (lane & 15)];
  } else {
    return img[(4 * ks + (lane >> 4)) * 64 + ((woff + 16 * s + (lane & 15)) ^ (((lane >> 4) & 1) << 4))];
  }
}

// TRIL as in gemm_tile (no 64-tile caller uses it: the skips cost more than they save there).
template <int LA, int LB, int T, bool NEGA = false, bool TRIL = false>
__device__ __forceinline__ void gemm_tile_glds(v4d (&acc)[T / 32][T / 32], const double* __restrict__ A, int64_t lda,
                                               int64_t m0, const double* __restrict__ B, int64_t ldb, int64_t n0,
                                               int64_t kbeg, int64_t kend, double* smem, int tid = threadIdx.x) {
  constexpr int BK = 16, F = T / 32;
  static_assert(has_glds_core<T, BK>, "no direct-to-LDS core for this tile");
  constexpr int IA = ImgGlds<LA, T>::doubles, IB = ImgGlds<LB, T>::doubles;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (wave >> 1) * (T / 2);
  const int wn = (wave & 1) * (T / 2);
  if (kend <= kbeg) return;
  auto stage = [&](int64_t k0, int b) {
    double* ia = smem + b * (IA + IB);
    glds_stage<LA, T>(A, lda, m0, k0, ia, wave, lane);
    glds_stage<LB, T>(B, ldb, n0, k0, ia + IA, wave, lane);
  };
  double fa[2][F], fb[2][F];
  auto frags = [&](double (&a)[F], double (&b)[F], const double* ia, int ks) {
#pragma unroll
    for (int s = 0; s < F; ++s) a[s] = frag_read_glds<LA, T>(ia, wm, s, ks, lane);
#pragma unroll
    for (int s = 0; s < F; ++s) b[s] = frag_read_glds<LB, T>(ia + IA, wn, s, ks, lane);
  };
  stage(kbeg, 0);
  __syncthreads();
  BOBE_STAMPS_DECL
  frags(fa[0], fb[0], smem, 0);
  BOBE_STAMP(0);
  int buf = 0;
  auto kstep = [&](int64_t k0, auto in_c, int rel) {
    constexpr bool IN = decltype(in_c)::value;
    const bool more = (k0 + BK) < kend;
    // (NEGA negates A in the MFMA phase, a sub-step after its read: negated where it is read, every sub-step would wait
    // for the reads it has just issued)
    auto mfmas = [&](int ks) {
#pragma unroll
      for (int i = 0; i < F; ++i) {
        if (IN && rel + 4 * ks > wm + 16 * i + 15) continue;        // columns right of the fragment's rows: zeros
        const double a = NEGA ? -fa[ks & 1][i] : fa[ks & 1][i];
#pragma unroll
        for (int j = 0; j < F; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, fb[ks & 1][j], acc[i][j], 0, 0, 0);
      }
    };
    stage(more ? k0 + BK : k0, buf ^ 1);
    const double* ia = smem + buf * (IA + IB);
    // (the phases are pinned: left alone, the scheduler sinks the reads of a sub-step behind the MFMAs that should hide them)
#pragma unroll
    for (int ks = 0; ks < BK / 4 - 1; ++ks) {
      frags(fa[(ks + 1) & 1], fb[(ks + 1) & 1], ia, ks + 1);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(ks);
      __builtin_amdgcn_sched_barrier(0);
    }
    BOBE_STAMP(1);
    BOBE_STAMP_VMWAIT();
    BOBE_STAMP(2);
    __syncthreads();
    BOBE_STAMP(3);
    BOBE_STAMP_STEP();
    buf ^= 1;
    // the next step's first sub-step is read under the MFMAs of this step's last one (whose fragments are in set 1)
    frags(fa[0], fb[0], smem + buf * (IA + IB), 0);
    __builtin_amdgcn_sched_barrier(0);
    mfmas(BK / 4 - 1);
    __builtin_amdgcn_sched_barrier(0);
    BOBE_STAMP(0);
  };
  const int64_t kd = TRIL ? (kend - T > kbeg ? kend - T : kbeg) : kend;        // start of the closing diagonal block
  for (int64_t k0 = kbeg; k0 < kd; k0 += BK) kstep(k0, std::false_type(), 0);
  if (TRIL)
    for (int64_t k0 = kd; k0 < kend; k0 += BK) kstep(k0, std::true_type(), (int)(k0 - (kend - T)));
  BOBE_STAMPS_END(tid);
}

// ---- the one way to ask for a tile product: acc += A(m0.., k) * B(n0.., k), k in [kbeg, kend) ---------------------------
// GLDS, a constant written at every call site (a kernel's tile core is a property of the kernel; nothing picks it at run
// time): take the direct-to-LDS core where the tile has one (has_glds_core), else - and with GLDS = false always - the
// register-staged gemm_tile; the bits are the same either way.  smem: the launch's GEMM_SMEM_BYTES / GEMM64_SMEM_BYTES /
// GEMM32_SMEM_BYTES serve both cores.
template <bool GLDS, int LA, int LB, int T, bool NEGA = false, bool TRIL = false, int BK = TileCfg<T>::bk>
__device__ __forceinline__ void tile_gemm(v4d (&acc)[T / 32][T / 32], const double* __restrict__ A, int64_t lda, int64_t m0,
                                          const double* __restrict__ B, int64_t ldb, int64_t n0, int64_t kbeg, int64_t kend,
                                          double* smem, int tid = threadIdx.x) {
  if constexpr (GLDS && has_glds_core<T, BK>)
    gemm_tile_glds<LA, LB, T, NEGA, TRIL>(acc, A, lda, m0, B, ldb, n0, kbeg, kend, smem, tid);
  else
    gemm_tile<LA, LB, T, T, BK, NEGA, TRIL>(acc, A, lda, m0, B, ldb, n0, kbeg, kend, smem, tid);
}

// Coordinates of accumulator element (i, j, r) of this lane inside the TM x TN tile.
template <int TM = 128>
__device__ __forceinline__ int acc_row(int i, int r, int tid = threadIdx.x) {
  const int t = tid;
  return ((t >> 6) >> 1) * (TM / 2) + 16 * i + ((t & 63) >> 4) + 4 * r;
}
template <int TN = 128>
__device__ __forceinline__ int acc_col(int j, int tid = threadIdx.x) {
  const int t = tid;
  return ((t >> 6) & 1) * (TN / 2) + 16 * j + (t & 15);
}

// C[m0+row][n0+col] = alpha*acc + beta*C   (row-major C, ldc)
template <int TM = 128, int TN = 128>
__device__ __forceinline__ void store_tile(const v4d (&acc)[TM / 32][TN / 32], double* __restrict__ C, int64_t ldc,
                                           int64_t m0, int64_t n0, double alpha, double beta, int tid = threadIdx.x) {
#pragma unroll
  for (int i = 0; i < TM / 32; ++i)
#pragma unroll
    for (int j = 0; j < TN / 32; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double* q = C + (m0 + acc_row<TM>(i, r, tid)) * ldc + n0 + acc_col<TN>(j, tid);
        double v = alpha * acc[i][j][r];
        if (beta != 0.0) v += beta * (*q);
        *q = v;
      }
}

// acc = C[m0+row][n0+col]  (issued early so the loads overlap the operand staging)
template <int TM = 128, int TN = 128>
__device__ __forceinline__ void load_tile(v4d (&acc)[TM / 32][TN / 32], const double* __restrict__ C, int64_t ldc,
                                          int64_t m0, int64_t n0, int tid = threadIdx.x) {
#pragma unroll
  for (int i = 0; i < TM / 32; ++i)
#pragma unroll
    for (int j = 0; j < TN / 32; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = C[(m0 + acc_row<TM>(i, r, tid)) * ldc + n0 + acc_col<TN>(j, tid)];
}

// map a linear index to a lower-triangular tile (i >= j), row-major enumeration: t = i(i+1)/2 + j
__device__ __forceinline__ void tri_decode(int t, int& i, int& j) {
  int ii = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((ii + 1) * (ii + 2) / 2 <= t) ++ii;
  while (ii * (ii + 1) / 2 > t) --ii;
  i = ii;
  j = t - ii * (ii + 1) / 2;
}

// ---- workgroup -> tile maps that keep a launch's operand panels in ONE XCD's L2 ------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (hardware ids b and b + 8 share an L2; MI355X_MICROARCH
// "Workgroup dispatch"), and an XCD starts its share in id order.  For launches whose workgroups all do the same
// amount of work, xcd_share() gives every XCD one CONTIGUOUS share of `per` logical ids (grid = 8 * per, ids past the
// tile count exit), and tri_grouped() / rect_grouped() enumerate tiles in 8 x 8 groups, so that the tiles an XCD has
// in flight share 8 A panels and 8 B panels instead of pulling one of each per tile through the fabric.  per <= 0:
// identity.  A pure speed choice: which workgroup computes a tile never changes the tile's bits.  Measured (round 2):
// nothing at N = 4096 (the panels of the default row-major order already stay in L2), 1.5-2.5 % at N = 8192.
// Launches with tiles of unequal length keep the row-major heavy-first order: runs of 64 logical ids dealt round-robin
// were 8-12 % SLOWER (a launch has only ~230 tiles per XCD, whole runs leave some XCDs a quarter more tiles than
// others), and equal-WORK contiguous shares cut on the host made the K^-1 launch 8 % slower (1.90 -> 2.05 ms for four
// matrices: the XCDs then hold tiles of very different length while ids are still handed out in order).
__device__ __forceinline__ int xcd_share(int b, int per) { return per > 0 ? (b & 7) * per + (b >> 3) : b; }

// lower triangle of an n x n tile grid: bands of 8 tile rows (top band first); inside a band the 8-column groups left
// to right, each row-major, then the band's diagonal triangle
__device__ __forceinline__ void tri_grouped(int t, int n, int& i, int& j) {
  int ii, jj;
  tri_decode(t, ii, jj);                       // (band boundaries coincide with row boundaries of the row-major order)
  const int R = ii & ~7;
  const int h = min(8, n - R);
  const int u = t - R * (R + 1) / 2;
  if (u < R * h) {
    const int g = u / (8 * h), w = u - g * 8 * h;
    i = R + (w >> 3);
    j = 8 * g + (w & 7);
  } else {
    tri_decode(u - R * h, ii, jj);
    i = R + ii;
    j = R + jj;
  }
}

// rows x cols tile grid: bands of 8 rows, inside a band groups of 8 columns, each group row-major
__device__ __forceinline__ void rect_grouped(int e, int rows, int cols, int& i, int& j) {
  const int r = e / (8 * cols);
  const int h = min(8, rows - 8 * r);
  const int u = e - r * 8 * cols;
  const int g = u / (8 * h);
  const int gw = min(8, cols - 8 * g);
  const int w = u - g * 8 * h;
  i = 8 * r + w / gw;
  j = 8 * g + w % gw;
}

}  // namespace bobe
