// libbobe_gp.so, tile-core harness unit: runs ONE instantiation of tile_gemm (gemm_f64.hpp) on caller-supplied operands,
// framed as every shipped kernel frames it - acc = load_tile(C) or 0, tile_gemm, store_tile - so that a test can hold each
// instantiation to an exact product (tests/test_gpu_tile_gemm.py).  A test hook: no shipped launch passes through here.
// What it does NOT cover: the shipped kernels' own code generation (their launch bounds differ from k_debug_tile_gemm's),
// their workgroup -> tile maps and the arithmetic of their K ranges.
#include "gp_handle.hpp"

using namespace bobe;

namespace {

// One row per instantiation the library ships (plus the two remaining layouts of k_debug_gemm); a new tile_gemm
// instantiation gets a row here and in the test's table.  Three register-staged rows - (64, 16, RC, RC), (64, 16, KC, RC)
// and (64, SYRK64_BK, KC, KC, NEGA) - belong to no shipped launch any more (those kernels run the direct-to-LDS core): they
// stay as the reference their direct-to-LDS twins are compared with, bit for bit.  Columns:
//   T, BK, GLDS, LA, LB, NEGA, TRIL, groups (256-thread tile groups per workgroup), single_buffer, dynamic LDS of the
//   shipped launch in bytes (for groups = 2: of both groups together; group g takes the g-th half)
// single_buffer: the launch has LDS for ONE pair of operand images, so the K range is one K-step.
#define BOBE_TILE_GEMM_VARIANTS(X)                                               \
  X(128, 16, true, RC, RC, false, false, 1, false, GEMM_SMEM_BYTES)              \
  X(128, 16, false, RC, RC, false, false, 1, false, GEMM_SMEM_BYTES)             \
  X(128, 16, true, KC, RC, false, false, 1, false, GEMM_SMEM_BYTES)              \
  X(128, 16, false, KC, RC, false, false, 1, false, GEMM_SMEM_BYTES)             \
  X(128, 16, true, KC, RC, false, true, 1, false, GEMM_SMEM_BYTES)               \
  X(128, 16, false, KC, RC, false, true, 1, false, GEMM_SMEM_BYTES)              \
  X(128, 16, false, KC, KC, false, false, 1, false, GEMM_SMEM_BYTES)             \
  X(128, 16, false, RC, KC, false, false, 1, false, GEMM_SMEM_BYTES)             \
  X(64, 16, true, RC, RC, false, false, 1, false, GEMM64_SMEM_BYTES)             \
  X(64, 16, false, RC, RC, false, false, 1, false, GEMM64_SMEM_BYTES)            \
  X(64, 16, true, KC, RC, false, false, 1, false, GEMM64_SMEM_BYTES)             \
  X(64, 16, false, KC, RC, false, false, 1, false, GEMM64_SMEM_BYTES)            \
  X(64, SYRK64_BK, true, KC, KC, true, false, 1, false, SYRK64_SMEM)             \
  X(64, SYRK64_BK, false, KC, KC, true, false, 1, false, SYRK64_SMEM)            \
  X(64, FILL_BK, false, KC, KC, true, false, 2, false, 2 * FILL_SMEM_DOUBLES * 8) \
  X(32, 32, false, RC, RC, false, false, 1, false, GEMM32_SMEM_BYTES)            \
  X(32, 32, false, KC, RC, false, false, 1, false, GEMM32_SMEM_BYTES)            \
  X(32, SYRK32_BK, false, KC, KC, true, false, 1, true, SYRK32_SMEM)

// Tile (p, q) of the grid: p = blockIdx.y, q = GROUPS * blockIdx.x + group.  With GROUPS = 2 the workgroup is two tile
// groups as in k_chol_panel<true, .>: tid = threadIdx.x & 255 and the group's own LDS slice.
template <bool GLDS, int LA, int LB, int T, int BK, bool NEGA, bool TRIL, int GROUPS, int SMEM>
__global__ __launch_bounds__(256 * GROUPS) void k_debug_tile_gemm(const double* A, int64_t lda, const double* B, int64_t ldb,
                                                                  double* C, int64_t ldc, int64_t m0, int64_t n0,
                                                                  int64_t kbeg, int64_t kend, double alpha, double beta,
                                                                  int preload) {
  extern __shared__ double smem[];
  const int grp = GROUPS == 2 ? (int)(threadIdx.x >> 8) : 0;
  const int tid = GROUPS == 2 ? (int)(threadIdx.x & 255) : (int)threadIdx.x;
  const int64_t r0 = m0 + (int64_t)blockIdx.y * T, c0 = n0 + ((int64_t)blockIdx.x * GROUPS + grp) * T;
  v4d acc[T / 32][T / 32];
  if (preload) load_tile<T, T>(acc, C, ldc, r0, c0, tid);
  else acc_zero(acc);
  tile_gemm<GLDS, LA, LB, T, NEGA, TRIL, BK>(acc, A, lda, r0, B, ldb, c0, kbeg, kend, smem + grp * (SMEM / 8 / GROUPS), tid);
  store_tile<T, T>(acc, C, ldc, r0, c0, alpha, beta, tid);
}

using TileKern = void (*)(const double*, int64_t, const double*, int64_t, double*, int64_t, int64_t, int64_t, int64_t,
                          int64_t, double, double, int);
struct TileVariant {
  int T, BK, glds, la, lb, nega, tril, groups, single_buffer, smem;
  TileKern fn;
};
#define X(T, BK, GL, LA, LB, NE, TR, GR, SB, SM) \
  {T, BK, GL, LA, LB, NE, TR, GR, SB, SM, k_debug_tile_gemm<GL, LA, LB, T, BK, NE, TR, GR, SM>},
const TileVariant g_variants[] = {BOBE_TILE_GEMM_VARIANTS(X)};
#undef X
constexpr int NVARIANTS = (int)(sizeof(g_variants) / sizeof(g_variants[0]));

void configure_tile_harness() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  for (const TileVariant& v : g_variants) allow_big_lds(v.fn, v.smem);
}

#define NEED(cond, msg) \
  if (!(cond)) throw Err(BOBE_ERR_ARG, msg)

// half-open rectangle [r0, r1) x [c0, c1) of a row-major matrix
struct Rect { int64_t r0, r1, c0, c1; };
bool meets(const Rect& a, const Rect& b) { return a.r0 < b.r1 && b.r0 < a.r1 && a.c0 < b.c1 && b.c0 < a.c1; }
// what tile_gemm reads of an operand whose rows [x0, x1) take part: KC element (r, k) at [r][k], RC at [k][r]
Rect operand_rect(int layout, int64_t x0, int64_t x1, int64_t kbeg, int64_t kend) {
  return layout == KC ? Rect{x0, x1, kbeg, kend} : Rect{kbeg, kend, x0, x1};
}

int run_tile_gemm(int device, int variant, int tiles_m, int tiles_n, int64_t m0, int64_t n0, int64_t kbeg, int64_t kend,
                  const double* A, int64_t lda, int64_t rows_a, const double* B, int64_t ldb, int64_t rows_b, double* C,
                  int64_t ldc, int64_t rows_c, double alpha, double beta, int preload) {
  NEED(variant >= 0 && variant < NVARIANTS, "unknown tile_gemm variant");
  const TileVariant& v = g_variants[variant];
  NEED(A && B && C, "NULL argument");
  NEED(tiles_m >= 1 && tiles_n >= 1 && tiles_m <= 64 && tiles_n <= 64, "tile grid must be 1 .. 64 each way");
  NEED(lda > 0 && ldb > 0 && ldc > 0 && lda % 2 == 0 && ldb % 2 == 0 && ldc % 2 == 0, "leading dimensions must be even");
  NEED(m0 >= 0 && n0 >= 0 && kbeg >= 0 && m0 % v.T == 0 && n0 % v.T == 0 && kbeg % v.T == 0,
       "m0, n0 and kbeg must be multiples of the tile edge");
  NEED(kend > kbeg && (kend - kbeg) % v.BK == 0, "kend - kbeg must be a positive multiple of the K-step");
  NEED(!v.single_buffer || kend - kbeg == v.BK, "a single-buffer variant takes exactly one K-step");
  NEED(tiles_n % v.groups == 0, "a two-group variant needs an even number of tile columns");
  // every address the kernel touches lies inside the arrays it was given
  const int64_t m1 = m0 + (int64_t)tiles_m * v.T, n1 = n0 + (int64_t)tiles_n * v.T;
  NEED(rows_a > 0 && rows_b > 0 && rows_c > 0 && rows_a < (1 << 20) && rows_b < (1 << 20) && rows_c < (1 << 20) &&
           lda < (1 << 20) && ldb < (1 << 20) && ldc < (1 << 20), "array extents must be in (0, 2^20)");
  const Rect ra = operand_rect(v.la, m0, m1, kbeg, kend), rb = operand_rect(v.lb, n0, n1, kbeg, kend), rc{m0, m1, n0, n1};
  NEED(ra.r1 <= rows_a && ra.c1 <= lda, "the A operand does not fit rows_a x lda");
  NEED(rb.r1 <= rows_b && rb.c1 <= ldb, "the B operand does not fit rows_b x ldb");
  NEED(rc.r1 <= rows_c && rc.c1 <= ldc, "the C tiles do not fit rows_c x ldc");
  // arrays passed twice share one device buffer (k_syrk_trail's in-place form): same shape, and no tile may be written
  // where another workgroup still reads an operand
  const bool ab = (A == B), ac = (A == C), bc = (B == C);
  NEED(!ab || (lda == ldb && rows_a == rows_b), "A == B with different shapes");
  NEED(!ac || (lda == ldc && rows_a == rows_c), "A == C with different shapes");
  NEED(!bc || (ldb == ldc && rows_b == rows_c), "B == C with different shapes");
  NEED(!ac || !meets(ra, rc), "A == C: the K range runs into the tiles being written");
  NEED(!bc || !meets(rb, rc), "B == C: the K range runs into the tiles being written");

  HIPCHK(hipSetDevice(device));
  configure_tile_harness();
  CallBuf da, db, dc;
  const size_t na = (size_t)rows_a * lda * 8, nb = (size_t)rows_b * ldb * 8, nc = (size_t)rows_c * ldc * 8;
  dc.ensure(nc);
  HIPCHK(hipMemcpy(dc.p, C, nc, hipMemcpyHostToDevice));
  const double *pa, *pb;
  if (ac) pa = dc.d();
  else { da.ensure(na); HIPCHK(hipMemcpy(da.p, A, na, hipMemcpyHostToDevice)); pa = da.d(); }
  if (bc) pb = dc.d();
  else if (ab) pb = pa;
  else { db.ensure(nb); HIPCHK(hipMemcpy(db.p, B, nb, hipMemcpyHostToDevice)); pb = db.d(); }
  hipLaunchKernelGGL(v.fn, dim3((unsigned)(tiles_n / v.groups), (unsigned)tiles_m), dim3(256 * v.groups), v.smem, 0, pa, lda,
                     pb, ldb, dc.d(), ldc, m0, n0, kbeg, kend, alpha, beta, preload);
  LAUNCH_CHECK();
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(C, dc.p, nc, hipMemcpyDeviceToHost));
  return BOBE_OK;
}

}  // namespace

extern "C" {

int bobe_debug_tile_gemm_count(void) { return NVARIANTS; }

int bobe_debug_tile_gemm_info(int variant, int* info9) {
  try {
    NEED(variant >= 0 && variant < NVARIANTS, "unknown tile_gemm variant");
    NEED(info9, "NULL argument");
    const TileVariant& v = g_variants[variant];
    const int f[9] = {v.T, v.BK, v.glds, v.la, v.lb, v.nega, v.tril, v.groups, v.single_buffer};
    std::copy(f, f + 9, info9);
    return BOBE_OK;
  } catch (const Err& e) {
    g_err = e.what();
    return e.code;
  }
}

int bobe_debug_tile_gemm(int device, int variant, int tiles_m, int tiles_n, int64_t m0, int64_t n0, int64_t kbeg,
                         int64_t kend, const double* A, int64_t lda, int64_t rows_a, const double* B, int64_t ldb,
                         int64_t rows_b, double* C, int64_t ldc, int64_t rows_c, double alpha, double beta, int preload) {
  try {
    return run_tile_gemm(device, variant, tiles_m, tiles_n, m0, n0, kbeg, kend, A, lda, rows_a, B, ldb, rows_b, C, ldc,
                         rows_c, alpha, beta, preload);
  } catch (const Err& e) {
    g_err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_err = e.what();
    return BOBE_ERR_HIP;
  } catch (...) {
    g_err = "unknown error";
    return BOBE_ERR_HIP;
  }
}

}  // extern "C"
