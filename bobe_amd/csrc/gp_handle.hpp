// The handle behind include/bobe_gp.h (struct bobe_gp) and the host helpers shared by the translation units of
// libbobe_gp.so:
//   gp_factor.hip     K(X,X) assembly, blocked Cholesky + launch plan, triangular inverse, alpha, MLL value / gradient
//                     (single evaluation, evaluation slots, lock-step batch, graph replay), state restore
//   gp_sweep.hip      prediction / acquisition sweep, score and posterior gradients, rank-b append.  (Its few-candidate
//                     gradient chain and gp_criteria.hip's share wg_front, the device code of wg_kernels.hpp and the host
//                     staging below: wg_candidates, WgFront, WgOut, WG_MAX_N.)
//   gp_consumers.hip  HMC / NUTS / constrained random walks on the surrogate, EI / LogEI, the classifier gate, GP.kernel,
//                     device clone.  (What its chain kernels share with gp_paths.hip's - the rows' homes, the one-point
//                     evaluation, the HMC transition - is chain_common.hpp; the host staging of a chain call is ChainStage,
//                     below.)
//   gp_posterior.hip  joint posterior covariance at query points and correlated draws from it
//   gp_loo.hip        leave-one-out predictive terms of the state, the LOO objective and its gradient
//   gp_batch.hip      one-sweep batch selection for WIPV / WIPStd (the sweep's intermediates kept, rank-one downdates)
//   gp_criteria.hip   importance-weighted integration points, IMIQR / EIV: the weighted scoring pass of the sweep and the batch,
//                     the input gradients of the four scores (few-candidate chain); the total variance of the evidence estimate
//                     over the integration points (the pair sum on the 128-tile core)
//   gp_paths.hip      pathwise posterior draws of the latent surrogate (random Fourier features + Matheron's rule): path
//                     sets, their evaluation at query points and per-path argmax, input gradients, whole HMC chains on a path
//   gp_abi.hip        the extern "C" layer, the RCCL exchange step, test / bench hooks
//   gp_tile_harness.hip  test hook: one tile_gemm instantiation per call on caller-supplied operands
// Host side only: buffer management, launch sequencing, host/device pointer handling.  No CPU compute path exists:
// without a HIP device every entry point fails with BOBE_ERR_HIP.
#pragma once
#include "../../include/bobe_gp.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "gemm_f64.hpp"
#include "gp_types.hpp"

namespace bobe {

struct Err : std::runtime_error {
  int code;
  Err(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

extern thread_local std::string g_err;     // text behind bobe_last_error() (gp_abi.hip)

#define HIPCHK(expr)                                                                                           \
  do {                                                                                                         \
    hipError_t e_ = (expr);                                                                                    \
    if (e_ != hipSuccess)                                                                                      \
      throw ::bobe::Err(BOBE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                          std::to_string(__LINE__) + ")");                                     \
  } while (0)

#define LAUNCH_CHECK() HIPCHK(hipGetLastError())

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

inline bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

struct DBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void ensure(size_t b) {
    if (b <= bytes) return;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    bytes = 0;
    HIPCHK(hipMalloc(&p, b));
    bytes = b;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  double* d() const { return static_cast<double*>(p); }
};

// a device buffer of one call: freed when the call returns, whichever way
struct CallBuf : DBuf {
  CallBuf() = default;
  CallBuf(const CallBuf&) = delete;
  CallBuf& operator=(const CallBuf&) = delete;
  ~CallBuf() { release(); }
};

// The staging of one chain call (hmc_run, nuts_run, paths_hmc_run), host pointers in and out, in the buffer the caller
// names: state [P][3d+2] | adapt [P][5] | mass (ni doubles: inv_mass, d or P d, or NUTS's metric, 2 d d) | hist | keep |
// stats (NUTS: nt) | dbg (nd).  An output the caller did not ask for takes no room, and its device pointer is null.
struct ChainStage {
  size_t ns, na, ni, nh, nk, nt, nd;
  double *dS, *dA, *dI, *dH, *dK, *dT, *dD;
  ChainStage(DBuf& buf, int64_t P, int d, size_t ni_, int niter, int hist_from, bool hist, int thin, bool keep, size_t nt_,
             size_t nd_)
      : ns((size_t)P * (3 * (size_t)d + 2)), na((size_t)P * 5), ni(ni_),
        nh(hist ? (size_t)(niter - hist_from) * P * d : 0), nk(keep ? (size_t)(niter / thin) * P * (d + 1) : 0), nt(nt_),
        nd(nd_) {
    buf.ensure((ns + na + ni + nh + nk + nt + nd) * sizeof(double));
    dS = buf.d();
    dA = dS + ns;
    dI = dA + na;
    double* const h0 = dI + ni;
    dH = nh ? h0 : nullptr;
    dK = nk ? h0 + nh : nullptr;
    dT = nt ? h0 + nh + nk : nullptr;
    dD = nd ? h0 + nh + nk + nt : nullptr;
  }
  void copy_in(hipStream_t stream, const double* state, const double* adapt, const double* mass) const {
    HIPCHK(hipMemcpyAsync(dS, state, ns * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dA, adapt, na * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dI, mass, ni * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  void copy_out(hipStream_t stream, double* state, double* adapt, double* hist, double* keep, double* stats,
                double* dbg) const {
    HIPCHK(hipMemcpyAsync(state, dS, ns * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(adapt, dA, na * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (dH) HIPCHK(hipMemcpyAsync(hist, dH, nh * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (dK) HIPCHK(hipMemcpyAsync(keep, dK, nk * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (dT) HIPCHK(hipMemcpyAsync(stats, dT, nt * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (dD) HIPCHK(hipMemcpyAsync(dbg, dD, nd * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
};

// The factorisation's rank test.  A pivot (L_jj^2) below 64 ulp of the kernel matrix's diagonal k(x,x) + noise is as large as
// the rounding accumulated in its column's update at N of a few thousand: it carries no information, and neither does the
// log-determinant built on it (a too small one - the optimiser is drawn to exactly these hyper-parameters).  Such a
// factorisation counts as NOT positive definite, like one with a non-positive pivot: NaN outputs, BOBE_NOT_PD.  (LAPACK's
// dpotrf, the reference's Cholesky, tests the sign only and fails or passes on the last bit in this regime)
// The factor is per handle: bobe_gp_set_pivot_floor_ulp, default from BOBE_PIVOT_FLOOR_ULP, else 0 = the rank test is OFF and
// LAPACK's rule alone holds (a pivot <= 0 or NaN fails, nothing else: the reference's behaviour).  The BO driver opts in
// with 64 (bobe_amd/bo.py).
inline double pivot_floor(const Hyper& h, double ulp) {
  const double f = ulp * 2.220446049250313e-16 * (h.kvar + h.noise);
  return f < 0.25 ? f : 0.25;                        // (the identity padding's pivots are 1)
}
// min_diag: the smallest L_jj of a factor (k_mll_terms, res[101]); NaN counts as failed
inline bool pivots_resolved(double min_diag, double floor) { return min_diag * min_diag >= floor; }
double default_pivot_floor_ulp();                    // BOBE_PIVOT_FLOOR_ULP, else 0 (the reference's sign test alone)
double default_refine_kappa();                       // BOBE_REFINE_KAPPA, else 1e6
int default_solve_block();                           // BOBE_SOLVE_BLOCK, else 128
int default_solve_panel();                           // BOBE_SOLVE_PANEL, else 512
int64_t default_solve_chunk();                       // BOBE_SOLVE_CHUNK, else 32768

template <typename K>
void allow_big_lds(K kernel, int bytes) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

// Tuning switches, read once per process from the environment (INTEGRATION.md lists them; none changes a result bit):
//   BOBE_SYRK32_BELOW   64x64-tile count below which a single-panel trailing update takes 32x32 tiles (512)
//   BOBE_TRTRI64        128-block count below which a level of the triangular inverse takes 64x64 tiles (600)
//   BOBE_PAIR_MIN       K = 256 update pairs while B * rem^2 exceeds this (300; 0: never)
//   BOBE_LOCKSTEP_MIN_N bobe_gp_mll_batch advances its evaluations in lock step from this many points (1: always)
//   BOBE_MLL_SLOTS      evaluations in flight below that size (8)
//   BOBE_GRAPH_MAX_N    a slot replays its pipeline as a hipGraph up to this many points (2048)
//   BOBE_XCD_SHARES     0: row-major tile order on every XCD (1)
//   BOBE_FILL           deferred trailing updates in the panel launches: 0 off, 1 where they pay (potrf), 2 everywhere
//   BOBE_INV_SIDE       the inverse's leading half on a side stream beside the late panel chain: 0 off, 1 where it pays
//                       (inv_side_pays), 2 wherever there are two block columns or more
//   BOBE_TRACE          print launch plans and batch timings to stderr
//   BOBE_FACTOR_REUSE   0: bobe_gp_factor always factorises, never adopts an evaluation's factor (1; for A/B runs)
struct Tuning {
  int syrk32_below, trtri64_below, pair_min, lockstep_min_n, mll_slots, graph_max_n, xcd_shares, fill, inv_side;
  bool mll_slots_set, trace, factor_reuse;
};
const Tuning& tuning();

// ---- kernel variants.  The kernels that read coordinates are templates over the family KE (0 RBF, anything else Matern)
// and the cap DC on d (8 / 16 / 32).  The host picks the instantiation here and nowhere else: f receives the choice as
// std::integral_constant values, which convert to int in template-argument position,
//   with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) { hipLaunchKernelGGL((k_x<KE, DC>), ...); });
inline int dcap_of(int d) { return d <= 8 ? 8 : (d <= 16 ? 16 : 32); }
template <typename F>
inline void with_dcap(int d, F&& f) {
  switch (dcap_of(d)) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}
template <typename F>
inline void with_kern_dcap(int kern, int d, F&& f) {
  with_dcap(d, [&](auto DC) {
    if (kern == 0) f(std::integral_constant<int, 0>{}, DC);
    else f(std::integral_constant<int, 1>{}, DC);
  });
}
template <typename F>
inline void for_each_kern_dcap(F&& f) {          // all six (KE, DC), for the configure_*_kernels functions
  for (int kern = 0; kern < 2; ++kern)
    for (int d : {8, 16, 32}) with_kern_dcap(kern, d, f);
}

constexpr int LAUUM64_BELOW = 1200;   // lower 128-tile count below which K^-1 runs on 64x64 tiles (fixes the order of the
                                      // gradient's partial sums: a function of N only)
// The tiles of K^-1 = Linv^T Linv over nb 128-blocks (k_lauum_grad, k_loo_grad): 64 x 64 tiles below LAUUM64_BELOW lower
// 128-tiles, 128 x 128 above; nt tiles per side, ntiles lower ones = the number of the gradient's partial sums.
struct LauumTiling { bool small; int nt, ntiles; };
inline LauumTiling lauum_tiling(int nb) {
  const bool small = nb * (nb + 1) / 2 < LAUUM64_BELOW;
  const int nt = small ? 2 * nb : nb;
  return {small, nt, nt * (nt + 1) / 2};
}
// with_kern_dcap extended by the tile size TT: f(KE, DC, TT)
template <typename F>
inline void with_lauum_variant(int kern, int d, const LauumTiling& t, F&& f) {
  with_kern_dcap(kern, d, [&](auto KE, auto DC) {
    if (t.small) f(KE, DC, std::integral_constant<int, 64>{});
    else f(KE, DC, std::integral_constant<int, 128>{});
  });
}

constexpr int FILL_NEAR = 2;          // the last panels of a block column always come from the update launches
constexpr int FILL_CHUNK = 3;         // panels per filler visit of a tile (a filler must not outlast the panel, ~28 us)
constexpr int FILL_SLACK = 16;        // caught-up work the plan accepts per deferred unit (1 / 16)
constexpr int FILL_PHASE = 1024;      // fillers ride in panel launches with B * rem^2 <= this

// Grid of an equal-work tile launch whose workgroups take their tile from xcd_share() (gemm_f64.hpp): `per` logical
// tiles per XCD, grid = 8 * per.  Small launches keep the plain order (per = 0).
struct TileGrid { int grid, per; };
inline TileGrid tile_grid(int ntiles) {
  if (!tuning().xcd_shares || ntiles < 256) return {ntiles, 0};
  const int per = (ntiles + 7) / 8;
  return {8 * per, per};
}

// per translation unit: raise the dynamic-LDS limit of its kernels (once per device)
void configure_factor_kernels();
void configure_sweep_kernels();
void configure_consumer_kernels();
void configure_posterior_kernels();
void configure_loo_kernels();
void configure_paths_kernels();
// their guard: true on the first call on the current device only (`done`: the translation unit's own flag per device)
inline bool first_use_on_device(bool (&done)[64]) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || done[dev]) return false;
  return done[dev] = true;
}

// Retention buffers of a sweep (SweepReq::keep; bobe_gp_wip_select_batch, gp_batch.hip): the caller's
// device buffers, all with leading dimension ld = C rounded up to 128, that receive what the sweep otherwise keeps per chunk
// or per super-chunk in the handle's workspace - CsT [d x ld] scaled candidates, V [Np x ld] = L^-1 K(X, C), crossT [Mp x ld],
// sc [ld] = s_c.  The launches and their order are the sweep's own; only the addresses they write to differ.
// V_used / ldv_used (out): where V ended up - the caller's buffer, or the handle's V_Z when the candidates are the
// integration points (that path forms no V of its own).
struct SweepKeep {
  double* CsT = nullptr;
  double* V = nullptr;
  double* crossT = nullptr;
  double* sc = nullptr;
  int64_t ld = 0;
  const double* V_used = nullptr;
  int64_t ldv_used = 0;
};

// Importance-weighted scoring of a sweep (SweepReq::w; bobe_gp_wip_sweep_w / bobe_gp_wip_select_batch_w, gp_criteria.hip).
// After prepare_z the sweep has the per-z table built (bobe_gp::wip_zterms) and scores every super-chunk with k_wip_score_w
// into out[criterion] (device memory, C each; NULL = not wanted) - next to, not instead of, what SweepReq::wipv / wipstd ask
// of the equal-weight scorer.  The buffers belong to the call.
struct SweepW {
  const double* logw = nullptr;     // M log-weights, host or device; NULL: the points are draws of the surrogate posterior
  double* out[4] = {nullptr, nullptr, nullptr, nullptr};   // wipv, wipstd, imiqr, eiv
  // the fifth output: zvar = -log T(c), the expected evidence variance's candidate term (k_wip_score_zz; bobe_gp_wip_sweep_zvar
  // / bobe_gp_wip_select_batch_zvar).  NULL: the table's lambda row and log E[Z] are not formed, no launch is added.
  double* zz = nullptr;
  CallBuf zt, zpart, lstage;        // the table [ZTERM_ROWS x Mp] + log S, the partial sums of K(X,Z)^T alpha, logw staged
  int64_t ldt = 0;
  double* log_s() const { return zt.d() + (int64_t)ZTERM_ROWS * ldt; }   // (zt holds 8 doubles behind the table)
  double* log_ez() const { return log_s() + 1; }
};

// What bobe_debug_batch_terms adds to a batch selection (bobe_gp::select_batch, gp_batch.hip): picks applied in place of the
// argmins and the downdated state copied out.  Host pointers, every one may be NULL; the outputs are written without padding.
struct BatchDebug {
  const int64_t* forced = nullptr;  // n_batch - 1 picks: forced[j] replaces stage j's argmin before stage j + 1 reads it
  double* crossT = nullptr;         // M x C
  double* sc = nullptr;             // C
  double* basez = nullptr;          // M, the call's copy
  double* UC = nullptr;             // (n_batch - 1) x C
  double* UZ = nullptr;             // (n_batch - 1) x M
};

// What bobe_gp::sweep is asked for: C candidates, optionally scored against M integration points Z (Z = NULL: prediction
// only).  Every output may be NULL (host or device memory otherwise; the argmin / min ones are host scalars).
struct SweepReq {
  const double* cand = nullptr;
  int64_t C = 0;
  const double* Z = nullptr;
  int64_t M = 0;
  double y_std = 1.0;
  double* wipv = nullptr;
  double* wipstd = nullptr;
  double* mean = nullptr;
  double* var = nullptr;
  int policy = 1;                   // k_predict_finalize's NaN policy for the variance
  int64_t* argmin_v = nullptr;
  double* min_v = nullptr;
  int64_t* argmin_s = nullptr;
  double* min_s = nullptr;
  double* fantasy_out = nullptr;    // C x M fantasy variances, dense
  bool gated = false;               // apply the classifier gate (when one is set) to mean / var (the predict family)
  SweepKeep* keep = nullptr;
  SweepW* w = nullptr;              // the weighted scoring pass in addition (NULL: today's launches, nothing else)
};

// What a member of an evaluation workspace (bobe_gp::EvalWs: the lock-step batch, an evaluation slot, the handle's own)
// holds once its evaluation was collected: the factor of `h` on data generation `gen` at padded size `Np`, and the
// factorisation's info word and smallest pivot root (res[100], res[101]).  The pipeline of an evaluation is factor_into's
// on the same data (same bits in every form), and what follows it - lauum, k_mll_grad_reduce / k_mll_terms - writes only
// Tmp, gpart and res, the noise component's launches (mll_noise_tail) in addition part and the member's LOO block: L (with
// its diagonal blocks back in place), Linv, alpha, w and the scaled coordinates stay intact until the workspace is used again.  bobe_gp_factor adopts such a factor instead of recomputing it (factor_state).
struct EvalTag {
  bool pending = false;     // enqueued, not collected yet
  bool valid = false;       // collected: info / min_diag are known
  Hyper h;
  uint64_t gen = 0;
  int64_t Np = 0;
  int info = 0;
  double min_diag = 0.0;
  void arm(const Hyper& hh, uint64_t g, int64_t np) {
    valid = false;
    pending = true;
    h = hh;
    gen = g;
    Np = np;
  }
  void collected(const double* hr) {     // hr: the evaluation's pinned results ([100] info word, [101] min L_jj)
    if (!pending) return;
    pending = false;
    valid = true;
    std::memcpy(&info, hr + 100, sizeof(int));
    min_diag = hr[101];
  }
  void clear() { pending = valid = false; }
};
// the same factor bit for bit: every field an evaluation's pipeline reads (ls[0..d), kvar, noise, d, kern)
inline bool same_hyper(const Hyper& a, const Hyper& b) {
  if (a.d != b.d || a.kern != b.kern || a.d < 0 || a.d > MAX_D) return false;
  return std::memcmp(a.ls, b.ls, (size_t)a.d * sizeof(double)) == 0 && std::memcmp(&a.kvar, &b.kvar, sizeof(double)) == 0 &&
         std::memcmp(&a.noise, &b.noise, sizeof(double)) == 0;
}

}  // namespace bobe

struct bobe_gp {
  typedef bobe::DBuf DBuf;
  typedef bobe::Hyper Hyper;
  int device = 0;
  int kern = 0;
  int d = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int64_t N = 0, Np = 0;
  int nb = 0;
  Hyper hyp;
  // bumped by everything that changes X, y or N (set_data, append, set_chol, clone, a data-less workspace): an evaluation's
  // factor of an older generation is never adopted
  uint64_t data_gen = 0;
  double pivot_ulp = bobe::default_pivot_floor_ulp();     // the rank test's factor (0: sign test only, as dpotrf)
  double pivot_floor(const Hyper& h) const { return bobe::pivot_floor(h, pivot_ulp); }
  bool have_data = false, factored = false, not_pd = false;
  // Where the installed factor is ill conditioned - (kvar + noise) / smallest pivot above refine_kappa (bobe_gp_set_refine_kappa;
  // default BOBE_REFINE_KAPPA, else 1e6; 0: always, negative: never) - every V = L^-1 K(X, .) is SOLVED for by a blocked
  // forward substitution (sweep_kernels.hpp, k_blk_step) instead of multiplied out with the inverse factor; the vector form
  // of bobe_gp_wip_grad's few-candidate path takes one step of iterative refinement.  Decided when a factor is installed: the
  // same bits on every rank.
  double refine_kappa = bobe::default_refine_kappa();
  bool refine_v = false;
  // solve_block: rows of the substitution's diagonal blocks (a multiple of 128; sets the accuracy).  Speed only: solve_panel
  // = rows per long update launch, solve_chunk = candidates per launch sequence of that path (0: `chunk`)
  int solve_block = bobe::default_solve_block();
  int solve_panel = bobe::default_solve_panel();
  int64_t solve_chunk = bobe::default_solve_chunk();
  void decide_refinement(double min_diag);
  // V = L^-1 B for ncp (a multiple of 128) columns: the product with the inverse factor, or - refine_v - the blocked
  // substitution, which overwrites B [Np x ldb] and needs V (V may be NULL only for the plain product); qp: the column sums
  // of squares per row tile (k_trimul's epilogue)
  void solve_v(double* B, int64_t ldb, int64_t ncp, double* V, int64_t ldv, double* qp, int64_t ldq);
  // the backward half, W = L^-T V for ncp (a multiple of 128) columns: the product with the inverse factor's transpose
  void solve_wt(const double* V, int64_t ldv, int64_t ncp, double* W, int64_t ldw);
  // prepare_z() keeps its results (ZsT, W_Z, base_z) while the same host Z arrives again and nothing they depend on
  // changed: an L-BFGS refinement of one acquisition point calls bobe_gp_wip_grad dozens of times with one Z
  std::vector<double> z_seen;
  int64_t z_seen_m = -1;
  bool wz_ready = false;        // W_Z = K^-1 K(X,Z) (the score GRADIENTS need it; the sweep itself does not)
  void forget_z() { z_seen_m = -1; wz_ready = false; zw_valid = false; }
  // bobe_gp_wip_grad_w and bobe_gp_wip_grad_zvar keep the weighted scorer's per-z table (mu, a, omega, e, l) beside them: valid while prepare_z's cache
  // is valid AND the log-weights (host memory; device ones are never taken as seen) have the same bytes, or are absent
  // again, and y_std is the same.  A hit launches neither wip_zterms' K(X,Z) assembly nor k_wip_zterms.
  bobe::SweepW zw;              // (its buffers are released with the handle)
  bool zw_valid = false, zw_has_logw = false;
  bool zw_lam = false;          // the table holds the lambda row and log E[Z] as well (bobe_gp_wip_grad_zvar asked for them)
  std::vector<double> zw_logw;
  double zw_ystd = 0.0;
  int64_t zw_m = -1;
  int64_t chunk = 8192;
  bool chunk_set = false;       // bobe_gp_set_chunk was called: the caller's chunk holds for the substitution path too

  // the data, the installed factor (XsT, A, Linv, alpha, w) and the scratch of what works on it - bobe_gp_factor, the sweep,
  // append, set_chol, bobe_gp_loo.  The evaluations have workspaces of their own (EvalWs below).
  DBuf X, y, XsT, A, Linv, Tmp, alpha, w, part, gpart, res, info, probs, diag;
  int num_cus = 0;
  // sweep / predict workspace
  // the few-candidate chains (bobe_gp_wip_grad's few path, bobe_gp_wip_grad_w, bobe_gp_wip_grad_zvar): their workspace, their
  // staged outputs and where the one copy of those lands before they go to the caller's arrays (WgOut)
  DBuf wg_ws, wg_out;
  std::vector<double> wg_host;
  DBuf in_stage, z_stage, CsT, ZsT, kXC, kXZ, VZ, WZ, basez, sc, qpart, pv, ps, o_mean, o_var, o_wipv, o_wipstd,
      o_misc, kin_a, kin_b, kout, vxc, vxc2;
  // the inverse's problem table (probs) by depth: whole levels, and their leading / trailing parts (tri_split.hpp)
  std::vector<bobe::Depth> depths, lead_depths, trail_depths;
  int tri_mid = 0;
  double* h_res = nullptr;  // pinned, 128 doubles
  double* h_in = nullptr;   // pinned, 16 x MAX_D doubles: host coordinates of the few-candidate chains (wg_candidates)

  // ---- classifier gate (gp_consumers.hip): support vectors SoA + dual coefficients (SVM) or the transformed L and the
  // centre (ellipsoid) on the device
  DBuf gate_sv, gate_dual, gate_ell;
  bobe::Gate gate{nullptr, nullptr, 0, 0, 0.0, 0.0, 0.5, -1e5};
  void set_gate(const double* sv, int64_t n_sv, const double* dual, double intercept, double gamma, double threshold,
                double minus_inf);
  void set_gate_ellipsoid(const double* flat_L, const double* mu, double alpha, double beta, double threshold,
                          double minus_inf);
  // k_ellipsoid_train: n_restarts AdamW runs in one launch (host arrays; see bobe_gp.h)
  DBuf ell_ws, ell_perm;
  void train_ellipsoid(const double* X, const double* y, int64_t N, const double* mu, int n_restarts, const double* init,
                       const int32_t* perm, int n_epochs, int batch, double lr, double wd, double* params_out,
                       double* loss_out);
  // decision / feasibility of C device-resident query points (row-major C x d); with mean / var / dmean / dvar (device,
  // any may be null) the gated entries are overwritten: mean = -inf, var = 1e-12, gradients 0
  void gate_apply(const double* xq_dev, int64_t C, double* decision, double* feasible, double* mean, double* var,
                  double* dmean, double* dvar, double* proba = nullptr);
  void gate_eval(const double* Xq, int64_t C, double* decision, double* feasible);
  void gate_proba(const double* Xq, int64_t C, double* proba);

  // ---- launch plan of a factorisation (potrf): which panel launch carries which deferred update tiles, and from which
  // panel on every block column still has to be updated by each separate update launch.  Host logic only (a function of
  // the block count, the batch width and the CU count); the tables live on the device.
  struct CholOp {
    int kind;             // 0 panel, 1 narrow update (block column `first`), 2 trailing update (block columns >= first)
    int k;                // panel: block index; updates: one past the last panel to apply (k1)
    int first;
    int tab_off, tab_cnt; // panel: filler jobs [off, off + cnt) of `jobs`; updates: offset of the column table in `colk0`
    int k0_min, k0_max;   // updates: smallest / largest first pending panel over the columns the launch touches
    bool uniform;         // updates: every column from `first` on takes part with the same first panel (no table needed)
    int last_active;      // updates: last block column that takes part
    int k0_plain;         // updates: first pending panel of the columns that are not deferred (they all share it)
  };
  struct CholPlan {
    std::vector<CholOp> ops;
    std::vector<bobe::FillJob> jobs;
    std::vector<int> colk0;
    DBuf d_jobs, d_colk0;
    int far_start = 0;    // first deferred block column (nb: none)
    int64_t deferred_units = 0, catchup_units = 0, total_units = 0;
  };
  std::map<uint64_t, CholPlan> chol_plans;
  bool fill_pays(int B) const;
  const CholPlan& chol_plan(int B, bool fill);
  void build_plans();
  // strips per workgroup of the panel launch with `rr` blocks below the diagonal block (chol_kernels.hpp, panel_workgroups)
  int panel_strips(int B, int rr) const;

  // ---- evaluation workspaces.  One value(+gradient) evaluation of a hyper-parameter vector needs the scaled coordinates,
  // K -> L, Linv, a scratch matrix, w, alpha, the partial sums, the results and the factorisation's info word and diagonal
  // scratch blocks.  An EvalWs holds that for `width` members; member b lives at b * (elements per member) of every buffer.
  // The handle has three kinds: `own` (width 1, the handle's stream: bobe_gp_mll, the LOO objective, the free functions),
  // `slots` (width 1 each, a private stream: bobe_gp_mll_submit / _wait and the batches below BOBE_LOCKSTEP_MIN_N) and
  // `batch` (up to BOBE_MAX_MLL_SLOTS members advancing through ONE launch sequence on the handle's stream, every kernel
  // taking the member from its last grid dimension: bobe_gp_mll_batch, bobe_gp_loo_objective_batch).
  // Replayable pipeline (launch-bound sizes): the kernels of one evaluation captured into a hipGraph per (workspace,
  // with / without gradient).  The hyper-parameters reach the kernels through the workspace's device copy, which the
  // graph's first node refreshes from the pinned one.
  struct EvalGraph {
    hipGraphExec_t exec[2] = {nullptr, nullptr};    // [want_grad]
    std::array<const void*, 16> sig[2] = {};        // every address / size the captured kernels were given
  };
  // How a stage of the factorisation front (assemble_kxx, potrf, trtri, lauum, loo_terms, factor_into / chol_solve) is told
  // where to work and how wide: B members, member b at b * stride of every buffer.  A workspace's buffers with its member
  // strides (EvalWs::bufs), or the installed factor's at width 1 (state_bufs); a width-1 view has stride 0 throughout.
  // mat strides a, linv and tmp; vec w and alpha; xs xst; prt part; gps gpart; rs res (128 per member); lvs loo.
  struct FactorBufs {
    int B;
    double *xst, *a, *linv, *tmp, *w, *alpha, *part, *diag, *gpart, *res, *loo;
    int* info;
    int64_t mat, vec, xs, prt, gps, rs, lvs;
  };
  struct EvalWs {
    explicit EvalWs(int width_) : width(width_), tag(width_), floor(width_, 0.0) {}
    const int width;                 // members it may hold
    int cap = 0;                     // members [0, cap) fit the buffers at Np (ensure)
    int64_t Np = 0;
    int nb = 0, d = 0;
    DBuf XsT, A, Linv, Tmp, w, alpha, part, gpart, res, info, diag, hyp;
    DBuf loo;                        // the LOO objective's seven vectors per member (gp_loo.hip): diag K^-1, mean, var, lpd,
                                     // sqrt c, b / sqrt c, w
    double* h_res = nullptr;         // pinned [width][128]: [0] y^T K^-1 y, [1] sum log L_ii, [2..2+d] gradient, [2+d+1] its
                                     // noise component (the *_noise calls), [100] the factorisation's info word,
                                     // [101] min L_jj, [102] the LOO sum (LOO evaluations)
    Hyper* h_hyp = nullptr;          // pinned [width] (the same allocation)
    EvalGraph eg;
    std::vector<bobe::EvalTag> tag;  // per member: what it holds
    std::vector<double> floor;       // per member: the rank test's floor of the evaluation in flight (read at collect)
    // evaluation slots only: the private stream (the handle's, of slot_stream_set) and the state of submit / wait
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;
    bool busy = false, want_grad = false;
    // elements per member
    int64_t mat() const { return Np * Np; }
    int64_t vec() const { return Np; }
    int64_t xs() const { return (int64_t)d * Np; }
    int64_t prt() const { return (int64_t)nb * Np; }
    int64_t gps() const { return (int64_t)(2 * nb) * (2 * nb + 1) / 2 * (bobe::MAX_D + 1); }
    int64_t lvs() const { return 7 * Np; }
    // the strides the launches are given: a width-1 workspace is the plain call (B = 1, stride 0)
    int64_t stride(int64_t per_member) const { return width > 1 ? per_member : 0; }
    FactorBufs bufs(int B) const {               // the view the stages are given: members [0, B)
      return {B, XsT.d(), A.d(), Linv.d(), Tmp.d(), w.d(), alpha.d(), part.d(), diag.d(), gpart.d(), res.d(), loo.d(),
              static_cast<int*>(info.p), stride(mat()), stride(vec()), stride(xs()), stride(prt()), stride(gps()),
              stride(128), stride(lvs())};
    }
    void ensure(const bobe_gp& g, int B);      // room for B members at the handle's Np / nb / d
    void release();
  };
  EvalWs own{1}, batch{BOBE_MAX_MLL_SLOTS};
  std::vector<EvalWs*> slots;                // (reserved once: bobe_gp_mll_wait reads it without the submit mutex)
  // The workspace an evaluation runs on.  It holds buffers and records only - no stage leaves hand-over state on it (the
  // stages get a FactorBufs view and pass what they hand over by value) - so `cur` is just what on_slot() reads, and on a
  // slot the handle's `stream` is the slot's.  UseWs makes one current for a scope; nothing else of the handle changes.
  EvalWs* cur = &own;
  bool on_slot() const { return cur->stream != nullptr; }
  struct UseWs {
    bobe_gp& g;
    EvalWs* const prev;
    const hipStream_t prev_stream;
    UseWs(bobe_gp& g_, EvalWs& ws) : g(g_), prev(g_.cur), prev_stream(g_.stream) {
      g.cur = &ws;
      if (ws.stream) g.stream = ws.stream;
    }
    ~UseWs() {
      g.cur = prev;
      g.stream = prev_stream;
    }
    UseWs(const UseWs&) = delete;
    UseWs& operator=(const UseWs&) = delete;
  };
  FactorBufs state_bufs() const {            // the installed factor (loo: loo_ws, once loo_state has sized it)
    return {1, XsT.d(), A.d(), Linv.d(), Tmp.d(), w.d(), alpha.d(), part.d(), diag.d(), gpart.d(), res.d(), loo_ws.d(),
            static_cast<int*>(info.p), 0, 0, 0, 0, 0, 0, 0};
  }
  std::vector<hipStream_t> slot_streams;     // one per evaluation slot, created on first use
  const std::vector<hipStream_t>& slot_stream_set();
  hipEvent_t ev_batch = nullptr;
  std::mutex submit_mutex;          // serialises bobe_gp_mll_submit (it makes a slot current on the handle)
  void ensure_slots(int n);
  void ensure_batch(int B);
  // the launches of B evaluations on ws (hdev: the device copy of the hyper-parameters, refreshed first; NULL: the kernels
  // take hs[0] by value); eval_start picks the form (plain, graph replay, lock step) and keeps the members' records
  // noise_grad (bobe_gp_mll_noise, with a gradient only): mll_noise_tail's launches are appended, the gradient has d + 2
  // entries per member (the last from res[2 + d + 1]); never replayed as a graph
  void eval_enqueue(EvalWs& ws, int B, const Hyper* hs, bool want_grad, const Hyper* hdev, bool noise_grad = false);
  void eval_replay(EvalWs& ws, const Hyper* hs, bool want_grad);
  void eval_start(EvalWs& ws, int B, const Hyper* hs, bool want_grad, bool noise_grad = false);
  int eval_collect(EvalWs& ws, int B, double* mll, double* grad, int* status, bool noise_grad = false);
  // hr: an evaluation's pinned results; NaN outputs, g_err and BOBE_NOT_PD when the factorisation failed or a pivot is below floor
  int eval_result(const double* hr, double floor, double* mll, double* grad, bool noise_grad = false) const;
  int mll_batch(int64_t B, const double* ls, const double* kvar, double* mll, double* grad, int* status);
  // bobe_gp_mll_noise_batch: lock step on `batch`, a lone member and N < BOBE_LOCKSTEP_MIN_N singly on `own` (no slot form)
  int mll_noise_batch(int64_t B, const double* ls, const double* kvar, const double* noise, double* mll, double* grad,
                      int* status);
  void mll_submit(int slot, const double* ls, double kvar, int want_grad);
  int mll_wait(int slot, double* mll, double* grad);

  // optional per-kernel-class timing with HIP events on the handle's stream (bobe_gp_profile_*)
  int prof_tag = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  size_t prof_used = 0;
  void prof_begin(int tag) {
    if (tag != prof_tag) return;
    if (prof_used == prof_events.size()) {
      hipEvent_t a, b;
      HIPCHK(hipEventCreate(&a));
      HIPCHK(hipEventCreate(&b));
      prof_events.emplace_back(a, b);
    }
    HIPCHK(hipEventRecord(prof_events[prof_used].first, stream));
  }
  void prof_end(int tag) {
    if (tag != prof_tag) return;
    HIPCHK(hipEventRecord(prof_events[prof_used].second, stream));
    ++prof_used;
  }

  void use() {
    HIPCHK(hipSetDevice(device));
    bobe::configure_factor_kernels();
    bobe::configure_sweep_kernels();
    bobe::configure_consumer_kernels();
    bobe::configure_posterior_kernels();
    bobe::configure_loo_kernels();
    bobe::configure_paths_kernels();
  }
  void sync() { HIPCHK(hipStreamSynchronize(stream)); }

  // host or device input -> device pointer (staged through `stage` when it is host memory)
  const double* fetch(const double* p, size_t n, DBuf& stage) {
    if (bobe::is_device_ptr(p)) return p;
    stage.ensure(n * sizeof(double));
    HIPCHK(hipMemcpyAsync(stage.p, p, n * sizeof(double), hipMemcpyHostToDevice, stream));
    return stage.d();
  }
  // output: device pointer to write to (user's when it is device memory, else `stage`)
  double* out_dev(double* user, size_t n, DBuf& stage) {
    if (!user) return nullptr;
    if (bobe::is_device_ptr(user)) return user;
    stage.ensure(n * sizeof(double));
    return stage.d();
  }
  void out_finish(double* user, size_t n, DBuf& stage) {
    if (!user || bobe::is_device_ptr(user)) return;
    HIPCHK(hipMemcpyAsync(user, stage.p, n * sizeof(double), hipMemcpyDeviceToHost, stream));
  }

  // ---- what the few-candidate chains share on the host (wip_grad's few path in gp_sweep.hip, wip_grad_chain in gp_criteria.hip)
  static constexpr int64_t WG_MAX_N = 4096;       // the chains' limit on N: the cross kernels keep v in N doubles of LDS
  // The candidates of a call.  One group (C <= 16) of host coordinates goes through the pinned block h_in: the first stage
  // reads them there (first) and leaves the device copy (dev) that the later stages read (later) - no copy command in front of
  // the chain.  Anything else is fetch()'s: dev is null and first == later.
  struct WgCand {
    const double* first;
    double* dev;
    const double* later;
  };
  WgCand wg_candidates(const double* cand, int64_t C, bool one_group) {
    if (!one_group || bobe::is_device_ptr(cand)) {
      const double* cin = fetch(cand, (size_t)C * d, in_stage);
      return {cin, nullptr, cin};
    }
    const size_t cap = (size_t)16 * bobe::MAX_D * sizeof(double);
    if (!h_in) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h_in), cap, hipHostMallocDefault));
    std::memcpy(h_in, cand, (size_t)C * d * sizeof(double));
    in_stage.ensure(cap);
    return {h_in, in_stage.d(), in_stage.d()};
  }
  // wg_front's six vectors (k_c, v, u and the refinement step's three temporaries), n_vec doubles each, carved from p
  struct WgFront {
    double *kc, *vv, *uu, *t1, *t2, *t3, *end;      // end: what follows them
    WgFront(double* p, size_t n_vec)
        : kc(p), vv(kc + n_vec), uu(vv + n_vec), t1(uu + n_vec), t2(t1 + n_vec), t3(t2 + n_vec), end(t3 + n_vec) {}
  };
  // The outputs of a call.  A device pointer is written directly and NULL stays NULL (the last stage skips it); the requested
  // HOST arrays share one block, back to back in the order they were added: the pinned result block h_res (128 doubles), which
  // the last stage writes itself - no copy command -, when there is no device output, one group and they fit, else a staged
  // block that ONE copy brings home.  add every output (dev receives its device pointer at place()), place, launch, finish
  // (the copy command), sync, scatter (into the caller's arrays).
  struct WgOut {
    bobe_gp& g;
    struct Item {
      double* user;
      double** dev;
      size_t off, n;
    } items[8];
    int n_items = 0;
    size_t n_host = 0;
    bool any_dev = false, packed = false;
    const double* home = nullptr;
    explicit WgOut(bobe_gp& g_) : g(g_) {}
    void add(double* user, size_t n, double*& dev) {
      dev = user;
      if (!user) return;
      if (bobe::is_device_ptr(user)) {
        any_dev = true;
        return;
      }
      items[n_items++] = {user, &dev, n_host, n};
      n_host += n;
    }
    void place(bool one_group) {
      packed = one_group && n_host <= 128 && !any_dev;
      double* base = g.h_res;
      if (!packed && n_host) {
        g.wg_out.ensure(n_host * sizeof(double));
        base = g.wg_out.d();
      }
      for (int i = 0; i < n_items; ++i) *items[i].dev = base + items[i].off;
      home = g.h_res;
    }
    void finish() {
      if (packed || !n_host) return;
      g.wg_host.resize(n_host);
      HIPCHK(hipMemcpyAsync(g.wg_host.data(), g.wg_out.p, n_host * sizeof(double), hipMemcpyDeviceToHost, g.stream));
      home = g.wg_host.data();
    }
    void scatter() const {
      for (int i = 0; i < n_items; ++i) std::memcpy(items[i].user, home + items[i].off, items[i].n * sizeof(double));
    }
  };

  // ---- gp_factor.hip
  void build_probs();
  void alloc_for_n();
  void set_data(const double* X, const double* ys, int64_t N);
  // Batched forms (B > 1): slot b of a batch works on base + b * stride of every matrix / vector it is given and
  // reads its hyper-parameters from hdev[b]; B = 1 with zero strides is the plain call.
  void scale(const double* in, int64_t n, int64_t npad, const Hyper& h, double* out, int64_t ldo,
             const Hyper* hdev = nullptr, int B = 1, int64_t bsO = 0, int* info_reset = nullptr);
  // wv / prt: also prt[row tile][column] = the tile's share of out^T wv (k_gemv_t_part's partial sums, same bits)
  void kernel_matrix_cross(const double* AT, int64_t lda, int64_t na, int64_t napad, const double* BT, int64_t ldb,
                           int64_t nbv, int64_t nbpad, const Hyper& h, double* out, int64_t ldo,
                           const double* wv = nullptr, double* prt = nullptr, int64_t ldp = 0);
  void assemble_kxx(const Hyper& h, const FactorBufs& f, const Hyper* hdev = nullptr);
  void syrk(const FactorBufs& f, int k0, int k1, int first, int colmode, const int* colk0 = nullptr, int far_col = 0,
            int ncols = 0);
  // What a factorisation hands to the inverse that follows it: the L_kk of steps >= first are still in the scratch blocks
  // dg (first = nb: none).  It travels by value - potrf returns it, the inverse takes it - and nothing of it stays behind.
  struct Aside {
    int first;
    const double* dg;
  };
  Aside no_aside() const { return {nb, nullptr}; }           // an inverse of a factor that no potrf of ours left behind
  // The factorisation of f.a (L in place, the 16 x 16 diagonal inverses into f.linv): potrf_ops runs the ops
  // [op_begin, op_end) of the launch plan and lowers `aside` to the first step it left in the scratch blocks; potrf is the
  // whole plan.  defer_diag: return what is aside for the trtri() that follows to put in place (one launch less); else
  // k_copy_diag puts the blocks back here and nothing is aside.
  void potrf_ops(const FactorBufs& f, const CholPlan& pl, size_t op_begin, size_t op_end, Aside& aside);
  Aside potrf(const FactorBufs& f, bool defer_diag = false);
  // The parts of the inverse (tri_split.hpp): TRI_ALL is the whole of it, TRI_LEAD + TRI_TRAIL + TRI_TOP_R in this order
  // (LEAD and TRAIL in either order, or side by side) the same launches on the same data.  trtri_part / trtri_level launch
  // on the stream they are given; trtri is TRI_ALL on the handle's.
  enum TriPart { TRI_ALL, TRI_LEAD, TRI_TRAIL, TRI_TOP_R };
  void trtri_part(TriPart part, const FactorBufs& f, Aside aside, hipStream_t st);
  void trtri_level(const FactorBufs& f, const bobe::Depth& part, int level_blocks, bool do_t, bool do_r, hipStream_t st);
  void trtri(const FactorBufs& f, Aside aside) { trtri_part(TRI_ALL, f, aside, stream); }
  // ---- the side stream of the inverse's leading half (chol_solve).  With mid = nb / 2, once panel mid - 1 has run the
  // factorisation only writes A[mid:, mid:], the scratch blocks and 16 x 16 inverses of steps >= mid and the info word:
  // TRI_LEAD reads L[:, 0:mid) and writes Linv[0:mid, 0:mid) and Tmp[:, 0:mid), so it can run beside panels mid .. nb-1,
  // which leave most CUs empty.  chol_solve cuts the plan's op list after that panel: one fork (ev_fork, recorded between
  // the two ranges) and one join (ev_join, waited for before TRI_TOP_R) per factorisation; ordering by events only, and the
  // handle's `stream` is never swapped for it.  Only on the handle's own stream: never on an evaluation slot, never under
  // graph capture (`capturing`), never while the inverse's launches are being timed as a class.
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool capturing = false;
  bool inv_side_pays(int B) const;
  void ensure_side();
  // K^-1 tiles with the gradient's partial sums into f.gpart; returns their count.  store_kinv: K^-1's lower tiles go to
  // f.tmp (the LOO objective, kinv_debug); else f.tmp is the scratch of the 32-tile form (the MLL gradient)
  int lauum(const Hyper& h, const FactorBufs& f, const Hyper* hdev, bool store_kinv);
  // wv = Linv rhs, al = Linv^T wv (rhs: y unless given; bsY: its stride per batch member).  Pointer form: bobe_gp_wip_grad
  // solves for many right-hand sides against ONE factor, a pattern no FactorBufs describes
  void solve_alpha(const double* linv, double* wv, double* al, double* prt, int B = 1, int64_t bsL = 0, int64_t bsV = 0,
                   int64_t bsP = 0, const double* rhs = nullptr, int64_t bsY = 0);
  // scale, K(X, X), chol_solve on f's buffers; chol_solve: potrf, trtri, w / alpha of the right-hand side (y unless given)
  void factor_into(const Hyper& h, const FactorBufs& f, const Hyper* hdev = nullptr);
  void chol_solve(const FactorBufs& f, const double* rhs = nullptr);
  // k_mll_terms of one factor (w may be NULL: the pivots only) into res; res_to_host: its first n doubles, synchronised
  void mll_terms(const double* wv, const double* a, double* res_dev, const int* info_dev);
  void res_to_host(const double* res_dev, double* h, int n);
  std::string not_pd_text(int inf, double min_diag) const;
  // gp_mll(k, train_y, num_points) / fast_update_cholesky(L, k, k_self) on caller-supplied matrices (gp.py:170-197)
  void size_workspace(int64_t n);
  int mll_from_k(const double* K, int64_t n, const double* yv, double* mll);
  void chol_row_update(const double* L, int64_t n, const double* k, double k_self, double* v, double* diag_out);
  int factor_state();                                  // bobe_gp_factor
  // Adoption of an evaluation's factor by factor_state: forget_evals() drops every workspace's record (the data changed, a
  // workspace was reallocated or used for something else); adopt_factor() copies a matching one into A / Linv / alpha / w /
  // XsT and returns its tag (nullptr: none matches).  factor_source: where the installed factor came from
  // (bobe_debug_factor_source: -1 none yet, 0 factorised, 1 lock-step batch slot, 2 evaluation slot, 3 single evaluation)
  void forget_evals();
  const bobe::EvalTag* adopt_factor();
  int factor_source = -1;
  void copy_out_matrix(const double* src, double* dst, int lower_only);
  void get_chol(double* L, double* alpha_out);
  void set_chol(const double* L, const double* alpha_in);
  double min_pivot_root();
  void kinv_debug(double* Kinv);
  double time_potrf(int reps);
  double time_potrf_batch(int B, int reps);
  double time_potrf_lockstep(int B, int reps);
  double time_potrf_wide(EvalWs& ws, int B, int reps);
  void fill(double* p, int64_t n, double v);

  // ---- gp_sweep.hip
  void prepare_z(const double* Z, int64_t M, int64_t Mp, bool need_w);
  void wip_score(const double* crossT, int64_t ldx, const double* cst, const double* scs, const double* bz, int64_t ns,
                 int64_t M, int64_t Mp, double y_std, double* wv, double* ws, double* vo);
  void sweep(const bobe::SweepReq& r);
  void wip_grad(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, double* wipv, double* wipstd,
                double* dwipv, double* dwipstd);
  // the front of the few-candidate chains for the C candidates from c0 on: k_wg_col, solve_alpha and - refine_v - the vector
  // refinement step
  void wg_front(const WgCand& cc, int64_t c0, int64_t C, const WgFront& f);
  void predict_grad(const double* Xq, int64_t C, double* mean, double* var, double* dmean, double* dvar);
  // predict_grad's full-mode launches, the gate included, on device pointers (cin: C x d; d_mean may be null): nothing is
  // copied home and nothing waits for the stream - what predict_grad and acq_ei_grad share
  void predict_grad_chain(const double* cin, int64_t C, double* d_mean, double* d_var, double* d_dm, double* d_dv);
  int append(const double* X_new, int64_t b, const double* y_all);

  // ---- gp_posterior.hip (call-local buffers only; the factorisation of Sigma runs on a data-less child handle)
  int predict_cov(const double* Xq, int64_t C, double* cov);
  int posterior_sample(const double* Xq, int64_t C, int64_t S, uint64_t seed, const double* z, int centered, double* draws,
                       double* jitter_out);

  // ---- gp_loo.hip (loo_ws: seven vectors of Np - diag K^-1, mean, var, lpd, sqrt c, b / sqrt c, w - of the state form;
  // an evaluation works on its workspace's own)
  DBuf loo_ws;
  // The LOO terms of f's factors, from their inverse factors and alphas through f.part into the seven-vector blocks f.loo; the
  // sums land in f.res[102].  loo_kinv_diag is their front: diag K^-1 into the first vector of f.loo
  void loo_kinv_diag(const FactorBufs& f);
  void loo_terms(const FactorBufs& f, bool with_grad_terms);
  int loo_state(double* mean, double* var, double* lpd, double* sum_lpd);
  // the launches of B LOO evaluations on ws (eval_enqueue's counterpart), and their start-to-collect on ws
  void loo_enqueue(EvalWs& ws, int B, const Hyper* hs, bool want_grad, const Hyper* hdev, bool noise_grad = false);
  int loo_eval(EvalWs& ws, int B, const Hyper* hs, double* loo, double* grad, int* status, bool noise_grad = false);
  int loo_objective(const Hyper& h, double* loo, double* grad, bool noise_grad = false);
  int loo_batch(int64_t B, const double* ls, const double* kvar, double* loo, double* grad, int* status,
                const double* noise = nullptr);
  // the noise component of the gradient, d / d log nu: the launches appended to an MLL / a LOO evaluation with a gradient
  void mll_noise_tail(const FactorBufs& f, const Hyper* hs, const Hyper* hdev);
  void loo_noise_tail(const FactorBufs& f, const Hyper* hs, const Hyper* hdev);

  // ---- gp_batch.hip (call-local buffers only; the handle's Z-side state is read, never written)
  int wip_select_batch(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, int n_batch, int criterion,
                       int64_t* picks, double* pick_scores, double* stage_scores);
  // the batch selection itself; w: score with the weighted scorer (criterion 0 .. 3) instead of wip_score (0 / 1)
  int select_batch(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, int n_batch, int criterion,
                   int64_t* picks, double* pick_scores, double* stage_scores, bobe::SweepW* w,
                   const bobe::BatchDebug* dbg = nullptr);
  // select_batch with n_stage downdates, forced picks and the downdated state copied out (bobe_debug_batch_terms)
  int debug_batch_terms(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                        int criterion, int n_stage, const int64_t* forced, double* crossT, double* sc_out, double* basez_out,
                        double* UC, double* UZ, int64_t* picks, double* stage_scores);
  // what the sweep forms on the way to its scores (bobe_debug_sweep_terms): the sweep with a SweepKeep, copied out unpadded
  int debug_sweep_terms(const double* cand, int64_t C, const double* Z, int64_t M, double* V, double* VZ_out, double* crossT,
                        double* sc_out, double* basez_out);

  // ---- gp_criteria.hip: the importance-weighted scoring pass (criteria_kernels.hpp)
  // the per-z table of w for the base_z in bz (first: mu, a, omega as well; else only the terms that follow base_z)
  // lam: the lambda row and log E[Z] too, as for a w with zz set
  void wip_zterms(bobe::SweepW& w, int64_t M, int64_t Mp, double y_std, const double* bz, bool first, bool lam = false);
  // k_wip_score_w on ns candidates (wip_score's arguments); writes w.out[k] + off
  void wip_score_w(const bobe::SweepW& w, const double* crossT, int64_t ldx, const double* cst, const double* scs,
                   const double* bz, int64_t ns, int64_t M, int64_t Mp, double y_std, int64_t off);
  // k_wip_score_zz on ns candidates (the same arguments); writes w.zz + off
  void wip_score_zz(const bobe::SweepW& w, const double* crossT, int64_t ldx, const double* cst, const double* scs,
                    const double* bz, int64_t ns, int64_t M, int64_t Mp, double y_std, int64_t off);
  int wip_sweep_w(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                  double* const outs[4], double* log_s, int64_t* argmin, double* mins);
  int wip_sweep_zvar(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                     double* zvar, double* log_ez, int64_t* argmin, double* min);
  int wip_select_batch_zvar(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                            int n_batch, int64_t* picks, double* pick_scores, double* stage_scores);
  int wip_select_batch_w(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                         int n_batch, int criterion, int64_t* picks, double* pick_scores, double* stage_scores);
  // values and input gradients of the four scores through the few-candidate chain, in groups of 16 (WG_MAX_N: its limit on N)
  int wip_grad_w(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                 double* const scores[4], double* const grads[4]);
  // value and input gradient of the evidence-variance score through the same chain, the same limit on N
  int wip_grad_zvar(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw, double* zvar,
                    double* dzvar, double* log_ez);
  // what the two share: the kept per-z table, and the chain itself (entry: the name in front of its refusals)
  void wip_grad_table(int64_t M, int64_t Mp, double y_std, const double* logw, bool lam);
  int wip_grad_chain(const char* entry, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                     const double* logw, double* const scores[4], double* const grads[4], int mask, bool zv, double* log_ez);

  // ---- gp_criteria.hip: log E[Z] and log T0 = log (Var Z / E[Z]^2) of the evidence estimate over Z (evidence_kernels.hpp);
  // prepare_z, the per-z table with its lambda row, then k_evid_h -> k_evid_pairs -> k_evid_fold and one copy home
  int evidence_moments(const double* Z, int64_t M, double y_std, const double* logw, double* log_ez, double* log_t0);

  // ---- gp_consumers.hip
  void acq_ei(const double* Xq, int64_t C, double best_y, double zeta, int mode, double* out);
  // +EI / +logEI and their input gradients: predict_grad_chain into the o_* staging buffers, then k_ei_grad; one sync
  void acq_ei_grad(const double* Xq, int64_t C, double best_y, double zeta, int mode, double* val, double* grad);
  void hmc_leapfrog(int64_t P, double* U, double* Pm, const double* inv_mass, double eps, int L, double y_std,
                    double y_mean, double temp, double* logp, double* grad, double* mean, double* X);
  void hmc_run(int64_t P, double* state, double* adapt, const double* inv_mass, uint64_t seed, int64_t it0, int niter,
               int do_adapt, double y_std, double y_mean, double temp, int hist_from, double* hist, int thin, double* keep,
               double* dbg);
  void nuts_run(int64_t P, double* state, double* adapt, const double* inv_metric, int max_depth, uint64_t seed,
                int64_t it0, int niter, int do_adapt, double y_std, double y_mean, double temp, int hist_from, double* hist,
                int thin, double* keep, double* stats, double* dbg);
  void rwalk(int64_t P, double* Xw, double* logl, const double* step, double lstar, int walks, uint64_t seed, double y_std,
             double y_mean, int* nacc, int* nin, double* dbg);
  // sqdist: the squared distances of the rows as they are (dist_sq, gp.py:80-96) instead of kernel values
  void kernel_eval(const double* A, int64_t nA, const double* B, int64_t nB, const double* ls, double kvar, double noise,
                   int include_noise, double* out, bool sqdist = false);
  void clone_from(bobe_gp& src);
  void release_all();
};

// ---- gp_paths.hip: the path set behind bobe_gp_paths_* (a snapshot of its parent's state; it uses the parent's stream, chunk
// and launch helpers, so it is destroyed first).  The functions throw Err like the members above.
namespace bobe {
int paths_create(bobe_gp& g, int64_t S, int64_t F, uint64_t seed, const double* u, const double* phase, const double* w,
                 const double* eps, bobe_paths** out);
int paths_get(bobe_paths& p, double* u, double* phase, double* w, double* eps);
int paths_eval(bobe_paths& p, const double* Xq, int64_t C, int centered, double* f);
int paths_argmax(bobe_paths& p, const double* Xq, int64_t C, const double* bias, int64_t* idx, double* best);
int paths_grad(bobe_paths& p, const double* Xq, int64_t T, const int64_t* path_idx, int centered, double* f, double* df);
int paths_hmc_run(bobe_paths& p, int64_t P, const int64_t* path_idx, double* state, double* adapt, const double* inv_mass,
                  uint64_t seed, int64_t it0, int niter, int do_adapt, double y_std, double y_mean, double temp,
                  int hist_from, double* hist, int thin, double* keep, double* dbg);
int paths_chain_layout(bobe_paths& p, int* info4);
void paths_destroy(bobe_paths* p);
}  // namespace bobe
