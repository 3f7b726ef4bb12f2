// libbobe_gp.so, criteria unit: importance-weighted integration points and the IMIQR / EIV criteria (bobe_gp_wip_sweep_w,
// bobe_gp_wip_select_batch_w).  Kernels: criteria_kernels.hpp (the per-z table, the weighted scorer), batch_kernels.hpp
// (k_argmin_masked).  The launch sequence is bobe_gp::sweep's (gp_sweep.hip) and the batch selection's (gp_batch.hip): this
// unit adds one scoring pass per super-chunk and one small kernel per call (per stage for criterion 3).
// The per-z table, the partial sums, the staged weights and outputs belong to the call (SweepW's CallBufs) and are freed
// before it returns.  One buffer of the handle is written: kXZ, the sweep workspace's K(X, Z), which prepare_z fills and
// nothing reads once prepare_z is through (the substitution path overwrites it there) - scratch, rewritten here with its
// own bits; the handle's Z-side STATE (ZsT, V_Z, base_z and prepare_z's cache of them) is read, never written.
// bobe_gp_wip_grad_w (values and input gradients of the four scores through bobe_gp_wip_grad's few-candidate chain) and
// bobe_gp_wip_grad_zvar (the same for the evidence-variance score) are the entries here that go through prepare_z themselves
// and keep something between calls: the per-z table beside prepare_z's cache (bobe_gp::zw), their workspace and staged outputs.
// bobe_gp_evidence_moments (the total variance of the evidence estimate; kernels: evidence_kernels.hpp) goes through
// prepare_z too and keeps nothing of its own: its table, rows, tile sums and staged weights are freed before it returns.
#include "gp_handle.hpp"

#include "batch_kernels.hpp"
#include "criteria_kernels.hpp"
#include "evidence_kernels.hpp"

using namespace bobe;

void bobe_gp::wip_zterms(SweepW& w, int64_t M, int64_t Mp, double y_std, const double* bz, bool first, bool lam) {
  const double* lw = nullptr;
  if (first) {
    w.ldt = Mp;
    w.zt.ensure((size_t)(ZTERM_ROWS * Mp + 8) * sizeof(double));
    w.zpart.ensure((size_t)nb * Mp * sizeof(double));
    if (w.logw) lw = fetch(w.logw, (size_t)M, w.lstage);
    // K(X,Z) assembled once more with alpha riding along: the row-block partial sums of K(X,Z)^T alpha (k_gemv_t_part's bits).
    // Whether prepare_z assembled it in this call or hit its cache, kXZ cannot be trusted to hold K(X,Z) - the blocked
    // substitution solves in place - so it is not read but rewritten (an Np x Mp assembly, 1 / (C / M) of the sweep's own
    // K(X, C); kXZ is scratch after prepare_z, see the file header), and mu_z has the same bits on every path.
    kernel_matrix_cross(XsT.d(), Np, N, Np, ZsT.d(), Mp, M, Mp, hyp, kXZ.d(), Mp, (const double*)alpha.d(), w.zpart.d(), Mp);
  }
  hipLaunchKernelGGL(k_wip_zterms, dim3(1), dim3(256), 0, stream, (const double*)w.zpart.d(), Mp, nb, M, y_std, lw, bz,
                     w.zt.d(), Mp, first ? 1 : 0, w.log_s(), (w.zz || lam) ? 1 : 0, w.log_ez());
  LAUNCH_CHECK();
}

void bobe_gp::wip_score_w(const SweepW& w, const double* crossT, int64_t ldx, const double* cst, const double* scs,
                          const double* bz, int64_t ns, int64_t M, int64_t Mp, double y_std, int64_t off) {
  const dim3 grid((unsigned)((ns + 63) / 64));
  const size_t sm = (size_t)(d + 4) * 128 * sizeof(double);
  auto at = [&](int k) { return w.out[k] ? w.out[k] + off : nullptr; };
  with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) {
    hipLaunchKernelGGL((k_wip_score_w<KE, DC>), grid, dim3(256), sm, stream, crossT, ldx, cst, ldx, (const double*)ZsT.d(), Mp,
                       M, scs, bz, (const double*)w.zt.d(), w.ldt, ns, hyp, y_std * y_std, at(0), at(1), at(2), at(3));
  });
}

void bobe_gp::wip_score_zz(const SweepW& w, const double* crossT, int64_t ldx, const double* cst, const double* scs,
                           const double* bz, int64_t ns, int64_t M, int64_t Mp, double y_std, int64_t off) {
  const dim3 grid((unsigned)((ns + ZZ_G - 1) / ZZ_G));
  with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) {
    hipLaunchKernelGGL((k_wip_score_zz<KE, DC>), grid, dim3(256), 0, stream, crossT, ldx, cst, ldx, (const double*)ZsT.d(), Mp,
                       M, scs, bz, (const double*)w.zt.d(), w.ldt, ns, hyp, y_std, w.zz + off);
  });
}

int bobe_gp::wip_sweep_w(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                         double* const outs[4], double* log_s, int64_t* argmin, double* mins) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (C <= 0 || M <= 0) throw Err(BOBE_ERR_ARG, "C and M must be positive");
  use();
  const bool want_min = argmin || mins;
  SweepW w;
  w.logw = logw;
  SweepReq rq;
  rq.cand = cand; rq.C = C; rq.Z = Z; rq.M = M; rq.y_std = y_std;
  int64_t am[4] = {-1, -1, -1, -1};
  double mv[4];
  for (double& x : mv) x = std::numeric_limits<double>::quiet_NaN();
  // equal weights (logw NULL): WIPV / WIPStd are the existing scorer's, bit for bit
  const bool old_v = !logw && outs[0], old_s = !logw && outs[1];
  if (old_v) { rq.wipv = outs[0]; if (want_min) { rq.argmin_v = &am[0]; rq.min_v = &mv[0]; } }
  if (old_s) { rq.wipstd = outs[1]; if (want_min) { rq.argmin_s = &am[1]; rq.min_s = &mv[1]; } }
  CallBuf stage[4], dmin;
  bool any_w = log_s != nullptr;
  for (int k = 0; k < 4; ++k) {
    if (!outs[k] || (k == 0 && old_v) || (k == 1 && old_s)) continue;
    any_w = true;
    if (is_device_ptr(outs[k])) w.out[k] = outs[k];
    else { stage[k].ensure((size_t)C * sizeof(double)); w.out[k] = stage[k].d(); }
  }
  if (any_w) rq.w = &w;
  sweep(rq);
  if (any_w) {
    dmin.ensure(8 * sizeof(double));
    double* dv = dmin.d();
    int64_t* di = reinterpret_cast<int64_t*>(dmin.d() + 4);
    for (int k = 0; k < 4; ++k) {
      if (!w.out[k]) continue;
      if (want_min)
        hipLaunchKernelGGL(k_argmin_masked, dim3(1), dim3(1024), 0, stream, (const double*)w.out[k], C, di + k, 0, dv + k);
      if (w.out[k] != outs[k])
        HIPCHK(hipMemcpyAsync(outs[k], w.out[k], (size_t)C * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    LAUNCH_CHECK();
    double hb[8];
    if (want_min) HIPCHK(hipMemcpyAsync(hb, dmin.p, 8 * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (log_s) HIPCHK(hipMemcpyAsync(log_s, w.log_s(), sizeof(double), hipMemcpyDefault, stream));
    sync();
    if (want_min)
      for (int k = 0; k < 4; ++k)
        if (w.out[k]) {
          mv[k] = hb[k];
          std::memcpy(&am[k], hb + 4 + k, sizeof(int64_t));
        }
  }
  for (int k = 0; k < 4; ++k) {
    if (argmin) argmin[k] = am[k];
    if (mins) mins[k] = mv[k];
  }
  return BOBE_OK;
}

// Values and input gradients of the four scores (criteria_kernels.hpp, "input gradients of the four scores").  Per group of up
// to 16 candidates: wg_front (bobe_gp_wip_grad's first stages) -> k_wg_cross_w -> k_wg_weights_w -> k_wg_rows -> k_wg_final_w.
int bobe_gp::wip_grad_w(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                        double* const scores[4], double* const grads[4]) {
  int mask = 0;
  for (int k = 0; k < 4; ++k)
    if (scores[k] || grads[k]) mask |= 1 << k;
  return wip_grad_chain("bobe_gp_wip_grad_w", cand, C, Z, M, y_std, logw, scores, grads, mask, false, nullptr);
}

// Value and input gradient of the evidence-variance score (criteria_kernels.hpp, "input gradient of the evidence-variance
// score"): the same chain with k_wg_zv_r -> k_wg_zv_pair -> k_wg_zv_fold in k_wg_weights_w's place, criterion slot 0.
int bobe_gp::wip_grad_zvar(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                           double* zvar, double* dzvar, double* log_ez) {
  double* const scores[4] = {zvar, nullptr, nullptr, nullptr};
  double* const grads[4] = {dzvar, nullptr, nullptr, nullptr};
  return wip_grad_chain("bobe_gp_wip_grad_zvar", cand, C, Z, M, y_std, logw, scores, grads, (zvar || dzvar) ? 1 : 0, true,
                        log_ez);
}

// The per-z table of the few-candidate chains: the handle's copy (bobe_gp::zw) while Z, the log-weights and y_std are the ones
// it was made for.  lam: the lambda row and log E[Z] as well (bobe_gp_wip_grad_zvar) - added to a kept table that lacks them
// by the table's second half alone (k_wip_zterms with first = 0: the e row and log S are rewritten with their own bits).
void bobe_gp::wip_grad_table(int64_t M, int64_t Mp, double y_std, const double* logw, bool lam) {
  const bool host_lw = logw && !is_device_ptr(logw);
  const bool hit = zw_valid && zw_m == M && zw_ystd == y_std && zw_has_logw == (logw != nullptr) && (!logw || host_lw) &&
                   (!logw || std::memcmp(zw_logw.data(), logw, (size_t)M * sizeof(double)) == 0);
  if (hit) {
    if (lam && !zw_lam) {
      wip_zterms(zw, M, Mp, y_std, basez.d(), false, true);
      zw_lam = true;
    }
    return;
  }
  zw_valid = false;
  zw.logw = logw;
  wip_zterms(zw, M, Mp, y_std, basez.d(), true, lam);
  zw.logw = nullptr;
  zw_lam = lam;
  // (a device Z leaves prepare_z without a cache - z_seen_m < 0 - and device log-weights cannot be compared: no table kept)
  if (z_seen_m == M && (!logw || host_lw)) {
    zw_valid = true;
    zw_m = M;
    zw_ystd = y_std;
    zw_has_logw = logw != nullptr;
    if (logw) zw_logw.assign(logw, logw + M);
  }
}

// mask: the criteria of k_wg_weights_w asked for; zv: the evidence-variance stages instead (mask 1: their slot).
int bobe_gp::wip_grad_chain(const char* entry, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                            const double* logw, double* const scores[4], double* const grads[4], int mask, bool zv,
                            double* log_ez) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (C <= 0 || M <= 0) throw Err(BOBE_ERR_ARG, "C and M must be positive");
  int nv = 0;
  for (int k = 0; k < 4; ++k) nv += (mask >> k) & 1;
  if (!mask)
    throw Err(BOBE_ERR_ARG, std::string(entry) + (zv ? ": no output requested (zvar and dzvar are NULL)"
                                                     : ": no criterion requested (every scores[k] and grads[k] is NULL)"));
  if (N > WG_MAX_N)
    throw Err(BOBE_ERR_ARG, std::string(entry) + ": " + std::to_string(N) + " training points exceed the matrix-vector chain's " +
                                "limit of " + std::to_string(WG_MAX_N) + " (there is no tile path)");
  use();
  const int64_t Mp = round_up(M, TILE), G = std::min<int64_t>(C, 16);
  const double kself = hyp.kvar + hyp.noise;
  const WgCand cc = wg_candidates(cand, C, C <= 16);
  prepare_z(Z, M, Mp, true);                             // ZsT, V_Z, W_Z, base_z (forget_z on a miss drops the table too)
  wip_grad_table(M, Mp, y_std, logw, zv);
  const int nzw = (int)(Mp / 64), nnw = (int)((N + WG_ROWS - 1) / WG_ROWS);
  const size_t n_vec = (size_t)G * Np, n_a = (size_t)G * Mp;
  const size_t n_pn = (size_t)G * nnw * (nv + 1) * MAX_D;
  wg_ws.ensure((6 * n_vec + (3 + 4) * n_a + 16 + (size_t)G * nzw * 4 + (size_t)G * 4 * WGW_ZS + n_pn +
                (zv ? 6 * n_a + 16 : 0)) * sizeof(double));
  const WgFront f(wg_ws.d(), n_vec);
  double* crossA = f.end;
  double* vplusA = crossA + n_a;
  double* flagA = vplusA + n_a;
  double* wv = flagA + n_a;                         // [nv][G][Mp]
  double* sA = wv + 4 * n_a;
  double* pairs = sA + 16;
  double* zs = pairs + (size_t)G * nzw * 4;
  double* pn = zs + (size_t)G * 4 * WGW_ZS;
  double* rA = pn + n_pn;                           // zv: r, p, E, the constant flag, t, G [G][Mp] each, and h_c
  double* pA = rA + n_a;
  double* eA = pA + n_a;
  double* constA = eA + n_a;
  double* tA = constA + n_a;
  double* gA = tA + n_a;
  double* hA = gA + n_a;
  WgOut home(*this);
  WgwOut out;
  for (int k = 0; k < 4; ++k) {
    home.add(scores[k], (size_t)C, out.score[k]);
    home.add(grads[k], (size_t)C * d, out.grad[k]);
  }
  home.place(C <= 16);
  const Hyper& h = hyp;
  for (int64_t c0 = 0; c0 < C; c0 += 16) {
    const int64_t g = std::min<int64_t>(16, C - c0);
    const double* clater = cc.later + c0 * d;
    wg_front(cc, c0, g, f);
    with_kern_dcap(h.kern, d, [&](auto KE, auto DC) {
      hipLaunchKernelGGL((k_wg_cross_w<KE, DC>), dim3((unsigned)nzw, (unsigned)g), dim3(256), (size_t)N * sizeof(double),
                         stream, (const double*)ZsT.d(), Mp, M, (const double*)VZ.d(), Mp, N, Np, (const double*)f.vv, clater,
                         h, kself, (const double*)basez.d(), y_std * y_std, (const double*)zw.zt.d(), zw.ldt, mask, crossA,
                         vplusA, flagA, Mp, sA, pairs);
      if (zv) {
        hipLaunchKernelGGL(k_wg_zv_r, dim3((unsigned)g), dim3(256), 0, stream, (const double*)crossA, Mp, (const double*)sA,
                           (const double*)basez.d(), (const double*)zw.zt.d(), zw.ldt, M, Mp, y_std, rA, pA, eA, constA, hA);
        hipLaunchKernelGGL(k_wg_zv_pair, dim3((unsigned)nzw, (unsigned)g), dim3(256), 0, stream, (const double*)rA,
                           (const double*)pA, (const double*)eA, Mp, M, tA, gA);
        hipLaunchKernelGGL((k_wg_zv_fold<KE, DC>), dim3((unsigned)g), dim3(256), 0, stream, (const double*)ZsT.d(), Mp, M,
                           Mp, clater, h, y_std, (const double*)rA, (const double*)constA, (const double*)tA,
                           (const double*)gA, Mp, (const double*)sA, (const double*)hA, wv, zs);
      } else {
        hipLaunchKernelGGL((k_wg_weights_w<KE, DC>), dim3((unsigned)g), dim3(256), 0, stream, (const double*)ZsT.d(), Mp, M,
                           Mp, clater, h, y_std * y_std, (const double*)zw.zt.d(), zw.ldt, mask, logw ? 0 : 1,
                           (const double*)crossA, (const double*)vplusA, (const double*)flagA, Mp, (const double*)sA,
                           (const double*)pairs, nzw, G, wv, zs);
      }
      auto rows = [&](auto NV) {
        // (KE, DC are captured: their types carry the values)
        hipLaunchKernelGGL((k_wg_rows<decltype(KE)::value, decltype(DC)::value, decltype(NV)::value>),
                           dim3((unsigned)nnw, (unsigned)g), dim3(256), 0, stream, (const double*)XsT.d(), Np, N, Np, clater, h,
                           (const double*)WZ.d(), Mp, Mp, (const double*)wv, Mp, G, (const double*)f.uu, pn);
      };
      switch (nv) {
        case 1: rows(std::integral_constant<int, 1>{}); break;
        case 2: rows(std::integral_constant<int, 2>{}); break;
        case 3: rows(std::integral_constant<int, 3>{}); break;
        default: rows(std::integral_constant<int, 4>{}); break;
      }
    });
    hipLaunchKernelGGL(k_wg_final_w, dim3((unsigned)g), dim3(256), 0, stream, (const double*)zs, (const double*)pn, nnw, nv,
                       mask, h, c0, out);
    LAUNCH_CHECK();
  }
  home.finish();
  if (log_ez) HIPCHK(hipMemcpyAsync(log_ez, zw.log_ez(), sizeof(double), hipMemcpyDefault, stream));
  sync();
  home.scatter();
  return BOBE_OK;
}

// bobe_gp_wip_sweep_zvar: the sweep with the evidence-variance scorer alone (SweepW::zz), its argmin by k_argmin_masked with
// nothing masked (+inf never beats a finite score; all +inf: index 0) and log E[Z] from behind the table.
int bobe_gp::wip_sweep_zvar(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                            double* zvar, double* log_ez, int64_t* argmin, double* min) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (C <= 0 || M <= 0) throw Err(BOBE_ERR_ARG, "C and M must be positive");
  use();
  const bool want_min = argmin || min;
  SweepW w;
  w.logw = logw;
  SweepReq rq;
  rq.cand = cand; rq.C = C; rq.Z = Z; rq.M = M; rq.y_std = y_std;
  CallBuf stage, dmin;
  if (zvar && is_device_ptr(zvar)) w.zz = zvar;
  else { stage.ensure((size_t)C * sizeof(double)); w.zz = stage.d(); }
  rq.w = &w;
  sweep(rq);
  dmin.ensure(2 * sizeof(double));
  if (want_min)
    hipLaunchKernelGGL(k_argmin_masked, dim3(1), dim3(1024), 0, stream, (const double*)w.zz, C,
                       reinterpret_cast<int64_t*>(dmin.d() + 1), 0, dmin.d());
  LAUNCH_CHECK();
  if (zvar && w.zz != zvar) HIPCHK(hipMemcpyAsync(zvar, w.zz, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, stream));
  double hb[2] = {0.0, 0.0};
  if (want_min) HIPCHK(hipMemcpyAsync(hb, dmin.p, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (log_ez) HIPCHK(hipMemcpyAsync(log_ez, w.log_ez(), sizeof(double), hipMemcpyDefault, stream));
  sync();
  if (min) *min = hb[0];
  if (argmin) std::memcpy(argmin, hb + 1, sizeof(int64_t));
  return BOBE_OK;
}

int bobe_gp::wip_select_batch_zvar(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                                   int n_batch, int64_t* picks, double* pick_scores, double* stage_scores) {
  SweepW w;
  w.logw = logw;
  return select_batch(cand, C, Z, M, y_std, n_batch, 4, picks, pick_scores, stage_scores, &w);
}

int bobe_gp::wip_select_batch_w(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                                int n_batch, int criterion, int64_t* picks, double* pick_scores, double* stage_scores) {
  if (criterion < 0 || criterion > 3) throw Err(BOBE_ERR_ARG, "criterion must be 0 (WIPV), 1 (WIPStd), 2 (IMIQR) or 3 (EIV)");
  // equal weights with WIPV / WIPStd: the existing scorer at every stage
  if (!logw && criterion < 2)
    return select_batch(cand, C, Z, M, y_std, n_batch, criterion, picks, pick_scores, stage_scores, nullptr);
  SweepW w;
  w.logw = logw;
  return select_batch(cand, C, Z, M, y_std, n_batch, criterion, picks, pick_scores, stage_scores, &w);
}

// bobe_gp_evidence_moments: log E[Z] (bobe_gp_wip_sweep_zvar's bits: the same table launch) and log T0 = log (Var Z / E[Z]^2).
// prepare_z (the sweep's, with its cache of a repeated host Z), the per-z table with its lambda row, then k_evid_h ->
// k_evid_pairs over the lower tile pairs -> k_evid_fold, and one copy home.
namespace {
void configure_evidence_kernels() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  allow_big_lds(k_evid_pairs<0>, GEMM_SMEM_BYTES);
  allow_big_lds(k_evid_pairs<1>, GEMM_SMEM_BYTES);
}
constexpr int64_t EVID_CAP_DOUBLES = int64_t(1) << 31;   // the batch selection's cap (gp_batch.hip): 16 GiB
}  // namespace

int bobe_gp::evidence_moments(const double* Z, int64_t M, double y_std, const double* logw, double* log_ez, double* log_t0) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (M <= 0) throw Err(BOBE_ERR_ARG, "M must be positive");
  const int64_t Mp = round_up(M, TILE);
  // prepare_z keeps K(X,Z), V_Z and W_Z on the handle, Np x Mp each; the call adds one double per tile pair (nothing is read
  // or allocated before this test)
  const bool over = Mp > EVID_CAP_DOUBLES / (3 * Np);
  if (over || 3 * Np * Mp + (Mp / TILE) * (Mp / TILE + 1) / 2 > EVID_CAP_DOUBLES)
    throw Err(BOBE_ERR_ARG, "too many integration points: the handle's Z-side buffers, 3 x Np x Mp doubles, and the tile pairs' "
                            "sums exceed 16 GiB");
  use();
  configure_evidence_kernels();
  prepare_z(Z, M, Mp, false);
  SweepW w;
  w.logw = logw;
  wip_zterms(w, M, Mp, y_std, basez.d(), true, true);
  const int64_t nt = Mp / TILE, ntiles = nt * (nt + 1) / 2;
  CallBuf ev, parts, res;
  ev.ensure((size_t)(EVID_ROWS * Mp + 8) * sizeof(double));
  parts.ensure((size_t)ntiles * sizeof(double));
  res.ensure(8 * sizeof(double));
  hipLaunchKernelGGL(k_evid_h, dim3(1), dim3(256), 0, stream, (const double*)(w.zt.d() + 5 * w.ldt), (const double*)basez.d(), M,
                     Mp, y_std, ev.d());
  prof_begin(BOBE_PROF_CROSSVV);              // (the class of the tile products V^T V: k_cross_vv, k_sigma_tiles, the paths' product)
  if (kern == BOBE_KERNEL_RBF)
    hipLaunchKernelGGL(k_evid_pairs<0>, dim3((unsigned)ntiles), dim3(256), GEMM_SMEM_BYTES, stream, (const double*)VZ.d(), Mp,
                       Np, (const double*)ZsT.d(), Mp, (const double*)ev.d(), Mp, M, hyp, y_std, parts.d());
  else
    hipLaunchKernelGGL(k_evid_pairs<1>, dim3((unsigned)ntiles), dim3(256), GEMM_SMEM_BYTES, stream, (const double*)VZ.d(), Mp,
                       Np, (const double*)ZsT.d(), Mp, (const double*)ev.d(), Mp, M, hyp, y_std, parts.d());
  prof_end(BOBE_PROF_CROSSVV);
  hipLaunchKernelGGL(k_evid_fold, dim3(1), dim3(256), 0, stream, (const double*)parts.d(), ntiles,
                     (const double*)(ev.d() + EVID_ROWS * Mp), (const double*)w.log_ez(), res.d());   // log E[Z] rides home with it
  LAUNCH_CHECK();
  double hb[2] = {0.0, 0.0};
  HIPCHK(hipMemcpyAsync(hb, res.p, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
  if (log_t0) *log_t0 = hb[0];
  if (log_ez) *log_ez = hb[1];
  return BOBE_OK;
}
