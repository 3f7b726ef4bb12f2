// libbobe_gp.so, criteria unit: importance-weighted integration points and the IMIQR / EIV criteria (bobe_gp_wip_sweep_w,
// bobe_gp_wip_select_batch_w).  Kernels: criteria_kernels.hpp (the per-z table, the weighted scorer), batch_kernels.hpp
// (k_argmin_masked).  The launch sequence is bobe_gp::sweep's (gp_sweep.hip) and the batch selection's (gp_batch.hip): this
// unit adds one scoring pass per super-chunk and one small kernel per call (per stage for criterion 3).
// The per-z table, the partial sums, the staged weights and outputs belong to the call (SweepW's CallBufs) and are freed
// before it returns.  One buffer of the handle is written: kXZ, the sweep workspace's K(X, Z), which prepare_z fills and
// nothing reads once prepare_z is through (the substitution path overwrites it there) - scratch, rewritten here with its
// own bits; the handle's Z-side STATE (ZsT, V_Z, base_z and prepare_z's cache of them) is read, never written.
#include "gp_handle.hpp"

#include "batch_kernels.hpp"
#include "criteria_kernels.hpp"

using namespace bobe;

void bobe_gp::wip_zterms(SweepW& w, int64_t M, int64_t Mp, double y_std, const double* bz, bool first) {
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
                     w.zt.d(), Mp, first ? 1 : 0, w.log_s());
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
