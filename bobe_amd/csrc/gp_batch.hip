// libbobe_gp.so, batch unit: one-sweep batch selection for WIPV / WIPStd (bobe_gp_wip_select_batch).  Kernels:
// batch_kernels.hpp (the downdates), kernels_common.hpp (k_gemv_t_part); stage 0 and every scoring launch are bobe_gp::sweep's
// and bobe_gp::wip_score's own (gp_sweep.hip).
// Every buffer of the call (the retained V, crossT, s_c, base_z copy, u rows, scores) belongs to the call and is freed before
// it returns.  The handle's Z-side state (ZsT, V_Z, base_z) is read, never written: a later bobe_gp_wip_sweep sees what it
// would have seen without the call.
#include "gp_handle.hpp"

#include "batch_kernels.hpp"

using namespace bobe;

namespace {
// Cap of the call's buffers that grow with the candidate count: 16 GiB = 2^31 doubles.  Counted are V, crossT, the scaled
// candidates and s_c, (Np + Mp + d + 1) x Cp, the row-block partial sums and the u rows of the later stages, (Np / 128 +
// n_batch - 1) x Cp, and the staging rows of scores that go to host memory, (n_batch or 1) x C.  N = 4096, d = 8 with 512
// integration points and the largest batch (64, all stage scores to the host: 4776 doubles per candidate) admits 449 536
// candidates; a larger pool is the caller's to split (BOBE_ERR_ARG).
constexpr size_t BATCH_KEEP_BYTES = size_t(16) << 30;
}  // namespace

int bobe_gp::wip_select_batch(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, int n_batch,
                              int criterion, int64_t* picks, double* pick_scores, double* stage_scores) {
  if (criterion != 0 && criterion != 1) throw Err(BOBE_ERR_ARG, "criterion must be 0 (WIPV) or 1 (WIPStd)");
  return select_batch(cand, C, Z, M, y_std, n_batch, criterion, picks, pick_scores, stage_scores, nullptr);
}

// w (bobe_gp_wip_select_batch_w, gp_criteria.hip): the weighted scorer in place of wip_score - stage 0's row comes from the
// sweep's own weighted pass and its argmin from k_argmin_masked with nothing masked (k_argmin's rule), a later stage refreshes
// the table's base_z terms from the call's downdated copy and scores with k_wip_score_w.  Everything else is shared.
// criterion 4 (bobe_gp_wip_select_batch_zvar only: the _w entry refuses it) is the evidence-variance scorer, k_wip_score_zz
// into SweepW::zz, with the table's lambda row refreshed at every stage like criterion 3's e row.
// dbg (bobe_debug_batch_terms): the same launches in the same order; a forced pick is a device-to-device copy over the pick
// record behind the stage's k_argmin_masked, and the state is copied out before the buffers go.  NULL: nothing is added.
int bobe_gp::select_batch(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, int n_batch,
                          int criterion, int64_t* picks, double* pick_scores, double* stage_scores, SweepW* w,
                          const BatchDebug* dbg) {
  if (C <= 0 || M <= 0) throw Err(BOBE_ERR_ARG, "C and M must be positive");
  if (n_batch < 1 || n_batch > BATCH_MAX || n_batch > C) throw Err(BOBE_ERR_ARG, "n_batch must be in [1, min(C, 64)]");
  if (criterion < 0 || criterion > (w ? 4 : 1)) throw Err(BOBE_ERR_ARG, "criterion out of range");
  if (!picks) throw Err(BOBE_ERR_ARG, "picks is NULL");
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  const int64_t Cp = round_up(C, TILE), Mp = round_up(M, TILE);
  const int nu = n_batch - 1;                            // u rows kept
  const int64_t* forced = dbg && nu > 0 ? dbg->forced : nullptr;
  if (forced)
    for (int j = 0; j < nu; ++j) {
      if (forced[j] < 0 || forced[j] >= C) throw Err(BOBE_ERR_ARG, "a forced pick lies outside [0, C)");
      for (int i = 0; i < j; ++i)
        if (forced[i] == forced[j]) throw Err(BOBE_ERR_ARG, "a forced pick is repeated");
    }
  const bool dev_scores = stage_scores && is_device_ptr(stage_scores);
  const size_t n_stage_rows = dev_scores ? 0 : (stage_scores ? (size_t)n_batch : 1);
  const size_t per_col = (size_t)(Np + Mp + d + 1) + (nu > 0 ? (size_t)(nb + nu) : 0);
  if ((per_col * (size_t)Cp + n_stage_rows * (size_t)C) * sizeof(double) > BATCH_KEEP_BYTES)
    throw Err(BOBE_ERR_ARG, "too many candidates: the call's buffers, (Np + Mp + d + 1 + Np / 128 + n_batch - 1) x Cp + staged "
                            "score rows x C doubles, exceed 16 GiB");
  use();
  const bool wipv = criterion == 0;
  CallBuf cst, vkeep, xT, scb, bz, scores, vstar, pin, partc, partz, uc, uz, dpick, dval, dforce;
  cst.ensure((size_t)d * Cp * sizeof(double));
  vkeep.ensure((size_t)Np * Cp * sizeof(double));
  xT.ensure((size_t)Mp * Cp * sizeof(double));
  scb.ensure((size_t)Cp * sizeof(double));
  dpick.ensure((size_t)n_batch * sizeof(int64_t));
  dval.ensure((size_t)n_batch * sizeof(double));
  // the scores of stage j: the caller's row j when stage_scores is device memory, else a row of a staging buffer (one
  // row, overwritten per stage, when the caller wants none)
  if (!dev_scores) scores.ensure(n_stage_rows * (size_t)C * sizeof(double));
  auto stage_row = [&](int j) -> double* {
    if (dev_scores) return stage_scores + (int64_t)j * C;
    return scores.d() + (stage_scores ? (int64_t)j * C : 0);
  };
  int64_t* d_picks = static_cast<int64_t*>(dpick.p);

  // ---- stage 0: the sweep itself, writing into the retained buffers
  SweepKeep keep;
  keep.CsT = cst.d();
  keep.V = vkeep.d();
  keep.crossT = xT.d();
  keep.sc = scb.d();
  keep.ld = Cp;
  int64_t pick0 = -1;
  double val0 = 0.0;
  SweepReq rq;
  rq.cand = cand; rq.C = C; rq.Z = Z; rq.M = M; rq.y_std = y_std;
  rq.keep = &keep;
  if (w) {
    for (double*& o : w->out) o = nullptr;
    (criterion == 4 ? w->zz : w->out[criterion]) = stage_row(0);
    rq.w = w;
    sweep(rq);
    hipLaunchKernelGGL(k_argmin_masked, dim3(1), dim3(1024), 0, stream, (const double*)stage_row(0), C, d_picks, 0,
                       static_cast<double*>(dval.p));
    LAUNCH_CHECK();
  } else {
    (wipv ? rq.wipv : rq.wipstd) = stage_row(0);
    (wipv ? rq.argmin_v : rq.argmin_s) = &pick0;
    (wipv ? rq.min_v : rq.min_s) = &val0;
    sweep(rq);                                           // (synchronises: pick0 / val0 are on the host)
    HIPCHK(hipMemcpyAsync(d_picks, &pick0, sizeof(int64_t), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dval.p, &val0, sizeof(double), hipMemcpyHostToDevice, stream));
  }

  // ---- stages 1 .. n_batch - 1: rank-one downdates of crossT, base_z, s_c and a rescoring, queued without a host round trip
  if (nu > 0) {
    bz.ensure((size_t)Mp * sizeof(double));
    vstar.ensure((size_t)Np * sizeof(double));
    pin.ensure((size_t)BATCH_PIN * sizeof(double));
    partc.ensure((size_t)nb * Cp * sizeof(double));
    partz.ensure((size_t)nb * Mp * sizeof(double));
    uc.ensure((size_t)nu * Cp * sizeof(double));
    uz.ensure((size_t)nu * Mp * sizeof(double));
    HIPCHK(hipMemcpyAsync(bz.p, basez.p, (size_t)Mp * sizeof(double), hipMemcpyDeviceToDevice, stream));
  } else if (dbg) {
    bz.ensure((size_t)Mp * sizeof(double));
    HIPCHK(hipMemcpyAsync(bz.p, basez.p, (size_t)Mp * sizeof(double), hipMemcpyDeviceToDevice, stream));
  }
  auto force = [&](int j) {                              // stage j's pick, before stage j + 1's k_batch_gather reads it
    if (forced && j < nu)
      HIPCHK(hipMemcpyAsync(d_picks + j, static_cast<int64_t*>(dforce.p) + j, sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  };
  if (forced) {
    dforce.ensure((size_t)nu * sizeof(int64_t));
    HIPCHK(hipMemcpyAsync(dforce.p, forced, (size_t)nu * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    force(0);
  }
  for (int j = 1; j < n_batch; ++j) {
    const int nprev = j - 1;
    double* ucj = uc.d() + (int64_t)nprev * Cp;
    double* uzj = uz.d() + (int64_t)nprev * Mp;
    hipLaunchKernelGGL(k_batch_gather, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, stream, keep.V_used, keep.ldv_used,
                       Np, (const double*)cst.d(), Cp, d, (const double*)scb.d(), (const double*)uc.d(), Cp, nprev,
                       (const int64_t*)(d_picks + nprev), vstar.d(), pin.d());
    // V_C^T v* and V_Z^T v*: partial sums per row block of 128, added up in k_batch_u
    hipLaunchKernelGGL(k_gemv_t_part, dim3((unsigned)(Cp / 64), (unsigned)nb), dim3(256), 0, stream, keep.V_used,
                       keep.ldv_used, 0, (const double*)vstar.d(), partc.d(), Cp, (int64_t)0, (int64_t)0, (int64_t)0);
    hipLaunchKernelGGL(k_gemv_t_part, dim3((unsigned)(Mp / 64), (unsigned)nb), dim3(256), 0, stream, (const double*)VZ.d(), Mp,
                       0, (const double*)vstar.d(), partz.d(), Mp, (int64_t)0, (int64_t)0, (int64_t)0);
    hipLaunchKernelGGL(k_batch_u, dim3((unsigned)((Cp + 255) / 256)), dim3(256), 0, stream, (const double*)partc.d(), Cp, nb,
                       (const double*)cst.d(), Cp, C, Cp, hyp, (const double*)pin.d(), (const double*)uc.d(), Cp, nprev, ucj,
                       scb.d());
    hipLaunchKernelGGL(k_batch_u, dim3((unsigned)((Mp + 255) / 256)), dim3(256), 0, stream, (const double*)partz.d(), Mp, nb,
                       (const double*)ZsT.d(), Mp, M, Mp, hyp, (const double*)pin.d(), (const double*)uz.d(), Mp, nprev, uzj,
                       bz.d());
    hipLaunchKernelGGL(k_batch_rank1, dim3((unsigned)((Cp + 255) / 256), (unsigned)(Mp / 16)), dim3(256), 0, stream, xT.d(), Cp, Cp,
                       (const double*)uzj, (const double*)ucj);
    double* row = stage_row(j);
    if (w) {
      if (criterion >= 3) wip_zterms(*w, M, Mp, y_std, bz.d(), false);
      if (criterion == 4) {
        w->zz = row;
        wip_score_zz(*w, xT.d(), Cp, cst.d(), scb.d(), bz.d(), C, M, Mp, y_std, 0);
      } else {
        w->out[criterion] = row;
        wip_score_w(*w, xT.d(), Cp, cst.d(), scb.d(), bz.d(), C, M, Mp, y_std, 0);
      }
    } else {
      wip_score(xT.d(), Cp, cst.d(), scb.d(), bz.d(), C, M, Mp, y_std, wipv ? row : nullptr, wipv ? nullptr : row, nullptr);
    }
    hipLaunchKernelGGL(k_argmin_masked, dim3(1), dim3(1024), 0, stream, (const double*)row, C, d_picks, j,
                       static_cast<double*>(dval.p) + j);
    LAUNCH_CHECK();
    force(j);
  }
  if (dbg) {
    auto rows_out = [&](double* dst, const double* src, int64_t ld, int64_t rows, int64_t cols) {
      if (dst && rows > 0)
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)cols * 8, src, (size_t)ld * 8, (size_t)cols * 8, (size_t)rows, hipMemcpyDeviceToHost,
                                stream));
    };
    rows_out(dbg->crossT, xT.d(), Cp, M, C);
    rows_out(dbg->sc, scb.d(), Cp, 1, C);
    rows_out(dbg->basez, bz.d(), Mp, 1, M);
    rows_out(dbg->UC, uc.d(), Cp, nu, C);
    rows_out(dbg->UZ, uz.d(), Mp, nu, M);
  }
  HIPCHK(hipMemcpyAsync(picks, dpick.p, (size_t)n_batch * sizeof(int64_t), hipMemcpyDefault, stream));
  if (pick_scores) HIPCHK(hipMemcpyAsync(pick_scores, dval.p, (size_t)n_batch * sizeof(double), hipMemcpyDefault, stream));
  if (stage_scores && !dev_scores)
    HIPCHK(hipMemcpyAsync(stage_scores, scores.p, (size_t)n_batch * C * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
  return BOBE_OK;
}

// bobe_debug_batch_terms: select_batch itself with n_stage + 1 stages, routed as the three shipped entries route it (the
// equal-weight scorer for criterion 0 / 1 without log-weights, else the weighted one; 4: the evidence variance).
int bobe_gp::debug_batch_terms(const double* cand, int64_t C, const double* Z, int64_t M, double y_std, const double* logw,
                               int criterion, int n_stage, const int64_t* forced, double* crossT, double* sc_out,
                               double* basez_out, double* UC, double* UZ, int64_t* picks, double* stage_scores) {
  if (n_stage < 0 || n_stage > BATCH_MAX - 1) throw Err(BOBE_ERR_ARG, "n_stage must be in [0, 63]");
  if (criterion < 0 || criterion > 4) throw Err(BOBE_ERR_ARG, "criterion must be 0 .. 4");
  BatchDebug dbg;
  dbg.forced = forced; dbg.crossT = crossT; dbg.sc = sc_out; dbg.basez = basez_out; dbg.UC = UC; dbg.UZ = UZ;
  int64_t own[BATCH_MAX];
  if (!picks) picks = own;
  if (!logw && criterion < 2)
    return select_batch(cand, C, Z, M, y_std, n_stage + 1, criterion, picks, nullptr, stage_scores, nullptr, &dbg);
  SweepW w;
  w.logw = logw;
  return select_batch(cand, C, Z, M, y_std, n_stage + 1, criterion, picks, nullptr, stage_scores, &w, &dbg);
}

// bobe_debug_sweep_terms: the sweep of stage 0 above - bobe_gp_wip_sweep's launches in their order, a WIPV row as the scorer's
// output - into call-local retention buffers, then V_used, V_Z, crossT, s_c and base_z copied to the host without their
// padding.  The retention buffers and the score row count against select_batch's cap.
int bobe_gp::debug_sweep_terms(const double* cand, int64_t C, const double* Z, int64_t M, double* V, double* VZ_out,
                               double* crossT, double* sc_out, double* basez_out) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (C <= 0 || M <= 0) throw Err(BOBE_ERR_ARG, "C and M must be positive");
  const int64_t Cp = round_up(C, TILE), Mp = round_up(M, TILE);
  if (((size_t)(Np + Mp + d + 1) * (size_t)Cp + (size_t)C) * sizeof(double) > BATCH_KEEP_BYTES)
    throw Err(BOBE_ERR_ARG, "too many candidates: the call's buffers, (Np + Mp + d + 1) x Cp + C doubles, exceed 16 GiB");
  use();
  CallBuf cst, vkeep, xT, scb, scores;
  cst.ensure((size_t)d * Cp * sizeof(double));
  vkeep.ensure((size_t)Np * Cp * sizeof(double));
  xT.ensure((size_t)Mp * Cp * sizeof(double));
  scb.ensure((size_t)Cp * sizeof(double));
  scores.ensure((size_t)C * sizeof(double));
  SweepKeep keep;
  keep.CsT = cst.d();
  keep.V = vkeep.d();
  keep.crossT = xT.d();
  keep.sc = scb.d();
  keep.ld = Cp;
  SweepReq rq;
  rq.cand = cand; rq.C = C; rq.Z = Z; rq.M = M;
  rq.wipv = scores.d();
  rq.keep = &keep;
  sweep(rq);
  auto rows_out = [&](double* dst, const double* src, int64_t ld, int64_t rows, int64_t cols) {
    if (dst)
      HIPCHK(hipMemcpy2DAsync(dst, (size_t)cols * 8, src, (size_t)ld * 8, (size_t)cols * 8, (size_t)rows, hipMemcpyDeviceToHost,
                              stream));
  };
  rows_out(V, keep.V_used, keep.ldv_used, N, C);
  rows_out(VZ_out, VZ.d(), Mp, N, M);
  rows_out(crossT, xT.d(), Cp, M, C);
  rows_out(sc_out, scb.d(), Cp, 1, C);
  rows_out(basez_out, basez.d(), Mp, 1, M);
  sync();
  return BOBE_OK;
}
