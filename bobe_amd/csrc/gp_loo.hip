// libbobe_gp.so, leave-one-out unit: the LOO predictive terms of the factorised state (bobe_gp_loo) and the LOO log
// pseudo-likelihood with its gradient at a hyper-parameter vector (bobe_gp_loo_objective) or at several in lock step
// (bobe_gp_loo_objective_batch), and the noise component that the *_noise entry points append to the gradient of either
// objective (mll_noise_tail, loo_noise_tail).  Kernels: loo_kernels.hpp; the factorisation, the triangular inverse and K^-1
// are gp_factor.hip's (factor_into, lauum).
#include "gp_handle.hpp"

#include "loo_kernels.hpp"

using namespace bobe;

namespace bobe {

void configure_loo_kernels() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  for_each_kern_dcap([](auto KE, auto DC) {
    allow_big_lds((k_loo_grad<KE, DC, 64>), GEMM64_SMEM_BYTES);
    allow_big_lds((k_loo_grad<KE, DC, 128>), GEMM_SMEM_BYTES);
  });
}

}  // namespace bobe

// a = diag(K^-1) of f's members, from their inverse factors through f.part into the first vector of their LOO blocks
void bobe_gp::loo_kinv_diag(const FactorBufs& f) {
  const unsigned nm = (unsigned)f.B;
  hipLaunchKernelGGL(k_loo_colsq_part, dim3((unsigned)(Np / 64), (unsigned)nb, nm), dim3(256), 0, stream,
                     (const double*)f.linv, Np, f.part, Np, f.mat, f.prt);
  hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((Np + 255) / 256), nm), dim3(256), 0, stream, (const double*)f.part, Np,
                     nb, 1, Np, f.loo, f.prt, f.lvs);
}

// a (loo_kinv_diag), then mean / var / lpd (and sqrt c, b / sqrt c when `with_grad_terms`) into the LOO blocks, and sum lpd
// into res[102].  A LOO block: seven vectors of Np per member - a, mean, var, lpd, sqrt c, b / sqrt c, w.
void bobe_gp::loo_terms(const FactorBufs& f, bool with_grad_terms) {
  const unsigned nm = (unsigned)f.B;
  double* lw = f.loo;
  loo_kinv_diag(f);
  hipLaunchKernelGGL(k_loo_point, dim3((unsigned)((Np + 255) / 256), nm), dim3(256), 0, stream, (const double*)lw,
                     (const double*)f.alpha, (const double*)y.d(), N, Np, lw + Np, lw + 2 * Np, lw + 3 * Np,
                     with_grad_terms ? lw + 4 * Np : nullptr, with_grad_terms ? lw + 5 * Np : nullptr, f.vec, f.lvs);
  hipLaunchKernelGGL(k_loo_sum, dim3(1, nm), dim3(256), 0, stream, (const double*)(lw + 3 * Np), N, f.res + 102, f.lvs, f.rs);
  LAUNCH_CHECK();
}

// bobe_gp_loo: the factorised state's Linv and alpha, whatever installed them (factorisation, append, clone, set_chol)
int bobe_gp::loo_state(double* mean, double* var, double* lpd, double* sum_lpd) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  use();
  loo_ws.ensure((size_t)7 * Np * sizeof(double));
  loo_terms(state_bufs(), false);
  const double* ws = loo_ws.d();
  double* outs[3] = {mean, var, lpd};
  for (int q = 0; q < 3; ++q)
    if (outs[q])
      HIPCHK(hipMemcpyAsync(outs[q], ws + (q + 1) * Np, (size_t)N * sizeof(double),
                            is_device_ptr(outs[q]) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  if (sum_lpd)
    HIPCHK(hipMemcpyAsync(sum_lpd, res.d() + 102, sizeof(double),
                          is_device_ptr(sum_lpd) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  sync();
  if (not_pd) {                        // (the NaN state gave NaN outputs)
    g_err = "the factorised state is not positive definite";
    return BOBE_NOT_PD;
  }
  return BOBE_OK;
}

// The launches bobe_gp_mll_noise appends to an evaluation with a gradient (eval_enqueue, after everything it queues
// otherwise): a = diag(K~^-1) from the members' inverse factors into their LOO blocks, then 1/2 nu (sum alpha^2 - sum a) into
// res[2 + d + 1].  Writes part, the LOO block and that one result: L, Linv, alpha, w stay what bobe_gp_factor adopts.
void bobe_gp::mll_noise_tail(const FactorBufs& f, const Hyper* hs, const Hyper* hdev) {
  loo_kinv_diag(f);
  hipLaunchKernelGGL(k_noise_mll_grad, dim3(1, (unsigned)f.B), dim3(256), 0, stream, (const double*)f.loo,
                     (const double*)f.alpha, N, hs[0].noise, hdev, f.res + 2 + d + 1, f.lvs, f.vec, f.rs);
}

// The launches bobe_gp_loo_objective_noise appends (loo_enqueue, after k_mll_grad_reduce): A holds the dense B = diag(sqrt c)
// K~^-1, the LOO block w; |B|_F^2 over the true N x N block in two stages through part, then -nu (|B|_F^2 + w^T alpha) into
// res[2 + d + 1].
void bobe_gp::loo_noise_tail(const FactorBufs& f, const Hyper* hs, const Hyper* hdev) {
  const unsigned nm = (unsigned)f.B;
  hipLaunchKernelGGL(k_loo_bsq_part, dim3((unsigned)(Np / 64), (unsigned)nb, nm), dim3(256), 0, stream, (const double*)f.a, Np,
                     N, f.part, Np, f.mat, f.prt);
  hipLaunchKernelGGL(k_noise_loo_grad, dim3(1, nm), dim3(256), 0, stream, (const double*)f.part, Np, nb,
                     (const double*)(f.loo + 6 * Np), (const double*)f.alpha, N, hs[0].noise, hdev, f.res + 2 + d + 1, f.prt,
                     f.lvs, f.vec, f.rs);
}

// The launches of B LOO evaluations on ws, on the current stream - eval_enqueue's counterpart: the single evaluation (B = 1,
// stride 0, h by value) and the lock-step batch (every launch widened by the member dimension, the hyper-parameters read
// from the workspace's device copy).  The front of bobe_gp_mll's pipeline (factor_into: up to Linv / alpha), then
//   value     the info word and the smallest pivot's root (res[100], res[101]) while A still holds L, a, the per-point
//             terms, the fixed-order sum into res[102]                                                       (loo_terms)
//   gradient  K^-1 stored by the existing lauum into Tmp (its partial sums go unused), B = diag(sqrt c) K^-1 into A (the
//             factor L is no longer needed), w = B^T (b / sqrt c), the dense B^T B tiles with the gradient epilogue,
//             k_mll_grad_reduce on the d + 1 gradient components.
// Without a gradient the list stops after the value.  noise_grad (with a gradient only): loo_noise_tail's launches follow.
// Results land in the pinned ws.h_res[b * 128 + ...].
void bobe_gp::loo_enqueue(EvalWs& ws, int B, const Hyper* hs, bool want_grad, const Hyper* hdev, bool noise_grad) {
  const FactorBufs f = ws.bufs(B);
  double* lw = f.loo;
  const unsigned nm = (unsigned)B;
  if (hdev) HIPCHK(hipMemcpyAsync(ws.hyp.p, ws.h_hyp, (size_t)B * sizeof(Hyper), hipMemcpyHostToDevice, stream));
  factor_into(hs[0], f, hdev);
  hipLaunchKernelGGL(k_mll_terms, dim3(nm), dim3(256), 0, stream, (const double*)f.w, (const double*)f.a, Np, Np, f.res, f.vec,
                     f.mat, f.rs, (const int*)f.info);
  loo_terms(f, want_grad);
  if (want_grad) {
    (void)lauum(hs[0], f, hdev, true);
    const int nt32 = (int)(Np / 32);
    hipLaunchKernelGGL(k_loo_make_b, dim3((unsigned)(nt32 * (nt32 + 1) / 2), nm), dim3(256), 0, stream, (const double*)f.tmp, Np,
                       (const double*)(lw + 4 * Np), f.a, f.mat, f.lvs);
    hipLaunchKernelGGL(k_gemv_t_part, dim3((unsigned)(Np / 64), (unsigned)nb, nm), dim3(256), 0, stream, (const double*)f.a, Np, 0,
                       (const double*)(lw + 5 * Np), f.part, Np, f.mat, f.lvs, f.prt);
    hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((Np + 255) / 256), nm), dim3(256), 0, stream, (const double*)f.part, Np,
                       nb, 0, Np, lw + 6 * Np, f.prt, f.lvs);
    const LauumTiling t = lauum_tiling(nb);       // (the dense B^T B on the tiles and the tile core K^-1 was formed on)
    prof_begin(BOBE_PROF_LAUUM);
    with_lauum_variant(hs[0].kern, hs[0].d, t, [&](auto KE, auto DC, auto TT) {
      hipLaunchKernelGGL((k_loo_grad<KE, DC, TT>), dim3(t.ntiles * B), dim3(256),
                         (TT == 128 ? GEMM_SMEM_BYTES : GEMM64_SMEM_BYTES), stream, (const double*)f.a, Np, Np, N,
                         (const double*)f.alpha, (const double*)(lw + 6 * Np), (const double*)f.xst, Np, hs[0], f.gpart,
                         hdev, f.mat, f.vec, f.lvs, f.xs, f.gps, B);
    });
    prof_end(BOBE_PROF_LAUUM);
    // (d + 1 workgroups per member: the gradient components; the scalar terms were reduced above)
    hipLaunchKernelGGL(k_mll_grad_reduce, dim3(d + 1, nm), dim3(256), 0, stream, (const double*)f.gpart, t.ntiles,
                       dcap_of(d) + 1, d, dcap_of(d), f.res, (const double*)nullptr, (const double*)nullptr, Np, Np,
                       (const int*)nullptr, f.gps, f.rs, (int64_t)0, (int64_t)0);
    if (noise_grad) loo_noise_tail(f, hs, hdev);
  }
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(ws.h_res, ws.res.p, (size_t)(ws.width > 1 ? B * 128 : 103) * sizeof(double), hipMemcpyDeviceToHost,
                        stream));
}

// Start-to-collect of B LOO evaluations on ws.  With a gradient a member ends up holding no factor (A is overwritten): its
// record is cleared - also one armed by an earlier bobe_gp_mll_batch on the same member - and stays cleared, so that
// bobe_gp_factor never adopts it.  A member's status is bobe_gp_mll's rule (eval_result) on its own info word and
// smallest pivot; the value is the LOO sum instead.  noise_grad: d + 2 gradient entries per member, the last d L_LOO / d log nu.
int bobe_gp::loo_eval(EvalWs& ws, int B, const Hyper* hs, double* loo, double* grad, int* status, bool noise_grad) {
  const int ng = d + 1 + (noise_grad ? 1 : 0);
  UseWs use_ws(*this, ws);
  for (int b = 0; b < B; ++b) {
    ws.tag[b].clear();
    ws.h_hyp[b] = hs[b];
    ws.floor[b] = pivot_floor(hs[b]);
  }
  loo_enqueue(ws, B, hs, grad != nullptr, ws.width > 1 ? static_cast<const Hyper*>(ws.hyp.p) : nullptr,
              noise_grad && grad != nullptr);
  sync();
  int worst = BOBE_OK;
  for (int b = 0; b < B; ++b) {
    const double* hr = ws.h_res + (size_t)b * 128;
    const int st = eval_result(hr, ws.floor[b], loo + b, grad ? grad + (size_t)b * ng : nullptr, noise_grad);
    if (st == BOBE_OK) loo[b] = hr[102];
    if (status) status[b] = st;
    if (st != BOBE_OK) worst = st;
  }
  return worst;
}

// bobe_gp_loo_objective (_noise): the width-1, stride-0 case on the handle's own evaluation workspace
int bobe_gp::loo_objective(const Hyper& h, double* loo, double* grad, bool noise_grad) {
  use();
  return loo_eval(own, 1, &h, loo, grad, nullptr, noise_grad);
}

// bobe_gp_loo_objective_batch: BOBE_MAX_MLL_SLOTS members at a time in lock step on the batch workspace, as bobe_gp_mll_batch;
// a lone member, and every member below BOBE_LOCKSTEP_MIN_N points, takes the single path (there is no slot form).
// noise (bobe_gp_loo_objective_noise_batch; NULL: the installed one): the members' own noise levels, and d + 2 gradient entries.
int bobe_gp::loo_batch(int64_t B, const double* ls, const double* kvar, double* loo, double* grad, int* status,
                       const double* noise) {
  use();
  const int ng = d + 1 + (noise ? 1 : 0);
  const bool lockstep = N >= tuning().lockstep_min_n;
  int worst = BOBE_OK;
  for (int64_t b0 = 0; b0 < B; b0 += BOBE_MAX_MLL_SLOTS) {
    const int nbat = (int)std::min<int64_t>(BOBE_MAX_MLL_SLOTS, B - b0);
    Hyper hs[BOBE_MAX_MLL_SLOTS];
    for (int i = 0; i < nbat; ++i) {
      hs[i] = hyp;
      for (int j = 0; j < d; ++j) hs[i].ls[j] = ls[(b0 + i) * d + j];
      hs[i].kvar = kvar[b0 + i];
      if (noise) hs[i].noise = noise[b0 + i];
    }
    double* gr = grad ? grad + b0 * ng : nullptr;
    int* sts = status ? status + b0 : nullptr;
    if (lockstep && nbat >= 2) {
      ensure_batch(nbat);
      const int st = loo_eval(batch, nbat, hs, loo + b0, gr, sts, noise != nullptr);
      if (st != BOBE_OK) worst = st;
      continue;
    }
    for (int i = 0; i < nbat; ++i) {
      const int st = loo_eval(own, 1, hs + i, loo + b0 + i, gr ? gr + (size_t)i * ng : nullptr, sts ? sts + i : nullptr,
                              noise != nullptr);
      if (st != BOBE_OK) worst = st;
    }
  }
  return worst;
}
