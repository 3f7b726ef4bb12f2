// libbobe_gp.so, leave-one-out unit: the LOO predictive terms of the factorised state (bobe_gp_loo) and the LOO log
// pseudo-likelihood with its gradient at a hyper-parameter vector (bobe_gp_loo_objective).  Kernels: loo_kernels.hpp; the
// factorisation, the triangular inverse and K^-1 are gp_factor.hip's (factor_into, lauum).
#include "gp_handle.hpp"

#include "loo_kernels.hpp"

using namespace bobe;

namespace bobe {

void configure_loo_kernels() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  for_each_kern_dcap([](auto KE, auto DC) {
    allow_big_lds((k_loo_grad<KE, DC, 64>), GEMM64_SMEM_BYTES);
    allow_big_lds((k_loo_grad<KE, DC, 64, true>), GEMM64_SMEM_BYTES);
    allow_big_lds((k_loo_grad<KE, DC, 128>), GEMM_SMEM_BYTES);
  });
}

}  // namespace bobe

// a = diag(K^-1) from the inverse factor `linv`, then mean / var / lpd (and sqrt c, b / sqrt c when `with_grad_terms`) into
// loo_ws, and sum lpd into sum_out (device).  loo_ws: seven vectors of Np - a, mean, var, lpd, sqrt c, b / sqrt c, w.
void bobe_gp::loo_terms(const double* linv, const double* al, bool with_grad_terms, double* sum_out) {
  loo_ws.ensure((size_t)7 * Np * sizeof(double));
  double* ws = loo_ws.d();
  hipLaunchKernelGGL(k_loo_colsq_part, dim3((unsigned)(Np / 64), (unsigned)nb), dim3(256), 0, stream, linv, Np, part.d(), Np);
  hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((Np + 255) / 256), 1u), dim3(256), 0, stream, (const double*)part.d(), Np,
                     nb, 1, Np, ws, (int64_t)0, (int64_t)0);
  hipLaunchKernelGGL(k_loo_point, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, stream, (const double*)ws, al,
                     (const double*)y.d(), N, Np, ws + Np, ws + 2 * Np, ws + 3 * Np, with_grad_terms ? ws + 4 * Np : nullptr,
                     with_grad_terms ? ws + 5 * Np : nullptr);
  hipLaunchKernelGGL(k_loo_sum, dim3(1), dim3(256), 0, stream, (const double*)(ws + 3 * Np), N, sum_out);
  LAUNCH_CHECK();
}

// bobe_gp_loo: the factorised state's Linv and alpha, whatever installed them (factorisation, append, clone, set_chol)
int bobe_gp::loo_state(double* mean, double* var, double* lpd, double* sum_lpd) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  use();
  loo_terms(Linv.d(), alpha.d(), false, res.d() + 102);
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

// bobe_gp_loo_objective: the front of bobe_gp_mll's pipeline on the handle's own evaluation workspace (factor_into: up to
// Linv / alpha), then
//   value     a, the per-point terms, the fixed-order sum                                    (loo_terms)
//   gradient  K^-1 stored by the existing lauum into Tmp, B = diag(sqrt c) K^-1 into A (the factor L is no longer
//             needed), w = B^T (b / sqrt c), the dense B^T B tiles with the gradient epilogue, k_mll_grad_reduce.
// The workspace ends up holding no factor (A is overwritten): its record is cleared, bobe_gp_factor will not adopt it.
int bobe_gp::loo_objective(const Hyper& h, double* loo, double* grad) {
  use();
  EvalWs& ws = own;
  const FactorBufs f = ws.bufs();
  ws.tag[0].clear();
  const double floor_h = pivot_floor(h);
  factor_into(h, f);
  // the info word and the smallest pivot's root (res[100], res[101]), while A still holds L
  mll_terms(f.w, f.a, ws.res.d(), f.info);
  loo_terms(f.linv, f.alpha, grad != nullptr, ws.res.d() + 102);
  if (grad) {
    double* lw = loo_ws.d();
    (void)lauum(h, f.linv, f.alpha, f.xst, f.tmp, nullptr, ws.gpart.d());      // K^-1's lower tiles -> Tmp (its partial sums go unused)
    const int nt32 = (int)(Np / 32);
    hipLaunchKernelGGL(k_loo_make_b, dim3((unsigned)(nt32 * (nt32 + 1) / 2)), dim3(256), 0, stream, (const double*)f.tmp, Np,
                       (const double*)(lw + 4 * Np), f.a);
    hipLaunchKernelGGL(k_gemv_t_part, dim3((unsigned)(Np / 64), (unsigned)nb, 1u), dim3(256), 0, stream, (const double*)f.a, Np,
                       0, (const double*)(lw + 5 * Np), part.d(), Np, (int64_t)0, (int64_t)0, (int64_t)0);
    hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((Np + 255) / 256), 1u), dim3(256), 0, stream, (const double*)part.d(), Np,
                       nb, 0, Np, lw + 6 * Np, (int64_t)0, (int64_t)0);
    const LauumTiling t = lauum_tiling(nb);       // (the dense B^T B on the tiles and the tile core K^-1 was formed on)
    prof_begin(BOBE_PROF_LAUUM);
    with_lauum_variant(h.kern, h.d, t, [&](auto KE, auto DC, auto TT, auto GL) {
      hipLaunchKernelGGL((k_loo_grad<KE, DC, TT, GL>), dim3(t.ntiles), dim3(256),
                         (TT == 128 ? GEMM_SMEM_BYTES : GEMM64_SMEM_BYTES), stream, (const double*)f.a, Np, Np, N,
                         (const double*)f.alpha, (const double*)(lw + 6 * Np), (const double*)f.xst, Np, h, ws.gpart.d());
    });
    prof_end(BOBE_PROF_LAUUM);
    // (d + 1 workgroups: the gradient components; the scalar terms were reduced above)
    hipLaunchKernelGGL(k_mll_grad_reduce, dim3(d + 1), dim3(256), 0, stream, (const double*)ws.gpart.d(), t.ntiles,
                       dcap_of(d) + 1, d, dcap_of(d), ws.res.d(), (const double*)nullptr, (const double*)nullptr, Np, Np,
                       (const int*)nullptr, (int64_t)0, (int64_t)0, (int64_t)0, (int64_t)0);
    LAUNCH_CHECK();
  }
  res_to_host(ws.res.d(), ws.h_res, 103);
  const int st = eval_result(ws.h_res, floor_h, loo, grad);      // (bobe_gp_mll's rule; the value is the LOO sum instead)
  if (st == BOBE_OK) *loo = ws.h_res[102];
  return st;
}
