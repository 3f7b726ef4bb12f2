// libbobe_gp.so, consumers unit: what reads the factorised surrogate besides the sweep - Hamiltonian Monte Carlo on the
// posterior mean, EI / LogEI, the classifier gate of GPwithClassifier, GP.kernel, the device-side clone - and the
// handle's teardown.  Kernels: kernels_common.hpp, consumer_kernels.hpp.
#include "gp_handle.hpp"

#include "consumer_kernels.hpp"

using namespace bobe;

namespace bobe {
void configure_consumer_kernels() {       // (the chain kernels keep training points in up to 150 KB of LDS)
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  for_each_kern_dcap([](auto KE, auto DC) {
    allow_big_lds((k_hmc_run<KE, DC>), CHAIN_LDS_BYTES);
    allow_big_lds((k_rwalk<KE, DC>), CHAIN_LDS_BYTES);
    allow_big_lds((k_nuts_run<KE, DC>), NUTS_LDS_BYTES);
  });
}
}  // namespace bobe

// ---- classifier gate ------------------------------------------------------------------------------------------------
void bobe_gp::set_gate(const double* sv, int64_t n_sv, const double* dual, double intercept, double gamma, double threshold,
                       double minus_inf) {
  use();
  sync();
  if (!sv || n_sv <= 0) {                      // clear
    gate = Gate{nullptr, nullptr, 0, 0, 0.0, 0.0, threshold, minus_inf, GATE_NONE, nullptr, nullptr, 0.0, 0.0};
    return;
  }
  if (!dual) throw Err(BOBE_ERR_ARG, "dual_coef is NULL");
  if (n_sv > INT_MAX) throw Err(BOBE_ERR_ARG, "too many support vectors");
  // support vectors SoA (coordinate j of vector i at svT[j * n_sv + i]): a wave's lanes read consecutive vectors
  std::vector<double> host_sv((size_t)n_sv * d), svt((size_t)n_sv * d);
  const double* hs = sv;
  if (is_device_ptr(sv)) {
    HIPCHK(hipMemcpy(host_sv.data(), sv, host_sv.size() * sizeof(double), hipMemcpyDeviceToHost));
    hs = host_sv.data();
  }
  for (int64_t i = 0; i < n_sv; ++i)
    for (int j = 0; j < d; ++j) svt[(size_t)j * n_sv + i] = hs[i * d + j];
  gate_sv.ensure(svt.size() * sizeof(double));
  gate_dual.ensure((size_t)n_sv * sizeof(double));
  HIPCHK(hipMemcpy(gate_sv.p, svt.data(), svt.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(gate_dual.p, dual, (size_t)n_sv * sizeof(double),
                   is_device_ptr(dual) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  gate = Gate{gate_sv.d(), gate_dual.d(), n_sv, (int)n_sv, intercept, gamma, threshold, minus_inf, GATE_SVM, nullptr,
              nullptr, 0.0, 0.0};
}

// the reference's raw flat_L (tril_indices order) -> L with softplus(.) + 1e-4 on the diagonal, once, dense row-major
void bobe_gp::set_gate_ellipsoid(const double* flat_L, const double* mu, double alpha, double beta, double threshold,
                                 double minus_inf) {
  if (!flat_L || !mu) throw Err(BOBE_ERR_ARG, "flat_L / mu is NULL");
  use();
  sync();
  const int T = d * (d + 1) / 2;
  std::vector<double> fl(T), m(d), buf((size_t)d * d + d, 0.0);
  HIPCHK(hipMemcpy(fl.data(), flat_L, T * sizeof(double), is_device_ptr(flat_L) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  HIPCHK(hipMemcpy(m.data(), mu, d * sizeof(double), is_device_ptr(mu) ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
  for (int i = 0, p = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j, ++p) {
      const double v = fl[p];
      buf[(size_t)i * d + j] = (i == j) ? std::fmax(v, 0.0) + std::log1p(std::exp(-std::fabs(v))) + 1e-4 : v;
    }
  for (int j = 0; j < d; ++j) buf[(size_t)d * d + j] = m[j];
  gate_ell.ensure(buf.size() * sizeof(double));
  HIPCHK(hipMemcpy(gate_ell.p, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
  gate = Gate{nullptr, nullptr, 0, 0, 0.0, 0.0, threshold, minus_inf, GATE_ELLIPSOID, gate_ell.d(), gate_ell.d() + (size_t)d * d,
              alpha, beta};
}

void bobe_gp::train_ellipsoid(const double* X, const double* yv, int64_t N, const double* mu, int n_restarts,
                              const double* init, const int32_t* perm, int n_epochs, int batch, double lr, double wd,
                              double* params_out, double* loss_out) {
  if (N < 1 || n_restarts < 1 || n_epochs < 0 || batch < 1) throw Err(BOBE_ERR_ARG, "bad argument");
  if (N > INT_MAX) throw Err(BOBE_ERR_ARG, "N too large");
  const int B = (int)std::min<int64_t>(batch, N);
  const int steps = (int)std::max<int64_t>(1, N / batch);
  const int P = d * (d + 1) / 2 + 2;
  const size_t np = (size_t)n_restarts * n_epochs * steps * B;
  for (size_t i = 0; i < np; ++i)                       // (every row index the kernel will read must exist)
    if ((uint32_t)perm[i] >= (uint32_t)N) throw Err(BOBE_ERR_ARG, "perm holds a row index outside [0, N)");
  use();
  // workspace: X (N d) | y (N) | mu (d) | init (R P) | params_out (R P) | loss_out (R)
  const size_t nx = (size_t)N * d, ni = (size_t)n_restarts * P;
  ell_ws.ensure((nx + N + d + 2 * ni + n_restarts) * sizeof(double));
  double* dX = ell_ws.d();
  double* dy = dX + nx;
  double* dmu = dy + N;
  double* dinit = dmu + d;
  double* dout = dinit + ni;
  double* dloss = dout + ni;
  ell_perm.ensure(std::max<size_t>(np, 1) * sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(dX, X, nx * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dy, yv, N * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dmu, mu, d * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dinit, init, ni * sizeof(double), hipMemcpyHostToDevice, stream));
  if (np) HIPCHK(hipMemcpyAsync(ell_perm.p, perm, np * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_ellipsoid_train, dim3((unsigned)n_restarts), dim3(ELL_NT), 0, stream, (const double*)dX,
                     (const double*)dy, N, d, (const double*)dmu, (const double*)dinit, (const int*)ell_perm.p, n_epochs,
                     steps, B, lr, wd, dout, dloss);
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(params_out, dout, ni * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(loss_out, dloss, n_restarts * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
}

void bobe_gp::gate_apply(const double* xq_dev, int64_t C, double* decision, double* feasible, double* mean, double* var,
                         double* dmean, double* dvar, double* proba) {
  if (!gate_on(gate)) throw Err(BOBE_ERR_STATE, "no classifier gate is set (bobe_gp_set_gate)");
  with_dcap(d, [&](auto DC) {
    hipLaunchKernelGGL((k_gate<DC>), dim3((unsigned)C), dim3(256), 0, stream, gate, xq_dev, d, decision, feasible, mean, var,
                       dmean, dvar, proba);
  });
  LAUNCH_CHECK();
}

void bobe_gp::gate_eval(const double* Xq, int64_t C, double* decision, double* feasible) {
  if (C <= 0) throw Err(BOBE_ERR_ARG, "C must be positive");
  use();
  const double* cin = fetch(Xq, (size_t)C * d, in_stage);
  double* d_dec = out_dev(decision, C, o_mean);
  double* d_fe = out_dev(feasible, C, o_var);
  gate_apply(cin, C, d_dec, d_fe, nullptr, nullptr, nullptr, nullptr);
  out_finish(decision, C, o_mean);
  out_finish(feasible, C, o_var);
  sync();
}

void bobe_gp::gate_proba(const double* Xq, int64_t C, double* proba) {
  if (C <= 0) throw Err(BOBE_ERR_ARG, "C must be positive");
  use();
  const double* cin = fetch(Xq, (size_t)C * d, in_stage);
  double* d_p = out_dev(proba, C, o_mean);
  gate_apply(cin, C, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_p);
  out_finish(proba, C, o_mean);
  sync();
}

void bobe_gp::acq_ei(const double* Xq, int64_t C, double best_y, double zeta, int mode, double* out) {
  use();
  o_mean.ensure(C * sizeof(double));
  o_var.ensure(C * sizeof(double));
  // (predict_single, acquisition.py:246 / 323: gated for a GPwithClassifier)
  SweepReq rq;
  rq.cand = Xq; rq.C = C;
  rq.mean = o_mean.d(); rq.var = o_var.d();
  rq.gated = true;
  sweep(rq);
  double* d_out = out_dev(out, C, o_wipv);
  hipLaunchKernelGGL(k_ei, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, (const double*)o_mean.d(),
                     (const double*)o_var.d(), C, best_y, zeta, mode, d_out, gate.minus_inf);
  LAUNCH_CHECK();
  out_finish(out, C, o_wipv);
  sync();
}

void bobe_gp::acq_ei_grad(const double* Xq, int64_t C, double best_y, double zeta, int mode, double* val, double* grad) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (C <= 0) throw Err(BOBE_ERR_ARG, "C must be positive");
  if (mode != 0 && mode != 1) throw Err(BOBE_ERR_ARG, "mode must be 0 (EI) or 1 (LogEI)");
  use();
  const size_t cd = (size_t)C * d;
  const double* cin = fetch(Xq, cd, in_stage);
  // the posterior and its gradients stay in the staging buffers predict_grad copies home from; host outputs are staged in
  // o_misc, the value in front of the gradient
  o_mean.ensure((size_t)C * sizeof(double));
  o_var.ensure((size_t)C * sizeof(double));
  o_wipv.ensure(cd * sizeof(double));
  o_wipstd.ensure(cd * sizeof(double));
  const bool val_dev = is_device_ptr(val), grad_dev = is_device_ptr(grad);
  if (!val_dev || !grad_dev) o_misc.ensure(((size_t)C + cd) * sizeof(double));
  predict_grad_chain(cin, C, o_mean.d(), o_var.d(), o_wipv.d(), o_wipstd.d());
  double* d_val = val_dev ? val : o_misc.d();
  double* d_grad = grad_dev ? grad : o_misc.d() + C;
  hipLaunchKernelGGL(k_ei_grad, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, (const double*)o_mean.d(),
                     (const double*)o_var.d(), (const double*)o_wipv.d(), (const double*)o_wipstd.d(), C, d, best_y, zeta,
                     mode, gate.minus_inf, d_val, d_grad);
  LAUNCH_CHECK();
  if (!val_dev) HIPCHK(hipMemcpyAsync(val, d_val, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (!grad_dev) HIPCHK(hipMemcpyAsync(grad, d_grad, cd * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
}

void bobe_gp::hmc_leapfrog(int64_t P, double* U, double* Pm, const double* inv_mass, double eps, int L, double y_std,
                           double y_mean, double temp, double* logp, double* grad, double* mean, double* X) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (P <= 0 || L < 1 || !(temp > 0.0)) throw Err(BOBE_ERR_ARG, "bad argument");
  use();
  const size_t pd = (size_t)P * d;
  // staging: [U | Pm | grad | X] (P*d each), [logp | mean] (P each), inv_mass (d)
  in_stage.ensure((4 * pd + 2 * (size_t)P + d) * sizeof(double));
  double* dU = in_stage.d();
  double* dP = dU + pd;
  double* dG = dP + pd;
  double* dX = dG + pd;
  double* dL = dX + pd;
  double* dM = dL + P;
  double* dI = dM + P;
  const bool dev = is_device_ptr(U);
  const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIPCHK(hipMemcpyAsync(dU, U, pd * sizeof(double), in, stream));
  HIPCHK(hipMemcpyAsync(dP, Pm, pd * sizeof(double), in, stream));
  HIPCHK(hipMemcpyAsync(dI, inv_mass, (size_t)d * sizeof(double), is_device_ptr(inv_mass) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        stream));
  with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) {
    hipLaunchKernelGGL((k_hmc_leapfrog<KE, DC>), dim3((unsigned)P), dim3(256), 0, stream, (const double*)XsT.d(), Np, N,
                       (const double*)alpha.d(), hyp, dU, dP, (const double*)dI, eps, L, y_std, y_mean, temp, dL, dG, dM, dX,
                       gate);
  });
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(U, dU, pd * sizeof(double), out, stream));
  HIPCHK(hipMemcpyAsync(Pm, dP, pd * sizeof(double), out, stream));
  HIPCHK(hipMemcpyAsync(grad, dG, pd * sizeof(double), out, stream));
  HIPCHK(hipMemcpyAsync(X, dX, pd * sizeof(double), out, stream));
  HIPCHK(hipMemcpyAsync(logp, dL, (size_t)P * sizeof(double), out, stream));
  HIPCHK(hipMemcpyAsync(mean, dM, (size_t)P * sizeof(double), out, stream));
  sync();
}

void bobe_gp::hmc_run(int64_t P, double* state, double* adapt, const double* inv_mass, uint64_t seed, int64_t it0, int niter,
                      int do_adapt, double y_std, double y_mean, double temp, int hist_from, double* hist, int thin,
                      double* keep, double* dbg) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (P <= 0 || niter < 1 || it0 < 0 || !(temp > 0.0) || thin < 1 || hist_from < 0 || hist_from > niter)
    throw Err(BOBE_ERR_ARG, "bad argument");
  use();
  const ChainStage st(in_stage, P, d, (size_t)d, niter, hist_from, hist != nullptr, thin, keep != nullptr, 0,
                      dbg ? (size_t)P * (d + 3) : 0);
  st.copy_in(stream, state, adapt, inv_mass);
  // training points of a chain's workgroup: registers first, then LDS (chain_lds_groups), the rest streamed
  with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) {
    const int lg = chain_lds_groups(N, d, ChainRows<DC>::HMC);
    hipLaunchKernelGGL((k_hmc_run<KE, DC>), dim3((unsigned)P), dim3(256), (size_t)lg * 256 * (d + 1) * sizeof(double),
                       stream, (const double*)XsT.d(), Np, N, (const double*)alpha.d(), hyp, P, st.dS, st.dA,
                       (const double*)st.dI, (unsigned long long)seed, it0, niter, do_adapt, y_std, y_mean, temp, hist_from,
                       st.dH, thin, st.dK, st.dD, gate, lg);
  });
  LAUNCH_CHECK();
  st.copy_out(stream, state, adapt, hist, keep, nullptr, dbg);
  sync();
}

// Host side of k_nuts_run: checks the inverse metric (symmetric, positive definite, its inverse too) and passes it with
// the lower Cholesky factor C of its inverse, C C^T = Sigma^-1, from which the kernel draws momenta p = C z.
void bobe_gp::nuts_run(int64_t P, double* state, double* adapt, const double* inv_metric, int max_depth, uint64_t seed,
                       int64_t it0, int niter, int do_adapt, double y_std, double y_mean, double temp, int hist_from,
                       double* hist, int thin, double* keep, double* stats, double* dbg) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (P <= 0 || niter < 1 || it0 < 0 || !(temp > 0.0) || thin < 1 || hist_from < 0 || hist_from > niter)
    throw Err(BOBE_ERR_ARG, "bad argument");
  if (max_depth < 1 || max_depth > NUTS_MAX_DEPTH) throw Err(BOBE_ERR_ARG, "max_tree_depth must be in [1, 10]");
  const int dd = d;
  std::vector<double> met(2 * (size_t)dd * dd, 0.0), Ls((size_t)dd * dd, 0.0), Li((size_t)dd * dd, 0.0);
  for (int i = 0; i < dd; ++i)
    for (int j = 0; j < dd; ++j) {
      const double a = inv_metric[i * dd + j], b = inv_metric[j * dd + i];
      if (!std::isfinite(a) || std::fabs(a - b) > 1e-12 * (std::fabs(a) + std::fabs(b)))
        throw Err(BOBE_ERR_ARG, "inv_metric is not symmetric");
      met[(size_t)i * dd + j] = a;
    }
  // Cholesky factorisation (lower, in place); false when a pivot is not positive
  auto chol = [dd](std::vector<double>& A) {
    for (int j = 0; j < dd; ++j) {
      double s = A[(size_t)j * dd + j];
      for (int k = 0; k < j; ++k) s -= A[(size_t)j * dd + k] * A[(size_t)j * dd + k];
      if (!(s > 0.0) || !std::isfinite(s)) return false;
      const double r = std::sqrt(s);
      A[(size_t)j * dd + j] = r;
      for (int i = j + 1; i < dd; ++i) {
        double t = A[(size_t)i * dd + j];
        for (int k = 0; k < j; ++k) t -= A[(size_t)i * dd + k] * A[(size_t)j * dd + k];
        A[(size_t)i * dd + j] = t / r;
      }
      for (int i = 0; i < j; ++i) A[(size_t)i * dd + j] = 0.0;
    }
    return true;
  };
  for (int i = 0; i < dd * dd; ++i) Ls[i] = met[i];
  if (!chol(Ls)) throw Err(BOBE_ERR_ARG, "inv_metric is not positive definite");
  // M = Sigma^-1 = Ls^-T Ls^-1: Li = Ls^-1 by forward substitution, then M = Li^T Li, then C = chol(M)
  for (int c = 0; c < dd; ++c)
    for (int i = c; i < dd; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s -= Ls[(size_t)i * dd + k] * Li[(size_t)k * dd + c];
      Li[(size_t)i * dd + c] = s / Ls[(size_t)i * dd + i];
    }
  double* Cm = met.data() + (size_t)dd * dd;
  for (int i = 0; i < dd; ++i)
    for (int j = 0; j < dd; ++j) {
      double s = 0.0;
      for (int k = (i > j ? i : j); k < dd; ++k) s += Li[(size_t)k * dd + i] * Li[(size_t)k * dd + j];
      Cm[(size_t)i * dd + j] = s;
    }
  std::vector<double> Cv(Cm, Cm + (size_t)dd * dd);
  if (!chol(Cv)) throw Err(BOBE_ERR_ARG, "the inverse of inv_metric is not positive definite");
  std::copy(Cv.begin(), Cv.end(), Cm);
  use();
  // (the metric, Sigma then C, goes where hmc_run stages inv_mass)
  const ChainStage st(in_stage, P, d, met.size(), niter, hist_from, hist != nullptr, thin, keep != nullptr,
                      stats ? (size_t)niter * P * 4 : 0, dbg ? (size_t)P * d : 0);
  st.copy_in(stream, state, adapt, met.data());
  with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) {
    const int lg = chain_lds_groups(N, d, ChainRows<DC>::NUTS, NUTS_LDS_BYTES);
    hipLaunchKernelGGL((k_nuts_run<KE, DC>), dim3((unsigned)P), dim3(256), (size_t)lg * 256 * (d + 1) * sizeof(double),
                       stream, (const double*)XsT.d(), Np, N, (const double*)alpha.d(), hyp, P, st.dS, st.dA,
                       (const double*)st.dI, max_depth, (unsigned long long)seed, it0, niter, do_adapt, y_std, y_mean, temp,
                       hist_from, st.dH, thin, st.dK, st.dT, st.dD, gate, lg);
  });
  LAUNCH_CHECK();
  st.copy_out(stream, state, adapt, hist, keep, stats, dbg);
  sync();
}

void bobe_gp::rwalk(int64_t P, double* Xw, double* logl, const double* step, double lstar, int walks, uint64_t seed,
                    double y_std, double y_mean, int* nacc, int* nin, double* dbg) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  if (P <= 0 || walks < 1) throw Err(BOBE_ERR_ARG, "bad argument");
  use();
  const size_t pd = (size_t)P * d;
  // staging: X | logl | step | dbg (doubles), then nacc | nin (ints)
  in_stage.ensure((2 * pd + (size_t)P + (size_t)d * d) * sizeof(double) + 2 * (size_t)P * sizeof(int));
  double* dX = in_stage.d();
  double* dL = dX + pd;
  double* dS = dL + P;
  double* dD = dS + (size_t)d * d;
  int* dA = reinterpret_cast<int*>(dD + pd);
  int* dN = dA + P;
  HIPCHK(hipMemcpyAsync(dX, Xw, pd * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dL, logl, (size_t)P * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(dS, step, (size_t)d * d * sizeof(double), hipMemcpyHostToDevice, stream));
  with_kern_dcap(hyp.kern, d, [&](auto KE, auto DC) {
    const int lg = chain_lds_groups(N, d, ChainRows<DC>::WALK);
    hipLaunchKernelGGL((k_rwalk<KE, DC>), dim3((unsigned)P), dim3(256), (size_t)lg * 256 * (d + 1) * sizeof(double),
                       stream, (const double*)XsT.d(), Np, N, (const double*)alpha.d(), hyp, dX, dL, (const double*)dS,
                       lstar, walks, (unsigned long long)seed, y_std, y_mean, dA, dN, dbg ? dD : nullptr, gate, lg);
  });
  LAUNCH_CHECK();
  HIPCHK(hipMemcpyAsync(Xw, dX, pd * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(logl, dL, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(nacc, dA, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(nin, dN, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, stream));
  if (dbg) HIPCHK(hipMemcpyAsync(dbg, dD, pd * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
}

void bobe_gp::kernel_eval(const double* A, int64_t nA, const double* B, int64_t nB, const double* ls, double kvar,
                          double noise, int include_noise, double* out, bool sqdist) {
  if (nA < 1 || nB < 1) throw Err(BOBE_ERR_ARG, "empty input");
  if (include_noise && nA != nB) throw Err(BOBE_ERR_ARG, "include_noise needs a square kernel matrix (gp.py:153)");
  use();
  Hyper hk = hyp;
  if (ls) {
    for (int j = 0; j < d; ++j) hk.ls[j] = ls[j];
    hk.kvar = kvar;
    hk.noise = noise;
  }
  if (sqdist) {                                  // dist_sq: unscaled coordinates, kernel id 2 = the distance itself
    for (int j = 0; j < d; ++j) hk.ls[j] = 1.0;
    hk.kern = 2;
  }
  const int64_t pa = round_up(nA, TILE), pb = round_up(nB, TILE);
  const double* a_in = fetch(A, (size_t)nA * d, in_stage);
  const double* b_in = fetch(B, (size_t)nB * d, z_stage);
  kin_a.ensure((size_t)d * pa * sizeof(double));
  kin_b.ensure((size_t)d * pb * sizeof(double));
  kout.ensure((size_t)pa * pb * sizeof(double));
  scale(a_in, nA, pa, hk, kin_a.d(), pa);
  scale(b_in, nB, pb, hk, kin_b.d(), pb);
  kernel_matrix_cross(kin_a.d(), pa, nA, pa, kin_b.d(), pb, nB, pb, hk, kout.d(), pb);
  const bool dev = is_device_ptr(out);
  HIPCHK(hipMemcpy2DAsync(out, (size_t)nB * sizeof(double), kout.p, (size_t)pb * sizeof(double),
                          (size_t)nB * sizeof(double), (size_t)nA, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          stream));
  sync();
  if (include_noise) {
    // noise * eye(n) (gp.py:153): added on the host side of the copy for host outputs, by a tiny kernel otherwise
    if (!dev) {
      for (int64_t i = 0; i < nA; ++i) out[i * nB + i] += hk.noise;
    } else {
      std::vector<double> dg((size_t)nA);
      HIPCHK(hipMemcpy2D(dg.data(), sizeof(double), out, (size_t)(nB + 1) * sizeof(double), sizeof(double), (size_t)nA,
                         hipMemcpyDeviceToHost));
      for (auto& v : dg) v += hk.noise;
      HIPCHK(hipMemcpy2D(out, (size_t)(nB + 1) * sizeof(double), dg.data(), sizeof(double), sizeof(double), (size_t)nA,
                         hipMemcpyHostToDevice));
    }
  }
}

// GP.copy (gp.py:740-750) without leaving the device: training data, hyper-parameters and factorised state by
// device-to-device copies.  The classifier gate is not part of a GP's state_dict and is not cloned.
void bobe_gp::clone_from(bobe_gp& src) {
  if (this == &src) return;
  if (d != src.d || kern != src.kern || device != src.device)
    throw Err(BOBE_ERR_ARG, "clone needs handles of the same kernel, dimension and device");
  if (!src.have_data) throw Err(BOBE_ERR_STATE, "source holds no data");
  src.use();
  src.sync();
  sync();
  ++data_gen;
  forget_evals();
  factor_source = -1;
  N = src.N;
  hyp = src.hyp;
  pivot_ulp = src.pivot_ulp;
  refine_kappa = src.refine_kappa;
  solve_block = src.solve_block;
  solve_panel = src.solve_panel;
  solve_chunk = src.solve_chunk;
  refine_v = src.factored && src.refine_v;      // (A is copied with its diagonal blocks as the source left them)
  if (Np != src.Np) {
    Np = src.Np;
    nb = src.nb;
    alloc_for_n();
  }
  const size_t mat = (size_t)src.Np * src.Np * sizeof(double), vec = (size_t)src.Np * sizeof(double);
  X.ensure((size_t)(src.Np + TILE) * src.d * sizeof(double));
  HIPCHK(hipMemcpyAsync(X.p, src.X.p, (size_t)src.N * src.d * sizeof(double), hipMemcpyDeviceToDevice, stream));
  HIPCHK(hipMemcpyAsync(y.p, src.y.p, vec, hipMemcpyDeviceToDevice, stream));
  if (src.factored) {
    HIPCHK(hipMemcpyAsync(XsT.p, src.XsT.p, (size_t)src.d * vec, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(A.p, src.A.p, mat, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(Linv.p, src.Linv.p, mat, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(alpha.p, src.alpha.p, vec, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemcpyAsync(w.p, src.w.p, vec, hipMemcpyDeviceToDevice, stream));
  }
  sync();
  have_data = true;
  factored = src.factored;
  forget_z();
  not_pd = src.not_pd;
}

// everything the handle owns on the device and in pinned memory (bobe_gp_destroy)
void bobe_gp::release_all() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  DBuf* bufs[] = {&X, &y, &XsT, &A, &Linv, &Tmp, &alpha, &w, &part, &gpart, &res, &info, &probs, &diag, &in_stage, &z_stage, &CsT, &ZsT, &kXC, &kXZ, &VZ, &WZ, &basez, &sc, &qpart, &pv,
                  &ps, &o_mean, &o_var, &o_wipv, &o_wipstd, &o_misc, &kin_a, &kin_b, &kout, &wg_ws, &gate_sv, &gate_dual, &gate_ell, &ell_ws, &ell_perm,
                  &vxc, &vxc2, &loo_ws, &wg_out, &zw.zt, &zw.zpart, &zw.lstage};
  for (DBuf* b : bufs) b->release();
  for (auto& pr : prof_events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  if (h_res) (void)hipHostFree(h_res);
  if (h_in) (void)hipHostFree(h_in);
  h_in = nullptr;
  for (hipStream_t st : slot_streams) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
  own.release();
  batch.release();
  for (EvalWs* sl : slots) {
    sl->release();
    delete sl;
  }
  slots.clear();
  for (auto& kv : chol_plans) {
    kv.second.d_jobs.release();
    kv.second.d_colk0.release();
  }
  if (ev_batch) (void)hipEventDestroy(ev_batch);
  if (side_stream) {
    (void)hipStreamSynchronize(side_stream);
    (void)hipStreamDestroy(side_stream);
  }
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (ev_join) (void)hipEventDestroy(ev_join);
  if (own_stream && stream) (void)hipStreamDestroy(stream);
}
