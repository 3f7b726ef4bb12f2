// libbobe_gp.so, paths unit: pathwise posterior draws of the LATENT surrogate f (bobe_gp_paths_*).  Matheron's rule with the
// prior drawn through F random Fourier features:
//     f_s(x) = phi(x)^T w_s + k(x, X) v_s,     v_s = K^-1 (y - Phi(X) w_s - eps_s) = alpha + V_c[:, s].
// A path set is a SNAPSHOT of the handle's factorised state: it owns the scaled training coordinates, alpha, the
// hyper-parameters, the frequencies / phases / weights and V_c = -K^-1 (Phi(X) W^T + E^T); the parent's factor is read while
// the set is created and never again.  The parent's stream, chunk and launch helpers are used by every call, so the set is
// destroyed before its parent.  paths_hmc_run (whole HMC chains on a path, k_paths_hmc_run) also reads the parent's classifier
// gate at call time: the gate is not part of the snapshot.  Kernels: paths_kernels.hpp.  Every call-scoped buffer is a CallBuf.  paths_grad (value and
// input gradient of one path per point, k_paths_grad) adds one lazily built member, the transposed coefficients VcT.
#include "gp_handle.hpp"

#include "paths_kernels.hpp"

#include <memory>

using namespace bobe;

struct bobe_paths {
  bobe_gp* g = nullptr;
  int64_t S = 0, F = 0, Fp = 0, Sp = 0, N = 0, Np = 0;
  int nb = 0, d = 0, T = TILE;
  Hyper hyp;
  // XsT [d x Np], alpha [Np]: copies of the parent's; U [F x d], B [F], W [S x F], E [S x N]: the set's random arrays, dense;
  // VW [(Np + Fp) x Sp]: V_c over W^T, the B operand of the evaluation product
  DBuf XsT, alpha, U, B, W, E, VW;
  // VcT [S x Np]: V_c transposed, a path's coefficients as a contiguous row; built by the first paths_grad call
  DBuf VcT;
  void release() {
    for (DBuf* b : {&XsT, &alpha, &U, &B, &W, &E, &VW, &VcT}) b->release();
  }
};

namespace bobe {
void configure_paths_kernels() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  allow_big_lds(k_paths_rhs, GEMM_SMEM_BYTES);
  allow_big_lds(k_paths_tiles<128, false>, GEMM_SMEM_BYTES);
  allow_big_lds(k_paths_tiles<128, true>, GEMM_SMEM_BYTES);
  allow_big_lds(k_paths_tiles<64, false>, GEMM64_SMEM_BYTES);
  allow_big_lds(k_paths_tiles<64, true>, GEMM64_SMEM_BYTES);
  allow_big_lds(k_paths_tiles<32, false>, GEMM32_SMEM_BYTES);
  allow_big_lds(k_paths_tiles<32, true>, GEMM32_SMEM_BYTES);
  // (the chain kernel keeps training rows in up to 148 KB of LDS, like k_hmc_run)
  for_each_kern_dcap([](auto KE, auto DC) { allow_big_lds((k_paths_hmc_run<KE, DC>), CHAIN_LDS_BYTES); });
}
}  // namespace bobe

namespace {

constexpr int64_t MAX_FEATURES = 65536;             // bobe_gp.h: 1 <= F <= 65536
constexpr size_t OP_CHUNK_BYTES = size_t(1) << 30;  // the operand [K(X, chunk); Phi(chunk)] is formed for at most this many bytes

struct PathsDeleter {
  void operator()(bobe_paths* p) const {
    p->release();
    delete p;
  }
};

// dst (device) <- src (host or device), n doubles, on the stream
void copy_in(bobe_gp& g, double* dst, const double* src, size_t n) {
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        g.stream));
}
void copy_out(bobe_gp& g, double* dst, const double* src, size_t n) {
  if (!dst) return;
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                        g.stream));
}

// PhiT [Fp x ldo] of n points with scaled coordinates xst (leading dimension ldx), padded to npad columns
void features(bobe_paths& p, const double* xst, int64_t ldx, int64_t n, int64_t npad, double* phiT, int64_t ldo) {
  const double amp = std::sqrt(2.0 * p.hyp.kvar / (double)p.F);
  const dim3 grid((unsigned)(npad / TILE), (unsigned)((p.Fp + 63) / 64));
  with_dcap(p.d, [&](auto DC) {
    hipLaunchKernelGGL((k_paths_features<DC>), grid, dim3(256), 0, p.g->stream, xst, ldx, n, p.d, (const double*)p.U.d(),
                       (const double*)p.B.d(), p.F, p.Fp, amp, phiT, ldo);
  });
  LAUNCH_CHECK();
}

// the evaluation product of one chunk (k_paths_tiles) on the tile the set was given
template <bool ARGMAX, typename... Args>
void launch_tiles(bobe_paths& p, int64_t ncp, Args... args) {
  const int T = p.T;
  const dim3 grid((unsigned)(ncp / T), (unsigned)(round_up(p.S, T) / T));
  hipStream_t st = p.g->stream;
  if (T == 128)
    hipLaunchKernelGGL((k_paths_tiles<128, ARGMAX>), grid, dim3(256), GEMM_SMEM_BYTES, st, args...);
  else if (T == 64)
    hipLaunchKernelGGL((k_paths_tiles<64, ARGMAX>), grid, dim3(256), GEMM64_SMEM_BYTES, st, args...);
  else
    hipLaunchKernelGGL((k_paths_tiles<32, ARGMAX>), grid, dim3(256), GEMM32_SMEM_BYTES, st, args...);
  LAUNCH_CHECK();
}

// The chunks of an evaluation.  out (device, S x C; NULL: argmax mode): the values; else best / idx (device, S each) receive
// the running maximum of f + bias (bias: device S x C or NULL) and its index.
void run_chunks(bobe_paths& p, const double* Xq, int64_t C, bool centered, double* out, const double* bias, double* best,
                int64_t* idx) {
  bobe_gp& g = *p.g;
  const int64_t Np = p.Np, K = p.Np + p.Fp, Cp = round_up(C, TILE);
  CallBuf xin, qst, op, part, mean, pmax, pidx;
  const double* xq = Xq;
  if (!is_device_ptr(Xq)) {
    xin.ensure((size_t)C * p.d * sizeof(double));
    HIPCHK(hipMemcpyAsync(xin.p, Xq, (size_t)C * p.d * sizeof(double), hipMemcpyHostToDevice, g.stream));
    xq = xin.d();
  }
  qst.ensure((size_t)p.d * Cp * sizeof(double));
  g.scale(xq, C, Cp, p.hyp, qst.d(), Cp);
  const int64_t cap = std::max<int64_t>(TILE, (int64_t)(OP_CHUNK_BYTES / sizeof(double) / K) / TILE * TILE);
  const int64_t CH = std::min(Cp, std::min<int64_t>(g.chunk, cap));
  op.ensure((size_t)K * CH * sizeof(double));
  if (!centered) {
    part.ensure((size_t)p.nb * CH * sizeof(double));
    mean.ensure((size_t)CH * sizeof(double));
  }
  const int npt_max = (int)(CH / p.T);
  if (!out) {
    pmax.ensure((size_t)p.S * npt_max * sizeof(double));
    pidx.ensure((size_t)p.S * npt_max * sizeof(int));
    hipLaunchKernelGGL(k_paths_argmax_arm, dim3((unsigned)((p.S + 255) / 256)), dim3(256), 0, g.stream, best, idx, p.S);
    LAUNCH_CHECK();
  }
  const double* mn = centered ? nullptr : mean.d();
  for (int64_t c0 = 0; c0 < C; c0 += CH) {
    const int64_t nc = std::min(CH, C - c0), ncp = round_up(nc, TILE);
    // K(X, chunk) into rows [0, Np) of the operand (and, uncentred, the posterior mean K(X, chunk)^T alpha on the way, as
    // bobe_gp_predict forms it), Phi(chunk) into rows [Np, Np + Fp)
    g.prof_begin(BOBE_PROF_KXC);
    g.kernel_matrix_cross(p.XsT.d(), Np, p.N, Np, qst.d() + c0, Cp, nc, ncp, p.hyp, op.d(), CH,
                          centered ? nullptr : (const double*)p.alpha.d(), centered ? nullptr : part.d(), CH);
    if (!centered) {
      hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, g.stream, (const double*)part.d(),
                         CH, p.nb, 0, nc, mean.d(), (int64_t)0, (int64_t)0);
      LAUNCH_CHECK();
    }
    features(p, qst.d() + c0, Cp, nc, ncp, op.d() + Np * CH, CH);
    g.prof_end(BOBE_PROF_KXC);
    g.prof_begin(BOBE_PROF_CROSSVV);
    if (out) {
      launch_tiles<false>(p, ncp, (const double*)p.VW.d(), p.Sp, (const double*)op.d(), CH, K, mn, p.S, nc, out + c0, C,
                          (const double*)nullptr, (int64_t)0, (double*)nullptr, (int*)nullptr, 0);
    } else {
      const int npt = (int)(ncp / p.T);
      launch_tiles<true>(p, ncp, (const double*)p.VW.d(), p.Sp, (const double*)op.d(), CH, K, mn, p.S, nc, (double*)nullptr,
                         (int64_t)0, bias ? bias + c0 : (const double*)nullptr, C, pmax.d(), static_cast<int*>(pidx.p), npt);
      const dim3 mg((unsigned)((p.S + 255) / 256));
      if (p.T == 128)
        hipLaunchKernelGGL(k_paths_argmax_merge<128>, mg, dim3(256), 0, g.stream, (const double*)pmax.d(),
                           (const int*)pidx.p, npt, p.S, c0, best, idx);
      else if (p.T == 64)
        hipLaunchKernelGGL(k_paths_argmax_merge<64>, mg, dim3(256), 0, g.stream, (const double*)pmax.d(),
                           (const int*)pidx.p, npt, p.S, c0, best, idx);
      else
        hipLaunchKernelGGL(k_paths_argmax_merge<32>, mg, dim3(256), 0, g.stream, (const double*)pmax.d(),
                           (const int*)pidx.p, npt, p.S, c0, best, idx);
      LAUNCH_CHECK();
    }
    g.prof_end(BOBE_PROF_CROSSVV);
  }
  g.sync();     // (the call's buffers are freed on return)
}

// VcT, the transposed coefficients: built by the set's first paths_grad / paths_hmc_run call
void ensure_vct(bobe_paths& p) {
  if (p.VcT.p) return;
  p.VcT.ensure((size_t)p.S * p.Np * sizeof(double));
  hipLaunchKernelGGL(k_paths_transpose_vc, dim3((unsigned)p.S, (unsigned)((p.Np + 255) / 256)), dim3(256), 0, p.g->stream,
                     (const double*)p.VW.d(), p.Sp, p.Np, p.VcT.d(), p.Np);
  LAUNCH_CHECK();
}

}  // namespace

namespace bobe {

int paths_create(bobe_gp& g, int64_t S, int64_t F, uint64_t seed, const double* u, const double* phase, const double* w,
                 const double* eps, bobe_paths** out) {
  if (S < 1) throw Err(BOBE_ERR_ARG, "S must be positive");
  if (F < 1 || F > MAX_FEATURES) throw Err(BOBE_ERR_ARG, "F must be in [1, 65536]");
  if (!g.factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  g.use();
  if (g.not_pd) {
    g_err = "the handle's factor is not positive definite";
    return BOBE_NOT_PD;
  }
  std::unique_ptr<bobe_paths, PathsDeleter> hold(new bobe_paths());
  bobe_paths& p = *hold;
  p.g = &g;
  p.S = S;
  p.F = F;
  p.Fp = round_up(F, 32);           // (a multiple of every tile's K-step: 16 at T = 64 / 128, 32 at T = 32)
  p.Sp = round_up(S, TILE);
  p.N = g.N;
  p.Np = g.Np;
  p.nb = g.nb;
  p.d = g.d;
  p.hyp = g.hyp;
  p.T = S <= 32 ? 32 : (S <= 64 ? 64 : TILE);
  const int64_t N = p.N, Np = p.Np, Sp = p.Sp, Fp = p.Fp;
  const size_t vec = (size_t)Np * sizeof(double);
  p.XsT.ensure((size_t)p.d * vec);
  p.alpha.ensure(vec);
  p.U.ensure((size_t)F * p.d * sizeof(double));
  p.B.ensure((size_t)F * sizeof(double));
  p.W.ensure((size_t)S * F * sizeof(double));
  p.E.ensure((size_t)S * N * sizeof(double));
  p.VW.ensure((size_t)(Np + Fp) * Sp * sizeof(double));
  HIPCHK(hipMemcpyAsync(p.XsT.p, g.XsT.p, (size_t)p.d * vec, hipMemcpyDeviceToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(p.alpha.p, g.alpha.p, vec, hipMemcpyDeviceToDevice, g.stream));
  // the random arrays: the caller's, or drawn here (paths_kernels.hpp has the layout)
  if (u) copy_in(g, p.U.d(), u, (size_t)F * p.d);
  if (phase) copy_in(g, p.B.d(), phase, (size_t)F);
  if (!u || !phase)
    hipLaunchKernelGGL(k_paths_draw_freq, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, g.stream, u ? nullptr : p.U.d(),
                       phase ? nullptr : p.B.d(), F, p.d, p.hyp.kern == BOBE_KERNEL_RBF ? 0 : 1, (unsigned long long)seed);
  if (w) copy_in(g, p.W.d(), w, (size_t)S * F);
  else
    hipLaunchKernelGGL(k_paths_draw_normals, dim3((unsigned)S, (unsigned)((F + 255) / 256)), dim3(256), 0, g.stream, p.W.d(),
                       S, F, (unsigned long long)seed, 3, 1.0);
  if (eps) copy_in(g, p.E.d(), eps, (size_t)S * N);
  else
    hipLaunchKernelGGL(k_paths_draw_normals, dim3((unsigned)S, (unsigned)((N + 255) / 256)), dim3(256), 0, g.stream, p.E.d(),
                       S, N, (unsigned long long)seed, 4, std::sqrt(p.hyp.noise));
  LAUNCH_CHECK();
  double* WT = p.VW.d() + Np * Sp;
  hipLaunchKernelGGL(k_paths_pack_w, dim3((unsigned)Fp, (unsigned)((Sp + 255) / 256)), dim3(256), 0, g.stream,
                     (const double*)p.W.d(), S, F, WT, Sp);
  LAUNCH_CHECK();
  {
    // Rc = -(Phi(X) W^T + E^T), then V_c = K^-1 Rc for all S columns as the state's alpha is formed from y: the forward half
    // with the inverse factor (or the blocked substitution while the refine switch is on), the backward half with its transpose
    CallBuf phix, rc, wf;
    phix.ensure((size_t)Fp * Np * sizeof(double));
    rc.ensure((size_t)Np * Sp * sizeof(double));
    wf.ensure((size_t)Np * Sp * sizeof(double));
    features(p, p.XsT.d(), Np, N, Np, phix.d(), Np);
    hipLaunchKernelGGL(k_paths_rhs, dim3((unsigned)(Sp / TILE), (unsigned)(Np / TILE)), dim3(256), GEMM_SMEM_BYTES, g.stream,
                       (const double*)phix.d(), Np, (const double*)WT, Sp, Fp, (const double*)p.E.d(), N, S, rc.d(), Sp);
    LAUNCH_CHECK();
    g.solve_v(rc.d(), Sp, Sp, wf.d(), Sp, nullptr, 0);
    LAUNCH_CHECK();
    g.solve_wt(wf.d(), Sp, Sp, p.VW.d(), Sp);
    g.sync();
  }
  *out = hold.release();
  return BOBE_OK;
}

int paths_get(bobe_paths& p, double* u, double* phase, double* w, double* eps) {
  bobe_gp& g = *p.g;
  g.use();
  copy_out(g, u, p.U.d(), (size_t)p.F * p.d);
  copy_out(g, phase, p.B.d(), (size_t)p.F);
  copy_out(g, w, p.W.d(), (size_t)p.S * p.F);
  copy_out(g, eps, p.E.d(), (size_t)p.S * p.N);
  g.sync();
  return BOBE_OK;
}

int paths_eval(bobe_paths& p, const double* Xq, int64_t C, int centered, double* f) {
  if (C < 1) throw Err(BOBE_ERR_ARG, "C must be positive");
  bobe_gp& g = *p.g;
  g.use();
  const size_t n = (size_t)p.S * C;
  const bool dev_out = is_device_ptr(f);
  CallBuf stage;
  double* out = f;
  if (!dev_out) {
    stage.ensure(n * sizeof(double));
    out = stage.d();
  }
  run_chunks(p, Xq, C, centered != 0, out, nullptr, nullptr, nullptr);
  if (!dev_out) {
    HIPCHK(hipMemcpyAsync(f, out, n * sizeof(double), hipMemcpyDeviceToHost, g.stream));
    g.sync();
  }
  return BOBE_OK;
}

int paths_argmax(bobe_paths& p, const double* Xq, int64_t C, const double* bias, int64_t* idx, double* best) {
  if (C < 1) throw Err(BOBE_ERR_ARG, "C must be positive");
  bobe_gp& g = *p.g;
  g.use();
  const size_t n = (size_t)p.S * C;
  CallBuf bstage, res;
  const double* bd = bias;
  if (bias && !is_device_ptr(bias)) {
    bstage.ensure(n * sizeof(double));
    HIPCHK(hipMemcpyAsync(bstage.p, bias, n * sizeof(double), hipMemcpyHostToDevice, g.stream));
    bd = bstage.d();
  }
  res.ensure((size_t)2 * p.S * sizeof(double));           // best [S], then idx [S] (int64)
  double* d_best = res.d();
  int64_t* d_idx = reinterpret_cast<int64_t*>(res.d() + p.S);
  run_chunks(p, Xq, C, false, nullptr, bd, d_best, d_idx);
  HIPCHK(hipMemcpyAsync(best, d_best, (size_t)p.S * sizeof(double),
                        is_device_ptr(best) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(idx, d_idx, (size_t)p.S * sizeof(int64_t),
                        is_device_ptr(idx) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g.stream));
  g.sync();
  return BOBE_OK;
}

int paths_grad(bobe_paths& p, const double* Xq, int64_t T, const int64_t* path_idx, int centered, double* f, double* df) {
  if (T < 1) throw Err(BOBE_ERR_ARG, "T must be positive");
  if (!f && !df) throw Err(BOBE_ERR_ARG, "f and df are both NULL");
  if (is_device_ptr(path_idx)) throw Err(BOBE_ERR_ARG, "path_idx must be host memory");
  for (int64_t t = 0; t < T; ++t)
    if (path_idx[t] < 0 || path_idx[t] >= p.S) throw Err(BOBE_ERR_ARG, "path_idx out of range");
  bobe_gp& g = *p.g;
  g.use();
  const int d = p.d;
  ensure_vct(p);
  CallBuf xin, idx, fout, dout;
  const double* xq = Xq;
  if (!is_device_ptr(Xq)) {
    xin.ensure((size_t)T * d * sizeof(double));
    HIPCHK(hipMemcpyAsync(xin.p, Xq, (size_t)T * d * sizeof(double), hipMemcpyHostToDevice, g.stream));
    xq = xin.d();
  }
  idx.ensure((size_t)T * sizeof(int64_t));
  HIPCHK(hipMemcpyAsync(idx.p, path_idx, (size_t)T * sizeof(int64_t), hipMemcpyHostToDevice, g.stream));
  double* fd = f;
  double* dd = df;
  if (f && !is_device_ptr(f)) {
    fout.ensure((size_t)T * sizeof(double));
    fd = fout.d();
  }
  if (df && !is_device_ptr(df)) {
    dout.ensure((size_t)T * d * sizeof(double));
    dd = dout.d();
  }
  const double amp = std::sqrt(2.0 * p.hyp.kvar / (double)p.F);
  with_kern_dcap(p.hyp.kern, d, [&](auto KE, auto DC) {
    hipLaunchKernelGGL((k_paths_grad<KE, DC>), dim3((unsigned)T), dim3(256), 0, g.stream, (const double*)p.XsT.d(), p.Np,
                       p.N, p.hyp, (const double*)p.alpha.d(), (const double*)p.VcT.d(), p.Np, (const double*)p.U.d(),
                       (const double*)p.B.d(), (const double*)p.W.d(), p.F, amp, xq, (const int64_t*)idx.p,
                       centered != 0 ? 1 : 0, fd, dd);
  });
  LAUNCH_CHECK();
  if (fd != f) HIPCHK(hipMemcpyAsync(f, fd, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  if (dd != df) HIPCHK(hipMemcpyAsync(df, dd, (size_t)T * d * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  g.sync();     // (the call's buffers are freed on return)
  return BOBE_OK;
}

// where a chain workgroup of k_paths_hmc_run keeps this set's training rows, and its features per thread
static void chain_layout(const bobe_paths& p, int* reg, int* lds, int* streamed, int* feat, int* lgroups) {
  int rmax = 0;
  with_dcap(p.d, [&](auto DC) { rmax = ChainRows<DC>::PATHS; });
  const int lg = chain_lds_groups(p.N, p.d, rmax);
  const int64_t r = std::min<int64_t>(p.N, 256 * (int64_t)rmax);
  const int64_t l = std::min<int64_t>(p.N - r, 256 * (int64_t)lg);
  *reg = (int)r;
  *lds = (int)l;
  *streamed = (int)(p.N - r - l);
  *feat = (int)((p.F + 255) / 256);
  *lgroups = lg;
}

int paths_chain_layout(bobe_paths& p, int* info4) {
  int lg = 0;
  chain_layout(p, info4, info4 + 1, info4 + 2, info4 + 3, &lg);
  return BOBE_OK;
}

int paths_hmc_run(bobe_paths& p, int64_t P, const int64_t* path_idx, double* state, double* adapt, const double* inv_mass,
                  uint64_t seed, int64_t it0, int niter, int do_adapt, double y_std, double y_mean, double temp,
                  int hist_from, double* hist, int thin, double* keep, double* dbg) {
  if (P <= 0 || P > INT_MAX || niter < 1 || it0 < 0 || !(temp > 0.0) || thin < 1 || hist_from < 0 || hist_from > niter)
    throw Err(BOBE_ERR_ARG, "bad argument");
  for (int64_t c = 0; c < P; ++c)
    if (path_idx[c] < 0 || path_idx[c] >= p.S) throw Err(BOBE_ERR_ARG, "path_idx out of range");
  bobe_gp& g = *p.g;
  g.use();
  ensure_vct(p);
  const int d = p.d;
  // the chain staging (inv_mass per chain), and the path indices
  CallBuf stage, idx;
  const ChainStage st(stage, P, d, (size_t)P * d, niter, hist_from, hist != nullptr, thin, keep != nullptr, 0,
                      dbg ? (size_t)P * (d + 3) : 0);
  idx.ensure((size_t)P * sizeof(int64_t));
  st.copy_in(g.stream, state, adapt, inv_mass);
  HIPCHK(hipMemcpyAsync(idx.p, path_idx, (size_t)P * sizeof(int64_t), hipMemcpyHostToDevice, g.stream));
  int reg, lds, streamed, feat, lg;
  chain_layout(p, &reg, &lds, &streamed, &feat, &lg);
  const double amp = std::sqrt(2.0 * p.hyp.kvar / (double)p.F);
  with_kern_dcap(p.hyp.kern, d, [&](auto KE, auto DC) {
    hipLaunchKernelGGL((k_paths_hmc_run<KE, DC>), dim3((unsigned)P), dim3(256), (size_t)lg * 256 * (d + 1) * sizeof(double),
                       g.stream, (const double*)p.XsT.d(), p.Np, p.N, p.hyp, (const double*)p.alpha.d(),
                       (const double*)p.VcT.d(), p.Np, (const double*)p.U.d(), (const double*)p.B.d(),
                       (const double*)p.W.d(), p.F, amp, (const int64_t*)idx.p, P, st.dS, st.dA, (const double*)st.dI,
                       (unsigned long long)seed, it0, niter, do_adapt, y_std, y_mean, temp, hist_from, st.dH, thin, st.dK,
                       st.dD, g.gate, lg);
  });
  LAUNCH_CHECK();
  st.copy_out(g.stream, state, adapt, hist, keep, nullptr, dbg);
  g.sync();     // (the call's buffers are freed on return)
  return BOBE_OK;
}

void paths_destroy(bobe_paths* p) {
  if (!p) return;
  if (p->g) {
    (void)hipSetDevice(p->g->device);
    if (p->g->stream) (void)hipStreamSynchronize(p->g->stream);
  }
  p->release();
  delete p;
}

}  // namespace bobe
