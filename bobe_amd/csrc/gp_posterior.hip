// libbobe_gp.so, posterior unit: the joint posterior of the surrogate at C query points - its covariance (bobe_gp_predict_cov)
// and correlated draws from it (bobe_gp_posterior_sample).  Kernels: posterior_kernels.hpp.
// Every buffer of these calls (V, Sigma, its factor, the normals) belongs to the call and is freed before it returns; the
// factorisation of Sigma runs on a data-less child handle that shares the device and the stream, so the handle's own factor,
// workspace and adoption records are not touched.
#include "gp_handle.hpp"

#include "posterior_kernels.hpp"

#include <memory>

using namespace bobe;

namespace bobe {
void configure_posterior_kernels() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  allow_big_lds(k_sigma_tiles<0>, GEMM_SMEM_BYTES);
  allow_big_lds(k_sigma_tiles<1>, GEMM_SMEM_BYTES);
  allow_big_lds(k_trmm_draws, GEMM_SMEM_BYTES);
}
}  // namespace bobe

namespace {

constexpr int64_t MAX_QUERIES = 16384;             // bobe_gp.h: C <= 16384
constexpr size_t V_CHUNK_BYTES = size_t(1) << 30;  // V and K(X, chunk) are formed for at most this many bytes of columns each

// the scaled query coordinates QsT (d x Cp) and, optionally, the posterior mean
struct Queries {
  int64_t C = 0, Cp = 0;
  CallBuf xin, qst;
};

void load_queries(bobe_gp& g, const double* Xq, int64_t C, Queries& q) {
  q.C = C;
  q.Cp = round_up(C, TILE);
  const double* xq = Xq;
  if (!is_device_ptr(Xq)) {
    q.xin.ensure((size_t)C * g.d * sizeof(double));
    HIPCHK(hipMemcpyAsync(q.xin.p, Xq, (size_t)C * g.d * sizeof(double), hipMemcpyHostToDevice, g.stream));
    xq = q.xin.d();
  }
  q.qst.ensure((size_t)g.d * q.Cp * sizeof(double));
  g.scale(xq, C, q.Cp, g.hyp, q.qst.d(), q.Cp);
}

// Sigma (C x C, both triangles, row-major with leading dimension ldo) into `out` (device), and - mean != nullptr - the
// posterior mean into mean[0, C).  V = L^-1 K(X, Q) is formed exactly as bobe_gp_predict forms it (bobe_gp::solve_v: the
// product with the inverse factor, or the blocked substitution while the refine switch is on), in column chunks of at most
// V_CHUNK_BYTES: the tiles of chunk pair (I, J < I) need V_I and V_J at once, so V_J is formed again for every I (nothing
// is repeated when one chunk holds all C columns - N = 4096 up to 32768 queries).
void assemble_sigma(bobe_gp& g, const Queries& q, double* out, int64_t ldo, double* mean) {
  const int64_t C = q.C, Cp = q.Cp, Np = g.Np;
  const int64_t CH = std::min<int64_t>(Cp, std::max<int64_t>(TILE, (int64_t)(V_CHUNK_BYTES / sizeof(double) / Np) / TILE * TILE));
  const bool one = CH >= Cp;
  CallBuf kxc, vi, vj, part, qpart;
  kxc.ensure((size_t)Np * CH * sizeof(double));
  vi.ensure((size_t)Np * CH * sizeof(double));
  if (!one) vj.ensure((size_t)Np * CH * sizeof(double));
  part.ensure((size_t)g.nb * CH * sizeof(double));
  qpart.ensure((size_t)g.nb * CH * sizeof(double));
  auto form_v = [&](int64_t c0, double* V, bool with_mean) {
    const int64_t nc = std::min(CH, C - c0), ncp = round_up(nc, TILE);
    g.kernel_matrix_cross(g.XsT.d(), Np, g.N, Np, q.qst.d() + c0, Cp, nc, ncp, g.hyp, kxc.d(), CH,
                          with_mean ? (const double*)g.alpha.d() : nullptr, with_mean ? part.d() : nullptr, CH);
    if (with_mean)
      hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, g.stream, (const double*)part.d(),
                         CH, g.nb, 0, nc, mean + c0, (int64_t)0, (int64_t)0);
    g.solve_v(kxc.d(), CH, ncp, V, CH, qpart.d(), CH);
    LAUNCH_CHECK();
  };
  auto tiles = [&](const double* VI, const double* VJ, int64_t i0, int64_t j0, int ntI, int ntJ, int diag) {
    const int n = diag ? ntI * (ntI + 1) / 2 : ntI * ntJ;
    if (g.kern == BOBE_KERNEL_RBF)
      hipLaunchKernelGGL(k_sigma_tiles<0>, dim3((unsigned)n), dim3(256), GEMM_SMEM_BYTES, g.stream, VI, VJ, CH, Np,
                         (const double*)q.qst.d(), Cp, i0, j0, ntJ, diag, C, g.hyp, out, ldo);
    else
      hipLaunchKernelGGL(k_sigma_tiles<1>, dim3((unsigned)n), dim3(256), GEMM_SMEM_BYTES, g.stream, VI, VJ, CH, Np,
                         (const double*)q.qst.d(), Cp, i0, j0, ntJ, diag, C, g.hyp, out, ldo);
    LAUNCH_CHECK();
  };
  for (int64_t i0 = 0; i0 < C; i0 += CH) {
    const int ntI = (int)(round_up(std::min(CH, C - i0), TILE) / TILE);
    form_v(i0, vi.d(), mean != nullptr);
    g.prof_begin(BOBE_PROF_CROSSVV);
    tiles(vi.d(), vi.d(), i0, i0, ntI, ntI, 1);
    g.prof_end(BOBE_PROF_CROSSVV);
    for (int64_t j0 = 0; j0 < i0; j0 += CH) {
      form_v(j0, vj.d(), false);
      g.prof_begin(BOBE_PROF_CROSSVV);
      tiles(vi.d(), vj.d(), i0, j0, ntI, (int)(CH / TILE), 0);
      g.prof_end(BOBE_PROF_CROSSVV);
    }
  }
}

// true when some diagonal entry of Sigma is NaN (a NaN factor or NaN hyper-parameters); dg receives the diagonal
bool sigma_diag(bobe_gp& g, const double* sig, int64_t lds, int64_t C, std::vector<double>& dg) {
  CallBuf d;
  d.ensure((size_t)C * sizeof(double));
  hipLaunchKernelGGL(k_take_diag, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, g.stream, sig, lds, C, d.d());
  LAUNCH_CHECK();
  dg.resize((size_t)C);
  HIPCHK(hipMemcpyAsync(dg.data(), d.p, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, g.stream));
  g.sync();
  for (double v : dg)
    if (v != v) return true;
  return false;
}

struct ChildDeleter {
  void operator()(bobe_gp* c) const {
    c->release_all();
    delete c;
  }
};

}  // namespace

int bobe_gp::predict_cov(const double* Xq, int64_t C, double* cov) {
  if (C < 1 || C > MAX_QUERIES) throw Err(BOBE_ERR_ARG, "C must be in [1, 16384]");
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  use();
  const size_t n2 = (size_t)C * C;
  const bool dev_out = is_device_ptr(cov);
  CallBuf stage;
  double* out = cov;
  if (!dev_out) {
    stage.ensure(n2 * sizeof(double));
    out = stage.d();
  }
  int st = BOBE_OK;
  if (not_pd) {
    st = BOBE_NOT_PD;
  } else {
    Queries q;
    load_queries(*this, Xq, C, q);
    assemble_sigma(*this, q, out, C, nullptr);
    std::vector<double> dg;
    if (sigma_diag(*this, out, C, C, dg)) st = BOBE_NOT_PD;
  }
  if (st == BOBE_NOT_PD) {
    fill(out, (int64_t)n2, std::nan(""));
    LAUNCH_CHECK();
    g_err = "the posterior covariance is NaN (the factor is not positive definite or NaN)";
  }
  if (!dev_out) HIPCHK(hipMemcpyAsync(cov, out, n2 * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
  return st;
}

int bobe_gp::posterior_sample(const double* Xq, int64_t C, int64_t S, uint64_t seed, const double* z, int centered,
                              double* draws, double* jitter_out) {
  if (C < 1 || C > MAX_QUERIES) throw Err(BOBE_ERR_ARG, "C must be in [1, 16384]");
  if (S < 1) throw Err(BOBE_ERR_ARG, "S must be positive");
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  use();
  const int64_t Cp = round_up(C, TILE), Sp = round_up(S, TILE);
  const size_t nd = (size_t)S * C;
  const bool dev_out = is_device_ptr(draws);
  CallBuf stage, sig, mean;
  double* out = draws;
  if (!dev_out) {
    stage.ensure(nd * sizeof(double));
    out = stage.d();
  }
  double jitter = std::nan("");
  int st = not_pd ? BOBE_NOT_PD : BOBE_OK;
  std::unique_ptr<bobe_gp, ChildDeleter> child;
  if (st == BOBE_OK) {
    sig.ensure((size_t)C * C * sizeof(double));
    if (!centered) mean.ensure((size_t)C * sizeof(double));
    {
      Queries q;
      load_queries(*this, Xq, C, q);
      assemble_sigma(*this, q, sig.d(), C, centered ? nullptr : mean.d());
    }
    std::vector<double> dg;
    if (sigma_diag(*this, sig.d(), C, C, dg)) st = BOBE_NOT_PD;
    double dmean = 0.0;
    for (double v : dg) dmean += v;
    dmean /= (double)C;
    // the factor of Sigma + tau mean(diag Sigma) I on a data-less child handle (bobe_gp_mll_from_k's factorisation and test)
    if (st == BOBE_OK) {
      child.reset(new bobe_gp());
      bobe_gp& c = *child;
      c.device = device;
      c.kern = kern;
      c.d = d;
      c.hyp = hyp;
      c.stream = stream;
      c.own_stream = false;
      c.num_cus = num_cus;
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c.h_res), 128 * sizeof(double), hipHostMallocDefault));
      c.N = C;
      c.Np = Cp;
      c.nb = (int)(Cp / TILE);
      c.A.ensure((size_t)Cp * Cp * sizeof(double));
      c.Linv.ensure((size_t)Cp * Cp * sizeof(double));
      c.diag.ensure((size_t)c.nb * TILE * TILE * sizeof(double));
      c.res.ensure(128 * sizeof(double));
      c.info.ensure(sizeof(int));
      c.build_plans();
      static const double taus[] = {0.0, 1e-12, 1e-10, 1e-8, 1e-6};
      st = BOBE_NOT_PD;
      for (double tau : taus) {
        const double jit = tau * dmean;
        hipLaunchKernelGGL(k_sigma_load_jitter, dim3((unsigned)((Cp + 255) / 256), (unsigned)Cp), dim3(256), 0, stream,
                           (const double*)sig.d(), C, C, jit, c.A.d(), Cp, Cp);
        HIPCHK(hipMemsetAsync(c.info.p, 0x7f, sizeof(int), stream));
        prof_begin(BOBE_PROF_POTF2);
        c.potrf(c.state_bufs());
        prof_end(BOBE_PROF_POTF2);
        hipLaunchKernelGGL(k_mll_terms, dim3(1), dim3(256), 0, stream, (const double*)nullptr, (const double*)c.A.d(), Cp, Cp,
                           c.res.d(), (int64_t)0, (int64_t)0, (int64_t)0, (const int*)c.info.p);
        LAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(c.h_res, c.res.p, 102 * sizeof(double), hipMemcpyDeviceToHost, stream));
        sync();
        int inf;
        std::memcpy(&inf, c.h_res + 100, sizeof(int));
        if (inf == 0x7f7f7f7f && c.h_res[101] > 0.0) {
          st = BOBE_OK;
          jitter = jit;
          break;
        }
        char msg[128];
        std::snprintf(msg, sizeof msg, "the posterior covariance does not factorise with a jitter of %g x mean(diag)", tau);
        g_err = msg;
      }
    }
    sig.release();
  }
  if (st == BOBE_OK) {
    bobe_gp& c = *child;
    hipLaunchKernelGGL(k_zero_diag_upper, dim3((unsigned)c.nb), dim3(256), 0, stream, c.A.d(), Cp);
    c.Linv.release();
    CallBuf zt;
    zt.ensure((size_t)Cp * Sp * sizeof(double));
    const double* zin = nullptr;
    CallBuf zstage;
    if (z) {
      zin = z;
      if (!is_device_ptr(z)) {
        zstage.ensure(nd * sizeof(double));
        HIPCHK(hipMemcpyAsync(zstage.p, z, nd * sizeof(double), hipMemcpyHostToDevice, stream));
        zin = zstage.d();
      }
    }
    hipLaunchKernelGGL(k_draw_normals, dim3((unsigned)((Sp + 255) / 256), (unsigned)Cp), dim3(256), 0, stream, zt.d(), Sp, S,
                       C, (unsigned long long)seed, zin);
    prof_begin(BOBE_PROF_TRIMUL);
    hipLaunchKernelGGL(k_trmm_draws, dim3((unsigned)(Sp / TILE), (unsigned)c.nb), dim3(256), GEMM_SMEM_BYTES, stream,
                       (const double*)c.A.d(), Cp, c.nb, (const double*)zt.d(), Sp,
                       centered ? (const double*)nullptr : (const double*)mean.d(), S, C, out, C);
    prof_end(BOBE_PROF_TRIMUL);
    LAUNCH_CHECK();
    sync();
  } else {
    fill(out, (int64_t)nd, std::nan(""));
    LAUNCH_CHECK();
    if (not_pd) g_err = "the handle's factor is not positive definite";
  }
  if (!dev_out) HIPCHK(hipMemcpyAsync(draws, out, nd * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
  if (jitter_out) *jitter_out = jitter;
  return st;
}
