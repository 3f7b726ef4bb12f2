// What the chain kernels of two translation units share (gfx950): the classifier gate's per-point arithmetic, the homes of
// a chain workgroup's training rows (ChainTrain), the evaluation of the surrogate at the chain's point (chain_point,
// chain_reduce, chain_wsum) and the whole HMC transition with its contract (hmc_chain_run, on a Target).  Included by consumer_kernels.hpp (k_hmc_run, k_nuts_run, k_rwalk, k_gate) and by paths_kernels.hpp
// (k_paths_hmc_run).  Inline device functions, templates and constants only: no kernel lives here.
#pragma once
#include "kernels_common.hpp"

namespace bobe {

// ---- the classifier gate of GPwithClassifier (clf_gp.py:173-205) ---------------------------------------------------
// One 256-thread workgroup per point, ONE summation order everywhere (the batch kernel and the HMC / random-walk kernels
// share gate_partial / gate_combine): gate_partial's per-thread value, lanes by chain_wave_sum, then the four waves
// ((r0 + r1) + r2) + r3 in gate_combine.  A point near the boundary is therefore classified the same way by every entry
// point.  x: the point's d raw (unit-cube) coordinates, readable by every thread.
//   GATE_SVM        (clf.py:188-213, by DIRECT DIFFERENCES, as the reference computes it: diff = support_vectors - x;
//                   norm_sq = sum_j diff_j^2; decision = sum_i dual_i exp(-gamma norm_sq_i) + intercept): thread t adds
//                   the vectors t, t + 256, ... in ascending order; + intercept after the waves.
//   GATE_ELLIPSOID  (clf.py:377-412): thread t < d computes u_t = sum_{i >= t} L[i][t] (x_i - mu_i) in ascending i and
//                   contributes u_t^2 (md2 = |L^T diff|^2 = diff^T L L^T diff); logit = -alpha md2 + beta after the waves.
template <int DCAP>
__device__ __forceinline__ double gate_partial(const Gate& gt, const double* x, int d, int t) {
  double s = 0.0;
  if (gt.kind == GATE_ELLIPSOID) {
    if (t < d) {
      double u = 0.0;
      for (int i = t; i < d; ++i) u = fma(gt.Lt[i * d + t], x[i] - gt.mu[i], u);
      s = u * u;
    }
    return chain_wave_sum(s);
  }
  double xr[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xr[j] = (j < d) ? x[j] : 0.0;
  for (int i = t; i < gt.n_sv; i += 256) {
    double r2 = 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      if (j < d) {
        const double df = gt.svT[j * gt.ld + i] - xr[j];
        r2 += df * df;
      }
    }
    s += gt.dual[i] * exp(-gt.gamma * r2);
  }
  return chain_wave_sum(s);
}
// red[4]: the four waves' sums (written by lane 0 of each wave, followed by a barrier) -> the decision value (the SVM's
// decision function, the ellipsoid's logit)
__device__ __forceinline__ double gate_combine(const Gate& gt, const double* red) {
  const double r = ((red[0] + red[1]) + red[2]) + red[3];
  if (gt.kind == GATE_ELLIPSOID) return fma(-gt.alpha, r, gt.beta);
  return r + gt.intercept;
}
// the classifier's probability: svm_predict_proba (clf.py:210-213) or sigmoid(logit) (clf.py:134-136)
__device__ __forceinline__ double gate_proba(const Gate& gt, double decision) {
  if (gt.kind == GATE_ELLIPSOID) return 1.0 / (1.0 + exp(-decision));
  return (decision >= 0.0) ? 1.0 : 0.0;
}
// ... against the probability threshold (clf_gp.py:179): NaN decisions are infeasible (a NaN probability compares false)
__device__ __forceinline__ bool gate_feasible(const Gate& gt, double decision) {
  return gate_proba(gt, decision) >= gt.threshold;
}

// ---- the homes of a chain workgroup's training rows -------------------------------------------------------------------
// Training points a thread of a 256-thread chain workgroup keeps in registers for the whole launch (a launch is hundreds
// of leapfrog / random-walk steps over the same points): 256 x RESIDENT rows, the rest is streamed from L2 every step.
// (One wave per SIMD: the 512 unified registers of a lane hold them; chosen as the largest counts without scratch spills.)
template <int DCAP>
struct ChainRows {
  static constexpr int HMC = DCAP == 8 ? 14 : (DCAP == 16 ? 6 : 2);
  static constexpr int WALK = DCAP == 8 ? 16 : (DCAP == 16 ? 8 : 4);
  static constexpr int STREAM = DCAP == 32 ? 1 : 2;      // streamed rows in flight per thread
  static constexpr int NUTS = DCAP == 8 ? 10 : (DCAP == 16 ? 3 : 1);   // (k_nuts_run: its tree needs ~50 more registers)
  static constexpr int PATHS = DCAP == 8 ? 14 : (DCAP == 16 ? 6 : 1);  // (k_paths_hmc_run: its resource note)
};
// ... and as many more as the CU's LDS holds next to them: groups of 256 rows of d coordinates + alpha, [d + 1][rows]
// (a lane reads consecutive doubles: no bank conflicts).  Host side: the group count for n points and `resident` register rows.
constexpr int CHAIN_LDS_BYTES = 148 * 1024;                            // (of 160 KB: the kernels' static arrays stay below 10 KB)
inline int chain_lds_groups(int64_t n, int d, int resident, int bytes = CHAIN_LDS_BYTES) {
  const int64_t left = n - 256 * (int64_t)resident;
  if (left <= 0) return 0;
  const int64_t cap = bytes / (8 * (int64_t)(d + 1)) / 256;
  const int64_t want = (left + 255) / 256;
  return (int)(want < cap ? want : cap);
}

// Row i's coefficient, formed once where the row is loaded: alpha_i for the posterior mean, vc_i + alpha_i (one rounding) for
// a posterior path.
struct CoefMean {
  const double* alpha;
  __device__ __forceinline__ double operator()(int64_t i) const { return alpha[i]; }
};
struct CoefPath {
  const double* vc;
  const double* alpha;
  __device__ __forceinline__ double operator()(int64_t i) const { return vc[i] + alpha[i]; }
};

// The rows of thread t (t, t + 256, ...) in their homes.  The first RMAX are loaded ONCE per launch into registers - a
// launch is hundreds of leapfrog / random-walk steps, each of which would otherwise wait for the same global loads again -;
// rows past n carry the coefficient 0.  The next 256 lgroups rows live in LDS (every thread its own), and what fits neither
// is streamed from L2 on every visit.  The constructor fills registers and LDS; the caller's __syncthreads() follows it.
// One object per kernel, never copied (its arrays are the registers).
template <int DCAP, int RMAX, class Coef>
struct ChainTrain {
  static constexpr int NT = 256, UNR = ChainRows<DCAP>::STREAM;
  double cx[RMAX][DCAP], ca[RMAX];
  const double* const XsT;
  const double* const lrows;                   // [d + 1][256 lgroups] (chain_lds_groups)
  const Coef coef;
  const int64_t ldx, n;
  const int d, t, lgroups, lld, nrow;

  __device__ __forceinline__ ChainTrain(const double* XsT_, int64_t ldx_, int64_t n_, int d_, Coef coef_, double* lds,
                                        int lgroups_, int t_)
      : XsT(XsT_), lrows(lds), coef(coef_), ldx(ldx_), n(n_), d(d_), t(t_), lgroups(lgroups_), lld(NT * lgroups_),
        nrow((int)((n_ + NT - 1) / NT)) {
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int64_t i = t + NT * r;
      ca[r] = (i < n) ? coef(i) : 0.0;
#pragma unroll
      for (int j = 0; j < DCAP; ++j) cx[r][j] = (j < d && i < n) ? XsT[j * ldx + i] : 0.0;
    }
    for (int q = 0; q < lgroups; ++q) {
      const int64_t i = t + (int64_t)NT * (RMAX + q);
      for (int j = 0; j < d; ++j) lds[j * lld + q * NT + t] = (i < n) ? XsT[j * ldx + i] : 0.0;
      lds[d * lld + q * NT + t] = (i < n) ? coef(i) : 0.0;
    }
  }
  ChainTrain(const ChainTrain&) = delete;

  // point(xr, a) for every row of this thread, ascending rows throughout
  template <class Point>
  __device__ __forceinline__ void for_each(Point&& point) const {
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
      if (r < nrow) point(cx[r], ca[r]);                       // (uniform) in registers,
    for (int q = 0; q < lgroups; ++q) {                        // in LDS,
      double xr[DCAP];
#pragma unroll
      for (int j = 0; j < DCAP; ++j) xr[j] = (j < d) ? lrows[j * lld + q * NT + t] : 0.0;
      point(xr, lrows[d * lld + q * NT + t]);
    }
    for (int64_t i = t + (int64_t)NT * (RMAX + lgroups); i < n; i += UNR * NT) {   // and streamed, UNR in flight
      double xr[UNR][DCAP], ar[UNR];
#pragma unroll
      for (int q = 0; q < UNR; ++q) {                          // (all loads of the group first)
        const int64_t iq = i + q * NT;
        ar[q] = (iq < n) ? coef(iq) : 0.0;
#pragma unroll
        for (int j = 0; j < DCAP; ++j) xr[q][j] = (j < d && iq < n) ? XsT[j * ldx + iq] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < UNR; ++q) point(xr[q], ar[q]);
    }
  }
};

// ---- the surrogate at the chain's point ---------------------------------------------------------------------------------
// c + a b, as ONE explicit fma or as written and left to the compiler's contraction (the device default).  The spelling
// belongs to the kernel (k_paths_hmc_run was written with explicit fmas, the kernels on the mean without), and the two do
// not compile to the same roundings: the same chain under k_hmc_run and k_paths_hmc_run agrees to ~1e-10 after four
// iterations, not bit for bit (tests/test_gpu_paths_hmc.py).  Each kernel keeps its own.
template <bool FMA>
__device__ __forceinline__ double chain_madd(double a, double b, double c) {
  if constexpr (FMA) return __builtin_fma(a, b, c);
  else return c + a * b;
}
// The chain's point (scaled coordinates: xs in LDS) into this thread's registers, once per evaluation; coordinates >= d
// read as 0.  (Handed to chain_point in LDS, every row would read it again, and one wave per SIMD hides none of that
// latency: up to a tenth of a leapfrog step, measured.)
template <int DCAP>
__device__ __forceinline__ void chain_load_point(const double* xs, int d, double (&xsr)[DCAP]) {
#pragma unroll
  for (int j = 0; j < DCAP; ++j) xsr[j] = (j < d) ? xs[j] : 0.0;
}
// One training row (xr: its scaled coordinates, a: its coefficient) at the point xs (chain_load_point's registers): the
// value's and the gradient's contributions into ms / gm (the difference is formed twice rather than kept) ...
template <int KERN, int DCAP, bool FMA>
__device__ __forceinline__ void chain_point(const double (&xr)[DCAP], double a, const double (&xs)[DCAP], int d, double kvar,
                                            double& ms, double (&gm)[DCAP]) {
  double r2 = 0.0;
#pragma unroll
  for (int j = 0; j < DCAP; ++j) {
    const double df = (j < d) ? xr[j] - xs[j] : 0.0;
    r2 = chain_madd<FMA>(df, df, r2);
  }
  const double kv = kern_eval<KERN>(r2, kvar);
  const double ag = a * kern_grad_factor<KERN>(r2, kvar, kv);
  ms = chain_madd<FMA>(a, kv, ms);
#pragma unroll
  for (int j = 0; j < DCAP; ++j) gm[j] = chain_madd<FMA>(ag, (j < d) ? xr[j] - xs[j] : 0.0, gm[j]);
}
// ... and the value alone (k_rwalk)
template <int KERN, int DCAP>
__device__ __forceinline__ void chain_point_value(const double (&xr)[DCAP], double a, const double (&xs)[DCAP], int d, double kvar,
                                                  double& ms) {
  double r2 = 0.0;
#pragma unroll
  for (int j = 0; j < DCAP; ++j) {
    const double df = (j < d) ? xr[j] - xs[j] : 0.0;
    r2 += df * df;
  }
  ms += a * kern_eval<KERN>(r2, kvar);
}
// The 256 threads' sums into LDS, one slot per wave: the value in red[wave][DCAP], gradient component j in red[wave][j],
// the gate's partial sum at the raw point x (k_gate's order) in gred[wave].  The caller's __syncthreads() follows; then
// chain_wsum / gate_combine read them.
template <int DCAP>
__device__ __forceinline__ void chain_reduce_gate(const Gate& gt, const double* x, int d, int t, double* gred) {
  if (gate_on(gt)) {
    const double gs = gate_partial<DCAP>(gt, x, d, t);
    if ((t & 63) == 0) gred[t >> 6] = gs;
  }
}
template <int DCAP>
__device__ __forceinline__ void chain_reduce(double ms, double (&gm)[DCAP], const Gate& gt, const double* x, int d, int t,
                                             double (*red)[DCAP + 1], double* gred) {
  const int lane = t & 63, wave = t >> 6;
  ms = chain_wave_sum(ms);
  if (lane == 0) red[wave][DCAP] = ms;
  const double v = wave_sum_components<DCAP>(gm, lane);
  if ((lane & (64 / DCAP - 1)) == 0) red[wave][lane / (64 / DCAP)] = v;
  chain_reduce_gate<DCAP>(gt, x, d, t, gred);
}
template <int DCAP>
__device__ __forceinline__ void chain_reduce_value(double ms, const Gate& gt, const double* x, int d, int t, double* red,
                                                   double* gred) {
  ms = chain_wave_sum(ms);
  if ((t & 63) == 0) red[t >> 6] = ms;
  chain_reduce_gate<DCAP>(gt, x, d, t, gred);
}
// the four waves' sums in wave order, ((r0 + r1) + r2) + r3; slot w at red[w * stride]
__device__ __forceinline__ double chain_wsum(const double* red, int stride) {
  return ((red[0] + red[stride]) + red[2 * stride]) + red[3 * stride];
}

// ---- whole HMC chains on the device ---------------------------------------------------------------------------
// `niter` trajectories of every chain in ONE launch (one 256-thread workgroup = one chain): momentum draw, 4-12 leapfrog
// steps (the arithmetic of k_hmc_leapfrog), Metropolis test, and - while warming up - the chain's own dual-averaging
// step-size update (Hoffman & Gelman 2014, what NumPyro's warm-up does per chain: t0 10, gamma 0.05, kappa 0.75, target 0.8,
// eps in [1e-4, 2]).  The host only cuts the run at the mass-matrix windows.  Random numbers are a counter hash (splitmix64
// finaliser: hmc_mix64 / hmc_u01, kernels_common.hpp) of (seed, chain, iteration, index): ckey = mix(seed ^ mix(c)), ikey =
// ckey + ((it0 + it) << 12), indices 2t / 2t + 1 for the momentum of coordinate t, 4000 for L = 4 + hash % 9, 4001 for the
// Metropolis uniform.  No atomics: a chain's path depends on nothing but its own inputs and seed, whatever the batch or the
// launch boundaries.
//   S     [P][3d+2]  chain state in/out: u (d), g = dlogp/du (d), x (d), logp, mean (physical units)
//   adapt [P][5]     eps, mu, hbar, log_eps_bar, m (dual averaging; only eps is read when do_adapt == 0)
//   hist  [niter - hist_from][P][d]   u after iterations >= hist_from of this launch        (may be null)
//   keep  [niter / thin][P][d+1]      x and mean after every thin-th iteration of this launch (may be null)
//   dbg   [P][d+3]   last iteration's p0 (d), L, uniform, acceptance probability             (may be null)
// The Target is what a kernel built on this body supplies (k_paths_hmc_run: a posterior path; k_hmc_run, the posterior
// mean, is this same body written out in consumer_kernels.hpp and says there why):
//   RMAX          rows per thread in registers (ChainRows)
//   FMA           the spelling of chain_point's multiply-adds
//   coef()        the rows' coefficients (CoefMean / CoefPath)
//   inv_mass      the d inverse masses of THIS chain
//   extra(xs, d, t, ms, gm)   thread t's further terms of the value and its gradient, after its rows (xs: the point in
//                 registers, coordinates >= d zero)
// and the surrogate's value is sum_n coef_n k(x_n, x) + extra, its gradient with respect to xs likewise.
template <int KERN, int DCAP, class Target>
__device__ __forceinline__ void hmc_chain_run(const Target& tg, const double* XsT, int64_t ldx, int64_t n, const Hyper& h,
                                              int64_t P, double* S, double* adapt, unsigned long long seed, int64_t it0,
                                              int niter, int do_adapt, double ystd, double ymean, double temp,
                                              int hist_from, double* hist, int thin, double* keep, double* dbg,
                                              const Gate& gt, int lgroups) {
  constexpr int NW = 4;
  extern __shared__ double lrows[];            // [d + 1][256 lgroups]: training rows and coefficients resident in LDS
  __shared__ double x[DCAP], xs[DCAP], red[NW][DCAP + 1], lp_s, mean_s, gred[4], kin_s[2];
  __shared__ double u0[DCAP], g0[DCAP], x0[DCAP], lp0, mean0, eps_s;
  __shared__ int acc_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c = blockIdx.x;
  const int d = h.d, sw = 3 * d + 2;
  double* Sc = S + c * sw;
  double* ad = adapt + c * 5;
  if (t < d) {
    u0[t] = Sc[t];
    g0[t] = Sc[d + t];
    x0[t] = Sc[2 * d + t];
  }
  if (t == 0) {
    lp0 = Sc[3 * d];
    mean0 = Sc[3 * d + 1];
    eps_s = ad[0];
  }
  const unsigned long long ckey = hmc_mix64(seed ^ hmc_mix64((unsigned long long)c));
  const ChainTrain<DCAP, Target::RMAX, decltype(tg.coef())> rows(XsT, ldx, n, d, tg.coef(), lrows, lgroups, t);
  __syncthreads();
  // Thread t < d owns coordinate t of the trajectory (position, momentum, gradient: registers); the others only ever need
  // the point itself (x, xs in LDS).  A leapfrog step is two barriers: [every thread: its training points, the wave sums]
  // | [thread t < d: gradient, momentum, next position -> x, xs] |.  Thread 0 carries the chain's scalars and its dual-
  // averaging state in registers for the whole launch.
  const double im_r = (t < d) ? tg.inv_mass[t] : 0.0, inv_ls = (t < d) ? 1.0 / h.ls[t] : 0.0;
  double a_eps = 0.0, a_mu = 0.0, a_hbar = 0.0, a_leb = 0.0, a_m = 0.0;
  if (t == 0) {
    a_eps = ad[0];
    a_mu = ad[1];
    a_hbar = ad[2];
    a_leb = ad[3];
    a_m = ad[4];
  }
  for (int it = 0; it < niter; ++it) {
    const unsigned long long ikey = ckey + ((unsigned long long)(it0 + it) << 12);
    const double eps = eps_s;
    double u_r = 0.0, pm_r = 0.0, p0_r = 0.0, g_r = 0.0, x_r = 0.0;
    // position update of thread t < d, and the point in cube coordinates for everybody
    auto advance = [&]() {
      u_r += eps * im_r * pm_r;
      double xv = 1.0 / (1.0 + exp(-u_r));
      xv = xv < 1e-12 ? 1e-12 : (xv > 1.0 - 1e-12 ? 1.0 - 1e-12 : xv);
      x_r = xv;
      x[t] = xv;
      xs[t] = xv * inv_ls;
    };
    if (t < d) {                                               // momentum ~ N(0, M), M = diag(1 / inv_mass)
      const double a = hmc_u01(hmc_mix64(ikey + 2 * t)), b = hmc_u01(hmc_mix64(ikey + 2 * t + 1));
      const double z = sqrt(-2.0 * log(a)) * cos(6.283185307179586 * b);
      p0_r = z / sqrt(im_r);
      pm_r = p0_r + 0.5 * eps * g0[t];
      u_r = u0[t];
      advance();
    }
    const int L = 4 + (int)(hmc_mix64(ikey + 4000) % 9ull);    // (every thread: the same counter hash)
    __syncthreads();
    for (int s = 0; s < L; ++s) {
      double ms = 0.0, gm[DCAP];
#pragma unroll
      for (int j = 0; j < DCAP; ++j) gm[j] = 0.0;
      double xsr[DCAP];
      chain_load_point<DCAP>(xs, d, xsr);
      rows.for_each([&](const double (&xr)[DCAP], double a) {
        chain_point<KERN, DCAP, Target::FMA>(xr, a, xsr, d, h.kvar, ms, gm);
      });
      tg.extra(xsr, d, t, ms, gm);
      // classifier gate (clf_gp.py:173-205): an infeasible point has mean = minus_inf and no mean gradient - its
      // trajectory ends in a state that the Metropolis test never accepts
      chain_reduce<DCAP>(ms, gm, gt, x, d, t, red, gred);
      __syncthreads();
      const bool ok = gate_on(gt) ? gate_feasible(gt, gate_combine(gt, gred)) : true;
      const bool last = s == L - 1;
      if (t < d) {
        const double dm = ok ? chain_wsum(&red[0][t], DCAP + 1) * inv_ls : 0.0;
        g_r = dm * ystd / temp * (x_r * (1.0 - x_r)) + (1.0 - 2.0 * x_r);
        pm_r += (last ? 0.5 * eps : eps) * g_r;
        if (!last) advance();
      }
      if (last) {
        if (wave == 0) {                                       // kinetic energies at both ends (lanes = coordinates)
          const double k0 = chain_wave_sum(p0_r * p0_r * im_r), k1 = chain_wave_sum(pm_r * pm_r * im_r);
          if (lane == 0) {
            kin_s[0] = k0;
            kin_s[1] = k1;
          }
        } else if (wave == 1) {                                // the end point's log-density
          double jl = (lane < d) ? log(x[lane]) + log1p(-x[lane]) : 0.0;
          jl = chain_wave_sum(jl);
          if (lane == 0) {
            const double m = ok ? chain_wsum(&red[0][DCAP], DCAP + 1) * ystd + ymean : gt.minus_inf;
            mean_s = m;
            lp_s = m / temp + jl;
          }
        }
      }
      __syncthreads();
    }
    if (t == 0) {                                              // Metropolis test and the chain's step-size update
      const double h0 = lp0 - 0.5 * kin_s[0], h1 = lp_s - 0.5 * kin_s[1];
      double ap = 0.0;
      if (isfinite(h1)) ap = h1 >= h0 ? 1.0 : exp(h1 - h0);
      const double r = hmc_u01(hmc_mix64(ikey + 4001));
      const int acc = r < ap;
      acc_s = acc;
      if (acc) {
        lp0 = lp_s;
        mean0 = mean_s;
      }
      if (do_adapt) {
        constexpr double t0 = 10.0, gamma = 0.05, kappa = 0.75, target = 0.8;
        const double m = a_m + 1.0;
        const double hbar = (1.0 - 1.0 / (m + t0)) * a_hbar + (target - ap) / (m + t0);
        const double le = a_mu - sqrt(m) / gamma * hbar;
        const double eta = pow(m, -kappa);
        a_hbar = hbar;
        a_leb = eta * le + (1.0 - eta) * a_leb;
        a_m = m;
        double e = exp(le);
        e = e < 1e-4 ? 1e-4 : (e > 2.0 ? 2.0 : e);
        a_eps = e;
        eps_s = e;
      }
      if (dbg && it == niter - 1) {
        double* dc = dbg + c * (d + 3);
        dc[d] = (double)L;
        dc[d + 1] = r;
        dc[d + 2] = ap;
      }
    }
    if (dbg && it == niter - 1 && t < d) dbg[c * (d + 3) + t] = p0_r;
    __syncthreads();
    if (t < d) {
      if (acc_s) {
        u0[t] = u_r;
        g0[t] = g_r;
        x0[t] = x_r;
      }
      if (hist && it >= hist_from) hist[((int64_t)(it - hist_from) * P + c) * d + t] = u0[t];
      if (keep && (it + 1) % thin == 0) keep[((int64_t)((it + 1) / thin - 1) * P + c) * (d + 1) + t] = x0[t];
    }
    if (t == 0 && keep && (it + 1) % thin == 0) keep[((int64_t)((it + 1) / thin - 1) * P + c) * (d + 1) + d] = mean0;
    // (no barrier here: the next iteration's first one comes before anything of this one is read again - u0 / g0 / x0 are
    //  read by their own thread only, x / xs are written by advance() after every reader of this iteration has passed the
    //  barrier above, eps_s and acc_s were written before it)
  }
  if (t < d) {
    Sc[t] = u0[t];
    Sc[d + t] = g0[t];
    Sc[2 * d + t] = x0[t];
  }
  if (t == 0) {
    Sc[3 * d] = lp0;
    Sc[3 * d + 1] = mean0;
    if (do_adapt) {
      ad[0] = a_eps;
      ad[2] = a_hbar;
      ad[3] = a_leb;
      ad[4] = a_m;
    }
  }
}

}  // namespace bobe
