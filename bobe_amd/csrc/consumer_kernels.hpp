// Kernels of the surrogate's consumers: HMC on the posterior mean, EI / LogEI, the classifier gate (gfx950).
// Included by gp_consumers.hip only.
#pragma once
#include "chain_common.hpp"

namespace bobe {

// EI / LogEI pointwise scorers (BOBE/acquisition.py:21-75, 226-253, 318-330); mu, var standardised
__device__ __forceinline__ double norm_pdf(double u) { return exp(-0.5 * u * u) * 0.39894228040143267794; }
__device__ __forceinline__ double norm_cdf(double u) { return 0.5 * erfc(-u * 0.70710678118654752440); }
__device__ __forceinline__ double ei_helper(double u) { return norm_pdf(u) + u * norm_cdf(u); }
__device__ __forceinline__ double log1mexp_tfp(double x) {
  x = fabs(x);
  return (x < 0.69314718055994530942) ? log(-expm1(-x)) : log1p(-exp(-x));
}
__device__ __forceinline__ double log_ei_helper(double u) {
  const double bound = -1.0, neg_inv_sqrt_eps = -1e6;
  if (u > bound) return log(ei_helper(u));
  const double u_lower = u;
  const double u_eps = (u_lower < neg_inv_sqrt_eps) ? neg_inv_sqrt_eps : u_lower;
  const double w = log(fabs(u_eps) * erfcx(-0.70710678118654752440 * u_eps)) + 0.22579135264472743236;
  const double log_phi_u = -0.5 * (u * u + 1.83787706640934548356);
  const double second = (u > neg_inv_sqrt_eps) ? log1mexp_tfp(w) : -2.0 * log(fabs(u_lower));
  return log_phi_u + second;
}

// ---- the classifier gate of GPwithClassifier: gate_partial / gate_combine / gate_proba / gate_feasible, chain_common.hpp ----

// decision / feasibility / probability of C points (xq: C x d row-major, raw coordinates); optionally the gating of a prediction in
// place: mean -> -inf (the wrapper's sentinel for minus_inf, bobe_gp.h), var -> 1e-12 (clf_gp.py:189, 203), gradients -> 0
template <int DCAP>
__global__ __launch_bounds__(256) void k_gate(Gate gt, const double* __restrict__ xq, int d, double* __restrict__ decision,
                                              double* __restrict__ feasible, double* __restrict__ mean,
                                              double* __restrict__ var, double* __restrict__ dmean,
                                              double* __restrict__ dvar, double* __restrict__ proba) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  const double s = gate_partial<DCAP>(gt, xq + c * d, d, t);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  const double dec = gate_combine(gt, red);
  const bool ok = gate_feasible(gt, dec);
  if (t == 0) {
    if (decision) decision[c] = dec;
    if (feasible) feasible[c] = ok ? 1.0 : 0.0;
    if (proba) proba[c] = gate_proba(gt, dec);
    if (!ok) {
      if (mean) mean[c] = -INFINITY;
      if (var) var[c] = NOISE_FLOOR;
    }
  }
  if (!ok && t < d) {
    if (dmean) dmean[c * d + t] = 0.0;
    if (dvar) dvar[c * d + t] = 0.0;
  }
}

// ---- Hamiltonian Monte Carlo on the surrogate: L leapfrog steps of every chain in ONE launch ---------------------
// Consumer of the posterior mean (the reference's NUTS differentiates predict_mean_batched through JAX, one call per
// step and chain, samplers.py:268-288).  One workgroup = one chain.  Target on u = logit(x), x in the unit cube:
//   logp(u) = (mean(x) * ystd + ymean) / temp + sum_j [log x_j + log(1 - x_j)]          (Jacobian of the logit map)
//   g(u)    = dmean/dx * ystd / temp * x (1 - x) + (1 - 2x)
// with mean(x) = sum_n alpha_n k(x_n, x), dmean/dx_j = sum_n alpha_n G(r2) (s_nj - s_j) / ls_j (k_predict_grad's
// mean-only arithmetic).  In:  U, Pm = p0 + eps/2 * g(U)  (P x d).  Per step: u += eps * inv_mass * p; evaluate;
// p += (eps | eps/2 on the last step) * g.  Out: U, Pm (final), logp, grad, mean (physical units), X.
// Fixed reduction order (4 waves x lanes, then a fixed tree): a chain's trajectory does not depend on the batch.
// (Not built from chain_common.hpp's pieces on purpose: it sums the lanes with wave_sum, not chain_wave_sum, and keeps no
// rows resident - folding it in would move its bits.)
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_hmc_leapfrog(const double* __restrict__ XsT, int64_t ldx, int64_t n,
                                                      const double* __restrict__ alpha, Hyper h,
                                                      double* __restrict__ U, double* __restrict__ Pm,
                                                      const double* __restrict__ inv_mass, double eps, int L,
                                                      double ystd, double ymean, double temp,
                                                      double* __restrict__ logp, double* __restrict__ grad,
                                                      double* __restrict__ mean_out, double* __restrict__ Xout, Gate gt) {
  __shared__ double u[DCAP], pm[DCAP], x[DCAP], xs[DCAP], g[DCAP], red[4][DCAP + 1], lp_s, mean_s, gred[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c = blockIdx.x;
  const int d = h.d;
  if (t < d) {
    u[t] = U[c * d + t];
    pm[t] = Pm[c * d + t];
  }
  __syncthreads();
  for (int s = 0; s < L; ++s) {
    if (t < d) {
      const double un = u[t] + eps * inv_mass[t] * pm[t];
      u[t] = un;
      double xv = 1.0 / (1.0 + exp(-un));
      xv = xv < 1e-12 ? 1e-12 : (xv > 1.0 - 1e-12 ? 1.0 - 1e-12 : xv);
      x[t] = xv;
      xs[t] = xv / h.ls[t];
    }
    __syncthreads();
    double ms = 0.0, gm[DCAP];
#pragma unroll
    for (int j = 0; j < DCAP; ++j) gm[j] = 0.0;
    for (int64_t i = t; i < n; i += 256) {
      double df[DCAP];
      double r2 = 0.0;
#pragma unroll
      for (int j = 0; j < DCAP; ++j) {
        df[j] = (j < d) ? XsT[j * ldx + i] - xs[j] : 0.0;
        r2 += df[j] * df[j];
      }
      const double kv = kern_eval<KERN>(r2, h.kvar);
      const double a = alpha[i];
      const double ag = a * kern_grad_factor<KERN>(r2, h.kvar, kv);
      ms += a * kv;
#pragma unroll
      for (int j = 0; j < DCAP; ++j) gm[j] += ag * df[j];
    }
    ms = wave_sum(ms);
    if (lane == 0) red[wave][DCAP] = ms;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) {
      if (j < d) {
        const double v = wave_sum(gm[j]);
        if (lane == 0) red[wave][j] = v;
      }
    }
    // classifier gate (clf_gp.py:173-205): an infeasible point has mean = minus_inf and no mean gradient
    if (gate_on(gt)) {
      const double gs = gate_partial<DCAP>(gt, x, d, t);
      if (lane == 0) gred[wave] = gs;
    }
    __syncthreads();
    const bool ok = gate_on(gt) ? gate_feasible(gt, gate_combine(gt, gred)) : true;
    if (t < d) {
      const double dm = ok ? (((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]) / h.ls[t] : 0.0;
      const double xv = x[t];
      const double gv = dm * ystd / temp * (xv * (1.0 - xv)) + (1.0 - 2.0 * xv);
      g[t] = gv;
      pm[t] += ((s < L - 1) ? eps : 0.5 * eps) * gv;
    }
    if (t == 0) {
      const double m = ok ? (((red[0][DCAP] + red[1][DCAP]) + red[2][DCAP]) + red[3][DCAP]) * ystd + ymean : gt.minus_inf;
      double jac = 0.0;
      for (int j = 0; j < d; ++j) jac += log(x[j]) + log1p(-x[j]);
      mean_s = m;
      lp_s = m / temp + jac;
    }
    __syncthreads();
  }
  if (t < d) {
    U[c * d + t] = u[t];
    Pm[c * d + t] = pm[t];
    grad[c * d + t] = g[t];
    Xout[c * d + t] = x[t];
  }
  if (t == 0) {
    logp[c] = lp_s;
    mean_out[c] = mean_s;
  }
}

// ---- whole HMC chains on the posterior mean ------------------------------------------------------------------------
// The contract (one 256-thread workgroup per chain, the state / adapt / hist / keep / dbg layouts, the random numbers, dual
// averaging) is the comment above hmc_chain_run (chain_common.hpp), and this kernel is that body on the target of
// k_hmc_leapfrog - coefficients alpha, one inv_mass vector for every chain, nothing beyond the training rows, multiply-adds
// left to the compiler's contraction - written out.  It stays its OWN COPY for speed alone: built on hmc_chain_run (the
// target would be {RMAX = ChainRows::HMC, FMA = false, coef = CoefMean, no extra terms}) it gave the same bits with fewer
// registers, but ran 2 - 5 % slower per leapfrog step on every line of tools/paths_hmc_timing.py
// (profiles/chain_core_unify_ab.txt), and the cause was not found.  A change to the transition is made in both places;
// tests/test_gpu_paths_hmc.py (the same chain under both kernels) holds them together.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950), rbf / matern, with ChainRows<DCAP>::HMC = 14 / 6 / 2 rows
// in registers: DCAP 8: 256 VGPRs + 210 / 228 AGPRs, DCAP 16: 256 + 227 / 245, DCAP 32: 256 + 220 / 230; one wave per SIMD
// and scratch 0 in all six.  LDS: 704 / 1280 / 2432 bytes static.
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_hmc_run(const double* __restrict__ XsT, int64_t ldx, int64_t n,
                                                 const double* __restrict__ alpha, Hyper h, int64_t P,
                                                 double* __restrict__ S, double* __restrict__ adapt,
                                                 const double* __restrict__ inv_mass, unsigned long long seed,
                                                 int64_t it0, int niter, int do_adapt, double ystd, double ymean,
                                                 double temp, int hist_from, double* __restrict__ hist, int thin,
                                                 double* __restrict__ keep, double* __restrict__ dbg, Gate gt,
                                                 int lgroups) {
  constexpr int NT = 256, NW = NT / 64;
  extern __shared__ double lrows[];            // [d + 1][256 lgroups]: training points resident in LDS (chain_lds_groups)
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
  // The first RMAX training points of a thread (rows t, t + 256, ...) are loaded ONCE per launch - a launch is hundreds of
  // leapfrog steps, each of which would otherwise wait for the same global loads again -; points past n carry alpha = 0.
  // The next 256 lgroups rows live in LDS (every thread its own), and what fits neither is streamed from L2 in every step.
  constexpr int RMAX = ChainRows<DCAP>::HMC, UNR = ChainRows<DCAP>::STREAM;
  const int nrow = (int)((n + NT - 1) / NT);
  const int lld = NT * lgroups;
  double cx[RMAX][DCAP], ca[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    const int64_t i = t + NT * r;
    ca[r] = (i < n) ? alpha[i] : 0.0;
#pragma unroll
    for (int j = 0; j < DCAP; ++j) cx[r][j] = (j < d && i < n) ? XsT[j * ldx + i] : 0.0;
  }
  for (int q = 0; q < lgroups; ++q) {
    const int64_t i = t + (int64_t)NT * (RMAX + q);
    for (int j = 0; j < d; ++j) lrows[j * lld + q * NT + t] = (i < n) ? XsT[j * ldx + i] : 0.0;
    lrows[d * lld + q * NT + t] = (i < n) ? alpha[i] : 0.0;
  }
  __syncthreads();
  // Thread t < d owns coordinate t of the trajectory (position, momentum, gradient: registers); the others only ever need
  // the point itself (x, xs in LDS).  A leapfrog step is two barriers: [every thread: its training points, the wave sums]
  // | [thread t < d: gradient, momentum, next position -> x, xs] |.  Thread 0 carries the chain's scalars and its dual-
  // averaging state in registers for the whole launch.
  const double im_r = (t < d) ? inv_mass[t] : 0.0, inv_ls = (t < d) ? 1.0 / h.ls[t] : 0.0;
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
      // one training point: mean and mean-gradient contributions (the difference is formed twice rather than kept)
      auto point = [&](const double (&xr)[DCAP], double a) {
        double r2 = 0.0;
#pragma unroll
        for (int j = 0; j < DCAP; ++j) {
          const double df = (j < d) ? xr[j] - xs[j] : 0.0;
          r2 += df * df;
        }
        const double kv = kern_eval<KERN>(r2, h.kvar);
        const double ag = a * kern_grad_factor<KERN>(r2, h.kvar, kv);
        ms += a * kv;
#pragma unroll
        for (int j = 0; j < DCAP; ++j) gm[j] += ag * ((j < d) ? xr[j] - xs[j] : 0.0);
      };
#pragma unroll
      for (int r = 0; r < RMAX; ++r)
        if (r < nrow) point(cx[r], ca[r]);                     // (uniform) this thread's points in registers,
      for (int q = 0; q < lgroups; ++q) {                      // in LDS,
        double xr[DCAP];
#pragma unroll
        for (int j = 0; j < DCAP; ++j) xr[j] = (j < d) ? lrows[j * lld + q * NT + t] : 0.0;
        point(xr, lrows[d * lld + q * NT + t]);
      }
      for (int64_t i = t + (int64_t)NT * (RMAX + lgroups); i < n; i += UNR * NT) {  // and streamed: ascending rows throughout
        double xr[UNR][DCAP], ar[UNR];
#pragma unroll
        for (int q = 0; q < UNR; ++q) {                                // (all loads of the group first)
          const int64_t iq = i + q * NT;
          ar[q] = (iq < n) ? alpha[iq] : 0.0;
#pragma unroll
          for (int j = 0; j < DCAP; ++j) xr[q][j] = (j < d && iq < n) ? XsT[j * ldx + iq] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < UNR; ++q) point(xr[q], ar[q]);
      }
      ms = chain_wave_sum(ms);
      if (lane == 0) red[wave][DCAP] = ms;
      {
        const double v = wave_sum_components<DCAP>(gm, lane);
        if ((lane & (64 / DCAP - 1)) == 0) red[wave][lane / (64 / DCAP)] = v;
      }
      // classifier gate (clf_gp.py:173-205): an infeasible point has mean = minus_inf and no mean gradient - its
      // trajectory ends in a state that the Metropolis test never accepts
      if (gate_on(gt)) {                                       // (the gate's 256 partial sums: k_gate's order)
        const double gs = gate_partial<DCAP>(gt, x, d, t);
        if (lane == 0) gred[wave] = gs;
      }
      __syncthreads();
      const bool ok = gate_on(gt) ? gate_feasible(gt, gate_combine(gt, gred)) : true;
      // (the waves' sums in wave order: ((r0 + r1) + r2) + r3)
      auto wsum = [&](int j) {
        double sres = red[0][j];
#pragma unroll
        for (int w_ = 1; w_ < NW; ++w_) sres += red[w_][j];
        return sres;
      };
      const bool last = s == L - 1;
      if (t < d) {
        const double dm = ok ? wsum(t) * inv_ls : 0.0;
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
            const double m = ok ? wsum(DCAP) * ystd + ymean : gt.minus_inf;
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

// ---- No-U-Turn sampling on the device (NumPyro's NUTS, the reference's sampler: samplers.py:216-330) ---------------
// `niter` NUTS transitions of every chain in ONE launch, one 256-thread workgroup per chain; the target and the state layout
// are those of k_hmc_run, and the one-point evaluation is chain_common.hpp's (ChainTrain, chain_point, chain_reduce,
// chain_wsum: the same rows, arithmetic, reduction order and gate).
//
// Contract (tests/nuts_restatement.py restates it in NumPy):
//   Metric.  Sigma = the d x d inverse metric, C = lower Cholesky factor of M = Sigma^-1 (both from the host).  Momentum
//     p = C z, z ~ N(0, I); kinetic energy K(p) = 1/2 p^T Sigma p; velocity Sigma p.  H = -logp + K, H0 at the start.
//   Leaf.  One velocity-Verlet step of signed size e (+eps going right, -eps going left) from the tree's edge in that
//     direction (from the previous leaf inside a subtree): p' = p + e/2 g(u); u += e Sigma p'; p = p' + e/2 g(u).
//     dH = H - H0 (NaN -> +inf); log weight w = -dH; acceptance min(1, exp(-dH)); divergent if dH > 1000 or dH is not
//     finite (a gated leaf has mean minus_inf: at the default -1e5 it is divergent).
//   Tree (iterative_build_tree of NumPyro, Betancourt 2017 appendix A).  Start: one node, the current state, weight 0,
//     rho = p0.  Doubling j = 0, 1, ... while j < max_tree_depth and the tree neither turned nor diverged:
//     direction bit b_j; a subtree of up to 2^j leaves k = 0, 1, ... is built leaf by leaf:
//       - progressive sampling: leaf 0 is the subtree's proposal; leaf k > 0 replaces it when its uniform is below
//         exp(w_k - logaddexp(W_sub, w_k)); then W_sub = logaddexp(W_sub, w_k), rho_sub += p_k;
//       - checkpoints (Stan / NumPyro): at even k, slot popcount(k >> 1) keeps p_k, Sigma p_k and rho_sub; at odd k the
//         completed sub-subtrees ending at k are checked, slots i = popcount(k >> 1) down to that minus (trailing ones of
//         k) + 1: with r = rho_sub - rho_ck[i] + p_ck[i] - (p_ck[i] + p_k) / 2, the subtree turned if
//         (Sigma p_ck[i]) . r <= 0 or (Sigma p_k) . r <= 0;
//       - the subtree stops at 2^j leaves, at a turned check or at a divergent leaf.
//     Merge: unless the subtree turned or diverged, its proposal replaces the tree's when the merge uniform is below
//     min(1, exp(W_sub - W)) (biased progressive sampling); W = logaddexp(W, W_sub), rho += rho_sub, the edge in direction
//     b_j becomes the subtree's last leaf, depth = j + 1; the whole tree turned if the subtree did or, with
//     r = rho - (p_left + p_right) / 2, (Sigma p_left) . r <= 0 or (Sigma p_right) . r <= 0.
//   Transition: the tree's proposal is the next state.  Acceptance statistic = mean over all leaves built of
//     min(1, exp(-dH)); it drives k_hmc_run's per-chain dual averaging (target 0.8) while adapting.
//   Random numbers: ikey = ckey + ((it0 + iteration) << 14), ckey as in k_hmc_run; index 2t, 2t + 1 -> Box-Muller normal
//     z_t; 64 + j -> direction of doubling j (top bit: 1 = right); 128 + 1024 j -> the merge uniform of doubling j;
//     128 + 1024 j + k -> the selection uniform of leaf k >= 1 of subtree j.
// Control flow: every lane of wave 0 (which holds the d <= 32 coordinate threads) computes the same scalars from the same
// wave sums and decides; thread 0 publishes "stop" through LDS, and every barrier sits under a loop condition read from
// there, i.e. a workgroup-uniform one.
//   metric [2][d][d]  Sigma, then C (row-major, C lower)
//   stats  [niter][P][4]  tree depth, leapfrog steps, divergent flag, acceptance statistic        (may be null)
//   dbg    [P][d]         last transition's momentum draw p0                                       (may be null)
//   S, adapt, hist, keep as k_hmc_run.
constexpr int NUTS_MAX_DEPTH = 10;
constexpr int NUTS_LDS_BYTES = 138 * 1024;             // (the static arrays: Sigma, checkpoints, ... stay below 22 KB)

__device__ __forceinline__ double nuts_logaddexp(double a, double b) {
  const double hi = a > b ? a : b, lo = a > b ? b : a;
  if (hi == -INFINITY) return hi;
  return hi + log1p(exp(lo - hi));
}

template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_nuts_run(const double* __restrict__ XsT, int64_t ldx, int64_t n,
                                                  const double* __restrict__ alpha, Hyper h, int64_t P,
                                                  double* __restrict__ S, double* __restrict__ adapt,
                                                  const double* __restrict__ metric, int max_depth,
                                                  unsigned long long seed, int64_t it0, int niter, int do_adapt,
                                                  double ystd, double ymean, double temp, int hist_from,
                                                  double* __restrict__ hist, int thin, double* __restrict__ keep,
                                                  double* __restrict__ stats, double* __restrict__ dbg, Gate gt,
                                                  int lgroups) {
  constexpr int NT = 256, NW = NT / 64, SLD = DCAP + 1;
  extern __shared__ double lrows[];            // [d + 1][256 lgroups]: training points resident in LDS (chain_lds_groups)
  __shared__ double x[DCAP], xs[DCAP], red[NW][DCAP + 1], gred[4];
  __shared__ double sig[DCAP * SLD], zb[DCAP], pv[DCAP], phs[DCAP];
  __shared__ double ck_p[NUTS_MAX_DEPTH][DCAP], ck_v[NUTS_MAX_DEPTH][DCAP], ck_r[NUTS_MAX_DEPTH][DCAP];
  __shared__ int stop_leaf, stop_tree;
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t c = blockIdx.x;
  const int d = h.d, sw = 3 * d + 2;
  const bool own = t < d;                      // coordinate thread (all of them in wave 0)
  double* Sc = S + c * sw;
  double* ad = adapt + c * 5;
  for (int i = t; i < d * d; i += NT) sig[(i / d) * SLD + i % d] = metric[i];
  const double* Crow = metric + (int64_t)d * d + (int64_t)(own ? t : 0) * d;
  // chain state: coordinates in the registers of their thread, scalars in every lane of wave 0
  double u0 = 0.0, g0 = 0.0, x0 = 0.0, lp0 = 0.0, mean0 = 0.0;
  double a_eps = 0.0, a_mu = 0.0, a_hbar = 0.0, a_leb = 0.0, a_m = 0.0;
  if (own) {
    u0 = Sc[t];
    g0 = Sc[d + t];
    x0 = Sc[2 * d + t];
  }
  if (wave == 0) {
    lp0 = Sc[3 * d];
    mean0 = Sc[3 * d + 1];
    a_eps = ad[0];
    a_mu = ad[1];
    a_hbar = ad[2];
    a_leb = ad[3];
    a_m = ad[4];
  }
  const unsigned long long ckey = hmc_mix64(seed ^ hmc_mix64((unsigned long long)c));
  const ChainTrain<DCAP, ChainRows<DCAP>::NUTS, CoefMean> rows(XsT, ldx, n, d, CoefMean{alpha}, lrows, lgroups, t);
  __syncthreads();
  const double inv_ls = own ? 1.0 / h.ls[t] : 0.0;
  auto sig_dot = [&](const double* vec) {                    // row t of Sigma against a vector in LDS
    double s = 0.0;
    for (int q = 0; q < d; ++q) s = fma(sig[t * SLD + q], vec[q], s);
    return s;
  };
  // the surrogate at x / xs (LDS): every thread's training points, then the waves' sums (k_hmc_run's arithmetic and
  // order); ends with a barrier, after which wsum() / the gate's decision can be read
  auto evaluate = [&]() {
    double ms = 0.0, gm[DCAP];
#pragma unroll
    for (int j = 0; j < DCAP; ++j) gm[j] = 0.0;
    double xsr[DCAP];
    chain_load_point<DCAP>(xs, d, xsr);
    rows.for_each([&](const double (&xr)[DCAP], double a) { chain_point<KERN, DCAP, false>(xr, a, xsr, d, h.kvar, ms, gm); });
    chain_reduce<DCAP>(ms, gm, gt, x, d, t, red, gred);
    __syncthreads();
  };
  auto wsum = [&](int j) { return chain_wsum(&red[0][j], DCAP + 1); };
  for (int it = 0; it < niter; ++it) {
    const unsigned long long ikey = ckey + ((unsigned long long)(it0 + it) << 14);
    const double eps = a_eps;
    // momentum p0 = C z and its velocity
    if (own) {
      const double a = hmc_u01(hmc_mix64(ikey + 2 * t)), b = hmc_u01(hmc_mix64(ikey + 2 * t + 1));
      zb[t] = sqrt(-2.0 * log(a)) * cos(6.283185307179586 * b);
    }
    __syncthreads();
    double p0 = 0.0;
    if (own) {
      for (int q = 0; q <= t; ++q) p0 = fma(Crow[q], zb[q], p0);
      pv[t] = p0;
    }
    __syncthreads();
    // the tree (wave 0): edges, momentum sum, proposal; scalars identical in every lane of wave 0
    double v0 = own ? sig_dot(pv) : 0.0;
    double H0 = 0.0;
    if (wave == 0) H0 = -lp0 + 0.5 * chain_wave_sum(p0 * v0);
    double uL = u0, pL = p0, gL = g0, vL = v0, uR = u0, pR = p0, gR = g0, vR = v0, rho = p0;
    double uP = u0, gP = g0, xP = x0, lpP = lp0, meanP = mean0;
    double W = 0.0, sum_acc = 0.0;
    int nleap = 0, depth = 0;
    bool diverged = false;
    double u = 0.0, p = 0.0, g = 0.0, xv = 0.0, v = 0.0;
    for (int j = 0; j < max_depth; ++j) {
      const bool right = (hmc_mix64(ikey + 64 + (unsigned long long)j) >> 63) != 0;
      const double e = right ? eps : -eps;
      const int nleaf = 1 << j;
      double rs = 0.0, uS = 0.0, gS = 0.0, xS = 0.0, lpS = 0.0, meanS = 0.0, Ws = -INFINITY;
      bool tsub = false;
      if (own) {
        u = right ? uR : uL;
        p = right ? pR : pL;
        g = right ? gR : gL;
        phs[t] = p + 0.5 * e * g;
      }
      __syncthreads();
      for (int k = 0; k < nleaf; ++k) {
        if (own) {                                             // position half of the leapfrog step
          u += e * sig_dot(phs);
          double xx = 1.0 / (1.0 + exp(-u));
          xx = xx < 1e-12 ? 1e-12 : (xx > 1.0 - 1e-12 ? 1.0 - 1e-12 : xx);
          xv = xx;
          x[t] = xx;
          xs[t] = xx * inv_ls;
        }
        __syncthreads();
        evaluate();
        const bool ok = gate_on(gt) ? gate_feasible(gt, gate_combine(gt, gred)) : true;
        if (own) {                                             // gradient and momentum
          const double dm = ok ? wsum(t) * inv_ls : 0.0;
          g = dm * ystd / temp * (xv * (1.0 - xv)) + (1.0 - 2.0 * xv);
          p = phs[t] + 0.5 * e * g;
          pv[t] = p;
        }
        __syncthreads();
        if (wave == 0) {
          v = own ? sig_dot(pv) : 0.0;
          const double kin = chain_wave_sum(p * v);
          const double jl = chain_wave_sum(own ? log(xv) + log1p(-xv) : 0.0);
          const double m = ok ? wsum(DCAP) * ystd + ymean : gt.minus_inf;
          const double lp = m / temp + jl;
          double dH = (0.5 * kin - lp) - H0;
          if (dH != dH) dH = INFINITY;
          const double w = -dH;
          const bool dvg = !isfinite(dH) || dH > 1000.0;
          sum_acc += dH <= 0.0 ? 1.0 : exp(-dH);
          ++nleap;
          bool take = k == 0;
          if (k == 0) {
            Ws = w;
          } else {
            const double Wn = nuts_logaddexp(Ws, w);
            take = hmc_u01(hmc_mix64(ikey + 128 + 1024 * (unsigned long long)j + k)) < exp(w - Wn);
            Ws = Wn;
          }
          if (take) {
            uS = u;
            gS = g;
            xS = xv;
            lpS = lp;
            meanS = m;
          }
          rs += p;
          const int imax = __popc((unsigned)k >> 1);
          if ((k & 1) == 0) {
            if (own) {
              ck_p[imax][t] = p;
              ck_v[imax][t] = v;
              ck_r[imax][t] = rs;
            }
          } else {
            const int imin = imax - __builtin_ctz(~(unsigned)k) + 1;
            for (int i = imax; i >= imin && !tsub; --i) {      // (a lane reads back only its own coordinate)
              const double r = own ? rs - ck_r[i][t] + ck_p[i][t] - 0.5 * (ck_p[i][t] + p) : 0.0;
              const double a = chain_wave_sum(own ? ck_v[i][t] * r : 0.0), b = chain_wave_sum(v * r);
              tsub = a <= 0.0 || b <= 0.0;
            }
          }
          diverged = dvg;
          if (t == 0) stop_leaf = dvg || tsub;
          if (own) phs[t] = p + 0.5 * e * g;                   // the next leaf starts here
        }
        __syncthreads();
        if (stop_leaf) break;
      }
      if (wave == 0) {                                         // merge the subtree into the tree
        const bool usable = !tsub && !diverged;
        const double pr = usable ? (Ws >= W ? 1.0 : exp(Ws - W)) : 0.0;
        if (hmc_u01(hmc_mix64(ikey + 128 + 1024 * (unsigned long long)j)) < pr) {
          uP = uS;
          gP = gS;
          xP = xS;
          lpP = lpS;
          meanP = meanS;
        }
        W = nuts_logaddexp(W, Ws);
        rho += rs;
        if (right) {
          uR = u; pR = p; gR = g; vR = v;
        } else {
          uL = u; pL = p; gL = g; vL = v;
        }
        depth = j + 1;
        const double r = own ? rho - 0.5 * (pL + pR) : 0.0;
        const double a = chain_wave_sum(vL * r), b = chain_wave_sum(vR * r);
        const bool turned = tsub || a <= 0.0 || b <= 0.0;
        if (t == 0) stop_tree = turned || diverged;
      }
      __syncthreads();
      if (stop_tree) break;
    }
    if (wave == 0) {                                           // the transition and the chain's step-size update
      u0 = uP;
      g0 = gP;
      x0 = xP;
      lp0 = lpP;
      mean0 = meanP;
      const double ap = sum_acc / (double)nleap;
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
      }
      if (t == 0 && stats) {
        double* sc = stats + ((int64_t)it * P + c) * 4;
        sc[0] = (double)depth;
        sc[1] = (double)nleap;
        sc[2] = diverged ? 1.0 : 0.0;
        sc[3] = ap;
      }
      if (own) {
        if (dbg && it == niter - 1) dbg[c * d + t] = p0;
        if (hist && it >= hist_from) hist[((int64_t)(it - hist_from) * P + c) * d + t] = u0;
        if (keep && (it + 1) % thin == 0) keep[((int64_t)((it + 1) / thin - 1) * P + c) * (d + 1) + t] = x0;
      }
      if (t == 0 && keep && (it + 1) % thin == 0) keep[((int64_t)((it + 1) / thin - 1) * P + c) * (d + 1) + d] = mean0;
    }
    // (no barrier here: zb is next written after every reader has passed two barriers, pv / phs after one more)
  }
  if (own) {
    Sc[t] = u0;
    Sc[d + t] = g0;
    Sc[2 * d + t] = x0;
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

// ---- constrained random walks for nested sampling, whole walks on the device -----------------------------------------
// The replacement search of a nested-sampling iteration (dynesty's 'rwalk', the reference's choice: samplers.py:64, 152):
// every walker starts at a live point and takes `walks` Metropolis steps inside {mean(x) > lstar, unit cube}; a step is
// x' = x + step[d x d] z, z ~ N(0, I) (step = scale x the Cholesky factor of the live points' covariance, lower, row-major).
// One workgroup = one walker, every step's surrogate mean by the reduction of k_hmc_run (training points in registers),
// the classifier gate applied like everywhere else (an infeasible proposal has mean = minus_inf and is never accepted).
// Random numbers: the counter hash of k_hmc_run on (seed, walker, step, index).
//   X    [P][d]  in: start points, out: end points        logl [P]  in / out: physical-unit mean at the point
//   nacc [P]     accepted steps                            nin  [P]  proposals inside the cube (= surrogate calls)
//   dbg  [P][d]  the LAST proposal of every walker (tests)                                             (may be null)
template <int KERN, int DCAP>
__global__ __launch_bounds__(256) void k_rwalk(const double* __restrict__ XsT, int64_t ldx, int64_t n,
                                               const double* __restrict__ alpha, Hyper h, double* __restrict__ X,
                                               double* __restrict__ logl, const double* __restrict__ step, double lstar,
                                               int walks, unsigned long long seed, double ystd, double ymean,
                                               int* __restrict__ nacc, int* __restrict__ nin, double* __restrict__ dbg,
                                               Gate gt, int lgroups) {
  constexpr int NT = 256, NW = NT / 64;
  extern __shared__ double lrows[];
  __shared__ double x[DCAP], xp[DCAP], xs[DCAP], z[DCAP], red[NW], gred[4], lx, stp[DCAP * DCAP];
  __shared__ int inside_s, na_s, ni_s;
  const int t = threadIdx.x, wave = t >> 6;
  const int64_t c = blockIdx.x;
  const int d = h.d;
  if (t < d) x[t] = X[c * d + t];
  for (int k = t; k < d * d; k += NT) stp[k] = step[k];               // (read in every step: keep it in LDS)
  if (t == 0) {
    lx = logl[c];
    na_s = 0;
    ni_s = 0;
  }
  const unsigned long long ckey = hmc_mix64(seed ^ hmc_mix64((unsigned long long)c));
  // training points in registers, in LDS and streamed, like k_hmc_run (only the mean is needed here)
  const ChainTrain<DCAP, ChainRows<DCAP>::WALK, CoefMean> rows(XsT, ldx, n, d, CoefMean{alpha}, lrows, lgroups, t);
  __syncthreads();
  for (int s = 0; s < walks; ++s) {
    const unsigned long long ikey = ckey + ((unsigned long long)s << 12);
    if (t < d) {
      const double a = hmc_u01(hmc_mix64(ikey + 2 * t)), b = hmc_u01(hmc_mix64(ikey + 2 * t + 1));
      z[t] = sqrt(-2.0 * log(a)) * cos(6.283185307179586 * b);
    }
    __syncthreads();
    if (wave == 0) {                                                       // (d <= 32: the coordinates live in wave 0)
      bool in = true;
      if (t < d) {
        double v = x[t];
        for (int j = 0; j <= t; ++j) v += stp[t * d + j] * z[j];            // (lower-triangular factor)
        xp[t] = v;
        xs[t] = v / h.ls[t];
        in = (v >= 0.0) && (v <= 1.0);
      }
      const int all_in = __all(in);
      if (t == 0) {
        inside_s = all_in;
        ni_s += all_in;
      }
    }
    __syncthreads();
    if (inside_s) {                                                        // (uniform: a proposal outside costs no evaluation)
      double ms = 0.0, xsr[DCAP];
      chain_load_point<DCAP>(xs, d, xsr);
      rows.for_each([&](const double (&xr)[DCAP], double a) { chain_point_value<KERN, DCAP>(xr, a, xsr, d, h.kvar, ms); });
      chain_reduce_value<DCAP>(ms, gt, xp, d, t, red, gred);
      __syncthreads();
      if (t == 0) {
        double m = chain_wsum(red, 1) * ystd + ymean;
        if (gate_on(gt) && !gate_feasible(gt, gate_combine(gt, gred))) m = gt.minus_inf;
        const int acc = m > lstar;
        inside_s = acc;                                                    // (reused: accepted)
        if (acc) {
          lx = m;
          ++na_s;
        }
      }
      __syncthreads();
      if (inside_s && t < d) x[t] = xp[t];
    }
    __syncthreads();
  }
  if (t < d) {
    X[c * d + t] = x[t];
    if (dbg) dbg[c * d + t] = xp[t];
  }
  if (t == 0) {
    logl[c] = lx;
    nacc[c] = na_s;
    nin[c] = ni_s;
  }
}

// mode 0: EI, 1: LogEI.  out = +EI / +logEI (the reference minimises the negative).  A mean of -inf is the gate's mark
// (k_gate): the reference's predict_single returns minus_inf there (clf_gp.py:201-204)
__global__ void k_ei(const double* __restrict__ mu, const double* __restrict__ var, int64_t n, double best_y, double zeta,
                     int mode, double* __restrict__ out, double minus_inf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = var[i];
  const double lo = mode ? 1e-18 : 1e-20;
  if (v < lo) v = lo;
  const double sigma = sqrt(v);
  double m = mu[i];
  if (m == -INFINITY) m = minus_inf;
  const double u = (m - zeta - best_y) / sigma;
  out[i] = mode ? (log_ei_helper(u) + log(sigma)) : (ei_helper(u) * sigma);
}

// k_ei with its input gradient, from predict_grad's chain (mu, var: n; dmu, dvar: n x d, standardised units).  One thread per
// point: the point's scalars once - the value by k_ei's statements on k_ei's device functions -, then its d coordinates.
// sigma = sqrt(max(var, lo)), dsigma = dvar / (2 sigma), and 0 where var was clipped; u = (mu - zeta - best_y) / sigma.
//   EI:    grad = Phi(u) dmu + phi(u) dsigma
//   LogEI: grad = A dmu + B dsigma, A = Phi / (sigma h), B = phi / (sigma h), h = phi + u Phi; directly for u > -1.  At and
//          below (log_ei_helper's own bound; Phi / h turns into 0 / 0 near u = -38) through the Mills ratio
//          R = Phi / phi = sqrt(pi / 2) erfcx(-u / sqrt 2):  g = h / phi = 1 - |u| R,  B = 1 / (sigma g),  A = R B.
//          1 - |u| R cancels to ~1 / u^2, so from |u| = 30 on g is its asymptotic series
//          1/u^2 - 3/u^4 + 15/u^6 - ... (nine terms: the ninth is 8e-17 of the first at |u| = 30), and the difference itself
//          only below, where it loses at most log10(900) ~ 3 of the 16 digits.  (log h is NOT taken from log_ei_helper here:
//          its log1mexp(w), w -> -1 / u^2, carries an absolute error ~1e-16 u^2 - invisible beside the value's u^2 / 2,
//          but 1e-9 of B at u = -4500 and 1e-4 at u = -1e6, where a floored point one unit below the target sits.)
// A gated point (mu = -inf, k_gate's mark) has the value of (minus_inf, 1e-12) and a gradient of exactly 0.
__global__ __launch_bounds__(256) void k_ei_grad(const double* __restrict__ mu, const double* __restrict__ var,
                                                 const double* __restrict__ dmu, const double* __restrict__ dvar, int64_t n,
                                                 int d, double best_y, double zeta, int mode, double minus_inf,
                                                 double* __restrict__ val, double* __restrict__ grad) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  double v = var[c];
  const double lo = mode ? 1e-18 : 1e-20;
  const bool clipped = v < lo;
  if (v < lo) v = lo;
  const double sigma = sqrt(v);
  double m = mu[c];
  const bool gated = m == -INFINITY;
  if (m == -INFINITY) m = minus_inf;
  const double u = (m - zeta - best_y) / sigma;
  val[c] = mode ? (log_ei_helper(u) + log(sigma)) : (ei_helper(u) * sigma);
  double a = 0.0, b = 0.0;
  if (gated) {
    // (a = b = 0)
  } else if (!mode) {
    a = norm_cdf(u);
    b = norm_pdf(u);
  } else if (u > -1.0) {
    const double sh = sigma * ei_helper(u);
    a = norm_cdf(u) / sh;
    b = norm_pdf(u) / sh;
  } else {
    const double x = -u, r = 1.25331413731550025121 * erfcx(0.70710678118654752440 * x);
    double g;
    if (x < 30.0) {
      g = 1.0 - x * r;
    } else {
      const double t = 1.0 / (x * x);
      g = t * (1.0 - t * (3.0 - t * (15.0 - t * (105.0 - t * (945.0 - t * (10395.0 - t * (135135.0 - t * (2027025.0 - t * 34459425.0))))))));
    }
    b = 1.0 / (sigma * g);
    a = r * b;
  }
  for (int j = 0; j < d; ++j) {
    const int64_t i = c * d + j;
    const double ds = clipped ? 0.0 : dvar[i] / (2.0 * sigma);
    grad[i] = gated ? 0.0 : a * dmu[i] + b * ds;
  }
}

// ---- training of the ellipsoid classifier (clf.py:415-472): every restart's whole AdamW run in ONE launch ----------
// One 256-thread workgroup = one restart (blockIdx.x).  Parameters theta = [flat_L (T = d(d+1)/2, tril_indices order:
// (0,0), (1,0), (1,1), (2,0), ...), alpha, beta], P = T + 2 <= 530: thread t owns theta[t], theta[t + 256], theta[t + 512]
// and their Adam moments in registers; the transformed L (diagonal softplus + 1e-4) lives in LDS, dense [i][j].
// Per step (batch b of B rows, rows perm[...]; B = min(batch, N)), in chunks of 64 rows:
//   A  gather diff = x - mu of the chunk's rows into LDS
//   B  wave q, lane b: u_j = sum_{i >= j} L[i][j] diff_i (ascending i) for j = q, q + 4, ...; the wave's sum of u_j^2
//   C  thread b: md2 = ((s0 + s1) + s2) + s3, logit = -alpha md2 + beta, g_b = (sigmoid(logit) - y_b) / B
//      (the gradient of optax.sigmoid_binary_cross_entropy(logit, y).mean())
//   D  thread of theta_p: accumulate over the chunk's rows in ascending order
//        dL[i][j] = sum_b g_b u_bj diff_bi (x -2 alpha, x sigmoid(flat) on the diagonal), dalpha = -sum_b g_b md2_b,
//        dbeta = sum_b g_b
// then optax.adamw (b1 0.9, b2 0.999, eps 1e-8, eps_root 0, decay on every parameter) in optax's order of operations.
// At the end: the parameters and the full-data loss (rows t, t + 256, ... per thread, then the waves in order).
//   perm  [R][n_epochs][steps * B] int32 row indices (the host's RandomState permutations; validated by the host)
//   init  [R][P]   starting parameters;   params_out [R][P];   loss_out [R]
constexpr int ELL_NT = 256, ELL_ROWS = 64, ELL_DS = MAX_D + 1;
__global__ __launch_bounds__(256) void k_ellipsoid_train(const double* __restrict__ X, const double* __restrict__ y,
                                                         int64_t N, int d, const double* __restrict__ mu,
                                                         const double* __restrict__ init, const int* __restrict__ perm,
                                                         int n_epochs, int steps, int B, double lr, double wd,
                                                         double* __restrict__ params_out, double* __restrict__ loss_out) {
  __shared__ double sL[MAX_D * MAX_D], smu[MAX_D], sdiff[ELL_ROWS * ELL_DS], su[ELL_ROWS * ELL_DS],
      spart[4][ELL_ROWS], sy[ELL_ROWS], sg[ELL_ROWS], sgm[ELL_ROWS], red[4], s_ab[2];
  constexpr int KP = 3;                                   // ceil(530 / 256)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = blockIdx.x;
  const int T = d * (d + 1) / 2, P = T + 2;
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
  double pv[KP], mv[KP], vv[KP], G[KP];
  int pi[KP], pj[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int p = t + ELL_NT * k;
    pv[k] = p < P ? init[(int64_t)r * P + p] : 0.0;
    mv[k] = vv[k] = G[k] = 0.0;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;             // row of tril index p (only meaningful for p < T)
    pi[k] = i;
    pj[k] = p - i * (i + 1) / 2;
  }
  for (int e = t; e < MAX_D * MAX_D; e += ELL_NT) sL[e] = 0.0;
  if (t < d) smu[t] = mu[t];
  __syncthreads();
  auto publish = [&]() {                                 // theta -> the LDS copy the forward pass reads
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int p = t + ELL_NT * k;
      if (p < T) {
        const double v = pv[k];
        sL[pi[k] * MAX_D + pj[k]] = (pi[k] == pj[k]) ? fmax(v, 0.0) + log1p(exp(-fabs(v))) + 1e-4 : v;
      } else if (p < P) {
        s_ab[p - T] = pv[k];
      }
    }
  };
  publish();
  __syncthreads();
  const int R = steps * B;
  int64_t count = 0;
  for (int ep = 0; ep < n_epochs; ++ep) {
    for (int st = 0; st < steps; ++st) {
      const int* pr = perm + ((int64_t)r * n_epochs + ep) * R + (int64_t)st * B;
      const double alpha = s_ab[0], beta = s_ab[1];
#pragma unroll
      for (int k = 0; k < KP; ++k) G[k] = 0.0;
      for (int b0 = 0; b0 < B; b0 += ELL_ROWS) {
        const int nb = min(ELL_ROWS, B - b0);
        // A: the chunk's rows
        for (int e = t; e < nb * d; e += ELL_NT) {
          const int b = e / d, i = e - b * d;
          const int64_t row = pr[b0 + b];
          sdiff[b * ELL_DS + i] = X[row * d + i] - smu[i];
          if (i == 0) sy[b] = y[row];
        }
        __syncthreads();
        // B: u = L^T diff, split over the waves by column
        if (lane < nb) {
          double part = 0.0;
          for (int j = wave; j < d; j += 4) {
            double u = 0.0;
            for (int i = j; i < d; ++i) u = fma(sL[i * MAX_D + j], sdiff[lane * ELL_DS + i], u);
            su[lane * ELL_DS + j] = u;
            part = fma(u, u, part);
          }
          spart[wave][lane] = part;
        }
        __syncthreads();
        // C: the loss gradient per row
        if (t < nb) {
          const double md2 = ((spart[0][t] + spart[1][t]) + spart[2][t]) + spart[3][t];
          const double logit = fma(-alpha, md2, beta);
          const double g = (1.0 / (1.0 + exp(-logit)) - sy[t]) / (double)B;
          sg[t] = g;
          sgm[t] = g * md2;
        }
        __syncthreads();
        // D: the parameter gradients, rows in ascending order
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const int p = t + ELL_NT * k;
          double acc = G[k];
          if (p < T) {
            const int i = pi[k], j = pj[k];
            for (int b = 0; b < nb; ++b) acc = fma(sdiff[b * ELL_DS + i], sg[b] * su[b * ELL_DS + j], acc);
          } else if (p == T) {
            for (int b = 0; b < nb; ++b) acc += sgm[b];
          } else if (p == T + 1) {
            for (int b = 0; b < nb; ++b) acc += sg[b];
          }
          G[k] = acc;
        }
        if (b0 + ELL_ROWS < B) __syncthreads();         // (the next chunk overwrites the rows)
      }
      // AdamW (optax.adamw: scale_by_adam, add_decayed_weights, scale_by_learning_rate, apply_updates)
      ++count;
      const double bc1 = 1.0 - pow(b1, (double)count), bc2 = 1.0 - pow(b2, (double)count);
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const int p = t + ELL_NT * k;
        if (p < P) {
          double g = G[k];
          if (p < T) {
            g *= -2.0 * alpha;
            if (pi[k] == pj[k]) g *= 1.0 / (1.0 + exp(-pv[k]));
          } else if (p == T) {
            g = -g;
          }
          mv[k] = (1.0 - b1) * g + b1 * mv[k];
          vv[k] = (1.0 - b2) * (g * g) + b2 * vv[k];
          const double mh = mv[k] / bc1, vh = vv[k] / bc2;
          const double upd = mh / (sqrt(vh) + eps) + wd * pv[k];
          pv[k] = pv[k] + (-lr) * upd;
        }
      }
      publish();
      __syncthreads();
    }
  }
  // full-data loss: optax.sigmoid_binary_cross_entropy(logit, y).mean(), log_sigmoid(z) = -softplus(-z); the rows in
  // chunks of 64 through phases A / B (thread b sums rows b, b + 64, ...), then the four waves in order
  const double alpha = s_ab[0], beta = s_ab[1];
  double ls = 0.0;
  for (int64_t b0 = 0; b0 < N; b0 += ELL_ROWS) {
    const int nb = (int)min<int64_t>(ELL_ROWS, N - b0);
    __syncthreads();
    for (int e = t; e < nb * d; e += ELL_NT) {
      const int b = e / d, i = e - b * d;
      sdiff[b * ELL_DS + i] = X[(b0 + b) * d + i] - smu[i];
    }
    __syncthreads();
    if (lane < nb) {
      double part = 0.0;
      for (int j = wave; j < d; j += 4) {
        double u = 0.0;
        for (int i = j; i < d; ++i) u = fma(sL[i * MAX_D + j], sdiff[lane * ELL_DS + i], u);
        part = fma(u, u, part);
      }
      spart[wave][lane] = part;
    }
    __syncthreads();
    if (t < nb) {
      const double md2 = ((spart[0][t] + spart[1][t]) + spart[2][t]) + spart[3][t];
      const double l = fma(-alpha, md2, beta), yn = y[b0 + t];
      const double sp_neg = fmax(-l, 0.0) + log1p(exp(-fabs(l)));     // softplus(-l) = -log_sigmoid(l)
      const double sp_pos = fmax(l, 0.0) + log1p(exp(-fabs(l)));      // softplus(l)  = -log_sigmoid(-l)
      ls += yn * sp_neg + (1.0 - yn) * sp_pos;
    }
  }
  ls = wave_sum(ls);
  if (lane == 0) red[wave] = ls;
  __syncthreads();
  if (t == 0) loss_out[r] = (((red[0] + red[1]) + red[2]) + red[3]) / (double)N;
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int p = t + ELL_NT * k;
    if (p < P) params_out[(int64_t)r * P + p] = pv[k];
  }
}

}  // namespace bobe
