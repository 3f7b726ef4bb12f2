// Diagnostic build of the sweep GEMM (k_trimul) with in-kernel stamps: the clock the chip holds under this loop and where
// a K-step's cycles go.  BOBE_GEMM_STAMPS switches the stamps on in gemm_f64.hpp; the product never defines it.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/bin/gemm_stamps tools/gemm_stamps.hip
//   tools/bin/gemm_stamps [seconds] > profiles/<name>.json
//
// k_trimul at the headline shape (N = 4096: nb = 32 row tiles, a chunk of 8192 candidates, no cross tiles) on random data,
// launched back to back for `seconds` (default 3), then one more launch whose stamps are read.  Per wave: clock =
// d(s_memtime) / d(s_memrealtime) x 100 MHz around the loop; segment cycles per K-step (see gemm_f64.hpp).  The kernel
// runs the direct-to-LDS tile core, the one it ships with; the register-staged core can no longer be stamped through it.
#define BOBE_GEMM_STAMPS 1
#include "../bobe_amd/csrc/sweep_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) {                                                            \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
      std::exit(1);                                                                    \
    }                                                                                  \
  } while (0)

using namespace bobe;

static double run(int nb, int64_t ncols, const double* Li, const double* B, double* V, double* qp, double secs,
                  unsigned long long* st, std::vector<unsigned long long>& host) {
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_trimul), hipFuncAttributeMaxDynamicSharedMemorySize,
                         GEMM_SMEM_BYTES));
  const int64_t Np = (int64_t)nb * TILE;
  const dim3 grid((unsigned)(ncols / TILE), (unsigned)nb);
  auto launch = [&] {
    hipLaunchKernelGGL(k_trimul, grid, dim3(256), GEMM_SMEM_BYTES, 0, Li, Np, nb, B, ncols, V, ncols, qp, ncols,
                       (const double*)nullptr, (int64_t)0, 0, (double*)nullptr, (int64_t)0);
  };
  launch();
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  int n = 0;
  const auto t0 = std::chrono::steady_clock::now();
  CK(hipEventRecord(e0, 0));
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < secs) {
    for (int i = 0; i < 50; ++i) launch();
    n += 50;
    CK(hipDeviceSynchronize());
  }
  CK(hipEventRecord(e1, 0));
  CK(hipMemset(st, 0, host.size() * sizeof(unsigned long long)));
  launch();
  CK(hipDeviceSynchronize());
  CK(hipGetLastError());
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipMemcpy(host.data(), st, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return ms / n;
}

int main(int argc, char** argv) {
  const double secs = argc > 1 ? std::atof(argv[1]) : 3.0;
  const int nb = 32;
  const int64_t ncols = 8192, Np = (int64_t)nb * TILE;
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<double> hL((size_t)Np * Np, 0.0), hB((size_t)Np * ncols);
  for (int64_t i = 0; i < Np; ++i)
    for (int64_t j = 0; j <= i; ++j) hL[i * Np + j] = u(rng);
  for (auto& x : hB) x = u(rng);
  double *Li, *B, *V, *qp;
  unsigned long long* st;
  const size_t nst = (size_t)(ncols / TILE) * nb * 4 * 8;
  CK(hipMalloc(&Li, hL.size() * 8));
  CK(hipMalloc(&B, hB.size() * 8));
  CK(hipMalloc(&V, hB.size() * 8));
  CK(hipMalloc(&qp, (size_t)nb * ncols * 8));
  CK(hipMalloc(&st, nst * 8));
  CK(hipMemcpy(Li, hL.data(), hL.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(B, hB.data(), hB.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &st, sizeof(st)));
  std::vector<unsigned long long> h(nst);
  const double ms = run(nb, ncols, Li, B, V, qp, secs, st, h);
  std::vector<double> clk;
  double seg[4] = {0, 0, 0, 0}, loop = 0, steps = 0;
  for (size_t w = 0; w < nst / 8; ++w) {
    const unsigned long long* o = &h[w * 8];
    if (o[7] != 1 || o[1] == 0) continue;
    clk.push_back((double)o[0] / (double)o[1] * 0.1);           // GHz: s_memrealtime ticks at 100 MHz
    for (int i = 0; i < 4; ++i) seg[i] += (double)o[2 + i];
    loop += (double)o[0];
    steps += (double)o[6];
  }
  std::sort(clk.begin(), clk.end());
  const double med = clk.empty() ? 0.0 : clk[clk.size() / 2];
  std::printf("{\"loop\": \"gemm_tile_glds<128>\", \"stamped_ms_per_launch\": %.4f, \"waves\": %zu, "
              "\"clock_ghz_median\": %.4f, \"clock_ghz_p10\": %.4f, \"clock_ghz_p90\": %.4f, \"cycles_per_kstep\": "
              "{\"first_fragment_wait\": %.1f, \"mfma_body\": %.1f, \"staging_wait\": %.1f, \"barrier\": %.1f, "
              "\"loop_total\": %.1f}}\n",
              ms, clk.size(), med, clk.empty() ? 0.0 : clk[clk.size() / 10], clk.empty() ? 0.0 : clk[clk.size() * 9 / 10],
              seg[0] / steps, seg[1] / steps, seg[2] / steps, seg[3] / steps, loop / steps);
  return 0;
}
