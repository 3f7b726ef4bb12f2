// libbobe_gp.so, factorisation unit: K(X,X) assembly, the blocked Cholesky and its launch plan, the triangular inverse,
// alpha, the marginal likelihood and its gradient (single evaluation, evaluation slots, lock-step batch, graph replay),
// restore of a given factor.  Kernels: kernels_common.hpp, chol_kernels.hpp.
#include "gp_handle.hpp"

#include <chrono>

#include "chol_kernels.hpp"

using namespace bobe;

namespace bobe {

// (SYRK32_BK, SYRK64_BK, SYRK32_SMEM, SYRK64_SMEM: gemm_f64.hpp)
void configure_factor_kernels() {
  static bool done[64] = {false};
  if (!first_use_on_device(done)) return;
  allow_big_lds(k_potf2<true>, POTF2_SMEM_BYTES);
  allow_big_lds(k_potf2<false>, POTF2_SMEM_BYTES);
  allow_big_lds(k_trti_diag, POTF2_SMEM_BYTES);
  allow_big_lds(k_trsm_panel, TRSM_SMEM_BYTES);
  allow_big_lds((k_chol_panel<false, 3>), POTF2_SMEM_BYTES);
  allow_big_lds((k_chol_panel<false, 4>), POTF2_SMEM_BYTES);
  allow_big_lds((k_chol_panel<true, 3>), POTF2_SMEM_BYTES);
  allow_big_lds((k_chol_panel<true, 4>), POTF2_SMEM_BYTES);
  allow_big_lds(k_trtri_T<128>, GEMM_SMEM_BYTES);
  allow_big_lds(k_trtri_R<128>, GEMM_SMEM_BYTES);
  allow_big_lds(k_syrk_trail<64, SYRK64_BK>, SYRK64_SMEM);
  allow_big_lds(k_syrk_trail<32, SYRK32_BK>, SYRK32_SMEM);
  allow_big_lds(k_trtri_T<64>, GEMM64_SMEM_BYTES);
  allow_big_lds(k_trtri_R<64>, GEMM64_SMEM_BYTES);
  allow_big_lds(k_trtri_T<32>, GEMM32_SMEM_BYTES);
  allow_big_lds(k_trtri_R<32>, GEMM32_SMEM_BYTES);
  allow_big_lds(k_lauum_tiles32, GEMM32_SMEM_BYTES);
  for_each_kern_dcap([](auto KE, auto DC) {
    allow_big_lds((k_lauum_grad<KE, DC, 64>), GEMM64_SMEM_BYTES);
    allow_big_lds((k_lauum_grad<KE, DC, 128>), GEMM_SMEM_BYTES);
  });
}

const Tuning& tuning() {
  static Tuning t = [] {
    Tuning v{512, 600, 300, 1, BOBE_MAX_MLL_SLOTS, 2048, 1, 1, 1, false, false, true};
    auto geti = [](const char* name, int& dst) {
      const char* e = std::getenv(name);
      if (e) dst = std::atoi(e);
      return e != nullptr;
    };
    geti("BOBE_SYRK32_BELOW", v.syrk32_below);
    geti("BOBE_TRTRI64", v.trtri64_below);
    geti("BOBE_PAIR_MIN", v.pair_min);
    geti("BOBE_LOCKSTEP_MIN_N", v.lockstep_min_n);
    v.mll_slots_set = geti("BOBE_MLL_SLOTS", v.mll_slots);
    geti("BOBE_GRAPH_MAX_N", v.graph_max_n);
    geti("BOBE_XCD_SHARES", v.xcd_shares);
    geti("BOBE_FILL", v.fill);
    geti("BOBE_INV_SIDE", v.inv_side);
    v.trace = std::getenv("BOBE_TRACE") != nullptr;
    int reuse = 1;
    geti("BOBE_FACTOR_REUSE", reuse);
    v.factor_reuse = reuse != 0;
    return v;
  }();
  return t;
}

double default_refine_kappa() {
  static const double v = [] {
    const char* e = std::getenv("BOBE_REFINE_KAPPA");
    return e ? std::atof(e) : 1e6;
  }();
  return v;
}

int default_solve_block() {
  static const int v = [] {
    const char* e = std::getenv("BOBE_SOLVE_BLOCK");
    const int b = e ? std::atoi(e) : TILE;
    return b > 0 ? (b + TILE - 1) / TILE * TILE : TILE;
  }();
  return v;
}

int default_solve_panel() {
  static const int v = [] {
    const char* e = std::getenv("BOBE_SOLVE_PANEL");
    const int b = e ? std::atoi(e) : 512;
    return b > 0 ? (b + TILE - 1) / TILE * TILE : 512;
  }();
  return v;
}

int64_t default_solve_chunk() {
  static const int64_t v = [] {
    const char* e = std::getenv("BOBE_SOLVE_CHUNK");
    const int64_t c = e ? std::atoll(e) : 32768;       // (K(X, chunk) and V: 1 GiB each at N = 4096)
    return c > 0 ? (c + TILE - 1) / TILE * TILE : 0;
  }();
  return v;
}

double default_pivot_floor_ulp() {
  static const double v = [] {
    const char* e = std::getenv("BOBE_PIVOT_FLOOR_ULP");
    if (!e) return 0.0;
    const double u = std::atof(e);
    return u >= 0.0 ? u : 0.0;
  }();
  return v;
}

}  // namespace bobe

void bobe_gp::build_probs() {
  const TriSplit sp = tri_split(nb);
  depths = sp.depths;
  lead_depths = sp.lead;
  trail_depths = sp.trail;
  tri_mid = sp.mid;
  if (!sp.table.empty()) {
    probs.ensure(sp.table.size() * sizeof(TriProb));
    HIPCHK(hipMemcpy(probs.p, sp.table.data(), sp.table.size() * sizeof(TriProb), hipMemcpyHostToDevice));
  }
}

void bobe_gp::alloc_for_n() {
  own.ensure(*this, 1);
  const size_t mat = (size_t)Np * Np * sizeof(double);
  const size_t vec = (size_t)Np * sizeof(double);
  A.ensure(mat);
  Linv.ensure(mat);
  Tmp.ensure(mat);
  y.ensure(vec);
  alpha.ensure(vec);
  w.ensure(vec);
  XsT.ensure((size_t)d * vec);
  const int64_t pw = Np > chunk ? Np : chunk;        // (the sweep's partial sums: a chunk wide)
  part.ensure((size_t)nb * pw * sizeof(double));
  gpart.ensure((size_t)own.gps() * sizeof(double));   // (kinv_debug's lauum)
  res.ensure(128 * sizeof(double));
  info.ensure(sizeof(int));
  diag.ensure((size_t)nb * TILE * TILE * sizeof(double));
  build_probs();
  build_plans();
  forget_evals();
}

// Room for B members at the handle's current sizes.  The only place that knows what an evaluation workspace is made of.
void bobe_gp::EvalWs::ensure(const bobe_gp& g, int B) {
  if (!h_res) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h_res), (size_t)width * (128 * sizeof(double) + sizeof(Hyper)),
                         hipHostMallocDefault));
    h_hyp = reinterpret_cast<Hyper*>(h_res + (size_t)width * 128);
  }
  if (B > cap || g.Np != Np) {            // (buffers reallocated or their member stride changed)
    for (bobe::EvalTag& t : tag) t.clear();
    cap = g.Np != Np ? B : std::max(cap, B);
  }
  Np = g.Np;
  nb = g.nb;
  d = g.d;
  const size_t n = (size_t)B * sizeof(double);
  A.ensure(n * mat());
  Linv.ensure(n * mat());
  Tmp.ensure(n * mat());
  XsT.ensure(n * xs());
  w.ensure(n * vec());
  alpha.ensure(n * vec());
  part.ensure(n * prt());
  gpart.ensure(n * gps());
  res.ensure(n * 128);
  diag.ensure(n * nb * TILE * TILE);
  loo.ensure(n * lvs());
  info.ensure((size_t)width * sizeof(int));
  hyp.ensure((size_t)width * sizeof(Hyper));
}

void bobe_gp::EvalWs::release() {
  for (DBuf* b : {&XsT, &A, &Linv, &Tmp, &w, &alpha, &part, &gpart, &res, &info, &diag, &hyp, &loo}) b->release();
  for (hipGraphExec_t& e : eg.exec) {
    if (e) (void)hipGraphExecDestroy(e);
    e = nullptr;
  }
  if (h_res) (void)hipHostFree(h_res);
  h_res = nullptr;
  h_hyp = nullptr;
  if (ev) (void)hipEventDestroy(ev);
  ev = nullptr;
}

void bobe_gp::scale(const double* in, int64_t n, int64_t npad, const Hyper& h, double* out, int64_t ldo,
                    const Hyper* hdev, int B, int64_t bsO, int* info_reset) {
  hipLaunchKernelGGL(k_scale_coords, dim3((unsigned)((npad + 255) / 256), (unsigned)B), dim3(256), 0, stream, in, n, npad,
                     h, out, ldo, hdev, bsO, info_reset);
  LAUNCH_CHECK();
}

// k_kernel_matrix<KE, SQ, DC, EXACT> (SQ: the symmetric form K(X, X); EXACT: d fills the cap DC) on `stream`
template <bool SQ, typename KE, typename DC, typename... Args>
static void launch_kernel_matrix(KE, DC, int d, dim3 grid, hipStream_t stream, Args... args) {
  auto kernel = d == DC::value ? k_kernel_matrix<KE::value, SQ, DC::value, true>
                               : k_kernel_matrix<KE::value, SQ, DC::value, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, args...);
}

void bobe_gp::kernel_matrix_cross(const double* AT, int64_t lda, int64_t na, int64_t napad, const double* BT,
                                  int64_t ldb, int64_t nbv, int64_t nbpad, const Hyper& h, double* out, int64_t ldo,
                                  const double* wv, double* prt, int64_t ldp) {
  const dim3 grid((unsigned)(nbpad / TILE), (unsigned)(napad / TILE));
  auto launch = [&](auto KE, auto DC) {
    launch_kernel_matrix<false>(KE, DC, h.d, grid, stream, AT, lda, na, BT, ldb, nbv, h, out, ldo, (const Hyper*)nullptr,
                                (int64_t)0, (int64_t)0, wv, prt, ldp);
  };
  if (h.kern == 2)                       // dist_sq (kernel_eval): the squared distance itself, this cross form only
    with_dcap(h.d, [&](auto DC) { launch(std::integral_constant<int, 2>{}, DC); });
  else
    with_kern_dcap(h.kern, h.d, launch);
  LAUNCH_CHECK();
}

void bobe_gp::assemble_kxx(const Hyper& h, const FactorBufs& f, const Hyper* hdev) {
  const dim3 grid((unsigned)(2 * nb * (nb + 1)), (unsigned)f.B);   // four workgroups per lower 128x128 tile
  prof_begin(BOBE_PROF_KXX);
  with_kern_dcap(h.kern, h.d, [&](auto KE, auto DC) {
    launch_kernel_matrix<true>(KE, DC, h.d, grid, stream, (const double*)f.xst, Np, N, (const double*)f.xst, Np, N, h, f.a,
                               Np, hdev, f.xs, f.mat, (const double*)nullptr, (double*)nullptr, (int64_t)0);
  });
  prof_end(BOBE_PROF_KXX);
  LAUNCH_CHECK();
}

// Trailing update with the panels of 128-blocks [k0, k1): colmode 0 = every lower tile from 128-block `first`
// on, colmode 1 = only 128-block column `first` (rows from `first` down).  A tile's time is set by its MFMAs
// per wave (512 / 128 / 32 per 128 of K): small trailing matrices take the smallest tile that still fills the
// chip, large ones the cheapest by a rounds x tile-time estimate.  (Tile shape does not change the bits: every
// element accumulates its K range in the same order, four k per MFMA.)
// colk0 (device table, one entry per block column): the columns of the launch start at different panels (deferred
// columns, see potrf) - 64 x 64 tiles only.
void bobe_gp::syrk(const FactorBufs& f, int k0, int k1, int first, int colmode, const int* colk0, int far_col, int ncols) {
  const Tuning& tu = tuning();
  const int B = f.B;
  const int rem = nb - first;                 // 128-blocks in the trailing matrix
  if (rem <= 0 || (!colk0 && k1 <= k0)) return;
  const int kb = k1 - k0;
  const int n64 = 2 * rem, n32 = 4 * rem;
  // colmode 2: only the first `ncols` block columns of the trailing matrix take part (the rest is deferred)
  const int nc64 = 2 * ncols;
  const int t64 = colmode == 2 ? nc64 * n64 - nc64 * (nc64 - 1) / 2 : (colmode ? 2 * n64 - 1 : n64 * (n64 + 1) / 2);
  const int t32 = colmode ? 4 * n32 - 6 : n32 * (n32 + 1) / 2;
  // 64x64 tiles with BK = 16 (36 KB of LDS, four workgroups per CU) have the best saturated throughput of all
  // variants at every K (profiles/r02_a_ubench_update_variants.txt); when they would leave most of the chip idle, a single-panel
  // update takes 32x32 tiles, which stage the whole K = 128 panel in one LDS buffer
  if (kb == 1 && !colk0 && colmode != 2 && B * t64 < tu.syrk32_below) {
    hipLaunchKernelGGL((k_syrk_trail<32, SYRK32_BK>), dim3(t32, B), dim3(256), SYRK32_SMEM, stream, f.a, Np, k0, k1, first,
                       colmode, n32, f.mat, 0, (const int*)nullptr, 0, 0);
    return;
  }
  const TileGrid tg = colmode ? TileGrid{t64, 0} : tile_grid(t64);
  hipLaunchKernelGGL((k_syrk_trail<64, SYRK64_BK>), dim3(tg.grid, B), dim3(256), SYRK64_SMEM, stream, f.a, Np, k0, k1, first,
                     colmode, n64, f.mat, tg.per, colk0, far_col, nc64);
}

int bobe_gp::panel_strips(int B, int rr) const {
  // three 16-row strips per panel workgroup wherever the launch still fits the chip (a third more workgroups), else four
  return B * panel_workgroups(rr, 3) <= std::max(num_cus, 1) ? 3 : 4;
}

// Where deferred updates in the panel launches pay.  Measured on 256 CUs (profiles/r04_fill_rule.txt: a lone
// factorisation, fillers forced on / off): N = 2048 1.008, 2560 0.990, 3072 1.017, 3584 0.989, 3840 0.974, 4096 0.965,
// 4352 0.966, 4608 1.040, 4992 1.136, 5120 1.140, 6144 1.157, 8192 1.066.  They pay in a narrow band: the matrix must have
// enough block columns for the update launches to be worth replacing (below ~28 they last a few microseconds each and the
// difference is inside the noise), and the FIRST panel launch - the widest - must leave about two thirds of the chip free
// (from 36 block columns up it occupies 94+ of 256 CUs, whole block columns of update tiles no longer fit beside the chain,
// a filler workgroup runs the tile core at ~3/4 of its usual rate and every launch lasts as long as its slowest filler).
// Hence: nb >= 28 and B * (panel workgroups of step 0) <= 35 % of the CUs - on 256 CUs a lone factorisation of 28 ... 34
// block columns (N = 3457 ... 4352), never a lock-step batch (B >= 2 fails the second test for every nb >= 28).  Never on
// an evaluation slot's private stream, where the other slots' kernels want those CUs.  BOBE_FILL=2 forces the fillers on
// everywhere, BOBE_FILL=0 off.
bool bobe_gp::fill_pays(int B) const {
  const int f = tuning().fill;
  if (f == 0 || on_slot()) return false;
  if (f == 2) return true;
  return nb >= 28 && 20 * B * panel_workgroups(nb - 1, panel_strips(B, nb - 1)) <= 7 * std::max(num_cus, 1);
}

// The launch plan of a factorisation of B matrices in lock step (see potrf).  Block columns >= far_start are DEFERRED:
// the update launches leave them alone until they are about to be factored (the last FILL_NEAR panels of a column
// always come from the update launches), and the panel launches carry their pending updates as filler workgroups on the
// CUs the panel workgroups do not occupy - whole block columns at a time, FILL_CHUNK panels per visit (a filler must
// not outlast the panel, ~28 us), earliest deadline first.  far_start is the smallest column from which the fillers keep
// up (what they leave behind is caught up by the update launch that makes the column current, with a longer K range).
const bobe_gp::CholPlan& bobe_gp::chol_plan(int B, bool fill) {
  const Tuning& tu = tuning();
  const uint64_t key = ((uint64_t)nb << 32) | ((uint64_t)B << 8) | (fill ? 1u : 0u);
  auto it = chol_plans.find(key);
  if (it != chol_plans.end()) return it->second;
  const int ncu = std::max(num_cus, 1);
  constexpr int D = FILL_NEAR, CH = FILL_CHUNK;
  auto npanel = [&](int k) { return panel_workgroups(nb - 1 - k, panel_strips(B, nb - 1 - k)); };
  auto one_launch = [&](int k) { return B * npanel(k) <= ncu; };
  auto tiles_of = [&](int c) { return 4 * (nb - c) - 1; };   // 64 x 64 tiles of block column c from its diagonal block down

  auto build = [&](int far, CholPlan* out) {
    std::vector<int> applied(nb, 0);
    int64_t deferred = 0, catchup = 0, total = 0;
    auto panel = [&](int k) {
      CholOp op{0, k, k, out ? (int)out->jobs.size() : 0, 0, 0, 0, true, k, k};
      const int64_t remk = nb - 1 - k;
      int cap = one_launch(k) ? (ncu - B * npanel(k)) / B : 0;   // filler workgroups per slot, two jobs each
      if (fill && far < nb && cap > 0 && (int64_t)B * remk * remk <= FILL_PHASE) {
        for (int c = std::max(far, k + 2); c < nb && cap > 0; ++c) {     // earliest deadline first
          const int pend = std::min(k, c - D);                           // panels < k are final; the last D are never deferred
          if (applied[c] >= pend) continue;
          const int k1 = std::min(applied[c] + CH, pend);
          const int need = (tiles_of(c) + 1) / 2;
          if (need > cap) continue;
          cap -= need;
          deferred += (int64_t)tiles_of(c) * (k1 - applied[c]);
          if (out) {
            for (int tj = 2 * c; tj <= 2 * c + 1; ++tj)
              for (int ti = tj; ti < 2 * nb; ++ti) out->jobs.push_back({ti, tj, 2 * applied[c], 2 * k1, 0, 0});
            FillJob twin = out->jobs.back();                             // an odd count: a twin that is computed, not stored,
            twin.flags |= FILL_TWIN;                                     // keeps the two groups of a workgroup in step
            out->jobs.push_back(twin);
            op.tab_cnt += tiles_of(c) + 1;
          }
          applied[c] = k1;
        }
      }
      if (out) out->ops.push_back(op);
    };
    auto update = [&](int kind, int first, int k1, int last_near, int newest) {
      // columns taking part: the block column `first` alone (narrow) or every column from `first` on that is not deferred
      // or is within FILL_NEAR panels of being factored (c <= last_near)
      CholOp op{kind, k1, first, out ? (int)out->colk0.size() : 0, nb, INT_MAX, INT_MIN, true, first, k1};
      std::vector<int> tab(nb, k1);
      const int cend = kind == 1 ? first + 1 : nb;
      for (int c = first; c < cend; ++c) {
        const bool active = c < far || c <= last_near;
        if (!active) { op.uniform = false; continue; }
        tab[c] = applied[c];
        op.last_active = c;
        if (c < far) op.k0_plain = applied[c];
        op.k0_min = std::min(op.k0_min, applied[c]);
        op.k0_max = std::max(op.k0_max, applied[c]);
        total += (int64_t)tiles_of(c) * (k1 - applied[c]);
        if (c >= far) catchup += (int64_t)tiles_of(c) * std::max(0, (k1 - applied[c]) - newest);   // beyond the newest panel(s)
        applied[c] = k1;
      }
      if (op.k0_min != op.k0_max) op.uniform = false;
      if (op.k0_min == INT_MAX) return;                                   // nothing to do
      if (out) {
        out->colk0.insert(out->colk0.end(), tab.begin(), tab.end());
        out->ops.push_back(op);
      }
    };
    for (int k = 0; k < nb;) {
      const int rem = nb - 1 - k;
      panel(k);
      // Update-bound steps go in PAIRS: panel k, block column k+1 <- its pending panels (narrow), panel k+1, then ONE
      // trailing pass with both panels (K = 256): half the passes over the trailing matrix and a tile kernel that runs
      // 15 % faster at K = 256 than at 128, for one narrow launch more on the chain.  Same bits (every element still
      // receives panel k before panel k+1).
      if (tu.pair_min > 0 && rem >= 2 && (int64_t)B * rem * rem > tu.pair_min) {
        update(1, k + 1, k + 1, nb, 1);
        panel(k + 1);
        update(2, k + 2, k + 2, k + 1 + D, 2);
        k += 2;
      } else {
        if (rem > 0) update(2, k + 1, k + 1, k + D, 1);
        k += 1;
      }
    }
    if (out) {
      out->far_start = far;
      out->deferred_units = deferred;
      out->catchup_units = catchup;
      out->total_units = total + deferred;
    }
    return std::make_pair(deferred, catchup);
  };
  int far = nb;
  if (fill) {
    for (int f = 1; f < nb; ++f) {
      const auto dc = build(f, nullptr);
      if (dc.first > 0 && dc.second * FILL_SLACK <= dc.first) { far = f; break; }
    }
  }
  CholPlan& pl = chol_plans[key];
  build(far, &pl);
  for (const FillJob& j : pl.jobs)             // (the tables drive device addresses: check them on the host)
    if (!(j.ti >= j.tj && j.ti < 2 * nb && j.tj >= 0 && j.k0 >= 0 && j.k1 > j.k0 && j.k1 <= j.tj - (j.tj & 1)))
      throw Err(BOBE_ERR_STATE, "internal error: filler job outside the matrix");
  if (!pl.jobs.empty()) {
    pl.d_jobs.ensure(pl.jobs.size() * sizeof(FillJob));
    HIPCHK(hipMemcpy(pl.d_jobs.p, pl.jobs.data(), pl.jobs.size() * sizeof(FillJob), hipMemcpyHostToDevice));
  }
  bool need_tab = false;                      // (a plan without deferred columns needs no device table: its launches are uniform)
  for (const CholOp& op : pl.ops) need_tab = need_tab || (op.kind != 0 && !op.uniform);
  if (need_tab) {
    pl.d_colk0.ensure(pl.colk0.size() * sizeof(int));
    HIPCHK(hipMemcpy(pl.d_colk0.p, pl.colk0.data(), pl.colk0.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  if (tu.trace)
    std::fprintf(stderr, "[bobe] chol plan nb=%d B=%d fill=%d: deferred columns from %d, %lld of %lld tile-panels in fillers, "
                 "%lld caught up (%zu jobs)\n", nb, B, (int)fill, pl.far_start, (long long)pl.deferred_units,
                 (long long)pl.total_units, (long long)pl.catchup_units, pl.jobs.size());
  return pl;
}

// The plans the evaluation paths will ask for, built where allocation is allowed (a plan uploads its tables with
// hipMalloc + a synchronous copy: not on the evaluation path, and never while a slot's stream is capturing a graph)
void bobe_gp::build_plans() {
  if (nb <= 0) return;
  (void)chol_plan(1, false);
  if (fill_pays(1)) (void)chol_plan(1, true);
}

// Blocked right-looking Cholesky (NB = 128) of B matrices in lock step on one stream; every launch carries the slot
// in its last grid dimension.  Per step k:
//   panel k   diagonal factor + solve of the rows below.  One launch (k_chol_panel: every 48- or 64-row workgroup factors
//             the diagonal block itself) while all B * npanel workgroups fit on the chip at once, else the
//             k_potf2 + k_trsm_panel pair (one factorisation per slot).
//   update    A22 -= L21 L21^T on the lower tiles (k_syrk_trail).
//             Update-bound steps go in pairs: one K = 256 pass for two panels (chol_plan).
// A batch shares the latency-bound panel chain (32 x ~27 us at N = 4096, the same for 1 or 8 matrices) and gives the
// update 4-8x the tiles: 44 % of the fp64 MFMA peak with four in flight, 50 % with eight, against 21 % alone and 28 %
// for four on private streams (whose 150 KB-LDS panel kernels wait for a CU the others' update tiles keep occupied).
// The panel launches leave most of the chip empty (one 150 KB workgroup per 48 / 64 rows): where that pays (fill_pays),
// updates of block columns that are not needed soon are DEFERRED and ride in those launches as filler workgroups
// (chol_plan, k_chol_panel<true, .>).  Every matrix element sees the same operation sequence in all forms (same bits).
// potrf_ops launches the ops [op_begin, op_end) of the plan - a linear list, which chol_solve cuts where it forks the
// inverse - and potrf the whole of it.  The k_chol_panel steps leave their L_kk in the scratch blocks f.diag: `aside`.
void bobe_gp::potrf_ops(const FactorBufs& f, const CholPlan& pl, size_t op_begin, size_t op_end, Aside& aside) {
  const int B = f.B;
  const int64_t bsD = (int64_t)nb * TILE * TILE;              // (f.diag: scratch for the L_kk of the panel launches)
  const FillJob* jobs = static_cast<const FillJob*>(pl.d_jobs.p);
  const int* coltab = static_cast<const int*>(pl.d_colk0.p);
  for (size_t i = op_begin; i < op_end; ++i) {
    const CholOp& op = pl.ops[i];
    if (op.kind == 0) {
      const int kk = op.k;
      const int rr = nb - 1 - kk;
      const int strips = panel_strips(B, rr);
      const int np_ = panel_workgroups(rr, strips);
      const int nv = (int)std::min<int64_t>(TILE, N - (int64_t)kk * TILE);
      if (B * np_ <= std::max(num_cus, 1)) {
        aside.first = std::min(aside.first, kk);              // (this step's L_kk stays in the scratch blocks)
        auto panel = [&](auto FILLV, int gridx, const FillJob* jb, int njobs) {
          const auto kern = strips == 3 ? k_chol_panel<decltype(FILLV)::value, 3> : k_chol_panel<decltype(FILLV)::value, 4>;
          hipLaunchKernelGGL(kern, dim3(gridx, B), dim3(PANEL_THREADS), POTF2_SMEM_BYTES, stream, f.a, Np, f.mat, f.linv, Np,
                             f.mat, kk, np_, f.info, nv, f.diag, bsD, jb, njobs, rr * TILE);
        };
        prof_begin(BOBE_PROF_POTF2);
        if (op.tab_cnt > 0) panel(std::true_type{}, np_ + op.tab_cnt / 2, jobs + op.tab_off, op.tab_cnt);
        else panel(std::false_type{}, np_, nullptr, 0);
        prof_end(BOBE_PROF_POTF2);
      } else {
        prof_begin(BOBE_PROF_POTF2);
        hipLaunchKernelGGL(k_potf2<true>, dim3(B), dim3(256), POTF2_SMEM_BYTES, stream, f.a, Np, f.linv, Np, kk, f.info, nv,
                           f.mat, f.mat);
        prof_end(BOBE_PROF_POTF2);
        if (rr > 0) {
          prof_begin(BOBE_PROF_TRSM);
          hipLaunchKernelGGL(k_trsm_panel, dim3(2 * rr, B), dim3(256), TRSM_SMEM_BYTES, stream, f.a, Np,
                             (const double*)f.linv, Np, kk, f.mat, f.mat);
          prof_end(BOBE_PROF_TRSM);
        }
      }
    } else {
      prof_begin(BOBE_PROF_SYRK);
      if (op.uniform) {
        syrk(f, op.k0_min, op.k, op.first, op.kind == 1 ? 1 : 0);
      } else {
        // (columns before far_start share one first panel and take it as a scalar; deferred ones read the table.  A launch
        // whose active columns are few enumerates just those)
        const int ncols = op.last_active - op.first + 1;
        const bool few = ncols <= 8 && ncols < nb - op.first;
        syrk(f, op.k0_plain, op.k, op.first, few ? 2 : 0, coltab + op.tab_off, pl.far_start, few ? ncols : 0);
      }
      prof_end(BOBE_PROF_SYRK);
    }
  }
  LAUNCH_CHECK();
}

bobe_gp::Aside bobe_gp::potrf(const FactorBufs& f, bool defer_diag) {
  const CholPlan& pl = chol_plan(f.B, fill_pays(f.B));
  Aside aside{nb, f.diag};
  potrf_ops(f, pl, 0, pl.ops.size(), aside);
  if (defer_diag) return aside;
  // (the scratch blocks of the k_chol_panel steps; k_potf2 steps wrote in place, and come first:
  // B * npanel and rem only shrink with k)
  if (aside.first < nb) {
    hipLaunchKernelGGL(k_copy_diag, dim3(nb - aside.first, f.B), dim3(256), 0, stream, f.a, Np, f.mat, aside.dg,
                       (int64_t)nb * TILE * TILE, aside.first);
    LAUNCH_CHECK();
  }
  return no_aside();
}

// One level of the recursive doubling (or the leading / trailing part of one): the problems of `part`, k_trtri_T and / or
// k_trtri_R.  level_blocks: the 128-blocks of the WHOLE level, which pick the tile size - a part of a level takes the tiles
// the level would (the bits do not depend on them; a timing comparison should not mix two changes).
void bobe_gp::trtri_level(const FactorBufs& f, const Depth& part, int level_blocks, bool do_t, bool do_r, hipStream_t st) {
  const Tuning& tu = tuning();
  const TriProb* pr = static_cast<const TriProb*>(probs.p) + part.first;
  // (64x64 tiles while a level of ONE matrix has too few 128x128 tiles to fill the chip; a tile's K order is the
  // same either way.  Batches keep the per-matrix choice: four in lock step at N = 4096 take 7.0 ms per evaluation
  // round with 64x64 tiles at every level against 7.4 with 128x128 tiles at the top level)
  if (f.B * 2 * level_blocks <= std::max(num_cus, 1)) {
    // A level with fewer 64 x 64 tile pairs than CUs (N <= 1024 in a batch of four, the deep levels of larger
    // matrices): 32 x 32 tiles - four times the workgroups, a quarter of the work each.  Such a launch lasts as long as
    // ONE workgroup's K loop, and a wave issues a 16 x 16 x 4 fp64 MFMA every 64 cycles at best: a quarter of the MFMAs
    // per wave and K-step is a shorter launch.  Tile shape does not change an element's accumulation order (same bits).
    const TileGrid tg = tile_grid(8 * part.nblocks);
    if (do_t)
      hipLaunchKernelGGL(k_trtri_T<32>, dim3(tg.grid, f.B), dim3(256), GEMM32_SMEM_BYTES, st, f.a, Np,
                         (const double*)f.linv, Np, f.tmp, Np, pr, part.count, f.mat, f.mat, f.mat, tg.per);
    if (do_r)
      hipLaunchKernelGGL(k_trtri_R<32>, dim3(tg.grid, f.B), dim3(256), GEMM32_SMEM_BYTES, st, f.linv, Np,
                         (const double*)f.tmp, Np, pr, part.count, f.mat, f.mat, tg.per);
  } else if (level_blocks < tu.trtri64_below) {
    const TileGrid tg = tile_grid(2 * part.nblocks);             // (tile pairs of complementary K: equal work)
    if (do_t)
      hipLaunchKernelGGL(k_trtri_T<64>, dim3(tg.grid, f.B), dim3(256), GEMM64_SMEM_BYTES, st, f.a, Np,
                         (const double*)f.linv, Np, f.tmp, Np, pr, part.count, f.mat, f.mat, f.mat, tg.per);
    if (do_r)
      hipLaunchKernelGGL(k_trtri_R<64>, dim3(tg.grid, f.B), dim3(256), GEMM64_SMEM_BYTES, st, f.linv, Np,
                         (const double*)f.tmp, Np, pr, part.count, f.mat, f.mat, tg.per);
  } else {
    if (do_t)
      hipLaunchKernelGGL(k_trtri_T<128>, dim3(part.nblocks, f.B), dim3(256), GEMM_SMEM_BYTES, st, f.a, Np,
                         (const double*)f.linv, Np, f.tmp, Np, pr, part.count, f.mat, f.mat, f.mat);
    if (do_r)
      hipLaunchKernelGGL(k_trtri_R<128>, dim3(part.nblocks, f.B), dim3(256), GEMM_SMEM_BYTES, st, f.linv, Np,
                         (const double*)f.tmp, Np, pr, part.count, f.mat, f.mat);
  }
}

// Linv = L^-1, or one part of it, on the stream `st`: the diagonal 128-blocks of the part in one batched launch, then
// recursive doubling (two GEMM launches per level).  TRI_LEAD ends with the top problem's T, TRI_TOP_R is its R alone.
// (prof_begin / prof_end record on the handle's stream.  They fire only while the inverse is timed as a class, and then
// inv_side_pays keeps the fork off: st is the handle's stream whenever they do.)
void bobe_gp::trtri_part(TriPart part, const FactorBufs& f, Aside aside, hipStream_t st) {
  const int b0 = part == TRI_TRAIL ? tri_mid : 0, b1 = part == TRI_LEAD ? tri_mid : nb;
  if (part != TRI_TOP_R) {
    prof_begin(BOBE_PROF_TRTRI);
    hipLaunchKernelGGL(k_trti_diag, dim3(b1 - b0, f.B), dim3(256), POTF2_SMEM_BYTES, st, f.a, Np, f.linv, Np, f.mat, f.mat,
                       aside.dg, (int64_t)nb * TILE * TILE, aside.first, b0);
    prof_end(BOBE_PROF_TRTRI);
  }
  for (int dd = (int)depths.size() - 1; dd >= 0; --dd) {
    const Depth& D = depths[dd];
    if (part != TRI_ALL && dd > 0) {
      const Depth& P = part == TRI_LEAD ? lead_depths[dd] : trail_depths[dd];
      if (part != TRI_TOP_R && P.count > 0) trtri_level(f, P, D.nblocks, true, true, st);
      continue;
    }
    if (part == TRI_TRAIL) continue;
    prof_begin(BOBE_PROF_TRTRI);
    trtri_level(f, D, D.nblocks, part != TRI_TOP_R, part != TRI_LEAD, st);
    prof_end(BOBE_PROF_TRTRI);
  }
  LAUNCH_CHECK();
}

// K^-1 tiles fused with the gradient partial sums (into f.gpart); returns #partials.  store_kinv: K^-1's lower tiles are
// stored to f.tmp (every member's: the LOO objective; kinv_debug).  Else f.tmp is scratch: small launches - fewer 64 x 64
// tiles than four per CU - form K^-1 on 32 x 32 tiles into it first (k_lauum_tiles) and run the gradient epilogue from
// there: N = 1024 in a batch of four, 77 -> 36 us (the fused launch is as long as its longest tile, K = 1024 on one CU).
// Same partial sums, same bits.
int bobe_gp::lauum(const Hyper& h, const FactorBufs& f, const Hyper* hdev, bool store_kinv) {
  // (the tile size fixes the order of the gradient's partial sums: it depends on N only, so that an evaluation
  // returns the same bits alone, on a slot and in a batch)
  const LauumTiling t = lauum_tiling(nb);
  const int ntiles = t.ntiles, B = f.B;
  const bool split = t.small && !store_kinv && B * ntiles < 4 * std::max(num_cus, 1);
  double* kio = split || store_kinv ? f.tmp : nullptr;
  prof_begin(BOBE_PROF_LAUUM);
  if (split) {
    hipLaunchKernelGGL(k_lauum_tiles32, dim3(4 * ntiles * B), dim3(256), GEMM32_SMEM_BYTES, stream, (const double*)f.linv, Np,
                       Np, f.tmp, Np, f.mat, f.mat, B);
  }
  with_lauum_variant(h.kern, h.d, t, [&](auto KE, auto DC, auto TT) {
    hipLaunchKernelGGL((k_lauum_grad<KE, DC, TT>), dim3(ntiles * B), dim3(256),
                       (TT == 128 ? GEMM_SMEM_BYTES : GEMM64_SMEM_BYTES), stream, (const double*)f.linv, Np, Np, N,
                       (const double*)f.alpha, (const double*)f.xst, Np, h, f.gpart, kio, Np, hdev, f.mat, f.vec, f.xs, f.gps,
                       B, split ? 1 : 0, kio ? f.mat : (int64_t)0);
  });
  prof_end(BOBE_PROF_LAUUM);
  LAUNCH_CHECK();
  return ntiles;
}

void bobe_gp::solve_alpha(const double* linv, double* wv, double* al, double* prt, int B, int64_t bsL, int64_t bsV,
                          int64_t bsP, const double* rhs, int64_t bsY) {
  hipLaunchKernelGGL(k_gemv_lower, dim3((unsigned)(Np / 4), (unsigned)B), dim3(256), 0, stream, linv, Np, Np,
                     rhs ? rhs : (const double*)y.d(), wv, bsL, bsV, rhs ? bsY : (int64_t)0);
  hipLaunchKernelGGL(k_gemv_t_part, dim3((unsigned)(Np / 64), (unsigned)nb, (unsigned)B), dim3(256), 0, stream, linv, Np, 1,
                     (const double*)wv, prt, Np, bsL, bsV, bsP);
  hipLaunchKernelGGL(k_colsum_parts, dim3((unsigned)((Np + 255) / 256), (unsigned)B), dim3(256), 0, stream,
                     (const double*)prt, Np, nb, 1, Np, al, bsP, bsV);
  LAUNCH_CHECK();
}

// Where the inverse's leading half goes to the side stream (chol_solve).  Measured on 256 CUs, one evaluation round
// (value + gradient) forked / unforked (profiles/inverse_side_stream_ab.txt):
//            B = 1    B = 4    B = 8
//   N = 2048  0.993    0.964    0.973        (nb = 16)
//       3072  0.935    0.939    0.957        (nb = 24)
//       4096  0.980    0.947    0.989        (nb = 32)
//       6144  0.926    0.962    0.986        (nb = 48)
//       8192  0.950    1.004    1.020        (nb = 64)
// The window it fills - panels mid .. nb-1 and their updates - grows with the chain (nb launches) and its updates; the work
// it moves, the leading half's inverse and the top level's T, grows as B * nb^3 and runs on three quarters of the chip
// (ensure_side).  Beyond B * nb^3 ~ 900 000 (between 8 x 48^3 and 4 x 64^3) the side stream outlasts the window and the
// top level's R waits for it: unforked there.  Below 16 block columns nothing was measured: unforked (an evaluation of a
// few hundred microseconds has no window worth a cross-stream hop of ~15 us).  Never on an evaluation slot's private stream
// (the other slots' kernels want those CUs), never under graph capture (a captured pipeline keeps one stream), never while
// the inverse's launches are timed as a class (prof_begin / prof_end bracket launches on one stream).  BOBE_INV_SIDE=2
// forces the fork wherever there are two block columns, BOBE_INV_SIDE=0 turns it off.
bool bobe_gp::inv_side_pays(int B) const {
  const int f = tuning().inv_side;
  if (f == 0 || nb < 2 || on_slot() || capturing || prof_tag == BOBE_PROF_TRTRI) return false;
  if (f == 2) return true;
  return nb >= 16 && (int64_t)B * nb * nb * nb <= 900000;
}

// The side stream and its two events, on first use.  Placement (profiles/inverse_side_stream_ab.txt): a plain or a
// low-priority stream gains 1-2 % per round and never loses, but its 36 KB GEMM workgroups keep refilling every CU and the
// 150 KB panel workgroups of the chain wait for a whole one; a stream confined to three quarters of the CUs
// (hipExtStreamCreateWithCUMask, the first 3/4 of the mask's bits) leaves the chain CUs of its own and gains 2-7 %; half the
// CUs is too few (the join waits), 7/8 gains less at N = 4096.  Without the entry point: a plain stream.
void bobe_gp::ensure_side() {
  if (side_stream) return;
  if (!ev_fork) HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
  if (!ev_join) HIPCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
  const int words = (num_cus + 31) / 32;
  std::vector<uint32_t> mask(words, 0u);
  for (int c = 0; c < 3 * num_cus / 4; ++c) mask[c / 32] |= (1u << (c % 32));
  hipStream_t st = nullptr;
  if (num_cus < 4 || hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask.data()) != hipSuccess) {
    (void)hipGetLastError();
    st = nullptr;
  }
  if (!st) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  side_stream = st;
}

// potrf, the inverse, w / alpha.  Where it pays (inv_side_pays) the inverse's leading half leaves the critical path: the
// plan's op list is cut one past panel mid - 1, the side stream is forked off between the two ranges and gets TRI_LEAD with
// what is aside so far; the handle's stream finishes the factorisation, inverts the trailing half, waits for the side
// stream and closes with the top level's R.  The same launches on the same data in an order every element's dependencies
// allow: the same bits.
void bobe_gp::chol_solve(const FactorBufs& f, const double* rhs) {
  if (inv_side_pays(f.B)) {
    ensure_side();
    const CholPlan& pl = chol_plan(f.B, fill_pays(f.B));
    size_t cut = 0;                       // one past the panel op after which block columns < mid are final
    while (cut < pl.ops.size() && !(pl.ops[cut].kind == 0 && pl.ops[cut].k == tri_mid - 1)) ++cut;
    if (cut == pl.ops.size())
      throw Err(BOBE_ERR_STATE, "internal error: the factorisation has no panel to fork the inverse after");
    ++cut;
    struct Join {                         // no exception leaves with the side stream still working on the caller's buffers
      bobe_gp& g;
      bool forked = false, joined = false;
      ~Join() {
        if (forked && !joined) (void)hipStreamSynchronize(g.side_stream);
      }
    } join{*this};
    Aside aside{nb, f.diag};
    potrf_ops(f, pl, 0, cut, aside);
    HIPCHK(hipEventRecord(ev_fork, stream));
    HIPCHK(hipStreamWaitEvent(side_stream, ev_fork, 0));
    join.forked = true;
    trtri_part(TRI_LEAD, f, aside, side_stream);
    HIPCHK(hipEventRecord(ev_join, side_stream));
    potrf_ops(f, pl, cut, pl.ops.size(), aside);
    trtri_part(TRI_TRAIL, f, aside, stream);
    HIPCHK(hipStreamWaitEvent(stream, ev_join, 0));
    join.joined = true;
    trtri_part(TRI_TOP_R, f, no_aside(), stream);
  } else {
    trtri(f, potrf(f, true));
  }
  solve_alpha(f.linv, f.w, f.alpha, f.part, f.B, f.mat, f.vec, f.prt, rhs, 0);
}

void bobe_gp::factor_into(const Hyper& h, const FactorBufs& f, const Hyper* hdev) {
  scale(X.d(), N, Np, h, f.xst, Np, hdev, f.B, f.xs, f.info);    // (also arms the B info words)
  assemble_kxx(h, f, hdev);
  chol_solve(f);
}

void bobe_gp::mll_terms(const double* wv, const double* a, double* res_dev, const int* info_dev) {
  hipLaunchKernelGGL(k_mll_terms, dim3(1), dim3(256), 0, stream, wv, a, Np, Np, res_dev, (int64_t)0, (int64_t)0, (int64_t)0,
                     info_dev);
  LAUNCH_CHECK();
}

void bobe_gp::res_to_host(const double* res_dev, double* h, int n) {
  HIPCHK(hipMemcpyAsync(h, res_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
  sync();
}

// the text of a BOBE_NOT_PD status: a non-positive pivot (the factorisation's info word), or pivots below pivot_floor
std::string bobe_gp::not_pd_text(int inf, double min_diag) const {
  if (inf != 0x7f7f7f7f) return "kernel matrix not positive definite at column " + std::to_string(inf - 1);
  char buf[200];
  if (min_diag != min_diag)
    std::snprintf(buf, sizeof buf, "kernel matrix not positive definite: NaN pivot");
  else
    std::snprintf(buf, sizeof buf,
                  "kernel matrix numerically singular: smallest pivot %.3g is below %g ulp of its diagonal (rank test)",
                  min_diag * min_diag, pivot_ulp);
  return buf;
}

// The slots' streams are made through the CU-mask entry point with every CU enabled: such a stream gets a
// hardware queue of its own, which plain streams (multiplexed on a few queues) do not - 34 vs 42 ms for the
// 20-evaluation fit at N = 4096.  (Real CU partitions were measured and dropped, DESIGN.md.)
const std::vector<hipStream_t>& bobe_gp::slot_stream_set() {
  std::vector<hipStream_t>& v = slot_streams;
  if (!v.empty()) return v;
  const int words = (num_cus + 31) / 32;
  for (int i = 0; i < BOBE_MAX_MLL_SLOTS; ++i) {
    hipStream_t st = nullptr;
    std::vector<uint32_t> mask(words, 0u);
    for (int c = 0; c < num_cus; ++c) mask[c / 32] |= (1u << (c % 32));
    if (hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask.data()) != hipSuccess) {
      (void)hipGetLastError();
      st = nullptr;
    }
    if (!st) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    v.push_back(st);
  }
  return v;
}

void bobe_gp::ensure_slots(int n) {
  if (!ev_batch) HIPCHK(hipEventCreateWithFlags(&ev_batch, hipEventDisableTiming));
  const std::vector<hipStream_t>& sts = slot_stream_set();
  while ((int)slots.size() < n) {
    slots.push_back(new EvalWs(1));
    slots.back()->stream = sts[slots.size() - 1];
  }
  for (int i = 0; i < n; ++i) slots[i]->ensure(*this, 1);
}

void bobe_gp::ensure_batch(int B) {
  batch.ensure(*this, B);
  (void)chol_plan(B, fill_pays(B));      // (uploads its tables on first use: here, not between the launches of a batch)
}

// The launches of B value (+ gradient) evaluations on ws, on the current stream: the single evaluation and a slot (B = 1,
// stride 0 - plain or under capture) and the lock-step batch (every launch widened by the member dimension).  Results land
// in the pinned ws.h_res[b * 128 + ...]; the info word of member b rides in res[b * 128 + 100], so one copy brings
// everything to the host.  noise_grad: the launches of the gradient's noise component follow the others (gp_loo.hip).
void bobe_gp::eval_enqueue(EvalWs& ws, int B, const Hyper* hs, bool want_grad, const Hyper* hdev, bool noise_grad) {
  const FactorBufs f = ws.bufs(B);
  if (hdev) HIPCHK(hipMemcpyAsync(ws.hyp.p, ws.h_hyp, (size_t)B * sizeof(Hyper), hipMemcpyHostToDevice, stream));
  factor_into(hs[0], f, hdev);
  if (want_grad) {
    const int ntiles = lauum(hs[0], f, hdev, false);
    hipLaunchKernelGGL(k_mll_grad_reduce, dim3(d + 2, B), dim3(256), 0, stream, (const double*)f.gpart, ntiles,
                       dcap_of(d) + 1, d, dcap_of(d), f.res, (const double*)f.w, (const double*)f.a, Np, Np,
                       (const int*)f.info, f.gps, f.rs, f.vec, f.mat);
    if (noise_grad) mll_noise_tail(f, hs, hdev);
  } else {
    hipLaunchKernelGGL(k_mll_terms, dim3(B), dim3(256), 0, stream, (const double*)f.w, (const double*)f.a, Np, Np, f.res,
                       f.vec, f.mat, f.rs, (const int*)f.info);
  }
  LAUNCH_CHECK();
  // ([100] = info, [101] = min L_jj are the last a member writes; the batch brings its members' whole blocks)
  HIPCHK(hipMemcpyAsync(ws.h_res, ws.res.p, (size_t)(ws.width > 1 ? B * 128 : 102) * sizeof(double), hipMemcpyDeviceToHost,
                        stream));
}

// Up to graph_max_n points an evaluation is tens of kernels of a few microseconds each, and with several slots
// in flight the host cannot enqueue them as fast as the GPU retires them: a slot replays its pipeline as one
// graph (N = 64 / 512 / 2048 with four in flight: 42 / 107 / 419 us per evaluation instead of 66 / 141 / 553).
void bobe_gp::eval_replay(EvalWs& ws, const Hyper* hs, bool want_grad) {
  EvalGraph& eg = ws.eg;
  const int w = want_grad ? 1 : 0;
  const std::array<const void*, 16> sig = {ws.XsT.p, ws.A.p, ws.Linv.p, ws.Tmp.p, ws.w.p, ws.alpha.p, ws.part.p, ws.gpart.p,
                                           ws.res.p, ws.info.p, X.p, y.p, probs.p, static_cast<const void*>(ws.h_res),
                                           reinterpret_cast<const void*>(static_cast<uintptr_t>(N)),
                                           static_cast<const void*>(stream)};
  if (!eg.exec[w] || eg.sig[w] != sig) {     // first use, or N / a buffer changed since the capture
    if (eg.exec[w]) {
      (void)hipGraphExecDestroy(eg.exec[w]);
      eg.exec[w] = nullptr;
    }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    capturing = true;
    try {
      eval_enqueue(ws, 1, hs, want_grad, static_cast<const Hyper*>(ws.hyp.p));
    } catch (...) {
      capturing = false;
      (void)hipStreamEndCapture(stream, &graph);
      if (graph) (void)hipGraphDestroy(graph);
      throw;
    }
    capturing = false;
    HIPCHK(hipStreamEndCapture(stream, &graph));
    const hipError_t ie = hipGraphInstantiate(&eg.exec[w], graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) {
      eg.exec[w] = nullptr;
      HIPCHK(ie);
    }
    eg.sig[w] = sig;
  }
  HIPCHK(hipGraphLaunch(eg.exec[w], stream));      // (its first node reads ws.h_hyp when it executes; the caller collects before reusing it)
}

// Queue the evaluation of hs[0 .. B) on ws (B = 1 unless ws is the batch) and record what its members will hold.
void bobe_gp::eval_start(EvalWs& ws, int B, const Hyper* hs, bool want_grad, bool noise_grad) {
  noise_grad = noise_grad && want_grad;
  UseWs use_ws(*this, ws);
  for (int b = 0; b < B; ++b) {
    ws.tag[b].clear();                      // (the member's factor is being overwritten; armed once the pipeline is queued)
    ws.h_hyp[b] = hs[b];
    ws.floor[b] = pivot_floor(hs[b]);
  }
  // A lone evaluation on the handle's stream is NOT faster as a graph (125 vs 107 us at N = 64) and stays a
  // plain launch sequence; so does everything while a kernel class is being timed (events are not captured).
  if (ws.width > 1) eval_enqueue(ws, B, hs, want_grad, static_cast<const Hyper*>(ws.hyp.p), noise_grad);
  else if (noise_grad || !on_slot() || N > tuning().graph_max_n || prof_tag != 0)
    eval_enqueue(ws, 1, hs, want_grad, nullptr, noise_grad);
  else eval_replay(ws, hs, want_grad);
  for (int b = 0; b < B; ++b) ws.tag[b].arm(hs[b], data_gen, Np);
}

int bobe_gp::eval_result(const double* hr, double floor, double* mll, double* grad, bool noise_grad) const {
  const int ng = d + 1 + (noise_grad ? 1 : 0);
  int inf;
  std::memcpy(&inf, hr + 100, sizeof(int));
  if (inf != 0x7f7f7f7f || !pivots_resolved(hr[101], floor)) {
    *mll = std::nan("");
    if (grad)
      for (int j = 0; j < ng; ++j) grad[j] = std::nan("");
    g_err = not_pd_text(inf, hr[101]);
    return BOBE_NOT_PD;
  }
  *mll = -0.5 * hr[0] - hr[1] - 0.5 * (double)N * std::log(2.0 * M_PI);
  if (grad)
    for (int j = 0; j < ng; ++j) grad[j] = hr[2 + j];
  return BOBE_OK;
}

// A slot's collect touches only the slot's own stream, records and pinned results: safe while another thread submits to
// another slot.
int bobe_gp::eval_collect(EvalWs& ws, int B, double* mll, double* grad, int* status, bool noise_grad) {
  const int ng = d + 1 + (noise_grad ? 1 : 0);
  HIPCHK(hipStreamSynchronize(ws.stream ? ws.stream : stream));
  int worst = BOBE_OK;
  for (int b = 0; b < B; ++b) {
    const double* hr = ws.h_res + (size_t)b * 128;
    ws.tag[b].collected(hr);
    const int st = eval_result(hr, ws.floor[b], mll + b, grad ? grad + (size_t)b * ng : nullptr, noise_grad);
    if (status) status[b] = st;
    if (st != BOBE_OK) worst = st;
  }
  return worst;
}

// ---- entry-point bodies of this unit (the extern "C" layer is gp_abi.hip) ----------------------------------------------
void bobe_gp::fill(double* p, int64_t n, double v) {
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, n, v);
}

void bobe_gp::set_data(const double* Xin, const double* ys, int64_t n) {
  use();
  sync();
  ++data_gen;
  forget_evals();
  const int64_t np_new = round_up(n, TILE);
  N = n;
  if (np_new != Np) {
    Np = np_new;
    nb = (int)(Np / TILE);
    alloc_for_n();
  }
  X.ensure((size_t)(Np + TILE) * d * sizeof(double));     // (room for bobe_gp_append's rows up to the next block and one more)
  HIPCHK(hipMemcpyAsync(X.p, Xin, (size_t)N * d * sizeof(double),
                        is_device_ptr(Xin) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(y.p, 0, (size_t)Np * sizeof(double), stream));
  HIPCHK(hipMemcpyAsync(y.p, ys, (size_t)N * sizeof(double),
                        is_device_ptr(ys) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  sync();
  have_data = true;
  factored = false;
  forget_z();
}

void bobe_gp::forget_evals() {
  for (bobe::EvalTag& t : own.tag) t.clear();
  for (bobe::EvalTag& t : batch.tag) t.clear();
  for (EvalWs* sl : slots) sl->tag[0].clear();
}

// The fit has usually just evaluated the hyper-parameters bobe_gp_factor is asked for (the best restart's last iterate; the
// benchmark's last theta): its workspace still holds L, Linv, alpha, w and the scaled coordinates, the bits factor_into would
// compute again (2 ms at N = 4096).  A workspace whose record matches hyp bit for bit, the data generation and Np is copied
// into the handle's buffers instead (k_copy_factor: the lower tiles, ~0.1 ms); anything else factorises.
const bobe::EvalTag* bobe_gp::adopt_factor() {
  if (!tuning().factor_reuse || on_slot()) return nullptr;
  // the first matching member, in this order: the batch's members ascending, the slots that are not in flight, the handle's own
  const EvalWs* ws = nullptr;
  int b = 0, src = 0;
  auto find = [&](const EvalWs& c, int source) {
    for (int i = 0; !ws && c.Np == Np && i < c.cap; ++i) {      // (members [0, cap) fit c's buffers at c.Np: EvalWs::ensure)
      const bobe::EvalTag& t = c.tag[i];
      if (!(t.valid && t.gen == data_gen && t.Np == Np && bobe::same_hyper(t.h, hyp))) continue;
      ws = &c;
      b = i;
      src = source;
    }
  };
  find(batch, 1);
  if (!ws) {
    std::lock_guard<std::mutex> lock(submit_mutex);      // (the slot table grows under this mutex)
    for (const EvalWs* sl : slots)
      if (!sl->busy) find(*sl, 2);
  }
  find(own, 3);
  if (!ws) return nullptr;
  const int64_t xs = ws->xs();
  const int vgroups = (int)std::min<int64_t>(64, (xs + 255) / 256);
  hipLaunchKernelGGL(k_copy_factor, dim3((unsigned)(nb * (nb + 1) + vgroups)), dim3(256), 0, stream,
                     (const double*)ws->A.d() + b * ws->mat(), A.d(), (const double*)ws->Linv.d() + b * ws->mat(), Linv.d(), nb,
                     (const double*)ws->alpha.d() + b * ws->vec(), alpha.d(), (const double*)ws->w.d() + b * ws->vec(), w.d(),
                     (const double*)ws->XsT.d() + b * xs, XsT.d(), Np, xs);
  LAUNCH_CHECK();
  sync();
  factor_source = src;
  if (tuning().trace) std::fprintf(stderr, "[bobe] factor: adopted the factor of an evaluation (source %d)\n", src);
  return &ws->tag[b];
}

int bobe_gp::factor_state() {
  use();
  int inf;
  double min_diag;
  if (const bobe::EvalTag* t = adopt_factor()) {
    inf = t->info;
    min_diag = t->min_diag;
  } else {
    factor_into(hyp, state_bufs());
    // the info word and the smallest pivot's root in one copy (k_mll_terms: res[100], res[101])
    mll_terms(w.d(), A.d(), res.d(), static_cast<const int*>(info.p));
    res_to_host(res.d(), h_res, 102);
    std::memcpy(&inf, h_res + 100, sizeof(int));
    min_diag = h_res[101];
    factor_source = 0;
  }
  factored = true;
  forget_z();
  not_pd = (inf != 0x7f7f7f7f) || !pivots_resolved(min_diag, pivot_floor(hyp));
  if (not_pd) {
    const double nan = std::nan("");
    fill(A.d(), Np * Np, nan);
    fill(Linv.d(), Np * Np, nan);
    fill(alpha.d(), Np, nan);
    LAUNCH_CHECK();
    sync();
    g_err = not_pd_text(inf, min_diag);
    refine_v = false;
    return BOBE_NOT_PD;
  }
  decide_refinement(min_diag);
  return BOBE_OK;
}

int bobe_gp::mll_batch(int64_t B, const double* ls, const double* kvar, double* mll, double* grad, int* status) {
  use();
  const Tuning& tu = tuning();
  int worst = BOBE_OK;
  if (B >= 2 && N >= tu.lockstep_min_n) {      // (kernel-class event timing works there too: one stream, no capture)
    // The evaluations advance in lock step through ONE batched launch sequence.  At every size (round 4, with the launches
    // of small matrices no longer as long as one workgroup's K loop): the 10-D Rosenbrock loop's fits 3.0 -> 2.2 s, the 2-D
    // examples 0.8-1.2 -> 0.4-0.8 s against one graph replay per evaluation on private streams (BOBE_LOCKSTEP_MIN_N = 1024,
    // the default until then); same bits either way.
    for (int64_t b0 = 0; b0 < B; b0 += BOBE_MAX_MLL_SLOTS) {
      const int nbat = (int)std::min<int64_t>(BOBE_MAX_MLL_SLOTS, B - b0);
      Hyper hs[BOBE_MAX_MLL_SLOTS];
      for (int i = 0; i < nbat; ++i) {
        hs[i] = hyp;
        for (int j = 0; j < d; ++j) hs[i].ls[j] = ls[(b0 + i) * d + j];
        hs[i].kvar = kvar[b0 + i];
      }
      ensure_batch(nbat);
      eval_start(batch, nbat, hs, grad != nullptr);
      const int st = eval_collect(batch, nbat, mll + b0, grad ? grad + b0 * (d + 1) : nullptr, status ? status + b0 : nullptr);
      if (st != BOBE_OK) worst = st;
    }
    return worst;
  }
  // (batches below BOBE_LOCKSTEP_MIN_N points, when that is raised: one evaluation slot - private stream, workspace, graph
  //  replay - per member, BOBE_MLL_SLOTS at a time; also what bobe_gp_mll_submit / _wait run on)
  const int width = std::max(1, std::min<int>(tu.mll_slots, BOBE_MAX_MLL_SLOTS));
  for (int64_t b0 = 0; b0 < B; b0 += width) {
    const int nbat = (int)std::min<int64_t>(width, B - b0);
    const auto t_start = std::chrono::steady_clock::now();
    // (a lone evaluation owns the whole chip on the handle's stream)
    auto ws_of = [&](int i) -> EvalWs& { return nbat == 1 ? own : *slots[i]; };
    if (nbat > 1) {
      ensure_slots(nbat);
      for (int i = 0; i < nbat; ++i)
        if (slots[i]->busy)
          throw Err(BOBE_ERR_STATE, "an evaluation submitted with bobe_gp_mll_submit is still in flight on a slot this batch needs");
      // the batch streams start after everything already queued on the handle's stream (data uploads)
      HIPCHK(hipEventRecord(ev_batch, stream));
    }
    for (int i = 0; i < nbat; ++i) {
      Hyper h = hyp;
      for (int j = 0; j < d; ++j) h.ls[j] = ls[(b0 + i) * d + j];
      h.kvar = kvar[b0 + i];
      if (nbat > 1) HIPCHK(hipStreamWaitEvent(slots[i]->stream, ev_batch, 0));
      eval_start(ws_of(i), 1, &h, grad != nullptr);
    }
    const auto t_enq = std::chrono::steady_clock::now();
    for (int i = 0; i < nbat; ++i) {
      const int st = eval_collect(ws_of(i), 1, mll + b0 + i, grad ? grad + (b0 + i) * (d + 1) : nullptr, nullptr);
      if (status) status[b0 + i] = st;
      if (st != BOBE_OK) worst = st;
    }
    if (tu.trace) {
      const auto t_end = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[bobe] mll_batch B=%d: enqueue %.3f ms, total %.3f ms\n", nbat,
                   std::chrono::duration<double, std::milli>(t_enq - t_start).count(),
                   std::chrono::duration<double, std::milli>(t_end - t_start).count());
    }
  }
  return worst;
}

// bobe_gp_mll_noise_batch: the members' own noise levels and d + 2 gradient entries; loo_batch's rule for the form - lock step
// on `batch` BOBE_MAX_MLL_SLOTS at a time, a lone member and everything below BOBE_LOCKSTEP_MIN_N points singly on `own`.
int bobe_gp::mll_noise_batch(int64_t B, const double* ls, const double* kvar, const double* noise, double* mll, double* grad,
                             int* status) {
  use();
  const bool lockstep = N >= tuning().lockstep_min_n;
  const bool want = grad != nullptr;
  int worst = BOBE_OK;
  for (int64_t b0 = 0; b0 < B; b0 += BOBE_MAX_MLL_SLOTS) {
    const int nbat = (int)std::min<int64_t>(BOBE_MAX_MLL_SLOTS, B - b0);
    Hyper hs[BOBE_MAX_MLL_SLOTS];
    for (int i = 0; i < nbat; ++i) {
      hs[i] = hyp;
      for (int j = 0; j < d; ++j) hs[i].ls[j] = ls[(b0 + i) * d + j];
      hs[i].kvar = kvar[b0 + i];
      hs[i].noise = noise[b0 + i];
    }
    double* gr = grad ? grad + b0 * (d + 2) : nullptr;
    int* sts = status ? status + b0 : nullptr;
    if (lockstep && nbat >= 2) {
      ensure_batch(nbat);
      eval_start(batch, nbat, hs, want, true);
      const int st = eval_collect(batch, nbat, mll + b0, gr, sts, true);
      if (st != BOBE_OK) worst = st;
      continue;
    }
    for (int i = 0; i < nbat; ++i) {
      eval_start(own, 1, hs + i, want, true);
      const int st = eval_collect(own, 1, mll + b0 + i, gr ? gr + (size_t)i * (d + 2) : nullptr, sts ? sts + i : nullptr, true);
      if (st != BOBE_OK) worst = st;
    }
  }
  return worst;
}

void bobe_gp::mll_submit(int slot, const double* ls, double kvar, int want_grad) {
  std::lock_guard<std::mutex> lock(submit_mutex);
  use();
  ensure_slots(slot + 1);
  Hyper h = hyp;
  for (int j = 0; j < d; ++j) h.ls[j] = ls[j];
  h.kvar = kvar;
  EvalWs& sl = *slots[slot];
  if (sl.busy)      // its pinned inputs / workspace / results are still in use by the evaluation not yet collected
    throw Err(BOBE_ERR_STATE, "slot already has an evaluation in flight: call bobe_gp_mll_wait first");
  // ordered after whatever is queued on the handle's stream (data uploads); the event is private to the slot
  if (!sl.ev) HIPCHK(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(sl.ev, stream));
  HIPCHK(hipStreamWaitEvent(sl.stream, sl.ev, 0));
  eval_start(sl, 1, &h, want_grad != 0);
  sl.busy = true;
  sl.want_grad = want_grad != 0;
}

int bobe_gp::mll_wait(int slot, double* mll, double* grad) {
  EvalWs* slp = nullptr;
  {
    std::lock_guard<std::mutex> lock(submit_mutex);    // (the slot table grows under this mutex)
    if (slot < 0 || slot >= (int)slots.size() || !slots[slot]->busy)
      throw Err(BOBE_ERR_STATE, "no evaluation was submitted to this slot");
    slp = slots[slot];
  }
  HIPCHK(hipSetDevice(device));
  EvalWs& sl = *slp;
  struct Release {                                        // the slot is free again once its stream has drained
    EvalWs& s;
    ~Release() { s.busy = false; }
  } release{sl};
  return eval_collect(sl, 1, mll, sl.want_grad ? grad : nullptr, nullptr);
}

void bobe_gp::copy_out_matrix(const double* src, double* dst, int lower_only) {
  double* d_out = out_dev(dst, (size_t)N * N, kout);
  hipLaunchKernelGGL(k_copy2d, dim3((unsigned)((N + 255) / 256), (unsigned)N), dim3(256), 0, stream, src, Np, d_out, N, N, N,
                     lower_only);
  LAUNCH_CHECK();
  out_finish(dst, (size_t)N * N, kout);
}

void bobe_gp::get_chol(double* L, double* alpha_out) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  use();
  if (L) copy_out_matrix(A.d(), L, not_pd ? 0 : 1);   // not PD: all-NaN, like jnp.linalg.cholesky
  if (alpha_out)
    HIPCHK(hipMemcpyAsync(alpha_out, alpha.p, (size_t)N * sizeof(double),
                          is_device_ptr(alpha_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  sync();
}

void bobe_gp::set_chol(const double* L, const double* alpha_in) {
  if (!have_data) throw Err(BOBE_ERR_STATE, "call bobe_gp_set_data first");
  use();
  ++data_gen;
  forget_evals();
  factor_source = -1;
  const double* l_in = fetch(L, (size_t)N * N, kout);
  hipLaunchKernelGGL(k_load_padded_lower, dim3((unsigned)((Np + 255) / 256), (unsigned)Np), dim3(256), 0, stream, l_in, N,
                     A.d(), Np, Np);
  HIPCHK(hipMemsetAsync(alpha.p, 0, (size_t)Np * sizeof(double), stream));
  HIPCHK(hipMemcpyAsync(alpha.p, alpha_in, (size_t)N * sizeof(double),
                        is_device_ptr(alpha_in) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  scale(X.d(), N, Np, hyp, XsT.d(), Np);
  for (int k = 0; k < nb; ++k)                       // the 16 x 16 diagonal inverses the block inverse starts from
    hipLaunchKernelGGL(k_potf2<false>, dim3(1), dim3(256), POTF2_SMEM_BYTES, stream, A.d(), Np, Linv.d(), Np, k,
                       static_cast<int*>(info.p));
  LAUNCH_CHECK();
  trtri(state_bufs(), no_aside());
  // the restored factor's smallest pivot decides how the products with Linv are formed, as after a factorisation
  const double min_diag = min_pivot_root();
  factored = true;
  forget_z();
  not_pd = false;
  decide_refinement(min_diag);
}

// the smallest L_jj of the factor in A (k_mll_terms without a right-hand side); synchronises
double bobe_gp::min_pivot_root() {
  mll_terms(nullptr, A.d(), res.d(), nullptr);
  res_to_host(res.d(), h_res, 102);
  return h_res[101];
}

// ---- the reference's free functions on caller-supplied matrices (gp.py:170-197), on a handle that holds no training data
void bobe_gp::size_workspace(int64_t n) {
  if (have_data && n != N) throw Err(BOBE_ERR_STATE, "the handle holds training data of another size (use a data-less handle)");
  if (have_data) return;
  ++data_gen;
  const int64_t np_new = round_up(n, TILE);
  N = n;
  if (np_new != Np) {
    Np = np_new;
    nb = (int)(Np / TILE);
    alloc_for_n();
  }
}

// gp_mll(k, train_y, num_points) (gp.py:170-178): Cholesky of the matrix handed in, alpha, the three MLL terms.  The
// matrix has no kernel variance to scale a rank test with: a pivot <= 0 (or NaN) fails, nothing else - LAPACK's rule.
int bobe_gp::mll_from_k(const double* K, int64_t n, const double* yv, double* mll) {
  use();
  sync();
  size_workspace(n);
  forget_evals();                                  // (the handle's own workspace holds this matrix's factor from here on)
  const FactorBufs f = own.bufs(1);
  const double* k_in = fetch(K, (size_t)n * n, kout);
  hipLaunchKernelGGL(k_load_padded_lower, dim3((unsigned)((Np + 255) / 256), (unsigned)Np), dim3(256), 0, stream, k_in, n,
                     f.a, Np, Np, 1);
  HIPCHK(hipMemsetAsync(w.p, 0, (size_t)Np * sizeof(double), stream));            // (w: the padded right-hand side)
  HIPCHK(hipMemcpyAsync(w.p, yv, (size_t)n * sizeof(double),
                        is_device_ptr(yv) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(f.info, 0x7f, sizeof(int), stream));
  chol_solve(f, w.d());
  mll_terms(f.w, f.a, own.res.d(), f.info);
  res_to_host(own.res.d(), own.h_res, 102);
  // (this entry's own rule instead of a floor: min L_jj > 0; a NaN floor fails whatever the pivot)
  return eval_result(own.h_res, own.h_res[101] > 0.0 ? 0.0 : std::nan(""), mll, nullptr);
}

// fast_update_cholesky(L, k, k_self) (gp.py:181-197): v = L^-1 k and the new diagonal entry sqrt(k_self - v.v) (NaN when
// that is negative, like jnp.sqrt); the caller owns L and lays out the (n+1) x (n+1) factor itself.
void bobe_gp::chol_row_update(const double* L, int64_t n, const double* k, double k_self, double* v, double* diag_out) {
  use();
  sync();
  size_workspace(n);
  forget_evals();
  const FactorBufs f = own.bufs(1);
  const double* l_in = fetch(L, (size_t)n * n, kout);
  hipLaunchKernelGGL(k_load_padded_lower, dim3((unsigned)((Np + 255) / 256), (unsigned)Np), dim3(256), 0, stream, l_in, n,
                     f.a, Np, Np, 0);
  HIPCHK(hipMemsetAsync(w.p, 0, (size_t)Np * sizeof(double), stream));
  HIPCHK(hipMemcpyAsync(w.p, k, (size_t)n * sizeof(double),
                        is_device_ptr(k) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  for (int kb = 0; kb < nb; ++kb)                      // the 16 x 16 diagonal inverses the block inverse starts from
    hipLaunchKernelGGL(k_potf2<false>, dim3(1), dim3(256), POTF2_SMEM_BYTES, stream, f.a, Np, f.linv, Np, kb, f.info);
  LAUNCH_CHECK();
  trtri(f, no_aside());
  hipLaunchKernelGGL(k_gemv_lower, dim3((unsigned)(Np / 4), 1u), dim3(256), 0, stream, (const double*)f.linv, Np, Np,
                     (const double*)w.d(), f.w, (int64_t)0, (int64_t)0, (int64_t)0);
  mll_terms(f.w, f.a, own.res.d(), nullptr);
  HIPCHK(hipMemcpyAsync(v, f.w, (size_t)n * sizeof(double),
                        is_device_ptr(v) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  res_to_host(own.res.d(), own.h_res, 2);                                                        // [0] = v.v
  *diag_out = std::sqrt(k_self - own.h_res[0]);
}

void bobe_gp::kinv_debug(double* Kinv) {
  if (!factored) throw Err(BOBE_ERR_STATE, "call bobe_gp_factor first");
  use();
  lauum(hyp, state_bufs(), nullptr, true);
  // symmetrise on the host side of the copy
  std::vector<double> full((size_t)N * N);
  HIPCHK(hipMemcpy2DAsync(full.data(), (size_t)N * 8, Tmp.p, (size_t)Np * 8, (size_t)N * 8, (size_t)N, hipMemcpyDeviceToHost,
                          stream));
  sync();
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = i + 1; j < N; ++j) full[i * N + j] = full[j * N + i];
  if (is_device_ptr(Kinv)) HIPCHK(hipMemcpy(Kinv, full.data(), full.size() * 8, hipMemcpyHostToDevice));
  else std::memcpy(Kinv, full.data(), full.size() * 8);
}

// ---- factorisation timers (bench.py's Cholesky figures): the launch sequence of potrf() - the one bobe_gp_factor and the
// evaluations issue, its update fillers included - between two HIP events, after one untimed pass
namespace {
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() {
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
  }
  ~EventPair() {
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  double ms() {
    HIPCHK(hipEventSynchronize(e1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, e0, e1));
    return t;
  }
};
}  // namespace

// one untimed pass, then reps timed ones: prep() queues what a pass factorises, run(e0) the factorisation (e0: recorded on
// the handle's stream just before it); the time is taken on the handle's stream
template <typename Prep, typename Run>
static double timed_passes(hipStream_t stream, int reps, Prep prep, Run run) {
  EventPair ev;
  double total = 0.0;
  for (int r = -1; r < reps; ++r) {                            // (pass -1 is untimed: first touch of the workspace, clocks)
    prep();
    HIPCHK(hipEventRecord(ev.e0, stream));
    run(ev.e0);
    HIPCHK(hipEventRecord(ev.e1, stream));
    const double t = ev.ms();
    if (r >= 0) total += t;
  }
  return total / reps;
}

// B factorisations through one launch sequence on the handle's stream: the handle's own workspace (B = 1, the plain call)
// or the lock-step batch (the fit's restarts from lockstep_min_n points up)
double bobe_gp::time_potrf_wide(EvalWs& ws, int B, int reps) {
  if (!have_data) throw Err(BOBE_ERR_STATE, "call bobe_gp_set_data first");
  use();
  forget_evals();                                              // (the timers factorise into the evaluation workspaces)
  if (ws.width > 1) ensure_batch(B);
  UseWs use_ws(*this, ws);
  const FactorBufs f = ws.bufs(B);
  const Hyper* hdev = nullptr;
  if (ws.width > 1) {
    for (int b = 0; b < B; ++b) ws.h_hyp[b] = hyp;
    HIPCHK(hipMemcpyAsync(ws.hyp.p, ws.h_hyp, (size_t)B * sizeof(Hyper), hipMemcpyHostToDevice, stream));
    hdev = static_cast<const Hyper*>(ws.hyp.p);
  }
  scale(X.d(), N, Np, hyp, f.xst, Np, hdev, B, f.xs);
  return timed_passes(
      stream, reps,
      [&] {
        assemble_kxx(hyp, f, hdev);
        HIPCHK(hipMemsetAsync(f.info, 0x7f, (size_t)B * sizeof(int), stream));
      },
      [&](hipEvent_t) { potrf(f); });
}

double bobe_gp::time_potrf(int reps) { return time_potrf_wide(own, 1, reps); }
double bobe_gp::time_potrf_lockstep(int B, int reps) { return time_potrf_wide(batch, B, reps); }

// B factorisations in flight at once, one evaluation slot each (the state of the fit's concurrent restarts):
// device time from the first to the last factorisation kernel, averaged over reps, for all B together
double bobe_gp::time_potrf_batch(int B, int reps) {
  if (!have_data) throw Err(BOBE_ERR_STATE, "call bobe_gp_set_data first");
  use();
  forget_evals();
  ensure_slots(B);
  std::vector<hipEvent_t> done(B);
  for (auto& e : done) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const double ms = timed_passes(
      stream, reps,
      [&] {
        for (int i = 0; i < B; ++i) {      // K(X,X) of every slot, on the handle's stream
          const FactorBufs f = slots[i]->bufs(1);
          scale(X.d(), N, Np, hyp, f.xst, Np);
          assemble_kxx(hyp, f);
          HIPCHK(hipMemsetAsync(f.info, 0x7f, sizeof(int), stream));
        }
      },
      [&](hipEvent_t e0) {
        for (int i = 0; i < B; ++i) {
          EvalWs& sl = *slots[i];
          const FactorBufs f = sl.bufs(1);
          HIPCHK(hipStreamWaitEvent(sl.stream, e0, 0));
          {
            UseWs use_ws(*this, sl);
            potrf(f);
          }
          HIPCHK(hipEventRecord(done[i], sl.stream));
          HIPCHK(hipStreamWaitEvent(stream, done[i], 0));
        }
      });
  for (auto& e : done) (void)hipEventDestroy(e);
  return ms;
}
