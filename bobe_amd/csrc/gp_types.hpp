// Plain types shared by the kernels and the host side of libbobe_gp.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tri_split.hpp"

namespace bobe {

constexpr int MAX_D = 32;
// rows of the weighted scorer's per-z table (criteria_kernels.hpp, k_wip_zterms): mu, a, omega, e = l + 2 mu + 2 b, l,
// lambda = l + mu + b / 2 - log E[Z] (written for the evidence-variance scorer only).  The host sizes the table and places
// log S and log E[Z] behind it (gp_handle.hpp, SweepW) with the same constant.
constexpr int ZTERM_ROWS = 6;

struct Hyper {
  double ls[MAX_D];
  double kvar;
  double noise;
  int d;
  int kern;  // 0 rbf, 1 matern-5/2
};

// (TriProb, the problem {lo, mid, hi} of the recursive triangular inverse: tri_split.hpp)

// A filler job of a panel launch (k_chol_panel<true, .>): update tile A[ti][tj] -= sum_k A[ti][k] A[tj][k]^T over the
// 64-column units [k0, k1) - k_syrk_trail's tile.  The two jobs of a workgroup run the same number of K-steps
// (workgroup-wide barriers): the plan pairs tiles of one block column; FILL_TWIN completes an odd count (computed, not stored).
enum { FILL_TWIN = 1 };
struct FillJob { int ti, tj, k0, k1, flags, pad0; };

// The classifier gate of GPwithClassifier (clf_gp.py:173-205).  `kind` selects the decision function:
//   GATE_SVM        SVM-RBF of clf.py:188-213: decision(x) = sum_i dual[i] exp(-gamma |sv_i - x|^2) + intercept,
//                   proba = decision >= 0.  svT: support vectors SoA, coordinate j of vector i at svT[j * ld + i]
//                   (unit-cube coordinates, not scaled).
//   GATE_ELLIPSOID  the learned Mahalanobis ball of clf.py:377-412: decision(x) = logit = -alpha |L^T (x - mu)|^2 + beta,
//                   proba = sigmoid(logit).  Lt: L with its diagonal already through softplus + 1e-4, dense row-major
//                   d x d (L[i][j] at Lt[i * d + j], zero above the diagonal); mu: the centre (d).
// feasible = proba >= threshold.  GATE_NONE: no gate (gate_on).
enum GateKind { GATE_NONE = 0, GATE_SVM = 1, GATE_ELLIPSOID = 2 };
struct Gate {
  const double* svT;
  const double* dual;
  int64_t ld;
  int n_sv;
  double intercept, gamma, threshold, minus_inf;
  int kind;
  const double* Lt;
  const double* mu;
  double alpha, beta;
};
// "a gate is set" - the one test every entry point uses (host and device)
__host__ __device__ inline bool gate_on(const Gate& g) { return g.kind != GATE_NONE; }

}  // namespace bobe
