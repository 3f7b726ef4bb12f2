/* bobe_gp.h — C ABI of libbobe_gp.so, the MI355X (gfx950) GP-surrogate engine for BOBE.
 *
 * Drop-in boundary for the hot path of Ameek94/BOBE (BOBE/gp.py + the integrated-variance half of
 * BOBE/acquisition.py).  The reference has no FFI of its own (it is pure Python on jax); the boundary
 * it would bind is the method set of its `GP` class, so every entry point below names the reference
 * method(s) it replaces (file:line relative to the reference tree).  bobe_amd/gp.py is the ctypes
 * binding that presents those methods again; INTEGRATION.md shows the stub a maintainer would add.
 *
 * Conventions
 *   - all arrays are C-contiguous fp64 (int64 for indices); matrices are row-major;
 *   - every data pointer may be HOST memory (NumPy) or DEVICE memory (hipMalloc / torch.cuda
 *     tensor); the library detects which and copies only when needed;
 *   - y / alpha / mean / var are in STANDARDISED units (the wrapper applies y_mean, y_std exactly
 *     where gp.py does: gp.py:456, 466, 576);
 *   - return value: 0 ok; > 0 numerical condition (BOBE_NOT_PD: outputs are NaN, like XLA's
 *     Cholesky, so np.isfinite filters such as optim.py:328,341 keep working); < 0 usage / HIP error,
 *     text in bobe_last_error().  Nothing throws or aborts across this boundary;
 *   - BOBE_NOT_PD is raised by a pivot <= 0 or NaN: what LAPACK's dpotrf, the reference's Cholesky (gp.py:175, 549), reports.
 *     A handle can be told to refuse a positive pivot below `ulp` machine epsilons of the kernel matrix's diagonal k(x,x) +
 *     noise as well (bobe_gp_set_pivot_floor_ulp; process default BOBE_PIVOT_FLOOR_ULP, else 0 = off): such a pivot is the
 *     rounding of its column's update, the log-determinant built on it is too small, and a fit is drawn to exactly those
 *     hyper-parameters (dpotrf passes or fails on the last bit there).  The BO driver (bobe_amd/bo.py) runs its surrogate
 *     with ulp = 64; at the reference's default noise of 1e-8 that bounds the usable kernel variance near 1e6;
 *   - a handle is not thread-safe; distinct handles are independent (own stream).
 *   - limits: d <= 32.
 */
#ifndef BOBE_GP_H
#define BOBE_GP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bobe_gp bobe_gp_t;

#define BOBE_OK 0
#define BOBE_NOT_PD 1
#define BOBE_ERR_ARG (-1)
#define BOBE_ERR_HIP (-2)
#define BOBE_ERR_STATE (-3)

#define BOBE_KERNEL_RBF 0    /* gp.py:124-154 */
#define BOBE_KERNEL_MATERN 1 /* gp.py:156-168 */

/* version / build info ("bobe_gp <ver> gfx950") */
const char* bobe_version(void);
/* thread-local text of the last error on this thread */
const char* bobe_last_error(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int bobe_device_count(void);

/* GP.__init__ (gp.py:201-281): handle for one GP on one GPU.  kernel = BOBE_KERNEL_*; d = ndim. */
int bobe_gp_create(bobe_gp_t** out, int device, int kernel, int d);
void bobe_gp_destroy(bobe_gp_t* gp);

/* The HIP stream all work of this handle is issued on (void* = hipStream_t).  set: adopt a caller
 * stream (e.g. torch.cuda.current_stream().cuda_stream) so caller-side events see the kernels. */
void* bobe_gp_get_stream(bobe_gp_t* gp);
int bobe_gp_set_stream(bobe_gp_t* gp, void* hip_stream);
/* block until everything issued on the handle's stream has finished */
int bobe_gp_sync(bobe_gp_t* gp);

/* GP._setup_training_data / GP.update data part (gp.py:283-307, 529-539): X is N x d, y is the
 * already-standardised target vector (N).  Invalidates the factorisation. */
int bobe_gp_set_data(bobe_gp_t* gp, const double* X, const double* y_standardised, int64_t N);

/* GP.lengthscales / kernel_variance / noise assignment (gp.py:253-255, 444-447).  Does NOT refactor. */
int bobe_gp_set_hyper(bobe_gp_t* gp, const double* lengthscales, double kernel_variance, double noise);

/* GP.recompute_cholesky (gp.py:544-550): K = k(X,X)+noise I, L = chol(K), alpha = K^-1 y, and the
 * inverse factor used by every later call.  BOBE_NOT_PD -> L, alpha are NaN. */
int bobe_gp_factor(bobe_gp_t* gp);

/* gp_mll (gp.py:170-178) + its gradient, i.e. the data term of GP.neg_mll (gp.py:385-398) and of the
 * jax.value_and_grad closure of optim.py:306-309, at the given hyper-parameters (noise from
 * set_hyper).  *mll = -1/2 y^T K^-1 y - sum log L_ii - N/2 log 2 pi.  grad (may be NULL) has d+1
 * entries: d mll / d log ls_j (j < d), d mll / d log kernel_variance.  Does not disturb the state
 * left by bobe_gp_factor.  BOBE_NOT_PD -> *mll and grad are NaN. */
int bobe_gp_mll(bobe_gp_t* gp, const double* lengthscales, double kernel_variance, double* mll, double* grad);

/* bobe_gp_mll for B hyper-parameter vectors at once: lengthscales is B x d, kernel_variance has B entries,
 * mll B, grad (may be NULL) B x (d+1), status (may be NULL) B per-vector codes (BOBE_OK / BOBE_NOT_PD).
 * The restarts of optimize_scipy (optim.py:335-354) are independent L-BFGS-B runs which the reference walks
 * one after the other; here up to BOBE_MAX_MLL_SLOTS of their evaluations advance together through ONE launch
 * sequence on the handle's stream (every kernel takes the batch member from a grid dimension), with exactly the
 * arithmetic of bobe_gp_mll per member (bit-identical results).  Returns BOBE_NOT_PD when any vector was not
 * positive definite (its outputs are NaN), < 0 on usage / HIP errors. */
#define BOBE_MAX_MLL_SLOTS 8
int bobe_gp_mll_batch(bobe_gp_t* gp, int64_t B, const double* lengthscales, const double* kernel_variance,
                      double* mll, double* grad, int* status);

/* The same evaluation, split into a non-blocking submit to one of BOBE_MAX_MLL_SLOTS slots and a blocking wait,
 * so that every restart of the fit can run in its own host thread and advance at its own pace (no round
 * barrier): the restarts end up in different phases of the pipeline, the single-workgroup factorisation steps of
 * one overlapping the matrix-core phases of the others.  Results are those of bobe_gp_mll, bit for bit.
 * Threading: submit calls are serialised inside the library; bobe_gp_mll_wait may run concurrently with submits
 * and waits on OTHER slots; a slot holds one evaluation at a time; no other entry point of the same handle may
 * run while evaluations are in flight.  wait returns BOBE_OK / BOBE_NOT_PD (NaN outputs) / < 0. */
int bobe_gp_mll_submit(bobe_gp_t* gp, int slot, const double* lengthscales, double kernel_variance, int want_grad);
int bobe_gp_mll_wait(bobe_gp_t* gp, int slot, double* mll, double* grad);

/* Leave-one-out cross-validation of the factorised state (Rasmussen & Williams, section 5.4.2; the reference has no
 * counterpart): what the surrogate predicts at training point i when that point is left out, with the hyper-parameters, the
 * noise and the y-standardisation held fixed.  Standardised units.  With A = K^-1 (noise included), a_i = A_ii, alpha = A y:
 *   mean[i] = y_i - alpha_i / a_i,   var[i] = 1 / a_i (noise included, no floor: a_i > 0 whenever the factor exists),
 *   lpd[i]  = 1/2 log a_i - alpha_i^2 / (2 a_i) - 1/2 log 2 pi,   *sum_lpd = sum_i lpd[i] (fixed order).
 * a_i = sum_{k >= i} (L^-1)_ki^2, the column sums of squares of the stored inverse factor: one pass over its lower triangle,
 * no product.  Reads the state as it is - after bobe_gp_factor, bobe_gp_append, bobe_gp_clone_state or bobe_gp_set_chol - and
 * returns the same bits for the same state.  mean / var / lpd: N (host or device memory), sum_lpd: one double (host or
 * device); any of them may be NULL.  NOT gated by the classifier (the outputs are about training points).
 * BOBE_ERR_STATE without a factorised state; BOBE_NOT_PD (outputs NaN) for a NaN state. */
int bobe_gp_loo(bobe_gp_t* gp, double* mean, double* var, double* lpd, double* sum_lpd);

/* The LOO log pseudo-likelihood L_LOO = sum_i lpd[i] at the given hyper-parameters (noise from set_hyper) and its gradient:
 * the counterpart of bobe_gp_mll for a fit that maximises L_LOO instead of the marginal likelihood.  *loo (host) = L_LOO;
 * grad (host, may be NULL: the value alone, same bits) has d+1 entries: d L_LOO / d log ls_j (j < d), d L_LOO / d log
 * kernel_variance,
 *   dL_LOO / dtheta_j = sum_ab M_ab dK_ab / dtheta_j,   M = -A diag(c) A - 1/2 (w alpha^T + alpha w^T),
 *   c_i = 1 / (2 a_i) + alpha_i^2 / (2 a_i^2),   b_i = -alpha_i / a_i,   w = A b.
 * Runs on the evaluation workspace: does not disturb the state left by bobe_gp_factor.  BOBE_NOT_PD (the rank test of
 * bobe_gp_set_pivot_floor_ulp included) -> *loo and grad are NaN. */
int bobe_gp_loo_objective(bobe_gp_t* gp, const double* lengthscales, double kernel_variance, double* loo, double* grad);

/* bobe_gp_loo_objective for B >= 1 hyper-parameter vectors at once, the counterpart of bobe_gp_mll_batch: lengthscales is
 * B x d, kernel_variance has B entries, loo B, grad (may be NULL: the values alone) B x (d+1), status (may be NULL) B
 * per-vector codes (BOBE_OK / BOBE_NOT_PD).  Up to BOBE_MAX_MLL_SLOTS vectors advance together through ONE launch sequence
 * on the handle's stream (every kernel takes the batch member from a grid dimension), with exactly the arithmetic of
 * bobe_gp_loo_objective per member (bit-identical results); below BOBE_LOCKSTEP_MIN_N points the members run one after
 * another (there is no slot form).  Does not disturb the state left by bobe_gp_factor, and leaves no factor behind that
 * bobe_gp_factor could adopt.  Returns BOBE_NOT_PD when any vector was not positive definite (its outputs are NaN, the
 * others' are unaffected), < 0 on usage / HIP errors. */
int bobe_gp_loo_objective_batch(bobe_gp_t* gp, int64_t B, const double* lengthscales, const double* kernel_variance,
                                double* loo, double* grad, int* status);

/* The noise level as a hyper-parameter (a build addition: the reference keeps the noise a constructor constant).  The four
 * calls below are their namesakes with the noise nu given explicitly instead of taken from set_hyper, and with a gradient of
 * d+2 entries: d / d log ls_j (j < d), d / d log kernel_variance, d / d log nu.  With K~ = K + nu I, A = K~^-1, alpha = A y,
 * a_i = A_ii = sum_{k >= i} (L^-1)_ki^2 and the c, b, w, B = diag(sqrt c) A of bobe_gp_loo_objective:
 *   d MLL   / d log nu = 1/2 nu (sum_i alpha_i^2 - sum_i a_i)              (tr K~^-1 = |L^-1|_F^2: no product, no K^-1)
 *   d L_LOO / d log nu = nu tr M = -nu (|B|_F^2 + w^T alpha)               (|B|_F^2 = sum_k c_k (A^2)_kk)
 * every sum over the true N x N block, in a fixed order.  The value and the first d+1 gradient entries are, bit for bit, what
 * bobe_gp_mll / bobe_gp_loo_objective return on a handle whose set_hyper noise is the same nu: the extra component comes from
 * launches appended after theirs (one pass over L^-1's lower triangle resp. over B, bandwidth-bound).  grad == NULL: the value
 * alone, no extra launch.  nu must be finite and > 0 (BOBE_ERR_ARG otherwise).  The installed hyper-parameters and the
 * factorised state are not touched.  BOBE_NOT_PD (rank test included, its floor from the member's own kernel_variance + nu)
 * -> the value and all d+2 entries are NaN.  The batch forms take noise[B] and grad B x (d+2); up to BOBE_MAX_MLL_SLOTS
 * members advance in lock step, a lone member and every member below BOBE_LOCKSTEP_MIN_N points runs singly, and a member
 * returns the bits of its single call.  There is NO slot form (bobe_gp_mll_submit) and no graph replay of these calls.
 * An MLL member evaluated this way still holds its factor, recorded with its own nu: bobe_gp_set_hyper(.., nu) +
 * bobe_gp_factor adopts it (bobe_debug_factor_source != 0); the LOO forms leave nothing to adopt. */
int bobe_gp_mll_noise(bobe_gp_t* gp, const double* lengthscales, double kernel_variance, double noise, double* mll,
                      double* grad);
int bobe_gp_mll_noise_batch(bobe_gp_t* gp, int64_t B, const double* lengthscales, const double* kernel_variance,
                            const double* noise, double* mll, double* grad, int* status);
int bobe_gp_loo_objective_noise(bobe_gp_t* gp, const double* lengthscales, double kernel_variance, double noise, double* loo,
                                double* grad);
int bobe_gp_loo_objective_noise_batch(bobe_gp_t* gp, int64_t B, const double* lengthscales, const double* kernel_variance,
                                      const double* noise, double* loo, double* grad, int* status);

/* GP.predict_mean_batched / predict_var_batched / predict_batched (gp.py:450-493) for C query points
 * Xq (C x d).  mean[c] = k_c^T alpha; var[c] = kvar + noise - |L^-1 k_c|^2 with
 *   nan_policy 0: clip(var, 1e-12) keeps NaN (predict_var_single, gp.py:465)
 *   nan_policy 1: NaN and < 1e-12 -> 1e-12     (predict_single,     gp.py:487-488)
 * either output may be NULL. */
int bobe_gp_predict(bobe_gp_t* gp, const double* Xq, int64_t C, double* mean, double* var, int nan_policy);

/* WeightedIntegratedPosteriorBase.get_next_point sweep (acquisition.py:385-398) with WIPV.fun /
 * WIPStd.fun (acquisition.py:438-440, 463-465) over GP.fantasy_var (gp.py:552-576), evaluated for
 * EVERY candidate (C x d) against the integration points Z (M x d) in the algebraically identical
 * rank-1 form.  wipv[c] = mean_z var+(z|c) * y_std^2, wipstd[c] = mean_z sqrt(var+ * y_std^2).
 * argmin_* / min_* follow jnp.argmin (first occurrence).  mean / var: as bobe_gp_predict with
 * nan_policy 1.  Any output pointer may be NULL. */
int bobe_gp_wip_sweep(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                      double* wipv, double* wipstd, double* mean, double* var, int64_t* argmin_v, double* min_v,
                      int64_t* argmin_s, double* min_s);

/* A kriging-believer batch of n_batch WIPV (criterion 0) or WIPStd (criterion 1) picks out of the C candidates from ONE sweep
 * (the reference has no counterpart; its loop, acquisition.py:147-196, sweeps once per member on a surrogate that gained the
 * previous pick at its predicted mean).  The scores depend on the design points only, so appending a pick c* is a rank-one
 * change of what the scorer reads: with s* the pick's noise-included posterior variance and
 *   u(.) = (k(., c*) - V(.)^T V(c*) - sum_{i<j} u_i(.) u_i(c*)) / sqrt(s*),   V = L^-1 K(X, .),
 * the cross term gains u(z) u(c), base_z loses u(z)^2, s_c loses u(c)^2, and the scoring kernel runs again.
 *   stage 0  is bobe_gp_wip_sweep's own launch sequence (the plain product or the blocked substitution, the chunking, the fused
 *            cross tiles) with its intermediates kept for all candidates: stage_scores row 0, picks[0] and pick_scores[0] are
 *            the bits bobe_gp_wip_sweep returns as wipv / wipstd, argmin_* and min_* for the same inputs (cand == Z included).
 *   stage j  one pass over the retained V, one read-modify-write of the cross terms, one scoring pass; all on the handle's
 *            stream, fixed summation orders: the same state gives the same bits.
 * picks[j] (n_batch, required) = the argmin of stage j over the candidates NOT picked before (first occurrence; a picked
 * index is masked - the reference's update() would drop it as a duplicate); pick_scores[j] (n_batch, may be NULL) its score;
 * stage_scores (n_batch x C, may be NULL) every stage's scores of ALL candidates, picked ones included (the computed value).
 * The NaN / 1e-12 floor rules are the scorer's (gp.py:574-576) at every stage.  picks, pick_scores and stage_scores may be
 * host or device memory.
 * Units: y_std is the CALLER's at every stage.  The believer loop standardises its data again after every appended point
 * (gp.py:520-536), which rescales its scores by (y_std_j / y_std)^p, p = 2 (WIPV) or 1 (WIPStd), a factor common to all
 * candidates of a stage; that re-standardisation is NOT imitated: in standardised units (scores / y_std^p) the two agree.
 * NOT gated (like bobe_gp_wip_sweep's scores).  All work buffers are call-local and freed before the call returns; the
 * handle's state is left as it was.  The buffers that grow with C are capped at 16 GiB = 2^31 doubles in all: (Np + Mp + d + 1)
 * x Cp for V, the cross terms, the scaled candidates and s_c, (Np / 128 + n_batch - 1) x Cp for the later stages' partial sums
 * and u rows (n_batch > 1), and (n_batch, or 1 without stage_scores) x C for scores staged on their way to host memory (Np, Mp,
 * Cp: N, M, C rounded up to 128).  N = 4096, M = 512, d = 8 with n_batch = 64 and host stage_scores admits 449 536 candidates.
 * Returns BOBE_ERR_ARG for n_batch outside 1 ... min(C, 64), a criterion other than 0 / 1, a NULL picks / cand / Z, C or M
 * < 1, or a candidate count above the cap; BOBE_ERR_STATE without a factorised state.  A NaN state behaves as in
 * bobe_gp_wip_sweep (BOBE_OK, scores at the floor).  One handle, one device: there is no bobe_mgpu_* form. */
int bobe_gp_wip_select_batch(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                             int n_batch, int criterion, int64_t* picks, double* pick_scores, double* stage_scores);

/* bobe_gp_wip_sweep with importance-weighted integration points and two criteria on the scale of the likelihood (a build
 * addition; the criteria are IMIQR and EIV of Jarvenpaa, Gutmann, Vehtari, Marttinen, Bayesian Analysis 2021).  For candidate
 * c and integration point z, with v+(z|c) the scorer's fantasy variance in physical units (base_z - cross^2 / s_c, the rules
 * of gp.py:574-576, times y_std^2):
 *   b_z  = y_std^2 base_z (non-finite or < 1e-12 -> 1e-12),   mu_z = y_std (K(X,Z)^T alpha)_z  (no y_mean),
 *   l_z  = logw[z]: the log of z's quadrature weight under the flat prior on the unit cube, up to a constant
 *          (logw NULL: the points are draws of the surrogate posterior, l_z = -mu_z),
 *   a_z  = l_z + mu_z,   omega = softmax(a),   u = Phi^-1(3/4) = 0.6744897501960817
 *   wipv[c]   = sum_z omega_z v+                        wipstd[c] = sum_z omega_z sqrt(v+)
 *   imiqr[c]  = log sum_z exp(a_z) 2 sinh(u sqrt(v+))   (the integrated median interquartile range of the lognormal estimate)
 *   eiv[c]    = -log sum_z exp(l_z + 2 mu_z + 2 b_z - v+) = -log R(c)
 *   *log_s    = log sum_z exp(l_z + 2 mu_z + 2 b_z)     = log S:  the expected integrated variance is S - R(c)
 * All four are scores to MINIMISE.  eiv is the negative log of the candidate's gain R(c) rather than S - R(c): 1 - exp(-v+)
 * is 1 in fp64 once v+ exceeds ~37, and every candidate ties; -log R(c) has the same argmin and does not saturate.  The two
 * log scores are log-sum-exps with a running maximum per candidate: finite for any finite inputs with y_std > 0 (the domain:
 * y_std = 0 or non-finite logw / state give NaN scores).
 * With logw NULL, wipv / wipstd are bobe_gp_wip_sweep's bits (the equal-weight scorer itself).  The launch sequence is
 * bobe_gp_wip_sweep's (plain product or blocked substitution, chunking, fused cross tiles, cand == Z) plus one scoring pass;
 * all sums run in a fixed order: the same state gives the same bits whatever the chunk width, host or device pointers.
 * wipv, wipstd, imiqr, eiv (C each), log_s (one double): host or device, any may be NULL and is then not computed.
 * argmin[4] / min[4] (host, may be NULL): first-occurrence argmin (NaN counts as minimal) and minimum per criterion in the
 * order above; -1 / NaN for a criterion whose array is NULL.  NOT gated.  The handle's state is left as it was.
 * BOBE_ERR_ARG: NULL cand / Z, C or M < 1; BOBE_ERR_STATE without a factorised state; a NaN state behaves as in
 * bobe_gp_wip_sweep (BOBE_OK). */
int bobe_gp_wip_sweep_w(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                        const double* logw, double* wipv, double* wipstd, double* imiqr, double* eiv, double* log_s,
                        int64_t* argmin, double* min);

/* bobe_gp_wip_select_batch with bobe_gp_wip_sweep_w's scorer: criterion 0 wipv, 1 wipstd, 2 imiqr, 3 eiv, weights logw (M,
 * host or device, may be NULL).  Row 0 of stage_scores and picks[0] are bobe_gp_wip_sweep_w's bits and argmin.  Under the
 * believer append mu_z does not change, so omega and a_z are the call's; b_z follows the downdated base_z, so the terms of
 * criterion 3 (and log S) are formed again at every stage.  y_std (and with it every physical quantity) is the CALLER's at
 * every stage.  With logw NULL and criterion 0 / 1 the call IS bobe_gp_wip_select_batch.  Same cap, argument rules and
 * return codes as bobe_gp_wip_select_batch (criterion outside 0 .. 3: BOBE_ERR_ARG). */
int bobe_gp_wip_select_batch_w(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                               const double* logw, int n_batch, int criterion, int64_t* picks, double* pick_scores,
                               double* stage_scores);

/* The expected variance of the EVIDENCE estimate after one more evaluation, as a sweep criterion (a build addition: the
 * Bayesian-quadrature criterion for the lognormal estimate exp(f); the reference has no counterpart).  Notation and units are
 * bobe_gp_wip_sweep_w's (physical, no y_mean).  Z = sum_z e^{l_z} e^{f(z)}; an observation at c moves mu_z by r_z xi,
 * xi ~ N(0, 1), and lowers b_z by r_z^2, with r_z(c) = y_std cross_z / sqrt(s_c) (cross_z, s_c: the scorer's).  By the law of
 * total variance
 *   E_xi[Var+ Z] = Var Z - E[Z]^2 T(c),   T(c) = sum_z sum_z' omega_z omega_z' expm1(r_z r_z'),
 *   omega = softmax(l_z + mu_z + b_z / 2),   E[Z] = exp(*log_ez),   *log_ez = LSE_z (l_z + mu_z + b_z / 2).
 * The posterior covariance among the integration points enters the c-independent Var Z only, which this entry does not
 * form: bobe_gp_evidence_moments returns it (as log T0 = log (Var Z / E[Z]^2), the denominator of the share exp(-zvar[c] -
 * log T0) of the evidence variance that an evaluation at c is expected to remove).  T >= 0; for small r it tends to
 * (sum_z omega_z r_z)^2.
 *   zvar[c] = -log T(c), to MINIMISE; the expected reduction of Var Z is exp(2 *log_ez - zvar[c]).  omega is normalised: the
 *   score carries no y_mean shift (a caller in physical units adds y_mean to *log_ez).
 * Rules: |r_z| is capped at sqrt(b_z) (b+ >= 0, the counterpart of the scorer's 1e-12 floor on v+); a non-finite cross_z
 * gives r_z = 0; a candidate whose s_c is not > 0 has every r_z = 0; T <= 0 - every r_z = 0, T underflown, a
 * rounding-negative T - gives zvar = +inf: the candidate teaches nothing.  +inf never wins the argmin over a finite score;
 * all +inf: index 0.  No exponent above 0 is taken (every pair is scaled by the candidate's largest possible pair term), so
 * y_std ~ 4e3 (r r' ~ 1e7, l + mu + b / 2 spread over 1e5) stays finite.
 * COST: a pair sum over the integration points per candidate, C M^2 / 2 transcendental terms where the other scorers do
 * C M - the scoring pass can outweigh the sweep it rides on at M = 512.  M is whatever the sweep accepts.
 * Every sum runs in a fixed order that depends on the candidate and M alone: the same state gives the same bits whatever
 * C, the chunk width, the neighbours, host or device pointers.  The launch sequence is bobe_gp_wip_sweep_w's with this scorer
 * in place of the four-score pass.
 * logw (M, host or device; NULL: l_z = -mu_z), zvar (C, host or device, may be NULL), log_ez / argmin / min (host, one value
 * each, may be NULL; argmin: first occurrence, NaN counts as minimal).  NOT gated.  The handle's state is left as it was.
 * BOBE_ERR_ARG: NULL cand / Z, C or M < 1; BOBE_ERR_STATE without a factorised state; a NaN state behaves as in
 * bobe_gp_wip_sweep (BOBE_OK; the scores are NaN where mu_z is, +inf where only the cross terms are). */
int bobe_gp_wip_sweep_zvar(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                           const double* logw, double* zvar, double* log_ez, int64_t* argmin, double* min);

/* The TOTAL variance of the evidence estimate under the surrogate's joint posterior at the M integration points Z (a build
 * addition; the closed form of the lognormal estimate, the c-independent term of bobe_gp_wip_sweep_zvar).  Notation and units
 * are bobe_gp_wip_sweep_zvar's (physical, no y_mean): Z = sum_z e^{l_z} e^{f(z)}, l_z = logw[z] or -mu_z when logw is NULL,
 *   mu_z = y_std (K(X,Z)^T alpha)_z,   b_z = y_std^2 base_z (non-finite or < 1e-12 -> 1e-12 before the scaling),
 *   S_zz' = y_std^2 (k(z,z') - V_z . V_z') for z != z',   S_zz = b_z,
 *   g_z = l_z + mu_z + b_z / 2,   *log_ez = LSE_z g_z,   lambda_z = g_z - *log_ez,   omega = e^lambda,
 *   T0 = sum_z sum_z' omega_z omega_z' expm1(S_zz')  over all M^2 ordered pairs,   Var Z = e^{2 *log_ez} T0,
 *   *log_t0 = log T0: the log of the squared coefficient of variation of Z.
 * Rules: for z != z', |S_zz'| is capped at sqrt(b_z b_z') (Cauchy-Schwarz; it binds only where rounding or the floor left
 * the diagonal small); a non-finite off-diagonal S counts as 0; T0 <= 0 (underflown or rounding-negative) gives
 * *log_t0 = -inf.  No exponent above 0 is taken: with h = max_z (lambda_z + b_z / 2), p_z = lambda_z - h, E_z = e^{p_z}, a
 * pair with |S| < 1 adds E_z E_z' expm1(S), any other exp(p_z + p_z' + S) - E_z E_z', and log T0 = 2 h + log sum - one
 * transcendental per pair; y_std ~ 4e3 (log T0 ~ 1e7) stays finite.
 * Consequences: exp(-zvar[c] - *log_t0) is the expected share of the evidence variance that an evaluation at c removes, in
 * [0, 1]; the lognormal-matched standard deviation of log Z is sqrt(log1p(T0)).
 * Sigma is never stored, nothing is factorised, no jitter is added, nothing is drawn: one launch over the M / 128 (M / 128 + 1)
 * / 2 lower 128 x 128 tile pairs forms V_z . V_z' on the sweep's tile core and sums the pair terms in its epilogue (an
 * off-diagonal pair counts twice, the diagonal once).  M is bounded by the Np x Mp buffers the sweep itself holds for Z:
 * BOBE_ERR_ARG when the three of them (K(X,Z), V_Z, W_Z) and the call's one double per tile pair would pass
 * bobe_gp_wip_select_batch's 16 GiB in all (the tile sums matter at small Np only: Mp^2 / 32768 doubles).
 * Summation order: a lane adds its 64 (or fewer) elements of the tile in fragment order; the 64 lanes of a wave fold in one
 * fixed tree, the four waves in order; the tiles' sums are added per thread t = tile mod 256 ascending, then pairwise.  No
 * atomics.  The bits depend on the state, Z, logw and y_std alone - not on the pointer kinds, on a hit or miss of the
 * handle's cache of Z's quantities (the sweep's: a repeated host Z is not prepared again, and a later bobe_gp_wip_sweep* on
 * the same Z hits it too), or on which output is NULL.  *log_ez carries bobe_gp_wip_sweep_zvar's bits.
 * Z (M x d) and logw (M, may be NULL): host or device.  log_ez, log_t0: host, one value each; either may be NULL, not both.
 * NOT gated.  BOBE_ERR_ARG: NULL Z, M < 1, both outputs NULL, the cap; BOBE_ERR_STATE without a factorised state - no output
 * is touched then; a NaN state (NaN mu_z) returns BOBE_OK with both outputs NaN, with or without logw (l_z + mu_z is NaN
 * either way), as bobe_gp_wip_sweep_zvar does. */
int bobe_gp_evidence_moments(bobe_gp_t* gp, const double* Z, int64_t M, double y_std, const double* logw, double* log_ez,
                             double* log_t0);

/* bobe_gp_wip_select_batch_w with bobe_gp_wip_sweep_zvar's scorer at every stage.  Row 0 of stage_scores and picks[0] are
 * bobe_gp_wip_sweep_zvar's bits and argmin.  Under the believer append mu_z does not change: omega's l_z + mu_z part is the
 * call's, its b_z part (and the cap on r_z) follows the downdated base_z, so omega is formed again at every stage.  Same cap,
 * argument rules and return codes as bobe_gp_wip_select_batch (there is no criterion argument).  NOT gated. */
int bobe_gp_wip_select_batch_zvar(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                                  const double* logw, int n_batch, int64_t* picks, double* pick_scores,
                                  double* stage_scores);

/* GP.fantasy_var (gp.py:552-576) for C candidates at once: out is C x M, out[c][z] = var+(z|c)*y_std^2. */
int bobe_gp_fantasy_var(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                        double* out);

/* WIPV.fun / WIPStd.fun (acquisition.py:438-440, 463-465) of C candidates TOGETHER WITH their gradients with respect
 * to the candidate coordinates - what the reference obtains with jax.grad in the local refinement of
 * get_next_point (acquisition.py:403-412).  wipv, wipstd: C (may be NULL); dwipv, dwipstd: C x d (may be NULL).
 * Integration points whose fantasy variance sits at the 1e-12 floor contribute no gradient (gradient of where). */
int bobe_gp_wip_grad(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                     double* wipv, double* wipstd, double* dwipv, double* dwipstd);

/* bobe_gp_wip_grad for bobe_gp_wip_sweep_w's four scores (a build addition; it stands in for what the reference takes with
 * jax.grad of the score in the local refinement, acquisition.py:385-412).  Each score is a function of the v+_z alone, and
 * d v+_z/dx_j = y_std^2 [-2 cross_z/s d cross_z/dx_j + cross_z^2/s^2 d s/dx_j] (a z at a floor of gp.py:574-576 is a constant:
 * zero gradient), so d score_k/dx_j = sum_z rho^k_z d v+_z/dx_j with
 *   rho^0 = omega_z,   rho^1 = omega_z / (2 sqrt(v+)),   rho^3 = exp(e_z - v+ + eiv),   e_z = l_z + 2 mu_z + 2 b_z,
 *   rho^2 = exp(t_z - imiqr) coth(x) u / (2 sqrt(v+)),   t_z = a_z + x + log1p(-exp(-2x)),   x = u sqrt(v+);
 * the two softmax weights are formed against the candidate's finished log-sum-exp, so no exponent above 0 is taken.
 * scores[k] (C each) / grads[k] (C x d each), k = 0 wipv, 1 wipstd, 2 imiqr, 3 eiv: host or device; criterion k is computed
 * when either is non-NULL (scores / grads themselves may be NULL).  Units and logw (M, host or device, NULL: l_z = -mu_z) as
 * in bobe_gp_wip_sweep_w: physical, no y_mean.  Matrix-vector work in groups of 16 candidates - there is no tile path - for
 * at most 4096 training points.  A candidate's bits depend on the state, Z, logw, y_std and the candidate alone: not on C,
 * its neighbours, the pointer kinds, the other criteria requested or the handle's caches (Z's quantities and the per-z table
 * are kept while the same host Z, host logw and y_std arrive again).  NOT gated.
 * BOBE_ERR_ARG: NULL cand / Z, C or M < 1, no criterion requested, more than 4096 training points; BOBE_ERR_STATE without a
 * factorised state; a NaN state behaves as in bobe_gp_wip_grad (BOBE_OK). */
int bobe_gp_wip_grad_w(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                       const double* logw, double* const scores[4], double* const grads[4]);

/* bobe_gp_wip_grad_w for bobe_gp_wip_sweep_zvar's score (a build addition): zvar[c] = -log T(c) and its gradient with respect
 * to the candidate's coordinates, dzvar (C x d).  With omega_z = exp(lambda_z), b_z, r_z(c) = y_std cross_z / sqrt(s_c) as
 * there, h_c = max_z (lambda_z + r_z^2 / 2), p_z = lambda_z - h_c and the scaled pair sum T_s (zvar = -(2 h_c + log T_s)):
 *   G_z = sum_z' r_z' exp(p_z + p_z' + r_z r_z')     (the diagonal included; every exponent <= 0, nothing is subtracted),
 *   d zvar/dx_j = sum_z rho_z d r_z/dx_j,   rho_z = -2 G_z / T_s,
 *   d r_z/dx_j = w1 d cross_z/dx_j + w2_z d s/dx_j,   w1 = y_std / sqrt(s),   w2_z = -r_z / (2 s);
 * d cross_z/dx_j and d s/dx_j are bobe_gp_wip_grad_w's.  The pair sum is formed as the sweep forms it (a pair with
 * |r_z r_z'| < 1 through expm1, any other as a difference of two exponentials), over all M^2 ordered pairs.
 * Rules, "gradient of where": a z whose r_z sits at its cap +-sqrt(b_z), or whose cross_z is not finite, is a constant - it
 * keeps its value in T and in G and has rho_z = 0; a candidate whose s_c is not > 0, or whose T <= 0, has zvar = +inf and a
 * zero gradient (on a finite state).
 * Summation order: z's row of the pair sum and G_z over z' in four interleaved quarters (z' = q, q + 4, ...), each ascending,
 * combined (0 + 1) + (2 + 3); T_s, sum_z rho_z w2_z and the z-side sums as bobe_gp_wip_grad_w sums over z (z = t, t + 256, ...
 * per thread, the 64 lanes of a wave, the four waves); the rest is bobe_gp_wip_grad_w's chain.  No atomics.
 * cand, Z, logw (M, NULL: l_z = -mu_z), zvar (C, may be NULL), dzvar (C x d, may be NULL): host or device; log_ez (host, one
 * value, may be NULL): bobe_gp_wip_sweep_zvar's.  Units as there: physical, no y_mean.  Matrix-vector work in groups of 16
 * candidates - there is no tile path - for at most 4096 training points; the pair stage costs C M^2 transcendental terms.
 * A candidate's bits depend on the state, Z, logw, y_std and the candidate alone: not on C, its neighbours, the pointer kinds,
 * which outputs are NULL, or the handle's caches - it shares bobe_gp_wip_grad_w's (Z's quantities and the per-z table, kept
 * while the same host Z, host logw and y_std arrive again; the table gains its lambda row here and keeps the bits of the
 * rows bobe_gp_wip_grad_w reads).  NOT gated.  The handle's state is left as it was.
 * BOBE_ERR_ARG: NULL cand / Z, C or M < 1, zvar and dzvar both NULL, more than 4096 training points; BOBE_ERR_STATE without a
 * factorised state - no output is touched then; a NaN state behaves as in bobe_gp_wip_sweep_zvar (BOBE_OK). */
int bobe_gp_wip_grad_zvar(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                          const double* logw, double* zvar, double* dzvar, double* log_ez);

/* The JOINT posterior of the latent-plus-noise process at C query points Xq (C x d), 1 <= C <= 16384 - what scikit-learn's
 * GaussianProcessRegressor.predict(return_cov=True) (plus noise I) and sample_y return; the reference has no counterpart.
 * Standardised units.  Every work buffer (V: N x C, Sigma and its factor: C x C each) belongs to the call and is freed before
 * it returns.  NOT gated: the classifier gate is not applied (like bobe_gp_fantasy_var).
 *   cov[i][j] = k(q_i, q_j) + noise [i = j] - v_i . v_j,   v = L^-1 k(X, q)   (C x C, row-major, both triangles; the upper one is
 *               the lower one bit for bit; not clipped).  The diagonal is predict_var_single (gp.py:459-466) before its clip;
 *               v is formed as bobe_gp_predict forms it (the product with the inverse factor, or the blocked substitution
 *               while the refine switch is active, bobe_gp_set_refine_kappa).
 * Returns BOBE_ERR_STATE without a factorised state, BOBE_ERR_ARG for C out of range or a NULL pointer, BOBE_NOT_PD (cov is
 * NaN) for a NaN state. */
int bobe_gp_predict_cov(bobe_gp_t* gp, const double* Xq, int64_t C, double* cov);

/* S correlated draws of that posterior at Xq (C x d), S >= 1:
 *   draws[s] = m + L_S z_s   (S x C, row-major),   m = bobe_gp_predict's mean (centered != 0: m is left out),
 *   L_S = chol(cov + tau mean(diag cov) I), tau the first of {0, 1e-12, 1e-10, 1e-8, 1e-6} that factorises under
 *   bobe_gp_mll_from_k's test for a bare matrix (a pivot <= 0 or NaN fails); *jitter_out (may be NULL) = the jitter added,
 *   tau mean(diag cov).  No tau works: BOBE_NOT_PD, draws NaN.
 * z: S x C standard normals of the caller, or NULL: the device draws them from a counter hash of (seed, s, c) -
 *   key = mix(seed ^ mix(s)), u1 = u01(mix(key + 2c)), u2 = u01(mix(key + 2c + 1)), z = sqrt(-2 log u1) cos(2 pi u2), with
 *   mix the splitmix64 finaliser and u01(b) = ((b >> 11) + 0.5) / 2^53 of the HMC / NUTS / random-walk kernels (the exact
 *   contract is above k_draw_normals in posterior_kernels.hpp).  The same seed gives the same draws, bit for bit.
 * Errors as bobe_gp_predict_cov (S < 1 or a NULL draws: BOBE_ERR_ARG; a NaN state: BOBE_NOT_PD, draws NaN).  NOT gated. */
int bobe_gp_posterior_sample(bobe_gp_t* gp, const double* Xq, int64_t C, int64_t S, uint64_t seed, const double* z,
                             int centered, double* draws, double* jitter_out);

/* PATHWISE posterior draws of the LATENT surrogate f (no observation noise added: bobe_gp_predict_cov / _posterior_sample above
 * describe f + noise; here noise enters only through the conditioning).  A path is a function that can be evaluated anywhere,
 * Matheron's rule with the prior drawn through F random Fourier features (the reference has no counterpart):
 *   f_s(x) = phi(x)^T w_s + k(x, X) v_s,   v_s = K^-1 (y - Phi(X) w_s - eps_s),
 *   phi_j(x) = sqrt(2 kvar / F) cos(u_j . (x / ls) + b_j),   w ~ N(0, 1),   eps ~ N(0, noise),   b_j ~ U[0, 2 pi),
 *   u_j ~ N(0, I_d) (RBF) or g_j sqrt(5 / c_j), g_j ~ N(0, I_d), c_j ~ chi^2_5 (Matern-5/2: Student-t with 5 degrees of freedom).
 * Standardised units.  Creating S paths costs a few multi-right-hand-side passes through the factor the handle holds;
 * evaluating them at C points is linear in C and has no cap on C.
 *   create: S >= 1 paths, 1 <= F <= 65536 features.  u (F x d), phase (F), w (S x F), eps (S x N): the caller's arrays (host
 *     or device) or NULL = drawn on the device from `seed` with the counter hash of bobe_gp_posterior_sample, one sub-stream
 *     per array (the exact layout is above k_paths_draw_normals in paths_kernels.hpp); the same seed gives the same bits.
 *     The set is a SNAPSHOT of the factorised state: later set_data / set_hyper / factor / append calls on gp do not change
 *     it.  It must be destroyed BEFORE gp (it works on gp's stream and honours bobe_gp_set_chunk).
 *     BOBE_ERR_STATE without a factorised state, BOBE_ERR_ARG for bad sizes or a NULL out, BOBE_NOT_PD for a NaN state
 *     (*out = NULL, nothing allocated).
 *   get: copies of the four arrays as the set holds them (any pointer may be NULL).
 *   eval: f[s][c] = f_s(Xq_c) (S x C, row-major); centered != 0: f_s - posterior mean (bobe_gp_predict's mean).
 *   argmax: idx[s] = argmax_c f_s(Xq_c) + bias[s][c] and best[s] = that maximum, without forming the S x C matrix; bias (S x C)
 *     may be NULL; ties go to the lower index.
 *   grad: value and INPUT gradient of one path per point: for t < T, with s = path_idx[t], x = Xq[t], xs = x / ls,
 *     c_n = V_c[n][s] + alpha_n (centered != 0: V_c[n][s] alone), amp = sqrt(2 kvar / F), arg_j = u_j . xs + b_j, r2_n = |xs_n - xs|^2,
 *       f[t]     = sum_n c_n k(r2_n) + amp sum_j w_sj cos(arg_j)
 *       df[t][k] = (1 / ls_k) [ sum_n c_n G(r2_n) (xs_nk - xs_k) - amp sum_j w_sj sin(arg_j) u_jk ]
 *     G = k for the RBF kernel, kvar (5/3) (1 + sqrt5 r) exp(-sqrt5 r) for Matern-5/2 (taken as 0 below r2 = 1e-30, where it
 *     multiplies a zero difference).  Xq: T x d, host or device.  path_idx: T entries in [0, S), HOST memory, checked.  f (T)
 *     and df (T x d, row-major): host or device; either may be NULL, not both.  Summation order: one 256-thread workgroup per
 *     point; thread tau adds the kernel terms n = tau, tau + 256, ... and then the feature terms j = tau, tau + 256, ... in
 *     ascending order into one accumulator per component; the 256 partials are added in one fixed tree (lanes of a wave, then
 *     the four waves in order); the division by ls_k comes last.  Invariance: the bits of (f[t], df[t]) depend on the set, the
 *     point, its path index and the centred flag alone - not on T, the other points of the call, the pointer kinds or a NULL
 *     output.  The first call of a set transposes V_c once (8 S Np bytes, freed with the set).  BOBE_ERR_ARG for T < 1, a NULL
 *     p / Xq / path_idx, both outputs NULL, or an index out of range.
 *   hmc_run: whole HMC chains on a PATH - bobe_gp_hmc_run (below) in every respect but the target and the mass matrix.  Chain
 *     c < P samples the posterior implied by the draw s = path_idx[c]: with f and df as under `grad` (uncentred),
 *       mean slot of state / keep = y_mean + y_std f(x),   logp(u) = mean / temp + sum_k [log x_k + log(1 - x_k)],  u = logit(x).
 *     state [P][3d+2], adapt [P][5], hist, keep, dbg, the trajectory lengths, the dual averaging and the random-number layout
 *     are bobe_gp_hmc_run's (a counter hash of (seed, chain, it0 + iteration, index)).  inv_mass is PER CHAIN, [P][d]: paths
 *     differ in shape and the caller pools the spread per path.  One launch runs `niter` whole trajectories of all P chains;
 *     the coefficients c_n = V_c[n][s] + alpha_n are formed once per launch and kept with the training rows in registers and
 *     LDS; thread tau adds its kernel terms and then its features in ascending order, the sums take bobe_gp_hmc_run's tree.
 *     GATED by the PARENT handle's gate as it is set at call time (the gate is not part of the snapshot): an infeasible point
 *     has mean = minus_inf and no gradient, and is never accepted.  Invariance: a chain's bits depend on the set, its path
 *     index, its own state / adapt / inv_mass rows, the seed, its chain number and the iteration numbers - not on P, the
 *     other chains' paths or where launches are cut.  All pointers are HOST memory (a device pointer: BOBE_ERR_ARG);
 *     path_idx is checked against [0, S).  BOBE_ERR_ARG for P < 1, niter < 1, it0 < 0, temp <= 0, thin < 1, hist_from outside
 *     [0, niter], a NULL p / path_idx / state / adapt / inv_mass, or an index out of range.  Shares the transposed V_c with
 *     `grad`.  y_std, y_mean: the units of the snapshot (the caller's: the set does not keep them).
 * eval / argmax / grad are NOT gated (like bobe_gp_predict_cov).  eval / argmax: BOBE_ERR_ARG for C < 1 or a NULL pointer. */
typedef struct bobe_paths bobe_paths_t;
int bobe_gp_paths_create(bobe_gp_t* gp, int64_t S, int64_t F, uint64_t seed, const double* u, const double* phase,
                         const double* w, const double* eps, bobe_paths_t** out);
int bobe_gp_paths_get(bobe_paths_t* p, double* u, double* phase, double* w, double* eps);
int bobe_gp_paths_eval(bobe_paths_t* p, const double* Xq, int64_t C, int centered, double* f);
int bobe_gp_paths_argmax(bobe_paths_t* p, const double* Xq, int64_t C, const double* bias, int64_t* idx, double* best);
int bobe_gp_paths_grad(bobe_paths_t* p, const double* Xq, int64_t T, const int64_t* path_idx, int centered, double* f,
                       double* df);
int bobe_gp_paths_hmc_run(bobe_paths_t* p, int64_t P, const int64_t* path_idx, double* state, double* adapt,
                          const double* inv_mass /* P x d */, uint64_t seed, int64_t it0, int niter, int do_adapt,
                          double y_std, double y_mean, double temp, int hist_from, double* hist, int thin, double* keep,
                          double* dbg);
void bobe_gp_paths_destroy(bobe_paths_t* p);

/* EI.fun / LogEI.fun (acquisition.py:226-253, 318-330) for C points: out[c] = +EI (mode 0) or
 * +log EI (mode 1); best_y, zeta in standardised units. */
int bobe_gp_acq_ei(bobe_gp_t* gp, const double* Xq, int64_t C, double best_y, double zeta, int mode, double* out);

/* The same scores with their input gradients, for C points in one call: val[c] = +EI (mode 0) or +log EI (mode 1) and
 * grad (C x d) = d val / d x, standardised units like bobe_gp_acq_ei; Xq, val, grad: host or device pointers.  The call runs
 * bobe_gp_predict_grad's full chain (mean m, variance v, dm, dv stay on the device) and one elementwise kernel behind it, with
 * one stream synchronisation at the end; value and gradient come from the same (m, v).  Per point, with lo = 1e-18 (LogEI) /
 * 1e-20 (EI): sigma = sqrt(max(v, lo)), dsigma = dv / (2 sigma) and exactly 0 where v < lo (dv arrives as 0 on the 1e-12
 * floor), u = (m - zeta - best_y) / sigma, h = phi(u) + u Phi(u);
 *   EI:    val = sigma h,                grad = Phi(u) dm + phi(u) dsigma
 *   LogEI: val = log h + log sigma (the reference's _log_ei_helper, as bobe_gp_acq_ei), grad = A dm + B dsigma with
 *          A = Phi / (sigma h), B = phi / (sigma h) for u > -1; for u <= -1, with the Mills ratio R = Phi / phi =
 *          sqrt(pi / 2) erfcx(-u / sqrt 2) and g = h / phi = 1 - |u| R (its series 1/u^2 - 3/u^4 + ... from |u| = 30 on),
 *          B = 1 / (sigma g) and A = R B, which stay finite where Phi / h is 0 / 0 (u < -38) and accurate at any |u|.
 * Under a classifier gate an infeasible point has the value of (m = minus_inf, v = 1e-12), like bobe_gp_acq_ei, and a
 * gradient of exactly 0.  A point's outputs do not depend on the rest of its batch.  C <= 0 or mode outside {0, 1}:
 * BOBE_ERR_ARG; a handle that was not factorised: BOBE_ERR_STATE. */
int bobe_gp_acq_ei_grad(bobe_gp_t* gp, const double* Xq, int64_t C, double best_y, double zeta, int mode, double* val,
                        double* grad);

/* Input gradients of GP.predict_single (gp.py:476-489) — what the reference obtains by differentiating through
 * the GP with JAX (EI restarts acquisition.py:246-253/281-290; NUTS on predict_mean_batched samplers.py:268-276).
 * mean, var (may be NULL): as bobe_gp_predict with nan_policy 1.  dmean, dvar: C x d, derivatives with respect
 * to the query coordinates, standardised units; dvar is 0 where var sits at its 1e-12 floor (gradient of where).
 * var == dvar == NULL selects the mean-only mode (one small kernel, no K(X,C)): what HMC on the surrogate calls. */
int bobe_gp_predict_grad(bobe_gp_t* gp, const double* Xq, int64_t C, double* mean, double* var, double* dmean,
                         double* dvar);

/* GP.kernel(xa, xb, ls, kvar, noise, include_noise) (gp.py:124-168; call site acquisition.py:388).
 * lengthscales == NULL uses the handle's current hyper-parameters (kernel_variance / noise arguments
 * are then ignored).  The factorised state is not touched.  out is nA x nB. */
int bobe_gp_kernel(bobe_gp_t* gp, const double* A, int64_t nA, const double* B, int64_t nB,
                   const double* lengthscales, double kernel_variance, double noise, int include_noise, double* out);

/* dist_sq(x, y) (gp.py:80-96): out[a][b] = |A_a - B_b|^2 of the rows as they are; nA x nB, d = the handle's. */
int bobe_gp_dist_sq(bobe_gp_t* gp, const double* A, int64_t nA, const double* B, int64_t nB, double* out);

/* gp_mll(k, train_y, num_points) (gp.py:170-178) on a kernel matrix the CALLER assembled: Cholesky, alpha, and
 *   mll = -0.5 y^T K^-1 y - sum_i log L_ii - 0.5 n log(2 pi).
 * K: n x n symmetric, row-major; y: n.  The handle must hold no training data of another size (a data-less handle is
 * sized on the fly and stays data-less).  BOBE_NOT_PD (mll = NaN) for a pivot <= 0 only: a bare matrix has no kernel
 * variance to scale the rank test with. */
int bobe_gp_mll_from_k(bobe_gp_t* gp, const double* K, int64_t n, const double* y, double* mll);

/* fast_update_cholesky(L, k, k_self) (gp.py:181-197): v = L^-1 k (n entries: the new factor's last row) and
 * diag = sqrt(k_self - v.v) (NaN when negative, as jnp.sqrt); L: n x n lower, row-major.  Same handle rule as above. */
int bobe_gp_chol_row_update(bobe_gp_t* gp, const double* L, int64_t n, const double* k, double k_self, double* v,
                            double* diag);

/* The rank test's factor (see "Conventions"): a positive pivot below `ulp` machine epsilons of k(x,x) + noise counts as
 * not positive definite.  0 (the default) = LAPACK's sign test alone (the reference's behaviour); applies to bobe_gp_factor, the
 * bobe_gp_mll family and bobe_gp_append of this handle; copied by bobe_gp_clone_state.  get returns -1 for NULL. */
int bobe_gp_set_pivot_floor_ulp(bobe_gp_t* gp, double ulp);
double bobe_gp_get_pivot_floor_ulp(bobe_gp_t* gp);

/* Where the installed factor is ill conditioned - (kernel_variance + noise) / smallest pivot above `kappa` - the products
 * with the explicit inverse factor (v = Linv k in bobe_gp_predict, _wip_sweep, _fantasy_var, _wip_grad, _predict_grad,
 * _append) are replaced by a SOLVE with the factor, as the reference does everywhere (solve_triangular, gp.py:462, 484, 571):
 * a blocked forward substitution V_t = inv(L_tt) (B_t - sum_{j<t} L_tj V_j) whose diagonal blocks of `rows` rows are the
 * diagonal blocks of the inverse factor (bobe_gp_wip_grad's path for <= 16 candidates: one step of iterative refinement in
 * vector form instead).  The plain product loses the fantasy variance at the reference's default noise of 1e-8 from kernel
 * variances of ~1e4 on; the substitution with rows = 128 is at or below the error of LAPACK's dtrsm on every rung of
 * profiles/r06_conditioning.txt, at 1.3 x the time of the plain product (N = 4096, 65 536 candidates).
 * kappa: default BOBE_REFINE_KAPPA, else 1e6; 0 = always, negative = never.  The decision is taken when a factor is
 * installed (bobe_gp_factor, _set_chol, _append, _clone_state) - set kappa before.  get: either output may be NULL; *active
 * = 1 while the current factor's products are solved for.
 * rows: a positive multiple of 128; default BOBE_SOLVE_BLOCK, else 128 (256 / 512 are ~10 % faster and lose the fantasy
 * variance two decades of kernel variance earlier); copied by bobe_gp_clone_state.  get returns -1 for NULL. */
int bobe_gp_set_refine_kappa(bobe_gp_t* gp, double kappa);
int bobe_gp_get_refine(bobe_gp_t* gp, double* kappa, int* active);
int bobe_gp_set_solve_block(bobe_gp_t* gp, int rows);
int bobe_gp_get_solve_block(bobe_gp_t* gp);

/* GP.cholesky / GP.alphas (gp.py:259-260; state_dict keys gp.py:626-627): L is N x N lower with
 * zeros above the diagonal, alpha has N entries.  Either may be NULL. */
int bobe_gp_get_chol(bobe_gp_t* gp, double* L, double* alpha);
/* GP.from_state_dict restore without refactorisation (gp.py:671-675). */
int bobe_gp_set_chol(bobe_gp_t* gp, const double* L, const double* alpha);

/* Hamiltonian Monte Carlo on the surrogate (the consumer behind sample_GP_NUTS, samplers.py:216-360, whose NUTS calls
 * the jitted predict_mean once per leapfrog step and chain, samplers.py:268-288): L leapfrog steps of P chains in ONE
 * launch.  Target on u = logit(x): logp = (mean(x) y_std + y_mean) / temp + sum_j [log x_j + log(1 - x_j)].
 * In/out: U (P x d positions), Pm (P x d momenta: in = p0 + eps/2 grad(U), out = final momenta); inv_mass (d).
 * Out: logp (P), grad (P x d, d logp / du at the end point), mean (P, physical units), X (P x d, the end points in
 * the unit cube).  Host or device pointers (all of one kind). */
int bobe_gp_hmc_leapfrog(bobe_gp_t* gp, int64_t P, double* U, double* Pm, const double* inv_mass, double eps, int L,
                         double y_std, double y_mean, double temp, double* logp, double* grad, double* mean, double* X);

/* Whole HMC chains on the device: `niter` trajectories (momentum draw, 4-12 leapfrog steps, Metropolis test and - with
 * do_adapt - the chain's own dual-averaging step-size update) of P chains in ONE launch.  Replaces the per-step JAX
 * calls of NumPyro's NUTS in sample_GP_NUTS (BOBE/samplers.py:216-360) for a plain GP.  All pointers are HOST memory.
 *   state [P][3d+2]  in/out: u = logit(x) (d), dlogp/du (d), x (d), logp, mean (physical units)
 *   adapt [P][5]     in/out: eps, mu, hbar, log_eps_bar, m
 *   hist  [niter - hist_from][P][d]  u after the iterations >= hist_from of this call (NULL: not recorded)
 *   keep  [niter / thin][P][d+1]     x and mean after every thin-th iteration of this call (NULL: not recorded)
 *   dbg   [P][d+3]   the last iteration's momentum draw, L, uniform and acceptance probability (NULL; tests replay it)
 * Random numbers are a counter hash of (seed, chain, it0 + iteration, index).  */
int bobe_gp_hmc_run(bobe_gp_t* g, int64_t P, double* state, double* adapt, const double* inv_mass, uint64_t seed,
                    int64_t it0, int niter, int do_adapt, double y_std, double y_mean, double temp, int hist_from,
                    double* hist, int thin, double* keep, double* dbg);

/* No-U-Turn sampling on the device: `niter` NUTS transitions of P chains in ONE launch - the sampler the reference's
 * sample_GP_NUTS runs through NumPyro (BOBE/samplers.py:216-330): multinomial NUTS with the generalised U-turn criterion
 * (NumPyro's iterative_build_tree), a dense inverse metric and - with do_adapt - the chain's own dual-averaging step-size
 * update towards a mean acceptance statistic of 0.8.  Same target and state as bobe_gp_hmc_run.  All pointers are HOST
 * memory (a device pointer is refused with BOBE_ERR_ARG).
 *   state, adapt, hist, keep   as bobe_gp_hmc_run
 *   inv_metric [d][d]  the inverse metric Sigma (symmetric positive definite: else BOBE_ERR_ARG); momenta are drawn from
 *                      N(0, Sigma^-1), the kinetic energy is p^T Sigma p / 2
 *   max_tree_depth     in [1, 10] (else BOBE_ERR_ARG): at most 2^max_tree_depth - 1 leapfrog steps per transition
 *   stats [niter][P][4]  tree depth, leapfrog steps, divergent flag, acceptance statistic (NULL: not recorded)
 *   dbg   [P][d]         the last transition's momentum draw (NULL: not recorded; tests replay it)
 * Random numbers are a counter hash of (seed, chain, it0 + iteration, index); consumer_kernels.hpp (k_nuts_run) writes
 * out the tree rule and the index layout. */
int bobe_gp_nuts_run(bobe_gp_t* g, int64_t P, double* state, double* adapt, const double* inv_metric, int max_tree_depth,
                     uint64_t seed, int64_t it0, int niter, int do_adapt, double y_std, double y_mean, double temp,
                     int hist_from, double* hist, int thin, double* keep, double* stats, double* dbg);

/* The replacement search of nested sampling on the surrogate (the consumer behind nested_sampling_Dy, samplers.py:55-194,
 * which hands gp.predict_mean_single to dynesty's 'rwalk' sampler one point per call, samplers.py:112-115, 152): P walkers,
 * each `walks` constrained Metropolis steps x' = x + step z, z ~ N(0, I), accepted when x' lies in the unit cube and
 * mean(x') * y_std + y_mean > lstar (and, with a classifier gate set, x' is feasible) - ALL steps of all walkers in ONE
 * launch.  step: d x d lower-triangular, row-major (scale x Cholesky factor of the live points' covariance).
 *   X [P][d]  in: start points (live points), out: end points     logl [P]  in / out: physical-unit mean at the point
 *   n_accepted [P], n_inside [P]: accepted steps / proposals inside the cube (= surrogate evaluations) per walker
 *   dbg [P][d]: every walker's LAST proposal (NULL: not recorded; tests replay it).  All pointers are HOST memory (a
 *   device pointer is refused with BOBE_ERR_ARG; the same holds for bobe_gp_hmc_run).
 * Random numbers: a counter hash of (seed, walker, step, index). */
int bobe_gp_rwalk(bobe_gp_t* gp, int64_t P, double* X, double* logl, const double* step, double lstar, int walks,
                  uint64_t seed, double y_std, double y_mean, int* n_accepted, int* n_inside, double* dbg);

/* GPwithClassifier's gate (clf_gp.py:173-205), evaluated on the device.  One gate per handle, of one of two kinds:
 *  - SVM-RBF (clf.py:188-213), by direct differences, as the reference computes it (bobe_gp_set_gate):
 *      decision(x) = sum_i dual_coef[i] exp(-gamma |support_vectors[i] - x|^2) + intercept   (svm_predict)
 *      proba(x)    = decision >= 0 ? 1 : 0                                                   (svm_predict_proba)
 *    support_vectors: n_sv x d (unit-cube coordinates), dual_coef: n_sv; scikit-learn's SVC supplies them (clf.py:36-69).
 *  - ellipsoid (clf.py:377-412; bobe_gp_set_gate_ellipsoid):
 *      decision(x) = logit = -alpha (x - mu)^T L L^T (x - mu) + beta,   proba(x) = sigmoid(logit)
 *  feasible(x) = proba >= probability_threshold                                                 (clf_gp.py:179)
 * support_vectors == NULL or n_sv == 0 clears the gate, whatever its kind.  While a gate is set, an infeasible query point
 * comes back as
 *   bobe_gp_predict / bobe_gp_predict_grad   mean = -INFINITY (the mark for the wrapper, which returns minus_inf in the
 *                                            units of the method at hand: clf_gp.py:179 physical, :203 standardised),
 *                                            var = 1e-12 (clf_gp.py:189, 204), dmean = dvar = 0
 *   bobe_gp_acq_ei                           EI / LogEI of (mean = minus_inf, var = 1e-12), i.e. what EI.fun computes from
 *                                            the gated predict_single (acquisition.py:246, 323)
 *   bobe_gp_hmc_leapfrog / bobe_gp_hmc_run   mean = minus_inf (physical units), no mean gradient: never accepted
 *   bobe_gp_nuts_run                         mean = minus_inf: a divergent leaf at the default minus_inf, never chosen
 *   bobe_gp_rwalk                            mean = minus_inf: never accepted
 * bobe_gp_wip_sweep, bobe_gp_fantasy_var and bobe_gp_wip_grad are NOT gated (fantasy_var is not, clf_gp.py:207-212), nor
 * are bobe_gp_predict_cov and bobe_gp_posterior_sample.
 * One summation order serves every entry point (256 partial sums, a fixed tree), so a point near the boundary falls on
 * the same side everywhere.  The gate is not part of the state bobe_gp_clone_state copies. */
int bobe_gp_set_gate(bobe_gp_t* gp, const double* support_vectors, int64_t n_sv, const double* dual_coef, double intercept,
                     double gamma, double probability_threshold, double minus_inf);
/* The ellipsoid gate of the reference's parameters: flat_L (d(d+1)/2, the lower triangle in tril_indices order
 * (0,0), (1,0), (1,1), (2,0), ...; RAW: the library puts the diagonal through softplus(.) + 1e-4 once), the centre mu
 * (d), alpha, beta.  Host or device pointers. */
int bobe_gp_set_gate_ellipsoid(bobe_gp_t* gp, const double* flat_L, const double* mu, double alpha, double beta,
                               double probability_threshold, double minus_inf);
/* decision[c] (svm_predict, or the ellipsoid's logit) and feasible[c] (1.0 / 0.0) of C query points; either output may
 * be NULL. */
int bobe_gp_gate_eval(bobe_gp_t* gp, const double* Xq, int64_t C, double* decision, double* feasible);
/* proba[c]: the gate's probability (SVM 0 / 1, ellipsoid sigmoid(logit)) of C query points. */
int bobe_gp_gate_proba(bobe_gp_t* gp, const double* Xq, int64_t C, double* proba);

/* Training of the ellipsoid classifier (clf.py:415-472): n_restarts independent AdamW runs in ONE launch, one workgroup
 * each.  Loss optax.sigmoid_binary_cross_entropy(logit, y).mean() over batches of B = min(batch, N) rows,
 * steps = max(1, N / batch) per epoch; optax.adamw(lr, b1 0.9, b2 0.999, eps 1e-8, weight_decay = wd on every parameter).
 *   X [N][d], y [N] (labels 0 / 1), mu [d] (the centre, not trained)
 *   init [n_restarts][P] starting parameters, P = d(d+1)/2 + 2: raw flat_L, alpha, beta
 *   perm [n_restarts][n_epochs][steps * B] int32 rows of every batch, each in [0, N) (checked)
 *   params_out [n_restarts][P] the final parameters, loss_out [n_restarts] each run's full-data loss
 * Host pointers.  Uses the handle's device, stream and dimension only (no data need be set). */
int bobe_gp_train_ellipsoid(bobe_gp_t* gp, const double* X, const double* y, int64_t N, const double* mu, int n_restarts,
                            const double* init, const int32_t* perm, int n_epochs, int batch, double lr, double wd,
                            double* params_out, double* loss_out);

/* GP.copy (gp.py:740-750) without leaving the device: dst (created with the same kernel, d and device) receives
 * src's training data, hyper-parameters and factorised state by device-to-device copies - no host round trip of the
 * N x N factor and no refactorisation (the reference copies through state_dict / from_state_dict). */
int bobe_gp_clone_state(bobe_gp_t* dst, bobe_gp_t* src);

/* GP.update at unchanged hyper-parameters as a rank-b append, O(b N^2) instead of the O(N^3) recompute_cholesky of
 * gp.py:541-550 (the reference has the rank-1 form as fast_update_cholesky, gp.py:181-197, but uses it only inside
 * fantasy_var).  X_new: b x d new points (1 <= b <= 64); y_all: the N+b targets after re-standardisation
 * (gp.py:520-536 changes all of them; L does not depend on y, alpha is re-solved).  Requires a positive-definite
 * factorised state; if the appended matrix is not positive definite the call ends like bobe_gp_factor (NaN state,
 * BOBE_NOT_PD). */
int bobe_gp_append(bobe_gp_t* gp, const double* X_new, int64_t b, const double* y_all);

/* ---- multi-GPU exchange step (the reference's counterpart is the MPI pool's pickled send/recv,
 * BOBE/pool.py:298-326, and it has no candidate parallelism at all: acquisition.py:394 maps sequentially) ----------
 * One process per GPU.  The library owns a RCCL communicator (librccl.so is opened on first use):
 *   rank 0:      bobe_mgpu_unique_id(id)  -> ship the BOBE_MGPU_ID_BYTES bytes to the other ranks (any channel)
 *   every rank:  bobe_mgpu_init(id, world, rank, device)
 * bobe_mgpu_wip_sweep = bobe_gp_wip_sweep on this rank's contiguous shard [global_offset, global_offset + C) of the
 * candidates (C may be 0), then ONE ncclAllGather of (min wipv, index, min wipstd, index, status) - 40 bytes per rank -
 * and the merge every rank repeats: smallest score, ties to the lowest GLOBAL index (jnp.argmin's first occurrence,
 * acquisition.py:397), NaN counts as minimal.  argmin_* / min_* are the global results; the score vectors stay local.
 * A rank whose local sweep fails still joins the collective (status word): EVERY rank then returns that error code
 * instead of the healthy ones waiting in the all-gather for ever.  The handle must live on bobe_mgpu_init's device.
 * bobe_mgpu_best_fit = all-gather of (mll, theta) and max by mll (pool.py:322-326) for the restart-sharded fit. */
#define BOBE_MGPU_ID_BYTES 128
int bobe_mgpu_unique_id(char* id128);
int bobe_mgpu_init(const char* id128, int world, int rank, int device);
int bobe_mgpu_world(void);
int bobe_mgpu_rank(void);
void bobe_mgpu_finalize(void);
int bobe_mgpu_wip_sweep(bobe_gp_t* gp, const double* cand_shard, int64_t C, int64_t global_offset, const double* Z,
                        int64_t M, double y_std, double* wipv, double* wipstd, double* mean, double* var,
                        int64_t* argmin_v, double* min_v, int64_t* argmin_s, double* min_s);
int bobe_mgpu_best_fit(double mll, const double* theta, int n, double* best_mll, double* best_theta);

/* number of training points / padded leading dimension currently held */
int64_t bobe_gp_npoints(bobe_gp_t* gp);

/* test / bench hooks (not part of the reference surface) -------------------------------------- */
/* C[M x N] = sum_k A(m,k) B(n,k) through the fp64 MFMA tile core.  layout 0: element (r,k) at
 * p[r*ld+k]; layout 1: at p[k*ld+r].  M, N multiples of 128, K multiple of 16.  Device or host ptrs. */
int bobe_debug_gemm(int device, int layoutA, int layoutB, int64_t M, int64_t N, int64_t K, const double* A,
                    int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc);
/* One instantiation ("variant") of the tile core tile_gemm<GLDS, LA, LB, T, NEGA, TRIL, BK> on the caller's operands, with
 * the dynamic LDS of the launch that ships it (a register-staged variant on 64 x 64 tiles with BK = 16, which no launch
 * ships: of the launch that ships its direct-to-LDS twin).  bobe_debug_tile_gemm_count: the number of variants compiled in.
 * bobe_debug_tile_gemm_info: info9 = {T, BK, glds, layoutA, layoutB, nega, tril, groups, single_buffer} (layouts as in
 * bobe_debug_gemm; groups = 2: two 256-thread tile groups per workgroup, side by side in n; single_buffer: LDS for one
 * K-step only).
 * bobe_debug_tile_gemm runs a tiles_m x tiles_n grid of T x T tiles.  Tile (p, q), with r = m0 + p T and c = n0 + q T:
 *   acc = preload ? C[r.., c..] : 0;  acc (+/-)= sum over k in [kbeg, kend) of A(r + i, k) B(c + j, k);
 *   C[r.., c..] = alpha acc + beta C[r.., c..]
 * HOST pointers only: A [rows_a x lda], B [rows_b x ldb] and C [rows_c x ldc] are copied in whole (whatever surrounds the
 * operands included) and the whole of C is copied back.  An array passed more than once (A == B, or A == B == C: the
 * trailing update's in-place form) is ONE device buffer.  Refused with BOBE_ERR_ARG before anything is launched or
 * written: an unknown variant; an odd leading dimension; m0, n0 or kbeg not a multiple of T; kend - kbeg not a positive
 * multiple of BK; more than one K-step on a single_buffer variant; an odd tiles_n with groups = 2; operands or tiles that
 * do not fit their arrays; an array that is both read and written where the two regions meet. */
int bobe_debug_tile_gemm_count(void);
int bobe_debug_tile_gemm_info(int variant, int* info9);
int bobe_debug_tile_gemm(int device, int variant, int tiles_m, int tiles_n, int64_t m0, int64_t n0, int64_t kbeg,
                         int64_t kend, const double* A, int64_t lda, int64_t rows_a, const double* B, int64_t ldb,
                         int64_t rows_b, double* C, int64_t ldc, int64_t rows_c, double alpha, double beta, int preload);
/* K^-1 (N x N, full symmetric) from the current factorisation — used by the parity tests */
int bobe_debug_kinv(bobe_gp_t* gp, double* Kinv);
/* L^-1 (N x N lower) from the current factorisation */
int bobe_debug_linv(bobe_gp_t* gp, double* Linv);
/* What the acquisition sweep forms on the way to its scores, for the tests of the intermediates: runs the sweep of
 * bobe_gp_wip_sweep (the same launches in the same order, a WIPV row as the scorer's output; stage 0 of
 * bobe_gp_wip_select_batch) into buffers of the call and copies out, row-major and without padding, V [N x C] = L^-1 K(X, C)
 * (V_Z when the candidates are the integration points: that path forms no V of its own), VZ [N x M] = L^-1 K(X, Z),
 * crossT [M x C] = V_Z^T V, sc [C] = kself - |V[:, c]|^2 and basez [M] = kself - |V_Z[:, z]|^2.  Host pointers (cand and Z may
 * be device memory); every output may be NULL.  BOBE_ERR_STATE without a factor, BOBE_ERR_ARG for C < 1, M < 1, a NULL cand
 * or Z, or a C over which the call's buffers, (Np + Mp + d + 1) x Cp + C doubles, pass bobe_gp_wip_select_batch's 16 GiB. */
int bobe_debug_sweep_terms(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double* V, double* VZ,
                           double* crossT, double* sc, double* basez);
/* The batch selection's downdated state, for the tests of its later stages: runs bobe_gp_wip_select_batch's own code (the same
 * launches in the same order, no kernel of its own) with n_stage + 1 stages, n_stage in [0, 63], that is n_stage rank-one
 * downdates, and copies out row-major and without padding what the last stage scored from: crossT [M x C], sc [C], basez [M]
 * (the call's downdated copy; the handle's stays) and the u rows UC [n_stage x C], UZ [n_stage x M] of the downdates.
 * criterion 0 wipv, 1 wipstd, 2 imiqr, 3 eiv, 4 zvar, routed as the shipped entries route them: 0 / 1 with logw NULL through
 * bobe_gp_wip_select_batch's scorer, 0 .. 3 otherwise through bobe_gp_wip_select_batch_w's, 4 through
 * bobe_gp_wip_select_batch_zvar's.  forced (n_stage, host, may be NULL): forced[j] is written over the pick record on the
 * device after stage j's argmin and before stage j + 1 reads it, so stage j + 1 downdates by forced[j]; the argmins of the
 * later stages mask the forced picks.  picks (n_stage + 1, may be NULL): the n_stage picks applied, then the last stage's
 * argmin; stage_scores ((n_stage + 1) x C, may be NULL) as bobe_gp_wip_select_batch's.  With forced equal to the shipped
 * entry's own picks, or NULL, stage_scores are the shipped entry's bits; n_stage = 0 hands out bobe_debug_sweep_terms' bits.
 * The state outputs and forced are host pointers, every output may be NULL.  Refusals and the 16 GiB cap are
 * bobe_gp_wip_select_batch's at n_batch = n_stage + 1; BOBE_ERR_ARG too for n_stage outside [0, 63], a forced index outside
 * [0, C) or a repeated one, before anything is launched or written. */
int bobe_debug_batch_terms(bobe_gp_t* gp, const double* cand, int64_t C, const double* Z, int64_t M, double y_std,
                           const double* logw, int criterion, int n_stage, const int64_t* forced, double* crossT, double* sc,
                           double* basez, double* UC, double* UZ, int64_t* picks, double* stage_scores);
/* run only the Cholesky factorisation of the current K `reps` times after ONE untimed pass (first touch of the
 * workspace, clocks) and return the mean device time per factorisation in milliseconds (HIP events on the handle's
 * stream).  The two batch forms below time the same way. */
int bobe_debug_time_potrf(bobe_gp_t* gp, int reps, double* ms);
/* B factorisations in flight at once (one evaluation slot each); *ms = device time for all B together */
int bobe_debug_time_potrf_batch(bobe_gp_t* gp, int B, int reps, double* ms);
/* the same B factorisations advancing in lock step through one batched launch sequence on the handle's stream */
int bobe_debug_time_potrf_lockstep(bobe_gp_t* gp, int B, int reps, double* ms);
/* where the factor of the last bobe_gp_factor came from: 0 factorised; adopted from the workspace of an evaluation at the
 * same hyper-parameters and data - 1 a lock-step batch slot (bobe_gp_mll_batch), 2 an evaluation slot (bobe_gp_mll_submit),
 * 3 the single evaluation's (bobe_gp_mll); -1 no bobe_gp_factor since the data or the factor was last set otherwise */
int bobe_debug_factor_source(bobe_gp_t* gp);
/* Per-kernel-class device timing with HIP events recorded on the handle's stream around every launch
 * of the selected class (0 = off).  read() synchronises, returns the summed milliseconds and the
 * number of launches since the last select()/read(), and resets the counters. */
#define BOBE_PROF_POTF2 1  /* diagonal-block Cholesky + inverse */
#define BOBE_PROF_TRSM 2   /* panel solve (GEMM with the inverted diagonal block) */
#define BOBE_PROF_SYRK 3   /* trailing update of the blocked Cholesky */
#define BOBE_PROF_TRTRI 4  /* one level of the recursive triangular inverse (two launches) */
#define BOBE_PROF_LAUUM 5  /* K^-1 = Linv^T Linv fused with the gradient reduction */
#define BOBE_PROF_TRIMUL 6 /* sweep: V = Linv * K(X, C_chunk) with column sum of squares */
#define BOBE_PROF_CROSS 7  /* sweep: WIPV / WIPStd scoring */
#define BOBE_PROF_KXX 8    /* K(X,X) assembly */
#define BOBE_PROF_CROSSVV 9 /* sweep: cross-covariance GEMM V_Z^T V of the two solved factors; the class also brackets the other
                             * tile products of solved factors - bobe_gp_predict_cov's Sigma pass, the paths' product and
                             * bobe_gp_evidence_moments' pair launch - so a total mixes whichever of them ran while it was selected */
#define BOBE_PROF_KXC 10   /* sweep: K(X, C_chunk) assembly */
int bobe_gp_profile_select(bobe_gp_t* gp, int kernel_class);
int bobe_gp_profile_read(bobe_gp_t* gp, double* total_ms, int64_t* launches);
/* back-to-back v_mfma_f64_16x16x4_f64 issue rate on all CUs (1 or 2 waves per SIMD), in TFLOP/s */
int bobe_debug_mfma_peak(int device, int waves_per_simd, double* tflops);
/* The samplers' cross-lane sums (v_permlane32/16_swap + DPP, kernels_common.hpp) on one wave: in [64][D] (lane, component),
 * D = 8, 16 or 32; out[j] = sum over the lanes of component j by the all-components butterfly, out[D + j] = the same by the
 * single-value sum. */
int bobe_debug_wave_sums(int device, int D, const double* in, double* out);
/* where a chain workgroup of bobe_gp_paths_hmc_run keeps this set's training rows: info4 = rows in registers, rows in LDS,
 * rows streamed from L2 in every step, features per thread (tests prove with it that they cover every home) */
int bobe_debug_paths_chain_layout(bobe_paths_t* p, int* info4);
/* candidate chunk size of the sweep (multiple of 128); 0 returns to the defaults (8192; 32 768 on the substitution path of an
 * ill-conditioned factor) */
int bobe_gp_set_chunk(bobe_gp_t* gp, int64_t chunk);
/* launch shape of the blocked forward substitution (bobe_gp_set_solve_block), speed only: panel = rows per long update
 * launch (a multiple of 128), chunk = candidates per launch sequence (0: the sweep's) */
int bobe_debug_solve_opts(bobe_gp_t* gp, int panel, int64_t chunk);

#ifdef __cplusplus
}
#endif
#endif
