/*
 * ppbo_hip.h -- C-ABI of libppbo_hip.so: the MI355X (gfx950) GP-surrogate and
 * acquisition engine behind PPBO's GPModel / next_query() / Hsampler surface.
 *
 * The reference (AaltoPML/PPBO) has no FFI layer: its boundary is a Python
 * object surface.  Each entry point below names the reference expression it
 * replaces (file:line relative to the reference repository).  INTEGRATION.md
 * shows the ctypes stub a PPBO maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every function returns int: 0 ok, <0 invalid argument, >0 HIP error code
 *     (PPBO_ERR_NOT_PD = 1001 is the only non-HIP positive code).  Nothing throws.
 *   - pointers named d_* are DEVICE pointers owned by the caller (row-major,
 *     C-contiguous float64 unless stated); h_* are HOST pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Functions with host outputs synchronise that stream before returning.  Calls WITHOUT host outputs
 *     (ppbo_gram, ppbo_cross_cov, ppbo_rff_project, ppbo_predict / ppbo_rff_score with NULL h_best_*, ...)
 *     neither synchronise nor -- after their first call at a given size -- allocate, so a sequence of them can be
 *     captured in a HIP graph on that stream and replayed (tests/test_gpu_concurrent.py).
 *   - a ppbo_ctx is bound to ONE device; every entry point runs on that device and restores
 *     the caller's current device on return.  Several contexts (on the same or different
 *     devices) may live in one process; a single ctx is not re-entrant across threads.
 *     A ctx owns only private workspaces; the library has no process-global mutable state.
 */
#ifndef PPBO_HIP_H
#define PPBO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPBO_ABI_VERSION 9
#define PPBO_ERR_NOT_PD 1001

/* The library is built with -fvisibility=hidden: the entry points declared here are its ONLY dynamic symbols
 * (tests/test_abi.py checks `nm -D --defined-only` against this header). */
#if defined(__GNUC__) || defined(__clang__)
#define PPBO_API __attribute__((visibility("default")))
#else
#define PPBO_API
#endif

typedef struct ppbo_ctx ppbo_ctx;

/* kernel ids: src/kernels.py:19 (SE), :27 (RQ, alpha=2), :36 (camphor-copper, D must be 6).
 * The Matern kernels have no reference line; they are the GPy / scikit-learn Matern(nu) definition with
 * r = |x - x'| and theta = [sigma, l, sigma_f]:
 *   PPBO_KERNEL_MATERN52  k = sigma_f^2 (1 + a + a^2 / 3) exp(-a),  a = sqrt(5) r / l   (nu = 5/2)
 *   PPBO_KERNEL_MATERN32  k = sigma_f^2 (1 + a) exp(-a),            a = sqrt(3) r / l   (nu = 3/2)
 * Any other id is rejected with "invalid argument". */
enum {
  PPBO_KERNEL_SE = 0,
  PPBO_KERNEL_RQ = 1,
  PPBO_KERNEL_CAMPHOR = 2,
  PPBO_KERNEL_MATERN52 = 3,
  PPBO_KERNEL_MATERN32 = 4
};

/* candidate score folded into the running argmax */
enum {
  PPBO_SCORE_MEAN = 0,         /* mu(x): what mu_star maximises, src/gp_model.py:422 */
  PPBO_SCORE_POINTWISE_EI = 1, /* (mu-mu*)Phi(z)+s phi(z): G=1 closed form of src/acquisition.py:72-81 */
  PPBO_SCORE_VARIANCE = 2      /* sigma^2(x): G=1 form of varmax, src/acquisition.py:170-178 */
};

PPBO_API int ppbo_abi_version(void);
PPBO_API int ppbo_ctx_create(int device, ppbo_ctx** out);
PPBO_API int ppbo_ctx_destroy(ppbo_ctx* ctx);
/* copies the last error text of this ctx into buf (NUL terminated) */
PPBO_API int ppbo_last_error(ppbo_ctx* ctx, char* buf, size_t n);

/* ---- per-kernel event timing (the reference only prints time.time() deltas when verbose,
 * src/gp_model.py:110-132).  When enabled, the named hot kernels are bracketed
 * by hipEvents on the caller's stream; ppbo_profile_read synchronises those events and
 * returns the accumulated duration and launch count since the last reset.
 * names: "gram", "kstar", "quadform", "score", "rff_project", "rff_score", "potrf", "line_kstar", "line_y",
 * "line_cov", "line_mc", "fused_score" (the one-launch scoring kernel of models with up to 1024 rows). */
PPBO_API int ppbo_profile_enable(ppbo_ctx* ctx, int on);
PPBO_API int ppbo_profile_reset(ppbo_ctx* ctx);
PPBO_API int ppbo_profile_read(ppbo_ctx* ctx, const char* name, double* h_total_ms, int* h_count);

/* ---- K1: Gram matrix with the closed-form shrinkage --------------------
 * replaces GPModel.create_Gramian (src/gp_model.py:147-151) =
 * kernel(X,X,theta) (src/kernels.py:19-53) + regularize_covariance
 * (src/misc.py:71-88; SVD round trip == identity, shrink == (1-s)K + s tr(K)/N I).
 * d_X[N,D] -> d_Sigma[N,N]. */
PPBO_API int ppbo_gram(ppbo_ctx* ctx, int kernel_id, const double* d_X, int N, int D,
              const double h_theta[3], double shrink, double* d_Sigma, void* stream);

/* a-3 as its own operator: regularize_covariance(X, reg_level, pos_diag=True, jitter) of src/misc.py:71-88 applied
 * IN PLACE to any device matrix d_K[N, ldk] (gp_model.py:150 calls it on the raw Gramian; ppbo_gram fuses the same
 * closed form): negative diagonal entries -> jitter when pos_diag != 0, then K <- (1 - reg_level) K + reg_level tr(K)/N I
 * (sklearn.covariance.shrunk_covariance).  The SVD round trip of misc.py:79-80 is the identity and is not executed. */
PPBO_API int ppbo_regularize_covariance(ppbo_ctx* ctx, double* d_K, int N, int ldk, double reg_level, int pos_diag,
                               double jitter, void* stream);

/* measurement probe, not part of the path: a write-only pass over d_S[N,N] (32 x 128 tiles, 16-byte write-through
 * stores, the fastest store shape tools/store_floor.hip found): the ceiling of ANY Gram kernel at that N on this
 * chip.  bench.py times it beside ppbo_gram (`write_only_floor_*`) instead of quoting constants. */
PPBO_API int ppbo_store_floor(ppbo_ctx* ctx, double* d_S, int N, void* stream);

/* ---- K2: raw cross-covariance ------------------------------------------
 * replaces GPModel.create_Gramian_nonsquare (src/gp_model.py:153-155).
 * d_X1[n1,D], d_X2[n2,D] -> d_K[n1,n2] (row stride ldk >= n2). */
PPBO_API int ppbo_cross_cov(ppbo_ctx* ctx, int kernel_id, const double* d_X1, int n1,
                   const double* d_X2, int n2, int D, const double h_theta[3],
                   double* d_K, int ldk, void* stream);

/* ---- K6: dense SPD factor / inverse (fp64, hand-written blocked kernels) --
 * ppbo_potrf: in-place lower Cholesky of d_A[N,N] (upper triangle untouched).
 *   *h_info = 0 on success, k>0 if the leading minor of order k is not PD
 *   (LAPACK convention); return value PPBO_ERR_NOT_PD in that case.
 * ppbo_pd_inverse replaces misc.pd_inverse (src/misc.py:96-100): d_Ainv = A^-1
 *   (full symmetric matrix written). */
PPBO_API int ppbo_potrf(ppbo_ctx* ctx, double* d_A, int N, int lda, int* h_info, void* stream);
PPBO_API int ppbo_pd_inverse(ppbo_ctx* ctx, const double* d_A, int N, double* d_Ainv, int* h_info, void* stream);

/* ppbo_pd_inverse that also hands out L^-1 (A = L L^T, full matrix, zeros above the diagonal); d_Linv may be NULL */
PPBO_API int ppbo_pd_inverse_factors(ppbo_ctx* ctx, const double* d_A, int N, double* d_Ainv, double* d_Linv, int* h_info,
                            void* stream);
/* ... and, when d_L is not NULL, the Cholesky factor itself: d_L[N,N], lower triangle = L, the strict upper triangle
 * is a copy of A's and is never read by this library.  L is what ppbo_fit_fmap_whitened iterates with, and
 * L z (ppbo_dgemv, lower = 1) is the prior draw of src/gp_model.py:374,381.  d_L and d_Linv may each be NULL. */
PPBO_API int ppbo_pd_inverse_ex(ppbo_ctx* ctx, const double* d_A, int N, double* d_Ainv, double* d_L, double* d_Linv,
                       int* h_info, void* stream);

/* ---- f-4: the inverse after one query has been appended --------------------------------
 * FeedbackProcessing.update_X (src/feedback_processing.py:133-154) only ever APPENDS the m+1 rows of the
 * new query, so Sigma_new = [[Sigma_old, B], [B^T, C]] with Sigma_old unchanged.  Instead of the reference's
 * full refactorisation (update_Sigma_inv -> pd_inverse, src/gp_model.py:161-162) the Cholesky factor is
 * bordered and the inverse follows from it -- through L^-1 (condition sqrt(cond Sigma)), never through
 * Sigma_old^-1 B (bordering the explicit inverse loses cond(Sigma) * eps relative to the tiny Schur complement):
 *   Y = L11^-1 B,  S = C - Y^T Y = L22 L22^T,  X = L22^-1 Y^T L11^-1  (k x N1, k = N - N1 <= 64),
 *   L_new^-1 = [[L11^-1, 0], [-X, L22^-1]],
 *   Sigma_new^-1 = [[Sigma_old^-1 + X^T X, -X^T L22^-1], [-L22^-T X, L22^-T L22^-1]].
 * d_A[N,N] is the new matrix; d_A11inv / d_L11inv [N1,N1] (row stride N1) the inverse of its leading block and of
 * that block's Cholesky factor (from ppbo_pd_inverse_factors or a previous append); d_Ainv / d_Linv [N,N] the
 * results.  PPBO_ERR_NOT_PD (info = failing column of A) when S is not positive definite. */
PPBO_API int ppbo_pd_inverse_append(ppbo_ctx* ctx, const double* d_A, int N, const double* d_A11inv, const double* d_L11inv,
                           int N1, double* d_Ainv, double* d_Linv, int* h_info, void* stream);
/* ... that also borders the factor itself: d_L11[N1,N1] (row stride N1, lower triangle = factor of the leading block,
 * as ppbo_pd_inverse_ex or a previous call returned it) -> d_L[N,N] = [[L11, 0], [Y^T, L22]], so the appended design
 * can go straight into ppbo_fit_fmap_whitened.  d_L11 and d_L are both NULL or both given. */
PPBO_API int ppbo_pd_inverse_append_ex(ppbo_ctx* ctx, const double* d_A, int N, const double* d_A11inv, const double* d_L11inv,
                              const double* d_L11, int N1, double* d_Ainv, double* d_Linv, double* d_L, int* h_info,
                              void* stream);

/* ---- K5: Laplace terms of the projective-preference likelihood -----------
 * replaces sum_Phi/sum_Phi_vec (src/gp_model.py:176-218), the likelihood part of
 * T (:221-226), beta of T_grad (:234-238) and create_Lambda (:249-274).
 * Design contract (src/feedback_processing.py:110-130): N = n_q (m+1); row
 * q(m+1) is the observation of query q, the next m rows its pseudo-observations.
 * Outputs (any may be NULL): d_Tlik[1] = -(1/m) sum_q sum_j Phi(Delta_qj/sqrt2);
 * d_beta[N]; d_lam_diag[N], d_lam_off[N] = Lambda in star-graph form
 * (off[j] = Lambda[obs(j), j] for pseudo rows, 0 on observation rows). */
PPBO_API int ppbo_laplace_terms(ppbo_ctx* ctx, const double* d_f, int N, int m, double sigma,
                       double* d_Tlik, double* d_beta, double* d_lam_diag,
                       double* d_lam_off, void* stream);

/* sum_Phi_vec(order_of_derivative, f, sigma) of src/gp_model.py:206-218 (sum_Phi :176-204 is one element of it):
 * d_out[q] for the n_q = N/(m+1) queries, order 0 = sum_j Phi(Delta_qj/sqrt2) (closed form of the Gauss-Hermite
 * integral at :192), 1 = sum_j var2_normal_pdf(Delta_qj), 2 = sum_j -Delta_qj/2 var2_normal_pdf(Delta_qj);
 * any other order is an argument error (the reference prints and returns None). */
PPBO_API int ppbo_sum_phi(ppbo_ctx* ctx, const double* d_f, int N, int m, double sigma, int order, double* d_out,
                 void* stream);

/* ---- a-8: f_MAP by trust-region Newton -----------------------------------
 * replaces GPModel.update_fMAP's scipy.optimize.minimize(method='trust-exact')
 * (src/gp_model.py:354-389) for ONE start vector d_f_init[N].
 * Radius rules follow SciPy's trust-region driver (initial 1, max 1000,
 * eta 0.15); the subproblem is a More-Sorensen iteration on device Cholesky
 * factors.  Stops when |grad T|_2 < gtol or after maxiter outer iterations. */
typedef struct ppbo_fit_opts {
  double gtol;    /* reference default 1e-4 (SciPy); 100 during initialisation (src/gp_model.py:365-366) */
  int maxiter;    /* <=0: 200*N like SciPy */
  int verbose;
  double initial_radius;   /* first trust radius; <= 0: SciPy's default 1.0 (what the reference runs with) */
  int lbfgs_max_evals;     /* ppbo_fit_fmap_whitened: evaluation budget of the whitened pre-phase; <= 0: 4000 */
  int judge_by_gradient_below_noise;  /* 0 (what ppbo_fit_fmap's callers pass): SciPy trust-exact's acceptance and
                            * radius rules throughout (actual / predicted decrease).  1 (set internally by
                            * ppbo_fit_fmap_whitened for its finishing phase): a step whose predicted decrease is below
                            * the rounding noise of the objective difference is accepted when it lowers |grad| --
                            * next to the optimum actual / predicted is a random number */
  int start_is_whitened;   /* ppbo_gp_fit only: d_f_init holds z0 (e.g. the standard-normal draw itself) and the search
                            * starts at f = L z0 -- the reference's prior draw N(0, Sigma) (src/gp_model.py:374,381)
                            * without forming it and whitening it again */
} ppbo_fit_opts;
typedef struct ppbo_fit_stats {
  int iterations;   /* outer trust-region iterations */
  int n_cholesky;   /* factorizations attempted */
  int converged;    /* 1 if |grad| < gtol */
  double T;         /* T(f_MAP) (src/gp_model.py:221-226) */
  double gradnorm;  /* |grad T(f_MAP)|_2 */
  int lbfgs_iterations; /* ppbo_fit_fmap_whitened: accepted quasi-Newton steps of the whitened pre-phase (else 0) */
  int lbfgs_evals;      /* ... its objective/gradient evaluations (each O(N^2): two products with L, one with Sigma^-1) */
  int lbfgs_status;     /* ... how it ended: 1 |grad T| < gtol, 2 rounding floor, 3 line search failed, 4 non-finite
                         * start, 5 budget spent, 6 the factor does not exist (Sigma not positive definite: ppbo_gp_fit
                         * returns PPBO_ERR_NOT_PD); -1 when the pre-phase did not run */
} ppbo_fit_stats;
PPBO_API int ppbo_fit_fmap(ppbo_ctx* ctx, const double* d_Sigma_inv, int N, int m, double sigma,
                  const double* d_f_init, const ppbo_fit_opts* opts, double* d_fMAP,
                  ppbo_fit_stats* h_stats, void* stream);

/* ---- a-8, the production path: the same minimiser found in the prior-whitened variable ------------------
 * replaces the same call (src/gp_model.py:354-389, scipy trust-exact on f) for ONE start vector.
 * With Sigma = L L^T (d_L from ppbo_pd_inverse_ex, row stride ldl) and f = L z,
 *   -T(L z) = 1/2 |z|^2 + (1/m) sum_q sum_j Phi(Delta_qj / sqrt2)
 * has the Hessian I - L^T Lambda L, free of cond(Sigma) ~ 1e7: a device-resident L-BFGS (history 8, Armijo /
 * approximate-Wolfe acceptance) needs tens of O(N^2) evaluations where the trust-region Newton on f needs
 * tens of O(N^3) factorizations.  It stops on the reference's own rule |grad_f T|_2 < gtol; whatever is left
 * (a request below the rounding floor of the whitened iteration, a stalled line search) is finished by
 * ppbo_fit_fmap from the point reached, so the result satisfies exactly what ppbo_fit_fmap's does.
 * Same optimum as the reference on every golden fixture; the PATH (and hence, on a multi-modal posterior, which
 * local maximum is found) is not SciPy's. */
PPBO_API int ppbo_fit_fmap_whitened(ppbo_ctx* ctx, const double* d_L, int ldl, const double* d_Sigma_inv, int N, int m,
                           double sigma, const double* d_f_init, const ppbo_fit_opts* opts, double* d_fMAP,
                           ppbo_fit_stats* h_stats, void* stream);

/* ---- a-1 ... a-8 + the posterior in ONE call: what GPModel.update_model does between update_data and mu_star ----
 * replaces update_Sigma + update_Sigma_inv + update_fMAP (one trial from d_f_init) + create_Lambda + the posterior
 * covariance (src/gp_model.py:91-117) -- i.e. ppbo_gram, ppbo_pd_inverse_ex, ppbo_fit_fmap_whitened and
 * ppbo_posterior behind one entry, with what that allows:
 *   - the start is whitened with the factor's inverse that is at hand anyway (z0 = L^-1 f_init: one triangular product);
 *   - no host wait between the phases: the two factorizations' info words and the search's state are read once, at
 *     the end (the search itself is steered through a host-mapped progress word, not through stream synchronisation);
 *   - with start_is_whitened and N >= 1024 the triangular inverse and Sigma^-1 -- which the search does not need until
 *     its |grad_f T| rule is armed -- are formed on a second stream owned by the ctx beside the first evaluations; the
 *     search's stream joins it at a fixed slot (PPBO_FIT_GF_FROM, default 8), the first evaluation that may apply the
 *     |grad_f T| rule.  That slot -- not the stream layout -- is what the result depends on: with start_is_whitened and
 *     N >= 1024 the rule is armed from the same evaluation in the one-stream form (PPBO_FIT_OVERLAP=0) too, so the two
 *     forms agree bit for bit for every start; without start_is_whitened, or below N = 1024, the rule is armed from
 *     the first evaluation.  Everything (both streams) is complete when the call returns.
 *   - a Sigma that is not positive definite ends the search before its first evaluation (the factorization's info word
 *     is read on the device by the search's first launch): the search performs no evaluation and the call returns
 *     PPBO_ERR_NOT_PD without a posterior phase.  The inverse pipeline that was enqueued behind the factorization
 *     (triangular inverse, Sigma^-1, the start product) still runs to completion on the half-factored matrix; its
 *     outputs (d_Sigma_inv, d_L, d_Linv, d_fMAP) are undefined in that case.
 * Outputs (device, caller-owned): d_Sigma [N,N] (NULL to skip), d_Sigma_inv [N,N], d_L [N,N] (Cholesky factor of
 * Sigma, lower triangle valid), d_Linv [N,N] (NULL: kept in a workspace), d_fMAP [N], and -- all four or none --
 * d_alpha, d_lam_diag, d_lam_off [N], d_G [N,N] as ppbo_posterior defines them (form: as there).
 * Returns PPBO_ERR_NOT_PD with *h_info = 1 when Sigma is not positive definite, *h_info = 2 when Sigma^-1 - Lambda_MAP
 * is not (f_MAP and the factors of Sigma are valid then; the reference prints its '---!!!---' line and keeps the
 * previous posterior, src/gp_model.py:118-120). */
PPBO_API int ppbo_gp_fit(ppbo_ctx* ctx, int kernel_id, const double* d_X, int N, int D, const double theta[3], double shrink,
                int m, const double* d_f_init, const ppbo_fit_opts* opts, double* d_Sigma, double* d_Sigma_inv,
                double* d_L, double* d_Linv, double* d_fMAP, double* d_alpha, double* d_lam_diag, double* d_lam_off,
                double* d_G, int form, ppbo_fit_stats* h_stats, int* h_info, void* stream);

/* T(f) and grad T(f) for a given f (src/gp_model.py:221-240); h_T / d_grad may be NULL */
PPBO_API int ppbo_T_and_grad(ppbo_ctx* ctx, const double* d_Sigma_inv, const double* d_f, int N, int m,
                    double sigma, double* h_T, double* d_grad, void* stream);

/* ---- posterior state for prediction ---------------------------------------
 * replaces update_model's tail (src/gp_model.py:111-117) and the per-call
 * A = Sigma^-1 - Sigma^-1 P Sigma^-1 of mu_Sigma_pred (:449).  With
 * W = -Lambda_MAP, B = Sigma^-1 + W = L_B L_B^T, R = L_B^-1:
 *   d_alpha[N] = Sigma^-1 f_MAP;  d_G[N,N] = R W (block lower triangular);
 *   k*^T A k* = k*^T W k* - |G k*|^2   (Woodbury; identical operator).
 * form = PPBO_FORM_NODE writes that G; PPBO_FORM_EDGE writes H, the same operator in edge coordinates ("the variance
 * operator in EDGE form" below) -- hand the same value on as ppbo_model.form.  Any other value is refused.
 * d_P (optional, may be NULL) = posterior_covariance = B^-1 (src/gp_model.py:117), whatever the form.
 * Returns PPBO_ERR_NOT_PD when B is not positive definite (the reference prints
 * '---!!!--- Posterior covariance matrix is not PSD ---!!!---' and continues). */
PPBO_API int ppbo_posterior(ppbo_ctx* ctx, const double* d_Sigma_inv, const double* d_fMAP, int N, int m,
                   double sigma, double* d_alpha, double* d_lam_diag, double* d_lam_off,
                   double* d_G, double* d_P, int form, int* h_info, void* stream);

/* ---- K2+K3+K4: batched candidate scoring with on-device argmax ------------
 * replaces mu_pred (src/gp_model.py:454-458) / diag of mu_Sigma_pred (:441-452)
 * called once per candidate by mu_star's differential evolution (:415-437) and
 * by EI/varmax (src/acquisition.py:72-81,170-178).
 * d_Xc[M,D] candidates in [0,1]^D.  Outputs (NULL to skip): d_mu[M], d_var[M],
 * d_score[M]; h_best_val / h_best_idx = max score and its FIRST index
 * (np.argmax semantics).  d_G may be NULL when only the mean is wanted.
 * A candidate row with any NaN or infinite coordinate gets NaN in d_mu, d_var and d_score and never wins the argmax (the
 * finite rows are scored exactly as without it); when no row has a non-NaN score, h_best_idx = -1 and h_best_val = NaN.
 * Any N = n_q (m + 1), any m, any M: where N is not a multiple of the 128-row tile / 16-deep chunk of the variance
 * contraction (m = 25, the reference's default) the call works on a zero-framed copy of G in a ctx workspace (from
 * 2048 candidates on; ~3 N^2 x 8 bytes moved per call), and K* is always padded to whole 128-candidate tiles. */
enum { PPBO_FORM_NODE = 0, PPBO_FORM_EDGE = 1 };   /* the two layouts of a variance operator: "EDGE form" below */

/* ---- the coordinate map of a model (ABI 8; no reference counterpart) -----------------------------------------------------
 * A model with per-dimension length scales holds rows in coordinates other than the caller's.  Which ones is data of the
 * model -- ppbo_model.coords -- not a function name and not state of the ctx: rows read with the wrong map, or with none,
 * give a finite, plausible and wrong maximiser.
 * PPBO_COORDS_MODEL (0, a zero-initialised struct): the caller's coordinates are the model's; h_coef and d_Xc are not read.
 * PPBO_COORDS_SCALED, ARD for a radial kernel (SE, RQ, Matern-5/2, Matern-3/2): k(x, x'; l_1..l_D) = k(s (.) x, s (.) x';
 *   l = 1) with s_d = 1 / l_d, so the model holds its SCALED rows in d_X and theta = [sigma, 1, sigma_f]; h_coef = s[D].
 *   ppbo_scale_points (no reference counterpart): d_out[i,d] = d_in[i,d] * h_scale[d] for M rows of D (in place allowed).
 * PPBO_COORDS_CAMPHOR, camphor-copper with l_0..l_5 (x, y, z, alpha, beta, gamma; z is the non-periodic coordinate 2): SE
 *   with l = 1 on embedded rows e(x) in R^11,
 *     camphor(x, x'; l, sigma_f) = SE(e(x), e(x'); 1, sigma_f),   |e_d(x) - e_d(x')|^2 = 4 sin^2(pi (x_d - x'_d)) / l_d^2,
 *   column order (c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5) with c_d = cos(2 pi x_d) / l_d, s_d = sin(2 pi x_d) / l_d and
 *   z = x_2 / l_2.  The reference's kernel is l = (l, l, l + 0.05, l, l, l).  The model holds its EMBEDDED rows in d_X
 *   (D = 11), kernel_id = PPBO_KERNEL_SE and theta = [sigma, 1, sigma_f]; h_coef = l[6] and d_Xc[N,6] = its design rows in
 *   the caller's coordinates.
 *   ppbo_camphor_embed: d_out[M,11] = e(d_in[M,6]) for the length scales h_l[6] (one memory-bound pass; an output that
 *     overlaps the input is rejected, as is M beyond one launch grid, 2^31 - 1 blocks of 256 / 6 rows).
 *   ppbo_camphor_line_points: the embedded grid d_out[B*G,11] of the B lines x_b + alpha_g xi_b (d_xi, d_x [B,6]; d_alpha
 *     [G], or [B,G] with alpha_per_line), formed in the caller's coordinates; ppbo_line_acq takes it as d_grid[B,G,11]
 *     (d_out must not overlap the inputs).
 * Who reads it: ppbo_mean_grad, ppbo_mean_ascent and ppbo_mean_search_multi read model->coords; ppbo_rff_search,
 * ppbo_rff_search_multi and ppbo_path_search_multi, which have no model, take a `const ppbo_coords*` (NULL = the identity).
 * With a map, points, pool rotation, extra points, h_xprev, the [0,1]^D box, sep, tol, the returned points and gradients
 * are all in the caller's coordinates (D = 6 for CAMPHOR).  ppbo_mean_search refuses a map.  EVERY other entry that takes a
 * model (ppbo_predict*, ppbo_predict_pairs, ppbo_predict_cov, ppbo_line_acq*, ppbo_search_sharded) ignores coords, as the
 * fit and evidence entries know none: they take rows in the MODEL's coordinates (scaled or embedded by the caller).
 * "invalid argument", with nothing launched: a kind outside 0..2; SCALED with PPBO_KERNEL_CAMPHOR; CAMPHOR on a model that
 * is not SE at D = 11, or without d_Xc; a coefficient array that is NULL or has a non-positive or non-finite entry. */
enum { PPBO_COORDS_MODEL = 0, PPBO_COORDS_SCALED = 1, PPBO_COORDS_CAMPHOR = 2 };
typedef struct ppbo_coords {
  int kind;              /* PPBO_COORDS_* */
  const double* h_coef;  /* host, read during the call only.  SCALED: s[D] = 1 / l_d.  CAMPHOR: l[6] */
  const double* d_Xc;    /* CAMPHOR, model entries only: the design rows in the caller's coordinates [N,6] */
} ppbo_coords;

/* a projected variance operator T = Q^T H of one model ("the projected edge form" below; ABI 9: ppbo_model.proj) */
typedef struct ppbo_var_projection {
  const double* d_T;   /* [rows_padded][ld] */
  int rows;            /* r: rows of T in use; 0 = no projection */
  int rows_padded;     /* r rounded up to the 128-row tile */
  int ld;              /* row stride of d_T */
  double bound;        /* certified bound on var - var_projected >= 0, units of variance */
  double tol;          /* the tolerance it was built for, relative to sigma_f^2 */
} ppbo_var_projection;

typedef struct ppbo_model {
  int kernel_id, N, D, m;
  double theta[3];
  const double* d_X;        /* [N,D] */
  const double* d_alpha;    /* [N]   */
  const double* d_lam_diag; /* [N]  Lambda_MAP diagonal   */
  const double* d_lam_off;  /* [N]  Lambda_MAP star edges */
  const double* d_G;        /* [N,N] the variance operator in the layout `form` names: R W (ppbo_posterior) or H.
                             * Block lower triangular, and stored that way: every
                             * entry right of the last star that reaches into its row must be an explicit ZERO
                             * (ppbo_posterior / ppbo_gp_fit write them): the contractions round their K ranges up to
                             * whole 16-column chunks and read up to 15 of those zeros per row */
  int kstar_fp32;           /* 0: everything fp64 (the product path).  1: K* entries evaluated in fp32 from direct
                             * differences, all accumulation fp64 -- BASELINE config 5's "fp32 tolerance" variant;
                             * its error against the fp64 path is REPORTED (bench.py), it does not meet 1e-5 */
  const double* d_Gt;       /* optional (ABI 6): the TRANSPOSE of d_G as ppbo_transposed_G writes it.  Models of up to ~500
                             * rows are scored by one launch (csrc/fused.hip) whose matrix-core loop reads G transposed;
                             * NULL: the library forms the transpose in a workspace on every call (2-4 us) */
  int form;                 /* (ABI 7) what d_G holds: PPBO_FORM_NODE (0, so a zero-initialised model is a node-form one),
                             * G = R W as ppbo_posterior / ppbo_gp_fit write it with that form, or PPBO_FORM_EDGE, H = L22^-1
                             * ("the variance operator in EDGE form" below); it must be the form the operator was built
                             * with -- read by the other rule an operator gives a finite, plausible and wrong variance.
                             * d_Gt is not read for the edge form.  Any other value is refused ("invalid argument").
                             * Ignored where no operator is read: d_G == NULL, and the mean-only ppbo_mean_* entries */
  ppbo_coords coords;       /* (ABI 8) the coordinates d_X is in, relative to the caller's ("the coordinate map of a model"
                             * above); zero-initialised: the same */
  ppbo_var_projection proj; /* (ABI 9) the projected operator built for THIS model (ppbo_var_projection_build; "the projected
                             * edge form" below, which names the entries that read it); zero-initialised (rows == 0): none */
} ppbo_model;

/* The transpose of G = R Lambda in the layout the one-launch scoring kernel reads: d_Gt[rows][ld] with
 * rows = (N rounded up to 16) + 16, ld = (N rounded up to 32) + 32 (ppbo_transposed_G_shape), d_Gt[k][i] = d_G[i][k] for
 * i, k < N and zero elsewhere.  Form it once per fit and hand it over as ppbo_model.d_Gt.  No reference counterpart (G
 * itself replaces the dense A = Sigma^-1 - Sigma^-1 P Sigma^-1 of src/gp_model.py:449). */
PPBO_API int ppbo_transposed_G_shape(int N, int* rows, int* ld);
PPBO_API int ppbo_transposed_G(ppbo_ctx* ctx, const double* d_G, int N, double* d_Gt, void* stream);
PPBO_API int ppbo_predict(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M,
                 int score_kind, double mustar, double* d_mu, double* d_var, double* d_score,
                 double* h_best_val, int64_t* h_best_idx, void* stream);

/* The same scoring passes for ONE SHARD of a sharded candidate search: nothing comes back to the
 * host and nothing synchronises.  d_record[2] (device) receives (best score, index_offset + its FIRST row index as
 * a double, exact below 2^53) -- (NaN, -1) when no candidate has a non-NaN score -- i.e. exactly the 16-byte record
 * that ppbo_argmax_allgather_record / torch.distributed all-gather (written by the one-workgroup argmax launch that
 * ends the pass). */
PPBO_API int ppbo_predict_record(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M,
                        int score_kind, double mustar, int64_t index_offset, double* d_record, void* stream);

/* ---- duels: mean, variance and win probability of f(a) - f(b) for M pairs (no reference counterpart) ----------------
 * The likelihood of the model is a probit on differences of noisy utilities (src/gp_model.py:176-204, sum_Phi:
 * Phi((f_obs - f_j) / (sqrt2 sigma)) per pseudo-observation); this entry extends those lines from the fitted rows to
 * any two points under the Laplace posterior.  The reference itself never predicts a comparison: the only route there
 * is the dense M x M covariance of mu_Sigma_pred (:441-452).  With d = k(a, X) - k(b, X):
 *   mu_d  = d' alpha
 *   var_d = Var[f(a) - f(b)] = (2 sigma_f^2 - 2 k(a, b)) + d' Lambda d + |G d|^2   (the operator of ppbo_posterior on d)
 *   p     = P(a > b) = Phi(mu_d / sqrt(2 sigma^2 + max(var_d, 0))),  sigma = theta[0]
 * d is formed directly (both points against each design row in one instruction chain), so a near-tie keeps its digits,
 * a == b gives mu_d = var_d = 0 and p = 1/2 exactly, and swapping the sides negates mu_d bit for bit.  The prior term
 * 2 sigma_f^2 - 2 k(a, b) comes from the direct differences a - b in a form that does not cancel at small distances; it
 * is NOT shrunk (mu_Sigma_pred shrinks its M x M prior block by 1e-6).
 * d_Xa / d_Xb [M, D]: the two sides in the MODEL's coordinates, as ppbo_predict takes d_Xc (scaled rows of an ARD model,
 * embedded rows of a camphor model with per-coordinate length scales).  Outputs, each may be NULL: d_mu, d_var, d_prob,
 * d_score [M] (the quantity score_kind names) and h_best_val / h_best_idx, the largest score and its FIRST index; NaN
 * never wins, (NaN, -1) when nothing scored.  A pair with a NaN or infinite coordinate on either side gets NaN outputs.
 * PPBO_PAIR_MEAN with d_var == d_prob == NULL reads neither d_G nor Lambda and runs no contraction.  Pairs go in
 * chunks of 65536 through ppbo_predict's workspaces; both operator forms take the same three launches, whatever N.
 * "invalid argument": a NULL model, d_Xa or d_Xb; M outside 1 .. 2^31 - 1; an unknown score_kind; model->kstar_fp32 set
 * (fp64 only); a model without d_G (or Lambda) when the variance, the probability or a score other than the mean is
 * asked for. */
enum { PPBO_PAIR_MEAN = 0, PPBO_PAIR_VARIANCE = 1, PPBO_PAIR_PROB = 2 };
PPBO_API int ppbo_predict_pairs(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, const double* d_Xb, int64_t M,
                       int score_kind, double* d_mu, double* d_var, double* d_prob, double* d_score,
                       double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- slopes: mean, variance and sign probability of d/da f(x + a xi) at a = 0 for M rows (no reference counterpart) --
 * The infinitesimal form of a duel: does the utility rise when the query goes on from x along xi, and how sure is the
 * model.  The directional derivative of a GP is Gaussian; with the column
 *   g_j = d/da k(x + a xi, x_j) at a = 0 = 2 sigma_f^2 kappa'(rho_j^2) ((x - x_j).xi) / l^2     (k = sigma_f^2 kappa(rho^2),
 *         rho_j^2 = |x - x_j|^2 / l^2;  camphor-copper: g_j = -k_j ds_j/da, s its exponent, kernels.py:36-53)
 *   mu_s  = g' alpha
 *   var_s = prior + g' Lambda g + |G g|^2                            (the operator of ppbo_posterior on g)
 *   prior = xi' (d^2 k / dx dx')(x, x) xi = -2 kappa'(0) sigma_f^2 |xi|^2 / l^2: sigma_f^2 |xi|^2 / l^2 times 1 (SE, RQ),
 *           5/3 (Matern-5/2), 3 (Matern-3/2);  camphor-copper: sigma_f^2 (sum_{d != 2} 4 pi^2 xi_d^2 / l^2 + xi_2^2 / (l + 0.05)^2)
 *   p     = P(slope > 0) = Phi(mu_s / sqrt(max(var_s, 0)));  no noise term (a slope is not an observation);
 *           var_s = 0: the sign of mu_s decides, mu_s = 0 gives 1/2
 * The prior term is NOT shrunk (as in ppbo_predict_pairs).  x - x_j comes from direct differences and kappa' from a form
 * that is finite at 0, so x on a design row gives g_j = 0 for that row; xi = 0 gives (0, 0, 1/2) exactly; -xi negates
 * mu_s bit for bit and leaves var_s bitwise unchanged.
 * d_X / d_Xi [M, D]: points and directions in the MODEL's coordinates, as ppbo_predict_pairs takes its sides (an ARD
 * model: s . x and s . xi; embedded camphor rows: e(x) and J_e(x) xi).  Outputs, each may be NULL: d_mu, d_var, d_prob,
 * d_score [M] (the quantity score_kind names) and h_best_val / h_best_idx, the largest score and its FIRST index; NaN
 * never wins, (NaN, -1) when nothing scored.  A row with a NaN or infinite coordinate in x or xi gets NaN outputs; the
 * other rows do not see it.  PPBO_SLOPE_MEAN with d_var == d_prob == NULL reads neither d_G nor Lambda and runs no
 * contraction.  Rows go in chunks of 65536 through ppbo_predict's workspaces (kstar_slope_kernel, the quadform kernel of
 * ppbo_predict, slope_score_kernel); both operator forms take the same three launches, whatever N.  The K* launch is
 * timed under the "kstar" name of ppbo_profile_read.
 * "invalid argument": a NULL model, d_X or d_Xi; M outside 1 .. 2^31 - 1; an unknown score_kind; model->kstar_fp32 set
 * (fp64 only); a model without d_G (or Lambda) when the variance, the probability or a score other than the mean is
 * asked for. */
enum { PPBO_SLOPE_MEAN = 0, PPBO_SLOPE_VARIANCE = 1, PPBO_SLOPE_PROB = 2 };
PPBO_API int ppbo_predict_slopes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, const double* d_Xi, int64_t M,
                        int score_kind, double* d_mu, double* d_var, double* d_prob, double* d_score,
                        double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- gradients: mean and D x D covariance of grad f(x) for M points (no reference counterpart) --------------------------
 * The object the slopes are projections of: grad f(x) ~ N(m(x), C(x)) with xi' m = mu_s and xi' C xi = var_s of
 * ppbo_predict_slopes for every xi.  With the D columns g_d = d k(x, X) / d x_d of a point (radial kernels:
 * g_jd = c(r_j^2) (x_d - x_jd), ONE kernel-function evaluation per design row for all D of them)
 *   m_d  = g_d' alpha
 *   C_de = P_de + g_d' Lambda g_e + (G g_d)'(G g_e)                   (the operator of ppbo_posterior, bilinear)
 *   P    = (d^2 k / dx dx')(x, x), unshrunk and diagonal: the prior constant of ppbo_predict_slopes times I for the radial
 *          kernels, diag(sigma_f^2 (4 pi^2 / l^2, ..., 1 / (l + 0.05)^2 at d = 2, ...)) for camphor-copper
 * C is symmetric bit for bit.  d_X [M, D]: points in the MODEL's coordinates, as ppbo_predict_slopes takes them.  Outputs,
 * each may be NULL: d_mean [M, D], d_cov [M, D, D], d_score [M] and h_best_val / h_best_idx, the largest score and its
 * FIRST index; NaN never wins, (NaN, -1) when nothing scored (PPBO_GRAD_NONE scores nothing).  h_metric: NULL or D positive
 * weights w_d (host);  PPBO_GRAD_TRACE = sum_d w_d C_dd, PPBO_GRAD_NORM2 = sum_d w_d (m_d^2 + C_dd) = E |grad f|_w^2 (an ARD
 * caller passes s_d^2 and gets the score in its own coordinates).  A point with a NaN or infinite coordinate gets NaN in
 * all its outputs; the other points do not see it.  With d_cov == NULL and PPBO_GRAD_NONE the call reads neither d_G nor
 * Lambda and runs no contraction.  Points go in chunks of 512 (at most 512 x 64 columns, which the workspaces of the line
 * entries hold for every D) through kstar_grad_kernel (camphor-copper: its direct-difference form), the
 * Y = G K* product and line_cov_kernel of the line entries with the D columns of a point as one group, and
 * grad_finish_kernel; both operator forms, the projected operator is not offered.  ppbo_profile_read: "grad_kstar",
 * "line_y", "line_cov", "grad_finish".
 * "invalid argument": a NULL model or d_X; M outside 1 .. 2^31 - 1; an unknown score_kind; a metric entry that is not
 * positive and finite; model->kstar_fp32 set (fp64 only); a model without d_G (or Lambda) when the covariance or a score
 * is asked for. */
enum { PPBO_GRAD_NONE = 0, PPBO_GRAD_TRACE = 1, PPBO_GRAD_NORM2 = 2 };
PPBO_API int ppbo_predict_gradients(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, int64_t M,
                        const double* h_metric, int score_kind, double* d_mean, double* d_cov, double* d_score,
                        double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- curvatures: mean, variance and sign probability of d^2/da^2 f(gamma(a)) at a = 0 for M rows (no reference counterpart) --
 * The companion of a slope where the slope vanishes: is x a peak along xi, how sharp is it, and how sure is the model.
 * gamma is a path in the MODEL's coordinates with gamma(0) = x, gamma'(0) = xi, gamma''(0) = acc (d_Xa == NULL: straight
 * lines, acc = 0).  The second directional derivative of a GP is Gaussian; with the column
 *   c_j = d^2/da^2 k(gamma(a), x_j) at a = 0 = 2 c'(s_j) b_j^2 + c(s_j) (n2 + (x - x_j).acc)
 *         (radial kernels, k = sigma_f^2 kappa(rho^2): s_j = |x - x_j|^2 and b_j = (x - x_j).xi from direct differences,
 *         n2 = |xi|^2, c(s) = 2 dk/ds as in ppbo_predict_slopes, c'(s) = 2 d^2k/ds^2 -- with c0 of the device's KernParams
 *         SE: 2 c0^2 k;  RQ: 12 c0^2 sigma_f^2 / t^4, t = 1 + c0 s;  Matern-5/2: sigma_f^2 c0^4 e^(-c0 r) / 6; all finite at s = 0;
 *         camphor-copper, k = sigma_f^2 e^-s: c_j = k_j ((ds_j/da)^2 - d^2 s_j/da^2),
 *         d^2 s_j/da^2 = sum_{d != 2} 2 pi^2 c0 xi_d^2 cos 2 pi (x_d - x_jd) + 2 c1 xi_2^2)
 *   mu_c  = c' alpha
 *   var_c = prior + c' Lambda c + |G c|^2                            (the operator of ppbo_posterior on c)
 *   prior = Var[d^2/da^2 f(gamma(a))] = q4 n2^2 + q2 |acc|^2 (no cross term: the kernels are stationary);  q2 = -c(0), the
 *           constant of a slope's prior;  q4 = 12 kappa''(0) sigma_f^2 / l^4: sigma_f^2 / l^4 times 3 (SE), 9/2 (RQ),
 *           25 (Matern-5/2);  camphor-copper: sigma_f^2 (12 A^2 + 8 pi^4 c0 sum_{d != 2} xi_d^4),
 *           A = sum_{d != 2} pi^2 c0 xi_d^2 + c1 xi_2^2
 *   p     = P(curvature < 0) = Phi(-mu_c / sqrt(max(var_c, 0)));  no noise term;  var_c = 0: the sign of mu_c decides,
 *           mu_c = 0 gives 1/2
 * The prior term is NOT shrunk (as in ppbo_predict_slopes).  Every term is of even degree in xi: with d_Xa NULL, xi = 0
 * gives (0, 0, 1/2) exactly, -xi leaves all three outputs bitwise unchanged, and for the radial kernels 2 xi gives
 * 4 mu_c and 16 var_c bit for bit.
 * d_X / d_Xi / d_Xa [M, D]: points, directions and accelerations in the MODEL's coordinates (an ARD model: s . x and
 * s . xi, straight lines stay straight; embedded camphor rows: e(x), J_e(x) xi and d^2 e(x + a xi) / da^2).  Outputs, each
 * may be NULL: d_mu, d_var, d_prob, d_score [M] (the quantity score_kind names) and h_best_val / h_best_idx, the largest
 * score and its FIRST index; NaN never wins, (NaN, -1) when nothing scored.  A row with a NaN or infinite coordinate in
 * x, xi or acc gets NaN outputs; the other rows do not see it.  PPBO_CURV_MEAN with d_var == d_prob == NULL reads
 * neither d_G nor Lambda and runs no contraction.  Rows go in chunks of 65536 through ppbo_predict's workspaces
 * (kstar_curv_kernel, the quadform kernel of ppbo_predict, curv_score_kernel); both operator forms take the same three
 * launches, whatever N.  The K* launch is timed under the "kstar" name of ppbo_profile_read.
 * "invalid argument": everything ppbo_predict_slopes refuses (a NULL model, d_X or d_Xi; M outside 1 .. 2^31 - 1; an
 * unknown score_kind; model->kstar_fp32; a model without d_G or Lambda when more than the mean is asked for);
 * PPBO_KERNEL_MATERN32 (a sample path of that kernel is differentiable once only: c'(s) ~ 1 / sqrt(s), no finite variance);
 * d_Xa with D > 16 or with PPBO_KERNEL_CAMPHOR (there the caller's coordinates are the model's: lines are straight). */
enum { PPBO_CURV_MEAN = 0, PPBO_CURV_VARIANCE = 1, PPBO_CURV_PROB = 2 };
PPBO_API int ppbo_predict_curvatures(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, const double* d_Xi,
                        const double* d_Xa, int64_t M, int score_kind, double* d_mu, double* d_var, double* d_prob,
                        double* d_score, double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- averages and contrasts: mean, variance and sign of L f = sum_g w_g f(x_g) for M groups of G points ---------------
 * The general linear functional of the utility over a small group of points (no reference counterpart: the only route
 * there is w' Sigma w through the dense covariance of mu_Sigma_pred, :441-452).  Averages (all weights 1 / G: the
 * utility of a design under implementation tolerance, along a segment, over contexts) and contrasts (sum w = 0: is
 * shortlist A better than shortlist B on average, is x better than the mean of its neighbours, any difference
 * stencil).  With the column c = sum_g w_g k(x_g, X):
 *   mu  = c' alpha
 *   var = w' K w + c' Lambda c + |G c|^2                             (the operator of ppbo_posterior on c)
 *   w' K w = sigma_f^2 (sum_g w_g)^2 - 2 sum_{g < h} w_g w_h (sigma_f^2 - k(x_g, x_h)),  the bracket from the direct
 *           differences x_g - x_h in the non-cancelling form of ppbo_predict_pairs' prior term; NOT shrunk
 *   p   = P(L f > threshold) = Phi((mu - threshold) / sqrt(max(var, 0)));  no noise term (as for slopes);
 *           var = 0: the sign of mu - threshold decides, equality gives 1/2
 * ONE contraction per group, whatever G is.  Every point of a group meets a design row in the same instruction chain
 * and the column is accumulated as fma(w_g, k, c) in the order of g: two identical points get the same kernel bits
 * (G = 2, w = (1, -1), a == b gives (0, 0, 1/2) exactly), all-zero weights give (0, 0, 1/2), -w negates mu bit for bit
 * and leaves var bitwise unchanged, 2 w gives exactly 2 mu and 4 var.  No atomics and a fixed order of every sum: a
 * call is bitwise repeatable and a group's results do not depend on its place in the call.
 * d_Xg [M, G, D]: the groups in the MODEL's coordinates, as ppbo_predict_pairs takes its sides.  d_w: the weights,
 * w_stride = 0: one row w[G] for all groups, w_stride = G: w[M, G].  Outputs, each may be NULL: d_mu, d_var, d_prob,
 * d_score [M] (the quantity score_kind names) and h_best_val / h_best_idx, the largest score and its FIRST index; NaN
 * never wins, (NaN, -1) when nothing scored.  A group with a NaN or infinite coordinate gets NaN outputs whatever its
 * weights; the other groups do not see it.  PPBO_FUNCTIONAL_MEAN with d_var == d_prob == NULL reads neither d_G nor
 * Lambda and runs no contraction.  Groups go in chunks of 65536 through ppbo_predict's workspaces (kstar_func_kernel on
 * the fp64 matrix cores -- camphor-copper, id 2: a vector kernel in the feature form --, the quadform kernel of
 * ppbo_predict, functional_score_kernel); both operator forms take the same three launches, whatever N.  The K* launch
 * is timed under the "kstar" name of ppbo_profile_read.
 * "invalid argument": everything ppbo_predict_pairs refuses (a NULL model; M outside 1 .. 2^31 - 1; an unknown
 * score_kind; model->kstar_fp32; a model without d_G or Lambda when more than the mean is asked for); a NULL d_Xg or
 * d_w; G outside 1 .. PPBO_FUNCTIONAL_MAX_G; w_stride other than 0 or G; a threshold that is not finite. */
#define PPBO_FUNCTIONAL_MAX_G 64
enum { PPBO_FUNCTIONAL_MEAN = 0, PPBO_FUNCTIONAL_VARIANCE = 1, PPBO_FUNCTIONAL_PROB = 2 };
PPBO_API int ppbo_predict_functionals(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xg, const double* d_w,
                        int w_stride, int64_t M, int G, double threshold, int score_kind, double* d_mu, double* d_var,
                        double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- main effects and interactions: f with all but at most two coordinates averaged over the unit box ------------------
 * The global companion of the local entries above (no reference counterpart: its plots, camphor_copper/plot_results.py, are
 * two-dimensional SLICES through x*).  Which coordinates matter, how does the utility depend on coordinate d once the
 * others are averaged out, do d and e interact.  The SE kernel (scalar or per-dimension length scales) and the
 * camphor-copper kernels are PRODUCTS over the caller's unit-box coordinates,
 *   k(x, x') = sigma_f^2 prod_d kappa_d(x_d - x'_d),   kappa_d(D) = exp(-D^2 / (2 l_d^2))            (an SE axis)
 *                                                      kappa_d(D) = exp(-2 sin^2(pi D) / l_d^2)      (a periodic axis)
 * so the average of k(x, x_j) over [0,1] in any subset of coordinates is closed form, and a main effect or an
 * interaction is one more linear functional with an exactly known column: nothing is sampled, no quadrature size.
 *   I_d(c) = int_0^1 kappa_d(u - c) du = l sqrt(pi/2) (erf((1 - c) / (sqrt2 l)) + erf(c / (sqrt2 l)))   | e^-a I0(a), a = 1 / l^2
 *   A_d    = int int kappa_d(u - u') du du' = 2 (l sqrt(pi/2) erf(1 / (sqrt2 l)) - l^2 (1 - e^(-1/(2 l^2))))   | e^-a I0(a)
 * Per design row j: Q_jd = I_d(x_jd), P_j = sigma_f^2 prod_d Q_jd (the product in axis order).  A row of the call keeps the
 * axes J (|J| = 0, 1 or 2) at the values t: r_d = kappa_d(t_d - x_jd) / Q_jd for d in J.  With S = sigma_f^2 prod_{d not in J} A_d,
 * a_d = I_d(t_d) and b_d = 1 - 2 a_d + A_d:
 *   PPBO_EFFECT_RAW          L f = f_J(t) = int f dx_{-J}           c_j = P_j prod_J r_d           prior = S
 *   PPBO_EFFECT_CENTRED      f_J(t) - fbar, fbar = int f dx         c_j = P_j (prod_J r_d - 1)     prior = S (1 - 2 prod_J a_d + prod_J A_d)
 *   PPBO_EFFECT_INTERACTION  f_de - f_d - f_e + fbar  (|J| = 2)     c_j = P_j (r_d - 1)(r_e - 1)   prior = S b_d b_e
 *   mu = c' alpha,   var = prior + c' Lambda c + |G c|^2 (the operator of ppbo_posterior on c, as ppbo_predict_functionals),
 *   p = P(L f > 0) = Phi(mu / sqrt(max(var, 0)));  no noise term;  var = 0: the sign of mu decides, mu = 0 gives 1/2
 * A utility learned from preferences is defined up to a constant: CENTRED and INTERACTION are the identifiable ones.
 * An order-0 row under CENTRED is the zero functional and gives (0, 0, 1/2) exactly.
 * axes: Dc caller coordinates (the model's D; 6 for PPBO_KERNEL_CAMPHOR and for a PPBO_COORDS_CAMPHOR model), d_Xu[N, Dc]
 * the design rows in those unit-box coordinates -- BEFORE the scaling of an ARD model or the camphor embedding --, and on
 * the host l[Dc], periodic[Dc] (0: an SE axis, 1: a periodic one) and I0[Dc] = e^-a I0(a) of the periodic axes (the
 * scaled Bessel function, scipy.special.ive(0, a): never a product of two factors; used on the periodic axes only, but
 * every entry must be positive and finite).  The host
 * arrays are consumed before the call returns.  From the model the entry reads alpha, Lambda, G, form, N, m and sigma_f
 * (theta[2]); the column is formed from `axes`, NOT from model->d_X.  THE LIBRARY DOES NOT CHECK that d_Xu are the rows the
 * model was fitted on, nor that l and periodic are its kernel's: other rows give a finite, plausible and wrong answer.
 * d_dims [M, 2] (int): the kept axes of a row, -1 = unused: (-1, -1) order 0, (d, -1) order 1, (d, e) order 2.  d_t [M, 2]:
 * their values (not read where the axis is -1).  A row's two axes are processed in ascending axis order whatever order
 * the caller gave them: (d, e, t, u) and (e, d, u, t) give the same bits.  Every sum has a fixed order and there are no
 * atomics: a call is bitwise repeatable, and a row's results depend neither on its place in the call nor on M (the row
 * splits are those of a full chunk).
 * score_kind (PPBO_PAIR_*: mean, variance, probability), the outputs (each may be NULL), the argmax record, the chunks of
 * 65536 rows and the NaN rule are ppbo_predict_pairs': a row with a NaN or infinite t on a kept axis gets NaN outputs
 * and never wins; the other rows do not see it.  The mean alone (d_var == d_prob == NULL) reads neither d_G nor Lambda.
 * Launches: marginal_table_kernel once per call (1 / Q and P), then per chunk kstar_marginal_kernel, the quadform kernel
 * of ppbo_predict, marginal_score_kernel; the K* launch is timed under the "kstar" name of ppbo_profile_read.
 * "invalid argument", nothing written to an output, the context still usable: everything ppbo_predict_pairs refuses; a
 * kernel id other than PPBO_KERNEL_SE and PPBO_KERNEL_CAMPHOR (RQ and the Matern kernels are radial, not products: sample
 * the box with ppbo_predict_functionals); a NULL axes, d_Xu, h_l, h_periodic, h_I0, d_dims or d_t; Dc outside 1 .. 64 or
 * not the model's; an l or an I0 that is not positive and finite (on any axis); a periodic flag other than 0 / 1;
 * an unknown effect; and, looked for on the device before the first launch that writes an output (one small launch and a
 * wait on the host-mapped record), a row of d_dims with an axis outside -1 .. Dc - 1, with d == e >= 0, with a first axis
 * of -1 and a second >= 0, or of order below 2 under PPBO_EFFECT_INTERACTION.  On a stream that is being captured the host
 * cannot wait: there the look is left out and such a row gets NaN outputs. */
typedef struct ppbo_marginal_axes {
  int Dc;                  /* caller coordinates: D, or 6 for the camphor kernels; 1 .. 64 */
  const double* d_Xu;      /* [N,Dc] the design rows in unit-box caller coordinates */
  const double* h_l;       /* [Dc] length scales */
  const int* h_periodic;   /* [Dc] 0 SE axis, 1 camphor periodic axis */
  const double* h_I0;      /* [Dc] e^-a I0(a), a = 1 / l^2, for the periodic axes */
} ppbo_marginal_axes;
enum { PPBO_EFFECT_RAW = 0, PPBO_EFFECT_CENTRED = 1, PPBO_EFFECT_INTERACTION = 2 };
PPBO_API int ppbo_predict_marginals(ppbo_ctx* ctx, const ppbo_model* model, const ppbo_marginal_axes* axes, const int* d_dims,
                        const double* d_t, int64_t M, int effect, int score_kind, double* d_mu, double* d_var,
                        double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- tournaments: every candidate a_i against every opponent b_j, win matrix and scores (no reference counterpart) ----
 * How does each of Ma candidates fare against a whole field of Mb opponents: the K x K win matrix of a shortlist, the
 * Borda (soft-Copeland) winner of preferential Bayesian optimisation, the candidate with the best chance against its
 * strongest opponent.  ppbo_predict_pairs on the Ma Mb explicit pairs pays one N^2 contraction per pair; the covariance
 * is bilinear, so none of that is needed.  With sigma^2(x) = sigma_f^2 + k*' Lambda k* + |M k*|^2, M = G in the node form
 * and M = H diag(w) D in the edge form ("the variance operator in EDGE form" below):
 *   cov(f(a), f(b)) = k(a, b) + k_a' u_b,   u_b = (Lambda + M'M) k_b
 *   var_d(a, b)     = var_a + var_b - 2 cov(a, b)
 *   p(a > b)        = Phi((mu_a - mu_b) / sqrt(2 sigma^2 + max(var_d, 0))),  sigma = theta[0]
 * The Mb opponents cost O(N^2 Mb) once per call (u_b for the whole field, in the row layout of the model's form), every
 * candidate the one contraction ppbo_predict pays for var_a, and all Ma x Mb cross terms are ONE Ma x N x Mb product on
 * the fp64 matrix cores whose epilogue adds the prior k(a, b) (direct differences) and forms cov, var_d and p in registers.
 * d_Xa [Ma, D], d_Xb [Mb, D]: the two sets in the MODEL's coordinates, as ppbo_predict_pairs takes its sides (scaled rows
 * of an ARD model, embedded rows of a camphor model with per-coordinate length scales).
 * Outputs, each may be NULL: d_mu_a, d_var_a [Ma] and d_mu_b, d_var_b [Mb], bit for bit what ppbo_predict gives for the
 * same set (the same launches); d_cov, d_prob [Ma, Mb] row-major -- nothing of size Ma Mb is formed unless asked for;
 * d_score [Ma], the quantity score_kind names:
 *   PPBO_TOURNAMENT_BORDA   (1 / Mb) sum_j p_ij, the chance of beating a random opponent of the field: summed in a FIXED
 *                           order (the 16 opponents of a lane group, the groups of a 128- or 32-column tile, then the
 *                           tiles in index order), so a repeated call is bitwise equal
 *   PPBO_TOURNAMENT_WORST   min_j p_ij, the chance against the strongest opponent
 * and h_best_val / h_best_idx, the largest score and its FIRST index; NaN never wins, (NaN, -1) when nothing scored.
 * A non-finite coordinate in a_i gives NaN in row i only (mu, var, cov, p, score).  A non-finite coordinate in b_j gives
 * NaN in column j and in EVERY row's score, sum and minimum alike: a NaN opponent poisons the field.
 * The a rows go in chunks of 65536 through ppbo_predict's workspaces; a row's cov, var_d and p depend on its own mu_a and
 * var_a and on the field only, so they follow ppbo_predict's own independence of the other rows of the call.
 * Accuracy: var_d is formed from the three terms var_a, var_b and cov, each accurate to ~1e-15 sigma_f^2 in ABSOLUTE
 * terms; it inherits that absolute accuracy, not the relative digits of a small difference.  For near-ties (a ~ b, where
 * var_d << sigma_f^2 and its relative digits decide p) ppbo_predict_pairs remains the tool: it forms the difference
 * column directly.  cov is clipped at (var_a + var_b) / 2, its bound from Var[f(a) - f(b)] >= 0, so var_d formed from
 * the outputs in that order is never negative, and a == b gives var_d = 0 and p = 1/2 wherever ppbo_predict gives
 * the point the same bits in both sets.
 * "invalid argument", with nothing launched: a NULL model, d_Xa or d_Xb; Ma outside 1 .. 2^31 - 1; Mb outside
 * 1 .. PPBO_TOURNAMENT_MAX_B (callers chunk the field); an unknown score_kind; model->kstar_fp32 set (fp64 only); a model
 * without d_G or Lambda; a form outside {PPBO_FORM_NODE, PPBO_FORM_EDGE}.
 * The launches of the cross product are timed as "tournament", the field pass as "tournament_field" (ppbo_profile_read). */
#define PPBO_TOURNAMENT_MAX_B 1024
enum { PPBO_TOURNAMENT_BORDA = 0, PPBO_TOURNAMENT_WORST = 1 };
PPBO_API int ppbo_predict_tournament(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, int64_t Ma,
                        const double* d_Xb, int Mb, int score_kind, double* d_mu_a, double* d_var_a, double* d_mu_b,
                        double* d_var_b, double* d_cov, double* d_prob, double* d_score, double* h_best_val,
                        int64_t* h_best_idx, void* stream);

/* ---- shortlists: q candidates picked greedily under the conditioned variance (no reference counterpart) ----------------
 * "The q configurations worth showing next": the producer of the point sets that the choice, ranking and tournament
 * predictions consume.  The q best values of ppbo_predict's d_score ignore the posterior correlation (q neighbours of one
 * basin); this entry conditions the GP on every pick before it takes the next (kriging believer / pivoted Cholesky).
 * Conditioning on "f(p) observed with noise tau^2 = noise_var" leaves the mean unchanged and subtracts a rank-one term
 * from the variance.  With mu, var_0 exactly ppbo_predict's for the same rows (the same launches, bit for bit), for
 * j = 0 .. q - 1:
 *   p_j        = the FIRST index of the largest score(mu[c], var_j[c]) over the candidates not picked yet (score_kind and
 *                mustar as in ppbo_predict); NaN never wins, and a picked index never scores again whatever tau is
 *   c_j[c]     = cov_{j-1}(c, p_j) = k(c, p_j) + k_c' u_{p_j} - sum_{i<j} V_i[c] V_i[p_j],  u_b = (Lambda + M'M) k_b  (the
 *                tournament's bilinear form; the prior term k(c, p_j) from direct differences, as in its epilogue)
 *   V_j[c]     = c_j[c] / sqrt(var_j[p_j] + tau^2);  V_j = 0 where that denominator is 0 (tau = 0, a zero-variance pick)
 *   var_j+1[c] = max(var_j[c] - V_j[c]^2, 0)
 * d_Xc [M, D]: the candidates in the MODEL's coordinates, as ppbo_predict_tournament takes its sets.
 * h_idx [q] = p_j and h_score [q] (may be NULL) = its score at the time of the pick; once nothing scoreable is left
 * (M < q, NaN rows) the remaining entries are (-1, NaN).  d_mu, d_var, d_var_cond [M], each may be NULL: mu, var_0 and
 * var_q.  A candidate with a non-finite coordinate has NaN mu, var and var_cond, is never picked and disturbs no other row.
 * score_kind: PPBO_SCORE_POINTWISE_EI or PPBO_SCORE_VARIANCE; PPBO_SCORE_MEAN is refused (the mean does not change under
 * this conditioning, so its shortlist is the q best values of d_score).
 * Stages: ppbo_predict's launches (mu, var_0, pick 0), then per pick a gather of the pick's row, its var_j and its
 * V_i[p_j] from the device-resident record, the tournament's field pass on that ONE row (O(N^2)), and ONE streaming pass
 * over the candidates' K* (batch_step_kernel: an M x N matrix-vector product, the downdate with the q x M doubles of
 * V, the new score and the block bests), then the one-workgroup argmax.  The whole loop is enqueued; the host waits once,
 * at the end, for one copy of the q records.  All reductions run in a fixed order without floating-point atomics: a
 * repeated call is bitwise equal.
 * Cost: M <= 65536 reuses the K* workspace that ppbo_predict's launches left (8 N M bytes read per pick; behind the
 * one-launch scoring path one K* launch of this entry's own forms it).  Above that every chunk's K* is formed AGAIN per
 * pick, into a workspace of this entry's own: q K* passes over all M candidates on top of the reads.  The workspace of
 * V is 8 q M bytes.  Without d_var_cond the last pick's pass is skipped (nobody reads var_q).
 * "invalid argument", with nothing launched: a NULL model, d_Xc or h_idx; M outside 1 .. 2^31 - 1; q outside
 * 1 .. PPBO_BATCH_MAX_Q; noise_var negative or not finite (a huge finite value is allowed: nothing is conditioned, the
 * picks are the q best scores in index order); a score_kind other than EI or VARIANCE; model->kstar_fp32 set (fp64 only);
 * a model without d_G or Lambda; a form outside {PPBO_FORM_NODE, PPBO_FORM_EDGE}.
 * The streaming passes are timed as "batch_step", the gathers and field passes as "batch_field" (ppbo_profile_read). */
#define PPBO_BATCH_MAX_Q 64
PPBO_API int ppbo_search_batch(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                        double mustar, double noise_var, int q, int64_t* h_idx, double* h_score, double* d_mu,
                        double* d_var, double* d_var_cond, void* stream);

/* ---- knowledge gradient: a candidate scored by what observing it does to the maximum of the mean (no reference counterpart) --
 * Users of the model take argmax mu as their answer.  Pointwise EI and the variance look at a candidate's own marginal;
 * the knowledge gradient for correlated beliefs (Frazier, Powell and Dayanik 2009) measures what an observation at a_i
 * would do to that answer: a point of small EI that is correlated with a broad basin can move the mean's maximum most.
 * The imagined observation is the shortlist's convention (ppbo_search_batch): "f(a_i) observed with noise tau^2 =
 * noise_var" -- a Gaussian observation of the latent value, NOT the answer to a preference query.  It moves the mean of
 * every point x by cov(a_i, x) Z / s_i, Z ~ N(0, 1).  For candidate a_i and the field B = {b_j}, j < Mb:
 *   v_i = max(var_i, 0),  s_i = sqrt(v_i + tau^2)
 *   lines    the field's, intercept mu(b_j) and slope cov(a_i, b_j) / s_i, and the candidate's own, intercept mu(a_i) and
 *            slope v_i / s_i: Mb + 1 beliefs about a mean after the observation
 *   h_i(z) = the largest of the lines at z
 *   KG_i   = E_Z[h_i(Z)] - h_i(0)  >= 0
 * The field should hold the current recommendation (argmax mu): without it h_i(0) understates the present answer and
 * KG is inflated.  With the lines of the upper envelope in order of slope, kinks c_k and slopes beta_k,
 *   KG_i = sum_k (beta_{k+1} - beta_k) psi(|c_k|),   psi(c) = phi(c) - c Phi(-c)
 * exactly: no quadrature.  s_i = 0 gives slopes 0 and KG_i = 0.
 *
 * ppbo_kg_envelope: lines in, KG out.  d_a [Mb]: the intercepts of the field lines, the same for every row; d_slope [Ma,
 * ld] row-major (ld >= Mb): their slopes per row; d_self_a, d_self_b [Ma]: each row's own line, both NULL for none.
 * d_kg [Ma]; d_kinks [Ma] (int32, may be NULL): the kinks of the row's envelope, at most (lines - 1); h_best_val /
 * h_best_idx: the largest KG and its FIRST row, (NaN, -1) when nothing scored.
 * A gift-wrapping march per row, a fixed group of 16 (Mb <= 256) or 64 lanes on it with the lines in registers: from the
 * line of the smallest slope (of equal slopes the largest intercept) to the steeper line that crosses the current one
 * first (of equal crossings the steepest, then the largest intercept), until no steeper line is left -- a counted loop of
 * at most (lines) passes.  Every reduction is a minimum or a maximum and the sum runs in march order, so a row's result
 * is a function of the SET of its lines: the order of the lines, duplicated lines and the other rows of the call change
 * no bit of it, and a repeated call is bitwise equal.
 * A row with a non-finite slope or own line gives NaN in that row only (kinks 0), and NaN never wins; a non-finite
 * intercept in d_a gives NaN in EVERY row (the tournament's rule: a NaN opponent poisons the field).
 * "invalid argument", with nothing launched: NULL d_a, d_slope or d_kg; Ma outside 1 .. 2^31 - 1; Mb outside
 * 1 .. PPBO_KG_MAX_B; ld < Mb; one of d_self_a / d_self_b without the other.
 *
 * ppbo_predict_kg: KG of the candidates d_Xa [Ma, D] over the field d_Xb [Mb, D], both in the MODEL's coordinates as
 * ppbo_predict_tournament takes its sets.  The tournament's stages unchanged -- ppbo_predict's launches on the field, the
 * field pass, then per chunk of 65536 candidates ppbo_predict's launches and the cross product on the fp64 matrix cores,
 * which writes the chunk's covariances [Mc, Mb] into a workspace of the ctx (8 Mc Mb bytes, 512 MB at the largest shape)
 * -- then s_i and the own slope per row, the envelope march (which divides the covariances by s_i as it loads them) and
 * the one-workgroup argmax.  Everything is enqueued; the host waits once, for the record.  cov is the tournament's,
 * clipped at (var_a + var_b) / 2.  A field point that IS candidate i -- the same D coordinates and the same mean, bit for
 * bit -- takes the own line's slope v_i / s_i: cov(a, a) is var(a), and the cross product sums that quadratic form in
 * another order than ppbo_predict does (a few ulp apart), which would leave two beliefs where there is one.  So a candidate
 * that is in the field scores as if its own point were not, and Mb = 1 with the field equal to the candidate gives
 * KG = 0 exactly.  d_mu_a, d_var_a [Ma], d_mu_b, d_var_b [Mb], each may be NULL: bit for bit ppbo_predict's.
 * d_kinks may be NULL.  A non-finite coordinate in a_i gives NaN in row i only; one in b_j gives NaN in every row.
 * "invalid argument", with nothing launched: ppbo_predict_tournament's refusals, a NULL d_kg, and a noise_var that is
 * negative or not finite.
 * The envelope launches are timed as "kg", the cross product as "tournament" (ppbo_profile_read). */
#define PPBO_KG_MAX_B 1024
PPBO_API int ppbo_kg_envelope(ppbo_ctx* ctx, const double* d_a, const double* d_slope, int64_t ld, const double* d_self_a,
                        const double* d_self_b, int64_t Ma, int Mb, double* d_kg, int* d_kinks, double* h_best_val,
                        int64_t* h_best_idx, void* stream);
PPBO_API int ppbo_predict_kg(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, int64_t Ma, const double* d_Xb,
                        int Mb, double noise_var, double* d_kg, int* d_kinks, double* d_mu_a, double* d_var_a,
                        double* d_mu_b, double* d_var_b, double* h_best_val, int64_t* h_best_idx, void* stream);

/* full predictive covariance of small sets (the G=70 line grid of EI):
 * d_cov[M,M] = (1-s)K(Xc,Xc) + s sigma_f^2 I - K*^T A K*  (src/gp_model.py:447-450) */
PPBO_API int ppbo_predict_cov(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int M,
                     double shrink, double* d_mu, double* d_cov, void* stream);

/* ---- f-2: posterior mean with its analytic gradient ----------------------------
 * d_mu[M] = K*^T alpha (src/gp_model.py:454-458), d_grad[M,D] = d mu / d x at d_Xc[M,D], both in the caller's
 * coordinates (model->coords).  SCALED: mu at s (.) x, d mu / d x_d = s_d d mu / d x~_d.  CAMPHOR (D = 6): the 11-D
 * gradient on e(x) pulled back through de/dx, 2 pi (c_d g_s - s_d g_c) for a periodic d, g_z / l_2 for z.
 * The reference has no gradient: mu_star (src/gp_model.py:415-437) maximises mu_pred by
 * differential evolution; the drop-in refines the best candidates of the batched search by a
 * multi-start ascent on these gradients instead.  Only kernel_id, N, D, theta, d_X, d_alpha and coords of
 * the model are read. */
PPBO_API int ppbo_mean_grad(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M,
                   double* d_mu, double* d_grad, void* stream);

/* ---- f-2, device-resident: the maximiser of the posterior mean ---------------------------------------
 * replaces GPModel.mu_star's differential evolution (src/gp_model.py:415-437: ~2 k ... 17 k sequential mu_pred
 * calls per trial) by one enqueue: score the M candidates (ppbo_predict, mean only), thin them to <= 4096 group
 * winners, pick the K best that are pairwise more than `sep` apart, and run a projected Barzilai-Borwein gradient
 * ascent from each -- the WHOLE iteration inside one kernel, one workgroup per start, no host round trip.
 * d_x[K,D] / d_mu[K]: the refined maxima (rows >= *h_found: mu = -inf).  h_found may be NULL (then nothing
 * synchronises).  ppbo_mean_ascent is the last stage alone, from caller-chosen starts (d_iters[K] optional).
 * The start selection, the same in every search of this library (tests/search_ref.py restates it in NumPy):
 *   - the survivor capacity is cap = clamp(147456 / (8 + 8 D), 64, 4096), rounded down (survivors and their coordinates
 *     in one workgroup's LDS); the M scored rows are cut into groups of G = ceil(M / cap) CONSECUTIVE rows, ceil(M / G)
 *     groups in all (the last one may be short);
 *   - a group's survivor is its first maximum (strict >: of equal scores the smaller row index wins); NaN never wins,
 *     and a group whose rows are all NaN or -inf yields no survivor;
 *   - then at most K greedy picks: each is the first maximum among the live survivors (ties again to the smaller
 *     index), and after it every live survivor with sum_d (x_d - x*_d)^2 <= sep^2 is struck -- inclusive, so a
 *     survivor exactly `sep` away goes, and so does the winner itself (sep = 0 strikes the winner and its duplicates);
 *     the picks stop early when no survivor above -inf is left, so *h_found may be less than K;
 *   - distances are plain Euclidean in the coordinates of d_cand (the caller's coordinates under a coordinate map).
 * iters = 0 returns the picked rows (clipped to the unit box) and the mean there.
 * ppbo_mean_search (one trial) has no form for a coordinate map: model->coords.kind != 0 is "invalid argument".
 * ppbo_mean_ascent under a map: starts, box, tol and results in the caller's coordinates; SCALED evaluates the mean at
 * s (.) x and scales its gradient by s, CAMPHOR evaluates mu and its gradient on d_Xc with the camphor form
 * s = sum_{d != 2} (2 / l_d^2) sin^2(pi dx_d) + dx_2^2 / (2 l_2^2).
 * ppbo_shift_points: d_out = frac(d_in + h_shift[D]) row-wise -- a rotation of a RESIDENT uniform candidate pool,
 * so that repeated searches see fresh candidates without regenerating and uploading M x D numbers. */
PPBO_API int ppbo_mean_search(ppbo_ctx* ctx, const ppbo_model* model, const double* d_cand, int64_t M, int K, double sep,
                     int iters, double tol, double* d_x, double* d_mu, int* h_found, void* stream);
PPBO_API int ppbo_mean_ascent(ppbo_ctx* ctx, const ppbo_model* model, const double* d_starts, int K, int iters, double tol,
                     double* d_x, double* d_mu, int* d_iters, void* stream);
PPBO_API int ppbo_shift_points(ppbo_ctx* ctx, const double* d_in, int64_t M, int D, const double* h_shift, double* d_out,
                      void* stream);

/* ALL trials of one mu_star call in one enqueue (src/gp_model.py:415-437: `mustar_finding_trials` differential-evolution
 * runs, 3 per iteration, 20 on the last).  Trial t scores the resident uniform pool d_pool[M,D] through its own rotation
 * frac(pool + h_shifts[t]) -- formed on the fly, nothing is written out -- and trial 0 also E_rows extra points
 * d_extra[E_rows,D] (NULL with E_rows = N: the model's own design points) and, when h_xprev[D] is given, the previous
 * x*; then, for all trials together: one thinning launch, one start-selection launch (a workgroup per trial), ONE ascent
 * launch of T K workgroups.  Against T calls of ppbo_mean_search on three contexts / streams: 3 trials at C3 2.2 -> 1.1 ms.
 * screen_fp32 = 1: the candidates are RANKED by a mean whose kernel values are evaluated in fp32 (packed fp32 math,
 * v_exp_f32; accumulated in fp64; relative error ~1e-6) -- every reported value and point comes from the fp64 ascent;
 * 0: ranked by the fp64 mean of ppbo_predict, as ppbo_mean_search does (bit-identical results to T such calls).
 * d_x[T,K,D], d_mu[T,K]: the refined maxima per trial (rows that found no start: mu = -inf).  Nothing synchronises.
 * Under a coordinate map (model->coords) d_extra = NULL with E_rows = N stands for the design in the caller's coordinates
 * (SCALED: the model's rows divided by s; CAMPHOR: d_Xc), and the candidates are screened on their scaled / embedded rows. */
PPBO_API int ppbo_mean_search_multi(ppbo_ctx* ctx, const ppbo_model* model, const double* d_pool, int64_t M,
                           const double* h_shifts, int T, const double* d_extra, int E_rows, const double* h_xprev,
                           int K, double sep, int iters, double tol, int screen_fp32, double* d_x, double* d_mu,
                           void* stream);

/* ---- searches inside boxes: conditional optima, trust regions, profiles of the mean ------------------------------------
 * A box is lo[D] followed by hi[D], 0 <= lo_d <= hi_d <= 1, all finite, in the caller's coordinates (model->coords);
 * lo_d == hi_d fixes coordinate d.  Boxes are HOST arrays: a bad box is refused before anything is launched.
 *
 * ppbo_mean_ascent_boxes is ppbo_mean_ascent inside boxes: start k of d_starts[K,D] uses box k / per_box of
 * h_boxes[B,2,D], B == ceil(K / per_box).  The iteration is the unit-box one with three changes: the start and every
 * iterate are clipped to [lo, hi]; the projection zeroes g_d where x_d <= lo_d and g_d < 0 or x_d >= hi_d and g_d > 0; the
 * first step is 0.02 max_d (hi_d - lo_d) / max(|g|, 1e-300), |g| the unprojected norm.  A fixed coordinate never moves and
 * its gradient never enters the projected norm; a box with every side zero returns the point, the mean there and 0
 * iterations.  With lo = 0, hi = 1 the results are ppbo_mean_ascent's bit for bit.  All three coordinate maps.
 * d_x[K,D], d_mu[K], d_iters[K] (optional).
 *
 * ppbo_mean_search_boxes runs T searches, trial t inside box t of h_boxes[T,2,D], in one enqueue.  With
 * u = frac(pool + h_shifts[t]) (u = pool when h_shifts is NULL) the candidates of trial t are fma(hi_t - lo_t, u, lo_t)
 * for the M rows of d_pool[M,D], followed by the S rows d_seeds[t,S,D] clipped into box t: Mt = M + S slots in EVERY
 * trial.  Screening, thinning and start selection are ppbo_mean_search_multi's (the rule above; `sep` is Euclidean in the
 * caller's coordinates on the mapped candidates), then K ascents per trial inside its box.
 * screen_fp32 = 1 without a coordinate map: nothing is written out, the boxed screening kernel forms the candidates on
 * the fly with the trial in its grid; screen_fp32 = 0, and both screenings under a map: each trial's rows are written out,
 * scaled or embedded, and scored by ppbo_predict or the one-trial screen, as ppbo_mean_search_multi does.
 * Trials run in batches of at most 64 for screening, selection and ascent; the fp32 screening's row split depends on M, S
 * and N alone, so a trial's result does not depend on T, on its position or on the batch it falls into (T one-trial calls
 * return the same bits).  Unit boxes, no seeds and the same shifts return ppbo_mean_search_multi's bits (extra points and
 * x_prev absent) wherever both use the same row split: always with screen_fp32 = 0, and with the fp32 screening while
 * ceil(M / 1024) T_multi <= 128.
 * d_x[T,K,D], d_mu[T,K]: the refined maxima per trial, best start first (rows past the trial's count: mu = -inf);
 * d_count[T] (optional): starts found per trial.  iters = 0 returns the picked candidates and the mean there.
 * Limits: 1 <= T <= 4096, 1 <= K <= 1024, T K <= 65536, 0 <= S <= 64, M >= 1, 64 (M + S) < 2^31, D <= 64.
 * "invalid argument", with nothing launched and the outputs untouched: a NULL model, pool, starts, boxes or output; S > 0
 * without seeds; a box with lo > hi, a bound outside [0, 1] or not finite; the sizes above; B != ceil(K / per_box);
 * negative sep, iters or tol; a model that ppbo_mean_ascent refuses.  Nothing synchronises. */
PPBO_API int ppbo_mean_ascent_boxes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_starts, int K,
                           const double* h_boxes, int B, int per_box, int iters, double tol, double* d_x, double* d_mu,
                           int* d_iters, void* stream);
PPBO_API int ppbo_mean_search_boxes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_pool, int64_t M,
                           const double* h_shifts, const double* h_boxes, int T, const double* d_seeds, int S, int K,
                           double sep, int iters, double tol, int screen_fp32, double* d_x, double* d_mu, int* d_count,
                           void* stream);

/* ---- acquisition gradients and their ascent (no reference counterpart) --------------------------------------------------
 * The reference evaluates EI and varmax on lines (src/acquisition.py:72-81, 170-178) and has no gradient of either; the
 * ppbo_predict* and ppbo_search_* entries here return pool rows.  These two entries give the pointwise EI and the posterior variance
 * their analytic gradients and a continuous maximiser.  Everything is in the MODEL's coordinates, as for every
 * ppbo_predict* entry (model->coords is not applied; callers scale ARD points, boxes and gradients themselves).
 * With k = k(x, X), J = dk/dx (analytic, direct differences) and M the variance operator of model->form:
 *   mu = k' alpha,  grad mu = J' alpha;   var = sigma_f^2 + k' Lambda k + |M k|^2,  grad var = 2 J' u,  u = (Lambda + M'M) k
 *   score: ppbo_predict's.  MEAN: grad mu.  VARIANCE: grad var.  POINTWISE_EI with sd = sqrt(max(var, 0)) > 0 and
 *   z = (mu - mustar) / sd: Phi(z) grad mu + phi(z) grad var / (2 sd); with sd = 0: grad mu where mu > mustar, else 0.
 * var is formed as ppbo_predict forms it (the Lambda term and the sum of squares of M k), not from k'u, which cancels; mu
 * as ppbo_mean_grad forms it.  A point with a non-finite coordinate gets NaN in every output and disturbs no other row.
 *
 * ppbo_acq_grad: d_X[M,D] -> d_mu, d_var, d_score [M] and d_grad_mu, d_grad_var, d_grad_score [M,D]; each may be NULL,
 * not all.  Points go in chunks of at most 1024: per chunk the tournament's field pass (K*, Y = M K*, U = (Lambda + M'M) K*)
 * with its GEMM tile configuration pinned and a row split that depends on the model alone, then one workgroup per point
 * (a value pass and one pass over the design rows per requested gradient).  With score_kind MEAN and neither d_var nor
 * d_grad_var the operator is not read and no field pass runs.
 *
 * ppbo_acq_ascent: K <= 1024 starts d_starts[K,D] refined in lockstep inside ONE box h_box[2,D] (lo then hi, host, finite,
 * lo <= hi, any range: an ARD model's unit box is [0, s_d]; NULL = the unit box; lo_d == hi_d fixes coordinate d).  The
 * iteration is ppbo_mean_ascent_boxes' with the score in the place of the mean: clip the start; first step
 * 0.02 max_d (hi_d - lo_d) / max(|g|, 1e-300); stop when |projected g| step < tol; trial point clip(x + step pg); accept iff
 * s_new >= s (a NaN fails); Barzilai-Borwein step ss / curv when curv > 0, else twice the step; a quarter of it after a
 * rejection.  One evaluation round per iteration for all K starts together -- ppbo_acq_grad's launches on the K trial
 * points, then one judging launch (a wavefront per start) -- iters + 1 rounds, all enqueued: nothing synchronises, and a
 * start that has stopped repeats its point.  iters = 0 returns the clipped starts and the values there.
 * d_x[K,D], d_score[K], d_mu[K], d_var[K]: the refined points and ppbo_acq_grad's values there; d_iters[K] (optional): the
 * evaluated moves.  A start with a NaN coordinate keeps it, gets NaN values and 0 iterations.
 * Bits: a round's values are those ppbo_acq_grad returns for the same point; a start's result does not depend on K, on its
 * position or on the other starts; M points in one call equal any split of them over several; no atomics, every sum in
 * a fixed order, so a repeated call is bitwise equal.
 * "invalid argument", with nothing launched and the outputs untouched: a NULL model, points or (ascent) output; every
 * output of ppbo_acq_grad NULL; M outside 1 .. 2^31 - 1; K outside 1 .. 1024; iters outside 0 .. 1000; tol negative or not
 * finite; a box with lo > hi or a non-finite bound; an unknown score_kind; model->kstar_fp32 set (fp64 only); a
 * PPBO_COORDS_CAMPHOR model (a box in x is not a box in e(x)); where the operator is read (ppbo_acq_ascent always: d_var
 * is an output), a model without d_G or Lambda or with a form outside {PPBO_FORM_NODE, PPBO_FORM_EDGE}.
 * The field passes are timed as "acq_field", the launches of acq_grad_kernel as "acq_grad" (ppbo_profile_read). */
PPBO_API int ppbo_acq_grad(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, int64_t M, int score_kind,
                  double mustar, double* d_mu, double* d_var, double* d_score, double* d_grad_mu, double* d_grad_var,
                  double* d_grad_score, void* stream);
PPBO_API int ppbo_acq_ascent(ppbo_ctx* ctx, const ppbo_model* model, const double* d_starts, int K, const double* h_box,
                    int score_kind, double mustar, int iters, double tol, double* d_x, double* d_score, double* d_mu,
                    double* d_var, int* d_iters, void* stream);

/* ---- into a model's coordinates ("the coordinate map of a model" above) ------------------------------------------------ */
PPBO_API int ppbo_scale_points(ppbo_ctx* ctx, const double* d_in, int64_t M, int D, const double* h_scale, double* d_out,
                      void* stream);
PPBO_API int ppbo_camphor_embed(ppbo_ctx* ctx, const double* d_in, int64_t M, const double* h_l, double* d_out, void* stream);
PPBO_API int ppbo_camphor_line_points(ppbo_ctx* ctx, const double* d_xi, const double* d_x, const double* d_alpha,
                             int alpha_per_line, int B, int G, const double* h_l, double* d_out, void* stream);

/* ---- K10: Monte-Carlo line acquisition -------------------------------------
 * replaces EI / varmax (src/acquisition.py:72-81, 170-178) for B lines of G points
 * with stored standard-normal draws d_z[S,G]: f = mu + chol(cov) z.
 * d_grid[B,G,D] -> d_ei[B], d_varmax[B] (either may be NULL). */
PPBO_API int ppbo_line_acq(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, int B, int G,
                  double shrink, const double* d_z, int S, double mustar, double jitter,
                  double* d_ei, double* d_varmax, void* stream);
/* The same with the grid points formed ON THE DEVICE: line b is {alpha[g] * d_xi[b,:] + d_x[b,:]}, g < G -- what
 * FeedbackProcessing.xi_grid(xi, x, 'equispaced', m = 70, is_scaled = True) (src/feedback_processing.py:57-107) returns
 * for the abscissae alpha the caller has drawn (the reference: 70 noisy-equispaced values in [0, 1] per EI call,
 * src/acquisition.py:72-75).  d_alpha[G] when alpha_per_line == 0 (one abscissa vector shared by all lines: common
 * random numbers), d_alpha[B,G] otherwise.  Nothing of size B x G x D crosses the host boundary: (xi, x, alpha) are
 * B x (2 D + G) numbers (EI-EXT at D = 20: 1000 lines, 110 KB instead of an 11 MB grid built by 1000 Python calls). */
PPBO_API int ppbo_line_acq_xi(ppbo_ctx* ctx, const ppbo_model* model, const double* d_xi, const double* d_x,
                     const double* d_alpha, int alpha_per_line, int B, int G, double shrink, const double* d_z, int S,
                     double mustar, double jitter, double* d_ei, double* d_varmax, void* stream);

/* ---- the answer to a query: choice probabilities over B groups of G points ------------------------------------------
 * The likelihood is a choice model: on a query line the user marks the point they like best, and sum_Phi
 * (src/gp_model.py:176-204) scores that answer as the marked point beating every other point of the line under noisy
 * utilities.  The reference has no route to the prediction of such an answer; this extends ppbo_predict_pairs' reading
 * of the likelihood from 2 items to G.  In draw s < S the user sees
 *   u_g = f_g + noise_sd eps[s][g],   f = mu + L z[s],   L L' = cov + jitter I,
 * with (mu, cov) the posterior mean and the symmetrised G x G posterior covariance of the group (the covariance
 * ppbo_line_acq factors: prior block shrunk by `shrink`), and picks argmax_g u_g.  noise_sd = 0 (d_e may then be NULL)
 * is the noise-free argmax of the posterior path; the likelihood's own noise is noise_sd = theta[0].
 *   d_prob[B,G]   = count / S (double): the share of the S draws in which point g was picked
 *   d_count[B,G]  (int32, may be NULL): the counts themselves; integer adds, so exact and independent of any order
 *   d_choice[B,S] (int32, may be NULL): the point picked in draw s
 * Rules: of equal values the LOWER index wins (np.argmax's rule); NaN never wins; a draw in which no value is a number
 * (every u_g NaN or -inf) chooses -1 and counts nowhere, so the probabilities of its group sum to less than 1.  A group
 * in which the mean of any point is NaN (a point with a NaN coordinate: its row of the covariance is no number either)
 * chooses -1 in EVERY draw, all its counts 0; the other groups of the call are not touched.  d_choice and d_count do not
 * depend on how the draws are spread over workgroups.
 * d_z[S,G] and d_e[S,G] are shared by all groups (common random numbers), as d_z in ppbo_line_acq; ppbo_randn fills
 * them.  The points are in the MODEL's coordinates, as ppbo_line_acq takes them, a line or G arbitrary points alike.
 * G = 2: P(0 is picked) -> Phi(mu_d / sqrt(2 noise_sd^2 + var_d)) as S grows, ppbo_predict_pairs' p for the pair
 * (a, b) = (point 0, point 1) at noise_sd = theta[0], up to the shrinkage of the prior block and the jitter.
 * ppbo_line_choice_xi forms the points of line b on the device, {alpha[g] d_xi[b,:] + d_x[b,:]}, as ppbo_line_acq_xi.
 * "invalid argument", nothing launched: a NULL model, d_grid (d_xi, d_x, d_alpha), d_z or d_prob; G outside 1 .. 128;
 * B < 1 or S < 1; a negative or non-finite noise_sd or jitter; noise_sd > 0 with d_e == NULL; a model without d_G or
 * Lambda. */
PPBO_API int ppbo_line_choice(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, int B, int G, double shrink,
                     const double* d_z, const double* d_e, int S, double noise_sd, double jitter, double* d_prob,
                     int* d_count, int* d_choice, void* stream);
PPBO_API int ppbo_line_choice_xi(ppbo_ctx* ctx, const ppbo_model* model, const double* d_xi, const double* d_x,
                        const double* d_alpha, int alpha_per_line, int B, int G, double shrink, const double* d_z,
                        const double* d_e, int S, double noise_sd, double jitter, double* d_prob, int* d_count,
                        int* d_choice, void* stream);

/* ---- scoring the answers: leave-one-query-out and held-out predictive checks ------------------------------------------
 * How well does the model explain an answer?  The likelihood of an answer is sum_Phi's per-query term
 * (src/gp_model.py:176-226): for a star of G = m + 1 points, point 0 the one the user chose,
 *   l(f) = -(1/m) sum_j Phi((f_j - f_0) / (sigma sqrt 2)).
 * Both entries below have no reference counterpart: the reference has no predictive score of its answers.  A group with
 * mean mu and covariance C is scored by
 *   edge probabilities  p_j  = Phi((mu_0 - mu_j) / sqrt(2 sigma^2 + C_00 + C_jj - 2 C_0j))   (ppbo_predict_pairs' rule)
 *   agreement           a    = mean_j p_j                                                     (= 1 + E[l])
 *   log score           lpd  = log((1/S) sum_s exp l(mu + L z_s)),   L L' = (C + C')/2 + jitter I
 * with d_z[S,G] shared by all groups (common random numbers, as d_z in ppbo_line_acq; ppbo_randn fills it, draw s of
 * point g at index s G + g).  exp l lies in (1/e, 1], so the mean is a plain one.  Every sum runs in an order fixed by
 * the shapes: a call repeats bit for bit, and a group's bits do not depend on the other groups of the call.  A group
 * whose mean holds a NaN gets NaN in all its outputs.
 *
 * ppbo_loo_answers: the cavity form of leave-one-out for the Laplace posterior N(f, P), P = (Sigma^-1 - Lambda)^-1 as
 * ppbo_posterior returns it (d_P, leading dimension ldp) -- for star q, rows I = q b .. q b + m, b = m + 1, the query's
 * own likelihood site is taken out of the Gaussian,
 *   K_q = P_II^-1 + Lambda_q,   C_q = K_q^-1,   m_q = f_I - C_q g_q,
 * with Lambda_q = sum_j w_j (e_0 - e_j)(e_0 - e_j)', w_j = Delta_j phi2(Delta_j) / (2 m sigma^2), and g_q the star's part
 * of beta (g_0 = sum_j phi2(Delta_j) / (sigma m), g_j = -phi2(Delta_j) / (sigma m)), Delta_j = (f_j - f_0) / sigma, and the
 * answer is scored under N(m_q, C_q).  No refit.
 *   d_lpd[n_q], d_agree[n_q]     the two scores of every query
 *   d_edge[N]                    row q b: a_q, rows q b + j: p_j
 *   d_cav_mean[N], d_cav_var[N]  m_q and diag C_q;   d_cav_cov[n_q,b,b]: C_q
 *   d_info[n_q] (int32)          0: fine; 1: P_II is not positive definite; 2: the cavity K_q is not.  For 1 and 2 every
 *                                output of that star is NaN, and no other star is disturbed.
 * Every output may be NULL, but not all of them.  S = 0 with d_z = d_lpd = NULL runs the closed-form part only.
 *
 * ppbo_score_answers: the held-out score of B new answers d_grid[B,G,D] (point 0 of each group the chosen one) under the
 * full posterior: the group's mean and covariance by the stages ppbo_line_choice shares with ppbo_line_acq (the same
 * `shrink` and `jitter`, points in the MODEL's coordinates), sigma = model->theta[0], m = G - 1.  d_lpd[B], d_agree[B],
 * d_edge[B,G] (column 0: a, column j: p_j); each may be NULL, not all.
 *
 * "invalid argument", nothing launched, outputs untouched: NULL inputs; m < 1, m + 1 > 128, G outside 2 .. 128; N not a
 * multiple of m + 1; ldp < N; S < 0, S > 0 without d_z, d_lpd with S = 0; sigma or jitter not finite, sigma <= 0,
 * jitter < 0; every output NULL; for ppbo_score_answers B < 1 or a model without d_G or Lambda. */
PPBO_API int ppbo_loo_answers(ppbo_ctx* ctx, const double* d_P, int ldp, const double* d_f, int N, int m, double sigma,
                     const double* d_z, int S, double jitter, double* d_lpd, double* d_agree, double* d_edge,
                     double* d_cav_mean, double* d_cav_var, double* d_cav_cov, int* d_info, void* stream);
PPBO_API int ppbo_score_answers(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, int B, int G, double shrink,
                       const double* d_z, int S, double jitter, double* d_lpd, double* d_agree, double* d_edge,
                       void* stream);


/* standard normal draws for the Monte-Carlo acquisitions, generated on the device: d_out[n] = a pure function of
 * (seed, index) (Philox-4x32-10 + Box-Muller), i.e. reproducible and independent of the launch geometry.  Replaces
 * the np.random.multivariate_normal / standard_normal draws of src/acquisition.py:76,174 where the caller does not
 * need NumPy's own stream (the batched searches; EI() / varmax() called with explicit draws keep the caller's z). */
PPBO_API int ppbo_randn(ppbo_ctx* ctx, uint64_t seed, double* d_out, int64_t n, void* stream);

/* ---- K7/K8/K9: random Fourier features --------------------------------------
 * ppbo_rff_project replaces Hsampler.phiVec/update_phi_X
 *   (src/random_fourier_sampler.py:45-47,57-58): d_Phi[F,N] = sqrt(2 sf^2/F) cos(W X^T + b).
 * ppbo_rff_score replaces phi(x)^T omega (:166,170) batched over M candidates with
 *   an on-device argmax (Phi(Xc) never materialised).
 * ppbo_rff_terms replaces S, S_grad, diag(S_hessian) (:106-122); outputs may be NULL. */
PPBO_API int ppbo_rff_project(ppbo_ctx* ctx, const double* d_X, int N, int D, const double* d_W, int F,
                     const double* d_b, double sigma_f, double* d_Phi, void* stream);
PPBO_API int ppbo_rff_score(ppbo_ctx* ctx, const double* d_Xc, int64_t M, int D, const double* d_W, int F,
                   const double* d_b, double sigma_f, const double* d_omega, double* d_score,
                   double* h_best_val, int64_t* h_best_idx, void* stream);
PPBO_API int ppbo_rff_terms(ppbo_ctx* ctx, const double* d_Phi, int F, int N, int m, double sigma,
                   const double* d_omega, double* h_S, double* d_grad, double* d_hdiag, void* stream);

/* Hsampler.update_omega_MAP (src/random_fourier_sampler.py:124-132): maximise S from the start vector in d_omega[F]
 * (in: start, out: omega_MAP).  The reference hands -S to SciPy's trust-exact; S_hessian is diagonal, so the trust
 * region subproblem has the closed form s_i = g_i / (max(-h_i, 1e-12) + lam) with lam = 0 when the Newton step fits
 * and the More-Sorensen root of |s(lam)| = radius otherwise, under SciPy's radius rules (x1/4 below rho = 1/4, x2
 * above 3/4 on the boundary, accept above 0.15).  The whole loop is device-resident: omega, gradient, Hessian diagonal
 * AND the trust region's state stay on the device, one workgroup judges each trial and forms the next (four launches per
 * iteration), the host only keeps a few iterations enqueued ahead of a host-mapped progress word and reads S, |grad S|
 * and the iteration count once, at the end.  d_omega is written on `stream` (ordered for later work on that stream).
 * Stops on |grad S| < gtol (h_gradnorm belongs to the point returned), maxiter, or a collapsed radius. */
PPBO_API int ppbo_rff_omega_map(ppbo_ctx* ctx, const double* d_Phi, int F, int N, int m, double sigma, double* d_omega,
                       int maxiter, double gtol, double* h_S, double* h_gradnorm, int* h_iterations, void* stream);

/* the maximiser of ONE posterior sample phi(x)^T omega, device-resident: replaces Hsampler.return_xstar's 5-30
 * L-BFGS-B starts on NumPy phi / Dphi (src/random_fourier_sampler.py:143-176).  Scores the M candidates
 * (ppbo_rff_score), keeps the K best that are > sep apart and runs the whole projected Barzilai-Borwein ascent of
 * each inside one kernel with the analytic gradient -a sum_f omega_f sin(w_f.x + b_f) w_f (:51-53).
 * d_x[K,D] / d_val[K]: refined maxima (rows >= *h_found: value -inf).
 * coords = NULL (or kind 0): d_W[F,D] acts on the points themselves.  PPBO_COORDS_CAMPHOR, a camphor-copper basis
 * (camphor_copper_kernel, camphor_copper_ard_kernel; D must be 6): the features live on the embedded point e(x) in R^11,
 * phi(x) = sqrt(2 sf^2 / F) cos(W e(x) + b) with d_W[F,11], and the search runs in the caller's six coordinates.
 * d_cand[M,6] are embedded (ppbo_camphor_embed) and scored (ppbo_rff_score); the starts are chosen on d_cand, so sep is in
 * the caller's units; each ascent forms e(x) and pulls the gradient back through de/dx (2 pi (c_d g_s - s_d g_c) for a
 * periodic d, g_z / l_2 for z).  h_coef = l[6] (the scalar kernel: l, l, l + 0.05, l, l, l); d_Xc is not read.
 * PPBO_COORDS_SCALED is "invalid argument": a scaled basis is a basis (W s). */
PPBO_API int ppbo_rff_search(ppbo_ctx* ctx, const double* d_cand, int64_t M, int D, const double* d_W, int F,
                    const double* d_b, double sigma_f, const double* d_omega, const ppbo_coords* coords, int K,
                    double sep, int iters, double tol, double* d_x, double* d_val, int* h_found, void* stream);

/* ---- batches of posterior samples: S weight vectors omega_s per enqueue ----------------------------------------
 * The upstream workflow draws the posterior of the maximiser with one Hsampler.sample_xstar() per sample
 * (src/random_fourier_sampler.py:143-176 per sample, :207-220 for the weight draw).  These entries serve S samples at
 * once: one scoring launch forms the cosine features of a candidate tile once and contracts them with all S weight
 * vectors on the fp64 matrix cores, one selection launch serves every sample and one ascent launch runs S x K starts.
 * At most PPBO_RFF_MULTI_MAX_S samples per call (larger batches go in chunks). */
#define PPBO_RFF_MULTI_MAX_S 1024

/* Omega[s][f] = omega_MAP[f] + sqrt(cov_diag[f]) z[s][f] for s < S: S draws of the weights from their Laplace
 * posterior N(omega_MAP, diag(cov_diag)) (src/random_fourier_sampler.py:207-220, the dense covariance is diagonal),
 * z the ppbo_randn stream of `seed` at index s F + f -- bitwise reproducible for a given seed.  d_omegas[S,F]. */
PPBO_API int ppbo_rff_omega_draws(ppbo_ctx* ctx, uint64_t seed, const double* d_omega_map, const double* d_cov_diag, int F,
                         int S, double* d_omegas, void* stream);

/* ppbo_rff_score for S weight vectors: d_score[s][c] = phi(x_c)^T omega_s, d_omegas[S,F] row-major, d_score[S,M]
 * (:166,170 per sample).  Every feature summed in one fixed order: a repeated call is bitwise equal.
 * "invalid argument": null pointers, M outside 1 .. 2^31 - 1, D outside 1 .. 64, S outside 1 .. PPBO_RFF_MULTI_MAX_S. */
PPBO_API int ppbo_rff_score_multi(ppbo_ctx* ctx, const double* d_Xc, int64_t M, int D, const double* d_W, int F,
                         const double* d_b, double sigma_f, const double* d_omegas, int S, double* d_score,
                         void* stream);

/* ppbo_rff_search for S weight vectors over one shared candidate set (:143-176 per sample): scores every candidate for
 * every sample (ppbo_rff_score_multi), picks each sample's K best starts > sep apart in its own scores, and ascends all
 * S x K starts in one launch, workgroup s K + k on omega_s.  d_x[S,K,D] / d_val[S,K]: refined maxima of sample s in
 * rows < d_found[s] (an int array on the device), value -inf in the others.  Enqueued only: nothing is read back.
 * coords as ppbo_rff_search: with PPBO_COORDS_CAMPHOR d_W[F,11], d_cand[M,6] embedded once and scored at D = 11;
 * selection, box, sep and d_x[S,K,6] in the caller's coordinates.
 * "invalid argument" as ppbo_rff_score_multi, and K outside 1 .. 1024. */
PPBO_API int ppbo_rff_search_multi(ppbo_ctx* ctx, const double* d_cand, int64_t M, int D, const double* d_W, int F,
                          const double* d_b, double sigma_f, const double* d_omegas, const ppbo_coords* coords, int S,
                          int K, double sep, int iters, double tol, double* d_x, double* d_val, int* d_found,
                          void* stream);

/* ---- pathwise posterior samples (decoupled sampling, Wilson et al. 2020, on the Laplace posterior) -----------------
 * g_s(x) = phi(x)^T w_s + k(x, X) v_s with prior weights w_s ~ N(0, I_F) and v_s = Sigma^-1 (f_s - Phi(X)^T w_s),
 * f_s ~ N(f_MAP, P): a draw from the GP posterior itself (no reference counterpart: src/random_fourier_sampler.py samples
 * the weight-space posterior with a diagonal covariance).  The host assembles d_Wp[S,F] and d_V[S,N] from resident
 * pieces (ppbo_randn, ppbo_potrf, ppbo_dgemm); these entries evaluate and maximise the S paths.  Radial kernels only
 * (SE, RQ, Matern-5/2, Matern-3/2): PPBO_KERNEL_CAMPHOR is "invalid argument".
 *
 * ppbo_path_score_multi: d_score[s][c] = phi(x_c)^T w_s + sum_i V[s][i] k(x_c, x_i), d_score[S,M] row-major.  One launch:
 * per candidate tile the cosine tile and the tile of k(x_c, x_i) are formed in turn and contracted with [W_prior | V]
 * on the fp64 matrix cores, inner dimension F + N in one fixed order (a repeated call is bitwise equal).  d_Xc[M,D],
 * d_W[F,D] and d_X[N,D] in the SAME coordinates, theta = (sigma, l, sigma_f) the kernel's there; per-dimension length
 * scales: the rows scaled by s = 1 / l as the model holds them, W unscaled (w_f / s), theta[1] = 1.
 * "invalid argument" as ppbo_rff_score_multi, and N < 1. */
PPBO_API int ppbo_path_score_multi(ppbo_ctx* ctx, int kernel_id, const double theta[3], const double* d_Xc, int64_t M, int D,
                          const double* d_W, int F, const double* d_b, const double* d_Wp, const double* d_X, int N,
                          const double* d_V, int S, double* d_score, void* stream);

/* ppbo_rff_search_multi for S paths: scores every candidate for every path (ppbo_path_score_multi), picks each path's K
 * best starts > sep apart in its own scores, and ascends all S x K starts in one launch with the value and gradient of
 * g_s (both halves) evaluated per iterate.  d_cand[M,D], the [0,1]^D box, sep and d_x[S,K,D] in the caller's coordinates
 * with d_W[F,D] the basis there; coords = NULL (or kind 0): d_X[N,D] the design, theta its kernel's; PPBO_COORDS_SCALED
 * (h_coef[D] = 1 / l, ARD): d_X the scaled rows and theta[1] = 1.  d_x / d_val / d_found as ppbo_rff_search_multi.
 * Enqueued only.  "invalid argument" as ppbo_path_score_multi, K outside 1 .. 1024, a scale that is not positive and
 * finite, PPBO_COORDS_CAMPHOR (as the camphor kernel id). */
PPBO_API int ppbo_path_search_multi(ppbo_ctx* ctx, int kernel_id, const double theta[3], const double* d_cand, int64_t M,
                          int D, const double* d_W, int F, const double* d_b, const double* d_Wp, const double* d_X, int N,
                          const double* d_V, const ppbo_coords* coords, int S, int K, double sep, int iters, double tol,
                          double* d_x, double* d_val, int* d_found, void* stream);

/* ---- generic fp64 MFMA GEMM (exposed for tests and host-side composition) ----
 * C[M,N] = alpha op(A) op(B) + beta C.  transA/transB: 0 = as stored, 1 = transposed.  Row-major storage with leading
 * dimensions lda >= (transA ? M : K), ldb >= (transB ? K : N), ldc >= N; a shorter one is "invalid argument".  K = 0
 * gives C = beta C; C is not read when beta == 0. */
PPBO_API int ppbo_dgemm(ppbo_ctx* ctx, int transA, int transB, int M, int N, int K, double alpha,
               const double* d_A, int lda, const double* d_B, int ldb, double beta,
               double* d_C, int ldc, void* stream);

/* ---- a-9: the determinant term of the Laplace evidence ---------------------------------
 * ppbo_lu_slogdet replaces  P,L,U = scipy.linalg.lu(M); slogdet(P), slogdet(L), slogdet(U)
 * (src/gp_model.py:303-310): LU with partial pivoting (LAPACK pivot rule) IN PLACE on d_A;
 * returns *h_u_sign = prod sign(u_ii) and *h_u_logdet = sum log|u_ii|.  P and L contribute
 * sign*0, so the reference's sum of sign*logdet is exactly (*h_u_sign) * (*h_u_logdet).
 * *h_info = k>0 if u_kk == 0.
 * ppbo_laplace_logdet forms M = I + Sigma*Lambda (src/gp_model.py:301-302, plus sign as in the
 * reference) from the star-form Lambda and calls ppbo_lu_slogdet on it. */
PPBO_API int ppbo_lu_slogdet(ppbo_ctx* ctx, double* d_A, int N, int lda, double* h_u_sign, double* h_u_logdet,
                    int* h_info, void* stream);
PPBO_API int ppbo_laplace_logdet(ppbo_ctx* ctx, const double* d_Sigma, const double* d_lam_diag,
                        const double* d_lam_off, int N, int m, double* h_u_sign, double* h_u_logdet,
                        int* h_info, void* stream);

/* ---- gradient of the Laplace evidence (no reference counterpart: the reference's theta search is derivative-free,
 * src/gp_model.py:391-413) ----------------------------------------------------------------------------------------------
 * ppbo_evidence_grad takes what one evidence leaves behind -- the rows d_X[N,D] and theta[3] as the device sees them (an
 * ARD model passes its scaled rows and theta[1] = 1), the shrink, m, d_Sigma, d_Sigma_inv, d_fMAP and the star-form
 * d_lam_diag / d_lam_off of Lambda(f_MAP) -- and returns
 *   *h_u_sign, *h_u_logdet   bit-identical to ppbo_laplace_logdet on the same inputs (the same LU launches);
 *   h_sums[D + 1]            h_sums[d] = sum_ij W_ij kappa'(rho_ij^2) (x_id - x_jd)^2 for d < D and
 *                            h_sums[D] = sum_ij W_ij Sigma_ij, with rho^2 = |x_i - x_j|^2 / theta[1]^2 and
 *                            W = 1/2 alpha alpha^T - 1/2 s_U Lambda A^-1 - 1/2 s_U (Sigma^-1 Q^-1 v) alpha^T
 *                            (A = I + Sigma Lambda, Q = Sigma^-1 - Lambda, alpha = Sigma^-1 f_MAP, v the implicit f_MAP
 *                            term).  The host forms dE/dl_d = -2 (1 - shrink) sigma_f^2 h_sums[d] /
 *                            (theta[1]^2 l_d) and dE/dsigma_f = 2 h_sums[D] / sigma_f, plus the log-prior's terms.
 * Deterministic: fixed-order reductions, no floating-point atomics.  Radial kernels only (camphor-copper: "invalid
 * argument"); N <= 20480.  *h_info = 0; -k when u_kk == 0 (log|det A| = -inf); PPBO_ERR_NOT_PD with *h_info = 2 when Q
 * is not positive definite (f_MAP is not a maximum, the implicit term is undefined). */
PPBO_API int ppbo_evidence_grad(ppbo_ctx* ctx, int kernel_id, const double* d_X, int N, int D, const double theta[3],
                       double shrink, int m, const double* d_Sigma, const double* d_Sigma_inv, const double* d_fMAP,
                       const double* d_lam_diag, const double* d_lam_off, double* h_u_sign, double* h_u_logdet,
                       double* h_sums, int* h_info, void* stream);

/* ---- (e) the path's one collective, over RCCL / xGMI ---------------------------------------------------
 * Candidate rows are sharded over one process per GPU; every rank scores its shard with
 * ppbo_predict and contributes (best score, GLOBAL row index).  ppbo_argmax_allgather is ONE ncclAllGather of a
 * 16-byte record per rank followed by a local reduction: largest value, ties to the smallest index
 * (np.argmax first-occurrence semantics), NaN or index < 0 never win.  librccl is dlopen'ed on first use.
 *   rank 0:  ppbo_dist_unique_id(ctx, id)  -> ship the 128 bytes to the other ranks by any means (file, MPI, env)
 *   all:     ppbo_dist_init(ctx, id, rank, world)   (collective; the ctx's device is the rank's GPU)
 *   search:  ppbo_argmax_allgather(ctx, local_val, local_idx + shard_offset, &val, &idx, stream)
 * Return codes 2000 + ncclResult_t for RCCL failures. */
PPBO_API int ppbo_dist_unique_id(ppbo_ctx* ctx, void* h_id128);
PPBO_API int ppbo_dist_init(ppbo_ctx* ctx, const void* h_id128, int rank, int world);
PPBO_API int ppbo_dist_destroy(ppbo_ctx* ctx);
PPBO_API int ppbo_argmax_allgather(ppbo_ctx* ctx, double local_val, int64_t local_global_idx, double* h_best_val,
                          int64_t* h_best_idx, void* stream);
/* the same exchange fed from DEVICE memory (d_record[2] as written by ppbo_predict_record): no host value is
 * uploaded first; all-gather, reduction and the 16-byte read-back run behind each other on `stream`. */
PPBO_API int ppbo_argmax_allgather_record(ppbo_ctx* ctx, const double* d_record, double* h_best_val, int64_t* h_best_idx,
                                 void* stream);
/* one whole sharded search step in ONE call: ppbo_predict_record on this rank's M rows (global row index =
 * index_offset + local row), ncclAllGather of the records, reduction, one 16-byte read-back, ONE host wait.
 * Every rank returns the job-wide (best score, global index).  Without ppbo_dist_init (a single-process search)
 * the collective is skipped.  Replaces the sequential search of mu_star (src/gp_model.py:415-437) over a sharded
 * candidate set; the reference itself is process-per-run (ppbo_numerical_main.py:192-193). */
PPBO_API int ppbo_search_sharded(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                        double mustar, int64_t index_offset, double* h_best_val, int64_t* h_best_idx, void* stream);

/* ---- the variance operator in EDGE form ----------------------------------------------------------------------------
 * Lambda_MAP = sum over the E = N - n_q star edges (obs_q, j) of w_j (e_obs - e_j)(e_obs - e_j)^T, so with D the E x N
 * edge incidence matrix and e = diag(w) D k* (e_j = w_j (k*_obs - k*_j)) the variance term is |G k*|^2 = e^T (D P D^T) e,
 * P = B^-1.  Ordering the coordinates as [n_q observation values; the E edge differences x_obs - x_j, star-major] turns
 * B into the congruent Btilde (positive definite exactly when B is); with Btilde = L L^T, D P D^T = L22^-T L22^-1 for
 * the trailing E x E block L22, hence
 *   sigma^2(x) = sigma_f^2 + k*^T Lambda k* + |H e|^2,   H = L22^-1 (lower triangular, E x E).
 * No square root of the sign-changing edge weights is taken.  H is stored in the N x N d_G of the node form: rows and
 * columns [0, n_q) zero, edge (q, t) (pseudo row q (m + 1) + 1 + t) at row / column n_q + q m + t, zeros above the
 * diagonal.  Its contraction costs (E / N)^2 of the node form's and ends at each row's own diagonal instead of at the end
 * of its star.
 * ppbo_posterior_form: PPBO_FORM_NODE when the one-launch scoring kernel (fused.hip, node form only) takes a model of
 * this shape by default (radial kernel, D <= 16, up to ~500 rows), else PPBO_FORM_EDGE -- which form the caller should
 * build.  It does not depend on the ctx's PPBO_FUSED setting: the shapes that only PPBO_FUSED=2 sends to the one-launch
 * kernel (up to ~1000 rows, or D > 16) get the edge form, and are then scored by the three-launch path.
 * The `form` argument of ppbo_posterior / ppbo_gp_fit selects what they write to d_G (same PPBO_ERR_NOT_PD / h_info
 * reporting either way; with PPBO_FORM_EDGE d_P, when asked for, is formed as for the node form, from a second
 * factorization in node coordinates whose failure is reported the same way), and ppbo_model.form tells every consumer
 * of the operator (ppbo_predict, ppbo_predict_record, ppbo_predict_cov, ppbo_line_acq, ppbo_line_acq_xi,
 * ppbo_search_sharded) which of the two it holds. */
PPBO_API int ppbo_posterior_form(ppbo_ctx* ctx, int kernel_id, int N, int D, int m);
/* the reduction alone, for callers that run the all-gather themselves (torch.distributed in ppbo_amd/dist.py):
 * d_records[world][2] = (value, global index as a double) per rank, already gathered in device memory; one
 * single-wavefront kernel applies the rule above and ONE 16-byte record is copied back. */
PPBO_API int ppbo_argmax_combine(ppbo_ctx* ctx, const double* d_records, int world, double* h_best_val, int64_t* h_best_idx,
                        void* stream);

/* ---- the projected edge form: the variance contraction in a bounded low-rank basis (no reference counterpart) -------------
 * |H e|^2 costs E^2 flops per candidate.  For every candidate x the extended Gram matrix [K k*; k*^T k(x,x)] is positive
 * semidefinite, so k* k*^T <= k(x,x) K <= kappa Sigma with kappa = sigma_f^2 / (1 - s) (s = PPBO_VAR_PROJECTION_SHRINK, the
 * covariance shrinkage; k(x,x) = sigma_f^2 for every kernel of this library).  With e = B k* (B the E x N edge map, rows
 * lam_off_j (e_j - e_obs)), Sigma = L L^T and W = H B L, any Q with orthonormal columns (E x r) gives, for all candidates,
 *   0 <= |H e|^2 - |Q^T H e|^2 = |(I - Q Q^T) H B k*|^2 <= kappa |(I - Q Q^T) W|_F^2.
 * T = Q^T H is a dense r x E operator: 2 r E flops per candidate, and an error bounded once per model by a computed number.
 * ppbo_var_projection_build forms Q on the device by a randomised range finder -- Y = W (W^T Omega), Omega the ppbo_randn
 * stream of seed PPBO_VAR_PROJECTION_SEED as an [N][r_max] matrix, r_max the largest multiple of 128 with 2 r_max <= 0.8 E;
 * orthonormalised in panels of 128 columns by block Gram-Schmidt with shifted, then plain Cholesky-QR -- takes the smallest
 * multiple of 128 whose estimate |W|_F^2 - sum_{i<=r} |z_i|^2 (Z = Q^T W) meets tol, and certifies it without cancellation:
 *   bound = kappa (|W - Q_r Z_r|_F^2 + 2 |Q_r^T Q_r - I|_F |W|_F^2)      (units of variance; tol is relative to sigma_f^2).
 * If the certified bound misses tol sigma_f^2 the next multiple of 128 is tried once.  The result is bitwise reproducible:
 * every rank of a sharded search builds the same T.
 * d_T: the caller's buffer of rows_max_padded x ld doubles (ppbo_var_projection_shape; ld = N rounded up to 16); on return
 * rows [rows, rows_max_padded) and columns [0, n_q) and [N, ld) hold explicit zeros, and *proj names it.
 * proj->rows == 0 (d_T is then not to be used; not an error): the model is not an edge-form one with d_G, it is one the
 * one-launch scoring kernel takes, r_max < 128, a factorization failed, or tol was not reached.
 * A projection is built for one model and is data of that model -- ppbo_model.proj (ABI 9) -- not a function name and not a
 * trailing argument: the caller copies the struct that ppbo_var_projection_build filled into the model it built it for.
 * Who reads it: ppbo_predict, ppbo_predict_record, ppbo_search_sharded and ppbo_predict_prune_report read model->proj.
 * rows <= 0 (a zero-initialised model): exactly the launches of a model without one; otherwise the contraction launch reads
 * T (rows_padded / 128 row tiles, each over the full K range) in place of H.  The mean, the k*^T Lambda k* term, the score
 * rule and the argmax are the same.  A projection whose ld, row counts or form do not fit the model is refused ("invalid
 * argument", with nothing launched); a call whose model has d_G == NULL reads no operator and no projection.
 * EVERY other entry that takes a model ignores proj (it needs H itself, or no operator): the two-set predictors
 * (ppbo_predict_pairs, _slopes, _curvatures, _functionals, _marginals), ppbo_predict_tournament, ppbo_predict_kg,
 * ppbo_search_batch, ppbo_predict_cov, the ppbo_line_* entries and ppbo_score_answers, ppbo_predict_gradients, ppbo_acq_grad
 * and ppbo_acq_ascent, the ppbo_mean_* entries, and ppbo_var_projection_shape / _build themselves (so _build may write
 * straight into the proj of the model it is given).  The consequence: the mu / var that ppbo_predict_tournament,
 * ppbo_predict_kg and ppbo_search_batch return are bit for bit those of ppbo_predict on the same model WITHOUT a projection,
 * whatever model->proj holds. */
#define PPBO_VAR_PROJECTION_SEED 0x70726f6a65637431ull
#define PPBO_VAR_PROJECTION_SHRINK 1e-6
PPBO_API int ppbo_var_projection_shape(const ppbo_model* model, int* rows_max_padded, int* ld);
PPBO_API int ppbo_var_projection_build(ppbo_ctx* ctx, const ppbo_model* model, double tol, double* d_T,
                                       ppbo_var_projection* proj, void* stream);

/* The pruned search, a diagnostic of it.  A call that asks only for the best record (ppbo_search_sharded,
 * ppbo_predict_record, ppbo_predict with no per-candidate output) of an edge-form model on the three-launch
 * path, scored by pointwise EI or VARIANCE, contracts the variance only for the candidates that a certified upper bound
 * of their score cannot rule out (env PPBO_PRUNE, default 1; 0 = contract all).  The record is bit for bit that of
 * PPBO_PRUNE=0.  This entry runs the passes of ONE chunk (M <= 65536) with the pruning on, whatever PPBO_PRUNE says, and
 * reports what they decided: per candidate (device arrays of M doubles, any may be NULL) u2 >= the contraction's sum of
 * squares, and the score interval [s_lo, s_hi] (s_hi = +inf: a candidate with a non-finite sum, which always survives);
 * on the host the threshold (the largest s_lo), the number of survivors and whether the chunk was pruned (0: more than
 * the capacity survived, or no finite threshold -- the full contraction ran).  Synchronises the stream.  ABI 8; it
 * reads model->proj since ABI 9. */
PPBO_API int ppbo_predict_prune_report(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M,
                          int score_kind, double mustar, double* d_u2, double* d_s_lo, double* d_s_hi,
                          double* h_threshold, int* h_n_surv, int* h_pruned, void* stream);

/* y = op(A) x for a square fp64 matrix; lower != 0 reads only the lower triangle (A is then
 * treated as lower-triangular).  Used for alpha = Sigma^-1 f_MAP (src/gp_model.py:445) and
 * prior draws L z (src/gp_model.py:374). */
PPBO_API int ppbo_dgemv(ppbo_ctx* ctx, int trans, int lower, int N, const double* d_A, int lda,
               const double* d_x, double* d_y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPBO_HIP_H */
