// The projected edge form (include/ppbo_hip.h, "the projected edge form"): T = Q^T H for an orthonormal Q (E x r) whose
// span carries all but a certified sliver of W = H B L, so that |H e|^2 - |T e|^2 lies in [0, bound] for EVERY candidate.
// Built once per model from the library's own pieces -- ppbo_gram, ppbo_potrf_async, ppbo_trtri_async, ppbo_gemm_launch,
// ppbo_randn, edge_apply_kernel -- on the caller's stream.  Everything is kept in the N x N layout of the edge form
// (rows / columns [0, n_q) zero), so the E x . matrices of the derivation are N x . here with n_q zero rows.
//
// Cost at N = 2048, r_max = 768 (flops, fp64): potrf N^3/3 = 2.9 G; W = H (B L) (triangular K) ~N^3 = 8.6 G; W^T Omega and
// Y = W (.) 2 x 2 N^2 r_max = 12.9 G; Z = Q^T W 6.4 G; the certificate (W - Q_r Z_r, Q_r^T Q_r) 2 N^2 r + 2 N r^2 = 5.4 G at
// r = 512; T = Q_r^T H (triangular K) ~N^2 r = 2.1 G; the panel work (6 projections, 5 Cholesky-QR per panel) ~8 G of
// skinny products that are latency- rather than rate-bound.  ~46 GF in all plus ~60 short launches per panel.
// Host waits: two -- the cumulative estimates that choose r, and the certificate of that r (a third when the next r is tried).
#include "linalg.h"

namespace {

constexpr int PJ_PANEL = 128;
// shift of a shifted Cholesky-QR pass, relative to the trace of the panel's Gram matrix: above that matrix's rounding
// (N eps ~ 5e-13 at N = 4096), so its factorization exists whatever the panel's rank
constexpr double PJ_SHIFT = 1e-11;

// out[i] = sum_j (A[i][j] - (diag_minus && i == j))^2: one workgroup per row, a fixed summation tree (bitwise reproducible)
__global__ __launch_bounds__(256) void proj_row_sumsq_kernel(const double* __restrict__ A, int cols, int ld, int diag_minus,
                                                             double* __restrict__ out) {
  __shared__ double red[256];
  const int i = blockIdx.x;
  const double* __restrict__ row = A + (size_t)i * ld;
  double s = 0.0;
  for (int j = threadIdx.x; j < cols; j += 256) {
    const double v = row[j] - ((diag_minus && j == i) ? 1.0 : 0.0);
    s = fma(v, v, s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[i] = red[0];
}

// zeros above the diagonal of a factor whose upper triangle still holds the matrix it was computed from
__global__ __launch_bounds__(256) void proj_tril_kernel(double* __restrict__ L, int N, int ld) {
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j < N && j > i) L[(size_t)i * ld + j] = 0.0;
}

// G[i][i] += shift * trace(G) for a 128 x 128 Gram matrix (one workgroup, a fixed summation tree)
__global__ __launch_bounds__(128) void proj_shift_diag_kernel(double* __restrict__ G, int ld, double shift) {
  __shared__ double red[128];
  const int i = threadIdx.x;
  const double d = G[(size_t)i * ld + i];
  red[i] = d;
  __syncthreads();
  for (int o = 64; o > 0; o >>= 1) {
    if (i < o) red[i] += red[i + o];
    __syncthreads();
  }
  G[(size_t)i * ld + i] = d + shift * red[0];
}

int gemm(ppbo_ctx* ctx, int tA, int tB, int M, int N, int K, double alpha, const double* A, int lda, const double* B, int ldb,
         double beta, double* C, int ldc, hipStream_t s, int khi_mode = 0, int klo_mode = 0) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.alpha = alpha; g.beta = beta;
  g.khi_mode = khi_mode; g.klo_mode = klo_mode; g.tri_block = 1;
  return ppbo_gemm_launch(ctx, g, tA, tB, s);
}

int r_max_of(const ppbo_model* m) {
  if (!m || m->N <= 0 || m->m < 1 || m->N % (m->m + 1) != 0) return 0;
  const int E = m->N - m->N / (m->m + 1);
  return (int)((long long)E * 4 / 10) / PJ_PANEL * PJ_PANEL;      // the largest multiple of 128 with 2 r <= 0.8 E
}

}  // namespace

extern "C" {

int ppbo_var_projection_shape(const ppbo_model* model, int* rows_max_padded, int* ld) {
  if (!model || model->N <= 0 || model->m < 1 || model->N % (model->m + 1) != 0) return -1;
  if (rows_max_padded) *rows_max_padded = r_max_of(model);
  if (ld) *ld = (model->N + 15) & ~15;
  return 0;
}

int ppbo_var_projection_build(ppbo_ctx* ctx, const ppbo_model* model, double tol, double* d_T, ppbo_var_projection* proj,
                              void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, model && proj && d_T, "null pointer");
  PPBO_REQUIRE(ctx, tol > 0.0 && std::isfinite(tol), "tol");
  PPBO_REQUIRE(ctx, model->N > 0 && model->D > 0 && model->m >= 1 && model->N % (model->m + 1) == 0 && model->d_X,
               "model sizes (N must be n_q*(m+1))");
  PPBO_REQUIRE_KERNEL(ctx, model->kernel_id, model->D);
  hipStream_t s = (hipStream_t)stream;
  const int N = model->N, mblk = model->m + 1, ld = (N + 15) & ~15;
  const int rm = r_max_of(model);
  proj->d_T = d_T; proj->rows = 0; proj->rows_padded = 0; proj->ld = ld; proj->bound = 0.0; proj->tol = tol;
  // k(x, x) = sigma_f^2 for every kernel id (kern_finish at s = 0; camphor-copper: sf2 exp(0), camphor.h's embedding is SE)
  if (model->form != PPBO_FORM_EDGE || !model->d_G || !model->d_lam_off || ppbo_fused_eligible(ctx, model) || rm < PJ_PANEL)
    return 0;
  const int npan = rm / PJ_PANEL;
  const size_t nn = (size_t)N * N, nr = (size_t)N * rm;
  const size_t doubles = 3 * nn + 4 * nr + (size_t)N * PJ_PANEL + (size_t)rm * PJ_PANEL + 2 * PJ_PANEL * PJ_PANEL + 2 * (size_t)(N + rm);
  double* ws = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PROJECT, doubles * sizeof(double));
  int* d_info = (int*)ppbo_workspace(ctx, ppbo_ctx::WS_PROJECT_SMALL, (size_t)(2 * npan + 1) * sizeof(int));
  const size_t host_bytes = 2 * (size_t)(N + rm) * sizeof(double) + (size_t)(2 * npan + 1) * sizeof(int);
  if (!ws || !d_info) return (int)hipErrorOutOfMemory;
  double* L = ws;
  double* BL = L + nn;            // B L, later the residual W - Q_r Z_r
  double* W = BL + nn;
  double* Om = W + nn;            // Omega [N][rm], later Q_r^T Q_r
  double* V = Om + nr;            // W^T Omega
  double* Q = V + nr;             // Y, orthonormalised in place [N][rm]
  double* Z = Q + nr;             // Q^T W [rm][N]
  double* Pt = Z + nr;            // a panel [N][128]
  double* Cc = Pt + (size_t)N * PJ_PANEL;   // coefficients against the finished panels [rm][128]
  double* Gm = Cc + (size_t)rm * PJ_PANEL;  // a panel's Gram matrix, then its Cholesky factor
  double* Ri = Gm + PJ_PANEL * PJ_PANEL;    // the factor's inverse
  double* sums = Ri + PJ_PANEL * PJ_PANEL;  // [N] |w_i|^2, [rm] |z_i|^2, [N] |r_i|^2, [rm] rows of Q^T Q - I

  // 1. Sigma = L L^T
  if (int rc = ppbo_gram(ctx, model->kernel_id, model->d_X, N, model->D, model->theta, PPBO_VAR_PROJECTION_SHRINK, L, stream))
    return rc;
  if (int rc = ppbo_potrf_async(ctx, L, N, N, d_info + 2 * npan, s)) return rc;
  proj_tril_kernel<<<dim3((N + 255) / 256, N), 256, 0, s>>>(L, N, N);
  PPBO_LAUNCH_CHECK(ctx);
  // 2. W = H (B L)
  if (int rc = ppbo_edge_apply_async(ctx, L, N, N, N, mblk, model->d_lam_off, BL, s)) return rc;
  if (int rc = gemm(ctx, 0, 0, N, N, N, 1.0, model->d_G, N, BL, N, 0.0, W, N, s, 1)) return rc;
  // 3. Y = W (W^T Omega)
  if (int rc = ppbo_randn(ctx, PPBO_VAR_PROJECTION_SEED, Om, (int64_t)nr, stream)) return rc;
  if (int rc = gemm(ctx, 1, 0, N, rm, N, 1.0, W, N, Om, rm, 0.0, V, rm, s)) return rc;
  if (int rc = gemm(ctx, 0, 0, N, rm, N, 1.0, W, N, V, rm, 0.0, Q, rm, s)) return rc;
  // 4. panels of 128 columns.  Y = W W^T Omega squares a spectrum that falls off a cliff, so a panel's Gram matrix is
  // numerically singular more often than not.  Each step below follows a projection off the finished panels: three
  // SHIFTED Cholesky-QR passes (each lifts the panel's smallest singular value by ~1 / sqrt(PJ_SHIFT) and cannot fail),
  // then two plain ones, of a panel that is by then well conditioned.  Directions that are rounding noise come out as
  // orthonormal junk: harmless, the bound below is certified for whatever Q is.  A failed pivot of a plain pass ends the
  // basis at the previous panel.
  for (int p = 0; p < npan; ++p) {
    const int c0 = p * PJ_PANEL;
    double* Yp = Q + c0;
    auto project_out = [&]() -> int {
      if (p == 0) return 0;
      if (int rc = gemm(ctx, 1, 0, c0, PJ_PANEL, N, 1.0, Q, rm, Yp, rm, 0.0, Cc, PJ_PANEL, s)) return rc;
      return gemm(ctx, 0, 0, N, PJ_PANEL, c0, -1.0, Q, rm, Cc, PJ_PANEL, 1.0, Yp, rm, s);
    };
    auto cholesky_qr = [&](int* info, double shift) -> int {
      if (int rc = gemm(ctx, 1, 0, PJ_PANEL, PJ_PANEL, N, 1.0, Yp, rm, Yp, rm, 0.0, Gm, PJ_PANEL, s)) return rc;
      if (shift > 0.0) {
        proj_shift_diag_kernel<<<1, PJ_PANEL, 0, s>>>(Gm, PJ_PANEL, shift);
        PPBO_LAUNCH_CHECK(ctx);
      }
      if (int rc = ppbo_potrf_async(ctx, Gm, PJ_PANEL, PJ_PANEL, info, s)) return rc;
      if (int rc = ppbo_trtri_async(ctx, Gm, PJ_PANEL, PJ_PANEL, Ri, PJ_PANEL, s)) return rc;
      if (int rc = gemm(ctx, 0, 1, N, PJ_PANEL, PJ_PANEL, 1.0, Yp, rm, Ri, PJ_PANEL, 0.0, Pt, PJ_PANEL, s)) return rc;
      PPBO_HIP_CHECK(ctx, hipMemcpy2DAsync(Yp, (size_t)rm * sizeof(double), Pt, PJ_PANEL * sizeof(double),
                                           PJ_PANEL * sizeof(double), N, hipMemcpyDeviceToDevice, s));
      return 0;
    };
    if (int rc = project_out()) return rc;
    for (int pass = 0; pass < 5; ++pass) {
      if (int rc = project_out()) return rc;
      // (the info word of a shifted pass is overwritten by the plain pass that shares it)
      if (int rc = cholesky_qr(d_info + 2 * p + (pass == 4 ? 1 : 0), pass < 3 ? PJ_SHIFT : 0.0)) return rc;
    }
  }
  // 5. Z = Q^T W; |W|_F^2 and the row square sums of Z give the estimate for every prefix in one pass
  if (int rc = gemm(ctx, 1, 0, rm, N, N, 1.0, Q, rm, W, N, 0.0, Z, N, s)) return rc;
  proj_row_sumsq_kernel<<<N, 256, 0, s>>>(W, N, N, 0, sums);
  proj_row_sumsq_kernel<<<rm, 256, 0, s>>>(Z, N, N, 0, sums + N);
  PPBO_LAUNCH_CHECK(ctx);
  // (the staging buffer is taken here, behind every library call above that may have grown it)
  char* host = (char*)ppbo_pinned(ctx, host_bytes);
  if (!host) return (int)hipErrorOutOfMemory;
  double* h_sums = (double*)host;
  int* h_info = (int*)(host + 2 * (size_t)(N + rm) * sizeof(double));
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h_sums, sums, (size_t)(N + rm) * sizeof(double), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h_info, d_info, (size_t)(2 * npan + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if (h_info[2 * npan] != 0) return 0;                         // Sigma itself did not factor: no projection
  int good = npan;                                             // a failed pivot ends the basis at the previous panel
  for (int p = 0; p < npan; ++p)
    if (h_info[2 * p] != 0 || h_info[2 * p + 1] != 0) { good = p; break; }
  double w2 = 0.0;
  for (int i = 0; i < N; ++i) w2 += h_sums[i];
  const double sf2 = model->theta[2] * model->theta[2];
  const double kappa = sf2 / (1.0 - PPBO_VAR_PROJECTION_SHRINK), tol_abs = tol * sf2;
  if (!(w2 >= 0.0) || !std::isfinite(w2)) return 0;
  int r = 0;
  {
    double cum = 0.0;
    for (int p = 0; p < good && r == 0; ++p) {
      for (int i = p * PJ_PANEL; i < (p + 1) * PJ_PANEL; ++i) cum += h_sums[N + i];
      if (std::isfinite(cum) && kappa * (w2 - cum) <= tol_abs) r = (p + 1) * PJ_PANEL;
    }
  }
  if (r == 0) return 0;
  // the certificate, for this r and once for the next: R = W - Q_r Z_r summed without cancellation, and the
  // orthogonality defect delta = |Q_r^T Q_r - I|_F;   bound = kappa (|R|_F^2 + 2 delta |W|_F^2)
  double bound = 0.0;
  bool ok = false;
  for (int attempt = 0; attempt < 2 && !ok; ++attempt, r += PJ_PANEL) {
    if (r > good * PJ_PANEL) return 0;
    PPBO_HIP_CHECK(ctx, hipMemcpyAsync(BL, W, nn * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (int rc = gemm(ctx, 0, 0, N, N, r, -1.0, Q, rm, Z, N, 1.0, BL, N, s)) return rc;
    if (int rc = gemm(ctx, 1, 0, r, r, N, 1.0, Q, rm, Q, rm, 0.0, Om, r, s)) return rc;
    proj_row_sumsq_kernel<<<N, 256, 0, s>>>(BL, N, N, 0, sums + N + rm);
    proj_row_sumsq_kernel<<<r, 256, 0, s>>>(Om, r, r, 1, sums + 2 * N + rm);
    PPBO_LAUNCH_CHECK(ctx);
    PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h_sums + N + rm, sums + N + rm, (size_t)(N + r) * sizeof(double), hipMemcpyDeviceToHost, s));
    PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
    double r2 = 0.0, d2 = 0.0;
    for (int i = 0; i < N; ++i) r2 += h_sums[N + rm + i];
    for (int i = 0; i < r; ++i) d2 += h_sums[2 * N + rm + i];
    bound = kappa * (r2 + 2.0 * std::sqrt(d2) * w2);
    ok = std::isfinite(bound) && bound <= tol_abs;
    if (ok) break;
  }
  if (!ok) return 0;
  // 6. T = Q_r^T H (H lower triangular: the K range of a column tile starts at its first column), zeros elsewhere
  int rows_max = 0;
  ppbo_var_projection_shape(model, &rows_max, nullptr);
  PPBO_HIP_CHECK(ctx, hipMemsetAsync(d_T, 0, (size_t)rows_max * ld * sizeof(double), s));
  if (int rc = gemm(ctx, 1, 0, r, N, N, 1.0, Q, rm, model->d_G, N, 0.0, d_T, ld, s, 0, 2)) return rc;
  proj->rows = r;
  proj->rows_padded = r;           // r is a whole number of 128-row tiles
  proj->bound = bound;
  return 0;
}

}  // extern "C"
