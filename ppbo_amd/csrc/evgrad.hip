// Gradient of the Laplace evidence with respect to the length scales and sigma_f (no reference counterpart: the
// reference searches theta derivative-free, src/gp_model.py:391-413).  The objective is exactly what ppbo_laplace_logdet
// and the fit make of it, E = T(f) - 1/2 s_U log|det A| (+ the host's log-prior), A = I + Sigma Lambda, s_U the sign of
// prod u_kk of A's LU with LAPACK's pivoting.  With alpha = Sigma^-1 f, Q = Sigma^-1 - Lambda, Z = Lambda A^-1,
// C = A^-1 Sigma, pairs p = (obs i, pseudo j), u_p = e_j - e_i, Delta_p = (f_j - f_i) / sigma,
//   v = sum_p (h'(Delta_p) / sigma) (C_ii + C_jj - C_ij - C_ji) u_p     (the implicit d f_MAP / d theta term)
//   w = Sigma^-1 Q^-1 v,   W = 1/2 alpha alpha^T - 1/2 s_U Z - 1/2 s_U w alpha^T
//   dE/dtheta_k = sum_ij W_ij dSigma_ij/dtheta_k
// and every dSigma is a pair function the reduction recomputes from the rows.  Stages:
//   posterior       ppbo_posterior: alpha, Q^-1 (d_P), and the PD check of Q
//   LU              ppbo_ipsl_async + ppbo_getrf_async: the very launches of ppbo_laplace_logdet, pivots kept
//   A^-1            U^T and unit L split out (evg_split_kernel), both inverted by ppbo_trtri_async, L^-1's columns
//                   permuted (evg_perm_kernel, evg_scatter_kernel), A^-1 = U^-1 (L^-1 P) on the fp64 MFMA GEMM
//   star            Z (evg_z_kernel), the diagonal / star entries of C and v (evg_star_kernel)
//   w               two ppbo_gemv_async
//   pairs           evg_pair_kernel: one pass over 64 x 64 tiles, partial sums per tile, evg_reduce_kernel sums them in
//                   a fixed order (no atomics: repeated calls are bitwise identical)
#include "linalg.h"

namespace {

constexpr int EVG_T = 64;      // pair tile edge
constexpr int EVG_CH = 8;      // length-scale sums per pair-kernel launch slice (grid.z)
constexpr int EVG_SLOTS = EVG_CH + 1;   // + the sigma_f sum (slice 0)

// perm[k] = the row of A that sits at row k of the LU (the row swaps replayed in order); one lane walks them in LDS
__global__ __launch_bounds__(64) void evg_perm_kernel(const int* __restrict__ ipiv, int N, int* __restrict__ perm) {
  extern __shared__ int sp[];
  int* p = sp;
  int* piv = sp + N;
  for (int k = threadIdx.x; k < N; k += 64) { p[k] = k; piv[k] = ipiv[k]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < N; ++k) {
      const int q = piv[k];
      if (q != k) { const int x = p[k]; p[k] = p[q]; p[q] = x; }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < N; k += 64) perm[k] = p[k];
}

// From the LU held in place: Lu = unit lower factor, Ut = U^T (lower).  Only the lower triangles are written (and read
// by ppbo_trtri_async); 32 x 32 tiles on or below the diagonal, U transposed through LDS.
__global__ __launch_bounds__(256) void evg_split_kernel(const double* __restrict__ LU, int N, double* __restrict__ Lu,
                                                        double* __restrict__ Ut) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx > by) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = by * 32, c0 = bx * 32;
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    if (r < N && c < N && c <= r) Lu[(size_t)r * N + c] = (c < r) ? LU[(size_t)r * N + c] : 1.0;
    const int rr = c0 + k, cc = r0 + tx;      // U[rr][cc], rr <= cc, becomes Ut[cc][rr]
    tile[k][tx] = (rr < N && cc < N) ? LU[(size_t)rr * N + cc] : 0.0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;        // Ut[r][c] = U[c][r] = tile[tx][k]
    if (r < N && c < N && c <= r) Ut[(size_t)r * N + c] = tile[tx][k];
  }
}

// B[:, perm[k]] = Linv[:, k]  (A^-1 = U^-1 L^-1 P with P A = L U: the column swaps of getri)
__global__ __launch_bounds__(256) void evg_scatter_kernel(const double* __restrict__ Linv, int N,
                                                          const int* __restrict__ perm, double* __restrict__ B) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const size_t i = blockIdx.y;
  if (k >= N) return;
  B[i * N + perm[k]] = Linv[i * N + k];
}

// Z = Lambda A^-1 for the star-form Lambda: row q0 (observation) = ld[q0] Ainv[q0] + sum_k lo[q0+k] Ainv[q0+k],
// row j (pseudo) = ld[j] Ainv[j] + lo[j] Ainv[q0]
__global__ __launch_bounds__(256) void evg_z_kernel(const double* __restrict__ Ainv, int N, int mblk,
                                                    const double* __restrict__ ld, const double* __restrict__ lo,
                                                    double* __restrict__ Z) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (c >= N) return;
  const int q0 = (i / mblk) * mblk;
  double z = ld[i] * Ainv[(size_t)i * N + c];
  if (i == q0) {
    for (int k = 1; k < mblk; ++k) z += lo[q0 + k] * Ainv[(size_t)(q0 + k) * N + c];
  } else {
    z += lo[i] * Ainv[(size_t)q0 * N + c];
  }
  Z[(size_t)i * N + c] = z;
}

__device__ __forceinline__ double evg_dot(const double* __restrict__ a, const double* __restrict__ b, int N, int lane) {
  double acc = 0.0;
  for (int k = lane; k < N; k += 64) acc += a[k] * b[k];
  return wave_sum(acc);
}

// One workgroup per query (mblk rows): C_rr, C_{r,q0}, C_{q0,r} (C = A^-1 Sigma, Sigma symmetric: C_ij = Ainv[i] . Sigma[j])
// by one wavefront per row, then v on the query's rows: v_j = t_j, v_q0 = -sum_j t_j,
// t_j = h'(Delta_j) / sigma (C_q0q0 + C_jj - C_q0j - C_jq0),  h'(D) = phi2(D) (1 - D^2 / 2) / (2 m sigma^2)
__global__ __launch_bounds__(256) void evg_star_kernel(const double* __restrict__ Ainv, const double* __restrict__ S,
                                                       int N, int mblk, const double* __restrict__ f, double sigma,
                                                       double* __restrict__ v) {
  extern __shared__ double sc[];      // [3][mblk]: C_rr, C_{r,q0}, C_{q0,r}
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.x * mblk;
  const double* a0 = Ainv + (size_t)q0 * N;
  const double* s0 = S + (size_t)q0 * N;
  for (int r = wave; r < mblk; r += 4) {
    const double* ar = Ainv + (size_t)(q0 + r) * N;
    const double* sr = S + (size_t)(q0 + r) * N;
    const double crr = evg_dot(ar, sr, N, lane);
    const double cr0 = (r > 0) ? evg_dot(ar, s0, N, lane) : crr;
    const double c0r = (r > 0) ? evg_dot(a0, sr, N, lane) : crr;
    if (lane == 0) { sc[r] = crr; sc[mblk + r] = cr0; sc[2 * mblk + r] = c0r; }
  }
  __syncthreads();
  const int m = mblk - 1;
  const double c = 1.0 / (2.0 * m * sigma * sigma * sigma);      // h' / sigma = phi2 (1 - D^2/2) c
  const double inv_sqrt_4pi = 0.28209479177387814347;
  for (int r = 1 + threadIdx.x; r < mblk; r += 256) {
    const double D = (f[q0 + r] - f[q0]) / sigma;
    const double phi2 = inv_sqrt_4pi * exp(-0.25 * D * D);
    const double t = phi2 * (1.0 - 0.5 * D * D) * c * (sc[0] + sc[r] - sc[2 * mblk + r] - sc[mblk + r]);
    sc[mblk + r] = t;         // each thread reads and rewrites only its own r (sc[0] is never rewritten)
  }
  __syncthreads();
  for (int r = 1 + threadIdx.x; r < mblk; r += 256) v[q0 + r] = sc[mblk + r];
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int r = 1; r < mblk; ++r) acc += sc[mblk + r];
    v[q0] = -acc;
  }
}

// kappa'(rho^2) with rho^2 = s / l^2 (s = |x_i - x_j|^2 of the rows as passed), from the kernel's own parameters
template <int KID>
__device__ __forceinline__ double evg_kappa_prime(double s, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    return -0.5 * exp_nonpos(-p.c0 * s);                        // -1/2 e^{-rho^2/2}
  } else if constexpr (KID == PPBO_KERNEL_RQ) {
    const double t = 1.0 + s * p.c0;                            // (1 + rho^2 / 4)
    return -0.5 / (t * t * t);
  } else if constexpr (KID == PPBO_KERNEL_MATERN52) {
    const MaternAE ae = matern_ae<KID>(s, p);
    return -(5.0 / 6.0) * ((1.0 + ae.a) * ae.e);
  } else {
    static_assert(KID == PPBO_KERNEL_MATERN32, "radial kernels only");
    const MaternAE ae = matern_ae<KID>(s, p);
    return -1.5 * ae.e;
  }
}

// One 64 x 64 tile of pairs; thread = (column j, rows i = i0 + wave + 4 k).  Slice z accumulates
// g_d = sum W_ij kappa'_ij (x_id - x_jd)^2 for d in [8 z, 8 z + 8); slice 0 also sum W_ij Sigma_ij.  One row of
// EVG_SLOTS partial sums per (slice, tile).
template <int KID>
__global__ __launch_bounds__(256) void evg_pair_kernel(const double* __restrict__ X, int N, int D, KernParams p,
                                                       const double* __restrict__ alpha, const double* __restrict__ w,
                                                       const double* __restrict__ Z, const double* __restrict__ S,
                                                       const double* __restrict__ d_sgn, double* __restrict__ part) {
  __shared__ double red[EVG_SLOTS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * EVG_T + lane;
  const int i0 = blockIdx.y * EVG_T;
  const int d0 = blockIdx.z * EVG_CH;
  const double hs = -0.5 * d_sgn[0];
  double acc[EVG_SLOTS];
#pragma unroll
  for (int q = 0; q < EVG_SLOTS; ++q) acc[q] = 0.0;
  if (j < N) {
    const double aj = alpha[j];
    const double* xj = X + (size_t)j * D;
    for (int k = 0; k < EVG_T / 4; ++k) {
      const int i = i0 + wave + 4 * k;
      if (i >= N) break;
      const double* xi = X + (size_t)i * D;
      double s = 0.0;
      for (int d = 0; d < D; ++d) {
        const double dx = xi[d] - xj[d];
        s += dx * dx;
      }
      const double Wij = aj * (0.5 * alpha[i] + hs * w[i]) + hs * Z[(size_t)i * N + j];
      const double g = Wij * evg_kappa_prime<KID>(s, p);
#pragma unroll
      for (int q = 0; q < EVG_CH; ++q) {
        const int d = d0 + q;
        if (d < D) {
          const double dx = xi[d] - xj[d];
          acc[q] += g * (dx * dx);
        }
      }
      if (blockIdx.z == 0) acc[EVG_CH] += Wij * S[(size_t)i * N + j];
    }
  }
#pragma unroll
  for (int q = 0; q < EVG_SLOTS; ++q) {
    const double t = wave_sum(acc[q]);
    if (lane == 0) red[q][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < EVG_SLOTS) {
    const int q = threadIdx.x;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const size_t row = (size_t)blockIdx.z * gridDim.x * gridDim.y + tile;
    part[row * EVG_SLOTS + q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
  }
}

// out[d] (d < D) = the length-scale sum of dimension d, out[D] = the sigma_f sum: the tiles' partials in a fixed order
__global__ __launch_bounds__(256) void evg_reduce_kernel(const double* __restrict__ part, int ntiles, int D,
                                                         double* __restrict__ out) {
  __shared__ double red[4];
  const int o = blockIdx.x;
  const int z = (o < D) ? o / EVG_CH : 0, q = (o < D) ? o % EVG_CH : EVG_CH;
  const double* base = part + (size_t)z * ntiles * EVG_SLOTS + q;
  double acc = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += 256) acc += base[(size_t)t * EVG_SLOTS];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[o] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

extern "C" {

int ppbo_evidence_grad(ppbo_ctx* ctx, int kernel_id, const double* d_X, int N, int D, const double theta[3],
                       double shrink, int m, const double* d_Sigma, const double* d_Sigma_inv, const double* d_fMAP,
                       const double* d_lam_diag, const double* d_lam_off, double* h_u_sign, double* h_u_logdet,
                       double* h_sums, int* h_info, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_X && theta && d_Sigma && d_Sigma_inv && d_fMAP && d_lam_diag && d_lam_off && h_sums, "null pointer");
  PPBO_REQUIRE(ctx, N > 0 && D > 0 && m >= 1 && N % (m + 1) == 0 && theta[0] > 0 && theta[1] > 0, "sizes");
  PPBO_REQUIRE(ctx, ppbo_kernel_id_valid(kernel_id), "kernel_id");
  PPBO_REQUIRE(ctx, kernel_id != PPBO_KERNEL_CAMPHOR, "the evidence gradient is defined for the radial kernels only");
  PPBO_REQUIRE(ctx, N <= 20480, "N (the pivot replay holds 2 N ints in LDS)");
  (void)shrink;   // enters the host's gradient as the factor (1 - shrink); the device sums do not depend on it
  hipStream_t s = (hipStream_t)stream;
  if (h_info) *h_info = 0;
  const int mblk = m + 1, n_q = N / mblk;
  const size_t nn = (size_t)N * N;
  const int nt = (N + EVG_T - 1) / EVG_T, ntiles = nt * nt, nz = (D + EVG_CH - 1) / EVG_CH;
  double* big = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_EVGRAD, 5 * nn * sizeof(double));
  const size_t nvec = 6 * (size_t)N + 4 + (size_t)nz * ntiles * EVG_SLOTS + (size_t)D + 1;
  double* vec = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_EVGRAD_VEC, nvec * sizeof(double) + (2 * (size_t)N + 8) * sizeof(int));
  if (!big || !vec) return (int)hipErrorOutOfMemory;
  double *bA = big, *bB = big + nn, *bC = big + 2 * nn, *bD = big + 3 * nn, *bE = big + 4 * nn;
  double *alpha = vec, *ld2 = vec + N, *lo2 = vec + 2 * (size_t)N, *v = vec + 3 * (size_t)N, *u = vec + 4 * (size_t)N,
         *w = vec + 5 * (size_t)N, *lu_out = vec + 6 * (size_t)N, *part = lu_out + 4, *out = part + (size_t)nz * ntiles * EVG_SLOTS;
  int* ipiv = reinterpret_cast<int*>(vec + nvec);
  int* perm = ipiv + N;
  int* lu_info = perm + N;

  // alpha, Q^-1 = (Sigma^-1 - Lambda)^-1 and Q's PD check (G lands in bA and is not used)
  int pinfo = 0;
  const int prc = ppbo_posterior(ctx, d_Sigma_inv, d_fMAP, N, m, theta[0], alpha, ld2, lo2, bA, bB, PPBO_FORM_NODE, &pinfo, stream);
  if (prc == PPBO_ERR_NOT_PD) {
    if (h_info) *h_info = 2;
    return ppbo_set_error(ctx, PPBO_ERR_NOT_PD, "Sigma^-1 - Lambda_MAP is not positive definite (leading minor %d): "
                          "f_MAP is not a maximum", pinfo);
  }
  if (prc) return prc;
  // the LU of ppbo_laplace_logdet, pivots kept
  if (int rc = ppbo_ipsl_async(ctx, d_Sigma, N, m, d_lam_diag, d_lam_off, bC, s)) return rc;
  if (int rc = ppbo_getrf_async(ctx, bC, N, N, ipiv, lu_info, lu_out, s)) return rc;
  // A^-1 = U^-1 (L^-1 P)
  evg_split_kernel<<<dim3((N + 31) / 32, (N + 31) / 32), 256, 0, s>>>(bC, N, bD, bA);
  PPBO_LAUNCH_CHECK(ctx);
  if (int rc = ppbo_trtri_async(ctx, bA, N, N, bE, N, s)) return rc;     // (U^T)^-1 = (U^-1)^T, zeros above
  if (int rc = ppbo_trtri_async(ctx, bD, N, N, bC, N, s)) return rc;     // L^-1, zeros above
  const int perm_lds = 2 * N * (int)sizeof(int);
  if (perm_lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)evg_perm_kernel, perm_lds);
  evg_perm_kernel<<<1, 64, perm_lds, s>>>(ipiv, N, perm);
  evg_scatter_kernel<<<dim3((N + 255) / 256, N), 256, 0, s>>>(bC, N, perm, bD);
  PPBO_LAUNCH_CHECK(ctx);
  {
    GemmArgs g{};
    g.A = bE; g.lda = N; g.B = bD; g.ldb = N; g.C = bA; g.ldc = N;
    g.M = N; g.N = N; g.K = N; g.alpha = 1.0; g.beta = 0.0;
    if (int rc = ppbo_gemm_launch(ctx, g, 1, 0, s)) return rc;
  }
  // Z = Lambda A^-1, the star entries of C = A^-1 Sigma and v
  evg_z_kernel<<<dim3((N + 255) / 256, N), 256, 0, s>>>(bA, N, mblk, d_lam_diag, d_lam_off, bC);
  const int star_lds = 3 * mblk * (int)sizeof(double);
  if (star_lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)evg_star_kernel, star_lds);
  evg_star_kernel<<<n_q, 256, star_lds, s>>>(bA, d_Sigma, N, mblk, d_fMAP, theta[0], v);
  PPBO_LAUNCH_CHECK(ctx);
  // w = Sigma^-1 Q^-1 v
  if (int rc = ppbo_gemv_async(ctx, bB, N, N, v, u, 0, 0, s)) return rc;
  if (int rc = ppbo_gemv_async(ctx, d_Sigma_inv, N, N, u, w, 0, 0, s)) return rc;
  // the pair reduction
  const KernParams kp = make_kern_params(kernel_id, theta);
  const dim3 pg(nt, nt, nz);
  if (int rc = ppbo_kernel_dispatch<true>(ctx, kernel_id, [&](auto kid) {
        evg_pair_kernel<decltype(kid)::value><<<pg, 256, 0, s>>>(d_X, N, D, kp, alpha, w, bC, d_Sigma, lu_out, part);
        return 0;
      }))
    return rc;
  evg_reduce_kernel<<<D + 1, 256, 0, s>>>(part, ntiles, D, out);
  PPBO_LAUNCH_CHECK(ctx);
  double h[2];
  int info = 0;
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h, lu_out, sizeof(h), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h_sums, out, ((size_t)D + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(&info, lu_info, sizeof(int), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if (h_u_sign) *h_u_sign = h[0];
  if (h_u_logdet) *h_u_logdet = h[1];
  if (h_info && info != 0) *h_info = -info;      // exact zero pivot of A: log|det A| = -inf, the sums are not finite
  return 0;
}

}  // extern "C"
