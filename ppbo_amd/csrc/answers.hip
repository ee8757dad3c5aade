// Scoring the answers (ppbo_loo_answers, ppbo_score_answers; no reference counterpart -- the likelihood they score is
// sum_Phi of src/gp_model.py:176-226): how probable was the answer to a query under a Gaussian belief about the
// utilities of its G = m + 1 points, point 0 the chosen one?
//   loo_cavity_kernel     the belief with the query's own likelihood site taken out of the Laplace posterior (the cavity):
//                         K_q = P_II^-1 + Lambda_q, C_q = K_q^-1, m_q = f_I - C_q g_q, one workgroup per star
//   answer_edge_kernel    the closed-form edge probabilities p_j and their mean, the agreement
//   answer_score_kernel   lpd = log mean_s exp l(mu + L z_s) by line_mc_kernel's plan (factor in LDS, F = Z L' on the fp64
//                         matrix cores) with the likelihood of the draw as the epilogue
// Everything is fp64, nothing is added atomically and every sum runs in an order fixed by the shapes alone, so a call
// repeats bit for bit and a star scored alone gets the bits it gets among others.
#include "common.h"
#include "mc_factor.h"

namespace {

constexpr double INV_SQRT_4PI = 0.28209479177387814347;

// In-place lower Cholesky of the b x b matrix A (row stride ld, LDS) by the whole workgroup: mc_factor_lds' right-looking
// sweep, but a pivot that is not positive ends it.  Returns false then (the same value in every thread: the pivot is
// read by all of them behind a barrier).  Reads and writes the lower triangle and the diagonal only.
__device__ __forceinline__ bool chol_lds(double* A, int b, int ld) {
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  for (int j = 0; j < b; ++j) {
    const double d = A[j * ld + j];
    if (!(d > 0.0)) return false;                      // (a NaN lands here too)
    const double piv = sqrt(d);
    __syncthreads();                                   // every thread has read d before it is replaced
    if (threadIdx.x == 0) A[j * ld + j] = piv;
    for (int i = j + 1 + threadIdx.x; i < b; i += blockDim.x) A[i * ld + j] /= piv;
    __syncthreads();
    for (int a = j + 1 + ty; a < b; a += 16) {
      const double la = A[a * ld + j];
      for (int c = j + 1 + tx; c <= a; c += 16) A[a * ld + c] -= la * A[c * ld + j];
    }
    __syncthreads();
  }
  return true;
}

// One workgroup per star q (rows I = q b .. q b + m of P and f):
//   1. A <- P_II (LDS), w_j and g_q from f with laplace_kernel's expressions (fit.hip)
//   2. P_II = L L'                                             (not positive definite: status 1)
//   3. M = I + L' Lambda_q L = I + sum_j w_j v_j v_j',  v_j = L'(e_0 - e_j) = l_00 e_0 - (row j of L)': its strict lower
//      triangle goes into the strict UPPER triangle of A, which the factor does not use, its diagonal to dM; L goes to T
//   4. A <- M (lower), M = R R'                                (not positive definite: status 2 -- M is exactly when K_q is)
//   5. T <- L R^-T: row i of T solves R t = (row i of L)', one thread per row, in place
//   6. C_q = T T', m_q = f_I - T (T' g_q)
// T is the second b x b matrix: in LDS behind A where both fit into 64 KB (b <= 62), else in global memory (`scratch`,
// b (b + 1) doubles per star).  A failed star gets NaN in every output and disturbs no other star.
__global__ __launch_bounds__(256) void loo_cavity_kernel(const double* __restrict__ P, int ldp, const double* __restrict__ f,
                                                         int b, double sigma, double* __restrict__ scratch,
                                                         double* __restrict__ cav_mean, double* __restrict__ cav_var,
                                                         double* __restrict__ cav_cov, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int q = blockIdx.x, t = threadIdx.x, ld = b + 1, m = b - 1;
  const size_t r0 = (size_t)q * b;
  double* A = sm;                         // [b][ld]
  double* dM = A + (size_t)b * ld;        // [b]
  double* w = dM + b;                     // [b], w[0] unused
  double* gq = w + b;                     // [b]
  double* u = gq + b;                     // [b]
  double* T = scratch ? scratch + (size_t)q * b * ld : u + b;     // [b][ld]
  for (int e = t; e < b * b; e += blockDim.x) {
    const int i = e / b, j = e - i * b;
    A[i * ld + j] = P[(r0 + i) * (size_t)ldp + r0 + j];
  }
  const double f0 = f[r0];
  const double c = 1.0 / ((double)m * (sigma * sigma));
  const double bsc = sigma * (double)m;
  for (int j = 1 + t; j < b; j += blockDim.x) {
    const double delta = (f[r0 + j] - f0) / sigma;
    const double p2 = INV_SQRT_4PI * exp(-0.25 * (delta * delta));
    w[j] = 0.5 * c * delta * p2;
    gq[j] = -p2 / bsc;
    u[j] = p2;
  }
  __syncthreads();
  if (t == 0) {
    double sp2 = 0.0;
    for (int j = 1; j < b; ++j) sp2 += u[j];
    gq[0] = sp2 / bsc;
    w[0] = 0.0;
  }
  int status = 0;
  if (!chol_lds(A, b, ld)) status = 1;
  if (status == 0) {
    __syncthreads();
    const double l00 = A[0];
    for (int e = t; e < b * b; e += blockDim.x) {
      const int k = e / b, l = e - k * b;
      if (l > k) { T[k * ld + l] = 0.0; continue; }
      T[k * ld + l] = A[k * ld + l];
      // sum over the stars' edges j >= max(k, 1): v_j[k] = -L[j][k] for k >= 1, l_00 - L[j][0] for k = 0 (v_j is zero beyond j)
      double s = 0.0;
      for (int j = (k > 1 ? k : 1); j < b; ++j) {
        const double vk = (k == 0 ? l00 : 0.0) - A[j * ld + k];
        const double vl = (l == 0 ? l00 : 0.0) - A[j * ld + l];
        s += w[j] * (vk * vl);
      }
      if (l == k) dM[k] = 1.0 + s;
      else A[l * ld + k] = s;                          // the strict upper triangle: free
    }
    __syncthreads();
    for (int e = t; e < b * b; e += blockDim.x) {
      const int k = e / b, l = e - k * b;
      if (l < k) A[k * ld + l] = A[l * ld + k];
      else if (l == k) A[k * ld + k] = dM[k];
    }
    __syncthreads();
    if (!chol_lds(A, b, ld)) status = 2;
  }
  if (status != 0) {
    for (int e = t; e < b * b; e += blockDim.x)
      if (cav_cov) cav_cov[r0 * b + e] = NAN;
    for (int i = t; i < b; i += blockDim.x) {
      if (cav_mean) cav_mean[r0 + i] = NAN;
      if (cav_var) cav_var[r0 + i] = NAN;
    }
    if (t == 0 && info) info[q] = status;
    return;
  }
  __syncthreads();
  // T <- L R^-T, row by row: t_k = (L[i][k] - sum_{l < k} R[k][l] t_l) / R[k][k]   (every thread reads the same R[k][l]:
  // an LDS broadcast)
  for (int i = t; i < b; i += blockDim.x) {
    double* ti = T + (size_t)i * ld;
    for (int k = 0; k < b; ++k) {
      double s = ti[k];
      const double* rk = A + (size_t)k * ld;
      for (int l = 0; l < k; ++l) s -= rk[l] * ti[l];
      ti[k] = s / rk[k];
    }
  }
  __syncthreads();
  for (int k = t; k < b; k += blockDim.x) {
    double s = 0.0;
    for (int j = 0; j < b; ++j) s += T[j * ld + k] * gq[j];
    u[k] = s;
  }
  for (int e = t; e < b * b; e += blockDim.x) {
    const int i = e / b, j = e - i * b;
    if (j > i) continue;
    double s = 0.0;
    for (int k = 0; k < b; ++k) s += T[i * ld + k] * T[j * ld + k];
    if (cav_cov) {
      cav_cov[(r0 + i) * b + j] = s;
      cav_cov[(r0 + j) * b + i] = s;
    }
    if (i == j && cav_var) cav_var[r0 + i] = s;
  }
  __syncthreads();
  for (int i = t; i < b; i += blockDim.x) {
    double s = 0.0;
    for (int k = 0; k < b; ++k) s += T[i * ld + k] * u[k];
    if (cav_mean) cav_mean[r0 + i] = f[r0 + i] - s;
  }
  if (t == 0 && info) info[q] = 0;
}

// entry (g, h) of a group's symmetrised covariance as mc_factor_lds forms it, without the jitter: the same sums in the
// same order
__device__ __forceinline__ double group_cov_entry(const double* __restrict__ c, const double* __restrict__ cp, int n_parts,
                                                  long long part_stride, int parts_lower_only, int G, int g, int h) {
  double a = c[g * G + h], b = c[h * G + g];
  const bool up = parts_lower_only && (g >> 4) < (h >> 4);
  const int ia = up ? h * G + g : g * G + h, ib = (parts_lower_only && !up && (g >> 4) > (h >> 4)) ? g * G + h : h * G + g;
  for (int k = 0; k < n_parts; ++k) { a += cp[(size_t)k * part_stride + ia]; b += cp[(size_t)k * part_stride + ib]; }
  return 0.5 * (a + b);
}

// One workgroup per group: p_j = Phi((mu_0 - mu_j) / sqrt(2 sigma^2 + C_00 + C_jj - 2 C_0j)), pair_score_kernel's rule
// (score.h) with its den = 0 branch, and the agreement a = (1 / m) sum_j p_j added in the order of j.  edge[group][0] = a,
// edge[group][j] = p_j.  A NaN anywhere in the group's mean: NaN everywhere.
__global__ __launch_bounds__(128) void answer_edge_kernel(const double* __restrict__ mu, const double* __restrict__ cov,
                                                          int G, double sigma, const double* __restrict__ cov_parts,
                                                          int n_parts, long long part_stride, int parts_lower_only,
                                                          double* __restrict__ agree, double* __restrict__ edge) {
  __shared__ double ps[128];
  const int j = threadIdx.x;
  const double* c = cov + (size_t)blockIdx.x * G * G;
  const double* cp = cov_parts ? cov_parts + (size_t)blockIdx.x * G * G : nullptr;
  const double* mg = mu + (size_t)blockIdx.x * G;
  bool poisoned = false;
  for (int g = 0; g < G; ++g) poisoned |= mg[g] != mg[g];
  double p = 0.0;
  if (j >= 1 && j < G) {
    const double c00 = group_cov_entry(c, cp, n_parts, part_stride, parts_lower_only, G, 0, 0);
    const double cjj = group_cov_entry(c, cp, n_parts, part_stride, parts_lower_only, G, j, j);
    const double c0j = group_cov_entry(c, cp, n_parts, part_stride, parts_lower_only, G, j, 0);
    const double var = c00 + cjj - 2.0 * c0j, d = mg[0] - mg[j];
    const double den = sqrt(2.0 * (sigma * sigma) + fmax(var, 0.0));
    // den = 0 (no noise, no variance): the sign of the difference decides, a tie is 1/2
    const double zz = den > 0.0 ? d / den : (d > 0.0 ? INFINITY : (d < 0.0 ? -INFINITY : 0.0));
    p = 0.5 * erfc(-zz * 0.70710678118654752440);
    if (poisoned || var != var) p = NAN;
    if (edge) edge[(size_t)blockIdx.x * G + j] = p;
  }
  ps[j] = p;
  __syncthreads();
  if (j == 0) {
    double s = 0.0;
    for (int g = 1; g < G; ++g) s += ps[g];
    const double a = s / (double)(G - 1);
    if (agree) agree[blockIdx.x] = a;
    if (edge) edge[(size_t)blockIdx.x * G] = a;
  }
}

// draws per split: a function of S alone (at most 16 splits of at least 256 draws), so that the partial sums of a group
// -- and with them its bits -- do not depend on how many groups the call holds
inline int answer_draws_per_split(int S) {
  int d = (((S + 15) / 16) + 15) & ~15;
  return d < 256 ? 256 : d;
}

// The log score of a group by line_mc_kernel's plan: grid = (groups, draw splits); the factor of the symmetrised
// covariance + jitter I in LDS (mc_factor_lds); a wavefront takes 16 draws at a time as A fragments, one 16 x 16 tile of
// F = mu + Z L' per 16 points with the mean as the accumulator's initial value.  The epilogue of a draw:
//   f_0 sits in tile 0 at lr = 0 and is broadcast to the 16 lanes of its row; each lane evaluates
//   Phi((f_g - f_0) / (sigma sqrt 2)) = erfc(-Delta / 2) / 2 for its points g >= 1 (fit.hip's closed form; padded points
//   and g = 0 add nothing), tiles in ascending order, then the 16 lanes are added by a butterfly; l = -sum / m and
//   exp(l), in (1 / e, 1], is added to the lane's sum of its draws.
// part[(group, split)] = the sum over the split's draws (wavefront sums added in wavefront order); NaN for a group whose
// mean holds a NaN.
__global__ __launch_bounds__(256) void answer_score_kernel(const double* __restrict__ mu, const double* __restrict__ cov,
                                                           int G, const double* __restrict__ z, int S, double sigma,
                                                           double jitter, int draws_per_split, double* __restrict__ part,
                                                           const double* __restrict__ cov_parts, int n_parts,
                                                           long long part_stride, int parts_lower_only) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int G16 = (G + 15) & ~15, ld = G16 + 2;
  double* Lm = sm;                           // [G16][ld], rows / columns >= G zero
  double* mus = sm + (size_t)G16 * ld;       // [G16], -inf beyond G
  double* red = mus + G16;                   // [4]
  mc_factor_lds(Lm, mus, mu, cov, G, G16, ld, jitter, cov_parts, n_parts, part_stride, parts_lower_only);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int s_beg = blockIdx.y * draws_per_split;
  int s_end = s_beg + draws_per_split;
  if (s_end > S) s_end = S;
  const int nj = G16 >> 4;
  const double dm = (double)(G - 1);
  bool poisoned = false;                                              // every lane reads the same word: a broadcast
  for (int g = 0; g < G; ++g) poisoned |= mus[g] != mus[g];
  double sum_e = 0.0;
  for (int s0 = s_beg + 16 * wave; s0 < s_end; s0 += 64) {
    // A fragments of the 16 draws s0 .. s0+15: lane (lr, lk) holds z[s0 + lr][4 kk + lk]
    double az[MC_MAXG16 / 4];
    const int sr = s0 + lr;
    const double* zr = z + (size_t)(sr < s_end ? sr : s_beg) * G;
#pragma unroll
    for (int kk = 0; kk < MC_MAXG16 / 4; ++kk) {
      const int k = 4 * kk + lk;
      az[kk] = (kk < (G16 >> 2) && k < G) ? zr[k] : 0.0;
    }
    double f0[4] = {0.0, 0.0, 0.0, 0.0}, sphi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < MC_MAXG16 / 16; ++j) {                        // unrolled: the triangle's edge is a constant per j
      if (j >= nj) break;
      const int g = 16 * j + lr;
      const double mg = mus[g];
      double4_t acc = double4_t{mg, mg, mg, mg};
      const double* lrow = Lm + (size_t)g * ld + lk;                  // B operand: L^T[k][g] = L[g][k]
#pragma unroll
      for (int kk = 0; kk < 4 * (j + 1); ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(az[kk], lrow[4 * kk], acc, 0, 0, 0);
      // acc[r] belongs to draw s0 + lk + 4 r and point g; the chosen point's value is in the lane (lr = 0, lk)
      if (j == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) f0[r] = __shfl(acc[r], lane & 48, 64);
      }
      if (g >= 1 && g < G) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double delta = (acc[r] - f0[r]) / sigma;
          sphi[r] += 0.5 * erfc(-0.5 * delta);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = sphi[r];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if (lr == 0 && s0 + lk + 4 * r < s_end) sum_e += exp_nonpos(-v / dm);
    }
  }
  sum_e = wave_sum(sum_e);
  if (lane == 0) red[wave] = sum_e;
  __syncthreads();
  if (threadIdx.x == 0)
    part[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = poisoned ? NAN : ((red[0] + red[1]) + (red[2] + red[3]));
}

// lpd = log((1 / S) sum of the splits' sums, in split order)
__global__ __launch_bounds__(256) void answer_finish_kernel(const double* __restrict__ part, int B, int nsplit, int S,
                                                            double* __restrict__ lpd) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double e = 0.0;
  for (int k = 0; k < nsplit; ++k) e += part[(size_t)b * nsplit + k];
  lpd[b] = log(e / (double)S);
}

}  // namespace

int ppbo_answer_score_groups(ppbo_ctx* ctx, const double* mu, const double* cov, int Bc, int G, double sigma,
                             const double* d_z, int S, double jitter, const double* cov_parts, int n_parts,
                             long long part_stride, int parts_lower_only, double* d_lpd, double* d_agree, double* d_edge,
                             hipStream_t s) {
  if (d_agree || d_edge) {
    answer_edge_kernel<<<Bc, 128, 0, s>>>(mu, cov, G, sigma, cov_parts, n_parts, part_stride, parts_lower_only, d_agree,
                                          d_edge);
    PPBO_LAUNCH_CHECK(ctx);
  }
  if (!d_lpd || S <= 0) return 0;
  const int G16 = (G + 15) & ~15;
  const size_t lds = ((size_t)G16 * (G16 + 2) + G16 + 16) * sizeof(double);   // G = 128: 134 KB of the CU's 160 KB
  if (lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)answer_score_kernel, (128 * 130 + 128 + 16) * (int)sizeof(double));
  const int dps = answer_draws_per_split(S), nsplit = (S + dps - 1) / dps;
  double* part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SMALL, (size_t)Bc * nsplit * sizeof(double));
  if (!part) return (int)hipErrorOutOfMemory;
  {
    PpboProfScope pf(ctx, ppbo_ctx::PF_LINE_MC, s);
    answer_score_kernel<<<dim3(Bc, nsplit), 256, lds, s>>>(mu, cov, G, d_z, S, sigma, jitter, dps, part, cov_parts, n_parts,
                                                           part_stride, parts_lower_only);
  }
  answer_finish_kernel<<<(Bc + 255) / 256, 256, 0, s>>>(part, Bc, nsplit, S, d_lpd);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" {

int ppbo_loo_answers(ppbo_ctx* ctx, const double* d_P, int ldp, const double* d_f, int N, int m, double sigma,
                     const double* d_z, int S, double jitter, double* d_lpd, double* d_agree, double* d_edge,
                     double* d_cav_mean, double* d_cav_var, double* d_cav_cov, int* d_info, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  const double dmax = 1.79769313486231570815e308;
  PPBO_REQUIRE(ctx, d_P && d_f, "d_P / d_f");
  PPBO_REQUIRE(ctx, m >= 1 && m + 1 <= 128, "m (1 .. 127: a star of at most 128 rows)");
  PPBO_REQUIRE(ctx, N > 0 && N % (m + 1) == 0, "N must be n_q*(m+1) (feedback_processing.py:110-130)");
  PPBO_REQUIRE(ctx, ldp >= N, "ldp >= N");
  PPBO_REQUIRE(ctx, S >= 0, "S >= 0");
  PPBO_REQUIRE(ctx, S == 0 || d_z != nullptr, "S > 0 needs the draws d_z");
  PPBO_REQUIRE(ctx, S > 0 || d_lpd == nullptr, "d_lpd needs S > 0 draws");
  PPBO_REQUIRE(ctx, sigma > 0.0 && sigma <= dmax, "sigma (finite, > 0)");
  PPBO_REQUIRE(ctx, jitter >= 0.0 && jitter <= dmax, "jitter (finite, >= 0)");
  PPBO_REQUIRE(ctx, d_lpd || d_agree || d_edge || d_cav_mean || d_cav_var || d_cav_cov || d_info, "every output is NULL");
  const int b = m + 1, n_q = N / b, ld = b + 1;
  const bool want_lpd = d_lpd != nullptr, want_score = want_lpd || d_agree || d_edge;
  // the cavity's mean and covariance where the caller takes none but the scores need them: the line acquisitions' slot
  double* mean = d_cav_mean;
  double* cov = d_cav_cov;
  if (want_score && (!mean || !cov)) {
    double* ws = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, ((size_t)N * b + N) * sizeof(double));
    if (!ws) return (int)hipErrorOutOfMemory;
    if (!cov) cov = ws;
    if (!mean) mean = ws + (size_t)N * b;
  }
  // both b x b matrices of a star in LDS where they fit into 64 KB, else the second in the dense factorizations' slot
  const size_t lds_one = ((size_t)b * ld + 4 * (size_t)b) * sizeof(double), lds_two = lds_one + (size_t)b * ld * sizeof(double);
  double* scratch = nullptr;
  size_t lds = lds_two;
  if (lds_two > 64 * 1024) {
    scratch = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_LINALG, (size_t)n_q * b * ld * sizeof(double));
    if (!scratch) return (int)hipErrorOutOfMemory;
    lds = lds_one;
    if (lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)loo_cavity_kernel, (128 * 129 + 4 * 128) * (int)sizeof(double));
  }
  loo_cavity_kernel<<<n_q, 256, lds, s>>>(d_P, ldp, d_f, b, sigma, scratch, mean, d_cav_var, cov, d_info);
  PPBO_LAUNCH_CHECK(ctx);
  if (!want_score) return 0;
  return ppbo_answer_score_groups(ctx, mean, cov, n_q, b, sigma, d_z, S, jitter, nullptr, 0, 0, 0, d_lpd, d_agree, d_edge, s);
}

}  // extern "C"
