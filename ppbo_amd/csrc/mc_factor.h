// Step 1 of the Monte-Carlo kernels on groups of points (line_mc_kernel and line_choice_kernel of predict.hip,
// answer_score_kernel of answers.hip): the factor of a group's covariance in LDS.
#pragma once
#include "common.h"

namespace {

constexpr int MC_MAXG16 = 128;
// By the whole workgroup: the G x G posterior covariance of group blockIdx.x,
// symmetrised, jitter on its diagonal, factored in LDS.  On return Lm[G16][ld] holds L (zeros above the diagonal and in
// rows / columns >= G) and mus[G16] the group's mean (-inf beyond G); the last statement is a barrier.
__device__ __forceinline__ void mc_factor_lds(double* Lm, double* mus, const double* mu, const double* cov, int G,
                                              int G16, int ld, double jitter, const double* cov_parts, int n_parts,
                                              long long part_stride, int parts_lower_only) {
  const double* c = cov + (size_t)blockIdx.x * G * G;
  const double* m = mu + (size_t)blockIdx.x * G;
  // cov_parts: the data term K*' Lambda K* + Y'Y as line_cov_kernel leaves it -- n_parts row-split slabs per line, the
  // Lambda part in its one-sided form -- added here in slab order
  const double* cp = cov_parts ? cov_parts + (size_t)blockIdx.x * G * G : nullptr;
  for (int e = threadIdx.x; e < G16 * ld; e += blockDim.x) {
    const int g = e / ld, h = e - g * ld;
    double v = 0.0;
    if (g < G && h < G) {
      double a = c[g * G + h], b = c[h * G + g];
      // parts_lower_only: the slabs are exactly symmetric and hold the 16 x 16 tiles of the lower triangle only
      const bool up = parts_lower_only && (g >> 4) < (h >> 4);
      const int ia = up ? h * G + g : g * G + h, ib = (parts_lower_only && !up && (g >> 4) > (h >> 4)) ? g * G + h : h * G + g;
      for (int k = 0; k < n_parts; ++k) { a += cp[(size_t)k * part_stride + ia]; b += cp[(size_t)k * part_stride + ib]; }
      // symmetrise (the contributions are symmetric only up to rounding; line_cov_kernel's Lambda term only after this)
      v = 0.5 * (a + b) + ((g == h) ? jitter : 0.0);
    }
    Lm[e] = v;
  }
  for (int g = threadIdx.x; g < G16; g += blockDim.x) mus[g] = (g < G) ? m[g] : -INFINITY;
  __syncthreads();
  // right-looking Cholesky in LDS, two barriers per column: scale the column below the diagonal, then the 16 x 16
  // thread grid sweeps the trailing lower triangle (no integer division per element)
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  for (int j = 0; j < G; ++j) {
    const double d = Lm[j * ld + j];
    const double piv = (d > 0.0) ? sqrt(d) : 0.0;     // semi-definite: drop the direction
    for (int i = j + 1 + threadIdx.x; i < G; i += blockDim.x) Lm[i * ld + j] = (piv > 0.0) ? Lm[i * ld + j] / piv : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) Lm[j * ld + j] = piv;        // nobody reads the diagonal entry below
    for (int a = j + 1 + ty; a < G; a += 16) {
      const double la = Lm[a * ld + j];
      for (int b = j + 1 + tx; b <= a; b += 16) Lm[a * ld + b] -= la * Lm[b * ld + j];
    }
    __syncthreads();
  }
  // the strict upper triangle still holds the symmetric input: the contraction below stops at the diagonal TILE, so
  // inside the diagonal tiles it must read zeros there
  for (int e = threadIdx.x; e < G * G; e += blockDim.x) {
    const int g = e / G, h = e - g * G;
    if (h > g) Lm[g * ld + h] = 0.0;
  }
  __syncthreads();
}

}  // namespace
