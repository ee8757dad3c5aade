// Pathwise (decoupled, Matheron) posterior samples: g_s(x) = phi(x)^T w_s + k(x, X) v_s for S samples at once.
//   w_s: prior weights of the RFF basis, v_s = Sigma^-1 (f_s - Phi(X)^T w_s) with f_s ~ N(f_MAP, P) (assembled by the host
//   from the resident pieces: random_fourier_sampler.py, Hsampler.sample_paths).
// path_score_multi_kernel is rff_score_multi_kernel (rff.hip) with the inner dimension grown from the F features to
// F + N: after the feature steps the same workgroup walks the N design rows, forms the tile k(x_c, x_i) where the cosine
// tile stood and contracts it with V where Omega stood.
#include "linalg.h"
#include "rffmath.h"

namespace {

// One half of the contraction, acc[g][j] += C[16 samples x rows] . tile[rows x 16 candidates], over the `n` rows of R
// [n][D] (KERN = false: the basis W, tile = a cos(w_f.x_c + b_f); KERN = true: the design X, tile = k(x_c, x_i)) with the
// coefficients C [S][n] (W_prior, V), 32 rows staged per step.  Row products come off the matrix cores with the
// accumulator's initial value h[row] (b_f; -|x_i|^2 / 2, so that r^2 = |x_c|^2 - 2 (x_i.x_c - |x_i|^2 / 2)): register r of
// lane (lr, lk) then holds row lk + 4 r of candidate lr, which is the B fragment of rows 4 r .. 4 r + 3 of the second
// product -- no lane movement (rff_score_multi_kernel).  Padded rows carry C = 0 and a finite tile value.
template <bool KERN, int KID, int DP, int CG, int SB>
__device__ __forceinline__ void path_half(const double* __restrict__ R, int n, int D, const double* __restrict__ h,
                                          const double* __restrict__ Cf, int S, int s0, const double (&xb)[CG][DP / 4],
                                          const double (&xn)[CG], const RffPoly& P, const KernParams& kp, double* ws,
                                          double* s_h, double* s_c, double4_t (&acc)[CG][SB]) {
  constexpr int Q = DP / 4, LD = DP + 2, RJ = 32, NS = 16 * SB, LO = RJ + 1;
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  for (int r0 = 0; r0 < n; r0 += RJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < RJ * DP; e += 256) {
      const int r = e / DP, d = e - r * DP;
      const int f = r0 + r;
      ws[r * LD + d] = (f < n && d < D) ? R[(size_t)f * D + d] : 0.0;
    }
    if (threadIdx.x < RJ) {
      const int f = r0 + threadIdx.x;
      double v = 0.0;
      if (f < n) {
        if constexpr (KERN) {
          for (int d = 0; d < D; ++d) { const double x = R[(size_t)f * D + d]; v = fma(x, x, v); }
          v *= -0.5;
        } else {
          v = h[f];
        }
      }
      s_h[threadIdx.x] = v;
    }
    for (int e = threadIdx.x; e < NS * RJ; e += 256) {
      const int j = e / RJ, r = e - j * RJ;
      const int s = s0 + j, f = r0 + r;
      s_c[j * LO + r] = (s < S && f < n) ? Cf[(size_t)s * n + f] : 0.0;   // zero weight kills padded rows
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < RJ / 16; ++t) {
      if (r0 + 16 * t >= n) break;
      double af[Q], br[4];
#pragma unroll
      for (int kk = 0; kk < Q; ++kk) af[kk] = ws[(16 * t + lr) * LD + kk * 4 + lk];
#pragma unroll
      for (int r = 0; r < 4; ++r) br[r] = s_h[16 * t + lk + 4 * r];
#pragma unroll
      for (int g = 0; g < CG; ++g) {
        double4_t ph = double4_t{br[0], br[1], br[2], br[3]};
#pragma unroll
        for (int kk = 0; kk < Q; ++kk) ph = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk], xb[g][kk], ph, 0, 0, 0);
        double v[4];
        if constexpr (KERN) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = kern_finish<KID>(fmax(fma(-2.0, ph[r], xn[g]), 0.0), kp);
        } else {
          bool big = false;
#pragma unroll
          for (int r = 0; r < 4; ++r) big |= !(fabs(ph[r]) < RFF_COS_FAST_RANGE);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = rff_cos_fast(ph[r], P);
          if (__builtin_amdgcn_ballot_w64(big)) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (!(fabs(ph[r]) < RFF_COS_FAST_RANGE)) v[r] = P.c[0] * rff_cos_slow(ph[r]);
          }
        }
        // k-step r of the second product: A[i = lr][k = lk] = C[sample 16 j + lr][row 16 t + 4 r + lk]
#pragma unroll
        for (int j = 0; j < SB; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[g][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(s_c[(16 * j + lr) * LO + 16 * t + 4 * r + lk], v[r],
                                                             acc[g][j], 0, 0, 0);
      }
    }
  }
}

// score[s][c] = a sum_f Wp[s][f] cos(w_f.x_c + b_f) + sum_i V[s][i] k(x_c, x_i)   (ppbo_path_score_multi)
// One workgroup: 4 wavefronts x CG groups of 16 candidates, SB blocks of 16 samples (blockIdx.y); the features, then the
// design rows, each in index order into one accumulator (no split, no atomics: a call is bitwise repeatable).  The two
// tile generators (cosine: ~20 fp64 VALU instructions per element; kernel value: ~20 for SE, ~35 for the Matern
// kernels, 8 for RQ) run serially with the matrix-core contraction -- fp64 VALU and fp64 MFMA share the CU's DP datapath.
// LDS: 32 rows x (DP + 2) + 32 + 16 SB x 33 doubles (34 KB at DP = 64, SB = 4).
template <int KID, int DP, int CG, int SB>
__global__ __launch_bounds__(256) void path_score_multi_kernel(const double* __restrict__ Xc, int M, int D,
                                                               const double* __restrict__ W, int F,
                                                               const double* __restrict__ b,
                                                               const double* __restrict__ Wp,
                                                               const double* __restrict__ X, int N, KernParams kp,
                                                               const double* __restrict__ V, int S, RffPoly P,
                                                               double* __restrict__ score) {
  constexpr int Q = DP / 4, LD = DP + 2, RJ = 32, NS = 16 * SB, LO = RJ + 1;
  __shared__ __attribute__((aligned(16))) double ws[RJ * LD];
  __shared__ double s_h[RJ];
  __shared__ double s_c[NS * LO];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int cw = blockIdx.x * (64 * CG) + wv * (16 * CG);
  const int s0 = blockIdx.y * NS;
  double xb[CG][Q], xn[CG];
  double4_t acc[CG][SB];
#pragma unroll
  for (int g = 0; g < CG; ++g) {
    const int c = cw + 16 * g + lr;
    double t = 0.0;
#pragma unroll
    for (int kk = 0; kk < Q; ++kk) {
      const int d = kk * 4 + lk;
      xb[g][kk] = (d < D && c < M) ? Xc[(size_t)c * D + d] : 0.0;
      t = fma(xb[g][kk], xb[g][kk], t);
    }
    // |x_c|^2: the four lanes (lr, 0..3) hold the coordinates of candidate lr between them
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    xn[g] = t;
#pragma unroll
    for (int j = 0; j < SB; ++j) acc[g][j] = double4_t{0.0, 0.0, 0.0, 0.0};
  }
  path_half<false, KID, DP, CG, SB>(W, F, D, b, Wp, S, s0, xb, xn, P, kp, ws, s_h, s_c, acc);
  path_half<true, KID, DP, CG, SB>(X, N, D, nullptr, V, S, s0, xb, xn, P, kp, ws, s_h, s_c, acc);
  // C/D map of the f64 form: acc[g][j][r] is sample 16 j + lk + 4 r of candidate lr
#pragma unroll
  for (int g = 0; g < CG; ++g) {
    const int c = cw + 16 * g + lr;
#pragma unroll
    for (int j = 0; j < SB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = s0 + 16 * j + lk + 4 * r;
        if (s < S && c < M) score[(size_t)s * M + c] = acc[g][j][r];
      }
  }
}

}  // namespace

extern "C" int ppbo_path_score_multi(ppbo_ctx* ctx, int kernel_id, const double theta[3], const double* d_Xc, int64_t M, int D,
                                     const double* d_W, int F, const double* d_b, const double* d_Wp, const double* d_X,
                                     int N, const double* d_V, int S, double* d_score, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, theta && d_Xc && d_W && d_b && d_Wp && d_X && d_V && d_score, "null pointer");
  PPBO_REQUIRE(ctx, M > 0 && M < ((int64_t)1 << 31) && D > 0 && D <= 64 && F > 0 && N > 0, "sizes (D <= 64)");
  PPBO_REQUIRE(ctx, S > 0 && S <= PPBO_RFF_MULTI_MAX_S, "S (1 .. PPBO_RFF_MULTI_MAX_S samples)");
  hipStream_t s = (hipStream_t)stream;
  const RffPoly P = make_rff_poly(std::sqrt(2.0 * theta[2] * theta[2] / (double)F));
  const KernParams kp = make_kern_params(kernel_id, theta);
  // sample blocks as ppbo_rff_score_multi: one 16-sample block per workgroup for a handful of samples, four otherwise;
  // three dimension buckets (the ascent's), each padded with zero coordinates
  const bool one = S <= 16;
  const int mi = (int)M;
  return ppbo_kernel_dispatch<true>(ctx, kernel_id, [&](auto kid) -> int {
    constexpr int KID = decltype(kid)::value;
#define PSM_GO(DP, CG, SB)                                                                                              \
  path_score_multi_kernel<KID, DP, CG, SB><<<dim3((mi + 64 * CG - 1) / (64 * CG), (S + 16 * SB - 1) / (16 * SB)), 256, 0, s>>>( \
      d_Xc, mi, D, d_W, F, d_b, d_Wp, d_X, N, kp, d_V, S, P, d_score)
#define PSM_LAUNCH(DP, CG)      \
  do {                          \
    if (one) PSM_GO(DP, CG, 1); \
    else PSM_GO(DP, CG, 4);     \
  } while (0)
    if (D <= 8) PSM_LAUNCH(8, 4);
    else if (D <= 24) PSM_LAUNCH(24, 4);
    else PSM_LAUNCH(64, 2);
#undef PSM_LAUNCH
#undef PSM_GO
    PPBO_LAUNCH_CHECK(ctx);
    return 0;
  }, "invalid argument: kernel_id (a radial kernel: SE, RQ, Matern-5/2, Matern-3/2)");
}
