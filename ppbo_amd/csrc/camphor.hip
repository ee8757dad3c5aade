// The camphor-copper kernel with one length scale per coordinate (no reference counterpart; the reference's kernel,
// src/kernels.py:36-53, is the profile l = (l, l, l + 0.05, l, l, l)).  With e(x) in R^11,
//   e = (c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5),   c_d = cos(2 pi x_d) / l_d,  s_d = sin(2 pi x_d) / l_d,  z = x_2 / l_2,
// |e_d(x) - e_d(x')|^2 = (2 - 2 cos(2 pi dx_d)) / l_d^2 = 4 sin^2(pi dx_d) / l_d^2, so camphor(x, x'; l) = SE(e(x), e(x'); 1)
// exactly and the whole SE machinery runs on the embedded rows.  What works in the caller's coordinates is here:
//   ppbo_camphor_embed        e of M rows: one thread per (row, coordinate), sinpi / cospi (exact range reduction)
//   ppbo_camphor_line_points  the embedded points of B lines x_b + alpha_g xi_b (the line is not linear in e)
//   ppbo_camphor_pullback     (internal) a gradient on the embedded points pulled back through de/dx, for ppbo_mean_grad:
//                             d mu / d x_d = 2 pi (c_d g_s - s_d g_c) (periodic d),  g_z / l_2 (z)
// Everything that reads a model's coordinate map (ppbo_coords with PPBO_COORDS_CAMPHOR: the mean gradient, mu_star and
// the RFF search in the caller's coordinates) lives in meangrad.hip beside the search it reuses.
#include "camphor.h"

namespace {

// rows of one embedding / pull-back launch: one thread per (row, coordinate), 256 per block, grid.x <= 2^31 - 1
constexpr long long CAMPHOR_MAX_ROWS = ((1LL << 31) - 1) * 256 / CAMPHOR_D;

// [a, a + na) and [b, b + nb) (in doubles) share memory
inline bool camphor_overlap(const double* a, long long na, const double* b, long long nb) {
  return a < b + nb && b < a + na;
}

__global__ __launch_bounds__(256) void camphor_embed_kernel(const double* __restrict__ in, int64_t n, CamphorInvL L,
                                                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // i = row * 6 + d
  if (i >= n) return;
  const int64_t r = i / CAMPHOR_D;
  camphor_embed_one(in[i], (int)(i - r * CAMPHOR_D), L, out + r * CAMPHOR_E);
}

// line points formed as line_grid_kernel (predict.hip) forms them, a xi + x, then embedded; out row = b G + g
__global__ __launch_bounds__(256) void camphor_line_points_kernel(const double* __restrict__ xi, const double* __restrict__ x,
                                                                  const double* __restrict__ alpha, int per_line, int B,
                                                                  int G, CamphorInvL L, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * G * CAMPHOR_D) return;
  const int d = (int)(e % CAMPHOR_D);
  const long long bg = e / CAMPHOR_D;
  const int g = (int)(bg % G), b = (int)(bg / G);
  const double a = alpha[per_line ? (size_t)b * G + g : g];
  const double v = a * xi[(size_t)b * CAMPHOR_D + d] + x[(size_t)b * CAMPHOR_D + d];
  camphor_embed_one(v, d, L, out + (size_t)bg * CAMPHOR_E);
}

// grad[r][d] from the embedded point e[r] and the embedded gradient g[r] (both [M][11])
__global__ __launch_bounds__(256) void camphor_pullback_kernel(const double* __restrict__ e, const double* __restrict__ g,
                                                               int64_t n, double inv_lz, double* __restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // i = row * 6 + d
  if (i >= n) return;
  const int64_t r = i / CAMPHOR_D;
  const int d = (int)(i - r * CAMPHOR_D), c = camphor_col(d);
  const double* er = e + r * CAMPHOR_E;
  const double* gr = g + r * CAMPHOR_E;
  grad[i] = (d == 2) ? gr[c] * inv_lz : 6.28318530717958647693 * (er[c] * gr[c + 1] - er[c + 1] * gr[c]);
}

}  // namespace

extern "C" int ppbo_camphor_embed(ppbo_ctx* ctx, const double* d_in, int64_t M, const double* h_l, double* d_out,
                                  void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_in && d_out && M >= 0 && M <= CAMPHOR_MAX_ROWS, "rows (at most one launch grid) / output");
  PPBO_REQUIRE(ctx, !camphor_overlap(d_in, M * CAMPHOR_D, d_out, M * CAMPHOR_E), "d_out must not overlap d_in");
  PPBO_REQUIRE_CAMPHOR_L(ctx, h_l);
  if (M == 0) return 0;
  const int64_t n = M * CAMPHOR_D;
  camphor_embed_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_in, n, camphor_inv_l(h_l), d_out);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" int ppbo_camphor_line_points(ppbo_ctx* ctx, const double* d_xi, const double* d_x, const double* d_alpha,
                                        int alpha_per_line, int B, int G, const double* h_l, double* d_out, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_xi && d_x && d_alpha && d_out && B > 0 && G > 0 && (long long)B * G <= CAMPHOR_MAX_ROWS,
               "xi / x / alpha / output / B / G (B G rows: at most one launch grid)");
  const long long BG = (long long)B * G;
  PPBO_REQUIRE(ctx, !camphor_overlap(d_xi, (long long)B * CAMPHOR_D, d_out, BG * CAMPHOR_E) &&
                    !camphor_overlap(d_x, (long long)B * CAMPHOR_D, d_out, BG * CAMPHOR_E) &&
                    !camphor_overlap(d_alpha, alpha_per_line ? BG : G, d_out, BG * CAMPHOR_E),
               "d_out must not overlap the inputs");
  PPBO_REQUIRE_CAMPHOR_L(ctx, h_l);
  const long long n = (long long)B * G * CAMPHOR_D;
  camphor_line_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      d_xi, d_x, d_alpha, alpha_per_line != 0, B, G, camphor_inv_l(h_l), d_out);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

int ppbo_camphor_pullback(ppbo_ctx* ctx, const double* d_e, const double* d_g, int64_t M, double inv_lz, double* d_grad,
                          hipStream_t s) {
  const int64_t n = M * CAMPHOR_D;
  camphor_pullback_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_e, d_g, n, inv_lz, d_grad);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}
