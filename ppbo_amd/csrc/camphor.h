// The camphor-copper kernel with one length scale per coordinate (include/ppbo_hip.h): SE with l = 1 on the embedded
// rows e(x) in R^11, column order (c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5).  Shared by camphor.hip (embedding, line
// points, the gradient's pull-back) and meangrad.hip (the mean gradient, mu_star and the RFF search in the caller's
// coordinates).
#pragma once
#include "common.h"

constexpr int CAMPHOR_D = 6;      // caller's coordinates: x, y, z, alpha, beta, gamma (z = coordinate 2, not periodic)
constexpr int CAMPHOR_E = 11;     // embedded width: two columns per periodic coordinate, one for z

// first embedded column of caller coordinate d: 0, 2, 4, 5, 7, 9
__host__ __device__ constexpr int camphor_col(int d) { return d < 2 ? 2 * d : (d == 2 ? 4 : 2 * d - 1); }

// 1 / l_d, passed by value
struct CamphorInvL { double v[CAMPHOR_D]; };
// the camphor form's coefficients in the caller's coordinates: 2 / l_d^2 (periodic d), 1 / (2 l_2^2) (z), passed by value
struct CamphorCoef { double k[CAMPHOR_D]; };

static inline bool camphor_l_valid(const double* h_l) {
  if (!h_l) return false;
  for (int d = 0; d < CAMPHOR_D; ++d)
    if (!(h_l[d] > 0.0 && std::isfinite(h_l[d]))) return false;
  return true;
}
static inline CamphorInvL camphor_inv_l(const double* h_l) {
  CamphorInvL r;
  for (int d = 0; d < CAMPHOR_D; ++d) r.v[d] = 1.0 / h_l[d];
  return r;
}
static inline CamphorCoef camphor_coef(const double* h_l) {
  CamphorCoef c;
  for (int d = 0; d < CAMPHOR_D; ++d) c.k[d] = (d == 2 ? 0.5 : 2.0) / (h_l[d] * h_l[d]);
  return c;
}

namespace {
// L.v[d] for a lane-dependent d without dynamic indexing of a by-value argument (which would go through scratch)
__device__ __forceinline__ double camphor_pick(const CamphorInvL& L, int d) {
  return d == 0 ? L.v[0] : d == 1 ? L.v[1] : d == 2 ? L.v[2] : d == 3 ? L.v[3] : d == 4 ? L.v[4] : L.v[5];
}

// the embedded columns of coordinate d of one point with value v
__device__ __forceinline__ void camphor_embed_one(double v, int d, const CamphorInvL& L, double* __restrict__ row) {
  const double il = camphor_pick(L, d);
  double* o = row + camphor_col(d);
  if (d == 2) { o[0] = v * il; return; }
  o[0] = cospi(2.0 * v) * il;
  o[1] = sinpi(2.0 * v) * il;
}
}  // namespace

// h_l: six positive finite length scales; a model: SE at D = 11 (embedded rows, theta = [sigma, 1, sigma_f])
#define PPBO_REQUIRE_CAMPHOR_L(ctx, h_l) \
  PPBO_REQUIRE(ctx, camphor_l_valid(h_l), "h_l: six positive finite length scales")
#define PPBO_REQUIRE_CAMPHOR_MODEL(ctx, m)                                                                         \
  PPBO_REQUIRE(ctx, (m) != nullptr && (m)->d_X && (m)->d_alpha && (m)->N > 0 && (m)->kernel_id == PPBO_KERNEL_SE && \
                        (m)->D == CAMPHOR_E, "a camphor model is SE on embedded rows (D = 11) with X / alpha")

// d_grad[M][6] from the embedded points d_e and a gradient d_g on them (both [M][11]); inv_lz = 1 / l_2 (camphor.hip)
int ppbo_camphor_pullback(ppbo_ctx* ctx, const double* d_e, const double* d_g, int64_t M, double inv_lz, double* d_grad,
                          hipStream_t s);
