// Knowledge gradient for correlated beliefs (Frazier, Powell and Dayanik 2009): the expected maximum of up to 1025 lines
// a_j + b_j Z, Z ~ N(0, 1), per candidate, exactly -- ppbo_kg_envelope, and behind the tournament's cross product
// ppbo_predict_kg (predict.hip), which hands this file the covariances and lets it divide them by s_i on the way in.
//
// With the lines of the upper envelope h(z) = max_j (a_j + b_j z) in order of slope, kinks c_k and slopes beta_k,
//   E[h(Z)] - h(0) = sum_k (beta_{k+1} - beta_k) psi(|c_k|),   psi(c) = phi(c) - c Phi(-c) >= 0.
// The envelope is found by a gift-wrapping march: start on the line of the smallest slope (of equal slopes the largest
// intercept: it is the envelope at z -> -inf); standing on (a_cur, b_cur), every steeper line crosses it at
// c_j = (a_cur - a_j) / (b_j - b_cur), and the next line of the envelope is the one that crosses first (of equal c the
// steepest: the lines through one point that it skips are never on top).  On GP-shaped inputs the march takes 3 to 13
// steps whatever the number of lines; sorting them by slope first would cost more than all of its steps.
//
// A fixed group of LANES lanes works on one candidate and keeps its lines in registers, LPL field lines per lane (line
// j in lane j % LANES) and the candidate's own line in lane 0.  Every reduction of a step is a minimum or a maximum over
// the group -- the smallest c, then the largest slope among those, then the largest intercept among those -- and the
// sum runs in march order, so the result is a function of the SET of lines: the order of the field, duplicated lines
// and the other rows of the call change no bit of it.
// The loop is counted: the slope strictly increases from step to step, so n lines give at most n - 1 kinks, and the
// n-th pass finds no steeper line and leaves.  No exit depends on a floating-point comparison coming out one way.
#include "common.h"
#include "score.h"

namespace {

constexpr int KG_THREADS = 256;
constexpr double KG_DBL_MAX = 1.7976931348623157e308;

// psi(c) = phi(c) - c Phi(-c) for c >= 0, with Phi(-c) formed directly (no 1 - Phi).  Both terms are 0 in fp64 from
// c = 40 on (exp(-800), erfc(28.3)); there, and for c = inf (a crossing that overflowed), psi is 0 and never inf * 0.
// The two terms cancel to phi(c) / c^2 for large c: the last bits may leave a negative difference, clipped.
__device__ __forceinline__ double kg_psi(double c) {
  if (!(c < 40.0)) return 0.0;
  return fmax(__builtin_fma(-c, norm_cdf(-c), 0.39894228040143267794 * exp_nonpos(-0.5 * c * c)), 0.0);
}

template <int LANES>
__device__ __forceinline__ double group_min(double v) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, LANES));
  return v;
}
template <int LANES>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
  for (int o = LANES / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, LANES));
  return v;
}

// One group of LANES lanes per candidate row; a [Mb] the intercepts of the field lines (the same for every row), slope
// [Ma][ld] their slopes -- divided by div[row] on the way in when div is given (0 / 0 = 0: a candidate without variance
// observed without noise moves nothing) -- and (self_a, self_b) [Ma] the row's own line, NULL for none.  A line that is
// not finite (NaN or inf, intercept or slope) gives the row NaN: a NaN intercept of the field poisons every row, a NaN
// slope or own line its own row only.  kinks [Ma] (NULL: not wanted) = the steps the march took, 0 for a NaN row.
// blk_best [gridDim.x]: the block's largest KG and its first row + idx_base; NaN never wins.
// With the points behind the lines (xa [Ma][D], xb [Mb][D]; ppbo_predict_kg) a field point that IS the row's candidate --
// the same intercept and the same D coordinates, bit for bit -- takes the own line's slope: cov(a, a) is var(a), and the
// cross product's few-ulp different sum of the same quadratic form would leave two beliefs where there is one.
template <int LANES, int LPL>
__global__ __launch_bounds__(KG_THREADS) void kg_envelope_kernel(
    const double* __restrict__ a, const double* __restrict__ slope, long long ld, const double* __restrict__ div,
    const double* __restrict__ self_a, const double* __restrict__ self_b, long long Ma, int Mb, long long idx_base,
    double* __restrict__ kg_out, int* __restrict__ kinks_out, Best* __restrict__ blk_best,
    const double* __restrict__ xa, const double* __restrict__ xb, int D) {
  static_assert(KG_THREADS % LANES == 0 && (LANES == 16 || LANES == 64), "a group is a quarter of a wavefront or a whole one");
  __shared__ Best sh[KG_THREADS / 64];
  constexpr int GROUPS = KG_THREADS / LANES, NL = LPL + 1;
  const int gl = threadIdx.x % LANES;
  const long long row = (long long)blockIdx.x * GROUPS + threadIdx.x / LANES;
  Best best{0.0, -1};
  if (row < Ma) {                                 // (the same for every lane of a group, as every branch below)
    // padding: slope -inf is steeper than nothing and is left out of the start by name
    double la[NL], lb[NL];
    int bad = 0;
    const double dv = div ? div[row] : 1.0;
    const double* srow = slope + row * ld;
    const double own_a = self_a ? self_a[row] : 0.0, own_b = self_a ? self_b[row] : 0.0;
#pragma unroll
    for (int k = 0; k < LPL; ++k) {
      const int j = gl + LANES * k;
      la[k] = -INFINITY;
      lb[k] = -INFINITY;
      if (j < Mb) {
        double sv = srow[j];
        if (div) sv = (dv == 0.0 && sv == sv) ? 0.0 : sv / dv;
        la[k] = a[j];
        if (xa && self_a && la[k] == own_a) {     // (rare: the coordinates are read only behind an equal mean)
          bool same = true;
          for (int d = 0; d < D; ++d) same = same && (xa[row * D + d] == xb[(long long)j * D + d]);
          if (same) sv = own_b;
        }
        lb[k] = sv;
        bad |= !(fabs(la[k]) <= KG_DBL_MAX) || !(fabs(sv) <= KG_DBL_MAX);
      }
    }
    la[LPL] = -INFINITY;
    lb[LPL] = -INFINITY;
    if (self_a && gl == 0) {
      la[LPL] = own_a;
      lb[LPL] = own_b;
      bad |= !(fabs(la[LPL]) <= KG_DBL_MAX) || !(fabs(lb[LPL]) <= KG_DBL_MAX);
    }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, LANES);
    double kg = NAN;
    int kinks = 0;
    if (!bad) {
      double bcur = INFINITY, acur = -INFINITY;
#pragma unroll
      for (int k = 0; k < NL; ++k)
        if (lb[k] != -INFINITY) bcur = fmin(bcur, lb[k]);
      bcur = group_min<LANES>(bcur);
#pragma unroll
      for (int k = 0; k < NL; ++k)
        if (lb[k] == bcur) acur = fmax(acur, la[k]);
      acur = group_max<LANES>(acur);
      kg = 0.0;
      const int n_lines = Mb + (self_a ? 1 : 0);
      for (int step = 0; step < n_lines; ++step) {
        // the lane's own best line under (smallest c, then largest slope, then largest intercept): a total order, so
        // the order of the lines within a lane does not matter either
        double cl = INFINITY, bl = -INFINITY, al = -INFINITY;
#pragma unroll
        for (int k = 0; k < NL; ++k)
          if (lb[k] > bcur) {
            const double c = (acur - la[k]) / (lb[k] - bcur);
            if (c < cl || (c == cl && (lb[k] > bl || (lb[k] == bl && la[k] > al)))) {
              cl = c;
              bl = lb[k];
              al = la[k];
            }
          }
        const double cmin = group_min<LANES>(cl);
        const double bsel = group_max<LANES>(cl == cmin ? bl : -INFINITY);
        if (bsel == -INFINITY) break;             // no steeper line is left
        const double asel = group_max<LANES>((cl == cmin && bl == bsel) ? al : -INFINITY);
        kg += (bsel - bcur) * kg_psi(fabs(cmin));
        acur = asel;
        bcur = bsel;
        ++kinks;
      }
    }
    if (gl == 0) {
      kg_out[row] = kg;
      if (kinks_out) kinks_out[row] = kinks;
      if (kg == kg) { best.val = kg; best.idx = idx_base + row; }
    }
  }
  best = block_best(best, sh);
  if (threadIdx.x == 0 && blk_best) blk_best[blockIdx.x] = best;
}

// s = sqrt(max(var, 0) + noise_var) and the slope of the candidate's own line max(var, 0) / s (0 for s = 0); a NaN
// variance stays NaN in both
__global__ __launch_bounds__(256) void kg_rows_kernel(const double* __restrict__ var, double noise_var, int M,
                                                      double* __restrict__ s_out, double* __restrict__ self_b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const double v = var[i], vc = (v != v) ? v : fmax(v, 0.0);
  const double s = sqrt(vc + noise_var);
  s_out[i] = s;
  self_b[i] = (s == 0.0) ? 0.0 : vc / s;
}

// rows per workgroup: groups of 16 lanes up to 256 field lines, whole wavefronts above
inline int kg_groups(int Mb) { return Mb <= 256 ? KG_THREADS / 16 : KG_THREADS / 64; }

}  // namespace

long long ppbo_kg_blocks(long long Ma, int Mb) {
  const int g = kg_groups(Mb);
  return (Ma + g - 1) / g;
}

int ppbo_kg_rows(ppbo_ctx* ctx, const double* d_var, double noise_var, int M, double* d_s, double* d_self_b, hipStream_t s) {
  kg_rows_kernel<<<(M + 255) / 256, 256, 0, s>>>(d_var, noise_var, M, d_s, d_self_b);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

int ppbo_kg_launch(ppbo_ctx* ctx, const double* d_a, const double* d_slope, long long ld, const double* d_div,
                   const double* d_self_a, const double* d_self_b, long long Ma, int Mb, long long idx_base, double* d_kg,
                   int* d_kinks, void* blk_best, hipStream_t s, const double* d_Xa, const double* d_Xb, int D) {
  const unsigned nblk = (unsigned)ppbo_kg_blocks(Ma, Mb);
  Best* bb = (Best*)blk_best;
  if (Mb <= 64)
    kg_envelope_kernel<16, 4><<<nblk, KG_THREADS, 0, s>>>(d_a, d_slope, ld, d_div, d_self_a, d_self_b, Ma, Mb, idx_base, d_kg,
                                                          d_kinks, bb, d_Xa, d_Xb, D);
  else if (Mb <= 256)
    kg_envelope_kernel<16, 16><<<nblk, KG_THREADS, 0, s>>>(d_a, d_slope, ld, d_div, d_self_a, d_self_b, Ma, Mb, idx_base, d_kg,
                                                           d_kinks, bb, d_Xa, d_Xb, D);
  else
    kg_envelope_kernel<64, 16><<<nblk, KG_THREADS, 0, s>>>(d_a, d_slope, ld, d_div, d_self_a, d_self_b, Ma, Mb, idx_base, d_kg,
                                                           d_kinks, bb, d_Xa, d_Xb, D);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" {

int ppbo_kg_envelope(ppbo_ctx* ctx, const double* d_a, const double* d_slope, int64_t ld, const double* d_self_a,
                     const double* d_self_b, int64_t Ma, int Mb, double* d_kg, int* d_kinks, double* h_best_val,
                     int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  PPBO_REQUIRE(ctx, d_a != nullptr && d_slope != nullptr && d_kg != nullptr, "kg_envelope (d_a / d_slope / d_kg)");
  PPBO_REQUIRE(ctx, Ma >= 1 && Ma <= (int64_t)0x7fffffff, "row count (1 .. 2^31 - 1)");
  PPBO_REQUIRE(ctx, Mb >= 1 && Mb <= PPBO_KG_MAX_B, "line count (1 .. PPBO_KG_MAX_B)");
  PPBO_REQUIRE(ctx, ld >= Mb, "ld (at least Mb)");
  PPBO_REQUIRE(ctx, (d_self_a == nullptr) == (d_self_b == nullptr), "the own line needs both d_self_a and d_self_b");
  const bool want_best = h_best_val || h_best_idx;
  const long long nblk = ppbo_kg_blocks(Ma, Mb);
  Best* bests = nullptr;
  PpboHostRecord hr{};
  if (want_best) {
    bests = (Best*)ppbo_workspace(ctx, ppbo_ctx::WS_SMALL, (size_t)nblk * sizeof(Best));
    if (!bests) return (int)hipErrorOutOfMemory;
    if (int rc = ppbo_host_record(ctx, &hr)) return rc;
  }
  {
    PpboProfScope pf(ctx, ppbo_ctx::PF_KG, s);
    if (int rc = ppbo_kg_launch(ctx, d_a, d_slope, ld, nullptr, d_self_a, d_self_b, Ma, Mb, 0, d_kg, d_kinks, bests, s)) return rc;
  }
  if (!want_best) return 0;
  argmax_final_kernel<<<1, 256, 0, s>>>(bests, (int)nblk, nullptr, hr.d_rec, 0, hr.d_flag, hr.epoch);
  PPBO_LAUNCH_CHECK(ctx);
  if (int rc = ppbo_host_record_wait(ctx, hr, s)) return rc;
  if (h_best_val) *h_best_val = hr.h_rec[0];      // (NaN, -1) when every row is NaN
  if (h_best_idx) *h_best_idx = (int64_t)hr.h_rec[1];
  return 0;
}

}  // extern "C"
