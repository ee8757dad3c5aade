// Score finishing shared by ppbo_predict and ppbo_rff_score: partial-slab sums,
// variance / score evaluation and a deterministic argmax (first index wins ties,
// np.argmax semantics; NaN scores never win).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ double norm_cdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

struct Best {
  double val;
  long long idx;
};
__device__ __forceinline__ Best best_merge(Best a, Best b) {
  // larger value wins; ties -> smaller index (np.argmax first-occurrence); idx<0 == empty
  if (b.idx < 0) return a;
  if (a.idx < 0) return b;
  if (b.val > a.val || (b.val == a.val && b.idx < a.idx)) return b;
  return a;
}
__device__ __forceinline__ Best block_best(Best b, Best* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) b = best_merge(b, sh[w]);
  }
  return b;  // valid in thread 0
}

// Geometry of the score pass: a workgroup finishes SC_CAND candidates; its SC_WAVES wavefronts split the partial slabs
// of those candidates between them (wavefront w sums slabs w, w + SC_WAVES, ...: every load of the pass is in flight at
// once -- the first version had one thread walk all 2 n_mu + n_slab slabs of its candidate, a dependent chain of up
// to 144 strided loads: 38 us for 8192 candidates, 27 us for 65536, on a pass that moves 9-25 MB), the wavefront
// sums meet in LDS and are added in wavefront order (a fixed order: results do not depend on timing).
// The launch-wide best is a SECOND, one-workgroup launch (argmax_final_kernel).  Round 4 tried to fold it into this
// kernel ("the last workgroup to retire merges the records": a device-scope ticket per workgroup): the tickets cost
// ~40 ns per workgroup whatever their layout -- one word, or 32 group words + a top word -- because every one of
// them is a release at device scope: 45-51 us for the 1024 workgroups of a 65536-candidate launch against 6 + 3 us
// for the two launches.
constexpr int SC_CAND = 64, SC_WAVES = 16, SC_THREADS = SC_CAND * SC_WAVES;
static inline int score_blocks(long long M) { return (int)((M + SC_CAND - 1) / SC_CAND); }

// the score of a candidate from its mean and variance: score_kernel's expression, shared with the bounds of the pruned
// search (prune_bounds_kernel evaluates it at the two ends of a variance interval)
__device__ __forceinline__ double score_value(double mu, double var, int kind, double mustar) {
  double sc;
  if (mu != mu) sc = mu;                 // a NaN mean (kstar_kernel: a candidate with a non-finite coordinate) never scores
  else if (kind == PPBO_SCORE_MEAN) sc = mu;
  else if (kind == PPBO_SCORE_VARIANCE) sc = var;
  else {
    const double d = mu - mustar;
    const double sd = sqrt(fmax(var, 0.0));
    if (sd > 0.0) {
      const double z = d / sd;
      sc = d * norm_cdf(z) + sd * 0.39894228040143267794 * exp(-0.5 * z * z);
    } else sc = fmax(d, 0.0);
  }
  return sc;
}

// The plan of a pruned search chunk (prune_select_kernel writes it, the launches behind it read it): pruned = 1: only
// the n_surv candidates idx[0 .. n_surv), ascending, can hold the chunk's argmax and only they are contracted, in
// compact columns; pruned = 0: every launch does what it does without a plan.
struct PrunePlan {
  int pruned, n_surv;
};
__device__ __forceinline__ int uniform_load_int(const int* p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) int*>(reinterpret_cast<uintptr_t>(p));
}

// PLAN: with a pruned plan column j = the compact position: the partial sums of candidate idx[j], the slab of column j
// (row stride n_cap, the compact launch's), the reported index that of the candidate; columns from n_surv on are
// empty.  With pruned = 0, and without PLAN, today's pass over all M candidates.
template <bool PLAN>
__device__ __forceinline__ void score_body(const double* __restrict__ mu_part, int n_mu,
                                           const double* __restrict__ t_part,
                                           const double* __restrict__ slab, int n_slab, int M,
                                           double sf2, int kind, double mustar, long long idx_base,
                                           double* __restrict__ mu_out, double* __restrict__ var_out,
                                           double* __restrict__ score_out, Best* __restrict__ blk_best,
                                           const PrunePlan* __restrict__ plan, const int* __restrict__ idx, int n_cap) {
  __shared__ double part[3][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int c = blockIdx.x * SC_CAND + lane;   // the candidate
  int j = c, ncol = M, lds = M;          // its slab column, the number of columns, the slab's row stride
  if constexpr (PLAN) {
    if (uniform_load_int(&plan->pruned)) {
      ncol = uniform_load_int(&plan->n_surv);
      lds = n_cap;
      if (j < ncol) c = idx[j];
    }
  }
  double pm = 0.0, pt = 0.0, pq = 0.0;
  if (j < ncol) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    if (slab) {
      for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
      for (int s = wave; s < n_slab; s += SC_WAVES) pq += slab[(size_t)s * lds + j];
    }
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pq;
  __syncthreads();
  if (wave != 0) return;                 // the rest is one wavefront's work
  Best b{0.0, -1};
  if (j < ncol) {
    double mu = 0.0, t = 0.0, q = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { mu += part[0][w][lane]; t += part[1][w][lane]; q += part[2][w][lane]; }
    const double var = slab ? sf2 + t + q : sf2;
    const double sc = score_value(mu, var, kind, mustar);
    if (mu_out) mu_out[c] = mu;
    if (var_out) var_out[c] = var;
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  if (!blk_best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (lane == 0) blk_best[blockIdx.x] = b;
}

__global__ __launch_bounds__(SC_THREADS) void score_kernel(const double* __restrict__ mu_part, int n_mu,
                                                           const double* __restrict__ t_part,
                                                           const double* __restrict__ slab, int n_slab, int M,
                                                           double sf2, int kind, double mustar, long long idx_base,
                                                           double* __restrict__ mu_out, double* __restrict__ var_out,
                                                           double* __restrict__ score_out, Best* __restrict__ blk_best) {
  score_body<false>(mu_part, n_mu, t_part, slab, n_slab, M, sf2, kind, mustar, idx_base, mu_out, var_out, score_out,
                    blk_best, nullptr, nullptr, 0);
}
// score_kernel with a plan (the pruned search: the best only, no per-candidate output)
__global__ __launch_bounds__(SC_THREADS) void score_plan_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                const double* __restrict__ t_part,
                                                                const double* __restrict__ slab, int n_slab, int M,
                                                                double sf2, int kind, double mustar, long long idx_base,
                                                                Best* __restrict__ blk_best,
                                                                const PrunePlan* __restrict__ plan,
                                                                const int* __restrict__ idx, int n_cap) {
  score_body<true>(mu_part, n_mu, t_part, slab, n_slab, M, sf2, kind, mustar, idx_base, nullptr, nullptr, nullptr,
                   blk_best, plan, idx, n_cap);
}

// 1 - k(a, b) / sigma_f^2 from s, the summed kern_term<KID> of the DIRECT differences a - b, in a form that does not
// cancel where the two points nearly coincide (2 sigma_f^2 - 2 k(a, b) formed from k itself keeps 1e-16 sigma_f^2 of
// absolute error, all of the value at r ~ 1e-8 l); exactly 0 at s = 0
template <int KID>
__device__ __forceinline__ double kern_one_minus(double s, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    return -expm1(-p.c0 * s);
  } else if constexpr (KID == PPBO_KERNEL_RQ) {
    const double u = p.c0 * s, t = 1.0 + u;
    return u * (2.0 + u) / (t * t);
  } else if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    return -expm1(-s);
  } else {
    // Matern: 1 - (1 + a + w a^2) e^-a = e^-a (e^a - 1 - a - w a^2), w = 1/3 (5/2) or 0 (3/2), a = c r.  Below a = 1 the
    // bracket is its series (1/2 - w) a^2 + sum_{k >= 3} a^k / k! (all terms positive; a^21 / 21! < 2e-20); above, the
    // closed form loses at most three bits
    static_assert(kid_matern<KID>, "unknown kernel id");
    constexpr double w = (KID == PPBO_KERNEL_MATERN52) ? 1.0 / 3.0 : 0.0;
    const double a = p.c0 * sqrt(s);
    if (a >= 1.0) return 1.0 - fma(a, fma(a, w, 1.0), 1.0) * exp(-a);
    double term = a * a * 0.5, g = 0.0;
#pragma unroll
    for (int k = 3; k <= 20; ++k) { term *= a / (double)k; g += term; }
    return ((0.5 - w) * a * a + g) * exp(-a);
  }
}

// Pass 3 of ppbo_predict_pairs: score_kernel's slab sums (same geometry) for the column d = k(a, X) - k(b, X), then
//   mu_d = sum of the mean partials,   var_d = c(a, b) + d' Lambda d + |G d|^2,   c(a, b) = 2 sigma_f^2 - 2 k(a, b),
//   p = Phi(mu_d / sqrt(2 sigma^2 + max(var_d, 0)))
// c(a, b) comes from the direct differences a - b of the two rows (wavefront w sums the dimensions w, w + SC_WAVES, ...
// beside its slabs; the sums meet in wavefront order).  A NaN mean (a non-finite coordinate) gives NaN everywhere.
template <int KID>
__global__ __launch_bounds__(SC_THREADS) void pair_score_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                const double* __restrict__ t_part,
                                                                const double* __restrict__ slab, int n_slab, int M,
                                                                const double* __restrict__ Xa,
                                                                const double* __restrict__ Xb, int D, KernParams p,
                                                                double two_sigma2, int kind, long long idx_base,
                                                                double* __restrict__ mu_out, double* __restrict__ var_out,
                                                                double* __restrict__ prob_out,
                                                                double* __restrict__ score_out, Best* __restrict__ blk_best) {
  __shared__ double part[4][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SC_CAND + lane;
  double pm = 0.0, pt = 0.0, pq = 0.0, ps = 0.0;
  if (c < M) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    if (slab) {
      for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
      for (int s = wave; s < n_slab; s += SC_WAVES) pq += slab[(size_t)s * M + c];
      for (int d = wave; d < D; d += SC_WAVES) ps += kern_term<KID>(Xa[(size_t)c * D + d] - Xb[(size_t)c * D + d], d, p);
    }
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pq;
  part[3][wave][lane] = ps;
  __syncthreads();
  if (wave != 0) return;                 // the rest is one wavefront's work
  Best b{0.0, -1};
  if (c < M) {
    double mu = 0.0, t = 0.0, q = 0.0, s = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { mu += part[0][w][lane]; t += part[1][w][lane]; q += part[2][w][lane]; s += part[3][w][lane]; }
    double var = NAN, pr = NAN, sc = mu;   // mean only (no slab): nothing but mu is formed
    if (slab) {
      var = 2.0 * p.sf2 * kern_one_minus<KID>(s, p) + t + q;
      const double den = sqrt(two_sigma2 + fmax(var, 0.0));
      // den = 0 (no noise, no variance): the sign of mu_d decides, a tie is 1/2
      pr = norm_cdf(den > 0.0 ? mu / den : (mu > 0.0 ? INFINITY : (mu < 0.0 ? -INFINITY : 0.0)));
      if (mu != mu) { var = mu; pr = mu; }
      if (kind == PPBO_PAIR_VARIANCE) sc = var;
      else if (kind == PPBO_PAIR_PROB) sc = pr;
    }
    if (mu_out) mu_out[c] = mu;
    if (var_out) var_out[c] = var;
    if (prob_out) prob_out[c] = pr;
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  if (!blk_best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (lane == 0) blk_best[blockIdx.x] = b;
}

// Pass 3 of ppbo_predict_slopes: score_kernel's slab sums (same geometry) for the column g = d/da k(x + a xi, X), then
//   mu_s = sum of the mean partials,   var_s = prior + g' Lambda g + |G g|^2,   p = Phi(mu_s / sqrt(max(var_s, 0)))
// prior = xi' (d^2 k / dx dx')(x, x) xi, a sum of squares over the dimensions (wavefront w sums the dimensions w,
// w + SC_WAVES, ... beside its slabs; the sums meet in wavefront order), so it does not see the sign of xi:
//   radial kernels   -c(0) |xi|^2, c = 2 dk/dr^2 (kern_slope_coef): 2 c0 sf2 (SE), 4 c0 sf2 (RQ), sf2 c0^2 / 3 (Matern-5/2),
//                    sf2 c0^2 (Matern-3/2) -- sf2 / l^2 times 1, 1, 5/3, 3
//   camphor-copper   sf2 (sum_{d != 2} 2 pi^2 c0 xi_d^2 + 2 c1 xi_2^2)
// No noise term: a slope is not an observation.  mu_s = var_s = 0 gives 1/2; a NaN mean (a non-finite coordinate) gives
// NaN everywhere.
template <int KID>
__device__ __forceinline__ double slope_prior_weight(int d, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) return 2.0 * p.c0 * p.sf2;
  else if constexpr (KID == PPBO_KERNEL_RQ) return 4.0 * p.c0 * p.sf2;
  else if constexpr (KID == PPBO_KERNEL_MATERN52) return p.sf2 * (p.c0 * p.c0) * (1.0 / 3.0);
  else if constexpr (KID == PPBO_KERNEL_MATERN32) return p.sf2 * (p.c0 * p.c0);
  else {
    static_assert(KID == PPBO_KERNEL_CAMPHOR, "unknown kernel id");
    return p.sf2 * (d == 2 ? 2.0 * p.c1 : 19.73920880217871723767 * p.c0);     // 2 pi^2
  }
}
template <int KID>
__global__ __launch_bounds__(SC_THREADS) void slope_score_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                 const double* __restrict__ t_part,
                                                                 const double* __restrict__ slab, int n_slab, int M,
                                                                 const double* __restrict__ Xi, int D, KernParams p,
                                                                 int kind, long long idx_base,
                                                                 double* __restrict__ mu_out, double* __restrict__ var_out,
                                                                 double* __restrict__ prob_out,
                                                                 double* __restrict__ score_out, Best* __restrict__ blk_best) {
  __shared__ double part[4][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SC_CAND + lane;
  double pm = 0.0, pt = 0.0, pq = 0.0, ps = 0.0;
  if (c < M) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    if (slab) {
      for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
      for (int s = wave; s < n_slab; s += SC_WAVES) pq += slab[(size_t)s * M + c];
      for (int d = wave; d < D; d += SC_WAVES) {
        const double w = Xi[(size_t)c * D + d];
        ps += slope_prior_weight<KID>(d, p) * (w * w);
      }
    }
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pq;
  part[3][wave][lane] = ps;
  __syncthreads();
  if (wave != 0) return;                 // the rest is one wavefront's work
  Best b{0.0, -1};
  if (c < M) {
    double mu = 0.0, t = 0.0, q = 0.0, s = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { mu += part[0][w][lane]; t += part[1][w][lane]; q += part[2][w][lane]; s += part[3][w][lane]; }
    double var = NAN, pr = NAN, sc = mu;   // mean only (no slab): nothing but mu is formed
    if (slab) {
      var = s + t + q;
      const double sd = sqrt(fmax(var, 0.0));
      // sd = 0 (no variance): the sign of mu_s decides, a tie is 1/2
      pr = norm_cdf(sd > 0.0 ? mu / sd : (mu > 0.0 ? INFINITY : (mu < 0.0 ? -INFINITY : 0.0)));
      if (mu != mu) { var = mu; pr = mu; }
      if (kind == PPBO_SLOPE_VARIANCE) sc = var;
      else if (kind == PPBO_SLOPE_PROB) sc = pr;
    }
    if (mu_out) mu_out[c] = mu;
    if (var_out) var_out[c] = var;
    if (prob_out) prob_out[c] = pr;
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  if (!blk_best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (lane == 0) blk_best[blockIdx.x] = b;
}

// Pass 3 of ppbo_predict_curvatures: slope_score_kernel's plan for the column c = d^2/da^2 k(gamma(a), X) at a = 0, then
//   mu_c = sum of the mean partials,   var_c = prior + c' Lambda c + |G c|^2,   p = P(curvature < 0) = Phi(-mu_c / sqrt(max(var_c, 0)))
// prior = Var[d^2/da^2 f(gamma(a))] = q4 n2^2 + q2 |acc|^2 (the cross term vanishes for a stationary kernel), from two
// sums over the dimensions, n2 = |xi|^2 and, when accelerations are given, |acc|^2 (wavefront w sums the dimensions w,
// w + SC_WAVES, ... beside its slabs; the sums meet in wavefront order):
//   q2 = -c(0), slope_prior_weight's constant;   q4 = 6 c'(0): 12 c0^2 sf2 (SE), 72 c0^2 sf2 (RQ), c0^4 sf2 (Matern-5/2)
//                                                -- sf2 / l^4 times 3, 9/2, 25
//   camphor-copper   sf2 (12 A^2 + 8 pi^4 c0 sum_{d != 2} xi_d^4), A = sum_{d != 2} pi^2 c0 xi_d^2 + c1 xi_2^2: the two
//                    sums are A and sum xi_d^4 (no acceleration there)
// Even in xi, so -xi leaves all three outputs bitwise unchanged.  No noise term.  var_c = 0: the sign of mu_c decides,
// mu_c = 0 gives 1/2; a NaN mean (a non-finite coordinate) gives NaN everywhere.
template <int KID>
__global__ __launch_bounds__(SC_THREADS) void curv_score_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                const double* __restrict__ t_part,
                                                                const double* __restrict__ slab, int n_slab, int M,
                                                                const double* __restrict__ Xi, const double* __restrict__ Xa,
                                                                int D, KernParams p, int kind, long long idx_base,
                                                                double* __restrict__ mu_out, double* __restrict__ var_out,
                                                                double* __restrict__ prob_out,
                                                                double* __restrict__ score_out, Best* __restrict__ blk_best) {
  static_assert(KID != PPBO_KERNEL_MATERN32, "no curvature for Matern-3/2");
  __shared__ double part[5][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SC_CAND + lane;
  double pm = 0.0, pt = 0.0, pq = 0.0, ps = 0.0, pa = 0.0;
  if (c < M) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    if (slab) {
      for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
      for (int s = wave; s < n_slab; s += SC_WAVES) pq += slab[(size_t)s * M + c];
      for (int d = wave; d < D; d += SC_WAVES) {
        const double w = Xi[(size_t)c * D + d];
        if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
          const double w2 = w * w;
          ps += (d == 2 ? p.c1 : 9.86960440108935861883 * p.c0) * w2;      // pi^2
          if (d != 2) pa += w2 * w2;
        } else {
          ps += w * w;
          if (Xa) {
            const double a = Xa[(size_t)c * D + d];
            pa += a * a;
          }
        }
      }
    }
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pq;
  part[3][wave][lane] = ps;
  part[4][wave][lane] = pa;
  __syncthreads();
  if (wave != 0) return;                 // the rest is one wavefront's work
  Best b{0.0, -1};
  if (c < M) {
    double mu = 0.0, t = 0.0, q = 0.0, s = 0.0, a = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) {
      mu += part[0][w][lane]; t += part[1][w][lane]; q += part[2][w][lane]; s += part[3][w][lane]; a += part[4][w][lane];
    }
    double var = NAN, pr = NAN, sc = mu;   // mean only (no slab): nothing but mu is formed
    if (slab) {
      double prior;
      if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
        prior = p.sf2 * fma(12.0 * s, s, (779.27272827201949789152 * p.c0) * a);       // 8 pi^4
      } else {
        const double c02 = p.c0 * p.c0;
        const double q4 = KID == PPBO_KERNEL_SE ? 12.0 * c02 * p.sf2 : (KID == PPBO_KERNEL_RQ ? 72.0 * c02 * p.sf2 : c02 * c02 * p.sf2);
        prior = fma(q4 * s, s, slope_prior_weight<KID>(0, p) * a);
      }
      var = prior + t + q;
      const double sd = sqrt(fmax(var, 0.0));
      // sd = 0 (no variance): the sign of mu_c decides, a tie is 1/2
      pr = norm_cdf(sd > 0.0 ? -mu / sd : (mu > 0.0 ? -INFINITY : (mu < 0.0 ? INFINITY : 0.0)));
      if (mu != mu) { var = mu; pr = mu; }
      if (kind == PPBO_CURV_VARIANCE) sc = var;
      else if (kind == PPBO_CURV_PROB) sc = pr;
    }
    if (mu_out) mu_out[c] = mu;
    if (var_out) var_out[c] = var;
    if (prob_out) prob_out[c] = pr;
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  if (!blk_best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (lane == 0) blk_best[blockIdx.x] = b;
}

// The prior term of ppbo_predict_functionals, prior[c] = w' K w for group c, rearranged so that nothing cancels between
// nearby points:
//   w' K w = sigma_f^2 (sum_g w_g)^2 - 2 sigma_f^2 sum_{g < h} w_g w_h (1 - k(x_g, x_h) / sigma_f^2)
// with the bracket from the direct differences x_g - x_h through kern_one_minus (pair_score_kernel's prior term): a
// contrast (sum w = 0) between nearby points keeps its digits, and two coincident points contribute exactly 0.
// One wavefront = one group: its G points go to LDS once (coalesced reads, rows padded to D + 1), lane l takes the pairs
// l, l + 64, ... of the G (G - 1) / 2 in row-major order of (g, h), the lane sums meet in a fixed exchange order, and
// sum_g w_g is added in index order.  w_g w_h and the square do not see the sign of w, so -w leaves the term bitwise
// unchanged; 2 w gives exactly four times it.  (With slope_score_kernel's geometry -- one lane per group, the pairs
// dealt to the workgroup's wavefronts -- every load of a point touched 64 cache lines: 25.4 ms for 65536 groups of
// G = 64 at D = 20, 0.97 ms at G = 16.)  Dynamic LDS: (blockDim.x / 64) G (D + 1) doubles.
__device__ __forceinline__ int functional_pair_offset(int g, int G) { return g * (2 * G - g - 1) / 2; }   // pairs before row g
template <int KID>
__global__ __launch_bounds__(256) void functional_prior_kernel(const double* __restrict__ Xg, const double* __restrict__ W,
                                                               int w_stride, int G, int D, int M, KernParams p,
                                                               double* __restrict__ prior) {
  extern __shared__ double fp_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, LD = D + 1;
  const int c = blockIdx.x * (blockDim.x >> 6) + wave;
  if (c >= M) return;                      // (a whole wavefront; no workgroup barrier below)
  double* __restrict__ xs = fp_lds + (size_t)wave * G * LD;
  const double* __restrict__ xg = Xg + (size_t)c * G * D;
  const double* __restrict__ w = W + (size_t)c * w_stride;
  for (int e = lane; e < G * D; e += 64) {
    const int g = e / D, d = e - g * D;
    xs[g * LD + d] = xg[e];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int npairs = G * (G - 1) / 2;
  double ps = 0.0;
  for (int q = lane; q < npairs; q += 64) {
    // row g of pair q: the root of g (2 G - g - 1) / 2 = q, corrected by at most a step either way
    const double tg = 2.0 * G - 1.0;
    int g = (int)((tg - sqrt(tg * tg - 8.0 * q)) * 0.5);
    if (g < 0) g = 0;
    if (g > G - 2) g = G - 2;
    while (g < G - 2 && functional_pair_offset(g + 1, G) <= q) ++g;
    while (g > 0 && functional_pair_offset(g, G) > q) --g;
    const int h = g + 1 + (q - functional_pair_offset(g, G));
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += kern_term<KID>(xs[g * LD + d] - xs[h * LD + d], d, p);
    ps += (w[g] * w[h]) * kern_one_minus<KID>(s, p);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
  if (lane == 0) {
    double sw = 0.0;
    for (int g = 0; g < G; ++g) sw += w[g];
    prior[c] = p.sf2 * (sw * sw - 2.0 * ps);
  }
}

// Pass 3 of ppbo_predict_functionals: score_kernel's slab sums (same geometry) for the column c = sum_g w_g k(x_g, X),
// then with prior[c] of functional_prior_kernel
//   mu = sum of the mean partials,   var = prior + c' Lambda c + |G c|^2,   p = P(L f > threshold) = Phi((mu - threshold) / sqrt(max(var, 0)))
// No noise term.  var = 0: the sign of mu - threshold decides, equality gives 1/2; a NaN mean (a non-finite coordinate)
// gives NaN everywhere.
__global__ __launch_bounds__(SC_THREADS) void functional_score_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                      const double* __restrict__ t_part,
                                                                      const double* __restrict__ slab, int n_slab, int M,
                                                                      const double* __restrict__ prior,
                                                                      double threshold, int kind, long long idx_base,
                                                                      double* __restrict__ mu_out, double* __restrict__ var_out,
                                                                      double* __restrict__ prob_out,
                                                                      double* __restrict__ score_out, Best* __restrict__ blk_best) {
  __shared__ double part[3][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SC_CAND + lane;
  double pm = 0.0, pt = 0.0, pq = 0.0;
  if (c < M) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    if (slab) {
      for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
      for (int s = wave; s < n_slab; s += SC_WAVES) pq += slab[(size_t)s * M + c];
    }
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pq;
  __syncthreads();
  if (wave != 0) return;                 // the rest is one wavefront's work
  Best b{0.0, -1};
  if (c < M) {
    double mu = 0.0, t = 0.0, q = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { mu += part[0][w][lane]; t += part[1][w][lane]; q += part[2][w][lane]; }
    double var = NAN, pr = NAN, sc = mu;   // mean only (no slab): nothing but mu is formed
    if (slab) {
      var = prior[c] + t + q;
      const double sd = sqrt(fmax(var, 0.0)), dm = mu - threshold;
      // sd = 0 (no variance): the sign of mu - threshold decides, a tie is 1/2
      pr = norm_cdf(sd > 0.0 ? dm / sd : (dm > 0.0 ? INFINITY : (dm < 0.0 ? -INFINITY : 0.0)));
      if (mu != mu) { var = mu; pr = mu; }
      if (kind == PPBO_FUNCTIONAL_VARIANCE) sc = var;
      else if (kind == PPBO_FUNCTIONAL_PROB) sc = pr;
    }
    if (mu_out) mu_out[c] = mu;
    if (var_out) var_out[c] = var;
    if (prob_out) prob_out[c] = pr;
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  if (!blk_best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (lane == 0) blk_best[blockIdx.x] = b;
}

// ---- main effects and interactions (ppbo_predict_marginals) -----------------------------------------------------------
// The axis table a call leaves in the ctx (marginal_table_kernel, predict.hip): five rows of MG_AXES doubles per axis d
//   MG_COEF  the exponent's coefficient: 1 / (2 l^2) on an SE axis, 2 / l^2 on a periodic one
//   MG_PER   1.0 on a periodic axis, else 0.0
//   MG_I0    e^-a I0(a), a = 1 / l^2: the integral of a periodic factor over [0, 1], whatever its centre
//   MG_L     l
//   MG_A     A_d, the factor integrated over both of its arguments
// followed by 1 / Q[N, Dc] and P[N] of the design rows.
constexpr int MG_AXES = 64;
enum { MG_COEF = 0, MG_PER = MG_AXES, MG_I0 = 2 * MG_AXES, MG_L = 3 * MG_AXES, MG_A = 4 * MG_AXES, MG_ROWS = 5 * MG_AXES };

// I_d(c) = int_0^1 kappa_d(u - c) du of an SE axis: l sqrt(pi / 2) (erf((1 - c) / (sqrt2 l)) + erf(c / (sqrt2 l)))
__device__ __forceinline__ double marginal_se_integral(double c, double l) {
  const double il = 0.70710678118654752440 / l;
  return (1.25331413731550025121 * l) * (erf((1.0 - c) * il) + erf(c * il));
}

// One row of the call in canonical form: its kept axes in ASCENDING order with their values (lo < hi, or hi = -1, or
// both -1), so that (d, e, t, u) and (e, d, u, t) are the same row to every kernel.  ok = false: a row that breaks the
// rules of the entry (an axis outside -1 .. Dc - 1, the same axis twice, a first axis of -1 with a second one, an
// interaction of order below 2).  The entry refuses such a call before anything is launched; where it cannot look (a
// stream that is being captured) the row gets NaN results.
struct MargRow {
  int lo, hi;
  double tlo, thi;
  bool ok;
};
__device__ __forceinline__ MargRow marginal_row(const int* __restrict__ dims, const double* __restrict__ T, long long c,
                                                int Dc, int effect) {
  MargRow r;
  r.lo = dims[2 * c]; r.hi = dims[2 * c + 1];
  r.tlo = T ? T[2 * c] : 0.0; r.thi = T ? T[2 * c + 1] : 0.0;
  r.ok = r.lo >= -1 && r.lo < Dc && r.hi >= -1 && r.hi < Dc && (r.lo >= 0 || r.hi < 0) && (r.lo != r.hi || r.lo < 0) &&
         (effect != PPBO_EFFECT_INTERACTION || r.hi >= 0);
  if (r.hi >= 0 && r.hi < r.lo) {
    const int d = r.lo; r.lo = r.hi; r.hi = d;
    const double t = r.tlo; r.tlo = r.thi; r.thi = t;
  }
  return r;
}

// The first row of d_dims that breaks the rules, as a Best record per workgroup (value 1, the row's index; idx = -1:
// none), merged by argmax_final_kernel into the host-mapped record: equal values, so the smallest index wins.
__global__ __launch_bounds__(256) void marginal_check_kernel(const int* __restrict__ dims, long long M, int Dc, int effect,
                                                             Best* __restrict__ blk_best) {
  __shared__ Best sh[4];
  Best b{0.0, -1};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256)
    if (b.idx < 0 && !marginal_row(dims, nullptr, i, Dc, effect).ok) b = Best{1.0, i};
  b = block_best(b, sh);
  if (threadIdx.x == 0) blk_best[blockIdx.x] = b;
}

// Pass 3 of ppbo_predict_marginals: slope_score_kernel's geometry and slab sums for the column of a main effect or an
// interaction, then
//   mu = sum of the mean partials,   var = prior + c' Lambda c + |G c|^2,   p = P(L f > 0) = Phi(mu / sqrt(max(var, 0)))
// With S = sf2 prod_{d not kept} A_d (the host's product over ALL axes divided by the kept A_d), a_d = I_d(t_d) (erf at t_d
// on an SE axis, the table's constant on a periodic one) and b_d = 1 - 2 a_d + A_d:
//   RAW S;   CENTRED S (1 - 2 prod a_d + prod A_d);   INTERACTION S b_d b_e          (products over the kept axes)
// An order-0 row under CENTRED: 1 - 2 + 1 = 0 exactly, and its column is zero, so (0, 0, 1/2).  No noise term.  var = 0: the
// sign of mu decides, mu = 0 gives 1/2; a NaN mean (a non-finite t on a kept axis) gives NaN everywhere.
__global__ __launch_bounds__(SC_THREADS) void marginal_score_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                    const double* __restrict__ t_part,
                                                                    const double* __restrict__ slab, int n_slab, int M,
                                                                    const int* __restrict__ dims,
                                                                    const double* __restrict__ T,
                                                                    const double* __restrict__ tab, int Dc, double sf2,
                                                                    double prod_A, int effect, int kind, long long idx_base,
                                                                    double* __restrict__ mu_out, double* __restrict__ var_out,
                                                                    double* __restrict__ prob_out,
                                                                    double* __restrict__ score_out, Best* __restrict__ blk_best) {
  __shared__ double part[3][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SC_CAND + lane;
  double pm = 0.0, pt = 0.0, pq = 0.0;
  if (c < M) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    if (slab) {
      for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
      for (int s = wave; s < n_slab; s += SC_WAVES) pq += slab[(size_t)s * M + c];
    }
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pq;
  __syncthreads();
  if (wave != 0) return;                 // the rest is one wavefront's work
  Best b{0.0, -1};
  if (c < M) {
    double mu = 0.0, t = 0.0, q = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { mu += part[0][w][lane]; t += part[1][w][lane]; q += part[2][w][lane]; }
    double var = NAN, pr = NAN, sc = mu;   // mean only (no slab): nothing but mu is formed
    if (slab) {
      const MargRow row = marginal_row(dims, T, c, Dc, effect);
      double S = sf2 * prod_A, pa = 1.0, pA = 1.0, bb = 1.0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int d = k ? row.hi : row.lo;
        if (!row.ok || d < 0) continue;
        const double A = tab[MG_A + d];
        const double a = tab[MG_PER + d] != 0.0 ? tab[MG_I0 + d] : marginal_se_integral(k ? row.thi : row.tlo, tab[MG_L + d]);
        S /= A;
        pa *= a;
        pA *= A;
        bb *= (1.0 - 2.0 * a) + A;
      }
      const double prior = effect == PPBO_EFFECT_RAW ? S : (effect == PPBO_EFFECT_CENTRED ? S * ((1.0 - 2.0 * pa) + pA) : S * bb);
      var = prior + t + q;
      const double sd = sqrt(fmax(var, 0.0));
      // sd = 0 (no variance): the sign of mu decides, a tie is 1/2
      pr = norm_cdf(sd > 0.0 ? mu / sd : (mu > 0.0 ? INFINITY : (mu < 0.0 ? -INFINITY : 0.0)));
      if (mu != mu) { var = mu; pr = mu; }
      if (kind == PPBO_PAIR_VARIANCE) sc = var;
      else if (kind == PPBO_PAIR_PROB) sc = pr;
    }
    if (mu_out) mu_out[c] = mu;
    if (var_out) var_out[c] = var;
    if (prob_out) prob_out[c] = pr;
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  if (!blk_best) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (lane == 0) blk_best[blockIdx.x] = b;
}

// per-block records of one launch -> *out; with `record` also the 16-byte (value, GLOBAL index as a double: exact
// below 2^53; index + record_offset; (NaN, -1) when nothing scored) record that the sharded search all-gathers, and
// with `publish` the flag publish[0] raised to `epoch` AFTER the record with system-scope release semantics (the
// record may live in host-mapped memory: the host polls the flag instead of waiting for a copy and a stream
// synchronisation)
__global__ __launch_bounds__(256) void argmax_final_kernel(const Best* __restrict__ blk_best, int n,
                                                           Best* __restrict__ out, double* __restrict__ record = nullptr,
                                                           long long record_offset = 0,
                                                           unsigned long long* __restrict__ publish = nullptr,
                                                           unsigned long long epoch = 0) {
  __shared__ Best sh[4];
  Best b{0.0, -1};
  for (int i = threadIdx.x; i < n; i += blockDim.x) b = best_merge(b, blk_best[i]);
  b = block_best(b, sh);
  if (threadIdx.x == 0) {
    if (out) *out = b;
    if (record) {
      record[0] = b.idx < 0 ? NAN : b.val;
      record[1] = b.idx < 0 ? -1.0 : (double)(b.idx + record_offset);
    }
    if (publish) __hip_atomic_store(publish, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// per-chunk bests -> the 16-byte (value, global index as a double) record of a sharded search; one wavefront
__global__ __launch_bounds__(64) void best_record_kernel(const Best* __restrict__ chunk_best, int n, long long offset,
                                                         double* __restrict__ record,
                                                         unsigned long long* __restrict__ publish = nullptr,
                                                         unsigned long long epoch = 0) {
  Best b{0.0, -1};
  for (int i = threadIdx.x; i < n; i += 64) b = best_merge(b, chunk_best[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best other;
    other.val = __shfl_xor(b.val, o, 64);
    other.idx = __shfl_xor(b.idx, o, 64);
    b = best_merge(b, other);
  }
  if (threadIdx.x == 0) {
    record[0] = b.idx < 0 ? NAN : b.val;
    record[1] = b.idx < 0 ? -1.0 : (double)(b.idx + offset);
    if (publish) __hip_atomic_store(publish, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}


// host: reduce per-chunk bests (device) to one (value, index); synchronises the stream
inline int merge_chunk_bests(ppbo_ctx* ctx, const Best* d_chunk_best, int n_chunks, double* h_best_val,
                             int64_t* h_best_idx, hipStream_t s) {
  if (!h_best_val && !h_best_idx) return 0;
  Best* hb = (Best*)ppbo_pinned(ctx, (size_t)n_chunks * sizeof(Best));
  if (!hb) return ppbo_set_error(ctx, (int)hipErrorOutOfMemory, "pinned staging");
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(hb, d_chunk_best, (size_t)n_chunks * sizeof(Best), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  double bv = 0.0;
  long long bi = -1;
  for (int ch = 0; ch < n_chunks; ++ch) {
    if (hb[ch].idx < 0) continue;
    if (bi < 0 || hb[ch].val > bv || (hb[ch].val == bv && hb[ch].idx < bi)) { bv = hb[ch].val; bi = hb[ch].idx; }
  }
  if (h_best_val) *h_best_val = bv;
  if (h_best_idx) *h_best_idx = (int64_t)bi;
  return 0;
}

}  // namespace
