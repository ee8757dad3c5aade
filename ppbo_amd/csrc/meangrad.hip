// f-2: posterior mean and its analytic gradient at M points, the device half of the batched multi-start
// refinement that replaces mu_star's differential evolution (gp_model.py:415-437).
//   mu(x) = sum_i alpha_i k(x, x_i),   d mu / d x_d = sum_i alpha_i dk/dx_d
//   SE      dk/dx_d = -(x_d - x_i,d) / l^2 * k                               (kernels.py:19-25)
//   RQ      dk/dx_d = -(x_d - x_i,d) / l^2 * k / (1 + r^2 / (4 l^2))         (kernels.py:27-34, alpha = 2)
//   camphor dk/dx_d = -(2 pi / l^2) sin(2 pi (x_d - x_i,d)) * k  (d != 2),   -(x_2 - x_i,2) / (l + 0.05)^2 * k
//                                                                            (kernels.py:36-53)
//   Matern  dk/dx_d = -(x_d - x_i,d) sf^2 (c^2 / 3) (1 + a) e^-a  (5/2),  -(x_d - x_i,d) sf^2 c^2 e^-a  (3/2),  a = c r
//                                                                            (common.h matern_grad; finite at r = 0)
// One 256-thread workgroup per point: lanes stride over the N design rows with the point held in
// registers, accumulate mu and D gradient components, then a shuffle + LDS reduction.  M is small here
// (a few hundred ascent iterates), so the work per launch is M * N * D * ~6 flops -- microseconds.
#include "common.h"
#include "camphor.h"
#include "rffmath.h"

namespace {

template <int KID, int DP>
__global__ __launch_bounds__(256) void mean_grad_kernel(const double* __restrict__ X, int N, int D, KernParams p,
                                                        const double* __restrict__ alpha,
                                                        const double* __restrict__ Xc, double* __restrict__ mu,
                                                        double* __restrict__ grad) {
  __shared__ double red[4][DP + 1];
  const int c = blockIdx.x;
  double xc[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    xc[d] = (d < D) ? Xc[(size_t)c * D + d] : 0.0;
    g[d] = 0.0;
  }
  double m = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    const double* __restrict__ xi = X + (size_t)i * D;
    double dx[DP], s = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      dx[d] = (d < D) ? xc[d] - xi[d] : 0.0;
      s += kern_term<KID>(dx[d], d, p);
    }
    double w, coef;
    if constexpr (kid_matern<KID>) {     // one exponential for the value and the gradient
      const MaternAE ae = matern_ae<KID>(s, p);
      w = alpha[i] * matern_value<KID>(ae, p.sf2);
      coef = alpha[i] * matern_grad<KID>(ae, p);
    } else {
      w = alpha[i] * kern_finish<KID>(s, p);
    }
    m += w;
    if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        if (d == 2) g[d] -= 2.0 * p.c1 * dx[d] * w;
        else if (d < 6) g[d] -= p.c0 * 3.14159265358979323846 * sinpi(2.0 * dx[d]) * w;
      }
    } else {
      if constexpr (!kid_matern<KID>) coef = kern_grad_coef<KID>(s, w, p);
#pragma unroll
      for (int d = 0; d < DP; ++d) g[d] += coef * dx[d];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  m = wave_sum(m);
#pragma unroll
  for (int d = 0; d < DP; ++d) g[d] = wave_sum(g[d]);
  if (lane == 0) {
    red[wave][DP] = m;
#pragma unroll
    for (int d = 0; d < DP; ++d) red[wave][d] = g[d];
  }
  __syncthreads();
  if (threadIdx.x <= DP) {
    const int d = threadIdx.x;
    const double v = (red[0][d] + red[1][d]) + (red[2][d] + red[3][d]);
    if (d == DP) mu[c] = v;
    else if (d < D) grad[(size_t)c * D + d] = v;
  }
}

// ---------------------------------------------------------------------------------------------------
// Device-resident maximiser of the posterior mean (ppbo_mean_search): what mu_star's differential evolution
// (gp_model.py:415-437) is replaced by, without a host round trip per iterate.
//   1. group_max_kernel: the M scored candidates are cut into T <= 4096 groups of consecutive rows (T such that the
//      survivors and their coordinates fit one workgroup's LDS: 2633 at D = 6, 877 at D = 20); each group's best row
//      survives (the candidates are i.i.d. uniform, so this is a thinning, not a loss of coverage; the best candidate
//      always survives).
//   2. select_starts_kernel (one workgroup): greedy choice of the K best survivors that are pairwise more than
//      `sep` apart -- argmax, then strike everything within sep of the winner -- the rule the host loop applied.
//   3. mean_ascent_kernel: one workgroup per start runs the WHOLE projected Barzilai-Borwein ascent: evaluations
//      of mu and its gradient by all 256 threads (as mean_grad_kernel), the D-vector bookkeeping by wavefront 0 with
//      lane = coordinate (D <= 64), monotone safeguard, per-start stopping rule.

// The candidates of the trials of ONE mu_star call (ppbo_mean_search_multi), never materialised: trial t sees the
// resident uniform pool through its own rotation frac(pool + shift_t) (what ppbo_shift_points writes out for the
// one-trial entry: the same expression, the same bits), and trial 0 also the E extra points (the design, the previous
// x*).  Every trial has Mt = M + E slots; slots >= M of the later trials are absent (score -inf).
struct TrialCands {
  const double* pool = nullptr; long long M = 0; const double* shifts = nullptr;
  const double* extra = nullptr;   // E_rows rows (the design points: the model's own X, or caller-given points) ...
  const double* xprev = nullptr;   // ... followed by one more point (the previous x*) when given
  int E_rows = 0, E = 0, D = 0;    // E = E_rows + (xprev ? 1 : 0)
};
__device__ __forceinline__ double trial_coord(const TrialCands& c, int trial, long long i, int d) {
  if (i < c.M) { const double v = c.pool[(size_t)i * c.D + d] + c.shifts[(size_t)trial * c.D + d]; return v - floor(v); }
  const long long e = i - c.M;
  return e < c.E_rows ? c.extra[(size_t)e * c.D + d] : c.xprev[d];
}

// Screening pass of a mu_star trial: the posterior mean of every candidate, good enough to RANK them (the starts of the
// ascents are picked from it; every value that is reported comes from the fp64 ascent).  Kernel values in fp32 from
// direct differences -- v_exp_f32 instead of an 18-instruction fp64 exponential, fp32 FMAs at twice the fp64 rate --
// accumulated in fp64 (alpha has both signs and |mu| << sum |alpha_i k_i|).  Relative error of mu ~1e-6: two candidates
// closer than that may swap ranks.  grid (candidate blocks, row splits, trials); part[trial][split][Mt].
constexpr int SCR_T = 256, SCR_CPT = 4, SCR_RJ = 64;
// the DP buckets of mean_screen_kernel and box_screen_kernel (camphor-copper, D = 6: a bucket of its own)
using ScreenLadder = DpLadder<4, 8, 12, 16, 20, 24, 32, 48, 64>;
typedef float float2_t __attribute__((ext_vector_type(2)));
// two candidates per packed operation (v_pk_add_f32 / v_pk_fma_f32: both halves at the price of one fp32 instruction)
template <int KID>
__device__ __forceinline__ float2_t screen_term2(float2_t dx, int d, float c0, float c1) {
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    if (d == 2) return c1 * dx * dx;
    float2_t sn;
    sn.x = sinpif(fabsf(dx.x)); sn.y = sinpif(fabsf(dx.y));
    return c0 * sn * sn;
  } else {
    static_assert(kid_radial<KID>, "unknown kernel id");
    return dx * dx;
  }
}
template <int KID>
__device__ __forceinline__ float screen_finish(float s, float sf2, float c0) {
  if constexpr (KID == PPBO_KERNEL_RQ) {
    const float t = 1.0f + s * c0; return sf2 * __builtin_amdgcn_rcpf(t * t);
  } else if constexpr (KID == PPBO_KERNEL_SE || KID == PPBO_KERNEL_CAMPHOR) {
    const float e = (KID == PPBO_KERNEL_SE) ? -c0 * s : -s;
    return sf2 * __builtin_amdgcn_exp2f(fmaxf(e * 1.44269504088896340736f, -126.0f));
  } else {
    // Matern: a = c r from v_sqrt_f32 (s >= 0: a sum of squares), e^-a by v_exp_f32 as above
    static_assert(kid_matern<KID>, "unknown kernel id");
    const float a = c0 * __builtin_amdgcn_sqrtf(s);
    const float e = __builtin_amdgcn_exp2f(fmaxf(-a * 1.44269504088896340736f, -126.0f));
    const float poly = (KID == PPBO_KERNEL_MATERN52) ? fmaf(a, fmaf(a, 1.0f / 3.0f, 1.0f), 1.0f) : 1.0f + a;
    return sf2 * (poly * e);
  }
}
template <int KID, int DP>
__global__ __launch_bounds__(SCR_T) void mean_screen_kernel(const double* __restrict__ X, int N, int D, KernParams p,
                                                            const double* __restrict__ alpha, TrialCands tc,
                                                            int rows_per_split, int n_split, double* __restrict__ part,
                                                            int extra_trial) {
  static_assert(SCR_CPT % 2 == 0, "candidates in packed pairs");
  constexpr int NP = SCR_CPT / 2;
  __shared__ __attribute__((aligned(16))) float xs[SCR_RJ][DP];
  __shared__ double sa[SCR_RJ];
  const int trial = blockIdx.z;
  const long long Mt = tc.M + tc.E;
  const long long c0 = ((long long)blockIdx.x * SCR_T + threadIdx.x) * SCR_CPT;
  float2_t xc[NP][DP];
  double mu[SCR_CPT];
#pragma unroll
  for (int q = 0; q < SCR_CPT; ++q) {
    mu[q] = 0.0;
    const bool there = c0 + q < tc.M || (trial == extra_trial && c0 + q < Mt);   // (the launch's trial that carries the extra points)
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const float v = (d < D && there) ? (float)trial_coord(tc, trial, c0 + q, d) : 0.0f;
      if (q & 1) xc[q >> 1][d].y = v; else xc[q >> 1][d].x = v;
    }
  }
  const float c0f = (float)p.c0, c1f = (float)p.c1, sf2f = (float)p.sf2;
  const int j_beg = blockIdx.y * rows_per_split;
  int j_end = j_beg + rows_per_split;
  if (j_end > N) j_end = N;
  for (int row0 = j_beg; row0 < j_end; row0 += SCR_RJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < SCR_RJ * DP; e += SCR_T) {
      const int r = e / DP, d = e - r * DP, j = row0 + r;
      xs[r][d] = (j < j_end && d < D) ? (float)X[(size_t)j * D + d] : 0.0f;
    }
    if (threadIdx.x < SCR_RJ) sa[threadIdx.x] = (row0 + (int)threadIdx.x < j_end) ? alpha[row0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int rmax = (j_end - row0 < SCR_RJ) ? (j_end - row0) : SCR_RJ;
    for (int r = 0; r < rmax; ++r) {
      float2_t sv[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) sv[q] = float2_t{0.0f, 0.0f};
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const float x = xs[r][d];
        const float2_t xx = {x, x};
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          if (KID == PPBO_KERNEL_CAMPHOR) sv[q] += screen_term2<KID>(xx - xc[q][d], d, c0f, c1f);
          else { const float2_t dx = xx - xc[q][d]; sv[q] = __builtin_elementwise_fma(dx, dx, sv[q]); }
        }
      }
      const double a = sa[r];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        mu[2 * q] = fma(a, (double)screen_finish<KID>(sv[q].x, sf2f, c0f), mu[2 * q]);
        mu[2 * q + 1] = fma(a, (double)screen_finish<KID>(sv[q].y, sf2f, c0f), mu[2 * q + 1]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < SCR_CPT; ++q)
    if (c0 + q < Mt) part[((size_t)trial * n_split + blockIdx.y) * Mt + c0 + q] = mu[q];
}

// mu[trial][c] = sum over the row splits (fixed order); absent slots -inf
__global__ __launch_bounds__(256) void screen_sum_kernel(const double* __restrict__ part, int n_split, long long Mt,
                                                         long long M, int extra_trial, double* __restrict__ mu) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  const int trial = blockIdx.y;
  if (c >= Mt) return;
  double s = 0.0;
  if (c >= M && trial != extra_trial) s = -INFINITY;
  else
    for (int k = 0; k < n_split; ++k) s += part[((size_t)trial * n_split + k) * Mt + c];
  mu[(size_t)trial * Mt + c] = s;
}

__global__ __launch_bounds__(256) void fill_kernel(double* __restrict__ p, long long n, double v) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// candidates of trial t as rows (the fp64 screening path scores them with ppbo_predict)
__global__ __launch_bounds__(256) void trial_rows_kernel(TrialCands tc, int trial, double* __restrict__ out) {
  const long long n = (tc.M + (trial == 0 ? tc.E : 0)) * tc.D;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  out[e] = trial_coord(tc, trial, e / tc.D, (int)(e % tc.D));
}

// blockIdx.y = trial: mu, gval, gidx are per-trial arrays of M (resp. T) entries
__global__ __launch_bounds__(256) void group_max_kernel(const double* __restrict__ mu, int64_t M, int G, int T,
                                                        double* __restrict__ gval, int* __restrict__ gidx) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  mu += (size_t)blockIdx.y * M; gval += (size_t)blockIdx.y * T; gidx += (size_t)blockIdx.y * T;
  const int64_t lo = (int64_t)t * G, hi = (lo + G < M) ? lo + G : M;
  double best = -INFINITY;
  int64_t bi = lo;
  for (int64_t i = lo; i < hi; ++i) {
    const double v = mu[i];
    if (v > best) { best = v; bi = i; }         // NaN never wins
  }
  gval[t] = best;
  gidx[t] = (int)bi;
}

// (score, index) argmax over a wavefront by DPP (no LDS crossbar): larger score wins, ties go to the smaller index.
struct SelRec { double v; int i; };
__device__ __forceinline__ SelRec sel_merge(SelRec a, SelRec b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
template <int CTRL>
__device__ __forceinline__ SelRec sel_dpp_step(SelRec a) {
  SelRec o;
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(a.v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(a.v), CTRL, 0xF, 0xF, true);
  o.i = __builtin_amdgcn_mov_dpp(a.i, CTRL, 0xF, 0xF, true);
  o.v = __hiloint2double(hi, lo);
  return sel_merge(a, o);
}
__device__ __forceinline__ SelRec wave_sel(SelRec a) {
  a = sel_dpp_step<0xB1>(a);
  a = sel_dpp_step<0x4E>(a);
  a = sel_dpp_step<0x141>(a);
  a = sel_dpp_step<0x140>(a);
  SelRec r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r[k].v = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(a.v), 16 * k),
                              __builtin_amdgcn_readlane(__double2loint(a.v), 16 * k));
    r[k].i = __builtin_amdgcn_readlane(a.i, 16 * k);
  }
  return sel_merge(sel_merge(r[0], r[1]), sel_merge(r[2], r[3]));
}

// One workgroup.  The T survivors' scores AND coordinates live in LDS (the host sizes T for it): a pick is an argmax
// (DPP per wavefront, every wavefront merges the 16 wave records itself) and a strike pass over LDS -- no global
// round trip inside the K-step loop (the first form re-read gidx and the coordinates from memory in every step:
// 13 us per pick, 0.44 of the 0.68 ms of a mu_star trial).
// blockIdx.x = trial (ppbo_mean_search_multi; the one-trial entries launch one workgroup): every per-trial array is
// offset by it, and with tc.pool the candidate coordinates are formed on the fly (TrialCands) instead of read from `cand`.
__global__ __launch_bounds__(1024) void select_starts_kernel(const double* __restrict__ gval,
                                                             const int* __restrict__ gidx, int T,
                                                             const double* __restrict__ cand, int D, int K, double sep2,
                                                             double* __restrict__ starts, int* __restrict__ count,
                                                             TrialCands tc) {
  extern __shared__ double sv[];          // [T] survivor scores (struck: -inf) | [T][D] coordinates | 16 wave records
  double* xc = sv + T;
  __shared__ double wv[16];
  __shared__ int wi[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int trial = blockIdx.x;
  gval += (size_t)trial * T; gidx += (size_t)trial * T; starts += (size_t)trial * K * D; count += trial;
  for (int t = tid; t < T; t += 1024) sv[t] = gval[t];
  for (int e = tid; e < T * D; e += 1024) {
    const int t = e / D, d = e - t * D;
    xc[e] = tc.pool ? trial_coord(tc, trial, gidx[t], d) : cand[(size_t)gidx[t] * D + d];
  }
  __syncthreads();
  int k = 0;
  for (; k < K; ++k) {
    SelRec best{-INFINITY, 0x7fffffff};
    for (int t = tid; t < T; t += 1024) {
      const double v = sv[t];
      if (v > best.v) { best.v = v; best.i = t; }       // ascending t per thread: first index wins
    }
    best = wave_sel(best);
    if (lane == 0) { wv[wave] = best.v; wi[wave] = best.i; }
    __syncthreads();
    SelRec mine{-INFINITY, 0x7fffffff};
    if (lane < 16) { mine.v = wv[lane]; mine.i = wi[lane]; }
    const SelRec top = wave_sel(mine);                  // the same in every wavefront
    if (!(top.v > -INFINITY)) break;
    const int w = top.i;
    const double* pw = xc + (size_t)w * D;
    if (tid < D) starts[(size_t)k * D + tid] = pw[tid];
    for (int t = tid; t < T; t += 1024) {
      if (!(sv[t] > -INFINITY)) continue;
      const double* pt = xc + (size_t)t * D;
      double d2 = 0.0;
      for (int d = 0; d < D; ++d) { const double dx = pt[d] - pw[d]; d2 += dx * dx; }
      if (d2 <= sep2) sv[t] = -INFINITY;        // strikes the winner itself too
    }
    __syncthreads();                             // sv and the wave records are rewritten by the next pick
  }
  if (tid == 0) *count = k;
}

// survivors of the thinning: as many as fit one workgroup's LDS next to their coordinates (<= 4096)
static inline int select_capacity(int D) {
  const int cap = (144 * 1024) / (8 + 8 * D);
  return cap > 4096 ? 4096 : (cap < 64 ? 64 : cap);
}

// The start selection of every search: B score vectors (trials, samples) of Mt candidates each, cut into Tg groups of G
// consecutive rows (Tg <= select_capacity), reduced to K starts per vector.  alloc() lays out WS_SEARCH as
//   head[n_head] | scores[B][Mt] | gval[B][Tg] | starts[B][K][D] | gidx[B][Tg] (int) | counts (int)
// with room for n_counts ints beyond 16 of slack; the caller scores into `scores`, then select() runs.
struct StartSelection {
  long long Mt; int B, D, K;
  int G = 0, Tg = 0;
  double *head = nullptr, *scores = nullptr, *gval = nullptr, *starts = nullptr;
  int *gidx = nullptr, *counts = nullptr;
  bool alloc(ppbo_ctx* ctx, size_t n_head, size_t n_counts) {
    const int T_MAX = select_capacity(D);
    G = (int)((Mt + T_MAX - 1) / T_MAX);
    Tg = (int)((Mt + G - 1) / G);
    const size_t nd = n_head + (size_t)B * Mt + (size_t)B * Tg + (size_t)B * K * D;
    head = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SEARCH, nd * sizeof(double) + ((size_t)B * Tg + n_counts + 16) * sizeof(int));
    if (!head) return false;
    scores = head + n_head;
    gval = scores + (size_t)B * Mt;
    starts = gval + (size_t)B * Tg;
    gidx = (int*)(starts + (size_t)B * K * D);
    counts = gidx + (size_t)B * Tg;
    return true;
  }
  // each group's best row survives (group_max_kernel); one workgroup per vector picks its starts, pairwise more than
  // sep apart, among the survivors held in LDS (select_starts_kernel) and writes their number to out_counts[b].  The
  // coordinates come from cand (rows) or tc (tc.pool set).
  void select(ppbo_ctx* ctx, double sep, const double* cand, const TrialCands& tc, int* out_counts, hipStream_t s) const {
    group_max_kernel<<<dim3((Tg + 255) / 256, B), 256, 0, s>>>(scores, Mt, G, Tg, gval, gidx);
    const size_t sel_lds = (size_t)Tg * (1 + D) * sizeof(double);
    if (sel_lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)select_starts_kernel, 150 * 1024);
    select_starts_kernel<<<B, 1024, sel_lds, s>>>(gval, gidx, Tg, cand, D, K, sep * sep, starts, out_counts, tc);
  }
};

// mu and its gradient at the point held in LDS (sx), partial sums of this thread's rows reduced into red[wave][.]
// TR: X is given TRANSPOSED ([D][N]): the threads of a wavefront then read consecutive addresses per coordinate.  With
// row-major X every lane reads its own row (a 8 D-byte segment each, 64 cache lines per load instruction) and the
// ascent is bound by the L1's transaction rate, not by arithmetic or latency.
template <int KID, int DP, int NT = 256, bool TR = false>
__device__ __forceinline__ void eval_mean_grad(const double* __restrict__ X, int N, int D, const KernParams& p,
                                               const double* __restrict__ alpha, const double* sx,
                                               double (*red)[DP + 1]) {
  double xc[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) { xc[d] = sx[d]; g[d] = 0.0; }
  double m = 0.0;
  for (int i = threadIdx.x; i < N; i += NT) {
    const double* __restrict__ xi = TR ? X + i : X + (size_t)i * D;
    const size_t xs = TR ? (size_t)N : 1;
    double dx[DP], s = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      dx[d] = (d < D) ? xc[d] - xi[d * xs] : 0.0;
      s += kern_term<KID>(dx[d], d, p);
    }
    double w, coef;
    if constexpr (kid_matern<KID>) {     // one exponential for the value and the gradient
      const MaternAE ae = matern_ae<KID>(s, p);
      w = alpha[i] * matern_value<KID>(ae, p.sf2);
      coef = alpha[i] * matern_grad<KID>(ae, p);
    } else {
      w = alpha[i] * kern_finish<KID>(s, p);
    }
    m += w;
    if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        if (d == 2) g[d] -= 2.0 * p.c1 * dx[d] * w;
        else if (d < 6) g[d] -= p.c0 * 3.14159265358979323846 * sinpi(2.0 * dx[d]) * w;
      }
    } else {
      if constexpr (!kid_matern<KID>) coef = kern_grad_coef<KID>(s, w, p);
#pragma unroll
      for (int d = 0; d < DP; ++d) g[d] += coef * dx[d];
    }
  }
  // DPP sums over rows of 16 lanes (DP + 1 reductions through ds_bpermute would queue on the LDS pipe, and finishing
  // each of them across the four rows costs eight v_readlane more): one record per row, 4 per wavefront
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  m = row16_sum_dpp(m);
#pragma unroll
  for (int d = 0; d < DP; ++d) g[d] = row16_sum_dpp(g[d]);
  if ((lane & 15) == 0) {
    double* r = red[4 * wave + (lane >> 4)];
    r[DP] = m;
#pragma unroll
    for (int d = 0; d < DP; ++d) r[d] = g[d];
  }
}

// the objective of an ascent: fills red[wave][0..DP) with the gradient's and red[wave][DP] with the value's partial sums
template <int KID, int DP, int NT>
struct MeanEval {
  const double* X; int N, D; KernParams p; const double* alpha;
  __device__ __forceinline__ void operator()(const double* sx, double (*red)[DP + 1]) const {
    eval_mean_grad<KID, DP, NT, true>(X, N, D, p, alpha, sx, red);       // X: the transposed design [D][N]
  }
};

// ARD (PPBO_COORDS_SCALED): the ascent runs in the caller's coordinates x over the model's scaled rows -- mu at
// s (.) x, d mu / d x_d = s_d d mu / d x~_d.  The scaled point goes through LDS of its own (one barrier); the gradient's
// partial sums are scaled by the threads that wrote them (eval_mean_grad: lane 16 k of each wavefront writes record
// 4 wave + k), so the barrier behind the evaluation in bb_ascent_kernel still orders them before they are read.
template <int KID, int DP, int NT>
struct ScaledMeanEval {
  MeanEval<KID, DP, NT> ev; const double* scale;   // scale: D values (device)
  __device__ __forceinline__ void operator()(const double* sx, double (*red)[DP + 1]) const {
    __shared__ double sxs[DP];
    if (threadIdx.x < DP) sxs[threadIdx.x] = ((int)threadIdx.x < ev.D) ? sx[threadIdx.x] * scale[threadIdx.x] : 0.0;
    __syncthreads();
    ev(sxs, red);
    const int lane = threadIdx.x & 63;
    if ((lane & 15) == 0) {
      double* r = red[4 * (threadIdx.x >> 6) + (lane >> 4)];
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < ev.D) r[d] *= scale[d];
    }
  }
};

// camphor-copper with one length scale per coordinate (PPBO_COORDS_CAMPHOR): mu and its gradient in the caller's
// coordinates over the design's caller-coordinate rows (X transposed, [6][N]) -- the camphor form of eval_mean_grad with
// a coefficient per coordinate, c.k[d] = 2 / l_d^2 (periodic) and 1 / (2 l_2^2) (z); the same reduction records.
template <int DP, int NT>
struct CamphorMeanEval {
  static_assert(DP >= CAMPHOR_D, "six coordinates");
  const double* X; int N; double sf2; CamphorCoef c; const double* alpha;
  __device__ __forceinline__ void operator()(const double* sx, double (*red)[DP + 1]) const {
    double xc[CAMPHOR_D], g[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) g[d] = 0.0;
#pragma unroll
    for (int d = 0; d < CAMPHOR_D; ++d) xc[d] = sx[d];
    double m = 0.0;
    for (int i = threadIdx.x; i < N; i += NT) {
      double dx[CAMPHOR_D], s = 0.0;
#pragma unroll
      for (int d = 0; d < CAMPHOR_D; ++d) {
        dx[d] = xc[d] - X[(size_t)d * N + i];
        if (d == 2) s += c.k[2] * dx[d] * dx[d];
        else { const double sn = sinpi(fabs(dx[d])); s += c.k[d] * sn * sn; }
      }
      const double w = alpha[i] * (sf2 * exp_nonpos(-s));
      m += w;
#pragma unroll
      for (int d = 0; d < CAMPHOR_D; ++d) {
        if (d == 2) g[d] -= 2.0 * c.k[2] * dx[d] * w;
        else g[d] -= c.k[d] * 3.14159265358979323846 * sinpi(2.0 * dx[d]) * w;
      }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = row16_sum_dpp(m);
#pragma unroll
    for (int d = 0; d < DP; ++d) g[d] = row16_sum_dpp(g[d]);
    if ((lane & 15) == 0) {
      double* r = red[4 * wave + (lane >> 4)];
      r[DP] = m;
#pragma unroll
      for (int d = 0; d < DP; ++d) r[d] = g[d];
    }
  }
};

// the per-feature body of a posterior sample in weight space, shared by RffEval and CamphorRffEval (a macro, so that
// RffEval compiles to the instruction stream it had as a loop body of its own): with W (the transposed basis [D][F]),
// F, D, b, omega, amp, P, the point xc[NC] and the accumulators m, g[NC] in scope, feature f's phase, its cosine into m
// and its sine times w_f into g
#define RFF_FEATURE_BODY(NC)                                                                                   \
  {                                                                                                            \
    const double* __restrict__ wf = W + f;                 /* coalesced per coordinate */                      \
    double wv[NC], ph = b[f];                                                                                  \
    _Pragma("unroll") for (int d = 0; d < NC; ++d) { wv[d] = (d < D) ? wf[(size_t)d * F] : 0.0; ph = fma(wv[d], xc[d], ph); } \
    /* cos and sin = cos(. - pi/2) by the branch-free polynomial of the RFF kernels (2 x 20 instructions against a  \
       library sincos with its own range reduction); phases beyond its range take the library path */          \
    double sn, cs;                                                                                             \
    if (fabs(ph) < 0.5 * RFF_COS_FAST_RANGE) {                                                                 \
      cs = rff_cos_fast(ph, P);                                                                                \
      sn = rff_cos_fast(ph - 1.57079632679489661923, P);                                                       \
    } else {                                                                                                   \
      sincos(ph, &sn, &cs);                                                                                    \
    }                                                                                                          \
    const double om = amp * omega[f];                                                                          \
    m = fma(om, cs, m);                                                                                        \
    const double c = -om * sn;                                                                                 \
    _Pragma("unroll") for (int d = 0; d < NC; ++d) g[d] = fma(c, wv[d], g[d]);                                 \
  }

// one posterior sample of the utility in weight space (random_fourier_sampler.py:45-53,166):
//   f(x) = a sum_f omega_f cos(w_f.x + b_f),   grad f = -a sum_f omega_f sin(w_f.x + b_f) w_f,   a = sqrt(2 sf^2 / F)
template <int DP, int NT>
struct RffEval {
  const double* W; int F, D; const double* b; const double* omega; double amp; RffPoly P;   // P: unit amplitude
  __device__ __forceinline__ void operator()(const double* sx, double (*red)[DP + 1]) const {
    double xc[DP], g[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) { xc[d] = sx[d]; g[d] = 0.0; }
    double m = 0.0;
    for (int f = threadIdx.x; f < F; f += NT) RFF_FEATURE_BODY(DP)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = row16_sum_dpp(m);
#pragma unroll
    for (int d = 0; d < DP; ++d) g[d] = row16_sum_dpp(g[d]);
    if ((lane & 15) == 0) {
      double* r = red[4 * wave + (lane >> 4)];
      r[DP] = m;
#pragma unroll
      for (int d = 0; d < DP; ++d) r[d] = g[d];
    }
  }
};

// one camphor-copper posterior sample in the caller's coordinates (ppbo_rff_search, PPBO_COORDS_CAMPHOR): the basis lives on the
// embedded point e(x) in R^11 (camphor.h), f(x) = a sum_f omega_f cos(w_f.e(x) + b_f).  The threads of wavefront 0
// form e(sx) once per evaluation in LDS (camphor_embed_one: the bits ppbo_camphor_embed writes), every thread runs
// RffEval's per-feature body (RFF_FEATURE_BODY) over its features at D = 11 and pulls its partial gradient back through de/dx before
// the same fixed-order reductions: d f / d x_d = 2 pi (c_d g_s - s_d g_c) for a periodic d, g_z / l_2 for z.
// The records are RffEval's at DP = 8 (six live coordinates).
template <int NT>
struct CamphorRffEval {
  static constexpr int DP = 8, DE = CAMPHOR_E;             // records of 8 columns; 11 embedded columns
  const double* W; int F; const double* b; const double* omega; double amp; RffPoly P;   // W: transposed [11][F]
  CamphorInvL L;
  __device__ __forceinline__ void operator()(const double* sx, double (*red)[DP + 1]) const {
    __shared__ double se[DE];
    if (threadIdx.x < CAMPHOR_D) camphor_embed_one(sx[threadIdx.x], (int)threadIdx.x, L, se);
    __syncthreads();
    constexpr int D = DE;
    double xc[DE], g[DE];                                    // the embedded point and the gradient in e
#pragma unroll
    for (int k = 0; k < DE; ++k) { xc[k] = se[k]; g[k] = 0.0; }
    double m = 0.0;
    for (int f = threadIdx.x; f < F; f += NT) RFF_FEATURE_BODY(DE)
    double gx[DP];                                           // ... pulled back to the caller's coordinates
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      if (d >= CAMPHOR_D) { gx[d] = 0.0; continue; }
      const int c = camphor_col(d);
      gx[d] = (d == 2) ? g[c] * L.v[2] : 6.28318530717958647693 * (xc[c] * g[c + 1] - xc[c + 1] * g[c]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = row16_sum_dpp(m);
#pragma unroll
    for (int d = 0; d < DP; ++d) gx[d] = row16_sum_dpp(gx[d]);
    if ((lane & 15) == 0) {
      double* r = red[4 * wave + (lane >> 4)];
      r[DP] = m;
#pragma unroll
      for (int d = 0; d < DP; ++d) r[d] = gx[d];
    }
  }
};

// the batched forms (ppbo_rff_search_multi): one launch runs S x K starts, workgroup s K + k on sample s, whose
// weights follow sample 0's at s F.  They ARE the single-sample evaluations (RffEval, CamphorRffEval) with omega moved
// to the workgroup's sample.
template <class EV>
struct RffSampleEval {
  EV ev; int per;                            // ev.omega: the [S, F] weights; per = K starts per sample
  template <class RED>
  __device__ __forceinline__ void operator()(const double* sx, RED red) const {
    EV e = ev;
    e.omega = ev.omega + (size_t)(blockIdx.x / per) * ev.F;
    e(sx, red);
  }
};

// one pathwise posterior sample (ppbo_path_search_multi): g(x) = a sum_f w_f cos(w_f.x + b_f) + sum_i v_i k(x, x_i) and its
// gradient -- RffEval's feature half (RFF_FEATURE_BODY) and the kernel half of eval_mean_grad (radial kernels, the design
// transposed [D][N]) with sample s's v_s for alpha, summed into ONE set of records: the design rows first, then the
// features, each thread's share in index order.  scale (ARD, D device values s_d, else NULL): the box and the basis live
// in the caller's coordinates x, the design holds the scaled rows, so the kernel half runs at s (.) x and its gradient
// is taken back (d / d x_d = s_d d / d x~_d) before the feature half joins it.  One workgroup = one start of sample
// blockIdx.x / per, whose weights follow sample 0's at s F (wp) and s N (v), as RffSampleEval moves omega.
template <int KID, int DP, int NT>
struct PathEval {
  static_assert(kid_radial<KID>, "radial kernels only");
  const double* W; int F, D; const double* b; const double* wp; double amp; RffPoly P;   // W: the transposed basis [D][F]
  const double* X; int N; KernParams p; const double* v; const double* scale; int per;
  __device__ __forceinline__ void operator()(const double* sx, double (*red)[DP + 1]) const {
    const int smp = blockIdx.x / per;
    double xc[DP], g[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) { xc[d] = (scale && d < D) ? sx[d] * scale[d] : sx[d]; g[d] = 0.0; }
    double m = 0.0;
    const double* __restrict__ alpha = v + (size_t)smp * N;
    for (int i = threadIdx.x; i < N; i += NT) {
      const double* __restrict__ xi = X + i;
      double dx[DP], s = 0.0;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        dx[d] = (d < D) ? xc[d] - xi[(size_t)d * N] : 0.0;
        s += dx[d] * dx[d];
      }
      double w, coef;
      if constexpr (kid_matern<KID>) {
        const MaternAE ae = matern_ae<KID>(s, p);
        w = alpha[i] * matern_value<KID>(ae, p.sf2);
        coef = alpha[i] * matern_grad<KID>(ae, p);
      } else {
        w = alpha[i] * kern_finish<KID>(s, p);
        coef = kern_grad_coef<KID>(s, w, p);
      }
      m += w;
#pragma unroll
      for (int d = 0; d < DP; ++d) g[d] += coef * dx[d];
    }
    if (scale) {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        if (d < D) g[d] *= scale[d];
        xc[d] = sx[d];
      }
    }
    const double* __restrict__ omega = wp + (size_t)smp * F;
    for (int f = threadIdx.x; f < F; f += NT) RFF_FEATURE_BODY(DP)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = row16_sum_dpp(m);
#pragma unroll
    for (int d = 0; d < DP; ++d) g[d] = row16_sum_dpp(g[d]);
    if ((lane & 15) == 0) {
      double* r = red[4 * wave + (lane >> 4)];
      r[DP] = m;
#pragma unroll
      for (int d = 0; d < DP; ++d) r[d] = g[d];
    }
  }
};

// fixed-order sum of the NW records of column c
template <int NW, int DP>
__device__ __forceinline__ double red_col(const double (*red)[DP + 1], int c) {
  double t = red[0][c];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w][c];
  return t;
}

template <int DP, class EVAL, int NT>
__global__ __launch_bounds__(NT) void bb_ascent_kernel(EVAL ev, int D, const double* __restrict__ starts,
                                                        const int* __restrict__ count, int iters, double tol,
                                                        double* __restrict__ x_out, double* __restrict__ mu_out,
                                                        int* __restrict__ it_out, int per_trial) {
  static_assert(DP <= 64, "lane = coordinate");
  constexpr int NW = NT / 16;              // one record per row of 16 lanes
  __shared__ double red[NW][DP + 1];
  __shared__ double sx[DP];
  __shared__ int done;
  const int c = blockIdx.x, tid = threadIdx.x;
  // count: starts that exist -- one number for the launch (per_trial = 0) or one per block of per_trial starts (the
  // trials of ppbo_mean_search_multi)
  if (count && (per_trial > 0 ? (c % per_trial) >= count[c / per_trial] : c >= *count)) {
    if (tid == 0) { mu_out[c] = -INFINITY; if (it_out) it_out[c] = 0; }
    return;
  }
  const bool w0 = tid < 64;
  const int d = tid;                       // coordinate of this lane (wavefront 0 only)
  const bool live = w0 && d < D;
  double x = 0.0, g = 0.0, mu = 0.0, step = 0.0, xn = 0.0;
  if (tid < DP) {
    x = live ? fmin(fmax(starts[(size_t)c * D + d], 0.0), 1.0) : 0.0;
    sx[tid] = x;
  }
  if (tid == 0) done = 0;
  __syncthreads();
  ev(sx, red);
  __syncthreads();
  if (w0) {
    const int dd = d < DP ? d : DP - 1;
    g = live ? red_col<NW, DP>(red, dd) : 0.0;
    mu = red_col<NW, DP>(red, DP);
    const double gn = sqrt(wave_sum_dpp(g * g));
    step = 0.02 / fmax(gn, 1e-300);        // first move: 0.02 in the unit box
  }
  int it = 0;
  for (; it < iters; ++it) {
    if (w0) {
      const double pg = ((x <= 0.0 && g < 0.0) || (x >= 1.0 && g > 0.0)) ? 0.0 : g;
      const double pn = sqrt(wave_sum_dpp(pg * pg));
      if (!(pn * step >= tol)) { if (tid == 0) done = 1; }
      else {
        xn = fmin(fmax(x + step * pg, 0.0), 1.0);
        if (tid < DP) sx[tid] = live ? xn : 0.0;
      }
    }
    __syncthreads();
    if (done) break;
    ev(sx, red);
    __syncthreads();
    if (w0) {
      const int dd = d < DP ? d : DP - 1;
      const double gnew = live ? red_col<NW, DP>(red, dd) : 0.0;
      const double mun = red_col<NW, DP>(red, DP);
      const bool ok = mun >= mu;
      const double sv = live ? xn - x : 0.0, yv = gnew - g;
      const double curv = -wave_sum_dpp(sv * yv);          // > 0 where mu is locally concave along the move
      const double ss = wave_sum_dpp(sv * sv);
      step = ok ? (curv > 0.0 ? ss / fmax(curv, 1e-300) : 2.0 * step) : 0.25 * step;
      if (ok) { x = xn; g = gnew; mu = mun; }
    }
    // the next write to sx / red happens after every wave has passed the barrier above
  }
  if (live) x_out[(size_t)c * D + d] = x;
  if (tid == 0) { mu_out[c] = mu; if (it_out) it_out[c] = it; }
}

// out = frac(in + shift): a Cranley-Patterson rotation of a resident uniform candidate pool (keeps it uniform)
__global__ __launch_bounds__(256) void shift_points_kernel(const double* __restrict__ in, int64_t n, int D,
                                                           const double* __restrict__ shift,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = in[i] + shift[i % D];
  out[i] = v - floor(v);
}

// out = in * scale row-wise (in place allowed): ARD's input scaling s (.) x and the gradient's way back
__global__ __launch_bounds__(256) void scale_points_kernel(const double* in, int64_t n, int D,
                                                           const double* __restrict__ scale, double* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = in[i] * scale[i % D];
}

// out[d][r] = in[r][d]  (R x D row-major -> D x R): the ascent kernels read their operand transposed
__global__ __launch_bounds__(256) void transpose_rows_kernel(const double* __restrict__ in, int R, int D,
                                                             double* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  for (int d = 0; d < D; ++d) out[(size_t)d * R + r] = in[(size_t)r * D + d];
}

// A call's coordinate map (ppbo_coords), resolved on the host: what the launchers need of it.
struct CoordMap {
  int kind = PPBO_COORDS_MODEL, D = 0;
  const double* h_coef = nullptr;    // SCALED: s[D]; CAMPHOR: l[6] (host)
  double* d_scale = nullptr;         // SCALED, after upload(): s[D] | 1 / s[D] on the device
  CamphorCoef cam;                   // CAMPHOR: the camphor form's coefficients ...
  CamphorInvL inv_l;                 // ... and 1 / l
  const ppbo_model* model = nullptr; // model entries: the model in the CALLER's coordinates -- the model itself, or `view`
  ppbo_model view;                   // CAMPHOR: kernel camphor at D = 6 over d_Xc with the embedded model's alpha and theta
                                     // (its KernParams carry sf2 only, the coefficients travel in cam)
  // s and 1 / s in one upload (nothing for the other kinds); after every refusal of the entry, ahead of its launches
  int upload(ppbo_ctx* ctx, hipStream_t s) {
    if (kind != PPBO_COORDS_SCALED) return 0;
    d_scale = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SCALE, 128 * sizeof(double));
    if (!d_scale) return (int)hipErrorOutOfMemory;
    double hs[128];
    for (int d = 0; d < D; ++d) { hs[d] = h_coef[d]; hs[D + d] = 1.0 / h_coef[d]; }
    return ppbo_upload_async(ctx, d_scale, hs, 2 * (size_t)D * sizeof(double), s);
  }
};

// The one validation of a map (c = NULL: the identity) over points of D <= 64 caller coordinates and a kernel id
static int resolve_coords(ppbo_ctx* ctx, const ppbo_coords* c, int kernel_id, int D, CoordMap& co) {
  co.D = D;
  if (!c || c->kind == PPBO_COORDS_MODEL) return 0;
  PPBO_REQUIRE(ctx, c->kind == PPBO_COORDS_SCALED || c->kind == PPBO_COORDS_CAMPHOR, "coords.kind (PPBO_COORDS_*)");
  if (c->kind == PPBO_COORDS_SCALED) {
    PPBO_REQUIRE(ctx, c->h_coef != nullptr, "coords.h_coef (D scales)");
    PPBO_REQUIRE(ctx, kernel_id != PPBO_KERNEL_CAMPHOR, "per-dimension scales need a radial kernel");
    for (int d = 0; d < D; ++d)
      PPBO_REQUIRE(ctx, c->h_coef[d] > 0.0 && std::isfinite(c->h_coef[d]), "coords.h_coef: positive finite scales");
  } else {
    PPBO_REQUIRE_CAMPHOR_L(ctx, c->h_coef);
    PPBO_REQUIRE(ctx, D == CAMPHOR_D, "camphor coordinates: six of them");
    co.cam = camphor_coef(c->h_coef);
    co.inv_l = camphor_inv_l(c->h_coef);
  }
  co.kind = c->kind;
  co.h_coef = c->h_coef;
  return 0;
}

// ... of a model's map, behind the checks every mean entry makes of its model
static int resolve_model_coords(ppbo_ctx* ctx, const ppbo_model* m, CoordMap& co) {
  PPBO_REQUIRE(ctx, m != nullptr && m->d_X && m->d_alpha, "model X/alpha");
  PPBO_REQUIRE(ctx, m->N > 0 && m->D > 0 && m->D <= 64, "model sizes (D<=64)");
  PPBO_REQUIRE_KERNEL(ctx, m->kernel_id, m->D);
  co.model = m;
  if (m->coords.kind != PPBO_COORDS_CAMPHOR) return resolve_coords(ctx, &m->coords, m->kernel_id, m->D, co);
  PPBO_REQUIRE_CAMPHOR_MODEL(ctx, m);
  PPBO_REQUIRE(ctx, m->coords.d_Xc != nullptr, "coords.d_Xc (the design rows in the caller's coordinates)");
  if (int rc = resolve_coords(ctx, &m->coords, PPBO_KERNEL_CAMPHOR, CAMPHOR_D, co)) return rc;
  co.view = *m;
  co.view.kernel_id = PPBO_KERNEL_CAMPHOR;
  co.view.D = CAMPHOR_D;
  co.view.d_X = m->coords.d_Xc;
  co.view.d_G = nullptr;
  co.view.d_Gt = nullptr;
  co.model = &co.view;
  return 0;
}

// m: the model in the caller's coordinates (co.model, where the call has a map)
template <int KID>
int launch_mean_ascent(ppbo_ctx* ctx, const ppbo_model* m, const KernParams& p, const CoordMap& co, const double* starts,
                       const int* count, int K, int iters, double tol, double* x_out, double* mu_out, int* it_out,
                       hipStream_t s, int per_trial = 0) {
  double* Xt = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_TRANSPOSE, (size_t)m->N * m->D * sizeof(double));
  if (!Xt) return (int)hipErrorOutOfMemory;
  transpose_rows_kernel<<<(m->N + 255) / 256, 256, 0, s>>>(m->d_X, m->N, m->D, Xt);
  // threads per start: one wavefront per SIMD (256 threads) leaves every dependent fp64 instruction's latency exposed;
  // more wavefronts hide it, as far as the registers of the dimension bucket allow (and the design has rows for them)
#define MA_LAUNCH(DP, NT)                                                                                             \
  do {                                                                                                                \
    MeanEval<KID, DP, NT> ev{Xt, m->N, m->D, p, m->d_alpha};                                                        \
    if constexpr (kid_radial<KID>) {                                                                                  \
      if (co.d_scale) {                                                                                               \
        ScaledMeanEval<KID, DP, NT> sev{ev, co.d_scale};                                                              \
        bb_ascent_kernel<DP, ScaledMeanEval<KID, DP, NT>, NT><<<K, NT, 0, s>>>(sev, m->D, starts, count, iters, tol, x_out, mu_out, it_out, per_trial); \
        break;                                                                                                        \
      }                                                                                                               \
    }                                                                                                                 \
    if constexpr (KID == PPBO_KERNEL_CAMPHOR) {                                                                       \
      if (co.kind == PPBO_COORDS_CAMPHOR) {                                                                           \
        CamphorMeanEval<DP, NT> cev{Xt, m->N, p.sf2, co.cam, m->d_alpha};                                             \
        bb_ascent_kernel<DP, CamphorMeanEval<DP, NT>, NT><<<K, NT, 0, s>>>(cev, m->D, starts, count, iters, tol, x_out, mu_out, it_out, per_trial); \
        break;                                                                                                        \
      }                                                                                                               \
    }                                                                                                                 \
    bb_ascent_kernel<DP, MeanEval<KID, DP, NT>, NT><<<K, NT, 0, s>>>(ev, m->D, starts, count, iters, tol, x_out, mu_out, it_out, per_trial); \
  } while (0)
  const bool tall = m->N >= 1024;
  if (KID == PPBO_KERNEL_CAMPHOR || m->D <= 8) { if (tall) MA_LAUNCH(8, 1024); else MA_LAUNCH(8, 256); }
  else if constexpr (KID != PPBO_KERNEL_CAMPHOR) {     // (camphor-copper: D = 6)
    if (m->D <= 24) { if (tall) MA_LAUNCH(24, 512); else MA_LAUNCH(24, 256); }
    else MA_LAUNCH(64, 256);
  }
#undef MA_LAUNCH
  return 0;
}

// one ascent launch of an RFF posterior sample: S = 0 one sample, K workgroups; S > 0 S samples of K starts each, S K
// workgroups (RffSampleEval), count[s] starts exist
template <int DP, int NT, class EV>
void rff_ascent_run(const EV& ev, int D, int S, int K, const double* starts, const int* count, int iters, double tol,
                    double* x_out, double* v_out, hipStream_t s) {
  if (S > 0)
    bb_ascent_kernel<DP, RffSampleEval<EV>, NT><<<S * K, NT, 0, s>>>(RffSampleEval<EV>{ev, K}, D, starts, count, iters, tol,
                                                                     x_out, v_out, nullptr, K);
  else
    bb_ascent_kernel<DP, EV, NT><<<K, NT, 0, s>>>(ev, D, starts, count, iters, tol, x_out, v_out, nullptr, 0);
}

// the RFF ascent over the basis W_rows [F][D] or (PPBO_COORDS_CAMPHOR) the camphor basis W_rows [F][11] with starts and
// results in the caller's six coordinates
int launch_rff_ascent(ppbo_ctx* ctx, const double* W_rows, int F, int D, const CoordMap& co, const double* b,
                      const double* omega, double amp, const double* starts, const int* count, int S, int K, int iters,
                      double tol, double* x_out, double* v_out, hipStream_t s) {
  const bool camphor = co.kind == PPBO_COORDS_CAMPHOR;
  const int DW = camphor ? CAMPHOR_E : D;
  double* W = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_TRANSPOSE, (size_t)F * DW * sizeof(double));
  if (!W) return (int)hipErrorOutOfMemory;
  transpose_rows_kernel<<<(F + 255) / 256, 256, 0, s>>>(W_rows, F, DW, W);
  const RffPoly P = make_rff_poly(1.0);
  const bool wide = F >= 1024;
  if (camphor) {
#define RA_LAUNCH(NT) \
  rff_ascent_run<8, NT>(CamphorRffEval<NT>{W, F, b, omega, amp, P, co.inv_l}, CAMPHOR_D, S, K, starts, count, iters, tol, x_out, v_out, s)
    // 11 embedded columns of point, gradient and feature row: ~170 VGPRs, so at most two wavefronts per SIMD (1024
    // threads would spill)
    if (wide) RA_LAUNCH(512); else RA_LAUNCH(256);
#undef RA_LAUNCH
  } else {
#define RA_LAUNCH(DP, NT) \
  rff_ascent_run<DP, NT>(RffEval<DP, NT>{W, F, D, b, omega, amp, P}, D, S, K, starts, count, iters, tol, x_out, v_out, s)
    if (D <= 8) { if (wide) RA_LAUNCH(8, 1024); else RA_LAUNCH(8, 256); }
    else if (D <= 24) { if (wide) RA_LAUNCH(24, 512); else RA_LAUNCH(24, 256); }
    else RA_LAUNCH(64, 256);
#undef RA_LAUNCH
  }
  return 0;
}

// the pathwise ascent: S x K workgroups over the basis W_rows [F][D] and the design X_rows [N][D], both transposed into
// one workspace slot ([D][F] | [D][N])
template <int KID>
int launch_path_ascent(ppbo_ctx* ctx, const KernParams& p, const double* W_rows, int F, int D, const double* b,
                       const double* wp, double amp, const double* X_rows, int N, const double* v, const double* d_scale,
                       const double* starts, const int* count, int S, int K, int iters, double tol, double* x_out,
                       double* v_out, hipStream_t s) {
  double* W = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_TRANSPOSE, ((size_t)F + N) * D * sizeof(double));
  if (!W) return (int)hipErrorOutOfMemory;
  double* Xt = W + (size_t)F * D;
  transpose_rows_kernel<<<(F + 255) / 256, 256, 0, s>>>(W_rows, F, D, W);
  transpose_rows_kernel<<<(N + 255) / 256, 256, 0, s>>>(X_rows, N, D, Xt);
  const RffPoly P = make_rff_poly(1.0);
  const bool wide = F + N >= 1024;
#define PA_LAUNCH(DP, NT)                                                                                          \
  bb_ascent_kernel<DP, PathEval<KID, DP, NT>, NT><<<S * K, NT, 0, s>>>(                                            \
      PathEval<KID, DP, NT>{W, F, D, b, wp, amp, P, Xt, N, p, v, d_scale, K}, D, starts, count, iters, tol, x_out, \
      v_out, nullptr, K)
  // threads per start as launch_rff_ascent
  if (D <= 8) { if (wide) PA_LAUNCH(8, 1024); else PA_LAUNCH(8, 256); }
  else if (D <= 24) { if (wide) PA_LAUNCH(24, 512); else PA_LAUNCH(24, 256); }
  else PA_LAUNCH(64, 256);
#undef PA_LAUNCH
  return 0;
}

template <int KID>
int launch_mean_grad(const ppbo_model* m, const KernParams& p, const double* d_Xc, int M, double* d_mu, double* d_grad,
                     hipStream_t s) {
#define MG_LAUNCH(DP) mean_grad_kernel<KID, DP><<<M, 256, 0, s>>>(m->d_X, m->N, m->D, p, m->d_alpha, d_Xc, d_mu, d_grad)
  if (KID == PPBO_KERNEL_CAMPHOR || m->D <= 8) MG_LAUNCH(8);
  else if constexpr (KID != PPBO_KERNEL_CAMPHOR) {     // (camphor-copper: D = 6)
    if (m->D <= 24) MG_LAUNCH(24);
    else MG_LAUNCH(64);
  }
#undef MG_LAUNCH
  return 0;
}

// ---- searches inside boxes (ppbo_mean_ascent_boxes, ppbo_mean_search_boxes) -------------------------------------------
// Kernels of their own beside the unit-box ones, which keep their code: the box costs the ascent two registers per
// coordinate lane, the screening two wave-uniform operands per coordinate.
// A box on the device is lo[D] | hi[D] | hi - lo [D] | max_d (hi_d - lo_d): box_stride(D) doubles, packed on the host from
// the validated h_boxes (one IEEE subtraction: the same bits wherever it is made).
static inline size_t box_stride(int D) { return 3 * (size_t)D + 1; }

// The candidates of the trials of one ppbo_mean_search_boxes launch, never materialised: slot i < M of trial t is
// fma(hi_t - lo_t, u, lo_t) with u = frac(pool + shift_t) (u = pool without shifts), the S slots behind are trial t's seed
// rows clipped into its box.  Every trial has all Mt = M + S slots.
struct BoxCands {
  const double* pool = nullptr; long long M = 0; const double* shifts = nullptr;
  const double* boxes = nullptr;   // box_stride(D) doubles per trial
  const double* seeds = nullptr;   // [trials][S][D]
  int S = 0, D = 0;
};
__device__ __forceinline__ double box_coord(const BoxCands& c, int trial, long long i, int d) {
  const double* __restrict__ b = c.boxes + (size_t)trial * (3 * c.D + 1);
  if (i < c.M) {
    double u = c.pool[(size_t)i * c.D + d];
    if (c.shifts) { const double v = u + c.shifts[(size_t)trial * c.D + d]; u = v - floor(v); }
    return fma(b[2 * c.D + d], u, b[d]);
  }
  return fmin(fmax(c.seeds[((size_t)trial * c.S + (i - c.M)) * c.D + d], b[d]), b[c.D + d]);
}

// mean_screen_kernel over BoxCands: the trial is blockIdx.z, so lo and hi - lo are wave-uniform (scalar loads), and
// every slot of every trial is present.  The row loop is mean_screen_kernel's.
template <int KID, int DP>
__global__ __launch_bounds__(SCR_T) void box_screen_kernel(const double* __restrict__ X, int N, int D, KernParams p,
                                                           const double* __restrict__ alpha, BoxCands bc,
                                                           int rows_per_split, int n_split, double* __restrict__ part) {
  constexpr int NP = SCR_CPT / 2;
  __shared__ __attribute__((aligned(16))) float xs[SCR_RJ][DP];
  __shared__ double sa[SCR_RJ];
  const int trial = blockIdx.z;
  const long long Mt = bc.M + bc.S;
  const long long c0 = ((long long)blockIdx.x * SCR_T + threadIdx.x) * SCR_CPT;
  float2_t xc[NP][DP];
  double mu[SCR_CPT];
#pragma unroll
  for (int q = 0; q < SCR_CPT; ++q) {
    mu[q] = 0.0;
    const bool there = c0 + q < Mt;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const float v = (d < D && there) ? (float)box_coord(bc, trial, c0 + q, d) : 0.0f;
      if (q & 1) xc[q >> 1][d].y = v; else xc[q >> 1][d].x = v;
    }
  }
  const float c0f = (float)p.c0, c1f = (float)p.c1, sf2f = (float)p.sf2;
  const int j_beg = blockIdx.y * rows_per_split;
  int j_end = j_beg + rows_per_split;
  if (j_end > N) j_end = N;
  for (int row0 = j_beg; row0 < j_end; row0 += SCR_RJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < SCR_RJ * DP; e += SCR_T) {
      const int r = e / DP, d = e - r * DP, j = row0 + r;
      xs[r][d] = (j < j_end && d < D) ? (float)X[(size_t)j * D + d] : 0.0f;
    }
    if (threadIdx.x < SCR_RJ) sa[threadIdx.x] = (row0 + (int)threadIdx.x < j_end) ? alpha[row0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int rmax = (j_end - row0 < SCR_RJ) ? (j_end - row0) : SCR_RJ;
    for (int r = 0; r < rmax; ++r) {
      float2_t sv[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) sv[q] = float2_t{0.0f, 0.0f};
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const float x = xs[r][d];
        const float2_t xx = {x, x};
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          if (KID == PPBO_KERNEL_CAMPHOR) sv[q] += screen_term2<KID>(xx - xc[q][d], d, c0f, c1f);
          else { const float2_t dx = xx - xc[q][d]; sv[q] = __builtin_elementwise_fma(dx, dx, sv[q]); }
        }
      }
      const double a = sa[r];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        mu[2 * q] = fma(a, (double)screen_finish<KID>(sv[q].x, sf2f, c0f), mu[2 * q]);
        mu[2 * q + 1] = fma(a, (double)screen_finish<KID>(sv[q].y, sf2f, c0f), mu[2 * q + 1]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < SCR_CPT; ++q)
    if (c0 + q < Mt) part[((size_t)trial * n_split + blockIdx.y) * Mt + c0 + q] = mu[q];
}

// candidates of trial t as rows (the fp64 screening and the screenings under a coordinate map)
__global__ __launch_bounds__(256) void box_rows_kernel(BoxCands bc, int trial, double* __restrict__ out) {
  const long long n = (bc.M + bc.S) * bc.D;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  out[e] = box_coord(bc, trial, e / bc.D, (int)(e % bc.D));
}

// group_max_kernel of the boxed trials (blockIdx.y): a group's survivor is also written out as a row, surv[trial][t][D],
// and gidx[trial][t] names that row -- select_starts_kernel then reads its coordinates from `surv` as from any
// candidate array and needs no boxed form
__global__ __launch_bounds__(256) void box_group_max_kernel(const double* __restrict__ mu, int64_t Mt, int G, int T,
                                                            BoxCands bc, double* __restrict__ gval,
                                                            int* __restrict__ gidx, double* __restrict__ surv) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int trial = blockIdx.y;
  mu += (size_t)trial * Mt;
  const int64_t lo = (int64_t)t * G, hi = (lo + G < Mt) ? lo + G : Mt;
  double best = -INFINITY;
  int64_t bi = lo;
  for (int64_t i = lo; i < hi; ++i) {
    const double v = mu[i];
    if (v > best) { best = v; bi = i; }         // NaN never wins
  }
  const size_t row = (size_t)trial * T + t;
  gval[row] = best;
  gidx[row] = (int)row;
  for (int d = 0; d < bc.D; ++d) surv[row * bc.D + d] = box_coord(bc, trial, bi, d);
}

// bb_ascent_kernel inside a box: start c uses box c / per_box (boxes: box_stride(D) doubles each).  lo_d and hi_d sit in
// two registers of the coordinate's lane; the start and every iterate are clipped to [lo, hi], the projection zeroes g_d
// at an active bound, the first move is 0.02 of the longest side.  A coordinate with lo == hi never moves and never
// enters the projected norm; a box of one point ends at it = 0.  With lo = 0, hi = 1 every expression is
// bb_ascent_kernel's (0.02 * 1.0 is exact).  count: one number of existing starts per box.
template <int DP, class EVAL, int NT>
__global__ __launch_bounds__(NT) void bb_ascent_box_kernel(EVAL ev, int D, const double* __restrict__ starts,
                                                            const int* __restrict__ count,
                                                            const double* __restrict__ boxes, int per_box, int iters,
                                                            double tol, double* __restrict__ x_out,
                                                            double* __restrict__ mu_out, int* __restrict__ it_out) {
  static_assert(DP <= 64, "lane = coordinate");
  constexpr int NW = NT / 16;              // one record per row of 16 lanes
  __shared__ double red[NW][DP + 1];
  __shared__ double sx[DP];
  __shared__ int done;
  const int c = blockIdx.x, tid = threadIdx.x;
  const int b = c / per_box;
  if (count && (c - b * per_box) >= count[b]) {
    if (tid == 0) { mu_out[c] = -INFINITY; if (it_out) it_out[c] = 0; }
    return;
  }
  const bool w0 = tid < 64;
  const int d = tid;                       // coordinate of this lane (wavefront 0 only)
  const bool live = w0 && d < D;
  const double* __restrict__ bx = boxes + (size_t)b * (3 * D + 1);
  const double lo = live ? bx[d] : 0.0, hi = live ? bx[D + d] : 0.0;
  const double wmax = bx[3 * D];           // the longest side (the same for every lane)
  double x = 0.0, g = 0.0, mu = 0.0, step = 0.0, xn = 0.0;
  if (tid < DP) {
    x = live ? fmin(fmax(starts[(size_t)c * D + d], lo), hi) : 0.0;
    sx[tid] = x;
  }
  if (tid == 0) done = 0;
  __syncthreads();
  ev(sx, red);
  __syncthreads();
  if (w0) {
    const int dd = d < DP ? d : DP - 1;
    g = live ? red_col<NW, DP>(red, dd) : 0.0;
    mu = red_col<NW, DP>(red, DP);
    const double gn = sqrt(wave_sum_dpp(g * g));
    step = (0.02 * wmax) / fmax(gn, 1e-300);        // first move: 0.02 of the longest side
  }
  int it = 0;
  for (; it < iters; ++it) {
    if (w0) {
      const double pg = ((x <= lo && g < 0.0) || (x >= hi && g > 0.0)) ? 0.0 : g;
      const double pn = sqrt(wave_sum_dpp(pg * pg));
      if (!(pn * step >= tol) || !(wmax > 0.0)) { if (tid == 0) done = 1; }
      else {
        xn = fmin(fmax(x + step * pg, lo), hi);
        if (tid < DP) sx[tid] = live ? xn : 0.0;
      }
    }
    __syncthreads();
    if (done) break;
    ev(sx, red);
    __syncthreads();
    if (w0) {
      const int dd = d < DP ? d : DP - 1;
      const double gnew = live ? red_col<NW, DP>(red, dd) : 0.0;
      const double mun = red_col<NW, DP>(red, DP);
      const bool ok = mun >= mu;
      const double sv = live ? xn - x : 0.0, yv = gnew - g;
      const double curv = -wave_sum_dpp(sv * yv);          // > 0 where mu is locally concave along the move
      const double ss = wave_sum_dpp(sv * sv);
      step = ok ? (curv > 0.0 ? ss / fmax(curv, 1e-300) : 2.0 * step) : 0.25 * step;
      if (ok) { x = xn; g = gnew; mu = mun; }
    }
    // the next write to sx / red happens after every wave has passed the barrier above
  }
  if (live) x_out[(size_t)c * D + d] = x;
  if (tid == 0) { mu_out[c] = mu; if (it_out) it_out[c] = it; }
}

// launch_mean_ascent's buckets over bb_ascent_box_kernel; Xt: the design of m transposed (transposed_design)
template <int KID>
int launch_mean_ascent_boxes(const ppbo_model* m, const KernParams& p, const CoordMap& co, const double* Xt,
                             const double* starts, const int* count, const double* boxes, int per_box, int K, int iters,
                             double tol, double* x_out, double* mu_out, int* it_out, hipStream_t s) {
#define MB_RUN(DP, NT, ev) \
  bb_ascent_box_kernel<DP, decltype(ev), NT><<<K, NT, 0, s>>>(ev, m->D, starts, count, boxes, per_box, iters, tol, x_out, mu_out, it_out)
#define MB_LAUNCH(DP, NT)                                                                                             \
  do {                                                                                                                \
    MeanEval<KID, DP, NT> ev{Xt, m->N, m->D, p, m->d_alpha};                                                        \
    if constexpr (kid_radial<KID>) {                                                                                  \
      if (co.d_scale) {                                                                                               \
        ScaledMeanEval<KID, DP, NT> sev{ev, co.d_scale};                                                              \
        MB_RUN(DP, NT, sev);                                                                                          \
        break;                                                                                                        \
      }                                                                                                               \
    }                                                                                                                 \
    if constexpr (KID == PPBO_KERNEL_CAMPHOR) {                                                                       \
      if (co.kind == PPBO_COORDS_CAMPHOR) {                                                                           \
        CamphorMeanEval<DP, NT> cev{Xt, m->N, p.sf2, co.cam, m->d_alpha};                                             \
        MB_RUN(DP, NT, cev);                                                                                          \
        break;                                                                                                        \
      }                                                                                                               \
    }                                                                                                                 \
    MB_RUN(DP, NT, ev);                                                                                             \
  } while (0)
  const bool tall = m->N >= 1024;
  if (KID == PPBO_KERNEL_CAMPHOR || m->D <= 8) { if (tall) MB_LAUNCH(8, 1024); else MB_LAUNCH(8, 256); }
  else if constexpr (KID != PPBO_KERNEL_CAMPHOR) {     // (camphor-copper: D = 6)
    if (m->D <= 24) { if (tall) MB_LAUNCH(24, 512); else MB_LAUNCH(24, 256); }
    else MB_LAUNCH(64, 256);
  }
#undef MB_LAUNCH
#undef MB_RUN
  return 0;
}

// the design of m ([N][D]) transposed into the ascent's workspace slot
static double* transposed_design(ppbo_ctx* ctx, const ppbo_model* m, hipStream_t s) {
  double* Xt = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_TRANSPOSE, (size_t)m->N * m->D * sizeof(double));
  if (Xt) transpose_rows_kernel<<<(m->N + 255) / 256, 256, 0, s>>>(m->d_X, m->N, m->D, Xt);
  return Xt;
}

// h_boxes[B][2][D] validated and packed into the device form (box_stride(D) doubles per box)
static int pack_boxes(ppbo_ctx* ctx, const double* h_boxes, int B, int D, std::vector<double>& out) {
  const size_t bs = box_stride(D);
  out.assign((size_t)B * bs, 0.0);
  for (int b = 0; b < B; ++b) {
    const double* lo = h_boxes + (size_t)b * 2 * D;
    const double* hi = lo + D;
    double* o = out.data() + (size_t)b * bs;
    double wmax = 0.0;
    for (int d = 0; d < D; ++d) {
      PPBO_REQUIRE(ctx, std::isfinite(lo[d]) && std::isfinite(hi[d]) && lo[d] >= 0.0 && hi[d] <= 1.0 && lo[d] <= hi[d],
                   "boxes: 0 <= lo <= hi <= 1, finite");
      o[d] = lo[d]; o[D + d] = hi[d]; o[2 * D + d] = hi[d] - lo[d];
      if (o[2 * D + d] > wmax) wmax = o[2 * D + d];
    }
    o[3 * D] = wmax;
  }
  return 0;
}

template <int KID>
int launch_box_screen(const ppbo_model* m, const KernParams& p, const BoxCands& bc, int nb, int rows_per_split,
                      int n_split, double* part, hipStream_t s) {
  const long long Mt = bc.M + bc.S;
  const dim3 grid((unsigned)((Mt + SCR_T * SCR_CPT - 1) / (SCR_T * SCR_CPT)), n_split, nb);
  auto launch = [&](auto dp) {
    box_screen_kernel<KID, decltype(dp)::value><<<grid, SCR_T, 0, s>>>(m->d_X, m->N, m->D, p, m->d_alpha, bc, rows_per_split, n_split, part);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 6>{});
  else ScreenLadder::dispatch(m->D, launch);
  return 0;
}

}  // namespace


extern "C" int ppbo_mean_grad(ppbo_ctx* ctx, const ppbo_model* m, const double* d_Xc, int64_t M, double* d_mu,
                              double* d_grad, void* stream) {
  PPBO_ENTER(ctx);
  CoordMap co;
  if (int rc = resolve_model_coords(ctx, m, co)) return rc;
  PPBO_REQUIRE(ctx, d_Xc && d_mu && d_grad && M >= 0 && M < (1 << 30), "points / outputs");
  if (M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = co.upload(ctx, s)) return rc;
  // the kernel runs in the model's coordinates: on the points mapped forward, its gradient pulled back afterwards
  const double* pts = d_Xc;
  double* g = d_grad;
  const int64_t n = M * co.D;
  if (co.kind == PPBO_COORDS_SCALED) {
    double* rows = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SCALE_SEARCH, (size_t)n * sizeof(double));
    if (!rows) return (int)hipErrorOutOfMemory;
    scale_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_Xc, n, co.D, co.d_scale, rows);
    PPBO_LAUNCH_CHECK(ctx);
    pts = rows;
  } else if (co.kind == PPBO_COORDS_CAMPHOR) {
    // workspace: the embedded points [M][11] | their gradient [M][11]
    double* e = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_CAMPHOR, (size_t)2 * M * CAMPHOR_E * sizeof(double));
    if (!e) return (int)hipErrorOutOfMemory;
    if (int rc = ppbo_camphor_embed(ctx, d_Xc, M, co.h_coef, e, stream)) return rc;
    pts = e;
    g = e + (size_t)M * CAMPHOR_E;
  }
  const KernParams p = make_kern_params(m->kernel_id, m->theta);
  if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
        return launch_mean_grad<decltype(kid)::value>(m, p, pts, (int)M, d_mu, g, s);
      }))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  if (co.kind == PPBO_COORDS_SCALED) {          // d mu / d x_d = s_d d mu / d x~_d
    scale_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_grad, n, co.D, co.d_scale, d_grad);
    PPBO_LAUNCH_CHECK(ctx);
  } else if (co.kind == PPBO_COORDS_CAMPHOR) {
    return ppbo_camphor_pullback(ctx, pts, g, M, co.inv_l.v[2], d_grad, s);
  }
  return 0;
}


extern "C" int ppbo_shift_points(ppbo_ctx* ctx, const double* d_in, int64_t M, int D, const double* h_shift,
                                 double* d_out, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_in && d_out && h_shift && M > 0 && D > 0 && D <= 64, "arguments (D <= 64)");
  hipStream_t s = (hipStream_t)stream;
  double* dsh = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SEARCH_SMALL, 64 * sizeof(double));
  if (!dsh) return (int)hipErrorOutOfMemory;
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(dsh, h_shift, (size_t)D * sizeof(double), hipMemcpyHostToDevice, s));
  const int64_t n = M * D;
  shift_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_in, n, D, dsh, d_out);
  PPBO_LAUNCH_CHECK(ctx);
  // h_shift is pageable host memory: the copy above is only asynchronous with respect to the DEVICE, the host
  // buffer has been consumed when hipMemcpyAsync returns
  return 0;
}

extern "C" int ppbo_mean_ascent(ppbo_ctx* ctx, const ppbo_model* model, const double* d_starts, int K, int iters,
                                double tol, double* d_x, double* d_mu, int* d_iters, void* stream) {
  PPBO_ENTER(ctx);
  CoordMap co;
  if (int rc = resolve_model_coords(ctx, model, co)) return rc;
  PPBO_REQUIRE(ctx, d_starts && d_x && d_mu && K > 0 && K <= 65536 && iters >= 0 && tol >= 0, "starts / outputs");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = co.upload(ctx, s)) return rc;
  const ppbo_model* m = co.model;
  const KernParams p = make_kern_params(m->kernel_id, m->theta);
  if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
        return launch_mean_ascent<decltype(kid)::value>(ctx, m, p, co, d_starts, nullptr, K, iters, tol, d_x, d_mu, d_iters, s);
      }))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" int ppbo_scale_points(ppbo_ctx* ctx, const double* d_in, int64_t M, int D, const double* h_scale,
                                 double* d_out, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_in && d_out && h_scale && M >= 0 && D > 0 && D <= 64, "arguments (D <= 64)");
  if (M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  double* dsc = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SCALE_PTS, 64 * sizeof(double));
  if (!dsc) return (int)hipErrorOutOfMemory;
  if (int rc = ppbo_upload_async(ctx, dsc, h_scale, (size_t)D * sizeof(double), s)) return rc;
  const int64_t n = M * D;
  scale_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_in, n, D, dsc, d_out);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" int ppbo_mean_search(ppbo_ctx* ctx, const ppbo_model* m, const double* d_cand, int64_t M, int K, double sep,
                                int iters, double tol, double* d_x, double* d_mu, int* h_found, void* stream) {
  PPBO_ENTER(ctx);
  CoordMap co;
  if (int rc = resolve_model_coords(ctx, m, co)) return rc;
  PPBO_REQUIRE(ctx, co.kind == PPBO_COORDS_MODEL, "a model with a coordinate map: ppbo_mean_search_multi has that form");
  PPBO_REQUIRE(ctx, d_cand && d_x && d_mu && M > 0 && M < ((int64_t)1 << 31), "candidates / outputs");
  PPBO_REQUIRE(ctx, K > 0 && K <= 1024 && sep >= 0 && iters >= 0 && tol >= 0, "K (<= 1024) / sep / iters / tol");
  hipStream_t s = (hipStream_t)stream;
  StartSelection sel{M, 1, m->D, K};
  if (!sel.alloc(ctx, 0, 0)) return (int)hipErrorOutOfMemory;
  ppbo_model mean_only = *m;
  mean_only.d_G = nullptr;
  mean_only.proj.rows = 0;   // the mean entries ignore model->proj (ppbo_predict would check that it fits)
  if (int rc = ppbo_predict(ctx, &mean_only, d_cand, M, PPBO_SCORE_MEAN, 0.0, sel.scores, nullptr, nullptr, nullptr, nullptr,
                            stream))
    return rc;
  sel.select(ctx, sep, d_cand, TrialCands{}, sel.counts, s);
  const KernParams p = make_kern_params(m->kernel_id, m->theta);
  if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
        return launch_mean_ascent<decltype(kid)::value>(ctx, m, p, co, sel.starts, sel.counts, K, iters, tol, d_x, d_mu, nullptr, s);
      }))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  if (h_found) {
    PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h_found, sel.counts, sizeof(int), hipMemcpyDeviceToHost, s));
    PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  }
  return 0;
}


// row splits of a screening launch: enough workgroups to fill the chip (2048), at most 16 splits of >= SCR_RJ rows
static void screen_split(int blocks_x, int nb, int N, int& n_split, int& rows_per_split) {
  n_split = (2048 + blocks_x * nb - 1) / (blocks_x * nb);
  if (n_split > 16) n_split = 16;
  if (n_split > (N + SCR_RJ - 1) / SCR_RJ) n_split = (N + SCR_RJ - 1) / SCR_RJ;
  if (n_split < 1) n_split = 1;
  rows_per_split = (N + n_split - 1) / n_split;
  n_split = (N + rows_per_split - 1) / rows_per_split;
}

template <int KID>
int launch_screen(const ppbo_model* m, const KernParams& p, const TrialCands& tc, int nb, int rows_per_split, int n_split,
                  double* part, int extra_trial, hipStream_t s) {
  const long long Mt = tc.M + tc.E;
  const dim3 grid((unsigned)((Mt + SCR_T * SCR_CPT - 1) / (SCR_T * SCR_CPT)), n_split, nb);
  auto launch = [&](auto dp) {
    mean_screen_kernel<KID, decltype(dp)::value><<<grid, SCR_T, 0, s>>>(m->d_X, m->N, m->D, p, m->d_alpha, tc, rows_per_split, n_split, part,
                                                                        extra_trial);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 6>{});
  else ScreenLadder::dispatch(m->D, launch);
  return 0;
}

extern "C" int ppbo_mean_search_multi(ppbo_ctx* ctx, const ppbo_model* model, const double* d_pool, int64_t M,
                                      const double* h_shifts, int T, const double* d_extra, int E_rows,
                                      const double* h_xprev, int K, double sep, int iters, double tol, int screen_fp32,
                                      double* d_x, double* d_mu, void* stream) {
  PPBO_ENTER(ctx);
  CoordMap co;
  if (int rc = resolve_model_coords(ctx, model, co)) return rc;
  // m: the model in the caller's coordinates, where the search runs; emb (camphor): the embedded model, screened as SE
  const ppbo_model* m = co.model;
  const ppbo_model* emb = co.kind == PPBO_COORDS_CAMPHOR ? model : nullptr;
  PPBO_REQUIRE(ctx, d_pool && h_shifts && d_x && d_mu && M > 0 && E_rows >= 0 && M + E_rows + 1 < ((int64_t)1 << 31),
               "pool / shifts / extra points / outputs");
  const bool design = E_rows > 0 && !d_extra;
  if (design) {       // NULL with a row count: the model's own design points
    PPBO_REQUIRE(ctx, E_rows == m->N, "d_extra = NULL stands for the model's N design points: E_rows must be N");
    d_extra = m->d_X;
  }
  const int E = E_rows + (h_xprev ? 1 : 0);
  PPBO_REQUIRE(ctx, T >= 1 && T <= 64 && K > 0 && K <= 1024 && sep >= 0 && iters >= 0 && tol >= 0, "T (<= 64) / K (<= 1024) / sep / iters / tol");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D;
  const long long Mt = M + E;
  // workspace: shifts[T][D] + xprev[D] ahead of the start selection's T score vectors; counts[T]
  // (ARD: the design's rows in the caller's coordinates [N][D] in a slot of their own)
  StartSelection sel{Mt, T, D, K};
  if (!sel.alloc(ctx, (size_t)(T + 1) * D, T)) return (int)hipErrorOutOfMemory;
  double* shifts = sel.head;
  double* xprev = shifts + (size_t)T * D;
  double* mu = sel.scores;
  // the shifts and the previous x* leave the host through pinned upload slots of the ctx (ppbo_upload_async): the call
  // has consumed h_shifts / h_xprev when it returns and never blocks on the stream
  if (int rc = ppbo_upload_async(ctx, shifts, h_shifts, (size_t)T * D * sizeof(double), s)) return rc;
  if (h_xprev)
    if (int rc = ppbo_upload_async(ctx, xprev, h_xprev, (size_t)D * sizeof(double), s)) return rc;
  if (int rc = co.upload(ctx, s)) return rc;
  const double* d_scale = co.d_scale;
  if (d_scale && design) {
    // the design points (the model's scaled rows) are taken back to the caller's coordinates, x_i = x~_i / s, so that
    // rotation, separation and box all live there
    const int64_t n = (int64_t)m->N * D;
    double* xo = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SCALE_SEARCH, (size_t)n * sizeof(double));
    if (!xo) return (int)hipErrorOutOfMemory;
    scale_points_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(m->d_X, n, D, d_scale + D, xo);
    PPBO_LAUNCH_CHECK(ctx);
    d_extra = xo;
  }
  TrialCands tc;
  tc.pool = d_pool; tc.M = M; tc.shifts = shifts; tc.extra = d_extra; tc.xprev = h_xprev ? xprev : nullptr;
  tc.E_rows = E_rows; tc.E = E; tc.D = D;
  const KernParams p = make_kern_params(m->kernel_id, m->theta);
  if (screen_fp32 && co.kind == PPBO_COORDS_MODEL) {
    // the trials in batches of <= 8 (bounds the partial sums: 8 x n_split x Mt doubles)
    const int blocks_x = (int)((Mt + SCR_T * SCR_CPT - 1) / (SCR_T * SCR_CPT));
    for (int t0 = 0; t0 < T; t0 += 8) {
      const int nb = (T - t0 < 8) ? (T - t0) : 8;
      int n_split, rows_per_split;
      screen_split(blocks_x, nb, m->N, n_split, rows_per_split);
      double* part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, (size_t)nb * n_split * Mt * sizeof(double));
      if (!part) return (int)hipErrorOutOfMemory;
      TrialCands tb = tc;
      tb.shifts = shifts + (size_t)t0 * D;
      const int extra_trial = (t0 == 0 && E > 0) ? 0 : -1;     // only the job's trial 0 sees the extra points
      if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
            return launch_screen<decltype(kid)::value>(m, p, tb, nb, rows_per_split, n_split, part, extra_trial, s);
          }))
        return rc;
      screen_sum_kernel<<<dim3((unsigned)((Mt + 255) / 256), nb), 256, 0, s>>>(part, n_split, Mt, M, extra_trial, mu + (size_t)t0 * Mt);
      PPBO_LAUNCH_CHECK(ctx);
    }
  } else {
    // fp64 screening: every trial's candidates written out as rows and scored by ppbo_predict (mean only), exactly
    // what the one-trial entry does with the rows ppbo_shift_points leaves.  ARD: the rows are scaled to s (.) x first,
    // and the fp32 screening takes them as the extra points of a one-trial launch of mean_screen_kernel (which reads
    // extra points as they are), so that the kernel itself needs no scaled form
    // camphor: the candidates are embedded and screened on the embedded model, as SE
    double* rows = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SEARCH_ROWS, (size_t)Mt * D * sizeof(double));
    if (!rows) return (int)hipErrorOutOfMemory;
    double* erows = rows;
    int De = D;
    if (emb) {
      erows = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_CAMPHOR_ROWS, (size_t)Mt * CAMPHOR_E * sizeof(double));
      if (!erows) return (int)hipErrorOutOfMemory;
      De = CAMPHOR_E;
    }
    const ppbo_model* sm = emb ? emb : m;
    const KernParams sp = emb ? make_kern_params(PPBO_KERNEL_SE, emb->theta) : p;
    ppbo_model mean_only = *sm;
    mean_only.d_G = nullptr;
    mean_only.proj.rows = 0;   // the mean entries ignore model->proj (ppbo_predict would check that it fits)
    for (int t = 0; t < T; ++t) {
      const long long nt = M + (t == 0 ? E : 0);
      trial_rows_kernel<<<(unsigned)((nt * D + 255) / 256), 256, 0, s>>>(tc, t, rows);
      if (d_scale) scale_points_kernel<<<(unsigned)((nt * D + 255) / 256), 256, 0, s>>>(rows, nt * D, D, d_scale, rows);
      PPBO_LAUNCH_CHECK(ctx);
      if (emb)
        if (int rc = ppbo_camphor_embed(ctx, rows, nt, co.h_coef, erows, stream)) return rc;
      if (screen_fp32) {
        TrialCands tr;
        tr.pool = erows; tr.M = 0; tr.shifts = shifts; tr.extra = erows; tr.E_rows = (int)nt; tr.E = (int)nt; tr.D = De;
        int n_split, rows_per_split;
        screen_split((int)((nt + SCR_T * SCR_CPT - 1) / (SCR_T * SCR_CPT)), 1, m->N, n_split, rows_per_split);
        double* part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, (size_t)n_split * nt * sizeof(double));
        if (!part) return (int)hipErrorOutOfMemory;
        // (camphor-copper has no ARD form: refused above; the camphor model screens as SE)
        if (int rc = ppbo_kernel_dispatch<true>(ctx, sm->kernel_id, [&](auto kid) {
              return launch_screen<decltype(kid)::value>(sm, sp, tr, 1, rows_per_split, n_split, part, 0, s);
            }))
          return rc;
        screen_sum_kernel<<<dim3((unsigned)((nt + 255) / 256), 1), 256, 0, s>>>(part, n_split, nt, 0, 0, mu + (size_t)t * Mt);
        PPBO_LAUNCH_CHECK(ctx);
      } else if (int rc = ppbo_predict(ctx, &mean_only, erows, nt, PPBO_SCORE_MEAN, 0.0, mu + (size_t)t * Mt, nullptr, nullptr,
                                       nullptr, nullptr, stream)) {
        return rc;
      }
      if (nt < Mt) {
        // absent slots: -inf (0xFFF0000000000000 is not a byte pattern: a tiny fill kernel)
        fill_kernel<<<(unsigned)((Mt - nt + 255) / 256), 256, 0, s>>>(mu + (size_t)t * Mt + nt, Mt - nt, -INFINITY);
      }
    }
  }
  sel.select(ctx, sep, nullptr, tc, sel.counts, s);
  PPBO_LAUNCH_CHECK(ctx);
  if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
        return launch_mean_ascent<decltype(kid)::value>(ctx, m, p, co, sel.starts, sel.counts, T * K, iters, tol, d_x, d_mu,
                                                        nullptr, s, K);
      }))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

// the map of an RFF search: the identity, or the camphor basis over six caller coordinates
extern "C" int ppbo_mean_ascent_boxes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_starts, int K,
                                      const double* h_boxes, int B, int per_box, int iters, double tol, double* d_x,
                                      double* d_mu, int* d_iters, void* stream) {
  PPBO_ENTER(ctx);
  CoordMap co;
  if (int rc = resolve_model_coords(ctx, model, co)) return rc;
  PPBO_REQUIRE(ctx, d_starts && h_boxes && d_x && d_mu && K > 0 && K <= 65536 && iters >= 0 && tol >= 0,
               "starts / boxes / outputs");
  PPBO_REQUIRE(ctx, per_box >= 1 && B == (K + per_box - 1) / per_box, "B == ceil(K / per_box), per_box >= 1");
  const ppbo_model* m = co.model;
  std::vector<double> hb;
  if (int rc = pack_boxes(ctx, h_boxes, B, m->D, hb)) return rc;
  hipStream_t s = (hipStream_t)stream;
  double* boxes = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_BOX, hb.size() * sizeof(double));
  if (!boxes) return (int)hipErrorOutOfMemory;
  if (int rc = ppbo_upload_async(ctx, boxes, hb.data(), hb.size() * sizeof(double), s)) return rc;
  if (int rc = co.upload(ctx, s)) return rc;
  const double* Xt = transposed_design(ctx, m, s);
  if (!Xt) return (int)hipErrorOutOfMemory;
  const KernParams p = make_kern_params(m->kernel_id, m->theta);
  if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
        return launch_mean_ascent_boxes<decltype(kid)::value>(m, p, co, Xt, d_starts, nullptr, boxes, per_box, K, iters, tol,
                                                              d_x, d_mu, d_iters, s);
      }))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" int ppbo_mean_search_boxes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_pool, int64_t M,
                                      const double* h_shifts, const double* h_boxes, int T, const double* d_seeds, int S,
                                      int K, double sep, int iters, double tol, int screen_fp32, double* d_x, double* d_mu,
                                      int* d_count, void* stream) {
  PPBO_ENTER(ctx);
  CoordMap co;
  if (int rc = resolve_model_coords(ctx, model, co)) return rc;
  // m: the model in the caller's coordinates, where the search runs; emb (camphor): the embedded model, screened as SE
  const ppbo_model* m = co.model;
  const ppbo_model* emb = co.kind == PPBO_COORDS_CAMPHOR ? model : nullptr;
  PPBO_REQUIRE(ctx, d_pool && h_boxes && d_x && d_mu && M >= 1, "pool / boxes / outputs");
  PPBO_REQUIRE(ctx, T >= 1 && T <= 4096 && K >= 1 && K <= 1024 && (int64_t)T * K <= 65536, "T (<= 4096) / K (<= 1024) / T K (<= 65536)");
  PPBO_REQUIRE(ctx, S >= 0 && S <= 64 && (S == 0 || d_seeds) && M < ((int64_t)1 << 31) / 64 - S, "seeds (S <= 64) / 64 (M + S) < 2^31");
  PPBO_REQUIRE(ctx, sep >= 0 && iters >= 0 && tol >= 0, "sep / iters / tol");
  const int D = m->D;
  std::vector<double> hb;
  if (int rc = pack_boxes(ctx, h_boxes, T, D, hb)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long long Mt = M + S;
  const size_t bs = box_stride(D);
  constexpr int TB = 64;                 // trials per batch: bounds the score vectors (TB x Mt doubles)
  const int nb_max = T < TB ? T : TB;
  // device copies: the packed boxes of all trials, then the shifts -- one host array, one upload
  const size_t n_box = hb.size();
  if (h_shifts) hb.insert(hb.end(), h_shifts, h_shifts + (size_t)T * D);
  double* boxes = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_BOX, hb.size() * sizeof(double));
  if (!boxes) return (int)hipErrorOutOfMemory;
  double* shifts = h_shifts ? boxes + n_box : nullptr;
  StartSelection sel{Mt, nb_max, D, K};
  if (!sel.alloc(ctx, 0, nb_max)) return (int)hipErrorOutOfMemory;
  double* surv = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_BOX_SURV, (size_t)nb_max * sel.Tg * D * sizeof(double));
  if (!surv) return (int)hipErrorOutOfMemory;
  const bool on_the_fly = screen_fp32 && co.kind == PPBO_COORDS_MODEL;
  // the row split of the fp32 screening depends on the candidates and the design alone, never on T or the batch: a
  // trial's scores are the same bits in whichever call and batch it runs
  const int blocks_x = (int)((Mt + SCR_T * SCR_CPT - 1) / (SCR_T * SCR_CPT));
  int n_split = 1, rows_per_split = m->N;
  screen_split(blocks_x, 1, m->N, n_split, rows_per_split);
  double *rows = nullptr, *erows = nullptr, *part = nullptr;
  int De = D;
  if (on_the_fly) {
    part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, (size_t)(nb_max < 8 ? nb_max : 8) * n_split * Mt * sizeof(double));
    if (!part) return (int)hipErrorOutOfMemory;
  } else {
    erows = rows = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SEARCH_ROWS, (size_t)Mt * D * sizeof(double));
    if (!rows) return (int)hipErrorOutOfMemory;
    if (emb) {
      erows = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_CAMPHOR_ROWS, (size_t)Mt * CAMPHOR_E * sizeof(double));
      if (!erows) return (int)hipErrorOutOfMemory;
      De = CAMPHOR_E;
    }
    if (screen_fp32) {
      part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, (size_t)n_split * Mt * sizeof(double));
      if (!part) return (int)hipErrorOutOfMemory;
    }
  }
  // every refusal lies above; the boxes and shifts leave the host through a pinned upload slot (nothing blocks)
  if (int rc = ppbo_upload_async(ctx, boxes, hb.data(), hb.size() * sizeof(double), s)) return rc;
  if (int rc = co.upload(ctx, s)) return rc;
  const double* d_scale = co.d_scale;
  const double* Xt = transposed_design(ctx, m, s);
  if (!Xt) return (int)hipErrorOutOfMemory;
  const KernParams p = make_kern_params(m->kernel_id, m->theta);
  const ppbo_model* sm = emb ? emb : m;
  const KernParams sp = emb ? make_kern_params(PPBO_KERNEL_SE, emb->theta) : p;
  ppbo_model mean_only = *sm;
  mean_only.d_G = nullptr;
  mean_only.proj.rows = 0;   // the mean entries ignore model->proj (ppbo_predict would check that it fits)
  double* mu = sel.scores;
  for (int t0 = 0; t0 < T; t0 += TB) {
    const int nb = (T - t0 < TB) ? (T - t0) : TB;
    BoxCands bc;
    bc.pool = d_pool; bc.M = M; bc.shifts = shifts ? shifts + (size_t)t0 * D : nullptr; bc.boxes = boxes + (size_t)t0 * bs;
    bc.seeds = S ? d_seeds + (size_t)t0 * S * D : nullptr; bc.S = S; bc.D = D;
    if (on_the_fly) {
      for (int u0 = 0; u0 < nb; u0 += 8) {      // (bounds the partial sums: 8 x n_split x Mt doubles)
        const int nu = (nb - u0 < 8) ? (nb - u0) : 8;
        BoxCands bu = bc;
        if (bu.shifts) bu.shifts += (size_t)u0 * D;
        bu.boxes += (size_t)u0 * bs;
        if (bu.seeds) bu.seeds += (size_t)u0 * S * D;
        if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
              return launch_box_screen<decltype(kid)::value>(m, p, bu, nu, rows_per_split, n_split, part, s);
            }))
          return rc;
        screen_sum_kernel<<<dim3((unsigned)((Mt + 255) / 256), nu), 256, 0, s>>>(part, n_split, Mt, Mt, -1, mu + (size_t)u0 * Mt);
        PPBO_LAUNCH_CHECK(ctx);
      }
    } else {
      // the routes of ppbo_mean_search_multi: a trial's candidates written out as rows, scaled (ARD) or embedded
      // (camphor), and scored by ppbo_predict or by a one-trial launch of mean_screen_kernel over the rows
      for (int t = 0; t < nb; ++t) {
        box_rows_kernel<<<(unsigned)((Mt * D + 255) / 256), 256, 0, s>>>(bc, t, rows);
        if (d_scale) scale_points_kernel<<<(unsigned)((Mt * D + 255) / 256), 256, 0, s>>>(rows, Mt * D, D, d_scale, rows);
        PPBO_LAUNCH_CHECK(ctx);
        if (emb)
          if (int rc = ppbo_camphor_embed(ctx, rows, Mt, co.h_coef, erows, stream)) return rc;
        if (screen_fp32) {
          TrialCands tr;
          tr.pool = erows; tr.M = 0; tr.shifts = erows; tr.extra = erows; tr.E_rows = (int)Mt; tr.E = (int)Mt; tr.D = De;
          if (int rc = ppbo_kernel_dispatch<true>(ctx, sm->kernel_id, [&](auto kid) {
                return launch_screen<decltype(kid)::value>(sm, sp, tr, 1, rows_per_split, n_split, part, 0, s);
              }))
            return rc;
          screen_sum_kernel<<<dim3((unsigned)((Mt + 255) / 256), 1), 256, 0, s>>>(part, n_split, Mt, 0, 0, mu + (size_t)t * Mt);
          PPBO_LAUNCH_CHECK(ctx);
        } else if (int rc = ppbo_predict(ctx, &mean_only, erows, Mt, PPBO_SCORE_MEAN, 0.0, mu + (size_t)t * Mt, nullptr, nullptr,
                                         nullptr, nullptr, stream)) {
          return rc;
        }
      }
    }
    int* counts = d_count ? d_count + t0 : sel.counts;
    box_group_max_kernel<<<dim3((sel.Tg + 255) / 256, nb), 256, 0, s>>>(mu, Mt, sel.G, sel.Tg, bc, sel.gval, sel.gidx, surv);
    const size_t sel_lds = (size_t)sel.Tg * (1 + D) * sizeof(double);
    if (sel_lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)select_starts_kernel, 150 * 1024);
    select_starts_kernel<<<nb, 1024, sel_lds, s>>>(sel.gval, sel.gidx, sel.Tg, surv, D, K, sep * sep, sel.starts, counts, TrialCands{});
    PPBO_LAUNCH_CHECK(ctx);
    if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
          return launch_mean_ascent_boxes<decltype(kid)::value>(m, p, co, Xt, sel.starts, counts, bc.boxes, K, nb * K, iters, tol,
                                                                d_x + (size_t)t0 * K * D, d_mu + (size_t)t0 * K, nullptr, s);
        }))
      return rc;
    PPBO_LAUNCH_CHECK(ctx);
  }
  return 0;
}

static int resolve_rff_coords(ppbo_ctx* ctx, const ppbo_coords* coords, int D, CoordMap& co) {
  PPBO_REQUIRE(ctx, !coords || coords->kind != PPBO_COORDS_SCALED, "coords: a scaled basis is a basis, pass W s");
  return resolve_coords(ctx, coords, PPBO_KERNEL_SE, D, co);
}

// the candidates a search scores: d_cand itself, or (camphor) its embedding at Dr = 11 columns in a workspace
static int rff_score_rows(ppbo_ctx* ctx, const CoordMap& co, const double* d_cand, int64_t M, const double*& rows, int& Dr,
                          void* stream) {
  rows = d_cand;
  Dr = co.D;
  if (co.kind != PPBO_COORDS_CAMPHOR) return 0;
  double* e = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_CAMPHOR_ROWS, (size_t)M * CAMPHOR_E * sizeof(double));
  if (!e) return ppbo_set_error(ctx, (int)hipErrorOutOfMemory, "invalid argument: no workspace for the embedded candidates");
  rows = e;
  Dr = CAMPHOR_E;
  return ppbo_camphor_embed(ctx, d_cand, M, co.h_coef, e, stream);
}

extern "C" int ppbo_rff_search(ppbo_ctx* ctx, const double* d_cand, int64_t M, int D, const double* d_W, int F,
                               const double* d_b, double sigma_f, const double* d_omega, const ppbo_coords* coords, int K,
                               double sep, int iters, double tol, double* d_x, double* d_val, int* h_found, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_cand && d_W && d_b && d_omega && d_x && d_val, "null pointer");
  PPBO_REQUIRE(ctx, M > 0 && M < ((int64_t)1 << 31) && D > 0 && D <= 64 && F > 0, "sizes (D <= 64)");
  CoordMap co;
  if (int rc = resolve_rff_coords(ctx, coords, D, co)) return rc;
  PPBO_REQUIRE(ctx, K > 0 && K <= 1024 && sep >= 0 && iters >= 0 && tol >= 0, "K (<= 1024) / sep / iters / tol");
  hipStream_t s = (hipStream_t)stream;
  StartSelection sel{M, 1, D, K};
  if (!sel.alloc(ctx, 0, 0)) return (int)hipErrorOutOfMemory;
  const double* rows;
  int Dr;
  if (int rc = rff_score_rows(ctx, co, d_cand, M, rows, Dr, stream)) return rc;
  if (int rc = ppbo_rff_score(ctx, rows, M, Dr, d_W, F, d_b, sigma_f, d_omega, sel.scores, nullptr, nullptr, stream)) return rc;
  // start selection on the caller-coordinate rows: sep is in the caller's units
  sel.select(ctx, sep, d_cand, TrialCands{}, sel.counts, s);
  if (int rc = launch_rff_ascent(ctx, d_W, F, D, co, d_b, d_omega, std::sqrt(2.0 * sigma_f * sigma_f / (double)F), sel.starts,
                                 sel.counts, 0, K, iters, tol, d_x, d_val, s))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  if (h_found) {
    PPBO_HIP_CHECK(ctx, hipMemcpyAsync(h_found, sel.counts, sizeof(int), hipMemcpyDeviceToHost, s));
    PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  }
  return 0;
}

// ppbo_rff_search for S samples over one candidate set
extern "C" int ppbo_rff_search_multi(ppbo_ctx* ctx, const double* d_cand, int64_t M, int D, const double* d_W, int F,
                                     const double* d_b, double sigma_f, const double* d_omegas, const ppbo_coords* coords,
                                     int S, int K, double sep, int iters, double tol, double* d_x, double* d_val,
                                     int* d_found, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_cand && d_W && d_b && d_omegas && d_x && d_val && d_found, "null pointer");
  PPBO_REQUIRE(ctx, M > 0 && M < ((int64_t)1 << 31) && D > 0 && D <= 64 && F > 0, "sizes (D <= 64)");
  CoordMap co;
  if (int rc = resolve_rff_coords(ctx, coords, D, co)) return rc;
  PPBO_REQUIRE(ctx, S > 0 && S <= PPBO_RFF_MULTI_MAX_S, "S (1 .. PPBO_RFF_MULTI_MAX_S samples)");
  PPBO_REQUIRE(ctx, K > 0 && K <= 1024 && sep >= 0 && iters >= 0 && tol >= 0, "K (<= 1024) / sep / iters / tol");
  hipStream_t s = (hipStream_t)stream;
  // one "trial" per sample over the shared candidates: each sample's K starts are > sep apart in its own scores; the
  // start counts go to d_found
  StartSelection sel{M, S, D, K};
  if (!sel.alloc(ctx, 0, 0))
    return ppbo_set_error(ctx, (int)hipErrorOutOfMemory, "invalid argument: no workspace for %d samples of %lld candidates",
                          S, (long long)M);
  const double* rows;
  int Dr;
  if (int rc = rff_score_rows(ctx, co, d_cand, M, rows, Dr, stream)) return rc;
  if (int rc = ppbo_rff_score_multi(ctx, rows, M, Dr, d_W, F, d_b, sigma_f, d_omegas, S, sel.scores, stream)) return rc;
  sel.select(ctx, sep, d_cand, TrialCands{}, d_found, s);
  PPBO_LAUNCH_CHECK(ctx);
  if (int rc = launch_rff_ascent(ctx, d_W, F, D, co, d_b, d_omegas, std::sqrt(2.0 * sigma_f * sigma_f / (double)F),
                                 sel.starts, d_found, S, K, iters, tol, d_x, d_val, s))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

// ppbo_rff_search_multi for pathwise samples g_s = phi^T w_s + k(., X) v_s: the same three stages with the scoring launch
// and the evaluator of the ascent replaced (ppbo_path_score_multi, PathEval)
extern "C" int ppbo_path_search_multi(ppbo_ctx* ctx, int kernel_id, const double theta[3], const double* d_cand, int64_t M,
                                      int D, const double* d_W, int F, const double* d_b, const double* d_Wp,
                                      const double* d_X, int N, const double* d_V, const ppbo_coords* coords, int S, int K,
                                      double sep, int iters, double tol, double* d_x, double* d_val, int* d_found,
                                      void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, theta && d_cand && d_W && d_b && d_Wp && d_X && d_V && d_x && d_val && d_found, "null pointer");
  PPBO_REQUIRE(ctx, M > 0 && M < ((int64_t)1 << 31) && D > 0 && D <= 64 && F > 0 && N > 0, "sizes (D <= 64)");
  PPBO_REQUIRE(ctx, S > 0 && S <= PPBO_RFF_MULTI_MAX_S, "S (1 .. PPBO_RFF_MULTI_MAX_S samples)");
  PPBO_REQUIRE(ctx, K > 0 && K <= 1024 && sep >= 0 && iters >= 0 && tol >= 0, "K (<= 1024) / sep / iters / tol");
  PPBO_REQUIRE(ctx, kernel_id != PPBO_KERNEL_CAMPHOR && ppbo_kernel_id_valid(kernel_id),
               "kernel_id (a radial kernel: SE, RQ, Matern-5/2, Matern-3/2)");
  PPBO_REQUIRE(ctx, !coords || coords->kind != PPBO_COORDS_CAMPHOR, "coords: pathwise samples have no camphor form");
  CoordMap co;
  if (int rc = resolve_coords(ctx, coords, kernel_id, D, co)) return rc;
  hipStream_t s = (hipStream_t)stream;
  StartSelection sel{M, S, D, K};
  if (!sel.alloc(ctx, 0, 0))
    return ppbo_set_error(ctx, (int)hipErrorOutOfMemory, "invalid argument: no workspace for %d samples of %lld candidates",
                          S, (long long)M);
  // ARD: the scoring launch works in the model's coordinates -- the candidates scaled, the basis unscaled (w / s).(s x)
  // = w.x -- in a slot of their own: cand s [M][D] | W / s [F][D]
  const double *rows = d_cand, *Wm = d_W;
  if (int rc = co.upload(ctx, s)) return rc;
  if (co.d_scale) {
    double* cs = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SCALE_SEARCH, ((size_t)M + F) * D * sizeof(double));
    if (!cs) return (int)hipErrorOutOfMemory;
    double* Ws = cs + (size_t)M * D;
    scale_points_kernel<<<(unsigned)((M * D + 255) / 256), 256, 0, s>>>(d_cand, M * D, D, co.d_scale, cs);
    scale_points_kernel<<<(unsigned)(((int64_t)F * D + 255) / 256), 256, 0, s>>>(d_W, (int64_t)F * D, D, co.d_scale + D, Ws);
    PPBO_LAUNCH_CHECK(ctx);
    rows = cs; Wm = Ws;
  }
  if (int rc = ppbo_path_score_multi(ctx, kernel_id, theta, rows, M, D, Wm, F, d_b, d_Wp, d_X, N, d_V, S, sel.scores, stream))
    return rc;
  // start selection on the caller-coordinate rows: sep is in the caller's units
  sel.select(ctx, sep, d_cand, TrialCands{}, d_found, s);
  PPBO_LAUNCH_CHECK(ctx);
  const KernParams p = make_kern_params(kernel_id, theta);
  const double amp = std::sqrt(2.0 * theta[2] * theta[2] / (double)F);
  if (int rc = ppbo_kernel_dispatch<true>(ctx, kernel_id, [&](auto kid) -> int {
        return launch_path_ascent<decltype(kid)::value>(ctx, p, d_W, F, D, d_b, d_Wp, amp, d_X, N, d_V, co.d_scale, sel.starts,
                                                        d_found, S, K, iters, tol, d_x, d_val, s);
      }))
    return rc;
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}
