// K2+K3+K4: batched candidate scoring (posterior mean, variance, score, argmax).
//   reference: gp_model.py:441-461 (mu_Sigma_pred / mu_pred), called per candidate by
//   mu_star's DE (:415-437) and per 70-point line by EI/varmax (acquisition.py:72-81,170-178).
//
// Posterior state (see ppbo_posterior): alpha = Sigma^-1 f_MAP, Lambda_MAP in star form,
// G = R Lambda with R = chol(Sigma^-1 - Lambda)^-1 (block lower triangular).  For a candidate x
//   mu(x)  = k*' alpha
//   var(x) = sigma_f^2 - k*' A k*,  A = Sigma^-1 - Sigma^-1 P Sigma^-1  (gp_model.py:449)
//          = sigma_f^2 + k*' Lambda k* + |G k*|^2                        (Woodbury, same operator)
// Pass 1 (star_geom_kernel, then kstar_kernel, VALU): one lane = two candidates held in registers.  SE / RQ / Matern in
//   fp64: the m + 1 rows of a star lie on one line x_obs + s_j xi, so |c - x_j|^2 = r0^2 - 2 s_j beta + s_j^2 |xi|^2 with
//   r0^2 = |c - x_obs|^2 and beta = xi.(c - x_obs): two inner products of depth D per (candidate, star), from x_obs and xi
//   staged in LDS, then two FMAs, the clip and the kernel function per row; s_j, s_j^2 |xi|^2, alpha and Lambda of the
//   row arrive by scalar loads.  star_geom_kernel forms xi, s_j and a collinearity flag per star on every call (N D
//   doubles read; nothing cached); a star that is not collinear to 2^-50, the fp32 evaluation and camphor take one inner
//   product per row from X rows staged in LDS and read as broadcasts (SE / RQ / Matern: the reference's expansion with the
//   candidate pre-scaled by -2, one FMA per dimension; camphor: its feature form).  Writes K*[N, Mc] (j-major) once and
//   reduces mu and k*'Lambda k* in registers.  C3 (N = 2048, D = 20, 65536 candidates): 0.336 -> 0.259 ms + 0.011 ms for
//   the geometry, 122 M -> 80 M vector and 15.8 M -> 0.7 M LDS instructions per launch
//   (profiles/r15_kstar_star_form.txt).  PPBO_KSTAR_STAR=0: always one inner product per row.
// Pass 2 (quadform_kernel, fp64 MFMA): Y = G K* on 128x128 tiles (16 wavefronts of 32x32), K range cut
//   at the block-triangular edge per wavefront, epilogue = column sums of Y^2 into per-row-tile slabs.
//   Workgroups are ordered candidate-tile-fastest in chunks of 128 tiles (PPBO_QF_ORDER, default 514):
//   all resident workgroups stream the same G row panel out of L2 while their K* chunk sits in the
//   Infinity Cache.  PPBO_QF_VARIANT (default 4: 16 wavefronts of 32x32) selects the measured tile shapes, see DESIGN.md.
// Pass 3 (score_kernel): slab sums -> var, score, per-block argmax; (argmax_final_kernel) -> 1 value.
// Host drivers: every entry plans its call with the same objects, each on its caller's stack and each requesting its
//   workspace slots once, before the caller's first launch.  Chunks (common.h) walks the chunks of a call; ScorePlan owns
//   the padded operator, K* and the partial sums of predict_passes / two_set_passes, LineWorkspace those of the line
//   entries and the gradients, OwnKstar a K* workspace of an entry's own, FieldPass (common.h) the tournament's field
//   pass; BestReturn brings the best back through the host-mapped record; PredictRequest names what predict_passes is asked.
#include <functional>
#include <optional>

#include "gemm_f64.h"
#include "linalg.h"
#include "mc_factor.h"
#include "score.h"
#include "tile_walk.h"

namespace {

using namespace gemm64;

constexpr int KS_THREADS = 256;
constexpr int KS_CPT = 2;  // candidates per thread (even); 4 halves the LDS reads per pair but was measured slower (fewer waves, 32-byte store pieces)

constexpr int KS_RJ = 32;   // X rows staged in LDS per step

// DP = padded dimension (compile time): X rows are zero-padded to DP in LDS and the
// candidate registers likewise, so the inner product loop is branch-free and fully
// unrolled; every lane reads the same LDS address (broadcast), one ds_read_b128 per 2 dims.
// KS_CPT candidates per lane share each of those reads: with the one-FMA-per-dimension form the kernel is
// bound by the LDS pipe (a broadcast b128 read still returns 1 KB per wavefront), not by the vector ALUs.
// fp32 kernel evaluation (F32 = true): the "fp32 tolerance" variant BASELINE config 5 names.  K* entries are
// evaluated in single precision from direct differences (the expansion form loses 4e-5 of mu in fp32),
// then widened; every accumulation (mu, k*'Lambda k*, the MFMA contraction) stays fp64.
template <int KID>
__device__ __forceinline__ float kern_term32(float dx, int d, float c0, float c1) {
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    if (d == 2) return c1 * dx * dx;
    const float sn = sinpif(fabsf(dx));
    return c0 * sn * sn;
  } else {
    static_assert(kid_radial<KID>, "unknown kernel id");
    return dx * dx;
  }
}
template <int KID>
__device__ __forceinline__ float kern_finish32(float s, float sf2, float c0) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    return sf2 * expf(-c0 * s);
  } else if constexpr (KID == PPBO_KERNEL_RQ) {
    const float t = 1.0f + s * c0; return sf2 / (t * t);
  } else if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    return sf2 * expf(-s);
  } else if constexpr (KID == PPBO_KERNEL_MATERN52) {
    const float a = c0 * sqrtf(s);
    return sf2 * (fmaf(a, fmaf(a, 1.0f / 3.0f, 1.0f), 1.0f) * expf(-a));
  } else {
    static_assert(KID == PPBO_KERNEL_MATERN32, "unknown kernel id");
    const float a = c0 * sqrtf(s);
    return sf2 * ((1.0f + a) * expf(-a));
  }
}

// The star-geometry table of a model, [2 N + n_q + n_q D] doubles: s[N], g[N], collinear[n_q] (1.0 / 0.0), xi[n_q][D].
// The rows of star q are its observation x_obs and m points that the feedback places on ONE line through it
// (feedback_processing.py:110-130), x_j = x_obs + s_j xi, so for a candidate c
//   |c - x_j|^2 = |c - x_obs|^2 - 2 s_j xi.(c - x_obs) + s_j^2 |xi|^2 = r0^2 - 2 s_j beta + g_j:
// two inner products per (candidate, star) in place of one per (candidate, row).  xi = the star's difference x_j - x_obs
// of largest norm (the lowest such row), s_j = (x_j - x_obs).xi / |xi|^2, g_j = s_j^2 |xi|^2.  collinear is a CONDITION:
//   max_{j, d} |x_jd - x_obs,d - s_j xi_d| <= 2^-50 max(|x|_inf of the star, |xi|_inf)
// (rows built as x_obs + s xi in fp64 sit at 2^-53); a star that misses it, or holds a non-finite coordinate, keeps
// kstar_kernel's inner product per row.  xi = 0 (every row equals x_obs): collinear, every s_j = 0.
constexpr int SG_STARS = 4;   // stars per workgroup, one wavefront each (no LDS, no barrier)
inline size_t star_geo_doubles(int N, int n_q, int D) { return (size_t)2 * N + n_q + (size_t)n_q * D; }
__global__ __launch_bounds__(64 * SG_STARS) void star_geom_kernel(const double* __restrict__ X, int N, int D, int mblk,
                                                                  int n_q, double* __restrict__ geo) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * SG_STARS + (threadIdx.x >> 6);
  if (q >= n_q) return;       // (a whole wavefront)
  const double* __restrict__ xo = X + (size_t)q * mblk * D;
  double best = -1.0;
  int bj = 0;
  for (int r = lane; r < mblk; r += 64) {
    double n2 = 0.0;
    for (int d = 0; d < D; ++d) { const double v = xo[(size_t)r * D + d] - xo[d]; n2 = fma(v, v, n2); }
    if (n2 > best) { best = n2; bj = r; }            // (a NaN norm is never taken: the row's residual is NaN below)
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int oj = __shfl_xor(bj, o, 64);
    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
  }
  const double xi2 = fmax(best, 0.0);
  const double* __restrict__ xb = xo + (size_t)bj * D;
  double resid = 0.0, big = 0.0;
  bool bad = false;
  for (int r = lane; r < mblk; r += 64) {
    const double* __restrict__ xr = xo + (size_t)r * D;
    double dot = 0.0;
    for (int d = 0; d < D; ++d) dot = fma(xr[d] - xo[d], xb[d] - xo[d], dot);
    const double sj = xi2 > 0.0 ? dot / xi2 : 0.0;
    for (int d = 0; d < D; ++d) {
      const double z = xb[d] - xo[d];
      const double e = fabs((xr[d] - xo[d]) - sj * z);
      bad |= !(e == e);                              // (fmax drops a NaN)
      resid = fmax(resid, e);
      big = fmax(big, fmax(fabs(xr[d]), fabs(z)));
    }
    geo[(size_t)q * mblk + r] = sj;
    geo[(size_t)N + (size_t)q * mblk + r] = sj * sj * xi2;
  }
  resid = wave_max(resid);
  big = wave_max(big);
  bad = __ballot(bad) != 0;
  double* __restrict__ xi = geo + (size_t)2 * N + n_q + (size_t)q * D;
  for (int d = lane; d < D; d += 64) xi[d] = xb[d] - xo[d];
  if (lane == 0) geo[(size_t)2 * N + q] = (!bad && resid <= 0x1.0p-50 * big) ? 1.0 : 0.0;
}

// (the fp64 radial buckets up to DP = 20 are held to 128 VGPRs = 4 wavefronts per SIMD, the occupancy the flagship shape
// D = 20 had before the star path added r0^2 and beta to the live set; SE fits there without scratch.  RQ and the Matern
// kernels would spill two registers at DP = 20 and are left unbound in that bucket: three wavefronts, no scratch)
// UB (the pruned search, predict_passes): an edge-layout launch that also leaves an upper bound of the contraction.
// The stored column e is cut into its stars; with sig[s] >= the Frobenius norm of the operator's column block of star s
// (block_norm_kernel), |op e| <= sum_s sig[s] |e_s| =: u (Cauchy-Schwarz per star).  The flagged instantiation sums
// ev^2 over the rows of a star and adds sig[s] sqrt(.) at the star's end into u_part[split][c]; splits are whole stars,
// so the partial sums add.  Nothing that the unflagged instantiation computes reads these sums: K*, mu_part and t_part
// are bit for bit its own.  The lane's running u sits in LDS beside |c|^2 (touched once per star); the star's sum of
// squares is two more live doubles, which the buckets DP = 16 and 20 do not have at 128 registers (12-64 bytes of scratch
// per lane), so the flagged instantiation is left unbound there like RQ and Matern at DP = 20: 145 registers, no scratch (bound to
// four wavefronts with the scratch it measured the same: 310 us against the unflagged 252 us at C3).
template <int KID, int DP, bool F32 = false, bool UB = false>
__global__ __launch_bounds__(KS_THREADS, (!F32 && KID != PPBO_KERNEL_CAMPHOR && (DP < 20 || (DP == 20 && KID == PPBO_KERNEL_SE)) && !(UB && DP >= 16)) ? 4 : 1) void kstar_kernel(
    const double* __restrict__ X, int N, int D, KernParams p, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk,
    const double* __restrict__ Xc, int M, double* __restrict__ Kt, int ldk, double* __restrict__ mu_part,
    double* __restrict__ t_part, int q_per_split, int n_q, int edge_k0, const double* __restrict__ geo,
    const double* __restrict__ sig = nullptr, double* __restrict__ u_part = nullptr) {
  static_assert(!UB || !F32, "the bound rides on the fp64 launches");
  __shared__ __attribute__((aligned(16))) double xs[KS_RJ * DP];
  __shared__ double s_alpha[KS_RJ], s_ld[KS_RJ], s_lo[KS_RJ], s_nx[KS_RJ];
  __shared__ int s_col[KS_RJ];
  const int c0 = (blockIdx.x * KS_THREADS + threadIdx.x) * KS_CPT;
  // The camphor kernel in FEATURE form (fp64 path; DP = 12): sin^2(pi (a - b)) = (1 - cos 2pi a cos 2pi b - sin 2pi a sin 2pi b) / 2
  // turns kernels.py:36-53's exponent  c0 sum_k sin^2(pi |a_k - b_k|) + c1 (a_2 - b_2)^2  into
  //   5 c0 / 2 + sum_{f < 10} phi_f(a) psi_f(b) + c1 (a_2 - b_2)^2,  phi = (cos 2pi a_k, sin 2pi a_k)_k,  psi = -(c0 / 2) phi(b):
  // ten FMAs per pair instead of five sinpi evaluations (~20 instructions each: K* was 1.88 ms of C5's 16.6 ms step, six
  // times the SE kernel's cost per pair).  The features of a design row are formed once when it is staged (per 512
  // candidates), those of a candidate once per thread.  Terms of size c0 cancel to the true exponent with an absolute
  // error of ~1e-15 (the kernel value moves by <= 1e-14 relative; Sigma / K* parity is asserted at 1e-12).
  constexpr bool CAMF = (KID == PPBO_KERNEL_CAMPHOR) && !F32 && DP == 12;   // (the only fp64 camphor bucket launched)
  // SE / RQ / Matern use the reference's own expansion r^2 = (|x|^2 + |c|^2) - 2 x.c (kernels.py:7-10) with the
  // candidate pre-scaled by -2: one FMA per dimension and pair instead of a subtract and an FMA.  Its
  // rounding is the rounding every entry of Sigma already carries (posterior mean / variance move by
  // <= 3e-13 / 1e-13 sigma_f^2 on the fixtures against direct differences).  The camphor kernel needs the
  // differences themselves.
  constexpr bool EXPAND = (KID != PPBO_KERNEL_CAMPHOR) && !F32;
  // The STAR path (the expansion-form kernels, geo = star_geom_kernel's table): a collinear star's rows come from
  //   r^2 = max(r0^2 - 2 s_j beta + g_j, 0),  r0^2 = |c - x_obs|^2 and beta = xi.(c - x_obs) formed at the star's first row
  // from direct differences (x_obs and xi staged in LDS, xi in the place of the star's second row): two depth-D inner
  // products per star, then two FMAs and the clip per row -- no LDS row, no |x_j|^2.  The rows are then staged in steps
  // of WHOLE stars (stars of more than KS_RJ rows: pieces of one star), so that a star's first two rows always sit in
  // one step.  A star whose flag is clear takes the inner product per row, bit for bit what geo == nullptr computes
  // (a row's value does not depend on how the rows are cut into steps).  The branch is uniform per workgroup.
  const bool use_geo = EXPAND && geo != nullptr;
  const double* __restrict__ geo_col = use_geo ? geo + (size_t)2 * N : nullptr;
  const double* __restrict__ geo_xi = use_geo ? geo_col + n_q : nullptr;
  double xc[KS_CPT][DP], nc[KS_CPT], mu[KS_CPT], tl[KS_CPT], ko[KS_CPT];
  float xcf[KS_CPT][DP];
  const float c0f = (float)p.c0, c1f = (float)p.c1, sf2f = (float)p.sf2;
#pragma unroll
  for (int q = 0; q < KS_CPT; ++q) {
    nc[q] = 0.0; mu[q] = 0.0; tl[q] = 0.0; ko[q] = 0.0;
    if (CAMF) {
      // psi: -(c0 / 2) (cos, sin)(2 pi c_k) for the periodic coordinates k = 0, 1, 3, 4, 5; then c_2 itself
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int d = k < 2 ? k : k + 1;
        const double v = (c0 + q < M) ? Xc[(size_t)(c0 + q) * D + d] : 0.0;
        double sn, cs;
        sincospi(2.0 * v, &sn, &cs);
        xc[q][k] = -0.5 * p.c0 * cs;
        xc[q][5 + k] = -0.5 * p.c0 * sn;
      }
      xc[q][10] = (c0 + q < M) ? Xc[(size_t)(c0 + q) * D + 2] : 0.0;
      xc[q][11] = 0.0;
      continue;
    }
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      double v = (d < D && c0 + q < M) ? Xc[(size_t)(c0 + q) * D + d] : 0.0;
      if (F32) xcf[q][d] = (float)v;
      if (EXPAND) { nc[q] = fma(v, v, nc[q]); v *= -2.0; }
      xc[q][d] = v;
    }
  }
  // |c|^2 of the lane's candidates, in a slot of the lane's own: read by the plain rows and at the end, so not held in
  // registers across the rows of the collinear stars (the D = 20 bucket has none to spare at four wavefronts per SIMD)
  __shared__ double s_nc[EXPAND ? KS_CPT * KS_THREADS : 1];
  if (EXPAND) {
#pragma unroll
    for (int q = 0; q < KS_CPT; ++q) s_nc[q * KS_THREADS + threadIdx.x] = nc[q];
  }
  __shared__ double s_up[UB ? KS_CPT * KS_THREADS : 1];
  double se[KS_CPT];                       // UB: sum of ev^2 over the rows of the current star
  (void)se;
  if constexpr (UB) {
#pragma unroll
    for (int q = 0; q < KS_CPT; ++q) { s_up[q * KS_THREADS + threadIdx.x] = 0.0; se[q] = 0.0; }
  }
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool vec = (Kt != nullptr) && ((ldk & 1) == 0) && (c0 + KS_CPT - 1 < M);
  const bool has_lam = (lam_diag != nullptr);
  int rb = 0;  // row index inside the current star block (splits start on a block edge)
  int qs = j_beg / mblk;  // ... and that block's star
  // staged row r of the step at row0, from its r^2 (sv; F32: from kv itself) on: the kernel value, the stored entry, the sums
  // a, ld, lo: alpha, lam_diag and lam_off of the row
  auto finish_row = [&](int row0, int r, double (&sv)[KS_CPT], double (&kv)[KS_CPT], double a, double ld, double lo) __attribute__((always_inline)) {
    if (!F32) {
#pragma unroll
      for (int q = 0; q < KS_CPT; ++q) kv[q] = kern_finish<KID>(sv[q], p);
    }
    if (Kt) {
      // node form: row j holds k*_j.  Edge form (edge_k0 >= 0): row n_q + q m + t holds the edge value
      // lam_off[j] (k*_j - k*_obs) of pseudo row j = q (m + 1) + 1 + t; row q (an observation coordinate, a zero column
      // of H) holds zeros where the contraction reads it, i.e. from edge_k0 on
      int drow = row0 + r;
      bool wr = true;
      double ev[KS_CPT];
      if (edge_k0 >= 0) {
        if (rb == 0) {
          drow = qs;
          wr = qs >= edge_k0;
#pragma unroll
          for (int q = 0; q < KS_CPT; ++q) ev[q] = 0.0;
        } else {
          drow = n_q + qs * (mblk - 1) + rb - 1;
#pragma unroll
          for (int q = 0; q < KS_CPT; ++q) ev[q] = lo * (kv[q] - ko[q]);
          if constexpr (UB) {
#pragma unroll
            for (int q = 0; q < KS_CPT; ++q) se[q] = fma(ev[q], ev[q], se[q]);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) ev[q] = kv[q];
      }
      double* dst = Kt + (size_t)drow * ldk + c0;
      if (!wr) {
      } else if (vec) {      // 1 GB streamed out once, read back by the next kernel
#pragma unroll
        for (int q = 0; q < KS_CPT; q += 2) store_through2(dst + q, ev[q], ev[q + 1]);
      } else {
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q)
          if (c0 + q < M) dst[q] = ev[q];
      }
    }
#pragma unroll
    for (int q = 0; q < KS_CPT; ++q) mu[q] += a * kv[q];
    if (has_lam) {
      if (rb == 0) {
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) { ko[q] = kv[q]; tl[q] += ld * kv[q] * kv[q]; }
      } else {
        const double lo2 = 2.0 * lo;
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) tl[q] += kv[q] * (ld * kv[q] + lo2 * ko[q]);
      }
    }
    if constexpr (UB) {
      if (rb + 1 == mblk) {                // the star's last row: its term of the bound (the slot is the lane's own)
        const double sg = uniform_load(sig + qs);
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) {
          s_up[q * KS_THREADS + threadIdx.x] = fma(sg, sqrt(se[q]), s_up[q * KS_THREADS + threadIdx.x]);
          se[q] = 0.0;
        }
      }
    }
    if (++rb == mblk) { rb = 0; ++qs; }
  };
  // ... with r^2 from the staged row itself: one inner product (or sum of terms) of depth D per candidate
  auto plain_row = [&](int row0, int r) __attribute__((always_inline)) {
    const double* __restrict__ xr = xs + r * DP;
    double sv[KS_CPT];
    double kv[KS_CPT];
#pragma unroll
    for (int q = 0; q < KS_CPT; ++q) sv[q] = 0.0;
    if (F32) {
      float sf[KS_CPT];
#pragma unroll
      for (int q = 0; q < KS_CPT; ++q) sf[q] = 0.0f;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const float x = (float)xr[d];
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) sf[q] += kern_term32<KID>(x - xcf[q][d], d, c0f, c1f);
      }
#pragma unroll
      for (int q = 0; q < KS_CPT; ++q) kv[q] = (double)kern_finish32<KID>(sf[q], sf2f, c0f);
    } else if (EXPAND) {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const double x = xr[d];
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) sv[q] = fma(x, xc[q][d], sv[q]);
      }
      const double nx = s_nx[r];
#pragma unroll
      for (int q = 0; q < KS_CPT; ++q) sv[q] = fmax(sv[q] + (nx + s_nc[q * KS_THREADS + threadIdx.x]), 0.0);
    } else if (CAMF) {
#pragma unroll
      for (int d = 0; d < 10; ++d) {
        const double x = xr[d];
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) sv[q] = fma(x, xc[q][d], sv[q]);
      }
      const double x2 = xr[10], base = 2.5 * p.c0;
#pragma unroll
      for (int q = 0; q < KS_CPT; ++q) {
        const double dd = x2 - xc[q][10];
        sv[q] = fma(p.c1 * dd, dd, sv[q] + base);
      }
    } else {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        const double x = xr[d];
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) sv[q] += kern_term<KID>(x - xc[q][d], d, p);
      }
    }
    finish_row(row0, r, sv, kv, s_alpha[r], s_ld[r], s_lo[r]);
  };
  const bool pieces = mblk > KS_RJ;
  int len = 0;
  for (int row0 = j_beg; row0 < j_end; row0 += len) {
    len = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
    if (use_geo) {                         // whole stars, or a piece of one (splits end on a star edge)
      const int whole = pieces ? mblk - rb : (KS_RJ / mblk) * mblk;
      if (whole < len) len = whole;
    }
    // (with a table the lane's index is opaque per step: a staged element's row, star and addresses are formed here, not
    // held in registers across the row loops)
    int tid = threadIdx.x;
    if (use_geo) asm volatile("" : "+v"(tid));
    __syncthreads();
    if (use_geo) {
      // a collinear star leaves x_obs and xi in the first two rows of its place (a piece: of the step, whichever rows
      // of the star it holds) and reads no other row; any other star stages its rows
      const int nst = len < 2 ? 2 : len;
      for (int e = tid; e < nst * DP; e += KS_THREADS) {
        const int r = e / DP, d = e - r * DP;
        const int sq = pieces ? 0 : r / mblk, pos = r - sq * mblk;
        const int star = qs + sq;
        double v = 0.0;
        if (geo_col[star] != 0.0) {
          if (pos > 1) continue;
          if (d < D) v = pos ? geo_xi[(size_t)star * D + d] : X[(size_t)star * mblk * D + d];
        } else {
          if (r >= len) continue;
          if (d < D) v = X[(size_t)(row0 + r) * D + d];
        }
        xs[e] = v;
      }
    } else
    if (CAMF) {                            // phi of the staged rows: (cos, sin)(2 pi x_k) for k = 0, 1, 3, 4, 5; then x_2
      for (int e = threadIdx.x; e < KS_RJ * 6; e += KS_THREADS) {
        const int r = e / 6, k = e - r * 6;
        const int j = row0 + r;
        if (k < 5) {
          const double v = (j < j_end) ? X[(size_t)j * D + (k < 2 ? k : k + 1)] : 0.0;
          double sn, cs;
          sincospi(2.0 * v, &sn, &cs);
          xs[r * DP + k] = cs;
          xs[r * DP + 5 + k] = sn;
        } else {
          xs[r * DP + 10] = (j < j_end) ? X[(size_t)j * D + 2] : 0.0;
          xs[r * DP + 11] = 0.0;
        }
      }
    } else
    for (int e = threadIdx.x; e < KS_RJ * DP; e += KS_THREADS) {
      const int r = e / DP, d = e - r * DP;
      const int j = row0 + r;
      xs[e] = (j < j_end && d < D) ? X[(size_t)j * D + d] : 0.0;
    }
    if (tid < KS_RJ) {
      const int j = row0 + tid;
      const bool ok = j < j_end && (!use_geo || tid < len);
      bool col = false;
      if (use_geo) {
        col = ok && geo_col[qs + (pieces ? 0 : tid / mblk)] != 0.0;
        s_col[tid] = col;
      }
      if (!col) {                          // (the rows of a collinear star take these three by scalar loads)
        s_alpha[tid] = ok ? alpha[j] : 0.0;
        s_ld[tid] = (ok && has_lam) ? lam_diag[j] : 0.0;
        s_lo[tid] = (ok && has_lam) ? lam_off[j] : 0.0;
      }
      if (EXPAND) {
        double nx = 0.0;
        if (ok && !col)
          for (int d = 0; d < D; ++d) { const double v = X[(size_t)j * D + d]; nx = fma(v, v, nx); }
        s_nx[tid] = nx;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < len;) {
      // the staged rows of ONE star (all the staged rows without a table)
      int r_end = len;
      if (use_geo && r + mblk - rb < len) r_end = r + mblk - rb;
      if (!use_geo || __builtin_amdgcn_readfirstlane(s_col[r]) == 0) {
#pragma unroll 1
        for (; r < r_end; ++r) plain_row(row0, r);
        continue;
      }
      if constexpr (EXPAND) {
        // r0^2 = |c - x_obs|^2 and beta = xi.(c - x_obs) from direct differences; xc holds -2 c
        const double* __restrict__ xo = xs + r * DP;
        double r0[KS_CPT], be[KS_CPT];
#pragma unroll
        for (int q = 0; q < KS_CPT; ++q) { r0[q] = 0.0; be[q] = 0.0; }
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double o = xo[d], z = xo[DP + d];
#pragma unroll
          for (int q = 0; q < KS_CPT; ++q) {
            const double df = fma(-0.5, xc[q][d], -o);
            r0[q] = fma(df, df, r0[q]);
            be[q] = fma(z, df, be[q]);
          }
        }
#pragma unroll 1
        for (; r < r_end; ++r) {           // (the observation row: s = g = 0, r^2 = r0^2)
          // the row's five coefficients by scalar loads: the star path has no vector register to hold them in
          const int j = row0 + r;
          const double m2s = -2.0 * uniform_load(geo + j), g = uniform_load(geo + (size_t)N + j);
          double sv[KS_CPT], kv[KS_CPT];
#pragma unroll
          for (int q = 0; q < KS_CPT; ++q) sv[q] = fmax(fma(m2s, be[q], r0[q] + g), 0.0);
          finish_row(row0, r, sv, kv, uniform_load(alpha + j), has_lam ? uniform_load(lam_diag + j) : 0.0,
                     has_lam ? uniform_load(lam_off + j) : 0.0);
        }
      }
    }
  }
  // (the lane's first candidate once more, from an opaque lane index: nothing of the epilogue's addresses is carried
  // through the row loops)
  int tide = threadIdx.x;
  asm volatile("" : "+v"(tide));
  const int ce = (blockIdx.x * KS_THREADS + tide) * KS_CPT;
#pragma unroll
  for (int q = 0; q < KS_CPT; ++q) {
    if (ce + q < M) {
      // A candidate with a NaN or infinite coordinate leaves as NaN partial sums (score_kernel then gives the row NaN
      // results): the pair loop clips r^2 with fmax, which drops a NaN, so its sums are those of a row on top of every
      // design row or infinitely far from all of them.  |c|^2 says so where it is formed; the other forms look at the
      // coordinates once more here, after the pair loop, where the registers are free
      bool finite;
      if (EXPAND) finite = s_nc[q * KS_THREADS + threadIdx.x] < INFINITY;
      else {
        double chk = 0.0;
        for (int d = 0; d < D; ++d) chk = fma(Xc[(size_t)(ce + q) * D + d], 0.0, chk);
        finite = chk == 0.0;
      }
      mu_part[(size_t)blockIdx.y * M + ce + q] = finite ? mu[q] : NAN;
      if (t_part) t_part[(size_t)blockIdx.y * M + ce + q] = finite ? tl[q] : NAN;
      if constexpr (UB) u_part[(size_t)blockIdx.y * M + ce + q] = finite ? s_up[q * KS_THREADS + threadIdx.x] : NAN;
    }
  }
}

// Pass 1 of ppbo_predict_pairs: the column of a DUEL, d = k(a, X) - k(b, X), in place of k*.  One lane = ONE pair, its two
// points in the registers kstar_kernel gives its two candidates (two pairs per lane would spill in the DP = 64 bucket).
// Both points meet each staged design row in the same instruction chain (q = 0: a, q = 1: b; the expansion form, or the
// camphor feature form), so a == b gives ka == kb bit for bit and swapping the sides negates dv exactly.  Everything
// that kstar_kernel does with kv is done with dv = ka - kb: the mean sum, the star sums of d' Lambda d (ko = the
// observation row's dv) and the stored column in node or edge form -- all of them linear or quadratic in the column.
// fp64 only.  Launch geometry: kstar_kernel's row splits, KS_THREADS pairs per workgroup.
template <int KID, int DP>
__global__ __launch_bounds__(KS_THREADS) void kstar_pair_kernel(
    const double* __restrict__ X, int N, int D, KernParams p, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk,
    const double* __restrict__ Xa, const double* __restrict__ Xb, int M, double* __restrict__ Kt, int ldk,
    double* __restrict__ mu_part, double* __restrict__ t_part, int q_per_split, int n_q, int edge_k0) {
  static_assert(KID != PPBO_KERNEL_CAMPHOR || DP == 12, "camphor-copper: the feature form only");
  __shared__ __attribute__((aligned(16))) double xs[KS_RJ * DP];
  __shared__ double s_alpha[KS_RJ], s_ld[KS_RJ], s_lo[KS_RJ], s_nx[KS_RJ];
  constexpr bool CAMF = (KID == PPBO_KERNEL_CAMPHOR);     // see kstar_kernel for both forms
  const int c = blockIdx.x * KS_THREADS + threadIdx.x;
  const bool live = c < M;
  double xc[2][DP], nc[2];
  double mu = 0.0, tl = 0.0, ko = 0.0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double* __restrict__ src = (q == 0 ? Xa : Xb) + (size_t)(live ? c : 0) * D;
    nc[q] = 0.0;
    if constexpr (CAMF) {
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const double v = live ? src[k < 2 ? k : k + 1] : 0.0;
        double sn, cs;
        sincospi(2.0 * v, &sn, &cs);
        xc[q][k] = -0.5 * p.c0 * cs;
        xc[q][5 + k] = -0.5 * p.c0 * sn;
      }
      xc[q][10] = live ? src[2] : 0.0;
      xc[q][11] = 0.0;
    } else {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        double v = (d < D && live) ? src[d] : 0.0;
        nc[q] = fma(v, v, nc[q]);
        xc[q][d] = -2.0 * v;
      }
    }
  }
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool has_lam = (lam_diag != nullptr);
  int rb = 0;  // row index inside the current star block (splits start on a block edge)
  int qs = j_beg / mblk;  // ... and that block's star
  for (int row0 = j_beg; row0 < j_end; row0 += KS_RJ) {
    __syncthreads();
    if constexpr (CAMF) {
      for (int e = threadIdx.x; e < KS_RJ * 6; e += KS_THREADS) {
        const int r = e / 6, k = e - r * 6;
        const int j = row0 + r;
        if (k < 5) {
          const double v = (j < j_end) ? X[(size_t)j * D + (k < 2 ? k : k + 1)] : 0.0;
          double sn, cs;
          sincospi(2.0 * v, &sn, &cs);
          xs[r * DP + k] = cs;
          xs[r * DP + 5 + k] = sn;
        } else {
          xs[r * DP + 10] = (j < j_end) ? X[(size_t)j * D + 2] : 0.0;
          xs[r * DP + 11] = 0.0;
        }
      }
    } else {
      for (int e = threadIdx.x; e < KS_RJ * DP; e += KS_THREADS) {
        const int r = e / DP, d = e - r * DP;
        const int j = row0 + r;
        xs[e] = (j < j_end && d < D) ? X[(size_t)j * D + d] : 0.0;
      }
    }
    if (threadIdx.x < KS_RJ) {
      const int j = row0 + threadIdx.x;
      const bool ok = j < j_end;
      s_alpha[threadIdx.x] = ok ? alpha[j] : 0.0;
      s_ld[threadIdx.x] = (ok && has_lam) ? lam_diag[j] : 0.0;
      s_lo[threadIdx.x] = (ok && has_lam) ? lam_off[j] : 0.0;
      if (!CAMF) {
        double nx = 0.0;
        if (ok)
          for (int d = 0; d < D; ++d) { const double v = X[(size_t)j * D + d]; nx = fma(v, v, nx); }
        s_nx[threadIdx.x] = nx;
      }
    }
    __syncthreads();
    const int rmax = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
    for (int r = 0; r < rmax; ++r) {
      const double* __restrict__ xr = xs + r * DP;
      double sv[2] = {0.0, 0.0}, kv[2];
      if constexpr (CAMF) {
#pragma unroll
        for (int d = 0; d < 10; ++d) {
          const double x = xr[d];
#pragma unroll
          for (int q = 0; q < 2; ++q) sv[q] = fma(x, xc[q][d], sv[q]);
        }
        const double x2 = xr[10], base = 2.5 * p.c0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const double dd = x2 - xc[q][10];
          sv[q] = fma(p.c1 * dd, dd, sv[q] + base);
        }
      } else {
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double x = xr[d];
#pragma unroll
          for (int q = 0; q < 2; ++q) sv[q] = fma(x, xc[q][d], sv[q]);
        }
        const double nx = s_nx[r];
#pragma unroll
        for (int q = 0; q < 2; ++q) sv[q] = fmax(sv[q] + (nx + nc[q]), 0.0);
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) kv[q] = kern_finish<KID>(sv[q], p);
      // the two values as opaque registers: the subtraction must not be contracted with the product that ends
      // kern_finish (fma(sf2, ea, -(sf2 eb)) is not 0 when ea == eb)
      asm volatile("" : "+v"(kv[0]), "+v"(kv[1]));
      const double dv = kv[0] - kv[1];
      if (Kt) {
        // the layouts of kstar_kernel: node form row j, edge form row n_q + q m + t = lam_off[j] (d_j - d_obs)
        int drow = row0 + r;
        bool wr = true;
        double ev = dv;
        if (edge_k0 >= 0) {
          if (rb == 0) {
            drow = qs;
            wr = qs >= edge_k0;
            ev = 0.0;
          } else {
            drow = n_q + qs * (mblk - 1) + rb - 1;
            ev = s_lo[r] * (dv - ko);
          }
        }
        if (wr && live) store_through(Kt + (size_t)drow * ldk + c, ev);
      }
      mu += s_alpha[r] * dv;
      if (has_lam) {
        const double ld = s_ld[r];
        if (rb == 0) { ko = dv; tl += ld * dv * dv; }
        else tl += dv * (ld * dv + 2.0 * s_lo[r] * ko);
      }
      if (++rb == mblk) { rb = 0; ++qs; }
    }
  }
  if (live) {
    // a non-finite coordinate in either point: NaN partial sums (kstar_kernel; the fmax above drops a NaN)
    bool finite;
    if constexpr (CAMF) {
      double chk = 0.0;
      for (int d = 0; d < D; ++d) chk = fma(Xb[(size_t)c * D + d], 0.0, fma(Xa[(size_t)c * D + d], 0.0, chk));
      finite = chk == 0.0;
    } else {
      finite = (nc[0] + nc[1]) < INFINITY;
    }
    mu_part[(size_t)blockIdx.y * M + c] = finite ? mu : NAN;
    if (t_part) t_part[(size_t)blockIdx.y * M + c] = finite ? tl : NAN;
  }
}

// Pass 1 of ppbo_predict_functionals: the column of a LINEAR FUNCTIONAL L f = sum_g w_g f(x_g) over a group of G points,
// c_j = sum_g w_g k(x_g, x_j), in place of k*.  G points of up to 64 coordinates do not fit one lane's registers, so the
// radial kernels form their kernel values on the matrix cores (path_half's lane layout, pathwise.hip): a wavefront owns
// 16 groups, the workgroup's four wavefronts 64, and all walk the design rows of their row split in staged slabs of
// KF_RJ = 32.  Per slab the A fragments of its two 16-row tiles (design rows x dimensions, from LDS) stay in registers;
// for g = 0 .. G - 1 in order the B fragment is the g-th point of the wavefront's 16 groups (read from global memory:
// DP / 4 loads per lane, |x_g|^2 by two lane exchanges), v_mfma_f64_16x16x4_f64 with the accumulator started at
// -|x_j|^2 / 2 gives x_j.x_g - |x_j|^2 / 2, r^2 = max(|x_g|^2 - 2 (that), 0) -- kstar_pair_kernel's expansion form --
// then kern_finish and col = fma(w_g, k, col).  Register r of lane (lr, lk) is row lk + 4 r of group lr for every g, so
// the column accumulates in place with no lane movement, and every g takes the same instruction chain: two identical
// points of a group get the same bits, -w negates the column bit for bit and 2 w doubles it.
// The tail is kstar_pair_kernel's, on the finished slab: the mean sum, the star sums of c' Lambda c and the node- or
// edge-form store to Kt in that kernel's layouts and row splits.  Each lane keeps the rows it already holds (four
// consecutive rows x 16 groups = 128-byte pieces per store instruction); only ko, the value of the row's observation
// row, comes from elsewhere: every wavefront posts its slab of the column in a private LDS tile whose slot 0 carries the
// last observation row of the slabs before (a row split starts on a star's edge, so the slot is written before it is
// read).  Sums: each lane adds its rows in index order, the four row phases lk of a group meet by two exchanges in a
// fixed order; no atomics, so a call is bitwise repeatable and a group's results do not depend on its place in the call.
// A group with a non-finite coordinate leaves as NaN partial sums whatever its weights.  fp64 only.
constexpr int KF_RJ = 32;        // design rows per slab (two MFMA row tiles)
constexpr int KF_GROUPS = 64;    // groups per workgroup (16 per wavefront)
template <int KID, int DP>
__global__ __launch_bounds__(256) void kstar_func_kernel(
    const double* __restrict__ X, int N, int D, KernParams p, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk,
    const double* __restrict__ Xg, const double* __restrict__ W, int w_stride, int G, int M, double* __restrict__ Kt,
    int ldk, double* __restrict__ mu_part, double* __restrict__ t_part, int q_per_split, int n_q, int edge_k0) {
  static_assert(kid_radial<KID> && DP % 4 == 0, "radial kernels, whole k-steps of 4");
  constexpr int Q = DP / 4, LD = DP + 2, T = KF_RJ / 16, LC = 17;
  __shared__ __attribute__((aligned(16))) double ws[KF_RJ * LD];
  __shared__ double s_h[KF_RJ], s_alpha[KF_RJ], s_ld[KF_RJ], s_lo[KF_RJ];
  __shared__ double colS[4][KF_RJ + 1][LC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int c = blockIdx.x * KF_GROUPS + wv * 16 + lr;
  const bool live = c < M;
  const double* __restrict__ xg0 = Xg + (size_t)(live ? c : 0) * G * D;
  const double* __restrict__ wp = W + (size_t)(live ? c : 0) * w_stride;
  double mu = 0.0, tl = 0.0, chk = 0.0;
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool has_lam = (lam_diag != nullptr);
  for (int row0 = j_beg; row0 < j_end; row0 += KF_RJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < KF_RJ * DP; e += 256) {
      const int r = e / DP, d = e - r * DP;
      const int j = row0 + r;
      ws[r * LD + d] = (j < j_end && d < D) ? X[(size_t)j * D + d] : 0.0;
    }
    if (threadIdx.x < KF_RJ) {
      const int j = row0 + threadIdx.x;
      const bool ok = j < j_end;
      s_alpha[threadIdx.x] = ok ? alpha[j] : 0.0;
      s_ld[threadIdx.x] = (ok && has_lam) ? lam_diag[j] : 0.0;
      s_lo[threadIdx.x] = (ok && has_lam) ? lam_off[j] : 0.0;
      double nx = 0.0;
      if (ok)
        for (int d = 0; d < D; ++d) { const double v = X[(size_t)j * D + d]; nx = fma(v, v, nx); }
      s_h[threadIdx.x] = -0.5 * nx;
    }
    __syncthreads();
    double af[T][Q], hr[T][4];
    double4_t col[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int kk = 0; kk < Q; ++kk) af[t][kk] = ws[(16 * t + lr) * LD + kk * 4 + lk];
#pragma unroll
      for (int r = 0; r < 4; ++r) hr[t][r] = s_h[16 * t + lk + 4 * r];
      col[t] = double4_t{0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      double xb[Q], xn = 0.0;
#pragma unroll
      for (int kk = 0; kk < Q; ++kk) {
        const int d = kk * 4 + lk;
        xb[kk] = (d < D && live) ? xg0[(size_t)g * D + d] : 0.0;
        xn = fma(xb[kk], xb[kk], xn);
      }
      // |x_g|^2: the four lanes (lr, 0..3) hold the coordinates of group lr's point between them
      xn += __shfl_xor(xn, 16, 64);
      xn += __shfl_xor(xn, 32, 64);
      chk = fma(xn, 0.0, chk);             // NaN once a coordinate is not finite
      const double wg = live ? wp[g] : 0.0;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        double4_t ph = double4_t{hr[t][0], hr[t][1], hr[t][2], hr[t][3]};
#pragma unroll
        for (int kk = 0; kk < Q; ++kk) ph = __builtin_amdgcn_mfma_f64_16x16x4f64(af[t][kk], xb[kk], ph, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double kv = kern_finish<KID>(fmax(fma(-2.0, ph[r], xn), 0.0), p);
          // an opaque register: the product that ends kern_finish must not be contracted into the accumulation
          // (kstar_pair_kernel)
          asm volatile("" : "+v"(kv));
          col[t][r] = fma(wg, kv, col[t][r]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) colS[wv][1 + 16 * t + lk + 4 * r][lr] = col[t][r];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jr = 16 * t + lk + 4 * r, j = row0 + jr;
        if (j >= j_end) continue;
        const int qs = j / mblk, rb = j - qs * mblk;     // the row's star and its index inside it
        const double dv = col[t][r];
        const int jo = jr - rb;                          // the star's observation row: in this slab, or carried in slot 0
        const double ko = colS[wv][jo >= 0 ? jo + 1 : 0][lr];
        if (Kt) {
          // the layouts of kstar_kernel: node form row j, edge form row n_q + q m + t = lam_off[j] (c_j - c_obs)
          int drow = j;
          bool wr = true;
          double ev = dv;
          if (edge_k0 >= 0) {
            if (rb == 0) {
              drow = qs;
              wr = qs >= edge_k0;
              ev = 0.0;
            } else {
              drow = n_q + qs * (mblk - 1) + rb - 1;
              ev = s_lo[jr] * (dv - ko);
            }
          }
          if (wr && live) store_through(Kt + (size_t)drow * ldk + c, ev);
        }
        mu += s_alpha[jr] * dv;
        if (has_lam) {
          const double ld = s_ld[jr];
          if (rb == 0) tl += ld * dv * dv;
          else tl += dv * (ld * dv + 2.0 * s_lo[jr] * ko);
        }
      }
    __syncthreads();
    {
      // carry the slab's last observation row (if it holds one) into slot 0 for the slabs that follow
      const int j_hi = (row0 + KF_RJ < j_end ? row0 + KF_RJ : j_end) - 1;
      const int j_obs = (j_hi / mblk) * mblk;
      if (j_obs >= row0 && lk == 0) colS[wv][0][lr] = colS[wv][j_obs - row0 + 1][lr];
    }
  }
  mu += __shfl_xor(mu, 16, 64);
  mu += __shfl_xor(mu, 32, 64);
  tl += __shfl_xor(tl, 16, 64);
  tl += __shfl_xor(tl, 32, 64);
  if (live && lk == 0) {
    const bool finite = chk == 0.0;
    mu_part[(size_t)blockIdx.y * M + c] = finite ? mu : NAN;
    if (t_part) t_part[(size_t)blockIdx.y * M + c] = finite ? tl : NAN;
  }
}

// The camphor-copper instance of that pass: a plain vector kernel in kstar_pair_kernel's feature form (the kernel's
// exponent is no squared distance of the raw coordinates).  One lane = ONE group; per staged slab of KS_RJ rows the
// lane walks its G points in order -- the twelve feature values of a point formed from its six coordinates each time,
// ten sincospi per (point, slab) against 32 rows x 12 FMAs + 32 exponentials -- and accumulates col[r] = fma(w_g, k, col[r])
// in registers; then kstar_pair_kernel's sequential tail, one lane per group.
__global__ __launch_bounds__(KS_THREADS) void kstar_func_camphor_kernel(
    const double* __restrict__ X, int N, int D, KernParams p, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk,
    const double* __restrict__ Xg, const double* __restrict__ W, int w_stride, int G, int M, double* __restrict__ Kt,
    int ldk, double* __restrict__ mu_part, double* __restrict__ t_part, int q_per_split, int n_q, int edge_k0) {
  constexpr int KID = PPBO_KERNEL_CAMPHOR, DP = 12;
  __shared__ __attribute__((aligned(16))) double xs[KS_RJ * DP];
  __shared__ double s_alpha[KS_RJ], s_ld[KS_RJ], s_lo[KS_RJ];
  const int c = blockIdx.x * KS_THREADS + threadIdx.x;
  const bool live = c < M;
  const double* __restrict__ xg0 = Xg + (size_t)(live ? c : 0) * G * D;
  const double* __restrict__ wp = W + (size_t)(live ? c : 0) * w_stride;
  double mu = 0.0, tl = 0.0, ko = 0.0;
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool has_lam = (lam_diag != nullptr);
  int rb = 0, qs = j_beg / mblk;
  for (int row0 = j_beg; row0 < j_end; row0 += KS_RJ) {
    __syncthreads();
    for (int e = threadIdx.x; e < KS_RJ * 6; e += KS_THREADS) {
      const int r = e / 6, k = e - r * 6;
      const int j = row0 + r;
      if (k < 5) {
        const double v = (j < j_end) ? X[(size_t)j * D + (k < 2 ? k : k + 1)] : 0.0;
        double sn, cs;
        sincospi(2.0 * v, &sn, &cs);
        xs[r * DP + k] = cs;
        xs[r * DP + 5 + k] = sn;
      } else {
        xs[r * DP + 10] = (j < j_end) ? X[(size_t)j * D + 2] : 0.0;
        xs[r * DP + 11] = 0.0;
      }
    }
    if (threadIdx.x < KS_RJ) {
      const int j = row0 + threadIdx.x;
      const bool ok = j < j_end;
      s_alpha[threadIdx.x] = ok ? alpha[j] : 0.0;
      s_ld[threadIdx.x] = (ok && has_lam) ? lam_diag[j] : 0.0;
      s_lo[threadIdx.x] = (ok && has_lam) ? lam_off[j] : 0.0;
    }
    __syncthreads();
    double col[KS_RJ];
#pragma unroll
    for (int r = 0; r < KS_RJ; ++r) col[r] = 0.0;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      const double* __restrict__ src = xg0 + (size_t)g * D;
      double xc[11];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const double v = live ? src[k < 2 ? k : k + 1] : 0.0;
        double sn, cs;
        sincospi(2.0 * v, &sn, &cs);
        xc[k] = -0.5 * p.c0 * cs;
        xc[5 + k] = -0.5 * p.c0 * sn;
      }
      xc[10] = live ? src[2] : 0.0;
      const double wg = live ? wp[g] : 0.0;
      const double base = 2.5 * p.c0;
#pragma unroll
      for (int r = 0; r < KS_RJ; ++r) {
        const double* __restrict__ xr = xs + r * DP;
        double sv = 0.0;
#pragma unroll
        for (int d = 0; d < 10; ++d) sv = fma(xr[d], xc[d], sv);
        const double dd = xr[10] - xc[10];
        sv = fma(p.c1 * dd, dd, sv + base);
        double kv = kern_finish<KID>(sv, p);
        asm volatile("" : "+v"(kv));
        col[r] = fma(wg, kv, col[r]);
      }
    }
    const int rmax = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
#pragma unroll
    for (int r = 0; r < KS_RJ; ++r) {
      if (r < rmax) {
        const double dv = col[r];
        if (Kt) {
          int drow = row0 + r;
          bool wr = true;
          double ev = dv;
          if (edge_k0 >= 0) {
            if (rb == 0) {
              drow = qs;
              wr = qs >= edge_k0;
              ev = 0.0;
            } else {
              drow = n_q + qs * (mblk - 1) + rb - 1;
              ev = s_lo[r] * (dv - ko);
            }
          }
          if (wr && live) store_through(Kt + (size_t)drow * ldk + c, ev);
        }
        mu += s_alpha[r] * dv;
        if (has_lam) {
          const double ld = s_ld[r];
          if (rb == 0) { ko = dv; tl += ld * dv * dv; }
          else tl += dv * (ld * dv + 2.0 * s_lo[r] * ko);
        }
        if (++rb == mblk) { rb = 0; ++qs; }
      }
    }
  }
  if (live) {
    double chk = 0.0;
    for (int e = 0; e < G * D; ++e) chk = fma(xg0[e], 0.0, chk);
    const bool finite = chk == 0.0;
    mu_part[(size_t)blockIdx.y * M + c] = finite ? mu : NAN;
    if (t_part) t_part[(size_t)blockIdx.y * M + c] = finite ? tl : NAN;
  }
}

// d k / d r^2 times 2: the c with grad_x k(x, x') = c (x - x') at r^2 = s, finite at s = 0 (SE / RQ: kern_grad_coef's forms
// on the value itself, Matern: matern_grad) -- never (dk/dr) / r
template <int KID>
__device__ __forceinline__ double kern_slope_coef(double s, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    return -2.0 * p.c0 * (p.sf2 * exp_nonpos(-p.c0 * s));
  } else if constexpr (KID == PPBO_KERNEL_RQ) {
    const double t = 1.0 + p.c0 * s;
    return -4.0 * p.c0 * p.sf2 / (t * t * t);
  } else {
    static_assert(kid_matern<KID>, "radial kernels only");
    return matern_grad<KID>(matern_ae<KID>(s, p), p);
  }
}

// Pass 1 of ppbo_predict_slopes: the column of a SLOPE, g_j = d/da k(x + a xi, x_j) at a = 0, in place of k*.  One lane
// = ONE (point, direction) row, x and xi in the registers kstar_pair_kernel gives its two points.
//   radial kernels: g_j = c(r_j^2) b_j with r_j^2 = |x - x_j|^2 and b_j = (x - x_j).xi from the DIRECT differences x - x_j
//     (an add and two FMAs per dimension: nothing cancels next to a design row, where g_j -> 0, and x == x_j gives 0
//     exactly) and c = kern_slope_coef: ONE kernel-function evaluation per design row;
//   camphor-copper: g_j = -k_j ds_j/da in kstar_kernel's feature form; s_j is its ten-term dot product, and
//     ds_j/da = sum_k (pi c0) xi_k sin(2 pi (x_k - x_jk)) + 2 c1 (x_2 - x_j2) xi_2 a second one on the same staged
//     (cos, sin)(2 pi x_jk), with the candidate-side coefficients (pi c0) xi_k (sin, -cos)(2 pi x_k).
// xi enters every row through ONE chain of FMAs whose terms are all linear in it (b_j, or ds_j/da), so -xi negates g_j
// bit for bit and xi = 0 gives g_j = 0.  Everything that kstar_pair_kernel does with dv is done with g: the mean sum,
// the star sums of g' Lambda g (ko = the observation row's g) and the stored column in node or edge form.  fp64 only.
// Launch geometry: kstar_kernel's row splits, KS_THREADS rows per workgroup.  Registers: two D-vectors per lane, as
// kstar_pair_kernel; no instance uses scratch (DP = 64: 256 VGPRs + 40-58 AGPRs, one wavefront per SIMD).  The buckets
// up to DP = 16 fit 128 VGPRs (four wavefronts per SIMD) unbound; at DP = 20 SE and RQ are held there (137 / 119
// unbound), the Matern kernels would spill three registers and keep their 137 (three wavefronts); the camphor instance
// (two 12-vectors and the two dot products' temporaries) is left unbound as well: held to 128 it spills.
template <int KID, int DP>
__global__ __launch_bounds__(KS_THREADS, (KID != PPBO_KERNEL_CAMPHOR && (DP < 20 || (DP == 20 && !kid_matern<KID>))) ? 4 : 1) void kstar_slope_kernel(
    const double* __restrict__ X, int N, int D, KernParams p, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk,
    const double* __restrict__ Xp, const double* __restrict__ Xi, int M, double* __restrict__ Kt, int ldk,
    double* __restrict__ mu_part, double* __restrict__ t_part, int q_per_split, int n_q, int edge_k0) {
  static_assert(KID != PPBO_KERNEL_CAMPHOR || DP == 12, "camphor-copper: the feature form only");
  __shared__ __attribute__((aligned(16))) double xs[KS_RJ * DP];
  __shared__ double s_alpha[KS_RJ], s_ld[KS_RJ], s_lo[KS_RJ];
  constexpr bool CAMF = (KID == PPBO_KERNEL_CAMPHOR);     // see kstar_kernel for the feature form
  const int c = blockIdx.x * KS_THREADS + threadIdx.x;
  const bool live = c < M;
  // xc: the point (camphor: its value features, as kstar_kernel's);  xw: the direction (camphor: the slope features)
  double xc[DP], xw[DP];
  double mu = 0.0, tl = 0.0, ko = 0.0;
  // a non-finite coordinate in the point or the direction, found where they are loaded (NaN partial sums at the end, as
  // kstar_kernel's; the flag rides through the row loop as a lane mask, the coordinates are not read a second time)
  double chk = 0.0;
  {
    const double* __restrict__ px = Xp + (size_t)(live ? c : 0) * D;
    const double* __restrict__ pw = Xi + (size_t)(live ? c : 0) * D;
    if constexpr (CAMF) {
      const double pc0 = 3.14159265358979323846 * p.c0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int d = k < 2 ? k : k + 1;
        const double v = live ? px[d] : 0.0, w = live ? pw[d] : 0.0;
        chk = fma(w, 0.0, fma(v, 0.0, chk));
        double sn, cs;
        sincospi(2.0 * v, &sn, &cs);
        xc[k] = -0.5 * p.c0 * cs;
        xc[5 + k] = -0.5 * p.c0 * sn;
        xw[k] = (pc0 * sn) * w;              // meets cos 2 pi x_jk
        xw[5 + k] = (-pc0 * cs) * w;         // meets sin 2 pi x_jk
      }
      xc[10] = live ? px[2] : 0.0;
      xc[11] = 0.0;
      xw[10] = (2.0 * p.c1) * (live ? pw[2] : 0.0);
      xw[11] = 0.0;
      chk = fma(xw[10], 0.0, fma(xc[10], 0.0, chk));
    } else {
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        xc[d] = (d < D && live) ? px[d] : 0.0;
        xw[d] = (d < D && live) ? pw[d] : 0.0;
        chk = fma(xw[d], 0.0, fma(xc[d], 0.0, chk));
      }
    }
  }
  const bool finite = chk == 0.0;
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool has_lam = (lam_diag != nullptr);
  int rb = 0;  // row index inside the current star block (splits start on a block edge)
  int qs = j_beg / mblk;  // ... and that block's star
  for (int row0 = j_beg; row0 < j_end; row0 += KS_RJ) {
    __syncthreads();
    if constexpr (CAMF) {
      for (int e = threadIdx.x; e < KS_RJ * 6; e += KS_THREADS) {
        const int r = e / 6, k = e - r * 6;
        const int j = row0 + r;
        if (k < 5) {
          const double v = (j < j_end) ? X[(size_t)j * D + (k < 2 ? k : k + 1)] : 0.0;
          double sn, cs;
          sincospi(2.0 * v, &sn, &cs);
          xs[r * DP + k] = cs;
          xs[r * DP + 5 + k] = sn;
        } else {
          xs[r * DP + 10] = (j < j_end) ? X[(size_t)j * D + 2] : 0.0;
          xs[r * DP + 11] = 0.0;
        }
      }
    } else {
      for (int e = threadIdx.x; e < KS_RJ * DP; e += KS_THREADS) {
        const int r = e / DP, d = e - r * DP;
        const int j = row0 + r;
        xs[e] = (j < j_end && d < D) ? X[(size_t)j * D + d] : 0.0;
      }
    }
    if (threadIdx.x < KS_RJ) {
      const int j = row0 + threadIdx.x;
      const bool ok = j < j_end;
      s_alpha[threadIdx.x] = ok ? alpha[j] : 0.0;
      s_ld[threadIdx.x] = (ok && has_lam) ? lam_diag[j] : 0.0;
      s_lo[threadIdx.x] = (ok && has_lam) ? lam_off[j] : 0.0;
    }
    __syncthreads();
    const int rmax = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
    for (int r = 0; r < rmax; ++r) {
      const double* __restrict__ xr = xs + r * DP;
      double sv = 0.0, bv = 0.0, cf;
      if constexpr (CAMF) {
#pragma unroll
        for (int d = 0; d < 10; ++d) {
          const double x = xr[d];
          sv = fma(x, xc[d], sv);
          bv = fma(x, xw[d], bv);
        }
        const double dd = xc[10] - xr[10];
        sv = fma(p.c1 * dd, dd, sv + 2.5 * p.c0);
        bv = fma(xw[10], dd, bv);                       // ds_j / da
        cf = -kern_finish<KID>(sv, p);
      } else {
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double df = xc[d] - xr[d];
          sv = fma(df, df, sv);
          bv = fma(df, xw[d], bv);                      // (x - x_j).xi
        }
        cf = kern_slope_coef<KID>(sv, p);
      }
      // the two factors as opaque registers: the product below is formed alone, whatever ends the coefficient's chain
      asm volatile("" : "+v"(cf), "+v"(bv));
      const double dv = cf * bv;
      if (Kt) {
        // the layouts of kstar_kernel: node form row j, edge form row n_q + q m + t = lam_off[j] (g_j - g_obs)
        int drow = row0 + r;
        bool wr = true;
        double ev = dv;
        if (edge_k0 >= 0) {
          if (rb == 0) {
            drow = qs;
            wr = qs >= edge_k0;
            ev = 0.0;
          } else {
            drow = n_q + qs * (mblk - 1) + rb - 1;
            ev = s_lo[r] * (dv - ko);
          }
        }
        if (wr && live) store_through(Kt + (size_t)drow * ldk + c, ev);
      }
      mu += s_alpha[r] * dv;
      if (has_lam) {
        const double ld = s_ld[r];
        if (rb == 0) { ko = dv; tl += ld * dv * dv; }
        else tl += dv * (ld * dv + 2.0 * s_lo[r] * ko);
      }
      if (++rb == mblk) { rb = 0; ++qs; }
    }
  }
  if (live) {
    mu_part[(size_t)blockIdx.y * M + c] = finite ? mu : NAN;
    if (t_part) t_part[(size_t)blockIdx.y * M + c] = finite ? tl : NAN;
  }
}

// Pass 1 of ppbo_predict_gradients: ALL D columns of a point's gradient, g_jd = d k(x, x_j) / d x_d =
// c(r_j^2) (x_d - x_jd), from ONE kern_slope_coef per (point, design row) -- the D coordinate slopes of the point share
// their coefficient, where kstar_slope_kernel on the rows (x, e_d) would evaluate it D times.  One lane = one point, its
// coordinates and its D running mean sums in registers (two D-vectors per lane, kstar_slope_kernel's budget); the
// workgroup is ONE wavefront of KG_PTS = 64 points.  The columns go to the node layout at column point D + d, so the 64 D
// values a wavefront forms for one design row are one contiguous segment of that workspace row.  A lane storing its own D
// values would scatter 8-byte pieces at a stride of D; instead the row's 64 x D tile is staged in LDS (row stride DP | 1
// doubles: odd, the lanes of a write land in different banks) and read back in segment order, so that every store
// instruction of the wavefront writes 512 contiguous bytes.  The kernel is store-bound by construction: D stores per
// kernel-function evaluation.  The mean partials of a row split leave through the same tile.
// x - x_j from direct differences (x on a design row gives g_j = 0 exactly).  A point with a non-finite coordinate is
// taken as the origin here (finite columns: nothing non-finite reaches the contractions behind this pass);
// grad_finish_kernel finds it again and gives it NaN results.  Launch geometry: kstar_slope_kernel's dimension buckets
// and row splits (whole stars per split).  fp64 only, no Lambda sums, no edge layout (edge_apply_kernel forms it).
// camphor-copper (D = 6): g_jd = -k_j ds_j / dx_d in the DIRECT-difference form, not kstar_slope_kernel's feature form: the
// exponent and the five sines come from sincospi(x_d - x_jd), one per periodic coordinate, so a coordinate that equals
// the design row's gives g_jd = 0 exactly and an entry of the mean keeps its digits relative to sum_j |g_jd alpha_j|
// (the feature form's sin a cos b - cos a sin b leaves 1e-16 of k_j there, which is all of an entry when a whole star
// shares that coordinate).  One exponential per design row for the six columns.
constexpr int KG_PTS = 64;
template <int KID, int DP>
__global__ __launch_bounds__(KG_PTS) void kstar_grad_kernel(const double* __restrict__ X, int N, int D, KernParams p,
                                                            const double* __restrict__ alpha, int mblk,
                                                            const double* __restrict__ Xp, int P, double* __restrict__ Kt,
                                                            int ldk, double* __restrict__ mu_part, int q_per_split) {
  static_assert(KID != PPBO_KERNEL_CAMPHOR || DP == 6, "camphor-copper: D = 6");
  constexpr int DS = DP | 1;
  __shared__ __attribute__((aligned(16))) double xs[KS_RJ * DP];
  __shared__ double s_alpha[KS_RJ];
  __shared__ double tile[KG_PTS * DS];
  const int lane = threadIdx.x;
  const int p0 = blockIdx.x * KG_PTS;
  const bool live = p0 + lane < P;
  double xc[DP], mu[DP];
  {
    const double* __restrict__ px = Xp + (size_t)(live ? p0 + lane : 0) * D;
    double chk = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      xc[d] = (d < D && live) ? px[d] : 0.0;
      chk = fma(xc[d], 0.0, chk);
      mu[d] = 0.0;
    }
    if (chk != 0.0) {
#pragma unroll
      for (int d = 0; d < DP; ++d) xc[d] = 0.0;
    }
  }
  // the segment of this workgroup in a workspace row: nseg values from column p0 D on; lane L reads back its elements
  // L, L + 64, ... (point pt, dimension dd: stepped without a division per element)
  const int npts = (P - p0 < KG_PTS) ? (P - p0) : KG_PTS;
  const int nseg = npts * D;
  const int q64 = KG_PTS / D, r64 = KG_PTS - q64 * D;
  const int pt0 = lane / D, dd0 = lane - pt0 * D;
  const size_t seg0 = (size_t)p0 * D;
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  for (int row0 = j_beg; row0 < j_end; row0 += KS_RJ) {
    __syncthreads();
    for (int e = lane; e < KS_RJ * DP; e += KG_PTS) {
      const int r = e / DP, d = e - r * DP;
      const int j = row0 + r;
      xs[e] = (j < j_end && d < D) ? X[(size_t)j * D + d] : 0.0;
    }
    if (lane < KS_RJ) s_alpha[lane] = (row0 + lane < j_end) ? alpha[row0 + lane] : 0.0;
    __syncthreads();
    const int rmax = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
    for (int r = 0; r < rmax; ++r) {
      const double* __restrict__ xr = xs + r * DP;
      const double a = s_alpha[r];
      if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
        // b_d = ds_j / dx_d from the direct differences D_d = x_d - x_jd: pi c0 sin(2 pi D_d) = 2 pi c0 sin(pi D_d) cos(pi D_d)
        // (d = 2: 2 c1 D_2), the exponent from the same sin(pi D_d); g_jd = -k_j b_d
        double bd[DP], sv = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double df = xc[d] - xr[d];
          if (d == 2) {
            sv = fma(p.c1 * df, df, sv);
            bd[d] = (2.0 * p.c1) * df;
          } else {
            double sn, cs;
            sincospi(df, &sn, &cs);
            sv = fma(p.c0 * sn, sn, sv);
            bd[d] = (6.28318530717958647692 * p.c0) * (sn * cs);
          }
        }
        double cf = -kern_finish<KID>(sv, p);
        asm volatile("" : "+v"(cf));
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double g = cf * bd[d];
          mu[d] += a * g;
          if (Kt) tile[lane * DS + d] = g;
        }
      } else {
        double sv = 0.0;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double df = xc[d] - xr[d];
          sv = fma(df, df, sv);
        }
        double cf = kern_slope_coef<KID>(sv, p);
        asm volatile("" : "+v"(cf));              // the coefficient as an opaque register: every g_jd is one product
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double g = cf * (xc[d] - xr[d]);
          mu[d] += a * g;
          if (Kt) tile[lane * DS + d] = g;
        }
      }
      if (Kt) {
        __syncthreads();
        double* __restrict__ dst = Kt + (size_t)(row0 + r) * ldk + seg0;
        int pt = pt0, dd = dd0;
        for (int e = lane; e < nseg; e += KG_PTS) {
          store_through(dst + e, tile[pt * DS + dd]);
          pt += q64;
          dd += r64;
          if (dd >= D) { dd -= D; ++pt; }
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < DP; ++d) tile[lane * DS + d] = mu[d];
  __syncthreads();
  {
    double* __restrict__ dst = mu_part + (size_t)blockIdx.y * P * D + seg0;
    int pt = pt0, dd = dd0;
    for (int e = lane; e < nseg; e += KG_PTS) {
      dst[e] = tile[pt * DS + dd];
      pt += q64;
      dd += r64;
      if (dd >= D) { dd -= D; ++pt; }
    }
  }
}

// The two coefficients of a CURVATURE column at r^2 = s: c = 2 dk/dr^2 (kern_slope_coef's value) and c' = 2 d^2k/d(r^2)^2,
// both finite at s = 0, from ONE kernel-function evaluation (SE: one exponential; RQ: one reciprocal; Matern-5/2: the
// exponential of matern_ae, c' = sf2 c0^4 e^-a / 6 -- never a quotient by r).  Matern-3/2 has no second coefficient: its
// c' ~ 1 / sqrt(s), the curvature of its sample paths has no finite variance, and ppbo_predict_curvatures refuses it.
struct CurvCoef { double c, cp; };
template <int KID>
__device__ __forceinline__ CurvCoef kern_curv_coef(double s, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    const double k = p.sf2 * exp_nonpos(-p.c0 * s);
    return CurvCoef{-2.0 * p.c0 * k, (2.0 * p.c0 * p.c0) * k};
  } else if constexpr (KID == PPBO_KERNEL_RQ) {
    const double r = 1.0 / (1.0 + p.c0 * s), r2 = r * r;
    return CurvCoef{(-4.0 * p.c0 * p.sf2) * (r2 * r), (12.0 * p.c0 * p.c0 * p.sf2) * (r2 * r2)};
  } else {
    static_assert(KID == PPBO_KERNEL_MATERN52, "SE, RQ and Matern-5/2 only");
    const MaternAE ae = matern_ae<KID>(s, p);
    const double c2 = p.c0 * p.c0;
    return CurvCoef{matern_grad<KID>(ae, p), (p.sf2 * c2 * c2 * (1.0 / 6.0)) * ae.e};
  }
}

// wavefronts per SIMD that kstar_curv_kernel is held to (its second launch bound), from the register table of
// profiles/r18_curvature.txt: 4 (128 VGPRs, no scratch) for the buckets up to DP = 16 without an acceleration, as
// kstar_slope_kernel at DP = 20 for SE and RQ (unbound 141 / 123; Matern-5/2 would spill 12 bytes per lane there and keeps
// its 141), and up to DP = 10 with an acceleration: held, DP = 12 with one spills 12 (SE) and 16 (Matern-5/2) bytes per
// lane, so it and everything larger, and the camphor instance (three 12-vectors), stay unbound
template <int KID, int DP, bool ACC>
constexpr int curv_waves() {
  if (KID == PPBO_KERNEL_CAMPHOR) return 1;
  if (ACC) return DP <= 10 ? 4 : 1;
  return (DP <= 16 || (DP == 20 && !kid_matern<KID>)) ? 4 : 1;
}

// Pass 1 of ppbo_predict_curvatures: the column of a CURVATURE, c_j = d^2/da^2 k(gamma(a), x_j) at a = 0 for a path with
// gamma(0) = x, gamma'(0) = xi, gamma''(0) = acc (ACC = false: a straight line, acc = 0), in place of k*.  One lane = ONE
// (x, xi[, acc]) row, on the plan of kstar_slope_kernel: its launch geometry, row splits, star bookkeeping, NaN flag
// and node / edge stores.
//   radial kernels: with s_j = |x - x_j|^2, b_j = (x - x_j).xi, n2 = |xi|^2 (formed once per lane, before the row loop),
//     c_j = 2 c'(s_j) b_j^2 + c(s_j) (n2 + (x - x_j).acc),     (c, c') = kern_curv_coef: ONE evaluation per design row;
//     the direct differences x - x_j feed two (ACC: three) FMA chains per dimension;
//   camphor-copper (feature form, k = sf2 e^-s): c_j = k_j ((ds_j/da)^2 - d^2 s_j/da^2); s_j and ds_j/da are the slope
//     kernel's two dot products, d^2 s_j/da^2 = sum_{d != 2} 2 pi^2 c0 xi_d^2 cos 2 pi (x_d - x_jd) + 2 c1 xi_2^2 a third
//     one on the same staged (cos, sin)(2 pi x_jk) with the candidate-side coefficients 2 pi^2 c0 xi_k^2 (cos, sin)(2 pi x_k).
//     No acceleration: the caller's coordinates are the model's.
// Every term is of even degree in xi: -xi leaves c_j bitwise unchanged, xi = 0 (acc = 0) gives c_j = 0, and for the
// radial kernels 2 xi gives 4 c_j exactly (b_j doubles, n2 quadruples, every product scales by a power of two).  fp64
// only.  Registers: two D-vectors per lane (ACC: three, instantiated for DP <= 16 only -- the 11-column embedding is the
// only source of an acceleration, and three 64-vectors do not fit the register file); no instance uses scratch.
template <int KID, int DP, bool ACC>
__global__ __launch_bounds__(KS_THREADS, (curv_waves<KID, DP, ACC>())) void kstar_curv_kernel(
    const double* __restrict__ X, int N, int D, KernParams p, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk,
    const double* __restrict__ Xp, const double* __restrict__ Xi, const double* __restrict__ Xa, int M,
    double* __restrict__ Kt, int ldk, double* __restrict__ mu_part, double* __restrict__ t_part, int q_per_split, int n_q,
    int edge_k0) {
  static_assert(KID != PPBO_KERNEL_CAMPHOR || (DP == 12 && !ACC), "camphor-copper: the feature form only, straight lines");
  static_assert(!ACC || DP <= 16, "an acceleration vector: the buckets up to 16 only");
  __shared__ __attribute__((aligned(16))) double xs[KS_RJ * DP];
  __shared__ double s_alpha[KS_RJ], s_ld[KS_RJ], s_lo[KS_RJ];
  constexpr bool CAMF = (KID == PPBO_KERNEL_CAMPHOR);     // see kstar_kernel for the feature form
  constexpr int DA = (ACC || CAMF) ? DP : 1;
  const int c = blockIdx.x * KS_THREADS + threadIdx.x;
  const bool live = c < M;
  // xc: the point (camphor: its value features);  xw: the direction (camphor: the slope features);  xa: the
  // acceleration (camphor: the features of d^2 s / da^2)
  double xc[DP], xw[DP];
  [[maybe_unused]] double xa[DA];
  double mu = 0.0, tl = 0.0, ko = 0.0;
  [[maybe_unused]] double n2 = 0.0;       // |xi|^2 (camphor: unused, its constant 2 c1 xi_2^2 sits in xa[10])
  double chk = 0.0;      // a non-finite coordinate, found where the row is loaded (kstar_slope_kernel)
  {
    const double* __restrict__ px = Xp + (size_t)(live ? c : 0) * D;
    const double* __restrict__ pw = Xi + (size_t)(live ? c : 0) * D;
    if constexpr (CAMF) {
      const double pc0 = 3.14159265358979323846 * p.c0;
      const double qc0 = 19.73920880217871723767 * p.c0;     // 2 pi^2 c0
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int d = k < 2 ? k : k + 1;
        const double v = live ? px[d] : 0.0, w = live ? pw[d] : 0.0;
        chk = fma(w, 0.0, fma(v, 0.0, chk));
        double sn, cs;
        sincospi(2.0 * v, &sn, &cs);
        xc[k] = -0.5 * p.c0 * cs;
        xc[5 + k] = -0.5 * p.c0 * sn;
        xw[k] = (pc0 * sn) * w;              // meets cos 2 pi x_jk
        xw[5 + k] = (-pc0 * cs) * w;         // meets sin 2 pi x_jk
        const double w2 = qc0 * (w * w);
        xa[k] = w2 * cs;                     // meets cos 2 pi x_jk
        xa[5 + k] = w2 * sn;                 // meets sin 2 pi x_jk
      }
      const double w2 = live ? pw[2] : 0.0;
      xc[10] = live ? px[2] : 0.0;
      xc[11] = 0.0;
      xw[10] = (2.0 * p.c1) * w2;
      xw[11] = 0.0;
      xa[10] = (2.0 * p.c1) * (w2 * w2);
      xa[11] = 0.0;
      chk = fma(xw[10], 0.0, fma(xc[10], 0.0, chk));
    } else {
      const double* __restrict__ pa = ACC ? Xa + (size_t)(live ? c : 0) * D : nullptr;
#pragma unroll
      for (int d = 0; d < DP; ++d) {
        xc[d] = (d < D && live) ? px[d] : 0.0;
        xw[d] = (d < D && live) ? pw[d] : 0.0;
        chk = fma(xw[d], 0.0, fma(xc[d], 0.0, chk));
        n2 = fma(xw[d], xw[d], n2);
        if constexpr (ACC) {
          xa[d] = (d < D && live) ? pa[d] : 0.0;
          chk = fma(xa[d], 0.0, chk);
        }
      }
    }
  }
  const bool finite = chk == 0.0;
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool has_lam = (lam_diag != nullptr);
  int rb = 0;  // row index inside the current star block (splits start on a block edge)
  int qs = j_beg / mblk;  // ... and that block's star
  for (int row0 = j_beg; row0 < j_end; row0 += KS_RJ) {
    __syncthreads();
    if constexpr (CAMF) {
      for (int e = threadIdx.x; e < KS_RJ * 6; e += KS_THREADS) {
        const int r = e / 6, k = e - r * 6;
        const int j = row0 + r;
        if (k < 5) {
          const double v = (j < j_end) ? X[(size_t)j * D + (k < 2 ? k : k + 1)] : 0.0;
          double sn, cs;
          sincospi(2.0 * v, &sn, &cs);
          xs[r * DP + k] = cs;
          xs[r * DP + 5 + k] = sn;
        } else {
          xs[r * DP + 10] = (j < j_end) ? X[(size_t)j * D + 2] : 0.0;
          xs[r * DP + 11] = 0.0;
        }
      }
    } else {
      for (int e = threadIdx.x; e < KS_RJ * DP; e += KS_THREADS) {
        const int r = e / DP, d = e - r * DP;
        const int j = row0 + r;
        xs[e] = (j < j_end && d < D) ? X[(size_t)j * D + d] : 0.0;
      }
    }
    if (threadIdx.x < KS_RJ) {
      const int j = row0 + threadIdx.x;
      const bool ok = j < j_end;
      s_alpha[threadIdx.x] = ok ? alpha[j] : 0.0;
      s_ld[threadIdx.x] = (ok && has_lam) ? lam_diag[j] : 0.0;
      s_lo[threadIdx.x] = (ok && has_lam) ? lam_off[j] : 0.0;
    }
    __syncthreads();
    const int rmax = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
    for (int r = 0; r < rmax; ++r) {
      const double* __restrict__ xr = xs + r * DP;
      double sv = 0.0, bv = 0.0, dv;
      if constexpr (CAMF) {
        double qv = 0.0;
#pragma unroll
        for (int d = 0; d < 10; ++d) {
          const double x = xr[d];
          sv = fma(x, xc[d], sv);
          bv = fma(x, xw[d], bv);
          qv = fma(x, xa[d], qv);
        }
        const double dd = xc[10] - xr[10];
        sv = fma(p.c1 * dd, dd, sv + 2.5 * p.c0);
        bv = fma(xw[10], dd, bv);                       // ds_j / da
        qv += xa[10];                                   // d^2 s_j / da^2
        dv = kern_finish<KID>(sv, p) * fma(bv, bv, -qv);
      } else {
        double av = n2;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
          const double df = xc[d] - xr[d];
          sv = fma(df, df, sv);
          bv = fma(df, xw[d], bv);                      // (x - x_j).xi
          if constexpr (ACC) av = fma(df, xa[d], av);   // n2 + (x - x_j).acc
        }
        const CurvCoef cc = kern_curv_coef<KID>(sv, p);
        dv = fma((2.0 * cc.cp) * bv, bv, cc.c * av);
      }
      if (Kt) {
        // the layouts of kstar_kernel: node form row j, edge form row n_q + q m + t = lam_off[j] (c_j - c_obs)
        int drow = row0 + r;
        bool wr = true;
        double ev = dv;
        if (edge_k0 >= 0) {
          if (rb == 0) {
            drow = qs;
            wr = qs >= edge_k0;
            ev = 0.0;
          } else {
            drow = n_q + qs * (mblk - 1) + rb - 1;
            ev = s_lo[r] * (dv - ko);
          }
        }
        if (wr && live) store_through(Kt + (size_t)drow * ldk + c, ev);
      }
      mu += s_alpha[r] * dv;
      if (has_lam) {
        const double ld = s_ld[r];
        if (rb == 0) { ko = dv; tl += ld * dv * dv; }
        else tl += dv * (ld * dv + 2.0 * s_lo[r] * ko);
      }
      if (++rb == mblk) { rb = 0; ++qs; }
    }
  }
  if (live) {
    mu_part[(size_t)blockIdx.y * M + c] = finite ? mu : NAN;
    if (t_part) t_part[(size_t)blockIdx.y * M + c] = finite ? tl : NAN;
  }
}

// ---- main effects and interactions (ppbo_predict_marginals) -----------------------------------------------------------
// A kernel that is a PRODUCT over the caller's coordinates, k(x, x') = sf2 prod_d kappa_d(x_d - x'_d) with kappa_d SE or the
// camphor kernel's periodic factor, integrates over the unit box in any subset of coordinates in closed form.  With
//   Q_jd = I_d(x_jd) = int_0^1 kappa_d(u - x_jd) du,   P_j = sf2 prod_d Q_jd,   r_d = kappa_d(t_d - x_jd) / Q_jd
// the column of f with every axis but the kept ones (at most two, at the values t) averaged out is c_j = P_j prod_kept r_d.
//
// The axes of a call by value (at most 1.6 KB of kernel arguments: nothing of the host's is read after the launch is
// enqueued, and a captured launch carries its own copy).
struct MargAxesArg {
  double l[MG_AXES], i0[MG_AXES], a[MG_AXES];
  unsigned long long periodic;     // bit d: axis d is periodic
  int Dc;
};
inline size_t marginal_table_doubles(int N, int Dc) { return (size_t)MG_ROWS + (size_t)N * Dc + N; }

// Once per call: the axis table (score.h; written by workgroup 0), 1 / Q[N, Dc] and P[N].  One lane per design row; P_j
// is the product in axis order.  The by-value arrays are read with compile-time indices only (a lane-dependent index
// into a by-value argument goes through scratch, see camphor_pick): lane d of a workgroup picks axis d by a chain of
// selects and leaves it in LDS, where the row loop reads it.
__global__ __launch_bounds__(256) void marginal_table_kernel(MargAxesArg ax, const double* __restrict__ Xu, int N, double sf2,
                                                             double* __restrict__ tab) {
  __shared__ double s_l[MG_AXES], s_i0[MG_AXES];
  __shared__ int s_per[MG_AXES];
  const int Dc = ax.Dc;
  if (threadIdx.x < MG_AXES) {
    const int d = threadIdx.x;
    double l = 1.0, i0 = 1.0, a = 1.0;
#pragma unroll
    for (int k = 0; k < MG_AXES; ++k)
      if (k == d) { l = ax.l[k]; i0 = ax.i0[k]; a = ax.a[k]; }
    const int per = (int)((ax.periodic >> d) & 1ull);
    s_l[d] = l; s_i0[d] = i0; s_per[d] = per;
    if (blockIdx.x == 0 && d < Dc) {
      tab[MG_COEF + d] = (per ? 2.0 : 0.5) / (l * l);
      tab[MG_PER + d] = per ? 1.0 : 0.0;
      tab[MG_I0 + d] = i0;
      tab[MG_L + d] = l;
      tab[MG_A + d] = a;
    }
  }
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  double* __restrict__ iq = tab + MG_ROWS;
  double P = sf2;
  for (int d = 0; d < Dc; ++d) {
    const double q = s_per[d] ? s_i0[d] : marginal_se_integral(Xu[(size_t)j * Dc + d], s_l[d]);
    iq[(size_t)j * Dc + d] = 1.0 / q;
    P *= q;
  }
  tab[MG_ROWS + (size_t)N * Dc + j] = P;
}

// Pass 1 of ppbo_predict_marginals: the column c_j = P_j F(r_d, r_e) in place of k*, on kstar_pair_kernel's plan: one lane =
// ONE row of the call, the design rows (in the caller's unit-box coordinates) and their 1 / Q rows staged per KS_RJ-row
// slab in LDS, its row splits, star bookkeeping and node / edge stores.  F = r_d r_e (RAW), r_d r_e - 1 (CENTRED),
// (r_d - 1)(r_e - 1) (INTERACTION); an axis that is not kept has r = 1.  Per entry at most two factor values -- a
// difference, sinpi on a periodic axis, the project's exp, a product with 1 / Q -- and no D-long distance.  The lanes of a
// wavefront carry different axes: each reads ITS column of the staged slab (an LDS address per lane; nothing is
// indexed in registers) and keeps its axes' two coefficients in registers.  Every row of the call takes the same
// instruction chain on its canonical form (marginal_row), so swapped axes give the same bits and a row's sums do not
// depend on its place in the call.  A row with a non-finite t on a kept axis, or one that breaks the entry's rules,
// leaves as NaN partial sums.  Dynamic LDS: 2 KS_RJ Dc doubles.
__global__ __launch_bounds__(KS_THREADS) void kstar_marginal_kernel(
    const double* __restrict__ Xu, int N, int Dc, const double* __restrict__ tab, const double* __restrict__ alpha,
    const double* __restrict__ lam_diag, const double* __restrict__ lam_off, int mblk, const int* __restrict__ dims,
    const double* __restrict__ T, int effect, int M, double* __restrict__ Kt, int ldk, double* __restrict__ mu_part,
    double* __restrict__ t_part, int q_per_split, int n_q, int edge_k0) {
  extern __shared__ double mg_lds[];
  __shared__ double s_P[KS_RJ], s_alpha[KS_RJ], s_ld[KS_RJ], s_lo[KS_RJ];
  double* __restrict__ xs = mg_lds;
  double* __restrict__ iqs = mg_lds + KS_RJ * Dc;
  const int c = blockIdx.x * KS_THREADS + threadIdx.x;
  const bool live = c < M;
  const MargRow row = marginal_row(dims, T, live ? c : 0, Dc, effect);
  const bool has_d = row.ok && row.lo >= 0, has_e = row.ok && row.hi >= 0;
  const int di = has_d ? row.lo : 0, ei = has_e ? row.hi : 0;      // (a column of the slab that exists, read or not)
  const double td = row.tlo, te = row.thi;
  const double cf_d = -tab[MG_COEF + di], cf_e = -tab[MG_COEF + ei];
  const bool per_d = tab[MG_PER + di] != 0.0, per_e = tab[MG_PER + ei] != 0.0;
  const bool finite = row.ok && fma(has_d ? td : 0.0, 0.0, (has_e ? te : 0.0) * 0.0) == 0.0;
  const double* __restrict__ tab_iq = tab + MG_ROWS;
  const double* __restrict__ tab_P = tab_iq + (size_t)N * Dc;
  double mu = 0.0, tl = 0.0, ko = 0.0;
  const int j_beg = blockIdx.y * q_per_split * mblk;
  int j_end = j_beg + q_per_split * mblk;
  if (j_end > N) j_end = N;
  const bool has_lam = (lam_diag != nullptr);
  int rb = 0;  // row index inside the current star block (splits start on a block edge)
  int qs = j_beg / mblk;  // ... and that block's star
  for (int row0 = j_beg; row0 < j_end; row0 += KS_RJ) {
    __syncthreads();
    const int rmax = (j_end - row0 < KS_RJ) ? (j_end - row0) : KS_RJ;
    for (int e = threadIdx.x; e < KS_RJ * Dc; e += KS_THREADS) {
      const bool ok = e < rmax * Dc;
      xs[e] = ok ? Xu[(size_t)row0 * Dc + e] : 0.0;
      iqs[e] = ok ? tab_iq[(size_t)row0 * Dc + e] : 0.0;
    }
    if (threadIdx.x < KS_RJ) {
      const int j = row0 + threadIdx.x;
      const bool ok = j < j_end;
      s_P[threadIdx.x] = ok ? tab_P[j] : 0.0;
      s_alpha[threadIdx.x] = ok ? alpha[j] : 0.0;
      s_ld[threadIdx.x] = (ok && has_lam) ? lam_diag[j] : 0.0;
      s_lo[threadIdx.x] = (ok && has_lam) ? lam_off[j] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < rmax; ++r) {
      double rd = 1.0, re = 1.0;
      if (has_d) {
        const double dx = td - xs[r * Dc + di];
        const double u = per_d ? sinpi(dx) : dx;
        rd = exp_nonpos(cf_d * (u * u)) * iqs[r * Dc + di];
      }
      if (has_e) {
        const double dx = te - xs[r * Dc + ei];
        const double u = per_e ? sinpi(dx) : dx;
        re = exp_nonpos(cf_e * (u * u)) * iqs[r * Dc + ei];
      }
      // the two ratios as opaque registers: F is formed from them alone, whichever branches produced them
      asm volatile("" : "+v"(rd), "+v"(re));
      double f;
      if (effect == PPBO_EFFECT_INTERACTION) f = (rd - 1.0) * (re - 1.0);
      else {
        f = rd * re;
        if (effect == PPBO_EFFECT_CENTRED) f -= 1.0;
      }
      const double dv = s_P[r] * f;
      if (Kt) {
        // the layouts of kstar_kernel: node form row j, edge form row n_q + q m + t = lam_off[j] (c_j - c_obs)
        int drow = row0 + r;
        bool wr = true;
        double ev = dv;
        if (edge_k0 >= 0) {
          if (rb == 0) {
            drow = qs;
            wr = qs >= edge_k0;
            ev = 0.0;
          } else {
            drow = n_q + qs * (mblk - 1) + rb - 1;
            ev = s_lo[r] * (dv - ko);
          }
        }
        if (wr && live) store_through(Kt + (size_t)drow * ldk + c, ev);
      }
      mu += s_alpha[r] * dv;
      if (has_lam) {
        const double ld = s_ld[r];
        if (rb == 0) { ko = dv; tl += ld * dv * dv; }
        else tl += dv * (ld * dv + 2.0 * s_lo[r] * ko);
      }
      if (++rb == mblk) { rb = 0; ++qs; }
    }
  }
  if (live) {
    mu_part[(size_t)blockIdx.y * M + c] = finite ? mu : NAN;
    if (t_part) t_part[(size_t)blockIdx.y * M + c] = finite ? tl : NAN;
  }
}

// Y = G K* ; slab[mt][c] = sum over the BM rows of tile mt of Y[i,c]^2
// EDGE: an edge-form operator (H lower triangular, zero in its first n_q rows and columns).  G and Kt then arrive offset
// by kshift = n_q rounded down to the chunk depth (G + kshift, Kt + kshift ldk): the K loop starts at 0 of the shifted
// operands, so the main loop is the node form's own code (a non-zero start in the loop cost 16 more bytes of spilled
// state per lane and ~5 % of the matrix-core rate)
// DENSE (FORM == QF_DENSE): the operand is a projected operator T = Q^T H (project.hip) -- ntm row tiles of a dense
// matrix in the edge column layout, shifted like the edge form's; every tile and every wavefront runs the full K range
// PLAN (the pruned search): the launch is one of a pair behind prune_select_kernel, and every workgroup first reads the
// chunk's plan by scalar loads.  plan_compact = 1: the compact launch -- Kt is the gathered workspace Kc, column j the
// compact position, M the survivor capacity; it runs when the plan is pruned, on the column tiles below n_surv.
// plan_compact = 0: today's launch over all candidates, which runs when the plan is not pruned.  A workgroup that does
// not run returns before it touches an operand.
constexpr int QF_NODE = 0, QF_EDGE = 1, QF_DENSE = 2;

// One column of a wavefront's TM accumulator tiles, squared and summed over the tiles' rows: each lane its own
// TM x 4 entries (tile i outermost, register r inside, from 0.0), then the butterfly over the four lane groups of the
// C/D layout (row = (lane >> 4) + 4 r, column = lane & 15).  Every lane returns the sum of column lane & 15.
// The tile kernel and the thin one both end in this function: a column's bits do not depend on which of them ran.
template <int TM>
__device__ __forceinline__ double col_square_sum(const double4_t (&a)[TM]) {
  // What `s = 0.0; s += a * a; ...` compiled to before the split, spelled out so that no instance can come out
  // differently: the compiler contracted the sum of the first two squares as fma(a00, a00, a01 a01) -- the ROUNDED product
  // is the second entry's -- and every later term as fma(a, a, s).
  double s = a[0][1] * a[0][1];
  s = __builtin_fma(a[0][0], a[0][0], s);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = (i == 0 ? 2 : 0); r < 4; ++r) s = __builtin_fma(a[i][r], a[i][r], s);
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  return s;
}

// ---- the thin contraction: a handful of survivors of a pruned chunk ------------------------------------------------------
// The compact launch of a chunk with n_surv survivors contracts ceil(n_surv / 128) column tiles of 128: with 2 survivors
// (the headline step) 4 workgroups run 16 wavefronts x 4 accumulator tiles over the whole K range on the matrix cores of
// 4 CUs, 126 of every 128 columns padding.  Here a wavefront owns ONE 16 x 16 tile of Y = G Kc over the whole K range:
// a workgroup takes a row tile mt and C::WN / C::TM groups of 16 columns, wavefront (cg, wm, i) the rows
// [mt BM + (wm TM + i) 16, + 16) of column group cg.  No operand is shared through LDS and no barrier stands in the K
// loop; two rounds of 4 k-steps are in flight per wavefront:
//   * Kc: a k-step's fragment is four whole 128-byte rows of the column group -- straight to registers (buffer loads
//     with a fixed per-lane offset, the K walk on the SALU);
//   * G: a fragment read straight from memory takes 32 bytes of 16 lines, and the lines of rows a power of two apart
//     evict each other before the next k-step returns to them (measured: 138 us at the headline shape against 70).
//     A round's 16 x 16 block is therefore fetched as whole lines (two 16-byte loads per lane) and turned into fragments
//     through a wavefront-private LDS image in gemm64's padded layout: the wavefront's own LDS accesses execute in
//     order, so the image needs neither a second buffer nor a barrier.
// Bit identity with the tile kernel, per output column:
//   * Y[r, c] is one chain of v_mfma_f64_16x16x4 over k = 0, 4, 8, ... of the shifted operands, as in gemm64::mainloop;
//   * the chain ends where the tile kernel's wavefront (wm) ends it: the whole range (dense form), the end of its TM 16
//     rows (edge form), nowhere in the zero frame;
//   * wavefronts i > 0 hand their tile to wavefront i = 0 through LDS, which forms col_square_sum over the TM tiles;
//     the WM partials are added in the order w = 0 .. WM-1.
// The host launches it only where the lean loop would run (every tile in bounds, K ranges whole chunks).
// THIN_MAX: the largest n_surv that takes it.  profiles/r27_thin_contraction.txt, section 2: at the headline operator
// (4 row tiles) the thin path is ahead by 127 - 158 us at every count from 2 up to the 2048 its grid can hold (a quarter
// of the capacity), and a second column group on a workgroup costs 47 us.  It reads the operator once per 32 columns
// where the tiles read it once per 128, which only a launch that leaves most of the part idle can afford: 256 keeps
// it to 8 workgroups per row tile, the range in which the tiles' grid (2 column tiles) cannot fill the part either.
constexpr int THIN_MAX = 256;

__device__ __forceinline__ double buffer_load1(const double* __restrict__ sbase, unsigned byte_off, int sbyte_off) {
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(sbase), 0, -1, 0x00020000);
  return __builtin_bit_cast(double, (u32x2)__builtin_amdgcn_raw_buffer_load_b64(r, (int)byte_off, sbyte_off, 0));
}
__device__ __forceinline__ double2 buffer_load2s(const double* __restrict__ sbase, unsigned byte_off, int sbyte_off) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(sbase), 0, -1, 0x00020000);
  return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, sbyte_off, 0));
}

template <class C>
struct Thin {
  static constexpr int NW = C::NT / 64;                 // wavefronts of the launch's workgroup
  static constexpr int NSUB = C::WM * C::TM;            // 16-row tiles of a row tile
  static constexpr int CG = C::WN / C::TM;              // column groups of a workgroup
  static constexpr int COLS = 16 * CG;
  static constexpr int IMG = 16 * KC_LD;                // a wavefront's LDS image: [16 rows][16 + 2], doubles
  static constexpr bool OK = (C::WN % C::TM == 0);      // (Cfg<2,2,4,4> has fewer wavefronts than 16-row tiles: tile path)
};

// One round of a thin chain: 4 k-steps from operands that are already in registers -- G's 16 x 16 block as whole lines in
// `raw` (lane -> row (lane >> 3) + 8 h, k 2 (lane & 7)), Kc's fragments in `b` -- and the loads of round `nxt` into the
// same registers.
__device__ __forceinline__ void thin_round(const double* __restrict__ A, int lda, const double* __restrict__ B, int ldb,
                                           int nxt, unsigned offA, unsigned offB, int wr, int rd, double2 (&raw)[2],
                                           double (&b)[4], double4_t& acc) {
  *reinterpret_cast<double2*>(&lds_dyn[wr]) = raw[0];
  *reinterpret_cast<double2*>(&lds_dyn[wr + 8 * KC_LD]) = raw[1];
  const double* pa = A + (size_t)nxt * BK;
  const double* pb = B + (size_t)nxt * BK * ldb;
  raw[0] = buffer_load2s(pa, offA, 0);
  raw[1] = buffer_load2s(pa, offA, 64 * lda);
  __builtin_amdgcn_wave_barrier();                     // (the image is the wavefront's own: program order is enough)
  double a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = lds_dyn[rd + 4 * j];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], b[j], acc, 0, 0, 0);
    b[j] = buffer_load1(pb, offB, j * 32 * ldb);
  }
  __builtin_amdgcn_wave_barrier();
}

template <class C, int FORM>
__device__ __forceinline__ void quadform_thin(const double* __restrict__ G, int N, const double* __restrict__ Kt, int ldk,
                                              int M, double* __restrict__ slab, int mt, int grp, int n_live, int n_rows,
                                              int kshift) {
  static_assert(FORM == QF_EDGE || FORM == QF_DENSE, "the pruned search contracts an edge-form or a projected operator");
  using T = Thin<C>;
  static_assert(T::IMG >= 256 && C::LDS_DOUBLES >= T::NW * T::IMG + T::CG * C::WM * 16, "images and hand-over fit the launch's LDS");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cg = wave / T::NSUB, sub = wave % T::NSUB, wm = sub / C::TM, ti = sub % C::TM;
  const int m0 = mt * C::BM, n0 = grp * T::COLS;
  // the K cut of the tile kernel's wavefront wm (quadform_kernel below)
  const int e = FORM == QF_DENSE ? N : m0 + C::BM;
  const int kend = (e < N ? e : N) - kshift;
  const int wrow_beg = m0 + wm * C::TM * 16;
  const int wk = FORM == QF_DENSE ? kend : wrow_beg >= n_rows ? 0 : wrow_beg + C::TM * 16 - kshift;
  const int kmax = (n0 + cg * 16 < n_live) ? (wk < kend ? wk : kend) : 0;   // (a column group beyond the survivors: nothing)
  const int img = wave * T::IMG;                       // this wavefront's image; its hand-over tile afterwards
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  if (kmax > 0) {
    const int nr = kmax / BK;                          // (K ranges are whole chunks on this path)
    const unsigned offA = (unsigned)((((sub * 16 + (lane >> 3)) * N) + (lane & 7) * 2) * 8);
    const unsigned offB = (unsigned)((((lane >> 4) * ldk) + cg * 16 + (lane & 15)) * 8);
    const int wr = img + (lane >> 3) * KC_LD + (lane & 7) * 2, rd = img + (lane & 15) * KC_LD + (lane >> 4);
    const double* A = G + (size_t)m0 * N;
    const double* B = Kt + n0;
    double2 raw0[2], raw1[2];
    double b0[4], b1[4];
    const int r1 = nr > 1 ? 1 : 0;
    raw0[0] = buffer_load2s(A, offA, 0);
    raw0[1] = buffer_load2s(A, offA, 64 * N);
    raw1[0] = buffer_load2s(A + (size_t)r1 * BK, offA, 0);
    raw1[1] = buffer_load2s(A + (size_t)r1 * BK, offA, 64 * N);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b0[j] = buffer_load1(B, offB, j * 32 * ldk);
      b1[j] = buffer_load1(B + (size_t)r1 * BK * ldk, offB, j * 32 * ldk);
    }
    int r = 0;
    // two rounds per turn, each refilling its registers for the round after next (the last rounds re-read the final
    // one: no branch in the body)
    for (; r + 2 <= nr; r += 2) {
      thin_round(A, N, B, ldk, r + 2 < nr ? r + 2 : nr - 1, offA, offB, wr, rd, raw0, b0, acc);
      thin_round(A, N, B, ldk, r + 3 < nr ? r + 3 : nr - 1, offA, offB, wr, rd, raw1, b1, acc);
    }
    if (r < nr) thin_round(A, N, B, ldk, nr - 1, offA, offB, wr, rd, raw0, b0, acc);
  }
  double* xch = lds_dyn + img;                         // [4][64]: the tile of a wavefront i > 0
  double* red = lds_dyn + T::NW * T::IMG;              // [CG][WM][16]
  if (ti != 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) xch[q * 64 + lane] = acc[q];
  }
  __syncthreads();
  if (ti == 0) {
    double4_t col[C::TM];
    col[0] = acc;
#pragma unroll
    for (int i = 1; i < C::TM; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) col[i][q] = xch[i * T::IMG + q * 64 + lane];
    const double s = col_square_sum<C::TM>(col);
    if (lane < 16) red[(cg * C::WM + wm) * 16 + lane] = s;
  }
  __syncthreads();
  if (threadIdx.x < T::COLS) {
    const int c = n0 + threadIdx.x;
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < C::WM; ++w) t += red[((threadIdx.x >> 4) * C::WM + w) * 16 + (threadIdx.x & 15)];
    if (c < n_live) slab[(size_t)mt * M + c] = t;
  }
}

// THIN (the compact launch of a pruned search, lean operands): a chunk with at most thin_max survivors is contracted by
// quadform_thin on the first ntm ceil(n_surv / COLS) workgroups of the grid; any other chunk by the tiles below.
template <class C, int MINW, bool ALWAYS_FAST, int FORM, bool PLAN = false, bool THIN = false>
__global__ __launch_bounds__(C::NT, MINW) void quadform_kernel(const double* __restrict__ G, int N,
                                                               const double* __restrict__ Kt, int ldk, int M,
                                                               int tri_block, double* __restrict__ slab, int ntm,
                                                               int ntn, int swizzle, int n_rows, int kshift,
                                                               const PrunePlan* __restrict__ plan = nullptr,
                                                               int plan_compact = 0, int thin_max = 0) {
  int n_live = M;                      // PLAN: the columns of this launch that anything reads
  (void)n_live;
  if constexpr (PLAN) {
    const int pruned = uniform_load_int(&plan->pruned);
    if ((pruned != 0) != (plan_compact != 0)) return;
    if (plan_compact) n_live = uniform_load_int(&plan->n_surv);
  }
  if constexpr (THIN) {
    static_assert(PLAN && ALWAYS_FAST && Thin<C>::OK, "the thin path: the compact launch on lean operands");
    const int ng = (n_live + Thin<C>::COLS - 1) / Thin<C>::COLS;
    if (n_live <= thin_max && ng * ntm <= (int)gridDim.x) {
      if ((int)blockIdx.x >= ng * ntm) return;
      quadform_thin<C, FORM>(G, N, Kt, ldk, M, slab, (int)blockIdx.x % ntm, (int)blockIdx.x / ntm, n_live, n_rows, kshift);
      return;
    }
  }
  int mt, nt;                          // the walk (XCD remap, candidate- or row-tile fastest, chunks): tile_walk.h
  ppbo_qf_tile(blockIdx.x, gridDim.x, swizzle, ntm, ntn, mt, nt);
  const int m0 = mt * C::BM, n0 = nt * C::BN;
  if constexpr (PLAN) {
    if (n0 >= n_live) return;
  }
  // G is zero right of the last star that reaches into this row tile; the K range ends there, rounded UP to the chunk
  // depth (g_build_kernel writes the zeros of every row explicitly, so the extra columns multiply zeros): every K
  // range is then a whole number of chunks whatever the star size -- m = 25, the reference's default, has 26-row stars
  // Edge form: the K range of a tile ends with the tile's rows, that of a wavefront with its 32 rows (both shifted)
  constexpr bool EDGE = (FORM == QF_EDGE);
  const int e = FORM == QF_DENSE ? N : EDGE ? m0 + C::BM : (((m0 + C::BM + tri_block - 1) / tri_block) * tri_block + BK - 1) & ~(BK - 1);
  const int kend = (e < N ? e : N) - kshift;
  double4_t acc[C::TM][C::TN];
  zero_acc<C>(acc);
  // rows of this wavefront end at m0 + (wm+1)*TM*16: G is zero beyond the end of their last star block
  const int wrow_beg = m0 + ((int)(threadIdx.x >> 6) / C::WN) * C::TM * 16;
  const int wrow_end = wrow_beg + C::TM * 16;
  // (a wavefront whose rows all lie in the zero frame below the real matrix multiplies nothing)
  const int wk = FORM == QF_DENSE ? kend : wrow_beg >= n_rows ? 0 : (EDGE ? wrow_end : ((wrow_end + tri_block - 1) / tri_block) * tri_block) - kshift;
  mainloop<C, KC, RC, ALWAYS_FAST>(G, N, Kt, ldk, N, M, m0, n0, 0, kend, acc, wk < kend ? wk : kend);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / C::WN, wn = wave % C::WN;
  double* red = lds_dyn;  // [WM][BN]; mainloop ended with a barrier
#pragma unroll
  for (int j = 0; j < C::TN; ++j) {
    double4_t col[C::TM];
#pragma unroll
    for (int i = 0; i < C::TM; ++i) col[i] = acc[i][j];
    const double s = col_square_sum<C::TM>(col);
    if (lane < 16) red[wm * C::BN + (wn * C::TN + j) * 16 + lane] = s;
  }
  __syncthreads();
  if (threadIdx.x < C::BN) {
    const int c = n0 + threadIdx.x;
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < C::WM; ++w) t += red[w * C::BN + threadIdx.x];
    if (c < M) slab[(size_t)mt * M + c] = t;
  }
}

// tile shapes tried on MI355X: variant id -> (WM, WN, TM, TN, min waves/SIMD)
using QF0 = Cfg<2, 2, 4, 4>;   // 4 waves of 64x64, 2 WG/CU -> 2 waves/SIMD
using QF1 = Cfg<2, 4, 4, 2>;   // 8 waves of 64x32, 2 WG/CU -> 4 waves/SIMD
using QF2 = Cfg<4, 2, 2, 4>;   // 8 waves of 32x64
using QF3 = Cfg<4, 4, 2, 2>;   // 16 waves of 32x32, 1 WG/CU -> 4 waves/SIMD
using QF4 = Cfg<4, 4, 2, 2>;   // same tile, 2 WG/CU -> 8 waves/SIMD (<= 64 VGPRs)
using QF5 = Cfg<8, 2, 2, 4>;   // 256 x 128 tile, 16 waves of 32x64, 1 WG/CU: K* re-read once per 256 G rows

// G [rows >= ntm BM][N] with row stride N, Kt [N][ldk]: `N` is the K extent AND G's row stride.  The lean (unguarded)
// loop runs when every tile is in bounds and every K range a whole number of chunks: N % 16 == 0, the row tiles
// backed by memory (g_rows >= ntm BM) and the candidate tiles too (ldk >= ntn BN; what the columns beyond Mc hold does
// not matter, each output column depends on its own K* column only and the slab is written for c < Mc).
// predict_passes pads its operands so that this always holds.
template <class C, int MINW>
int launch_quadform(ppbo_ctx* ctx, const double* G, int N, int g_rows, int n_rows, const double* Kt, int ldk, int Mc,
                    int mblk, double* slab, int edge_k0, bool dense, hipStream_t s, const PrunePlan* plan = nullptr,
                    int plan_compact = 0) {
  const size_t lds = C::LDS_DOUBLES * sizeof(double);
  const bool edge = edge_k0 >= 0;
  const int kshift = edge ? edge_k0 : 0;
  if (dense) {
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, true, QF_DENSE>, (int)lds);
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, false, QF_DENSE>, (int)lds);
  } else if (edge) {
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, true, QF_EDGE>, (int)lds);
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, false, QF_EDGE>, (int)lds);
  } else {
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, true, QF_NODE>, (int)lds);
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, false, QF_NODE>, (int)lds);
  }
  const int ntm = (g_rows + C::BM - 1) / C::BM, ntn = (Mc + C::BN - 1) / C::BN;
  const int grid = ntm * ntn;
  // PPBO_QF_ORDER; default: candidate-tile fastest in chunks of 128 tiles (514; measured best at N >= 2048:
  // profiles/r04_quadform_traffic_vs_order.txt), of 256 tiles up to N = 1024 (1026: the same 268 MB of K* per chunk as 128
  // tiles at N = 2048; round 6, interleaved on one box at C4: 0.899-0.903 against 0.891-0.894 of the MFMA peak)
  const int order = ctx->qf_order >= 0 ? ctx->qf_order : (N <= 1024 ? 1026 : 514);
  const int swz = ppbo_qf_swizzle(order, grid);
  // every tile in bounds, 16-byte aligned, and every K range a multiple of 16?
  const bool fast = (g_rows % C::BM == 0) && (ldk >= ntn * C::BN) && (N % BK == 0) && (ldk % 2 == 0) &&
                    ((reinterpret_cast<uintptr_t>(G) & 15) == 0) && ((reinterpret_cast<uintptr_t>(Kt) & 15) == 0);
  const double* Gs = G + kshift;
  const double* Ks = Kt + (size_t)kshift * ldk;
  if (plan) {                          // (edge or dense form only: predict_passes prunes no node-form model)
#define QF_PLAN(FAST, FORM)                                                                                          \
  do {                                                                                                               \
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, FAST, FORM, true>, (int)lds);                          \
    quadform_kernel<C, MINW, FAST, FORM, true><<<grid, C::NT, lds, s>>>(Gs, N, Ks, ldk, Mc, mblk, slab, ntm, ntn, swz, \
                                                                        n_rows, kshift, plan, plan_compact);         \
  } while (0)
    // the compact launch on lean operands carries the thin path (PPBO_PRUNE_THIN; its per-lane byte offsets are 32-bit)
    const int thin_max = ctx->prune_thin == 1 ? THIN_MAX : ctx->prune_thin;
    const bool thin = Thin<C>::OK && plan_compact && fast && thin_max > 0 &&
                      (size_t)C::BM * (size_t)N < ((size_t)1 << 28) && ldk < (1 << 20);
    if (thin) {
      if constexpr (Thin<C>::OK) {
#define QF_THIN(FORM)                                                                                                \
  do {                                                                                                               \
    ppbo_lds_limit(ctx, (const void*)quadform_kernel<C, MINW, true, FORM, true, true>, (int)lds);                    \
    quadform_kernel<C, MINW, true, FORM, true, true><<<grid, C::NT, lds, s>>>(Gs, N, Ks, ldk, Mc, mblk, slab, ntm, ntn, swz, \
                                                                              n_rows, kshift, plan, plan_compact, thin_max); \
  } while (0)
        if (dense) QF_THIN(QF_DENSE);
        else QF_THIN(QF_EDGE);
#undef QF_THIN
      }
    } else if (dense && fast) QF_PLAN(true, QF_DENSE);
    else if (dense) QF_PLAN(false, QF_DENSE);
    else if (fast) QF_PLAN(true, QF_EDGE);
    else QF_PLAN(false, QF_EDGE);
#undef QF_PLAN
    PPBO_LAUNCH_CHECK(ctx);
    return 0;
  }
  if (dense && fast) quadform_kernel<C, MINW, true, QF_DENSE><<<grid, C::NT, lds, s>>>(Gs, N, Ks, ldk, Mc, mblk, slab, ntm, ntn, swz, n_rows, kshift);
  else if (dense) quadform_kernel<C, MINW, false, QF_DENSE><<<grid, C::NT, lds, s>>>(Gs, N, Ks, ldk, Mc, mblk, slab, ntm, ntn, swz, n_rows, kshift);
  else if (edge && fast) quadform_kernel<C, MINW, true, QF_EDGE><<<grid, C::NT, lds, s>>>(Gs, N, Ks, ldk, Mc, mblk, slab, ntm, ntn, swz, n_rows, kshift);
  else if (edge) quadform_kernel<C, MINW, false, QF_EDGE><<<grid, C::NT, lds, s>>>(Gs, N, Ks, ldk, Mc, mblk, slab, ntm, ntn, swz, n_rows, kshift);
  else if (fast) quadform_kernel<C, MINW, true, QF_NODE><<<grid, C::NT, lds, s>>>(G, N, Kt, ldk, Mc, mblk, slab, ntm, ntn, swz, n_rows, 0);
  else quadform_kernel<C, MINW, false, QF_NODE><<<grid, C::NT, lds, s>>>(G, N, Kt, ldk, Mc, mblk, slab, ntm, ntn, swz, n_rows, 0);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

// ctx->qf_variant (PPBO_QF_VARIANT); default 4 since round 6: 16 wavefronts of 32x32, two workgroups per CU = 8 waves/SIMD.
// Rounds 1-5 shipped variant 2 (8 wavefronts of 32x64, 4 waves/SIMD: the winner of round 1's sweep, 58.1 against 54.7 TF, taken
// BEFORE the lean main loop); re-measured interleaved on one box in round 6: variant 4 3.74-3.75 ms against 3.78-3.79 at C3 (0.948
// against 0.938 of the MFMA peak), 0.979 against 0.996 ms at C4 (0.921 / 0.906), level at C5 -- with no vector instruction left in
// the loop to pay for, twice the wavefronts hide more of the LDS and barrier latency
int quadform_variant(const ppbo_ctx* ctx) { return ctx->qf_variant; }

// dense: G is a projected operator T (g_rows = n_rows = its padded row count, a multiple of 128) of an edge-form model
// (edge_k0 >= 0); the 256-row tile of variant 5 does not divide every such count, so variant 5 runs it as variant 4
int dispatch_quadform(ppbo_ctx* ctx, const double* G, int N, int g_rows, int n_rows, const double* Kt, int ldk, int Mc,
                      int mblk, double* slab, int edge_k0, hipStream_t s, bool dense = false,
                      const PrunePlan* plan = nullptr, int plan_compact = 0) {
  switch (quadform_variant(ctx)) {
    case 1: return launch_quadform<QF1, 4>(ctx, G, N, g_rows, n_rows, Kt, ldk, Mc, mblk, slab, edge_k0, dense, s, plan, plan_compact);
    case 2: return launch_quadform<QF2, 4>(ctx, G, N, g_rows, n_rows, Kt, ldk, Mc, mblk, slab, edge_k0, dense, s, plan, plan_compact);
    case 3: return launch_quadform<QF3, 4>(ctx, G, N, g_rows, n_rows, Kt, ldk, Mc, mblk, slab, edge_k0, dense, s, plan, plan_compact);
    case 5: if (!dense) return launch_quadform<QF5, 4>(ctx, G, N, g_rows, n_rows, Kt, ldk, Mc, mblk, slab, edge_k0, false, s, plan, plan_compact);
            [[fallthrough]];
    case 4: return launch_quadform<QF4, 8>(ctx, G, N, g_rows, n_rows, Kt, ldk, Mc, mblk, slab, edge_k0, dense, s, plan, plan_compact);
    default: return launch_quadform<QF0, 2>(ctx, G, N, g_rows, n_rows, Kt, ldk, Mc, mblk, slab, edge_k0, dense, s, plan, plan_compact);
  }
}

// Gp [rows_p][cols_p] = G [N][N] framed with zeros: the operand of the quadratic form when N is not a multiple of its
// row tile / chunk depth (every tile of the launch is then in bounds and takes the lean loop; 3 N^2 x 8 bytes moved
// once per call -- 20 us at N = 2080 against the ~1 ms the guarded loop costs per 65536 candidates)
__global__ __launch_bounds__(256) void pad_square_kernel(const double* __restrict__ G, int N, double* __restrict__ Gp,
                                                         int rows_p, int cols_p) {
  const int i = blockIdx.y;
  const int j = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (j >= cols_p) return;
  double2 v = {0.0, 0.0};
  if (i < N) {
    if (j < N) v.x = G[(size_t)i * N + j];
    if (j + 1 < N) v.y = G[(size_t)i * N + j + 1];
  }
  *reinterpret_cast<double2*>(Gp + (size_t)i * cols_p + j) = v;
}

// G of the model as the block-triangular products want it: rows up to a whole 128-row tile, columns up to the chunk
// depth, framed with zeros -- the model's own array when it already has that shape.  *Nk_out = its row stride = K extent.
// worth = false (few columns on the other side of the product: the copy would cost more than the guarded loop does):
// the model's own array, whatever its shape.
const double* padded_G(ppbo_ctx* ctx, const ppbo_model* model, int row_tile, bool worth, int* Nk_out, int* g_rows_out,
                       hipStream_t s) {
  const int N = model->N;
  const int Nk = (N + BK - 1) & ~(BK - 1);
  const int g_rows = ((N + row_tile - 1) / row_tile) * row_tile;
  *Nk_out = N; *g_rows_out = N;
  if (!worth || (g_rows == N && Nk == N && (reinterpret_cast<uintptr_t>(model->d_G) & 15) == 0)) return model->d_G;
  *Nk_out = Nk; *g_rows_out = g_rows;
  double* Gp = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_GPAD, (size_t)g_rows * Nk * sizeof(double));
  if (!Gp) return nullptr;
  pad_square_kernel<<<dim3((Nk / 2 + 255) / 256, g_rows), 256, 0, s>>>(model->d_G, N, Gp, g_rows, Nk);
  return Gp;
}

// Z = Lambda K*  (star-graph rows), Kt/Z are [N, M] with row stride ld
__global__ void lam_apply_kernel(const double* __restrict__ Kt, int ld, int N, int M, int mblk,
                                 const double* __restrict__ lam_diag, const double* __restrict__ lam_off,
                                 double* __restrict__ Z) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (c >= M) return;
  const int i = q * mblk;
  const double ko = Kt[(size_t)i * ld + c];
  double zo = lam_diag[i] * ko;
  for (int r = 1; r < mblk && i + r < N; ++r) {
    const int j = i + r;
    const double kj = Kt[(size_t)j * ld + c];
    const double lo = lam_off[j];
    Z[(size_t)j * ld + c] = lam_diag[j] * kj + lo * ko;
    zo += lo * kj;
  }
  Z[(size_t)i * ld + c] = zo;
}

// E = the edge-layout K* of an edge-form model from the node-layout one: row q < n_q is zero, row n_q + q m + t holds
// lam_off[j] (K*[j] - K*[obs_q]) for pseudo row j = q (m + 1) + 1 + t (kstar_kernel writes the same values in its epilogue)
__global__ __launch_bounds__(128) void edge_apply_kernel(const double* __restrict__ Kt, int ld, int M, int mblk, int n_q,
                                                         const double* __restrict__ lam_off, double* __restrict__ E) {
  const int c = blockIdx.x * 128 + threadIdx.x, r = blockIdx.y;
  if (c >= M) return;
  double v = 0.0;
  if (r >= n_q) {
    const int m = mblk - 1, q = (r - n_q) / m, obs = q * mblk, j = obs + 1 + (r - n_q - q * m);
    v = lam_off[j] * (Kt[(size_t)j * ld + c] - Kt[(size_t)obs * ld + c]);
  }
  E[(size_t)r * ld + c] = v;
}

// ---- tournaments (ppbo_predict_tournament): every a against every b ---------------------------------------------------
// The covariance is bilinear: cov(f(a), f(b)) = k(a, b) + k_a' u_b with u_b = (Lambda + M'M) k_b, M = G (node form) or
// H diag(w) D (edge form).  U [K rows][ldu] holds u_b for the Mb opponents in the row layout of a chunk's K* workspace:
//   node form   U = Lambda K*_B + G'(G K*_B)                                     (lam_apply_kernel, two GEMMs)
//   edge form   the K* pass stores e_a,j = lam_off[j] (k_a,j - k_a,obs) = w_j (k_a,obs - k_a,j) in row n_q + q m + t, so
//               k_a' Lambda k_b = sum_j e_a,j (k_b,obs - k_b,j) and U = H'(H E_B) + Delta_B, Delta_B,j = k_b,obs - k_b,j
//               (tournament_delta_kernel; the plain difference, not E_B / w: a zero edge weight is harmless)
// so that all Ma x Mb cross terms are ONE product K*_A' U on the fp64 matrix cores.

// Delta_B in the edge layout from the node-layout K*_B: rows [0, n_q) zero, row n_q + q m + t = K*[obs_q] - K*[q (m + 1) + 1 + t]
__global__ __launch_bounds__(128) void tournament_delta_kernel(const double* __restrict__ Kt, int ld, int M, int mblk, int n_q,
                                                               double* __restrict__ Dl) {
  const int c = blockIdx.x * 128 + threadIdx.x, r = blockIdx.y;
  if (c >= M) return;
  double v = 0.0;
  if (r >= n_q) {
    const int m = mblk - 1, q = (r - n_q) / m, obs = q * mblk, j = obs + 1 + (r - n_q - q * m);
    v = Kt[(size_t)obs * ld + c] - Kt[(size_t)j * ld + c];
  }
  Dl[(size_t)r * ld + c] = v;
}

// the smaller of two values, NaN if either is (fmin drops a NaN operand)
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a) ? a : ((b != b) ? b : fmin(a, b)); }

// tile shapes: candidates (a) x opponents (b)
using TQ_BIG = Cfg<4, 4, 2, 2>;     // 128 x 128, 16 wavefronts of 32 x 32 (the shape of the shipped quadform_kernel)
using TQ_SMALL = Cfg<4, 1, 2, 2>;   // 128 x 32, 4 wavefronts of 32 x 32: fields of up to 64 opponents, and camphor-copper
constexpr int TQ_DCH = 16;          // coordinates staged in LDS per step of the prior term

// One BM x BN tile of the tournament: rows = the chunk's candidates, columns = the opponents.  Both operands are stored
// [K][rows] (RC): the chunk's K* workspace and U, each offset to the first contracted row by the host, so the main loop
// is the one quadform_kernel drives, with a full K range for every tile (U is dense).  The accumulators then hold
// k_a' u_b in the MFMA C layout (column = lane & 15 = opponent, row = candidate): 16 consecutive opponents of one
// candidate sit in 16 consecutive lanes, so the rows of the row-major [Ma][Mb] outputs are written in 128-byte runs.
// Epilogue, in registers: the prior k(a, b) from direct differences (rows staged in LDS TQ_DCH coordinates at a time),
//   cov = k(a, b) + k_a' u_b,  var_d = var_a + var_b - 2 cov,  p = Phi((mu_a - mu_b) / sqrt(2 sigma^2 + max(var_d, 0)))
// and per candidate the sum and the minimum of p over the tile's opponents -> slab_sum / slab_min [b tile][Mc].  No
// atomics: lanes meet by shuffles, wavefronts in LDS, in a fixed order.  A NaN mean on either side (a non-finite
// coordinate) gives NaN cov and p; the minimum propagates NaN as the sum does.
template <class C, int KID, bool ALWAYS_FAST>
__global__ __launch_bounds__(C::NT, (C::NT == 1024) ? 4 : 2) void tournament_kernel(
    const double* __restrict__ Kt, int ldk, const double* __restrict__ U, int ldu, int kext, int Mc, int Mb,
    const double* __restrict__ Xa, const double* __restrict__ Xb, int D, KernParams p, double two_sigma2,
    const double* __restrict__ mu_a, const double* __restrict__ var_a, const double* __restrict__ mu_b,
    const double* __restrict__ var_b, double* __restrict__ cov_out, double* __restrict__ prob_out,
    double* __restrict__ slab_sum, double* __restrict__ slab_min, int ntb) {
  // opponent tile fastest: the workgroups that share a K* panel are neighbours
  const int bt = blockIdx.x % ntb, at = blockIdx.x / ntb;
  const int m0 = at * C::BM, n0 = bt * C::BN;
  double4_t acc[C::TM][C::TN];
  zero_acc<C>(acc);
  // (every column of either workspace up to its row stride is backed by memory: the strides are the bounds)
  mainloop<C, RC, RC, ALWAYS_FAST>(Kt, ldk, U, ldu, ldk, ldu, m0, n0, 0, kext, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / C::WN, wn = wave % C::WN;
  constexpr int XLD = TQ_DCH + 1;              // odd row stride: the 16 opponent rows of a read fall into distinct banks
  double* xa_s = lds_dyn;                      // [BM][XLD]; mainloop ended with a barrier
  double* xb_s = lds_dyn + C::BM * XLD;        // [BN][XLD]
  double* red = xb_s + C::BN * XLD;            // [2][WN][BM]
  static_assert((C::BM + C::BN) * XLD + 2 * C::WN * C::BM <= C::LDS_DOUBLES, "the epilogue's LDS fits the main loop's");
  const int arow = wm * C::TM * 16 + (lane >> 4);   // + 16 i + 4 r
  const int bcol = wn * C::TN * 16 + (lane & 15);   // + 16 j
  double sq[C::TM][C::TN][4];
#pragma unroll
  for (int i = 0; i < C::TM; ++i)
#pragma unroll
    for (int j = 0; j < C::TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sq[i][j][r] = 0.0;
  for (int d0 = 0; d0 < D; d0 += TQ_DCH) {
    const int dc = (D - d0) < TQ_DCH ? (D - d0) : TQ_DCH;
    for (int e = threadIdx.x; e < (C::BM + C::BN) * TQ_DCH; e += C::NT) {
      const int row = e / TQ_DCH, d = e % TQ_DCH;
      double v = 0.0;
      if (d < dc) {
        if (row < C::BM) {
          if (m0 + row < Mc) v = Xa[(size_t)(m0 + row) * D + d0 + d];
        } else if (n0 + row - C::BM < Mb) {
          v = Xb[(size_t)(n0 + row - C::BM) * D + d0 + d];
        }
      }
      lds_dyn[row * XLD + d] = v;
    }
    __syncthreads();
    for (int d = 0; d < dc; ++d) {
      double bv[C::TN];
#pragma unroll
      for (int j = 0; j < C::TN; ++j) bv[j] = xb_s[(bcol + 16 * j) * XLD + d];
#pragma unroll
      for (int i = 0; i < C::TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double av = xa_s[(arow + 16 * i + 4 * r) * XLD + d];
#pragma unroll
          for (int j = 0; j < C::TN; ++j) sq[i][j][r] += kern_term<KID>(av - bv[j], d0 + d, p);
        }
    }
    __syncthreads();
  }
  double mb[C::TN], vb[C::TN];
  bool bok[C::TN];
#pragma unroll
  for (int j = 0; j < C::TN; ++j) {
    const int b = n0 + bcol + 16 * j;
    bok[j] = b < Mb;
    mb[j] = bok[j] ? mu_b[b] : 0.0;
    vb[j] = bok[j] ? var_b[b] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < C::TM; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int al = arow + 16 * i + 4 * r, a = m0 + al;
      const bool aok = a < Mc;
      const double ma = aok ? mu_a[a] : 0.0, va = aok ? var_a[a] : 0.0;
      double rs = 0.0, rm = INFINITY;
#pragma unroll
      for (int j = 0; j < C::TN; ++j) {
        // Var[f(a) - f(b)] >= 0 bounds the covariance by the mean of the two variances: clipped there (a matter of the
        // last bits, for a ~ b), var_a + var_b - 2 cov is never negative and exactly 0 for a == b
        double cv = fmin(acc[i][j][r] + kern_finish<KID>(sq[i][j][r], p), 0.5 * (va + vb[j]));
        const double vd = va + vb[j] - 2.0 * cv, mud = ma - mb[j];
        const double den = sqrt(two_sigma2 + fmax(vd, 0.0));
        // den = 0 (no noise, no variance): the sign of mu_d decides, a tie is 1/2 (pair_score_kernel's rule)
        double pr = norm_cdf(den > 0.0 ? mud / den : (mud > 0.0 ? INFINITY : (mud < 0.0 ? -INFINITY : 0.0)));
        if (mud != mud) { cv = mud; pr = mud; }
        if (aok && bok[j]) {
          const size_t o = (size_t)a * Mb + (n0 + bcol + 16 * j);
          if (cov_out) cov_out[o] = cv;
          if (prob_out) prob_out[o] = pr;
          rs += pr;
          rm = nan_min(rm, pr);
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {        // the 16 lanes of a row of the MFMA layout hold the row's 16 opponents
        rs += __shfl_xor(rs, o, 64);
        rm = nan_min(rm, __shfl_xor(rm, o, 64));
      }
      if ((lane & 15) == 0) {
        red[wn * C::BM + al] = rs;
        red[(C::WN + wn) * C::BM + al] = rm;
      }
    }
  __syncthreads();
  if (threadIdx.x < C::BM) {
    const int a = m0 + threadIdx.x;
    double ts = 0.0, tm = INFINITY;
#pragma unroll
    for (int w = 0; w < C::WN; ++w) {
      ts += red[w * C::BM + threadIdx.x];
      tm = nan_min(tm, red[(C::WN + w) * C::BM + threadIdx.x]);
    }
    if (a < Mc) {
      slab_sum[(size_t)bt * Mc + a] = ts;
      slab_min[(size_t)bt * Mc + a] = tm;
    }
  }
}

// the per-tile partials in tile order -> the score of every candidate of the chunk and the per-workgroup bests that the
// one-workgroup argmax (argmax_final_kernel) merges; NaN never wins
__global__ __launch_bounds__(256) void tournament_finish_kernel(const double* __restrict__ slab_sum,
                                                                const double* __restrict__ slab_min, int ntb, int Mc, int Mb,
                                                                int kind, long long idx_base, double* __restrict__ score_out,
                                                                Best* __restrict__ blk_best) {
  __shared__ Best sh[4];
  const int c = blockIdx.x * 256 + threadIdx.x;
  Best b{0.0, -1};
  if (c < Mc) {
    double sc;
    if (kind == PPBO_TOURNAMENT_BORDA) {
      double t = 0.0;
      for (int k = 0; k < ntb; ++k) t += slab_sum[(size_t)k * Mc + c];
      sc = t / (double)Mb;
    } else {
      sc = INFINITY;
      for (int k = 0; k < ntb; ++k) sc = nan_min(sc, slab_min[(size_t)k * Mc + c]);
    }
    if (score_out) score_out[c] = sc;
    if (sc == sc) { b.val = sc; b.idx = idx_base + c; }
  }
  b = block_best(b, sh);
  if (threadIdx.x == 0 && blk_best) blk_best[blockIdx.x] = b;
}

template <class C, int KID>
int launch_tournament(ppbo_ctx* ctx, const double* Kt, int ldk, const double* U, int ldu, int kext, int Mc, int Mb,
                      const double* Xa, const double* Xb, int D, const KernParams& p, double two_sigma2, const double* mu_a,
                      const double* var_a, const double* mu_b, const double* var_b, double* cov_out, double* prob_out,
                      double* slab_sum, double* slab_min, hipStream_t s) {
  const size_t lds = C::LDS_DOUBLES * sizeof(double);
  ppbo_lds_limit(ctx, (const void*)tournament_kernel<C, KID, true>, (int)lds);
  ppbo_lds_limit(ctx, (const void*)tournament_kernel<C, KID, false>, (int)lds);
  const int nta = (Mc + C::BM - 1) / C::BM, ntb = (Mb + C::BN - 1) / C::BN;
  // every tile in bounds and 16-byte aligned, the K range a whole number of chunks?
  const bool fast = (ldk >= nta * C::BM) && (ldu >= ntb * C::BN) && (kext % BK == 0) && (ldk % 2 == 0) && (ldu % 2 == 0) &&
                    ((reinterpret_cast<uintptr_t>(Kt) & 15) == 0) && ((reinterpret_cast<uintptr_t>(U) & 15) == 0);
  if (fast)
    tournament_kernel<C, KID, true><<<nta * ntb, C::NT, lds, s>>>(Kt, ldk, U, ldu, kext, Mc, Mb, Xa, Xb, D, p, two_sigma2, mu_a,
                                                                  var_a, mu_b, var_b, cov_out, prob_out, slab_sum, slab_min, ntb);
  else
    tournament_kernel<C, KID, false><<<nta * ntb, C::NT, lds, s>>>(Kt, ldk, U, ldu, kext, Mc, Mb, Xa, Xb, D, p, two_sigma2, mu_a,
                                                                   var_a, mu_b, var_b, cov_out, prob_out, slab_sum, slab_min, ntb);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

// ---- shortlists (ppbo_search_batch): q greedy picks under the conditioned variance ------------------------------------
// Conditioning on "f(p_j) observed with noise tau^2" leaves the mean and subtracts a rank-one term from the variance:
//   c_j[c] = cov_{j-1}(c, p_j) = k(c, p_j) + k_c' u_{p_j} - sum_{i<j} V_i[c] V_i[p_j],   V_j = c_j / sqrt(var_j[p_j] + tau^2),
//   var_{j+1} = max(var_j - V_j^2, 0)
// (the pivoted-Cholesky / kriging-believer rule).  Per pick: batch_gather_kernel reads the device-resident record of the
// pick, the field pass of the tournament forms u_{p_j} for that ONE opponent, batch_ucol_kernel packs its column, and
// batch_step_kernel streams the candidates' K* workspace once.

// the pick's record (value, index as a double; (NaN, -1) = nothing left to pick) -> picks[j], the pick's row xp [D], the
// earlier columns at the pick vp[i] = V_i[p_j], and pv[0] = sqrt(var_j[p_j] + tau^2), 0 where that is not positive
__global__ __launch_bounds__(64) void batch_gather_kernel(const double* __restrict__ rec, const double* __restrict__ Xc, int D,
                                                          const double* __restrict__ var, const double* __restrict__ V,
                                                          long long M, int j, double noise_var, long long* __restrict__ picks,
                                                          double* __restrict__ xp, double* __restrict__ vp,
                                                          double* __restrict__ pv) {
  const long long pick = (long long)rec[1];
  const int t = threadIdx.x;
  if (t == 0) {
    picks[j] = pick;
    const double den = pick >= 0 ? var[pick] + noise_var : 0.0;
    pv[0] = den > 0.0 ? sqrt(den) : 0.0;
  }
  for (int d = t; d < D; d += 64) xp[d] = pick >= 0 ? Xc[(size_t)pick * D + d] : 0.0;
  for (int i = t; i < j; i += 64) vp[i] = pick >= 0 ? V[(size_t)i * M + pick] : 0.0;
}

// column 0 of the field's U [kext][ldu] as a dense vector: batch_step_kernel reads it through scalar loads
__global__ __launch_bounds__(256) void batch_ucol_kernel(const double* __restrict__ U, int ldu, int kext, double* __restrict__ uc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < kext) uc[i] = U[(size_t)i * ldu];
}

// One greedy step for BS_CAND candidates per workgroup, in score_kernel's geometry doubled along c: a lane owns two adjacent
// candidates, so every row of Ks [kext][ldk] is read by 16-byte loads in 1-KB runs along c; the K range is split into
// SC_WAVES contiguous pieces, one per wavefront (u is wave-uniform: scalar loads), BS_UNROLL rows in flight per lane; the
// wavefront sums meet in LDS and are added in wavefront order.  Wavefronts 0 and 1 then finish 64 candidates each: the prior
// k(c, p_j) from direct differences, the downdate with V_0 .. V_{j-1}, V_j[c] and var_{j+1}[c], the new score, and the
// workgroup's best over the candidates that are not picked yet (picks[0 .. j]); NaN never wins.  A pick of -1 (nothing
// left) leaves var alone.  A NaN variance (a non-finite coordinate) stays NaN: fmax would drop it.
// Ks is 16-byte aligned and ldk even and at least the grid's BS_CAND columns (the host checks): the columns past Mc are
// read (whatever they hold) and feed nothing.
constexpr int BS_CAND = 2 * SC_CAND, BS_UNROLL = 8;
static inline int batch_blocks(long long M) { return (int)((M + BS_CAND - 1) / BS_CAND); }
template <int KID>
__global__ __launch_bounds__(SC_THREADS) void batch_step_kernel(
    const double* __restrict__ Ks, int ldk, int kext, const double* __restrict__ uc, const double* __restrict__ Xc, int D,
    KernParams p, int Mc, long long c_beg, long long M, const double* __restrict__ mu, double* __restrict__ var,
    double* __restrict__ V, int j, const double* __restrict__ vp, const double* __restrict__ pv,
    const long long* __restrict__ picks, const double* __restrict__ xp, int kind, double mustar, Best* __restrict__ blk_best) {
  __shared__ double part[SC_WAVES][BS_CAND];
  __shared__ Best sh[2];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (picks[j] < 0) {                    // (uniform over the launch)
    if (threadIdx.x == 0) blk_best[blockIdx.x] = Best{0.0, -1};
    return;
  }
  const int per = (kext + SC_WAVES - 1) / SC_WAVES;
  const int k0 = wave * per, k1 = (k0 + per < kext) ? k0 + per : kext;
  const size_t ld2 = (size_t)(ldk >> 1);
  const double2_t* kp = reinterpret_cast<const double2_t*>(Ks + (size_t)k0 * ldk + (size_t)blockIdx.x * BS_CAND) + lane;
  double a0 = 0.0, a1 = 0.0;
  int k = k0;
  for (; k + BS_UNROLL <= k1; k += BS_UNROLL) {
    double2_t v[BS_UNROLL];
#pragma unroll
    for (int t = 0; t < BS_UNROLL; ++t) v[t] = __builtin_nontemporal_load(kp + (size_t)t * ld2);
#pragma unroll
    for (int t = 0; t < BS_UNROLL; ++t) {
      const double u = uniform_load(uc + k + t);
      a0 = fma(v[t].x, u, a0);
      a1 = fma(v[t].y, u, a1);
    }
    kp += (size_t)BS_UNROLL * ld2;
  }
  for (; k < k1; ++k) {
    const double2_t v = __builtin_nontemporal_load(kp);
    const double u = uniform_load(uc + k);
    a0 = fma(v.x, u, a0);
    a1 = fma(v.y, u, a1);
    kp += ld2;
  }
  part[wave][2 * lane] = a0;
  part[wave][2 * lane + 1] = a1;
  __syncthreads();
  if (wave < 2) {                        // the rest is two wavefronts' work, a candidate per lane
    Best b{0.0, -1};
    const int cl = wave * SC_CAND + lane, c = blockIdx.x * BS_CAND + cl;
    if (c < Mc) {
      double dot = 0.0;
#pragma unroll
      for (int w = 0; w < SC_WAVES; ++w) dot += part[w][cl];
      const long long g = c_beg + c;
      double sq = 0.0;
      for (int d = 0; d < D; ++d) sq += kern_term<KID>(Xc[(size_t)g * D + d] - uniform_load(xp + d), d, p);
      double cj = kern_finish<KID>(sq, p) + dot;
      for (int i = 0; i < j; ++i) cj -= V[(size_t)i * M + g] * uniform_load(vp + i);
      const double sd = uniform_load(pv);
      const double vj = sd > 0.0 ? cj / sd : 0.0;
      V[(size_t)j * M + g] = vj;
      const double dv = var[g] - vj * vj;
      const double vn = (dv == dv) ? fmax(dv, 0.0) : dv;
      var[g] = vn;
      bool taken = false;
      for (int i = 0; i <= j; ++i) taken = taken || (picks[i] == g);
      const double sc = score_value(mu[g], vn, kind, mustar);
      if (!taken && sc == sc) { b.val = sc; b.idx = g; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      Best other;
      other.val = __shfl_xor(b.val, o, 64);
      other.idx = __shfl_xor(b.idx, o, 64);
      b = best_merge(b, other);
    }
    if (lane == 0) sh[wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) blk_best[blockIdx.x] = best_merge(sh[0], sh[1]);
}

// prior block of one line: cov_b[g][h] = (1-s) k(x_g, x_h), diagonal (1-s) sf2 + s sf2  (gp_model.py:447)
template <int KID>
__global__ __launch_bounds__(256) void line_prior_kernel(const double* __restrict__ grid, int G, int D,
                                                         KernParams p, double shrink, double* __restrict__ cov) {
  const double* xg = grid + (size_t)blockIdx.x * G * D;
  double* c = cov + (size_t)blockIdx.x * G * G;
  if (KID == PPBO_KERNEL_CAMPHOR) {
    // feature form of the camphor exponent (see kstar_kernel): (cos, sin)(2 pi x_k) of the line's points once, then ten
    // FMAs per pair; the same chain of the same products for (g, h) and (h, g)
    __shared__ double ph[128 * 11];        // G <= 128 (line_acq_impl)
    for (int e = threadIdx.x; e < G * 6; e += blockDim.x) {
      const int g = e / 6, k = e - g * 6;
      if (k < 5) {
        double sn, cs;
        sincospi(2.0 * xg[g * D + (k < 2 ? k : k + 1)], &sn, &cs);
        ph[g * 11 + k] = cs;
        ph[g * 11 + 5 + k] = sn;
      } else {
        ph[g * 11 + 10] = xg[g * D + 2];
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < G * G; e += blockDim.x) {
      const int g = e / G, h = e - g * G;
      double dot = 0.0;
#pragma unroll
      for (int f = 0; f < 10; ++f) dot = fma(ph[g * 11 + f], ph[h * 11 + f], dot);
      const double dd = ph[g * 11 + 10] - ph[h * 11 + 10];
      const double s = fma(p.c1 * dd, dd, 0.5 * p.c0 * (5.0 - dot));
      c[e] = (g == h) ? ((1.0 - shrink) * p.sf2 + shrink * p.sf2) : (1.0 - shrink) * kern_finish<KID>(s, p);
    }
    return;
  }
  for (int e = threadIdx.x; e < G * G; e += blockDim.x) {
    const int g = e / G, h = e - g * G;
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += kern_term<KID>(xg[g * D + d] - xg[h * D + d], d, p);
    c[e] = (g == h) ? ((1.0 - shrink) * p.sf2 + shrink * p.sf2) : (1.0 - shrink) * kern_finish<KID>(s, p);
  }
}

// The data term of a line's G x G predictive covariance, C_b = K*_b' Lambda K*_b + Y_b' Y_b (Y = G K*; gp_model.py:447-450
// through the Woodbury form of DESIGN 2.4), for one line per workgroup and one slice of the N rows per blockIdx.y.
// Replaces lam_apply_kernel + two batched 128 x 128-tile GEMMs whose 70 x 70 outputs used 30 % of every tile
// (1.61 ms of the 4.6 ms of 512 lines x 70 points at N = 2048): the rows are streamed once, 32 at a time, through
// LDS (next chunk in registers while the current one is multiplied), Lambda is applied while a chunk is staged --
//   K*' Lambda K* = sum_j k_j b_j' + (its transpose) / 2,  b_j = lam_jj k_j + 2 lam_off,j k_obs(j)  (pseudo rows),
//                                                          b_obs = lam_obs k_obs,
// the ONE-SIDED form: a row's b needs only its own row and its star's observation row; the consumer symmetrises --
// and both products accumulate in the same NT16 x NT16 grid of 16 x 16 MFMA tiles.  out[blockIdx.y][b][G*G].
// tile t of the NT16 x NT16 grid in the order the wavefronts share them out: SYM walks the lower triangle (mt >= nt)
// only, row by row
template <int NT16, bool SYM>
struct LcTiles {
  static constexpr int N = SYM ? NT16 * (NT16 + 1) / 2 : NT16 * NT16;
  static constexpr int mt(int t) {
    if (!SYM) return t / NT16;
    int m = 0;
    while ((m + 1) * (m + 2) / 2 <= t) ++m;
    return m;
  }
  static constexpr int nt(int t) { return SYM ? t - mt(t) * (mt(t) + 1) / 2 : t % NT16; }
};

// the MFMAs of one k-step over the tiles W, W + 4, ... (compile-time recursion: the fragment indices are constants)
template <int NT16, bool SYM, int W, int I>
__device__ __forceinline__ void lc_mfma_k(const double (&fk)[NT16], const double (&fb)[NT16],
                                          double4_t (&acc)[(LcTiles<NT16, SYM>::N + 3) / 4]) {
  using T = LcTiles<NT16, SYM>;
  constexpr int tile = W + 4 * I;
  if constexpr (tile < T::N) {
    acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(fk[T::mt(tile)], fb[T::nt(tile)], acc[I], 0, 0, 0);
    lc_mfma_k<NT16, SYM, W, I + 1>(fk, fb, acc);
  }
}
template <int NT16, bool SYM, int W, int I>
__device__ __forceinline__ void lc_mfma_y(const double (&fy)[NT16], double4_t (&acc)[(LcTiles<NT16, SYM>::N + 3) / 4]) {
  using T = LcTiles<NT16, SYM>;
  constexpr int tile = W + 4 * I;
  if constexpr (tile < T::N) {
    acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(fy[T::mt(tile)], fy[T::nt(tile)], acc[I], 0, 0, 0);
    lc_mfma_y<NT16, SYM, W, I + 1>(fy, acc);
  }
}

// one 32-row chunk of line_cov_kernel for wavefront W: its tiles are W, W + 4, ... of the tile list
template <int NT16, bool SYM, int W, int LDC>
__device__ __forceinline__ void line_cov_mm(const double* Ks, const double* Bs, const double* Ys, int lk, int lr,
                                            double4_t (&accK)[(LcTiles<NT16, SYM>::N + 3) / 4],
                                            double4_t (&accY)[(LcTiles<NT16, SYM>::N + 3) / 4], int ksteps) {
#pragma unroll 1
  for (int kk = 0; kk < ksteps; ++kk) {     // not unrolled: 3 NT16 fragments per step are live, not 24 NT16
    const int ko = (4 * kk + lk) * LDC + lr;
    // this k-step's fragments of all NT16 column blocks, once: every tile of the wavefront draws on them
    double fk[NT16], fb[NT16], fy[NT16];
#pragma unroll
    for (int c = 0; c < NT16; ++c) { fk[c] = Ks[ko + 16 * c]; fb[c] = Bs[ko + 16 * c]; fy[c] = Ys[ko + 16 * c]; }
    lc_mfma_k<NT16, SYM, W, 0>(fk, fb, accK);
    lc_mfma_y<NT16, SYM, W, 0>(fy, accY);
  }
}

constexpr int LC_MAXROWS = 512;      // rows of one (line, slice) workgroup: their Lambda entries sit in LDS

// SYM (the host picks it for stars of up to 32 rows, with row slices that hold whole stars): a chunk is `cs` rows = as many
// WHOLE stars as fit 32 rows (one at m = 31 and at the reference's default m = 25, two at m = 15, ...; the rest of the 32
// staged rows are zeros and k-steps beyond them are not run), so Lambda K* is formed EXACTLY -- every observation row gets
// lam_obs k_obs + sum_j lam_off,j k_j from the staged chunk -- both products are symmetric and only the tiles of the
// lower triangle (15 of 25 at G = 70) are computed.  Not SYM: cs = 32 rows of anything, the one-sided form.
template <int NT16, bool SYM>
__global__ __launch_bounds__(256, (NT16 <= 5) ? 2 : 1) void line_cov_kernel(const double* __restrict__ Kt, const double* __restrict__ Y, int ld,
                                                          int N, int G, int mblk, const double* __restrict__ lam_diag,
                                                          const double* __restrict__ lam_off, int rows_per_split,
                                                          double* __restrict__ out, long long out_stride, int cs) {
  using TL = LcTiles<NT16, SYM>;
  constexpr int CH = 32, LDC = 16 * NT16 + 8, NTILE = TL::N, TPW = (NTILE + 3) / 4;
  constexpr int NQ = (CH * 16 * NT16 + 255) / 256;
  __shared__ __attribute__((aligned(16))) double Ks[CH * LDC], Bs[CH * LDC], Ys[CH * LDC];
  __shared__ double s_ld[LC_MAXROWS], s_lo[LC_MAXROWS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4;
  const int col0 = blockIdx.x * G;
  const int r_beg = blockIdx.y * rows_per_split;
  int r_end = r_beg + rows_per_split;
  if (r_end > N) r_end = N;
  // two accumulator sets (K*'B and Y'Y): consecutive MFMAs never share an accumulator (a dependent fp64 MFMA issues
  // every ~138 cycles, an independent one every 64)
  double4_t accK[TPW], accY[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) { accK[i] = double4_t{0.0, 0.0, 0.0, 0.0}; accY[i] = double4_t{0.0, 0.0, 0.0, 0.0}; }
  for (int e = t; e < CH * LDC; e += 256) { Ks[e] = 0.0; Bs[e] = 0.0; Ys[e] = 0.0; }    // the padding columns stay zero
  for (int i = t; i < r_end - r_beg; i += 256) { s_ld[i] = lam_diag[r_beg + i]; s_lo[i] = lam_off[r_beg + i]; }
  // element q of this thread inside a chunk: (row rq, column gq), fixed for the whole walk (no division per chunk)
  int rq[NQ], gq[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = t + 256 * q;
    rq[q] = e / G;
    gq[q] = e - rq[q] * G;
  }
  // A chunk is FETCHED by unconditional loads only (addresses clamped into the matrix, values masked when they are
  // staged): the first version computed lam * k inside per-element guards, which made every one of the NQ elements its
  // own memory round trip -- 9 dependent round trips per 32-row chunk, 1.0 ms for a pass that is 0.35 ms of MFMA work.
  double rk[NQ], ro[NQ], ry[NQ];
  auto fetch = [&](int row0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int j = row0 + rq[q];
      j = j < N ? j : N - 1;
      const int q0 = (j / mblk) * mblk;
      const size_t c = (size_t)col0 + gq[q];
      rk[q] = Kt[(size_t)j * ld + c];
      ro[q] = Kt[(size_t)q0 * ld + c];           // the star's observation row (L2: the same row for the whole star)
      ry[q] = Y[(size_t)j * ld + c];
    }
  };
  fetch(r_beg);
  const int ksteps = (cs + 3) >> 2;
  for (int row0 = r_beg; row0 < r_end; row0 += cs) {
    __syncthreads();                         // the previous chunk's operands are done with (and, first time, s_ld / s_lo are there)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int r = rq[q], j = row0 + r;
      if (r < CH) {
        const bool on = r < cs && j < r_end;
        const int jl = on ? j - r_beg : 0;
        const double kv = on ? rk[q] : 0.0;
        // Lambda row: lam_jj k_j + c lam_off,j k_obs (lam_off is 0 on observation rows); c = 2: the one-sided form,
        // c = 1 (SYM): the pseudo-observation rows of the exact product, the observation row follows below
        Ks[r * LDC + gq[q]] = kv;
        Bs[r * LDC + gq[q]] = on ? s_ld[jl] * kv + (SYM ? 1.0 : 2.0) * s_lo[jl] * ro[q] : 0.0;
        Ys[r * LDC + gq[q]] = on ? ry[q] : 0.0;
      }
    }
    __syncthreads();
    if (SYM) {
      // the chunk is whole stars, each led by its observation row o: B[o][g] += sum_r lam_off,o+r K[o+r][g] (m terms per
      // column; rows past the slice's end were staged as zeros and are not touched)
      if (t < 16 * NT16) {
        const int jl0 = row0 - r_beg;
        for (int o = 0; o < cs && row0 + o < r_end; o += mblk) {
          double sg = 0.0;
#pragma unroll 8
          for (int r = 1; r < mblk; ++r) sg += s_lo[jl0 + o + r] * Ks[(o + r) * LDC + t];
          Bs[o * LDC + t] += sg;
        }
      }
      __syncthreads();
    }
    if (row0 + cs < r_end) fetch(row0 + cs);
    // the tile list of a wavefront is a compile-time list (W + 4 i): a run-time tile index would turn the fragment
    // arrays into dynamically indexed registers (measured: 1.84 ms instead of 0.99)
    switch (wave) {
      case 0: line_cov_mm<NT16, SYM, 0, LDC>(Ks, Bs, Ys, lk, lr, accK, accY, ksteps); break;
      case 1: line_cov_mm<NT16, SYM, 1, LDC>(Ks, Bs, Ys, lk, lr, accK, accY, ksteps); break;
      case 2: line_cov_mm<NT16, SYM, 2, LDC>(Ks, Bs, Ys, lk, lr, accK, accY, ksteps); break;
      default: line_cov_mm<NT16, SYM, 3, LDC>(Ks, Bs, Ys, lk, lr, accK, accY, ksteps); break;
    }
  }
  double* o = out + (size_t)blockIdx.y * out_stride + (size_t)blockIdx.x * G * G;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int tile = wave + 4 * i;
    if (tile >= NTILE) continue;
    const int mt = TL::mt(tile), nt = TL::nt(tile);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int g = 16 * mt + lk + 4 * r, h = 16 * nt + lr;
      if (g < G && h < G) o[g * G + h] = accK[i][r] + accY[i][r];
    }
  }
}

// (MC_MAXG16 and mc_factor_lds, step 1 of the Monte-Carlo kernels below: mc_factor.h)

// Monte-Carlo part of EI / varmax on a line (acquisition.py:72-81, :170-178): f = mu + L z for S draws, max over the
// line, statistics of the maxima.  grid = (lines, draw splits); one workgroup = one line x one slice of the draws.
//   1. Cholesky of the G x G posterior covariance in LDS (every split of a line repeats it: 70 short steps, and the
//      splits run side by side);
//   2. F = Z L^T on the fp64 matrix cores: a wavefront takes 16 draws at a time (A fragments straight from the
//      shared z[S][G], which stays in L2), one 16 x 16 tile of F per 16 grid points with mu as the accumulator's
//      initial value and the contraction cut at the triangle's edge; the maximum over the line is an elementwise
//      max over the tiles and one 16-lane reduction;
//   3. partial sums (sum max(f - mustar, 0), sum f, sum f^2) per (line, split); mc_finish_kernel combines them.
// Round 1-2's form (lane = draw, a scalar loop over the triangle with z re-read from memory) took 1.3 ms for 1200
// draws of a 70-point line whatever the batch size; this one ~0.1 ms.
__global__ __launch_bounds__(256) void line_mc_kernel(const double* __restrict__ mu, const double* __restrict__ cov,
                                                      int G, const double* __restrict__ z, int S, double mustar,
                                                      double jitter, int draws_per_split, double* __restrict__ part,
                                                      const double* __restrict__ cov_parts = nullptr, int n_parts = 0,
                                                      long long part_stride = 0, int parts_lower_only = 0) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int G16 = (G + 15) & ~15, ld = G16 + 2;
  double* Lm = sm;                           // [G16][ld], rows / columns >= G zero
  double* mus = sm + (size_t)G16 * ld;       // [G16], -inf beyond G: a padded grid point never is the maximum
  double* red = mus + G16;                   // [3][4]
  mc_factor_lds(Lm, mus, mu, cov, G, G16, ld, jitter, cov_parts, n_parts, part_stride, parts_lower_only);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int s_beg = blockIdx.y * draws_per_split;
  int s_end = s_beg + draws_per_split;
  if (s_end > S) s_end = S;
  const int nj = G16 >> 4;
  double sum_ei = 0.0, sum_f = 0.0, sum_f2 = 0.0;
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
    double fmx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < MC_MAXG16 / 16; ++j) {                        // unrolled: the triangle's edge is a constant per j
      if (j >= nj) break;
      const double mg = mus[16 * j + lr];
      double4_t acc = double4_t{mg, mg, mg, mg};
      const double* lrow = Lm + (size_t)(16 * j + lr) * ld + lk;      // B operand: L^T[k][g] = L[g][k]
#pragma unroll
      for (int kk = 0; kk < 4 * (j + 1); ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(az[kk], lrow[4 * kk], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) fmx[r] = fmax(fmx[r], acc[r]);
    }
    // acc[r] belongs to draw s0 + lk + 4 r and grid point 16 j + lr: maximum over the 16 lanes that share lk
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = fmx[r];
      v = fmax(v, __shfl_xor(v, 1, 64));
      v = fmax(v, __shfl_xor(v, 2, 64));
      v = fmax(v, __shfl_xor(v, 4, 64));
      v = fmax(v, __shfl_xor(v, 8, 64));
      if (lr == 0 && s0 + lk + 4 * r < s_end) {
        sum_ei += fmax(v - mustar, 0.0);
        sum_f += v;
        sum_f2 += v * v;
      }
    }
  }
  sum_ei = wave_sum(sum_ei);
  sum_f = wave_sum(sum_f);
  sum_f2 = wave_sum(sum_f2);
  if (lane == 0) { red[wave] = sum_ei; red[4 + wave] = sum_f; red[8 + wave] = sum_f2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* r = red + 4 * threadIdx.x;
    part[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 3 + threadIdx.x] = r[0] + r[1] + r[2] + r[3];
  }
}

// EI and varmax of every line from the per-split partial sums (fixed order: deterministic)
__global__ __launch_bounds__(256) void mc_finish_kernel(const double* __restrict__ part, int B, int nsplit, int S,
                                                        double* __restrict__ ei, double* __restrict__ varmax) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double e = 0.0, f1 = 0.0, f2 = 0.0;
  for (int k = 0; k < nsplit; ++k) {
    const double* p = part + ((size_t)b * nsplit + k) * 3;
    e += p[0]; f1 += p[1]; f2 += p[2];
  }
  if (ei) ei[b] = e / S;
  const double mean = f1 / S;
  if (varmax) varmax[b] = f2 / S - mean * mean;
}

// The answer to a query: WHICH point of a group is the maximum of a draw, under the likelihood's noise (ppbo_line_choice).
// line_mc_kernel's plan -- the same grid, factor, A fragments and MFMA chains -- with the other half of the draw kept:
//   - the accumulator of (draw s, point g) starts at mu_g + noise_sd eps[s][g] (eps == NULL: at mu_g), so the chain
//     leaves u = mu + L z + noise_sd eps; a lane's four loads of eps per tile are 16 consecutive g of one draw each:
//     coalesced, and issued for all tiles before the first chain;
//   - every lane keeps (value, point) of its best u over the tiles: strict >, tiles ascending, so of equal values the
//     lower point stays and a NaN never enters; (-inf, -1) until something does -- a padded point (mu = -inf) never;
//   - one 16-lane reduction of the pair, equal values to the lower point, gives the draw's choice (-1: no value of the
//     draw was a number);
//   - a group whose mean holds a NaN (a point with a NaN coordinate: its row of the covariance is no number either, and
//     the factor would drop that point silently) chooses -1 in every draw;
//   - a chosen point counts one in hist[G16] by an integer LDS add: exact, whatever the order.
// A draw's row of F depends on no other row, so choice[s] does not depend on how the draws are cut into wavefronts,
// workgroups or splits, and the counts are sums of integers.  part[(group, split)][G] <- hist; choice_finish_kernel adds
// the splits.
__global__ __launch_bounds__(256) void line_choice_kernel(const double* __restrict__ mu, const double* __restrict__ cov,
                                                          int G, const double* __restrict__ z,
                                                          const double* __restrict__ eps, int S, double noise_sd,
                                                          double jitter, int draws_per_split, int* __restrict__ part,
                                                          int* __restrict__ choice, const double* __restrict__ cov_parts,
                                                          int n_parts, long long part_stride, int parts_lower_only) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int G16 = (G + 15) & ~15, ld = G16 + 2;
  double* Lm = sm;                           // [G16][ld]
  double* mus = sm + (size_t)G16 * ld;       // [G16]
  int* hist = (int*)(mus + G16);             // [G16]
  for (int g = threadIdx.x; g < G16; g += blockDim.x) hist[g] = 0;
  mc_factor_lds(Lm, mus, mu, cov, G, G16, ld, jitter, cov_parts, n_parts, part_stride, parts_lower_only);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int s_beg = blockIdx.y * draws_per_split;
  int s_end = s_beg + draws_per_split;
  if (s_end > S) s_end = S;
  const int nj = G16 >> 4;
  bool poisoned = false;                                              // every lane reads the same word: a broadcast
  for (int g = 0; g < G; ++g) poisoned |= mus[g] != mus[g];
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
    // the noise of this lane's (draw, point) pairs, all tiles at once: the loads are in flight under the first chains
    double ev[MC_MAXG16 / 16][4];
#pragma unroll
    for (int j = 0; j < MC_MAXG16 / 16; ++j) {
      if (j >= nj) break;
      const int g = 16 * j + lr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int sd = s0 + lk + 4 * r;
        ev[j][r] = (eps && g < G && sd < s_end) ? eps[(size_t)sd * G + g] : 0.0;
      }
    }
    double bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int bi[4] = {-1, -1, -1, -1};
#pragma unroll
    for (int j = 0; j < MC_MAXG16 / 16; ++j) {                        // unrolled: the triangle's edge is a constant per j
      if (j >= nj) break;
      const int g = 16 * j + lr;
      const double mg = mus[g];
      // acc[r] belongs to draw s0 + lk + 4 r and point g
      double4_t acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = mg + noise_sd * ev[j][r];     // no noise: + 0
      const double* lrow = Lm + (size_t)g * ld + lk;                  // B operand: L^T[k][g] = L[g][k]
#pragma unroll
      for (int kk = 0; kk < 4 * (j + 1); ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(az[kk], lrow[4 * kk], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (acc[r] > bv[r]) { bv[r] = acc[r]; bi[r] = g; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = bv[r];
      int i = bi[r];
#pragma unroll
      for (int msk = 1; msk < 16; msk <<= 1) {
        const double ov = __shfl_xor(v, msk, 64);
        const int oi = __shfl_xor(i, msk, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      if (poisoned) i = -1;
      const int sd = s0 + lk + 4 * r;
      if (lr == 0 && sd < s_end) {
        if (choice) choice[(size_t)blockIdx.x * S + sd] = i;
        if (i >= 0) atomicAdd(&hist[i], 1);
      }
    }
  }
  __syncthreads();
  int* o = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * G;
  for (int g = threadIdx.x; g < G; g += blockDim.x) o[g] = hist[g];
}

// prob = count / S and the counts themselves from the per-split histograms, added in split order
__global__ __launch_bounds__(256) void choice_finish_kernel(const int* __restrict__ part, int n, int G, int nsplit, int S,
                                                            double* __restrict__ prob, int* __restrict__ count) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;      // (group, point)
  if (e >= n) return;
  const int b = e / G, g = e - b * G;
  int c = 0;
  for (int k = 0; k < nsplit; ++k) c += part[((size_t)b * nsplit + k) * G + g];
  prob[e] = (double)c / (double)S;
  if (count) count[e] = c;
}

// Standard normal draws for the Monte-Carlo acquisitions, generated where they are used (4800 x 70 draws cost the host
// 3 ms -- as much as the whole search they feed).  Counter-based: Philox-4x32-10 (Salmon et al. 2011) keyed by the
// seed, counter = output pair index; two 53-bit uniforms per counter -> one Box-Muller pair.  The stream is a pure
// function of (seed, index): reproducible, independent of launch geometry.
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
  const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
  const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__global__ __launch_bounds__(256) void randn_kernel(unsigned long long seed, double* __restrict__ out, long long n) {
  const long long pair = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (2 * pair >= n) return;
  unsigned c[4] = {(unsigned)pair, (unsigned)((unsigned long long)pair >> 32), 0u, 0u};
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const unsigned long long a = ((unsigned long long)c[1] << 32) | c[0], b = ((unsigned long long)c[3] << 32) | c[2];
  const double u1 = ((double)(a >> 11) + 0.5) * 0x1.0p-53;       // (0, 1): the logarithm is finite
  const double u2 = ((double)(b >> 11) + 0.5) * 0x1.0p-53;
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  out[2 * pair] = rad * cs;
  if (2 * pair + 1 < n) out[2 * pair + 1] = rad * sn;
}

// Omega[s][f] = omega_MAP[f] + sqrt(cov_diag[f]) z[s][f] in place over the randn_kernel draws z (ppbo_rff_omega_draws);
// product and sum rounded separately (no contraction), as the host states them
__global__ __launch_bounds__(256) void omega_draws_kernel(const double* __restrict__ om, const double* __restrict__ cov,
                                                          int F, long long n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i % F);
  out[i] = __dadd_rn(om[f], __dmul_rn(sqrt(cov[f]), out[i]));
}

// The DP buckets of the K* kernels, named once: every launch_kstar* below dispatches through one of them.  The camphor-
// copper instances take a fixed DP instead (12 staged features per row, or its 6 dimensions).
using KstarLadder = DpLadder<4, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64>;
using KstarFuncLadder = DpLadder<8, 20, 32, 48, 64>;    // kstar_func_kernel: whole MFMA k-steps of 4 dimensions
using KstarFp32Ladder = DpLadder<6, 20, 64>;            // the fp32-tolerance report: the BASELINE shapes' buckets and a generic one
constexpr int KSTAR_CURV_ACC_MAX_DP = 16;               // kstar_curv_kernel's acceleration twins (ACC = true) exist up to here

// What every K* launcher takes, and what each derives from it; unpacked at the <<<>>> statement.
struct KstarLaunch {
  const ppbo_model* m;
  KernParams p;
  double* Kt;
  int ldk;
  double *mu_part, *t_part;
  int q_per_split, n_split;
  bool with_lam;
  int edge_k0;
  hipStream_t s;
  int mblk() const { return m->m + 1; }
  int n_q() const { return (m->N + mblk() - 1) / mblk(); }
  const double* lam_diag() const { return with_lam ? m->d_lam_diag : nullptr; }
  const double* lam_off() const { return with_lam ? m->d_lam_off : nullptr; }
  double* t_or_null() const { return with_lam ? t_part : nullptr; }
  dim3 grid(int cols, int per_wg) const { return dim3((cols + per_wg - 1) / per_wg, n_split); }   // per_wg columns per workgroup
};

template <int KID>
int launch_kstar(const KstarLaunch& k, const double* d_Xc, int M, const double* geo, const double* sig, double* u_part) {
  const ppbo_model* m = k.m;
  const dim3 grid = k.grid(M, KS_THREADS * KS_CPT);
  if (m->kstar_fp32) {
    auto launch32 = [&](auto dp) {
      kstar_kernel<KID, decltype(dp)::value, true><<<grid, KS_THREADS, 0, k.s>>>(
          m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_Xc, M, k.Kt, k.ldk, k.mu_part,
          k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0, nullptr);
    };
    if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch32(std::integral_constant<int, 6>{});     // (camphor-copper: D = 6)
    else KstarFp32Ladder::dispatch(m->D, launch32);
    return 0;
  }
  // (sig: the flagged instantiation, an edge-layout launch with Lambda and a K* store; predict_passes asks for no other)
  auto launch = [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    if (sig)
      kstar_kernel<KID, DP, false, true><<<grid, KS_THREADS, 0, k.s>>>(
          m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_Xc, M, k.Kt, k.ldk, k.mu_part, k.t_part,
          k.q_per_split, k.n_q(), k.edge_k0, geo, sig, u_part);
    else
      kstar_kernel<KID, DP><<<grid, KS_THREADS, 0, k.s>>>(
          m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_Xc, M, k.Kt, k.ldk, k.mu_part,
          k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0, geo);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 12>{});  // the feature form: 12 staged values per row
  else KstarLadder::dispatch(m->D, launch);
  return 0;
}

// edge_k0 >= 0: K* in the edge layout of an edge-form model (kstar_kernel), which needs with_lam
// geo: the model's star-geometry table (star_geometry), or NULL = one inner product per row
int dispatch_kstar(const ppbo_model* m, const double* d_Xc, int M, double* Kt, int ldk, double* mu_part,
                   double* t_part, int q_per_split, int n_split, bool with_lam, hipStream_t s, int edge_k0 = -1,
                   const double* geo = nullptr, const double* sig = nullptr, double* u_part = nullptr) {
  const KstarLaunch k{m, make_kern_params(m->kernel_id, m->theta), Kt, ldk, mu_part, t_part, q_per_split, n_split, with_lam,
                      edge_k0, s};
  // (no ctx: an unknown id returns -1 and sets no message; check_model rejects any such id first)
  return ppbo_kernel_dispatch(nullptr, m->kernel_id,
                              [&](auto kid) { return launch_kstar<decltype(kid)::value>(k, d_Xc, M, geo, sig, u_part); });
}

// star_geom_kernel on `s` into the ctx's table for this model: the operand `geo` of the K* launch enqueued behind it.
// Formed in front of EVERY K* launch, i.e. once per chunk of 65536 candidates (N D doubles read, ~10 microseconds):
// nothing is cached, so nothing can go stale when a model's rows are updated in place.  NULL (and no launch) where the K* launch has no star path: PPBO_KSTAR_STAR=0, the
// fp32 evaluation, camphor-copper.  *oom is set when the table could not be allocated
// (ppbo_workspace has left the message in ctx->err).
const double* star_geometry(ppbo_ctx* ctx, const ppbo_model* m, hipStream_t s, bool* oom) {
  *oom = false;
  if (!ctx->kstar_star || m->kstar_fp32 || m->kernel_id == PPBO_KERNEL_CAMPHOR) return nullptr;
  const int mblk = m->m + 1, n_q = m->N / mblk;
  double* geo = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_KSTAR_GEO, star_geo_doubles(m->N, n_q, m->D) * sizeof(double));
  if (!geo) { *oom = true; return nullptr; }
  star_geom_kernel<<<(n_q + SG_STARS - 1) / SG_STARS, 64 * SG_STARS, 0, s>>>(m->d_X, m->N, m->D, mblk, n_q, geo);
  return geo;
}

// kstar_pair_kernel in launch_kstar's D buckets (fp64 only); n_split rows splits as there, KS_THREADS pairs per workgroup
template <int KID>
void launch_kstar_pair(const KstarLaunch& k, const double* d_Xa, const double* d_Xb, int M) {
  const ppbo_model* m = k.m;
  auto launch = [&](auto dp) {
    kstar_pair_kernel<KID, decltype(dp)::value><<<k.grid(M, KS_THREADS), KS_THREADS, 0, k.s>>>(
        m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_Xa, d_Xb, M, k.Kt, k.ldk, k.mu_part,
        k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 12>{});
  else KstarLadder::dispatch(m->D, launch);
}

// kstar_slope_kernel in the same buckets and geometry: d_X the points, d_Xi the directions
template <int KID>
void launch_kstar_slope(const KstarLaunch& k, const double* d_X, const double* d_Xi, int M) {
  const ppbo_model* m = k.m;
  auto launch = [&](auto dp) {
    kstar_slope_kernel<KID, decltype(dp)::value><<<k.grid(M, KS_THREADS), KS_THREADS, 0, k.s>>>(
        m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_X, d_Xi, M, k.Kt, k.ldk, k.mu_part,
        k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 12>{});
  else KstarLadder::dispatch(m->D, launch);
}

// kstar_grad_kernel in the same buckets and row splits: P points, KG_PTS of them per (one-wavefront) workgroup (the mean only)
template <int KID>
void launch_kstar_grad(const KstarLaunch& k, const double* d_X, int P) {
  const ppbo_model* m = k.m;
  auto launch = [&](auto dp) {
    kstar_grad_kernel<KID, decltype(dp)::value><<<k.grid(P, KG_PTS), KG_PTS, 0, k.s>>>(
        m->d_X, m->N, m->D, k.p, m->d_alpha, k.mblk(), d_X, P, k.Kt, k.ldk, k.mu_part, k.q_per_split);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 6>{});
  else KstarLadder::dispatch(m->D, launch);
}

// kstar_curv_kernel in the same buckets and geometry: d_X the points, d_Xi the directions, d_Xa the accelerations or
// nullptr (the caller has refused d_Xa with D > 16 or on the camphor kernel, and Matern-3/2 altogether)
template <int KID>
void launch_kstar_curv(const KstarLaunch& k, const double* d_X, const double* d_Xi, const double* d_Xa, int M) {
  static_assert(KID != PPBO_KERNEL_MATERN32, "no curvature for Matern-3/2");
  const ppbo_model* m = k.m;
  auto launch = [&](auto dp, auto acc) {
    kstar_curv_kernel<KID, decltype(dp)::value, decltype(acc)::value><<<k.grid(M, KS_THREADS), KS_THREADS, 0, k.s>>>(
        m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_X, d_Xi, d_Xa, M, k.Kt, k.ldk, k.mu_part,
        k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0);
  };
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) launch(std::integral_constant<int, 12>{}, std::false_type{});
  else
    KstarLadder::dispatch(m->D, [&](auto dp) {
      if constexpr (decltype(dp)::value <= KSTAR_CURV_ACC_MAX_DP)
        if (d_Xa) return launch(dp, std::true_type{});
      launch(dp, std::false_type{});
    });
}

// kstar_func_kernel in five D buckets (whole MFMA k-steps of 4 dimensions; KF_GROUPS groups per workgroup), the camphor
// instance as a vector kernel with KS_THREADS groups per workgroup; n_split row splits as launch_kstar_pair
template <int KID>
void launch_kstar_func(const KstarLaunch& k, const double* d_Xg, const double* d_w, int w_stride, int G, int M) {
  const ppbo_model* m = k.m;
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    kstar_func_camphor_kernel<<<k.grid(M, KS_THREADS), KS_THREADS, 0, k.s>>>(
        m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_Xg, d_w, w_stride, G, M, k.Kt, k.ldk,
        k.mu_part, k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0);
  } else {
    KstarFuncLadder::dispatch(m->D, [&](auto dp) {
      kstar_func_kernel<KID, decltype(dp)::value><<<k.grid(M, KF_GROUPS), 256, 0, k.s>>>(
          m->d_X, m->N, m->D, k.p, m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), d_Xg, d_w, w_stride, G, M, k.Kt, k.ldk,
          k.mu_part, k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0);
    });
  }
}

// ppbo_predict_marginals' operands: the rows of the call are d_dims / d_t [M, 2]
struct MargArgs {
  const ppbo_marginal_axes* ax;
  const int* d_dims;
  const double* d_t;
  int effect;
  MargAxesArg arg;       // filled by marginal_axes_arg
  double prod_A;         // prod_d A_d over ALL axes
};

// A_d = int int kappa_d(u - u') du du' on the host: 2 (l sqrt(pi / 2) erf(1 / (sqrt2 l)) - l^2 (1 - e^(-1 / (2 l^2)))) on an SE
// axis, e^-a I0(a) on a periodic one
int marginal_axes_arg(ppbo_ctx* ctx, MargArgs* ma) {
  const ppbo_marginal_axes* ax = ma->ax;
  PPBO_REQUIRE(ctx, ax != nullptr, "axes");
  PPBO_REQUIRE(ctx, ax->Dc >= 1 && ax->Dc <= MG_AXES, "axes->Dc (1 .. 64)");
  PPBO_REQUIRE(ctx, ax->d_Xu && ax->h_l && ax->h_periodic && ax->h_I0, "axes (d_Xu / h_l / h_periodic / h_I0)");
  MargAxesArg& a = ma->arg;
  a.Dc = ax->Dc;
  a.periodic = 0;
  ma->prod_A = 1.0;
  for (int d = 0; d < MG_AXES; ++d) { a.l[d] = 1.0; a.i0[d] = 1.0; a.a[d] = 1.0; }
  for (int d = 0; d < ax->Dc; ++d) {
    const double l = ax->h_l[d];
    PPBO_REQUIRE(ctx, std::isfinite(l) && l > 0.0, "axes->h_l: positive finite length scales");
    PPBO_REQUIRE(ctx, ax->h_periodic[d] == 0 || ax->h_periodic[d] == 1, "axes->h_periodic (0 or 1)");
    a.l[d] = l;
    const double i0 = ax->h_I0[d];
    PPBO_REQUIRE(ctx, std::isfinite(i0) && i0 > 0.0, "axes->h_I0: positive finite values (e^-a I0(a), a = 1 / l^2)");
    a.i0[d] = i0;
    if (ax->h_periodic[d]) {
      a.periodic |= 1ull << d;
      a.a[d] = i0;
    } else {
      a.a[d] = 2.0 * (1.25331413731550025121 * l * std::erf(0.70710678118654752440 / l) + l * l * std::expm1(-0.5 / (l * l)));
    }
    ma->prod_A *= a.a[d];
  }
  return 0;
}

// ---- the pruned search (predict_passes) --------------------------------------------------------------------------------
// A search that returns only its best record needs the variance of a candidate only if that candidate can be the argmax.
// Pointwise EI and VARIANCE do not decrease in the variance at a fixed mean, so an interval [var_lo, var_hi] of a
// candidate's variance gives an interval [s_lo, s_hi] of its score, and a candidate whose s_hi lies below the best s_lo of
// the chunk cannot win.  With var = (sf2 + t) + q, q = |op e|^2 >= 0 the contraction (op: the operand of the launch, H or a
// projected T; e: the candidate's edge-layout K* column):
//   var_lo = sf2 + t          (exactly <= the fp var: q >= 0 and fp addition is monotone)
//   var_hi = var_lo + (1 + 2^-20) u^2,  u = sum_s sig[s] |e_s|  >=  |op e|   (Cauchy-Schwarz per star s of the columns)
// sig[s] = the Frobenius norm of op's column block of star s (block_norm_kernel, rounded up), |e_s| accumulated by the
// flagged K* instantiation.  2^-20 covers every rounding between u and the fp q (sums of <= 2^17 non-negative terms,
// relative error <= 2^-35 each, the sqrt's and the matrix cores' accumulation).
// Per chunk: block_norm -> K* with bounds -> prune_bounds -> prune_select (threshold, stable compaction, the plan) ->
// gather of the survivors' columns -> contraction (a compact and a full launch, one of which runs) -> score with the
// plan -> argmax.  Nothing waits on the host; the plan lives in device memory.

// sig[s] >= ||op[:, n_q + s m .. n_q + (s + 1) m)||_F for the n_q stars; op [rows][ld].  One workgroup per star, 32 rows x
// 32 columns of lanes; formed on every call (the model's operator may be rewritten in place between calls).  A
// non-finite entry gives a non-finite sig and through it candidates that always survive.
constexpr int BN_THREADS = 1024;
__global__ __launch_bounds__(BN_THREADS) void block_norm_kernel(const double* __restrict__ op, int rows, int ld, int n_q,
                                                                int m, double* __restrict__ sig) {
  __shared__ double red[BN_THREADS / 64];
  const int s = blockIdx.x, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const double* __restrict__ col = op + n_q + (size_t)s * m;
  double acc = 0.0;
  for (int c = tx; c < m; c += 32) {
#pragma unroll 8
    for (int r = ty; r < rows; r += 32) { const double v = col[(size_t)r * ld + c]; acc = fma(v, v, acc); }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < BN_THREADS / 64; ++w) t += red[w];
    sig[s] = sqrt(t) * (1.0 + 0x1.0p-30);   // (the sum of <= 2^22 squares: relative error <= 2^-31 before the root halves it)
  }
}

// The bounds of a chunk's candidates, in score_kernel's geometry and summation order (mu and t are bit for bit what the
// score pass forms): s_hi[c] (+inf = always survives: a non-finite partial sum or bound), per workgroup the largest s_lo
// of its candidates with finite sums (-inf: none) and the largest |mu - mustar| + sd_hi (the scale of prune_select's
// tolerance; 0 for VARIANCE).  rep_*: the report entry's per-candidate copies (NULL on the search path).
__global__ __launch_bounds__(SC_THREADS) void prune_bounds_kernel(const double* __restrict__ mu_part, int n_mu,
                                                                  const double* __restrict__ t_part,
                                                                  const double* __restrict__ u_part, int M, double sf2,
                                                                  int kind, double mustar, double* __restrict__ s_hi_out,
                                                                  double* __restrict__ blk_lo, double* __restrict__ blk_scale,
                                                                  double* __restrict__ rep_u2, double* __restrict__ rep_lo,
                                                                  double* __restrict__ rep_hi) {
  __shared__ double part[3][SC_WAVES][SC_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * SC_CAND + lane;
  double pm = 0.0, pt = 0.0, pu = 0.0;
  if (c < M) {
    for (int s = wave; s < n_mu; s += SC_WAVES) pm += mu_part[(size_t)s * M + c];
    for (int s = wave; s < n_mu; s += SC_WAVES) pt += t_part[(size_t)s * M + c];
    for (int s = wave; s < n_mu; s += SC_WAVES) pu += u_part[(size_t)s * M + c];
  }
  part[0][wave][lane] = pm;
  part[1][wave][lane] = pt;
  part[2][wave][lane] = pu;
  __syncthreads();
  if (wave != 0) return;
  double lo = -INFINITY, scale = 0.0;
  if (c < M) {
    double mu = 0.0, t = 0.0, u = 0.0;
#pragma unroll
    for (int w = 0; w < SC_WAVES; ++w) { mu += part[0][w][lane]; t += part[1][w][lane]; u += part[2][w][lane]; }
    const double var_lo = sf2 + t;
    const double u2 = u * u;
    const double var_hi = var_lo + (1.0 + 0x1.0p-20) * u2;
    double s_lo = score_value(mu, var_lo, kind, mustar), s_hi = score_value(mu, var_hi, kind, mustar);
    const bool ok = fabs(mu) < INFINITY && fabs(var_lo) < INFINITY && fabs(var_hi) < INFINITY && fabs(s_lo) < INFINITY &&
                    fabs(s_hi) < INFINITY;      // (every comparison is false on a NaN)
    if (ok) {
      lo = s_lo;
      if (kind == PPBO_SCORE_POINTWISE_EI) scale = fabs(mu - mustar) + sqrt(fmax(var_hi, 0.0));
    } else s_hi = INFINITY;
    s_hi_out[c] = s_hi;
    if (rep_u2) rep_u2[c] = u2;
    if (rep_lo) rep_lo[c] = s_lo;
    if (rep_hi) rep_hi[c] = s_hi;
  }
  lo = wave_max(lo);
  scale = wave_max(scale);
  if (lane == 0) { blk_lo[blockIdx.x] = lo; blk_scale[blockIdx.x] = scale; }
}

// One workgroup: the threshold b = max s_lo, the survivors {c : !(s_hi[c] + tol < b)} in ascending order (a STABLE
// compaction: the score pass then breaks ties towards the lowest candidate exactly as the full pass does) and the plan.
//   tol = 2^-36 max_c (|mu_c - mustar| + sd_hi,c) for pointwise EI, 0 for VARIANCE.
// Why tol dominates the non-monotonicity of the fp score: VARIANCE is the identity, monotone as it stands.  The fp EI
// F(var) = d Phi(z) + sd phi(z), z = d / sd, follows the exact EI f (which does not decrease in var) to within
//   eps <= (|d| Phi + sd phi) (z^2 + 8) 2^-52  <=  2^-50 (|d| + sd):
// sqrt and the division are correctly rounded, erfc and exp are good to <= 4 ulp (tests/test_gpu_elementary.py holds the
// project's own exp and sqrt to <= 1 ulp), the rounding of z moves Phi and phi by <= z^2 2^-52 relative, and
// (Phi + phi)(z^2 + 8) <= 4.  For the true fp winner w and the candidate a that sets b:
//   F(var_hi,w) >= f(var_hi,w) - eps >= f(var_w) - eps >= F(var_w) - 2 eps >= F(var_a) - 2 eps >= F(var_lo,a) - 4 eps = b - 4 eps,
// so w survives whenever tol >= 4 eps = 2^-48 scale: 2^-36 leaves 2^12.
// pruned = 0 (every launch runs unpruned) when b is not finite, nothing or more than n_cap candidates survive.
// Geometry: the candidates in groups of 64, group g = [64 g, 64 g + 64); in pass A the workgroup walks the groups 16 at a
// time (wavefront w takes group 16 i + w) and leaves each group's ballot in LDS; thread g
// then owns the count of group g for the workgroup-wide scan; pass B (a pruned plan only) writes the indices.
// report[2] = (b, tol).
constexpr int PS_THREADS = 1024, PS_BATCH = 8;    // (loads in flight per lane; 32 measured slower: 21 against 17 us at 65536 candidates)
__global__ __launch_bounds__(PS_THREADS) void prune_select_kernel(const double* __restrict__ s_hi, int M,
                                                                  const double* __restrict__ blk_lo,
                                                                  const double* __restrict__ blk_scale, int n_blk,
                                                                  int n_cap, int* __restrict__ idx,
                                                                  PrunePlan* __restrict__ plan, double* __restrict__ report) {
  constexpr int NW = PS_THREADS / 64;
  __shared__ double sh_b[NW], sh_s[NW];
  __shared__ unsigned long long masks[PS_THREADS];
  __shared__ int excl[PS_THREADS], sh_cnt[NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double b = -INFINITY, sc = 0.0;
  for (int i = threadIdx.x; i < n_blk; i += PS_THREADS) { b = fmax(b, blk_lo[i]); sc = fmax(sc, blk_scale[i]); }
  b = wave_max(b);
  sc = wave_max(sc);
  if (lane == 0) { sh_b[wave] = b; sh_s[wave] = sc; }
  __syncthreads();
  b = sh_b[0]; sc = sh_s[0];
  for (int w = 1; w < NW; ++w) { b = fmax(b, sh_b[w]); sc = fmax(sc, sh_s[w]); }
  const double tol = 0x1.0p-36 * sc;
  const int it = (M + PS_THREADS - 1) / PS_THREADS;          // <= 64 (M <= 65536): at most PS_THREADS groups
  for (int i0 = 0; i0 < 64; i0 += PS_BATCH) {
    double v[PS_BATCH];
#pragma unroll
    for (int k = 0; k < PS_BATCH; ++k) {
      const int c = ((i0 + k) * NW + wave) * 64 + lane;
      v[k] = (i0 + k < it && c < M) ? s_hi[c] : -INFINITY;   // (beyond M: never kept -- b is finite wherever that matters)
    }
#pragma unroll
    for (int k = 0; k < PS_BATCH; ++k) {
      const int c = ((i0 + k) * NW + wave) * 64 + lane;
      const unsigned long long bal = __ballot(c < M && i0 + k < it && !(v[k] + tol < b));
      if (lane == 0) masks[(i0 + k) * NW + wave] = bal;
    }
  }
  __syncthreads();
  const int cnt = __popcll(masks[threadIdx.x]);
  int incl = cnt;                                            // inclusive scan over the wavefront's 64 groups
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) sh_cnt[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < NW; ++w) { if (w < wave) base += sh_cnt[w]; total += sh_cnt[w]; }
  excl[threadIdx.x] = base + incl - cnt;
  const bool pruned = fabs(b) < INFINITY && total > 0 && total <= n_cap;
  if (threadIdx.x == 0) {
    plan->pruned = pruned ? 1 : 0;
    plan->n_surv = total;
    report[0] = b;
    report[1] = tol;
  }
  if (!pruned) return;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i = 0; i < it; ++i) {
    const int g = i * NW + wave;
    const unsigned long long bal = masks[g];
    if ((bal >> lane) & 1ull) idx[excl[g] + __popcll(bal & below)] = g * 64 + lane;
  }
}

// Kc[r][j] = Kt[r][idx[j]] for the rows [r_beg, Nk) that the contraction reads and the survivors j < n_surv of a pruned
// plan; the columns of a tile beyond n_surv keep whatever they held (a column feeds only its own, unread, output)
constexpr int GA_ROWS = 16;
__global__ __launch_bounds__(128) void prune_gather_kernel(const double* __restrict__ Kt, int ldk, int r_beg, int Nk,
                                                           const PrunePlan* __restrict__ plan, const int* __restrict__ idx,
                                                           double* __restrict__ Kc, int n_cap) {
  if (!uniform_load_int(&plan->pruned)) return;
  const int n = uniform_load_int(&plan->n_surv);
  if ((int)blockIdx.x * 128 >= n) return;
  const int j = blockIdx.x * 128 + threadIdx.x;
  if (j >= n) return;
  const int c = idx[j];
  const int r0 = r_beg + blockIdx.y * GA_ROWS;
  double v[GA_ROWS];                       // (every load of the lane in flight at once)
#pragma unroll
  for (int k = 0; k < GA_ROWS; ++k) v[k] = r0 + k < Nk ? Kt[(size_t)(r0 + k) * ldk + c] : 0.0;
#pragma unroll
  for (int k = 0; k < GA_ROWS; ++k)
    if (r0 + k < Nk) Kc[(size_t)(r0 + k) * n_cap + j] = v[k];
}

// what ppbo_predict_prune_report asks predict_passes to leave behind (device arrays of one chunk; any may be NULL)
struct PruneReport {
  double *d_u2 = nullptr, *d_s_lo = nullptr, *d_s_hi = nullptr;
  const PrunePlan* d_plan = nullptr;       // out: the chunk's plan and (threshold, tol), in the ctx's workspace
  const double* d_thr = nullptr;
};

int check_model(ppbo_ctx* ctx, const ppbo_model* m) {
  PPBO_REQUIRE(ctx, m != nullptr, "model");
  PPBO_REQUIRE(ctx, m->d_X && m->d_alpha, "model X/alpha");
  PPBO_REQUIRE(ctx, m->N > 0 && m->D > 0 && m->D <= 64 && m->m >= 1, "model sizes (D<=64)");
  PPBO_REQUIRE(ctx, m->N % (m->m + 1) == 0, "N must be n_q*(m+1) (feedback_processing.py:110-130)");
  PPBO_REQUIRE_KERNEL(ctx, m->kernel_id, m->D);
  if (m->d_G) PPBO_REQUIRE_FORM(ctx, m->form);   // the form of d_G: without an operator there is nothing to misread
  return 0;
}

int pick_split(int M, int n_q) {
  // enough (block, split) pairs to give every SIMD several wavefronts
  const int blocks = (M + KS_THREADS * KS_CPT - 1) / (KS_THREADS * KS_CPT);
  // ~1024 workgroups: from 16384 candidates on a workgroup then covers 64+ rows (round 5 sweep at N = 2048, K* launch:
  // 16384 candidates 0.112 -> 0.099 ms against a target of 2048; 8192 and 65536 candidates unchanged at 0.064 / 0.305)
  int want = (1024 + blocks - 1) / blocks;
  if (want > n_q) want = n_q;
  if (want > 64) want = 64;
  if (want < 1) want = 1;
  return want;
}

// the row splits of a K* launch over M columns: pick_split's count, the stars per split, the splits that hold a star
RowSplit row_split(int M, int n_q) {
  const int n_split = pick_split(M, n_q);
  const int q_per_split = (n_q + n_split - 1) / n_split;
  return RowSplit{n_split, q_per_split, (n_q + q_per_split - 1) / q_per_split};
}

// The operands and workspaces of a scoring pass (predict_passes, two_set_passes), sized for the largest chunk.
// The quadratic form's operands are PADDED so that every tile of its launch takes the unguarded main loop whatever
// N, the star size and the candidate count are (the reference's default m = 25 gives N = 26 n_q: the guarded loop
// cost 23 % at N = 2080, profiles/r05_ragged_shapes.txt): K extent Nk = N rounded up to the chunk depth (K* rows
// [N, Nk) zeroed), G's rows up to a whole row tile (copied into a zero frame when N itself is not one), K*'s row
// stride up to a whole candidate tile (the surplus columns feed only their own, unread, outputs).
struct ScorePlan {
  const ppbo_var_projection* proj = nullptr;   // a projected operator: T carries the padded shape itself
  bool full_chunk_splits = false;              // row splits picked for a full chunk whatever M is
  int extra_part_rows = 0;                     // the predictor's own rows [Mc_max] behind the slabs
  int slab_cols = 0;                           // the pruned search's wider slab rows (0: Mc_max)
  int ntm = 0, Nk = 0, g_rows = 0, ldk = 0, Mc_max = 0, sblocks_max = 0;
  const double* Gq = nullptr;
  RowSplit rs{};
  double *Kt = nullptr, *part = nullptr;
  Best *bests = nullptr, *chunk_best = nullptr;
  int prepare(ppbo_ctx* ctx, const ppbo_model* model, const Chunks& ck, bool want_var, hipStream_t s) {
    const int N = model->N, n_q = N / (model->m + 1), qf_bm = (quadform_variant(ctx) == 5) ? 256 : 128;
    // slabs = row tiles of the shipped quadform shape; of the projected operator when there is one
    ntm = proj ? proj->rows_padded / 128 : (N + qf_bm - 1) / qf_bm;
    Nk = g_rows = N;
    if (proj) {                      // ld = N rounded up to the chunk depth
      Gq = proj->d_T;
      Nk = proj->ld;
      g_rows = proj->rows_padded;
    } else if (want_var) {
      Gq = padded_G(ctx, model, qf_bm, ck.M >= 2048, &Nk, &g_rows, s);
      if (!Gq) return (int)hipErrorOutOfMemory;
      PPBO_LAUNCH_CHECK(ctx);
    }
    Mc_max = ck.Mc_max;
    ldk = (Mc_max + 127) & ~127;
    rs = row_split(full_chunk_splits ? (int)ck.cap : Mc_max, n_q);
    if (want_var) {
      Kt = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_KSTAR, (size_t)Nk * ldk * sizeof(double));
      if (!Kt) return (int)hipErrorOutOfMemory;
      if (Nk != N) PPBO_HIP_CHECK(ctx, hipMemsetAsync(Kt + (size_t)N * ldk, 0, (size_t)(Nk - N) * ldk * sizeof(double), s));
    }
    // (the compact launch's slabs of a pruned chunk, row stride slab_cols, share the full launch's: one of the two writes them)
    part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, ((size_t)(2 * rs.n_split_eff + extra_part_rows) * Mc_max +
                                                            (size_t)ntm * (slab_cols ? slab_cols : Mc_max)) * sizeof(double));
    if (!part) return (int)hipErrorOutOfMemory;
    sblocks_max = score_blocks(Mc_max);
    bests = (Best*)ppbo_workspace(ctx, ppbo_ctx::WS_SMALL, (size_t)(sblocks_max + ck.n) * sizeof(Best));
    if (!bests) return (int)hipErrorOutOfMemory;
    chunk_best = bests + sblocks_max;
    return 0;
  }
  // the partial sums of a chunk of Mc columns: the mean's and the Lambda term's per row split, the contraction's slabs
  double* mu_part() const { return part; }
  double* t_part(int Mc) const { return part + (size_t)rs.n_split_eff * Mc; }
  double* slab(int Mc) const { return part + (size_t)2 * rs.n_split_eff * Mc; }
  double* extra() const { return part + (size_t)(2 * rs.n_split_eff + ntm) * Mc_max; }
};

// The workspace of the line entries and ppbo_predict_gradients (cols_max columns in the largest chunk): the row split of
// their K* launch and, with_operator, the padded operator and Kt [Nk][ld], Y [g_rows][ld] and -- edge form: Y = H E
// with E the edge-layout K* beside the node-layout one -- Ke [Nk][ld] in one WS_KSTAR, rows [N, Nk) of Kt and Ke zeroed.
struct LineWorkspace {
  int ld = 0, Nk = 0, g_rows = 0;
  RowSplit rs{};
  const double* Gq = nullptr;
  double *Kt = nullptr, *Y = nullptr, *Ke = nullptr;
  // operands of Y = G K* padded to whole tiles / chunks, as in ScorePlan: every tile of that product then takes the
  // unguarded loop whatever N, the star size and the column count are (m = 25: 4.16 -> 3.6 ms for 512 lines at N = 2080)
  int prepare(ppbo_ctx* ctx, const ppbo_model* model, int cols_max, bool with_operator, bool worth_padding_G, hipStream_t s) {
    const int N = model->N;
    ld = (cols_max + 127) & ~127;
    rs = row_split(cols_max, N / (model->m + 1));
    if (!with_operator) return 0;
    Nk = g_rows = N;
    Gq = padded_G(ctx, model, 128, worth_padding_G, &Nk, &g_rows, s);
    if (!Gq) return (int)hipErrorOutOfMemory;
    PPBO_LAUNCH_CHECK(ctx);
    const bool edge = model->form == PPBO_FORM_EDGE;
    double* ws = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_KSTAR, (size_t)((edge ? 2 : 1) * Nk + g_rows) * ld * sizeof(double));
    if (!ws) return (int)hipErrorOutOfMemory;
    Kt = ws;
    Y = ws + (size_t)Nk * ld;
    Ke = edge ? Y + (size_t)g_rows * ld : nullptr;
    if (Nk != N) PPBO_HIP_CHECK(ctx, hipMemsetAsync(Kt + (size_t)N * ld, 0, (size_t)(Nk - N) * ld * sizeof(double), s));
    if (edge && Nk != N) PPBO_HIP_CHECK(ctx, hipMemsetAsync(Ke + (size_t)N * ld, 0, (size_t)(Nk - N) * ld * sizeof(double), s));
    return 0;
  }
};

// The best of a call comes back through the ctx's host-mapped record (written by the last argmax workgroup, flag polled
// by the host) instead of a device-to-host copy + stream synchronisation.  begin() takes the record when a best is wanted
// (else chunk() and finish() do nothing); chunk(): the one-workgroup argmax of a chunk, which with ONE chunk writes the
// record itself; finish(): the record of several chunks, the wait, the copy out ((NaN, -1): no non-NaN score).
struct BestReturn {
  PpboHostRecord hr{};
  bool want = false;
  int begin(ppbo_ctx* ctx, bool want_best) { return (want = want_best) ? ppbo_host_record(ctx, &hr) : 0; }
  int chunk(ppbo_ctx* ctx, const Best* blk_bests, int n_blocks, Best* chunk_best, int64_t ch, const Chunks& ck, hipStream_t s) const {
    if (!want) return 0;
    argmax_final_kernel<<<1, 256, 0, s>>>(blk_bests, n_blocks, chunk_best + ch, ck.n == 1 ? hr.d_rec : nullptr, 0,
                                          ck.n == 1 ? hr.d_flag : nullptr, hr.epoch);
    PPBO_LAUNCH_CHECK(ctx);
    return 0;
  }
  int wait(ppbo_ctx* ctx, hipStream_t s, double* h_best_val, int64_t* h_best_idx) const {
    if (int rc = ppbo_host_record_wait(ctx, hr, s)) return rc;
    if (h_best_val) *h_best_val = hr.h_rec[0];
    if (h_best_idx) *h_best_idx = (int64_t)hr.h_rec[1];
    return 0;
  }
  int finish(ppbo_ctx* ctx, const Best* chunk_best, const Chunks& ck, hipStream_t s, double* h_best_val, int64_t* h_best_idx) const {
    if (!want) return 0;
    if (ck.n > 1) {
      best_record_kernel<<<1, 64, 0, s>>>(chunk_best, (int)ck.n, 0, hr.d_rec, hr.d_flag, hr.epoch);
      PPBO_LAUNCH_CHECK(ctx);
    }
    return wait(ctx, s, h_best_val, h_best_idx);
  }
};

// A K* workspace of an entry's own (ppbo_predict_tournament behind the one-launch scoring path, ppbo_search_batch):
// K [NkU][ldk] in the layout of the model's form and the part_rows (1: mean, 2: mean and Lambda term) x n_split_eff
// partial sums of its launch, which nobody reads, in one slot; zero_tail: rows [N, NkU) zeroed.
struct OwnKstar {
  int ldk = 0;
  RowSplit rs{};
  double *K = nullptr, *part = nullptr;
  int prepare(ppbo_ctx* ctx, int slot, const ppbo_model* model, int NkU, int Mc_max, int part_rows, bool zero_tail, hipStream_t s) {
    const int N = model->N, n_q = N / (model->m + 1);
    ldk = (Mc_max + 127) & ~127;
    rs = row_split(Mc_max, n_q);
    K = (double*)ppbo_workspace(ctx, slot, ((size_t)NkU * ldk + (size_t)part_rows * rs.n_split_eff * Mc_max) * sizeof(double));
    if (!K) return (int)hipErrorOutOfMemory;
    part = K + (size_t)NkU * ldk;
    if (zero_tail && NkU != N) PPBO_HIP_CHECK(ctx, hipMemsetAsync(K + (size_t)N * ldk, 0, (size_t)(NkU - N) * ldk * sizeof(double), s));
    return 0;
  }
  // K* of the Mc columns xc.  edge_k0 >= 0: the edge layout from that row on, with the Lambda term's sums; else the node layout
  int form(ppbo_ctx* ctx, const ppbo_model* model, const double* xc, int Mc, hipStream_t s, int edge_k0 = -1) const {
    PpboProfScope pf(ctx, ppbo_ctx::PF_KSTAR, s);
    const bool edge = edge_k0 >= 0;
    bool oom = false;
    const double* geo = edge ? star_geometry(ctx, model, s, &oom) : nullptr;
    if (oom) return (int)hipErrorOutOfMemory;
    dispatch_kstar(model, xc, Mc, K, ldk, part, edge ? part + (size_t)rs.n_split_eff * Mc : nullptr, rs.q_per_split,
                   rs.n_split_eff, edge, s, edge_k0, geo);
    PPBO_LAUNCH_CHECK(ctx);
    return 0;
  }
};

}  // namespace

extern "C" {

// the scoring passes of ppbo_predict / ppbo_predict_record: per 65536-candidate chunk kstar -> quadform -> score ->
// one-workgroup argmax.  Leaves the per-chunk bests in chunk_best (device); with d_record and ONE chunk the
// argmax launch writes the record (and raises the publication flag) itself.
// after_chunk (ppbo_predict_tournament): called behind the launches of every chunk with the chunk's first row, its size and
// its K* workspace -- Kt [Nk][ldk] in the layout of the model's form, valid until the next chunk's launches -- and ONCE,
// with Kt == NULL and (0, M), on the one-launch path, which leaves no K* in memory.  The launches themselves do not change.
using PredictChunkHook = std::function<int(int64_t c_beg, int64_t Mc, const double* Kt, int ldk, int Nk)>;
// what a caller asks of the passes (points, score, outputs in this order; by name what else it uses) and what they leave
struct PredictRequest {
  const double* d_Xc = nullptr;                // [M][D]
  int64_t M = 0;
  int score_kind = PPBO_SCORE_MEAN;
  double mustar = 0.0;
  double *d_mu = nullptr, *d_var = nullptr, *d_score = nullptr;   // [M] each, any may be NULL
  bool want_best = false;
  double* d_record = nullptr;                  // the caller's record (value, index + record_offset); NULL: chunk bests only
  int64_t record_offset = 0;
  unsigned long long *publish = nullptr, epoch = 0;   // the flag raised to `epoch` behind the record
  const PredictChunkHook* after_chunk = nullptr;
  bool projected = false;                      // read model->proj (the entries the header names); else the model has none
  PruneReport* report = nullptr;
  Best* chunk_best = nullptr;                  // results: [n_chunks] on the device
  int n_chunks = 0;
  int predict_passes(ppbo_ctx* ctx, const ppbo_model* model, hipStream_t s);
};
int PredictRequest::predict_passes(ppbo_ctx* ctx, const ppbo_model* model, hipStream_t s) {
  if (int rc = check_model(ctx, model)) return rc;
  const ppbo_var_projection* proj = projected ? &model->proj : nullptr;
  PPBO_REQUIRE(ctx, d_Xc != nullptr && M > 0, "candidates");
  // a projected operator (ppbo_var_projection_build): rows == 0 = none, today's launches.  One with rows must
  // have been built for a model of this shape and form.
  if (proj && proj->rows <= 0) proj = nullptr;
  if (proj) {
    int rows_max = 0, ld = 0;
    PPBO_REQUIRE(ctx, ppbo_var_projection_shape(model, &rows_max, &ld) == 0 && model->form == PPBO_FORM_EDGE &&
                          !ppbo_fused_eligible(ctx, model) && proj->d_T && proj->ld == ld && proj->rows_padded % 128 == 0 &&
                          proj->rows <= proj->rows_padded && proj->rows_padded <= rows_max,
                 "the variance projection was not built for a model of this N, m and form");
    if (!model->d_G) proj = nullptr;     // a mean-only call reads no operator
  }
  PPBO_REQUIRE(ctx, score_kind >= 0 && score_kind <= 2, "score_kind");
  const bool want_var = (model->d_G != nullptr);
  PPBO_REQUIRE(ctx, want_var || (d_var == nullptr && score_kind == PPBO_SCORE_MEAN),
               "variance / EI scores need model->d_G");
  PPBO_REQUIRE(ctx, !want_var || (model->d_lam_diag && model->d_lam_off), "model Lambda");
  const int N = model->N, mblk = model->m + 1, n_q = N / mblk;
  // an edge-form operator is always contracted by the three-launch form (the one-launch kernel reads node-form G)
  const int edge_k0 = (want_var && model->form == PPBO_FORM_EDGE) ? ppbo_edge_k0(n_q) : -1;
  // the pruned search (above): the best record only, an edge-form operator on the three-launch path, a score that does
  // not decrease in the variance, fp64 K*.  Every other call enqueues today's launches.
  const bool prune = (ctx->prune || report) && want_best && !d_mu && !d_var && !d_score && !after_chunk && edge_k0 >= 0 &&
                     !ppbo_fused_eligible(ctx, model) && !model->kstar_fp32 &&
                     (score_kind == PPBO_SCORE_POINTWISE_EI || score_kind == PPBO_SCORE_VARIANCE);
  PPBO_REQUIRE(ctx, !report || (prune && M <= 65536),
               "the prune report takes one chunk of an edge-form model on the three-launch path, pointwise EI or VARIANCE");
  if (ppbo_fused_eligible(ctx, model)) {
    // Models of up to 1024 rows: ONE launch forms K* in LDS, contracts it with G on the matrix cores and scores
    // (fused.hip) -- no K* in HBM, no slab pass, no candidate chunks -- then the one-workgroup argmax.  The choice
    // depends on the model only: a shard of a sharded search scores a candidate exactly as the unsharded search does.
    int ldgt = N;
    const double* Gt = ppbo_fused_transposed_G(ctx, model, &ldgt, s);
    if (!Gt) return (int)hipErrorOutOfMemory;
    PPBO_LAUNCH_CHECK(ctx);
    const long long nblk = (M + 31) / 32;
    PPBO_REQUIRE(ctx, nblk < ((long long)1 << 31), "candidate count");
    Best* bests = (Best*)ppbo_workspace(ctx, ppbo_ctx::WS_SMALL, (size_t)(nblk + 1) * sizeof(Best));
    if (!bests) return (int)hipErrorOutOfMemory;
    Best* chunk_best = bests + nblk;
    {
      PpboProfScope pf(ctx, ppbo_ctx::PF_FUSED, s);
      if (int rc = ppbo_fused_score(ctx, model, Gt, ldgt, d_Xc, (long long)M, score_kind, mustar, 0, d_mu, d_var, d_score,
                                    want_best ? bests : nullptr, s))
        return rc;
    }
    if (want_best) {
      PpboProfScope pfs(ctx, ppbo_ctx::PF_SCORE, s);
      argmax_final_kernel<<<1, 256, 0, s>>>(bests, (int)nblk, chunk_best, d_record, (long long)record_offset, publish, epoch);
      PPBO_LAUNCH_CHECK(ctx);
    }
    this->chunk_best = chunk_best;
    n_chunks = 1;
    if (after_chunk)
      if (int rc = (*after_chunk)(0, M, nullptr, 0, 0)) return rc;
    return 0;
  }
  const Chunks ck(M);
  const int Mc_max = ck.Mc_max;
  // the survivor capacity of a pruned chunk: an eighth of the chunk in whole 128-column tiles (PPBO_PRUNE_CAP: tests)
  int n_cap = ((ctx->prune_cap > 0 ? ctx->prune_cap : Mc_max / 8) / 128) * 128;
  if (n_cap < 128) n_cap = 128;
  ScorePlan pl;
  pl.proj = proj;
  pl.slab_cols = (prune && n_cap > Mc_max) ? n_cap : 0;
  if (int rc = pl.prepare(ctx, model, ck, want_var, s)) return rc;
  const int ntm = pl.ntm, Nk = pl.Nk, g_rows = pl.g_rows, ldk = pl.ldk, sblocks_max = pl.sblocks_max;
  const int q_per_split = pl.rs.q_per_split, n_split_eff = pl.rs.n_split_eff;
  const double* const Gq = pl.Gq;
  double* const Kt = pl.Kt;
  Best *const bests = pl.bests, *const chunk_best = pl.chunk_best;
  // the pruned search's own arrays: u_part [n_split][Mc], s_hi [Mc], sig [n_q], per score workgroup (max s_lo, scale),
  // (threshold, tol), then idx [n_cap] and the plan; the gathered columns Kc [Nk][n_cap]
  double *u_part = nullptr, *s_hi = nullptr, *sig = nullptr, *blk_lo = nullptr, *blk_scale = nullptr, *thr = nullptr, *Kc = nullptr;
  int* sidx = nullptr;
  PrunePlan* plan = nullptr;
  if (prune) {
    const size_t nd = (size_t)(n_split_eff + 1) * Mc_max + n_q + 2 * (size_t)sblocks_max + 2;
    char* pw = (char*)ppbo_workspace(ctx, ppbo_ctx::WS_PRUNE, nd * sizeof(double) + (size_t)(n_cap + 2) * sizeof(int));
    Kc = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PRUNE_KC, (size_t)Nk * n_cap * sizeof(double));
    if (!pw || !Kc) return (int)hipErrorOutOfMemory;
    u_part = (double*)pw;
    s_hi = u_part + (size_t)n_split_eff * Mc_max;
    sig = s_hi + Mc_max;
    blk_lo = sig + n_q;
    blk_scale = blk_lo + sblocks_max;
    thr = blk_scale + sblocks_max;
    sidx = (int*)(thr + 2);
    plan = (PrunePlan*)(sidx + n_cap);
    if (report) { report->d_plan = plan; report->d_thr = thr; }
  }
  for (const Chunk c : ck) {
    const int Mc = c.Mc;
    const double* xc = d_Xc + (size_t)c.beg * model->D;
    double *mu_part = pl.mu_part(), *t_part = pl.t_part(Mc), *slab = pl.slab(Mc);
    {
      PpboProfScope pf(ctx, ppbo_ctx::PF_KSTAR, s);
      bool oom = false;
      const double* geo = star_geometry(ctx, model, s, &oom);
      if (oom) return (int)hipErrorOutOfMemory;
      if (prune) block_norm_kernel<<<n_q, BN_THREADS, 0, s>>>(Gq, g_rows, Nk, n_q, mblk - 1, sig);
      dispatch_kstar(model, xc, Mc, Kt, ldk, mu_part, t_part, q_per_split, n_split_eff, want_var, s, edge_k0, geo,
                     prune ? sig : nullptr, u_part);
    }
    PPBO_LAUNCH_CHECK(ctx);
    const int sblocks = score_blocks(Mc);
    const double sf2 = model->theta[2] * model->theta[2];
    if (prune) {
      PpboProfScope pf(ctx, ppbo_ctx::PF_QUADFORM, s);
      prune_bounds_kernel<<<sblocks, SC_THREADS, 0, s>>>(mu_part, n_split_eff, t_part, u_part, Mc, sf2, score_kind, mustar,
                                                         s_hi, blk_lo, blk_scale, report ? report->d_u2 : nullptr,
                                                         report ? report->d_s_lo : nullptr, report ? report->d_s_hi : nullptr);
      prune_select_kernel<<<1, PS_THREADS, 0, s>>>(s_hi, Mc, blk_lo, blk_scale, sblocks, n_cap, sidx, plan, thr);
      prune_gather_kernel<<<dim3(n_cap / 128, (Nk - edge_k0 + GA_ROWS - 1) / GA_ROWS), 128, 0, s>>>(Kt, ldk, edge_k0, Nk, plan,
                                                                                                    sidx, Kc, n_cap);
      PPBO_LAUNCH_CHECK(ctx);
      // the compact launch (runs when the plan is pruned), then today's (runs when it is not)
      if (int rc = dispatch_quadform(ctx, Gq, Nk, g_rows, proj ? g_rows : N, Kc, n_cap, n_cap, mblk, slab, edge_k0, s,
                                     proj != nullptr, plan, 1))
        return rc;
      if (int rc = dispatch_quadform(ctx, Gq, Nk, g_rows, proj ? g_rows : N, Kt, ldk, Mc, mblk, slab, edge_k0, s,
                                     proj != nullptr, plan, 0))
        return rc;
    } else
    if (want_var) {
      PpboProfScope pf(ctx, ppbo_ctx::PF_QUADFORM, s);
      if (int rc = dispatch_quadform(ctx, Gq, Nk, g_rows, proj ? g_rows : N, Kt, ldk, Mc, mblk, slab, edge_k0, s, proj != nullptr))
        return rc;
    }
    std::optional<PpboProfScope> pfs;          // (ends before after_chunk's launches)
    pfs.emplace(ctx, ppbo_ctx::PF_SCORE, s);
    const bool one = (ck.n == 1);
    if (prune)
      score_plan_kernel<<<sblocks, SC_THREADS, 0, s>>>(mu_part, n_split_eff, t_part, slab, ntm, Mc, sf2, score_kind, mustar,
                                                       (long long)c.beg, bests, plan, sidx, n_cap);
    else
    score_kernel<<<sblocks, SC_THREADS, 0, s>>>(mu_part, n_split_eff, t_part, want_var ? slab : nullptr, ntm, Mc,
                                                sf2, score_kind, mustar,
                                                (long long)c.beg, d_mu ? d_mu + c.beg : nullptr,
                                                d_var ? d_var + c.beg : nullptr, d_score ? d_score + c.beg : nullptr,
                                                want_best ? bests : nullptr);
    PPBO_LAUNCH_CHECK(ctx);
    if (want_best) {
      argmax_final_kernel<<<1, 256, 0, s>>>(bests, sblocks, chunk_best + c.ch, one ? d_record : nullptr,
                                            (long long)record_offset, one ? publish : nullptr, epoch);
      PPBO_LAUNCH_CHECK(ctx);
    }
    pfs.reset();
    if (after_chunk)
      if (int rc = (*after_chunk)(c.beg, Mc, Kt, ldk, Nk)) return rc;
  }
  if (d_record && ck.n > 1) {
    best_record_kernel<<<1, 64, 0, s>>>(chunk_best, (int)ck.n, (long long)record_offset, d_record, publish, epoch);
    PPBO_LAUNCH_CHECK(ctx);
  }
  this->chunk_best = chunk_best;
  n_chunks = (int)ck.n;
  return 0;
}

int ppbo_predict(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                 double mustar, double* d_mu, double* d_var, double* d_score, double* h_best_val,
                 int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  PredictRequest rq{d_Xc, M, score_kind, mustar, d_mu, d_var, d_score};
  rq.projected = true;
  rq.want_best = h_best_val || h_best_idx;
  // predict_passes writes the record itself: the ctx's when a best is wanted, taken before its refusals (else none)
  BestReturn br;
  if (int rc = br.begin(ctx, rq.want_best)) return rc;
  rq.d_record = br.hr.d_rec; rq.publish = br.hr.d_flag; rq.epoch = br.hr.epoch;
  if (int rc = rq.predict_passes(ctx, model, s)) return rc;
  return rq.want_best ? br.wait(ctx, s, h_best_val, h_best_idx) : 0;
}

int ppbo_predict_record(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                        double mustar, int64_t index_offset, double* d_record, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_record != nullptr, "d_record");
  return ppbo_predict_record_publish(ctx, model, d_Xc, M, score_kind, mustar, index_offset, d_record, nullptr, 0, (hipStream_t)stream);
}

int ppbo_predict_prune_report(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                              double mustar, double* d_u2, double* d_s_lo, double* d_s_hi, double* h_threshold,
                              int* h_n_surv, int* h_pruned, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  PruneReport rep;
  rep.d_u2 = d_u2; rep.d_s_lo = d_s_lo; rep.d_s_hi = d_s_hi;
  PpboHostRecord hr;
  if (int rc = ppbo_host_record(ctx, &hr)) return rc;
  PredictRequest rq{d_Xc, M, score_kind, mustar};
  rq.projected = true; rq.report = &rep;
  rq.want_best = true; rq.d_record = hr.d_rec; rq.publish = hr.d_flag; rq.epoch = hr.epoch;
  if (int rc = rq.predict_passes(ctx, model, s)) return rc;
  if (int rc = ppbo_host_record_wait(ctx, hr, s)) return rc;
  PrunePlan pl{0, 0};
  double thr[2] = {0.0, 0.0};
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(&pl, rep.d_plan, sizeof(pl), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(thr, rep.d_thr, sizeof(thr), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if (h_threshold) *h_threshold = thr[0];
  if (h_n_surv) *h_n_surv = pl.n_surv;
  if (h_pruned) *h_pruned = pl.pruned;
  return 0;
}

}  // extern "C"

// The two-set predictors: duels, slopes, curvatures, functionals and marginals.  (Their entry points are extern "C" by
// their declarations in ppbo_hip.h; the descriptors beside them hold templates, so this section is outside the block.)
// Each scores M columns that are no single point -- the sides of a duel, a point and a direction, a group of points and
// its weights, a pair of axes -- and brings a small descriptor with its messages, its own argument rules, its
// preparation, and its K* and score launches for a chunk.  two_set_passes is what they share: per chunk of 65536
// columns K* -> quadform -> score -> one-workgroup argmax, with predict_passes' workspaces and operand padding.  Both
// operator forms take these three launches (the one-launch kernel of fused.hip holds one point per column).  The score
// kinds of the five entries carry the same values (mean, variance, probability).
static_assert(PPBO_SLOPE_MEAN == PPBO_PAIR_MEAN && PPBO_SLOPE_VARIANCE == PPBO_PAIR_VARIANCE && PPBO_SLOPE_PROB == PPBO_PAIR_PROB,
              "one score_kind check for both entries");
static_assert(PPBO_CURV_MEAN == PPBO_PAIR_MEAN && PPBO_CURV_VARIANCE == PPBO_PAIR_VARIANCE && PPBO_CURV_PROB == PPBO_PAIR_PROB,
              "one score_kind check for all three entries");
static_assert(PPBO_FUNCTIONAL_MEAN == PPBO_PAIR_MEAN && PPBO_FUNCTIONAL_VARIANCE == PPBO_PAIR_VARIANCE &&
                  PPBO_FUNCTIONAL_PROB == PPBO_PAIR_PROB,
              "one score_kind check for all four entries");

// A code object holds its kernels in the order their instantiations are first asked for.  For this section that order
// is stated here, per kernel id (the K* launchers, then the score kernels), so that it depends neither on the order of
// the entry points below nor on how they share their code.  Never called; it names nothing that no entry point launches.
template <int KID>
static void two_set_kernel_order() {
  (void)&launch_kstar_func<KID>;
  if constexpr (KID != PPBO_KERNEL_MATERN32) (void)&launch_kstar_curv<KID>;
  (void)&launch_kstar_slope<KID>;
  (void)&launch_kstar_pair<KID>;
  (void)&functional_prior_kernel<KID>;
  if constexpr (KID != PPBO_KERNEL_MATERN32) (void)&curv_score_kernel<KID>;
  (void)&slope_score_kernel<KID>;
  (void)&pair_score_kernel<KID>;
}
template void two_set_kernel_order<PPBO_KERNEL_SE>();
template void two_set_kernel_order<PPBO_KERNEL_RQ>();
template void two_set_kernel_order<PPBO_KERNEL_MATERN52>();
template void two_set_kernel_order<PPBO_KERNEL_MATERN32>();
template void two_set_kernel_order<PPBO_KERNEL_CAMPHOR>();

// A chunk's score launch: the sums of its K* and contraction launches (slab NULL: no variance; extra: the predictor's
// extra_part_rows rows behind them), its first column, its results (stepped to the chunk, or NULL; bests NULL: no best)
struct TwoSetScore {
  const ppbo_model* m;
  KernParams p;
  const double *mu_part, *t_part, *slab;
  double* extra;
  int n_split, ntm, Mc, score_kind, sblocks;
  long long c_beg;
  double *d_mu, *d_var, *d_prob, *d_score;
  Best* bests;
  hipStream_t s;
};
// the parts of a descriptor that most predictors leave as they are
struct TwoSetBase {
  static constexpr const char* rows = "row count (1 .. 2^31 - 1)";
  static constexpr bool full_chunk_splits = false;     // row splits picked for a full chunk whatever M is
  static constexpr int extra_part_rows = 0;
  int check(ppbo_ctx*, const ppbo_model*) { return 0; }                      // its own argument rules
  // (once per call, before the first chunk; the Best records: sblocks_max of them that nothing has written yet)
  int prepare(ppbo_ctx*, const ppbo_model*, const KernParams&, int64_t, Best*, int, hipStream_t) { return 0; }
};

template <class Pred>
static int two_set_passes(ppbo_ctx* ctx, const ppbo_model* model, Pred& pr, int64_t M, int score_kind, double* d_mu,
                          double* d_var, double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx,
                          hipStream_t s) {
  if (int rc = check_model(ctx, model)) return rc;
  PPBO_REQUIRE(ctx, pr.has_operands(), Pred::operands);
  PPBO_REQUIRE(ctx, M >= 1 && M <= (int64_t)0x7fffffff, Pred::rows);
  PPBO_REQUIRE(ctx, score_kind == PPBO_PAIR_MEAN || score_kind == PPBO_PAIR_VARIANCE || score_kind == PPBO_PAIR_PROB,
               "score_kind");
  if (int rc = pr.check(ctx, model)) return rc;
  PPBO_REQUIRE(ctx, !model->kstar_fp32, Pred::fp64_only);
  const bool want_var = d_var || d_prob || score_kind != PPBO_PAIR_MEAN;
  PPBO_REQUIRE(ctx, !want_var || model->d_G != nullptr, "variance / probability need model->d_G");
  PPBO_REQUIRE(ctx, !want_var || (model->d_lam_diag && model->d_lam_off), "model Lambda");
  const bool want_best = h_best_val || h_best_idx;
  const int N = model->N, mblk = model->m + 1, n_q = N / mblk;
  const int edge_k0 = (want_var && model->form == PPBO_FORM_EDGE) ? ppbo_edge_k0(n_q) : -1;
  const KernParams p = make_kern_params(model->kernel_id, model->theta);
  const Chunks ck(M);
  ScorePlan pl;
  pl.full_chunk_splits = Pred::full_chunk_splits;
  pl.extra_part_rows = Pred::extra_part_rows;
  if (int rc = pl.prepare(ctx, model, ck, want_var, s)) return rc;
  if (int rc = pr.prepare(ctx, model, p, M, pl.bests, pl.sblocks_max, s)) return rc;
  BestReturn br;                   // (behind the preparation, which may have used the ctx's record for a check of its own)
  if (int rc = br.begin(ctx, want_best)) return rc;
  for (const Chunk c : ck) {
    const int Mc = c.Mc;
    double *mu_part = pl.mu_part(), *t_part = pl.t_part(Mc), *slab = pl.slab(Mc);
    const int sblocks = score_blocks(Mc);
    const KstarLaunch k{model, p, pl.Kt, pl.ldk, mu_part, t_part, pl.rs.q_per_split, pl.rs.n_split_eff, want_var, edge_k0, s};
    const TwoSetScore sc{model, p, mu_part, t_part, want_var ? slab : nullptr, pl.extra(),
                         pl.rs.n_split_eff, pl.ntm, Mc, score_kind, sblocks, (long long)c.beg, d_mu ? d_mu + c.beg : nullptr,
                         d_var ? d_var + c.beg : nullptr, d_prob ? d_prob + c.beg : nullptr,
                         d_score ? d_score + c.beg : nullptr, want_best ? pl.bests : nullptr, s};
    if (int rc = ppbo_kernel_dispatch(ctx, model->kernel_id, [&](auto kid) {
          constexpr int KID = decltype(kid)::value;
          {
            PpboProfScope pf(ctx, ppbo_ctx::PF_KSTAR, s);
            pr.template kstar<KID>(k, c.beg, Mc);
          }
          PPBO_LAUNCH_CHECK(ctx);
          if (want_var) {
            PpboProfScope pf(ctx, ppbo_ctx::PF_QUADFORM, s);
            if (int rc2 = dispatch_quadform(ctx, pl.Gq, pl.Nk, pl.g_rows, N, pl.Kt, pl.ldk, Mc, mblk, slab, edge_k0, s)) return rc2;
          }
          PpboProfScope pfs(ctx, ppbo_ctx::PF_SCORE, s);
          pr.template score<KID>(sc);
          PPBO_LAUNCH_CHECK(ctx);
          return 0;
        }))
      return rc;
    if (int rc = br.chunk(ctx, pl.bests, sblocks, pl.chunk_best, c.ch, ck, s)) return rc;
  }
  return br.finish(ctx, pl.chunk_best, ck, s, h_best_val, h_best_idx);
}

// Duels: the sides (a, b) of a duel, [M, D] each; kstar_pair -> quadform -> pair_score
struct PairsPred : TwoSetBase {
  static constexpr const char* operands = "pairs (d_Xa / d_Xb)";
  static constexpr const char* rows = "pair count (1 .. 2^31 - 1)";
  static constexpr const char* fp64_only = "pairs are fp64 only (kstar_fp32)";
  const double *d_Xa, *d_Xb;
  bool has_operands() const { return d_Xa && d_Xb; }
  template <int KID>
  void kstar(const KstarLaunch& k, int64_t c_beg, int Mc) const {
    const size_t o = (size_t)c_beg * k.m->D;
    launch_kstar_pair<KID>(k, d_Xa + o, d_Xb + o, Mc);
  }
  template <int KID>
  void score(const TwoSetScore& sc) const {
    const size_t o = (size_t)sc.c_beg * sc.m->D;
    const double two_sigma2 = 2.0 * sc.m->theta[0] * sc.m->theta[0];
    pair_score_kernel<KID><<<sc.sblocks, SC_THREADS, 0, sc.s>>>(sc.mu_part, sc.n_split, sc.t_part, sc.slab, sc.ntm, sc.Mc,
                                                                d_Xa + o, d_Xb + o, sc.m->D, sc.p, two_sigma2, sc.score_kind,
                                                                sc.c_beg, sc.d_mu, sc.d_var, sc.d_prob, sc.d_score, sc.bests);
  }
};
int ppbo_predict_pairs(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, const double* d_Xb, int64_t M,
                       int score_kind, double* d_mu, double* d_var, double* d_prob, double* d_score, double* h_best_val,
                       int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  PairsPred pr{{}, d_Xa, d_Xb};
  return two_set_passes(ctx, model, pr, M, score_kind, d_mu, d_var, d_prob, d_score, h_best_val, h_best_idx, (hipStream_t)stream);
}

// Slopes: the column g = d/da k(x + a xi, X) at a = 0 in place of a duel's difference column, from the point and the
// direction (x, xi), [M, D] each; kstar_slope -> quadform -> slope_score.  The K* launches share the "kstar" profile slot
// with ppbo_predict and ppbo_predict_pairs.
struct SlopesPred : TwoSetBase {
  static constexpr const char* operands = "slopes (d_X / d_Xi)";
  static constexpr const char* fp64_only = "slopes are fp64 only (kstar_fp32)";
  const double *d_X, *d_Xi;
  bool has_operands() const { return d_X && d_Xi; }
  template <int KID>
  void kstar(const KstarLaunch& k, int64_t c_beg, int Mc) const {
    const size_t o = (size_t)c_beg * k.m->D;
    launch_kstar_slope<KID>(k, d_X + o, d_Xi + o, Mc);
  }
  template <int KID>
  void score(const TwoSetScore& sc) const {
    slope_score_kernel<KID><<<sc.sblocks, SC_THREADS, 0, sc.s>>>(sc.mu_part, sc.n_split, sc.t_part, sc.slab, sc.ntm, sc.Mc,
                                                                 d_Xi + (size_t)sc.c_beg * sc.m->D, sc.m->D, sc.p, sc.score_kind,
                                                                 sc.c_beg, sc.d_mu, sc.d_var, sc.d_prob, sc.d_score, sc.bests);
  }
};
int ppbo_predict_slopes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, const double* d_Xi, int64_t M,
                        int score_kind, double* d_mu, double* d_var, double* d_prob, double* d_score, double* h_best_val,
                        int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  SlopesPred pr{{}, d_X, d_Xi};
  return two_set_passes(ctx, model, pr, M, score_kind, d_mu, d_var, d_prob, d_score, h_best_val, h_best_idx, (hipStream_t)stream);
}

// Curvatures: the column c = d^2/da^2 k(gamma(a), X) at a = 0 for the path through x with velocity xi and acceleration
// acc (d_Xa == NULL: straight lines), [M, D] each; kstar_curv -> quadform -> curv_score.  The K* launches share the
// "kstar" profile slot.  Matern-3/2 is refused by check(), and nothing is instantiated for it.
struct CurvaturesPred : TwoSetBase {
  static constexpr const char* operands = "curvatures (d_X / d_Xi)";
  static constexpr const char* fp64_only = "curvatures are fp64 only (kstar_fp32)";
  const double *d_X, *d_Xi, *d_Xa;
  bool has_operands() const { return d_X && d_Xi; }
  int check(ppbo_ctx* ctx, const ppbo_model* model) {
    PPBO_REQUIRE(ctx, model->kernel_id != PPBO_KERNEL_MATERN32,
                 "no curvature for Matern-3/2 (its sample paths are differentiable once only)");
    PPBO_REQUIRE(ctx, d_Xa == nullptr || (model->D <= KSTAR_CURV_ACC_MAX_DP && model->kernel_id != PPBO_KERNEL_CAMPHOR),
                 "accelerations (d_Xa): D <= 16 and not the camphor-copper kernel");
    return 0;
  }
  template <int KID>
  void kstar(const KstarLaunch& k, int64_t c_beg, int Mc) const {
    const size_t o = (size_t)c_beg * k.m->D;
    if constexpr (KID != PPBO_KERNEL_MATERN32) launch_kstar_curv<KID>(k, d_X + o, d_Xi + o, d_Xa ? d_Xa + o : nullptr, Mc);
  }
  template <int KID>
  void score(const TwoSetScore& sc) const {
    const size_t o = (size_t)sc.c_beg * sc.m->D;
    if constexpr (KID != PPBO_KERNEL_MATERN32)
      curv_score_kernel<KID><<<sc.sblocks, SC_THREADS, 0, sc.s>>>(sc.mu_part, sc.n_split, sc.t_part, sc.slab, sc.ntm, sc.Mc,
                                                                  d_Xi + o, d_Xa ? d_Xa + o : nullptr, sc.m->D, sc.p,
                                                                  sc.score_kind, sc.c_beg, sc.d_mu, sc.d_var, sc.d_prob,
                                                                  sc.d_score, sc.bests);
  }
};
int ppbo_predict_curvatures(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, const double* d_Xi, const double* d_Xa,
                            int64_t M, int score_kind, double* d_mu, double* d_var, double* d_prob, double* d_score,
                            double* h_best_val, int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  CurvaturesPred pr{{}, d_X, d_Xi, d_Xa};
  return two_set_passes(ctx, model, pr, M, score_kind, d_mu, d_var, d_prob, d_score, h_best_val, h_best_idx, (hipStream_t)stream);
}

// Functionals: the column c = sum_g w_g k(x_g, X) of L f = sum_g w_g f(x_g) for M groups of G points, d_Xg [M, G, D], with
// the weights d_w ([G], or [M, G]): ONE contraction per group whatever G is; kstar_func -> quadform -> functional_score.
// The groups' prior terms take one more row of the partial-sum workspace.  The K* launches share the "kstar" profile slot.
struct FunctionalsPred : TwoSetBase {
  static constexpr const char* operands = "functionals (d_Xg / d_w)";
  static constexpr const char* fp64_only = "functionals are fp64 only (kstar_fp32)";
  static constexpr int extra_part_rows = 1;
  const double *d_Xg, *d_w;
  int w_stride, G;
  double threshold;
  bool has_operands() const { return d_Xg && d_w; }
  int check(ppbo_ctx* ctx, const ppbo_model*) {
    PPBO_REQUIRE(ctx, G >= 1 && G <= PPBO_FUNCTIONAL_MAX_G, "G (1 .. PPBO_FUNCTIONAL_MAX_G points per group)");
    PPBO_REQUIRE(ctx, w_stride == 0 || w_stride == G, "w_stride (0: one weight row for all groups, G: one per group)");
    PPBO_REQUIRE(ctx, std::isfinite(threshold), "threshold (finite)");
    return 0;
  }
  template <int KID>
  void kstar(const KstarLaunch& k, int64_t c_beg, int Mc) const {
    launch_kstar_func<KID>(k, d_Xg + (size_t)c_beg * k.m->D * G, d_w + (size_t)c_beg * w_stride, w_stride, G, Mc);
  }
  template <int KID>
  void score(const TwoSetScore& sc) const {
    const int D = sc.m->D;
    if (sc.slab) {
      // one wavefront per group; as many per workgroup (4, 2, 1) as 48 KB of LDS hold of G (D + 1) doubles each
      const size_t per_wave = (size_t)G * (D + 1) * sizeof(double);
      const int wpb = 4 * per_wave <= 49152 ? 4 : (2 * per_wave <= 49152 ? 2 : 1);
      functional_prior_kernel<KID><<<(sc.Mc + wpb - 1) / wpb, 64 * wpb, wpb * per_wave, sc.s>>>(
          d_Xg + (size_t)sc.c_beg * D * G, d_w + (size_t)sc.c_beg * w_stride, w_stride, G, D, sc.Mc, sc.p, sc.extra);
    }
    functional_score_kernel<<<sc.sblocks, SC_THREADS, 0, sc.s>>>(sc.mu_part, sc.n_split, sc.t_part, sc.slab, sc.ntm, sc.Mc,
                                                                 sc.extra, threshold, sc.score_kind, sc.c_beg, sc.d_mu,
                                                                 sc.d_var, sc.d_prob, sc.d_score, sc.bests);
  }
};
int ppbo_predict_functionals(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xg, const double* d_w, int w_stride,
                             int64_t M, int G, double threshold, int score_kind, double* d_mu, double* d_var,
                             double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  FunctionalsPred pr{{}, d_Xg, d_w, w_stride, G, threshold};
  return two_set_passes(ctx, model, pr, M, score_kind, d_mu, d_var, d_prob, d_score, h_best_val, h_best_idx, (hipStream_t)stream);
}

// Main effects and interactions: the column c_j = P_j F(r_d, r_e) of f with every axis but at most two averaged over the
// unit box.  The rows of the call are d_dims / d_t [M, 2]; the column comes from the caller's axes and the table
// marginal_table_kernel leaves per call, not from model->d_X; kstar_marginal -> quadform -> marginal_score.  Its row
// splits are those of a FULL chunk whatever M is, so that a row's sums do not depend on the size of the call.  The K*
// launches share the "kstar" profile slot.
struct MarginalsPred : TwoSetBase {
  static constexpr const char* operands = "marginals (d_dims / d_t)";
  static constexpr const char* fp64_only = "marginals are fp64 only (kstar_fp32)";
  static constexpr bool full_chunk_splits = true;
  MargArgs ma;
  double* tab = nullptr;
  bool has_operands() const { return ma.d_dims && ma.d_t; }
  int check(ppbo_ctx* ctx, const ppbo_model* model) {
    PPBO_REQUIRE(ctx, model->kernel_id == PPBO_KERNEL_SE || model->kernel_id == PPBO_KERNEL_CAMPHOR,
                 "marginals need a kernel that is a product over coordinates (SE, camphor-copper); RQ and Matern: sample with "
                 "ppbo_predict_functionals (average_pred)");
    PPBO_REQUIRE(ctx, ma.effect == PPBO_EFFECT_RAW || ma.effect == PPBO_EFFECT_CENTRED || ma.effect == PPBO_EFFECT_INTERACTION,
                 "effect");
    if (int rc = marginal_axes_arg(ctx, &ma)) return rc;
    const bool six = model->kernel_id == PPBO_KERNEL_CAMPHOR || model->coords.kind == PPBO_COORDS_CAMPHOR;
    PPBO_REQUIRE(ctx, ma.ax->Dc == (six ? 6 : model->D), "axes->Dc: the model's D (6 for the camphor kernels)");
    return 0;
  }
  int prepare(ppbo_ctx* ctx, const ppbo_model* model, const KernParams& p, int64_t M, Best* bests, int sblocks_max, hipStream_t s) {
    const int N = model->N;
    tab = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_MARGINAL, marginal_table_doubles(N, ma.arg.Dc) * sizeof(double));
    if (!tab) return (int)hipErrorOutOfMemory;
    // the rows of d_dims are looked at on the device BEFORE anything is launched on the outputs: the first row that breaks
    // the rules comes back through the host-mapped record.  A stream that is being captured cannot be waited on: there
    // the look is left out, and such a row gets NaN results (marginal_row)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    if (cap == hipStreamCaptureStatusNone) {
      PpboHostRecord chk{};
      if (int rc = ppbo_host_record(ctx, &chk)) return rc;
      const int cblocks = (int)std::min<int64_t>((M + 255) / 256, (int64_t)sblocks_max);
      marginal_check_kernel<<<cblocks, 256, 0, s>>>(ma.d_dims, (long long)M, ma.arg.Dc, ma.effect, bests);
      PPBO_LAUNCH_CHECK(ctx);
      argmax_final_kernel<<<1, 256, 0, s>>>(bests, cblocks, nullptr, chk.d_rec, 0, chk.d_flag, chk.epoch);
      PPBO_LAUNCH_CHECK(ctx);
      if (int rc = ppbo_host_record_wait(ctx, chk, s)) return rc;
      const long long bad = (long long)chk.h_rec[1];
      if (bad >= 0)
        return ppbo_set_error(ctx, -1,
                              "invalid argument: d_dims row %lld (axes in -1 .. Dc - 1, two different ones, no first axis of -1 "
                              "with a second one, two axes for an interaction)", bad);
    }
    marginal_table_kernel<<<(N + 255) / 256, 256, 0, s>>>(ma.arg, ma.ax->d_Xu, N, p.sf2, tab);
    PPBO_LAUNCH_CHECK(ctx);
    return 0;
  }
  template <int KID>
  void kstar(const KstarLaunch& k, int64_t c_beg, int Mc) const {
    const int Dc = ma.arg.Dc;
    kstar_marginal_kernel<<<k.grid(Mc, KS_THREADS), KS_THREADS, (size_t)2 * KS_RJ * Dc * sizeof(double), k.s>>>(
        ma.ax->d_Xu, k.m->N, Dc, tab, k.m->d_alpha, k.lam_diag(), k.lam_off(), k.mblk(), ma.d_dims + (size_t)c_beg * 2,
        ma.d_t + (size_t)c_beg * 2, ma.effect, Mc, k.Kt, k.ldk, k.mu_part, k.t_or_null(), k.q_per_split, k.n_q(), k.edge_k0);
  }
  template <int KID>
  void score(const TwoSetScore& sc) const {
    marginal_score_kernel<<<sc.sblocks, SC_THREADS, 0, sc.s>>>(
        sc.mu_part, sc.n_split, sc.t_part, sc.slab, sc.ntm, sc.Mc, ma.d_dims + (size_t)sc.c_beg * 2, ma.d_t + (size_t)sc.c_beg * 2,
        tab, ma.arg.Dc, sc.p.sf2, ma.prod_A, ma.effect, sc.score_kind, sc.c_beg, sc.d_mu, sc.d_var, sc.d_prob, sc.d_score, sc.bests);
  }
};
int ppbo_predict_marginals(ppbo_ctx* ctx, const ppbo_model* model, const ppbo_marginal_axes* axes, const int* d_dims,
                           const double* d_t, int64_t M, int effect, int score_kind, double* d_mu, double* d_var,
                           double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  MarginalsPred pr{{}, MargArgs{axes, d_dims, d_t, effect, {}, 0.0}};
  return two_set_passes(ctx, model, pr, M, score_kind, d_mu, d_var, d_prob, d_score, h_best_val, h_best_idx, (hipStream_t)stream);
}

extern "C" {

// The field pass of a tournament: U [NkU][ldu] = u_b = (Lambda + M'M) k_b for the Mb opponents d_Xb, in the row layout of the
// model's form (see tournament_kernel).  KB, Y, Z: [N][ldu] each; part_b: the mean partials of the field's own K* launch
// (not read).  Touches no workspace of predict_passes.  ppbo_search_batch runs it per pick with Mb = 1.  FieldPass is
// declared in common.h for acq.hip, which pins the tile configuration of the two GEMMs (gemm_cfg = GemmArgs.force_cfg).
double* FieldPass::prepare(ppbo_ctx* ctx, const ppbo_model* m, int Mb_max, const RowSplit& rs, size_t extra_doubles,
                           size_t head_doubles) {
  model = m;
  split = rs;
  const int N = m->N;
  NkU = (N + BK - 1) & ~(BK - 1);            // rows of U: the K extent of a padded chunk workspace
  ldu = (Mb_max + 127) & ~127;               // whole opponent tiles
  // every workspace before the first launch (growing one waits for the device)
  U = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_TOURN_U, (size_t)NkU * ldu * sizeof(double));
  if (!U) return nullptr;
  const size_t f_y = (size_t)N * ldu, f_part = 3 * f_y + head_doubles, f_extra = f_part + (size_t)rs.n_split_eff * Mb_max;
  KB = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_TOURN_FIELD, (f_extra + extra_doubles) * sizeof(double));
  if (!KB) return nullptr;
  Y = KB + f_y; Z = Y + f_y; head = Z + f_y; part = KB + f_part;
  return KB + f_extra;
}

int FieldPass::run(ppbo_ctx* ctx, const double* d_Xb, int Mb, hipStream_t s, int gemm_cfg) const {
  const int N = model->N, mblk = model->m + 1, n_q = N / mblk;
  const bool edge = model->form == PPBO_FORM_EDGE;
  PPBO_HIP_CHECK(ctx, hipMemsetAsync(U, 0, (size_t)NkU * ldu * sizeof(double), s));
  dispatch_kstar(model, d_Xb, Mb, KB, ldu, part, nullptr, split.q_per_split, split.n_split_eff, false, s);
  PPBO_LAUNCH_CHECK(ctx);
  GemmArgs y{};
  y.A = model->d_G; y.lda = N; y.B = KB; y.ldb = ldu; y.C = Y; y.ldc = ldu;
  y.M = N; y.N = Mb; y.K = N; y.alpha = 1.0; y.beta = 0.0; y.khi_mode = 1; y.tri_block = mblk;
  y.force_cfg = gemm_cfg;
  if (edge) {
    edge_apply_kernel<<<dim3((Mb + 127) / 128, N), 128, 0, s>>>(KB, ldu, Mb, mblk, n_q, model->d_lam_off, Z);
    PPBO_LAUNCH_CHECK(ctx);
    tournament_delta_kernel<<<dim3((Mb + 127) / 128, N), 128, 0, s>>>(KB, ldu, Mb, mblk, n_q, U);
    PPBO_LAUNCH_CHECK(ctx);
    y.B = Z; y.tri_block = 1;    // H lower triangular
  } else {
    lam_apply_kernel<<<dim3((Mb + 127) / 128, n_q), 128, 0, s>>>(KB, ldu, N, Mb, mblk, model->d_lam_diag, model->d_lam_off, U);
    PPBO_LAUNCH_CHECK(ctx);
  }
  if (int rc = ppbo_gemm_launch(ctx, y, 0, 0, s)) return rc;       // Y = G K*_B  (H E_B)
  GemmArgs u{};
  u.A = model->d_G; u.lda = N; u.B = Y; u.ldb = ldu; u.C = U; u.ldc = ldu;
  u.M = N; u.N = Mb; u.K = N; u.alpha = 1.0; u.beta = 1.0; u.tri_block = 1;
  u.force_cfg = gemm_cfg;
  if (int rc = ppbo_gemm_launch(ctx, u, 1, 0, s)) return rc;       // U += G' Y
  return 0;
}

// Tournaments: every candidate a_i against every opponent b_j.  Field pass once per call (ppbo_predict's own launches on
// d_Xb for mu_b / var_b, then K*_B in the node layout -> U, see tournament_kernel), then per chunk of 65536 candidates
// ppbo_predict's own launches (predict_passes: mu_a, var_a and the chunk's K* workspace) -> tournament_kernel ->
// tournament_finish_kernel -> one-workgroup argmax.  A model that the one-launch scoring kernel takes leaves no K* in
// memory: there the chunks' K* are formed by a K* launch of their own, behind the scoring launch.
// With `kg` (ppbo_predict_kg) the same stages run, tournament_kernel writes the chunk's covariances into a workspace
// [Mc][Mb] behind the field's, and the envelope march of kg.hip stands where tournament_finish_kernel does: its
// per-workgroup bests feed the same one-workgroup argmax.
struct KgRequest {
  double noise_var;   // tau^2 of the imagined observation
  double* d_kg;       // [Ma]
  int* d_kinks;       // [Ma], may be NULL
};
static int tournament_passes(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, int64_t Ma, const double* d_Xb, int Mb,
                             int score_kind, double* d_mu_a, double* d_var_a, double* d_mu_b, double* d_var_b, double* d_cov,
                             double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx, hipStream_t s,
                             const KgRequest* kg) {
  if (int rc = check_model(ctx, model)) return rc;
  PPBO_REQUIRE(ctx, d_Xa != nullptr && d_Xb != nullptr, "tournament (d_Xa / d_Xb)");
  PPBO_REQUIRE(ctx, Ma >= 1 && Ma <= (int64_t)0x7fffffff, "candidate count (1 .. 2^31 - 1)");
  PPBO_REQUIRE(ctx, Mb >= 1 && Mb <= PPBO_TOURNAMENT_MAX_B, "opponent count (1 .. PPBO_TOURNAMENT_MAX_B; chunk the field)");
  PPBO_REQUIRE(ctx, score_kind == PPBO_TOURNAMENT_BORDA || score_kind == PPBO_TOURNAMENT_WORST, "score_kind");
  PPBO_REQUIRE(ctx, !model->kstar_fp32, "tournaments are fp64 only (kstar_fp32)");
  PPBO_REQUIRE(ctx, model->d_G != nullptr, "tournaments need model->d_G");
  PPBO_REQUIRE(ctx, model->d_lam_diag && model->d_lam_off, "model Lambda");
  const bool want_best = h_best_val || h_best_idx;
  const int N = model->N, D = model->D, mblk = model->m + 1, n_q = N / mblk;
  const bool edge = model->form == PPBO_FORM_EDGE;
  const int kshift = edge ? ppbo_edge_k0(n_q) : 0;
  const KernParams p = make_kern_params(model->kernel_id, model->theta);
  const double two_sigma2 = 2.0 * model->theta[0] * model->theta[0];
  const Chunks ck(Ma);
  const int Mc_max = ck.Mc_max;
  // camphor-copper always takes the small tile: its sin(pi |dx|) per element and coordinate needs more registers than
  // the 128 a lane of the 16-wavefront shape has (the compiler spilled 116 bytes per lane there)
  const bool small = Mb <= 2 * TQ_SMALL::BN || model->kernel_id == PPBO_KERNEL_CAMPHOR;
  const int ntb = small ? (Mb + TQ_SMALL::BN - 1) / TQ_SMALL::BN : (Mb + TQ_BIG::BN - 1) / TQ_BIG::BN;
  const int ldu = (Mb + 127) & ~127;                   // whole opponent tiles
  const int fblocks_max = kg ? (int)ppbo_kg_blocks(Mc_max, Mb) : (Mc_max + 255) / 256;
  // behind the field's arrays (mu_b, var_b [ldu] each in front of its partials): slabs, mu_a / var_a where the caller has
  // none, the bests (a Best is 16 bytes), the knowledge gradient's chunk covariances [Mc][Mb], s_i and own slopes [Mc] each
  const size_t f_mua = (size_t)2 * ntb * Mc_max, f_bests = f_mua + (size_t)(d_mu_a ? 0 : Ma) + (size_t)(d_var_a ? 0 : Ma),
               f_kg = f_bests + (size_t)2 * (fblocks_max + ck.n), f_end = f_kg + (kg ? (size_t)Mc_max * Mb + (size_t)2 * Mc_max : 0);
  FieldPass field;                 // (the split of the field's own K* launch, whose mean partials are not read)
  double* fw = field.prepare(ctx, model, Mb, row_split(Mb, n_q), f_end, (size_t)2 * ldu);
  if (!fw) return (int)hipErrorOutOfMemory;
  double *kg_cov = fw + f_kg, *kg_s = kg_cov + (size_t)Mc_max * Mb, *kg_self_b = kg_s + Mc_max;
  double *mu_b = field.head, *var_b = mu_b + ldu;
  double *slab_sum = fw, *slab_min = slab_sum + (size_t)ntb * Mc_max;
  double* mu_a = d_mu_a ? d_mu_a : fw + f_mua;
  double* var_a = d_var_a ? d_var_a : fw + f_mua + (d_mu_a ? 0 : Ma);
  Best* bests = reinterpret_cast<Best*>(fw + f_bests);
  Best* chunk_best = bests + fblocks_max;
  BestReturn br;
  if (int rc = br.begin(ctx, want_best)) return rc;

  // ---- the field, once per call
  // mu_b, var_b: exactly ppbo_predict's launches on d_Xb
  PredictRequest rq_b{d_Xb, Mb, PPBO_SCORE_MEAN, 0.0, mu_b, var_b};
  if (int rc = rq_b.predict_passes(ctx, model, s)) return rc;
  if (d_mu_b) PPBO_HIP_CHECK(ctx, hipMemcpyAsync(d_mu_b, mu_b, (size_t)Mb * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (d_var_b) PPBO_HIP_CHECK(ctx, hipMemcpyAsync(d_var_b, var_b, (size_t)Mb * sizeof(double), hipMemcpyDeviceToDevice, s));
  {
    PpboProfScope pf(ctx, ppbo_ctx::PF_TOURNAMENT_FIELD, s);
    if (int rc = field.run(ctx, d_Xb, Mb, s)) return rc;
  }

  // ---- the candidates: per chunk behind ppbo_predict's own launches
  // one chunk with its K* workspace Kc [Nk][ldk] in the layout of the model's form
  auto chunk = [&](int64_t c_beg, int Mc, const double* Kc, int ldk, int Nk, int ch) -> int {
    const double* xa = d_Xa + (size_t)c_beg * D;
    const int kext = Nk - kshift;
    {
      PpboProfScope pf(ctx, ppbo_ctx::PF_TOURNAMENT, s);
      if (int rc = ppbo_kernel_dispatch(ctx, model->kernel_id, [&](auto kid) {
            constexpr int KID = decltype(kid)::value;
            const double* Ks = Kc + (size_t)kshift * ldk;
            const double* Us = field.U + (size_t)kshift * ldu;
            double* cov = kg ? kg_cov : (d_cov ? d_cov + (size_t)c_beg * Mb : nullptr);
            double* prob = d_prob ? d_prob + (size_t)c_beg * Mb : nullptr;
            if (small)
              return launch_tournament<TQ_SMALL, KID>(ctx, Ks, ldk, Us, ldu, kext, Mc, Mb, xa, d_Xb, D, p, two_sigma2, mu_a + c_beg,
                                                      var_a + c_beg, mu_b, var_b, cov, prob, slab_sum, slab_min, s);
            if constexpr (KID == PPBO_KERNEL_CAMPHOR) return -1;      // (not reached: `small` above)
            else
              return launch_tournament<TQ_BIG, KID>(ctx, Ks, ldk, Us, ldu, kext, Mc, Mb, xa, d_Xb, D, p, two_sigma2, mu_a + c_beg,
                                                    var_a + c_beg, mu_b, var_b, cov, prob, slab_sum, slab_min, s);
          }))
        return rc;
    }
    const int fblocks = kg ? (int)ppbo_kg_blocks(Mc, Mb) : (Mc + 255) / 256;
    if (kg) {
      // lines of candidate i: the field's, intercept mu_b[j] and slope cov[i][j] / s_i, and its own (mu_a[i], v_i / s_i)
      PpboProfScope pf(ctx, ppbo_ctx::PF_KG, s);
      if (int rc = ppbo_kg_rows(ctx, var_a + c_beg, kg->noise_var, Mc, kg_s, kg_self_b, s)) return rc;
      if (int rc = ppbo_kg_launch(ctx, mu_b, kg_cov, Mb, kg_s, mu_a + c_beg, kg_self_b, Mc, Mb, (long long)c_beg,
                                  kg->d_kg + c_beg, kg->d_kinks ? kg->d_kinks + c_beg : nullptr,
                                  want_best ? bests : nullptr, s, xa, d_Xb, D))
        return rc;
    } else {
      tournament_finish_kernel<<<fblocks, 256, 0, s>>>(slab_sum, slab_min, ntb, Mc, Mb, score_kind, (long long)c_beg,
                                                       d_score ? d_score + c_beg : nullptr, want_best ? bests : nullptr);
      PPBO_LAUNCH_CHECK(ctx);
    }
    return br.chunk(ctx, bests, fblocks, chunk_best, ch, ck, s);
  };
  const PredictChunkHook hook = [&](int64_t c_beg, int64_t Mh, const double* Kc, int ldk, int Nk) -> int {
    if (Kc) return chunk(c_beg, (int)Mh, Kc, ldk, Nk, (int)(c_beg / ck.cap));
    // the one-launch path (node form): mu_a / var_a of all rows are enqueued; K* of each chunk by a launch of its own
    OwnKstar k1;
    if (int rc = k1.prepare(ctx, ppbo_ctx::WS_TOURN_K, model, field.NkU, Mc_max, 1, true, s)) return rc;
    for (const Chunk c : ck) {
      if (int rc = k1.form(ctx, model, d_Xa + (size_t)c.beg * D, c.Mc, s)) return rc;
      if (int rc = chunk(c.beg, c.Mc, k1.K, k1.ldk, field.NkU, (int)c.ch)) return rc;
    }
    return 0;
  };
  PredictRequest rq_a{d_Xa, Ma, PPBO_SCORE_MEAN, 0.0, mu_a, var_a};
  rq_a.after_chunk = &hook;
  if (int rc = rq_a.predict_passes(ctx, model, s)) return rc;
  return br.finish(ctx, chunk_best, ck, s, h_best_val, h_best_idx);
}

int ppbo_predict_tournament(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, int64_t Ma, const double* d_Xb, int Mb,
                            int score_kind, double* d_mu_a, double* d_var_a, double* d_mu_b, double* d_var_b, double* d_cov,
                            double* d_prob, double* d_score, double* h_best_val, int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  return tournament_passes(ctx, model, d_Xa, Ma, d_Xb, Mb, score_kind, d_mu_a, d_var_a, d_mu_b, d_var_b, d_cov, d_prob, d_score,
                           h_best_val, h_best_idx, (hipStream_t)stream, nullptr);
}

// The knowledge gradient of every candidate a_i over the field B: the tournament's stages with the envelope march
// (kg.hip) behind each chunk's cross product, see tournament_passes.
int ppbo_predict_kg(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xa, int64_t Ma, const double* d_Xb, int Mb,
                    double noise_var, double* d_kg, int* d_kinks, double* d_mu_a, double* d_var_a, double* d_mu_b,
                    double* d_var_b, double* h_best_val, int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_kg != nullptr, "knowledge gradient (d_kg)");
  PPBO_REQUIRE(ctx, noise_var >= 0.0 && noise_var <= 1.7976931348623157e308, "noise_var (finite, >= 0)");
  const KgRequest kg{noise_var, d_kg, d_kinks};
  return tournament_passes(ctx, model, d_Xa, Ma, d_Xb, Mb, PPBO_TOURNAMENT_BORDA, d_mu_a, d_var_a, d_mu_b, d_var_b, nullptr,
                           nullptr, nullptr, h_best_val, h_best_idx, (hipStream_t)stream, &kg);
}

// Shortlists: q greedy picks under the conditioned variance (batch_step_kernel and its neighbours, above).  ppbo_predict's
// own launches give mu, var_0 and pick 0; then per pick gather -> field pass on the one gathered row -> one streaming pass
// over the candidates' K* -> one-workgroup argmax -> record.  One chunk (M <= 65536): the K* workspace predict_passes
// left (or, behind the one-launch scoring path, one K* launch of this entry's own) serves every pick.  More chunks: every
// chunk's K* is formed again per pick in a workspace of this entry's own.  Everything is enqueued; the host waits once,
// for the copy of the q records.
int ppbo_search_batch(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind, double mustar,
                      double noise_var, int q, int64_t* h_idx, double* h_score, double* d_mu, double* d_var,
                      double* d_var_cond, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_model(ctx, model)) return rc;
  PPBO_REQUIRE(ctx, d_Xc != nullptr && h_idx != nullptr, "shortlist (d_Xc / h_idx)");
  PPBO_REQUIRE(ctx, M >= 1 && M <= (int64_t)0x7fffffff, "candidate count (1 .. 2^31 - 1)");
  PPBO_REQUIRE(ctx, q >= 1 && q <= PPBO_BATCH_MAX_Q, "q (1 .. PPBO_BATCH_MAX_Q)");
  PPBO_REQUIRE(ctx, noise_var >= 0.0 && noise_var <= 1.7976931348623157e308, "noise_var (finite, >= 0)");
  PPBO_REQUIRE(ctx, score_kind == PPBO_SCORE_POINTWISE_EI || score_kind == PPBO_SCORE_VARIANCE,
               "score_kind (EI or VARIANCE: the mean does not change under this conditioning)");
  PPBO_REQUIRE(ctx, !model->kstar_fp32, "shortlists are fp64 only (kstar_fp32)");
  PPBO_REQUIRE(ctx, model->d_G != nullptr, "shortlists need model->d_G");
  PPBO_REQUIRE(ctx, model->d_lam_diag && model->d_lam_off, "model Lambda");
  const int N = model->N, D = model->D, mblk = model->m + 1, n_q = N / mblk;
  const bool edge = model->form == PPBO_FORM_EDGE;
  const int kshift = edge ? ppbo_edge_k0(n_q) : 0;
  const KernParams p = make_kern_params(model->kernel_id, model->theta);
  const Chunks ck(M);
  const int Mc_max = ck.Mc_max;
  const int blocks_max = batch_blocks(Mc_max);
  // the last step only finishes var_q: without d_var_cond nobody reads it
  const int n_steps = d_var_cond ? q : q - 1;
  // every workspace of this entry before the first launch (growing one waits for the device); the field pass of one
  // opponent: a whole opponent tile
  FieldPass field;
  if (!field.prepare(ctx, model, 1, row_split(1, n_q), 0)) return (int)hipErrorOutOfMemory;
  const int NkU = field.NkU, ldu = field.ldu;
  const double* U = field.U;
  const size_t b_rec = 0, b_picks = b_rec + 2 * (size_t)q, b_xp = b_picks + q, b_vp = b_xp + 64, b_pv = b_vp + PPBO_BATCH_MAX_Q,
               b_uc = b_pv + 2, b_bests = b_uc + NkU, b_mu = b_bests + 2 * (size_t)(blocks_max + ck.n),   // (a Best is 16 bytes)
               b_var = b_mu + (size_t)(d_mu ? 0 : M), b_varw = b_var + (size_t)(d_var ? 0 : M),
               b_V = b_varw + (size_t)(d_var_cond ? 0 : M), b_end = b_V + (size_t)(n_steps > 0 ? n_steps : 1) * (size_t)M;
  double* bw = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_BATCH, b_end * sizeof(double));
  if (!bw) return (int)hipErrorOutOfMemory;
  double* rec = bw + b_rec;
  long long* picks = reinterpret_cast<long long*>(bw + b_picks);
  double *xp = bw + b_xp, *vp = bw + b_vp, *pv = bw + b_pv, *uc = bw + b_uc;
  Best* bests = reinterpret_cast<Best*>(bw + b_bests);
  Best* step_best = bests + blocks_max;
  double* mu = d_mu ? d_mu : bw + b_mu;
  double* var = d_var ? d_var : bw + b_var;
  double* varw = d_var_cond ? d_var_cond : bw + b_varw;
  double* V = bw + b_V;
  double* hrec = (double*)ppbo_pinned(ctx, (size_t)2 * q * sizeof(double));
  if (!hrec) return ppbo_set_error(ctx, (int)hipErrorOutOfMemory, "pinned staging");

  // ---- mu, var_0 and pick 0: exactly ppbo_predict's launches; a single chunk's K* workspace stays for the picks
  const double* Kr = nullptr;
  int ldk = 0, kext = 0;
  const PredictChunkHook hook = [&](int64_t, int64_t, const double* Kc, int ldk_c, int Nk_c) -> int {
    if (Kc && ck.n == 1) { Kr = Kc + (size_t)kshift * ldk_c; ldk = ldk_c; kext = Nk_c - kshift; }
    return 0;
  };
  PredictRequest rq{d_Xc, M, score_kind, mustar, mu, var};
  rq.want_best = true; rq.after_chunk = &hook;
  if (int rc = rq.predict_passes(ctx, model, s)) return rc;
  best_record_kernel<<<1, 64, 0, s>>>(rq.chunk_best, rq.n_chunks, 0, rec);
  PPBO_LAUNCH_CHECK(ctx);
  if (Kr && kext > NkU - kshift) return ppbo_set_error(ctx, -1, "shortlist: the K* workspace is deeper than the field's U");

  // ---- a K* workspace of this entry's own where predict_passes left none that lasts
  OwnKstar k2;
  if (!Kr && n_steps > 0) {
    if (int rc = k2.prepare(ctx, ppbo_ctx::WS_BATCH_K, model, NkU, Mc_max, 2, false, s)) return rc;
    ldk = k2.ldk;
    kext = N - kshift;
  }
  const double* const K2 = k2.K;
  // K* of one chunk in the layout of the model's form (the partial sums of its mean and Lambda term are not read)
  auto form_kstar = [&](const Chunk& c) { return k2.form(ctx, model, d_Xc + (size_t)c.beg * D, c.Mc, s, edge ? kshift : -1); };
  if (K2 && ck.n == 1) {
    if (int rc = form_kstar(ck.at(0))) return rc;
    Kr = K2 + (size_t)kshift * ldk;
  }
  if (n_steps > 0) PPBO_HIP_CHECK(ctx, hipMemcpyAsync(varw, var, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice, s));

  // ---- the picks
  for (int j = 0; j < n_steps; ++j) {
    {
      PpboProfScope pf(ctx, ppbo_ctx::PF_BATCH_FIELD, s);
      batch_gather_kernel<<<1, 64, 0, s>>>(rec + 2 * j, d_Xc, D, varw, V, (long long)M, j, noise_var, picks, xp, vp, pv);
      PPBO_LAUNCH_CHECK(ctx);
      if (int rc = field.run(ctx, xp, 1, s)) return rc;
      batch_ucol_kernel<<<(kext + 255) / 256, 256, 0, s>>>(U + (size_t)kshift * ldu, ldu, kext, uc);
      PPBO_LAUNCH_CHECK(ctx);
    }
    for (const Chunk c : ck) {
      const double* Ks = Kr;
      if (ck.n > 1) {
        if (int rc = form_kstar(c)) return rc;
        Ks = K2 + (size_t)kshift * ldk;
      }
      PpboProfScope pf(ctx, ppbo_ctx::PF_BATCH_STEP, s);
      const int blocks = batch_blocks(c.Mc);
      if (ldk % 2 != 0 || ldk < blocks * BS_CAND || (reinterpret_cast<uintptr_t>(Ks) & 15) != 0)
        return ppbo_set_error(ctx, -1, "shortlist: the K* workspace is not laid out for 16-byte loads");
      if (int rc = ppbo_kernel_dispatch(ctx, model->kernel_id, [&](auto kid) {
            constexpr int KID = decltype(kid)::value;
            batch_step_kernel<KID><<<blocks, SC_THREADS, 0, s>>>(Ks, ldk, kext, uc, d_Xc, D, p, c.Mc, (long long)c.beg, (long long)M,
                                                                 mu, varw, V, j, vp, pv, picks, xp, score_kind, mustar, bests);
            return 0;
          }))
        return rc;
      PPBO_LAUNCH_CHECK(ctx);
      if (j + 1 < q) {
        argmax_final_kernel<<<1, 256, 0, s>>>(bests, blocks, step_best + c.ch);
        PPBO_LAUNCH_CHECK(ctx);
      }
    }
    if (j + 1 < q) {
      best_record_kernel<<<1, 64, 0, s>>>(step_best, (int)ck.n, 0, rec + 2 * (j + 1));
      PPBO_LAUNCH_CHECK(ctx);
    }
  }
  PPBO_HIP_CHECK(ctx, hipMemcpyAsync(hrec, rec, (size_t)2 * q * sizeof(double), hipMemcpyDeviceToHost, s));
  PPBO_HIP_CHECK(ctx, hipStreamSynchronize(s));
  for (int j = 0; j < q; ++j) {
    h_idx[j] = (int64_t)hrec[2 * j + 1];            // (NaN, -1) from the first pick that found nothing left
    if (h_score) h_score[j] = hrec[2 * j];
  }
  return 0;
}

}  // extern "C"

// internal (dist.hip): ppbo_predict_record whose record lives in host-mapped memory, the flag raised after it
int ppbo_predict_record_publish(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                                double mustar, int64_t index_offset, double* d_record, unsigned long long* d_flag,
                                unsigned long long epoch, hipStream_t s) {
  PredictRequest rq{d_Xc, M, score_kind, mustar};
  rq.projected = true; rq.want_best = true; rq.d_record = d_record; rq.record_offset = index_offset; rq.publish = d_flag; rq.epoch = epoch;
  return rq.predict_passes(ctx, model, s);
}

// internal (project.hip): edge_apply_kernel on the caller's stream -- E [N][ld] = the edge-layout rows of Kt [N][ld]
int ppbo_edge_apply_async(ppbo_ctx* ctx, const double* Kt, int ld, int M, int N, int mblk, const double* d_lam_off, double* E,
                          hipStream_t s) {
  edge_apply_kernel<<<dim3((M + 127) / 128, N), 128, 0, s>>>(Kt, ld, M, mblk, N / mblk, d_lam_off, E);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" {

int ppbo_predict_cov(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int M, double shrink,
                     double* d_mu, double* d_cov, void* stream) {
  PPBO_ENTER(ctx);
  if (int rc = check_model(ctx, model)) return rc;
  PPBO_REQUIRE(ctx, d_Xc && d_cov && M > 0 && M <= 16384, "candidates (M <= 16384 for a full covariance)");
  PPBO_REQUIRE(ctx, model->d_G && model->d_lam_diag && model->d_lam_off, "model G/Lambda");
  hipStream_t s = (hipStream_t)stream;
  const int N = model->N, mblk = model->m + 1, n_q = N / mblk;
  const int ld = (M + 1) & ~1;
  double* ws = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_KSTAR, (size_t)3 * N * ld * sizeof(double));
  if (!ws) return (int)hipErrorOutOfMemory;
  double* Kt = ws;
  double* Z = ws + (size_t)N * ld;
  double* Y = ws + (size_t)2 * N * ld;
  const RowSplit rs = row_split(M, n_q);
  const int q_per_split = rs.q_per_split, n_split_eff = rs.n_split_eff;
  double* part = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_PART, (size_t)n_split_eff * M * sizeof(double));
  if (!part) return (int)hipErrorOutOfMemory;
  dispatch_kstar(model, d_Xc, M, Kt, ld, part, nullptr, q_per_split, n_split_eff, false, s);
  PPBO_LAUNCH_CHECK(ctx);
  if (d_mu) {
    score_kernel<<<score_blocks(M), SC_THREADS, 0, s>>>(part, n_split_eff, nullptr, nullptr, 0, M, 0.0, PPBO_SCORE_MEAN,
                                                        0.0, 0, d_mu, nullptr, nullptr, nullptr);
    PPBO_LAUNCH_CHECK(ctx);
  }
  // prior block with the reference's shrinkage (gp_model.py:447)
  if (int rc = ppbo_gram(ctx, model->kernel_id, d_Xc, M, model->D, model->theta, shrink, d_cov, stream)) return rc;
  // + K*' Lambda K*
  lam_apply_kernel<<<dim3((M + 127) / 128, n_q), 128, 0, s>>>(Kt, ld, N, M, mblk, model->d_lam_diag,
                                                              model->d_lam_off, Z);
  PPBO_LAUNCH_CHECK(ctx);
  GemmArgs g{};
  g.A = Kt; g.lda = ld; g.B = Z; g.ldb = ld; g.C = d_cov; g.ldc = M;
  g.M = M; g.N = M; g.K = N; g.alpha = 1.0; g.beta = 1.0; g.tri_block = 1;
  if (int rc = ppbo_gemm_launch(ctx, g, 1, 0, s)) return rc;
  // + (G K*)' (G K*); edge form: (H E)' (H E), E (in Z, whose product above is enqueued first) the edge-layout K*
  GemmArgs y{};
  y.A = model->d_G; y.lda = N; y.B = Kt; y.ldb = ld; y.C = Y; y.ldc = ld;
  y.M = N; y.N = M; y.K = N; y.alpha = 1.0; y.beta = 0.0; y.khi_mode = 1; y.tri_block = mblk;
  if (model->form == PPBO_FORM_EDGE) {
    edge_apply_kernel<<<dim3((M + 127) / 128, N), 128, 0, s>>>(Kt, ld, M, mblk, n_q, model->d_lam_off, Z);
    PPBO_LAUNCH_CHECK(ctx);
    y.B = Z; y.tri_block = 1;    // H lower triangular
  }
  if (int rc = ppbo_gemm_launch(ctx, y, 0, 0, s)) return rc;
  GemmArgs c{};
  c.A = Y; c.lda = ld; c.B = Y; c.ldb = ld; c.C = d_cov; c.ldc = M;
  c.M = M; c.N = M; c.K = N; c.alpha = 1.0; c.beta = 1.0; c.tri_block = 1;
  return ppbo_gemm_launch(ctx, c, 1, 0, s);
}

}  // extern "C"

namespace {

// grid[b][g][:] = alpha_(b)[g] * xi[b][:] + x[b][:]: the G points of line b (what FeedbackProcessing.xi_grid returns with
// is_scaled = True, src/feedback_processing.py:57-107, for abscissae alpha that the host has drawn); per_line = 0: one
// shared abscissa vector alpha[G] (common random numbers across lines), 1: alpha[B][G]
__global__ __launch_bounds__(256) void line_grid_kernel(const double* __restrict__ xi, const double* __restrict__ x,
                                                        const double* __restrict__ alpha, int per_line, int B, int G,
                                                        int D, double* __restrict__ grid) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)B * G * D) return;
  const int d = (int)(e % D);
  const long long bg = e / D;
  const int g = (int)(bg % G), b = (int)(bg / G);
  const double a = alpha[per_line ? (size_t)b * G + g : g];
  grid[e] = a * xi[(size_t)b * D + d] + x[(size_t)b * D + d];
}

// row slices of the covariance's data term: enough (group, slice) workgroups for every CU to hold several
// a slice walks its rows in chunks of cov_cs: whole stars (as many as fit the 32 staged rows) where a star has at most
// 32 rows -- the symmetric form of line_cov_kernel --, else 32 rows of anything
struct LineCovPlan {
  bool sym;
  int cov_cs, cov_splits, cov_rows;
};
LineCovPlan line_cov_plan(int N, int mblk, int Bc_max) {
  LineCovPlan pl;
  pl.sym = mblk <= 32;
  pl.cov_cs = pl.sym ? (32 / mblk) * mblk : 32;
  int cov_splits = (1024 + Bc_max - 1) / Bc_max;
  if (cov_splits < (N + LC_MAXROWS - 1) / LC_MAXROWS) cov_splits = (N + LC_MAXROWS - 1) / LC_MAXROWS;   // <= LC_MAXROWS rows per slice
  if (cov_splits > (N + pl.cov_cs - 1) / pl.cov_cs) cov_splits = (N + pl.cov_cs - 1) / pl.cov_cs;
  if (cov_splits < 1) cov_splits = 1;
  int cov_rows = ((((N + cov_splits - 1) / cov_splits) + pl.cov_cs - 1) / pl.cov_cs) * pl.cov_cs;
  if (cov_rows > LC_MAXROWS) cov_rows = (LC_MAXROWS / pl.cov_cs) * pl.cov_cs;
  pl.cov_rows = cov_rows;
  pl.cov_splits = (N + cov_rows - 1) / cov_rows;
  return pl;
}

// The contraction stage shared by the line entries and ppbo_predict_gradients: for the Bc groups of G columns each that Kt
// [Nk][ld] holds in the node layout (M = Bc G columns), Y = G K* (edge form: E into Ke, then Y = H E) and the groups' data
// terms K*' Lambda K* + Y'Y in cov_parts, pl.cov_splits row-slice slabs of stride pst.
int line_y_cov(ppbo_ctx* ctx, const ppbo_model* model, const LineWorkspace& lw, int M, int Bc, int G, const LineCovPlan& pl,
               double* cov_parts, long long pst, hipStream_t s) {
  const int N = model->N, mblk = model->m + 1, n_q = N / mblk;
  const int ld = lw.ld;
  const double* const Kt = lw.Kt;
  const bool edge = model->form == PPBO_FORM_EDGE, sym = pl.sym;
  const int cov_splits = pl.cov_splits, cov_rows = pl.cov_rows, cov_cs = pl.cov_cs;
  GemmArgs y{};  // Y = G K*
  y.A = lw.Gq; y.lda = lw.Nk; y.B = Kt; y.ldb = ld; y.C = lw.Y; y.ldc = ld;
  y.M = lw.g_rows; y.N = (M + 127) & ~127; y.K = lw.Nk; y.alpha = 1.0; y.beta = 0.0; y.khi_mode = 1; y.tri_block = mblk;
  if (edge) {
    edge_apply_kernel<<<dim3((M + 127) / 128, N), 128, 0, s>>>(Kt, ld, M, mblk, n_q, model->d_lam_off, lw.Ke);
    PPBO_LAUNCH_CHECK(ctx);
    y.B = lw.Ke; y.tri_block = 1;   // H lower triangular
  }
  // (rows [N, g_rows) of Y come out as zeros, columns [M, y.N) as whatever the K* padding holds: neither is read)
  // column tiles in chunks through all row tiles, heaviest first (a chunk's slice of K* -- 134 MB at 64 tiles -- stays
  // in the Infinity Cache); equal chunks of at most 72 tiles: a ragged last chunk costs 5 % (512 lines: 280 tiles in
  // chunks of 70: 2.33 ms; 64 + ragged 24: 2.47; 56: 2.35; 96: 2.35; 128: 4.85; one chunk: 4.2)
  const int y_tiles = (M + 127) / 128, y_chunks = (y_tiles + 71) / 72;
  y.nt_chunk = ctx->line_y_chunk > 0 ? ctx->line_y_chunk : (y_tiles + y_chunks - 1) / y_chunks;
  {
    PpboProfScope pf(ctx, ppbo_ctx::PF_LINE_Y, s);
    if (int rc = ppbo_gemm_launch(ctx, y, 0, 0, s)) return rc;
  }
  // data term of every group's covariance: K*' Lambda K* + Y'Y, one workgroup per (group, row slice)
  {
    PpboProfScope pf(ctx, ppbo_ctx::PF_LINE_COV, s);
    const dim3 cg(Bc, cov_splits);
    // sym: every chunk is whole stars: the symmetric form (lower-triangle tiles only)
#define LC_LAUNCH(NT)                                                                                                   \
  do {                                                                                                                  \
    if (sym) line_cov_kernel<NT, true><<<cg, 256, 0, s>>>(Kt, lw.Y, ld, N, G, mblk, model->d_lam_diag, model->d_lam_off,   \
                                                          cov_rows, cov_parts, pst, cov_cs);                            \
    else line_cov_kernel<NT, false><<<cg, 256, 0, s>>>(Kt, lw.Y, ld, N, G, mblk, model->d_lam_diag, model->d_lam_off,      \
                                                       cov_rows, cov_parts, pst, cov_cs);                               \
  } while (0)
    switch ((G + 15) / 16) {
      case 1: LC_LAUNCH(1); break;
      case 2: LC_LAUNCH(2); break;
      case 3: LC_LAUNCH(3); break;
      case 4: LC_LAUNCH(4); break;
      case 5: LC_LAUNCH(5); break;
      case 6: LC_LAUNCH(6); break;
      case 7: LC_LAUNCH(7); break;
      default: LC_LAUNCH(8); break;
    }
#undef LC_LAUNCH
  }
  return 0;
}

// what ppbo_line_choice asks of the draws in place of EI / varmax: the chosen point of every draw, counted
struct LineChoice {
  const double* d_e;   // [S,G] or NULL
  double noise_sd;
  double* d_prob;      // [B,G]
  int* d_count;        // [B,G] or NULL
  int* d_choice;       // [B,S] or NULL
};
// what ppbo_score_answers asks of the groups instead: point 0 of each group is the answer, scored by answers.hip
struct LineAnswers {
  double sigma;
  double* d_lpd;       // [B] or NULL
  double* d_agree;     // [B] or NULL
  double* d_edge;      // [B,G] or NULL
};

// EI / varmax of B lines whose grid points are either given (d_grid) or formed on the device from (xi, x, alpha); with
// `ch` the choice probabilities of the same B groups instead (everything before the Monte-Carlo launch is shared)
int line_acq_impl(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, const double* d_xi, const double* d_x,
                  const double* d_alpha, int alpha_per_line, int B, int G, double shrink, const double* d_z, int S,
                  double mustar, double jitter, double* d_ei, double* d_varmax, hipStream_t s,
                  const LineChoice* ch = nullptr, const LineAnswers* an = nullptr) {
  if (int rc = check_model(ctx, model)) return rc;
  // (the answers' own entry has checked d_z and S: it also runs without draws)
  PPBO_REQUIRE(ctx, (d_grid || (d_xi && d_x && d_alpha)) && (an || (d_z && S > 0)) && B > 0 && G > 0 && G <= 128,
               "line arguments (G <= 128)");
  PPBO_REQUIRE(ctx, model->d_G && model->d_lam_diag && model->d_lam_off, "model G/Lambda");
  const int N = model->N, mblk = model->m + 1, D = model->D;
  const KernParams p = make_kern_params(model->kernel_id, model->theta);
  const Chunks ck(B, 512);
  const int Bc_max = ck.Mc_max;
  LineWorkspace lw;
  if (int rc = lw.prepare(ctx, model, Bc_max * G, true, (long long)B * G >= 2048, s)) return rc;
  double* gridws = nullptr;
  if (!d_grid) {
    gridws = (double*)ppbo_workspace(ctx, ppbo_ctx::WS_SEARCH, (size_t)Bc_max * G * D * sizeof(double));
    if (!gridws) return (int)hipErrorOutOfMemory;
  }
  const int q_per_split = lw.rs.q_per_split, n_split_eff = lw.rs.n_split_eff;
  const LineCovPlan lcp = line_cov_plan(N, mblk, Bc_max);
  const bool sym = lcp.sym;
  const int cov_splits = lcp.cov_splits;
  double* part = (double*)ppbo_workspace(
      ctx, ppbo_ctx::WS_PART,
      ((size_t)(n_split_eff + 1) * Bc_max * G + (size_t)(1 + cov_splits) * Bc_max * G * G) * sizeof(double));
  if (!part) return (int)hipErrorOutOfMemory;
  double* mu = part + (size_t)n_split_eff * Bc_max * G;
  double* cov = mu + (size_t)Bc_max * G;
  double* cov_parts = cov + (size_t)Bc_max * G * G;
  const int G16 = (G + 15) & ~15;
  const size_t mc_lds = ((size_t)G16 * (G16 + 2) + G16 + 16) * sizeof(double);   // G = 128: 134 KB of the CU's 160 KB
  // the choice kernel: the same factor and mean, then its histogram (G = 128: 512 B more)
  const size_t ch_lds = ((size_t)G16 * (G16 + 2) + G16) * sizeof(double) + (size_t)G16 * sizeof(int);
  if (!ch && !an && mc_lds > 64 * 1024) ppbo_lds_limit(ctx, (const void*)line_mc_kernel, (128 * 130 + 128 + 16) * (int)sizeof(double));
  if (ch && ch_lds > 64 * 1024)
    ppbo_lds_limit(ctx, (const void*)line_choice_kernel, (128 * 130 + 128) * (int)sizeof(double) + 128 * (int)sizeof(int));
  // draws of a line spread over several workgroups when the batch alone does not fill the chip (>= 64 draws each)
  int nsplit = (2 * 256 + Bc_max - 1) / Bc_max;
  if (nsplit > (S + 63) / 64) nsplit = (S + 63) / 64;
  if (nsplit < 1) nsplit = 1;
  // (the answers' scores split their draws themselves, and may come with S = 0: this plan is not theirs)
  const int draws_per_split = an ? 16 : (((S + nsplit - 1) / nsplit) + 15) & ~15;
  nsplit = (S + draws_per_split - 1) / draws_per_split;
  // per-(line, split) partial results: three sums, or a histogram of G counts (the answers' scores keep their own)
  void* mc_ws = an ? nullptr : ppbo_workspace(ctx, ppbo_ctx::WS_SMALL,
                               (size_t)Bc_max * nsplit * (ch ? (size_t)G * sizeof(int) : 3 * sizeof(double)));
  if (!mc_ws && !an) return (int)hipErrorOutOfMemory;
  double* mc_part = (double*)mc_ws;
  for (const Chunk c : ck) {
    const int b0 = (int)c.beg, Bc = c.Mc;
    const int M = Bc * G;
    const double* xg;
    if (d_grid) {
      xg = d_grid + (size_t)b0 * G * D;
    } else {
      const long long ne = (long long)Bc * G * D;
      line_grid_kernel<<<(unsigned)((ne + 255) / 256), 256, 0, s>>>(d_xi + (size_t)b0 * D, d_x + (size_t)b0 * D,
                                                                    alpha_per_line ? d_alpha + (size_t)b0 * G : d_alpha,
                                                                    alpha_per_line, Bc, G, D, gridws);
      xg = gridws;
    }
    {
      PpboProfScope pf(ctx, ppbo_ctx::PF_LINE_KSTAR, s);
      dispatch_kstar(model, xg, M, lw.Kt, lw.ld, part, nullptr, q_per_split, n_split_eff, false, s);
    }
    score_kernel<<<score_blocks(M), SC_THREADS, 0, s>>>(part, n_split_eff, nullptr, nullptr, 0, M, 0.0, PPBO_SCORE_MEAN,
                                                        0.0, 0, mu, nullptr, nullptr, nullptr);
    if (int rc = ppbo_kernel_dispatch(ctx, model->kernel_id, [&](auto kid) {
          line_prior_kernel<decltype(kid)::value><<<Bc, 256, 0, s>>>(xg, G, D, p, shrink, cov);
          return 0;
        }))
      return rc;
    PPBO_LAUNCH_CHECK(ctx);
    if (int rc = line_y_cov(ctx, model, lw, M, Bc, G, lcp, cov_parts, (long long)Bc_max * G * G, s)) return rc;
    if (an) {
      if (int rc = ppbo_answer_score_groups(ctx, mu, cov, Bc, G, an->sigma, d_z, S, jitter, cov_parts, cov_splits,
                                            (long long)Bc_max * G * G, sym ? 1 : 0, an->d_lpd ? an->d_lpd + b0 : nullptr,
                                            an->d_agree ? an->d_agree + b0 : nullptr,
                                            an->d_edge ? an->d_edge + (size_t)b0 * G : nullptr, s))
        return rc;
      continue;
    }
    if (ch) {
      {
        PpboProfScope pf(ctx, ppbo_ctx::PF_LINE_MC, s);
        line_choice_kernel<<<dim3(Bc, nsplit), 256, ch_lds, s>>>(
            mu, cov, G, d_z, ch->d_e, S, ch->noise_sd, jitter, draws_per_split, (int*)mc_ws,
            ch->d_choice ? ch->d_choice + (size_t)b0 * S : nullptr, cov_parts, cov_splits, (long long)Bc_max * G * G,
            sym ? 1 : 0);
      }
      choice_finish_kernel<<<(M + 255) / 256, 256, 0, s>>>((const int*)mc_ws, M, G, nsplit, S,
                                                           ch->d_prob + (size_t)b0 * G,
                                                           ch->d_count ? ch->d_count + (size_t)b0 * G : nullptr);
      PPBO_LAUNCH_CHECK(ctx);
      continue;
    }
    {
      PpboProfScope pf(ctx, ppbo_ctx::PF_LINE_MC, s);
      line_mc_kernel<<<dim3(Bc, nsplit), 256, mc_lds, s>>>(mu, cov, G, d_z, S, mustar, jitter, draws_per_split, mc_part,
                                                           cov_parts, cov_splits, (long long)Bc_max * G * G, sym ? 1 : 0);
    }
    mc_finish_kernel<<<(Bc + 255) / 256, 256, 0, s>>>(mc_part, Bc, nsplit, S, d_ei ? d_ei + b0 : nullptr,
                                                      d_varmax ? d_varmax + b0 : nullptr);
    PPBO_LAUNCH_CHECK(ctx);
  }
  return 0;
}

// the refusals of the choice entries that line_acq_impl does not make itself
int choice_args(ppbo_ctx* ctx, const double* d_e, double noise_sd, double jitter, const double* d_prob) {
  PPBO_REQUIRE(ctx, d_prob != nullptr, "d_prob");
  PPBO_REQUIRE(ctx, noise_sd >= 0.0 && noise_sd <= 1.79769313486231570815e308, "noise_sd (finite, >= 0)");
  PPBO_REQUIRE(ctx, jitter >= 0.0 && jitter <= 1.79769313486231570815e308, "jitter (finite, >= 0)");
  PPBO_REQUIRE(ctx, noise_sd == 0.0 || d_e != nullptr, "noise_sd > 0 needs the draws d_e");
  return 0;
}

// ---- ppbo_predict_gradients: the posterior N(m, C) of grad f at P points per chunk --------------------------------------
struct GradMetric {
  double w[64];      // (check_model: D <= 64)
};

// Pass 3 of ppbo_predict_gradients, one workgroup per point b:
//   m_d  = the mean partials of column b D + d, summed in split order
//   C_de = P_de + the data term of line_cov_kernel's slabs (K*' Lambda K* + Y'Y of the point's D columns), added in slab
//          order and symmetrised as mc_factor_lds does it -- v = (a + b) / 2 with a, b the sums at (d, e) and (e, d), so
//          C_de and C_ed are the same bits;  P = the unshrunk prior diag(slope_prior_weight)
//   score = sum_d w_d C_dd (PPBO_GRAD_TRACE) or sum_d w_d (m_d^2 + C_dd) (PPBO_GRAD_NORM2), summed in the order of d
// A point with a non-finite coordinate (read again from d_X here) gets NaN everywhere and an empty record.
template <int KID>
__global__ __launch_bounds__(256) void grad_finish_kernel(const double* __restrict__ Xp, int P, int D, KernParams p,
                                                          const double* __restrict__ mu_part, int n_mu,
                                                          const double* __restrict__ cov_parts, int n_parts,
                                                          long long part_stride, int parts_lower_only, GradMetric w,
                                                          int kind, long long idx_base, double* __restrict__ mean_out,
                                                          double* __restrict__ cov_out, double* __restrict__ score_out,
                                                          Best* __restrict__ blk_best) {
  __shared__ double s_m[64], s_c[64];
  const int b = blockIdx.x, t = threadIdx.x;
  double chk = 0.0;
  for (int i = 0; i < D; ++i) chk = fma(Xp[(size_t)b * D + i], 0.0, chk);
  const bool bad = chk != 0.0;
  if (t < D) {
    double m = 0.0;
    for (int s = 0; s < n_mu; ++s) m += mu_part[(size_t)s * P * D + (size_t)b * D + t];
    if (bad) m = NAN;
    s_m[t] = m;
    if (mean_out) mean_out[(size_t)b * D + t] = m;
  }
  if (cov_parts) {
    const double* cp = cov_parts + (size_t)b * D * D;
    for (int e = t; e < D * D; e += 256) {
      const int g = e / D, h = e - g * D;
      double a = (g == h) ? slope_prior_weight<KID>(g, p) : 0.0, c = a;
      // parts_lower_only: the slabs are exactly symmetric and hold the 16 x 16 tiles of the lower triangle only
      const bool up = parts_lower_only && (g >> 4) < (h >> 4);
      const int ia = up ? h * D + g : g * D + h, ib = (parts_lower_only && !up && (g >> 4) > (h >> 4)) ? g * D + h : h * D + g;
      for (int k = 0; k < n_parts; ++k) { a += cp[(size_t)k * part_stride + ia]; c += cp[(size_t)k * part_stride + ib]; }
      double v = 0.5 * (a + c);
      if (bad) v = NAN;
      if (cov_out) cov_out[(size_t)b * D * D + e] = v;
      if (g == h) s_c[g] = v;
    }
  }
  if (kind == PPBO_GRAD_NONE) return;
  __syncthreads();
  if (t != 0) return;
  double sc = 0.0;
  for (int d = 0; d < D; ++d) sc += w.w[d] * (kind == PPBO_GRAD_NORM2 ? s_m[d] * s_m[d] + s_c[d] : s_c[d]);
  if (bad) sc = NAN;
  if (score_out) score_out[b] = sc;
  if (blk_best) {
    Best r{0.0, -1};
    if (sc == sc) { r.val = sc; r.idx = idx_base + b; }
    blk_best[b] = r;
  }
}

}  // namespace

extern "C" {

int ppbo_line_acq(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, int B, int G, double shrink,
                  const double* d_z, int S, double mustar, double jitter, double* d_ei, double* d_varmax,
                  void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_grid != nullptr, "d_grid");
  return line_acq_impl(ctx, model, d_grid, nullptr, nullptr, nullptr, 0, B, G, shrink, d_z, S, mustar, jitter, d_ei,
                       d_varmax, (hipStream_t)stream);
}

int ppbo_line_acq_xi(ppbo_ctx* ctx, const ppbo_model* model, const double* d_xi, const double* d_x,
                     const double* d_alpha, int alpha_per_line, int B, int G, double shrink, const double* d_z, int S,
                     double mustar, double jitter, double* d_ei, double* d_varmax, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_xi && d_x && d_alpha, "xi / x / alpha");
  return line_acq_impl(ctx, model, nullptr, d_xi, d_x, d_alpha, alpha_per_line != 0, B, G, shrink, d_z, S, mustar,
                       jitter, d_ei, d_varmax, (hipStream_t)stream);
}

int ppbo_line_choice(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, int B, int G, double shrink,
                     const double* d_z, const double* d_e, int S, double noise_sd, double jitter, double* d_prob,
                     int* d_count, int* d_choice, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_grid != nullptr, "d_grid");
  if (int rc = choice_args(ctx, d_e, noise_sd, jitter, d_prob)) return rc;
  const LineChoice ch{noise_sd > 0.0 ? d_e : nullptr, noise_sd, d_prob, d_count, d_choice};
  return line_acq_impl(ctx, model, d_grid, nullptr, nullptr, nullptr, 0, B, G, shrink, d_z, S, 0.0, jitter, nullptr,
                       nullptr, (hipStream_t)stream, &ch);
}

int ppbo_line_choice_xi(ppbo_ctx* ctx, const ppbo_model* model, const double* d_xi, const double* d_x,
                        const double* d_alpha, int alpha_per_line, int B, int G, double shrink, const double* d_z,
                        const double* d_e, int S, double noise_sd, double jitter, double* d_prob, int* d_count,
                        int* d_choice, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_xi && d_x && d_alpha, "xi / x / alpha");
  if (int rc = choice_args(ctx, d_e, noise_sd, jitter, d_prob)) return rc;
  const LineChoice ch{noise_sd > 0.0 ? d_e : nullptr, noise_sd, d_prob, d_count, d_choice};
  return line_acq_impl(ctx, model, nullptr, d_xi, d_x, d_alpha, alpha_per_line != 0, B, G, shrink, d_z, S, 0.0, jitter,
                       nullptr, nullptr, (hipStream_t)stream, &ch);
}

int ppbo_score_answers(ppbo_ctx* ctx, const ppbo_model* model, const double* d_grid, int B, int G, double shrink,
                       const double* d_z, int S, double jitter, double* d_lpd, double* d_agree, double* d_edge,
                       void* stream) {
  PPBO_ENTER(ctx);
  const double dmax = 1.79769313486231570815e308;
  PPBO_REQUIRE(ctx, model != nullptr && d_grid != nullptr, "model / d_grid");
  PPBO_REQUIRE(ctx, B >= 1 && G >= 2 && G <= 128, "groups (B >= 1, 2 <= G <= 128: the answer and at least one other point)");
  PPBO_REQUIRE(ctx, S >= 0, "S >= 0");
  PPBO_REQUIRE(ctx, S == 0 || d_z != nullptr, "S > 0 needs the draws d_z");
  PPBO_REQUIRE(ctx, S > 0 || d_lpd == nullptr, "d_lpd needs S > 0 draws");
  PPBO_REQUIRE(ctx, jitter >= 0.0 && jitter <= dmax, "jitter (finite, >= 0)");
  PPBO_REQUIRE(ctx, model->theta[0] > 0.0 && model->theta[0] <= dmax, "sigma = theta[0] (finite, > 0)");
  PPBO_REQUIRE(ctx, d_lpd || d_agree || d_edge, "every output is NULL");
  const LineAnswers an{model->theta[0], d_lpd, d_agree, d_edge};
  return line_acq_impl(ctx, model, d_grid, nullptr, nullptr, nullptr, 0, B, G, shrink, d_z, S, 0.0, jitter, nullptr,
                       nullptr, (hipStream_t)stream, nullptr, &an);
}

// Gradients: per chunk of at most GRAD_CHUNK = 512 points kstar_grad ->
// line_y_cov with the D columns of a point as one group -> grad_finish -> one-workgroup argmax.  A chunk is at most
// 512 x 64 = 32768 columns, half of what the line entries put through the same workspaces (512 lines of 128 points), so
// the cap is 512 for every D.  The column pass is timed as "grad_kstar", the contraction under the line entries' "line_y"
// and "line_cov", the finishing pass as "grad_finish".
int ppbo_predict_gradients(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, int64_t M, const double* h_metric,
                           int score_kind, double* d_mean, double* d_cov, double* d_score, double* h_best_val,
                           int64_t* h_best_idx, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_model(ctx, model)) return rc;
  PPBO_REQUIRE(ctx, d_X != nullptr, "gradients (d_X)");
  PPBO_REQUIRE(ctx, M >= 1 && M <= (int64_t)0x7fffffff, "point count (1 .. 2^31 - 1)");
  PPBO_REQUIRE(ctx, score_kind == PPBO_GRAD_NONE || score_kind == PPBO_GRAD_TRACE || score_kind == PPBO_GRAD_NORM2, "score_kind");
  PPBO_REQUIRE(ctx, !model->kstar_fp32, "gradients are fp64 only (kstar_fp32)");
  const int N = model->N, D = model->D, mblk = model->m + 1;
  GradMetric gm;
  for (int d = 0; d < 64; ++d) gm.w[d] = 1.0;
  if (h_metric)
    for (int d = 0; d < D; ++d) {
      PPBO_REQUIRE(ctx, h_metric[d] > 0.0 && h_metric[d] <= 1.79769313486231570815e308, "metric (positive, finite)");
      gm.w[d] = h_metric[d];
    }
  const bool want_cov = d_cov || score_kind != PPBO_GRAD_NONE;
  PPBO_REQUIRE(ctx, !want_cov || model->d_G != nullptr, "covariance / score need model->d_G");
  PPBO_REQUIRE(ctx, !want_cov || (model->d_lam_diag && model->d_lam_off), "model Lambda");
  const bool want_best = (h_best_val || h_best_idx) && score_kind != PPBO_GRAD_NONE;
  if (score_kind == PPBO_GRAD_NONE) {      // nothing is scored
    if (h_best_val) *h_best_val = NAN;
    if (h_best_idx) *h_best_idx = -1;
  }
  BestReturn br;
  if (int rc = br.begin(ctx, want_best)) return rc;
  constexpr int GRAD_CHUNK = 512;
  const KernParams p = make_kern_params(model->kernel_id, model->theta);
  const Chunks ck(M, GRAD_CHUNK);
  const int Pc_max = ck.Mc_max;
  LineWorkspace lw;
  if (int rc = lw.prepare(ctx, model, Pc_max * D, want_cov, (long long)Pc_max * D >= 2048, s)) return rc;
  const LineCovPlan lcp = want_cov ? line_cov_plan(N, mblk, Pc_max) : LineCovPlan{};
  const int q_per_split = lw.rs.q_per_split, n_split_eff = lw.rs.n_split_eff;
  const long long pst = (long long)Pc_max * D * D;
  double* part = (double*)ppbo_workspace(
      ctx, ppbo_ctx::WS_PART,
      ((size_t)n_split_eff * Pc_max * D + (want_cov ? (size_t)lcp.cov_splits * pst : 0)) * sizeof(double));
  if (!part) return (int)hipErrorOutOfMemory;
  double* cov_parts = want_cov ? part + (size_t)n_split_eff * Pc_max * D : nullptr;
  Best* bests = (Best*)ppbo_workspace(ctx, ppbo_ctx::WS_SMALL, (size_t)(Pc_max + ck.n) * sizeof(Best));
  if (!bests) return (int)hipErrorOutOfMemory;
  Best* chunk_best = bests + Pc_max;
  for (const Chunk c : ck) {
    const int Pc = c.Mc;
    const double* xp = d_X + (size_t)c.beg * D;
    if (int rc = ppbo_kernel_dispatch(ctx, model->kernel_id, [&](auto kid) {
          constexpr int KID = decltype(kid)::value;
          {
            PpboProfScope pf(ctx, ppbo_ctx::PF_GRAD_KSTAR, s);
            launch_kstar_grad<KID>(KstarLaunch{model, p, lw.Kt, lw.ld, part, nullptr, q_per_split, n_split_eff, false, -1, s}, xp, Pc);
          }
          PPBO_LAUNCH_CHECK(ctx);
          if (want_cov)
            if (int rc2 = line_y_cov(ctx, model, lw, Pc * D, Pc, D, lcp, cov_parts, pst, s)) return rc2;
          PpboProfScope pf(ctx, ppbo_ctx::PF_GRAD_FINISH, s);
          grad_finish_kernel<KID><<<Pc, 256, 0, s>>>(xp, Pc, D, p, part, n_split_eff, cov_parts, lcp.cov_splits, pst,
                                                     lcp.sym ? 1 : 0, gm, score_kind, (long long)c.beg,
                                                     d_mean ? d_mean + (size_t)c.beg * D : nullptr,
                                                     d_cov ? d_cov + (size_t)c.beg * D * D : nullptr,
                                                     d_score ? d_score + c.beg : nullptr, want_best ? bests : nullptr);
          PPBO_LAUNCH_CHECK(ctx);
          return 0;
        }))
      return rc;
    if (int rc = br.chunk(ctx, bests, Pc, chunk_best, c.ch, ck, s)) return rc;
  }
  return br.finish(ctx, chunk_best, ck, s, h_best_val, h_best_idx);
}

int ppbo_randn(ppbo_ctx* ctx, uint64_t seed, double* d_out, int64_t n, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_out && n > 0, "output");
  const long long pairs = (n + 1) / 2;
  PPBO_REQUIRE(ctx, (pairs + 255) / 256 < ((long long)1 << 31), "n too large for one launch");
  randn_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, (hipStream_t)stream>>>((unsigned long long)seed, d_out, (long long)n);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

int ppbo_rff_omega_draws(ppbo_ctx* ctx, uint64_t seed, const double* d_omega_map, const double* d_cov_diag, int F, int S,
                         double* d_omegas, void* stream) {
  PPBO_ENTER(ctx);
  PPBO_REQUIRE(ctx, d_omega_map && d_cov_diag && d_omegas, "null pointer");
  PPBO_REQUIRE(ctx, F > 0 && S > 0, "F / S");
  const long long n = (long long)S * F, pairs = (n + 1) / 2;
  PPBO_REQUIRE(ctx, (n + 255) / 256 < ((long long)1 << 31), "S x F too large for one launch");
  hipStream_t s = (hipStream_t)stream;
  randn_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, s>>>((unsigned long long)seed, d_omegas, n);
  omega_draws_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_omega_map, d_cov_diag, F, n, d_omegas);
  PPBO_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
