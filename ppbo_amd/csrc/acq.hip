// Acquisition gradients and their device ascent (ppbo_acq_grad, ppbo_acq_ascent; no reference counterpart).
// With k = k(x, X), J = dk/dx [N][D] (analytic, on direct differences: mean_grad_kernel's expressions), alpha and the
// variance operator M of the model (G in node form, H diag(w) D in edge form):
//   mu = k' alpha                                   grad mu  = J' alpha
//   var = sf2 + k' Lambda k + |M k|^2               grad var = 2 J' u,   u = (Lambda + M'M) k
// u is a column of the tournament's field pass (tournament_field, predict.hip), which runs per chunk of at most 1024
// points with its GEMM tile configuration pinned and a K* row split that depends on the model alone: a point's column
// then has the same bits whatever stands next to it.
//   node form   u_j = U[j]
//   edge form   U = H'(H E) + Delta lives in the edge layout against e_r = lam_off[j] (k_j - k_obs), whose Jacobian is
//               lam_off[j] (J_j - J_obs): grad var = 2 sum_r de_r/dx U_r = 2 J' u~ with u~_j = lam_off[j] U[r(j)] on a
//               pseudo row and u~_obs = -sum_{j in star} lam_off[j] U[r(j)] on an observation row
// The value var is formed as ppbo_predict forms it, never from k'u (which cancels): the Lambda term by kstar_kernel's
// star sums over the field pass's K* column, |M k|^2 as the column's sum of squares of Y = M K*.  mu is the sum over
// directly evaluated kernel values, as ppbo_mean_grad forms it.
// score_value's expression (score.h) gives the score; its gradient is ONE contraction of J with a alpha_j + b u_j:
//   MEAN (1, 0)     VARIANCE (0, 2)     EI, sd > 0: (Phi(z), phi(z) / sd)     EI, sd = 0: (mu > mu* ? 1 : 0, 0)
// acq_grad_kernel: one 256-thread workgroup per point (mean_grad_kernel's geometry), a value pass, then one pass over
// the design rows per requested gradient -- point, accumulator and differences are three D-vectors of doubles per lane,
// 384 of the 512 registers at DP = 64, so a second accumulator beside them would spill there.  Every sum meets by
// shuffles and in LDS in a fixed order: no atomics, a repeated call is bitwise equal.
#include "common.h"
#include "linalg.h"
#include "score.h"

namespace {

constexpr int AQ_T = 256;          // threads per point
constexpr int AQ_CHUNK = 1024;     // points per field pass (PPBO_TOURNAMENT_MAX_B)
constexpr int AQ_GEMM_CFG = 3;     // the field pass's GEMMs on 32 x 32 tiles, whatever the number of columns

// what the field pass left for a chunk's points; KB == NULL: no operator is read (the mean and its gradient alone)
struct AcqField {
  const double *KB, *Y, *U;        // K* [N][ldu] (node layout), Y = M K* [N][ldu], U [NkU][ldu] (the form's layout)
  int ldu;
  const double *lam_diag, *lam_off;
  int mblk, n_q, edge;
};
struct AcqOut {
  double *mu, *var, *score;        // [M], each may be NULL
  double *gmu, *gvar, *gscore;     // [M][D], each may be NULL
};

// u~_i of the header comment for design row i and column c
__device__ __forceinline__ double acq_u(const AcqField& f, int c, int i) {
  if (!f.edge) return f.U[(size_t)i * f.ldu + c];
  const int m = f.mblk - 1, q = i / f.mblk, r = i - q * f.mblk;
  const size_t row0 = (size_t)f.n_q + (size_t)q * m;
  if (r) return f.lam_off[i] * f.U[(row0 + r - 1) * f.ldu + c];
  double t = 0.0;
  for (int e = 0; e < m; ++e) t += f.lam_off[i + 1 + e] * f.U[(row0 + e) * f.ldu + c];
  return -t;
}

// the four wavefront records of column d, in wavefront order
template <int DP>
__device__ __forceinline__ double acq_red(const double (*red)[DP + 1], int d) {
  return (red[0][d] + red[1][d]) + (red[2][d] + red[3][d]);
}

// out[d] = sum_i (wa alpha_i + wb u~_i) dk_i/dx_d for the point xc (mean_grad_kernel's row loop with that weight in the
// place of alpha_i)
template <int KID, int DP>
__device__ __forceinline__ void acq_grad_pass(const double (&xc)[DP], const double* __restrict__ X, int N, int D,
                                              const KernParams& p, const double* __restrict__ alpha, const AcqField& f,
                                              int c, double wa, double wb, double (*red)[DP + 1],
                                              double* __restrict__ out) {
  double g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) g[d] = 0.0;
  for (int i = threadIdx.x; i < N; i += AQ_T) {
    const double* __restrict__ xi = X + (size_t)i * D;
    double dx[DP], s = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      dx[d] = (d < D) ? xc[d] - xi[d] : 0.0;
      s += kern_term<KID>(dx[d], d, p);
    }
    double wgt = wa * alpha[i];
    if (wb != 0.0) wgt += wb * acq_u(f, c, i);
    double w, coef;
    if constexpr (kid_matern<KID>) {
      const MaternAE ae = matern_ae<KID>(s, p);
      coef = wgt * matern_grad<KID>(ae, p);
    } else {
      w = wgt * kern_finish<KID>(s, p);
    }
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
#pragma unroll
  for (int d = 0; d < DP; ++d) g[d] = wave_sum(g[d]);
  __syncthreads();                       // the records of the pass before this one have been read
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < DP; ++d) red[wave][d] = g[d];
  }
  __syncthreads();
  if ((int)threadIdx.x < D) out[threadIdx.x] = acq_red<DP>(red, threadIdx.x);
}

template <int KID, int DP>
__global__ __launch_bounds__(AQ_T) void acq_grad_kernel(const double* __restrict__ X, int N, int D, KernParams p,
                                                        const double* __restrict__ alpha,
                                                        const double* __restrict__ Xc, AcqField f, int kind,
                                                        double mustar, AcqOut o) {
  __shared__ double red[4][DP + 1];
  const int c = blockIdx.x;
  double xc[DP], chk = 0.0;
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    xc[d] = (d < D) ? Xc[(size_t)c * D + d] : 0.0;
    chk = fma(xc[d], 0.0, chk);          // NaN once a coordinate is not finite
  }
  if (!(chk == 0.0)) {                   // (the whole workgroup: a row with a non-finite coordinate gets NaN everywhere)
    if (threadIdx.x == 0) {
      if (o.mu) o.mu[c] = NAN;
      if (o.var) o.var[c] = NAN;
      if (o.score) o.score[c] = NAN;
    }
    if ((int)threadIdx.x < D) {
      if (o.gmu) o.gmu[(size_t)c * D + threadIdx.x] = NAN;
      if (o.gvar) o.gvar[(size_t)c * D + threadIdx.x] = NAN;
      if (o.gscore) o.gscore[(size_t)c * D + threadIdx.x] = NAN;
    }
    return;
  }
  // ---- the values: mu from direct differences, the Lambda term and |M k|^2 from the field pass's columns
  double m = 0.0, t = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < N; i += AQ_T) {
    const double* __restrict__ xi = X + (size_t)i * D;
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) s += kern_term<KID>((d < D) ? xc[d] - xi[d] : 0.0, d, p);
    m += alpha[i] * kern_finish<KID>(s, p);
    if (f.KB) {
      const double kv = f.KB[(size_t)i * f.ldu + c];
      const int obs = (i / f.mblk) * f.mblk;
      if (i == obs) t += f.lam_diag[i] * kv * kv;
      else t += kv * (f.lam_diag[i] * kv + 2.0 * f.lam_off[i] * f.KB[(size_t)obs * f.ldu + c]);
      const double y = f.Y[(size_t)i * f.ldu + c];
      q += y * y;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  m = wave_sum(m); t = wave_sum(t); q = wave_sum(q);
  if (lane == 0) { red[wave][0] = m; red[wave][1] = t; red[wave][2] = q; }
  __syncthreads();
  const double mu = acq_red<DP>(red, 0);
  const double var = f.KB ? p.sf2 + acq_red<DP>(red, 1) + acq_red<DP>(red, 2) : p.sf2;
  if (threadIdx.x == 0) {
    if (o.mu) o.mu[c] = mu;
    if (o.var) o.var[c] = var;
    if (o.score) o.score[c] = score_value(mu, var, kind, mustar);
  }
  // ---- the gradients, one pass each
  if (o.gmu) acq_grad_pass<KID, DP>(xc, X, N, D, p, alpha, f, c, 1.0, 0.0, red, o.gmu + (size_t)c * D);
  if (o.gvar) acq_grad_pass<KID, DP>(xc, X, N, D, p, alpha, f, c, 0.0, 2.0, red, o.gvar + (size_t)c * D);
  if (o.gscore) {
    double wa = 1.0, wb = 0.0;
    if (kind == PPBO_SCORE_VARIANCE) { wa = 0.0; wb = 2.0; }
    else if (kind == PPBO_SCORE_POINTWISE_EI) {
      const double dm = mu - mustar, sd = sqrt(fmax(var, 0.0));
      if (sd > 0.0) {
        const double z = dm / sd;
        wa = norm_cdf(z);
        wb = 0.39894228040143267794 * exp(-0.5 * z * z) / sd;
      } else wa = dm > 0.0 ? 1.0 : 0.0;
    }
    acq_grad_pass<KID, DP>(xc, X, N, D, p, alpha, f, c, wa, wb, red, o.gscore + (size_t)c * D);
  }
}

// The judgement of one round of ppbo_acq_ascent: bb_ascent_box_kernel's bookkeeping, one wavefront per start with
// lane = coordinate, between two evaluation rounds.  round < 0: the trial points are the starts clipped into the box (a
// NaN coordinate stays NaN).  round 0 takes the values at the clipped start and the first step; a later round judges
// the trial point (accept iff s_new >= s, so a NaN fails), updates x, g and the step; every round but the last then
// applies the stopping rule and writes the next trial point.  A stopped start repeats its point.
// box: lo[D] | hi[D] | hi - lo [D] | max_d (hi_d - lo_d).  x, sc, mu, var, it are the entry's outputs.
struct AcqState {
  double *trial, *gt, *st, *mut, *vart;   // the round's points [K][D] and what acq_grad_kernel returned for them
  double *x, *g, *sc, *mu, *var, *step;   // the accepted state
  int *stopped, *it;
};
__global__ __launch_bounds__(64) void acq_step_kernel(int D, int round, int iters, double tol,
                                                      const double* __restrict__ box,
                                                      const double* __restrict__ starts, AcqState a) {
  const int k = blockIdx.x, d = threadIdx.x;
  const bool live = d < D;
  const size_t e = (size_t)k * D + d;
  const double lo = live ? box[d] : 0.0, hi = live ? box[D + d] : 0.0, wmax = box[3 * D];
  if (round < 0) {
    if (live) {
      const double v = starts[e];
      a.trial[e] = (v != v) ? v : fmin(fmax(v, lo), hi);
    }
    if (d == 0) { a.stopped[k] = 0; a.it[k] = 0; }
    return;
  }
  int stop = a.stopped[k];
  const double xn = live ? a.trial[e] : 0.0, gn = live ? a.gt[e] : 0.0, sn = a.st[k];
  double x, g, s, step;
  bool take = false;
  if (round == 0) {
    x = xn; g = gn; s = sn;
    const double gnorm = sqrt(wave_sum_dpp(g * g));
    step = (0.02 * wmax) / fmax(gnorm, 1e-300);        // first move: 0.02 of the longest side
    take = true;
  } else {
    x = live ? a.x[e] : 0.0; g = live ? a.g[e] : 0.0; s = a.sc[k]; step = a.step[k];
    if (!stop) {
      const bool ok = sn >= s;
      const double sv = live ? xn - x : 0.0, yv = gn - g;
      const double curv = -wave_sum_dpp(sv * yv);      // > 0 where the score is locally concave along the move
      const double ss = wave_sum_dpp(sv * sv);
      step = ok ? (curv > 0.0 ? ss / fmax(curv, 1e-300) : 2.0 * step) : 0.25 * step;
      if (ok) { x = xn; g = gn; s = sn; take = true; }
      if (d == 0) a.it[k] += 1;
    }
  }
  if (take) {
    if (live) { a.x[e] = x; a.g[e] = g; }
    if (d == 0) { a.sc[k] = s; a.mu[k] = a.mut[k]; a.var[k] = a.vart[k]; }
  }
  if (round < iters && !stop) {
    const double pg = ((x <= lo && g < 0.0) || (x >= hi && g > 0.0)) ? 0.0 : g;
    const double pn = sqrt(wave_sum_dpp(pg * pg));
    if (!(pn * step >= tol) || !(wmax > 0.0)) stop = 1;
    else if (live) a.trial[e] = fmin(fmax(x + step * pg, lo), hi);
  }
  if (stop && live) a.trial[e] = x;
  if (d == 0) { a.step[k] = step; a.stopped[k] = stop; }
}

// the D ladder of acq_grad_kernel (mean_grad_kernel's rungs)
template <int KID>
int launch_acq_grad(const ppbo_model* m, const KernParams& p, const double* pts, int Mc, const AcqField& f, int kind,
                    double mustar, const AcqOut& o, hipStream_t s) {
#define AQ_LAUNCH(DP) \
  acq_grad_kernel<KID, DP><<<Mc, AQ_T, 0, s>>>(m->d_X, m->N, m->D, p, m->d_alpha, pts, f, kind, mustar, o)
  if (KID == PPBO_KERNEL_CAMPHOR || m->D <= 8) AQ_LAUNCH(8);
  else if constexpr (KID != PPBO_KERNEL_CAMPHOR) {     // (camphor-copper: D = 6)
    if (m->D <= 24) AQ_LAUNCH(24);
    else AQ_LAUNCH(64);
  }
#undef AQ_LAUNCH
  return 0;
}

// The workspaces of one evaluation round of up to Mc_max points, and the round itself.
struct AcqRound {
  const ppbo_model* m = nullptr;
  bool field = false;              // the operator is read: the field pass runs in front of acq_grad_kernel
  FieldPass fp;
  double* state = nullptr;         // state_doubles doubles of the caller's behind the field's arrays (the ascent's state)

  // every workspace before the first launch (growing one waits for the device); without a field pass there is none
  int prepare(ppbo_ctx* ctx, const ppbo_model* model, int Mc_max, bool with_field, size_t state_doubles = 0) {
    m = model;
    field = with_field;
    if (!field) return 0;
    const int n_q = m->N / (m->m + 1);
    // the row split of the field's K* launch from the model alone (pick_split's answer for one column): it decides
    // nothing a column of K* depends on, and so it must not depend on the number of points either
    const int want = n_q < 64 ? n_q : 64, q_per_split = (n_q + want - 1) / want;
    state = fp.prepare(ctx, m, Mc_max, RowSplit{want, q_per_split, (n_q + q_per_split - 1) / q_per_split}, state_doubles);
    return state ? 0 : (int)hipErrorOutOfMemory;
  }
  int run(ppbo_ctx* ctx, const double* pts, int Mc, int kind, double mustar, const AcqOut& o, hipStream_t s) const {
    AcqField f{};
    if (field) {
      PpboProfScope pf(ctx, ppbo_ctx::PF_ACQ_FIELD, s);
      if (int rc = fp.run(ctx, pts, Mc, s, AQ_GEMM_CFG)) return rc;
      f.KB = fp.KB; f.Y = fp.Y; f.U = fp.U; f.ldu = fp.ldu;
      f.lam_diag = m->d_lam_diag; f.lam_off = m->d_lam_off;
      f.mblk = m->m + 1; f.n_q = m->N / (m->m + 1); f.edge = m->form == PPBO_FORM_EDGE;
    }
    const KernParams p = make_kern_params(m->kernel_id, m->theta);
    PpboProfScope pf(ctx, ppbo_ctx::PF_ACQ_GRAD, s);
    if (int rc = ppbo_kernel_dispatch(ctx, m->kernel_id, [&](auto kid) {
          return launch_acq_grad<decltype(kid)::value>(m, p, pts, Mc, f, kind, mustar, o, s);
        }))
      return rc;
    PPBO_LAUNCH_CHECK(ctx);
    return 0;
  }
};

// the refusals the two entries share
int acq_check(ppbo_ctx* ctx, const ppbo_model* m, int score_kind, bool with_field) {
  PPBO_REQUIRE(ctx, m != nullptr, "model");
  PPBO_REQUIRE(ctx, m->d_X && m->d_alpha, "model X/alpha");
  PPBO_REQUIRE(ctx, m->N > 0 && m->D > 0 && m->D <= 64 && m->m >= 1, "model sizes (D<=64)");
  PPBO_REQUIRE(ctx, m->N % (m->m + 1) == 0, "N must be n_q*(m+1)");
  PPBO_REQUIRE_KERNEL(ctx, m->kernel_id, m->D);
  PPBO_REQUIRE(ctx, score_kind == PPBO_SCORE_MEAN || score_kind == PPBO_SCORE_POINTWISE_EI || score_kind == PPBO_SCORE_VARIANCE,
               "score_kind");
  PPBO_REQUIRE(ctx, !m->kstar_fp32, "acquisition gradients are fp64 only (kstar_fp32)");
  PPBO_REQUIRE(ctx, m->coords.kind != PPBO_COORDS_CAMPHOR, "a box in x is not a box in e(x): no PPBO_COORDS_CAMPHOR model");
  if (with_field) {
    PPBO_REQUIRE(ctx, m->d_G != nullptr, "anything but the mean needs model->d_G");
    PPBO_REQUIRE(ctx, m->d_lam_diag && m->d_lam_off, "anything but the mean needs the model's Lambda");
    PPBO_REQUIRE_FORM(ctx, m->form);
  }
  return 0;
}

}  // namespace

extern "C" {

int ppbo_acq_grad(ppbo_ctx* ctx, const ppbo_model* model, const double* d_X, int64_t M, int score_kind, double mustar,
                  double* d_mu, double* d_var, double* d_score, double* d_grad_mu, double* d_grad_var,
                  double* d_grad_score, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  const bool with_field = score_kind != PPBO_SCORE_MEAN || d_var || d_grad_var;
  if (int rc = acq_check(ctx, model, score_kind, with_field)) return rc;
  PPBO_REQUIRE(ctx, d_X != nullptr, "points");
  PPBO_REQUIRE(ctx, d_mu || d_var || d_score || d_grad_mu || d_grad_var || d_grad_score, "every output is NULL");
  PPBO_REQUIRE(ctx, M >= 1 && M <= (int64_t)0x7fffffff, "point count (1 .. 2^31 - 1)");
  const int D = model->D;
  AcqRound round;
  if (int rc = round.prepare(ctx, model, (int)(M < AQ_CHUNK ? M : AQ_CHUNK), with_field)) return rc;
  for (int64_t c0 = 0; c0 < M; c0 += AQ_CHUNK) {
    const int Mc = (int)((M - c0) < AQ_CHUNK ? (M - c0) : AQ_CHUNK);
    AcqOut o{d_mu ? d_mu + c0 : nullptr, d_var ? d_var + c0 : nullptr, d_score ? d_score + c0 : nullptr,
             d_grad_mu ? d_grad_mu + (size_t)c0 * D : nullptr, d_grad_var ? d_grad_var + (size_t)c0 * D : nullptr,
             d_grad_score ? d_grad_score + (size_t)c0 * D : nullptr};
    if (int rc = round.run(ctx, d_X + (size_t)c0 * D, Mc, score_kind, mustar, o, s)) return rc;
  }
  return 0;
}

int ppbo_acq_ascent(ppbo_ctx* ctx, const ppbo_model* model, const double* d_starts, int K, const double* h_box,
                    int score_kind, double mustar, int iters, double tol, double* d_x, double* d_score, double* d_mu,
                    double* d_var, int* d_iters, void* stream) {
  PPBO_ENTER(ctx);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = acq_check(ctx, model, score_kind, true)) return rc;      // (d_var is an output: the operator is read)
  PPBO_REQUIRE(ctx, d_starts && d_x && d_score && d_mu && d_var, "starts / outputs");
  PPBO_REQUIRE(ctx, K >= 1 && K <= AQ_CHUNK, "K (1 .. 1024)");
  PPBO_REQUIRE(ctx, iters >= 0 && iters <= 1000, "iters (0 .. 1000)");
  PPBO_REQUIRE(ctx, tol >= 0.0 && std::isfinite(tol), "tol (finite, >= 0)");
  const int D = model->D;
  double hb[3 * 64 + 1];
  double wmax = 0.0;
  for (int d = 0; d < D; ++d) {
    const double lo = h_box ? h_box[d] : 0.0, hi = h_box ? h_box[D + d] : 1.0;
    PPBO_REQUIRE(ctx, std::isfinite(lo) && std::isfinite(hi) && lo <= hi, "box: lo <= hi, finite");
    hb[d] = lo; hb[D + d] = hi; hb[2 * D + d] = hi - lo;
    if (hb[2 * D + d] > wmax) wmax = hb[2 * D + d];
  }
  hb[3 * D] = wmax;
  // the state, behind the field's arrays in their workspace: the box, three [K][D] and four [K] arrays of doubles, then
  // the two flag arrays (2 K ints = K doubles)
  const size_t KD = (size_t)K * D, n_dbl = (size_t)(3 * D + 1) + 3 * KD + 4 * (size_t)K;
  AcqRound round;
  if (int rc = round.prepare(ctx, model, K, true, n_dbl + (size_t)K)) return rc;
  double* box = round.state;
  AcqState a{};
  a.trial = box + (3 * D + 1); a.gt = a.trial + KD; a.g = a.gt + KD;
  a.st = a.g + KD; a.mut = a.st + K; a.vart = a.mut + K; a.step = a.vart + K;
  a.stopped = reinterpret_cast<int*>(a.step + K);
  a.it = d_iters ? d_iters : a.stopped + K;
  a.x = d_x; a.sc = d_score; a.mu = d_mu; a.var = d_var;
  if (int rc = ppbo_upload_async(ctx, box, hb, (size_t)(3 * D + 1) * sizeof(double), s)) return rc;
  acq_step_kernel<<<K, 64, 0, s>>>(D, -1, iters, tol, box, d_starts, a);
  PPBO_LAUNCH_CHECK(ctx);
  const AcqOut o{a.mut, a.vart, a.st, nullptr, nullptr, a.gt};
  for (int r = 0; r <= iters; ++r) {
    if (int rc = round.run(ctx, a.trial, K, score_kind, mustar, o, s)) return rc;
    acq_step_kernel<<<K, 64, 0, s>>>(D, r, iters, tol, box, d_starts, a);
    PPBO_LAUNCH_CHECK(ctx);
  }
  return 0;
}

}  // extern "C"
