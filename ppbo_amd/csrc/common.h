// Shared host/device helpers for libppbo_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <sched.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/ppbo_hip.h"

struct PpboUniqueId { char internal[128]; };   // layout of ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
struct ppbo_dist_state;                          // dist.hip: the RCCL communicator of a ctx

// A ctx owns private device workspaces (grown on demand, freed on destroy) and
// the last error string.  No global mutable state.
struct ppbo_ctx {
  int device = 0;
  std::string err;
  // named workspace slots
  enum { WS_KSTAR = 0, WS_PART, WS_SCRATCH, WS_LINALG, WS_LINALG2, WS_VEC, WS_SMALL, WS_POTRF, WS_APPEND, WS_DIST, WS_LBFGS, WS_SEARCH, WS_SEARCH_SMALL, WS_LBFGS_U, WS_TRANSPOSE, WS_GPAD, WS_SEARCH_ROWS, WS_SCALE, WS_SCALE_PTS, WS_SCALE_SEARCH, WS_EVGRAD, WS_EVGRAD_VEC, WS_CAMPHOR, WS_CAMPHOR_ROWS, WS_KSTAR_GEO, WS_MARGINAL, WS_TOURN_U, WS_TOURN_FIELD, WS_TOURN_K, WS_PROJECT, WS_PROJECT_SMALL, WS_PRUNE, WS_PRUNE_KC, WS_BATCH, WS_BATCH_K, WS_BOX, WS_BOX_SURV, WS_COUNT };
  void* ws[WS_COUNT] = {};
  size_t ws_bytes[WS_COUNT] = {};
  void* pinned = nullptr;  // small pinned host staging buffer
  size_t pinned_bytes = 0;
  // ring of pinned upload slots for small host arguments that travel by hipMemcpyAsync (ppbo_upload_async): a slot is
  // reused only after the event recorded behind its last copy has completed
  struct UploadSlot { void* p = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool used = false; };
  UploadSlot upload[4];
  unsigned upload_next = 0;
  // optional per-kernel event timing
  bool profiling = false;
  enum { PF_GRAM = 0, PF_KSTAR, PF_QUADFORM, PF_SCORE, PF_RFF_PROJECT, PF_RFF_SCORE, PF_POTRF, PF_LINE_KSTAR, PF_LINE_Y, PF_LINE_COV, PF_LINE_MC, PF_FUSED, PF_TOURNAMENT, PF_TOURNAMENT_FIELD, PF_BATCH_STEP, PF_BATCH_FIELD, PF_GRAD_KSTAR, PF_GRAD_FINISH, PF_ACQ_FIELD, PF_ACQ_GRAD, PF_KG, PF_COUNT };
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pf_events[PF_COUNT];
  size_t pf_used[PF_COUNT] = {};
  // kernels whose dynamic-LDS limit has been raised on THIS ctx's device (hipFuncSetAttribute is per device)
  std::vector<const void*> lds_raised;
  std::vector<int> lds_raised_bytes;
  // tuning knobs, read from the environment once per ctx (ppbo_ctx_create); defaults = measured best
  int qf_variant = 4, qf_order = -1, potrf_gen = 3, rff_nt = 0, gram_variant = -1, rff_score_mfma = 1;
  // PPBO_FUSED: 1 (default) = models of up to 1024 rows are scored by the one-launch kernel of fused.hip, 0 = always the
  // three-launch form (kstar -> quadform -> score)
  int fused_score = 1;
  // PPBO_KSTAR_STAR: 1 (default) = kstar_kernel forms the rows of a collinear star from two inner products per star
  // (star_geom_kernel's table), 0 = always one inner product per row
  int kstar_star = 1;
  // PPBO_PRUNE: 1 (default) = a search that returns only its best record (edge form, pointwise EI or VARIANCE, the
  // three-launch path) contracts the variance only for the candidates that a certified bound cannot rule out
  // (predict_passes), 0 = always for all.  PPBO_PRUNE_CAP (tests): the survivor capacity per chunk, 0 = a chunk's eighth
  int prune = 1, prune_cap = 0;
  // PPBO_PRUNE_THIN: 1 (default) = the compact launch of a pruned chunk with at most THIN_MAX survivors contracts them
  // on 16-column thin tiles (quadform_thin, predict.hip: the same bits), 0 = always on the tile shape of the launch;
  // a value above 1 (measurements: the sweep that set THIN_MAX) is the switch point itself
  int prune_thin = 1;
  int gemm_big16 = 1;     // PPBO_GEMM_BIG16: large GEMMs on 16 wavefronts of 32 x 32 (default since round 6) instead of 8 of 32 x 64
  int n_cu = 0;           // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  int fused_dbg = 0;      // PPBO_FUSED_DBG: measurement switches of fused.hip (results are wrong when set)
  // ppbo_gp_fit runs the triangular inverse and Sigma^-1 on a second stream beside the first evaluations of the f_MAP
  // search, which needs only L until the |grad_f| rule is armed (fit.hip)
  int fit_overlap = 1;    // PPBO_FIT_OVERLAP
  int fit_gf_from = 8;    // PPBO_FIT_GF_FROM: the first evaluation that may apply the |grad_f| rule in that mode
  // the host-polled searches let the runtime wait (hipStreamSynchronize) when their progress word has been still for
  // this long, and carry on if that advanced the search (PPBO_POLL_LIMIT_MS; tests set it to 0 to walk that path)
  int poll_limit_ms = 5000;
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int syrk_cfg = 0;       // PPBO_SYRK_CFG: tile configuration of Sigma^-1 = Linv^T Linv (0 = by size; 1 / 2 / 3 = 128 / 64 / 32)
  int line_y_chunk = 0;   // PPBO_LINE_Y_CHUNK: column tiles per chunk of Y = G K* in the line acquisition (0 = chosen by size)
  ppbo_dist_state* dist = nullptr;   // set by ppbo_dist_init
  // host-mapped (pinned, device-visible) result record: [0] value, [1] index as a double, [2] the epoch flag the
  // publishing kernel raises last; the host polls it (ppbo_host_record_wait)
  double* hostrec = nullptr;         // host address
  double* hostrec_dev = nullptr;     // the same memory as the device sees it
  unsigned long long hostrec_epoch = 0;
};

// Waiting on a host-mapped word without burning a core: spin with `pause` while the word keeps changing (a search
// slot is 5-50 us), yield the core once it has been still for a while (other contexts' threads -- evidence_batch runs
// eight -- and the Python interpreter get it), and report after `limit_s` seconds without a change.
struct PpboSpinWait {
  unsigned long long last = ~0ull;
  unsigned still = 0;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  double limit_s = 5.0;
  void reset() { still = 0; t_last = std::chrono::steady_clock::now(); }
  // true: the word has not changed for limit_s seconds
  bool idle(unsigned long long w) {
    if (w != last) { last = w; reset(); return false; }
    ++still;
    if (still < 2048) { __builtin_ia32_pause(); return false; }
    sched_yield();
    if ((still & 0xff) == 0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_last).count() > limit_s) return true;
    return false;
  }
};

// The chunks of a pass over M columns (points, lines), at most `cap` each: `for (const Chunk c : chunks)` walks them
// in order with the chunk's number, its first column and its size.  Mc_max: the largest (what workspaces are sized for)
struct Chunk { int64_t ch, beg; int Mc; };
struct Chunks {
  int64_t cap, M, n;
  int Mc_max;
  explicit Chunks(int64_t M_, int64_t cap_ = 65536)
      : cap(cap_), M(M_), n((M_ + cap_ - 1) / cap_), Mc_max((int)(M_ < cap_ ? M_ : cap_)) {}
  Chunk at(int64_t ch) const { return Chunk{ch, ch * cap, (int)((M - ch * cap) < cap ? (M - ch * cap) : cap)}; }
  struct It {
    const Chunks* c;
    int64_t ch;                    // (what a range-for needs)
    Chunk operator*() const { return c->at(ch); }
    void operator++() { ++ch; }
    bool operator!=(const It& o) const { return ch != o.ch; }
  };
  It begin() const { return It{this, 0}; }   It end() const { return It{this, n}; }
};

struct PpboHostRecord {
  double* d_rec;                     // device view of the record (2 doubles)
  unsigned long long* d_flag;        // device view of the flag
  const volatile double* h_rec;      // host view
  unsigned long long epoch;          // the value the flag takes when the record is complete
};
// a fresh epoch on the ctx's host-mapped record (allocated on first use)
int ppbo_host_record(ppbo_ctx* ctx, PpboHostRecord* out);
// spin until the kernel enqueued on `s` has raised the flag to the record's epoch; falls back to a stream
// synchronisation (and reports an error if the flag still is not there: the kernel did not run to completion)
int ppbo_host_record_wait(ppbo_ctx* ctx, const PpboHostRecord& r, hipStream_t s);
// fused.hip: the one-launch scoring path (K*, contraction, score in one kernel) for models of up to 1024 rows
struct ppbo_model;
bool ppbo_fused_eligible(const ppbo_ctx* ctx, const ppbo_model* m);
const double* ppbo_fused_transposed_G(ppbo_ctx* ctx, const ppbo_model* m, int* ldgt_out, hipStream_t s);
int ppbo_fused_score(ppbo_ctx* ctx, const ppbo_model* m, const double* Gt, int ldgt, const double* d_Xc, long long M,
                     int score_kind, double mustar, long long idx_base, double* d_mu, double* d_var, double* d_score,
                     void* blk_best, hipStream_t s);
// predict.hip, for dist.hip: one shard's scoring passes with the record published to host-mapped memory
int ppbo_predict_record_publish(ppbo_ctx* ctx, const ppbo_model* model, const double* d_Xc, int64_t M, int score_kind,
                                double mustar, int64_t index_offset, double* d_record, unsigned long long* d_flag,
                                unsigned long long epoch, hipStream_t s);
// predict.hip, for project.hip: E [N][ld] = the edge-layout rows of the node-layout Kt [N][ld] (edge_apply_kernel), M columns
int ppbo_edge_apply_async(ppbo_ctx* ctx, const double* Kt, int ld, int M, int N, int mblk, const double* d_lam_off, double* E,
                          hipStream_t s);
// the row splits of a K* launch (row_split, predict.hip): pick_split's count, the stars per split, the splits that hold a star
struct RowSplit { int n_split, q_per_split, n_split_eff; };
// predict.hip, for acq.hip: the field pass of a tournament, U [NkU][ldu] = (Lambda + M'M) K* for the Mb <= Mb_max <= 1024
// points d_Xb in the row layout of the model's form, beside K* (KB, node layout) and Y = M K* [N][ldu] each; Z [N][ldu] is
// scratch, part [split.n_split_eff][Mb_max] the mean partials of its K* launch.  prepare(): U, and ONE WS_TOURN_FIELD of KB,
// Y, Z, head_doubles, part, extra_doubles; returns the caller's extra (NULL: out of memory).  gemm_cfg: GemmArgs.force_cfg
struct FieldPass {
  const ppbo_model* model = nullptr;
  int ldu = 0, NkU = 0;
  RowSplit split{};
  double *U = nullptr, *KB = nullptr, *Y = nullptr, *Z = nullptr, *head = nullptr, *part = nullptr;
  double* prepare(ppbo_ctx* ctx, const ppbo_model* m, int Mb_max, const RowSplit& rs, size_t extra_doubles, size_t head_doubles = 0);
  int run(ppbo_ctx* ctx, const double* d_Xb, int Mb, hipStream_t s, int gemm_cfg = 0) const;
};

// kg.hip, for predict.hip: the envelope march behind a chunk's cross product.  ppbo_kg_rows: d_s = sqrt(max(var, 0) +
// noise_var) and the own line's slope d_self_b = max(var, 0) / d_s for M rows.  ppbo_kg_launch: the knowledge gradient of
// Ma rows of lines (ppbo_kg_envelope's arguments; the slopes divided by d_div[row] on the way in when d_div is given),
// rows numbered from idx_base in the ppbo_kg_blocks(Ma, Mb) per-workgroup bests blk_best (a Best each; NULL: none);
// d_Xa [Ma][D], d_Xb [Mb][D]: the points behind the lines (NULL: none) -- a field point that is the row's candidate, bit
// for bit, takes the own line's slope
long long ppbo_kg_blocks(long long Ma, int Mb);
int ppbo_kg_rows(ppbo_ctx* ctx, const double* d_var, double noise_var, int M, double* d_s, double* d_self_b, hipStream_t s);
int ppbo_kg_launch(ppbo_ctx* ctx, const double* d_a, const double* d_slope, long long ld, const double* d_div,
                   const double* d_self_a, const double* d_self_b, long long Ma, int Mb, long long idx_base, double* d_kg,
                   int* d_kinks, void* blk_best, hipStream_t s, const double* d_Xa = nullptr, const double* d_Xb = nullptr,
                   int D = 0);

// answers.hip, for predict.hip: scores Bc groups of G points (point 0 the chosen one) whose means mu [Bc][G] and
// covariances cov [Bc][G][G] (+ cov_parts: mc_factor_lds' slabs) are on the device -- the closed-form edge probabilities
// into d_edge [Bc][G] (column 0 the agreement) and d_agree [Bc], the Monte-Carlo log score of the S draws d_z [S][G] into
// d_lpd [Bc]; any of the three may be NULL, S = 0 skips the draws
int ppbo_answer_score_groups(ppbo_ctx* ctx, const double* mu, const double* cov, int Bc, int G, double sigma,
                             const double* d_z, int S, double jitter, const double* cov_parts, int n_parts,
                             long long part_stride, int parts_lower_only, double* d_lpd, double* d_agree, double* d_edge,
                             hipStream_t s);

// first row / column of an edge-form operator that the contractions read: the n_q observation coordinates hold zeros,
// the K loops start at n_q rounded down to the chunk depth
inline int ppbo_edge_k0(int n_q) { return n_q & ~15; }

// Every extern "C" entry runs on its ctx's device and leaves the caller's current device as it found it.
struct PpboDeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit PpboDeviceGuard(const ppbo_ctx* c) {
    if (c && hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = (hipSetDevice(c->device) == hipSuccess);
  }
  ~PpboDeviceGuard() { if (switched) (void)hipSetDevice(prev); }
  PpboDeviceGuard(const PpboDeviceGuard&) = delete;
  PpboDeviceGuard& operator=(const PpboDeviceGuard&) = delete;
};
#define PPBO_ENTER(ctx)      \
  if (!(ctx)) return -1;     \
  PpboDeviceGuard _ppbo_dev_guard(ctx)

// RAII bracket: records two events around a launch when profiling is on
struct PpboProfScope {
  ppbo_ctx* ctx; int slot; hipStream_t s; hipEvent_t stop = nullptr;
  PpboProfScope(ppbo_ctx* c, int slot_, hipStream_t s_) : ctx(c), slot(slot_), s(s_) {
    if (!ctx || !ctx->profiling) return;
    auto& v = ctx->pf_events[slot];
    if (ctx->pf_used[slot] == v.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      v.emplace_back(a, b);
    }
    auto& pr = v[ctx->pf_used[slot]++];
    (void)hipEventRecord(pr.first, s);
    stop = pr.second;
  }
  ~PpboProfScope() { if (stop) (void)hipEventRecord(stop, s); }
};

int ppbo_set_error(ppbo_ctx* ctx, int code, const char* fmt, ...);
// returns a device pointer of at least `bytes` (contents undefined); nullptr on failure
void* ppbo_workspace(ppbo_ctx* ctx, int slot, size_t bytes);
void* ppbo_pinned(ppbo_ctx* ctx, size_t bytes);
// copies h_src (any host memory; consumed before the call returns) to d_dst through a pinned slot of the ctx, truly
// asynchronously on `s`: neither blocks the host on the stream nor relies on how the runtime stages pageable memory
int ppbo_upload_async(ppbo_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, hipStream_t s);
// raise a kernel's dynamic-LDS limit to `bytes` once per ctx (i.e. once per device)
void ppbo_lds_limit(ppbo_ctx* ctx, const void* kernel_fn, int bytes);

#define PPBO_HIP_CHECK(ctx, expr)                                                      \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return ppbo_set_error((ctx), (int)_e, "%s failed: %s (%s:%d)", #expr,            \
                            hipGetErrorString(_e), __FILE__, __LINE__);                \
  } while (0)

#define PPBO_LAUNCH_CHECK(ctx) PPBO_HIP_CHECK(ctx, hipGetLastError())

#define PPBO_REQUIRE(ctx, cond, msg)                                    \
  do {                                                                  \
    if (!(cond)) return ppbo_set_error((ctx), -1, "invalid argument: %s", msg); \
  } while (0)

// the form of a variance operator: ppbo_model.form, or the form parameter of ppbo_posterior / ppbo_gp_fit
#define PPBO_REQUIRE_FORM(ctx, form) \
  PPBO_REQUIRE(ctx, (form) == PPBO_FORM_NODE || (form) == PPBO_FORM_EDGE, "form (PPBO_FORM_NODE or PPBO_FORM_EDGE)")

// an entry point's kernel id and the camphor kernel's shape rule (D is the design's dimension)
#define PPBO_REQUIRE_KERNEL(ctx, kernel_id, D)                                                  \
  do {                                                                                          \
    PPBO_REQUIRE(ctx, ppbo_kernel_id_valid(kernel_id), "kernel_id");                            \
    PPBO_REQUIRE(ctx, (kernel_id) != PPBO_KERNEL_CAMPHOR || (D) == 6, "camphor kernel needs D == 6"); \
  } while (0)

// fn(std::integral_constant<int, KID>{}) for the runtime kernel id, returning fn's status.  RADIAL_ONLY leaves camphor-
// copper out at compile time (nothing is instantiated for it).  An id without a branch sets `err` on ctx (a NULL ctx
// sets nothing) and returns -1.
template <bool RADIAL_ONLY = false, class Fn>
static inline int ppbo_kernel_dispatch(ppbo_ctx* ctx, int kernel_id, Fn&& fn,
                                       const char* err = "invalid argument: kernel_id") {
  switch (kernel_id) {
    case PPBO_KERNEL_SE: return fn(std::integral_constant<int, PPBO_KERNEL_SE>{});
    case PPBO_KERNEL_RQ: return fn(std::integral_constant<int, PPBO_KERNEL_RQ>{});
    case PPBO_KERNEL_MATERN52: return fn(std::integral_constant<int, PPBO_KERNEL_MATERN52>{});
    case PPBO_KERNEL_MATERN32: return fn(std::integral_constant<int, PPBO_KERNEL_MATERN32>{});
    case PPBO_KERNEL_CAMPHOR:
      if constexpr (!RADIAL_ONLY) return fn(std::integral_constant<int, PPBO_KERNEL_CAMPHOR>{});
      break;
    default: break;
  }
  return ppbo_set_error(ctx, -1, "%s", err);
}

// The padded dimensions DP a kernel template is instantiated for, in rising order.  pick(D): the first rung >= D, the
// last rung for everything above.  dispatch(D, fn): fn(std::integral_constant<int, pick(D)>{}), returning what fn returns.
// A ladder is named once, next to the kernel it serves.
template <int... DPS>
struct DpLadder {
  static constexpr int rungs[] = {DPS...};
  static constexpr int pick(int D) {
    for (int r : rungs)
      if (D <= r) return r;
    return rungs[sizeof...(DPS) - 1];
  }
  template <class Fn>
  static decltype(auto) dispatch(int D, Fn&& fn) { return step<DPS...>(pick(D), fn); }

 private:
  template <int DP, int... REST, class Fn>
  static decltype(auto) step(int dp, Fn& fn) {
    if constexpr (sizeof...(REST) == 0) return fn(std::integral_constant<int, DP>{});
    else if (dp == DP) return fn(std::integral_constant<int, DP>{});
    else return step<REST...>(dp, fn);
  }
};
static_assert(DpLadder<4, 6, 64>::pick(1) == 4 && DpLadder<4, 6, 64>::pick(4) == 4, "a rung takes D up to itself");
static_assert(DpLadder<4, 6, 64>::pick(5) == 6 && DpLadder<4, 6, 64>::pick(7) == 64 && DpLadder<4, 6, 64>::pick(64) == 64,
              "the next rung starts one above");
static_assert(DpLadder<4, 6, 64>::pick(65) == 64 && DpLadder<6>::pick(100) == 6, "the last rung takes everything above");

// ---- kernel-function parameters (host-prepared, passed by value) ------------
struct KernParams {
  double sf2;      // sigma_f^2
  double c0;       // SE: 0.5/l^2     RQ: 1/(4 l^2)    camphor: 2/l^2    Matern-5/2: sqrt(5)/l    Matern-3/2: sqrt(3)/l
  double c1;       // camphor: 0.5/(l+0.05)^2
};

// the kernel ids every entry point accepts (include/ppbo_hip.h); anything else is "invalid argument"
static inline bool ppbo_kernel_id_valid(int kernel_id) {
  return kernel_id == PPBO_KERNEL_SE || kernel_id == PPBO_KERNEL_RQ || kernel_id == PPBO_KERNEL_CAMPHOR ||
         kernel_id == PPBO_KERNEL_MATERN52 || kernel_id == PPBO_KERNEL_MATERN32;
}
// Matern kernels: functions of r = sqrt(r^2), evaluated from the same summed r^2 as SE / RQ
template <int KID>
constexpr bool kid_matern = (KID == PPBO_KERNEL_MATERN52 || KID == PPBO_KERNEL_MATERN32);
// radial kernels: every path that forms r^2 (expansion or direct differences) takes them
template <int KID>
constexpr bool kid_radial = (KID == PPBO_KERNEL_SE || KID == PPBO_KERNEL_RQ || kid_matern<KID>);

static inline KernParams make_kern_params(int kernel_id, const double theta[3]) {
  KernParams p;
  const double l = theta[1], sf = theta[2];
  p.sf2 = sf * sf;
  p.c1 = 0.0;
  p.c0 = 0.0;
  switch (kernel_id) {
    case PPBO_KERNEL_SE: p.c0 = 0.5 / (l * l); break;
    case PPBO_KERNEL_RQ: p.c0 = 1.0 / (4.0 * l * l); break;
    case PPBO_KERNEL_CAMPHOR: p.c0 = 2.0 / (l * l); p.c1 = 0.5 / ((l + 0.05) * (l + 0.05)); break;
    case PPBO_KERNEL_MATERN52: p.c0 = 2.23606797749978969641 / l; break;
    case PPBO_KERNEL_MATERN32: p.c0 = 1.73205080756887729353 / l; break;
    default: break;   // rejected by every entry point before a launch (ppbo_kernel_id_valid)
  }
  return p;
}

#ifdef __HIPCC__
typedef double double4_t __attribute__((ext_vector_type(4)));

// Write-through ("sc1") global stores for bulk results that the NEXT kernel reads: a plain store leaves the
// line dirty in the XCD's L2 and the whole dirty footprint is written back when the kernel ends -- serial
// time on a chain of dependent launches (measured: 3-4 us per Cholesky step with 16 MB of dirty tiles).
// hipcc does not count an asm store in vmcnt; that only makes its waits for earlier loads conservative.
__device__ __forceinline__ void store_through(double* p, double v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
typedef double double2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_through2(double* p, double x, double y) {
  const double2_t v = {x, y};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// *p for a wave-uniform p into memory that no launch in flight writes (model arrays, a table the previous launch left):
// through the constant address space, so the value arrives by a scalar load and occupies no vector register
__device__ __forceinline__ double uniform_load(const double* p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) double*>(reinterpret_cast<uintptr_t>(p));
}

// the value lane ^ 1 holds (DPP quad_perm [1,0,3,2]): two 32-bit moves, no LDS
__device__ __forceinline__ double lane_xor1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// 64-lane wavefront reductions (gfx950: wave = 64)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// The same sum without the LDS crossbar: __shfl_xor compiles to ds_bpermute_b32, and a workgroup of 16 wavefronts
// that all reduce through it is bound by the CU's one LDS pipe (measured: 12 us for 25 sums x 16 waves).  DPP moves
// are plain VALU instructions: xor 1, xor 2 (quad_perm), row_half_mirror, row_mirror give every lane its row-of-16
// sum; the four row sums are combined through scalar registers (v_readlane).  Fixed order: bitwise reproducible.
__device__ __forceinline__ double dpp_add(double v, const int ctrl_selector) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  switch (ctrl_selector) {
    case 0: lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true); break;
    case 1: lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true); break;
    case 2: lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true); break;
    default: lo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true); break;
  }
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_sum_dpp(double v) { return dpp_add(dpp_add(v, 0), 1); }
// sum over each row of 16 lanes (every lane of the row ends with the row's sum): four DPP steps, no LDS, no readlane
__device__ __forceinline__ double row16_sum_dpp(double v) { return dpp_add(dpp_add(dpp_add(dpp_add(v, 0), 1), 2), 3); }
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v = dpp_add(dpp_add(dpp_add(dpp_add(v, 0), 1), 2), 3);
  double r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    r[k] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 16 * k),
                            __builtin_amdgcn_readlane(__double2loint(v), 16 * k));
  return (r[0] + r[1]) + (r[2] + r[3]);
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// exp(x) for x <= 0 (every covariance kernel's exponent): Cody-Waite reduction by ln2, degree-11 near-minimax
// polynomial on |r| <= ln2/2 (fit error 3e-18, tools/expfit.py), scaling by v_ldexp_f64.  18 VALU
// instructions and no special-case branches (the library exp spends as many again on range checks);
// measured against 50-digit arithmetic: <= 1 ulp.
__device__ __forceinline__ double exp_nonpos(double x) {
  x = fmax(x, -750.0);                       // exp underflows to 0 below -745.2; keeps (int)n in range
  const double n = __builtin_rint(x * 1.4426950408889634);
  double r = __builtin_fma(n, -6.93147180369123816490e-01, x);
  r = __builtin_fma(n, -1.90821492927058770002e-10, r);
  double q = 0x1.af632a0f7e2cep-26;
  q = __builtin_fma(q, r, 0x1.28b4101c77212p-22);
  q = __builtin_fma(q, r, 0x1.71ddf56d8deb5p-19);
  q = __builtin_fma(q, r, 0x1.a01991a10d9aep-16);
  q = __builtin_fma(q, r, 0x1.a01a01b1461c5p-13);
  q = __builtin_fma(q, r, 0x1.6c16c1880029fp-10);
  q = __builtin_fma(q, r, 0x1.111111110f21ep-7);
  q = __builtin_fma(q, r, 0x1.555555554f0bap-5);
  q = __builtin_fma(q, r, 0x1.555555555555ap-3);
  q = __builtin_fma(q, r, 0x1.0000000000011p-1);
  q = __builtin_fma(q, r, 1.0);
  q = __builtin_fma(q, r, 1.0);
  return ldexp(q, (int)n);
}

// sqrt(s) for s >= 0 without the library's range handling: v_rsq_f64, then the Goldschmidt refinement the compiler
// itself emits for sqrt() (one step on (g, h) = (s y, y / 2), two corrections of g against the residual s - g^2).
// 9 VALU instructions in one dependent chain, one of them a transcendental; s = 0 (rsq = inf) selects 0.
__device__ __forceinline__ double sqrt_nonneg(double s) {
  const double y = __builtin_amdgcn_rsq(s);
  double g = s * y, h = 0.5 * y;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double d = __builtin_fma(-g, g, s);
  g = __builtin_fma(d, h, g);
  d = __builtin_fma(-g, g, s);
  g = __builtin_fma(d, h, g);
  return s > 0.0 ? g : 0.0;
}

// Matern pieces from r^2 (clipped at 0 by the caller): a = c r and e = exp(-a), formed once per pair and shared by the
// value and the gradient.
struct MaternAE { double a, e; };
template <int KID>
__device__ __forceinline__ MaternAE matern_ae(double s, const KernParams& p) {
  static_assert(kid_matern<KID>, "Matern kernels only");
  // (a capped where e is already 0: the value and gradient stay 0, never inf * 0, for the far rows some paths stage
  // with r^2 = 1e300)
  const double a = fmin(p.c0 * sqrt_nonneg(s), 800.0);
  return MaternAE{a, exp_nonpos(-a)};
}
//   5/2: sf2 (1 + a + a^2/3) e      3/2: sf2 (1 + a) e          (times `scale` = sf2 or (1 - shrink) sf2)
template <int KID>
__device__ __forceinline__ double matern_value(const MaternAE& m, double scale) {
  if constexpr (KID == PPBO_KERNEL_MATERN52) {
    return scale * (__builtin_fma(m.a, __builtin_fma(m.a, 1.0 / 3.0, 1.0), 1.0) * m.e);
  } else {
    static_assert(KID == PPBO_KERNEL_MATERN32, "Matern kernels only");
    return scale * ((1.0 + m.a) * m.e);
  }
}
// g with grad_x k(x, x') = g (x - x'):   5/2: -sf2 (c^2/3) (1 + a) e      3/2: -sf2 c^2 e      (finite at r = 0)
template <int KID>
__device__ __forceinline__ double matern_grad(const MaternAE& m, const KernParams& p) {
  const double c2 = p.c0 * p.c0;
  if constexpr (KID == PPBO_KERNEL_MATERN52) {
    return -(p.sf2 * c2 * (1.0 / 3.0)) * ((1.0 + m.a) * m.e);
  } else {
    static_assert(KID == PPBO_KERNEL_MATERN32, "Matern kernels only");
    return -(p.sf2 * c2) * m.e;
  }
}

// Kernel value from accumulated per-dimension terms.
//   SE / RQ / Matern : s = sum_d (x_d - y_d)^2
//   camphor : s = c0 * sum_{d in 0,1,3,4,5} sin^2(pi |dx_d|) + c1 * dx_2^2  (already scaled)
template <int KID>
__device__ __forceinline__ double kern_finish(double s, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    return p.sf2 * exp_nonpos(-p.c0 * s);
  } else if constexpr (KID == PPBO_KERNEL_RQ) {
    const double t = 1.0 + s * p.c0;
    return p.sf2 / (t * t);
  } else if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    return p.sf2 * exp_nonpos(-s);
  } else {
    static_assert(kid_matern<KID>, "unknown kernel id");
    return matern_value<KID>(matern_ae<KID>(s, p), p.sf2);
  }
}

// g with grad_x k = g (x - x') for SE / RQ, from w = alpha k (the ascent's and mean_grad's form; Matern: matern_grad)
template <int KID>
__device__ __forceinline__ double kern_grad_coef(double s, double w, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_SE) {
    return -2.0 * p.c0 * w;
  } else {
    static_assert(KID == PPBO_KERNEL_RQ, "SE / RQ only");
    return -4.0 * p.c0 * w / (1.0 + p.c0 * s);
  }
}

template <int KID>
__device__ __forceinline__ double kern_term(double dx, int d, const KernParams& p) {
  if constexpr (KID == PPBO_KERNEL_CAMPHOR) {
    if (d == 2) return p.c1 * dx * dx;
    const double sn = sinpi(fabs(dx));
    return p.c0 * sn * sn;
  } else {
    static_assert(kid_radial<KID>, "unknown kernel id");
    return dx * dx;
  }
}
#endif
