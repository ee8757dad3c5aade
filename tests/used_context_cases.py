"""The cases of tests/test_gpu_used_context.py: every checked call, the three histories that run before it on a used
engine (larger, non-finite, smaller), the neighbours sequence and the NumPy reference of every call -- test infrastructure
only, importable without a GPU (nothing here touches torch or the library until a run function is called).

A case is a run function run(eng, variant) -> {name: array or scalar} with variant one of VARIANTS:

  checked     the call that is compared bit for bit
  larger      the same entry, other seed, strictly larger in every dimension that sizes a workspace, other operator form
              and kernel family where the entry takes them
  nonfinite   the larger call with inputs that leave NaN / Inf behind (CASE.doc names the header line or the test that
              documents the input as accepted); an expected error return is caught by the caller
  smaller     the same entry at the smallest legal sizes

Inputs are functions of (case, variant) alone (seeded), so the checked call is the same call on every engine.  The
scoring entries run on hand-built posteriors in the layout of synth_post() (tests/test_gpu_fused.py): Lambda in star form,
the node-form G block lower triangular with explicit zeros, the edge-form H lower triangular with zero observation rows
and columns (operator() of tests/test_gpu_kstar_star.py).  Their dense variance operator A (var = prior - k' A k) feeds the
NumPy twins of the predictors."""
from __future__ import annotations

import ctypes as C
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import ppbo_oracle as orc

VARIANTS = ("checked", "larger", "nonfinite", "smaller")
FORM_NODE, FORM_EDGE = 0, 1          # PPBO_FORM_NODE / PPBO_FORM_EDGE (include/ppbo_hip.h; ppbo_amd.engine re-exports them)
TOL = 1e-6                           # the package's parity tolerance (README, "Parity"): every predictor's test file
EPS = np.finfo(float).eps

# ---- tile constants, quoted from the code -----------------------------------------------------------------------------
CAND_TILE = 128      # csrc/predict.hip, predict_passes: ldk = (Mc_max + 127) & ~127 -- K* padded to whole candidate tiles
K_CHUNK = 16         # csrc/predict.hip, predict_passes: "K extent Nk = N rounded up to the chunk depth" (gemm_f64.h BK = 16)
FUSED_BN = 32        # csrc/fused.hip: FS_BN = 32 candidates per workgroup of the one-launch kernel
GPAD_FROM = 2048     # csrc/predict.hip, predict_passes: padded_G(..., M >= 2048, ...) -- the zero-framed copy of G
DENSE_NB = 64        # csrc/linalg.hip: NB = 64 (potrf / trtri panels); csrc/gram.hip and csrc/rff.hip: TS = 64 tile side
LU_NB = 16           # csrc/lu.hip: LNB = 16 columns per LU panel
POINT_BLOCK = 256    # csrc/meangrad.hip, csrc/camphor.hip: (n + 255) / 256 blocks of 256 elements
GRAD_CHUNK = 512     # csrc/predict.hip, ppbo_predict_gradients: GRAD_CHUNK = 512 points per chunk
LINE_ROWS = 512      # csrc/predict.hip: LC_MAXROWS = 512 rows of one (line, slice) workgroup


def ceil_div(a, b):
    return -(-int(a) // int(b))


def tiles(d):
    """The tile / chunk counts of a call with the sizing dimensions d (whichever of them the entry has)."""
    t = {}
    if "M" in d:
        t["cand_tiles"] = ceil_div(d["M"], CAND_TILE)
        t["fused_blocks"] = ceil_div(d["M"], FUSED_BN)
        t["gpad"] = int(d["M"] >= GPAD_FROM)
        t["grad_chunks"] = ceil_div(d["M"], GRAD_CHUNK)
    if "N" in d:
        t["k_chunks"] = ceil_div(d["N"], K_CHUNK)
        t["panels"] = ceil_div(d["N"], DENSE_NB)
        t["lu_panels"] = ceil_div(d["N"], LU_NB)
    if "F" in d:
        t["feature_tiles"] = ceil_div(d["F"], DENSE_NB)
    if "B" in d and "G" in d:
        t["line_tiles"] = ceil_div(d["B"] * d["G"], CAND_TILE)
    if "P" in d:
        t["point_blocks"] = ceil_div(d["P"], POINT_BLOCK)
    return t


# ---- the registry -------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str                 # fit / predict / rff / lu / predictor / line / dense / search / points (the neighbours order)
    slots: tuple                # the WS_* slots the entry requests (read off the code)
    dims: dict                  # variant -> {dimension: size}; "nonfinite" runs at the larger sizes
    doc: str                    # where the non-finite input is documented as accepted
    run: object
    ref: object
    env: tuple = ()             # PPBO_* settings of the engine, ((name, value), ...)
    legal: object = None        # smaller: (n_q, m, N) where the entry has a design

    def sizes(self, variant):
        return self.dims["larger" if variant == "nonfinite" else variant]


CASES = {}


def register(name, family, slots, dims, doc, env=(), legal=None):
    def deco(pair):
        run, ref = pair()
        CASES[name] = Case(name, family, tuple(slots), dims, doc, run, ref, tuple(sorted(dict(env).items())), legal)
        return pair
    return deco


def rng_of(name, variant):
    """The larger and the non-finite call share a seed (the same call but for the poisoned inputs)."""
    v = "larger" if variant == "nonfinite" else variant
    return np.random.default_rng(zlib.crc32(f"{name}:{v}".encode()))


def host(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        return t.detach().cpu().numpy()
    return np.asarray(t)


def outputs(**kw):
    return {k: host(v) for k, v in kw.items() if v is not None}


def rel(a, b):
    """max|a - b| / max|b| (tests/test_gpu_parity.py: the norm its relative tolerances are stated in)."""
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


# ---- hand-built posteriors ------------------------------------------------------------------------------------------------
def star_rows(rng, n_q, m, D):
    """n_q stars of m + 1 rows inside the unit box: an observation and m points on a line through it."""
    X = np.empty((n_q, m + 1, D))
    for q in range(n_q):
        xo = 0.3 + 0.4 * rng.random(D)
        xi = rng.uniform(0.2, 1.0, D) * rng.choice([-1.0, 1.0], D)
        s = rng.uniform(-0.3, 0.3, m)
        X[q, 0] = xo
        X[q, 1:] = xo + s[:, None] * xi
    return X.reshape(n_q * (m + 1), D)


class HostModel:
    """A posterior state on the host and its device twin on any engine."""

    def __init__(self, seed, n_q, m, D, kernel, form, theta=None):
        rng = np.random.default_rng(seed)
        N = n_q * (m + 1)
        self.n_q, self.m, self.D, self.N, self.kernel, self.form = n_q, m, D, N, kernel, form
        self.theta = (0.05, 0.35 * np.sqrt(D / 3.0), 0.7) if theta is None else theta
        sf = float(self.theta[2])
        self.sf2 = sf * sf
        self.X = star_rows(rng, n_q, m, D)
        self.alpha = rng.standard_normal(N)
        self.ld = -np.abs(rng.standard_normal(N)) * 0.3 / (N * self.sf2)
        self.lo = np.abs(rng.standard_normal(N)) * 0.1 / (N * self.sf2)
        self.lo[::m + 1] = 0.0
        i, j = np.indices((N, N))
        if form == FORM_EDGE:
            G = np.where(j <= i, rng.standard_normal((N, N)), 0.0) * sf * np.sqrt(N)
            G[:n_q] = 0.0
            G[:, :n_q] = 0.0
            G[np.arange(n_q, N), np.arange(n_q, N)] = (0.5 + rng.random(N - n_q)) * sf * np.sqrt(N)
        else:
            G = np.where(j // (m + 1) <= i // (m + 1), rng.standard_normal((N, N)), 0.0) * 0.3 / (sf * np.sqrt(N))
        self.G = G

    def on(self, eng, alpha=None, G=None):
        from ppbo_amd.engine import Posterior
        return Posterior(self.kernel, tuple(self.theta), self.m, eng.dev(self.X), eng.dev(self.alpha if alpha is None else alpha),
                         eng.dev(self.ld), eng.dev(self.lo), eng.dev(self.G if G is None else G), form=self.form)

    def lam_dense(self):
        lam = np.diag(self.ld)
        j = np.arange(self.N)
        pse = j[j % (self.m + 1) != 0]
        obs = pse // (self.m + 1) * (self.m + 1)
        lam[obs, pse] = self.lo[pse]
        lam[pse, obs] = self.lo[pse]
        return lam

    def edge_map(self):
        """B [N, N] with E = B k: rows n_q.. hold lam_off_j (k_j - k_obs(j)), star by star (mean_var_ref of
        tests/test_gpu_kstar_star.py)."""
        B = np.zeros((self.N, self.N))
        mb = self.m + 1
        for q in range(self.n_q):
            for jj in range(1, mb):
                r, c = self.n_q + q * self.m + jj - 1, q * mb + jj
                B[r, c] = self.lo[c]
                B[r, q * mb] = -self.lo[c]
        return B

    @functools.cached_property
    def A(self):
        """var = prior - k' A k: A = -(Lambda + (G B)' (G B)), B = I in node form."""
        GB = self.G @ self.edge_map() if self.form == FORM_EDGE else self.G
        return -(self.lam_dense() + GB.T @ GB)

    def args(self):
        return self.X, list(self.theta), self.kernel, self.alpha, self.A

    def mean_var(self, Xc):
        import pairs_numpy as pn
        K = pn.cross(Xc, self.X, self.theta, self.kernel)
        return K @ self.alpha, self.sf2 - np.einsum("ij,ij->i", K, K @ self.A)


# (n_q, m, D, kernel, form) per variant: N = 78 off every tile edge in D = 3, N = 32 in D = 6; the larger histories N = 216
# (m = 26, not 25: m sizes the star slabs, so it grows too) and N = 160 in D = 7 and D = 21 (other dimension buckets), the
# other operator form and the RQ family; "Am": a product kernel on both sides, for the marginals.
MODELS = {
    "A": dict(checked=(3, 25, 3, "SE_kernel", FORM_NODE), larger=(8, 26, 7, "RQ_kernel", FORM_EDGE),
              smaller=(1, 1, 1, "SE_kernel", FORM_NODE)),
    "B": dict(checked=(8, 3, 6, "SE_kernel", FORM_EDGE), larger=(16, 9, 21, "RQ_kernel", FORM_NODE),
              smaller=(1, 1, 1, "SE_kernel", FORM_EDGE)),
    "Am": dict(checked=(3, 25, 3, "SE_kernel", FORM_NODE), larger=(8, 26, 7, "SE_kernel", FORM_EDGE),
               smaller=(1, 1, 2, "SE_kernel", FORM_NODE)),
}


@functools.lru_cache(maxsize=None)
def model(key, variant):
    v = "larger" if variant == "nonfinite" else variant
    n_q, m, D, kernel, form = MODELS[key][v]
    return HostModel(zlib.crc32(f"model:{key}:{v}".encode()), n_q, m, D, kernel, form)


def model_dims(key, **extra):
    """{variant: sizes} of a case on model `key`; extra: name -> (checked, larger, smaller)."""
    out = {}
    for i, v in enumerate(("checked", "larger", "smaller")):
        n_q, m, D, _, _ = MODELS[key][v]
        out[v] = dict(N=n_q * (m + 1), m=m, n_q=n_q, D=D, **{k: t[i] for k, t in extra.items()})
    return out


def model_legal(key):
    n_q, m, _, _, _ = MODELS[key]["smaller"]
    return n_q, m, n_q * (m + 1)


def points(rng, mod, M, variant, per=7):
    """M candidates in the box, a few of them design rows; non-finite: every per-th row has a NaN or an infinite coordinate."""
    X = rng.random((M, mod.D))
    k = min(4, M // 4)
    if k:
        X[:k] = mod.X[rng.integers(0, mod.N, k)]
    if variant == "nonfinite":
        X[::per, 0] = np.nan
        X[3::2 * per, -1] = np.inf
    return X


NAN_ROWS = "include/ppbo_hip.h: 'A candidate row with any NaN or infinite coordinate gets NaN in d_mu, d_var and d_score'"
M_SIZES = dict(M=(130, 1000, 1))


# ============================================================ scoring ====================================================
def _predict_case(name, key, score, M, env=(), fp32=False, slots=(), larger_M=1000):
    dims = model_dims(key, M=(M, larger_M, 1))

    @register(name, "predict", slots, dims, NAN_ROWS, env, model_legal(key))
    def _():
        def run(eng, v):
            mod = model(key, v)
            Xc = points(rng_of(name, v), mod, dims["larger" if v == "nonfinite" else v]["M"], v)
            o = eng.predict(mod.on(eng), Xc, score=score, mustar=0.1, want_score=True, kstar_fp32=fp32)
            return outputs(mu=o["mu"], var=o["var"], score=o["score"], best_val=o["best_val"], best_idx=o["best_idx"])

        def ref(out):
            mod = model(key, "checked")
            Xc = points(rng_of(name, "checked"), mod, M, "checked")
            mu0, var0 = mod.mean_var(Xc)
            if fp32:       # tests/test_gpu_parity.py: the fp32-K* report path
                assert np.abs(out["mu"] - mu0).max() <= 1e-3 * np.abs(mu0).max()
                assert np.abs(out["var"] - var0).max() <= 1e-2 * mod.sf2
            elif mod.form == FORM_NODE:      # tests/test_gpu_fused.py: dense_reference
                assert np.abs(out["mu"] - mu0).max() <= 1e-11 * np.abs(mu0).max()
                assert np.abs(out["var"] - var0).max() <= 1e-11 * np.abs(var0).max()
            else:                            # tests/test_gpu_kstar_star.py: check_paths
                assert np.abs(out["mu"] - mu0).max() <= 1e-9 * np.abs(mu0).max()
                assert np.abs(out["var"] - var0).max() <= 1e-8 * mod.sf2
            sc = out["score"]
            assert out["best_idx"] == int(np.argmax(sc)) and out["best_val"] == sc[int(out["best_idx"])]
            if score == 2:
                assert np.array_equal(sc, out["var"])
            if score == 1 and not fp32:      # tests/test_gpu_parity.py: test_argmax_first_occurrence_and_scores
                want = orc.pointwise_ei(out["mu"], out["var"], 0.1)
                assert np.abs(sc - want).max() <= 1e-10 * max(1e-12, np.abs(want).max())
        return run, ref


SCORE_SLOTS = ("WS_KSTAR", "WS_PART", "WS_SMALL", "WS_KSTAR_GEO")
_predict_case("predict_mean_A130", "A", 0, 130, slots=SCORE_SLOTS)
_predict_case("predict_ei_A33", "A", 1, 33, slots=SCORE_SLOTS)
_predict_case("predict_var_A130", "A", 2, 130, slots=SCORE_SLOTS)
_predict_case("predict_ei_B130", "B", 1, 130, slots=SCORE_SLOTS + ("WS_PRUNE", "WS_PRUNE_KC"))
_predict_case("predict_var_B33", "B", 2, 33, slots=SCORE_SLOTS + ("WS_PRUNE", "WS_PRUNE_KC"))
_predict_case("predict_fp32_A130", "A", 1, 130, fp32=True, slots=SCORE_SLOTS)
for _s, _n in ((0, "mean"), (1, "ei"), (2, "var")):
    _predict_case(f"predict3_{_n}_A130", "A", _s, 130, env=dict(PPBO_FUSED=0), slots=SCORE_SLOTS)
_predict_case("predict3_ei_A2050", "A", 1, 2050, env=dict(PPBO_FUSED=0), slots=SCORE_SLOTS + ("WS_GPAD",), larger_M=4100)
_predict_case("predict3_var_B2050", "B", 2, 2050, env=dict(PPBO_FUSED=0), slots=SCORE_SLOTS + ("WS_GPAD", "WS_PRUNE", "WS_PRUNE_KC"),
              larger_M=4100)


@register("predict_record_A130", "predict", SCORE_SLOTS, model_dims("A", **M_SIZES), NAN_ROWS, legal=model_legal("A"))
def _():
    name = "predict_record_A130"

    def run(eng, v):
        mod = model("A", v)
        Xc = points(rng_of(name, v), mod, CASES[name].sizes(v)["M"], v)
        return outputs(record=eng.predict_record(mod.on(eng), Xc, score=1, mustar=0.1, index_offset=1000))

    def ref(out):
        mod = model("A", "checked")
        Xc = points(rng_of(name, "checked"), mod, 130, "checked")
        mu0, var0 = mod.mean_var(Xc)
        sc = orc.pointwise_ei(mu0, var0, 0.1)
        top = np.sort(sc)[-2:]
        assert top[1] - top[0] > 1e-9 * top[1], "a tied reference: another seed"
        assert out["record"][1] == 1000 + int(np.argmax(sc))
        assert abs(out["record"][0] - sc.max()) <= 1e-9 * sc.max()
    return run, ref


@register("predict_cov_A33", "predict", ("WS_KSTAR", "WS_PART"), model_dims("A", M=(33, 200, 1)),
          "finite but huge (1e300) alpha and G entries: the header documents no non-finite input for ppbo_predict_cov",
          legal=model_legal("A"))
def _():
    name = "predict_cov_A33"

    def run(eng, v):
        mod = model("A", v)
        Xc = points(rng_of(name, v), mod, CASES[name].sizes(v)["M"], "checked")
        post = mod.on(eng, alpha=mod.alpha * 1e300, G=mod.G * 1e300) if v == "nonfinite" else mod.on(eng)
        mu, cov = eng.predict_cov(post, Xc)
        return outputs(mu=mu, cov=cov)

    def ref(out):
        import pairs_numpy as pn
        mod = model("A", "checked")
        Xc = points(rng_of(name, "checked"), mod, 33, "checked")
        K = pn.cross(Xc, mod.X, mod.theta, mod.kernel)
        cov0 = orc.regularize_covariance(pn.cross(Xc, Xc, mod.theta, mod.kernel), orc.SHRINKAGE) - K @ mod.A @ K.T
        assert rel(out["mu"], K @ mod.alpha) < 1e-6                      # tests/test_gpu_parity.py: test_predict_cov_line_vs_reference
        assert np.abs(out["cov"] - cov0).max() <= 1e-6 * mod.sf2
    return run, ref


@register("search_batch_A130", "predictor", ("WS_TOURN_U", "WS_TOURN_FIELD", "WS_BATCH", "WS_BATCH_K", "WS_KSTAR", "WS_PART", "WS_SMALL"),
          model_dims("A", M=(130, 1000, 1), q=(4, 16, 1)),
          "include/ppbo_hip.h: 'A candidate with a non-finite coordinate has NaN mu, var and var_cond, is never picked'",
          legal=model_legal("A"))
def _():
    name = "search_batch_A130"

    def run(eng, v):
        mod = model("A", v)
        d = CASES[name].sizes(v)
        Xc = points(rng_of(name, v), mod, d["M"], v)
        o = eng.search_batch(mod.on(eng), Xc, d["q"], score=2, want_var_cond=True)
        return outputs(idx=o["idx"], score=o["score"], mu=o["mu"], var=o["var"], var_cond=o["var_cond"])

    def ref(out):
        import batch_numpy as bn
        mod = model("A", "checked")
        Xc = points(rng_of(name, "checked"), mod, 130, "checked")
        tau2 = float(mod.theta[0]) ** 2
        r = bn.greedy(Xc, *mod.args(), 4, bn.VARIANCE, 0.0, tau2)
        assert np.all(r["gap"] > 1e-6), "a tied reference: another seed"
        assert np.array_equal(out["idx"], r["idx"])
        e = dict(score=(np.abs(out["score"] - r["score"]) / np.maximum(np.abs(r["score"]), 1e-300)).max(),
                 var_cond=np.abs(out["var_cond"] - r["var_cond"]).max() / mod.sf2,
                 mu=np.abs(out["mu"] - r["mu"]).max() / mod.sf2, var=np.abs(out["var"] - r["var"]).max() / mod.sf2)
        assert all(x <= TOL for x in e.values()), e                       # tests/test_gpu_batch.py: _errors
    return run, ref


# ---- real edge-form posteriors: the projected contraction and the pruned search ------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted_design(n_q, m, D, kernel, l, sigma, seed):
    """(X, theta, Sigma^-1, f) on the host: a prior draw scaled by 1/2 (smooth_posterior / real_posterior of the tests of
    the projection and of the pruned search, with the host's factorizations in place of the device's)."""
    rng = np.random.default_rng(seed)
    X = star_rows(rng, n_q, m, D)
    th = [sigma, l, 1.3]
    S = orc.gram(X, th, kernel)
    f = 0.5 * np.linalg.cholesky(S) @ rng.standard_normal(X.shape[0])
    Sinv = orc.pd_inverse(S)
    P = orc.posterior_covariance(Sinv, f, m, sigma)
    A = orc.variance_operator(Sinv, P, False, lam=orc.lambda_dense(f, m, sigma))
    near = X[rng.integers(0, X.shape[0], 1500)] + 0.05 * rng.standard_normal((1500, D))
    pool = np.concatenate([near, rng.random((1500, D))])[rng.permutation(3000)]
    return dict(X=X, th=th, Sinv=Sinv, f=f, alpha=Sinv @ f, A=A, pool=pool, m=m, kernel=kernel)


# (n_q, m, D, kernel, l, sigma, seed): d20_96 / d20_384 of tests/test_gpu_prune.py, d2_416 / d2_384 of the projection's tests
FITTED = {
    "prune": dict(checked=(3, 31, 20, "SE_kernel", 0.45, 1.0, 11), larger=(12, 33, 24, "SE_kernel", 0.5, 1.0, 12),
                  smaller=(1, 1, 1, "SE_kernel", 0.45, 1.0, 13)),
    "proj": dict(checked=(16, 25, 2, "SE_kernel", 1.5, 0.1, 21), larger=(20, 31, 2, "SE_kernel", 1.5, 0.1, 22),
                 smaller=(1, 1, 1, "SE_kernel", 1.5, 0.1, 23)),
}


def fitted(key, variant):
    return fitted_design(*FITTED[key]["larger" if variant == "nonfinite" else variant])


def fitted_dims(key, M):
    """(the projection is taken on smooth designs in two dimensions only: D is no free dimension of its case)"""
    out = {}
    for i, v in enumerate(("checked", "larger", "smaller")):
        n_q, m, D = FITTED[key][v][:3]
        out[v] = dict(N=n_q * (m + 1), m=m, n_q=n_q, M=M[i], **(dict(D=D) if key != "proj" else {}))
    return out


def edge_posterior(eng, fd):
    return eng.posterior(fd["X"], fd["th"], fd["kernel"], eng.dev(fd["Sinv"]), fd["f"], fd["m"], form=FORM_EDGE)


def _prune_case(name, env):
    dims = fitted_dims("prune", (300, 2049, 1))

    @register(name, "predict", SCORE_SLOTS + ("WS_PRUNE", "WS_PRUNE_KC", "WS_LINALG", "WS_GPAD"), dims, NAN_ROWS, env,
              FITTED["prune"]["smaller"][:2] + (2,))
    def _():
        def inputs(v):
            fd = fitted("prune", v)
            Xc = fd["pool"][:dims["larger" if v == "nonfinite" else v]["M"]].copy()
            if v == "nonfinite":
                Xc[::7, 0] = np.nan
            mu = Xc[~np.isnan(Xc).any(axis=1)] if v == "nonfinite" else Xc
            K = orc.KERNELS[fd["kernel"]](fd["X"], mu, fd["th"])
            return fd, Xc, float(np.sort(K.T @ fd["alpha"])[-3:][0])

        def run(eng, v):
            fd, Xc, mustar = inputs(v)
            post = edge_posterior(eng, fd)
            rec = eng.predict_record(post, Xc, score=1, mustar=mustar, index_offset=1000)
            rep = eng.prune_report(post, Xc, 1, mustar)
            return outputs(record=rec, s_lo=rep["s_lo"], s_hi=rep["s_hi"], u2=rep["u2"], threshold=rep["threshold"],
                           n_surv=rep["n_surv"], pruned=rep["pruned"])

        def ref(out):
            fd, Xc, mustar = inputs("checked")
            mu0, var0 = orc.predict_mean_var(Xc, fd["X"], fd["th"], fd["alpha"], fd["A"], fd["kernel"])
            sc = orc.pointwise_ei(mu0, var0, mustar)
            assert out["pruned"] == 1 and out["n_surv"] <= 300 // 8      # tests/test_gpu_prune.py: test_few_survivors
            top = np.sort(sc)[-2:]
            assert top[1] - top[0] > 1e-5 * top[1], "a near-tied reference: another seed"
            assert out["record"][1] == 1000 + int(np.argmax(sc))
            assert abs(out["record"][0] - sc.max()) <= 1e-5 * sc.max()   # the score of a (mu, var) at the README's 1e-6
            ok = np.isfinite(sc)
            assert np.all(out["s_lo"][ok] <= sc[ok] * (1 + 1e-5) + 1e-12) and np.all(out["s_hi"][ok] >= sc[ok] * (1 - 1e-5) - 1e-12)
        return run, ref


_prune_case("prune_thin_300", dict(PPBO_FUSED=0, PPBO_PRUNE=1))
_prune_case("prune_tile_300", dict(PPBO_FUSED=0, PPBO_PRUNE=1, PPBO_PRUNE_THIN=0))


@register("projected_predict_416", "predict", SCORE_SLOTS + ("WS_PROJECT", "WS_PROJECT_SMALL", "WS_LINALG"),
          fitted_dims("proj", (130, 1000, 1)), NAN_ROWS, legal=FITTED["proj"]["smaller"][:2] + (2,))
def _():
    name = "projected_predict_416"

    def inputs(v):
        fd = fitted("proj", v)
        Xc = np.random.default_rng(5).random((CASES[name].sizes(v)["M"], fd["X"].shape[1]))
        if v == "nonfinite":
            Xc[::7, 0] = np.nan
        return fd, Xc

    def run(eng, v):
        fd, Xc = inputs(v)
        post = edge_posterior(eng, fd)
        pj = eng.project_variance(post, 1e-6)
        o = eng.predict(post, Xc, score=2, want_score=True, projection=pj)
        return outputs(T=pj.T, rows=pj.rows, bound=pj.bound, mu=o["mu"], var=o["var"], best_val=o["best_val"], best_idx=o["best_idx"])

    def ref(out):
        fd, Xc = inputs("checked")
        sf2 = fd["th"][2] ** 2
        mu0, var0 = orc.predict_mean_var(Xc, fd["X"], fd["th"], fd["alpha"], fd["A"], fd["kernel"])
        assert out["rows"] > 0 and 0.0 <= out["bound"] <= 1e-6 * sf2     # tests/test_gpu_var_projection.py: the projection is taken
        assert rel(out["mu"], mu0) < 1e-6
        d = var0 - out["var"]                                            # 0 <= var - var_projected <= bound, var to 1e-6 sf2
        assert d.min() >= -1e-6 * sf2 and d.max() <= out["bound"] + 1e-6 * sf2
        assert out["best_idx"] == int(np.argmax(out["var"])) and out["best_val"] == out["var"].max()
    return run, ref


# ============================================================ per-point predictors =======================================
def _two_set_case(name, entry, twin, key="A", M=130, slots=("WS_KSTAR", "WS_PART", "WS_SMALL", "WS_KSTAR_GEO"), doc=NAN_ROWS,
                  larger_M=1000):
    dims = model_dims(key, M=(M, larger_M, 1))

    @register(name, "predictor", slots, dims, doc, legal=model_legal(key))
    def _():
        def inputs(v):
            mod, rng = model(key, v), rng_of(name, v)
            n = dims["larger" if v == "nonfinite" else v]["M"]
            Xa = points(rng, mod, n, v)
            Xb = rng.random((n, mod.D)) if entry == "pairs" else rng.standard_normal((n, mod.D))
            return mod, Xa, Xb

        def run(eng, v):
            mod, Xa, Xb = inputs(v)
            fn = dict(pairs=eng.predict_pairs, slopes=eng.predict_slopes, curvatures=eng.predict_curvatures)[entry]
            o = fn(mod.on(eng), Xa, Xb, want_score=True)
            return outputs(mu=o["mu"], var=o["var"], prob=o["prob"], score=o["score"], best_val=o["best_val"], best_idx=o["best_idx"])

        def ref(out):
            mod, Xa, Xb = inputs("checked")
            twin(mod, Xa, Xb, out)
            p = out["prob"]
            assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()
        return run, ref


def _pairs_twin(mod, Xa, Xb, out):            # tests/test_gpu_pairs.py: _parity
    import pairs_numpy as pn
    from ppbo_amd.misc import preference_probability
    mu0, var0 = pn.pair_reference(Xa, Xb, *mod.args())
    p0 = preference_probability(mu0, var0, mod.theta[0])
    assert np.abs(out["mu"] - mu0).max() / np.abs(mu0).max() <= TOL
    assert np.abs(out["var"] - var0).max() / mod.sf2 <= TOL and np.abs(out["prob"] - p0).max() <= TOL


def _slopes_twin(mod, X, Xi, out):            # tests/test_gpu_slopes.py: _errors, _parity
    import slopes_numpy as sn
    mu0, var0, g = sn.slope_reference(X, Xi, *mod.args())
    assert np.max(np.abs(out["mu"] - mu0) / (np.abs(g) @ np.abs(mod.alpha))) <= TOL
    assert np.max(np.abs(out["var"] - var0) / sn.slope_prior(Xi, mod.theta, mod.kernel)) <= TOL
    assert np.abs(out["prob"] - sn.slope_probability(out["mu"], out["var"])).max() <= 4 * EPS


def _curv_twin(mod, X, Xi, out):              # tests/test_gpu_curvature.py: _errors, _parity
    import curvature_numpy as cn
    mu0, var0, c = cn.curvature_reference(X, Xi, *mod.args(), None)
    assert np.max(np.abs(out["mu"] - mu0) / (np.abs(c) @ np.abs(mod.alpha))) <= TOL
    assert np.max(np.abs(out["var"] - var0) / cn.curvature_prior(Xi, mod.theta, mod.kernel, None)) <= TOL
    assert np.abs(out["prob"] - cn.curvature_probability(out["mu"], out["var"])).max() <= 4 * EPS


_two_set_case("pairs_A130", "pairs", _pairs_twin)
_two_set_case("pairs_B2050", "pairs", _pairs_twin, key="B", M=2050, larger_M=4100,
              slots=("WS_KSTAR", "WS_PART", "WS_SMALL", "WS_KSTAR_GEO", "WS_GPAD"))
_two_set_case("slopes_A130", "slopes", _slopes_twin)
_two_set_case("curvatures_B33", "curvatures", _curv_twin, key="B", M=33)


@register("curvatures_acc_A130", "predictor", ("WS_KSTAR", "WS_PART", "WS_SMALL"), model_dims("A", **M_SIZES),
          "include/ppbo_hip.h: 'A row with a NaN or infinite coordinate in x, xi or acc gets NaN outputs'", legal=model_legal("A"))
def _():
    name = "curvatures_acc_A130"

    def inputs(v):
        mod, rng = model("A", v), rng_of(name, v)
        n = CASES[name].sizes(v)["M"]
        X, Xi, Xa = points(rng, mod, n, "checked"), rng.standard_normal((n, mod.D)), rng.standard_normal((n, mod.D))
        if v == "nonfinite":
            Xa[::5, 0] = np.nan
            Xi[2::11, -1] = np.inf
        return mod, X, Xi, Xa

    def run(eng, v):
        from ppbo_amd.engine import CURV_PROB, _ptr
        mod, X, Xi, Xa = inputs(v)
        post = mod.on(eng)                     # (alive until the outputs are on the host: md holds raw pointers)
        md = eng._model(post, True)
        dX, dXi, dXa = eng.dev(X), eng.dev(Xi), eng.dev(Xa)
        n = X.shape[0]
        mu, var, pr = eng.empty(n), eng.empty(n), eng.empty(n)
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        rc = eng.lib.ppbo_predict_curvatures(eng.ctx, C.byref(md), _ptr(dX), _ptr(dXi), _ptr(dXa), n, int(CURV_PROB), _ptr(mu),
                                             _ptr(var), _ptr(pr), None, C.byref(bv), C.byref(bi), eng._stream())
        eng._check(rc, "ppbo_predict_curvatures")
        return outputs(mu=mu, var=var, prob=pr, best_val=bv.value, best_idx=bi.value)

    def ref(out):                              # tests/test_gpu_curvature.py: _errors with Xa
        import curvature_numpy as cn
        mod, X, Xi, Xa = inputs("checked")
        mu0, var0, c = cn.curvature_reference(X, Xi, *mod.args(), Xa)
        assert np.max(np.abs(out["mu"] - mu0) / (np.abs(c) @ np.abs(mod.alpha))) <= TOL
        assert np.max(np.abs(out["var"] - var0) / cn.curvature_prior(Xi, mod.theta, mod.kernel, Xa)) <= TOL
        assert out["best_idx"] == int(np.argmax(out["prob"])) and out["best_val"] == out["prob"].max()
    return run, ref


@register("gradients_A130", "predictor", ("WS_KSTAR", "WS_PART", "WS_SMALL"), model_dims("A", M=(130, 1000, 1)),
          "include/ppbo_hip.h: 'A point with a NaN or infinite coordinate gets NaN in' its mean, covariance and score",
          legal=model_legal("A"))
def _():
    name = "gradients_A130"

    def inputs(v):
        mod = model("A", v)
        return mod, points(rng_of(name, v), mod, CASES[name].sizes(v)["M"], v)

    def run(eng, v):
        from ppbo_amd.engine import GRAD_NORM2
        mod, X = inputs(v)
        o = eng.predict_gradients(mod.on(eng), X, score=GRAD_NORM2, want_score=True)
        return outputs(mean=o["mean"], cov=o["cov"], score=o["score"], best_val=o["best_val"], best_idx=o["best_idx"])

    def ref(out):                              # tests/test_gpu_gradients.py: _parity
        import gradients_numpy as gn
        mod, X = inputs("checked")
        m0, C0, g = gn.gradient_reference(X, *mod.args())
        assert np.max(np.abs(out["mean"] - m0) / gn.mean_scale(g, mod.alpha)) <= TOL
        assert np.max(np.abs(out["cov"] - C0) / gn.cov_scale(mod.theta, mod.kernel, mod.D)) <= TOL
        assert np.array_equal(out["cov"], out["cov"].transpose(0, 2, 1))
        assert out["best_idx"] == int(np.argmax(out["score"])) and out["best_val"] == out["score"].max()
    return run, ref


@register("functionals_A130", "predictor", ("WS_KSTAR", "WS_PART", "WS_SMALL"), model_dims("A", M=(130, 1000, 1), G=(5, 16, 1)),
          "include/ppbo_hip.h: 'A group with a NaN or infinite coordinate gets NaN outputs'", legal=model_legal("A"))
def _():
    name = "functionals_A130"

    def inputs(v):
        mod, rng = model("A", v), rng_of(name, v)
        d = CASES[name].sizes(v)
        Xg = points(rng, mod, d["M"] * d["G"], v, per=37).reshape(d["M"], d["G"], mod.D)
        return mod, Xg, rng.standard_normal((d["M"], d["G"]))

    def run(eng, v):
        mod, Xg, w = inputs(v)
        o = eng.predict_functionals(mod.on(eng), Xg, w, threshold=0.05, want_score=True)
        return outputs(mu=o["mu"], var=o["var"], prob=o["prob"], score=o["score"], best_val=o["best_val"], best_idx=o["best_idx"])

    def ref(out):                              # tests/test_gpu_functionals.py: _errors
        import functionals_numpy as fn
        mod, Xg, w = inputs("checked")
        mu0, var0 = fn.functional_reference(Xg, w, *mod.args())
        p0 = fn.threshold_probability(mu0, var0, 0.05)
        scale = mod.sf2 * np.abs(w).sum(axis=1) ** 2
        assert np.abs(out["mu"] - mu0).max() / np.abs(mu0).max() <= TOL
        assert np.max(np.abs(out["var"] - var0) / scale) <= TOL and np.abs(out["prob"] - p0).max() <= TOL
        assert out["best_idx"] == int(np.argmax(out["prob"])) and out["best_val"] == out["prob"].max()
    return run, ref


def marginal_rows(rng, mod, M, effect, variant):
    """tests/test_gpu_marginals.py: _rows (orders 0, 1, 2 in turn; order 2 everywhere under INTERACTION)."""
    D = mod.D
    dims, t = np.full((M, 2), -1), rng.random((M, 2))
    order = np.full(M, 2) if effect == 2 else rng.integers(0, 3, M)
    if D == 1:
        order = np.minimum(order, 1)
    for i in range(M):
        if order[i] >= 1:
            dims[i, 0] = rng.integers(0, D)
        if order[i] == 2:
            dims[i, 1] = (dims[i, 0] + 1 + rng.integers(0, D - 1)) % D
    if variant == "nonfinite":
        t[::7, 0] = np.nan
    return dims, t


def _marginal_case(effect, label):
    name = f"marginals_{label}_A130"
    dims_ = model_dims("Am", M=(130, 1000, 1))

    @register(name, "predictor", ("WS_KSTAR", "WS_PART", "WS_SMALL", "WS_MARGINAL"), dims_,
              "include/ppbo_hip.h: 'a row with a NaN or infinite t on a kept axis gets NaN outputs'", legal=model_legal("Am"))
    def _():
        def inputs(v):
            mod = model("Am", v)
            return (mod,) + marginal_rows(rng_of(name, v), mod, CASES[name].sizes(v)["M"], effect, v)

        def run(eng, v):
            mod, dims, t = inputs(v)
            o = eng.predict_marginals(mod.on(eng), dims, t, effect=effect, want_score=True)
            return outputs(mu=o["mu"], var=o["var"], prob=o["prob"], score=o["score"], best_val=o["best_val"], best_idx=o["best_idx"])

        def ref(out):                          # tests/test_gpu_marginals.py: _errors
            import marginals_numpy as mn
            mod, dims, t = inputs("checked")
            mu0, var0, _ = mn.marginal_reference(dims, t, *mod.args(), effect)
            p0 = mn.sign_probability(mu0, var0)
            zero = (dims < 0).all(axis=1) & (effect == mn.CENTRED)
            assert np.all(out["mu"][zero] == 0.0) and np.all(out["var"][zero] == 0.0) and np.all(out["prob"][zero] == 0.5)
            assert np.abs(out["mu"] - mu0).max() / np.abs(mu0).max() <= TOL
            assert np.abs(out["var"] - var0).max() / mod.sf2 <= TOL and np.abs(out["prob"] - p0)[~zero].max() <= TOL
            assert out["best_idx"] == int(np.argmax(out["prob"])) and out["best_val"] == out["prob"].max()
        return run, ref


for _e, _l in ((0, "raw"), (1, "centred"), (2, "interaction")):
    _marginal_case(_e, _l)


def _tournament_case(kind, label):
    name = f"tournament_{label}_A130x3"

    @register(name, "predictor", ("WS_TOURN_U", "WS_TOURN_FIELD", "WS_TOURN_K", "WS_KSTAR", "WS_PART", "WS_SMALL"),
              model_dims("A", M=(130, 700, 1), Mb=(3, 40, 1)),
              "include/ppbo_hip.h: 'A non-finite coordinate in b_j gives NaN in column j and in EVERY row's score'",
              legal=model_legal("A"))
    def _():
        def inputs(v):
            mod, rng = model("A", v), rng_of(name, v)
            d = CASES[name].sizes(v)
            Xa, Xb = points(rng, mod, d["M"], v), points(rng, mod, d["Mb"], "checked")
            if v == "nonfinite":
                Xb[d["Mb"] // 2, 0] = np.nan
            return mod, Xa, Xb

        def run(eng, v):
            mod, Xa, Xb = inputs(v)
            o = eng.predict_tournament(mod.on(eng), Xa, Xb, score=kind, want_cov=True, want_prob=True)
            return outputs(**o)

        def ref(out):                          # tests/test_gpu_tournament.py: _parity
            import tournament_numpy as tn
            mod, Xa, Xb = inputs("checked")
            r = tn.tournament_reference(Xa, Xb, *mod.args())
            p0 = tn.win_matrix(r, mod.theta[0])
            mx = max(np.abs(r["mu_a"]).max(), np.abs(r["mu_b"]).max())
            e = dict(mu=max(np.abs(out["mu_a"] - r["mu_a"]).max(), np.abs(out["mu_b"] - r["mu_b"]).max()) / mx,
                     var=max(np.abs(out["var_a"] - r["var_a"]).max(), np.abs(out["var_b"] - r["var_b"]).max()) / mod.sf2,
                     cov=np.abs(out["cov"] - r["cov"]).max() / mod.sf2, p=np.abs(out["prob"] - p0).max(),
                     score=np.abs(out["score"] - tn.scores(p0, kind)).max())
            assert all(x <= TOL for x in e.values()), e
            assert out["best_idx"] == int(np.argmax(out["score"])) and out["best_val"] == out["score"].max()
        return run, ref


_tournament_case(0, "borda")
_tournament_case(1, "worst")


# ============================================================ lines ======================================================
LINE_DIMS = dict(B=(2, 7, 1), G=(17, 70, 1), S=(65, 1000, 1))
HUGE = "finite but huge (1e300) alpha and G entries: the header documents no non-finite input for this entry"


def line_inputs(name, v, key="A"):
    mod, rng = model(key, v), rng_of(name, v)
    d = CASES[name].sizes(v)
    B, G, S = d["B"], d["G"], d["S"]
    al = np.linspace(0.005, 0.995, G)
    xis, xs = np.zeros((B, mod.D)), rng.random((B, mod.D))
    for b in range(B):
        xis[b, b % mod.D] = 1.0
        xs[b, b % mod.D] = 0.0
    grid = np.stack([orc.line_grid(xis[b], xs[b], al) for b in range(B)])
    return mod, xis, xs, al, grid, rng.standard_normal((S, G)), rng.standard_normal((S, G))


def huge_post(mod, eng, v):
    return mod.on(eng, alpha=mod.alpha * 1e300, G=mod.G * 1e300) if v == "nonfinite" else mod.on(eng)


def _line_acq_case(name, xi):
    @register(name, "line", ("WS_KSTAR", "WS_SEARCH", "WS_PART", "WS_SMALL"), model_dims("A", **LINE_DIMS), HUGE, legal=model_legal("A"))
    def _():
        def run(eng, v):
            mod, xis, xs, al, grid, z, _ = line_inputs(name, v)
            post, jit = huge_post(mod, eng, v), 1e-9 * mod.sf2
            ei, vm = eng.line_acq_xi(post, xis, xs, al, z, 0.1, jitter=jit) if xi else eng.line_acq(post, grid, z, 0.1, jitter=jit)
            return outputs(ei=ei, varmax=vm)

        def ref(out):                          # tests/test_gpu_parity.py: test_line_acq_matches_oracle_with_same_draws
            import pairs_numpy as pn
            mod, xis, xs, al, grid, z, _ = line_inputs(name, "checked")
            jit = 1e-9 * mod.sf2
            for b in range(grid.shape[0]):
                K = pn.cross(grid[b], mod.X, mod.theta, mod.kernel)
                cov = orc.regularize_covariance(pn.cross(grid[b], grid[b], mod.theta, mod.kernel), orc.SHRINKAGE) - K @ mod.A @ K.T
                e0, v0 = orc.line_ei(K @ mod.alpha, cov, z, 0.1, jitter=jit), orc.line_varmax(K @ mod.alpha, cov, z, jitter=jit)
                assert abs(out["ei"][b] - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(mod.sf2))
                assert abs(out["varmax"][b] - v0) <= 1e-5 * max(abs(v0), 1e-6 * mod.sf2)
        return run, ref


_line_acq_case("line_acq_A", False)
_line_acq_case("line_acq_xi_A", True)


@register("line_choice_A", "line", ("WS_KSTAR", "WS_SEARCH", "WS_PART", "WS_SMALL"), model_dims("A", **LINE_DIMS),
          "include/ppbo_hip.h: 'in which the mean of any point is NaN (a point with a NaN coordinate'",
          legal=model_legal("A"))
def _():
    name = "line_choice_A"

    def run(eng, v):
        mod, xis, xs, al, grid, z, e = line_inputs(name, v)
        if v == "nonfinite":
            grid = grid.copy()
            grid[::2, 3, 0] = np.nan
        o = eng.line_choice(mod.on(eng), grid, z, e, jitter=1e-9 * mod.sf2, want_count=True, want_choice=True)
        return outputs(**o)

    def ref(out):                              # tests/test_gpu_line_choice.py: _check
        import choice_numpy as cn
        import pairs_numpy as pn
        mod, xis, xs, al, grid, z, e = line_inputs(name, "checked")
        B, G = grid.shape[:2]
        S = z.shape[0]
        ch, cnt, pr = out["choice"], out["count"], out["prob"]
        assert ch.min() >= 0 and ch.max() < G and np.array_equal(pr, cnt / S)
        tol, close_n = 1e-6 * float(mod.theta[2]), 0
        for b in range(B):
            assert np.array_equal(cnt[b], np.bincount(ch[b], minlength=G))
            K = pn.cross(grid[b], mod.X, mod.theta, mod.kernel)
            cov = orc.regularize_covariance(pn.cross(grid[b], grid[b], mod.theta, mod.kernel), orc.SHRINKAGE) - K @ mod.A @ K.T
            u = cn.utilities(K @ mod.alpha, cov, z, e, float(mod.theta[0]), 1e-9 * mod.sf2)
            close = cn.top_two_gap(u) <= tol
            close_n += int(close.sum())
            assert np.all(u.max(axis=1) - u[np.arange(S), ch[b]] <= tol)
            assert np.array_equal(ch[b][~close], u.argmax(axis=1)[~close])
        assert close_n <= max(1, 0.002 * S * B), "near-tied reference draws: another seed"
    return run, ref


# ============================================================ mean searches ==============================================
SEARCH_DIMS = dict(M=(130, 1000, 1), K=(4, 16, 1), T=(2, 5, 1))
NAN_POOL = "include/ppbo_hip.h: 'NaN never wins, and a group whose rows are all NaN or -inf yields no survivor'"


def mean_post(mod, eng, v):
    return eng.mean_posterior(mod.X, mod.theta, mod.kernel, mod.m, eng.dev(mod.alpha * (1e300 if v == "nonfinite" else 1.0)))


def mean_is_there(mod, x, mu):
    """tests/test_gpu_mean_search.py: 'the value IS the mean there', inside the box."""
    mu1, _ = orc.mean_grad(x, mod.X, mod.theta, mod.alpha, mod.kernel)
    assert np.all((x >= 0) & (x <= 1))
    assert np.abs(mu1 - mu).max() <= 1e-9 * np.abs(mu1).max() + 1e-14


@register("mean_grad_A", "search", (), model_dims("A", **SEARCH_DIMS), HUGE, legal=model_legal("A"))
def _():
    name = "mean_grad_A"

    def run(eng, v):
        mod = model("A", v)
        mu, g = eng.mean_grad(mean_post(mod, eng, v), points(rng_of(name, v), mod, CASES[name].sizes(v)["M"], "checked"))
        return outputs(mu=mu, grad=g)

    def ref(out):                              # tests/test_gpu_parity.py: test_mean_grad_vs_oracle
        mod = model("A", "checked")
        mu0, g0 = orc.mean_grad(points(rng_of(name, "checked"), mod, 130, "checked"), mod.X, mod.theta, mod.alpha, mod.kernel)
        assert rel(out["mu"], mu0) < 1e-9 and np.abs(out["grad"] - g0).max() <= 1e-9 * np.abs(g0).max()
    return run, ref


@register("mean_ascent_A", "search", ("WS_TRANSPOSE",), model_dims("A", **SEARCH_DIMS), HUGE, legal=model_legal("A"))
def _():
    name = "mean_ascent_A"

    def run(eng, v):
        mod = model("A", v)
        x, mu, it = eng.mean_ascent(mean_post(mod, eng, v), rng_of(name, v).random((CASES[name].sizes(v)["K"], mod.D)), iters=10, tol=1e-9)
        return outputs(x=x, mu=mu, it=it)

    def ref(out):
        mean_is_there(model("A", "checked"), out["x"], out["mu"])
        assert np.all(out["it"] <= 10)
    return run, ref


def _multi_case(name, fp32):
    @register(name, "search", ("WS_SEARCH", "WS_SEARCH_SMALL", "WS_SEARCH_ROWS", "WS_PART", "WS_TRANSPOSE"),
              model_dims("A", **SEARCH_DIMS), NAN_POOL, legal=model_legal("A"))
    def _():
        def inputs(v):
            mod, rng = model("A", v), rng_of(name, v)
            d = CASES[name].sizes(v)
            pool, shifts, xprev = rng.random((d["M"], mod.D)), rng.random((d["T"], mod.D)), rng.random(mod.D)
            if v == "nonfinite":
                pool[::7, 0] = np.nan
            return mod, d, pool, shifts, xprev

        def run(eng, v):
            mod, d, pool, shifts, xprev = inputs(v)
            x, mu = eng.mean_search_multi(mean_post(mod, eng, "checked"), pool, shifts, extra="design", xprev=xprev, K=d["K"],
                                          sep=0.05, iters=10, tol=1e-9, screen_fp32=fp32)
            return outputs(x=x, mu=mu)

        def ref(out):                          # tests/test_gpu_mean_search.py: the multi-trial search
            import search_ref as sr
            mod, d, pool, shifts, xprev = inputs("checked")
            for t in range(d["T"]):
                ok = np.isfinite(out["mu"][t])
                assert ok.any() and np.all(out["mu"][t][~ok] == -np.inf) and np.all(ok[:ok.sum()])
                mean_is_there(mod, out["x"][t][ok], out["mu"][t][ok])
                rows, n = sr.trial_rows(pool, shifts, t, mod.X, xprev)
                mu_c, _ = orc.mean_grad(rows[:n], mod.X, mod.theta, mod.alpha, mod.kernel)
                assert out["mu"][t][ok].max() >= mu_c.max() - (1e-5 if fp32 else 1e-12) * max(1.0, np.abs(mu_c).max())
        return run, ref


_multi_case("mean_search_multi_fp32_A", True)
_multi_case("mean_search_multi_fp64_A", False)


def box_of(rng, T, D):
    lo = rng.uniform(0.0, 0.4, (T, D))
    return np.stack([lo, lo + rng.uniform(0.2, 0.6, (T, D))], axis=1)


@register("mean_ascent_boxes_A", "search", ("WS_TRANSPOSE", "WS_BOX"), model_dims("A", **SEARCH_DIMS), HUGE,
          legal=model_legal("A"))
def _():
    name = "mean_ascent_boxes_A"

    def inputs(v):
        mod, rng = model("A", v), rng_of(name, v)
        K = CASES[name].sizes(v)["K"]
        return mod, rng.random((K, mod.D)), box_of(rng, K, mod.D)

    def run(eng, v):
        mod, starts, boxes = inputs(v)
        x, mu, it = eng.mean_ascent_boxes(mean_post(mod, eng, v), starts, boxes, per_box=1, iters=10, tol=1e-9)
        return outputs(x=x, mu=mu, it=it)

    def ref(out):                              # tests/test_gpu_box_search.py: inside the box, the value is the mean there
        mod, starts, boxes = inputs("checked")
        mean_is_there(mod, out["x"], out["mu"])
        assert np.all(out["x"] >= boxes[:, 0]) and np.all(out["x"] <= boxes[:, 1])
        mu0, _ = orc.mean_grad(np.clip(starts, boxes[:, 0], boxes[:, 1]), mod.X, mod.theta, mod.alpha, mod.kernel)
        assert np.all(out["mu"] >= mu0 - 1e-12 * np.abs(mu0).max())      # the monotone safeguard
    return run, ref


@register("mean_search_boxes_A", "search", ("WS_SEARCH", "WS_SEARCH_ROWS", "WS_PART", "WS_TRANSPOSE", "WS_BOX", "WS_BOX_SURV"),
          model_dims("A", **SEARCH_DIMS), NAN_POOL, legal=model_legal("A"))
def _():
    name = "mean_search_boxes_A"

    def inputs(v):
        mod, rng = model("A", v), rng_of(name, v)
        d = CASES[name].sizes(v)
        pool, boxes, shifts = rng.random((d["M"], mod.D)), box_of(rng, d["T"], mod.D), rng.random((d["T"], mod.D))
        if v == "nonfinite":
            pool[::7, 0] = np.nan
        return mod, d, pool, boxes, shifts

    def run(eng, v):
        mod, d, pool, boxes, shifts = inputs(v)
        x, mu, cnt = eng.mean_search_boxes(mean_post(mod, eng, "checked"), pool, boxes, shifts=shifts, K=d["K"], sep=0.05, iters=10,
                                           tol=1e-9, screen_fp32=False)
        return outputs(x=x, mu=mu, count=cnt)

    def ref(out):                              # tests/test_gpu_box_search.py; rows: box_search_numpy.box_rows
        import box_search_numpy as bs
        mod, d, pool, boxes, shifts = inputs("checked")
        for t in range(d["T"]):
            n = int(out["count"][t])
            assert 1 <= n <= d["K"] and np.all(out["mu"][t][n:] == -np.inf)
            x = out["x"][t][:n]
            mean_is_there(mod, x, out["mu"][t][:n])
            assert np.all(x >= boxes[t, 0]) and np.all(x <= boxes[t, 1])
            rows = bs.box_rows(pool, shifts[t], boxes[t, 0], boxes[t, 1])
            mu_c, _ = orc.mean_grad(rows, mod.X, mod.theta, mod.alpha, mod.kernel)
            assert out["mu"][t][:n].max() >= mu_c.max() - 1e-12 * max(1.0, np.abs(mu_c).max())
    return run, ref


# ============================================================ RFF and paths ==============================================
RFF_DIMS = dict(checked=dict(F=70, S=2, M=130, N=78, D=3, K=4), larger=dict(F=300, S=5, M=1000, N=216, D=7, K=16),
                smaller=dict(F=1, S=1, M=1, N=2, D=1, K=1))
HUGE_W = "finite but huge (1e300) weights: the header documents no non-finite input for this entry"


def rff_inputs(name, v):
    d, rng = CASES[name].sizes(v), rng_of(name, v)
    D, F = d["D"], d["F"]
    r = dict(d=d, X=rng.random((d["N"], D)), cand=rng.random((d["M"], D)), W=rng.standard_normal((F, D)) / 0.5,
             b=rng.uniform(0, 2 * np.pi, F), om=rng.standard_normal(F), oms=rng.standard_normal((d["S"], F)),
             V=rng.standard_normal((d["S"], d["N"])))
    if v == "nonfinite":
        r["om"], r["oms"], r["V"] = r["om"] * 1e300, r["oms"] * 1e300, r["V"] * 1e300
    return r


def _rff_case(name, slots, doc, family="rff"):
    def deco(pair):
        return register(name, family, slots, RFF_DIMS, doc)(pair)
    return deco


@_rff_case("rff_project", (), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("rff_project", v)
        return outputs(Phi=eng.rff_project(r["X"], r["W"], r["b"], 1e150 if v == "nonfinite" else 0.7))

    def ref(out):                              # tests/test_gpu_parity.py: rff_project against orc.rff_features
        r = rff_inputs("rff_project", "checked")
        assert np.abs(out["Phi"] - orc.rff_features(r["X"], r["W"], r["b"], 0.7)).max() <= 1e-12
    return run, ref


@_rff_case("rff_score", ("WS_PART", "WS_SMALL"), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("rff_score", v)
        sc, bv, bi = eng.rff_score(r["cand"], r["W"], r["b"], 0.7, r["om"])
        return outputs(score=sc, best_val=bv, best_idx=bi)

    def ref(out):                              # tests/test_gpu_parity.py: test_rff_vs_reference
        r = rff_inputs("rff_score", "checked")
        assert rel(out["score"], orc.rff_score(r["cand"], r["W"], r["b"], 0.7, r["om"])) < 1e-9
        assert out["best_idx"] == int(np.argmax(out["score"])) and out["best_val"] == out["score"].max()
    return run, ref


@_rff_case("rff_score_multi", (), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("rff_score_multi", v)
        return outputs(score=eng.rff_score_multi(r["cand"], r["W"], r["b"], 0.7, r["oms"]))

    def ref(out):
        r = rff_inputs("rff_score_multi", "checked")
        want = np.stack([orc.rff_score(r["cand"], r["W"], r["b"], 0.7, o) for o in r["oms"]])
        assert rel(out["score"], want) < 1e-9
    return run, ref


def rff_maxima(r, x, vals, om):
    """tests/test_gpu_mean_search.py: the RFF search (inside the box, the value is the sample there, no worse than the raw rows)."""
    assert 1 <= len(vals) and np.all((x >= 0) & (x <= 1))
    assert np.abs(orc.rff_score(x, r["W"], r["b"], 0.7, om) - vals).max() <= 1e-9 * np.abs(vals).max() + 1e-13
    assert vals.max() >= orc.rff_score(r["cand"], r["W"], r["b"], 0.7, om).max() - 1e-12


@_rff_case("rff_search", ("WS_SEARCH", "WS_TRANSPOSE", "WS_PART"), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("rff_search", v)
        x, vals = eng.rff_search(r["cand"], r["W"], r["b"], 0.7, r["om"], K=r["d"]["K"], sep=0.05, iters=10, tol=1e-10)
        return outputs(x=x, values=vals, found=len(vals))

    def ref(out):
        r = rff_inputs("rff_search", "checked")
        rff_maxima(r, out["x"], out["values"], r["om"])
    return run, ref


@_rff_case("rff_search_multi", ("WS_SEARCH", "WS_TRANSPOSE", "WS_PART"), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("rff_search_multi", v)
        x, vals, found = eng.rff_search_multi(r["cand"], r["W"], r["b"], 0.7, r["oms"], K=r["d"]["K"], sep=0.05, iters=10, tol=1e-10)
        return outputs(x=x, values=vals, found=found)

    def ref(out):
        r = rff_inputs("rff_search_multi", "checked")
        for s in range(r["d"]["S"]):
            n = int(out["found"][s])
            assert np.all(out["values"][s][n:] == -np.inf)
            rff_maxima(r, out["x"][s][:n], out["values"][s][:n], r["oms"][s])
    return run, ref


@_rff_case("rff_omega_map", ("WS_SEARCH_SMALL", "WS_VEC"), HUGE_W)
def _():
    def inputs(v):
        d, rng = CASES["rff_omega_map"].sizes(v), rng_of("rff_omega_map", v)
        n_q, m = (3, 25) if v == "checked" else ((8, 26) if v != "smaller" else (1, 1))
        Phi = rng.standard_normal((d["F"], n_q * (m + 1))) * 0.3
        return Phi, rng.standard_normal(d["F"]) * (1e300 if v == "nonfinite" else 1.0), m

    def run(eng, v):
        Phi, w0, m = inputs(v)
        om, S, gn, it = eng.rff_omega_map(Phi, w0, m, 0.3, maxiter=500, gtol=1e-6)
        return outputs(omega=om, S=S, gradnorm=gn, iterations=it)

    def ref(out):                              # tests/test_gpu_compat.py: the maximiser against orc.rff_terms
        Phi, w0, m = inputs("checked")
        S1, g1, h1 = orc.rff_terms(Phi, out["omega"], m, 0.3)
        assert out["gradnorm"] < 1e-6 and 0 < out["iterations"] < 500
        assert abs(S1 - out["S"]) <= 1e-12 * max(1.0, abs(out["S"])) and np.linalg.norm(g1) < 1e-6 and np.all(h1 < 0)
    return run, ref


PATH_TH = (0.1, 0.5, 0.7)


@_rff_case("path_score_multi", (), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("path_score_multi", v)
        kern = "SE_kernel" if v in ("checked", "smaller") else "RQ_kernel"
        return outputs(score=eng.path_score_multi(r["cand"], r["W"], r["b"], PATH_TH, kern, r["X"], r["oms"], r["V"]))

    def ref(out):                              # tests/test_gpu_pathwise.py: err / scale <= 1e-12
        import pathwise_numpy as pw
        r = rff_inputs("path_score_multi", "checked")
        want = pw.paths(r["cand"], r["oms"], r["V"], r["W"], r["b"], r["X"], PATH_TH, "SE_kernel")
        scale = pw.paths_abs(r["cand"], r["oms"], r["V"], r["W"], r["b"], r["X"], PATH_TH, "SE_kernel").max(axis=1)
        assert np.all(np.abs(out["score"] - want).max(axis=1) <= 1e-12 * scale)
    return run, ref


@_rff_case("path_search_multi", ("WS_SEARCH", "WS_TRANSPOSE", "WS_PART"), HUGE_W)
def _():
    def run(eng, v):
        r = rff_inputs("path_search_multi", v)
        kern = "SE_kernel" if v in ("checked", "smaller") else "RQ_kernel"
        x, vals, found = eng.path_search_multi(r["cand"], r["W"], r["b"], PATH_TH, kern, r["X"], r["oms"], r["V"], K=r["d"]["K"],
                                               sep=0.05, iters=10, tol=1e-10)
        return outputs(x=x, values=vals, found=found)

    def ref(out):                              # tests/test_gpu_pathwise.py: the value is the path there
        import pathwise_numpy as pw
        r = rff_inputs("path_search_multi", "checked")
        for s in range(r["d"]["S"]):
            n = int(out["found"][s])
            assert n >= 1 and np.all(out["values"][s][n:] == -np.inf)
            x, vals = out["x"][s][:n], out["values"][s][:n]
            assert np.all((x >= 0) & (x <= 1))
            want = pw.paths(x, r["oms"][s], r["V"][s], r["W"], r["b"], r["X"], PATH_TH, "SE_kernel")[0]
            scale = pw.paths_abs(x, r["oms"][s], r["V"][s], r["W"], r["b"], r["X"], PATH_TH, "SE_kernel")[0]
            assert np.all(np.abs(want - vals) <= 1e-12 * scale)
    return run, ref


# ============================================================ points =====================================================
POINT_DIMS = dict(checked=dict(P=130 * 6), larger=dict(P=1000 * 6), smaller=dict(P=6))
CAM_L = np.array([0.3, 0.4, 0.5, 0.6, 0.8, 1.0])
HUGE_X = "finite but huge (1e300) coordinates: the header documents no non-finite input for this entry"


def point_rows(name, v):
    X = rng_of(name, v).random((CASES[name].sizes(v)["P"] // 6, 6))
    return X * 1e300 if v == "nonfinite" else X


@register("scale_points", "points", ("WS_SCALE_PTS",), POINT_DIMS, HUGE_X)
def _():
    def run(eng, v):
        return outputs(out=eng.scale_points(point_rows("scale_points", v), 1.0 / CAM_L))

    def ref(out):
        assert np.array_equal(out["out"], point_rows("scale_points", "checked") * (1.0 / CAM_L))
    return run, ref


@register("shift_points", "points", ("WS_SEARCH_SMALL",), POINT_DIMS, HUGE_X)
def _():
    def run(eng, v):
        return outputs(out=eng.shift_points(point_rows("shift_points", v), CAM_L))

    def ref(out):                              # tests/test_gpu_mean_search.py: frac(P + shift), exactly
        P = point_rows("shift_points", "checked") + CAM_L
        assert np.array_equal(out["out"], P - np.floor(P))
    return run, ref


@register("camphor_embed", "points", (), POINT_DIMS, HUGE_X)
def _():
    def run(eng, v):
        return outputs(out=eng.camphor_embed(point_rows("camphor_embed", v), CAM_L))

    def ref(out):                              # tests/search_ref.py: camphor_embed, to a few ulp of the unit circle
        import search_ref as sr
        want = np.stack([sr.camphor_embed(x, CAM_L)[0] for x in point_rows("camphor_embed", "checked")])
        assert np.abs(out["out"] - want).max() <= 1e-12 * np.abs(want).max()
    return run, ref


@register("camphor_line_points", "points", (), dict(checked=dict(P=2 * 17 * 6, B=2, G=17), larger=dict(P=7 * 70 * 6, B=7, G=70),
                                                     smaller=dict(P=6, B=1, G=1)), HUGE_X)
def _():
    name = "camphor_line_points"

    def inputs(v):
        d, rng = CASES[name].sizes(v), rng_of(name, v)
        s = 1e300 if v == "nonfinite" else 1.0
        return rng.standard_normal((d["B"], 6)), rng.random((d["B"], 6)) * s, np.linspace(0.0, 1.0, d["G"])

    def run(eng, v):
        from ppbo_amd.engine import _ptr
        xis, xs, al = inputs(v)
        B, G = xis.shape[0], al.size
        dxi, dx, dal, grid = eng.dev(xis), eng.dev(xs), eng.dev(al), eng.empty(B, G, 11)
        rc = eng.lib.ppbo_camphor_line_points(eng.ctx, _ptr(dxi), _ptr(dx), _ptr(dal), 0, B, G, eng._dptr(CAM_L), _ptr(grid), eng._stream())
        eng._check(rc, "ppbo_camphor_line_points")
        return outputs(grid=grid)

    def ref(out):
        import search_ref as sr
        xis, xs, al = inputs("checked")
        want = np.stack([[sr.camphor_embed(a * xis[b] + xs[b], CAM_L)[0] for a in al] for b in range(xis.shape[0])])
        assert np.abs(out["grid"] - want).max() <= 1e-12 * np.abs(want).max()
    return run, ref


# ============================================================ dense ======================================================
def spd(rng, N):
    Q = rng.standard_normal((N, N))
    return Q @ Q.T + N * np.eye(N)


def dense_dims(N, **extra):
    return dict(checked=dict(N=N, **{k: v[0] for k, v in extra.items()}), larger=dict(N=650, **{k: v[1] for k, v in extra.items()}),
                smaller=dict(N=1, **{k: v[2] for k, v in extra.items()}))


NOT_PD = "include/ppbo_hip.h: PPBO_ERR_NOT_PD; tests/test_gpu_parity.py::test_potrf_failure_column_is_lapacks sends a NaN pivot"
HUGE_M = "finite but huge (1e300) entries: the header documents no non-finite input for this entry"


def design(name, v, sizes=((5, 12, 3), (25, 25, 7), (1, 1, 1))):
    n_q, m, D = sizes[("checked", "larger", "smaller").index("larger" if v == "nonfinite" else v)]
    return orc.synthetic_design(n_q, D, m=m, seed=zlib.crc32(name.encode()) % 1000 + (v != "checked")), m


def _gram_case(name, sizes, N):
    dims = {v: dict(N=s[0] * (s[1] + 1), D=s[2]) for v, s in zip(("checked", "larger", "smaller"), sizes)}

    @register(name, "dense", (), dims, HUGE_X, legal=(sizes[2][0], sizes[2][1], sizes[2][0] * (sizes[2][1] + 1)))
    def _():
        def run(eng, v):
            X, _ = design(name, v, sizes)
            kern = "SE_kernel" if v in ("checked", "smaller") else "RQ_kernel"
            return outputs(Sigma=eng.gram(X * (1e300 if v == "nonfinite" else 1.0), [0.1, 0.4, 1.3], kern))

        def ref(out):                          # tests/test_gpu_parity.py: test_gram_odd_sizes
            X, _ = design(name, "checked", sizes)
            assert X.shape[0] == N and rel(out["Sigma"], orc.gram(X, [0.1, 0.4, 1.3], "SE_kernel")) < 1e-12
            assert np.array_equal(out["Sigma"], out["Sigma"].T)
        return run, ref


_gram_case("gram_65", ((5, 12, 3), (25, 25, 7), (1, 1, 1)), 65)
_gram_case("gram_129", ((3, 42, 6), (25, 25, 21), (1, 1, 1)), 129)


@register("cross_cov_65x129", "dense", (), dict(checked=dict(N=65, M=129, D=3), larger=dict(N=650, M=700, D=7), smaller=dict(N=1, M=1, D=1)),
          HUGE_X)
def _():
    name = "cross_cov_65x129"

    def inputs(v):
        d, rng = CASES[name].sizes(v), rng_of(name, v)
        s = 1e300 if v == "nonfinite" else 1.0
        return rng.random((d["N"], d["D"])) * s, rng.random((d["M"], d["D"]))

    def run(eng, v):
        X1, X2 = inputs(v)
        return outputs(K=eng.cross_cov(X1, X2, [0.05, 0.31, 0.7], "SE_kernel" if v in ("checked", "smaller") else "RQ_kernel"))

    def ref(out):                              # tests/test_gpu_parity.py: test_cross_cov_ragged
        X1, X2 = inputs("checked")
        assert rel(out["K"], orc.cross_cov(X1, X2, [0.05, 0.31, 0.7], "SE_kernel")) < 1e-12
    return run, ref


@register("regularize_covariance_65", "dense", ("WS_VEC",), dense_dims(65), HUGE_M)
def _():
    name = "regularize_covariance_65"

    def inputs(v):
        N, rng = CASES[name].sizes(v)["N"], rng_of(name, v)
        K = spd(rng, N) / N
        K[N // 2, N // 2] = -0.5
        return K * (1e300 if v == "nonfinite" else 1.0)

    def run(eng, v):
        return outputs(K=eng.regularize_covariance(inputs(v), 1e-4))

    def ref(out):                              # tests/test_gpu_compat.py: <= 1e-13 max|K|
        K = inputs("checked")
        assert np.abs(out["K"] - orc.regularize_covariance(K, 1e-4)).max() <= 1e-13 * np.abs(K).max()
    return run, ref


def bad_matrix(A, v):
    """Non-finite history: a NaN pivot two thirds down (the factor left of it is written, NaN right of it)."""
    if v == "nonfinite":
        A = A.copy()
        k = 2 * A.shape[0] // 3
        A[k, k] = np.nan
    return A


@register("potrf_129", "dense", ("WS_POTRF", "WS_SMALL"), dense_dims(129), NOT_PD)
def _():
    def run(eng, v):
        A = bad_matrix(spd(rng_of("potrf_129", v), CASES["potrf_129"].sizes(v)["N"]), v)
        return outputs(L=eng.potrf_(eng.dev(A)))

    def ref(out):                              # tests/test_gpu_parity.py: test_potrf_and_inverse
        assert rel(np.tril(out["L"]), np.linalg.cholesky(spd(rng_of("potrf_129", "checked"), 129))) < 1e-12
    return run, ref


def _inverse_case(name, method, N):
    @register(name, "dense", ("WS_LINALG", "WS_LINALG2", "WS_POTRF", "WS_SMALL"), dense_dims(N), NOT_PD)
    def _():
        def run(eng, v):
            A = bad_matrix(spd(rng_of(name, v), CASES[name].sizes(v)["N"]), v)
            r = getattr(eng, method)(A)
            r = r if isinstance(r, tuple) else (r,)
            return outputs(**{k: t for k, t in zip(("Ainv", "second", "third"), r)})

        def ref(out):                          # tests/test_gpu_parity.py: test_potrf_and_inverse, the factors3 test
            A = spd(rng_of(name, "checked"), N)
            Ai, L0 = out["Ainv"], np.linalg.cholesky(A)
            assert np.abs(Ai @ A - np.eye(N)).max() < 1e-10 and np.abs(Ai - Ai.T).max() <= 1e-12 * np.abs(Ai).max()
            if method == "pd_inverse_chol":
                assert rel(np.tril(out["second"]), L0) < 1e-12
            if method == "pd_inverse_factors3":
                assert rel(np.tril(out["third"]), L0) < 1e-12
                Li = out["second"]
                assert np.all(np.triu(Li, 1) == 0.0), "the full triangular inverse: zeros above the diagonal"
                assert np.abs(Li @ L0 - np.eye(N)).max() < 1e-10
        return run, ref


_inverse_case("pd_inverse_65", "pd_inverse", 65)
_inverse_case("pd_inverse_chol_129", "pd_inverse_chol", 129)
_inverse_case("pd_inverse_factors3_65", "pd_inverse_factors3", 65)


APPEND_DIMS = dense_dims(65, k=(13, 26, 1))
APPEND_DIMS["smaller"]["N"] = 2


@register("pd_inverse_append_65", "dense", ("WS_APPEND", "WS_SMALL"), APPEND_DIMS, NOT_PD)
def _():
    name = "pd_inverse_append_65"

    def inputs(v):
        d = CASES[name].sizes(v)
        N = d["N"]
        A = spd(rng_of(name, v), N)
        N1 = N - d["k"]
        L1 = np.linalg.cholesky(A[:N1, :N1])
        Li1 = np.linalg.inv(L1)
        if v == "nonfinite":
            A = A.copy()
            A[N - 1, N - 1] = -1.0            # an indefinite border: tests/test_gpu_incremental.py::test_append_reports_indefinite_border
        return A, Li1.T @ Li1, Li1, L1

    def run(eng, v):
        A, Ai1, Li1, L1 = inputs(v)
        Ai, Li, L = eng.pd_inverse_append(A, Ai1, Li1, L1)
        return outputs(Ainv=Ai, Linv=Li, L=L)

    def ref(out):                              # tests/test_gpu_incremental.py
        A = inputs("checked")[0]
        want, L0 = np.linalg.inv(A), np.linalg.cholesky(A)
        assert np.abs(out["Ainv"] - want).max() <= 1e-9 * np.abs(want).max()
        assert np.abs(np.tril(out["L"]) - L0).max() <= 1e-10 * np.abs(L0).max()
    return run, ref


@register("dgemm_65x129x33", "dense", (), dict(checked=dict(N=65, M=129, K=33), larger=dict(N=650, M=700, K=300),
                                               smaller=dict(N=1, M=1, K=1)), HUGE_M)
def _():
    name = "dgemm_65x129x33"

    def inputs(v):
        d, rng = CASES[name].sizes(v), rng_of(name, v)
        s = 1e300 if v == "nonfinite" else 1.0
        return rng.standard_normal((d["K"], d["N"])) * s, rng.standard_normal((d["M"], d["K"])) * s, rng.standard_normal((d["N"], d["M"]))

    def run(eng, v):
        A, B, C0 = inputs(v)
        return outputs(C=eng.dgemm(A, B, True, True, alpha=1.5, beta=-0.5, C_out=eng.dev(C0.copy())))

    def ref(out):                              # tests/test_gpu_parity.py: test_dgemm
        A, B, C0 = inputs("checked")
        assert rel(out["C"], 1.5 * A.T @ B.T - 0.5 * C0) < 1e-13
    return run, ref


@register("dgemv_129", "dense", ("WS_VEC",), dense_dims(129), HUGE_M)
def _():
    name = "dgemv_129"

    def inputs(v):
        N, rng = CASES[name].sizes(v)["N"], rng_of(name, v)
        return rng.standard_normal((N, N)) * (1e300 if v == "nonfinite" else 1.0), rng.standard_normal(N)

    def run(eng, v):
        A, x = inputs(v)
        return outputs(y=eng.dgemv(A, x, trans=True, lower=True), y2=eng.dgemv(A, x))

    def ref(out):                              # tests/test_gpu_parity.py: test_dgemv
        A, x = inputs("checked")
        for y, want in ((out["y"], np.tril(A).T @ x), (out["y2"], A @ x)):
            assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) * np.sqrt(129)
    return run, ref


def _lu_case(N):
    name = f"lu_slogdet_{N}"

    @register(name, "lu", ("WS_VEC",), dense_dims(N), HUGE_M)
    def _():
        def inputs(v):
            import lu_ref as lr
            n = CASES[name].sizes(v)["N"]
            A = lr.scaled_gaussian(n, n + (v != "checked"))
            return A * 1e300 if v == "nonfinite" else A

        def run(eng, v):
            d = eng.dev(inputs(v))
            sg, ld, info = eng.lu_slogdet_(d)
            return outputs(packed=d, sign=sg, logdet=ld, info=info)

        def ref(out):                          # tests/test_gpu_lu.py: test_pivot_sequence_and_backward_error
            import lu_ref as lr
            import scipy.linalg
            A = inputs("checked")
            lu, piv = scipy.linalg.lu_factor(A)
            piv = piv.astype(np.int64)
            assert lr.pivot_gap(lu) >= 1e-8
            assert out["info"] == 0 and np.array_equal(lr.recover_rows(A, out["packed"]), lr.perm_of(piv))
            assert lr.backward_ratio(A, out["packed"], piv, lr.sample_rows(N)) <= 1.0
            s_ref, ld_ref = lr.u_slogdet(lu)
            assert out["sign"] == s_ref and abs(out["logdet"] - ld_ref) <= 2.0 * lr.logdet_bound(A, lu, piv)
        return run, ref


_lu_case(33)
_lu_case(257)


def laplace_state(name, v, sizes):
    """(X, theta, m, Sigma, Sigma^-1, f, lam_diag, lam_off) on the host: f a Newton-converged f_MAP."""
    import evgrad_numpy as eg
    X, m = design(name, v, sizes)
    th = [0.3, np.full(X.shape[1], 0.1), 0.9]       # (cond Sigma ~ 1e5: the twin's own rounding stays below its 1e-7 bound)
    Sig = eg.sigma_matrix(X, th, "SE_kernel")
    f0 = 0.3 * np.linalg.cholesky(Sig) @ np.random.default_rng(X.shape[0]).standard_normal(X.shape[0])
    f = eg.fit(X, th, "SE_kernel", m, f0)
    ld, lo = orc.lambda_compact(f, m, th[0])
    return X, th, m, Sig, np.linalg.inv(Sig), f, ld, lo


EV_SIZES = ((5, 12, 3), (8, 19, 7), (1, 1, 1))
EV_DIMS = {v: dict(N=s[0] * (s[1] + 1), D=s[2], m=s[1]) for v, s in zip(("checked", "larger", "smaller"), EV_SIZES)}


@functools.lru_cache(maxsize=None)
def ev_state(name, v):
    return laplace_state(name, "larger" if v == "nonfinite" else v, EV_SIZES)


@register("laplace_logdet_65", "lu", ("WS_LINALG", "WS_VEC"), EV_DIMS, HUGE_M, legal=(1, 1, 2))
def _():
    name = "laplace_logdet_65"

    def run(eng, v):
        X, th, m, Sig, Sinv, f, ld, lo = ev_state(name, v)
        s = 1e300 if v == "nonfinite" else 1.0
        sg, ldet, info = eng.laplace_logdet(eng.dev(Sig), eng.dev(ld * s), eng.dev(lo * s), m)
        return outputs(sign=sg, logdet=ldet, info=info)

    def ref(out):                              # tests/test_gpu_lu.py: test_ipsl_real
        import lu_ref as lr
        import scipy.linalg
        X, th, m, Sig, Sinv, f, ld, lo = ev_state(name, "checked")
        M = lr.ipsl_dense(Sig, ld, lo, m)
        lu, piv = scipy.linalg.lu_factor(M)
        ref_, rpiv, info_ref = lr.getf2(M, np.longdouble)
        assert info_ref == 0 and np.array_equal(piv.astype(np.int64), rpiv) and lr.pivot_gap(lu) >= 1e-8
        s_ref, ld_ref = lr.u_slogdet(ref_)
        assert out["info"] == 0 and out["sign"] == s_ref
        assert abs(float(out["logdet"] - ld_ref)) <= lr.logdet_bound(M, lu, piv.astype(np.int64))
    return run, ref


@register("evidence_grad_65", "lu", ("WS_EVGRAD", "WS_EVGRAD_VEC", "WS_LINALG", "WS_VEC"), EV_DIMS,
          "include/ppbo_hip.h: PPBO_ERR_NOT_PD with info = 2 when Sigma^-1 - Lambda is not positive definite (Engine.evidence_grad)",
          legal=(1, 1, 2))
def _():
    name = "evidence_grad_65"

    def run(eng, v):
        X, th, m, Sig, Sinv, f, ld, lo = ev_state(name, v)
        if v == "nonfinite":
            ld = np.abs(ld) * 1e6 + 1e6        # Sigma^-1 - Lambda far from positive definite
        sg, ldet, sums, info = eng.evidence_grad(X, th, "SE_kernel", eng.dev(Sig), eng.dev(Sinv), f, eng.dev(ld), eng.dev(lo), m)
        return outputs(sign=sg, logdet=ldet, sums=sums, info=info)

    def ref(out):                              # tests/test_gpu_evidence_grad.py: _grad_case; ppbo_amd/gp_model.py: the sums' scaling
        import evgrad_numpy as eg
        X, th, m, Sig, Sinv, f, ld, lo = ev_state(name, "checked")
        want, sU = eg.evidence_grad(X, th, "SE_kernel", m, f, with_prior=False)
        g = np.append(-2.0 * (1.0 - orc.SHRINKAGE) * th[2] ** 2 * out["sums"][:-1] / th[1], 2.0 * out["sums"][-1] / th[2])
        assert out["sign"] == sU and out["info"] == 0
        assert np.max(np.abs(g - want) / np.maximum(np.abs(want), 1e-3 * np.max(np.abs(want)))) <= 1e-7, (g, want)
    return run, ref


# ============================================================ fit ========================================================
FIT_SIZES = ((3, 25, 3), (8, 26, 7), (1, 1, 1))
FIT_DIMS = {v: dict(N=s[0] * (s[1] + 1), D=s[2], m=s[1], n_q=s[0]) for v, s in zip(("checked", "larger", "smaller"), FIT_SIZES)}
NAN_START = ("tests/test_gpu_whitened.py::test_whitened_fit_rejects_bad_arguments sends a NaN start; csrc/fit.hip: 'non-finite "
             "objective at the start vector'")
FIT_TH = [0.3, 0.45, 0.9]


@functools.lru_cache(maxsize=None)
def fit_state(name, v):
    """(X, m, Sigma, Sigma^-1, L, f) on the host: f a prior draw scaled by 0.3."""
    X, m = design(name, "larger" if v == "nonfinite" else v, FIT_SIZES)
    S = orc.gram(X, FIT_TH, "SE_kernel")
    L = np.linalg.cholesky(S)
    return X, m, S, orc.pd_inverse(S), L, 0.3 * L @ np.random.default_rng(len(name)).standard_normal(X.shape[0])


def nan_start(f, v):
    if v == "nonfinite":
        f = f.copy()
        f[f.size // 2] = np.nan
    return f


def _fit_case(name, slots, doc=NAN_START):
    def deco(pair):
        return register(name, "fit", slots, FIT_DIMS, doc, legal=(1, 1, 2))(pair)
    return deco


@_fit_case("laplace_terms_78", ("WS_VEC",), "a NaN entry of f: the start vector of " + NAN_START)
def _():
    def run(eng, v):
        X, m, S, Sinv, L, f = fit_state("laplace_terms_78", v)
        T, beta, ld, lo = eng.laplace_terms(nan_start(f, v), m, FIT_TH[0])
        return outputs(T=T, beta=beta, lam_diag=ld, lam_off=lo)

    def ref(out):                              # tests/test_gpu_parity.py: test_laplace_terms_general_m
        X, m, S, Sinv, L, f = fit_state("laplace_terms_78", "checked")
        assert abs(out["T"] - (-orc.sum_phi0(f, m, FIT_TH[0]).sum() / m)) < 1e-12
        assert np.abs(out["beta"] - orc.beta_vector(f, m, FIT_TH[0])).max() < 1e-11
        d0, o0 = orc.lambda_compact(f, m, FIT_TH[0])
        assert np.abs(out["lam_diag"] - d0).max() <= 1e-12 * np.abs(d0).max()
        assert np.abs(out["lam_off"] - o0).max() <= 1e-12 * np.abs(d0).max()
    return run, ref


@_fit_case("sum_phi_78", (), "a NaN entry of f: the start vector of " + NAN_START)
def _():
    def run(eng, v):
        X, m, S, Sinv, L, f = fit_state("sum_phi_78", v)
        return outputs(phi0=eng.sum_phi(nan_start(f, v), m, FIT_TH[0], 0))

    def ref(out):
        X, m, S, Sinv, L, f = fit_state("sum_phi_78", "checked")
        want = orc.sum_phi0(f, m, FIT_TH[0])
        assert np.abs(out["phi0"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    return run, ref


@_fit_case("T_and_grad_78", ("WS_SCRATCH",), "a NaN entry of f: the start vector of " + NAN_START)
def _():
    def run(eng, v):
        X, m, S, Sinv, L, f = fit_state("T_and_grad_78", v)
        T, g = eng.T_and_grad(eng.dev(Sinv), nan_start(f, v), m, FIT_TH[0])
        return outputs(T=T, grad=g)

    def ref(out):                              # tests/test_gpu_parity.py: test_T_and_grad
        X, m, S, Sinv, L, f = fit_state("T_and_grad_78", "checked")
        T0, g0 = orc.T_value(f, Sinv, m, FIT_TH[0]), orc.T_grad(f, Sinv, m, FIT_TH[0])
        assert abs(out["T"] - T0) <= 1e-7 * max(1.0, abs(T0))
        assert np.abs(out["grad"] - g0).max() <= 1e-6 * max(np.abs(Sinv @ f).max(), 1e-300) + 1e-9
    return run, ref


def fmap_close(name, fmap):
    """__graft_entry__.smoke: |f_MAP - the oracle's| <= 3e-5 max|f| at gtol 1e-6."""
    X, m, S, Sinv, L, f = fit_state(name, "checked")
    f0, _ = orc.fit_fmap_trust_exact(f, Sinv, m, FIT_TH[0])
    assert np.abs(fmap - f0).max() <= 3e-5 * np.abs(f0).max()
    return f0


def _fmap_case(name, whitened):
    slots = ("WS_LINALG", "WS_SCRATCH", "WS_SMALL", "WS_POTRF") + (("WS_LBFGS", "WS_LBFGS_U", "WS_VEC") if whitened else ())

    @_fit_case(name, slots)
    def _():
        def run(eng, v):
            X, m, S, Sinv, L, f = fit_state(name, v)
            fm, st = eng.fit_fmap(eng.dev(Sinv), nan_start(f, v), m, FIT_TH[0], gtol=1e-6, L=eng.dev(L) if whitened else None)
            return outputs(fMAP=fm, **{k: st[k] for k in ("iterations", "n_cholesky", "converged", "T", "gradnorm", "lbfgs_iterations",
                                                          "lbfgs_evals", "lbfgs_status")})

        def ref(out):
            fmap_close(name, out["fMAP"])
            assert out["converged"]
        return run, ref


_fmap_case("fit_fmap_exact_78", False)
_fmap_case("fit_fmap_whitened_78", True)


@_fit_case("gp_fit_78", ("WS_LINALG", "WS_LINALG2", "WS_SCRATCH", "WS_SMALL", "WS_POTRF", "WS_LBFGS", "WS_LBFGS_U", "WS_VEC"))
def _():
    name = "gp_fit_78"

    def run(eng, v):
        X, m, S, Sinv, L, f = fit_state(name, v)
        kern = "SE_kernel" if v in ("checked", "smaller") else "RQ_kernel"
        form = FORM_NODE if v in ("checked", "smaller") else FORM_EDGE
        r = eng.gp_fit(X, FIT_TH, kern, m, nan_start(f, v), gtol=1e-6, want_Linv=True, form=form)
        p, st = r["post"], r["stats"]
        return outputs(Sigma=r["Sigma"], Sigma_inv=r["Sigma_inv"], L=r["L"], Linv=r["Linv"], fMAP=r["fMAP"], alpha=p.alpha,
                       lam_diag=p.lam_diag, lam_off=p.lam_off, G=p.G, info=r["info"], iterations=st["iterations"],
                       n_cholesky=st["n_cholesky"], T=st["T"], gradnorm=st["gradnorm"], lbfgs_evals=st["lbfgs_evals"])

    def ref(out):                              # __graft_entry__.smoke's bounds
        X, m, S, Sinv, L, f = fit_state(name, "checked")
        sf2 = FIT_TH[2] ** 2
        assert np.abs(out["Sigma"] - S).max() <= 1e-12 * sf2
        Ld = np.tril(out["L"])                 # tests/test_gpu_incremental.py: the factor by its backward error
        assert np.abs(Ld @ Ld.T - S).max() <= 1e-12 * np.abs(L).max() ** 2
        fmap_close(name, out["fMAP"])
        assert np.all(np.triu(out["Linv"], 1) == 0.0), "the full triangular inverse: zeros above the diagonal"
        # (triangular inversion, forward bound: |Linv L - I| <= c N eps |Linv| |L|; Sigma's condition is ~4e7 here)
        assert np.abs(out["Linv"] @ Ld - np.eye(78)).max() <= 4 * 78 * EPS * np.abs(out["Linv"]).max() * np.abs(Ld).max()
        assert np.abs(S @ out["alpha"] - out["fMAP"]).max() <= 1e-6 * np.abs(out["fMAP"]).max() and out["info"] == 0
    return run, ref


def _posterior_case(name, form):
    @_fit_case(name, ("WS_LINALG", "WS_SMALL", "WS_POTRF", "WS_LINALG2"), NOT_PD)
    def _():
        def run(eng, v):
            X, m, S, Sinv, L, f = fit_state(name, v)
            # non-finite: every pseudo-observation sqrt(2) sigma above its observation, which maximises Lambda's weights
            # (tests/test_gpu_parity.py::test_error_codes_and_messages: Sigma^-1 - Lambda is then indefinite)
            fm = np.where(np.arange(f.size) % (m + 1) != 0, 1.414 * FIT_TH[0], 0.0) if v == "nonfinite" else f
            other = v in ("larger", "nonfinite")
            p = eng.posterior(X, FIT_TH, "SE_kernel", eng.dev(Sinv), fm, m, want_P=True, form=(1 - form) if other else form)
            return outputs(alpha=p.alpha, lam_diag=p.lam_diag, lam_off=p.lam_off, G=p.G, P=p.P)

        def ref(out):                          # tests/test_gpu_parity.py: alpha, P at 1e-6; the variance through the form's G
            X, m, S, Sinv, L, f = fit_state(name, "checked")
            P0 = orc.posterior_covariance(Sinv, f, m, FIT_TH[0])
            assert rel(out["alpha"], Sinv @ f) < 1e-6
            assert np.abs(out["P"] - P0).max() <= 1e-6 * np.abs(np.diag(P0)).max()
            d0, o0 = orc.lambda_compact(f, m, FIT_TH[0])
            assert np.abs(out["lam_diag"] - d0).max() <= 1e-12 * np.abs(d0).max()
            hm = HostModel(0, 3, 25, 3, "SE_kernel", form, theta=tuple(FIT_TH))
            hm.X, hm.alpha, hm.ld, hm.lo, hm.G = X, out["alpha"], out["lam_diag"], out["lam_off"], out["G"]
            Xc = np.random.default_rng(3).random((50, 3))
            A = orc.variance_operator(Sinv, P0, False, lam=orc.lambda_dense(f, m, FIT_TH[0]))
            _, var0 = orc.predict_mean_var(Xc, X, FIT_TH, Sinv @ f, A, "SE_kernel")
            assert np.abs(hm.mean_var(Xc)[1] - var0).max() <= 1e-6 * FIT_TH[2] ** 2
        return run, ref


_posterior_case("posterior_node_78", FORM_NODE)
_posterior_case("posterior_edge_78", FORM_EDGE)


@_fit_case("posterior_form_78", (), "takes sizes only: the history is the call at the larger sizes")
def _():
    def run(eng, v):
        d = FIT_DIMS["larger" if v == "nonfinite" else v]
        return outputs(form=eng.posterior_form("SE_kernel" if v != "nonfinite" else "camphor_copper_kernel", d["N"], d["D"], d["m"]))

    def ref(out):                              # csrc/fused.hip: the default one-launch shapes take FORM_NODE (N = 78, D = 3, SE)
        assert out["form"] == FORM_NODE
    return run, ref


@_fit_case("transposed_G_78", (), HUGE_M)
def _():
    def run(eng, v):
        mod = model("A", v)
        return outputs(Gt=eng.transposed_G(eng.dev(mod.G * (1e300 if v == "nonfinite" else 1.0))))

    def ref(out):                              # csrc/fused.hip: "zeros outside [N][N]", the transpose inside
        mod = model("A", "checked")
        Gt, N = out["Gt"], mod.N
        assert Gt.shape == (((N + 15) & ~15) + 16, ((N + 31) & ~31) + 32)
        assert np.array_equal(Gt[:N, :N], mod.G.T) and np.all(Gt[N:] == 0.0) and np.all(Gt[:, N:] == 0.0)
    return run, ref


# ============================================================ the coordinate maps of the mean searches ====================
CAMPHOR_ARD = "camphor_copper_ard_kernel"


def _coords_case(name, kind):
    """mean_grad, mean_ascent and mean_search_multi of a mean-only model with per-dimension length scales (kind "ard":
    SE, the scaled map) or the per-coordinate camphor kernel (kind "cam": the embedding), as mean_calls of
    tests/test_gpu_coords.py runs them; they reach the slots of the maps' coefficients and mapped rows."""
    sz = dict(checked=(8, 3, 6), larger=(16, 9, 21 if kind == "ard" else 6), smaller=(1, 1, 1 if kind == "ard" else 6))
    dims = {v: dict(N=s[0] * (s[1] + 1), n_q=s[0], m=s[1], M=M, K=K, T=T, **(dict(D=s[2]) if kind == "ard" else {}))
            for (v, s), M, K, T in zip(sz.items(), (130, 1000, 1), (4, 16, 1), (2, 5, 1))}
    slots = ("WS_TRANSPOSE", "WS_SEARCH", "WS_SEARCH_SMALL", "WS_SEARCH_ROWS", "WS_PART") + (
        ("WS_SCALE", "WS_SCALE_SEARCH") if kind == "ard" else ("WS_CAMPHOR", "WS_CAMPHOR_ROWS"))

    @register(name, "search", slots, dims, NAN_POOL + "; finite but huge (1e300) alpha for mean_grad and mean_ascent",
              legal=(1, 1, 2))
    def _():
        def inputs(v):
            vv = "larger" if v == "nonfinite" else v
            n_q, m, D = sz[vv]
            rng = rng_of(name, v)
            d = dims[vv]
            X = star_rows(rng, n_q, m, D)
            th = [0.1, rng.uniform(0.3, 1.1, D) if kind == "ard" else CAM_L, 0.7]
            r = dict(X=X, th=th, m=m, alpha=rng.standard_normal(X.shape[0]), pts=rng.random((5, D)), starts=rng.random((d["K"], D)),
                     pool=rng.random((d["M"], D)), shifts=rng.random((d["T"], D)), xprev=rng.random(D), K=d["K"])
            if v == "nonfinite":
                r["pool"][::7, 0] = np.nan
            return r

        def run(eng, v):
            r = inputs(v)
            kern = "SE_kernel" if kind == "ard" else CAMPHOR_ARD
            post = eng.mean_posterior(r["X"], r["th"], kern, r["m"], eng.dev(r["alpha"]))
            huge = eng.mean_posterior(r["X"], r["th"], kern, r["m"], eng.dev(r["alpha"] * 1e300)) if v == "nonfinite" else post
            mu, g = eng.mean_grad(huge, r["pts"])
            xa, ma, it = eng.mean_ascent(huge, r["starts"], iters=10, tol=1e-9)
            xs, ms = eng.mean_search_multi(post, r["pool"], r["shifts"], extra="design", xprev=r["xprev"], K=r["K"], sep=0.05,
                                           iters=10, tol=1e-9)
            return outputs(grad_mu=mu, grad=g, ascent_x=xa, ascent_mu=ma, ascent_it=it, multi_x=xs, multi_mu=ms)

        def ref(out):                          # tests/search_ref.py: fg_ard / fg_camphor_ard in the caller's coordinates
            import search_ref as sr
            r = inputs("checked")
            fg = sr.fg_ard(r["X"], r["th"], r["alpha"], "SE_kernel") if kind == "ard" else sr.fg_camphor_ard(r["X"], CAM_L, 0.7, r["alpha"])
            for x, mu, g in zip(r["pts"], out["grad_mu"], out["grad"]):
                f0, g0 = fg(x)
                assert abs(mu - f0) <= 1e-9 * max(abs(f0), 1e-300) + 1e-14
                assert np.abs(g - g0).max() <= 1e-5 * max(1.0, np.abs(g0).max())      # tests/test_gpu_ard.py
            ok = np.isfinite(out["multi_mu"])
            xs = np.concatenate([out["ascent_x"], out["multi_x"][ok]])
            ms = np.concatenate([out["ascent_mu"], out["multi_mu"][ok]])
            want = np.array([fg(x)[0] for x in xs])
            assert ok.any() and np.all((xs >= 0) & (xs <= 1))
            assert np.abs(want - ms).max() <= 1e-9 * np.abs(want).max() + 1e-14        # the value IS the mean there
        return run, ref


_coords_case("mean_ard_B", "ard")
_coords_case("mean_camphor_B", "cam")


# ============================================================ the slots ==================================================
# slots no checked call requests, and why
UNREACHED = {
    "WS_DIST": "requested by ppbo_dist_* / ppbo_argmax_allgather* / ppbo_search_sharded* only: they need several ranks "
               "(tests/test_gpu_sharded.py and tests/test_gpu_dist.py own them)",
}


def reached():
    return {s for c in CASES.values() for s in c.slots}


# ============================================================ the neighbours sequence ====================================
FAMILY_ORDER = ("fit", "predict", "rff", "lu", "predictor", "line", "dense", "search", "points")


def neighbours(env=()):
    """One fixed order of the checked calls of an engine setting that interleaves the families sharing WS_SMALL, WS_VEC,
    WS_LINALG, WS_PART, WS_KSTAR and WS_TRANSPOSE: fit, predict, RFF, LU, predictors, lines, dense, searches, points, the
    fit again, ... -- one call of each family in turn until every family is used up."""
    env = tuple(sorted(dict(env).items()))
    by = {f: [c.name for c in CASES.values() if c.family == f and c.env == env] for f in FAMILY_ORDER}
    seq = []
    while any(by.values()):
        for f in FAMILY_ORDER:
            if by[f]:
                seq.append(by[f].pop(0))
    return seq


def envs():
    return sorted({c.env for c in CASES.values()})
