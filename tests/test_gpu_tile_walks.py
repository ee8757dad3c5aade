"""GPU: every tile shape (PPBO_QF_VARIANT 0-5), operand form (node, edge with kshift, dense T) and tile walk
(PPBO_QF_ORDER) of quadform_kernel against NumPy on EVERY column; the default walk at production tile counts; and the
two other knobs no test set before: PPBO_GRAM_VARIANT (the walk of gram_mfma_kernel) and PPBO_POTRF_GEN=2.

How the checks reach the kernel: the hand-built posteriors of test_gpu_kstar_star.py (random alpha, Lambda and operator of
the form's sparsity) make mean and variance plain functions of K* that NumPy evaluates from its own K*:
    mu = K*' alpha,   var = sf2 + t + |G K*|^2 (node)  or  |H E|^2 (edge)  or  |T E|^2 (dense, a hand-built projection),
and every engine is created with PPBO_FUSED=0, so every model takes kstar_kernel -> quadform_kernel -> score_kernel.  The
knobs are read once per ctx: one engine per (variant, order), closed afterwards.

Models (the smallest that reach each branch) and the candidate counts 130 / 2100 / 4200 = 2 / 17 / 33 column tiles of 128:
    N = 234 (n_q =  9, m = 25)  N % 16 != 0, ragged 26-row stars; M < 2048: guarded loop on the model's own G
    N = 416 (n_q = 13, m = 31)  a multiple of 16, not of 128; M >= 2048: padded operands, lean loop; 4 row tiles of 128, 2 of 256
    N = 384 (n_q = 12, m = 31)  three whole 128-row tiles; variant 5 pads to 512 and its zero frame takes wrow_beg >= n_rows
    N = 272 (n_q = 17, m = 15)  edge form: ppbo_edge_k0(17) = 16, kshift > 0 (0 for the other models)
    N = 676 (n_q = 26, m = 25)  dense mode: ld = 688 > N, kshift = 16, r_max = 256

Grids ntm x ntn (workgroups; the XCD remap of bit 0 is on from 64 workgroups, uneven over the XCDs when grid % 8 != 0):
                     variants 0-4 (128-row tiles)           variant 5 (256-row tiles)
    M =              130      2100      4200                130      2100      4200
    N = 234         2x2=4    2x17=34   2x33=66             1x2=2    1x17=17   1x33=33
    N = 416         4x2=8    4x17=68   4x33=132            2x2=4    2x17=34   2x33=66
    N = 384, 272    3x2=6    3x17=51   3x33=99             2x2=4    2x17=34   2x33=66
    dense r = 128   1x2=2    1x17=17   1x33=33             (variant 5 runs dense operands as variant 4)
    dense r = 256   2x2=4    2x17=34   2x33=66
so every variant has grids of 66 / 68 / 99 / 132 (remap on, none a multiple of 8) and grids below 64 (remap off).  Orders 14
and 23 (chunks of 3 and 5 tiles) leave a narrower last chunk at 17 and 33 tiles; 258 (chunk of 64 >= ntn) is the unchunked
branch; unset is 1026 here (N <= 1024).  The cross product is small enough to run whole: 6 variants x 8 orders x 4 models
x 2 forms x 3 counts.

Bounds (the project's own, test_gpu_kstar_star.py): mu 1e-9 relative in the max norm, var 1e-8 sf2, argued there for
N <= 288 with |var| <= 20 sf2.  Here N <= 676 in the sweeps and |var| <= 570 sf2 (G's entries are O(1 / sqrt(N)), K*'s up to
sf2): a depth-676 fp64 sum of such terms rounds at no more than 1.1e-16 * 676 * 570 = 4e-11 sf2, two orders below the bound.
At N = 1040 the float64 reference itself is checked against np.longdouble (test_default_walk_at_production_tile_counts).
Between the orders of one variant mu, var, best index and best value are BITWISE equal: a tile's K range depends on mt
only and score_kernel adds the slabs in a fixed order.  Between variants they lie within the reference bound of each other
(the 256-row tile cuts the slabs differently)."""
import functools
import os

import numpy as np
import pytest

from test_gpu_kstar_star import Hand, _engine, host, kstar_ref, mean_var_ref, star_design

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 2, 3, 4, 5)
ORDERS = (None, 0, 1, 2, 3, 14, 23, 258)          # None: PPBO_QF_ORDER unset
MS = (130, 2100, 4200)
THETA = [1.0, 0.45, 1.3]
SF2 = THETA[2] ** 2
# name -> (n_q, m, D, kernel)
MODELS = {234: (9, 25, 3, "SE_kernel"), 416: (13, 31, 5, "RQ_kernel"), 384: (12, 31, 2, "Matern52_kernel"),
          272: (17, 15, 4, "Matern32_kernel")}
DENSE = (26, 25, 3, "SE_kernel")                  # N = 676


def grid_of(variant, N, M, rows=None):
    """(ntm, ntn) of the launch: rows = the padded row count of a dense operand (always on 128-row tiles)."""
    bm = 256 if (variant == 5 and rows is None) else 128
    return -(-(rows or N) // bm), -(-M // 128)


def knob_engine(variant=None, order=None, **more):
    """PPBO_FUSED=0 and the two contraction knobs; None = unset, whatever the caller's environment holds."""
    env = dict(PPBO_FUSED=0, **more)
    gone = {}
    for k, v in (("PPBO_QF_VARIANT", variant), ("PPBO_QF_ORDER", order)):
        if v is None:
            gone[k] = os.environ.pop(k, None)
        else:
            env[k] = v
    try:
        return _engine(**env)
    finally:
        os.environ.update({k: v for k, v in gone.items() if v is not None})


# ---- the cases: hand-built posteriors, candidates and their NumPy references, formed once -------------------------------
@functools.lru_cache(maxsize=None)
def case(N, form):
    """(Hand, {M: (Xc, mu0, var0)}) of a model of MODELS in one form."""
    n_q, m, D, kernel = MODELS[N]
    rng = np.random.default_rng(10 * N + form)
    hand = Hand(rng, star_design(rng, n_q, m, D, "general", zero_row=True), THETA, kernel, m, form)
    refs = {}
    for M in MS:
        Xc = rng.random((M, D))
        refs[M] = (Xc,) + hand.reference(Xc)[1:]
    return hand, refs


_DEVICE = {}


def on_device(key, make):
    """Device twins shared by all engines of this file (they are plain tensors on the one GPU)."""
    if key not in _DEVICE:
        _DEVICE[key] = make()
    return _DEVICE[key]


def scored(eng, post, key, Xc, projection=None):
    """One checked call.  Before it the same engine scores 1 - Xc, a call of the same shape: the slab lives in a
    workspace that survives calls, so a tile that a wrong walk never writes would otherwise keep the previous call's value
    -- in a sweep that repeats shapes, the CORRECT one.  After the poisoning call the workspace holds the numbers of other
    candidates wherever the checked call fails to write."""
    from ppbo_amd.engine import SCORE_VARIANCE
    Xd, Xp = on_device(("Xc",) + key, lambda: (eng.dev(Xc), eng.dev(1.0 - Xc)))
    eng.predict(post, Xp, score=SCORE_VARIANCE, projection=projection)
    out = eng.predict(post, Xd, score=SCORE_VARIANCE, projection=projection)
    return host(out["mu"]), host(out["var"]), out["best_idx"], out["best_val"]


def errors(res, mu0, var0):
    mu, var, bi, bv = res
    return np.abs(mu - mu0).max() / np.abs(mu0).max(), np.abs(var - var0).max() / SF2


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


_SWEEP = {}


def sweep(variant):
    """{order: {(N, form, M): (mu, var, best_idx, best_val)}} of one tile shape, every order on every model, run once."""
    if variant in _SWEEP:
        return _SWEEP[variant]
    out = {}
    for order in ORDERS:
        eng = knob_engine(variant, order)
        try:
            res = {}
            for N in MODELS:
                for form in (0, 1):
                    hand, refs = case(N, form)
                    post = on_device(("post", N, form), lambda: hand.on(eng))
                    for M in MS:
                        res[N, form, M] = scored(eng, post, (N, form, M), refs[M][0])
            out[order] = res
        finally:
            eng.close()
    _SWEEP[variant] = out
    return out


# ---- 1. every shape x form x walk ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_order_of_a_tile_shape_against_numpy(variant):
    """All eight orders on all four models in both forms at 2, 17 and 33 column tiles: mu and var of every column against
    NumPy, best_idx = argmax of the returned var, and the orders of the variant bitwise equal to each other."""
    grids = sorted({g[0] * g[1] for N in MODELS for M in MS for g in [grid_of(variant, N, M)]})
    print(f"variant {variant}: grids " + " ".join(f"N={N}:" + ",".join("%dx%d" % grid_of(variant, N, M) for M in MS) for N in MODELS))
    assert any(g >= 64 and g % 8 for g in grids) and any(g < 64 for g in grids)
    res = sweep(variant)
    worst_mu = worst_var = 0.0
    bad = []
    for order in ORDERS:
        for key, r in res[order].items():
            N, form, M = key
            _, mu0, var0 = case(N, form)[1][M]
            e_mu, e_var = errors(r, mu0, var0)
            worst_mu, worst_var = max(worst_mu, e_mu), max(worst_var, e_var)
            ok = e_mu <= 1e-9 and e_var <= 1e-8 and r[2] == int(np.argmax(r[1])) and r[3] == r[1][r[2]]
            if not (ok and same_bits(r, res[None][key])):
                bad.append((order, key, float(e_mu), float(e_var), ok))
    print(f"variant {variant}: worst mu {worst_mu:.2e} (relative), worst var {worst_var:.2e} sf2 over {len(ORDERS)} orders x "
          f"{len(res[None])} cases; largest |var| {max(np.abs(r[1]).max() for r in res[None].values()) / SF2:.1f} sf2")
    assert not bad, bad[:8]


def test_tile_shapes_agree_with_each_other():
    """Between variants (default order; the others are bitwise equal to it): within the reference bound of each other."""
    base = sweep(4)[None]
    for variant in VARIANTS:
        other = sweep(variant)[None]
        d_mu = max(np.abs(other[k][0] - base[k][0]).max() / np.abs(base[k][0]).max() for k in base)
        d_var = max(np.abs(other[k][1] - base[k][1]).max() / SF2 for k in base)
        print(f"variant {variant} against 4: mu {d_mu:.2e} var {d_var:.2e} sf2")
        assert d_mu <= 1e-9 and d_var <= 1e-8


# ---- dense operands: a hand-built projection -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(r):
    """An edge-form Hand of N = 676, a random dense T [r][ld] in the layout ppbo_model.proj names (columns [0, n_q) and
    [N, ld) zero), and {M: (Xc, mu0, var0)} with var0 = sf2 + t + |T E|^2: mean_var_ref with T's first N columns as the
    operator (its rows [0, n_q) of E are zero, the columns beyond N meet the zeroed K* rows)."""
    n_q, m, D, kernel = DENSE
    N, ld = n_q * (m + 1), (n_q * (m + 1) + 15) & ~15
    rng = np.random.default_rng(5000 + r)
    hand = Hand(rng, star_design(rng, n_q, m, D, "general"), THETA, kernel, m, 1)
    T = rng.standard_normal((r, ld)) / np.sqrt(N)
    T[:, :n_q] = 0.0
    T[:, N:] = 0.0
    refs = {}
    for M in MS:
        Xc = rng.random((M, D))
        K = kstar_ref(hand.X, Xc, THETA, kernel)
        refs[M] = (Xc,) + mean_var_ref(K, hand.alpha, hand.ld, hand.lo, T[:, :N], m, 1, SF2)
    return hand, T, refs


@pytest.mark.parametrize("r", [128, 256])
def test_dense_operand_against_numpy(r):
    """QF_DENSE with an operator the library did not build: every order on variants 4 and 5 (which runs dense operands as
    4: the same bits), every column against NumPy."""
    from ppbo_amd import _lib
    from ppbo_amd.engine import VarianceProjection
    hand, T, refs = dense_case(r)
    N, ld = hand.X.shape[0], T.shape[1]
    assert ld > N and (N // (hand.m + 1)) & ~15 > 0          # the zero columns behind N exist, kshift > 0
    print(f"dense r={r}: grids " + ",".join("%dx%d" % grid_of(4, N, M, rows=r) for M in MS))
    results, worst_mu, worst_var = {}, 0.0, 0.0
    for variant in (4, 5):
        for order in ORDERS:
            eng = knob_engine(variant, order)
            try:
                post = on_device(("dense post", r), lambda: hand.on(eng))
                Td = on_device(("T", r), lambda: eng.dev(T))
                st = _lib.VarProjection(d_T=Td.data_ptr(), rows=r, rows_padded=r, ld=ld, bound=0.0, tol=1e-10)
                pj = VarianceProjection(Td, st, 1e-10)
                for M in MS:
                    results[variant, order, M] = scored(eng, post, ("dense", r, M), refs[M][0], projection=pj)
            finally:
                eng.close()
    bad = []
    for (variant, order, M), res in results.items():
        e_mu, e_var = errors(res, *refs[M][1:])
        worst_mu, worst_var = max(worst_mu, e_mu), max(worst_var, e_var)
        ok = e_mu <= 1e-9 and e_var <= 1e-8 and res[2] == int(np.argmax(res[1])) and res[3] == res[1][res[2]]
        if not (ok and same_bits(res, results[4, None, M])):
            bad.append((variant, order, M, float(e_mu), float(e_var), ok))
    print(f"dense r={r}: worst mu {worst_mu:.2e} (relative), worst var {worst_var:.2e} sf2 over {len(results)} calls")
    assert not bad, bad[:8]


# ---- the default walk at production tile counts --------------------------------------------------------------------------
def se_kstar_longdouble(X, Xc, theta):
    ld = np.longdouble
    r2 = ((X.astype(ld)[:, None, :] - Xc.astype(ld)[None, :, :]) ** 2).sum(-1)
    return ld(theta[2]) ** 2 * np.exp(ld(-0.5) * r2 / ld(theta[1]) ** 2)


@pytest.mark.parametrize("n_q,m,M,chunks", [(9, 25, 40000, (256, 57)), (40, 25, 20000, (128, 29))])
@pytest.mark.parametrize("form", [0, 1])
def test_default_walk_at_production_tile_counts(n_q, m, M, chunks, form):
    """The walks that ship, where they chunk: N = 234, M = 40000 (order 1026: 313 column tiles = a chunk of 256 and one of
    57) and N = 1040, M = 20000 (order 514: 157 tiles = 128 + 29), on an engine with neither knob set.  NumPy on the first,
    the last and one random column of EVERY 128-column tile; best_idx = argmax of the returned var.
    N = 1040 is beyond the N <= 288 the bounds were argued for, so the float64 reference is first compared with the same
    expression in np.longdouble on those columns; it must agree to 1e-10 sf2 (measured: node form 1.2e-12 sf2 with |var| up
    to 1045 sf2, edge form 9.1e-13 sf2; mu 1.3e-15 relative), two orders below the bound it is then used at."""
    from ppbo_amd.engine import SCORE_VARIANCE
    N, D = n_q * (m + 1), 4
    ntn = -(-M // 128)
    assert N <= 1024 or chunks[0] == 128
    assert ntn == sum(chunks) and ntn > chunks[0] and ntn % chunks[0] == chunks[1]
    rng = np.random.default_rng(N + form)
    hand = Hand(rng, star_design(rng, n_q, m, D, "general", zero_row=True), THETA, "SE_kernel", m, form)
    Xc = rng.random((M, D))
    first = np.arange(ntn) * 128
    last = np.minimum(first + 127, M - 1)
    sel = np.unique(np.r_[first, last, first + rng.integers(1, np.maximum(last - first, 2))])
    sel = sel[sel < M]
    K, mu0, var0 = hand.reference(Xc[sel])
    if N > 288:
        ldt = np.longdouble
        mu1, var1 = mean_var_ref(se_kstar_longdouble(hand.X, Xc[sel], THETA), hand.alpha.astype(ldt), hand.ld.astype(ldt),
                                 hand.lo.astype(ldt), hand.G.astype(ldt), m, form, ldt(SF2))
        r_mu, r_var = float(np.abs(mu0 - mu1).max() / np.abs(mu1).max()), float(np.abs(var0 - var1).max() / SF2)
        print(f"N={N} form={form}: float64 reference against longdouble: mu {r_mu:.2e} (relative) var {r_var:.2e} sf2")
        assert r_mu <= 1e-10 and r_var <= 1e-10
    eng = knob_engine()
    try:
        mu, var, bi, bv = scored(eng, hand.on(eng), ("prod", N, form), Xc)
    finally:
        eng.close()
    _DEVICE.pop(("Xc", "prod", N, form))
    e_mu, e_var = np.abs(mu[sel] - mu0).max() / np.abs(mu0).max(), np.abs(var[sel] - var0).max() / SF2
    print(f"N={N} form={form} M={M}: {ntn} column tiles, {len(sel)} reference columns: mu {e_mu:.2e} (relative) "
          f"var {e_var:.2e} sf2, largest |var| {np.abs(var).max() / SF2:.1f} sf2")
    assert e_mu <= 1e-9 and e_var <= 1e-8
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
    assert bi == int(np.argmax(var)) and bv == var[bi]


# ---- 3. PPBO_GRAM_VARIANT: the two walks of gram_mfma_kernel -------------------------------------------------------------
@pytest.fixture(scope="module")
def gram_engines():
    engines = [_engine(PPBO_GRAM_VARIANT=0), _engine(PPBO_GRAM_VARIANT=1)]
    yield engines
    for e in engines:
        e.close()


@pytest.mark.parametrize("kernel", ["SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel"])
@pytest.mark.parametrize("D", [3, 20])
def test_gram_walks(gram_engines, kernel, D):
    """Row-major (0) and diagonal-major (1) at 1, 2, 3 and 11 tiles of 64 per side with ragged last tiles: every entry
    against direct differences with the shrinkage applied (1e-12 sf2, the suite's K* / Sigma parity level), Sigma bitwise
    symmetric, the two walks bitwise equal (only the walk differs).  The output buffer is filled with NaN first: a tile
    that a walk leaves out cannot pass as the previous call's value."""
    from ppbo_amd.engine import SHRINKAGE
    rng = np.random.default_rng(D)
    theta = [1.0, 0.5 * np.sqrt(D / 3.0), 1.3]
    worst = 0.0
    for N in (1, 65, 130, 650, 700):
        X = rng.random((N, D))
        S0 = (1.0 - SHRINKAGE) * kstar_ref(X, X, theta, kernel) + SHRINKAGE * SF2 * np.eye(N)
        got = []
        for eng in gram_engines:
            out = eng.empty(N, N)
            out.fill_(float("nan"))
            got.append(host(eng.gram(X, theta, kernel, out=out)))
        worst = max(worst, np.abs(got[0] - S0).max() / SF2)
        assert np.abs(got[0] - S0).max() <= 1e-12 * SF2, N
        assert np.array_equal(got[0], got[0].T), N
        assert np.array_equal(got[0], got[1]), N
    print(f"{kernel} D={D}: worst entry against direct differences {worst:.2e} sf2")


# ---- 3. PPBO_POTRF_GEN=2: potf2_block_kernel + trsm_mfma_kernel + SYRK ---------------------------------------------------
@pytest.fixture(scope="module")
def gen2():
    e = _engine(PPBO_POTRF_GEN=2)
    yield e
    e.close()


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("N", [1, 64, 65, 200, 650, 1031])
def test_factorization_generation_2(gen2, N):
    """The matrices and bounds of test_gpu_parity.py::test_factor_triangular_inverse_and_inverse_together on the three-launch
    factorization: L, L^-1 and A^-1 entry by entry, the not-positive-definite report with its leading minor, and a ctx
    that stays usable."""
    eng = gen2
    rng = np.random.default_rng(N)
    Q = rng.standard_normal((N, N))
    A = Q @ Q.T + N * np.eye(N)
    Ai, Li, L = eng.pd_inverse_factors3(A)
    Ai, Li, L = host(Ai), host(Li), np.tril(host(L))
    assert rel(L, np.linalg.cholesky(A)) < 1e-12
    assert np.array_equal(np.triu(Li, 1), np.zeros_like(Li))
    assert np.abs(Li @ L - np.eye(N)).max() < 1e-11
    assert rel(Li, np.linalg.inv(np.linalg.cholesky(A))) < 1e-11
    assert np.abs(Ai - Li.T @ Li).max() <= 1e-12 * np.abs(Ai).max()
    if N >= 3:
        B = A.copy()
        bad = max(1, (2 * N) // 3)
        B[bad, bad] = -1.0
        from ppbo_amd.engine import NotPositiveDefinite
        with pytest.raises(NotPositiveDefinite) as ei:
            eng.pd_inverse_factors3(B)
        assert ei.value.info == bad + 1
    Ai2 = host(eng.pd_inverse(A))
    assert np.array_equal(Ai2, Ai)
