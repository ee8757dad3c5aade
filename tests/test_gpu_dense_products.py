"""GPU: the fp64 MFMA GEMM engine (ppbo_gemm_launch, ppbo_amd/csrc/gemm.hip) in each of its four tile configurations,
and the library's dense products at the sizes that put them on the 128 x 128 tiles, against CPU references that take
no device intermediate (tests/dense_ref.py).

The engine picks a configuration by size: GCBig16 (128 x 128, 16 wavefronts) when there are >= 1024 tiles of 128 x 128
and K >= 256 (GCBig, 8 wavefronts, with PPBO_GEMM_BIG16=0); else GCTiny (32 x 32) when there are <= 384 tiles of
64 x 64 and K >= 128; else GCSmall (64 x 64).  GCTiny and GCSmall start from C when alpha = +-beta ("preload")."""
import ctypes as C
import os

import numpy as np
import pytest

import dense_ref as dr
import evgrad_numpy as eg
from conftest import load_golden
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu

U = dr.U
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _engine(**env):
    """A fresh Engine whose ctx reads the given PPBO_* settings (they are read once, at ppbo_ctx_create)."""
    from ppbo_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng8(eng):
    """GCBig (8 wavefronts) in place of GCBig16 for every large product."""
    e = _engine(PPBO_GEMM_BIG16=0)
    yield e
    e.close()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- ppbo_dgemm in every configuration
# (M, N, K) per configuration, off the tile edges and off BK = 16 unless stated.  M = 1 / N = 1 put a whole row / column
# of tiles on their first row / column; on the 128 x 128 tiles that takes 1025 column (row) tiles, the last one 1 wide.
SHAPES = {
    "tiny": [(200, 190, 129), (1, 190, 300), (190, 1, 300), (31, 33, 2047)],
    "small": [(1300, 1201, 259), (1100, 1500, 100), (130, 75, 33), (1, 70, 17), (70, 1, 17)],
    "big": [(4097, 4095, 257), (4096, 4096, 256), (4000, 4129, 270), (1, 131073, 257), (131073, 1, 257)],
}
CASES = [(cfg, s) for cfg, shapes in SHAPES.items() for s in shapes]


def _config(M, N, K):
    """The configuration ppbo_gemm_launch picks for an unbatched product (gemm.hip)."""
    if ((M + 127) // 128) * ((N + 127) // 128) >= 1024 and K >= 256:
        return "big"
    if ((M + 63) // 64) * ((N + 63) // 64) <= 384 and K >= 128:
        return "tiny"
    return "small"


def _operands(rng, M, N, K, ta, tb, integer):
    draw = (lambda s: rng.integers(-8, 9, s).astype(np.float64)) if integer else rng.standard_normal
    return draw((K, M) if ta else (M, K)), draw((N, K) if tb else (K, N)), draw((M, N))


def _engines(cfg, eng, eng8):
    return [eng, eng8] if cfg == "big" else [eng]


@pytest.mark.parametrize("cfg,shape", CASES)
@pytest.mark.parametrize("ta,tb", TRANS)
def test_dgemm_exact_on_integer_operands(eng, eng8, cfg, shape, ta, tb):
    """Integer operands in [-8, 8] and alpha, beta multiples of 1/2: every partial sum is exact in fp64, so C must equal
    NumPy's product bit for bit, every entry, in any summation order.  (alpha, beta): alpha = beta and alpha = -beta
    (GCTiny / GCSmall start from C), and beta = 0 with C full of NaN (C is not read: no NaN may survive).  On the
    128 x 128 tiles both GCBig16 and GCBig."""
    M, N, K = shape
    assert _config(M, N, K) == cfg
    rng = np.random.default_rng(M * 31 + N * 7 + K + 2 * ta + tb)
    A, B, C0 = _operands(rng, M, N, K, ta, tb, integer=True)
    AB = dr.op(A, ta) @ dr.op(B, tb)
    for alpha, beta in [(1.5, 1.5), (2.5, -2.5), (-0.5, 0.0)]:
        c0 = C0 if beta != 0.0 else np.full((M, N), np.nan)
        ref = alpha * AB + (beta * c0 if beta != 0.0 else 0.0)
        for e in _engines(cfg, eng, eng8):
            out = host(e.dgemm(A, B, bool(ta), bool(tb), alpha=alpha, beta=beta, C_out=e.dev(c0)))
            assert np.array_equal(out, ref), (alpha, beta, np.argwhere(out != ref)[:5])


@pytest.mark.parametrize("cfg,shape", CASES)
@pytest.mark.parametrize("ta,tb", TRANS)
def test_dgemm_rounding_vs_long_double(eng, eng8, cfg, shape, ta, tb):
    """Random operands against long-double dot products on every row / column that is a 32-, 64- or 128-tile edge plus
    the whole last partial 128-tile, entry by entry within 2 K u (|alpha| (|A||B|)_ij + |beta| |C0_ij|).  On the
    128 x 128 tiles GCBig and GCBig16 must agree bit for bit (a K sum's order does not depend on the wavefront layout).
    Worst measured ratio to the bound on MI355X: GCTiny 0.015, GCSmall 0.058 (K = 17 / 33), GCBig16 0.010."""
    M, N, K = shape
    rng = np.random.default_rng(M * 13 + N * 5 + K + 2 * ta + tb)
    A, B, C0 = _operands(rng, M, N, K, ta, tb, integer=False)
    rows, cols = dr.edge_indices(M, extra=16, seed=1), dr.edge_indices(N, extra=16, seed=2)
    worst = 0.0
    for alpha, beta in [(0.7, 0.7), (1.3, -1.3), (1.1, 0.0)]:
        c0 = C0 if beta != 0.0 else np.full((M, N), np.nan)
        ref, bound = dr.gemm_reference(A, B, c0, alpha, beta, ta, tb, rows, cols)
        outs = [host(e.dgemm(A, B, bool(ta), bool(tb), alpha=alpha, beta=beta, C_out=e.dev(c0)))
                for e in _engines(cfg, eng, eng8)]
        assert np.isfinite(outs[0]).all()
        ratio, _ = dr.gemm_errors(outs[0][np.ix_(rows, cols)], ref, bound)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (alpha, beta, ratio)
        for o in outs[1:]:
            assert np.array_equal(o, outs[0]), "GCBig and GCBig16 differ"
    print(f"dgemm {cfg} {shape} t{ta}{tb}: worst |C - C_ref| / bound = {worst:.3g}")


def _raw_dgemm(e, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, Cv, ldc):
    return e.lib.ppbo_dgemm(e.ctx, int(ta), int(tb), M, N, K, float(alpha), C.c_void_p(A.data_ptr()), int(lda),
                            C.c_void_p(B.data_ptr()), int(ldb), float(beta), C.c_void_p(Cv.data_ptr()), int(ldc),
                            e._stream())


def _last_error(e):
    buf = C.create_string_buffer(512)
    e.lib.ppbo_last_error(e.ctx, buf, 512)
    return buf.value.decode()


@pytest.mark.parametrize("M,N", [(1, 1), (200, 190), (4097, 4095)])
@pytest.mark.parametrize("ta,tb", TRANS)
def test_dgemm_k0_scales_c(eng, M, N, ta, tb):
    """K = 0: C = beta C exactly (alpha = -beta: the preload branch; alpha = 1: the epilogue's beta C), and C = 0 for
    beta = 0 even where C held NaN.  A and B are never read (one-element buffers)."""
    import torch
    rng = np.random.default_rng(M + N + ta + tb)
    dummy = torch.zeros(1, dtype=torch.float64, device=eng.device)
    lda, ldb = (M if ta else 1), (1 if tb else N)
    for alpha, beta in [(0.75, -0.75), (1.0, -0.3), (1.0, 0.0)]:
        c0 = rng.standard_normal((M, N)) if beta != 0.0 else np.full((M, N), np.nan)
        Cd = eng.dev(c0)
        assert _raw_dgemm(eng, ta, tb, M, N, 0, alpha, dummy, lda, dummy, ldb, beta, Cd, N) == 0, _last_error(eng)
        ref = beta * c0 if beta != 0.0 else np.zeros((M, N))
        assert np.array_equal(host(Cd), ref)


@pytest.mark.parametrize("cfg,shape,pads", [("tiny", (200, 190, 129), (3, 5, 7)), ("small", (1300, 1201, 259), (3, 5, 7)),
                                            ("big", (4097, 4095, 257), (3, 5, 7)), ("big", (4096, 4096, 256), (16, 8, 2))])
@pytest.mark.parametrize("ta,tb", TRANS)
def test_dgemm_strided_views(eng, cfg, shape, pads, ta, tb):
    """A, B and C as views into larger buffers (lda, ldb, ldc longer than the row; odd pads take the guarded loads,
    even ones on whole-chunk K the lean loop).  The buffers' padding columns and extra last row hold NaN in A and B (a
    read outside the view poisons C) and a sentinel in C (a write outside the view is seen).  Exact integer operands:
    the view must equal NumPy's product bit for bit."""
    import torch
    M, N, K = shape
    assert _config(M, N, K) == cfg
    rng = np.random.default_rng(M + 3 * N + K + 2 * ta + tb)
    A, B, C0 = _operands(rng, M, N, K, ta, tb, integer=True)
    pa, pb, pc = pads

    def embed(X, pad, fill):
        buf = np.full((X.shape[0] + 1, X.shape[1] + pad), fill)
        buf[:X.shape[0], :X.shape[1]] = X
        return torch.as_tensor(buf, device=eng.device)

    Ab, Bb, Cb = embed(A, pa, np.nan), embed(B, pb, np.nan), embed(C0, pc, 12345.0)
    before = host(Cb)
    alpha, beta = 1.5, -0.5
    rc = _raw_dgemm(eng, ta, tb, M, N, K, alpha, Ab, Ab.stride(0), Bb, Bb.stride(0), beta, Cb, Cb.stride(0))
    assert rc == 0, _last_error(eng)
    after = host(Cb)
    ref = alpha * (dr.op(A, ta) @ dr.op(B, tb)) + beta * C0
    assert np.array_equal(after[:M, :N], ref)
    outside = np.ones(after.shape, dtype=bool)
    outside[:M, :N] = False
    assert np.array_equal(after[outside], before[outside])


def test_dgemm_rejects_short_leading_dimensions(eng):
    """lda < (transA ? M : K), ldb < (transB ? K : N) or ldc < N is "invalid argument" and C is left alone; the ctx
    serves the next valid call."""
    import torch
    M, N, K = 70, 50, 40
    rng = np.random.default_rng(5)
    for ta, tb in TRANS:
        A, B, C0 = _operands(rng, M, N, K, ta, tb, integer=True)
        Ad, Bd = eng.dev(A), eng.dev(B)
        lda, ldb, ldc = (M if ta else K), (K if tb else N), N
        for bad in [(lda - 1, ldb, ldc), (lda, ldb - 1, ldc), (lda, ldb, ldc - 1), (0, ldb, ldc)]:
            Cd = eng.dev(C0)
            rc = _raw_dgemm(eng, ta, tb, M, N, K, 1.0, Ad, bad[0], Bd, bad[1], 0.0, Cd, bad[2])
            assert rc < 0, (ta, tb, bad)
            msg = _last_error(eng)
            assert "invalid argument" in msg and "leading dimension" in msg, msg
            assert np.array_equal(host(Cd), C0)
        Cd = eng.dev(C0)
        assert _raw_dgemm(eng, ta, tb, M, N, K, 1.0, Ad, lda, Bd, ldb, 1.0, Cd, ldc) == 0, _last_error(eng)
        assert np.array_equal(host(Cd), dr.op(A, ta) @ dr.op(B, tb) + C0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the consumers at the sizes of the 128 x 128 tiles
_CPU = {}


def _cpu_fixture(name):
    """The CPU posterior of a fixture's model at its f_MAP (cached for the module)."""
    if name not in _CPU:
        g = load_golden(name)
        _CPU[name] = (g, dr.CpuModel(g["X"], g["theta"], str(g["kernel"]), int(g["m"]), g["fMAP"]))
    return _CPU[name]


def _device_posterior(eng, g, form=None):
    """The device posterior of a fixture from the device's own Gram and inverse (no CPU intermediate)."""
    X, th, kern = g["X"], g["theta"], str(g["kernel"])
    Sinv = eng.pd_inverse(eng.gram(X, th, kern))
    return eng.posterior(X, th, kern, Sinv, g["fMAP"], int(g["m"]), form=form)


# c3 in the form its shape selects (edge: Y = H E, H lower triangular), c4 in node form (Y = G K* with the block-
# triangular K limit, khi_mode 1); c4's own choice would be the edge form too
FORMS = [("c3", None, 1), ("c4", 0, 0)]


# 35 000 points: 274 column tiles in chunks of 69, the last one 67 wide.  (The library scores at most 512 lines per
# Y product: 514 lines would be 512 in four equal chunks of 70 and a 2-line product on the small tiles.)
LINE_B, LINE_G, LINE_S = 500, 70, 128


def _line_batch(D, seed):
    rng = np.random.default_rng(seed)
    xis = np.eye(D)[rng.integers(0, D, LINE_B)]
    xs = rng.random((LINE_B, D)) * (xis == 0)
    al = np.sort(np.clip(np.linspace(0.005, 0.995, LINE_G) + rng.normal(0, 0.01, (LINE_B, LINE_G)), 0, 1), axis=1)
    z = rng.standard_normal((LINE_S, LINE_G))
    return xis, xs, al, z


@pytest.mark.parametrize("name,form,expect", FORMS)
def test_line_acq_big_tiles_vs_cpu(eng, name, form, expect):
    """EI and varmax of a 500-line batch (Y = G K* on the 128 x 128 tiles: 16 (c3) / 8 (c4) row tiles x 274 column
    tiles, chunks of 69 with a ragged last one) on ~64 lines -- the first, the last, every line across a chunk boundary
    (also of PPBO_LINE_Y_CHUNK = 7) and lines across column-tile boundaries -- against orc.line_ei / orc.line_varmax of
    the CPU posterior on the same draws, with test_pipeline_general_m_vs_oracle's tolerances
    (EI 1e-6 max(|EI|, 1e-3 sigma_f), varmax 1e-5 max(|varmax|, 1e-6 sigma_f^2)).  Measured: EI 6.5e-10 (c3) /
    4.8e-9 (c4), varmax 1.1e-9 / 7.7e-10."""
    g, cpu = _cpu_fixture(name)
    post = _device_posterior(eng, g, form)
    assert post.form == expect
    D, sf = int(g["D"]), float(g["theta"][2])
    xis, xs, al, z = _line_batch(D, seed=7)
    assert (LINE_B * LINE_G + 127) // 128 % dr.line_y_chunk(LINE_B * LINE_G) != 0      # the last chunk is ragged
    mustar, jit = float(np.max(g["mu"])), 1e-9 * sf ** 2
    ei, vm = eng.line_acq_xi(post, xis, xs, al, z, mustar, jitter=jit)
    ei, vm = host(ei), host(vm)
    lines = dr.line_picks(LINE_B, LINE_G, chunk_tiles=(dr.line_y_chunk(LINE_B * LINE_G), 7), seed=3)
    e0, v0 = cpu.line_acq(xis, xs, al, z, mustar, jit, lines)
    de = np.abs(ei[lines] - e0) / np.maximum(np.abs(e0), 1e-3 * sf)
    dv = np.abs(vm[lines] - v0) / np.maximum(np.abs(v0), 1e-6 * sf ** 2)
    print(f"{name}: {len(lines)} lines, worst EI error {de.max():.2e} (bound 1e-6), varmax {dv.max():.2e} (bound 1e-5)")
    assert de.max() <= 1e-6
    assert dv.max() <= 1e-5


@pytest.mark.parametrize("name,form,expect", FORMS)
def test_line_acq_bits_do_not_depend_on_the_tile_walk(eng, name, form, expect):
    """The same batch on engines with PPBO_LINE_Y_CHUNK = 1, 7, 300 (one chunk) and with PPBO_GEMM_BIG16=0 gives the
    default engine's bits: chunking only reorders the output tiles, and a tile's K sum does not depend on the
    wavefront layout."""
    g, _ = _cpu_fixture(name)
    post = _device_posterior(eng, g, form)
    assert post.form == expect
    xis, xs, al, z = _line_batch(int(g["D"]), seed=7)
    mustar, jit = float(np.max(g["mu"])), 1e-9 * float(g["theta"][2]) ** 2
    ref = [host(t) for t in eng.line_acq_xi(post, xis, xs, al, z, mustar, jitter=jit)]
    for env in [dict(PPBO_LINE_Y_CHUNK=1), dict(PPBO_LINE_Y_CHUNK=7), dict(PPBO_LINE_Y_CHUNK=300),
                dict(PPBO_GEMM_BIG16=0)]:
        e = _engine(**env)
        try:
            out = [host(t) for t in e.line_acq_xi(post, xis, xs, al, z, mustar, jitter=jit)]
        finally:
            e.close()
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]), env


@pytest.mark.parametrize("name,form,expect", FORMS)
def test_predict_cov_big_tiles_vs_cpu(eng, name, form, expect):
    """predict_cov at M = 4096 (K*' Lambda K* and (G K*)'(G K*) on 32 x 32 tiles of 128): the mean of every point and
    the covariance on every row / column at a 32-tile edge plus the last 128-tile, against the CPU posterior:
    mean 1e-6 relative (max norm), covariance 1e-6 sigma_f^2 (test_predict_cov_line_vs_reference's bounds).  Measured:
    mean 5.8e-9 (c3) / 5.9e-8 (c4), covariance 2.6e-11 / 2.6e-9 sigma_f^2."""
    g, cpu = _cpu_fixture(name)
    post = _device_posterior(eng, g, form)
    assert post.form == expect
    M = 4096
    Xc = np.random.default_rng(9).random((M, int(g["D"])))
    mu, cov = eng.predict_cov(post, Xc)
    mu, cov = host(mu), host(cov)
    idx = dr.edge_indices(M, extra=32, seed=4)
    mu0 = cpu.mean(Xc)
    cov0 = cpu.cov_entries(Xc, idx, idx)
    sf2 = float(g["theta"][2]) ** 2
    dmu = np.abs(mu - mu0).max() / np.abs(mu0).max()
    dcov = np.abs(cov[np.ix_(idx, idx)] - cov0).max() / sf2
    print(f"{name}: predict_cov M = {M}: mean {dmu:.2e} (bound 1e-6), covariance {dcov:.2e} sigma_f^2 (bound 1e-6)")
    assert dmu <= 1e-6
    assert dcov <= 1e-6


def _synthetic_se(n_q, m, D=10, seed=12):
    """An SE model on uniform random rows in [0, 1]^10 (l = 0.25, sigma = 0.5, f ~ N(0, 0.1^2)): Sigma^-1 - Lambda has
    kappa_1 ~ 3e2, so a relative bound on P of N u kappa_1 ~ 1e-10 means something (the recipe's line designs put
    pseudo-observations next to their observation: kappa_1 ~ 1e6 whatever the length scale)."""
    th = [0.5, 0.25, 1.0]
    rng = np.random.default_rng(seed)
    X = rng.random((n_q * (m + 1), D))
    f = rng.normal(0.0, 0.1, X.shape[0])
    return X, th, f


@pytest.mark.parametrize("n_q,m", [(128, 31), (100, 40)])        # N = 4096 and N = 4100 (33 row tiles of 128)
def test_posterior_P_big_tiles_vs_cpu(eng, eng8, n_q, m):
    """P = R'R of ppbo_posterior on the 128 x 128 tiles against the CPU's (Sigma^-1 - Lambda)^-1, the device fed the
    CPU's Sigma^-1 so that only the posterior's own factor and products are compared: max |P - P0| <= N u kappa_1 max|P0|
    with kappa_1 = ||Sigma^-1 - Lambda||_1 ||P0||_1 (a backward-stable inverse).  GCBig gives GCBig16's bits.  Measured:
    1.2e-14 against a bound of 1.5e-10 at both sizes."""
    X, th, f = _synthetic_se(n_q, m)
    cpu = dr.CpuModel(X, th, "SE_kernel", m, f)
    N = X.shape[0]
    Sinv = eng.dev(cpu.Sinv)
    post = eng.posterior(X, th, "SE_kernel", Sinv, f, m, want_P=True)
    P = host(post.P)
    Mq = cpu.Sinv - cpu.lam
    kappa = np.abs(Mq).sum(axis=0).max() * np.abs(cpu.P).sum(axis=0).max()
    err = np.abs(P - cpu.P).max() / np.abs(cpu.P).max()
    print(f"P at N = {N}: max|P - P0| / max|P0| = {err:.2e}, bound N u kappa_1 = {N * U * kappa:.2e} (kappa_1 {kappa:.2e})")
    assert err <= N * U * kappa
    post8 = eng8.posterior(X, th, "SE_kernel", Sinv, f, m, want_P=True)
    assert np.array_equal(host(post8.P), P)


def test_posterior_P_c5_residual(eng):
    """c5 (camphor-copper, N = 4096): the device's P from the CPU's Sigma^-1 satisfies the normwise residual bound of
    an inverse through a Cholesky factor, max |(Sigma^-1 - Lambda) P - I| <= N u ||Sigma^-1 - Lambda||_inf ||P||_inf,
    both sides on the CPU.  Measured: 7.1e-8 against 2.2e-5."""
    g, cpu = _cpu_fixture("c5")
    N = g["X"].shape[0]
    post = eng.posterior(g["X"], g["theta"], str(g["kernel"]), eng.dev(cpu.Sinv), g["fMAP"], int(g["m"]), want_P=True)
    P = host(post.P)
    Mq = cpu.Sinv - cpu.lam
    res = np.abs(Mq @ P - np.eye(N)).max()
    bound = N * U * np.abs(Mq).sum(axis=1).max() * np.abs(P).sum(axis=1).max()
    print(f"c5: max|(Sigma^-1 - Lambda) P - I| = {res:.2e}, bound {bound:.2e}")
    assert res <= bound


@pytest.fixture(scope="module")
def syrk_engines(eng):
    es = {0: eng}
    for cfg in (1, 2, 3):
        es[cfg] = _engine(PPBO_SYRK_CFG=cfg)
    yield es
    for cfg in (1, 2, 3):
        es[cfg].close()


@pytest.mark.parametrize("N", [3072, 3073, 4096, 5761])
def test_pd_inverse_every_syrk_config(syrk_engines, N):
    """pd_inverse's Sigma^-1 = Linv' Linv through every SYRK configuration (default by size -- GCTiny to 3072, GCSmall
    lower_only to 5760, GCBig16 from 5761 -- and PPBO_SYRK_CFG = 1 / 2 / 3: 128 / 64 / 32 tiles) on A = S + 2.5 I,
    S symmetric with spectrum in [-2, 2] (kappa(A) <= 9): max |A A^-1 - I| <= kappa N u on every column at a 32-tile
    edge plus the last 128-tile, the symmetry bound of test_potrf_and_inverse, and every configuration within
    2 kappa N u max|A^-1| of the default.  (Not bitwise: under klo_mode the first k depends on the tile size.)
    Measured: residual <= 1.2e-14 against >= 3.1e-12; the configurations happened to agree bit for bit."""
    rng = np.random.default_rng(N)
    S = rng.standard_normal((N, N))
    A = (S + S.T) / np.sqrt(8.0 * N) + 2.5 * np.eye(N)
    kappa = 9.0
    cols = dr.edge_indices(N, extra=32, seed=N)
    inv, worst = {}, [0.0, 0.0]
    for cfg, e in syrk_engines.items():
        Ai = host(e.pd_inverse(A))
        res = np.abs(A @ Ai[:, cols] - np.eye(N)[:, cols]).max()
        assert res <= kappa * N * U, (cfg, res)
        assert np.abs(Ai - Ai.T).max() <= 1e-12 * np.abs(Ai).max(), cfg
        inv[cfg] = Ai
        worst[0] = max(worst[0], res)
    scale = np.abs(inv[0]).max()
    for cfg in (1, 2, 3):
        d = np.abs(inv[cfg] - inv[0]).max()
        assert d <= 2 * kappa * N * U * scale, (cfg, d)
        worst[1] = max(worst[1], d / scale)
    print(f"pd_inverse N = {N}: residual {worst[0]:.2e} (bound {kappa * N * U:.2e}), configurations apart "
          f"{worst[1]:.2e} (bound {2 * kappa * N * U:.2e})")


def test_evidence_grad_at_n4096_vs_restatement(eng):
    """evidence_grad at N = 4096 (its A^-1 product on GCBig16) against the NumPy restatement at the device's f_MAP, with
    test_gradient_matches_the_restatement's tolerance (1e-7 per component, relative to max(|g_i|, 1e-3 max|g|)) and the
    same sign s_U.  Measured: 3.9e-15."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    D, m, n_q = 8, 31, 128
    th = [1.0, 0.25, 1.5]
    X = np.random.default_rng(17).random((n_q * (m + 1), D))
    st = PPBO_settings(D=D, bounds=((0, 1),) * D, xi_acquisition_function="EI-EXT-FAST", kernel="SE_kernel", m=m,
                       theta_initial=th, verbose=False)
    gp = GPModel(st)
    gp.X, gp.N = X, X.shape[0]
    gp._dX = gp.eng.dev(gp.X)
    gp.theta = th
    gp.update_Sigma(th)
    f0 = np.linalg.cholesky(eg.sigma_matrix(X, th, "SE_kernel")) @ np.random.RandomState(3).standard_normal(gp.N)
    _, g, _, sU, fm = gp.evidence_grad(th, f_initial=f0, gtol=1e-10)
    ref, sU_ref = eg.evidence_grad(X, th, "SE_kernel", m, host(fm).astype(float))
    rel = np.max(np.abs(g - ref) / np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(ref))))
    print(f"evidence_grad N = {gp.N}: worst component error {rel:.2e} (bound 1e-7)")
    assert sU == sU_ref
    assert rel <= 1e-7, (g, ref)
