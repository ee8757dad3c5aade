"""CPU: the sampled references of tests/dense_ref.py equal the full computation they stand for, on cases small enough
to form it whole (the GPU tests of test_gpu_dense_products.py evaluate them on subsets of much larger outputs)."""
import numpy as np
import pytest

import dense_ref as dr
from oracle import ppbo_oracle as orc


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 4095, 4097])
def test_edge_indices_hold_every_tile_edge(n):
    idx = dr.edge_indices(n, extra=5, seed=1)
    assert np.all(np.diff(idx) > 0) and idx[0] == 0 and idx[-1] == n - 1
    s = set(idx.tolist())
    for tile in (32, 64, 128):
        for t0 in range(0, n, tile):
            assert t0 in s and min(t0 + tile, n) - 1 in s
    assert set(range((n - 1) // 128 * 128, n)) <= s


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("alpha,beta", [(0.7, 0.7), (1.3, -1.3), (1.1, 0.0)])
def test_gemm_reference_is_the_dense_product(ta, tb, alpha, beta):
    """On the sampled entries the long-double reference equals NumPy's whole product within the bound, the bound holds
    NumPy's own product, and an error of a few ulps of the largest term breaks it."""
    M, N, K = 150, 140, 97
    rng = np.random.default_rng(3)
    A = rng.standard_normal((K, M) if ta else (M, K))
    B = rng.standard_normal((N, K) if tb else (K, N))
    C0 = rng.standard_normal((M, N)) if beta != 0.0 else np.full((M, N), np.nan)
    rows, cols = dr.edge_indices(M, extra=8), dr.edge_indices(N, extra=8, seed=2)
    ref, bound = dr.gemm_reference(A, B, C0, alpha, beta, ta, tb, rows, cols)
    full = alpha * (dr.op(A, ta) @ dr.op(B, tb)) + (beta * C0 if beta != 0.0 else 0.0)
    ratio, err = dr.gemm_errors(full[np.ix_(rows, cols)], ref, bound)
    assert ratio <= 0.25 and err > 0
    # integer operands: the reference is the exact product
    Ai, Bi = np.round(A * 4), np.round(B * 4)
    ref_i, _ = dr.gemm_reference(Ai, Bi, None, 1.0, 0.0, ta, tb, rows, cols)
    assert np.array_equal(ref_i.astype(np.float64), (dr.op(Ai, ta) @ dr.op(Bi, tb))[np.ix_(rows, cols)])
    # a wrong entry is seen: one skipped k term, or K u of the magnitude on one entry
    bad = full[np.ix_(rows, cols)].copy()
    bad[3, 5] -= alpha * dr.op(A, ta)[rows[3], K - 1] * dr.op(B, tb)[K - 1, cols[5]]
    assert dr.gemm_errors(bad, ref, bound)[0] > 1.0
    bad = full[np.ix_(rows, cols)].copy()
    bad[-1, -1] += 3 * bound[-1, -1]
    assert dr.gemm_errors(bad, ref, bound)[0] > 1.0


def _small_model(kernel="SE_kernel"):
    m, n_q, D = 5, 8, 3
    th = [0.3, 0.3, 0.7]
    X = orc.synthetic_design(n_q, D, m=m, seed=4)
    S0 = orc.gram(X, th, kernel)
    f = np.linalg.cholesky(S0) @ np.random.default_rng(5).standard_normal(X.shape[0]) * 0.1
    return dr.CpuModel(X, th, kernel, m, f)


@pytest.mark.parametrize("kernel", ["SE_kernel", "RQ_kernel"])
def test_cpu_model_is_the_oracle_chain(kernel):
    cpu = _small_model(kernel)
    Sinv0 = orc.pd_inverse(orc.gram(cpu.X, cpu.theta, kernel))
    P0 = orc.posterior_covariance(Sinv0, cpu.f, cpu.m, cpu.theta[0])
    assert np.array_equal(cpu.Sinv, Sinv0) and np.array_equal(cpu.P, P0)
    Xc = np.random.default_rng(6).random((40, 3))
    mu, var = cpu.mean_var(Xc)
    mu1, cov1 = orc.mu_sigma_pred(Xc, cpu.X, cpu.theta, cpu.Sinv, cpu.f, cpu.P, kernel, faithful=False, A=cpu.A)
    assert np.abs(mu - mu1).max() <= 1e-14 * np.abs(mu1).max()
    assert np.abs(var - np.diag(cov1)).max() <= 1e-13 * cpu.theta[2] ** 2
    assert np.abs(cpu.mean(Xc) - mu1).max() <= 1e-14 * np.abs(mu1).max()


@pytest.mark.parametrize("kernel", ["SE_kernel", "RQ_kernel"])
def test_cov_entries_are_the_oracles_covariance(kernel):
    """The sampled predictive covariance equals orc.mu_sigma_pred's whole M x M covariance on those entries (the
    shrink's tr(K)/M taken over all M points, the diagonal included)."""
    cpu = _small_model(kernel)
    M = 300
    Xc = np.random.default_rng(7).random((M, 3))
    rows, cols = dr.edge_indices(M, extra=10), dr.edge_indices(M, extra=10, seed=3)
    _, cov = orc.mu_sigma_pred(Xc, cpu.X, cpu.theta, cpu.Sinv, cpu.f, cpu.P, kernel, faithful=False, A=cpu.A)
    assert np.abs(cpu.cov_entries(Xc, rows, cols) - cov[np.ix_(rows, cols)]).max() <= 1e-14 * cpu.theta[2] ** 2


def test_line_reference_is_the_per_line_oracle():
    """line_acq on a subset of lines equals orc.line_ei / orc.line_varmax of each of those lines' own grid and
    orc.mu_sigma_pred covariance, for shared and per-line abscissae."""
    cpu = _small_model()
    B, G, D = 9, 20, 3
    rng = np.random.default_rng(8)
    xis = np.eye(D)[rng.integers(0, D, B)]
    xs = rng.random((B, D)) * (xis == 0)
    z = rng.standard_normal((50, G))
    jit = 1e-9 * cpu.theta[2] ** 2
    for al in (np.linspace(0.005, 0.995, G), np.sort(rng.random((B, G)), axis=1)):
        lines = np.array([0, 4, B - 1])
        ei, vm = cpu.line_acq(xis, xs, al, z, 0.1, jit, lines)
        for i, b in enumerate(lines):
            a = al[b] if al.ndim == 2 else al
            grid = a[:, None] * xis[b][None, :] + xs[b][None, :]
            mu, cov = orc.mu_sigma_pred(grid, cpu.X, cpu.theta, cpu.Sinv, cpu.f, cpu.P, "SE_kernel", faithful=False,
                                        A=cpu.A)
            assert ei[i] == orc.line_ei(mu, cov, z, 0.1, jitter=jit)
            assert vm[i] == orc.line_varmax(mu, cov, z, jitter=jit)


def test_line_chunking_and_picks():
    assert dr.line_y_chunk(512 * 70) == 70          # 280 tiles: four equal chunks
    assert dr.line_y_chunk(500 * 70) == 69          # 274 tiles: 69, 69, 69, 67
    assert dr.line_y_chunk(100) == 1
    lines = dr.line_picks(500, 70, chunk_tiles=(69, 7), n=64)
    assert lines[0] == 0 and lines[-1] == 499 and len(lines) >= 64
    for c in (69, 7):
        w = 128 * c
        for b in range(500):
            if (b * 70) // w != (b * 70 + 69) // w:
                assert b in lines
