"""CPU: the host half of the batched maximiser samples -- the weight draw Omega = omega_MAP + sqrt(cov) z, the per-sample
"best refined maximum, else redraw once" bookkeeping of Hsampler.sample_xstars (on a scripted stand-in for the engine),
its chunking, and the argument checks that run before anything reaches the device."""
import types

import numpy as np
import pytest

from ppbo_amd import random_fourier_sampler as rfs
from ppbo_amd.engine import RFF_MULTI_MAX_S, Engine


def test_omega_draws_host_restates_the_draw():
    om, cov = np.array([1.0, -2.0, 0.5]), np.array([4.0, 0.25, 1.0])
    z = np.array([[1.0, -1.0, 0.0], [0.5, 2.0, -3.0]])
    want = np.array([[3.0, -2.5, 0.5], [2.0, -1.0, -2.5]])
    assert np.array_equal(rfs.omega_draws_host(om, cov, z), want)


def test_best_per_sample():
    inf = np.inf
    x = np.arange(4 * 3 * 2, dtype=float).reshape(4, 3, 2)
    val = np.array([[1.0, 3.0, 2.0],          # best row 1
                    [5.0, 9.0, -inf],         # found = 1: row 1 does not count
                    [np.nan, -inf, -inf],     # nothing finite
                    [-1.0, -0.5, 7.0]])       # found = 0
    found = np.array([3, 1, 1, 0])
    X, V, missing = rfs.best_per_sample(x, val, found)
    assert np.array_equal(missing, [2, 3])
    assert np.array_equal(V[:2], [3.0, 5.0]) and np.all(np.isnan(V[2:]))
    assert np.array_equal(X[0], x[0, 1]) and np.array_equal(X[1], x[1, 0]) and np.all(np.isnan(X[2:]))


class _ScriptedEngine:
    """Stands in for the device: omega draws are rows of a counter, a search answers from `plan` (sample -> found)."""

    def __init__(self, D, K, plan):
        self.D, self.K, self.plan, self.calls, self.draws = D, K, plan, [], 0

    def dev(self, a):
        return np.asarray(a, dtype=float)

    def rff_omega_draws(self, seed, om, cov, n):
        out = 1000.0 * (self.draws + np.arange(n))[:, None] + np.zeros((n, len(om)))
        self.draws += n
        return out

    def rff_search_multi(self, cand, W, b, sf, omegas, K, iters):
        S = omegas.shape[0]
        self.calls.append(omegas[:, 0].copy())
        x = np.full((S, K, self.D), 0.5)
        val = np.full((S, K), -np.inf)
        found = np.zeros(S, dtype=np.int32)
        for s in range(S):
            tag = omegas[s, 0]
            if self.plan(tag):
                found[s] = 2
                val[s, :2] = [tag, tag + 1.0]
                x[s, 1] = tag
        return x, val, found


def _hs(plan, F=4, D=2):
    hs = rfs.Hsampler.__new__(rfs.Hsampler)
    hs.kernel, hs.nFeatures, hs.D, hs.theta = "SE_kernel", F, D, [0.1, 0.3, 1.0]
    hs.W, hs.b = np.ones((F, D)), np.zeros((F, 1))
    hs.omega_MAP, hs.cov_diag = np.zeros(F), np.ones(F)
    hs.eng = _ScriptedEngine(D, rfs.RFF_STARTS, plan)
    hs._dcache, hs.camphor_l = {}, None
    hs._xstar_candidates = lambda: np.zeros((8, D))
    return hs


def test_sample_xstars_bookkeeping_redraws_once():
    # the draws are tagged 0, 1000, 2000, ...: sample 1 (tag 1000) finds nothing, its redraw (tag 3000) does
    hs = _hs(lambda tag: tag != 1000.0)
    X, V = hs.sample_xstars(3, seed=7)
    assert np.array_equal(V, [1.0, 3001.0, 2001.0])
    assert np.array_equal(X[:, 0], [0.0, 3000.0, 2000.0])
    assert len(hs.eng.calls) == 2 and np.array_equal(hs.eng.calls[1], [3000.0])


def test_sample_xstars_raises_after_a_failed_redraw():
    hs = _hs(lambda tag: tag < 1000.0)
    with pytest.raises(RuntimeError):
        hs.sample_xstars(2, seed=7)


def test_sample_xstars_chunks(monkeypatch):
    monkeypatch.setattr(rfs, "RFF_MULTI_MAX_S", 3)
    hs = _hs(lambda tag: True)
    om = 1000.0 * np.arange(7)[:, None] + np.zeros((7, 4))
    X, V = hs.sample_xstars(7, omegas=om)
    assert [len(c) for c in hs.eng.calls] == [3, 3, 1]
    assert np.array_equal(V, 1000.0 * np.arange(7) + 1.0)


def test_sample_xstars_argument_checks():
    hs = _hs(lambda tag: True)
    with pytest.raises(ValueError):
        hs.sample_xstars(0)
    with pytest.raises(ValueError):
        hs.sample_xstars(3, omegas=np.zeros((3, 5)))       # width != F
    hs.cov_diag = None
    with pytest.raises(RuntimeError):
        hs.sample_omegas(2, seed=1)


def test_engine_validates_before_the_device():
    eng = Engine.__new__(Engine)                            # no context: any device call would fail differently
    rng = np.random.default_rng(0)
    M, D, F = 16, 3, 8
    cand, W, b, om = rng.random((M, D)), rng.random((F, D)), rng.random(F), rng.random((2, F))
    bad = [dict(omegas=np.zeros((0, F))), dict(omegas=np.zeros((RFF_MULTI_MAX_S + 1, F))), dict(K=0), dict(K=1025),
           dict(omegas=np.zeros((2, F + 1))), dict(W=rng.random((F, D + 1))), dict(b=rng.random(F - 1)),
           dict(cand=rng.random((M, 65)), W=rng.random((F, 65)))]
    for kw in bad:
        args = dict(cand=cand, W=W, b=b, sigma_f=0.5, omegas=om)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.rff_search_multi(**args)
    with pytest.raises(ValueError):                         # camphor: W must be [F, 11], the candidates [M, 6]
        eng.rff_search_multi_camphor(rng.random((M, 6)), np.full(6, 0.3), rng.random((F, 6)), b, 0.5, om)
    with pytest.raises(ValueError):
        eng.rff_search_multi_camphor(rng.random((M, 5)), np.full(6, 0.3), rng.random((F, 11)), b, 0.5, om)
    with pytest.raises(ValueError):
        eng.rff_score_multi(cand, W, b, 0.5, np.zeros((0, F)))
    assert Engine._rff_multi_widths("t", D, W, b, om, 32) == (F, 2)
