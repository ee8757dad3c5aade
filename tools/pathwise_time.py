#!/usr/bin/env python3
"""Hsampler.sample_xstars(256, posterior="pathwise") against sample_xstars(256) -- the weight-space posterior with its
diagonal covariance -- on one device, in one process, alternating (weights, pathwise, weights, ...) so that clock drift
falls on both.

  C2 (tests/golden/c2.npz: N = 512, D = 6), F = 1000;   C3 (tests/golden/c3.npz: N = 2048, D = 20), F = 4096;   SE_kernel

  weights   sample_xstars(256): device draws of omega, rff_score_multi, selection, 256 x 32-start ascent
  pathwise  sample_xstars(256, posterior="pathwise") = sample_paths(256) + PosteriorPaths.xstars()
  setup     sample_paths(256) alone: the draws, one factorization of P, three GEMMs
  score     Engine.path_score_multi / rff_score_multi alone over the 65536-row pool (inner dimension F + N against F)
  search    Engine.path_search_multi / rff_search_multi alone (score + selection + ascent)

and, for the paths of each configuration: |v_s| / |alpha| (median over the paths), the cancellation
sum_i |v_i k_i| / |sum_i v_i k_i| (median over 50 paths x 200 uniform points), and ppbo_path_score_multi's error measure
(max |device - NumPy| / max sum of absolute terms) on 8 paths x 4096 pool rows.

Per-kernel times come from a run of its own under the profiler, which times only the pathwise call at C3:

  rocprofv3 --kernel-trace --stats -d <dir> -o pw -- python tools/pathwise_time.py --profile

usage: python tools/pathwise_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ppbo_amd.engine import get_engine  # noqa: E402
from ppbo_amd.random_fourier_sampler import Hsampler  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_PATHS = 256


def _sampler(eng, name, F):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    X, m, kern = g["X"], int(g["m"]), "SE_kernel"
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(X, th, kern, m, g["f_init"], gtol=1e-6)
    post = eng.posterior(X, th, kern, r["Sigma_inv"], r["fMAP"], m, want_P=True)
    loc = g["Xc"][np.argsort(g["mu"])[-4:]]
    gp = types.SimpleNamespace(eng=eng, D=X.shape[1], m=m, X=X, xstar=loc[-1], xstars_local=loc,
                               n_gausshermite_sample_points=None, obs_indices=np.arange(0, X.shape[0], m + 1),
                               kernel=types.SimpleNamespace(__name__=kern), theta=th, _dSigma_inv=r["Sigma_inv"],
                               Sigma_inv=None, fMAP=r["fMAP"].cpu().numpy(), posterior_covariance=post.P, _post=post)
    hs = Hsampler(gp, F)
    np.random.seed(1)
    hs.generate_basis()
    hs.update_phi_X()
    hs.update_omega_MAP()
    hs.update_covariancematrix()
    hs.sample_xstars(8)                                   # warm: workspaces, the resident pool
    hs.sample_xstars(8, posterior="pathwise")
    return hs, post


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _conditioning(eng, hs, post, paths, out):
    import pathwise_numpy as pw
    V, Wp = paths.V.cpu().numpy(), paths.W_prior.cpu().numpy()
    alpha = post.alpha.cpu().numpy()
    out(f"    |v_s| / |alpha|: median {np.median(np.linalg.norm(V, axis=1)) / np.linalg.norm(alpha):.3g}")
    Xq = np.random.default_rng(9).random((200, hs.D))
    K, _ = pw.kernel_matrix(Xq, hs.X, hs.theta, hs.kernel)
    kv, akv = V[:50] @ K.T, np.abs(V[:50]) @ K.T
    out(f"    cancellation sum |v_i k_i| / |sum v_i k_i|: median {np.median(akv / np.abs(kv)):.3g}")
    pool = hs._xstar_candidates()[:4096]
    got = eng.path_score_multi(pool, hs._dev("W"), hs._dev("b"), hs.theta, hs.kernel, hs._dev("X"), paths.W_prior[:8],
                               paths.V[:8]).cpu().numpy()
    xs = pool.cpu().numpy()
    want = pw.paths(xs, Wp[:8], V[:8], hs.W, hs.b, hs.X, hs.theta, hs.kernel)
    scale = pw.paths_abs(xs, Wp[:8], V[:8], hs.W, hs.b, hs.X, hs.theta, hs.kernel)
    out(f"    path_score_multi error measure (8 paths x 4096 rows): {(np.abs(got - want).max(axis=1) / scale.max(axis=1)).max():.3g}"
        f"   (against max |g_s|: {(np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max():.3g})")


def profile():
    eng = get_engine(0)
    hs, _ = _sampler(eng, "c3", 4096)
    for _ in range(3):
        hs.sample_xstars(N_PATHS, posterior="pathwise")
    torch.cuda.synchronize()


def main():
    if "--profile" in sys.argv:
        return profile()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    fh = open(args[1], "w") if len(args) > 1 else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    eng = get_engine(0)
    out(f"sample_xstars({N_PATHS}) against sample_xstars({N_PATHS}, posterior='pathwise'): median of {rounds} alternating rounds, ms")
    for name, F in (("c2", 1000), ("c3", 4096)):
        hs, post = _sampler(eng, name, F)
        N, D = hs.X.shape
        t = {k: [] for k in ("weights", "pathwise", "setup", "score_w", "score_p", "search_w", "search_p")}
        pool = hs._xstar_candidates()
        W, b, X = hs._dev("W"), hs._dev("b"), hs._dev("X")
        paths = hs.sample_paths(N_PATHS, seed=3)
        om = hs.sample_omegas(N_PATHS, seed=3)
        for _ in range(rounds):
            t["weights"].append(_ms(lambda: hs.sample_xstars(N_PATHS)))
            t["pathwise"].append(_ms(lambda: hs.sample_xstars(N_PATHS, posterior="pathwise")))
            t["setup"].append(_ms(lambda: hs.sample_paths(N_PATHS)))
            t["score_w"].append(_ms(lambda: eng.rff_score_multi(pool, W, b, hs.theta[2], om)))
            t["score_p"].append(_ms(lambda: eng.path_score_multi(pool, W, b, hs.theta, hs.kernel, X, paths.W_prior, paths.V)))
            t["search_w"].append(_ms(lambda: eng.rff_search_multi(pool, W, b, hs.theta[2], om, K=32, iters=100)))
            t["search_p"].append(_ms(lambda: eng.path_search_multi(pool, W, b, hs.theta, hs.kernel, X, paths.W_prior, paths.V,
                                                                  K=32, iters=100)))
        md = {k: float(np.median(v)) for k, v in t.items()}
        sp = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
        out(f"  {name}: N = {N}, D = {D}, F = {F}, (F + N) / F = {(F + N) / F:.2f}")
        out(f"    weights  {md['weights']:8.2f}  [{sp['weights'][0]:.2f} .. {sp['weights'][1]:.2f}]")
        out(f"    pathwise {md['pathwise']:8.2f}  [{sp['pathwise'][0]:.2f} .. {sp['pathwise'][1]:.2f}]   ratio {md['pathwise'] / md['weights']:.2f}")
        out(f"    setup (sample_paths alone) {md['setup']:8.2f}  = {100 * md['setup'] / md['pathwise']:.0f}% of pathwise")
        out(f"    score   weights {md['score_w']:7.2f}   pathwise {md['score_p']:7.2f}   ratio {md['score_p'] / md['score_w']:.2f}"
            f"   = {100 * md['score_p'] / md['search_p']:.0f}% of the pathwise search")
        out(f"    search  weights {md['search_w']:7.2f}   pathwise {md['search_p']:7.2f}   ratio {md['search_p'] / md['search_w']:.2f}"
            f"   (selection + ascent: {md['search_w'] - md['score_w']:.2f} -> {md['search_p'] - md['score_p']:.2f})")
        _conditioning(eng, hs, post, paths, out)
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
