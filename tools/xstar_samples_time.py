#!/usr/bin/env python3
"""Hsampler.sample_xstars(n) -- n posterior maximiser samples in batched enqueues -- against a loop of n sample_xstar()
calls, in one process, alternating (loop, batch, loop, batch, ...) so that clock drift falls on both.

  C3 (tests/golden/c3.npz: N = 2048, D = 20), F = 4096: SE_kernel and RQ_kernel features
  C5 (tests/golden/c5.npz: N = 4096, D = 6), F = 8192: camphor_copper_kernel features (W [F, 11])
  n in {32, 256, 1024}

  loop    n x (sample_omega + return_xstar): one score / select / 32-start ascent per sample, wall clock
  batch   sample_xstars(n): device draws, one multi-score, one selection and one S x 32-start ascent launch per call
  score   Engine.rff_score_multi alone over the same 65536-row pool for the n draws: wall clock, and the share of the
          fp64 matrix-core peak (78.6 TF) that 2 M F S flop in that time is

Every sampler is set up once (generate_basis, update_phi_X, update_omega_MAP, update_covariancematrix) and warmed.
Per-stage kernel times come from a run of its own under the profiler, which times only sample_xstars(256) at C3 SE:

  rocprofv3 --kernel-trace --stats -d <dir> -o xs -- python tools/xstar_samples_time.py --profile

usage: python tools/xstar_samples_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ppbo_amd.engine import get_engine  # noqa: E402
from ppbo_amd.random_fourier_sampler import Hsampler  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
PEAK_F64_MFMA = 78.6e12


def _sampler(eng, g, kernel, F):
    X, m = g["X"], int(g["m"])
    th = [float(t) for t in g["theta"]]
    loc = g["Xc"][np.argsort(g["mu"])[-4:]]
    gp = types.SimpleNamespace(eng=eng, D=X.shape[1], m=m, X=X, xstar=loc[-1], xstars_local=loc,
                               n_gausshermite_sample_points=None, obs_indices=np.arange(0, X.shape[0], m + 1),
                               kernel=types.SimpleNamespace(__name__=kernel), theta=th)
    hs = Hsampler(gp, F)
    np.random.seed(1)
    hs.generate_basis()
    hs.update_phi_X()
    hs.update_omega_MAP()
    hs.update_covariancematrix()
    hs.sample_xstar()                                     # warm: workspaces, the resident pool, the embedded rows
    hs.sample_xstars(8)
    return hs


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _score_ms(eng, hs, n, pool, reps=5):
    om = hs.sample_omegas(n, seed=3)
    X = pool if hs._camphor() is None else eng.camphor_embed(pool, hs._camphor())
    f = lambda: eng.rff_score_multi(X, hs._dev("W"), hs._dev("b"), hs.theta[2], om)  # noqa: E731
    f()
    return float(np.median([_ms(f) for _ in range(reps)])), X.shape[0]


def profile():
    eng = get_engine(0)
    g = dict(np.load(os.path.join(GOLDEN, "c3.npz")))
    hs = _sampler(eng, g, "SE_kernel", 4096)
    for _ in range(3):
        hs.sample_xstars(256)
    torch.cuda.synchronize()


def main(rounds=2, out_file=None):
    eng = get_engine(0)
    legs = [("C3 F=4096", "c3.npz", 4096, "SE_kernel"), ("C3 F=4096", "c3.npz", 4096, "RQ_kernel"),
            ("C5 F=8192", "c5.npz", 8192, "camphor_copper_kernel")]
    lines = [f"device: {torch.cuda.get_device_name(0)}; {rounds} rounds, medians in ms, (min-max) over the rounds"]
    for title, fx, F, kernel in legs:
        g = dict(np.load(os.path.join(GOLDEN, fx)))
        hs = _sampler(eng, g, kernel, F)
        pool = eng.dev(np.random.default_rng(2).random((65536, hs.D)))
        lines.append(f"{title} {kernel}")
        for n in (32, 256, 1024):
            loop, batch = [], []
            for _ in range(rounds):
                loop.append(_ms(lambda: [hs.sample_xstar() for _ in range(n)]))
                batch.append(_ms(lambda: hs.sample_xstars(n)))
            sc, M = _score_ms(eng, hs, n, pool)
            share = 2.0 * M * F * n / (sc * 1e-3) / PEAK_F64_MFMA
            lines.append(f"  n={n:5d}  loop {np.median(loop):9.2f} ({min(loop):.2f}-{max(loop):.2f})   batch "
                         f"{np.median(batch):8.2f} ({min(batch):.2f}-{max(batch):.2f})   speed-up "
                         f"{np.median(loop) / np.median(batch):6.1f}x   score_multi {sc:7.3f} ms = {share * 100:5.1f}% of "
                         "the fp64 MFMA peak (wall clock)")
    txt = "\n".join(lines)
    print(txt)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    if "--profile" in sys.argv:
        profile()
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 2, sys.argv[2] if len(sys.argv) > 2 else None)
