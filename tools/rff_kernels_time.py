#!/usr/bin/env python3
"""Hsampler with the camphor-copper and RQ bases against the SE basis on the same design, in one process, alternating
(SE, other, SE, other, ...) so that clock drift falls on both.

  C5 (tests/golden/c5.npz: N = 4096, D = 6, m = 31), F = 8192: camphor_copper_kernel features ([F, 11], embedded rows,
     ppbo_rff_search with the camphor coordinate map) against SE features ([F, 6], ppbo_rff_search) at the same theta
  C3 (tests/golden/c3.npz: N = 2048, D = 20), F = 4096: RQ features against SE features

  sample_xstar   Hsampler.sample_omega + return_xstar (score the rotated 65536-row pool plus the perturbed local maxima,
                 select 32 starts, 32 ascents of 100 iterations), wall clock to the host result
  screen+select  Engine.rff_search / rff_search_camphor over a 65536-row pool with iters = 0 (embedding, scoring, thinning,
                 start selection and the launch of the ascents that stop at once), wall clock
  ascent         the same search with iters = 100 minus the above: the 32 ascents
  cycle          generate_basis, update_phi_X, update_omega_MAP, update_covariancematrix, sample_xstar

Output: one line per quantity, medians in ms, the ratio to SE and the (min-max) over the rounds.

usage: python tools/rff_kernels_time.py [rounds] [out_file]
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


def _sampler(eng, g, kernel, F):
    X, m = g["X"], int(g["m"])
    th = [float(t) for t in g["theta"]]
    loc = g["Xc"][np.argsort(g["mu"])[-4:]]
    gp = types.SimpleNamespace(eng=eng, D=X.shape[1], m=m, X=X, xstar=loc[-1], xstars_local=loc,
                               n_gausshermite_sample_points=None, obs_indices=np.arange(0, X.shape[0], m + 1),
                               kernel=types.SimpleNamespace(__name__=kernel), theta=th)
    return Hsampler(gp, F)


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(eng, g, kernel, F, reps=5):
    hs = _sampler(eng, g, kernel, F)
    np.random.seed(1)

    def cycle():
        hs.generate_basis()
        hs.update_phi_X()
        hs.update_omega_MAP()
        hs.update_covariancematrix()
        hs.sample_xstar()

    cycle()                                               # warm: workspaces, the resident pool, the embedded rows
    out = {"cycle": float(np.median([_ms(cycle) for _ in range(reps)]))}
    out["sample_xstar"] = float(np.median([_ms(hs.sample_xstar) for _ in range(4 * reps)]))
    om = hs.sample_omega()
    pool = eng.dev(np.random.default_rng(2).random((65536, hs.D)))
    l = hs._camphor()

    def search(iters):
        if l is None:
            return lambda: eng.rff_search(pool, hs._dev("W"), hs._dev("b"), hs.theta[2], om, K=32, iters=iters)
        return lambda: eng.rff_search_camphor(pool, l, hs._dev("W"), hs._dev("b"), hs.theta[2], om, K=32, iters=iters)

    full = float(np.median([_ms(search(100)) for _ in range(4 * reps)]))
    screen = float(np.median([_ms(search(0)) for _ in range(4 * reps)]))
    out["ascent"] = full - screen
    out["screen+select"] = screen
    return out


def main(rounds=3, out_file=None):
    eng = get_engine(0)
    c5 = dict(np.load(os.path.join(GOLDEN, "c5.npz")))
    c3 = dict(np.load(os.path.join(GOLDEN, "c3.npz")))
    legs = [("C5 F=8192", c5, 8192, "SE_kernel", "camphor_copper_kernel"),
            ("C3 F=4096", c3, 4096, "SE_kernel", "RQ_kernel")]
    lines = [f"device: {torch.cuda.get_device_name(0)}; {rounds} rounds, medians in ms"]
    for title, g, F, base, other in legs:
        res = {base: [], other: []}
        for _ in range(rounds):
            for k in (base, other):
                res[k].append(measure(eng, g, k, F))
        lines.append(f"{title}: {other} against {base}")
        for q in ("sample_xstar", "screen+select", "ascent", "cycle"):
            a = [r[q] for r in res[base]]
            b = [r[q] for r in res[other]]
            lines.append(f"  {q:14s} {base} {np.median(a):8.3f} ({min(a):.3f}-{max(a):.3f})   {other} {np.median(b):8.3f} "
                         f"({min(b):.3f}-{max(b):.3f})   ratio {np.median(b) / np.median(a):.2f}")
    txt = "\n".join(lines)
    print(txt)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, sys.argv[2] if len(sys.argv) > 2 else None)
