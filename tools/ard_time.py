#!/usr/bin/env python3
"""Scalar length scale against per-dimension length scales (ARD) on the same inputs, in one process, alternating
(scalar ARD scalar ARD ...) so that clock drift falls on both.

  C3 scoring step (N = 2048, D = 20, 65536 candidates, EI: K*, contraction, score, argmax)   wall clock of
      Engine.predict, synchronised; ARD adds one ppbo_scale_points pass over the candidates
  mu_star's device search at C3 (Engine.mean_search_multi: 3 trials over the 65536-row pool, the design and x_prev,
      32 ascents per trial, fp32 screening)   wall clock; ARD = ppbo_mean_search_multi on a PPBO_COORDS_SCALED model
  its ascent alone (Engine.mean_ascent from 96 fixed starts, 100 iterations at most)   wall clock
  one fit at C3 (Engine.gp_fit from the stored start)   wall clock; ARD adds the scaling of the design

The C3 design is that of tests/golden/c3.npz.  ARD runs twice: with D equal entries l_d = l (the scalar model through
the ARD path: what the path itself costs) and with l_d spread geometrically over 20x around l (another landscape: the
ascents of mu_star see another conditioning).  Output: one line per quantity, medians in ms, ratios to the scalar
run and the (min-max) over the rounds.

usage: python tools/ard_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ppbo_amd.engine import SCORE_POINTWISE_EI, get_engine  # noqa: E402


def wall_ms(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main(rounds=5, out_file=None):
    eng = get_engine(0)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    c3 = dict(np.load(os.path.join(root, "c3.npz")))
    X, m, th = c3["X"], int(c3["m"]), [float(t) for t in c3["theta"]]
    D = X.shape[1]
    l_ard = th[1] * np.geomspace(0.2, 4.0, D)
    # "ARD =": equal entries, the scalar model's landscape through the ARD path (the path's own cost); "ARD": a spread of
    # 20x, a different (more anisotropic) landscape
    thetas = {"scalar": th, "ARD =": [th[0], np.full(D, th[1]), th[2]], "ARD": [th[0], l_ard, th[2]]}
    rng = np.random.default_rng(1)
    Xc = eng.dev(rng.random((65536, D)))
    pool = eng.dev(rng.random((65536, D)))
    shifts = rng.random((3, D))
    xprev = X[0].copy()
    starts = rng.random((96, D))
    posts = {}
    for k, t in thetas.items():
        r = eng.gp_fit(X, t, "SE_kernel", m, c3["f_init"])
        posts[k] = eng.posterior(X, t, "SE_kernel", r["Sigma_inv"], c3["fMAP"], m)
    mustar = float(np.max(c3["mu"]))
    cases = [
        ("C3 scoring step (Engine.predict, wall)", lambda k: wall_ms(lambda: eng.predict(
            posts[k], Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_var=False, want_mu=False), reps=20)),
        ("mu_star search at C3 (mean_search_multi, 3 trials, wall)", lambda k: wall_ms(lambda: eng.mean_search_multi(
            posts[k], pool, shifts, "design", xprev, K=32), reps=5)),
        ("mu_star ascent alone at C3 (mean_ascent, 96 fixed starts, wall)", lambda k: wall_ms(lambda: eng.mean_ascent(
            posts[k], starts, iters=100), reps=5)),
        ("fit at C3 (Engine.gp_fit, wall)", lambda k: wall_ms(lambda: eng.gp_fit(
            X, thetas[k], "SE_kernel", m, c3["f_init"]), reps=5)),
    ]
    lines = [f"device: {torch.cuda.get_device_name(0)}; {rounds} alternating rounds per quantity; medians in ms"]
    print(lines[0], flush=True)
    for name, fn in cases:
        t = {k: [] for k in thetas}
        for _ in range(rounds):
            for k in thetas:
                t[k].append(fn(k))
        med = {k: float(np.median(v)) for k, v in t.items()}
        a = med["scalar"]
        ln = f"{name:58s} " + "  ".join(f"{k} {med[k]:7.4f} ({med[k] / a:5.3f}x; {min(t[k]):.4f}-{max(t[k]):.4f})"
                                        for k in thetas)
        lines.append(ln)
        print(ln, flush=True)
    if out_file:
        with open(out_file, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else None)
