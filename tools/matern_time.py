#!/usr/bin/env python3
"""SE against Matern-5/2 on the same inputs, in one process, alternating (A B A B ...) so that clock drift falls on both.

  Gram N = 2048 / 4096 (D = 20)    graph replay: 100 launches captured in a HIP graph, replayed back to back, the second
                                   half timed with one event pair (DESIGN_HISTORY "How short kernels are timed")
  K* at C3 (N = 2048, D = 20, 65536 candidates, EI)   per-kernel events (ppbo_profile "kstar"), as tools/kstar_time.py
  C3 scoring step (K*, contraction, score, argmax)     wall clock of ppbo_predict, synchronised, median of the rounds
  one-launch scorer at C2 (N = 512, D = 6)             per-kernel events ("fused_score")
  mu_star's device search at C3 (ppbo_mean_search, 65536 candidates, 32 ascents)   wall clock
  one fit at C3 (ppbo_gp_fit from the stored start)    wall clock

The C3 / C2 designs are those of tests/golden/c3.npz / c2.npz; both kernels see the same X, theta, candidates and the
same f_MAP (the timing does not depend on its values).  Output: one line per quantity, SE and Matern-5/2 medians in ms
and their ratio.

usage: python tools/matern_time.py [rounds]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ppbo_amd.engine import SCORE_POINTWISE_EI, get_engine  # noqa: E402

KERNELS = ("SE_kernel", "Matern52_kernel")


def graph_ms(fn, per_graph=100, replays=40):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for _ in range(per_graph):
                fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(replays):
        if r == replays // 2:
            e0.record()
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ((replays - replays // 2) * per_graph)


def event_ms(eng, name, fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, n = eng.profile_read(name)
    eng.profile(False)
    return ms / max(n, 1)


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


def main(rounds=5):
    eng = get_engine(0)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    c3 = dict(np.load(os.path.join(root, "c3.npz")))
    c2 = dict(np.load(os.path.join(root, "c2.npz")))
    rng = np.random.default_rng(1)
    Xg = {N: eng.dev(rng.random((N, 20))) for N in (2048, 4096)}
    Sg = {N: eng.empty(N, N) for N in (2048, 4096)}
    th3 = c3["theta"]
    Xc3 = eng.dev(rng.random((65536, 20)))
    Xc2 = eng.dev(rng.random((65536, 6)))
    posts = {}
    for k in KERNELS:
        Sinv = eng.pd_inverse(eng.gram(c3["X"], th3, k))
        posts[("c3", k)] = eng.posterior(c3["X"], th3, k, Sinv, c3["fMAP"], int(c3["m"]))
        Sinv = eng.pd_inverse(eng.gram(c2["X"], c2["theta"], k))
        posts[("c2", k)] = eng.posterior(c2["X"], c2["theta"], k, Sinv, c2["fMAP"], int(c2["m"]))
    mustar3 = float(np.max(c3["mu"]))
    mustar2 = float(np.max(c2["mu"]))
    cases = [
        ("gram N=2048 D=20 (graph replay)", lambda k: graph_ms(lambda: eng.gram(Xg[2048], th3, k, out=Sg[2048]))),
        ("gram N=4096 D=20 (graph replay)", lambda k: graph_ms(lambda: eng.gram(Xg[4096], th3, k, out=Sg[4096]))),
        ("K* at C3 (kstar kernel, events)", lambda k: event_ms(eng, "kstar", lambda: eng.predict(
            posts[("c3", k)], Xc3, score=SCORE_POINTWISE_EI, mustar=mustar3, want_var=False, want_mu=False))),
        ("C3 scoring step (ppbo_predict, wall)", lambda k: wall_ms(lambda: eng.predict(
            posts[("c3", k)], Xc3, score=SCORE_POINTWISE_EI, mustar=mustar3, want_var=False, want_mu=False))),
        ("fused scorer at C2 (fused_score, events)", lambda k: event_ms(eng, "fused_score", lambda: eng.predict(
            posts[("c2", k)], Xc2, score=SCORE_POINTWISE_EI, mustar=mustar2, want_var=False, want_mu=False))),
        ("mu_star search at C3 (ppbo_mean_search, wall)", lambda k: wall_ms(lambda: eng.mean_search(
            posts[("c3", k)], Xc3, K=32), reps=5)),
        ("fit at C3 (ppbo_gp_fit, wall)", lambda k: wall_ms(lambda: eng.gp_fit(
            c3["X"], th3, k, int(c3["m"]), c3["f_init"]), reps=5)),
    ]
    print(f"device: {torch.cuda.get_device_name(0)}; {rounds} alternating rounds per quantity; medians in ms")
    for name, fn in cases:
        t = {k: [] for k in KERNELS}
        for _ in range(rounds):
            for k in KERNELS:
                t[k].append(fn(k))
        se, ma = float(np.median(t["SE_kernel"])), float(np.median(t["Matern52_kernel"]))
        spread = {k: (min(v), max(v)) for k, v in t.items()}
        print(f"{name:48s} SE {se:9.4f}  Matern-5/2 {ma:9.4f}  ratio {ma / se:5.3f}   "
              f"(SE {spread['SE_kernel'][0]:.4f}-{spread['SE_kernel'][1]:.4f}, "
              f"M52 {spread['Matern52_kernel'][0]:.4f}-{spread['Matern52_kernel'][1]:.4f})", flush=True)
    # the fit's work: L-BFGS evaluations and TR iterations under each kernel (the conditioning prediction)
    for k in KERNELS:
        st = eng.gp_fit(c3["X"], th3, k, int(c3["m"]), c3["f_init"])["stats"]
        print(f"fit at C3 {k}: converged={st['converged']} lbfgs_evals={st['lbfgs_evals']} iterations={st['iterations']} "
              f"n_cholesky={st['n_cholesky']}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
