#!/usr/bin/env python3
"""Engine.predict_functionals (mean, variance and sign probability of sum_g w_g f(x_g) over groups of G points) against
Engine.predict_pairs (duels) and Engine.predict (single points) at the same column count, on one device, in one process.

  C3 (tests/golden/c3.npz: N = 2048, D = 20), M = 65536 groups / pairs / points, G in {1, 2, 8, 16, 64}

  steady   each call captured ten times into a HIP graph (torch.cuda.CUDAGraph over the stream the library launches on:
           device-resident inputs, no host output, workspaces warm, so nothing allocates or synchronises) and the graphs
           replayed in turn (functionals G = 1, 2, ..., pairs, predict, functionals G = 1, ...) so that clock drift falls on
           all of them; the time of a call is the event time of a block of replays over its calls, median of the rounds
  kernels  the library's event brackets ("kstar", "quadform", "score") in a separate pass.  ppbo_predict_functionals' K*
           launch (kstar_func_kernel) is timed under "kstar", the name kstar_kernel and kstar_pair_kernel are timed under
  mean     the column passes once more with the mean alone asked for: no K* store, no star sums, no contraction -- what is
           left is staging, tile generation and the mean sum
  route    for context, the only route to such a quantity before this entry that scales: predict on the same M G points
           (G = 2 and 8), which yields only the diagonal of the group's covariance -- a lower bound for any per-point route

kstar_pair_kernel, quadform_kernel, pair_score_kernel and ppbo_predict are the parent commit's own device code, so the
ratios below are against the parent in the same run.  Per-kernel times by name come from a run of its own under the
profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o functionals -- python tools/functionals_time.py --profile

usage: python tools/functionals_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import FUNCTIONAL_MEAN, FUNCTIONAL_PROB, PAIR_MEAN, PAIR_PROB, SCORE_POINTWISE_EI, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M = 65536
GS = (1, 2, 8, 16, 64)
ROUTE_GS = (2, 8)
SLOTS = ("kstar", "quadform", "score", "fused_score")
PER_GRAPH, REPLAYS = 10, 5


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1], float(np.max(g["mu"]))


def _calls(eng, post, D, mustar, gs=GS, route_gs=ROUTE_GS):
    gen = torch.Generator(device=eng.device).manual_seed(1)
    pts = torch.rand((M * max(gs), D), dtype=torch.float64, device=eng.device, generator=gen)
    calls = {}
    for G in gs:
        Xg = pts[:M * G].reshape(M, G, D)
        w = eng.dev(np.random.default_rng(G).standard_normal(G))
        calls[f"func{G}"] = (lambda Xg=Xg, w=w: eng.predict_functionals(post, Xg, w, score=FUNCTIONAL_PROB, want_score=True,
                                                                         want_best=False))
    Xa, Xb = pts[:M], pts[M:2 * M]
    calls["pairs"] = lambda: eng.predict_pairs(post, Xa, Xb, score=PAIR_PROB, want_score=True, want_best=False)
    calls["predict"] = lambda: eng.predict(post, Xa, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True, want_best=False)
    for G in route_gs:
        Xp = pts[:M * G]
        calls[f"points{G}"] = (lambda Xp=Xp: eng.predict(post, Xp, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True,
                                                         want_best=False))
    return calls


def _mean_only_calls(eng, post, D):
    """The column passes without their stores and star sums (the mean alone: no K* is written, no contraction runs)."""
    gen = torch.Generator(device=eng.device).manual_seed(1)
    pts = torch.rand((M * 2, D), dtype=torch.float64, device=eng.device, generator=gen)
    calls = {}
    for G in (1, 2):
        Xg, w = pts[:M * G].reshape(M, G, D), eng.dev(np.random.default_rng(G).standard_normal(G))
        calls[f"func{G}"] = (lambda Xg=Xg, w=w: eng.predict_functionals(post, Xg, w, score=FUNCTIONAL_MEAN, want_var=False,
                                                                         want_prob=False, want_score=True, want_best=False))
    calls["pairs"] = lambda: eng.predict_pairs(post, pts[:M], pts[M:], score=PAIR_MEAN, want_var=False, want_prob=False,
                                               want_score=True, want_best=False)
    return calls


def _capture(fn):
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
            for _ in range(PER_GRAPH):
                fn()
    torch.cuda.synchronize()
    return graph


def _replay_ms(graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    e0.record()
    for _ in range(REPLAYS):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (REPLAYS * PER_GRAPH)


def _brackets(eng, fn, reps):
    eng.profile(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    got = {}
    for s in SLOTS:
        tot, cnt = eng.profile_read(s)
        if cnt:
            got[s] = tot / reps
    eng.profile(False)
    return got


def profile():
    eng = get_engine(0)
    calls = _calls(eng, *_model(eng, "c3"), gs=(2, 16), route_gs=())
    for _ in range(5):
        for fn in calls.values():
            fn()
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
    post, D, mustar = _model(eng, "c3")
    calls = _calls(eng, post, D, mustar)
    N = post.X.shape[0]
    out(f"predict_functionals against predict_pairs and predict at C3 (N = {N}, D = {D}, operator form {post.form}), M = {M} columns")
    out(f"steady state: graphs of {PER_GRAPH} calls, {REPLAYS} replays per block, median of {rounds} alternating rounds, ms per call")
    graphs = {k: _capture(fn) for k, fn in calls.items()}
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, g in graphs.items():
            t[k].append(_replay_ms(g))
    md = {k: float(np.median(v)) for k, v in t.items()}
    for k in calls:
        name = (f"predict_functionals G={k[4:]}" if k.startswith("func") else
                f"predict on M G points, G={k[6:]}" if k.startswith("points") else f"predict_{k}" if k == "pairs" else k)
        out(f"    {name:32s} {md[k]:9.3f}  [{min(t[k]):.3f} .. {max(t[k]):.3f}]")
    for G in GS:
        out(f"    G = {G:2d}: predict_functionals / predict_pairs = {md[f'func{G}'] / md['pairs']:.3f}    / predict = {md[f'func{G}'] / md['predict']:.3f}")
    for G in ROUTE_GS:
        out(f"    G = {G:2d}: predict on M G points / predict_functionals = {md[f'points{G}'] / md[f'func{G}']:.3f}")
    del graphs
    br = {k: _brackets(eng, fn, 5) for k, fn in calls.items() if not k.startswith("points")}
    out("event brackets, ms per call")
    for k in br:
        out(f"    {k:8s} " + ", ".join(f"{s} {v:.3f}" for s, v in br[k].items()))
    ks = {G: br[f"func{G}"]["kstar"] for G in GS}
    out(f"    column pass at G = 2 / kstar_pair_kernel = {ks[2] / br['pairs']['kstar']:.3f}")
    out(f"    column pass per point, ms: " + ", ".join(f"G={G}: {ks[G] / G:.4f}" for G in GS)
        + f";  kstar_pair_kernel per point {br['pairs']['kstar'] / 2:.4f}")
    out(f"    column pass slope in G (G = 16 .. 64): {(ks[64] - ks[16]) / 48:.4f} ms per point")
    out("    contraction: " + ", ".join(f"G={G}: {br[f'func{G}'].get('quadform', float('nan')):.3f}" for G in GS)
        + f";  pairs {br['pairs'].get('quadform', float('nan')):.3f}")
    bm = {k: _brackets(eng, fn, 5) for k, fn in _mean_only_calls(eng, post, D).items()}
    out("the mean alone (no K* store, no star sums, no contraction), kstar bracket, ms per call: "
        + ", ".join(f"{k} {v['kstar']:.3f}" for k, v in bm.items()))
    out("    stores + star sums (full - mean alone): " + ", ".join(
        f"{k} {br[k]['kstar'] - bm[k]['kstar']:.3f}" for k in bm))
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
