#!/usr/bin/env python3
"""Engine.predict_curvatures (mean, variance and sign probability of d^2/da^2 f(x + a xi)) against Engine.predict_slopes
and Engine.predict (single points) at the same column count, on one device, in one process.

  C3 (tests/golden/c3.npz: N = 2048, D = 20), M = 65536 rows / points

  steady   each call captured ten times into a HIP graph (torch.cuda.CUDAGraph over the stream the library launches on:
           device-resident inputs, no host output, workspaces warm, so nothing allocates or synchronises) and the three
           graphs replayed in turn (curvatures, slopes, predict, curvatures, ...) so that clock drift falls on all of them; the
           time of a call is the event time of a block of replays over its calls, median of the rounds
  kernels  the library's event brackets ("kstar", "quadform", "score") in a separate pass.  ppbo_predict_curvatures' K*
           launch (kstar_curv_kernel) is timed under "kstar", the name kstar_kernel and kstar_slope_kernel are timed under

kstar_slope_kernel, quadform_kernel, slope_score_kernel, ppbo_predict_slopes' launches and ppbo_predict are the parent
commit's own device code, so the ratios below are against the parent in the same run.  Per-kernel times by name come
from a run of its own under the profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o curvature -- python tools/curvature_time.py --profile

usage: python tools/curvature_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import CURV_PROB, SCORE_POINTWISE_EI, SLOPE_PROB, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M = 65536
SLOTS = ("kstar", "quadform", "score", "fused_score")
PER_GRAPH, REPLAYS = 10, 10


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    rng = np.random.default_rng(1)
    D = g["X"].shape[1]
    return r["post"], eng.dev(rng.random((M, D))), eng.dev(rng.standard_normal((M, D))), float(np.max(g["mu"]))


def _calls(eng, post, X, Xi, mustar):
    return dict(
        curv=lambda: eng.predict_curvatures(post, X, Xi, score=CURV_PROB, want_score=True, want_best=False),
        slopes=lambda: eng.predict_slopes(post, X, Xi, score=SLOPE_PROB, want_score=True, want_best=False),
        predict=lambda: eng.predict(post, X, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True, want_best=False))


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
    calls = _calls(eng, *_model(eng, "c3"))
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
    post, X, Xi, mustar = _model(eng, "c3")
    calls = _calls(eng, post, X, Xi, mustar)
    N, D = post.X.shape
    out(f"predict_curvatures against predict_slopes and predict at C3 (N = {N}, D = {D}, operator form {post.form}), M = {M} columns")
    out(f"steady state: graphs of {PER_GRAPH} calls, {REPLAYS} replays per block, median of {rounds} alternating rounds, ms per call")
    graphs = {k: _capture(fn) for k, fn in calls.items()}
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, g in graphs.items():
            t[k].append(_replay_ms(g))
    md = {k: float(np.median(v)) for k, v in t.items()}
    for k, name in (("curv", "predict_curvatures"), ("slopes", "predict_slopes"), ("predict", "predict")):
        out(f"    {name:19s} {md[k]:8.3f}  [{min(t[k]):.3f} .. {max(t[k]):.3f}]")
    out(f"    predict_curvatures / predict_slopes = {md['curv'] / md['slopes']:.3f}    predict_curvatures / predict = {md['curv'] / md['predict']:.3f}")
    br = {k: _brackets(eng, fn, 10) for k, fn in calls.items()}
    out("event brackets, ms per call")
    for k in ("curv", "slopes", "predict"):
        out(f"    {k:8s} " + ", ".join(f"{s} {v:.3f}" for s, v in br[k].items()))
    for s in ("kstar", "quadform", "score"):
        if all(s in br[k] for k in br):
            out(f"    {s:9s} curv / slopes = {br['curv'][s] / br['slopes'][s]:.3f}    curv / predict = {br['curv'][s] / br['predict'][s]:.3f}")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
