#!/usr/bin/env python3
"""Engine.predict_kg (the knowledge gradient of every candidate over a field: the tournament's cross product with the
envelope march behind it) against Engine.predict_tournament on the same sets, on one device, in one process.

  C3 (tests/golden/c3.npz: N = 2048, D = 20) and C2 (tests/golden/c2.npz: N = 512, D = 6), Ma = 65536 uniform candidates,
  fields of Mb in {16, 256, 1024}: the Mb candidates of the largest posterior mean, so the recommendation is among them

  steady    each call captured ten times into a HIP graph (torch.cuda.CUDAGraph over the stream the library launches on:
            device-resident sets, no host output, workspaces warm, so nothing allocates or synchronises) and the two
            graphs replayed in turn so that clock drift falls on both; the time of a call is the event time of a block
            of replays over its calls, median of the rounds.  predict_tournament's device code is the parent commit's.
  brackets  the library's event brackets in a separate pass: "kg" (s_i and the own slopes, then kg_envelope_kernel, per
            chunk), "tournament" (tournament_kernel, which in predict_kg also writes the chunk's covariances),
            "tournament_field", and predict's own "kstar", "quadform", "score", "fused_score"
  kinks     the histogram of the kinks of the 65536 envelopes
  argmax    KG's best row against pointwise EI's (mustar = the largest mean of the field) on the same candidates

Per-kernel times by name come from a run of its own under the profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o kg -- python tools/kg_time.py --profile

usage: python tools/kg_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import SCORE_POINTWISE_EI, TOURNAMENT_BORDA, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MA = 65536
FIELDS = (16, 256, 1024)
SLOTS = ("kg", "tournament", "tournament_field", "kstar", "quadform", "score", "fused_score")
PER_GRAPH, REPLAYS = 10, 3


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1]


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


def _sets(eng, post, D, Mb):
    """The candidates and the field: the Mb candidates of the largest mean."""
    gen = torch.Generator(device=eng.device).manual_seed(1)
    Xa = torch.rand((MA, D), dtype=torch.float64, device=eng.device, generator=gen)
    mu = eng.predict(post, Xa, want_best=False)["mu"]
    return Xa, Xa[torch.topk(mu, Mb).indices].contiguous()


def profile():
    eng = get_engine(0)
    post, D = _model(eng, "c3")
    Xa, Xb = _sets(eng, post, D, 1024)
    for _ in range(5):
        eng.predict_tournament(post, Xa, Xb, score=TOURNAMENT_BORDA, want_best=False)
        eng.predict_kg(post, Xa, Xb, want_best=False)
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
    out(f"predict_kg against predict_tournament: HIP-graph replays ({PER_GRAPH} calls per graph, blocks of {REPLAYS} replays), "
        f"medians of {rounds} alternating rounds, ms per call")
    for name in ("c3", "c2"):
        post, D = _model(eng, name)
        out(f"{name}: N = {post.X.shape[0]}, D = {D}, operator form {post.form}, Ma = {MA}")
        for Mb in FIELDS:
            Xa, Xb = _sets(eng, post, D, Mb)
            calls = {"tournament": lambda: eng.predict_tournament(post, Xa, Xb, score=TOURNAMENT_BORDA, want_best=False),
                     "kg": lambda: eng.predict_kg(post, Xa, Xb, want_best=False)}
            # the two entries share the tournament's workspace slot and predict_kg asks more of it: a graph holds the
            # addresses it was captured with, and a slot that grows is freed -- so both run once, to the slot's final
            # size, before either is captured (the graphs of the previous field are gone by now)
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            graphs = {k: _capture(fn) for k, fn in calls.items()}
            t = {k: [] for k in graphs}
            for _ in range(rounds):
                for k, g in graphs.items():
                    t[k].append(_replay_ms(g))
            md = {k: float(np.median(v)) for k, v in t.items()}
            out(f"    Mb = {Mb:4d}: tournament {md['tournament']:8.3f} [{min(t['tournament']):.3f} .. {max(t['tournament']):.3f}]   "
                f"kg {md['kg']:8.3f} [{min(t['kg']):.3f} .. {max(t['kg']):.3f}]   = {md['kg'] / md['tournament']:.2f} x tournament")
            del graphs
            kb, tb = _brackets(eng, calls["kg"], 5), _brackets(eng, calls["tournament"], 5)
            out("              brackets, ms per call, kg: " + ", ".join(f"{k} {v:.3f}" for k, v in kb.items())
                + "   | tournament: " + ", ".join(f"{k} {v:.3f}" for k, v in tb.items()))
            if "kg" in kb:
                out(f"              the envelope launches: {kb['kg']:.3f} ms = {kb['kg'] / md['kg']:.2f} of the call; the cross product "
                    f"with its covariances written {kb['tournament']:.3f} against {tb['tournament']:.3f} without")
            res = eng.predict_kg(post, Xa, Xb, want_kinks=True)
            kinks, kg = res["kinks"].cpu().numpy(), res["kg"].cpu().numpy()
            hist = np.bincount(kinks)
            out(f"              kinks: mean {kinks.mean():.2f}, max {kinks.max()}, histogram from 0: " + " ".join(str(int(h)) for h in hist))
            mustar = float(res["mu_b"].max().item())
            ei = eng.predict(post, Xa, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
            sc = ei["score"].cpu().numpy()
            i_kg, i_ei = int(res["best_idx"]), int(ei["best_idx"])
            dist = float((Xa[i_kg] - Xa[i_ei]).norm().item())
            out(f"              argmax: KG row {i_kg} (KG {kg[i_kg]:.4e}, EI {sc[i_kg]:.4e}, EI rank {int((sc > sc[i_kg]).sum()) + 1}), "
                f"EI row {i_ei} (KG {kg[i_ei]:.4e}, EI {sc[i_ei]:.4e}, KG rank {int((kg > kg[i_ei]).sum()) + 1}), "
                f"|x_KG - x_EI| = {dist:.3f}")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
