#!/usr/bin/env python3
"""Engine.predict_marginals (main effects and interactions: f with all but two coordinates averaged over the box) against
Engine.predict_pairs (duels) and Engine.predict (single points) at the same column count, on one device, in one process.

  C3 (tests/golden/c3.npz: N = 2048, D = 20), M = 65536 order-2 rows (pure interactions, axes mixed from lane to lane) /
  pairs / points

  steady   each call captured ten times into a HIP graph (torch.cuda.CUDAGraph over the stream the library launches on:
           device-resident rows, axes formed once, no host output, workspaces warm, so nothing allocates or synchronises)
           and the graphs replayed in turn (marginals, pairs, predict, store floor, marginals, ...) so that clock drift
           falls on all of them; the time of a call is the event time of a block of replays over its calls, median of
           the rounds.  On a stream that is being captured the entry leaves out its look at d_dims (include/ppbo_hip.h):
           the graph holds marginal_table_kernel, kstar_marginal_kernel, the contraction and marginal_score_kernel
  floor    ppbo_store_floor over an 11586 x 11586 matrix (1.0002 x the N x M doubles of K*), replayed in the same rounds:
           what writing the column costs on this chip whatever fills it
  kernels  the library's event brackets ("kstar", "quadform", "score") in a separate pass; ppbo_predict_marginals' column
           launch (kstar_marginal_kernel) is timed under "kstar", the name kstar_pair_kernel is timed under
  mean     the column passes once more with the mean alone asked for: no K* store, no star sums, no contraction
  small    the D x 33 = 660 centred main-effect rows of effect_importance() as one call with variance, graph-replayed: the
           row splits are those of a full chunk whatever M is, so a small call runs few workgroups over many design rows
  eager    the calls once more outside a graph, host time from the call to the end of its stream work (rows on the
           device, axes formed once, no best): ppbo_predict_marginals then looks at d_dims first -- one small launch, the
           one-workgroup merge and a wait on the host-mapped record -- which the graph replays leave out
  global   GPModel.effect_importance() end to end (host rows built, two calls, results on the host) at D = 20, T = 33:
           660 main-effect rows and 190 x 1089 = 206910 interaction rows

kstar_pair_kernel, quadform_kernel, pair_score_kernel and ppbo_predict are the parent commit's own device code, so the
ratios below are against the parent in the same run.  Per-kernel times by name come from a run of its own under the
profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o marginals -- python tools/marginals_time.py --profile

usage: python tools/marginals_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import EFFECT_INTERACTION, PAIR_MEAN, PAIR_PROB, SCORE_POINTWISE_EI, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M = 65536
FLOOR_N = 11586
SLOTS = ("kstar", "quadform", "score", "fused_score")
PER_GRAPH, REPLAYS = 10, 5


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1], float(np.max(g["mu"]))


def _rows(eng, D):
    rng = np.random.default_rng(1)
    d = rng.integers(0, D, M)
    e = (d + 1 + rng.integers(0, D - 1, M)) % D
    dims = eng.dev(np.stack([d, e], axis=1).astype(np.int32), dtype=torch.int32)
    return dims, eng.dev(rng.random((M, 2)))


def _calls(eng, post, D, mustar, mean_only=False):
    gen = torch.Generator(device=eng.device).manual_seed(1)
    pts = torch.rand((2 * M, D), dtype=torch.float64, device=eng.device, generator=gen)
    Xa, Xb = pts[:M], pts[M:]
    dims, t = _rows(eng, D)
    ax = eng.marginal_axes(post)
    kw = dict(want_var=False, want_prob=False) if mean_only else {}
    kind = PAIR_MEAN if mean_only else PAIR_PROB
    calls = {"marginals": lambda: eng.predict_marginals(post, dims, t, effect=EFFECT_INTERACTION, kind=kind, want_score=True,
                                                        want_best=False, axes=ax, **kw),
             "pairs": lambda: eng.predict_pairs(post, Xa, Xb, score=kind, want_score=True, want_best=False, **kw)}
    if not mean_only:
        calls["predict"] = lambda: eng.predict(post, Xa, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True, want_best=False)
        buf = torch.empty((FLOOR_N, FLOOR_N), dtype=torch.float64, device=eng.device)
        calls["floor"] = lambda: eng.store_floor(buf)
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
    calls = _calls(eng, *_model(eng, "c3"))
    for _ in range(5):
        for k in ("marginals", "pairs"):
            calls[k]()
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
    out(f"predict_marginals against predict_pairs and predict at C3 (N = {N}, D = {D}, operator form {post.form}), M = {M} order-2 rows")
    out(f"steady state: graphs of {PER_GRAPH} calls, {REPLAYS} replays per block, median of {rounds} alternating rounds, ms per call")
    graphs = {k: _capture(fn) for k, fn in calls.items()}
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, g in graphs.items():
            t[k].append(_replay_ms(g))
    md = {k: float(np.median(v)) for k, v in t.items()}
    names = {"marginals": "predict_marginals (interaction)", "pairs": "predict_pairs", "predict": "predict",
             "floor": f"store floor {FLOOR_N}^2"}
    for k in calls:
        out(f"    {names[k]:32s} {md[k]:9.3f}  [{min(t[k]):.3f} .. {max(t[k]):.3f}]")
    floor = md["floor"] * (N * M) / (FLOOR_N * FLOOR_N)
    out(f"    predict_marginals / predict_pairs = {md['marginals'] / md['pairs']:.3f}    / predict = {md['marginals'] / md['predict']:.3f}")
    out(f"    store floor for the N x M column block: {floor:.3f} ms")
    del graphs
    br = {k: _brackets(eng, fn, 5) for k, fn in calls.items() if k != "floor"}
    out("event brackets, ms per call")
    for k in br:
        out(f"    {k:10s} " + ", ".join(f"{s} {v:.3f}" for s, v in br[k].items()))
    km, kp = br["marginals"]["kstar"], br["pairs"]["kstar"]
    out(f"    column pass: kstar_marginal_kernel {km:.3f}, kstar_pair_kernel {kp:.3f} (ratio {km / kp:.3f}), store floor {floor:.3f} "
        f"(kstar_marginal_kernel / floor = {km / floor:.2f}, kstar_pair_kernel / floor = {kp / floor:.2f})")
    out(f"    contraction: marginals {br['marginals'].get('quadform', float('nan')):.3f}, pairs {br['pairs'].get('quadform', float('nan')):.3f}")
    # a small call: the main-effect rows of effect_importance()
    ax = eng.marginal_axes(post)
    sd = eng.dev(np.stack([np.repeat(np.arange(D), 33), np.full(D * 33, -1)], axis=1).astype(np.int32), dtype=torch.int32)
    st = eng.dev(np.stack([np.tile(np.linspace(0.0, 1.0, 33), D), np.zeros(D * 33)], axis=1))
    small = lambda: eng.predict_marginals(post, sd, st, effect=1, kind=PAIR_PROB, want_score=True, want_best=False, axes=ax)
    gs = _capture(small)
    ts = [_replay_ms(gs) for _ in range(rounds)]
    out(f"small call ({D * 33} order-1 rows, mean + variance + p), graph replays: {float(np.median(ts)):.3f} ms  [{min(ts):.3f} .. {max(ts):.3f}]")
    del gs
    out("    its brackets: " + ", ".join(f"{s} {v:.3f}" for s, v in _brackets(eng, small, 5).items()))

    def eager(fn, reps=20):
        v = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(v))
    out("outside a graph, host time per call to the end of its stream work, ms: "
        + ", ".join(f"{k} {eager(calls[k]):.3f}" for k in ("marginals", "pairs", "predict")) + f", small call {eager(small):.3f}")
    bm = {k: _brackets(eng, fn, 5) for k, fn in _calls(eng, post, D, mustar, mean_only=True).items()}
    out("the mean alone (no K* store, no star sums, no contraction), kstar bracket, ms per call: "
        + ", ".join(f"{k} {v['kstar']:.3f}" for k, v in bm.items()))
    out("    stores + star sums (full - mean alone): " + ", ".join(f"{k} {br[k]['kstar'] - bm[k]['kstar']:.3f}" for k in bm))
    # effect_importance end to end
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp.eng, gp._post, gp.D = eng, post, D
    gp.effect_importance(T=33)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        imp = gp.effect_importance(T=33)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out(f"effect_importance(T = 33) at D = {D}: {D * 33} main-effect rows + {len(imp['pairs'])} x {33 * 33} interaction rows, "
        f"end to end {1e3 * float(np.median(ts)):.1f} ms [{1e3 * min(ts):.1f} .. {1e3 * max(ts):.1f}]")
    order = np.argsort(-imp["main_range"])[:3]
    top = tuple(int(v) for v in imp["pairs"][int(np.argmax(imp["interaction_max"]))])
    out("    largest main-effect ranges: " + ", ".join(f"axis {d}: {imp['main_range'][d]:.3e}" for d in order)
        + f";  largest interaction |mu|: pair {top} {imp['interaction_max'].max():.3e}")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
