#!/usr/bin/env python3
"""Engine.predict_pairs (duels: mean, variance and win probability of f(a) - f(b)) against Engine.predict (mean,
variance, pointwise EI of single points) at the same column count, on one device, in one process, alternating
(predict, pairs, predict, ...) so that clock drift falls on both.

  C3 (tests/golden/c3.npz: N = 2048, D = 20) and C2 (tests/golden/c2.npz: N = 512, D = 6), M = 65536 pairs / points

  wall      the whole call, device-resident inputs, no host output (no argmax read-back): median of the rounds
  kernels   the library's event brackets ("kstar", "quadform", "score", "fused_score") in a separate pass: the pair
            call's three launches beside predict's (kstar_kernel, quadform_kernel and score_kernel, or the one-launch
            kernel where predict takes it -- pairs never do)

kstar_kernel, quadform_kernel, score_kernel and ppbo_predict are the parent commit's own (their code is untouched), so
the ratios below are against the parent in the same run.  Per-kernel times by name come from a run of its own under
the profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o pairs -- python tools/pairs_time.py --profile

usage: python tools/pairs_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import PAIR_PROB, SCORE_POINTWISE_EI, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M = 65536
SLOTS = ("kstar", "quadform", "score", "fused_score")


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    rng = np.random.default_rng(1)
    D = g["X"].shape[1]
    return r["post"], eng.dev(rng.random((M, D))), eng.dev(rng.random((M, D))), float(np.max(g["mu"]))


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _calls(eng, post, Xa, Xb, mustar):
    single = lambda: eng.predict(post, Xa, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True, want_best=False)  # noqa: E731
    pairs = lambda: eng.predict_pairs(post, Xa, Xb, score=PAIR_PROB, want_score=True, want_best=False)  # noqa: E731
    return single, pairs


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
    post, Xa, Xb, mustar = _model(eng, "c3")
    single, pairs = _calls(eng, post, Xa, Xb, mustar)
    for _ in range(5):
        single()
        pairs()
    torch.cuda.synchronize()


def main():
    if "--profile" in sys.argv:
        return profile()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 15
    fh = open(args[1], "w") if len(args) > 1 else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    eng = get_engine(0)
    out(f"predict_pairs against predict, M = {M} columns: median of {rounds} alternating rounds, ms")
    for name in ("c3", "c2"):
        post, Xa, Xb, mustar = _model(eng, name)
        single, pairs = _calls(eng, post, Xa, Xb, mustar)
        for _ in range(3):
            single()
            pairs()
        t = {"predict": [], "pairs": []}
        for _ in range(rounds):
            t["predict"].append(_ms(single))
            t["pairs"].append(_ms(pairs))
        md = {k: float(np.median(v)) for k, v in t.items()}
        sp = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
        N, D = post.X.shape
        out(f"  {name}: N = {N}, D = {D}, operator form {post.form}")
        out(f"    predict        {md['predict']:8.3f}  [{sp['predict'][0]:.3f} .. {sp['predict'][1]:.3f}]")
        out(f"    predict_pairs  {md['pairs']:8.3f}  [{sp['pairs'][0]:.3f} .. {sp['pairs'][1]:.3f}]   ratio {md['pairs'] / md['predict']:.3f}")
        ks, kp = _brackets(eng, single, 10), _brackets(eng, pairs, 10)
        out("    event brackets, ms per call:   predict: " + ", ".join(f"{k} {v:.3f}" for k, v in ks.items()))
        out("                                   pairs:   " + ", ".join(f"{k} {v:.3f}" for k, v in kp.items()))
        for s in ("kstar", "quadform", "score"):
            if s in ks and s in kp:
                out(f"    {s:9s} pairs / predict = {kp[s] / ks[s]:.3f}")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
