#!/usr/bin/env python3
"""Engine.predict_tournament (every candidate against every opponent: win matrix, Borda / worst-case scores) against
Engine.predict on the same candidates and against Engine.predict_pairs on the explicit pairs, on one device, in one
process, alternating so that clock drift falls on both.

  C3 (tests/golden/c3.npz: N = 2048, D = 20) and C2 (tests/golden/c2.npz: N = 512, D = 6)

  (a) Ma = 65536 candidates against Mb in {16, 256, 1024} opponents, scores only (no Ma x Mb output):
      wall       the whole call, device-resident inputs, no argmax read-back: median of the rounds, and its multiple of
                 predict on the same 65536 rows in the same rounds
      brackets   the library's event brackets in a separate pass: "tournament" (tournament_kernel, one launch per chunk),
                 "tournament_field" (the field pass: K*_B, U), and predict's own "kstar", "quadform", "score", "fused_score"
      share      2 Ma K Mb flop of tournament_kernel over its bracket time, as a share of the 78.6 TF fp64 MFMA peak; K the
                 contracted rows of the layout (N rounded up to 16, less the n_q skipped rows of the edge form)
  (b) Ma = 4096 against Mb = 256 with both matrices written, against predict_pairs on the 1,048,576 explicit pairs
      (pairs built once, outside the timing): five alternating rounds, medians, the ratio

Per-kernel times by name come from a run of its own under the profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o tournament -- python tools/tournament_time.py --profile

usage: python tools/tournament_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import FORM_EDGE, PAIR_PROB, SCORE_MEAN, TOURNAMENT_BORDA, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MA = 65536
FIELDS = (16, 256, 1024)
SLOTS = ("tournament", "tournament_field", "kstar", "quadform", "score", "fused_score")
PEAK_TF = 78.6


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1]


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


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


def _contracted_rows(post):
    N = post.X.shape[0]
    n_q = N // (post.m + 1)
    return ((N + 15) & ~15) - ((n_q & ~15) if post.form == FORM_EDGE else 0)


def profile():
    eng = get_engine(0)
    post, D = _model(eng, "c3")
    rng = np.random.default_rng(1)
    Xa, Xb = eng.dev(rng.random((MA, D))), eng.dev(rng.random((1024, D)))
    for _ in range(5):
        eng.predict(post, Xa, score=SCORE_MEAN, want_best=False)
        eng.predict_tournament(post, Xa, Xb, score=TOURNAMENT_BORDA, want_best=False)
    torch.cuda.synchronize()


def main():
    if "--profile" in sys.argv:
        return profile()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 11
    fh = open(args[1], "w") if len(args) > 1 else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    eng = get_engine(0)
    out(f"predict_tournament: medians of {rounds} alternating rounds after 3 warm-up rounds, ms (device-synchronised wall)")
    for name in ("c3", "c2"):
        post, D = _model(eng, name)
        N, K = post.X.shape[0], _contracted_rows(post)
        rng = np.random.default_rng(1)
        Xa = eng.dev(rng.random((MA, D)))
        out(f"{name}: N = {N}, D = {D}, operator form {post.form}, contracted rows K = {K}")
        out(f"  (a) Ma = {MA}, scores only")
        single = lambda: eng.predict(post, Xa, score=SCORE_MEAN, want_best=False)  # noqa: E731
        for Mb in FIELDS:
            Xb = eng.dev(rng.random((Mb, D)))
            tour = lambda: eng.predict_tournament(post, Xa, Xb, score=TOURNAMENT_BORDA, want_best=False)  # noqa: E731
            for _ in range(3):
                single()
                tour()
            t = {"predict": [], "tournament": []}
            for _ in range(rounds):
                t["predict"].append(_ms(single))
                t["tournament"].append(_ms(tour))
            md = {k: float(np.median(v)) for k, v in t.items()}
            sp = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
            kb = _brackets(eng, tour, 5)
            ks = _brackets(eng, single, 5)
            out(f"    Mb = {Mb:4d}: predict {md['predict']:8.3f} [{sp['predict'][0]:.3f} .. {sp['predict'][1]:.3f}]   "
                f"tournament {md['tournament']:8.3f} [{sp['tournament'][0]:.3f} .. {sp['tournament'][1]:.3f}]   "
                f"= {md['tournament'] / md['predict']:.2f} x predict")
            out("              brackets, ms per call: " + ", ".join(f"{k} {v:.3f}" for k, v in kb.items())
                + "   | predict alone: " + ", ".join(f"{k} {v:.3f}" for k, v in ks.items()))
            if "tournament" in kb:
                tf = 2.0 * MA * K * Mb / (kb["tournament"] * 1e-3) / 1e12
                own = sum(v for k, v in ks.items())
                out(f"              tournament_kernel {kb['tournament']:.3f} ms = {tf:.1f} TF = {tf / PEAK_TF:.3f} of the fp64 MFMA peak"
                    f" on 2 Ma K Mb flop; {kb['tournament'] / own:.2f} x predict's launches, field pass "
                    f"{kb.get('tournament_field', 0.0) / own:.2f} x")
        Ma2, Mb2 = 4096, 256
        Xa2, Xb2 = Xa[:Ma2].contiguous(), eng.dev(rng.random((Mb2, D)))
        Pa = Xa2.repeat_interleave(Mb2, dim=0).contiguous()
        Pb = Xb2.repeat(Ma2, 1).contiguous()
        tour = lambda: eng.predict_tournament(post, Xa2, Xb2, want_cov=True, want_prob=True, want_best=False)  # noqa: E731
        pairs = lambda: eng.predict_pairs(post, Pa, Pb, score=PAIR_PROB, want_best=False)  # noqa: E731
        for _ in range(2):
            tour()
            pairs()
        t = {"tournament": [], "pairs": []}
        for _ in range(5):
            t["tournament"].append(_ms(tour))
            t["pairs"].append(_ms(pairs))
        md = {k: float(np.median(v)) for k, v in t.items()}
        out(f"  (b) Ma = {Ma2}, Mb = {Mb2}, cov and prob written, against predict_pairs on the {Ma2 * Mb2} explicit pairs (5 rounds)")
        out(f"    tournament {md['tournament']:9.3f} [{min(t['tournament']):.3f} .. {max(t['tournament']):.3f}]   "
            f"predict_pairs {md['pairs']:9.3f} [{min(t['pairs']):.3f} .. {max(t['pairs']):.3f}]   "
            f"ratio {md['pairs'] / md['tournament']:.1f} x")
        d = (tour()["prob"].reshape(-1) - pairs()["prob"]).abs().max().item()
        out(f"    max |p_tournament - p_pairs| = {d:.2e}")
        del Pa, Pb
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
