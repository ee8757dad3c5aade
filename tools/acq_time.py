#!/usr/bin/env python3
"""Engine.acq_grad / Engine.acq_ascent / GPModel.maximize_acquisition on one device, in one process, alternating with
Engine.predict so that clock drift falls on all.

  C3 (tests/golden/c3.npz: N = 2048, D = 20) and C2 (c2.npz: N = 512, D = 6), pool M = 65536, K = 32 starts

  round      one evaluation round of the ascent, acq_grad on K = 32 points with the score gradient alone: the wall, and
             the library's event brackets in a pass of its own -- "acq_field" (the tournament's field pass: K*, the
             edge rows, two GEMMs on pinned 32 x 32 tiles) and "acq_grad" (acq_grad_kernel)
  ascent     the whole acq_ascent(K = 32, iters = 60): 61 rounds and 62 judging launches, nothing synchronises inside
  maximize   maximize_acquisition(n_starts = 32, iters = 60) on the resident pool (search_batch's 32 picks, then the
             ascent, then the copies back) next to one predict step (EI, best record) on the same pool
  gain       the refined EI / variance over the pool's best (the shortlist's pick 0), per score kind

usage: python tools/acq_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE, get_engine  # noqa: E402
from ppbo_amd.gp_model import GPModel  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M, K, ITERS = 65536, 32, 60


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1], float(np.max(g["mu"]))


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _brackets(eng, fn, reps, slots):
    eng.profile(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    got = {}
    for s in slots:
        tot, cnt = eng.profile_read(s)
        if cnt:
            got[s] = (tot / cnt, cnt // reps)          # ms per bracket, brackets per call
    eng.profile(False)
    return got


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 9
    fh = open(args[1], "w") if len(args) > 1 else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    eng = get_engine(0)
    out(f"acquisition gradients and ascent: medians [min .. max] of {rounds} alternating rounds after 2 warm-up rounds, ms "
        f"(device-synchronised wall); pool M = {M}, K = {K} starts, iters = {ITERS}")
    for name in ("c3", "c2"):
        post, D, mustar = _model(eng, name)
        N = post.X.shape[0]
        rng = np.random.default_rng(1)
        pool = eng.dev(rng.random((M, D)))
        gp = GPModel.__new__(GPModel)
        gp.eng, gp._post, gp.xstar, gp.D, gp.mustar = eng, post, None, D, mustar
        starts = eng.dev(gp.shortlist(q=K, score="EI", X_cand=pool)[0])
        out(f"{name}: N = {N}, D = {D}, kernel {post.kernel}, operator form {post.form}")
        fns = {
            "predict": lambda: eng.predict(post, pool, score=SCORE_POINTWISE_EI, mustar=mustar),
            "round": lambda: eng.acq_grad(post, starts, mustar=mustar, want_values=False, want_grad_mu=False, want_grad_var=False),
            "ascent": lambda: eng.acq_ascent(post, starts, mustar=mustar, iters=ITERS),
            "shortlist": lambda: gp.shortlist(q=K, score="EI", X_cand=pool),
            "maximize": lambda: gp.maximize_acquisition(score="EI", n_starts=K, X_cand=pool, iters=ITERS),
        }
        for _ in range(2):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(rounds):
            for k, f in fns.items():
                t[k].append(_ms(f))
        for k in fns:
            out(f"  {k:9s} {np.median(t[k]):8.3f} [{min(t[k]):.3f} .. {max(t[k]):.3f}]")
        md = {k: float(np.median(v)) for k, v in t.items()}
        out(f"  maximize_acquisition = {md['maximize'] / md['predict']:.2f} x one predict step, of which the shortlist "
            f"{md['shortlist']:.3f} and the ascent {md['ascent']:.3f}; the ascent = {md['ascent'] / (ITERS + 1) * 1e3:.1f} us per round")
        br = _brackets(eng, fns["round"], 20, ("acq_field", "acq_grad"))
        out("  one round, brackets: " + ", ".join(f"{k} {v[0] * 1e3:.1f} us ({v[1]} per call)" for k, v in br.items())
            + f"; wall of the call {md['round'] * 1e3:.1f} us")
        ba = _brackets(eng, fns["ascent"], 3, ("acq_field", "acq_grad"))
        out("  inside the ascent, brackets: " + ", ".join(f"{k} {v[0] * 1e3:.1f} us ({v[1]} per call)" for k, v in ba.items()))
        for score, kind in (("EI", SCORE_POINTWISE_EI), ("variance", SCORE_VARIANCE)):
            r = gp.maximize_acquisition(score=score, n_starts=K, X_cand=pool, iters=ITERS)
            best0 = float(np.max(r["start_scores"]))
            at = eng.acq_grad(post, r["starts"], score=kind, mustar=mustar, want_grad_mu=False, want_grad_var=False,
                              want_grad_score=False)["score"].cpu().numpy()
            up = r["scores"] - at
            out(f"  gain {score}: pool best {best0:.6g} -> refined {r['score']:.6g} ({r['score'] / best0:.3f} x; the best start alone "
                f"{float(at.max()):.6g}); per start: median gain {np.median(up):.3g}, all >= 0: {bool(np.all(up >= 0))}; "
                f"iterations {np.bincount(r['iters'], minlength=ITERS + 1)[[0, ITERS]]} at (0, {ITERS}), median {int(np.median(r['iters']))}")
        del pool
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
