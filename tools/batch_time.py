#!/usr/bin/env python3
"""Engine.search_batch (a shortlist: q greedy picks under the conditioned variance) against Engine.predict on the same
candidates, against today's composition (q host-looped predict_tournament(Xc, [pick]) calls) and against a plain
streaming read of the K* workspace's bytes, on one device, in one process, alternating so that clock drift falls on all.

  C3 (tests/golden/c3.npz: N = 2048, D = 20), C2 (c2.npz: N = 512, D = 6) and C5 (c5.npz: N = 4096, D = 6), M = 65536

  per q in {1, 8, 32, 64}:
    wall       the whole call (device-resident candidates, var_cond written so that all q passes run): median of the
               rounds, and predict (EI, best record, mu and var written) on the same rows in the same rounds
    brackets   the library's event brackets in a pass of its own: "batch_step" and "batch_field" per pick, and predict's
               own "kstar", "quadform", "score", "fused_score"
    floor      torch.sum over a device tensor of the step's K* bytes (contracted rows x M doubles), timed in the same
               rounds: the plain streaming read.  batch_step per pick over it, and the step's TB/s on those bytes plus
               the downdate's reads (V_0 .. V_{j-1}: (q - 1) / 2 x M doubles on average) and the per-candidate arrays
  q = 8:       the host loop of predict_tournament(Xc, [pick]) calls, for the ratio

usage: python tools/batch_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import FORM_EDGE, SCORE_POINTWISE_EI, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M = 65536
QS = (1, 8, 32, 64)
SLOTS = ("batch_step", "batch_field", "kstar", "quadform", "score", "fused_score")


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


def _brackets(eng, fn, reps):
    eng.profile(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    got = {}
    for s in SLOTS:
        tot, cnt = eng.profile_read(s)
        if cnt:
            got[s] = (tot / reps, cnt // reps)
    eng.profile(False)
    return got


def _contracted_rows(post):
    """Rows of the K* workspace a step reads: N (rounded up to 16 where the scoring launches left the workspace), less
    the skipped observation rows of the edge form."""
    N = post.X.shape[0]
    n_q = N // (post.m + 1)
    return ((N + 15) & ~15) - ((n_q & ~15) if post.form == FORM_EDGE else 0)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    fh = open(args[1], "w") if len(args) > 1 else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    eng = get_engine(0)
    out(f"search_batch: medians of {rounds} alternating rounds after 2 warm-up rounds, ms (device-synchronised wall), M = {M}")
    for name in ("c3", "c2", "c5"):
        post, D, mustar = _model(eng, name)
        N, K = post.X.shape[0], _contracted_rows(post)
        rng = np.random.default_rng(1)
        Xc = eng.dev(rng.random((M, D)))
        kbytes = 8.0 * K * M
        stream = torch.empty(K * M, dtype=torch.float64, device=Xc.device).normal_()
        out(f"{name}: N = {N}, D = {D}, kernel {post.kernel}, operator form {post.form}, contracted rows K = {K}, "
            f"K* bytes per pick {kbytes / 1e9:.3f} GB")
        single = lambda: eng.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar)  # noqa: E731
        floor = lambda: stream.sum()  # noqa: E731
        for q in QS:
            batch = lambda: eng.search_batch(post, Xc, q, score=SCORE_POINTWISE_EI, mustar=mustar, want_var_cond=True)  # noqa: E731
            for _ in range(2):
                single(), batch(), floor()
            t = {"predict": [], "batch": [], "floor": []}
            for _ in range(rounds):
                t["predict"].append(_ms(single))
                t["batch"].append(_ms(batch))
                t["floor"].append(_ms(floor))
            md = {k: float(np.median(v)) for k, v in t.items()}
            sp = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
            kb = _brackets(eng, batch, 3)
            out(f"  q = {q:2d}: predict {md['predict']:7.3f} [{sp['predict'][0]:.3f} .. {sp['predict'][1]:.3f}]   "
                f"search_batch {md['batch']:8.3f} [{sp['batch'][0]:.3f} .. {sp['batch'][1]:.3f}]   "
                f"= {md['batch'] / md['predict']:.2f} x predict, {(md['batch'] - md['predict']) / q:.3f} per pick beyond it")
            out("          brackets, ms per call (count): " + ", ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in kb.items()))
            if "batch_step" in kb:
                step = kb["batch_step"][0] / kb["batch_step"][1]
                field = kb["batch_field"][0] / kb["batch_field"][1]
                extra = 8.0 * M * ((q - 1) / 2.0 + 4.0 + D)          # V_i reads, V_j write, var in / out, mu, the rows
                out(f"          per pick: batch_step {step * 1e3:.1f} us, batch_field {field * 1e3:.1f} us;  streaming read of "
                    f"the K* bytes (torch.sum) {md['floor'] * 1e3:.1f} us [{sp['floor'][0] * 1e3:.1f} .. {sp['floor'][1] * 1e3:.1f}] "
                    f"= {kbytes / (md['floor'] * 1e-3) / 1e12:.2f} TB/s;  batch_step = {step / md['floor']:.2f} x that read, "
                    f"{(kbytes + extra) / (step * 1e-3) / 1e12:.2f} TB/s on its own bytes ({kbytes / (step * 1e-3) / 1e12:.2f} on K* alone)")
        # today's composition at q = 8: one predict_tournament(Xc, [pick]) per pick, the pick read back by the host
        def host_loop(q=8):
            i = eng.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar)["best_idx"]
            for _ in range(q):
                i = eng.predict_tournament(post, Xc, Xc[i:i + 1])["best_idx"]
        batch8 = lambda: eng.search_batch(post, Xc, 8, score=SCORE_POINTWISE_EI, mustar=mustar, want_var_cond=True)  # noqa: E731
        host_loop(), batch8()
        t = {"loop": [], "batch": []}
        for _ in range(max(3, rounds // 2)):
            t["loop"].append(_ms(host_loop))
            t["batch"].append(_ms(batch8))
        out(f"  q =  8 against the host loop of 8 predict_tournament(Xc, [pick]) calls: loop {np.median(t['loop']):.3f} "
            f"[{min(t['loop']):.3f} .. {max(t['loop']):.3f}], search_batch {np.median(t['batch']):.3f}, "
            f"ratio {np.median(t['loop']) / np.median(t['batch']):.1f} x")
        del stream, Xc
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
