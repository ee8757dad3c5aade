#!/usr/bin/env python3
"""Engine.line_choice_xi (choice probabilities over the points of query lines) against Engine.line_acq_xi (EI / varmax
of the same lines) on one device, in one process, alternating (acq, choice, acq, ...) so that clock drift falls on both.

  C3 (tests/golden/c3.npz: N = 2048, D = 20), 512 lines x 70 points, S = 150 and S = 4096 draws, noise on

  wall      the whole call, device-resident inputs, nothing read back: median of the rounds
  stages    the library's event brackets ("line_kstar", "line_y", "line_cov", "line_mc") in a separate pass; every
            stage before the Monte-Carlo launch is the same code on the same operands in both calls, "line_mc" brackets
            line_mc_kernel in one and line_choice_kernel in the other

usage: python tools/line_choice_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
B, G = 512, 70
SLOTS = ("line_kstar", "line_y", "line_cov", "line_mc")


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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 15
    fh = open(args[1], "w") if len(args) > 1 else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()

    eng = get_engine(0)
    g = dict(np.load(os.path.join(GOLDEN, "c3.npz")))
    th = [float(t) for t in g["theta"]]
    post = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)["post"]
    N, D = post.X.shape
    rng = np.random.default_rng(1)
    xis, xs = eng.dev(rng.random((B, D))), eng.dev(rng.random((B, D)) * 0.2)
    al = eng.dev(np.linspace(0.005, 0.995, G))
    mustar, jit = float(np.max(g["mu"])), 1e-10 * th[2] ** 2
    out(f"line_choice_xi against line_acq_xi, C3 (N = {N}, D = {D}, operator form {post.form}), {B} lines x {G} points: "
        f"median of {rounds} alternating rounds, ms")
    for S in (150, 4096):
        ze = eng.randn(7, 2, S, G)
        acq = lambda: eng.line_acq_xi(post, xis, xs, al, ze[0], mustar, jitter=jit)  # noqa: E731
        cho = lambda: eng.line_choice_xi(post, xis, xs, al, ze[0], ze[1], jitter=jit)  # noqa: E731
        full = lambda: eng.line_choice_xi(post, xis, xs, al, ze[0], ze[1], jitter=jit, want_count=True, want_choice=True)  # noqa: E731
        free = lambda: eng.line_choice_xi(post, xis, xs, al, ze[0], None, noise_sd=0.0, jitter=jit)  # noqa: E731
        calls = {"line_acq_xi": acq, "line_choice_xi": cho, "  + count, choice": full, "  noise-free": free}
        for _ in range(3):
            for fn in calls.values():
                fn()
        t = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                t[k].append(_ms(fn))
        md = {k: float(np.median(v)) for k, v in t.items()}
        out(f"  S = {S}")
        for k, v in t.items():
            out(f"    {k:18s} {md[k]:8.3f}  [{min(v):.3f} .. {max(v):.3f}]   ratio {md[k] / md['line_acq_xi']:.3f}")
        ka, kc = _brackets(eng, acq, 10), _brackets(eng, cho, 10)
        out("    event brackets, ms per call:   line_acq_xi:    " + ", ".join(f"{k} {v:.3f}" for k, v in ka.items()))
        out("                                   line_choice_xi: " + ", ".join(f"{k} {v:.3f}" for k, v in kc.items()))
        out(f"    line_mc   choice / acq = {kc['line_mc'] / ka['line_mc']:.3f}")
        p = full()
        out(f"    sum of prob per line in [{float(p['prob'].sum(1).min()):.6f}, {float(p['prob'].sum(1).max()):.6f}], "
            f"choices in [{int(p['choice'].min())}, {int(p['choice'].max())}]")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
