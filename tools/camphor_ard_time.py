#!/usr/bin/env python3
"""The scalar camphor-copper kernel against camphor_copper_ard_kernel (SE on the 11-column embedding) at the C5 shape
(tests/golden/c5.npz: N = 4096, D = 6, m = 31), in one process, alternating (scalar, per-coordinate at the profile,
per-coordinate with l spread 10x, ...) so that clock drift falls on all three.

  scoring step     Engine.predict of 65536 candidates with pointwise EI (K*, contraction, score, argmax), wall clock;
                   the per-coordinate kernel adds one ppbo_camphor_embed pass over the candidates
  K*, quadform     the same call's "kstar" / "quadform" event brackets (ppbo_profile_*)
  embedding        ppbo_camphor_embed of the 65536 candidates alone, wall clock
  Gram             Engine.gram of the design, wall clock (the per-coordinate kernel includes the design's embedding)
  mu_star          Engine.mean_search_multi: 3 trials over a 65536-row pool, the design and x_prev, 32 ascents per trial
  fit              Engine.gp_fit from the stored start
  evidence         GPModel.evidence (Gram, inverse, f_MAP from a prior draw, LU), wall clock
  evidence_grad    GPModel.evidence_grad at the same theta and start (per-coordinate kernel only; the scalar camphor
                   kernel has no gradient), reported as a multiple of the same kernel's evidence()

Output: one line per quantity, medians in ms, ratios to the scalar kernel and the (min-max) over the rounds.

usage: python tools/camphor_ard_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ppbo_amd.engine import SCORE_POINTWISE_EI, camphor_lengthscales, get_engine  # noqa: E402

CAM, SCALAR = "camphor_copper_ard_kernel", "camphor_copper_kernel"


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


def event_ms(eng, fn, name, reps=10):
    fn()
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(reps):
        fn()
    tot, cnt = eng.profile_read(name)
    eng.profile(False)
    return tot / max(cnt, 1)


def _gp(X, m, kernel, theta):
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    st = PPBO_settings(D=6, bounds=((0, 1),) * 6, xi_acquisition_function="EI-EXT-FAST", kernel=kernel, m=m,
                       theta_initial=theta, verbose=False)
    gp = GPModel(st)
    gp.X, gp.N = np.asarray(X, dtype=float), X.shape[0]
    gp._dX = gp.eng.dev(gp.X)
    gp.theta = theta
    gp.update_Sigma(theta)
    return gp


def main(rounds=3, out_file=None):
    eng = get_engine(0)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    c5 = dict(np.load(os.path.join(root, "c5.npz")))
    X, m, th = c5["X"], int(c5["m"]), [float(t) for t in c5["theta"]]
    spread = np.array([0.1, 0.1, 0.5, 1.0, 1.0, 1.0]) * (th[1] / 0.3)
    cases_k = {"scalar": (SCALAR, th), "ARD prof": (CAM, th), "ARD 10x": (CAM, [th[0], spread, th[2]])}
    rng = np.random.default_rng(1)
    Xc = eng.dev(rng.random((65536, 6)))
    pool = eng.dev(rng.random((65536, 6)))
    shifts = rng.random((3, 6))
    xprev = X[0].copy()
    posts, gps = {}, {}
    for k, (kern, t) in cases_k.items():
        r = eng.gp_fit(X, t, kern, m, c5["f_init"])
        posts[k] = eng.posterior(X, t, kern, r["Sigma_inv"], c5["fMAP"], m)
        gps[k] = _gp(X, m, kern, [1.0, t[1], t[2]])
    mustar = float(np.max(c5["mu"]))
    l_prof = camphor_lengthscales(th, 6)

    def step(k):
        return eng.predict(posts[k], Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_var=False, want_mu=False)

    def evidence(k):
        np.random.seed(5)
        return gps[k].evidence(gps[k].theta, None)

    def evidence_grad(k):
        np.random.seed(5)
        return gps[k].evidence_grad(gps[k].theta)

    cases = [
        ("C5 scoring step (Engine.predict, EI, wall)", lambda k: wall_ms(lambda: step(k), reps=10)),
        ("  K* (kstar event)", lambda k: event_ms(eng, lambda: step(k), "kstar")),
        ("  quadratic form (quadform event)", lambda k: event_ms(eng, lambda: step(k), "quadform")),
        ("embedding of 65536 candidates (ppbo_camphor_embed, wall)",
         lambda k: wall_ms(lambda: eng.camphor_embed(Xc, l_prof), reps=20) if k != "scalar" else float("nan")),
        ("Gram (Engine.gram, wall)", lambda k: wall_ms(lambda: eng.gram(X, cases_k[k][1], cases_k[k][0]), reps=10)),
        ("mu_star (mean_search_multi, 3 trials, wall)", lambda k: wall_ms(lambda: eng.mean_search_multi(
            posts[k], pool, shifts, "design", xprev, K=32), reps=5)),
        ("fit (Engine.gp_fit, wall)", lambda k: wall_ms(lambda: eng.gp_fit(
            X, cases_k[k][1], cases_k[k][0], m, c5["f_init"]), reps=3)),
        ("evidence (GPModel.evidence, wall)", lambda k: wall_ms(lambda: evidence(k), reps=3)),
        ("evidence_grad (GPModel.evidence_grad, wall)",
         lambda k: wall_ms(lambda: evidence_grad(k), reps=3) if k != "scalar" else float("nan")),
    ]
    lines = [f"device: {torch.cuda.get_device_name(0)}; C5 shape N = {X.shape[0]}, theta = {th}; spread l = {spread}; "
             f"{rounds} alternating rounds per quantity; medians in ms"]
    print(lines[0], flush=True)
    meds = {}
    for name, fn in cases:
        t = {k: [] for k in cases_k}
        for _ in range(rounds):
            for k in cases_k:
                t[k].append(fn(k))
        med = {k: float(np.median(v)) for k, v in t.items()}
        meds[name] = med
        a = med["scalar"]
        ln = f"{name:58s} " + "  ".join(
            f"{k} {med[k]:8.4f} ({med[k] / a:5.3f}x; {min(t[k]):.4f}-{max(t[k]):.4f})" if np.isfinite(a) else
            f"{k} {med[k]:8.4f} ({min(t[k]):.4f}-{max(t[k]):.4f})" for k in cases_k)
        lines.append(ln)
        print(ln, flush=True)
    ev, eg = meds["evidence (GPModel.evidence, wall)"], meds["evidence_grad (GPModel.evidence_grad, wall)"]
    ln = ("evidence_grad / evidence of the same kernel: " +
          "  ".join(f"{k} {eg[k] / ev[k]:.3f}" for k in ("ARD prof", "ARD 10x")) + "  (finite differences: 7 evidences)")
    lines.append(ln)
    print(ln, flush=True)
    if out_file:
        with open(out_file, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, sys.argv[2] if len(sys.argv) > 2 else None)
