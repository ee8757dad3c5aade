#!/usr/bin/env python3
"""Engine.loo_answers (leave-one-query-out scores of the answers, ppbo_loo_answers) timed on one device at three shapes

  C3        tests/golden/c3.npz: n_q = 64 stars of b = 32 rows, D = 20, SE
  default   the reference's default star, n_q = 80, b = 26 (oracle.synthetic_design, D = 20, C3's hyper-parameters)
  C5        tests/golden/c5.npz: n_q = 128, b = 32, camphor-copper

with S = 4096 draws, against (a) Engine.posterior of the same model with P asked for -- the call that precedes it -- and
(b) Engine.line_acq on the same B x G x S (the design's own stars as the groups), whose plan the scoring kernel follows:
whole calls, and the "line_mc" event bracket, which holds line_mc_kernel in one and answer_score_kernel in the other.
All calls alternate in one process so that clock drift falls on all of them.

Then, for DESIGN section 8's open question, GPModel.loo_score against GPModel.evidence along a common factor on the six
length scales of tests/golden/camphor_ard/spread.npz.  Nothing is asserted on that curve.

usage: python tools/answer_scores_time.py [rounds] [out_file]      (default out_file: profiles/r29_answer_scores.txt)
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from oracle import ppbo_oracle as orc  # noqa: E402
from ppbo_amd.engine import get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
S = 4096


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _bracket(eng, fn, slot, reps=10):
    eng.profile(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    tot, cnt = eng.profile_read(slot)
    eng.profile(False)
    return tot / reps if cnt else float("nan")


def _shapes(eng):
    c3 = dict(np.load(os.path.join(GOLDEN, "c3.npz")))
    th3 = [float(t) for t in c3["theta"]]
    yield "C3", c3["X"], th3, str(c3["kernel"]), int(c3["m"]), c3["fMAP"]
    X = orc.synthetic_design(80, 20, m=25, seed=0)
    f = eng.gp_fit(X, th3, "SE_kernel", 25, np.zeros(len(X)), gtol=1e-6)["fMAP"]
    yield "default", X, th3, "SE_kernel", 25, f
    c5 = dict(np.load(os.path.join(GOLDEN, "c5.npz")))
    yield "C5", c5["X"], [float(t) for t in c5["theta"]], str(c5["kernel"]), int(c5["m"]), c5["fMAP"]


def timings(eng, rounds, out):
    out(f"loo_answers, S = {S} draws: median of {rounds} alternating rounds [min .. max], ms")
    for name, X, th, kern, m, f in _shapes(eng):
        b = m + 1
        n_q, D = X.shape[0] // b, X.shape[1]
        Xd, fd = eng.dev(X), eng.dev(f).reshape(-1)
        Sinv = eng.pd_inverse(eng.gram(Xd, th, kern))
        post = eng.posterior(Xd, th, kern, Sinv, fd, m, want_P=True)
        z = eng.randn(7, S, b)
        jit = 1e-10 * th[2] ** 2
        grid = eng.dev(X.reshape(n_q, b, D))
        calls = {
            "posterior (with P)": lambda: eng.posterior(Xd, th, kern, Sinv, fd, m, want_P=True),
            "loo_answers": lambda: eng.loo_answers(post.P, fd, m, th[0], z=z, jitter=jit),
            "  closed form only": lambda: eng.loo_answers(post.P, fd, m, th[0], S=0, jitter=jit),
            "line_acq": lambda: eng.line_acq(post, grid, z, 0.0, jitter=jit),
            "score_answers": lambda: eng.score_answers(post, grid, z=z, jitter=jit),
        }
        for _ in range(3):
            for fn in calls.values():
                fn()
        t = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                t[k].append(_ms(fn))
        md = {k: float(np.median(v)) for k, v in t.items()}
        r = calls["loo_answers"]()
        info = r["info"].cpu().numpy()
        out(f"  {name}: n_q = {n_q}, b = {b}, N = {n_q * b}, D = {D}, {kern}, operator form {post.form}; info != 0 in "
            f"{int((info != 0).sum())} stars, sum lpd = {float(r['lpd'].sum()):.6f}, "
            f"agreement in [{float(r['agreement'].min()):.4f}, {float(r['agreement'].max()):.4f}]")
        for k, v in t.items():
            out(f"    {k:20s} {md[k]:8.3f}  [{min(v):.3f} .. {max(v):.3f}]")
        mc_loo = _bracket(eng, calls["loo_answers"], "line_mc")
        mc_acq = _bracket(eng, calls["line_acq"], "line_mc")
        out(f"    (a) loo_answers / posterior = {md['loo_answers'] / md['posterior (with P)']:.3f}")
        out(f"    (b) loo_answers / line_acq  = {md['loo_answers'] / md['line_acq']:.3f} whole calls; the Monte-Carlo launch "
            f"alone (event bracket line_mc): answer_score_kernel {mc_loo:.3f} ms, line_mc_kernel {mc_acq:.3f} ms, "
            f"ratio {mc_loo / mc_acq:.3f}")
        out(f"        the cavity, the closed form and the launches around them: {md['  closed form only']:.3f} ms")


def curve(out):
    """loo_score against the evidence along a common factor on the length scales of camphor_ard/spread."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    g = dict(np.load(os.path.join(GOLDEN, "camphor_ard", "spread.npz")))
    D, m = int(g["D"]), int(g["m"])
    sig, sf, l = float(g["theta_sf"][0]), float(g["theta_sf"][1]), np.asarray(g["theta_l"], dtype=float)
    st = PPBO_settings(D=D, bounds=((0.0, 1.0),) * D, xi_acquisition_function="PCD", theta_initial=[sig, l.copy(), sf], m=m,
                       verbose=False, kernel="camphor_copper_ard_kernel")
    gp = GPModel(st)
    np.random.seed(0)
    gp.update_feedback_processing_object(g["X_obs"])
    gp.FP.X = g["X"].copy()
    gp.update_data()
    gp.initialization_running = False
    gp.set_theta()
    gp.update_Sigma(gp.theta)
    gp.update_Sigma_inv(gp.theta)
    gp.fMAP = g["fMAP"].copy()
    out(f"camphor_ard/spread (N = {g['X'].shape[0]}, l = {l.tolist()}): loo_score (4096 draws, seed 1; the sum over "
        f"{g['X'].shape[0] // (m + 1)} queries) and evidence (log-prior included) at theta = [sigma, c l, sigma_f]")
    out("       c      loo_score      evidence")
    for c in (0.1, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0):
        th = [sig, c * l, sf]
        try:
            loo = gp.loo_score(th, n_draws=4096, seed=1)
        except Exception as e:  # noqa: BLE001  (a row that cannot be fitted is a finding, not the end of the run)
            loo = f"failed: {type(e).__name__}: {e}"
        try:
            np.random.seed(1)
            ev = gp.evidence(th, None)
        except Exception as e:  # noqa: BLE001
            ev = f"failed: {type(e).__name__}: {e}"
        out(f"  {c:6.2f}  {loo if isinstance(loo, str) else format(loo, '13.6f')}  {ev if isinstance(ev, str) else format(ev, '12.4f')}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 15
    path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "r29_answer_scores.txt")
    fh = open(path, "w")

    def out(line):
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    eng = get_engine(0)
    timings(eng, rounds, out)
    out("")
    curve(out)
    fh.close()


if __name__ == "__main__":
    main()
