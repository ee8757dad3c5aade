#!/usr/bin/env python3
"""Engine.predict_gradients (mean and D x D covariance of grad f at M points) against the only earlier route to the same
matrix -- polarisation from D (D + 1) / 2 rows of Engine.predict_slopes per point -- and its column pass against a plain
streaming store of the same bytes, on one device, in one process.

  C3 (tests/golden/c3.npz: N = 2048, D = 20) and C2 (tests/golden/c2.npz), M = 512 points (one chunk)

  call     event time of REPS back-to-back calls (device-resident inputs, workspaces warm), median of the rounds, the
           two routes and the store floor in turn so that clock drift falls on all of them
  floor    ppbo_store_floor on a square matrix of n x n doubles with n^2 the nearest to N x M D, the bytes the column
           pass writes; scaled to the exact byte count
  stages   the library's event brackets "grad_kstar", "line_y", "line_cov", "grad_finish" in a separate pass

predict_slopes is the parent commit's own device code, so the ratio is against the parent in the same run.

usage: python tools/gradients_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import GRAD_NORM2, SLOPE_VARIANCE, get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
M, REPS = 512, 10
SLOTS = ("grad_kstar", "line_y", "line_cov", "grad_finish")


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1]


def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / REPS


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
    for name in ("c3", "c2"):
        post, D = _model(eng, name)
        N = post.X.shape[0]
        gen = torch.Generator(device=eng.device).manual_seed(1)
        X = torch.rand((M, D), dtype=torch.float64, device=eng.device, generator=gen)
        ia, ib = np.triu_indices(D)
        E = np.eye(D)
        Xi = eng.dev(np.tile(np.where((ia == ib)[:, None], E[ia], E[ia] + E[ib]), (M, 1)))
        Xr = X.repeat_interleave(ia.size, dim=0).contiguous()
        n = 2 * int(round(np.sqrt(float(N) * M * D) / 2.0))     # (ppbo_store_floor takes an even n)
        S = eng.empty(n, n)
        calls = {
            "gradients": lambda: eng.predict_gradients(post, X, score=GRAD_NORM2, want_score=True, want_best=False),
            "gradients, mean alone": lambda: eng.predict_gradients(post, X, want_cov=False, want_best=False),
            "slopes": lambda: eng.predict_slopes(post, Xr, Xi, score=SLOPE_VARIANCE, want_prob=False, want_best=False),
            "floor": lambda: eng.store_floor(S),
        }
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                t[k].append(_ms(fn))
        md = {k: float(np.median(v)) for k, v in t.items()}
        out(f"{name.upper()}: N = {N}, D = {D}, operator form {post.form}, M = {M} points = {M * D} columns; "
            f"polarisation: {ia.size} slope rows per point = {M * ia.size} rows; ms per call, median of {rounds} rounds of {REPS}")
        for k in calls:
            out(f"    {k:24s} {md[k]:9.4f}  [{min(t[k]):.4f} .. {max(t[k]):.4f}]")
        floor = md["floor"] * (float(N) * M * D) / (float(n) * n)
        out(f"    predict_slopes polarisation / predict_gradients = {md['slopes'] / md['gradients']:.2f}")
        eng.profile(True)
        eng.profile_reset()
        for _ in range(REPS):
            calls["gradients"]()
        torch.cuda.synchronize()
        br = {}
        for s in SLOTS:
            tot, cnt = eng.profile_read(s)
            br[s] = tot / REPS if cnt else float("nan")
        eng.profile(False)
        out("    stages, ms per call: " + ", ".join(f"{s} {v:.4f}" for s, v in br.items()))
        out(f"    store floor for {N * M * D * 8 / 1e6:.1f} MB: {floor:.4f} ms;  column pass / floor = {br['grad_kstar'] / floor:.2f}")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
