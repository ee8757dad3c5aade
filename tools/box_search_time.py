#!/usr/bin/env python3
"""Engine.mean_search_boxes (ppbo_mean_search_boxes) timed on one device, in one process, on the fitted C2 and C3 models
(tests/golden/c2.npz, c3.npz).

  unit     T = 3 unit boxes over a pool of 65536 rows, K = 32, fp32 screening, against Engine.mean_search_multi (the
           parent commit's own entry, unchanged here) on the same pool and shifts, the two in turn within every round.
           The margin is mean_search_multi's own min .. max over the rounds.  Stage shares by differences of calls:
           screening = the call at K = 1, iters = 0; selection = K = 32, iters = 0 minus that; ascent = the rest.
  profile  T = 33 boxes fixing one coordinate and T = 1089 fixing two (a 33 x 33 grid), K = 8, M = 4096, seeded with the
           slice points: ms per call and per box, stage shares as above.  Against the parent's only route to a
           conditional optimum, a GPModel._polish-style SciPy L-BFGS-B in the same box from the slice point, one start,
           one device round trip per function value -- timed on 33 boxes of each set (a ratio to report, not a gate).

  call     event time of REPS back-to-back calls (device-resident inputs, workspaces warm), median of the rounds

usage: python tools/box_search_time.py [rounds] [out_file]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import scipy.optimize
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from ppbo_amd.engine import get_engine  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REPS = 5


def _model(eng, name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))
    th = [float(t) for t in g["theta"]]
    r = eng.gp_fit(g["X"], th, str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    return r["post"], g["X"].shape[1]


def _ms(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _rounds(calls, rounds):
    for fn in calls.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():              # in turn: clock drift falls on all of them
            t[k].append(_ms(fn))
    return t


def _line(k, v):
    return f"    {k:34s} {np.median(v):9.4f}  [{min(v):.4f} .. {max(v):.4f}]"


def _polish_ms(eng, post, boxes, starts):
    """L-BFGS-B in each box from its start, as GPModel._polish: wall ms per box and the values reached."""
    vals = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b, x0 in zip(boxes, starts):
        lo, hi = b

        def fg(x):
            mu, g = eng.mean_grad(post, np.clip(x, lo, hi)[None, :])
            return -float(mu.cpu().numpy()[0]), -g.cpu().numpy()[0]
        res = scipy.optimize.minimize(fg, np.clip(x0, lo, hi), jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                                      options={"maxiter": 200, "ftol": 1e-15, "gtol": 1e-10})
        vals.append(-float(res.fun))
    return (time.perf_counter() - t0) * 1e3 / len(boxes), np.array(vals)


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
    for name in ("c2", "c3"):
        post, D = _model(eng, name)
        N = post.X.shape[0]
        gen = torch.Generator(device=eng.device).manual_seed(1)
        pool = torch.rand((65536, D), dtype=torch.float64, device=eng.device, generator=gen)
        rng = np.random.default_rng(2)
        # ---- unit boxes against mean_search_multi
        T, K = 3, 32
        shifts = rng.random((T, D))
        unit = np.tile(np.stack([np.zeros(D), np.ones(D)]), (T, 1, 1))
        kw = dict(sep=0.05, tol=1e-9, screen_fp32=True)
        calls = {
            "mean_search_multi (parent's entry)": lambda: eng.mean_search_multi(post, pool, shifts, None, None, K=K, iters=100, **kw),
            "mean_search_boxes, unit boxes": lambda: eng.mean_search_boxes(post, pool, unit, shifts=shifts, K=K, iters=100, **kw),
            "  boxes: K = 1, iters = 0": lambda: eng.mean_search_boxes(post, pool, unit, shifts=shifts, K=1, iters=0, **kw),
            "  boxes: K = 32, iters = 0": lambda: eng.mean_search_boxes(post, pool, unit, shifts=shifts, K=K, iters=0, **kw),
            "  multi: K = 32, iters = 0": lambda: eng.mean_search_multi(post, pool, shifts, None, None, K=K, iters=0, **kw),
        }
        t = _rounds(calls, rounds)
        keys = list(calls)
        out(f"{name.upper()}: N = {N}, D = {D}; unit boxes: T = {T}, M = {pool.shape[0]}, K = {K}, 100 iterations, fp32 screening; "
            f"ms per call, median of {rounds} rounds of {REPS}  [min .. max]")
        for k in keys:
            out(_line(k, t[k]))
        par, box = t[keys[0]], t[keys[1]]
        ratio = np.median(box) / np.median(par)
        verdict = ("inside" if min(par) <= np.median(box) <= max(par) else "below it (faster)" if np.median(box) < min(par)
                   else "ABOVE it (the lines below say which launches carry it)")
        out(f"    boxes / multi = {ratio:.3f}; the parent call's own spread is {min(par) / np.median(par):.3f} .. "
            f"{max(par) / np.median(par):.3f}: {verdict}")
        scr, sel = np.median(t[keys[2]]), np.median(t[keys[3]]) - np.median(t[keys[2]])
        asc = np.median(box) - np.median(t[keys[3]])
        out(f"    stages of the boxed call: screening {scr:.4f}, selection {sel:.4f}, ascent {asc:.4f} ms; up to the ascent: "
            f"boxes {np.median(t[keys[3]]):.4f}, multi {np.median(t[keys[4]]):.4f}; the ascent launch: boxes {asc:.4f}, multi "
            f"{np.median(par) - np.median(t[keys[4]]):.4f}")
        xm, mm = eng.mean_search_multi(post, pool, shifts, None, None, K=K, iters=100, **kw)
        xb, mb, _ = eng.mean_search_boxes(post, pool, unit, shifts=shifts, K=K, iters=100, **kw)
        bx_ = -(-pool.shape[0] // 1024)                  # screening workgroups per trial and row split
        split = [min(16, -(-2048 // (bx_ * nb)), -(-N // 64)) for nb in (1, T)]
        out(f"    outputs: mu bitwise equal {bool(torch.equal(mm, mb))}, best per trial equal "
            f"{bool(torch.equal(mm.max(dim=1).values, mb.max(dim=1).values))} (row splits of the fp32 screening: boxes {split[0]}, "
            f"multi {split[1]})")
        # ---- profiles
        sub = pool[:4096].contiguous()
        xs, ms_, _ = eng.mean_search_boxes(post, pool, unit[:1], K=K, iters=100, **kw)
        xstar = xs[0, int(torch.argmax(ms_[0]))].cpu().numpy()
        g33 = np.linspace(0.0, 1.0, 33)
        sets = {"one fixed coordinate, T = 33": ([0], g33.reshape(-1, 1)),
                "two fixed coordinates, T = 1089": ([0, 1], np.stack(np.meshgrid(g33, g33, indexing="ij"), axis=-1).reshape(-1, 2))}
        for label, (dims, vals) in sets.items():
            Tn = vals.shape[0]
            boxes = np.tile(np.stack([np.zeros(D), np.ones(D)]), (Tn, 1, 1))
            boxes[:, :, dims] = vals[:, None, :]
            seeds = np.tile(xstar[None, None, :], (Tn, 1, 1))
            seeds[:, :, dims] = vals[:, None, :]
            seeds_d = eng.dev(seeds)
            pc = {
                "profile": lambda: eng.mean_search_boxes(post, sub, boxes, seeds=seeds_d, K=8, iters=100, **kw),
                "  K = 1, iters = 0": lambda: eng.mean_search_boxes(post, sub, boxes, seeds=seeds_d, K=1, iters=0, **kw),
                "  K = 8, iters = 0": lambda: eng.mean_search_boxes(post, sub, boxes, seeds=seeds_d, K=8, iters=0, **kw),
            }
            tp = _rounds(pc, rounds)
            pk = list(pc)
            out(f"  profile, {label}: M = 4096, K = 8, one seed (the slice point); ms per call")
            for k in pk:
                out(_line(k, tp[k]))
            full, s0, s1 = (np.median(tp[k]) for k in pk)
            out(f"    per box {full / Tn * 1e3:.2f} us; shares: screening {s0 / full:.2f}, selection {(s1 - s0) / full:.2f}, "
                f"ascent {(full - s1) / full:.2f}")
            pick = np.linspace(0, Tn - 1, 33).astype(int)
            per_box, v_polish = _polish_ms(eng, post, boxes[pick], seeds[pick, 0])
            _, mu_d, _ = eng.mean_search_boxes(post, sub, boxes, seeds=seeds_d, K=8, iters=100, **kw)
            v_dev = mu_d.max(dim=1).values.cpu().numpy()[pick]
            out(f"    L-BFGS-B in the same boxes from the slice point (33 of them): {per_box:.2f} ms per box, {per_box * Tn:.0f} ms for "
                f"all {Tn}; ratio to the profile call {per_box * Tn / full:.0f}x; the device's value is the higher one in "
                f"{int((v_dev >= v_polish - 1e-12 * np.abs(v_polish).max()).sum())} of 33 boxes")
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
