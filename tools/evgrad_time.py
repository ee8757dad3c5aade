"""Cost of the Laplace-evidence gradient against one evidence (GPModel.evidence_grad vs evidence()'s core) at the C2
(N = 512, D = 6) and C3 (N = 2048, D = 20) shapes, per-dimension length scales, SE kernel; the device entry alone
against ppbo_laplace_logdet on the same state; the A^-1 product's share of the fp64 MFMA peak.

    python tools/evgrad_time.py [--reps 10] [--shapes c2,c3]

Under `rocprofv3 --kernel-trace --stats -- python tools/evgrad_time.py --reps 3` the evg_* kernels appear by name."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c2": (16, 6, 31), "c3": (64, 20, 31)}     # (queries, D, m): N = queries * (m + 1)
FP64_MFMA_PEAK = 78.6e12                              # MI355X dense fp64 matrix peak, FLOP/s


def main():
    import torch
    from oracle import ppbo_oracle as orc
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="c2,c3")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        n_q, D, m = SHAPES[name]
        X = orc.synthetic_design(n_q, D, m=m, seed=0)
        th = [1.0, np.geomspace(0.3, 1.5, D), 2.0]
        st = PPBO_settings(D=D, bounds=((0, 1),) * D, xi_acquisition_function="EI-EXT-FAST", m=m, theta_initial=th,
                           verbose=False)
        gp = GPModel(st)
        gp.X, gp.N = X, X.shape[0]
        gp._dX = gp.eng.dev(X)
        gp.update_Sigma(th)
        eng = gp.eng
        np.random.seed(1)
        f0 = gp._draw_prior()
        _, _, _, _, fm = gp.evidence_grad(th, f_initial=f0)       # warm-up, and a converged start for the timings
        sync = torch.cuda.synchronize

        def clock(fn):
            fn()
            sync()
            t = time.perf_counter()
            for _ in range(a.reps):
                fn()
            sync()
            return (time.perf_counter() - t) / a.reps * 1e3

        t_ev = clock(lambda: gp._evidence_core(eng, th, f0))
        t_gr = clock(lambda: gp.evidence_grad(th, f_initial=f0))
        Sig, Sinv, fmap, _, ld, lo = gp._evidence_fit(eng, th, fm)
        t_ld = clock(lambda: eng.laplace_logdet(Sig, ld, lo, m))
        t_eg = clock(lambda: eng.evidence_grad(X, th, "SE_kernel", Sig, Sinv, fmap, ld, lo, m))
        # the A^-1 product alone (N^3 multiply-adds, a full GEMM on the fp64 matrix cores), same shape and transposition
        N = X.shape[0]
        A, B = torch.rand(N, N, dtype=torch.float64, device=eng.device), torch.rand(N, N, dtype=torch.float64,
                                                                                    device=eng.device)
        Cm = torch.empty_like(A)
        t_mm = clock(lambda: eng.dgemm(A, B, transA=True, C_out=Cm))
        print(json.dumps(dict(shape=name, N=N, D=D, m=m, reps=a.reps, evidence_ms=round(t_ev, 3),
                              evidence_grad_ms=round(t_gr, 3), ratio=round(t_gr / t_ev, 3),
                              laplace_logdet_ms=round(t_ld, 3), evidence_grad_entry_ms=round(t_eg, 3),
                              ainv_gemm_ms=round(t_mm, 4),
                              ainv_gemm_share_of_fp64_mfma_peak=round(2.0 * N ** 3 / (t_mm * 1e-3) / FP64_MFMA_PEAK, 3))),
              flush=True)


if __name__ == "__main__":
    main()
