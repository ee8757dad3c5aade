"""The projected edge form on a fixture, in NumPy (the construction itself: tests/var_projection_numpy.py): the estimate
and the certified bound of every 128-row prefix, the error measured over 2048 seeded candidates, and the flops saved.

    python tests/probes/var_projection.py [c3]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import var_projection_numpy as vp          # noqa: E402
from oracle import ppbo_oracle as orc      # noqa: E402


def main(name):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"), allow_pickle=False))
    X, th, kern, m = g["X"], g["theta"], str(g["kernel"]), int(g["m"])
    N, sf2 = X.shape[0], float(th[2]) ** 2
    E = N - N // (m + 1)
    Sigma = orc.gram(X, th, kern)
    Sinv = orc.pd_inverse(Sigma)
    _, lo = vp.efi.star_lambda(g["fMAP"], m, float(th[0]))
    H, W = vp.operators(Sigma, 0.5 * (Sinv + Sinv.T), lo, m)
    ev = np.linalg.eigvalsh(W @ W.T)[::-1]
    print(f"{name}: N = {N}, E = {E}, r_max = {vp.r_max(N, m)}; eigenvalues of C = W W' at #1, 100, 200, 300, 400, 500: "
          + ", ".join(f"{ev[i]:.1e}" for i in (0, 99, 199, 299, 399, 499) if i < N))
    Q = vp.range_basis(W, vp.r_max(N, m))
    K = orc.cross_cov(X, np.random.default_rng(2048).random((2048, X.shape[1])), th, kern)
    est = vp.estimates(W, Q)
    for r in range(vp.PANEL, Q.shape[1] + 1, vp.PANEL):
        full, proj = vp.variance_terms(H, Q[:, :r], K, lo, m)
        print(f"  r = {r:4d}: estimate {est[r] / (1 - vp.SHRINK):.2e}  bound {vp.certified_bound(W, Q[:, :r], sf2) / sf2:.2e}  "
              f"measured max {np.max(full - proj) / sf2:.1e} min {np.min(full - proj) / sf2:.1e} (sf2; largest reduction "
              f"{full.max() / sf2:.1e})  flops {E / (2.0 * r):.2f} x fewer")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c3")
