#!/usr/bin/env python3
"""Golden vectors of the camphor-copper kernel with one length scale per coordinate, produced by running the REFERENCE
ITSELF (build container only; the in-memory shims of tools/make_golden.py, nothing copied).

The reference's camphor-copper kernel takes one length scale l (z at l + 0.05).  Its GPModel resolves the kernel by
eval()ing the settings string in the namespace of its gp_model module (src/gp_model.py:48), so a per-coordinate form --
in the reference's call signature, theta = [sigma, l, sigma_f] with l = (l_x, l_y, l_z, l_alpha, l_beta, l_gamma),
  k = sigma_f^2 exp(- sum_{d != 2} (2 / l_d^2) sin^2(pi |x_d - x'_d|) - (x_2 - x'_2)^2 / (2 l_2^2)),
written out here from that formula -- is injected into that namespace under the name camphor_copper_kernel, checked
first against the reference's own kernel at the profile (l, l, l + 0.05, l, l, l).  The reference's own fit
(update_Sigma, update_Sigma_inv, update_fMAP from a stored start), posterior (update_model :111-117), mu_Sigma_pred and
line EI (src/acquisition.py:72-81) then run unchanged and write

  tests/golden/camphor_ard/<name>.npz     name in {spread}

with theta_sf = [sigma, sigma_f] and theta_l = the six length scales (translations 0.1, z 0.5, angles 1.0: spread 10x).
The evidence is not pinned here (the reference's log_prior takes one l); the GPU tests pin it against the scalar kernel.

usage: python tools/make_golden_camphor_ard.py [spread]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_ard as mga  # noqa: E402

OUT = os.path.join(mg.OUT, "camphor_ard")

CONFIGS = {
    "spread": dict(D=6, n_q=6, theta=[0.05, np.array([0.1, 0.1, 0.5, 1.0, 1.0, 1.0]), 0.4],
                   kernel="camphor_copper_kernel"),
}


def camphor_copper_ard(X1, X2, theta):
    X1, X2 = np.atleast_2d(X1), np.atleast_2d(X2)
    l = np.asarray(theta[1], dtype=float)
    s = np.zeros((X1.shape[0], X2.shape[0]))
    for d in range(6):
        dx = X1[:, d][:, None] - X2[:, d][None, :]
        if d == 2:
            s += 0.5 * dx * dx / l[2] ** 2
        else:
            s += (2.0 / l[d] ** 2) * np.sin(np.pi * np.abs(dx)) ** 2
    return theta[2] ** 2 * np.exp(-s)


def check_against_the_reference():
    import kernels as ref_k
    rng = np.random.default_rng(0)
    X1, X2 = rng.random((17, 6)), rng.random((11, 6))
    for l in (0.1, 0.26, 1.3):
        th = [0.1, l, 1.3]
        prof = l + np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0])
        err = np.abs(camphor_copper_ard(X1, X2, [0.1, prof, 1.3]) - ref_k.camphor_copper_kernel(X1, X2, th)).max()
        assert err <= 1e-12 * th[2] ** 2, (l, err)
    print("the per-coordinate form at the profile agrees with the reference's camphor_copper_kernel to 1e-12 sigma_f^2",
          flush=True)


if __name__ == "__main__":
    from threadpoolctl import threadpool_limits
    mg.install_shims()
    import gp_model as _ref_gp  # noqa: E402  (importable only after the shims)
    check_against_the_reference()
    _ref_gp.camphor_copper_kernel = camphor_copper_ard
    mga.OUT = OUT
    mga.CONFIGS = CONFIGS
    os.makedirs(OUT, exist_ok=True)
    with threadpool_limits(limits=1):
        for nm in (sys.argv[1:] or list(CONFIGS)):
            t0 = time.time()
            mga.run(nm)
            print(f"[{nm}] done in {time.time() - t0:.1f}s", flush=True)
