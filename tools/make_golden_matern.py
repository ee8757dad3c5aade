#!/usr/bin/env python3
"""Golden vectors of the Matern-5/2 and Matern-3/2 kernels, produced by running the REFERENCE ITSELF (build container
only; the in-memory shims of tools/make_golden.py, nothing copied).

The reference has no Matern kernel.  Its GPModel resolves the kernel by eval()ing the settings string in the namespace
of its gp_model module (src/gp_model.py:48), so the two kernels below -- the GPy / scikit-learn Matern(nu) definition
in the reference's own call signature and with its expansion-form r^2 (src/kernels.py:3-11) -- are injected into that
namespace in memory, checked against sklearn.gaussian_process.kernels.Matern first.  Then make_golden.run_config runs
unchanged, with F = 0 (the reference has no Matern spectral density), and writes

  tests/golden/matern/<name>.npz     name in {m52_small, m32_small, m52_c2}

(a subdirectory: conftest.golden_names() parametrises the existing suites over the top-level *.npz only, and their
oracle knows no Matern).  Each file also carries the reference's own mu_star (src/gp_model.py:415-439, differential
evolution, np.random.seed(11)) at the stored f_MAP: de_mustar, de_xstar.

usage: python tools/make_golden_matern.py [m52_small m32_small m52_c2]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

OUT = os.path.join(mg.OUT, "matern")

mg.CONFIGS["m52_small"] = dict(D=3, n_q=2, theta=[0.09, 0.3, 0.5], kernel="Matern52_kernel", F=0, ev=True, omap=False)
mg.CONFIGS["m32_small"] = dict(D=4, n_q=4, theta=[0.09, 0.3, 0.5], kernel="Matern32_kernel", F=0, ev=True, omap=False)
mg.CONFIGS["m52_c2"] = dict(D=6, n_q=16, theta=[0.001, 0.26, 0.1], kernel="Matern52_kernel", F=0, ev=False, omap=False)


def _sqdist(X1, X2):
    """r^2 by the expansion |x|^2 + |y|^2 - 2 x.y, clipped at 0 (the form of src/kernels.py:3-11)."""
    X1 = np.atleast_2d(X1)
    X2 = np.atleast_2d(X2)
    a = np.sum(X1 * X1, 1)
    b = np.sum(X2 * X2, 1)
    return np.clip(-2.0 * X1 @ X2.T + (a[:, None] + b[None, :]), 0.0, np.inf)


def Matern52_kernel(X1, X2, theta):
    a = np.sqrt(5.0) * np.sqrt(_sqdist(X1, X2)) / theta[1]
    return theta[2] ** 2 * (1.0 + a + a * a / 3.0) * np.exp(-a)


def Matern32_kernel(X1, X2, theta):
    a = np.sqrt(3.0) * np.sqrt(_sqdist(X1, X2)) / theta[1]
    return theta[2] ** 2 * (1.0 + a) * np.exp(-a)


def check_against_sklearn():
    from sklearn.gaussian_process.kernels import Matern
    rng = np.random.default_rng(0)
    for fn, nu in ((Matern52_kernel, 2.5), (Matern32_kernel, 1.5)):
        for D in (1, 3, 6):
            X1, X2 = rng.random((17, D)), rng.random((11, D))
            th = [0.1, 0.37, 1.3]
            ref = th[2] ** 2 * Matern(length_scale=th[1], nu=nu)(X1, X2)
            got = fn(X1, X2, th)
            err = np.abs(got - ref).max()
            assert err <= 1e-12 * th[2] ** 2, (fn.__name__, D, err)
    print("Matern kernels agree with sklearn Matern(nu) to 1e-12 sigma_f^2", flush=True)


def inject(ref_gp):
    ref_gp.Matern52_kernel = Matern52_kernel
    ref_gp.Matern32_kernel = Matern32_kernel


def add_mustar(name):
    """The reference's differential-evolution mu_star at the stored f_MAP."""
    import gp_model as ref_gp
    import ppbo_settings as ref_settings
    path = os.path.join(OUT, f"{name}.npz")
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    gp, _, _ = mg.build_design(ref_gp, ref_settings, mg.CONFIGS[name])
    assert np.array_equal(np.asarray(gp.X), out["X"])
    gp.set_theta()
    gp.update_Sigma(gp.theta)
    gp.update_Sigma_inv(gp.theta)
    gp.fMAP = out["fMAP"].reshape(-1, 1) if np.ndim(gp.fMAP) == 2 else out["fMAP"].copy()
    np.random.seed(11)
    xstar, mustar, _ = gp.mu_star(1)
    out.update(de_xstar=np.asarray(xstar, dtype=float).ravel(), de_mustar=float(mustar))
    np.savez_compressed(path, **out)
    print(f"[{name}] reference DE mu_star = {float(mustar):.10g}", flush=True)


if __name__ == "__main__":
    from threadpoolctl import threadpool_limits
    check_against_sklearn()
    mg.install_shims()
    import gp_model as _ref_gp  # noqa: E402  (importable only after the shims)
    inject(_ref_gp)
    mg.OUT = OUT
    os.makedirs(OUT, exist_ok=True)
    with threadpool_limits(limits=1):
        for nm in (sys.argv[1:] or ["m52_small", "m32_small", "m52_c2"]):
            t0 = time.time()
            mg.run_config(nm)
            add_mustar(nm)
            print(f"[{nm}] done in {time.time() - t0:.1f}s", flush=True)
