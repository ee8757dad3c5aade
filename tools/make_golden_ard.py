#!/usr/bin/env python3
"""Golden vectors of per-dimension length scales (ARD), produced by running the REFERENCE ITSELF (build container only;
the in-memory shims of tools/make_golden.py, nothing copied).

The reference's kernels take one length scale.  Its GPModel resolves the kernel by eval()ing the settings string in the
namespace of its gp_model module (src/gp_model.py:48), so ARD forms of SE and Matern-5/2 -- in the reference's call
signature, theta = [sigma, l, sigma_f] with l a length-D vector, r^2 = sum_d (x_d - x'_d)^2 / l_d^2 by the expansion
of src/kernels.py:3-11 on the scaled inputs -- are injected into that namespace under the names SE_kernel and
Matern52_kernel, checked against sklearn's anisotropic RBF / Matern first.  The reference's own fit (update_Sigma,
update_Sigma_inv, update_fMAP from a stored start), posterior (update_model :111-117), mu_Sigma_pred and line EI
(src/acquisition.py:72-81) then run unchanged and write

  tests/golden/ard/<name>.npz     name in {se_d4, m52_d6}

with theta_sf = [sigma, sigma_f] and theta_l = the length scales (spread over more than 20x).  The evidence is NOT pinned
here: the reference's log_prior (src/gp_model.py:287-290) cannot take a vector l, so the GPU tests pin the ARD evidence
by its identities instead (equal entries against a scalar l: the log-evidence is the same, the prior differs by
(D - 1) log p(l)).

usage: python tools/make_golden_ard.py [se_d4 m52_d6]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

OUT = os.path.join(mg.OUT, "ard")

CONFIGS = {
    "se_d4": dict(D=4, n_q=6, theta=[0.09, np.array([0.05, 0.3, 0.6, 1.2]), 0.5], kernel="SE_kernel"),
    "m52_d6": dict(D=6, n_q=8, theta=[0.05, np.array([0.08, 0.2, 0.35, 0.5, 1.0, 2.0]), 0.4], kernel="Matern52_kernel"),
}


def _sqdist_scaled(X1, X2, l):
    """sum_d (x_d - x'_d)^2 / l_d^2 by the expansion |u|^2 + |v|^2 - 2 u.v of u = x / l, clipped at 0."""
    U = np.atleast_2d(X1) / l
    V = np.atleast_2d(X2) / l
    a = np.sum(U * U, 1)
    b = np.sum(V * V, 1)
    return np.clip(-2.0 * U @ V.T + (a[:, None] + b[None, :]), 0.0, np.inf)


def SE_kernel(X1, X2, theta):
    return theta[2] ** 2 * np.exp(-0.5 * _sqdist_scaled(X1, X2, np.asarray(theta[1], dtype=float)))


def Matern52_kernel(X1, X2, theta):
    a = np.sqrt(5.0) * np.sqrt(_sqdist_scaled(X1, X2, np.asarray(theta[1], dtype=float)))
    return theta[2] ** 2 * (1.0 + a + a * a / 3.0) * np.exp(-a)


def check_against_sklearn():
    from sklearn.gaussian_process.kernels import RBF, Matern
    rng = np.random.default_rng(0)
    for D in (2, 4, 6):
        X1, X2 = rng.random((17, D)), rng.random((11, D))
        l = np.geomspace(0.05, 1.5, D)
        th = [0.1, l, 1.3]
        for fn, ref in ((SE_kernel, RBF(length_scale=l)), (Matern52_kernel, Matern(length_scale=l, nu=2.5))):
            err = np.abs(fn(X1, X2, th) - th[2] ** 2 * ref(X1, X2)).max()
            assert err <= 1e-12 * th[2] ** 2, (fn.__name__, D, err)
    print("ARD kernels agree with sklearn's anisotropic RBF / Matern(2.5) to 1e-12 sigma_f^2", flush=True)


def run(name):
    import gp_model as ref_gp
    import ppbo_settings as ref_settings
    import acquisition as ref_acq
    cfg = CONFIGS[name]
    gp, _, X_obs = mg.build_design(ref_gp, ref_settings, cfg)
    N, D = gp.N, gp.D
    rng = np.random.default_rng(7)
    gp.set_theta()
    gp.update_Sigma(gp.theta)
    gp.update_Sigma_inv(gp.theta)
    Sig = gp.Sigma
    f_init = np.random.default_rng(2).multivariate_normal(np.zeros(N), Sig, method="cholesky")
    _mvn = np.random.multivariate_normal
    np.random.multivariate_normal = lambda mean, cov, *a, **k: f_init.copy()
    try:
        gp.fMAP = None
        gp.update_fMAP()
    finally:
        np.random.multivariate_normal = _mvn
    fMAP = np.asarray(gp.fMAP).ravel()
    gp.Lambda_MAP = gp.create_Lambda(gp.fMAP, gp.theta[0])
    gp.posterior_covariance_inv = gp.Sigma_inv - gp.Lambda_MAP
    gp.posterior_covariance = ref_gp.pd_inverse(gp.posterior_covariance_inv)
    Mc = 512
    Xc = rng.random((Mc, D))
    near = gp.X[rng.integers(0, N, Mc // 2)] + 0.02 * rng.standard_normal((Mc // 2, D))
    Xc[Mc // 2:] = np.clip(near, 0, 1)
    mu, Spred = gp.mu_Sigma_pred(Xc)
    # one projective line, its grid / mean / covariance as the reference's EI formed them
    rec = {}
    _msp = gp.mu_Sigma_pred

    def rec_msp(Xp):
        r = _msp(Xp)
        rec["grid"], rec["mu"], rec["cov"] = np.array(Xp), np.asarray(r[0]).ravel(), np.array(r[1])
        return r

    gp.mu_Sigma_pred = rec_msp
    gp.mustar = float(np.max(mu))
    xi = np.zeros(D)
    xi[1] = 1.0
    xl = rng.random(D)
    xl[1] = 0.0
    np.random.seed(123)
    ei_ref = ref_acq.EI(xi, xl, gp, 150)
    gp.mu_Sigma_pred = _msp
    out = dict(name=name, X=np.asarray(gp.X), X_obs=X_obs, theta_sf=np.array([cfg["theta"][0], cfg["theta"][2]]),
               theta_l=np.asarray(cfg["theta"][1], dtype=float), m=gp.m, D=D, N=N, kernel=cfg["kernel"],
               Sigma=np.asarray(Sig), f_init=f_init, fMAP=fMAP, alpha=gp.Sigma_inv.dot(fMAP),
               T_fMAP=float(gp.T(fMAP, gp.theta)), P_diag=np.diag(gp.posterior_covariance).copy(),
               Xc=Xc, mu=np.asarray(mu).ravel(), var=np.diag(Spred).copy(),
               line_xi=xi, line_x=xl, line_grid=rec["grid"], line_mu=rec["mu"], line_cov=rec["cov"],
               line_mustar=gp.mustar, line_ei_ref150=ei_ref)
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)
    print(f"[{name}] N={N} D={D} written", flush=True)


if __name__ == "__main__":
    from threadpoolctl import threadpool_limits
    check_against_sklearn()
    mg.install_shims()
    import gp_model as _ref_gp  # noqa: E402  (importable only after the shims)
    _ref_gp.SE_kernel = SE_kernel
    _ref_gp.Matern52_kernel = Matern52_kernel
    os.makedirs(OUT, exist_ok=True)
    with threadpool_limits(limits=1):
        for nm in (sys.argv[1:] or list(CONFIGS)):
            t0 = time.time()
            run(nm)
            print(f"[{nm}] done in {time.time() - t0:.1f}s", flush=True)
