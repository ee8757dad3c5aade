"""CPU: the Laplace-evidence gradient -- its NumPy restatement (tests/evgrad_numpy.py) against central
differences of the oracle-built evidence with Newton-converged f_MAP, the new C-ABI entry in the header, the linker
version script and the built library, the log-prior's gradient and the theta_optimizer setting."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import evgrad_numpy as eg
from conftest import ROOT
from oracle import ppbo_oracle as orc

RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")


def _case(kernel, theta, seed, n_q=10, D=3, m=3):
    X = orc.synthetic_design(n_q, D, m=m, seed=seed)
    rs = np.random.RandomState(seed)
    f0 = np.linalg.cholesky(eg.sigma_matrix(X, theta, kernel)) @ rs.standard_normal(X.shape[0])
    _, f = eg.evidence(X, theta, kernel, m, f0)
    return X, m, f


def _central(X, theta, kernel, m, f, rel_h=1e-5):
    p = eg.params(theta)
    fd, signs = np.empty_like(p), []
    for k in range(p.size):
        h = rel_h * p[k]
        vals = []
        for sgn in (1.0, -1.0):
            q = p.copy()
            q[k] += sgn * h
            th = eg.with_params(theta, q)
            v, fq = eg.evidence(X, th, kernel, m, f)          # warm-started at the centre's f_MAP
            Sig = eg.sigma_matrix(X, th, kernel)
            signs.append(eg.slogdet_lu(np.eye(len(f)) + Sig @ orc.lambda_dense(fq, m, th[0]))[0])
            vals.append(v)
        fd[k] = (vals[0] - vals[1]) / (2.0 * h)
    return fd, signs


@pytest.mark.parametrize("kernel", RADIAL)
@pytest.mark.parametrize("ard", [False, True])
def test_restatement_matches_central_differences(kernel, ard):
    theta = [1.0, np.array([0.3, 0.6, 1.2]) if ard else 0.5, 2.0 if ard else 3.0]
    X, m, f = _case(kernel, theta, seed=1 if ard else 2)
    g, sU = eg.evidence_grad(X, theta, kernel, m, f)
    fd, signs = _central(X, theta, kernel, m, f)
    assert all(s == sU for s in signs)            # no pivot-sequence change inside the stencil
    assert g.shape == ((4,) if ard else (2,))
    assert np.max(np.abs(g - fd) / np.abs(fd)) <= 1e-5


def test_sign_comes_from_the_lu_not_the_determinant():
    # Matern-5/2 at this point: the LU's prod sign(u_kk) is +1 while det A < 0 (an odd pivot permutation)
    kernel, theta = "Matern52_kernel", [1.0, 0.5, 3.0]
    X, m, f = _case(kernel, theta, seed=2)
    Sig = eg.sigma_matrix(X, theta, kernel)
    sU, _, sdet = eg.slogdet_lu(np.eye(len(f)) + Sig @ orc.lambda_dense(f, m, theta[0]))
    assert sU != sdet
    g, sU2 = eg.evidence_grad(X, theta, kernel, m, f)
    assert sU2 == sU
    fd, _ = _central(X, theta, kernel, m, f)
    assert np.max(np.abs(g - fd) / np.abs(fd)) <= 1e-5
    # the determinant's sign in its place gives a gradient that does not match the objective
    g_det, _ = eg.evidence_grad(X, theta, kernel, m, f, sign=sdet)
    assert np.max(np.abs(g_det - fd) / np.abs(fd)) > 1e-2


def test_header_version_script_and_library_list_the_entry():
    from ppbo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"PPBO_API int ppbo_evidence_grad\(", hdr)
    assert "ppbo_evidence_grad" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 9
    vs = open(os.path.join(ROOT, "ppbo_amd", "csrc", "libppbo_hip.map")).read()
    pats = [p.strip() for p in vs.split("global:")[1].split("local:")[0].split(";") if p.strip()]
    assert any(fnmatch.fnmatch("ppbo_evidence_grad", p) for p in pats)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libppbo_hip.so is not built (build() runs before the suite)")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "ppbo_evidence_grad" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("theta", [[1.0, 0.3, 2.0], [0.7, np.array([0.05, 0.4, 1.9]), 12.0]])
def test_log_prior_gradient(theta):
    from ppbo_amd.gp_model import log_prior, log_prior_grad
    g = log_prior_grad(theta)
    p = eg.params(theta)
    fd = np.empty_like(p)
    for k in range(p.size):
        h = 1e-6 * p[k]
        q1, q2 = p.copy(), p.copy()
        q1[k] += h
        q2[k] -= h
        fd[k] = (log_prior(eg.with_params(theta, q1)) - log_prior(eg.with_params(theta, q2))) / (2 * h)
    assert np.allclose(g, fd, rtol=1e-7, atol=1e-9)
    assert np.allclose(g, eg.log_prior_grad(theta), rtol=1e-14)


def test_theta_optimizer_setting():
    from ppbo_amd.ppbo_settings import PPBO_settings
    bounds = ((0, 1),) * 3
    assert PPBO_settings(3, bounds, "EI").theta_optimizer == "search"
    assert PPBO_settings(3, bounds, "EI", theta_optimizer="ard-gradient").theta_optimizer == "ard-gradient"
    for bad in ("ard", "gradient", "", None):
        with pytest.raises(ValueError):
            PPBO_settings(3, bounds, "EI", theta_optimizer=bad)
