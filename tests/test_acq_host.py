"""CPU: the NumPy statement of the acquisition gradients (tests/acq_numpy.py) against central differences, the two new
entries in the header and the ctypes binding, and the cap that tests/test_gpu_acq.py asserts of the ascent comparison,
on the reference alone.

Central differences: h = 1e-5 on points at least ~1e-2 from every design row, so the truncation error h^2 f''' / 6 is some
1e-9 of the terms the derivative cancels down from; the bound is 1e-6 of sum_j |J_jd alpha_j| (mean), 2 sum_j |J_jd| |u_j|
(variance) and the weighted sum of the two (score), plus, for the variance, the rounding noise of the difference quotient
itself, 8 eps (sf^2 + |k|' |A| |k|) / h."""
import os
import re

import numpy as np
import pytest

import acq_numpy as aq
import box_search_numpy as bsn
import search_ref as sr
import slopes_numpy as sn
from oracle import ppbo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-5
ARD6 = np.array([0.3, 0.5, 0.8, 1.1, 1.6, 0.6])

# (kernel, D, n_q, m, l): scalar length scales, then per-dimension ones
CASES = {
    "SE": ("SE_kernel", 5, 6, 4, None), "RQ": ("RQ_kernel", 5, 6, 4, None), "Matern52": ("Matern52_kernel", 5, 6, 4, None),
    "Matern32": ("Matern32_kernel", 5, 6, 4, None), "camphor": ("camphor_copper_kernel", 6, 6, 4, 1.0),
    "SE-ard": ("SE_kernel", 6, 6, 4, ARD6), "RQ-ard": ("RQ_kernel", 6, 6, 4, ARD6),
    "Matern52-ard": ("Matern52_kernel", 6, 6, 4, ARD6), "Matern32-ard": ("Matern32_kernel", 6, 6, 4, ARD6),
    "camphor-ard": (sn.CAMPHOR_ARD, 6, 6, 4, sr.CAMPHOR_LS),
}
_MODELS = {}


def _model(name):
    """A tiny host-fitted model (search_ref.host_fit): dict(X, th, kernel, alpha, A, Sinv, f, P, m)."""
    if name not in _MODELS:
        kernel, D, n_q, m, l = CASES[name]
        X = orc.synthetic_design(n_q, D, m=m, seed=40 + D)
        th = [0.1, 0.35 * np.sqrt(D) if l is None else l, 0.7]
        f, Sinv = sr.host_fit(X, th, kernel, m, 11)
        P = orc.posterior_covariance(Sinv, f, m, th[0])
        _MODELS[name] = dict(X=X, th=th, kernel=kernel, alpha=Sinv @ f, A=orc.variance_operator(Sinv, P, True), Sinv=Sinv, f=f,
                             P=P, m=m)
    return _MODELS[name]


def _values(mod, Xq):
    """(mu, var) of the rows of Xq: the oracle's mu_Sigma_pred diagonal where the oracle has the kernel, else the dense
    expression on the statement's own cross-covariance."""
    if mod["kernel"] in orc.KERNELS and np.ndim(mod["th"][1]) == 0:
        out = [orc.mu_sigma_pred(x[None, :], mod["X"], mod["th"], mod["Sinv"], mod["f"], mod["P"], mod["kernel"]) for x in Xq]
        return np.array([float(np.ravel(o[0])[0]) for o in out]), np.array([float(np.ravel(o[1])[0]) for o in out])
    k = sn.cross(Xq, mod["X"], mod["th"], mod["kernel"])
    return k @ mod["alpha"], float(mod["th"][2]) ** 2 - np.einsum("ij,ij->i", k, k @ mod["A"])


@pytest.mark.parametrize("name", list(CASES))
def test_statement_against_central_differences(name):
    mod = _model(name)
    X, th, kernel = mod["X"], mod["th"], mod["kernel"]
    D = X.shape[1]
    Xq = 0.05 + 0.9 * np.random.default_rng(3).random((9, D))
    mustar = aq.best_design_mean(X, th, kernel, mod["alpha"])
    worst = {}
    for kind in (aq.MEAN, aq.EI, aq.VARIANCE):
        ref = aq.acq_reference(Xq, X, th, kernel, mod["alpha"], mod["A"], kind, mustar)
        mu0, var0 = _values(mod, Xq)
        assert np.max(np.abs(ref["mu"] - mu0) / ref["abs_mu"]) <= 1e-9
        assert np.max(np.abs(ref["var"] - var0)) <= 1e-9 * float(th[2]) ** 2
        a, b = aq.score_weights(ref["mu"], ref["var"], kind, mustar)
        num = {k: np.zeros((len(Xq), D)) for k in ("grad_mu", "grad_var", "grad_score")}
        for d in range(D):
            e = np.zeros(D)
            e[d] = H
            (mp, vp), (mm, vm) = _values(mod, Xq + e), _values(mod, Xq - e)
            num["grad_mu"][:, d] = (mp - mm) / (2 * H)
            num["grad_var"][:, d] = (vp - vm) / (2 * H)
            num["grad_score"][:, d] = (aq.score_value(mp, vp, kind, mustar) - aq.score_value(mm, vm, kind, mustar)) / (2 * H)
        # the rounding noise of a difference quotient of the dense variance sf^2 - k' A k: the quadratic form is summed
        # from terms of size |k|' |A| |k| (A carries Sigma^-1's dynamic range) and subtracted from sf^2, each good to eps
        # (far from the data the gradient is 1e-10 of sf^2 / h and drowns in it)
        k = np.abs(sn.cross(Xq, X, th, kernel))
        noise = (8 * np.finfo(float).eps / H) * (float(th[2]) ** 2 + np.einsum("ij,ij->i", k, k @ np.abs(mod["A"])))[:, None]
        scale = dict(grad_mu=ref["abs_gmu"], grad_var=ref["abs_gvar"] + 1e6 * noise,
                     grad_score=np.abs(a)[:, None] * ref["abs_gmu"] + np.abs(b)[:, None] * (ref["abs_gvar"] + 1e6 * noise))
        for k in num:
            worst[k] = max(worst.get(k, 0.0), float(np.max(np.abs(ref[k] - num[k]) / scale[k])))
    print(f"acq statement {name}: central differences, worst relative error {worst}")
    assert max(worst.values()) <= 1e-6, worst


def test_expected_improvement_without_variance():
    """sd = 0: the score is max(mu - mu*, 0), its gradient grad mu where mu > mu*, else 0 (and a negative variance is 0)."""
    mu = np.array([0.3, -0.2, 0.0, 0.3])
    var = np.array([0.0, 0.0, 0.0, -1e-18])
    assert np.array_equal(aq.score_value(mu, var, aq.EI, 0.1), np.maximum(mu - 0.1, 0.0))
    a, b = aq.score_weights(mu, var, aq.EI, 0.1)
    assert np.array_equal(a, [1.0, 0.0, 0.0, 1.0]) and np.array_equal(b, np.zeros(4))
    d = (aq.score_value(mu + H, var, aq.EI, 0.1) - aq.score_value(mu - H, var, aq.EI, 0.1)) / (2 * H)
    assert np.max(np.abs(d - a)) <= 1e-10
    # continuity: the sd > 0 expression tends to it
    assert abs(aq.score_value(0.3, 1e-30, aq.EI, 0.1) - 0.2) <= 1e-15 and abs(aq.score_value(-0.2, 1e-30, aq.EI, 0.1)) <= 1e-15
    assert np.isnan(aq.score_value(np.nan, 1.0, aq.EI, 0.0)) and np.isnan(aq.score_value(np.nan, 1.0, aq.VARIANCE, 0.0))


def test_header_and_binding_have_the_two_entries():
    from ppbo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppbo_hip.h")).read(), flags=re.S)
    for name, nargs in (("ppbo_acq_grad", 13), ("ppbo_acq_ascent", 15)):
        mt = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert mt, f"include/ppbo_hip.h does not declare {name}"
        assert len(mt.group(1).split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
    assert _lib.ABI_VERSION == 9 and "#define PPBO_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert "acq.hip" in __import__("ppbo_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("case", list(aq.ASCENT_CASES))
def test_the_reference_alone_passes_the_cap_of_the_ascent_comparison(case):
    """What tests/test_gpu_acq.py asserts of the device's ascent is compared over the (start, n) pairs the statement's own
    branch margins keep; the cap on the pairs left out (tests/test_gpu_search_stages.py: 0.125) and `no flipped branch
    among the kept ones` hold for the statement on its host-fitted twin of the GPU test's model."""
    X, th, kernel, m = aq.ascent_design(case)
    f, Sinv = sr.host_fit(X, th, kernel, m, 11)
    P = orc.posterior_covariance(Sinv, f, m, th[0])
    alpha, A = Sinv @ f, orc.variance_operator(Sinv, P, True)
    kind, lo, hi, starts = aq.ascent_setup(case)
    mustar = aq.best_design_mean(X, th, kernel, alpha)
    s = bsn.sensitivity_box(aq.acq_fg(X, th, kernel, alpha, A, kind, mustar), starts, lo, hi, sr.ASCENT_ITERS, sr.TOLS[0])
    print(f"acq ascent reference {case}: flips {s.flips}, left out {s.left_out:.3f}, dev {np.array2string(s.dev, precision=1)}, "
          f"it at n = {sr.ASCENT_ITERS}: {np.bincount(s.its[:, -1], minlength=sr.ASCENT_ITERS + 1)}")
    assert s.flips == 0 and s.left_out <= 0.125, (s.flips, s.left_out)
