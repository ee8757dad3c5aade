"""CPU-only: the projected edge form in NumPy (tests/var_projection_numpy.py) on the c2 and c3 fixtures, with the oracle's
Sigma and the reference's f_MAP.  The bound is the construction's own; -1e-14 sf2 is the rounding allowed to a difference
of two sums of squares that must not be negative."""
import numpy as np
import pytest

import var_projection_numpy as vp
from oracle import ppbo_oracle as orc


@pytest.fixture(scope="module")
def models(golden):
    """name -> (H, W, Q at r_max, lam_off, m, sf2, K* of 2048 seeded candidates), formed once."""
    out = {}
    for name in ("c2", "c3"):
        g = golden(name)
        X, th, kern, m = g["X"], g["theta"], str(g["kernel"]), int(g["m"])
        Sigma = orc.gram(X, th, kern)
        Sinv = orc.pd_inverse(Sigma)
        Sinv = 0.5 * (Sinv + Sinv.T)
        _, lo = vp.efi.star_lambda(g["fMAP"], m, float(th[0]))
        H, W = vp.operators(Sigma, Sinv, lo, m)
        Q = vp.range_basis(W, vp.r_max(X.shape[0], m))
        K = orc.cross_cov(X, np.random.default_rng(2048).random((2048, X.shape[1])), th, kern)
        out[name] = (H, W, Q, lo, m, float(th[2]) ** 2, K)
    return out


def test_r_max():
    assert vp.r_max(2048, 31) == 768 and vp.r_max(384, 31) == 128 and vp.r_max(416, 25) == 128 and vp.r_max(256, 31) == 0


def test_c3_reaches_the_tolerance_at_512(models):
    H, W, Q, lo, m, sf2, K = models["c3"]
    assert Q.shape[1] == 768
    b = vp.certified_bound(W, Q[:, :512], sf2)
    est = vp.estimates(W, Q)
    print(f"c3: bound(512) = {b / sf2:.3e} sf2, estimates " + " ".join(f"{r}:{e * sf2 / (1 - vp.SHRINK) / sf2:.2e}" for r, e in est.items()))
    assert b <= 1e-10 * sf2
    # the smallest prefix whose estimate meets 1e-10 sf2 is 512: 384 does not
    kappa = sf2 / (1.0 - vp.SHRINK)
    assert kappa * est[384] > 1e-10 * sf2 >= kappa * est[512]


@pytest.mark.parametrize("name,r", [("c2", 128), ("c3", 128), ("c3", 384), ("c3", 512), ("c3", 768)])
def test_measured_error_within_the_bound(models, name, r):
    H, W, Q, lo, m, sf2, K = models[name]
    assert Q.shape[1] >= r
    Qr = Q[:, :r]
    b = vp.certified_bound(W, Qr, sf2)
    full, proj = vp.variance_terms(H, Qr, K, lo, m)
    d = full - proj
    print(f"{name} r={r}: bound {b / sf2:.3e} sf2, measured [{d.min() / sf2:.2e}, {d.max() / sf2:.2e}] sf2, "
          f"largest reduction {full.max() / sf2:.2e} sf2")
    assert d.max() <= b
    assert d.min() >= -1e-14 * sf2          # the projection never over-subtracts


def test_delta_term_covers_a_perturbed_basis(models):
    """Q perturbed off orthonormality (delta ~ 1e-6): |Q'He|^2 may now EXCEED |He|^2 -- by no more than the bound says."""
    H, W, Q, lo, m, sf2, K = models["c3"]
    rng = np.random.default_rng(6)
    Qp = Q[:, :512] + 1e-6 / np.sqrt(Q.shape[0] * 512) * rng.standard_normal((Q.shape[0], 512))
    delta = np.linalg.norm(Qp.T @ Qp - np.eye(512))
    assert 3e-7 <= delta <= 3e-6
    b0, b = vp.certified_bound(W, Q[:, :512], sf2), vp.certified_bound(W, Qp, sf2)
    full, proj = vp.variance_terms(H, Qp, K, lo, m)
    print(f"delta = {delta:.2e}: bound {b0 / sf2:.2e} -> {b / sf2:.2e} sf2, measured |d| {np.abs(full - proj).max() / sf2:.2e} sf2")
    assert b > 100 * b0                     # the delta term dominates
    assert np.abs(full - proj).max() <= b
