"""NumPy statement of the projected edge form (ppbo_var_projection_build, include/ppbo_hip.h).

For every candidate x the extended Gram matrix [K k*; k*' k(x,x)] is positive semidefinite, so
    k* k*' <= k(x,x) K <= kappa Sigma,   kappa = sf2 / (1 - s)      (Sigma = (1 - s) K + s mu I, k(x,x) = sf2).
With e = B k* (the edge-layout K*), Sigma = L L', W = H B L and ANY Q with orthonormal columns
    0 <= |H e|^2 - |Q' H e|^2 = |(I - Q Q') H B k*|^2 <= kappa |(I - Q Q') W|_F^2,
and with a Q that is orthonormal only up to delta = |Q'Q - I|_F the certified form
    bound = kappa (|W - Q Z|_F^2 + 2 delta |W|_F^2),   Z = Q' W.
Q comes from a randomised range finder Y = W (W' Omega), orthonormalised in panels of 128 columns the way the device does
it (range_basis): finished panels projected out, shifted and plain Cholesky-QR passes.  The prefixes are nested.
"""
import importlib.util
import os

import numpy as np

_PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes", "edge_form_identity.py")
_spec = importlib.util.spec_from_file_location("edge_form_identity", _PROBE)
efi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(efi)

SHRINK = 1e-6
PANEL = 128


def r_max(N, m):
    """The largest multiple of 128 with 2 r <= 0.8 E."""
    E = N - N // (m + 1)
    return (E * 4 // 10) // PANEL * PANEL


def operators(Sigma, Sinv, lo, m):
    """H (edge operator, library layout) and W = H B L for Sigma = L L'."""
    H = efi.edge_operator(Sinv, lo, m)
    L = np.linalg.cholesky(Sigma)
    return H, H @ efi.edge_kstar(L, lo, m)


SHIFT = 1e-11      # relative to the trace of a panel's Gram matrix: above its rounding (N eps ~ 5e-13), so the factor exists


def _cholesky_qr(P, shift=0.0):
    G = P.T @ P
    G[np.diag_indices_from(G)] += shift * np.trace(G)
    R = np.linalg.cholesky(G)
    return np.linalg.solve(R, P.T).T          # P R^-T


def range_basis(W, r, seed=0):
    """Q [N, <= r] with nested 128-column prefixes.  Per panel, each step behind a projection off the finished panels:
    three SHIFTED Cholesky-QR passes (Y = W W' Omega squares a spectrum that falls off a cliff, so a panel's Gram matrix is
    numerically singular; each shifted pass lifts the smallest singular value by ~1 / sqrt(SHIFT) without failing), then
    two plain ones.  Directions that are rounding noise come out as orthonormal junk: harmless, the bound is certified
    for whatever Q is.  A failed pivot of a plain pass ends the basis at the previous panel."""
    N = W.shape[0]
    Om = np.random.default_rng(seed).standard_normal((N, r))
    Q = W @ (W.T @ Om)
    for c0 in range(0, r, PANEL):
        P, Qp = Q[:, c0:c0 + PANEL], Q[:, :c0]
        try:
            P = P - Qp @ (Qp.T @ P)
            for shift in (SHIFT, SHIFT, SHIFT, 0.0, 0.0):
                P = P - Qp @ (Qp.T @ P)
                P = _cholesky_qr(P, shift)
            Q[:, c0:c0 + PANEL] = P
        except np.linalg.LinAlgError:
            return Q[:, :c0]
    return Q


def estimates(W, Q):
    """kappa-free estimate |W|_F^2 - sum_{i <= r} |z_i|^2 for every 128-prefix r."""
    z2 = ((Q.T @ W) ** 2).sum(1)
    w2 = (W ** 2).sum()
    return {r: w2 - z2[:r].sum() for r in range(PANEL, Q.shape[1] + 1, PANEL)}


def certified_bound(W, Qr, sf2):
    """kappa (|W - Q Z|_F^2 + 2 delta |W|_F^2), in units of variance."""
    kappa = sf2 / (1.0 - SHRINK)
    R = W - Qr @ (Qr.T @ W)
    delta = np.linalg.norm(Qr.T @ Qr - np.eye(Qr.shape[1]))
    return kappa * ((R ** 2).sum() + 2.0 * delta * (W ** 2).sum())


def variance_terms(H, Qr, K, lo, m):
    """(|H e|^2, |Q' H e|^2) per candidate column of the raw cross-covariance K [N, M]."""
    Y = H @ efi.edge_kstar(K, lo, m)
    return (Y ** 2).sum(0), ((Qr.T @ Y) ** 2).sum(0)
