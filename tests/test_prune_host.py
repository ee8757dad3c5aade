"""Host (no GPU): the bound and the selection rule of the pruned search as tests/prune_numpy.py states them.

On random edge-form models (the exact pieces of tests/probes/edge_form_identity.py) the bound must hold for every
candidate -- u^2 >= |H e|^2 -- and the exact winner must survive the selection, for pointwise EI and VARIANCE.  On the C3
fixture the bound must also be SHARP enough to be worth anything: 4096 candidates leave at most one column tile.
"""
import numpy as np
import pytest

import prune_numpy as pn
from conftest import load_golden


def _kernel(X, Y, l, sf2, kind):
    r2 = ((X[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    if kind == "se":
        return sf2 * np.exp(-0.5 * r2 / l ** 2)
    a = np.sqrt(5.0 * r2) / l
    return sf2 * (1.0 + a + a * a / 3.0) * np.exp(-a)


def _model(rng, n_q, m, D, kind):
    """A star design, its exact edge operator and a posterior at a random latent vector."""
    N = n_q * (m + 1)
    X = rng.random((N, D))
    for q in range(n_q):            # the rows of a star on one line through its observation
        o = q * (m + 1)
        X[o + 1:o + m + 1] = X[o] + rng.uniform(-0.3, 0.3, (m, 1)) * rng.standard_normal(D)
    l, sf2 = 0.3 * np.sqrt(D / 2.0), 1.3 ** 2
    Sigma = _kernel(X, X, l, sf2, kind) + 1e-6 * sf2 * np.eye(N)
    Sinv = np.linalg.inv(Sigma)
    Sinv = 0.5 * (Sinv + Sinv.T)
    f = 0.5 * np.linalg.cholesky(Sigma) @ rng.standard_normal(N)
    ld, lo = pn.star_lambda(f, m, 0.5)
    return dict(X=X, l=l, sf2=sf2, kind=kind, alpha=Sinv @ f, ld=ld, lo=lo, H=pn.edge_operator(Sinv, lo, m), m=m)


CASES = [(3, 3, 2, "se"), (5, 7, 2, "se"), (12, 31, 2, "se"), (4, 31, 20, "se"), (12, 5, 20, "se"), (7, 12, 20, "se"),
         (6, 9, 2, "matern52"), (9, 25, 20, "matern52")]


@pytest.mark.parametrize("n_q,m,D,kind", CASES)
def test_bound_holds_and_the_winner_survives(n_q, m, D, kind):
    rng = np.random.default_rng(100 * n_q + m + D)
    md = _model(rng, n_q, m, D, kind)
    Xc = np.concatenate([rng.random((400, D)), md["X"][::3]])          # (some candidates on design rows: q ~ -t)
    K = _kernel(md["X"], Xc, md["l"], md["sf2"], kind)
    mu = K.T @ md["alpha"]
    for score, mustar in ((pn.VARIANCE, 0.0), (pn.EI, float(mu.max())), (pn.EI, float(np.median(mu)))):
        r = pn.prune(K, md["alpha"], md["ld"], md["lo"], md["H"], m, md["sf2"], score, mustar)
        # the bound, with only the rounding of the two NumPy sums between the sides
        assert np.all(r["u"] ** 2 >= r["q"] * (1.0 - 1e-12)), (r["q"] / r["u"] ** 2).max()
        assert np.all(r["s_lo"] <= r["score"] + 1e-12 * np.abs(r["score"]).max())
        assert np.all(r["s_hi"] >= r["score"] - 1e-12 * np.abs(r["score"]).max())
        win = int(np.argmax(r["score"]))
        assert win in r["survivors"]
        assert np.all(np.diff(r["survivors"]) > 0)
        print(f"n_q={n_q} m={m} D={D} {kind} {score}: u^2/q median {np.median(r['u'] ** 2 / np.maximum(r['q'], 1e-300)):.3g}, "
              f"{r['survivors'].size} of {Xc.shape[0]} survive")


def test_nonfinite_candidates_survive_and_set_no_threshold():
    mu = np.array([0.1, np.nan, 0.3, 0.2])
    t = np.array([-0.5, -0.5, np.inf, -0.9])
    u = np.array([0.1, 0.1, 0.1, 0.1])
    var_lo, var_hi, s_lo, s_hi = pn.interval(mu, t, u, 1.0, pn.VARIANCE)
    b, tol, surv = pn.select(mu, var_hi, s_lo, s_hi, pn.VARIANCE)
    assert b == 0.5 and tol == 0.0
    assert list(surv) == [0, 1, 2]          # candidate 3 (var_hi = 0.11) is ruled out, the non-finite ones stay
    b, tol, surv = pn.select(np.full(3, np.nan), var_hi[:3], s_lo[:3], s_hi[:3], pn.VARIANCE)
    assert b == -np.inf and list(surv) == [0, 1, 2]


def test_c3_fixture_leaves_one_tile():
    """The flagship model with the benchmark's candidate stream (its first 4096 rows), the edge operator H itself (no
    projection), pointwise EI over the fixture's best mean: the survivors fit one 128-column tile."""
    from oracle import ppbo_oracle as orc
    g = load_golden("c3")
    th, m, kern = g["theta"], int(g["m"]), str(g["kernel"])
    X, f = g["X"], g["fMAP"]
    Sinv = orc.pd_inverse(orc.gram(X, th, kern))
    Sinv = 0.5 * (Sinv + Sinv.T)
    ld, lo = orc.lambda_compact(f, m, float(th[0]))
    H = pn.edge_operator(Sinv, lo, m)
    Xc = np.random.default_rng(1).random((4096, X.shape[1]))
    K = orc.cross_cov(X, Xc, th, kern)
    r = pn.prune(K, Sinv @ f, ld, lo, H, m, float(th[2]) ** 2, pn.EI, float(np.max(g["mu"])))
    ratio = r["u"] ** 2 / np.maximum(r["q"], 1e-300)
    print(f"c3: u^2/q median {np.median(ratio):.3g} min {ratio.min():.3g}; {r['survivors'].size} of 4096 survive "
          f"(threshold {r['threshold']:.3e}, tol {r['tol']:.1e})")
    assert np.all(r["u"] ** 2 >= r["q"] * (1.0 - 1e-12))
    assert int(np.argmax(r["score"])) in r["survivors"]
    assert r["survivors"].size <= 128
