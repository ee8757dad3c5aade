"""GPU: every K* launcher of csrc/predict.hip in every padded-dimension bucket, every radial family, at both edges of the
bucket.  Each launcher carries its own `if (m->D <= ...)` ladder over separately compiled <family, DP> instances, and each
kernel masks the padded columns of a row itself; a wrong rung, a mask that drops the last real column or a miscompiled
instance shows only at the D that reaches it.

The matrix (tests/kstar_bucket_cases.py, tied to the ladders in the source by tests/test_kstar_bucket_cases_host.py): one
case per (bucket b of 4 6 8 10 12 16 20 24 32 48 64, family k of SE RQ Matern-5/2 Matern-3/2), 44 in all.  D is the
bucket's upper edge when b + k is even, else its lower edge (the bucket below + 1; 2 in the bucket 4); the variance
operator is in node form when b + k // 2 is even, else in edge form; the design is 8 stars of 4 rows (N = 32) when b is
even, else 3 stars of 26 (N = 78: off every tile edge, a star across two staging steps of 32 rows).

A case fits its model once (tests/test_gpu_slopes.py::_fitted; (alpha, A) the host's own, from the device's f_MAP only) and
runs every entry that goes through a K* launcher.  Each call is held by the helper, the error measure and the bound of the
module that owns the entry:
  * predict_pairs        test_gpu_pairs._parity                               TOL = 1e-6
  * predict_slopes       test_gpu_slopes._parity, M = 257                     TOL = 1e-6
  * predict_gradients    test_gpu_gradients._parity, M = 37; C symmetric bit for bit, smallest eigenvalue >= -TOL
  * predict_curvatures   test_gpu_curvature._parity (Matern-3/2 is refused by the library: no call); for D <= 16 a second
                         call with random accelerations (the ACC instances), test_gpu_curvature._errors, the same TOL
  * predict_functionals  test_gpu_functionals._parity, the combos of its test_parity_other_shapes
  * predict              on an engine with PPBO_FUSED=0 (the one-launch kernel would take node-form models of D <= 16):
                         130 uniform candidates and 4 design rows against oracle.predict_mean_var at the bounds of
                         test_gpu_parity.py::test_every_dimension_bucket: mean 1e-7 relative, variance 1e-7 sf2; with
                         kstar_fp32 1e-3 / 1e-2 sf2
  * the pruned search    test_gpu_prune.check, EI and VARIANCE, on the edge-form model of the same (kernel, D, n_q, m):
                         the flagged K* instance, its record bitwise that of an engine with PPBO_PRUNE=0 and NumPy's argmax

No case asks that the chunk is pruned (at these smooth models most of 300 candidates survive; 4 of the 44 EI searches
take the compact launch): the flagged pass writes the K*, the mean and the t sums of the record either way.

Measured on MI355X, the worst over the 44 cases (the whole module 12 s, no case above 0.6 s): pairs mean 2.5e-9, variance
3.7e-9, |p - ref| 1.7e-10; slopes 6.9e-10 / 4.6e-10 / 5.6e-11; gradients mean 3.5e-10, covariance 1.2e-9, smallest
eigenvalue of C >= 0.22 of the largest prior entry; curvatures 6.6e-10 / 2.4e-9 / 1.3e-10, with accelerations (18 cases)
6.8e-10 / 1.5e-9 / 8.4e-11; functionals 4.3e-9 / 9.6e-10 / 2.8e-10; predict mean 2.7e-9, variance 3.9e-9 sf2, with fp32 K*
3.1e-6 / 2.7e-7 sf2; every pruned-search record bitwise the unpruned one.  The host reference's own two forms of the
variance operator (Sigma^-1 - Sigma^-1 P Sigma^-1 against the Woodbury form) differ by up to 5e-9 sf2 on these designs.
With launch_kstar_slope's `m->D <= 10` rung sent to the 8-bucket instance (a scratch build), tests/test_gpu_slopes.py
passes and the four bucket-10 cases here fail in the slopes call at 0.32 - 1.5 (mean) and 6.9e-3 - 5.4e-2 (variance)."""
import numpy as np
import pytest

import curvature_numpy as cn
import gradients_numpy as gn
import kstar_bucket_cases as kc
import slopes_numpy as sn
import test_gpu_curvature as tc
import test_gpu_functionals as tf
import test_gpu_gradients as tg
import test_gpu_pairs as tp
import test_gpu_slopes as ts
from oracle import ppbo_oracle as orc
from test_gpu_kstar_star import _engine
from test_gpu_parity import rel
from test_gpu_prune import check
from test_gpu_slopes import host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def unfused():
    e = _engine(PPBO_FUSED=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def on():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def off():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=0)
    yield e
    e.close()


def _accelerated_curvature(eng, mod, label):
    """Random accelerations against the curved-path statement, as test_gpu_curvature.py::test_acceleration_on_an_se_model."""
    from ppbo_amd.engine import CURV_PROB
    M, D = 257, mod["X"].shape[1]
    rng = np.random.default_rng(21)
    X, Xi = ts._rows(rng, mod, M)
    Xa = rng.standard_normal((M, D)) * 10.0 ** rng.uniform(-2.0, 2.0, (M, 1))
    md = eng._model(mod["post"], True)
    mu, var, p = eng.empty(M), eng.empty(M), eng.empty(M)
    rc, msg = tc._c_call(eng, md, eng.dev(X), eng.dev(Xi), eng.dev(Xa), M, CURV_PROB, mu, var, p)
    assert rc == 0, msg
    mu, var, p = host(mu), host(var), host(p)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var)) and np.all(np.isfinite(p))
    e_mu, e_var, e_p = tc._errors(mod, X, Xi, mu, var, p, Xa)
    print(f"curvature parity {label} with accelerations M={M}: |mu_c - ref| / sum|c alpha| = {e_mu:.2e}, "
          f"|var_c - ref| / prior = {e_var:.2e}, |p - ref| = {e_p:.2e}")
    assert e_mu <= tc.TOL and e_var <= tc.TOL
    assert np.abs(p - cn.curvature_probability(mu, var)).max() <= 4 * tc.EPS


def _mean_var_reference(Xc, mod):
    """oracle.predict_mean_var on the case's (alpha, A).  The oracle has no Matern kernel: there the same two lines
    (mu = K*' alpha, var = sf2 - diag(K*' A K*)) on the K* of tests/slopes_numpy.py, the statement (alpha, A) came from."""
    if mod["kernel"] in orc.KERNELS:
        return orc.predict_mean_var(Xc, mod["X"], mod["th"], mod["alpha"], mod["A"], mod["kernel"])
    k = sn.cross(mod["X"], Xc, mod["th"], mod["kernel"])
    return k.T @ mod["alpha"], float(mod["th"][2]) ** 2 - np.einsum("ij,ij->j", k, mod["A"] @ k)


def _plain_pass(unfused, mod, label):
    """kstar_kernel<KID, DP> and its fp32 twin at the bounds of test_gpu_parity.py::test_every_dimension_bucket."""
    N, D = mod["X"].shape
    rng = np.random.default_rng(D)
    Xc = np.concatenate([rng.random((130, D)), mod["X"][rng.integers(0, N, 4)]])
    mu0, var0 = _mean_var_reference(Xc, mod)
    sf2 = float(mod["th"][2]) ** 2
    out = unfused.predict(mod["post"], Xc)
    mu, var = host(out["mu"]), host(out["var"])
    o32 = unfused.predict(mod["post"], Xc, want_best=False, kstar_fp32=True)
    mu32, var32 = host(o32["mu"]), host(o32["var"])
    print(f"predict parity {label}: |mu - ref| / max|ref| = {rel(mu, mu0):.2e}, |var - ref| / sf2 = {np.abs(var - var0).max() / sf2:.2e}; "
          f"fp32 K*: {np.abs(mu32 - mu0).max() / np.abs(mu0).max():.2e}, {np.abs(var32 - var0).max() / sf2:.2e}")
    assert rel(mu, mu0) < 1e-7
    assert np.abs(var - var0).max() <= 1e-7 * sf2
    assert np.abs(mu32 - mu0).max() <= 1e-3 * np.abs(mu0).max()
    assert np.abs(var32 - var0).max() <= 1e-2 * sf2
    return Xc


def _pruned_search(on, off, mod, Xc, label):
    """The flagged instance kstar_kernel<KID, DP, false, true>: candidates around the design and the uniform ones of the
    plain pass; the incumbent is the third best mean, as in test_gpu_prune.py::test_few_survivors."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    N, D = mod["X"].shape
    rng = np.random.default_rng(100 + D)
    Xc = np.concatenate([mod["X"][rng.integers(0, N, 166)] + 0.05 * rng.standard_normal((166, D)), Xc])
    mu = host(off.predict(mod["post"], Xc)["mu"])
    check(on, off, mod["post"], Xc, SCORE_POINTWISE_EI, float(np.sort(mu)[-3]), label=f"pruned search {label}")
    check(on, off, mod["post"], Xc, SCORE_VARIANCE, 0.0, label=f"pruned search {label}")


@pytest.mark.parametrize("c", kc.CASES, ids=kc.case_id)
def test_bucket(eng, unfused, on, off, c):
    # test_gpu_gradients._model(which) is the cached test_gpu_slopes._fitted(kernel, D, n_q, m, form) that its _parity takes
    which, which_edge = (f"{c.kernel[:-7]}-{c.D}-{c.n_q}-{c.m}-{form}" for form in (c.form, "edge"))
    mod = tg._model(which)
    label = f"{c.kernel} D={c.D} (bucket {kc.BUCKETS[c.b]}, {c.edge} edge) N={c.n_q * (c.m + 1)} {c.form}"
    assert mod["X"].shape == (c.n_q * (c.m + 1), c.D) and mod["kernel"] == c.kernel
    tp._parity(eng, mod, label=label)
    ts._parity(eng, mod, M=257, label=label)
    # gradients: parity, and the structure checks of test_gpu_gradients.py::test_parity
    X, out = tg._parity(eng, which, M=37)
    Cv = host(out["cov"])
    assert np.array_equal(Cv, Cv.transpose(0, 2, 1))
    low = np.linalg.eigvalsh(Cv).min() / gn.prior_diagonal(mod["th"], mod["kernel"], c.D).max()
    print(f"gradients structure {which}: smallest eigenvalue / largest prior entry = {low:.3e}")
    assert low >= -tg.TOL
    if c.kernel in tc.RADIAL:
        tc._parity(eng, mod, label=label)
        if c.D <= 16:
            _accelerated_curvature(eng, mod, label)
    tf._parity(eng, mod, combos=(tf.COMBOS[1], tf.COMBOS[3], tf.COMBOS[5]), label=label)
    Xc = _plain_pass(unfused, mod, label)
    _pruned_search(on, off, tg._model(which_edge), Xc, label)
