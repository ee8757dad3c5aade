"""GPU: the Laplace-evidence gradient (ppbo_evidence_grad, GPModel.evidence_grad) and the ARD length-scale fit
(GPModel.optimize_theta_ard).  The device gradient is checked against the NumPy restatement of tests/evgrad_numpy.py
evaluated at the device's own f_MAP, and against central differences of its own value; the fit against the
derivative-free search on data whose utility depends on two of six coordinates."""
import numpy as np
import pytest

import evgrad_numpy as eg
from conftest import load_golden

pytestmark = pytest.mark.gpu

RADIAL = ["SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def _gp(X, m, kernel, theta):
    """A GPModel on the rows X as they stand (the reference's layout: query row, then its m pseudo-observations)."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    D = X.shape[1]
    st = PPBO_settings(D=D, bounds=((0, 1),) * D, xi_acquisition_function="EI-EXT-FAST", kernel=kernel, m=m,
                       theta_initial=theta, verbose=False)
    gp = GPModel(st)
    gp.X, gp.N = np.asarray(X, dtype=float), X.shape[0]
    gp._dX = gp.eng.dev(gp.X)
    gp.theta = theta
    gp.update_Sigma(theta)
    return gp


def _design(D, n_q, m, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n_q * (m + 1), D))


def _start(gp, theta, seed):
    rs = np.random.RandomState(seed)
    return np.linalg.cholesky(eg.sigma_matrix(gp.X, theta, gp.kernel.__name__)) @ rs.standard_normal(gp.N)


def _rel_components(g, ref):
    return np.max(np.abs(g - ref) / np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(ref))))


CASES = [(k, ard) for k in RADIAL for ard in (False, True)]


def _theta(ard, D, sigma=1.0, sf=1.5):
    return [sigma, np.geomspace(0.2, 1.2, D) if ard else 0.4, sf]


@pytest.mark.parametrize("kernel, ard", CASES)
def test_value_and_sign_equal_the_evidence(eng, kernel, ard):
    X = _design(4, 16, 3, seed=5)
    th = _theta(ard, 4)
    gp = _gp(X, 3, kernel, th)
    f0 = _start(gp, th, 7)
    v, g, le, sU, fm = gp.evidence_grad(th, f_initial=f0)
    v_ref, le_ref = gp._evidence_core(gp.eng, th, gp.eng.dev(f0))
    assert abs(v - v_ref) <= 1e-12 * abs(v_ref)
    assert abs(le - le_ref) <= 1e-12 * abs(le_ref)
    Sig, _, fm2, _, ld, lo = gp._evidence_fit(gp.eng, th, gp.eng.dev(f0))
    s2, logdet2, _ = eng.laplace_logdet(Sig, ld, lo, 3)
    assert sU == s2
    assert g.shape == ((5,) if ard else (2,))


def _grad_case(gp, th, f0):
    v, g, _, sU, fm = gp.evidence_grad(th, f_initial=f0, gtol=1e-10)
    ref, sU_ref = eg.evidence_grad(gp.X, th, gp.kernel.__name__, gp.m, host(fm).astype(float))
    assert sU == sU_ref
    assert _rel_components(g, ref) <= 1e-7, (g, ref)


@pytest.mark.parametrize("kernel, ard", CASES)
def test_gradient_matches_the_restatement(eng, kernel, ard):
    X = _design(4, 16, 3, seed=11)
    th = _theta(ard, 4)
    gp = _gp(X, 3, kernel, th)
    _grad_case(gp, th, _start(gp, th, 3))


@pytest.mark.parametrize("kernel", RADIAL)
def test_gradient_ragged_rows(eng, kernel):
    m = 25                                   # N = 208: no multiple of any tile edge
    X = _design(5, 8, m, seed=21)
    th = _theta(True, 5, sigma=0.7, sf=2.0)
    gp = _gp(X, m, kernel, th)
    _grad_case(gp, th, _start(gp, th, 4))


@pytest.mark.parametrize("name", ["ard/se_d4", "ard/m52_d6", "c2"])
def test_gradient_on_fixtures(eng, name):
    g = load_golden(name)
    if "theta_l" in g:
        th = [float(g["theta_sf"][0]), np.asarray(g["theta_l"], dtype=float), float(g["theta_sf"][1])]
    else:
        th = [float(g["theta"][0]), float(g["theta"][1]), float(g["theta"][2])]
    th[0] = max(th[0], 0.3)         # sigma << sigma_f gives T several local maxima; any sigma is a valid point
    gp = _gp(g["X"], int(g["m"]), str(g["kernel"]), th)
    _grad_case(gp, th, g["f_init"])


@pytest.mark.parametrize("kernel, ard", [("SE_kernel", True), ("Matern32_kernel", False), ("RQ_kernel", True),
                                         ("Matern52_kernel", True)])
def test_gradient_matches_central_differences_of_its_value(eng, kernel, ard):
    X = _design(3, 12, 3, seed=31)
    th = _theta(ard, 3)
    gp = _gp(X, 3, kernel, th)
    _, g, _, sU, fm = gp.evidence_grad(th, f_initial=_start(gp, th, 5), gtol=1e-10)
    f_warm = host(fm)
    p = eg.params(th)
    for k in range(p.size):
        h = 1e-5 * p[k]
        vals = []
        for sgn in (1.0, -1.0):
            q = p.copy()
            q[k] += sgn * h
            v, _, _, s, _ = gp.evidence_grad(eg.with_params(th, q), f_initial=f_warm, gtol=1e-10)
            assert s == sU
            vals.append(v)
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(g[k] - fd) <= 1e-4 * max(abs(fd), 1e-2 * np.max(np.abs(g))), (k, g[k], fd)


def test_repeated_calls_are_bit_identical(eng):
    X = _design(6, 40, 5, seed=41)
    th = _theta(True, 6)
    gp = _gp(X, 5, "Matern52_kernel", th)
    f0 = _start(gp, th, 6)
    a = gp.evidence_grad(th, f_initial=f0)
    b = gp.evidence_grad(th, f_initial=f0)
    assert a[0] == b[0] and a[3] == b[3]
    assert np.array_equal(a[1], b[1])


def test_camphor_is_refused(eng):
    X = _design(6, 4, 3, seed=1)
    th = [1.0, 0.4, 1.5]
    gp = _gp(X, 3, "camphor_copper_kernel", th)
    with pytest.raises(ValueError):
        gp.evidence_grad(th, f_initial=np.zeros(gp.N))
    Sig = eng.gram(X, th, "camphor_copper_kernel")
    z = eng.dev(np.zeros(gp.N))
    with pytest.raises(ValueError):
        eng.evidence_grad(X, th, "camphor_copper_kernel", Sig, Sig, z, z, z, 3)


# ---------------------------------------------------------------- the relevance fit
def _relevance_model(seed, D=6, n_q=40, m=5):
    """Preference data from u(z) = -(z0 - 0.3 - 0.5 z1)^2 - 0.5 (z1 - 0.6)^2: queries along e_0 and e_1, every other
    coordinate uniform; the answer is the line's maximiser, so it depends on z0 and z1 only."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, 1.0, 2001)
    rows = []
    for q in range(n_q):
        d = q % 2
        xi = np.zeros(D)
        xi[d] = 1.0
        x = rng.random(D)
        x[d] = 0.0
        Z = x[None, :] + grid[:, None] * xi[None, :]
        u = -(Z[:, 0] - 0.3 - 0.5 * Z[:, 1]) ** 2 - 0.5 * (Z[:, 1] - 0.6) ** 2
        a = grid[int(np.argmax(u))]
        rows.append(np.concatenate([a * xi + x, xi, [a]]))
    st = PPBO_settings(D=D, bounds=((0, 1),) * D, xi_acquisition_function="EI-EXT-FAST", m=m,
                       theta_initial=[1.0, 0.5, 1.0], verbose=False, skip_computations_during_initialization=False)
    gp = GPModel(st)
    np.random.seed(seed)
    gp.update_feedback_processing_object(np.array(rows))
    gp.update_data()
    gp.turn_initialization_off()
    gp.update_model()
    return gp


def test_ard_fit_finds_the_relevant_coordinates(eng):
    from ppbo_amd.gp_model import THETA_BOX
    gp = _relevance_model(61)
    np.random.seed(62)
    gp.optimize_theta(workers=2)
    best_search = max(v for _, _, v in gp.theta_search_log)
    np.random.seed(62)
    gp.optimize_theta_ard(maxfun=60, start=[1.0, np.full(6, 0.5), 1.0])
    log = gp.theta_search_log
    assert 1 <= len(log) <= 60
    v_start, v_best = log[0][2], max(v for _, _, v in log)
    assert v_best >= v_start
    assert v_best >= best_search
    l = np.asarray(gp.theta[1])
    assert l.shape == (6,)
    assert np.min(l[2:]) > np.max(l[:2]), l
    (llo, lhi), (slo, shi) = THETA_BOX
    assert np.all(l >= llo * (1 - 1e-12)) and np.all(l <= lhi * (1 + 1e-12))
    assert slo * (1 - 1e-12) <= gp.theta[2] <= shi * (1 + 1e-12)
    assert gp.theta[0] == 1.0
    # theta is the best entry of the log
    k = int(np.argmax([v for _, _, v in log]))
    assert np.allclose(log[k][0], l, rtol=1e-15) and log[k][1] == gp.theta[2]


def test_run_ppbo_loop_with_the_gradient_fit(eng):
    from ppbo_amd.numerical_main import line_search_user, run_ppbo_loop
    from ppbo_amd.ppbo_settings import PPBO_settings
    D = 4
    lo, hi = np.zeros(D), np.ones(D)
    w = np.array([4.0, 1.0, 0.1, 0.01])

    def objective(P):
        return ((np.atleast_2d(P) - 0.3) ** 2 * w).sum(axis=1)

    st = PPBO_settings(D=D, bounds=list(zip(lo, hi)), xi_acquisition_function="EI-EXT-FAST",
                       theta_initial=[1.0, 0.3, 1.0], m=5, verbose=False, EI_EXR_mc_samples=50, EI_EXR_BO_maxiter=5,
                       theta_optimizer="ard-gradient")
    np.random.seed(71)
    xi0 = np.eye(D)[:3]
    x0 = np.random.uniform(0, 1, (3, D))
    res, xs, mus, gp = run_ppbo_loop(line_search_user(objective, lo, hi), xi0, x0, 2, st,
                                     optimize_hyperparameters_after_initialization=True)
    assert res.shape == (5, 2 * D + 1)
    assert np.ndim(gp.theta[1]) == 1 and np.asarray(gp.theta[1]).shape == (D,)
    assert 1 <= len(gp.theta_search_log) <= 60
    assert np.all(np.isfinite(xs[3:]))
