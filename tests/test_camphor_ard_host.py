"""CPU: camphor-copper with one length scale per coordinate (camphor_copper_ard_kernel) -- validation of theta, the
embedding identity camphor(x, x'; l) = SE(e(x), e(x'); 1) in NumPy, the grouped evidence gradient against central
differences of a NumPy Laplace evidence on embedded rows (tests/evgrad_numpy.py), the summed prior, and the new C-ABI
entries in the header, the binding, the version script and the built library."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import evgrad_numpy as eg
from conftest import ROOT
from oracle import ppbo_oracle as orc

# the camphor entries, and those that read ppbo_model.coords (PPBO_COORDS_CAMPHOR)
ENTRIES = ("ppbo_camphor_embed", "ppbo_camphor_line_points", "ppbo_mean_grad",
           "ppbo_mean_search_multi", "ppbo_mean_ascent")
PERIODIC = (0, 1, 3, 4, 5)


def camphor_ard_numpy(X1, X2, l, sf):
    """The per-coordinate camphor kernel from its definition: sin^2 for the periodic coordinates, a square for z."""
    s = np.zeros((X1.shape[0], X2.shape[0]))
    for d in range(6):
        dx = X1[:, d][:, None] - X2[:, d][None, :]
        s += (2.0 / l[d] ** 2) * np.sin(np.pi * np.abs(dx)) ** 2 if d != 2 else 0.5 * dx * dx / l[2] ** 2
    return sf * sf * np.exp(-s)


def camphor_reference_formula(X1, X2, l, sf):
    """The reference's scalar form (one l for the five periodic coordinates, l + 0.05 for z)."""
    per = np.zeros((X1.shape[0], X2.shape[0]))
    for d in PERIODIC:
        per += np.sin(np.pi * np.abs(X1[:, d][:, None] - X2[:, d][None, :])) ** 2
    dz = X1[:, 2][:, None] - X2[:, 2][None, :]
    return sf * sf * np.exp(-2.0 * per / l ** 2 - 0.5 * dz * dz / (l + 0.05) ** 2)


def embed_numpy(X, l):
    """e(X) in the column order of include/ppbo_hip.h: (c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5)."""
    cols = []
    for d in range(6):
        if d == 2:
            cols.append(X[:, 2] / l[2])
        else:
            cols += [np.cos(2 * np.pi * X[:, d]) / l[d], np.sin(2 * np.pi * X[:, d]) / l[d]]
    return np.stack(cols, axis=1)


def se_numpy(E1, E2, sf):
    return sf * sf * np.exp(-0.5 * orc.sqdist_direct(E1, E2))


def group(g11):
    """The 11 embedded columns' sums -> the six coordinates', by the grouping GPModel.evidence_grad applies."""
    from ppbo_amd.gp_model import camphor_coordinate_sums
    return camphor_coordinate_sums(g11)


def test_grouping_of_the_embedded_columns():
    from ppbo_amd.gp_model import camphor_coordinate_sums
    e = np.eye(11)
    cols = [int(np.argmax(camphor_coordinate_sums(e[k]))) for k in range(11)]
    assert cols == [0, 0, 1, 1, 2, 3, 3, 4, 4, 5, 5]
    with pytest.raises(ValueError):
        camphor_coordinate_sums(np.ones(12))


def test_validation():
    from ppbo_amd.engine import CAMPHOR_ARD, camphor_lengthscales, lengthscales
    v = [0.1, 0.2, 0.5, 1.0, 1.5, 2.0]
    assert np.array_equal(lengthscales([1.0, v, 1.0], 6, CAMPHOR_ARD), v)
    assert np.allclose(lengthscales([1.0, 0.26, 1.0], 6, CAMPHOR_ARD), [0.26, 0.26, 0.31, 0.26, 0.26, 0.26], rtol=0, atol=1e-15)
    assert np.allclose(camphor_lengthscales([1.0, np.float64(0.4), 1.0], 6), [0.4, 0.4, 0.45, 0.4, 0.4, 0.4])
    bad = [[0.1] * 5, [0.1] * 7, np.ones((2, 3)), [0.1, 0.1, 0.0, 0.1, 0.1, 0.1], [0.1, -0.1, 0.1, 0.1, 0.1, 0.1],
           [0.1, 0.1, np.nan, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, np.inf, 0.1, 0.1], 0.0, -0.2, np.nan, np.inf]
    for l in bad:
        with pytest.raises(ValueError):
            lengthscales([1.0, l, 1.0], 6, CAMPHOR_ARD)
    for D in (5, 7, 11):
        with pytest.raises(ValueError, match="D == 6"):
            lengthscales([1.0, 0.3, 1.0], D, CAMPHOR_ARD)
    # the scalar kernel keeps refusing a vector
    with pytest.raises(ValueError):
        lengthscales([1.0, v, 1.0], 6, "camphor_copper_kernel")


def test_kernels_module_and_settings_take_the_name():
    from ppbo_amd import kernels
    from ppbo_amd.ppbo_settings import PPBO_settings
    assert kernels.BY_NAME["camphor_copper_ard_kernel"] is kernels.camphor_copper_ard_kernel
    st = PPBO_settings(D=6, bounds=((0, 1),) * 6, xi_acquisition_function="EI", kernel="camphor_copper_ard_kernel",
                       theta_initial=[1.0, [0.1, 0.1, 0.5, 1.0, 1.0, 1.0], 8.0], theta_optimizer="ard-gradient")
    assert st.kernel == "camphor_copper_ard_kernel" and st.theta_optimizer == "ard-gradient"


@pytest.mark.parametrize("l", [[0.26, 0.26, 0.31, 0.26, 0.26, 0.26], [0.1, 0.1, 0.5, 1.0, 1.0, 1.0],
                               [0.02, 0.7, 1.9, 0.05, 0.3, 1.1]])
def test_embedding_identity(l):
    rng = np.random.default_rng(7)
    X1, X2 = rng.random((40, 6)), rng.random((33, 6))
    X2[:5] = X1[:5]                                     # coincident points: kernel value sf^2
    l = np.asarray(l)
    K = camphor_ard_numpy(X1, X2, l, 1.7)
    Ke = se_numpy(embed_numpy(X1, l), embed_numpy(X2, l), 1.7)
    assert np.max(np.abs(K - Ke)) / np.max(np.abs(K)) <= 1e-13


def test_profile_is_the_reference_kernel():
    rng = np.random.default_rng(8)
    X1, X2 = rng.random((30, 6)), rng.random((25, 6))
    for lsc in (0.1, 0.26, 1.3):
        prof = lsc + np.array([0, 0, 0.05, 0, 0, 0])
        K = camphor_ard_numpy(X1, X2, prof, 0.1)
        ref = camphor_reference_formula(X1, X2, lsc, 0.1)
        assert np.max(np.abs(K - ref)) / np.max(np.abs(ref)) <= 1e-13


def _camphor_case(l, sf, seed, n_q=8, m=3):
    X = orc.synthetic_design(n_q, 6, m=m, seed=seed)
    E = embed_numpy(X, l)
    th = [1.0, 1.0, sf]
    rs = np.random.RandomState(seed)
    f0 = np.linalg.cholesky(eg.sigma_matrix(E, th, "SE_kernel")) @ rs.standard_normal(X.shape[0])
    _, f = eg.evidence(E, th, "SE_kernel", m, f0)
    return X, m, f


def _camphor_evidence(X, l, sf, m, f0):
    E = embed_numpy(X, l)
    th = [1.0, 1.0, sf]
    v, f = eg.evidence(E, th, "SE_kernel", m, f0)
    return v - eg.log_prior(th) + eg.log_prior([1.0, l, sf]), f


def _grouped_grad(X, l, sf, m, f, sign=None):
    """dE/d(l_0..l_5, sigma_f): the embedded rows' per-column gradient (unit length scales, no prior) grouped by
    coordinate and divided by l_d, plus the six-coordinate prior's gradient."""
    E = embed_numpy(X, l)
    g11, sU = eg.evidence_grad(E, [1.0, np.ones(11), sf], "SE_kernel", m, f, with_prior=False, sign=sign)
    g = np.append(group(g11[:-1]) / l, g11[-1]) + eg.log_prior_grad([1.0, l, sf])
    return g, sU


def _central(X, l, sf, m, f, rel_h=1e-5):
    """Central differences of the evidence (f_MAP warm-started at f) and the LU signs met inside the stencil."""
    p = np.append(l, sf)
    fd, signs = np.empty_like(p), []
    for k in range(p.size):
        h = rel_h * p[k]
        vals = []
        for sgn in (1.0, -1.0):
            q = p.copy()
            q[k] += sgn * h
            v, fq = _camphor_evidence(X, q[:6], q[6], m, f)
            Sig = eg.sigma_matrix(embed_numpy(X, q[:6]), [1.0, 1.0, q[6]], "SE_kernel")
            signs.append(eg.slogdet_lu(np.eye(len(f)) + Sig @ orc.lambda_dense(fq, m, 1.0))[0])
            vals.append(v)
        fd[k] = (vals[0] - vals[1]) / (2.0 * h)
    return fd, signs


@pytest.mark.parametrize("l,sf,seed", [([0.3, 0.6, 0.9, 1.2, 0.5, 1.0], 2.0, 4)])
def test_grouped_gradient_matches_central_differences(l, sf, seed):
    l = np.asarray(l, dtype=float)
    X, m, f = _camphor_case(l, sf, seed)
    g, sU = _grouped_grad(X, l, sf, m, f)
    fd, signs = _central(X, l, sf, m, f)
    assert all(s == sU for s in signs)            # no pivot-sequence change inside the stencil
    assert g.shape == (7,)
    assert np.max(np.abs(g - fd) / np.abs(fd)) <= 1e-5


def test_grouped_gradient_where_the_lu_sign_is_not_the_determinants():
    # a design where prod sign(u_kk) != sign det A (an odd pivot permutation), away from a sign change of the LU
    l, sf = np.array([0.3, 0.6, 0.9, 1.2, 0.5, 1.0]), 3.0
    X, m, f = _camphor_case(l, sf, seed=4)
    Sig = eg.sigma_matrix(embed_numpy(X, l), [1.0, 1.0, sf], "SE_kernel")
    sU, _, sdet = eg.slogdet_lu(np.eye(len(f)) + Sig @ orc.lambda_dense(f, m, 1.0))
    assert sU != sdet
    fd, signs = _central(X, l, sf, m, f)
    assert all(s == sU for s in signs)
    g, sU2 = _grouped_grad(X, l, sf, m, f)
    assert sU2 == sU
    assert np.max(np.abs(g - fd) / np.abs(fd)) <= 1e-5
    g_det, _ = _grouped_grad(X, l, sf, m, f, sign=sdet)
    assert np.max(np.abs(g_det - fd) / np.abs(fd)) > 1e-3


def test_prior_is_the_sum_over_six_coordinates():
    import scipy.stats
    from ppbo_amd.gp_model import log_prior
    l = np.array([0.1, 0.2, 0.5, 1.0, 1.5, 2.0])
    one = lambda x: np.log(scipy.stats.lognorm.pdf(x, s=0.5, scale=np.exp(-1.4)))  # noqa: E731
    base = log_prior([1.0, 0.3, 8.0]) - one(0.3)
    assert abs(log_prior([1.0, l, 8.0]) - (base + sum(one(v) for v in l))) <= 1e-12
    # a scalar stands for its profile: six terms, z at l + 0.05
    prof = 0.26 + np.array([0, 0, 0.05, 0, 0, 0])
    assert abs(log_prior([1.0, prof, 8.0]) - (base + 5 * one(0.26) + one(0.31))) <= 1e-12


def test_entries_in_header_binding_map_and_library():
    from ppbo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    vs = open(os.path.join(ROOT, "ppbo_amd", "csrc", "libppbo_hip.map")).read()
    pats = [p.strip() for p in vs.split("global:")[1].split("local:")[0].split(";") if p.strip()]
    for e in ENTRIES:
        assert re.search(r"PPBO_API int %s\(" % e, hdr), e
        assert e in _lib.SIGNATURES, e
        assert any(fnmatch.fnmatch(e, p) for p in pats), e
    assert _lib.ABI_VERSION == 9
    assert "camphor_copper_ard_kernel" not in _lib.KERNEL_IDS        # no device kernel id: SE on embedded rows
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libppbo_hip.so is not built (build() runs before the suite)")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for e in ENTRIES:
        assert e in syms, e
