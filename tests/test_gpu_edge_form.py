"""GPU: the variance operator in edge form (ppbo_posterior / ppbo_gp_fit with PPBO_FORM_EDGE, and every consumer of a
model whose `form` says so) against the node form on the same posterior and against the golden vectors.
tests/probes/edge_form_identity.py states the identity."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_names

pytestmark = pytest.mark.gpu

ALL = golden_names()
FITTED = [n for n in ("smoke", "rq", "c2", "c3", "c5") if n in ALL]
EXTRA = ["ard/se_d4", "ard/m52_d6", "matern/m52_small", "matern/m32_small", "camphor_ard/spread"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def load(name):
    g = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
    if "theta_l" in g:
        g["theta"] = [float(g["theta_sf"][0]), g["theta_l"], float(g["theta_sf"][1])]
    if name.startswith("camphor_ard/"):
        g["kernel"] = "camphor_copper_ard_kernel"
    return g


def both_forms(eng, g):
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE
    th, kern, m = g["theta"], str(g["kernel"]), int(g["m"])
    Sinv = eng.pd_inverse(eng.gram(g["X"], th, kern))
    node = eng.posterior(g["X"], th, kern, Sinv, g["fMAP"], m, form=FORM_NODE)
    edge = eng.posterior(g["X"], th, kern, Sinv, g["fMAP"], m, form=FORM_EDGE)
    return node, edge, float(th[2]) ** 2


def check_layout(eng, post):
    """H: zero in the observation rows / columns and above the diagonal."""
    N, n_q = post.X.shape[0], post.X.shape[0] // (post.m + 1)
    H = host(post.G)
    assert not H[:n_q].any() and not H[:, :n_q].any()
    assert not np.triu(H, 1).any()
    assert np.all(np.diag(H)[n_q:] > 0)


@pytest.mark.parametrize("name", FITTED + EXTRA)
def test_edge_form_variance_matches_node_form(eng, name):
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    g = load(name)
    node, edge, sf2 = both_forms(eng, g)
    check_layout(eng, edge)
    Xc = g["Xc"]
    if Xc.shape[0] < 4096:       # the padded (>= 2048 candidates) quadform path as well as the direct one
        Xc = np.concatenate([Xc, np.random.default_rng(3).random((4096, Xc.shape[1]))])
    mustar = float(np.max(g["mu"]))
    a = eng.predict(node, Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
    b = eng.predict(edge, Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
    # (small node-form models are scored by the one-launch kernel: the mean agrees to rounding, not bit for bit)
    assert np.abs(host(a["mu"]) - host(b["mu"])).max() <= 1e-12 * np.abs(host(a["mu"])).max()
    # two factorizations of congruent matrices in different coordinates: at c3 (cond(B) ~ 2e7) they differ by 2.0e-8 sf2,
    # at most 5.6e-9 on the other fixtures
    assert np.abs(host(a["var"]) - host(b["var"])).max() <= 5e-8 * sf2
    n = g["Xc"].shape[0]
    assert np.abs(host(b["var"])[:n] - g["var"]).max() <= 1e-6 * sf2     # the golden tolerance of test_gpu_parity
    # the edge form's own error against the golden variance stays of the node form's size (c3: 2.2e-8 against 8.7e-9)
    err_node = np.abs(host(a["var"])[:n] - g["var"]).max()
    err_edge = np.abs(host(b["var"])[:n] - g["var"]).max()
    assert err_edge <= max(3.0 * err_node, 1e-8 * sf2)
    assert b["best_idx"] == int(np.argmax(host(b["score"])))
    if edge.camphor is None:
        rec = eng.search_sharded(edge, Xc, SCORE_POINTWISE_EI, mustar, 7)
        assert rec == (b["best_val"], b["best_idx"] + 7)


@pytest.mark.parametrize("m,n_q,D", [(25, 80, 20), (31, 9, 5), (7, 37, 3)])
def test_edge_form_ragged_shapes(eng, m, n_q, D):
    """m = 25 (the reference's default: N = 2080, E = 2000) and shapes off every tile / chunk boundary."""
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE, SCORE_VARIANCE
    rng = np.random.default_rng(m * 100 + n_q)
    N = n_q * (m + 1)
    X = rng.random((N, D))
    th = [1.0, 0.4, 1.3]
    Sinv = eng.pd_inverse(eng.gram(X, th, "SE_kernel"))
    f = 0.5 * eng.dgemv(eng.potrf_(eng.gram(eng.dev(X), th, "SE_kernel").clone()), rng.standard_normal(N), lower=True)
    node = eng.posterior(X, th, "SE_kernel", Sinv, f, m, form=FORM_NODE)
    edge = eng.posterior(X, th, "SE_kernel", Sinv, f, m, form=FORM_EDGE)
    check_layout(eng, edge)
    sf2 = th[2] ** 2
    for M in (1000, 5000):
        Xc = rng.random((M, D))
        a = eng.predict(node, Xc, score=SCORE_VARIANCE)
        b = eng.predict(edge, Xc, score=SCORE_VARIANCE)
        assert np.abs(host(a["var"]) - host(b["var"])).max() <= 1e-8 * sf2
    mu_a, cov_a = eng.predict_cov(node, Xc[:70])
    mu_b, cov_b = eng.predict_cov(edge, Xc[:70])
    assert np.array_equal(host(mu_a), host(mu_b))
    assert np.abs(host(cov_a) - host(cov_b)).max() <= 1e-8 * sf2


@pytest.mark.parametrize("name", [n for n in ("smoke", "c3") if n in ALL] + ["camphor_ard/spread"])
def test_gp_fit_and_posterior_give_the_same_edge_operator(eng, name):
    from ppbo_amd.engine import FORM_EDGE
    g = load(name)
    th, kern, m = g["theta"], str(g["kernel"]), int(g["m"])
    r = eng.gp_fit(g["X"], th, kern, m, g["f_init"], gtol=1e-6, form=FORM_EDGE)
    p = eng.posterior(g["X"], th, kern, r["Sigma_inv"], r["fMAP"], m, form=FORM_EDGE)
    assert r["post"].form == FORM_EDGE
    assert np.array_equal(host(r["post"].G), host(p.G))
    assert np.array_equal(host(r["post"].alpha), host(p.alpha))


@pytest.mark.parametrize("name", [n for n in ("smoke", "c2", "c3") if n in ALL] + ["matern/m52_small"])
def test_line_acquisitions_on_an_edge_form_model(eng, name):
    g = load(name)
    node, edge, sf2 = both_forms(eng, g)
    rng = np.random.default_rng(11)
    D = int(g["D"])
    B, G, S = 6, 70, 150
    al = np.linspace(0.005, 0.995, G)
    xis = np.eye(D)[np.arange(B) % D]
    xs = rng.random((B, D))
    xs[np.arange(B), np.arange(B) % D] = 0.0
    z = rng.standard_normal((S, G))
    mustar = float(g["line_mustar"])
    jit = 1e-9 * sf2
    ei_a, vm_a = eng.line_acq_xi(node, xis, xs, al, z, mustar, jitter=jit)
    ei_b, vm_b = eng.line_acq_xi(edge, xis, xs, al, z, mustar, jitter=jit)
    assert np.allclose(host(ei_a), host(ei_b), rtol=1e-7, atol=1e-9 * np.sqrt(sf2))
    assert np.allclose(host(vm_a), host(vm_b), rtol=1e-7, atol=1e-9 * sf2)
    grid = np.stack([al[:, None] * xis[b] + xs[b] for b in range(B)])
    ei_c, vm_c = eng.line_acq(edge, grid, z, mustar, jitter=jit)
    assert np.allclose(host(ei_c), host(ei_b), rtol=1e-9, atol=1e-12)
    mu_a, cov_a = eng.predict_cov(node, g["line_grid"])
    mu_b, cov_b = eng.predict_cov(edge, g["line_grid"])
    assert np.abs(host(cov_a) - host(cov_b)).max() <= 1e-8 * sf2
    assert np.abs(host(cov_b) - g["line_cov"]).max() <= 1e-6 * sf2


def test_engine_picks_the_form_by_the_fused_rule(eng):
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE
    assert eng.posterior_form("SE_kernel", 2048, 20, 31) == FORM_EDGE
    assert eng.posterior_form("SE_kernel", 256, 4, 31) == FORM_NODE
    assert eng.posterior_form("camphor_copper_kernel", 256, 6, 31) == FORM_EDGE


@pytest.mark.parametrize("name", [n for n in ("c2", "c3") if n in ALL] + ["camphor_ard/spread"])
def test_edge_form_with_fp32_kstar(eng, name):
    """The edge epilogue of the fp32 K* kernel: the same candidates scored on both forms with kstar_fp32 agree as the
    fp64 ones do, and stay within the fp32 option's tolerance of the fp64 edge-form result."""
    from ppbo_amd.engine import SCORE_VARIANCE
    g = load(name)
    node, edge, sf2 = both_forms(eng, g)
    Xc = np.concatenate([g["Xc"], np.random.default_rng(5).random((3000, g["Xc"].shape[1]))])
    a = host(eng.predict(node, Xc, score=SCORE_VARIANCE, kstar_fp32=True)["var"])
    b = host(eng.predict(edge, Xc, score=SCORE_VARIANCE, kstar_fp32=True)["var"])
    c = host(eng.predict(edge, Xc, score=SCORE_VARIANCE)["var"])
    assert np.abs(a - b).max() <= 5e-8 * sf2
    assert np.abs(b - c).max() <= 1e-4 * sf2


def test_a_form_outside_node_and_edge_is_refused(eng):
    """ppbo_model.form = 2, and ppbo_posterior(..., form = 2): a negative status and a message naming the form, from the
    argument checks (nothing is launched)."""
    import ctypes as C
    from ppbo_amd.engine import FORM_EDGE, _ptr
    g = load("smoke")
    th, kern, m = g["theta"], str(g["kernel"]), int(g["m"])
    Sinv = eng.pd_inverse(eng.gram(g["X"], th, kern))
    post = eng.posterior(g["X"], th, kern, Sinv, g["fMAP"], m, form=FORM_EDGE)
    md = eng._model(post, True)
    md.form = 2
    N, D = post.X.shape
    M, B, G, S = 64, 2, 16, 8
    Xc = eng.dev(np.random.default_rng(0).random((M, D)))
    z = eng.dev(np.random.default_rng(1).standard_normal((S, G)))
    mu, var, cov, ei, vm = eng.empty(M), eng.empty(M), eng.empty(M, M), eng.empty(B), eng.empty(B)
    buf = C.create_string_buffer(256)

    def refused(rc):
        assert rc < 0
        eng.lib.ppbo_last_error(eng.ctx, buf, 256)
        assert b"invalid argument" in buf.value and b"form" in buf.value, buf.value

    refused(eng.lib.ppbo_predict(eng.ctx, C.byref(md), _ptr(Xc), M, 0, 0.0, _ptr(mu), _ptr(var), None, None, None,
                                 eng._stream()))
    refused(eng.lib.ppbo_predict_cov(eng.ctx, C.byref(md), _ptr(Xc), M, 0.0, _ptr(mu), _ptr(cov), eng._stream()))
    refused(eng.lib.ppbo_line_acq(eng.ctx, C.byref(md), _ptr(Xc), B, G, 0.0, _ptr(z), S, 0.0, 0.0, _ptr(ei), _ptr(vm),
                                  eng._stream()))
    f = eng.dev(g["fMAP"]).reshape(-1)
    info = C.c_int(0)
    refused(eng.lib.ppbo_posterior(eng.ctx, _ptr(Sinv), _ptr(f), N, m, float(th[0]), _ptr(eng.empty(N)), _ptr(eng.empty(N)),
                                   _ptr(eng.empty(N)), _ptr(eng.empty(N, N)), None, 2, C.byref(info), eng._stream()))
    md.form = FORM_EDGE     # the same descriptor with its own form is taken
    assert eng.lib.ppbo_predict(eng.ctx, C.byref(md), _ptr(Xc), M, 0, 0.0, _ptr(mu), _ptr(var), None, None, None,
                                eng._stream()) == 0


@pytest.mark.parametrize("name", [n for n in ("smoke", "c3") if n in ALL])
def test_alternating_forms_on_one_engine_match_single_form_engines(name):
    """One engine serving a node-form and an edge-form posterior in turn (node, edge, node, edge) computes, bit for bit,
    what an engine that only ever saw one of the two computes: the form travels with the model, no call leaves anything
    behind for the next.  Every path compared here (posterior, predict, predict_cov, line_acq_xi) repeats bit for bit
    between two engines of the same form."""
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE, SCORE_POINTWISE_EI, Engine
    g = load(name)
    th, kern, m, sf2 = g["theta"], str(g["kernel"]), int(g["m"]), float(g["theta"][2]) ** 2
    rng = np.random.default_rng(17)
    D = int(g["D"])
    Xc = np.concatenate([g["Xc"][:1000], rng.random((3000, D))])
    B, G, S = 6, 70, 150
    al = np.linspace(0.005, 0.995, G)
    xis = np.eye(D)[np.arange(B) % D]
    xs = rng.random((B, D))
    xs[np.arange(B), np.arange(B) % D] = 0.0
    z = rng.standard_normal((S, G))
    mustar = float(np.max(g["mu"]))

    def build(e, form):
        return e.posterior(g["X"], th, kern, e.pd_inverse(e.gram(g["X"], th, kern)), g["fMAP"], m, form=form)

    def calls(e, post):
        p = e.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
        out = [host(p["mu"]), host(p["var"]), host(p["score"]), np.array([p["best_val"], p["best_idx"]])]
        out += [host(t) for t in e.predict_cov(post, g["line_grid"])]
        out += [host(t) for t in e.line_acq_xi(post, xis, xs, al, z, float(g["line_mustar"]), jitter=1e-9 * sf2)]
        return out

    forms = (FORM_NODE, FORM_EDGE)
    mixed = Engine(0)
    posts = {f: build(mixed, f) for f in forms}
    got = [(f, calls(mixed, posts[f])) for f in forms + forms]
    mixed.close()
    for form in forms:
        alone = Engine(0)
        post = build(alone, form)
        assert np.array_equal(host(post.G), host(posts[form].G))
        want = [calls(alone, post) for _ in range(2)]
        alone.close()
        for w, (_, r) in zip(want, [x for x in got if x[0] == form]):
            assert len(w) == len(r) == 8
            for a, b in zip(w, r):
                assert np.array_equal(a, b)
