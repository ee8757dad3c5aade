"""GPU: the answer to a query -- ppbo_line_choice(_xi) / Engine.line_choice(_xi) / GPModel.answer_pred, choice_pred
against the NumPy statement (tests/choice_numpy.py) on the same draws, the duel's closed form, an independent NumPy
stream, the tie / NaN / -1 rules, the refusals and the drop-in surface.

The per-draw check: with u_ref the reference's utilities (mean and covariance from Engine.predict_cov, as
test_line_acq_matches_oracle_with_same_draws takes them), every draw must satisfy
    u_ref[s, choice[b, s]] >= max_g u_ref[s, g] - tol,        tol = 1e-6 sigma_f,
the tolerance that test holds the same samples to; where the reference's top-two gap exceeds tol this is
choice == argmax.  At most 0.2 % of the reference's draws may have a gap <= tol (else the seed is a bad one)."""
import ctypes as C
import functools

import numpy as np
import pytest

import choice_numpy as cn
from conftest import load_golden
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model(form=None):
    """The smoke fixture's posterior at the reference's f_MAP: dict(post, g, D, sigma, sf)."""
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    g = load_golden("smoke")
    Sinv = eng.pd_inverse(eng.gram(g["X"], g["theta"], str(g["kernel"])))
    post = eng.posterior(g["X"], g["theta"], str(g["kernel"]), Sinv, g["fMAP"], int(g["m"]), form=form)
    return dict(post=post, g=g, D=int(g["D"]), sigma=float(g["theta"][0]), sf=float(g["theta"][2]))


def _lines(rng, D, B, G, fixture_line=None):
    """(xis, xs, alphas, grid) of B coordinate lines of G points; line 0 the fixture's own where given (G = 70)."""
    al = np.linspace(0.005, 0.995, G)
    xis, xs = np.zeros((B, D)), rng.random((B, D))
    xis[np.arange(B), np.arange(B) % D] = 1.0
    xs[np.arange(B), np.arange(B) % D] = 0.0
    grid = np.stack([orc.line_grid(xis[b], xs[b], al) for b in range(B)])
    if fixture_line is not None:
        grid[0] = fixture_line
    return xis, xs, al, grid


def _scattered(rng, D, B, G):
    return rng.random((B, G, D))


def _check(eng, mod, grid, z, e, sd, jit, out, groups=None, label=""):
    """The per-draw check of the module docstring on `groups` (all by default).  Groups outside `groups` (B = 513 checks
    the two on either side of the 512-group chunk boundary and the first two) are held only to consistency:
    count == bincount(choice) and prob == count / S, exactly, which every group is."""
    ch, cnt, pr = host(out["choice"]), host(out["count"]), host(out["prob"])
    B, G = grid.shape[:2]
    S = z.shape[0]
    assert ch.shape == (B, S) and cnt.shape == pr.shape == (B, G) and ch.dtype == cnt.dtype == np.int32
    assert ch.min() >= 0 and ch.max() < G
    for b in range(B):
        assert np.array_equal(cnt[b], np.bincount(ch[b], minlength=G))
    assert np.array_equal(pr, cnt / S)
    if G == 1:
        assert np.all(ch == 0)
        return
    tol = 1e-6 * mod["sf"]
    worst, close_n = 0.0, 0
    groups = range(B) if groups is None else groups
    for b in groups:
        mu, cov = eng.predict_cov(mod["post"], grid[b])
        u = cn.utilities(host(mu), host(cov), z, e, sd, jit)
        close = cn.top_two_gap(u) <= tol
        short = u.max(axis=1) - u[np.arange(S), ch[b]]
        worst, close_n = max(worst, float(short.max())), close_n + int(close.sum())
        assert np.all(short <= tol), (label, b, float(short.max()), tol)
        assert np.array_equal(ch[b][~close], u.argmax(axis=1)[~close])
    assert close_n <= 0.002 * S * len(groups), f"{label}: {close_n} reference draws within tol of a tie: another seed"
    print(f"line_choice {label}: worst u_max - u[choice] = {worst:.2e} (tol {tol:.2e}), {close_n} near-tied reference draws")


def _noise(mod, rng, S, G, on):
    return (rng.standard_normal((S, G)), mod["sigma"]) if on else (None, 0.0)


# ---------------------------------------------------------------- 1. per draw, same draws
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("form", ["node", "edge"])
def test_per_draw_against_numpy(eng, form, noise):
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE
    mod = _model({"node": FORM_NODE, "edge": FORM_EDGE}[form])
    g, D = mod["g"], mod["D"]
    rng = np.random.default_rng(11)
    B, G, S = 5, 70, 150
    xis, xs, al, grid = _lines(rng, D, B, G, g["line_grid"])
    z = rng.standard_normal((S, G))
    e, sd = _noise(mod, rng, S, G, noise)
    jit = 1e-9 * mod["sf"] ** 2
    out = eng.line_choice(mod["post"], grid, z, e, sd, jitter=jit, want_count=True, want_choice=True)
    _check(eng, mod, grid, z, e, sd, jit, out, label=f"{form} noise={noise}")
    # the same lines as (xi, x, alpha): the fixture's own line through its (xi, x) and the abscissae of its grid
    xis[0], xs[0] = g["line_xi"], g["line_x"]
    d = int(np.argmax(g["line_xi"]))
    al0 = (g["line_grid"][:, d] - g["line_x"][d]) / g["line_xi"][d]
    per = np.tile(al, (B, 1))
    per[0] = al0
    per[1:] = np.sort(np.clip(per[1:] + rng.normal(0.0, 0.003, (B - 1, G)), 0.0, 1.0), axis=1)
    grid_per = np.stack([orc.line_grid(xis[b], xs[b], per[b]) for b in range(B)])
    out = eng.line_choice_xi(mod["post"], xis, xs, per, z, e, sd, jitter=jit, want_count=True, want_choice=True)
    _check(eng, mod, grid_per, z, e, sd, jit, out, label=f"{form} noise={noise} xi, per-line alpha")
    grid_sh = np.stack([orc.line_grid(xis[b], xs[b], al0) for b in range(B)])
    out = eng.line_choice_xi(mod["post"], xis, xs, al0, z, e, sd, jitter=jit, want_count=True, want_choice=True)
    _check(eng, mod, grid_sh, z, e, sd, jit, out, label=f"{form} noise={noise} xi, shared alpha")


# ---------------------------------------------------------------- 2. shapes where the kernel can go wrong
SHAPES = ([(3, G, 150) for G in (1, 2, 3, 16, 17, 70, 128)]             # one point, tile edges, the LDS limit
          + [(3, 17, S) for S in (1, 15, 16, 17, 64, 65, 1000)]         # a wavefront's 16 draws, a workgroup's 64, split edges
          + [(1, 17, 150), (513, 17, 65)])                              # one group; the 512-group chunk


@pytest.mark.parametrize("B,G,S", SHAPES)
def test_shapes(eng, B, G, S):
    mod = _model()
    rng = np.random.default_rng(1000 * G + 10 * S + B)
    # lines and groups of scattered points, alternating
    grid = _lines(rng, mod["D"], B, G)[3]
    grid[1::2] = _scattered(rng, mod["D"], B, G)[1::2]
    z, e = rng.standard_normal((S, G)), rng.standard_normal((S, G))
    sd, jit = mod["sigma"], 1e-9 * mod["sf"] ** 2
    kw = dict(noise_sd=sd, jitter=jit, want_count=True, want_choice=True)
    out = eng.line_choice(mod["post"], grid, z, e, **kw)
    groups = None if B <= 3 else (0, 1, 511, 512)
    _check(eng, mod, grid, z, e, sd, jit, out, groups=groups, label=f"B={B} G={G} S={S}")
    again = eng.line_choice(mod["post"], grid, z, e, **kw)
    for k in ("prob", "count", "choice"):
        assert np.array_equal(host(out[k]), host(again[k]))
    if S >= 2:
        # the draws cut in two calls (other splits, other wavefronts): the same choices, and counts that add up
        h = S // 2
        lo = eng.line_choice(mod["post"], grid, z[:h], e[:h], **kw)
        hi = eng.line_choice(mod["post"], grid, z[h:], e[h:], **kw)
        assert np.array_equal(host(out["choice"]), np.concatenate([host(lo["choice"]), host(hi["choice"])], axis=1))
        assert np.array_equal(host(out["count"]), host(lo["count"]) + host(hi["count"]))
    # the outputs that were not asked for are not needed for the probabilities
    bare = eng.line_choice(mod["post"], grid, z, e, noise_sd=sd, jitter=jit)
    assert bare["count"] is None and bare["choice"] is None and np.array_equal(host(bare["prob"]), host(out["prob"]))


# ---------------------------------------------------------------- 3. G = 2 against the closed form
def test_pairs_against_the_closed_form(eng):
    """|prob[:, 0] - p| <= 5 sqrt(p (1 - p) / S), p = ppbo_predict_pairs' win probability: 64 bins at 5 standard errors
    fail a correct sampler with probability < 1e-4.  The prior block's shrinkage (1e-6) moves p by ~1e-6: far inside."""
    mod = _model()
    rng = np.random.default_rng(31)
    M, S = 64, 16384
    Xa, Xb = rng.random((M, mod["D"])), rng.random((M, mod["D"]))
    Xb[:8] = Xa[:8] + 0.02 * rng.standard_normal((8, mod["D"]))             # close calls as well
    p = host(eng.predict_pairs(mod["post"], Xa, Xb, want_best=False)["prob"])
    ze = eng.randn(5, 2, S, 2)
    out = eng.line_choice(mod["post"], np.stack([Xa, Xb], axis=1), ze[0], ze[1], want_count=True)
    pr = host(out["prob"])
    dev = np.abs(pr[:, 0] - p) / np.sqrt(p * (1.0 - p) / S)
    print(f"G = 2 against predict_pairs: worst deviation {dev.max():.2f} standard errors, p in [{p.min():.3f}, {p.max():.3f}]")
    assert np.all(host(out["count"]).sum(axis=1) == S)
    assert np.all(np.abs(pr[:, 0] - p) <= 5.0 * np.sqrt(p * (1.0 - p) / S))
    # a == b: nothing but the noise decides
    same = host(eng.line_choice(mod["post"], np.stack([Xa, Xa], axis=1), ze[0], ze[1])["prob"])
    assert np.all(np.abs(same[:, 0] - 0.5) <= 5.0 * np.sqrt(0.25 / S))


# ---------------------------------------------------------------- 4. distribution on a line, independent draws
def test_distribution_against_an_independent_stream(eng):
    """The fixture's line, 65536 device draws (ppbo_randn) against 2^20 NumPy draws of the restatement:
    per bin |dp| <= 5 sqrt(p (1 - p) (1 / S + 1 / S_ref)) + 1 / S_ref."""
    mod = _model()
    g = mod["g"]
    G, S, S_ref, chunk = 70, 65536, 2 ** 20, 2 ** 16
    jit = 1e-9 * mod["sf"] ** 2
    ze = eng.randn(77, 2, S, G)
    pr = host(eng.line_choice(mod["post"], g["line_grid"][None], ze[0], ze[1], jitter=jit)["prob"])[0]
    mu, cov = (host(t) for t in eng.predict_cov(mod["post"], g["line_grid"]))
    rng = np.random.default_rng(123)
    count = np.zeros(G, dtype=np.int64)
    for _ in range(S_ref // chunk):
        count += cn.choice(mu, cov, rng.standard_normal((chunk, G)), rng.standard_normal((chunk, G)), mod["sigma"], jit)[1]
    p = count / S_ref
    band = 5.0 * np.sqrt(p * (1.0 - p) * (1.0 / S + 1.0 / S_ref)) + 1.0 / S_ref
    print(f"line distribution: worst |dp| / band = {np.max(np.abs(pr - p) / band):.2f}, max p = {p.max():.3f}")
    assert abs(pr.sum() - 1.0) <= 1e-12
    assert np.all(np.abs(pr - p) <= band)


# ---------------------------------------------------------------- 5. rules
def test_nan_rules(eng):
    mod = _model()
    rng = np.random.default_rng(41)
    B, G, S = 3, 17, 100
    grid = _lines(rng, mod["D"], B, G)[3]
    z, e = rng.standard_normal((S, G)), rng.standard_normal((S, G))
    kw = dict(noise_sd=mod["sigma"], jitter=1e-9 * mod["sf"] ** 2, want_count=True, want_choice=True)
    clean = eng.line_choice(mod["post"], grid, z, e, **kw)
    # a group with a NaN coordinate: -1 in every draw, nothing counted; the other groups bit for bit
    bad = grid.copy()
    bad[1, 5, 0] = np.nan
    out = eng.line_choice(mod["post"], bad, z, e, **kw)
    assert np.all(host(out["choice"])[1] == -1) and np.all(host(out["count"])[1] == 0) and np.all(host(out["prob"])[1] == 0.0)
    for k in ("prob", "count", "choice"):
        assert np.array_equal(host(out[k])[[0, 2]], host(clean[k])[[0, 2]])
    # NaN never wins: a NaN utility leaves the draw to the other points; a draw without a number chooses -1
    e2 = e.copy()
    win = host(clean["choice"])[:, 3]                     # draw 3: take its winner of group 0 out
    e2[3, win[0]] = np.nan
    e2[7, :] = np.nan
    out = eng.line_choice(mod["post"], grid, z, e2, **kw)
    ch, cnt = host(out["choice"]), host(out["count"])
    assert ch[0, 3] != win[0] and ch[0, 3] >= 0
    assert np.all(ch[:, 7] == -1) and np.all(cnt.sum(axis=1) == S - 1)
    keep = np.ones(S, dtype=bool)
    keep[[3, 7]] = False
    assert np.array_equal(ch[:, keep], host(clean["choice"])[:, keep])
    # ties go to the lower index, within a tile's lanes and across tiles: equal utilities (+inf) at two points
    e3 = e.copy()
    e3[0, [11, 3]], e3[1, [16, 2]], e3[2, 16], e3[4, [15, 16]] = np.inf, np.inf, np.inf, np.inf
    ch = host(eng.line_choice(mod["post"], grid, z, e3, **kw)["choice"])
    assert np.all(ch[:, 0] == 3) and np.all(ch[:, 1] == 2) and np.all(ch[:, 2] == 16) and np.all(ch[:, 4] == 15)


def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd.engine import SHRINKAGE, _ptr
    import torch
    mod = _model()
    post = mod["post"]
    rng = np.random.default_rng(51)
    B, G, S = 3, 17, 40
    xis, xs, al, grid = _lines(rng, mod["D"], B, G)
    z, e = rng.standard_normal((S, G)), rng.standard_normal((S, G))
    before = eng.line_choice(post, grid, z, e, want_count=True, want_choice=True)
    dg, dz, de, dxi, dx, da = (eng.dev(a) for a in (grid, z, e, xis, xs, al))
    prob = eng.empty(B, G)
    md, bare = eng._model(post, True), eng._model(post, False)
    ok = dict(model=md, grid=dg, B=B, G=G, z=dz, e=de, S=S, sd=mod["sigma"], jit=0.0, prob=prob)

    def call(model, grid, B, G, z, e, S, sd, jit, prob):
        rc = eng.lib.ppbo_line_choice(eng.ctx, C.byref(model) if model is not None else None, _ptr(grid), B, G, SHRINKAGE,
                                      _ptr(z), _ptr(e), S, sd, jit, _ptr(prob), None, None, eng._stream())
        return rc, eng._err()

    def call_xi(model, xi, x, a, B, G, z, e, S, sd, jit, prob):
        rc = eng.lib.ppbo_line_choice_xi(eng.ctx, C.byref(model) if model is not None else None, _ptr(xi), _ptr(x), _ptr(a),
                                         0, B, G, SHRINKAGE, _ptr(z), _ptr(e), S, sd, jit, _ptr(prob), None, None,
                                         eng._stream())
        return rc, eng._err()

    assert call(**ok)[0] == 0
    for kw in (dict(model=None), dict(grid=None), dict(z=None), dict(prob=None), dict(G=0), dict(G=129), dict(G=-1),
               dict(B=0), dict(B=-2), dict(S=0), dict(S=-1), dict(sd=-0.1), dict(sd=float("nan")), dict(sd=float("inf")),
               dict(jit=-1e-9), dict(jit=float("nan")), dict(jit=float("inf")), dict(e=None), dict(model=bare)):
        rc, msg = call(**{**ok, **kw})
        assert rc < 0 and msg.startswith("invalid argument"), (kw, rc, msg)
    assert call(**{**ok, "e": None, "sd": 0.0})[0] == 0                  # no noise needs no noise draws
    okx = dict(model=md, xi=dxi, x=dx, a=da, B=B, G=G, z=dz, e=de, S=S, sd=mod["sigma"], jit=0.0, prob=prob)
    assert call_xi(**okx)[0] == 0
    for kw in (dict(model=None), dict(xi=None), dict(x=None), dict(a=None), dict(z=None), dict(prob=None), dict(G=129),
               dict(G=0), dict(B=0), dict(S=0), dict(sd=-0.1), dict(jit=float("nan")), dict(e=None), dict(model=bare)):
        rc, msg = call_xi(**{**okx, **kw})
        assert rc < 0 and msg.startswith("invalid argument"), (kw, rc, msg)
    torch.cuda.synchronize()
    after = eng.line_choice(post, grid, z, e, want_count=True, want_choice=True)
    for k in ("prob", "count", "choice"):
        assert np.array_equal(host(before[k]), host(after[k]))
    # through Engine: a ValueError before the device
    with pytest.raises(ValueError, match="line_choice"):
        eng.line_choice(post, rng.random((2, 129, mod["D"])), rng.standard_normal((S, 129)), None, noise_sd=0.0)
    with pytest.raises(ValueError, match="line_choice"):
        eng.line_choice(post, grid, z, None)                           # noise_sd = theta[0] without draws for it
    with pytest.raises(ValueError, match="line_choice_xi"):
        eng.line_choice_xi(post, xis, xs[:2], al, z, e)
    # a posterior without its variance operator
    mean_only = eng.mean_posterior(mod["g"]["X"], mod["g"]["theta"], str(mod["g"]["kernel"]), int(mod["g"]["m"]), post.alpha)
    with pytest.raises(RuntimeError, match="invalid argument"):
        eng.line_choice(mean_only, grid, z, e)


# ---------------------------------------------------------------- 6. the drop-in surface
def _golden_gp(name):
    """A GPModel on the reference's own design and f_MAP (the set-up of tests/test_gpu_dropin.py); the ARD fixtures keep
    their length scales apart and carry no bounds: the unit box."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    g = load_golden(name)
    D = int(g["D"])
    if "theta_l" in g:
        theta, bounds = [float(g["theta_sf"][0]), g["theta_l"].copy(), float(g["theta_sf"][1])], ((0.0, 1.0),) * D
    else:
        theta, bounds = list(g["theta"]), tuple(map(tuple, g["bounds"]))
    st = PPBO_settings(D=D, bounds=bounds, xi_acquisition_function="PCD", theta_initial=theta, m=int(g["m"]),
                       verbose=False, kernel=str(g["kernel"]))
    gp = GPModel(st)
    np.random.seed(0)
    gp.update_feedback_processing_object(g["X_obs"])
    gp.FP.X = g["X"].copy()
    gp.update_data()
    gp.set_theta(); gp.update_Sigma(gp.theta); gp.update_Sigma_inv(gp.theta)
    gp.fMAP = g["fMAP"].copy()
    gp.initialization_running = False
    gp._post = gp.eng.posterior(gp._dX, gp.theta, gp.kernel.__name__, gp._dSigma_inv, gp.eng.dev(gp.fMAP), gp.m)
    gp._post_mean = gp._post
    return gp, g


@pytest.mark.parametrize("name", ["ard/se_d4", "cam_small"])
def test_answer_pred_and_choice_pred(name):
    gp, g = _golden_gp(name)
    D, S = gp.D, 2048
    xi, x = g["line_xi"], g["line_x"]
    sf2 = float(gp.theta[2]) ** 2
    # one line, the default abscissae
    al, p = gp.answer_pred(xi, x, n_draws=S, seed=3)
    assert al.shape == p.shape == (70,) and np.array_equal(al, np.linspace(0.005, 0.995, 70))
    assert abs(p.sum() - 1.0) <= 1e-12 and p.min() >= 0.0
    assert np.array_equal(gp.answer_pred(xi, x, n_draws=S, seed=3)[1], p)
    assert not np.array_equal(gp.answer_pred(xi, x, n_draws=S, seed=4)[1], p)
    np.random.seed(9)
    a = gp.answer_pred(xi, x, n_draws=S)[1]
    np.random.seed(9)
    assert np.array_equal(gp.answer_pred(xi, x, n_draws=S)[1], a)          # seed = None: off the global NumPy stream
    # Engine.line_choice_xi on the seed's stream -- z its first S G normals, e the next S G, noise theta[0] -- and with
    # neither e nor noise for noisy = False: bit for bit (the seed, the order of z and e, jitter and shrinkage)
    ze = gp.eng.randn(3, 2, S, 70)
    kw = dict(shrink=gp.COVARIANCE_SHRINKAGE, jitter=1e-10 * sf2)
    ref = host(gp.eng.line_choice_xi(gp._post, xi[None], x[None], al, ze[0], ze[1], float(gp.theta[0]), **kw)["prob"])[0]
    assert np.array_equal(ref, p)
    ref_free = host(gp.eng.line_choice_xi(gp._post, xi[None], x[None], al, ze[0], None, 0.0, **kw)["prob"])[0]
    assert np.array_equal(ref_free, gp.answer_pred(xi, x, n_draws=S, noisy=False, seed=3)[1])
    assert not np.array_equal(ref_free, ref)
    # the host's grid through Engine.line_choice: its points differ from the device's in their last bits (alpha xi + x
    # formed here), which can turn a draw whose top two are within ~1e-15: at most one draw of the 2048
    grid = orc.line_grid(xi, x, al)[None]
    ref = host(gp.eng.line_choice(gp._post, grid, ze[0], ze[1], None, **kw)["prob"])[0]
    assert np.abs(ref - p).max() <= 1.0 / S
    # stacked lines, abscissae of the caller's
    rng = np.random.default_rng(61)
    xis, xs = np.vstack([xi, rng.random((2, D))]), np.vstack([x, rng.random((2, D)) * 0.1])
    al5 = np.linspace(0.0, 1.0, 33)
    al_out, pB = gp.answer_pred(xis, xs, alphas=al5, n_draws=S, seed=3)
    assert al_out.shape == (33,) and pB.shape == (3, 33) and np.abs(pB.sum(axis=1) - 1.0).max() <= 1e-12
    # without the likelihood's noise the best bin of a line holds more of the mass.  The line: the coordinate line through
    # the design's best row, 128 abscissae over a segment of 0.04 around it.  Neighbouring points are 3e-4 apart, so their
    # utilities differ by far less than the noise (sigma sqrt 2) on either fixture -- cam_small's sigma = 0.01 sigma_f
    # included, where on the 70-point grid of [0, 1] the noise moves a draw or two of 2048 either way -- while the path's
    # range over the segment exceeds it: the noise spreads the answer over many bins that the path itself tells apart
    best = g["X"][int(np.argmax(g["fMAP"]))]
    xi_b, x_b = np.zeros(D), best.copy()
    xi_b[0], x_b[0] = 1.0, 0.0
    lo = min(max(float(best[0]) - 0.02, 0.0), 0.96)
    seg = np.linspace(lo, lo + 0.04, 128)
    p_noisy = gp.answer_pred(xi_b, x_b, alphas=seg, n_draws=S, seed=3)[1]
    p_free = gp.answer_pred(xi_b, x_b, alphas=seg, n_draws=S, noisy=False, seed=3)[1]
    k = int(np.argmax(p_free))
    se = np.sqrt((p_free[k] * (1.0 - p_free[k]) + p_noisy[k] * (1.0 - p_noisy[k])) / S)
    print(f"answer_pred {name}: best bin {k} holds {p_free[k]:.4f} noise-free, {p_noisy[k]:.4f} with noise "
          f"(difference {(p_free[k] - p_noisy[k]) / se:.1f} standard errors of independent draws)")
    assert abs(p_free.sum() - 1.0) <= 1e-12 and abs(p_noisy.sum() - 1.0) <= 1e-12
    assert p_free[k] > p_noisy[k]
    # shortlists
    items = rng.random((6, D))
    q = gp.choice_pred(items, n_draws=S, seed=8)
    assert q.shape == (6,) and abs(q.sum() - 1.0) <= 1e-12
    assert np.array_equal(gp.choice_pred(items, n_draws=S, seed=8), q)
    assert not np.array_equal(gp.choice_pred(items, n_draws=S, seed=9), q)
    ze = gp.eng.randn(8, 2, S, 6)
    ref = host(gp.eng.line_choice(gp._post, items[None], ze[0], ze[1], None, gp.COVARIANCE_SHRINKAGE, 1e-10 * sf2)["prob"])[0]
    assert np.array_equal(ref, q)
    qB = gp.choice_pred(np.stack([items, items[::-1]]), n_draws=S, seed=8)
    assert qB.shape == (2, 6) and np.array_equal(qB[0], q) and np.abs(qB.sum(axis=1) - 1.0).max() <= 1e-12
    # two items: preference_pred's p within 5 binomial standard errors
    pair = gp.choice_pred(items[:2], n_draws=16384, seed=2)
    p2 = gp.preference_pred(items[0], items[1])[2][0]
    assert abs(pair[0] - p2) <= 5.0 * np.sqrt(p2 * (1.0 - p2) / 16384)
