"""GPU: main effects and interactions -- ppbo_predict_marginals / Engine.predict_marginals / GPModel.marginal_pred and its
layers against the NumPy statement (tests/marginals_numpy.py, whose closed forms tests/test_marginals_host.py confirms by
quadrature; the oracle's dense variance operator), the exact identities of the construction, the bitwise promises, the
NaN rule and the refusals.

Bound (TOL = 1e-6, the package's parity standard), normalised as the functionals test normalises:
max|mu - ref| / max|ref|, max|var - ref| / sf^2, max|p - ref|.  Shapes: N = 52 and 78 (stars of 26, off every tile edge) and
N = 64 (32-row stars).

Measured on MI355X: see profiles/r20_marginals.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

import marginals_numpy as mn
import pairs_numpy as pn
import slopes_numpy as sn
from conftest import load_golden
from test_gpu_pairs import TOL, _fitted, _fitted_golden, _forms, host

pytestmark = pytest.mark.gpu

EFFECTS = (mn.RAW, mn.CENTRED, mn.INTERACTION)
NAMES = {mn.RAW: "raw", mn.CENTRED: "centred", mn.INTERACTION: "interaction"}
# D -> (n_q, m, forms): N = 52 / 78 (m = 25) and 64 (m = 31); both operator forms
SHAPES = {1: (2, 25, ("node",)), 2: (3, 25, ("edge",)), 3: (2, 31, ("node",)), 6: (3, 25, ("node", "edge")),
          20: (2, 25, ("node", "edge")), 40: (2, 31, ("edge",)), 64: (3, 25, ("node",))}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _se(D, form):
    n_q, m, _ = SHAPES[D]
    return _fitted("SE_kernel", D, _forms()[form], n_q=n_q, m=m)


@functools.lru_cache(maxsize=None)
def _fitted_ard_golden():
    """tests/golden/ard/se_d4.npz: SE with l = (0.05, 0.3, 0.6, 1.2), N = 192."""
    from ppbo_amd.engine import get_engine
    g = load_golden("ard/se_d4")
    X, m = g["X"], int(g["m"])
    th = [float(g["theta_sf"][0]), np.asarray(g["theta_l"], dtype=float), float(g["theta_sf"][1])]
    r = get_engine(0).gp_fit(X, th, "SE_kernel", m, g["f_init"], gtol=1e-6)
    assert r["post"] is not None
    alpha, A = pn.operator_from_fit(X, th, "SE_kernel", m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel="SE_kernel", alpha=alpha, A=A)


@functools.lru_cache(maxsize=None)
def _fitted_camphor_ard_golden():
    """tests/golden/camphor_ard/spread.npz as the per-coordinate camphor kernel, l = (0.1, 0.1, 0.5, 1, 1, 1), N = 192."""
    from ppbo_amd.engine import get_engine
    g = load_golden("camphor_ard/spread")
    X, m = g["X"], int(g["m"])
    th = [float(g["theta_sf"][0]), np.asarray(g["theta_l"], dtype=float), float(g["theta_sf"][1])]
    r = get_engine(0).gp_fit(X, th, sn.CAMPHOR_ARD, m, g["f_init"], gtol=1e-6)
    assert r["post"] is not None
    alpha, A = sn.operator_from_fit(X, th, sn.CAMPHOR_ARD, m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel=sn.CAMPHOR_ARD, alpha=alpha, A=A)


def _rows(rng, mod, M, effect):
    """M rows that mix orders and axes from lane to lane: order 2 everywhere under INTERACTION, else orders 0, 1, 2 in
    turn; values uniform in the box, some of them 0, 1 and coordinates of design rows."""
    N, D = mod["X"].shape
    dims = np.full((M, 2), -1)
    t = rng.random((M, 2))
    order = np.full(M, 2) if effect == mn.INTERACTION else rng.integers(0, 3, M)
    if D == 1:
        order = np.minimum(order, 1)
    for i in range(M):
        if order[i] >= 1:
            dims[i, 0] = rng.integers(0, D)
        if order[i] == 2:
            dims[i, 1] = (dims[i, 0] + 1 + rng.integers(0, D - 1)) % D
    k = max(1, M // 8)
    t[:k, 0] = np.where(np.arange(k) % 2, 0.0, 1.0)
    for i in range(k, min(2 * k, M)):
        if dims[i, 0] >= 0:
            t[i, 0] = mod["X"][rng.integers(0, N), dims[i, 0]]
    return dims, t


def _errors(mod, dims, t, effect, mu, var, p):
    mu0, var0, _ = mn.marginal_reference(dims, t, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"], effect)
    p0 = mn.sign_probability(mu0, var0)
    sf2 = float(mod["th"][2]) ** 2
    zero = (dims < 0).all(axis=1) & (effect == mn.CENTRED)          # the zero functional: exact, and p = 1/2 by rule
    if zero.any():
        assert np.all(mu[zero] == 0.0) and np.all(var[zero] == 0.0) and np.all(p[zero] == 0.5)
    live = ~zero
    if not live.any():
        return 0.0, 0.0, 0.0
    scale = np.abs(mu0).max()
    return (np.abs(mu - mu0).max() / scale, np.abs(var - var0).max() / sf2, np.abs(p - p0)[live].max())


def _parity(eng, mod, M=257, seed=3, label="", effects=EFFECTS, call=None):
    worst = np.zeros(3)
    D = mod["X"].shape[1]
    for effect in effects:
        if effect == mn.INTERACTION and D == 1:
            continue
        rng = np.random.default_rng(seed + 10 * effect + M)
        dims, t = _rows(rng, mod, M, effect)
        if call is None:
            out = eng.predict_marginals(mod["post"], dims, t, effect=effect)
            mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
            finite = ~np.isnan(p)
            assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max() and finite.all()
        else:
            mu, var, p = call(dims, t, NAMES[effect])
        e = np.array(_errors(mod, dims, t, effect, mu, var, p))
        worst = np.maximum(worst, e)
        print(f"marginals parity {label} {NAMES[effect]} M={M}: |mu - ref| / max|ref| = {e[0]:.2e}, "
              f"|var - ref| / sf2 = {e[1]:.2e}, |p - ref| = {e[2]:.2e}")
        assert np.all(e <= TOL), (label, NAMES[effect], M, e)
    return worst


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("D,form", [(D, f) for D, s in SHAPES.items() for f in s[2]])
def test_parity_se(eng, D, form):
    _parity(eng, _se(D, form), label=f"SE D={D} N={SHAPES[D][0] * (SHAPES[D][1] + 1)} {form}")


@pytest.mark.parametrize("M", [1, 255, 256])
def test_parity_call_sizes(eng, M):
    _parity(eng, _se(6, "node"), M=M, label="SE D=6")


def test_parity_ard(eng):
    _parity(eng, _fitted_ard_golden(), label="SE ARD ard/se_d4")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    mod = _fitted_golden("cam_small", _forms()[form])
    assert mod["kernel"] == mn.CAMPHOR
    _parity(eng, mod, label=f"camphor cam_small {form}")


def _stub_gp(eng, mod):
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp.eng, gp._post, gp.D = eng, mod["post"], mod["X"].shape[1]
    return gp


def test_parity_camphor_ard_through_marginal_pred(eng):
    """SE on the 11 embedded columns; the column comes from the caller's six-column rows and the six length scales."""
    mod = _fitted_camphor_ard_golden()
    gp = _stub_gp(eng, mod)
    _parity(eng, mod, label="camphor ARD camphor_ard/spread (marginal_pred)", call=gp.marginal_pred)


def test_chunk_edge(eng):
    """M = 65541 order-2 and order-1 rows cross a chunk: parity on rows either side of the edge, the argmax across
    chunks, one call against the tail alone bitwise."""
    mod = _se(6, "node")
    rng = np.random.default_rng(9)
    M = 65541
    dims, t = _rows(rng, mod, M, mn.CENTRED)
    full = eng.predict_marginals(mod["post"], dims, t, effect=mn.CENTRED, want_score=True)
    mu, var, p = host(full["mu"]), host(full["var"]), host(full["prob"])
    sel = np.r_[0:64, 65536 - 64:65541]
    e = _errors(mod, dims[sel], t[sel], mn.CENTRED, mu[sel], var[sel], p[sel])
    print(f"marginals parity across the chunk edge (M = 65541): mu {e[0]:.2e}, var {e[1]:.2e}, p {e[2]:.2e}")
    assert max(e) <= TOL
    assert np.array_equal(host(full["score"]), p)
    i = int(np.argmax(p))
    assert full["best_idx"] == i and full["best_val"] == p[i]
    tail = eng.predict_marginals(mod["post"], dims[65536:], t[65536:], effect=mn.CENTRED)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(full[k])[65536:], host(tail[k]))


# ---------------------------------------------------------------- 2. exact identities
def test_raw_with_both_axes_kept_is_the_point_prediction(eng):
    """D = 2, RAW with both axes kept: c_j = P_j r_d r_e = k(x, x_j) and the prior is sf^2 -- ppbo_predict at the same
    points.  Other instructions, so the parity bound; the measured value is printed."""
    mod = _se(2, "edge")
    rng = np.random.default_rng(4)
    M = 513
    pts = rng.random((M, 2))
    pts[:8] = mod["X"][:8]
    out = eng.predict_marginals(mod["post"], np.tile([0, 1], (M, 1)), pts, effect=mn.RAW)
    ref = eng.predict(mod["post"], pts, want_best=False)
    sf2 = float(mod["th"][2]) ** 2
    e_mu = np.abs(host(out["mu"]) - host(ref["mu"])).max() / np.abs(host(ref["mu"])).max()
    e_var = np.abs(host(out["var"]) - host(ref["var"])).max() / sf2
    print(f"RAW with both axes kept against ppbo_predict (D = 2): mu {e_mu:.2e}, var {e_var:.2e}")
    assert e_mu <= TOL and e_var <= TOL


@pytest.mark.parametrize("D,form", [(2, "edge"), (6, "node")])
def test_decomposition_and_vanishing_integrals(eng, D, form):
    """RAW(t, u) = fbar + C_d(t) + C_e(u) + INT(t, u) for the means, and the centred main effect and the pure interaction,
    summed over Gauss-Legendre nodes in t with their weights, vanish: both to 1e-10 of sum_j |c_j alpha_j| (c the RAW
    column of the row; for the integrals the largest over the nodes)."""
    mod = _se(D, form)
    post = mod["post"]
    rng = np.random.default_rng(12)
    M = 200
    d = rng.integers(0, D, M)
    e = (d + 1 + rng.integers(0, D - 1, M)) % D
    de, t = np.stack([d, e], axis=1), rng.random((M, 2))
    mean = lambda dims, tt, eff: host(eng.predict_marginals(post, dims, tt, effect=eff, want_var=False, want_prob=False,
                                                            kind=0, want_best=False)["mu"])
    raw, inter = mean(de, t, mn.RAW), mean(de, t, mn.INTERACTION)
    cd, ce = mean(d, t[:, 0], mn.CENTRED), mean(e, t[:, 1], mn.CENTRED)
    fbar = mean(np.full((1, 2), -1), np.zeros((1, 2)), mn.RAW)[0]
    l, per = mn.axes_of(mod["th"], mod["kernel"], D)
    c = mn.marginal_column(de, t, mod["X"], l, per, float(mod["th"][2]) ** 2, mn.RAW)
    scale = np.abs(c) @ np.abs(mod["alpha"])
    err = np.max(np.abs(raw - (fbar + cd + ce + inter)) / scale)
    print(f"decomposition RAW = fbar + C_d + C_e + INT (D = {D}): {err:.2e} of sum |c_j alpha_j|")
    assert err <= 1e-10
    x, w = np.polynomial.legendre.leggauss(64)
    x, w = 0.5 * (x + 1.0), 0.5 * w
    worst = 0.0
    for axis, other, u in ((0, D - 1, 0.3), (D - 1, 0, 0.85)):
        cm = mean(np.full(64, axis), x, mn.CENTRED)
        dims = np.tile([axis, other], (64, 1))
        tt = np.stack([x, np.full(64, u)], axis=1)
        ci = mean(dims, tt, mn.INTERACTION)
        sc = (np.abs(mn.marginal_column(dims, tt, mod["X"], l, per, float(mod["th"][2]) ** 2, mn.RAW)) @ np.abs(mod["alpha"])).max()
        worst = max(worst, abs(w @ cm) / sc, abs(w @ ci) / sc)
    print(f"integrals of the centred main effect and the pure interaction over t (D = {D}): {worst:.2e} of sum |c_j alpha_j|")
    assert worst <= 1e-10


# ---------------------------------------------------------------- 3. bitwise promises
def _raw_call(eng, post, ax, dims, t, effect, kind=2, want_best=False):
    """ppbo_predict_marginals itself, on rows exactly as given (Engine.predict_marginals canonicalises them first)."""
    from ppbo_amd.engine import _ptr
    import torch
    d_dims = eng.dev(np.ascontiguousarray(dims, dtype=np.int32), dtype=torch.int32)
    d_t = eng.dev(np.ascontiguousarray(t, dtype=float))
    M = d_dims.shape[0]
    md = eng._model(post, True)
    mu, var, pr = eng.empty(M), eng.empty(M), eng.empty(M)
    bv, bi = C.c_double(0.0), C.c_int64(-1)
    rc = eng.lib.ppbo_predict_marginals(eng.ctx, C.byref(md), C.byref(ax), _ptr(d_dims), _ptr(d_t), M, effect, kind, _ptr(mu),
                                        _ptr(var), _ptr(pr), None, C.byref(bv) if want_best else None,
                                        C.byref(bi) if want_best else None, eng._stream())
    assert rc == 0, eng._err()
    return host(mu), host(var), host(pr), bv.value, bi.value


@pytest.mark.parametrize("D,form", [(6, "edge"), (20, "node")])
def test_bitwise_promises(eng, D, form):
    mod = _se(D, form)
    post = mod["post"]
    ax = eng.marginal_axes(post)
    rng = np.random.default_rng(20)
    for effect in EFFECTS:
        dims, t = _rows(rng, mod, 257, effect)
        a = _raw_call(eng, post, ax, dims, t, effect)
        b = _raw_call(eng, post, ax, dims, t, effect)
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v)                                   # repeated calls
        sw = _raw_call(eng, post, ax, dims[:, ::-1], t[:, ::-1], effect) if effect == mn.INTERACTION else None
        if sw is None:                                                    # swap the order-2 rows only: (-1, d) is refused
            two = dims[:, 1] >= 0
            ds, ts = dims.copy(), t.copy()
            ds[two], ts[two] = dims[two][:, ::-1], t[two][:, ::-1]
            sw = _raw_call(eng, post, ax, ds, ts, effect)
        for u, v in zip(a[:3], sw[:3]):
            assert np.array_equal(u, v)                                   # swapped axis order
        # a row does not see its place in the call nor M: reversed, alone, and inside a call of another size class
        rev = _raw_call(eng, post, ax, dims[::-1], t[::-1], effect)
        one = _raw_call(eng, post, ax, dims[100:101], t[100:101], effect)
        big_d, big_t = _rows(rng, mod, 3000, effect)
        big_d[1500:1757], big_t[1500:1757] = dims, t
        big = _raw_call(eng, post, ax, big_d, big_t, effect)
        for k in range(3):
            assert np.array_equal(rev[k][::-1], a[k])
            assert one[k][0] == a[k][100]
            assert np.array_equal(big[k][1500:1757], a[k])
    zero = _raw_call(eng, post, ax, np.full((70, 2), -1), rng.random((70, 2)), mn.CENTRED, want_best=True)
    assert np.all(zero[0] == 0.0) and np.all(zero[1] == 0.0) and np.all(zero[2] == 0.5)
    assert zero[3] == 0.5 and zero[4] == 0                                # all tied: the first index


# ---------------------------------------------------------------- 4. NaN rows and the argmax
@pytest.mark.parametrize("form", ["node", "edge"])
def test_nan_rows_score_kinds_and_argmax(eng, form):
    from ppbo_amd.engine import PAIR_MEAN, PAIR_PROB, PAIR_VARIANCE
    mod = _se(6, form)
    post = mod["post"]
    ax = eng.marginal_axes(post)
    rng = np.random.default_rng(10)
    M = 1001
    dims, t = _rows(rng, mod, M, mn.CENTRED)
    dims[[3, 10, 999]] = [[2, -1], [0, 4], [5, 1]]
    clean = _raw_call(eng, post, ax, dims, t, mn.CENTRED)
    t[3, 0], t[10, 1], t[999, 0] = np.nan, np.inf, -np.inf
    unused = dims[:, 1] < 0
    unused[[3, 10, 999]] = False
    t[unused, 1] = np.nan                                # a value on an axis that is not kept is not read
    bad = np.zeros(M, dtype=bool)
    bad[[3, 10, 999]] = True
    for kind, k in ((PAIR_MEAN, 0), (PAIR_VARIANCE, 1), (PAIR_PROB, 2)):
        out = _raw_call(eng, post, ax, dims, t, mn.CENTRED, kind=kind, want_best=True)
        for j in range(3):
            assert np.all(np.isnan(out[j][bad])) and np.array_equal(out[j][~bad], clean[j][~bad])
        assert out[4] == int(np.nanargmax(out[k])) and out[3] == np.nanmax(out[k]) and not bad[out[4]]
    none = _raw_call(eng, post, ax, dims[[3, 10]], t[[3, 10]], mn.CENTRED, want_best=True)
    assert none[4] == -1 and np.isnan(none[3])
    # the Python layer: the same rows, the mean alone from a model without an operator
    bare = eng.mean_posterior(mod["X"], mod["th"], mod["kernel"], mod["m"], post.alpha)
    t2 = np.where(np.isnan(t) & ~bad[:, None], 0.0, t)
    mean = eng.predict_marginals(bare, dims, t2, effect=mn.CENTRED, kind=PAIR_MEAN, want_var=False, want_prob=False,
                                 want_score=True)
    assert mean["var"] is None and mean["prob"] is None
    assert np.array_equal(host(mean["mu"])[~bad], clean[0][~bad]) and np.all(np.isnan(host(mean["mu"])[bad]))
    assert mean["best_idx"] == int(np.nanargmax(host(mean["score"])))


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_context_usable(eng):
    import torch
    from ppbo_amd import _lib
    from ppbo_amd.engine import PAIR_MEAN, PAIR_PROB, _ptr
    mod = _se(6, "node")
    post = mod["post"]
    rng = np.random.default_rng(11)
    M = 100
    dims, t = _rows(rng, mod, M, mn.INTERACTION)
    before = eng.predict_marginals(post, dims, t, effect=mn.INTERACTION)
    d_dims, d_t = eng.dev(dims.astype(np.int32), dtype=torch.int32), eng.dev(t)
    mu = eng.dev(np.full(M, -7.0))                      # the sentinel a refused call must leave alone
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    rq = _fitted("RQ_kernel", 6, None)
    m52 = _fitted("Matern52_kernel", 6, None)
    ax = eng.marginal_axes(post)
    Xu, l, per, i0 = ax._Xu, ax._l.copy(), ax._per.copy(), ax._i0.copy()

    def axes(Dc=6, xu=True, l_=l, per_=per, i0_=i0, null=None):
        a = _lib.marginal_axes(Xu.data_ptr() if xu else None, l_, per_, i0_)
        a.Dc = Dc
        if null:
            setattr(a, null, None)
        return a

    def call(model, a, dd, tt, M_, effect, kind):
        rc = eng.lib.ppbo_predict_marginals(eng.ctx, C.byref(model) if model is not None else None,
                                            C.byref(a) if a is not None else None, _ptr(dd), _ptr(tt), M_, effect, kind, _ptr(mu),
                                            None, None, None, None, None, eng._stream())
        return rc, eng._err()

    def rows(r):
        return eng.dev(np.array(r, dtype=np.int32).reshape(-1, 2), dtype=torch.int32)

    P, I = PAIR_PROB, mn.INTERACTION
    per1 = per.copy()
    per1[1] = 1
    bad_l = [np.where(np.arange(6) == 2, v, l) for v in (0.0, -0.3, np.nan, np.inf)]
    bad_i0 = [np.where(np.arange(6) == 1, v, i0) for v in (0.0, -1.0, np.nan, np.inf)]
    cases = [(None, ax, d_dims, d_t, M, I, P), (md, None, d_dims, d_t, M, I, P), (md, ax, None, d_t, M, I, P),
             (md, ax, d_dims, None, M, I, P), (md, axes(xu=False), d_dims, d_t, M, I, P),
             (md, axes(null="h_l"), d_dims, d_t, M, I, P), (md, axes(null="h_periodic"), d_dims, d_t, M, I, P),
             (md, axes(null="h_I0"), d_dims, d_t, M, I, P),
             (md, axes(Dc=0), d_dims, d_t, M, I, P), (md, axes(Dc=65), d_dims, d_t, M, I, P), (md, axes(Dc=5), d_dims, d_t, M, I, P),
             (md, ax, d_dims, d_t, 0, I, P), (md, ax, d_dims, d_t, -5, I, P), (md, ax, d_dims, d_t, 2 ** 31, I, P),
             (md, ax, d_dims, d_t, M, I, 3), (md, ax, d_dims, d_t, M, I, -1), (md, ax, d_dims, d_t, M, 3, P),
             (md, ax, d_dims, d_t, M, -1, P), (md32, ax, d_dims, d_t, M, I, P), (bare, ax, d_dims, d_t, M, I, P),
             (eng._model(rq["post"], True), ax, d_dims, d_t, M, I, P), (eng._model(m52["post"], True), ax, d_dims, d_t, M, I, P)]
    cases += [(md, axes(l_=v), d_dims, d_t, M, I, P) for v in bad_l]
    cases += [(md, axes(per_=per1, i0_=v), d_dims, d_t, M, I, P) for v in bad_i0]
    cases += [(md, axes(i0_=v), d_dims, d_t, M, I, P) for v in bad_i0]          # ... on an SE axis too
    cases += [(md, axes(per_=np.where(np.arange(6) == 0, 2, per)), d_dims, d_t, M, I, P)]
    # rows of d_dims that break the rules, one bad row among good ones
    for r, eff in (([6, 1], mn.CENTRED), ([0, 6], mn.CENTRED), ([-2, -1], mn.CENTRED), ([0, -2], mn.CENTRED), ([3, 3], mn.CENTRED),
                   ([-1, 2], mn.CENTRED), ([-1, 2], mn.RAW), ([2, -1], I), ([-1, -1], I)):
        dd = dims.copy()
        dd[57] = r
        cases.append((md, ax, rows(dd), d_t, M, eff, P))
    for args in cases:
        rc, msg = call(*args)
        assert rc < 0 and msg.startswith("invalid argument"), (args[4:], rc, msg)
    assert np.all(host(mu) == -7.0)                     # nothing was written
    rc, msg = call(md, ax, rows(np.where(np.arange(M)[:, None] == 57, [[3, 3]], dims)), d_t, M, mn.CENTRED, P)
    assert "row 57" in msg
    # the mean alone needs no operator
    assert call(bare, ax, d_dims, d_t, M, I, PAIR_MEAN)[0] == 0
    assert np.array_equal(host(mu), host(before["mu"]))
    after = eng.predict_marginals(post, dims, t, effect=mn.INTERACTION)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(before[k]), host(after[k]))
    assert (before["best_idx"], before["best_val"]) == (after["best_idx"], after["best_val"])
    # Python: refused before anything reaches the device
    for bad in (rq, m52):
        with pytest.raises(ValueError, match="average_pred"):
            eng.predict_marginals(bad["post"], dims, t)
    for dd, eff in (([[6, 1]], "centred"), ([[3, 3]], "centred"), ([[-1, 2]], "raw"), ([[2, -1]], "interaction")):
        with pytest.raises(ValueError, match="predict_marginals"):
            eng.predict_marginals(post, dd, [[0.1, 0.2]], effect=eff)
    with pytest.raises(ValueError, match="unknown effect"):
        eng.predict_marginals(post, dims, t, effect="pure")
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError, match="posterior covariance unavailable"):
        gp.marginal_pred(dims, t)


# ---------------------------------------------------------------- 6. the drop-in surface
def test_layers_of_gp_model(eng):
    mod = _se(6, "node")
    gp = _stub_gp(eng, mod)
    g, mu, var, p = gp.main_effect(2)
    assert g.shape == mu.shape == var.shape == p.shape == (65,) and g[0] == 0.0 and g[-1] == 1.0
    m2 = gp.marginal_pred(np.full(65, 2), g)
    assert np.array_equal(mu, m2[0]) and np.array_equal(var, m2[1]) and np.array_equal(p, m2[2])
    e = _errors(mod, np.stack([np.full(65, 2), np.full(65, -1)], axis=1), np.stack([g, np.zeros(65)], axis=1), mn.CENTRED, mu, var, p)
    assert max(e) <= TOL
    g2, mu2, _, _ = gp.main_effect(2, [0.0, 1.0])                          # a two-point grid: two order-1 rows
    assert mu2.shape == (2,) and mu2[0] == mu[0] and mu2[1] == mu[-1]
    gd, ge = np.linspace(0.0, 1.0, 9), np.linspace(0.1, 0.9, 5)
    pure = gp.interaction_effect(4, 1, gd, ge)
    cent = gp.interaction_effect(4, 1, gd, ge, pure=False)
    assert all(a.shape == (9, 5) for a in pure + cent)
    cd, ce = gp.main_effect(4, gd)[1], gp.main_effect(1, ge)[1]
    scale = np.abs(mod["alpha"]).sum() * float(mod["th"][2]) ** 2
    assert np.abs(cent[0] - (cd[:, None] + ce[None, :] + pure[0])).max() <= 1e-10 * scale
    tr = gp.interaction_effect(1, 4, ge, gd)
    assert all(np.array_equal(a.T, b) for a, b in zip(tr, pure))           # the axes in the other order: the same bits
    imp = gp.effect_importance(T=9)
    assert imp["main_range"].shape == imp["main_argmax"].shape == imp["main_sd"].shape == (6,)
    assert imp["pairs"].shape == (15, 2) and imp["interaction_max"].shape == (15,)
    for d in range(6):
        _, m_d, v_d, _ = gp.main_effect(d, imp["grid"])
        assert imp["main_range"][d] == m_d.max() - m_d.min() and imp["main_argmax"][d] == imp["grid"][m_d.argmax()]
        assert imp["main_sd"][d] == np.sqrt(np.maximum(v_d, 0.0)).max()
    k = int(np.flatnonzero((imp["pairs"] == [1, 4]).all(axis=1))[0])
    assert imp["interaction_max"][k] == np.abs(gp.interaction_effect(1, 4, imp["grid"], imp["grid"])[0]).max()
    one = _stub_gp(eng, _se(1, "node")).effect_importance(T=5)
    assert one["main_range"].shape == (1,) and one["interaction_max"].shape == (0,)
