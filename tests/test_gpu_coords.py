"""GPU: a model's coordinate map (ppbo_coords, include/ppbo_hip.h) -- what every entry that reads it refuses, and that the
map is data of the call: nothing of it stays in the ctx.

Shapes: n_q = 4, m = 3 (N = 16); D = 3 for the radial models, 6 -> 11 for camphor; a pool of 256 rows, T = 2, K = 4,
iters = 10; F = 32, S = 2.  The models are mean-only posteriors over a seeded alpha (no fit is needed: every entry here
reads X, alpha and theta only)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAM = "camphor_copper_ard_kernel"
N, M_ROWS, D3, POOL, T, K, ITERS, F, S = 16, 3, 3, 256, 2, 4, 10, 32, 2
ARD_L = np.array([0.3, 0.6, 1.1])
CAM_L = np.array([0.3, 0.4, 0.5, 0.6, 0.8, 1.0])
THETA = {"id": [0.1, 0.5, 0.7], "ard": [0.1, ARD_L, 0.7], "cam": [0.1, CAM_L, 0.7]}
KERNEL = {"id": "SE_kernel", "ard": "SE_kernel", "cam": CAM}
SENTINEL = 7.0


def host(t):
    return t.detach().cpu().numpy()


def _data():
    """Every input of the file, seeded: per model the design, alpha, pool, shifts, xprev, points and starts; the RFF bases."""
    rng = np.random.default_rng(1606)
    d = {}
    for which, D in (("id", D3), ("ard", D3), ("cam", 6)):
        d[which] = dict(X=rng.random((N, D)), alpha=rng.standard_normal(N), pool=rng.random((POOL, D)),
                        shifts=rng.random((T, D)), xprev=rng.random(D), pts=rng.random((5, D)), starts=rng.random((K, D)))
    d["rff"] = dict(cand=rng.random((POOL, D3)), W=rng.standard_normal((F, D3)) / 0.5, b=rng.uniform(0, 2 * np.pi, F),
                    om=rng.standard_normal(F), oms=rng.standard_normal((S, F)))
    d["rff_cam"] = dict(cand=rng.random((POOL, 6)), W=rng.standard_normal((F, 11)), b=rng.uniform(0, 2 * np.pi, F),
                        om=rng.standard_normal(F), oms=rng.standard_normal((S, F)))
    d["path"] = dict(cand=rng.random((POOL, D3)), W=rng.standard_normal((F, D3)) / 0.5, b=rng.uniform(0, 2 * np.pi, F),
                     X=rng.random((N, D3)), Wp=rng.standard_normal((S, F)), V=rng.standard_normal((S, N)))
    return d


DATA = _data()


def _post(eng, which):
    d = DATA[which]
    return eng.mean_posterior(d["X"], THETA[which], KERNEL[which], M_ROWS, eng.dev(d["alpha"]))


# ---- the calls of test 2, through the Engine's public surface only: {name: array}
def mean_calls(eng, which):
    d, post = DATA[which], _post(eng, which)
    out = {}
    mu, g = eng.mean_grad(post, d["pts"])
    out["grad.mu"], out["grad.g"] = host(mu), host(g)
    x, mu, it = eng.mean_ascent(post, d["starts"], iters=ITERS, tol=1e-9)
    out["ascent.x"], out["ascent.mu"], out["ascent.it"] = host(x), host(mu), host(it)
    for fp32 in (0, 1):
        x, mu = eng.mean_search_multi(post, d["pool"], d["shifts"], extra="design", xprev=d["xprev"], K=K, sep=0.05,
                                      iters=ITERS, tol=1e-9, screen_fp32=bool(fp32))
        out[f"multi{fp32}.x"], out[f"multi{fp32}.mu"] = host(x), host(mu)
    return out


def rff_calls(eng, which):
    d = DATA[which]
    kw = dict(K=K, sep=0.05, iters=ITERS, tol=1e-10)
    if which == "rff":
        one = eng.rff_search(d["cand"], d["W"], d["b"], 0.7, d["om"], **kw)
        many = eng.rff_search_multi(d["cand"], d["W"], d["b"], 0.7, d["oms"], **kw)
    else:
        one = eng.rff_search_camphor(d["cand"], CAM_L, d["W"], d["b"], 0.7, d["om"], **kw)
        many = eng.rff_search_multi_camphor(d["cand"], CAM_L, d["W"], d["b"], 0.7, d["oms"], **kw)
    return dict(zip(("one.x", "one.v", "many.x", "many.v", "many.found"), one + many))


def path_calls(eng, which):
    d = DATA["path"]
    r = eng.path_search_multi(d["cand"], d["W"], d["b"], THETA[which], "SE_kernel", d["X"], d["Wp"], d["V"], K=K, sep=0.05,
                              iters=ITERS, tol=1e-10)
    return dict(zip(("x", "v", "found"), r))


# what one engine runs, in this order, and the fresh engines it is held against (one per distinct (calls, which))
SEQUENCE = [(mean_calls, "id"), (mean_calls, "ard"), (mean_calls, "cam"), (mean_calls, "id"),
            (rff_calls, "rff"), (rff_calls, "rff_cam"), (rff_calls, "rff"), (rff_calls, "rff_cam"),
            (path_calls, "id"), (path_calls, "ard"), (path_calls, "id"), (path_calls, "ard")]


def sequence_against_fresh_engines(make_engine):
    """[(step, name, equal)] of SEQUENCE on one engine against the same calls on engines that have seen nothing else."""
    fresh = {}
    for fn, which in SEQUENCE:
        if (fn, which) not in fresh:
            e = make_engine()
            fresh[(fn, which)] = fn(e, which)
            torch.cuda.synchronize()
            e.close()
    eng = make_engine()
    rows = []
    for step, (fn, which) in enumerate(SEQUENCE):
        got = fn(eng, which)
        for name, ref in fresh[(fn, which)].items():
            rows.append((f"{step}:{fn.__name__}:{which}", name, np.array_equal(got[name], ref, equal_nan=True) and
                         np.asarray(got[name]).size > 0))
    eng.close()
    return rows


@pytest.fixture(scope="module")
def eng():
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def test_the_map_is_data_of_the_call_not_state_of_the_ctx():
    """One engine serves an identity, an ARD and a camphor model in turn (and the identity model again), the plain and the
    camphor RFF search alternating, the scalar and the ARD path search alternating: every array equals, bit for bit, the
    same call on a fresh engine that has seen only that model.  (Two engines repeat bit for bit on the commit before the
    map became data, too -- measured with this very function, profiles/r16_coordinate_map.txt -- so this asserts what
    held there.)"""
    from ppbo_amd.engine import Engine
    rows = sequence_against_fresh_engines(lambda: Engine(0))
    assert len(rows) == 4 * 9 + 4 * 5 + 4 * 3
    assert not [r for r in rows if not r[2]], [r[:2] for r in rows if not r[2]]


def test_zero_filled_coords_are_the_identity(eng):
    """A zero-filled ppbo_coords on a scalar model, and kind 0 with coefficients that would be refused (they are not
    read), through eng.lib against the Engine's own call."""
    from ppbo_amd import _lib
    from ppbo_amd.engine import _ptr
    d, post = DATA["id"], _post(eng, "id")
    ref_x, ref_mu, ref_it = (host(t) for t in eng.mean_ascent(post, d["starts"], iters=ITERS, tol=1e-9))
    bad = np.array([-1.0, np.nan, 0.0])
    for co in (_lib.Coords(), _lib.coords(_lib.COORDS_MODEL, bad, 12345)):
        md = eng._model(post, False)
        md.coords = co
        starts = eng.dev(d["starts"])
        xs, mus = eng.empty(K, D3), eng.empty(K)
        its = torch.zeros(K, dtype=torch.int32, device=eng.device)
        rc = eng.lib.ppbo_mean_ascent(eng.ctx, C.byref(md), _ptr(starts), K, ITERS, 1e-9, _ptr(xs), _ptr(mus), _ptr(its),
                                      eng._stream())
        eng._check(rc, "ppbo_mean_ascent")
        assert np.array_equal(host(xs), ref_x) and np.array_equal(host(mus), ref_mu) and np.array_equal(host(its), ref_it)
    r = DATA["rff"]
    ref = eng.rff_search_multi(r["cand"], r["W"], r["b"], 0.7, r["oms"], K=K, sep=0.05, iters=ITERS, tol=1e-10)
    cand, W, b, oms = eng.dev(r["cand"]), eng.dev(r["W"]), eng.dev(r["b"]), eng.dev(r["oms"])
    for co in (_lib.Coords(), _lib.coords(_lib.COORDS_MODEL, bad)):
        xs, vals = eng.empty(S, K, D3), eng.empty(S, K)
        fnd = torch.zeros(S, dtype=torch.int32, device=eng.device)
        rc = eng.lib.ppbo_rff_search_multi(eng.ctx, _ptr(cand), POOL, D3, _ptr(W), F, _ptr(b), 0.7, _ptr(oms), co, S, K, 0.05,
                                           ITERS, 1e-10, _ptr(xs), _ptr(vals), _ptr(fnd), eng._stream())
        eng._check(rc, "ppbo_rff_search_multi")
        assert all(np.array_equal(host(a), b_) for a, b_ in zip((xs, vals, fnd), ref))


# ---------------------------------------------------------------- refusals
class _Entries:
    """Every entry that reads a map, over buffers pre-filled with SENTINEL: call(md or coords) -> rc; unchanged() says
    whether a refusal left the outputs alone."""

    def __init__(self, eng):
        self.eng = eng
        self.f = {}      # float outputs by name
        self.i = {}      # int outputs
        self.found = C.c_int(-7)
        self.keep = []

    def out(self, name, *shape):
        self.f[name] = torch.full(shape, SENTINEL, dtype=torch.float64, device=self.eng.device)
        return C.c_void_p(self.f[name].data_ptr())

    def iout(self, name, n):
        self.i[name] = torch.full((n,), -7, dtype=torch.int32, device=self.eng.device)
        return C.c_void_p(self.i[name].data_ptr())

    def unchanged(self):
        return (all(bool((t == SENTINEL).all()) for t in self.f.values()) and
                all(bool((t == -7).all()) for t in self.i.values()) and self.found.value == -7)

    def dev(self, a):
        t = self.eng.dev(a)
        self.keep.append(t)
        return C.c_void_p(t.data_ptr())

    # the model entries: md is a _lib.Model; D is the width of the caller's points
    def mean_grad(self, md, D):
        e = self.eng
        return e.lib.ppbo_mean_grad(e.ctx, C.byref(md), self.dev(np.full((5, D), 0.5)), 5, self.out("g.mu", 5),
                                    self.out("g.g", 5, D), e._stream())

    def mean_ascent(self, md, D):
        e = self.eng
        return e.lib.ppbo_mean_ascent(e.ctx, C.byref(md), self.dev(np.full((K, D), 0.5)), K, ITERS, 1e-9, self.out("a.x", K, D),
                                      self.out("a.mu", K), self.iout("a.it", K), e._stream())

    def mean_search_multi(self, md, D, fp32=1):
        e = self.eng
        sh, xp = np.full((T, D), 0.25), np.full(D, 0.5)
        dp = C.POINTER(C.c_double)
        return e.lib.ppbo_mean_search_multi(e.ctx, C.byref(md), self.dev(np.full((POOL, D), 0.5)), POOL, sh.ctypes.data_as(dp), T,
                                            None, md.N, xp.ctypes.data_as(dp), K, 0.05, ITERS, 1e-9, fp32,
                                            self.out("m.x", T, K, D), self.out("m.mu", T, K), e._stream())

    def mean_search(self, md, D):
        e = self.eng
        return e.lib.ppbo_mean_search(e.ctx, C.byref(md), self.dev(np.full((POOL, D), 0.5)), POOL, K, 0.05, ITERS, 1e-9,
                                      self.out("s.x", K, D), self.out("s.mu", K), C.byref(self.found), e._stream())

    # the entries without a model: co is a _lib.Coords or None
    def rff_search(self, co, D, Dw):
        e, r = self.eng, DATA["rff"]
        return e.lib.ppbo_rff_search(e.ctx, self.dev(np.full((POOL, D), 0.5)), POOL, D, self.dev(np.ones((F, Dw))), F,
                                     self.dev(r["b"]), 0.7, self.dev(r["om"]), co, K, 0.05, ITERS, 1e-10, self.out("r.x", K, D),
                                     self.out("r.v", K), C.byref(self.found), e._stream())

    def rff_search_multi(self, co, D, Dw):
        e, r = self.eng, DATA["rff"]
        return e.lib.ppbo_rff_search_multi(e.ctx, self.dev(np.full((POOL, D), 0.5)), POOL, D, self.dev(np.ones((F, Dw))), F,
                                           self.dev(r["b"]), 0.7, self.dev(r["oms"]), co, S, K, 0.05, ITERS, 1e-10,
                                           self.out("rm.x", S, K, D), self.out("rm.v", S, K), self.iout("rm.f", S), e._stream())

    def path_search_multi(self, co, kid=0):
        e, p = self.eng, DATA["path"]
        th = (C.c_double * 3)(0.1, 1.0, 0.7)
        return e.lib.ppbo_path_search_multi(e.ctx, kid, th, self.dev(p["cand"]), POOL, D3, self.dev(p["W"]), F, self.dev(p["b"]),
                                            self.dev(p["Wp"]), self.dev(p["X"]), N, self.dev(p["V"]), co, S, K, 0.05, ITERS,
                                            1e-10, self.out("p.x", S, K, D3), self.out("p.v", S, K), self.iout("p.f", S),
                                            e._stream())


def test_every_entry_refuses_a_bad_map_and_launches_nothing(eng):
    """Section "Validation" of the map: a kind outside 0..2, SCALED with the camphor kernel id, CAMPHOR on a model that
    is not SE at D = 11 (or without d_Xc), a NULL, non-positive or non-finite coefficient -- on every entry that reads a
    map; ppbo_mean_search with any map, the RFF searches with SCALED, the path search with CAMPHOR.  Each is rc < 0 with
    "invalid argument", and the outputs keep their sentinel."""
    from ppbo_amd import _lib
    MODEL, SCALED, CAMPHOR = _lib.COORDS_MODEL, _lib.COORDS_SCALED, _lib.COORDS_CAMPHOR
    posts = {w: _post(eng, w) for w in ("id", "ard", "cam")}
    ref_cam = eng.mean_posterior(DATA["cam"]["X"], [0.1, 1.0, 0.7], "camphor_copper_kernel", M_ROWS, eng.dev(DATA["cam"]["alpha"]))
    xc = posts["cam"].Xc.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad3 = [None, [0.3, -1.0, 1.0], [0.3, 0.0, 1.0], [0.3, nan, 1.0], [inf, 0.5, 1.0]]
    bad6 = [None, [0.3, 0.4, -0.5, 0.6, 0.8, 1.0], [0.3, 0.4, 0.5, 0.6, 0.8, 0.0], [0.3, nan, 0.5, 0.6, 0.8, 1.0],
            [0.3, 0.4, 0.5, inf, 0.8, 1.0]]

    def model(which, kind, coef, d_Xc=None, **fields):
        md = eng._model(ref_cam if which == "ref_cam" else posts[which], False)
        md._coords = _lib.coords(kind, coef, d_Xc)
        md.coords = md._coords
        for k, v in fields.items():
            setattr(md, k, v)
        return md

    cases = []        # (what, entry, args)
    model_entries = ("mean_grad", "mean_ascent", "mean_search_multi")
    for name in model_entries:
        for kind in (3, -1):
            cases.append((f"{name} kind {kind}", name, (model("ard", kind, 1.0 / ARD_L), D3)))
        cases.append((f"{name} SCALED + camphor id", name, (model("ref_cam", SCALED, np.ones(6)), 6)))
        cases.append((f"{name} CAMPHOR on SE D = 3", name, (model("id", CAMPHOR, CAM_L, xc), 6)))
        cases.append((f"{name} CAMPHOR on RQ D = 11", name, (model("cam", CAMPHOR, CAM_L, xc, kernel_id=1), 6)))
        cases.append((f"{name} CAMPHOR without d_Xc", name, (model("cam", CAMPHOR, CAM_L, None), 6)))
        for c in bad3:
            cases.append((f"{name} SCALED coef {c}", name, (model("ard", SCALED, c), D3)))
        for c in bad6:
            cases.append((f"{name} CAMPHOR coef {c}", name, (model("cam", CAMPHOR, c, xc), 6)))
    cases.append(("mean_search_multi fp64 SCALED coef", "mean_search_multi", (model("ard", SCALED, bad3[1]), D3, 0)))
    cases.append(("mean_search SCALED", "mean_search", (model("ard", SCALED, 1.0 / ARD_L), D3)))
    cases.append(("mean_search CAMPHOR", "mean_search", (model("cam", CAMPHOR, CAM_L, xc), 6)))
    for name in ("rff_search", "rff_search_multi"):
        for kind in (3, -1):
            cases.append((f"{name} kind {kind}", name, (_lib.coords(kind, CAM_L), 6, 11)))
        cases.append((f"{name} SCALED", name, (_lib.coords(SCALED, np.ones(D3)), D3, D3)))
        cases.append((f"{name} CAMPHOR at D = 3", name, (_lib.coords(CAMPHOR, CAM_L), D3, 11)))
        for c in bad6:
            cases.append((f"{name} CAMPHOR coef {c}", name, (_lib.coords(CAMPHOR, c), 6, 11)))
    for kind in (3, -1):
        cases.append((f"path kind {kind}", "path_search_multi", (_lib.coords(kind, 1.0 / ARD_L),)))
    cases.append(("path CAMPHOR", "path_search_multi", (_lib.coords(CAMPHOR, CAM_L),)))
    cases.append(("path SCALED + camphor id", "path_search_multi", (_lib.coords(SCALED, 1.0 / ARD_L), 2)))
    for c in bad3:
        cases.append((f"path SCALED coef {c}", "path_search_multi", (_lib.coords(SCALED, c),)))

    for what, name, args in cases:
        en = _Entries(eng)
        rc = getattr(en, name)(*args)
        assert rc < 0, (what, rc)
        assert "invalid argument" in eng._err(), (what, eng._err())
        torch.cuda.synchronize()
        assert en.unchanged(), what
    # the same callers with a good map: accepted, and the outputs are written (the sentinel checks above can fail)
    good = [("mean_grad", (model("ard", SCALED, 1.0 / ARD_L), D3)), ("mean_ascent", (model("cam", CAMPHOR, CAM_L, xc), 6)),
            ("mean_search_multi", (model("cam", CAMPHOR, CAM_L, xc), 6)), ("mean_search", (model("id", MODEL, None), D3)),
            ("rff_search", (_lib.coords(CAMPHOR, CAM_L), 6, 11)), ("rff_search_multi", (None, D3, D3)),
            ("path_search_multi", (_lib.coords(SCALED, 1.0 / ARD_L),))]
    for name, args in good:
        en = _Entries(eng)
        assert getattr(en, name)(*args) == 0, (name, eng._err())
        torch.cuda.synchronize()
        assert not en.unchanged(), name
