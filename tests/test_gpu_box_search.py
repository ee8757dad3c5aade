"""GPU: searches inside boxes (ppbo_mean_ascent_boxes, ppbo_mean_search_boxes, GPModel.mu_star_in / conditional_xstar /
profile_effect / profile_interaction) against today's unit-box search, the NumPy restatement tests/box_search_numpy.py,
and the properties a box promises.  Models are those of search_ref.mean_case, fitted as tests/test_gpu_search_stages.py
fits its own.

1. the unit box returns the bits of mean_ascent / mean_search_multi        5. trials are independent (T = 130, batches)
2. the boxed ascent, n = 0 .. 6, against bb_ascent_box                     6. the best candidate is never lost
3. the box holds; fixed coordinates; the box of one point                  7. refusals leave the outputs untouched
4. the start selection is exact on lattice inputs                          8. GPModel: profiles, conditional optima"""
import ctypes as C

import numpy as np
import pytest
import torch

import box_search_numpy as bx
import search_ref as sr

pytestmark = pytest.mark.gpu

NEG = -np.inf
DP = C.POINTER(C.c_double)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    from ppbo_amd.engine import get_engine
    return get_engine(0)


_MODELS = {}


def _model(eng, name):
    """dict(post, X, th, alpha, fg, starts, scale, D) of a search_ref.MEAN_CASES model; designs of 1024 rows are fitted on
    the device (the oracle's fit of 1024 unknowns takes over a minute)."""
    if name not in _MODELS:
        c = sr.MEAN_CASES[name]
        X, th, kernel, m = sr.mean_case(name)
        D = c["D"]
        if X.shape[0] > 256:
            r = eng.gp_fit(X, th, kernel, m, np.random.default_rng(D).standard_normal(X.shape[0]), gtol=1e-6, start_is_whitened=True)
            post = r["post"]
            assert post is not None
        else:
            f0, _ = sr.host_fit(X, th, kernel, m, D)
            post = eng.posterior(X, th, kernel, eng.pd_inverse(eng.gram(X, th, kernel)), f0, m)
        alpha = host(post.alpha)
        fg = sr.mean_fg(X, th, kernel, alpha)
        starts = sr.ascent_starts(D, 7, fg)
        mu0 = np.array([fg(np.clip(s, 0, 1))[0] for s in starts])
        _MODELS[name] = dict(post=post, X=X, th=th, alpha=alpha, fg=fg, starts=starts, scale=float(np.abs(mu0).max()), D=D)
    return _MODELS[name]


def _mean(eng, post, rows):
    return host(eng.predict(post, rows, want_var=False, want_best=False)["mu"])


def _unit(D, T=1):
    return np.tile(np.stack([np.zeros(D), np.ones(D)]), (T, 1, 1))


def _box_array(D, names=bx.BOX_NAMES):
    b = bx.boxes(D)
    return np.stack([np.stack(b[n]) for n in names])


# =============================================================== 1. the unit box is today's search
@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_unit_box_ascent_returns_the_bits_of_mean_ascent(eng, name):
    c = _model(eng, name)
    post, starts, D = c["post"], c["starts"], c["D"]
    K = starts.shape[0]
    for iters, tol in ((0, 1e-9), (sr.ASCENT_ITERS, 1e-9), (sr.ASCENT_ITERS, 1e-2), (100, 1e-9)):
        ref = eng.mean_ascent(post, starts, iters=iters, tol=tol)
        for per_box in (K, 1, 5):
            got = eng.mean_ascent_boxes(post, starts, _unit(D, -(-K // per_box)), per_box=per_box, iters=iters, tol=tol)
            for a, b, what in zip(ref, got, ("x", "mu", "it")):
                assert torch.equal(a, b), (name, iters, tol, per_box, what)


@pytest.mark.parametrize("fp32", [True, False])
@pytest.mark.parametrize("name", ["se_d3", "se_d20_tall", "ard_se_d5", "camphor_ard"])
def test_unit_box_search_returns_the_bits_of_mean_search_multi(eng, name, fp32):
    c = _model(eng, name)
    post, D = c["post"], c["D"]
    rng = np.random.default_rng(11 + D)
    T, M, K = 3, 3000, 16
    pool, shifts = rng.random((M, D)), rng.random((T, D))
    sep = 0.05 * np.sqrt(D)
    for iters in (0, 20):
        xm, mm = eng.mean_search_multi(post, pool, shifts, None, None, K=K, sep=sep, iters=iters, tol=1e-9, screen_fp32=fp32)
        xb, mb, cb = eng.mean_search_boxes(post, pool, _unit(D, T), shifts=shifts, K=K, sep=sep, iters=iters, tol=1e-9,
                                           screen_fp32=fp32)
        xm, mm, xb, mb, cb = host(xm), host(mm), host(xb), host(mb), host(cb)
        assert np.array_equal(mm, mb), (name, fp32, iters)
        found = np.isfinite(mm)
        assert np.array_equal(cb, found.sum(axis=1)) and np.all(cb >= 1)
        assert np.array_equal(xm[found], xb[found]), (name, fp32, iters)


# =============================================================== 2. the ascent against NumPy
@pytest.mark.parametrize("box,tol", bx.CONFIGS)
@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_boxed_ascent_steps(eng, name, box, tol):
    c = _model(eng, name)
    post, fg, starts, scale, D = c["post"], c["fg"], c["starts"], c["scale"], c["D"]
    lo, hi = bx.boxes(D)[box]
    s = bx.sensitivity_box(fg, starts, lo, hi, sr.ASCENT_ITERS, tol, scale)
    bound = sr.x_bound(s.dev)
    print(f"BOX {name} / {box} tol {tol:g}: flips {s.flips}, left out {s.left_out:.3f}, bound {bound.max():.1e}")
    assert s.flips == 0 and s.left_out <= 0.125 and bound.max() <= 1e-6, (s.flips, s.left_out, bound.max())
    worst = np.zeros(sr.ASCENT_ITERS + 1)
    boxes = np.stack([lo, hi])[None]
    for n in range(sr.ASCENT_ITERS + 1):
        x, mu, it = (host(t) for t in eng.mean_ascent_boxes(post, starts, boxes, per_box=len(starts), iters=n, tol=tol))
        keep = s.keep[:, n]
        if n == 0:
            assert np.array_equal(x, np.clip(starts, lo, hi)) and not np.array_equal(x, starts)
        assert np.array_equal(it[keep], s.its[keep, n]), (n, it, s.its[:, n])
        worst[n] = np.abs(x - s.xs[:, n])[keep].max()
        assert np.abs(mu - s.mus[:, n])[keep].max() <= 1e-9 * scale + 1e-14, n
    print(f"BOX {name} / {box} tol {tol:g}: |x_dev - x_ref| per n {np.array2string(worst, precision=1)}, bound "
          f"{np.array2string(bound, precision=1)}, it at n = {sr.ASCENT_ITERS}: "
          f"{np.bincount(s.its[:, -1], minlength=sr.ASCENT_ITERS + 1)}")
    assert np.all(worst <= bound), (worst, bound)


# =============================================================== 3. the box holds
@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_the_box_holds(eng, name):
    c = _model(eng, name)
    post, starts, scale, D = c["post"], c["starts"], c["scale"], c["D"]
    K = starts.shape[0]
    point = 0.1 + 0.8 * np.random.default_rng(D).random(D)
    boxes = np.concatenate([_box_array(D), np.stack([point, point])[None]])          # the five, then the box of one point
    B = boxes.shape[0]
    x, mu, it = (host(t) for t in eng.mean_ascent_boxes(post, np.tile(starts, (B, 1)), boxes, per_box=K, iters=100, tol=1e-9))
    x, mu, it = x.reshape(B, K, D), mu.reshape(B, K), it.reshape(B, K)
    for b in range(B):
        lo, hi = boxes[b]
        assert np.all((x[b] >= lo) & (x[b] <= hi)), b
        fixed = lo == hi
        assert np.array_equal(x[b][:, fixed], np.tile(lo[fixed], (K, 1))), b
        assert np.abs(_mean(eng, post, x[b]) - mu[b]).max() <= 1e-9 * scale + 1e-14, b        # mu IS the mean at x
    assert np.all(it[B - 1] == 0) and np.array_equal(x[B - 1], np.tile(point, (K, 1)))
    assert np.abs(mu[B - 1] - _mean(eng, post, point[None])[0]).max() <= 1e-9 * abs(_mean(eng, post, point[None])[0])
    # ... and with tol = 0, where nothing else would stop it
    _, _, it0 = eng.mean_ascent_boxes(post, starts[:3], boxes[B - 1:], per_box=3, iters=5, tol=0.0)
    assert np.all(host(it0) == 0)


@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_the_best_of_a_boxed_search_is_stationary_in_its_box(eng, name):
    """The criterion of test_gpu_mean_search.py (the winner of a search against the gradient scale of its raw candidates),
    with the gradient projected at the box's bounds: one search per test box, 100 iterations at tol = 1e-9.
    The criterion presumes that the iteration has stopped by itself.  Whether it does within 100 iterations is a property
    of the model, not of the box: the NumPy reference decides it.  Where bb_ascent_box from the winner's start uses up all
    100 iterations the criterion is asserted at 400, the budget of mu_star's re-ascent of a winner that is not stationary.
    That happens in camphor_ard only (length scales 0.3 .. 1.0; the reference needs 140 .. 300 iterations there and stands
    at a projected gradient of 9e-3 after 100, in the unit box, where the device is ppbo_mean_search_multi bit for bit:
    1.0e-2 measured against the allowed 2.2e-3)."""
    c = _model(eng, name)
    post, fg, scale, D = c["post"], c["fg"], c["scale"], c["D"]
    rng = np.random.default_rng(30 + D)
    boxes = _box_array(D)
    T, M, K = boxes.shape[0], 3000, 16
    pool, shifts = rng.random((M, D)), rng.random((T, D))
    run = {n: tuple(host(t) for t in eng.mean_search_boxes(post, pool, boxes, shifts=shifts, K=K, sep=0.05 * np.sqrt(D), iters=n,
                                                           tol=1e-9, screen_fp32=False)) for n in (0, 100, 400)}
    for t in range(T):
        lo, hi = boxes[t]
        fixed = lo == hi
        n = int(run[100][2][t])
        assert n >= 1 and n == run[0][2][t] == run[400][2][t]
        g_c = host(eng.mean_grad(post, bx.box_rows(pool, shifts[t], lo, hi))[1])
        for iters in (100, 400):
            x, mu = run[iters][0][t][:n], run[iters][1][t][:n]
            assert np.all((x >= lo) & (x <= hi)) and np.array_equal(x[:, fixed], np.tile(lo[fixed], (n, 1))), (t, iters)
            m_at, g_at = (host(a) for a in eng.mean_grad(post, x))
            assert np.abs(m_at - mu).max() <= 1e-9 * scale + 1e-14
            best = int(np.argmax(mu))
            pg = np.abs(bx.project_box(x[best], g_at[best], lo, hi)).max()
            if iters == 100:
                ref = bx.bb_ascent_box(fg, run[0][0][t][best], lo, hi, 100, 1e-9)
                if ref.it < 100:
                    assert pg <= 1e-3 * np.abs(g_c).max() + 1e-9, (t, pg, np.abs(g_c).max())
                else:
                    print(f"BOX {name} box {t}: the reference uses up 100 iterations from the winner's start; device "
                          f"|projected gradient| there {pg:.2e} (scale {np.abs(g_c).max():.2e}): asserted at 400")
                    assert name == "camphor_ard"
            elif ref.it >= 100:
                assert pg <= 1e-3 * np.abs(g_c).max() + 1e-9, (t, pg, np.abs(g_c).max())


# =============================================================== 4. selection is exact
@pytest.mark.parametrize("name,M", [("se_d3", 9000), ("se_d20_tall", 2000)])
def test_selection_is_exact_on_lattice_inputs(eng, name, M):
    c = _model(eng, name)
    post, D = c["post"], c["D"]
    rng = np.random.default_rng(M + D)
    T, S, K = 3, 2, 32
    assert sr.group_shape(M + S, D)[0] > 1                                # thinning groups by G > 1
    pool, shifts, seeds = sr.lattice(rng, M, D, 10), sr.lattice(rng, T, D, 10), sr.lattice(rng, T * S, D, 10).reshape(T, S, D)
    pool = np.where(pool == 1.0, 0.0, pool)
    ab = sr.lattice(rng, 2 * T, D, 4).reshape(T, 2, D)                    # multiples of 1 / 16: (hi - lo) u + lo is exact
    boxes = np.stack([ab.min(axis=1), ab.max(axis=1)], axis=1)
    boxes[1, :, 0] = 0.25                                                 # a fixed coordinate
    for sep in (0.1 * np.sqrt(D), 0.0):
        x, mu, cnt = (host(t) for t in eng.mean_search_boxes(post, pool, boxes, shifts=shifts, seeds=seeds, K=K, sep=sep, iters=0,
                                                             screen_fp32=False))
        for t in range(T):
            rows = bx.box_rows(pool, shifts[t], boxes[t, 0], boxes[t, 1], seeds[t])
            sc = _mean(eng, post, rows)
            ref = sr.select_starts(sc, rows, K, sep)
            assert cnt[t] == ref.count and 1 <= ref.count <= K, (t, cnt[t], ref.count)
            assert np.array_equal(x[t][:ref.count], rows[ref.idx]), (t, sep)
            assert np.abs(mu[t][:ref.count] - sc[ref.idx]).max() <= 1e-9 * np.abs(sc).max() + 1e-14
            assert np.all(mu[t][ref.count:] == NEG)
        if sep == 0.0:
            assert np.all(cnt == K)


# =============================================================== 5. trials are independent
def _mixed_boxes(D, T, rng):
    five = _box_array(D)
    out = np.empty((T, 2, D))
    for t in range(T):
        if t % 7 == 5:
            p = rng.random(D)
            out[t] = np.stack([p, p])                                     # a box of one point
        elif t % 7 == 6:
            a, b = rng.random(D), rng.random(D)
            out[t] = np.stack([np.minimum(a, b), np.maximum(a, b)])
        else:
            out[t] = five[t % 7 % 5]
    return out


@pytest.mark.parametrize("fp32", [True, False])
def test_trials_are_independent_of_batch_and_order(eng, fp32):
    c = _model(eng, "se_d3")
    post, D = c["post"], c["D"]
    rng = np.random.default_rng(130)
    T, M, K, S = 130, 600, 4, 2                                           # 64 + 64 + 2: two batch boundaries
    pool, shifts = rng.random((M, D)), rng.random((T, D))
    boxes = _mixed_boxes(D, T, rng)
    seeds = -0.2 + 1.4 * rng.random((T, S, D))                            # some outside their box: they enter clipped
    kw = dict(K=K, sep=0.05, iters=30, tol=1e-9, screen_fp32=fp32)
    x, mu, cnt = (host(t) for t in eng.mean_search_boxes(post, pool, boxes, shifts=shifts, seeds=seeds, **kw))
    found = np.isfinite(mu)
    assert np.array_equal(cnt, found.sum(axis=1)) and np.all(cnt >= 1) and len(set(cnt.tolist())) > 1
    xr, mr, cr = (host(t)[::-1] for t in eng.mean_search_boxes(post, pool, boxes[::-1], shifts=shifts[::-1], seeds=seeds[::-1], **kw))
    assert np.array_equal(mu, mr) and np.array_equal(cnt, cr) and np.array_equal(x[found], xr[found])
    singles = [eng.mean_search_boxes(post, pool, boxes[t:t + 1], shifts=shifts[t:t + 1], seeds=seeds[t:t + 1], **kw) for t in range(T)]
    x1, m1, c1 = (host(torch.cat([s[i] for s in singles])) for i in range(3))
    assert np.array_equal(mu, m1) and np.array_equal(cnt, c1) and np.array_equal(x[found], x1[found])
    for t in range(T):
        assert np.all((x[t][found[t]] >= boxes[t, 0]) & (x[t][found[t]] <= boxes[t, 1])), t


def test_a_seed_outside_its_box_enters_clipped(eng):
    c = _model(eng, "se_d3")
    post = c["post"]
    lo, hi = bx.boxes(3)["inner"]
    pool, seeds = np.array([[0.5, 0.5, 0.5]]), np.array([[[1.5, -0.3, 0.45]]])
    x, mu, cnt = (host(t) for t in eng.mean_search_boxes(post, pool, np.stack([lo, hi])[None], seeds=seeds, K=4, sep=0.0, iters=0,
                                                         screen_fp32=False))
    rows = bx.box_rows(pool, None, lo, hi, seeds[0])
    assert np.array_equal(rows[1], [0.7, 0.2, 0.45]) and cnt[0] == 2
    sc = _mean(eng, post, rows)
    assert np.array_equal(x[0][:2], rows[np.argsort(-sc, kind="stable")]) and np.all(mu[0][2:] == NEG)


# =============================================================== 6. the best candidate is never lost
@pytest.mark.parametrize("fp32", [True, False])
@pytest.mark.parametrize("name", ["se_d3", "se_d20_tall", "ard_se_d5", "camphor_ard"])
def test_the_best_candidate_is_never_lost(eng, name, fp32):
    c = _model(eng, name)
    post, D = c["post"], c["D"]
    rng = np.random.default_rng(60 + D)
    M, S, K = 3000, 2, 8
    boxes = _box_array(D)
    T = boxes.shape[0]
    pool, shifts, seeds = rng.random((M, D)), rng.random((T, D)), rng.random((T, S, D))
    x, mu, cnt = (host(t) for t in eng.mean_search_boxes(post, pool, boxes, shifts=shifts, seeds=seeds, K=K, sep=0.05 * np.sqrt(D),
                                                         iters=20, tol=1e-9, screen_fp32=fp32))
    for t in range(T):
        sc = _mean(eng, post, bx.box_rows(pool, shifts[t], boxes[t, 0], boxes[t, 1], seeds[t]))
        top = np.abs(sc).max()
        margin = 1e-5 * top if fp32 else 1e-12 * max(1.0, top)
        assert mu[t].max() >= sc.max() - margin, (t, mu[t].max(), sc.max())
        ok = np.isfinite(mu[t])
        assert np.abs(_mean(eng, post, x[t][ok]) - mu[t][ok]).max() <= 1e-9 * top + 1e-14


# =============================================================== 7. refusals
class _Raw:
    """The two entries called on raw pointers, with poisoned outputs."""

    def __init__(self, eng, post, D):
        self.e, self.post, self.D = eng, post, D
        self.T, self.K, self.M, self.S = 2, 4, 50, 1
        self.pool = eng.dev(np.full((self.M, D), 0.5))
        self.seeds = eng.dev(np.full((self.T, self.S, D), 0.5))
        self.starts = eng.dev(np.full((self.K, D), 0.5))
        self.reset()

    def reset(self):
        e, D = self.e, self.D
        self.x = torch.full((self.T, self.K, D), 7.0, dtype=torch.float64, device=e.device)
        self.mu = torch.full((self.T, self.K), 7.0, dtype=torch.float64, device=e.device)
        self.cnt = torch.full((self.T,), 7, dtype=torch.int32, device=e.device)
        self.its = torch.full((self.K,), 7, dtype=torch.int32, device=e.device)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.x == 7.0).all() and (self.mu == 7.0).all() and (self.cnt == 7).all() and (self.its == 7).all())

    def search(self, **o):
        from ppbo_amd.engine import _ptr
        e, D = self.e, self.D
        md = o.get("md", e._model(self.post, False))
        boxes = np.ascontiguousarray(o.get("boxes", _unit(D, self.T)))
        sh = np.zeros((4200, D))
        return e.lib.ppbo_mean_search_boxes(
            e.ctx, None if o.get("no_model") else C.byref(md), None if o.get("no_pool") else _ptr(self.pool), o.get("M", self.M),
            sh.ctypes.data_as(DP), None if o.get("no_boxes") else boxes.ctypes.data_as(DP), o.get("T", self.T),
            None if o.get("no_seeds") else _ptr(self.seeds), o.get("S", self.S), o.get("K", self.K), o.get("sep", 0.05),
            o.get("iters", 5), o.get("tol", 1e-9), o.get("fp32", 1), None if o.get("no_x") else _ptr(self.x),
            None if o.get("no_mu") else _ptr(self.mu), _ptr(self.cnt), e._stream())

    def ascent(self, **o):
        from ppbo_amd.engine import _ptr
        e, D = self.e, self.D
        md = o.get("md", e._model(self.post, False))
        boxes = np.ascontiguousarray(o.get("boxes", _unit(D, 1)))
        return e.lib.ppbo_mean_ascent_boxes(
            e.ctx, None if o.get("no_model") else C.byref(md), None if o.get("no_starts") else _ptr(self.starts), o.get("K", self.K),
            None if o.get("no_boxes") else boxes.ctypes.data_as(DP), o.get("B", 1), o.get("per_box", self.K), o.get("iters", 5),
            o.get("tol", 1e-9), None if o.get("no_x") else _ptr(self.x), None if o.get("no_mu") else _ptr(self.mu), _ptr(self.its),
            e._stream())


def _bad_boxes(D, T):
    out = {}
    for label, (i, v) in {"lo > hi": (0, 0.6), "lo < 0": (0, -1e-9), "hi > 1": (1, 1.0 + 1e-9), "lo nan": (0, np.nan),
                          "hi inf": (1, np.inf), "lo -inf": (0, -np.inf)}.items():
        b = _unit(D, T)
        b[T - 1, :, D - 1] = (0.2, 0.5)
        b[T - 1, i, D - 1] = v
        out[label] = b
    return out


def test_refusals_leave_the_outputs_untouched(eng):
    c = _model(eng, "se_d3")
    post, D = c["post"], c["D"]
    raw = _Raw(eng, post, D)

    def model(**f):
        md = eng._model(post, False)
        for k, v in f.items():
            setattr(md, k, v)
        return md
    search = [("model", dict(no_model=True)), ("pool", dict(no_pool=True)), ("boxes", dict(no_boxes=True)), ("x", dict(no_x=True)),
              ("mu", dict(no_mu=True)), ("S without seeds", dict(no_seeds=True)), ("T = 0", dict(T=0)), ("T = 4097", dict(T=4097)),
              ("K = 0", dict(K=0)), ("K = 1025", dict(K=1025)), ("S = 65", dict(S=65)), ("S = -1", dict(S=-1)), ("M = 0", dict(M=0)),
              ("64 (M + S) = 2^31", dict(M=(1 << 25) - 1)), ("sep < 0", dict(sep=-1e-3)), ("iters < 0", dict(iters=-1)),
              ("tol < 0", dict(tol=-1e-9)), ("N = 0", dict(md=model(N=0))), ("D = 65", dict(md=model(D=65))),
              ("kernel id", dict(md=model(kernel_id=99))), ("alpha", dict(md=model(d_alpha=None)))]
    search += [("box " + k, dict(boxes=b)) for k, b in _bad_boxes(D, raw.T).items()]
    # T K = 65537 > 65536 with T and K inside their own limits
    search.append(("T K", dict(T=4096, K=17, boxes=_unit(D, 4096))))
    ascent = [("model", dict(no_model=True)), ("starts", dict(no_starts=True)), ("boxes", dict(no_boxes=True)), ("x", dict(no_x=True)),
              ("mu", dict(no_mu=True)), ("K = 0", dict(K=0)), ("B != ceil", dict(B=2, boxes=_unit(D, 2))),
              ("B != ceil (per_box 3)", dict(B=1, per_box=3)), ("per_box = 0", dict(per_box=0)), ("iters < 0", dict(iters=-1)),
              ("tol < 0", dict(tol=-1.0)), ("N = 0", dict(md=model(N=0))), ("kernel id", dict(md=model(kernel_id=99)))]
    ascent += [("box " + k, dict(boxes=b)) for k, b in _bad_boxes(D, 1).items()]
    for entry, cases in ((raw.search, search), (raw.ascent, ascent)):
        for label, o in cases:
            rc = entry(**o)
            assert rc != 0 and "invalid argument" in eng._err(), (entry.__name__, label, rc, eng._err())
            assert raw.untouched(), (entry.__name__, label)
    # the same arguments without the fault run
    assert raw.search() == 0 and not raw.untouched()
    raw.reset()
    assert raw.ascent() == 0 and not raw.untouched()
    with pytest.raises(ValueError):
        eng.mean_search_boxes(post, np.full((10, D + 1), 0.5), _unit(D + 1, 1))
    with pytest.raises(ValueError):
        eng.mean_search_boxes(post, np.full((10, D), 0.5), _unit(D, 2), shifts=np.zeros((3, D)))
    with pytest.raises(ValueError):
        eng.mean_ascent_boxes(post, np.full((4, D + 1), 0.5), _unit(D + 1, 4))


# =============================================================== 8. GPModel
@pytest.fixture(scope="module", params=["c2", "cam_small"])
def fitted(request, golden):
    from test_gpu_golden_r2 import _fitted
    g, gp, st = _fitted(golden, request.param)
    np.random.seed(8)
    gp.xstar, gp.mustar, gp.xstars_local = gp.mu_star(mustar_finding_trials=3)
    return gp


def test_profile_effect(fitted):
    gp = fitted
    D, xs, ms = gp.D, np.asarray(gp.xstar), float(gp.mustar)
    for d in (0, D - 1):
        grid = np.sort(np.r_[np.linspace(0.0, 1.0, 9), xs[d]])
        p = gp.profile_effect(d, grid)
        assert np.array_equal(p["t"], grid) and p["x"].shape == (grid.size, D) and np.array_equal(p["x"][:, d], grid)
        assert np.all((p["x"] >= 0) & (p["x"] <= 1))
        mu_at = gp.mu_pred_batch(p["x"])
        assert np.abs(mu_at - p["mu"]).max() <= 1e-9 * max(1.0, np.abs(mu_at).max())
        var_ref = np.array([gp.mu_Sigma_pred(x[None])[1][0, 0] for x in p["x"]])
        assert np.abs(p["var"] - var_ref).max() <= 1e-6 * max(1.0, np.abs(var_ref).max())
        sl = np.tile(xs, (grid.size, 1))
        sl[:, d] = grid
        assert np.all(p["mu"] >= gp.mu_pred_batch(sl) - 1e-5 * abs(ms))                 # never below the slice through x*
        k = int(np.flatnonzero(grid == xs[d])[0])
        assert p["mu"][k] >= ms - 1e-9 * abs(ms)
    assert gp.profile_effect(0)["t"].size == 65


def test_conditional_xstar_and_mu_star_in(fitted):
    gp = fitted
    D, xs, ms = gp.D, np.asarray(gp.xstar), float(gp.mustar)
    np.random.seed(9)
    x, mu, loc = gp.conditional_xstar({})
    assert mu >= ms - 1e-6 * abs(ms) and x.shape == (D,) and loc.shape[1] == D and np.array_equal(loc[0], x)
    x, mu, _ = gp.conditional_xstar({1: 0.4})
    assert x[1] == 0.4 and abs(gp.mu_pred(x) - mu) <= 1e-9 * max(1.0, abs(mu)) and mu <= ms + 1e-6 * abs(ms)
    lower, upper = np.clip(xs - 0.1, 0, 1), np.clip(xs + 0.1, 0, 1)
    x, mu, loc = gp.mu_star_in(lower=lower, upper=upper)
    assert np.all((x >= lower) & (x <= upper)) and np.all((loc >= lower) & (loc <= upper))
    assert mu >= ms - 1e-9 * abs(ms)                                                     # x* itself is a seed
    lo2, hi2 = np.full(D, 0.55), np.full(D, 0.8)
    x, mu, loc = gp.mu_star_in(lower=lo2, upper=hi2, fixed={0: 0.6}, trials=2)
    assert np.all((x[1:] >= 0.55) & (x[1:] <= 0.8)) and x[0] == 0.6 and np.all(loc[:, 0] == 0.6)
    with pytest.raises(ValueError):
        gp.mu_star_in(lower=np.full(D, 0.6), upper=np.full(D, 0.4))
    with pytest.raises(ValueError):
        gp.conditional_xstar({D: 0.5})


def test_profile_interaction(fitted):
    gp = fitted
    D = gp.D
    gd, ge = np.linspace(0.0, 1.0, 5), np.array([0.25, 0.5, 0.75])
    p = gp.profile_interaction(0, 2, gd, ge)
    assert p["mu"].shape == (5, 3) and p["x"].shape == (5, 3, D) and p["var"].shape == (5, 3)
    assert np.array_equal(p["x"][:, :, 0], np.tile(gd[:, None], (1, 3))) and np.array_equal(p["x"][:, :, 2], np.tile(ge[None, :], (5, 1)))
    mu_at = gp.mu_pred_batch(p["x"].reshape(-1, D)).reshape(5, 3)
    assert np.abs(mu_at - p["mu"]).max() <= 1e-9 * max(1.0, np.abs(mu_at).max())
    # max over x_2 of the two-dimensional profile on a row is the one-dimensional profile there, wherever x_2's maximiser
    # of the latter lies on the grid: put it there
    one = gp.profile_effect(0, gd)
    row = 2
    p2 = gp.profile_interaction(0, 2, gd[row:row + 1], np.array([one["x"][row, 2]]))
    assert abs(p2["mu"][0, 0] - one["mu"][row]) <= 1e-6 * max(1.0, abs(one["mu"][row]))
    with pytest.raises(ValueError):
        gp.profile_interaction(1, 1)
