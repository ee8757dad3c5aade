"""GPU: acquisition gradients and their ascent -- ppbo_acq_grad / ppbo_acq_ascent, Engine.acq_grad / acq_ascent,
GPModel.acquisition_grad / maximize_acquisition against the NumPy statement (tests/acq_numpy.py: analytic kernel
derivatives on direct differences, the oracle's dense variance operator; itself checked by central differences in
tests/test_acq_host.py), against ppbo_mean_grad and ppbo_predict, the bit rules of the two entries, the ascent's
identities, the iteration step by step against tests/box_search_numpy.bb_ascent_box, and the refusals.

Bound (TOL = 1e-6, the package's parity standard), per component, each quantity against the sum of absolute terms it
cancels down from: mu against sum_j |k_j alpha_j|, var against sf^2, grad mu_d against sum_j |J_jd alpha_j|, grad var_d
against 2 sum_j |J_jd| |u_j| (u the reference's), the score and its gradient against the two sums weighted by
|d score / d mu| and |d score / d var|.

Measured on MI355X (the worst component over the 32 parity models and the three score kinds; profiles/r28_acq_ascent.txt
has them per quantity): mu 1.2e-10 (camphor on cam_small), var 4.3e-9 and score 4.3e-9 (SE, D = 20, N = 78), grad mu
2.5e-10 (camphor), grad var and grad score 9.8e-8 (RQ, D = 20, N = 78; the SE models 6.6e-9); the ladder's rungs at both
edges at most 1.5e-8 (D = 1, grad var).  grad mu and mu against ppbo_mean_grad: 0 (the same bits) in all six cases; mu, var
and score against ppbo_predict's at most 2.5e-15.  The ascent's iterates against the NumPy replay on the device's own
acq_grad: at most 2.8e-14 for n = 0 .. 6 against a bound of 1e-10 .. 2.4e-10, `it` equal, at most 0.071 of the pairs left
out (SE, D = 20, variance, unit box) and none flipped."""
import ctypes as C

import numpy as np
import pytest

import acq_numpy as aq
import box_search_numpy as bsn
import search_ref as sr
from test_gpu_slopes import RADIAL, TOL, _fitted, _fitted_camphor, _fitted_camphor_ard, _stub_gp, eng, host  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = {"mean": aq.MEAN, "EI": aq.EI, "variance": aq.VARIANCE}
SHAPES = [(6, 8, 3), (20, 3, 25), (40, 8, 3)]
LADDER = (8, 24, 64)               # the rungs of acq_grad_kernel (csrc/acq.hip: launch_acq_grad)


def _same(a, b):
    """Bitwise equality (NaN equals the same NaN) of two device tensors, arrays or scalars."""
    a, b = (np.ascontiguousarray(v if isinstance(v, (np.ndarray, np.generic)) else host(v)) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _points(mod, M, seed=3):
    """M points of the unit box: the first six ON design rows, the next six on faces of the box."""
    rng = np.random.default_rng(seed)
    N, D = mod["X"].shape
    X = rng.random((M, D))
    X[:6] = mod["X"][rng.integers(0, N, 6)]
    for r in range(6, 12):
        X[r, rng.integers(0, D)] = float(r % 2)
    return X


def _mustar(mod):
    return aq.best_design_mean(mod["X"], mod["th"], mod["kernel"], mod["alpha"])


def _errors(mod, X, out, kind, mustar):
    """The worst component of each output against its bound's scale, and the row it sits in."""
    ref = aq.acq_reference(X, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"], kind, mustar)
    sf2 = float(mod["th"][2]) ** 2
    a, b = (np.abs(w) for w in aq.score_weights(ref["mu"], ref["var"], kind, mustar))
    scale = dict(mu=ref["abs_mu"], var=np.full(len(X), sf2), score=a * ref["abs_mu"] + b * sf2, grad_mu=ref["abs_gmu"],
                 grad_var=ref["abs_gvar"], grad_score=a[:, None] * ref["abs_gmu"] + b[:, None] * ref["abs_gvar"])
    err, row = {}, {}
    for k, s in scale.items():
        if out.get(k) is None:
            continue
        v = host(out[k])
        assert np.all(np.isfinite(v)), k
        e = np.abs(v - ref[k]) / np.where(s > 0.0, s, 1.0)       # (a zero weight pair: EI's gradient where EI is flat)
        e = e.reshape(len(X), -1).max(axis=1)
        err[k], row[k] = float(e.max()), int(e.argmax())
    return err, row


def _parity(eng, mod, label, M=37):
    X = _points(mod, M)
    mustar = _mustar(mod)
    worst = {}
    for name, kind in KINDS.items():
        err, row = _errors(mod, X, eng.acq_grad(mod["post"], X, score=kind, mustar=mustar), kind, mustar)
        print(f"acq parity {label} {name}: " + ", ".join(f"{k} {err[k]:.2e} (row {row[k]})" for k in err))
        for k, e in err.items():
            worst[k] = max(worst.get(k, 0.0), e)
    assert max(worst.values()) <= TOL, worst
    return worst


# ---------------------------------------------------------------- 1. parity with the NumPy statement
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D,n_q,m", SHAPES)
@pytest.mark.parametrize("kernel", RADIAL)
def test_parity_radial(eng, kernel, D, n_q, m, form):
    _parity(eng, _fitted(kernel, D, n_q, m, form), f"{kernel} D={D} N={n_q * (m + 1)} {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D,n_q,m", [(3, 8, 3), (50, 3, 25)])
def test_parity_smallest_and_largest_dimension(eng, D, n_q, m, form):
    _parity(eng, _fitted("Matern52_kernel", D, n_q, m, form), f"Matern52 D={D} N={n_q * (m + 1)} {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_ard(eng, form):
    """Per-dimension length scales: points and gradients in the caller's coordinates, d / d x_d = s_d d / d x~_d."""
    _parity(eng, _fitted("Matern52_kernel", 6, 3, 25, form, ard=True), f"Matern52 ARD D=6 N=78 {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    _parity(eng, _fitted_camphor(form), f"camphor cam_small {form}")


# ---------------------------------------------------------------- 2. against ppbo_mean_grad and ppbo_predict
@pytest.mark.parametrize("which", ["SE", "RQ", "Matern52", "Matern32", "ard", "camphor"])
def test_mean_against_mean_grad(eng, which):
    """tests/test_gpu_gradients.py::test_mean_against_mean_grad's bound: 2 TOL of sum_j |J_jd alpha_j|."""
    mod = (_fitted_camphor("edge") if which == "camphor" else _fitted("Matern52_kernel", 6, 3, 25, "edge", ard=True)
           if which == "ard" else _fitted(which + "_kernel", 20, 3, 25, "node"))
    X = _points(mod, 37)
    out = eng.acq_grad(mod["post"], X, score=aq.MEAN, want_grad_var=False, want_grad_score=False)
    mu, grad = eng.mean_grad(mod["post"], X)
    ref = aq.acq_reference(X, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"], aq.MEAN)
    e_g = np.max(np.abs(host(out["grad_mu"]) - host(grad)) / ref["abs_gmu"])
    e_m = np.max(np.abs(host(out["mu"]) - host(mu)) / ref["abs_mu"])
    print(f"acq against mean_grad {which}: |grad mu - mean_grad| / sum|J alpha| = {e_g:.2e}, |mu - mu| / sum|k alpha| = {e_m:.2e}")
    assert e_g <= 2 * TOL and e_m <= 2 * TOL


@pytest.mark.parametrize("which", ["SE-node", "RQ-edge", "Matern32-edge", "camphor-node"])
def test_values_against_predict(eng, which):
    """mu, var and the score of both entries are within TOL of the statement; their mutual distance is printed."""
    k, form = which.split("-")
    mod = _fitted_camphor(form) if k == "camphor" else _fitted(k + "_kernel", 20, 3, 25, form)
    X = _points(mod, 37)
    mustar = _mustar(mod)
    for name, kind in KINDS.items():
        a = eng.acq_grad(mod["post"], X, score=kind, mustar=mustar, want_grad_mu=False, want_grad_var=False,
                         want_grad_score=False)
        p = eng.predict(mod["post"], X, score=kind, mustar=mustar, want_score=True, want_best=False)
        ea, _ = _errors(mod, X, a, kind, mustar)
        ep, _ = _errors(mod, X, dict(mu=p["mu"], var=p["var"], score=p["score"]), kind, mustar)
        dist = {q: float(np.max(np.abs(host(a[q]) - host(p[q])))) for q in ("mu", "var", "score")}
        print(f"acq against predict {which} {name}: acq_grad {ea}, predict {ep}, |acq_grad - predict| {dist}")
        assert max(ea.values()) <= TOL and max(ep.values()) <= TOL


# ---------------------------------------------------------------- 3. the D ladder
@pytest.mark.parametrize("D", sorted({d for i, dp in enumerate(LADDER) for d in (dp, 1 if i == 0 else LADDER[i - 1] + 1)}))
def test_every_rung_of_the_ladder_at_both_edges(eng, D):
    mod = _fitted("SE_kernel", D, 8, 3, "node")
    X = _points(mod, 12)[:8]
    mustar = _mustar(mod)
    err, row = _errors(mod, X, eng.acq_grad(mod["post"], X, score=aq.EI, mustar=mustar), aq.EI, mustar)
    print(f"acq ladder D={D}: " + ", ".join(f"{k} {err[k]:.2e}" for k in err))
    assert max(err.values()) <= TOL, err


# ---------------------------------------------------------------- 4. bits
OUTS = ("mu", "var", "score", "grad_mu", "grad_var", "grad_score")


@pytest.mark.parametrize("which", ["SE-6-8-3-node", "Matern52-20-3-25-edge"])
def test_chunks_repeats_and_nan_rows(eng, which):
    k, D, n_q, m, form = which.split("-")
    mod = _fitted(k + "_kernel", int(D), int(n_q), int(m), form)
    post, mustar = mod["post"], _mustar(mod)
    X = np.random.default_rng(8).random((1029, int(D)))
    whole = eng.acq_grad(post, X, mustar=mustar)
    again = eng.acq_grad(post, X, mustar=mustar)
    head, tail = eng.acq_grad(post, X[:1024], mustar=mustar), eng.acq_grad(post, X[1024:], mustar=mustar)
    for q in OUTS:
        assert _same(whole[q], again[q]), q
        assert _same(host(whole[q])[:1024], head[q]) and _same(host(whole[q])[1024:], tail[q]), q
    # one gradient asked for alone: the same pass, the same bits
    alone = eng.acq_grad(post, X[:40], mustar=mustar, want_values=False, want_grad_mu=False, want_grad_var=False)
    assert _same(alone["grad_score"], host(whole["grad_score"])[:40])
    Xb = X[:70].copy()
    Xb[3, 1], Xb[64, 0], Xb[69, -1] = np.nan, np.inf, -np.inf
    bad = np.zeros(70, dtype=bool)
    bad[[3, 64, 69]] = True
    out = eng.acq_grad(post, Xb, mustar=mustar)
    for q in OUTS:
        v = host(out[q])
        assert np.all(np.isnan(v[bad])), q
        assert _same(v[~bad], host(whole[q])[:70][~bad]), q


# ---------------------------------------------------------------- 5. the ascent's identities
@pytest.mark.parametrize("kind", ["EI", "variance"])
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D,n_q,m", [(6, 8, 3), (20, 3, 25)])
def test_ascent_identities(eng, D, n_q, m, form, kind):
    mod = _fitted("SE_kernel", D, n_q, m, form)
    post, mustar, kd = mod["post"], _mustar(mod), KINDS[kind]
    rng = np.random.default_rng(12)
    starts = -0.1 + 1.2 * rng.random((130, D))
    lo, hi = bsn.boxes(D)["fixed3"]
    fixed = lo == hi

    def run(s, iters, lower=None, upper=None):
        return {q: host(v) for q, v in eng.acq_ascent(post, s, score=kd, mustar=mustar, lower=lower, upper=upper, iters=iters).items()}

    # iters = 0: the clipped starts and acq_grad's bits there
    r0 = run(starts, 0, lo, hi)
    assert _same(r0["x"], np.clip(starts, lo, hi)) and not r0["iters"].any()
    at = eng.acq_grad(post, r0["x"], score=kd, mustar=mustar, want_grad_mu=False, want_grad_var=False, want_grad_score=False)
    for q in ("score", "mu", "var"):
        assert _same(r0[q], at[q]), q
    # the score never decreases, every x is inside its box, a fixed coordinate never moves, the values are acq_grad's at x
    prev, moved = r0["score"], 0
    for n in range(1, 7):
        r = run(starts, n, lo, hi)
        assert np.all(r["score"] >= prev), n
        assert np.all((r["x"] >= lo) & (r["x"] <= hi)) and np.all(r["x"][:, fixed] == lo[fixed])
        assert np.all(r["iters"] <= n)
        moved += int((r["score"] > prev).sum())
        prev = r["score"]
    assert moved > 0
    at = eng.acq_grad(post, r["x"], score=kd, mustar=mustar, want_grad_mu=False, want_grad_var=False, want_grad_score=False)
    for q in ("score", "mu", "var"):
        assert _same(r[q], at[q]), q
    # a box of one point: the point, its values, no iteration
    pt = 0.1 + 0.8 * rng.random(D)
    one = run(starts[:5], 6, pt, pt)
    assert _same(one["x"], np.tile(pt, (5, 1))) and not one["iters"].any()
    # a start's result does not depend on K, on its position or on its neighbours
    full = run(starts, 6)
    assert all(_same(full[q], run(starts, 6)[q]) for q in full)                 # a repeated call
    for K, row in ((33, 17), (130, 129)):
        many = run(starts[:K], 6) if K < 130 else full
        alone = run(starts[row:row + 1], 6)
        for q in full:
            assert _same(alone[q][0], many[q][row]), (q, K)
    perm = rng.permutation(130)
    shuffled = run(starts[perm], 6)
    for q in full:
        assert _same(shuffled[q], full[q][perm]), q
    # a NaN start: a NaN row, the others untouched
    sb = starts.copy()
    sb[7, 2] = np.nan
    nan = run(sb, 6)
    keep = np.arange(130) != 7
    assert np.isnan(nan["score"][7]) and np.isnan(nan["mu"][7]) and np.isnan(nan["var"][7]) and np.isnan(nan["x"][7, 2])
    assert nan["iters"][7] == 0
    for q in full:
        assert _same(nan[q][keep], full[q][keep]), q


# ---------------------------------------------------------------- 6. the iteration, step by step
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("case", list(aq.ASCENT_CASES))
def test_iteration_against_the_numpy_statement(eng, case, form):
    """The device's iterates against bb_ascent_box replayed on the DEVICE's own acq_grad (which test 1 holds to the
    statement), over the (start, n) pairs the statement's branch margins keep; the bound is search_ref.x_bound of the
    statement's own sensitivity, `it` is equal, and the cap on the pairs left out is tests/test_gpu_search_stages.py's
    (checked on the reference alone in tests/test_acq_host.py)."""
    kernel, D, n_q, m = aq.ASCENT_CASES[case][:4]
    mod = _fitted(kernel, D, n_q, m, form)
    Xd, th, _, _ = aq.ascent_design(case)
    assert np.array_equal(Xd, mod["X"]) and th == mod["th"]          # the host test's twin is this model's
    kind, lo, hi, starts = aq.ascent_setup(case)
    post, mustar, tol = mod["post"], _mustar(mod), sr.TOLS[0]
    s = bsn.sensitivity_box(aq.acq_fg(mod["X"], th, kernel, mod["alpha"], mod["A"], kind, mustar), starts, lo, hi,
                            sr.ASCENT_ITERS, tol)
    bound = sr.x_bound(s.dev)
    assert s.flips == 0 and s.left_out <= 0.125, (case, s.flips, s.left_out)

    def fg(x):
        o = eng.acq_grad(post, x[None, :], score=kind, mustar=mustar, want_grad_mu=False, want_grad_var=False)
        return float(host(o["score"])[0]), host(o["grad_score"])[0]

    xs, _, its, _ = bsn.ascend_all_box(fg, starts, lo, hi, sr.ASCENT_ITERS, tol)
    worst = np.zeros(sr.ASCENT_ITERS + 1)
    for n in range(sr.ASCENT_ITERS + 1):
        r = eng.acq_ascent(post, starts, score=kind, mustar=mustar, lower=lo, upper=hi, iters=n, tol=tol)
        keep = s.keep[:, n]
        assert np.array_equal(host(r["iters"])[keep], its[keep, n]), (case, n)
        worst[n] = np.abs(host(r["x"]) - xs[:, n])[keep].max()
    print(f"acq iteration {case} {form}: |x_dev - x_replay| per n {np.array2string(worst, precision=1)}, bound "
          f"{np.array2string(bound, precision=1)}, left out {s.left_out:.3f}, it at n = {sr.ASCENT_ITERS}: "
          f"{np.bincount(its[:, -1], minlength=sr.ASCENT_ITERS + 1)}")
    assert np.all(worst <= bound), (case, worst, bound)


# ---------------------------------------------------------------- 7. GPModel
@pytest.mark.parametrize("score", ["EI", "variance"])
def test_maximize_acquisition(eng, score):
    mod = _fitted("SE_kernel", 6, 8, 3, "edge")
    gp = _stub_gp(eng, mod)
    gp.D, gp.mustar = 6, _mustar(mod)
    cand = np.random.default_rng(4).random((4096, 6))
    out = gp.maximize_acquisition(score=score, n_starts=8, X_cand=cand, iters=30)
    assert out["x"].shape == (6,) and np.all((out["x"] >= 0.0) & (out["x"] <= 1.0))
    assert out["starts"].shape == (8, 6) and out["scores"].shape == (8,) and out["iters"].shape == (8,)
    assert out["score"] == out["scores"].max() and out["score"] >= out["start_scores"][0]      # monotone: exactly
    at = gp.acquisition_grad(out["x"], score=score)
    assert at["score"][0] == out["score"] and at["mu"][0] == out["mu"] and at["var"][0] == out["var"]
    print(f"maximize_acquisition {score}: pool best {out['start_scores'][0]:.6g} -> {out['score']:.6g}, iterations {out['iters']}")
    lo = np.zeros(6)
    lo[1] = 0.25
    boxed = gp.maximize_acquisition(score=score, n_starts=4, X_cand=cand, lower=lo, fixed={3: 0.5}, iters=10)
    assert boxed["x"][3] == 0.5 and boxed["x"][1] >= 0.25 and np.all(boxed["xs"][:, 3] == 0.5)
    with pytest.raises(ValueError, match="maximize_acquisition"):
        gp.maximize_acquisition(score="mean")


def test_ard_round_trip(eng):
    """The gradient in the caller's coordinates is s_d times the one in the model's; x comes back inside the caller's box."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, _ptr
    mod = _fitted("Matern52_kernel", 6, 3, 25, "edge", ard=True)
    post, mustar = mod["post"], _mustar(mod)
    assert post.scale is not None
    X = _points(mod, 37)
    out = eng.acq_grad(post, X, mustar=mustar)
    pts, md, raw = eng.scale_points(X, post.scale), eng._model(post, True), eng.empty(37, 6)
    rc = eng.lib.ppbo_acq_grad(eng.ctx, C.byref(md), _ptr(pts), 37, SCORE_POINTWISE_EI, mustar, None, None, None, None, None,
                               _ptr(raw), eng._stream())
    assert rc == 0
    assert np.array_equal(host(out["grad_score"]), host(raw) * post.scale[None, :])
    lo, hi = bsn.boxes(6)["ragged"]
    r = eng.acq_ascent(post, X, mustar=mustar, lower=lo, upper=hi, iters=6)
    x = host(r["x"])
    assert np.all((x >= lo) & (x <= hi))
    at = eng.acq_grad(post, x, mustar=mustar)
    ref = aq.acq_reference(x, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"], aq.EI, mustar)
    assert np.max(np.abs(host(r["score"]) - host(at["score"]))) <= TOL * np.max(ref["abs_mu"] + 1.0)


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd import _lib
    from ppbo_amd.engine import SCORE_MEAN, SCORE_POINTWISE_EI, SCORE_VARIANCE, _ptr
    mod = _fitted("SE_kernel", 6, 8, 3, "node")
    post = mod["post"]
    X = _points(mod, 37)
    before = eng.acq_grad(post, X)
    dx = eng.dev(X)
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam, badform, cam = eng._model(post, True), eng._model(post, True), eng._model(post, True)
    nolam.d_lam_diag = 0
    badform.form = 2
    cam._coords = _lib.coords(_lib.COORDS_CAMPHOR, np.ones(6), None)
    cam.coords = cam._coords
    EI, VAR, MEAN = SCORE_POINTWISE_EI, SCORE_VARIANCE, SCORE_MEAN
    sent = -12345.0
    o1 = [eng.empty(37).fill_(sent) for _ in range(3)]
    o2 = [eng.empty(37, 6).fill_(sent) for _ in range(3)]
    its = eng.dev(np.full(37, -7), dtype=__import__("torch").int32)

    def grad(model, x, M, kind, outs="all"):
        ptrs = [_ptr(t) for t in o1 + o2] if outs == "all" else [None] * 6 if outs == "none" else outs
        rc = eng.lib.ppbo_acq_grad(eng.ctx, C.byref(model) if model is not None else None, _ptr(x), M, kind, 0.1, *ptrs, eng._stream())
        return rc, eng._err()

    def ascent(model, s, K, kind, box=None, iters=3, tol=1e-9, x_out=o2[0]):
        bx = np.ascontiguousarray(np.asarray(box, dtype=np.float64)) if box is not None else None
        rc = eng.lib.ppbo_acq_ascent(eng.ctx, C.byref(model) if model is not None else None, _ptr(s), K,
                                     eng._dptr(bx) if bx is not None else None, kind, 0.1, iters, tol, _ptr(x_out), _ptr(o1[0]),
                                     _ptr(o1[1]), _ptr(o1[2]), _ptr(its), eng._stream())
        return rc, eng._err()

    only_var = [None, _ptr(o1[1]), None, None, None, None]
    for args in ((None, dx, 37, EI), (md, None, 37, EI), (md, dx, 37, EI, "none"), (md, dx, 0, EI), (md, dx, -5, EI),
                 (md, dx, 2 ** 31, EI), (md, dx, 37, 3), (md, dx, 37, -1), (md32, dx, 37, EI), (md32, dx, 37, MEAN),
                 (badform, dx, 37, VAR), (cam, dx, 37, EI), (cam, dx, 37, MEAN), (bare, dx, 37, EI), (bare, dx, 37, VAR),
                 (bare, dx, 37, MEAN, only_var), (nolam, dx, 37, VAR), (nolam, dx, 37, MEAN, only_var)):
        rc, msg = grad(*args)
        assert rc != 0 and "invalid argument" in msg, ("acq_grad", args[2:], rc, msg)
    unit = np.stack([np.zeros(6), np.ones(6)])
    flipped, nanbox, infbox = unit.copy(), unit.copy(), unit.copy()
    flipped[0, 2], flipped[1, 2] = 0.6, 0.4
    nanbox[0, 1] = np.nan
    infbox[1, 4] = np.inf
    for args in ((None, dx, 37, EI), (md, None, 37, EI), (md, dx, 37, EI, None, 3, 1e-9, None), (md, dx, 0, EI), (md, dx, -1, EI),
                 (md, dx, 1025, EI), (md, dx, 37, EI, None, -1), (md, dx, 37, EI, None, 1001), (md, dx, 37, EI, None, 3, -1e-9),
                 (md, dx, 37, EI, None, 3, np.nan), (md, dx, 37, EI, None, 3, np.inf), (md, dx, 37, EI, flipped),
                 (md, dx, 37, EI, nanbox), (md, dx, 37, EI, infbox), (md, dx, 37, 5), (md32, dx, 37, EI), (badform, dx, 37, EI),
                 (cam, dx, 37, VAR), (bare, dx, 37, EI), (bare, dx, 37, MEAN), (nolam, dx, 37, VAR)):
        rc, msg = ascent(*args)
        assert rc != 0 and "invalid argument" in msg, ("acq_ascent", args[2:], rc, msg)
    # nothing was launched: the outputs are untouched
    assert all(bool((t == sent).all()) for t in o1 + o2) and bool((its == -7).all())
    # the mean alone needs no operator
    assert grad(bare, dx, 37, MEAN, [_ptr(o1[0]), None, _ptr(o1[2]), _ptr(o2[0]), None, _ptr(o2[2])])[0] == 0
    assert _same(o1[0], before["mu"]) and _same(o2[0], before["grad_mu"]) and _same(o2[2], before["grad_mu"])
    assert ascent(md, dx, 37, EI, [[0.0] * 6, [2.0] * 6])[0] == 0          # any finite box, e.g. an ARD model's [0, s]
    after = eng.acq_grad(post, X)
    for q in OUTS:
        assert _same(before[q], after[q]), q
    with pytest.raises(ValueError, match="acq_grad"):
        eng.acq_grad(post, X[:, :5])
    with pytest.raises(ValueError, match="score kind"):
        eng.acq_grad(post, X, score=7)
    with pytest.raises(ValueError, match="acq_ascent"):
        eng.acq_ascent(post, np.zeros((1025, 6)))
    cam_ard = _fitted_camphor_ard()
    with pytest.raises(ValueError, match="camphor_copper_ard_kernel"):
        eng.acq_grad(cam_ard["post"], np.random.default_rng(0).random((5, 6)))
    with pytest.raises(ValueError, match="camphor_copper_ard_kernel"):
        eng.acq_ascent(cam_ard["post"], np.random.default_rng(0).random((5, 6)))
