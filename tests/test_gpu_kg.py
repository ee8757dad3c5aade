"""GPU: the knowledge gradient -- ppbo_kg_envelope / Engine.kg_envelope on constructed lines and ppbo_predict_kg /
Engine.predict_kg / GPModel.knowledge_gradient on fitted models, against the NumPy statements of tests/kg_numpy.py, the
exact identities of the march, the oracle-based reference of the tournament, NaN rows and fields, and the refusals.  The
star design of test_gpu_pairs: n_q = 7, m = 25, N = 182.

Bound against kg_numpy: 1e-12 (max|a| + max|b|) per row -- four orders above what the two NumPy statements differ by,
room for the device's exp, erfc and division.  Worst figures measured on MI355X are in DESIGN.md section 7 ("Knowledge
gradient")."""
import ctypes as C

import numpy as np
import pytest

import kg_numpy as kn
import tournament_numpy as tn
from test_gpu_pairs import _fitted, _fitted_golden, _forms, host

pytestmark = pytest.mark.gpu

TOL = 1e-12
MBS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1024)     # both sides of every lane-group and register-tile edge
MAS = (1, 127, 129)                                           # one row, and both sides of a whole number of workgroups


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _row_scale(a, slopes, self_a, self_b):
    sa = np.abs(a).max() * np.ones(len(slopes))
    sb = np.abs(slopes).max(axis=1)
    if self_a is not None:
        sa, sb = np.maximum(sa, np.abs(self_a)), np.maximum(sb, np.abs(self_b))
    return sa + sb


def _envelope(eng, a, slopes, self_a=None, self_b=None, label=""):
    """One call of the direct entry against kg_numpy.kg_march row by row; returns (out, worst error / scale)."""
    out = eng.kg_envelope(a, slopes, self_a, self_b)
    kg, kinks = host(out["kg"]), host(out["kinks"])
    kg0, kinks0 = kn.rows(a, slopes, self_a, self_b)
    err = np.abs(kg - kg0) / _row_scale(a, slopes, self_a, self_b)
    n_lines = slopes.shape[1] + (self_a is not None)
    print(f"kg_envelope {label} Ma={len(slopes)} Mb={slopes.shape[1]} own={self_a is not None}: worst {err.max():.2e} of "
          f"max|a| + max|b|, kinks {kinks.min()} .. {kinks.max()}")
    assert err.max() <= TOL
    assert np.all(kg >= 0.0) and np.all(kinks >= 0) and np.all(kinks <= n_lines - 1)
    assert np.array_equal(kinks, kinks0)
    assert (out["best_val"], out["best_idx"]) == kn.best(kg)
    return out, err.max()


def _gp_lines(rng, Ma, Mb):
    """Lines of the shape a posterior gives: intercepts a smooth function of a position plus noise, slopes a bump around
    each row's own position with a few small ones elsewhere."""
    x = rng.random(Mb)
    a = np.sin(6.0 * x + 1.0) + 0.3 * rng.standard_normal(Mb)
    c = rng.random(Ma)
    slopes = 0.3 * np.exp(-0.5 * ((x[None, :] - c[:, None]) / 0.15) ** 2) * rng.choice([-1.0, 1.0], (Ma, 1))
    slopes += 1e-3 * rng.standard_normal((Ma, Mb))
    return a, slopes, np.sin(6.0 * c + 1.0) + 0.3 * rng.standard_normal(Ma), 0.3 + 0.05 * rng.random(Ma)


# ---------------------------------------------------------------- 1. the envelope entry on constructed lines
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("Mb", MBS)
def test_envelope_against_numpy(eng, Mb, own):
    rng = np.random.default_rng(100 + Mb)
    for Ma in MAS:
        a, slopes, sa, sb = _gp_lines(rng, Ma, Mb)
        _envelope(eng, a, slopes, *((sa, sb) if own else ()), label="gp-shaped")
        a, slopes = rng.standard_normal(Mb), rng.standard_normal((Ma, Mb))
        _envelope(eng, a, slopes, *((rng.standard_normal(Ma), rng.standard_normal(Ma)) if own else ()), label="normal")


@pytest.mark.parametrize("own", [False, True])
def test_envelope_tangent_family_is_the_longest_loop(eng, own):
    """Mb = 1024 lines -t^2 / 2 + f t z: every one on the envelope, so the march takes every step its count allows."""
    Mb = 1024
    a, t = kn.tangents(Mb)
    f = np.array([1.0, 0.5, 2.0])
    slopes = f[:, None] * t[None, :]
    t_own = 3.0 + 6.0 / (Mb - 1)                                  # the next tangent beyond the grid
    sa, sb = (np.full(3, -0.5 * t_own * t_own), f * t_own) if own else (None, None)
    out, _ = _envelope(eng, a, slopes, sa, sb, label="tangents")
    assert np.all(host(out["kinks"]) == (Mb if own else Mb - 1))


@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("Mb", (17, 256, 1024))
def test_envelope_ties(eng, Mb, own):
    rng = np.random.default_rng(200 + Mb)
    Ma = 129
    ints = lambda *shape: rng.integers(-3, 4, shape).astype(float)      # noqa: E731
    # small integers: equal slopes, equal intercepts, many lines through one point
    _envelope(eng, ints(Mb), ints(Ma, Mb), *((ints(Ma), ints(Ma)) if own else ()), label="integers")
    # all intercepts equal: every line passes through (0, a)
    _envelope(eng, np.full(Mb, 0.7), rng.standard_normal((Ma, Mb)), *((np.full(Ma, 0.7), rng.standard_normal(Ma)) if own else ()),
              label="equal intercepts")
    # all slopes of a row equal: nothing is ever steeper, KG = 0 exactly
    s = rng.standard_normal(Ma)
    out, _ = _envelope(eng, rng.standard_normal(Mb), np.repeat(s[:, None], Mb, axis=1),
                       *((rng.standard_normal(Ma), s) if own else ()), label="equal slopes")
    assert np.all(host(out["kg"]) == 0.0) and np.all(host(out["kinks"]) == 0)
    assert out["best_idx"] == 0 and out["best_val"] == 0.0               # all tied: the first row


def test_envelope_is_a_function_of_the_set_of_lines(eng):
    """Bitwise: a repeated call, the first rows alone, permuted lines, every line twice (which crosses from the 16-lane
    groups to whole wavefronts at Mb = 200 -> 400), the own line moved into the field."""
    rng = np.random.default_rng(7)
    Ma, Mb = 300, 200
    a, slopes, sa, sb = _gp_lines(rng, Ma, Mb)
    slopes[5] = np.round(slopes[5] * 8.0)                            # a row of heavy ties
    ref = eng.kg_envelope(a, slopes, sa, sb)
    kg, kinks = host(ref["kg"]), host(ref["kinks"])

    def same(out, rows=slice(None)):
        assert np.array_equal(host(out["kg"]), kg[rows]) and np.array_equal(host(out["kinks"]), kinks[rows])

    same(eng.kg_envelope(a, slopes, sa, sb))
    same(eng.kg_envelope(a, slopes[:100], sa[:100], sb[:100]), slice(0, 100))
    p = rng.permutation(Mb)
    same(eng.kg_envelope(a[p], slopes[:, p], sa, sb))
    same(eng.kg_envelope(np.tile(a, 2), np.tile(slopes, (1, 2)), sa, sb))
    for Mb2 in (16, 64, 256):                                        # the same across each kernel shape's edge
        r = eng.kg_envelope(a[:Mb2], slopes[:, :Mb2], sa, sb)
        d = eng.kg_envelope(np.tile(a[:Mb2], 2), np.tile(slopes[:, :Mb2], (1, 2)), sa, sb)
        assert np.array_equal(host(r["kg"]), host(d["kg"])) and np.array_equal(host(r["kinks"]), host(d["kinks"]))
    # one row's own line as a field line of that row
    one = eng.kg_envelope(np.append(a, sa[3]), np.append(slopes[3], sb[3])[None, :])
    assert host(one["kg"])[0] == kg[3] and host(one["kinks"])[0] == kinks[3]
    assert ref["best_idx"] == int(np.argmax(kg)) and ref["best_val"] == kg.max()


def test_envelope_nan_rules(eng):
    rng = np.random.default_rng(8)
    Ma, Mb = 150, 70
    a, slopes, sa, sb = _gp_lines(rng, Ma, Mb)
    clean = eng.kg_envelope(a, slopes, sa, sb)
    kg = host(clean["kg"])
    top = int(np.argmax(kg))
    s2, sa2, sb2 = slopes.copy(), sa.copy(), sb.copy()
    s2[top, 31], s2[11, 69], sa2[20], sb2[140] = np.nan, np.inf, np.nan, -np.inf
    bad = np.zeros(Ma, dtype=bool)
    bad[[top, 11, 20, 140]] = True
    out = eng.kg_envelope(a, s2, sa2, sb2)
    got = host(out["kg"])
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], kg[~bad])
    assert np.all(host(out["kinks"])[bad] == 0)
    assert not bad[out["best_idx"]] and (out["best_val"], out["best_idx"]) == kn.best(got)
    # a NaN intercept poisons every row
    a2 = a.copy()
    a2[37] = np.nan
    out = eng.kg_envelope(a2, slopes, sa, sb)
    assert np.all(np.isnan(host(out["kg"]))) and out["best_idx"] == -1 and np.isnan(out["best_val"])


# ---------------------------------------------------------------- 2. predict_kg on the device's own outputs
def _sets(rng, mod, Ma, Mb):
    """Candidates and a field in the box: uniform points, a few design rows in either set."""
    N, D = mod["X"].shape
    Xa, Xb = rng.random((Ma, D)), rng.random((Mb, D))
    ka, kb = min(8, Ma // 4), min(4, Mb // 4)
    Xa[:ka] = mod["X"][rng.integers(0, N, ka)]
    Xb[:kb] = mod["X"][rng.integers(0, N, kb)]
    return Xa, Xb


def _kg(eng, post, Xa, Xb, **kw):
    out = eng.predict_kg(post, Xa, Xb, want_kinks=True, **kw)
    return {k: (host(v) if hasattr(v, "cpu") else v) for k, v in out.items()}


def _device_lines(eng, post, Xa, Xb, noise_var):
    t = eng.predict_tournament(post, Xa, Xb, want_cov=True, want_best=False)
    return t, kn.lines_from_posterior(host(t["mu_a"]), host(t["var_a"]), host(t["mu_b"]), host(t["cov"]), noise_var, Xa, Xb)


def _on_device_outputs(eng, mod, Ma=300, Mb=200, seed=3, label="", rows=None):
    post = mod["post"]
    Xa, Xb = _sets(np.random.default_rng(seed), mod, Ma, Mb)
    nv = float(mod["th"][0]) ** 2
    out = _kg(eng, post, Xa, Xb)
    t, (a, slopes, sa, sb) = _device_lines(eng, post, Xa, Xb, nv)
    for k in ("mu_a", "var_a", "mu_b", "var_b"):
        assert np.array_equal(out[k], host(t[k])), k
    pa, pb = eng.predict(post, Xa), eng.predict(post, Xb)
    assert np.array_equal(out["mu_a"], host(pa["mu"])) and np.array_equal(out["var_a"], host(pa["var"]))
    assert np.array_equal(out["mu_b"], host(pb["mu"])) and np.array_equal(out["var_b"], host(pb["var"]))
    rows = np.arange(Ma) if rows is None else rows
    kg0, kinks0 = kn.rows(a, slopes[rows], sa[rows], sb[rows])
    err = np.abs(out["kg"][rows] - kg0) / _row_scale(a, slopes[rows], sa[rows], sb[rows])
    print(f"predict_kg against kg_numpy on the device's lines, {label} {Ma} x {Mb}: worst {err.max():.2e} of max|a| + max|b|, "
          f"kinks {out['kinks'].min()} .. {out['kinks'].max()} (mean {out['kinks'].mean():.2f}), max KG {out['kg'].max():.3e}")
    assert err.max() <= TOL
    assert np.array_equal(out["kinks"][rows], kinks0) and np.all(out["kinks"] <= Mb)
    assert np.all(out["kg"] >= 0.0)
    assert (out["best_val"], out["best_idx"]) == kn.best(out["kg"])
    return out


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20), ("RQ_kernel", 40)])
def test_predict_kg_radial(eng, kernel, D, form):
    """SE D = 6 in the node form is scored by the one-launch kernel (the chunk's K* from a launch of its own); the others
    take the three-launch path."""
    _on_device_outputs(eng, _fitted(kernel, D, _forms()[form]), label=f"{kernel} D={D} {form}")


def test_predict_kg_ard(eng):
    _on_device_outputs(eng, _fitted("Matern52_kernel", 6, None, ard=True), label="Matern52 ARD D=6")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_predict_kg_camphor(eng, form):
    _on_device_outputs(eng, _fitted_golden("cam_small", _forms()[form]), label=f"camphor cam_small {form}")


def test_predict_kg_camphor_ard(eng):
    from test_gpu_marginals import _fitted_camphor_ard_golden
    _on_device_outputs(eng, _fitted_camphor_ard_golden(), label="camphor ARD camphor_ard/spread")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_predict_kg_chunk_boundary(eng, form):
    """Ma = 65536 + 77 against Mb = 16: the rows on either side of the chunk edge against NumPy, and the index that comes
    back is the global row."""
    Ma = 65536 + 77
    rows = np.r_[0:40, 65536 - 40:Ma]
    out = _on_device_outputs(eng, _fitted("SE_kernel", 6, _forms()[form]), Ma=Ma, Mb=16, seed=15, label=f"SE D=6 {form}", rows=rows)
    assert out["best_idx"] == int(np.argmax(out["kg"]))


# ---------------------------------------------------------------- 3. exact identities of predict_kg
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20)])
def test_predict_kg_exact_identities(eng, kernel, D, form):
    mod = _fitted(kernel, D, _forms()[form])
    post = mod["post"]
    rng = np.random.default_rng(5)
    Xa, Xb = _sets(rng, mod, 777, 100)
    out = _kg(eng, post, Xa, Xb)
    again = _kg(eng, post, Xa, Xb)
    for k in ("kg", "kinks", "mu_a", "var_a", "mu_b", "var_b"):
        assert np.array_equal(out[k], again[k]), k
    assert (out["best_idx"], out["best_val"]) == (again["best_idx"], again["best_val"])
    assert out["best_idx"] == int(np.argmax(out["kg"])) and out["best_val"] == out["kg"].max()
    head = _kg(eng, post, Xa[:100], Xb)
    assert np.array_equal(head["kg"], out["kg"][:100]) and np.array_equal(head["kinks"], out["kinks"][:100])
    perm = _kg(eng, post, Xa, Xb[rng.permutation(100)])
    assert np.array_equal(perm["kg"], out["kg"]) and np.array_equal(perm["kinks"], out["kinks"])
    twice = _kg(eng, post, Xa, np.tile(Xb, (2, 1)))
    assert np.array_equal(twice["kg"], out["kg"]) and np.array_equal(twice["kinks"], out["kinks"])
    lean = eng.predict_kg(post, Xa, Xb, want_best=False)
    assert lean["kinks"] is None and np.array_equal(host(lean["kg"]), out["kg"])


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20)])
def test_predict_kg_field_equal_to_the_candidate(eng, kernel, D, form):
    """Mb = 1 with the field equal to the candidate: the two lines are the same belief, so KG == 0.0 and there is no kink.
    cov(a, a) from the cross product and var_a from predict's contraction are the same quadratic form summed in two orders
    and differ in the last bits (4.4e-17 .. 5.8e-16 of KG in 4 of these 12 cases, as first measured on MI355X), so a field
    point that is the candidate, bit for bit, takes the own line's slope (csrc/kg.hip)."""
    mod = _fitted(kernel, D, _forms()[form])
    Xa, _ = _sets(np.random.default_rng(5), mod, 777, 100)
    ones = [_kg(eng, mod["post"], Xa[i:i + 1], Xa[i:i + 1]) for i in (0, 9, 500)]
    print(f"field == candidate {kernel} D={D} {form}: KG = " + ", ".join(f"{o['kg'][0]:.2e}" for o in ones))
    for one in ones:
        assert one["kg"][0] == 0.0 and one["best_idx"] == 0 and one["best_val"] == 0.0 and one["kinks"][0] == 0


@pytest.mark.parametrize("form", ["node", "edge"])
def test_predict_kg_field_taken_from_the_candidates(eng, form):
    """The field a subset of the candidates (the recommendation and its runners-up among the pool's rows): against the
    NumPy statement with the same rule, kink counts included; for a candidate that is in the field, dropping its own
    point from the field changes no bit (the own line already stands for it); other rows keep the bits they have
    against the field alone."""
    mod = _fitted("Matern52_kernel", 6, _forms()[form])
    post = mod["post"]
    rng = np.random.default_rng(6)
    Xa, _ = _sets(rng, mod, 400, 8)
    idx = rng.choice(400, 70, replace=False)
    Xb = Xa[idx].copy()
    nv = float(mod["th"][0]) ** 2
    out = _kg(eng, post, Xa, Xb)
    _, (a, slopes, sa, sb) = _device_lines(eng, post, Xa, Xb, nv)
    assert np.array_equal(slopes[idx, np.arange(70)], sb[idx])               # the rule reached the statement
    kg0, kinks0 = kn.rows(a, slopes, sa, sb)
    err = np.abs(out["kg"] - kg0) / _row_scale(a, slopes, sa, sb)
    print(f"predict_kg, field inside the candidates, {form}: worst {err.max():.2e} of max|a| + max|b|")
    assert err.max() <= TOL and np.array_equal(out["kinks"], kinks0)
    for j in (0, 33, 69):
        alone = _kg(eng, post, Xa[idx[j]:idx[j] + 1], np.delete(Xb, j, axis=0))
        assert alone["kg"][0] == out["kg"][idx[j]] and alone["kinks"][0] == out["kinks"][idx[j]]


# ---------------------------------------------------------------- 4. against the oracle-based reference
@pytest.mark.parametrize("tau0", [False, True])
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20), ("RQ_kernel", 40)])
def test_predict_kg_against_the_reference(eng, kernel, D, form, tau0):
    """KG is Lipschitz in its lines: moving every intercept by at most d_mu moves E[h] and h(0) by at most d_mu each, and
    moving every slope by at most d_b moves E[h] by at most d_b E|Z| < 0.8 d_b.  So per row
        |kg - kg_ref| <= 2 max|d_mu| + 0.8 max|d_slope| + 1e-12 scale
    with the deviations of that row's own lines from the reference's as measured -- no tolerance is invented."""
    mod = _fitted(kernel, D, _forms()[form])
    rng = np.random.default_rng(31)
    Xa, Xb = rng.random((300, D)), rng.random((200, D))
    nv = 0.0 if tau0 else float(mod["th"][0]) ** 2
    out = _kg(eng, mod["post"], Xa, Xb, noise_var=nv)
    _, (a, slopes, sa, sb) = _device_lines(eng, mod["post"], Xa, Xb, nv)
    ref = tn.tournament_reference(Xa, Xb, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"])
    a0, slopes0, sa0, sb0 = kn.lines_from_posterior(ref["mu_a"], ref["var_a"], ref["mu_b"], ref["cov"], nv)
    kg0, _ = kn.rows(a0, slopes0, sa0, sb0)
    d_mu = np.maximum(np.abs(a - a0).max(), np.abs(sa - sa0))
    d_b = np.maximum(np.abs(slopes - slopes0).max(axis=1), np.abs(sb - sb0))
    bound = 2.0 * d_mu + 0.8 * d_b + TOL * _row_scale(a0, slopes0, sa0, sb0)
    err = np.abs(out["kg"] - kg0)
    print(f"predict_kg against the reference {kernel} D={D} {form} tau^2={nv:.1e}: |kg - ref| <= {err.max():.2e} (max KG "
          f"{kg0.max():.2e}), worst share of its bound {np.max(err / bound):.2f}; d_mu <= {d_mu.max():.1e}, d_slope <= {d_b.max():.1e}")
    assert np.all(err <= bound)


# ---------------------------------------------------------------- 5. behaviour
@pytest.mark.parametrize("form", ["node", "edge"])
def test_more_noise_is_less_knowledge(eng, form):
    mod = _fitted("Matern52_kernel", 6, _forms()[form])
    Xa, Xb = _sets(np.random.default_rng(41), mod, 500, 64)
    kg = [_kg(eng, mod["post"], Xa, Xb, noise_var=nv)["kg"] for nv in (0.0, float(mod["th"][0]) ** 2, 1e6)]
    scale = np.abs(host(eng.predict(mod["post"], Xb)["mu"])).max() + float(mod["th"][2])     # max|a| + a bound of the slopes
    for hi, lo in zip(kg[:-1], kg[1:]):
        assert np.all(hi >= lo - 1e-15 * scale)
    assert np.all(kg[2] >= 0.0) and kg[0].max() > 0.0


@pytest.mark.parametrize("form", ["node", "edge"])
def test_predict_kg_nan_rows_and_field(eng, form):
    mod = _fitted("Matern52_kernel", 6, _forms()[form])
    Xa, Xb = _sets(np.random.default_rng(18), mod, 150, 70)
    clean = _kg(eng, mod["post"], Xa, Xb)
    Xa_bad = Xa.copy()
    Xa_bad[clean["best_idx"], 2], Xa_bad[140, 0] = np.nan, np.inf
    bad = np.zeros(150, dtype=bool)
    bad[[clean["best_idx"], 140]] = True
    out = _kg(eng, mod["post"], Xa_bad, Xb)
    assert np.all(np.isnan(out["kg"][bad])) and np.array_equal(out["kg"][~bad], clean["kg"][~bad])
    assert not bad[out["best_idx"]] and (out["best_val"], out["best_idx"]) == kn.best(out["kg"])
    Xb_bad = Xb.copy()
    Xb_bad[37, 4] = np.nan
    out = _kg(eng, mod["post"], Xa, Xb_bad)
    assert np.all(np.isnan(out["kg"])) and out["best_idx"] == -1 and np.isnan(out["best_val"])
    assert np.array_equal(out["mu_a"], clean["mu_a"]) and np.isnan(out["mu_b"][37])


def test_refusals_leave_the_context_usable(eng):
    import torch
    from ppbo_amd import _lib
    from ppbo_amd.engine import _ptr
    mod = _fitted("SE_kernel", 6, None)
    post = mod["post"]
    Xa, Xb = _sets(np.random.default_rng(19), mod, 100, 30)
    before = _kg(eng, post, Xa, Xb)
    da, db = eng.dev(Xa), eng.dev(Xb)
    sentinel = -12345.0
    kg = eng.empty(100).fill_(sentinel)
    kinks = torch.full((100,), -7, dtype=torch.int32, device=kg.device)
    outs = [eng.empty(100).fill_(sentinel), eng.empty(100).fill_(sentinel), eng.empty(30).fill_(sentinel),
            eng.empty(30).fill_(sentinel)]
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam, badform = eng._model(post, True), eng._model(post, True)
    nolam.d_lam_off = 0
    badform.form = 2

    def call(model, a, b, Ma, Mb, nv, out=kg):
        bv, bi = C.c_double(sentinel), C.c_int64(-7)
        rc = eng.lib.ppbo_predict_kg(eng.ctx, C.byref(model) if model is not None else None, _ptr(a), Ma, _ptr(b), Mb, nv,
                                     _ptr(out), _ptr(kinks), *[_ptr(o) for o in outs], C.byref(bv), C.byref(bi), eng._stream())
        return rc, eng._err(), bv.value, bi.value

    for args in ((None, da, db, 100, 30, 0.0), (md, None, db, 100, 30, 0.0), (md, da, None, 100, 30, 0.0),
                 (md, da, db, 0, 30, 0.0), (md, da, db, 2 ** 31, 30, 0.0), (md, da, db, 100, 0, 0.0),
                 (md, da, db, 100, _lib.KG_MAX_B + 1, 0.0), (md, da, db, 100, 30, -1e-300), (md, da, db, 100, 30, np.inf),
                 (md, da, db, 100, 30, np.nan), (md, da, db, 100, 30, 0.0, None), (md32, da, db, 100, 30, 0.0),
                 (bare, da, db, 100, 30, 0.0), (nolam, da, db, 100, 30, 0.0), (badform, da, db, 100, 30, 0.0)):
        rc, msg, bv, bi = call(*args)
        assert rc < 0 and msg.startswith("invalid argument"), (args[3:], rc, msg)
        assert (bv, bi) == (sentinel, -7)
    # the direct entry
    a, s = eng.dev(np.zeros(30)), eng.dev(np.zeros((100, 30)))
    for args in ((None, s, 30, None, None, 100, 30), (a, None, 30, None, None, 100, 30), (a, s, 29, None, None, 100, 30),
                 (a, s, 30, kg, None, 100, 30), (a, s, 30, None, kg, 100, 30), (a, s, 30, None, None, 0, 30),
                 (a, s, 30, None, None, 100, 0), (a, s, 30, None, None, 100, _lib.KG_MAX_B + 1)):
        bv, bi = C.c_double(sentinel), C.c_int64(-7)
        rc = eng.lib.ppbo_kg_envelope(eng.ctx, _ptr(args[0]), _ptr(args[1]), args[2], _ptr(args[3]), _ptr(args[4]), args[5], args[6],
                                      _ptr(kg), _ptr(kinks), C.byref(bv), C.byref(bi), eng._stream())
        assert rc < 0 and eng._err().startswith("invalid argument"), (args[2:], rc, eng._err())
        assert (bv.value, bi.value) == (sentinel, -7)
    torch.cuda.synchronize()
    assert bool((kg == sentinel).all()) and bool((kinks == -7).all()) and all(bool((o == sentinel).all()) for o in outs)
    after = _kg(eng, post, Xa, Xb)
    for k in ("kg", "kinks", "mu_a", "var_a", "mu_b", "var_b"):
        assert np.array_equal(before[k], after[k]), k


def test_profile_name(eng):
    """The envelope launches are timed as "kg", one bracket per chunk, beside the tournament's own."""
    import torch
    mod = _fitted("SE_kernel", 6, None)
    Xa, Xb = _sets(np.random.default_rng(21), mod, 50, 10)
    eng.profile(True)
    try:
        eng.predict_kg(mod["post"], Xa, Xb)
        torch.cuda.synchronize()
        (t, n), (tt, nt) = eng.profile_read("kg"), eng.profile_read("tournament")
    finally:
        eng.profile(False)
    assert (n, nt) == (1, 1) and t > 0.0 and tt > 0.0


# ---------------------------------------------------------------- 6. the GPModel surface
def test_gpmodel_knowledge_gradient():
    from conftest import load_golden
    from test_gpu_pairs import _golden_gp
    gp = _golden_gp(load_golden("rq"))
    np.random.seed(3)
    gp.xstar, gp.mustar, gp.xstars_local = gp.mu_star(mustar_finding_trials=1)
    field = gp.kg_field(24)
    assert field.shape == (24, gp.D) and np.array_equal(field[0], np.asarray(gp.xstar, dtype=float).reshape(-1))
    rng = np.random.default_rng(22)
    X = rng.random((2000, gp.D))
    out = gp.knowledge_gradient(X, field=field)
    assert out["kg"].shape == out["mu"].shape == out["var"].shape == (2000,) and out["field"] is field
    b = out["best_idx"]
    assert b == int(np.argmax(out["kg"])) and np.isfinite(out["kg"][b]) and out["kg"][b] > 0.0
    assert np.array_equal(out["x"], X[b]) and np.all(out["kg"] >= 0.0)
    # the defaults: the resident pool under a fresh rotation, the field of kg_field()
    auto = gp.knowledge_gradient()
    assert auto["field"].shape == (64, gp.D) and np.array_equal(auto["field"][0], field[0])
    assert np.isfinite(auto["kg"][auto["best_idx"]]) and auto["x"].shape == (gp.D,)
    assert np.all((auto["x"] >= 0.0) & (auto["x"] < 1.0))
    # noisier observations teach less
    noisy = gp.knowledge_gradient(X, field=field, noise_var=1e6)
    assert noisy["kg"].max() <= out["kg"].max()
