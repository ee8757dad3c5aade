"""GPU: every pass split, strip pairing, peel residue, ring loop and fold of the one-launch scoring kernel
(csrc/fused.hip, fused_score_kernel) against dense NumPy, on the cases tests/fused_cases.py chooses from the kernel's
launch plan (58 models: 23 that together run every one of the plan's 165 classes of code path, and every n_q of the
workload at m = 25 and m = 31), and the paths the plan does not index: the K* phase in every dimension count, every
candidate count of a ragged block, candidates in every dispatch round, variances at and below zero, and the library's own
transpose of G.

Inputs: the hand-built posteriors of test_gpu_fused.synth_post (random alpha, star-form Lambda, block lower triangular G),
X and candidates uniform in [0, 1]^D, theta = (., 0.6 sqrt(D), 1): K* lies in roughly [0.25, 1] and the contraction term
is as large as sf^2 or larger, so a chunk of G read twice or not at all moves a variance by at least 3e-6 of the bound's
scale (tests/test_fused_cases_host.py::test_every_block_of_G_shows), 10^5 times the bound.  The reference is
fused_cases.reference: K* from direct differences, then dense_reference's expression; it agrees with np.longdouble to
4e-15 of the same scale (test_reference_rounding).

Bound of every comparison with NumPy: |mu - ref| <= 1e-11 max|mu|, |var - ref| <= 1e-11 max_c (sf^2 + |t_c| + q_c) with
t = k*' Lambda k* and q = |G k*|^2 -- the sum of the terms, not |var|, which hand-built Lambda can make cancel.  The score
is compared with acq_numpy.score_value of the GPU's OWN mu and var: EI = d Phi(z) + sd phi(z) is bounded by |d| + sd and
the device's erfc, exp and sqrt are good to a few ulp, so 1e-11 max_c (|d_c| + sd_c); where sd = 0 the score is max(d, 0)
exactly.  Against the three-launch engine: 1e-12 relative in the max norm, as test_gpu_fused.py.

Every checked call is preceded by a call of the same shape on 1 - Xc by the same engine (a freed output tensor, or a
workspace, otherwise comes back holding the right numbers), and asserts through the profile counters that the one-launch
kernel ran once and the three-launch contraction did not.

Largest errors observed on the MI355X over the structure sweep, in units of the scales above (the bound is 1e-11):
    mu  4.75e-15 on N = 258, m = 128, D = 3, Matern-3/2
    var 1.61e-15 on N = 825, m = 32, D = 3, RQ
and at most 9.6e-15 / 1.3e-15 in the other tests of this file.  The file runs in about 4 s.
"""
import ctypes as C

import numpy as np
import pytest

import acq_numpy as an
import fused_cases as fc
from test_gpu_fused import _engine, host, synth_post

pytestmark = pytest.mark.gpu

EI = an.EI
WORST = {"mu": (0.0, None), "var": (0.0, None)}


@pytest.fixture(scope="module")
def engines():
    e = {k: _engine(k) for k in (1, 2, 0)}
    for v in e.values():
        v.profile(True)
    yield e
    for v in e.values():
        v.close()
    print(f"\nfused structure sweep, largest error against NumPy: mu {WORST['mu'][0]:.2e} of max|mu| on {WORST['mu'][1]}, "
          f"var {WORST['var'][0]:.2e} of max(sf2 + |t| + q) on {WORST['var'][1]}")


def checked(eng, post, Xc, fused=True, **kw):
    """One checked call: the poisoning call on 1 - Xc, then the call itself, then the launch counts."""
    Xd, Xp = eng.dev(Xc), eng.dev(1.0 - Xc)
    eng.predict(post, Xp, **kw)
    eng.profile_reset()
    out = eng.predict(post, Xd, **kw)
    assert (eng.profile_read("fused_score")[1], eng.profile_read("quadform")[1]) == ((1, 0) if fused else (0, 1))
    return out


def check_best(out, sc):
    """The best record against the returned scores: first occurrence of the largest."""
    assert out["best_idx"] == int(np.argmax(sc)) and out["best_val"] == sc[out["best_idx"]]


def check_score(mu, var, sc, mustar):
    want = an.score_value(mu, var, EI, mustar)
    d, sd = mu - mustar, np.sqrt(np.maximum(var, 0.0))
    assert np.abs(sc - want).max() <= 1e-11 * (np.abs(d) + sd).max()
    assert np.array_equal(sc[sd == 0.0], np.maximum(d, 0.0)[sd == 0.0])


def check_three_launch(out, out0):
    for k in ("mu", "var", "score"):
        a, b = host(out[k]), host(out0[k])
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), k


def full_check(engines, fused, N, D, m, kernel, seed, Xc, name=None, arrs_edit=None, mustar=None):
    """The checks of the structure sweep for one model on engine `fused`: NumPy, score, best record, three launches.
    Returns (out, arrs, (mu_ref, var_ref, t, q))."""
    th = fc.theta_of(D)
    e, e0 = engines[fused], engines[0]
    p, arrs = synth_post(e, N, D, m, kernel, th, seed=seed)
    p0, _ = synth_post(e0, N, D, m, kernel, th, seed=seed)
    if arrs_edit:
        arrs_edit(arrs)
        for post, eng in ((p, e), (p0, e0)):
            post.lam_diag = eng.dev(arrs["lam_diag"])
    ref = fc.reference(arrs, Xc, kernel, th, m)
    mu_ref, var_ref, t, q = ref
    s_mu, s_var = fc.scales(th, mu_ref, t, q)
    mustar = float(np.median(mu_ref)) if mustar is None else mustar
    out = checked(e, p, Xc, score=EI, mustar=mustar, want_score=True)
    mu, var, sc = host(out["mu"]), host(out["var"]), host(out["score"])
    e_mu, e_var = np.abs(mu - mu_ref).max() / s_mu, np.abs(var - var_ref).max() / s_var
    print(f"{name or (N, D, m, kernel)}: mu {e_mu:.2e} var {e_var:.2e}")
    if name:
        for k, v in (("mu", e_mu), ("var", e_var)):
            if v > WORST[k][0]:
                WORST[k] = (v, name)
    assert e_mu <= 1e-11 and e_var <= 1e-11
    check_score(mu, var, sc, mustar)
    check_best(out, sc)
    check_three_launch(out, checked(e0, p0, Xc, fused=False, score=EI, mustar=mustar, want_score=True))
    return out, arrs, ref


# ---- 1. the structure sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_structure_sweep(engines, c):
    full_check(engines, fc.engine_of(c), c.N, c.D, c.m, c.kernel, c.seed, fc.candidates(c), name=fc.case_id(c))


# ---- 2. the K* phase ----------------------------------------------------------------------------------------------------
# one single-pass model, N = 48 = three stars of 16 rows: D = 1 .. 16 is one round of operand loads with 1 - 4 k-steps, the
# last one partial unless D % 4 == 0 (the select on the B operand); D > 16 (PPBO_FUSED=2) two to four rounds
@pytest.mark.parametrize("D", list(range(1, 17)) + [17, 20, 31, 32, 33, 47, 48, 49, 64])
def test_kstar_phase_every_dimension_count(engines, D):
    for i, kernel in enumerate(fc.KERNELS):
        Xc = np.random.default_rng(7000 + 10 * D + i).random((fc.M_CASE, D))
        full_check(engines, 1 if D <= fc.D_DEFAULT_MAX else 2, 48, D, 15, kernel, 7100 + 10 * D + i, Xc)


@pytest.mark.parametrize("kernel", ["Matern52_kernel", "Matern32_kernel"])
def test_kstar_phase_matern_two_passes(engines, kernel):
    """Two passes with both panels ragged: rows behind either pass's rows are staged with |x|^2 = 1e300 and must come out
    of the Matern tail as exact zeros (matern_ae's cap), in the mean, in Lambda's part and in the panel the contraction
    reads.  N = 299 = 23 stars of 13: R1 = 247, 52 rows in pass 2."""
    assert (fc.plan(299, 12).NW, fc.plan(299, 12).R1) == (8, 247)
    Xc = np.random.default_rng(7900).random((fc.M_CASE, 5))
    full_check(engines, 1, 299, 5, 12, kernel, 7901, Xc)


# ---- 3. candidate counts ------------------------------------------------------------------------------------------------
def test_every_candidate_count_of_a_ragged_block(engines):
    """M = 1 .. 65 on a two-pass 8-wavefront model: the first M rows of the M = 65 call, bit for bit."""
    N, D, m, kernel, th = 338, 3, 25, "SE_kernel", fc.theta_of(3)
    assert fc.plan(N, m).NW == 8 and fc.plan(N, m).passes == 2
    Xc = np.random.default_rng(8000).random((65, D))
    full, arrs, ref = full_check(engines, 1, N, D, m, kernel, 8001, Xc)
    mustar = float(np.median(ref[0]))
    e = engines[1]
    p, _ = synth_post(e, N, D, m, kernel, th, seed=8001)
    want = {k: host(full[k]) for k in ("mu", "var", "score")}
    for M in range(1, 66):
        out = checked(e, p, Xc[:M], score=EI, mustar=mustar, want_score=True)
        for k in want:
            assert np.array_equal(host(out[k]), want[k][:M]), (M, k)
        check_best(out, want["score"][:M])


def test_a_candidate_scores_the_same_wherever_it_sits(engines):
    """3 x 8192 + 5 candidates, the same 64 rows repeated: blocks in every dispatch round (the odd rounds start late) and
    both column tiles of each.  Every repeat carries the bits of its first copy; the best record names the first copy."""
    N, D, m, kernel, th = 338, 3, 25, "RQ_kernel", fc.theta_of(3)
    rows = np.random.default_rng(8100).random((64, D))
    M = 3 * 8192 + 5
    Xc = np.tile(rows, (M // 64 + 1, 1))[:M]
    first, arrs, ref = full_check(engines, 1, N, D, m, kernel, 8101, rows)
    e = engines[1]
    p, _ = synth_post(e, N, D, m, kernel, th, seed=8101)
    out = checked(e, p, Xc, score=EI, mustar=float(np.median(ref[0])), want_score=True)
    for k in ("mu", "var", "score"):
        got, one = host(out[k]), host(first[k])
        assert np.array_equal(got, np.tile(one, M // 64 + 1)[:M]), k
    assert 0 <= out["best_idx"] < 64
    check_best(out, host(out["score"]))
    assert (out["best_idx"], out["best_val"]) == (first["best_idx"], first["best_val"])


# ---- 4. variances at and below zero --------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["all-negative", "straddling"])
@pytest.mark.parametrize("where", ["below", "inside", "above"])
def test_zero_and_negative_variance(engines, how, where):
    """lam_diag scaled until var <= 0 for every candidate, or for about half of them: var comes back unclipped, and EI takes
    the branch sd == 0 -> max(d, 0) there -- with mustar below, inside and above the means."""
    N, D, m, kernel, th = 260, 3, 25, "SE_kernel", fc.theta_of(3)
    Xc = np.random.default_rng(8200).random((fc.M_CASE, D))
    _, arrs = synth_post(fc._HostEngine(), N, D, m, kernel, th, seed=8201)
    mu0, var0, t0, q0 = fc.reference(arrs, Xc, kernel, th, m)
    ks = fc.kstar(arrs["X"], Xc, kernel, th)
    t_diag = (arrs["lam_diag"][:, None] * ks * ks).sum(axis=0)              # < 0: lam_diag is negative
    zero_at = 1.0 + (var0 / -t_diag)                                         # the scale of lam_diag at which var_c = 0
    scale = 2.0 * zero_at.max() if how == "all-negative" else float(np.median(zero_at))
    mustar = {"below": mu0.min() - 1.0, "inside": float(np.median(mu0)), "above": mu0.max() + 1.0}[where]

    def edit(a):
        a["lam_diag"] = a["lam_diag"] * scale

    out, _, (mu_ref, var_ref, _, _) = full_check(engines, 1, N, D, m, kernel, 8201, Xc, arrs_edit=edit, mustar=float(mustar))
    var, sc, mu = host(out["var"]), host(out["score"]), host(out["mu"])
    if how == "all-negative":
        assert (var_ref < 0.0).all() and (var < 0.0).all()
        assert np.array_equal(sc, np.maximum(mu - mustar, 0.0))
    else:
        assert 20 <= (var_ref < 0.0).sum() <= 45 and np.array_equal(var < 0.0, var_ref < 0.0)
        assert np.array_equal(sc[var <= 0.0], np.maximum(mu - mustar, 0.0)[var <= 0.0])
    if where == "above" and how == "all-negative":
        assert not sc.any() and (out["best_idx"], out["best_val"]) == (0, 0.0)


# ---- 5. the library's own transpose ---------------------------------------------------------------------------------------
def test_the_librarys_own_transpose_of_G(engines):
    """ppbo_model.d_Gt = NULL (a C caller that formed no transpose): ppbo_fused_transposed_G builds it per call in a ctx
    workspace.  After a 512-row model has used that workspace, a 286-row model (ragged in every direction: N % 16 = 14)
    gives the bits of the d_Gt path."""
    from ppbo_amd.engine import _ptr
    e = engines[1]
    M = fc.M_CASE

    def raw(post, Xd, with_gt):
        md = e._model(post, True)
        assert md.d_Gt
        if not with_gt:
            md.d_Gt = 0
        mu, var, sc = e.empty(M), e.empty(M), e.empty(M)
        bv, bi = C.c_double(0.0), C.c_int64(-1)
        e.profile_reset()
        rc = e.lib.ppbo_predict(e.ctx, C.byref(md), _ptr(Xd), M, EI, 0.1, _ptr(mu), _ptr(var), _ptr(sc), C.byref(bv),
                                C.byref(bi), e._stream())
        assert rc == 0 and e.profile_read("fused_score")[1] == 1
        return host(mu), host(var), host(sc), bv.value, bi.value

    big, _ = synth_post(e, 512, 3, 31, "SE_kernel", fc.theta_of(3), seed=8300)
    Xb = np.random.default_rng(8301).random((M, 3))
    got_big = raw(big, e.dev(Xb), False)
    small, arrs = synth_post(e, 286, 3, 25, "RQ_kernel", fc.theta_of(3), seed=8302)
    Xs = np.random.default_rng(8303).random((M, 3))
    raw(small, e.dev(1.0 - Xs), False)                                      # the poisoning call
    got = raw(small, e.dev(Xs), False)
    want = raw(small, e.dev(Xs), True)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for a, b in zip(got_big, raw(big, e.dev(Xb), True)):
        assert np.array_equal(a, b)
    mu_ref, var_ref, t, q = fc.reference(arrs, Xs, "RQ_kernel", fc.theta_of(3), 25)
    s_mu, s_var = fc.scales(fc.theta_of(3), mu_ref, t, q)
    assert np.abs(got[0] - mu_ref).max() <= 1e-11 * s_mu and np.abs(got[1] - var_ref).max() <= 1e-11 * s_var
