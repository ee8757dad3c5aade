"""GPU: every entry on a USED context against the same call on a fresh one.

A ppbo_ctx owns 37 workspace slots that only grow and are never cleared, and the kernels read more of them than a call
writes (K* padded to whole 128-candidate tiles, K ranges rounded up to 16-column chunks, G copied into a zero frame, slabs
and per-block records sized for the largest chunk).  The library promises that "a ctx owns only private workspaces; the
library has no process-global mutable state" and documents its entries as bitwise repeatable, so the same call must
return the same bits whatever the context ran before.  For every checked call c of tests/used_context_cases.py and every
history h, h and then c run on one engine; every output array and host scalar of c must equal, bit for bit
(np.array_equal(..., equal_nan=True) on a non-empty array), those of c on a fresh engine:

  larger      the same entry, strictly larger in every sizing dimension, another tile count, the other operator form and
              another kernel family where the entry takes them
  nonfinite   that larger call with inputs that leave NaN / Inf in the intermediate buffers (each documented as accepted,
              CASES[name].doc; an expected error return is caught)
  smaller     the smallest legal sizes first, so that every slot regrows during the checked call beside an older allocation
  neighbours  one fixed sequence of all checked calls that interleaves the families sharing WS_SMALL, WS_VEC, WS_LINALG,
              WS_PART, WS_KSTAR and WS_TRANSPOSE, run twice through on one engine; every call of the second pass is compared

The used engine's output buffers are handed over filled with NaN (poison_outputs), so that an output the library promises
but leaves unwritten cannot pass on what the allocator happened to return.

Two controls keep the comparison honest: the call on two fresh engines agrees bit for bit (test_fresh_engines_agree; no
entry failed it, so NOT_REPEATABLE is empty and no entry is compared at a tolerance), and the fresh engine's result is
held against the NumPy twin the project already has at the tolerance of the entry's own test file
(test_fresh_engine_matches_the_numpy_twin), so that a fresh engine on dirty memory cannot make a wrong reference.

Left out: ppbo_dist_*, ppbo_argmax_allgather* and ppbo_search_sharded* (they need several ranks; tests/test_gpu_sharded.py
and tests/test_gpu_dist.py own them), randn and store_floor (no workspace).

The slots (csrc/common.h), and the checked calls that request each, from reading the code:

  WS_KSTAR          predict*, predict_record, predict_cov, prune_*, projected_predict, pairs, slopes, curvatures*, gradients,
                    functionals, marginals_*, tournament_*, search_batch, line_acq*, line_choice
  WS_PART           the same scoring, predictor and line calls; rff_score; mean_search_multi_*, mean_search_boxes
  WS_SCRATCH        T_and_grad, fit_fmap_*, gp_fit
  WS_LINALG         pd_inverse*, lu / laplace_logdet, evidence_grad, fit_fmap_*, gp_fit, posterior_* (and through them
                    prune_*, projected_predict)
  WS_LINALG2        pd_inverse* (the triangular inverse), gp_fit, posterior_*
  WS_VEC            regularize_covariance, dgemv, lu_slogdet_*, laplace_logdet, evidence_grad, laplace_terms,
                    fit_fmap_whitened, gp_fit, rff_omega_map
  WS_SMALL          predict* (block records), every predictor, line_*, rff_score, potrf, pd_inverse*, pd_inverse_append,
                    fit_fmap_*, gp_fit, posterior_*
  WS_POTRF          potrf, pd_inverse*, fit_fmap_*, gp_fit, posterior_*
  WS_APPEND         pd_inverse_append
  WS_DIST           none: ppbo_dist_* / ppbo_argmax_allgather* / ppbo_search_sharded* only (left out above)
  WS_LBFGS, WS_LBFGS_U   fit_fmap_whitened, gp_fit
  WS_SEARCH         mean_search_multi_*, mean_search_boxes, rff_search*, path_search_multi; line_* (the grid of the _xi form)
  WS_SEARCH_SMALL   shift_points, rff_omega_map, mean_search_multi_*
  WS_TRANSPOSE      mean_ascent*, mean_search_*, mean_ard_B, mean_camphor_B, rff_search*, path_search_multi
  WS_GPAD           predict3_*_2050, pairs_B2050, prune_* (the zero-framed copy of G from 2048 candidates on)
  WS_SEARCH_ROWS    mean_search_multi_*, mean_search_boxes
  WS_SCALE, WS_SCALE_SEARCH   mean_ard_B (the scaled coordinate map: its coefficients and the mapped rows)
  WS_SCALE_PTS      scale_points
  WS_EVGRAD, WS_EVGRAD_VEC   evidence_grad
  WS_CAMPHOR, WS_CAMPHOR_ROWS   mean_camphor_B (the camphor coordinate map: the embedded points and rows)
  WS_KSTAR_GEO      predict*, the predictors (the star geometry of the K* pass)
  WS_MARGINAL       marginals_*
  WS_TOURN_U, WS_TOURN_FIELD   tournament_*, search_batch
  WS_TOURN_K        tournament_*
  WS_PROJECT, WS_PROJECT_SMALL   projected_predict
  WS_PRUNE, WS_PRUNE_KC   prune_thin, prune_tile, and the edge-form predict_*_B cases on the three-launch path
  WS_BATCH, WS_BATCH_K   search_batch
  WS_BOX            mean_ascent_boxes, mean_search_boxes
  WS_BOX_SURV       mean_search_boxes
"""
import os

import numpy as np
import pytest

import used_context_cases as uc

pytestmark = pytest.mark.gpu

NAMES = list(uc.CASES)
HISTORIES = ("larger", "nonfinite", "smaller")
NOT_REPEATABLE = ()        # entries that failed the fresh-against-fresh control (at most 3 allowed; none did)


def make_engine(env=()):
    """A fresh Engine whose ctx reads the given PPBO_* settings (they are read once, at ppbo_ctx_create)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import Engine
    env = dict(env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def poison_outputs(eng):
    """From here on the engine hands the library output buffers filled with NaN in place of uninitialised ones (Engine.empty
    is torch.empty: a caller's buffer is whatever the allocator returns).  An output element the library promises but
    does not write -- the zeros above the diagonal of a triangular inverse, say -- then differs from the fresh engine's
    whatever the allocator happened to hand out there."""
    import torch
    eng.empty = lambda *shape: torch.full(tuple(shape), float("nan"), dtype=torch.float64, device=eng.device)


def close(eng):
    import torch
    torch.cuda.synchronize()
    eng.close()


_FRESH = {}


def fresh(name, which=0):
    """The checked call on a fresh engine (which = 1: on a second one, whose output buffers start as NaN), computed once and
    never written to."""
    if (name, which) not in _FRESH:
        case = uc.CASES[name]
        eng = make_engine(case.env)
        if which:
            poison_outputs(eng)
        try:
            out = case.run(eng, "checked")
        finally:
            close(eng)
        for a in out.values():
            a.setflags(write=False)
        _FRESH[name, which] = out
    return _FRESH[name, which]


def differences(got, want):
    """The outputs that are not the same bits (or are empty, or missing)."""
    bad = [k for k in want if k not in got or np.asarray(got[k]).size == 0 or
           not np.array_equal(got[k], want[k], equal_nan=True)]
    return bad + [k for k in got if k not in want]


def worst(got, want, keys):
    return {k: float(np.nanmax(np.abs(np.asarray(got[k], dtype=float) - np.asarray(want[k], dtype=float))))
            for k in keys if k in got and np.shape(got[k]) == np.shape(want[k])}


def run_history(eng, case, history):
    """The history on the used engine; the documented error returns of a non-finite input are caught."""
    if history != "nonfinite":
        case.run(eng, history)
        return
    try:
        case.run(eng, history)
    except RuntimeError:          # (NotPositiveDefinite is one)
        pass


@pytest.mark.parametrize("name", NAMES)
def test_fresh_engines_agree(name):
    """Control 1: the call on two fresh engines, bit for bit, before any history runs."""
    a, b = fresh(name, 0), fresh(name, 1)
    bad = differences(b, a)
    assert not bad, (name, bad, worst(b, a, bad))


@pytest.mark.parametrize("name", NAMES)
def test_fresh_engine_matches_the_numpy_twin(name):
    """Control 2: the fresh engine's result against the entry's NumPy twin, at the tolerance of the entry's own test file."""
    uc.CASES[name].ref(fresh(name))


@pytest.mark.parametrize("history", HISTORIES)
@pytest.mark.parametrize("name", NAMES)
def test_a_history_does_not_change_the_call(name, history):
    case = uc.CASES[name]
    want = fresh(name)
    eng = make_engine(case.env)
    try:
        run_history(eng, case, history)
        poison_outputs(eng)
        got = case.run(eng, "checked")
    finally:
        close(eng)
    if name in NOT_REPEATABLE:
        case.ref(got)
        return
    bad = differences(got, want)
    assert not bad, (name, history, bad, worst(got, want, bad))


@pytest.mark.parametrize("env", uc.envs(), ids=lambda e: "-".join(f"{k}={v}" for k, v in e) or "default")
def test_neighbours_do_not_change_the_calls(env):
    """Every checked call of one engine setting in the interleaved order, twice through on ONE engine: each call of the
    second pass against its fresh engine."""
    seq = uc.neighbours(env)
    want = {name: fresh(name) for name in seq}
    eng = make_engine(env)
    failed = []
    try:
        for name in seq:
            uc.CASES[name].run(eng, "checked")
        poison_outputs(eng)
        for name in seq:
            got = uc.CASES[name].run(eng, "checked")
            bad = [] if name in NOT_REPEATABLE else differences(got, want[name])
            if bad:
                failed.append((name, bad, worst(got, want[name], bad)))
    finally:
        close(eng)
    assert not failed, failed
