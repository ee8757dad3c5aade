"""Host: the launch plan of tests/fused_cases.py -- that its case list reaches every code path the plan tells apart, that
the constants it rests on are the ones in ppbo_amd/csrc/fused.hip (read as text), that the plan is coherent (every row of
G is folded once, every K range reaches the end of its strip's last star and stays inside the transposed operand), and
that the inputs of tests/test_gpu_fused_structure.py make the check there a sharp one: the float64 reference is exact to
1e-13 of the bound's scale, and no 16 x 16 block of G can be skipped or doubled without moving a variance by 1e-6 of it,
10^5 times the bound the GPU is held to."""
import os
import re

import numpy as np
import pytest

import fused_cases as fc

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "ppbo_amd", "csrc", "fused.hip")


def source():
    with open(SOURCE) as fh:
        return fh.read()


def body(text, head):
    """The text of the function whose definition begins with `head`, up to its closing brace in column 0."""
    beg = text.index(head)
    return text[beg:text.index("\n}\n", beg)]


# ---- coverage -------------------------------------------------------------------------------------------------------------
def test_the_enumeration():
    shapes = fc.accepted()
    assert len(shapes) == len(set(shapes)) == 5536
    forms = [fc.form_of(N, mblk - 1)[0] for N, mblk in shapes]
    assert forms.count(8) == 2420 and forms.count(16) == 3116
    assert max(N for N, _ in shapes) == 1024 and max(b for _, b in shapes) == 512
    # the three-launch form's own: a second pass that fits no panel, a star that fits none
    assert fc.plan(1040, 25) is None and fc.plan(1026, 512) is None and fc.plan(520, 25).NW == 16


def test_the_covering_set_reaches_every_class():
    """Recomputed from the enumeration: a case dropped from COVER, or a class added to the plan, fails here."""
    want = fc.all_classes()
    got = set().union(*(fc.classes(N, mblk - 1) for N, mblk in fc.COVER))
    before = set().union(*(fc.classes(N, mblk - 1) for N, mblk in fc.BEFORE))
    everything = set().union(*(fc.classes(c.N, c.m) for c in fc.CASES))
    print(f"fused_score_kernel: {len(want)} classes over {len(fc.accepted())} shapes; the {len(fc.BEFORE)} shapes of "
          f"test_gpu_fused.py reach {len(before & want)}, the {len(fc.COVER)} covering shapes {len(got & want)}, "
          f"all {len(fc.CASES)} cases {len(everything & want)}")
    assert got == want, sorted(want - got, key=str)
    assert before < want                       # the gap this list closes
    assert len(fc.COVER) == len(set(fc.COVER)) and set(fc.COVER) <= set(fc.accepted())
    assert len(fc.COVER) <= len(fc.greedy_cover())     # no longer than a fresh greedy pass


def test_the_classification_tells_apart_what_it_must():
    """The paths named one by one when the gap was found, each as a class (or a conjunction of classes) of its own."""
    allc = fc.all_classes()
    named = [
        (8, "lower", "pair", 1, 0),            # a lower pair of one chunk: the peel, no loop
        (8, "lower", "strip", 1, 0),           # a lone lower strip, residue 1, no loop
        (8, "lower", "strip", 2, 1), (8, "lower", "strip", 3, 1),           # residues 2 and 3 followed by the loop
        (8, "upper1", "strip", 0, 2), (8, "upper1", "strip", 1, 2), (8, "upper1", "strip", 2, 2),   # the four-deep loop runs
        (8, "upper2", "pair", 1, 0),           # the pass-2 upper pair of one chunk
        (8, "upper2", "strip", 1, 0), (8, "upper2", "strip", 2, 1), (8, "upper2", "strip", 3, 1),
        (8, "upper2", "tail", 3, 1),           # the pass-2 tail with residue 3
        (8, "stars", "16"),                    # stars coincide with tiles
        (16, "lower", "strip", 1, 1), (16, "lower", "strip", 2, 1), (16, "lower", "strip", 3, 1), (16, "lower", "strip", 0, 1),
        (16, "upper2", "tail", 1, 0), (16, "upper2", "tail", 3, 0), (16, "upper2", "tail", 1, 1),
        (16, "upper2", "fold", "b", "masked"),  # the masked fold of the long upper strip
        (16, "passes", 1),                     # the single-pass launch, 256 < N <= 512
        (16, "stars", "<16"), (16, "stars", "16"), (16, "stars", "33..KP/2"), (16, "stars", ">KP/2"),
    ]
    assert set(named) <= allc, sorted(set(named) - allc, key=str)
    before = set().union(*(fc.classes(N, mblk - 1) for N, mblk in fc.BEFORE))
    assert not set(named) & before            # none of them ran
    pl = fc.plan(257, 256)
    assert (pl.NW, pl.R1, pl.passes) == (16, 257, 1)
    assert fc.plan(512, 31).NW == 8 and fc.plan(512, 31).R1 == 256 and fc.plan(528, 15).NW == 16


def test_the_case_list():
    ids = [fc.case_id(c) for c in fc.CASES]
    assert len(ids) == len(set(ids))
    shapes = {(c.N, c.m + 1) for c in fc.CASES}
    assert shapes == set(fc.COVER) | set(fc.WORKLOAD)
    # every n_q of the workload at m = 25 and m = 31: 35 models.  All but N = 494 take the default 8-wavefront form (at
    # n_q = 19, m = 25 the second pass has 260 rows: the 16-wavefront form); each runs on the engine that takes it
    assert len(fc.WORKLOAD) == 35 and {N for N, b in fc.WORKLOAD if b == 26} == set(range(26, 495, 26))
    assert {N for N, b in fc.WORKLOAD if b == 32} == set(range(32, 513, 32))
    assert [s for s in fc.WORKLOAD if fc.form_of(s[0], s[1] - 1)[0] != 8] == [(494, 26)]
    for c in fc.CASES:
        NW = fc.form_of(c.N, c.m)[0]
        assert NW in (8, 16) and fc.engine_of(c) == (1 if NW == 8 and c.D <= 16 else 2)
        assert c.D in (3, 16) and c.kernel in fc.KERNELS
    assert 3 <= sum(c.D == 16 for c in fc.CASES) <= 10
    for NW in (8, 16):                         # every kernel family in two-pass launches of either form
        assert {c.kernel for c in fc.CASES if fc.plan(c.N, c.m).passes == 2 and fc.plan(c.N, c.m).NW == NW} == set(fc.KERNELS)


# ---- the plan against itself: every shape the kernel accepts -----------------------------------------------------------------
def test_every_plan_is_coherent():
    """Rows: the folds of a plan take every row of G below N exactly once (a whole fold 16 rows, a masked one the rows
    below its limit).  K ranges: a strip's chunks reach the end of the last star that has a row in it -- nothing of the
    block-triangular support is left out -- a lower strip's end inside pass 1's panel, an upper strip's inside pass 2's,
    and no chunk reads the transposed operand beyond its (N rounded up to 16) + 16 rows, or the panel beyond KP + 4."""
    for N, mblk in fc.accepted():
        pl = fc.plan(N, mblk - 1)
        NW, KP, R1 = pl.NW, pl.KP, pl.R1
        assert (R1 == N) == (pl.passes == 1) and R1 % mblk == 0 and 0 < R1 <= KP and fc.up16(N - R1) <= KP
        rows_t = fc.up16(N) + 16
        seen = np.zeros(N, dtype=int)
        for s in pl.strips:
            base, hi, P0 = (0, R1, 0) if s.kind == "lower" else (R1, N, 0 if s.kind == "upper1" else R1)
            for r0, n, f in ((base + 16 * s.wave, s.na, s.fold_a), (base + 16 * (2 * NW - 1 - s.wave), s.nb, s.fold_b)):
                if n == 0:
                    assert f is None
                    continue
                assert r0 < hi
                last = min(r0 + 16, hi)
                kend = -(-last // mblk) * mblk
                if s.kind == "upper1":
                    assert 16 * n == fc.up16(R1) and f is None
                else:
                    assert P0 + 16 * n >= kend > P0 + 16 * (n - 1) and (f == "whole") == (r0 + 16 <= hi)
                    seen[r0:last] += 1
                assert P0 + 16 * n <= rows_t and 16 * n <= KP                # the operand's rows; the panel's (+ 4 of slack)
                assert r0 + 32 <= ((N + 31) & ~31) + 32                      # ... and its columns: a strip reads 32
        assert (seen == 1).all(), (N, mblk)


# ---- the constants, from the source text -------------------------------------------------------------------------------------
def test_the_constants_are_the_kernels():
    text = source()
    assert re.search(r"^constexpr int FS_BN = (\d+);", text, re.M).group(1) == str(fc.FS_BN)
    assert re.search(r"^constexpr int FS_LD = (\d+);", text, re.M).group(1) == "36"
    kern = body(text, "__global__ __launch_bounds__(64 * NW, 4) void fused_score_kernel(")
    assert re.findall(r"constexpr int KP = (\d+) \* NW\b", kern) == ["32"]
    assert "const int ra = 16 * wave, rb = 16 * (2 * NW - 1 - wave);" in kern
    assert "const int ra = R1 + 16 * wave, rb = R1 + 16 * (2 * NW - 1 - wave);" in kern
    split = body(text, "static int fused_split(int N, int mblk, int KP)")
    for line in ("if (((N + 15) & ~15) <= KP) return N;", "const int R1 = (KP / mblk) * mblk;", "if (R1 <= 0) return -1;",
                 "if (((N - R1 + 15) & ~15) > KP) return -1;"):
        assert line in split, line
    launch = body(text, "int fused_launch(ppbo_ctx* ctx, FusedArgs& a, hipStream_t s)")
    assert re.findall(r"fused_split\(a\.N, a\.mblk, (\d+)\)", launch) == [str(fc.PANELS[8]), str(fc.PANELS[16])]
    assert re.findall(r"constexpr int NW = (\d+);", launch) == ["8", "16"]
    assert launch.index("fused_split(a.N, a.mblk, 256)") < launch.index("NW = 8") < launch.index("NW = 16")
    for NW, KP in fc.PANELS.items():
        assert KP == 32 * NW
    elig = body(text, "bool ppbo_fused_eligible(const ppbo_ctx* ctx, const ppbo_model* m)")
    assert "if (fused_split(m->N, m->m + 1, 256) >= 0 && m->D <= 16) return true;" in elig
    assert sorted(re.findall(r"fused_split\(m->N, m->m \+ 1, (\d+)\)", elig)) == ["256", "256", "512"]
    assert re.findall(r"D <= (\d+)", elig) == [str(fc.D_DEFAULT_MAX)]
    form = body(text, 'extern "C" int ppbo_posterior_form(')
    assert re.findall(r"D <= (\d+) && fused_split\(N, m \+ 1, (\d+)\)", form) == [(str(fc.D_DEFAULT_MAX), str(fc.PANELS[8]))]


def test_a_moved_constant_is_noticed():
    """The same reads on an edited text: a 384-row panel in fused_launch, D <= 20 in the eligibility rule."""
    text = source()
    moved = text.replace("fused_split(a.N, a.mblk, 256)", "fused_split(a.N, a.mblk, 384)")
    launch = body(moved, "int fused_launch(ppbo_ctx* ctx, FusedArgs& a, hipStream_t s)")
    assert re.findall(r"fused_split\(a\.N, a\.mblk, (\d+)\)", launch) != ["256", "512"]
    moved = text.replace("m->D <= 16", "m->D <= 20")
    assert re.findall(r"D <= (\d+)", body(moved, "bool ppbo_fused_eligible(")) == ["20"]


# ---- the inputs: a sharp check ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def states():
    cache = {}

    def get(c):
        if c not in cache:
            arrs, Xc, th = fc.host_state(c), fc.candidates(c), fc.theta_of(c.D)
            cache[c] = (arrs, Xc, th, fc.reference(arrs, Xc, c.kernel, th, c.m))
        return cache[c]

    return get


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_reference_rounding(states, c):
    """float64 against the same expression in np.longdouble: 1e-13 of the bound's scale (measured: at most 4e-15)."""
    assert np.finfo(np.longdouble).eps < 1e-18
    arrs, Xc, th, (mu, var, t, q) = states(c)
    mu_l, var_l, _, _ = fc.reference(arrs, Xc, c.kernel, th, c.m, dtype=np.longdouble)
    s_mu, s_var = fc.scales(th, mu, t, q)
    e_mu, e_var = float(np.abs(mu - mu_l).max()) / s_mu, float(np.abs(var - var_l).max()) / s_var
    print(f"{fc.case_id(c)}: float64 against longdouble mu {e_mu:.1e} var {e_var:.1e}")
    assert e_mu <= 1e-13 and e_var <= 1e-13
    ks = fc.kstar(arrs["X"], Xc, c.kernel, th)
    assert 0.2 <= ks.min() and ks.max() <= 1.0 + 1e-15          # K* in roughly [0.25, 1]: the contraction cannot drown
    assert q.max() >= th[2] ** 2


@pytest.mark.parametrize("c", fc.CASES, ids=fc.case_id)
def test_every_block_of_G_shows(states, c):
    """Zeroing any one 16 x 16 block of G that meets the block-triangular support moves some candidate's variance by more
    than 1e-6 of the bound's scale (measured: at least 3.2e-6, N = 257 with one star)."""
    arrs, Xc, th, (mu, var, t, q) = states(c)
    ks = fc.kstar(arrs["X"], Xc, c.kernel, th)
    moved = fc.block_sensitivity(arrs, ks, c.m) / fc.scales(th, mu, t, q)[1]
    nb = -(-c.N // 16)
    assert len(moved) >= nb * (nb + 1) // 2
    print(f"{fc.case_id(c)}: {len(moved)} blocks, least visible {moved.min():.1e} of the scale")
    assert moved.min() > 1e-6
    # the closed form above is the dense computation: one block, zeroed for real
    i, j = 16 * ((c.N - 1) // 16), 0
    G2 = arrs["G"].copy()
    G2[i:i + 16, j:j + 16] = 0.0
    q2 = fc.reference(arrs, Xc, c.kernel, th, c.m, G=G2)[3]
    pick = moved[(c.N - 1) // 16]                               # block column 0 comes first, its rows in order
    assert abs(np.abs(q2 - q).max() / fc.scales(th, mu, t, q)[1] - pick) <= 1e-12


def test_the_reference_is_dense_reference_with_direct_differences():
    """For the kernels the oracle has (its expansion-form distances): the two references agree to rounding."""
    from test_gpu_fused import dense_reference
    for c in [c for c in fc.CASES if c.kernel in ("SE_kernel", "RQ_kernel")][:6]:
        arrs, Xc, th = fc.host_state(c), fc.candidates(c), fc.theta_of(c.D)
        mu, var, t, q = fc.reference(arrs, Xc, c.kernel, th, c.m)
        mu_d, var_d = dense_reference(arrs, Xc, c.kernel, th, c.m)
        s_mu, s_var = fc.scales(th, mu, t, q)
        assert np.abs(mu - mu_d).max() <= 1e-13 * s_mu and np.abs(var - var_d).max() <= 1e-13 * s_var
