"""The launch plan of the one-launch scoring kernel (ppbo_amd/csrc/fused.hip), stated on the host -- test infrastructure
only, no device input, importable without torch.

For a model of N = n_q (m + 1) rows `plan(N, m)` says what the head comment of fused.hip promises and what
fused_score_kernel then does, wavefront by wavefront, by the same integer arithmetic on (N, m + 1):

    form      8 wavefronts with a 256-row panel (fused_split(N, m + 1, 256) >= 0), else 16 wavefronts with a 512-row panel,
              else None (the three-launch form)
    R1        rows of the first pass: N when one panel holds every row, else the last star boundary inside the panel
    strips    per pass and wavefront w the two strips of 16 rows it owns -- a = w (short K range), b = 2 NW - 1 - w (long),
              counted from row 0 (lower, pass 1), from R1 with pass 1's K range (upper, pass 1) or from R1 with the rest of
              the K range (upper, pass 2) -- the routine they run through (fs_pair, fs_pair and fs_strip on the rest of b,
              fs_strip alone, or nothing), their chunk counts (16 K rows each), and how `fold` takes each finished strip
              (whole, or masked at R1 / N)
    K* tiles  per pass the 16-row tiles of the panel: full, ragged (the pass's rows end inside), or behind them

`classes(N, m)` turns a plan into the set of code paths it runs: a routine with its peel residue (fs_pair: chunks & 1,
fs_strip: chunks & 3) and how often its unrolled loop runs (0, 1 = every refill clamped at the strip's end, 2 = also an
iteration whose refills all advance), a fold, an idle wavefront, a K* tile kind, the pass count, the star size against
the 16-row tile.  The plan only CHOOSES cases and proves that they cover: the oracle of tests/test_gpu_fused_structure.py
is dense NumPy (`reference` below), never this module.  It must be kept in step with fused.hip;
tests/test_fused_cases_host.py reads the constants it rests on from the source text.

The case list: COVER, a greedy cover (small N first) of every class that occurs among all shapes the kernel accepts, and
WORKLOAD, every n_q the default form takes at m = 25 (N = 26 .. 494) and m = 31 (N = 32 .. 512)."""
from __future__ import annotations

import collections
import functools

import numpy as np

FS_BN = 32                      # candidates per workgroup
PANELS = {8: 256, 16: 512}      # wavefronts per workgroup -> rows of the K* panel (KP = 32 NW)
D_DEFAULT_MAX = 16              # the default engine (PPBO_FUSED=1) takes D <= 16
MBLK_MAX = 512                  # a star of more rows fits no panel


def up16(n):
    return (n + 15) & ~15


def fused_split(N, mblk, KP):
    """fused.hip's fused_split: rows of the first pass, N when one pass holds every row, -1 when two passes do not do."""
    if up16(N) <= KP:
        return N
    R1 = (KP // mblk) * mblk
    if R1 <= 0 or up16(N - R1) > KP:
        return -1
    return R1


def form_of(N, m):
    """(NW, R1) of fused_launch, or (None, -1)."""
    for NW, KP in PANELS.items():
        R1 = fused_split(N, m + 1, KP)
        if R1 >= 0:
            return NW, R1
    return None, -1


Strips = collections.namedtuple("Strips", "kind wave routine na nb fold_a fold_b")
# kind: "lower" | "upper1" | "upper2";  routine: "idle" | "strip" | "pair" | "pair+tail";  na, nb: chunks of strips a and b
# (nb = 0: no strip b);  fold_a, fold_b: "whole" | "masked" | None (no fold: no strip, or the upper strips in pass 1)
Plan = collections.namedtuple("Plan", "N m NW KP R1 passes strips ktiles")


def _kend_chunks(r0, hi, mblk, P0):
    """chunks from K row P0 to the end of the last star that reaches into the strip [r0, min(r0 + 16, hi))."""
    last = min(r0 + 16, hi)
    kend = -(-last // mblk) * mblk
    return up16(kend - P0) >> 4


def _fold(r0, hi):
    return "whole" if r0 + 16 <= hi else "masked"


def plan(N, m):
    mblk = m + 1
    assert m >= 1 and N > 0 and N % mblk == 0
    NW, R1 = form_of(N, m)
    if NW is None:
        return None
    KP = PANELS[NW]
    strips = []
    span = up16(R1)
    for w in range(NW):
        ra, rb = 16 * w, 16 * (2 * NW - 1 - w)
        if ra >= R1:
            strips.append(Strips("lower", w, "idle", 0, 0, None, None))
        else:
            na = _kend_chunks(ra, R1, mblk, 0)
            nb = _kend_chunks(rb, R1, mblk, 0) if rb < R1 else 0
            if nb:
                strips.append(Strips("lower", w, "pair+tail" if nb > na else "pair", na, nb, _fold(ra, R1), _fold(rb, R1)))
            else:
                strips.append(Strips("lower", w, "strip", na, 0, _fold(ra, R1), None))
    if R1 < N:
        for w in range(NW):
            ra, rb = R1 + 16 * w, R1 + 16 * (2 * NW - 1 - w)
            if ra >= N:
                strips.append(Strips("upper1", w, "idle", 0, 0, None, None))
                strips.append(Strips("upper2", w, "idle", 0, 0, None, None))
                continue
            hb = rb < N
            strips.append(Strips("upper1", w, "pair" if hb else "strip", span >> 4, (span >> 4) if hb else 0, None, None))
            na = _kend_chunks(ra, N, mblk, R1)
            if hb:
                nb = _kend_chunks(rb, N, mblk, R1)
                strips.append(Strips("upper2", w, "pair+tail" if nb > na else "pair", na, nb, _fold(ra, N), _fold(rb, N)))
            else:
                strips.append(Strips("upper2", w, "strip", na, 0, _fold(ra, N), None))
    ktiles = []
    for p, (P0, Pend) in enumerate(((0, R1), (R1, N))[:1 if R1 == N else 2]):
        for jl in range(0, KP, 16):
            rows = Pend - P0 - jl
            ktiles.append((p + 1, jl, "full" if rows >= 16 else "ragged" if rows > 0 else "behind"))
    return Plan(N, m, NW, KP, R1, 1 if R1 == N else 2, tuple(strips), tuple(ktiles))


def _pair_path(n):
    return ("pair", n & 1, min(n >> 1, 2))


def _strip_path(n, what="strip"):
    return (what, n & 3, min(n >> 2, 2))


def star_bin(mblk, KP):
    """the star size against the 16-row tile, the two-tile strip pair and the panel."""
    if mblk < 16:
        return "<16"
    if mblk == 16:
        return "16"
    if mblk <= 32:
        return "17..32"
    return "33..KP/2" if 2 * mblk <= KP else ">KP/2"


def classes_of(pl):
    out = {(pl.NW, "passes", pl.passes), (pl.NW, "stars", star_bin(pl.m + 1, pl.KP))}
    for s in pl.strips:
        assert 0 <= s.na and (s.nb == 0 or s.na <= s.nb)
        if s.routine == "idle":
            out.add((pl.NW, s.kind, "idle"))
        elif s.routine == "strip":
            out.add((pl.NW, s.kind) + _strip_path(s.na))
        else:
            out.add((pl.NW, s.kind) + _pair_path(s.na))
            if s.nb > s.na:
                out.add((pl.NW, s.kind) + _strip_path(s.nb - s.na, "tail"))
        for which, f in (("a", s.fold_a), ("b", s.fold_b)):
            if f:
                out.add((pl.NW, s.kind, "fold", which, f))
    for p, _, kind in pl.ktiles:
        out.add((pl.NW, "ktile", p, kind))
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def classes(N, m):
    return classes_of(plan(N, m))


@functools.lru_cache(maxsize=None)
def accepted():
    """Every (N, m + 1) the kernel accepts, ordered by N then m + 1."""
    out = []
    for mblk in range(2, MBLK_MAX + 1):
        for N in range(mblk, 2 * max(PANELS.values()) + 1, mblk):
            if form_of(N, mblk - 1)[0] is not None:
                out.append((N, mblk))
    return tuple(sorted(out))


def all_classes():
    out = set()
    for N, mblk in accepted():
        out |= classes(N, mblk - 1)
    return out


def greedy_cover():
    """The shape that adds the most classes not covered yet, the smallest N (then the smallest star) among equals."""
    shapes, todo, out = accepted(), set(all_classes()), []
    while todo:
        best = max(shapes, key=lambda s: (len(classes(s[0], s[1] - 1) & todo), -s[0], -s[1]))
        out.append(best)
        todo -= classes(best[0], best[1] - 1)
    return out


# greedy_cover() of the classification above, (N, m + 1); tests/test_fused_cases_host.py proves that it covers
COVER = ((836, 19), (480, 15), (330, 33), (994, 2), (98, 2), (515, 103), (390, 30), (258, 129), (496, 16), (825, 33), (257, 257),
         (290, 145), (476, 28), (322, 161), (513, 57), (1024, 16), (113, 113), (273, 273), (289, 289), (305, 305), (430, 86),
         (455, 65), (498, 2))

# the shapes tests/test_gpu_fused.py runs, (N, m + 1): what the suite reached before this module
BEFORE = ((32, 32), (64, 32), (78, 26), (200, 10), (240, 15), (256, 32), (260, 26), (264, 33), (416, 26), (462, 33), (512, 32),
          (480, 40), (650, 26), (1024, 32), (512, 32), (992, 31))

WORKLOAD = tuple((n_q * 26, 26) for n_q in range(1, 20)) + tuple((n_q * 32, 32) for n_q in range(1, 17))

KERNELS = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")
M_CASE = 65                     # two full blocks of 32 candidates and a ragged one
SIGMA_F = 1.0

Case = collections.namedtuple("Case", "N m D kernel seed")


def theta_of(D):
    """(sigma, l, sigma_f): l = 0.6 sqrt(D) keeps K* on [0, 1]^D in roughly [0.25, 1], the contraction as large as sf^2."""
    return (0.05, 0.6 * np.sqrt(D), SIGMA_F)


def _cases():
    out, seen = [], set()
    for i, (N, mblk) in enumerate(COVER + WORKLOAD):
        if (N, mblk) in seen:
            continue
        seen.add((N, mblk))
        # D = 3 throughout; every eighth case at D = 16 (four k-steps per K* tile: both phases long)
        out.append(Case(N, mblk - 1, 16 if i % 8 == 5 else 3, KERNELS[i % 4], 1000 + i))
    return tuple(out)


CASES = _cases()


def case_id(c):
    return f"N{c.N}-m{c.m}-D{c.D}-{c.kernel.split('_')[0]}"


def engine_of(c):
    """The PPBO_FUSED value of the engine that takes the case on the one-launch kernel."""
    return 1 if (form_of(c.N, c.m)[0] == 8 and c.D <= D_DEFAULT_MAX) else 2


# ---- the dense reference ------------------------------------------------------------------------------------------------
def kstar(X, Xc, kernel, theta, dtype=np.float64):
    """K* [N, M] from direct differences, in `dtype`."""
    X, Xc = np.asarray(X, dtype=dtype), np.asarray(Xc, dtype=dtype)
    l, sf = dtype(theta[1]), dtype(theta[2])
    r2 = np.zeros((X.shape[0], Xc.shape[0]), dtype=dtype)
    for d in range(X.shape[1]):
        dd = (X[:, d][:, None] - Xc[:, d][None, :]) / l
        r2 += dd * dd
    if kernel == "SE_kernel":
        k = np.exp(-r2 / dtype(2))
    elif kernel == "RQ_kernel":
        k = (dtype(1) + r2 / dtype(4)) ** -2
    elif kernel == "Matern52_kernel":
        a = np.sqrt(dtype(5) * r2)
        k = (dtype(1) + a + a * a / dtype(3)) * np.exp(-a)
    elif kernel == "Matern32_kernel":
        a = np.sqrt(dtype(3) * r2)
        k = (dtype(1) + a) * np.exp(-a)
    else:
        raise ValueError(kernel)
    return sf * sf * k


def reference(arrs, Xc, kernel, theta, m, dtype=np.float64, G=None, Ks=None):
    """(mu, var, t, q) [M] of the state `arrs` (tests/test_gpu_fused.synth_post) in NumPy: mu = K*' alpha,
    var = sf^2 + t + q with t = k*' Lambda k* (star form) and q = |G k*|^2 -- dense_reference's expression with K* from
    direct differences and its terms returned, for the bound's scale."""
    Ks = kstar(arrs["X"], Xc, kernel, theta, dtype) if Ks is None else Ks
    G = np.asarray(arrs["G"] if G is None else G, dtype=dtype)
    al, ld, lo = (np.asarray(arrs[k], dtype=dtype) for k in ("alpha", "lam_diag", "lam_off"))
    N, mblk = Ks.shape[0], m + 1
    obs = (np.arange(N) // mblk) * mblk
    mu = al @ Ks
    t = (ld[:, None] * Ks * Ks).sum(axis=0) + dtype(2) * (lo[:, None] * Ks * Ks[obs]).sum(axis=0)   # lam_off = 0 on observation rows
    Y = G @ Ks
    q = (Y * Y).sum(axis=0)
    sf2 = dtype(theta[2]) * dtype(theta[2])
    return mu, sf2 + t + q, t, q


def scales(theta, mu, t, q):
    """(scale of the mean, scale of the variance) the bounds multiply: max |mu| and max_c (sf^2 + |t_c| + q_c)."""
    return float(np.abs(mu).max()), float((float(theta[2]) ** 2 + np.abs(t) + q).max())


def block_sensitivity(arrs, Ks, m):
    """For every 16-row x 16-column block of G that meets the block-triangular support: the largest change over the
    candidates of q = |G k*|^2 when the block is zeroed.  Returns the array of these maxima (one per block)."""
    G = arrs["G"]
    N, M = Ks.shape
    mblk, nb = m + 1, -(-N // 16)
    P = 16 * nb
    Gp = np.zeros((P, P))
    Gp[:N, :N] = G
    Kp = np.zeros((P, M))
    Kp[:N] = Ks
    Y = Gp @ Kp
    kend = np.zeros(P, dtype=int)
    kend[:N] = (np.arange(N) // mblk + 1) * mblk
    out = []
    for J in range(nb):
        d = Gp[:, 16 * J:16 * J + 16] @ Kp[16 * J:16 * J + 16]          # [P, M]: what block column J adds to Y
        dq = (d * d - 2.0 * Y * d).reshape(nb, 16, M).sum(axis=1)        # [nb, M]: q' - q per block row
        inside = (kend.reshape(nb, 16) > 16 * J).any(axis=1)
        out.append(np.abs(dq[inside]).max(axis=1))
    return np.concatenate(out)


def candidates(c, M=M_CASE):
    """The case's candidates, uniform in [0, 1]^D."""
    return np.random.default_rng(c.seed + 500000).random((M, c.D))


class _HostEngine:
    """Stands in for an Engine where synth_post only needs the arrays."""
    @staticmethod
    def dev(a):
        return a


def host_state(c):
    """The arrays of the case's hand-built posterior (tests/test_gpu_fused.synth_post, the generator the GPU test hands
    its engines), without a device."""
    from test_gpu_fused import synth_post
    return synth_post(_HostEngine(), c.N, c.D, c.m, c.kernel, theta_of(c.D), seed=c.seed)[1]
