"""Host: exp_nonpos (ppbo_amd/csrc/common.h) and rff_cos_fast (ppbo_amd/csrc/rffmath.h) emulated step by step on the CPU
from the constants PARSED out of those sources (a re-fit by tools/expfit.py is followed, nothing is copied here), every
fma an exact rational product-sum rounded once, against mpmath at 300 bits on the sweeps of elementary_points.py.

This is the evidence that the per-element bounds of test_gpu_elementary.py are attainable by the routines as written:
the device executes the same IEEE operations (v_fma_f64, v_rndne_f64, v_ldexp_f64), so a correct build reproduces
these numbers.

Measured on the sweeps (4096 exponents, 6144 fast-range phases):
  exp_nonpos    worst |result - exp(x)| = 0.854 ulp for normal results, 0.695 ulp (of 5e-324) in the subnormal band; every
                result is the correctly rounded value or its neighbour (6.6 % of the normal results are the neighbour);
                exactly 0 from -745.2 down and below the clamp, exactly 1 at 0
  rff_cos_fast  worst |result - cos(x)| = 2.0000 x 2^-53 absolute (bound 2^-51 = 4 x 2^-53); next to the zeros of the
                cosine the RELATIVE error reaches 2.2e3 x 2^-53, which is why the bound is absolute
  reduction     n = 2k - 1 <= 1018591 < 2^20 against three pieces of pi/2 of at most 33 significant bits: every
                product n x piece fits 53 bits"""
import math
import os
from fractions import Fraction

import numpy as np

import elementary_points as ep

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppbo_amd", "csrc")
EXP = ep.parse_exp_nonpos(os.path.join(CSRC, "common.h"))
COS = ep.parse_rff_cos(os.path.join(CSRC, "rffmath.h"))


def fma(a, b, c):
    """a * b + c, rounded once (Fraction arithmetic is exact; float() of a Fraction rounds to nearest even, subnormals
    included)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def rint(v):
    return float(np.rint(v))


def exp_nonpos(x):
    x = max(x, EXP["clamp"])
    n = rint(x * EXP["inv_ln2"])
    r = fma(n, -EXP["ln2"][0], x)
    r = fma(n, -EXP["ln2"][1], r)
    q = EXP["q0"]
    for c in EXP["coef"]:
        q = fma(q, r, c)
    return math.ldexp(q, int(n))


def rff_cos_fast(x):
    ax = abs(x)
    kf = rint(fma(ax, COS["inv_pi"], 0.5))
    n = fma(2.0, kf, -1.0)
    r = ax
    for piece in COS["pio2"]:
        r = fma(-n, piece, r)
    z = r * r
    q = COS["s"][8]
    for k in range(7, -1, -1):
        q = fma(q, z, COS["s"][k])
    sn = r * q
    return -sn if int(kf) & 1 else sn


def test_parsed_constants_are_the_routines():
    """The parser found the reduction the comments describe: two pieces of ln 2 and three of pi/2 that sum to the
    constant far below double precision, 1 / ln 2 and 1 / pi, and Taylor-like leading coefficients."""
    assert abs(EXP["inv_ln2"] * math.log(2.0) - 1.0) < 1e-15
    assert abs(Fraction(EXP["ln2"][0]) + Fraction(EXP["ln2"][1]) - Fraction(math.log(2.0))) < Fraction(1, 2 ** 52)
    assert EXP["coef"][-2:] == [1.0, 1.0] and abs(EXP["coef"][-3] - 0.5) < 1e-14
    assert abs(COS["inv_pi"] * math.pi - 1.0) < 1e-15 and COS["range"] == ep.COS_FAST_RANGE
    with ep.mp_ctx():
        import mpmath
        s = sum(mpmath.mpf(p) for p in COS["pio2"])
        assert abs(s - mpmath.pi / 2) < mpmath.mpf(2) ** -96
    assert COS["s"][0] == 1.0 and abs(COS["s"][1] + 1.0 / 6.0) < 1e-15


def test_exp_nonpos_within_one_ulp_of_the_rounded_value():
    _, arg = ep.exp_points()
    cr, exact = ep.exp_reference()
    got = np.array([exp_nonpos(a) for a in arg.tolist()])
    dist = np.abs(ep.ordinal(got) - ep.ordinal(cr))
    with ep.mp_ctx():
        import mpmath
        err = np.array([float(abs(mpmath.mpf(g) - e) / u) for g, e, u in zip(got.tolist(), exact, ep.spacing(cr).tolist())])
    sub = cr < 2.2250738585072014e-308
    print(f"exp_nonpos emulated: worst {err[~sub].max():.3f} ulp normal, {err[sub].max():.3f} ulp subnormal; "
          f"{(dist[~sub] == 1).mean():.2%} of the normal results are the neighbour of the rounded value")
    assert dist.max() <= 1, (arg[dist.argmax()], got[dist.argmax()], cr[dist.argmax()])
    assert np.all(got[arg <= -745.2] == 0.0)         # below ln(2^-1075) = -745.13 the value rounds to zero
    assert got[arg == 0.0].tolist() == [1.0]
    assert sub.sum() > 500 and (got[sub] > 0).sum() > 400      # the subnormal band is really walked


def test_rff_cos_fast_within_2_pow_minus_51():
    ph, near = ep.cos_points()
    ref = ep.cos_reference()
    fast = np.abs(ph) < COS["range"]
    got = np.array([rff_cos_fast(v) for v in ph[fast].tolist()])
    err = np.abs(got - ref[fast])
    rel = err[ref[fast] != 0] / np.abs(ref[fast][ref[fast] != 0])
    print(f"rff_cos_fast emulated: worst {err.max() * 2.0 ** 53:.4f} x 2^-53 absolute, "
          f"{rel.max() * 2.0 ** 53:.3g} x 2^-53 relative")
    assert err.max() <= 2.0 ** -51, (ph[fast][err.argmax()], got[err.argmax()])
    nf = near[fast]
    assert np.array_equal(np.signbit(got[nf]), np.signbit(ref[fast][nf]))     # the right side of every zero
    assert np.all(got[ph[fast] == 0.0] == 1.0)
    neg = ep.cos_negated_index()
    full = np.full(len(ph), np.nan)
    full[fast] = got
    assert np.array_equal(full[fast], full[neg][fast])                        # cos(-x) == cos(x) bit for bit


def test_odd_multiplier_is_exact_against_every_piece():
    """Every k the fast path can reach, k = rint(|x| / pi + 1/2) for |x| < 1.6e6, gives n = 2k - 1 whose product with each
    piece of pi/2 is a double: the odd part of the piece's significand times n stays below 2^53 (the source: "the odd
    multiplier 2k-1 < 2^21 is exact against each")."""
    top = float(np.nextafter(COS["range"], 0.0))
    k_max = int(rint(fma(top, COS["inv_pi"], 0.5)))
    n_max = 2 * k_max - 1
    assert ep.K_MAX <= n_max < 2 ** 21      # the sweep's multiples of pi/2 stay inside what the routine reaches
    for piece in COS["pio2"]:
        num = Fraction(piece).numerator
        while num % 2 == 0:
            num //= 2
        assert num * n_max < 2 ** 53, (piece, num.bit_length(), n_max)
    # ... and spelled out for the first piece at the multipliers the sweep reaches
    rng = np.random.default_rng(7)
    for n in [n_max, n_max - 2, 1, 3] + (2 * rng.integers(1, k_max, 2000) - 1).tolist():
        p = COS["pio2"][0] * float(n)
        assert Fraction(p) == Fraction(COS["pio2"][0]) * n
