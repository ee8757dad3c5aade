"""Seeded argument sweeps and high-precision references for the hand-written fp64 elementary functions: exp_nonpos and
sqrt_nonneg (ppbo_amd/csrc/common.h) and rff_cos_fast (ppbo_amd/csrc/rffmath.h).  Shared by test_elementary_host.py (a
CPU emulation of the routines from their parsed constants) and test_gpu_elementary.py (the device kernels, one output
element = one function value).

Everything here is exact end to end.  A covariance argument is a coordinate x of at most 26 significant bits paired with
the origin, at l = 2^-6 and sigma_f = 1: x^2 is an exact double, |x|^2 + |0|^2 - 2 x.0 is x^2 in either evaluation
order, the SE constant c0 = 0.5 / l^2 is 2048, so the exponent -c0 x^2 is an exact double that the helpers check with
fractions.Fraction.  A cosine phase is a weight W_f against x = 1 with b = 0 (or b_f against W = 0).
References are mpmath at PREC bits on those exact doubles, rounded once (through Fraction, so subnormals round
correctly too)."""
import functools
import math
import re
from fractions import Fraction

import mpmath
import numpy as np

PREC = 300
LENGTHSCALE = 2.0 ** -6       # theta[1] of every covariance sweep
SE_C0 = 2048.0                # 0.5 / l^2
RQ_C0 = 1024.0                # 1 / (4 l^2)
SQRT5 = 2.23606797749978969641   # the literals of make_kern_params (common.h), parsed to the same doubles
SQRT3 = 1.73205080756887729353
COS_FAST_RANGE = 1.6e6
COS_F = 512                   # features per call: with sigma_f = 16 the amplitude sqrt(2 sf^2 / F) is exactly 1
COS_SIGMA_F = 16.0
K_MAX = 1018000               # multiples of pi/2 probed (1.6e6 / (pi/2) = 1018591.6)


def mp_ctx():
    return mpmath.workprec(PREC)


def mp_to_float(v):
    """An mpf rounded ONCE to the nearest double, subnormals and zero included."""
    sign, man, exp, _ = v._mpf_
    if man == 0:
        return 0.0
    fr = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return float(-fr if sign else fr)


def ordinal(a):
    """Doubles of one sign as consecutive integers: |ordinal(a) - ordinal(b)| counts the representable values between
    two results (an ulp distance that is right across binades and in the subnormals)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert not np.signbit(a).any()
    return a.view(np.int64).astype(np.int64)


def spacing(ref):
    """ulp of each reference value (5e-324 at zero and in the subnormals)."""
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float64)))


def round_bits(x, bits=26):
    """x rounded to `bits` significant bits."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)


# ---- the covariance sweeps -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exp_points():
    """(x, arg): coordinates x >= 0 of at most 26 significant bits and the exact SE exponents arg = -2048 x^2:
    dense in [-40, 0], uniform in [-708, -40], the subnormal-result band [-745.2, -708], (-750, -745.2] and below -750
    (results exactly 0), and x = 0 (result exactly 1)."""
    rng = np.random.default_rng(20240611)
    t = np.concatenate([
        -40.0 * rng.random(2048),
        -40.0 - 668.0 * rng.random(1024),
        -708.0 - 37.2 * rng.random(640),
        -745.2 - 4.8 * rng.random(190),
        -750.0 - 350.0 * rng.random(190),
        -np.ldexp(1.0, -np.arange(1, 60, 20)),      # tiny arguments: results just below 1
    ])
    x = round_bits(np.sqrt(-t / SE_C0))
    x = np.concatenate([[0.0], x])
    arg = -SE_C0 * (x * x)
    for xi, ai in zip(x.tolist(), arg.tolist()):      # exactness is asserted, not assumed
        assert Fraction(ai) == -2048 * Fraction(xi) ** 2
    assert len(x) == 4096
    assert (arg > -40).sum() > 2000 and ((arg < -708) & (arg > -745.2)).sum() > 500 and (arg < -750).sum() > 100
    x.setflags(write=False)
    arg.setflags(write=False)
    return x, arg


@functools.lru_cache(maxsize=None)
def exp_reference():
    """(correctly rounded exp(arg), exp(arg) as mpf) at exp_points()."""
    _, arg = exp_points()
    with mp_ctx():
        exact = [mpmath.exp(mpmath.mpf(a)) for a in arg.tolist()]
        cr = np.array([mp_to_float(v) for v in exact])
    cr.setflags(write=False)
    return cr, exact


RQ_EXACT_T = 4096             # the first RQ_EXACT_T points of rq_points() have an exact t = 1 + 1024 x^2


@functools.lru_cache(maxsize=None)
def rq_points():
    """Coordinates for the RQ kernel 1 / t^2, t = 1 + 1024 x^2 (l = 2^-6).  The first RQ_EXACT_T are the coordinates of
    exp_points() cut to 13 significant bits: x^2 has 26 bits and t is an exact double (asserted), so sf2 / (t * t) is
    two roundings away from the true value.  Behind them the first 2048 of exp_points() as they are (26 bits, the dense
    range): there t itself is rounded, a third rounding."""
    x26 = exp_points()[0]
    x13 = round_bits(x26, 13)
    for xi in x13.tolist():
        assert Fraction(1.0 + RQ_C0 * (xi * xi)) == 1 + 1024 * Fraction(xi) ** 2
    x = np.concatenate([x13, x26[:2048]])
    assert len(x13) == RQ_EXACT_T
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rq_reference():
    """(correctly rounded 1 / (1 + 1024 x^2)^2, the same as mpf) at rq_points(): the RQ kernel at l = 2^-6."""
    x = rq_points()
    with mp_ctx():
        exact = [1 / (1 + 1024 * mpmath.mpf(v) ** 2) ** 2 for v in x.tolist()]
        cr = np.array([mp_to_float(v) for v in exact])
    cr.setflags(write=False)
    return cr, exact


def matern_c0(nu):
    """The host's own rounded constant of make_kern_params at l = 2^-6: sqrt(5) / l or sqrt(3) / l."""
    return {52: SQRT5, 32: SQRT3}[nu] / LENGTHSCALE


@functools.lru_cache(maxsize=None)
def matern_points(nu):
    """Coordinates x >= 0 of at most 26 significant bits with a = c0 x swept over [0, 900]: dense in [0, 40], uniform to
    745, the band where exp(-a) is subnormal or flushes, the cap at 800 and beyond it (value exactly 0), x = 0."""
    rng = np.random.default_rng(520 + nu)
    a = np.concatenate([40.0 * rng.random(1024), 40.0 + 668.0 * rng.random(640), 708.0 + 42.0 * rng.random(256),
                        750.0 + 50.0 * rng.random(63), 800.0 + 100.0 * rng.random(64)])
    x = np.concatenate([[0.0], round_bits(a / matern_c0(nu))])
    for xi in x.tolist():
        assert Fraction(xi * xi) == Fraction(xi) ** 2
    assert len(x) == 2048
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def matern_reference(nu):
    """(a, value) as mpf lists at matern_points(nu): a = c0_host * sqrt(s) with s = x^2 exact, then the closed form at
    sigma_f = 1."""
    x = matern_points(nu)
    c0 = matern_c0(nu)
    with mp_ctx():
        a = [mpmath.mpf(c0) * mpmath.sqrt(mpmath.mpf(v) ** 2) for v in x.tolist()]
        poly = (lambda t: 1 + t + t * t / 3) if nu == 52 else (lambda t: 1 + t)
        val = [poly(t) * mpmath.exp(-t) for t in a]
    return a, val


# ---- the cosine sweep ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cos_points():
    """8192 phases, every magnitude with both signs.  In the fast range |x| < 1.6e6: uniform in +-100 and +-1.6e6, the
    nearest double to k pi/2 and its two neighbours for random k <= 1,018,000 of both parities, the top of the range up
    to nextafter(1.6e6, 0), and 0, 5e-324, 1e-300.  On the library path: exactly 1.6e6, its upper neighbour, and values up
    to 1e9.  Ordered so that index i holds a library-path phase exactly when i % 4 == 3: every aligned group of four,
    and so every group of 64, mixes the two (the kernels branch on a wave-uniform ballot and select per element).
    Returns (phases, near) with near[i] = True at the k pi/2 neighbourhoods."""
    rng = np.random.default_rng(1618)
    with mp_ctx():
        ks = np.concatenate([rng.integers(1, K_MAX, 252), [1, 2, 3, 4, K_MAX - 1, K_MAX]])
        assert (ks % 2 == 0).sum() > 50 and (ks % 2 == 1).sum() > 50
        mid = np.array([mp_to_float(mpmath.mpf(int(k)) * mpmath.pi / 2) for k in ks])
    near_pts = np.concatenate([np.nextafter(mid, 0.0), mid, np.nextafter(mid, np.inf)])          # 774
    top = np.concatenate([1.5e6 + 1e5 * rng.random(762), [np.nextafter(COS_FAST_RANGE, 0.0), 1.5e6]])   # 764
    special = np.array([0.0, 5e-324, 1e-300, 0.5 * math.pi, math.pi])
    fast = np.concatenate([near_pts, top, special, 100.0 * rng.random(764), COS_FAST_RANGE * rng.random(765)])
    assert len(fast) == 3072 and np.all(fast < COS_FAST_RANGE)
    slow = np.concatenate([[COS_FAST_RANGE, np.nextafter(COS_FAST_RANGE, np.inf), 1e9],
                           COS_FAST_RANGE * (1e9 / COS_FAST_RANGE) ** rng.random(1021)])
    assert len(slow) == 1024 and np.all(slow >= COS_FAST_RANGE) and np.all(slow <= 1e9)
    near = np.zeros(len(fast), dtype=bool)
    near[:len(near_pts)] = True
    pf = rng.permutation(len(fast))
    fast, near = fast[pf], near[pf]
    slow = slow[rng.permutation(len(slow))]
    # both signs, the negative right behind its positive twin within each class
    fast2 = np.stack([fast, -fast], axis=1).reshape(-1)
    near2 = np.repeat(near, 2)
    slow2 = np.stack([slow, -slow], axis=1).reshape(-1)
    ph = np.empty(8192)
    nr = np.zeros(8192, dtype=bool)
    is_slow = (np.arange(8192) % 4) == 3
    ph[is_slow], ph[~is_slow], nr[~is_slow] = slow2, fast2, near2
    assert np.array_equal(is_slow, ~(np.abs(ph) < COS_FAST_RANGE))
    ph.setflags(write=False)
    nr.setflags(write=False)
    return ph, nr


@functools.lru_cache(maxsize=None)
def cos_reference():
    """cos(phase) at cos_points(), each rounded once from PREC bits (the error of this reference, half an ulp of a value
    of at most 1, i.e. 2^-54, is part of what the 2^-51 bound allows)."""
    ph, _ = cos_points()
    with mp_ctx():
        ref = np.array([mp_to_float(mpmath.cos(mpmath.mpf(v))) for v in ph.tolist()])
    ref.setflags(write=False)
    return ref


def cos_negated_index():
    """For each phase the index of its negative in cos_points() (+0 and -0 are each other's)."""
    ph, _ = cos_points()
    where = {}
    for i, v in enumerate(ph.tolist()):
        where[(v, math.copysign(1.0, v))] = i
    return np.array([where[(-v, math.copysign(1.0, -v))] for v in ph.tolist()])


# ---- the routines' constants, read from the sources ---------------------------------------------------------------------------
def _body(text, head):
    """The brace-balanced body that follows `head` in a C++ source."""
    i = text.index(head)
    j = text.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        if depth == 0:
            return text[j:k + 1]
        k += 1


_NUM = r"-?(?:0x[0-9a-fA-F.]+p[-+]?\d+|\d+\.\d*(?:e[-+]?\d+)?)"


def _val(tok):
    return float.fromhex(tok) if "0x" in tok.lower() else float(tok)


def parse_exp_nonpos(path):
    """common.h -> dict(clamp, inv_ln2, ln2 = [two Cody-Waite pieces as positive numbers], q0, coef = [the constants
    of the Horner steps in source order])."""
    body = _body(open(path).read(), "double exp_nonpos(double x)")
    clamp = _val(re.search(r"fmax\(x,\s*(" + _NUM + r")\)", body).group(1))
    inv_ln2 = _val(re.search(r"rint\(x \*\s*(" + _NUM + r")\)", body).group(1))
    ln2 = [-_val(m) for m in re.findall(r"fma\(n,\s*(" + _NUM + r"),", body)]
    q0 = _val(re.search(r"double q =\s*(" + _NUM + r");", body).group(1))
    coef = [_val(m) for m in re.findall(r"q = __builtin_fma\(q, r,\s*(" + _NUM + r")\);", body)]
    assert clamp == -750.0 and len(ln2) == 2 and len(coef) == 11 and "ldexp(q, (int)n)" in body, "exp_nonpos changed shape"
    return dict(clamp=clamp, inv_ln2=inv_ln2, ln2=ln2, q0=q0, coef=coef)


def parse_rff_cos(path):
    """rffmath.h -> dict(range, inv_pi, pio2 = [three pieces], s = [nine coefficients of r^(2k+1)])."""
    text = open(path).read()
    rng = _val(re.search(r"RFF_COS_FAST_RANGE =\s*(" + _NUM + r");", text).group(1))
    table = re.search(r"static const double s\[9\] = \{(.*?)\};", text, re.S).group(1)
    s = [_val(m) for m in re.findall(_NUM, table)]
    body = _body(text, "double rff_cos_fast(double x, const RffPoly& P)")
    inv_pi = _val(re.search(r"fma\(ax,\s*(" + _NUM + r"),\s*0\.5\)", body).group(1))
    pio2 = [_val(m) for m in re.findall(r"fma\(-n,\s*(" + _NUM + r"),", body)]
    assert len(s) == 9 and len(pio2) == 3 and "fma(2.0, kf, -1.0)" in body, "rff_cos_fast changed shape"
    return dict(range=rng, inv_pi=inv_pi, pio2=pio2, s=s)
