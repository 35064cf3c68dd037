"""TEST INFRASTRUCTURE — arguments, exact references, the error measure and the bounds for the lean float64 routines of
csrc/wf_f64_math.h, shared by tests/test_f64_math.py (CPU: the generator and the measure) and tests/test_f64_math_gpu.py
(the routines on the device through libwfcheck.so, csrc/check/wf_math_check.hip).

REFERENCE  mpmath at 50 digits on the exact double arguments.  A reference value is split into hi = float(ref) and
lo = float(ref - hi); the error of a result `got` is |(got - hi) - lo| / ulp(hi), ulp the spacing of doubles at hi.

BOUNDS, in ulp of the reference.  None is taken from a routine's own output: each is the next integer above the worst value
of a host stand-in of the header (the hardware rcp / rsq estimates replaced by exact values perturbed by 3e-8, built without
fused contraction, compared with 80-bit libm), which shows that the arithmetic itself stays inside.  `device` = the worst
value measured on an MI355X over the cases below, lean routine / the device library on the same arguments.

  routine        bound                    stand-in     device (lean / library)
  rcp64          1                        0.13         0.50 / 0.50
  sqrt_pos       1                        0.50         0.50 / 0.50
  sqrt_nn        1 (sqrt_pos above 1e-280; exactly 0 at and below)   0.50 / 0.50
  sincos_small   2                        1.09 / 0.88  0.97, 0.76 / 0.66, 0.63
  atan_small     2                        1.00         0.90 / 0.54
  cbrt_pos       2                        0.95         0.84 / 0.50
  cbrt_any       2                        0.95         0.85 / 0.50
  exp_lean       3 (normal results)       2.00         1.74 / 0.85 (subnormal: 0.98 / 0.69 of 2^-1074)
                 2 * 2^-1074 absolute (subnormal results)
  log_lean       4                        3.27         1.65 / 0.52
  log_any        4                        3.27         1.65 / 0.52
  tan_small      4                        2.80         2.33 / 0.60
  asin_small     4                        2.44         2.00 / 0.62
  atan_01        4                        2.40         1.42 / 0.77
  tan_any        5                        3.63         2.69 / 0.88 (1.15e8 before the pi/2 parts were mended)
  atan2_any      5                        3.65         1.59 / 1.12
  asin_any       5                        3.82         2.13 / 0.64 (974 with the radicand 1 - x * x)
  pow_lean/_any  3 + 2 |y ln x|           5.6 at 4.2   8.65 / 1.16; at most 0.45 of the bound
                 (exp's 3; the error of y log x, relative to |y ln x|, enters the result undamped as a relative error;
                 x in 1e-6 .. 1e6 under the kernels' exponents keeps |y ln x| below 12.2)
  sincos_any     3.3e-16 absolute         1.5e-16      1.3e-16 / 8.0e-17
"""
import collections
import functools
import zlib

import mpmath
import numpy as np

DPS = 50
N_RANDOM = 2000
SEED = 5
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
SQRT_HALF = 0.70710678118654752
TINY = 2.0 ** -1074  # the smallest subnormal
HUGE = float(np.finfo(np.float64).max)
MIN_NORMAL = 2.0 ** -1022

# ids of csrc/check/wf_math_check.hip (enum WfCheckFn)
IDS = {n: i for i, n in enumerate((
    "rcp64", "sqrt_pos", "sqrt_nn", "exp_lean", "log_lean", "log_any", "pow_lean", "pow_any", "sincos_small", "sincos_any",
    "tan_small", "tan_any", "asin_small", "asin_any", "atan_small", "atan_01", "atan2_any", "cbrt_pos", "cbrt_any"))}
LIB_IDS = {n: 100 + i for i, n in enumerate(("rcp", "sqrt", "exp", "log", "pow", "sincos", "tan", "asin", "atan", "atan2", "cbrt"))}
# the device library's counterpart of each routine: printed next to the lean figure, never asserted
LIB_OF = {"rcp64": "rcp", "sqrt_pos": "sqrt", "sqrt_nn": "sqrt", "exp_lean": "exp", "log_lean": "log", "log_any": "log",
          "pow_lean": "pow", "pow_any": "pow", "sincos_small": "sincos", "sincos_any": "sincos", "tan_small": "tan",
          "tan_any": "tan", "asin_small": "asin", "asin_any": "asin", "atan_small": "atan", "atan_01": "atan",
          "atan2_any": "atan2", "cbrt_pos": "cbrt", "cbrt_any": "cbrt"}
N_OUT = {n: 2 if n.startswith("sincos") else 1 for n in IDS}

# ulp bounds (see the table above); pow: (a, b) = a + b |y ln x|; sincos_any: absolute
ULP_BOUND = {"rcp64": 1, "sqrt_pos": 1, "sqrt_nn": 1, "sincos_small": 2, "atan_small": 2, "cbrt_pos": 2, "cbrt_any": 2,
             "exp_lean": 3, "log_lean": 4, "log_any": 4, "tan_small": 4, "asin_small": 4, "atan_01": 4, "tan_any": 5,
             "atan2_any": 5, "asin_any": 5}
POW_BOUND = (3.0, 2.0)
EXP_SUBNORMAL_ABS = 2.0 * TINY
SINCOS_ANY_ABS = 3.3e-16

# the exponents the kernels pass to pow_any with the default model (wf_resolve.hip: POW_F64(ai, ch_ai),
# POW_F64(dx / D, ch_downstream), POW_F64(cos yaw, pP / 3); probe/wf_probe_kernels.hip: the same two Crespo-Hernandez
# powers, pow_any(z / HH, shear) and pow_any(z, shear - 1)); -0.32 is ch_downstream, the old tool's exponent
POW_EXPONENTS = (0.8, -0.32, 1.88 / 3.0, 0.12, 0.12 - 1.0)


def _rng(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def _loguniform(rng, lo, hi, n=N_RANDOM):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _neighbours(a):
    a = np.asarray(a, np.float64)
    return np.concatenate([np.nextafter(a, -np.inf), a, np.nextafter(a, np.inf)])


def _both_signs(a):
    return np.concatenate([a, -a])


def _small_range(name, lim):
    """|x| <= lim: uniform, log-uniform towards 0, both ends and 0."""
    rng = _rng(name)
    return np.concatenate([rng.uniform(-lim, lim, N_RANDOM), _both_signs(_loguniform(rng, 1e-12, lim, N_RANDOM // 4)),
                           [-lim, lim, 0.0]])


# ---- the aimed points (tests/test_f64_math.py checks what each of them straddles) -------------------------------------
def powers_of_two(lo_exp, hi_exp):
    return np.ldexp(1.0, np.arange(lo_exp, hi_exp + 1))


def exp_boundaries():
    """(k + 1/2) ln 2 (1 -+ 1e-13), k = -1000 .. 1000: the two sides of every tie of exp_lean's rint(x / ln 2)."""
    k = np.arange(-1000, 1001, dtype=np.float64)
    c = (k + 0.5) * LN2
    return c * (1.0 - 1e-13), c * (1.0 + 1e-13)


def log_switch():
    """sqrt(1/2) (1 -+ 1e-12) 2^e, e = -20 .. 20: the two sides of log_lean's choice between m and 2 m."""
    e = np.arange(-20, 21)
    return np.ldexp(SQRT_HALF * (1.0 - 1e-12), e), np.ldexp(SQRT_HALF * (1.0 + 1e-12), e)


def log_near_one():
    d = 10.0 ** -np.arange(1.0, 13.5, 0.5)
    return np.concatenate([1.0 + d, 1.0 - d])


def atan_ties():
    """(2 j + 1) / 16 (1 -+ 1e-14), j = 0 .. 7: the two sides of every tie of atan_01's rint(8 r)."""
    c = (2.0 * np.arange(8) + 1.0) / 16.0
    return c * (1.0 - 1e-14), c * (1.0 + 1e-14)


def quarter_turns():
    """k pi/2 (1 -+ 1e-13), k = -200 .. 200: zeros and extrema of sin / cos, and the ties' neighbours of the reduction."""
    k = np.arange(-200, 201, dtype=np.float64)
    c = k * (np.pi / 2.0)
    return np.concatenate([c * (1.0 - 1e-13), c * (1.0 + 1e-13)])


def asin_near_one(rng):
    """+-(1 - e^(-36 u)): every decade of 1 - |x| down to the last bit."""
    return _both_signs(1.0 - np.exp(-36.0 * rng.uniform(0.0, 1.0, N_RANDOM // 2)))


def cbrt_exponents():
    """2^e and 1.7 * 2^e for every exponent residue mod 3, negative exponents and subnormals included, both signs."""
    e = np.concatenate([np.arange(-1074, -1060), np.arange(-1030, -1015), np.arange(-12, 13), np.arange(990, 1000)])
    return _both_signs(np.concatenate([np.ldexp(1.0, e), np.ldexp(1.7, e[e > -1070])]))


ATAN2_AXES = (  # (y, x): the axes, signed zeros on either side, the origin
    (0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (1.0, -0.0), (-1.0, 0.0), (-1.0, -0.0), (0.0, 0.0),
    (0.0, 3.5), (2.5, 0.0), (-2.5, 0.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))


@functools.lru_cache(maxsize=None)
def cases(name):
    """The arguments of routine `name`: a tuple of one or two float64 arrays (fixed rng: the same on every call)."""
    rng = _rng(name)
    if name == "rcp64":
        x = np.concatenate([_both_signs(_loguniform(rng, 1e-300, 1e300)), _neighbours(powers_of_two(-996, 996))])
    elif name == "sqrt_pos":
        x = np.concatenate([_loguniform(rng, 1e-280, 1e280), _neighbours(powers_of_two(-929, 929))])
    elif name == "sqrt_nn":
        x = np.concatenate([_loguniform(rng, 1e-279, 1e280), [1e-279]])  # (0 and 1e-281 -> exactly 0: SPECIALS)
    elif name == "exp_lean":
        lo, hi = exp_boundaries()
        x = np.concatenate([rng.uniform(-708.0, 700.0, N_RANDOM), _both_signs(_loguniform(rng, 1e-300, 1.0, N_RANDOM // 4)),
                            lo, hi, [0.0, 1e-300, -1e-300, -1000.0, 709.7, -708.0, -745.2],
                            rng.uniform(-745.2, -708.0, N_RANDOM // 4)])  # (710 -> inf: SPECIALS)
    elif name in ("log_lean", "log_any"):
        lo, hi = log_switch()
        x = np.concatenate([_loguniform(_rng("log"), 1e-300, 1e300), log_near_one(), lo, hi, [TINY, HUGE, 1.0, 2.0, 0.5]])
    elif name in ("pow_lean", "pow_any"):
        x = np.tile(_loguniform(_rng("pow"), 1e-6, 1e6, N_RANDOM // 2), len(POW_EXPONENTS))
        y = np.repeat(np.array(POW_EXPONENTS), N_RANDOM // 2)
        return x, y
    elif name == "sincos_small":
        x = _small_range(name, 0.8)
    elif name == "tan_small":
        x = _small_range(name, 0.5)
    elif name == "asin_small":
        x = _small_range(name, 0.3)
    elif name == "atan_small":
        x = _small_range(name, 0.1)
    elif name == "atan_01":
        lo, hi = atan_ties()
        x = np.concatenate([rng.uniform(0.0, 1.0, N_RANDOM), _loguniform(rng, 1e-12, 1.0, N_RANDOM // 4), lo, hi, [0.0, 1.0]])
    elif name == "atan2_any":
        # all four quadrants; |y| < |x| and |y| > |x| (both swaps) over twelve decades of the ratio
        m = _loguniform(rng, 1e-3, 1e3)
        ratio = _loguniform(rng, 1e-6, 1e6)
        sy, sx = rng.choice([-1.0, 1.0], N_RANDOM), rng.choice([-1.0, 1.0], N_RANDOM)
        ax = np.array(ATAN2_AXES)
        return np.concatenate([sy * m * ratio, ax[:, 0]]), np.concatenate([sx * m, ax[:, 1]])
    elif name == "asin_any":
        x = np.concatenate([rng.uniform(-1.0, 1.0, N_RANDOM), asin_near_one(rng), [1.0, -1.0, 0.0]])
    elif name in ("sincos_any", "tan_any"):
        x = np.concatenate([_rng("trig_any").uniform(-100.0, 100.0, N_RANDOM), quarter_turns()])
        if name == "tan_any":  # 1e-3 away from the poles (odd multiples of pi/2)
            h = x / (np.pi / 2.0)
            k = np.rint(h)
            x = x[~((k.astype(np.int64) % 2 == 1) & (np.abs(h - k) * (np.pi / 2.0) < 1e-3))]
    elif name == "cbrt_pos":
        x = _loguniform(rng, 1e-6, 1e6)
    elif name == "cbrt_any":
        x = np.concatenate([_both_signs(_loguniform(rng, 1e-320, 1e300, N_RANDOM // 2)), cbrt_exponents(), [-27.0, -8.0, 27.0, 8.0]])
    else:
        raise KeyError(name)
    return (np.ascontiguousarray(x, np.float64),)


# (routine, arguments, expected): asserted exactly — value and sign bit, or "is nan"
SPECIALS = (
    ("exp_lean", (-np.inf,), 0.0), ("exp_lean", (np.inf,), np.inf), ("exp_lean", (np.nan,), np.nan), ("exp_lean", (710.0,), np.inf),
    ("log_any", (0.0,), -np.inf), ("log_any", (-1.0,), np.nan), ("log_any", (np.inf,), np.inf),
    ("pow_any", (0.0, -0.32), np.inf), ("pow_any", (0.0, 0.5), 0.0),
    ("cbrt_any", (0.0,), 0.0), ("cbrt_any", (-0.0,), -0.0), ("cbrt_any", (np.inf,), np.inf), ("cbrt_any", (-np.inf,), -np.inf),
    ("cbrt_any", (np.nan,), np.nan),
    ("atan2_any", (-0.0, -1.0), -np.pi),
    ("asin_any", (1.0,), 1.5707963267948966), ("asin_any", (-1.0,), -1.5707963267948966),
    ("sqrt_nn", (0.0,), 0.0), ("sqrt_nn", (1e-281,), 0.0),
)


# ---- references ------------------------------------------------------------------------------------------------------
def _mp_atan2(y, x):
    """atan2 with the sign of y carried by a zero y (mpmath has no signed zero)."""
    a = mpmath.atan2(abs(y), x)
    return -a if np.signbit(float(y)) else a


def _mp_cbrt(x):
    return -mpmath.cbrt(-x) if x < 0 else mpmath.cbrt(x)


_MP = {
    "rcp64": lambda x: (1 / x,), "sqrt_pos": lambda x: (mpmath.sqrt(x),), "sqrt_nn": lambda x: (mpmath.sqrt(x),),
    "exp_lean": lambda x: (mpmath.exp(x),), "log_lean": lambda x: (mpmath.log(x),), "log_any": lambda x: (mpmath.log(x),),
    "pow_lean": lambda x, y: (mpmath.power(x, y),), "pow_any": lambda x, y: (mpmath.power(x, y),),
    "sincos_small": lambda x: (mpmath.sin(x), mpmath.cos(x)), "sincos_any": lambda x: (mpmath.sin(x), mpmath.cos(x)),
    "tan_small": lambda x: (mpmath.tan(x),), "tan_any": lambda x: (mpmath.tan(x),),
    "asin_small": lambda x: (mpmath.asin(x),), "asin_any": lambda x: (mpmath.asin(x),),
    "atan_small": lambda x: (mpmath.atan(x),), "atan_01": lambda x: (mpmath.atan(x),),
    "atan2_any": lambda y, x: (_mp_atan2(y, x),),
    "cbrt_pos": lambda x: (_mp_cbrt(x),), "cbrt_any": lambda x: (_mp_cbrt(x),),
}

# hi, lo as above; frac = (ref - hi) / ulp(hi), the same remainder in units of the spacing: lo itself cannot be held where hi
# is subnormal (it is below the smallest double), frac always can
Split = collections.namedtuple("Split", "hi lo frac")


def split(ref):
    """hi = float(ref), lo = float(ref - hi), frac = float((ref - hi) / ulp(hi)) of one mpmath value."""
    hi = float(ref)
    d = ref - mpmath.mpf(hi)
    if abs(d) > mpmath.mpf(TINY) / 2 and abs(hi) < MIN_NORMAL:  # (mpmath rounds a subnormal twice: take the nearest double)
        hi = float(np.nextafter(hi, np.inf if d > 0 else -np.inf))
        d = ref - mpmath.mpf(hi)
    return hi, float(d), float(d / mpmath.mpf(float(np.spacing(abs(hi)))))


def split_values(fn, args):
    """The Split arrays of fn(*args[i]) (a tuple of mpmath values) over the rows of the argument arrays."""
    with mpmath.workdps(DPS):
        rows = [[split(r) for r in fn(*(mpmath.mpf(float(a)) if a != 0 else float(a) for a in row))] for row in zip(*args)]
    out = np.array(rows, np.float64)  # (n, n_out, 3)
    return tuple(Split(*(out[:, k, j].copy() for j in range(3))) for k in range(out.shape[1]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per output of routine `name`: Split(hi, lo) float64 arrays over cases(name) — computed once per session."""
    key = {"log_any": "log_lean", "pow_any": "pow_lean"}.get(name)
    if key:  # (the same arguments and the same function)
        return reference(key)
    return split_values(_MP[name], cases(name))


# ---- the error measure ---------------------------------------------------------------------------------------------------
def ulp(hi):
    """The spacing of doubles at hi."""
    return np.spacing(np.abs(np.asarray(hi, np.float64)))


def ulp_error(got, ref):
    """|(got - hi) - lo| / ulp(hi), evaluated as |(got - hi) / ulp(hi) - frac|: got - hi is exact for a result near hi, the
    spacing is a power of two, and frac is lo / ulp(hi) without lo's underflow (tests/test_f64_math.py holds the two equal)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs((np.asarray(got, np.float64) - ref.hi) / ulp(ref.hi) - ref.frac)


def abs_error(got, ref):
    return ulp_error(got, ref) * ulp(ref.hi)


def violations(name, outs):
    """For the outputs `outs` (a tuple of float64 arrays over cases(name)) of routine `name` or of its library counterpart:
    (figures, bad) — `figures` a dict of the worst errors by label, `bad` the indices of the arguments outside the bound."""
    args, refs = cases(name), reference(name)
    figures, bad = {}, np.zeros(args[0].shape, bool)
    for k, (got, ref) in enumerate(zip(outs, refs)):
        tag = ("sin", "cos")[k] if len(refs) == 2 else "ulp"
        eu, ea = ulp_error(got, ref), abs_error(got, ref)
        wrong = ~np.isfinite(got)
        if name == "sincos_any":
            figures[tag + " abs"] = float(ea.max())
            wrong |= ea > SINCOS_ANY_ABS
        elif name == "exp_lean":
            sub = ref.hi < MIN_NORMAL  # (the spacing there is 2^-1074: eu is the absolute error in that unit)
            figures["ulp"] = float(eu[~sub].max())
            figures["subnormal abs / 2^-1074"] = float(eu[sub].max())
            wrong |= np.where(sub, eu > EXP_SUBNORMAL_ABS / TINY, eu > ULP_BOUND[name])
        elif name in ("pow_lean", "pow_any"):
            yl = np.abs(args[1] * np.log(args[0]))
            lim = POW_BOUND[0] + POW_BOUND[1] * yl
            i = int(np.argmax(eu / lim))
            figures["ulp"] = float(eu.max())
            figures["worst ulp / bound"] = float(eu[i] / lim[i])
            figures["at |y ln x|"] = float(yl[i])
            wrong |= eu > lim
        else:
            figures[tag] = float(eu.max())
            wrong |= eu > ULP_BOUND[name]
        bad |= wrong
    return figures, np.flatnonzero(bad)
