"""CPU side of the checks of csrc/wf_f64_math.h (tests/test_f64_math_gpu.py runs the routines): the hook library is built
and exports its launcher, the case generator yields every aimed point — and each aimed pair really straddles what it is
aimed at —, and the error measure counts half a spacing as 0.5 ulp."""
import math

import mpmath
import numpy as np
import pytest

import f64_math_cases as fc
import helpers


def test_hook_library_is_built_and_exports_the_launcher():
    lib = helpers.load_wfcheck()
    assert lib.wf_math_check.restype is not None
    # one id per routine of the header, distinct from the library's
    assert sorted(fc.IDS.values()) == list(range(19)) and set(fc.LIB_OF) == set(fc.IDS)
    assert not set(fc.IDS.values()) & set(fc.LIB_IDS.values()) and set(fc.LIB_OF.values()) == set(fc.LIB_IDS)


def test_ids_mirror_the_hook_source():
    import os
    import re

    src = open(os.path.join(os.path.dirname(helpers.WFCHECK_PATH), "csrc", "check", "wf_math_check.hip")).read()
    body = re.search(r"enum WfCheckFn : int \{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names, nxt = {}, 0
    for item in (s.strip() for s in body.split(",") if s.strip()):
        m = re.fullmatch(r"(\w+)(?:\s*=\s*(\d+))?", item)
        nxt = int(m.group(2)) if m.group(2) else nxt
        names[m.group(1)] = nxt
        nxt += 1
    want = {"WFC_" + n.upper(): i for n, i in fc.IDS.items()}
    want.update({"WFC_LIB_" + n.upper(): i for n, i in fc.LIB_IDS.items()})
    assert names == want


def _has(name, points, arg=0):
    return np.isin(np.asarray(points, np.float64), fc.cases(name)[arg]).all()


def test_generator_is_deterministic_and_sized():
    for name in fc.IDS:
        a = fc.cases(name)
        fc.cases.cache_clear()
        b = fc.cases(name)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), name
        assert 1000 <= a[0].size <= 12000 and all(x.shape == a[0].shape and np.isfinite(x).all() for x in a), name


def test_generator_yields_the_aimed_points():
    # powers of two with both neighbours
    for name, e in (("rcp64", 996), ("sqrt_pos", 929)):
        p = fc.powers_of_two(-e, e)
        assert _has(name, p) and _has(name, np.nextafter(p, 0.0)) and _has(name, np.nextafter(p, np.inf))
        assert (np.frexp(p)[0] == 0.5).all()
    assert _has("sqrt_nn", [1e-279]) and fc.cases("sqrt_nn")[0].min() > 1e-280
    assert ("sqrt_nn", (0.0,), 0.0) in fc.SPECIALS and ("sqrt_nn", (1e-281,), 0.0) in fc.SPECIALS
    # exp: both sides of every reduction tie, the ends, the subnormal results
    lo, hi = fc.exp_boundaries()
    assert lo.size == 2001 and _has("exp_lean", lo) and _has("exp_lean", hi)
    klo, khi = np.rint(lo * 1.4426950408889634), np.rint(hi * 1.4426950408889634)
    assert (np.abs(klo - khi) == 1).all()  # (the pair straddles the tie of rint(x / ln 2))
    assert _has("exp_lean", [0.0, 1e-300, -1e-300, -1000.0, 709.7, -708.0, -745.2])
    x = fc.cases("exp_lean")[0]
    assert ((x > -745.2) & (x < -709.0)).sum() >= 100 and x.min() == -1000.0 and x.max() == 709.7
    hi_ref = fc.reference("exp_lean")[0].hi
    assert ((hi_ref > 0) & (hi_ref < fc.MIN_NORMAL)).sum() >= 100 and hi_ref[x == -1000.0] == 0.0
    # log: 1 + d down to 1e-13, both sides of the mantissa switch at every exponent, the smallest and largest doubles
    for name in ("log_lean", "log_any"):
        assert _has(name, [1.0 + 1e-13, 1.0 - 1e-13, 1.1, 0.9, fc.TINY, fc.HUGE])
        lo, hi = fc.log_switch()
        assert lo.size == 41 and _has(name, lo) and _has(name, hi)
        mlo, elo = np.frexp(lo)
        mhi, ehi = np.frexp(hi)
        assert (mlo < fc.SQRT_HALF).all() and (mhi >= fc.SQRT_HALF).all() and (elo == ehi).all()
        assert set(elo) == set(range(-20, 21))
    assert fc.TINY == 5e-324 and fc.TINY / 2 == 0.0 and math.isinf(fc.HUGE * 2)
    # the small-range series: both ends
    for name, lim in (("sincos_small", 0.8), ("tan_small", 0.5), ("asin_small", 0.3), ("atan_small", 0.1)):
        x = fc.cases(name)[0]
        assert x.min() == -lim and x.max() == lim and _has(name, [0.0])
    # atan_01: both sides of every rint tie, 0 and 1
    lo, hi = fc.atan_ties()
    assert _has("atan_01", lo) and _has("atan_01", hi) and _has("atan_01", [0.0, 1.0])
    assert (np.rint(hi * 8.0) - np.rint(lo * 8.0) == 1).all() and set(np.rint(lo * 8.0)) == set(range(8))
    x = fc.cases("atan_01")[0]
    assert x.min() == 0.0 and x.max() == 1.0
    # atan2: four quadrants, both swaps, the axes, signed zeros
    y, x = fc.cases("atan2_any")
    for sy in (-1, 1):
        for sx in (-1, 1):
            q = (np.sign(y) == sy) & (np.sign(x) == sx)
            assert (q & (np.abs(y) > np.abs(x))).sum() > 50 and (q & (np.abs(y) < np.abs(x))).sum() > 50
    pairs = {(float(a), math.copysign(1.0, a), float(b), math.copysign(1.0, b)) for a, b in zip(y, x)}
    for a in (0.0, -0.0):
        for b in (1.0, -1.0):
            assert (a, math.copysign(1.0, a), b, math.copysign(1.0, b)) in pairs  # (+-0, +-1)
            assert (b, math.copysign(1.0, b), a, math.copysign(1.0, a)) in pairs  # (+-1, +-0)
    assert (0.0, 1.0, 0.0, 1.0) in pairs
    # asin_any: exactly +-1, 0, and every decade of 1 - |x| down to 1e-15
    x = fc.cases("asin_any")[0]
    assert _has("asin_any", [1.0, -1.0, 0.0]) and np.abs(x).max() == 1.0
    gap = 1.0 - np.abs(x)
    for d in range(1, 15):
        assert ((gap > 10.0 ** -(d + 1)) & (gap <= 10.0 ** -d)).sum() >= 10, d
    assert ((gap > 0) & (gap < 1e-8)).sum() >= 100  # (where the rounded product of the parent's radicand cancels)
    # sincos_any / tan_any: both sides of every multiple of pi/2; tan_any 1e-3 away from its poles
    q = fc.quarter_turns()
    assert q.size == 2 * 401 and _has("sincos_any", q) and np.abs(fc.cases("sincos_any")[0]).max() < 315.0
    t = fc.cases("tan_any")[0]
    k = np.arange(-199, 200, 2) * (np.pi / 2.0)
    assert np.abs(t[:, None] - k[None, :]).min() >= 1e-3
    even = np.arange(-200, 201, 2) * (np.pi / 2.0)
    assert _has("tan_any", even * (1.0 - 1e-13)) and _has("tan_any", even * (1.0 + 1e-13))
    assert t.size >= fc.cases("sincos_any")[0].size - 2 * 200 - 50
    # cbrt_any: every exponent residue mod 3 on both sides of 0, subnormals, both signs, the exact cubes
    x = fc.cases("cbrt_any")[0]
    e = np.frexp(np.abs(x))[1]
    for r in range(3):
        assert ((e % 3 == r) & (e < 0)).sum() > 10 and ((e % 3 == r) & (e > 0)).sum() > 10
        assert ((e % 3 == r) & (np.abs(x) < fc.MIN_NORMAL)).sum() >= 3
    assert _has("cbrt_any", [-27.0, -8.0, fc.TINY, -fc.TINY]) and (x < 0).sum() > 1000 and (x > 0).sum() > 1000
    # pow: the kernels' exponents, each over the whole range of x
    x, y = fc.cases("pow_any")
    assert set(y) == set(fc.POW_EXPONENTS) and -0.32 in fc.POW_EXPONENTS
    for p in fc.POW_EXPONENTS:
        assert x[y == p].min() < 1e-5 and x[y == p].max() > 1e5
    assert x.min() >= 1e-6 and x.max() <= 1e6


def test_error_measure_counts_half_a_spacing_as_half_an_ulp():
    with mpmath.workdps(fc.DPS):
        for base in (1.0, 1.5, 3.0e-5, 7.0e200, 2.0 ** -1040):
            step = float(np.spacing(base))
            ref = mpmath.mpf(base) + mpmath.mpf(step) / 4  # a quarter spacing above `base`
            hi, lo, frac = fc.split(ref)
            assert hi == base and frac == 0.25
            s = fc.Split(np.array([hi]), np.array([lo]), np.array([frac]))
            assert fc.ulp_error(np.array([base]), s)[0] == 0.25
            assert fc.ulp_error(np.array([base + step]), s)[0] == 0.75
            assert fc.ulp_error(np.array([base - step]), s)[0] == 1.25
            ref = mpmath.mpf(base) + mpmath.mpf(step) / 2  # half a spacing off either neighbour
            s = fc.Split(*(np.array([v]) for v in fc.split(ref)))
            assert fc.ulp_error(np.array([base]), s)[0] == 0.5 and fc.ulp_error(np.array([base + step]), s)[0] == 0.5
    # at a power of two the spacing is the one above it
    assert fc.ulp(1.0) == 2.0 ** -52 and fc.ulp(-4.0) == 2.0 ** -50 and fc.ulp(0.0) == fc.TINY


def test_reference_split_is_exact_and_cached():
    ref = fc.reference("asin_any")
    assert fc.reference("asin_any") is ref and fc.reference("log_any") is fc.reference("log_lean")
    (s,) = ref
    x = fc.cases("asin_any")[0]
    assert s.hi[x == 1.0] == 1.5707963267948966 and s.hi[x == -1.0] == -1.5707963267948966
    assert (np.abs(s.frac) <= 0.5).all()
    # frac is lo in units of the spacing wherever lo is a normal double: the measure is |(got - hi) - lo| / ulp(hi)
    ok = np.abs(s.lo) >= fc.MIN_NORMAL
    assert ok.sum() > 1000 and np.allclose(s.lo[ok] / fc.ulp(s.hi[ok]), s.frac[ok], rtol=1e-15, atol=0)
    # NumPy's own asin is within an ulp of it on [-1, 1]: the harness measures a correct routine as correct
    assert fc.ulp_error(np.arcsin(x), s).max() <= 1.0
    # and the parent's radicand, 1 - x * x rounded before the subtraction, is what the asin_any cases are aimed at
    near = (np.abs(x) < 1.0) & (1.0 - np.abs(x) < 1e-8)
    rad = np.maximum(1.0 - x[near] * x[near], 0.0)
    assert fc.ulp_error(np.arctan2(x[near], np.sqrt(rad)), fc.Split(*(v[near] for v in s))).max() > 100.0


@pytest.mark.parametrize("name", sorted(fc.IDS))
def test_bounds_accept_a_correctly_rounded_result_and_refuse_a_wrong_one(name):
    refs = fc.reference(name)
    exact = tuple(r.hi for r in refs)
    fig, bad = fc.violations(name, exact)
    assert bad.size == 0 and all(v <= 0.5 or "at" in k for k, v in fig.items()), fig
    # a relative error of 1e-9, far below the end-to-end tolerance, is refused on (nearly) every argument
    off = tuple(r.hi * (1.0 + 1e-9) + (1e-9 if name == "sincos_any" else 0.0) for r in refs)
    fig, bad = fc.violations(name, off)
    assert bad.size >= 0.9 * exact[0].size, (fig, bad.size)
