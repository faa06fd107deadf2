"""The portable math of include/chroma_fmath.h against float64 numpy."""
import numpy as np

import oracle


def ulp_err(got, exact):
    got = got.astype(np.float64)
    spacing = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return np.abs(got - exact) / spacing


def test_log_exp():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(1e-10, 1, 20000), rng.uniform(1, 1e6, 20000),
                        (np.arange(1, 2 ** 16, 7, dtype=np.float64) * 2.0 ** -32)]).astype(np.float32)
    assert ulp_err(oracle.math('log', x), np.log(x.astype(np.float64))).max() <= 2
    y = rng.uniform(-80, 80, 40000).astype(np.float32)
    assert ulp_err(oracle.math('exp', y), np.exp(y.astype(np.float64))).max() <= 2


def test_trig():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-7, 7, 40000), rng.uniform(-200, 200, 10000)]).astype(np.float32)
    x64 = x.astype(np.float64)
    for name, fn in (('sin', np.sin), ('cos', np.cos)):
        err = np.abs(oracle.math(name, x).astype(np.float64) - fn(x64))
        assert err.max() < 2e-7
    t = rng.uniform(-1.5, 1.5, 20000).astype(np.float32)
    assert ulp_err(oracle.math('tan', t), np.tan(t.astype(np.float64))).max() <= 4


def test_inverse_trig():
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-1, 1, 40000), [-1, 1, 0, 0.5, -0.5]]).astype(np.float32)
    x64 = x.astype(np.float64)
    assert np.abs(oracle.math('asin', x) - np.arcsin(x64)).max() < 3e-7
    assert np.abs(oracle.math('acos', x) - np.arccos(x64)).max() < 5e-7
    assert np.isnan(oracle.math('acos', np.array([1.5], np.float32))).all()
    y = rng.normal(size=20000).astype(np.float32)
    z = rng.normal(size=20000).astype(np.float32)
    assert np.abs(oracle.math('atan2', z, y) - np.arctan2(y.astype(np.float64), z.astype(np.float64))).max() < 5e-7


# ---------------------------------------------------------------------------
# The same header over the input sets of tests/fmath_cases.py (specials, branch
# thresholds, bit-pattern sweeps, worst-case windows).  The reference is float64
# libm (numpy, scipy), never the header itself.  Every bound below that the
# first three tests above do not already state is the maximum measured over
# these sets, rounded up to the next quarter ulp (absolute bounds: to the next
# 1e-8); the header's accuracy comment and DESIGN.md quote them.  Where a
# maximum lives in a bounded range, every float of that range is swept too
# (_every_float), so that no asserted maximum hangs on a stride; the arguments
# found there are kept in fmath_cases.WORST.
import json
import os
import re

import pytest

import fmath_cases as fc
from conftest import ROOT

try:
    import mpmath
except ImportError:      # test_worst_cases_high_precision then compares with float64 libm alone
    mpmath = None

F32_MAX = float(np.finfo(np.float32).max)
MIN_NORMAL = 2.0 ** -126


def _worst(err, x, mask):
    e = np.where(mask, err, -1.0)
    i = int(np.argmax(e))
    return float(e[i]), float(x[i]).hex()


def _check(label, err, x, mask, bound):
    """Print the largest err under mask and its argument, then assert the bound
    (err is a zero-argument function: evaluated with numpy's warnings off, NaN
    and inf being part of the sets)."""
    with np.errstate(all='ignore'):
        worst, at = _worst(err(), x, mask)
    print('%-32s %.6g at %s (n = %d), bound %g' % (label, worst, at, int(mask.sum()), bound))
    assert mask.any() and worst <= bound, (label, worst, at, bound)


def _every_float(label, op, fn, lo, hi, err, bound, negative=False):
    """The largest err(got, exact) over every float of [lo, hi) (of (-hi, -lo]
    with negative), a binade's worth at a time; printed, then held to bound.
    Returns the argument that attains it."""
    worst, at, n = -1.0, None, 0
    with np.errstate(all='ignore'):
        for start in range(fc.bit(lo), fc.bit(hi), 1 << 23):
            x = fc.f32(np.arange(start, min(start + (1 << 23), fc.bit(hi)), dtype=np.uint32))
            x = -x if negative else x
            e = err(oracle.math(op, x), fn(x.astype(np.float64)))
            i = int(np.argmax(e))
            n += len(x)
            if e[i] > worst:
                worst, at = float(e[i]), float(x[i]).hex()
    print('%-32s %.6g at %s (every float, n = %d), bound %g' % (label, worst, at, n, bound))
    assert n > 0 and worst <= bound, (label, worst, at, bound)
    return at


def _abs_err(got, exact):
    return np.abs(got.astype(np.float64) - exact)


def _one(op, fn):
    x, _ = fc.cases(op)
    with np.errstate(all='ignore'):
        return x, oracle.math(op, x), fn(x.astype(np.float64))


def test_present_bounds_hold_on_the_case_sets():
    """The bounds of the three tests above, unchanged, over the wider sets."""
    x, g, ex = _one('log', np.log)
    _check('log ulp', lambda: ulp_err(g, ex), x, (x > 0) & np.isfinite(x), 2)
    x, g, ex = _one('exp', np.exp)
    finite_result = np.isfinite(x) & (ex <= F32_MAX) & (x >= np.float32(-103.972084045))
    _check('exp ulp', lambda: ulp_err(g, ex), x, finite_result, 2)
    x, g, ex = _one('tan', np.tan)
    _check('tan ulp [-1.5, 1.5]', lambda: ulp_err(g, ex), x, np.abs(x) <= 1.5, 4)
    for op, fn in (('sin', np.sin), ('cos', np.cos)):
        x, g, ex = _one(op, fn)
        _check(op + ' abs |x| <= 200', lambda: np.abs(g - ex), x, np.abs(x) <= 200, 2e-7)
    x, g, ex = _one('asin', np.arcsin)
    _check('asin abs', lambda: np.abs(g - ex), x, np.abs(x) <= 1, 3e-7)
    x, g, ex = _one('acos', np.arccos)
    _check('acos abs', lambda: np.abs(g - ex), x, np.abs(x) <= 1, 5e-7)
    x, y = fc.cases('atan2')
    with np.errstate(all='ignore'):
        ex = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    _check('atan2 abs', lambda: np.abs(oracle.math('atan2', x, y) - ex), x, np.isfinite(ex), 5e-7)


def test_atan_bounds():
    x, g, ex = _one('atan', np.arctan)
    m = ~np.isnan(x)
    _check('atan ulp', lambda: ulp_err(g, ex), x, m, 3)
    _check('atan abs', lambda: np.abs(g - ex), x, m, 1.4e-7)
    # both branch thresholds and both maxima lie in [0.25, 4): 2.804 ulp, 1.399e-7
    at = _every_float('atan ulp [0.25, 4)', 'atan', np.arctan, 0.25, 4.0, ulp_err, 3)
    assert at in ('0x1.ba70360000000p-2',) and float.fromhex(at) in fc.worst('atan')
    _every_float('atan abs [0.25, 4)', 'atan', np.arctan, 0.25, 4.0, _abs_err, 1.4e-7)


def test_asin_acos_ulp_bounds():
    x, g, ex = _one('asin', np.arcsin)
    _check('asin ulp', lambda: ulp_err(g, ex), x, np.abs(x) <= 1, 2.5)
    x, g, ex = _one('acos', np.arccos)
    _check('acos ulp', lambda: ulp_err(g, ex), x, np.abs(x) <= 1, 1.5)
    # the maxima sit just above the 0.5 branch: 2.350, 1.282
    at = _every_float('asin ulp [0.25, 1)', 'asin', np.arcsin, 0.25, 1.0, ulp_err, 2.5)
    assert float.fromhex(at) in fc.worst('asin')
    _every_float('acos ulp [0.25, 1)', 'acos', np.arccos, 0.25, 1.0, ulp_err, 1.5)
    at = _every_float('acos ulp (-1, -0.25]', 'acos', np.arccos, 0.25, 1.0, ulp_err, 1.5, negative=True)
    assert float.fromhex(at) in fc.worst('acos')


def test_sin_cos_ulp_bounds_on_the_first_octant():
    for op, fn, bound in (('sin', np.sin, 0.75), ('cos', np.cos, 1.25)):
        x, g, ex = _one(op, fn)
        with np.errstate(all='ignore'):
            octant = (x >= 0) & (x.astype(np.float64) <= np.pi / 4)
        _check(op + ' ulp [0, pi/4]', lambda: ulp_err(g, ex), x, octant, bound)
        at = _every_float(op + ' ulp [0.25, pi/4]', op, fn, 0.25, np.float32(np.pi / 4), ulp_err, bound)   # 0.734, 1.241
        assert float.fromhex(at) in fc.worst(op)
    at = _every_float('tan ulp [0.25, 1.5)', 'tan', np.tan, 0.25, 1.5, ulp_err, 4)                          # 3.232
    assert float.fromhex(at) in fc.worst('tan')


def test_exp_subnormal_results_and_log_of_subnormals():
    x, g, ex = _one('exp', np.exp)
    m = (x >= np.float32(-103.972084045)) & (ex < MIN_NORMAL)
    assert m.sum() > 2000000          # every float of [-103.97, -87.34] is there
    _check('exp ulp, subnormal results', lambda: ulp_err(g, ex), x, m, 0.75)
    x, g, ex = _one('log', np.log)
    _check('log ulp, subnormal x', lambda: ulp_err(g, ex), x, (x > 0) & (x < MIN_NORMAL), 0.75)


# (lo, hi]: the bound of |sin - exact| and of |cos - exact| for lo < |x| <= hi.  Up to 1e5 the maxima
# are 9.3e-8 / 9.4e-8 (every float of [1, 1e5] tried once: 9.30e-8 / 9.31e-8); the last two rows are the
# maxima over every float, which test_sin_cos_absolute_error_at_large_arguments repeats
SINCOS_DECADES = ((0, 1, 1e-7, 1e-7), (1, 10, 1e-7, 1e-7), (10, 1e2, 1e-7, 1e-7), (1e2, 1e3, 1e-7, 1e-7),
                  (1e3, 1e4, 1e-7, 1e-7), (1e4, 1e5, 1e-7, 1e-7), (1e5, 1e6, 1.2e-7, 1e-7),
                  (1e6, float(fc.SINCOS_MAX), 7.81e-6, 9.4e-7))


def test_sin_cos_absolute_error_by_decade():
    """The three-term reduction's error grows with |x|: within 1e-7 up to 1e5,
    1.2e-7 up to 1e6, up to 8e-6 from there to CHR_SINCOS_MAX."""
    for col, (op, fn) in enumerate((('sin', np.sin), ('cos', np.cos))):
        x, g, ex = _one(op, fn)
        a = np.abs(x)
        for row in SINCOS_DECADES:
            _check('%s abs (%g, %g]' % (op, row[0], row[1]), lambda: np.abs(g - ex), x, (a > row[0]) & (a <= row[1]),
                   row[2 + col])


def test_sin_cos_absolute_error_at_large_arguments():
    """Every float of (1e5, CHR_SINCOS_MAX], where the error leaves 1e-7:
    1.147e-7 / 9.43e-8 up to 1e6, 7.803e-6 / 9.33e-7 beyond."""
    end = np.nextafter(fc.SINCOS_MAX, np.float32(np.inf))
    for col, (op, fn) in enumerate((('sin', np.sin), ('cos', np.cos))):
        for lo, hi, row in ((1e5, 1e6, SINCOS_DECADES[-2]), (1e6, end, SINCOS_DECADES[-1])):
            at = _every_float('%s abs [%g, %g)' % (op, lo, hi), op, fn, lo, hi, _abs_err, row[2 + col])
            assert float.fromhex(at) in fc.worst(op)


def test_erf_bound():
    """3.488e-7 at 0x1.0990cap-1, just above the 0.5 branch (Abramowitz & Stegun
    7.1.26 evaluated in float32), over every float of [0.5, 4): the header's
    comment says 3.5e-7.  Below 0.5 the series stays under 1e-7."""
    from scipy import special
    x, g, ex = _one('erf', special.erf)
    _check('erf abs', lambda: np.abs(g - ex), x, ~np.isnan(x), 3.5e-7)
    at = _every_float('erf abs [0.5, 4)', 'erf', special.erf, 0.5, 4.0, _abs_err, 3.5e-7)
    assert at == '0x1.0990ca0000000p-1' and float.fromhex(at) in fc.worst('erf')
    _every_float('erf abs [0.25, 0.5)', 'erf', special.erf, 0.25, 0.5, _abs_err, 1e-7)
    at = np.array([float.fromhex(at)], np.float32)
    assert abs(float(oracle.math('erf', at)[0]) - float(special.erf(np.float64(at[0])))) > 3.4e-7
    assert np.array_equal(oracle.erff(x).view(np.uint32), oracle.math_bits('erf', x))


HP_BOUNDS = {'atan': 3, 'asin': 2.5, 'acos': 1.5, 'sin': 0.75, 'cos': 1.25, 'tan': 4, 'exp': 0.75, 'log': 2}


@pytest.mark.parametrize('op', sorted(HP_BOUNDS))
def test_worst_cases_high_precision(op):
    """The 33 floats nearest each worst case against 40-digit mpmath: float64
    libm agrees with it to 1e-6 ulp of the float result there (so the maxima
    above are the header's error and not the reference's), and the bound holds
    against it too.  Without mpmath the bound is held against float64 libm."""
    x = fc.around(fc.worst(op), 16)
    x = x[np.abs(x) <= 1.5] if op in ('sin', 'cos', 'tan') else x
    if op in ('sin', 'cos'):
        x = x[(x >= 0) & (x <= 0.785)]
    f64 = getattr(np, {'atan': 'arctan', 'asin': 'arcsin', 'acos': 'arccos'}.get(op, op))(x.astype(np.float64))
    got = oracle.math(op, x)
    sp = np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
    assert len(x) >= 33
    if mpmath is None:
        assert (np.abs(got.astype(np.float64) - f64) / sp).max() <= HP_BOUNDS[op]
        return
    mpmath.mp.dps = 40
    for i in range(len(x)):
        exact = getattr(mpmath, op)(mpmath.mpf(float(x[i])))
        assert abs(mpmath.mpf(float(f64[i])) - exact) / float(sp[i]) < 1e-6
        assert abs(mpmath.mpf(float(got[i])) - exact) / float(sp[i]) <= HP_BOUNDS[op], (op, float(x[i]).hex())


# ------------------------------------------------------------------ special values, exactly
def _b(values):
    return np.asarray(values, np.float32).view(np.uint32)


INF, NAN = np.float32(np.inf), np.float32(np.nan)
PI, PIO2 = np.float32(np.pi), np.float32(np.pi / 2)


def test_log_specials():
    z = np.array([0.0, -0.0], np.float32)
    assert np.array_equal(_b(oracle.math('log', z)), _b([-INF, -INF]))
    neg = np.concatenate([fc.f32([0x80000001, 0x80800000]), np.array([-1.0, -F32_MAX, -INF], np.float32)])
    assert np.isnan(oracle.math('log', neg)).all()
    assert np.array_equal(_b(oracle.math('log', np.array([INF, 1.0], np.float32))), _b([INF, 0.0]))
    assert np.isnan(oracle.math('log', np.array([NAN], np.float32))).all()


def test_exp_specials():
    hi, lo = np.float32(88.7228393555), np.float32(-103.972084045)
    up, down = lambda v: np.nextafter(v, INF), lambda v: np.nextafter(v, -INF)
    got = oracle.math('exp', np.array([down(hi), hi, up(hi), INF], np.float32))
    assert np.isfinite(got[0]) and got[0] > 3.4027e38 and np.array_equal(_b(got[1:]), _b([INF, INF, INF]))
    got = oracle.math('exp', np.array([-INF, -F32_MAX, down(lo), lo, up(lo), 0.0, -0.0], np.float32))
    assert np.array_equal(_b(got), _b([0.0, 0.0, 0.0, 0.0, 2.0 ** -149, 1.0, 1.0]))
    assert np.isnan(oracle.math('exp', np.array([NAN], np.float32))).all()


def test_asin_acos_specials():
    x = np.array([1.0, -1.0, 0.0, -0.0], np.float32)
    assert np.array_equal(_b(oracle.math('asin', x)), _b([PIO2, -PIO2, 0.0, -0.0]))
    assert np.array_equal(_b(oracle.math('acos', x)), _b([0.0, PI, PIO2, PIO2]))
    h = np.array([0.5, -0.5], np.float32)
    # float(pi/6), float(pi/3), float(2 pi/3): the correctly rounded values, word for word
    assert [hex(w) for w in oracle.math_bits('asin', h)] == ['0x3f060a92', '0xbf060a92']
    assert [hex(w) for w in oracle.math_bits('acos', h)] == ['0x3f860a92', '0x40060a92']
    assert np.array_equal(oracle.math('asin', h), np.array([np.pi / 6, -np.pi / 6], np.float32))
    assert np.array_equal(oracle.math('acos', h), np.array([np.pi / 3, 2 * np.pi / 3], np.float32))
    assert np.array_equal(_b(oracle.math('asin', -h)), _b(-oracle.math('asin', h)))
    out = np.array([np.nextafter(np.float32(1), INF), -np.nextafter(np.float32(1), INF), 2.0, -F32_MAX, INF, -INF, NAN],
                   np.float32)
    assert np.isnan(oracle.math('asin', out)).all() and np.isnan(oracle.math('acos', out)).all()


def test_atan2_sign_zero_inf_combinations():
    """All sixteen (y, x) of {+0, -0, +inf, -inf}^2, and each of them against
    +-1, to 1 ulp of numpy's float result, the sign of a zero result included."""
    v = np.array([0.0, -0.0, np.inf, -np.inf], np.float32)
    w = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0], np.float32)
    y, x = (a.ravel() for a in np.meshgrid(w, w, indexing='ij'))
    assert sum(1 for a, b in zip(y, x) if a in v and b in v) == 16
    got = oracle.math('atan2', x, y)
    want = np.arctan2(y, x)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    assert np.array_equal(np.signbit(got), np.signbit(want)), (got, want)
    assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), (got, want)
    assert np.isnan(oracle.math('atan2', np.array([NAN, 1.0], np.float32), np.array([1.0, NAN], np.float32))).all()


def test_atan_specials():
    x = np.array([0.0, -0.0, INF, -INF], np.float32)
    assert np.array_equal(_b(oracle.math('atan', x)), _b([0.0, -0.0, PIO2, -PIO2]))
    assert np.isnan(oracle.math('atan', np.array([NAN], np.float32))).all()


def test_erf_specials():
    assert np.array_equal(_b(oracle.math('erf', np.array([0.0, -0.0], np.float32))), _b([0.0, -0.0]))
    big = np.concatenate([fc.around(np.float32(4.0), 64)[64:], np.array([5.0, 100.0, F32_MAX, INF], np.float32)])
    assert big[0] == 4.0
    assert np.array_equal(_b(oracle.math('erf', big)), _b(np.ones(len(big))))
    assert np.array_equal(_b(oracle.math('erf', -big)), _b(-np.ones(len(big))))
    assert np.isnan(oracle.math('erf', np.array([NAN], np.float32))).all()


def test_ldexp_is_ldexpf():
    """One rounding across both clamps: the named cases, then the whole set
    (k in [-300, 300], subnormal x and results) bit for bit against ldexpf."""
    want = {(1.0, -149): 2.0 ** -149, (1.0, -150): 0.0, (1.75, -149): 2.0 ** -148, (1.0, 128): np.inf,
            (1.0, 127): 2.0 ** 127, (3.0, -151): 2.0 ** -149, (0.5, 129): np.inf, (1.5, -126): 1.5 * 2.0 ** -126,
            (16777216.0, -173): 2.0 ** -149, (16777216.0, -174): 0.0,
            (2.0 ** -149, 276): 2.0 ** 127, (2.0 ** -149, 277): np.inf, (2.0 ** -140, 300): np.inf,
            (-(2.0 ** -127), 255): -np.inf}
    assert set(want) <= set(fc.LDEXP_NAMED)
    for (v, k), r in want.items():
        got = oracle.math('ldexp', np.array([v], np.float32), np.array([k], np.float32))
        assert np.array_equal(_b(got), _b([r])), (v, k, got)
    x, k = fc.cases('ldexp')
    with np.errstate(all='ignore'):
        ref = np.ldexp(x, k.astype(np.int32))
    assert ref.dtype == np.float32
    got = oracle.math_bits('ldexp', x, k)
    bad = np.flatnonzero(fc.canonical('ldexp', got) != fc.canonical('ldexp', ref.view(np.uint32)))
    assert len(bad) == 0, [(float(x[i]).hex(), int(k[i])) for i in bad[:5]]


def test_sat_u32():
    x = np.array([NAN, -0.0, 0.0, -1.0, -INF, -2.0 ** -149, 0.999, 1.0, 2.0 ** 32 - 256, 2.0 ** 32, 1e20, INF],
                 np.float32)
    want = np.array([0, 0, 0, 0, 0, 0, 0, 1, 2 ** 32 - 256, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1], np.uint32)
    assert np.array_equal(oracle.math('sat_u32', x), want)
    x, _ = fc.cases('sat_u32')
    with np.errstate(all='ignore'):
        ref = np.where(x > 0, np.minimum(np.floor(x.astype(np.float64)), 2.0 ** 32 - 1), 0.0).astype(np.uint32)
    assert np.array_equal(oracle.math('sat_u32', x), ref)


def test_ieee_primitives_on_the_host():
    """What the header rests on, as the oracle's build compiles it: correctly
    rounded sqrt, division and fma, subnormal operands and results included."""
    x, _ = fc.cases('sqrt')
    with np.errstate(all='ignore'):
        assert np.array_equal(fc.canonical('sqrt', oracle.math_bits('sqrt', x)),
                              fc.canonical('sqrt', np.sqrt(x).view(np.uint32)))
    x, y = fc.cases('div')
    with np.errstate(all='ignore'):
        assert np.array_equal(fc.canonical('div', oracle.math_bits('div', x, y)),
                              fc.canonical('div', (x / y).view(np.uint32)))
    x, y = fc.cases('fma')
    assert np.array_equal(fc.canonical('fma', oracle.math_bits('fma', x, y)),
                          fc.canonical('fma', fc.fma_x_y_x(x, y).view(np.uint32)))
    x, _ = fc.cases('rint_small')
    m = np.abs(x) < 2.0 ** 22
    assert m.sum() > 1000000 and np.array_equal(oracle.math('rint_small', x)[m], np.rint(x[m]))


# ------------------------------------------------------------------ the sincos domain
def test_sincos_domain():
    """|x| <= CHR_SINCOS_MAX: the largest float whose rounded product with
    two_over_pi is below 2^22 (chr_rintf_small's own condition); a sine and a
    cosine there, NaN beyond, and never a magnitude above 1."""
    text = open(os.path.join(ROOT, 'include', 'chroma_fmath.h')).read()
    lim = np.float32(re.search(r'#define CHR_SINCOS_MAX ([0-9.]+)f', text).group(1))
    two_over_pi = np.float32(re.search(r'two_over_pi = ([0-9.e+-]+)f', text).group(1))
    assert lim == fc.SINCOS_MAX
    assert np.float32(lim * two_over_pi) < 2.0 ** 22 <= np.float32(np.nextafter(lim, INF) * two_over_pi)
    assert float(lim) <= 2.0 ** 22 * np.pi / 2
    x, _ = fc.cases('sin')
    inside = np.abs(x) <= lim
    assert inside.sum() > 4000000 and (np.isfinite(x) & ~inside).sum() > 500000
    for op in ('sin', 'cos', 'tan'):
        g = oracle.math(op, x)
        assert np.isnan(g[~inside]).all(), op
        assert not np.isnan(g[inside]).any(), op
        if op != 'tan':
            assert np.abs(g[inside]).max() <= 1.0, op
    edge = np.array([lim, -lim], np.float32)
    assert np.abs(oracle.math('sin', edge) - np.sin(edge.astype(np.float64))).max() < 7.46e-6
    assert np.abs(oracle.math('cos', edge) - np.cos(edge.astype(np.float64))).max() < 7.46e-6


# ------------------------------------------------------------------ the bit pin
@pytest.mark.parametrize('op', fc.OPS)
def test_bits_pinned(op):
    """sha256 of the host's result words over op's whole input set (NaNs
    canonical, inputs outside the sincos domain left out) against
    tests/golden/fmath_bits.json: an edit of the header that moves one
    in-domain bit of this function fails here, by name."""
    with open(fc.GOLDEN) as f:
        pin = json.load(f)
    assert sorted(pin) == sorted(fc.OPS)
    x, y = fc.cases(op)
    assert len(x) == pin[op]['n']
    assert fc.digest(op, x, oracle.math_bits(op, x, y)) == pin[op]['sha256'], \
        '%s: bits of include/chroma_fmath.h moved' % op


def test_op_numbering_is_one_list():
    """enum chr_fmath_op (the device entry), oracle.MATH (the host entry) and
    fmath_cases.OPS name the same ops in the same order."""
    text = open(os.path.join(ROOT, 'include', 'chroma_amd.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'enum chr_fmath_op \{(.*?)\}', text, re.S).group(1), flags=re.S)
    names = [n.strip().split('=')[0].strip() for n in body.split(',')]
    assert names == ['CHR_FMATH_' + op.upper() for op in fc.OPS] + ['CHR_FMATH_NOPS']
    assert [oracle.MATH[op] for op in fc.OPS] == list(range(len(fc.OPS))) and len(oracle.MATH) == len(fc.OPS)
