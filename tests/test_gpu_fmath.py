"""include/chroma_fmath.h on the device against the same header on the host,
bit for bit.

Every parity test of the suite (photons, PDFs, gensteps, the library) rests
on the header's claim that gfx950 and the gcc-built oracle compute the same
bits.  This module tests the claim itself: per function one launch of
chr_selftest_fmath (csrc/selftest.hip) over the function's whole input set of
tests/fmath_cases.py -- specials, every branch threshold with 64 floats a
side, bit-pattern sweeps of the domain, worst-case windows -- compared with
the oracle's orc_math_bits over the same inputs.  tests/test_fmath.py holds
the host side to float64 libm and to a pinned digest, so equality here puts
the device under the same bounds.

NaNs: the comparison is bit for bit wherever either side is not a NaN; where
one side is a NaN the other must be one too, and a NaN's sign and payload are
not compared.  They are no part of the header's contract and the targets differ
by design: inf - inf (the x - x the header once returned for a non-finite sine
argument, and what every inf / inf and 0 * inf below evaluates) is 0xffc00000
on x86 and the default NaN 0x7fc00000 on gfx950.
"""
import numpy as np
import pytest

import fmath_cases as fc

pytestmark = pytest.mark.gpu

SENTINEL = 0xdeadbeef


def _device_bits(op, x, y, pad=0):
    """The device's result words of op over (x, y); pad: words allocated beyond
    len(x), preset to SENTINEL and returned too."""
    import oracle
    from chroma.gpu import _native
    from chroma.gpu import gpuarray as ga
    from chroma.gpu.tools import current_stream
    dx, dy = ga.to_gpu(np.array(x)), ga.to_gpu(np.array(y))     # writable copies: the sets are shared and read-only
    out = ga.empty(len(x) + pad, np.uint32).fill(SENTINEL)
    _native.call('chr_selftest_fmath', oracle.MATH[op], len(x), dx.gpudata, dy.gpudata, out.gpudata, current_stream())
    return out.get()            # synchronises; dx, dy and out are alive until here


def _assert_same_bits(op, x, y, got, want):
    if op != 'sat_u32':         # its words are integers
        gn, wn = (((b & 0x7fffffff) > 0x7f800000) for b in (got, want))
        bad = np.flatnonzero(gn != wn)
        assert len(bad) == 0, ('%s: NaN on one side only' % op,
                               [(float(x[i]).hex(), float(y[i]).hex(), hex(got[i]), hex(want[i])) for i in bad[:5]])
        got, want = np.where(gn, 0, got), np.where(wn, 0, want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, ('%s: %d of %d words differ' % (op, len(bad), len(x)),
                           [(float(x[i]).hex(), float(y[i]).hex(), hex(got[i]), hex(want[i])) for i in bad[:5]])


@pytest.mark.parametrize('op', fc.OPS)
def test_device_bits_equal_host_bits(op):
    import oracle
    x, y = fc.cases(op)
    got = _device_bits(op, x, y)
    _assert_same_bits(op, x, y, got, oracle.math_bits(op, x, y))
    if op in ('sin', 'cos', 'tan'):     # beyond CHR_SINCOS_MAX: NaN, not a quadrant the two targets pick differently
        outside = ~(np.abs(x) <= fc.SINCOS_MAX)
        assert outside.sum() > 500000 and ((got[outside] & 0x7fffffff) > 0x7f800000).all()


def test_ieee_primitives_are_correctly_rounded_on_the_device():
    """sqrt, division and fma as the library's flags compile them for gfx950,
    against numpy's float32 sqrt and /, and against fmaf worked out from float64
    (the oracle's fmaf is the parametrised case above): correct rounding with
    subnormal operands and results, no flush to zero, no reciprocal shortcut.
    rint_small against rint on its domain."""
    with np.errstate(all='ignore'):
        x, y = fc.cases('sqrt')
        _assert_same_bits('sqrt', x, y, _device_bits('sqrt', x, y), np.sqrt(x).view(np.uint32))
        x, y = fc.cases('div')
        sub = np.abs(x / y) < np.float32(2.0 ** -126)
        assert (sub & (x / y != 0)).sum() > 1000
        _assert_same_bits('div', x, y, _device_bits('div', x, y), (x / y).view(np.uint32))
        x, y = fc.cases('fma')
        _assert_same_bits('fma', x, y, _device_bits('fma', x, y), fc.fma_x_y_x(x, y).view(np.uint32))
    x, y = fc.cases('rint_small')
    m = np.abs(x) < 2.0 ** 22
    got = _device_bits('rint_small', x, y).view(np.float32)
    assert np.array_equal(got[m], np.rint(x[m]))


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_block_edge(n):
    """One work-item per element in blocks of 256: exactly n words are written."""
    import oracle
    x = fc.cases('atan')[0][1000:1000 + n]
    got = _device_bits('atan', x, np.zeros_like(x), pad=300)
    assert np.array_equal(got[:n], oracle.math_bits('atan', x))
    assert (got[n:] == SENTINEL).all()


def test_bad_arguments():
    from chroma.gpu import _native
    from chroma.gpu import gpuarray as ga
    from chroma.gpu.tools import current_stream
    x = ga.to_gpu(np.ones(4, np.float32))
    out = ga.empty(4, np.uint32).fill(SENTINEL)
    s = current_stream()
    for op in (-1, len(fc.OPS), 1000):
        with pytest.raises(_native.NativeError, match='unknown op'):
            _native.call('chr_selftest_fmath', op, 4, x.gpudata, x.gpudata, out.gpudata, s)
    for args in ((None, x.gpudata, out.gpudata), (x.gpudata, None, out.gpudata), (x.gpudata, x.gpudata, None)):
        with pytest.raises(_native.NativeError, match='null'):
            _native.call('chr_selftest_fmath', 0, 4, *args, s)
    _native.call('chr_selftest_fmath', 0, 0, None, None, None, s)      # n == 0: nothing to do
    assert (out.get() == SENTINEL).all()
