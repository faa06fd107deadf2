"""The input sets of include/chroma_fmath.h's tests, shared by the host tests
(tests/test_fmath.py) and the device tests (tests/test_gpu_fmath.py).

Plain numpy, deterministic (no numpy random generator: a splitmix64 counter),
no GPU.  Per op of oracle.MATH / enum chr_fmath_op, cases(op) is (x, y): two
float32 arrays of equal length (y all zero for a one-argument op) made of

  specials     +-0, +-min/max subnormal, +-min normal, +-1, +-max finite, +-inf, a quiet NaN
  thresholds   every branch threshold of the function in the header with the
               64 floats on each side of it
  a sweep      bit patterns at an odd prime stride over the function's whole
               domain (a bounded domain more densely, a sparse sweep of all
               patterns beside it); log: every float of [1, 2); exp: every
               float of [-104, -87]
  worst cases  every float within 2048 of each argument where the function's
               error is largest (WORST)
  pairs        two-argument ops: 2^20 pairs of random bit patterns, 2^18 pairs
               uniform in [-1, 1)^2, the specials' cross product, and
               quotients that are subnormal, overflow or sit on chr_atanf's thresholds

`python tests/fmath_cases.py --write` rewrites tests/golden/fmath_bits.json
(one sha256 per op of the host's result words, see digest()) from the header
as it stands: to be run only when an in-domain bit is meant to move.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np

OPS = ('log', 'exp', 'sin', 'cos', 'tan', 'asin', 'acos', 'atan2', 'atan', 'erf', 'ldexp', 'sat_u32', 'rint_small',
       'sqrt', 'fma', 'div')
TWO_ARG = ('atan2', 'ldexp', 'fma', 'div')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fmath_bits.json')

# CHR_SINCOS_MAX (chroma_fmath.h): sin, cos and tan are defined for |x| <= this, NaN beyond
SINCOS_MAX = np.float32(6588397.0)
# full-range sweeps: 2^32 / 509 = 8.4 M patterns; bounded domains: stride 251; the sparse rest: 8191
STRIDE, STRIDE_DENSE, STRIDE_SPARSE = 509, 251, 8191
INF_BITS = 0x7f800000


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits_of(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bit(v):
    return int(np.float32(v).view(np.uint32))


SPECIALS = f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
                0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000])


def around(values, k=64):
    """Each value with the k floats on each side of it (stepping through 0 into
    the other sign, stopping at +-inf)."""
    b = bits_of(np.atleast_1d(np.asarray(values, dtype=np.float32))).astype(np.int64)
    o = np.where(b < 0x80000000, b, -(b & 0x7fffffff))          # monotone integer order of the floats
    o = (o[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).ravel()
    o = np.clip(o, -INF_BITS, INF_BITS)
    return f32(np.where(o >= 0, o, 0x80000000 | -o).astype(np.uint32))


def sweep(lo_bits, hi_bits, stride, both_signs=False):
    """The floats of bit patterns lo_bits, lo_bits + stride, ... < hi_bits."""
    b = np.arange(lo_bits, hi_bits, stride, dtype=np.int64).astype(np.uint32)
    if both_signs:
        b = np.concatenate([b, b | np.uint32(0x80000000)])
    return f32(b)


def splitmix(n, seed):
    """n 64-bit words of splitmix64 from the counter seed, seed + 1, ..."""
    with np.errstate(over='ignore'):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _pm(values):
    v = np.asarray(values, dtype=np.float32)
    return np.concatenate([v, -v])


def _pio4_odd():
    """The odd multiples of pi/4 up to 64, as the nearest floats: where the
    reduction's quadrant changes."""
    k = np.arange(1, 83, 2, dtype=np.float64)
    v = k * (np.pi / 4)
    return v[v <= 64.0].astype(np.float32)


# per one-argument op: (thresholds around which 64 floats a side are taken, sweeps)
def _one_arg(op):
    full = lambda stride: sweep(0, 1 << 32, stride)
    if op == 'log':
        thr = f32([0x3f3504f3, 0x3fb504f3, 0x3eb504f3, 0x3f800000, 0x00800000])
        # every float of [1, 2); the rest of the patterns at twice the stride (12.6 M in all)
        return thr, [full(2 * STRIDE + 3), sweep(0x3f800000, 0x40000000, 1)]
    if op == 'exp':
        thr = np.array([88.7228393555, -103.972084045, -87.33654475, 0.0], np.float32)
        return thr, [full(STRIDE), sweep(bit(-87.0), bit(-104.0) + 1, 1)]
    if op in ('sin', 'cos', 'tan'):
        lim = bit(SINCOS_MAX)
        thr = np.concatenate([_pm(_pio4_odd()), around(_pm([SINCOS_MAX]), 4)])
        return thr, [sweep(0, lim + 1, STRIDE, both_signs=True), full(4 * STRIDE + 3)]
    if op in ('asin', 'acos'):
        thr = _pm([1e-4, 0.5, 1.0])
        return thr, [sweep(0, 0x3f800000 + 1, STRIDE_DENSE, both_signs=True), full(STRIDE_SPARSE)]
    if op == 'atan':
        return _pm([0.41421356, 2.41421356]), [full(STRIDE)]
    if op == 'erf':
        return _pm([0.5, 4.0]), [sweep(0, bit(5.0), STRIDE_DENSE, both_signs=True),
                                 full(STRIDE_SPARSE)]
    if op == 'sat_u32':
        return np.array([1.0, 16777216.0, 2147483648.0, 4294967296.0], np.float32), [full(STRIDE)]
    if op == 'rint_small':
        return _pm([0.5, 1.5, 2.5, 4194304.0, 8388608.0, 12582912.0]), [full(STRIDE)]
    if op == 'sqrt':
        return f32([0x00800000, 0x3f800000, 0x40000000, 0x40800000]), [full(STRIDE)]
    raise KeyError(op)


def _uniform_pairs(n, seed):
    """n pairs uniform in [-1, 1)^2 on a 2^-23 grid."""
    z = splitmix(n, seed)
    a = ((z >> np.uint64(40)).astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32)
    b = (((z >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.float64) / 2.0 ** 23 - 1.0).astype(np.float32)
    return a, b


def _random_pairs(n, seed):
    z = splitmix(n, seed)
    return f32((z >> np.uint64(32)).astype(np.uint32)), f32((z & np.uint64(0xffffffff)).astype(np.uint32))


def _cross(a, b):
    return np.repeat(a, len(b)), np.tile(b, len(a))


def _quotient_pairs():
    """(numerator, denominator) whose quotient is subnormal, overflows, or is
    exactly a float beside one of chr_atanf's two thresholds (the denominator a
    power of two, so the division is exact)."""
    e = np.arange(-20, 21, dtype=np.float64)
    thr = around(np.array([0.4142135623730950, 2.414213562373095], np.float32), 2).astype(np.float64)
    num, den = _cross(thr, 2.0 ** e)
    num = num * den
    m = np.concatenate([[1.0, 1.5, 1.9999999], 1.0 + np.arange(1, 64) / 64.0])
    sub_num, sub_den = _cross(m * 2.0 ** -100, 2.0 ** np.arange(27, 51, dtype=np.float64))    # 2^-127 .. 2^-150
    ovf_num, ovf_den = _cross(m * 2.0 ** 100, 2.0 ** -np.arange(26, 30, dtype=np.float64))    # around 2^128
    num = np.concatenate([num, sub_num, ovf_num]).astype(np.float32)
    den = np.concatenate([den, sub_den, ovf_den]).astype(np.float32)
    return np.concatenate([num, -num, num, -num]), np.concatenate([den, den, -den, -den])


# where each function's error against float64 libm is largest (tests/test_fmath.py asserts the bounds):
# the arguments found by sweeps of every float of the bounded ranges (tests/test_fmath.py repeats them),
# by the strided sweeps above and by an independent stride-37 sweep; each is taken with
# the WORST_K floats on each side of it, so that the asserted maxima do not hang on one stride
# sin / cos on the first octant, tan, and sin / cos absolute error in (1e5, 1e6] and (1e6, CHR_SINCOS_MAX]
_TRIG_WORST = ('0x1.9205aap-1', '0x1.91baf2p-1', '0x1.76e054p-1', '0x1.9070e4p-1', '0x1.51252ap+0', '0x1.4dcf2ap+0',
               '0x1.e62e28p+19', '0x1.ee725p+17', '0x1.8f0bep+22', '0x1.8d60c4p+22')
WORST = {
    'atan': ('0x1.ba7036p-2', '0x1.c4e7fep-2', '0x1.bc3206p-2', '0x1.4560ep+1', '-0x1.4d0aaap+1'),
    'asin': ('0x1.0020a6p-1', '0x1.01312cp-1', '0x1.01ab8ap-1', '0x1.be7ff2p-1', '0x1.b8f7fcp-1'),
    'acos': ('-0x1.007356p-1', '-0x1.01312cp-1', '-0x1.01ab8ap-1', '0x1.3ce1b6p-1'),
    'erf': ('0x1.0990cap-1', '0x1.0dd0ccp-1', '0x1.067774p-1'),
    'sin': _TRIG_WORST, 'cos': _TRIG_WORST, 'tan': _TRIG_WORST,
    'exp': ('-0x1.601e0ap+6',),
    'log': ('0x1.67cc32p+0', '0x1.855b2p-129'),
}
WORST_K = 2048


def worst(op):
    return np.array([float.fromhex(h) for h in WORST.get(op, ())], np.float32)


# the inputs of special values the tests pin by name, and inputs kept because a build once got them wrong
LDEXP_NAMED = ((1.0, -149), (1.0, -150), (1.75, -149), (1.0, 128), (1.0, 127), (1.5, -126), (1.0, -126), (1.0, -127),
               (3.0, -151), (0.5, 129), (16777216.0, -173), (16777216.0, -174),
               # a subnormal x with k > 254: chr_ldexpf once clamped k after a single factor of 2^127
               (2.0 ** -149, 276), (2.0 ** -149, 277), (2.0 ** -140, 300), (-(2.0 ** -127), 255))


def _two_arg(op):
    ra, rb = _random_pairs(1 << 20, seed=0x1000 + OPS.index(op))
    ua, ub = _uniform_pairs(1 << 18, seed=0x2000 + OPS.index(op))
    if op == 'ldexp':
        k = (splitmix(1 << 20, seed=77) % np.uint64(601)).astype(np.float32) - np.float32(300)
        sx, sk = _cross(SPECIALS, np.arange(-300, 301, dtype=np.float32))
        nx, nk = (np.array(v, np.float32) for v in zip(*LDEXP_NAMED))
        return np.concatenate([ra, ua, sx, nx]), np.concatenate([k, k[:len(ua)], sk, nk])
    sa, sb = _cross(SPECIALS, SPECIALS)
    qn, qd = _quotient_pairs()
    if op == 'atan2':     # x is the second argument of chr_atan2f(y, x): the quotient is y / x
        return np.concatenate([ra, ua, sa, qd]), np.concatenate([rb, ub, sb, qn])
    return np.concatenate([ra, ua, sa, qn]), np.concatenate([rb, ub, sb, qd])


@functools.lru_cache(maxsize=2)
def cases(op):
    """(x, y) float32 arrays of op's inputs; read-only."""
    if op in TWO_ARG:
        x, y = _two_arg(op)
    else:
        thr, sweeps = _one_arg(op)
        x = np.concatenate([SPECIALS, around(thr), around(worst(op), WORST_K)] + sweeps)
        y = np.zeros_like(x)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert x.shape == y.shape
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def in_domain(op, x):
    """False where x is outside op's documented domain with an unpinned result:
    finite |x| > CHR_SINCOS_MAX for sin, cos and tan (NaN since the limit
    exists, garbage before).  These inputs are left out of the digests."""
    if op in ('sin', 'cos', 'tan'):
        return ~(np.isfinite(x) & (np.abs(x) > SINCOS_MAX))
    return np.ones(len(x), bool)


def canonical(op, bits):
    """Result words with every NaN replaced by 0x7fc00000 (a NaN's sign and
    payload are not part of the contract; sat_u32's words are integers)."""
    if op == 'sat_u32':
        return bits
    return np.where((bits & np.uint32(0x7fffffff)) > np.uint32(INF_BITS), np.uint32(0x7fc00000), bits)


def digest(op, x, bits):
    """sha256 of op's in-domain result words, NaNs canonical, little endian."""
    words = canonical(op, np.asarray(bits, np.uint32))[in_domain(op, x)]
    return hashlib.sha256(words.astype('<u4').tobytes()).hexdigest()


def fma_x_y_x(x, y):
    """fmaf(x, y, x) correctly rounded, from float64: the product is exact
    there, the sum is taken with round-to-odd (TwoSum gives the error's sign),
    and rounding that to float32 is then a single rounding."""
    with np.errstate(all='ignore'):
        p = x.astype(np.float64) * y.astype(np.float64)
        a = x.astype(np.float64)
        s = p + a
        t = s - p
        e = (p - (s - t)) + (a - t)                                # s + e == p + a exactly
        inexact = np.isfinite(s) & (e != 0)
        b = s.view(np.int64).copy()
        b[inexact & ((e > 0) != (s > 0))] -= 1                     # truncate towards zero ...
        b[inexact] |= 1                                            # ... and make the last bit sticky
        return b.view(np.float64).astype(np.float32)


def host_digests():
    import oracle
    out = {}
    for op in OPS:
        x, y = cases(op)
        out[op] = {'n': int(len(x)), 'sha256': digest(op, x, oracle.math_bits(op, x, y))}
    return out


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
    with open(GOLDEN, 'w') as f:
        json.dump(host_digests(), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s' % GOLDEN)
