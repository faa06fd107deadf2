"""What the photon-library tests share: a numpy restatement of both lookup rules
(include/chroma_amd.h, "photon library") -- the expected words never come from
the code under test --, down to the generator, chr_expf, chr_logf, chr_sincosf
and chr_normal in float32 with an exactly rounded fmaf, and the made libraries
and events.  The sampled rule runs vectorised over the work-items, each lane
with its own generator state, so a lane's draws come in the order the rule
gives them."""
from types import SimpleNamespace

import numpy as np

f32, u32, u64 = np.float32, np.uint32, np.uint64
NO_KEY = u32(0xFFFFFFFF)
NO_SOURCE = 0xFFFFFFFF
MAX_TIME_DRAWS = 64
MAX_FACTORS = 1024
NO_HIT_TIME = f32(1e9)
INF = f32(np.inf)

# ---------------------------------------------------------------- float32 arithmetic


def fmaf(a, b, c):
    """fmaf of float32 arrays, exactly rounded: the product is exact in float64, the
    sum is brought to round-to-odd with its TwoSum error, and the float32 rounding
    of a round-to-odd float64 (29 spare bits) is the rounding of the exact value."""
    a, b, c = np.broadcast_arrays(*[np.asarray(x, f32).astype(np.float64) for x in (a, b, c)])
    with np.errstate(all='ignore'):
        p = a * b
        s = np.atleast_1d(p + c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32).reshape(np.shape(p))


def bits(x):
    return np.ascontiguousarray(x, f32).view(u32)


def from_bits(b):
    return np.ascontiguousarray(b, u32).view(f32)


def rint_small(x):
    magic = f32(12582912.0)
    return (x + magic) - magic


def expf(x):
    """chr_expf where its result is a normal float32 (the rule's -32 < x <= 0)."""
    x = np.atleast_1d(np.asarray(x, f32))
    assert ((x > -87.0) & (x < 88.0)).all()
    ln2_hi, ln2_lo, inv_ln2 = f32(6.9314575195e-01), f32(1.4286067653e-06), f32(1.4426950216e+00)
    P1, P2 = f32(1.6666625440e-1), f32(-2.7667332906e-3)
    kf = rint_small(x * inv_ln2)
    k = kf.astype(np.int64)
    hi = fmaf(-kf, ln2_hi, x)
    lo = kf * ln2_lo
    r = hi - lo
    rr = r * r
    c = r - rr * fmaf(rr, P2, P1)
    y = f32(1.0) - ((lo - (r * c) / (f32(2.0) - c)) - hi)
    return y * from_bits(((k + 127) << 23).astype(u32))


def logf(x):
    """chr_logf of normal positive float32."""
    x = np.atleast_1d(np.asarray(x, f32))
    assert ((x >= f32(1.1754944e-38)) & np.isfinite(x)).all()
    ln2_hi, ln2_lo = f32(6.9313812256e-01), f32(9.0580006145e-06)
    L1, L2, L3, L4 = f32(0.66666662693), f32(0.40000972152), f32(0.28498786688), f32(0.24279078841)
    ix = bits(x) + u32(0x3f800000 - 0x3f3504f3)
    k = (ix >> u32(23)).astype(np.int64) - 127
    ix = (ix & u32(0x007fffff)) + u32(0x3f3504f3)
    f = from_bits(ix) - f32(1.0)
    s = f / (f32(2.0) + f)
    z = s * s
    w = z * z
    t1 = w * fmaf(w, L4, L2)
    t2 = z * fmaf(w, L3, L1)
    R = t2 + t1
    hfsq = f32(0.5) * f * f
    dk = k.astype(f32)
    return fmaf(s, hfsq + R, dk * ln2_lo) - hfsq + f + dk * ln2_hi


def sincosf(x):
    """chr_sincosf of finite float32 within the reduction's range."""
    x = np.atleast_1d(np.asarray(x, f32))
    n = rint_small(x * f32(6.3661974669e-01))
    y = fmaf(-n, f32(1.5707963705062866e+00), x)
    y = fmaf(-n, f32(-4.3711388286737929e-08), y)
    y = fmaf(-n, f32(-1.7151245100059665e-15), y)
    z = y * y
    ps = fmaf(fmaf(f32(-1.9515295891e-4), z, f32(8.3321608736e-3)), z, f32(-1.6666654611e-1))
    sr = fmaf(y * z, ps, y)
    pc = fmaf(fmaf(f32(2.443315711809948e-5), z, f32(-1.388731625493765e-3)), z, f32(4.166664568298827e-2))
    cr = fmaf(z * z, pc, fmaf(f32(-0.5), z, f32(1.0)))
    q = n.astype(np.int64) & 3
    s = np.select([q == 0, q == 1, q == 2], [sr, cr, -sr], -cr)
    c = np.select([q == 0, q == 1, q == 2], [cr, -sr, -cr], sr)
    return s.astype(f32), c.astype(f32)


def sat_u32(x):
    """chr_sat_u32"""
    x = np.atleast_1d(np.asarray(x, f32))
    with np.errstate(invalid='ignore'):
        zero = ~(x > 0)
        top = ~zero & (x >= f32(4294967296.0))
        out = np.where(zero | top, f32(0), x).astype(u64).astype(u32)
    out[top] = 0xFFFFFFFF
    return out


# ---------------------------------------------------------------- the generator, one state per lane
class Lanes(object):
    """XORWOW states (6, n) uint32, rows d, v0..v4: chr_xorwow_next, chr_uniform01
    and chr_normal for the lanes of a mask; the other lanes stay as they are."""

    def __init__(self, states):
        self.s = np.array(states, u32).reshape(6, -1)

    def next(self):
        d, v0, v1, v2, v3, v4 = self.s
        t = v0 ^ (v0 >> u32(2))
        new4 = (v4 ^ (v4 << u32(4))) ^ (t ^ (t << u32(1)))
        d = d + u32(362437)
        self.s = np.stack([d, v1, v2, v3, v4, new4])
        return new4 + d

    def uniform01(self):
        return self.next().astype(f32) * f32(2.3283064365386963e-10) + f32(1.1641532182693481e-10)

    def normal_pair(self):
        """Both values of one Box-Muller draw: (returned now, cached)."""
        x, y = self.next(), self.next()
        u = x.astype(f32) * f32(2.3283064365386963e-10) + f32(1.1641532182693481e-10)
        v = y.astype(f32) * f32(1.4629180792671596e-09) + f32(7.3145903963357980e-10)
        r = np.sqrt(f32(-2.0) * logf(u)).astype(f32)
        sv, cv = sincosf(v)
        return sv * r, cv * r


def time_of_key(key):
    key = np.asarray(key, u32)
    return from_bits(np.where(key >> u32(31) == 1, key ^ u32(0x80000000), key ^ u32(0xFFFFFFFF)).astype(u32))


# ---------------------------------------------------------------- the rules
def _entry_of(lib, en, i):
    """(counts?, w) of entry i: None when it adds nothing."""
    s = int(en.source[i])
    if s >= lib.nsources or int(lib.emitted[s]) == 0:
        return None, None
    w = np.asarray(en.nphotons[i], u32).astype(f32) / np.asarray(lib.emitted[s], u64).astype(f32)
    return s, f32(w)


def numpy_expect(lib, en):
    """mu, tfirst (None without tmin), skipped of the expected-value rule."""
    nch = lib.nchannels
    mu = np.zeros((en.nevents, nch), f32)
    tfirst = np.full((en.nevents, nch), INF, f32) if lib.tmin is not None else None
    nan_candidates = 0
    for e in range(en.nevents):
        for i in range(int(en.offsets[e]), int(en.offsets[e + 1])):
            s, w = _entry_of(lib, en, i)
            if s is None:
                continue
            k = lib.counts[s * nch:(s + 1) * nch]
            mu[e] = fmaf(w, k.astype(f32), mu[e])
            if tfirst is not None:
                key = lib.tmin[s * nch:(s + 1) * nch]
                with np.errstate(invalid='ignore'):
                    cand = f32(en.t[i]) + time_of_key(key)
                    take = (k > 0) & (key != NO_KEY)
                    nan_candidates += int((take & np.isnan(cand)).sum())
                    take &= cand < tfirst[e]
                tfirst[e][take] = cand[take]
    sources = en.source[int(en.offsets[0]):int(en.offsets[-1])]
    return SimpleNamespace(mu=mu, tfirst=tfirst, skipped=int((sources >= lib.nsources).sum()),
                           nan_candidates=nan_candidates)


def numpy_sample(lib, en, rng_states, nslots):
    """n, t, the states afterwards and skipped of the sampled rule, with counts of
    what happened on the way (`stats`)."""
    nch, tb = lib.nchannels, lib.tbins
    npairs = en.nevents * nch
    T = min(nslots, npairs)
    states = np.array(rng_states, u32).reshape(6, nslots)
    n_out, t_out = np.zeros(npairs, u32), np.zeros(npairs, f32)
    stats = dict(knuth=0, normal=0, capped=0, saturated=0, cache_used=0, empty_hist=0)
    lengths = np.diff(en.offsets.astype(np.int64))
    width = f32(1.0) / f32(lib.inv) if tb else f32(0)
    rounds = (npairs + T - 1) // T if T else 0
    for rnd in range(rounds):
        pair = np.arange(T, dtype=np.int64) + rnd * T
        live = np.flatnonzero(pair < npairs)                # a prefix of the lanes
        pair = pair[live]
        e, c = pair // nch, pair % nch
        n = np.zeros(len(live), u32)
        mu = np.zeros(len(live), f32)
        tfirst = np.full(len(live), INF, f32)
        tdrawn = np.full(len(live), INF, f32)
        flag = np.zeros(len(live), bool)
        extra = np.zeros(len(live), f32)
        for pos in range(int(lengths[e].max()) if len(live) else 0):
            on = np.flatnonzero(pos < lengths[e])
            i = en.offsets[e[on]].astype(np.int64) + pos
            s = en.source[i].astype(np.int64)
            ok = s < lib.nsources
            ok[ok] = lib.emitted[s[ok]] != 0
            on, i, s = on[ok], i[ok], s[ok]
            if not len(on):
                continue
            w = en.nphotons[i].astype(f32) / lib.emitted[s].astype(f32)
            word = s * nch + c[on]
            k = lib.counts[word]
            t = en.t[i]
            # the expected values on the way (tfirst is the pair's time without a histogram)
            mu[on] = fmaf(w, k.astype(f32), mu[on])
            if lib.tmin is not None:
                key = lib.tmin[word]
                with np.errstate(invalid='ignore'):
                    cand = t + time_of_key(key)
                    take = (k > 0) & (key != NO_KEY) & (cand < tfirst[on])
                tfirst[on[take]] = cand[take]
            with np.errstate(over='ignore'):
                m = w * k.astype(f32)
            ni = np.zeros(len(on), u32)
            rng = Lanes(states[:, live[on]])
            # Knuth's product
            small = np.flatnonzero((m > 0) & (m < f32(32.0)))
            if len(small):
                stats['knuth'] += len(small)
                limit = expf(-m[small])
                p = np.ones(len(small), f32)
                factors = np.zeros(len(small), np.int64)
                run = np.ones(len(small), bool)
                sub = Lanes(rng.s[:, small])
                while run.any():
                    draw = Lanes(sub.s[:, run])
                    p[run] = p[run] * draw.uniform01()
                    sub.s[:, run] = draw.s
                    factors[run] += 1
                    run &= (p > limit) & (factors < MAX_FACTORS)
                rng.s[:, small] = sub.s
                ni[small] = (factors - 1).astype(u32)
            # the normal form
            big = np.flatnonzero(m >= f32(32.0))
            if len(big):
                stats['normal'] += len(big)
                z = np.zeros(len(big), f32)
                cached = flag[on[big]]
                stats['cache_used'] += int(cached.sum())
                z[cached] = extra[on[big][cached]]
                flag[on[big][cached]] = False
                fresh = np.flatnonzero(~cached)
                if len(fresh):
                    sub = Lanes(rng.s[:, big[fresh]])
                    now, later = sub.normal_pair()
                    rng.s[:, big[fresh]] = sub.s
                    z[fresh] = now
                    extra[on[big][fresh]] = later
                    flag[on[big][fresh]] = True
                with np.errstate(over='ignore'):
                    ni[big] = sat_u32(fmaf(np.sqrt(m[big]).astype(f32), z, m[big]) + f32(0.5))
            total_n = n[on].astype(u64) + ni.astype(u64)
            stats['saturated'] += int((total_n > 0xFFFFFFFF).sum())
            n[on] = np.minimum(total_n, u64(0xFFFFFFFF)).astype(u32)
            # times from the histogram
            if tb:
                h = lib.thist.reshape(-1, tb)[word]
                cum = np.cumsum(h, axis=1, dtype=u32)
                total = cum[:, -1]
                stats['empty_hist'] += int(((ni > 0) & (total == 0)).sum())
                draws = np.where(total > 0, np.minimum(ni, u32(MAX_TIME_DRAWS)), u32(0)).astype(np.int64)
                stats['capped'] += int(((ni > MAX_TIME_DRAWS) & (total > 0)).sum())
                for d in range(int(draws.max())):
                    act = np.flatnonzero(d < draws)
                    sub = Lanes(rng.s[:, act])
                    u = sub.uniform01()
                    r = np.minimum(sat_u32(u * total[act].astype(f32)), total[act] - u32(1))
                    above = cum[act] > r[:, None]
                    b = np.where(above.any(axis=1), above.argmax(axis=1), tb - 1)
                    x = b.astype(f32) + sub.uniform01()
                    rng.s[:, act] = sub.s
                    with np.errstate(invalid='ignore'):
                        cand = t[act] + fmaf(x, width, f32(lib.t_lo))
                        take = cand < tdrawn[on[act]]
                    tdrawn[on[act[take]]] = cand[take]
            states[:, live[on]] = rng.s
        n_out[pair] = n
        t_out[pair] = np.where(n == 0, NO_HIT_TIME, tdrawn if tb else tfirst)
    sources = en.source[int(en.offsets[0]):int(en.offsets[-1])]
    return SimpleNamespace(n=n_out, t=t_out, states=states.reshape(-1), skipped=int((sources >= lib.nsources).sum()),
                           stats=stats)


# ---------------------------------------------------------------- made libraries and events
NSOURCES, TBINS = 8, 4
T_LO, INV = f32(-8.0), f32(0.125)             # four bins of 8 ns from -8 ns
CHANNELS = (2, 300, 4096, 4097)
EVENT_SIZES = (0, 1, 3, 4, 5, 8, 9, 65)
EMITTED = np.array([1024, 1, 0, 7, 123456789, 50, 2 ** 33 + 5, 1000], u64)
DARK, UNLIT = 5, 2                            # a source with all counts 0; one with emitted == 0


def made_library(nchannels, tmin=True, thist=True, seed=5):
    """A library of NSOURCES sources as a stand-in for a HostHitMap (the attributes
    HostPhotonLibrary adopts): source UNLIT emitted nothing (its words say otherwise and
    must be ignored), source DARK has all counts 0, the others counts up to 2^24 + 1,
    NO_KEY words, negative tmin times and histogram rows that hold nothing.  Sources 0
    and 1 hold the words the made events aim at (made_entries)."""
    r = np.random.RandomState(seed + nchannels)
    words = NSOURCES * nchannels
    counts = r.randint(0, 40, words).astype(u32)
    counts[r.uniform(size=words) < 0.3] = 0
    counts[r.uniform(size=words) < 0.02] = 2 ** 24 + 1
    counts = counts.reshape(NSOURCES, nchannels)
    counts[DARK] = 0
    counts[0, 0], counts[0, 1] = 1024, 1          # emitted[0] = 1024: m = nphotons, nphotons / 1024
    counts[1, 0], counts[1, 1] = 2 ** 24 + 1, 3   # emitted[1] = 1: m = nphotons * counts
    times = r.uniform(-30.0, 90.0, words).astype(f32)
    lost = r.uniform(size=words) < 0.2
    times.reshape(NSOURCES, nchannels)[0:2, 0:2] = ((5.0, -2.5), (7.25, 0.0))
    lost.reshape(NSOURCES, nchannels)[0:2, 0:2] = False
    b = times.view(u32)
    keys = np.where(b >> u32(31) == 1, b ^ u32(0xFFFFFFFF), b ^ u32(0x80000000)).astype(u32)
    keys[lost] = NO_KEY
    hist = r.randint(0, 6, (words, TBINS)).astype(u32)
    hist[r.uniform(size=words) < 0.25] = 0
    hist.reshape(NSOURCES, nchannels, TBINS)[0:2, 0:2] = (3, 0, 5, 1)
    return SimpleNamespace(nsources=NSOURCES, nchannels=nchannels, tbins=TBINS if thist else 0,
                           t_lo=T_LO if thist else f32(0), inv=INV if thist else f32(0), emitted=EMITTED.copy(),
                           counts=counts.reshape(-1).copy(), tmin=keys if tmin else None,
                           thist=hist.reshape(-1).copy() if thist else None)


def made_entries(seed=9):
    """Events of EVENT_SIZES entries.  The 9-entry event aims at sources 0 and 1 so that
    channel 0 / channel 1 see m = 0 / 0, 32 / 0.03125, 200 / 0.195, 32758 / 31.99,
    1 / 0.00098, then (source 1) above 2^32 / 3000, twice, with a NaN and a negative
    time among them; the others mix every source, sources that do not exist, nphotons
    == 0, NaN and negative times."""
    from chroma.library import LibraryEntries
    r = np.random.RandomState(seed)
    source, nphotons, t = [], [], []
    for size in EVENT_SIZES:
        s = r.randint(0, NSOURCES + 2, size).astype(np.int64)
        s[s == NSOURCES + 1] = NO_SOURCE
        n = r.randint(0, 60, size)
        n[r.uniform(size=size) < 0.2] = 0
        tt = r.uniform(-20.0, 50.0, size).astype(f32)
        tt[r.uniform(size=size) < 0.1] = np.nan
        if size == 9:
            s[:] = (0, 0, 0, 0, 0, 1, 1, NSOURCES, 0)
            n[:] = (0, 32, 200, 32758, 1, 1000, 1000, 5, 33)
            tt[:] = (1.0, 2.0, np.nan, -3.0, 0.5, 4.0, -50.0, 0.0, np.nan)
        if size == 65:
            n[r.uniform(size=size) < 0.5] = 0          # half the long event draws nothing
        source.append(s), nphotons.append(n), t.append(tt)
    offsets = np.concatenate([[0], np.cumsum(EVENT_SIZES)])
    return LibraryEntries(offsets, np.concatenate(source), np.concatenate(nphotons), np.concatenate(t))


def host_library(made):
    from chroma import gpu
    return gpu.HostPhotonLibrary(made)
