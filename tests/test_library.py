"""The photon-library lookup (chr_library_expect, chr_library_sample,
GPUPhotonLibrary / HostPhotonLibrary, chroma.library) as far as it can be
checked without a GPU: the exports, every refusal (all made before anything is
read through a pointer), the host twins -- library.h's rules built by the host
compiler -- against the numpy restatement of tests/library_model.py, every word
of every output and of the generator states, the Poisson draw's mean, and the
host-side helpers."""
import ctypes
import math

import numpy as np
import pytest

import library_model as lm

CHR_OK, CHR_ERR_INVALID = 0, 1
FAKE = 0x1000


# ------------------------------------------------------------------ exports and refusals
def test_entry_points_are_exported():
    from chroma import gpu
    from chroma.gpu import _native
    l = ctypes.CDLL(_native.library_path())
    for name in ('chr_library_expect', 'chr_library_sample', 'chr_library_expect_host', 'chr_library_sample_host',
                 'chr_library_last_path'):
        assert name in _native.EXPORTED and hasattr(l, name)
    assert gpu.GPUPhotonLibrary and gpu.HostPhotonLibrary


def _call(entry, null=(), nevents=0, nsources=8, nchannels=2, ntbins=4, inv=0.5, thist=FAKE, tmin=FAKE, nslots=16):
    """One of the four entry points with made-up addresses: every refusal comes before
    the first dereference or launch, and nevents == 0 touches nothing, so none is used."""
    from chroma.gpu import _native
    arg = lambda name, value=FAKE: None if name in null else value      # noqa: E731
    desc = _native.HitMapDesc(nsources, nchannels, ntbins, 0.0, inv, arg('emitted'), arg('counts'), tmin, thist, None,
                              None)
    en = _native.LibraryEntriesDesc(nevents, arg('offsets'), arg('source'), arg('nphotons'), arg('t'))
    lib = None if 'desc' in null else ctypes.byref(desc)
    entries = None if 'entries' in null else ctypes.byref(en)
    host = entry.endswith('_host')
    if 'expect' in entry:
        args = (lib, entries, arg('mu'), arg('tfirst'), arg('skipped'))
    else:
        args = (lib, entries, arg('rng'), nslots, arg('n'), arg('t_out'), arg('skipped'))
    return getattr(_native.lib(), entry)(*(args if host else args + (None,)))


ENTRIES = ('chr_library_expect', 'chr_library_sample', 'chr_library_expect_host', 'chr_library_sample_host')
OUTPUTS = {'expect': ('mu', 'tfirst'), 'sample': ('n', 't_out', 'rng')}


@pytest.mark.parametrize('entry', ENTRIES)
def test_no_events_is_ok(entry):
    # the arguments every refusal below starts from are themselves accepted
    assert _call(entry) == CHR_OK
    assert _call(entry, ntbins=0, thist=None, tmin=None) == CHR_OK
    assert _call(entry, null=('offsets', 'source', 'nphotons', 't')) == CHR_OK      # not looked at without events
    if 'expect' in entry:
        assert _call(entry, tmin=None, null=('tfirst',)) == CHR_OK                   # no tmin, no tfirst


@pytest.mark.parametrize('entry', ENTRIES)
def test_refuses_null_arguments(entry):
    from chroma.gpu import _native
    kind = 'expect' if 'expect' in entry else 'sample'
    for null in ('desc', 'entries', 'emitted', 'counts', 'skipped') + OUTPUTS[kind]:
        assert _call(entry, null=(null,)) == CHR_ERR_INVALID, null
        assert b'null' in _native.lib().chr_last_error()
    # with events, a null entry array is refused before any is read (without events it is accepted)
    for null in ('offsets', 'source', 'nphotons', 't'):
        assert _call(entry, null=(null,), nevents=1) == CHR_ERR_INVALID, null
        assert b'null' in _native.lib().chr_last_error()


@pytest.mark.parametrize('entry', ENTRIES)
def test_refuses_bad_libraries(entry):
    from chroma.gpu import _native
    err = lambda: _native.lib().chr_last_error()      # noqa: E731
    assert _call(entry, thist=None) == CHR_ERR_INVALID and b'histogram' in err()       # bins without the array
    assert _call(entry, ntbins=0) == CHR_ERR_INVALID and b'histogram' in err()         # the array without bins
    assert _call(entry, nsources=0) == CHR_ERR_INVALID
    assert _call(entry, nchannels=0) == CHR_ERR_INVALID
    assert _call(entry, nchannels=-2) == CHR_ERR_INVALID
    for inv in (0.0, -0.5, float('inf'), float('nan')):
        assert _call(entry, inv=inv) == CHR_ERR_INVALID and b'inv' in err()
    assert _call(entry, ntbins=0, thist=None, inv=float('nan')) == CHR_OK              # not looked at without bins
    # arrays over 2^31 words: emitted, counts, thist, the outputs
    assert _call(entry, nsources=2 ** 31 + 1, nchannels=1, ntbins=0, thist=None) == CHR_ERR_INVALID
    assert b'2^31' in err()
    assert _call(entry, nsources=2 ** 16 + 1, nchannels=2 ** 15, ntbins=0, thist=None) == CHR_ERR_INVALID
    assert _call(entry, nsources=2 ** 16, nchannels=2 ** 15, ntbins=2) == CHR_ERR_INVALID
    assert _call(entry, nsources=2 ** 16, nchannels=2 ** 15, ntbins=1) == CHR_OK       # exactly 2^31
    assert _call(entry, nevents=2 ** 30 + 1, nchannels=2) == CHR_ERR_INVALID and b'events' in err()
    if 'sample' in entry:
        assert _call(entry, nslots=0) == CHR_ERR_INVALID and b'slots' in err()
        assert _call(entry, nslots=2 ** 31) == CHR_ERR_INVALID


@pytest.mark.parametrize('sampling', [False, True])
def test_host_twins_refuse_descending_offsets(sampling):
    from chroma.gpu import _native
    lib = lm.host_library(lm.made_library(2))
    en = lm.made_entries()
    bad = en.offsets.copy()
    bad[3] = bad[2] - 1
    desc = _native.LibraryEntriesDesc(en.nevents, bad.ctypes.data, en.source.ctypes.data, en.nphotons.ctypes.data,
                                      en.t.ctypes.data)
    n = en.nevents * 2
    a, b, skipped = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(1, np.uint64)
    if sampling:
        st = np.arange(6 * 4, dtype=np.uint32)
        rc = _native.lib().chr_library_sample_host(ctypes.byref(lib._desc()), ctypes.byref(desc), st.ctypes.data, 4,
                                                   a.ctypes.data, b.ctypes.data, skipped.ctypes.data)
        assert np.array_equal(st, np.arange(6 * 4, dtype=np.uint32))
    else:
        rc = _native.lib().chr_library_expect_host(ctypes.byref(lib._desc()), ctypes.byref(desc), b.ctypes.data,
                                                   a.ctypes.data, skipped.ctypes.data)
    assert rc == CHR_ERR_INVALID and b'ascending' in _native.lib().chr_last_error()
    assert not a.any() and not b.any() and skipped[0] == 0


def test_library_entries_refusals():
    from chroma.library import LibraryEntries
    ok = LibraryEntries([0, 2, 2, 3], [1, 2, 0xFFFFFFFF], [5, 0, 7], [0.0, 1.5, np.nan])
    assert ok.nevents == 3 and ok.nentries == 3 and ok.source.dtype == np.uint32 and ok.t.dtype == np.float32
    assert LibraryEntries([0], [], [], []).nevents == 0
    with pytest.raises(ValueError):
        LibraryEntries([0, 2, 1], [1, 2], [5, 0], [0.0, 1.5])           # not ascending
    with pytest.raises(ValueError):
        LibraryEntries([0, 3], [1, 2], [5, 0], [0.0, 1.5])              # beyond the entries
    with pytest.raises(ValueError):
        LibraryEntries([0, 2], [1, 2], [5], [0.0, 1.5])                 # lengths differ
    with pytest.raises(ValueError):
        LibraryEntries([], [], [], [])                                  # no offsets at all
    with pytest.raises(ValueError):
        LibraryEntries([0, 1], [-1], [5], [0.0])                        # no uint32
    with pytest.raises(ValueError):
        LibraryEntries([0, 1], [1], [2 ** 32], [0.0])
    with pytest.raises(TypeError):
        lm.host_library(lm.made_library(2)).expect(([0], [], [], []))


# ------------------------------------------------------------------ the host twins against numpy
@pytest.fixture(scope='module')
def entries():
    return lm.made_entries()


@pytest.fixture(scope='module')
def models(entries):
    """The numpy model's words, computed once per case and shared (left unchanged)."""
    cache = {}

    def get(nchannels, tmin=True, thist=True, nslots=None):
        key = (nchannels, tmin, thist, nslots)
        if key not in cache:
            made = lm.made_library(nchannels, tmin=tmin, thist=thist)
            if nslots is None:
                cache[key] = lm.numpy_expect(made, entries)
            else:
                from chroma.gensteps import rng_init_host
                cache[key] = lm.numpy_sample(made, entries, rng_init_host(nslots, seed=3), nslots)
        return cache[key]
    return get


def _same_floats(got, want):
    return np.array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32).reshape(-1),
                          np.ascontiguousarray(want, np.float32).view(np.uint32).reshape(-1))


OPTIONAL = [(True, True), (False, True), (True, False), (False, False)]


@pytest.mark.parametrize('nchannels', lm.CHANNELS)
def test_expect_host_twin_matches_numpy(models, entries, nchannels):
    for tmin, thist in (OPTIONAL if nchannels == 300 else OPTIONAL[:1]):
        made = lm.made_library(nchannels, tmin=tmin, thist=thist)
        lib = lm.host_library(made)
        before = lib.words()
        got = lib.expect(entries).get()
        want = models(nchannels, tmin, thist)
        assert _same_floats(got.mu, want.mu), 'mu words differ'
        assert (got.tfirst is None) == (not tmin)
        if tmin:
            assert _same_floats(got.tfirst, want.tfirst), 'tfirst words differ'
        assert got.skipped == want.skipped > 0
        after = lib.words()
        assert all(before[k] is None or np.array_equal(before[k], after[k]) for k in before)


def _sample_cases():
    for nchannels in lm.CHANNELS:
        npairs = nchannels * len(lm.EVENT_SIZES)
        for nslots in ((1, 7, npairs, npairs + 5) if nchannels == 2 else (npairs, npairs + 5)):
            yield nchannels, nslots, True, True
    for tmin, thist in OPTIONAL[1:]:
        yield 300, 300 * len(lm.EVENT_SIZES), tmin, thist
    yield 300, 301, True, True            # T far below npairs on a wider row: eight strided rounds per slot


@pytest.mark.parametrize('nchannels,nslots,tmin,thist', list(_sample_cases()))
def test_sample_host_twin_matches_numpy(models, entries, nchannels, nslots, tmin, thist):
    from chroma.gensteps import rng_init_host
    lib = lm.host_library(lm.made_library(nchannels, tmin=tmin, thist=thist))
    before = lib.words()
    states = rng_init_host(nslots, seed=3)
    start = states.copy()
    got = lib.sample(entries, states)
    want = models(nchannels, tmin, thist, nslots)
    assert np.array_equal(got.n, want.n), 'n words differ'
    assert _same_floats(got.t, want.t), 't words differ'
    assert int(got.skipped[0]) == want.skipped > 0
    assert np.array_equal(states, want.states), 'rng states differ'
    T = min(nslots, nchannels * entries.nevents)
    moved = (states.reshape(6, nslots) != start.reshape(6, nslots)).any(axis=0)
    assert moved[:T].any() and not moved[T:].any(), 'slots >= T are untouched'
    after = lib.words()
    assert all(before[k] is None or np.array_equal(before[k], after[k]) for k in before)
    channels = got.get()
    assert len(channels) == entries.nevents and channels[0].q.dtype == np.float32
    n = want.n.reshape(entries.nevents, nchannels)
    assert np.array_equal(channels[3].hit, n[3] > 0) and np.array_equal(channels[3].q, n[3].astype(np.float32))
    assert not channels[0].hit.any() and (channels[0].t == np.float32(1e9)).all()      # the event without entries


def trailing_empty_entries():
    """(label, entries): an event without entries last, a run of them last, and nothing but
    such events -- with the entry arrays exactly as long as the offsets say."""
    from chroma.library import LibraryEntries
    full = lm.made_entries()
    n = int(full.offsets[4])                                       # the events of 0, 1, 3 and 4 entries
    cut = lambda offsets: LibraryEntries(offsets, full.source[:n], full.nphotons[:n], full.t[:n])      # noqa: E731
    head = full.offsets[:5].tolist()
    return [('empty last', cut(head + [n])), ('two empty last', cut(head + [n, n])),
            ('all empty', LibraryEntries([0, 0, 0, 0], [], [], [])),
            ('all empty behind entries', LibraryEntries([n, n, n], full.source[:n], full.nphotons[:n], full.t[:n]))]


def test_events_without_entries_last():
    for label, en in trailing_empty_entries():
        made = lm.made_library(300)
        lib = lm.host_library(made)
        got, want = lib.expect(en).get(), lm.numpy_expect(made, en)
        assert _same_floats(got.mu, want.mu) and _same_floats(got.tfirst, want.tfirst), label
        assert got.skipped == want.skipped
        assert (got.mu[-1] == 0).all() and np.isinf(got.tfirst[-1]).all(), label
        from chroma.gensteps import rng_init_host
        states = rng_init_host(64, seed=3)
        drawn, model = lib.sample(en, states), lm.numpy_sample(made, en, rng_init_host(64, seed=3), 64)
        assert np.array_equal(drawn.n, model.n) and _same_floats(drawn.t, model.t), label
        assert np.array_equal(states, model.states), label


def test_made_records_exercise_what_they_claim(models, entries):
    """On the numpy model alone."""
    assert tuple(np.diff(entries.offsets.astype(np.int64))) == lm.EVENT_SIZES
    src = entries.source
    assert (src == lm.NO_SOURCE).any() and (src == lm.NSOURCES).any() and (src == lm.UNLIT).any() \
        and (src == lm.DARK).any()
    assert (entries.nphotons == 0).any() and np.isnan(entries.t).any() and (entries.t < 0).any()
    made = lm.made_library(2)
    assert made.emitted[lm.UNLIT] == 0 and made.counts.reshape(lm.NSOURCES, 2)[lm.UNLIT].any()
    wide = lm.made_library(4097)
    assert wide.counts.max() == 2 ** 24 + 1 and not wide.counts.reshape(lm.NSOURCES, -1)[lm.DARK].any()
    assert (wide.tmin == lm.NO_KEY).any() and (wide.tmin < np.uint32(0x80000000)).any()       # negative times
    assert (wide.thist.reshape(-1, lm.TBINS).sum(axis=1) == 0).any()
    # the 9-entry event's values of m on channels 0 and 1 of the 2-channel library
    first = int(entries.offsets[lm.EVENT_SIZES.index(9)])
    m = []
    for i in range(first, first + 9):
        s, w = lm._entry_of(made, entries, i)
        if s is not None:
            m.extend((w * made.counts[s * 2:s * 2 + 2].astype(np.float32)).tolist())
    assert 0.0 in m and 32.0 in m and 200.0 in m and max(m) > 2.0 ** 32
    assert any(abs(x - 1e-3) < 1e-4 for x in m) and any(31.98 < x < 32.0 for x in m)
    expect = models(2)
    assert expect.nan_candidates > 0, 'a NaN candidate was met and not taken'
    assert not np.isnan(expect.tfirst).any() and np.isinf(expect.tfirst).any() and (expect.tfirst < 0).any()
    assert (expect.mu[0] == 0).all() and (expect.mu > 2.0 ** 24).any()
    s = models(2, True, True, 16).stats
    assert s['knuth'] > 0 and s['normal'] > 0 and s['cache_used'] > 0, 'both Poisson branches, and the cached normal'
    assert s['capped'] > 0, 'the 64-draw cap'
    assert s['saturated'] > 0 and (models(2, True, True, 16).n == 0xFFFFFFFF).any(), 'a saturated n'
    assert models(300, True, True, 2400).stats['empty_hist'] > 0, 'a histogram row that holds nothing'


def test_model_arithmetic():
    """A guard on the oracle, not coverage of the feature (it runs no code of the package):
    the model's own fmaf and functions against exact rational arithmetic and float64."""
    from fractions import Fraction
    r = np.random.RandomState(1)
    a = (r.uniform(-4, 4, 2000) * 10.0 ** r.randint(-6, 6, 2000)).astype(np.float32)
    b = (r.uniform(-4, 4, 2000) * 10.0 ** r.randint(-6, 6, 2000)).astype(np.float32)
    c = (-a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)            # heavy cancellation
    c[::2] = r.uniform(-4, 4, 1000).astype(np.float32)
    got = lm.fmaf(a, b, c)
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(float(lo))),
                                                           abs(exact - Fraction(float(hi))))
    # just below a float32 tie, 1 + 2^-23 + 2^-24 - 2^-70: rounding to float64 first lands on the tie
    # and then on the even neighbour 1 + 2^-22; the exact fmaf gives 1 + 2^-23
    x = np.float32(1.0 + 2.0 ** -23)
    assert float(lm.fmaf(np.float32(2.0 ** -24) * x, np.float32(1.0 - 2.0 ** -23), x)) == x
    assert np.float32(np.float64(2.0 ** -24) * x * np.float64(1.0 - 2.0 ** -23) + np.float64(x)) != x
    assert float(lm.fmaf(x, x, np.float32(-1.0))) == np.float32(2.0 ** -22 + 2.0 ** -46)
    xs = np.linspace(-31.9, 0.0, 500).astype(np.float32)
    assert np.allclose(lm.expf(xs), np.exp(xs.astype(np.float64)), rtol=3e-7)
    us = np.linspace(1e-9, 1.0, 500).astype(np.float32)
    assert np.allclose(lm.logf(us), np.log(us.astype(np.float64)), rtol=3e-7, atol=1e-7)
    vs = np.linspace(0.0, 6.3, 500).astype(np.float32)
    s, c = lm.sincosf(vs)
    assert np.allclose(s, np.sin(vs.astype(np.float64)), atol=3e-7) and np.allclose(c, np.cos(vs.astype(np.float64)),
                                                                                   atol=3e-7)


# ------------------------------------------------------------------ the Poisson draw
POISSON_K = 200000
# m as nphotons / emitted with a count of 1: both float32 conversions and the divide are the rule's
POISSON_CASES = {0.01: (1, 100), 0.5: (1, 2), 3.0: (3, 1), 31.9: (319, 10), 32.0: (32, 1), 200.0: (200, 1),
                 1e4: (10000, 1)}


@pytest.mark.parametrize('m', sorted(POISSON_CASES))
def test_poisson_mean(m):
    """K = 200,000 draws of the host twin with a fixed seed: the sample mean lies within
    5 sqrt(m / K), five standard errors of a Poisson mean, of m.  For m >= 32 the draw is
    a rounded normal, n = floor(m + sqrt(m) z + 0.5) cut at 0, whose mean differs from m by:
    the cut at 0, below sqrt(m) * phi(sqrt(m)) <= 2e-7 for m >= 32; the rounding to the
    nearest integer of a density of width sqrt(m) >= 5.6, below 2 exp(-2 pi^2 m) (nothing);
    and the float32 roundings of the fmaf and of the + 0.5, each at most half an ulp of a
    value below m + 6 sqrt(m), together 2^-24 (m + 6 sqrt(m)).  That bias is added to the
    bound; the multiple stays 5."""
    from chroma.gensteps import rng_init_host
    from chroma.library import LibraryEntries
    nphotons, emitted = POISSON_CASES[m]
    nch, nev = 2000, POISSON_K // 2000
    made = lm.SimpleNamespace(nsources=1, nchannels=nch, tbins=0, t_lo=np.float32(0), inv=np.float32(0),
                              emitted=np.array([emitted], np.uint64), counts=np.ones(nch, np.uint32), tmin=None,
                              thist=None)
    en = LibraryEntries(np.arange(nev + 1), np.zeros(nev), np.full(nev, nphotons), np.zeros(nev))
    got = lm.host_library(made).sample(en, rng_init_host(1000, seed=12345))
    mf = float(np.float32(nphotons) / np.float32(emitted))
    assert abs(mf - m) <= 1e-6 * m
    mean = got.n.astype(np.float64).mean()
    bias = 0.0 if m < 32 else 2e-7 + 2.0 ** -24 * (mf + 6.0 * math.sqrt(mf))
    print('m = %g: mean %.6f, |mean - m| = %.3g, bound %.3g' % (m, mean, abs(mean - mf),
                                                                 5.0 * math.sqrt(mf / POISSON_K) + bias))
    assert abs(mean - mf) <= 5.0 * math.sqrt(mf / POISSON_K) + bias
    if m < 32:          # the second moment too: a Poisson's variance is its mean (loose: a sanity check of the form)
        assert abs(got.n.astype(np.float64).var() - mf) < 0.05 * mf + 1e-3


# ------------------------------------------------------------------ the voxel grid and the entries of gensteps
def test_voxel_grid():
    from chroma.library import VoxelGrid
    g = VoxelGrid((-10.0, 0.0, 100.0), (10.0, 30.0, 140.0), (4, 3, 2))
    assert g.nvoxels == 24
    pts = np.array([[-10.0, 0.0, 100.0],        # the low corner: voxel 0
                    [-5.0, 0.0, 100.0],         # on the face between ix 0 and 1: the upper voxel
                    [9.999, 29.999, 139.999],   # just inside the high corner: the last voxel
                    [10.0, 15.0, 120.0],        # on a high face: outside
                    [0.0, 30.0, 120.0], [0.0, 15.0, 140.0],
                    [-10.001, 15.0, 120.0], [0.0, -1.0, 120.0], [0.0, 15.0, 99.0],
                    [np.nan, 15.0, 120.0], [np.inf, 15.0, 120.0],
                    [0.0, 15.0, 120.0],         # ix 2, iy 1, iz 1
                    [-7.5, 25.0, 110.0]])       # ix 0, iy 2, iz 0
    want = [0, 1, 23, -1, -1, -1, -1, -1, -1, -1, -1, 2 + 4 * (1 + 3 * 1), 0 + 4 * (2 + 3 * 0)]
    assert g.index(pts).tolist() == want and g.index(pts).dtype == np.int64
    c = g.centers()
    assert c.shape == (24, 3) and c.dtype == np.float64
    assert np.array_equal(g.index(c), np.arange(24)), 'the id order: x fastest, then y, then z'
    assert np.allclose(c[0], (-7.5, 5.0, 110.0)) and np.allclose(c[1], (-2.5, 5.0, 110.0)) \
        and np.allclose(c[4], (-7.5, 15.0, 110.0)) and np.allclose(c[12], (-7.5, 5.0, 130.0))
    fl = g.flashes(3, 500, wavelength_range=(300.0, 600.0))
    assert fl.nsteps == 24 and fl.nphotons == 24 * 500
    assert np.array_equal(fl.steps['evidx'], np.arange(24)) and (fl.steps['material'] == 3).all()
    assert np.array_equal(fl.steps['x0'], c.astype(np.float32)) and not fl.steps['dx'].any()
    assert (fl.steps['wl_lo'] == 300.0).all() and (fl.steps['wl_hi'] == 600.0).all() and (fl.steps['kind'] == 0).all()
    material = object()
    assert all(m is material for m in g.flashes(material, 1).materials)
    for bad in (((0, 0, 0), (1, 1, 1), (2, 2)), ((0, 0, 0), (1, 0, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (2, 0, 2)),
                ((0, 0, 0), (1, np.inf, 1), (2, 2, 2))):
        with pytest.raises(ValueError):
            VoxelGrid(*bad)


def test_entries_from_gensteps():
    from chroma import gensteps as gs
    from chroma.library import NO_SOURCE, VoxelGrid, entries_from_gensteps
    g = VoxelGrid((0.0, 0.0, 0.0), (10.0, 10.0, 10.0), (2, 2, 2))
    a = gs.isotropic_flash(0, 100, x0=(1, 1, 1), t0=2.0) \
        + gs.cherenkov_step(0, 7, x0=(4, 1, 1), dx=(4, 0, 0), beta=0.9, t0=1.0, dt=0.5) \
        + gs.scintillation_step(0, 0, x0=(9, 9, 9), dx=(4, 4, 4), t0=3.0)             # its midpoint is outside
    b = gs.Gensteps()
    c = gs.isotropic_flash(0, 5, x0=(1, 9, 9), dx=(0, 0, -8), t0=-1.0, dt=np.float32(0.1))
    en = entries_from_gensteps(g, [a, b, c])
    assert en.offsets.tolist() == [0, 3, 3, 4] and en.nevents == 3
    assert en.source.tolist() == [0, 1, NO_SOURCE, 0 + 2 * (1 + 2 * 1)]      # z = 5 is the upper voxel's low face
    assert en.nphotons.tolist() == [100, 7, 0, 5]
    assert en.t.dtype == np.float32 and en.t.tolist() == [2.0, 1.25, 3.0, float(np.float32(-1.0) + np.float32(0.5)
                                                                              * np.float32(0.1))]
    empty = entries_from_gensteps(g, [])
    assert empty.nevents == 0 and empty.nentries == 0
    assert entries_from_gensteps(g, [b, b]).offsets.tolist() == [0, 0, 0]


def test_save_and_load(tmp_path, entries):
    from chroma import gpu
    from chroma.library import VoxelGrid
    grid = VoxelGrid((0, 0, 0), (4, 2, 1), (4, 2, 1))
    for tmin, thist, with_grid in ((True, True, True), (False, False, False), (True, False, True)):
        lib = gpu.HostPhotonLibrary(lm.made_library(300, tmin=tmin, thist=thist), grid=grid if with_grid else None)
        path = str(tmp_path / ('lib_%d%d.npz' % (tmin, thist)))
        lib.save(path)
        back = gpu.HostPhotonLibrary.load(path)
        assert (back.nsources, back.nchannels, back.tbins) == (lib.nsources, 300, lib.tbins)
        assert back.t_lo == lib.t_lo and back.inv == lib.inv and (back.grid == grid if with_grid else back.grid is None)
        a, b = lib.words(), back.words()
        assert all((a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]))
                   for k in a)
        assert _same_floats(back.expect(entries).get().mu, lib.expect(entries).get().mu)
    with pytest.raises(ValueError):
        gpu.HostPhotonLibrary(lm.made_library(2), grid=VoxelGrid((0, 0, 0), (1, 1, 1), (3, 1, 1)))    # 3 voxels, 8 sources


def test_library_of_a_host_hit_map(entries):
    """A HitMap (what Simulation.hit_map returns) gives the library of its words."""
    from chroma import gpu
    made = lm.made_library(300)
    table = gpu.HitMap.from_words(lm.NSOURCES, 300, lm.TBINS, np.where(made.emitted >= 2 ** 32, 5, made.emitted),
                                  made.counts, made.tmin, made.thist, t_lo=made.t_lo, inv=made.inv)
    made.emitted = table.emitted.copy()
    a, b = gpu.HostPhotonLibrary(table), gpu.HostPhotonLibrary(made)
    wa, wb = a.words(), b.words()
    assert all(np.array_equal(wa[k], wb[k]) for k in wa)
    assert _same_floats(a.expect(entries).get().tfirst, b.expect(entries).get().tfirst)


def test_expected_channels():
    from chroma.gpu.library import Expected, expected_channels
    mu = np.array([[0.0, 2.5], [1.0, 0.0]], np.float32)
    tf = np.array([[np.inf, 3.0], [-1.0, 7.0]], np.float32)
    ch = expected_channels(Expected(2, 2, mu, tf, 0, None))
    assert ch[0].hit.tolist() == [False, True] and ch[0].t.tolist() == [1e9, 3.0] and ch[0].q.tolist() == [0.0, 2.5]
    assert ch[1].hit.tolist() == [True, False] and ch[1].t.tolist() == [-1.0, 1e9]
    assert (expected_channels(Expected(2, 2, mu, None, 0, None))[0].t == np.float32(1e9)).all()


# ------------------------------------------------------------------ the host twins in a stand-alone program
def test_stand_alone_host_program(tmp_path):
    """tests/library_host_check.cpp with csrc/library_host.cpp, built for the host: the twins
    and their refusals over heap blocks of exactly the documented sizes (the program a
    sanitizer build checks; here it is built plain)."""
    import os
    import subprocess
    from test_host_driver import CSRC, ROOT, _compiler
    exe = str(tmp_path / 'library_host_check')
    subprocess.check_call([_compiler(), '-O2', '-std=c++17', '-Wall', '-ffp-contract=off', '-I', CSRC, '-o', exe,
                           os.path.join(ROOT, 'tests', 'library_host_check.cpp'),
                           os.path.join(CSRC, 'library_host.cpp'), '-lm'])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(p.stdout)
    assert p.stdout.strip().splitlines()[-1] == 'variants=4 failures=0' and p.returncode == 0
