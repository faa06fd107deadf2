"""Hit maps (chr_hitmap_accumulate, GPUHitMap, Simulation.hit_map) as far as they
can be checked without a GPU: the exports, the device entry's refusals (all made
before a device is touched), the host twin -- hitmap.h's per-photon rule built
by the host compiler -- against a numpy restatement of the rule, every word of
every array, the host HitMap, and the batch cutting of Simulation.hit_map."""
import ctypes

import numpy as np
import pytest

import hitmap_model as hmm
from hitmap_model import SIZES, NSOURCES, START, N_USED, TBINS, TRANGE

CHR_OK, CHR_ERR_INVALID = 0, 1
FAKE = 0x1000


# ------------------------------------------------------------------ exports and refusals
def test_entry_points_are_exported():
    from chroma import gpu
    from chroma.gpu import _native
    l = ctypes.CDLL(_native.library_path())
    for name in ('chr_hitmap_clear', 'chr_hitmap_accumulate', 'chr_hitmap_accumulate_host', 'chr_hitmap_last_path'):
        assert name in _native.EXPORTED and hasattr(l, name)
    assert gpu.GPUHitMap and gpu.HostHitMap and gpu.HitMap


def _call(null=(), start=0, nphotons=100, nsources=8, nchannels=2, ntbins=4, inv=0.5, thist=FAKE, tmin=FAKE,
          wsum=FAKE, host=False):
    """chr_hitmap_accumulate (or its host twin) with made-up addresses: every
    refusal comes before the first dereference or launch, so none is ever used."""
    from chroma.gpu import _native
    arg = lambda name, value=FAKE: None if name in null else value      # noqa: E731
    ph = _native.PhotonsDesc(FAKE, FAKE, FAKE, FAKE, arg('photon_t'), arg('photon_weights'), arg('photon_flags'),
                             arg('photon_last_hit'), arg('photon_evidx'))
    desc = _native.HitMapDesc(nsources, nchannels, ntbins, 0.0, inv, arg('emitted'), arg('counts'), tmin, thist, wsum,
                              arg('skipped'))
    args = (None if 'ph' in null else ctypes.byref(ph), start, nphotons, 0x4, arg('solid_map'), arg('s2c'),
            None if 'desc' in null else ctypes.byref(desc))
    if host:
        return _native.lib().chr_hitmap_accumulate_host(*args)
    return _native.lib().chr_hitmap_accumulate(*args + (None,))


@pytest.mark.parametrize('host', [False, True])
def test_no_photons_is_ok(host):
    # the arguments every refusal below starts from are themselves accepted
    assert _call(nphotons=0, host=host) == CHR_OK
    assert _call(nphotons=-3, host=host) == CHR_OK
    assert _call(nphotons=0, ntbins=0, thist=None, tmin=None, wsum=None, null=('photon_t', 'photon_weights'),
                 host=host) == CHR_OK


@pytest.mark.parametrize('host', [False, True])
@pytest.mark.parametrize('null', ['ph', 'photon_evidx', 'photon_flags', 'photon_last_hit', 'photon_t', 'photon_weights',
                                  'solid_map', 's2c', 'desc', 'emitted', 'counts', 'skipped'])
def test_refuses_null_arguments(null, host):
    from chroma.gpu import _native
    assert _call(null=(null,), nphotons=0, host=host) == CHR_ERR_INVALID
    assert b'null' in _native.lib().chr_last_error()


@pytest.mark.parametrize('host', [False, True])
def test_refuses_bad_maps(host):
    from chroma.gpu import _native
    err = lambda: _native.lib().chr_last_error()      # noqa: E731
    assert _call(thist=None, host=host) == CHR_ERR_INVALID and b'histogram' in err()      # bins without the array
    assert _call(ntbins=0, host=host) == CHR_ERR_INVALID and b'histogram' in err()        # the array without bins
    assert _call(nsources=0, host=host) == CHR_ERR_INVALID
    assert _call(nchannels=0, host=host) == CHR_ERR_INVALID
    assert _call(nchannels=-2, host=host) == CHR_ERR_INVALID
    assert _call(start=-1, host=host) == CHR_ERR_INVALID and b'negative start' in err()
    for inv in (0.0, -0.5, float('inf'), float('nan')):
        assert _call(inv=inv, host=host) == CHR_ERR_INVALID and b'inv' in err()
    # inv is not looked at without bins
    assert _call(ntbins=0, thist=None, inv=float('nan'), nphotons=0, host=host) == CHR_OK
    # arrays over 2^31 words: emitted, counts, thist
    assert _call(nsources=2 ** 31 + 1, nchannels=1, ntbins=0, thist=None, host=host) == CHR_ERR_INVALID
    assert b'2^31' in err()
    assert _call(nsources=2 ** 16 + 1, nchannels=2 ** 15, ntbins=0, thist=None, host=host) == CHR_ERR_INVALID
    assert _call(nsources=2 ** 16, nchannels=2 ** 15, ntbins=2, host=host) == CHR_ERR_INVALID
    assert _call(nsources=2 ** 16, nchannels=2 ** 15, ntbins=2 ** 31, host=host) == CHR_ERR_INVALID
    assert _call(nsources=2 ** 16, nchannels=2 ** 15, ntbins=1, nphotons=0, host=host) == CHR_OK     # exactly 2^31


def test_clear_refuses_bad_maps():
    from chroma.gpu import _native
    desc = _native.HitMapDesc(8, 2, 4, 0.0, 0.5, FAKE, FAKE, FAKE, None, FAKE, FAKE)
    assert _native.lib().chr_hitmap_clear(ctypes.byref(desc), None) == CHR_ERR_INVALID
    assert _native.lib().chr_hitmap_clear(None, None) == CHR_ERR_INVALID
    desc = _native.HitMapDesc(0, 2, 0, 0.0, 0.0, FAKE, FAKE, FAKE, None, FAKE, FAKE)
    assert _native.lib().chr_hitmap_clear(ctypes.byref(desc), None) == CHR_ERR_INVALID


# ------------------------------------------------------------------ the host twin against numpy
@pytest.fixture(scope='module')
def made(small_detector):
    """(maps, {shuffled: photons}, kind) of the made records"""
    maps = hmm.detector_maps(small_detector)
    assert maps.nchannels == 2
    ordered, kind = hmm.made_records(small_detector)
    shuffled, _ = hmm.made_records(small_detector, shuffled=True)
    return maps, {False: ordered, True: shuffled}, kind


def _model(maps, ph, start, n, nsources, opt, into=None):
    t_lo, inv = hmm.scale(opt['tbins'], opt['trange'])
    return hmm.numpy_map(ph, start, n, maps.solid_id_map, maps.solid_id_to_channel_index_gpu, nsources,
                         maps.nchannels, tbins=opt['tbins'], t_lo=t_lo, inv=inv, earliest=opt['earliest'],
                         weights=opt['weights'], into=into)


def test_made_records_exercise_what_they_claim(made):
    """On the numpy model alone."""
    maps, photons, kind = made
    ph = photons[False]
    m = _model(maps, ph, START, N_USED, NSOURCES, hmm.OPTIONS[0])
    counts = m['counts'].reshape(NSOURCES, 2)
    ids = ph.evidx[START:START + N_USED]
    assert np.array_equal(m['emitted'], np.bincount(ids[ids < NSOURCES], minlength=NSOURCES).astype(np.uint64))
    assert (counts[SIZES >= 63] > 0).all(), 'both channels in every source of 63 photons or more'
    assert (SIZES == 0).any() and m['emitted'][SIZES == 0].sum() == 0
    assert m['skipped'][0] > 0 and m['skipped'][0] + m['emitted'].sum() == N_USED
    assert m['emitted'].sum() > m['counts'].sum() > 0
    # an earliest time that is negative: its key is below the key of +0
    tmin = m['tmin']
    assert (tmin < np.uint32(0x80000000)).any() and (tmin == hmm.NO_KEY).any()
    # the largest float below t_hi lands in the last bin, t_hi itself is dropped, t_lo is in bin 0
    k = {name: kind[START:START + N_USED] == i for i, name in enumerate(hmm.KINDS)}
    used = slice(START, START + N_USED)
    known = ph.evidx[used] < NSOURCES
    thist = m['thist'].reshape(NSOURCES, 2, TBINS)
    only = lambda name: hmm.numpy_map(        # noqa: E731
        _subset(ph, used, k[name] & known), 0, int((k[name] & known).sum()), maps.solid_id_map,
        maps.solid_id_to_channel_index_gpu, NSOURCES, 2, tbins=TBINS, t_lo=hmm.scale(TBINS, TRANGE)[0],
        inv=hmm.scale(TBINS, TRANGE)[1])
    below, at_hi, at_lo = only('t_below_hi'), only('t_hi'), only('t_lo')
    assert below['counts'].sum() > 0 and below['thist'].reshape(-1, TBINS)[:, -1].sum() == below['counts'].sum()
    assert at_hi['counts'].sum() > 0 and at_hi['thist'].sum() == 0
    assert at_lo['counts'].sum() > 0 and at_lo['thist'].reshape(-1, TBINS)[:, 0].sum() == at_lo['counts'].sum()
    assert thist.sum() < m['counts'].sum()                        # no under- or overflow bins
    # weights: saturated, truncated, and dropped words all occur
    assert np.array_equal(hmm.weight_words(np.array([0.0, 0.3, np.nan, 300.0, -1.0, 1.0, 255.99999], np.float32)),
                          np.array([0, 5033165, 0, 2 ** 32 - 1, 0, 2 ** 24, 2 ** 32 - 256], np.uint64))
    light = np.float32(0.05)                                       # 0.05 * 2^24 is no integer: truncated
    exact = float(light) * 2 ** 24
    assert exact != int(exact) and hmm.weight_words(np.array([light]))[0] == int(exact)
    assert (m['wsum'] != m['counts'].astype(np.uint64) << np.uint64(24)).any()


def _subset(ph, used, mask):
    from chroma.event import Photons
    f = lambda a: a[used][mask]      # noqa: E731
    return Photons(f(ph.pos), f(ph.dir), f(ph.pol), f(ph.wavelengths), t=f(ph.t),
                   last_hit_triangles=f(ph.last_hit_triangles), flags=f(ph.flags), weights=f(ph.weights),
                   evidx=f(ph.evidx))


@pytest.mark.parametrize('shuffled', [False, True])
@pytest.mark.parametrize('opt', hmm.OPTIONS, ids=lambda o: 'bins%d_tmin%d_w%d' % (o['tbins'], o['earliest'],
                                                                                  o['weights']))
def test_host_twin_matches_numpy(made, shuffled, opt):
    from chroma import gpu
    maps, photons, _ = made
    ph = photons[shuffled]
    hm = gpu.HostHitMap(maps, NSOURCES, **opt)
    cleared = hmm.words_of(hm)
    assert all((cleared[a] == (hmm.NO_KEY if a == 'tmin' else 0)).all() for a in hmm.ARRAYS if cleared[a] is not None)
    hm.accumulate(ph, START, N_USED)
    want = _model(maps, ph, START, N_USED, NSOURCES, opt)
    hmm.assert_same_words(hmm.words_of(hm), want, 'once')
    assert want['counts'].sum() > 0 and want['skipped'][0] > 0
    # twice: the sums double, the earliest times stay
    hm.accumulate(ph, START, N_USED)
    twice = {a: None if want[a] is None else (want[a] if a == 'tmin' else want[a] * 2) for a in hmm.ARRAYS}
    hmm.assert_same_words(hmm.words_of(hm), twice, 'twice')
    hmm.assert_same_words(twice, _model(maps, ph, START, N_USED, NSOURCES, opt, into=want), 'the model, twice')
    # in two calls of uneven parts = in one
    hm.clear()
    hmm.assert_same_words(hmm.words_of(hm), cleared, 'cleared')
    hm.accumulate(ph, START, 1000)
    hm.accumulate(ph, START + 1000, 0)
    hm.accumulate(ph, START + 1000, N_USED - 1000)
    hmm.assert_same_words(hmm.words_of(hm), _model(maps, ph, START, N_USED, NSOURCES, opt), 'in parts')


def test_host_map_fields(made):
    from chroma import gpu
    maps, photons, _ = made
    ph = photons[False]
    opt = hmm.OPTIONS[0]
    hm = gpu.HostHitMap(maps, NSOURCES, **opt)
    hm.accumulate(ph, START, N_USED)
    want = _model(maps, ph, START, N_USED, NSOURCES, opt)
    got = hm.get()
    assert got.counts.shape == (NSOURCES, 2) and got.counts.dtype == np.uint32
    assert got.emitted.shape == (NSOURCES,) and got.emitted.dtype == np.uint64
    assert got.thist.shape == (NSOURCES, 2, TBINS) and got.tmin.dtype == np.float32 and got.wsum.dtype == np.float64
    assert np.array_equal(got.counts.reshape(-1), want['counts']) and np.array_equal(got.emitted, want['emitted'])
    assert np.array_equal(got.thist.reshape(-1), want['thist']) and got.skipped == int(want['skipped'][0])
    assert np.array_equal(got.wsum.reshape(-1), want['wsum'] / 2.0 ** 24)
    # tmin: the smallest time of the channel's detected photons that is not NaN; +inf where there is none
    used = slice(START, START + N_USED)
    solid, s2c = maps.solid_id_map, maps.solid_id_to_channel_index_gpu
    for s in range(NSOURCES):
        for c in range(2):
            sel = (ph.evidx[used] == s) & ((ph.flags[used] & 4) != 0) & (ph.last_hit_triangles[used] > -1)
            sel[sel] = s2c[solid[ph.last_hit_triangles[used][sel]]] == c
            ts = ph.t[used][sel]
            ts = ts[~np.isnan(ts)]
            expect = np.float32(ts.min()) if len(ts) else np.float32(np.inf)
            assert got.tmin[s, c] == expect, (s, c)
    assert (got.tmin < 0).any() and np.isinf(got.tmin[SIZES == 0]).all()
    # visibility
    vis = got.visibility()
    assert vis.dtype == np.float64 and vis.shape == (NSOURCES, 2)
    assert (vis[SIZES == 0] == 0).all()
    lit = want['emitted'] > 0
    assert np.array_equal(vis[lit], want['counts'].reshape(NSOURCES, 2)[lit] / want['emitted'][lit][:, None].astype(float))
    # a source that emitted 2^32 photons: a count may have wrapped
    hm.emitted[3] = 2 ** 32 - 1
    hm.get()
    hm.emitted[3] = 2 ** 32
    with pytest.raises(OverflowError):
        hm.get()


def test_python_refusals(made):
    from chroma import gpu
    maps = made[0]
    with pytest.raises(ValueError):
        gpu.HostHitMap(maps, 8, tbins=4)                       # no trange
    with pytest.raises(ValueError):
        gpu.HostHitMap(maps, 8, tbins=4, trange=(5.0, 5.0))    # no width
    with pytest.raises(ValueError):
        gpu.HostHitMap(maps, 8, tbins=4, trange=(9.0, 5.0))    # negative width
    with pytest.raises(ValueError):
        gpu.HostHitMap(maps, 0)
    with pytest.raises(ValueError):
        gpu.HostHitMap(maps, 2 ** 31)                          # counts over 2^31 words
    hm = gpu.HostHitMap(maps, 8)
    with pytest.raises(ValueError):
        hm.accumulate(made[1][False], 2990, 11)                # beyond the records
    from chroma.gpu.hitmap import bin_scale
    assert bin_scale(8, (16.0, 80.0)) == (np.float32(16.0), np.float32(0.125))
    t_lo, inv = bin_scale(7, (-10.0, 90.0))
    assert inv.dtype == np.float32 and inv == np.float32(7) / np.float32(100)


# ------------------------------------------------------------------ 4096 channels through a stand-in
@pytest.mark.parametrize('opt', [dict(tbins=16, trange=(0.0, 64.0), earliest=True, weights=True),
                                 dict(tbins=0, trange=None, earliest=True, weights=False)], ids=['bins16', 'tmin_only'])
def test_wide_stand_in_detector(opt):
    from chroma import gpu
    maps, ph = hmm.wide_maps(), hmm.wide_records()
    hm = gpu.HostHitMap(maps, hmm.WIDE_SOURCES, **opt)
    hm.accumulate(ph)
    want = _model(maps, ph, 0, len(ph), hmm.WIDE_SOURCES, opt)
    hmm.assert_same_words(hmm.words_of(hm), want, 'wide')
    assert (want['emitted'] == hmm.WIDE_PER_SOURCE).all() and want['skipped'][0] == 0
    assert want['counts'].sum() == len(ph) - len(ph[::8]) and want['counts'].max() >= 2
    # the row against the privatised path's LDS budget (tests/test_gpu_hitmap.py relies on it)
    from chroma.gpu.hitmap import LDS_WORDS
    assert (hm.row_words > LDS_WORDS) == bool(opt['tbins']) and (opt['tbins'] or hm.row_words == LDS_WORDS)
    # fewer sources than the photons name: the others are skipped, the rest is unchanged
    hm3 = gpu.HostHitMap(maps, 3, **opt)
    hm3.accumulate(ph)
    got = hmm.words_of(hm3)
    assert got['skipped'][0] == 5 * hmm.WIDE_PER_SOURCE
    assert np.array_equal(got['counts'], want['counts'][:3 * hmm.WIDE_CHANNELS])


# ------------------------------------------------------------------ Simulation.hit_map's batches
def test_batch_cutting():
    from chroma.sim import hit_map_batches
    assert hit_map_batches([], 1000) == []
    assert hit_map_batches([5], 1000) == [(0, 1)]
    # a batch closes after the step that brings it to the limit or beyond; steps are never split
    assert hit_map_batches([700, 64, 1, 0, 3000, 333], 1000) == [(0, 5), (5, 6)]
    assert hit_map_batches([700, 300, 1, 0, 3000, 333], 1000) == [(0, 2), (2, 5), (5, 6)]
    assert hit_map_batches([3000, 3000], 1000) == [(0, 1), (1, 2)]
    assert hit_map_batches([1000, 0, 0], 1000) == [(0, 1), (1, 3)]            # trailing steps without photons
    assert hit_map_batches([0, 0], 1000) == [(0, 2)]
    assert hit_map_batches([2, 2, 2], 0) == [(0, 1), (1, 2), (2, 3)]
    big = hit_map_batches([2 ** 32 - 1, 2 ** 32 - 1, 1], 2 ** 33)                   # 64-bit sums
    assert big == [(0, 3)]
    r = np.random.RandomState(4)
    counts = r.randint(0, 500, 300)
    batches = hit_map_batches(counts, 2000)
    assert batches[0][0] == 0 and batches[-1][1] == len(counts)
    assert all(a[1] == b[0] for a, b in zip(batches[:-1], batches[1:]))
    for a, b in batches[:-1]:
        assert counts[a:b].sum() >= 2000 > counts[a:b - 1].sum()
    assert counts[batches[-1][0]:batches[-1][1] - 1].sum() < 2000


def test_sharded_simulation_has_no_hit_map():
    from chroma.sim import ShardedSimulation
    with pytest.raises(NotImplementedError):
        ShardedSimulation.hit_map(object(), [], 1)
