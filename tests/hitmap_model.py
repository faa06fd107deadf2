"""What the hit-map tests share: a numpy restatement of the per-photon rule
(include/chroma_amd.h, "hit maps") -- the expected words never come from the
code under test --, the made records and the stand-in detector."""
from types import SimpleNamespace

import numpy as np

from test_daq_events import BOUNDS, SIZES

SURFACE_DETECT, SURFACE_ABSORB, REFLECT_DIFFUSE = 1 << 2, 1 << 3, 1 << 5
NO_KEY = np.uint32(0xFFFFFFFF)
ARRAYS = ('emitted', 'counts', 'tmin', 'thist', 'wsum', 'skipped')

# ---------------------------------------------------------------- the rule in numpy


def keys_of(t):
    b = np.ascontiguousarray(t, np.float32).view(np.uint32)
    return np.where((b >> 31) == 1, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def times_of(keys):
    """keys_of inverted; +inf for the cleared word"""
    k = np.asarray(keys, np.uint32)
    b = np.where((k >> 31) == 1, k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return np.where(k == NO_KEY, np.float32(np.inf), b.view(np.float32))


def weight_words(w):
    with np.errstate(invalid='ignore', over='ignore'):
        x = np.asarray(w, np.float32) * np.float32(16777216.0)
        zero = np.isnan(x) | (x < 0)
        top = ~zero & (x >= np.float32(4294967296.0))
        q = np.where(zero | top, np.float32(0), x).astype(np.uint64)      # astype truncates
    q[top] = 2 ** 32 - 1
    return q


def numpy_map(ph, start, n, solid_map, s2c, nsources, nchannels, tbins=0, t_lo=0.0, inv=0.0, earliest=True,
              weights=False, detection_state=SURFACE_DETECT, into=None):
    """The map's words after photons [start, start+n) of `ph` (evidx, flags,
    last_hit_triangles, t, weights), as a dict over ARRAYS (None where not kept);
    `into`: such a dict to add to."""
    words = nsources * nchannels
    m = into if into is not None else dict(
        emitted=np.zeros(nsources, np.uint64), counts=np.zeros(words, np.uint32),
        tmin=np.full(words, NO_KEY, np.uint32) if earliest else None,
        thist=np.zeros(words * tbins, np.uint32) if tbins else None,
        wsum=np.zeros(words, np.uint64) if weights else None, skipped=np.zeros(1, np.uint64))
    sl = slice(start, start + n)
    s = np.asarray(ph.evidx, np.uint32)[sl].astype(np.int64)
    flags = np.asarray(ph.flags, np.uint32)[sl]
    last = np.asarray(ph.last_hit_triangles, np.int32)[sl].astype(np.int64)
    t = np.asarray(ph.t, np.float32)[sl]
    w = np.asarray(ph.weights, np.float32)[sl]
    known = s < nsources                                                     # step 1
    m['skipped'][0] += np.uint64((~known).sum())
    np.add.at(m['emitted'], s[known], np.uint64(1))                          # step 2
    hit = known & ((flags & np.uint32(detection_state)) != 0) & (last > -1)  # step 3
    c = np.full(len(s), -1, np.int64)
    c[hit] = np.asarray(s2c, np.int64)[np.asarray(solid_map, np.int64)[last[hit]]]
    hit &= (c >= 0) & (c < nchannels)
    word = (s * nchannels + c)[hit]                                          # step 4
    np.add.at(m['counts'], word, np.uint32(1))
    t, w = t[hit], w[hit]
    if earliest:                                                             # step 5
        timed = ~np.isnan(t)
        np.minimum.at(m['tmin'], word[timed], keys_of(t[timed]))
    if tbins:                                                                # step 6
        with np.errstate(invalid='ignore', over='ignore'):
            x = (t - np.float32(t_lo)) * np.float32(inv)
            inside = (x >= np.float32(0)) & (x < np.float32(tbins))
        np.add.at(m['thist'], word[inside] * tbins + x[inside].astype(np.uint32), np.uint32(1))
    if weights:                                                              # step 7
        np.add.at(m['wsum'], word, weight_words(w))
    return m


def words_of(hm):
    """The words of a GPUHitMap / HostHitMap as numpy_map returns them."""
    out = {}
    for name in ARRAYS:
        a = getattr(hm, name)
        out[name] = None if a is None else (a.copy() if isinstance(a, np.ndarray) else a.get())
    return out


def assert_same_words(got, want, label=''):
    for name in ARRAYS:
        if want[name] is None:
            assert got[name] is None, '%s: %s kept but not asked for' % (label, name)
        else:
            assert got[name] is not None and got[name].dtype == want[name].dtype, (label, name)
            assert np.array_equal(got[name], want[name]), '%s: %s words differ' % (label, name)


# ---------------------------------------------------------------- made records on the 2-PMT detector
N_MADE = 3000
NSOURCES = len(SIZES)
START, N_USED = int(BOUNDS[0]), int(BOUNDS[-1] - BOUNDS[0])
TBINS, TRANGE = 8, (16.0, 80.0)               # inv = 0.125 and t - t_lo near t_hi are exact
T_BELOW_HI = np.nextafter(np.float32(TRANGE[1]), np.float32(0))
KINDS = ('ch0', 'ch1', 'no_channel', 'no_hit', 'wire', 'not_detected', 't_negative', 't_inf', 't_nan', 't_lo',
         't_below_hi', 't_hi', 'w_zero', 'w_0.3', 'w_nan', 'w_300', 'foreign')
# every combination of the optional arrays' presence the tests run
OPTIONS = (dict(tbins=TBINS, trange=TRANGE, earliest=True, weights=True),
           dict(tbins=0, trange=None, earliest=True, weights=True),
           dict(tbins=TBINS, trange=TRANGE, earliest=False, weights=True),
           dict(tbins=TBINS, trange=TRANGE, earliest=True, weights=False),
           dict(tbins=0, trange=None, earliest=False, weights=False))


def detector_maps(detector):
    """The (host) stand-in HostHitMap takes, of a Detector."""
    return SimpleNamespace(solid_id_map=np.asarray(detector.solid_id, np.uint32),
                           solid_id_to_channel_index_gpu=np.asarray(detector.solid_id_to_channel_index, np.int32),
                           nchannels=int(detector.num_channels()))


def made_records(detector, shuffled=False, seed=91):
    """N_MADE records cycling through KINDS, the sources of test_daq_events.BOUNDS
    (source e = photons [BOUNDS[e], BOUNDS[e+1]); the 'foreign' kind carries an evidx
    that is no source).  shuffled: the same records with evidx permuted."""
    from chroma.event import Photons
    n = N_MADE
    r = np.random.RandomState(seed)
    solid = np.asarray(detector.solid_id)
    s2c = np.asarray(detector.solid_id_to_channel_index)
    tri = {c: np.flatnonzero(s2c[solid] == c) for c in (-1, 0, 1)}
    assert all(len(v) > 0 for v in tri.values())
    kind = np.arange(n) % len(KINDS)
    k = {name: kind == i for i, name in enumerate(KINDS)}
    channel = (np.arange(n) // len(KINDS)) % 2          # of the kinds that only vary t or the weight
    channel[k['ch0']], channel[k['ch1']], channel[k['no_channel']] = 0, 1, -1
    last = np.empty(n, np.int32)
    for c in (-1, 0, 1):
        last[channel == c] = r.choice(tri[c], int((channel == c).sum()))
    last[k['no_hit']] = -1
    last[k['wire']] = -2
    flags = np.full(n, SURFACE_DETECT, np.uint32)
    flags |= np.where(r.uniform(size=n) < 0.3, REFLECT_DIFFUSE, 0).astype(np.uint32)
    flags[k['not_detected']] = SURFACE_ABSORB | REFLECT_DIFFUSE
    t = r.uniform(5.0, 120.0, n).astype(np.float32)
    t[k['t_negative']] = r.uniform(-80.0, -1.0, int(k['t_negative'].sum())).astype(np.float32)
    t[k['t_inf']], t[k['t_nan']] = np.inf, np.nan
    t[k['t_lo']], t[k['t_below_hi']], t[k['t_hi']] = TRANGE[0], T_BELOW_HI, TRANGE[1]
    w = np.where(r.uniform(size=n) < 0.5, 1.0, r.uniform(0.05, 0.95, n)).astype(np.float32)
    w[k['w_zero']], w[k['w_0.3']], w[k['w_nan']], w[k['w_300']] = 0.0, 0.3, np.nan, 300.0
    evidx = np.zeros(n, np.uint32)
    for e in range(NSOURCES):
        evidx[BOUNDS[e]:BOUNDS[e + 1]] = e
    evidx[k['foreign']] = np.where(np.arange(int(k['foreign'].sum())) % 2, NSOURCES, 0xFFFFFFFF)
    if shuffled:
        evidx = evidx[r.permutation(n)]
    pos = np.zeros((n, 3), np.float32)
    dir = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    pol = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    return Photons(pos, dir, pol, np.full(n, 400.0, np.float32), t=t, last_hit_triangles=last, flags=flags,
                   weights=w, evidx=evidx), kind


# ---------------------------------------------------------------- 4096 channels through a stand-in
WIDE_CHANNELS, WIDE_SOURCES, WIDE_PER_SOURCE = 4096, 8, 1000


def wide_maps():
    """4096 triangles, each its own solid and channel (the channels permuted)."""
    r = np.random.RandomState(17)
    return SimpleNamespace(solid_id_map=np.arange(WIDE_CHANNELS, dtype=np.uint32),
                           solid_id_to_channel_index_gpu=r.permutation(WIDE_CHANNELS).astype(np.int32),
                           nchannels=WIDE_CHANNELS)


def wide_records(seed=23):
    """8 sources of 1000 photons on random channels; one in eight is not detected."""
    from chroma.event import Photons
    n = WIDE_SOURCES * WIDE_PER_SOURCE
    r = np.random.RandomState(seed)
    last = r.randint(0, WIDE_CHANNELS, n).astype(np.int32)
    last[::8] = -1
    flags = np.full(n, SURFACE_DETECT, np.uint32)
    t = r.uniform(-5.0, 70.0, n).astype(np.float32)
    w = r.uniform(0.0, 2.0, n).astype(np.float32)
    evidx = np.repeat(np.arange(WIDE_SOURCES, dtype=np.uint32), WIDE_PER_SOURCE)
    pos = np.zeros((n, 3), np.float32)
    dir = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    pol = np.tile(np.array([1, 0, 0], np.float32), (n, 1))
    return Photons(pos, dir, pol, np.full(n, 400.0, np.float32), t=t, last_hit_triangles=last, flags=flags,
                   weights=w, evidx=evidx)


def scale(tbins, trange):
    """(t_lo, inv) in float32, restated."""
    if not tbins:
        return np.float32(0), np.float32(0)
    return np.float32(trange[0]), np.float32(tbins) / (np.float32(trange[1]) - np.float32(trange[0]))


# ---------------------------------------------------------------- flashes in the 2-PMT detector
FLASH_SIZES = (700, 64, 1, 0, 3000, 333)
FLASH_SPOTS = ((0, 0, 0), (100, 50, -200), (-300, 0, 100), (0, 0, 500), (50, -100, 0), (0, 200, -400))
FLASH_SEED, FLASH_SLOTS = 11, 4096


def flashes(material_objects):
    """Six isotropic flashes in the detector's water, evidx 0-5.  With FLASH_SEED and
    FLASH_SLOTS states, after 100 steps, the oracle's propagate of the host twin's
    photons detects on both channels from sources 0 (6 and 4 photons) and 4 (16 and 23)."""
    from chroma import gensteps as gs
    water = [m for m in material_objects if getattr(m, 'name', None) == 'water'][0]
    return gs.Gensteps.join([gs.isotropic_flash(water, n, x0=x, evidx=i)
                             for i, (n, x) in enumerate(zip(FLASH_SIZES, FLASH_SPOTS))])
