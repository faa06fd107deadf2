"""Hit maps: per source and channel, how many photons arrived, when the first
one did and how the arrival times are distributed -- the optical map (photon
library) of fast simulation and reconstruction, accumulated on the device by
chr_hitmap_accumulate (include/chroma_amd.h documents the per-photon rule).

A photon's source is its evidx.  GPUHitMap holds the map's arrays on the
device and adds any GPUPhotons to them; HostHitMap is the same over host arrays
through the host twin (chr_hitmap_accumulate_host: the kernel's source built by
the host compiler, word-identical, no GPU needed).  get() gives a HitMap.

    hm = gpu.GPUHitMap(gpu_detector, nsources=1000, tbins=50, trange=(0.0, 100.0))
    hm.accumulate(gpu_photons)            # after a propagate; as often as needed
    table = hm.get()                      # counts (1000, nchannels), emitted, tmin, thist, ...
    vis = table.visibility()
"""
import ctypes

import numpy as np

from chroma.gpu import _native

SURFACE_DETECT = 0x1 << 2
NO_KEY = np.uint32(0xFFFFFFFF)        # the cleared tmin word
WEIGHT_UNIT = 2.0 ** -24              # one wsum word
LDS_WORDS = 8192                      # CHR_HITMAP_LDS_WORDS: the row the privatised path keeps in LDS
MAX_WORDS = 2 ** 31                   # of one array
DIRECT, PRIVATISED = 0, 1             # chr_hitmap_last_path


def time_keys(t):
    """The order-preserving uint32 keys of float32 times (rule step 5)."""
    b = np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000))


def times_of_keys(keys):
    """The float32 times of tmin words; +inf where the word was never written."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF))
    t = b.astype(np.uint32).view(np.float32).copy()
    t[k == NO_KEY] = np.inf
    return t


def bin_scale(tbins, trange):
    """(t_lo, inv) as float32: inv = tbins / (t_hi - t_lo), every operation in float32."""
    if not tbins:
        return np.float32(0.0), np.float32(0.0)
    if trange is None:
        raise ValueError('tbins > 0 needs trange=(t_lo, t_hi)')
    t_lo, t_hi = np.float32(trange[0]), np.float32(trange[1])
    with np.errstate(all='ignore'):
        inv = np.float32(np.float32(tbins) / np.float32(t_hi - t_lo))
    if not (np.isfinite(inv) and inv > 0):
        raise ValueError('trange=(%r, %r) gives no positive finite bin scale' % (trange[0], trange[1]))
    return t_lo, inv


class HitMap(object):
    """A hit map on the host.  counts (nsources, nchannels) uint32; emitted
    (nsources,) uint64; tmin (nsources, nchannels) float32, +inf where no time
    was recorded, or None; thist (nsources, nchannels, tbins) uint32 or None;
    wsum (nsources, nchannels) float64 (sum of weights, in steps of 2^-24) or
    None; skipped: photons whose evidx was no source."""

    def __init__(self, counts, emitted, tmin=None, thist=None, wsum=None, skipped=0, t_lo=0.0, inv=0.0):
        self.counts, self.emitted, self.tmin, self.thist, self.wsum = counts, emitted, tmin, thist, wsum
        self.skipped = int(skipped)
        self.t_lo, self.inv = np.float32(t_lo), np.float32(inv)
        self.nsources, self.nchannels = counts.shape

    @classmethod
    def from_words(cls, nsources, nchannels, tbins, emitted, counts, tmin=None, thist=None, wsum=None, skipped=0,
                   t_lo=0.0, inv=0.0):
        """A HitMap of the map's words as the device holds them.  OverflowError
        when a source emitted 2^32 photons or more: a uint32 count of it may
        have wrapped."""
        emitted = np.asarray(emitted, dtype=np.uint64).reshape(nsources)
        if (emitted >= np.uint64(2 ** 32)).any():
            s = int(np.flatnonzero(emitted >= np.uint64(2 ** 32))[0])
            raise OverflowError('source %d emitted %d photons: its uint32 counts may have wrapped'
                                % (s, int(emitted[s])))
        shape = (nsources, nchannels)
        return cls(np.asarray(counts, dtype=np.uint32).reshape(shape).copy(), emitted.copy(),
                   None if tmin is None else times_of_keys(tmin).reshape(shape),
                   None if thist is None else np.asarray(thist, dtype=np.uint32).reshape(shape + (tbins,)).copy(),
                   None if wsum is None else np.asarray(wsum, dtype=np.uint64).reshape(shape) * WEIGHT_UNIT,
                   skipped, t_lo, inv)

    def visibility(self):
        """counts / emitted per (source, channel), float64; 0 where nothing was emitted."""
        out = np.zeros(self.counts.shape, np.float64)
        lit = self.emitted > 0
        out[lit] = self.counts[lit] / self.emitted[lit].astype(np.float64)[:, None]
        return out


class _Map(object):
    """The parameters and the six arrays of a map; subclasses say where they live."""
    _ARRAYS = (('emitted', np.uint64), ('counts', np.uint32), ('tmin', np.uint32), ('thist', np.uint32),
               ('wsum', np.uint64), ('skipped', np.uint64))

    def _setup(self, detector, nsources, tbins, trange, earliest, weights):
        self.nsources, self.nchannels, self.tbins = int(nsources), int(detector.nchannels), int(tbins)
        if self.nsources <= 0 or self.nchannels <= 0 or self.tbins < 0:
            raise ValueError('%d sources of %d channels with %d time bins' % (self.nsources, self.nchannels,
                                                                             self.tbins))
        self.t_lo, self.inv = bin_scale(self.tbins, trange)
        words = self.nsources * self.nchannels
        if max(self.nsources, words, words * self.tbins) > MAX_WORDS:
            raise ValueError('%d sources x %d channels x %d bins exceed 2^31 words'
                             % (self.nsources, self.nchannels, self.tbins))
        self.solid_id_map = detector.solid_id_map
        self.solid_id_to_channel_index = detector.solid_id_to_channel_index_gpu
        sizes = dict(emitted=self.nsources, counts=words, tmin=words if earliest else 0,
                     thist=words * self.tbins, wsum=words if weights else 0, skipped=1)
        for name, dtype in self._ARRAYS:
            setattr(self, name, self._alloc(sizes[name], dtype) if sizes[name] else None)
        self.clear()

    @property
    def row_words(self):
        """Words of one source's row (what the privatised path must fit into LDS_WORDS)."""
        return self.nchannels * (1 + (self.tmin is not None) + self.tbins + 2 * (self.wsum is not None))

    def _desc(self):
        ptr = [self._ptr(getattr(self, name)) for name, _ in self._ARRAYS]
        return _native.HitMapDesc(self.nsources, self.nchannels, self.tbins, float(self.t_lo), float(self.inv), *ptr)

    def get(self):
        host = {name: None if getattr(self, name) is None else self._host(getattr(self, name))
                for name, _ in self._ARRAYS}
        return HitMap.from_words(self.nsources, self.nchannels, self.tbins, host['emitted'], host['counts'],
                                 host['tmin'], host['thist'], host['wsum'], int(host['skipped'][0]), self.t_lo,
                                 self.inv)


class GPUHitMap(_Map):
    """A hit map on the device.  gpu_detector: anything with `solid_id_map`
    (uint32 GPUArray, solid of each triangle), `solid_id_to_channel_index_gpu`
    (int32 GPUArray) and `nchannels` -- a GPUDetector, or a stand-in.  tbins,
    trange=(t_lo, t_hi): the time histogram; earliest: keep tmin; weights: keep
    wsum.  The arrays `emitted`, `counts`, `tmin`, `thist`, `wsum`, `skipped`
    are GPUArrays of the map's words (None where not kept) for callers who
    keep the map on the device; see include/chroma_amd.h for their layout."""

    def __init__(self, gpu_detector, nsources, tbins=0, trange=None, earliest=True, weights=False):
        self.last_path = None
        self._setup(gpu_detector, nsources, tbins, trange, earliest, weights)

    @staticmethod
    def _alloc(n, dtype):
        from chroma.gpu import gpuarray as ga
        return ga.empty(n, dtype)

    @staticmethod
    def _ptr(a):
        return None if a is None else a.gpudata

    @staticmethod
    def _host(a):
        return a.get()

    def clear(self):
        from chroma.gpu.tools import current_stream
        _native.call('chr_hitmap_clear', ctypes.byref(self._desc()), current_stream())

    def accumulate(self, gpuphotons, start_photon=None, nphotons=None, detection_state=SURFACE_DETECT):
        """Add photons [start_photon, start_photon + nphotons) of a GPUPhotons
        (default: all) to the map; asynchronous on the current stream.
        `last_path` records the path the call took (DIRECT or PRIVATISED)."""
        from chroma.gpu.tools import current_stream
        start = 0 if start_photon is None else int(start_photon)
        n = len(gpuphotons) - start if nphotons is None else int(nphotons)
        if start < 0 or n < 0 or start + n > len(gpuphotons):
            raise ValueError('photons [%d, %d) of %d' % (start, start + n, len(gpuphotons)))
        _native.call('chr_hitmap_accumulate', ctypes.byref(gpuphotons._desc()), start, n, int(detection_state),
                     self.solid_id_map.gpudata, self.solid_id_to_channel_index.gpudata, ctypes.byref(self._desc()),
                     current_stream())
        if n > 0:
            self.last_path = int(_native.lib().chr_hitmap_last_path())


class HostHitMap(_Map):
    """GPUHitMap's twin over host arrays (chr_hitmap_accumulate_host; no GPU):
    `detector` holds numpy arrays under the same three names, accumulate()
    takes an event.Photons (or anything with its evidx, flags,
    last_hit_triangles, t and weights arrays)."""

    def __init__(self, detector, nsources, tbins=0, trange=None, earliest=True, weights=False):
        self._setup(detector, nsources, tbins, trange, earliest, weights)
        self.solid_id_map = np.ascontiguousarray(self.solid_id_map, dtype=np.uint32)
        self.solid_id_to_channel_index = np.ascontiguousarray(self.solid_id_to_channel_index, dtype=np.int32)

    @staticmethod
    def _alloc(n, dtype):
        return np.empty(n, dtype)

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    @staticmethod
    def _host(a):
        return a

    def clear(self):
        for name, _ in self._ARRAYS:
            a = getattr(self, name)
            if a is not None:
                a[:] = NO_KEY if name == 'tmin' else 0

    def accumulate(self, photons, start_photon=None, nphotons=None, detection_state=SURFACE_DETECT):
        f32, u32 = np.float32, np.uint32
        fields = dict(evidx=np.ascontiguousarray(photons.evidx, dtype=u32),
                      flags=np.ascontiguousarray(photons.flags, dtype=u32),
                      last=np.ascontiguousarray(photons.last_hit_triangles, dtype=np.int32),
                      t=np.ascontiguousarray(photons.t, dtype=f32),
                      weights=np.ascontiguousarray(photons.weights, dtype=f32))
        total = len(fields['evidx'])
        start = 0 if start_photon is None else int(start_photon)
        n = total - start if nphotons is None else int(nphotons)
        if start < 0 or n < 0 or start + n > total or any(len(a) != total for a in fields.values()):
            raise ValueError('photons [%d, %d) of %d' % (start, start + n, total))
        desc = _native.PhotonsDesc(None, None, None, None, fields['t'].ctypes.data, fields['weights'].ctypes.data,
                                   fields['flags'].ctypes.data, fields['last'].ctypes.data,
                                   fields['evidx'].ctypes.data)
        _native.call('chr_hitmap_accumulate_host', ctypes.byref(desc), start, n, int(detection_state),
                     self.solid_id_map.ctypes.data, self.solid_id_to_channel_index.ctypes.data,
                     ctypes.byref(self._desc()))
