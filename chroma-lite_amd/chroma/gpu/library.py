"""Photon-library lookup: from a hit map (the library) and the entries of some
events, every event's expected charge and earliest time per channel, or sampled
channels, on the device without propagating a photon (chr_library_expect,
chr_library_sample; include/chroma_amd.h documents both rules) -- and the way
back: the log-likelihood of one observed event under many hypotheses, each a set
of entries (chr_library_loglike; chroma.likelihood.LibraryLikelihood scans and
fits with it).

GPUPhotonLibrary holds the map's arrays on the device; HostPhotonLibrary is the
same over host arrays through the host twins (the kernels' source built by the
host compiler, word-identical, no GPU needed).

    lib = gpu.GPUPhotonLibrary(sim.hit_map(grid.flashes(water, 100000), grid.nvoxels), grid=grid)
    entries = entries_from_gensteps(grid, [steps])
    table = lib.expect(entries).get()                  # .mu, .tfirst: (nevents, nchannels)
    channels = lib.sample(entries, rng_states).get()   # one event.Channels per event
    ll = lib.log_likelihood(entries, n, t).get().ll    # per hypothesis (event of the table), float64
"""
import ctypes

import numpy as np

from chroma import event
from chroma.gpu import _native
from chroma.gpu.hitmap import NO_KEY, HitMap, time_keys
from chroma.library import MAX_WORDS, LibraryEntries, VoxelGrid

NARROW, WIDE = 0, 1                   # chr_library_last_path
NO_HIT_TIME = np.float32(1e9)         # the DAQ's time of a channel without a hit
_ARRAYS = (('emitted', np.uint64), ('counts', np.uint32), ('tmin', np.uint32), ('thist', np.uint32))


class Expected(object):
    """expect()'s outputs where they were computed: `mu`, `tfirst` (None when the
    library keeps no tmin), `skipped`; get() brings them to the host, mu and
    tfirst as (nevents, nchannels) float32, skipped as an int."""

    def __init__(self, nevents, nchannels, mu, tfirst, skipped, host):
        self.nevents, self.nchannels, self.mu, self.tfirst, self.skipped, self._host = \
            nevents, nchannels, mu, tfirst, skipped, host

    def get(self):
        shape = (self.nevents, self.nchannels)
        return Expected(self.nevents, self.nchannels, self._host(self.mu).reshape(shape),
                        None if self.tfirst is None else self._host(self.tfirst).reshape(shape),
                        int(self._host(self.skipped)[0]), lambda a: a)


class Sampled(object):
    """sample()'s outputs where they were computed: `n` (uint32), `t` (float32),
    `skipped`; get() gives one event.Channels per event: hit = n > 0, t, q = n
    as float32."""

    def __init__(self, nevents, nchannels, n, t, skipped, host):
        self.nevents, self.nchannels, self.n, self.t, self.skipped, self._host = nevents, nchannels, n, t, skipped, host

    def get(self):
        n = self._host(self.n).reshape(self.nevents, self.nchannels)
        t = self._host(self.t).reshape(self.nevents, self.nchannels)
        return [event.Channels(n[e] > 0, t[e].copy(), n[e].astype(np.float32)) for e in range(self.nevents)]


class LogLikelihood(object):
    """log_likelihood()'s outputs where they were computed: `words` (int64, one per
    hypothesis, in units of 2^-20), `bad` (uint32: the channels whose term was a NaN
    and counted as 0), `skipped`; get() brings them to the host and adds `ll`, the
    log-likelihoods as float64 (words / 2**20), with skipped as an int."""

    def __init__(self, nhypotheses, words, bad, skipped, host):
        self.nhypotheses, self.words, self.bad, self.skipped, self._host = nhypotheses, words, bad, skipped, host
        self.ll = None

    def get(self):
        out = LogLikelihood(self.nhypotheses, self._host(self.words), self._host(self.bad),
                            int(self._host(self.skipped)[0]), lambda a: a)
        out.ll = out.words.astype(np.float64) / 2.0 ** 20
        return out


MODES = {'poisson': 0, 'hit': 1}


def expected_channels(expected):
    """One event.Channels per event of a host Expected: q = mu, hit = mu > 0, t =
    tfirst where hit (1e9 elsewhere, and everywhere when the library keeps no tmin)."""
    out = []
    for e in range(expected.nevents):
        hit = expected.mu[e] > 0
        t = np.full(expected.nchannels, NO_HIT_TIME, np.float32)
        if expected.tfirst is not None:
            t[hit] = expected.tfirst[e][hit]
        out.append(event.Channels(hit, t, expected.mu[e].copy()))
    return out


class _Library(object):
    """The scalars and the four arrays of a library; subclasses say where they live."""
    last_loglike_path = None

    def _setup(self, source, grid):
        if grid is not None and not isinstance(grid, VoxelGrid):
            raise TypeError('grid must be a chroma.library.VoxelGrid')
        self.grid = grid
        if isinstance(source, HitMap):
            self.nsources, self.nchannels = int(source.nsources), int(source.nchannels)
            self.tbins = 0 if source.thist is None else int(source.thist.shape[2])
            self.t_lo, self.inv = np.float32(source.t_lo), np.float32(source.inv)
            tmin = None
            if source.tmin is not None:
                tmin = time_keys(source.tmin.reshape(-1)).astype(np.uint32)
                tmin[np.isposinf(source.tmin.reshape(-1))] = NO_KEY        # "no time" and +inf look up alike
            words = dict(emitted=source.emitted, counts=source.counts, tmin=tmin, thist=source.thist)
            for name, dtype in _ARRAYS:
                a = words[name]
                setattr(self, name, None if a is None else
                        self._upload(np.ascontiguousarray(a, dtype=dtype).reshape(-1)))
        else:                                                              # a GPUHitMap / HostHitMap: no copy
            self.nsources, self.nchannels, self.tbins = source.nsources, source.nchannels, source.tbins
            self.t_lo, self.inv = np.float32(source.t_lo), np.float32(source.inv)
            for name, _ in _ARRAYS:
                setattr(self, name, self._adopt(getattr(source, name)))
        if grid is not None and grid.nvoxels != self.nsources:
            raise ValueError('a grid of %d voxels for a library of %d sources' % (grid.nvoxels, self.nsources))
        if self.nsources <= 0 or self.nchannels <= 0:
            raise ValueError('%d sources of %d channels' % (self.nsources, self.nchannels))

    def _desc(self):
        ptr = {name: self._ptr(getattr(self, name)) for name, _ in _ARRAYS}
        return _native.HitMapDesc(self.nsources, self.nchannels, self.tbins, float(self.t_lo), float(self.inv),
                                  ptr['emitted'], ptr['counts'], ptr['tmin'], ptr['thist'], None, None)

    def _entries(self, entries):
        if not isinstance(entries, LibraryEntries):
            raise TypeError('entries must be a chroma.library.LibraryEntries')
        if entries.nevents * self.nchannels > MAX_WORDS:
            raise ValueError('%d events x %d channels exceed 2^31 words' % (entries.nevents, self.nchannels))
        return entries

    def default_tfloor(self, floor):
        """floor / (t_hi - t_lo) of the library's time histogram as float32: the noise time
        density that normalises the time term of log_likelihood."""
        if self.tbins <= 0:
            raise ValueError('the library keeps no time histogram')
        return np.float32(float(np.float32(floor)) * float(self.inv) / self.tbins)

    def _observed(self, n, t, mode, floor, tfloor):
        """The chr_library_observed of an observed event and the arrays it points into."""
        if mode not in MODES:
            raise ValueError("mode must be 'poisson' or 'hit'")
        if t is not None and self.thist is None:
            raise ValueError('observed times need a library with a time histogram')
        if tfloor is None:
            tfloor = 0.0 if t is None else self.default_tfloor(floor)
        floor, tfloor = np.float32(floor), np.float32(tfloor)
        if not (floor >= 0 and tfloor >= 0):
            raise ValueError('floor = %r and tfloor = %r must not be negative or NaN' % (floor, tfloor))
        n = self._observed_array(n, np.uint32, 'n')
        t = None if t is None else self._observed_array(t, np.float32, 't')
        return (n, t), _native.LibraryObservedDesc(self._ptr(n), self._ptr(t), MODES[mode], float(floor), float(tfloor))

    def _host_observed_array(self, a, dtype, name):
        a = np.asarray(a)
        out = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        if out.size != self.nchannels:
            raise ValueError('%s holds %d words for %d channels' % (name, out.size, self.nchannels))
        if dtype == np.uint32 and not np.array_equal(out.astype(np.float64), a.reshape(-1)):
            raise ValueError('%s does not fit uint32' % name)
        return out

    def words(self):
        """The library's arrays on the host, as the device holds them (None where not kept)."""
        return {name: None if getattr(self, name) is None else self._host(getattr(self, name)) for name, _ in _ARRAYS}

    def save(self, path):
        """One .npz of the map's arrays, scalars and the grid (when there is one)."""
        out = {k: v for k, v in self.words().items() if v is not None}
        out.update(nsources=np.int64(self.nsources), nchannels=np.int64(self.nchannels), tbins=np.int64(self.tbins),
                   t_lo=np.float32(self.t_lo), inv=np.float32(self.inv))
        if self.grid is not None:
            out.update(grid_lo=self.grid.lo, grid_hi=self.grid.hi, grid_shape=np.asarray(self.grid.shape, np.int64))
        with open(path, 'wb') as f:
            np.savez(f, **out)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
        nsources, nchannels, tbins = int(d['nsources']), int(d['nchannels']), int(d['tbins'])
        grid = VoxelGrid(d['grid_lo'], d['grid_hi'], d['grid_shape']) if 'grid_shape' in d else None
        self = cls.__new__(cls)
        self.last_path = None
        self.grid, self.nsources, self.nchannels, self.tbins = grid, nsources, nchannels, tbins
        self.t_lo, self.inv = np.float32(d['t_lo']), np.float32(d['inv'])
        sizes = dict(emitted=nsources, counts=nsources * nchannels, tmin=nsources * nchannels,
                     thist=nsources * nchannels * tbins)
        for name, dtype in _ARRAYS:
            a = d.get(name)
            if a is not None and (a.dtype != dtype or a.size != sizes[name]):
                raise ValueError('%s: %s of %d words in the file' % (name, a.dtype, a.size))
            setattr(self, name, None if a is None else self._upload(np.ascontiguousarray(a).reshape(-1)))
        if self.emitted is None or self.counts is None or (tbins > 0) != (self.thist is not None):
            raise ValueError('%s holds no complete library' % path)
        return self


class GPUPhotonLibrary(_Library):
    """A photon library on the device.  source: a chroma.gpu.hitmap.HitMap (what
    Simulation.hit_map returns; uploaded) or a GPUHitMap (its device arrays are
    adopted without a copy and only ever read).  grid: the VoxelGrid whose voxels
    are the sources, carried for entries_from_gensteps and save()."""

    def __init__(self, source, grid=None):
        self.last_path = None
        self._setup(source, grid)

    @staticmethod
    def _upload(a):
        from chroma.gpu import gpuarray as ga
        return ga.to_gpu(a)

    @staticmethod
    def _adopt(a):
        return a

    @staticmethod
    def _ptr(a):
        return None if a is None else a.gpudata

    @staticmethod
    def _host(a):
        return a.get()

    def _upload_entries(self, entries):
        from chroma.gpu import gpuarray as ga
        entries = self._entries(entries)
        # one word at least, so an event list without entries still has addresses to pass
        pad = lambda a: ga.to_gpu(a if len(a) else np.zeros(1, a.dtype))      # noqa: E731
        arrays = [pad(entries.offsets), pad(entries.source), pad(entries.nphotons), pad(entries.t)]
        return arrays, _native.LibraryEntriesDesc(entries.nevents, *[a.gpudata for a in arrays])

    def expect(self, entries):
        """Expected charge and earliest time per event and channel; asynchronous on
        the current stream.  `last_path` records the path taken (NARROW or WIDE)."""
        from chroma.gpu import gpuarray as ga
        from chroma.gpu.tools import current_stream
        keep, desc = self._upload_entries(entries)
        n = entries.nevents * self.nchannels
        mu = ga.empty(n, np.float32)
        tfirst = ga.empty(n, np.float32) if self.tmin is not None else None
        skipped = ga.zeros(1, np.uint64)
        if entries.nevents > 0:     # an empty event list has no output address to pass
            _native.call('chr_library_expect', ctypes.byref(self._desc()), ctypes.byref(desc), mu.gpudata,
                         None if tfirst is None else tfirst.gpudata, skipped.gpudata, current_stream())
            self.last_path = int(_native.lib().chr_library_last_path())
        out = Expected(entries.nevents, self.nchannels, mu, tfirst, skipped, lambda a: a.get())
        out._keep = keep               # the entries' device arrays, until the launch has run
        return out

    def _observed_array(self, a, dtype, name):
        from chroma.gpu import gpuarray as ga
        if isinstance(a, ga.GPUArray):                 # e.g. a Sampled's n and t: used where they are
            if a.dtype != dtype or a.size != self.nchannels:
                raise ValueError('%s: a device array of %d %s words for %d channels' % (name, a.size, a.dtype,
                                                                                        self.nchannels))
            return a
        return ga.to_gpu(self._host_observed_array(a, dtype, name))

    def log_likelihood(self, entries, n, t=None, mode='poisson', floor=1e-3, tfloor=None):
        """The log-likelihood of one observed event under every hypothesis of `entries`
        (event h of the table is hypothesis h), by chr_library_loglike's rule
        (include/chroma_amd.h): a LogLikelihood.  n: the observed photo-electron counts
        per channel (or 0 / 1 for mode='hit'); t: the observed times of the hit channels,
        or None for no time term; both numpy arrays or device arrays (a Sampled's n and t
        of one event are used without a download).  floor: the expected noise charge per
        channel; tfloor: the noise time density, by default floor / (t_hi - t_lo) of the
        library's histogram.  The Poisson form leaves out lgamma(n + 1), which no
        hypothesis changes.  Asynchronous on the current stream; `last_loglike_path`
        records the path taken (NARROW or WIDE)."""
        from chroma.gpu import gpuarray as ga
        from chroma.gpu.tools import current_stream
        observed, obs = self._observed(n, t, mode, floor, tfloor)
        keep, desc = self._upload_entries(entries)
        count = max(entries.nevents, 1)
        words, bad = ga.empty(count, np.int64), ga.empty(count, np.uint32)
        skipped = ga.zeros(1, np.uint64)
        if entries.nevents > 0:
            _native.call('chr_library_loglike', ctypes.byref(self._desc()), ctypes.byref(desc), ctypes.byref(obs),
                         words.gpudata, bad.gpudata, skipped.gpudata, current_stream())
            self.last_loglike_path = int(_native.lib().chr_library_loglike_last_path())
        out = LogLikelihood(entries.nevents, words[:entries.nevents], bad[:entries.nevents], skipped,
                            lambda a: a.get())
        out._keep = (keep, observed)       # the device arrays the launch reads, until it has run
        return out

    def sample(self, entries, rng_states):
        """Sampled charge and time per event and channel, drawn from rng_states
        (chroma.gpu.get_rng_states), which advance; asynchronous on the current stream."""
        from chroma.gpu import gpuarray as ga
        from chroma.gpu.tools import current_stream
        keep, desc = self._upload_entries(entries)
        npairs = entries.nevents * self.nchannels
        n, t = ga.empty(npairs, np.uint32), ga.empty(npairs, np.float32)
        skipped = ga.zeros(1, np.uint64)
        if entries.nevents > 0:
            _native.call('chr_library_sample', ctypes.byref(self._desc()), ctypes.byref(desc), rng_states.gpudata,
                         int(rng_states.size), n.gpudata, t.gpudata, skipped.gpudata, current_stream())
        out = Sampled(entries.nevents, self.nchannels, n, t, skipped, lambda a: a.get())
        out._keep = keep
        return out


class HostPhotonLibrary(_Library):
    """GPUPhotonLibrary's twin over host arrays (chr_library_expect_host,
    chr_library_sample_host; no GPU).  source: a HitMap or a HostHitMap;
    sample() takes rng_states as 6*nslots uint32 (chroma.gensteps.rng_init_host),
    advanced in place."""

    def __init__(self, source, grid=None):
        self._setup(source, grid)

    @staticmethod
    def _upload(a):
        return np.array(a, copy=True)

    @staticmethod
    def _adopt(a):
        return a

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    @staticmethod
    def _host(a):
        return a.copy()

    def _entries_desc(self, entries):
        entries = self._entries(entries)
        return _native.LibraryEntriesDesc(entries.nevents, entries.offsets.ctypes.data, entries.source.ctypes.data,
                                          entries.nphotons.ctypes.data, entries.t.ctypes.data)

    def expect(self, entries):
        desc = self._entries_desc(entries)
        n = entries.nevents * self.nchannels
        mu = np.empty(n, np.float32)
        tfirst = np.empty(n, np.float32) if self.tmin is not None else None
        skipped = np.zeros(1, np.uint64)
        _native.call('chr_library_expect_host', ctypes.byref(self._desc()), ctypes.byref(desc), mu.ctypes.data,
                     None if tfirst is None else tfirst.ctypes.data, skipped.ctypes.data)
        return Expected(entries.nevents, self.nchannels, mu, tfirst, skipped, lambda a: a)

    _observed_array = _Library._host_observed_array

    def log_likelihood(self, entries, n, t=None, mode='poisson', floor=1e-3, tfloor=None):
        """GPUPhotonLibrary.log_likelihood over host arrays (chr_library_loglike_host)."""
        observed, obs = self._observed(n, t, mode, floor, tfloor)
        desc = self._entries_desc(entries)
        words, bad = np.zeros(entries.nevents, np.int64), np.zeros(entries.nevents, np.uint32)
        skipped = np.zeros(1, np.uint64)
        if entries.nevents > 0:
            _native.call('chr_library_loglike_host', ctypes.byref(self._desc()), ctypes.byref(desc), ctypes.byref(obs),
                         words.ctypes.data, bad.ctypes.data, skipped.ctypes.data)
        return LogLikelihood(entries.nevents, words, bad, skipped, lambda a: a)

    def sample(self, entries, rng_states):
        if not (isinstance(rng_states, np.ndarray) and rng_states.dtype == np.uint32 and rng_states.flags.c_contiguous
                and rng_states.size % 6 == 0):
            raise ValueError('rng_states: a contiguous uint32 array of 6*nslots words')
        desc = self._entries_desc(entries)
        npairs = entries.nevents * self.nchannels
        n, t = np.empty(npairs, np.uint32), np.empty(npairs, np.float32)
        skipped = np.zeros(1, np.uint64)
        _native.call('chr_library_sample_host', ctypes.byref(self._desc()), ctypes.byref(desc), rng_states.ctypes.data,
                     rng_states.size // 6, n.ctypes.data, t.ctypes.data, skipped.ctypes.data)
        return Sampled(entries.nevents, self.nchannels, n, t, skipped, lambda a: a)
