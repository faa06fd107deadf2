"""Photoelectron trains and digitised waveforms: the pulse train behind a
channel's one time and one charge.

GPUDaq.acquire_photoelectrons keeps what the DAQ draws for every accepted
photon (GPUPhotoelectrons); .trains() bins those records into charge trains per
(event, channel) row and .digitise() convolves the trains with a
single-photoelectron template and quantises them to ADC words, all on the
device (chr_daq_pe_trains, chr_daq_digitise; include/chroma_amd.h documents
both rules).  HostWaveforms is the same over host arrays through the host
twins (the kernels' rule text built by the host compiler, word-identical, no
GPU needed).  Nothing here draws a random number: the RNG stream of a run with
waveforms is the stream of acquire_events.  Electronic noise is not modelled.

    chans, pe = daq.acquire_photoelectrons(gpu_photons, rng_states, bounds)
    wf = pe.trains((0.0, 128.0), 256).digitise(template, scale=gain * daq.charge_unit, pedestal=100.0)
    for w in wf.get():                    # one event.Waveforms per event
        w.channels, w.trains, w.adc
"""
import numpy as np

from chroma import event
from chroma.gpu import _native
from chroma.gpu.hitmap import bin_scale

NO_HIT_BITS = np.float32(1e9).view(np.uint32)      # the earliest-time word of a channel without a photoelectron
MAX_WORDS = 2 ** 31                                # of one array
LDS_WORDS = 16384                                  # CHR_WAVE_LDS_WORDS


class WaveformSpec(object):
    """What Simulation.simulate(..., run_daq=True, waveforms=spec) builds per
    event: charge trains of `nsamples` bins over trange=(t_lo, t_hi) for the hit
    channels (rows='hit') or all of them ('all'); with a `template` (the
    single-photoelectron response, one float per sample step) also the ADC words
    min(adc_max, round(pedestal + scale * (trains * template))) of adc_bits
    bits.  keep_photoelectrons: also fill ev.photoelectrons."""

    def __init__(self, trange, nsamples, template=None, scale=1.0, pedestal=0.0, adc_bits=12, rows='hit',
                 keep_photoelectrons=False):
        self.nsamples = int(nsamples)
        if self.nsamples <= 0:
            raise ValueError('nsamples must be positive')
        if trange is None or len(trange) != 2:
            raise ValueError('trange must be (t_lo, t_hi)')
        self.trange = (float(trange[0]), float(trange[1]))
        bin_scale(self.nsamples, self.trange)          # raises on a window without a positive finite scale
        if rows not in ('hit', 'all'):
            raise ValueError("rows must be 'hit' or 'all'")
        self.rows = rows
        self.template = None if template is None else check_template(template, self.nsamples)
        self.scale, self.pedestal = float(scale), float(pedestal)
        self.adc_bits = int(adc_bits)
        adc_max_of(self.adc_bits)
        self.keep_photoelectrons = bool(keep_photoelectrons)

    def event_bytes(self, nphotons, nchannels):
        """Bytes one event of `nphotons` photons adds to a DAQ group: the 16 bytes
        per channel of its rows and 4 per train word -- every word for
        rows='all', for 'hit' the bound of one row per photon."""
        rows = int(nchannels) if self.rows == 'all' else min(int(nphotons), int(nchannels))
        return 16 * int(nchannels) + 4 * self.nsamples * rows


def adc_max_of(adc_bits):
    if not 1 <= int(adc_bits) <= 16:
        raise ValueError('adc_bits must be 1 .. 16')
    return 2 ** int(adc_bits) - 1


def check_template(template, nsamples):
    t = np.ascontiguousarray(template, dtype=np.float32)
    if t.ndim != 1 or len(t) == 0:
        raise ValueError('the template must be a 1-D array of at least one tap')
    if nsamples + min(len(t), nsamples) > LDS_WORDS:
        raise ValueError('%d samples and %d taps exceed the %d words of a row' % (nsamples, len(t), LDS_WORDS))
    return t


def waveform_event_groups(bounds, nchannels, budget, spec):
    """daq_event_groups with the train words counted: consecutive groups
    [first, last) of the events with photon offsets `bounds`, each as many
    events as fit `budget` bytes by spec.event_bytes, at least one.  Every event
    is in exactly one group, in order."""
    sizes = np.diff(np.asarray(bounds, dtype=np.int64))
    groups, first, held = [], 0, 0
    for e, n in enumerate(sizes.tolist()):
        need = spec.event_bytes(n, nchannels)
        if e > first and held + need > int(budget):
            groups.append((first, e))
            first, held = e, 0
        held += need
    if len(sizes) > first:
        groups.append((first, len(sizes)))
    return groups


def hit_rows(time_int, nevents, nchannels):
    """(row_of_word, event, channel) of the zero-suppressed read-out: a row for
    every word of the (nevents, nchannels) earliest-time words that is not the
    1e9 pattern, in ascending (event, channel) order; -1 for the others."""
    hit = np.asarray(time_int, dtype=np.uint32).reshape(-1) != NO_HIT_BITS
    row_of_word = np.where(hit, np.cumsum(hit) - 1, -1).astype(np.int32)
    words = np.flatnonzero(hit)
    return row_of_word, (words // nchannels).astype(np.int32), (words % nchannels).astype(np.int32)


class _Waveforms(object):
    """The window, the row list and the arrays of a set of trains; subclasses say
    where the arrays live.  trains (nrows*nsamples u32), outside_q (nrows u32),
    adc (nrows*nsamples u16, None until digitise), `event` and `channel` of every
    row (host int32), dropped (photoelectrons without a row) and bad (samples
    that digitised from a NaN)."""

    def _window(self, trange, nsamples):
        self.nsamples = int(nsamples)
        if self.nsamples <= 0:
            raise ValueError('nsamples must be positive')
        self.trange = (float(trange[0]), float(trange[1]))
        self.t_lo, self.inv = bin_scale(self.nsamples, self.trange)
        self.dt = (float(np.float32(self.trange[1])) - float(self.t_lo)) / self.nsamples

    def _rows(self, rows, event, channel, row_of_word):
        """The row list; with a caller's map, a row's (event, channel) is that of
        its first word."""
        self.row_of_word = row_of_word
        self.event, self.channel = event, channel
        self.nrows = len(event)
        if self.nrows * self.nsamples > MAX_WORDS:
            raise ValueError('%d rows of %d samples exceed 2^31 train words' % (self.nrows, self.nsamples))
        self.adc, self.bad, self.dropped = None, 0, 0

    @staticmethod
    def _map_rows(row_of_word, nchannels):
        m = np.ascontiguousarray(row_of_word, dtype=np.int32).reshape(-1)
        nrows = int(m.max()) + 1 if len(m) and m.max() >= 0 else 0
        first = np.full(nrows, -1, np.int64)
        kept = np.flatnonzero(m >= 0)
        first[m[kept][::-1]] = kept[::-1]          # the lowest word of every row
        if (first < 0).any():
            raise ValueError('the row map leaves row %d without a word' % int(np.flatnonzero(first < 0)[0]))
        return m, (first // nchannels).astype(np.int32), (first % nchannels).astype(np.int32)

    def digitise(self, template, scale, pedestal=0.0, adc_bits=12):
        """Fill `adc`: every row convolved with `template` (ntaps floats, tap k
        weighs the charge k samples earlier), times `scale`, plus `pedestal`,
        rounded and clipped to [0, 2^adc_bits - 1].  Returns self."""
        taps = check_template(template, self.nsamples)
        adc_max = adc_max_of(adc_bits)
        self.adc = self._alloc(self.nrows * self.nsamples, np.uint16)
        self.bad = self._digitise(taps, float(scale), float(pedestal), adc_max)
        return self

    def get(self):
        """One event.Waveforms per event, each owning copies of its rows."""
        trains = self._host(self.trains).reshape(self.nrows, self.nsamples)
        outside = self._host(self.outside_q)
        adc = None if self.adc is None else self._host(self.adc).reshape(self.nrows, self.nsamples)
        order = np.argsort(self.event, kind='stable')      # the identity for 'hit' and 'all'
        cuts = np.searchsorted(self.event[order], np.arange(self.nevents + 1))
        out = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            r = order[a:b]
            out.append(event.Waveforms(self.channel[r], trains[r], None if adc is None else adc[r], outside[r],
                                       float(self.t_lo), self.dt))
        return out


class GPUPhotoelectrons(object):
    """The photoelectron records GPUDaq.acquire_photoelectrons left on the device,
    one per photon of [bounds[0], bounds[-1]) and indexed from bounds[0]: channel
    (i32, -1 where the photon made no photoelectron), t (f32, the time handed to
    the channel's earliest-time minimum; 1e9 where none) and q_int (u32 quantised
    charge; 0 where none).  It owns its arrays, and a copy of the events'
    earliest-time words for the zero-suppressed row list."""

    def __init__(self, channel, t, q_int, bounds, nchannels, charge_unit, time_int):
        self.channel, self.t, self.q_int = channel, t, q_int
        self.bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        self.nevents = len(self.bounds) - 1
        self.nchannels = int(nchannels)
        self.charge_unit = float(charge_unit)
        self.time_int = time_int

    def __len__(self):
        return self.nevents

    def get(self):
        """One event.Photoelectrons per event: channel, t, q_int and q = q_int *
        charge_unit of the accepted photons, in photon order."""
        c, t, q = self.channel.get(), self.t.get(), self.q_int.get()
        out = []
        for a, b in zip(self.bounds[:-1] - self.bounds[0], self.bounds[1:] - self.bounds[0]):
            keep = c[a:b] >= 0
            out.append(event.Photoelectrons(c[a:b][keep], t[a:b][keep], q[a:b][keep],
                                            q[a:b][keep].astype(np.float32) * np.float32(self.charge_unit)))
        return out

    def trains(self, trange, nsamples, rows='hit'):
        """The charge trains of the records over the window trange=(t_lo, t_hi) in
        nsamples bins (GPUWaveforms): a row per hit channel (rows='hit': the
        words whose earliest time is not 1e9, in ascending (event, channel)
        order), per channel ('all'), or as an int32 map of nevents*nchannels
        entries says (-1: no row; its photoelectrons count in `dropped`)."""
        return GPUWaveforms(self, trange, nsamples, rows)


class GPUWaveforms(_Waveforms):
    """Charge trains on the device (chr_daq_pe_trains), and after digitise() their
    ADC words (chr_daq_digitise).  trains, outside_q and adc are GPUArrays."""

    def __init__(self, pe, trange, nsamples, rows='hit'):
        import torch
        from chroma.gpu import gpuarray as ga
        from chroma.gpu.tools import current_stream
        self._window(trange, nsamples)
        self.nevents, self.nchannels = pe.nevents, pe.nchannels
        words = self.nevents * self.nchannels
        if isinstance(rows, str) and rows == 'all':
            idx = np.arange(words)
            self._rows(rows, (idx // self.nchannels).astype(np.int32), (idx % self.nchannels).astype(np.int32), None)
        elif isinstance(rows, str) and rows == 'hit':
            # torch plumbing: the row of every hit word is its rank among the hit words
            hit = pe.time_int.tensor != int(NO_HIT_BITS)
            rank = torch.cumsum(hit, 0, dtype=torch.int32) - 1
            row_of_word = ga.from_tensor(torch.where(hit, rank, torch.full_like(rank, -1)), np.int32)
            w = torch.nonzero(hit).reshape(-1).cpu().numpy()
            self._rows(rows, (w // self.nchannels).astype(np.int32), (w % self.nchannels).astype(np.int32),
                       row_of_word)
        elif isinstance(rows, str):
            raise ValueError("rows must be 'hit', 'all' or a map of the (event, channel) words")
        else:
            m, ev, ch = self._map_rows(rows, self.nchannels)
            if len(m) != words:
                raise ValueError('a row map needs %d entries' % words)
            self._rows('map', ev, ch, ga.to_gpu(m) if len(m) else ga.empty(0, np.int32))
        self.trains = self._alloc(self.nrows * self.nsamples, np.uint32)
        self.outside_q = self._alloc(self.nrows, np.uint32)
        dropped = ga.empty(1, np.uint32)
        m = self.row_of_word
        _native.call('chr_daq_pe_trains', pe.channel.gpudata, pe.t.gpudata, pe.q_int.gpudata, pe.bounds.ctypes.data,
                     self.nevents, self.nchannels, None if m is None else m.gpudata, self.nrows, float(self.t_lo),
                     float(self.inv), self.nsamples, self.trains.gpudata, self.outside_q.gpudata, dropped.gpudata,
                     current_stream())
        self.dropped = int(dropped.get()[0])

    @staticmethod
    def _alloc(n, dtype):
        from chroma.gpu import gpuarray as ga
        return ga.empty(n + 1, dtype)[:n]          # one spare word: an empty array has no address to hand over

    @staticmethod
    def _host(a):
        return a.get()

    def _digitise(self, taps, scale, pedestal, adc_max):
        from chroma.gpu import gpuarray as ga
        from chroma.gpu.tools import current_stream
        bad = ga.empty(1, np.uint32)
        device_taps = ga.to_gpu(taps)         # held until the download below has waited for the kernel
        _native.call('chr_daq_digitise', self.trains.gpudata, self.nrows, self.nsamples, device_taps.gpudata,
                     len(taps), scale, pedestal, adc_max, self.adc.gpudata, bad.gpudata, current_stream())
        return int(bad.get()[0])


class HostWaveforms(_Waveforms):
    """GPUWaveforms' twin over host arrays (chr_daq_pe_trains_host,
    chr_daq_digitise_host; no GPU): the photoelectron records as numpy arrays
    (pe_channel, pe_time, pe_q, one per photon of [bounds[0], bounds[-1])), the
    events' `bounds` and the channel count.  rows as GPUPhotoelectrons.trains;
    'hit' needs `time_int`, the events' earliest-time words."""

    def __init__(self, pe_channel, pe_time, pe_q, bounds, nchannels, trange, nsamples, rows='all', time_int=None):
        self._window(trange, nsamples)
        bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        if bounds.ndim != 1 or len(bounds) < 1:
            raise ValueError('bounds must be a 1-D array of nevents + 1 photon offsets')
        self.nevents, self.nchannels = len(bounds) - 1, int(nchannels)
        words = self.nevents * self.nchannels
        span = int(bounds[-1] - bounds[0])
        pe = [np.ascontiguousarray(a, dtype=d) for a, d in
              ((pe_channel, np.int32), (pe_time, np.float32), (pe_q, np.uint32))]
        if any(a.ndim != 1 or len(a) != span for a in pe):
            raise ValueError('the records must be three 1-D arrays of bounds[-1] - bounds[0] = %d entries' % span)
        if isinstance(rows, str) and rows == 'all':
            idx = np.arange(words)
            self._rows(rows, (idx // self.nchannels).astype(np.int32), (idx % self.nchannels).astype(np.int32), None)
        elif isinstance(rows, str) and rows == 'hit':
            if time_int is None or np.size(time_int) != words:
                raise ValueError("rows='hit' needs the %d earliest-time words" % words)
            m, ev, ch = hit_rows(time_int, self.nevents, self.nchannels)
            self._rows(rows, ev, ch, m)
        elif isinstance(rows, str):
            raise ValueError("rows must be 'hit', 'all' or a map of the (event, channel) words")
        else:
            m, ev, ch = self._map_rows(rows, self.nchannels)
            if len(m) != words:
                raise ValueError('a row map needs %d entries' % words)
            self._rows('map', ev, ch, m)
        # one spare word: an empty array has no address to hand over
        self.trains = np.empty(self.nrows * self.nsamples + 1, np.uint32)[:self.nrows * self.nsamples]
        self.outside_q = np.empty(self.nrows + 1, np.uint32)[:self.nrows]
        dropped = np.zeros(1, np.uint32)
        m = self.row_of_word
        if m is not None and len(m) == 0:
            m = np.zeros(1, np.int32)
        _native.call('chr_daq_pe_trains_host', *[a.ctypes.data if len(a) else np.zeros(1, a.dtype).ctypes.data
                                                 for a in pe],
                     bounds.ctypes.data, self.nevents, self.nchannels, None if m is None else m.ctypes.data,
                     self.nrows, float(self.t_lo), float(self.inv), self.nsamples, self.trains.ctypes.data,
                     self.outside_q.ctypes.data, dropped.ctypes.data)
        self.dropped = int(dropped[0])

    @staticmethod
    def _alloc(n, dtype):
        return np.empty(n + 1, dtype)[:n]

    @staticmethod
    def _host(a):
        return a

    def _digitise(self, taps, scale, pedestal, adc_max):
        bad = np.zeros(1, np.uint32)
        _native.call('chr_daq_digitise_host', self.trains.ctypes.data, self.nrows, self.nsamples, taps.ctypes.data,
                     len(taps), scale, pedestal, adc_max, self.adc.ctypes.data, bad.ctypes.data)
        return int(bad[0])
