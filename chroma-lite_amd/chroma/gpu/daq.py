"""GPUDaq / GPUChannels (drop-in for reference chroma/gpu/daq.py:8-101).

The DAQ turns detected photons into per-channel readout: earliest time
(photon time + a sample of the detector's time CDF), integrated charge (a
sample of the charge CDF, quantised by charge_unit) and the OR of the photon
histories.  Kernels: csrc/daq.hip through the C ABI (chr_daq_begin /
chr_daq_acquire / chr_daq_end, and chr_daq_acquire_events /
chr_daq_acquire_events_many for all events of a batch in one call, and
chr_daq_acquire_events_pe, which also keeps every accepted photon's time and
charge for chroma.gpu.waveform); no host fallback.
"""
import ctypes

import numpy as np
import torch

from chroma import event
from chroma.gpu import _native
from chroma.gpu import gpuarray as ga
from chroma.gpu.tools import current_stream


class GPUChannels(object):
    """Per-channel device arrays t (f32), q (f32), flags (u32); ndaq copies of
    `stride` channels each (daq.py:8-36)."""

    def __init__(self, t, q, flags, ndaq=1, stride=None):
        self.t = t
        self.q = q
        self.flags = flags
        self.ndaq = ndaq
        self.stride = len(t) if stride is None else stride

    def iterate_copies(self):
        for i in range(self.ndaq):
            w = slice(i * self.stride, (i + 1) * self.stride)
            yield GPUChannels(self.t[w], self.q[w], self.flags[w])

    def get(self):
        t = self.t.get()
        q = self.q.get()
        # a channel counts as hit when its earliest time is below 1e8 (daq.py:32-34)
        return event.Channels(t < 1e8, t, q, self.flags.get())

    def __len__(self):
        return self.t.size


class GPUEventChannels(object):
    """The rows GPUDaq.acquire_events left on the device, nevents x nchannels each
    and row e = event e: time_int (u32, the f32 earliest times' bit patterns),
    q_int (u32 quantised charge), flags (u32 history) and q (f32 charge).  They
    are views of arrays the GPUDaq reuses: valid until its next acquire_events."""

    def __init__(self, time_int, q_int, flags, q, nevents, nchannels, host=None):
        self.time_int = time_int
        self.q_int = q_int
        self.flags = flags
        self.q = q
        self.nevents = nevents
        self.nchannels = nchannels
        self._host = host

    def get(self):
        """One event.Channels per event (hit = earliest time below 1e8, as
        GPUChannels.get).  t, q and flags are downloaded once each, through
        pinned host memory, and every event owns copies of its rows."""
        n = self.nevents * self.nchannels
        if n == 0:
            return []
        host = self._host(3 * n)        # the GPUDaq's pinned words, grown on demand
        for k, a in enumerate((self.time_int, self.q, self.flags)):
            host[k * n:(k + 1) * n].copy_(a.tensor.view(torch.int32), non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rows = host[:3 * n].numpy().reshape(3, self.nevents, self.nchannels)
        out = []
        for e in range(self.nevents):
            t = rows[0, e].view(np.float32).copy()
            out.append(event.Channels(t < 1e8, t, rows[1, e].view(np.float32).copy(),
                                      rows[2, e].view(np.uint32).copy()))
        return out

    def as_channels(self):
        """The rows as one GPUChannels of nevents copies of nchannels words (no
        copy, nothing downloaded): t is the f32 view of the time words."""
        t = ga.from_tensor(self.time_int.tensor.view(torch.float32), np.float32)
        return GPUChannels(t, self.q, self.flags, self.nevents, self.nchannels)

    def __len__(self):
        return self.nevents


class _DetectorDesc(ctypes.Structure):   # chr_daq_detector (include/chroma_amd.h)
    _fields_ = [('d_solid_id_to_channel_index', ctypes.c_void_p), ('d_time_cdf_x', ctypes.c_void_p),
                ('d_time_cdf_y', ctypes.c_void_p), ('d_charge_cdf_x', ctypes.c_void_p),
                ('d_charge_cdf_y', ctypes.c_void_p), ('nchannels', ctypes.c_int32), ('time_cdf_len', ctypes.c_int32),
                ('charge_cdf_len', ctypes.c_int32), ('charge_unit', ctypes.c_float)]


def detector_desc(gpu_detector):
    """chr_daq_detector for a GPUDetector (the reference's Detector struct,
    gpu/detector.py:29-40)."""
    return _DetectorDesc(gpu_detector.solid_id_to_channel_index_gpu.gpudata, gpu_detector.time_cdf_x_gpu.gpudata,
                         gpu_detector.time_cdf_y_gpu.gpudata, gpu_detector.charge_cdf_x_gpu.gpudata,
                         gpu_detector.charge_cdf_y_gpu.gpudata, int(gpu_detector.nchannels),
                         int(gpu_detector.time_cdf_len), int(gpu_detector.charge_cdf_len),
                         float(gpu_detector.charge_unit))


class GPUDaq(object):
    def __init__(self, gpu_detector, ndaq=1):
        assert gpu_detector.nchannels > 0, "Geometry has no detectors, DAQ can't be initialized."
        n = gpu_detector.nchannels * ndaq
        self.earliest_time_gpu = ga.empty(n, np.float32)
        self.earliest_time_int_gpu = ga.empty(n, np.uint32)
        self.channel_history_gpu = ga.zeros(n, np.uint32)
        self.channel_q_int_gpu = ga.zeros(n, np.uint32)
        self.channel_q_gpu = ga.zeros(n, np.float32)
        self.detector_gpu = gpu_detector.detector_gpu
        self.solid_id_map_gpu = gpu_detector.solid_id_map
        self.solid_id_to_channel_index_gpu = gpu_detector.solid_id_to_channel_index_gpu
        self._desc = detector_desc(gpu_detector)
        self.charge_unit = float(gpu_detector.charge_unit)
        self.nchannels = int(gpu_detector.nchannels)
        self.ndaq = ndaq
        self.stride = gpu_detector.nchannels
        self._event_rows = None      # acquire_events' device arrays, grown on demand
        self._event_host = None      # and the pinned host words GPUEventChannels.get stages through

    def begin_acquire(self, nthreads_per_block=64):
        """daq.py:56-60: earliest times = 1e9, charges and histories = 0."""
        _native.call('chr_daq_begin', self.earliest_time_int_gpu.gpudata, self.channel_q_int_gpu.gpudata,
                     self.channel_history_gpu.gpudata, len(self.earliest_time_int_gpu), ctypes.c_float(1e9),
                     current_stream())
        self.channel_q_gpu.fill(0)

    def acquire(self, gpuphotons, rng_states, nthreads_per_block=64, max_blocks=1024, start_photon=None,
                nphotons=None, weight=1.0):
        """daq.py:62-91 (run_daq for ndaq == 1, run_daq_many otherwise)."""
        start = 0 if start_photon is None else int(start_photon)
        n = len(gpuphotons.pos) - start if nphotons is None else int(nphotons)
        ph = gpuphotons._desc()
        normal = rng_states.normal_cache.gpudata if self.ndaq > 1 else None
        _native.call('chr_daq_acquire', ctypes.byref(ph), rng_states.gpudata, len(rng_states), normal,
                     0x1 << 2, start, n, self.solid_id_map_gpu.gpudata, ctypes.byref(self._desc),
                     self.earliest_time_int_gpu.gpudata, self.channel_q_int_gpu.gpudata,
                     self.channel_history_gpu.gpudata, int(self.ndaq), int(self.stride), ctypes.c_float(weight),
                     int(nthreads_per_block), int(max_blocks), current_stream())

    def end_acquire(self, nthreads_per_block=64):
        """daq.py:93-101: times back to float, charges * charge_unit."""
        _native.call('chr_daq_end', self.earliest_time_int_gpu.gpudata, self.earliest_time_gpu.gpudata,
                     self.channel_q_int_gpu.gpudata, self.channel_q_gpu.gpudata, len(self.earliest_time_int_gpu),
                     self.nchannels, ctypes.c_float(self.charge_unit), current_stream())
        return GPUChannels(self.earliest_time_gpu, self.channel_q_gpu, self.channel_history_gpu, self.ndaq,
                           self.stride)

    def _event_arrays(self, n):
        if self._event_rows is None or len(self._event_rows[0]) < n:
            self._event_rows = None          # release before growing
            self._event_rows = (ga.empty(n, np.uint32), ga.empty(n, np.uint32), ga.empty(n, np.uint32),
                                ga.empty(n, np.float32))
        return [a[:n] for a in self._event_rows]

    def _event_host_words(self, n):
        if self._event_host is None or self._event_host.numel() < n:
            self._event_host = None
            self._event_host = torch.empty(n, dtype=torch.int32, pin_memory=True)
        return self._event_host

    def acquire_events(self, gpuphotons, rng_states, bounds, nthreads_per_block=64, max_blocks=1024, weight=1.0):
        """begin_acquire / acquire / end_acquire (daq.py:56-101) for every event
        [bounds[e], bounds[e+1]) of `gpuphotons`, as sim.py:143-152 runs them one
        after another, in one native call whose launches do not depend on the
        number of events (chr_daq_acquire_events): the same channel words and
        the same rng_states afterwards, bit for bit.  Returns a GPUEventChannels
        of len(bounds) - 1 rows.  ndaq > 1 (run_daq_many) is not batched here:
        acquire_events_many is its counterpart."""
        if self.ndaq != 1:
            raise ValueError('acquire_events runs ndaq = 1 acquisitions only (this GPUDaq has ndaq = %d)' % self.ndaq)
        bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        if bounds.ndim != 1 or len(bounds) < 1:
            raise ValueError('bounds must be a 1-D array of nevents + 1 photon offsets')
        nevents = len(bounds) - 1
        t_int, q_int, hist, q = self._event_arrays(nevents * self.nchannels)
        if nevents == 0:
            return GPUEventChannels(t_int, q_int, hist, q, 0, self.nchannels, host=self._event_host_words)
        ph = gpuphotons._desc()
        _native.call('chr_daq_acquire_events', ctypes.byref(ph), len(gpuphotons.pos), bounds.ctypes.data, nevents,
                     rng_states.gpudata, len(rng_states), 0x1 << 2, self.solid_id_map_gpu.gpudata,
                     ctypes.byref(self._desc), t_int.gpudata, q_int.gpudata, hist.gpudata, q.gpudata,
                     ctypes.c_float(weight), int(nthreads_per_block), int(max_blocks), current_stream())
        return GPUEventChannels(t_int, q_int, hist, q, nevents, self.nchannels, host=self._event_host_words)

    def acquire_photoelectrons(self, gpuphotons, rng_states, bounds, nthreads_per_block=64, max_blocks=1024,
                               weight=1.0):
        """acquire_events that also keeps what it draws (chr_daq_acquire_events_pe):
        returns (GPUEventChannels, GPUPhotoelectrons).  The channel rows and the
        rng_states afterwards are bit for bit acquire_events' on the same inputs
        -- the same stream as acquire_events --; the second value holds, per
        photon of [bounds[0], bounds[-1]), the channel, time and quantised charge
        of the photoelectron it made (chroma.gpu.waveform).  The channel rows are
        views of arrays this GPUDaq reuses, as acquire_events'; the
        GPUPhotoelectrons owns its arrays."""
        from chroma.gpu.waveform import GPUPhotoelectrons
        if self.ndaq != 1:
            raise ValueError('acquire_photoelectrons runs ndaq = 1 acquisitions only (this GPUDaq has ndaq = %d)'
                             % self.ndaq)
        bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        if bounds.ndim != 1 or len(bounds) < 1:
            raise ValueError('bounds must be a 1-D array of nevents + 1 photon offsets')
        nevents = len(bounds) - 1
        span = int(bounds[-1] - bounds[0])
        if span < 0:
            raise ValueError('bounds decrease')
        t_int, q_int, hist, q = self._event_arrays(nevents * self.nchannels)
        # one spare word: an empty array has no address to hand over
        pe = [ga.empty(span + 1, d)[:span] for d in (np.int32, np.float32, np.uint32)]
        if nevents:
            ph = gpuphotons._desc()
            _native.call('chr_daq_acquire_events_pe', ctypes.byref(ph), len(gpuphotons.pos), bounds.ctypes.data,
                         nevents, rng_states.gpudata, len(rng_states), 0x1 << 2, self.solid_id_map_gpu.gpudata,
                         ctypes.byref(self._desc), t_int.gpudata, q_int.gpudata, hist.gpudata, q.gpudata,
                         pe[0].gpudata, pe[1].gpudata, pe[2].gpudata, ctypes.c_float(weight),
                         int(nthreads_per_block), int(max_blocks), current_stream())
        chans = GPUEventChannels(t_int, q_int, hist, q, nevents, self.nchannels, host=self._event_host_words)
        return chans, GPUPhotoelectrons(pe[0], pe[1], pe[2], bounds, self.nchannels, self.charge_unit, t_int.copy())

    def acquire_events_many(self, gpuphotons, rng_states, bounds, nthreads_per_block=64, max_blocks=1024, weight=1.0):
        """acquire_events for ndaq > 1 (run_daq_many, daq.py:62-91): begin_acquire
        / acquire / end_acquire for every event [bounds[e], bounds[e+1]) of
        `gpuphotons` in one native call (chr_daq_acquire_events_many), with the
        same channel words, rng_states and normal cache afterwards, bit for
        bit.  Returns GPUChannels of nevents * ndaq copies of nchannels words:
        event e's copy i is copy e*ndaq + i, so the rows of all events stack as
        one acquisition of that many copies (GPUPDF.accumulate_pdf_eval takes
        them as such).  t is the f32 view of the earliest-time words; q holds
        what end_acquire leaves (copy 0 of every event converted, the others 0).
        The arrays are views of arrays this GPUDaq reuses: valid until its next
        acquire_events_many or acquire_events."""
        if self.ndaq < 2:
            raise ValueError('acquire_events_many runs ndaq > 1 acquisitions only (acquire_events runs ndaq = 1)')
        bounds = np.ascontiguousarray(bounds, dtype=np.int64)
        if bounds.ndim != 1 or len(bounds) < 1:
            raise ValueError('bounds must be a 1-D array of nevents + 1 photon offsets')
        nevents = len(bounds) - 1
        t_int, q_int, hist, q = self._event_arrays(nevents * self.ndaq * self.nchannels)
        if nevents:
            ph = gpuphotons._desc()
            _native.call('chr_daq_acquire_events_many', ctypes.byref(ph), len(gpuphotons.pos), bounds.ctypes.data,
                         nevents, rng_states.gpudata, len(rng_states), rng_states.normal_cache.gpudata, 0x1 << 2,
                         self.solid_id_map_gpu.gpudata, ctypes.byref(self._desc), t_int.gpudata, q_int.gpudata,
                         hist.gpudata, q.gpudata, int(self.ndaq), ctypes.c_float(weight), int(nthreads_per_block),
                         int(max_blocks), current_stream())
        t = ga.from_tensor(t_int.tensor.view(torch.float32), np.float32)
        return GPUChannels(t, q, hist, nevents * self.ndaq, self.nchannels)
