"""Simulation driver (drop-in for reference chroma/sim.py:22-282).

Batches events (never splitting one), uploads photons, propagates them on the
device with the reference's launch shape (nthreads_per_block=512,
max_blocks=1024 -> 524,288 RNG slots) and splits the detected hits back into
events.  Photon tracking, GPU-resident inputs and the per-event DAQ
(run_daq=True, chroma.gpu.daq) are supported as in the reference; the DAQ of a
batch's events runs in groups of one native call each (Simulation.daq_events),
with the per-event loop's results; simulate(..., waveforms=WaveformSpec(...))
also fills every event's charge trains and ADC words (chroma.gpu.waveform).
"""
import os
import time
from types import SimpleNamespace

import numpy as np

from chroma import event
from chroma import gpu
from chroma.gensteps import Gensteps
from chroma.gpu import gpuarray as ga
from chroma.gpu.waveform import WaveformSpec, waveform_event_groups  # noqa: F401
from chroma.itertoolset import peek


def pick_seed():
    """A seed from the current time and process id."""
    return int(time.time()) ^ (os.getpid() << 16) & 2 ** 32 - 1


def agree_seed(seed, group=None):
    """Rank 0's seed on every rank of `group` (a sharded job draws one seed).  The
    value travels as a tensor on the backend's device: the rank's own GPU for
    RCCL (bound by the caller before this collective), the CPU for gloo."""
    import torch
    import torch.distributed as dist
    from chroma.gpu import shard
    if shard.dist_info(group)[1] <= 1:
        return seed
    on_gpu = torch.cuda.is_available() and dist.get_backend(group) != 'gloo'
    box = torch.tensor([seed], dtype=torch.int64,
                       device=torch.device('cuda', shard.local_device()) if on_gpu else 'cpu')
    dist.broadcast(box, src=0, group=group)
    return int(box.item())


def daq_event_groups(bounds, nchannels, budget):
    """The events of a batch (photon offsets `bounds`) in consecutive groups
    [first, last) for GPUDaq.acquire_events: as many events per group as fit
    `budget` bytes of channel rows (four 4-byte words per channel and event),
    at least one.  Every event is in exactly one group, in order."""
    nevents = len(bounds) - 1
    per_group = max(1, int(budget) // (16 * int(nchannels)))
    return [(first, min(first + per_group, nevents)) for first in range(0, nevents, per_group)]


def pdf_copy_groups(nreps, ndaq, nchannels, budget):
    """The nreps photon copies of one eval_pdf / create_pdf source in consecutive
    groups [first, last) for GPUDaq.acquire_events_many (acquire_events when
    ndaq = 1): as many copies per group as fit `budget` bytes of channel rows
    (four 4-byte words per channel, DAQ copy and photon copy), at least one.
    Every copy is in exactly one group, in order."""
    per_group = max(1, int(budget) // (16 * int(ndaq) * int(nchannels)))
    return [(first, min(first + per_group, int(nreps))) for first in range(0, int(nreps), per_group)]


def hit_map_batches(step_photons, photons_per_batch):
    """The steps of Simulation.hit_map (their photon counts `step_photons`, in
    order) in consecutive batches [first, last): a batch closes after the step
    that brings it to photons_per_batch photons or more, so steps are never
    split.  Every step is in exactly one batch; a last batch may stay below
    photons_per_batch (or hold no photon at all)."""
    counts = np.asarray(step_photons, dtype=np.uint64)
    need = max(1, int(photons_per_batch))
    batches, first, held = [], 0, 0
    for i, n in enumerate(counts.tolist()):
        held += n
        if held >= need:
            batches.append((first, i + 1))
            first, held = i + 1, 0
    if first < len(counts):
        batches.append((first, len(counts)))
    return batches


def _event_tracks_flat(flat, start, end):
    """(offsets, Photons) of the photons [start, end) of a batch's photon-major
    tracks (PhotonTracks.flat()): the event's own offsets, from 0."""
    offsets, photons = flat
    lo, hi = int(offsets[start]), int(offsets[end])
    return offsets[start:end + 1] - lo, photons[lo:hi]


def _track_list(offsets, photons):
    """One event.Photons per photon: the slices of `photons` between consecutive
    offsets (an empty Photons() for a photon that was never queued)."""
    return [photons[a:b] if b > a else event.Photons() for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]


class _Batch(object):
    """One batch of events on the device: its GPUPhotons (uploaded when the
    batch closes, before a later batch can restamp a shared source's evidx),
    the event bounds in the batch's photon range, and this process's part of
    that range ([lo, hi): everything for Simulation, a shard for
    ShardedSimulation)."""
    __slots__ = ('events', 'gpu_photons', 'bounds', 'lo', 'hi', 'tracking')

    def __init__(self, events, gpu_photons, bounds, lo, hi):
        self.events, self.gpu_photons, self.bounds, self.lo, self.hi = events, gpu_photons, bounds, lo, hi
        self.tracking = None


class Simulation(object):
    # batches propagated per chr_propagate_batches call by simulate(): batch k's
    # multi-step tail (its longest-lived photon's serial chain) runs on a second
    # HIP stream under batch k+1's first step; results are bit-identical to one
    # propagate per batch (tests/test_gpu_sim_pipeline.py).  1 = the reference's
    # one-batch-at-a-time loop (sim.py:116-160).
    pipeline_batches = 8
    # run_daq: the DAQ of a batch's events in groups of one native call each
    # (GPUDaq.acquire_events; channels and rng_states bit-identical to the
    # per-event loop, tests/test_gpu_daq_events.py).  False = the reference's
    # begin / acquire / end per event (sim.py:143-152).
    daq_events = True
    # bytes of channel rows (16 per channel and event) one group may hold on the
    # device; a cap on device and pinned host memory (a batch of one-photon
    # events on a large detector would otherwise ask for its product).  With
    # waveforms the train words count too (WaveformSpec.event_bytes).
    daq_group_bytes = 64 << 20
    # photon_tracking: build ev.photon_tracks, one event.Photons per photon (the
    # reference's list).  False leaves it None for callers who read only
    # ev.photon_tracks_flat = (offsets, Photons), the same records back to back.
    photon_track_lists = True
    # eval_pdf / create_pdf: the DAQ of a source's photon copies in groups of one native
    # call each (GPUDaq.acquire_events_many, or acquire_events for ndaq = 1; groups by
    # pdf_copy_groups under daq_group_bytes) and one accumulation over a group's stacked
    # rows; accumulators, rng_states and the normal cache bit-identical to the per-copy
    # loop (tests/test_gpu_pdf_eval.py).  False = that loop: begin / acquire / end /
    # accumulate per copy.
    pdf_rows = True
    # groups of fewer copies than this take the per-copy loop (DESIGN, "Event likelihoods")
    pdf_rows_min_group = 2

    def __init__(self, detector, seed=None, cuda_device=None, photon_tracking=False, nthreads_per_block=512,
                 max_blocks=1024):
        self.detector = detector
        self.nthreads_per_block = nthreads_per_block
        self.max_blocks = max_blocks
        self.photon_tracking = photon_tracking
        self.seed = pick_seed() if seed is None else seed
        np.random.seed(self.seed & 0xFFFFFFFF)
        self.context = gpu.create_cuda_context(cuda_device)
        if hasattr(detector, 'num_channels'):
            self.gpu_geometry = gpu.GPUDetector(detector)
            self.gpu_daq = gpu.GPUDaq(self.gpu_geometry) if self.gpu_geometry.nchannels > 0 else None
            self.gpu_pdf = gpu.GPUPDF()                # sim.py:45-46
            self.gpu_pdf_kernel = gpu.GPUKernelPDF()
        else:
            self.gpu_geometry = gpu.GPUGeometry(detector)
        self.rng_states = gpu.get_rng_states(self.nthreads_per_block * self.max_blocks, seed=self.seed)
        self.pdf_config = None
        self.last_pipeline = None     # (batches, propagate_batches calls) of the last simulate()

    def generate(self, gensteps):
        """The photons of a Gensteps, drawn on the device with rng_states
        (chroma.gpu.generate_photons); `last_exhausted` counts the Cherenkov
        photons whose rejection loop ran out."""
        made = gpu.generate_photons(gensteps, self.gpu_geometry, self.rng_states)
        self.last_exhausted = made.exhausted
        return made

    # ------------------------------------------------------------ batch stages
    def _upload(self, batch_events):
        """The batch's photons on the device (sim.py:54-70)."""
        sources = [ev.photons_beg for ev in batch_events]
        bounds = np.cumsum(np.concatenate([[0], [len(s) for s in sources]])).astype(np.int64)
        src = self._stack_gpu_photon_sources(sources)
        if src is None:
            src = event.Photons.join(sources)
        gpu_photons = gpu.GPUPhotons(src, copy_flags=True, copy_triangles=False, copy_weights=False)
        return _Batch(batch_events, gpu_photons, bounds, 0, int(bounds[-1]))

    def _propagate(self, batches, max_steps):
        """Propagate the batches in order with the one rng_states: one
        pipelined chr_propagate_batches call for several (chroma.gpu.propagate_batches),
        GPUPhotons.propagate for one or with photon tracking."""
        kw = dict(nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks, max_steps=max_steps)
        live = [b for b in batches if b.hi > b.lo]
        if len(live) > 1 and not self.photon_tracking:
            gpu.propagate_batches([b.gpu_photons for b in live], self.gpu_geometry, self.rng_states, **kw)
            return 1
        for b in live:
            if self.photon_tracking and b.gpu_photons.device_tracking:
                # the tracks stay on the device until _emit downloads them once, photon-major
                b.tracking = b.gpu_photons.propagate_tracks(self.gpu_geometry, self.rng_states, **kw)
            else:
                b.tracking = b.gpu_photons.propagate(self.gpu_geometry, self.rng_states, track=self.photon_tracking,
                                                     **kw)
        return 0

    def _batch_hits(self, b):
        return b.gpu_photons.get_flat_hits(self.gpu_geometry)

    def _photons_end(self, b):
        """The batch's photons after propagation, batch order (sim.py:72-75)."""
        return b.gpu_photons.get()

    def _acquire(self, b, start, end):
        """DAQ of one event (sim.py:143-152)."""
        self.gpu_daq.begin_acquire()
        self.gpu_daq.acquire(b.gpu_photons, self.rng_states, start_photon=int(start), nphotons=int(end - start),
                             nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks)
        return self.gpu_daq.end_acquire().get()

    def _acquire_events(self, b, bounds):
        """DAQ of the consecutive events [bounds[e], bounds[e+1]) of the batch in
        one call: their event.Channels in order, or None where the DAQ is not
        batched (the caller then runs _acquire per event)."""
        return self.gpu_daq.acquire_events(b.gpu_photons, self.rng_states, bounds,
                                           nthreads_per_block=self.nthreads_per_block,
                                           max_blocks=self.max_blocks).get()

    def _acquire_waveforms(self, b, bounds, spec):
        """DAQ of the consecutive events [bounds[e], bounds[e+1]) of the batch with
        their photoelectrons kept (GPUDaq.acquire_photoelectrons: the channels
        and rng_states of _acquire_events): per event its event.Channels, its
        event.Waveforms by `spec`, and its event.Photoelectrons or None."""
        chans, pe = self.gpu_daq.acquire_photoelectrons(b.gpu_photons, self.rng_states, bounds,
                                                        nthreads_per_block=self.nthreads_per_block,
                                                        max_blocks=self.max_blocks)
        wf = pe.trains(spec.trange, spec.nsamples, rows=spec.rows)
        if spec.template is not None:
            wf.digitise(spec.template, spec.scale, spec.pedestal, spec.adc_bits)
        kept = pe.get() if spec.keep_photoelectrons else [None] * len(pe)
        return chans.get(), wf.get(), kept

    def _emit(self, b, keep_photons_beg=False, keep_photons_end=False, keep_hits=True, keep_flat_hits=True,
              run_daq=False, waveforms=None):
        """Split a propagated batch back into its events (sim.py:72-110).

        With run_daq and daq_events the DAQ runs for a group of events at a time
        (daq_event_groups under daq_group_bytes), each group just before its
        first event is yielded, so its draws fall between the same propagates
        as the per-event loop's.  A caller who abandons the generator inside a
        batch leaves rng_states advanced to the end of the current group, not
        of the current event.

        With `waveforms` (a WaveformSpec) every group, one of a single event
        too, runs through _acquire_waveforms, in the groups of
        waveform_event_groups (the train words count against daq_group_bytes):
        ev.channels and rng_states are what the run without it gives, and
        ev.waveforms (ev.photoelectrons) are filled."""
        if keep_photons_end:
            photons_end = self._photons_end(b)
        has_channels = hasattr(self.detector, 'num_channels')
        batch_hits = None
        if has_channels and (keep_hits or keep_flat_hits):
            batch_hits = self._batch_hits(b)
        run_daq = run_daq and getattr(self, 'gpu_daq', None) is not None
        groups = {}
        if run_daq and waveforms is not None:
            groups = dict(waveform_event_groups(b.bounds, self.gpu_daq.nchannels, self.daq_group_bytes, waveforms))
        elif run_daq and self.daq_events:
            groups = dict(daq_event_groups(b.bounds, self.gpu_daq.nchannels, self.daq_group_bytes))
        group_first, group_channels, group_waveforms = 0, None, None
        flat = None
        if self.photon_tracking and isinstance(b.tracking, gpu.PhotonTracks):
            flat = b.tracking.flat()      # one download of the batch's records, photon-major
            b.tracking.close()
        for i, (ev, (start, end)) in enumerate(zip(b.events, zip(b.bounds[:-1], b.bounds[1:]))):
            if not keep_photons_beg:
                ev.photons_beg = None
            if flat is not None:
                ev.photon_tracks_flat = _event_tracks_flat(flat, int(start), int(end))
                if self.photon_track_lists:
                    ev.photon_tracks = _track_list(*ev.photon_tracks_flat)
            elif self.photon_tracking:
                step_ids, step_photons = b.tracking
                tracks = [[] for _ in range(end - start)]
                for ids, photons in zip(step_ids, step_photons):
                    mask = (ids >= start) & (ids < end)
                    if not mask.any():
                        break
                    sel = photons[mask]
                    for k, pid in enumerate(ids[mask] - start):
                        tracks[pid].append(sel[k])
                ev.photon_tracks = [event.Photons.join(t, concatenate=False) if t else event.Photons()
                                    for t in tracks]
            if keep_photons_end:
                ev.photons_end = photons_end[start:end] if photons_end is not None else None
            if batch_hits is not None:
                ev_hits = batch_hits[batch_hits.evidx == i]
                if keep_hits:
                    ev.hits = {int(ch): ev_hits[ev_hits.channel == ch] for ch in np.unique(ev_hits.channel)}
                if keep_flat_hits:
                    ev.flat_hits = ev_hits
            if run_daq and waveforms is not None:
                if i in groups:
                    group_first = i
                    group_waveforms = self._acquire_waveforms(b, b.bounds[i:groups[i] + 1], waveforms)
                ev.channels, ev.waveforms, ev.photoelectrons = (part[i - group_first] for part in group_waveforms)
                for part in group_waveforms:
                    part[i - group_first] = None
            elif run_daq:
                if i in groups:
                    group_first, group_channels = i, None
                    if groups[i] - i > 1:           # one event alone is quicker through _acquire (DESIGN)
                        group_channels = self._acquire_events(b, b.bounds[i:groups[i] + 1])
                        if group_channels is None:  # not batched: per event from here on
                            groups = {}
                if group_channels is not None:
                    ev.channels = group_channels[i - group_first]
                    group_channels[i - group_first] = None
                else:
                    ev.channels = self._acquire(b, start, end)
            yield ev

    def _simulate_batch(self, batch_events, keep_photons_beg=False, keep_photons_end=False, keep_hits=True,
                        keep_flat_hits=True, run_daq=False, max_steps=100, verbose=False):
        """One batch, as the reference's _simulate_batch (sim.py:54-110)."""
        t0 = time.time()
        b = self._upload(batch_events)
        self._propagate([b], max_steps)
        if verbose:
            print('Batch took %0.2f s' % (time.time() - t0))
        yield from self._emit(b, keep_photons_beg=keep_photons_beg, keep_photons_end=keep_photons_end,
                              keep_hits=keep_hits, keep_flat_hits=keep_flat_hits, run_daq=run_daq)

    @staticmethod
    def _is_gpu_photon_source(photons):
        return all(isinstance(getattr(photons, f, None), ga.GPUArray)
                   for f in ('pos', 'dir', 'pol', 'wavelengths', 't', 'evidx', 'flags'))

    @classmethod
    def _stack_gpu_photon_sources(cls, sources):
        """Join GPU-resident inputs on the device (sim.py:171-223)."""
        if not sources or not all(cls._is_gpu_photon_source(s) for s in sources):
            return None
        total = sum(len(s) for s in sources)
        fields = ('pos', 'dir', 'pol', 'wavelengths', 't', 'evidx', 'flags')
        out = {}
        for f in fields:
            dest = ga.empty(total, getattr(sources[0], f).dtype)
            off = 0
            for s in sources:
                n = len(s)
                if n:
                    dest[off:off + n].tensor.copy_(getattr(s, f)[:n].tensor)
                    off += n
            out[f] = dest
        out['true_nphotons'] = total
        return SimpleNamespace(**out)

    def _pipeline_depth(self, run_daq):
        """Batches per propagate call: 1 where the reference's interleaving is
        observable -- the DAQ draws from rng_states between two batches'
        propagates, photon tracking downloads every step."""
        if run_daq or self.photon_tracking:
            return 1
        return max(1, int(self.pipeline_batches))

    def simulate(self, iterable, keep_photons_beg=False, keep_photons_end=False, keep_hits=True,
                 keep_flat_hits=True, run_daq=False, max_steps=1000, photons_per_batch=1000000, waveforms=None):
        """sim.py:112-160.  Events are batched as the reference batches them
        (never split, a batch closes once it holds photons_per_batch photons)
        and yielded in order; up to pipeline_batches closed batches are
        propagated in one pipelined call (read ahead from the iterable), with
        results bit-identical to the reference's one-batch-at-a-time loop.

        waveforms: a WaveformSpec (with run_daq) also fills ev.waveforms -- the
        charge trains of the event's photoelectrons per read-out row and, with a
        template, their ADC words -- and ev.photoelectrons when the spec keeps
        them.  The DAQ draws what it draws without it (the same stream as
        acquire_events): ev.channels and rng_states do not change, bit for bit."""
        if waveforms is not None:
            if not isinstance(waveforms, WaveformSpec):
                raise TypeError('waveforms must be a WaveformSpec')
            if not run_daq:
                raise ValueError('waveforms need run_daq=True')
            self._check_waveforms()
        return self._simulate_events(iterable, keep_photons_beg, keep_photons_end, keep_hits, keep_flat_hits, run_daq,
                                     max_steps, photons_per_batch, waveforms)

    def _simulate_events(self, iterable, keep_photons_beg, keep_photons_end, keep_hits, keep_flat_hits, run_daq,
                         max_steps, photons_per_batch, waveforms):
        """simulate's generator (simulate itself refuses bad arguments when it is called)."""
        if isinstance(iterable, (event.Photons, Gensteps)):
            first, iterable = iterable, [iterable]
        else:
            first, iterable = peek(iterable)
        if isinstance(first, Gensteps):
            # one event per Gensteps: its photons are drawn on the device with this
            # simulation's rng_states, in input order as the events are read (a pipelined
            # run reads ahead, so every batch of a propagate call is generated before it),
            # and enter as a GPU-resident source (_stack_gpu_photon_sources)
            iterable = (event.Event(photons_beg=self.generate(x)) for x in iterable)
        elif isinstance(first, event.Photons):
            iterable = (event.Event(photons_beg=x) for x in iterable)
        elif isinstance(first, event.Vertex):
            raise NotImplementedError('Vertex input not supported in Chroma')
        emit_kw = dict(keep_photons_beg=keep_photons_beg, keep_photons_end=keep_photons_end, keep_hits=keep_hits,
                       keep_flat_hits=keep_flat_hits, run_daq=run_daq, waveforms=waveforms)
        depth = self._pipeline_depth(run_daq)
        stats = [0, 0]
        pending = []

        def flush():
            stats[0] += len(pending)
            stats[1] += self._propagate(pending, max_steps)
            for b in pending:
                yield from self._emit(b, **emit_kw)
            del pending[:]

        nphotons = 0
        batch = []
        for ev in iterable:
            ev.nphotons = len(ev.photons_beg)
            idx = len(batch)
            evidx = getattr(ev.photons_beg, 'evidx', None)
            if evidx is not None:
                if isinstance(evidx, ga.GPUArray):
                    if ev.nphotons > 0:
                        evidx[:ev.nphotons].fill(np.uint32(idx))
                else:
                    evidx[:ev.nphotons] = np.uint32(idx)
            nphotons += ev.nphotons
            batch.append(ev)
            if nphotons >= photons_per_batch:
                pending.append(self._upload(batch))
                nphotons, batch = 0, []
                if len(pending) >= depth:
                    yield from flush()
        if batch:
            pending.append(self._upload(batch))
        if pending:
            yield from flush()
        self.last_pipeline = tuple(stats)

    def _check_waveforms(self):
        if getattr(self, 'gpu_daq', None) is None:
            raise ValueError('waveforms need a detector with channels')

    def hit_map(self, gensteps, nsources, tbins=0, trange=None, earliest=True, weights=False, max_steps=1000,
                photons_per_batch=1000000, use_weights=False):
        """The hit map (chroma.gpu.hitmap.HitMap) of the photons of `gensteps`, a
        Gensteps or an iterable of them: per source and channel the detected
        photons, the earliest arrival, the arrival-time histogram (tbins bins
        over trange) and the weight sum.  A step's `evidx` is the caller's
        absolute source id (0 .. nsources-1; photons of other ids are counted
        in `skipped`) and is not restamped.  No Event is built and no photon
        or hit leaves the device: the only downloads are the map and
        `last_exhausted` (the generator's count, summed over the batches).

        The call sequence, on which the RNG stream depends:
          records = the steps of all the Gensteps, in order;
          batches = hit_map_batches(records['nphotons'], photons_per_batch),
                    those without photons dropped;
          for each group of up to `pipeline_batches` consecutive batches:
              made = [chroma.gpu.generate_photons(records[a:b], gpu_geometry, rng_states)
                      for (a, b) in group]                          # in order
              chroma.gpu.propagate_batches(made, gpu_geometry, rng_states, nthreads_per_block,
                                           max_blocks, max_steps, use_weights)
              GPUHitMap.accumulate(m) for m in made                 # draws nothing
        """
        return self._hit_map_device(gensteps, nsources, tbins, trange, earliest, weights, max_steps,
                                    photons_per_batch, use_weights).get()

    def _hit_map_device(self, gensteps, nsources, tbins, trange, earliest, weights, max_steps, photons_per_batch,
                        use_weights):
        """hit_map's work; the GPUHitMap itself, nothing downloaded but `last_exhausted`."""
        if not hasattr(self.detector, 'num_channels') or self.gpu_geometry.nchannels <= 0:
            raise ValueError('hit_map needs a detector with channels')
        from chroma import gensteps as gs
        parts = [gensteps] if isinstance(gensteps, Gensteps) else list(gensteps)
        material_objects = getattr(getattr(self.gpu_geometry, 'packed', None), 'material_objects', None)
        records = [gs._as_records(p, material_objects) for p in parts]
        records = np.concatenate(records) if records else np.zeros(0, gs.GENSTEP_DTYPE)
        hm = gpu.GPUHitMap(self.gpu_geometry, nsources, tbins=tbins, trange=trange, earliest=earliest,
                           weights=weights)
        cum = np.concatenate([[0], np.cumsum(records['nphotons'].astype(np.uint64))])
        batches = [(a, b) for a, b in hit_map_batches(records['nphotons'], photons_per_batch) if cum[b] > cum[a]]
        depth = max(1, int(self.pipeline_batches))
        self.last_exhausted = 0
        calls = 0
        for first in range(0, len(batches), depth):
            made = [gpu.generate_photons(records[a:b], self.gpu_geometry, self.rng_states)
                    for a, b in batches[first:first + depth]]
            self.last_exhausted += sum(m.exhausted for m in made)
            gpu.propagate_batches(made, self.gpu_geometry, self.rng_states,
                                  nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks,
                                  max_steps=max_steps, use_weights=use_weights)
            calls += 1
            for m in made:
                hm.accumulate(m)
        self.last_pipeline = (len(batches), calls)
        return hm

    # ------------------------------------------------------------ photon library
    def build_library(self, grid, material, photons_per_voxel, tbins=0, trange=None, earliest=True,
                      wavelength_range=(380.0, 500.0), max_steps=1000, photons_per_batch=1000000, use_weights=False):
        """A chroma.gpu.GPUPhotonLibrary of `grid` (chroma.library.VoxelGrid): the
        hit map of grid.flashes(material, photons_per_voxel, wavelength_range) --
        one isotropic flash at every voxel centre, source id = voxel id --, kept
        on the device (nothing of it is downloaded) and carrying the grid.  The
        call sequence, on which the RNG stream depends, is hit_map's for those
        flashes."""
        hm = self._hit_map_device(grid.flashes(material, photons_per_voxel, wavelength_range), grid.nvoxels, tbins,
                                  trange, earliest, False, max_steps, photons_per_batch, use_weights)
        return gpu.GPUPhotonLibrary(hm, grid=grid)

    def simulate_library(self, library, iterable, sample=True):
        """One event.Event per Gensteps of `iterable` with `channels` filled from a
        GPUPhotonLibrary instead of a propagation: sampled (hit = n > 0, q = n, t
        drawn from the library's time histogram or its earliest time), or with
        sample=False the expected values (q = mu, hit = mu > 0, t = tfirst).  The
        library needs its grid.  ev.nphotons is the photons the steps name; no
        photon is made.

        The call sequence, on which the RNG stream depends:
          parts = list(iterable);
          groups = consecutive runs of max(1, daq_group_bytes // (8 * nchannels)) parts;
          for each group, just before its first event is yielded:
              entries = chroma.library.entries_from_gensteps(library.grid, group)
              sample:     library.sample(entries, rng_states).get()   # chr_library_sample, all slots
              otherwise:  chroma.gpu.library.expected_channels(library.expect(entries).get())   # draws nothing
        """
        from chroma.gpu.library import expected_channels
        from chroma.library import entries_from_gensteps
        if library.grid is None:
            raise ValueError('simulate_library needs a library that carries its grid')
        parts = [iterable] if isinstance(iterable, Gensteps) else list(iterable)
        per_group = max(1, int(self.daq_group_bytes) // (8 * int(library.nchannels)))
        for first in range(0, len(parts), per_group):
            group = parts[first:first + per_group]
            entries = entries_from_gensteps(library.grid, group)
            if sample:
                channels = library.sample(entries, self.rng_states).get()
            else:
                channels = expected_channels(library.expect(entries).get())
            for g, ch in zip(group, channels):
                ev = event.Event(channels=ch)
                ev.nphotons = g.nphotons
                yield ev

    # ------------------------------------------------------------ likelihood support
    def _pdf_sources(self, iterable):
        """The photon sources of eval_pdf / create_pdf / setup_kernel / eval_kernel,
        in order: event.Photons as they are, an event.Event's photons_beg, the
        photons of a Gensteps drawn with self.generate (as simulate does)."""
        if isinstance(iterable, (event.Photons, event.Event, Gensteps)):
            iterable = [iterable]
        for x in iterable:
            if isinstance(x, event.Vertex):
                raise NotImplementedError('Vertex input not supported in Chroma')
            if isinstance(x, Gensteps):
                yield self.generate(x)
            elif isinstance(x, event.Event):
                yield x.photons_beg
            else:
                yield x

    def _pdf_daq(self, ndaq):
        """The GPUDaq of `ndaq` copies (kept: its arrays are reused from call to call)."""
        if not hasattr(self.detector, 'num_channels') or self.gpu_geometry.nchannels <= 0:
            raise ValueError('the likelihood methods need a detector with channels')
        ndaq = int(ndaq)
        if ndaq < 1:
            raise ValueError('ndaq must be at least 1')
        if ndaq == 1:
            return self.gpu_daq
        daqs = self.__dict__.setdefault('_pdf_daqs', {})
        if ndaq not in daqs:
            daqs[ndaq] = gpu.GPUDaq(self.gpu_geometry, ndaq)
        return daqs[ndaq]

    def _pdf_copies(self, iterable, nreps, max_steps, use_weights=False):
        """Per source: (GPUPhotons of nreps propagated copies, photons per copy)."""
        for source in self._pdf_sources(iterable):
            gp = gpu.GPUPhotons(source, ncopies=nreps)
            n = len(gp.pos) // nreps
            gp.propagate(self.gpu_geometry, self.rng_states, nthreads_per_block=self.nthreads_per_block,
                         max_blocks=self.max_blocks, max_steps=max_steps, use_weights=use_weights)
            yield gp, n

    def _acquire_copy(self, daq, gp, c, n):
        """begin / acquire / end for copy c of gp's n-photon copies."""
        daq.begin_acquire()
        daq.acquire(gp, self.rng_states, nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks,
                    start_photon=c * n, nphotons=n)
        return daq.end_acquire()

    def _acquire_copy_rows(self, daq, gp, n, nreps, accumulate, accumulate_rows):
        """The DAQ of all nreps copies of gp, copy by copy (pdf_rows False, and
        groups below pdf_rows_min_group) or a group per native call, each
        acquisition handed to accumulate / each group's stacked rows to
        accumulate_rows.  No row is downloaded."""
        kw = dict(nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks)
        if not self.pdf_rows:
            groups = [(0, nreps)]
        else:
            groups = pdf_copy_groups(nreps, daq.ndaq, daq.nchannels, self.daq_group_bytes)
        for first, last in groups:
            if not self.pdf_rows or last - first < self.pdf_rows_min_group:
                for c in range(first, last):
                    accumulate(self._acquire_copy(daq, gp, c, n))
                continue
            bounds = np.arange(first, last + 1, dtype=np.int64) * n
            if daq.ndaq == 1:
                rows = daq.acquire_events(gp, self.rng_states, bounds, **kw).as_channels()
            else:
                rows = daq.acquire_events_many(gp, self.rng_states, bounds, **kw)
            accumulate_rows(rows)

    def eval_pdf(self, event_channels, iterable, min_twidth, trange, min_qwidth, qrange, min_bin_content=100,
                 nreps=1, ndaq=1, time_only=True, max_steps=100, use_weights=False):
        """The adaptive-bin PDF of `iterable`'s sources (event.Photons, Events with
        photons_beg, or Gensteps) evaluated at the observed event_channels:
        (hitcount, pdf_value, pdf_uncert) per channel (GPUPDF.get_pdf_eval).
        Every source is propagated nreps times and every propagated copy read
        out by ndaq DAQ copies, so a channel's hitcount is out of
        nsources * nreps * ndaq.

        The call sequence, on which the RNG stream depends:
          gpu_pdf.setup_pdf_eval(hit, t, q, min_twidth, trange, min_qwidth, qrange, min_bin_content,
                                 time_only); gpu_pdf.clear_pdf_eval()
          daq = GPUDaq(gpu_geometry, ndaq)                       # kept per ndaq
          for each source, n photons:
              gp = GPUPhotons(source, ncopies=nreps)
              gp.propagate(gpu_geometry, rng_states, nthreads_per_block, max_blocks,
                           max_steps=max_steps, use_weights=use_weights)
              for c in range(nreps):
                  daq.begin_acquire()
                  daq.acquire(gp, rng_states, nthreads_per_block, max_blocks, start_photon=c*n, nphotons=n)
                  gpu_pdf.accumulate_pdf_eval(daq.end_acquire())
          return gpu_pdf.get_pdf_eval()
        With pdf_rows the copies of a source are taken in the groups of
        pdf_copy_groups(nreps, ndaq, nchannels, daq_group_bytes): one
        GPUDaq.acquire_events_many (acquire_events for ndaq = 1) and one
        accumulate_pdf_eval over the group's stacked rows per group, with the
        same accumulator words, rng_states and normal cache."""
        daq = self._pdf_daq(ndaq)
        pdf = self.gpu_pdf
        pdf.setup_pdf_eval(event_channels.hit, event_channels.t, event_channels.q, min_twidth, trange, min_qwidth,
                           qrange, min_bin_content=min_bin_content, time_only=time_only)
        pdf.clear_pdf_eval()
        for gp, n in self._pdf_copies(iterable, nreps, max_steps, use_weights):
            self._acquire_copy_rows(daq, gp, n, nreps, pdf.accumulate_pdf_eval, pdf.accumulate_pdf_eval)
        return pdf.get_pdf_eval()

    def create_pdf(self, iterable, tbins, trange, qbins, qrange, nreps=1, max_steps=100):
        """The [channel, time bin, charge bin] histogram of `iterable`'s sources,
        every source propagated nreps times and every copy read out by one
        DAQ: (hitcount, pdf) (GPUPDF.get_pdfs).  eval_pdf's sequence with ndaq =
        1 and gpu_pdf.add_hits_to_pdf in place of the accumulation (with
        pdf_rows: acquire_events and add_rows_to_pdf per group).  A call with
        the configuration of the one before adds to its histogram; a changed
        configuration starts a new one."""
        daq = self._pdf_daq(1)
        config = (int(tbins), tuple(float(x) for x in trange), int(qbins), tuple(float(x) for x in qrange))
        pdf = self.gpu_pdf
        if self.pdf_config != config:
            self.pdf_config = config
            pdf.setup_pdf(self.gpu_geometry.nchannels, tbins, trange, qbins, qrange)
        for gp, n in self._pdf_copies(iterable, nreps, max_steps):
            self._acquire_copy_rows(daq, gp, n, nreps, pdf.add_hits_to_pdf, pdf.add_rows_to_pdf)
        return pdf.get_pdfs()

    def _kernel_acquisitions(self, iterable, nreps, ndaq, accumulate):
        """Per source and propagated copy, ndaq acquisitions of one DAQ copy each
        through self.gpu_daq, each handed to `accumulate`.  Not batched: the
        kernel estimator's float sums depend on the order of the acquisitions."""
        daq = self._pdf_daq(1)
        for gp, n in self._pdf_copies(iterable, nreps, 100):
            for c in range(nreps):
                for _ in range(int(ndaq)):
                    accumulate(self._acquire_copy(daq, gp, c, n))

    def setup_kernel(self, event_channels, bandwidth_iterable, trange, qrange, nreps=1, ndaq=1, time_only=True,
                     scale_factor=1.0):
        """Choose the kernel estimator's per-channel bandwidths from the moments of
        the sources of bandwidth_iterable (GPUKernelPDF.setup_moments /
        accumulate_moments / compute_bandwidth) and set the observed event
        (GPUKernelPDF.setup_kernel) for eval_kernel."""
        kpdf = self.gpu_pdf_kernel
        kpdf.setup_moments(self.gpu_geometry.nchannels, trange, qrange, time_only=time_only)
        self._kernel_acquisitions(bandwidth_iterable, nreps, ndaq, kpdf.accumulate_moments)
        kpdf.compute_bandwidth(event_channels.hit, event_channels.t, event_channels.q, scale_factor=scale_factor)
        kpdf.setup_kernel(event_channels.hit, event_channels.t, event_channels.q)

    def eval_kernel(self, event_channels, kernel_iterable, trange, qrange, nreps=1, ndaq=1, time_only=True):
        """The kernel estimate of the PDF at the event given to setup_kernel, from
        the sources of kernel_iterable: (hitcount, pdf_value, pdf_uncert)
        (GPUKernelPDF.get_kernel_eval).  trange, qrange and time_only are
        setup_kernel's (the estimator keeps them)."""
        kpdf = self.gpu_pdf_kernel
        kpdf.clear_kernel()
        self._kernel_acquisitions(kernel_iterable, nreps, ndaq, kpdf.accumulate_kernel)
        return kpdf.get_kernel_eval()

    def __del__(self):
        ctx = getattr(self, 'context', None)
        if ctx is not None:
            try:
                ctx.pop()
            except Exception:
                pass


class ShardedSimulation(Simulation):
    """Simulation across the ranks of a torch.distributed job, one process per
    GPU (launch with torchrun; backend "nccl" = RCCL).  Every rank must call
    simulate() with the same events; each propagates its contiguous share of
    every batch on its own GPU (geometry replicated; a rank's batches are
    pipelined as Simulation's), then the detected hits are gathered in global
    photon order -- to rank 0 only (hits='root', the default: other ranks'
    events carry hits/flat_hits None) or to every rank (hits='all') -- and the
    per-event DAQ channels are reduced on every rank (chroma.gpu.shard).  The
    events equal a single-GPU run's except for the RNG streams of ranks > 0
    (rank r draws from curand subsequences r*S .. r*S+S-1).  keep_photons_end
    gathers the end photons the same way as the hits (to rank 0, or to every
    rank with hits='all'; None elsewhere).  photon_tracking is not sharded (use
    Simulation)."""

    def __init__(self, detector, seed=None, group=None, nthreads_per_block=512, max_blocks=1024, hits='root'):
        import torch
        from chroma.gpu import shard
        if hits not in ('root', 'all'):
            raise ValueError("hits must be 'root' or 'all'")
        self.hits_to = hits
        self.group = group
        self.rank, self.world = shard.dist_info(group)
        # bind this rank's GPU before any collective: RCCL stages on the current
        # device, which is cuda:0 on every rank unless set (all ranks would collide)
        if torch.cuda.is_available():
            torch.cuda.set_device(shard.local_device())
        if seed is None:
            seed = agree_seed(pick_seed(), group)
        Simulation.__init__(self, detector, seed=seed, cuda_device=shard.local_device(),
                            nthreads_per_block=nthreads_per_block, max_blocks=max_blocks)
        nslots = self.nthreads_per_block * self.max_blocks
        if self.rank:
            self.rng_states = gpu.get_rng_states(nslots, seed=self.seed, first_subsequence=self.rank * nslots)
        self._torch = torch

    def generate(self, gensteps):
        # every rank must see the same photons of an event, and the ranks' rng_states are
        # different streams: generate with Simulation (or chroma.gpu.generate_photons from
        # states seeded alike on every rank) and pass the photons
        raise NotImplementedError('Gensteps input is not sharded: generate the photons first')

    def _check_waveforms(self):
        # a channel's photoelectrons are spread over the ranks' shares of an event
        raise NotImplementedError('waveforms are not sharded: use Simulation')

    def hit_map(self, *args, **kwargs):
        # the map of a rank's photons would have to be reduced over the ranks (SUM; MIN for tmin)
        raise NotImplementedError('hit_map is not sharded: use Simulation')

    def build_library(self, *args, **kwargs):
        raise NotImplementedError('build_library is not sharded: use Simulation')

    def simulate_library(self, *args, **kwargs):
        # every rank would draw the same channels from a different stream
        raise NotImplementedError('simulate_library is not sharded: use Simulation')

    # the accumulators of a rank's photons would have to be reduced over the ranks before they are read
    def eval_pdf(self, *args, **kwargs):
        raise NotImplementedError('eval_pdf is not sharded: use Simulation')

    def create_pdf(self, *args, **kwargs):
        raise NotImplementedError('create_pdf is not sharded: use Simulation')

    def setup_kernel(self, *args, **kwargs):
        raise NotImplementedError('setup_kernel is not sharded: use Simulation')

    def eval_kernel(self, *args, **kwargs):
        raise NotImplementedError('eval_kernel is not sharded: use Simulation')

    def _upload(self, batch_events):
        from chroma.gpu import shard
        sources = [ev.photons_beg for ev in batch_events]
        bounds = np.cumsum(np.concatenate([[0], [len(s) for s in sources]])).astype(np.int64)
        lo, hi = shard.shard_range(int(bounds[-1]), self.rank, self.world)
        src = self._stack_gpu_photon_sources(sources)
        if src is None:
            local = event.Photons.join(sources)[lo:hi]
        else:
            local = SimpleNamespace(**{f: getattr(src, f)[lo:hi] for f in
                                       ('pos', 'dir', 'pol', 'wavelengths', 't', 'evidx', 'flags')})
            local.true_nphotons = hi - lo
        gpu_photons = gpu.GPUPhotons(local, copy_flags=True, copy_triangles=False, copy_weights=False)
        return _Batch(batch_events, gpu_photons, bounds, lo, hi)

    def _batch_hits(self, b):
        from chroma.gpu import shard
        fields, channels = b.gpu_photons.flat_hits_device(self.gpu_geometry)
        rows = shard.pack_hits(fields, channels)
        if self.hits_to == 'all':
            return shard.unpack_hits(shard.allgather_rows(rows, self.group))
        rows = shard.gather_rows(rows, 0, self.group)
        return shard.unpack_hits(rows) if rows is not None else None

    def _photons_end(self, b):
        """Every rank's shard of the batch's end photons, concatenated in rank
        (= global photon) order on rank 0 (hits='root'; None on the others) or on
        every rank (hits='all')."""
        from chroma.gpu import shard
        rows = shard.pack_photons(b.gpu_photons)
        if self.hits_to == 'all':
            return shard.unpack_photons(shard.allgather_rows(rows, self.group))
        rows = shard.gather_rows(rows, 0, self.group)
        return shard.unpack_photons(rows) if rows is not None else None

    def _acquire_events(self, b, bounds):
        return None     # not batched: every event's channels are reduced across the ranks (_acquire)

    def _acquire(self, b, start, end):
        from chroma.gpu import shard
        daq = self.gpu_daq
        daq.begin_acquire()
        a, c = max(int(start), b.lo), min(int(end), b.hi)     # this rank's part of the event
        if c > a:
            daq.acquire(b.gpu_photons, self.rng_states, start_photon=a - b.lo, nphotons=c - a,
                        nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks)
        t, q, h = shard.reduce_channels(daq.earliest_time_int_gpu.tensor, daq.channel_q_int_gpu.tensor,
                                        daq.channel_history_gpu.tensor, self.group)
        daq.earliest_time_int_gpu.tensor.copy_(t)
        daq.channel_q_int_gpu.tensor.copy_(q)
        daq.channel_history_gpu.tensor.copy_(h)
        return daq.end_acquire().get()
