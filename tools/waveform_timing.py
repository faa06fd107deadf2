#!/usr/bin/env python3
"""Dev tool (GPU box): time the photoelectron read-out of one propagated batch
against the plain batched DAQ and against what a user had to do before it.

E events of P isotropic photons each (default 100 x 10,000: the shape of DESIGN
section 17) are propagated once on the chosen detector (bench.py's detectors
and geometry cache: demo = 10,055 PMTs) with the simulation's 524,288 RNG slots.
Then, in the same process, each after a warm-up, `repeats` times (median, min,
max; HIP events around the calls on the device, the host clock where host work
is part of the step):

  acquire_events          GPUDaq.acquire_events, one call for all events (unchanged by
                          the photoelectron variant: re-measured here as its baseline)
  acquire_photoelectrons  the same draws with the three record arrays kept
  native_*                the two native calls alone, into arrays made once (no allocation,
                          no copy of the time words)
  trains_hit, trains_all  GPUPhotoelectrons.trains at S samples (default 256), a row per
                          hit channel / per channel (the row map's torch plumbing and
                          the allocation of the rows included)
  digitise_hit, _all      GPUWaveforms.digitise with T taps (default 32)
  device_chain            wall: acquire_photoelectrons + trains('hit') + digitise, and
                          the download of the trains and ADC words
  host_route              wall: get_flat_hits (selection on the device, download) and a
                          numpy np.add.at binning of the hits' times over the same
                          window -- without any smearing, which favours it

and two ratios: acquire_photoelectrons / acquire_events (device medians) and
device_chain / host_route (wall medians).  Prints one JSON line per case.

usage: tools/waveform_timing.py [--detector demo] [--events 100] [--photons-per-event 10000]
                                [--samples 256] [--taps 32] [--repeats 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))
sys.path.insert(0, ROOT)


def summary(ms):
    ms = np.asarray(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4),
                max_ms=round(float(ms.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--detector', default='demo', choices=('demo', '29k', 'small'))
    ap.add_argument('--events', type=int, default=100)
    ap.add_argument('--photons-per-event', type=int, default=10000)
    ap.add_argument('--samples', type=int, default=256)
    ap.add_argument('--taps', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=20)
    args = ap.parse_args()
    import torch
    import bench
    from chroma import event
    from chroma.gpu.hitmap import bin_scale
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation
    assert torch.cuda.is_available(), 'waveform_timing needs a HIP device'
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    det = bench.build_geometry(args.detector, bench.default_cache_dir())
    sim = Simulation(det, seed=1)
    daq, nch = sim.gpu_daq, sim.gpu_daq.nchannels
    nevents, per = args.events, args.photons_per_event
    events = []
    for e in range(nevents):
        ph = isotropic(per, seed=1 + e)
        ph.evidx[:] = e
        events.append(event.Event(photons_beg=ph))
    b = sim._upload(events)
    sim._propagate([b], 100)
    torch.cuda.synchronize()
    gp, bounds = b.gpu_photons, b.bounds
    kw = dict(nthreads_per_block=sim.nthreads_per_block, max_blocks=sim.max_blocks)
    # the window: the detected photons' times, the DAQ's smearing on both sides
    times = gp.t.get()[(gp.flags.get() & 4) != 0]
    trange = (float(np.floor(times.min())) - 8.0, float(np.ceil(np.percentile(times, 99))) + 8.0)
    taps = np.exp(-np.arange(args.taps) / 4.0).astype(np.float32)
    scale = np.float32(daq.charge_unit * 200.0)
    print(json.dumps(dict(case='setup', detector=args.detector, nchannels=nch, events=nevents, photons_per_event=per,
                          detected=int(len(times)), samples=args.samples, taps=args.taps, trange=trange,
                          rng_slots=len(sim.rng_states), setup_s=round(time.perf_counter() - t0, 1),
                          device=torch.cuda.get_device_name(0))), flush=True)

    def device_ms(run):
        """HIP events around run(), after one warm-up"""
        run()
        out = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def wall_ms(run):
        run()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            run()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e3)
        return out

    medians = {}

    def report(case, ms, **extra):
        s = summary(ms)
        medians[case] = s['median_ms']
        print(json.dumps(dict(extra, case=case, **s)), flush=True)

    report('acquire_events', device_ms(lambda: daq.acquire_events(gp, sim.rng_states, bounds, **kw)),
           clock='hip events')
    report('acquire_photoelectrons', device_ms(lambda: daq.acquire_photoelectrons(gp, sim.rng_states, bounds, **kw)),
           clock='hip events', record_bytes=12 * int(bounds[-1] - bounds[0]))
    # the native call alone, into arrays made once: without the Python method's three
    # allocations and its copy of the earliest-time words
    import ctypes
    from chroma.gpu import _native, gpuarray as ga
    from chroma.gpu.tools import current_stream
    span = int(bounds[-1] - bounds[0])
    rows4 = daq._event_arrays(nevents * nch)
    rec = [ga.empty(span, d) for d in (np.int32, np.float32, np.uint32)]
    desc = gp._desc()

    def native(name, extra):
        _native.call(name, ctypes.byref(desc), len(gp.pos), bounds.ctypes.data, nevents, sim.rng_states.gpudata,
                     len(sim.rng_states), 0x4, daq.solid_id_map_gpu.gpudata, ctypes.byref(daq._desc),
                     *([a.gpudata for a in rows4] + extra + [ctypes.c_float(1.0), int(sim.nthreads_per_block),
                                                             int(sim.max_blocks), current_stream()]))

    report('native_acquire_events', device_ms(lambda: native('chr_daq_acquire_events', [])), clock='hip events')
    report('native_acquire_events_pe',
           device_ms(lambda: native('chr_daq_acquire_events_pe', [a.gpudata for a in rec])), clock='hip events')
    chans, pe = daq.acquire_photoelectrons(gp, sim.rng_states, bounds, **kw)
    npe = int((pe.channel.get() >= 0).sum())
    for rows in ('hit', 'all'):
        report('trains_' + rows, device_ms(lambda: pe.trains(trange, args.samples, rows=rows)), clock='hip events')
        wf = pe.trains(trange, args.samples, rows=rows)
        report('digitise_' + rows, device_ms(lambda: wf.digitise(taps, scale, pedestal=100.0)), clock='hip events',
               rows=wf.nrows, train_bytes=4 * wf.nrows * args.samples, photoelectrons=npe,
               outside=int(wf.outside_q.get().astype(np.uint64).sum() > 0), dropped=wf.dropped)
        del wf

    def device_chain():
        _, p = daq.acquire_photoelectrons(gp, sim.rng_states, bounds, **kw)
        w = p.trains(trange, args.samples, rows='hit').digitise(taps, scale, pedestal=100.0)
        return w.trains.get(), w.adc.get()

    t_lo, inv = bin_scale(args.samples, trange)

    def host_route():
        hits = gp.get_flat_hits(sim.gpu_geometry)
        x = (hits.t - t_lo) * inv
        inside = (x >= 0) & (x < np.float32(args.samples))
        rows = hits.evidx[inside].astype(np.int64) * nch + hits.channel[inside]
        trains = np.zeros((nevents * nch, args.samples), np.uint32)
        np.add.at(trains, (rows, x[inside].astype(np.int64)), 1)
        return trains

    report('device_chain', wall_ms(device_chain), clock='host wall', rows='hit', download='trains and adc')
    report('host_route', wall_ms(host_route), clock='host wall', rows='all (dense numpy array)')
    print(json.dumps(dict(case='ratios',
                          pe_over_acquire_events=round(medians['acquire_photoelectrons']
                                                       / medians['acquire_events'], 3),
                          native_pe_over_native_acquire_events=round(medians['native_acquire_events_pe']
                                                                     / medians['native_acquire_events'], 3),
                          device_chain_over_host_route=round(medians['device_chain'] / medians['host_route'], 4))),
          flush=True)


if __name__ == '__main__':
    main()
