#!/usr/bin/env python3
"""Dev tool (GPU box): time the DAQ of one propagated batch, split into E equal
events, through the per-event loop (Simulation._acquire: begin / acquire / end
and three downloads per event, the reference's sim.py:143-152) and through
GPUDaq.acquire_events in groups (Simulation._acquire_events under
daq_group_bytes), in the same process.

1 M isotropic photons are propagated once on the chosen detector (bench.py's
detectors and geometry cache: demo = 10,055 PMTs, 29k = 29,007 PMTs, small =
2 PMTs) with the simulation's 524,288 RNG slots.  For every E the DAQ of that
batch is repeated (warm-up, then `repeats` times; median, min, max):

  wall    host clock from the first native call to the last event's host
          Channels (downloads and the per-event row copies included)
  device  HIP events around the native calls: for the batched path the span of
          one chr_daq_acquire_events (fill, bounds copy, kernels, convert),
          summed over the groups; for the loop the span from chr_daq_begin to
          chr_daq_end of every event (their host gaps between the synchronous
          calls included), summed over the events; one extra pass each

The batched path is timed for daq_group_bytes of 16, 64 and 256 MiB and for
both kernel shapes (CHR_DAQ_EVENTS_SHAPE=b: candidate pass + draw pass, the
default; a: one kernel reading candidates one event ahead).  Prints one JSON
line per case.

usage: tools/daq_events_timing.py [--detector demo] [--photons 1000000] [--repeats 10]
                                  [--events 1,10,100,1000,10000] [--loop-max-events 10000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))
sys.path.insert(0, ROOT)

MIB = 1 << 20


def summary(ms):
    ms = np.asarray(ms)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(ms.min()), 3),
                max_ms=round(float(ms.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--detector', default='demo', choices=('demo', '29k', 'small'))
    ap.add_argument('--photons', type=int, default=1000000)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--events', default='1,10,100,1000,10000')
    ap.add_argument('--loop-max-events', type=int, default=10000,
                    help='skip the per-event loop above this many events (a short run)')
    ap.add_argument('--budgets', default='16,64,256', help='daq_group_bytes to time, MiB')
    args = ap.parse_args()
    import torch
    import bench
    from chroma import event
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation, daq_event_groups
    assert torch.cuda.is_available(), 'daq_events_timing needs a HIP device'
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    det = bench.build_geometry(args.detector, bench.default_cache_dir())
    sim = Simulation(det, seed=1)
    nch = sim.gpu_daq.nchannels
    n = args.photons
    b = sim._upload([event.Event(photons_beg=isotropic(n, seed=1))])
    sim._propagate([b], 100)
    torch.cuda.synchronize()
    detected = int(((b.gpu_photons.flags.get() & 4) != 0).sum())
    print(json.dumps(dict(case='setup', detector=args.detector, nchannels=nch, photons=n, detected=detected,
                          rng_slots=len(sim.rng_states), setup_s=round(time.perf_counter() - t0, 1),
                          device=torch.cuda.get_device_name(0))), flush=True)

    def timed(run, repeats):
        """run() -> (channels, device_ms): wall over `repeats` passes after one warm-up, device from one more"""
        run(False)
        wall = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            chans, _ = run(False)
            wall.append((time.perf_counter() - t) * 1e3)
        chans, dev = run(True)
        return chans, wall, dev

    for nevents in [int(x) for x in args.events.split(',')]:
        bounds = np.linspace(0, n, nevents + 1).astype(np.int64)
        b.bounds = bounds

        def loop(device):
            out, spans = [], []
            for start, end in zip(bounds[:-1], bounds[1:]):
                if device:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    sim.gpu_daq.begin_acquire()
                    sim.gpu_daq.acquire(b.gpu_photons, sim.rng_states, start_photon=int(start),
                                        nphotons=int(end - start), nthreads_per_block=sim.nthreads_per_block,
                                        max_blocks=sim.max_blocks)
                    ch = sim.gpu_daq.end_acquire()
                    e1.record()
                    out.append(ch.get())
                    spans.append((e0, e1))
                else:
                    out.append(sim._acquire(b, start, end))
            torch.cuda.synchronize()
            return out, sum(a.elapsed_time(z) for a, z in spans)

        def batched(budget):
            def run(device):
                out, spans = [], []
                for first, last in daq_event_groups(bounds, nch, budget):
                    if device:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        chans = sim.gpu_daq.acquire_events(b.gpu_photons, sim.rng_states, bounds[first:last + 1],
                                                           nthreads_per_block=sim.nthreads_per_block,
                                                           max_blocks=sim.max_blocks)
                        e1.record()
                        out += chans.get()
                        spans.append((e0, e1))
                    else:
                        out += sim._acquire_events(b, bounds[first:last + 1])
                torch.cuda.synchronize()
                return out, sum(a.elapsed_time(z) for a, z in spans)
            return run

        base = dict(events=nevents, photons_per_event=n // nevents, nchannels=nch)
        if nevents <= args.loop_max_events:
            chans, wall, dev = timed(loop, args.repeats)
            print(json.dumps(dict(base, case='loop', wall=summary(wall), device_ms=round(dev, 3),
                                  hit_channels=int(sum(c.hit.sum() for c in chans)))), flush=True)
        for shape in ('b', 'a'):
            os.environ['CHR_DAQ_EVENTS_SHAPE'] = shape
            for mib in [int(x) for x in args.budgets.split(',')]:
                if shape == 'a' and mib != 64:
                    continue
                groups = daq_event_groups(bounds, nch, mib * MIB)
                chans, wall, dev = timed(batched(mib * MIB), args.repeats)
                print(json.dumps(dict(base, case='acquire_events', shape=shape, group_mib=mib, groups=len(groups),
                                      wall=summary(wall), device_ms=round(dev, 3),
                                      hit_channels=int(sum(c.hit.sum() for c in chans)))), flush=True)
        os.environ.pop('CHR_DAQ_EVENTS_SHAPE', None)


if __name__ == '__main__':
    main()
