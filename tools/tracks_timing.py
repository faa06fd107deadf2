#!/usr/bin/env python3
"""Dev tool (GPU box): time photon tracking through the host-driven loop
(GPUPhotons.device_tracking cleared: one chunk launch, nine gathers and ten
downloads per step, then per-record Python in Simulation._emit) and through the
tracks recorded on the device (device_tracking set: chr_propagate_tracked, one
download), in the same process, on bench.py's demo detector (10,055 PMTs) with
the simulation's 512 x 1024 RNG slots and max_steps = 100.

  propagate   GPUPhotons.propagate(track=True) of N isotropic photons: wall
              time to the returned (step_photon_ids, step_photons) and the HIP
              event span around the call (host gaps between its synchronous
              parts included); the upload is not timed
  simulate    Simulation(photon_tracking=True).simulate of N photons in 10
              events: wall time to the last yielded event with photon_tracks
              built, and (device path) with only photon_tracks_flat read
              (Simulation.photon_track_lists cleared)

Every case: one warm-up, then `repeats` passes (median, min, max).  The device
path also reports the records, the entries and the bytes the handle holds.
Prints one JSON line per case.

usage: tools/tracks_timing.py [--detector demo] [--propagate 10000,100000,1000000]
                              [--simulate 10000,100000] [--repeats 10] [--paths host,device]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))
sys.path.insert(0, ROOT)

NTPB, MAX_BLOCKS, MAX_STEPS = 512, 1024, 100


def summary(ms):
    ms = np.asarray(ms)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(ms.min()), 3),
                max_ms=round(float(ms.max()), 3))


def sizes(text):
    return [int(x) for x in text.split(',') if x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--detector', default='demo', choices=('demo', '29k', 'small'))
    ap.add_argument('--propagate', default='10000,100000,1000000')
    ap.add_argument('--simulate', default='10000,100000')
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--paths', default='host,device')
    args = ap.parse_args()
    import torch
    import bench
    from chroma import gpu
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation
    assert torch.cuda.is_available(), 'tracks_timing needs a HIP device'
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    det = bench.build_geometry(args.detector, bench.default_cache_dir())
    sim = Simulation(det, seed=1, photon_tracking=True, nthreads_per_block=NTPB, max_blocks=MAX_BLOCKS)
    gg = sim.gpu_geometry
    print(json.dumps(dict(case='setup', detector=args.detector, rng_slots=len(sim.rng_states), max_steps=MAX_STEPS,
                          setup_s=round(time.perf_counter() - t0, 1), device=torch.cuda.get_device_name(0))),
          flush=True)
    paths = [p for p in args.paths.split(',') if p]

    def timed(run, repeats):
        """run() -> info dict: wall and HIP-event span over `repeats` passes after one warm-up"""
        run()
        wall, dev, info = [], [], None
        for _ in range(repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            info = run(e1)
            wall.append((time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1))
        return wall, dev, info

    for n in sizes(args.propagate):
        photons = isotropic(n, seed=1)
        results = {}
        for path in paths:
            gpu.GPUPhotons.device_tracking = path == 'device'

            def run(done=None):
                rng = gpu.get_rng_states(NTPB * MAX_BLOCKS, seed=1)      # the same draws every pass
                gp = gpu.GPUPhotons(photons)
                torch.cuda.synchronize()
                t = time.perf_counter()
                ids, steps = gp.propagate(gg, rng, nthreads_per_block=NTPB, max_blocks=MAX_BLOCKS,
                                          max_steps=MAX_STEPS, track=True)
                if done is not None:
                    done.record()
                return dict(entries=len(ids), records=int(sum(len(q) for q in ids)),
                            call_ms=(time.perf_counter() - t) * 1e3, flags_sum=int(gp.flags.get().sum(dtype=np.uint64)))

            # the pass's wall clock is the call alone (run() also makes the states and uploads the photons)
            run()
            wall, info = [], None
            for _ in range(args.repeats):
                info = run()
                wall.append(info['call_ms'])
            results[path] = info
            line = dict(case='propagate', path=path, photons=n, entries=info['entries'], records=info['records'],
                        wall=summary(wall), flags_sum=info['flags_sum'])
            # HIP-event span of the call: passes of its own, events on the stream either side of it
            spans = []
            for _ in range(3):
                gp = gpu.GPUPhotons(photons)
                rng = gpu.get_rng_states(NTPB * MAX_BLOCKS, seed=1)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gp.propagate(gg, rng, nthreads_per_block=NTPB, max_blocks=MAX_BLOCKS, max_steps=MAX_STEPS, track=True)
                e1.record()
                torch.cuda.synchronize()
                spans.append(e0.elapsed_time(e1))
            line['device_span_ms'] = round(float(np.median(spans)), 3)
            if path == 'device':      # what the handle holds, and the driver's own kernel time
                gp = gpu.GPUPhotons(photons)
                rng = gpu.get_rng_states(NTPB * MAX_BLOCKS, seed=1)
                with gp.propagate_tracks(gg, rng, nthreads_per_block=NTPB, max_blocks=MAX_BLOCKS,
                                         max_steps=MAX_STEPS) as tr:
                    st = tr.last_stats
                    line.update(step_counts=tr.step_counts.tolist(), host_syncs=int(st.host_syncs),
                                steps_run=int(st.steps_run), step_kernels_ms=round(float(st.kernel_ms), 3),
                                records_bytes=int(tr.nrecords) * 64,
                                held_bytes_max=int(tr.nrecords) * 64 * 3 + 8 * (n + 1 + tr.nentries + 1))
            print(json.dumps(line), flush=True)
        if len(results) == 2:
            a, b = results['host'], results['device']
            assert (a['entries'], a['records'], a['flags_sum']) == (b['entries'], b['records'], b['flags_sum']), (a, b)

    for n in sizes(args.simulate):
        events = [isotropic(n // 10, seed=100 + e) for e in range(10)]
        cases = [(p, True) for p in paths] + ([('device', False)] if 'device' in paths else [])
        for path, lists in cases:
            gpu.GPUPhotons.device_tracking = path == 'device'
            sim.photon_track_lists = lists

            def run(done=None):
                nrec = ntracks = 0
                for ev in sim.simulate(events, keep_photons_end=False, keep_hits=False, keep_flat_hits=False,
                                       max_steps=MAX_STEPS):
                    if ev.photon_tracks is not None:
                        ntracks += len(ev.photon_tracks)
                    if ev.photon_tracks_flat is not None:
                        nrec += len(ev.photon_tracks_flat[1])
                if done is not None:
                    done.record()
                return dict(tracks=ntracks, flat_records=nrec)

            wall, dev, info = timed(run, args.repeats)
            print(json.dumps(dict(case='simulate', path=path, photon_tracks=lists, photons=n, events=10,
                                  wall=summary(wall), **info)), flush=True)
        sim.photon_track_lists = True
    gpu.GPUPhotons.device_tracking = True


if __name__ == '__main__':
    main()
