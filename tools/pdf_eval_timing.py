#!/usr/bin/env python3
"""Dev tool (GPU box): time one likelihood point, Simulation.eval_pdf, with the
DAQ of a source's photon copies taken copy by copy (pdf_rows = False: begin /
acquire / end / accumulate per copy, the native calls the per-event loop has
always made) and in groups of one native call each (pdf_rows = True:
GPUDaq.acquire_events_many and one accumulation over the stacked rows), in the
same process.

`sources` isotropic sources of `photons` photons each on the chosen detector
(bench.py's detectors and geometry cache: demo = 10,055 PMTs, small = 2 PMTs),
the observed event simulated from the first of them, ndaq DAQ copies, and for
every nreps (warm-up, then `repeats` times; median, min, max):

  wall    host clock around eval_pdf (propagation, DAQ, accumulation, the
          final download)
  device  HIP events around the same call, one extra pass
  daq     the DAQ and accumulation alone: one source propagated once, then
          host clock around Simulation._acquire_copy_rows over its copies,
          `sources` times

For pdf_rows = True every case is timed with groups of one copy taking the
batched call (pdf_rows_min_group = 1) and taking the per-copy loop (2).  The
RNG stream runs on from case to case, so the cases' hit totals are compared on
scale only (5 %); word equality from equal seeds is tests/test_gpu_pdf_eval.py's.
Prints one JSON line per case.

--trace-pass runs every case once and times nothing: the run to put under
`rocprofv3 --kernel-trace --stats`, whose kernel table gives the shares of
run_daq_events_many_kernel and run_daq_many_kernel in the DAQ part.

usage: tools/pdf_eval_timing.py [--detector demo] [--sources 100] [--photons 10000] [--ndaq 50]
                                [--nreps 1,4,16] [--repeats 3] [--group-mib 64] [--trace-pass]"""
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
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(ms.min()), 3),
                max_ms=round(float(ms.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--detector', default='demo', choices=('demo', '29k', 'small'))
    ap.add_argument('--sources', type=int, default=100)
    ap.add_argument('--photons', type=int, default=10000)
    ap.add_argument('--ndaq', type=int, default=50)
    ap.add_argument('--nreps', default='1,4,16')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--group-mib', type=int, default=0, help='daq_group_bytes in MiB (default: Simulation\'s)')
    ap.add_argument('--trace-pass', action='store_true', help='every case once, nothing timed (for rocprofv3)')
    args = ap.parse_args()
    import torch
    import bench
    from chroma import gpu
    from chroma.photon_source import isotropic
    from chroma.sim import Simulation, pdf_copy_groups
    assert torch.cuda.is_available(), 'pdf_eval_timing needs a HIP device'
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    det = bench.build_geometry(args.detector, bench.default_cache_dir())
    sim = Simulation(det, seed=1)
    nch = sim.gpu_daq.nchannels
    if args.group_mib:
        sim.daq_group_bytes = args.group_mib << 20
    sources = [isotropic(args.photons, seed=100 + i) for i in range(args.sources)]
    ev, = sim.simulate([sources[0]], run_daq=True, max_steps=100)
    channels = ev.channels
    print(json.dumps(dict(case='setup', detector=args.detector, nchannels=nch, sources=args.sources,
                          photons=args.photons, ndaq=args.ndaq, observed_hits=int(channels.hit.sum()),
                          setup_s=round(time.perf_counter() - t0, 1), device=torch.cuda.get_device_name(0))),
          flush=True)
    pdf_args = (0.2, (-0.5, 999.5), 1, (-0.5, 49.5))

    def point(nreps):
        return sim.eval_pdf(channels, iter(sources), *pdf_args, min_bin_content=320, nreps=nreps, ndaq=args.ndaq)

    for nreps in [int(x) for x in args.nreps.split(',')]:
        groups = pdf_copy_groups(nreps, args.ndaq, nch, sim.daq_group_bytes)
        counts = {}
        for rows, min_group in ((False, 2), (True, 1), (True, 2)):
            if rows and min_group == 2 and all(b - a >= 2 for a, b in groups):
                continue            # no group of one copy: the same calls as min_group = 1
            sim.pdf_rows, sim.pdf_rows_min_group = rows, min_group
            base = dict(case='eval_pdf', detector=args.detector, nreps=nreps, ndaq=args.ndaq, pdf_rows=rows,
                        min_group=min_group, group_mib=sim.daq_group_bytes >> 20,
                        groups=len(groups) * args.sources if rows else 0)
            if args.trace_pass:
                hitcount, _, _ = point(nreps)
                print(json.dumps(dict(base, hits=int(hitcount.sum()))), flush=True)
                continue
            point(nreps)                                   # warm-up
            wall = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t = time.perf_counter()
                hitcount, value, _ = point(nreps)
                wall.append((time.perf_counter() - t) * 1e3)
            counts[rows, min_group] = float(hitcount.sum())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            point(nreps)
            e1.record()
            torch.cuda.synchronize()
            device_ms = e0.elapsed_time(e1)
            # the DAQ and the accumulation alone, on one propagated source
            daq = sim._pdf_daq(args.ndaq)
            gp = gpu.GPUPhotons(sources[0], ncopies=nreps)
            gp.propagate(sim.gpu_geometry, sim.rng_states, nthreads_per_block=sim.nthreads_per_block,
                         max_blocks=sim.max_blocks, max_steps=100)
            acc = sim.gpu_pdf.accumulate_pdf_eval
            daq_ms = []
            for k in range(args.repeats + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(args.sources):
                    sim._acquire_copy_rows(daq, gp, args.photons, nreps, acc, acc)
                torch.cuda.synchronize()
                if k:
                    daq_ms.append((time.perf_counter() - t) * 1e3)
            print(json.dumps(dict(base, wall=summary(wall), device_ms=round(device_ms, 3), daq=summary(daq_ms),
                                  hits=int(hitcount.sum()), finite=bool(np.isfinite(value).all()))), flush=True)
        if counts:
            ref = next(iter(counts.values()))
            assert all(abs(h - ref) <= 0.05 * max(ref, 1.0) for h in counts.values()), counts
    sim.pdf_rows, sim.pdf_rows_min_group = Simulation.pdf_rows, Simulation.pdf_rows_min_group


if __name__ == '__main__':
    main()
