#!/usr/bin/env python3
"""Dev tool (GPU box): time the photon-library lookup (chr_library_expect and
chr_library_sample through GPUPhotonLibrary's arrays) and Simulation.simulate_library
end to end.  Prints one JSON line per case; the records are kept under
profiles/library/.

  lookup      a made library of --sources sources holding counts and tmin, for every
              channel count of --channels (29007 = the benchmark detector's PMTs), and
              --events events of --entries entries on random sources.  Timed: expect on
              every path the shape admits, sample with --slots generator states, and
              the route a user has without the kernel: the same mu on the device with
              torch (index_select of the rows, cast to float32, weighted sum; its
              result agrees to rounding, not bit for bit).
  end_to_end  on the chosen detector (bench.py's detectors and geometry cache): a
              library of a --grid^3 voxel grid built with Simulation.build_library,
              then --e2e-events events of --e2e-steps isotropic steps through
              simulate_library (sampled) against Simulation.simulate(run_daq=True) on
              the same gensteps.  Wall clock.

Device times are HIP events around one call, after a warm-up, over --repeats repeats;
the median, minimum and maximum are reported.  `bytes` is what the expect kernel must
read, entries x nchannels x 4 B x (1 + [tmin]); `hbm_fraction` is bytes / time / 8 TB/s.

usage: tools/library_timing.py [--cases lookup,end_to_end] [--channels 29007,300] [--sources 1000]
                               [--events 64] [--entries 256] [--repeats 20] [--detector 29k]"""
import argparse
import ctypes
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def summary(ms):
    ms = np.asarray(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4),
                max_ms=round(float(ms.max()), 4))


def timed(fn, repeats):
    """ms per call of fn (HIP events), over `repeats` after a warm-up"""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def case_lookup(args, nch):
    import torch
    from chroma import gpu
    from chroma.gpu import _native, gpuarray as ga
    from chroma.gpu.tools import current_stream
    from chroma.library import LibraryEntries
    r = np.random.RandomState(7)
    ns, nev, per = args.sources, args.events, args.entries
    counts = r.randint(0, 30, ns * nch).astype(np.uint32)
    times = r.uniform(5.0, 200.0, ns * nch).astype(np.float32)
    made = SimpleNamespace(nsources=ns, nchannels=nch, tbins=0, t_lo=np.float32(0), inv=np.float32(0),
                           emitted=ga.to_gpu(np.full(ns, 100000, np.uint64)), counts=ga.to_gpu(counts),
                           tmin=ga.to_gpu(times.view(np.uint32) ^ np.uint32(0x80000000)), thist=None)
    lib = gpu.GPUPhotonLibrary(made)
    en = LibraryEntries(np.arange(nev + 1) * per, r.randint(0, ns, nev * per), r.randint(1, 5000, nev * per),
                        r.uniform(0.0, 10.0, nev * per))
    keep, desc = lib._upload_entries(en)
    mu, tfirst = ga.empty(nev * nch, np.float32), ga.empty(nev * nch, np.float32)
    n_out, t_out = ga.empty(nev * nch, np.uint32), ga.empty(nev * nch, np.float32)
    skipped = ga.zeros(1, np.uint64)
    rng = gpu.get_rng_states(args.slots, seed=1)
    nbytes = nev * per * nch * 4 * 2
    base = dict(case='lookup', nchannels=nch, sources=ns, events=nev, entries_per_event=per, bytes=nbytes)

    def expect():
        _native.call('chr_library_expect', ctypes.byref(lib._desc()), ctypes.byref(desc), mu.gpudata, tfirst.gpudata,
                     skipped.gpudata, current_stream())

    def sample():
        _native.call('chr_library_sample', ctypes.byref(lib._desc()), ctypes.byref(desc), rng.gpudata, rng.size,
                     n_out.gpudata, t_out.gpudata, skipped.gpudata, current_stream())

    results = {}
    for forced in ((None, 'n') if nch % 4 == 0 else (None,)):
        if forced:
            os.environ['CHR_LIBRARY_PATH'] = forced
        ms = timed(expect, args.repeats)
        os.environ.pop('CHR_LIBRARY_PATH', None)
        path = 'wide' if _native.lib().chr_library_last_path() == 1 else 'narrow'
        med = float(np.median(ms))
        results[path] = med
        print(json.dumps(dict(base, what='expect', path=path, per_call=summary(ms),
                              gbytes_per_s=round(nbytes / med / 1e6, 1),
                              hbm_fraction=round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4))), flush=True)
    ours = mu.get()

    # the route without the kernel: gather, cast, weight, sum (mu only: no earliest time)
    src = torch.from_numpy(en.source.astype(np.int64)).cuda()
    w = torch.from_numpy((en.nphotons.astype(np.float32) / np.float32(100000))).cuda()
    table = lib.counts.tensor.view(ns, nch)

    def torch_route():
        rows = table.index_select(0, src).to(torch.float32)
        return (rows * w[:, None]).view(nev, per, nch).sum(dim=1)

    ms = timed(torch_route, args.repeats)
    theirs = torch_route().cpu().numpy().reshape(-1)
    print(json.dumps(dict(base, what='torch_index_select_mu', per_call=summary(ms),
                          max_rel_diff_to_expect=float(np.max(np.abs(theirs - ours) / np.maximum(ours, 1e-30))),
                          over_expect=round(float(np.median(ms)) / min(results.values()), 2))), flush=True)
    ms = timed(sample, args.repeats)
    print(json.dumps(dict(base, what='sample', slots=args.slots, per_call=summary(ms),
                          hits=int((n_out.get() > 0).sum()))), flush=True)
    del keep


def case_end_to_end(args):
    import torch
    import bench
    from chroma import gensteps as gs, gpu
    from chroma.library import VoxelGrid
    from chroma.sim import Simulation
    t0 = time.perf_counter()
    det = bench.build_geometry(args.detector, bench.default_cache_dir())
    sim = Simulation(det, seed=1)
    nch = int(sim.gpu_geometry.nchannels)
    water = [m for m in sim.gpu_geometry.packed.material_objects if getattr(m, 'name', None) == 'water'][0]
    half = 0.5 * bench.DETECTORS[args.detector][1].get('pmt_radius', 14000.0) / np.sqrt(3.0)
    grid = VoxelGrid((-half,) * 3, (half,) * 3, (args.grid,) * 3)
    print(json.dumps(dict(case='setup', detector=args.detector, nchannels=nch, setup_s=round(time.perf_counter() - t0, 1),
                          device=torch.cuda.get_device_name(0))), flush=True)
    t0 = time.perf_counter()
    lib = sim.build_library(grid, water, args.per_voxel, tbins=args.tbins, trange=(0.0, 400.0))
    torch.cuda.synchronize()
    print(json.dumps(dict(case='end_to_end', what='build_library', voxels=grid.nvoxels, per_voxel=args.per_voxel,
                          tbins=args.tbins, wall_s=round(time.perf_counter() - t0, 2))), flush=True)
    r = np.random.RandomState(11)
    events = []
    for _ in range(args.e2e_events):
        spots = r.uniform(-half, half, (args.e2e_steps, 3))
        events.append(gs.Gensteps.join([gs.isotropic_flash(water, args.e2e_photons, x0=tuple(x), t0=float(i))
                                        for i, x in enumerate(spots)]))
    nslots = len(sim.rng_states)
    results = {}
    routes = (('simulate_library', lambda: [ev.channels.hit.sum() for ev in sim.simulate_library(lib, events)]),
              ('simulate_run_daq', lambda: [ev.channels.hit.sum() for ev in
                                            sim.simulate(events, run_daq=True, keep_hits=False, keep_flat_hits=False)]))
    for name, route in routes:
        wall = []
        for k in range(args.e2e_repeats + 1):                      # the first pass is the warm-up
            sim.rng_states = gpu.get_rng_states(nslots, seed=3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            hits = route()
            torch.cuda.synchronize()
            if k:
                wall.append((time.perf_counter() - t) * 1e3)
        results[name] = float(np.median(wall))
        print(json.dumps(dict(case='end_to_end', route=name, detector=args.detector, nchannels=nch,
                              events=args.e2e_events, steps=args.e2e_steps, photons_per_step=args.e2e_photons,
                              wall=summary(wall), hit_channels=int(np.sum(hits)))), flush=True)
    print(json.dumps(dict(case='end_to_end', route='ratio', simulate_over_simulate_library=round(
        results['simulate_run_daq'] / results['simulate_library'], 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='lookup,end_to_end')
    ap.add_argument('--channels', default='29007,300')
    ap.add_argument('--sources', type=int, default=1000)
    ap.add_argument('--events', type=int, default=64)
    ap.add_argument('--entries', type=int, default=256)
    ap.add_argument('--slots', type=int, default=524288)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--detector', default='29k', choices=('29k', 'demo', 'tiny', 'small'))
    ap.add_argument('--grid', type=int, default=4)
    ap.add_argument('--per-voxel', type=int, default=100000)
    ap.add_argument('--tbins', type=int, default=0)
    ap.add_argument('--e2e-events', type=int, default=16)
    ap.add_argument('--e2e-steps', type=int, default=32)
    ap.add_argument('--e2e-photons', type=int, default=2000)
    ap.add_argument('--e2e-repeats', type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'library_timing needs a HIP device'
    torch.cuda.set_device(0)
    cases = args.cases.split(',')
    if 'lookup' in cases:
        from chroma.gpu import create_cuda_context
        create_cuda_context()
        for nch in [int(x) for x in args.channels.split(',')]:
            case_lookup(args, nch)
    if 'end_to_end' in cases:
        case_end_to_end(args)


if __name__ == '__main__':
    main()
