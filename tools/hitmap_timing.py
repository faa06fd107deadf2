#!/usr/bin/env python3
"""Dev tool (GPU box): time hit-map accumulation (chr_hitmap_accumulate through
GPUHitMap) alone and Simulation.hit_map end to end.  Prints one JSON line per
case; the records are kept under profiles/hitmap/.

  flash       one isotropic flash of --photons photons at the centre of the
              chosen detector (bench.py's detectors and geometry cache; 29k =
              the benchmark's 29,007 PMTs), generated and propagated once, then
              accumulated `repeats` times after a warm-up, for every path the
              row admits (CHR_HITMAP_PATH=d, l) and for the sweep that also adds
              empty words (CHR_HITMAP_SWEEP=a).
  synthetic   made records on a stand-in detector of --channels channels (each
              triangle its own solid and channel): --sources sources of
              --per-source consecutive photons, a fraction --detected of them
              detected on random channels; the same photons with evidx
              shuffled; both paths, a small row (counts + tmin) and a large one
              (16 time bins, tmin, wsum).
  end_to_end  --sources flashes of --per-source photons at random points of
              the detector's inner sphere through Simulation.hit_map, against
              the route without it for the same table: simulate(one Gensteps per
              source, keep_flat_hits=True, keep_hits=False) and np.add.at on each
              event's flat-hit channels.  Same seed, same detector; wall clock.

Device times are HIP events around `--calls` back-to-back accumulate calls,
divided by their number (the calls are asynchronous: launch gaps are inside the
span, which is why several are chained).  `bytes` is what the kernel must read:
12 B per photon (evidx, flags, last hit) + 8 B per detected one (its solid-map
entry and its time); `hbm_fraction` is bytes / time / 8 TB/s.

usage: tools/hitmap_timing.py [--cases flash,synthetic,end_to_end] [--detector 29k] [--photons 10000000]
                              [--sources 1000] [--per-source 10000] [--channels 300] [--repeats 20]"""
import argparse
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


def time_accumulate(hm, gp, repeats, calls):
    """ms per accumulate call (HIP events around `calls` chained calls), over `repeats` after a warm-up"""
    import torch
    hm.accumulate(gp)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            hm.accumulate(gp)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def accumulate_cases(label, gdet, gp, nsources, detected, variants, args, extra):
    from chroma import gpu
    n = len(gp)
    nbytes = 12 * n + 8 * detected
    for name, opt in variants:
        for path, sweep in (('d', None), ('l', None), ('l', 'a')):
            os.environ['CHR_HITMAP_PATH'] = path
            if sweep:
                os.environ['CHR_HITMAP_SWEEP'] = sweep
            else:
                os.environ.pop('CHR_HITMAP_SWEEP', None)
            hm = gpu.GPUHitMap(gdet, nsources, **opt)
            fits = hm.row_words <= gpu.hitmap.LDS_WORDS
            if path == 'l' and not fits:
                continue                       # falls back to d: timed above
            ms = time_accumulate(hm, gp, args.repeats, args.calls)
            took = 'privatised' if hm.last_path == gpu.hitmap.PRIVATISED else 'direct'
            med = float(np.median(ms))
            print(json.dumps(dict(extra, case=label, rows=name, row_words=hm.row_words, path=took,
                                  sweep='all' if sweep else 'nonempty', photons=n, detected=detected, bytes=nbytes,
                                  per_call=summary(ms), gbytes_per_s=round(nbytes / med / 1e6, 1),
                                  hbm_fraction=round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4))), flush=True)
    os.environ.pop('CHR_HITMAP_PATH', None)
    os.environ.pop('CHR_HITMAP_SWEEP', None)


def detected_of(gp, gdet):
    fl, last = gp.flags.get(), gp.last_hit_triangles.get()
    sel = ((fl & 4) != 0) & (last > -1)
    ch = gdet.solid_id_to_channel_index_gpu.get()[gdet.solid_id_map.get()[last[sel]]]
    return int(((ch >= 0) & (ch < gdet.nchannels)).sum())


def case_flash(sim, args):
    from chroma import gensteps as gs, gpu
    water = [m for m in sim.gpu_geometry.packed.material_objects if getattr(m, 'name', None) == 'water'][0]
    t0 = time.perf_counter()
    made = gpu.generate_photons(gs.isotropic_flash(water, args.photons, evidx=0), sim.gpu_geometry, sim.rng_states)
    gpu.propagate_batches([made], sim.gpu_geometry, sim.rng_states, nthreads_per_block=sim.nthreads_per_block,
                          max_blocks=sim.max_blocks, max_steps=1000)
    import torch
    torch.cuda.synchronize()
    extra = dict(detector=args.detector, nchannels=int(sim.gpu_geometry.nchannels), sources=1,
                 generate_propagate_s=round(time.perf_counter() - t0, 3))
    variants = (('counts', dict(earliest=False)), ('counts+tmin', dict(earliest=True)),
                ('counts+tmin+16bins+wsum', dict(tbins=16, trange=(0.0, 400.0), earliest=True, weights=True)))
    accumulate_cases('flash', sim.gpu_geometry, made, 1, detected_of(made, sim.gpu_geometry), variants, args, extra)


def case_synthetic(args):
    from chroma import gpu
    from chroma.event import Photons
    from chroma.gpu import gpuarray as ga
    nch, n = args.channels, args.sources * args.per_source
    r = np.random.RandomState(5)
    gdet = SimpleNamespace(solid_id_map=ga.to_gpu(np.arange(nch, dtype=np.uint32)),
                           solid_id_to_channel_index_gpu=ga.to_gpu(r.permutation(nch).astype(np.int32)),
                           nchannels=nch)
    hit = r.uniform(size=n) < args.detected
    last = np.where(hit, r.randint(0, nch, n), -1).astype(np.int32)
    flags = np.where(hit, 4, 2).astype(np.uint32)
    evidx = np.repeat(np.arange(args.sources, dtype=np.uint32), args.per_source)
    zeros = np.zeros((n, 3), np.float32)
    variants = (('counts+tmin', dict(earliest=True)),
                ('counts+tmin+16bins+wsum', dict(tbins=16, trange=(0.0, 100.0), earliest=True, weights=True)))
    for order in ('by_source', 'shuffled'):
        if order == 'shuffled':
            evidx = evidx[r.permutation(n)]
        ph = Photons(zeros, zeros, zeros, np.full(n, 400.0, np.float32), t=r.uniform(0.0, 100.0, n).astype(np.float32),
                     last_hit_triangles=last, flags=flags, weights=np.ones(n, np.float32), evidx=evidx)
        gp = gpu.GPUPhotons(ph, copy_flags=True, copy_triangles=True, copy_weights=True)
        accumulate_cases('synthetic', gdet, gp, args.sources, int(hit.sum()), variants, args,
                         dict(nchannels=nch, sources=args.sources, per_source=args.per_source, order=order))


def case_end_to_end(sim, det, args):
    import torch
    from chroma import gensteps as gs
    water = [m for m in sim.gpu_geometry.packed.material_objects if getattr(m, 'name', None) == 'water'][0]
    r = np.random.RandomState(9)
    import bench
    radius = 0.5 * bench.DETECTORS[args.detector][1].get('pmt_radius', 14000.0)     # well inside the PMT sphere
    spots = r.uniform(-1, 1, (args.sources, 3)) * radius / np.sqrt(3.0)
    steps = [gs.isotropic_flash(water, args.per_source, x0=tuple(x), evidx=i) for i, x in enumerate(spots)]
    nch = int(sim.gpu_geometry.nchannels)
    kw = dict(nthreads_per_block=sim.nthreads_per_block, max_blocks=sim.max_blocks)

    def new_route(s):
        return s.hit_map(steps, args.sources, earliest=True, max_steps=1000).counts

    def old_route(s):
        counts = np.zeros((args.sources, nch), np.uint32)
        for i, ev in enumerate(s.simulate(steps, keep_flat_hits=True, keep_hits=False, max_steps=1000)):
            np.add.at(counts[i], ev.flat_hits.channel, 1)
        return counts

    from chroma import gpu
    from chroma.sim import hit_map_batches
    nslots = len(sim.rng_states)
    results = {}
    for name, route in (('hit_map', new_route), ('simulate', old_route)):
        wall = []
        for k in range(args.e2e_repeats + 1):                      # the first pass is the warm-up
            sim.rng_states = gpu.get_rng_states(nslots, seed=3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            counts = route(sim)
            torch.cuda.synchronize()
            if k:
                wall.append((time.perf_counter() - t) * 1e3)
        results[name] = (float(np.median(wall)), counts)
        print(json.dumps(dict(case='end_to_end', route=name, detector=args.detector, nchannels=nch,
                              sources=args.sources, per_source=args.per_source, wall=summary(wall),
                              detected=int(counts.sum()))), flush=True)
    # the two routes draw in different orders (one generate call per batch against one per source), so
    # their tables agree statistically, not word for word
    print(json.dumps(dict(case='end_to_end', route='ratio', simulate_over_hit_map=round(
        results['simulate'][0] / results['hit_map'][0], 2))), flush=True)
    # the parts of the new route on its first batch: generate + propagate (wall) and accumulate (device)
    sim.rng_states = gpu.get_rng_states(nslots, seed=3)
    records = np.concatenate([g.records(sim.gpu_geometry.packed.material_objects) for g in steps])
    a, b = hit_map_batches(records['nphotons'], 1000000)[0]
    torch.cuda.synchronize()
    t = time.perf_counter()
    made = gpu.generate_photons(records[a:b], sim.gpu_geometry, sim.rng_states)
    gpu.propagate_batches([made], sim.gpu_geometry, sim.rng_states, max_steps=1000, **kw)
    torch.cuda.synchronize()
    gen_prop_ms = (time.perf_counter() - t) * 1e3
    hm = gpu.GPUHitMap(sim.gpu_geometry, args.sources, earliest=True)
    ms = time_accumulate(hm, made, args.repeats, args.calls)
    print(json.dumps(dict(case='end_to_end', route='parts_of_one_batch', batch_photons=len(made),
                          batches=-(-args.sources * args.per_source // len(made)),
                          generate_propagate_ms=round(gen_prop_ms, 3), accumulate=summary(ms),
                          path='privatised' if hm.last_path == gpu.hitmap.PRIVATISED else 'direct')), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='flash,synthetic,end_to_end')
    ap.add_argument('--detector', default='29k', choices=('29k', 'demo', 'tiny', 'small'))
    ap.add_argument('--photons', type=int, default=10000000)
    ap.add_argument('--sources', type=int, default=1000)
    ap.add_argument('--per-source', type=int, default=10000)
    ap.add_argument('--channels', type=int, default=300)
    ap.add_argument('--detected', type=float, default=0.1, help='synthetic: fraction of photons detected')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--e2e-repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=10, help='accumulate calls chained between two HIP events')
    args = ap.parse_args()
    import torch
    import bench
    from chroma.sim import Simulation
    assert torch.cuda.is_available(), 'hitmap_timing needs a HIP device'
    torch.cuda.set_device(0)
    cases = args.cases.split(',')
    sim = det = None
    if 'flash' in cases or 'end_to_end' in cases:
        t0 = time.perf_counter()
        det = bench.build_geometry(args.detector, bench.default_cache_dir())
        sim = Simulation(det, seed=1)
        print(json.dumps(dict(case='setup', detector=args.detector, nchannels=int(sim.gpu_geometry.nchannels),
                              setup_s=round(time.perf_counter() - t0, 1), device=torch.cuda.get_device_name(0))),
              flush=True)
    else:
        from chroma.gpu import create_cuda_context
        create_cuda_context()
    if 'flash' in cases:
        case_flash(sim, args)
    if 'synthetic' in cases:
        case_synthetic(args)
    if 'end_to_end' in cases:
        case_end_to_end(sim, det, args)


if __name__ == '__main__':
    main()
